"""Pure-Python statement of include/snappier_hip_frame_verify.h (snp_frame_verify_indexed_batch, snp_frame_repair_plan_batch), written from
the header's text on top of oracle (the frame decoder: the status of one chunk is what it gives the identifier plus that chunk),
frame_buffers_model.hop (one header), frame_index_model.row_end and frame_rechunk_model.begin / rows_of (the index and its clamps): the
verdict of every stream over an untrusted index, the status of every row, what the rows of a stream add up to, the rounds, d_result; and the
planner: what admits a pair, the segments of its rows, the in-order admission by max_segs.  The CPU and the GPU tests share it."""
import struct

import frame_buffers_model as M
import frame_index_model as X
import frame_rechunk_model as RC
import oracle as O

U64 = (1 << 64) - 1
NONE = U64                      # SNP_VERIFY_NONE
SKIPPED = -1                    # SNP_VERIFY_SKIPPED
MAX_ROWS = (1 << 31) - 1
MAX_SLOT = 65536
NO_IDENT = 1


def nentries_of(ix) -> int:
    return min(len(ix["start"]), len(ix["pos"]))


# ---- rounds ------------------------------------------------------------------------------------------------------------------------------------------
def rounds_of(slot_bytes: int, scratch_cap: int, ne: int):
    """-> (stride, rows per round, rounds)."""
    stride = (slot_bytes + 15) // 16 * 16
    per = min(scratch_cap // stride, ne)
    return stride, per, (ne + per - 1) // per if per else 0


# ---- one chunk -----------------------------------------------------------------------------------------------------------------------------------------
def chunk_status(chunk: bytes) -> int:
    """What the oracle's frame decoder gives the identifier plus this one chunk."""
    try:
        O.frame_decode(M.STREAM_ID + chunk)
        return O.OK
    except O.OracleError as e:
        return e.status


# ---- the verify ------------------------------------------------------------------------------------------------------------------------------------------
def verify_plan(streams, ix, slot_bytes: int = MAX_SLOT, scratch_cap: int = 1 << 40, status_of=chunk_status):
    """snp_frame_verify_indexed_batch: -> dict of row_status, status, nbad, first_bad, bad_bytes, flags, result [8].  status_of(chunk): what
    the decode and CRC verify give one checked chunk."""
    ns, ne = len(streams), nentries_of(ix)
    assert ne <= MAX_ROWS and 1 <= slot_bytes <= MAX_SLOT
    _, per, rounds = rounds_of(slot_bytes, scratch_cap, ne)
    row_status = [SKIPPED] * ne
    status, nbad, first_bad, bad_bytes, flags = [], [], [], [], []
    looked = notok = okbytes = longest = unverified = 0
    before = 0
    for b, s in enumerate(streams):
        flags.append(0 if s[:10] == M.STREAM_ID else NO_IDENT)
        st = RC.begin(ix, b)
        f0, n = RC.rows_of(ix, b)
        if st == O.OK and f0 < before:
            st = O.ERR_BAD_ARG
        before = max(before, min(ix["first"][b], ne))
        if st != O.OK:
            status.append(st)
            nbad.append(0)
            first_bad.append(NONE)
            bad_bytes.append(0)
            continue
        f1, total = f0 + n, ix["total"][b]
        bad = bb = 0
        first = NONE
        for i in range(f0, f1):
            a, e, pos = ix["start"][i], X.row_end(ix, f1, total, i), ix["pos"][i]
            ln = e - a if e >= a else 0
            checked = False
            if e < a or pos >= len(s):
                rs = O.ERR_BAD_ARG
            else:
                h = M.hop(s, pos)
                if h.kind != "data" or e - a != h.dec or (i + 1 < f1 and ix["pos"][i + 1] < h.next):
                    rs = O.ERR_BAD_ARG
                else:
                    checked = True
                    longest = max(longest, ln)
                    rs = O.ERR_OUTPUT_TOO_SMALL if ln > slot_bytes or per == 0 else status_of(s[pos:h.next])
            row_status[i] = rs
            looked += 1
            if rs == O.OK:
                okbytes += ln
                continue
            bad, bb = bad + 1, (bb + ln) & U64
            first = min(first, i)
            if checked and rs == O.ERR_OUTPUT_TOO_SMALL:
                unverified += 1
        status.append(row_status[first] if first != NONE else O.OK)
        nbad.append(bad)
        first_bad.append(first)
        bad_bytes.append(bb)
        notok += bad
    result = [looked, notok, okbytes & U64, sum(1 for v in status if v == O.OK), longest, unverified, rounds, sum(bad_bytes) & U64]
    return dict(row_status=row_status, status=status, nbad=nbad, first_bad=first_bad, bad_bytes=bad_bytes, flags=flags, result=result)


# ---- the planner -------------------------------------------------------------------------------------------------------------------------------------------
def pair_status(ix, ns: int, rep_total, rep_tail, s: int, t: int) -> int:
    """rp_begin."""
    if s >= ns or t >= len(rep_total):
        return O.ERR_BAD_ARG
    if RC.begin(ix, s) != O.OK or rep_tail[t] != O.OK:
        return O.ERR_BAD_ARG
    return O.OK if rep_total[t] == ix["total"][s] else O.ERR_BAD_ARG


def pair_segments(ix, ns: int, row_status, s: int, t: int):
    """rp_plan: -> (segments [(source, off, len)], bytes taken, bytes kept)."""
    f0, n = RC.rows_of(ix, s)
    f1, total = f0 + n, ix["total"][s]
    segs, taken, kept = [], 0, 0
    cur = None                                                          # [good, off]
    for i in range(f0, f1):
        a, e = ix["start"][i], X.row_end(ix, f1, total, i)
        ln = e - a if e >= a else 0
        if ln == 0:
            continue
        good = row_status[i] == O.OK
        if cur is None or cur[0] != good:
            if cur is not None:
                segs.append((s if cur[0] else ns + t, cur[1], (a - cur[1]) & U64))
            cur = [good, a]
        if good:
            kept = (kept + ln) & U64
        else:
            taken = (taken + ln) & U64
    if cur is not None:
        segs.append((s if cur[0] else ns + t, cur[1], (total - cur[1]) & U64))
    return segs, taken, kept


def repair_plan(ix, ns: int, row_status, rep_total, rep_tail, rp_stream, rp_replica, max_segs: int | None = None):
    """snp_frame_repair_plan_batch.  The index needs no positions; nentries is the rows of start that row_status covers.  None: a bound that
    admits all.  -> dict of plan_status, segs (first, stream, off, len), result [4]."""
    max_segs = 1 << 62 if max_segs is None else max_segs
    ix = dict(ix)
    ne = min(len(ix["start"]), len(row_status))
    ix["start"], ix["pos"] = ix["start"][:ne], [0] * ne
    plan_status, segs = [], dict(first=[0], stream=[], off=[], len=[])
    need = taken = kept = 0
    for s, t in zip(rp_stream, rp_replica):
        st = pair_status(ix, ns, rep_total, rep_tail, s, t)
        if st == O.OK:
            mine, tk, kp = pair_segments(ix, ns, row_status, s, t)
            need, taken, kept = need + len(mine), (taken + tk) & U64, (kept + kp) & U64
            if need <= max_segs:
                for src, off, ln in mine:
                    segs["stream"].append(src)
                    segs["off"].append(off)
                    segs["len"].append(ln)
            else:
                st = O.ERR_OUTPUT_TOO_SMALL
        plan_status.append(st)
        segs["first"].append(len(segs["stream"]))
    return dict(plan_status=plan_status, segs=segs, result=[need, sum(1 for v in plan_status if v == O.OK), taken, kept])


def joined(streams, ix, rep_streams, rep_ix):
    """The batch a repair recipe is composed from: the streams followed by the replicas: -> (streams, index)."""
    ne = nentries_of(ix)
    rows = min(ix["first"][len(streams)], ne)
    out = dict(first=list(ix["first"][:len(streams)]) + [v + rows for v in rep_ix["first"]], start=ix["start"][:rows] + list(rep_ix["start"]),
               pos=ix["pos"][:rows] + list(rep_ix["pos"]), total=list(ix["total"]) + list(rep_ix["total"]), tail=list(ix["tail"]) + list(rep_ix["tail"]))
    return list(streams) + list(rep_streams), out


# ---- the plan check program (tests/abi/frame_verify_plan_check.hip) ----------------------------------------------------------------------------------
def write_cases(path: str, rounds, streams, indexes, plans):
    """rounds: (slot_bytes, scratch_cap, nentries); then the streams and, per index (any lists at all), (slot_bytes, scratch_cap); then the
    planner's cases: (index, nstreams, row_status, rep_total, rep_tail, pairs) with the index given as numbers alone."""
    ns = len(streams)
    with open(path, "wb") as f:
        f.write(struct.pack("<4Q", len(rounds), ns, len(indexes), len(plans)))
        for q in rounds:
            f.write(struct.pack("<3Q", *q))
        for s in streams:
            f.write(struct.pack("<Q", len(s)))
            f.write(s)
        for ix, slot_bytes, scratch_cap in indexes:
            ne = nentries_of(ix)
            f.write(struct.pack("<3Q", ne, slot_bytes, scratch_cap))
            for key, n in (("first", ns + 1), ("total", ns), ("tail", ns), ("start", ne), ("pos", ne)):
                assert len(ix[key]) >= n
                f.write(struct.pack("<%dQ" % n, *[int(v) & U64 for v in ix[key][:n]]))
        for ix, pns, row_status, rep_total, rep_tail, pairs in plans:
            ne = min(len(ix["start"]), len(row_status))
            f.write(struct.pack("<4Q", pns, ne, len(rep_total), len(pairs)))
            for vals, n in ((ix["first"], pns + 1), (ix["total"], pns), (ix["tail"], pns), (ix["start"], ne), (row_status, ne),
                            (rep_total, len(rep_total)), (rep_tail, len(rep_total))):
                assert len(vals) >= n
                f.write(struct.pack("<%dQ" % n, *[int(v) & U64 for v in vals[:n]]))
            for s, t in pairs:
                f.write(struct.pack("<2Q", s, t))


def check_lines(rounds, streams, indexes, plans):
    """What the plan check program must print for write_cases' input.  The program knows no decoder: a row whose round would tell prints 0."""
    lines = []
    for slot_bytes, scratch_cap, ne in rounds:
        stride, per, n = rounds_of(slot_bytes, scratch_cap, ne)
        probe = [i % per * stride for i in (0, ne // 2, ne - 1)] if per and ne else [0, 0, 0]
        lines.append("R %d %d %d %d %d %d" % (stride, per, n, *probe))
    for ix, slot_bytes, scratch_cap in indexes:
        got = verify_plan(streams, ix, slot_bytes, scratch_cap)
        pending = [O.OK if v not in (SKIPPED, O.ERR_BAD_ARG, O.ERR_OUTPUT_TOO_SMALL) else v for v in got["row_status"]]
        # (a decoded row's status is left open: the program prints the sums as if every such row were OK)
        sums = verify_plan(streams, ix, slot_bytes, scratch_cap, status_of=lambda chunk: O.OK)
        assert sums["row_status"] == pending
        lines.append("V" + "".join(" %d" % v for v in pending))
        lines.append("S" + "".join(" %d:%d:%d:%d:%d" % (st, nb, fb, bb, fl) for st, nb, fb, bb, fl in
                                   zip(sums["status"], sums["nbad"], sums["first_bad"], sums["bad_bytes"], sums["flags"])) +
                     " |" + "".join(" %d" % v for v in sums["result"]))
    for ix, pns, row_status, rep_total, rep_tail, pairs in plans:
        want = repair_plan(ix, pns, row_status, rep_total, rep_tail, [p[0] for p in pairs], [p[1] for p in pairs])
        f = want["segs"]["first"]
        parts = []
        for j, st in enumerate(want["plan_status"]):
            mine = range(f[j], f[j + 1])
            parts.append(" %d" % st + "".join(" %d:%d:%d" % (want["segs"]["stream"][g], want["segs"]["off"][g], want["segs"]["len"][g]) for g in mine) + " ;")
        lines.append("P" + "".join(parts) + " |" + "".join(" %d" % v for v in want["result"]))
    return lines


# ---- cases the CPU and the GPU tests share -----------------------------------------------------------------------------------------------------------
def stream_of_chunks(chunks) -> bytes:
    return M.STREAM_ID + b"".join(chunks)


def shape_streams(html: bytes, variant: int = O.HASH_CRC32C):
    """name -> stream: 0, 1 and 7 rows; rows of 0, 1, 4096 and 65536 decoded bytes; type-0x01 chunks; skippable and padding chunks between rows."""
    ch = lambda raw, comp=True: M.data_chunk(raw, comp, variant)         # noqa: E731
    skip, pad, zero = M.chunk(0x80, b"note"), M.chunk(0xFE, bytes(21)), M.data_chunk(b"", compressed=False)
    seven = [ch(html[o:o + n]) for o, n in ((0, 700), (700, 1), (701, 4096), (4797, 300), (5097, 2000), (7097, 64), (7161, 999))]
    return {
        "no_rows": M.STREAM_ID,
        "one_row": stream_of_chunks([ch(html[:4096])]),
        "seven_rows": stream_of_chunks(seven),
        "sizes": stream_of_chunks([zero, ch(html[:1]), ch(html[1:4097]), ch(html[:65536]), ch(b"", True), ch(html[5:6], False)]),
        "raw_chunks": stream_of_chunks([ch(html[:300], False), ch(html[300:4396], False), ch(html[:65536], False)]),
        "skippable_between": M.STREAM_ID + skip + ch(html[:1000]) + pad + ch(html[1000:1700]) + skip + M.STREAM_ID + ch(html[1700:3000]) + skip,
    }


def seven_by_three(html: bytes):
    """The 7-row, 3-stream batch of the round tests: 21 rows of 100 .. 3000 bytes."""
    streams = []
    for b in range(3):
        o, chunks = 9000 * b, []
        for k in range(7):
            n = 100 + 400 * ((k * 3 + b) % 7)
            chunks.append(M.data_chunk(html[o:o + n], compressed=(k + b) % 3 != 0))
            o += n
        streams.append(stream_of_chunks(chunks))
    return streams


FLIP_RAW = bytes(range(40, 80))                                         # the short chunk of the flip tests: 40 bytes with no repeat, so one literal


def flip(s: bytes, at: int, bit: int) -> bytes:
    out = bytearray(s)
    out[at] ^= 1 << bit
    return bytes(out)


def flip_stream(html: bytes, compressed: bool):
    """The stream of the flip tests: a short chunk (FLIP_RAW) between two others: -> (stream, index, where the chunk begins, its bytes)."""
    chunk = M.data_chunk(FLIP_RAW, compressed)
    first = M.data_chunk(html[:300])
    s = stream_of_chunks([first, chunk, M.data_chunk(html[300:500])])
    return s, X.build_index([s]), 10 + len(first), len(chunk)


def same_bytes_flips(s: bytes, lo: int, n: int):
    """The single-bit flips (at, bit) of the chunk s[lo .. lo + n) after which the oracle's frame decoder still gives the chunk's bytes --
    the chunk alone behind the identifier, flipped: no damage to what the CRC covers, by the reference's own rules."""
    want = O.frame_decode(M.STREAM_ID + s[lo:lo + n])
    out = set()
    for at in range(lo, lo + n):
        for bit in range(8):
            bad = flip(s, at, bit)
            try:
                if O.frame_decode(M.STREAM_ID + bad[lo:lo + n]) == want:
                    out.add((at, bit))
            except O.OracleError:
                pass
    return out


def unsound_indexes(ix, streams, rng):
    """name -> an index that does not hold for the streams: the dedup model's."""
    import frame_dedup_model as D
    return D.unsound_indexes(ix, streams, rng)

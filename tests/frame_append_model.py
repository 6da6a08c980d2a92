"""Pure-Python statement of include/snappier_hip_frame_append.h (snp_frame_append_indexed_batch): bytes appended in place to framed streams kept
with their chunk index.  The planning half is a transliteration of csrc/frame_append_device.h on top of frame_index_model.py and
frame_buffers_model.hop (the index is untrusted input: clamp for clamp, so that it also says what the header does with an index filled with
anything at all); the rest states the contract: reopen or not, the cut, the new chunks (frame_chunked_model.chunks_of: slots of the chunked
encode), the in-order admission by max_tails / max_slots over the streams that passed, buf_cap, the verdicts, the new index, out_bound and
d_result.  The CPU and the GPU tests share it."""
import struct

import frame_buffers_model as M
import frame_chunked_model as K
import frame_index_model as X
import frame_range_model as R
import oracle as O

U64 = R.U64
MAX_DEC = 65536
CHUNK_SIZES = [1, 63, 64, 65, 4096, 65536]


def a_lengths(cb: int):
    return [0, 1, cb - 1, cb, cb + 1, 3 * cb + 7]


def s_lengths(cb: int):
    return [1, cb - 1, cb, cb + 1, 2 * cb + 3]


# ---- the planning (csrc/frame_append_device.h) -------------------------------------------------------------------------------------------------
def rows_of(ix, b: int):
    """fa_rows: -> (f0, rows), inside nentries whatever idx_first holds."""
    ne = min(len(ix["start"]), len(ix["pos"]))
    a, e = min(ix["first"][b], ne), min(ix["first"][b + 1], ne)
    return a, max(e - a, 0)


def plan(ix, b: int, n: int, src_len: int, cb: int, hop_at):
    """fa_plan: -> dict of status, append, reopen, ident, d, fill, f0, rows, cut, rest, fresh, bound, row (the reopened tail as the chunk table
    takes it).  hop_at(pos) -> M.Hop of the header at pos < n."""
    f0, rows = rows_of(ix, b)
    k = dict(status=O.OK, append=False, reopen=False, ident=False, d=0, fill=0, f0=f0, rows=rows, cut=n, rest=0, fresh=0, bound=n, row=None)
    if src_len == 0:
        return k
    k["status"] = O.ERR_BAD_ARG
    tail = ix["tail"][b]
    if tail < O.OK or tail > O.ERR_TRUNCATED_STREAM:
        return k
    if tail != O.OK:
        k["status"] = tail
        return k
    ne = min(len(ix["start"]), len(ix["pos"]))
    g0, g1 = min(ix["first"][b], ne), min(ix["first"][b + 1], ne)
    if g1 < g0:
        return k
    total = ix["total"][b]
    if total + src_len > U64:
        return k
    old = 0
    if g1 > g0:
        last = g1 - 1
        start, pos = ix["start"][last], ix["pos"][last]
        if start > total or pos >= n:
            return k
        h = hop_at(pos)
        if h.kind != "data" or h.dec != total - start:
            return k
        if 0 < h.dec < cb and h.next == n:
            if h.dec > MAX_DEC:
                return k
            k.update(reopen=True, d=h.dec, cut=pos, row=(h.type, pos + 8, h.body_len, h.crc, start, h.dec))
            old = h.next - pos
    elif total != 0:
        return k
    fill = min(src_len, cb - k["d"]) if k["reopen"] else 0
    rest = src_len - fill
    fresh = K.nchunks(rest, cb)
    k.update(status=O.OK, append=True, ident=n == 0, fill=fill, rest=rest, fresh=fresh,
             bound=n - old + (8 + k["d"] + fill if k["reopen"] else 0) + 8 * fresh + rest + (10 if n == 0 else 0))
    return k


def piece(rest: int, fill: int, cb: int, j: int):
    """fa_piece: -> (len, offset among the stream's appended bytes)."""
    return min(rest - j * cb, cb), fill + j * cb


# ---- the whole append --------------------------------------------------------------------------------------------------------------------------
def append_plan(streams, ix, srcs, cb: int, caps=None, max_tails: int | None = None, max_slots: int | None = None, variant: int = O.HASH_CRC32C):
    """snp_frame_append_indexed_batch.  srcs: the bytes each stream takes.  None: a bound that admits all.
    -> dict of status, new_len, streams (the new stream, None unless written), cut, index (the new one: first, start, pos, total, tail),
    out_bound, result [4]."""
    assert 1 <= cb <= MAX_DEC
    ns = len(streams)
    BIG = 1 << 62
    max_tails = BIG if max_tails is None else max_tails
    max_slots = BIG if max_slots is None else max_slots
    caps = [BIG] * ns if caps is None else caps
    ne = min(len(ix["start"]), len(ix["pos"]))
    cap_rows = ne + max_slots                                           # rows the new start / pos arrays hold
    pl = [plan(ix, b, len(streams[b]), len(srcs[b]), cb, lambda pos, s=streams[b]: M.hop(s, pos)) for b in range(ns)]
    tails = slots = 0
    status, new_len, new, cut, bound = [], [], [None] * ns, [], []
    fresh_pos = [[] for _ in range(ns)]
    for b, k in enumerate(pl):
        s = streams[b]
        status.append(k["status"])
        new_len.append(len(s))
        cut.append(k["cut"])
        bound.append(k["bound"])
        if not k["append"]:
            continue
        tails += k["reopen"]
        slots += min(k["fresh"], 1 << 32)                               # (no bound admits 2^32 slots: a stream is counted as at most that)
        status[b] = O.ERR_OUTPUT_TOO_SMALL
        if tails > max_tails or slots > max_slots:
            continue
        old = b""
        if k["reopen"]:
            st, old = R.chunk_result(s, k["row"])
            if st != O.OK:
                status[b], bound[b] = st, len(s)
                continue
        src = srcs[b]
        out = [s[:k["cut"]]] + ([M.STREAM_ID] if k["ident"] else [])
        if k["reopen"]:
            out += K.chunks_of(old + src[:k["fill"]], MAX_DEC, variant)
        at = sum(len(x) for x in out)
        for c in K.chunks_of(src[k["fill"]:], cb, variant):
            fresh_pos[b].append(at)
            out.append(c)
            at += len(c)
        assert len(fresh_pos[b]) == k["fresh"]
        if at > caps[b]:
            fresh_pos[b] = []
            continue
        new[b] = b"".join(out)
        assert len(new[b]) == at <= k["bound"]
        status[b], new_len[b] = O.OK, at
    # the new index: every stream's old rows (clamped), the rows of a written stream's fresh chunks; cut off at the capacity of the row arrays
    first, start, pos, total, tail = [0], [], [], [], []
    for b, k in enumerate(pl):
        start += ix["start"][k["f0"]:k["f0"] + k["rows"]]
        pos += ix["pos"][k["f0"]:k["f0"] + k["rows"]]
        if new[b] is not None:
            start += [(ix["total"][b] + k["fill"] + j * cb) & U64 for j in range(k["fresh"])]
            pos += fresh_pos[b]
        first.append(len(start))
        total.append((ix["total"][b] + len(srcs[b])) & U64 if new[b] is not None else ix["total"][b])
        tail.append(O.OK if new[b] is not None else ix["tail"][b])
    index = dict(first=[min(f, cap_rows) for f in first], start=start[:cap_rows], pos=pos[:cap_rows], total=total, tail=tail)
    grown = sum(new_len[b] - len(streams[b]) for b in range(ns) if new[b] is not None) & U64
    return dict(status=status, new_len=new_len, streams=new, cut=cut, index=index, out_bound=bound,
                result=[slots, grown, tails, sum(1 for x in new if x is not None)])


def needs(streams, ix, srcs, cb: int):
    """-> (max_tails, max_slots) that admit every stream: the sizing call."""
    res = append_plan(streams, ix, srcs, cb, max_tails=0, max_slots=0)["result"]
    return res[2], res[0]


def after(streams, got):
    """The batch after a call: the new streams where one was written, else the old."""
    return [n if n is not None else s for s, n in zip(streams, got["streams"])]


def same_index(a, b) -> bool:
    return all(list(a[key]) == list(b[key]) for key in ("first", "start", "pos", "total", "tail"))


# ---- streams the CPU and the GPU tests share ---------------------------------------------------------------------------------------------------
def tail_shapes(html: bytes, cb: int = 1000):
    """name -> (stream, reopened?) at chunk size cb: the tails the contract tells apart."""
    a = html[:2 * cb + cb // 2]
    s = K.stream_of(a, cb)
    return {
        "short_tail": (s, True),
        "full_tail": (K.stream_of(a[:2 * cb], cb), False),
        "tail_then_padding": (s + M.chunk(0xFE, bytes(37)), False),
        "tail_then_skippable": (s + M.chunk(0x80, b"note"), False),
        "zero_length_tail": (s + M.data_chunk(b"", compressed=False), False),
        "larger_chunks": (K.stream_of(a, 2 * cb + cb // 2), False),
        "identifier_only": (M.STREAM_ID, False),
        "empty": (b"", False),
        "one_byte_tail": (K.stream_of(a[:2 * cb + 1], cb), True),
    }


def unsound_indexes(ix, streams, rng):
    """frame_update_model.unsound_indexes: the thirteen."""
    import frame_update_model as U
    return U.unsound_indexes(ix, streams, rng)


# ---- the cases of the planning check (tests/abi/frame_append_plan_check.hip) ---------------------------------------------------------------------
def plan_line(k, cb: int, total: int) -> str:
    """What the planning header must give for one stream, as the check program prints it: the plan, then the first and the last fresh piece
    and row start."""
    p0 = p1 = (0, 0)
    r0 = r1 = 0
    if k["fresh"]:
        p0, p1 = piece(k["rest"], k["fill"], cb, 0), piece(k["rest"], k["fill"], cb, k["fresh"] - 1)
        r0, r1 = (total + k["fill"]) & U64, (total + k["fill"] + (k["fresh"] - 1) * cb) & U64
    return "%d %d %d %d %d %d %d %d %d %d %d %d | %d %d %d %d %d %d" % (
        k["status"], k["append"], k["reopen"], k["ident"], k["d"], k["fill"], k["f0"], k["rows"], k["cut"], k["rest"], k["fresh"], k["bound"] & U64,
        p0[0], p0[1], r0, p1[0], p1[1], r1)


def plan_lines(ix, streams, src_lens, cb: int):
    return [plan_line(plan(ix, b, len(s), src_lens[b], cb, lambda pos, s=s: M.hop(s, pos)), cb, ix["total"][b]) for b, s in enumerate(streams)]


def numeric_hop(n: int, pos: int, kind: int, size: int, dec: int) -> M.Hop:
    """A hop given as numbers (the check program's second kind of case): a header at `pos` of a stream of n bytes that is too long to hold.
    kind: 0 data, 1 skippable."""
    return M.Hop("data" if kind == 0 else "skip", pos + 4 + size, type=1, body_len=size - 4, dec=dec)


def numeric_line(case) -> str:
    """case: dict of n, src_len, cb, total, start, pos, tail, rows (0 | 1), kind, size, dec."""
    c = case
    ix = dict(first=[0, c["rows"]], start=[c["start"]] * c["rows"], pos=[c["pos"]] * c["rows"], total=[c["total"]], tail=[c["tail"]])
    k = plan(ix, 0, c["n"], c["src_len"], c["cb"], lambda pos: numeric_hop(c["n"], pos, c["kind"], c["size"], c["dec"]))
    return plan_line(k, c["cb"], c["total"])


def write_cases(path: str, streams, cases, numeric):
    """The input of the check program: the streams; every case -- an index (any lists at all), chunk_bytes and src_len per stream; then the
    numeric cases, eleven words each."""
    with open(path, "wb") as f:
        f.write(struct.pack("<Q", len(streams)))
        for s in streams:
            f.write(struct.pack("<Q", len(s)))
            f.write(s)
        f.write(struct.pack("<Q", len(cases)))
        for ix, cb, src_lens in cases:
            ne = min(len(ix["start"]), len(ix["pos"]))
            f.write(struct.pack("<2Q", ne, cb))
            for key, n in (("first", len(streams) + 1), ("total", len(streams)), ("tail", len(streams)), ("start", ne), ("pos", ne)):
                assert len(ix[key]) >= n
                f.write(struct.pack("<%dQ" % n, *[int(v) & U64 for v in ix[key][:n]]))
            f.write(struct.pack("<%dQ" % len(streams), *[int(v) & U64 for v in src_lens]))
        f.write(struct.pack("<Q", len(numeric)))
        for c in numeric:
            f.write(struct.pack("<11Q", *[int(c[key]) & U64 for key in ("n", "src_len", "cb", "total", "start", "pos", "tail", "rows", "kind", "size", "dec")]))

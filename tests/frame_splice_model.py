"""Pure-Python statement of include/snappier_hip_frame_splice.h (snp_frame_splice_indexed_batch): ONE splice per framed stream kept with its chunk
index -- decoded bytes [off, off + del) replaced by ins source bytes.  The planning half is a transliteration of csrc/frame_splice_device.h on top
of frame_index_model.py and frame_buffers_model.hop (the index is untrusted input: clamp for clamp and probe for probe, so that it also says
what the header does with an index filled with anything at all); the rest states the contract: the owned rows, the edges, the hole, the new
chunks (frame_chunked_model.chunks_of: slots of the chunked encode), the in-order admission by max_slots / stage_cap over the streams that
passed, out_cap, the verdicts, the new index, out_bound and d_result.  The CPU and the GPU tests share it."""
import struct

import frame_buffers_model as M
import frame_chunked_model as K
import frame_index_model as X
import frame_range_model as R
import oracle as O

U64 = R.U64
MAX_DEC = 65536
MAX_PIECES = 1 << 32
MAX_STAGE = (1 << 48) + (1 << 18)
CHUNK_SIZES = [1, 63, 64, 65, 4096, 65536]


# ---- the planning (csrc/frame_splice_device.h) -------------------------------------------------------------------------------------------------
def rows_of(ix, b: int):
    """fs_rows: -> (f0, rows), inside nentries whatever idx_first holds."""
    ne = min(len(ix["start"]), len(ix["pos"]))
    a, e = min(ix["first"][b], ne), min(ix["first"][b + 1], ne)
    return a, max(e - a, 0)


def _blank(f0: int, rows: int, status: int):
    return dict(status=status, splice=False, ident=False, head=False, tail=False, hl=0, tl=0, e0=0, e1=0, f0=f0, rows=rows, r0=f0, r1=f0, p0=0, p1=0,
                tpos=0, region=0, pieces=0, stage=0, bound=0, hrow=None, trow=None)


def plan(ix, b: int, n: int, off: int, dele: int, ins: int, cb: int, hop_at):
    """fs_plan: -> dict of status, splice, ident, head, tail, hl, tl, e0, e1, f0, rows, r0, r1, p0, p1, tpos, region, pieces, stage, bound, and
    the edge rows as the chunk table takes them (hrow: the head row when it is decoded, trow: the tail row when it is another one).  A stream
    that is left alone or refused has its verdict and its old rows, nothing half-planned.  hop_at(pos) -> M.Hop of the header at pos < n."""
    k = _plan(ix, b, n, off, dele, ins, cb, hop_at)
    return k if k["splice"] else _blank(k["f0"], k["rows"], k["status"])


def _plan(ix, b: int, n: int, off: int, dele: int, ins: int, cb: int, hop_at):
    f0, rows = rows_of(ix, b)
    k = _blank(f0, rows, O.OK)
    if dele == 0 and ins == 0:
        return k
    k["status"] = O.ERR_BAD_ARG
    walk = ix["tail"][b]
    if walk < O.OK or walk > O.ERR_TRUNCATED_STREAM:
        return k
    if walk != O.OK:
        k["status"] = walk
        return k
    ne = min(len(ix["start"]), len(ix["pos"]))
    g0, g1 = min(ix["first"][b], ne), min(ix["first"][b + 1], ne)
    if g1 < g0:
        return k
    total, lo, hi = ix["total"][b], off, off + dele
    if hi > U64 or hi > total:
        return k
    if total - dele + ins > U64:
        return k
    if dele == 0 and lo == total:
        if g1 == g0 and total != 0:
            return k
        k.update(r0=g1, r1=g1, p0=n, p1=n, tpos=n)
    else:
        i0 = X.first_where(g0, g1, lambda i: X.row_end(ix, g1, total, i) > lo)
        if i0 >= g1:
            return k
        i1 = i0 + 1
        if dele:
            i1 = X.first_where(g0, g1, lambda i: ix["start"][i] >= hi)
            if i1 <= i0:
                return k
        s0 = ix["start"][i0]
        if s0 > lo:
            return k
        pos0 = ix["pos"][i0]
        if pos0 >= n:
            return k
        h0 = hop_at(pos0)
        if h0.kind != "data":
            return k
        k.update(r0=i0, p0=pos0)
        if dele == 0 and s0 == lo:
            k.update(r1=i0, p1=pos0, tpos=pos0)
        else:
            z0 = X.row_end(ix, g1, total, i0)
            if z0 < s0 or z0 - s0 != h0.dec:
                return k
            h1, last, tpos, s1 = h0, i1 - 1, pos0, s0
            if last != i0:
                s1, pos1 = ix["start"][last], ix["pos"][last]
                e1 = X.row_end(ix, g1, total, last)
                if e1 < s1 or pos1 >= n or pos1 < h0.next:
                    return k
                h1 = hop_at(pos1)
                if h1.kind != "data" or e1 - s1 != h1.dec:
                    return k
                tpos = pos1
            else:
                e1 = z0
            if e1 < hi:
                return k
            head, tail = s0 < lo, e1 > hi
            if (head and h0.dec > MAX_DEC) or (tail and h1.dec > MAX_DEC):
                return k
            shared = head and last == i0
            k.update(r1=i1, p1=h1.next, tpos=tpos, head=head, tail=tail, hl=lo - s0, tl=e1 - hi, e0=h0.dec if head else 0,
                     e1=h1.dec if tail and not shared else 0,
                     hrow=(h0.type, pos0 + 8, h0.body_len, h0.crc, s0, h0.dec) if head else None,
                     trow=(h1.type, tpos + 8, h1.body_len, h1.crc, s1, h1.dec) if tail and not shared else None)
    region = k["hl"] + ins + k["tl"]
    pieces = K.nchunks(region, cb)
    k.update(status=O.OK, splice=True, ident=n == 0, region=region, pieces=pieces, stage=min(k["e0"] + k["e1"] + region, U64),
             bound=(n - (k["p1"] - k["p0"]) + 8 * pieces + region + (10 if n == 0 else 0)) & U64)
    return k


def piece(region: int, cb: int, j: int):
    """fs_piece: -> (len, offset in the region)."""
    return min(region - j * cb, cb), j * cb


# ---- the whole splice --------------------------------------------------------------------------------------------------------------------------
def splice_plan(streams, ix, reqs, srcs, cb: int, caps=None, max_slots: int | None = None, stage_cap: int | None = None, variant: int = O.HASH_CRC32C):
    """snp_frame_splice_indexed_batch.  reqs: (off, del) per stream; srcs: the bytes each stream takes in their place.  None: a bound that admits all.
    -> dict of status, out_len, streams (the new stream, None unless written), hole ((P0, P1) per stream), index (the new one: first, start,
    pos, total, tail), out_bound, result [4]."""
    assert 1 <= cb <= MAX_DEC
    ns = len(streams)
    BIG = 1 << 62
    max_slots = BIG if max_slots is None else max_slots
    stage_cap = BIG if stage_cap is None else stage_cap
    caps = [BIG] * ns if caps is None else caps
    ne = min(len(ix["start"]), len(ix["pos"]))
    cap_rows = ne + max_slots                                           # rows the new start / pos arrays hold
    pl = [plan(ix, b, len(streams[b]), reqs[b][0], reqs[b][1], len(srcs[b]), cb, lambda pos, s=streams[b]: M.hop(s, pos)) for b in range(ns)]
    slots = stage = 0
    status, out_len, new, bound = [], [], [None] * ns, []
    new_pos, fresh = [[] for _ in range(ns)], [0] * ns
    for b, k in enumerate(pl):
        s = streams[b]
        status.append(k["status"])
        out_len.append(0)
        bound.append(k["bound"] if k["splice"] else 0)
        if not k["splice"]:
            continue
        slots += min(k["pieces"], MAX_PIECES)
        stage += min(k["stage"], MAX_STAGE)
        status[b] = O.ERR_OUTPUT_TOO_SMALL
        if slots > max_slots or stage > stage_cap:
            continue
        head = tail = b""
        failed = O.OK
        for row in (k["hrow"], k["trow"]):                              # the head edge's status first
            if row is not None and failed == O.OK:
                failed, dec = R.chunk_result(s, row)
                if failed == O.OK:
                    if row is k["hrow"]:
                        head = dec
                    else:
                        tail = dec
        if failed != O.OK:
            status[b], bound[b] = failed, 0
            continue
        if k["tail"] and k["trow"] is None:
            tail = head                                                 # both edges are one row: decoded once
        region = head[:k["hl"]] + srcs[b] + (tail[len(tail) - k["tl"]:] if k["tl"] else b"")
        assert len(region) == k["region"]
        out = [s[:k["p0"]]] + ([M.STREAM_ID] if k["ident"] else [])
        at = sum(len(x) for x in out)
        for c in K.chunks_of(region, cb, variant):
            new_pos[b].append(at)
            out.append(c)
            at += len(c)
        assert len(new_pos[b]) == k["pieces"]
        fresh[b] = at - k["p0"]
        out.append(s[k["p1"]:])
        at += len(s) - k["p1"]
        if at > caps[b]:
            new_pos[b] = []
            continue
        new[b] = b"".join(out)
        assert len(new[b]) == at <= k["bound"]
        status[b], out_len[b] = O.OK, at
    # the new index: a written stream's rows before r0, its new chunks' rows, its rows from r1 on, moved; every other stream's old rows (clamped)
    first, start, pos, total, tail = [0], [], [], [], []
    for b, k in enumerate(pl):
        f0, f1 = k["f0"], k["f0"] + k["rows"]
        if new[b] is None:
            start += ix["start"][f0:f1]
            pos += ix["pos"][f0:f1]
        else:
            off, dele, ins = reqs[b][0], reqs[b][1], len(srcs[b])
            start += ix["start"][f0:k["r0"]] + [(off - k["hl"] + j * cb) & U64 for j in range(k["pieces"])]
            start += [(v + ins - dele) & U64 for v in ix["start"][k["r1"]:f1]]
            pos += ix["pos"][f0:k["r0"]] + new_pos[b] + [(v + fresh[b] - (k["p1"] - k["p0"])) & U64 for v in ix["pos"][k["r1"]:f1]]
        first.append(len(start))
        total.append((ix["total"][b] - reqs[b][1] + len(srcs[b])) & U64 if new[b] is not None else ix["total"][b])
        tail.append(O.OK if new[b] is not None else ix["tail"][b])
    index = dict(first=[min(f, cap_rows) for f in first], start=start[:cap_rows], pos=pos[:cap_rows], total=total, tail=tail)
    return dict(status=status, out_len=out_len, streams=new, hole=[(k["p0"], k["p1"]) for k in pl], index=index, out_bound=bound,
                result=[slots & U64, sum(out_len) & U64, stage & U64, sum(1 for x in new if x is not None)])


def needs(streams, ix, reqs, srcs, cb: int):
    """-> (max_slots, stage_cap) that admit every stream: the sizing call."""
    res = splice_plan(streams, ix, reqs, srcs, cb, caps=[0] * len(streams), max_slots=0, stage_cap=0)["result"]
    return res[0], res[2]


def after(streams, got):
    """The batch after a call: the new streams where one was written, else the old."""
    return [n if n is not None else s for s, n in zip(streams, got["streams"])]


def edited(raw: bytes, off: int, dele: int, src: bytes) -> bytes:
    return raw[:off] + src + raw[off + dele:]


def same_index(a, b) -> bool:
    return all(list(a[key]) == list(b[key]) for key in ("first", "start", "pos", "total", "tail"))


# ---- cases the CPU and the GPU tests share ---------------------------------------------------------------------------------------------------------
def named_cases(cb: int, nchunks: int = 5):
    """name -> (decoded length of the stream, off, del, ins) for a stream of at most `nchunks` chunks of cb bytes, the last one short: the splices
    the contract tells apart.  (cb = 1 has no mid-chunk offset: those cases fall on boundaries there, which is what one-byte chunks allow.)"""
    n = (nchunks - 1) * cb + (cb + 1) // 2
    mid = cb + cb // 2                                                  # inside chunk 1
    return {
        "insert_at_0": (n, 0, 0, cb // 3 + 1),
        "insert_mid_chunk": (n, mid, 0, cb + 7),
        "insert_on_boundary": (n, 2 * cb, 0, 2 * cb),
        "insert_at_total": (n, n, 0, cb + 1),
        "delete_inside_one_chunk": (n, cb + cb // 4, cb // 2, 0),
        "delete_across_chunks": (n, cb // 2, 2 * cb, 0),
        "delete_whole_chunks": (n, cb, 2 * cb, 0),
        "delete_everything": (n, 0, n, 0),
        "truncate_to_0": (n, 0, n, 0),
        "truncate_mid_chunk": (n, mid, n - mid, 0),
        "truncate_to_boundary": (n, 2 * cb, n - 2 * cb, 0),
        "drop_prefix": (n, 0, mid, 0),
        "delete_everything_and_insert": (n, 0, n, 2 * cb + 1),
        "replace_longer": (n, cb // 2, cb, 2 * cb + 3),
        "replace_shorter": (n, mid, 2 * cb, 5),
        "empty_stream_insert": (0, 0, 0, cb + 2),
        "not_named": (n, 3, 0, 0),
    }


def foreign_streams(html: bytes):
    """name -> (stream, decoded bytes, (off, del, ins), non-data chunks dropped?): streams no encoder of this project writes -- skippable,
    padding and repeated-identifier chunks inside and outside the hole, zero-length data chunks at both borders of it and inside."""
    a, b, c, d = html[:1000], html[1000:1700], html[1700:3000], html[3000:3400]
    skip, pad, zero = M.chunk(0x80, b"note"), M.chunk(0xFE, bytes(21)), M.data_chunk(b"", compressed=False)
    ch = M.data_chunk
    raw = a + b + c + d
    inside = M.STREAM_ID + ch(a) + ch(b) + skip + pad + M.STREAM_ID + ch(c) + ch(d)
    outside = M.STREAM_ID + skip + ch(a) + pad + ch(b) + ch(c) + M.STREAM_ID + ch(d) + skip
    zeros = M.STREAM_ID + ch(a) + zero + ch(b) + zero + ch(c) + zero + ch(d) + zero
    return {
        "non_data_inside_the_hole": (inside, raw, (1500, 1000, 300), True),           # rows 1 and 2 owned: what lies between them goes
        "non_data_outside_the_hole": (outside, raw, (1200, 1000, 300), False),        # rows 1 and 2 owned, neighbours: everything else stays
        "non_data_before_an_insertion_point": (inside, raw, (1700, 0, 50), False),    # on the boundary behind them: in front of the header
        "zero_length_at_both_borders": (zeros, raw, (1000, 700, 10), False),          # exactly row b: the zero-length chunks around it stay
        "zero_length_inside": (zeros, raw, (500, 1700, 10), False),                   # a .. c in part: the two between them vanish
        "zero_length_tail_insert_at_total": (zeros, raw, (3400, 0, 99), False),
        "identifier_only": (M.STREAM_ID, b"", (0, 0, 777), False),
        "no_identifier": (ch(a) + ch(b), a + b, (990, 20, 0), False),
    }


def unsound_indexes(ix, streams, rng):
    """frame_update_model.unsound_indexes: the thirteen."""
    import frame_update_model as U
    return U.unsound_indexes(ix, streams, rng)


# ---- the cases of the planning check (tests/abi/frame_splice_plan_check.hip) ---------------------------------------------------------------------
def plan_line(k, cb: int, off: int) -> str:
    """What the planning header must give for one stream, as the check program prints it: the plan, then the first and the last piece and the
    start of their rows."""
    p0 = p1 = (0, 0)
    r0 = r1 = 0
    if k["pieces"]:
        p0, p1 = piece(k["region"], cb, 0), piece(k["region"], cb, k["pieces"] - 1)
        r0, r1 = (off - k["hl"]) & U64, (off - k["hl"] + (k["pieces"] - 1) * cb) & U64
    return "%d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d | %d %d %d %d %d %d" % (
        k["status"], k["splice"], k["ident"], k["head"], k["tail"], k["hl"], k["tl"], k["e0"], k["e1"], k["f0"], k["rows"], k["r0"], k["r1"],
        k["p0"], k["p1"], k["tpos"], k["region"], k["pieces"], k["stage"], k["bound"] & U64, p0[0], p0[1], r0, p1[0], p1[1], r1)


def plan_lines(ix, streams, reqs, cb: int):
    """reqs: (off, del, ins) per stream."""
    return [plan_line(plan(ix, b, len(s), *reqs[b], cb, lambda pos, s=s: M.hop(s, pos)), cb, reqs[b][0]) for b, s in enumerate(streams)]


NUMERIC_KEYS = ("n", "off", "del", "ins", "cb", "total", "tail", "rows", "start0", "pos0", "kind0", "size0", "dec0", "start1", "pos1", "kind1",
                "size1", "dec1")


def numeric_line(case) -> str:
    """case: dict of NUMERIC_KEYS -- a stream of n bytes that is too long to hold, given as up to two index rows and the headers they point at
    (kind: 0 data, 1 skippable)."""
    c = case
    rows = c["rows"]
    ix = dict(first=[0, rows], start=[c["start0"], c["start1"]][:rows], pos=[c["pos0"], c["pos1"]][:rows], total=[c["total"]], tail=[c["tail"]])

    def hop_at(pos):
        j = 0 if pos == c["pos0"] else 1
        size = c["size%d" % j]
        return M.Hop("data" if c["kind%d" % j] == 0 else "skip", pos + 4 + size, type=1, body_len=size - 4, dec=c["dec%d" % j])

    return plan_line(plan(ix, 0, c["n"], c["off"], c["del"], c["ins"], c["cb"], hop_at), c["cb"], c["off"])


def write_cases(path: str, streams, cases, numeric):
    """The input of the check program: the streams; every case -- an index (any lists at all), chunk_bytes and (off, del, ins) per stream; then the
    numeric cases, eighteen words each."""
    with open(path, "wb") as f:
        f.write(struct.pack("<Q", len(streams)))
        for s in streams:
            f.write(struct.pack("<Q", len(s)))
            f.write(s)
        f.write(struct.pack("<Q", len(cases)))
        for ix, cb, reqs in cases:
            ne = min(len(ix["start"]), len(ix["pos"]))
            f.write(struct.pack("<2Q", ne, cb))
            for key, n in (("first", len(streams) + 1), ("total", len(streams)), ("tail", len(streams)), ("start", ne), ("pos", ne)):
                assert len(ix[key]) >= n
                f.write(struct.pack("<%dQ" % n, *[int(v) & U64 for v in ix[key][:n]]))
            for j in range(3):
                f.write(struct.pack("<%dQ" % len(streams), *[int(r[j]) & U64 for r in reqs]))
        f.write(struct.pack("<Q", len(numeric)))
        for c in numeric:
            f.write(struct.pack("<%dQ" % len(NUMERIC_KEYS), *[int(c[key]) & U64 for key in NUMERIC_KEYS]))

"""Pure-Python statement of include/snappier_hip_frame_update.h (snp_frame_write_indexed_batch): requests that replace decoded bytes of framed
streams through their chunk index.  The planning half is a transliteration of csrc/frame_update_device.h on top of frame_index_model.py (the
index is untrusted input: search for search, so that it also says what the header does with an index or a request list filled with anything at
all); the rest states the contract: which chunks are dirty, which of them are decoded, the new chunk (frame_chunked_model.chunks_of: one slot of
the chunked encode), the in-order admission by max_slots / stage_cap over the streams that passed, out_cap, the verdicts per stream and per
request, new_pos, out_bound and d_result.  The CPU and the GPU tests share it."""
import struct

import numpy as np

import frame_buffers_model as M
import frame_chunked_model as K
import frame_index_model as X
import frame_range_model as R
import oracle as O

U64 = R.U64
MAX_DEC = 65536
CHUNK_SIZES = [1, 63, 64, 65, 4096, 65536]


def lengths(cb: int):
    return [0, 1, cb - 1, cb, cb + 1, 3 * cb + 7]


# ---- the planning (csrc/frame_update_device.h) -------------------------------------------------------------------------------------------------
def lower(req_stream, b: int) -> int:
    """fu_lower."""
    return X.first_where(0, len(req_stream), lambda i: req_stream[i] >= b)


def window(ix, b: int, off: int, ln: int):
    """fu_window: the stream-side half of X.plan's dict, for row_check."""
    ne = min(len(ix["start"]), len(ix["pos"]))
    return dict(lo=off, hi=(off + ln) & U64, f1=min(ix["first"][b + 1], ne), total=ix["total"][b])


def plan(ix, streams, reqs, r: int):
    """fu_plan: -> dict of status, head, last, r0, r1."""
    k = dict(status=O.ERR_BAD_ARG, head=False, last=False, r0=0, r1=0)
    ns = len(streams)
    rs = [q[0] for q in reqs]
    b, off, ln = reqs[r]
    if b >= ns:
        return k
    if r > 0:
        pb, po, pl = reqs[r - 1]
        if pb > b:
            return k
        if pb == b and (po > off or min(po + pl, U64) > off):
            return k
    lb, ub = lower(rs, b), lower(rs, b + 1)
    if r < lb or r >= ub:
        return k
    if r > lb and rs[r - 1] != b:
        return k
    if r + 1 < ub and rs[r + 1] != b:
        return k
    p = X.plan(ix, ns, b, off, ln, ln)
    if p["status"] != O.OK:
        k["status"] = p["status"]
        return k
    if p["tail"] != O.OK:
        k["status"] = p["tail"]
        return k
    if off + ln > U64 or off + ln > p["total"]:
        return k
    if ln == 0:
        k["status"] = O.OK
        return k
    s = streams[b]
    for flag, i in ((p["head"], p["r0"]), (p["last"], p["r1"] - 1)):
        if flag:
            row = X.row_check(ix, s, p, i, False)
            if row is None or row[5] > MAX_DEC:
                return k
    k.update(status=O.OK, head=p["head"], last=p["last"], r0=p["r0"], r1=p["r1"])
    return k


def own(k, pred):
    """fu_own: -> (status, own0, cnt).  pred: the r1 of the previous request with rows, if it is one of the same stream, else None."""
    r0, r1 = k["r0"], k["r1"]
    if pred is None or pred <= r0:
        return O.OK, r0, r1 - r0
    if pred > r0 + 1:
        return O.ERR_BAD_ARG, r0, 0
    return O.OK, r0 + 1, r1 - r0 - 1


def row_check(ix, s: bytes, w, k, i: int, prev):
    """fu_row_check: -> the row as X.row_check gives it, or None.  prev: the stream's previous dirty row, or None."""
    edge = (i == k["r0"] and k["head"]) or (i == k["r1"] - 1 and k["last"])
    if i >= w["f1"]:
        return None
    row = X.row_check(ix, s, w, i, not edge)
    if row is None or row[5] > MAX_DEC:
        return None
    if prev is None:
        return row
    pp = ix["pos"][prev]
    if pp >= len(s):
        return None
    hp = M.hop(s, pp)
    return row if hp.kind == "data" and hp.next <= ix["pos"][i] else None


def planned(ix, streams, reqs):
    """Every request's plan, owned rows and checked slots, as the plan, own and check kernels make them.
    -> list of dict(status, head, last, r0, r1, own0, cnt, bytes, slots [(row number, row or None)], bad)."""
    out = []
    last_live = None
    for r, (b, off, ln) in enumerate(reqs):
        k = plan(ix, streams, reqs, r)
        k.update(own0=k["r0"], cnt=0, bytes=0, slots=[], bad=0, live=k["status"] == O.OK and k["r0"] < k["r1"])
        if k["live"]:
            p = out[last_live] if last_live is not None and reqs[last_live][0] == b else None
            st, own0, cnt = own(k, p["r1"] if p else None)
            if st != O.OK:
                k["status"] = st
            k.update(own0=own0, cnt=cnt)
            w = window(ix, b, off, ln)
            if cnt:
                k["bytes"] = (X.row_end(ix, w["f1"], w["total"], k["r1"] - 1) - ix["start"][own0]) & U64
            prev = p["r1"] - 1 if p else None
            for i in range(own0, own0 + cnt):
                row = row_check(ix, streams[b], w, k, i, prev)
                k["slots"].append((i, row))
                k["bad"] += row is None
                prev = i
            last_live = r
        out.append(k)
    return out


# ---- the whole write ---------------------------------------------------------------------------------------------------------------------------
def owner_of(first, nb: int, t: int) -> int:
    """scan_tiles.h owner_of over a table of first slots, whatever it holds."""
    lo, hi = 0, nb
    while hi - lo > 1:
        mid = lo + (hi - lo) // 2
        if first[mid] <= t:
            lo = mid
        else:
            hi = mid
    return lo


def new_chunk(piece: bytes, variant: int) -> bytes:
    return K.chunks_of(piece, MAX_DEC, variant)[0]


def write_plan(streams, ix, reqs, srcs, caps=None, max_slots: int | None = None, stage_cap: int | None = None, variant: int = O.HASH_CRC32C):
    """snp_frame_write_indexed_batch.  reqs: (stream number, req_off, req_len), srcs: the bytes of each.  None: a bound that admits all.
    -> dict of status, out_len, streams (the new stream, None unless written), req_status, new_pos, out_bound, result [4], dirty (per stream:
    [(old pos, old size, new chunk)] of the written ones)."""
    ns, nreq = len(streams), len(reqs)
    BIG = 1 << 62
    max_slots = BIG if max_slots is None else max_slots
    stage_cap = BIG if stage_cap is None else stage_cap
    caps = [BIG] * ns if caps is None else caps
    pl = planned(ix, streams, reqs)
    rs = [q[0] for q in reqs]
    fail = {}

    def failed(b, r, st):
        fail[b] = min(fail.get(b, (BIG, 0)), (r, st))

    for r, k in enumerate(pl):
        if rs[r] < ns and (k["status"] != O.OK or k["bad"]):
            failed(rs[r], r, k["status"] if k["status"] != O.OK else O.ERR_BAD_ARG)
    named, passed, mine = [], [], []
    for b in range(ns):
        lb, ub = lower(rs, b), lower(rs, b + 1)
        named.append(b in fail or (lb < ub and rs[lb] == b))
        passed.append(named[b] and b not in fail)
        mine.append(range(lb, ub) if passed[b] else range(0))
    slots = bytes_ = 0
    admitted = []
    for b in range(ns):
        slots += sum(pl[r]["cnt"] for r in mine[b])
        bytes_ += sum(pl[r]["bytes"] for r in mine[b])
        admitted.append(passed[b] and slots <= max_slots and bytes_ <= stage_cap)
    result = [slots, 0, bytes_, 0]
    status, out_len, new, bound, dirty = [O.OK] * ns, [0] * ns, [None] * ns, [0] * ns, [None] * ns
    new_pos = list(ix["pos"][:min(len(ix["start"]), len(ix["pos"]))])
    shifts = {}
    for b in range(ns):
        if not named[b]:
            continue
        if b in fail:
            status[b] = fail[b][1]
            continue
        s = streams[b]
        rows = [(i, row, r) for r in mine[b] for i, row in pl[r]["slots"]]
        bound[b] = len(s) + sum(8 + row[5] - (8 + row[2]) for _, row, _ in rows if row[5])
        status[b] = O.ERR_OUTPUT_TOO_SMALL
        if not admitted[b]:
            continue
        # the old bytes of the edges (decoded and verified whole), zeros where a request covers the chunk
        pieces, bad = {}, None
        for i, row, r in rows:
            k = pl[r]
            edge = (i == k["r0"] and k["head"]) or (i == k["r1"] - 1 and k["last"])
            if edge and row[5]:
                st, data = R.chunk_result(s, row)
                if st != O.OK:
                    bad = min(bad or (BIG, 0), (r, st))
                    continue
                pieces[i] = bytearray(data)
            else:
                pieces[i] = bytearray(row[5])
        if bad:
            status[b], bound[b] = bad[1], 0                            # (a stream that fails has no bound; the sizing call decodes nothing)
            continue
        start = {i: row[4] for i, row, _ in rows}
        for r in mine[b]:
            k, (_, off, ln) = pl[r], reqs[r]
            for i in range(k["r0"], k["r1"]) if k["live"] else ():
                lo, hi = max(off, start[i]), min(off + ln, start[i] + len(pieces[i]))
                if hi > lo:
                    pieces[i][lo - start[i]:hi - start[i]] = srcs[r][lo - off:hi - off]
        swaps = [(row[1] - 8, 8 + row[2], new_chunk(bytes(pieces[i]), variant), i) for i, row, _ in rows if row[5]]
        size = len(s) + sum(len(c) - o for _, o, c, _ in swaps)
        if size > caps[b]:
            continue
        out, at = [], 0
        for p, o, c, _ in swaps:
            out += [s[at:p], c]
            at = p + o
        new[b] = b"".join(out) + s[at:]
        assert len(new[b]) == size <= bound[b]
        status[b], out_len[b], dirty[b] = O.OK, size, [(p, o, c) for p, o, c, _ in swaps]
        shifts[b] = [(i, len(c) - o) for _, o, c, i in swaps]
    ne = len(new_pos)
    for i in range(ne):                                                 # k_fu_new_pos: idx_first is untrusted, the row is checked to be the stream's
        if not ns:
            break
        b = owner_of(ix["first"], ns, i)
        if b in shifts and min(ix["first"][b], ne) <= i < min(ix["first"][b + 1], ne):
            new_pos[i] = (new_pos[i] + sum(d for row, d in shifts[b] if row < i)) & U64
    # a request's own failure, else its stream's status (a row that failed its check is recorded with the stream only)
    req_status = [k["status"] if k["status"] != O.OK else status[rs[r]] for r, k in enumerate(pl)]
    result[1], result[3] = sum(out_len), sum(1 for x in new if x is not None)
    return dict(status=status, out_len=out_len, streams=new, req_status=req_status, new_pos=new_pos, out_bound=bound, result=result, dirty=dirty)


def patched(raw: bytes, reqs, srcs, b: int) -> bytes:
    """What stream b decodes to after its requests."""
    a = bytearray(raw)
    for (sb, off, ln), src in zip(reqs, srcs):
        if sb == b:
            a[off:off + ln] = src
    return bytes(a)


def request_shapes(n: int, cb: int):
    """Lists of (off, len), each list sorted and disjoint, over a stream of n decoded bytes in chunks of cb: inside one chunk, exactly one chunk,
    head edge + interiors + tail edge, two and three requests in one chunk, two requests sharing an edge chunk, the last byte, the whole
    stream, a zero-length request."""
    def fit(lst):
        out = []
        for off, ln in lst:
            off = min(off, n)
            ln = min(ln, n - off)
            if not out or out[-1][0] + out[-1][1] <= off:
                out.append((off, ln))
        return out

    h = max(cb // 2, 1)
    shapes = [[(cb // 3, h)], [(cb, cb)], [(h, 2 * cb + 1)], [(cb + 1, max(cb // 4, 1)), (cb + 1 + h, 1)],
              [(0, 1), (cb // 3 + 1, max(cb // 4, 1)), (cb - 1, 1)], [(1, cb + h - 1), (cb + h, cb)], [(max(n - 1, 0), 1)], [(0, n)],
              [(min(cb, n), 0)], [(0, 0), (0, min(n, 2)), (min(n, 2), 0)]]
    return [fit(x) for x in shapes]


# ---- requests and indexes the CPU and the GPU tests share ---------------------------------------------------------------------------------------
def fresh(rng, n: int) -> bytes:
    """New bytes for a request: half of them compressible."""
    half = n // 2
    return bytes(rng.integers(0, 256, n - half, dtype=np.uint8)) + b"ab" * (half // 2) + b"c" * (half % 2)


def row_requests(s: bytes):
    """Request lists for a foreign stream, from its walk: inside one chunk, exactly one chunk, across the chunk's neighbours, the last byte, the
    whole stream, a zero-length request -- around the middle one of its non-empty chunks."""
    rows, total, _, _ = R.walk(s)
    full = [r for r in rows if r[5] > 0]
    if not full or total == 0:
        return [[(0, 0)]]
    m = full[len(full) // 2]
    a, d = m[4], m[5]
    lists = [[(a + (d > 2), max(d - 2, 1))], [(a, d)], [(max(a - 1, 0), min(d + 2, total - max(a - 1, 0)))], [(total - 1, 1)], [(0, total)],
             [(a, 0)], [(a, 1), (a + d - 1, 1)] if d > 1 else [(a, 1)]]
    return lists


def unsound_indexes(ix, streams, rng):
    """The twelve unsound indexes of the indexed read's check, plus rows that point at one header twice."""
    ns, ne = len(streams), len(ix["start"])
    lens = [len(s) for s in streams]

    def rnd(n, hi=1 << 64):
        return [int(v) % hi for v in rng.integers(0, 1 << 63, n, dtype=np.uint64) * 2 + rng.integers(0, 2, n, dtype=np.uint64)]

    twice = list(ix["pos"])
    for i in range(1, ne, 3):
        twice[i] = twice[i - 1]
    return [{**ix, "start": rnd(ne), "pos": rnd(ne)},
            {**ix, "first": rnd(ns + 1), "total": rnd(ns), "start": rnd(ne), "pos": rnd(ne)},
            {**ix, "start": rnd(ne, 1 << 17), "pos": rnd(ne, 1 << 12), "total": rnd(ns, 1 << 18)},
            {**ix, "first": [f + (1 << 33) * (i % 2) for i, f in enumerate(ix["first"])]},
            {**ix, "first": list(reversed(ix["first"]))},
            {**ix, "pos": [p + lens[i % ns] for i, p in enumerate(ix["pos"])]},
            {**ix, "pos": [max(lens) - 1 - (i % 20) for i in range(ne)]},
            {**ix, "start": list(reversed(ix["start"]))},
            {**ix, "start": [v ^ ((i % 3 == 0) << 9) for i, v in enumerate(ix["start"])]},
            {**ix, "tail": [int(v) % 40 - 20 for v in rng.integers(0, 1000, ns)]},
            {**ix, "start": ix["start"][:ne // 2], "pos": ix["pos"][:ne // 2]},
            {**ix, "start": [], "pos": []},
            {**ix, "pos": twice}]


def sound_lists(streams, ix):
    """One sorted request list over the whole batch: per updatable stream an edge pair around its middle chunk and a request sharing its tail."""
    reqs = []
    for b, s in enumerate(streams):
        if ix["tail"][b] != O.OK or not ix["total"][b]:
            continue
        rows = [r for r in R.walk(s)[0] if 0 < r[5] <= 65536]
        if len(rows) < 2 or any(r[5] > 65536 for r in R.walk(s)[0]):
            reqs.append((b, 0, 1))
            continue
        m = rows[len(rows) // 2]
        reqs += [(b, max(m[4] - 1, 0), 2), (b, m[4] + 1, max(m[5] - 1, 0)), (b, ix["total"][b], 0)]
    return reqs


# ---- the cases of the planning check (tests/abi/frame_update_plan_check.hip) ---------------------------------------------------------------------
def plan_lines(ix, streams, reqs):
    """What the planning header must give for a request list, one line per request, as the check program prints them."""
    out = []
    for k in planned(ix, streams, reqs):
        out.append("%d %d %d %d %d %d %d %d %d" % (k["status"], k["r0"], k["r1"], k["head"], k["last"], k["own0"], k["cnt"], k["bytes"], k["bad"]))
    return out


def write_cases(path: str, streams, cases):
    """The input of the check program: the streams, then every case -- an index (any lists at all) and its request list (stream, off, len)."""
    with open(path, "wb") as f:
        f.write(struct.pack("<Q", len(streams)))
        for s in streams:
            f.write(struct.pack("<Q", len(s)))
            f.write(s)
        f.write(struct.pack("<Q", len(cases)))
        for ix, reqs in cases:
            ne = min(len(ix["start"]), len(ix["pos"]))
            f.write(struct.pack("<Q", ne))
            for key, n in (("first", len(streams) + 1), ("total", len(streams)), ("tail", len(streams)), ("start", ne), ("pos", ne)):
                assert len(ix[key]) >= n
                f.write(struct.pack("<%dQ" % n, *[int(v) & U64 for v in ix[key][:n]]))
            f.write(struct.pack("<Q", len(reqs)))
            for b, off, ln in reqs:
                f.write(struct.pack("<3Q", b, off & U64, ln & U64))

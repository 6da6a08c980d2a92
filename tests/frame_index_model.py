"""Pure-Python statement of include/snappier_hip_frame_index.h: the chunk index of a batch of framed streams (snp_frame_index_batch: rows, totals,
tails, the in-order admission by max_spans / max_entries, d_result) and the indexed read (snp_frame_read_indexed_batch: the clip, the two
binary searches, head / interior / tail, the check of every row against the header it points at -- the index is untrusted input -- the
in-order admission by max_chunks / edge_cap, the verdict and d_result).  The planning half is a transliteration of csrc/frame_index_device.h,
search for search, so that it also says what that header does with an index filled with anything at all; built on the walk, the hop and the
chunk status of frame_range_model.py / frame_buffers_model.py, which also provide the streams and windows the CPU and the GPU tests share."""
import struct

import decode_layout_model as L
import frame_buffers_model as M
import frame_range_model as R
import oracle as O

U64 = R.U64
SPAN = R.SPAN


# ---- the streams every test of the indexed calls uses ----------------------------------------------------------------------------------------
def named_streams():
    """name -> framed stream: the contract's constructed cases, the long two-span stream, tiny foreign chunks, zero-length chunks, a chunk
    above 65536 bytes and a short stream of the project's own encoder.  The largest is 1.4 MB."""
    return {**L.stream_cases(), "long_two_spans": R.long_stream_with_a_skippable_chunk_across_the_span_boundary()[0],
            "tiny_chunks": R.tiny_chunk_stream(1)[0], "zero_length_chunks": R.zero_length_chunk_stream()[0], "big_chunk": R.big_chunk_stream()[0],
            "uniform_5": R.uniform_stream(5, last=777)[0]}


def all_windows(streams):
    """(stream number, range_off, range_len) for every window of R.windows over every stream."""
    out = []
    for b, s in enumerate(streams):
        rows, total, _, _ = R.walk(s)
        out += [(b, ro, rl) for ro, rl in R.windows(rows, total)]
    return out


# ---- the index -------------------------------------------------------------------------------------------------------------------------------
def index_of(s: bytes):
    """One stream's index from its walk: -> (start list, pos list (header positions, stream-relative), total, tail)."""
    rows, total, tail, _ = R.walk(s)
    return [r[4] for r in rows], [r[1] - 8 for r in rows], total, tail


def build_index(streams, max_spans: int | None = None, max_entries: int | None = None):
    """snp_frame_index_batch over a batch: -> dict of first, start, pos, total, tail (lists) and result [4].  None: a bound that admits all."""
    ns = len(streams)
    max_spans = 1 << 62 if max_spans is None else max_spans
    max_entries = 1 << 62 if max_entries is None else max_entries
    ix = {"first": [0], "start": [], "pos": [], "total": [], "tail": []}
    spans = need = missed = 0
    for s in streams:
        spans += (len(s) + SPAN - 1) // SPAN
        walked = spans <= max_spans
        if walked:
            start, pos, total, tail = index_of(s)
            need += len(start)
            missed += R.walk(s)[3]
        if walked and need <= max_entries:
            ix["start"] += start
            ix["pos"] += pos
            ix["total"].append(total)
            ix["tail"].append(tail)
        else:
            ix["total"].append(0)
            ix["tail"].append(O.ERR_OUTPUT_TOO_SMALL)
        ix["first"].append(len(ix["start"]))
    ix["result"] = [need, sum(ix["total"]), spans, missed]
    assert len(ix["first"]) == ns + 1
    return ix


# ---- one request's plan (csrc/frame_index_device.h) ------------------------------------------------------------------------------------------
def first_where(a: int, b: int, pred) -> int:
    """ix_first_where: the same probes in the same order, so that an unsound index gives the same answer."""
    while a < b:
        mid = a + (b - a) // 2
        if pred(mid):
            b = mid
        else:
            a = mid + 1
    return a


def row_end(ix, f1: int, total: int, i: int) -> int:
    return ix["start"][i + 1] if i + 1 < f1 else total


def plan(ix, ns: int, b: int, req_off: int, req_len: int, cap: int):
    """ix_plan: -> dict of status, tail, small, head, last, lo, hi, r0, r1, f1, total."""
    k = dict(status=O.ERR_BAD_ARG, tail=0, small=False, head=False, last=False, lo=0, hi=0, r0=0, r1=0, f1=0, total=0)
    if b >= ns:
        return k
    k["tail"] = ix["tail"][b]
    if k["tail"] == O.ERR_OUTPUT_TOO_SMALL:
        k["status"] = O.ERR_OUTPUT_TOO_SMALL
        return k
    if k["tail"] < O.OK or k["tail"] > O.ERR_TRUNCATED_STREAM:
        return k
    nentries = min(len(ix["start"]), len(ix["pos"]))
    f0, f1 = min(ix["first"][b], nentries), min(ix["first"][b + 1], nentries)
    if f1 < f0:
        return k
    total = ix["total"][b]
    lo, hi = R.clip(total, req_off, req_len)
    k.update(lo=lo, hi=hi, f1=f1, total=total, r0=f0, r1=f0, small=hi - lo > cap)
    if k["small"]:
        k["status"] = O.OK
        return k
    i0 = first_where(f0, f1, lambda i: row_end(ix, f1, total, i) > lo)
    i1 = first_where(f0, f1, lambda i: ix["start"][i] >= hi)
    k.update(r0=i0, r1=max(i0, i1))
    if k["r0"] == k["r1"]:
        if hi <= lo:
            k["status"] = O.OK
        return k
    s0, e1 = ix["start"][k["r0"]], row_end(ix, f1, total, k["r1"] - 1)
    if s0 > lo or e1 < hi:
        return k
    k["head"] = s0 < lo
    k["last"] = e1 > hi and not (k["head"] and k["r1"] - 1 == k["r0"])
    k["status"] = O.OK
    return k


def row_check(ix, s: bytes, k, i: int, interior: bool):
    """ix_row_check: -> the row as the chunk table takes it (type, body_off, body_len, crc, start, dec), or None."""
    start, end, pos = ix["start"][i], row_end(ix, k["f1"], k["total"], i), ix["pos"][i]
    if end < start or pos >= len(s):
        return None
    h = M.hop(s, pos)
    if h.kind != "data" or end - start != h.dec:
        return None
    if interior and not (start >= k["lo"] and end <= k["hi"]):
        return None
    return (h.type, pos + 8, h.body_len, h.crc, start, h.dec)


def planned(ix, streams, b: int, req_off: int, req_len: int, cap: int):
    """The plan kernel for one request: ix_plan, then the check of its edge rows.  -> (plan, head row, tail row, interior count, edge bytes)."""
    k = plan(ix, len(streams), b, req_off, req_len, cap)
    head = tail = None
    if k["status"] == O.OK and k["r0"] < k["r1"]:
        s = streams[b]
        head = row_check(ix, s, k, k["r0"], False) if k["head"] else None
        tail = row_check(ix, s, k, k["r1"] - 1, False) if k["last"] and not (k["head"] and head is None) else None
        if (k["head"] and head is None) or (k["last"] and tail is None):
            k["status"] = O.ERR_BAD_ARG
            return k, None, None, 0, 0
        return k, head, tail, k["r1"] - k["r0"] - k["head"] - k["last"], sum(r[5] for r in (head, tail) if r)
    return k, None, None, 0, 0


def interior_rows(ix, s: bytes, k):
    """The checked interior rows of a planned request, in order; None in place of one that fails its check."""
    first = k["r0"] + k["head"]
    n = k["r1"] - k["r0"] - k["head"] - k["last"]
    return [row_check(ix, s, k, i, True) if i < k["f1"] else None for i in range(first, first + n)]


# ---- the whole read --------------------------------------------------------------------------------------------------------------------------
def read_plan(streams, ix, requests, caps, max_chunks: int, edge_cap: int):
    """snp_frame_read_indexed_batch.  requests: (stream number, req_off, req_len).
    -> (status list, out_len list, bytes per request (None unless OK), d_result [4])."""
    nreq = len(requests)
    status, out_len, data = [O.ERR_OUTPUT_TOO_SMALL] * nreq, [0] * nreq, [None] * nreq
    slots = edge_bytes = 0
    for r, (b, ro, rl) in enumerate(requests):
        k, head, tail, cnt, ebytes = planned(ix, streams, b, ro, rl, caps[r])
        slots += cnt
        edge_bytes += ebytes
        if slots > max_chunks or edge_bytes > edge_cap:
            continue                                                    # not admitted (the sums only grow: nor is any later request)
        if k["status"] != O.OK:
            status[r] = k["status"]
            continue
        s = streams[b]
        inner = interior_rows(ix, s, k)
        if any(x is None for x in inner):
            status[r] = O.ERR_BAD_ARG                                   # nothing of it is decoded
            continue
        sel = [x for x in ([head] if head else []) + inner + ([tail] if tail else []) if x[5] > 0]    # a zero-length row is never decoded
        st = int(M.verdict(s, sel, 0, k["tail"])[0])
        if st == O.OK and k["small"]:
            st = O.ERR_OUTPUT_TOO_SMALL
        status[r] = st
        if st == O.OK:
            lo, hi = k["lo"], k["hi"]
            data[r] = b"".join(R.chunk_result(s, x)[1][max(x[4], lo) - x[4]:max(min(x[4] + x[5], hi), max(x[4], lo)) - x[4]] for x in sel)
            out_len[r] = hi - lo
    return status, out_len, data, [slots, sum(out_len), edge_bytes, sum(1 for x in status if x == O.OK)]


def read_needs(streams, ix, requests, caps):
    """-> (max_chunks, edge_cap) that admit every request."""
    res = read_plan(streams, ix, requests, caps, 0, 0)[3]
    return res[0], res[2]


# ---- the cases of the planning check (tests/abi/frame_index_plan_check.hip) ----------------------------------------------------------------------
def plan_line(ix, streams, request, cap):
    """What the planning header must give for one request, as the check program prints it."""
    b, ro, rl = request
    k, head, tail, cnt, ebytes = planned(ix, streams, b, ro, rl, cap)
    bad = 0
    if k["status"] == O.OK:
        bad = sum(1 for x in interior_rows(ix, streams[b], k) if x is None)
    ok = k["status"] == O.OK
    return "%d %d %d %d %d %d %d %d %d %d" % (k["status"], k["lo"] if ok else 0, k["hi"] if ok else 0, k["r0"] if ok else 0, k["r1"] if ok else 0, int(k["head"] and ok),
                                              int(k["last"] and ok), cnt, ebytes, bad)


def write_cases(path: str, streams, cases):
    """The input of the check program: the streams, then every case -- an index (any lists at all) and its requests (stream, off, len, cap)."""
    with open(path, "wb") as f:
        f.write(struct.pack("<Q", len(streams)))
        for s in streams:
            f.write(struct.pack("<Q", len(s)))
            f.write(s)
        f.write(struct.pack("<Q", len(cases)))
        for ix, requests in cases:
            ne = min(len(ix["start"]), len(ix["pos"]))
            f.write(struct.pack("<Q", ne))
            for key, n in (("first", len(streams) + 1), ("total", len(streams)), ("tail", len(streams)), ("start", ne), ("pos", ne)):
                assert len(ix[key]) >= n
                f.write(struct.pack("<%dQ" % n, *[int(v) & U64 for v in ix[key][:n]]))
            f.write(struct.pack("<Q", len(requests)))
            for b, ro, rl, cap in requests:
                f.write(struct.pack("<4Q", b, ro & U64, rl & U64, cap & U64))

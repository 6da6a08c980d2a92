"""Pure-Python statement of include/snappier_hip_frame_find.h (snp_frame_find_indexed_batch): per request the rows and bytes it needs (from the
indexed read's plan: frame_index_model.plan), the two-bound admission in request order with its saturating sums, the status (what the indexed
read's model, frame_index_model.read_plan, gives for the same window with a capacity that holds it and bounds that admit it), d_result, and
win_len, count and hits by a plain bytes.find loop over the oracle's decode of the window.  Nothing of the read is restated here.  Also states
the tile arithmetic of csrc/frame_find_device.h (fd_starts, fd_tiles, fd_tile) for the planning check.  The CPU and the GPU tests share it."""
import os
import re

import frame_index_model as X
import frame_range_model as R
import oracle as O

U64 = R.U64
MAX_NEEDLE = 256
ROW_CLAMP = 1 << 31                                                     # a request's rows count as no more than this
CAP_MAX = (1 << 40) - 1                                                 # scratch_cap counts as no more than this
_HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "snappier_amd", "csrc", "frame_find_device.h")
TILE = int(re.search(r"constexpr u32 kFindTile = (\d+);", open(_HEADER).read()).group(1))


# ---- the ground truth --------------------------------------------------------------------------------------------------------------------------
def occurrences(data: bytes, needle: bytes):
    """Every offset at which needle occurs in data, overlapping ones included, ascending."""
    out, p = [], data.find(needle)
    while p >= 0:
        out.append(p)
        p = data.find(needle, p + 1)
    return out


def window_bytes(s: bytes, off: int, ln: int):
    """-> (lo, what the oracle decodes of a stream, clipped like a request)."""
    data = O.frame_decode(s)
    lo, hi = R.clip(len(data), off, ln)
    return lo, data[lo:hi]


def truth(s: bytes, off: int, ln: int, needle: bytes, cap: int):
    """-> (win_len, count, hits) of an OK request, the hits as offsets into what the stream decodes to."""
    lo, data = window_bytes(s, off, ln)
    occ = occurrences(data, needle)
    return len(data), len(occ), [lo + p for p in occ[:cap]]


# ---- one request's needs (fd_plan) -------------------------------------------------------------------------------------------------------------
def per_request(needles, nreq: int):
    """One needle for all requests, or one per request."""
    return [needles] * nreq if isinstance(needles, (bytes, bytearray)) else list(needles)


def needs_of(ix, ns: int, request, m: int):
    """-> (plan status, rows, bytes): what the request adds to the two sums.  A needle length that is not legal, a refused plan and a window
    that owns no row add nothing; the bytes are where the last owned row ends minus where the first begins."""
    if m == 0 or m > MAX_NEEDLE:
        return O.ERR_BAD_ARG, 0, 0
    b, ro, rl = request
    k = X.plan(ix, ns, b, ro, rl, U64)
    if k["status"] != O.OK or k["r0"] >= k["r1"]:
        return k["status"], 0, 0
    return O.OK, k["r1"] - k["r0"], X.row_end(ix, k["f1"], k["total"], k["r1"] - 1) - ix["start"][k["r0"]]


# ---- the whole call ----------------------------------------------------------------------------------------------------------------------------
def find_plan(streams, ix, requests, needles, hit_caps, max_rows: int, scratch_cap: int):
    """snp_frame_find_indexed_batch.  requests: (stream number, req_off, req_len); needles: bytes, or one per request.
    -> (status, win_len, count, nhits lists, hits per request (a list each), d_result [4])."""
    nreq = len(requests)
    needles = per_request(needles, nreq)
    status = [O.ERR_OUTPUT_TOO_SMALL] * nreq
    win_len, count, nhits, hits = [0] * nreq, [0] * nreq, [0] * nreq, [[] for _ in range(nreq)]
    rows = scratch = 0
    cap = min(scratch_cap, CAP_MAX)
    for r, q in enumerate(requests):
        m = len(needles[r])
        planned, nrows, nbytes = needs_of(ix, len(streams), q, m)
        rows += min(nrows, ROW_CLAMP)
        scratch = min(scratch + nbytes, U64)
        if rows > max_rows or scratch > cap:
            continue                                                    # not admitted (the sums only grow: nor is any later request)
        if m == 0 or m > MAX_NEEDLE:
            status[r] = O.ERR_BAD_ARG
            continue
        st, _, data, _ = X.read_plan(streams, ix, [q], [U64], 1 << 62, 1 << 62)
        status[r] = st[0]
        if st[0] != O.OK:
            continue
        assert planned == O.OK
        lo = R.clip(ix["total"][q[0]], q[1], q[2])[0]
        occ = occurrences(data[0], needles[r])
        win_len[r], count[r], nhits[r] = len(data[0]), len(occ), min(len(occ), hit_caps[r])
        hits[r] = [lo + p for p in occ[:hit_caps[r]]]
    return status, win_len, count, nhits, hits, [rows, sum(count), scratch, sum(1 for x in status if x == O.OK)]


def needs(streams, ix, requests, needles):
    """-> (max_rows, scratch_cap) that admit every request: the one sizing round."""
    res = find_plan(streams, ix, requests, needles, [0] * len(requests), 0, 0)[5]
    return res[0], res[2]


# ---- the tiles (fd_starts, fd_tiles, fd_tile) -----------------------------------------------------------------------------------------------------
def starts_of(n: int, m: int) -> int:
    return n - m + 1 if n >= m else 0


def tiles_of(starts: int) -> int:
    return (starts + TILE - 1) // TILE


def tile(lo: int, starts: int, t: int):
    """-> (first, end): the start positions of tile t of a window that begins at lo."""
    return lo + t * TILE, lo + min((t + 1) * TILE, starts)


# ---- the cases of the planning check (tests/abi/frame_find_plan_check.hip) -------------------------------------------------------------------------
def plan_line(ix, streams, request, m: int) -> str:
    """What the planning header must give for one request, as the check program prints it: status rows bytes, and when the plan is OK the
    start positions, the tiles, the first tile's and the last tile's first and end, and the owned rows that fail fd_row's check."""
    st, rows, nbytes = needs_of(ix, len(streams), request, m)
    out = [st, rows, nbytes & U64]
    if st == O.OK:
        b, ro, rl = request
        k = X.plan(ix, len(streams), b, ro, rl, U64)
        starts = starts_of(k["hi"] - k["lo"], m)
        nt = tiles_of(starts)
        out += [starts, nt, *(tile(k["lo"], starts, 0) if nt else (0, 0)), *(tile(k["lo"], starts, nt - 1) if nt else (0, 0))]
        bad = 0
        for i in range(k["r0"], k["r1"]):
            edge = (k["head"] and i == k["r0"]) or (k["last"] and i == k["r1"] - 1)
            bad += i >= k["f1"] or X.row_check(ix, streams[b], k, i, not edge) is None
        out.append(bad)
    return " ".join(map(str, out))


def write_cases(path: str, streams, cases):
    """The input of the check program: the streams, then every case -- an index (any lists at all) and its requests (stream, off, len, m)."""
    X.write_cases(path, streams, cases)


def pack_needles(needles):
    """-> (one buffer, needle_off, needle_len): the needles one after the other (an empty buffer still has one byte)."""
    off, at = [], 0
    for n in needles:
        off.append(at)
        at += len(n)
    return b"".join(needles) or b"\0", off, [len(n) for n in needles]


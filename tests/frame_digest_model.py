"""Pure-Python statement of include/snappier_hip_frame_digest.h: the CRC-32C combine (csrc/frame_digest_device.h: the GF(2) multiply on reflected
values, the table of x^(8 * 2^k), crc_shift, the combine) and the batch digest (snp_frame_digest_indexed_batch: per request the indexed read's
plan with no capacity, the check of every owned row, the in-order admission by edge_cap, the read's verdict over the EDGES alone -- an
interior row is never decoded -- the digest, dig_len and d_result).  Built on frame_index_model.py (the plan and the row check are the read's,
imported, not restated) and on the oracle's CRC-32C; the CPU and the GPU tests share it."""
import struct

import frame_buffers_model as M
import frame_index_model as X
import frame_range_model as R
import oracle as O

U64 = R.U64
POLY = 0x82F63B78
MASK_DELTA = 0xA282EAD8


# ---- the arithmetic ----------------------------------------------------------------------------------------------------------------------------
def gf2_mul(a: int, b: int) -> int:
    """a * b mod P on reflected 32-bit values (bit 31 is x^0)."""
    p = 0
    for i in range(32):
        if a & (0x80000000 >> i):
            p ^= b
        b = (b >> 1) ^ (POLY if b & 1 else 0)
    return p


def _table():
    t, v = [], 0x00800000                                               # x^8
    for _ in range(64):
        t.append(v)
        v = gf2_mul(v, v)
    return t


SHIFT = _table()                                                        # x^(8 * 2^k), k = 0 .. 63


def crc_shift(c: int, n: int) -> int:
    """c * x^(8n) mod P: the CRC register after n more zero bytes; any n below 2^64."""
    assert 0 <= n <= U64
    k = 0
    while n:
        if n & 1:
            c = gf2_mul(SHIFT[k], c)
        n >>= 1
        k += 1
    return c


def crc_combine(crc_a: int, crc_b: int, len_b: int) -> int:
    """Plain CRC-32C of A || B from the plain CRCs of A and B and B's length."""
    return crc_shift(crc_a, len_b) ^ crc_b


def crc_unmask(m: int) -> int:
    r = (m - MASK_DELTA) & 0xFFFFFFFF
    return ((r << 15) | (r >> 17)) & 0xFFFFFFFF


def combine_all(pieces) -> int:
    """The digest formula over pieces (crc, length) in order: XOR_i shift(crc_i, bytes behind piece i)."""
    behind, dg = 0, 0
    for crc, n in reversed(list(pieces)):
        dg ^= crc_shift(crc, behind)
        behind += n
    return dg


def repeat_digest(crc: int, length: int, count: int) -> int:
    """The digest of `count` copies of one piece (crc, length) in a row, by doubling: O(log count) combines."""
    dg, n = 0, 0                                                        # the digest of the first n copies
    for bit in reversed(range(count.bit_length())):
        dg = crc_combine(dg, dg, n * length)                            # n -> 2n
        n *= 2
        if (count >> bit) & 1:
            dg = crc_combine(dg, crc, length)                           # -> 2n + 1
            n += 1
    assert n == count
    return dg


# ---- one request -------------------------------------------------------------------------------------------------------------------------------
def request_plan(ix, streams, b: int, req_off: int, req_len: int):
    """-> (plan, head row, tail row, interior rows (None in place of one that fails its check), edge bytes): the read's plan, capacity unbounded."""
    k, head, tail, cnt, ebytes = X.planned(ix, streams, b, req_off, req_len, U64)
    inner = X.interior_rows(ix, streams[b], k) if k["status"] == O.OK else []
    assert len(inner) == cnt
    return k, head, tail, inner, ebytes


def interior_term(k, row) -> int:
    """What a checked interior row adds: nothing if it is empty (its header CRC is not looked at), else its header's CRC shifted over hi - end."""
    _, _, _, crc, start, dec = row
    return crc_shift(crc_unmask(crc), k["hi"] - (start + dec)) if dec else 0


def digest_plan(streams, ix, requests, edge_cap: int):
    """snp_frame_digest_indexed_batch.  requests: (stream number, req_off, req_len).
    -> (status list, dig_len list, digest list, d_result [4])."""
    nreq = len(requests)
    status, dig_len, digest = [O.ERR_OUTPUT_TOO_SMALL] * nreq, [0] * nreq, [0] * nreq
    edge_bytes = rows = 0
    for r, (b, ro, rl) in enumerate(requests):
        if b >= len(streams):
            k, head, tail, inner, ebytes = X.plan(ix, len(streams), b, ro, rl, U64), None, None, [], 0
        else:
            k, head, tail, inner, ebytes = request_plan(ix, streams, b, ro, rl)
        edge_bytes += ebytes
        if edge_bytes > edge_cap:
            continue                                                    # not admitted (the sum only grows: nor is any later request)
        if k["status"] != O.OK:
            status[r] = k["status"]
            continue
        if any(x is None for x in inner):
            status[r] = O.ERR_BAD_ARG
            continue
        s = streams[b]
        edges = [x for x in (head, tail) if x and x[5] > 0]
        st = int(M.verdict(s, edges, 0, k["tail"])[0])                  # only the edges are decoded and verified
        status[r] = st
        if st != O.OK:
            continue
        lo, hi = k["lo"], k["hi"]
        dg = 0
        for x in inner:
            dg ^= interior_term(k, x)
        for x in edges:
            start, dec = x[4], x[5]
            frm, to = max(start, lo), min(start + dec, hi)
            to = max(to, frm)
            dg ^= crc_shift(O.crc32c(R.chunk_result(s, x)[1][frm - start:to - start], masked=False), hi - to)
        digest[r], dig_len[r] = dg, hi - lo
        rows += len(inner)
    return status, dig_len, digest, [rows, sum(dig_len), edge_bytes, sum(1 for x in status if x == O.OK)]


def edge_need(streams, ix, requests) -> int:
    """-> the edge_cap that admits every request."""
    return digest_plan(streams, ix, requests, 0)[3][2]


# ---- the cases of the planning check (tests/abi/frame_digest_plan_check.hip) ---------------------------------------------------------------------
def plan_line(ix, streams, request) -> str:
    """What the planning header must give for one request, as the check program prints it."""
    b, ro, rl = request
    if b >= len(streams):
        return "%d 0 0 0 0 0 0" % X.plan(ix, len(streams), b, ro, rl, U64)["status"]
    k, head, tail, inner, ebytes = request_plan(ix, streams, b, ro, rl)
    ok = k["status"] == O.OK
    bad = sum(1 for x in inner if x is None)
    dg = 0
    if ok and not bad:
        for x in inner:
            dg ^= interior_term(k, x)
    return "%d %d %d %d %d %d %d" % (k["status"], k["lo"] if ok else 0, k["hi"] if ok else 0, len(inner), ebytes, bad, dg)


def write_shifts(path: str, pairs):
    """The first input of the check program: (crc, byte count) pairs."""
    with open(path, "wb") as f:
        f.write(struct.pack("<Q", len(pairs)))
        for c, n in pairs:
            f.write(struct.pack("<2Q", c, n))

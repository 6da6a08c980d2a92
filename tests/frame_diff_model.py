"""Pure-Python statement of include/snappier_hip_frame_diff.h (snp_frame_diff_indexed_batch): per request the indexed read's plan of both sides,
the check of every owned row, the common cuts, the header CRC of every span between two of them, the pieces that are decoded and compared byte
for byte, the two-bound admission, the statuses and d_result.  The planning half is a transliteration of csrc/frame_diff_device.h, search for
search, so that it also says what that header does with an index filled with anything at all.  Built on frame_index_model.py (plan and row
check are the read's, imported, not restated) and frame_digest_model.py (the CRC arithmetic); also gives the ground truth by plain byte
comparison of the oracle's decodes.  The CPU and the GPU tests share it."""
import functools
import struct

import frame_buffers_model as M
import frame_digest_model as D
import frame_index_model as X
import frame_range_model as R
import oracle as O

U64 = R.U64
PREFIX, SUFFIX, EXACT = 1, 2, 4
NONE = U64                                                              # no mismatch found


@functools.lru_cache(maxsize=None)
def _shift_tables(k: int):
    """Multiplication by x^(8 * 2^k) as four 256-entry tables, one per byte of the CRC (the product is linear in the CRC's bits)."""
    basis = [D.gf2_mul(D.SHIFT[k], 1 << i) for i in range(32)]
    tabs = []
    for j in range(4):
        t = [0] * 256
        for v in range(1, 256):
            low = v & -v
            t[v] = t[v ^ low] ^ basis[8 * j + low.bit_length() - 1]
        tabs.append(t)
    return tabs


def crc_shift(c: int, n: int) -> int:
    """D.crc_shift, by table look-ups (the models of long streams shift once per chunk)."""
    k = 0
    while n:
        if n & 1:
            t = _shift_tables(k)
            c = t[0][c & 0xFF] ^ t[1][(c >> 8) & 0xFF] ^ t[2][(c >> 16) & 0xFF] ^ t[3][c >> 24]
        n >>= 1
        k += 1
    return c


# ---- the ground truth --------------------------------------------------------------------------------------------------------------------------
def common_prefix(a: bytes, b: bytes) -> int:
    n = min(len(a), len(b))
    if a[:n] == b[:n]:
        return n
    lo, hi = 0, n                                                       # a[:lo] == b[:lo], a[:hi] != b[:hi]
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if a[:mid] == b[:mid]:
            lo = mid
        else:
            hi = mid
    return lo


def truth(a: bytes, b: bytes, flags: int):
    """-> (prefix, suffix) of two windows' bytes as the header defines them."""
    n = min(len(a), len(b))
    p = common_prefix(a, b) if flags & PREFIX else 0
    s = common_prefix(a[::-1], b[::-1]) if flags & SUFFIX else 0
    if flags & PREFIX:
        s = min(s, n - p)
    return p, s


# ---- one side of one request (DfSide) ------------------------------------------------------------------------------------------------------------
class Side:
    """A batch of streams with its index, and per stream a cache of the hops its index rows point at."""

    def __init__(self, streams, ix):
        self.streams, self.ix = streams, ix
        self._rows, self._scans = {}, {}

    def plan(self, b: int, off: int, ln: int):
        return X.plan(self.ix, len(self.streams), b, off, ln, U64)

    def row(self, b: int, k, i: int, interior: bool):
        """ix_row_check, cached on everything it depends on but the window."""
        key = (b, i, k["f1"], k["total"])
        if key not in self._rows:
            wide = dict(k, lo=0, hi=U64)
            self._rows[key] = X.row_check(self.ix, self.streams[b], wide, i, False)
        row = self._rows[key]
        if row is not None and interior and not (row[4] >= k["lo"] and row[4] + row[5] <= k["hi"]):
            return None
        return row


class Req:
    """DfSide: one side of one request."""

    def __init__(self, side: Side, b: int, off: int, ln: int):
        self.side, self.b, self.k = side, b, side.plan(b, off, ln)
        self.ok = self.k["status"] == O.OK
        self.rows = self.k["r1"] - self.k["r0"] if self.ok else 0
        self.len = self.k["hi"] - self.k["lo"] if self.ok else 0

    def start(self, i):
        return self.side.ix["start"][i]

    def end(self, i):
        return X.row_end(self.side.ix, self.k["f1"], self.k["total"], i)


def df_row(q: Req, d: int, n: int, o: int, terms: bool):
    """-> (ok, full, tlo, thi, term)"""
    k = q.k
    i = k["r1"] - 1 - o if d else k["r0"] + o
    edge = (k["head"] and i == k["r0"]) or (k["last"] and i == k["r1"] - 1)
    row = q.side.row(q.b, k, i, not edge) if i < k["f1"] else None
    if row is None:
        return False, False, 0, 0, 0
    st, en = q.start(i), q.end(i)
    tlo = (k["hi"] - en if d else st - k["lo"]) & U64
    thi = (k["hi"] - st if d else en - k["lo"]) & U64
    full = st >= k["lo"] and en <= k["hi"] and thi <= n
    term = crc_shift(D.crc_unmask(row[3]), tlo if d else n - thi) if terms and full and row[5] else 0
    return True, full, tlo, thi, term


def df_cut(q: Req, d: int, t: int):
    """-> (found, ord)"""
    k = q.k
    if t > q.len or k["r0"] >= k["r1"]:
        return False, 0
    T = k["hi"] - t if d else k["lo"] + t
    j = X.first_where(k["r0"], k["r1"], lambda i: q.start(i) >= T)
    found = q.start(j) == T if j < k["r1"] else q.end(k["r1"] - 1) == T
    return found, (k["r1"] - j if d else j - k["r0"])


def df_need_rows(q: Req, d: int, n: int) -> int:
    k = q.k
    if n == 0 or k["r0"] >= k["r1"]:
        return 0
    if not d:
        return X.first_where(k["r0"], k["r1"], lambda i: q.start(i) >= k["lo"] + n) - k["r0"]
    return k["r1"] - X.first_where(k["r0"], k["r1"], lambda i: q.end(i) > k["hi"] - n)


def df_scan(a: Req, b: Req, d: int, n: int, cuts: bool):
    """df_scan_seq, once per pair of windows, direction and mode."""
    key = (id(b.side), a.b, a.k["lo"], a.k["hi"], a.k["status"], b.b, b.k["lo"], b.k["hi"], b.k["status"], d, cuts)
    if key not in a.side._scans:
        a.side._scans[key] = (b.side, _df_scan(a, b, d, n, cuts))       # (the other side is kept alive: its id stays its own)
    return a.side._scans[key][1]


def _df_scan(a: Req, b: Req, d: int, n: int, cuts: bool):
    """df_scan_seq -> dict(bad_a, bad_b, have0, diff, c0, prev, last, end): cuts are (t, ia, ib)."""
    s = dict(bad_a=False, bad_b=False, have0=False, diff=False, c0=None, prev=None, last=None, end=None, d0=0)

    def cut(c, dd):
        if not s["have0"]:
            s.update(have0=True, c0=c, last=c, d0=dd)
        elif dd != s["d0"]:
            s.update(diff=True, prev=s["last"], end=c)
        else:
            s["last"] = c

    gb, acc = [], 0
    for o in range(b.rows):
        ok, _, _, _, term = df_row(b, d, n, o, cuts)
        s["bad_b"] |= not ok
        gb.append(acc)
        acc ^= term
    gb.append(acc)
    if cuts and df_cut(a, d, 0)[0] and df_cut(b, d, 0)[0]:
        cut((0, 0, 0), 0)
    acc = 0
    for o in range(a.rows):
        ok, full, _, thi, term = df_row(a, d, n, o, cuts)
        s["bad_a"] |= not ok
        acc ^= term
        if cuts and not s["diff"] and ok and full:
            found, ob = df_cut(b, d, thi)
            if found:
                cut((thi, o + 1, ob), acc ^ gb[ob])
    return s


def df_pieces(s, need_a: int, need_b: int, n: int, exact: bool):
    """-> two pieces (a0, a1, b0, b1, t0, len)"""
    out = [(0, 0, 0, 0, n, 0), (0, 0, 0, 0, n, 0)]
    if n == 0:
        return out
    if exact or not s["have0"]:
        out[0] = (0, need_a, 0, need_b, 0, n)
        return out
    t, ia, ib = s["c0"]
    out[0] = (0, ia, 0, ib, 0, t) if t else (0, 0, 0, 0, 0, 0)
    if s["diff"]:
        (pt, pa, pb), (et, ea, eb) = s["prev"], s["end"]
        out[1] = (pa, ea, pb, eb, pt, et - pt)
    elif s["last"][0] < n:
        lt, la, lb = s["last"]
        out[1] = (la, max(need_a, la), lb, max(need_b, lb), lt, n - lt)
    return out


def df_piece_side(q: Req, d: int, o0: int, o1: int, t0: int, ln: int):
    """-> (good, row0, nrows, bytes, off)"""
    if o1 <= o0 or ln == 0:
        return ln == 0, 0, 0, 0, 0
    if o1 > q.rows:
        return False, 0, 0, 0, 0
    k = q.k
    i0 = k["r1"] - o1 if d else k["r0"] + o0
    i1 = i0 + (o1 - o0)
    s0, e1 = q.start(i0), q.end(i1 - 1)
    frm = k["hi"] - t0 - ln if d else k["lo"] + t0
    if e1 < s0 or frm < s0 or frm - s0 > e1 - s0 or ln > e1 - s0 - (frm - s0):
        return False, 0, 0, 0, 0
    return True, i0, i1 - i0, e1 - s0, frm - s0


# ---- one request ---------------------------------------------------------------------------------------------------------------------------------
class Analysis:
    """What the device knows of a request whose rows fit, before anything is decoded."""

    def __init__(self, a: Req, b: Req, flags: int):
        self.a, self.b, self.n = a, b, min(a.len, b.len)
        self.bad_a = self.bad_b = False
        self.pieces = {}                                                # (dir, k) -> dict(t0, len, sides: [(row0, nrows, bytes, off)] * 2, src)
        exact = bool(flags & EXACT)
        n = self.n
        good = True
        for d in (0, 1):
            if not flags & (PREFIX, SUFFIX)[d]:
                continue
            s = df_scan(a, b, d, n, not exact and n > 0)
            self.bad_a |= s["bad_a"]
            self.bad_b |= s["bad_b"]
            if s["bad_a"] or s["bad_b"]:
                continue
            for k, (a0, a1, b0, b1, t0, ln) in enumerate(df_pieces(s, df_need_rows(a, d, n), df_need_rows(b, d, n), n, exact)):
                ga, *sa = df_piece_side(a, d, a0, a1, t0, ln)
                gb, *sb = df_piece_side(b, d, b0, b1, t0, ln)
                good = good and ga and gb
                self.pieces[(d, k)] = dict(t0=t0, len=ln, sides=[tuple(sa), tuple(sb)], src=(d, k))
        if not good:
            self.bad_a = self.bad_b = True
        if self.bad_a or self.bad_b:
            self.pieces = {}
        if n and a.len == b.len and (0, 0) in self.pieces and (1, 0) in self.pieces:
            pk, sk = [next((k for k in (0, 1) if self.pieces[(d, k)]["len"] == n), None) for d in (0, 1)]
            if pk is not None and sk is not None:                       # the suffix compares what the prefix decoded
                s = self.pieces[(1, sk)]
                s["sides"] = [(0, 0, 0, x[3]) for x in s["sides"]]
                s["src"] = (0, pk)
        self.need = sum(max(x[2], x[1]) for pc in self.pieces.values() for x in pc["sides"])     # its bytes; a zero-length chunk costs one

    def decoded_rows(self, side: int):
        """The index rows this call decodes on a side, in stream order, as chunk table rows."""
        q = (self.a, self.b)[side]
        idx = sorted({i for pc in self.pieces.values() for i in range(pc["sides"][side][0], pc["sides"][side][0] + pc["sides"][side][1])})
        rows = [q.side.row(q.b, q.k, i, False) for i in idx]
        return [x for x in rows if x[5] > 0]

    def run(self, side: int, key):
        """The bytes of a piece's run on a side (every row decodes: the caller has checked the verdict)."""
        q = (self.a, self.b)[side]
        row0, nrows, _, _ = self.pieces[key]["sides"][side]
        rows = [q.side.row(q.b, q.k, i, False) for i in range(row0, row0 + nrows)]
        return b"".join(R.chunk_result(q.side.streams[q.b], x)[1] for x in rows if x[5] > 0)

    def answer(self, d: int) -> int:
        mis = []
        for k in (0, 1):
            pc = self.pieces[(d, k)]
            src = self.pieces[pc["src"]]
            ln = pc["len"]
            if ln == 0:
                mis.append(NONE)
                continue
            x = self.run(0, pc["src"])[src["sides"][0][3]:][:ln]
            y = self.run(1, pc["src"])[src["sides"][1][3]:][:ln]
            assert len(x) == ln and len(y) == ln
            m = common_prefix(x[::-1], y[::-1]) if d else common_prefix(x, y)
            mis.append(NONE if m == ln else m)
        t1, len1 = self.pieces[(d, 1)]["t0"], self.pieces[(d, 1)]["len"]
        return mis[0] if mis[0] != NONE else t1 + (mis[1] if mis[1] != NONE else len1)


def side_verdict(q: Req, bad: bool, rows) -> int:
    if not q.ok:
        return q.k["status"]
    if bad:
        return O.ERR_BAD_ARG
    return int(M.verdict(q.side.streams[q.b], rows, 0, q.k["tail"])[0])


def diff_plan(side_a: Side, side_b: Side, requests, flags: int, max_rows: int, scratch_cap: int):
    """snp_frame_diff_indexed_batch.  requests: (stream a, off a, len a, stream b, off b, len b).
    -> (status, len_a, len_b, prefix, suffix lists, d_result [4])."""
    assert flags & (PREFIX | SUFFIX) and not flags & ~(PREFIX | SUFFIX | EXACT)
    nreq = len(requests)
    status = [O.ERR_OUTPUT_TOO_SMALL] * nreq
    len_a, len_b, prefix, suffix = [0] * nreq, [0] * nreq, [0] * nreq, [0] * nreq
    rows = scratch = ok_n = 0
    for r, (ba, oa, la, bb, ob, lb) in enumerate(requests):
        a, b = Req(side_a, ba, oa, la), Req(side_b, bb, ob, lb)
        both = a.ok and b.ok
        rows += a.rows + b.rows if both else 0
        if rows > max_rows:
            continue                                                    # not admitted (the sum only grows: nor is any later request)
        an = Analysis(a, b, flags) if both else None
        scratch += an.need if an else 0
        if scratch > scratch_cap:
            continue
        st = side_verdict(a, an.bad_a if an else False, an.decoded_rows(0) if an else [])
        if st == O.OK:
            st = side_verdict(b, an.bad_b if an else False, an.decoded_rows(1) if an else [])
        status[r] = st
        if st != O.OK:
            continue
        n = an.n
        len_a[r], len_b[r] = a.len, b.len
        if flags & PREFIX:
            prefix[r] = an.answer(0)
        if flags & SUFFIX:
            suffix[r] = an.answer(1)
            if flags & PREFIX:
                suffix[r] = min(suffix[r], n - prefix[r])
        ok_n += n
    return status, len_a, len_b, prefix, suffix, [rows, ok_n, scratch, sum(1 for x in status if x == O.OK)]


def needs(side_a: Side, side_b: Side, requests, flags: int):
    """-> (max_rows, scratch_cap) that admit every request: the two sizing rounds."""
    rows = diff_plan(side_a, side_b, requests, flags, 0, 0)[5][0]
    return rows, diff_plan(side_a, side_b, requests, flags, rows, 0)[5][2]


def window_bytes(s: bytes, off: int, ln: int) -> bytes:
    """What the oracle decodes of a stream, clipped like a request."""
    data = O.frame_decode(s)
    lo, hi = R.clip(len(data), off, ln)
    return data[lo:hi]


# ---- the cases of the planning check (tests/abi/frame_diff_plan_check.hip) -------------------------------------------------------------------------
def plan_line(side_a: Side, side_b: Side, request, flags: int) -> str:
    """What the planning header must give for one request, as the check program prints it: both plans' statuses, n, then per direction asked
    for the flags bad_a bad_b have0 diff and the two pieces as t0 len and, per side, row0 nrows bytes off (all 0 when a row is bad)."""
    ba, oa, la, bb, ob, lb = request
    a, b = Req(side_a, ba, oa, la), Req(side_b, bb, ob, lb)
    out = [a.k["status"], b.k["status"]]
    if not (a.ok and b.ok):
        return " ".join(map(str, out))
    n = min(a.len, b.len)
    out.append(n)
    exact = bool(flags & EXACT)
    for d in (0, 1):
        if not flags & (PREFIX, SUFFIX)[d]:
            continue
        s = df_scan(a, b, d, n, not exact and n > 0)
        bad = s["bad_a"] or s["bad_b"]
        out += [int(s["bad_a"]), int(s["bad_b"]), int(s["have0"] and not bad), int(s["diff"] and not bad)]
        for a0, a1, b0, b1, t0, ln in df_pieces(s, df_need_rows(a, d, n), df_need_rows(b, d, n), n, exact) if not bad else [(0,) * 6] * 2:
            out += [t0, ln, *df_piece_side(a, d, a0, a1, t0, ln)[1:], *df_piece_side(b, d, b0, b1, t0, ln)[1:]]
    return " ".join(map(str, out))


def write_cases(path: str, cases):
    """The input of the check program.  cases: (side_a, side_b, flags, requests).  Per case both sides in full -- streams, then the index (any
    lists at all) -- and the requests."""
    with open(path, "wb") as f:
        f.write(struct.pack("<Q", len(cases)))
        for side_a, side_b, flags, requests in cases:
            for sd in (side_a, side_b):
                ns, ix = len(sd.streams), sd.ix
                f.write(struct.pack("<Q", ns))
                for s in sd.streams:
                    f.write(struct.pack("<Q", len(s)))
                    f.write(s)
                ne = min(len(ix["start"]), len(ix["pos"]))
                f.write(struct.pack("<Q", ne))
                for key, n in (("first", ns + 1), ("total", ns), ("tail", ns), ("start", ne), ("pos", ne)):
                    assert len(ix[key]) >= n
                    f.write(struct.pack("<%dQ" % n, *[int(v) & U64 for v in ix[key][:n]]))
            f.write(struct.pack("<2Q", flags, len(requests)))
            for q in requests:
                f.write(struct.pack("<6Q", *[int(v) & U64 for v in q]))

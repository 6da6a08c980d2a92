"""Pure-Python / numpy statement of include/snappier_hip_frame_cuts.h, written from the rule's text and not from the device header: the gear
hash, the content and the forced cuts of a buffer, the finder's admission and d_result (snp_content_cuts_batch), and the encoder that takes the
cuts as input (snp_frame_encode_cuts_batch) built on the oracle per piece through frame_chunked_model.  Also what the rule check program
(tests/abi/frame_cuts_rule_check.hip) reads and must print.  The CPU and the GPU tests share it."""
import struct

import numpy as np

import frame_chunked_model as K
import oracle as O

B = 65536
MIN_WINDOW, MAX_WINDOW = 32, 32767
M32 = 0xFFFFFFFF
U64 = (1 << 64) - 1


def fmix32(h: int) -> int:
    h ^= h >> 16
    h = h * 0x85EBCA6B & M32
    h ^= h >> 13
    h = h * 0xC2B2AE35 & M32
    return h ^ h >> 16


GEAR = np.array([fmix32((b + 1) * 0x9E3779B9 & M32) for b in range(256)], dtype=np.uint64)


def params_ok(w: int, mx: int) -> bool:
    return MIN_WINDOW <= w <= MAX_WINDOW and w < mx <= B


def hashes(x) -> np.ndarray:
    """g(0 .. n) as uint32: g(c) = sum over k = 1 .. min(32, c) of GEAR[x[c - k]] << (k - 1), which is what the recurrence unrolls to."""
    x = np.frombuffer(bytes(x), dtype=np.uint8)
    n = len(x)
    gear = GEAR[x]
    g = np.zeros(n + 1, dtype=np.uint64)
    for k in range(1, 33):
        if k <= n:
            g[k:] += gear[:n - k + 1] << np.uint64(k - 1)
    return (g & np.uint64(M32)).astype(np.uint32)


def _window_max(g: np.ndarray, w: int) -> np.ndarray:
    """out[i] = max(g[i : i + w]) for every i with i + w <= len(g)."""
    m, p = g, 1
    while 2 * p <= w:
        m = np.maximum(m[:-p], m[p:])
        p *= 2
    cnt = len(g) - w + 1
    return np.maximum(m[:cnt], m[w - p:w - p + cnt])


def content_cuts(x, w: int):
    n = len(x)
    if n <= 2 * w + 1:
        return []
    g = hashes(x)
    wm = _window_max(g, w)
    c = np.arange(w + 1, n - w)                                         # w < c < n - w
    keep = (g[c] > wm[c - w]) & (g[c] >= wm[c + 1])                     # [c - w, c) and (c, c + w]
    return [int(v) for v in c[keep]]


def cuts_of(x, w: int, mx: int):
    """-> (the buffer's cuts, ascending; how many of them are forced)."""
    assert params_ok(w, mx)
    n = len(x)
    marks = [0] + content_cuts(x, w) + [n]
    out, forced = [], 0
    for a, b in zip(marks, marks[1:]):
        f = list(range(a + mx, b, mx))
        forced += len(f)
        out += f
        if b < n:
            out.append(b)
    return out, forced


def cut_bound(n: int, w: int, mx: int) -> int:
    return n // (w + 1) + n // mx


def find(blobs, w: int, mx: int, span_bytes: int | None = None, max_cuts: int | None = None):
    """snp_content_cuts_batch: -> dict of cut_first, cuts, status, result [4].  None: a bound that admits all."""
    lens = [len(x) for x in blobs]
    span = sum(lens) if span_bytes is None else min(span_bytes, 1 << 40)
    per, total, fit = [], 0, 0
    for x in blobs:
        total += len(x)
        if total > span:
            break
        per.append(cuts_of(x, w, mx)[0])
        fit += 1
    need = sum(len(p) for p in per)
    cap = need if max_cuts is None else max_cuts
    first, cuts, status, run = [0], [], [], 0
    for b in range(len(blobs)):
        ok = b < fit and run + len(per[b]) <= cap and (not status or status[-1] == O.OK)
        if ok:
            run += len(per[b])
            cuts += per[b]
        first.append(run)
        status.append(O.OK if ok else O.ERR_OUTPUT_TOO_SMALL)
    return {"cut_first": first, "cuts": cuts, "status": status, "result": [need, run, min(sum(lens), U64), status.count(O.OK)]}


# ---- the encoder ----------------------------------------------------------------------------------------------------------------------------------
def stride(p: int) -> int:
    return K.stride(p)


def stage_bound(nbytes: int, pieces: int) -> int:
    return nbytes + nbytes // 6 + 69 * pieces


def list_verdict(n: int, lo: int, hi: int, cuts, ncuts: int | None = None):
    """-> (good, pieces as (start, length) pairs).  cuts: the whole list; the buffer's are cuts[lo : hi]."""
    ncuts = len(cuts) if ncuts is None else ncuts
    if lo > hi or hi > ncuts:
        return False, []
    prev, pieces = 0, []
    for c in cuts[lo:hi]:
        if not (prev < c < n and c - prev <= B):
            return False, []
        pieces.append((prev, c - prev))
        prev = c
    if n - prev > B:
        return False, []
    if n:
        pieces.append((prev, n - prev))
    return True, pieces


def encode_at_cuts(blobs, cut_first, cuts, variant: int = O.HASH_CRC32C, max_chunks: int | None = None, stage_cap: int | None = None, caps=None,
                   with_index: bool = True, ncuts: int | None = None):
    """snp_frame_encode_cuts_batch: -> the dict frame_chunked_model.encode gives.  None: a bound that admits all / the frame cap of the pieces."""
    nb = len(blobs)
    verdicts = [list_verdict(len(blobs[b]), cut_first[b], cut_first[b + 1], cuts, ncuts) for b in range(nb)]
    need = sum(len(p) for _, p in verdicts)
    need_stage = sum(stride(ln) for _, p in verdicts for _, ln in p)
    max_chunks = need if max_chunks is None else max_chunks
    stage_cap = need_stage if stage_cap is None else stage_cap
    r = {"status": [], "out_len": [], "streams": [], "first": [], "start": [], "pos": [], "total": [], "tail": []}
    slots = staged = rows = 0
    first = [0]
    for b, (good, pieces) in enumerate(verdicts):
        raw = blobs[b]
        st, stream = O.ERR_BAD_ARG, None
        if good:
            slots += len(pieces)
            staged += sum(stride(ln) for _, ln in pieces)
            st = O.ERR_OUTPUT_TOO_SMALL
            if slots <= max_chunks and staged <= stage_cap:
                chunks = [K.chunks_of(raw[s:s + ln], ln, variant)[0] for s, ln in pieces]
                size = 10 + sum(len(c) for c in chunks)
                if size <= (10 + 8 * len(pieces) + len(raw) if caps is None else caps[b]):
                    st, stream = O.OK, K.ID + b"".join(chunks)
                    if with_index:
                        p = 10
                        for (s, _), c in zip(pieces, chunks):
                            r["start"].append(s)
                            r["pos"].append(p)
                            p += len(c)
                        rows += len(pieces)
        r["status"].append(st)
        r["out_len"].append(len(stream) if stream is not None else 0)
        r["streams"].append(stream)
        first.append(rows)
        if with_index:
            r["total"].append(len(raw) if st == O.OK else 0)
            r["tail"].append(st)
    if with_index:
        r["first"] = first
    r["result"] = [need, sum(r["out_len"]), rows, r["status"].count(O.OK)]
    return r


def regular_cuts(lens, cb: int):
    """The cut list that puts every buffer's pieces on the grid k * cb: -> (cut_first, cuts)."""
    first, cuts = [0], []
    for n in lens:
        cuts += list(range(cb, n, cb))
        first.append(len(cuts))
    return first, cuts


# ---- the rule check program (tests/abi/frame_cuts_rule_check.hip) -------------------------------------------------------------------------------
def forced_in(a: int, lo: int, hi: int, mx: int):
    """The forced cuts a + k * mx, k >= 1, in [lo, hi): -> (how many, the first one's k)."""
    k0 = max(1, -(-(lo - a) // mx))
    k1 = (hi - 1 - a) // mx if hi > a else 0
    return max(0, k1 - k0 + 1), k0


def sat_join(hi: int, lo: int) -> int:
    return min(hi * (1 << 32) + lo, U64)


def write_cases(path: str, rule, lists, forced, joins):
    """rule: (w, mx, bytes); lists: (in_len, lo, hi, ncuts, cuts, piece queries, offset queries); forced: (a, lo, hi, mx); joins: (hi, lo)."""
    with open(path, "wb") as f:
        f.write(struct.pack("<4Q", len(rule), len(lists), len(forced), len(joins)))
        for w, mx, x in rule:
            f.write(struct.pack("<3Q", w, mx, len(x)) + bytes(x))
        for n, lo, hi, ncuts, cuts, ks, ats in lists:
            f.write(struct.pack("<7Q", n, lo, hi, ncuts, len(cuts), len(ks), len(ats)))
            f.write(struct.pack("<%dQ" % len(cuts), *cuts) + struct.pack("<%dQ" % len(ks), *ks) + struct.pack("<%dQ" % len(ats), *ats))
        for q in forced:
            f.write(struct.pack("<4Q", *q))
        for q in joins:
            f.write(struct.pack("<2Q", *q))


def check_lines(rule, lists, forced, joins):
    """What the rule check program must print for write_cases' input."""
    lines = ["%08x %08x %08x %08x %08x %08x" % (*(int(GEAR[b]) for b in (0, 1, 2, 97, 255)), int(hashes(bytes(range(32)))[32]))]
    for w, mx, x in rule:
        cuts, nforced = cuts_of(x, w, mx)
        lines.append("R %d %d %d %d%s" % (int(params_ok(w, mx)), len(cuts), nforced, cut_bound(len(x), w, mx), "".join(" %d" % c for c in cuts)))
    for n, lo, hi, ncuts, cuts, ks, ats in lists:
        good, pieces = list_verdict(n, lo, hi, cuts, ncuts)
        lines.append("V %d %d %d" % (int(good), len(pieces), sum(stride(ln) for _, ln in pieces)))
        if good:
            starts = [s for s, _ in pieces]
            lines.append("P" + "".join(" %d:%d" % pieces[k] for k in ks))
            lines.append("A" + "".join(" %d" % sum(1 for s in starts if s < at) for at in ats))
    for a, lo, hi, mx in forced:
        lines.append("F %d %d" % forced_in(a, lo, hi, mx))
    for hi, lo in joins:
        lines.append("J %d" % sat_join(hi, lo))
    return lines

"""NumPy / Python statement of csrc/frame_buffers.hip: the encode plan (chunk slots, framed sizes, emit positions) and the per-stream span walk of
the decode side (candidates, resolver, emit, admission by max_spans / max_chunks), next to the serial walk they must reproduce (scan_chunks of
capi_frame.hip).  The span and the candidate window are parameters: the device runs 1 MiB / 80 KiB, the CPU tests shrink them to a few hundred
bytes so that a small stream crosses many spans (as tag_index_model.py does for the tag index)."""
import numpy as np

import oracle as O

B = 65536
SPAN = 1 << 20
WINDOW = 80 * 1024
MAX_CAND = 4
STREAM_ID = b"\xff\x06\x00\x00sNaPpY"
EMPTY_MASKED_CRC = 0xA282EAD8


# ---- building framed streams ---------------------------------------------------------------------------------------------------------------
def chunk(t: int, body: bytes) -> bytes:
    return bytes([t]) + len(body).to_bytes(3, "little") + body


def data_chunk(raw: bytes, compressed: bool = True, variant: int = O.HASH_CRC32C) -> bytes:
    crc = O.crc32c(raw, masked=True).to_bytes(4, "little")
    return chunk(0 if compressed else 1, crc + (O.compress(raw, variant) if compressed else raw))


def oracle_chunks(raw: bytes, variant: int):
    """SnappyStreamCompressor's chunks of one buffer: (header + payload) per 65536 bytes, compressed only if smaller."""
    out = []
    for o in range(0, len(raw), B):
        piece = raw[o:o + B]
        comp = O.compress(piece, variant)
        t, pl = (0, comp) if len(comp) < len(piece) else (1, piece)
        out.append(bytes([t]) + (len(pl) + 4).to_bytes(3, "little") + O.crc32c(piece, masked=True).to_bytes(4, "little") + pl)
    return out


# ---- encode plan ---------------------------------------------------------------------------------------------------------------------------
def encode_plan(in_len, max_chunks: int, chunk_size, out_cap):
    """chunk_size(b, k) = 8 + payload of buffer b's chunk k.  -> (status, out_len, emit position of every (b, k) of an OK buffer, result)."""
    nb = len(in_len)
    first = np.zeros(nb + 1, dtype=np.int64)
    first[1:] = np.cumsum([(int(n) + B - 1) // B for n in in_len])
    owner = np.full(max_chunks, -1, dtype=np.int64)
    size = np.zeros(max_chunks, dtype=np.int64)
    for c in range(min(max_chunks, int(first[nb]))):
        b = int(np.searchsorted(first, c, side="right") - 1)
        if first[b + 1] <= max_chunks:
            owner[c] = b
            size[c] = chunk_size(b, c - int(first[b]))
    scan = np.zeros(max_chunks + 1, dtype=np.int64)
    scan[1:] = np.cumsum(size)
    status = np.full(nb, O.ERR_OUTPUT_TOO_SMALL, dtype=np.int32)
    out_len = np.zeros(nb, dtype=np.int64)
    for b in range(nb):
        if first[b + 1] <= max_chunks:
            s = 10 + int(scan[first[b + 1]] - scan[first[b]])
            if s <= out_cap[b]:
                status[b], out_len[b] = O.OK, s
    pos = {}
    for c in range(max_chunks):
        b = int(owner[c])
        if b >= 0 and status[b] == O.OK:
            pos[(b, c - int(first[b]))] = 10 + int(scan[c] - scan[first[b]])
    return status, out_len, pos, [int(first[nb]), int(out_len[status == O.OK].sum())]


# ---- one hop, the serial walk ----------------------------------------------------------------------------------------------------------------
class Hop:
    __slots__ = ("kind", "err", "type", "body_len", "crc", "dec", "next")

    def __init__(self, kind, nxt, err=0, type=0, body_len=0, crc=0, dec=0):
        self.kind, self.next, self.err, self.type, self.body_len, self.crc, self.dec = kind, nxt, err, type, body_len, crc, dec


def hop(s: bytes, ip: int) -> Hop:
    """frame_hop (frame_hop_device.h)."""
    n = len(s)
    if ip >= n:
        return Hop("end", ip)
    if n - ip < 4:
        return Hop("err", ip, O.ERR_TRUNCATED_STREAM)
    t, size = s[ip], int.from_bytes(s[ip + 1:ip + 4], "little")
    if n - (ip + 4) < size:
        return Hop("err", ip, O.ERR_TRUNCATED_STREAM)
    nxt = ip + 4 + size
    if t <= 1:
        if size < 4:
            return Hop("err", nxt, O.ERR_TRUNCATED_STREAM)
        dec = size - 4
        if t == 0:
            result = shift = 0
            done = bad = False
            for c in s[ip + 8:ip + 8 + min(size - 4, 5)]:
                val = c & 0x7F
                if val & ~(0xFFFFFFFF >> shift):
                    bad = True
                    break
                result |= val << shift
                shift += 7
                if c < 128:
                    done = True
                    break
            if bad or not done or result > 0x7FFFFFFF:
                return Hop("err", nxt, O.ERR_BAD_LENGTH)
            dec = result
            if dec > ((size - 4 - shift // 7) // 3 + 1) * 64:
                return Hop("err", nxt, O.ERR_INCOMPLETE)
        return Hop("data", nxt, type=t, body_len=size - 4, crc=int.from_bytes(s[ip + 4:ip + 8], "little"), dec=dec)
    if t < 0x80:
        return Hop("err", nxt, O.ERR_CHUNK_TYPE)
    return Hop("skip", nxt)


def serial_walk(s: bytes, cap: int):
    """scan_chunks (capi_frame.hip) with snp_frame_decode_device's cap rule: -> (rows [(type, body_off, body_len, crc, out_off, dec)], total, tail)."""
    rows, total, tail, ip = [], 0, O.OK, 0
    while True:
        h = hop(s, ip)
        if h.kind == "end":
            break
        if h.kind == "err":
            tail = h.err
            break
        if h.kind == "data":
            rows.append((h.type, ip + 8, h.body_len, h.crc, total, h.dec))
            total += h.dec
        ip = h.next
    if total > cap:
        return [], 0, O.ERR_OUTPUT_TOO_SMALL
    return rows, total, tail


# ---- the span walk ---------------------------------------------------------------------------------------------------------------------------
def chunk_shape(s: bytes, p: int):
    n = len(s)
    if n - p < 8:
        return False, 0
    t, size = s[p], int.from_bytes(s[p + 1:p + 4], "little")
    nxt = p + 4 + size
    if t == 0xFF:
        return size == 6 and n - p >= 10 and s[p + 4:p + 10] == b"sNaPpY", nxt
    if t > 1 or n - (p + 4) < size:
        return False, nxt
    if t == 1:
        return 4 <= size <= B + 4, nxt
    if size < 5 or size > 76496 + 4:
        return False, nxt
    h = hop(s, p)
    return h.kind == "data" and h.dec <= B, nxt


def plausible_start(s: bytes, p: int) -> bool:
    ok, nxt = chunk_shape(s, p)
    return ok and (nxt == len(s) or chunk_shape(s, nxt)[0])


def follow_chain(s: bytes, start: int, span_end: int):
    """-> (exit, dec, ndata, stop): stop 0 left the span, -1 clean end, > 0 the error."""
    ip, dec, nd, stop = start, 0, 0, 0
    while ip < span_end:
        h = hop(s, ip)
        if h.kind == "end":
            stop = -1
            break
        if h.kind == "err":
            stop = h.err
            break
        if h.kind == "data":
            nd += 1
            dec += h.dec
        ip = h.next
    if stop == 0 and ip >= len(s):
        stop = -1 if ip == len(s) else 0
    return ip, dec, nd, stop


def shape_prefilter(s: bytes, lo: int, hi: int) -> np.ndarray:
    """Positions p in [lo, hi) that pass chunk_shape's type and size rules (a superset of its answer, in NumPy): -> sorted int64 positions."""
    n = len(s)
    hi = min(hi, n - 7)                                                 # chunk_shape: n - p >= 8
    if hi <= lo:
        return np.zeros(0, dtype=np.int64)
    w = np.frombuffer(s, dtype=np.uint8, count=min(hi + 3, n) - lo, offset=lo)
    m = hi - lo
    t = w[:m]
    size = w[1:m + 1].astype(np.int64) | (w[2:m + 2].astype(np.int64) << 8) | (w[3:m + 3].astype(np.int64) << 16)
    p = np.arange(lo, hi, dtype=np.int64)
    fits = n - (p + 4) >= size
    ok = ((t == 0xFF) & (size == 6) & (n - p >= 10)) | \
         ((t == 1) & (size >= 4) & (size <= B + 4) & fits) | \
         ((t == 0) & (size >= 5) & (size <= 76496 + 4) & fits)
    return p[ok]


def candidates(s: bytes, k: int, span: int, window: int):
    """k_fd_candidates: span k's kept candidates (stream-relative) and their chains.  The scalar plausible_start runs only where
    shape_prefilter lets a position through."""
    n = len(s)
    s0 = k * span
    s1 = min(s0 + span, n)
    if k == 0:
        starts = [0]
    else:
        starts = []
        for p in shape_prefilter(s, s0, min(s0 + window, s1)).tolist():
            if plausible_start(s, p):
                starts.append(p)
                if len(starts) == MAX_CAND:
                    break
    return {p: follow_chain(s, p, s0 + span) for p in starts}


def candidates_scalar(s: bytes, k: int, span: int, window: int):
    """candidates() without the prefilter: plausible_start at every position of the window."""
    s0 = k * span
    s1 = min(s0 + span, len(s))
    starts = [0] if k == 0 else [p for p in range(s0, min(s0 + window, s1)) if plausible_start(s, p)][:MAX_CAND]
    return {p: follow_chain(s, p, s0 + span) for p in starts}


def span_walk(s: bytes, cap: int, span: int = SPAN, window: int = WINDOW):
    """k_fd_candidates + k_fd_resolve + k_fd_emit for one stream: -> (rows, total, tail, missed) with stream-relative offsets."""
    n = len(s)
    nspans = (n + span - 1) // span
    cands = [candidates(s, k, span, window) for k in range(nspans)]
    entry = {}
    e = total = nc = missed = 0
    tail = O.OK
    while nspans and e < n:
        k = e // span
        c = cands[k].get(e)
        if c is None:
            c = follow_chain(s, e, (k + 1) * span)
            missed += 1
        entry[k] = (e, nc, total)
        nc += c[2]
        total += c[1]
        if c[3] > 0:
            tail = c[3]
            break
        if c[3] < 0:
            break
        e = c[0]
    if total > cap:
        return [], 0, O.ERR_OUTPUT_TOO_SMALL, missed
    rows = [None] * nc
    for k, (ip, idx, off) in entry.items():
        while ip < (k + 1) * span and idx < nc:
            h = hop(s, ip)
            if h.kind in ("end", "err"):
                break
            if h.kind == "data":
                rows[idx] = (h.type, ip + 8, h.body_len, h.crc, off, h.dec)
                off += h.dec
                idx += 1
            ip = h.next
    return rows, total, tail, missed


def chunk_status(s: bytes, row) -> int:
    """What the decode and CRC launches give one row: the decoder's status, else the CRC check's."""
    t, bo, bl, crc, _, dec = row
    body = s[bo:bo + bl]
    if t == 0:
        st = O.decompress_status(body, dec)
        if st != O.OK:
            return st
        out = O.decompress(body, dec)
    else:
        out = body
    return O.OK if O.crc32c(out, masked=True) == crc else O.ERR_CRC_MISMATCH


def verdict(s: bytes, rows, total: int, tail: int):
    """k_fd_verdict: the first failing chunk, else the walk's tail, else OK -> (status, out_len)."""
    for r in rows:
        st = chunk_status(s, r)
        if st != O.OK:
            return st, 0
    return (tail, 0) if tail != O.OK else (O.OK, total)


def decode_plan(streams, caps, max_chunks: int, max_spans: int, span: int = SPAN, window: int = WINDOW, with_verdict: bool = True):
    """The whole decode side over a batch: -> (status, out_len, per-stream rows at their global slots, d_result)."""
    ns = len(streams)
    sfirst = np.zeros(ns + 1, dtype=np.int64)
    sfirst[1:] = np.cumsum([(len(x) + span - 1) // span for x in streams])
    walks = []
    missed = 0
    for b, x in enumerate(streams):
        if sfirst[b + 1] <= max_spans:
            w = span_walk(x, caps[b], span, window)
            missed += w[3]
        else:
            w = ([], 0, O.ERR_OUTPUT_TOO_SMALL, 0)
        walks.append(w)
    cfirst = np.zeros(ns + 1, dtype=np.int64)
    cfirst[1:] = np.cumsum([len(w[0]) for w in walks])
    status = np.full(ns, O.ERR_OUTPUT_TOO_SMALL, dtype=np.int32)
    out_len = np.zeros(ns, dtype=np.int64)
    slots = {}
    for b, (rows, total, tail, _) in enumerate(walks):
        if sfirst[b + 1] > max_spans or cfirst[b + 1] > max_chunks:
            continue
        for i, r in enumerate(rows):
            slots[int(cfirst[b]) + i] = (b, r)
        if with_verdict:
            status[b], out_len[b] = verdict(streams[b], rows, total, tail)
    return status, out_len, slots, [int(cfirst[ns]), int(out_len[status == O.OK].sum()), int(sfirst[ns]), missed], walks

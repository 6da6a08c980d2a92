"""Pure-Python statement of include/snappier_hip_frame_range.h (snp_frame_decode_range_batch): the window, which chunks it selects, which of those
are interior and which are edges, the status precedence, the in-order admission by max_spans / max_chunks / edge_cap and d_result -- built on the
span walk, the chunk status and the hop of frame_buffers_model.py -- and the streams and windows that the CPU and the GPU tests of the range call
share."""
import functools

import numpy as np

import frame_buffers_model as M
import oracle as O
from conftest import read_testdata

B = 65536
SPAN = M.SPAN
U64 = (1 << 64) - 1
ID = M.STREAM_ID


# ---- one stream ------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def walk(s: bytes, span: int = SPAN, window: int = M.WINDOW):
    """The span walk with no capacity bound: -> (rows [(type, body_off, body_len, crc, s, d)], total, tail, missed)."""
    return M.span_walk(s, 1 << 64, span, window)


@functools.lru_cache(maxsize=None)
def chunk_result(s: bytes, row):
    """-> (status, decoded bytes or None) of one row: the decoder's status, else the CRC check's."""
    st = M.chunk_status(s, row)
    if st != O.OK:
        return st, None
    t, bo, bl, _, _, dec = row
    body = s[bo:bo + bl]
    return O.OK, (O.decompress(body, dec) if t == 0 else body)


def clip(total: int, range_off: int, range_len: int):
    """-> (lo, hi): the window clipped like a read, the sum saturating at 2^64 - 1."""
    return min(range_off, total), min(min(range_off + range_len, U64), total)


def select(rows, lo: int, hi: int):
    """-> (selected rows in stream order, the edges among them)."""
    sel = [r for r in rows if r[5] > 0 and r[4] < hi and r[4] + r[5] > lo]
    edges = [r for r in sel if not (r[4] >= lo and r[4] + r[5] <= hi)]
    assert len(edges) <= 2
    assert not sel or [r for r in rows if r[5] > 0 and sel[0][4] <= r[4] <= sel[-1][4]] == sel      # contiguous among the non-empty chunks
    assert all(r is sel[0] or r is sel[-1] for r in edges)
    return sel, edges


def range_plan(streams, ranges, caps, max_chunks: int, max_spans: int, edge_cap: int, span: int = SPAN, window: int = M.WINDOW):
    """The whole call over a batch.  ranges: (range_off, range_len) per stream.
    -> (status list, out_len list, bytes per stream (None unless OK), d_result [6])."""
    ns = len(streams)
    status, out_len, data = [O.ERR_OUTPUT_TOO_SMALL] * ns, [0] * ns, [None] * ns
    spans = rows_needed = edge_bytes = missed = nselected = 0
    for b, s in enumerate(streams):
        spans += (len(s) + span - 1) // span
        if spans > max_spans:
            continue                                                    # not walked (and so is every later stream that has a span)
        rows, total, tail, m = walk(s, span, window)
        missed += m
        lo, hi = clip(total, *ranges[b])
        small = hi - lo > caps[b]
        sel, edges = ([], []) if small else select(rows, lo, hi)        # nothing of a stream whose window does not fit is decoded
        rows_needed += len(sel) - len(edges)
        edge_bytes += sum(r[5] for r in edges)
        nselected += len(sel)
        if rows_needed > max_chunks or edge_bytes > edge_cap:
            continue                                                    # not admitted (the sums only grow: nor is any later stream)
        # k_fd_verdict's precedence over the SELECTED chunks (edges are decoded and verified whole), then the capacity
        st = int(M.verdict(s, sel, hi - lo, tail)[0])
        if st == O.OK and small:
            st = O.ERR_OUTPUT_TOO_SMALL
        status[b] = st
        if st == O.OK:
            data[b] = b"".join(chunk_result(s, r)[1][max(r[4], lo) - r[4]:min(r[4] + r[5], hi) - r[4]] for r in sel)   # ... then trimmed
            out_len[b] = hi - lo
            assert len(data[b]) == hi - lo
    return status, out_len, data, [rows_needed, sum(out_len), spans, missed, edge_bytes, nselected]


def needs(streams, ranges, caps):
    """-> (max_chunks, max_spans, edge_cap) that admit the whole batch."""
    spans = sum((len(s) + SPAN - 1) // SPAN for s in streams)
    r = range_plan(streams, ranges, caps, 0, spans, 0)[3]
    return r[0], spans, r[4]


# ---- streams ---------------------------------------------------------------------------------------------------------------------------------
def long_stream_with_a_skippable_chunk_across_the_span_boundary():
    """More than one span; a skippable chunk crosses byte 2^20 and is followed by another one, so span 1 is entered at a header that is no
    candidate (the resolver walks it on the spot).  -> (stream, what it decodes to)."""
    rnd = np.random.default_rng(3).integers(0, 256, 1_040_000, dtype=np.uint8).tobytes()
    html = read_testdata("html")
    s = O.frame_encode(rnd)
    assert len(s) < SPAN - 100
    s += M.chunk(0xFE, bytes(20000)) + M.chunk(0x80, b"x" * 100) + O.frame_encode(html * 12)[10:] + M.data_chunk(rnd[:50000], compressed=False)
    assert SPAN < len(s) < 2 * SPAN
    return s, rnd + html * 12 + rnd[:50000]


def tiny_chunk_stream(seed: int, nchunks: int = 40):
    """A foreign stream of tiny chunks (1-300 bytes, compressed and raw mixed, an empty one now and then): -> (stream, decoded)."""
    rng = np.random.default_rng(seed)
    html = read_testdata("html")
    s, raw = ID, b""
    for k in range(nchunks):
        n = 0 if k % 11 == 5 else int(rng.integers(1, 301))
        o = int(rng.integers(0, 50000))
        piece = html[o:o + n]
        s += M.data_chunk(piece, compressed=bool(rng.integers(0, 2)))
        raw += piece
        if k % 13 == 7:
            s += M.chunk(0x80 + k, b"pad" * k)
    return s, raw


def big_chunk_stream():
    """A foreign stream with a chunk that decodes to more than 65536 bytes between two ordinary ones: -> (stream, decoded)."""
    html = read_testdata("html") * 3
    a, big, c = html[:5000], html[100:100 + 200_000], html[7:70007]
    return ID + M.data_chunk(a) + M.data_chunk(big) + M.data_chunk(c[:60000], compressed=False) + M.data_chunk(c[60000:]), a + big + c


def zero_length_chunk_stream():
    """Data chunks that decode to nothing (a compressed and a raw one) between, before and after ordinary chunks: -> (stream, decoded)."""
    html = read_testdata("html")
    d = M.data_chunk
    s = ID + d(b"") + d(html[:700]) + d(b"", compressed=False) + d(b"") + d(html[700:1500], compressed=False) + d(html[1500:1600]) + d(b"")
    return s, html[:1600]


def uniform_stream(nchunks: int, seed: int = 0, last: int = B):
    """nchunks chunks of 65536 bytes (the last one `last` bytes), as the project's own encoder cuts them: -> (stream, decoded)."""
    html = read_testdata("html") * 8
    rnd = np.random.default_rng(seed).integers(0, 256, B, dtype=np.uint8).tobytes()
    raw = b"".join(rnd if k % 3 == 2 else html[seed + 1000 * k:seed + 1000 * k + B] for k in range(nchunks))
    raw = raw[:(nchunks - 1) * B + last]
    return O.frame_encode(raw), raw


def corrupt_chunk(s: bytes, row) -> bytes:
    """s with one payload byte of the chunk `row` flipped (the last one: a literal's byte in a compressed chunk, so the decoder usually passes
    and the CRC check fails)."""
    p = row[1] + row[2] - 1
    return s[:p] + bytes([s[p] ^ 0x40]) + s[p + 1:]


# ---- windows ---------------------------------------------------------------------------------------------------------------------------------
def windows(rows, total: int):
    """(range_off, range_len) over a stream whose walk lists `rows` and `total` bytes: every shape the contract distinguishes."""
    w = [(0, 0), (total // 2, 0), (total, 0),                            # empty at 0, in the middle, at total
         (0, total), (0, total + 100), (0, U64),                          # the whole stream
         (total, 10), (total + 5, 10), (U64, U64),                        # range_off >= total
         (1, U64), (total // 3, U64 - 1), (total // 2, U64 - total // 2 + 1)]   # range_off + range_len overflows
    full = [r for r in rows if r[5] > 0]
    if full:
        picks = {0, len(full) // 2, len(full) - 1}
        for i in sorted(picks):
            s, d = full[i][4], full[i][5]
            w += [(s, d),                                               # exactly one chunk
                  (s, 1), (s + d - 1, 1),                               # one byte at its first and last position
                  (s + d - 1, 2), (max(s - 1, 0), 2),                   # two bytes across a chunk boundary
                  (s + d // 3, max(d // 3, 1)), (s + 1, max(d - 2, 0)),  # inside a single chunk: head and tail edge are the same chunk
                  (s, d + 1), (max(s - 1, 0), d + 1)]                   # one chunk and one byte of a neighbour
        i, j = len(full) // 4, max(len(full) * 3 // 4, len(full) // 4)
        w.append((full[i][4], full[j][4] + full[j][5] - full[i][4]))    # chunk-aligned over several chunks
        w.append((full[i][4] + full[i][5] // 2, full[j][4] + full[j][5] // 2 - full[i][4] - full[i][5] // 2))   # two edges and what lies between
    return list(dict.fromkeys(w))

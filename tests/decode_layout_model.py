"""Pure-Python statement of the two contracts of include/snappier_hip_layout.h (snp_decompress_layout_batch, snp_frame_decode_layout_batch): what
one item yields (a block's preamble with the expansion rule; a framed stream's header walk), the placement rule, and d_result -- and the inputs,
well-formed and malformed BY CONSTRUCTION, that the CPU and the GPU tests of the layout calls share.  The per-item parts are checked against the
host functions snp_get_uncompressed_length / snp_frame_decoded_length in test_decode_layout_model.py; the framed walk is frame_buffers_model's."""
import numpy as np

import frame_buffers_model as M
import oracle as O
from conftest import CORPUS, read_testdata

B = 65536
SPAN = M.SPAN
UNBOUNDED = 1 << 63
ID = M.STREAM_ID


# ---- one item --------------------------------------------------------------------------------------------------------------------------------
def varint(v: int) -> bytes:
    out = bytearray()
    while v >= 0x80:
        out.append((v & 0x7F) | 0x80)
        v >>= 7
    out.append(v)
    return bytes(out)


def read_preamble(buf: bytes):
    """snp_get_uncompressed_length: -> (status, value, header bytes)."""
    result = shift = 0
    for i, c in enumerate(buf[:5]):
        val = c & 0x7F
        if val & ~(0xFFFFFFFF >> shift):
            break
        result |= val << shift
        shift += 7
        if c < 128:
            return O.OK, result, i + 1
    return O.ERR_BAD_LENGTH, 0, 0


def expansion_bound(body_bytes: int) -> int:
    """No tag expands more than 3 bytes into 64 (a copy-2 of length 64)."""
    return (body_bytes // 3 + 1) * 64


def block_item(buf: bytes, in_len: int | None = None):
    """-> (status, declared).  in_len: the length the table gives when it is not len(buf) (only the first 5 bytes are ever read)."""
    n = len(buf) if in_len is None else in_len
    st, v, hb = read_preamble(buf[:n])
    if st != O.OK:
        return st, 0
    if v > expansion_bound(n - hb):
        return O.ERR_INCOMPLETE, 0
    return O.OK, v


def stream_item(s: bytes):
    """snp_frame_decoded_length, with the count of the chunks listed: -> (status, decoded_len, nchunks)."""
    rows, total, tail = M.serial_walk(s, 1 << 64)
    return tail, total, len(rows)


# ---- placement -------------------------------------------------------------------------------------------------------------------------------
def place(lengths, takes_part, align: int, arena_cap: int):
    """-> (offset of every item, f or None, arena bytes needed).  An item that takes part has a slot of its length rounded up to align."""
    off, o, f, need = [], 0, None, 0
    for n, t in zip(lengths, takes_part):
        off.append(o)
        if t:
            if f is None and o + n > arena_cap:
                f = len(off) - 1
            need = o + n
            o += (n + align - 1) // align * align
    return off, f, need


def block_layout(items, align: int = 1, arena_cap: int = UNBOUNDED):
    """items: (status, declared) per buffer -> dict of out_off, out_cap, declared, status (lists) and result."""
    n = len(items)
    ok = [st == O.OK for st, _ in items]
    off, f, need = place([d for _, d in items], ok, align, arena_cap)
    f = n if f is None else f
    status = [O.ERR_OUTPUT_TOO_SMALL if ok[b] and b >= f else items[b][0] for b in range(n)]
    cap = [items[b][1] if ok[b] and b < f else 0 for b in range(n)]
    return {"out_off": off, "out_cap": cap, "declared": [d for _, d in items], "status": status,
            "result": [need, f, sum((c + B - 1) // B for c in cap), sum(cap)]}


def stream_layout(items, in_len, max_spans: int, align: int = 1, arena_cap: int = UNBOUNDED, missed: int = 0, span: int = SPAN):
    """items: (status, decoded_len, nchunks) per stream, in_len their sizes -> dict of out_off, out_cap, decoded_len, nchunks, status, result.
    missed: the spans the resolver walks on the spot (frame_buffers_model.span_walk), over the walked streams."""
    n = len(items)
    sfirst = np.concatenate([[0], np.cumsum([(int(x) + span - 1) // span for x in in_len])])
    walked = [bool(sfirst[b + 1] <= max_spans) for b in range(n)]
    off, f, need = place([t for _, t, _ in items], walked, align, arena_cap)
    unwalked = [b for b in range(n) if not walked[b]]
    first = min([n if f is None else f] + unwalked[:1])
    f = n if f is None else f
    out = {"out_off": [], "out_cap": [], "decoded_len": [], "nchunks": [], "status": []}
    for b, (st, total, nc) in enumerate(items):
        if not walked[b]:
            row = (0, 0, 0, 0, O.ERR_OUTPUT_TOO_SMALL)
        elif b >= f:
            row = (off[b], 0, total, nc, O.ERR_OUTPUT_TOO_SMALL)
        else:
            row = (off[b], total, total, nc, st)
        for k, v in zip(out, row):
            out[k].append(v)
    placed = [b for b in range(n) if walked[b] and b < f]
    out["result"] = [need, first, int(sfirst[n]), sum(items[b][2] for b in placed), missed]
    return out


def missed_spans(streams, max_spans: int) -> int:
    sfirst = np.cumsum([(len(x) + SPAN - 1) // SPAN for x in streams])
    return sum(M.span_walk(x, 1 << 64)[3] for x, s in zip(streams, sfirst) if s <= max_spans)


# ---- inputs ----------------------------------------------------------------------------------------------------------------------------------
def max_expansion_body(m: int) -> bytes:
    """One literal byte, then m copy-2 tags of length 64 at offset 1: 2 + 3 m bytes that decode to 1 + 64 m."""
    return b"\x00a" + b"\xfe\x01\x00" * m


def block_cases():
    """name -> block bytes, one or more per class of the block contract."""
    html = read_testdata("html")
    c = {}
    c["empty"] = b""
    c["zero"] = b"\x00"
    c["one_literal"] = O.compress(b"a")
    c["html_64k"] = O.compress(html[:B])
    c["html_mul"] = O.compress(html[:30000], O.HASH_MUL)
    c["unterminated_1"] = b"\x80"
    c["unterminated_2"] = b"\xff\xff"
    c["unterminated_4"] = b"\x80\x80\x80\x80"
    c["bits_above_2_32"] = b"\xff\xff\xff\xff\x10" + bytes(40)
    c["six_bytes_zero_tail"] = b"\x80\x80\x80\x80\x80\x01" + bytes(40)
    c["six_bytes"] = b"\x80\x80\x80\x80\x8f\x00" + bytes(40)
    c["u32_max_short_body"] = b"\xff\xff\xff\xff\x0f" + bytes(40)          # a clean 2^32 - 1 that 40 bytes cannot produce
    for k in (0, 1, 2, 3, 10, 299):
        c[f"at_bound_{k}"] = varint(expansion_bound(k)) + bytes(k)
        c[f"over_bound_{k}"] = varint(expansion_bound(k) + 1) + bytes(k)
    for m in (1, 7, 100):
        body = max_expansion_body(m)
        c[f"max_expansion_{m}"] = varint(1 + 64 * m) + body                # well-formed, the most a body can expand
        c[f"max_expansion_over_{m}"] = varint(expansion_bound(len(body)) + 1) + body
    return c


def stream_cases():
    """name -> framed stream bytes, one or more per class of the framed contract."""
    html = read_testdata("html") * 3
    d = M.data_chunk
    good = ID + d(html[:600]) + d(html[600:5000], compressed=False)
    crc = b"\x01\x02\x03\x04"
    c = {}
    c["empty"] = b""
    c["id_only"] = ID
    c["plain"] = O.frame_encode(html[:200000])
    c["plain_mul"] = O.frame_encode(html[:70000], O.HASH_MUL)
    c["raw_chunks"] = ID + b"".join(d(html[i:i + 700], compressed=False) for i in range(0, 7000, 700))
    c["concat"] = O.frame_encode(html[:1000]) + O.frame_encode(html[5:5000])
    c["cut_in_header_1"] = good + b"\x00"
    c["cut_in_header_3"] = good + b"\x00\x10\x00"
    c["cut_in_body"] = (good + d(html[:900]))[:-9]
    c["cut_in_first_body"] = (ID + d(html[:900]))[:-1]
    c["cut_in_id"] = ID[:7]
    c["size_3_compressed"] = good + M.chunk(0x00, b"\x01\x02\x03") + d(html[:50])
    c["size_0_raw"] = good + M.chunk(0x01, b"") + d(html[:50])
    c["type_02"] = good + M.chunk(0x02, b"zz") + d(html[:80])
    c["type_7f"] = good + M.chunk(0x7F, b"") + d(html[:80])
    c["type_02_first"] = M.chunk(0x02, b"zzzz")
    c["skippable"] = ID + d(html[:300]) + M.chunk(0x80, b"x" * 17) + d(html[300:900]) + M.chunk(0xFE, b"") + M.chunk(0xFF, b"\x00" * 5) + \
        d(html[900:1000]) + M.chunk(0x85, bytes(1500))
    c["bad_varint_after_good"] = good + M.chunk(0x00, crc + b"\xff" * 6) + d(html[:80])
    c["unterminated_varint"] = good + M.chunk(0x00, crc + b"\x80\x80")
    c["varint_2_31"] = good + M.chunk(0x00, crc + varint(1 << 31) + bytes(30))
    c["over_bound"] = good + M.chunk(0x00, crc + varint(expansion_bound(10) + 1) + bytes(10)) + d(html[:80])
    c["at_bound"] = good + M.chunk(0x00, crc + varint(expansion_bound(10)) + bytes(10)) + d(html[:80])   # listed: it fails in the decoder
    c["bad_crc"] = ID + d(html[:500])[:5] + b"\x00" + d(html[:500])[6:] + d(html[:50])                    # the walk does not see it
    return c


def corpus_blocks():
    return {f"{f}/{v}": O.compress(read_testdata(f), v) for f in CORPUS for v in (O.HASH_CRC32C, O.HASH_MUL)}


def corpus_streams():
    return {f"{f}/{v}": O.frame_encode(read_testdata(f), v) for f in CORPUS for v in (O.HASH_CRC32C, O.HASH_MUL)}

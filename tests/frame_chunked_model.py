"""Pure-Python statement of include/snappier_hip_frame_chunked.h (snp_frame_encode_chunked_batch): framed streams with one chunk per chunk_bytes
input bytes, each chunk what M.data_chunk / O.compress / O.crc32c make of its piece; the admission plan (prefix admission by max_chunks), the
out_cap plan (a buffer in the middle may fail alone), the seek index by the conventions of include/snappier_hip_frame_index.h (rows of the OK
buffers only), d_result, the staging stride, and the slot arithmetic of csrc/frame_chunked_device.h as the planning check program
(tests/abi/frame_chunked_plan_check.hip) prints it.  The CPU and the GPU tests share it."""
import struct

import frame_buffers_model as M
import oracle as O

B = 65536
ID = M.STREAM_ID
CHUNK_SIZES = [1, 14, 15, 16, 17, 255, 256, 257, 4096, 16384, 16385, 65535, 65536]    # the compressor's seams (n < 15 all-literal, HashTable.cs:57-71 steps, its cap)


def nchunks(n: int, cb: int) -> int:
    return (n + cb - 1) // cb


def stride(cb: int) -> int:
    """The staging stride of a slot: snp_max_compressed_length(cb) rounded up to 16, plus 16 (kSnpCompStride's rule)."""
    return (38 + cb + cb // 6 + 15) // 16 * 16 + 16


def frame_cap(n: int, cb: int) -> int:
    return 10 + 8 * nchunks(n, cb) + n


def chunks_of(raw: bytes, cb: int, variant: int = O.HASH_CRC32C):
    """CompressBlock (SnappyStreamCompressor.cs:194-230) over every piece: type 0x00 when varint || fragment is smaller than the piece, else 0x01."""
    out = []
    for o in range(0, len(raw), cb):
        piece = raw[o:o + cb]
        comp = O.compress(piece, variant)
        crc = O.crc32c(piece, masked=True).to_bytes(4, "little")
        out.append(M.chunk(0, crc + comp) if len(comp) < len(piece) else M.chunk(1, crc + piece))     # (M.data_chunk of the piece, compressed once)
    return out


def stream_of(raw: bytes, cb: int, variant: int = O.HASH_CRC32C) -> bytes:
    return ID + b"".join(chunks_of(raw, cb, variant))


def buffer_lengths(cb: int):
    """The buffer lengths of the seam tests: 0, 1, cb - 1, cb, cb + 1, 3 cb, 3 cb + 1."""
    return [0, 1, cb - 1, cb, cb + 1, 3 * cb, 3 * cb + 1]


# ---- the plan (csrc/frame_chunked_device.h) ------------------------------------------------------------------------------------------------------
def first_slots(in_len, cb: int):
    first = [0]
    for n in in_len:
        first.append(first[-1] + nchunks(int(n), cb))
    return first


def slot(first, in_len, max_chunks: int, cb: int, c: int):
    """fc_slot: -> (owner or -1, piece length, k, piece offset)."""
    nb = len(in_len)
    if c >= first[nb]:
        return -1, 0, 0, 0
    lo, hi = 0, nb
    while hi - lo > 1:
        mid = lo + (hi - lo) // 2
        if first[mid] <= c:
            lo = mid
        else:
            hi = mid
    if first[lo + 1] > max_chunks:
        return -1, 0, 0, 0
    k = c - first[lo]
    return lo, min(int(in_len[lo]) - k * cb, cb), k, k * cb


def group(cb: int) -> int:
    return (B + cb - 1) // cb


def team(g: int) -> int:
    return 256 if g == 1 else 128 if g == 2 else 64


def verdicts(in_len, cb: int, max_chunks: int, sizes, out_cap):
    """sizes[b] = the size of buffer b's stream.  -> (status list, out_len list, first, ok_first)."""
    first = first_slots(in_len, cb)
    status, out_len, ok_first = [], [], [0]
    for b in range(len(in_len)):
        ok = first[b + 1] <= max_chunks and sizes[b] <= out_cap[b]
        status.append(O.OK if ok else O.ERR_OUTPUT_TOO_SMALL)
        out_len.append(sizes[b] if ok else 0)
        ok_first.append(ok_first[-1] + (first[b + 1] - first[b] if ok else 0))
    return status, out_len, first, ok_first


def encode(blobs, cb: int, variant: int = O.HASH_CRC32C, max_chunks: int | None = None, caps=None, with_index: bool = True):
    """snp_frame_encode_chunked_batch over a batch: -> dict of status, out_len, streams (None for a buffer that is not OK), first, start, pos,
    total, tail (the index; empty lists without one) and result [4].  None: a bound that admits all / frame_cap."""
    assert 1 <= cb <= B
    lens = [len(x) for x in blobs]
    chunks = [chunks_of(x, cb, variant) for x in blobs]
    sizes = [10 + sum(len(c) for c in cs) for cs in chunks]
    need = sum(nchunks(n, cb) for n in lens)
    max_chunks = need if max_chunks is None else max_chunks
    caps = [frame_cap(n, cb) for n in lens] if caps is None else caps
    status, out_len, first, ok_first = verdicts(lens, cb, max_chunks, sizes, caps)
    r = {"status": status, "out_len": out_len, "streams": [ID + b"".join(cs) if st == O.OK else None for cs, st in zip(chunks, status)],
         "first": [], "start": [], "pos": [], "total": [], "tail": []}
    if with_index:
        r["first"] = ok_first
        for b, cs in enumerate(chunks):
            ok = status[b] == O.OK
            r["total"].append(lens[b] if ok else 0)
            r["tail"].append(O.OK if ok else O.ERR_OUTPUT_TOO_SMALL)
            p = 10
            for k, c in enumerate(cs if ok else []):
                r["start"].append(k * cb)
                r["pos"].append(p)
                p += len(c)
    r["result"] = [need, sum(out_len), len(r["start"]), sum(1 for s in status if s == O.OK)]
    return r


# ---- the cases of the planning check (tests/abi/frame_chunked_plan_check.hip) -----------------------------------------------------------------
def interesting_slots(first, max_chunks: int):
    """Slots around every buffer's first and last chunk, around max_chunks and around 2^32 - 1, inside u32."""
    s = set()
    for f in first:
        s.update((f - 2, f - 1, f, f + 1, f + 2))
    s.update((0, 1, max_chunks - 1, max_chunks, max_chunks + 1, (1 << 20) + 1, (1 << 32) - 2, (1 << 32) - 1))
    return sorted(c for c in s if 0 <= c < (1 << 32))


def plan_lines(in_len, status, cb: int, max_chunks: int, slots):
    """What the planning header must give: one line for the case, one per queried slot, as the check program prints them."""
    first = first_slots(in_len, cb)
    ok_first = [0]
    for b in range(len(in_len)):
        ok_first.append(ok_first[-1] + (first[b + 1] - first[b] if status[b] == O.OK else 0))
    g = group(cb)
    lines = ["%d %d %d %d" % (first[-1], ok_first[-1], g, team(g))]
    for c in slots:
        b, ln, k, off = slot(first, in_len, max_chunks, cb, c)
        row = (ok_first[b] + k, k * cb) if b >= 0 and status[b] == O.OK else (0, 0)
        lines.append("%d %d %d %d %d %d %d" % (b, ln, k, off, c * stride(cb), row[0], row[1]))
    return lines


def write_cases(path: str, cases):
    """The input of the check program: per case cb, max_chunks, the stride, nb, in_len[nb], status[nb], the slots to query."""
    with open(path, "wb") as f:
        f.write(struct.pack("<Q", len(cases)))
        for in_len, status, cb, max_chunks, slots in cases:
            f.write(struct.pack("<4Q", cb, max_chunks, stride(cb), len(in_len)))
            f.write(struct.pack("<%dQ" % len(in_len), *in_len))
            f.write(struct.pack("<%dQ" % len(status), *status))
            f.write(struct.pack("<Q", len(slots)))
            f.write(struct.pack("<%dQ" % len(slots), *slots))

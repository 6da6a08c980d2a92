// frame_buffers.hip -- snp_frame_encode_buffers_batch / snp_frame_decode_buffers_batch: many Snappy framed streams in one call, each byte for byte
// what snp_frame_encode_device / snp_frame_decode_device give for it alone (SnappyStreamCompressor.cs:18-21,166-261; SnappyStreamDecompressor.cs:38-208),
// entirely on the device.  The framing counterpart of the buffers calls (buffers.hip, buffers_decode.hip): plans and scans (scan_tiles.h) around
// ONE launch of each existing codec kernel for the whole batch, instead of five or more launches per stream.  Built into
// libsnappier_hip_frame_buffers.so (C-ABI: include/snappier_hip_frame_buffers.h), linked against libsnappier_hip.so.  DESIGN.md 4.11.
//
// Encode (every buffer cut into 65536-byte chunks, the chunks of all buffers in one table of max_chunks slots):
//   scan      ceil(in_len / 65536) -> each buffer's first chunk slot (d_result[0] = slots needed)
//   plan      one thread per slot: owning buffer (binary search), input range, staging offset; slots past the batch, and the slots of buffers
//             that do not fit max_chunks, stay empty
//   compress  snp_ctx::launch_compress over every slot, varint on (a framed chunk body is a whole Snappy block), into kSnpCompStride staging
//   crc       masked CRC-32C of every raw slot (snp_launch_crc32c)
//   scan      8 + payload per slot, the payload compressed only if smaller than the raw chunk (CompressBlock  SnappyStreamCompressor.cs:212)
//   sizes     one thread per buffer: stream size, status, out_len, the 10-byte stream identifier of an OK buffer, d_result[1]
//   emit      one 256-thread workgroup per slot: header + payload at out_off[owner] + 10 + (its place among the owner's chunks)
// Decode (every stream cut into 1 MiB spans relative to its own start, the spans of all streams in one table of max_spans slots):
//   scan      ceil(in_len / 2^20) -> each stream's first span slot (d_result[2]); a stream whose spans do not fit is not walked
//   A         one wavefront per span slot: k_span_candidates of frame_scan.hip on the owner's span (span 0 enters at the stream's byte 0)
//   B         one wavefront per stream: k_span_resolve's chain through the stream's spans; an entry that is no candidate is walked on the spot and
//             counted in d_result[3]; total > out_cap[b] lists no chunk (OUTPUT_TOO_SMALL), as there
//   scan      chunks listed per stream -> each stream's first chunk slot (d_result[0]); a stream whose chunks do not fit is not decoded
//   C         one wavefront per span slot: the rows of the span's chunks at their global slots, body and output offsets absolute; one thread per
//             slot pads every other slot with an empty raw chunk and the CRC of nothing
//   decode    snp_ctx::decode_chunks over all max_chunks slots: launch_decompress(chunk_type) and the verifying snp_launch_crc32c
//   verdict   one thread per failing slot: atomicMin of its slot into its stream's word; one thread per stream: the first failing chunk, else
//             the walk's tail error, else OK (k_frame_result's precedence) -> status, out_len, d_result[1]
// Nothing here allocates, reads back or synchronises: both calls are capturable like the other _batch entry points.
#include "capi_internal.h"
#include "frame_walk_device.h"
#include "../../include/snappier_hip_frame_buffers.h"

namespace {

__constant__ u8 k_fb_stream_id[SNP_STREAM_HEADER_LEN] = {0xff, 0x06, 0x00, 0x00, 0x73, 0x4e, 0x61, 0x50, 0x70, 0x59};   // SnappyStreamCompressor.cs:18-21

__device__ __forceinline__ u32 payload_of(u32 comp, u32 raw, bool* shrink)
{
    *shrink = comp < raw;                                               // CompressBlock  SnappyStreamCompressor.cs:212
    return *shrink ? comp : raw;
}
// scan source: one framed chunk's size (0 for an empty slot)
struct ScanFramed {
    const u32* __restrict__ owner;
    const u32* __restrict__ comp_len;
    const u32* __restrict__ raw_len;
    __device__ __forceinline__ u64 operator()(u64 i) const
    {
        bool shrink;
        return owner[i] == kNone ? 0 : SNP_CHUNK_HEADER_LEN + payload_of(comp_len[i], raw_len[i], &shrink);
    }
};

// ---- encode ----------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_fe_plan(const u64* __restrict__ in_off, const u64* __restrict__ in_len, u32 nb, const u64* __restrict__ first,
                                                u32 max_chunks, u64* __restrict__ c_in_off, u32* __restrict__ c_in_len, u64* __restrict__ c_stage_off,
                                                u32* __restrict__ c_owner)
{
    const u32 c = blockIdx.x * 256u + threadIdx.x;
    if (c >= max_chunks) return;
    u64 io = 0;
    u32 il = 0, owner = kNone;
    if (c < first[nb]) {
        const u32 b = owner_of(first, nb, c);
        if (first[b + 1] <= max_chunks) {                               // else the buffer does not fit: its slots stay empty
            const u64 k = c - first[b];
            const u64 rest = in_len[b] - k * SNP_BLOCK_SIZE;
            io = in_off[b] + k * SNP_BLOCK_SIZE;
            il = rest < SNP_BLOCK_SIZE ? static_cast<u32>(rest) : static_cast<u32>(SNP_BLOCK_SIZE);
            owner = b;
        }
    }
    c_in_off[c] = io;
    c_in_len[c] = il;
    c_stage_off[c] = static_cast<u64>(c) * kSnpCompStride;
    c_owner[c] = owner;
}

// Stream size = identifier + the buffer's framed chunks; OK only when every chunk was planned and the stream fits out_cap.  Only an OK buffer's
// range is written (its identifier here, its chunks by k_fe_emit); result[1] += the OK sizes (one atomic per wavefront).
__global__ __launch_bounds__(256) void k_fe_sizes(u32 nb, const u64* __restrict__ first, u32 max_chunks, const u64* __restrict__ cscan,
                                                 u8* __restrict__ out, const u64* __restrict__ out_off, const u64* __restrict__ out_cap,
                                                 u64* __restrict__ out_len, i32* __restrict__ status, u64* __restrict__ result)
{
    const u32 b = blockIdx.x * 256u + threadIdx.x;
    u64 ok_len = 0;
    if (b < nb) {
        const u64 end = first[b + 1];
        i32 st = SNP_ERR_OUTPUT_TOO_SMALL;
        u64 len = 0;
        if (end <= max_chunks) {
            const u64 size = SNP_STREAM_HEADER_LEN + (cscan[end] - cscan[first[b]]);
            if (size <= out_cap[b]) {
                u8* const dst = out + out_off[b];
                for (u32 i = 0; i < SNP_STREAM_HEADER_LEN; ++i) dst[i] = k_fb_stream_id[i];   // EnsureStreamHeaderWritten  :148-157
                st = SNP_OK;
                len = size;
            }
        }
        out_len[b] = len;
        status[b] = st;
        ok_len = len;
    }
    ok_len = wave_sum(ok_len);
    if ((threadIdx.x & 63u) == 0 && ok_len) atomic_add64(result + 1, ok_len);
}

// One workgroup per slot: [type:1][len:3 LE = payload + 4][masked crc:4 LE][payload]  (:233-261), k_frame_emit's chunk at its buffer's place.
__global__ __launch_bounds__(256) void k_fe_emit(const u32* __restrict__ c_owner, const u64* __restrict__ c_in_off, const u32* __restrict__ c_in_len,
                                                const u32* __restrict__ comp_len, const u32* __restrict__ crc, const u64* __restrict__ cscan,
                                                const u64* __restrict__ first, const i32* __restrict__ status, const u8* __restrict__ stage,
                                                const u8* __restrict__ in, u8* __restrict__ out, const u64* __restrict__ out_off)
{
    const u32 c = blockIdx.x, tid = threadIdx.x;
    const u32 b = c_owner[c];
    if (b == kNone || status[b] != SNP_OK) return;
    bool shrink;
    const u32 pl = payload_of(comp_len[c], c_in_len[c], &shrink);
    u8* const dst = out + out_off[b] + SNP_STREAM_HEADER_LEN + (cscan[c] - cscan[first[b]]);
    chunk_header(dst, tid, shrink ? 0u : 1u, pl, crc[c]);
    const u8* const src = shrink ? stage + static_cast<u64>(c) * kSnpCompStride : in + c_in_off[c];
    block_copy(dst + SNP_CHUNK_HEADER_LEN, src, pl, tid);
}

// ---- decode ----------------------------------------------------------------------------------------------------------------------------------
// (the span table FbSpans, the chunk table ChunkRows and the per-span bodies are in frame_hop_device.h, the per-stream record FbStreams and walks A
// and B -- k_fd_candidates, k_fd_resolve -- in frame_walk_device.h; a row's tag is its stream here)

// C: the rows of every span of every decoded stream at their global slots (k_span_emit), body and output offsets absolute
__global__ __launch_bounds__(SNP_WAVE) void k_fd_emit(const u8* __restrict__ in, const u64* __restrict__ in_off, const u64* __restrict__ in_len,
                                                     const u64* __restrict__ out_off, u32 ns, const u64* __restrict__ sfirst, u32 max_spans,
                                                     const u64* __restrict__ cfirst, u32 max_chunks, FbSpans t, FbStreams st, ChunkRows r)
{
    const u32 g = blockIdx.x;
    if (lane_id() != 0 || g >= sfirst[ns]) return;
    const u32 b = owner_of(sfirst, ns, g);
    if (sfirst[b + 1] > max_spans || cfirst[b + 1] > max_chunks) return;   // not walked, or not decoded
    const u64 e = t.entry[g];
    if (e == kNoEntry) return;
    const u64 row0 = cfirst[b], ib = in_off[b], ob = out_off[b];
    for_span_chunks(in + ib, in_len[b], e, (g - sfirst[b] + 1) * kSpan, t.chunk_base[g], st.nc[b], t.out_base[g],
                    [&](const Hop& h, u64 ip, u32 idx, u64 off) {
                        chunk_row_set(r, row0 + idx, h, ib + ip, ob + off);
                        return true;
                    });
}

// one thread per chunk slot: its decoded stream, or an empty row (the decoder reads and writes nothing for it)
__global__ __launch_bounds__(256) void k_fd_pad(u32 ns, const u64* __restrict__ cfirst, u32 max_chunks, ChunkRows r)
{
    const u32 c = blockIdx.x * 256u + threadIdx.x;
    if (c >= max_chunks) return;
    u32 owner = kNone;
    if (c < cfirst[ns]) {
        const u32 b = owner_of(cfirst, ns, c);
        if (cfirst[b + 1] <= max_chunks) owner = b;                     // (a stream with chunks was walked)
    }
    r.tag[c] = owner;
    if (owner == kNone) chunk_row_clear(r, c, 0);
}

__global__ __launch_bounds__(256) void k_fd_fail(u32 max_chunks, ChunkRows r, FbStreams st)
{
    const u32 c = blockIdx.x * 256u + threadIdx.x;
    if (c >= max_chunks) return;
    const u32 b = r.tag[c];
    if (b != kNone && r.status[c] != SNP_OK) atomicMin(&st.fail[b], c);
}

// the stream's verdict (k_frame_result): the first failing chunk in stream order, else the error that ended the walk, else OK with the
// bytes listed; a stream that was not walked or not decoded is OUTPUT_TOO_SMALL.  result[1] += the OK lengths (one atomic per wavefront).
__global__ __launch_bounds__(256) void k_fd_verdict(u32 ns, const u64* __restrict__ sfirst, u32 max_spans, const u64* __restrict__ cfirst, u32 max_chunks,
                                                   FbStreams st, const i32* __restrict__ c_status, u64* __restrict__ out_len, i32* __restrict__ status,
                                                   u64* __restrict__ result)
{
    const u32 b = blockIdx.x * 256u + threadIdx.x;
    u64 ok_len = 0;
    if (b < ns) {
        i32 s = SNP_ERR_OUTPUT_TOO_SMALL;
        if (sfirst[b + 1] <= max_spans && cfirst[b + 1] <= max_chunks) {
            const u32 f = st.fail[b];
            s = f != kNone ? c_status[f] : st.tail[b];
            if (s == SNP_OK) ok_len = st.total[b];
        }
        status[b] = s;
        out_len[b] = ok_len;
    }
    ok_len = wave_sum(ok_len);
    if ((threadIdx.x & 63u) == 0 && ok_len) atomic_add64(result + 1, ok_len);
}

// ---- workspaces (every piece 256-byte aligned; nothing when there is no buffer) --------------------------------------------------------------
// encode.  Per buffer: first chunk slot (nb + 1) and its tile sums.  Per slot: input offset and length, staging offset, compressed length,
// compressor status, owner, masked CRC, the scan of the framed sizes (max_chunks + 1) and its tile sums; then kSnpCompStride of staging.
struct EncodeWork {
    u64 *first, *first_part, *c_in_off, *c_stage_off, *cscan, *c_part;
    u32 *c_in_len, *comp_len, *c_owner, *crc;
    i32* c_status;
    u8* stage;
    u64 bytes;
};
EncodeWork encode_work_layout(void* base, u32 nbuffers, u32 max_chunks)
{
    EncodeWork w{};
    if (nbuffers == 0) return w;
    const u64 nb = nbuffers, nc = max_chunks;
    WorkCarver k(base);
    w.first = k.take<u64>(nb + 1);
    w.first_part = k.take<u64>(scan_tiles_of(nb));
    w.cscan = k.take<u64>(nc + 1);
    w.c_part = k.take<u64>(scan_tiles_of(nc));
    w.c_in_off = k.take<u64>(nc);
    w.c_stage_off = k.take<u64>(nc);
    w.c_in_len = k.take<u32>(nc);
    w.comp_len = k.take<u32>(nc);
    w.c_owner = k.take<u32>(nc);
    w.crc = k.take<u32>(nc);
    w.c_status = k.take<i32>(nc);
    w.stage = k.take<u8>(nc * kSnpCompStride);
    w.bytes = k.bytes();
    return w;
}

// decode.  Per stream: first span slot and first chunk slot (ns + 1 each), the tile sums of their scans, the walk's record.  Per span slot: the
// candidates and the resolver's entry.  Per chunk slot: the chunk table (body and output offsets, lengths, CRC, status, owner, type).
struct DecodeWork {
    u64 *sfirst, *cfirst, *part;
    FbStreams st;
    FbSpans sp;
    ChunkRows r;
    u64 bytes;
};
DecodeWork decode_work_layout(void* base, u32 nstreams, u32 max_chunks, u32 max_spans)
{
    DecodeWork w{};
    if (nstreams == 0) return w;
    const u64 ns = nstreams, nc = max_chunks, nsp = max_spans;
    WorkCarver k(base);
    w.sfirst = k.take<u64>(ns + 1);
    w.cfirst = k.take<u64>(ns + 1);
    w.part = k.take<u64>(scan_tiles_of(ns));
    carve_span_walk(k, ns, nsp, w.st, w.sp);
    w.r = carve_chunk_rows(k, nc);
    w.bytes = k.bytes();
    return w;
}

bool result_empty(snp_ctx* c, u64* d_result, u32 words)
{
    return c->check(snp_zero_words_async(reinterpret_cast<u32*>(d_result), 2 * words, c->stream), "frame buffers result");
}

}  // namespace

extern "C" {

uint64_t snp_frame_encode_buffers_workspace(uint32_t nbuffers, uint32_t max_chunks)
{
    return encode_work_layout(nullptr, nbuffers, max_chunks).bytes;
}

snp_status snp_frame_encode_buffers_batch(snp_ctx* c, const uint8_t* in, const uint64_t* in_off, const uint64_t* in_len, uint32_t nbuffers,
                                          uint32_t max_chunks, uint8_t* out, const uint64_t* out_off, const uint64_t* out_cap, uint64_t* out_len,
                                          int32_t* status, void* d_work, uint64_t* d_result)
{
    if (!c || !d_result || (nbuffers && (!in || !in_off || !in_len || !out || !out_off || !out_cap || !out_len || !status || !d_work)))
        return SNP_ERR_BAD_ARG;
    DevGuard dg(c);
    if (!dg.ok) return SNP_ERR_DEVICE;
    hipStream_t s = c->stream;
    if (nbuffers == 0) return result_empty(c, d_result, 2) ? SNP_OK : SNP_ERR_DEVICE;
    const EncodeWork w = encode_work_layout(d_work, nbuffers, max_chunks);
    const u32 nb = nbuffers, M = max_chunks;
    // plan: first chunk slot of every buffer (d_result[0] = slots needed, d_result[1] = 0), then the chunk table over all max_chunks slots
    bool ok = c->check(launch_scan(ScanPieces{in_len, SNP_BLOCK_SIZE}, nb, w.first_part, w.first, d_result, s), "frame buffers scan");
    if (ok && M) {
        hipLaunchKernelGGL(k_fe_plan, dim3((M + 255u) / 256u), dim3(256), 0, s, in_off, in_len, nb, w.first, M, w.c_in_off, w.c_in_len,
                           w.c_stage_off, w.c_owner);
        // CompressBlock: TryCompress(chunk) = varint + one fragment (SnappyStreamCompressor.cs:206), every slot (the count picks the layout);
        // then the masked CRC-32C of every RAW chunk (:243-245,258-260)
        ok = c->check(hipGetLastError(), "frame buffers plan") &&
             c->launch_compress(in, w.c_in_off, w.c_in_len, M, w.stage, w.c_stage_off, w.comp_len, w.c_status, 1) &&
             c->check(snp_launch_crc32c(in, w.c_in_off, w.c_in_len, M, 1 | c->crc_bits(), w.crc, nullptr, nullptr, s), "frame buffers crc");
    }
    // the framed chunk sizes, then every buffer's size and status, then the chunks to their places (a buffer that is not OK is not written)
    ok = ok && c->check(launch_scan(ScanFramed{w.c_owner, w.comp_len, w.c_in_len}, M, w.c_part, w.cscan, nullptr, s), "frame buffers size scan");
    if (ok) {
        hipLaunchKernelGGL(k_fe_sizes, dim3((nb + 255u) / 256u), dim3(256), 0, s, nb, w.first, M, w.cscan, out, out_off, out_cap, out_len, status, d_result);
        if (M)
            hipLaunchKernelGGL(k_fe_emit, dim3(M), dim3(256), 0, s, w.c_owner, w.c_in_off, w.c_in_len, w.comp_len, w.crc, w.cscan, w.first, status,
                               w.stage, in, out, out_off);
        ok = c->check(hipGetLastError(), "frame buffers emit");
    }
    return ok ? SNP_OK : SNP_ERR_DEVICE;
}

uint64_t snp_frame_decode_buffers_workspace(uint32_t nstreams, uint32_t max_chunks, uint32_t max_spans)
{
    return decode_work_layout(nullptr, nstreams, max_chunks, max_spans).bytes;
}

snp_status snp_frame_decode_buffers_batch(snp_ctx* c, const uint8_t* in, const uint64_t* in_off, const uint64_t* in_len, uint32_t nstreams,
                                          uint32_t max_chunks, uint32_t max_spans, uint8_t* out, const uint64_t* out_off, const uint64_t* out_cap,
                                          uint64_t* out_len, int32_t* status, void* d_work, uint64_t* d_result)
{
    if (!c || !d_result || (nstreams && (!in || !in_off || !in_len || !out || !out_off || !out_cap || !out_len || !status || !d_work)))
        return SNP_ERR_BAD_ARG;
    DevGuard dg(c);
    if (!dg.ok) return SNP_ERR_DEVICE;
    hipStream_t s = c->stream;
    if (nstreams == 0) return result_empty(c, d_result, 4) ? SNP_OK : SNP_ERR_DEVICE;
    const DecodeWork w = decode_work_layout(d_work, nstreams, max_chunks, max_spans);
    const u32 ns = nstreams, M = max_chunks, S = max_spans;
    // the span walk: first span slot of every stream (d_result[2] = span slots needed, d_result[3] = 0), candidates, one chain per stream
    bool ok = c->check(launch_span_scan(in_len, ns, w.part, w.sfirst, d_result + 2, s), "frame buffers span scan") &&
              c->check(launch_span_walk(in, in_off, in_len, out_cap, ns, w.sfirst, S, w.sp, w.st, d_result + 3, s), "frame buffers walk");
    // first chunk slot of every stream (d_result[0] = chunk slots needed, d_result[1] = 0), then the chunk table over all max_chunks slots
    ok = ok && c->check(launch_scan(ScanPlain{w.st.nc}, ns, w.part, w.cfirst, d_result, s), "frame buffers chunk scan");
    if (ok && M) {
        if (S) hipLaunchKernelGGL(k_fd_emit, dim3(S), dim3(SNP_WAVE), 0, s, in, in_off, in_len, out_off, ns, w.sfirst, S, w.cfirst, M, w.sp, w.st, w.r);
        hipLaunchKernelGGL(k_fd_pad, dim3((M + 255u) / 256u), dim3(256), 0, s, ns, w.cfirst, M, w.r);
        // decode + CRC verify of every slot, as snp_frame_decode_chunks_device
        ok = c->check(hipGetLastError(), "frame buffers table") && c->decode_chunks(in, w.r, M, out);
        if (ok) hipLaunchKernelGGL(k_fd_fail, dim3((M + 255u) / 256u), dim3(256), 0, s, M, w.r, w.st);
    }
    if (ok) {
        hipLaunchKernelGGL(k_fd_verdict, dim3((ns + 255u) / 256u), dim3(256), 0, s, ns, w.sfirst, S, w.cfirst, M, w.st, w.r.status, out_len, status,
                           d_result);
        ok = c->check(hipGetLastError(), "frame buffers verdict");
    }
    return ok ? SNP_OK : SNP_ERR_DEVICE;
}

}  // extern "C"

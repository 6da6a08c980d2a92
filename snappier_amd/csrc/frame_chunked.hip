// frame_chunked.hip -- snp_frame_encode_chunked_batch: many Snappy framed streams in one call with a CHOSEN chunk size (1 .. 65536 input bytes per
// chunk, the unit of random access) and, when asked, the seek index of what it wrote -- the five arrays snp_frame_index_batch would give for
// the emitted streams, without the header walk.  What SnappyStreamCompressor gives for Write(chunk_bytes); Flush() in a loop
// (SnappyStreamCompressor.cs:82-97,194-261).  The encode half of frame_buffers.hip with 65536 made a parameter; at 65536 the output is that
// call's, byte for byte.  Built into libsnappier_hip_frame_chunked.so (C-ABI: include/snappier_hip_frame_chunked.h), linked against
// libsnappier_hip.so.  DESIGN.md 4.15.
//
//   scan      ceil(in_len / chunk_bytes) -> each buffer's first chunk slot (d_result[0] = slots needed)
//   plan      one thread per slot (fc_slot, frame_chunked_device.h): owner, input range, staging offset at a stride of snp_comp_stride(chunk_bytes)
//   compress  snp_ctx::launch_compress over every slot, varint on; crc: snp_launch_crc32c over every raw slot -- both as in frame_buffers.hip
//   scan      8 + payload per slot, the payload compressed only if smaller than the raw piece (CompressBlock  :212)
//   sizes     one thread per buffer: stream size, status, out_len, the identifier of an OK buffer, d_result[1] and [3]
//   index     (only when asked) scan of the OK buffers' chunk counts -> idx_first; one thread per buffer: idx_total, idx_tail, d_result[2]
//   emit      one 256-thread workgroup per fc_group(chunk_bytes) consecutive slots (64 KiB of input): header + payload of each at its buffer's
//             place, the workgroup's wavefronts taking slots in turn; with an index, the slot's row (idx_start, idx_pos)
// Nothing here allocates, reads back or synchronises: the call is capturable like the other _batch entry points.
#include "capi_internal.h"
#include "scan_tiles.h"
#include "work_carver.h"
#include "frame_chunked_device.h"
#include "../../include/snappier_hip_frame_chunked.h"

namespace {

// scan sources: the pieces of a buffer, one framed chunk's size (0 for an empty slot), the rows of a buffer (those of an OK one)
struct ScanChunks {
    const u64* __restrict__ len;
    u32 cb;
    __device__ __forceinline__ u64 operator()(u64 i) const { return fc_chunks(len[i], cb); }
};
struct ScanFramed {
    const u32* __restrict__ owner;
    const u32* __restrict__ comp_len;
    const u32* __restrict__ raw_len;
    __device__ __forceinline__ u64 operator()(u64 i) const
    {
        bool shrink;
        return owner[i] == kFcNone ? 0 : SNP_CHUNK_HEADER_LEN + payload_of(comp_len[i], raw_len[i], &shrink);
    }
};
struct ScanOkRows {
    const u64* __restrict__ first;
    const i32* __restrict__ status;
    __device__ __forceinline__ u64 operator()(u64 b) const { return status[b] == SNP_OK ? first[b + 1] - first[b] : 0; }
};

__global__ __launch_bounds__(256) void k_fc_plan(const u64* __restrict__ in_off, const u64* __restrict__ in_len, u32 nb, const u64* __restrict__ first,
                                                u32 max_chunks, u32 cb, u64 stride, u64* __restrict__ c_in_off, u32* __restrict__ c_in_len,
                                                u64* __restrict__ c_stage_off, u32* __restrict__ c_owner)
{
    const u32 c = blockIdx.x * 256u + threadIdx.x;
    if (c >= max_chunks) return;
    const FcSlot s = fc_slot(first, in_len, nb, max_chunks, cb, c);
    c_in_off[c] = s.owner == kFcNone ? 0 : in_off[s.owner] + s.off;
    c_in_len[c] = s.len;
    c_stage_off[c] = fc_stage_off(c, stride);
    c_owner[c] = s.owner;
}

// k_fe_sizes of frame_buffers.hip, plus result[3] += the OK buffers (one atomic per wavefront each)
__global__ __launch_bounds__(256) void k_fc_sizes(u32 nb, const u64* __restrict__ first, u32 max_chunks, const u64* __restrict__ cscan,
                                                 u8* __restrict__ out, const u64* __restrict__ out_off, const u64* __restrict__ out_cap,
                                                 u64* __restrict__ out_len, i32* __restrict__ status, u64* __restrict__ result)
{
    const u32 b = blockIdx.x * 256u + threadIdx.x;
    u64 ok_len = 0, ok = 0;
    if (b < nb) {
        const u64 end = first[b + 1];
        i32 st = SNP_ERR_OUTPUT_TOO_SMALL;
        u64 len = 0;
        if (end <= max_chunks) {
            const u64 size = SNP_STREAM_HEADER_LEN + (cscan[end] - cscan[first[b]]);
            if (size <= out_cap[b]) {
                u8* const dst = out + out_off[b];
                for (u32 i = 0; i < SNP_STREAM_HEADER_LEN; ++i) dst[i] = k_fc_stream_id[i];   // EnsureStreamHeaderWritten  :148-157
                st = SNP_OK;
                len = size;
                ok = 1;
            }
        }
        out_len[b] = len;
        status[b] = st;
        ok_len = len;
    }
    ok_len = wave_sum(ok_len);
    ok = wave_sum(ok);
    if ((threadIdx.x & 63u) == 0 && ok) {
        atomic_add64(result + 1, ok_len);
        atomic_add64(result + 3, ok);
    }
}

// the per-stream half of the index, by the conventions of include/snappier_hip_frame_index.h; result[2] = the rows written
__global__ __launch_bounds__(256) void k_fc_streams(u32 nb, const u64* __restrict__ in_len, const i32* __restrict__ status,
                                                   const u64* __restrict__ idx_first, u64* __restrict__ idx_total, i32* __restrict__ idx_tail,
                                                   u64* __restrict__ result)
{
    const u32 b = blockIdx.x * 256u + threadIdx.x;
    if (b == 0) result[2] = idx_first[nb];
    if (b >= nb) return;
    const bool ok = status[b] == SNP_OK;
    idx_total[b] = ok ? in_len[b] : 0;
    idx_tail[b] = ok ? SNP_OK : SNP_ERR_OUTPUT_TOO_SMALL;
}

// [type:1][len:3 LE = payload + 4][masked crc:4 LE][payload]  (:233-261) of every slot of the workgroup, each at its buffer's place: k_fe_emit over
// `group` consecutive slots, taken in turn by teams of `team` threads.  group = 1: one slot, the whole workgroup on its payload.
// idx_start != nullptr: the slot's index row too (OK buffers only, so row < ok_first[nb] <= max_chunks).
__global__ __launch_bounds__(256) void k_fc_emit(u32 max_chunks, u32 group, u32 team, u32 cb, u64 stride, const u32* __restrict__ c_owner,
                                                const u64* __restrict__ c_in_off, const u32* __restrict__ c_in_len, const u32* __restrict__ comp_len,
                                                const u32* __restrict__ crc, const u64* __restrict__ cscan, const u64* __restrict__ first,
                                                const i32* __restrict__ status, const u8* __restrict__ stage, const u8* __restrict__ in,
                                                u8* __restrict__ out, const u64* __restrict__ out_off, const u64* __restrict__ ok_first,
                                                u64* __restrict__ idx_start, u64* __restrict__ idx_pos)
{
    const u32 t = threadIdx.x % team, teams = 256u / team;
    const u64 c0 = static_cast<u64>(blockIdx.x) * group;
    const u64 c1 = c0 + group < max_chunks ? c0 + group : max_chunks;
    for (u64 cc = c0 + threadIdx.x / team; cc < c1; cc += teams) {
        const u32 c = static_cast<u32>(cc);
        const u32 b = c_owner[c];
        if (b == kFcNone || status[b] != SNP_OK) continue;
        bool shrink;
        const u32 pl = payload_of(comp_len[c], c_in_len[c], &shrink);
        const u64 pos = SNP_STREAM_HEADER_LEN + (cscan[c] - cscan[first[b]]);
        u8* const dst = out + out_off[b] + pos;
        chunk_header(dst, t, shrink ? 0u : 1u, pl, crc[c]);
        if (idx_start && t == 0) {
            const FcRow r = fc_row(ok_first[b], c - first[b], cb);
            idx_start[r.row] = r.start;
            idx_pos[r.row] = pos;
        }
        const u8* const src = shrink ? stage + fc_stage_off(c, stride) : in + c_in_off[c];
        team_copy(dst + SNP_CHUNK_HEADER_LEN, src, pl, t, team);
    }
}

// workspace (every piece 256-byte aligned; nothing when there is no buffer): frame_buffers.hip's encode pieces, the staging at the chunk size's stride
struct ChunkedWork {
    u64 *first, *first_part, *c_in_off, *c_stage_off, *cscan, *c_part;
    u32 *c_in_len, *comp_len, *c_owner, *crc;
    i32* c_status;
    u8* stage;
    u64 bytes;
};
ChunkedWork work_layout(void* base, u32 nbuffers, u32 max_chunks, u32 chunk_bytes)
{
    ChunkedWork w{};
    if (nbuffers == 0 || chunk_bytes == 0 || chunk_bytes > SNP_BLOCK_SIZE) return w;
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
    w.stage = k.take<u8>(nc * snp_comp_stride(chunk_bytes));
    w.bytes = k.bytes();
    return w;
}

}  // namespace

extern "C" {

uint64_t snp_frame_encode_chunked_workspace(uint32_t nbuffers, uint32_t max_chunks, uint32_t chunk_bytes)
{
    return work_layout(nullptr, nbuffers, max_chunks, chunk_bytes).bytes;
}

snp_status snp_frame_encode_chunked_batch(snp_ctx* c, const uint8_t* in, const uint64_t* in_off, const uint64_t* in_len, uint32_t nbuffers,
                                          uint32_t chunk_bytes, uint32_t max_chunks, uint8_t* out, const uint64_t* out_off, const uint64_t* out_cap,
                                          uint64_t* out_len, int32_t* status, uint64_t* idx_first, uint64_t* idx_start, uint64_t* idx_pos,
                                          uint64_t* idx_total, int32_t* idx_tail, void* d_work, uint64_t* d_result)
{
    const int given = (idx_first != nullptr) + (idx_start != nullptr) + (idx_pos != nullptr) + (idx_total != nullptr) + (idx_tail != nullptr);
    if (!c || !d_result || chunk_bytes == 0 || chunk_bytes > SNP_BLOCK_SIZE || (given != 0 && given != 5) ||
        (nbuffers && (!in || !in_off || !in_len || !out || !out_off || !out_cap || !out_len || !status || !d_work)))
        return SNP_ERR_BAD_ARG;
    const bool index = given == 5;
    DevGuard dg(c);
    if (!dg.ok) return SNP_ERR_DEVICE;
    hipStream_t s = c->stream;
    // d_result[2] and [3] start at zero (the first scan sets [0] and clears [1]); an empty batch has no row: idx_first[0] = 0 is all its index
    bool ok = c->check(snp_zero_words_async(reinterpret_cast<u32*>(d_result), 8, s), "frame chunked result");
    if (nbuffers == 0) {
        if (ok && index) ok = c->check(snp_zero_words_async(reinterpret_cast<u32*>(idx_first), 2, s), "frame chunked empty index");
        return ok ? SNP_OK : SNP_ERR_DEVICE;
    }
    const ChunkedWork w = work_layout(d_work, nbuffers, max_chunks, chunk_bytes);
    const u32 nb = nbuffers, M = max_chunks, cb = chunk_bytes;
    const u64 stride = snp_comp_stride(cb);
    // plan: first chunk slot of every buffer (d_result[0] = slots needed, d_result[1] = 0), then the chunk table over all max_chunks slots
    ok = ok && c->check(launch_scan(ScanChunks{in_len, cb}, nb, w.first_part, w.first, d_result, s), "frame chunked scan");
    if (ok && M) {
        hipLaunchKernelGGL(k_fc_plan, dim3((M + 255u) / 256u), dim3(256), 0, s, in_off, in_len, nb, w.first, M, cb, stride, w.c_in_off, w.c_in_len,
                           w.c_stage_off, w.c_owner);
        // CompressBlock: TryCompress(piece) = varint + one fragment (SnappyStreamCompressor.cs:206), every slot; then the masked CRC-32C of every RAW piece
        ok = c->check(hipGetLastError(), "frame chunked plan") &&
             c->launch_compress(in, w.c_in_off, w.c_in_len, M, w.stage, w.c_stage_off, w.comp_len, w.c_status, 1) &&
             c->check(snp_launch_crc32c(in, w.c_in_off, w.c_in_len, M, 1 | c->crc_bits(), w.crc, nullptr, nullptr, s), "frame chunked crc");
    }
    // the framed chunk sizes, then every buffer's size and status; the index of the OK buffers; then the chunks (and their rows) to their places
    ok = ok && c->check(launch_scan(ScanFramed{w.c_owner, w.comp_len, w.c_in_len}, M, w.c_part, w.cscan, nullptr, s), "frame chunked size scan");
    if (ok) {
        hipLaunchKernelGGL(k_fc_sizes, dim3((nb + 255u) / 256u), dim3(256), 0, s, nb, w.first, M, w.cscan, out, out_off, out_cap, out_len, status, d_result);
        ok = c->check(hipGetLastError(), "frame chunked sizes");
    }
    if (ok && index) {
        ok = c->check(launch_scan(ScanOkRows{w.first, status}, nb, w.first_part, idx_first, nullptr, s), "frame chunked row scan");
        if (ok) {
            hipLaunchKernelGGL(k_fc_streams, dim3((nb + 255u) / 256u), dim3(256), 0, s, nb, in_len, status, idx_first, idx_total, idx_tail, d_result);
            ok = c->check(hipGetLastError(), "frame chunked streams");
        }
    }
    if (ok && M) {
        const u32 group = fc_group(cb);
        hipLaunchKernelGGL(k_fc_emit, dim3((M + group - 1) / group), dim3(256), 0, s, M, group, fc_team(group), cb, stride, w.c_owner, w.c_in_off,
                           w.c_in_len, w.comp_len, w.crc, w.cscan, w.first, status, w.stage, in, out, out_off, index ? idx_first : nullptr,
                           index ? idx_start : nullptr, index ? idx_pos : nullptr);
        ok = c->check(hipGetLastError(), "frame chunked emit");
    }
    return ok ? SNP_OK : SNP_ERR_DEVICE;
}

}  // extern "C"

// buffers.hip -- snp_compress_buffers_batch: many device buffers of ANY length, each compressed to ONE Snappy block
// (SnappyCompressor.TryCompress  SnappyCompressor.cs:24-83: varint of the whole length, then one CompressFragment per 65536 bytes, back to back),
// entirely on the device.  The host-pointer snp_try_compress does the same job for one buffer with a read-back and a host prefix sum
// (capi_host.hip, compress_spans); here the fragments of all buffers are compressed in one launch of the existing compressor (capi_batch.hip,
// launch_compress with the varint off, into a fixed-stride staging area), and the plan before it and the emit after it are kernels:
//   scan    exclusive prefix sums, reduce-then-scan across workgroups (scan_tiles.h, tiles of 1024 values): fragments per buffer
//           (ceil(len / 65536)) -> each buffer's first fragment; compressed length per fragment -> each fragment's place in its block
//   plan    one thread per fragment slot: owning buffer (owner_of over the first-fragment table), input range, staging offset;
//           slots past the batch's fragments, and the fragments of buffers that do not fit in max_fragments, become empty fragments
//   sizes   one thread per buffer: block size, status, out_len, the varint preamble, and the batch totals of d_result
//   emit    one 256-thread workgroup per FRAGMENT (k_gather's copy), so a 4 GiB buffer is copied by 65 536 workgroups, not by one CU
// Nothing here allocates, reads back or synchronises: the call is capturable like the other _batch entry points.  Built into
// libsnappier_hip_buffers.so (C-ABI: include/snappier_hip_buffers.h), which is linked against libsnappier_hip.so and drives its contexts
// through the same snp_ctx members as capi_batch.hip.  DESIGN.md 4.9.
#include "capi_internal.h"
#include "scan_tiles.h"
#include "work_carver.h"
#include "../../include/snappier_hip_buffers.h"

namespace {

constexpr u32 kNoOwner = 0xffffffffu;

__global__ __launch_bounds__(256) void k_buffers_plan(const u64* __restrict__ in_off, const u32* __restrict__ in_len, u32 nbuffers,
                                                     const u64* __restrict__ first, u32 max_fragments, u64 stage_stride,
                                                     u64* __restrict__ frag_in_off, u32* __restrict__ frag_in_len,
                                                     u64* __restrict__ frag_stage_off, u32* __restrict__ frag_owner)
{
    const u32 f = blockIdx.x * 256u + threadIdx.x;
    if (f >= max_fragments) return;
    u64 io = 0;
    u32 il = 0, owner = kNoOwner;
    if (f < first[nbuffers]) {
        const u32 lo = owner_of(first, nbuffers, f);                    // first[lo] <= f < first[lo + 1]
        if (first[lo + 1] <= max_fragments) {                          // else the buffer does not fit: its slots stay empty
            const u64 k = f - first[lo];
            const u32 n = in_len[lo];
            io = in_off[lo] + k * SNP_BLOCK_SIZE;
            il = n - k * SNP_BLOCK_SIZE < SNP_BLOCK_SIZE ? static_cast<u32>(n - k * SNP_BLOCK_SIZE) : SNP_BLOCK_SIZE;
            owner = lo;
        }
    }
    frag_in_off[f] = io;
    frag_in_len[f] = il;
    frag_stage_off[f] = static_cast<u64>(f) * stage_stride;
    frag_owner[f] = owner;
}

__device__ __forceinline__ u32 varint_len(u32 n)                       // VarIntEncoding.TryWrite  VarIntEncoding.Write.cs:5-79
{
    return n < (1u << 7) ? 1u : n < (1u << 14) ? 2u : n < (1u << 21) ? 3u : n < (1u << 28) ? 4u : 5u;
}

// Block size = varint + the buffer's fragments; OK only when every fragment was planned and the block fits out_cap.  Only an OK buffer's
// range is written (its varint here, its fragments by k_buffers_emit); result[1] += the OK sizes (one atomic per wavefront).
__global__ __launch_bounds__(256) void k_buffers_sizes(const u32* __restrict__ in_len, u32 nbuffers, const u64* __restrict__ first,
                                                      u32 max_fragments, const u64* __restrict__ frag_scan, u8* __restrict__ out,
                                                      const u64* __restrict__ out_off, const u64* __restrict__ out_cap,
                                                      u64* __restrict__ out_len, i32* __restrict__ status, u64* __restrict__ result)
{
    const u32 b = blockIdx.x * 256u + threadIdx.x;
    u64 ok_len = 0;
    if (b < nbuffers) {
        const u32 n = in_len[b];
        const u64 end = first[b + 1];
        i32 st = SNP_ERR_OUTPUT_TOO_SMALL;                              // TryCompress returns false  SnappyCompressor.cs:63-68
        u64 len = 0;
        if (end <= max_fragments) {
            const u32 hb = varint_len(n);
            const u64 size = hb + (frag_scan[end] - frag_scan[first[b]]);
            if (size <= out_cap[b]) {
                u8* dst = out + out_off[b];
                for (u32 i = 0; i < hb; ++i) dst[i] = static_cast<u8>((n >> (7 * i)) | (i + 1 < hb ? 0x80u : 0u));
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

// One workgroup per fragment slot: the staged fragment to its place in its buffer's block.
__global__ __launch_bounds__(256) void k_buffers_emit(const u32* __restrict__ frag_owner, const u32* __restrict__ frag_comp_len,
                                                     const u64* __restrict__ frag_scan, const u64* __restrict__ first,
                                                     const u32* __restrict__ in_len, const i32* __restrict__ status,
                                                     const u8* __restrict__ stage, u64 stage_stride, u8* __restrict__ out,
                                                     const u64* __restrict__ out_off)
{
    const u32 f = blockIdx.x;
    const u32 b = frag_owner[f];
    if (b == kNoOwner || status[b] != SNP_OK) return;
    const u64 o = out_off[b] + varint_len(in_len[b]) + (frag_scan[f] - frag_scan[first[b]]);
    block_copy(out + o, stage + static_cast<u64>(f) * stage_stride, frag_comp_len[f], threadIdx.x);
}

// d_work layout (every piece 256-byte aligned).  Per buffer: first fragment (nbuffers + 1, the last = fragments needed) and the tile sums of
// its scan; per fragment slot: input offset and length, staging offset, compressed length, status, owning buffer, the scan of the compressed
// lengths (max_fragments + 1) and its tile sums; then the staging area, kSnpCompStride bytes per slot (the compressor's output bound, padded).
struct BuffersWork {
    u64 *first, *first_part, *frag_in_off, *frag_stage_off, *frag_scan, *frag_part;
    u32 *frag_in_len, *frag_comp_len, *frag_owner;
    i32* frag_status;
    u8* stage;
    u64 bytes;
};
BuffersWork buffers_work_layout(void* base, u32 nbuffers, u32 max_fragments)
{
    BuffersWork w{};
    if (nbuffers == 0) return w;                                         // (nothing is launched but the result)
    const u64 nb = nbuffers, nf = max_fragments;
    WorkCarver k(base);
    w.first = k.take<u64>(nb + 1);
    w.first_part = k.take<u64>(scan_tiles_of(nb));
    w.frag_scan = k.take<u64>(nf + 1);
    w.frag_part = k.take<u64>(scan_tiles_of(nf));
    w.frag_in_off = k.take<u64>(nf);
    w.frag_stage_off = k.take<u64>(nf);
    w.frag_in_len = k.take<u32>(nf);
    w.frag_comp_len = k.take<u32>(nf);
    w.frag_owner = k.take<u32>(nf);
    w.frag_status = k.take<i32>(nf);
    w.stage = k.take<u8>(nf * kSnpCompStride);
    w.bytes = k.bytes();
    return w;
}

}  // namespace

extern "C" {

uint64_t snp_compress_buffers_workspace(uint32_t nbuffers, uint32_t max_fragments)
{
    return buffers_work_layout(nullptr, nbuffers, max_fragments).bytes;
}

snp_status snp_compress_buffers_batch(snp_ctx* c, const uint8_t* in, const uint64_t* in_off, const uint32_t* in_len, uint32_t nbuffers,
                                      uint32_t max_fragments, uint8_t* out, const uint64_t* out_off, const uint64_t* out_cap,
                                      uint64_t* out_len, int32_t* status, void* d_work, uint64_t* d_result)
{
    if (!c || !d_result || (nbuffers && (!in || !in_off || !in_len || !out || !out_off || !out_cap || !out_len || !status || !d_work)))
        return SNP_ERR_BAD_ARG;
    DevGuard dg(c);
    if (!dg.ok) return SNP_ERR_DEVICE;
    hipStream_t s = c->stream;
    if (nbuffers == 0)
        return c->check(snp_zero_words_async(reinterpret_cast<u32*>(d_result), 2 * 2u, s), "buffers result") ? SNP_OK : SNP_ERR_DEVICE;   // 2 u64 words
    const BuffersWork w = buffers_work_layout(d_work, nbuffers, max_fragments);
    const u32 nb = nbuffers, M = max_fragments;
    // plan: first fragment of every buffer (d_result = {fragments needed, 0}), then the fragment table over all max_fragments slots
    bool ok = c->check(launch_scan(ScanFrags{in_len}, nb, w.first_part, w.first, d_result, s), "buffers scan");
    if (ok && M) {
        hipLaunchKernelGGL(k_buffers_plan, dim3((M + 255u) / 256u), dim3(256), 0, s, in_off, in_len, nb, w.first, M, kSnpCompStride, w.frag_in_off,
                           w.frag_in_len, w.frag_stage_off, w.frag_owner);
        // compress: every slot, the empty ones included (the count picks the layout: DESIGN.md 4.9), no varint -- CompressFragment only
        ok = c->check(hipGetLastError(), "buffers plan") &&
             c->launch_compress(in, w.frag_in_off, w.frag_in_len, M, w.stage, w.frag_stage_off, w.frag_comp_len, w.frag_status, 0);
    }
    // the scan of the compressed lengths, the sizes, then the fragments to their places (a buffer that is not OK is not written at all)
    ok = ok && c->check(launch_scan(ScanPlain{w.frag_comp_len}, M, w.frag_part, w.frag_scan, nullptr, s), "fragment scan");
    if (ok) {
        hipLaunchKernelGGL(k_buffers_sizes, dim3((nb + 255u) / 256u), dim3(256), 0, s, in_len, nb, w.first, M, w.frag_scan, out, out_off, out_cap,
                           out_len, status, d_result);
        ok = c->check(hipGetLastError(), "buffers sizes");
    }
    if (ok && M) {
        hipLaunchKernelGGL(k_buffers_emit, dim3(M), dim3(256), 0, s, w.frag_owner, w.frag_comp_len, w.frag_scan, w.first, in_len, status, w.stage,
                           kSnpCompStride, out, out_off);
        ok = c->check(hipGetLastError(), "buffers emit");
    }
    return ok ? SNP_OK : SNP_ERR_DEVICE;
}

}  // extern "C"

// buffers.hip -- device side of snp_compress_buffers_batch: many inputs of ANY length, each one Snappy block
// (SnappyCompressor.TryCompress  SnappyCompressor.cs:24-83: varint of the whole length, then one CompressFragment per 65536 bytes, back to back).
// The fragments of all buffers are compressed in one launch of the existing compressor (capi_batch.hip, launch_compress with the varint off,
// into a fixed-stride staging area); what is here is the plan before it and the emit after it:
//   scan    exclusive prefix sums, reduce-then-scan across workgroups (scan_tiles.h, tiles of 1024 values): fragments per buffer
//           (ceil(len / 65536)) -> each buffer's first fragment; compressed length per fragment -> each fragment's place in its block
//   plan    one thread per fragment slot: owning buffer (binary search over the first-fragment table), input range, staging offset;
//           slots past the batch's fragments, and the fragments of buffers that do not fit in max_fragments, become empty fragments
//   sizes   one thread per buffer: block size, status, out_len, the varint preamble, and the batch totals of d_result
//   emit    one 256-thread workgroup per FRAGMENT (k_gather's copy), so a 4 GiB buffer is copied by 65 536 workgroups, not by one CU
// Nothing here allocates or synchronises: the calls are capturable like the other _batch entry points.
#include "scan_tiles.h"

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
        // the buffer b with first[b] <= f < first[b + 1] (first[0] = 0 <= f < first[nbuffers] holds throughout)
        u32 lo = 0, hi = nbuffers;
        while (hi - lo > 1) {
            const u32 mid = lo + (hi - lo) / 2;
            if (first[mid] <= f) lo = mid;
            else hi = mid;
        }
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
    for (u32 d = 32; d >= 1; d >>= 1) ok_len += __shfl_xor(ok_len, d, 64);
    if ((threadIdx.x & 63u) == 0 && ok_len) atomicAdd(reinterpret_cast<unsigned long long*>(result + 1), static_cast<unsigned long long>(ok_len));
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

__global__ void k_buffers_result_empty(u64* result)
{
    if (threadIdx.x < 2) result[threadIdx.x] = 0;
}

}  // namespace

extern "C" {

// first[0 .. nbuffers] = exclusive scan of ceil(in_len / 65536); result = {fragments needed, 0}
hipError_t snp_launch_buffers_first(const u32* in_len, u32 nbuffers, u64* partial, u64* first, u64* result, hipStream_t stream)
{
    return launch_scan(ScanFrags{in_len}, nbuffers, partial, first, result, stream);
}

hipError_t snp_launch_buffers_plan(const u64* in_off, const u32* in_len, u32 nbuffers, const u64* first, u32 max_fragments, u64 stage_stride,
                                   u64* frag_in_off, u32* frag_in_len, u64* frag_stage_off, u32* frag_owner, hipStream_t stream)
{
    if (max_fragments == 0) return hipSuccess;
    hipLaunchKernelGGL(k_buffers_plan, dim3((max_fragments + 255u) / 256u), dim3(256), 0, stream, in_off, in_len, nbuffers, first, max_fragments,
                       stage_stride, frag_in_off, frag_in_len, frag_stage_off, frag_owner);
    return hipGetLastError();
}

// frag_scan[0 .. nfrag] = exclusive scan of the compressed lengths
hipError_t snp_launch_buffers_frag_scan(const u32* comp_len, u32 nfrag, u64* partial, u64* frag_scan, hipStream_t stream)
{
    return launch_scan(ScanPlain{comp_len}, nfrag, partial, frag_scan, nullptr, stream);
}

hipError_t snp_launch_buffers_sizes(const u32* in_len, u32 nbuffers, const u64* first, u32 max_fragments, const u64* frag_scan, u8* out,
                                    const u64* out_off, const u64* out_cap, u64* out_len, i32* status, u64* result, hipStream_t stream)
{
    if (nbuffers == 0) return hipSuccess;
    hipLaunchKernelGGL(k_buffers_sizes, dim3((nbuffers + 255u) / 256u), dim3(256), 0, stream, in_len, nbuffers, first, max_fragments, frag_scan,
                       out, out_off, out_cap, out_len, status, result);
    return hipGetLastError();
}

hipError_t snp_launch_buffers_emit(const u32* frag_owner, const u32* frag_comp_len, const u64* frag_scan, const u64* first, const u32* in_len,
                                   const i32* status, const u8* stage, u64 stage_stride, u8* out, const u64* out_off, u32 max_fragments,
                                   hipStream_t stream)
{
    if (max_fragments == 0) return hipSuccess;
    hipLaunchKernelGGL(k_buffers_emit, dim3(max_fragments), dim3(256), 0, stream, frag_owner, frag_comp_len, frag_scan, first, in_len, status,
                       stage, stage_stride, out, out_off);
    return hipGetLastError();
}

hipError_t snp_launch_buffers_result_empty(u64* result, hipStream_t stream)
{
    hipLaunchKernelGGL(k_buffers_result_empty, dim3(1), dim3(64), 0, stream, result);
    return hipGetLastError();
}

}  // extern "C"

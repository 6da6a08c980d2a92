// scan_tiles.h -- exclusive prefix sums of u64 values over up to 2^32 positions, reduce-then-scan across workgroups (tiles of SNP_SCAN_TILE values):
// the plan scans of the batch extension libraries (buffers.hip, buffers_decode.hip, frame_buffers.hip, layout.hip, frame_range.hip, frame_index.hip), and owner_of, their inverse.  What is scanned is a functor V: V(i) = the value at position i, so a scan
// reads its source as the caller's kernels see it (fragments of a length, a masked length, a packed pair of counts) with no array in between.
// Three launches; the partial array holds one tile sum per tile (+ 1), dst holds n + 1 values (dst[n] = the grand total).
#pragma once
#include "snp_device.h"

namespace {

constexpr u32 kScanThreads = 256;
constexpr u32 kScanItems = 4;
constexpr u32 kScanTile = SNP_SCAN_TILE;                  // values per workgroup (snp_device.h: the workspace holds one tile sum per tile)
static_assert(kScanTile == kScanThreads * kScanItems, "scan tile");

// the two sources of buffers.hip: fragments of a buffer of src[i] bytes, or src[i] itself
struct ScanFrags {
    const u32* __restrict__ src;
    __device__ __forceinline__ u64 operator()(u64 i) const { return (static_cast<u64>(src[i]) + SNP_BLOCK_SIZE - 1) / SNP_BLOCK_SIZE; }
};
struct ScanPlain {
    const u32* __restrict__ src;
    __device__ __forceinline__ u64 operator()(u64 i) const { return src[i]; }
};

// Exclusive scan of one u64 per thread over a 256-thread workgroup; *total = the workgroup's sum.  All threads must call it.
__device__ __forceinline__ u64 wg_exclusive_scan(u64 v, u64* total)
{
    __shared__ u64 wave_sum[kScanThreads / SNP_WAVE];
    const u32 tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    u64 x = v;
    for (u32 d = 1; d < 64; d <<= 1) {
        const u64 y = __shfl_up(x, d, 64);
        if (lane >= d) x += y;
    }
    if (lane == 63) wave_sum[wave] = x;
    __syncthreads();
    u64 before = 0, all = 0;
    for (u32 w = 0; w < kScanThreads / SNP_WAVE; ++w) {
        before += w < wave ? wave_sum[w] : 0;
        all += wave_sum[w];
    }
    __syncthreads();                                                    // (wave_sum is reused by the next call)
    *total = all;
    return before + x - v;
}

// pass 1: the sum of each tile
template <class V>
__global__ __launch_bounds__(kScanThreads) void k_scan_reduce(const V val, u32 n, u64* __restrict__ partial)
{
    const u64 base = static_cast<u64>(blockIdx.x) * kScanTile + threadIdx.x * kScanItems;
    u64 s = 0;
    for (u32 k = 0; k < kScanItems; ++k)
        if (base + k < n) s += val(base + k);
    u64 total;
    (void)wg_exclusive_scan(s, &total);
    if (threadIdx.x == 0) partial[blockIdx.x] = total;
}

// pass 2 (one workgroup): tile sums -> tile offsets in place; dst[n] = the grand total.  result != nullptr: result[0] = the total,
// result[1] = 0 (the sizes kernel adds to it later on the stream)
__global__ __launch_bounds__(kScanThreads) void k_scan_partials(u64* __restrict__ partial, u32 ntiles, u64* __restrict__ dst_total,
                                                               u64* __restrict__ result)
{
    u64 carry = 0;
    for (u32 base = 0; base < ntiles; base += kScanThreads) {
        const u32 i = base + threadIdx.x;
        const u64 v = i < ntiles ? partial[i] : 0;
        u64 total;
        const u64 excl = wg_exclusive_scan(v, &total);
        if (i < ntiles) partial[i] = carry + excl;
        carry += total;
    }
    if (threadIdx.x == 0) {
        *dst_total = carry;
        if (result) {
            result[0] = carry;
            result[1] = 0;
        }
    }
}

// pass 3: each tile scanned again, offset by its tile's place
template <class V>
__global__ __launch_bounds__(kScanThreads) void k_scan_tiles(const V val, u32 n, const u64* __restrict__ partial, u64* __restrict__ dst)
{
    const u64 base = static_cast<u64>(blockIdx.x) * kScanTile + threadIdx.x * kScanItems;
    u64 v[kScanItems], s = 0;
    for (u32 k = 0; k < kScanItems; ++k) {
        v[k] = base + k < n ? val(base + k) : 0;
        s += v[k];
    }
    u64 total;
    u64 run = partial[blockIdx.x] + wg_exclusive_scan(s, &total);
    for (u32 k = 0; k < kScanItems; ++k) {
        if (base + k < n) dst[base + k] = run;
        run += v[k];
    }
}

// dst[0 .. n] = exclusive scan of val(0 .. n - 1), dst[n] = the total (and result[0], result[1] = 0 when result != nullptr)
template <class V>
hipError_t launch_scan(const V val, u32 n, u64* partial, u64* dst, u64* result, hipStream_t stream)
{
    const u32 ntiles = static_cast<u32>((static_cast<u64>(n) + kScanTile - 1) / kScanTile);
    if (ntiles) hipLaunchKernelGGL((k_scan_reduce<V>), dim3(ntiles), dim3(kScanThreads), 0, stream, val, n, partial);
    hipLaunchKernelGGL(k_scan_partials, dim3(1), dim3(kScanThreads), 0, stream, partial, ntiles, dst + n, result);
    if (ntiles) hipLaunchKernelGGL((k_scan_tiles<V>), dim3(ntiles), dim3(kScanThreads), 0, stream, val, n, partial, dst);
    return hipGetLastError();
}

// values the `partial` array of a scan over n positions holds (one tile sum per tile, + 1)
inline u64 scan_tiles_of(u64 n) { return (n + kScanTile - 1) / kScanTile + 1; }

// The inverse of the scan: the last b in [0, nb) with key(b) <= t (key non-decreasing, key(0) = 0) -- the owner of slot t < key(nb).
template <class K>
__device__ __forceinline__ u32 owner_of(K key, u32 nb, u64 t)
{
    u32 lo = 0, hi = nb;
    while (hi - lo > 1) {
        const u32 mid = lo + (hi - lo) / 2;
        if (key(mid) <= t) lo = mid;
        else hi = mid;
    }
    return lo;
}
// ... over a plain table of first slots (the dst of launch_scan)
__device__ __forceinline__ u32 owner_of(const u64* __restrict__ first, u32 nb, u64 t)
{
    return owner_of([=](u32 b) { return first[b]; }, nb, t);
}

}  // namespace

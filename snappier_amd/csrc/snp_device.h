// snp_device.h -- shared device-side helpers for the gfx950 Snappy block codec kernels.
// One 64-lane wavefront owns one Snappy block; everything here is wave-level (no __syncthreads anywhere).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/snappier_hip.h"

typedef uint8_t u8;
typedef uint16_t u16;
typedef uint32_t u32;
typedef uint64_t u64;
typedef int32_t i32;

#define SNP_WAVE 64
#define SNP_SCAN_TILE 1024u   // values per workgroup of the multi-workgroup prefix scans (buffers.hip)

// The SNAPPIER_HIP_* environment variables are test and A/B knobs (kernel variants, layouts, thresholds): the product library reads NONE of them.
// Only variant libraries built with -DSNAPPIER_HIP_DEBUG_ENV do (scripts/build_variant.sh, LAB=1: snappier_amd/variants/, loaded by A/B scripts on request; no test loads one).
#ifdef SNAPPIER_HIP_DEBUG_ENV
#include <stdlib.h>
#define SNP_GETENV(name) getenv(name)
#else
#define SNP_GETENV(name) static_cast<const char*>(nullptr)
#endif

// The lane compressor's hash-table workspace (compress_lanes.hip): up to 16 separately allocated PIECES of `piece_frags` fragments' tables each
// (a multiple of 64, so a workgroup's tables never straddle two pieces); fragment f's table is table f % piece_frags of piece f / piece_frags.
// A workspace that is one allocation is one piece with piece_frags = 0xffffffc0.  Why pieces: capi_pool.hip, build_tables.
#define SNP_TABLE_PIECES_MAX 16
struct snp_table_pieces {
    uint32_t* p[SNP_TABLE_PIECES_MAX];
    uint32_t piece_frags;
    uint32_t n;
};

// Launch shape of the lane compressor (compress_lanes.hip), per context: SNP_OPT_COMPRESS_LANE_* (include/snappier_hip.h).  0 / -1 = chosen
// from the batch size and the context's hint; results never depend on it (tests/test_gpu_parity.py runs every combination against the oracle).
struct snp_lane_tuning {
    int lanes_per_wave;   // 0 auto | 8 | 16 | 32 | 64 fragments per wavefront
    int opts;             // -1 auto | a mask of the kernel's kOpt* bits (0..255)
    int probes;           // 0 auto | 1..4 probes of one lane's scan issued together
    int small_bytes;      // -1 auto (the hint) | 0 never | LDS slot bytes of the launch that keeps small fragments' input in LDS (<= 2048)
    int small_lanes;      // 0 auto (32) | 16 | 32 | 64 lanes per wavefront of that launch
    int hint;             // what the context learnt from its previous batch: 32 = fragments <= 512 B, 256 = <= 4 KiB, bits 9-14 = (longest + 15) / 16 when in (80, 768]
};

// Unaligned little-endian accesses.  gfx950 under HSA runs in unaligned-access mode, so a dword access at any byte
// address is one global_load_dword / global_store_dword (the packed struct tells the compiler align = 1).
struct __attribute__((packed)) snp_u32_unaligned { u32 v; };
struct __attribute__((packed)) snp_u64_unaligned { u64 v; };
struct __attribute__((packed)) snp_u128_unaligned { u32 v[4]; };

__device__ __forceinline__ u32 ld32u(const u8* p) { return reinterpret_cast<const snp_u32_unaligned*>(p)->v; }
__device__ __forceinline__ u64 ld64u(const u8* p) { return reinterpret_cast<const snp_u64_unaligned*>(p)->v; }
__device__ __forceinline__ void st32u(u8* p, u32 v) { reinterpret_cast<snp_u32_unaligned*>(p)->v = v; }

__device__ __forceinline__ u32 lane_id() { return __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u)); }
__device__ __forceinline__ u64 ballot64(bool p) { return __ballot(p); }
__device__ __forceinline__ u32 bcast_first(u32 v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ u32 read_lane(u32 v, u32 lane) { return __builtin_amdgcn_readlane(v, lane); }
// 64-bit masks: lanes strictly below `lane`
__device__ __forceinline__ u64 lanes_below(u32 lane) { return lane >= 64 ? ~0ull : ((1ull << lane) - 1ull); }

// Reductions over the wavefront (every lane gets the result) and the 64-bit atomics that take it to a result word: the tails of the plan and
// verdict kernels of the batch extension libraries ("one atomic per wavefront").  All lanes must call the reductions.
__device__ __forceinline__ u64 wave_min(u64 v)
{
    for (u32 d = 32; d >= 1; d >>= 1) {
        const u64 o = __shfl_xor(v, d, 64);
        v = o < v ? o : v;
    }
    return v;
}
__device__ __forceinline__ u64 wave_max(u64 v)
{
    for (u32 d = 32; d >= 1; d >>= 1) {
        const u64 o = __shfl_xor(v, d, 64);
        v = o > v ? o : v;
    }
    return v;
}
__device__ __forceinline__ u64 wave_sum(u64 v)
{
    for (u32 d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}
__device__ __forceinline__ void atomic_min64(u64* p, u64 v) { atomicMin(reinterpret_cast<unsigned long long*>(p), static_cast<unsigned long long>(v)); }
__device__ __forceinline__ void atomic_max64(u64* p, u64 v) { atomicMax(reinterpret_cast<unsigned long long*>(p), static_cast<unsigned long long>(v)); }
__device__ __forceinline__ void atomic_add64(u64* p, u64 v) { atomicAdd(reinterpret_cast<unsigned long long*>(p), static_cast<unsigned long long>(v)); }

// Wave-wide memcpy for a wave-uniform (dst, src, len): 16 B per lane per step while a full 1 KiB remains, then
// 4 B per lane, then a byte tail.  src and dst must not overlap.  All lanes must call it.
__device__ __forceinline__ void wave_copy(u8* dst, const u8* src, u32 len, u32 lane)
{
    u32 done = 0;
    while (len - done >= 1024) {
        snp_u128_unaligned w = *reinterpret_cast<const snp_u128_unaligned*>(src + done + lane * 16);
        *reinterpret_cast<snp_u128_unaligned*>(dst + done + lane * 16) = w;
        done += 1024;
    }
    while (len - done >= 256) {
        st32u(dst + done + lane * 4, ld32u(src + done + lane * 4));
        done += 256;
    }
#pragma clang loop vectorize(disable) unroll(disable)
    for (u32 k = done + lane; k < len; k += 64) dst[k] = src[k];   // (< 256 bytes: at most four trips -- not worth the unrolled code)
}

// Copy len bytes with a whole 256-thread workgroup (no overlap): 16 B per lane per step, then a byte tail.  All threads must call it.
__device__ __forceinline__ void block_copy(u8* dst, const u8* src, u32 len, u32 tid)
{
    u32 k = tid * 16;
    for (; k + 16 <= len; k += 256 * 16) {
        snp_u128_unaligned w = *reinterpret_cast<const snp_u128_unaligned*>(src + k);
        *reinterpret_cast<snp_u128_unaligned*>(dst + k) = w;
    }
    const u32 tail = len & ~15u;
    if (tid < (len & 15u)) dst[tail + tid] = src[tail + tid];
}

// Framing mask  Crc32CAlgorithm.ApplyMask  (Snappier/Internal/Crc32CAlgorithm.cs:156-158)
__host__ __device__ __forceinline__ u32 crc32c_mask(u32 x) { return ((x >> 15) | (x << 17)) + 0xa282ead8u; }

// The eight header bytes of a framed chunk, [type:1][len:3 LE = payload + 4][masked crc:4 LE], by the first 8 threads of a team (t: the
// thread's place in it).  type: 0 compressed, 1 uncompressed.  The one writer of the format: every emit kernel calls it.
__device__ __forceinline__ void chunk_header(u8* at, u32 t, u32 type, u32 pl, u32 crc)
{
    if (t < SNP_CHUNK_HEADER_LEN) {
        const u32 bs = pl + 4;                                          // SnappyStreamCompressor.cs:236,251
        const u32 v = t == 0 ? type : t < 4 ? (bs >> (8 * (t - 1))) : (crc >> (8 * (t - 4)));
        at[t] = static_cast<u8>(v);
    }
}

// A few control words set to zero ON THE STREAM.  Not hipMemsetAsync: as a node of a captured hipGraph a 4-byte memset runs on the first launch of the
// graph only (ROCm 7.0, scripts/probe_graph_memset.py), and the batch entry points are meant to be capturable (tests/test_gpu_graph_capture.py).
namespace {
__global__ void k_zero_words(u32* p, u32 n)
{
    for (u32 i = threadIdx.x; i < n; i += blockDim.x) p[i] = 0u;
}
}  // namespace
static inline hipError_t snp_zero_words_async(u32* p, u32 n, hipStream_t stream)
{
    hipLaunchKernelGGL(k_zero_words, dim3(1), dim3(64), 0, stream, p, n);
    return hipGetLastError();
}

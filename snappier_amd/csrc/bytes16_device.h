// bytes16_device.h -- the compare of 16 bytes at any alignment, stated once: where two 16-byte words first differ.  The compare kernel of the
// diff (frame_diff.hip: the first mismatch of two decoded runs, in either direction) and the chunk compare of the dedup (frame_dedup_device.h:
// are two chunks the same bytes) are both made of it.  __host__ __device__, so that the CPU checks of tests/abi run the same code.
#pragma once
#include "snp_device.h"

namespace {

// the first of 16 bytes (in the direction) at which two words differ, 16 if none
__host__ __device__ __forceinline__ u32 first_diff16(const snp_u128_unaligned& x, const snp_u128_unaligned& y, u32 dir)
{
    const u64 lo = (x.v[0] ^ y.v[0]) | static_cast<u64>(x.v[1] ^ y.v[1]) << 32, hi = (x.v[2] ^ y.v[2]) | static_cast<u64>(x.v[3] ^ y.v[3]) << 32;
    if (!(lo | hi)) return 16;
    if (!dir) return lo ? static_cast<u32>(__builtin_ctzll(lo)) >> 3 : 8u + (static_cast<u32>(__builtin_ctzll(hi)) >> 3);
    return hi ? static_cast<u32>(__builtin_clzll(hi)) >> 3 : 8u + (static_cast<u32>(__builtin_clzll(lo)) >> 3);
}

}  // namespace

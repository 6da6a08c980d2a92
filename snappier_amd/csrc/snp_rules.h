// snp_rules.h -- format rules that the host code and the kernels both apply, each stated once: the varint preamble of a block, the expansion
// bound, and the two rules of the tag index (its chunk count, and which streams skip the candidate pass).  Everything is __host__ __device__.
#pragma once
#include "snp_device.h"

// The varint preamble of a block (VarIntEncoding.TryReadSlow  VarIntEncoding.Read.cs:38-79) from its first bytes, packed little-endian, of
// which `avail` are really there.  `bytes` = bytes consumed: the preamble's length when DONE, else those before the one that stopped the read.
// (The loop is frame_hop's as it stood, flags included: in this form the header walks compile to within three instructions of what they were.)
enum : u32 {
    SNP_PRE_DONE = 0,
    SNP_PRE_SHORT = 1,       // the bytes ran out inside the varint
    SNP_PRE_OVERFLOW = 2,    // LeftShiftOverflows (Helpers.cs:65-70), or five continuation bytes (shift >= 32  :65-69)
};
struct snp_preamble { u32 value, bytes, end; };
__host__ __device__ __forceinline__ snp_preamble snp_read_preamble(u64 first, u32 avail)
{
    const u32 lim = avail < SNP_VARINT_MAX ? avail : SNP_VARINT_MAX;
    u32 result = 0, shift = 0;
    bool done = false, bad = false;
    for (u32 i = 0; i < lim && !done && !bad; ++i) {
        const u32 c = static_cast<u32>(first >> (8 * i)) & 0xffu;
        const u32 val = c & 0x7fu;
        if (val & ~(0xffffffffu >> shift)) { bad = true; break; }
        result |= val << shift;
        shift += 7;
        if (c < 128) done = true;
    }
    return snp_preamble{result, shift / 7, done ? SNP_PRE_DONE : bad || lim == SNP_VARINT_MAX ? SNP_PRE_OVERFLOW : SNP_PRE_SHORT};
}
// (a caller that holds a byte pointer: the first five of its n bytes, packed)
__host__ __device__ __forceinline__ snp_preamble snp_read_preamble(const u8* p, u64 n)
{
    const u32 avail = n < SNP_VARINT_MAX ? static_cast<u32>(n) : SNP_VARINT_MAX;
    u64 first = 0;
    for (u32 i = 0; i < avail; ++i) first |= static_cast<u64>(p[i]) << (8 * i);
    return snp_read_preamble(first, avail);
}

// No tag expands more than 3 bytes -> 64 (a copy-2 of length 64): a block that declares more than this for the bytes after its preamble can
// only end "Incomplete Snappy block.", whatever its tags say -- and must not size any allocation.
__host__ __device__ __forceinline__ u64 snp_max_expansion(u64 body_bytes) { return (body_bytes / 3 + 1) * 64; }

// The tag index (tag_index.hip) cuts the n - hb bytes after a block's preamble into chunks of 16 KiB ...
constexpr u32 SNP_TAG_CHUNK = 16384;
__host__ __device__ __forceinline__ u32 snp_tag_chunks(u32 n, u32 hb) { return (n - hb + SNP_TAG_CHUNK - 1) / SNP_TAG_CHUNK; }
// ... and skips its candidate pass for a stream of >= 85 % of its output: mostly literals longer than a chunk (hardly compressed data), where
// the pass would fail anyway.
__host__ __device__ __forceinline__ bool snp_look_back_only(u32 n, u32 expected) { return static_cast<u64>(n) * 100 >= static_cast<u64>(expected) * 85; }

// frame_cuts_device.h -- the rules of libsnappier_hip_frame_cuts.so (frame_cuts.hip), stated once: where the content-defined cuts of a buffer
// are (snp_content_cuts_batch), and when a cut list that a caller hands to the encoder is good (snp_frame_encode_cuts_batch).  __host__
// __device__ throughout: the kernels call these functions, and the same text runs on the CPU under sanitizers
// (tests/abi/frame_cuts_rule_check.hip), on offsets past 4 GiB too.  DESIGN.md 4.26.
//
// The cut rule, for a buffer x of n bytes and the parameters window w (32 .. 32 767) and max_bytes mx (w < mx <= 65 536):
//   GEAR[b] = fmix32((b + 1) * 0x9E3779B9)                                   (murmur3's finaliser; arithmetic, no table to keep)
//   g(0) = 0, g(c + 1) = (g(c) << 1) + GEAR[x[c]]   mod 2^32                 (so g(c) depends on x[c - 32 .. c) only)
//   c is a CONTENT cut iff  w < c < n - w,  g(c) >  g(c') for c' in [c - w, c)  and  g(c) >= g(c') for c' in (c, c + w]
//   between neighbours a < b of {0} + content cuts + {n}: every a + k * mx < b, k >= 1, is a FORCED cut
// A tie loses on the left and wins on the right, so a constant run has no content cut and two content cuts are more than w apart.
#pragma once
#include "snp_device.h"

namespace {

constexpr u32 kCutsMinWindow = 32, kCutsMaxWindow = 32767;
constexpr u32 kCutsHashBytes = 32;              // the bytes g(c) depends on
constexpr u32 kCutsBlock = 64;                  // positions one stored maximum covers
constexpr u32 kCutsTile = 4096;                 // positions one workgroup takes at a time (the finder's seam), in whole blocks
constexpr u32 kCutsRun = 17;                    // positions one lane hashes in a row (odd: its stores to LDS meet no bank twice)
constexpr u64 kCutsSpanMax = 1ull << 40;        // span_bytes is clamped to it: the tiles stay inside 32 bits
static_assert(kCutsTile % kCutsBlock == 0, "a tile is whole blocks");

__host__ __device__ __forceinline__ bool cc_params_ok(u32 w, u32 mx)
{
    return w >= kCutsMinWindow && w <= kCutsMaxWindow && mx > w && mx <= SNP_BLOCK_SIZE;
}

__host__ __device__ __forceinline__ u32 cc_fmix32(u32 h)
{
    h ^= h >> 16;
    h *= 0x85ebca6bu;
    h ^= h >> 13;
    h *= 0xc2b2ae35u;
    h ^= h >> 16;
    return h;
}
__host__ __device__ __forceinline__ u32 cc_gear(u32 b) { return cc_fmix32((b + 1u) * 0x9E3779B9u); }
__host__ __device__ __forceinline__ u32 cc_step(u32 g, u32 gear) { return (g << 1) + gear; }

// g(p), from the bytes before p alone (x: the buffer's first byte)
__host__ __device__ inline u32 cc_hash_at(const u8* x, u64 p)
{
    u32 g = 0;
    for (u64 i = p < kCutsHashBytes ? 0 : p - kCutsHashBytes; i < p; ++i) g = cc_step(g, cc_gear(x[i]));
    return g;
}

// the positions that can be content cuts, and the two comparisons of the rule: gc = g(c) against g of a position before / behind c
__host__ __device__ __forceinline__ bool cc_eligible(u64 c, u64 n, u32 w) { return c > w && n > w && c < n - w; }
__host__ __device__ __forceinline__ bool cc_beats_before(u32 gc, u32 g) { return gc > g; }
__host__ __device__ __forceinline__ bool cc_beats_behind(u32 gc, u32 g) { return gc >= g; }

// the forced cuts a + k * mx (k >= 1) that lie in [lo, hi), a <= lo: how many, and *k0 = the first one's k
__host__ __device__ __forceinline__ u64 cc_forced_in(u64 a, u64 lo, u64 hi, u32 mx, u64* k0)
{
    const u64 first = lo <= a ? 1 : (lo - a + mx - 1) / mx;             // (lo - a < 2^63 in every use: no wrap)
    *k0 = first;
    if (hi <= a) return 0;
    const u64 last = (hi - 1 - a) / mx;
    return last >= first ? last - first + 1 : 0;
}

// no buffer of len bytes has more cuts than this: content cuts are more than w apart, and the forced ones are mx apart
__host__ __device__ __forceinline__ u64 cc_cut_bound(u64 len, u32 w, u32 mx) { return len / (w + 1) + len / mx; }

// hi * 2^32 + lo, saturating: the two halves of a sum of u64 values that were scanned apart so that no sum wraps
__host__ __device__ __forceinline__ u64 cc_sat_join(u64 hi, u64 lo)
{
    const u64 h = hi + (lo >> 32);
    return h >> 32 ? ~0ull : (h << 32) | (lo & 0xffffffffull);
}

// ---- the encoder's cut list: untrusted input -------------------------------------------------------------------------------------------------------
// where slot bytes are staged: a piece of p bytes takes snp_comp_stride(p) (capi_internal.h) -- no more than p + p / 6 + 69
__host__ __device__ constexpr u64 ec_stride(u64 p) { return (38 + p + p / 6 + 15) / 16 * 16 + 16; }
// a documented bound for stage_cap from the bytes and the pieces of a batch
__host__ __device__ __forceinline__ u64 ec_stage_bound(u64 bytes, u64 pieces) { return bytes + bytes / 6 + 69 * pieces; }

// buffer b's cuts are cuts[lo .. hi), lo = cut_first[b], hi = cut_first[b + 1]: the range is inside the list
__host__ __device__ __forceinline__ bool ec_range_ok(u64 lo, u64 hi, u64 ncuts) { return lo <= hi && hi <= ncuts; }
// one cut after `prev` (0 before the first): strictly ascending, inside (0, in_len), the piece before it no longer than a chunk may be
__host__ __device__ __forceinline__ bool ec_cut_ok(u64 prev, u64 cut, u64 in_len) { return cut > prev && cut < in_len && cut - prev <= SNP_BLOCK_SIZE; }
// the piece behind the last cut (last = 0 without one; every cut passed ec_cut_ok, so last < in_len or both are 0)
__host__ __device__ __forceinline__ bool ec_tail_ok(u64 last, u64 in_len) { return in_len - last <= SNP_BLOCK_SIZE; }
// the pieces of a buffer with a good list
__host__ __device__ __forceinline__ u64 ec_pieces(u64 lo, u64 hi, u64 in_len) { return in_len ? hi - lo + 1 : 0; }

// piece k of a buffer with a good list: [*start, *start + return)
__host__ __device__ __forceinline__ u32 ec_piece(const u64* __restrict__ cuts, u64 lo, u64 hi, u64 in_len, u64 k, u64* start)
{
    const u64 s = k ? cuts[lo + k - 1] : 0, e = lo + k < hi ? cuts[lo + k] : in_len;
    *start = s;
    return static_cast<u32>(e - s);
}

// the first piece of a buffer with a good list that starts at or behind `at`: pieces start at 0 and at every cut
__host__ __device__ inline u64 ec_first_piece_from(const u64* __restrict__ cuts, u64 lo, u64 hi, u64 at)
{
    if (at == 0) return 0;
    u64 a = lo, b = hi;                                                 // the first cut >= at
    while (a < b) {
        const u64 mid = a + (b - a) / 2;
        if (cuts[mid] < at) a = mid + 1;
        else b = mid;
    }
    return a - lo + 1;
}

}  // namespace

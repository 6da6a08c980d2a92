// frame_dedup_device.h -- the rules of the batch DEDUP (snp_frame_dedup_indexed_batch, frame_dedup.hip), stated once: the verdict of a stream
// over a chunk index that is UNTRUSTED input, the key of a row and its slot in the table, when two chunks are the same bytes, what a row of a
// new stream stands for in the recipe and where a recipe segment begins.  On top of frame_rechunk_device.h (the verdict of a stream before its
// rows are looked at) and frame_compose_device.h, whose check of a kept row (cc_add) is the check of every row here: a stream is one segment
// that covers all of it and has no edge, so nothing of that check is restated.  __host__ __device__ throughout, so that the same code runs on
// the CPU under sanitizers (tests/abi/frame_dedup_plan_check.hip) against brute force.  DESIGN.md 4.27.
//
// Rows are numbered over the whole index ("global row").  A row TAKES PART when its stream's verdict is SNP_OK and it decodes to at least one
// byte.  Its KEY is (decoded length, the CRC field of its chunk header); the LEADER of a key is the lowest row that has it; canon[r] = the
// leader when chunk r and the leader's chunk are the same 4 + size bytes, else r.  One round: rows that differ from their leader stay as they
// are, whatever they are equal to.
#pragma once
#include "frame_compose_device.h"
#include "bytes16_device.h"

namespace {

constexpr u64 kDdNone = ~0ull;              // SNP_DEDUP_NONE: canon of a row that takes no part
constexpr u64 kDdEmpty = ~0ull;             // the key of an empty slot (no row has it: a chunk decodes to fewer than 2^31 bytes)
constexpr u32 kDdNoRow = 0xffffffffu;       // the row of an empty slot
constexpr u64 kDdMaxRows = 0x7fffffffull;   // rows a call takes: a row number fits 31 bits, the table 2^32 slots

__host__ __device__ __forceinline__ u64 dd_key(u32 dec, u32 crc) { return (static_cast<u64>(dec) << 32) | crc; }
// the CRC field of the data chunk whose header lies at p (a data chunk holds at least the 8 bytes of header and CRC), byte by byte
__host__ __device__ __forceinline__ u32 dd_crc_field(const u8* __restrict__ p)
{
    return static_cast<u32>(p[4]) | (static_cast<u32>(p[5]) << 8) | (static_cast<u32>(p[6]) << 16) | (static_cast<u32>(p[7]) << 24);
}

// slots of the table for an index of nentries rows: a power of two, at most half full, at least 64
__host__ __device__ inline u64 dd_slots(u64 nentries)
{
    u64 t = 64;
    while (t < 2 * nentries) t <<= 1;
    return t;
}
// where the probe of a key begins (the finaliser of splitmix64: the CRC's low bits and the length are both spread); the probe is linear
__host__ __device__ __forceinline__ u64 dd_slot(u64 key, u64 mask)
{
    u64 h = key;
    h ^= h >> 30;
    h *= 0xbf58476d1ce4e5b9ull;
    h ^= h >> 27;
    h *= 0x94d049bb133111ebull;
    h ^= h >> 31;
    return h & mask;
}

// ---- the verdict ------------------------------------------------------------------------------------------------------------------------------------
// idx_first clamped to nentries
__host__ __device__ __forceinline__ u64 dd_first(const FrameIndex& x, u64 j) { return x.first[j] < x.nentries ? x.first[j] : x.nentries; }

// Stream b as the one segment whose rows cc_add checks: all its rows, no edge, no border.  before: the largest clamped idx_first of the streams
// in front of it (0 for stream 0).  A stream that begins below that would share rows with one in front: its idx_first runs backwards.
__host__ __device__ inline CcSeg dd_stream(const FrameIndex& x, const u64* __restrict__ in_len, u32 b, u64 before)
{
    CcSeg k{};
    k.status = fr_begin(x, b);
    if (k.status != SNP_OK) return k;
    u64 f0, rows;
    fr_rows(x, b, &f0, &rows);
    if (f0 < before) { k.status = SNP_ERR_BAD_ARG; return k; }
    k.src = b;
    k.lo = 0;
    k.hi = ~0ull;
    k.r0 = f0;
    k.r1 = k.f1 = f0 + rows;
    k.total = x.total[b];
    k.n = in_len[b];
    return k;
}

// ---- two chunks ---------------------------------------------------------------------------------------------------------------------------------------
// bytes [16 k, min(16 k + 16, n)) of a and of b are the same (the chunks lie at any alignment)
__host__ __device__ __forceinline__ bool dd_same_part(const u8* __restrict__ a, const u8* __restrict__ b, u64 n, u64 k)
{
    const u64 at = 16 * k;
    if (at >= n) return true;
    if (n - at >= 16) {
        return first_diff16(*reinterpret_cast<const snp_u128_unaligned*>(a + at), *reinterpret_cast<const snp_u128_unaligned*>(b + at), 0) == 16;
    }
    bool same = true;
    for (u64 i = at; i < n; ++i) same = same && a[i] == b[i];
    return same;
}
__host__ __device__ __forceinline__ u64 dd_parts(u64 n) { return (n + 15) / 16; }
// the whole chunks, by one thread (the kernel has a wavefront take the parts 64 at a time)
__host__ __device__ inline bool dd_same(const u8* __restrict__ a, u64 na, const u8* __restrict__ b, u64 nb)
{
    if (na != nb) return false;
    for (u64 k = 0; k < dd_parts(na); ++k)
        if (!dd_same_part(a, b, na, k)) return false;
    return true;
}

// ---- the recipe -----------------------------------------------------------------------------------------------------------------------------------------
// What a row of a new stream stands for: its canonical row's decoded bytes -- in a base stream from that row's idx_start, in the pack (source
// nbase) from the decoded bytes of the packed rows before it.
struct DdSrc {
    u32 src;
    u64 off;
};
__host__ __device__ __forceinline__ DdSrc dd_source(u32 canon_stream, u32 nbase, u64 canon_start, u64 canon_packed)
{
    return canon_stream < nbase ? DdSrc{canon_stream, canon_start} : DdSrc{nbase, canon_packed};
}
// Row r (not empty) of a stream begins a segment unless the row that takes part before it in the same stream has the same source and ends where
// this one starts.
__host__ __device__ __forceinline__ bool dd_begins(bool first, const DdSrc& prev, u64 prev_len, const DdSrc& cur)
{
    return first || prev.src != cur.src || prev.off + prev_len != cur.off;
}

}  // namespace

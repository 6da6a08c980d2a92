// frame_find_device.h -- the planning and the arithmetic of the batch find (snp_frame_find_indexed_batch, frame_find.hip): where a byte string
// occurs in windows of what seekable framed streams decode to.  __host__ __device__ throughout, so that the same code runs on the CPU under
// sanitizers (tests/abi/frame_find_plan_check.hip) over indexes filled with anything at all.  The clip, the searches and the row check are the
// indexed read's (frame_index_device.h); nothing of them is restated.  DESIGN.md 4.24.
//
// A request owns the rows the read would select for its window, [r0, r1).  Decoded one after the other they are one RUN of
// end(r1 - 1) - start[r0] bytes whose byte 0 is byte start[r0] of the stream: rows and bytes follow from the index's starts alone.
// The START POSITIONS of a window [lo, hi) and a needle of m bytes are [lo, hi - m]; they are cut into TILES of kFindTile.
#pragma once
#include "frame_index_device.h"

namespace {

constexpr u32 kFindTile = 16384;            // start positions per tile (one workgroup: 4 steps of 256 lanes x 16)
constexpr u32 kFindMaxNeedle = 256;
constexpr u64 kFindRowClamp = 1ull << 31;   // a request's rows count as no more than this (max_rows is below it: such a request never fits)
constexpr u64 kFindCapMax = (1ull << 40) - 1;   // scratch_cap counts as no more than this
constexpr u32 kFindSlack = 32;              // bytes after the scratch arena that a 16-byte read from its last bytes may touch

// one request: the read's plan, and what its rows need
struct FdPlan {
    IxPlan k;
    u64 rows;           // r1 - r0
    u64 bytes;          // of the run
    u64 s0;             // the stream offset of the run's first byte
};
__host__ __device__ inline FdPlan fd_plan(const FrameIndex& x, u32 nstreams, u32 b, u64 req_off, u64 req_len, u32 m)
{
    FdPlan p{};
    p.k.status = SNP_ERR_BAD_ARG;
    if (m == 0 || m > kFindMaxNeedle) return p;
    p.k = ix_plan(x, nstreams, b, req_off, req_len, ~0ull);
    if (p.k.status != SNP_OK || p.k.r0 >= p.k.r1) return p;
    p.rows = p.k.r1 - p.k.r0;
    p.s0 = x.start[p.k.r0];
    p.bytes = ix_row_end(x, p.k.f1, p.k.total, p.k.r1 - 1) - p.s0;      // (the plan has checked s0 <= lo <= hi <= that end)
    return p;
}

// a + b, or 2^64 - 1
__host__ __device__ __forceinline__ u64 fd_sat_add(u64 a, u64 b) { return a + b < a ? ~0ull : a + b; }
// The sum of up to 2^30 u64 values, kept as the sums of their high and of their low 32-bit halves (neither can wrap): the sum, or 2^64 - 1.
__host__ __device__ __forceinline__ u64 fd_sat_join(u64 hi_sum, u64 lo_sum)
{
    const u64 h = hi_sum + (lo_sum >> 32);
    return h >> 32 ? ~0ull : (h << 32) | (lo_sum & 0xffffffffull);
}

// the start positions of a window of n bytes, and the tiles they make
__host__ __device__ __forceinline__ u64 fd_starts(u64 n, u32 m) { return n >= m ? n - m + 1 : 0; }
__host__ __device__ __forceinline__ u64 fd_tiles(u64 starts) { return starts / kFindTile + (starts % kFindTile ? 1 : 0); }
// tile t of a window that begins at lo: its start positions [*first, *end) as stream offsets
__host__ __device__ __forceinline__ void fd_tile(u64 lo, u64 starts, u64 t, u64* first, u64* end)
{
    const u64 a = t * kFindTile, b = starts - a < kFindTile ? starts : a + kFindTile;
    *first = lo + a;
    *end = lo + b;
}

// Row i of a request as a row of its run: the read's check (an edge row as an edge, any other as an interior row) gives *good; the row may be
// decoded at byte *at of the run only if it also lies inside the run.  (When every row of a request is good they tile the run, so a good row
// outside it means another row is not good: the request then decodes nothing.)
__host__ __device__ inline bool fd_row(const FrameIndex& x, const u8* __restrict__ p, u64 n, const FdPlan& q, u64 i, Hop* h, bool* good, u64* at)
{
    const bool edge = (q.k.head && i == q.k.r0) || (q.k.last && i == q.k.r1 - 1);
    *good = i < q.k.f1 && ix_row_check(x, p, n, q.k, i, !edge, h);
    if (!*good) return false;
    const u64 s = x.start[i], e = ix_row_end(x, q.k.f1, q.k.total, i);
    if (s < q.s0 || e - q.s0 > q.bytes) return false;
    *at = s - q.s0;
    return true;
}

}  // namespace

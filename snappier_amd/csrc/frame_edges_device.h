// frame_edges_device.h -- what a WINDOW of a framed stream takes beyond its interior chunks, whoever found the chunks: the two edge slots per
// window and their place in a workspace (FrEdges, carve_edges), the scans that place the edges in the scratch arena and in the compact edge
// table, an edge slot from a hop and its row in that table, the trim of a decoded edge into the window, the key of a failing interior row and
// the precedence of the verdict.  Shared by the range decode (frame_range.hip: one window per stream, the chunks found by the span walk) and the
// indexed read (frame_index.hip: any number of windows, the chunks found by two searches in a chunk index); a window's edge slots are 2 w (head)
// and 2 w + 1 (tail), w the window's number in the call.  DESIGN.md 4.13, 4.14.
#pragma once
#include "frame_hop_device.h"

namespace {

constexpr u64 kNoFail = ~0ull;

// two edge slots per window, where the selection records what it finds; dec == 0: an empty slot
struct FrEdges {
    u8* type;
    u64 *body_off, *start, *place, *rank;   // start: s, the chunk's first decoded byte in its stream; place, rank: the scans of dec and of dec != 0 (n + 1 each)
    u32 *body_len, *crc, *dec;
};
// the edge slots over ne = 2 x windows slots of a d_work workspace
inline FrEdges carve_edges(WorkCarver& c, u64 ne)
{
    FrEdges e;
    e.body_off = c.take<u64>(ne);
    e.start = c.take<u64>(ne);
    e.place = c.take<u64>(ne + 1);
    e.rank = c.take<u64>(ne + 1);
    e.body_len = c.take<u32>(ne);
    e.crc = c.take<u32>(ne);
    e.dec = c.take<u32>(ne);
    e.type = c.take<u8>(ne);
    return e;
}

struct ScanEdgeBytes {
    const u32* __restrict__ dec;
    __device__ __forceinline__ u64 operator()(u64 i) const { return dec[i]; }
};
struct ScanEdgeCount {
    const u32* __restrict__ dec;
    __device__ __forceinline__ u64 operator()(u64 i) const { return dec[i] != 0; }
};

// Edge slot `slot` as the data chunk a hop found: its header at byte `header` of the input, its first decoded byte at `start` of its stream.
__device__ __forceinline__ void edge_slot_set(const FrEdges& e, u64 slot, const Hop& h, u64 header, u64 start)
{
    e.type[slot] = static_cast<u8>(h.type);
    e.body_off[slot] = header + SNP_CHUNK_HEADER_LEN;
    e.body_len[slot] = h.body_len;
    e.crc[slot] = h.crc;
    e.dec[slot] = h.dec;
    e.start[slot] = start;
}

// The row of an admitted window's edge in the COMPACT edge table (row = the slot's rank among the slots in use), decoded whole at its place in
// the scratch arena.  (A rank belongs to one edge: every row is written by one thread.)
__device__ __forceinline__ void edge_row_place(const ChunkRows& c, const FrEdges& e, u64 slot)
{
    const u64 row = e.rank[slot];
    c.tag[row] = static_cast<u32>(slot);
    c.type[row] = e.type[slot];
    c.body_off[row] = e.body_off[slot];
    c.body_len[row] = e.body_len[slot];
    c.crc[row] = e.crc[slot];
    c.out_off[row] = e.place[slot];
    c.out_cap[row] = e.dec[slot];
}

// One workgroup per edge row: an OK edge's bytes inside the window [lo, hi), scratch -> dst (dst: where byte lo of the window goes).  (A row
// in use belongs to an admitted window that fits its capacity: max(s, lo) - lo + the bytes copied = min(s + d, hi) - lo <= hi - lo <= out_cap.)
// All threads must call it.
__device__ __forceinline__ void edge_trim(const ChunkRows& c, const FrEdges& e, u64 row, u32 slot, u64 lo, u64 hi, const u8* __restrict__ scratch,
                                          u8* __restrict__ dst, u32 tid)
{
    const u32 d = c.out_cap[row];
    if (c.status[row] != SNP_OK || c.out_len[row] != d) return;
    const u64 s = e.start[slot];
    const u64 from = s > lo ? s : lo, to = s + d < hi ? s + d : hi;
    if (to <= from) return;
    block_copy(dst + (from - lo), scratch + c.out_off[row] + (from - s), static_cast<u32>(to - from), tid);
}

// the word a failing interior row puts (atomicMin) into its window's failure word: the first in stream order wins
__device__ __forceinline__ u64 fail_key(u64 place, i32 status) { return ((1 + place) << 8) | static_cast<u64>(status & 0xff); }

// A window's verdict once it is admitted: the first failing selected chunk in stream order (head edge, interior rows, tail edge), else the error
// that ended the stream's walk, else the capacity, else OK.
__device__ __forceinline__ i32 window_verdict(i32 s_head, u64 fail, i32 s_tail, i32 walk_tail, bool small)
{
    if (s_head != SNP_OK) return s_head;
    if (fail != kNoFail) return static_cast<i32>(fail & 0xff);
    if (s_tail != SNP_OK) return s_tail;
    if (walk_tail != SNP_OK) return walk_tail;
    return small ? SNP_ERR_OUTPUT_TOO_SMALL : SNP_OK;
}
// ... and the status of an edge slot's row (an empty slot has none)
__device__ __forceinline__ i32 edge_status(const ChunkRows& c, const FrEdges& e, u64 slot) { return e.dec[slot] ? c.status[e.rank[slot]] : SNP_OK; }

}  // namespace

// frame_index_device.h -- the planning of ONE request of the indexed read (snp_frame_read_indexed_batch, frame_index.hip) over a chunk index that
// is UNTRUSTED input: the clip of the window, the two binary searches that replace the header walk, the classification of the rows the request
// owns (head edge, interior, tail edge) and the check of one row against the header it points at.  __host__ __device__ throughout, so that the
// same code runs on the CPU under sanitizers (tests/abi/frame_index_plan_check.hip) over indexes filled with anything at all.
//
// The index of stream b (snp_frame_index_batch): rows [first[b], first[b + 1]) of start / pos, one per data chunk in stream order -- the decoded
// bytes of the stream before the chunk and the position of its 4-byte header relative to the stream's first byte -- with total[b] the stream's
// decoded bytes and tail[b] the status that ended its walk.  Row i ends where row i + 1 starts (the last one at total).
// Every index read is bounded by nentries (first values are clamped to it), every header read by the stream's length.  DESIGN.md 4.14.
#pragma once
#include "frame_hop_device.h"

namespace {

struct FrameIndex {
    const u64 *first, *start, *pos, *total;
    const i32* tail;
    u64 nentries;
};

struct IxPlan {
    i32 status;         // SNP_OK: planned; SNP_ERR_BAD_ARG, SNP_ERR_OUTPUT_TOO_SMALL: the request's answer, it owns nothing
    i32 tail;           // the stream's idx_tail
    bool small;         // hi - lo > out_cap: nothing is selected
    bool head, last;    // row r0 is the head edge; row r1 - 1 is the tail edge
    u64 lo, hi;         // the clipped window
    u64 r0, r1;         // the rows the request owns (absolute)
    u64 f1;             // where the stream's rows end (clamped)
    u64 total;
    __host__ __device__ u64 interior() const { return r1 - r0 - (head ? 1 : 0) - (last ? 1 : 0); }
};

// where row i of a stream whose rows end at f1 ends
__host__ __device__ __forceinline__ u64 ix_row_end(const FrameIndex& x, u64 f1, u64 total, u64 i) { return i + 1 < f1 ? x.start[i + 1] : total; }

// first i in [a, b) for which pred(i) holds (pred false, then true: what a sound index gives; any answer in [a, b] otherwise)
template <class P>
__host__ __device__ __forceinline__ u64 ix_first_where(u64 a, u64 b, P pred)
{
    while (a < b) {
        const u64 mid = a + (b - a) / 2;
        if (pred(mid)) b = mid;
        else a = mid + 1;
    }
    return a;
}

// The request (stream b, window [req_off, req_off + req_len), capacity cap) against the index alone: no byte of a stream is read.
__host__ __device__ inline IxPlan ix_plan(const FrameIndex& x, u32 nstreams, u32 b, u64 req_off, u64 req_len, u64 cap)
{
    IxPlan k{};
    k.status = SNP_ERR_BAD_ARG;
    if (b >= nstreams) return k;
    k.tail = x.tail[b];
    if (k.tail == SNP_ERR_OUTPUT_TOO_SMALL) { k.status = SNP_ERR_OUTPUT_TOO_SMALL; return k; }   // the stream was not indexed
    if (k.tail < SNP_OK || k.tail > SNP_ERR_TRUNCATED_STREAM) return k;                          // (no status of the walk)
    const u64 f0 = x.first[b] < x.nentries ? x.first[b] : x.nentries, f1 = x.first[b + 1] < x.nentries ? x.first[b + 1] : x.nentries;
    if (f1 < f0) return k;
    const u64 total = x.total[b];
    const u64 end = req_off + req_len < req_off ? ~0ull : req_off + req_len;
    const u64 lo = req_off < total ? req_off : total, hi = end < total ? end : total;
    k.lo = lo;
    k.hi = hi;
    k.f1 = f1;
    k.total = total;
    k.r0 = k.r1 = f0;
    k.small = hi - lo > cap;
    if (k.small) { k.status = SNP_OK; return k; }
    const u64 i0 = ix_first_where(f0, f1, [&](u64 i) { return ix_row_end(x, f1, total, i) > lo; });
    const u64 i1 = ix_first_where(f0, f1, [&](u64 i) { return x.start[i] >= hi; });
    k.r0 = i0;
    k.r1 = i1 > i0 ? i1 : i0;
    if (k.r0 == k.r1) {
        if (hi > lo) return k;                                          // bytes to deliver and no row that holds them
        k.status = SNP_OK;
        return k;
    }
    // the owned rows must hold the window: row by row they are then checked to be data chunks of exactly end - start bytes, so they tile it
    const u64 s0 = x.start[k.r0], e1 = ix_row_end(x, f1, total, k.r1 - 1);
    if (s0 > lo || e1 < hi) return k;
    k.head = s0 < lo;
    k.last = e1 > hi && !(k.head && k.r1 - 1 == k.r0);
    k.status = SNP_OK;
    return k;
}

// The rule of a row [s, e) against the hop of the header it points at: a data chunk that decodes to exactly e - s bytes.
__host__ __device__ __forceinline__ bool ix_row_holds(u64 s, u64 e, const Hop& h) { return e >= s && h.kind == HOP_DATA && e - s == h.dec; }

// The check of row i of the stream (p, n): the header at pos[i] is re-read inside the stream's bytes and must be a data chunk that decodes to
// exactly end - start bytes; an interior row must also lie inside [lo, hi).  *h: the hop (body_len, crc and type come from the header).
__host__ __device__ inline bool ix_row_check(const FrameIndex& x, const u8* __restrict__ p, u64 n, const IxPlan& k, u64 i, bool interior, Hop* h)
{
    const u64 s = x.start[i], e = ix_row_end(x, k.f1, k.total, i), pos = x.pos[i];
    if (e < s || pos >= n) return false;
    *h = frame_hop(p, n, pos);
    if (!ix_row_holds(s, e, *h)) return false;
    return !interior || (s >= k.lo && e <= k.hi);
}

}  // namespace

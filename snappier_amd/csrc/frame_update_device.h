// frame_update_device.h -- the planning of the indexed WRITE (snp_frame_write_indexed_batch, frame_update.hip) over a chunk index that is UNTRUSTED
// input, on top of the planning of the indexed read (frame_index_device.h, reused as it is): where a stream's requests lie in the request list,
// the plan of ONE request (its order against its predecessor, its stream's verdict, its range, the rows it dirties, the check of its edge rows),
// which of those rows its predecessor dirtied already, and the check of one dirty row against the header it points at and against the dirty
// row before it.  __host__ __device__ throughout, so that the same code runs on the CPU under sanitizers (tests/abi/frame_update_plan_check.hip)
// over indexes and request lists filled with anything at all.  DESIGN.md 4.16.
//
// Requests are sorted by (req_stream, req_off) and byte-disjoint; a chunk is DIRTY when a request writes a byte of what it decodes to.  The dirty
// rows of a stream are numbered in request order; row i of request r is an EDGE when r covers it in part (it is decoded first), else it is
// wholly replaced.  Two requests meet in at most one row (the tail edge of the first, the head edge of the second): it belongs to the first.
#pragma once
#include "frame_index_device.h"

namespace {

constexpr u32 kFuMaxDec = SNP_BLOCK_SIZE;       // what one chunk may be re-encoded from

struct FuRequests {
    const u32* stream;
    const u64 *off, *len;
    u32 n;
};

// first r in [0, n) with stream[r] >= b (the list sorted: where stream b's requests start; anything else: some deterministic answer, monotone in b,
// so that [fu_lower(b), fu_lower(b + 1)) over all b are disjoint whatever the list holds)
__host__ __device__ __forceinline__ u64 fu_lower(const FuRequests& q, u64 b)
{
    return ix_first_where(0, q.n, [&](u64 i) { return q.stream[i] >= b; });
}

struct FuPlan {
    i32 status;         // SNP_OK: planned; else the request's answer, it dirties nothing
    bool head, last;    // row r0 is covered in part from its front / row r1 - 1 in part at its end (and is not the head)
    u64 r0, r1;         // the rows the request writes into (absolute); r0 == r1: none
};

// the stream-side half of a request's IxPlan again, for the check of one row
__host__ __device__ __forceinline__ IxPlan fu_window(const FrameIndex& x, u32 b, u64 off, u64 len)
{
    IxPlan k{};
    k.lo = off;
    k.hi = off + len;
    k.f1 = x.first[b + 1] < x.nentries ? x.first[b + 1] : x.nentries;
    k.total = x.total[b];
    return k;
}

// Request r against the request list, the index and the headers of its edge rows.  (p, n) = the stream's bytes is asked for only once the stream
// number is known to be one: bytes(b) -> p, length(b) -> n.
template <class Bytes, class Length>
__host__ __device__ inline FuPlan fu_plan(const FrameIndex& x, u32 nstreams, const FuRequests& q, u32 r, Bytes bytes, Length length)
{
    FuPlan k{};
    k.status = SNP_ERR_BAD_ARG;
    const u32 b = q.stream[r];
    if (b >= nstreams) return k;
    const u64 off = q.off[r], len = q.len[r];
    if (r > 0) {                                                        // sorted by (stream, offset), byte-disjoint: against the predecessor
        const u32 pb = q.stream[r - 1];
        if (pb > b) return k;
        if (pb == b) {
            const u64 po = q.off[r - 1], pe = po + q.len[r - 1] < po ? ~0ull : po + q.len[r - 1];
            if (po > off || pe > off) return k;
        }
    }
    // ... and against the list: the request lies where the search for its stream looks, between requests of its stream
    const u64 lb = fu_lower(q, b), ub = fu_lower(q, static_cast<u64>(b) + 1);
    if (r < lb || r >= ub) return k;
    if (r > lb && q.stream[r - 1] != b) return k;
    if (r + 1 < ub && q.stream[r + 1] != b) return k;
    const IxPlan p = ix_plan(x, nstreams, b, off, len, len);
    if (p.status != SNP_OK) { k.status = p.status; return k; }
    if (p.tail != SNP_OK) { k.status = p.tail; return k; }             // the stream's walk ended in an error: the stream is broken
    if (off + len < off || off + len > p.total) return k;               // this call never changes a stream's length
    if (len == 0) { k.status = SNP_OK; return k; }
    const u8* const s = bytes(b);
    const u64 n = length(b);
    Hop hh{}, ht{};
    if (p.head && !(ix_row_check(x, s, n, p, p.r0, false, &hh) && hh.dec <= kFuMaxDec)) return k;
    if (p.last && !(ix_row_check(x, s, n, p, p.r1 - 1, false, &ht) && ht.dec <= kFuMaxDec)) return k;
    k.status = SNP_OK;
    k.head = p.head;
    k.last = p.last;
    k.r0 = p.r0;
    k.r1 = p.r1;
    return k;
}

// The rows of a planned request (r0 < r1) that are its own: all but a first row that the previous request of the stream with rows (rows
// [.., pred_r1)) dirtied already.  status != SNP_OK: the two requests' rows overlap by more than that row (no sound index gives it).
struct FuOwn {
    i32 status;
    u64 own0, cnt;      // rows [own0, own0 + cnt)
};
__host__ __device__ __forceinline__ FuOwn fu_own(u64 r0, u64 r1, bool has_pred, u64 pred_r1)
{
    FuOwn o{SNP_OK, r0, r1 - r0};
    if (!has_pred || pred_r1 <= r0) return o;
    if (pred_r1 > r0 + 1) { o.status = SNP_ERR_BAD_ARG; o.cnt = 0; return o; }
    o.own0 = r0 + 1;
    o.cnt = r1 - r0 - 1;
    return o;
}

// The check of dirty row i of a planned request (stream b = (s, n), window k = fu_window): ix_row_check -- an edge as an edge, any other row inside
// the window -- no more than 65536 decoded bytes, and its header after the END of the chunk of the stream's previous dirty row `prev` (has_prev):
// two rows at one header, or rows out of order, would corrupt the copy.  *h: the hop.
__host__ __device__ inline bool fu_row_check(const FrameIndex& x, const u8* __restrict__ s, u64 n, const IxPlan& k, const FuPlan& pl, u64 i, bool has_prev,
                                             u64 prev, Hop* h)
{
    const bool edge = (i == pl.r0 && pl.head) || (i == pl.r1 - 1 && pl.last);
    if (i >= k.f1 || !ix_row_check(x, s, n, k, i, !edge, h) || h->dec > kFuMaxDec) return false;
    if (!has_prev) return true;
    const u64 pp = x.pos[prev];                                         // (prev is a row of an earlier plan: below nentries)
    if (pp >= n) return false;
    const Hop hp = frame_hop(s, n, pp);
    return hp.kind == HOP_DATA && hp.next <= x.pos[i];
}

}  // namespace

// frame_compose_device.h -- the planning of the indexed COMPOSE (snp_frame_compose_indexed_batch, frame_compose.hip): new framed streams made of
// windows ("segments") of old ones, over chunk indexes and a segment list that are both UNTRUSTED input.  On top of frame_index_device.h (the
// index, the window's rows by two searches -- ix_plan, the read call's rule --, the rule of a row against its header), frame_chunked_device.h
// (pieces of chunk_bytes) and frame_rechunk_device.h (the verdict of a source before its rows are looked at, the counting clamps).  Here: the
// plan of ONE segment on its own -- its rows, its edges, the check of one row and what it adds (CcAcc: the kernel has a workgroup walk the rows
// and joins what its threads found, the host walks them in a loop), the counts those sums give --, the segments of an output, the segment that
// owns the v-th edge, piece or new row of an output, and what a new row is: a piece of an edge or an old row, by subtraction.
// __host__ __device__ throughout, so that the same code runs on the CPU under sanitizers (tests/abi/frame_compose_plan_check.hip) over indexes
// and segment lists filled with anything at all and over positions and lengths past 4 GiB.  DESIGN.md 4.21.
//
// Segment g = the decoded bytes [lo, hi) of source s.  Its rows are [r0, r1): r0 the first row that ends above lo, r1 the first row at or behind
// r0 that starts at or above hi.  Row r0 is the HEAD EDGE when it starts below lo, row r1 - 1 the TAIL EDGE when it ends above hi; when both are
// one row it is the head edge and its region is [lo, hi).  An edge is decoded and the part of it inside the segment is cut into pieces of
// chunk_bytes; every other row is KEPT: its chunk is copied.  In the new stream the segment is its head pieces, its kept chunks, its tail pieces.
#pragma once
#include "frame_rechunk_device.h"

namespace {

// ---- one segment ------------------------------------------------------------------------------------------------------------------------------------
struct CcSeg {
    i32 status;         // SNP_OK: planned (also a segment of no bytes, which owns nothing); else the answer of every output that holds it
    bool head, tail;    // row r0 is the head edge; row r1 - 1 is the tail edge (and is not the head edge)
    u32 src;            // the source stream
    u64 lo, hi;
    u64 r0, r1, f1, total;
    u64 n;              // the source's bytes (what the headers are read inside)
    // from the rows (cc_finish)
    u32 hdec, tdec;     // what the edges decode to (0: no such edge)
    u32 hlen, tlen;     // the edges' bytes inside the segment
    u64 hskip;          // lo - the head edge's start: where the head region begins in what the edge decodes to
    u64 hp, tp;         // pieces of the head and of the tail region
    u64 kept, kbytes;   // kept rows, and the bytes of their chunks (4 + size each)
};

// The segment against the index alone: no byte of a stream is read.  A segment of no bytes asks only for src < nstreams.
__host__ __device__ inline CcSeg cc_begin(const FrameIndex& x, const u64* __restrict__ in_len, u32 nstreams, u32 src, u64 off, u64 len)
{
    CcSeg k{};
    k.status = SNP_ERR_BAD_ARG;
    k.src = src;
    if (src >= nstreams) return k;
    k.status = SNP_OK;
    if (len == 0) return k;
    k.status = fr_begin(x, src);                                        // the status that ended the source's walk; f1 < f0
    if (k.status != SNP_OK) return k;
    k.status = SNP_ERR_BAD_ARG;
    if (off + len < off || off + len > x.total[src]) return k;
    const IxPlan p = ix_plan(x, nstreams, src, off, len, ~0ull);        // (inside total: the window is not clipped)
    if (p.status != SNP_OK) return k;                                   // bytes and no row that holds them
    k.status = SNP_OK;
    k.head = p.head;
    k.tail = p.last;
    k.lo = p.lo;
    k.hi = p.hi;
    k.r0 = p.r0;
    k.r1 = p.r1;
    k.f1 = p.f1;
    k.total = p.total;
    k.n = in_len[src];
    return k;
}

// What the rows of a segment add up to.  Sums and ORs: the order in which rows are joined does not matter.
struct CcAcc {
    u64 kept, kbytes;
    u64 hdec, tdec;     // (one row each at most)
    u32 bad;
};
__host__ __device__ __forceinline__ bool cc_is_head(const CcSeg& k, u64 i) { return k.head && i == k.r0; }
__host__ __device__ __forceinline__ bool cc_is_tail(const CcSeg& k, u64 i) { return k.tail && i + 1 == k.r1; }

// Row i of [r0, r1): its header is read again inside the source's bytes and holds (ix_row_holds), the next row's chunk lies at or behind the end
// of this one's, and an edge decodes to no more than 65536 bytes.  hop_at(pos) -> the Hop of the header at pos < n.
template <class HopAt>
__host__ __device__ inline void cc_add(CcAcc* a, const FrameIndex& x, const CcSeg& k, u64 i, HopAt hop_at)
{
    const u64 s = x.start[i], e = ix_row_end(x, k.f1, k.total, i), pos = x.pos[i];
    if (e < s || pos >= k.n) { a->bad = 1; return; }
    const Hop h = hop_at(pos);
    if (!ix_row_holds(s, e, h) || (i + 1 < k.r1 && x.pos[i + 1] < h.next)) { a->bad = 1; return; }
    const bool head = cc_is_head(k, i), tail = cc_is_tail(k, i);
    if (head || tail) {
        // (an edge holds bytes on both sides of a border of the segment: ix_plan saw start < lo < end or start < hi < end)
        if (h.dec > kFrMaxDec || (head ? s >= k.lo || e <= k.lo : s >= k.hi || e <= k.hi)) { a->bad = 1; return; }
        if (head) a->hdec += h.dec;
        else a->tdec += h.dec;
    } else {
        if (s < k.lo || e > k.hi) { a->bad = 1; return; }              // a kept row lies inside the segment
        a->kept += 1;
        a->kbytes += h.next - pos;
    }
}

// The plan of a segment from what its rows add up to.  A segment that fails keeps its status and nothing else.
__host__ __device__ inline void cc_finish(CcSeg* k, const FrameIndex& x, u32 cb, const CcAcc& acc)
{
    if (k->status == SNP_OK && k->r0 != k->r1) {
        if (acc.bad || (k->head && acc.hdec == 0) || (k->tail && acc.tdec == 0)) k->status = SNP_ERR_BAD_ARG;
        k->kept = acc.kept;
        k->kbytes = acc.kbytes;
        if (k->status == SNP_OK && k->head) {
            const u64 s = x.start[k->r0], e = s + acc.hdec;
            k->hdec = static_cast<u32>(acc.hdec);
            k->hskip = k->lo - s;
            k->hlen = static_cast<u32>((e < k->hi ? e : k->hi) - k->lo);
            k->hp = fc_chunks(k->hlen, cb);
        }
        if (k->status == SNP_OK && k->tail) {
            k->tdec = static_cast<u32>(acc.tdec);
            k->tlen = static_cast<u32>(k->hi - x.start[k->r1 - 1]);
            k->tp = fc_chunks(k->tlen, cb);
        }
    }
    if (k->status != SNP_OK) *k = CcSeg{k->status};
}

// the whole plan of a segment by one thread: the host's walk (the kernel joins the same calls over a workgroup)
template <class HopAt>
__host__ __device__ inline CcSeg cc_plan(const FrameIndex& x, const u64* __restrict__ in_len, u32 nstreams, u32 src, u64 off, u64 len, u32 cb, HopAt hop_at)
{
    CcSeg k = cc_begin(x, in_len, nstreams, src, off, len);
    CcAcc acc{};
    if (k.status == SNP_OK)
        for (u64 i = k.r0; i < k.r1; ++i) cc_add(&acc, x, k, i, [&](u64 pos) { return hop_at(k.src, pos); });
    cc_finish(&k, x, cb, acc);
    return k;
}

// what a segment asks: decode rows, compressor slots, staging bytes, rows of the new index (a segment of 2^32 rows or more counts as 2^32: no
// bound admits it, and no sum over fewer than 2^31 segments wraps), decoded bytes, and the size bound of its part of the new stream
__host__ __device__ __forceinline__ u64 cc_seg_edges(const CcSeg& k) { return (k.head ? 1u : 0u) + (k.tail ? 1u : 0u); }
__host__ __device__ __forceinline__ u64 cc_seg_pieces(const CcSeg& k) { return k.hp + k.tp; }
__host__ __device__ __forceinline__ u64 cc_seg_stage(const CcSeg& k) { return static_cast<u64>(k.hdec) + k.tdec; }
__host__ __device__ __forceinline__ u64 cc_seg_rows(const CcSeg& k)
{
    const u64 rows = k.hp + k.tp + k.kept;
    return rows < kFrMaxCount ? rows : kFrMaxCount;
}
__host__ __device__ __forceinline__ u64 cc_seg_bytes(const CcSeg& k) { return k.hi - k.lo; }
__host__ __device__ __forceinline__ u64 cc_seg_bound(const CcSeg& k) { return k.kbytes + SNP_CHUNK_HEADER_LEN * (k.hp + k.tp) + k.hlen + k.tlen; }

// ---- one output ---------------------------------------------------------------------------------------------------------------------------------------
// the segments of output j: [s0, s1), inside nsegs whatever seg_first holds; false: the list runs backwards
__host__ __device__ __forceinline__ bool cc_segs(const u64* __restrict__ seg_first, u32 nsegs, u32 j, u64* s0, u64* s1)
{
    *s0 = seg_first[j] < nsegs ? seg_first[j] : nsegs;
    *s1 = seg_first[j + 1] < nsegs ? seg_first[j + 1] : nsegs;
    return *s1 >= *s0;
}
// what an output asks of a bound, from the sum over its segments
__host__ __device__ __forceinline__ u64 cc_count(u64 sum) { return sum < kFrMaxCount ? sum : kFrMaxCount; }
__host__ __device__ __forceinline__ u64 cc_count_stage(u64 sum) { return sum < kFrMaxStage ? sum : kFrMaxStage; }

// scan[0 .. nsegs] the exclusive scan of a count over ALL segments of the call: the segment of [s0, s1) that owns the v-th unit of the output
// (v < scan[s1] - scan[s0]), and the unit's number within it.  Segments that count nothing are passed over.
__host__ __device__ inline u64 cc_seg_of(const u64* __restrict__ scan, u64 s0, u64 s1, u64 v, u64* within)
{
    const u64 g = ix_first_where(s0, s1, [&](u64 i) { return scan[i + 1] - scan[s0] > v; });
    *within = v - (scan[g < s1 ? g : s0] - scan[s0]);
    return g;
}

// Row q of a segment's part of the new index (q < hp + kept + tp): a piece of an edge -- its number among the segment's pieces (slot), where it
// begins in what the edge decodes to and its length -- or an old row.  at: the row's first decoded byte, relative to the segment's.
struct CcRow {
    bool kept, tail;
    u64 row;            // kept: the old row
    u64 slot;           // piece: its number among the segment's pieces (head pieces first)
    u64 from;           // piece: its first byte in what its edge decodes to
    u32 len;            // piece: its bytes
    u64 at;
};
__host__ __device__ inline CcRow cc_piece(u64 hp, u64 hskip, u32 hlen, u32 tlen, u32 cb, u64 m)
{
    CcRow r{};
    r.slot = m;
    r.tail = m >= hp;
    const u64 k = r.tail ? m - hp : m, region = r.tail ? tlen : hlen;
    r.from = (r.tail ? 0 : hskip) + k * cb;
    r.len = region - k * cb < cb ? static_cast<u32>(region - k * cb) : cb;
    return r;
}
__host__ __device__ inline CcRow cc_row(const FrameIndex& x, u64 r0, bool head, u64 lo, u64 hp, u64 kept, u64 hskip, u32 hlen, u32 tlen, u32 cb, u64 q)
{
    if (q < hp) {
        CcRow r = cc_piece(hp, hskip, hlen, tlen, cb, q);
        r.at = q * cb;
        return r;
    }
    if (q < hp + kept) {
        CcRow r{};
        r.kept = true;
        r.row = r0 + (head ? 1 : 0) + (q - hp);
        r.at = x.start[r.row] - lo;
        return r;
    }
    CcRow r = cc_piece(hp, hskip, hlen, tlen, cb, q - kept);
    r.at = x.start[r0 + (head ? 1 : 0) + kept] - lo + (q - hp - kept) * cb;
    return r;
}

}  // namespace

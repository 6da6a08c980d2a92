// frame_recut_device.h -- the planning of the indexed RECUT (snp_frame_recut_indexed_batch, frame_recut.hip): a seekable stream brought to the
// pieces of a caller's cut list.  Both inputs are UNTRUSTED: the chunk index (frame_rows_device.h: the verdict of a stream, the check of one
// row, what the rows add up to -- shared with the rechunk) and the cut list (frame_cuts_device.h: the encoder's verdict, with the stream's decoded
// bytes in place of a buffer's length).  Here: the rule that makes a row CLEAN against a list, the sums of a stream's list and rows (RxAcc: the
// kernel joins them over a workgroup, the host in a loop), the plan they give, what a stream asks of each bound, piece j of the new stream (kept,
// and which old row it is, or rebuilt), and the two maps between the rebuilt pieces and the dirty rows.  __host__ __device__ throughout, so that
// the same text runs on the CPU under sanitizers (tests/abi/frame_recut_plan_check.hip) over indexes and lists filled with anything at all and
// over positions and cuts past 4 GiB.  DESIGN.md 4.28.
//
// Stream b decodes to total bytes; its cuts are cuts[lo .. hi), lo = cut_first[b], hi = cut_first[b + 1]; its pieces are the intervals between
// neighbours of {0} + cuts + {total}.  A row [s, e) of positive length is CLEAN when s is 0 or a cut and the next cut above s (total without one)
// is e: its chunk IS a piece and is copied.  Every other row is DIRTY.  The clean rows are whole pieces of a partition, so the dirty rows cover
// exactly the other pieces, in order: the decoded dirty rows back to back ARE the rebuilt pieces back to back, whatever the partition.
#pragma once
#include "frame_rows_device.h"
#include "frame_cuts_device.h"

namespace {

constexpr u32 kRxRewriteAll = 1u;                           // SNP_RECUT_REWRITE_ALL

// One binary search in the stream's list: the first cut above s.  (Any list at all: every read is inside [lo, hi).)
__host__ __device__ inline bool rx_clean(const u64* __restrict__ cuts, u64 lo, u64 hi, u64 total, u64 s, u64 len)
{
    if (len == 0) return false;
    const u64 j = ix_first_where(lo, hi, [&](u64 k) { return cuts[k] > s; });
    if (s != 0 && (j == lo || cuts[j - 1] != s)) return false;
    return (j < hi ? cuts[j] : total) == s + len;
}

// row i of a stream against its list (fr_row_as, frame_rows_device.h: the check itself)
template <class HopAt>
__host__ __device__ inline FrRow rx_row(const FrameIndex& x, u64 f0, u64 f1, u64 total, u64 n, const u64* __restrict__ cuts, u64 lo, u64 hi, bool all, u64 i,
                                        HopAt hop_at)
{
    return fr_row_as(x, f0, f1, total, n, i, hop_at, [&](u64 s, u64 len, bool) { return !all && rx_clean(cuts, lo, hi, total, s, len); });
}

// What the list and the rows of a stream add up to.  Sums and ORs: the order in which they are joined does not matter.
struct RxAcc {
    FrAcc rows;
    u64 pstride;        // snp_comp_stride of every piece of the list
    u64 cstride;        // ... of every clean row: the pieces that are not compressed again
    u32 badlist;        // a cut that failed the list's verdict
};
// cut i of [lo, hi): ec_cut_ok after the cut before it
__host__ __device__ __forceinline__ void rx_cut(RxAcc* a, const u64* __restrict__ cuts, u64 lo, u64 i, u64 total)
{
    const u64 prev = i > lo ? cuts[i - 1] : 0, cut = cuts[i];
    if (!ec_cut_ok(prev, cut, total)) a->badlist = 1;
    else a->pstride += ec_stride(cut - prev);
}
// the piece behind the last cut (once per stream).  A last cut at or above total wraps to a length no chunk may have.
__host__ __device__ __forceinline__ void rx_tail(RxAcc* a, const u64* __restrict__ cuts, u64 lo, u64 hi, u64 total)
{
    const u64 last = hi > lo ? cuts[hi - 1] : 0;
    if (!ec_tail_ok(last, total)) a->badlist = 1;
    else if (total) a->pstride += ec_stride(total - last);
}
__host__ __device__ inline void rx_add(RxAcc* a, const FrameIndex& x, u64 f0, u64 f1, u64 total, u64 n, u64 i, const FrRow& r)
{
    fr_add(&a->rows, x, f0, f1, total, n, i, r);
    if (r.ok && r.clean) a->cstride += ec_stride(r.len);
}

struct RxPlan {
    i32 status;         // SNP_OK: the stream passed (work: it is to be written, else it is canonical and left alone); else its answer
    bool work;
    u64 f0, rows;       // the stream's old rows (clamped; also of a stream that did not pass)
    u64 dirty, dbytes;  // rows to decode and what they decode to
    u64 pieces, rebuilt;// chunks of the new stream, and those of them that are compressed again
    u64 copied;         // ... and those that are copied (the clean rows)
    u64 kept;           // bytes of the chunks that are copied
    u64 cbytes;         // compressed staging: the sum of snp_comp_stride over the rebuilt pieces
    u64 bound;          // size bound of the new stream from the headers alone (0 for a stream that is left alone or refused)
};

// The plan of stream b from fr_begin's verdict `begin` and what its list and rows add up to.  range: ec_range_ok of [lo, hi) -- without it
// neither the list nor a row was looked at.  ident: fr_ident of its bytes.
__host__ __device__ inline RxPlan rx_finish(const FrameIndex& x, u32 b, u64 n, u64 lo, u64 hi, bool range, bool all, bool ident, i32 begin, const RxAcc& acc)
{
    RxPlan k{};
    fr_rows(x, b, &k.f0, &k.rows);
    k.status = begin;
    if (begin != SNP_OK) return k;
    const u64 total = x.total[b];
    k.status = SNP_ERR_BAD_ARG;
    if (!range || acc.badlist || acc.rows.bad || (k.rows == 0 && total != 0)) return k;      // a bad list; decoded bytes and no row that holds them
    k.status = SNP_OK;
    if (!all && !acc.rows.loose && ident && (k.rows != 0 || n == SNP_STREAM_HEADER_LEN)) return k;  // canonical already
    k.work = true;
    k.dirty = acc.rows.dirty;
    k.dbytes = acc.rows.dbytes;
    k.pieces = ec_pieces(lo, hi, total);
    k.copied = acc.rows.clean < k.pieces ? acc.rows.clean : k.pieces;   // (every clean row is one piece)
    k.rebuilt = k.pieces - k.copied;
    k.kept = acc.rows.kept;
    k.cbytes = acc.pstride > acc.cstride ? acc.pstride - acc.cstride : 0;
    k.bound = SNP_STREAM_HEADER_LEN + k.kept + SNP_CHUNK_HEADER_LEN * k.rebuilt + k.dbytes;
    return k;
}

// the whole plan by one thread: the host's walk (the kernel joins the same calls over a workgroup)
template <class HopAt>
__host__ __device__ inline RxPlan rx_plan(const FrameIndex& x, u32 b, u64 n, const u64* __restrict__ cut_first, const u64* __restrict__ cuts, u64 ncuts, bool all,
                                          bool ident, HopAt hop_at)
{
    const i32 begin = fr_begin(x, b);
    const u64 lo = cut_first[b], hi = cut_first[b + 1], total = x.total[b];
    const bool range = ec_range_ok(lo, hi, ncuts);
    RxAcc acc{};
    if (begin == SNP_OK && range) {
        for (u64 i = lo; i < hi; ++i) rx_cut(&acc, cuts, lo, i, total);
        rx_tail(&acc, cuts, lo, hi, total);
        u64 f0, rows;
        fr_rows(x, b, &f0, &rows);
        for (u64 i = f0; i < f0 + rows; ++i) rx_add(&acc, x, f0, f0 + rows, total, n, i, rx_row(x, f0, f0 + rows, total, n, cuts, lo, hi, all, i, hop_at));
    }
    return rx_finish(x, b, n, lo, hi, range, all, ident, begin, acc);
}

// what a stream asks of the bounds, as the admission scans count it: decode rows and compressor slots (against max_slots), the ONE staging
// budget -- what its dirty rows decode to plus the compressed staging of its rebuilt pieces -- and rows of the new index, the larger of its old
// and its new rows.  rx_count_dec: the decoded part of the staging alone (where the stream's dirty rows are decoded to).
__host__ __device__ __forceinline__ u64 rx_count_dirty(const RxPlan& k) { return !k.work ? 0 : k.dirty < kFrMaxCount ? k.dirty : kFrMaxCount; }
__host__ __device__ __forceinline__ u64 rx_count_slots(const RxPlan& k) { return !k.work ? 0 : k.rebuilt < kFrMaxCount ? k.rebuilt : kFrMaxCount; }
__host__ __device__ __forceinline__ u64 rx_count_dec(const RxPlan& k) { return !k.work ? 0 : k.dbytes < kFrMaxStage ? k.dbytes : kFrMaxStage; }
__host__ __device__ __forceinline__ u64 rx_count_stage(const RxPlan& k)
{
    if (!k.work) return 0;
    return k.dbytes < kFrMaxStage && k.cbytes < kFrMaxStage - k.dbytes ? k.dbytes + k.cbytes : kFrMaxStage;
}
__host__ __device__ __forceinline__ u64 rx_count_rows(const RxPlan& k)
{
    const u64 most = k.work && k.pieces > k.rows ? k.pieces : k.rows;
    return most < kFrMaxCount ? most : kFrMaxCount;
}
// the bound a caller passes for stage_cap: it always holds rx_count_stage
__host__ __device__ __forceinline__ u64 rx_stage_bound(u64 dbytes, u64 rebuilt) { return dbytes + ec_stage_bound(dbytes, rebuilt); }

// Piece j < pieces of the new stream of a stream that passed: the read call's search finds the first row that ends above the piece's start; the
// piece is KEPT when that row starts there and ends where the piece ends.
struct RxPiece {
    bool kept;
    u64 row;        // the old row that holds the piece's first byte (kept: the row that IS the piece)
    u64 at;         // where the piece starts
    u32 len;
};
__host__ __device__ inline RxPiece rx_piece(const FrameIndex& x, u64 f0, u64 f1, u64 total, const u64* __restrict__ cuts, u64 lo, u64 hi, bool all, u64 j)
{
    RxPiece p{};
    p.len = ec_piece(cuts, lo, hi, total, j, &p.at);                    // (a good list: at most 65 536)
    p.row = ix_first_where(f0, f1, [&](u64 i) { return ix_row_end(x, f1, total, i) > p.at; });
    if (p.row >= f1) return p;                                          // (no sound index)
    const u64 s = x.start[p.row], e = ix_row_end(x, f1, total, p.row);
    p.kept = !all && s == p.at && e == p.at + p.len;
    return p;
}

// The rebuilt pieces and the dirty rows.  A dirty row [s, s + len) holds the first byte of the pieces that start inside it:
__host__ __device__ inline u64 rx_row_pieces(const u64* __restrict__ cuts, u64 lo, u64 hi, u64 s, u64 len)
{
    return ec_first_piece_from(cuts, lo, hi, s + len) - ec_first_piece_from(cuts, lo, hi, s);
}
// With pbefore = the pieces that start in the stream's dirty rows before the row that starts at s (a scan over the rows): the m-th rebuilt piece,
// m >= pbefore, found in that row, is piece ...
__host__ __device__ inline u64 rx_piece_of_slot(const u64* __restrict__ cuts, u64 lo, u64 hi, u64 s, u64 pbefore, u64 m)
{
    return ec_first_piece_from(cuts, lo, hi, s) + (m - pbefore);
}
// ... and rebuilt piece j, which starts inside that row, is the stream's slot
__host__ __device__ inline u64 rx_slot_of_piece(const u64* __restrict__ cuts, u64 lo, u64 hi, u64 s, u64 pbefore, u64 j)
{
    return pbefore + (j - ec_first_piece_from(cuts, lo, hi, s));
}
// a piece that starts at `at` inside the dirty row that starts at s and is decoded to `place`: where the piece lies in staging
__host__ __device__ __forceinline__ u64 rx_place(u64 place, u64 s, u64 at) { return place + (at - s); }

}  // namespace

// frame_rechunk_device.h -- the planning of the indexed RECHUNK (snp_frame_rechunk_indexed_batch, frame_rechunk.hip) over a chunk index that is
// UNTRUSTED input, on top of frame_index_device.h (the index, its clamps, the search, the rule of a row against its header) and
// frame_chunked_device.h (pieces of chunk_bytes): the verdict of a stream before its rows are looked at, the check of ONE row and what it adds to
// its stream (FrAcc: the kernel has a workgroup walk the rows and joins what its threads found, the host walks them in a loop) -- these in
// frame_rows_device.h, which the recut to a cut list (frame_recut_device.h) shares; here the grid's rule of a clean row -- the plan those
// sums give (left alone as canonical, or its dirty rows, rebuilt pieces, staging bytes and size bound), what a stream asks of each bound, and
// piece k of the new stream: kept (and which old row it is) or rebuilt.  __host__ __device__ throughout, so that the same code runs on the CPU
// under sanitizers (tests/abi/frame_rechunk_plan_check.hip) over indexes filled with anything at all and over positions and lengths past 4 GiB.
// DESIGN.md 4.20.
//
// The canonical stream of b for chunk_bytes cb: the identifier, then piece k = [k cb, min((k + 1) cb, total)) of what the stream decodes to as one
// data chunk.  A row of positive length is CLEAN when it starts on a multiple of cb and is cb bytes long (or at most cb and ends the stream): its
// chunk IS piece start / cb and is copied.  Every other row is DIRTY: it is decoded.  The clean rows are whole pieces, so the dirty rows cover
// exactly the other pieces, in order: the decoded dirty rows back to back ARE the rebuilt pieces back to back.
#pragma once
#include "frame_rows_device.h"
#include "frame_chunked_device.h"

namespace {

constexpr u32 kFrRewriteAll = 1u;                           // SNP_RECHUNK_REWRITE_ALL

__host__ __device__ __forceinline__ bool fr_clean(u64 start, u64 len, bool at_end, u32 cb)
{
    return len > 0 && start % cb == 0 && (len == cb || (len <= cb && at_end));
}

// row i against the grid of cb (fr_row_as, frame_rows_device.h: the check itself)
template <class HopAt>
__host__ __device__ inline FrRow fr_row(const FrameIndex& x, u64 f0, u64 f1, u64 total, u64 n, u32 cb, bool all, u64 i, HopAt hop_at)
{
    return fr_row_as(x, f0, f1, total, n, i, hop_at, [&](u64 s, u64 len, bool at_end) { return !all && fr_clean(s, len, at_end, cb); });
}

struct FrPlan {
    i32 status;         // SNP_OK: the stream passed (work: it is to be written, else it is canonical and left alone); else its answer
    bool work;
    bool last;          // the new stream's last piece is rebuilt (it may be shorter than cb)
    u64 f0, rows;       // the stream's old rows (clamped; also of a stream that did not pass)
    u64 dirty, dbytes;  // rows to decode and the staging bytes they need
    u64 pieces, rebuilt;// chunks of the new stream, and those of them that are compressed again
    u64 kept;           // bytes of the chunks that are copied
    u64 bound;          // size bound of the new stream from the headers alone (0 for a stream that is left alone or refused)
};

// The plan of stream b from fr_begin's verdict `begin` and what its rows add up to.  ident: fr_ident of its bytes.
__host__ __device__ inline FrPlan fr_finish(const FrameIndex& x, u32 b, u64 n, u32 cb, bool all, bool ident, i32 begin, const FrAcc& acc)
{
    FrPlan k{};
    fr_rows(x, b, &k.f0, &k.rows);
    k.status = begin;
    if (begin != SNP_OK) return k;
    const u64 total = x.total[b];
    k.status = SNP_ERR_BAD_ARG;
    if (acc.bad || (k.rows == 0 && total != 0)) return k;               // decoded bytes and no row that holds them
    k.status = SNP_OK;
    if (!all && !acc.loose && ident && (k.rows != 0 || n == SNP_STREAM_HEADER_LEN)) return k;       // canonical already
    k.work = true;
    k.last = acc.last != 0;
    k.dirty = acc.dirty;
    k.dbytes = acc.dbytes;
    k.pieces = fc_chunks(total, cb);
    k.rebuilt = k.pieces - acc.clean;                                   // (every clean row is one piece)
    k.kept = acc.kept;
    k.bound = SNP_STREAM_HEADER_LEN + k.kept + SNP_CHUNK_HEADER_LEN * k.rebuilt + k.dbytes;
    return k;
}

// the whole plan by one thread: the host's walk (the kernel joins the same calls over a workgroup)
template <class HopAt>
__host__ __device__ inline FrPlan fr_plan(const FrameIndex& x, u32 b, u64 n, u32 cb, bool all, bool ident, HopAt hop_at)
{
    const i32 begin = fr_begin(x, b);
    FrAcc acc{};
    if (begin == SNP_OK) {
        u64 f0, rows;
        fr_rows(x, b, &f0, &rows);
        for (u64 i = f0; i < f0 + rows; ++i) fr_add(&acc, x, f0, f0 + rows, x.total[b], n, i, fr_row(x, f0, f0 + rows, x.total[b], n, cb, all, i, hop_at));
    }
    return fr_finish(x, b, n, cb, all, ident, begin, acc);
}

// what a stream asks of the bounds, as the admission scans count it: decode rows and compressor slots (against max_slots), staging bytes, and
// rows of the new index -- a stream that is to be written is counted with the larger of its old and its new rows, so that its rows fit whatever
// becomes of it
__host__ __device__ __forceinline__ u64 fr_count_dirty(const FrPlan& k) { return !k.work ? 0 : k.dirty < kFrMaxCount ? k.dirty : kFrMaxCount; }
__host__ __device__ __forceinline__ u64 fr_count_slots(const FrPlan& k) { return !k.work ? 0 : k.rebuilt < kFrMaxCount ? k.rebuilt : kFrMaxCount; }
__host__ __device__ __forceinline__ u64 fr_count_stage(const FrPlan& k) { return !k.work ? 0 : k.dbytes < kFrMaxStage ? k.dbytes : kFrMaxStage; }
__host__ __device__ __forceinline__ u64 fr_count_rows(const FrPlan& k)
{
    const u64 most = k.work && k.pieces > k.rows ? k.pieces : k.rows;
    return most < kFrMaxCount ? most : kFrMaxCount;
}

// Piece k < pieces of the new stream of a stream that passed: the read call's search finds the first row that ends above k cb; the piece is KEPT
// when that row is clean and starts there.
struct FrPiece {
    bool kept;
    u64 row;        // the old row that holds the piece's first byte (kept: the row that IS the piece)
    u64 at;         // k cb
    u32 len;
};
__host__ __device__ inline FrPiece fr_piece(const FrameIndex& x, u64 f0, u64 f1, u64 total, u32 cb, bool all, u64 k)
{
    FrPiece p{};
    p.at = k * cb;                                                      // (k < fc_chunks(total, cb): below total)
    p.len = total - p.at < cb ? static_cast<u32>(total - p.at) : cb;
    p.row = ix_first_where(f0, f1, [&](u64 i) { return ix_row_end(x, f1, total, i) > p.at; });
    if (p.row >= f1) return p;                                          // (no sound index)
    const u64 s = x.start[p.row], e = ix_row_end(x, f1, total, p.row);
    p.kept = !all && s == p.at && e >= s && fr_clean(s, e - s, e == total, cb);
    return p;
}

// the m-th rebuilt piece of a stream: where it lies among the stream's staging bytes, and its length
__host__ __device__ __forceinline__ u64 fr_slot_off(u32 cb, u64 m) { return m * cb; }
__host__ __device__ __forceinline__ u32 fr_slot_len(bool last, u64 rebuilt, u64 pieces, u64 total, u32 cb, u64 m)
{
    return last && m + 1 == rebuilt ? static_cast<u32>(total - (pieces - 1) * cb) : cb;
}

}  // namespace

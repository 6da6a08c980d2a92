// frame_rechunk_device.h -- the planning of the indexed RECHUNK (snp_frame_rechunk_indexed_batch, frame_rechunk.hip) over a chunk index that is
// UNTRUSTED input, on top of frame_index_device.h (the index, its clamps, the search, the rule of a row against its header) and
// frame_chunked_device.h (pieces of chunk_bytes): the verdict of a stream before its rows are looked at, the check of ONE row and what it adds to
// its stream (FrAcc: the kernel has a workgroup walk the rows and joins what its threads found, the host walks them in a loop), the plan those
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
#include "frame_index_device.h"
#include "frame_chunked_device.h"

namespace {

constexpr u32 kFrRewriteAll = 1u;                           // SNP_RECHUNK_REWRITE_ALL
constexpr u32 kFrMaxDec = SNP_BLOCK_SIZE;                   // what a dirty row may decode to
constexpr u64 kFrMaxCount = 1ull << 32;                     // no bound admits 2^32 rows or slots: a stream is counted as at most that, so that no scan wraps
constexpr u64 kFrMaxStage = 1ull << 48;                     // ... and as at most the staging bytes of that many dirty rows

// the old rows of stream b: [f0, f0 + rows), inside nentries whatever idx_first holds (f1 < f0: none)
__host__ __device__ __forceinline__ void fr_rows(const FrameIndex& x, u32 b, u64* f0, u64* rows)
{
    const u64 a = x.first[b] < x.nentries ? x.first[b] : x.nentries, e = x.first[b + 1] < x.nentries ? x.first[b + 1] : x.nentries;
    *f0 = a;
    *rows = e > a ? e - a : 0;
}

// The verdict of stream b before its rows are looked at: SNP_OK, the status that ended its walk, or SNP_ERR_BAD_ARG.
__host__ __device__ __forceinline__ i32 fr_begin(const FrameIndex& x, u32 b)
{
    const i32 walk = x.tail[b];
    if (walk < SNP_OK || walk > SNP_ERR_TRUNCATED_STREAM) return SNP_ERR_BAD_ARG;      // (no status of the walk)
    if (walk != SNP_OK) return walk;                                    // not indexed, or broken: a broken stream is not rechunked
    const u64 g0 = x.first[b] < x.nentries ? x.first[b] : x.nentries, g1 = x.first[b + 1] < x.nentries ? x.first[b + 1] : x.nentries;
    return g1 < g0 ? SNP_ERR_BAD_ARG : SNP_OK;
}

// in[0, 10) is the stream identifier
__host__ __device__ __forceinline__ bool fr_ident(const u8* __restrict__ p, u64 n)
{
    constexpr u8 id[SNP_STREAM_HEADER_LEN] = {0xff, 0x06, 0x00, 0x00, 0x73, 0x4e, 0x61, 0x50, 0x70, 0x59};
    if (n < SNP_STREAM_HEADER_LEN) return false;
    bool same = true;
    for (u32 i = 0; i < SNP_STREAM_HEADER_LEN; ++i) same = same && p[i] == id[i];
    return same;
}

__host__ __device__ __forceinline__ bool fr_clean(u64 start, u64 len, bool at_end, u32 cb)
{
    return len > 0 && start % cb == 0 && (len == cb || (len <= cb && at_end));
}

// Row i of a stream of n bytes whose rows are [f0, f1): with the rows before and behind it, it is one part of a partition of [0, total) -- the
// first row starts at 0, a row ends at or above its start (the last one at total) -- its header is read again inside the stream and holds
// (ix_row_holds), the next row's header lies at or behind the end of its chunk, and a dirty row decodes to no more than 65536 bytes.
// hop_at(pos) -> the Hop of the header at pos < n.
struct FrRow {
    bool ok, clean;
    u64 start, len, pos;
    Hop h;
};
template <class HopAt>
__host__ __device__ inline FrRow fr_row(const FrameIndex& x, u64 f0, u64 f1, u64 total, u64 n, u32 cb, bool all, u64 i, HopAt hop_at)
{
    FrRow r{};
    const u64 s = x.start[i], e = ix_row_end(x, f1, total, i), pos = x.pos[i];
    if ((i == f0 && s != 0) || e < s || pos >= n) return r;
    r.h = hop_at(pos);
    if (!ix_row_holds(s, e, r.h)) return r;
    if (i + 1 < f1 && x.pos[i + 1] < r.h.next) return r;               // positions strictly increasing, the chunks apart
    r.start = s;
    r.len = e - s;
    r.pos = pos;
    r.clean = !all && fr_clean(s, r.len, e == total, cb);
    r.ok = r.clean || r.len <= kFrMaxDec;
    return r;
}

// What the rows of a stream add up to.  Sums and ORs: the order in which rows are joined does not matter.
struct FrAcc {
    u64 dirty, dbytes;  // dirty rows and what they decode to
    u64 clean, kept;    // clean rows and the bytes of their chunks in the stream (4 + size each)
    u32 bad;            // a row that failed its check
    u32 loose;          // not canonical: a dirty row, a chunk that does not lie right behind the one before (the first at 10, the last up to in_len)
    u32 last;           // the row that holds the stream's last byte is dirty
};
__host__ __device__ __forceinline__ void fr_join(FrAcc* a, const FrAcc& b)
{
    a->dirty += b.dirty;
    a->dbytes += b.dbytes;
    a->clean += b.clean;
    a->kept += b.kept;
    a->bad |= b.bad;
    a->loose |= b.loose;
    a->last |= b.last;
}
__host__ __device__ inline void fr_add(FrAcc* a, const FrameIndex& x, u64 f0, u64 f1, u64 total, u64 n, u64 i, const FrRow& r)
{
    if (!r.ok) { a->bad = 1; return; }
    if (r.clean) {
        a->clean += 1;
        a->kept += r.h.next - r.pos;
    } else {
        a->dirty += 1;
        a->dbytes += r.len;
        a->loose = 1;
        if (r.len && r.start + r.len == total) a->last = 1;
    }
    if ((i == f0 && r.pos != SNP_STREAM_HEADER_LEN) || (i + 1 < f1 ? x.pos[i + 1] != r.h.next : r.h.next != n)) a->loose = 1;
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

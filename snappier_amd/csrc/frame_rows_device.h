// frame_rows_device.h -- the checks over the old rows of a seekable stream that the calls which bring a stream to a given partition share: the
// rechunk to a grid (frame_rechunk_device.h) and the recut to a cut list (frame_recut_device.h).  The chunk index is UNTRUSTED input: the verdict
// of a stream before its rows are looked at, the clamp of its rows, the identifier, the check of ONE row (fr_row_as; which rows are CLEAN is the
// caller's rule, handed in) and what a row adds to its stream (FrAcc).  __host__ __device__ throughout, as the two headers on top of it are.
// DESIGN.md 4.20, 4.28.
#pragma once
#include "frame_index_device.h"

namespace {

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

// Row i of a stream of n bytes whose rows are [f0, f1): with the rows before and behind it, it is one part of a partition of [0, total) -- the
// first row starts at 0, a row ends at or above its start (the last one at total) -- its header is read again inside the stream and holds
// (ix_row_holds), the next row's header lies at or behind the end of its chunk, and a dirty row decodes to no more than 65536 bytes.
// hop_at(pos) -> the Hop of the header at pos < n; is_clean(start, len, ends the stream) -> the row's chunk is a piece of the new stream as it is.
struct FrRow {
    bool ok, clean;
    u64 start, len, pos;
    Hop h;
};
template <class HopAt, class Clean>
__host__ __device__ inline FrRow fr_row_as(const FrameIndex& x, u64 f0, u64 f1, u64 total, u64 n, u64 i, HopAt hop_at, Clean is_clean)
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
    r.clean = is_clean(s, r.len, e == total);
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

}  // namespace

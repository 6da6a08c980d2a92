// frame_splice_device.h -- the planning of the indexed SPLICE (snp_frame_splice_indexed_batch, frame_splice.hip) over a chunk index that is UNTRUSTED
// input, on top of frame_index_device.h (the index, its clamps, the two searches, the hop) and frame_chunked_device.h (pieces of chunk_bytes, the
// owner of a slot): the plan of ONE stream (its verdict before anything is decoded, the rows the splice owns, the check of the first and the last
// of them against the headers they point at, the edges, the hole [P0, P1), |H| and |T|, the pieces of the rewritten region, the staging bytes
// and the size bound), piece j's length and place in the region, in 64 bits, and the three kinds of row of the new index.  __host__ __device__
// throughout, so that the same code runs on the CPU under sanitizers (tests/abi/frame_splice_plan_check.hip) over indexes filled with anything at
// all and over positions and lengths past 4 GiB.  DESIGN.md 4.19.
//
// ONE splice per stream: in what the stream decodes to, [lo, hi) = [off, off + del) is replaced by ins source bytes.  The rows [r0, r1) are the
// splice's own; H = the decoded bytes [start[r0], lo) and T = [hi, end[r1 - 1]) are the EDGES it keeps of them, and everything of the old stream
// in [P0, P1) = [pos[r0], the end of the chunk at pos[r1 - 1]) is replaced by the chunks of R = H || source bytes || T.
#pragma once
#include "frame_index_device.h"
#include "frame_chunked_device.h"

namespace {

constexpr u32 kFsMaxDec = SNP_BLOCK_SIZE;                   // what an edge may decode to
constexpr u64 kFsMaxPieces = 1ull << 32;                    // no bound admits 2^32 slots: a stream is counted as at most that, so that the scan cannot wrap
constexpr u64 kFsMaxStage = (1ull << 48) + (1ull << 18);    // ... and as at most the staging bytes of that many pieces and two edges

struct FsPlan {
    i32 status;         // SNP_OK: the stream passed (splice: it is named, else it is left alone); else its answer
    bool splice;        // passed and del + ins > 0
    bool ident;         // an empty stream: the identifier goes first
    bool head, tail;    // H / T is not empty: the row it lies in is decoded
    u32 hl, tl;         // |H|, |T|
    u32 e0, e1;         // decoded bytes of the head row when it is decoded, and of the tail row when it is another one
    u64 f0, rows;       // the stream's old rows [f0, f0 + rows) (clamped; also of a stream that did not pass)
    u64 r0, r1;         // the rows the splice owns (absolute); r0 == r1: none
    u64 p0, p1;         // the hole, stream-relative
    u64 tpos;           // the header of row r1 - 1 (p0 is that of row r0)
    u64 region, pieces; // |R| and its chunks
    u64 stage;          // staging bytes: e0 + e1 + |R|
    u64 bound;          // size bound of the new stream, from the headers alone (0 for a stream that is left alone or refused)
};

// the old rows of stream b as the new index copies them: [f0, f0 + rows), inside nentries whatever idx_first holds
__host__ __device__ __forceinline__ void fs_rows(const FrameIndex& x, u32 b, u64* f0, u64* rows)
{
    const u64 a = x.first[b] < x.nentries ? x.first[b] : x.nentries, e = x.first[b + 1] < x.nentries ? x.first[b + 1] : x.nentries;
    *f0 = a;
    *rows = e > a ? e - a : 0;
}

// Stream b of n = in_len bytes, its decoded bytes [off, off + del) replaced by ins bytes, in chunks of cb.  hop_at(pos) -> the Hop of the header at
// pos < n (frame_hop over the stream's bytes; the check program also gives hops as numbers, for streams too long to hold).
template <class HopAt>
__host__ __device__ inline FsPlan fs_plan_unchecked(const FrameIndex& x, u32 b, u64 n, u64 off, u64 del, u64 ins, u32 cb, HopAt hop_at);
template <class HopAt>
__host__ __device__ inline FsPlan fs_plan(const FrameIndex& x, u32 b, u64 n, u64 off, u64 del, u64 ins, u32 cb, HopAt hop_at)
{
    const FsPlan k = fs_plan_unchecked(x, b, n, off, del, ins, cb, hop_at);
    if (k.splice) return k;
    FsPlan z{};                                                         // left alone or refused: the verdict and the old rows, nothing half-planned
    z.status = k.status;
    z.f0 = z.r0 = z.r1 = k.f0;
    z.rows = k.rows;
    return z;
}
template <class HopAt>
__host__ __device__ inline FsPlan fs_plan_unchecked(const FrameIndex& x, u32 b, u64 n, u64 off, u64 del, u64 ins, u32 cb, HopAt hop_at)
{
    FsPlan k{};
    fs_rows(x, b, &k.f0, &k.rows);
    k.r0 = k.r1 = k.f0;
    k.status = SNP_OK;
    if (del == 0 && ins == 0) return k;                                 // not named: not one array of the index is trusted for it
    k.status = SNP_ERR_BAD_ARG;
    const i32 walk = x.tail[b];
    if (walk < SNP_OK || walk > SNP_ERR_TRUNCATED_STREAM) return k;     // (no status of the walk)
    if (walk != SNP_OK) { k.status = walk; return k; }                  // not indexed, or broken: a broken stream is not spliced
    const u64 g0 = x.first[b] < x.nentries ? x.first[b] : x.nentries, g1 = x.first[b + 1] < x.nentries ? x.first[b + 1] : x.nentries;
    if (g1 < g0) return k;
    const u64 total = x.total[b], lo = off, hi = off + del;
    if (hi < lo || hi > total) return k;
    if (total - del + ins < ins) return k;                              // the new length wraps
    u64 s0 = lo, e1 = hi;                                               // where the owned rows start and end in the decoded bytes
    if (del == 0 && lo == total) {                                      // at the very end: no row, behind the stream's last byte
        if (g1 == g0 && total != 0) return k;                           // decoded bytes and no row that holds them
        k.r0 = k.r1 = g1;
        k.p0 = k.p1 = k.tpos = n;
    } else {
        const u64 i0 = ix_first_where(g0, g1, [&](u64 i) { return ix_row_end(x, g1, total, i) > lo; });
        if (i0 >= g1) return k;                                         // bytes and no row that holds them
        u64 i1 = i0 + 1;
        if (del) {
            i1 = ix_first_where(g0, g1, [&](u64 i) { return x.start[i] >= hi; });
            if (i1 <= i0) return k;                                     // rows that run backwards
        }
        s0 = x.start[i0];
        if (s0 > lo) return k;
        const u64 pos0 = x.pos[i0];
        if (pos0 >= n) return k;
        const Hop h0 = hop_at(pos0);
        if (h0.kind != HOP_DATA) return k;
        k.r0 = i0;
        k.p0 = pos0;
        if (del == 0 && s0 == lo) {                                     // on a chunk boundary: no row, in front of this header
            k.r1 = i0;
            k.p1 = k.tpos = pos0;
            e1 = lo;
        } else {
            const u64 z0 = ix_row_end(x, g1, total, i0);
            if (z0 < s0 || z0 - s0 != h0.dec) return k;                 // a data chunk that decodes to exactly end - start bytes
            Hop h1 = h0;
            const u64 last = i1 - 1;
            k.tpos = pos0;
            if (last != i0) {
                const u64 s1 = x.start[last], pos1 = x.pos[last];
                e1 = ix_row_end(x, g1, total, last);
                if (e1 < s1 || pos1 >= n || pos1 < h0.next) return k;   // the second header at or after the end of the first chunk
                h1 = hop_at(pos1);
                if (h1.kind != HOP_DATA || e1 - s1 != h1.dec) return k;
                k.tpos = pos1;
            } else {
                e1 = z0;
            }
            if (e1 < hi) return k;                                      // the owned rows must hold the hole
            k.r1 = i1;
            k.p1 = h1.next;                                             // (a hop never runs past n: P1 <= in_len)
            k.head = s0 < lo;
            k.tail = e1 > hi;
            if ((k.head && h0.dec > kFsMaxDec) || (k.tail && h1.dec > kFsMaxDec)) return k;
            k.hl = static_cast<u32>(lo - s0);                           // (< h0.dec <= 65536 when there is a head)
            k.tl = static_cast<u32>(e1 - hi);
            k.e0 = k.head ? h0.dec : 0;
            k.e1 = k.tail && !(k.head && last == i0) ? h1.dec : 0;
        }
    }
    k.status = SNP_OK;
    k.splice = true;
    k.ident = n == 0;
    k.region = static_cast<u64>(k.hl) + ins + k.tl;                     // (<= total - del + ins: no wrap)
    k.pieces = fc_chunks(k.region, cb);
    k.stage = static_cast<u64>(k.e0) + k.e1 + k.region;
    if (k.stage < k.region) k.stage = ~0ull;
    k.bound = n - (k.p1 - k.p0) + SNP_CHUNK_HEADER_LEN * k.pieces + k.region + (k.ident ? SNP_STREAM_HEADER_LEN : 0);
    return k;
}

// what a stream asks of the two bounds, as the admission scans count it
__host__ __device__ __forceinline__ u64 fs_count_pieces(const FsPlan& k) { return !k.splice ? 0 : k.pieces < kFsMaxPieces ? k.pieces : kFsMaxPieces; }
__host__ __device__ __forceinline__ u64 fs_count_stage(const FsPlan& k) { return !k.splice ? 0 : k.stage < kFsMaxStage ? k.stage : kFsMaxStage; }

// Piece j of a region of `region` bytes: its bytes and where they start in the region
struct FsPiece { u32 len; u64 off; };
__host__ __device__ __forceinline__ FsPiece fs_piece(u64 region, u32 cb, u64 j)
{
    const u64 at = j * cb, left = region - at;                          // (j < fc_chunks(region, cb): at < region)
    return FsPiece{left < cb ? static_cast<u32>(left) : cb, at};
}

// The rows of a written stream's new index, in order: its old rows before r0 as they are; one row per new chunk (its pos comes from the size
// scan); its old rows from r1 on, moved by what the splice did to the decoded bytes and to the stream's bytes.
__host__ __device__ __forceinline__ u64 fs_row_start(u64 lo, u32 hl, u32 cb, u64 j) { return lo - hl + j * cb; }
__host__ __device__ __forceinline__ u64 fs_moved_start(u64 start, u64 del, u64 ins) { return start + ins - del; }
__host__ __device__ __forceinline__ u64 fs_moved_pos(u64 pos, u64 p0, u64 p1, u64 new_bytes) { return pos + (new_bytes - (p1 - p0)); }
// rows of the new index of a stream: rows - (r1 - r0) + pieces when it is written, else its old rows
__host__ __device__ __forceinline__ u64 fs_new_rows(u64 rows, u64 r0, u64 r1, u64 pieces) { return rows - (r1 - r0) + pieces; }

}  // namespace

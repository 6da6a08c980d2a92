// frame_diff.hip -- snp_frame_diff_indexed_batch: the longest common prefix and suffix of pairs of windows of what seekable framed streams
// decode to.  Wherever both streams have a chunk boundary at the same decoded offset, the span between two such common cuts is compared from
// the CRCs the chunk headers carry (CRC is GF(2)-linear: frame_digest_device.h); only the first span whose CRCs differ and the ragged pieces
// no common cut covers are decoded and compared byte for byte.  Built into libsnappier_hip_frame_diff.so (C-ABI:
// include/snappier_hip_frame_diff.h), linked against libsnappier_hip.so.  DESIGN.md 4.23.
//
//   plan      one thread per request: the indexed read's plan of both sides, the rows they own; every piece empty
//   scan      owned rows over the requests -> each request's place in the table of side B's exclusive XORs (d_result[0]; max_rows bounds it)
//   cuts      one wavefront per request and direction (frame_diff_device.h says what it finds): side B's rows, 64 at a time -- the check of
//             each, its term, the exclusive XOR into the table; then side A's rows, 64 at a time -- check, term, running XOR, a binary search
//             in side B's rows for a boundary at the row's far edge -> the first common cut, the first cut where the sides' XORs part, the cut
//             before it -> the at most two pieces the direction decodes, their rows and bytes on both sides
//   final     one thread per request: a request with a row that failed its check decodes nothing; suffix and prefix share one whole window
//   scans     per side the pieces' bytes -> each run's place in scratch (side A from the front, side B from the back) and the pieces' rows ->
//             each piece's rows in that side's chunk table
//   rows      one thread per row of the two chunk tables (min(2 x max_rows, scratch_cap) rows each)
//   decode    snp_ctx::decode_chunks, once per side, into scratch
//   fail      the first failing decoded row of each side, in stream order
//   compare   workgroups stride over each piece 4 KiB at a time, 16 bytes per lane; the first mismatch by ballot and atomicMin
//   verdict   one thread per request
// Nothing here allocates, reads back or synchronises: the call is capturable like the other _batch entry points.
#include "capi_internal.h"
#include "scan_tiles.h"
#include "frame_edges_device.h"
#include "frame_diff_device.h"
#include "bytes16_device.h"
#include "../../include/snappier_hip_frame_diff.h"

namespace {

constexpr u32 kBadA = 1u, kBadB = 2u;           // flags: a row of that side failed its check
constexpr u32 kPlanShiftA = 8, kPlanShiftB = 16;   // (flags >> shift) & 0xff: that side's plan status
constexpr u32 kCompareBlock = 4096;             // bytes a workgroup compares per step

struct DiffSideArgs {
    const u8* in;
    const u64 *in_off, *in_len;
    u32 ns;
    FrameIndex x;
    const u32* req_stream;
    const u64 *req_off, *req_len;
};
struct DiffArgs {
    DiffSideArgs s[2];
    u32 nreq, flags;
    u64 max_rows, scratch_cap;
};

// piece p4 = (request * 2 + direction) * 2 + piece; per side its rows, bytes and places
struct DfPieceSide {
    u64 *row0, *nrows, *bytes, *off;
    u64* charge;                // what the run takes of scratch_cap: its bytes, and no less than one byte per row (a zero-length chunk costs one)
    u64 *place, *rplace;        // the scans of charge and nrows (4 nreq + 1 each)
};
struct DfWork {
    u64 *rfirst, *part;
    u64* nrows;                 // per request: the rows both sides own (0 unless both plans are OK)
    u64 *len_a, *len_b;         // per request
    u64* fail[2];               // per request and side: min over the failing decoded rows of fail_key(header position, status)
    u32* flags;                 // per request
    DfPieceSide ps[2];
    u64 *t0, *len, *mis;        // per piece: the bytes compared and the first mismatch (counted from t0 in the direction)
    u32* src;                   // per piece: the piece whose runs it compares (itself, or the prefix's whole window)
    u32* g;                     // [2][max_rows]: side B's exclusive XORs, per direction
    ChunkRows c[2];
    u8* scratch;
    u64 bytes;
};

__device__ __forceinline__ DfSide side_of(const DiffSideArgs& a, u32 r)
{
    return df_side(a.x, a.in, a.in_off, a.in_len, a.ns, a.req_stream[r], a.req_off[r], a.req_len[r]);
}
__device__ __forceinline__ bool rows_fit(const DiffArgs& a, const DfWork& w, u32 r) { return w.rfirst[r + 1] <= a.max_rows; }
__device__ __forceinline__ bool scratch_fits(const DiffArgs& a, const DfWork& w, u32 r)
{
    return w.ps[0].place[4ull * r + 4] + w.ps[1].place[4ull * r + 4] <= a.scratch_cap;
}
// where the run of piece p4 on a side begins in scratch: side A's runs grow from the front, side B's from the back
__device__ __forceinline__ u64 run_place(const DiffArgs& a, const DfWork& w, u32 side, u64 p4)
{
    return side ? a.scratch_cap - w.ps[1].place[p4] - w.ps[1].charge[p4] : w.ps[0].place[p4];
}

struct ScanWords {
    const u64* __restrict__ src;
    __device__ __forceinline__ u64 operator()(u64 i) const { return src[i]; }
};

__global__ __launch_bounds__(256) void k_df_plan(DiffArgs a, DfWork w)
{
    const u32 r = blockIdx.x * 256u + threadIdx.x;
    if (r >= a.nreq) return;
    const DfSide A = side_of(a.s[0], r), B = side_of(a.s[1], r);
    const bool ok = A.k.status == SNP_OK && B.k.status == SNP_OK;
    w.nrows[r] = ok ? A.rows() + B.rows() : 0;
    w.len_a[r] = A.k.status == SNP_OK ? A.len() : 0;
    w.len_b[r] = B.k.status == SNP_OK ? B.len() : 0;
    w.fail[0][r] = w.fail[1][r] = kNoFail;
    w.flags[r] = (static_cast<u32>(A.k.status) & 0xffu) << kPlanShiftA | (static_cast<u32>(B.k.status) & 0xffu) << kPlanShiftB;
    for (u64 p = 4ull * r; p < 4ull * r + 4; ++p) {
        for (u32 side = 0; side < 2; ++side) w.ps[side].row0[p] = w.ps[side].nrows[p] = w.ps[side].bytes[p] = w.ps[side].off[p] = w.ps[side].charge[p] = 0;
        w.t0[p] = w.len[p] = 0;
        w.mis[p] = kDfNone;
        w.src[p] = static_cast<u32>(p);
    }
}

// inclusive XOR scan across the wavefront
__device__ __forceinline__ u32 wave_xor_scan(u32 v, u32 lane)
{
    for (u32 d = 1; d < 64; d <<= 1) {
        const u32 y = __shfl_up(v, d, 64);
        if (lane >= d) v ^= y;
    }
    return v;
}
__device__ __forceinline__ u64 lane_u64(u64 v, u32 l) { return __shfl(static_cast<unsigned long long>(v), static_cast<int>(l), 64); }

// One wavefront per (request, direction) of the requests whose rows fit; nwaves wavefronts stride over them.
__global__ __launch_bounds__(256) void k_df_cuts(DiffArgs a, DfWork w, u32 ndir, u32 dir0, u32 nwaves)
{
    const u32 lane = lane_id();
    const u64 items = static_cast<u64>(a.nreq) * ndir;
    const FrameIndex& xa = a.s[0].x;
    const FrameIndex& xb = a.s[1].x;
    for (u64 item = blockIdx.x * 4u + (threadIdx.x >> 6); item < items; item += nwaves) {
        const u32 r = static_cast<u32>(item / ndir), dir = ndir == 2 ? static_cast<u32>(item & 1) : dir0;
        if (w.nrows[r] == 0 || !rows_fit(a, w, r)) continue;            // (wave-uniform; nrows != 0: both plans are OK)
        const DfSide A = side_of(a.s[0], r), B = side_of(a.s[1], r);
        const u64 n = A.len() < B.len() ? A.len() : B.len(), rows_a = A.rows(), rows_b = B.rows();
        const bool exact = a.flags & kDiffExact, cuts = !exact && n > 0;
        // (cuts: n > 0, so side A owns a row and side B's rows_b + 1 words fit the request's rows_a + rows_b)
        u32* const gb = w.g + dir * a.max_rows + w.rfirst[r];
        DfScan s{};
        bool bad_a = false, bad_b = false;
        u32 carry = 0;
        for (u64 base = 0; base < rows_b; base += 64) {
            const u64 o = base + lane;
            DfRow rw{};
            rw.ok = true;
            if (o < rows_b) rw = df_row(xb, B, dir, n, o, cuts);
            bad_b |= !rw.ok;
            if (cuts) {
                const u32 inc = wave_xor_scan(rw.term, lane);
                if (o < rows_b) gb[o] = carry ^ inc ^ rw.term;
                carry ^= __shfl(inc, 63, 64);
            }
        }
        if (cuts) {
            if (lane == 0) gb[rows_b] = carry;
            __threadfence();                                            // the table is read back below, by other lanes
            u64 oa, ob;
            if (df_cut(xa, A, dir, 0, &oa) && df_cut(xb, B, dir, 0, &ob)) df_scan_cut(s, DfCut{0, 0, 0}, 0);
        }
        carry = 0;
        for (u64 base = 0; base < rows_a; base += 64) {
            const u64 o = base + lane;
            DfRow rw{};
            rw.ok = true;
            if (o < rows_a) rw = df_row(xa, A, dir, n, o, cuts);
            bad_a |= !rw.ok;
            if (!cuts || s.diff) continue;                              // (wave-uniform) the rest of the rows is only checked
            const u32 inc = wave_xor_scan(rw.term, lane);
            const u32 ga = carry ^ inc;
            carry ^= __shfl(inc, 63, 64);
            u64 ob = 0;
            const bool cut = o < rows_a && rw.ok && rw.full && df_cut(xb, B, dir, rw.thi, &ob);
            const u32 d = cut ? ga ^ __hip_atomic_load(gb + ob, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0;
            const u64 m = ballot64(cut);
            if (!m) continue;
            auto cut_of = [&](u32 l) { return DfCut{lane_u64(rw.thi, l), base + l + 1, lane_u64(ob, l)}; };
            if (!s.have0) {
                const u32 l = static_cast<u32>(__builtin_ctzll(m));
                df_scan_cut(s, cut_of(l), __shfl(d, static_cast<int>(l), 64));
            }
            const u64 dm = ballot64(cut && d != s.d0);
            if (dm) {
                const u32 l = static_cast<u32>(__builtin_ctzll(dm));
                const u64 below = m & ((1ull << l) - 1);
                if (below) s.last = cut_of(63u - static_cast<u32>(__builtin_clzll(below)));
                df_scan_cut(s, cut_of(l), ~s.d0);
            } else {
                s.last = cut_of(63u - static_cast<u32>(__builtin_clzll(m)));
            }
        }
        const bool any_a = ballot64(bad_a) != 0, any_b = ballot64(bad_b) != 0;
        if (lane != 0) continue;
        if (any_a || any_b) {
            atomicOr(w.flags + r, (any_a ? kBadA : 0u) | (any_b ? kBadB : 0u));
            continue;
        }
        DfPiece pc[2];
        df_pieces(s, df_need_rows(xa, A, dir, n), df_need_rows(xb, B, dir, n), n, exact, pc);
        bool good = true;
        for (u32 k = 0; k < 2; ++k) {
            const u64 p = (2ull * r + dir) * 2 + k;
            good = good && df_piece_side(xa, A, dir, pc[k].a0, pc[k].a1, pc[k].t0, pc[k].len, w.ps[0].row0 + p, w.ps[0].nrows + p, w.ps[0].bytes + p, w.ps[0].off + p);
            good = good && df_piece_side(xb, B, dir, pc[k].b0, pc[k].b1, pc[k].t0, pc[k].len, w.ps[1].row0 + p, w.ps[1].nrows + p, w.ps[1].bytes + p, w.ps[1].off + p);
            for (u32 side = 0; side < 2; ++side) w.ps[side].charge[p] = w.ps[side].bytes[p] > w.ps[side].nrows[p] ? w.ps[side].bytes[p] : w.ps[side].nrows[p];
            w.t0[p] = pc[k].t0;
            w.len[p] = pc[k].len;
        }
        if (!good) atomicOr(w.flags + r, kBadA | kBadB);                // (cannot be: every row passed its check, so the rows tile)
    }
}

// A request with a row that failed its check decodes nothing.  With both directions on windows of one length, a suffix piece that holds the
// whole window compares the runs of the prefix piece that does.
__global__ __launch_bounds__(256) void k_df_final(DiffArgs a, DfWork w, u64* __restrict__ result)
{
    const u32 r = blockIdx.x * 256u + threadIdx.x;
    if (r >= a.nreq) return;
    if (r == 0) { result[2] = 0; result[3] = 0; }
    const u64 p0 = 4ull * r, s0 = p0 + 2;
    if (w.flags[r] & (kBadA | kBadB)) {
        for (u64 q = p0; q < p0 + 4; ++q) {
            for (u32 side = 0; side < 2; ++side) w.ps[side].nrows[q] = w.ps[side].bytes[q] = w.ps[side].charge[q] = 0;
            w.len[q] = 0;
        }
        return;
    }
    const u64 n = w.len_a[r];
    if (n == 0 || n != w.len_b[r]) return;
    const u64 p = w.len[p0] == n ? p0 : p0 + 1, s = w.len[s0] == n ? s0 : s0 + 1;   // (one piece of a direction at most holds all n bytes)
    if (w.len[p] == n && w.len[s] == n) {
        for (u32 side = 0; side < 2; ++side) w.ps[side].nrows[s] = w.ps[side].bytes[s] = w.ps[side].charge[s] = 0;
        w.src[s] = static_cast<u32>(p);
    }
}

// One thread per row of a side's chunk table: an empty row unless it belongs to a piece of an admitted request and passes the check again,
// now against its piece's run, so that it writes inside the run whatever the index says.
__global__ __launch_bounds__(256) void k_df_rows(DiffArgs a, DfWork w, u32 nrows)
{
    const u32 side = blockIdx.y, t = blockIdx.x * 256u + threadIdx.x;
    if (t >= nrows) return;
    const ChunkRows& c = w.c[side];
    const DfPieceSide& ps = w.ps[side];
    const DiffSideArgs& sa = a.s[side];
    c.tag[t] = kNone;
    chunk_row_clear(c, t, 0);
    const u32 np = 4u * a.nreq;
    if (t >= ps.rplace[np]) return;
    const u32 p = owner_of(static_cast<const u64*>(ps.rplace), np, t), r = p >> 2;
    if (!rows_fit(a, w, r) || !scratch_fits(a, w, r)) return;
    const u32 b = sa.req_stream[r];                                     // (< ns: the request was planned)
    const u64 i = ps.row0[p] + (t - ps.rplace[p]);
    IxPlan k{};                                                         // the run as the window the row must lie in
    k.f1 = sa.x.first[b + 1] < sa.x.nentries ? sa.x.first[b + 1] : sa.x.nentries;
    k.total = sa.x.total[b];
    if (i >= k.f1 || ps.row0[p] >= k.f1) return;
    k.lo = sa.x.start[ps.row0[p]];
    k.hi = k.lo + ps.bytes[p];
    Hop h{};
    if (k.hi < k.lo || !ix_row_check(sa.x, sa.in + sa.in_off[b], sa.in_len[b], k, i, true, &h) || h.dec == 0) return;
    c.tag[t] = r;
    chunk_row_set(c, t, h, sa.in_off[b] + sa.x.pos[i], run_place(a, w, side, p) + (sa.x.start[i] - k.lo));
}

// the failing decoded rows of each side, keyed by where their headers are: the first in stream order wins
__global__ __launch_bounds__(256) void k_df_fail(DfWork w, u32 nrows)
{
    const u32 side = blockIdx.y, t = blockIdx.x * 256u + threadIdx.x;
    if (t >= nrows) return;
    const ChunkRows& c = w.c[side];
    const u32 r = c.tag[t];
    if (r == kNone || c.status[t] == SNP_OK) return;
    atomic_min64(w.fail[side] + r, fail_key(c.body_off[t], c.status[t]));
}

// Workgroups stride over (piece, slice); a slice takes every `slices`-th block of kCompareBlock bytes of the piece, counted in the direction,
// and stops once a mismatch before its block is known.  Each lane compares 16 bytes (the last ones of a piece byte by byte).
__global__ __launch_bounds__(256) void k_df_compare(DiffArgs a, DfWork w, u32 slices, u64* __restrict__ result)
{
    const u64 items = 4ull * a.nreq * slices;
    if (blockIdx.x == 0 && threadIdx.x == 0) result[2] = w.ps[0].place[4ull * a.nreq] + w.ps[1].place[4ull * a.nreq];
    for (u64 item = blockIdx.x; item < items; item += gridDim.x) {
        const u64 p = item / slices;
        const u32 slice = static_cast<u32>(item % slices), r = static_cast<u32>(p >> 2), dir = static_cast<u32>(p >> 1) & 1u;
        const u64 len = w.len[p];
        if (len == 0 || !rows_fit(a, w, r) || !scratch_fits(a, w, r)) continue;
        const u64 q = w.src[p];
        const u8* const pa = w.scratch + run_place(a, w, 0, q) + w.ps[0].off[q];
        const u8* const pb = w.scratch + run_place(a, w, 1, q) + w.ps[1].off[q];
        u64* const mis = w.mis + p;
        for (u64 blk = slice; blk * kCompareBlock < len; blk += slices) {
            const u64 k0 = blk * kCompareBlock + threadIdx.x * 16u;     // the lane's first byte, counted in the direction
            if (__hip_atomic_load(mis, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < blk * kCompareBlock) break;
            u64 found = kDfNone;
            if (k0 < len) {
                const u64 m = len - k0 < 16 ? len - k0 : 16;            // bytes [k0, k0 + m) in the direction = [f, f + m) in stream order
                const u64 f = dir ? len - k0 - m : k0;
                if (m == 16) {
                    const u32 d = first_diff16(*reinterpret_cast<const snp_u128_unaligned*>(pa + f), *reinterpret_cast<const snp_u128_unaligned*>(pb + f), dir);
                    if (d < 16) found = k0 + d;
                } else {
                    for (u64 j = 0; j < m && found == kDfNone; ++j) {
                        const u64 at = dir ? f + m - 1 - j : f + j;
                        if (pa[at] != pb[at]) found = k0 + j;
                    }
                }
            }
            const u64 any = ballot64(found != kDfNone);
            if (any && lane_id() == static_cast<u32>(__builtin_ctzll(any))) atomic_min64(mis, found);   // (lanes are in the direction's order)
        }
    }
}

// A side's verdict: what its plan refused, else a row that failed its check, else the first failing decoded row, else the stream's tail.
__device__ __forceinline__ i32 side_verdict(u32 plan, bool bad, u64 fail, i32 tail)
{
    const i32 s = static_cast<i32>(static_cast<int8_t>(plan & 0xffu));
    if (s != SNP_OK) return s;
    if (bad) return SNP_ERR_BAD_ARG;
    return window_verdict(SNP_OK, fail, SNP_OK, tail, false);
}

__global__ __launch_bounds__(256) void k_df_verdict(DiffArgs a, DfWork w, u64* __restrict__ len_a, u64* __restrict__ len_b, u64* __restrict__ prefix,
                                                   u64* __restrict__ suffix, i32* __restrict__ status, u64* __restrict__ result)
{
    const u32 r = blockIdx.x * 256u + threadIdx.x;
    u64 ok_len = 0, ok = 0;
    if (r < a.nreq) {
        i32 s = SNP_ERR_OUTPUT_TOO_SMALL;
        u64 la = 0, lb = 0, pre = 0, suf = 0;
        if (rows_fit(a, w, r) && scratch_fits(a, w, r)) {
            const u32 flags = w.flags[r];
            const u32 plan_a = flags >> kPlanShiftA, plan_b = flags >> kPlanShiftB;
            s = side_verdict(plan_a, flags & kBadA, w.fail[0][r], (plan_a & 0xffu) == SNP_OK ? a.s[0].x.tail[a.s[0].req_stream[r]] : 0);
            if (s == SNP_OK) s = side_verdict(plan_b, flags & kBadB, w.fail[1][r], (plan_b & 0xffu) == SNP_OK ? a.s[1].x.tail[a.s[1].req_stream[r]] : 0);
            if (s == SNP_OK) {
                la = w.len_a[r];
                lb = w.len_b[r];
                const u64 n = la < lb ? la : lb, p = 4ull * r;
                if (a.flags & kDiffPrefix) pre = df_answer(w.t0[p + 1], w.len[p + 1], w.mis[p], w.mis[p + 1]);
                if (a.flags & kDiffSuffix) suf = df_answer(w.t0[p + 3], w.len[p + 3], w.mis[p + 2], w.mis[p + 3]);
                if ((a.flags & kDiffPrefix) && suf > n - pre) suf = n - pre;
                ok_len = n;
                ok = 1;
            }
        }
        status[r] = s;
        len_a[r] = la;
        len_b[r] = lb;
        prefix[r] = pre;
        suffix[r] = suf;
    }
    ok_len = wave_sum(ok_len);
    ok = wave_sum(ok);
    if ((threadIdx.x & 63u) == 0 && ok) {
        atomic_add64(result + 3, ok);
        if (ok_len) atomic_add64(result + 1, ok_len);
    }
}

// workspace: per request a few words; per piece (4 per request) and side its rows, bytes and places; the tile sums of the scans; one word per
// owned row and direction; per side a chunk table of min(2 x max_rows, scratch_cap) rows; then scratch_cap bytes of scratch
// (a row may serve both directions; and every row of a run is charged a byte of scratch_cap, so no more rows than that are ever in use)
u32 table_rows(u64 max_rows, u64 scratch_cap) { return static_cast<u32>(std::min<u64>(2 * max_rows, scratch_cap)); }
DfWork diff_work_layout(void* base, u32 nreq, u64 max_rows, u64 scratch_cap)
{
    DfWork k{};
    if (nreq == 0) return k;
    const u64 nr = nreq, np = 4 * nr;
    WorkCarver c(base);
    k.rfirst = c.take<u64>(nr + 1);
    k.part = c.take<u64>(scan_tiles_of(np));
    k.nrows = c.take<u64>(nr);
    k.len_a = c.take<u64>(nr);
    k.len_b = c.take<u64>(nr);
    k.fail[0] = c.take<u64>(nr);
    k.fail[1] = c.take<u64>(nr);
    k.flags = c.take<u32>(nr);
    for (u32 side = 0; side < 2; ++side) {
        DfPieceSide& p = k.ps[side];
        p.row0 = c.take<u64>(np);
        p.nrows = c.take<u64>(np);
        p.bytes = c.take<u64>(np);
        p.off = c.take<u64>(np);
        p.charge = c.take<u64>(np);
        p.place = c.take<u64>(np + 1);
        p.rplace = c.take<u64>(np + 1);
    }
    k.t0 = c.take<u64>(np);
    k.len = c.take<u64>(np);
    k.mis = c.take<u64>(np);
    k.src = c.take<u32>(np);
    k.g = c.take<u32>(2 * max_rows);
    k.c[0] = carve_chunk_rows(c, table_rows(max_rows, scratch_cap));
    k.c[1] = carve_chunk_rows(c, table_rows(max_rows, scratch_cap));
    k.scratch = c.take<u8>(scratch_cap);
    k.bytes = c.bytes();
    return k;
}

constexpr u64 kMaxRows = 0x7fffffffull;         // two table rows per owned row must be a row count

}  // namespace

extern "C" {

uint64_t snp_frame_diff_indexed_workspace(uint32_t nreq, uint64_t max_rows, uint64_t scratch_cap)
{
    if (nreq > 0x3fffffffu || max_rows > kMaxRows) return 0;
    return diff_work_layout(nullptr, nreq, max_rows, scratch_cap).bytes;
}

snp_status snp_frame_diff_indexed_batch(snp_ctx* c, const uint8_t* in_a, const uint64_t* in_off_a, const uint64_t* in_len_a, uint32_t nstreams_a,
                                        const uint64_t* idx_first_a, const uint64_t* idx_start_a, const uint64_t* idx_pos_a,
                                        const uint64_t* idx_total_a, const int32_t* idx_tail_a, uint64_t nentries_a, const uint8_t* in_b,
                                        const uint64_t* in_off_b, const uint64_t* in_len_b, uint32_t nstreams_b, const uint64_t* idx_first_b,
                                        const uint64_t* idx_start_b, const uint64_t* idx_pos_b, const uint64_t* idx_total_b,
                                        const int32_t* idx_tail_b, uint64_t nentries_b, const uint32_t* req_stream_a, const uint64_t* req_off_a,
                                        const uint64_t* req_len_a, const uint32_t* req_stream_b, const uint64_t* req_off_b,
                                        const uint64_t* req_len_b, uint32_t nreq, uint32_t flags, uint64_t max_rows, uint64_t scratch_cap,
                                        uint64_t* len_a, uint64_t* len_b, uint64_t* prefix, uint64_t* suffix, int32_t* status, void* d_work,
                                        uint64_t* d_result)
{
    if (!c || !d_result || nreq > 0x3fffffffu || max_rows > kMaxRows || !(flags & (kDiffPrefix | kDiffSuffix)) ||
        (flags & ~(kDiffPrefix | kDiffSuffix | kDiffExact)) ||
        (nreq && (!req_stream_a || !req_off_a || !req_len_a || !req_stream_b || !req_off_b || !req_len_b || !len_a || !len_b || !prefix || !suffix ||
                  !status || !d_work)) ||
        (nreq && nstreams_a && (!in_a || !in_off_a || !in_len_a || !idx_first_a || !idx_total_a || !idx_tail_a)) ||
        (nreq && nstreams_a && nentries_a && (!idx_start_a || !idx_pos_a)) ||
        (nreq && nstreams_b && (!in_b || !in_off_b || !in_len_b || !idx_first_b || !idx_total_b || !idx_tail_b)) ||
        (nreq && nstreams_b && nentries_b && (!idx_start_b || !idx_pos_b)))
        return SNP_ERR_BAD_ARG;
    DevGuard dg(c);
    if (!dg.ok) return SNP_ERR_DEVICE;
    hipStream_t s = c->stream;
    if (nreq == 0)
        return c->check(snp_zero_words_async(reinterpret_cast<u32*>(d_result), 2 * 4, s), "frame diff result") ? SNP_OK : SNP_ERR_DEVICE;
    const DfWork w = diff_work_layout(d_work, nreq, max_rows, scratch_cap);
    const u32 P = 4 * nreq, T = table_rows(max_rows, scratch_cap), groups = (nreq + 255u) / 256u;
    DiffArgs a{};
    a.s[0] = DiffSideArgs{in_a, in_off_a, in_len_a, nstreams_a, FrameIndex{idx_first_a, idx_start_a, idx_pos_a, idx_total_a, idx_tail_a, nentries_a},
                          req_stream_a, req_off_a, req_len_a};
    a.s[1] = DiffSideArgs{in_b, in_off_b, in_len_b, nstreams_b, FrameIndex{idx_first_b, idx_start_b, idx_pos_b, idx_total_b, idx_tail_b, nentries_b},
                          req_stream_b, req_off_b, req_len_b};
    a.nreq = nreq;
    a.flags = flags;
    a.max_rows = max_rows;
    a.scratch_cap = scratch_cap;
    hipLaunchKernelGGL(k_df_plan, dim3(groups), dim3(256), 0, s, a, w);
    // each request's place in the table of XORs (d_result[0] = rows needed, [1] = 0)
    bool ok = c->check(hipGetLastError(), "frame diff plan") &&
              c->check(launch_scan(ScanWords{w.nrows}, nreq, w.part, w.rfirst, d_result, s), "frame diff row scan");
    if (ok) {
        const u32 ndir = (flags & kDiffPrefix) && (flags & kDiffSuffix) ? 2u : 1u, dir0 = flags & kDiffPrefix ? 0u : 1u;
        const u64 items = static_cast<u64>(nreq) * ndir;
        const u32 wgs = static_cast<u32>((std::min<u64>(items, 8ull * c->persistent_waves()) + 3) / 4);
        hipLaunchKernelGGL(k_df_cuts, dim3(wgs), dim3(256), 0, s, a, w, ndir, dir0, wgs * 4u);
        hipLaunchKernelGGL(k_df_final, dim3(groups), dim3(256), 0, s, a, w, d_result);
        ok = c->check(hipGetLastError(), "frame diff cuts");
    }
    // every run's place in scratch and every piece's rows in its side's chunk table
    for (u32 side = 0; ok && side < 2; ++side)
        ok = c->check(launch_scan(ScanWords{w.ps[side].charge}, P, w.part, w.ps[side].place, nullptr, s), "frame diff byte scan") &&
             c->check(launch_scan(ScanWords{w.ps[side].nrows}, P, w.part, w.ps[side].rplace, nullptr, s), "frame diff piece row scan");
    if (ok && T) {
        hipLaunchKernelGGL(k_df_rows, dim3((T + 255u) / 256u, 2), dim3(256), 0, s, a, w, T);
        ok = c->check(hipGetLastError(), "frame diff rows") && c->decode_chunks(in_a, w.c[0], T, w.scratch) && c->decode_chunks(in_b, w.c[1], T, w.scratch);
        if (ok) hipLaunchKernelGGL(k_df_fail, dim3((T + 255u) / 256u, 2), dim3(256), 0, s, w, T);
    }
    if (ok) {
        const u32 slices = static_cast<u32>(std::min<u64>(64, std::max<u64>(1, 4096 / P)));
        const u32 wgs = static_cast<u32>(std::min<u64>(static_cast<u64>(P) * slices, 1u << 20));
        hipLaunchKernelGGL(k_df_compare, dim3(wgs), dim3(256), 0, s, a, w, slices, d_result);
        hipLaunchKernelGGL(k_df_verdict, dim3(groups), dim3(256), 0, s, a, w, len_a, len_b, prefix, suffix, status, d_result);
        ok = c->check(hipGetLastError(), "frame diff verdict");
    }
    return ok ? SNP_OK : SNP_ERR_DEVICE;
}

}  // extern "C"

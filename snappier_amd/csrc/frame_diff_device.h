// frame_diff_device.h -- the planning and the arithmetic of the batch diff (snp_frame_diff_indexed_batch, frame_diff.hip): the longest common
// prefix and suffix of two windows of what seekable framed streams decode to, found from the CRCs the chunk headers carry wherever both
// streams have a chunk boundary at the same decoded offset.  __host__ __device__ throughout, so that the same code runs on the CPU under
// sanitizers (tests/abi/frame_diff_plan_check.hip) over indexes filled with anything at all.  The clip, the searches and the row check are the
// indexed read's (frame_index_device.h), the CRC arithmetic is the digest's (frame_digest_device.h); nothing of them is restated.  DESIGN.md 4.23.
//
// One DIRECTION of one request works in the coordinate t = distance from the windows' starts (prefix, dir 0) or from their ends (suffix,
// dir 1); n = min(len_a, len_b); rows are numbered in direction order (ordinal o: row r0 + o, or r1 - 1 - o).  A row wholly inside [0, n]
// adds the term shift(unmask(crc), bytes between its far edge and the common point K) -- K = n for the prefix, the window's end for the
// suffix -- so that XORs of terms over the same span of t compare equal on both sides iff the spans' CRCs do (x is a unit mod P).
// A COMMON CUT is a t at which both sides have a row boundary.  With G_x(t) the XOR of side x's terms before t, D(t) = G_a(t) ^ G_b(t): the
// first common cut whose D differs from the first cut's ends the first span whose CRCs differ.
#pragma once
#include "frame_digest_device.h"

namespace {

constexpr u32 kDiffPrefix = 1u, kDiffSuffix = 2u, kDiffExact = 4u;
constexpr u64 kDfNone = ~0ull;              // no mismatch found

// one side of one request: its stream's bytes and its plan
struct DfSide {
    const u8* p;        // the stream's first byte
    u64 n;              // the stream's bytes
    u64 base;           // in_off of the stream
    IxPlan k;
    __host__ __device__ u64 rows() const { return k.r1 - k.r0; }
    __host__ __device__ u64 len() const { return k.hi - k.lo; }
};
__host__ __device__ inline DfSide df_side(const FrameIndex& x, const u8* __restrict__ in, const u64* __restrict__ in_off, const u64* __restrict__ in_len,
                                          u32 nstreams, u32 b, u64 req_off, u64 req_len)
{
    DfSide s{};
    s.k = ix_plan(x, nstreams, b, req_off, req_len, ~0ull);
    if (s.k.status == SNP_OK) {
        s.base = in_off[b];
        s.p = in + s.base;
        s.n = in_len[b];
    }
    return s;
}

// Row of ordinal o in direction dir: ok = it passes the read's check (an edge row as an edge, any other as an interior row); [tlo, thi) = where
// it lies in t; full = wholly inside [0, n]; term = what it adds (0 unless full and not empty; computed only when `terms`).
struct DfRow {
    bool ok, full;
    u64 tlo, thi;
    u32 term;
};
__host__ __device__ inline DfRow df_row(const FrameIndex& x, const DfSide& s, u32 dir, u64 n, u64 o, bool terms)
{
    DfRow w{};
    const u64 i = dir ? s.k.r1 - 1 - o : s.k.r0 + o;
    const bool edge = (s.k.head && i == s.k.r0) || (s.k.last && i == s.k.r1 - 1);
    Hop h{};
    w.ok = i < s.k.f1 && ix_row_check(x, s.p, s.n, s.k, i, !edge, &h);
    if (!w.ok) return w;
    const u64 st = x.start[i], en = ix_row_end(x, s.k.f1, s.k.total, i);
    w.tlo = dir ? s.k.hi - en : st - s.k.lo;
    w.thi = dir ? s.k.hi - st : en - s.k.lo;
    w.full = st >= s.k.lo && en <= s.k.hi && w.thi <= n;
    if (terms && w.full && h.dec) w.term = crc_shift(crc_unmask(h.crc), dir ? w.tlo : n - w.thi);
    return w;
}

// Has side s a row boundary at t?  *ord = its rows, in direction order, that lie wholly before it.
__host__ __device__ inline bool df_cut(const FrameIndex& x, const DfSide& s, u32 dir, u64 t, u64* ord)
{
    *ord = 0;
    if (t > s.len() || s.k.r0 >= s.k.r1) return false;
    const u64 T = dir ? s.k.hi - t : s.k.lo + t;
    // j = the first owned row that starts at or after T.  Rows of one size are the rule: the row that size names is tried first, and is the
    // answer if it and the row before it bracket T (owned rows that pass their checks start in order, so the answer is the search's).
    u64 j = s.k.r1;
    bool known = false;
    if (s.k.r1 - s.k.r0 >= 2) {
        const u64 s0 = x.start[s.k.r0], s1 = x.start[s.k.r0 + 1];
        if (s1 > s0 && T >= s0) {
            const u64 q = (T - s0 + (s1 - s0) - 1) / (s1 - s0);
            j = q < s.k.r1 - s.k.r0 ? s.k.r0 + q : s.k.r1;
            known = (j == s.k.r1 || x.start[j] >= T) && (j == s.k.r0 || x.start[j - 1] < T);
        }
    }
    if (!known) j = ix_first_where(s.k.r0, s.k.r1, [&](u64 i) { return x.start[i] >= T; });
    *ord = dir ? s.k.r1 - j : j - s.k.r0;
    return j < s.k.r1 ? x.start[j] == T : ix_row_end(x, s.k.f1, s.k.total, s.k.r1 - 1) == T;
}

// the rows of side s, in direction order, that hold a byte of [0, n)
__host__ __device__ inline u64 df_need_rows(const FrameIndex& x, const DfSide& s, u32 dir, u64 n)
{
    if (n == 0 || s.k.r0 >= s.k.r1) return 0;
    if (!dir) return ix_first_where(s.k.r0, s.k.r1, [&](u64 i) { return x.start[i] >= s.k.lo + n; }) - s.k.r0;
    return s.k.r1 - ix_first_where(s.k.r0, s.k.r1, [&](u64 i) { return ix_row_end(x, s.k.f1, s.k.total, i) > s.k.hi - n; });
}

// a common cut: t, and the rows of each side before it
struct DfCut {
    u64 t, ia, ib;
};
// what the scan of one direction finds
struct DfScan {
    bool bad_a, bad_b;      // a row of that side failed its check
    bool have0, diff;       // there is a common cut; a span between two common cuts has differing CRCs
    DfCut c0, prev, last, end;   // the first cut; diff: the cuts around the first differing span; else last = the last cut
    u32 d0;                 // D at the first cut
};
// one common cut more, in order of t
__host__ __device__ __forceinline__ void df_scan_cut(DfScan& s, const DfCut& c, u32 d)
{
    if (!s.have0) { s.have0 = true; s.c0 = s.last = c; s.d0 = d; }
    else if (d != s.d0) { s.diff = true; s.prev = s.last; s.end = c; }
    else s.last = c;
}

// The scan, one row after the other (the wavefront of frame_diff.hip does the same 64 rows at a time).  gb: rows_b + 1 words, side B's
// exclusive XORs.  cuts = false (SNP_DIFF_EXACT, or n == 0): the rows are only checked.
__host__ __device__ inline DfScan df_scan_seq(const FrameIndex& xa, const DfSide& a, const FrameIndex& xb, const DfSide& b, u32 dir, u64 n, bool cuts,
                                              u32* gb)
{
    DfScan s{};
    u32 acc = 0;
    for (u64 o = 0; o < b.rows(); ++o) {
        const DfRow w = df_row(xb, b, dir, n, o, cuts);
        s.bad_b |= !w.ok;
        if (cuts) gb[o] = acc;
        acc ^= w.term;
    }
    u64 oa, ob;
    if (cuts) {
        gb[b.rows()] = acc;
        if (df_cut(xa, a, dir, 0, &oa) && df_cut(xb, b, dir, 0, &ob)) df_scan_cut(s, DfCut{0, 0, 0}, 0);
    }
    acc = 0;
    for (u64 o = 0; o < a.rows(); ++o) {
        const DfRow w = df_row(xa, a, dir, n, o, cuts);
        s.bad_a |= !w.ok;
        acc ^= w.term;
        if (cuts && !s.diff && w.ok && w.full && df_cut(xb, b, dir, w.thi, &ob)) df_scan_cut(s, DfCut{w.thi, o + 1, ob}, acc ^ gb[ob]);
    }
    return s;
}

// The at most two pieces of [0, n) a direction decodes and compares byte for byte: rows [a0, a1) of side A and [b0, b1) of side B (ordinals),
// the bytes [t0, t0 + len) of them.  piece 0: the bytes before the first common cut -- all of [0, n) when there is none, or with exact;
// piece 1: the first span whose CRCs differ, else the bytes after the last cut.  A piece of no bytes has no rows.
struct DfPiece {
    u64 a0, a1, b0, b1, t0, len;
};
__host__ __device__ inline void df_pieces(const DfScan& s, u64 need_a, u64 need_b, u64 n, bool exact, DfPiece out[2])
{
    out[0] = out[1] = DfPiece{0, 0, 0, 0, n, 0};
    if (n == 0) return;
    if (exact || !s.have0) {
        out[0] = DfPiece{0, need_a, 0, need_b, 0, n};
        return;
    }
    if (s.c0.t) out[0] = DfPiece{0, s.c0.ia, 0, s.c0.ib, 0, s.c0.t};
    else out[0].t0 = 0;
    if (s.diff) out[1] = DfPiece{s.prev.ia, s.end.ia, s.prev.ib, s.end.ib, s.prev.t, s.end.t - s.prev.t};
    else if (s.last.t < n)
        out[1] = DfPiece{s.last.ia, need_a > s.last.ia ? need_a : s.last.ia, s.last.ib, need_b > s.last.ib ? need_b : s.last.ib, s.last.t, n - s.last.t};
}

// A piece on one side: its rows [*row0, *row0 + *nrows) of the index, decoded consecutively they are one run of *bytes bytes whose byte *off
// is the first byte the piece compares (in stream order, in both directions).  false: the index contradicts itself (nothing is decoded).
__host__ __device__ inline bool df_piece_side(const FrameIndex& x, const DfSide& s, u32 dir, u64 o0, u64 o1, u64 t0, u64 len, u64* row0, u64* nrows,
                                              u64* bytes, u64* off)
{
    *row0 = *nrows = *bytes = *off = 0;
    if (o1 <= o0 || len == 0) return len == 0;
    if (o1 > s.rows()) return false;
    const u64 i0 = dir ? s.k.r1 - o1 : s.k.r0 + o0, i1 = i0 + (o1 - o0);
    const u64 s0 = x.start[i0], e1 = ix_row_end(x, s.k.f1, s.k.total, i1 - 1);
    const u64 from = dir ? s.k.hi - t0 - len : s.k.lo + t0;
    if (e1 < s0 || from < s0 || from - s0 > e1 - s0 || len > e1 - s0 - (from - s0)) return false;
    *row0 = i0;
    *nrows = i1 - i0;
    *bytes = e1 - s0;
    *off = from - s0;
    return true;
}

// A direction's answer from its pieces' first mismatches (kDfNone: the piece compared equal; counted in t from the piece's t0)
__host__ __device__ __forceinline__ u64 df_answer(u64 t1, u64 len1, u64 mis0, u64 mis1)
{
    return mis0 != kDfNone ? mis0 : t1 + (mis1 != kDfNone ? mis1 : len1);
}

}  // namespace

// frame_verify_device.h -- the rules of the batch VERIFY (snp_frame_verify_indexed_batch) and of the REPAIR PLANNER (snp_frame_repair_plan_batch),
// frame_verify.hip, stated once: the rounds and slots of the bounded scratch, the judgement of ONE row of a stream over a chunk index that is
// UNTRUSTED input before anything is decoded, what the rows of a stream add up to, and -- the planner -- what admits a pair, what a row of
// the index stands for in the plan and where a segment begins.  On top of frame_dedup_device.h (the verdict of a stream before its rows are
// looked at, dd_stream) and frame_compose_device.h, whose check of a kept row (cc_add) is the check of every row here.  __host__ __device__
// throughout, so that the same code runs on the CPU under sanitizers (tests/abi/frame_verify_plan_check.hip).  DESIGN.md 4.29.
//
// Rows are numbered over the whole index ("global row").  A row is LOOKED AT when its stream's verdict is SNP_OK; it is CHECKED when it
// passes the row check; a checked row is decoded and CRC-verified in its round unless its length exceeds slot_bytes or there is no round.
#pragma once
#include "frame_dedup_device.h"

namespace {

constexpr u64 kVfNone = ~0ull;                      // SNP_VERIFY_NONE: first_bad of a stream with no bad row
constexpr i32 kVfSkipped = -1;                      // SNP_VERIFY_SKIPPED: row_status of a row that was not looked at
constexpr u32 kVfMaxSlot = SNP_BLOCK_SIZE;          // the largest slot_bytes
constexpr u64 kVfMaxRows = 0x7fffffffull;           // rows a call takes
constexpr u32 kVfNoIdent = 1u;                      // flags bit 0: the first 10 bytes are not the stream identifier

// ---- rounds and slots -------------------------------------------------------------------------------------------------------------------------------
// Row i is decoded in round i / per_round into slot i % per_round of the scratch.  per_round is capped at the rows there are, so the scratch a
// call touches is per_round * stride bytes whatever scratch_cap is.  per_round == 0: the sizing call, nothing is decoded.
struct VfRounds {
    u64 stride, per_round, rounds;
};
__host__ __device__ inline VfRounds vf_rounds(u32 slot_bytes, u64 scratch_cap, u64 nentries)
{
    VfRounds r{};
    r.stride = (static_cast<u64>(slot_bytes) + 15) / 16 * 16;
    const u64 fit = r.stride ? scratch_cap / r.stride : 0;
    r.per_round = fit < nentries ? fit : nentries;
    r.rounds = r.per_round ? nentries / r.per_round + (nentries % r.per_round ? 1 : 0) : 0;
    return r;
}
__host__ __device__ __forceinline__ u64 vf_slot_off(const VfRounds& r, u64 i) { return i % r.per_round * r.stride; }

// ---- one row ------------------------------------------------------------------------------------------------------------------------------------------
// Row i of a stream that passed (k: dd_stream), before anything is decoded: SNP_ERR_BAD_ARG when it fails the compose call's check of a kept
// row, SNP_ERR_OUTPUT_TOO_SMALL when it is checked and cannot be decoded in this call, SNP_OK when its round will tell.  len: end - start by
// the index (0 when the row ends below its start): what the row is counted as.  hop_at(pos) -> the Hop of the header at pos < n.
struct VfRow {
    i32 status;
    bool checked;
    u64 len;
    Hop h;
};
template <class HopAt>
__host__ __device__ inline VfRow vf_row(const FrameIndex& x, const CcSeg& k, u64 i, u32 slot_bytes, const VfRounds& rounds, HopAt hop_at)
{
    VfRow r{};
    const u64 s = x.start[i], e = ix_row_end(x, k.f1, k.total, i);
    r.len = e >= s ? e - s : 0;
    CcAcc acc{};
    cc_add(&acc, x, k, i, [&](u64 pos) { r.h = hop_at(pos); return r.h; });
    r.checked = !acc.bad;
    r.status = acc.bad ? SNP_ERR_BAD_ARG : (r.h.dec > slot_bytes || rounds.per_round == 0) ? SNP_ERR_OUTPUT_TOO_SMALL : SNP_OK;
    return r;
}

// ---- one stream -----------------------------------------------------------------------------------------------------------------------------------------
// What the rows of a stream add up to, from their final row_status.  Sums, a minimum and a maximum: the order in which rows are joined does
// not matter.  (Sums of lengths wrap at 2^64, as the lengths of an unsound index may.)
struct VfAcc {
    u64 looked, bad, first, bad_bytes, ok_bytes, longest, unverified;
};
__host__ __device__ __forceinline__ VfAcc vf_none() { return VfAcc{0, 0, kVfNone, 0, 0, 0, 0}; }
__host__ __device__ __forceinline__ void vf_join(VfAcc* a, const VfAcc& b)
{
    a->looked += b.looked;
    a->bad += b.bad;
    a->first = b.first < a->first ? b.first : a->first;
    a->bad_bytes += b.bad_bytes;
    a->ok_bytes += b.ok_bytes;
    a->longest = b.longest > a->longest ? b.longest : a->longest;
    a->unverified += b.unverified;
}
// row i with its final status; checked and len as vf_row gave them
__host__ __device__ __forceinline__ void vf_add(VfAcc* a, u64 i, i32 status, bool checked, u64 len)
{
    a->looked += 1;
    if (checked && len > a->longest) a->longest = len;
    if (status == SNP_OK) { a->ok_bytes += len; return; }
    a->bad += 1;
    a->first = i < a->first ? i : a->first;
    a->bad_bytes += len;
    if (checked && status == SNP_ERR_OUTPUT_TOO_SMALL) a->unverified += 1;
}

// ---- the planner ------------------------------------------------------------------------------------------------------------------------------------------
// Pair j = (stream s, replica t): SNP_OK, or SNP_ERR_BAD_ARG for a pair out of range, a stream whose fr_begin fails, a replica whose tail is
// not SNP_OK and a replica of another length.
__host__ __device__ inline i32 rp_begin(const FrameIndex& x, u32 nstreams, const u64* __restrict__ rep_total, const i32* __restrict__ rep_tail,
                                        u32 nrep, u32 s, u32 t)
{
    if (s >= nstreams || t >= nrep) return SNP_ERR_BAD_ARG;
    if (fr_begin(x, s) != SNP_OK || rep_tail[t] != SNP_OK) return SNP_ERR_BAD_ARG;
    return rep_total[t] == x.total[s] ? SNP_OK : SNP_ERR_BAD_ARG;
}
// Row i of stream s in the plan: it takes part when it holds at least one byte; it is taken from the stream itself when its row_status is
// SNP_OK, else from the replica.
struct RpRow {
    bool live, good;
    u64 start, len;
};
__host__ __device__ __forceinline__ RpRow rp_row(const FrameIndex& x, const i32* __restrict__ row_status, u64 f1, u64 total, u64 i)
{
    RpRow r{};
    r.start = x.start[i];
    const u64 e = ix_row_end(x, f1, total, i);
    r.len = e >= r.start ? e - r.start : 0;
    r.live = r.len != 0;
    r.good = row_status[i] == SNP_OK;
    return r;
}
// A row that takes part begins a segment unless the row that takes part before it in its stream comes from the same side.
__host__ __device__ __forceinline__ bool rp_begins(bool has_prev, bool prev_good, bool good) { return !has_prev || prev_good != good; }
// the source of a segment: stream s is source s, replica t is source nstreams + t
__host__ __device__ __forceinline__ u32 rp_source(u32 nstreams, u32 s, u32 t, bool good) { return good ? s : nstreams + t; }

// The whole plan of a pair by one thread (the kernel walks the rows in tiles of a workgroup and joins the same calls by scans): seg(src, off,
// len) for every segment in order.  A segment runs from its first row's start to the start of the row that begins the next one, the last to
// the stream's total.  -> what the pair counts: segments, bytes taken from the replica, bytes kept.
struct RpCount {
    u64 segs, taken, kept;
};
template <class Seg>
__host__ __device__ inline RpCount rp_plan(const FrameIndex& x, const i32* __restrict__ row_status, u32 nstreams, u32 s, u32 t, Seg seg)
{
    RpCount c{};
    u64 f0, rows;
    fr_rows(x, s, &f0, &rows);
    const u64 f1 = f0 + rows, total = x.total[s];
    bool open = false, good = false;
    u64 off = 0;
    for (u64 i = f0; i < f1; ++i) {
        const RpRow r = rp_row(x, row_status, f1, total, i);
        if (!r.live) continue;
        if (rp_begins(open, good, r.good)) {
            if (open) seg(rp_source(nstreams, s, t, good), off, r.start - off);
            open = true;
            good = r.good;
            off = r.start;
            c.segs += 1;
        }
        if (r.good) c.kept += r.len;
        else c.taken += r.len;
    }
    if (open) seg(rp_source(nstreams, s, t, good), off, total - off);
    return c;
}

}  // namespace

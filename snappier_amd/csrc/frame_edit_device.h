// frame_edit_device.h -- what the indexed EDIT (snp_frame_edit_indexed_batch, frame_edit.hip) plans on top of the splice's plan of ONE edit
// (fs_plan, frame_splice_device.h: the rows an edit owns, its edges, its hole, the probes of the untrusted index -- called, not restated): the
// CSR list of a stream's edits, the LINK between two consecutive edits that own the same row, an edit's own verdict (the order of the edits, of
// their holes and of their rows; the running length), and the length of a group's region from sums that cannot wrap.  __host__ __device__
// throughout, so that the same code runs on the CPU under sanitizers (tests/abi/frame_edit_plan_check.hip).  DESIGN.md 4.25.
//
// A GROUP is a maximal run of linked edits.  It has ONE region R = H(first) || ins || G || ins || ... || ins || T(last), G the kept decoded bytes
// between two linked edits (they lie inside the shared row), and ONE hole [P0(first), P1(last)).
#pragma once
#include "frame_splice_device.h"

namespace {

// the edits of stream b: [e0, e1), inside nedits whatever ed_first holds; false: the list runs backwards
__host__ __device__ __forceinline__ bool fe_csr(const u64* __restrict__ ed_first, u64 nedits, u32 b, u64* e0, u64* e1)
{
    *e0 = ed_first[b] < nedits ? ed_first[b] : nedits;
    *e1 = ed_first[b + 1] < nedits ? ed_first[b + 1] : nedits;
    return *e1 >= *e0;
}
// an edit that does something: the others are passed over, and nothing of them is looked at
__host__ __device__ __forceinline__ bool fe_named(u64 del, u64 ins) { return (del | ins) != 0; }

// what the link and the verdict read of an edit: fs_plan's status and, when that is SNP_OK, its owned rows and its hole
struct FeEdit {
    i32 status;
    u64 lo, del;
    u64 r0, r1, p0, p1;
};
__host__ __device__ __forceinline__ FeEdit fe_edit(const FsPlan& k, u64 lo, u64 del) { return FeEdit{k.status, lo, del, k.r0, k.r1, k.p0, k.p1}; }

// p, then k, consecutive named edits of one stream: both passed, in order, both own rows, and the last owned row of p is the first owned row of
// k.  Then p keeps a tail of that row and k a head of it (fs_plan checked the same row against the same header for both), and the bytes
// between them, [hi_p, lo_k), are G.
__host__ __device__ __forceinline__ bool fe_linked(const FeEdit& p, const FeEdit& k)
{
    const u64 hi = p.lo + p.del;
    return p.status == SNP_OK && k.status == SNP_OK && hi >= p.lo && k.lo >= hi && p.r1 > p.r0 && k.r1 > k.r0 && p.r1 - 1 == k.r0;
}

// a sum of up to 2^32 u64 values kept as the sum of their low and of their high halves: neither wraps.  -> its low 64 bits; false: it needs more
__host__ __device__ __forceinline__ bool fe_wide(u64 sum_hi, u64 sum_lo, u64 plus, u64* v)
{
    const u64 t = sum_lo + plus, h = sum_hi + (t >> 32);                // (sum_lo, plus < 2^63)
    *v = (h << 32) | (t & 0xffffffffu);
    return h < (1ull << 32);
}

// The edit's own verdict.  p: the named edit before it in its stream (null: none).  ins_hi, ins_lo: the inserted bytes of the stream's edits up to
// and with this one (fe_wide); del_mod: their deleted bytes modulo 2^64 -- exact while the edits before were in order.
__host__ __device__ inline i32 fe_verdict(const FeEdit& k, const FeEdit* p, u64 total, u64 ins_hi, u64 ins_lo, u64 del_mod)
{
    if (k.status != SNP_OK) return k.status;
    if (p) {
        const u64 hi = p->lo + p->del;
        if (hi >= p->lo && k.lo < hi) return SNP_ERR_BAD_ARG;           // out of order with, or overlapping, its predecessor
        // two groups: P1(g) <= P0(g + 1), and the owned rows in order -- what a sound index gives
        if (p->status == SNP_OK && !fe_linked(*p, k) && (p->p1 > k.p0 || p->r1 > k.r0)) return SNP_ERR_BAD_ARG;
    }
    if (del_mod <= total) {                                             // the running length wraps
        u64 ins;
        if (!fe_wide(ins_hi, ins_lo, 0, &ins) || ins > ~0ull - (total - del_mod)) return SNP_ERR_BAD_ARG;
    }
    return SNP_OK;
}

// what a group asks of the two bounds: region = |R| (false: it does not fit 64 bits), edges = the decoded bytes of its distinct edge rows
__host__ __device__ __forceinline__ u64 fe_count_pieces(bool fits, u64 region, u32 cb)
{
    const u64 pieces = fits ? fc_chunks(region, cb) : kFsMaxPieces;
    return pieces < kFsMaxPieces ? pieces : kFsMaxPieces;
}
__host__ __device__ __forceinline__ u64 fe_count_stage(bool fits, u64 region, u64 edges)
{
    const u64 stage = edges + region;
    return fits && stage >= region && stage < kFsMaxStage ? stage : kFsMaxStage;
}

}  // namespace

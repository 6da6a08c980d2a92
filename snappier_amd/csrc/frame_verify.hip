// frame_verify.hip -- snp_frame_verify_indexed_batch and snp_frame_repair_plan_batch: which chunks of a batch of seekable framed streams are
// rotten, row by row, with nothing moved or rewritten and the decoded bytes held in a scratch of bounded size; and the compose recipes that
// take exactly the rotten rows from a replica.  The rules -- rounds and slots, the judgement of a row before it is decoded, what the rows of
// a stream add up to, what admits a pair, where a segment begins -- are frame_verify_device.h.  Built into libsnappier_hip_frame_verify.so
// (C-ABI: include/snappier_hip_frame_verify.h), linked against libsnappier_hip.so.  DESIGN.md 4.29.
//
// verify:  init      every row: SNP_VERIFY_SKIPPED, no length, an empty row of the chunk table
//          before    one workgroup: the largest clamped idx_first in front of every stream (frame_before_device.h)
//          check     a workgroup per stream: flags, dd_stream; a stream that passed: per row vf_row -> row_status (SNP_OK: its round will
//                    tell), its length, and for a row to decode its row of the chunk table with its slot in the scratch
//          rounds    host arithmetic: round q is rows [q * per_round, (q + 1) * per_round) of the table, a slice of it; snp_ctx::decode_chunks
//                    (decode + CRC verify) over the slice into the scratch, round after round on the stream
//          fold      one thread per row: a decoded row's status -> row_status
//          streams   a workgroup per stream: vf_add over its rows, joined (sums, a minimum, a maximum); status, nbad, first_bad, bad_bytes
//          result    one workgroup: the sums over the streams -> d_result
// plan:    count     a workgroup per pair: rp_begin; its rows in tiles of 256 -- the row that takes part before a row by ballots, the
//                    segment a row begins by a scan --: segments, bytes taken, bytes kept
//          scans     segments over the pairs -> admission in pair order (the sum only grows); the admitted pairs' segments -> seg_first
//          emit      a workgroup per admitted pair: the same walk; a row that begins a segment writes its source and offset and the end of
//                    the segment before it; then every segment's length
//          result    one workgroup: d_result
// No atomic is used.  Nothing here allocates, reads back or synchronises: both calls are capturable like the other _batch entry points.
#include "capi_internal.h"
#include "scan_tiles.h"
#include "frame_verify_device.h"
#include "frame_before_device.h"
#include "../../include/snappier_hip_frame_verify.h"

namespace {

static_assert(kVfNone == SNP_VERIFY_NONE, "SNP_VERIFY_NONE");
static_assert(kVfSkipped == SNP_VERIFY_SKIPPED, "SNP_VERIFY_SKIPPED");
static_assert(SNP_VERIFY_SKIPPED < SNP_OK, "SNP_VERIFY_SKIPPED lies outside snp_status");

inline u32 groups(u64 n) { return static_cast<u32>((n + 255) / 256); }

// the sum of v over the workgroup, in every thread.  All threads must call it.
__device__ __forceinline__ u64 block_sum(u64 v)
{
    u64 total;
    (void)wg_exclusive_scan(v, &total);
    return total;
}

// ---- verify ------------------------------------------------------------------------------------------------------------------------------------------
struct VfArgs {
    const u8* in;
    const u64 *in_off, *in_len;
    u32 ns;
    FrameIndex x;
    u32 slot_bytes;
    VfRounds rounds;
};
struct VfWork {
    // per stream
    u64* before;
    i32* verdict;
    u64 *looked, *ok_bytes, *longest, *unverified;
    // per row
    u64* len;
    u8* checked;
    ChunkRows rows;             // (no tag: a row's place in the table is its row in the index)
    u8* scratch;
    u64 total;
};

__global__ __launch_bounds__(256) void k_vf_init(u64 ne, VfWork w, i32* __restrict__ row_status)
{
    for (u64 i = static_cast<u64>(blockIdx.x) * 256u + threadIdx.x; i < ne; i += static_cast<u64>(gridDim.x) * 256u) {
        row_status[i] = kVfSkipped;
        w.len[i] = 0;
        w.checked[i] = 0;
        chunk_row_clear(w.rows, i, 0);
    }
}

// A workgroup per stream.  The stream steers the whole workgroup.
__global__ __launch_bounds__(256) void k_vf_check(VfArgs a, VfWork w, i32* __restrict__ row_status, u32* __restrict__ flags)
{
    const u32 b = blockIdx.x;
    const u8* const s = a.in + a.in_off[b];
    const CcSeg k = dd_stream(a.x, a.in_len, b, w.before[b]);
    if (threadIdx.x == 0) {
        w.verdict[b] = k.status;
        flags[b] = fr_ident(s, a.in_len[b]) ? 0u : kVfNoIdent;
    }
    if (k.status != SNP_OK) return;
    for (u64 i = k.r0 + threadIdx.x; i < k.r1; i += 256u) {
        const VfRow r = vf_row(a.x, k, i, a.slot_bytes, a.rounds, [&](u64 pos) { return frame_hop(s, k.n, pos); });
        row_status[i] = r.status;
        w.len[i] = r.len;
        w.checked[i] = r.checked ? 1 : 0;
        if (r.status == SNP_OK) chunk_row_set(w.rows, i, r.h, a.in_off[b] + a.x.pos[i], vf_slot_off(a.rounds, i));
    }
}

// One thread per row: a row that was decoded takes the status of its decode and CRC verify.
__global__ __launch_bounds__(256) void k_vf_fold(u64 ne, VfWork w, i32* __restrict__ row_status)
{
    const u64 i = static_cast<u64>(blockIdx.x) * 256u + threadIdx.x;
    if (i >= ne || !w.checked[i] || row_status[i] != SNP_OK) return;
    row_status[i] = w.rows.status[i];
}

// the join of what the threads of a workgroup hold; every thread gets it.  All threads must call it.
__device__ __forceinline__ VfAcc block_join(VfAcc v)
{
    __shared__ VfAcc s_acc[4];
    v.looked = wave_sum(v.looked);
    v.bad = wave_sum(v.bad);
    v.first = wave_min(v.first);
    v.bad_bytes = wave_sum(v.bad_bytes);
    v.ok_bytes = wave_sum(v.ok_bytes);
    v.longest = wave_max(v.longest);
    v.unverified = wave_sum(v.unverified);
    if ((threadIdx.x & 63u) == 0) s_acc[threadIdx.x >> 6] = v;
    __syncthreads();
    VfAcc all = vf_none();
    for (u32 q = 0; q < 4; ++q) vf_join(&all, s_acc[q]);
    __syncthreads();
    return all;
}

// A workgroup per stream: what its rows add up to.
__global__ __launch_bounds__(256) void k_vf_streams(VfArgs a, VfWork w, const i32* __restrict__ row_status, i32* __restrict__ status,
                                                   u64* __restrict__ nbad, u64* __restrict__ first_bad, u64* __restrict__ bad_bytes)
{
    const u32 b = blockIdx.x;
    const i32 verdict = w.verdict[b];
    VfAcc acc = vf_none();
    if (verdict == SNP_OK) {
        u64 f0, rows;
        fr_rows(a.x, b, &f0, &rows);
        for (u64 i = f0 + threadIdx.x; i < f0 + rows; i += 256u) vf_add(&acc, i, row_status[i], w.checked[i] != 0, w.len[i]);
    }
    acc = block_join(acc);
    if (threadIdx.x != 0) return;
    status[b] = verdict != SNP_OK ? verdict : acc.first != kVfNone ? row_status[acc.first] : SNP_OK;
    nbad[b] = acc.bad;
    first_bad[b] = acc.first;
    bad_bytes[b] = acc.bad_bytes;
    w.looked[b] = acc.looked;
    w.ok_bytes[b] = acc.ok_bytes;
    w.longest[b] = acc.longest;
    w.unverified[b] = acc.unverified;
}

// One workgroup: d_result, the join of what the streams hold.
__global__ __launch_bounds__(256) void k_vf_result(u32 ns, VfWork w, u64 rounds, const i32* __restrict__ status, const u64* __restrict__ nbad,
                                                  const u64* __restrict__ bad_bytes, u64* __restrict__ result)
{
    VfAcc acc = vf_none();
    u64 ok = 0;
    for (u32 b = threadIdx.x; b < ns; b += 256u) {
        vf_join(&acc, VfAcc{w.looked[b], nbad[b], kVfNone, bad_bytes[b], w.ok_bytes[b], w.longest[b], w.unverified[b]});
        ok += status[b] == SNP_OK ? 1 : 0;
    }
    acc = block_join(acc);
    ok = block_sum(ok);
    if (threadIdx.x != 0) return;
    result[0] = acc.looked;
    result[1] = acc.bad;
    result[2] = acc.ok_bytes;
    result[3] = ok;
    result[4] = acc.longest;
    result[5] = acc.unverified;
    result[6] = rounds;
    result[7] = acc.bad_bytes;
}

// workspace (every piece 256-byte aligned; nothing for arguments the call refuses or when there is no stream)
VfWork verify_layout(void* base, u32 ns, u64 ne, u32 slot_bytes, u64 scratch_cap)
{
    VfWork w{};
    if (ns == 0 || ns > 0x7fffffffu || ne > kVfMaxRows || slot_bytes == 0 || slot_bytes > kVfMaxSlot) return w;
    const VfRounds r = vf_rounds(slot_bytes, scratch_cap, ne);
    WorkCarver k(base);
    w.before = k.take<u64>(ns);
    w.verdict = k.take<i32>(ns);
    for (u64** p : {&w.looked, &w.ok_bytes, &w.longest, &w.unverified}) *p = k.take<u64>(ns);
    w.len = k.take<u64>(ne);
    w.checked = k.take<u8>(ne);
    w.rows.body_off = k.take<u64>(ne);
    w.rows.out_off = k.take<u64>(ne);
    for (u32** p : {&w.rows.body_len, &w.rows.crc, &w.rows.out_cap, &w.rows.out_len}) *p = k.take<u32>(ne);
    w.rows.status = k.take<i32>(ne);
    w.rows.type = k.take<u8>(ne);
    w.scratch = k.take<u8>(r.per_round * r.stride);
    w.total = k.bytes();
    return w;
}

// rows [at, ...) of the table
ChunkRows rows_from(const ChunkRows& r, u64 at)
{
    ChunkRows s = r;
    s.type += at;
    s.body_off += at;
    s.out_off += at;
    s.body_len += at;
    s.crc += at;
    s.out_cap += at;
    s.out_len += at;
    s.status += at;
    return s;
}

// ---- the repair planner --------------------------------------------------------------------------------------------------------------------------------
struct RpArgs {
    FrameIndex x;               // (no positions: the planner reads no stream)
    u32 ns;
    const i32* row_status;
    const u64* rep_total;
    const i32* rep_tail;
    u32 nrep;
    const u32 *rp_stream, *rp_replica;
    u32 nout;
};
struct RpWork {
    u64* part;
    i32* begin;                 // rp_begin of every pair
    u64 *segs, *taken, *kept;   // what every pair counts (0 for a pair that is refused)
    u64* need;                  // scan of segs (nout + 1)
    u64* csegs;                 // an admitted pair's segments
    u64 total;
};
struct ScanPairWords {
    const u64* __restrict__ src;
    __device__ __forceinline__ u64 operator()(u64 i) const { return src[i]; }
};

// The rows of stream s walked by a workgroup in tiles of 256, thread t of a tile at row base + t.  The row that takes part before a row: the
// highest lane below it in its wavefront's ballot, else the last such thread of an earlier wavefront, else of an earlier tile (carried).
// visit(row, begins, ordinal): every row that takes part, with the number of its segment among the pair's when it begins one.  -> what the
// thread's rows count; segs: the pair's segments, in every thread.  All threads must call it.
template <class Visit>
__device__ __forceinline__ RpCount rp_walk(const RpArgs& a, u32 s, Visit visit)
{
    __shared__ u32 s_good[256], s_last[4];
    const u32 tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    u64 f0, rows;
    fr_rows(a.x, s, &f0, &rows);
    const u64 f1 = f0 + rows, total = a.x.total[s];
    RpCount c{};
    bool carry_has = false, carry_good = false;
    for (u64 base = f0; base < f1; base += 256u) {
        const u64 i = base + tid;
        const RpRow r = i < f1 ? rp_row(a.x, a.row_status, f1, total, i) : RpRow{};
        const u64 m = ballot64(r.live);
        s_good[tid] = r.good ? 1u : 0u;
        if (lane == 0) s_last[wave] = m ? wave * 64u + (63u - static_cast<u32>(__builtin_clzll(m))) + 1u : 0u;
        __syncthreads();
        bool has_prev = carry_has, prev_good = carry_good;
        u32 last = 0;
        for (u32 q = 0; q < 4; ++q) {
            if (q < wave && s_last[q]) { has_prev = true; prev_good = s_good[s_last[q] - 1] != 0; }
            if (s_last[q]) last = s_last[q];
        }
        const u64 below = m & lanes_below(lane);
        if (below) { has_prev = true; prev_good = s_good[wave * 64u + (63u - static_cast<u32>(__builtin_clzll(below)))] != 0; }
        if (last) { carry_has = true; carry_good = s_good[last - 1] != 0; }
        const bool begins = r.live && rp_begins(has_prev, prev_good, r.good);
        u64 tile;
        const u64 ordinal = c.segs + wg_exclusive_scan(begins ? 1 : 0, &tile);      // (two barriers: s_good and s_last are free again behind it)
        c.segs += tile;
        if (r.live) {
            visit(r, begins, ordinal);
            if (r.good) c.kept += r.len;
            else c.taken += r.len;
        }
    }
    return c;
}

// A workgroup per pair.
__global__ __launch_bounds__(256) void k_rp_count(RpArgs a, RpWork w)
{
    const u32 j = blockIdx.x, s = a.rp_stream[j], t = a.rp_replica[j];
    const i32 st = rp_begin(a.x, a.ns, a.rep_total, a.rep_tail, a.nrep, s, t);
    RpCount c{};
    if (st == SNP_OK) c = rp_walk(a, s, [](const RpRow&, bool, u64) {});
    const u64 taken = block_sum(c.taken), kept = block_sum(c.kept);
    if (threadIdx.x != 0) return;
    w.begin[j] = st;
    w.segs[j] = c.segs;
    w.taken[j] = taken;
    w.kept[j] = kept;
}

// One thread per pair: admission in pair order -- the scan only grows, so a pair is admitted iff the segments up to its last one fit.
__global__ __launch_bounds__(256) void k_rp_admit(u32 nout, RpWork w, u32 max_segs, i32* __restrict__ plan_status)
{
    const u32 j = blockIdx.x * 256u + threadIdx.x;
    if (j >= nout) return;
    const i32 st = w.begin[j];
    const bool admit = st == SNP_OK && w.need[j + 1] <= max_segs;
    plan_status[j] = st != SNP_OK ? st : admit ? SNP_OK : SNP_ERR_OUTPUT_TOO_SMALL;
    w.csegs[j] = admit ? w.segs[j] : 0;
}

// A workgroup per admitted pair: its segments at seg_first[j] (admitted: seg_first[j] + segs <= max_segs).
__global__ __launch_bounds__(256) void k_rp_emit(RpArgs a, RpWork w, const i32* __restrict__ plan_status, const u64* __restrict__ seg_first,
                                                u32* __restrict__ seg_stream, u64* __restrict__ seg_off, u64* __restrict__ seg_len)
{
    const u32 j = blockIdx.x;
    if (plan_status[j] != SNP_OK || w.csegs[j] == 0) return;
    const u32 s = a.rp_stream[j], t = a.rp_replica[j];
    const u64 g0 = seg_first[j];
    const RpCount c = rp_walk(a, s, [&](const RpRow& r, bool begins, u64 ordinal) {
        if (!begins) return;
        seg_stream[g0 + ordinal] = rp_source(a.ns, s, t, r.good);
        seg_off[g0 + ordinal] = r.start;
        if (ordinal) seg_len[g0 + ordinal - 1] = r.start;               // where the segment before it ends; its length below
    });
    if (threadIdx.x == 0) seg_len[g0 + c.segs - 1] = a.x.total[s];
    __syncthreads();
    for (u64 q = threadIdx.x; q < c.segs; q += 256u) seg_len[g0 + q] -= seg_off[g0 + q];
}

// One workgroup: d_result.
__global__ __launch_bounds__(256) void k_rp_result(u32 nout, RpWork w, const i32* __restrict__ plan_status, u64* __restrict__ result)
{
    u64 ok = 0, taken = 0, kept = 0;
    for (u32 j = threadIdx.x; j < nout; j += 256u) {
        ok += plan_status[j] == SNP_OK ? 1 : 0;
        taken += w.taken[j];
        kept += w.kept[j];
    }
    ok = block_sum(ok);
    taken = block_sum(taken);
    kept = block_sum(kept);
    if (threadIdx.x != 0) return;
    result[0] = w.need[nout];
    result[1] = ok;
    result[2] = taken;
    result[3] = kept;
}

RpWork plan_layout(void* base, u32 nout)
{
    RpWork w{};
    if (nout == 0 || nout > 0x7fffffffu) return w;
    WorkCarver k(base);
    w.part = k.take<u64>(scan_tiles_of(nout));
    w.begin = k.take<i32>(nout);
    for (u64** p : {&w.segs, &w.taken, &w.kept, &w.csegs}) *p = k.take<u64>(nout);
    w.need = k.take<u64>(static_cast<u64>(nout) + 1);
    w.total = k.bytes();
    return w;
}

}  // namespace

extern "C" {

uint64_t snp_frame_verify_indexed_workspace(uint32_t nstreams, uint64_t nentries, uint32_t slot_bytes, uint64_t scratch_cap)
{
    return verify_layout(nullptr, nstreams, nentries, slot_bytes, scratch_cap).total;
}

snp_status snp_frame_verify_indexed_batch(snp_ctx* c, const uint8_t* in, const uint64_t* in_off, const uint64_t* in_len, uint32_t nstreams,
                                          const uint64_t* idx_first, const uint64_t* idx_start, const uint64_t* idx_pos, const uint64_t* idx_total,
                                          const int32_t* idx_tail, uint64_t nentries, uint32_t slot_bytes, uint64_t scratch_cap,
                                          int32_t* row_status, int32_t* status, uint64_t* nbad, uint64_t* first_bad, uint64_t* bad_bytes,
                                          uint32_t* flags, void* d_work, uint64_t* d_result)
{
    if (!c || !d_result || nstreams > 0x7fffffffu || nentries > kVfMaxRows || slot_bytes == 0 || slot_bytes > kVfMaxSlot ||   // (one workgroup per stream)
        (nstreams && (!in || !in_off || !in_len || !idx_first || !idx_total || !idx_tail || !status || !nbad || !first_bad || !bad_bytes || !flags ||
                      !d_work)) ||
        (nstreams && nentries && (!idx_start || !idx_pos || !row_status)))
        return SNP_ERR_BAD_ARG;
    DevGuard dg(c);
    if (!dg.ok) return SNP_ERR_DEVICE;
    hipStream_t s = c->stream;
    bool ok = c->check(snp_zero_words_async(reinterpret_cast<u32*>(d_result), 2 * 8, s), "frame verify result");
    if (nstreams == 0) return ok ? SNP_OK : SNP_ERR_DEVICE;
    const VfWork w = verify_layout(d_work, nstreams, nentries, slot_bytes, scratch_cap);
    const u64 ne = nentries;
    const VfArgs a{in, in_off, in_len, nstreams, FrameIndex{idx_first, idx_start, idx_pos, idx_total, idx_tail, nentries}, slot_bytes,
                   vf_rounds(slot_bytes, scratch_cap, ne)};
    // every stream's verdict; every row of those that passed: its status before the decode, its row of the table
    if (ne) hipLaunchKernelGGL(k_vf_init, dim3(static_cast<u32>(std::min<u64>(groups(ne), 1u << 16))), dim3(256), 0, s, ne, w, row_status);
    hipLaunchKernelGGL(k_fr_before, dim3(1), dim3(256), 0, s, a.x, a.ns, w.before);
    hipLaunchKernelGGL(k_vf_check, dim3(a.ns), dim3(256), 0, s, a, w, row_status, flags);
    ok = ok && c->check(hipGetLastError(), "frame verify check");
    // the rounds: decode + CRC verify of a slice of the table into the scratch
    for (u64 q = 0; ok && q < a.rounds.rounds; ++q) {
        const u64 at = q * a.rounds.per_round;
        ok = c->decode_chunks(in, rows_from(w.rows, at), static_cast<u32>(std::min(a.rounds.per_round, ne - at)), w.scratch);
    }
    if (ok) {
        if (ne && a.rounds.rounds) hipLaunchKernelGGL(k_vf_fold, dim3(groups(ne)), dim3(256), 0, s, ne, w, row_status);
        hipLaunchKernelGGL(k_vf_streams, dim3(a.ns), dim3(256), 0, s, a, w, row_status, status, nbad, first_bad, bad_bytes);
        hipLaunchKernelGGL(k_vf_result, dim3(1), dim3(256), 0, s, a.ns, w, a.rounds.rounds, status, nbad, bad_bytes, d_result);
        ok = c->check(hipGetLastError(), "frame verify result");
    }
    return ok ? SNP_OK : SNP_ERR_DEVICE;
}

uint64_t snp_frame_repair_plan_workspace(uint32_t nout) { return plan_layout(nullptr, nout).total; }

snp_status snp_frame_repair_plan_batch(snp_ctx* c, const uint64_t* idx_first, const uint64_t* idx_start, const uint64_t* idx_total,
                                       const int32_t* idx_tail, uint64_t nentries, uint32_t nstreams, const int32_t* row_status,
                                       const uint64_t* rep_total, const int32_t* rep_tail, uint32_t nrep_streams, const uint32_t* rp_stream,
                                       const uint32_t* rp_replica, uint32_t nout, uint32_t max_segs, uint64_t* seg_first, uint32_t* seg_stream,
                                       uint64_t* seg_off, uint64_t* seg_len, int32_t* plan_status, void* d_work, uint64_t* d_result)
{
    if (!c || !d_result || nout > 0x7fffffffu || nstreams > 0x7fffffffu || nrep_streams > 0x7fffffffu || nentries > kVfMaxRows ||   // (a workgroup per pair; a source number fits 32 bits)
        (nout && (!rp_stream || !rp_replica || !seg_first || !plan_status || !d_work)) ||
        (nout && nstreams && (!idx_first || !idx_total || !idx_tail)) || (nout && nstreams && nentries && (!idx_start || !row_status)) ||
        (nout && nrep_streams && (!rep_total || !rep_tail)) || (nout && max_segs && (!seg_stream || !seg_off || !seg_len)))
        return SNP_ERR_BAD_ARG;
    DevGuard dg(c);
    if (!dg.ok) return SNP_ERR_DEVICE;
    hipStream_t s = c->stream;
    bool ok = c->check(snp_zero_words_async(reinterpret_cast<u32*>(d_result), 2 * 4, s), "frame repair plan result");
    if (nout == 0) return ok ? SNP_OK : SNP_ERR_DEVICE;
    const RpWork w = plan_layout(d_work, nout);
    const RpArgs a{FrameIndex{idx_first, idx_start, nullptr, idx_total, idx_tail, nentries}, nstreams, row_status, rep_total, rep_tail, nrep_streams,
                   rp_stream, rp_replica, nout};
    hipLaunchKernelGGL(k_rp_count, dim3(nout), dim3(256), 0, s, a, w);
    ok = ok && c->check(hipGetLastError(), "frame repair plan count") &&
         c->check(launch_scan(ScanPairWords{w.segs}, nout, w.part, w.need, nullptr, s), "frame repair plan need scan");
    if (ok) {
        hipLaunchKernelGGL(k_rp_admit, dim3(groups(nout)), dim3(256), 0, s, nout, w, max_segs, plan_status);
        ok = c->check(hipGetLastError(), "frame repair plan admit") &&
             c->check(launch_scan(ScanPairWords{w.csegs}, nout, w.part, seg_first, nullptr, s), "frame repair plan segment scan");
    }
    if (ok) {
        if (max_segs) hipLaunchKernelGGL(k_rp_emit, dim3(nout), dim3(256), 0, s, a, w, plan_status, seg_first, seg_stream, seg_off, seg_len);
        hipLaunchKernelGGL(k_rp_result, dim3(1), dim3(256), 0, s, nout, w, plan_status, d_result);
        ok = c->check(hipGetLastError(), "frame repair plan emit");
    }
    return ok ? SNP_OK : SNP_ERR_DEVICE;
}

}  // extern "C"

// frame_walk_device.h -- the span walk over MANY framed streams, end to end: the span tables and the per-stream record with their place in a
// workspace (carve_span_walk), the piece scan that gives every stream its first span slot (launch_span_scan), walk A (k_fd_candidates) and walk B
// (k_fd_resolve) with their launch (launch_span_walk).  Shared by the batch decode (frame_buffers.hip, snp_frame_decode_buffers_batch), the
// decode layout (layout.hip, snp_frame_decode_layout_batch) and the range decode (frame_range.hip, snp_frame_decode_range_batch); the resolver takes out_cap == nullptr as "no bound" (the layout call asks for the
// totals, it has no capacities yet).
#pragma once
#include "scan_tiles.h"
#include "frame_hop_device.h"
#include "work_carver.h"

namespace {

constexpr u32 kNone = 0xffffffffu;

__host__ __device__ __forceinline__ u64 ceil_div(u64 n, u64 d) { return n / d + (n % d != 0); }

// scan source: pieces of `unit` bytes in a u64 length (chunks, spans)
struct ScanPieces {
    const u64* __restrict__ len;
    u64 unit;
    __device__ __forceinline__ u64 operator()(u64 i) const { return ceil_div(len[i], unit); }
};

// per span slot, structure of arrays ([max_spans][kMaxCand] for the candidates), as frame_scan.hip's SpanTables; exits are stream-relative
struct FbSpans {
    u32* count;
    u32* start_rel;
    u64* exit;
    u64* dec;
    u32* ndata;
    i32* stop;
    u64* entry;         // true entry of the span (stream-relative), kNoEntry if the chain never starts a header inside it
    u32* chunk_base;    // the stream's data chunks before the span
    u64* out_base;      // the stream's decoded bytes before the span
};
// per stream: what its walk found
struct FbStreams {
    u64* total;         // decoded bytes listed
    i32* tail;          // the error that ended the walk (OUTPUT_TOO_SMALL: not walked, or total > out_cap)
    u32* nc;            // data chunks listed
    u32* fail;          // first failing chunk slot (atomicMin), kNone if none
};

// A: candidates of every span of every walked stream and where their chains lead (k_span_candidates)
__global__ __launch_bounds__(SNP_WAVE) void k_fd_candidates(const u8* __restrict__ in, const u64* __restrict__ in_off, const u64* __restrict__ in_len,
                                                           u32 ns, const u64* __restrict__ sfirst, u32 max_spans, FbSpans t)
{
    __shared__ u32 s_cand[kMaxCand + 1];
    __shared__ u32 s_n;
    const u32 g = blockIdx.x;
    if (g >= sfirst[ns]) return;
    const u32 b = owner_of(sfirst, ns, g);
    if (sfirst[b + 1] > max_spans) return;                              // the stream is not walked
    const u8* const p = in + in_off[b];
    const u64 n = in_len[b];
    const u64 k = g - sfirst[b];
    const u32 lane = lane_id();
    const u64 s0 = k * kSpan;
    const u64 s1 = s0 + kSpan < n ? s0 + kSpan : n;
    if (lane == 0) s_n = 0;
    __syncthreads();
    if (k == 0) {
        if (lane == 0) { s_cand[0] = 0; s_n = 1; }                      // a stream starts at its byte 0, whatever is there
    } else {
        const u64 wend = s0 + kWindow < s1 ? s0 + kWindow : s1;
        for (u64 base = s0; base < wend; base += SNP_WAVE) {
            const u64 q = base + lane;
            const bool ok = q < wend && plausible_start(p, n, q);
            const u64 m = ballot64(ok);
            if (m) {
                const u32 have = s_n;
                if (ok) {
                    const u32 idx = have + static_cast<u32>(__builtin_popcountll(m & lanes_below(lane)));
                    if (idx < kMaxCand) s_cand[idx] = static_cast<u32>(q - s0);
                }
                __syncthreads();
                if (lane == 0) { const u32 tot = have + static_cast<u32>(__builtin_popcountll(m)); s_n = tot < kMaxCand ? tot : kMaxCand; }
                __syncthreads();
                if (s_n == kMaxCand) break;
            }
        }
    }
    __syncthreads();
    const u32 nc = s_n;
    if (lane == 0) t.count[g] = nc;
    if (lane < nc) {
        const Chain c = follow_chain(p, n, s0 + s_cand[lane], s0 + kSpan);
        const u64 i = static_cast<u64>(g) * kMaxCand + lane;
        t.start_rel[i] = s_cand[lane];
        t.exit[i] = c.exit;
        t.dec[i] = c.dec;
        t.ndata[i] = c.ndata;
        t.stop[i] = c.stop;
    }
}

// B: the true chain through each stream's spans, one wavefront per stream (k_span_resolve without a chunk-table bound: admission by
// max_chunks comes after, by the scan of what every stream lists).  out_cap == nullptr: no bound, every stream keeps what its walk lists.
// *missed += spans whose entry was no candidate.
__global__ __launch_bounds__(SNP_WAVE) void k_fd_resolve(const u8* __restrict__ in, const u64* __restrict__ in_off, const u64* __restrict__ in_len,
                                                        const u64* __restrict__ out_cap, const u64* __restrict__ sfirst, u32 max_spans, FbSpans t,
                                                        FbStreams st, u64* __restrict__ missed_total)
{
    const u32 b = blockIdx.x;
    const u32 lane = lane_id();
    const u8* const p = in + in_off[b];
    const u64 n = in_len[b];
    const u64 g0 = sfirst[b], nspans = sfirst[b + 1] - g0;
    u64 total = 0, e = 0;
    u32 nc = 0, missed = 0;
    i32 tail = SNP_OK;
    if (sfirst[b + 1] > max_spans) {
        tail = SNP_ERR_OUTPUT_TOO_SMALL;                                // not walked: its spans do not fit
    } else if (nspans) {
        for (u64 k = lane; k < nspans; k += SNP_WAVE) t.entry[g0 + k] = kNoEntry;
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        u64 batch0 = ~0ull;                                             // first span of the batch held in registers
        u32 cnt = 0, srel[kMaxCand] = {}, cnd[kMaxCand] = {};
        i32 cst[kMaxCand] = {};
        u64 cex[kMaxCand] = {}, cde[kMaxCand] = {};
        for (;;) {
            if (e >= n) break;                                          // clean end (n > 0: at least one header was walked)
            const u64 k = e / kSpan;
            if (k < batch0 || k >= batch0 + SNP_WAVE) {                 // load the candidates of 64 spans
                batch0 = k;
                const u64 mine = batch0 + lane;
                const u64 gi = g0 + mine;
                cnt = mine < nspans ? t.count[gi] : 0;
#pragma unroll
                for (u32 j = 0; j < kMaxCand; ++j) {
                    const bool have = mine < nspans && j < cnt;
                    srel[j] = have ? t.start_rel[gi * kMaxCand + j] : 0xffffffffu;
                    cex[j] = have ? t.exit[gi * kMaxCand + j] : 0;
                    cde[j] = have ? t.dec[gi * kMaxCand + j] : 0;
                    cnd[j] = have ? t.ndata[gi * kMaxCand + j] : 0;
                    cst[j] = have ? t.stop[gi * kMaxCand + j] : 0;
                }
            }
            const u32 l = static_cast<u32>(k - batch0);
            const u32 rel = static_cast<u32>(e - k * kSpan);
            Chain c{};
            bool found = false;
#pragma unroll
            for (u32 j = 0; j < kMaxCand; ++j) {
                if (!found && read_lane(srel[j], l) == rel) {
                    found = true;
                    c.exit = (static_cast<u64>(read_lane(static_cast<u32>(cex[j] >> 32), l)) << 32) | read_lane(static_cast<u32>(cex[j]), l);
                    c.dec = (static_cast<u64>(read_lane(static_cast<u32>(cde[j] >> 32), l)) << 32) | read_lane(static_cast<u32>(cde[j]), l);
                    c.ndata = read_lane(cnd[j], l);
                    c.stop = static_cast<i32>(read_lane(static_cast<u32>(cst[j]), l));
                }
            }
            if (!found) {                                               // not guessed: walk this span here
                c = follow_chain(p, n, e, (k + 1) * kSpan);
                ++missed;
            }
            if (lane == 0) { t.entry[g0 + k] = e; t.chunk_base[g0 + k] = nc; t.out_base[g0 + k] = total; }
            nc += c.ndata;
            total += c.dec;
            if (c.stop > 0) { tail = c.stop; break; }
            if (c.stop < 0) break;
            e = c.exit;
        }
        if (out_cap && total > out_cap[b]) { tail = SNP_ERR_OUTPUT_TOO_SMALL; nc = 0; total = 0; }   // nothing is decoded
    }
    if (lane == 0) {
        st.total[b] = total;
        st.tail[b] = tail;
        st.nc[b] = nc;
        st.fail[b] = kNone;
        if (missed) atomicAdd(reinterpret_cast<unsigned long long*>(missed_total), static_cast<unsigned long long>(missed));
    }
}

// ---- host side ---------------------------------------------------------------------------------------------------------------------------------
// The walk's pieces of a workspace, in the order both callers have always had them: the per-stream record, then per span slot the candidates
// and the resolver's entry.  (Each caller carves sfirst, its second per-stream table and the tile sums before this.)
inline void carve_span_walk(WorkCarver& k, u64 ns, u64 max_spans, FbStreams& st, FbSpans& sp)
{
    st.total = k.take<u64>(ns);
    st.tail = k.take<i32>(ns);
    st.nc = k.take<u32>(ns);
    st.fail = k.take<u32>(ns);
    sp.count = k.take<u32>(max_spans);
    sp.start_rel = k.take<u32>(max_spans * kMaxCand);
    sp.exit = k.take<u64>(max_spans * kMaxCand);
    sp.dec = k.take<u64>(max_spans * kMaxCand);
    sp.ndata = k.take<u32>(max_spans * kMaxCand);
    sp.stop = k.take<i32>(max_spans * kMaxCand);
    sp.entry = k.take<u64>(max_spans);
    sp.chunk_base = k.take<u32>(max_spans);
    sp.out_base = k.take<u64>(max_spans);
}

// sfirst[0 .. ns] = first span slot of every stream; span_result[0] = span slots needed, span_result[1] = 0.  The word launch_span_walk adds
// to must be zero by then: the scan does that when the word follows the count, a caller that keeps it elsewhere clears it between the two.
inline hipError_t launch_span_scan(const u64* in_len, u32 ns, u64* part, u64* sfirst, u64* span_result, hipStream_t stream)
{
    return launch_scan(ScanPieces{in_len, kSpan}, ns, part, sfirst, span_result, stream);
}

// walks A and B over max_spans slots; out_cap == nullptr: no bound; *missed += spans the resolver walked on the spot
inline hipError_t launch_span_walk(const u8* in, const u64* in_off, const u64* in_len, const u64* out_cap, u32 ns, const u64* sfirst,
                                   u32 max_spans, const FbSpans& sp, const FbStreams& st, u64* missed, hipStream_t stream)
{
    if (max_spans) hipLaunchKernelGGL(k_fd_candidates, dim3(max_spans), dim3(SNP_WAVE), 0, stream, in, in_off, in_len, ns, sfirst, max_spans, sp);
    hipLaunchKernelGGL(k_fd_resolve, dim3(ns), dim3(SNP_WAVE), 0, stream, in, in_off, in_len, out_cap, sfirst, max_spans, sp, st, missed);
    return hipGetLastError();
}

}  // namespace

// frame_walk_device.h -- the span walk over MANY framed streams, end to end: the per-stream record and its place in a workspace next to the span
// slots of the batch (carve_span_walk), the piece scan that gives every stream its first span slot (launch_span_scan), the drivers of walk A
// (k_fd_candidates) and walk B (k_fd_resolve) with their launch (launch_span_walk).  What one span of one stream takes -- the hop, the candidates,
// the lookup among them, the span and chunk tables -- is frame_hop_device.h; the drivers here only find their stream and span slot.  Shared by the
// batch decode (frame_buffers.hip, snp_frame_decode_buffers_batch), the decode layout (layout.hip, snp_frame_decode_layout_batch) and the range
// decode (frame_range.hip, snp_frame_decode_range_batch) and the index build (frame_index.hip, snp_frame_index_batch); the resolver takes out_cap == nullptr as "no bound" (the layout call asks for the totals,
// it has no capacities yet).
#pragma once
#include "scan_tiles.h"
#include "frame_hop_device.h"

namespace {

__host__ __device__ __forceinline__ u64 ceil_div(u64 n, u64 d) { return n / d + (n % d != 0); }

// scan source: pieces of `unit` bytes in a u64 length (chunks, spans)
struct ScanPieces {
    const u64* __restrict__ len;
    u64 unit;
    __device__ __forceinline__ u64 operator()(u64 i) const { return ceil_div(len[i], unit); }
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
    const u32 count = span_candidates(p, n, k, s_cand, &s_n);
    span_candidates_row(t, g, p, n, k, s_cand, count);
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
        SpanBatch held;
        for (;;) {
            if (e >= n) break;                                          // clean end (n > 0: at least one header was walked)
            const u64 k = e / kSpan;
            held.load(t, g0, nspans, k);
            Chain c{};
            if (!held.find(e, k, &c)) {                                 // not guessed: walk this span here
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
        if (missed) atomic_add64(missed_total, missed);
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
    sp = carve_spans(k, max_spans);
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

// frame_scan.hip -- chunk-header walk of a framed stream that is already in HBM and has no chunk table
// (SnappyStreamDecompressor.ReadChunkHeader / Decompress, Snappier/Internal/SnappyStreamDecompressor.cs:53-199,215-289).
//
// A framed stream carries no index: header i gives the position of header i+1, a serial chain of ~64 KiB hops, each a
// dependent HBM round trip (round 1: one lane, 0.9 us per chunk -- 146 ms of the 176 ms a 10 GiB stream took to decode).
// Here the chain is broken into 1 MiB SPANS that are walked concurrently:
//   A  k_span_candidates  one wavefront per span: test every byte of the span's first 80 KiB for "a data chunk or a stream
//                         identifier could start here" (type, 24-bit size, preamble varint, expansion bound, fits the stream:
//                         passes ~1e-5 of random positions, and always the true one if the chunk before it is a spec-sized
//                         data chunk), then lane c follows candidate c's chain to the end of the span: exit position, data
//                         chunks met, bytes they declare, the error that ended it if any;
//   B  k_span_resolve     one wavefront: the true chain enters span 0 at byte 0; its exit selects the candidate of the next
//                         span that starts exactly there, and so on -- 64 spans per batch out of registers.  An entry that
//                         is no candidate (behind a skippable chunk, a chunk larger than the window) is walked on the spot;
//   C  k_span_emit        one wavefront per span: walk the span again from its true entry and write the chunk table rows at
//                         their final indices; entries past the last chunk become empty chunks (the decode and CRC launches
//                         run over max_chunks rows without a host round trip).
// One hop, the candidates of a span, the lookup among them, the hops over a span's chunks and both tables live in frame_hop_device.h, shared with the
// many-stream walk (frame_walk_device.h); the kernels here are its drivers for ONE stream: span k is span slot k, and the resolver clips at a full
// chunk table.
#include "frame_hop_device.h"

namespace {

// ---- A: candidates of every span and where their chains lead ----------------------------------------------------------
__global__ __launch_bounds__(SNP_WAVE) void k_span_candidates(const u8* __restrict__ in, u64 n, u64 nspans, FbSpans t)
{
    __shared__ u32 s_cand[kMaxCand + 1];
    __shared__ u32 s_n;
    const u64 k = blockIdx.x;
    if (k >= nspans) return;
    const u32 count = span_candidates(in, n, k, s_cand, &s_n);
    span_candidates_row(t, k, in, n, k, s_cand, count);
}

// ---- B: the true chain through the spans ------------------------------------------------------------------------------
// hdr: [0] total decoded bytes, [1] tail status, [2] data chunks listed.
__global__ __launch_bounds__(SNP_WAVE) void k_span_resolve(const u8* __restrict__ in, u64 n, u64 cap, u32 max_chunks, u64 nspans,
                                                          FbSpans t, u64* __restrict__ hdr)
{
    const u32 lane = lane_id();
    for (u64 k = lane; k < nspans; k += SNP_WAVE) t.entry[k] = kNoEntry;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    u64 e = 0, total = 0;
    u32 nc = 0;
    i32 tail = SNP_OK;
    const bool stop = n == 0;
    SpanBatch held;
    while (!stop) {
        if (e >= n) break;                                              // clean end (n > 0: at least one header was walked)
        const u64 k = e / kSpan;
        held.load(t, 0, nspans, k);
        Chain c{};
        if (!held.find(e, k, &c)) c = follow_chain(in, n, e, (k + 1) * kSpan);   // not guessed: walk this span here
        if (lane == 0) { t.entry[k] = e; t.chunk_base[k] = nc; t.out_base[k] = total; }
        if (nc + c.ndata > max_chunks) {
            // the chunk table fills up inside this span: list what fits, exactly as a serial walk would (the emitter clips its rows at hdr[2])
            const i32 end = for_span_chunks(in, n, e, ~0ull, nc, ~0u, total, [&](const Hop& h, u64, u32, u64) {
                if (nc == max_chunks) { tail = SNP_ERR_OUTPUT_TOO_SMALL; return false; }   // chunk table full
                ++nc;
                total += h.dec;
                return true;
            });
            if (end > 0) tail = end;
            break;
        }
        nc += c.ndata;
        total += c.dec;
        if (c.stop > 0) { tail = c.stop; break; }
        if (c.stop < 0) break;
        e = c.exit;
    }
    if (total > cap) { tail = SNP_ERR_OUTPUT_TOO_SMALL; nc = 0; total = 0; }   // nothing is decoded
    if (lane == 0) {
        hdr[0] = total;
        hdr[1] = static_cast<u64>(static_cast<u32>(tail));
        hdr[2] = nc;
    }
}

// ---- C: the chunk table ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(SNP_WAVE) void k_span_emit(const u8* __restrict__ in, u64 n, u32 max_chunks, u64 nspans, FbSpans t,
                                                       const u64* __restrict__ hdr, ChunkRows r)
{
    const u64 k = blockIdx.x;
    const u32 lane = lane_id();
    const u32 nc_total = static_cast<u32>(hdr[2]);
    if (k >= nspans) {                                                  // the extra workgroups pad the table with empty chunks
        const u64 total = hdr[0];
        for (u64 i = nc_total + (k - nspans) * SNP_WAVE + lane; i < max_chunks; i += (gridDim.x - nspans) * SNP_WAVE) chunk_row_clear(r, i, total);
        return;
    }
    const u64 e = t.entry[k];
    if (e == kNoEntry || lane != 0) return;
    for_span_chunks(in, n, e, (k + 1) * kSpan, t.chunk_base[k], nc_total, t.out_base[k], [&](const Hop& h, u64 ip, u32 idx, u64 off) {
        chunk_row_set(r, idx, h, ip, off);
        return true;
    });
}

}  // namespace

// Internal: the span table in context scratch (snp_ctx::scan), carved like the d_work workspaces.
extern "C" size_t snp_frame_scan_workspace(u64 n)
{
    WorkCarver k(nullptr);
    (void)carve_spans(k, (n + kSpan - 1) / kSpan);
    return k.bytes();
}

extern "C" hipError_t snp_launch_frame_scan_spans(const u8* in, u64 n, u64 cap, u32 max_chunks, const ChunkRows& r, u64* hdr, void* work,
                                                  hipStream_t stream)
{
    const u64 nspans = (n + kSpan - 1) / kSpan;
    WorkCarver k(work);
    const FbSpans t = carve_spans(k, nspans);
    if (nspans) hipLaunchKernelGGL(k_span_candidates, dim3(static_cast<u32>(nspans)), dim3(SNP_WAVE), 0, stream, in, n, nspans, t);
    hipLaunchKernelGGL(k_span_resolve, dim3(1), dim3(SNP_WAVE), 0, stream, in, n, cap, max_chunks, nspans, t, hdr);
    const u32 pad = max_chunks ? 64u : 1u;
    hipLaunchKernelGGL(k_span_emit, dim3(static_cast<u32>(nspans) + pad), dim3(SNP_WAVE), 0, stream, in, n, max_chunks, nspans, t, hdr, r);
    return hipGetLastError();
}

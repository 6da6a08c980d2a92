// frame_range.hip -- snp_frame_decode_range_batch: a window [lo, hi) of decoded bytes out of every one of many Snappy framed streams, decoding only
// the chunks that meet it.  Every data chunk is an independent Snappy block with its own CRC (SnappyStreamDecompressor.cs:117-131), so the format
// allows random access at chunk granularity; the span walk of snp_frame_decode_buffers_batch already leaves, per 1 MiB span, where its first
// header is and how many chunks and decoded bytes precede it.  Built into libsnappier_hip_frame_range.so (C-ABI: include/snappier_hip_frame_range.h),
// linked against libsnappier_hip.so.  DESIGN.md 4.13.
//
//   scan      ceil(in_len / 2^20) -> each stream's first span slot (d_result[2]); a stream whose spans do not fit is not walked
//   A, B      the span walk (frame_walk_device.h) with no capacity bound: entry, chunk_base, out_base of every span, total and tail of every stream
//   window    one thread per stream: lo, hi, "the window does not fit out_cap" (such a stream selects nothing); its two edge slots, two rows of
//             the edge table and its failure word emptied
//   select    one wavefront per span slot: ONLY a span whose decoded bytes [out_base, the next entered span's out_base) meet the window is hopped
//             (for_span_chunks, frame_hop_device.h); it counts the span's interior chunks and records an edge chunk in its stream's head or tail slot
//   scans     interior counts over the span slots -> each span's (and so each stream's) first row (d_result[0]); over the edge slots, the decoded
//             sizes -> each edge's place in the scratch arena (d_result[4]), and the slots in use -> each edge's row in the edge table
//   admit     one thread per stream: spans, interior rows and edge bytes within their bounds -> its edges' rows.  The edge table is COMPACT
//             (the edges of the admitted streams first, empty rows behind them): with an empty row between any two edges the decoder took
//             17.5 ms for the 163 840 edges of the 64 KiB shape, against 9.3 ms for the same chunks as a dense table
//   emit      every row an empty raw chunk with the CRC of nothing (k_fd_pad), then one wavefront per span slot with interior chunks: their rows,
//             the output at out_off[b] + (s - lo)
//   decode    snp_ctx::decode_chunks (decode + CRC verify) over the interior table into `out`, and over the 2 x nstreams rows of the edge table
//             into scratch (two calls: the decoder takes one output base)
//   trim      one workgroup per edge row: the part of an OK edge inside the window, scratch -> out
//   verdict   one thread per failing row: atomicMin of (its place in the stream, status) into the stream's word (k_fd_fail); one thread per
//             stream: the head edge, else the first failing interior row, else the tail edge, else the walk's tail, else the capacity, else OK
// Nothing here allocates, reads back or synchronises: the call is capturable like the other _batch entry points.
#include "capi_internal.h"
#include "frame_walk_device.h"
#include "frame_edges_device.h"
#include "../../include/snappier_hip_frame_range.h"

namespace {

constexpr u32 kSmall = 1u;              // flags: hi - lo > out_cap (nothing of the stream is selected)
constexpr u32 kAdmitted = 2u;           // flags: spans, interior rows and edge bytes fit

// per stream
struct FrStreams {
    u64 *lo, *hi;       // the clipped window
    u32* flags;
    u64* fail;          // min over the failing interior rows of (1 + place among the stream's rows) << 8 | status
};
// Two edge slots per stream (FrEdges, frame_edges_device.h), where k_fr_select records what it finds (head: 2 b, tail: 2 b + 1).
// The two chunk tables (ChunkRows): the interior rows over max_chunks slots, tagged with their stream; and the edge table the decoder sees, 2 ns
// rows -- the edges of the admitted streams in stream order, then empty rows -- tagged with the edge slot the row came from.

__global__ __launch_bounds__(256) void k_fr_window(u32 ns, const u64* __restrict__ sfirst, u32 max_spans, const u64* __restrict__ range_off,
                                                  const u64* __restrict__ range_len, const u64* __restrict__ out_cap, FbStreams st, FrStreams w,
                                                  FrEdges e, ChunkRows c, u64* __restrict__ result)
{
    const u32 b = blockIdx.x * 256u + threadIdx.x;
    if (b == 0) { result[4] = 0; result[5] = 0; }
    if (b >= ns) return;
    const u64 total = st.total[b];                                      // (0 for a stream that was not walked)
    const u64 ro = range_off[b], rl = range_len[b];
    const u64 end = ro + rl < ro ? ~0ull : ro + rl;
    const u64 lo = ro < total ? ro : total, hi = end < total ? end : total;
    w.lo[b] = lo;
    w.hi[b] = hi;
    w.flags[b] = sfirst[b + 1] <= max_spans && hi - lo > out_cap[b] ? kSmall : 0u;
    w.fail[b] = kNoFail;
    e.dec[2ull * b] = 0;
    e.dec[2ull * b + 1] = 0;
    for (u64 row = 2ull * b; row < 2ull * b + 2; ++row) {
        c.tag[row] = kNone;
        chunk_row_clear(c, row, 0);
    }
}

// Where span g's decoded bytes end: the out_base of the stream's next span that the chain entered, else the stream's total.  (A span the chain
// never starts a header in -- a chunk larger than a span runs across it -- has no out_base.)
__device__ __forceinline__ u64 span_out_end(const FbSpans& t, u64 g, u64 g_end, u64 total)
{
    for (u64 k = g + 1; k < g_end; ++k)
        if (t.entry[k] != kNoEntry) return t.out_base[k];
    return total;
}

// One wavefront per span slot; lane 0 hops (a few headers per MiB), as in k_fd_emit.  Writes icount[g] for EVERY slot below max_spans.
__global__ __launch_bounds__(SNP_WAVE) void k_fr_select(const u8* __restrict__ in, const u64* __restrict__ in_off, const u64* __restrict__ in_len, u32 ns,
                                                       const u64* __restrict__ sfirst, u32 max_spans, FbSpans t, FbStreams st, FrStreams w, FrEdges e,
                                                       u32* __restrict__ icount)
{
    const u32 g = blockIdx.x;
    if (lane_id() != 0) return;
    u32 cnt = 0;
    if (g < sfirst[ns]) {
        const u32 b = owner_of(sfirst, ns, g);
        const u64 entry = sfirst[b + 1] <= max_spans && !(w.flags[b] & kSmall) ? t.entry[g] : kNoEntry;
        if (entry != kNoEntry) {
            const u64 lo = w.lo[b], hi = w.hi[b];
            const u64 off0 = t.out_base[g];
            // the test that makes a narrow window in a long stream cheap: a span wholly outside the window is not hopped
            if (off0 < hi && span_out_end(t, g, sfirst[b + 1], st.total[b]) > lo) {
                const u64 ib = in_off[b];
                for_span_chunks(in + ib, in_len[b], entry, (g - sfirst[b] + 1) * kSpan, t.chunk_base[g], st.nc[b], off0,
                                [&](const Hop& h, u64 ip, u32, u64 off) {
                                    if (h.dec > 0 && off + h.dec > lo) {            // selected (off < hi)
                                        if (off >= lo && off + h.dec <= hi) {
                                            ++cnt;
                                        } else {                        // an edge: the one chunk that holds lo is the head, any other the tail
                                            edge_slot_set(e, 2ull * b + (off > lo ? 1 : 0), h, ib + ip, off);
                                        }
                                    }
                                    return off + h.dec < hi;            // the chunks behind the window are not hopped
                                });
            }
        }
    }
    icount[g] = cnt;
}

// Admission (in stream order: the three sums only grow), the rows of the admitted streams' edges with their places in the scratch arena,
// d_result[4] and [5].  (A rank is below 2 ns and belongs to one edge: every row is written by one thread, after k_fr_window emptied it.)
__global__ __launch_bounds__(256) void k_fr_admit(u32 ns, const u64* __restrict__ sfirst, u32 max_spans, const u64* __restrict__ ispan, u32 max_chunks,
                                                 u64 edge_cap, FrStreams w, FrEdges e, ChunkRows c, u64* __restrict__ result)
{
    const u32 b = blockIdx.x * 256u + threadIdx.x;
    u64 nsel = 0;
    if (b < ns) {
        const bool ok = sfirst[b + 1] <= max_spans && ispan[sfirst[b + 1]] <= max_chunks && e.place[2ull * b + 2] <= edge_cap;
        if (ok) w.flags[b] |= kAdmitted;
        for (u64 slot = 2ull * b; slot < 2ull * b + 2; ++slot) {
            if (e.dec[slot] == 0) continue;
            ++nsel;
            if (ok) edge_row_place(c, e, slot);
        }
        if (b == 0) {
            result[4] = e.place[2ull * ns];
            nsel += ispan[max_spans];
        }
    }
    nsel = wave_sum(nsel);
    if ((threadIdx.x & 63u) == 0 && nsel) atomic_add64(result + 5, nsel);
}

// every interior slot an empty row owned by no stream (k_fd_pad); k_fr_emit then fills the rows in use
__global__ __launch_bounds__(256) void k_fr_pad(u32 max_chunks, ChunkRows r)
{
    const u32 c = blockIdx.x * 256u + threadIdx.x;
    if (c >= max_chunks) return;
    r.tag[c] = kNone;
    chunk_row_clear(r, c, 0);
}

// the interior rows of every span of every admitted stream: the hops of k_fr_select again, only where it counted a row
__global__ __launch_bounds__(SNP_WAVE) void k_fr_emit(const u8* __restrict__ in, const u64* __restrict__ in_off, const u64* __restrict__ in_len,
                                                     const u64* __restrict__ out_off, u32 ns, const u64* __restrict__ sfirst, u32 max_spans,
                                                     const u64* __restrict__ ispan, const u32* __restrict__ icount, u32 max_chunks, FbSpans t,
                                                     FbStreams st, FrStreams w, ChunkRows r)
{
    const u32 g = blockIdx.x;
    if (lane_id() != 0 || g >= sfirst[ns]) return;
    const u32 cnt = icount[g];
    if (cnt == 0) return;                                               // (a span with rows: its stream was walked and entered the span)
    const u32 b = owner_of(sfirst, ns, g);
    if (!(w.flags[b] & kAdmitted)) return;
    const u64 ib = in_off[b], ob = out_off[b], lo = w.lo[b], hi = w.hi[b];
    u64 row = ispan[g];
    const u64 row_end = row + cnt;                                      // <= ispan[sfirst[b + 1]] <= max_chunks: the stream is admitted
    if (row_end > max_chunks) return;
    for_span_chunks(in + ib, in_len[b], t.entry[g], (g - sfirst[b] + 1) * kSpan, t.chunk_base[g], st.nc[b], t.out_base[g],
                    [&](const Hop& h, u64 ip, u32, u64 off) {
                        if (h.dec > 0 && off >= lo && off + h.dec <= hi) {
                            r.tag[row] = b;
                            chunk_row_set(r, row, h, ib + ip, ob + (off - lo));
                            ++row;
                        }
                        return off + h.dec < hi && row < row_end;
                    });
}

// One workgroup per edge row: an OK edge's bytes inside the window, scratch -> out (edge_trim).
__global__ __launch_bounds__(256) void k_fr_trim(ChunkRows c, FrEdges e, FrStreams w, const u8* __restrict__ scratch, u8* __restrict__ out,
                                                const u64* __restrict__ out_off)
{
    const u64 row = blockIdx.x;
    const u32 slot = c.tag[row];
    if (slot == kNone) return;
    const u32 b = slot >> 1;
    edge_trim(c, e, row, slot, w.lo[b], w.hi[b], scratch, out + out_off[b], threadIdx.x);
}

// k_fd_fail over the interior table, keyed by the row's place in its stream
__global__ __launch_bounds__(256) void k_fr_fail(u32 max_chunks, ChunkRows r, const u64* __restrict__ sfirst, const u64* __restrict__ ispan, FrStreams w)
{
    const u32 c = blockIdx.x * 256u + threadIdx.x;
    if (c >= max_chunks) return;
    const u32 b = r.tag[c];
    if (b == kNone || r.status[c] == SNP_OK) return;
    atomic_min64(w.fail + b, fail_key(c - ispan[sfirst[b]], r.status[c]));
}

// the stream's verdict: the first failing selected chunk in stream order (head edge, interior rows, tail edge), else the error that ended the
// walk, else the capacity, else OK with hi - lo bytes.  result[1] += the OK lengths (one atomic per wavefront).
__global__ __launch_bounds__(256) void k_fr_verdict(u32 ns, FbStreams st, FrStreams w, FrEdges e, ChunkRows c, u64* __restrict__ out_len,
                                                   i32* __restrict__ status, u64* __restrict__ result)
{
    const u32 b = blockIdx.x * 256u + threadIdx.x;
    u64 ok_len = 0;
    if (b < ns) {
        i32 s = SNP_ERR_OUTPUT_TOO_SMALL;
        const u32 flags = w.flags[b];
        if (flags & kAdmitted) {
            s = window_verdict(edge_status(c, e, 2ull * b), w.fail[b], edge_status(c, e, 2ull * b + 1), st.tail[b], flags & kSmall);
            if (s == SNP_OK) ok_len = w.hi[b] - w.lo[b];
        }
        status[b] = s;
        out_len[b] = ok_len;
    }
    ok_len = wave_sum(ok_len);
    if ((threadIdx.x & 63u) == 0 && ok_len) atomic_add64(result + 1, ok_len);
}

// ---- workspace (every piece 256-byte aligned; nothing when there is no stream) -----------------------------------------------------------------
// Per stream: first span slot (ns + 1), the walk's record, the window, two edge slots and two rows of the edge table.  Per span slot: the candidates and the resolver's entry, the
// interior count and its scan (max_spans + 1).  Per chunk slot: the interior chunk table.  The tile sums of the scans (the largest of them).  Then
// edge_cap bytes of scratch.
struct RangeWork {
    u64 *sfirst, *part, *ispan;
    u32* icount;
    FbStreams st;
    FbSpans sp;
    FrStreams w;
    ChunkRows r;         // interior rows
    FrEdges e;
    ChunkRows c;         // edge rows
    u8* scratch;
    u64 bytes;
};
RangeWork range_work_layout(void* base, u32 nstreams, u32 max_chunks, u32 max_spans, u64 edge_cap)
{
    RangeWork k{};
    if (nstreams == 0) return k;
    const u64 ns = nstreams, nc = max_chunks, nsp = max_spans, ne = 2 * ns;
    WorkCarver c(base);
    k.sfirst = c.take<u64>(ns + 1);
    k.part = c.take<u64>(scan_tiles_of(ne > nsp ? ne : nsp));
    carve_span_walk(c, ns, nsp, k.st, k.sp);
    k.w.lo = c.take<u64>(ns);
    k.w.hi = c.take<u64>(ns);
    k.w.fail = c.take<u64>(ns);
    k.w.flags = c.take<u32>(ns);
    k.icount = c.take<u32>(nsp);
    k.ispan = c.take<u64>(nsp + 1);
    k.r = carve_chunk_rows(c, nc);
    k.e = carve_edges(c, ne);
    k.c = carve_chunk_rows(c, ne);
    k.scratch = c.take<u8>(edge_cap);
    k.bytes = c.bytes();
    return k;
}

}  // namespace

extern "C" {

uint64_t snp_frame_decode_range_workspace(uint32_t nstreams, uint32_t max_chunks, uint32_t max_spans, uint64_t edge_cap)
{
    return range_work_layout(nullptr, nstreams, max_chunks, max_spans, edge_cap).bytes;
}

snp_status snp_frame_decode_range_batch(snp_ctx* c, const uint8_t* in, const uint64_t* in_off, const uint64_t* in_len, uint32_t nstreams,
                                        const uint64_t* range_off, const uint64_t* range_len, uint32_t max_chunks, uint32_t max_spans,
                                        uint64_t edge_cap, uint8_t* out, const uint64_t* out_off, const uint64_t* out_cap, uint64_t* out_len,
                                        int32_t* status, void* d_work, uint64_t* d_result)
{
    if (!c || !d_result || nstreams > 0x3fffffffu ||   // (one workgroup per edge row: 2 x nstreams must be a grid)
        (nstreams && (!in || !in_off || !in_len || !range_off || !range_len || !out || !out_off || !out_cap || !out_len || !status || !d_work)))
        return SNP_ERR_BAD_ARG;
    DevGuard dg(c);
    if (!dg.ok) return SNP_ERR_DEVICE;
    hipStream_t s = c->stream;
    if (nstreams == 0)
        return c->check(snp_zero_words_async(reinterpret_cast<u32*>(d_result), 2 * 6, s), "frame range result") ? SNP_OK : SNP_ERR_DEVICE;
    const RangeWork w = range_work_layout(d_work, nstreams, max_chunks, max_spans, edge_cap);
    const u32 ns = nstreams, M = max_chunks, S = max_spans, E = 2 * ns, groups = (ns + 255u) / 256u;
    // the span walk: first span slot of every stream (d_result[2] = span slots needed, d_result[3] = 0), candidates, one chain per stream, no bound
    bool ok = c->check(launch_span_scan(in_len, ns, w.part, w.sfirst, d_result + 2, s), "frame range span scan") &&
              c->check(launch_span_walk(in, in_off, in_len, nullptr, ns, w.sfirst, S, w.sp, w.st, d_result + 3, s), "frame range walk");
    if (ok) {
        hipLaunchKernelGGL(k_fr_window, dim3(groups), dim3(256), 0, s, ns, w.sfirst, S, range_off, range_len, out_cap, w.st, w.w, w.e, w.c,
                           d_result);
        if (S) hipLaunchKernelGGL(k_fr_select, dim3(S), dim3(SNP_WAVE), 0, s, in, in_off, in_len, ns, w.sfirst, S, w.sp, w.st, w.w, w.e, w.icount);
        ok = c->check(hipGetLastError(), "frame range select");
    }
    // first interior row of every span slot (d_result[0] = rows needed, d_result[1] = 0), every edge's place in the scratch arena, admission
    ok = ok && c->check(launch_scan(ScanPlain{w.icount}, S, w.part, w.ispan, d_result, s), "frame range row scan") &&
         c->check(launch_scan(ScanEdgeBytes{w.e.dec}, E, w.part, w.e.place, nullptr, s), "frame range edge scan") &&
         c->check(launch_scan(ScanEdgeCount{w.e.dec}, E, w.part, w.e.rank, nullptr, s), "frame range edge rank scan");
    if (ok) {
        hipLaunchKernelGGL(k_fr_admit, dim3(groups), dim3(256), 0, s, ns, w.sfirst, S, w.ispan, M, edge_cap, w.w, w.e, w.c, d_result);
        ok = c->check(hipGetLastError(), "frame range admit");
    }
    if (ok && M) {
        hipLaunchKernelGGL(k_fr_pad, dim3((M + 255u) / 256u), dim3(256), 0, s, M, w.r);
        if (S) hipLaunchKernelGGL(k_fr_emit, dim3(S), dim3(SNP_WAVE), 0, s, in, in_off, in_len, out_off, ns, w.sfirst, S, w.ispan, w.icount, M, w.sp,
                                  w.st, w.w, w.r);
        // decode + CRC verify of every interior slot, straight into out
        ok = c->check(hipGetLastError(), "frame range table") && c->decode_chunks(in, w.r, M, out);
        if (ok) hipLaunchKernelGGL(k_fr_fail, dim3((M + 255u) / 256u), dim3(256), 0, s, M, w.r, w.sfirst, w.ispan, w.w);
    }
    // the edges, whole, into scratch; then their parts inside the windows
    ok = ok && c->decode_chunks(in, w.c, E, w.scratch);
    if (ok) {
        hipLaunchKernelGGL(k_fr_trim, dim3(E), dim3(256), 0, s, w.c, w.e, w.w, w.scratch, out, out_off);
        hipLaunchKernelGGL(k_fr_verdict, dim3(groups), dim3(256), 0, s, ns, w.st, w.w, w.e, w.c, out_len, status, d_result);
        ok = c->check(hipGetLastError(), "frame range verdict");
    }
    return ok ? SNP_OK : SNP_ERR_DEVICE;
}

}  // extern "C"

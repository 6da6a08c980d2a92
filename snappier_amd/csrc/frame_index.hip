// frame_index.hip -- snp_frame_index_batch and snp_frame_read_indexed_batch: many framed streams walked ONCE into a chunk index the caller keeps
// (16 bytes per data chunk: the decoded bytes before it and where its header is), then any number of windows, each naming a stream, read in
// one call with no header walk.  The range decode (frame_range.hip) walks every stream from byte 0 in every call and takes one window per
// stream; its walk is most of a narrow window's time on long streams.  Built into libsnappier_hip_frame_index.so (C-ABI:
// include/snappier_hip_frame_index.h), linked against libsnappier_hip.so.  DESIGN.md 4.14.
//
// index:  scan      ceil(in_len / 2^20) -> each stream's first span slot (d_result[2])
//         A, B      the span walk (frame_walk_device.h) with no capacity bound, as the layout call makes it
//         scans     the chunks every walked stream lists -> rows needed (d_result[0]); those of the streams that fit both bounds -> idx_first
//         streams   one thread per stream: idx_total, idx_tail
//         rows      one wavefront per span slot: the span's data chunks (for_span_chunks) -> idx_start, idx_pos
// read:   plan      one thread per request: the clip, the capacity, two binary searches in the index, the check of its edge rows against the
//                   headers they point at (frame_index_device.h: the index is untrusted), its edge slots, its count of interior rows
//         scans     interior counts over the requests -> each request's first slot (d_result[0]); over the edge slots, the decoded sizes ->
//                   each edge's place in the scratch arena (d_result[2]), and the slots in use -> each edge's row in the compact edge table
//         admit     one thread per request: interior slots and edge bytes within their bounds -> its edges' rows
//         rows      one thread per interior slot: its request (owner_of), the check of its row, the row of the chunk table; void: the rows of
//                   a request with a row that failed its check are emptied again, so nothing of it is decoded
//         decode    snp_ctx::decode_chunks over the interior table into `out`, and over the edge table into scratch
//         trim, fail, verdict   as in the range decode (frame_edges_device.h)
// Nothing here allocates, reads back or synchronises: both calls are capturable like the other _batch entry points.
#include "capi_internal.h"
#include "frame_walk_device.h"
#include "frame_edges_device.h"
#include "frame_index_device.h"
#include "../../include/snappier_hip_frame_index.h"

namespace {

// ---- the index ---------------------------------------------------------------------------------------------------------------------------------
// scan source: the rows of the streams that fit both bounds (admission is in stream order: both sums only grow)
struct ScanIndexedRows {
    const u64* __restrict__ sfirst;
    const u64* __restrict__ need;       // the scan of what every walked stream lists
    const u32* __restrict__ nc;
    u32 max_spans;
    u64 max_entries;
    __device__ __forceinline__ bool indexed(u64 b) const { return sfirst[b + 1] <= max_spans && need[b + 1] <= max_entries; }
    __device__ __forceinline__ u64 operator()(u64 b) const { return indexed(b) ? nc[b] : 0; }
};

__global__ __launch_bounds__(256) void k_ix_streams(u32 ns, ScanIndexedRows a, FbStreams st, u64* __restrict__ idx_total, i32* __restrict__ idx_tail,
                                                   u64* __restrict__ result)
{
    const u32 b = blockIdx.x * 256u + threadIdx.x;
    u64 total = 0;
    if (b < ns) {
        const bool in = a.indexed(b);
        total = in ? st.total[b] : 0;
        idx_total[b] = total;
        idx_tail[b] = in ? st.tail[b] : SNP_ERR_OUTPUT_TOO_SMALL;
    }
    total = wave_sum(total);
    if ((threadIdx.x & 63u) == 0 && total) atomic_add64(result + 1, total);
}

// One wavefront per span slot; lane 0 hops, as in k_fd_emit.  Row idx_first[b] + idx < idx_first[b + 1] <= max_entries: the hops end at the
// stream's chunk count.
__global__ __launch_bounds__(SNP_WAVE) void k_ix_index_rows(const u8* __restrict__ in, const u64* __restrict__ in_off, const u64* __restrict__ in_len,
                                                           u32 ns, ScanIndexedRows a, FbSpans t, FbStreams st, const u64* __restrict__ idx_first,
                                                           u64* __restrict__ idx_start, u64* __restrict__ idx_pos)
{
    const u32 g = blockIdx.x;
    if (lane_id() != 0 || g >= a.sfirst[ns]) return;
    const u32 b = owner_of(a.sfirst, ns, g);
    if (!a.indexed(b) || t.entry[g] == kNoEntry) return;
    const u64 row0 = idx_first[b];
    for_span_chunks(in + in_off[b], in_len[b], t.entry[g], (g - a.sfirst[b] + 1) * kSpan, t.chunk_base[g], st.nc[b], t.out_base[g],
                    [&](const Hop&, u64 ip, u32 idx, u64 off) {
                        idx_start[row0 + idx] = off;
                        idx_pos[row0 + idx] = ip;
                        return true;
                    });
}

// workspace: first span slot and rows needed before every stream (ns + 1 each), the tile sums of their scans, the walk's record; per span slot
// the candidates and the resolver's entry
struct IndexWork {
    u64 *sfirst, *need, *part;
    FbStreams st;
    FbSpans sp;
    u64 bytes;
};
IndexWork index_work_layout(void* base, u32 nstreams, u32 max_spans)
{
    IndexWork w{};
    if (nstreams == 0) return w;
    const u64 ns = nstreams;
    WorkCarver k(base);
    w.sfirst = k.take<u64>(ns + 1);
    w.need = k.take<u64>(ns + 1);
    w.part = k.take<u64>(scan_tiles_of(ns));
    carve_span_walk(k, ns, max_spans, w.st, w.sp);
    w.bytes = k.bytes();
    return w;
}

// ---- the indexed read --------------------------------------------------------------------------------------------------------------------------
constexpr u32 kSmall = 1u;              // flags: hi - lo > out_cap (nothing is selected)
constexpr u32 kAdmitted = 2u;           // flags: planned, and interior slots and edge bytes fit
constexpr u32 kFits = 4u;               // flags: interior slots and edge bytes fit (whatever the plan says)
constexpr u32 kBad = 8u;                // flags: an interior row failed its check
constexpr u32 kHead = 16u;              // flags: the request's first row is its head edge
constexpr u32 kPlanShift = 8;           // flags >> 8: the plan's status

// per request
struct IxRequests {
    u64 *lo, *hi;       // the clipped window
    u64* row0;          // its first owned row in the index
    u64* fail;          // min over the failing interior rows of fail_key(place in the request, status)
    u64* icount;        // interior rows
    u32* flags;
};

struct ReadArgs {
    const u8* in;
    const u64 *in_off, *in_len;
    u32 ns;
    FrameIndex x;
    const u32* req_stream;
    const u64 *req_off, *req_len;
    u32 nreq;
    const u64 *out_off, *out_cap;
};

struct ScanWords {
    const u64* __restrict__ src;
    __device__ __forceinline__ u64 operator()(u64 i) const { return src[i]; }
};

__global__ __launch_bounds__(256) void k_ix_plan(ReadArgs a, IxRequests q, FrEdges e, ChunkRows c)
{
    const u32 r = blockIdx.x * 256u + threadIdx.x;
    if (r >= a.nreq) return;
    const u32 b = a.req_stream[r];
    IxPlan k = ix_plan(a.x, a.ns, b, a.req_off[r], a.req_len[r], a.out_cap[r]);
    const u64 head = 2ull * r, tail = head + 1;
    e.dec[head] = 0;
    e.dec[tail] = 0;
    for (u64 row = head; row <= tail; ++row) {
        c.tag[row] = kNone;
        chunk_row_clear(c, row, 0);
    }
    u64 cnt = 0;
    if (k.status == SNP_OK && k.r0 < k.r1) {
        const u8* const p = a.in + a.in_off[b];
        const u64 n = a.in_len[b];
        Hop hh{}, ht{};
        const bool good = (!k.head || ix_row_check(a.x, p, n, k, k.r0, false, &hh)) && (!k.last || ix_row_check(a.x, p, n, k, k.r1 - 1, false, &ht));
        if (good) {
            if (k.head) edge_slot_set(e, head, hh, a.in_off[b] + a.x.pos[k.r0], a.x.start[k.r0]);
            if (k.last) edge_slot_set(e, tail, ht, a.in_off[b] + a.x.pos[k.r1 - 1], a.x.start[k.r1 - 1]);
            cnt = k.interior();
        } else {
            k.status = SNP_ERR_BAD_ARG;
        }
    }
    q.lo[r] = k.lo;
    q.hi[r] = k.hi;
    q.row0[r] = k.r0;
    q.fail[r] = kNoFail;
    q.icount[r] = cnt;
    q.flags[r] = (k.small ? kSmall : 0u) | (k.head ? kHead : 0u) | (static_cast<u32>(k.status) << kPlanShift);
}

// Admission (in request order: both sums only grow), the rows of the admitted requests' edges, d_result[2] and [3].
__global__ __launch_bounds__(256) void k_ix_admit(u32 nreq, const u64* __restrict__ ifirst, u32 max_chunks, u64 edge_cap, IxRequests q, FrEdges e,
                                                 ChunkRows c, u64* __restrict__ result)
{
    const u32 r = blockIdx.x * 256u + threadIdx.x;
    if (r >= nreq) return;
    if (r == 0) { result[2] = e.place[2ull * nreq]; result[3] = 0; }
    if (ifirst[r + 1] > max_chunks || e.place[2ull * r + 2] > edge_cap) return;
    const bool planned = (q.flags[r] >> kPlanShift) == SNP_OK;
    q.flags[r] |= planned ? kFits | kAdmitted : kFits;
    if (!planned) return;
    for (u64 slot = 2ull * r; slot < 2ull * r + 2; ++slot)
        if (e.dec[slot]) edge_row_place(c, e, slot);
}

// the stream-side half of a request's plan again, for the check of one row
__device__ __forceinline__ IxPlan plan_of(const ReadArgs& a, const IxRequests& q, u32 r, u32 b)
{
    IxPlan k{};
    k.lo = q.lo[r];
    k.hi = q.hi[r];
    k.f1 = a.x.first[b + 1] < a.x.nentries ? a.x.first[b + 1] : a.x.nentries;
    k.total = a.x.total[b];
    return k;
}

// One thread per interior slot: an empty row unless the slot belongs to an admitted request and its index row passes the check.
__global__ __launch_bounds__(256) void k_ix_rows(ReadArgs a, IxRequests q, const u64* __restrict__ ifirst, u32 max_chunks, ChunkRows rows)
{
    const u32 c = blockIdx.x * 256u + threadIdx.x;
    if (c >= max_chunks) return;
    rows.tag[c] = kNone;
    chunk_row_clear(rows, c, 0);
    if (c >= ifirst[a.nreq]) return;
    const u32 r = owner_of(ifirst, a.nreq, c);
    const u32 flags = q.flags[r];
    if (!(flags & kAdmitted)) return;
    const u32 b = a.req_stream[r];                                      // (< ns: the request was planned)
    const IxPlan k = plan_of(a, q, r, b);
    const u64 i = q.row0[r] + (flags & kHead ? 1 : 0) + (c - ifirst[r]);
    Hop h{};
    if (i >= k.f1 || !ix_row_check(a.x, a.in + a.in_off[b], a.in_len[b], k, i, true, &h)) {
        atomicOr(q.flags + r, kBad);
        return;
    }
    if (h.dec == 0) return;                                             // a zero-length chunk keeps its slot, empty: it is never decoded or verified
    rows.tag[c] = r;
    chunk_row_set(rows, c, h, a.in_off[b] + a.x.pos[i], a.out_off[r] + (a.x.start[i] - k.lo));
}

// the rows of a request with a row that failed its check, emptied again: interior slots, then the edge table
__global__ __launch_bounds__(256) void k_ix_void(u32 max_chunks, u32 nedges, IxRequests q, ChunkRows rows, ChunkRows c)
{
    const u32 t = blockIdx.x * 256u + threadIdx.x;
    if (t < max_chunks) {
        const u32 r = rows.tag[t];
        if (r != kNone && (q.flags[r] & kBad)) {
            rows.tag[t] = kNone;
            chunk_row_clear(rows, t, 0);
        }
    }
    if (t < nedges) {
        const u32 slot = c.tag[t];
        if (slot != kNone && (q.flags[slot >> 1] & kBad)) {
            c.tag[t] = kNone;
            chunk_row_clear(c, t, 0);
        }
    }
}

// One workgroup per edge row (edge_trim).
__global__ __launch_bounds__(256) void k_ix_trim(ChunkRows c, FrEdges e, IxRequests q, const u8* __restrict__ scratch, u8* __restrict__ out,
                                                const u64* __restrict__ out_off)
{
    const u64 row = blockIdx.x;
    const u32 slot = c.tag[row];
    if (slot == kNone) return;
    const u32 r = slot >> 1;
    edge_trim(c, e, row, slot, q.lo[r], q.hi[r], scratch, out + out_off[r], threadIdx.x);
}

// the failing interior rows, keyed by the row's place in its request
__global__ __launch_bounds__(256) void k_ix_fail(u32 max_chunks, ChunkRows rows, const u64* __restrict__ ifirst, IxRequests q)
{
    const u32 c = blockIdx.x * 256u + threadIdx.x;
    if (c >= max_chunks) return;
    const u32 r = rows.tag[c];
    if (r == kNone || rows.status[c] == SNP_OK) return;
    atomic_min64(q.fail + r, fail_key(c - ifirst[r], rows.status[c]));
}

// The request's status: a bound missed, else what the plan refused, else a row that failed its check, else the verdict of the range decode
// over the chunks it selected.  result[1] += the OK lengths, result[3] += the OK requests (one atomic per wavefront each).
__global__ __launch_bounds__(256) void k_ix_verdict(ReadArgs a, IxRequests q, FrEdges e, ChunkRows c, u64* __restrict__ out_len, i32* __restrict__ status,
                                                   u64* __restrict__ result)
{
    const u32 r = blockIdx.x * 256u + threadIdx.x;
    u64 ok_len = 0, ok = 0;
    if (r < a.nreq) {
        i32 s = SNP_ERR_OUTPUT_TOO_SMALL;
        const u32 flags = q.flags[r];
        if (flags & kFits) {
            s = static_cast<i32>(flags >> kPlanShift);
            if (s == SNP_OK && (flags & kBad)) s = SNP_ERR_BAD_ARG;
            else if (s == SNP_OK)
                s = window_verdict(edge_status(c, e, 2ull * r), q.fail[r], edge_status(c, e, 2ull * r + 1), a.x.tail[a.req_stream[r]], flags & kSmall);
            if (s == SNP_OK) { ok_len = q.hi[r] - q.lo[r]; ok = 1; }
        }
        status[r] = s;
        out_len[r] = ok_len;
    }
    ok_len = wave_sum(ok_len);
    ok = wave_sum(ok);
    if ((threadIdx.x & 63u) == 0 && ok) {
        atomic_add64(result + 3, ok);
        if (ok_len) atomic_add64(result + 1, ok_len);
    }
}

// workspace: per request its first interior slot (nreq + 1), the window, the plan's words, two edge slots and two rows of the edge table; the
// tile sums of the scans; per chunk slot the interior chunk table; then edge_cap bytes of scratch
struct ReadWork {
    u64 *ifirst, *part;
    IxRequests q;
    ChunkRows r;         // interior rows
    FrEdges e;
    ChunkRows c;         // edge rows
    u8* scratch;
    u64 bytes;
};
ReadWork read_work_layout(void* base, u32 nreq, u32 max_chunks, u64 edge_cap)
{
    ReadWork k{};
    if (nreq == 0) return k;
    const u64 nr = nreq, ne = 2 * nr;
    WorkCarver c(base);
    k.ifirst = c.take<u64>(nr + 1);
    k.part = c.take<u64>(scan_tiles_of(ne));
    k.q.lo = c.take<u64>(nr);
    k.q.hi = c.take<u64>(nr);
    k.q.row0 = c.take<u64>(nr);
    k.q.fail = c.take<u64>(nr);
    k.q.icount = c.take<u64>(nr);
    k.q.flags = c.take<u32>(nr);
    k.r = carve_chunk_rows(c, max_chunks);
    k.e = carve_edges(c, ne);
    k.c = carve_chunk_rows(c, ne);
    k.scratch = c.take<u8>(edge_cap);
    k.bytes = c.bytes();
    return k;
}

}  // namespace

extern "C" {

uint64_t snp_frame_index_workspace(uint32_t nstreams, uint32_t max_spans)
{
    return index_work_layout(nullptr, nstreams, max_spans).bytes;
}

snp_status snp_frame_index_batch(snp_ctx* c, const uint8_t* in, const uint64_t* in_off, const uint64_t* in_len, uint32_t nstreams,
                                 uint32_t max_spans, uint64_t max_entries, uint64_t* idx_first, uint64_t* idx_start, uint64_t* idx_pos,
                                 uint64_t* idx_total, int32_t* idx_tail, void* d_work, uint64_t* d_result)
{
    if (!c || !d_result || (nstreams && (!in || !in_off || !in_len || !idx_first || !idx_total || !idx_tail || !d_work)) ||
        (nstreams && max_entries && (!idx_start || !idx_pos)))
        return SNP_ERR_BAD_ARG;
    DevGuard dg(c);
    if (!dg.ok) return SNP_ERR_DEVICE;
    hipStream_t s = c->stream;
    if (nstreams == 0)
        return c->check(snp_zero_words_async(reinterpret_cast<u32*>(d_result), 2 * 4, s), "frame index result") ? SNP_OK : SNP_ERR_DEVICE;
    const IndexWork w = index_work_layout(d_work, nstreams, max_spans);
    const u32 ns = nstreams, S = max_spans, groups = static_cast<u32>((static_cast<u64>(ns) + 255) / 256);
    const ScanIndexedRows rows{w.sfirst, w.need, w.st.nc, S, max_entries};
    // the span walk (d_result[2] = span slots needed, [3] = spans resolved on the spot), the rows the walked streams list (d_result[0], [1] = 0:
    // a stream that was not walked lists none), the first row of every stream that fits
    bool ok = c->check(launch_span_scan(in_len, ns, w.part, w.sfirst, d_result + 2, s), "frame index span scan") &&
              c->check(launch_span_walk(in, in_off, in_len, nullptr, ns, w.sfirst, S, w.sp, w.st, d_result + 3, s), "frame index walk") &&
              c->check(launch_scan(ScanPlain{w.st.nc}, ns, w.part, w.need, d_result, s), "frame index need scan") &&
              c->check(launch_scan(rows, ns, w.part, idx_first, nullptr, s), "frame index row scan");
    if (ok) {
        hipLaunchKernelGGL(k_ix_streams, dim3(groups), dim3(256), 0, s, ns, rows, w.st, idx_total, idx_tail, d_result);
        if (S && max_entries)
            hipLaunchKernelGGL(k_ix_index_rows, dim3(S), dim3(SNP_WAVE), 0, s, in, in_off, in_len, ns, rows, w.sp, w.st, idx_first, idx_start, idx_pos);
        ok = c->check(hipGetLastError(), "frame index rows");
    }
    return ok ? SNP_OK : SNP_ERR_DEVICE;
}

uint64_t snp_frame_read_indexed_workspace(uint32_t nreq, uint32_t max_chunks, uint64_t edge_cap)
{
    return read_work_layout(nullptr, nreq, max_chunks, edge_cap).bytes;
}

snp_status snp_frame_read_indexed_batch(snp_ctx* c, const uint8_t* in, const uint64_t* in_off, const uint64_t* in_len, uint32_t nstreams,
                                        const uint64_t* idx_first, const uint64_t* idx_start, const uint64_t* idx_pos, const uint64_t* idx_total,
                                        const int32_t* idx_tail, uint64_t nentries, const uint32_t* req_stream, const uint64_t* req_off,
                                        const uint64_t* req_len, uint32_t nreq, uint32_t max_chunks, uint64_t edge_cap, uint8_t* out,
                                        const uint64_t* out_off, const uint64_t* out_cap, uint64_t* out_len, int32_t* status, void* d_work,
                                        uint64_t* d_result)
{
    if (!c || !d_result || nreq > 0x3fffffffu ||   // (one workgroup per edge row: 2 x nreq must be a grid)
        (nreq && (!req_stream || !req_off || !req_len || !out || !out_off || !out_cap || !out_len || !status || !d_work)) ||
        (nreq && nstreams && (!in || !in_off || !in_len || !idx_first || !idx_total || !idx_tail)) ||
        (nreq && nstreams && nentries && (!idx_start || !idx_pos)))
        return SNP_ERR_BAD_ARG;
    DevGuard dg(c);
    if (!dg.ok) return SNP_ERR_DEVICE;
    hipStream_t s = c->stream;
    if (nreq == 0)
        return c->check(snp_zero_words_async(reinterpret_cast<u32*>(d_result), 2 * 4, s), "frame read result") ? SNP_OK : SNP_ERR_DEVICE;
    const ReadWork w = read_work_layout(d_work, nreq, max_chunks, edge_cap);
    const u32 M = max_chunks, E = 2 * nreq, groups = (nreq + 255u) / 256u;
    const ReadArgs a{in, in_off, in_len, nstreams, FrameIndex{idx_first, idx_start, idx_pos, idx_total, idx_tail, nentries},
                     req_stream, req_off, req_len, nreq, out_off, out_cap};
    hipLaunchKernelGGL(k_ix_plan, dim3(groups), dim3(256), 0, s, a, w.q, w.e, w.c);
    // first interior slot of every request (d_result[0] = slots needed, d_result[1] = 0), every edge's place in the scratch arena, admission
    bool ok = c->check(hipGetLastError(), "frame read plan") &&
              c->check(launch_scan(ScanWords{w.q.icount}, nreq, w.part, w.ifirst, d_result, s), "frame read slot scan") &&
              c->check(launch_scan(ScanEdgeBytes{w.e.dec}, E, w.part, w.e.place, nullptr, s), "frame read edge scan") &&
              c->check(launch_scan(ScanEdgeCount{w.e.dec}, E, w.part, w.e.rank, nullptr, s), "frame read edge rank scan");
    if (ok) {
        hipLaunchKernelGGL(k_ix_admit, dim3(groups), dim3(256), 0, s, nreq, w.ifirst, M, edge_cap, w.q, w.e, w.c, d_result);
        if (M) hipLaunchKernelGGL(k_ix_rows, dim3((M + 255u) / 256u), dim3(256), 0, s, a, w.q, w.ifirst, M, w.r);
        const u32 widest = M > E ? M : E;
        hipLaunchKernelGGL(k_ix_void, dim3((widest + 255u) / 256u), dim3(256), 0, s, M, E, w.q, w.r, w.c);
        ok = c->check(hipGetLastError(), "frame read table");
    }
    if (ok && M) {
        // decode + CRC verify of every interior slot, straight into out
        ok = c->decode_chunks(in, w.r, M, out);
        if (ok) hipLaunchKernelGGL(k_ix_fail, dim3((M + 255u) / 256u), dim3(256), 0, s, M, w.r, w.ifirst, w.q);
    }
    // the edges, whole, into scratch; then their parts inside the windows
    ok = ok && c->decode_chunks(in, w.c, E, w.scratch);
    if (ok) {
        hipLaunchKernelGGL(k_ix_trim, dim3(E), dim3(256), 0, s, w.c, w.e, w.q, w.scratch, out, out_off);
        hipLaunchKernelGGL(k_ix_verdict, dim3(groups), dim3(256), 0, s, a, w.q, w.e, w.c, out_len, status, d_result);
        ok = c->check(hipGetLastError(), "frame read verdict");
    }
    return ok ? SNP_OK : SNP_ERR_DEVICE;
}

}  // extern "C"

// frame_digest.hip -- snp_frame_digest_indexed_batch: the CRC-32C of any number of windows of what seekable framed streams decode to, WITHOUT
// decoding them.  Every data chunk header carries the masked CRC-32C of the chunk's decoded bytes, and CRC is GF(2)-linear: a window's digest is
// the XOR of its chunks' CRCs, each multiplied by x^(8 x the bytes behind it) (frame_digest_device.h).  An interior chunk costs one header read
// and one modular multiplication; only the at most two chunks a window cuts are decoded.  The digest does not depend on the chunk grid, so
// streams that were spliced, rechunked or composed differently compare by content.  Built into libsnappier_hip_frame_digest.so (C-ABI:
// include/snappier_hip_frame_digest.h), linked against libsnappier_hip.so.  DESIGN.md 4.22.
//
//   plan      one thread per request: the indexed read's plan with no capacity (dg_plan: ix_plan, ix_row_check on the edge rows), its edge
//             slots, its count of interior rows; digest[r] = 0
//   scans     ceil(interior rows / 64) over the requests -> each request's first WORK ITEM; over the edge slots, the decoded sizes -> each
//             edge's place in the scratch arena (d_result[2]), and the slots in use -> each edge's row in the compact edge table
//   admit     one thread per request: its edge bytes within edge_cap -> its edges' rows
//   rows      a chip-full of wavefronts, each striding over the work items: its request by owner_of (the inverse of the scan), 64 rows, one
//             header read and one crc_shift per lane, XOR across the wavefront, one atomicXor into digest[r].  Rows are balanced, not
//             requests: one request may own a million rows and a batch may hold a million requests of one row.
//   decode    snp_ctx::decode_chunks over the edge table into scratch, as the read does it
//   ranges    one thread per edge row: the part of the edge inside its window; crc: snp_launch_crc32c over those ranges of the scratch
//   verdict   one thread per request: the read's status precedence; an OK request XORs its edges' shifted CRCs in; any other gets 0
// Nothing here allocates, reads back or synchronises: the call is capturable like the other _batch entry points.  No per-row table exists.
#include "capi_internal.h"
#include "scan_tiles.h"
#include "frame_edges_device.h"
#include "frame_digest_device.h"
#include "../../include/snappier_hip_frame_digest.h"

namespace {

constexpr u32 kAdmitted = 2u;           // flags: planned, and the edge bytes fit
constexpr u32 kFits = 4u;               // flags: the edge bytes fit (whatever the plan says)
constexpr u32 kBad = 8u;                // flags: an interior row failed its check
constexpr u32 kHead = 16u;              // flags: the request's first row is its head edge
constexpr u32 kPlanShift = 8;           // flags >> 8: the plan's status

// per request
struct DgRequests {
    u64 *lo, *hi;       // the clipped window
    u64* row0;          // its first owned row in the index
    u64* icount;        // interior rows
    u32* flags;
};

struct DigestArgs {
    const u8* in;
    const u64 *in_off, *in_len;
    u32 ns;
    FrameIndex x;
    const u32* req_stream;
    const u64 *req_off, *req_len;
    u32 nreq;
};

// scan source: the work items of a request (kDigestRows interior rows each)
struct ScanWorkItems {
    const u64* __restrict__ icount;
    __device__ __forceinline__ u64 operator()(u64 r) const { return (icount[r] + kDigestRows - 1) / kDigestRows; }
};

__global__ __launch_bounds__(256) void k_dg_plan(DigestArgs a, DgRequests q, FrEdges e, ChunkRows c, u32* __restrict__ digest)
{
    const u32 r = blockIdx.x * 256u + threadIdx.x;
    if (r >= a.nreq) return;
    const u32 b = a.req_stream[r];
    const DgPlan d = dg_plan(a.x, a.in, a.in_off, a.in_len, a.ns, b, a.req_off[r], a.req_len[r]);
    const u64 head = 2ull * r, tail = head + 1;
    e.dec[head] = 0;
    e.dec[tail] = 0;
    for (u64 row = head; row <= tail; ++row) {
        c.tag[row] = kNone;
        chunk_row_clear(c, row, 0);
    }
    if (d.k.status == SNP_OK) {
        if (d.k.head) edge_slot_set(e, head, d.hh, a.in_off[b] + a.x.pos[d.k.r0], a.x.start[d.k.r0]);
        if (d.k.last) edge_slot_set(e, tail, d.ht, a.in_off[b] + a.x.pos[d.k.r1 - 1], a.x.start[d.k.r1 - 1]);
    }
    q.lo[r] = d.k.lo;
    q.hi[r] = d.k.hi;
    q.row0[r] = d.k.r0;
    q.icount[r] = d.interior;
    q.flags[r] = (d.k.head ? kHead : 0u) | (static_cast<u32>(d.k.status) << kPlanShift);
    digest[r] = 0;
}

// Admission (in request order: the sum only grows), the rows of the admitted requests' edges, d_result.
__global__ __launch_bounds__(256) void k_dg_admit(u32 nreq, u64 edge_cap, DgRequests q, FrEdges e, ChunkRows c, u64* __restrict__ result)
{
    const u32 r = blockIdx.x * 256u + threadIdx.x;
    if (r >= nreq) return;
    if (r == 0) { result[0] = 0; result[1] = 0; result[2] = e.place[2ull * nreq]; result[3] = 0; }
    if (e.place[2ull * r + 2] > edge_cap) return;
    const bool planned = (q.flags[r] >> kPlanShift) == SNP_OK;
    q.flags[r] |= planned ? kFits | kAdmitted : kFits;
    if (!planned) return;
    for (u64 slot = 2ull * r; slot < 2ull * r + 2; ++slot)
        if (e.dec[slot]) edge_row_place(c, e, slot);
}

__device__ __forceinline__ u32 wave_xor(u32 v)
{
    for (u32 d = 32; d >= 1; d >>= 1) v ^= __shfl_xor(v, d, 64);
    return v;
}

// The interior rows.  nwaves wavefronts stride over the work items wfirst[nreq] counts (known on the device only: the grid is a chip-full, or
// fewer when the host's bound on the items is smaller).  Work item w of request r = its interior rows [64 j, 64 j + 64), j = w - wfirst[r].
__global__ __launch_bounds__(256) void k_dg_rows(DigestArgs a, DgRequests q, const u64* __restrict__ wfirst, u32 nwaves, u32* __restrict__ digest)
{
    const u32 lane = lane_id();
    const u64 items = wfirst[a.nreq];
    for (u64 w = blockIdx.x * 4u + (threadIdx.x >> 6); w < items; w += nwaves) {
        const u32 r = bcast_first(owner_of(wfirst, a.nreq, w));
        const u32 flags = q.flags[r];
        if (!(flags & kAdmitted)) continue;                             // (wave-uniform)
        const u32 b = a.req_stream[r];                                  // (< ns: the request was planned)
        IxPlan k{};                                                     // the stream-side half of the request's plan again, for the row check
        k.lo = q.lo[r];
        k.hi = q.hi[r];
        k.f1 = a.x.first[b + 1] < a.x.nentries ? a.x.first[b + 1] : a.x.nentries;
        k.total = a.x.total[b];
        const u64 j = (w - wfirst[r]) * kDigestRows + lane;
        u32 term = 0;
        bool bad = false;
        if (j < q.icount[r]) bad = !dg_row_term(a.x, a.in + a.in_off[b], a.in_len[b], k, q.row0[r] + (flags & kHead ? 1 : 0) + j, &term);
        term = wave_xor(term);
        const bool any_bad = ballot64(bad) != 0;
        if (lane == 0) {
            if (any_bad) atomicOr(q.flags + r, kBad);
            else if (term) atomicXor(digest + r, term);
        }
    }
}

// One thread per row of the compact edge table: the bytes of a decoded edge inside its window, as a range of the scratch for the CRC launch
// (an empty row, or an edge that failed, gives an empty range: the CRC of nothing is 0).
__global__ __launch_bounds__(256) void k_dg_ranges(u32 nedges, ChunkRows c, FrEdges e, DgRequests q, u64* __restrict__ crc_off, u32* __restrict__ crc_len)
{
    const u32 row = blockIdx.x * 256u + threadIdx.x;
    if (row >= nedges) return;
    const u32 slot = c.tag[row];
    u64 off = 0;
    u32 len = 0;
    if (slot != kNone && c.status[row] == SNP_OK && c.out_len[row] == c.out_cap[row]) {
        const u32 r = slot >> 1;
        const u64 s = e.start[slot];
        u64 from, to;
        dg_edge_part(s, c.out_cap[row], q.lo[r], q.hi[r], &from, &to);
        off = c.out_off[row] + (from - s);
        len = static_cast<u32>(to - from);
    }
    crc_off[row] = off;
    crc_len[row] = len;
}

// The request's status: the edge bound missed, else what the plan refused, else a row that failed its check, else the verdict of the read over
// its edges and the stream's tail (no interior row is decoded, so none can fail).  An OK request takes its edges' terms; any other gets 0.
// result[0] += interior rows combined, [1] += the OK lengths, [3] += the OK requests (one atomic per wavefront each).
__global__ __launch_bounds__(256) void k_dg_verdict(DigestArgs a, DgRequests q, FrEdges e, ChunkRows c, const u32* __restrict__ edge_crc,
                                                   u32* __restrict__ digest, u64* __restrict__ dig_len, i32* __restrict__ status, u64* __restrict__ result)
{
    const u32 r = blockIdx.x * 256u + threadIdx.x;
    u64 ok_len = 0, ok = 0, rows = 0;
    if (r < a.nreq) {
        i32 s = SNP_ERR_OUTPUT_TOO_SMALL;
        const u32 flags = q.flags[r];
        u32 dg = 0;
        if (flags & kFits) {
            s = static_cast<i32>(flags >> kPlanShift);
            if (s == SNP_OK && (flags & kBad)) s = SNP_ERR_BAD_ARG;
            else if (s == SNP_OK)
                s = window_verdict(edge_status(c, e, 2ull * r), kNoFail, edge_status(c, e, 2ull * r + 1), a.x.tail[a.req_stream[r]], false);
            if (s == SNP_OK) {
                const u64 lo = q.lo[r], hi = q.hi[r];
                dg = digest[r];
                for (u64 slot = 2ull * r; slot < 2ull * r + 2; ++slot) {
                    if (!e.dec[slot]) continue;
                    u64 from, to;
                    dg_edge_part(e.start[slot], e.dec[slot], lo, hi, &from, &to);
                    dg ^= crc_shift(edge_crc[e.rank[slot]], hi - to);
                }
                ok_len = hi - lo;
                ok = 1;
                rows = q.icount[r];
            }
        }
        status[r] = s;
        dig_len[r] = ok_len;
        digest[r] = dg;
    }
    ok_len = wave_sum(ok_len);
    ok = wave_sum(ok);
    rows = wave_sum(rows);
    if ((threadIdx.x & 63u) == 0 && ok) {
        atomic_add64(result + 3, ok);
        if (ok_len) atomic_add64(result + 1, ok_len);
        if (rows) atomic_add64(result + 0, rows);
    }
}

// workspace: per request its first work item (nreq + 1), the window, the plan's words, two edge slots and two rows of the edge table with
// their CRC range and CRC; the tile sums of the scans; then edge_cap bytes of scratch.  Nothing per interior row.
struct DigestWork {
    u64 *wfirst, *part;
    DgRequests q;
    FrEdges e;
    ChunkRows c;         // edge rows
    u64* crc_off;
    u32 *crc_len, *crc;
    u8* scratch;
    u64 bytes;
};
DigestWork digest_work_layout(void* base, u32 nreq, u64 edge_cap)
{
    DigestWork k{};
    if (nreq == 0) return k;
    const u64 nr = nreq, ne = 2 * nr;
    WorkCarver c(base);
    k.wfirst = c.take<u64>(nr + 1);
    k.part = c.take<u64>(scan_tiles_of(ne));
    k.q.lo = c.take<u64>(nr);
    k.q.hi = c.take<u64>(nr);
    k.q.row0 = c.take<u64>(nr);
    k.q.icount = c.take<u64>(nr);
    k.q.flags = c.take<u32>(nr);
    k.e = carve_edges(c, ne);
    k.c = carve_chunk_rows(c, ne);
    k.crc_off = c.take<u64>(ne);
    k.crc_len = c.take<u32>(ne);
    k.crc = c.take<u32>(ne);
    k.scratch = c.take<u8>(edge_cap);
    k.bytes = c.bytes();
    return k;
}

}  // namespace

extern "C" {

uint32_t snp_crc32c_combine(uint32_t crc_a, uint32_t crc_b, uint64_t len_b)
{
    return crc_combine(crc_a, crc_b, len_b);
}

uint64_t snp_frame_digest_indexed_workspace(uint32_t nreq, uint64_t edge_cap)
{
    return digest_work_layout(nullptr, nreq, edge_cap).bytes;
}

snp_status snp_frame_digest_indexed_batch(snp_ctx* c, const uint8_t* in, const uint64_t* in_off, const uint64_t* in_len, uint32_t nstreams,
                                          const uint64_t* idx_first, const uint64_t* idx_start, const uint64_t* idx_pos, const uint64_t* idx_total,
                                          const int32_t* idx_tail, uint64_t nentries, const uint32_t* req_stream, const uint64_t* req_off,
                                          const uint64_t* req_len, uint32_t nreq, uint64_t edge_cap, uint32_t* digest, uint64_t* dig_len,
                                          int32_t* status, void* d_work, uint64_t* d_result)
{
    if (!c || !d_result || nreq > 0x3fffffffu ||   // (two edge rows per request: 2 x nreq must be a row count)
        (nreq && (!req_stream || !req_off || !req_len || !digest || !dig_len || !status || !d_work)) ||
        (nreq && nstreams && (!in || !in_off || !in_len || !idx_first || !idx_total || !idx_tail)) ||
        (nreq && nstreams && nentries && (!idx_start || !idx_pos)))
        return SNP_ERR_BAD_ARG;
    DevGuard dg(c);
    if (!dg.ok) return SNP_ERR_DEVICE;
    hipStream_t s = c->stream;
    if (nreq == 0)
        return c->check(snp_zero_words_async(reinterpret_cast<u32*>(d_result), 2 * 4, s), "frame digest result") ? SNP_OK : SNP_ERR_DEVICE;
    const DigestWork w = digest_work_layout(d_work, nreq, edge_cap);
    const u32 E = 2 * nreq, groups = (nreq + 255u) / 256u;
    const DigestArgs a{in, in_off, in_len, nstreams, FrameIndex{idx_first, idx_start, idx_pos, idx_total, idx_tail, nentries},
                       req_stream, req_off, req_len, nreq};
    hipLaunchKernelGGL(k_dg_plan, dim3(groups), dim3(256), 0, s, a, w.q, w.e, w.c, digest);
    // first work item of every request, every edge's place in the scratch arena and its row in the edge table, admission
    bool ok = c->check(hipGetLastError(), "frame digest plan") &&
              c->check(launch_scan(ScanWorkItems{w.q.icount}, nreq, w.part, w.wfirst, nullptr, s), "frame digest work scan") &&
              c->check(launch_scan(ScanEdgeBytes{w.e.dec}, E, w.part, w.e.place, nullptr, s), "frame digest edge scan") &&
              c->check(launch_scan(ScanEdgeCount{w.e.dec}, E, w.part, w.e.rank, nullptr, s), "frame digest edge rank scan");
    if (ok) {
        hipLaunchKernelGGL(k_dg_admit, dim3(groups), dim3(256), 0, s, nreq, edge_cap, w.q, w.e, w.c, d_result);
        // the work items are counted on the device; the host bounds them by (rows / 64 + 1) per request and launches a chip-full at most
        const u64 bound = static_cast<u64>(nreq) * (nentries / kDigestRows + 1);
        const u32 chip = c->persistent_waves();
        const u32 wgs = static_cast<u32>((std::min<u64>(bound, chip) + 3) / 4);
        if (nentries) hipLaunchKernelGGL(k_dg_rows, dim3(wgs), dim3(256), 0, s, a, w.q, w.wfirst, wgs * 4u, digest);
        ok = c->check(hipGetLastError(), "frame digest rows");
    }
    // the edges, whole, into scratch; then the CRC of their parts inside the windows
    ok = ok && c->decode_chunks(in, w.c, E, w.scratch);
    if (ok) {
        hipLaunchKernelGGL(k_dg_ranges, dim3((E + 255u) / 256u), dim3(256), 0, s, E, w.c, w.e, w.q, w.crc_off, w.crc_len);
        ok = c->check(hipGetLastError(), "frame digest ranges") &&
             c->check(snp_launch_crc32c(w.scratch, w.crc_off, w.crc_len, E, c->crc_bits(), w.crc, nullptr, nullptr, s), "frame digest edge crc");
    }
    if (ok) {
        hipLaunchKernelGGL(k_dg_verdict, dim3(groups), dim3(256), 0, s, a, w.q, w.e, w.c, w.crc, digest, dig_len, status, d_result);
        ok = c->check(hipGetLastError(), "frame digest verdict");
    }
    return ok ? SNP_OK : SNP_ERR_DEVICE;
}

}  // extern "C"

// frame_dedup.hip -- snp_frame_dedup_indexed_batch: the duplicate chunks of a batch of seekable framed streams found on the device, proved equal
// byte for byte, the unique ones of the new streams written once into a PACK (a framed stream with its own index), and per new stream the
// compose segment list (its RECIPE) that rebuilds it from the base streams and the pack.  Nothing is decoded.  The rules -- the verdict of a
// stream, the key, the slot, when two chunks are the same, what a row stands for, where a segment begins -- are frame_dedup_device.h.  Built into
// libsnappier_hip_frame_dedup.so (C-ABI: include/snappier_hip_frame_dedup.h), linked against libsnappier_hip.so.  DESIGN.md 4.27.
//
//   init      every row: no key, no flag, canon = none; every slot of the table: empty
//   before    one workgroup: the largest clamped idx_first in front of every stream (a running maximum; frame_before_device.h)
//   verdict   a workgroup per stream: dd_stream, its rows walked by the threads (cc_add, the compose call's row check), joined; a stream that
//             passed: per row its stream, its chunk's bytes and, unless empty, its key
//   insert    one thread per row: the key's slot claimed by a 64-bit compare-and-swap, the slot's row lowered by an atomic minimum -- the lowest
//             row of a key, whatever the order of arrival
//   compare   a wavefront per row that is not its key's leader: the two chunks 16 bytes per lane (dd_same_part); canon
//   scans     over ALL rows, of the new streams that passed: unique rows, their chunk bytes, their decoded bytes, rows that take part, rows that
//             differ from their leader, chunk bytes of the merged rows
//   begins    one thread per row: its source and the source of the row before it in its stream (found over the scan of the rows that take
//             part) -> dd_begins; scan: segments
//   streams   one thread per stream: admission in stream order -- every scan only grows, so a stream is admitted iff the sums up to its last
//             row fit the three bounds; status; its segments; scans: admitted streams, seg_first
//   totals    the last admitted stream: what the pack holds.  result: one workgroup: the identifier, out_len, the pack's index words, d_result
//   emit      a wavefront per row: an admitted unique row's chunk copied to its place and its pack index row; an admitted segment's words
// No atomic decides an order or a value of an output: the table's minimum is the same in every run, everything else is a scan.  Nothing here
// allocates, reads back or synchronises: the call is capturable like the other _batch entry points.
#include "capi_internal.h"
#include "scan_tiles.h"
#include "frame_dedup_device.h"
#include "frame_before_device.h"
#include "../../include/snappier_hip_frame_dedup.h"

namespace {

static_assert(kDdNone == SNP_DEDUP_NONE, "SNP_DEDUP_NONE");

// row flags
constexpr u32 kNew = 1u, kLive = 2u, kUniq = 4u, kMerged = 8u, kColl = 16u, kBegin = 32u;

struct DdArgs {
    const u8* in;
    const u64 *in_off, *in_len;
    u32 ns, nbase;
    FrameIndex x;
    u64 slots;
};
struct DdWork {
    u64* part;
    // per stream
    u64* before;
    i32* verdict;
    u64 *admit, *csegs;         // per new stream: admitted (0 / 1); its segments when admitted
    u64* nadmit;                // scan of admit (nnew + 1)
    u64* tot;                   // what the pack holds: rows, chunk bytes, decoded bytes (+ 1 spare)
    // per row
    u64* key;
    u32 *size, *stream, *slot, *flag;
    u64 *uniq, *bytes, *dec, *live, *coll, *mbytes, *segs;     // scans (nentries + 1)
    // the table
    u64* tkey;
    u32* trow;
    u64 total;
};

// what a scan over the rows adds for row i: 1, the chunk's bytes or what it decodes to, for the rows that have every flag of `need`
struct ScanRows {
    const u32* __restrict__ flag;
    const u32* __restrict__ size;
    const u64* __restrict__ key;
    u32 need, what;
    __device__ __forceinline__ u64 operator()(u64 i) const
    {
        if ((flag[i] & need) != need) return 0;
        return what == 0 ? 1 : what == 1 ? size[i] : key[i] >> 32;
    }
};
struct ScanPlainWords {
    const u64* __restrict__ src;
    __device__ __forceinline__ u64 operator()(u64 i) const { return src[i]; }
};

inline u32 groups(u64 n) { return static_cast<u32>((n + 255) / 256); }

__global__ __launch_bounds__(256) void k_dd_init(u64 ne, u64 slots, DdWork w, u64* __restrict__ canon)
{
    const u64 most = ne > slots ? ne : slots;
    for (u64 i = static_cast<u64>(blockIdx.x) * 256u + threadIdx.x; i < most; i += static_cast<u64>(gridDim.x) * 256u) {
        if (i < ne) {
            w.key[i] = kDdNone;
            w.flag[i] = 0;
            w.size[i] = 0;
            w.stream[i] = 0;
            w.slot[i] = 0;
            canon[i] = kDdNone;
        }
        if (i < slots) {
            w.tkey[i] = kDdEmpty;
            w.trow[i] = kDdNoRow;
        }
        if (i < 4) w.tot[i] = 0;
    }
}

// A workgroup per stream.  The stream steers the whole workgroup.
__global__ __launch_bounds__(256) void k_dd_verdict(DdArgs a, DdWork w)
{
    const u32 b = blockIdx.x;
    const CcSeg k = dd_stream(a.x, a.in_len, b, w.before[b]);
    const u8* const s = a.in + a.in_off[b];
    CcAcc acc{};
    if (k.status == SNP_OK)
        for (u64 i = k.r0 + threadIdx.x; i < k.r1; i += 256u) cc_add(&acc, a.x, k, i, [&](u64 pos) { return frame_hop(s, k.n, pos); });
    const bool bad = __syncthreads_or(acc.bad ? 1 : 0) != 0;
    const i32 verdict = k.status != SNP_OK ? k.status : bad ? SNP_ERR_BAD_ARG : SNP_OK;
    if (threadIdx.x == 0) w.verdict[b] = verdict;
    if (verdict != SNP_OK) return;
    const u32 fresh = b >= a.nbase ? kNew : 0u;
    for (u64 i = k.r0 + threadIdx.x; i < k.r1; i += 256u) {
        const u64 pos = a.x.pos[i];
        const Hop h = frame_hop(s, k.n, pos);                           // (what cc_add saw: a data chunk inside the stream)
        w.stream[i] = b;
        w.size[i] = static_cast<u32>(h.next - pos);
        if (h.dec) {
            w.key[i] = dd_key(h.dec, dd_crc_field(s + pos));
            w.flag[i] = fresh | kLive;
        }
    }
}

// One thread per row that takes part.  The table is at most half full, so a probe ends; it is bounded by the table all the same.
__global__ __launch_bounds__(256) void k_dd_insert(u64 ne, u64 slots, DdWork w)
{
    const u64 r = static_cast<u64>(blockIdx.x) * 256u + threadIdx.x;
    if (r >= ne) return;
    const u64 key = w.key[r];
    if (key == kDdNone) return;
    const u64 mask = slots - 1;
    u64 s = dd_slot(key, mask);
    for (u64 n = 0; n < slots; ++n, s = (s + 1) & mask) {
        const u64 old = atomicCAS(reinterpret_cast<unsigned long long*>(w.tkey + s), static_cast<unsigned long long>(kDdEmpty),
                                  static_cast<unsigned long long>(key));
        if (old == kDdEmpty || old == key) {
            atomicMin(w.trow + s, static_cast<u32>(r));
            w.slot[r] = static_cast<u32>(s);
            return;
        }
    }
}

// A wavefront per row.  The row steers the whole wavefront.
__global__ __launch_bounds__(256) void k_dd_compare(DdArgs a, u64 ne, DdWork w, u64* __restrict__ canon)
{
    const u64 r = static_cast<u64>(blockIdx.x) * 4u + (threadIdx.x >> 6);
    if (r >= ne || w.key[r] == kDdNone) return;
    const u32 lane = threadIdx.x & 63u;
    const u64 leader = w.trow[w.slot[r]];
    bool same = true;
    if (leader != r) {
        const u64 n = w.size[r];
        same = leader < ne && n == w.size[leader];
        if (same) {
            const u8* const p = a.in + a.in_off[w.stream[r]] + a.x.pos[r];
            const u8* const q = a.in + a.in_off[w.stream[leader]] + a.x.pos[leader];
            const u64 parts = dd_parts(n);
            for (u64 k0 = 0; k0 < parts; k0 += 64) {
                const u64 k = k0 + lane;
                const bool ok = k >= parts || dd_same_part(p, q, n, k);
                if (ballot64(!ok)) { same = false; break; }
            }
        }
    }
    if (lane != 0) return;
    if (leader == r) {
        canon[r] = r;
        w.flag[r] |= kUniq;
    } else if (same) {
        canon[r] = leader;
        w.flag[r] |= kMerged;
    } else {
        canon[r] = r;
        w.flag[r] |= kUniq | kColl;
    }
}

// what row q (it takes part) stands for
__device__ __forceinline__ DdSrc source_of(const DdArgs& a, const DdWork& w, const u64* __restrict__ canon, u64 q)
{
    const u64 c = canon[q];
    return dd_source(w.stream[c], a.nbase, a.x.start[c], w.dec[c]);
}

// One thread per row of a new stream that takes part: does it begin a segment?
__global__ __launch_bounds__(256) void k_dd_begins(DdArgs a, u64 ne, DdWork w, const u64* __restrict__ canon)
{
    const u64 r = static_cast<u64>(blockIdx.x) * 256u + threadIdx.x;
    if (r >= ne || (w.flag[r] & (kNew | kLive)) != (kNew | kLive)) return;
    const u64 f0 = dd_first(a.x, w.stream[r]);
    const DdSrc cur = source_of(a, w, canon, r);
    bool first = w.live[r] == w.live[f0];
    DdSrc prev{};
    u64 plen = 0;
    if (!first) {
        const u64 p = ix_first_where(f0, r, [&](u64 q) { return w.live[q + 1] >= w.live[r]; });
        first = p >= r;                                                 // (never: a row that takes part lies in [f0, r))
        if (!first) {
            prev = source_of(a, w, canon, p);
            plen = w.key[p] >> 32;
        }
    }
    if (dd_begins(first, prev, plen, cur)) w.flag[r] |= kBegin;
}

// One thread per stream: the status, and for a new stream the admission.
__global__ __launch_bounds__(256) void k_dd_streams(DdArgs a, DdWork w, u32 max_entries, u32 max_segs, u64 out_cap, i32* __restrict__ status)
{
    const u32 b = blockIdx.x * 256u + threadIdx.x;
    if (b >= a.ns) return;
    i32 s = w.verdict[b];
    if (b >= a.nbase) {
        u64 admit = 0, segs = 0;
        if (s == SNP_OK) {
            const u64 f0 = dd_first(a.x, b), f1 = dd_first(a.x, b + 1);
            admit = w.uniq[f1] <= max_entries && w.bytes[f1] + SNP_STREAM_HEADER_LEN <= out_cap && w.segs[f1] <= max_segs ? 1 : 0;
            segs = admit ? w.segs[f1] - w.segs[f0] : 0;
            if (!admit) s = SNP_ERR_OUTPUT_TOO_SMALL;
        }
        w.admit[b - a.nbase] = admit;
        w.csegs[b - a.nbase] = segs;
    }
    status[b] = s;
}

// The last admitted stream: the sums up to its last row are what the pack holds.
__global__ __launch_bounds__(256) void k_dd_totals(DdArgs a, DdWork w)
{
    const u32 j = blockIdx.x * 256u + threadIdx.x, nnew = a.ns - a.nbase;
    if (j >= nnew || !w.admit[j] || w.nadmit[j + 1] != w.nadmit[nnew]) return;
    const u64 f1 = dd_first(a.x, a.nbase + j + 1);
    w.tot[0] = w.uniq[f1];
    w.tot[1] = w.bytes[f1];
    w.tot[2] = w.dec[f1];
}

// One workgroup: the pack's identifier, its length, the words of its index; d_result.
__global__ __launch_bounds__(256) void k_dd_result(DdArgs a, u64 ne, DdWork w, u64 out_cap, const i32* __restrict__ status, u8* __restrict__ out,
                                                  u64* __restrict__ out_len, u64* __restrict__ pk_first, u64* __restrict__ pk_total,
                                                  i32* __restrict__ pk_tail, u64* __restrict__ result)
{
    __shared__ u64 s_ok[4];
    u64 ok = 0;
    for (u32 b = threadIdx.x; b < a.ns; b += 256u) ok += status[b] == SNP_OK ? 1 : 0;
    ok = wave_sum(ok);
    if ((threadIdx.x & 63u) == 0) s_ok[threadIdx.x >> 6] = ok;
    __syncthreads();
    const bool room = out_cap >= SNP_STREAM_HEADER_LEN;
    if (room && threadIdx.x < SNP_STREAM_HEADER_LEN) out[threadIdx.x] = k_fc_stream_id[threadIdx.x];
    if (threadIdx.x != 0) return;
    out_len[0] = room ? SNP_STREAM_HEADER_LEN + w.tot[1] : 0;
    pk_first[0] = 0;
    pk_first[1] = w.tot[0];
    pk_total[0] = w.tot[2];
    pk_tail[0] = room ? SNP_OK : SNP_ERR_OUTPUT_TOO_SMALL;
    result[0] = w.uniq[ne];
    result[1] = w.bytes[ne] + SNP_STREAM_HEADER_LEN;
    result[2] = w.segs[ne];
    result[3] = s_ok[0] + s_ok[1] + s_ok[2] + s_ok[3];
    result[4] = w.live[ne];
    result[5] = w.live[ne] - w.uniq[ne];
    result[6] = w.coll[ne];
    result[7] = w.mbytes[ne];
}

// A wavefront per row of an admitted stream: a unique row's chunk and its row of the pack's index; a segment's words.
__global__ __launch_bounds__(256) void k_dd_emit(DdArgs a, u64 ne, DdWork w, const u64* __restrict__ canon, u8* __restrict__ out,
                                                u64* __restrict__ pk_start, u64* __restrict__ pk_pos, u32* __restrict__ seg_stream,
                                                u64* __restrict__ seg_off, u64* __restrict__ seg_len)
{
    const u64 r = static_cast<u64>(blockIdx.x) * 4u + (threadIdx.x >> 6);
    if (r >= ne) return;
    const u32 f = w.flag[r], lane = threadIdx.x & 63u;
    if ((f & (kNew | kLive)) != (kNew | kLive) || !(f & (kUniq | kBegin))) return;
    const u32 b = w.stream[r];
    if (!w.admit[b - a.nbase]) return;
    if (f & kUniq) {
        const u64 at = SNP_STREAM_HEADER_LEN + w.bytes[r];              // (admitted: at + size <= out_cap, uniq[r] < max_entries)
        wave_copy(out + at, a.in + a.in_off[b] + a.x.pos[r], w.size[r], lane);
        if (lane == 0) {
            pk_start[w.uniq[r]] = w.dec[r];
            pk_pos[w.uniq[r]] = at;
        }
    }
    if ((f & kBegin) && lane == 0) {
        const u64 f1 = dd_first(a.x, b + 1), g = w.segs[r];             // (admitted: g < max_segs)
        const u64 q = ix_first_where(r + 1, f1, [&](u64 i) { return w.segs[i + 1] > w.segs[r + 1]; });
        const DdSrc src = source_of(a, w, canon, r);
        seg_stream[g] = src.src;
        seg_off[g] = src.off;
        seg_len[g] = (q < f1 ? a.x.start[q] : a.x.total[b]) - a.x.start[r];
    }
}

// workspace (every piece 256-byte aligned; nothing when there is no stream)
DdWork work_layout(void* base, u32 ns, u64 ne)
{
    DdWork w{};
    if (ns == 0 || ne > kDdMaxRows) return w;
    const u64 slots = dd_slots(ne);
    WorkCarver k(base);
    w.part = k.take<u64>(scan_tiles_of(std::max<u64>(ns, ne)));
    w.before = k.take<u64>(ns);
    w.verdict = k.take<i32>(ns);
    w.admit = k.take<u64>(ns);
    w.csegs = k.take<u64>(ns);
    w.nadmit = k.take<u64>(static_cast<u64>(ns) + 1);
    w.tot = k.take<u64>(4);
    w.key = k.take<u64>(ne);
    for (u32** p : {&w.size, &w.stream, &w.slot, &w.flag}) *p = k.take<u32>(ne);
    for (u64** p : {&w.uniq, &w.bytes, &w.dec, &w.live, &w.coll, &w.mbytes, &w.segs}) *p = k.take<u64>(ne + 1);
    w.tkey = k.take<u64>(slots);
    w.trow = k.take<u32>(slots);
    w.total = k.bytes();
    return w;
}

}  // namespace

extern "C" {

uint64_t snp_frame_dedup_indexed_workspace(uint32_t nstreams, uint64_t nentries) { return work_layout(nullptr, nstreams, nentries).total; }

snp_status snp_frame_dedup_indexed_batch(snp_ctx* c, const uint8_t* in, const uint64_t* in_off, const uint64_t* in_len, uint32_t nstreams,
                                         const uint64_t* idx_first, const uint64_t* idx_start, const uint64_t* idx_pos, const uint64_t* idx_total,
                                         const int32_t* idx_tail, uint64_t nentries, uint32_t nbase, uint32_t max_entries, uint32_t max_segs,
                                         uint64_t out_cap, uint8_t* out, uint64_t* out_len, int32_t* status, uint64_t* canon, uint64_t* pk_first,
                                         uint64_t* pk_start, uint64_t* pk_pos, uint64_t* pk_total, int32_t* pk_tail, uint64_t* seg_first,
                                         uint32_t* seg_stream, uint64_t* seg_off, uint64_t* seg_len, void* d_work, uint64_t* d_result)
{
    if (!c || !d_result || nstreams > 0x7fffffffu || nbase > nstreams || nentries > kDdMaxRows ||       // (one workgroup per stream)
        (nstreams && (!in || !in_off || !in_len || !idx_first || !idx_total || !idx_tail || !out_len || !status || !pk_first || !pk_total || !pk_tail ||
                      !seg_first || !d_work)) ||
        (nstreams && nentries && (!idx_start || !idx_pos || !canon)) || (nstreams && out_cap && !out) ||
        (nstreams && max_entries && (!pk_start || !pk_pos)) || (nstreams && max_segs && (!seg_stream || !seg_off || !seg_len)))
        return SNP_ERR_BAD_ARG;
    DevGuard dg(c);
    if (!dg.ok) return SNP_ERR_DEVICE;
    hipStream_t s = c->stream;
    bool ok = c->check(snp_zero_words_async(reinterpret_cast<u32*>(d_result), 2 * 8, s), "frame dedup result");
    if (nstreams == 0) return ok ? SNP_OK : SNP_ERR_DEVICE;
    const DdWork w = work_layout(d_work, nstreams, nentries);
    const u32 ns = nstreams, nnew = nstreams - nbase, E = static_cast<u32>(nentries);
    const u64 ne = nentries, slots = dd_slots(ne);
    const DdArgs a{in, in_off, in_len, ns, nbase, FrameIndex{idx_first, idx_start, idx_pos, idx_total, idx_tail, nentries}, slots};
    const u32 wide = static_cast<u32>(std::min<u64>((std::max(ne, slots) + 255) / 256, 1u << 16)), waves = static_cast<u32>((ne + 3) / 4);
    // every stream's verdict and the rows of those that passed; the leader of every key; canon
    hipLaunchKernelGGL(k_dd_init, dim3(wide), dim3(256), 0, s, ne, slots, w, canon);
    hipLaunchKernelGGL(k_fr_before, dim3(1), dim3(256), 0, s, a.x, a.ns, w.before);
    hipLaunchKernelGGL(k_dd_verdict, dim3(ns), dim3(256), 0, s, a, w);
    if (ne) {
        hipLaunchKernelGGL(k_dd_insert, dim3(groups(ne)), dim3(256), 0, s, ne, slots, w);
        hipLaunchKernelGGL(k_dd_compare, dim3(waves), dim3(256), 0, s, a, ne, w, canon);
    }
    ok = ok && c->check(hipGetLastError(), "frame dedup canon");
    // what the rows of the new streams add up to; the segments
    const struct { u32 need, what; u64* dst; } row_scans[] = {{kNew | kUniq, 0, w.uniq},  {kNew | kUniq, 1, w.bytes},   {kNew | kUniq, 2, w.dec},
                                                             {kNew | kLive, 0, w.live},  {kNew | kColl, 0, w.coll},    {kNew | kMerged, 1, w.mbytes}};
    for (const auto& q : row_scans)
        ok = ok && c->check(launch_scan(ScanRows{w.flag, w.size, w.key, q.need, q.what}, E, w.part, q.dst, nullptr, s), "frame dedup row scan");
    if (ok && ne) hipLaunchKernelGGL(k_dd_begins, dim3(groups(ne)), dim3(256), 0, s, a, ne, w, canon);
    ok = ok && c->check(hipGetLastError(), "frame dedup begins") &&
         c->check(launch_scan(ScanRows{w.flag, w.size, w.key, kNew | kBegin, 0}, E, w.part, w.segs, nullptr, s), "frame dedup segment scan");
    // admission in stream order; the recipes' first segments; what the pack holds
    if (ok) {
        hipLaunchKernelGGL(k_dd_streams, dim3(groups(ns)), dim3(256), 0, s, a, w, max_entries, max_segs, out_cap, status);
        ok = c->check(hipGetLastError(), "frame dedup streams") &&
             c->check(launch_scan(ScanPlainWords{w.admit}, nnew, w.part, w.nadmit, nullptr, s), "frame dedup admission scan") &&
             c->check(launch_scan(ScanPlainWords{w.csegs}, nnew, w.part, seg_first, nullptr, s), "frame dedup recipe scan");
    }
    if (ok) {
        if (nnew) hipLaunchKernelGGL(k_dd_totals, dim3(groups(nnew)), dim3(256), 0, s, a, w);
        hipLaunchKernelGGL(k_dd_result, dim3(1), dim3(256), 0, s, a, ne, w, out_cap, status, out, out_len, pk_first, pk_total, pk_tail, d_result);
        if (ne && nnew)
            hipLaunchKernelGGL(k_dd_emit, dim3(waves), dim3(256), 0, s, a, ne, w, canon, out, pk_start, pk_pos, seg_stream, seg_off, seg_len);
        ok = c->check(hipGetLastError(), "frame dedup emit");
    }
    return ok ? SNP_OK : SNP_ERR_DEVICE;
}

}  // extern "C"

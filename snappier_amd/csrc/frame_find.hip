// frame_find.hip -- snp_frame_find_indexed_batch: where a byte string occurs in windows of what seekable framed streams decode to.  Per request
// the chunks the indexed read would select are decoded whole, one after the other, into one run of the scratch arena inside d_work; the run is
// searched there, so a match across chunk boundaries is no special case.  Built into libsnappier_hip_frame_find.so (C-ABI:
// include/snappier_hip_frame_find.h), linked against libsnappier_hip.so.  DESIGN.md 4.24.
//
//   plan      one thread per request: the indexed read's plan, the rows it owns, the bytes of its run (frame_find_device.h)
//   scans     owned rows over the requests -> each request's rows in the chunk table (d_result[0]; max_rows bounds it); the runs' bytes, as two
//             scans of their 32-bit halves so that no sum wraps -> each run's place in scratch (d_result[2]; scratch_cap bounds it)
//   rows      one thread per row of the chunk table: the read's check of the row, the row of the table; void: the rows of a request with a
//             row that failed its check are emptied again, so nothing of it is decoded
//   decode    snp_ctx::decode_chunks into scratch
//   fail      the first failing decoded row of each request, in stream order
//   tiles     scan of the tiles (kFindTile start positions) of the requests that are still good -> each request's first tile
//   count     workgroups take equal shares of consecutive tiles; 16 start positions per lane and step -> the occurrences that start in each tile
//   scan      of the tile counts -> each tile's rank base; a request's total
//   emit      the tiles whose base is below the request's hit_cap once more: positions written at base + rank in tile (a prefix sum over the
//             wavefront, wavefront sums in LDS: no atomic decides an order)
//   verdict   one thread per request
// Nothing here allocates, reads back or synchronises: the call is capturable like the other _batch entry points.
#include "capi_internal.h"
#include "scan_tiles.h"
#include "frame_edges_device.h"
#include "frame_find_device.h"
#include "../../include/snappier_hip_frame_find.h"

static_assert(kFindMaxNeedle == SNP_FIND_MAX_NEEDLE, "needle bound");

namespace {

constexpr u32 kBad = 1u;                // flags: a row failed its check
constexpr u32 kHead = 2u, kLast = 4u;   // flags: the plan's head and last
constexpr u32 kPlanShift = 8;           // (flags >> 8) & 0xff: the plan's status
constexpr u32 kStep = 256u * 16u;       // start positions a workgroup takes per step
static_assert(kFindTile % kStep == 0, "a tile is whole steps");

struct FindArgs {
    const u8* in;
    const u64 *in_off, *in_len;
    u32 ns;
    FrameIndex x;
    const u32* req_stream;
    const u64 *req_off, *req_len;
    u32 nreq;
    const u8* needles;
    const u64* needle_off;
    const u32* needle_len;
    u64 max_rows, scratch_cap;          // (scratch_cap: no more than kFindCapMax)
    const u64 *hit_off, *hit_cap;
};

struct FdWork {
    u64 *rfirst, *part;
    u64 *blo, *bhi;                     // the scans of the low and the high halves of the runs' bytes (nreq + 1 each)
    u64* tfirst;                        // each request's first tile (nreq + 1)
    u64 *nrows, *lo, *hi, *r0, *r1, *s0, *run, *fail;   // per request
    u32* flags;
    u32* tcnt;                          // per tile: the occurrences that start in it
    u64* tbase;                         // the scan of tcnt (tiles + 1)
    ChunkRows c;
    u8* scratch;
    u64 bytes;
    u32 tiles;                          // the tiles the arrays hold
};

__device__ __forceinline__ u64 run_place(const FdWork& w, u32 r) { return fd_sat_join(w.bhi[r], w.blo[r]); }
__device__ __forceinline__ bool fits(const FindArgs& a, const FdWork& w, u32 r)
{
    return w.rfirst[r + 1] <= a.max_rows && fd_sat_join(w.bhi[r + 1], w.blo[r + 1]) <= a.scratch_cap;
}
__device__ __forceinline__ i32 plan_status(u32 flags) { return static_cast<i32>(static_cast<int8_t>((flags >> kPlanShift) & 0xffu)); }
// the request is admitted, planned and every row passed its check: its run is decoded and searched
__device__ __forceinline__ bool live(const FindArgs& a, const FdWork& w, u32 r)
{
    const u32 f = w.flags[r];
    return plan_status(f) == SNP_OK && !(f & kBad) && fits(a, w, r);
}

struct ScanWords {
    const u64* __restrict__ src;
    __device__ __forceinline__ u64 operator()(u64 i) const { return src[i]; }
};
struct ScanLow {
    const u64* __restrict__ src;
    __device__ __forceinline__ u64 operator()(u64 i) const { return src[i] & 0xffffffffull; }
};
struct ScanHigh {
    const u64* __restrict__ src;
    __device__ __forceinline__ u64 operator()(u64 i) const { return src[i] >> 32; }
};
struct ScanTiles {
    FindArgs a;
    FdWork w;
    __device__ __forceinline__ u64 operator()(u64 i) const
    {
        const u32 r = static_cast<u32>(i);
        return live(a, w, r) ? fd_tiles(fd_starts(w.hi[r] - w.lo[r], a.needle_len[r])) : 0;
    }
};
struct ScanCounts {
    const u32* __restrict__ tcnt;
    const u64* __restrict__ ntiles;     // the tiles in use
    __device__ __forceinline__ u64 operator()(u64 i) const { return i < *ntiles ? tcnt[i] : 0; }
};

__global__ __launch_bounds__(256) void k_fd_plan(FindArgs a, FdWork w, u64* __restrict__ result)
{
    const u32 r = blockIdx.x * 256u + threadIdx.x;
    if (r >= a.nreq) return;
    if (r == 0) result[3] = 0;
    const FdPlan p = fd_plan(a.x, a.ns, a.req_stream[r], a.req_off[r], a.req_len[r], a.needle_len[r]);
    w.nrows[r] = p.rows < kFindRowClamp ? p.rows : kFindRowClamp;
    w.run[r] = p.bytes;
    w.lo[r] = p.k.lo;
    w.hi[r] = p.k.hi;
    w.r0[r] = p.k.r0;
    w.r1[r] = p.k.r1;
    w.s0[r] = p.s0;
    w.fail[r] = kNoFail;
    w.flags[r] = (static_cast<u32>(p.k.status) & 0xffu) << kPlanShift | (p.k.head ? kHead : 0u) | (p.k.last ? kLast : 0u);
}

// One thread per row of the chunk table: an empty row unless it belongs to an admitted request, passes the read's check and lies inside
// the request's run, so that it writes inside the run whatever the index says.
__global__ __launch_bounds__(256) void k_fd_rows(FindArgs a, FdWork w, u32 nrows)
{
    const u32 t = blockIdx.x * 256u + threadIdx.x;
    if (t >= nrows) return;
    w.c.tag[t] = kNone;
    chunk_row_clear(w.c, t, 0);
    if (t >= w.rfirst[a.nreq]) return;
    const u32 r = owner_of(static_cast<const u64*>(w.rfirst), a.nreq, t);
    if (!fits(a, w, r)) return;
    const u32 b = a.req_stream[r], flags = w.flags[r];                  // (b < ns: a request with rows was planned)
    FdPlan q{};
    q.k.lo = w.lo[r];
    q.k.hi = w.hi[r];
    q.k.r0 = w.r0[r];
    q.k.r1 = w.r1[r];
    q.k.head = flags & kHead;
    q.k.last = flags & kLast;
    q.k.f1 = a.x.first[b + 1] < a.x.nentries ? a.x.first[b + 1] : a.x.nentries;
    q.k.total = a.x.total[b];
    q.s0 = w.s0[r];
    q.bytes = w.run[r];
    const u64 i = q.k.r0 + (t - w.rfirst[r]);
    Hop h{};
    bool good = false;
    u64 at = 0;
    const bool inside = fd_row(a.x, a.in + a.in_off[b], a.in_len[b], q, i, &h, &good, &at);
    if (!good) atomicOr(w.flags + r, kBad);
    if (!inside || h.dec == 0) return;                                  // a zero-length chunk keeps its row, empty: it is never decoded or verified
    w.c.tag[t] = r;
    chunk_row_set(w.c, t, h, a.in_off[b] + a.x.pos[i], run_place(w, r) + at);
}

// the rows of a request with a row that failed its check, emptied again
__global__ __launch_bounds__(256) void k_fd_void(FdWork w, u32 nrows)
{
    const u32 t = blockIdx.x * 256u + threadIdx.x;
    if (t >= nrows) return;
    const u32 r = w.c.tag[t];
    if (r == kNone || !(w.flags[r] & kBad)) return;
    w.c.tag[t] = kNone;
    chunk_row_clear(w.c, t, 0);
}

// the failing decoded rows, keyed by the row's place in its request: the first in stream order wins
__global__ __launch_bounds__(256) void k_fd_fail(FdWork w, u32 nrows)
{
    const u32 t = blockIdx.x * 256u + threadIdx.x;
    if (t >= nrows) return;
    const u32 r = w.c.tag[t];
    if (r == kNone || w.c.status[t] == SNP_OK) return;
    atomic_min64(w.fail + r, fail_key(t - w.rfirst[r], w.c.status[t]));
}

// ---- the search ----------------------------------------------------------------------------------------------------------------------------------
// bit k of the result: byte k of the 16 bytes equals c
__device__ __forceinline__ u32 bytes_equal16(const snp_u128_unaligned& q, u32 c4)
{
    u32 mask = 0;
#pragma unroll
    for (u32 j = 0; j < 4; ++j) {
        const u32 y = q.v[j] ^ c4;
        const u32 z = ~(((y & 0x7f7f7f7fu) + 0x7f7f7f7fu) | y | 0x7f7f7f7fu);   // 0x80 in every byte of y that is zero
        mask |= (((z >> 7) * 0x10204080u) >> 28) << (4 * j);            // the four bits, gathered
    }
    return mask;
}

// how many of the 16 bytes equal c
__device__ __forceinline__ u32 bytes_equal16_count(const snp_u128_unaligned& q, u32 c4)
{
    u32 n = 0;
#pragma unroll
    for (u32 j = 0; j < 4; ++j) {
        const u32 y = q.v[j] ^ c4;
        n += static_cast<u32>(__builtin_popcount(~(((y & 0x7f7f7f7fu) + 0x7f7f7f7fu) | y | 0x7f7f7f7fu)));
    }
    return n;
}

// bit k of the result: the four bytes from byte k on equal n4 under fmask (v[0 .. 4]: 20 bytes)
__device__ __forceinline__ u32 prefix_equal16(const u32* v, u32 n4, u32 fmask)
{
    u32 mask = 0;
#pragma unroll
    for (u32 k = 0; k < 16; ++k) {
        const u32 x = (k & 3u) ? __builtin_amdgcn_alignbyte(v[(k >> 2) + 1], v[k >> 2], k & 3u) : v[k >> 2];
        mask |= (((x ^ n4) & fmask) == 0 ? 1u : 0u) << k;
    }
    return mask;
}

// bytes [4, m) of the needle (nd: its words in LDS) against the run's bytes at p + 4 ..., 16 at a time
__device__ __forceinline__ bool rest_equal(const u8* p, const u32* nd, u32 m)
{
    for (u32 off = 4; off < m; off += 16) {
        const snp_u128_unaligned q = *reinterpret_cast<const snp_u128_unaligned*>(p + off);
        const u32 rem = m - off;
        u32 d = 0;
#pragma unroll
        for (u32 j = 0; j < 4; ++j) {
            const u32 keep = rem >= 4 * (j + 1) ? ~0u : rem > 4 * j ? (1u << (8 * (rem - 4 * j))) - 1u : 0u;
            d |= (q.v[j] ^ nd[(off >> 2) + j]) & keep;
        }
        if (d) return false;
    }
    return true;
}

// The occurrences among the lane's `nvalid` (1 .. 16) start positions from p on, as a bit mask.  Reads at most m + 31 bytes from p on: inside
// the scratch arena and its slack, since p + m <= the window's end.
__device__ __forceinline__ u32 match16(const u8* p, u32 nvalid, u32 m, const u32* nd)
{
    const snp_u128_unaligned q = *reinterpret_cast<const snp_u128_unaligned*>(p);
    const u32 valid = (1u << nvalid) - 1u;
    if (m == 1) return bytes_equal16(q, (nd[0] & 0xffu) * 0x01010101u) & valid;
    const u32 v[5] = {q.v[0], q.v[1], q.v[2], q.v[3], ld32u(p + 16)};
    u32 cand = prefix_equal16(v, nd[0], m >= 4 ? ~0u : (1u << (8 * m)) - 1u) & valid;
    if (m <= 4) return cand;
    u32 hit = 0;
    while (cand) {
        const u32 k = static_cast<u32>(__builtin_ctz(cand));
        cand &= cand - 1;
        if (rest_equal(p + k, nd, m)) hit |= 1u << k;
    }
    return hit;
}

// Workgroups take equal shares of consecutive tiles.  EMIT false: tcnt[tile] = the occurrences that start in the tile.  EMIT true: a tile
// whose rank base is below its request's hit_cap writes its positions at base + rank, up to the cap.
template <bool EMIT>
__global__ __launch_bounds__(256) void k_fd_search(FindArgs a, FdWork w, u64* __restrict__ hits)
{
    __shared__ u32 s_needle[(kFindMaxNeedle + 16) / 4];
    __shared__ u32 s_wave[4];
    const u32 tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const u64 nt = w.tfirst[a.nreq];
    const u64 per = (nt + gridDim.x - 1) / gridDim.x, g0 = blockIdx.x * per, g1 = g0 + per < nt ? g0 + per : nt;
    if (g0 >= g1) return;
    u32 r = owner_of(static_cast<const u64*>(w.tfirst), a.nreq, g0), cur = kNone, m = 0;
    u64 lo = 0, starts = 0, s0 = 0, cap = 0, rank0 = 0;
    const u8* run = nullptr;
    u64* out = nullptr;
    bool wanted = true;
    for (u64 g = g0; g < g1; ++g) {
        while (g >= w.tfirst[r + 1]) ++r;                               // (g < nt = tfirst[nreq]: r stays below nreq)
        if (r != cur) {
            cur = r;
            m = a.needle_len[r];
            lo = w.lo[r];
            starts = fd_starts(w.hi[r] - lo, m);
            s0 = w.s0[r];
            run = w.scratch + run_place(w, r);
            if (EMIT) {
                cap = a.hit_cap[r];
                rank0 = w.tbase[w.tfirst[r]];
                out = hits + a.hit_off[r];
                wanted = cap != 0 && w.fail[r] == kNoFail && a.x.tail[a.req_stream[r]] == SNP_OK;
                if (!wanted) continue;
            }
            __syncthreads();                                            // (the previous request's needle is no longer read)
            if (tid < (kFindMaxNeedle + 16) / 4) s_needle[tid] = 0;
            __syncthreads();
            if (tid < m) reinterpret_cast<u8*>(s_needle)[tid] = a.needles[a.needle_off[r] + tid];
            __syncthreads();
        }
        u64 base = 0;
        if (EMIT) {
            base = w.tbase[g] - rank0;
            if (!wanted || w.tcnt[g] == 0 || base >= cap) continue;
        }
        u64 first, end;
        fd_tile(lo, starts, g - w.tfirst[r], &first, &end);
        u32 acc = 0;
        if (!EMIT && m == 1 && end - first == kFindTile) {
            // the delimiter count over a whole tile: the tile's loads are issued together, and nothing but a popcount follows them
            const u8* const p = run + (first - s0) + tid * 16u;
            snp_u128_unaligned q[kFindTile / kStep];
#pragma unroll
            for (u32 j = 0; j < kFindTile / kStep; ++j) q[j] = *reinterpret_cast<const snp_u128_unaligned*>(p + j * kStep);
            const u32 c4 = (s_needle[0] & 0xffu) * 0x01010101u;
#pragma unroll
            for (u32 j = 0; j < kFindTile / kStep; ++j) acc += bytes_equal16_count(q[j], c4);
            first = end;
        }
        for (u64 sb = first; sb < end; sb += kStep) {
            const u64 p0 = sb + tid * 16u;
            u32 mask = 0;
            if (p0 < end) mask = match16(run + (p0 - s0), end - p0 < 16 ? static_cast<u32>(end - p0) : 16u, m, s_needle);
            const u32 cnt = static_cast<u32>(__builtin_popcount(mask));
            if (!EMIT) {
                acc += cnt;
                continue;
            }
            u32 incl = cnt;                                             // the inclusive prefix sum across the wavefront
            for (u32 d = 1; d < 64; d <<= 1) {
                const u32 y = __shfl_up(incl, d, 64);
                if (lane >= d) incl += y;
            }
            if (lane == 63) s_wave[wave] = incl;
            __syncthreads();
            u32 before = 0, all = 0;
            for (u32 k = 0; k < 4; ++k) {
                before += k < wave ? s_wave[k] : 0;
                all += s_wave[k];
            }
            __syncthreads();                                            // (s_wave is written again by the next step)
            u64 rank = base + before + incl - cnt;
            while (mask && rank < cap) {
                out[rank++] = p0 + static_cast<u32>(__builtin_ctz(mask));
                mask &= mask - 1;
            }
            base += all;
            if (base >= cap) break;
        }
        if (!EMIT) {
            const u32 sum = static_cast<u32>(wave_sum(acc));
            if (lane == 0) s_wave[wave] = sum;
            __syncthreads();
            if (tid == 0) w.tcnt[g] = s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3];
            __syncthreads();                                            // (s_wave is written again by the next tile)
        }
    }
}

// The request's status: a bound missed, else what the plan refused, else a row that failed its check, else the first failing decoded row, else
// the stream's tail.  result[1] += the OK counts, result[3] += the OK requests (one atomic per wavefront each); result[2] = the bytes needed.
__global__ __launch_bounds__(256) void k_fd_verdict(FindArgs a, FdWork w, u64* __restrict__ win_len, u64* __restrict__ count, u64* __restrict__ nhits,
                                                   i32* __restrict__ status, u64* __restrict__ result)
{
    const u32 r = blockIdx.x * 256u + threadIdx.x;
    u64 ok_count = 0, ok = 0;
    if (r < a.nreq) {
        if (r == 0) result[2] = fd_sat_join(w.bhi[a.nreq], w.blo[a.nreq]);
        i32 s = SNP_ERR_OUTPUT_TOO_SMALL;
        u64 len = 0, n = 0;
        if (fits(a, w, r)) {
            const u32 flags = w.flags[r];
            s = plan_status(flags);
            if (s == SNP_OK && (flags & kBad)) s = SNP_ERR_BAD_ARG;
            else if (s == SNP_OK) s = window_verdict(SNP_OK, w.fail[r], SNP_OK, a.x.tail[a.req_stream[r]], false);
            if (s == SNP_OK) {
                len = w.hi[r] - w.lo[r];
                n = w.tbase[w.tfirst[r + 1]] - w.tbase[w.tfirst[r]];
                ok_count = n;
                ok = 1;
            }
        }
        status[r] = s;
        win_len[r] = len;
        count[r] = n;
        nhits[r] = n < a.hit_cap[r] ? n : a.hit_cap[r];
    }
    ok_count = wave_sum(ok_count);
    ok = wave_sum(ok);
    if ((threadIdx.x & 63u) == 0 && ok) {
        atomic_add64(result + 3, ok);
        if (ok_count) atomic_add64(result + 1, ok_count);
    }
}

// workspace: per request a few words; the tile sums of the scans; per tile a count and its rank base (admitted windows lie inside their runs,
// so they have no more than scratch_cap / kFindTile + nreq tiles); max_rows rows of a chunk table; then scratch_cap bytes of scratch and the
// slack a 16-byte read from its last bytes may touch
u32 tile_bound(u32 nreq, u64 scratch_cap) { return static_cast<u32>(scratch_cap / kFindTile + nreq); }
FdWork find_work_layout(void* base, u32 nreq, u64 max_rows, u64 scratch_cap)
{
    FdWork k{};
    if (nreq == 0) return k;
    const u64 nr = nreq;
    k.tiles = tile_bound(nreq, scratch_cap);
    WorkCarver c(base);
    k.rfirst = c.take<u64>(nr + 1);
    k.part = c.take<u64>(scan_tiles_of(std::max<u64>(nr, k.tiles)));
    k.blo = c.take<u64>(nr + 1);
    k.bhi = c.take<u64>(nr + 1);
    k.tfirst = c.take<u64>(nr + 1);
    k.nrows = c.take<u64>(nr);
    k.lo = c.take<u64>(nr);
    k.hi = c.take<u64>(nr);
    k.r0 = c.take<u64>(nr);
    k.r1 = c.take<u64>(nr);
    k.s0 = c.take<u64>(nr);
    k.run = c.take<u64>(nr);
    k.fail = c.take<u64>(nr);
    k.flags = c.take<u32>(nr);
    k.tcnt = c.take<u32>(k.tiles);
    k.tbase = c.take<u64>(static_cast<u64>(k.tiles) + 1);
    k.c = carve_chunk_rows(c, max_rows);
    k.scratch = c.take<u8>(scratch_cap + kFindSlack);
    k.bytes = c.bytes();
    return k;
}

constexpr u64 kMaxRows = 0x7fffffffull;

}  // namespace

extern "C" {

uint64_t snp_frame_find_indexed_workspace(uint32_t nreq, uint64_t max_rows, uint64_t scratch_cap)
{
    if (nreq > 0x3fffffffu || max_rows > kMaxRows) return 0;
    return find_work_layout(nullptr, nreq, max_rows, std::min<u64>(scratch_cap, kFindCapMax)).bytes;
}

snp_status snp_frame_find_indexed_batch(snp_ctx* c, const uint8_t* in, const uint64_t* in_off, const uint64_t* in_len, uint32_t nstreams,
                                        const uint64_t* idx_first, const uint64_t* idx_start, const uint64_t* idx_pos, const uint64_t* idx_total,
                                        const int32_t* idx_tail, uint64_t nentries, const uint32_t* req_stream, const uint64_t* req_off,
                                        const uint64_t* req_len, uint32_t nreq, const uint8_t* needles, const uint64_t* needle_off,
                                        const uint32_t* needle_len, uint64_t max_rows, uint64_t scratch_cap, uint64_t* hits,
                                        const uint64_t* hit_off, const uint64_t* hit_cap, uint64_t* win_len, uint64_t* count, uint64_t* nhits,
                                        int32_t* status, void* d_work, uint64_t* d_result)
{
    if (!c || !d_result || nreq > 0x3fffffffu || max_rows > kMaxRows ||
        (nreq && (!req_stream || !req_off || !req_len || !needles || !needle_off || !needle_len || !hits || !hit_off || !hit_cap || !win_len ||
                  !count || !nhits || !status || !d_work)) ||
        (nreq && nstreams && (!in || !in_off || !in_len || !idx_first || !idx_total || !idx_tail)) ||
        (nreq && nstreams && nentries && (!idx_start || !idx_pos)))
        return SNP_ERR_BAD_ARG;
    DevGuard dg(c);
    if (!dg.ok) return SNP_ERR_DEVICE;
    hipStream_t s = c->stream;
    if (nreq == 0)
        return c->check(snp_zero_words_async(reinterpret_cast<u32*>(d_result), 2 * 4, s), "frame find result") ? SNP_OK : SNP_ERR_DEVICE;
    scratch_cap = std::min<u64>(scratch_cap, kFindCapMax);
    const FdWork w = find_work_layout(d_work, nreq, max_rows, scratch_cap);
    const u32 T = static_cast<u32>(max_rows), groups = (nreq + 255u) / 256u;
    const FindArgs a{in, in_off, in_len, nstreams, FrameIndex{idx_first, idx_start, idx_pos, idx_total, idx_tail, nentries},
                     req_stream, req_off, req_len, nreq, needles, needle_off, needle_len, max_rows, scratch_cap, hit_off, hit_cap};
    hipLaunchKernelGGL(k_fd_plan, dim3(groups), dim3(256), 0, s, a, w, d_result);
    // each request's rows in the chunk table (d_result[0] = rows needed, [1] = 0) and its run's place in scratch
    bool ok = c->check(hipGetLastError(), "frame find plan") &&
              c->check(launch_scan(ScanWords{w.nrows}, nreq, w.part, w.rfirst, d_result, s), "frame find row scan") &&
              c->check(launch_scan(ScanLow{w.run}, nreq, w.part, w.blo, nullptr, s), "frame find byte scan") &&
              c->check(launch_scan(ScanHigh{w.run}, nreq, w.part, w.bhi, nullptr, s), "frame find byte scan");
    if (ok && T) {
        hipLaunchKernelGGL(k_fd_rows, dim3((T + 255u) / 256u), dim3(256), 0, s, a, w, T);
        hipLaunchKernelGGL(k_fd_void, dim3((T + 255u) / 256u), dim3(256), 0, s, w, T);
        ok = c->check(hipGetLastError(), "frame find rows") && c->decode_chunks(in, w.c, T, w.scratch);
        if (ok) hipLaunchKernelGGL(k_fd_fail, dim3((T + 255u) / 256u), dim3(256), 0, s, w, T);
    }
    ok = ok && c->check(launch_scan(ScanTiles{a, w}, nreq, w.part, w.tfirst, nullptr, s), "frame find tile scan");
    if (ok) {
        const u32 wgs = std::max<u32>(1, std::min<u32>(w.tiles, c->persistent_waves() / 4));
        hipLaunchKernelGGL(k_fd_search<false>, dim3(wgs), dim3(256), 0, s, a, w, hits);
        ok = c->check(hipGetLastError(), "frame find count") &&
             c->check(launch_scan(ScanCounts{w.tcnt, w.tfirst + nreq}, w.tiles, w.part, w.tbase, nullptr, s), "frame find count scan");
        if (ok) {
            hipLaunchKernelGGL(k_fd_search<true>, dim3(wgs), dim3(256), 0, s, a, w, hits);
            hipLaunchKernelGGL(k_fd_verdict, dim3(groups), dim3(256), 0, s, a, w, win_len, count, nhits, status, d_result);
            ok = c->check(hipGetLastError(), "frame find verdict");
        }
    }
    return ok ? SNP_OK : SNP_ERR_DEVICE;
}

}  // extern "C"

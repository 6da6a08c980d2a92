// frame_cuts.hip -- content-defined chunking on the device: snp_content_cuts_batch finds the cuts the bytes of every buffer define, and
// snp_frame_encode_cuts_batch is the chunked frame encoder (frame_chunked.hip) with the pieces given by the caller instead of a stride.  The rules
// of both -- the gear hash, what makes an offset a cut, when a cut list is good -- are frame_cuts_device.h.  Built into
// libsnappier_hip_frame_cuts.so (C-ABI: include/snappier_hip_frame_cuts.h), linked against libsnappier_hip.so.  DESIGN.md 4.26.
//
// The finder.  A buffer's positions are taken in tiles of kCutsTile, a tile in blocks of kCutsBlock; bmax holds the largest g of every block.
//   scans     the buffers' bytes, as two scans of their 32-bit halves so that no sum wraps (span_bytes bounds them); the tiles of the buffers
//             whose bytes fit -> each buffer's first tile
//   maxima    one workgroup per tile: the tile's bytes and a halo to LDS, lanes hash runs of kCutsRun positions after a 32-byte warm-up, the
//             hashes to LDS, the maximum of every block to bmax
//   count     the same hashing; a position that beats its 32 neighbours on either side is a survivor (two per block at the most); a survivor
//             is compared, by its whole wavefront, with the rest of its own and the two neighbouring blocks in LDS, then with bmax of the
//             blocks its window covers whole, then with a re-hash of the two ragged ends.  Per tile: the content cuts, the first and the last
//             of them, the forced cuts behind the first
//   scan      of the tiles' content cuts; lead: one thread per tile finds the last content cut before its tile through that scan and adds the
//             forced cuts in front of the tile's first content cut; scan of the tiles' cuts -> each tile's rank base
//   verdict   one thread per buffer: admission by max_cuts, status, cut_first, d_result
//   emit      the count pass once more over the admitted tiles that hold a cut: every cut written at base + its rank in the tile
// The encoder: frame_chunked.hip's sequence -- slot table, ONE compressor launch, ONE CRC launch, size scan, sizes, index, emit -- with a
// verdict over every buffer's cut list in front, staging at each piece's own stride, and emit units cut by bytes.
// Nothing here allocates, reads back or synchronises: both calls are capturable like the other _batch entry points.
#include "capi_internal.h"
#include "scan_tiles.h"
#include "work_carver.h"
#include "frame_rewrite_device.h"
#include "frame_cuts_device.h"
#include "../../include/snappier_hip_frame_cuts.h"

static_assert(kCutsMinWindow == SNP_CUTS_MIN_WINDOW && kCutsMaxWindow == SNP_CUTS_MAX_WINDOW, "window bounds");
static_assert(ec_stride(SNP_BLOCK_SIZE) == kSnpCompStride && ec_stride(4096) == snp_comp_stride(4096) && ec_stride(0) == 64, "staging stride");

namespace {

// ================================================================ the finder =======================================================================
constexpr u32 kBlocks = kCutsTile / kCutsBlock;                     // blocks of a tile
constexpr u32 kHalo = kCutsBlock;                                   // positions hashed on either side of the tile: the neighbouring blocks
constexpr u32 kHashed = kCutsTile + 2 * kHalo;                      // positions a workgroup hashes
constexpr u32 kStaged = (kHashed + kCutsHashBytes + 15) / 16 * 16;  // bytes it stages: those positions' and the warm-up of the first
constexpr u32 kNear = 32;                                           // neighbours on either side every position is compared with by its own lane
constexpr u32 kWaveCuts = kBlocks / 4 * kCutsBlock / (kCutsMinWindow + 1) + 1;   // content cuts among a wavefront's positions of a tile
constexpr u32 kTileCuts = 4 * kWaveCuts;
constexpr u32 kNoCut = 0xffffffffu;
static_assert(kHashed <= 256 * kCutsRun, "every hashed position has a lane");
static_assert(kNear <= kCutsMinWindow && kNear <= kHalo, "the near neighbours lie inside every window and inside the hashed range");
static_assert(kBlocks % 4 == 0 && kBlocks / 4 <= 64, "a wavefront's blocks");

struct CcArgs {
    const u8* in;
    const u64 *in_off, *in_len;
    u32 nb, w, mx;
    u64 span, max_cuts;
};

struct CcWork {
    u64 *blo, *bhi;                     // the scans of the low and the high halves of the buffers' bytes (nb + 1 each)
    u64* tfirst;                        // each buffer's first tile (nb + 1)
    u64* part;
    u32* bmax;                          // per block: the largest g in it
    u32 *ccnt, *first, *last, *fin, *tot;   // per tile: content cuts, the first and the last (offsets in the tile), forced cuts behind the first, all cuts
    u64* aprev;                         // per tile: the last content cut before the tile (0: none)
    u64 *cbase, *tbase;                 // the scans of ccnt and tot (tiles + 1)
    u64 bytes;
    u32 tiles;                          // the tiles the arrays hold
};

__device__ __forceinline__ bool bytes_fit(const CcArgs& a, const CcWork& w, u32 b) { return cc_sat_join(w.bhi[b + 1], w.blo[b + 1]) <= a.span; }
__device__ __forceinline__ bool cuts_fit(const CcArgs& a, const CcWork& w, u32 b) { return bytes_fit(a, w, b) && w.tbase[w.tfirst[b + 1]] <= a.max_cuts; }
// the admitted buffers: a prefix, so the first b that is not
__device__ inline u32 admitted(const CcArgs& a, const CcWork& w)
{
    u32 lo = 0, hi = a.nb;
    while (lo < hi) {
        const u32 mid = lo + (hi - lo) / 2;
        if (cuts_fit(a, w, mid)) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

struct ScanLow {
    const u64* __restrict__ src;
    __device__ __forceinline__ u64 operator()(u64 i) const { return src[i] & 0xffffffffull; }
};
struct ScanHigh {
    const u64* __restrict__ src;
    __device__ __forceinline__ u64 operator()(u64 i) const { return src[i] >> 32; }
};
struct ScanTilesOf {
    CcArgs a;
    CcWork w;
    __device__ __forceinline__ u64 operator()(u64 i) const
    {
        return bytes_fit(a, w, static_cast<u32>(i)) ? (a.in_len[i] + kCutsTile - 1) / kCutsTile : 0;
    }
};
struct ScanPerTile {
    const u32* __restrict__ cnt;
    const u64* __restrict__ ntiles;     // the tiles in use
    __device__ __forceinline__ u64 operator()(u64 i) const { return i < *ntiles ? cnt[i] : 0; }
};

__device__ __forceinline__ u32 wave_max32(u32 v)
{
    for (u32 d = 32; d; d >>= 1) {
        const u32 y = __shfl_xor(v, d, 64);
        v = y > v ? y : v;
    }
    return v;
}

// MODE 0: bmax of the tile's blocks.  MODE 1: the tile's counts.  MODE 2: the tile's cuts, written.
template <int MODE>
__global__ __launch_bounds__(256) void k_cc_tile(CcArgs a, CcWork w, u64* __restrict__ cuts)
{
    __shared__ u32 s_gear[256];
    __shared__ u32 s_h[kHashed];
    __shared__ __attribute__((aligned(16))) u8 s_x[kStaged];
    __shared__ u32 s_wcut[4][kWaveCuts];
    __shared__ u32 s_wn[4];
    __shared__ u32 s_cut[kTileCuts], s_forced[kTileCuts + 1], s_rank[kTileCuts + 1];
    __shared__ u64 s_k0[kTileCuts + 1];
    const u32 tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    s_gear[tid] = cc_gear(tid);
    const u64 nt = w.tfirst[a.nb];
    const u32 nadm = MODE == 2 ? admitted(a, w) : 0;
    for (u64 g = blockIdx.x; g < nt; g += gridDim.x) {
        if (MODE == 2 && w.tot[g] == 0) continue;
        const u32 b = owner_of(static_cast<const u64*>(w.tfirst), a.nb, g);
        if (MODE == 2 && b >= nadm) break;                              // (the tiles are in buffer order: every later one is out too)
        const u64 n = a.in_len[b], p0 = (g - w.tfirst[b]) * kCutsTile, p1 = p0 + kCutsTile < n ? p0 + kCutsTile : n;
        const u8* const x = a.in + a.in_off[b];
        // positions [h0, h1) are hashed: s_h[p - hbase]; bytes [x0, x1) are staged: s_x[i - sbase].  (hbase and sbase may lie before the buffer.)
        const long long hbase = static_cast<long long>(p0) - kHalo, sbase = hbase - kCutsHashBytes;
        const u64 h0 = p0 >= kHalo ? p0 - kHalo : 0, h1 = p0 + kCutsTile + kHalo < n ? p0 + kCutsTile + kHalo : n;
        const u64 x0 = h0 >= kCutsHashBytes ? h0 - kCutsHashBytes : 0, x1 = h1 - 1;   // (n > 0: the buffer has a tile)
        __syncthreads();                                                // (the previous tile's LDS is no longer read; s_gear is written)
        for (u32 q = tid; q < kStaged / 16; q += 256) {
            const long long lo = sbase + 16ll * q;
            if (lo >= static_cast<long long>(x0) && lo + 16 <= static_cast<long long>(x1)) {
                const snp_u128_unaligned v = *reinterpret_cast<const snp_u128_unaligned*>(x + lo);
                *reinterpret_cast<uint4*>(s_x + 16u * q) = make_uint4(v.v[0], v.v[1], v.v[2], v.v[3]);
            } else {
                for (u32 k = 0; k < 16; ++k)
                    if (lo + k >= static_cast<long long>(x0) && lo + k < static_cast<long long>(x1)) s_x[16u * q + k] = x[lo + k];
            }
        }
        if (tid < 4) s_wn[tid] = 0;
        __syncthreads();
        {
            // the lane's run: positions [s, e); g(s) from the (up to) 32 bytes before s, then one byte per position
            const long long r0 = hbase + static_cast<long long>(kCutsRun) * tid;
            const u64 s = r0 < static_cast<long long>(h0) ? h0 : static_cast<u64>(r0);
            const u64 e = r0 + kCutsRun < static_cast<long long>(h1) ? static_cast<u64>(r0 + kCutsRun) : h1;
            if (r0 + static_cast<long long>(kCutsRun) > static_cast<long long>(h0) && s < e) {
                const u64 q = s < kCutsHashBytes ? 0 : s - kCutsHashBytes;
                const u32 warm = static_cast<u32>(s - q), np = static_cast<u32>(e - s), hi = static_cast<u32>(static_cast<long long>(s) - hbase);
                u32 xi = static_cast<u32>(static_cast<long long>(q) - sbase), h = 0;
                for (u32 k = 0; k < warm; ++k) h = cc_step(h, s_gear[s_x[xi++]]);
                for (u32 k = 0; k < np; ++k) {
                    s_h[hi + k] = h;
                    if (k + 1 < np) h = cc_step(h, s_gear[s_x[xi++]]);
                }
            }
        }
        __syncthreads();
        if (MODE == 0) {
            u32 keep = 0;
            for (u32 k = 0; k < kBlocks / 4; ++k) {
                const u64 p = p0 + (wave * (kBlocks / 4) + k) * kCutsBlock + lane;
                const u32 m = wave_max32(p < p1 ? s_h[static_cast<long long>(p) - hbase] : 0u);
                if (lane == k) keep = m;
            }
            if (lane < kBlocks / 4) w.bmax[g * kBlocks + wave * (kBlocks / 4) + lane] = keep;
            continue;
        }
        const u64 mb = w.tfirst[b] * kBlocks;                           // bmax of the buffer's block 0
        for (u32 k = 0; k < kBlocks / 4; ++k) {
            const u64 j0 = p0 + (wave * (kBlocks / 4) + k) * kCutsBlock;    // the block's first position
            if (j0 >= p1) break;
            const u64 c = j0 + lane;
            bool ok = c < p1 && cc_eligible(c, n, a.w);
            const u32 hv = c < h1 ? s_h[static_cast<long long>(c) - hbase] : 0u;
            if (a.w >= kCutsBlock - 1) {
                // the window covers the whole block from any position in it: only the FIRST position that holds the block's maximum can be a cut
                const bool in = c < p1;
                const u32 m = wave_max32(in ? hv : 0u);
                const u64 top = __ballot(in && hv == m);
                ok = ok && top && lane == static_cast<u32>(__builtin_ctzll(top));
            } else {
                // an eligible c has c - w >= 1 and c + w < n, and w >= kNear: the near neighbours exist, and they are hashed
                for (u32 d = 1; d <= kNear; ++d) {
                    if (!__any(ok)) break;
                    if (ok) {
                        const u32 i = static_cast<u32>(static_cast<long long>(c) - hbase);
                        ok = cc_beats_before(hv, s_h[i - d]) && cc_beats_behind(hv, s_h[i + d]);
                    }
                }
            }
            for (u64 sv = __ballot(ok); sv; sv &= sv - 1) {
                const u32 l = static_cast<u32>(__builtin_ctzll(sv));
                const u64 cc = j0 + l;
                const u32 hc = __shfl(hv, l, 64);
                // the rest of the own block and the two neighbouring ones, inside the window: in LDS
                const u64 zl = j0 >= kCutsBlock ? j0 - kCutsBlock : 0, zr = j0 + 2 * kCutsBlock < h1 ? j0 + 2 * kCutsBlock : h1;   // [zl, zr)
                const u64 nl = cc - a.w > zl ? cc - a.w : zl, nr = cc + a.w + 1 < zr ? cc + a.w + 1 : zr;
                bool bad = false;
                for (u64 q = nl + lane; q < nr; q += 64) {
                    const u32 hq = s_h[static_cast<long long>(q) - hbase];
                    bad |= q < cc ? !cc_beats_before(hc, hq) : q > cc && !cc_beats_behind(hc, hq);
                }
                if (__any(bad)) continue;
                // the blocks the window covers whole, by their maxima: before [ja, jb), behind [jc, jd)
                const u64 wl = cc - a.w, wr = cc + a.w + 1;             // the window [wl, wr)
                const bool far_l = wl < zl, far_r = wr > zr;            // (far_r: zr = j0 + 128 < h1)
                const u64 ja = (wl + kCutsBlock - 1) / kCutsBlock, jb = zl / kCutsBlock, jc = zr / kCutsBlock, jd = wr / kCutsBlock;
                if (far_l)
                    for (u64 j = ja + lane; j < jb; j += 64) bad |= !cc_beats_before(hc, w.bmax[mb + j]);
                if (far_r)
                    for (u64 j = jc + lane; j < jd; j += 64) bad |= !cc_beats_behind(hc, w.bmax[mb + j]);
                if (__any(bad)) continue;
                // the two ragged ends, hashed again: [wl, ja * 64) and [jd * 64, wr), fewer than 64 positions each
                if (far_l && wl + lane < ja * kCutsBlock) bad |= !cc_beats_before(hc, cc_hash_at(x, wl + lane));
                if (far_r && jd * kCutsBlock + lane < wr) bad |= !cc_beats_behind(hc, cc_hash_at(x, jd * kCutsBlock + lane));
                if (__any(bad)) continue;
                if (lane == 0 && s_wn[wave] < kWaveCuts) s_wcut[wave][s_wn[wave]++] = static_cast<u32>(cc - p0);
            }
        }
        __syncthreads();
        // the tile's content cuts in ascending order: the wavefronts' lists one after the other
        const u32 nc = s_wn[0] + s_wn[1] + s_wn[2] + s_wn[3];
        if (tid < kTileCuts) {
            const u32 wv = tid / kWaveCuts, k = tid % kWaveCuts;
            u32 before = 0;
            for (u32 v = 0; v < wv; ++v) before += s_wn[v];
            if (k < s_wn[wv]) s_cut[before + k] = s_wcut[wv][k];
        }
        __syncthreads();
        // segment 0: before the first content cut (MODE 2 only: it needs the last content cut before the tile); segment i: behind content cut i - 1
        if (tid <= nc) {
            u64 k0 = 1, f = 0;
            const u64 hi = tid < nc ? p0 + s_cut[tid] : p1;
            if (tid > 0) f = cc_forced_in(p0 + s_cut[tid - 1], p0 + s_cut[tid - 1], hi, a.mx, &k0);
            else if (MODE == 2) f = cc_forced_in(w.aprev[g], p0, hi, a.mx, &k0);
            s_forced[tid] = static_cast<u32>(f);
            s_k0[tid] = k0;
        }
        __syncthreads();
        if (tid == 0) {
            u32 run = 0;                                                // s_rank[i]: the cuts of the tile before segment i
            for (u32 i = 0; i <= nc; ++i) {
                s_rank[i] = run;
                run += s_forced[i] + (i < nc ? 1u : 0u);
            }
            if (MODE == 1) {
                w.ccnt[g] = nc;
                w.first[g] = nc ? s_cut[0] : kNoCut;
                w.last[g] = nc ? s_cut[nc - 1] : kNoCut;
                w.fin[g] = run - nc;                                    // (segment 0 counted nothing)
            }
        }
        if (MODE == 2) {
            __syncthreads();
            u64* const dst = cuts + w.tbase[g];                         // (an admitted buffer's cut_first is tbase of its first tile)
            if (tid < nc) dst[s_rank[tid] + s_forced[tid]] = p0 + s_cut[tid];
            for (u32 i = 0; i <= nc; ++i) {
                const u64 from = i ? p0 + s_cut[i - 1] : w.aprev[g];
                for (u32 k = tid; k < s_forced[i]; k += 256) dst[s_rank[i] + k] = from + (s_k0[i] + k) * a.mx;
            }
        }
    }
}

// One thread per tile: the last content cut before the tile, found through the scan of the tiles' content cuts; the forced cuts in front of the
// tile's first content cut; the tile's cuts.
__global__ __launch_bounds__(256) void k_cc_lead(CcArgs a, CcWork w)
{
    const u64 g = static_cast<u64>(blockIdx.x) * 256u + threadIdx.x;
    const u64 nt = w.tfirst[a.nb];
    if (g >= nt) return;
    const u32 b = owner_of(static_cast<const u64*>(w.tfirst), a.nb, g);
    const u64 t0 = w.tfirst[b], n = a.in_len[b], p0 = (g - t0) * kCutsTile, p1 = p0 + kCutsTile < n ? p0 + kCutsTile : n;
    u64 prev = 0;
    const u64 r = w.cbase[g];
    if (r > w.cbase[t0]) {                                              // content cut r - 1 lies in the buffer: in the last tile u with cbase[u] <= r - 1
        const u64 u = owner_of(static_cast<const u64*>(w.cbase), static_cast<u32>(nt), r - 1);
        prev = (u - t0) * kCutsTile + w.last[u];
    }
    u64 k0;
    const u64 lead = cc_forced_in(prev, p0, w.ccnt[g] ? p0 + w.first[g] : p1, a.mx, &k0);
    w.aprev[g] = prev;
    w.tot[g] = static_cast<u32>(w.ccnt[g] + w.fin[g] + lead);
}

// One thread per buffer, and one more: status, cut_first, d_result.
__global__ __launch_bounds__(256) void k_cc_verdict(CcArgs a, CcWork w, u64* __restrict__ cut_first, i32* __restrict__ status, u64* __restrict__ result)
{
    const u32 b = blockIdx.x * 256u + threadIdx.x;
    if (b > a.nb) return;
    const u32 adm = admitted(a, w);
    cut_first[b] = w.tbase[w.tfirst[b < adm ? b : adm]];
    if (b < a.nb) status[b] = b < adm ? SNP_OK : SNP_ERR_OUTPUT_TOO_SMALL;
    if (b == a.nb) {
        result[0] = w.tbase[w.tfirst[a.nb]];
        result[1] = w.tbase[w.tfirst[adm]];
        result[2] = cc_sat_join(w.bhi[a.nb], w.blo[a.nb]);
        result[3] = adm;
    }
}

// workspace: per buffer the three scans; the tile sums of the scans; per tile kBlocks block maxima, six words and three scan values.  The
// buffers whose bytes fit span_bytes have no more than span_bytes / kCutsTile + nbuffers tiles.
CcWork cuts_work_layout(void* base, u32 nbuffers, u64 span)
{
    CcWork k{};
    if (nbuffers == 0) return k;
    const u64 nb = nbuffers;
    k.tiles = static_cast<u32>(span / kCutsTile + nb);
    const u64 nt = k.tiles;
    WorkCarver c(base);
    k.blo = c.take<u64>(nb + 1);
    k.bhi = c.take<u64>(nb + 1);
    k.tfirst = c.take<u64>(nb + 1);
    k.part = c.take<u64>(scan_tiles_of(std::max<u64>(nb, nt)));
    k.bmax = c.take<u32>(nt * kBlocks);
    k.ccnt = c.take<u32>(nt);
    k.first = c.take<u32>(nt);
    k.last = c.take<u32>(nt);
    k.fin = c.take<u32>(nt);
    k.tot = c.take<u32>(nt);
    k.aprev = c.take<u64>(nt);
    k.cbase = c.take<u64>(nt + 1);
    k.tbase = c.take<u64>(nt + 1);
    k.bytes = c.bytes();
    return k;
}

constexpr u32 kMaxBuffers = 0x3fffffffu;

// ================================================================ the encoder ======================================================================
struct EcArgs {
    const u8* in;
    const u64 *in_off, *in_len;
    u32 nb;
    const u64 *cut_first, *cuts;
    u64 ncuts;
    u32 max_chunks;
    u64 stage_cap;
};

struct EcWork {
    u64 *first, *sfirst, *gfirst, *part;    // per buffer (+ 1): first slot, first staged byte, first emit unit
    u64* need;                          // per buffer: the staging of its pieces
    u32* good;                          // per buffer: its cut list passed
    RwSlots sl;                         // (sl.coff: max_chunks + 1, the scan of the slots' strides)
    u32* owner;
    u64* cscan;
    u8* comp;
    u64 bytes;
};

__device__ __forceinline__ bool ec_admitted(const EcArgs& a, const EcWork& w, u32 b)
{
    return w.good[b] && w.first[b + 1] <= a.max_chunks && w.sfirst[b + 1] <= a.stage_cap;
}

struct ScanGoodPieces {
    EcArgs a;
    const u32* __restrict__ good;
    __device__ __forceinline__ u64 operator()(u64 b) const { return good[b] ? ec_pieces(a.cut_first[b], a.cut_first[b + 1], a.in_len[b]) : 0; }
};
struct ScanStrides {
    const u32* __restrict__ len;
    __device__ __forceinline__ u64 operator()(u64 i) const { return ec_stride(len[i]); }   // (an empty slot: the 64 bytes the compressor may touch)
};
struct ScanOkRows {
    const u64* __restrict__ first;
    const i32* __restrict__ status;
    __device__ __forceinline__ u64 operator()(u64 b) const { return status[b] == SNP_OK ? first[b + 1] - first[b] : 0; }
};
struct ScanUnits {
    const u64* __restrict__ in_len;
    const i32* __restrict__ status;
    __device__ __forceinline__ u64 operator()(u64 b) const { return status[b] == SNP_OK ? (in_len[b] + kUnit - 1) / kUnit : 0; }
};

// One workgroup per buffer at a time: the verdict over its cut list (every read of `cuts` below ncuts) and the staging its pieces need.
__global__ __launch_bounds__(256) void k_ec_verdict(EcArgs a, EcWork w)
{
    __shared__ u64 s_sum[4];
    const u32 tid = threadIdx.x;
    for (u32 b = blockIdx.x; b < a.nb; b += gridDim.x) {
        const u64 lo = a.cut_first[b], hi = a.cut_first[b + 1], n = a.in_len[b];
        bool bad = !ec_range_ok(lo, hi, a.ncuts);
        u64 sum = 0;
        if (!bad) {
            for (u64 i = lo + tid; i < hi; i += 256) {
                const u64 prev = i > lo ? a.cuts[i - 1] : 0, cut = a.cuts[i];
                if (!ec_cut_ok(prev, cut, n)) bad = true;
                else sum += ec_stride(cut - prev);
            }
        }
        bad = __syncthreads_or(bad);
        if (!bad && tid == 0) {
            const u64 last = hi > lo ? a.cuts[hi - 1] : 0;
            if (!ec_tail_ok(last, n)) bad = true;
            else if (n) sum += ec_stride(n - last);
        }
        bad = __syncthreads_or(bad);
        sum = wave_sum(sum);
        if ((tid & 63u) == 0) s_sum[tid >> 6] = sum;
        __syncthreads();
        if (tid == 0) {
            w.good[b] = bad ? 0u : 1u;
            w.need[b] = bad ? 0 : s_sum[0] + s_sum[1] + s_sum[2] + s_sum[3];
        }
        __syncthreads();                                                // (s_sum is written again for the next buffer)
    }
}

// one thread per slot: the piece, or nothing for a slot no admitted buffer owns
__global__ __launch_bounds__(256) void k_ec_plan(EcArgs a, EcWork w)
{
    const u32 c = blockIdx.x * 256u + threadIdx.x;
    if (c >= a.max_chunks) return;
    u32 owner = kFcNone, len = 0;
    u64 off = 0;
    if (c < w.first[a.nb]) {
        const u32 b = fc_owner(w.first, a.nb, c);                       // (a buffer with a slot: its list passed)
        if (ec_admitted(a, w, b)) {
            u64 start;
            len = ec_piece(a.cuts, a.cut_first[b], a.cut_first[b + 1], a.in_len[b], c - w.first[b], &start);
            off = a.in_off[b] + start;
            owner = b;
        }
    }
    w.owner[c] = owner;
    w.sl.in_off[c] = off;
    w.sl.len[c] = len;
}

// k_fc_sizes of frame_chunked.hip, with the verdict over the cut list in front
__global__ __launch_bounds__(256) void k_ec_sizes(EcArgs a, EcWork w, u8* __restrict__ out, const u64* __restrict__ out_off, const u64* __restrict__ out_cap,
                                                 u64* __restrict__ out_len, i32* __restrict__ status, u64* __restrict__ result)
{
    const u32 b = blockIdx.x * 256u + threadIdx.x;
    u64 ok_len = 0, ok = 0;
    if (b < a.nb) {
        i32 st = w.good[b] ? SNP_ERR_OUTPUT_TOO_SMALL : SNP_ERR_BAD_ARG;
        u64 len = 0;
        if (ec_admitted(a, w, b)) {
            const u64 size = SNP_STREAM_HEADER_LEN + (w.cscan[w.first[b + 1]] - w.cscan[w.first[b]]);
            if (size <= out_cap[b]) {
                u8* const dst = out + out_off[b];
                for (u32 i = 0; i < SNP_STREAM_HEADER_LEN; ++i) dst[i] = k_fc_stream_id[i];   // EnsureStreamHeaderWritten  :148-157
                st = SNP_OK;
                len = size;
                ok = 1;
            }
        }
        out_len[b] = len;
        status[b] = st;
        ok_len = len;
    }
    add_written(result, ok_len, ok, 0);
}

// the per-stream half of the index; result[2] = the rows written
__global__ __launch_bounds__(256) void k_ec_streams(u32 nb, const u64* __restrict__ in_len, const i32* __restrict__ status, const u64* __restrict__ idx_first,
                                                   u64* __restrict__ idx_total, i32* __restrict__ idx_tail, u64* __restrict__ result)
{
    const u32 b = blockIdx.x * 256u + threadIdx.x;
    if (b == 0) result[2] = idx_first[nb];
    if (b >= nb) return;
    idx_total[b] = status[b] == SNP_OK ? in_len[b] : 0;
    idx_tail[b] = status[b];
}

// One workgroup per emit unit of a written stream at a time: the pieces that start in 64 KiB of its input, taken by teams of threads in turn --
// the whole workgroup on one piece, half on each of two, else a wavefront each.  With an index, the piece's row.
__global__ __launch_bounds__(256) void k_ec_emit(EcArgs a, EcWork w, u8* __restrict__ out, const u64* __restrict__ out_off, const u64* __restrict__ ok_first,
                                                u64* __restrict__ idx_start, u64* __restrict__ idx_pos)
{
    const u32 tid = threadIdx.x;
    const u64 units = w.gfirst[a.nb];
    for (u64 g = blockIdx.x; g < units; g += gridDim.x) {
        const u32 b = fc_owner(w.gfirst, a.nb, g);
        const u64 u = g - w.gfirst[b], lo = a.cut_first[b], hi = a.cut_first[b + 1], n = a.in_len[b];
        const u64 k0 = ec_first_piece_from(a.cuts, lo, hi, u * kUnit);
        const u64 k1 = (u + 1) * kUnit >= n ? hi - lo + 1 : ec_first_piece_from(a.cuts, lo, hi, (u + 1) * kUnit);
        const u32 team = fc_team(k1 - k0 > 2 ? 3u : static_cast<u32>(k1 - k0)), t = tid % team, teams = 256u / team;
        u8* const dst = out + out_off[b];
        for (u64 k = k0 + tid / team; k < k1; k += teams) {
            const u64 c = w.first[b] + k, pos = SNP_STREAM_HEADER_LEN + (w.cscan[c] - w.cscan[w.first[b]]);
            emit_slot(dst + pos, w.sl, c, a.in, w.comp, t, team);
            if (idx_start && t == 0) {
                idx_start[ok_first[b] + k] = w.sl.in_off[c] - a.in_off[b];
                idx_pos[ok_first[b] + k] = pos;
            }
        }
    }
}

// workspace: per buffer three scans, the staging need and the verdict; per slot the table the compressor, the CRC and the emit read, its owner,
// and the two scans; then the staging: stage_cap for the admitted pieces and 64 bytes for every slot that may stay empty
EcWork encode_work_layout(void* base, u32 nbuffers, u32 max_chunks, u64 stage_cap)
{
    EcWork k{};
    if (nbuffers == 0) return k;
    const u64 nb = nbuffers, nc = max_chunks;
    WorkCarver c(base);
    k.first = c.take<u64>(nb + 1);
    k.sfirst = c.take<u64>(nb + 1);
    k.gfirst = c.take<u64>(nb + 1);
    k.part = c.take<u64>(scan_tiles_of(std::max<u64>(nb, nc)));
    k.need = c.take<u64>(nb);
    k.good = c.take<u32>(nb);
    k.sl.in_off = c.take<u64>(nc);
    k.sl.coff = c.take<u64>(nc + 1);
    k.sl.len = c.take<u32>(nc);
    k.sl.comp_len = c.take<u32>(nc);
    k.sl.crc = c.take<u32>(nc);
    k.sl.c_status = c.take<i32>(nc);
    k.owner = c.take<u32>(nc);
    k.cscan = c.take<u64>(nc + 1);
    k.comp = c.take<u8>(stage_cap + nc * ec_stride(0));
    k.bytes = c.bytes();
    return k;
}

}  // namespace

extern "C" {

uint64_t snp_content_cuts_workspace(uint32_t nbuffers, uint64_t span_bytes, uint32_t window)
{
    if (nbuffers > kMaxBuffers || window < kCutsMinWindow || window > kCutsMaxWindow) return 0;
    return cuts_work_layout(nullptr, nbuffers, std::min<u64>(span_bytes, kCutsSpanMax)).bytes;
}

snp_status snp_content_cuts_batch(snp_ctx* c, const uint8_t* in, const uint64_t* in_off, const uint64_t* in_len, uint32_t nbuffers, uint32_t window,
                                  uint32_t max_bytes, uint64_t span_bytes, uint64_t max_cuts, uint64_t* cut_first, uint64_t* cuts, int32_t* status,
                                  void* d_work, uint64_t* d_result)
{
    if (!c || !d_result || !cc_params_ok(window, max_bytes) || nbuffers > kMaxBuffers ||
        (nbuffers && (!in || !in_off || !in_len || !cut_first || !status || !d_work || (max_cuts && !cuts))))
        return SNP_ERR_BAD_ARG;
    DevGuard dg(c);
    if (!dg.ok) return SNP_ERR_DEVICE;
    hipStream_t s = c->stream;
    if (nbuffers == 0) {
        bool ok = c->check(snp_zero_words_async(reinterpret_cast<u32*>(d_result), 2 * 4, s), "content cuts result");
        if (ok && cut_first) ok = c->check(snp_zero_words_async(reinterpret_cast<u32*>(cut_first), 2, s), "content cuts empty scan");
        return ok ? SNP_OK : SNP_ERR_DEVICE;
    }
    span_bytes = std::min<u64>(span_bytes, kCutsSpanMax);
    const CcWork w = cuts_work_layout(d_work, nbuffers, span_bytes);
    const CcArgs a{in, in_off, in_len, nbuffers, window, max_bytes, span_bytes, max_cuts};
    const u32 wgs = std::max<u32>(1, std::min<u32>(w.tiles, c->persistent_waves() / 4));
    bool ok = c->check(launch_scan(ScanLow{in_len}, nbuffers, w.part, w.blo, nullptr, s), "content cuts byte scan") &&
              c->check(launch_scan(ScanHigh{in_len}, nbuffers, w.part, w.bhi, nullptr, s), "content cuts byte scan") &&
              c->check(launch_scan(ScanTilesOf{a, w}, nbuffers, w.part, w.tfirst, nullptr, s), "content cuts tile scan");
    if (ok) {
        hipLaunchKernelGGL(k_cc_tile<0>, dim3(wgs), dim3(256), 0, s, a, w, cuts);
        hipLaunchKernelGGL(k_cc_tile<1>, dim3(wgs), dim3(256), 0, s, a, w, cuts);
        ok = c->check(hipGetLastError(), "content cuts count") &&
             c->check(launch_scan(ScanPerTile{w.ccnt, w.tfirst + nbuffers}, w.tiles, w.part, w.cbase, nullptr, s), "content cuts count scan");
    }
    if (ok) {
        hipLaunchKernelGGL(k_cc_lead, dim3(groups_of(w.tiles)), dim3(256), 0, s, a, w);
        ok = c->check(hipGetLastError(), "content cuts lead") &&
             c->check(launch_scan(ScanPerTile{w.tot, w.tfirst + nbuffers}, w.tiles, w.part, w.tbase, nullptr, s), "content cuts rank scan");
    }
    if (ok) {
        hipLaunchKernelGGL(k_cc_verdict, dim3(groups_of(static_cast<u64>(nbuffers) + 1)), dim3(256), 0, s, a, w, cut_first, status, d_result);
        if (max_cuts) hipLaunchKernelGGL(k_cc_tile<2>, dim3(wgs), dim3(256), 0, s, a, w, cuts);
        ok = c->check(hipGetLastError(), "content cuts emit");
    }
    return ok ? SNP_OK : SNP_ERR_DEVICE;
}

uint64_t snp_frame_encode_cuts_workspace(uint32_t nbuffers, uint32_t max_chunks, uint64_t stage_cap)
{
    return encode_work_layout(nullptr, nbuffers, max_chunks, stage_cap).bytes;
}

snp_status snp_frame_encode_cuts_batch(snp_ctx* c, const uint8_t* in, const uint64_t* in_off, const uint64_t* in_len, uint32_t nbuffers,
                                       const uint64_t* cut_first, const uint64_t* cuts, uint64_t ncuts, uint32_t max_chunks, uint64_t stage_cap,
                                       uint8_t* out, const uint64_t* out_off, const uint64_t* out_cap, uint64_t* out_len, int32_t* status,
                                       uint64_t* idx_first, uint64_t* idx_start, uint64_t* idx_pos, uint64_t* idx_total, int32_t* idx_tail,
                                       void* d_work, uint64_t* d_result)
{
    const int given = (idx_first != nullptr) + (idx_start != nullptr) + (idx_pos != nullptr) + (idx_total != nullptr) + (idx_tail != nullptr);
    if (!c || !d_result || (given != 0 && given != 5) ||
        (nbuffers && (!in || !in_off || !in_len || !cut_first || (ncuts && !cuts) || !out || !out_off || !out_cap || !out_len || !status || !d_work)))
        return SNP_ERR_BAD_ARG;
    const bool index = given == 5;
    DevGuard dg(c);
    if (!dg.ok) return SNP_ERR_DEVICE;
    hipStream_t s = c->stream;
    const char* const what = "frame encode cuts";
    // d_result[2] and [3] start at zero (the first scan sets [0] and clears [1]); an empty batch has no row: idx_first[0] = 0 is all its index
    bool ok = check_step(c, snp_zero_words_async(reinterpret_cast<u32*>(d_result), 8, s), what, "result");
    if (nbuffers == 0) {
        if (ok && index) ok = check_step(c, snp_zero_words_async(reinterpret_cast<u32*>(idx_first), 2, s), what, "empty index");
        return ok ? SNP_OK : SNP_ERR_DEVICE;
    }
    const EcWork w = encode_work_layout(d_work, nbuffers, max_chunks, stage_cap);
    const EcArgs a{in, in_off, in_len, nbuffers, cut_first, cuts, ncuts, max_chunks, stage_cap};
    const u32 nb = nbuffers, M = max_chunks, bg = groups_of(nb);
    // the verdict over every list; then the slots and the staging of the buffers whose list passed (d_result[0] = slots needed, d_result[1] = 0)
    hipLaunchKernelGGL(k_ec_verdict, dim3(std::min<u32>(nb, kEmitGroups)), dim3(256), 0, s, a, w);
    ok = ok && check_step(c, hipGetLastError(), what, "verdict") &&
         check_step(c, launch_scan(ScanGoodPieces{a, w.good}, nb, w.part, w.first, d_result, s), what, "piece scan") &&
         check_step(c, launch_scan(ScanWords{w.need}, nb, w.part, w.sfirst, nullptr, s), what, "staging scan");
    if (ok && M) {
        hipLaunchKernelGGL(k_ec_plan, dim3(groups_of(M)), dim3(256), 0, s, a, w);
        ok = check_step(c, hipGetLastError(), what, "plan") &&
             check_step(c, launch_scan(ScanStrides{w.sl.len}, M, w.part, w.sl.coff, nullptr, s), what, "stride scan");
    }
    // CompressBlock and the masked CRC-32C of every slot, the framed sizes; every buffer's size and status; the index of the OK buffers
    ok = ok && reencode_slots(c, in, w.sl, M, w.comp, w.part, w.cscan, what);
    if (ok) {
        hipLaunchKernelGGL(k_ec_sizes, dim3(bg), dim3(256), 0, s, a, w, out, out_off, out_cap, out_len, status, d_result);
        ok = check_step(c, hipGetLastError(), what, "sizes");
    }
    if (ok && index) {
        ok = check_step(c, launch_scan(ScanOkRows{w.first, status}, nb, w.part, idx_first, nullptr, s), what, "row scan");
        if (ok) {
            hipLaunchKernelGGL(k_ec_streams, dim3(bg), dim3(256), 0, s, nb, in_len, status, idx_first, idx_total, idx_tail, d_result);
            ok = check_step(c, hipGetLastError(), what, "streams");
        }
    }
    // the chunks (and their rows) to their places, in units of 64 KiB of input
    ok = ok && check_step(c, launch_scan(ScanUnits{in_len, status}, nb, w.part, w.gfirst, nullptr, s), what, "unit scan");
    if (ok && M) {
        hipLaunchKernelGGL(k_ec_emit, dim3(kEmitGroups), dim3(256), 0, s, a, w, out, out_off, index ? idx_first : nullptr, index ? idx_start : nullptr,
                           index ? idx_pos : nullptr);
        ok = check_step(c, hipGetLastError(), what, "emit");
    }
    return ok ? SNP_OK : SNP_ERR_DEVICE;
}

}  // extern "C"

// buffers_decode.hip -- snp_decompress_buffers_batch: the device-batch counterpart of snp_try_decompress.  Every block that is large enough is
// decoded a wavefront per 64 KiB output fragment with the tag index (tag_index.hip), for all such blocks of the batch at once and
// with nothing read back to the host; the other blocks go through snp_decompress_batch's own launch sequence.  Built into
// libsnappier_hip_buffers_decompress.so (C-ABI: include/snappier_hip_buffers_decompress.h), linked against libsnappier_hip.so.
// The steps, all on the context's stream:
//   classify  one thread per block: varint preamble (snp_rules.h), candidate or not (the rule of snp_try_decompress plus a stream-length bound)
//   plan      scans (scan_tiles.h): the candidates' declared bytes (the makespan rule needs their sum), the fragments of the blocks chosen for
//             splitting (d_result[0]; admitted in buffer order while they fit max_fragments), the chunks and the count of the admitted blocks;
//             then one thread per block: masked in_len / out_cap (0 for a split block) and the block's tag-index control words
//   index     k_tag_cand, k_tag_scan and the look-back kernel of tag_index.hip over every split block at once: the first and the last take one
//             global ticket in block-major chunk order, the scan runs as persistent workgroups that take blocks, each with its own RunCache;
//             the kernels here are drivers of the same bodies as tag_index.hip's (tag_index_device.h: cand_chunk, scan_pass / fix_pass,
//             look_back_chunk, fragment_start)
//   decode    the fragment table (k_fragment_starts over all blocks), one launch of the fragment decoder, then snp_ctx::launch_decompress over
//             all blocks with the masked lengths (a split block is a no-op there)
//   finalize  a split block is OK when all its fragments are; the others go on a list that the list decoder decodes one wavefront each
#include "capi_internal.h"
#include "scan_tiles.h"
#include "tag_index_device.h"
#include "work_carver.h"
#include "../../include/snappier_hip_buffers_decompress.h"

namespace {

constexpr u32 kNone = 0xffffffffu;
constexpr u32 kSplitFactor = 2;          // c of the makespan rule: split when declared >= c * (sum of the candidates' declared bytes) / wave slots
constexpr u32 kScanSlots = 256;          // persistent k_tag_scan workgroups (RunCache slots) at most
constexpr u32 kMaxFragments = 1u << 26;  // max_fragments counts up to this (4 TiB of output): keeps the packed chunk | block counts in 32 bits each
constexpr u32 kSlotsPerFragment = 7;     // per-block tag-index slots (chunks + 2) <= 5 * fragments + 2 <= 7 * fragments
constexpr u32 kCtlWords = 16;            // per block: ScanCtl (words 0-8; word 2 = the look-back flag), word 12 = a fragment failed
constexpr u32 kCtlFail = 12;
// global control words: [0] candidate ticket, [1] look-back ticket, [2] scan ticket, [3] some block wants the look-back pass,
// [128 .. 255] the fallback list's control (snp_launch_decompress_list: [128 + s] = length of sub-list s, [192] its ticket)
constexpr u32 kGlobWords = 256;
constexpr u32 kGlobList = 128;

__device__ __forceinline__ bool admitted(const u64* __restrict__ first, u32 b, u32 max_fragments)
{
    return first[b + 1] > first[b] && first[b + 1] <= max_fragments;
}
// packed[b] = (chunks before b) << 32 | (split blocks before b); a split block's tag-index slots start at chunks + 2 * blocks
__device__ __forceinline__ u64 slot_of(const u64* __restrict__ packed, u32 b) { return (packed[b] >> 32) + 2ull * static_cast<u32>(packed[b]); }

// ---- classify + plan -------------------------------------------------------------------------------------------------------------------------
// decl[b] = declared length of a candidate, else 0; hbv[b] = preamble bytes.  Workgroup 0 also zeroes the global words and d_result[2..3].
__global__ __launch_bounds__(256) void k_bd_classify(const u8* __restrict__ in, const u64* __restrict__ in_off, const u32* __restrict__ in_len,
                                                    const u32* __restrict__ out_cap, u32 nb, u32 par_min, u32* __restrict__ decl,
                                                    u32* __restrict__ hbv, u32* __restrict__ glob, u64* __restrict__ result)
{
    if (blockIdx.x == 0) {
        glob[threadIdx.x] = 0;
        if (threadIdx.x < 2) result[2 + threadIdx.x] = 0;
    }
    const u32 b = blockIdx.x * 256u + threadIdx.x;
    if (b >= nb) return;
    const u8* const p = in + in_off[b];
    const u32 n = in_len[b];
    const snp_preamble pre = snp_read_preamble(p, n);                     // (as decompress_spans reads it)
    const u32 expected = pre.value, hb = pre.bytes;
    const bool clean = pre.end == SNP_PRE_DONE;
    const u64 max_comp = 38ull + expected + expected / 6;                 // snp_max_compressed_length (which is -1 above 2^31 - 1)
    const bool cand = clean && par_min && expected >= par_min && expected <= out_cap[b] && n > hb && max_comp <= 0x7fffffffull && n <= max_comp;
    decl[b] = cand ? expected : 0u;
    hbv[b] = hb;
}

// fragments of a block chosen for splitting (the makespan rule), else 0
struct ScanChosen {
    const u32* __restrict__ decl;
    const u64* __restrict__ sum;                                          // the sum of decl (the candidates' declared bytes)
    u32 wave_slots;
    __device__ __forceinline__ u64 operator()(u64 i) const
    {
        const u64 d = decl[i];
        return d && d * wave_slots >= kSplitFactor * *sum ? (d + SNP_BLOCK_SIZE - 1) / SNP_BLOCK_SIZE : 0;
    }
};
// an admitted block: its chunks << 32 | 1
struct ScanAdmitted {
    const u64* __restrict__ first;
    const u32* __restrict__ in_len;
    const u32* __restrict__ hbv;
    u32 max_fragments;
    __device__ __forceinline__ u64 operator()(u64 i) const
    {
        const u32 b = static_cast<u32>(i);
        return admitted(first, b, max_fragments) ? (static_cast<u64>(snp_tag_chunks(in_len[b], hbv[b])) << 32) | 1u : 0;
    }
};

// masked lengths for the blocks' own decode; a split block's control words (the look-back flag set up front by the rule of
// snp_tag_index_look_back_only)
__global__ __launch_bounds__(256) void k_bd_begin(const u32* __restrict__ in_len, const u32* __restrict__ out_cap, u32 nb, const u64* __restrict__ first,
                                                 u32 max_fragments, const u32* __restrict__ decl, u32* __restrict__ m_in_len, u32* __restrict__ m_out_cap,
                                                 u32* __restrict__ ctl, u32* __restrict__ glob)
{
    const u32 b = blockIdx.x * 256u + threadIdx.x;
    if (b >= nb) return;
    const bool split = admitted(first, b, max_fragments);
    m_in_len[b] = split ? 0u : in_len[b];
    m_out_cap[b] = split ? 0u : out_cap[b];
    if (split) {
        u32* const c = ctl + static_cast<u64>(b) * kCtlWords;
        const bool lbo = snp_look_back_only(in_len[b], decl[b]);
        for (u32 i = 0; i < kCtlWords; ++i) c[i] = i == 2 && lbo ? 1u : 0u;
        if (lbo) glob[3] = 1;
    }
}

// the entry tables and hand-offs of the split blocks (only as many slots as the batch uses)
__global__ __launch_bounds__(256) void k_bd_zero(const u64* __restrict__ packed, u32 nb, u64* __restrict__ scanned, u64* __restrict__ looked,
                                                u32* __restrict__ hand)
{
    const u64 slots = slot_of(packed, nb);
    const u64 step = static_cast<u64>(gridDim.x) * 256u;
    for (u64 i = blockIdx.x * 256ull + threadIdx.x; i < slots * kSubs; i += step) {
        scanned[i] = 0;
        looked[i] = 0;
    }
    const u64 hw = slots * (sizeof(CandHandoff) / 4);
    for (u64 i = blockIdx.x * 256ull + threadIdx.x; i < hw; i += step) hand[i] = 0;
}

// ---- the batched tag index -------------------------------------------------------------------------------------------------------------------
struct Split {                                                            // one split block, as the tag-index kernels see it
    const u8* src;
    u32 n, hb, k, nchunks;
    u64 slot;
    ScanCtl* ctl;
};
__device__ __forceinline__ Split split_block(u32 b, const u8* in, const u64* in_off, const u32* in_len, const u32* hbv, const u64* packed, u32* ctl)
{
    Split s;
    s.src = in + in_off[b];
    s.n = in_len[b];
    s.hb = hbv[b];
    s.k = 0;
    s.nchunks = snp_tag_chunks(s.n, s.hb);
    s.slot = slot_of(packed, b);
    s.ctl = reinterpret_cast<ScanCtl*>(ctl + static_cast<u64>(b) * kCtlWords);
    return s;
}

// k_tag_cand over every chunk of every split block: persistent workgroups take one ticket at a time, in block-major chunk order, so a workgroup
// only ever waits on a neighbour with an earlier ticket (a block's chunk 0 never waits).  Look-back-only blocks are skipped.  The body per chunk
// is k_tag_cand's: cand_chunk (tag_index_device.h).
__global__ __launch_bounds__(kThreads) void k_bd_tag_cand(const u8* __restrict__ in, const u64* __restrict__ in_off, const u32* __restrict__ in_len,
                                                         const u32* __restrict__ hbv, u32 nb, const u64* __restrict__ packed, u32* __restrict__ ctl_all,
                                                         CandTable* __restrict__ tables_all, CandHandoff* __restrict__ hand_all, u32* __restrict__ glob)
{
    __shared__ u64 T[kChunk];
    __shared__ __attribute__((aligned(16))) u8 s_raw[kChunk + 16];
    __shared__ u32 s_ticket, s_b;
    __shared__ u32 s_land[kProbe];
    __shared__ u32 s_ncand;
    __shared__ u32 s_key[kMaxCand];
    __shared__ u32 s_next_ncand;
    __shared__ u32 s_next_key[kMaxCand];
    const u64 total = packed[nb] >> 32;
    for (;;) {
        if (threadIdx.x == 0) {
            const u32 tk = atomicAdd(&glob[0], 1u);
            s_ticket = tk;
            s_b = tk < total ? owner_of([=](u32 b) { return packed[b] >> 32; }, nb, tk) : 0u;
        }
        __syncthreads();
        const u32 tk = s_ticket;
        if (tk >= total) return;
        const Split B = split_block(s_b, in, in_off, in_len, hbv, packed, ctl_all);
        if (B.ctl->fallback == 0)
            cand_chunk(T, s_raw, s_land, s_ncand, s_key, s_next_ncand, s_next_key, B.src, B.n, B.hb, static_cast<u32>(tk - (packed[s_b] >> 32)),
                       tables_all + B.slot, hand_all + B.slot);
        __syncthreads();                                                  // (the LDS of this chunk is read until here)
    }
}

// k_tag_scan as persistent workgroups (one per RunCache slot) that take the split blocks by ticket.  A block whose scan gives up raises its
// look-back flag, and the batch's.
__global__ __launch_bounds__(kThreads) void k_bd_tag_scan(const u8* __restrict__ in, const u64* __restrict__ in_off, const u32* __restrict__ in_len,
                                                         const u32* __restrict__ hbv, u32 nb, const u64* __restrict__ packed, u32* __restrict__ ctl_all,
                                                         CandTable* __restrict__ tables_all, u64* __restrict__ scanned, RunCache* __restrict__ caches,
                                                         u32* __restrict__ glob)
{
    __shared__ __attribute__((aligned(16))) u8 pool[sizeof(FixLds) > sizeof(ScanLds) ? sizeof(FixLds) : sizeof(ScanLds)];
    __shared__ FixVars vars;
    __shared__ u32 s_final, s_more, s_ticket, s_b;
    const u32 nsplit = static_cast<u32>(packed[nb]);
    RunCache* const cache = caches + blockIdx.x;
    for (;;) {
        if (threadIdx.x == 0) {
            const u32 tk = atomicAdd(&glob[2], 1u);
            s_ticket = tk;
            s_b = tk < nsplit ? owner_of([=](u32 b) { return static_cast<u64>(static_cast<u32>(packed[b])); }, nb, tk) : 0u;
        }
        __syncthreads();
        if (s_ticket >= nsplit) return;
        const Split B = split_block(s_b, in, in_off, in_len, hbv, packed, ctl_all);
        ScanCtl* const ctl = B.ctl;
        if (__hip_atomic_load(&ctl->fallback, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0) {
            CandTable* const tables = tables_all + B.slot;
            u64* const entries = scanned + B.slot * kSubs;
            for (u32 pass = 0;; ++pass) {
                scan_pass(tables, B.n, B.hb, B.nchunks, entries, ctl, cache, pass >= min(kFixPasses, max(1u, B.nchunks / kChunksPerPass)),
                          *reinterpret_cast<ScanLds*>(pool), s_final);
                if (threadIdx.x == 0) s_more = ctl->complete == 0 && ctl->fallback == 0 && ctl->pending != 0;
                __syncthreads();
                if (!s_more) break;
                fix_pass(B.src, B.n, B.hb, tables, ctl, *reinterpret_cast<FixLds*>(pool), vars);
            }
            if (threadIdx.x == 0 && ctl->fallback) __hip_atomic_store(&glob[3], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        __syncthreads();
    }
}

// The look-back kernel (k_tag_index) over the chunks of the blocks that want it, by one global ticket in block-major chunk order as above; the
// body per chunk is look_back_chunk (tag_index_device.h).
__global__ __launch_bounds__(kThreads) void k_bd_tag_look_back(const u8* __restrict__ in, const u64* __restrict__ in_off, const u32* __restrict__ in_len,
                                                              const u32* __restrict__ hbv, u32 nb, const u64* __restrict__ packed, u32* __restrict__ ctl_all,
                                                              u64* __restrict__ looked, u32* __restrict__ glob)
{
    __shared__ u64 T[kChunk];
    __shared__ __attribute__((aligned(16))) u8 s_raw[kChunk + 16];
    __shared__ u32 s_ticket, s_b;
    if (__hip_atomic_load(&glob[3], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0) return;   // (every split block was indexed by its scan)
    const u64 total = packed[nb] >> 32;
    for (;;) {
        if (threadIdx.x == 0) {
            const u32 tk = atomicAdd(&glob[1], 1u);
            s_ticket = tk;
            s_b = tk < total ? owner_of([=](u32 b) { return packed[b] >> 32; }, nb, tk) : 0u;
        }
        __syncthreads();
        const u32 tk = s_ticket;
        if (tk >= total) return;
        const Split B = split_block(s_b, in, in_off, in_len, hbv, packed, ctl_all);
        if (__hip_atomic_load(&B.ctl->fallback, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0)
            look_back_chunk(T, s_raw, B.src, B.n, B.hb, static_cast<u32>(tk - (packed[s_b] >> 32)), looked + B.slot * kSubs);
        __syncthreads();                                                  // (the LDS of this chunk is read until here)
    }
}

// One thread per fragment slot: k_fragment_starts for the fragment's block, offsets made absolute.  Slots past the admitted blocks' fragments are
// inert (nothing to read, nothing to write).
__global__ __launch_bounds__(256) void k_bd_fragment_starts(const u64* __restrict__ in_off, const u32* __restrict__ in_len, const u64* __restrict__ out_off,
                                                           u32 nb, const u64* __restrict__ first, u32 max_fragments, const u32* __restrict__ decl,
                                                           const u32* __restrict__ hbv, const u64* __restrict__ packed, const u32* __restrict__ ctl_all,
                                                           const u64* __restrict__ scanned, const u64* __restrict__ looked,
                                                           u64* __restrict__ f_in_off, u32* __restrict__ f_in_len, u64* __restrict__ f_out_off,
                                                           u32* __restrict__ f_out_cap, u32* __restrict__ f_skip, u32* __restrict__ f_owner)
{
    const u32 f = blockIdx.x * 256u + threadIdx.x;
    if (f >= max_fragments) return;
    u64 io = 0, oo = 0;
    u32 il = 0, cap = 0, skip = 0, owner = kNone;
    if (f < first[nb]) {
        const u32 b = owner_of(first, nb, f);
        if (first[b + 1] <= max_fragments) {
            const u32 n = in_len[b], expected = decl[b];
            const u64 slot = slot_of(packed, b);
            const u32 nent = snp_tag_chunks(n, hbv[b]) * kSubs + 1;
            const u64* const entries = (ctl_all[static_cast<u64>(b) * kCtlWords + 2] ? looked : scanned) + slot * kSubs;
            const u32 target = static_cast<u32>(f - first[b]) * SNP_BLOCK_SIZE;
            const FragStart fs = fragment_start(entries, nent, n, expected, target);
            owner = b;
            oo = out_off[b] + target;
            cap = expected - target < SNP_BLOCK_SIZE ? expected - target : SNP_BLOCK_SIZE;
            io = in_off[b] + fs.ip;
            il = fs.good ? n - fs.ip : 0u;                                // (0: the fragment decoder reports "incomplete", the block falls back)
            skip = fs.skip;
        }
    }
    f_in_off[f] = io;
    f_in_len[f] = il;
    f_out_off[f] = oo;
    f_out_cap[f] = cap;
    f_skip[f] = skip;
    f_owner[f] = owner;
}

// ---- finalize ----------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_bd_fragment_check(const u32* __restrict__ f_owner, const i32* __restrict__ f_status, u32 max_fragments,
                                                          u32* __restrict__ ctl_all)
{
    const u32 f = blockIdx.x * 256u + threadIdx.x;
    if (f >= max_fragments) return;
    const u32 b = f_owner[f];
    if (b != kNone && f_status[f] != SNP_OK) ctl_all[static_cast<u64>(b) * kCtlWords + kCtlFail] = 1;
}

// One thread per block: a split block whose fragments all came back OK is OK with its declared length; the others go on the fallback list.
// d_result[1..3] += split OK, fell back, took the look-back pass (one atomic per wavefront each).
__global__ __launch_bounds__(256) void k_bd_finalize(u32 nb, const u64* __restrict__ first, u32 max_fragments, const u32* __restrict__ decl,
                                                    const u32* __restrict__ ctl_all, u32* __restrict__ out_len, i32* __restrict__ status,
                                                    u32* __restrict__ list, u32* __restrict__ glob, u64* __restrict__ result)
{
    const u32 b = blockIdx.x * 256u + threadIdx.x;
    u64 ok = 0, back = 0, lb = 0;
    if (b < nb && admitted(first, b, max_fragments)) {
        const u32* const c = ctl_all + static_cast<u64>(b) * kCtlWords;
        lb = c[2] != 0;
        if (c[kCtlFail] == 0) {
            out_len[b] = decl[b];
            status[b] = SNP_OK;
            ok = 1;
        } else {
            list[atomicAdd(&glob[kGlobList], 1u)] = b;
            back = 1;
        }
    }
    for (u32 d = 32; d >= 1; d >>= 1) {
        ok += __shfl_xor(ok, d, 64);
        back += __shfl_xor(back, d, 64);
        lb += __shfl_xor(lb, d, 64);
    }
    if ((threadIdx.x & 63u) == 0) {
        if (ok) atomicAdd(reinterpret_cast<unsigned long long*>(result + 1), static_cast<unsigned long long>(ok));
        if (back) atomicAdd(reinterpret_cast<unsigned long long*>(result + 2), static_cast<unsigned long long>(back));
        if (lb) atomicAdd(reinterpret_cast<unsigned long long*>(result + 3), static_cast<unsigned long long>(lb));
    }
}

// d_work layout (every piece 256-byte aligned; nothing when nbuffers is 0).  Per block: the classification, the masked lengths, the fallback list,
// the control words and three scans over nbuffers + 1 values with their tile sums; the global control words; per fragment slot: the fragment
// table; per tag-index slot (kSlotsPerFragment per fragment): scanned and looked-back entries (kSubs each), a hand-off, a candidate table; then
// one RunCache per scan workgroup.
struct DecodeWork {
    u32 *decl, *hbv, *m_in_len, *m_out_cap, *list, *ctl, *glob;
    u64 *sum, *first, *packed, *part;
    u64 *f_in_off, *f_out_off;
    u32 *f_in_len, *f_out_cap, *f_skip, *f_out_len, *f_owner;
    i32* f_status;
    u64 *scanned, *looked;
    CandHandoff* hand;
    CandTable* tables;
    RunCache* caches;
    u32 max_fragments, scan_wgs;
    u64 bytes;
};
DecodeWork decode_work_layout(void* base, u32 nbuffers, u32 max_fragments)
{
    DecodeWork w{};
    if (nbuffers == 0) return w;
    const u64 nb = nbuffers, nf = max_fragments < kMaxFragments ? max_fragments : kMaxFragments, ns = nf * kSlotsPerFragment;
    w.max_fragments = static_cast<u32>(nf);
    w.scan_wgs = static_cast<u32>(nf < kScanSlots ? nf : kScanSlots);
    WorkCarver k(base);
    w.decl = k.take<u32>(nb);
    w.hbv = k.take<u32>(nb);
    w.m_in_len = k.take<u32>(nb);
    w.m_out_cap = k.take<u32>(nb);
    w.list = k.take<u32>(nb);
    w.ctl = k.take<u32>(nb * kCtlWords);
    w.sum = k.take<u64>(nb + 1);
    w.first = k.take<u64>(nb + 1);
    w.packed = k.take<u64>(nb + 1);
    w.part = k.take<u64>(scan_tiles_of(nb));
    w.glob = k.take<u32>(kGlobWords);
    w.f_in_off = k.take<u64>(nf);
    w.f_out_off = k.take<u64>(nf);
    w.f_in_len = k.take<u32>(nf);
    w.f_out_cap = k.take<u32>(nf);
    w.f_skip = k.take<u32>(nf);
    w.f_out_len = k.take<u32>(nf);
    w.f_owner = k.take<u32>(nf);
    w.f_status = k.take<i32>(nf);
    w.scanned = k.take<u64>(ns * kSubs);
    w.looked = k.take<u64>(ns * kSubs);
    w.hand = k.take<CandHandoff>(ns);
    w.tables = k.take<CandTable>(ns);
    w.caches = k.take<RunCache>(w.scan_wgs);
    w.bytes = k.bytes();
    return w;
}

}  // namespace

extern "C" {

uint64_t snp_decompress_buffers_workspace(uint32_t nbuffers, uint32_t max_fragments)
{
    return decode_work_layout(nullptr, nbuffers, max_fragments).bytes;
}

snp_status snp_decompress_buffers_batch(snp_ctx* c, const uint8_t* in, const uint64_t* in_off, const uint32_t* in_len, uint32_t nbuffers,
                                        uint32_t max_fragments, uint8_t* out, const uint64_t* out_off, const uint32_t* out_cap, uint32_t* out_len,
                                        int32_t* status, void* d_work, uint64_t* d_result)
{
    if (!c || !d_result || (nbuffers && (!in || !in_off || !in_len || !out || !out_off || !out_cap || !out_len || !status || !d_work)))
        return SNP_ERR_BAD_ARG;
    DevGuard dg(c);
    if (!dg.ok) return SNP_ERR_DEVICE;
    hipStream_t s = c->stream;
    if (nbuffers == 0)
        return c->check(snp_zero_words_async(reinterpret_cast<u32*>(d_result), 2 * 4u, s), "buffers result") ? SNP_OK : SNP_ERR_DEVICE;   // 4 u64 words
    const DecodeWork w = decode_work_layout(d_work, nbuffers, max_fragments);
    const u32 nb = nbuffers, M = w.max_fragments, grid_b = (nb + 255u) / 256u;
    const int dec_mode = c->fenced | ((c->dec_lds / 256) << 8);
    // classify + plan: d_result[0] = fragments the chosen blocks need, d_result[1..3] = 0
    hipLaunchKernelGGL(k_bd_classify, dim3(grid_b), dim3(256), 0, s, in, in_off, in_len, out_cap, nb, c->par_min, w.decl, w.hbv, w.glob, d_result);
    bool ok = c->check(hipGetLastError(), "buffers classify") &&
              c->check(launch_scan(ScanPlain{w.decl}, nb, w.part, w.sum, nullptr, s), "buffers scan") &&
              c->check(launch_scan(ScanChosen{w.decl, w.sum + nb, c->persistent_waves()}, nb, w.part, w.first, d_result, s), "buffers scan");
    if (!ok) return SNP_ERR_DEVICE;
    if (M == 0) {                                                        // nothing can be split: the call is snp_decompress_batch
        return c->launch_decompress(in, in_off, in_len, nb, out, out_off, out_cap, out_len, status, nullptr) ? SNP_OK : SNP_ERR_DEVICE;
    }
    const u32 cus = c->persistent_waves() / 32u;
    const u32 index_wgs = std::min<u64>(cus, static_cast<u64>(M) * 5);
    hipLaunchKernelGGL(k_bd_begin, dim3(grid_b), dim3(256), 0, s, in_len, out_cap, nb, w.first, M, w.decl, w.m_in_len, w.m_out_cap, w.ctl, w.glob);
    ok = c->check(hipGetLastError(), "buffers begin") &&
         c->check(launch_scan(ScanAdmitted{w.first, in_len, w.hbv, M}, nb, w.part, w.packed, nullptr, s), "buffers scan");
    // the tag index of every split block
    hipLaunchKernelGGL(k_bd_zero, dim3(1024), dim3(256), 0, s, w.packed, nb, w.scanned, w.looked, reinterpret_cast<u32*>(w.hand));
    hipLaunchKernelGGL(k_bd_tag_cand, dim3(index_wgs), dim3(kThreads), 0, s, in, in_off, in_len, w.hbv, nb, w.packed, w.ctl, w.tables, w.hand, w.glob);
    hipLaunchKernelGGL(k_bd_tag_scan, dim3(std::min(w.scan_wgs, cus)), dim3(kThreads), 0, s, in, in_off, in_len, w.hbv, nb, w.packed, w.ctl, w.tables,
                       w.scanned, w.caches, w.glob);
    hipLaunchKernelGGL(k_bd_tag_look_back, dim3(index_wgs), dim3(kThreads), 0, s, in, in_off, in_len, w.hbv, nb, w.packed, w.ctl, w.looked, w.glob);
    hipLaunchKernelGGL(k_bd_fragment_starts, dim3((M + 255u) / 256u), dim3(256), 0, s, in_off, in_len, out_off, nb, w.first, M, w.decl, w.hbv, w.packed,
                       w.ctl, w.scanned, w.looked, w.f_in_off, w.f_in_len, w.f_out_off, w.f_out_cap, w.f_skip, w.f_owner);
    ok = ok && c->check(hipGetLastError(), "buffers tag index");
    // the fragments, then every other block by snp_decompress_batch's policy (a split block has nothing to read and no room there)
    ok = ok && c->check(snp_launch_decompress(in, w.f_in_off, w.f_in_len, M, out, w.f_out_off, w.f_out_cap, w.f_out_len, w.f_status, nullptr, dec_mode, s,
                                              w.f_skip), "decompress fragments");
    ok = ok && c->launch_decompress(in, in_off, w.m_in_len, nb, out, out_off, w.m_out_cap, out_len, status, nullptr);
    // finalize; the split blocks that did not come back OK are decoded again, one wavefront each
    if (ok) {
        hipLaunchKernelGGL(k_bd_fragment_check, dim3((M + 255u) / 256u), dim3(256), 0, s, w.f_owner, w.f_status, M, w.ctl);
        hipLaunchKernelGGL(k_bd_finalize, dim3(grid_b), dim3(256), 0, s, nb, w.first, M, w.decl, w.ctl, out_len, status, w.list, w.glob, d_result);
        ok = c->check(hipGetLastError(), "buffers finalize") &&
             c->check(snp_launch_decompress_list(in, in_off, in_len, nb, out, out_off, out_cap, out_len, status, nullptr, dec_mode, s, w.list,
                                                 w.glob + kGlobList, std::min(c->persistent_waves(), static_cast<u32>(M)), nb), "decompress (fallback list)");
    }
    return ok ? SNP_OK : SNP_ERR_DEVICE;
}

}  // extern "C"

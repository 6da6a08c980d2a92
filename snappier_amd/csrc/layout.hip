// layout.hip -- snp_decompress_layout_batch / snp_frame_decode_layout_batch: the decoded length of every item of a device batch and the output
// layout (out_off, out_cap) the batch decoders take, from the compressed bytes alone: snp_get_uncompressed_length (capi_ctx.hip) and
// snp_frame_decoded_length (capi_frame.hip) over a whole batch, on the device, followed by the placement a host would do with their answers.
// Built into libsnappier_hip_layout.so (C-ABI: include/snappier_hip_layout.h), linked against libsnappier_hip.so.  DESIGN.md 4.12.
//
// Blocks:
//   probe     one thread per buffer: the varint preamble (at most 5 bytes) -> status, declared; the expansion rule of frame_hop
//   scan      slot = declared rounded up to align for an OK buffer, else 0 -> each buffer's offset (scan_tiles.h, multi-workgroup)
//   first     one thread per buffer: the OK buffers whose range ends beyond arena_cap, minimum index into d_result[1] (one atomic per wavefront)
//   write     four buffers per thread: out_off, out_cap, the status of the buffers at or behind the first one that does not fit, and the
//             workgroup-reduced sums of d_result
// Framed streams: the span scan, walk A and walk B of snp_frame_decode_buffers_batch (frame_walk_device.h) with no capacity bound, then the same
// scan / first / write over the totals the resolver found (every walked stream takes part, whatever ended its walk).
// Nothing here allocates, reads back or synchronises, and nothing is kept in the context: both calls are capturable.
#include "capi_internal.h"
#include "frame_walk_device.h"
#include "../../include/snappier_hip_layout.h"

namespace {

__device__ __forceinline__ u64 slot_of(u64 len, u32 align) { return (len + (align - 1)) & ~static_cast<u64>(align - 1); }

// ---- what the two calls share ------------------------------------------------------------------------------------------------------------------
// d_result before the atomics: [0] = 0 (a maximum), [1] = n (a minimum), the others 0.  `skip` is the word a scan has already written.
__global__ void k_lay_result_init(u64* result, u32 words, u32 n, u32 skip)
{
    const u32 i = threadIdx.x;
    if (i < words && i != skip) result[i] = i == 1 ? n : 0;
}

// ---- blocks ------------------------------------------------------------------------------------------------------------------------------------
// snp_get_uncompressed_length (VarIntEncoding.TryReadSlow  VarIntEncoding.Read.cs:38-79) on at most 5 bytes, then frame_hop's expansion rule
__global__ __launch_bounds__(256) void k_bl_probe(const u8* __restrict__ in, const u64* __restrict__ in_off, const u32* __restrict__ in_len, u32 nb,
                                                 u32* __restrict__ declared, i32* __restrict__ status)
{
    const u32 b = blockIdx.x * 256u + threadIdx.x;
    if (b >= nb) return;
    const u32 n = in_len[b];
    const u8* const p = in + in_off[b];
    const snp_preamble pre = snp_read_preamble(p, n);
    i32 st = SNP_ERR_BAD_LENGTH;
    u32 dec = 0;
    if (pre.end == SNP_PRE_DONE) {
        // (a block that declares more can only end "Incomplete Snappy block.": frame_hop, frame_hop_device.h)
        const bool fits = pre.value <= snp_max_expansion(n - pre.bytes);
        st = fits ? SNP_OK : SNP_ERR_INCOMPLETE;
        dec = fits ? pre.value : 0;
    }
    declared[b] = dec;
    status[b] = st;
}

struct ScanBlockSlots {
    const i32* __restrict__ status;
    const u32* __restrict__ declared;
    u32 align;
    __device__ __forceinline__ u64 operator()(u64 i) const { return status[i] == SNP_OK ? slot_of(declared[i], align) : 0; }
};

__global__ __launch_bounds__(256) void k_bl_first(u32 nb, const u64* __restrict__ off, const u32* __restrict__ declared, const i32* __restrict__ status,
                                                 u64 arena_cap, u64* __restrict__ result)
{
    const u32 b = blockIdx.x * 256u + threadIdx.x;
    u64 mine = ~0ull;
    if (b < nb && status[b] == SNP_OK && off[b] + declared[b] > arena_cap) mine = b;
    mine = wave_min(mine);
    if ((threadIdx.x & 63u) == 0 && mine != ~0ull) atomic_min64(result + 1, mine);
}

// kWriteItems items per thread and one set of atomics per WORKGROUP: the atomics all land on the same three words, and at 163 840 buffers one set
// per wavefront cost more than everything else in the call together
constexpr u32 kWriteItems = 4;
constexpr u32 kWriteTile = 256 * kWriteItems;

// the workgroup's maximum of a and sums of b and c, valid in thread 0
__device__ __forceinline__ void wg_reduce3(u64& a, u64& b, u64& c)
{
    __shared__ u64 s_red[3][256 / SNP_WAVE];
    a = wave_max(a);
    b = wave_sum(b);
    c = wave_sum(c);
    const u32 wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63u) == 0) { s_red[0][wave] = a; s_red[1][wave] = b; s_red[2][wave] = c; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (u32 w = 1; w < 256 / SNP_WAVE; ++w) {
            a = s_red[0][w] > a ? s_red[0][w] : a;
            b += s_red[1][w];
            c += s_red[2][w];
        }
    }
}

__global__ __launch_bounds__(256) void k_bl_write(u32 nb, const u64* __restrict__ off, const u32* __restrict__ declared, u64* __restrict__ out_off,
                                                 u32* __restrict__ out_cap, i32* __restrict__ status, u64* __restrict__ result)
{
    const u64 f = result[1];                                            // (k_bl_first has finished: the launches are in stream order)
    u64 end = 0, frags = 0, bytes = 0;
    for (u32 k = 0; k < kWriteItems; ++k) {
        const u64 b = static_cast<u64>(blockIdx.x) * kWriteTile + k * 256u + threadIdx.x;
        if (b >= nb) break;
        const u64 o = off[b];
        u32 cap = 0;
        if (status[b] == SNP_OK) {
            const u32 d = declared[b];
            end = o + d;                                                // (offsets grow with b: the last one is the largest)
            if (b >= f) {
                status[b] = SNP_ERR_OUTPUT_TOO_SMALL;
            } else {
                cap = d;
                frags += (static_cast<u64>(d) + SNP_BLOCK_SIZE - 1) / SNP_BLOCK_SIZE;
                bytes += d;
            }
        }
        out_off[b] = o;
        out_cap[b] = cap;
    }
    wg_reduce3(end, frags, bytes);
    if (threadIdx.x == 0) {
        if (end) atomic_max64(result + 0, end);
        if (frags) atomic_add64(result + 2, frags);
        if (bytes) atomic_add64(result + 3, bytes);
    }
}

// ---- framed streams ----------------------------------------------------------------------------------------------------------------------------
struct ScanStreamSlots {
    const u64* __restrict__ sfirst;
    const u64* __restrict__ total;
    u32 max_spans, align;
    __device__ __forceinline__ u64 operator()(u64 i) const { return sfirst[i + 1] <= max_spans ? slot_of(total[i], align) : 0; }
};

__global__ __launch_bounds__(256) void k_fl_first(u32 ns, const u64* __restrict__ sfirst, u32 max_spans, const u64* __restrict__ off,
                                                 const u64* __restrict__ total, u64 arena_cap, u64* __restrict__ result)
{
    const u32 b = blockIdx.x * 256u + threadIdx.x;
    u64 mine = ~0ull;
    if (b < ns && (sfirst[b + 1] > max_spans || off[b] + total[b] > arena_cap)) mine = b;
    mine = wave_min(mine);
    if ((threadIdx.x & 63u) == 0 && mine != ~0ull) atomic_min64(result + 1, mine);
}

__global__ __launch_bounds__(256) void k_fl_write(u32 ns, const u64* __restrict__ sfirst, u32 max_spans, const u64* __restrict__ off, FbStreams st,
                                                 u64* __restrict__ out_off, u64* __restrict__ out_cap, u64* __restrict__ decoded_len,
                                                 u32* __restrict__ nchunks, i32* __restrict__ status, u64* __restrict__ result)
{
    const u64 f = result[1];
    u64 end = 0, chunks = 0, unused = 0;
    for (u32 k = 0; k < kWriteItems; ++k) {
        const u64 b = static_cast<u64>(blockIdx.x) * kWriteTile + k * 256u + threadIdx.x;
        if (b >= ns) break;
        u64 o = 0, cap = 0, len = 0;
        u32 nc = 0;
        i32 s = SNP_ERR_OUTPUT_TOO_SMALL;
        if (sfirst[b + 1] <= max_spans) {                               // walked
            o = off[b];
            len = st.total[b];
            nc = st.nc[b];
            end = o + len;
            if (b < f) {
                s = st.tail[b];
                cap = len;
                chunks += nc;
            }
        }
        out_off[b] = o;
        out_cap[b] = cap;
        decoded_len[b] = len;
        nchunks[b] = nc;
        status[b] = s;
    }
    wg_reduce3(end, chunks, unused);
    if (threadIdx.x == 0) {
        if (end) atomic_max64(result + 0, end);
        if (chunks) atomic_add64(result + 3, chunks);
    }
}

// ---- workspaces (every piece 256-byte aligned; nothing when there is no item) ------------------------------------------------------------------
// blocks: each buffer's offset (nb + 1) and the tile sums of its scan
struct BlockWork {
    u64 *off, *part;
    u64 bytes;
};
BlockWork block_work_layout(void* base, u32 nbuffers)
{
    BlockWork w{};
    if (nbuffers == 0) return w;
    const u64 nb = nbuffers;
    WorkCarver k(base);
    w.off = k.take<u64>(nb + 1);
    w.part = k.take<u64>(scan_tiles_of(nb));
    w.bytes = k.bytes();
    return w;
}

// framed streams: first span slot and offset of every stream (ns + 1 each), the tile sums of their scans, the walk's record; per span slot the
// candidates and the resolver's entry (the span half of frame_buffers.hip's decode workspace)
struct StreamWork {
    u64 *sfirst, *off, *part;
    FbStreams st;
    FbSpans sp;
    u64 bytes;
};
StreamWork stream_work_layout(void* base, u32 nstreams, u32 max_spans)
{
    StreamWork w{};
    if (nstreams == 0) return w;
    const u64 ns = nstreams, nsp = max_spans;
    WorkCarver k(base);
    w.sfirst = k.take<u64>(ns + 1);
    w.off = k.take<u64>(ns + 1);
    w.part = k.take<u64>(scan_tiles_of(ns));
    carve_span_walk(k, ns, nsp, w.st, w.sp);
    w.bytes = k.bytes();
    return w;
}

bool align_ok(u32 align) { return align >= 1 && align <= (1u << 20) && (align & (align - 1)) == 0; }

}  // namespace

extern "C" {

uint64_t snp_decompress_layout_workspace(uint32_t nbuffers)
{
    return block_work_layout(nullptr, nbuffers).bytes;
}

snp_status snp_decompress_layout_batch(snp_ctx* c, const uint8_t* in, const uint64_t* in_off, const uint32_t* in_len, uint32_t nbuffers,
                                       uint32_t align, uint64_t arena_cap, uint64_t* out_off, uint32_t* out_cap, uint32_t* declared,
                                       int32_t* status, void* d_work, uint64_t* d_result)
{
    if (!c || !d_result || !align_ok(align) || (nbuffers && (!in || !in_off || !in_len || !out_off || !out_cap || !declared || !status || !d_work)))
        return SNP_ERR_BAD_ARG;
    DevGuard dg(c);
    if (!dg.ok) return SNP_ERR_DEVICE;
    hipStream_t s = c->stream;
    const u32 nb = nbuffers, groups = static_cast<u32>((static_cast<u64>(nb) + 255) / 256);
    const u32 wgroups = static_cast<u32>((static_cast<u64>(nb) + kWriteTile - 1) / kWriteTile);
    hipLaunchKernelGGL(k_lay_result_init, dim3(1), dim3(64), 0, s, d_result, 4u, nb, ~0u);
    if (nb == 0) return c->check(hipGetLastError(), "layout result") ? SNP_OK : SNP_ERR_DEVICE;
    const BlockWork w = block_work_layout(d_work, nb);
    hipLaunchKernelGGL(k_bl_probe, dim3(groups), dim3(256), 0, s, in, in_off, in_len, nb, declared, status);
    bool ok = c->check(hipGetLastError(), "layout probe") &&
              c->check(launch_scan(ScanBlockSlots{status, declared, align}, nb, w.part, w.off, nullptr, s), "layout scan");
    if (ok) {
        hipLaunchKernelGGL(k_bl_first, dim3(groups), dim3(256), 0, s, nb, w.off, declared, status, arena_cap, d_result);
        hipLaunchKernelGGL(k_bl_write, dim3(wgroups), dim3(256), 0, s, nb, w.off, declared, out_off, out_cap, status, d_result);
        ok = c->check(hipGetLastError(), "layout write");
    }
    return ok ? SNP_OK : SNP_ERR_DEVICE;
}

uint64_t snp_frame_decode_layout_workspace(uint32_t nstreams, uint32_t max_spans)
{
    return stream_work_layout(nullptr, nstreams, max_spans).bytes;
}

snp_status snp_frame_decode_layout_batch(snp_ctx* c, const uint8_t* in, const uint64_t* in_off, const uint64_t* in_len, uint32_t nstreams,
                                         uint32_t max_spans, uint32_t align, uint64_t arena_cap, uint64_t* out_off, uint64_t* out_cap,
                                         uint64_t* decoded_len, uint32_t* nchunks, int32_t* status, void* d_work, uint64_t* d_result)
{
    if (!c || !d_result || !align_ok(align) ||
        (nstreams && (!in || !in_off || !in_len || !out_off || !out_cap || !decoded_len || !nchunks || !status || !d_work)))
        return SNP_ERR_BAD_ARG;
    DevGuard dg(c);
    if (!dg.ok) return SNP_ERR_DEVICE;
    hipStream_t s = c->stream;
    const u32 ns = nstreams, S = max_spans, groups = static_cast<u32>((static_cast<u64>(ns) + 255) / 256);
    const u32 wgroups = static_cast<u32>((static_cast<u64>(ns) + kWriteTile - 1) / kWriteTile);
    if (ns == 0) {
        hipLaunchKernelGGL(k_lay_result_init, dim3(1), dim3(64), 0, s, d_result, 5u, 0u, ~0u);
        return c->check(hipGetLastError(), "layout result") ? SNP_OK : SNP_ERR_DEVICE;
    }
    const StreamWork w = stream_work_layout(d_work, ns, S);
    // the span walk of the decode call: first span slot of every stream (d_result[2] = span slots needed), candidates, one chain per stream with
    // no capacity bound (d_result[4] += spans resolved on the spot)
    bool ok = c->check(launch_span_scan(in_len, ns, w.part, w.sfirst, d_result + 2, s), "layout span scan");
    if (ok) {
        hipLaunchKernelGGL(k_lay_result_init, dim3(1), dim3(64), 0, s, d_result, 5u, ns, 2u);   // (after the scan wrote [2], before the resolver adds into [4])
        ok = c->check(launch_span_walk(in, in_off, in_len, nullptr, ns, w.sfirst, S, w.sp, w.st, d_result + 4, s), "layout walk");
    }
    ok = ok && c->check(launch_scan(ScanStreamSlots{w.sfirst, w.st.total, S, align}, ns, w.part, w.off, nullptr, s), "layout scan");
    if (ok) {
        hipLaunchKernelGGL(k_fl_first, dim3(groups), dim3(256), 0, s, ns, w.sfirst, S, w.off, w.st.total, arena_cap, d_result);
        hipLaunchKernelGGL(k_fl_write, dim3(wgroups), dim3(256), 0, s, ns, w.sfirst, S, w.off, w.st, out_off, out_cap, decoded_len, nchunks, status,
                           d_result);
        ok = c->check(hipGetLastError(), "layout write");
    }
    return ok ? SNP_OK : SNP_ERR_DEVICE;
}

}  // extern "C"

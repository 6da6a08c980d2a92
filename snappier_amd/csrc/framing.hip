// framing.hip -- device side of the Snappy framing format (SnappyStreamCompressor.cs:18-21,194-261) and the
// segment gather used to concatenate independently compressed fragments (SnappyCompressor.cs:40-80 writes them
// back to back).  Pure data movement: 256-thread workgroups, 16 B per lane.
#include "frame_hop_device.h"

namespace {

__global__ __launch_bounds__(256) void k_gather(const u8* __restrict__ src, const u64* __restrict__ src_off,
                                               const u32* __restrict__ seg_len, u8* __restrict__ dst,
                                               const u64* __restrict__ dst_off, u32 nseg)
{
    const u32 s = blockIdx.x;
    if (s >= nseg) return;
    block_copy(dst + dst_off[s], src + src_off[s], seg_len[s], threadIdx.x);
}

// Chunk table of a raw stream cut into 65536-byte chunks (SnappyStreamCompressor.CompressInput  :166-192)
__global__ void k_frame_chunks(u64 n, u32 nchunks, u64 comp_stride, u64* in_off, u32* in_len, u64* comp_off)
{
    const u32 c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= nchunks) return;
    const u64 o = static_cast<u64>(c) * SNP_BLOCK_SIZE;
    in_off[c] = o;
    in_len[c] = static_cast<u32>(n - o < SNP_BLOCK_SIZE ? n - o : SNP_BLOCK_SIZE);
    comp_off[c] = static_cast<u64>(c) * comp_stride;
}

// Per chunk: compressed-vs-raw decision (CompressBlock  :212-229) and the exclusive scan of encoded sizes.
// Single 1024-thread workgroup; dst_off has nchunks + 1 entries, the last one is the total encoded length.
__global__ __launch_bounds__(1024) void k_frame_plan(const u32* __restrict__ in_len, const u32* __restrict__ comp_len,
                                                    u32 nchunks, u8* __restrict__ type, u32* __restrict__ payload,
                                                    u64* __restrict__ dst_off, u64* __restrict__ total)
{
    __shared__ u64 wave_sum[16];
    __shared__ u64 carry;
    const u32 tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    if (tid == 0) carry = SNP_STREAM_HEADER_LEN;
    __syncthreads();
    for (u32 base = 0; base < nchunks; base += 1024) {
        const u32 i = base + tid;
        u64 v = 0;
        if (i < nchunks) {
            const bool shrink = comp_len[i] < in_len[i];                // :212
            const u32 pl = shrink ? comp_len[i] : in_len[i];
            type[i] = shrink ? 0 : 1;
            payload[i] = pl;
            v = SNP_CHUNK_HEADER_LEN + pl;
        }
        u64 x = v;
        for (u32 d = 1; d < 64; d <<= 1) {
            const u64 y = __shfl_up(x, d, 64);
            if (lane >= d) x += y;
        }
        if (lane == 63) wave_sum[wave] = x;
        __syncthreads();
        if (wave == 0) {
            u64 s = lane < 16 ? wave_sum[lane] : 0;
            for (u32 d = 1; d < 16; d <<= 1) {
                const u64 y = __shfl_up(s, d, 64);
                if (lane >= d) s += y;
            }
            if (lane < 16) wave_sum[lane] = s;
        }
        __syncthreads();
        const u64 excl = carry + (wave ? wave_sum[wave - 1] : 0) + x - v;
        if (i < nchunks) dst_off[i] = excl;
        __syncthreads();
        if (tid == 1023) carry = excl + v;
        __syncthreads();
    }
    if (tid == 0) {
        dst_off[nchunks] = carry;
        *total = carry;
    }
}

__constant__ u8 k_stream_header[SNP_STREAM_HEADER_LEN] = {0xff, 0x06, 0x00, 0x00, 0x73, 0x4e, 0x61, 0x50, 0x70, 0x59};   // :18-21

__global__ void k_frame_header_only(u8* dst, u64* total)
{
    if (threadIdx.x < SNP_STREAM_HEADER_LEN) dst[threadIdx.x] = k_stream_header[threadIdx.x];
    if (threadIdx.x == 0) *total = SNP_STREAM_HEADER_LEN;
}

// One workgroup per chunk: [type:1][len:3 LE = payload + 4][masked crc:4 LE][payload]   (:233-261)
__global__ __launch_bounds__(256) void k_frame_emit(const u8* __restrict__ raw, const u64* __restrict__ in_off,
                                                   const u8* __restrict__ comp, const u64* __restrict__ comp_off,
                                                   const u8* __restrict__ type, const u32* __restrict__ payload,
                                                   const u32* __restrict__ crc, const u64* __restrict__ dst_off,
                                                   u8* __restrict__ dst, u64 cap, u32 nchunks)
{
    const u32 c = blockIdx.x, tid = threadIdx.x;
    if (c >= nchunks) return;
    if (dst_off[nchunks] > cap) return;                                 // caller reports OUTPUT_TOO_SMALL from the total
    if (c == 0 && tid < SNP_STREAM_HEADER_LEN) dst[tid] = k_stream_header[tid];   // EnsureStreamHeaderWritten  :148-157
    const u64 o = dst_off[c];
    const u32 pl = payload[c];
    const u32 t = type[c];
    chunk_header(dst + o, tid, t, pl, crc[c]);
    const u8* src = t == 0 ? comp + comp_off[c] : raw + in_off[c];
    block_copy(dst + o + SNP_CHUNK_HEADER_LEN, src, pl, tid);
}


// ---- device-side chunk-header walk (SnappyStreamDecompressor.ReadChunkHeader / Decompress  :53-199,215-289) -----
// A framed stream carries no index: every header gives the position of the next one, so the walk is a serial chain of
// ~64 KiB hops (frame_hop of frame_hop_device.h: one 16-byte load per chunk -- type, 24-bit size, masked CRC and the first bytes of the block
// preamble).  One lane walks; the table it writes is exactly what the host walk in capi_frame.hip produces.  Entries past the last data
// chunk are filled as empty uncompressed chunks so that the decode and CRC launches can run over max_chunks without
// knowing the count on the host.
__global__ __launch_bounds__(SNP_WAVE) void k_frame_scan(const u8* __restrict__ in, u64 n, u64 cap, u32 max_chunks, ChunkRows r,
                                                        u64* __restrict__ hdr /* total, tail status, chunks */)
{
    __shared__ u64 s_total;
    __shared__ u32 s_nc;
    if (threadIdx.x == 0) {
        u64 ip = 0, total = 0;
        u32 nc = 0;
        i32 tail = SNP_OK;
        // for_span_chunks (frame_hop_device.h) over the whole stream, written out: as its visitor this loop came out 35 instructions longer
        for (;;) {
            const Hop h = frame_hop(in, n, ip);
            if (h.kind == HOP_END) break;
            if (h.kind == HOP_ERR) { tail = h.err; break; }
            if (h.kind == HOP_DATA) {
                if (nc == max_chunks) { tail = SNP_ERR_OUTPUT_TOO_SMALL; break; }   // chunk table full
                chunk_row_set(r, nc, h, ip, total);
                total += h.dec;
                ++nc;
            }
            ip = h.next;
        }
        if (total > cap) { tail = SNP_ERR_OUTPUT_TOO_SMALL; nc = 0; total = 0; }   // nothing is decoded
        hdr[0] = total;
        hdr[1] = static_cast<u64>(static_cast<u32>(tail));
        hdr[2] = nc;
        s_total = total;
        s_nc = nc;
    }
    __syncthreads();
    const u64 total = s_total;
    for (u32 k = s_nc + threadIdx.x; k < max_chunks; k += SNP_WAVE) chunk_row_clear(r, k, total);
}

// The stream's verdict: the first failing chunk in stream order (as the sequential reference would throw), else the
// error that ended the header walk, else OK with the byte count.
__global__ __launch_bounds__(256) void k_frame_result(const i32* __restrict__ status, const u64* __restrict__ hdr,
                                                     u64* __restrict__ result)
{
    __shared__ u32 s_first;
    if (threadIdx.x == 0) s_first = 0xffffffffu;
    __syncthreads();
    const u32 nc = static_cast<u32>(hdr[2]);
    u32 first = 0xffffffffu;
    for (u32 k = threadIdx.x; k < nc; k += 256)
        if (status[k] != SNP_OK) { first = k; break; }
    if (first != 0xffffffffu) atomicMin(&s_first, first);
    __syncthreads();
    if (threadIdx.x == 0) {
        i32 st = static_cast<i32>(hdr[1]);
        if (s_first != 0xffffffffu) st = status[s_first];
        result[0] = st == SNP_OK ? hdr[0] : 0;
        result[1] = static_cast<u64>(static_cast<u32>(st));
    }
}

}  // namespace

extern "C" hipError_t snp_launch_gather(const u8* src, const u64* src_off, const u32* seg_len, u8* dst,
                                        const u64* dst_off, u32 nseg, hipStream_t stream)
{
    if (nseg == 0) return hipSuccess;
    hipLaunchKernelGGL(k_gather, dim3(nseg), dim3(256), 0, stream, src, src_off, seg_len, dst, dst_off, nseg);
    return hipGetLastError();
}

extern "C" hipError_t snp_launch_frame_chunks(u64 n, u32 nchunks, u64 comp_stride, u64* in_off, u32* in_len,
                                              u64* comp_off, hipStream_t stream)
{
    if (nchunks == 0) return hipSuccess;
    hipLaunchKernelGGL(k_frame_chunks, dim3((nchunks + 255) / 256), dim3(256), 0, stream, n, nchunks, comp_stride,
                       in_off, in_len, comp_off);
    return hipGetLastError();
}

extern "C" hipError_t snp_launch_frame_plan(const u32* in_len, const u32* comp_len, u32 nchunks, u8* type, u32* payload,
                                            u64* dst_off, u64* total, hipStream_t stream)
{
    hipLaunchKernelGGL(k_frame_plan, dim3(1), dim3(1024), 0, stream, in_len, comp_len, nchunks, type, payload, dst_off,
                       total);
    return hipGetLastError();
}

extern "C" hipError_t snp_launch_frame_header_only(u8* dst, u64* total, hipStream_t stream)
{
    hipLaunchKernelGGL(k_frame_header_only, dim3(1), dim3(64), 0, stream, dst, total);
    return hipGetLastError();
}

extern "C" hipError_t snp_launch_frame_emit(const u8* raw, const u64* in_off, const u8* comp, const u64* comp_off,
                                            const u8* type, const u32* payload, const u32* crc, const u64* dst_off,
                                            u8* dst, u64 cap, u32 nchunks, hipStream_t stream)
{
    if (nchunks == 0) return hipSuccess;
    hipLaunchKernelGGL(k_frame_emit, dim3(nchunks), dim3(256), 0, stream, raw, in_off, comp, comp_off, type, payload,
                       crc, dst_off, dst, cap, nchunks);
    return hipGetLastError();
}

extern "C" hipError_t snp_launch_frame_scan(const u8* in, u64 n, u64 cap, u32 max_chunks, const ChunkRows& r, u64* hdr, hipStream_t stream)
{
    hipLaunchKernelGGL(k_frame_scan, dim3(1), dim3(SNP_WAVE), 0, stream, in, n, cap, max_chunks, r, hdr);
    return hipGetLastError();
}

extern "C" hipError_t snp_launch_frame_result(const i32* status, const u64* hdr, u64* result, hipStream_t stream)
{
    hipLaunchKernelGGL(k_frame_result, dim3(1), dim3(256), 0, stream, status, hdr, result);
    return hipGetLastError();
}

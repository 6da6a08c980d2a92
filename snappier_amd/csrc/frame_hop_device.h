// frame_hop_device.h -- one hop of a framed stream's chunk-header walk, and the span walk built on it: the device code that the one-stream
// header walks (the serial one of framing.hip, k_frame_scan, and the span walk of frame_scan.hip: snp_frame_decode_device) and the batched
// one (frame_buffers.hip, snp_frame_decode_buffers_batch) share.  The rules of one hop (frame_hop) are those of the host walk in
// capi_frame.hip (scan_chunks); the block preamble and the expansion bound inside it are snp_rules.h's.
#pragma once
#include "snp_rules.h"

namespace {

constexpr u64 kSpan = 1ull << 20;
constexpr u32 kWindow = 80 * 1024;          // > 8 + MaxCompressedLength(65536): the next header after any spec-sized data chunk
constexpr u32 kMaxCand = 4;                 // candidates kept per span (the lowest plausible positions of its window)
constexpr u32 kEmptyMaskedCrc = 0xa282ead8u;   // crc32c_mask(crc32c of no bytes)
constexpr u64 kNoEntry = ~0ull;

enum HopKind : u32 { HOP_DATA = 0, HOP_SKIP = 1, HOP_END = 2, HOP_ERR = 3 };

struct Hop {
    u32 kind;
    i32 err;        // HOP_ERR: the status that ends the walk
    u32 type;       // HOP_DATA: 0 compressed, 1 uncompressed
    u32 body_len, crc, dec;
    u64 next;       // position of the next header
};

// One header at ip (< n or == n).  Same rules, in the same order, as scan_chunks (capi_frame.hip) / the reference reader.
__device__ __forceinline__ Hop frame_hop(const u8* __restrict__ in, u64 n, u64 ip)
{
    Hop h{};
    h.next = ip;
    if (ip >= n) { h.kind = HOP_END; return h; }
    if (n - ip < 4) { h.kind = HOP_ERR; h.err = SNP_ERR_TRUNCATED_STREAM; return h; }
    u32 b[4] = {0, 0, 0, 0};                                            // 16 bytes at ip (fewer at the very end)
    if (n - ip >= 16) {
        const snp_u128_unaligned q = *reinterpret_cast<const snp_u128_unaligned*>(in + ip);
        b[0] = q.v[0]; b[1] = q.v[1]; b[2] = q.v[2]; b[3] = q.v[3];
    } else {
        for (u32 i = 0; i < static_cast<u32>(n - ip); ++i) b[i >> 2] |= static_cast<u32>(in[ip + i]) << (8 * (i & 3));
    }
    const u32 t = b[0] & 0xffu;
    const u32 size = b[0] >> 8;                                         // :64-65
    if (n - (ip + 4) < size) { h.kind = HOP_ERR; h.err = SNP_ERR_TRUNCATED_STREAM; return h; }
    h.next = ip + 4 + size;
    if (t <= 1) {
        if (size < 4) { h.kind = HOP_ERR; h.err = SNP_ERR_TRUNCATED_STREAM; return h; }
        u32 dec = size - 4;
        if (t == 0) {                                                   // block preamble  VarIntEncoding.Read.cs:38-79
            const snp_preamble pre = snp_read_preamble(b[2] | (static_cast<u64>(b[3]) << 32), size - 4);
            if (pre.end != SNP_PRE_DONE || pre.value > 0x7fffffffu) { h.kind = HOP_ERR; h.err = SNP_ERR_BAD_LENGTH; return h; }
            dec = pre.value;
            // (such a chunk can only end "Incomplete Snappy block.": capi_frame.hip scan_chunks)
            if (dec > snp_max_expansion(size - 4 - pre.bytes)) { h.kind = HOP_ERR; h.err = SNP_ERR_INCOMPLETE; return h; }
        }
        h.kind = HOP_DATA;
        h.type = t;
        h.body_len = size - 4;
        h.crc = b[1];                                                   // ReadChunkCrc  :260-289
        h.dec = dec;
        return h;
    }
    if (t < 0x80) { h.kind = HOP_ERR; h.err = SNP_ERR_CHUNK_TYPE; return h; }   // :182-185
    h.kind = HOP_SKIP;                                                  // 0x80..0xff skipped unvalidated  :187-196
    return h;
}

// "Could the true chain enter here?"  Only shapes a spec-conforming writer emits are candidates (a data chunk of at most
// 65536 raw bytes, or the stream identifier); everything else still DECODES -- it just is not guessed, the resolver walks it.
// Compressed payload is full of bytes that look like a raw-chunk header (0x01 is the commonest copy tag, followed by small
// numbers: ~3e-4 of positions), so a candidate must also be FOLLOWED by such a shape, or end the stream: ~1e-8.
__device__ __forceinline__ bool chunk_shape(const u8* __restrict__ in, u64 n, u64 p, u64* next)
{
    if (n - p < 8) return false;
    const u32 w0 = ld32u(in + p);
    const u32 t = w0 & 0xffu, size = w0 >> 8;
    *next = p + 4 + size;
    if (t == 0xffu) return size == 6 && n - p >= 10 && ld32u(in + p + 4) == 0x50614e73u && in[p + 8] == 0x70 && in[p + 9] == 0x59;
    if (t > 1) return false;
    if (n - (p + 4) < size) return false;
    if (t == 1) return size >= 4 && size <= 65536 + 4;
    if (size < 5 || size > 76496 + 4) return false;
    const Hop h = frame_hop(in, n, p);
    return h.kind == HOP_DATA && h.dec <= 65536;
}
__device__ __forceinline__ bool plausible_start(const u8* __restrict__ in, u64 n, u64 p)
{
    u64 next = 0, next2 = 0;
    if (!chunk_shape(in, n, p, &next)) return false;
    return next == n || chunk_shape(in, n, next, &next2);
}

// What following a chain from `start` to the end of its span yields.
struct Chain {
    u64 exit;       // position of the first header at or beyond the span's end (or where the chain stopped)
    u64 dec;        // bytes declared by the data chunks met
    u32 ndata;      // data chunks met
    i32 stop;       // 0: left the span; -1: clean end of stream; > 0: the status that ended it (chunks before it still count)
};

__device__ __forceinline__ Chain follow_chain(const u8* __restrict__ in, u64 n, u64 start, u64 span_end)
{
    Chain c{start, 0, 0, 0};
    u64 ip = start;
    while (ip < span_end) {
        const Hop h = frame_hop(in, n, ip);
        if (h.kind == HOP_END) { c.stop = -1; break; }
        if (h.kind == HOP_ERR) { c.stop = h.err; break; }
        if (h.kind == HOP_DATA) { ++c.ndata; c.dec += h.dec; }
        ip = h.next;
    }
    if (c.stop == 0 && ip >= n) c.stop = ip == n ? -1 : 0;   // ip > n cannot happen (a body never runs past n)
    c.exit = ip;
    return c;
}

}  // namespace

// frame_hop_device.h -- what every header walk of a framed stream is made of, for ONE stream and one span of it: one hop of the chunk-header chain
// (frame_hop, __host__ __device__: the host walk of capi_frame.hip is a loop over it too), the candidate test, the chain walk, the span table and
// the chunk table with their places in a workspace, and the per-span bodies of the span walk -- the candidates of a span (walk A), the lookup of a
// span's entry among the candidates of 64 spans (walk B), the hops over a span's data chunks from its entry (walk C) and the empty row.  Its users
// are thin drivers that find their stream and span: the one-stream walks (framing.hip k_frame_scan, frame_scan.hip k_span_*:
// snp_frame_decode_device), the many-stream walk (frame_walk_device.h k_fd_candidates, k_fd_resolve) and the kernels behind it (frame_buffers.hip,
// frame_range.hip, frame_index.hip) and the row check of the indexed read (frame_index_device.h, which calls frame_hop on the host too).  What belongs to MANY streams -- the per-stream record, the span slots of a batch, the launches -- is frame_walk_device.h.
// The block preamble and the expansion bound inside a hop are snp_rules.h's.
#pragma once
#include "snp_rules.h"
#include "work_carver.h"

namespace {

constexpr u64 kSpan = 1ull << 20;
constexpr u32 kWindow = 80 * 1024;          // > 8 + MaxCompressedLength(65536): the next header after any spec-sized data chunk
constexpr u32 kMaxCand = 4;                 // candidates kept per span (the lowest plausible positions of its window)
constexpr u32 kEmptyMaskedCrc = 0xa282ead8u;   // crc32c_mask(crc32c of no bytes)
constexpr u64 kNoEntry = ~0ull;
constexpr u32 kNone = 0xffffffffu;

// ---- the two tables ------------------------------------------------------------------------------------------------------------------------------
// per span slot, structure of arrays ([n][kMaxCand] for the candidates; count = candidates kept, the lowest positions); positions are stream-relative
struct FbSpans {
    u32* count;
    u32* start_rel;     // start - span * kSpan
    u64* exit;
    u64* dec;
    u32* ndata;
    i32* stop;
    // resolver -> emitter
    u64* entry;         // true entry of the span, kNoEntry if the chain never starts a header inside it
    u32* chunk_base;    // the stream's data chunks before the span
    u64* out_base;      // the stream's decoded bytes before the span
};
inline FbSpans carve_spans(WorkCarver& k, u64 n)
{
    FbSpans sp;
    sp.count = k.take<u32>(n);
    sp.start_rel = k.take<u32>(n * kMaxCand);
    sp.exit = k.take<u64>(n * kMaxCand);
    sp.dec = k.take<u64>(n * kMaxCand);
    sp.ndata = k.take<u32>(n * kMaxCand);
    sp.stop = k.take<i32>(n * kMaxCand);
    sp.entry = k.take<u64>(n);
    sp.chunk_base = k.take<u32>(n);
    sp.out_base = k.take<u64>(n);
    return sp;
}

// the chunk table (ChunkRows, capi_internal.h) over n rows of a d_work workspace
inline ChunkRows carve_chunk_rows(WorkCarver& k, u64 n)
{
    ChunkRows r;
    r.body_off = k.take<u64>(n);
    r.out_off = k.take<u64>(n);
    r.body_len = k.take<u32>(n);
    r.crc = k.take<u32>(n);
    r.out_cap = k.take<u32>(n);
    r.out_len = k.take<u32>(n);
    r.tag = k.take<u32>(n);
    r.status = k.take<i32>(n);
    r.type = k.take<u8>(n);
    return r;
}
// Row i as an empty raw chunk with the CRC of nothing: the decoder and the CRC verify read and write nothing for it and report OK, so they run
// over a whole table without the host knowing how many rows are in use.  (A table with tags sets the row's tag itself.)
__device__ __forceinline__ void chunk_row_clear(const ChunkRows& r, u64 i, u64 out_off)
{
    r.type[i] = 1;
    r.body_off[i] = 0;
    r.body_len[i] = 0;
    r.crc[i] = kEmptyMaskedCrc;
    r.out_off[i] = out_off;
    r.out_cap[i] = 0;
}

enum HopKind : u32 { HOP_DATA = 0, HOP_SKIP = 1, HOP_END = 2, HOP_ERR = 3 };

struct Hop {
    u32 kind;
    i32 err;        // HOP_ERR: the status that ends the walk
    u32 type;       // HOP_DATA: 0 compressed, 1 uncompressed
    u32 body_len, crc, dec;
    u64 next;       // position of the next header
};

// One header at ip (< n or == n): the rules of the reference reader, in its order.  The only statement of them: the host walk calls it too.
__host__ __device__ __forceinline__ Hop frame_hop(const u8* __restrict__ in, u64 n, u64 ip)
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
            // a chunk that declares more than its body can possibly produce (snp_rules.h) can only end "Incomplete Snappy block."
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

// Row i of a chunk table as the data chunk a hop found: its header at byte `header` of the input, its output at out_off.
__device__ __forceinline__ void chunk_row_set(const ChunkRows& r, u64 i, const Hop& h, u64 header, u64 out_off)
{
    r.type[i] = static_cast<u8>(h.type);
    r.body_off[i] = header + SNP_CHUNK_HEADER_LEN;
    r.body_len[i] = h.body_len;
    r.crc[i] = h.crc;
    r.out_off[i] = out_off;
    r.out_cap[i] = h.dec;
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

// ---- the per-span bodies of the span walk ----------------------------------------------------------------------------------------------------------
// Walk A, one wavefront per span: the candidates of span k of the stream (p, n) into s_cand, their count into *s_n (both in LDS) and back.  Span 0
// enters at byte 0, whatever is there.  Otherwise the kMaxCand LOWEST plausible positions of the span's first kWindow bytes: the true entry is the
// first true header of the span, and fewer than kMaxCand false positives precede it except in adversarial payloads (then the resolver walks the
// span itself).  All lanes must call it.
__device__ __forceinline__ u32 span_candidates(const u8* __restrict__ p, u64 n, u64 k, u32* s_cand, u32* s_n)
{
    const u32 lane = lane_id();
    const u64 s0 = k * kSpan;
    const u64 s1 = s0 + kSpan < n ? s0 + kSpan : n;
    if (lane == 0) *s_n = 0;
    __syncthreads();
    if (k == 0) {
        if (lane == 0) { s_cand[0] = 0; *s_n = 1; }
    } else {
        const u64 wend = s0 + kWindow < s1 ? s0 + kWindow : s1;
        for (u64 base = s0; base < wend; base += SNP_WAVE) {
            const u64 q = base + lane;
            const bool ok = q < wend && plausible_start(p, n, q);
            const u64 m = ballot64(ok);
            if (m) {
                const u32 have = *s_n;
                if (ok) {
                    const u32 idx = have + static_cast<u32>(__builtin_popcountll(m & lanes_below(lane)));
                    if (idx < kMaxCand) s_cand[idx] = static_cast<u32>(q - s0);
                }
                __syncthreads();
                if (lane == 0) { const u32 tot = have + static_cast<u32>(__builtin_popcountll(m)); *s_n = tot < kMaxCand ? tot : kMaxCand; }
                __syncthreads();
                if (*s_n == kMaxCand) break;
            }
        }
    }
    __syncthreads();
    return *s_n;
}
// ... and slot g of the span table: lane c follows candidate c's chain to the end of the span
__device__ __forceinline__ void span_candidates_row(const FbSpans& t, u64 g, const u8* __restrict__ p, u64 n, u64 k, const u32* s_cand, u32 count)
{
    const u32 lane = lane_id();
    if (lane == 0) t.count[g] = count;
    if (lane < count) {
        const Chain c = follow_chain(p, n, k * kSpan + s_cand[lane], (k + 1) * kSpan);
        const u64 i = g * kMaxCand + lane;
        t.start_rel[i] = s_cand[lane];
        t.exit[i] = c.exit;
        t.dec[i] = c.dec;
        t.ndata[i] = c.ndata;
        t.stop[i] = c.stop;
    }
}

// Walk B, one wavefront per stream: lane l holds the candidates of span batch0 + l of the stream whose first span slot is g0; the chain is
// followed with readlane, so a hop from span to span costs ~20 scalar instructions and no memory.
struct SpanBatch {
    u64 batch0 = ~0ull;                                                 // first span of the batch held in registers
    u32 srel[kMaxCand] = {}, cnd[kMaxCand] = {};
    i32 cst[kMaxCand] = {};
    u64 cex[kMaxCand] = {}, cde[kMaxCand] = {};

    // makes span k one of the 64 held (k is wave-uniform)
    __device__ __forceinline__ void load(const FbSpans& t, u64 g0, u64 nspans, u64 k)
    {
        if (k >= batch0 && k < batch0 + SNP_WAVE) return;
        batch0 = k;
        const u64 mine = batch0 + lane_id();
        const u64 gi = g0 + mine;
        const u32 cnt = mine < nspans ? t.count[gi] : 0;
#pragma unroll
        for (u32 j = 0; j < kMaxCand; ++j) {
            const bool have = mine < nspans && j < cnt;
            srel[j] = have ? t.start_rel[gi * kMaxCand + j] : 0xffffffffu;
            cex[j] = have ? t.exit[gi * kMaxCand + j] : 0;
            cde[j] = have ? t.dec[gi * kMaxCand + j] : 0;
            cnd[j] = have ? t.ndata[gi * kMaxCand + j] : 0;
            cst[j] = have ? t.stop[gi * kMaxCand + j] : 0;
        }
    }
    // the chain of the candidate of span k (held) that starts at e, if there is one
    __device__ __forceinline__ bool find(u64 e, u64 k, Chain* c) const
    {
        const u32 l = static_cast<u32>(k - batch0);
        const u32 rel = static_cast<u32>(e - k * kSpan);
        bool found = false;
#pragma unroll
        for (u32 j = 0; j < kMaxCand; ++j) {
            if (!found && read_lane(srel[j], l) == rel) {
                found = true;
                c->exit = (static_cast<u64>(read_lane(static_cast<u32>(cex[j] >> 32), l)) << 32) | read_lane(static_cast<u32>(cex[j]), l);
                c->dec = (static_cast<u64>(read_lane(static_cast<u32>(cde[j] >> 32), l)) << 32) | read_lane(static_cast<u32>(cde[j]), l);
                c->ndata = read_lane(cnd[j], l);
                c->stop = static_cast<i32>(read_lane(static_cast<u32>(cst[j]), l));
            }
        }
        return found;
    }
};

// Walk C, one lane: the hops from `entry` while the header lies below span_end and the data chunk index below idx_end.  visit(h, ip, idx, off) sees
// every data chunk -- the hop, its header's position, its index in the stream and the decoded bytes before it -- and returns false to stop.
// Returns what ended the hops, as Chain::stop: 0 a bound or the visitor, -1 the clean end of the stream, > 0 the status of a bad header.
template <class Visit>
__device__ __forceinline__ i32 for_span_chunks(const u8* __restrict__ p, u64 n, u64 entry, u64 span_end, u32 idx, u32 idx_end, u64 off, Visit visit)
{
    u64 ip = entry;
    while (ip < span_end && idx < idx_end) {
        const Hop h = frame_hop(p, n, ip);
        if (h.kind == HOP_END) return -1;
        if (h.kind == HOP_ERR) return h.err;
        if (h.kind == HOP_DATA) {
            if (!visit(h, ip, idx, off)) break;
            off += h.dec;
            ++idx;
        }
        ip = h.next;
    }
    return 0;
}

}  // namespace

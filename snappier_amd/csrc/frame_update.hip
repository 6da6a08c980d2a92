// frame_update.hip -- snp_frame_write_indexed_batch: requests that replace decoded bytes of framed streams kept with their chunk index, answered by
// new streams in which only the chunks the requests touch are compressed again and every other byte is a copy.  The write half of
// frame_index.hip's indexed read: its planning (frame_index_device.h) finds the rows, frame_update_device.h adds what a write needs on top.
// Built into libsnappier_hip_frame_update.so (C-ABI: include/snappier_hip_frame_update.h), linked against libsnappier_hip.so.  DESIGN.md 4.16.
//
//   plan      one thread per request (fu_plan): order against the predecessor, place in the request list, ix_plan, the range, the edge rows
//   own       scan of the requests with rows -> each one's predecessor; one thread per request: the rows it owns (fu_own), their decoded bytes
//   scans     owned rows -> each request's first dirty slot; owned bytes -> its place among its stream's staged bytes
//   check     one thread per dirty slot, grid-stride (the host does not know their number): fu_row_check; the size change of the row's chunk
//   streams   one thread per stream: its requests (two searches), named / passed, its slots and bytes
//   scans     slots and bytes of the streams that passed -> admission in stream order; d_result[0], [2]
//   slots     one thread per table slot: its stream, request and row, the hop, its place in staging; the decode row of an edge slot
//   decode    snp_ctx::decode_chunks over the table (edges only; every other row is empty) into raw staging; fail: a failing edge -> its stream
//   overlay   one workgroup per request and 64 KiB piece: src -> raw staging, over the decoded edges
//   compress  snp_ctx::launch_compress over every slot, varint on; crc: snp_launch_crc32c over every slot -- once each, from the raw staging
//   scans     new and old chunk sizes per slot -> the shift of everything behind a slot
//   sizes     one thread per stream: size, status, out_len, out_bound, d_result[1] and [3]; requests: one thread per request, req_status
//   emit      one 256-thread workgroup per 64 KiB of an OLD stream that is written, grid-stride: the clean runs at their shifted place, the new
//             chunks that start in the range
//   new_pos   (only when asked) one thread per index row: a search in its stream's slots
// Nothing here allocates, reads back or synchronises: the call is capturable like the other _batch entry points.
#include "capi_internal.h"
#include "frame_rewrite_device.h"
#include "frame_update_device.h"
#include "../../include/snappier_hip_frame_update.h"

namespace {

constexpr u32 kHead = 0x100u, kLast = 0x200u, kLive = 0x400u;       // request flags above the status byte: edges, r0 < r1
constexpr u32 kNamed = 1u, kPassed = 2u, kWritten = 4u;             // stream flags
constexpr u32 kOverlayPieces = 8;                                   // workgroups that share one request's bytes
constexpr u32 kMaxGroups = 8192;                                    // grid of the grid-stride check

__device__ __forceinline__ u64 fail_key(u32 r, i32 status) { return (static_cast<u64>(r) << 8) | static_cast<u64>(status & 0xff); }

struct UpArgs {
    const u8* in;
    const u64 *in_off, *in_len;
    u32 ns;
    FrameIndex x;
    FuRequests q;
};
// per request: the plan, the owned rows, the scans over the requests (n + 1 each)
struct UpReq {
    u64 *r0, *r1, *own0, *cnt, *bytes;
    u64 *live, *sfirst, *bfirst;        // requests with rows before r; dirty slots before r; owned decoded bytes before r
    u32* flags;
};
// per stream
struct UpStreams {
    u64 *fail, *delta;                  // min over the failing requests of fail_key; sum over the dirty chunks of new bound - old size
    u64 *slot0, *nslots, *byte0, *nbytes, *units;
    u64 *aslots, *abytes, *gfirst;      // scans (n + 1): slots / bytes of the passed streams before b; emit units of the written streams before b
    u32* flags;
};
// per table slot
struct UpSlots {
    u64 *pos, *place, *coff, *row;      // the old header (stream-relative), the raw and the compressed staging offsets, the index row
    u64 *nscan, *oscan;                 // scans (n + 1) of the new and the old chunk sizes
    u32 *old, *dec, *stream, *req, *comp_len, *crc;
    i32* c_status;
};

struct ScanLive {
    const u32* __restrict__ flags;
    __device__ __forceinline__ u64 operator()(u64 i) const { return (flags[i] & kLive) != 0; }
};
struct ScanOld {
    const u32* __restrict__ old;
    __device__ __forceinline__ u64 operator()(u64 i) const { return old[i]; }
};

// admission in stream order: both sums only grow
struct Admit {
    const u32* flags;
    const u64* __restrict__ aslots;
    const u64* __restrict__ abytes;
    u32 max_slots;
    u64 stage_cap;
    __device__ __forceinline__ bool operator()(u32 b) const { return (flags[b] & kPassed) && aslots[b + 1] <= max_slots && abytes[b + 1] <= stage_cap; }
};

__global__ __launch_bounds__(256) void k_fu_init(u32 ns, UpStreams st)
{
    const u32 b = blockIdx.x * 256u + threadIdx.x;
    if (b >= ns) return;
    st.fail[b] = kNoFail;
    st.delta[b] = 0;
}

__global__ __launch_bounds__(256) void k_fu_plan(UpArgs a, UpReq rq, UpStreams st)
{
    const u32 r = blockIdx.x * 256u + threadIdx.x;
    if (r >= a.q.n) return;
    const FuPlan k = fu_plan(a.x, a.ns, a.q, r, [&](u32 b) { return a.in + a.in_off[b]; }, [&](u32 b) { return a.in_len[b]; });
    rq.r0[r] = k.r0;
    rq.r1[r] = k.r1;
    rq.flags[r] = static_cast<u32>(k.status) | (k.head ? kHead : 0u) | (k.last ? kLast : 0u) | (k.status == SNP_OK && k.r0 < k.r1 ? kLive : 0u);
    const u32 b = a.q.stream[r];
    if (k.status != SNP_OK && b < a.ns) atomic_min64(st.fail + b, fail_key(r, k.status));
}

// the previous request with rows, if it is one of stream b: its r1
__device__ __forceinline__ bool pred_of(const UpArgs& a, const UpReq& rq, u32 r, u32 b, u64* pred_r1)
{
    const u64 e = rq.live[r];
    if (e == 0) return false;
    const u32 p = owner_of(static_cast<const u64*>(rq.live), a.q.n, e - 1);
    if (a.q.stream[p] != b) return false;
    *pred_r1 = rq.r1[p];
    return true;
}

__global__ __launch_bounds__(256) void k_fu_own(UpArgs a, UpReq rq, UpStreams st)
{
    const u32 r = blockIdx.x * 256u + threadIdx.x;
    if (r >= a.q.n) return;
    u32 flags = rq.flags[r];
    u64 own0 = rq.r0[r], cnt = 0, bytes = 0;
    if (flags & kLive) {
        const u32 b = a.q.stream[r];
        u64 pr1 = 0;
        const bool has = pred_of(a, rq, r, b, &pr1);
        const FuOwn o = fu_own(rq.r0[r], rq.r1[r], has, pr1);
        if (o.status != SNP_OK) {
            flags = (flags & ~0xffu) | static_cast<u32>(o.status);
            rq.flags[r] = flags;
            atomic_min64(st.fail + b, fail_key(r, o.status));
        }
        own0 = o.own0;
        cnt = o.cnt;
        if (cnt) {
            const u64 f1 = a.x.first[b + 1] < a.x.nentries ? a.x.first[b + 1] : a.x.nentries;
            bytes = ix_row_end(a.x, f1, a.x.total[b], rq.r1[r] - 1) - a.x.start[own0];
        }
    }
    rq.own0[r] = own0;
    rq.cnt[r] = cnt;
    rq.bytes[r] = bytes;
}

// One thread per dirty slot of the whole call, admitted or not: the check of its row, and what its chunk adds to its stream's size bound.
__global__ __launch_bounds__(256) void k_fu_check(UpArgs a, UpReq rq, UpStreams st)
{
    const u64 total = rq.sfirst[a.q.n];
    for (u64 c = static_cast<u64>(blockIdx.x) * 256u + threadIdx.x; c < total; c += static_cast<u64>(gridDim.x) * 256u) {
        const u32 r = owner_of(static_cast<const u64*>(rq.sfirst), a.q.n, c);
        const u32 b = a.q.stream[r], flags = rq.flags[r];
        const u64 i = rq.own0[r] + (c - rq.sfirst[r]);
        const FuPlan pl{SNP_OK, (flags & kHead) != 0, (flags & kLast) != 0, rq.r0[r], rq.r1[r]};
        const IxPlan k = fu_window(a.x, b, a.q.off[r], a.q.len[r]);
        bool has_prev = true;
        u64 prev = i - 1;
        if (c == rq.sfirst[r]) {
            u64 pr1 = 0;
            has_prev = pred_of(a, rq, r, b, &pr1);
            prev = pr1 - 1;
        }
        Hop h{};
        if (!fu_row_check(a.x, a.in + a.in_off[b], a.in_len[b], k, pl, i, has_prev, prev, &h)) atomic_min64(st.fail + b, fail_key(r, SNP_ERR_BAD_ARG));
        else if (h.dec) atomic_add64(st.delta + b, (SNP_CHUNK_HEADER_LEN + static_cast<u64>(h.dec)) - (h.next - a.x.pos[i]));    // (the old chunk ends at the next header)
    }
}

__global__ __launch_bounds__(256) void k_fu_streams(UpArgs a, UpReq rq, UpStreams st)
{
    const u32 b = blockIdx.x * 256u + threadIdx.x;
    if (b >= a.ns) return;
    const u64 lb = fu_lower(a.q, b), ub = fu_lower(a.q, static_cast<u64>(b) + 1);
    const bool failed = st.fail[b] != kNoFail;
    const bool named = failed || (lb < ub && a.q.stream[lb] == b);
    const bool passed = named && !failed;
    st.slot0[b] = rq.sfirst[lb];
    st.byte0[b] = rq.bfirst[lb];
    st.nslots[b] = passed ? rq.sfirst[ub] - rq.sfirst[lb] : 0;
    st.nbytes[b] = passed ? rq.bfirst[ub] - rq.bfirst[lb] : 0;
    st.flags[b] = (named ? kNamed : 0u) | (passed ? kPassed : 0u);
}

// where row i, owned by request o of stream b, lies in the raw staging
__device__ __forceinline__ u64 place_of(const UpArgs& a, const UpReq& rq, const UpStreams& st, u32 b, u32 o, u64 i)
{
    return st.abytes[b] + (rq.bfirst[o] - st.byte0[b]) + (a.x.start[i] - a.x.start[rq.own0[o]]);
}

__global__ __launch_bounds__(256) void k_fu_slots(UpArgs a, UpReq rq, UpStreams st, Admit admit, UpSlots sl, ChunkRows rows, u64 empty_base)
{
    const u32 t = blockIdx.x * 256u + threadIdx.x;
    if (t >= admit.max_slots) return;
    u64 pos = 0, place = 0, coff = empty_base + 64ull * t, row = 0;
    u32 old = 0, dec = 0, stream = kNone, req = 0;
    rows.tag[t] = kNone;
    chunk_row_clear(rows, t, 0);
    if (t < st.aslots[a.ns]) {
        const u32 b = owner_of(static_cast<const u64*>(st.aslots), a.ns, t);
        if (admit(b)) {
            const u64 c = st.slot0[b] + (t - st.aslots[b]);
            const u32 r = owner_of(static_cast<const u64*>(rq.sfirst), a.q.n, c);
            const u64 i = rq.own0[r] + (c - rq.sfirst[r]);
            const Hop h = frame_hop(a.in + a.in_off[b], a.in_len[b], a.x.pos[i]);
            if (h.kind == HOP_DATA && h.dec <= kFuMaxDec) {              // (what k_fu_check saw: the stream passed)
                const u32 flags = rq.flags[r];
                stream = b;
                req = r;
                row = i;
                pos = a.x.pos[i];
                dec = h.dec;
                old = dec ? SNP_CHUNK_HEADER_LEN + h.body_len : 0u;                       // a zero-length chunk stays as it is
                place = place_of(a, rq, st, b, r, i);
                coff = (place + place / 6 + 15) / 16 * 16 + 96ull * t;
                const bool edge = (i == rq.r0[r] && (flags & kHead)) || (i == rq.r1[r] - 1 && (flags & kLast));
                if (edge && dec) {
                    rows.tag[t] = t;
                    chunk_row_set(rows, t, h, a.in_off[b] + pos, place);
                }
            }
        }
    }
    sl.pos[t] = pos;
    sl.place[t] = place;
    sl.coff[t] = coff;
    sl.row[t] = row;
    sl.old[t] = old;
    sl.dec[t] = dec;
    sl.stream[t] = stream;
    sl.req[t] = req;
}

// an edge that did not decode or verify: its status to the request that dirtied it first
__global__ __launch_bounds__(256) void k_fu_fail(u32 max_slots, ChunkRows rows, UpSlots sl, UpStreams st)
{
    const u32 t = blockIdx.x * 256u + threadIdx.x;
    if (t >= max_slots || rows.tag[t] == kNone) return;
    const i32 s = row_verdict(rows, t);
    if (s != SNP_OK) atomic_min64(st.fail + sl.stream[t], fail_key(sl.req[t], s));
}

// len bytes by the 256 threads of a workgroup, src and dst apart and misaligned differently for every run: the destination is brought to a
// 16-byte boundary by byte stores, then aligned 16-byte stores from unaligned 16-byte loads: team_copy (frame_chunked_device.h) with T = 256
// and a 64-bit length.  It stays: with team_copy in its place k_fu_overlay came out at 338 instructions for 276 and k_fu_emit at 472 for 402
// (profiles/r21a_refactor_kernel_stats.md).  All threads must call it.
__device__ __forceinline__ void wg_copy(u8* dst, const u8* src, u64 len, u32 t)
{
    if (len < 64) {
        if (t < len) dst[t] = src[t];
        return;
    }
    const u32 head = static_cast<u32>(16u - (reinterpret_cast<uintptr_t>(dst) & 15u)) & 15u;
    if (t < head) dst[t] = src[t];
    const u64 body = (len - head) & ~15ull;
    for (u64 k = t * 16ull; k < body; k += 256 * 16) {
        const snp_u128_unaligned w = *reinterpret_cast<const snp_u128_unaligned*>(src + head + k);
        *reinterpret_cast<uint4*>(dst + head + k) = make_uint4(w.v[0], w.v[1], w.v[2], w.v[3]);
    }
    const u64 done = head + body;
    if (t < len - done) dst[done + t] = src[done + t];                  // (< 16 bytes)
}

// One workgroup per request and piece: the request's bytes over its rows in the raw staging (the rows a request writes into are neighbours there).
__global__ __launch_bounds__(256) void k_fu_overlay(UpArgs a, UpReq rq, UpStreams st, Admit admit, const u8* __restrict__ src,
                                                   const u64* __restrict__ src_off, u8* __restrict__ stage)
{
    const u32 r = blockIdx.x;
    const u32 flags = rq.flags[r];
    if ((flags & 0xffu) != SNP_OK || !(flags & kLive)) return;
    const u32 b = a.q.stream[r];
    if (!admit(b) || st.fail[b] != kNoFail) return;
    const u64 r0 = rq.r0[r];
    // the owner of row r0: the request itself, or the one that owns the slot before its own
    const u32 o = rq.own0[r] == r0 ? r : owner_of(static_cast<const u64*>(rq.sfirst), a.q.n, rq.sfirst[r] - 1);
    u8* const dst = stage + place_of(a, rq, st, b, o, r0) + (a.q.off[r] - a.x.start[r0]);
    const u8* const from = src + src_off[r];
    const u64 len = a.q.len[r];
    for (u64 at = blockIdx.y * kUnit; at < len; at += gridDim.y * kUnit) wg_copy(dst + at, from + at, len - at < kUnit ? len - at : kUnit, threadIdx.x);
}

__global__ __launch_bounds__(256) void k_fu_sizes(UpArgs a, UpStreams st, Admit admit, UpSlots sl, const u64* __restrict__ out_cap,
                                                 u64* __restrict__ out_len, i32* __restrict__ status, u64* __restrict__ out_bound,
                                                 u64* __restrict__ result)
{
    const u32 b = blockIdx.x * 256u + threadIdx.x;
    u64 ok_len = 0, ok = 0;
    if (b < a.ns) {
        u32 flags = st.flags[b];
        i32 s = SNP_OK;
        u64 bound = 0;
        if (flags & kNamed) {
            const u64 fail = st.fail[b];
            if (fail != kNoFail) {
                s = static_cast<i32>(fail & 0xff);
            } else {
                bound = a.in_len[b] + st.delta[b];
                s = SNP_ERR_OUTPUT_TOO_SMALL;
                if (admit(b)) {
                    const u64 t0 = st.aslots[b], t1 = st.aslots[b + 1];
                    u64 size = a.in_len[b];
                    if (t1 > t0) size = size - (sl.oscan[t1] - sl.oscan[t0]) + (sl.nscan[t1] - sl.nscan[t0]);
                    if (size <= out_cap[b]) {
                        s = SNP_OK;
                        ok_len = size;
                        ok = 1;
                        flags |= kWritten;
                    }
                }
            }
        }
        status[b] = s;
        out_len[b] = ok_len;
        if (out_bound) out_bound[b] = bound;
        st.flags[b] = flags;
        st.units[b] = ok ? (a.in_len[b] + kUnit - 1) / kUnit : 0;
    }
    ok_len = wave_sum(ok_len);
    ok = wave_sum(ok);
    if ((threadIdx.x & 63u) == 0 && ok) {
        atomic_add64(result + 1, ok_len);
        atomic_add64(result + 3, ok);
    }
}

__global__ __launch_bounds__(256) void k_fu_requests(UpArgs a, UpReq rq, const i32* __restrict__ status, i32* __restrict__ req_status)
{
    const u32 r = blockIdx.x * 256u + threadIdx.x;
    if (r >= a.q.n) return;
    const i32 own = static_cast<i32>(rq.flags[r] & 0xffu);
    req_status[r] = own != SNP_OK ? own : status[a.q.stream[r]];        // (own OK: the stream number is one)
}

// how far everything behind the dirty slots [t0, j) of a stream has moved
__device__ __forceinline__ u64 shift_of(const UpSlots& sl, u64 t0, u64 j) { return (sl.nscan[j] - sl.nscan[t0]) - (sl.oscan[j] - sl.oscan[t0]); }

// One workgroup per 64 KiB of an old stream that is written.  Everything that steers it is uniform over the workgroup.
__global__ __launch_bounds__(256) void k_fu_emit(UpArgs a, UpStreams st, UpSlots sl, const u8* __restrict__ raw, const u8* __restrict__ comp,
                                                u8* __restrict__ out, const u64* __restrict__ out_off)
{
    const u32 tid = threadIdx.x;
    const u64 units = st.gfirst[a.ns];
    for (u64 g = blockIdx.x; g < units; g += gridDim.x) {
        const u32 b = owner_of(static_cast<const u64*>(st.gfirst), a.ns, g);
        const u64 n = a.in_len[b], lo = (g - st.gfirst[b]) * kUnit, hi = lo + kUnit < n ? lo + kUnit : n;
        const u8* const src = a.in + a.in_off[b];
        u8* const dst = out + out_off[b];
        const u64 t0 = st.aslots[b], t1 = st.aslots[b + 1];
        u64 j = ix_first_where(t0, t1, [&](u64 t) { return sl.pos[t] + sl.old[t] > lo; });      // the first slot whose old chunk ends behind lo
        u64 cur = lo;
        while (cur < hi) {
            const u64 shift = j > t0 ? shift_of(sl, t0, j) : 0;
            const u64 next = j < t1 ? sl.pos[j] : ~0ull;
            if (next <= cur) {                                          // cur lies in (or at) the old chunk of slot j
                const u32 d = sl.dec[j];
                if (next >= lo && d) {                                  // it starts in this range: the new chunk
                    bool shrink;
                    const u32 pl = payload_of(sl.comp_len[j], d, &shrink);
                    u8* const at = dst + next + shift;
                    chunk_header(at, tid, shrink ? 0u : 1u, pl, sl.crc[j]);
                    wg_copy(at + SNP_CHUNK_HEADER_LEN, shrink ? comp + sl.coff[j] : raw + sl.place[j], pl, tid);
                }
                const u64 end = next + sl.old[j];
                cur = end > cur ? end : cur;
                ++j;
            } else {                                                    // a clean run up to the next dirty chunk
                const u64 stop = next < hi ? next : hi;
                wg_copy(dst + cur + shift, src + cur, stop - cur, tid);
                cur = stop;
            }
        }
    }
}

__global__ __launch_bounds__(256) void k_fu_new_pos(UpArgs a, UpStreams st, UpSlots sl, u64* __restrict__ new_pos)
{
    for (u64 i = static_cast<u64>(blockIdx.x) * 256u + threadIdx.x; i < a.x.nentries; i += static_cast<u64>(gridDim.x) * 256u) {
        u64 v = a.x.pos[i];
        const u32 b = owner_of(a.x.first, a.ns, i);                     // (idx_first is untrusted: any stream at all, so the row is checked to be its)
        const u64 f0 = a.x.first[b] < a.x.nentries ? a.x.first[b] : a.x.nentries, f1 = a.x.first[b + 1] < a.x.nentries ? a.x.first[b + 1] : a.x.nentries;
        if (i >= f0 && i < f1 && (st.flags[b] & kWritten)) {
            const u64 t0 = st.aslots[b], t1 = st.aslots[b + 1];
            const u64 j = ix_first_where(t0, t1, [&](u64 t) { return sl.row[t] >= i; });
            if (j > t0) v += shift_of(sl, t0, j);
        }
        new_pos[i] = v;
    }
}

// workspace (every piece 256-byte aligned; nothing when there is no request or no stream)
struct UpdateWork {
    UpReq rq;
    UpStreams st;
    UpSlots sl;
    ChunkRows rows;
    u64* part;
    u8 *raw, *comp;
    u64 empty_base, bytes;
};
UpdateWork work_layout(void* base, u32 nstreams, u32 nreq, u32 max_slots, u64 stage_cap)
{
    UpdateWork w{};
    if (nstreams == 0 || nreq == 0) return w;
    const u64 ns = nstreams, nr = nreq, M = max_slots;
    WorkCarver k(base);
    w.part = k.take<u64>(scan_tiles_of(std::max(std::max(ns, nr), M)));
    w.rq.r0 = k.take<u64>(nr);
    w.rq.r1 = k.take<u64>(nr);
    w.rq.own0 = k.take<u64>(nr);
    w.rq.cnt = k.take<u64>(nr);
    w.rq.bytes = k.take<u64>(nr);
    w.rq.live = k.take<u64>(nr + 1);
    w.rq.sfirst = k.take<u64>(nr + 1);
    w.rq.bfirst = k.take<u64>(nr + 1);
    w.rq.flags = k.take<u32>(nr);
    w.st.fail = k.take<u64>(ns);
    w.st.delta = k.take<u64>(ns);
    w.st.slot0 = k.take<u64>(ns);
    w.st.nslots = k.take<u64>(ns);
    w.st.byte0 = k.take<u64>(ns);
    w.st.nbytes = k.take<u64>(ns);
    w.st.units = k.take<u64>(ns);
    w.st.aslots = k.take<u64>(ns + 1);
    w.st.abytes = k.take<u64>(ns + 1);
    w.st.gfirst = k.take<u64>(ns + 1);
    w.st.flags = k.take<u32>(ns);
    w.sl.pos = k.take<u64>(M);
    w.sl.place = k.take<u64>(M);
    w.sl.coff = k.take<u64>(M);
    w.sl.row = k.take<u64>(M);
    w.sl.nscan = k.take<u64>(M + 1);
    w.sl.oscan = k.take<u64>(M + 1);
    w.sl.old = k.take<u32>(M);
    w.sl.dec = k.take<u32>(M);
    w.sl.stream = k.take<u32>(M);
    w.sl.req = k.take<u32>(M);
    w.sl.comp_len = k.take<u32>(M);
    w.sl.crc = k.take<u32>(M);
    w.sl.c_status = k.take<i32>(M);
    w.rows = carve_chunk_rows(k, M);
    // raw staging: the dirty slots' decoded bytes back to back (+ slack for the compressor's vector loads).  Compressed staging: slot t of decoded
    // bytes d at raw offset p starts at (p + p / 6) rounded up to 16, + 96 t, which leaves it snp_comp_stride(d) <= d + d / 6 + 69 bytes; the
    // slots not in use (they compress nothing into snp_comp_stride(0) = 64 bytes) follow at 64 bytes each.
    w.raw = k.take<u8>(stage_cap + 256);
    w.empty_base = (stage_cap + stage_cap / 6 + 15) / 16 * 16 + 96 * M + 256;
    w.comp = k.take<u8>(w.empty_base + 64 * M);
    w.bytes = k.bytes();
    return w;
}

}  // namespace

extern "C" {

uint64_t snp_frame_write_indexed_workspace(uint32_t nstreams, uint32_t nreq, uint32_t max_slots, uint64_t stage_cap)
{
    return work_layout(nullptr, nstreams, nreq, max_slots, stage_cap).bytes;
}

snp_status snp_frame_write_indexed_batch(snp_ctx* c, const uint8_t* in, const uint64_t* in_off, const uint64_t* in_len, uint32_t nstreams,
                                         const uint64_t* idx_first, const uint64_t* idx_start, const uint64_t* idx_pos, const uint64_t* idx_total,
                                         const int32_t* idx_tail, uint64_t nentries, const uint8_t* src, const uint32_t* req_stream,
                                         const uint64_t* req_off, const uint64_t* req_len, const uint64_t* src_off, uint32_t nreq, uint32_t max_slots,
                                         uint64_t stage_cap, uint8_t* out, const uint64_t* out_off, const uint64_t* out_cap, uint64_t* out_len,
                                         int32_t* status, int32_t* req_status, uint64_t* new_pos, uint64_t* out_bound, void* d_work,
                                         uint64_t* d_result)
{
    const bool work = nreq && nstreams;
    if (!c || !d_result || nreq > 0x7fffffffu ||                        // (one workgroup per request: nreq must be a grid)
        (work && (!in || !in_off || !in_len || !idx_first || !idx_total || !idx_tail || !src || !req_stream || !req_off || !req_len || !src_off ||
                  !out || !out_off || !out_cap || !out_len || !status || !req_status || !d_work)) ||
        (work && nentries && (!idx_start || !idx_pos)))
        return SNP_ERR_BAD_ARG;
    DevGuard dg(c);
    if (!dg.ok) return SNP_ERR_DEVICE;
    hipStream_t s = c->stream;
    bool ok = c->check(snp_zero_words_async(reinterpret_cast<u32*>(d_result), 2 * 4, s), "frame update result");
    if (!work) return ok ? SNP_OK : SNP_ERR_DEVICE;
    const UpdateWork w = work_layout(d_work, nstreams, nreq, max_slots, stage_cap);
    const u32 ns = nstreams, M = max_slots, sg = groups_of(ns), rg = groups_of(nreq), mg = groups_of(M);
    const UpArgs a{in, in_off, in_len, ns, FrameIndex{idx_first, idx_start, idx_pos, idx_total, idx_tail, nentries},
                   FuRequests{req_stream, req_off, req_len, nreq}};
    const Admit admit{w.st.flags, w.st.aslots, w.st.abytes, M, stage_cap};
    // the plan of every request, the rows each owns, its first slot and the place of its bytes
    hipLaunchKernelGGL(k_fu_init, dim3(sg), dim3(256), 0, s, ns, w.st);
    hipLaunchKernelGGL(k_fu_plan, dim3(rg), dim3(256), 0, s, a, w.rq, w.st);
    ok = ok && c->check(hipGetLastError(), "frame update plan") &&
         c->check(launch_scan(ScanLive{w.rq.flags}, nreq, w.part, w.rq.live, nullptr, s), "frame update live scan");
    if (ok) {
        hipLaunchKernelGGL(k_fu_own, dim3(rg), dim3(256), 0, s, a, w.rq, w.st);
        ok = c->check(hipGetLastError(), "frame update own") &&
             c->check(launch_scan(ScanWords{w.rq.cnt}, nreq, w.part, w.rq.sfirst, nullptr, s), "frame update slot scan") &&
             c->check(launch_scan(ScanWords{w.rq.bytes}, nreq, w.part, w.rq.bfirst, nullptr, s), "frame update byte scan");
    }
    // every dirty row checked, every stream's verdict so far, admission (d_result[0] = slots, [2] = staging bytes of the streams that passed)
    if (ok) {
        const u32 cg = std::min(std::max(std::max(mg, rg), 1u), kMaxGroups);
        hipLaunchKernelGGL(k_fu_check, dim3(cg), dim3(256), 0, s, a, w.rq, w.st);
        hipLaunchKernelGGL(k_fu_streams, dim3(sg), dim3(256), 0, s, a, w.rq, w.st);
        ok = c->check(hipGetLastError(), "frame update streams") &&
             c->check(launch_scan(ScanWords{w.st.nslots}, ns, w.part, w.st.aslots, d_result, s), "frame update admission scan") &&
             c->check(launch_scan(ScanWords{w.st.nbytes}, ns, w.part, w.st.abytes, d_result + 2, s), "frame update staging scan");
    }
    if (ok && M) {
        // the slot table; the edges decoded and verified whole into the raw staging, the requests' bytes over them
        hipLaunchKernelGGL(k_fu_slots, dim3(mg), dim3(256), 0, s, a, w.rq, w.st, admit, w.sl, w.rows, w.empty_base);
        ok = c->check(hipGetLastError(), "frame update slots") && c->decode_chunks(in, w.rows, M, w.raw);
        if (ok) {
            hipLaunchKernelGGL(k_fu_fail, dim3(mg), dim3(256), 0, s, M, w.rows, w.sl, w.st);
            hipLaunchKernelGGL(k_fu_overlay, dim3(nreq, kOverlayPieces), dim3(256), 0, s, a, w.rq, w.st, admit, src, src_off, w.raw);
            // every slot's new bytes re-encoded from the raw staging (reencode_slots), the new chunk sizes scanned into nscan
            ok = c->check(hipGetLastError(), "frame update overlay") &&
                 reencode_slots(c, w.raw, RwSlots{w.sl.place, w.sl.coff, w.sl.dec, w.sl.comp_len, w.sl.crc, w.sl.c_status}, M, w.comp, w.part, w.sl.nscan,
                                "frame update") &&
                 c->check(launch_scan(ScanOld{w.sl.old}, M, w.part, w.sl.oscan, nullptr, s), "frame update old size scan");
        }
    }
    if (ok) {
        hipLaunchKernelGGL(k_fu_sizes, dim3(sg), dim3(256), 0, s, a, w.st, admit, w.sl, out_cap, out_len, status, out_bound, d_result);
        hipLaunchKernelGGL(k_fu_requests, dim3(rg), dim3(256), 0, s, a, w.rq, status, req_status);
        ok = c->check(hipGetLastError(), "frame update sizes") &&
             c->check(launch_scan(ScanWords{w.st.units}, ns, w.part, w.st.gfirst, nullptr, s), "frame update unit scan");
    }
    if (ok) {
        hipLaunchKernelGGL(k_fu_emit, dim3(kEmitGroups), dim3(256), 0, s, a, w.st, w.sl, w.raw, w.comp, out, out_off);
        if (new_pos && nentries) hipLaunchKernelGGL(k_fu_new_pos, dim3(static_cast<u32>(std::min<u64>((nentries + 255) / 256, kRowGroups))), dim3(256), 0, s, a, w.st, w.sl, new_pos);
        ok = c->check(hipGetLastError(), "frame update emit");
    }
    return ok ? SNP_OK : SNP_ERR_DEVICE;
}

}  // extern "C"

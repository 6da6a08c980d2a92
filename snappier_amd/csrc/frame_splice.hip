// frame_splice.hip -- snp_frame_splice_indexed_batch: ONE splice per stream of framed streams kept with their chunk index -- decoded bytes
// [off, off + del) replaced by ins source bytes: insert, delete, truncate, drop-prefix -- answered out of place by new streams in which only the
// chunks around the hole are compressed again and every other kept byte is a copy, with the new index.  frame_splice_device.h plans a stream,
// frame_chunked_device.h cuts the rewritten region into slots, the decode of an edge is the update call's edge decode.  Built into
// libsnappier_hip_frame_splice.so (C-ABI: include/snappier_hip_frame_splice.h), linked against libsnappier_hip.so.  DESIGN.md 4.19.
//
//   plan      one thread per stream (fs_plan): the verdict so far, the owned rows, the edges, the hole, |H|, |T|, the pieces, the size bound
//   scans     pieces and staging bytes of the streams that passed -> admission in stream order; d_result[0], [2]
//   edges     one thread per stream: its two rows of the edge table (2 b the head row, 2 b + 1 the tail row when it is another one), else empty rows
//   decode    snp_ctx::decode_chunks over the edge table into staging; fail: one thread per stream, a failing edge -> its stream (the head first)
//   assemble  a workgroup per stream and 64 KiB piece of its region: H, the source bytes and T one behind the other in staging
//   slots     one thread per table slot (fc_owner, fs_piece): its stream, its piece of the region in staging, where its compressed bytes are staged
//   compress  snp_ctx::launch_compress and snp_launch_crc32c over every slot -- once each, from staging
//   scan      8 + payload per slot
//   sizes     one thread per stream: size against out_cap, status, out_len, out_bound, d_result[1] and [3]; its emit units; the rows of its new index
//   scans     emit units, rows of the new index
//   emit      one 256-thread workgroup per unit, grid-stride: 64 KiB of an old stream's kept bytes (before P0 and from P1) at their new place, or
//             fc_group(chunk_bytes) consecutive new chunks (header + payload; the identifier of an empty stream)
//   rows      one thread per new row: an old row copied, a new chunk's row from the size scan, or an old row moved; per stream: new_total, new_tail
// Nothing here allocates, reads back or synchronises: the call is capturable like the other _batch entry points.
#include "capi_internal.h"
#include "frame_rewrite_device.h"
#include "frame_splice_device.h"
#include "../../include/snappier_hip_frame_splice.h"

namespace {

constexpr u32 kSplice = 0x100u, kIdent = 0x200u, kHead = 0x400u, kTail = 0x800u, kWritten = 0x1000u;    // stream flags above the status byte
constexpr u32 kAssemblePieces = 8;                                  // workgroups that share one stream's region

struct SpArgs {
    const u8* in;
    const u64 *in_off, *in_len;
    u32 ns;
    FrameIndex x;
    const u8* src;
    const u64 *sp_off, *sp_del, *sp_ins, *src_off;
    u32 cb;
};
// per stream
struct SpStreams {
    u64 *f0, *rows, *r0, *r1, *p0, *p1, *tpos, *region, *bound;
    u64 *pieces, *stage;                                    // what the stream asks of each bound (0 unless it passed and is named)
    u64 *new_bytes, *nrows, *units;                         // identifier + new chunks; rows of its new index; emit units
    u64 *aslots, *abytes, *nfirst, *gfirst;                 // scans (n + 1): slots / staging bytes of the streams before b; new rows; emit units
    u32 *flags, *hl, *tl, *e0, *e1;
    i32* fail;                                              // the status of an edge that did not decode or verify
};
using SpSlots = RwOwnedSlots;                               // per table slot

// admission in stream order: both sums only grow
struct Admit {
    const u32* flags;
    const u64* __restrict__ aslots;
    const u64* __restrict__ abytes;
    u32 max_slots;
    u64 stage_cap;
    __device__ __forceinline__ bool operator()(u32 b) const { return (flags[b] & kSplice) && aslots[b + 1] <= max_slots && abytes[b + 1] <= stage_cap; }
};

__global__ __launch_bounds__(256) void k_fs_plan(SpArgs a, SpStreams st)
{
    const u32 b = blockIdx.x * 256u + threadIdx.x;
    if (b >= a.ns) return;
    const u8* const s = a.in + a.in_off[b];
    const u64 n = a.in_len[b];
    const FsPlan k = fs_plan(a.x, b, n, a.sp_off[b], a.sp_del[b], a.sp_ins[b], a.cb, [&](u64 pos) { return frame_hop(s, n, pos); });
    st.f0[b] = k.f0;
    st.rows[b] = k.rows;
    st.r0[b] = k.r0;
    st.r1[b] = k.r1;
    st.p0[b] = k.p0;
    st.p1[b] = k.p1;
    st.tpos[b] = k.tpos;
    st.region[b] = k.region;
    st.bound[b] = k.splice ? k.bound : 0;
    st.pieces[b] = fs_count_pieces(k);
    st.stage[b] = fs_count_stage(k);
    st.new_bytes[b] = 0;
    st.flags[b] = static_cast<u32>(k.status) | (k.splice ? kSplice : 0u) | (k.ident ? kIdent : 0u) | (k.head ? kHead : 0u) | (k.tail ? kTail : 0u);
    st.hl[b] = k.hl;
    st.tl[b] = k.tl;
    st.e0[b] = k.e0;
    st.e1[b] = k.e1;
    st.fail[b] = SNP_OK;
}

// One thread per stream: the rows 2 b and 2 b + 1 of the edge table.  An admitted stream's head row is decoded whole to the start of its staging
// bytes, its tail row (when it is another row) behind it; every other row is empty.
__global__ __launch_bounds__(256) void k_fs_edges(SpArgs a, SpStreams st, Admit admit, ChunkRows rows)
{
    const u32 b = blockIdx.x * 256u + threadIdx.x;
    if (b >= a.ns) return;
    const u64 t0 = 2ull * b, t1 = t0 + 1;
    rows.tag[t0] = rows.tag[t1] = kNone;
    chunk_row_clear(rows, t0, 0);
    chunk_row_clear(rows, t1, 0);
    if (!admit(b)) return;
    const u8* const s = a.in + a.in_off[b];
    const u64 n = a.in_len[b], place = st.abytes[b];
    if (st.e0[b]) {
        const Hop h = frame_hop(s, n, st.p0[b]);
        if (h.kind == HOP_DATA && h.dec == st.e0[b]) {                  // (what the plan saw)
            rows.tag[t0] = static_cast<u32>(t0);
            chunk_row_set(rows, t0, h, a.in_off[b] + st.p0[b], place);
        }
    }
    if (st.e1[b]) {
        const Hop h = frame_hop(s, n, st.tpos[b]);
        if (h.kind == HOP_DATA && h.dec == st.e1[b]) {
            rows.tag[t1] = static_cast<u32>(t1);
            chunk_row_set(rows, t1, h, a.in_off[b] + st.tpos[b], place + st.e0[b]);
        }
    }
}

// an edge that did not decode or verify: its status to its stream, the head edge's first
__global__ __launch_bounds__(256) void k_fs_fail(u32 ns, ChunkRows rows, SpStreams st)
{
    const u32 b = blockIdx.x * 256u + threadIdx.x;
    if (b >= ns) return;
    i32 s = SNP_OK;
    for (u64 t = 2ull * b; t < 2ull * b + 2 && s == SNP_OK; ++t) {
        if (rows.tag[t] == kNone) continue;
        s = row_verdict(rows, t);
    }
    st.fail[b] = s;
}

// the part [u0, u1) of a region that lies in its segment [s0, s0 + len): from `from` (the segment's first byte) to dst (the region's first byte)
__device__ __forceinline__ void segment_copy(u8* dst, const u8* from, u64 s0, u64 len, u64 u0, u64 u1, u32 tid)
{
    const u64 a = u0 > s0 ? u0 : s0, e = u1 < s0 + len ? u1 : s0 + len;
    if (a < e) team_copy(dst + a, from + (a - s0), static_cast<u32>(e - a), tid, 256u);      // (e - a <= kUnit)
}

// A workgroup per stream and piece of its region, 64 KiB at a time: R = H || source bytes || T behind the decoded edges in staging.  The stream
// steers the whole workgroup.
__global__ __launch_bounds__(256) void k_fs_assemble(SpArgs a, SpStreams st, Admit admit, u8* __restrict__ stage)
{
    const u32 b = blockIdx.x;
    if (!admit(b) || st.fail[b] != SNP_OK) return;
    const u64 region = st.region[b], ins = a.sp_ins[b];
    const u32 hl = st.hl[b], tl = st.tl[b], e0 = st.e0[b], e1 = st.e1[b];
    const u8* const edges = stage + st.abytes[b];
    u8* const dst = stage + st.abytes[b] + e0 + e1;
    // T: the last tl bytes of the tail row -- the head row itself when both edges are one row
    const u8* const tail = e1 ? edges + e0 + (e1 - tl) : edges + (e0 - tl);
    for (u64 u0 = blockIdx.y * kUnit; u0 < region; u0 += gridDim.y * kUnit) {
        const u64 u1 = u0 + kUnit < region ? u0 + kUnit : region;
        segment_copy(dst, edges, 0, hl, u0, u1, threadIdx.x);
        segment_copy(dst, a.src + a.src_off[b], hl, ins, u0, u1, threadIdx.x);
        segment_copy(dst, tail, hl + ins, tl, u0, u1, threadIdx.x);
    }
}

// One thread per table slot: its piece of its stream's region in staging and where its compressed bytes are staged.
__global__ __launch_bounds__(256) void k_fs_slots(SpArgs a, SpStreams st, Admit admit, SpSlots sl, u64 stride)
{
    const u32 c = blockIdx.x * 256u + threadIdx.x;
    if (c >= admit.max_slots) return;
    u64 in_off = 0;
    u32 len = 0, stream = kNone;
    if (c < st.aslots[a.ns]) {
        const u32 b = fc_owner(st.aslots, a.ns, c);
        if (admit(b) && st.fail[b] == SNP_OK) {
            const FsPiece p = fs_piece(st.region[b], a.cb, c - st.aslots[b]);
            in_off = st.abytes[b] + st.e0[b] + st.e1[b] + p.off;
            len = p.len;
            stream = b;
        }
    }
    sl.in_off[c] = in_off;
    sl.coff[c] = fc_stage_off(c, stride);
    sl.len[c] = len;
    sl.stream[c] = stream;
}

__global__ __launch_bounds__(256) void k_fs_sizes(SpArgs a, SpStreams st, Admit admit, const u64* __restrict__ cscan, u32 group,
                                                 const u64* __restrict__ out_cap, u64* __restrict__ out_len, i32* __restrict__ status,
                                                 u64* __restrict__ out_bound, u64* __restrict__ result)
{
    const u32 b = blockIdx.x * 256u + threadIdx.x;
    u64 ok_len = 0, ok = 0;
    if (b < a.ns) {
        u32 flags = st.flags[b];
        i32 s = static_cast<i32>(flags & 0xffu);
        u64 bound = st.bound[b], rows = st.rows[b], units = 0;
        if (flags & kSplice) {
            s = SNP_ERR_OUTPUT_TOO_SMALL;
            if (admit(b)) {
                if (st.fail[b] != SNP_OK) {
                    s = st.fail[b];
                    bound = 0;
                } else {
                    const u64 fresh = ((flags & kIdent) ? SNP_STREAM_HEADER_LEN : 0) + (cscan[st.aslots[b + 1]] - cscan[st.aslots[b]]);
                    const u64 kept = a.in_len[b] - (st.p1[b] - st.p0[b]), size = kept + fresh;
                    if (size <= out_cap[b]) {
                        s = SNP_OK;
                        ok_len = size;
                        ok = 1;
                        flags |= kWritten;
                        rows = fs_new_rows(rows, st.r0[b], st.r1[b], st.pieces[b]);
                        units = (kept + kUnit - 1) / kUnit + (st.pieces[b] + group - 1) / group;
                        st.new_bytes[b] = fresh;
                    }
                }
            }
        }
        status[b] = s;
        out_len[b] = ok_len;
        if (out_bound) out_bound[b] = bound;
        st.flags[b] = flags;
        st.nrows[b] = rows;
        st.units[b] = units;
    }
    ok_len = wave_sum(ok_len);
    ok = wave_sum(ok);
    if ((threadIdx.x & 63u) == 0 && ok) {
        atomic_add64(result + 1, ok_len);
        atomic_add64(result + 3, ok);
    }
}

// One workgroup per emit unit of a written stream.  The first units of a stream are 64 KiB each of its KEPT bytes -- the old stream without the hole
// [P0, P1): a byte before P0 stays where it was, a byte from P1 on moves by new_bytes - (P1 - P0) -- the others are `group` consecutive new chunks
// each, taken by teams of `team` threads in turn (fc_group and fc_team, frame_chunked_device.h; emit_slot, frame_rewrite_device.h).  The unit
// steers the whole workgroup, a slot its whole team.
__global__ __launch_bounds__(256) void k_fs_emit(SpArgs a, SpStreams st, SpSlots sl, u32 group, u32 team, const u64* __restrict__ cscan,
                                                const u8* __restrict__ stage, const u8* __restrict__ comp, u8* __restrict__ out,
                                                const u64* __restrict__ out_off)
{
    const u32 tid = threadIdx.x, t = tid % team, teams = 256u / team;
    const u64 units = st.gfirst[a.ns];
    for (u64 g = blockIdx.x; g < units; g += gridDim.x) {
        const u32 b = owner_of(static_cast<const u64*>(st.gfirst), a.ns, g);
        const u64 u = g - st.gfirst[b], p0 = st.p0[b], p1 = st.p1[b], kept = a.in_len[b] - (p1 - p0);
        const u64 kept_units = (kept + kUnit - 1) / kUnit;
        const u8* const old = a.in + a.in_off[b];
        u8* const dst = out + out_off[b];
        if (u < kept_units) {
            const u64 k0 = u * kUnit, k1 = k0 + kUnit < kept ? k0 + kUnit : kept;
            const u64 mid = p0 < k0 ? k0 : p0 < k1 ? p0 : k1;            // [k0, mid) lies before the hole, [mid, k1) behind it
            if (mid > k0) team_copy(dst + k0, old + k0, static_cast<u32>(mid - k0), tid, 256u);
            if (k1 > mid) team_copy(dst + mid + st.new_bytes[b], old + mid + (p1 - p0), static_cast<u32>(k1 - mid), tid, 256u);
            continue;
        }
        const u64 first = st.aslots[b], last = st.aslots[b + 1];
        const u64 c0 = first + (u - kept_units) * group, c1 = c0 + group < last ? c0 + group : last;
        const u64 base = p0 + ((st.flags[b] & kIdent) ? SNP_STREAM_HEADER_LEN : 0);
        for (u64 c = c0 + tid / team; c < c1; c += teams) {
            const u64 pos = base + (cscan[c] - cscan[first]);
            if (c == first && (st.flags[b] & kIdent) && t < SNP_STREAM_HEADER_LEN) dst[t] = k_fc_stream_id[t];   // EnsureStreamHeaderWritten  :148-157
            emit_slot(dst + pos, sl.rw(), c, stage, comp, t, team);
        }
    }
}

// One thread per row of the new index, grid-stride, and per stream its three words (k_fa_rows with a row count that changes).  Row i of stream
// b = owner(nfirst, i): of a stream that is not written, one of its old rows (f0 and the count are clamped to nentries: idx_first is untrusted);
// of a written one, an old row before r0, new chunk j, or an old row from r1 on, moved.  Rows at or past `cap` do not exist.
__global__ __launch_bounds__(256) void k_fs_rows(SpArgs a, SpStreams st, const u64* __restrict__ cscan, u64 cap, u64* __restrict__ new_first,
                                                u64* __restrict__ new_start, u64* __restrict__ new_pos, u64* __restrict__ new_total,
                                                i32* __restrict__ new_tail)
{
    const u64 total = st.nfirst[a.ns] < cap ? st.nfirst[a.ns] : cap;
    const u64 most = total > static_cast<u64>(a.ns) + 1 ? total : static_cast<u64>(a.ns) + 1;
    for (u64 i = static_cast<u64>(blockIdx.x) * 256u + threadIdx.x; i < most; i += static_cast<u64>(gridDim.x) * 256u) {
        if (i <= a.ns) new_first[i] = st.nfirst[i] < cap ? st.nfirst[i] : cap;
        if (i < a.ns) {
            const bool written = (st.flags[i] & kWritten) != 0;
            new_total[i] = written ? a.x.total[i] - a.sp_del[i] + a.sp_ins[i] : a.x.total[i];
            new_tail[i] = written ? SNP_OK : a.x.tail[i];
        }
        if (i >= total) continue;
        const u32 b = owner_of(static_cast<const u64*>(st.nfirst), a.ns, i);
        const u64 j = i - st.nfirst[b], f0 = st.f0[b];
        if (!(st.flags[b] & kWritten) || j < st.r0[b] - f0) {
            new_start[i] = a.x.start[f0 + j];
            new_pos[i] = a.x.pos[f0 + j];
            continue;
        }
        const u64 k = j - (st.r0[b] - f0), pieces = st.pieces[b];
        if (k < pieces) {
            const u64 first = st.aslots[b];
            new_start[i] = fs_row_start(a.sp_off[b], st.hl[b], a.cb, k);
            new_pos[i] = st.p0[b] + ((st.flags[b] & kIdent) ? SNP_STREAM_HEADER_LEN : 0) + (cscan[first + k] - cscan[first]);
        } else {
            const u64 r = st.r1[b] + (k - pieces);
            new_start[i] = fs_moved_start(a.x.start[r], a.sp_del[b], a.sp_ins[b]);
            new_pos[i] = fs_moved_pos(a.x.pos[r], st.p0[b], st.p1[b], st.new_bytes[b]);
        }
    }
}

// workspace (every piece 256-byte aligned; nothing when there is no stream)
struct SpliceWork {
    SpStreams st;
    SpSlots sl;
    ChunkRows rows;
    u64 *part, *cscan;
    u8 *stage, *comp;
    u64 bytes;
};
SpliceWork work_layout(void* base, u32 nstreams, u32 max_slots, u64 stage_cap, u32 chunk_bytes)
{
    SpliceWork w{};
    if (nstreams == 0 || chunk_bytes == 0 || chunk_bytes > SNP_BLOCK_SIZE) return w;
    const u64 ns = nstreams, M = max_slots;
    WorkCarver k(base);
    w.part = k.take<u64>(scan_tiles_of(std::max(2 * ns, M)));
    for (u64** p : {&w.st.f0, &w.st.rows, &w.st.r0, &w.st.r1, &w.st.p0, &w.st.p1, &w.st.tpos, &w.st.region, &w.st.bound, &w.st.pieces, &w.st.stage,
                    &w.st.new_bytes, &w.st.nrows, &w.st.units})
        *p = k.take<u64>(ns);
    for (u64** p : {&w.st.aslots, &w.st.abytes, &w.st.nfirst, &w.st.gfirst}) *p = k.take<u64>(ns + 1);
    for (u32** p : {&w.st.flags, &w.st.hl, &w.st.tl, &w.st.e0, &w.st.e1}) *p = k.take<u32>(ns);
    w.st.fail = k.take<i32>(ns);
    w.sl = carve_rw_owned_slots(k, M);
    w.rows = carve_chunk_rows(k, 2 * ns);
    w.cscan = k.take<u64>(M + 1);
    // staging: per admitted stream its decoded edges and its region behind them, the streams back to back (+ slack for the compressor's vector
    // loads).  Compressed staging: slot c at c * snp_comp_stride(chunk_bytes) (fc_stage_off).
    w.stage = k.take<u8>(stage_cap + 256);
    w.comp = k.take<u8>(M * snp_comp_stride(chunk_bytes));
    w.bytes = k.bytes();
    return w;
}

}  // namespace

extern "C" {

uint64_t snp_frame_splice_indexed_workspace(uint32_t nstreams, uint32_t max_slots, uint64_t stage_cap, uint32_t chunk_bytes)
{
    return work_layout(nullptr, nstreams, max_slots, stage_cap, chunk_bytes).bytes;
}

snp_status snp_frame_splice_indexed_batch(snp_ctx* c, const uint8_t* in, const uint64_t* in_off, const uint64_t* in_len, uint32_t nstreams,
                                          const uint64_t* idx_first, const uint64_t* idx_start, const uint64_t* idx_pos, const uint64_t* idx_total,
                                          const int32_t* idx_tail, uint64_t nentries, const uint8_t* src, const uint64_t* sp_off,
                                          const uint64_t* sp_del, const uint64_t* sp_ins, const uint64_t* src_off, uint32_t chunk_bytes,
                                          uint32_t max_slots, uint64_t stage_cap, uint8_t* out, const uint64_t* out_off, const uint64_t* out_cap,
                                          uint64_t* out_len, int32_t* status, uint64_t* new_first, uint64_t* new_start, uint64_t* new_pos,
                                          uint64_t* new_total, int32_t* new_tail, uint64_t* out_bound, void* d_work, uint64_t* d_result)
{
    const u64 cap = nentries + max_slots;                               // rows the new start / pos arrays hold
    if (!c || !d_result || chunk_bytes == 0 || chunk_bytes > SNP_BLOCK_SIZE || nstreams > 0x7fffffffu ||      // (one workgroup per stream: 2 nstreams rows)
        (nstreams && (!in || !in_off || !in_len || !idx_first || !idx_total || !idx_tail || !src || !sp_off || !sp_del || !sp_ins || !src_off || !out ||
                      !out_off || !out_cap || !out_len || !status || !new_first || !new_total || !new_tail || !d_work)) ||
        (nstreams && nentries && (!idx_start || !idx_pos)) || (nstreams && cap && (!new_start || !new_pos)))
        return SNP_ERR_BAD_ARG;
    DevGuard dg(c);
    if (!dg.ok) return SNP_ERR_DEVICE;
    hipStream_t s = c->stream;
    bool ok = c->check(snp_zero_words_async(reinterpret_cast<u32*>(d_result), 2 * 4, s), "frame splice result");
    if (nstreams == 0) return ok ? SNP_OK : SNP_ERR_DEVICE;
    const SpliceWork w = work_layout(d_work, nstreams, max_slots, stage_cap, chunk_bytes);
    const u32 ns = nstreams, E = 2 * ns, M = max_slots, cb = chunk_bytes, sg = groups_of(ns), mg = groups_of(M);
    const SpArgs a{in, in_off, in_len, ns, FrameIndex{idx_first, idx_start, idx_pos, idx_total, idx_tail, nentries}, src, sp_off, sp_del, sp_ins, src_off, cb};
    const Admit admit{w.st.flags, w.st.aslots, w.st.abytes, M, stage_cap};
    // the plan of every stream; admission in stream order (d_result[0] = slots, [2] = staging bytes of the streams that passed)
    hipLaunchKernelGGL(k_fs_plan, dim3(sg), dim3(256), 0, s, a, w.st);
    ok = ok && c->check(hipGetLastError(), "frame splice plan") &&
         c->check(launch_scan(ScanWords{w.st.pieces}, ns, w.part, w.st.aslots, d_result, s), "frame splice slot scan") &&
         c->check(launch_scan(ScanWords{w.st.stage}, ns, w.part, w.st.abytes, d_result + 2, s), "frame splice staging scan");
    if (ok && stage_cap) {
        // the edges decoded and verified whole into staging (a stream with an edge has staging bytes: none is admitted when stage_cap is 0), then
        // H, the source bytes and T of every admitted stream one behind the other
        hipLaunchKernelGGL(k_fs_edges, dim3(sg), dim3(256), 0, s, a, w.st, admit, w.rows);
        ok = c->check(hipGetLastError(), "frame splice edges") && c->decode_chunks(in, w.rows, E, w.stage);
        if (ok) {
            hipLaunchKernelGGL(k_fs_fail, dim3(sg), dim3(256), 0, s, ns, w.rows, w.st);
            hipLaunchKernelGGL(k_fs_assemble, dim3(ns, kAssemblePieces), dim3(256), 0, s, a, w.st, admit, w.stage);
            ok = c->check(hipGetLastError(), "frame splice assemble");
        }
    }
    if (ok && M) {
        hipLaunchKernelGGL(k_fs_slots, dim3(mg), dim3(256), 0, s, a, w.st, admit, w.sl, snp_comp_stride(cb));
        ok = c->check(hipGetLastError(), "frame splice slots");
        // every piece compressed from staging; without staging every slot is empty (reencode_slots in two steps: the scan below runs either way)
        if (ok && stage_cap) ok = compress_slots(c, w.stage, w.sl.rw(), M, w.comp, "frame splice");
    }
    // the framed sizes of the new chunks, every stream's verdict, its emit units and the rows of its new index
    ok = ok && c->check(launch_scan(ScanFramed{w.sl.len, w.sl.comp_len}, M, w.part, w.cscan, nullptr, s), "frame splice size scan");
    if (ok) {
        const u32 group = fc_group(cb);
        hipLaunchKernelGGL(k_fs_sizes, dim3(sg), dim3(256), 0, s, a, w.st, admit, w.cscan, group, out_cap, out_len, status, out_bound, d_result);
        ok = c->check(hipGetLastError(), "frame splice sizes") &&
             c->check(launch_scan(ScanWords{w.st.units}, ns, w.part, w.st.gfirst, nullptr, s), "frame splice unit scan") &&
             c->check(launch_scan(ScanWords{w.st.nrows}, ns, w.part, w.st.nfirst, nullptr, s), "frame splice row scan");
        if (ok) {
            hipLaunchKernelGGL(k_fs_emit, dim3(kEmitGroups), dim3(256), 0, s, a, w.st, w.sl, group, fc_team(group), w.cscan, w.stage, w.comp, out, out_off);
            const u64 most = std::max<u64>(cap, static_cast<u64>(ns) + 1);
            hipLaunchKernelGGL(k_fs_rows, dim3(static_cast<u32>(std::min<u64>((most + 255) / 256, kRowGroups))), dim3(256), 0, s, a, w.st, w.cscan, cap,
                               new_first, new_start, new_pos, new_total, new_tail);
            ok = c->check(hipGetLastError(), "frame splice emit");
        }
    }
    return ok ? SNP_OK : SNP_ERR_DEVICE;
}

}  // extern "C"

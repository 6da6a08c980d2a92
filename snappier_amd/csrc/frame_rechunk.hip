// frame_rechunk.hip -- snp_frame_rechunk_indexed_batch: framed streams kept with their chunk index brought to CANONICAL form -- what
// snp_frame_encode_chunked_batch writes for their decoded bytes with chunk_bytes -- out of place, with the new index.  An old chunk that already
// is a piece of the new stream is copied; only the other pieces are decoded and compressed again, with no read-back between the two.
// frame_rechunk_device.h plans a stream; the slot table, its re-encode, the piece table and the emit are frame_rewrite_device.h's, shared with
// the compose call.  Built into libsnappier_hip_frame_rechunk.so (C-ABI: include/snappier_hip_frame_rechunk.h), linked against
// libsnappier_hip.so.  DESIGN.md 4.20, 4.17.  The kernels here are k_rc_*: k_fr_* are frame_range.hip's.
//
//   plan      a workgroup per stream walks its rows (fr_row, fr_add; joined over the workgroup): the partition, every header, clean or dirty;
//             thread 0: fr_finish -- the verdict so far, canonical or not, the dirty rows, the rebuilt pieces, the staging bytes, the size bound
//   scans     dirty rows, rebuilt pieces, staging bytes, new rows -> admission in stream order; d_result[2], [4]
//   clear     one thread per row of the decode table: an empty row
//   fill      a workgroup per admitted stream walks its rows again: dirty row j -> row adirty[b] + j of the table, decoded to the stream's staging
//             bytes + the decoded bytes of the dirty rows before it
//   decode    snp_ctx::decode_chunks over the table into staging; fail: one thread per row, a failing row -> its stream (the first in order)
//   slots     one thread per table slot (fc_owner): the m-th rebuilt piece of its stream lies at m * chunk_bytes of the stream's staging bytes
//   re-encode reencode_slots: snp_ctx::launch_compress and snp_launch_crc32c over every slot -- once each, from staging; the scan of 8 + payload
//             per slot
//   sizes     one thread per stream: size against out_cap, status, out_len, out_bound, d_result[0], [1], [3], [5]; its emit units; its new rows
//   scans     emit units, rows of the new index
//   rows      one thread per new row: an old row copied, or piece k of a written stream -- kept (the old chunk's place in `in` and size) or
//             rebuilt (its slot and framed size); per stream: new_first, new_total, new_tail
//   scan      the chunk sizes of the new rows -> where each chunk lies
//   emit      k_rw_emit: one 256-thread workgroup per unit, grid-stride: fc_group(chunk_bytes) consecutive new chunks of a written stream, a
//             team each: a kept chunk copied from `in`, or header + payload from staging; new_pos of the row
// Nothing here allocates, reads back or synchronises: the call is capturable like the other _batch entry points.
#include "capi_internal.h"
#include "frame_rewrite_device.h"
#include "frame_rechunk_device.h"
#include "../../include/snappier_hip_frame_rechunk.h"

namespace {

constexpr u32 kWork = 0x100u, kLast = 0x200u, kWritten = 0x400u;    // stream flags above the status byte

struct RcArgs {
    const u8* in;
    const u64 *in_off, *in_len;
    u32 ns;
    FrameIndex x;
    u32 cb;
    bool all;
};
// per stream
struct RcStreams {
    u64 *f0, *rows, *pieces, *rebuilt, *kept, *bound;
    u64 *cdirty, *cslots, *cstage, *crows;                  // what the stream asks of each bound
    u64 *fail;                                              // min over its failing dirty rows of (table row << 8 | status)
    u64 *nrows, *units;                                     // rows of its new index; emit units
    u64 *adirty, *aslots, *abytes, *arows, *nfirst, *gfirst;// scans (n + 1): of the four counts; new rows; emit units
    u32* flags;
};

// admission in stream order: all four sums only grow
struct Admit {
    const u32* flags;
    const u64* __restrict__ adirty;
    const u64* __restrict__ aslots;
    const u64* __restrict__ abytes;
    const u64* __restrict__ arows;
    u32 max_slots;
    u64 stage_cap, max_entries;
    __device__ __forceinline__ bool operator()(u32 b) const
    {
        return (flags[b] & kWork) && adirty[b + 1] <= max_slots && aslots[b + 1] <= max_slots && abytes[b + 1] <= stage_cap && arows[b + 1] <= max_entries;
    }
};

// what the threads of a workgroup found, joined (every thread gets the result); s: 8 words of LDS
__device__ __forceinline__ FrAcc block_join(FrAcc a, u64* s)
{
    if (threadIdx.x < 8) s[threadIdx.x] = 0;
    __syncthreads();
    a.dirty = wave_sum(a.dirty);
    a.dbytes = wave_sum(a.dbytes);
    a.clean = wave_sum(a.clean);
    a.kept = wave_sum(a.kept);
    const u64 bits = wave_sum((a.bad ? 1ull : 0) | (a.loose ? 1ull << 16 : 0) | (a.last ? 1ull << 32 : 0));     // (64 lanes: no carry between the fields)
    if ((threadIdx.x & 63u) == 0) {
        atomic_add64(s + 0, a.dirty);
        atomic_add64(s + 1, a.dbytes);
        atomic_add64(s + 2, a.clean);
        atomic_add64(s + 3, a.kept);
        atomic_add64(s + 4, bits);
    }
    __syncthreads();
    FrAcc r{};
    r.dirty = s[0];
    r.dbytes = s[1];
    r.clean = s[2];
    r.kept = s[3];
    r.bad = (s[4] & 0xffffull) != 0;
    r.loose = ((s[4] >> 16) & 0xffffull) != 0;
    r.last = (s[4] >> 32) != 0;
    return r;
}

// A workgroup per stream.  The stream steers the whole workgroup.
__global__ __launch_bounds__(256) void k_rc_plan(RcArgs a, RcStreams st)
{
    __shared__ u64 s_acc[8];
    const u32 b = blockIdx.x;
    const u8* const s = a.in + a.in_off[b];
    const u64 n = a.in_len[b];
    const i32 begin = fr_begin(a.x, b);
    FrAcc acc{};
    if (begin == SNP_OK) {
        u64 f0, rows;
        fr_rows(a.x, b, &f0, &rows);
        const u64 f1 = f0 + rows, total = a.x.total[b];
        for (u64 i = f0 + threadIdx.x; i < f1; i += 256u)
            fr_add(&acc, a.x, f0, f1, total, n, i, fr_row(a.x, f0, f1, total, n, a.cb, a.all, i, [&](u64 pos) { return frame_hop(s, n, pos); }));
    }
    acc = block_join(acc, s_acc);
    if (threadIdx.x != 0) return;
    const FrPlan k = fr_finish(a.x, b, n, a.cb, a.all, fr_ident(s, n), begin, acc);
    st.f0[b] = k.f0;
    st.rows[b] = k.rows;
    st.pieces[b] = k.pieces;
    st.rebuilt[b] = k.rebuilt;
    st.kept[b] = k.kept;
    st.bound[b] = k.work ? k.bound : 0;
    st.cdirty[b] = fr_count_dirty(k);
    st.cslots[b] = fr_count_slots(k);
    st.cstage[b] = fr_count_stage(k);
    st.crows[b] = fr_count_rows(k);
    st.fail[b] = kNoFail;
    st.flags[b] = static_cast<u32>(k.status) | (k.work ? kWork : 0u) | (k.last ? kLast : 0u);
}

// One thread per row of the decode table: an empty row.
__global__ __launch_bounds__(256) void k_rc_clear(u32 max_slots, ChunkRows rows, u64* __restrict__ dstart)
{
    const u32 t = blockIdx.x * 256u + threadIdx.x;
    if (t >= max_slots) return;
    rows.tag[t] = kNone;
    chunk_row_clear(rows, t, 0);
    dstart[t] = 0;
}

// A workgroup per admitted stream walks its rows again, 256 at a time, with the dirty rows and their decoded bytes so far: dirty row j of the
// stream is row adirty[b] + j of the table and decodes to the stream's staging bytes + the decoded bytes of the dirty rows before it.
__global__ __launch_bounds__(256) void k_rc_fill(RcArgs a, RcStreams st, Admit admit, ChunkRows rows, u64* __restrict__ dstart)
{
    __shared__ u64 s_cnt[4], s_byt[4];
    const u32 b = blockIdx.x;
    if (!admit(b)) return;
    const u8* const s = a.in + a.in_off[b];
    const u64 n = a.in_len[b], f0 = st.f0[b], f1 = f0 + st.rows[b], total = a.x.total[b];
    const u64 t0 = st.adirty[b], t1 = st.adirty[b + 1], place0 = st.abytes[b], place1 = st.abytes[b + 1];
    const u32 wave = threadIdx.x >> 6;
    u64 cnt0 = 0, byt0 = 0;                                             // of the rows before this round
    for (u64 base = f0; base < f1; base += 256u) {
        const u64 i = base + threadIdx.x;
        FrRow r{};
        if (i < f1) r = fr_row(a.x, f0, f1, total, n, a.cb, a.all, i, [&](u64 pos) { return frame_hop(s, n, pos); });
        const bool dirty = r.ok && !r.clean;
        u64 wc, wb;
        u64 cnt = wave_scan(dirty ? 1 : 0, &wc), byt = wave_scan(dirty ? r.len : 0, &wb);
        if ((threadIdx.x & 63u) == 63u) { s_cnt[wave] = wc; s_byt[wave] = wb; }
        __syncthreads();
        u64 allc = 0, allb = 0;
        for (u32 w = 0; w < 4; ++w) {
            if (w < wave) { cnt += s_cnt[w]; byt += s_byt[w]; }
            allc += s_cnt[w];
            allb += s_byt[w];
        }
        const u64 t = t0 + cnt0 + cnt, place = place0 + byt0 + byt;
        if (dirty && t < t1 && place + r.len <= place1) {               // (what the plan saw: they fit)
            rows.tag[t] = static_cast<u32>(t);
            chunk_row_set(rows, t, r.h, a.in_off[b] + r.pos, place);
            dstart[t] = r.start;
        }
        cnt0 += allc;
        byt0 += allb;
        __syncthreads();
    }
}

// a dirty row that did not decode or verify: its status to its stream, the first row's in stream order
__global__ __launch_bounds__(256) void k_rc_fail(u32 ns, u32 max_slots, ChunkRows rows, RcStreams st)
{
    const u32 t = blockIdx.x * 256u + threadIdx.x;
    if (t >= max_slots || rows.tag[t] == kNone) return;
    const i32 s = row_verdict(rows, t);
    if (s != SNP_OK) atomic_min64(st.fail + owner_of(static_cast<const u64*>(st.adirty), ns, t), (static_cast<u64>(t) << 8) | static_cast<u64>(s & 0xff));
}

// One thread per table slot: the m-th rebuilt piece of its stream in staging and where its compressed bytes are staged.
__global__ __launch_bounds__(256) void k_rc_slots(RcArgs a, RcStreams st, Admit admit, RwSlots sl, u64 stride)
{
    const u32 c = blockIdx.x * 256u + threadIdx.x;
    if (c >= admit.max_slots) return;
    u64 in_off = 0;
    u32 len = 0;
    if (c < st.aslots[a.ns]) {
        const u32 b = fc_owner(st.aslots, a.ns, c);
        if (admit(b) && st.fail[b] == kNoFail) {
            const u64 m = c - st.aslots[b];
            const u32 want = fr_slot_len((st.flags[b] & kLast) != 0, st.rebuilt[b], st.pieces[b], a.x.total[b], a.cb, m);
            const u64 at = st.abytes[b] + fr_slot_off(a.cb, m);
            if (want <= a.cb && at + want <= st.abytes[b + 1]) {         // (what the plan saw: the rebuilt pieces are the dirty rows' bytes)
                in_off = at;
                len = want;
            }
        }
    }
    sl.in_off[c] = in_off;
    sl.coff[c] = fc_stage_off(c, stride);
    sl.len[c] = len;
}

__global__ __launch_bounds__(256) void k_rc_sizes(RcArgs a, RcStreams st, Admit admit, const u64* __restrict__ cscan, u32 group,
                                                 const u64* __restrict__ out_cap, u64* __restrict__ out_len, i32* __restrict__ status,
                                                 u64* __restrict__ out_bound, u64* __restrict__ result)
{
    const u32 b = blockIdx.x * 256u + threadIdx.x;
    u64 ok_len = 0, ok = 0, alone = 0;
    if (b == 0) result[0] = st.adirty[a.ns] > st.aslots[a.ns] ? st.adirty[a.ns] : st.aslots[a.ns];
    if (b < a.ns) {
        u32 flags = st.flags[b];
        i32 s = static_cast<i32>(flags & 0xffu);
        u64 bound = st.bound[b], rows = st.rows[b], units = 0;
        if (flags & kWork) {
            s = SNP_ERR_OUTPUT_TOO_SMALL;
            if (admit(b)) {
                if (st.fail[b] != kNoFail) {
                    s = static_cast<i32>(st.fail[b] & 0xff);
                    bound = 0;
                } else {
                    const u64 size = SNP_STREAM_HEADER_LEN + st.kept[b] + (cscan[st.aslots[b + 1]] - cscan[st.aslots[b]]);
                    if (size <= out_cap[b]) {
                        s = SNP_OK;
                        ok_len = size;
                        ok = 1;
                        flags |= kWritten;
                        rows = st.pieces[b];
                        units = rows ? (rows + group - 1) / group : 1;  // (the identifier of an empty stream is a unit's too)
                    }
                }
            }
        } else if (s == SNP_OK) {
            alone = 1;
        }
        status[b] = s;
        out_len[b] = ok_len;
        if (out_bound) out_bound[b] = bound;
        st.flags[b] = flags;
        st.nrows[b] = rows;
        st.units[b] = units;
    }
    add_written(result, ok_len, ok, alone);
}

// One thread per row of the new index, grid-stride, and per stream its three words.  Row i of stream b = owner(nfirst, i): of a stream that is
// not written, one of its old rows (f0 and the count are clamped to nentries: idx_first is untrusted); of a written one, piece i - nfirst[b]:
// kept -- the old chunk, its size from its header -- or rebuilt -- the slot of the dirty row that holds its first byte.  Rows at or past `cap` do
// not exist (a written stream's all do: it was admitted with them).
__global__ __launch_bounds__(256) void k_rc_rows(RcArgs a, RcStreams st, Admit admit, ChunkRows rows, const u64* __restrict__ dstart,
                                                const u64* __restrict__ cscan, RwPieces pc, u64 cap, u64* __restrict__ new_first,
                                                u64* __restrict__ new_start, u64* __restrict__ new_pos, u64* __restrict__ new_total,
                                                i32* __restrict__ new_tail)
{
    const u64 total = st.nfirst[a.ns] < cap ? st.nfirst[a.ns] : cap;
    const u64 most = total > static_cast<u64>(a.ns) + 1 ? total : static_cast<u64>(a.ns) + 1;
    for (u64 i = static_cast<u64>(blockIdx.x) * 256u + threadIdx.x; i < most; i += static_cast<u64>(gridDim.x) * 256u) {
        if (i <= a.ns) new_first[i] = st.nfirst[i] < cap ? st.nfirst[i] : cap;
        if (i < a.ns) {
            new_total[i] = a.x.total[i];
            new_tail[i] = (st.flags[i] & kWritten) ? SNP_OK : a.x.tail[i];
        }
        if (i >= total) continue;
        const u32 b = owner_of(static_cast<const u64*>(st.nfirst), a.ns, i);
        const u64 j = i - st.nfirst[b], f0 = st.f0[b];
        if (!(st.flags[b] & kWritten)) {
            new_start[i] = a.x.start[f0 + j];
            new_pos[i] = a.x.pos[f0 + j];
            pc.src[i] = 0;
            pc.size[i] = 0;
            continue;
        }
        const u64 f1 = f0 + st.rows[b];
        const FrPiece p = fr_piece(a.x, f0, f1, a.x.total[b], a.cb, a.all, j);
        u64 src = 0;
        u32 size = 0;
        if (p.kept) {
            const u64 pos = a.x.pos[p.row];
            src = pos;
            size = static_cast<u32>(frame_hop(a.in + a.in_off[b], a.in_len[b], pos).next - pos);      // (4 + size < 2^24 + 4)
        } else {
            // the stream's last dirty row that starts at or below the piece: the piece lies (at - its start) into what it decodes to
            const u64 t0 = st.adirty[b], t1 = st.adirty[b + 1];
            const u64 t = ix_first_where(t0, t1, [&](u64 q) { return dstart[q] > p.at; });
            const u64 m = t > t0 ? (rows.out_off[t - 1] - st.abytes[b] + (p.at - dstart[t - 1])) / a.cb : ~0ull;
            if (m < st.rebuilt[b]) {                                    // (what the plan saw; else a chunk of no bytes, which the emit skips)
                const u64 c = st.aslots[b] + m;
                src = kRebuilt | c;
                size = static_cast<u32>(cscan[c + 1] - cscan[c]);
            }
        }
        new_start[i] = p.at;
        pc.src[i] = p.kept ? a.in_off[b] + src : src;                   // a kept chunk by its place in `in` (added here: 21 VGPRs, not 25)
        pc.size[i] = size;
    }
}

// workspace (every piece 256-byte aligned; nothing when there is no stream)
struct RechunkWork {
    RcStreams st;
    RwSlots sl;
    RwPieces pc;
    ChunkRows rows;
    u64 *part, *cscan, *dstart;
    u8 *stage, *comp;
    u64 bytes;
};
RechunkWork work_layout(void* base, u32 nstreams, u32 max_slots, u64 stage_cap, u32 chunk_bytes, u32 max_entries)
{
    RechunkWork w{};
    if (nstreams == 0 || chunk_bytes == 0 || chunk_bytes > SNP_BLOCK_SIZE) return w;
    const u64 ns = nstreams, M = max_slots, E = max_entries;
    WorkCarver k(base);
    w.part = k.take<u64>(scan_tiles_of(std::max(std::max(ns, M), E)));
    for (u64** p : {&w.st.f0, &w.st.rows, &w.st.pieces, &w.st.rebuilt, &w.st.kept, &w.st.bound, &w.st.cdirty, &w.st.cslots, &w.st.cstage, &w.st.crows,
                    &w.st.fail, &w.st.nrows, &w.st.units})
        *p = k.take<u64>(ns);
    for (u64** p : {&w.st.adirty, &w.st.aslots, &w.st.abytes, &w.st.arows, &w.st.nfirst, &w.st.gfirst}) *p = k.take<u64>(ns + 1);
    w.st.flags = k.take<u32>(ns);
    w.sl = carve_rw_slots(k, M);
    w.rows = carve_chunk_rows(k, M);
    w.dstart = k.take<u64>(M);
    w.cscan = k.take<u64>(M + 1);
    w.pc = carve_rw_pieces(k, E);
    // staging: per admitted stream what its dirty rows decode to, one behind the other, the streams back to back (+ slack for the compressor's
    // vector loads).  Compressed staging: slot c at c * snp_comp_stride(chunk_bytes) (fc_stage_off).
    w.stage = k.take<u8>(stage_cap + 256);
    w.comp = k.take<u8>(M * snp_comp_stride(chunk_bytes));
    w.bytes = k.bytes();
    return w;
}

}  // namespace

extern "C" {

uint64_t snp_frame_rechunk_indexed_workspace(uint32_t nstreams, uint32_t max_slots, uint64_t stage_cap, uint32_t chunk_bytes, uint32_t max_entries)
{
    return work_layout(nullptr, nstreams, max_slots, stage_cap, chunk_bytes, max_entries).bytes;
}

snp_status snp_frame_rechunk_indexed_batch(snp_ctx* c, const uint8_t* in, const uint64_t* in_off, const uint64_t* in_len, uint32_t nstreams,
                                           const uint64_t* idx_first, const uint64_t* idx_start, const uint64_t* idx_pos, const uint64_t* idx_total,
                                           const int32_t* idx_tail, uint64_t nentries, uint32_t chunk_bytes, uint32_t flags, uint32_t max_slots,
                                           uint64_t stage_cap, uint32_t max_entries, uint8_t* out, const uint64_t* out_off, const uint64_t* out_cap,
                                           uint64_t* out_len, int32_t* status, uint64_t* new_first, uint64_t* new_start, uint64_t* new_pos,
                                           uint64_t* new_total, int32_t* new_tail, uint64_t* out_bound, void* d_work, uint64_t* d_result)
{
    if (!c || !d_result || chunk_bytes == 0 || chunk_bytes > SNP_BLOCK_SIZE || (flags & ~kFrRewriteAll) || nstreams > 0x7fffffffu ||      // (one workgroup per stream)
        (nstreams && (!in || !in_off || !in_len || !idx_first || !idx_total || !idx_tail || !out || !out_off || !out_cap || !out_len || !status ||
                      !new_first || !new_total || !new_tail || !d_work)) ||
        (nstreams && nentries && (!idx_start || !idx_pos)) || (nstreams && max_entries && (!new_start || !new_pos)))
        return SNP_ERR_BAD_ARG;
    DevGuard dg(c);
    if (!dg.ok) return SNP_ERR_DEVICE;
    hipStream_t s = c->stream;
    bool ok = c->check(snp_zero_words_async(reinterpret_cast<u32*>(d_result), 2 * 6, s), "frame rechunk result");
    if (nstreams == 0) return ok ? SNP_OK : SNP_ERR_DEVICE;
    const RechunkWork w = work_layout(d_work, nstreams, max_slots, stage_cap, chunk_bytes, max_entries);
    const u32 ns = nstreams, M = max_slots, E = max_entries, cb = chunk_bytes, sg = groups_of(ns), mg = groups_of(M);
    const RcArgs a{in, in_off, in_len, ns, FrameIndex{idx_first, idx_start, idx_pos, idx_total, idx_tail, nentries}, cb, (flags & kFrRewriteAll) != 0};
    const Admit admit{w.st.flags, w.st.adirty, w.st.aslots, w.st.abytes, w.st.arows, M, stage_cap, E};
    // the plan of every stream; admission in stream order (d_result[2] = staging bytes, [4] = new rows; [0] comes with the verdicts)
    hipLaunchKernelGGL(k_rc_plan, dim3(ns), dim3(256), 0, s, a, w.st);
    ok = ok && c->check(hipGetLastError(), "frame rechunk plan") &&
         c->check(launch_scan(ScanWords{w.st.cdirty}, ns, w.part, w.st.adirty, nullptr, s), "frame rechunk row scan") &&
         c->check(launch_scan(ScanWords{w.st.cslots}, ns, w.part, w.st.aslots, nullptr, s), "frame rechunk slot scan") &&
         c->check(launch_scan(ScanWords{w.st.cstage}, ns, w.part, w.st.abytes, d_result + 2, s), "frame rechunk staging scan") &&
         c->check(launch_scan(ScanWords{w.st.crows}, ns, w.part, w.st.arows, d_result + 4, s), "frame rechunk entry scan");
    if (ok && M) {
        // the dirty rows decoded and verified whole into staging, one behind the other: there the rebuilt pieces lie one behind the other
        hipLaunchKernelGGL(k_rc_clear, dim3(mg), dim3(256), 0, s, M, w.rows, w.dstart);
        hipLaunchKernelGGL(k_rc_fill, dim3(ns), dim3(256), 0, s, a, w.st, admit, w.rows, w.dstart);
        ok = c->check(hipGetLastError(), "frame rechunk fill") && c->decode_chunks(in, w.rows, M, w.stage);
        if (ok) {
            hipLaunchKernelGGL(k_rc_fail, dim3(mg), dim3(256), 0, s, ns, M, w.rows, w.st);
            hipLaunchKernelGGL(k_rc_slots, dim3(mg), dim3(256), 0, s, a, w.st, admit, w.sl, snp_comp_stride(cb));
            ok = c->check(hipGetLastError(), "frame rechunk slots");
        }
    }
    // every rebuilt piece re-encoded from staging and the framed sizes; every stream's verdict, its emit units and the rows of its new index
    ok = ok && reencode_slots(c, w.stage, w.sl, M, w.comp, w.part, w.cscan, "frame rechunk");
    if (ok) {
        const u32 group = fc_group(cb);
        hipLaunchKernelGGL(k_rc_sizes, dim3(sg), dim3(256), 0, s, a, w.st, admit, w.cscan, group, out_cap, out_len, status, out_bound, d_result);
        ok = c->check(hipGetLastError(), "frame rechunk sizes") &&
             c->check(launch_scan(ScanWords{w.st.units}, ns, w.part, w.st.gfirst, nullptr, s), "frame rechunk unit scan") &&
             c->check(launch_scan(ScanWords{w.st.nrows}, ns, w.part, w.st.nfirst, nullptr, s), "frame rechunk new row scan");
        if (ok) {
            const u64 most = std::max<u64>(E, static_cast<u64>(ns) + 1);
            hipLaunchKernelGGL(k_rc_rows, dim3(static_cast<u32>(std::min<u64>((most + 255) / 256, kRowGroups))), dim3(256), 0, s, a, w.st, admit, w.rows,
                               w.dstart, w.cscan, w.pc, E, new_first, new_start, new_pos, new_total, new_tail);
            ok = c->check(hipGetLastError(), "frame rechunk rows") &&
                 c->check(launch_scan(ScanPieces{w.pc.size, w.st.nfirst + ns, E}, E, w.part, w.pc.scan, nullptr, s), "frame rechunk chunk scan");
            if (ok) {
                hipLaunchKernelGGL(k_rw_emit<RwOwners>, dim3(kEmitGroups), dim3(256), 0, s, RwOwners{w.st.gfirst, w.st.nfirst, ns}, w.sl, w.pc, group, fc_team(group),
                                   in, w.stage, w.comp, out, out_off, new_pos);
                ok = c->check(hipGetLastError(), "frame rechunk emit");
            }
        }
    }
    return ok ? SNP_OK : SNP_ERR_DEVICE;
}

}  // extern "C"

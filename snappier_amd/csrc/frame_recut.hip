// frame_recut.hip -- snp_frame_recut_indexed_batch: framed streams kept with their chunk index brought to the pieces of a caller's CUT LIST --
// what snp_frame_encode_cuts_batch writes for their decoded bytes and that list -- out of place, with the new index.  An old chunk that already
// is a piece of the new stream is copied; only the other pieces are decoded and compressed again, with no read-back between the two.  The
// rechunk (frame_rechunk.hip) with the list in place of the grid: frame_recut_device.h plans a stream, frame_rows_device.h holds the checks over
// the old rows that both calls make, and the slot table, its re-encode, the piece table and the emit of one slot are frame_rewrite_device.h's.
// Built into libsnappier_hip_frame_recut.so (C-ABI: include/snappier_hip_frame_recut.h), linked against libsnappier_hip.so.  DESIGN.md 4.28.
//
//   plan      a workgroup per stream: the verdict over its cut list (rx_cut, rx_tail), then its rows (rx_row, rx_add: the partition, every header,
//             clean or dirty by ONE search in the list), joined over the workgroup; thread 0: rx_finish
//   scans     dirty rows, rebuilt pieces, the staging budget, new rows -> admission in stream order; d_result[2], [4]; the decoded bytes
//   clear     one thread per row of the decode table: an empty row
//   fill      a workgroup per admitted stream walks its rows again: dirty row j -> row adirty[b] + j of the table, decoded behind the dirty rows
//             before it, with where it starts and the rebuilt pieces that start in the rows before it
//   decode    snp_ctx::decode_chunks over the table into staging; fail: one thread per row, a failing row -> its stream (the first in order)
//   slots     one thread per table slot: the m-th rebuilt piece of its stream -- the dirty row it starts in by a search in that scan, its length
//             from the list, its bytes where the row was decoded to
//   strides   a scan of snp_comp_stride over the slots in use; coff: the decoded bytes grow from the front of the staging, the compressed
//             bytes from its back, an empty slot has 64 bytes of its own behind both
//   re-encode reencode_slots: snp_ctx::launch_compress and snp_launch_crc32c over every slot -- once each, from staging; the scan of 8 + payload
//   sizes     one thread per stream: size against out_cap, status, out_len, out_bound, d_result[0], [1], [3], [5], [6], [7]; its emit units
//   scans     emit units, rows of the new index
//   rows      one thread per new row: an old row copied, or piece j of a written stream -- kept (the old chunk's place in `in` and size) or
//             rebuilt (its slot and framed size); per stream: new_first, new_total, new_tail
//   scan      the chunk sizes of the new rows -> where each chunk lies
//   emit      one 256-thread workgroup per unit, grid-stride: the pieces that START in 64 KiB of what the stream decodes to, a team each: a kept
//             chunk copied from `in`, or header + payload from staging; new_pos of the row
// No atomic decides an order or a value of an output: the only ones add to sums.  Nothing here allocates, reads back or synchronises: the call is
// capturable like the other _batch entry points.
#include "capi_internal.h"
#include "frame_rewrite_device.h"
#include "frame_recut_device.h"
#include "../../include/snappier_hip_frame_recut.h"

static_assert(kRxRewriteAll == SNP_RECUT_REWRITE_ALL, "flag");
static_assert(ec_stride(SNP_BLOCK_SIZE) == kSnpCompStride && ec_stride(4096) == snp_comp_stride(4096) && ec_stride(0) == 64, "staging stride");

namespace {

constexpr u32 kWork = 0x100u, kWritten = 0x400u;                    // stream flags above the status byte
constexpr u64 kEmptySlot = 64;                                      // ec_stride(0): what the compressor may touch of an empty slot

struct RxArgs {
    const u8* in;
    const u64 *in_off, *in_len;
    u32 ns;
    FrameIndex x;
    const u64 *cut_first, *cuts;
    u64 ncuts;
    bool all;
};
// per stream
struct RxStreams {
    u64 *f0, *rows, *pieces, *rebuilt, *copied, *kept, *bound;
    u64 *cdirty, *cslots, *cstage, *cdec, *crows;           // what the stream asks of each bound; the decoded part of its staging
    u64 *fail;                                              // min over its failing dirty rows of (table row << 8 | status)
    u64 *nrows, *units;                                     // rows of its new index; emit units
    u64 *adirty, *aslots, *abytes, *adec, *arows, *nfirst, *gfirst;    // scans (n + 1): of the five counts; new rows; emit units
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

// the staging: decoded bytes from 0 up, compressed bytes from `top` down (a multiple of 16, as the compressor's staged stores want it), slot c's
// 64 bytes when it is empty at top + 64 c.  Admission holds decoded + compressed <= stage_cap, so with stage_cap rounded UP to 16 the lowest
// compressed byte lies at least 256 bytes above the last decoded one: the slack the rechunk's own staging keeps behind its decoded bytes for
// the compressor's vector loads past a slot's input (they read, never write, there).
__host__ __device__ __forceinline__ u64 stage_top(u64 stage_cap) { return ((stage_cap + 15) & ~15ull) + 256; }

// what the threads of a workgroup found, joined (every thread gets the result); s: 8 words of LDS
__device__ __forceinline__ RxAcc block_join(RxAcc a, u64* s)
{
    if (threadIdx.x < 8) s[threadIdx.x] = 0;
    __syncthreads();
    const u64 bits = wave_sum((a.rows.bad ? 1ull : 0) | (a.rows.loose ? 1ull << 16 : 0) | (a.badlist ? 1ull << 32 : 0));     // (64 lanes: no carry between the fields)
    const u64 v[6] = {wave_sum(a.rows.dirty), wave_sum(a.rows.dbytes), wave_sum(a.rows.clean), wave_sum(a.rows.kept), wave_sum(a.pstride), wave_sum(a.cstride)};
    if ((threadIdx.x & 63u) == 0) {
        for (u32 i = 0; i < 6; ++i) atomic_add64(s + i, v[i]);
        atomic_add64(s + 6, bits);
    }
    __syncthreads();
    RxAcc r{};
    r.rows.dirty = s[0];
    r.rows.dbytes = s[1];
    r.rows.clean = s[2];
    r.rows.kept = s[3];
    r.pstride = s[4];
    r.cstride = s[5];
    r.rows.bad = (s[6] & 0xffffull) != 0;
    r.rows.loose = ((s[6] >> 16) & 0xffffull) != 0;
    r.badlist = (s[6] >> 32) != 0;
    return r;
}

// A workgroup per stream.  The stream steers the whole workgroup.
__global__ __launch_bounds__(256) void k_rx_plan(RxArgs a, RxStreams st)
{
    __shared__ u64 s_acc[8];
    const u32 b = blockIdx.x;
    const u8* const s = a.in + a.in_off[b];
    const u64 n = a.in_len[b], lo = a.cut_first[b], hi = a.cut_first[b + 1];
    const i32 begin = fr_begin(a.x, b);
    const bool range = ec_range_ok(lo, hi, a.ncuts);
    RxAcc acc{};
    if (begin == SNP_OK && range) {
        const u64 total = a.x.total[b];
        for (u64 i = lo + threadIdx.x; i < hi; i += 256u) rx_cut(&acc, a.cuts, lo, i, total);
        if (threadIdx.x == 0) rx_tail(&acc, a.cuts, lo, hi, total);
        u64 f0, rows;
        fr_rows(a.x, b, &f0, &rows);
        const u64 f1 = f0 + rows;
        for (u64 i = f0 + threadIdx.x; i < f1; i += 256u)
            rx_add(&acc, a.x, f0, f1, total, n, i, rx_row(a.x, f0, f1, total, n, a.cuts, lo, hi, a.all, i, [&](u64 pos) { return frame_hop(s, n, pos); }));
    }
    acc = block_join(acc, s_acc);
    if (threadIdx.x != 0) return;
    const RxPlan k = rx_finish(a.x, b, n, lo, hi, range, a.all, fr_ident(s, n), begin, acc);
    st.f0[b] = k.f0;
    st.rows[b] = k.rows;
    st.pieces[b] = k.pieces;
    st.rebuilt[b] = k.rebuilt;
    st.copied[b] = k.copied;
    st.kept[b] = k.kept;
    st.bound[b] = k.work ? k.bound : 0;
    st.cdirty[b] = rx_count_dirty(k);
    st.cslots[b] = rx_count_slots(k);
    st.cstage[b] = rx_count_stage(k);
    st.cdec[b] = rx_count_dec(k);
    st.crows[b] = rx_count_rows(k);
    st.fail[b] = kNoFail;
    st.flags[b] = static_cast<u32>(k.status) | (k.work ? kWork : 0u);
}

// One thread per row of the decode table: an empty row.
__global__ __launch_bounds__(256) void k_rx_clear(u32 max_slots, ChunkRows rows, u64* __restrict__ dstart, u64* __restrict__ pfirst)
{
    const u32 t = blockIdx.x * 256u + threadIdx.x;
    if (t >= max_slots) return;
    rows.tag[t] = kNone;
    chunk_row_clear(rows, t, 0);
    dstart[t] = 0;
    pfirst[t] = 0;
}

// A workgroup per admitted stream walks its rows again, 256 at a time, with the dirty rows, their decoded bytes and the pieces that start in them
// so far: dirty row j of the stream is row adirty[b] + j of the table and decodes to the stream's decoded staging + the decoded bytes of the dirty
// rows before it.
__global__ __launch_bounds__(256) void k_rx_fill(RxArgs a, RxStreams st, Admit admit, ChunkRows rows, u64* __restrict__ dstart, u64* __restrict__ pfirst)
{
    __shared__ u64 s_cnt[4], s_byt[4], s_pcs[4];
    const u32 b = blockIdx.x;
    if (!admit(b)) return;
    const u8* const s = a.in + a.in_off[b];
    const u64 n = a.in_len[b], f0 = st.f0[b], f1 = f0 + st.rows[b], total = a.x.total[b], lo = a.cut_first[b], hi = a.cut_first[b + 1];
    const u64 t0 = st.adirty[b], t1 = st.adirty[b + 1], place0 = st.adec[b], place1 = st.adec[b + 1];
    const u32 wave = threadIdx.x >> 6;
    u64 cnt0 = 0, byt0 = 0, pcs0 = 0;                                   // of the rows before this round
    for (u64 base = f0; base < f1; base += 256u) {
        const u64 i = base + threadIdx.x;
        FrRow r{};
        if (i < f1) r = rx_row(a.x, f0, f1, total, n, a.cuts, lo, hi, a.all, i, [&](u64 pos) { return frame_hop(s, n, pos); });
        const bool dirty = r.ok && !r.clean;
        u64 wc, wb, wp;
        u64 cnt = wave_scan(dirty ? 1 : 0, &wc), byt = wave_scan(dirty ? r.len : 0, &wb);
        u64 pcs = wave_scan(dirty ? rx_row_pieces(a.cuts, lo, hi, r.start, r.len) : 0, &wp);
        if ((threadIdx.x & 63u) == 63u) { s_cnt[wave] = wc; s_byt[wave] = wb; s_pcs[wave] = wp; }
        __syncthreads();
        u64 allc = 0, allb = 0, allp = 0;
        for (u32 w = 0; w < 4; ++w) {
            if (w < wave) { cnt += s_cnt[w]; byt += s_byt[w]; pcs += s_pcs[w]; }
            allc += s_cnt[w];
            allb += s_byt[w];
            allp += s_pcs[w];
        }
        const u64 t = t0 + cnt0 + cnt, place = place0 + byt0 + byt;
        if (dirty && t < t1 && place + r.len <= place1) {               // (what the plan saw: they fit)
            rows.tag[t] = static_cast<u32>(t);
            chunk_row_set(rows, t, r.h, a.in_off[b] + r.pos, place);
            dstart[t] = r.start;
            pfirst[t] = pcs0 + pcs;
        }
        cnt0 += allc;
        byt0 += allb;
        pcs0 += allp;
        __syncthreads();
    }
}

// a dirty row that did not decode or verify: its status to its stream, the first row's in stream order
__global__ __launch_bounds__(256) void k_rx_fail(u32 ns, u32 max_slots, ChunkRows rows, RxStreams st)
{
    const u32 t = blockIdx.x * 256u + threadIdx.x;
    if (t >= max_slots || rows.tag[t] == kNone) return;
    const i32 s = row_verdict(rows, t);
    if (s != SNP_OK) atomic_min64(st.fail + owner_of(static_cast<const u64*>(st.adirty), ns, t), (static_cast<u64>(t) << 8) | static_cast<u64>(s & 0xff));
}

// One thread per table slot: the m-th rebuilt piece of its stream -- its length from the list, its bytes in staging.
__global__ __launch_bounds__(256) void k_rx_slots(RxArgs a, RxStreams st, Admit admit, ChunkRows rows, const u64* __restrict__ dstart,
                                                 const u64* __restrict__ pfirst, RwSlots sl)
{
    const u32 c = blockIdx.x * 256u + threadIdx.x;
    if (c >= admit.max_slots) return;
    u64 in_off = 0;
    u32 len = 0;
    if (c < st.aslots[a.ns]) {
        const u32 b = fc_owner(st.aslots, a.ns, c);
        if (admit(b) && st.fail[b] == kNoFail) {
            const u64 m = c - st.aslots[b], t0 = st.adirty[b], t1 = st.adirty[b + 1], lo = a.cut_first[b], hi = a.cut_first[b + 1], total = a.x.total[b];
            // the stream's last dirty row with no more than m rebuilt pieces before it: the m-th starts in it
            const u64 t = ix_first_where(t0, t1, [&](u64 q) { return rows.tag[q] == kNone || pfirst[q] > m; });
            if (t > t0) {
                const u64 s = dstart[t - 1], j = rx_piece_of_slot(a.cuts, lo, hi, s, pfirst[t - 1], m);
                if (j < ec_pieces(lo, hi, total)) {
                    u64 at;
                    const u32 want = ec_piece(a.cuts, lo, hi, total, j, &at);
                    const u64 place = rx_place(rows.out_off[t - 1], s, at);
                    // (what the plan saw: the rebuilt pieces are the dirty rows' bytes)
                    if (at >= s && want <= SNP_BLOCK_SIZE && place >= st.adec[b] && place + want <= st.adec[b + 1]) {
                        in_off = place;
                        len = want;
                    }
                }
            }
        }
    }
    sl.in_off[c] = in_off;
    sl.len[c] = len;
}

struct ScanUsedStrides {
    const u32* __restrict__ len;
    __device__ __forceinline__ u64 operator()(u64 i) const { return len[i] ? ec_stride(len[i]) : 0; }
};

// One thread per table slot: where its compressed bytes are staged.  The slots in use lie back to back below `top`, in slot order downwards; what
// the streams up to and including the slot's own asked of the budget holds them above the decoded bytes.
__global__ __launch_bounds__(256) void k_rx_coff(u32 ns, RxStreams st, Admit admit, RwSlots sl, const u64* __restrict__ gscan)
{
    const u32 c = blockIdx.x * 256u + threadIdx.x;
    if (c >= admit.max_slots) return;
    const u64 top = stage_top(admit.stage_cap);
    u64 off = top + kEmptySlot * c;
    if (sl.len[c]) {
        const u32 b = fc_owner(st.aslots, ns, c);                       // (a slot in use: c < aslots[ns], its stream admitted)
        if (gscan[c + 1] <= st.abytes[b + 1] - st.adec[b + 1]) off = top - gscan[c + 1];
        else sl.len[c] = 0;                                             // (never with the plan's own sums)
    }
    sl.coff[c] = off;
}

__global__ __launch_bounds__(256) void k_rx_sizes(RxArgs a, RxStreams st, Admit admit, const u64* __restrict__ cscan, const u64* __restrict__ out_cap,
                                                 u64* __restrict__ out_len, i32* __restrict__ status, u64* __restrict__ out_bound, u64* __restrict__ result)
{
    const u32 b = blockIdx.x * 256u + threadIdx.x;
    u64 ok_len = 0, ok = 0, alone = 0, copied = 0, rebuilt = 0;
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
                        copied = st.copied[b];
                        rebuilt = st.rebuilt[b];
                        const u64 total = a.x.total[b];
                        units = total ? (total + kUnit - 1) / kUnit : 1;    // (the identifier of an empty stream is a unit's too)
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
    copied = wave_sum(copied);
    rebuilt = wave_sum(rebuilt);
    if ((threadIdx.x & 63u) == 0) {
        if (copied) atomic_add64(result + 6, copied);
        if (rebuilt) atomic_add64(result + 7, rebuilt);
    }
}

// One thread per row of the new index, grid-stride, and per stream its three words.  Row i of stream b = owner(nfirst, i): of a stream that is
// not written, one of its old rows (f0 and the count are clamped to nentries: idx_first is untrusted); of a written one, piece i - nfirst[b]:
// kept -- the old chunk, its size from its header -- or rebuilt -- its slot, through the dirty row that holds its first byte.  Rows at or past
// `cap` do not exist (a written stream's all do: it was admitted with them).
__global__ __launch_bounds__(256) void k_rx_rows(RxArgs a, RxStreams st, ChunkRows rows, const u64* __restrict__ dstart, const u64* __restrict__ pfirst,
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
        const u64 f1 = f0 + st.rows[b], lo = a.cut_first[b], hi = a.cut_first[b + 1];
        const RxPiece p = rx_piece(a.x, f0, f1, a.x.total[b], a.cuts, lo, hi, a.all, j);
        u64 src = 0;
        u32 size = 0;
        if (p.kept) {
            const u64 pos = a.x.pos[p.row];
            src = a.in_off[b] + pos;                                    // a kept chunk by its place in `in`
            size = static_cast<u32>(frame_hop(a.in + a.in_off[b], a.in_len[b], pos).next - pos);      // (4 + size < 2^24 + 4)
        } else {
            // the stream's last dirty row that starts at or below the piece: the piece starts in it
            const u64 t0 = st.adirty[b], t1 = st.adirty[b + 1];
            const u64 t = ix_first_where(t0, t1, [&](u64 q) { return rows.tag[q] == kNone || dstart[q] > p.at; });
            const u64 m = t > t0 ? rx_slot_of_piece(a.cuts, lo, hi, dstart[t - 1], pfirst[t - 1], j) : ~0ull;
            if (m < st.rebuilt[b]) {                                    // (what the plan saw; else a chunk of no bytes, which the emit skips)
                const u64 c = st.aslots[b] + m;
                src = kRebuilt | c;
                size = static_cast<u32>(cscan[c + 1] - cscan[c]);
            }
        }
        new_start[i] = p.at;
        pc.src[i] = src;
        pc.size[i] = size;
    }
}

// One workgroup per emit unit of a written stream at a time: the pieces that START in 64 KiB of what the stream decodes to (pieces vary in
// size: a unit is cut by bytes, as the encoder at given cuts cuts them), taken by teams of threads in turn -- the whole workgroup on one piece,
// half on each of two, else a wavefront each.  A kept chunk is copied from `in` as it is; a rebuilt one is emit_slot.  The first unit of a
// stream writes the identifier.
__global__ __launch_bounds__(256) void k_rx_emit(RxArgs a, RxStreams st, RwSlots sl, RwPieces pc, const u8* __restrict__ stage, const u8* __restrict__ comp,
                                                u8* __restrict__ out, const u64* __restrict__ out_off, u64* __restrict__ new_pos)
{
    const u32 tid = threadIdx.x;
    const u64 units = st.gfirst[a.ns];
    for (u64 g = blockIdx.x; g < units; g += gridDim.x) {
        const u32 b = fc_owner(st.gfirst, a.ns, g);
        const u64 u = g - st.gfirst[b], lo = a.cut_first[b], hi = a.cut_first[b + 1], total = a.x.total[b];
        const u64 first = st.nfirst[b], np = st.nfirst[b + 1] - first;
        const u64 k0 = ec_first_piece_from(a.cuts, lo, hi, u * kUnit);
        u64 k1 = (u + 1) * kUnit >= total ? np : ec_first_piece_from(a.cuts, lo, hi, (u + 1) * kUnit);
        k1 = k1 < np ? k1 : np;                                         // (the rows the stream has)
        const u32 team = fc_team(k1 > k0 + 2 ? 3u : k1 > k0 ? static_cast<u32>(k1 - k0) : 1u), t = tid % team, teams = 256u / team;
        u8* const dst = out + out_off[b];
        if (u == 0 && tid < SNP_STREAM_HEADER_LEN) dst[tid] = k_fc_stream_id[tid];       // EnsureStreamHeaderWritten  SnappyStreamCompressor.cs:148-157
        for (u64 k = k0 + tid / team; k < k1; k += teams) {
            const u64 i = first + k, src = pc.src[i], pos = SNP_STREAM_HEADER_LEN + (pc.scan[i] - pc.scan[first]);
            if (t == 0) new_pos[i] = pos;
            if (pc.size[i] == 0) continue;
            if (src & kRebuilt) emit_slot(dst + pos, sl, src & ~kRebuilt, stage, comp, t, team);
            else team_copy(dst + pos, a.in + src, pc.size[i], t, team);
        }
    }
}

// workspace (every piece 256-byte aligned; nothing when there is no stream)
struct RecutWork {
    RxStreams st;
    RwSlots sl;
    RwPieces pc;
    ChunkRows rows;
    u64 *part, *cscan, *gscan, *dstart, *pfirst;
    u8* stage;
    u64 bytes;
};
RecutWork work_layout(void* base, u32 nstreams, u32 max_slots, u64 stage_cap, u32 max_entries)
{
    RecutWork w{};
    if (nstreams == 0) return w;
    const u64 ns = nstreams, M = max_slots, E = max_entries;
    WorkCarver k(base);
    w.part = k.take<u64>(scan_tiles_of(std::max(std::max(ns, M), E)));
    for (u64** p : {&w.st.f0, &w.st.rows, &w.st.pieces, &w.st.rebuilt, &w.st.copied, &w.st.kept, &w.st.bound, &w.st.cdirty, &w.st.cslots, &w.st.cstage,
                    &w.st.cdec, &w.st.crows, &w.st.fail, &w.st.nrows, &w.st.units})
        *p = k.take<u64>(ns);
    for (u64** p : {&w.st.adirty, &w.st.aslots, &w.st.abytes, &w.st.adec, &w.st.arows, &w.st.nfirst, &w.st.gfirst}) *p = k.take<u64>(ns + 1);
    w.st.flags = k.take<u32>(ns);
    w.sl = carve_rw_slots(k, M);
    w.rows = carve_chunk_rows(k, M);
    w.dstart = k.take<u64>(M);
    w.pfirst = k.take<u64>(M);
    w.gscan = k.take<u64>(M + 1);
    w.cscan = k.take<u64>(M + 1);
    w.pc = carve_rw_pieces(k, E);
    // ONE staging for both: per admitted stream what its dirty rows decode to, one behind the other from the front, the streams back to back; the
    // compressed bytes of the slots in use from stage_top down; 64 bytes per slot that may stay empty behind that
    w.stage = k.take<u8>(stage_top(stage_cap) + kEmptySlot * M);
    w.bytes = k.bytes();
    return w;
}

}  // namespace

extern "C" {

uint64_t snp_frame_recut_indexed_workspace(uint32_t nstreams, uint32_t max_slots, uint64_t stage_cap, uint32_t max_entries)
{
    return work_layout(nullptr, nstreams, max_slots, stage_cap, max_entries).bytes;
}

snp_status snp_frame_recut_indexed_batch(snp_ctx* c, const uint8_t* in, const uint64_t* in_off, const uint64_t* in_len, uint32_t nstreams,
                                         const uint64_t* idx_first, const uint64_t* idx_start, const uint64_t* idx_pos, const uint64_t* idx_total,
                                         const int32_t* idx_tail, uint64_t nentries, const uint64_t* cut_first, const uint64_t* cuts, uint64_t ncuts,
                                         uint32_t flags, uint32_t max_slots, uint64_t stage_cap, uint32_t max_entries, uint8_t* out,
                                         const uint64_t* out_off, const uint64_t* out_cap, uint64_t* out_len, int32_t* status, uint64_t* new_first,
                                         uint64_t* new_start, uint64_t* new_pos, uint64_t* new_total, int32_t* new_tail, uint64_t* out_bound, void* d_work,
                                         uint64_t* d_result)
{
    if (!c || !d_result || (flags & ~kRxRewriteAll) || nstreams > 0x7fffffffu ||      // (one workgroup per stream)
        (nstreams && (!in || !in_off || !in_len || !idx_first || !idx_total || !idx_tail || !cut_first || !out || !out_off || !out_cap || !out_len ||
                      !status || !new_first || !new_total || !new_tail || !d_work)) ||
        (nstreams && nentries && (!idx_start || !idx_pos)) || (nstreams && ncuts && !cuts) || (nstreams && max_entries && (!new_start || !new_pos)))
        return SNP_ERR_BAD_ARG;
    DevGuard dg(c);
    if (!dg.ok) return SNP_ERR_DEVICE;
    hipStream_t s = c->stream;
    const char* const what = "frame recut";
    bool ok = check_step(c, snp_zero_words_async(reinterpret_cast<u32*>(d_result), 2 * 8, s), what, "result");
    if (nstreams == 0) return ok ? SNP_OK : SNP_ERR_DEVICE;
    const RecutWork w = work_layout(d_work, nstreams, max_slots, stage_cap, max_entries);
    const u32 ns = nstreams, M = max_slots, E = max_entries, sg = groups_of(ns), mg = groups_of(M);
    const RxArgs a{in, in_off, in_len, ns, FrameIndex{idx_first, idx_start, idx_pos, idx_total, idx_tail, nentries}, cut_first, cuts, ncuts,
                   (flags & kRxRewriteAll) != 0};
    const Admit admit{w.st.flags, w.st.adirty, w.st.aslots, w.st.abytes, w.st.arows, M, stage_cap, E};
    u8* const comp = w.stage;                                           // (one region: sl.coff is counted from its first byte too)
    // the plan of every stream; admission in stream order (d_result[2] = staging bytes, [4] = new rows; [0] comes with the verdicts)
    hipLaunchKernelGGL(k_rx_plan, dim3(ns), dim3(256), 0, s, a, w.st);
    ok = ok && check_step(c, hipGetLastError(), what, "plan") &&
         check_step(c, launch_scan(ScanWords{w.st.cdirty}, ns, w.part, w.st.adirty, nullptr, s), what, "row scan") &&
         check_step(c, launch_scan(ScanWords{w.st.cslots}, ns, w.part, w.st.aslots, nullptr, s), what, "slot scan") &&
         check_step(c, launch_scan(ScanWords{w.st.cstage}, ns, w.part, w.st.abytes, d_result + 2, s), what, "staging scan") &&
         check_step(c, launch_scan(ScanWords{w.st.cdec}, ns, w.part, w.st.adec, nullptr, s), what, "decoded scan") &&
         check_step(c, launch_scan(ScanWords{w.st.crows}, ns, w.part, w.st.arows, d_result + 4, s), what, "entry scan");
    if (ok && M) {
        // the dirty rows decoded and verified whole into staging, one behind the other: there the rebuilt pieces lie one behind the other
        hipLaunchKernelGGL(k_rx_clear, dim3(mg), dim3(256), 0, s, M, w.rows, w.dstart, w.pfirst);
        hipLaunchKernelGGL(k_rx_fill, dim3(ns), dim3(256), 0, s, a, w.st, admit, w.rows, w.dstart, w.pfirst);
        ok = check_step(c, hipGetLastError(), what, "fill") && c->decode_chunks(in, w.rows, M, w.stage);
        if (ok) {
            hipLaunchKernelGGL(k_rx_fail, dim3(mg), dim3(256), 0, s, ns, M, w.rows, w.st);
            hipLaunchKernelGGL(k_rx_slots, dim3(mg), dim3(256), 0, s, a, w.st, admit, w.rows, w.dstart, w.pfirst, w.sl);
            ok = check_step(c, hipGetLastError(), what, "slots") &&
                 check_step(c, launch_scan(ScanUsedStrides{w.sl.len}, M, w.part, w.gscan, nullptr, s), what, "stride scan");
        }
        if (ok) {
            hipLaunchKernelGGL(k_rx_coff, dim3(mg), dim3(256), 0, s, ns, w.st, admit, w.sl, w.gscan);
            ok = check_step(c, hipGetLastError(), what, "staging places");
        }
    }
    // every rebuilt piece re-encoded from staging and the framed sizes; every stream's verdict, its emit units and the rows of its new index
    ok = ok && reencode_slots(c, w.stage, w.sl, M, comp, w.part, w.cscan, what);
    if (ok) {
        hipLaunchKernelGGL(k_rx_sizes, dim3(sg), dim3(256), 0, s, a, w.st, admit, w.cscan, out_cap, out_len, status, out_bound, d_result);
        ok = check_step(c, hipGetLastError(), what, "sizes") &&
             check_step(c, launch_scan(ScanWords{w.st.units}, ns, w.part, w.st.gfirst, nullptr, s), what, "unit scan") &&
             check_step(c, launch_scan(ScanWords{w.st.nrows}, ns, w.part, w.st.nfirst, nullptr, s), what, "new row scan");
        if (ok) {
            const u64 most = std::max<u64>(E, static_cast<u64>(ns) + 1);
            hipLaunchKernelGGL(k_rx_rows, dim3(static_cast<u32>(std::min<u64>((most + 255) / 256, kRowGroups))), dim3(256), 0, s, a, w.st, w.rows, w.dstart,
                               w.pfirst, w.cscan, w.pc, E, new_first, new_start, new_pos, new_total, new_tail);
            ok = check_step(c, hipGetLastError(), what, "rows") &&
                 check_step(c, launch_scan(ScanPieces{w.pc.size, w.st.nfirst + ns, E}, E, w.part, w.pc.scan, nullptr, s), what, "chunk scan");
            if (ok) {
                hipLaunchKernelGGL(k_rx_emit, dim3(kEmitGroups), dim3(256), 0, s, a, w.st, w.sl, w.pc, w.stage, comp, out, out_off, new_pos);
                ok = check_step(c, hipGetLastError(), what, "emit");
            }
        }
    }
    return ok ? SNP_OK : SNP_ERR_DEVICE;
}

}  // extern "C"

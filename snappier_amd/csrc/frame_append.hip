// frame_append.hip -- snp_frame_append_indexed_batch: bytes appended IN PLACE to framed streams kept with their chunk index, each stream inside a
// region of its own that it may grow into.  The tail chunk is reopened when it is short and physically last, the rest follows in fresh chunks,
// and the new index comes with it.  frame_append_device.h plans a stream, frame_chunked_device.h cuts the appended bytes into slots, the decode
// of a reopened tail is the update call's edge decode.  Built into libsnappier_hip_frame_append.so (C-ABI: include/snappier_hip_frame_append.h),
// linked against libsnappier_hip.so.  DESIGN.md 4.18.
//
//   plan      one thread per stream (fa_plan): the verdict so far, reopen or not, fill, cut, fresh slots, the size bound
//   scans     reopened tails and fresh slots of the streams that passed -> admission in stream order; d_result[2], [0]
//   tails     one thread per tail slot: its stream, its decode row, where it is staged
//   decode    snp_ctx::decode_chunks over the tail table into raw staging; fail: a failing tail -> its stream
//   overlay   one workgroup per tail slot, grid-stride: the fill bytes behind the decoded tail
//   fresh     one thread per fresh slot (fc_owner, fa_piece): its stream, its piece of src, where its compressed bytes are staged
//   compress  snp_ctx::launch_compress and snp_launch_crc32c over the tail table (from the raw staging) and over the fresh table (straight from src)
//   scan      8 + payload per fresh slot
//   sizes     one thread per stream: size against buf_cap, status, new_len, out_bound, d_result[1] and [3]; the rows of its new index
//   scan      rows of the new index -> new_first
//   emit      one 256-thread workgroup per fc_group(chunk_bytes) consecutive slots, grid-stride, first over the tail table and then over the fresh one:
//             header + payload at its stream's place, the identifier of an empty stream
//   rows      one thread per new row: an old row copied, or a fresh chunk's row from the size scan; per stream: new_first, new_total, new_tail
// Nothing here allocates, reads back or synchronises: the call is capturable like the other _batch entry points.
#include "capi_internal.h"
#include "frame_rewrite_device.h"
#include "frame_append_device.h"
#include "../../include/snappier_hip_frame_append.h"

namespace {

constexpr u32 kAppend = 0x100u, kReopen = 0x200u, kIdent = 0x400u, kWritten = 0x800u;    // stream flags above the status byte
constexpr u32 kOverlayGroups = 8192;                                // grid of the grid-stride overlay

struct ApArgs {
    u8* buf;
    const u64 *buf_off, *buf_len, *buf_cap;
    u32 ns;
    FrameIndex x;
    const u8* src;
    const u64 *src_off, *src_len;
    u32 cb;
};
// per stream
struct ApStreams {
    u64 *f0, *rows, *cut, *rest, *bound, *base, *nrows;     // base: where the first fresh chunk goes (stream-relative); nrows: rows of its new index
    u64 *tails, *fresh;                                     // what the stream asks of each table (0 unless it passed with bytes to take)
    u64 *atails, *aslots, *nfirst;                          // scans (n + 1): tails / fresh slots of the streams before b; new rows before b
    u32 *flags, *d, *fill;
    i32* fail;                                              // the status of a reopened tail that did not decode or verify
};
using ApSlots = RwOwnedSlots;                               // per slot of either table, tails and fresh

// admission in stream order: both sums only grow
struct Admit {
    const u32* flags;
    const u64* __restrict__ atails;
    const u64* __restrict__ aslots;
    u32 max_tails, max_slots;
    __device__ __forceinline__ bool operator()(u32 b) const { return (flags[b] & kAppend) && atails[b + 1] <= max_tails && aslots[b + 1] <= max_slots; }
};

__global__ __launch_bounds__(256) void k_fa_plan(ApArgs a, ApStreams st)
{
    const u32 b = blockIdx.x * 256u + threadIdx.x;
    if (b >= a.ns) return;
    const u8* const s = a.buf + a.buf_off[b];
    const u64 n = a.buf_len[b];
    const FaPlan k = fa_plan(a.x, b, n, a.src_len[b], a.cb, [&](u64 pos) { return frame_hop(s, n, pos); });
    st.f0[b] = k.f0;
    st.rows[b] = k.rows;
    st.cut[b] = k.cut;
    st.rest[b] = k.rest;
    st.bound[b] = k.bound;
    st.base[b] = 0;
    st.tails[b] = k.append && k.reopen;
    st.fresh[b] = !k.append ? 0 : k.fresh < (1ull << 32) ? k.fresh : 1ull << 32;     // (no bound admits 2^32 slots: counted as that, so that the scan cannot wrap)
    st.flags[b] = static_cast<u32>(k.status) | (k.append ? kAppend : 0u) | (k.reopen ? kReopen : 0u) | (k.ident ? kIdent : 0u);
    st.d[b] = k.d;
    st.fill[b] = k.fill;
    st.fail[b] = SNP_OK;
}

// One thread per tail slot: the reopened tail of an admitted stream as a decode row into the raw staging (slot t at t * cb), else an empty row.
__global__ __launch_bounds__(256) void k_fa_tails(ApArgs a, ApStreams st, Admit admit, ApSlots tl, ChunkRows rows, u64 stride)
{
    const u32 t = blockIdx.x * 256u + threadIdx.x;
    if (t >= admit.max_tails) return;
    const u64 place = static_cast<u64>(t) * a.cb;
    u32 len = 0, stream = kNone;
    rows.tag[t] = kNone;
    chunk_row_clear(rows, t, place);
    if (t < st.atails[a.ns]) {
        const u32 b = owner_of(static_cast<const u64*>(st.atails), a.ns, t);
        if (admit(b) && (st.flags[b] & kReopen)) {
            const Hop h = frame_hop(a.buf + a.buf_off[b], a.buf_len[b], st.cut[b]);
            if (h.kind == HOP_DATA && h.dec == st.d[b]) {                // (what the plan saw)
                rows.tag[t] = t;
                chunk_row_set(rows, t, h, a.buf_off[b] + st.cut[b], place);
                len = st.d[b] + st.fill[b];
                stream = b;
            }
        }
    }
    tl.in_off[t] = place;
    tl.coff[t] = fc_stage_off(t, stride);
    tl.len[t] = len;
    tl.stream[t] = stream;
}

// a tail that did not decode or verify: its status to its stream (one tail per stream)
__global__ __launch_bounds__(256) void k_fa_fail(u32 max_tails, ChunkRows rows, ApSlots tl, ApStreams st)
{
    const u32 t = blockIdx.x * 256u + threadIdx.x;
    if (t >= max_tails || rows.tag[t] == kNone) return;
    const i32 s = row_verdict(rows, t);
    if (s != SNP_OK) st.fail[tl.stream[t]] = s;
}

// One workgroup per tail slot, grid-stride: the first appended bytes behind the decoded tail.  The slot steers the whole workgroup.
__global__ __launch_bounds__(256) void k_fa_overlay(ApArgs a, ApStreams st, u32 max_tails, ApSlots tl, u8* __restrict__ raw)
{
    for (u32 t = blockIdx.x; t < max_tails; t += gridDim.x) {
        const u32 b = tl.stream[t];
        if (b == kNone) continue;
        team_copy(raw + tl.in_off[t] + st.d[b], a.src + a.src_off[b], st.fill[b], threadIdx.x, 256u);
    }
}

// One thread per fresh slot: its piece of src and where its compressed bytes are staged (behind the tail table's).
__global__ __launch_bounds__(256) void k_fa_fresh(ApArgs a, ApStreams st, Admit admit, ApSlots fr, u64 stride)
{
    const u32 c = blockIdx.x * 256u + threadIdx.x;
    if (c >= admit.max_slots) return;
    u64 in_off = 0;
    u32 len = 0, stream = kNone;
    if (c < st.aslots[a.ns]) {
        const u32 b = fc_owner(st.aslots, a.ns, c);
        if (admit(b)) {
            const FaPiece p = fa_piece(st.rest[b], st.fill[b], a.cb, c - st.aslots[b]);
            in_off = a.src_off[b] + p.off;
            len = p.len;
            stream = b;
        }
    }
    fr.in_off[c] = in_off;
    fr.coff[c] = fc_stage_off(admit.max_tails, stride) + fc_stage_off(c, stride);
    fr.len[c] = len;
    fr.stream[c] = stream;
}

__global__ __launch_bounds__(256) void k_fa_sizes(ApArgs a, ApStreams st, Admit admit, ApSlots tl, const u64* __restrict__ cscan, u64* __restrict__ new_len,
                                                 i32* __restrict__ status, u64* __restrict__ out_bound, u64* __restrict__ result)
{
    const u32 b = blockIdx.x * 256u + threadIdx.x;
    u64 grown = 0, ok = 0;
    if (b < a.ns) {
        u32 flags = st.flags[b];
        i32 s = static_cast<i32>(flags & 0xffu);
        const u64 n = a.buf_len[b];
        u64 len = n, bound = st.bound[b], rows = st.rows[b];
        if (flags & kAppend) {
            s = SNP_ERR_OUTPUT_TOO_SMALL;
            if (admit(b)) {
                if (st.fail[b] != SNP_OK) {
                    s = st.fail[b];
                    bound = n;
                } else {
                    u64 base = st.cut[b] + ((flags & kIdent) ? SNP_STREAM_HEADER_LEN : 0);
                    if (flags & kReopen) {
                        const u64 t = st.atails[b];
                        bool shrink;
                        base += SNP_CHUNK_HEADER_LEN + payload_of(tl.comp_len[t], tl.len[t], &shrink);
                    }
                    const u64 size = base + (cscan[st.aslots[b + 1]] - cscan[st.aslots[b]]);
                    if (size <= a.buf_cap[b]) {
                        s = SNP_OK;
                        len = size;
                        ok = 1;
                        grown = size - n;                                // (mod 2^64: a tail a foreign writer stored loosely may shrink)
                        flags |= kWritten;
                        rows += st.fresh[b];
                        st.base[b] = base;
                    }
                }
            }
        }
        status[b] = s;
        new_len[b] = len;
        if (out_bound) out_bound[b] = bound;
        st.flags[b] = flags;
        st.nrows[b] = rows;
    }
    grown = wave_sum(grown);
    ok = wave_sum(ok);
    if ((threadIdx.x & 63u) == 0 && ok) {
        atomic_add64(result + 1, grown);
        atomic_add64(result + 3, ok);
    }
}

// The shape of fc_group and fc_team (frame_chunked_device.h) over both tables: a workgroup takes `group` consecutive slots of one table (64 KiB of input), its teams of `team` threads take them
// in turn; units [0, tail_units) are the tail table's, the rest the fresh table's.  What steers a team is uniform over it; a chunk goes to its
// stream at the cut (a reopened tail), or behind it where the size scan puts it (a fresh chunk; the first one of an empty stream brings the identifier).
__global__ __launch_bounds__(256) void k_fa_emit(ApArgs a, ApStreams st, u32 max_tails, u32 max_slots, u32 group, u32 team, u64 tail_units, u64 units,
                                                ApSlots tl, ApSlots fr, const u64* __restrict__ cscan, const u8* __restrict__ raw,
                                                const u8* __restrict__ comp)
{
    const u32 t = threadIdx.x % team, teams = 256u / team;
    for (u64 g = blockIdx.x; g < units; g += gridDim.x) {
        const bool tails = g < tail_units;                              // (uniform over the workgroup)
        const ApSlots sl = tails ? tl : fr;
        const u64 n = tails ? max_tails : max_slots;
        const u64 c0 = (tails ? g : g - tail_units) * group;
        const u64 c1 = c0 + group < n ? c0 + group : n;
        for (u64 c = c0 + threadIdx.x / team; c < c1; c += teams) {
            const u32 b = sl.stream[c];
            if (b == kNone || !(st.flags[b] & kWritten)) continue;
            const u32 len = sl.len[c];
            bool shrink;
            const u32 pl = payload_of(sl.comp_len[c], len, &shrink);
            u8* const stream = a.buf + a.buf_off[b];
            u64 pos = st.cut[b];
            const u8* from = comp + sl.coff[c];
            if (tails) {
                if (!shrink) from = raw + sl.in_off[c];
            } else {
                const u64 first = st.aslots[b];
                pos = st.base[b] + (cscan[c] - cscan[first]);
                if (!shrink) from = a.src + sl.in_off[c];
                if (c == first && (st.flags[b] & kIdent) && t < SNP_STREAM_HEADER_LEN) stream[t] = k_fc_stream_id[t];   // EnsureStreamHeaderWritten  :148-157
            }
            chunk_header(stream + pos, t, shrink ? 0u : 1u, pl, sl.crc[c]);
            team_copy(stream + pos + SNP_CHUNK_HEADER_LEN, from, pl, t, team);
        }
    }
}

// One thread per row of the new index, grid-stride, and per stream its three words.  Row i of stream b = owner(nfirst, i): one of its old rows
// (f0 and the count are clamped to nentries: idx_first is untrusted), or fresh chunk j of a written stream.  Rows at or past `cap` do not exist.
__global__ __launch_bounds__(256) void k_fa_rows(ApArgs a, ApStreams st, const u64* __restrict__ cscan, u64 cap, u64* __restrict__ new_first,
                                                u64* __restrict__ new_start, u64* __restrict__ new_pos, u64* __restrict__ new_total,
                                                i32* __restrict__ new_tail)
{
    const u64 total = st.nfirst[a.ns] < cap ? st.nfirst[a.ns] : cap;
    const u64 most = total > static_cast<u64>(a.ns) + 1 ? total : static_cast<u64>(a.ns) + 1;
    for (u64 i = static_cast<u64>(blockIdx.x) * 256u + threadIdx.x; i < most; i += static_cast<u64>(gridDim.x) * 256u) {
        if (i <= a.ns) new_first[i] = st.nfirst[i] < cap ? st.nfirst[i] : cap;
        if (i < a.ns) {
            const bool written = (st.flags[i] & kWritten) != 0;
            new_total[i] = a.x.total[i] + (written ? a.src_len[i] : 0);
            new_tail[i] = written ? SNP_OK : a.x.tail[i];
        }
        if (i >= total) continue;
        const u32 b = owner_of(static_cast<const u64*>(st.nfirst), a.ns, i);
        const u64 j = i - st.nfirst[b];
        if (j < st.rows[b]) {
            new_start[i] = a.x.start[st.f0[b] + j];
            new_pos[i] = a.x.pos[st.f0[b] + j];
        } else {
            const u64 k = j - st.rows[b], first = st.aslots[b];
            new_start[i] = fa_row_start(a.x.total[b], st.fill[b], a.cb, k);
            new_pos[i] = st.base[b] + (cscan[first + k] - cscan[first]);
        }
    }
}

// workspace (every piece 256-byte aligned; nothing when there is no stream)
struct AppendWork {
    ApStreams st;
    ApSlots tl, fr;
    ChunkRows rows;
    u64 *part, *cscan;
    u8 *raw, *comp;
    u64 bytes;
};
AppendWork work_layout(void* base, u32 nstreams, u32 max_tails, u32 max_slots, u32 chunk_bytes)
{
    AppendWork w{};
    if (nstreams == 0 || chunk_bytes == 0 || chunk_bytes > SNP_BLOCK_SIZE) return w;
    const u64 ns = nstreams, T = max_tails, M = max_slots;
    WorkCarver k(base);
    w.part = k.take<u64>(scan_tiles_of(std::max(std::max(ns, T), M)));
    w.st.f0 = k.take<u64>(ns);
    w.st.rows = k.take<u64>(ns);
    w.st.cut = k.take<u64>(ns);
    w.st.rest = k.take<u64>(ns);
    w.st.bound = k.take<u64>(ns);
    w.st.base = k.take<u64>(ns);
    w.st.nrows = k.take<u64>(ns);
    w.st.tails = k.take<u64>(ns);
    w.st.fresh = k.take<u64>(ns);
    w.st.atails = k.take<u64>(ns + 1);
    w.st.aslots = k.take<u64>(ns + 1);
    w.st.nfirst = k.take<u64>(ns + 1);
    w.st.flags = k.take<u32>(ns);
    w.st.d = k.take<u32>(ns);
    w.st.fill = k.take<u32>(ns);
    w.st.fail = k.take<i32>(ns);
    w.tl = carve_rw_owned_slots(k, T);
    w.fr = carve_rw_owned_slots(k, M);
    w.rows = carve_chunk_rows(k, T);
    w.cscan = k.take<u64>(M + 1);
    // raw staging: tail slot t at t * chunk_bytes (+ slack for the compressor's vector loads).  Compressed staging: the tail slots, then the fresh
    // slots, at a stride of snp_comp_stride(chunk_bytes) (fc_stage_off); the appended bytes themselves are never staged.
    w.raw = k.take<u8>(T * chunk_bytes + 256);
    w.comp = k.take<u8>((T + M) * snp_comp_stride(chunk_bytes));
    w.bytes = k.bytes();
    return w;
}

}  // namespace

extern "C" {

uint64_t snp_frame_append_indexed_workspace(uint32_t nstreams, uint32_t max_tails, uint32_t max_slots, uint32_t chunk_bytes)
{
    return work_layout(nullptr, nstreams, max_tails, max_slots, chunk_bytes).bytes;
}

snp_status snp_frame_append_indexed_batch(snp_ctx* c, uint8_t* buf, const uint64_t* buf_off, const uint64_t* buf_len, const uint64_t* buf_cap,
                                          uint32_t nstreams, const uint64_t* idx_first, const uint64_t* idx_start, const uint64_t* idx_pos,
                                          const uint64_t* idx_total, const int32_t* idx_tail, uint64_t nentries, const uint8_t* src,
                                          const uint64_t* src_off, const uint64_t* src_len, uint32_t chunk_bytes, uint32_t max_tails,
                                          uint32_t max_slots, uint64_t* new_len, int32_t* status, uint64_t* new_first, uint64_t* new_start,
                                          uint64_t* new_pos, uint64_t* new_total, int32_t* new_tail, uint64_t* out_bound, void* d_work,
                                          uint64_t* d_result)
{
    const u64 cap = nentries + max_slots;                               // rows the new start / pos arrays hold
    if (!c || !d_result || chunk_bytes == 0 || chunk_bytes > SNP_BLOCK_SIZE ||
        (nstreams && (!buf || !buf_off || !buf_len || !buf_cap || !idx_first || !idx_total || !idx_tail || !src || !src_off || !src_len || !new_len ||
                      !status || !new_first || !new_total || !new_tail || !d_work)) ||
        (nstreams && nentries && (!idx_start || !idx_pos)) || (nstreams && cap && (!new_start || !new_pos)))
        return SNP_ERR_BAD_ARG;
    DevGuard dg(c);
    if (!dg.ok) return SNP_ERR_DEVICE;
    hipStream_t s = c->stream;
    bool ok = c->check(snp_zero_words_async(reinterpret_cast<u32*>(d_result), 2 * 4, s), "frame append result");
    if (nstreams == 0) return ok ? SNP_OK : SNP_ERR_DEVICE;
    const AppendWork w = work_layout(d_work, nstreams, max_tails, max_slots, chunk_bytes);
    const u32 ns = nstreams, T = max_tails, M = max_slots, cb = chunk_bytes, sg = groups_of(ns), tg = groups_of(T), mg = groups_of(M);
    const u64 stride = snp_comp_stride(cb);
    const ApArgs a{buf, buf_off, buf_len, buf_cap, ns, FrameIndex{idx_first, idx_start, idx_pos, idx_total, idx_tail, nentries}, src, src_off, src_len, cb};
    const Admit admit{w.st.flags, w.st.atails, w.st.aslots, T, M};
    // the plan of every stream; admission in stream order (d_result[2] = tails, [0] = fresh slots of the streams that passed)
    hipLaunchKernelGGL(k_fa_plan, dim3(sg), dim3(256), 0, s, a, w.st);
    ok = ok && c->check(hipGetLastError(), "frame append plan") &&
         c->check(launch_scan(ScanWords{w.st.tails}, ns, w.part, w.st.atails, d_result + 2, s), "frame append tail scan") &&
         c->check(launch_scan(ScanWords{w.st.fresh}, ns, w.part, w.st.aslots, d_result, s), "frame append slot scan");
    if (ok && T) {
        // the reopened tails decoded and verified whole into the raw staging, the fill bytes behind them; CompressBlock and the masked CRC-32C of each
        hipLaunchKernelGGL(k_fa_tails, dim3(tg), dim3(256), 0, s, a, w.st, admit, w.tl, w.rows, stride);
        ok = c->check(hipGetLastError(), "frame append tails") && c->decode_chunks(buf, w.rows, T, w.raw);
        if (ok) {
            hipLaunchKernelGGL(k_fa_fail, dim3(tg), dim3(256), 0, s, T, w.rows, w.tl, w.st);
            hipLaunchKernelGGL(k_fa_overlay, dim3(std::min(T, kOverlayGroups)), dim3(256), 0, s, a, w.st, T, w.tl, w.raw);
            ok = c->check(hipGetLastError(), "frame append overlay") && compress_slots(c, w.raw, w.tl.rw(), T, w.comp, "frame append tail");
        }
    }
    if (ok && M) {
        hipLaunchKernelGGL(k_fa_fresh, dim3(mg), dim3(256), 0, s, a, w.st, admit, w.fr, stride);
        ok = c->check(hipGetLastError(), "frame append fresh");
    }
    // the fresh chunks re-encoded straight from src (no copy of the appended bytes) and their framed sizes; every stream's verdict, the rows of the
    // new index
    ok = ok && reencode_slots(c, src, w.fr.rw(), M, w.comp, w.part, w.cscan, "frame append");
    if (ok) {
        hipLaunchKernelGGL(k_fa_sizes, dim3(sg), dim3(256), 0, s, a, w.st, admit, w.tl, w.cscan, new_len, status, out_bound, d_result);
        ok = c->check(hipGetLastError(), "frame append sizes") &&
             c->check(launch_scan(ScanWords{w.st.nrows}, ns, w.part, w.st.nfirst, nullptr, s), "frame append row scan");
    }
    if (ok) {
        const u32 group = fc_group(cb);
        const u64 tail_units = (static_cast<u64>(T) + group - 1) / group, units = tail_units + (static_cast<u64>(M) + group - 1) / group;
        if (units)
            hipLaunchKernelGGL(k_fa_emit, dim3(static_cast<u32>(std::min<u64>(units, kEmitGroups))), dim3(256), 0, s, a, w.st, T, M, group, fc_team(group),
                               tail_units, units, w.tl, w.fr, w.cscan, w.raw, w.comp);
        const u64 most = std::max<u64>(cap, static_cast<u64>(ns) + 1);
        hipLaunchKernelGGL(k_fa_rows, dim3(static_cast<u32>(std::min<u64>((most + 255) / 256, kRowGroups))), dim3(256), 0, s, a, w.st, w.cscan, cap,
                           new_first, new_start, new_pos, new_total, new_tail);
        ok = c->check(hipGetLastError(), "frame append emit");
    }
    return ok ? SNP_OK : SNP_ERR_DEVICE;
}

}  // extern "C"

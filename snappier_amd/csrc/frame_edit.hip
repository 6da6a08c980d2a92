// frame_edit.hip -- snp_frame_edit_indexed_batch: a sorted EDIT SCRIPT per stream of framed streams kept with their chunk index -- edit e replaces
// decoded bytes [off, off + del) of the OLD stream by ins source bytes -- answered out of place by new streams in which every touched chunk is
// decoded once, every rewritten region compressed once and every other kept byte copied once, with the new index.  fs_plan
// (frame_splice_device.h) plans an edit as the splice plans its one, frame_edit_device.h links the edits that own the same row into groups,
// frame_rewrite_device.h re-encodes and emits the slots.  Built into libsnappier_hip_frame_edit.so (C-ABI: include/snappier_hip_frame_edit.h),
// linked against libsnappier_hip.so.  DESIGN.md 4.25.
//
//   lists     one thread per stream: does its edit list run backwards; scan -> every stream from the first such one on is refused
//   owners    one thread per edit: its stream, is it named; scan -> the NAMED edits of the call, compacted in list order (k below)
//   plan      one thread per edit (fs_plan): the owned rows, the edges, the hole, |H|, |T|
//   scans     inserted bytes (low and high halves: exact), ins - del
//   link      one thread per named edit: linked to the one before / after it, its verdict (ed_status), is it a group's first, |H| + |G| or |T|,
//             the decoded bytes of the edge rows it enters into the table (a shared row is entered once, by the first edit that touches it)
//   scans     refused edits, group heads, those lengths, those bytes
//   groups    one thread per group: |R|, its pieces, its staging bytes, its hole, its owned rows; scans of the four
//   streams   one thread per stream: the verdict so far (the first refused edit's), what it asks of each bound, the size bound
//   scans     pieces and staging bytes of the streams that passed -> admission in stream order; d_result[0], [2]
//   edges     one thread per named edit: its two rows of the edge table; decode: snp_ctx::decode_chunks, ONCE; fail: the first failing row of a stream
//   assemble  a workgroup per 64 KiB of staging, grid-stride: of every region that meets it, the parts -- H, source bytes, G, ..., T -- found
//             by a search over the running lengths, a wavefront per edit
//   slots     one thread per table slot: its stream, its group, its piece of the group's region
//   compress  snp_ctx::launch_compress and snp_launch_crc32c over every slot -- once each; scan: 8 + payload per slot
//   sizes     one thread per stream: size against out_cap, status, out_len, out_bound, d_result[1] and [3]; its emit units; the rows of its new index
//   emit      one workgroup per unit, grid-stride: 64 KiB of an old stream's kept bytes -- several copies where the unit meets holes, found by
//             a search over the stream's holes -- or fc_group(chunk_bytes) consecutive new chunks
//   rows      one thread per new row: an old row moved by what the groups before it did, or a new chunk's row
// Nothing here allocates, reads back or synchronises: the call is capturable like the other _batch entry points.
#include "capi_internal.h"
#include "frame_rewrite_device.h"
#include "frame_edit_device.h"
#include "../../include/snappier_hip_frame_edit.h"

namespace {

constexpr u32 kPass = 0x100u, kIdent = 0x200u, kWritten = 0x400u;   // stream flags above the status byte
constexpr u32 kLinkP = 0x100u;                                      // edit flag above the status byte: linked to the edit before

struct EdArgs {
    const u8* in;
    const u64 *in_off, *in_len;
    u32 ns;
    FrameIndex x;
    const u8* src;
    const u64 *ed_first, *ed_off, *ed_del, *ed_ins, *src_off;
    u32 ne;                                                 // edits of the call
    u32 cb;
};
// per edit of the call (own, named, nscan) and per NAMED edit, compacted (the rest)
struct EdEdits {
    u32* own;                                               // the stream of edit e (kNone: none)
    u64 *named, *nscan;                                     // 1: owned and named; its scan (ne + 1): nscan[ne] = the named edits
    u64 *eidx, *r0, *r1, *p0, *p1, *tpos;
    u64 *vlo, *vhi, *vdl;                                   // ins: low half, high half; ins - del
    u64 *bad, *gh, *xtra, *se;                              // refused; a group's first; |H| + (|G| or |T|); edge bytes it enters
    u64 *ilo, *ihi, *dsc, *bsc, *gsc, *xsc, *ssc;           // scans (ne + 1)
    u32 *stream, *hl, *tl, *e0, *e1;
    u32* pstat;                                             // fs_plan's status
    u32* flags;                                             // the edit's verdict, kLinkP
};
// per group
struct EdGroups {
    u64* head;                                              // (ne + 1) its first edit; head[groups] = the named edits
    u64 *pieces, *stage, *hole, *owned;
    u64 *psc, *tsc, *hsc, *osc;                             // scans (ne + 1)
};
// per stream
struct EdStreams {
    u64 *csrbad, *csc;                                      // its list runs backwards; scan (ns + 1)
    u64 *f0, *rows, *c0, *c1, *bound;
    u64 *pieces, *stage;                                    // what the stream asks of each bound (0 unless it passed and is named)
    u64 *new_bytes, *nrows, *units;
    u64 *aslots, *abytes, *nfirst, *gfirst;                 // scans (ns + 1)
    u64* fail;                                              // (table row << 8 | status) of the first edge row that did not decode or verify
    u32* flags;
};
using EdSlots = RwOwnedSlots;

struct ScanLive {                                           // a table of which only the first *live entries exist
    const u64* __restrict__ src;
    const u64* __restrict__ live;
    __device__ __forceinline__ u64 operator()(u64 i) const { return i < *live ? src[i] : 0; }
};

struct Admit {
    const u32* flags;
    const u64* __restrict__ aslots;
    const u64* __restrict__ abytes;
    u32 max_slots;
    u64 stage_cap;
    __device__ __forceinline__ bool operator()(u32 b) const { return (flags[b] & kPass) && aslots[b + 1] <= max_slots && abytes[b + 1] <= stage_cap; }
};

// the region bytes of a stream's edits before edit k, modulo 2^64 (exact in differences over an admitted stream)
__device__ __forceinline__ u64 reg_off(const EdEdits& ed, u64 k) { return (ed.ihi[k] << 32) + ed.ilo[k] + ed.xsc[k]; }
// the groups [g0, g1) and the slots [a0, a1) of a stream that passed
struct EdSpan { u64 c0, c1, g0, g1, a0; };
__device__ __forceinline__ EdSpan span_of(const EdEdits& ed, const EdStreams& st, u32 b)
{
    const u64 c0 = st.c0[b], c1 = st.c1[b];
    return EdSpan{c0, c1, ed.gsc[c0], ed.gsc[c1], st.aslots[b]};
}
// where group g's hole starts among the stream's kept bytes; the first slot of group g
__device__ __forceinline__ u64 kept_at(const EdEdits& ed, const EdGroups& gr, const EdSpan& s, u64 g) { return ed.p0[gr.head[g]] - (gr.hsc[g] - gr.hsc[s.g0]); }
__device__ __forceinline__ u64 slot_at(const EdGroups& gr, const EdSpan& s, u64 g) { return s.a0 + (gr.psc[g] - gr.psc[s.g0]); }
// the group of [g0, g1) that holds piece j of the stream (j < its pieces)
__device__ __forceinline__ u64 group_of_piece(const EdGroups& gr, const EdSpan& s, u64 j)
{
    return ix_first_where(s.g0, s.g1, [&](u64 g) { return gr.psc[g + 1] - gr.psc[s.g0] > j; });
}

__global__ __launch_bounds__(256) void k_fe_lists(EdArgs a, EdStreams st)
{
    const u32 b = blockIdx.x * 256u + threadIdx.x;
    if (b >= a.ns) return;
    u64 e0, e1;
    st.csrbad[b] = fe_csr(a.ed_first, a.ne, b, &e0, &e1) ? 0 : 1;
}

// One thread per edit: the stream whose list holds it -- the last stream, among those before the first list that runs backwards, whose list starts
// at or before it -- and whether it is named.
__global__ __launch_bounds__(256) void k_fe_owners(EdArgs a, EdStreams st, EdEdits ed, i32* __restrict__ ed_status)
{
    const u32 e = blockIdx.x * 256u + threadIdx.x;
    if (e >= a.ne) return;
    const u32 b = owner_of([&](u32 m) { return st.csc[m] ? ~0ull : (a.ed_first[m] < a.ne ? a.ed_first[m] : a.ne); }, a.ns, e);
    u64 e0, e1;
    const bool mine = st.csc[b + 1] == 0 && fe_csr(a.ed_first, a.ne, b, &e0, &e1) && e0 <= e && e < e1;
    ed.own[e] = mine ? b : kNone;
    ed.named[e] = mine && fe_named(a.ed_del[e], a.ed_ins[e]) ? 1 : 0;
    ed_status[e] = SNP_OK;
}

__global__ __launch_bounds__(256) void k_fe_plan(EdArgs a, EdEdits ed)
{
    const u32 e = blockIdx.x * 256u + threadIdx.x;
    if (e >= a.ne || !ed.named[e]) return;
    const u64 k = ed.nscan[e];
    const u32 b = ed.own[e];
    const u8* const s = a.in + a.in_off[b];
    const u64 n = a.in_len[b], ins = a.ed_ins[e];
    const FsPlan p = fs_plan(a.x, b, n, a.ed_off[e], a.ed_del[e], ins, a.cb, [&](u64 pos) { return frame_hop(s, n, pos); });
    ed.eidx[k] = e;
    ed.stream[k] = b;
    ed.r0[k] = p.r0;
    ed.r1[k] = p.r1;
    ed.p0[k] = p.p0;
    ed.p1[k] = p.p1;
    ed.tpos[k] = p.tpos;
    ed.hl[k] = p.hl;
    ed.tl[k] = p.tl;
    ed.e0[k] = p.e0;
    ed.e1[k] = p.e1;
    ed.pstat[k] = static_cast<u32>(p.status) & 0xffu;
    ed.vlo[k] = ins & 0xffffffffu;
    ed.vhi[k] = ins >> 32;
    ed.vdl[k] = ins - a.ed_del[e];
}

__device__ __forceinline__ FeEdit edit_at(const EdArgs& a, const EdEdits& ed, u64 k)
{
    const u64 e = ed.eidx[k];
    return FeEdit{static_cast<i32>(ed.pstat[k]), a.ed_off[e], a.ed_del[e], ed.r0[k], ed.r1[k], ed.p0[k], ed.p1[k]};
}

// One thread per named edit.
__global__ __launch_bounds__(256) void k_fe_link(EdArgs a, EdEdits ed, i32* __restrict__ ed_status)
{
    const u64 k = blockIdx.x * 256u + threadIdx.x;
    if (k >= ed.nscan[a.ne]) return;
    const u32 b = ed.stream[k];
    u64 e0, e1;
    fe_csr(a.ed_first, a.ne, b, &e0, &e1);
    const u64 c0 = ed.nscan[e0], c1 = ed.nscan[e1];
    const FeEdit me = edit_at(a, ed, k);
    bool lp = false, ln = false;
    FeEdit prev{}, next{};
    if (k > c0) {
        prev = edit_at(a, ed, k - 1);
        lp = fe_linked(prev, me);
    }
    if (k + 1 < c1) {
        next = edit_at(a, ed, k + 1);
        ln = fe_linked(me, next);
    }
    const u64 ins_mod = ((ed.ihi[k + 1] - ed.ihi[c0]) << 32) + (ed.ilo[k + 1] - ed.ilo[c0]);
    const i32 v = fe_verdict(me, k > c0 ? &prev : nullptr, a.x.total[b], ed.ihi[k + 1] - ed.ihi[c0], ed.ilo[k + 1] - ed.ilo[c0],
                             ins_mod - (ed.dsc[k + 1] - ed.dsc[c0]));
    ed_status[ed.eidx[k]] = v;
    ed.bad[k] = v != SNP_OK;
    ed.gh[k] = lp ? 0 : 1;
    ed.xtra[k] = (lp ? 0 : ed.hl[k]) + (ln ? next.lo - (me.lo + me.del) : ed.tl[k]);
    ed.se[k] = (lp ? 0 : ed.e0[k]) + static_cast<u64>(ed.e1[k]);
    ed.flags[k] = (static_cast<u32>(v) & 0xffu) | (lp ? kLinkP : 0u);
}

__global__ __launch_bounds__(256) void k_fe_heads(EdArgs a, EdEdits ed, EdGroups gr)
{
    const u64 k = blockIdx.x * 256u + threadIdx.x, live = ed.nscan[a.ne];
    if (k == 0) gr.head[ed.gsc[a.ne]] = live;
    if (k < live && ed.gh[k]) gr.head[ed.gsc[k]] = k;
}

__global__ __launch_bounds__(256) void k_fe_groups(EdArgs a, EdEdits ed, EdGroups gr)
{
    const u64 g = blockIdx.x * 256u + threadIdx.x;
    if (g >= ed.gsc[a.ne]) return;
    const u64 f = gr.head[g], l = gr.head[g + 1];                       // its edits [f, l)
    u64 region;
    const bool fits = fe_wide(ed.ihi[l] - ed.ihi[f], ed.ilo[l] - ed.ilo[f], ed.xsc[l] - ed.xsc[f], &region);
    gr.pieces[g] = fe_count_pieces(fits, region, a.cb);
    gr.stage[g] = fe_count_stage(fits, region, ed.ssc[l] - ed.ssc[f]);
    gr.hole[g] = ed.p1[l - 1] - ed.p0[f];
    gr.owned[g] = ed.r1[l - 1] - ed.r0[f];
}

__global__ __launch_bounds__(256) void k_fe_streams(EdArgs a, EdEdits ed, EdGroups gr, EdStreams st)
{
    const u32 b = blockIdx.x * 256u + threadIdx.x;
    if (b >= a.ns) return;
    u64 e0, e1, c0 = 0, c1 = 0, pieces = 0, stage = 0, bound = 0;
    i32 status = SNP_OK;
    bool pass = false;
    if (st.csc[b + 1] != 0) {
        status = SNP_ERR_BAD_ARG;
    } else {
        fe_csr(a.ed_first, a.ne, b, &e0, &e1);
        c0 = ed.nscan[e0];
        c1 = ed.nscan[e1];
        if (c1 > c0) {                                                  // named
            if (ed.bsc[c1] != ed.bsc[c0]) {                             // the first refused edit's verdict
                const u64 k = ix_first_where(c0, c1, [&](u64 i) { return ed.bsc[i + 1] != ed.bsc[c0]; });
                status = static_cast<i32>(ed.flags[k < c1 ? k : c0] & 0xffu);
            } else {
                pass = true;
                const u64 g0 = ed.gsc[c0], g1 = ed.gsc[c1], n = a.in_len[b];
                const u64 asked = gr.psc[g1] - gr.psc[g0], staged = gr.tsc[g1] - gr.tsc[g0];
                pieces = asked < kFsMaxPieces ? asked : kFsMaxPieces;
                stage = staged < kFsMaxStage ? staged : kFsMaxStage;
                bound = n - (gr.hsc[g1] - gr.hsc[g0]) + SNP_CHUNK_HEADER_LEN * asked + (reg_off(ed, c1) - reg_off(ed, c0)) + (n == 0 ? SNP_STREAM_HEADER_LEN : 0);
            }
        }
    }
    fs_rows(a.x, b, &st.f0[b], &st.rows[b]);
    st.c0[b] = c0;
    st.c1[b] = c1;
    st.pieces[b] = pieces;
    st.stage[b] = stage;
    st.bound[b] = bound;
    st.new_bytes[b] = 0;
    st.fail[b] = kNoFail;
    st.flags[b] = (static_cast<u32>(status) & 0xffu) | (pass ? kPass : 0u) | (pass && a.in_len[b] == 0 ? kIdent : 0u);
}

// where the edge rows edit k enters are decoded to: behind those of the stream's edits before it
__device__ __forceinline__ u64 edge_at(const EdEdits& ed, const EdStreams& st, u32 b, u64 k) { return st.abytes[b] + (ed.ssc[k] - ed.ssc[st.c0[b]]); }

// One thread per row pair of the edge table: rows 2 k and 2 k + 1 are named edit k's -- its head row unless it is linked to the edit before (that
// one, or one before it, entered the row), its tail row when it is another row than its head row.
__global__ __launch_bounds__(256) void k_fe_edges(EdArgs a, EdEdits ed, EdStreams st, Admit admit, ChunkRows rows)
{
    const u64 k = blockIdx.x * 256u + threadIdx.x;
    if (k >= a.ne) return;
    const u64 t0 = 2 * k, t1 = t0 + 1;
    rows.tag[t0] = rows.tag[t1] = kNone;
    chunk_row_clear(rows, t0, 0);
    chunk_row_clear(rows, t1, 0);
    if (k >= ed.nscan[a.ne]) return;
    const u32 b = ed.stream[k];
    if (!admit(b)) return;
    const u8* const s = a.in + a.in_off[b];
    const u64 n = a.in_len[b], place = edge_at(ed, st, b, k);
    const u32 e0 = (ed.flags[k] & kLinkP) ? 0 : ed.e0[k], e1 = ed.e1[k];
    if (e0) {
        const Hop h = frame_hop(s, n, ed.p0[k]);
        if (h.kind == HOP_DATA && h.dec == e0) {                        // (what the plan saw)
            rows.tag[t0] = static_cast<u32>(t0);
            chunk_row_set(rows, t0, h, a.in_off[b] + ed.p0[k], place);
        }
    }
    if (e1) {
        const Hop h = frame_hop(s, n, ed.tpos[k]);
        if (h.kind == HOP_DATA && h.dec == e1) {
            rows.tag[t1] = static_cast<u32>(t1);
            chunk_row_set(rows, t1, h, a.in_off[b] + ed.tpos[k], place + e0);
        }
    }
}

// an edge row that did not decode or verify: the first one of its stream in table order
__global__ __launch_bounds__(256) void k_fe_fail(EdArgs a, EdEdits ed, EdStreams st, ChunkRows rows)
{
    const u64 k = blockIdx.x * 256u + threadIdx.x;
    if (k >= ed.nscan[a.ne]) return;
    for (u64 t = 2 * k; t < 2 * k + 2; ++t) {
        if (rows.tag[t] == kNone) continue;
        const i32 s = row_verdict(rows, t);
        if (s != SNP_OK) atomic_min64(st.fail + ed.stream[k], (t << 8) | (static_cast<u32>(s) & 0xffu));
    }
}

// where the decoded row that holds named edit k's tail lies in staging, and its decoded bytes: its own tail row; else its head row, which it
// entered itself or -- linked -- the first edit of its group whose last owned row it is
__device__ inline u64 tail_row_at(const EdEdits& ed, const EdGroups& gr, const EdStreams& st, u32 b, u64 k, u32* dec)
{
    u64 w = k;
    if (!ed.e1[k] && (ed.flags[k] & kLinkP)) {
        const u64 row = ed.r0[k];
        w = ix_first_where(gr.head[ed.gsc[k + 1] - 1], k, [&](u64 i) { return ed.r1[i] - 1 >= row; });
    }
    const u32 h = (ed.flags[w] & kLinkP) ? 0 : ed.e0[w];
    *dec = ed.e1[w] ? ed.e1[w] : h;
    return edge_at(ed, st, b, w) + (ed.e1[w] ? h : 0);
}

// the part [u0, u1) of a stream's regions that lies in [s0, s0 + len): from `from` (the part's first byte) to dst (the regions' first byte)
__device__ __forceinline__ void part_copy(u8* dst, const u8* from, u64 s0, u64 len, u64 u0, u64 u1, u32 lane)
{
    const u64 a = u0 > s0 ? u0 : s0, e = u1 < s0 + len ? u1 : s0 + len;
    if (len && a < e) team_copy(dst + a, from + (a - s0), static_cast<u32>(e - a), lane, 64u);      // (e - a <= kUnit)
}

// A workgroup per 64 KiB of staging, grid-stride.  The regions of an admitted stream lie behind its decoded edge rows, group by group, each
// R = H || ins || G || ins || ... || T.  Of every stream that meets the unit, the edits whose parts meet it are found by a search over the
// running lengths; a wavefront takes an edit's parts at a time.
__global__ __launch_bounds__(256) void k_fe_assemble(EdArgs a, EdEdits ed, EdGroups gr, EdStreams st, Admit admit, u8* __restrict__ stage)
{
    const u32 lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const u64 all = st.abytes[a.ns] < admit.stage_cap ? st.abytes[a.ns] : admit.stage_cap;
    for (u64 u0 = blockIdx.x * kUnit; u0 < all; u0 += gridDim.x * kUnit) {
        const u64 u1 = u0 + kUnit;
        for (u32 b = owner_of(static_cast<const u64*>(st.abytes), a.ns, u0); b < a.ns && st.abytes[b] < u1; ++b) {
            if (!admit(b) || st.fail[b] != kNoFail) continue;
            const u64 c0 = st.c0[b], c1 = st.c1[b], base = st.abytes[b] + (ed.ssc[c1] - ed.ssc[c0]), end = st.abytes[b + 1];
            if (base >= u1 || end <= u0 || base >= end) continue;
            const u64 q0 = (u0 > base ? u0 : base) - base, q1 = (u1 < end ? u1 : end) - base, r0 = reg_off(ed, c0);
            u8* const dst = stage + base;
            const u64 first = ix_first_where(c0, c1, [&](u64 i) { return reg_off(ed, i + 1) - r0 > q0; });
            for (u64 k = first + wave; k < c1 && reg_off(ed, k) - r0 < q1; k += 4) {
                const u64 e = ed.eidx[k], ins = a.ed_ins[e];
                const u32 f = ed.flags[k], hl = (f & kLinkP) ? 0 : ed.hl[k];
                u64 at = reg_off(ed, k) - r0;
                if (hl) part_copy(dst, stage + edge_at(ed, st, b, k), at, hl, q0, q1, lane);        // (a group's first edit entered its head row itself)
                at += hl;
                part_copy(dst, a.src + a.src_off[e], at, ins, q0, q1, lane);
                at += ins;
                const u64 rest = reg_off(ed, k + 1) - r0 - at;                                      // |G| or |T|
                if (rest) {
                    u32 dec;
                    const u64 row = tail_row_at(ed, gr, st, b, k, &dec);
                    part_copy(dst, stage + row + (dec - ed.tl[k]), at, rest, q0, q1, lane);
                }
            }
        }
    }
}

// One thread per table slot: its piece of its group's region in staging and where its compressed bytes are staged.
__global__ __launch_bounds__(256) void k_fe_slots(EdArgs a, EdEdits ed, EdGroups gr, EdStreams st, Admit admit, EdSlots sl, u64 stride)
{
    const u32 c = blockIdx.x * 256u + threadIdx.x;
    if (c >= admit.max_slots) return;
    u64 in_off = 0;
    u32 len = 0, stream = kNone;
    if (c < st.aslots[a.ns]) {
        const u32 b = fc_owner(st.aslots, a.ns, c);
        if (admit(b) && st.fail[b] == kNoFail) {
            const EdSpan s = span_of(ed, st, b);
            const u64 j = c - s.a0, g = group_of_piece(gr, s, j), f = gr.head[g], l = gr.head[g + 1];
            const FsPiece p = fs_piece(reg_off(ed, l) - reg_off(ed, f), a.cb, j - (gr.psc[g] - gr.psc[s.g0]));
            in_off = st.abytes[b] + (ed.ssc[s.c1] - ed.ssc[s.c0]) + (reg_off(ed, f) - reg_off(ed, s.c0)) + p.off;
            len = p.len;
            stream = b;
        }
    }
    sl.in_off[c] = in_off;
    sl.coff[c] = fc_stage_off(c, stride);
    sl.len[c] = len;
    sl.stream[c] = stream;
}

__global__ __launch_bounds__(256) void k_fe_sizes(EdArgs a, EdEdits ed, EdGroups gr, EdStreams st, Admit admit, const u64* __restrict__ cscan, u32 group,
                                                 const u64* __restrict__ out_cap, u64* __restrict__ out_len, i32* __restrict__ status,
                                                 u64* __restrict__ out_bound, u64* __restrict__ result)
{
    const u32 b = blockIdx.x * 256u + threadIdx.x;
    u64 ok_len = 0, ok = 0;
    if (b < a.ns) {
        u32 flags = st.flags[b];
        i32 s = static_cast<i32>(flags & 0xffu);
        u64 bound = st.bound[b], rows = st.rows[b], units = 0;
        if (flags & kPass) {
            s = SNP_ERR_OUTPUT_TOO_SMALL;
            if (admit(b)) {
                if (st.fail[b] != kNoFail) {
                    s = static_cast<i32>(st.fail[b] & 0xffu);
                    bound = 0;
                } else {
                    const EdSpan sp = span_of(ed, st, b);
                    const u64 fresh = ((flags & kIdent) ? SNP_STREAM_HEADER_LEN : 0) + (cscan[st.aslots[b + 1]] - cscan[sp.a0]);
                    const u64 kept = a.in_len[b] - (gr.hsc[sp.g1] - gr.hsc[sp.g0]), size = kept + fresh;
                    if (size <= out_cap[b]) {
                        s = SNP_OK;
                        ok_len = size;
                        ok = 1;
                        flags |= kWritten;
                        rows = rows - (gr.osc[sp.g1] - gr.osc[sp.g0]) + st.pieces[b];
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

// One workgroup per emit unit of a written stream.  The first units of a stream are 64 KiB each of its KEPT bytes -- the old stream without its
// holes: the kept bytes before group g's hole start at kept_at(g) among them, lie holes-before-g further on in the old stream and
// new-bytes-before-g further on in the new one, so a unit that meets holes is several copies.  The other units are `group` consecutive new chunks
// each, taken by teams of `team` threads in turn (emit_slot, frame_rewrite_device.h).  The unit steers the whole workgroup, a slot its whole team.
__global__ __launch_bounds__(256) void k_fe_emit(EdArgs a, EdEdits ed, EdGroups gr, EdStreams st, EdSlots sl, u32 group, u32 team,
                                                const u64* __restrict__ cscan, const u8* __restrict__ stage, const u8* __restrict__ comp,
                                                u8* __restrict__ out, const u64* __restrict__ out_off)
{
    const u32 tid = threadIdx.x, t = tid % team, teams = 256u / team;
    const u64 units = st.gfirst[a.ns];
    for (u64 w = blockIdx.x; w < units; w += gridDim.x) {
        const u32 b = owner_of(static_cast<const u64*>(st.gfirst), a.ns, w);
        const EdSpan s = span_of(ed, st, b);
        const u64 u = w - st.gfirst[b], kept = a.in_len[b] - (gr.hsc[s.g1] - gr.hsc[s.g0]);
        const u64 kept_units = (kept + kUnit - 1) / kUnit, ident = (st.flags[b] & kIdent) ? SNP_STREAM_HEADER_LEN : 0;
        const u8* const old = a.in + a.in_off[b];
        u8* const dst = out + out_off[b];
        if (u < kept_units) {
            u64 k0 = u * kUnit;
            const u64 k1 = k0 + kUnit < kept ? k0 + kUnit : kept;
            while (k0 < k1) {
                // [k0, e) lies behind the holes of the groups before g and before that of g
                const u64 g = ix_first_where(s.g0, s.g1, [&](u64 i) { return kept_at(ed, gr, s, i) > k0; });
                const u64 e = g < s.g1 && kept_at(ed, gr, s, g) < k1 ? kept_at(ed, gr, s, g) : k1;
                team_copy(dst + k0 + ident + (cscan[slot_at(gr, s, g)] - cscan[s.a0]), old + k0 + (gr.hsc[g] - gr.hsc[s.g0]), static_cast<u32>(e - k0), tid, 256u);
                k0 = e;
            }
            continue;
        }
        const u64 last = st.aslots[b + 1];
        const u64 c0 = s.a0 + (u - kept_units) * group, c1 = c0 + group < last ? c0 + group : last;
        for (u64 c = c0 + tid / team; c < c1; c += teams) {
            const u64 g = group_of_piece(gr, s, c - s.a0);
            const u64 pos = kept_at(ed, gr, s, g) + ident + (cscan[c] - cscan[s.a0]);
            if (c == s.a0 && ident && t < SNP_STREAM_HEADER_LEN) dst[t] = k_fc_stream_id[t];     // EnsureStreamHeaderWritten  :148-157
            emit_slot(dst + pos, sl.rw(), c, stage, comp, t, team);
        }
    }
}

// One thread per row of the new index, grid-stride, and per stream its three words.  Row i of stream b = owner(nfirst, i): of a stream that is
// not written, one of its old rows; of a written one, with rows_at(g) the row its group g's new chunks start at: an old row before the first
// hole, piece j of group g, or an old row behind group g's hole, moved by what the groups up to g did.  Rows at or past `cap` do not exist.
__global__ __launch_bounds__(256) void k_fe_rows(EdArgs a, EdEdits ed, EdGroups gr, EdStreams st, const u64* __restrict__ cscan, u64 cap,
                                                u64* __restrict__ new_first, u64* __restrict__ new_start, u64* __restrict__ new_pos,
                                                u64* __restrict__ new_total, i32* __restrict__ new_tail)
{
    const u64 total = st.nfirst[a.ns] < cap ? st.nfirst[a.ns] : cap;
    const u64 most = total > static_cast<u64>(a.ns) + 1 ? total : static_cast<u64>(a.ns) + 1;
    for (u64 i = static_cast<u64>(blockIdx.x) * 256u + threadIdx.x; i < most; i += static_cast<u64>(gridDim.x) * 256u) {
        if (i <= a.ns) new_first[i] = st.nfirst[i] < cap ? st.nfirst[i] : cap;
        if (i < a.ns) {
            const bool written = (st.flags[i] & kWritten) != 0;
            new_total[i] = written ? a.x.total[i] + (ed.dsc[st.c1[i]] - ed.dsc[st.c0[i]]) : a.x.total[i];
            new_tail[i] = written ? SNP_OK : a.x.tail[i];
        }
        if (i >= total) continue;
        const u32 b = owner_of(static_cast<const u64*>(st.nfirst), a.ns, i);
        const u64 j = i - st.nfirst[b], f0 = st.f0[b];
        if (!(st.flags[b] & kWritten)) {
            new_start[i] = a.x.start[f0 + j];
            new_pos[i] = a.x.pos[f0 + j];
            continue;
        }
        const EdSpan s = span_of(ed, st, b);
        const auto rows_at = [&](u64 g) { return (ed.r0[gr.head[g]] - f0) - (gr.osc[g] - gr.osc[s.g0]) + (gr.psc[g] - gr.psc[s.g0]); };
        if (j < rows_at(s.g0)) {
            new_start[i] = a.x.start[f0 + j];
            new_pos[i] = a.x.pos[f0 + j];
            continue;
        }
        const u64 g = ix_first_where(s.g0 + 1, s.g1, [&](u64 m) { return rows_at(m) > j; }) - 1;     // the last group with rows_at <= j
        const u64 k = j - rows_at(g), pieces = gr.psc[g + 1] - gr.psc[g], f = gr.head[g], l = gr.head[g + 1];
        const u64 ident = (st.flags[b] & kIdent) ? SNP_STREAM_HEADER_LEN : 0;
        if (k < pieces) {
            new_start[i] = fs_row_start(a.ed_off[ed.eidx[f]], ed.hl[f], a.cb, k) + (ed.dsc[f] - ed.dsc[s.c0]);
            new_pos[i] = kept_at(ed, gr, s, g) + ident + (cscan[slot_at(gr, s, g) + k] - cscan[s.a0]);
        } else {
            const u64 r = ed.r1[l - 1] + (k - pieces);
            new_start[i] = a.x.start[r] + (ed.dsc[l] - ed.dsc[s.c0]);
            new_pos[i] = a.x.pos[r] + ident + (cscan[slot_at(gr, s, g + 1)] - cscan[s.a0]) - (gr.hsc[g + 1] - gr.hsc[s.g0]);
        }
    }
}

// workspace (every piece 256-byte aligned; nothing when there is no stream)
struct EditWork {
    EdEdits ed;
    EdGroups gr;
    EdStreams st;
    EdSlots sl;
    ChunkRows rows;
    u64 *part, *cscan;
    u8 *stage, *comp;
    u64 bytes;
};
EditWork work_layout(void* base, u32 nstreams, u32 nedits, u32 max_slots, u64 stage_cap, u32 chunk_bytes)
{
    EditWork w{};
    if (nstreams == 0 || chunk_bytes == 0 || chunk_bytes > SNP_BLOCK_SIZE) return w;
    const u64 ns = nstreams, ne = nedits, M = max_slots;
    WorkCarver k(base);
    w.part = k.take<u64>(scan_tiles_of(std::max(std::max(ns, ne), M)));
    w.ed.own = k.take<u32>(ne);
    for (u64** p : {&w.ed.named, &w.ed.eidx, &w.ed.r0, &w.ed.r1, &w.ed.p0, &w.ed.p1, &w.ed.tpos, &w.ed.vlo, &w.ed.vhi, &w.ed.vdl, &w.ed.bad, &w.ed.gh,
                    &w.ed.xtra, &w.ed.se, &w.gr.pieces, &w.gr.stage, &w.gr.hole, &w.gr.owned})
        *p = k.take<u64>(ne);
    for (u64** p : {&w.ed.nscan, &w.ed.ilo, &w.ed.ihi, &w.ed.dsc, &w.ed.bsc, &w.ed.gsc, &w.ed.xsc, &w.ed.ssc, &w.gr.head, &w.gr.psc, &w.gr.tsc, &w.gr.hsc,
                    &w.gr.osc})
        *p = k.take<u64>(ne + 1);
    for (u32** p : {&w.ed.stream, &w.ed.hl, &w.ed.tl, &w.ed.e0, &w.ed.e1, &w.ed.pstat, &w.ed.flags}) *p = k.take<u32>(ne);
    for (u64** p : {&w.st.csrbad, &w.st.f0, &w.st.rows, &w.st.c0, &w.st.c1, &w.st.bound, &w.st.pieces, &w.st.stage, &w.st.new_bytes, &w.st.nrows,
                    &w.st.units, &w.st.fail})
        *p = k.take<u64>(ns);
    for (u64** p : {&w.st.csc, &w.st.aslots, &w.st.abytes, &w.st.nfirst, &w.st.gfirst}) *p = k.take<u64>(ns + 1);
    w.st.flags = k.take<u32>(ns);
    w.sl = carve_rw_owned_slots(k, M);
    w.rows = carve_chunk_rows(k, 2 * ne);
    w.cscan = k.take<u64>(M + 1);
    // staging: per admitted stream its decoded edge rows and its groups' regions behind them, the streams back to back (+ slack for the
    // compressor's vector loads).  Compressed staging: slot c at c * snp_comp_stride(chunk_bytes) (fc_stage_off).
    w.stage = k.take<u8>(stage_cap + 256);
    w.comp = k.take<u8>(M * snp_comp_stride(chunk_bytes));
    w.bytes = k.bytes();
    return w;
}

}  // namespace

extern "C" {

uint64_t snp_frame_edit_indexed_workspace(uint32_t nstreams, uint32_t nedits, uint32_t max_slots, uint64_t stage_cap, uint32_t chunk_bytes)
{
    return work_layout(nullptr, nstreams, nedits, max_slots, stage_cap, chunk_bytes).bytes;
}

snp_status snp_frame_edit_indexed_batch(snp_ctx* c, const uint8_t* in, const uint64_t* in_off, const uint64_t* in_len, uint32_t nstreams,
                                        const uint64_t* idx_first, const uint64_t* idx_start, const uint64_t* idx_pos, const uint64_t* idx_total,
                                        const int32_t* idx_tail, uint64_t nentries, const uint8_t* src, const uint64_t* ed_first,
                                        const uint64_t* ed_off, const uint64_t* ed_del, const uint64_t* ed_ins, const uint64_t* src_off,
                                        uint32_t nedits, uint32_t chunk_bytes, uint32_t max_slots, uint64_t stage_cap, uint8_t* out,
                                        const uint64_t* out_off, const uint64_t* out_cap, uint64_t* out_len, int32_t* status, int32_t* ed_status,
                                        uint64_t* new_first, uint64_t* new_start, uint64_t* new_pos, uint64_t* new_total, int32_t* new_tail,
                                        uint64_t* out_bound, void* d_work, uint64_t* d_result)
{
    const u64 cap = nentries + max_slots;                               // rows the new start / pos arrays hold
    if (!c || !d_result || chunk_bytes == 0 || chunk_bytes > SNP_BLOCK_SIZE || nstreams > 0x7fffffffu || nedits > 0x7fffffffu ||     // (2 nedits rows)
        (nstreams && (!in || !in_off || !in_len || !idx_first || !idx_total || !idx_tail || !src || !ed_first || !out || !out_off || !out_cap ||
                      !out_len || !status || !new_first || !new_total || !new_tail || !d_work)) ||
        (nstreams && nedits && (!ed_off || !ed_del || !ed_ins || !src_off || !ed_status)) || (nstreams && nentries && (!idx_start || !idx_pos)) ||
        (nstreams && cap && (!new_start || !new_pos)))
        return SNP_ERR_BAD_ARG;
    DevGuard dg(c);
    if (!dg.ok) return SNP_ERR_DEVICE;
    hipStream_t s = c->stream;
    bool ok = c->check(snp_zero_words_async(reinterpret_cast<u32*>(d_result), 2 * 4, s), "frame edit result");
    if (nstreams == 0) return ok ? SNP_OK : SNP_ERR_DEVICE;
    const EditWork w = work_layout(d_work, nstreams, nedits, max_slots, stage_cap, chunk_bytes);
    const u32 ns = nstreams, ne = nedits, M = max_slots, cb = chunk_bytes, sg = groups_of(ns), eg = std::max(groups_of(ne), 1u), mg = groups_of(M);
    const EdArgs a{in, in_off, in_len, ns, FrameIndex{idx_first, idx_start, idx_pos, idx_total, idx_tail, nentries}, src, ed_first, ed_off, ed_del,
                   ed_ins, src_off, ne, cb};
    const Admit admit{w.st.flags, w.st.aslots, w.st.abytes, M, stage_cap};
    const auto scan = [&](auto val, u32 n, u64* dst, u64* result, const char* step) {
        return ok && (ok = check_step(c, launch_scan(val, n, w.part, dst, result, s), "frame edit", step));
    };
    const u64* const live = w.ed.nscan + ne;                            // the named edits
    const u64* const groups = w.ed.gsc + ne;                            // the groups
    // the edit lists, the named edits of the call, the plan of each
    hipLaunchKernelGGL(k_fe_lists, dim3(sg), dim3(256), 0, s, a, w.st);
    scan(ScanWords{w.st.csrbad}, ns, w.st.csc, nullptr, "list scan");
    if (ok) hipLaunchKernelGGL(k_fe_owners, dim3(eg), dim3(256), 0, s, a, w.st, w.ed, ed_status);
    scan(ScanWords{w.ed.named}, ne, w.ed.nscan, nullptr, "named scan");
    if (ok) hipLaunchKernelGGL(k_fe_plan, dim3(eg), dim3(256), 0, s, a, w.ed);
    scan(ScanLive{w.ed.vlo, live}, ne, w.ed.ilo, nullptr, "insert scan");
    scan(ScanLive{w.ed.vhi, live}, ne, w.ed.ihi, nullptr, "insert scan");
    scan(ScanLive{w.ed.vdl, live}, ne, w.ed.dsc, nullptr, "delta scan");
    // the links, the verdicts, the groups
    if (ok) hipLaunchKernelGGL(k_fe_link, dim3(eg), dim3(256), 0, s, a, w.ed, ed_status);
    scan(ScanLive{w.ed.bad, live}, ne, w.ed.bsc, nullptr, "verdict scan");
    scan(ScanLive{w.ed.gh, live}, ne, w.ed.gsc, nullptr, "group scan");
    scan(ScanLive{w.ed.xtra, live}, ne, w.ed.xsc, nullptr, "region scan");
    scan(ScanLive{w.ed.se, live}, ne, w.ed.ssc, nullptr, "edge scan");
    if (ok) {
        hipLaunchKernelGGL(k_fe_heads, dim3(eg), dim3(256), 0, s, a, w.ed, w.gr);
        hipLaunchKernelGGL(k_fe_groups, dim3(eg), dim3(256), 0, s, a, w.ed, w.gr);
    }
    scan(ScanLive{w.gr.pieces, groups}, ne, w.gr.psc, nullptr, "piece scan");
    scan(ScanLive{w.gr.stage, groups}, ne, w.gr.tsc, nullptr, "staging scan");
    scan(ScanLive{w.gr.hole, groups}, ne, w.gr.hsc, nullptr, "hole scan");
    scan(ScanLive{w.gr.owned, groups}, ne, w.gr.osc, nullptr, "row scan");
    // every stream's verdict so far; admission in stream order (d_result[0] = slots, [2] = staging bytes of the streams that passed)
    if (ok) hipLaunchKernelGGL(k_fe_streams, dim3(sg), dim3(256), 0, s, a, w.ed, w.gr, w.st);
    scan(ScanWords{w.st.pieces}, ns, w.st.aslots, d_result, "slot scan");
    scan(ScanWords{w.st.stage}, ns, w.st.abytes, d_result + 2, "staging scan");
    ok = ok && c->check(hipGetLastError(), "frame edit plan");
    if (ok && stage_cap && ne) {
        // the edge rows decoded and verified whole into staging, ONCE each (a stream with an edge has staging bytes: none is admitted when
        // stage_cap is 0), then every group's region
        hipLaunchKernelGGL(k_fe_edges, dim3(eg), dim3(256), 0, s, a, w.ed, w.st, admit, w.rows);
        ok = c->check(hipGetLastError(), "frame edit edges") && c->decode_chunks(in, w.rows, 2 * ne, w.stage);
        if (ok) {
            hipLaunchKernelGGL(k_fe_fail, dim3(eg), dim3(256), 0, s, a, w.ed, w.st, w.rows);
            const u32 ag = static_cast<u32>(std::min<u64>((stage_cap + kUnit - 1) / kUnit, kEmitGroups));
            hipLaunchKernelGGL(k_fe_assemble, dim3(ag), dim3(256), 0, s, a, w.ed, w.gr, w.st, admit, w.stage);
            ok = c->check(hipGetLastError(), "frame edit assemble");
        }
    }
    if (ok && M) {
        hipLaunchKernelGGL(k_fe_slots, dim3(mg), dim3(256), 0, s, a, w.ed, w.gr, w.st, admit, w.sl, snp_comp_stride(cb));
        ok = c->check(hipGetLastError(), "frame edit slots");
        // every piece compressed from staging; without staging every slot is empty (reencode_slots in two steps: the scan below runs either way)
        if (ok && stage_cap) ok = compress_slots(c, w.stage, w.sl.rw(), M, w.comp, "frame edit");
    }
    // the framed sizes of the new chunks, every stream's verdict, its emit units and the rows of its new index
    scan(ScanFramed{w.sl.len, w.sl.comp_len}, M, w.cscan, nullptr, "size scan");
    if (ok) {
        const u32 group = fc_group(cb);
        hipLaunchKernelGGL(k_fe_sizes, dim3(sg), dim3(256), 0, s, a, w.ed, w.gr, w.st, admit, w.cscan, group, out_cap, out_len, status, out_bound, d_result);
        ok = c->check(hipGetLastError(), "frame edit sizes");
        scan(ScanWords{w.st.units}, ns, w.st.gfirst, nullptr, "unit scan");
        scan(ScanWords{w.st.nrows}, ns, w.st.nfirst, nullptr, "row scan");
        if (ok) {
            hipLaunchKernelGGL(k_fe_emit, dim3(kEmitGroups), dim3(256), 0, s, a, w.ed, w.gr, w.st, w.sl, group, fc_team(group), w.cscan, w.stage, w.comp,
                               out, out_off);
            const u64 most = std::max<u64>(cap, static_cast<u64>(ns) + 1);
            hipLaunchKernelGGL(k_fe_rows, dim3(static_cast<u32>(std::min<u64>((most + 255) / 256, kRowGroups))), dim3(256), 0, s, a, w.ed, w.gr, w.st,
                               w.cscan, cap, new_first, new_start, new_pos, new_total, new_tail);
            ok = c->check(hipGetLastError(), "frame edit emit");
        }
    }
    return ok ? SNP_OK : SNP_ERR_DEVICE;
}

}  // extern "C"

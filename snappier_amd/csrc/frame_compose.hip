// frame_compose.hip -- snp_frame_compose_indexed_batch: NEW framed streams made of windows ("segments") of old ones that are kept with their
// chunk index, out of place, with the new index.  A chunk that lies inside a segment is copied untouched; only the chunk a segment cuts at its
// head and the one it cuts at its tail are decoded, and the parts inside the segment compressed again, with no read-back between the two.
// frame_compose_device.h plans a segment and maps the rows of an output; the slot table, its re-encode, the piece table and the emit are
// frame_rewrite_device.h's, shared with the rechunk call.  Built into libsnappier_hip_frame_compose.so (C-ABI:
// include/snappier_hip_frame_compose.h), linked against libsnappier_hip.so.  DESIGN.md 4.21, 4.17.
//
//   plan      a workgroup per segment: cc_begin (the index alone), its rows walked by the threads (cc_add; joined over the workgroup), thread 0:
//             cc_finish -- the verdict, the edges, the pieces, the kept rows, what it asks of every bound
//   scans     over ALL segments: edges, pieces, staging bytes, new rows, decoded bytes, kept bytes, size bound, failed segments
//   join      one thread per output: its segments (clamped), the first failed one's status, its counts as differences of the scans
//   scans     edges, pieces, staging bytes, new rows over the outputs that passed -> admission in output order; d_result[2], [4]
//   clear     one thread per row of the decode table: an empty row
//   fill      one thread per row: its output (fc_owner), its segment (cc_seg_of over the edge scan), head or tail -> the edge's chunk, decoded to
//             the output's staging bytes + the edges before it
//   decode    snp_ctx::decode_chunks over the table into staging; fail: one thread per row, a failing row -> its output (the first in order)
//   slots     one thread per table slot: its output, its segment (over the piece scan), cc_piece -> where the piece lies in staging
//   re-encode reencode_slots: snp_ctx::launch_compress and snp_launch_crc32c over every slot -- once each, from staging; the scan of 8 + payload
//             per slot
//   sizes     one thread per output: size against out_cap, status, out_len, out_bound, d_result[0], [1], [3], [5]; its emit units; its new rows;
//             the identifier of an output without chunks
//   scans     emit units, rows of the new index
//   rows      one thread per new row: its output, its segment (over the row scan), cc_row -- an old row (its chunk's place in `in` and size)
//             or a piece (its slot and framed size); per output: new_first, new_total, new_tail
//   scan      the chunk sizes of the new rows -> where each chunk lies
//   emit      k_rw_emit: one 256-thread workgroup per unit, grid-stride: fc_group(chunk_bytes) consecutive new chunks of a written output, a
//             team each: a kept chunk copied from `in`, or header + payload from staging; new_pos of the row
// Nothing here allocates, reads back or synchronises: the call is capturable like the other _batch entry points.
#include "capi_internal.h"
#include "frame_rewrite_device.h"
#include "frame_compose_device.h"
#include "../../include/snappier_hip_frame_compose.h"

namespace {

constexpr u32 kPass = 0x100u, kWritten = 0x200u;                    // output flags above the status byte
constexpr u32 kHead = 0x100u, kTail = 0x200u;                       // segment flags above the status byte

struct CpArgs {
    const u8* in;
    const u64 *in_off, *in_len;
    u32 ns;
    FrameIndex x;
    const u64* seg_first;
    const u32* seg_stream;
    const u64 *seg_off, *seg_len;
    u32 nout, nsegs, cb;
};
// per segment: what the plan found, what it counts, and the scans of the counts over all segments (nsegs + 1)
struct CpSegs {
    u64 *r0, *hskip;
    u32 *hp, *hlen, *tlen, *hdec, *flags;
    u64 *c_edges, *c_pieces, *c_stage, *c_rows, *c_bytes, *c_kbytes, *c_bound, *c_bad;
    u64 *edges, *pieces, *stage, *rows, *bytes, *kbytes, *bound, *bad;
};
// per output
struct CpOuts {
    u64 *cedge, *cslots, *cstage, *crows;                   // what the output asks of each bound
    u64 *kbytes, *bound;                                    // bytes of its kept chunks; its size bound
    u64* fail;                                              // min over its failing edges of (table row << 8 | status)
    u64 *nrows, *units;                                     // rows of its new index; emit units
    u64 *aedge, *aslots, *abytes, *arows, *nfirst, *gfirst; // scans (nout + 1): of the four counts; new rows; emit units
    u32* flags;
};

// admission in output order: all four sums only grow
struct Admit {
    const u32* flags;
    const u64* __restrict__ aedge;
    const u64* __restrict__ aslots;
    const u64* __restrict__ abytes;
    const u64* __restrict__ arows;
    u32 max_slots;
    u64 stage_cap, max_entries;
    __device__ __forceinline__ bool operator()(u32 j) const
    {
        return (flags[j] & kPass) && aedge[j + 1] <= max_slots && aslots[j + 1] <= max_slots && abytes[j + 1] <= stage_cap && arows[j + 1] <= max_entries;
    }
};

// what the threads of a workgroup found, joined (every thread gets the result); s: 8 words of LDS
__device__ __forceinline__ CcAcc block_join(CcAcc a, u64* s)
{
    if (threadIdx.x < 8) s[threadIdx.x] = 0;
    __syncthreads();
    a.kept = wave_sum(a.kept);
    a.kbytes = wave_sum(a.kbytes);
    a.hdec = wave_sum(a.hdec);
    a.tdec = wave_sum(a.tdec);
    const u64 bad = wave_sum(a.bad ? 1ull : 0);
    if ((threadIdx.x & 63u) == 0) {
        atomic_add64(s + 0, a.kept);
        atomic_add64(s + 1, a.kbytes);
        atomic_add64(s + 2, a.hdec);
        atomic_add64(s + 3, a.tdec);
        atomic_add64(s + 4, bad);
    }
    __syncthreads();
    CcAcc r{};
    r.kept = s[0];
    r.kbytes = s[1];
    r.hdec = s[2];
    r.tdec = s[3];
    r.bad = s[4] != 0;
    return r;
}

// A workgroup per segment.  The segment steers the whole workgroup.
__global__ __launch_bounds__(256) void k_cc_plan(CpArgs a, CpSegs sg)
{
    __shared__ u64 s_acc[8];
    const u32 g = blockIdx.x;
    CcSeg k = cc_begin(a.x, a.in_len, a.ns, a.seg_stream[g], a.seg_off[g], a.seg_len[g]);
    CcAcc acc{};
    if (k.status == SNP_OK && k.r1 > k.r0) {
        const u8* const s = a.in + a.in_off[k.src];
        for (u64 i = k.r0 + threadIdx.x; i < k.r1; i += 256u) cc_add(&acc, a.x, k, i, [&](u64 pos) { return frame_hop(s, k.n, pos); });
    }
    acc = block_join(acc, s_acc);
    if (threadIdx.x != 0) return;
    cc_finish(&k, a.x, a.cb, acc);
    const bool ok = k.status == SNP_OK;
    sg.r0[g] = k.r0;
    sg.hskip[g] = k.hskip;
    sg.hp[g] = static_cast<u32>(k.hp);
    sg.hlen[g] = k.hlen;
    sg.tlen[g] = k.tlen;
    sg.hdec[g] = k.hdec;
    sg.flags[g] = static_cast<u32>(k.status & 0xff) | (k.head ? kHead : 0u) | (k.tail ? kTail : 0u);
    sg.c_edges[g] = cc_seg_edges(k);
    sg.c_pieces[g] = cc_seg_pieces(k);
    sg.c_stage[g] = cc_seg_stage(k);
    sg.c_rows[g] = cc_seg_rows(k);
    sg.c_bytes[g] = cc_seg_bytes(k);
    sg.c_kbytes[g] = k.kbytes;
    sg.c_bound[g] = cc_seg_bound(k);
    sg.c_bad[g] = ok ? 0 : 1;
}

// One thread per output: its segments, its verdict so far, and what it asks -- differences of the scans over the segments.
__global__ __launch_bounds__(256) void k_cc_join(CpArgs a, CpSegs sg, CpOuts o)
{
    const u32 j = blockIdx.x * 256u + threadIdx.x;
    if (j >= a.nout) return;
    u64 s0, s1;
    i32 status = SNP_OK;
    if (!cc_segs(a.seg_first, a.nsegs, j, &s0, &s1)) {
        status = SNP_ERR_BAD_ARG;
    } else if (sg.bad[s1] != sg.bad[s0]) {                              // the first failed segment in segment order
        u64 w;
        const u64 g = cc_seg_of(sg.bad, s0, s1, 0, &w);
        status = g < s1 ? static_cast<i32>(sg.flags[g] & 0xffu) : SNP_ERR_BAD_ARG;
        if (status == SNP_OK) status = SNP_ERR_BAD_ARG;
    }
    const bool ok = status == SNP_OK;
    o.cedge[j] = ok ? cc_count(sg.edges[s1] - sg.edges[s0]) : 0;
    o.cslots[j] = ok ? cc_count(sg.pieces[s1] - sg.pieces[s0]) : 0;
    o.cstage[j] = ok ? cc_count_stage(sg.stage[s1] - sg.stage[s0]) : 0;
    o.crows[j] = ok ? cc_count(sg.rows[s1] - sg.rows[s0]) : 0;
    o.kbytes[j] = ok ? sg.kbytes[s1] - sg.kbytes[s0] : 0;
    o.bound[j] = ok ? SNP_STREAM_HEADER_LEN + (sg.bound[s1] - sg.bound[s0]) : 0;
    o.fail[j] = kNoFail;
    o.flags[j] = static_cast<u32>(status & 0xff) | (ok ? kPass : 0u);
}

// One thread per row of the decode table: an empty row.
__global__ __launch_bounds__(256) void k_cc_clear(u32 max_slots, ChunkRows rows)
{
    const u32 t = blockIdx.x * 256u + threadIdx.x;
    if (t >= max_slots) return;
    rows.tag[t] = kNone;
    chunk_row_clear(rows, t, 0);
}

// One thread per row of the decode table: edge e of an admitted output is row aedge[j] + e, the edges in segment order, head before tail; it
// decodes to the output's staging bytes + what the edges before it decode to.
__global__ __launch_bounds__(256) void k_cc_fill(CpArgs a, CpSegs sg, CpOuts o, Admit admit, ChunkRows rows)
{
    const u32 t = blockIdx.x * 256u + threadIdx.x;
    if (t >= admit.max_slots || t >= o.aedge[a.nout]) return;
    const u32 j = fc_owner(o.aedge, a.nout, t);
    u64 s0, s1, w;
    if (!admit(j) || !cc_segs(a.seg_first, a.nsegs, j, &s0, &s1)) return;
    const u64 g = cc_seg_of(sg.edges, s0, s1, t - o.aedge[j], &w);
    if (g >= s1) return;
    const u32 head = (sg.flags[g] & kHead) ? 1u : 0u;
    const bool tail = w == 1 || !head;
    const u64 kept = sg.c_rows[g] - sg.c_pieces[g];
    const u64 row = sg.r0[g] + (tail ? head + kept : 0);
    const u32 src = a.seg_stream[g];
    const u64 pos = a.x.pos[row];                                       // (what the plan saw: row < r1 <= nentries, pos < in_len)
    const Hop h = frame_hop(a.in + a.in_off[src], a.in_len[src], pos);
    const u64 place = o.abytes[j] + (sg.stage[g] - sg.stage[s0]) + (tail ? sg.hdec[g] : 0);
    if (h.kind != HOP_DATA || place + h.dec > o.abytes[j + 1]) return;
    rows.tag[t] = t;
    chunk_row_set(rows, t, h, a.in_off[src] + pos, place);
}

// an edge that did not decode or verify: its status to its output, the first edge's in order
__global__ __launch_bounds__(256) void k_cc_fail(u32 nout, u32 max_slots, ChunkRows rows, CpOuts o)
{
    const u32 t = blockIdx.x * 256u + threadIdx.x;
    if (t >= max_slots || rows.tag[t] == kNone) return;
    const i32 s = row_verdict(rows, t);
    if (s != SNP_OK) atomic_min64(o.fail + fc_owner(o.aedge, nout, t), (static_cast<u64>(t) << 8) | static_cast<u64>(s & 0xff));
}

// One thread per table slot: piece m of an admitted output is slot aslots[j] + m, the pieces in segment order, head before tail; its bytes lie
// in what its edge decoded to -- there is no assemble pass.
__global__ __launch_bounds__(256) void k_cc_slots(CpArgs a, CpSegs sg, CpOuts o, Admit admit, RwSlots sl, u64 stride)
{
    const u32 c = blockIdx.x * 256u + threadIdx.x;
    if (c >= admit.max_slots) return;
    u64 in_off = 0;
    u32 len = 0;
    if (c < o.aslots[a.nout]) {
        const u32 j = fc_owner(o.aslots, a.nout, c);
        u64 s0, s1, m;
        if (admit(j) && o.fail[j] == kNoFail && cc_segs(a.seg_first, a.nsegs, j, &s0, &s1)) {
            const u64 g = cc_seg_of(sg.pieces, s0, s1, c - o.aslots[j], &m);
            if (g < s1) {
                const CcRow r = cc_piece(sg.hp[g], sg.hskip[g], sg.hlen[g], sg.tlen[g], a.cb, m);
                const u64 at = o.abytes[j] + (sg.stage[g] - sg.stage[s0]) + (r.tail ? sg.hdec[g] : 0) + r.from;
                if (r.len <= a.cb && at + r.len <= o.abytes[j + 1]) {   // (what the plan saw: the piece lies inside its edge)
                    in_off = at;
                    len = r.len;
                }
            }
        }
    }
    sl.in_off[c] = in_off;
    sl.coff[c] = fc_stage_off(c, stride);
    sl.len[c] = len;
}

__global__ __launch_bounds__(256) void k_cc_sizes(CpArgs a, CpOuts o, Admit admit, const u64* __restrict__ cscan, u32 group, u8* __restrict__ out,
                                                 const u64* __restrict__ out_off, const u64* __restrict__ out_cap, u64* __restrict__ out_len,
                                                 i32* __restrict__ status, u64* __restrict__ out_bound, u64* __restrict__ result)
{
    const u32 j = blockIdx.x * 256u + threadIdx.x;
    u64 ok_len = 0, ok = 0, copied = 0;
    if (j == 0) result[0] = o.aedge[a.nout] > o.aslots[a.nout] ? o.aedge[a.nout] : o.aslots[a.nout];
    if (j < a.nout) {
        u32 flags = o.flags[j];
        i32 s = static_cast<i32>(flags & 0xffu);
        u64 bound = o.bound[j], rows = 0, units = 0;
        if (flags & kPass) {
            s = SNP_ERR_OUTPUT_TOO_SMALL;
            if (admit(j)) {
                if (o.fail[j] != kNoFail) {
                    s = static_cast<i32>(o.fail[j] & 0xff);
                    bound = 0;
                } else {
                    const u64 size = SNP_STREAM_HEADER_LEN + o.kbytes[j] + (cscan[o.aslots[j + 1]] - cscan[o.aslots[j]]);
                    if (size <= out_cap[j]) {
                        s = SNP_OK;
                        ok_len = size;
                        ok = 1;
                        flags |= kWritten;
                        rows = o.crows[j];
                        units = (rows + group - 1) / group;
                        copied = rows - o.cslots[j];
                        if (rows == 0)                                  // an output without chunks: the identifier alone
                            for (u32 i = 0; i < SNP_STREAM_HEADER_LEN; ++i) out[out_off[j] + i] = k_fc_stream_id[i];
                    }
                }
            }
        }
        status[j] = s;
        out_len[j] = ok_len;
        if (out_bound) out_bound[j] = bound;
        o.flags[j] = flags;
        o.nrows[j] = rows;
        o.units[j] = units;
    }
    add_written(result, ok_len, ok, copied);
}

// One thread per row of the new index, grid-stride, and per output its three words.  Row i of output j = owner(nfirst, i) is row q of segment
// g = the owner of i - nfirst[j] among the output's segments; cc_row says what it is.  Only written outputs have rows, and they were admitted
// with them.
__global__ __launch_bounds__(256) void k_cc_rows(CpArgs a, CpSegs sg, CpOuts o, const u64* __restrict__ cscan, RwPieces pc, u64 cap,
                                                const i32* __restrict__ status, u64* __restrict__ new_first, u64* __restrict__ new_start,
                                                u64* __restrict__ new_pos, u64* __restrict__ new_total, i32* __restrict__ new_tail)
{
    const u64 total = o.nfirst[a.nout] < cap ? o.nfirst[a.nout] : cap;
    const u64 most = total > static_cast<u64>(a.nout) + 1 ? total : static_cast<u64>(a.nout) + 1;
    for (u64 i = static_cast<u64>(blockIdx.x) * 256u + threadIdx.x; i < most; i += static_cast<u64>(gridDim.x) * 256u) {
        if (i <= a.nout) new_first[i] = o.nfirst[i] < cap ? o.nfirst[i] : cap;
        if (i < a.nout) {
            u64 s0 = 0, s1 = 0;
            const bool written = (o.flags[i] & kWritten) && cc_segs(a.seg_first, a.nsegs, static_cast<u32>(i), &s0, &s1);
            new_total[i] = written ? sg.bytes[s1] - sg.bytes[s0] : 0;
            new_tail[i] = status[i];
        }
        if (i >= total) continue;
        const u32 j = fc_owner(o.nfirst, a.nout, i);
        u64 s0, s1, q, src = 0, start = 0;
        u32 size = 0;
        cc_segs(a.seg_first, a.nsegs, j, &s0, &s1);
        const u64 g = cc_seg_of(sg.rows, s0, s1, i - o.nfirst[j], &q);
        if (g < s1) {
            const u64 pieces = sg.c_pieces[g];
            const CcRow r = cc_row(a.x, sg.r0[g], (sg.flags[g] & kHead) != 0, a.seg_off[g], sg.hp[g], sg.c_rows[g] - pieces, sg.hskip[g], sg.hlen[g],
                                   sg.tlen[g], a.cb, q);
            start = sg.bytes[g] - sg.bytes[s0] + r.at;
            if (r.kept) {
                const u32 s = a.seg_stream[g];
                const u64 pos = a.x.pos[r.row];
                src = a.in_off[s] + pos;
                size = static_cast<u32>(frame_hop(a.in + a.in_off[s], a.in_len[s], pos).next - pos);      // (4 + size < 2^24 + 4)
            } else {
                const u64 c = o.aslots[j] + (sg.pieces[g] - sg.pieces[s0]) + r.slot;
                if (c < o.aslots[j + 1]) {
                    src = kRebuilt | c;
                    size = static_cast<u32>(cscan[c + 1] - cscan[c]);
                }
            }
        }
        new_start[i] = start;
        pc.src[i] = src;
        pc.size[i] = size;
    }
}

// workspace (every piece 256-byte aligned; nothing when there is no output)
struct ComposeWork {
    CpSegs sg;
    CpOuts o;
    RwSlots sl;
    RwPieces pc;
    ChunkRows rows;
    u64 *part, *cscan;
    u8 *stage, *comp;
    u64 bytes;
};
ComposeWork work_layout(void* base, u32 nout, u32 nsegs, u32 max_slots, u64 stage_cap, u32 chunk_bytes, u32 max_entries)
{
    ComposeWork w{};
    if (nout == 0 || chunk_bytes == 0 || chunk_bytes > SNP_BLOCK_SIZE) return w;
    const u64 no = nout, G = nsegs, M = max_slots, E = max_entries;
    WorkCarver k(base);
    w.part = k.take<u64>(scan_tiles_of(std::max(std::max(no, G), std::max(M, E))));
    for (u64** p : {&w.sg.r0, &w.sg.hskip, &w.sg.c_edges, &w.sg.c_pieces, &w.sg.c_stage, &w.sg.c_rows, &w.sg.c_bytes, &w.sg.c_kbytes, &w.sg.c_bound,
                    &w.sg.c_bad})
        *p = k.take<u64>(G);
    for (u32** p : {&w.sg.hp, &w.sg.hlen, &w.sg.tlen, &w.sg.hdec, &w.sg.flags}) *p = k.take<u32>(G);
    for (u64** p : {&w.sg.edges, &w.sg.pieces, &w.sg.stage, &w.sg.rows, &w.sg.bytes, &w.sg.kbytes, &w.sg.bound, &w.sg.bad}) *p = k.take<u64>(G + 1);
    for (u64** p : {&w.o.cedge, &w.o.cslots, &w.o.cstage, &w.o.crows, &w.o.kbytes, &w.o.bound, &w.o.fail, &w.o.nrows, &w.o.units}) *p = k.take<u64>(no);
    for (u64** p : {&w.o.aedge, &w.o.aslots, &w.o.abytes, &w.o.arows, &w.o.nfirst, &w.o.gfirst}) *p = k.take<u64>(no + 1);
    w.o.flags = k.take<u32>(no);
    w.sl = carve_rw_slots(k, M);
    w.rows = carve_chunk_rows(k, M);
    w.cscan = k.take<u64>(M + 1);
    w.pc = carve_rw_pieces(k, E);
    // staging: per admitted output what its edges decode to, one behind the other, the outputs back to back (+ slack for the compressor's
    // vector loads).  Compressed staging: slot c at c * snp_comp_stride(chunk_bytes) (fc_stage_off).
    w.stage = k.take<u8>(stage_cap + 256);
    w.comp = k.take<u8>(M * snp_comp_stride(chunk_bytes));
    w.bytes = k.bytes();
    return w;
}

}  // namespace

extern "C" {

uint64_t snp_frame_compose_indexed_workspace(uint32_t nstreams, uint32_t nout, uint32_t nsegs, uint32_t max_slots, uint64_t stage_cap,
                                             uint32_t chunk_bytes, uint32_t max_entries)
{
    (void)nstreams;                                                     // (nothing is kept per source)
    return work_layout(nullptr, nout, nsegs, max_slots, stage_cap, chunk_bytes, max_entries).bytes;
}

snp_status snp_frame_compose_indexed_batch(snp_ctx* c, const uint8_t* in, const uint64_t* in_off, const uint64_t* in_len, uint32_t nstreams,
                                           const uint64_t* idx_first, const uint64_t* idx_start, const uint64_t* idx_pos, const uint64_t* idx_total,
                                           const int32_t* idx_tail, uint64_t nentries, const uint64_t* seg_first, const uint32_t* seg_stream,
                                           const uint64_t* seg_off, const uint64_t* seg_len, uint32_t nout, uint32_t nsegs, uint32_t chunk_bytes,
                                           uint32_t max_slots, uint64_t stage_cap, uint32_t max_entries, uint8_t* out, const uint64_t* out_off,
                                           const uint64_t* out_cap, uint64_t* out_len, int32_t* status, uint64_t* new_first, uint64_t* new_start,
                                           uint64_t* new_pos, uint64_t* new_total, int32_t* new_tail, uint64_t* out_bound, void* d_work,
                                           uint64_t* d_result)
{
    if (!c || !d_result || chunk_bytes == 0 || chunk_bytes > SNP_BLOCK_SIZE || nout > 0x7fffffffu || nsegs > 0x7fffffffu ||      // (one workgroup per segment)
        nstreams > 0x7fffffffu ||
        (nout && (!seg_first || !out || !out_off || !out_cap || !out_len || !status || !new_first || !new_total || !new_tail || !d_work)) ||
        (nout && nsegs && (!seg_stream || !seg_off || !seg_len)) ||
        (nout && nstreams && (!in || !in_off || !in_len || !idx_first || !idx_total || !idx_tail)) ||
        (nout && nstreams && nentries && (!idx_start || !idx_pos)) || (nout && max_entries && (!new_start || !new_pos)))
        return SNP_ERR_BAD_ARG;
    DevGuard dg(c);
    if (!dg.ok) return SNP_ERR_DEVICE;
    hipStream_t s = c->stream;
    bool ok = c->check(snp_zero_words_async(reinterpret_cast<u32*>(d_result), 2 * 6, s), "frame compose result");
    if (nout == 0) return ok ? SNP_OK : SNP_ERR_DEVICE;
    const ComposeWork w = work_layout(d_work, nout, nsegs, max_slots, stage_cap, chunk_bytes, max_entries);
    const u32 no = nout, G = nsegs, M = max_slots, E = max_entries, cb = chunk_bytes, og = groups_of(no), mg = groups_of(M);
    const CpArgs a{in, in_off, in_len, nstreams, FrameIndex{idx_first, idx_start, idx_pos, idx_total, idx_tail, nentries}, seg_first, seg_stream,
                   seg_off, seg_len, no, G, cb};
    const Admit admit{w.o.flags, w.o.aedge, w.o.aslots, w.o.abytes, w.o.arows, M, stage_cap, E};
    // the plan of every segment on its own; what each counts, scanned over all segments: an output's share is a difference
    if (G) hipLaunchKernelGGL(k_cc_plan, dim3(G), dim3(256), 0, s, a, w.sg);
    ok = ok && c->check(hipGetLastError(), "frame compose plan");
    const struct { const u64* src; u64* dst; } seg_scans[] = {{w.sg.c_edges, w.sg.edges}, {w.sg.c_pieces, w.sg.pieces}, {w.sg.c_stage, w.sg.stage},
                                                              {w.sg.c_rows, w.sg.rows},   {w.sg.c_bytes, w.sg.bytes},   {w.sg.c_kbytes, w.sg.kbytes},
                                                              {w.sg.c_bound, w.sg.bound}, {w.sg.c_bad, w.sg.bad}};
    for (const auto& q : seg_scans) ok = ok && c->check(launch_scan(ScanWords{q.src}, G, w.part, q.dst, nullptr, s), "frame compose segment scan");
    // every output's verdict so far; admission in output order (d_result[2] = staging bytes, [4] = new rows; [0] comes with the verdicts)
    if (ok) {
        hipLaunchKernelGGL(k_cc_join, dim3(og), dim3(256), 0, s, a, w.sg, w.o);
        ok = c->check(hipGetLastError(), "frame compose join") &&
             c->check(launch_scan(ScanWords{w.o.cedge}, no, w.part, w.o.aedge, nullptr, s), "frame compose edge scan") &&
             c->check(launch_scan(ScanWords{w.o.cslots}, no, w.part, w.o.aslots, nullptr, s), "frame compose slot scan") &&
             c->check(launch_scan(ScanWords{w.o.cstage}, no, w.part, w.o.abytes, d_result + 2, s), "frame compose staging scan") &&
             c->check(launch_scan(ScanWords{w.o.crows}, no, w.part, w.o.arows, d_result + 4, s), "frame compose entry scan");
    }
    if (ok && M) {
        // the edges decoded and verified whole into staging, one behind the other
        hipLaunchKernelGGL(k_cc_clear, dim3(mg), dim3(256), 0, s, M, w.rows);
        hipLaunchKernelGGL(k_cc_fill, dim3(mg), dim3(256), 0, s, a, w.sg, w.o, admit, w.rows);
        ok = c->check(hipGetLastError(), "frame compose fill") && c->decode_chunks(in, w.rows, M, w.stage);
        if (ok) {
            hipLaunchKernelGGL(k_cc_fail, dim3(mg), dim3(256), 0, s, no, M, w.rows, w.o);
            hipLaunchKernelGGL(k_cc_slots, dim3(mg), dim3(256), 0, s, a, w.sg, w.o, admit, w.sl, snp_comp_stride(cb));
            ok = c->check(hipGetLastError(), "frame compose slots");
        }
    }
    // every piece re-encoded from where the edges were decoded to, and the framed sizes; every output's verdict, its emit units and the rows of
    // its new index
    ok = ok && reencode_slots(c, w.stage, w.sl, M, w.comp, w.part, w.cscan, "frame compose");
    if (ok) {
        const u32 group = fc_group(cb);
        hipLaunchKernelGGL(k_cc_sizes, dim3(og), dim3(256), 0, s, a, w.o, admit, w.cscan, group, out, out_off, out_cap, out_len, status, out_bound,
                           d_result);
        ok = c->check(hipGetLastError(), "frame compose sizes") &&
             c->check(launch_scan(ScanWords{w.o.units}, no, w.part, w.o.gfirst, nullptr, s), "frame compose unit scan") &&
             c->check(launch_scan(ScanWords{w.o.nrows}, no, w.part, w.o.nfirst, nullptr, s), "frame compose new row scan");
        if (ok) {
            const u64 most = std::max<u64>(E, static_cast<u64>(no) + 1);
            hipLaunchKernelGGL(k_cc_rows, dim3(static_cast<u32>(std::min<u64>((most + 255) / 256, kRowGroups))), dim3(256), 0, s, a, w.sg, w.o, w.cscan,
                               w.pc, E, status, new_first, new_start, new_pos, new_total, new_tail);
            ok = c->check(hipGetLastError(), "frame compose rows") &&
                 c->check(launch_scan(ScanPieces{w.pc.size, w.o.nfirst + no, E}, E, w.part, w.pc.scan, nullptr, s), "frame compose chunk scan");
            if (ok) {
                hipLaunchKernelGGL(k_rw_emit<RwOwners>, dim3(kEmitGroups), dim3(256), 0, s, RwOwners{w.o.gfirst, w.o.nfirst, no}, w.sl, w.pc, group, fc_team(group),
                                   in, w.stage, w.comp, out, out_off, new_pos);
                ok = c->check(hipGetLastError(), "frame compose emit");
            }
        }
    }
    return ok ? SNP_OK : SNP_ERR_DEVICE;
}

}  // extern "C"

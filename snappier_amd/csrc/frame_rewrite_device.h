// frame_rewrite_device.h -- what the calls that REWRITE seekable framed streams share: update (frame_update.hip), append (frame_append.hip),
// splice (frame_splice.hip), rechunk (frame_rechunk.hip) and compose (frame_compose.hip).  Each call keeps its own plan, kernels and launch
// sequence; here is only what is the same in all of them: the scan sources, the grid constants, the verdict over a decoded table row, the slot
// table the compressor, the CRC and the emit read, the host step that re-encodes the slots, the emit of one slot, and -- rechunk and compose --
// the piece table of a new stream and the emit over it.  The chunk header itself is chunk_header (snp_device.h), the CompressBlock rule
// payload_of (frame_chunked_device.h).  DESIGN.md 4.17.
#pragma once
#include <string>

#include "capi_internal.h"
#include "frame_chunked_device.h"
#include "scan_tiles.h"
#include "work_carver.h"

namespace {

constexpr u64 kNoFail = ~0ull;                                      // no row of the stream failed (the minimum of the failure keys)
constexpr u64 kRebuilt = 1ull << 63;                                // a new row's source: a slot, not a place in `in`
constexpr u64 kUnit = 65536;                                        // bytes of an old stream one emit workgroup takes at a time
constexpr u32 kEmitGroups = 2048;                                   // grid of the grid-stride emit: 8 workgroups per CU
constexpr u32 kRowGroups = 1u << 20;                                // ... of the kernels over the rows of the new index

inline u32 groups_of(u64 n) { return static_cast<u32>((n + 255) / 256); }

// scan sources: a table of words; 8 + payload of a slot (0 for an empty one); the chunk sizes of the new rows there are
struct ScanWords {
    const u64* __restrict__ src;
    __device__ __forceinline__ u64 operator()(u64 i) const { return src[i]; }
};
struct ScanFramed {
    const u32* __restrict__ len;
    const u32* __restrict__ comp_len;
    __device__ __forceinline__ u64 operator()(u64 i) const
    {
        bool shrink;
        return len[i] ? SNP_CHUNK_HEADER_LEN + payload_of(comp_len[i], len[i], &shrink) : 0;
    }
};
struct ScanPieces {
    const u32* __restrict__ size;
    const u64* __restrict__ nrows;                          // nfirst + n: the rows there are
    u64 cap;
    __device__ __forceinline__ u64 operator()(u64 i) const { return i < (*nrows < cap ? *nrows : cap) ? size[i] : 0; }
};

// the verdict over row t of a decode table after snp_ctx::decode_chunks: the row's own status, or INCOMPLETE when it decoded to fewer bytes
// than its header lists.  To whom a failure goes is each call's own.
__device__ __forceinline__ i32 row_verdict(const ChunkRows& rows, u64 t)
{
    return rows.status[t] != SNP_OK ? rows.status[t] : rows.out_len[t] != rows.out_cap[t] ? SNP_ERR_INCOMPLETE : SNP_OK;
}

// per table slot: what the compressor, the CRC and the emit read
struct RwSlots {
    u64 *in_off, *coff;
    u32 *len, *comp_len, *crc;
    i32* c_status;
};
// ... and the stream the slot belongs to (append, splice; the field and carve order these two have always had)
struct RwOwnedSlots {
    u64 *in_off, *coff;
    u32 *len, *stream, *comp_len, *crc;
    i32* c_status;
    __host__ __device__ RwSlots rw() const { return RwSlots{in_off, coff, len, comp_len, crc, c_status}; }
};
inline RwSlots carve_rw_slots(WorkCarver& k, u64 n)
{
    RwSlots s;
    s.in_off = k.take<u64>(n);
    s.coff = k.take<u64>(n);
    s.len = k.take<u32>(n);
    s.comp_len = k.take<u32>(n);
    s.crc = k.take<u32>(n);
    s.c_status = k.take<i32>(n);
    return s;
}
inline RwOwnedSlots carve_rw_owned_slots(WorkCarver& k, u64 n)
{
    RwOwnedSlots s;
    s.in_off = k.take<u64>(n);
    s.coff = k.take<u64>(n);
    s.len = k.take<u32>(n);
    s.stream = k.take<u32>(n);
    s.comp_len = k.take<u32>(n);
    s.crc = k.take<u32>(n);
    s.c_status = k.take<i32>(n);
    return s;
}

// snp_ctx::check with the message "<what> <step>": `what` names the call
inline bool check_step(snp_ctx* c, hipError_t e, const char* what, const char* step)
{
    return e == hipSuccess || c->check(e, (std::string(what) + " " + step).c_str());
}
// CompressBlock of every slot (varint on) and its masked CRC-32C: one launch sequence each, from `stage`
inline bool compress_slots(snp_ctx* c, const u8* stage, const RwSlots& sl, u32 M, u8* comp, const char* what)
{
    return c->launch_compress(stage, sl.in_off, sl.len, M, comp, sl.coff, sl.comp_len, sl.c_status, 1) &&
           check_step(c, snp_launch_crc32c(stage, sl.in_off, sl.len, M, 1 | c->crc_bits(), sl.crc, nullptr, nullptr, c->stream), what, "crc");
}
// ... and cscan[0 .. M] = the scan of the framed sizes.  The scan runs over an empty table too (cscan[0] = 0); the other two are not launched then.
inline bool reencode_slots(snp_ctx* c, const u8* stage, const RwSlots& sl, u32 M, u8* comp, u64* part, u64* cscan, const char* what)
{
    return (M == 0 || compress_slots(c, stage, sl, M, comp, what)) &&
           check_step(c, launch_scan(ScanFramed{sl.len, sl.comp_len}, M, part, cscan, nullptr, c->stream), what, "size scan");
}

// slot c as a framed chunk at `at`, by a team of `team` threads (t: the thread's place in it): header + what the compressor staged, or the
// slot's own bytes in `stage` where they did not shrink.  All threads of the team must call it.
__device__ __forceinline__ void emit_slot(u8* at, const RwSlots& sl, u64 c, const u8* stage, const u8* comp, u32 t, u32 team)
{
    bool shrink;
    const u32 pl = payload_of(sl.comp_len[c], sl.len[c], &shrink);
    chunk_header(at, t, shrink ? 0u : 1u, pl, sl.crc[c]);
    team_copy(at + SNP_CHUNK_HEADER_LEN, shrink ? comp + sl.coff[c] : stage + sl.in_off[c], pl, t, team);
}

// ---- rechunk and compose: a new stream is a run of rows, each a kept chunk of `in` or a rebuilt slot ---------------------------------------------
// per new row
struct RwPieces {
    u64* src;                                               // kept: the old chunk's header, in `in`; kRebuilt | slot
    u32* size;                                              // the chunk's bytes in the new stream (0: a row of a stream that is not written)
    u64* scan;                                              // (max_entries + 1)
};
inline RwPieces carve_rw_pieces(WorkCarver& k, u64 E)
{
    RwPieces p;
    p.src = k.take<u64>(E);
    p.size = k.take<u32>(E);
    p.scan = k.take<u64>(E + 1);
    return p;
}
// the n streams (outputs) that own the emit units and the new rows: the scans (n + 1) of each
struct RwOwners {
    const u64 *gfirst, *nfirst;
    u32 n;
};

// exclusive scan of v over the wavefront; *total: the sum (the fill kernels of the rechunk and the recut: a row's place among its stream's dirty rows)
__device__ __forceinline__ u64 wave_scan(u64 v, u64* total)
{
    const u32 lane = lane_id();
    u64 inc = v;
    for (u32 d = 1; d < 64; d <<= 1) {
        const u64 o = __shfl_up(inc, d, 64);
        if (lane >= d) inc += o;
    }
    *total = __shfl(inc, 63, 64);
    return inc - v;
}

// the tail of the sizes kernels: what the wavefront's streams add to d_result[1] (bytes written), [3] (streams written) and [5] (the call's own
// count), one atomic per wavefront each.  All lanes must call it.
__device__ __forceinline__ void add_written(u64* result, u64 ok_len, u64 ok, u64 extra)
{
    ok_len = wave_sum(ok_len);
    ok = wave_sum(ok);
    extra = wave_sum(extra);
    if ((threadIdx.x & 63u) == 0) {
        if (ok) {
            atomic_add64(result + 1, ok_len);
            atomic_add64(result + 3, ok);
        }
        if (extra) atomic_add64(result + 5, extra);
    }
}

// One workgroup per emit unit of a written stream: `group` consecutive chunks of the new stream, taken by teams of `team` threads in turn
// (fc_group and fc_team, frame_chunked_device.h).  A kept chunk is copied from `in` as it is; a rebuilt one is emit_slot.  The unit steers the whole
// workgroup, a chunk its whole team.  The first unit of a stream writes the identifier.  (A template so that only the two libraries that
// launch it hold a copy.)
template <class Owners>
__global__ __launch_bounds__(256) void k_rw_emit(Owners o, RwSlots sl, RwPieces pc, u32 group, u32 team, const u8* __restrict__ in,
                                                const u8* __restrict__ stage, const u8* __restrict__ comp, u8* __restrict__ out,
                                                const u64* __restrict__ out_off, u64* __restrict__ new_pos)
{
    const u32 tid = threadIdx.x, t = tid % team, teams = 256u / team;
    const u64 units = o.gfirst[o.n];
    for (u64 g = blockIdx.x; g < units; g += gridDim.x) {
        const u32 b = fc_owner(o.gfirst, o.n, g);
        const u64 u = g - o.gfirst[b], first = o.nfirst[b], last = o.nfirst[b + 1];
        const u64 i0 = first + u * group, i1 = i0 + group < last ? i0 + group : last;
        u8* const dst = out + out_off[b];
        if (u == 0 && tid < SNP_STREAM_HEADER_LEN) dst[tid] = k_fc_stream_id[tid];       // EnsureStreamHeaderWritten  SnappyStreamCompressor.cs:148-157
        for (u64 i = i0 + tid / team; i < i1; i += teams) {
            const u64 src = pc.src[i], pos = SNP_STREAM_HEADER_LEN + (pc.scan[i] - pc.scan[first]);
            if (t == 0) new_pos[i] = pos;
            if (pc.size[i] == 0) continue;
            if (src & kRebuilt) emit_slot(dst + pos, sl, src & ~kRebuilt, stage, comp, t, team);
            else team_copy(dst + pos, in + src, pc.size[i], t, team);
        }
    }
}

}  // namespace

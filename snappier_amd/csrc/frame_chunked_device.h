// frame_chunked_device.h -- the slot arithmetic of snp_frame_encode_chunked_batch (frame_chunked.hip): a batch of buffers cut into pieces of
// chunk_bytes, the pieces of all buffers in one table of max_chunks slots.  Which buffer owns a slot, which piece of it the slot is, where the
// slot's compressed bytes are staged, how many slots one emit workgroup takes, and the index row of a chunk once the scan over the OK buffers'
// chunk counts exists.  __host__ __device__ throughout, so that the same code runs on the CPU under sanitizers
// (tests/abi/frame_chunked_plan_check.hip) on buffers past 4 GiB, where k * chunk_bytes does not fit 32 bits.  DESIGN.md 4.15.
// At the end, device only: what the emit kernel of this call shares with those of the five calls that rewrite seekable streams (through
// frame_rewrite_device.h) -- the stream identifier, the CompressBlock rule for a chunk's payload, and team_copy.
//
// first[0 .. nb] is the exclusive scan of fc_chunks(in_len[b], cb) (first[nb] = the slots the batch needs); ok_first[0 .. nb] the same scan over
// the buffers whose status is SNP_OK only, made after the size verdict: an out_cap failure can hit a buffer in the middle of the batch, so the
// rows of the buffers after it move down.
#pragma once
#include "snp_device.h"

namespace {

constexpr u32 kFcNone = 0xffffffffu;            // a slot that no admitted buffer owns
constexpr u32 kFcGroupBytes = SNP_BLOCK_SIZE;   // input bytes one emit workgroup takes, in whole slots

__host__ __device__ __forceinline__ u64 fc_chunks(u64 len, u32 cb) { return len / cb + (len % cb != 0); }

// slots per emit workgroup: as many consecutive ones as hold 64 KiB of input (1 from 32 769-byte chunks up ... 65 536 at 1-byte chunks)
__host__ __device__ __forceinline__ u32 fc_group(u32 cb) { return (kFcGroupBytes + cb - 1) / cb; }
// threads of the 256 that copy one slot together: all of them when the workgroup has one slot, half with two, else one wavefront
__host__ __device__ __forceinline__ u32 fc_team(u32 group) { return group == 1 ? 256u : group == 2 ? 128u : 64u; }

// the last b in [0, nb) with first[b] <= c (first non-decreasing, first[0] = 0): the owner of slot c < first[nb]
__host__ __device__ inline u32 fc_owner(const u64* __restrict__ first, u32 nb, u64 c)
{
    u32 lo = 0, hi = nb;
    while (hi - lo > 1) {
        const u32 mid = lo + (hi - lo) / 2;
        if (first[mid] <= c) lo = mid;
        else hi = mid;
    }
    return lo;
}

struct FcSlot {
    u32 owner;      // kFcNone: past the batch, or the slot of a buffer whose chunks do not fit max_chunks (prefix admission: so does every later one)
    u32 len;        // the piece's bytes (1 .. cb)
    u64 k;          // its number among the owner's chunks
    u64 off;        // its first byte, relative to the owner's first: k * cb, in 64 bits
};

__host__ __device__ inline FcSlot fc_slot(const u64* __restrict__ first, const u64* __restrict__ in_len, u32 nb, u32 max_chunks, u32 cb, u32 c)
{
    FcSlot s{kFcNone, 0, 0, 0};
    if (c >= first[nb]) return s;
    const u32 b = fc_owner(first, nb, c);
    if (first[b + 1] > max_chunks) return s;
    s.owner = b;
    s.k = c - first[b];
    s.off = s.k * cb;
    const u64 rest = in_len[b] - s.off;
    s.len = rest < cb ? static_cast<u32>(rest) : cb;
    return s;
}

// where slot c's compressed bytes are staged (stride = snp_comp_stride(cb), capi_internal.h)
__host__ __device__ __forceinline__ u64 fc_stage_off(u32 c, u64 stride) { return static_cast<u64>(c) * stride; }

// the index row of chunk k of an OK buffer whose rows start at ok_first_b (include/snappier_hip_frame_index.h: the decoded bytes before the chunk)
struct FcRow { u64 row, start; };
__host__ __device__ __forceinline__ FcRow fc_row(u64 ok_first_b, u64 k, u32 cb) { return FcRow{ok_first_b + k, k * cb}; }

// ---- what the emit kernels of the chunked encode and of the rewrite calls (frame_rewrite_device.h) share ---------------------------------------
__constant__ u8 k_fc_stream_id[SNP_STREAM_HEADER_LEN] = {0xff, 0x06, 0x00, 0x00, 0x73, 0x4e, 0x61, 0x50, 0x70, 0x59};   // SnappyStreamCompressor.cs:18-21

__device__ __forceinline__ u32 payload_of(u32 comp, u32 raw, bool* shrink)
{
    *shrink = comp < raw;                                               // CompressBlock  SnappyStreamCompressor.cs:212
    return *shrink ? comp : raw;
}

// len bytes by a team of T threads (t = the thread's place in it), src and dst apart.  From 64 bytes on the destination is brought to a 16-byte
// boundary by byte stores first -- a chunk lands wherever the scan puts it -- and the body leaves as aligned 16-byte stores; shorter pieces
// are not worth the head.  All threads of the team must call it.
__device__ __forceinline__ void team_copy(u8* dst, const u8* src, u32 len, u32 t, u32 T)
{
    if (len < 64) {
        if (t < len) dst[t] = src[t];                                   // (T >= 64)
        return;
    }
    const u32 head = static_cast<u32>(16u - (reinterpret_cast<uintptr_t>(dst) & 15u)) & 15u;
    if (t < head) dst[t] = src[t];
    const u32 body = (len - head) & ~15u;
    for (u32 k = t * 16; k < body; k += T * 16) {
        const snp_u128_unaligned w = *reinterpret_cast<const snp_u128_unaligned*>(src + head + k);
        *reinterpret_cast<uint4*>(dst + head + k) = make_uint4(w.v[0], w.v[1], w.v[2], w.v[3]);
    }
    const u32 done = head + body;
    if (t < len - done) dst[done + t] = src[done + t];                  // (< 16 bytes)
}

}  // namespace

// frame_append_device.h -- the planning of the indexed APPEND (snp_frame_append_indexed_batch, frame_append.hip) over a chunk index that is UNTRUSTED
// input, on top of frame_index_device.h (the index, its clamps, the hop) and frame_chunked_device.h (pieces of chunk_bytes, the owner of a slot):
// the plan of ONE stream (its verdict before anything is decoded, the check of its last row against the header it points at, whether the tail
// chunk is reopened, the fill, the cut, the fresh slots and the size bound), a fresh slot's piece and where it lies in the source, in 64 bits,
// and the index row of a fresh chunk.  __host__ __device__ throughout, so that the same code runs on the CPU under sanitizers
// (tests/abi/frame_append_plan_check.hip) over indexes filled with anything at all and over positions and lengths past 4 GiB.  DESIGN.md 4.18.
//
// The tail chunk (the stream's last index row L, d = total - start[L] decoded bytes) is REOPENED iff 0 < d < chunk_bytes and the chunk ends exactly
// at the stream's last byte: it is decoded, filled up with the first appended bytes and encoded again at its old position, the CUT.  Else the cut
// is the stream's end.  Nothing before the cut is written, so no old row ever moves.
#pragma once
#include "frame_index_device.h"
#include "frame_chunked_device.h"

namespace {

constexpr u32 kFaMaxDec = SNP_BLOCK_SIZE;       // what one chunk may be re-encoded from

struct FaPlan {
    i32 status;         // SNP_OK: the stream passed (append: it has bytes to take, else it is left alone); else its answer
    bool append;        // passed and src_len > 0
    bool reopen;        // the tail chunk is decoded, filled and encoded again
    bool ident;         // an empty stream: the identifier goes first
    u32 d, fill;        // decoded bytes of the reopened tail; appended bytes that go into it
    u32 type, body_len, crc;    // the reopened tail's header, as the chunk table takes it
    u64 f0, rows;       // the stream's old rows [f0, f0 + rows) (clamped; also of a stream that did not pass)
    u64 cut;            // stream-relative: nothing before it is written
    u64 rest, fresh;    // appended bytes behind the fill; their chunks
    u64 bound;          // size bound of the new stream, from the headers alone (buf_len for a stream that is left alone or refused)
};

// the old rows of stream b as the new index copies them: [f0, f0 + rows), inside nentries whatever idx_first holds
__host__ __device__ __forceinline__ void fa_rows(const FrameIndex& x, u32 b, u64* f0, u64* rows)
{
    const u64 a = x.first[b] < x.nentries ? x.first[b] : x.nentries, e = x.first[b + 1] < x.nentries ? x.first[b + 1] : x.nentries;
    *f0 = a;
    *rows = e > a ? e - a : 0;
}

// Stream b of n = buf_len bytes with src_len bytes to take, in chunks of cb.  hop_at(pos) -> the Hop of the header at pos < n (frame_hop over
// the stream's bytes; the check program also gives hops as numbers, for streams too long to hold).
template <class HopAt>
__host__ __device__ inline FaPlan fa_plan(const FrameIndex& x, u32 b, u64 n, u64 src_len, u32 cb, HopAt hop_at)
{
    FaPlan k{};
    fa_rows(x, b, &k.f0, &k.rows);
    k.cut = n;
    k.bound = n;
    k.status = SNP_OK;
    if (src_len == 0) return k;                                         // nothing to append: not one array of the index is trusted for it
    k.status = SNP_ERR_BAD_ARG;
    const i32 tail = x.tail[b];
    if (tail < SNP_OK || tail > SNP_ERR_TRUNCATED_STREAM) return k;     // (no status of the walk)
    if (tail != SNP_OK) { k.status = tail; return k; }                  // not indexed, or broken: a broken stream is not appended to
    const u64 g0 = x.first[b] < x.nentries ? x.first[b] : x.nentries, g1 = x.first[b + 1] < x.nentries ? x.first[b + 1] : x.nentries;
    if (g1 < g0) return k;
    const u64 total = x.total[b];
    if (total + src_len < total) return k;
    u64 old = 0;                                                        // bytes of the reopened chunk, header included
    if (g1 > g0) {
        const u64 L = g1 - 1, start = x.start[L], pos = x.pos[L];
        if (start > total || pos >= n) return k;
        const Hop h = hop_at(pos);
        if (h.kind != HOP_DATA || h.dec != total - start) return k;     // a data chunk that decodes to exactly d bytes
        if (h.dec > 0 && h.dec < cb && h.next == n) {
            if (h.dec > kFaMaxDec) return k;                            // (cb <= 65536: never; the rule stands on its own)
            k.reopen = true;
            k.d = h.dec;
            k.type = h.type;
            k.body_len = h.body_len;
            k.crc = h.crc;
            k.cut = pos;
            old = h.next - pos;
        }
    } else if (total != 0) {
        return k;                                                       // decoded bytes and no row that holds them
    }
    k.status = SNP_OK;
    k.append = true;
    k.ident = n == 0;
    const u64 room = k.reopen ? cb - k.d : 0;
    k.fill = static_cast<u32>(src_len < room ? src_len : room);
    k.rest = src_len - k.fill;
    k.fresh = fc_chunks(k.rest, cb);
    k.bound = n - old + (k.reopen ? SNP_CHUNK_HEADER_LEN + static_cast<u64>(k.d) + k.fill : 0) + SNP_CHUNK_HEADER_LEN * k.fresh + k.rest +
              (k.ident ? SNP_STREAM_HEADER_LEN : 0);
    return k;
}

// Fresh chunk j of a stream whose appended bytes behind the fill are `rest`: its bytes and where they start among the stream's appended bytes
struct FaPiece { u32 len; u64 off; };
__host__ __device__ __forceinline__ FaPiece fa_piece(u64 rest, u32 fill, u32 cb, u64 j)
{
    const u64 at = j * cb, left = rest - at;                            // (j < fc_chunks(rest, cb): at < rest)
    return FaPiece{left < cb ? static_cast<u32>(left) : cb, fill + at};
}

// the decoded bytes before fresh chunk j: the row's start (its pos comes from the size scan)
__host__ __device__ __forceinline__ u64 fa_row_start(u64 total, u32 fill, u32 cb, u64 j) { return total + fill + j * cb; }

}  // namespace

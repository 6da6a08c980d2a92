/*
 * snappier_hip_frame_cuts.h -- C-ABI of libsnappier_hip_frame_cuts.so: CONTENT-DEFINED CHUNKING of many buffers on the device.  Two calls: a finder
 * that says where the bytes of a buffer put its cuts, and a chunked frame encoder that takes the cuts as input instead of a stride.
 * snp_frame_encode_chunked_batch (snappier_hip_frame_chunked.h) places chunks on a grid k * chunk_bytes: a function of the offset, so two
 * versions of a buffer that differ by an insert share no chunk behind it.  Cuts that follow the content fall back into step behind an edit (the
 * rsync / restic / borg family), and the seekable calls -- index, read, update, append, splice, edit, rechunk, compose, digest, diff, find --
 * take chunks of any size as they are.
 *
 * An extension of include/snappier_hip.h in a library of its own, linked against libsnappier_hip.so and taking that library's contexts (snp_ctx).
 * It adds no status code and no option, keeps no state in the context and reads no environment; the surfaces of snappier_hip.h and the other
 * extension headers are unchanged.  The C# side binds these functions in csharp/Snappier.Gpu/NativeMethodsFrameCuts.cs.
 */
#ifndef SNAPPIER_HIP_FRAME_CUTS_H
#define SNAPPIER_HIP_FRAME_CUTS_H

#include "snappier_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SNP_CUTS_MIN_WINDOW 32
#define SNP_CUTS_MAX_WINDOW 32767

/* The cut rule.  Parameters: window w (SNP_CUTS_MIN_WINDOW .. SNP_CUTS_MAX_WINDOW) and max_bytes mx (w < mx <= 65536).  For a buffer x of n bytes:
 *   GEAR[b] = fmix32((b + 1) * 0x9E3779B9 mod 2^32), fmix32 the murmur3 finaliser (h ^= h >> 16; h *= 0x85ebca6b; h ^= h >> 13; h *= 0xc2b2ae35;
 *   h ^= h >> 16);  g(0) = 0, g(c + 1) = (g(c) << 1) + GEAR[x[c]] mod 2^32 -- g(c) depends on the 32 bytes before offset c only.
 *   Offset c is a CONTENT cut iff w < c < n - w, g(c) > g(c') for every c' in [c - w, c), and g(c) >= g(c') for every c' in (c, c + w].  A tie
 *   loses on the left, so a constant run has none; two content cuts are more than w apart; a buffer of n <= 2 w + 1 bytes has none; whether c is
 *   one depends on x[c - w - 32, c + w) and the distance to the two ends only.
 *   FORCED cuts: for neighbours a < b of {0} + content cuts + {n}, every a + k * mx < b with k >= 1.  Every piece is then 1 .. mx bytes.
 *   The buffer's cuts are the union, ascending, strictly inside (0, n), relative to the buffer's first byte.  The mean piece is about 2 w.
 *   Buffer b never has more than in_len[b] / (w + 1) + in_len[b] / mx cuts.
 *
 * snp_content_cuts_batch: nbuffers raw buffers on the device, buffer b = in[in_off[b] .. +in_len[b]).  Admission is in buffer order: a buffer is
 * admitted when the bytes of the buffers up to and including it fit span_bytes and their cuts fit max_cuts (sums saturate; span_bytes above 2^40
 * counts as 2^40).  status[b] = SNP_OK for an admitted buffer; the first buffer that misses a bound and every later one get
 * SNP_ERR_OUTPUT_TOO_SMALL and own no cut.  cut_first[0 .. nbuffers] is the exclusive scan of the admitted buffers' cut counts, and
 * cuts[cut_first[b] .. cut_first[b + 1]) holds buffer b's cuts; nothing of `cuts` beyond cut_first[nbuffers] is written (cuts may be null when
 * max_cuts is 0).  An empty buffer is OK with no cut.  The result is deterministic: no atomic decides an order or a value.
 * d_result (device, 4 x u64): [0] = the cuts of the buffers whose bytes fit span_bytes (all of them when [2] <= span_bytes: grow max_cuts to it),
 * [1] = cuts written (= cut_first[nbuffers]), [2] = bytes the batch holds (grow span_bytes to it), [3] = buffers that are OK.  So sizing takes
 * one round with max_cuts = 0; a caller who sums the bound above over its buffers needs none.
 * d_work must hold snp_content_cuts_workspace(nbuffers, span_bytes, window) bytes (host arithmetic; 0 when nbuffers is 0): with
 * T = span_bytes / 4096 + nbuffers tiles, 256 + 44 bytes per tile -- one 32-bit hash maximum per 64 input bytes, no hash word per byte -- and
 * 24 bytes per buffer, every piece rounded up to 256: span_bytes / 13.6 + 332 nbuffers and a few KiB, the same at every window.
 * How: frame_cuts.hip -- workgroups take tiles of 4096 positions; lanes hash runs of 17 positions with a 32-byte warm-up; a first pass keeps the
 * maximum of every block of 64 positions; a position that is the maximum of its own and the two neighbouring blocks is confirmed against the block
 * maxima its window covers whole and a re-hash of the two ragged ends; a count pass, scans and an emit pass follow.  The input is read once per
 * pass, three times in all (the emit pass skips the tiles without a cut).
 * Stream capture: the call only enqueues -- nothing is allocated, read back or synchronised.
 * SNP_ERR_BAD_ARG for a window or max_bytes outside the rule, nbuffers >= 2^30, or a null pointer (nbuffers == 0 needs only ctx and d_result: it
 * writes d_result, and cut_first[0] = 0 when cut_first is given); SNP_ERR_DEVICE for a runtime failure. */
uint64_t snp_content_cuts_workspace(uint32_t nbuffers, uint64_t span_bytes, uint32_t window);
snp_status snp_content_cuts_batch(snp_ctx* ctx, const uint8_t* in, const uint64_t* in_off, const uint64_t* in_len, uint32_t nbuffers,
                                  uint32_t window, uint32_t max_bytes, uint64_t span_bytes, uint64_t max_cuts, uint64_t* cut_first,
                                  uint64_t* cuts, int32_t* status, void* d_work, uint64_t* d_result);

/* snp_frame_encode_cuts_batch: snp_frame_encode_chunked_batch with the pieces given by the caller.  Buffers, outputs, the index arrays (all null or
 * all given) and d_result are those of that call (snappier_hip_frame_chunked.h).  Buffer b's cuts are cuts[cut_first[b] .. cut_first[b + 1])
 * (cut_first: nbuffers + 1 values, as the finder writes them), offsets relative to the buffer's first byte, and its chunks are the pieces between
 * them: cuts + 1 pieces for in_len > 0, none for an empty buffer.  Each piece becomes a chunk by the CompressBlock rule of that call, with the
 * same masked CRC and header; with an index there is one row per piece, idx_start = the piece's offset, idx_pos = the position of its header.
 * With cuts = k * chunk_bytes every output is that call's, byte for byte.
 * The cut list is untrusted: reads of `cuts` are bounded by ncuts.  A buffer whose cut_first decreases or passes ncuts, whose cuts are not
 * strictly ascending inside (0, in_len), or one of whose pieces exceeds 65536 bytes gets SNP_ERR_BAD_ARG: out_len = 0, its out range untouched, no
 * slot, no row (idx_total = 0, idx_tail = SNP_ERR_BAD_ARG); the other buffers are unaffected.  The verdict comes before admission: a bad list
 * counts nothing.
 * Admission is in buffer order, by max_chunks (pieces) and by stage_cap (the staging of the pieces, snp_max_compressed_length(piece) rounded up
 * to 16, plus 16, each -- no more than bytes + bytes / 6 + 69 * pieces for the whole batch, which is the bound to pass): the first good buffer
 * that misses one and every later good one get SNP_ERR_OUTPUT_TOO_SMALL, as does a buffer whose stream is larger than out_cap[b], alone.
 * d_work must hold snp_frame_encode_cuts_workspace(nbuffers, max_chunks, stage_cap) bytes (host arithmetic; 0 when nbuffers is 0): stage_cap,
 * 44 bytes per slot and the 64 bytes of staging a slot that stays empty may touch, 36 per buffer, every piece rounded up to 256.
 * Stream capture: the call only enqueues, under the rule of snp_frame_encode_buffers_batch (the same call once before the capture).
 * SNP_ERR_BAD_ARG for an index given in part or a null pointer (cuts may be null when ncuts is 0; nbuffers == 0 needs only ctx and d_result),
 * SNP_ERR_DEVICE for a runtime failure. */
uint64_t snp_frame_encode_cuts_workspace(uint32_t nbuffers, uint32_t max_chunks, uint64_t stage_cap);
snp_status snp_frame_encode_cuts_batch(snp_ctx* ctx, const uint8_t* in, const uint64_t* in_off, const uint64_t* in_len, uint32_t nbuffers,
                                       const uint64_t* cut_first, const uint64_t* cuts, uint64_t ncuts, uint32_t max_chunks,
                                       uint64_t stage_cap, uint8_t* out, const uint64_t* out_off, const uint64_t* out_cap, uint64_t* out_len,
                                       int32_t* status, uint64_t* idx_first, uint64_t* idx_start, uint64_t* idx_pos, uint64_t* idx_total,
                                       int32_t* idx_tail, void* d_work, uint64_t* d_result);

#ifdef __cplusplus
}
#endif
#endif /* SNAPPIER_HIP_FRAME_CUTS_H */

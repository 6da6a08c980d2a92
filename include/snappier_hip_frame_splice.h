/*
 * snappier_hip_frame_splice.h -- C-ABI of libsnappier_hip_frame_splice.so: device batch SPLICE (insert, delete, truncate, drop-prefix) of seekable
 * Snappy framed streams through their chunk index.  A stream that is kept in device memory with its index can be read in any window
 * (snp_frame_read_indexed_batch, snappier_hip_frame_index.h), patched byte for byte (snp_frame_write_indexed_batch, snappier_hip_frame_update.h)
 * and grown at its end (snp_frame_append_indexed_batch, snappier_hip_frame_append.h); every one of these leaves each decoded byte at the offset it
 * had.  This call makes the edits that CHANGE LENGTH: a record deleted, one inserted in the middle, one replaced by a longer or a shorter one, a
 * log cut off at a position, a prefix dropped.  Without it each of those costs a decode and an encode of the whole stream.
 *
 * An extension of include/snappier_hip.h in a library of its own, linked against libsnappier_hip.so and taking that library's contexts (snp_ctx).
 * It adds no status code and no option and keeps no state in the context; the surfaces of snappier_hip.h and the other extension headers are
 * unchanged.  The C# side binds these functions in csharp/Snappier.Gpu/NativeMethodsFrameSplice.cs.
 */
#ifndef SNAPPIER_HIP_FRAME_SPLICE_H
#define SNAPPIER_HIP_FRAME_SPLICE_H

#include "snappier_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Stream b is in[in_off[b] .. +in_len[b]), as the sibling calls take it; idx_first, idx_start, idx_pos, idx_total, idx_tail and nentries are its
 * batch's index as snappier_hip_frame_index.h describes it.  The call takes ONE splice per stream: in what stream b decodes to, the bytes
 * [sp_off[b], sp_off[b] + sp_del[b]) are replaced by src[src_off[b] .. +sp_ins[b]).  Insert is del = 0, delete is ins = 0, truncate is
 * del = idx_total[b] - off, drop-prefix is off = 0.  Several edits of one stream are several calls: the new index goes straight into the next
 * one, and no synchronisation is needed between them.  A SORTED REQUEST LIST WITH SEVERAL SPLICES PER STREAM IS DELIBERATELY NOT PART OF THIS
 * CALL: merging the rewritten regions of neighbouring requests would double the planning.  (snp_frame_edit_indexed_batch, snappier_hip_frame_edit.h, is that call.)
 * Out of place, like the update call: `in`, `src` and the old index are only read; the new stream of b goes to out[out_off[b] .. +out_cap[b]),
 * which must not overlap `in`.
 *
 * The new stream.  Let lo = sp_off, hi = lo + sp_del, and the stream's rows be [f0, f1) (clamped to nentries); a row ends where the next one
 * starts, the last one at idx_total.  The rows the splice OWNS, [r0, r1):
 *   del > 0:  r0 is the first row with end > lo, r1 the first row at or after r0 with start >= hi (the read call's rule).
 *   del == 0 and lo == total:  no row; the insertion point is in_len[b], behind the stream's last byte.
 *   del == 0 otherwise:  r0 is the first row with end > lo.  If start[r0] == lo the splice owns no row and the insertion point is pos[r0];
 *             else it owns row r0 alone, which is split.
 * Zero-length rows at the borders are never owned; zero-length rows strictly inside are owned and vanish.
 * The EDGES: H = the decoded bytes [start[r0], lo) of the head row when start[r0] < lo, T = [hi, end[r1 - 1]) of the tail row when its end is above
 * hi.  Both may be the same row; it is decoded once.  An edge's chunk is decoded and CRC-verified whole into staging, as an edge of
 * snp_frame_write_indexed_batch is; one that decodes to more than 65536 bytes gives SNP_ERR_BAD_ARG.
 * The HOLE: P0 = pos[r0] and P1 = pos[r1 - 1] + 4 + size (size: the length field of the header there); with no owned row P0 = P1 = the insertion
 * point.  EVERYTHING IN [P0, P1) IS REPLACED: SKIPPABLE, PADDING AND REPEATED-IDENTIFIER CHUNKS THAT LIE BETWEEN THE OWNED DATA CHUNKS ARE
 * DROPPED WITH THEM.  It is the one place in the seekable calls where non-data bytes are not copied.
 * The REGION: R = H || the source bytes || T, cut into pieces of chunk_bytes (1 .. 65536, one value for the call), the last one shorter; an empty R
 * gives no chunk.  Every piece is one slot of snp_frame_encode_chunked_batch: what CompressBlock makes of it with the context's hash variant --
 * type 0x00 with varint || fragment when that is smaller than the piece, else type 0x01 with the piece -- and the masked CRC-32C of the piece.
 * The new stream = in[0, P0) || (the 10-byte stream identifier iff in_len == 0) || the new chunks || in[P1, in_len); both copies are verbatim.
 * So, byte for byte:
 *   - for a stream that snp_frame_encode_chunked_batch wrote from a buffer A with chunk_bytes c, a splice with the same c that deletes to the
 *     end (del > 0, hi == total) leaves exactly that call's output for A[:lo] || INS; a pure truncate is the case of an empty INS.  (With
 *     del == 0 and lo == total nothing is deleted and no row is owned: the bytes go into fresh chunks behind a short tail, which only
 *     snp_frame_append_indexed_batch fills up);
 *   - a splice whose lo and hi are multiples of c and whose ins is a multiple of c (or hi == total) equals that call's output for the edited
 *     buffer;
 *   - any other splice decodes to the edited buffer and may leave short chunks in the middle.  Fragmentation after many edits is accepted:
 *     snp_frame_rechunk_indexed_batch (snappier_hip_frame_rechunk.h) brings a stream back to the chunked encoder's output.
 *
 * The new index.  new_first[nstreams + 1], new_total[nstreams] and new_tail[nstreams] are per stream; new_start and new_pos hold
 * nentries + max_slots rows each (both numbers are the host's, so the rows need no bound of their own).  For a written stream: its rows
 * [f0, r0) are copied; one row per new chunk follows, start = lo - |H| + k * chunk_bytes and pos where the chunk lies; then its rows [r1, f1)
 * with start + ins - del and pos + (new bytes - (P1 - P0)); new_total[b] = idx_total[b] - del + ins and new_tail[b] = SNP_OK.  A stream that is
 * not written keeps its old rows, total and tail.  When the old index is what snp_frame_index_batch gives, the new arrays are, array for
 * array, what it gives for the new streams (the old one where a stream is not written): they go straight into the read, update, append and
 * splice calls.  Rows at and above new_first[nstreams] are not written.
 *
 * Verdicts.  A stream is spliced whole or not at all: a stream that fails has out_len[b] = 0, its out range untouched and its old rows.
 * sp_del[b] == 0 and sp_ins[b] == 0: the stream is not named: SNP_OK, out_len[b] = 0, nothing written, nothing of the index looked at.
 * A stream whose idx_tail is not SNP_OK gets that status (SNP_ERR_OUTPUT_TOO_SMALL: not indexed; a walk error: the stream is broken); a value
 * that is no status of the walk gives SNP_ERR_BAD_ARG.  SNP_ERR_BAD_ARG too for lo + del wrapping or above idx_total[b], and for
 * idx_total[b] - del + ins wrapping.
 * THE INDEX IS UNTRUSTED INPUT, as in snp_frame_read_indexed_batch: index reads are bounded by nentries (idx_first values are clamped), and the
 * header at pos[r0] and at pos[r1 - 1] is ALWAYS read again inside in_len[b], whether the row is an edge or wholly deleted: each must be a data
 * chunk that decodes to exactly end - start bytes; when the two rows differ the second header lies at or after the end of the first chunk; and
 * P1 <= in_len[b].  An insertion point that is a row's position must be a data chunk's header inside the stream.  Bytes to delete and no row
 * that holds them, decoded bytes and no row at all, rows that run backwards, f1 < f0: SNP_ERR_BAD_ARG.  Whatever the arrays hold, nothing is
 * read outside a stream's bytes or its source, and nothing is written outside out[out_off[b] .. +out_cap[b]), the new index arrays and the
 * per-stream arrays; with an idx_first that claims more than nentries rows in all, the new rows are cut off at nentries + max_slots and
 * new_first stays at that.
 * Which old bytes are read.  The two headers above and the edges.  A CHUNK THAT IS WHOLLY DELETED IS NEVER DECODED: A CORRUPT ONE IS NOT
 * NOTICED, AND IT IS GONE.  A CORRUPT CHUNK OUTSIDE THE HOLE IS COPIED AS IT IS.  An edge that fails to decode or verify gives its stream the
 * chunk's status (the head edge's when both fail).
 * Admission, in stream order over the named streams that passed the checks above: the new chunks are counted against max_slots and the staging
 * bytes -- the decoded bytes of the edge chunks plus |R| -- against stage_cap, each with those of the streams before.  The first stream that
 * misses a bound, and every later named stream, get SNP_ERR_OUTPUT_TOO_SMALL; so does a stream whose new size exceeds out_cap[b] (this can hit
 * one stream in the middle of a batch; the others go on).
 * d_result (device, 4 x u64): [0] = slots needed (a stream that needs 2^32 or more, which no bound admits, counted as 2^32), [1] = sum of out_len
 * over the written streams, [2] = staging bytes needed (such a stream counted as 2^48 + 2^18), [3] = streams written.  max_slots = stage_cap = 0
 * is the sizing call.  out_bound (nullable, nstreams x u64): for a named stream that passed the checks, from the headers alone,
 * in_len - (P1 - P0) + sum(8 + piece) (+ 10 for an empty stream) -- it always holds the new stream; 0 for the others (also for a stream whose edge
 * failed to decode in this call; the sizing call decodes nothing).
 * d_work must hold snp_frame_splice_indexed_workspace(nstreams, max_slots, stage_cap, chunk_bytes) bytes (host arithmetic; 0 when nstreams is 0
 * or chunk_bytes is out of range): about 270 bytes per stream, 45 per slot, stage_cap of staging and snp_max_compressed_length(chunk_bytes) + 32
 * of compressed staging per slot.  All arrays are device memory.
 * Stream capture: the call only enqueues on the context's stream -- no allocation, no read-back, no synchronisation -- under the rule of
 * snp_frame_encode_buffers_batch: make the same call, with the same max_slots, once before the capture.
 * How: frame_splice.hip -- a plan per stream, scans, ONE decode over an edge table of 2 x nstreams rows, an assemble kernel that puts H, the
 * source bytes and T one behind the other in staging (the inserted bytes are copied once, so that one launch serves every piece), ONE compressor
 * and ONE CRC launch over all pieces, an emit whose workgroups each take 64 KiB of an old stream's kept bytes or the new chunks of 64 KiB of a
 * region, and a merge of the index rows.
 * SNP_ERR_BAD_ARG for chunk_bytes of 0 or above 65536, for nstreams >= 2^31 and for a null pointer (nstreams == 0 needs only ctx and d_result:
 * it writes a zeroed d_result and nothing else; out_bound is optional, idx_start / idx_pos when nentries > 0, new_start / new_pos when
 * nentries + max_slots > 0), SNP_ERR_DEVICE for a runtime failure. */
uint64_t snp_frame_splice_indexed_workspace(uint32_t nstreams, uint32_t max_slots, uint64_t stage_cap, uint32_t chunk_bytes);
snp_status snp_frame_splice_indexed_batch(snp_ctx* ctx, const uint8_t* in, const uint64_t* in_off, const uint64_t* in_len, uint32_t nstreams,
                                          const uint64_t* idx_first, const uint64_t* idx_start, const uint64_t* idx_pos,
                                          const uint64_t* idx_total, const int32_t* idx_tail, uint64_t nentries,
                                          const uint8_t* src, const uint64_t* sp_off, const uint64_t* sp_del, const uint64_t* sp_ins,
                                          const uint64_t* src_off, uint32_t chunk_bytes, uint32_t max_slots, uint64_t stage_cap,
                                          uint8_t* out, const uint64_t* out_off, const uint64_t* out_cap, uint64_t* out_len, int32_t* status,
                                          uint64_t* new_first, uint64_t* new_start, uint64_t* new_pos, uint64_t* new_total, int32_t* new_tail,
                                          uint64_t* out_bound, void* d_work, uint64_t* d_result);

#ifdef __cplusplus
}
#endif
#endif /* SNAPPIER_HIP_FRAME_SPLICE_H */

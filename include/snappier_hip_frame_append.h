/*
 * snappier_hip_frame_append.h -- C-ABI of libsnappier_hip_frame_append.so: device batch APPEND to seekable Snappy framed streams, in place, through
 * their chunk index.  snp_frame_read_indexed_batch (snappier_hip_frame_index.h) reads any window of a stream that is kept in device memory with
 * its index and snp_frame_write_indexed_batch (snappier_hip_frame_update.h) replaces decoded bytes of it, but neither changes a stream's length;
 * this call makes such streams GROW: bytes appended to what each decodes to, written behind it in the region it is kept in, with the new index.
 * Without it appended bytes cost a decode and an encode of their whole stream.
 *
 * An extension of include/snappier_hip.h in a library of its own, linked against libsnappier_hip.so and taking that library's contexts (snp_ctx).
 * It adds no status code and no option and keeps no state in the context; the surfaces of snappier_hip.h and the other extension headers are
 * unchanged.  The C# side binds these functions in csharp/Snappier.Gpu/NativeMethodsFrameAppend.cs.
 */
#ifndef SNAPPIER_HIP_FRAME_APPEND_H
#define SNAPPIER_HIP_FRAME_APPEND_H

#include "snappier_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Stream b is buf[buf_off[b] .. +buf_len[b]), inside a region buf[buf_off[b] .. +buf_cap[b]) that is the caller's to grow into; idx_first,
 * idx_start, idx_pos, idx_total, idx_tail and nentries are the batch's index as snappier_hip_frame_index.h describes it.
 * src[src_off[b] .. +src_len[b]) is appended to what stream b decodes to, in chunks of chunk_bytes (1 .. 65536, one value for the call).
 * THE REGIONS MUST BE PAIRWISE DISJOINT, AND src AND THE NEW INDEX ARRAYS MUST OVERLAP NOTHING ELSE: that is the caller's duty, the call does not
 * check it.  `src` and the old index are only read.
 *
 * In place.  Nothing before the CUT of a stream is written, and nothing at or after buf_off[b] + buf_cap[b]; what a call costs follows the
 * appended bytes plus at most one chunk per stream, not the streams' sizes.  Let L be the stream's last index row and
 * d = idx_total[b] - idx_start[L].  The tail chunk is REOPENED iff the stream has rows, 0 < d < chunk_bytes, and the chunk at idx_pos[L] ends
 * exactly at buf_len[b] (pos + 4 + size == buf_len[b]; size: the length field of its header).  A reopened tail is decoded and CRC-verified
 * whole into staging, as an edge of snp_frame_write_indexed_batch is, filled up with the first min(src_len, chunk_bytes - d) appended bytes and
 * encoded again at idx_pos[L]: that position is the cut.  Otherwise the cut is buf_len[b] -- a zero-length tail chunk, a tail of chunk_bytes or
 * more bytes (a stream written with larger chunks), a tail followed by padding or skippable chunks: all of them stay as they are.  The rest of
 * the appended bytes follows in chunks of chunk_bytes, the last one shorter.  Every chunk is one slot of snp_frame_encode_chunked_batch: what
 * CompressBlock makes of the piece with the context's hash variant -- type 0x00 with varint || fragment when that is smaller than the piece, else
 * type 0x01 with the piece -- and the masked CRC-32C of the piece.  A stream of buf_len 0 gets the 10-byte stream identifier first.  So for a
 * stream that snp_frame_encode_chunked_batch wrote from a buffer A with chunk_bytes c, appending S with the same c leaves exactly that call's
 * output for A || S, byte for byte, and any sequence of appends leaves its output for the concatenation.
 *
 * Which old bytes are read.  The header of the last row's chunk, and the chunk itself when it is reopened.  A REOPENED TAIL THAT FAILS TO DECODE
 * OR VERIFY GIVES ITS STREAM THE CHUNK'S STATUS.  NOTHING BEFORE THE CUT IS LOOKED AT: A CORRUPT CHUNK THERE IS NOT NOTICED, AND IT STAYS AS IT IS.
 *
 * The new index.  new_first[nstreams + 1], new_total[nstreams] and new_tail[nstreams] are per stream; new_start and new_pos hold
 * nentries + max_slots rows each (both numbers are the host's, so the rows need no bound of their own).  Every stream's old rows are copied --
 * old positions never move, a reopened tail keeps its position -- and the rows of a written stream's fresh chunks follow them:
 * start = idx_total[b] + fill + k * chunk_bytes, pos relative to the stream's first byte.  new_total[b] = idx_total[b] + src_len[b] and
 * new_tail[b] = SNP_OK for a written stream; a stream that is not written keeps its old rows, total and tail.  When the old index is what
 * snp_frame_index_batch gives, the new arrays are, array for array, what it gives for the batch after the call: they go straight into the read,
 * update and append calls.  Rows at and above new_first[nstreams] are not written.
 *
 * Verdicts.  src_len[b] == 0: SNP_OK, new_len[b] = buf_len[b], nothing touched.  A stream whose idx_tail is not SNP_OK gets that status
 * (SNP_ERR_OUTPUT_TOO_SMALL: not indexed; a walk error: the stream is broken, and a broken stream is not appended to); a value that is no
 * status of the walk gives SNP_ERR_BAD_ARG.  THE INDEX IS UNTRUSTED INPUT, as in snp_frame_read_indexed_batch: index reads are bounded by nentries
 * (idx_first values are clamped), and when the stream has rows the header at idx_pos[L] is read again inside buf_len[b] and must be a data chunk
 * that decodes to exactly d bytes (a reopened one to at most 65536); rows that run backwards, idx_start[L] above idx_total[b], decoded bytes and
 * no row, or idx_total[b] + src_len[b] wrapping: anything else gives SNP_ERR_BAD_ARG.  Whatever the five arrays hold, nothing is read outside
 * a stream's bytes or its source, and nothing is written outside [cut, buf_cap[b]) of a stream, the new index arrays and the per-stream arrays;
 * with an idx_first that claims more than nentries rows in all, the new rows are cut off at nentries + max_slots and new_first stays at that.
 * Admission, in stream order over the streams that passed the checks above with bytes to take: reopened tails are counted against max_tails and
 * fresh chunk slots against max_slots (the tail's own slot not included), each with those of the streams before it.  The first stream that
 * misses a bound, and every later such stream, get SNP_ERR_OUTPUT_TOO_SMALL; so does a stream whose new size exceeds buf_cap[b] (this can hit
 * one stream in the middle of a batch; the others go on).  A stream that is not written has new_len[b] = buf_len[b] and not one byte changed:
 * it is appended to whole or not at all.
 * out_bound (nullable, nstreams x u64): for a stream that passed the checks, from the headers alone,
 * buf_len - (reopened ? 4 + size : 0) + sum(8 + piece) (+ 10 for an empty stream) -- it always holds the new stream; buf_len[b] for the others
 * (also for a stream whose tail failed to decode in this call; the sizing call decodes nothing).
 * d_result (device, 4 x u64): [0] = fresh slots needed (a stream that needs 2^32 or more, which no bound admits, counted as 2^32), [1] = sum of
 * new_len - buf_len over the written streams (modulo 2^64: a tail that a foreign writer stored loosely may shrink), [2] = tails needed,
 * [3] = streams written.  max_tails = max_slots = 0 is the sizing call.
 * d_work must hold snp_frame_append_indexed_workspace(nstreams, max_tails, max_slots, chunk_bytes) bytes (host arithmetic; 0 when nstreams is 0 or
 * chunk_bytes is out of range): about 110 bytes per stream, 80 per tail slot and 45 per fresh slot, chunk_bytes of raw staging per tail and
 * snp_max_compressed_length(chunk_bytes) + 32 of compressed staging per slot of either table.  All arrays are device memory.
 * Stream capture: the call only enqueues on the context's stream -- no allocation, no read-back, no synchronisation -- under the rule of
 * snp_frame_encode_buffers_batch: make the same call, with the same max_tails and max_slots, once before the capture.
 * How: frame_append.hip -- a plan per stream, scans, ONE decode over the reopened tails, an overlay of the fill bytes, a compressor and a CRC
 * launch over the tail table (from staging) and over the fresh table (straight from src), and an emit whose workgroups each take the slots of 64 KiB
 * of appended input.
 * SNP_ERR_BAD_ARG for chunk_bytes of 0 or above 65536 and for a null pointer (nstreams == 0 needs only ctx and d_result: it writes a zeroed
 * d_result and nothing else; out_bound is optional, idx_start / idx_pos when nentries > 0, new_start / new_pos when nentries + max_slots > 0),
 * SNP_ERR_DEVICE for a runtime failure. */
uint64_t snp_frame_append_indexed_workspace(uint32_t nstreams, uint32_t max_tails, uint32_t max_slots, uint32_t chunk_bytes);
snp_status snp_frame_append_indexed_batch(snp_ctx* ctx, uint8_t* buf, const uint64_t* buf_off, const uint64_t* buf_len, const uint64_t* buf_cap,
                                          uint32_t nstreams,
                                          const uint64_t* idx_first, const uint64_t* idx_start, const uint64_t* idx_pos,
                                          const uint64_t* idx_total, const int32_t* idx_tail, uint64_t nentries,
                                          const uint8_t* src, const uint64_t* src_off, const uint64_t* src_len,
                                          uint32_t chunk_bytes, uint32_t max_tails, uint32_t max_slots,
                                          uint64_t* new_len, int32_t* status,
                                          uint64_t* new_first, uint64_t* new_start, uint64_t* new_pos, uint64_t* new_total, int32_t* new_tail,
                                          uint64_t* out_bound, void* d_work, uint64_t* d_result);

#ifdef __cplusplus
}
#endif
#endif /* SNAPPIER_HIP_FRAME_APPEND_H */

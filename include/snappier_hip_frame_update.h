/*
 * snappier_hip_frame_update.h -- C-ABI of libsnappier_hip_frame_update.so: device batch UPDATE of seekable Snappy framed streams through their
 * chunk index.  snp_frame_read_indexed_batch (snappier_hip_frame_index.h) reads any window of a stream that is kept in device memory with its
 * index; this is its write half: requests that replace decoded bytes, answered by new streams in which only the chunks the requests touch
 * are compressed again and every other byte is a copy.  Without it a changed record costs a decode and an encode of its whole stream.
 *
 * An extension of include/snappier_hip.h in a library of its own, linked against libsnappier_hip.so and taking that library's contexts (snp_ctx).
 * It adds no status code and no option and keeps no state in the context; the surfaces of snappier_hip.h and the other extension headers are
 * unchanged.  The C# side binds these functions in csharp/Snappier.Gpu/NativeMethodsFrameUpdate.cs.
 */
#ifndef SNAPPIER_HIP_FRAME_UPDATE_H
#define SNAPPIER_HIP_FRAME_UPDATE_H

#include "snappier_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Stream b is in[in_off[b] .. +in_len[b]), as the sibling calls take it; idx_first, idx_start, idx_pos, idx_total, idx_tail and nentries are its
 * batch's index as snappier_hip_frame_index.h describes it.  Request r replaces the decoded bytes [req_off[r], req_off[r] + req_len[r]) of stream
 * req_stream[r] by src[src_off[r] .. +req_len[r]).  `in`, `src` and the index are only read; the new stream of b goes to
 * out[out_off[b] .. +out_cap[b]), which must not overlap `in`.
 *
 * The new stream.  A chunk is DIRTY when a request writes at least one byte of what it decodes to.  The new stream is the old one with the bytes
 * [pos, pos + 4 + size) of every dirty chunk (size: the length field of its header) replaced by a new chunk; every other byte -- the identifier, repeated identifiers, skippable
 * and padding chunks, clean data chunks, zero-length chunks, trailing bytes -- is copied verbatim and in order.  The new chunk is what
 * CompressBlock makes of the chunk's new decoded bytes with the context's hash variant: type 0x00 with varint || fragment when that is smaller
 * than the piece, else type 0x01 with the piece, and the masked CRC-32C of the piece -- exactly one slot of snp_frame_encode_chunked_batch.  So
 * for a stream that call wrote from a buffer A, the update equals that call's output for the patched A, byte for byte.  The decoded length, the
 * rows and every idx_start are unchanged: idx_first, idx_start, idx_total and idx_tail stay valid, only positions move.  new_pos (nullable,
 * nentries x u64) receives idx_pos of the new streams: new_pos[i] = idx_pos[i] + the size change of the dirty chunks of its stream before row i
 * (= idx_pos[i] for a row of a stream that is not written); with it in place of idx_pos the index is, array for array, what
 * snp_frame_index_batch gives for the new streams.
 *
 * A stream is updated whole or not at all.  A stream that no request names is left alone: status[b] = SNP_OK, out_len[b] = 0, nothing written.
 * A named stream is written whole (also when its requests are all empty: a copy), or, when anything fails, gets the status of its FIRST failing
 * request, out_len[b] = 0, its out range untouched and its new_pos rows = idx_pos; the other streams are unaffected.  req_status[r] is the
 * request's own failure, else its stream's status: SNP_OK means its bytes are in the new stream.
 *
 * Requests must be sorted by (req_stream, req_off) and byte-disjoint: the previous request of the same stream must end at or before req_off.
 * SNP_ERR_BAD_ARG for a request that is out of order with, or overlaps, its predecessor, or that does not lie among the requests of its stream
 * where a binary search of req_stream looks for them (in a sorted list every request does); for req_stream >= nstreams; for req_off + req_len
 * above idx_total[b] or wrapping (this call never changes a stream's length); for a dirty chunk that decodes to more than 65536 bytes (legal to
 * read, not something one chunk may be re-encoded as).  A stream whose idx_tail is not SNP_OK gives its requests that status
 * (SNP_ERR_OUTPUT_TOO_SMALL: not indexed; a walk error: the stream is broken); a value that is no status of the walk gives SNP_ERR_BAD_ARG.
 * A zero-length request in range is OK and dirties nothing.  Several requests may lie in one chunk, and the tail chunk of one may be the head
 * chunk of the next: such a chunk is re-encoded once.
 *
 * Which old bytes are read.  A dirty chunk that one request covers entirely is NOT DECODED: ITS OLD PAYLOAD AND CRC ARE NEVER LOOKED AT, SO A
 * CORRUPT CHUNK THAT IS WHOLLY REPLACED IS NOT NOTICED -- IT IS REPAIRED BY THE WRITE.  Every other dirty chunk (an edge) is decoded and
 * CRC-verified whole into staging; if that fails, the request that dirtied it first gets the chunk's status and the stream is not written.
 * A CORRUPT CHUNK THAT NO REQUEST TOUCHES IS COPIED AS IT IS.
 *
 * THE INDEX IS UNTRUSTED INPUT, as in snp_frame_read_indexed_batch: index reads are bounded by nentries (idx_first values are clamped), every
 * dirty row has its header read again at idx_pos inside in_len[b] and must be a data chunk that decodes to exactly end - start bytes, a wholly
 * covered row must lie inside the request, and the dirty rows of a stream must be strictly increasing with the header of each at or after the
 * end of the chunk of the one before it (two rows at one header would corrupt the copy).  Anything else gives SNP_ERR_BAD_ARG for the request
 * that owns the row.  Whatever the five arrays and the request list hold, nothing is read outside a stream's bytes or a request's source, and
 * nothing is written outside [out_off[b], out_off[b] + out_cap[b]), new_pos[0 .. nentries) and the per-stream and per-request arrays.
 *
 * Admission, in stream order over the streams whose requests all passed the checks above: a stream's dirty slots (one per dirty row; a
 * zero-length chunk inside a request takes a slot although it stays as it is) must fit max_slots and their decoded bytes stage_cap, each counted
 * with those of the streams before it.  The first stream that misses a bound, and every later such stream, get SNP_ERR_OUTPUT_TOO_SMALL; so does
 * a stream whose new size exceeds out_cap[b] (this can hit one stream in the middle of a batch; the others go on).
 * d_result (device, 4 x u64): [0] = dirty slots needed, [1] = sum of out_len over the written streams, [2] = staging bytes needed, [3] = streams
 * written.  max_slots = stage_cap = 0 is the sizing call.  out_bound (nullable, nstreams x u64): for every named stream that passed the checks,
 * in_len[b] - sum(4 + size) + sum(8 + dec) over its dirty chunks, from the headers alone -- it always holds the new stream; 0 for the others (also
 * for a stream whose edge failed to decode in this call; the sizing call decodes nothing).
 * d_work must hold snp_frame_write_indexed_workspace(nstreams, nreq, max_slots, stage_cap) bytes (host arithmetic; 0 when nreq is 0): about 100
 * bytes per slot, request and stream, and 2.2 x stage_cap + 160 x max_slots of staging.  All arrays are device memory.
 * Stream capture: the call only enqueues on the context's stream -- no allocation, no read-back, no synchronisation -- under the rule of
 * snp_frame_encode_buffers_batch: make the same call, with the same max_slots, once before the capture.
 * How: frame_update.hip -- a plan per request, scans, a check per dirty row, ONE decode over the edge slots, an overlay of the requests' bytes,
 * ONE compressor launch and ONE CRC launch over all dirty slots, and an emit whose workgroups each take 64 KiB of an old stream.
 * SNP_ERR_BAD_ARG for a null pointer (nreq == 0 or nstreams == 0 needs only ctx and d_result: it writes a zeroed d_result and nothing else) and
 * for nreq >= 2^31, SNP_ERR_DEVICE for a runtime failure. */
uint64_t snp_frame_write_indexed_workspace(uint32_t nstreams, uint32_t nreq, uint32_t max_slots, uint64_t stage_cap);
snp_status snp_frame_write_indexed_batch(snp_ctx* ctx, const uint8_t* in, const uint64_t* in_off, const uint64_t* in_len, uint32_t nstreams,
                                         const uint64_t* idx_first, const uint64_t* idx_start, const uint64_t* idx_pos,
                                         const uint64_t* idx_total, const int32_t* idx_tail, uint64_t nentries,
                                         const uint8_t* src, const uint32_t* req_stream, const uint64_t* req_off, const uint64_t* req_len,
                                         const uint64_t* src_off, uint32_t nreq, uint32_t max_slots, uint64_t stage_cap, uint8_t* out,
                                         const uint64_t* out_off, const uint64_t* out_cap, uint64_t* out_len, int32_t* status,
                                         int32_t* req_status, uint64_t* new_pos, uint64_t* out_bound, void* d_work, uint64_t* d_result);

#ifdef __cplusplus
}
#endif
#endif /* SNAPPIER_HIP_FRAME_UPDATE_H */

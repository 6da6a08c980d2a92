/*
 * snappier_hip_frame_index.h -- C-ABI of libsnappier_hip_frame_index.so: a device SEEK INDEX for Snappy framed streams and INDEXED window reads.
 * snp_frame_decode_range_batch (snappier_hip_frame_range.h) walks every stream's headers from byte 0 in every call and takes one window per
 * stream.  Here the streams are walked ONCE into a small chunk index that the caller keeps in device memory (16 bytes per data chunk); any number
 * of windows, each naming a stream, is then read in one call with no header walk: two binary searches per request and one thread per chunk.
 *
 * An extension of include/snappier_hip.h in a library of its own, linked against libsnappier_hip.so and taking that library's contexts (snp_ctx).
 * It adds no status code and no option and keeps no state in the context; the surfaces of snappier_hip.h and the other extension headers are
 * unchanged.  The C# side binds these functions in csharp/Snappier.Gpu/NativeMethodsFrameIndex.cs.
 */
#ifndef SNAPPIER_HIP_FRAME_INDEX_H
#define SNAPPIER_HIP_FRAME_INDEX_H

#include "snappier_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The index of a batch: five caller-owned device arrays.  Stream b is in[in_off[b] .. +in_len[b]), as the sibling calls take it.
 * Per stream: idx_first[nstreams + 1] (u64) = the stream's first row; idx_total[nstreams] (u64) and idx_tail[nstreams] (i32) = the decoded_len and
 * the status that snp_frame_decode_layout_batch gives for the stream (its walk's total, and the error that ended the walk or SNP_OK).
 * Per row: idx_start[max_entries] (u64) = decoded bytes of the stream before the chunk; idx_pos[max_entries] (u64) = position of the chunk's
 * 4-byte header RELATIVE TO THE STREAM'S FIRST BYTE, not to `in`.  Stream b has one row for every data chunk its walk lists, zero-length ones
 * included, in stream order -- as many as nchunks[b] of the layout call; starts are non-decreasing.  Positions being stream-relative, an index
 * stays valid when the framed bytes move: with another in_off, another tensor, or stored and loaded again.
 * Admission, in stream order: a stream's spans (ceil(in_len / 2^20)) must fit max_spans and its rows must fit max_entries, each counted with
 * those of the streams before it.  The first stream that misses a bound, and every later one, get idx_tail = SNP_ERR_OUTPUT_TOO_SMALL,
 * idx_total = 0 and no rows (idx_first[b + 1] == idx_first[b]).  A stream whose spans do not fit is not walked.
 * d_result (device, 4 x u64): [0] = rows the walked streams need, [1] = sum of idx_total over the indexed streams, [2] = span slots the batch
 * needs, [3] = spans the resolver walked on the spot.  max_entries = 0 is the sizing call (idx_start and idx_pos may then be null).
 * d_work must hold snp_frame_index_workspace(nstreams, max_spans) bytes (host arithmetic; 0 when nstreams is 0).
 * How: the span scan, walk A and walk B of snp_frame_decode_buffers_batch with no capacity bound, two scans, and one wavefront per span slot
 * that hops through the span's headers and writes a row per data chunk (frame_index.hip).  Capturable like snp_frame_read_indexed_batch.
 * SNP_ERR_BAD_ARG for a null pointer (nstreams == 0 needs only ctx and d_result, and still writes d_result), SNP_ERR_DEVICE for a runtime failure. */
uint64_t snp_frame_index_workspace(uint32_t nstreams, uint32_t max_spans);
snp_status snp_frame_index_batch(snp_ctx* ctx, const uint8_t* in, const uint64_t* in_off, const uint64_t* in_len, uint32_t nstreams,
                                 uint32_t max_spans, uint64_t max_entries, uint64_t* idx_first, uint64_t* idx_start, uint64_t* idx_pos,
                                 uint64_t* idx_total, int32_t* idx_tail, void* d_work, uint64_t* d_result);

/* nreq requests, independent of each other: request r reads bytes [req_off[r], req_off[r] + req_len[r]) of what stream req_stream[r] decodes to
 * into out[out_off[r] .. +out_cap[r]).  Any number of requests may name the same stream, in any order; two requests that meet the same chunk
 * decode it twice.  nentries = the rows the index arrays hold (idx_first[nstreams] of the index call, or more).
 *
 * Contract.  For a request whose stream b was indexed, status[r], out_len[r] and the bytes at out[out_off[r] ..) are exactly what
 * snp_frame_decode_range_batch gives for stream b alone with the window (req_off[r], req_len[r]), the capacity out_cap[r] and bounds that admit
 * it: the clipping, the selection rule, interior and edge chunks, the status precedence, the strict tail rule (idx_tail[b] is the walk's tail)
 * and "a window that does not fit out_cap selects nothing" carry over unchanged.  Edges are decoded and verified whole into the scratch arena
 * inside d_work, then trimmed into `out`.  A CORRUPT CHUNK OUTSIDE THE WINDOW IS NOT NOTICED.  A request with req_stream[r] >= nstreams gets
 * SNP_ERR_BAD_ARG; one on a stream whose idx_tail is SNP_ERR_OUTPUT_TOO_SMALL (not indexed) gets that status.
 *
 * Selection without a walk.  With end[i] = start[i + 1], or idx_total[b] for the stream's last row: i0 = the first row with end > lo, i1 = the
 * first row with start >= hi; the request owns rows [i0, i1).  Row i0 is the head edge iff start[i0] < lo; row i1 - 1 is the tail edge iff its
 * end > hi and it is not already the head; every other row is an interior slot, decoded straight to out_off[r] + (start - lo).  A zero-length
 * row inside the range keeps its slot, empty: it is never decoded or verified, as the range call never selects it.
 *
 * THE INDEX IS UNTRUSTED INPUT.  Index reads are bounded by nentries (idx_first values are clamped to it).  Every row a request uses has its
 * header read again at idx_pos, inside in_len[b]: it must be a data chunk that decodes to exactly end - start bytes, and an interior row must lie
 * inside [lo, hi); the owned rows must hold the window, and idx_tail must be a status of the walk.  A request that fails any of this gets
 * SNP_ERR_BAD_ARG and nothing of it is decoded.  So a stale index, one built from other bytes or one filled with anything at all gives a
 * per-request status: nothing is ever written outside [out_off[r], out_off[r] + out_cap[r]) or read outside a stream's bytes.  body_len, crc
 * and type come from the header, not from the index.  (A request refused by its window or its edge rows takes no slot and no scratch; one
 * refused by an interior row had its slots counted.)
 *
 * Admission, in request order: a request's interior slots must fit max_chunks and the decoded bytes of its edges must fit edge_cap, each counted
 * with those of the requests before it.  The first request that misses a bound, and every later one, get SNP_ERR_OUTPUT_TOO_SMALL with out_len 0.
 * d_result (device, 4 x u64): [0] = interior slots needed, [1] = sum of out_len over the OK requests, [2] = edge scratch bytes needed, [3] =
 * requests that are OK.  max_chunks = edge_cap = 0 is the sizing call.
 * d_work must hold snp_frame_read_indexed_workspace(nreq, max_chunks, edge_cap) bytes (host arithmetic; 0 when nreq is 0).  nreq must be below
 * 2^30 (two edge slots per request, one workgroup each), else SNP_ERR_BAD_ARG.  All arrays are device memory; the call only reads `in` and the index.
 * Stream capture: the call only enqueues on the context's stream -- no allocation, no read-back, no synchronisation -- under the rule of
 * snp_decompress_batch: make the same call once before the capture.  No option changes a result.
 * SNP_ERR_BAD_ARG for a null pointer (nreq == 0 needs only ctx and d_result, and still writes d_result), SNP_ERR_DEVICE for a runtime failure. */
uint64_t snp_frame_read_indexed_workspace(uint32_t nreq, uint32_t max_chunks, uint64_t edge_cap);
snp_status snp_frame_read_indexed_batch(snp_ctx* ctx, const uint8_t* in, const uint64_t* in_off, const uint64_t* in_len, uint32_t nstreams,
                                        const uint64_t* idx_first, const uint64_t* idx_start, const uint64_t* idx_pos,
                                        const uint64_t* idx_total, const int32_t* idx_tail, uint64_t nentries,
                                        const uint32_t* req_stream, const uint64_t* req_off, const uint64_t* req_len, uint32_t nreq,
                                        uint32_t max_chunks, uint64_t edge_cap, uint8_t* out, const uint64_t* out_off,
                                        const uint64_t* out_cap, uint64_t* out_len, int32_t* status, void* d_work, uint64_t* d_result);

#ifdef __cplusplus
}
#endif
#endif /* SNAPPIER_HIP_FRAME_INDEX_H */

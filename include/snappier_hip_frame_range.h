/*
 * snappier_hip_frame_range.h -- C-ABI of libsnappier_hip_frame_range.so: device batch RANGE decode of many Snappy framed streams: a window of
 * decoded bytes out of every stream, decoding only the chunks that meet it.  Every data chunk of the framing format is an independent Snappy
 * block with its own CRC, so a stream allows random access at chunk granularity with no format change and no side index; this call reads streams
 * that any Snappy framing writer produced.  The range counterpart of snp_frame_decode_buffers_batch (snappier_hip_frame_buffers.h).
 *
 * An extension of include/snappier_hip.h in a library of its own, linked against libsnappier_hip.so and taking that library's contexts (snp_ctx).
 * It adds no status code and no option; the surfaces of snappier_hip.h and the other extension headers are unchanged.  The C# side binds these
 * functions in csharp/Snappier.Gpu/NativeMethodsFrameRange.cs.
 */
#ifndef SNAPPIER_HIP_FRAME_RANGE_H
#define SNAPPIER_HIP_FRAME_RANGE_H

#include "snappier_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Stream b is in[in_off[b] .. +in_len[b]) (u64 lengths, as snp_frame_decode_buffers_batch takes them); bytes [lo, hi) of what it decodes to are
 * written at out[out_off[b] ..), when they fit in out_cap[b] bytes.
 *
 * Window and selection.  Stream b's headers are walked over its whole length with no capacity bound, as snp_frame_decode_layout_batch walks them:
 * `total` = the decoded bytes the walk lists, `tail` = the error that ended the walk, or SNP_OK.  lo = min(range_off[b], total), hi =
 * min(range_off[b] + range_len[b], total), the sum saturating at UINT64_MAX: a window past the end is clipped, like a read; it is no error.  A data
 * chunk whose decoded bytes are [s, s + d) of the stream is SELECTED iff d > 0 && s < hi && s + d > lo (so an empty window that lies strictly
 * inside a chunk selects that chunk, and one on a chunk boundary selects none).  The selected chunks are contiguous in chunk order.  A selected
 * chunk with s >= lo && s + d <= hi is INTERIOR and is decoded straight to its place in `out`; any other selected chunk is an EDGE: at most two per
 * stream (one chunk can be both ends).  An edge is decoded WHOLE into a scratch arena inside d_work and verified whole -- the CRC covers the whole
 * chunk -- and then only its part inside the window is copied to `out`.
 *
 * Verification and status.  Only selected chunks are decoded and CRC-verified: A CORRUPT CHUNK OUTSIDE THE WINDOW IS NOT NOTICED.  status[b], in
 * order of precedence: the status of the first failing selected chunk in stream order (the decoder's own error, else SNP_ERR_CRC_MISMATCH), else
 * `tail`, else SNP_ERR_OUTPUT_TOO_SMALL if hi - lo > out_cap[b], else SNP_OK.  The tail rule is STRICT on purpose: a stream whose walk ends in an
 * error (SNP_ERR_TRUNCATED_STREAM, SNP_ERR_BAD_LENGTH, SNP_ERR_INCOMPLETE, SNP_ERR_CHUNK_TYPE) is not OK even when the window lies before the
 * damage, so status[b] is never OK where snp_frame_decode_layout_batch reports an error for the stream.  A stream with hi - lo > out_cap[b] selects
 * no chunk: nothing of it is decoded, so no chunk of it can fail, and it takes no chunk slot and no scratch.
 * out_len[b] = hi - lo when status[b] is SNP_OK, else 0.  An OK stream's out[out_off[b] .. +out_len[b]) equals bytes [lo, hi) of what
 * snp_frame_decode_device gives for the stream alone.  A stream that is not OK may have had its own range written (contents unspecified); nothing
 * outside [out_off[b], out_off[b] + out_cap[b]) is ever written, by an edge chunk in particular.  The call only reads `in`: input ranges may overlap.
 *
 * Admission, in stream order, like the sibling calls: a stream is admitted only if its spans fit in max_spans (ceil(in_len / 2^20) spans, the
 * rule of snp_frame_decode_buffers_batch: a stream whose spans do not fit is not walked), its interior chunks fit in max_chunks, and the decoded
 * bytes of its edge chunks fit in edge_cap, each counted together with those of the streams before it.  The first stream that misses any bound
 * gets SNP_ERR_OUTPUT_TOO_SMALL with out_len 0, and so does every later stream.  The decoded size of a chunk of a foreign stream is not bounded by
 * 65536 (only by 2^31 - 1), which is why the edge scratch is an arena counted in bytes.  To size a call: grow max_spans to d_result[2] first, then
 * max_chunks to d_result[0] and edge_cap to d_result[4]; a call with max_chunks = 0 and edge_cap = 0 walks, selects and decodes nothing.
 * d_result (device, 6 x u64): [0] = interior chunk slots the walked streams need, [1] = sum of out_len over the OK streams, [2] = span slots the
 * batch needs, [3] = spans whose true entry was not among their candidates (as d_result[3] of snp_frame_decode_buffers_batch), [4] = edge scratch
 * bytes the walked streams need, [5] = selected chunks of the walked streams, interior plus edge.
 * d_work must hold snp_frame_decode_range_workspace(nstreams, max_chunks, max_spans, edge_cap) bytes (host arithmetic; 0 when nstreams is 0):
 * edge_cap bytes of scratch, ~41 B per chunk slot, ~148 B per span slot, ~220 B per stream.  All arrays are device memory.  nstreams must be
 * below 2^30 (two edge slots per stream, one workgroup each), else SNP_ERR_BAD_ARG.
 * Stream capture: the call only enqueues on the context's stream -- no allocation, no read-back, no synchronisation -- under the rule of
 * snp_decompress_batch: make the same call once before the capture.  No option changes a result.
 * How: the span scan, walk A and walk B of snp_frame_decode_buffers_batch -- the same kernels, with no capacity bound -- then, per span slot, a
 * wavefront that hops through the span's chunk headers ONLY IF the span's decoded bytes meet the window (a narrow window in a long stream costs
 * the walk and two spans' hops); scans that place the interior rows and the edges; one decode and one CRC launch over the interior table into
 * `out` and one of each over the edge table into scratch; a copy of one workgroup per edge; the verdict (frame_range.hip).
 * SNP_ERR_BAD_ARG for a null pointer (nstreams == 0 needs only ctx and d_result, and still writes d_result), SNP_ERR_DEVICE for a runtime failure. */
uint64_t snp_frame_decode_range_workspace(uint32_t nstreams, uint32_t max_chunks, uint32_t max_spans, uint64_t edge_cap);
snp_status snp_frame_decode_range_batch(snp_ctx* ctx, const uint8_t* in, const uint64_t* in_off, const uint64_t* in_len,
                                        uint32_t nstreams, const uint64_t* range_off, const uint64_t* range_len,
                                        uint32_t max_chunks, uint32_t max_spans, uint64_t edge_cap, uint8_t* out,
                                        const uint64_t* out_off, const uint64_t* out_cap, uint64_t* out_len,
                                        int32_t* status, void* d_work, uint64_t* d_result);

#ifdef __cplusplus
}
#endif
#endif /* SNAPPIER_HIP_FRAME_RANGE_H */

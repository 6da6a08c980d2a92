/*
 * snappier_hip_frame_buffers.h -- C-ABI of libsnappier_hip_frame_buffers.so: device batch encode and decode of many Snappy FRAMED streams (the
 * format of snp_frame_encode / SnappyStream), the framing counterpart of snappier_hip_buffers.h and snappier_hip_buffers_decompress.h.
 *
 * An extension of include/snappier_hip.h in a library of its own, linked against libsnappier_hip.so and taking that library's contexts (snp_ctx).
 * It adds no status code and no option; the surfaces of snappier_hip.h and the other extension headers are unchanged.  The C# side binds these
 * functions in csharp/Snappier.Gpu/NativeMethodsFrameBuffers.cs.
 */
#ifndef SNAPPIER_HIP_FRAME_BUFFERS_H
#define SNAPPIER_HIP_FRAME_BUFFERS_H

#include "snappier_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* snp_frame_encode_device over nbuffers independent inputs, on the device: buffer b reads in[in_off[b] .. +in_len[b]) and becomes the framed
 * stream snp_frame_encode_device gives for it alone with the context's hash variant -- the 10-byte stream identifier, then one chunk per 65536
 * input bytes (an empty buffer: the identifier only) -- written at out[out_off[b] ..) when it fits in out_cap[b] bytes.  Per buffer: status[b] =
 * SNP_OK with out_len[b] = the stream's size, or SNP_ERR_OUTPUT_TOO_SMALL with out_len[b] = 0 when the stream is larger than out_cap[b] or when the
 * buffer's chunks do not fit in max_chunks (chunks go to buffers in order: the first buffer that does not fit and every later one fail).  A
 * buffer that is not OK has its out range left untouched.  Lengths are u64 (a framed stream has no 4 GiB limit); a buffer must hold fewer than
 * 2^32 chunks.  d_result (device, 2 x u64): [0] = chunk slots the batch needs (sum of ceil(in_len / 65536): grow max_chunks to it), [1] = sum of
 * out_len over the OK buffers.  d_work must hold snp_frame_encode_buffers_workspace(nbuffers, max_chunks) bytes (host arithmetic; 0 when
 * nbuffers is 0): ~76.6 KB per chunk slot (the compressor's staging) and ~16 B per buffer.  All arrays are device memory.
 * Stream capture: the call only enqueues (nothing is read back), under the rule of snp_compress_buffers_batch: make the same call, with the same
 * max_chunks, once before the capture so that the compressor's workspaces exist.
 * How: scans plan max_chunks slots, ONE launch of the snp_compress_batch compressor compresses every slot (with varint) into staging, one CRC
 * launch takes the masked CRC-32C of every raw chunk, a scan of the framed chunk sizes places each chunk, and a copy of one workgroup per chunk
 * emits them (frame_buffers.hip).  The compressor's layout follows max_chunks, not the chunks the batch holds: a loose bound costs time (DESIGN.md
 * 4.11), never a different result.
 * SNP_ERR_BAD_ARG for a null pointer (nbuffers == 0 needs only ctx and d_result, and still writes d_result), SNP_ERR_DEVICE for a runtime failure. */
uint64_t snp_frame_encode_buffers_workspace(uint32_t nbuffers, uint32_t max_chunks);
snp_status snp_frame_encode_buffers_batch(snp_ctx* ctx, const uint8_t* in, const uint64_t* in_off, const uint64_t* in_len,
                                          uint32_t nbuffers, uint32_t max_chunks, uint8_t* out, const uint64_t* out_off,
                                          const uint64_t* out_cap, uint64_t* out_len, int32_t* status,
                                          void* d_work, uint64_t* d_result);

/* snp_frame_decode_device over nstreams independent framed streams, on the device: stream b is in[in_off[b] .. +in_len[b]) and decodes into
 * out[out_off[b] .. +out_cap[b]).  status[b] and out_len[b] are what snp_frame_decode_device returns as d_result[1] / d_result[0] for that stream
 * alone, called with cap = out_cap[b] and a max_chunks that holds all its chunks, and an OK stream's bytes are the same: the first failing chunk
 * in stream order, else the error that ended the header walk, else OK.  A stream that is not OK may have had its own range written (contents
 * unspecified); nothing outside the output ranges is ever written.
 * Admission, in stream order: a stream is walked only if its spans fit in max_spans (ceil(in_len / 2^20) spans; an empty stream needs none), and
 * decoded only if the data chunks its walk lists also fit in max_chunks; the first stream that fails either bound gets SNP_ERR_OUTPUT_TOO_SMALL
 * with out_len 0, and so does every later stream.  To size a call: grow max_spans to d_result[2] first, then max_chunks to d_result[0].
 * d_result (device, 4 x u64): [0] = chunk slots the walked streams need, [1] = sum of out_len over the OK streams, [2] = span slots the batch
 * needs, [3] = spans whose true entry was not among their candidates (the resolver walked them on the spot: chunks larger than the window,
 * skippable chunks that cross spans).  d_work must hold snp_frame_decode_buffers_workspace(nstreams, max_chunks, max_spans) bytes (host
 * arithmetic; 0 when nstreams is 0): ~41 B per chunk slot, ~136 B per span slot, ~40 B per stream.  All arrays are device memory.
 * The header walk is always the span walk of snp_frame_decode_device (SNP_OPT_FRAME_SCAN is not read); no option changes a result.
 * Stream capture: the call only enqueues (nothing is read back), under the rule of snp_decompress_batch: make the same call once before the capture.
 * SNP_ERR_BAD_ARG for a null pointer (nstreams == 0 needs only ctx and d_result, and still writes d_result), SNP_ERR_DEVICE for a runtime failure. */
uint64_t snp_frame_decode_buffers_workspace(uint32_t nstreams, uint32_t max_chunks, uint32_t max_spans);
snp_status snp_frame_decode_buffers_batch(snp_ctx* ctx, const uint8_t* in, const uint64_t* in_off, const uint64_t* in_len,
                                          uint32_t nstreams, uint32_t max_chunks, uint32_t max_spans, uint8_t* out,
                                          const uint64_t* out_off, const uint64_t* out_cap, uint64_t* out_len,
                                          int32_t* status, void* d_work, uint64_t* d_result);

#ifdef __cplusplus
}
#endif
#endif /* SNAPPIER_HIP_FRAME_BUFFERS_H */

/*
 * snappier_hip_layout.h -- C-ABI of libsnappier_hip_layout.so: the decoded length of every item of a device batch, and the output layout
 * (out_off[], out_cap[]) that the batch decoders take, computed on the device from the compressed bytes alone.  The missing link between
 * "compressed bytes in device memory" and snp_decompress_batch / snp_decompress_buffers_batch (snappier_hip_buffers_decompress.h) /
 * snp_frame_decode_buffers_batch (snappier_hip_frame_buffers.h): the device counterpart of snp_get_uncompressed_length and
 * snp_frame_decoded_length (Snappy.GetUncompressedLength, and the sizing half of DecompressToMemory, in the reference).
 *
 * An extension of include/snappier_hip.h in a library of its own, linked against libsnappier_hip.so and taking that library's contexts (snp_ctx).
 * It adds no status code and no option; the surfaces of snappier_hip.h and the other extension headers are unchanged.  The C# side binds these
 * functions in csharp/Snappier.Gpu/NativeMethodsLayout.cs.
 *
 * Both calls only enqueue on the context's stream: they read nothing back, allocate nothing, keep no state in the context, and can be captured
 * into a graph (make the same call once before the capture, the rule of the other batch calls).  Their out_off / out_cap outputs are, by type
 * and meaning, the out_off / out_cap inputs of the decoders named above, so layout -> decode chains on one stream with no host step in between.
 * Offsets are relative to whatever `out` pointer the decode call is given.  The calls only read `in`: input ranges may overlap each other.
 *
 * Placement, common to both (items in index order): an item that takes part has a SLOT of its decoded length rounded up to `align` (a power of
 * two from 1 to 2^20, else SNP_ERR_BAD_ARG); every other item has a slot of 0.  out_off[b] = the sum of the slots before b, so the first offset
 * is 0, every offset is a multiple of align, and the ranges [out_off, out_off + out_cap) are disjoint and in order.  Let f be the first item that
 * takes part and whose range ends beyond arena_cap (out_off[f] + length > arena_cap): f and every later item that takes part get
 * SNP_ERR_OUTPUT_TOO_SMALL and out_cap 0 -- even one that would fit: the in-order admission rule of the other batch calls -- and keep their
 * length outputs; the caller decodes what was placed and resumes from d_result[1].  arena_cap = UINT64_MAX (or anything >= d_result[0]) places
 * everything.  The u64 sums cannot overflow (2^32 items of less than 2^32 + 2^20 bytes each; a framed stream's total is bounded by its bytes).
 */
#ifndef SNAPPIER_HIP_LAYOUT_H
#define SNAPPIER_HIP_LAYOUT_H

#include "snappier_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Snappy blocks: buffer b is in[in_off[b] .. +in_len[b]) (in_len u32, as snp_decompress_batch takes it).
 * status[b] / declared[b] = what snp_get_uncompressed_length returns for those bytes: SNP_OK and the preamble's value, or SNP_ERR_BAD_LENGTH and
 * 0 (an empty buffer, an unterminated or over-long varint, bits above 2^32); at most 5 bytes of a buffer are read.  One rule more, the one the
 * framed walk applies to its chunks so that a hostile preamble never sizes an allocation: declared > ((in_len - header_bytes) / 3 + 1) * 64
 * gives SNP_ERR_INCOMPLETE with declared[b] = 0.  No tag expands more than 3 bytes into 64, so every such block fails in every decoder too,
 * whatever capacity it is given; the decoder's status for it may be a different one (it can meet another error first, or the capacity).
 * Only OK buffers take part in the placement (above): out_cap[b] = declared[b] for a placed one and 0 for every other; a buffer that is not OK
 * does not stop the placement, and one behind f keeps its own status.  declared is kept for the OK buffers that were not placed.
 * d_result (device, 4 x u64): [0] = arena bytes the whole batch needs with an unbounded arena_cap (out_off + declared of the last OK buffer, 0
 * if there is none), [1] = f, the first buffer not placed (nbuffers if all OK buffers were), [2] = sum of ceil(declared / 65536) over the placed
 * buffers (a safe max_fragments for snp_decompress_buffers_batch), [3] = sum of declared over the placed buffers.
 * d_work must hold snp_decompress_layout_workspace(nbuffers) bytes (host arithmetic; 0 when nbuffers is 0): ~8 B per buffer.  All arrays are
 * device memory.
 * How: one thread per buffer reads its preamble; an exclusive scan of the slots (scan_tiles.h); a minimum over the buffers that pass arena_cap;
 * one thread per buffer writes the outputs (layout.hip).  Seven launches, whatever the batch.
 * SNP_ERR_BAD_ARG for a null pointer or a bad align (nbuffers == 0 needs only ctx and d_result, and still writes d_result), SNP_ERR_DEVICE for a
 * runtime failure. */
uint64_t snp_decompress_layout_workspace(uint32_t nbuffers);
snp_status snp_decompress_layout_batch(snp_ctx* ctx, const uint8_t* in, const uint64_t* in_off, const uint32_t* in_len,
                                       uint32_t nbuffers, uint32_t align, uint64_t arena_cap, uint64_t* out_off,
                                       uint32_t* out_cap, uint32_t* declared, int32_t* status,
                                       void* d_work, uint64_t* d_result);

/* Framed streams: stream b is in[in_off[b] .. +in_len[b]) (u64 lengths, as snp_frame_decode_buffers_batch takes them).
 * status[b] / decoded_len[b] = the return value and *out_len of snp_frame_decoded_length on stream b alone: the sum over the data chunks listed
 * before the header walk ended, and the error that ended it (SNP_ERR_TRUNCATED_STREAM, SNP_ERR_BAD_LENGTH, SNP_ERR_INCOMPLETE,
 * SNP_ERR_CHUNK_TYPE) or SNP_OK.  nchunks[b] = the data chunks listed.  No chunk body is decoded and no CRC is checked.
 * Admission by spans, exactly as in snp_frame_decode_buffers_batch: a stream is walked only if its spans fit in max_spans (ceil(in_len / 2^20)
 * spans; an empty stream needs none); the first stream that does not fit and every later one get SNP_ERR_OUTPUT_TOO_SMALL with out_off, out_cap,
 * decoded_len and nchunks 0.
 * Every WALKED stream takes part in the placement (above), whatever its walk's status: out_cap[b] = decoded_len[b], so that the decode call
 * that follows has room for the listed chunks and reports exactly what snp_frame_decode_device reports for that stream (first failing chunk,
 * else the walk's error, else OK).  A walked stream at or behind f gets SNP_ERR_OUTPUT_TOO_SMALL in place of its walk's status and out_cap 0,
 * and keeps decoded_len and nchunks.
 * d_result (device, 5 x u64): [0] = arena bytes the walked streams need with an unbounded arena_cap, [1] = the first stream not placed (not
 * walked, or f; nstreams if all were placed), [2] = span slots the batch needs (grow max_spans to it), [3] = sum of nchunks over the placed
 * streams (the max_chunks the decode call wants for them; when every stream is placed, that call's d_result[0]), [4] = spans whose true entry
 * was not among their candidates (as d_result[3] of the decode call).
 * d_work must hold snp_frame_decode_layout_workspace(nstreams, max_spans) bytes (host arithmetic; 0 when nstreams is 0): ~136 B per span slot,
 * ~40 B per stream.  All arrays are device memory.
 * How: the span scan, walk A and walk B of snp_frame_decode_buffers_batch -- the same kernels (frame_walk_device.h), with no capacity bound --
 * then the slot scan, the minimum and the writing kernel of the block call.
 * SNP_ERR_BAD_ARG for a null pointer or a bad align (nstreams == 0 needs only ctx and d_result, and still writes d_result), SNP_ERR_DEVICE for a
 * runtime failure. */
uint64_t snp_frame_decode_layout_workspace(uint32_t nstreams, uint32_t max_spans);
snp_status snp_frame_decode_layout_batch(snp_ctx* ctx, const uint8_t* in, const uint64_t* in_off, const uint64_t* in_len,
                                         uint32_t nstreams, uint32_t max_spans, uint32_t align, uint64_t arena_cap,
                                         uint64_t* out_off, uint64_t* out_cap, uint64_t* decoded_len, uint32_t* nchunks,
                                         int32_t* status, void* d_work, uint64_t* d_result);

#ifdef __cplusplus
}
#endif
#endif /* SNAPPIER_HIP_LAYOUT_H */

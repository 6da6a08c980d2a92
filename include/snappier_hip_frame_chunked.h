/*
 * snappier_hip_frame_chunked.h -- C-ABI of libsnappier_hip_frame_chunked.so: device batch encode of many Snappy framed streams with a CHOSEN CHUNK
 * SIZE, and the seek index of what it wrote.  snp_frame_encode_buffers_batch (snappier_hip_frame_buffers.h) cuts every buffer into 65536-byte
 * chunks; the chunk is the unit of random access (a window that cuts a chunk pays for the whole chunk), so a caller who reads small records
 * wants smaller chunks, and wants the index that snp_frame_read_indexed_batch (snappier_hip_frame_index.h) takes without walking bytes it has
 * just written.
 *
 * An extension of include/snappier_hip.h in a library of its own, linked against libsnappier_hip.so and taking that library's contexts (snp_ctx).
 * It adds no status code and no option and keeps no state in the context; the surfaces of snappier_hip.h and the other extension headers are
 * unchanged.  The C# side binds these functions in csharp/Snappier.Gpu/NativeMethodsFrameChunked.cs.
 */
#ifndef SNAPPIER_HIP_FRAME_CHUNKED_H
#define SNAPPIER_HIP_FRAME_CHUNKED_H

#include "snappier_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* nbuffers independent inputs, on the device: buffer b reads in[in_off[b] .. +in_len[b]) and becomes a framed stream at out[out_off[b] ..) when
 * it fits in out_cap[b] bytes: the 10-byte stream identifier, then one chunk per chunk_bytes input bytes, the last one shorter (an empty buffer:
 * the identifier only) -- what SnappyStreamCompressor writes for Write(chunk_bytes bytes); Flush() in a loop.  chunk_bytes is 1 .. 65536, one
 * value for the call (the format allows no more than 65536 raw bytes in a chunk).  Each chunk is what CompressBlock makes of its piece with the
 * context's hash variant: type 0x00 with varint || fragment when that is smaller than the piece, else type 0x01 with the piece, and the masked
 * CRC-32C of the piece.  So the stream is the identifier plus, for each piece, snp_frame_encode_device(piece) without its identifier; every
 * decoder of this project, and any conforming one, reads it.  At chunk_bytes = 65536 out, out_len, status and d_result[0..1] are exactly those of
 * snp_frame_encode_buffers_batch.
 * Per buffer: status[b] = SNP_OK with out_len[b] = the stream's size, or SNP_ERR_OUTPUT_TOO_SMALL with out_len[b] = 0 when the stream is larger
 * than out_cap[b] or when the buffer's chunks (ceil(in_len / chunk_bytes)) do not fit in max_chunks (chunks go to buffers in order: the first
 * buffer that does not fit and every later one fail).  A buffer that is not OK has its out range left untouched.  Lengths are u64; a buffer must
 * hold fewer than 2^32 chunks.  10 + 8 * ceil(n / chunk_bytes) + n bytes always hold buffer b's stream.
 * d_result (device, 4 x u64): [0] = chunk slots the batch needs (grow max_chunks to it), [1] = sum of out_len over the OK buffers, [2] = index
 * rows written (= idx_first[nbuffers]; 0 without an index), [3] = buffers that are OK.
 *
 * The index: idx_first, idx_start, idx_pos, idx_total, idx_tail are either all null (no index: nothing else differs) or all given, as
 * snappier_hip_frame_index.h describes them -- idx_first[nbuffers + 1], idx_total[nbuffers], idx_tail[nbuffers], and idx_start / idx_pos of
 * max_chunks rows each.  An OK buffer gets one row per chunk, in order: idx_start = k * chunk_bytes, idx_pos = the position of the chunk's
 * 4-byte header relative to the stream's first byte; idx_total[b] = in_len[b], idx_tail[b] = SNP_OK.  A buffer that is not OK gets idx_total = 0,
 * idx_tail = SNP_ERR_OUTPUT_TOO_SMALL and no rows (idx_first[b + 1] == idx_first[b]) -- also one in the middle of the batch whose stream did not
 * fit out_cap: the rows of the buffers after it follow those of the buffers before it.  When every buffer is OK the five arrays are element
 * for element what snp_frame_index_batch writes for the emitted streams (in_off = out_off, in_len = out_len, bounds that admit them all), and
 * they go straight into snp_frame_read_indexed_batch with nentries = max_chunks.
 *
 * d_work must hold snp_frame_encode_chunked_workspace(nbuffers, max_chunks, chunk_bytes) bytes (host arithmetic; 0 when nbuffers is 0): per chunk
 * slot 44 bytes and the compressor's staging, snp_max_compressed_length(chunk_bytes) rounded up to 16, plus 16 -- about 1.2 x chunk_bytes, so the
 * workspace is about 1.2 x the input at every chunk size from a few hundred bytes up.  All arrays are device memory.
 * Stream capture: the call only enqueues (nothing is allocated, read back or synchronised), under the rule of snp_frame_encode_buffers_batch:
 * make the same call, with the same max_chunks, once before the capture so that the compressor's workspaces exist.
 * How: frame_chunked.hip -- the scans, the ONE compressor launch and the ONE CRC launch of snp_frame_encode_buffers_batch over max_chunks slots,
 * one more scan for the index, and an emit whose workgroups each take the slots of 64 KiB of input.
 * SNP_ERR_BAD_ARG for chunk_bytes = 0 or above 65536, for an index given in part, for a null pointer (nbuffers == 0 needs only ctx and d_result,
 * and still writes d_result), SNP_ERR_DEVICE for a runtime failure. */
uint64_t snp_frame_encode_chunked_workspace(uint32_t nbuffers, uint32_t max_chunks, uint32_t chunk_bytes);
snp_status snp_frame_encode_chunked_batch(snp_ctx* ctx, const uint8_t* in, const uint64_t* in_off, const uint64_t* in_len,
                                          uint32_t nbuffers, uint32_t chunk_bytes, uint32_t max_chunks, uint8_t* out,
                                          const uint64_t* out_off, const uint64_t* out_cap, uint64_t* out_len, int32_t* status,
                                          uint64_t* idx_first, uint64_t* idx_start, uint64_t* idx_pos, uint64_t* idx_total,
                                          int32_t* idx_tail, void* d_work, uint64_t* d_result);

#ifdef __cplusplus
}
#endif
#endif /* SNAPPIER_HIP_FRAME_CHUNKED_H */

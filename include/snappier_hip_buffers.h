/*
 * snappier_hip_buffers.h -- C-ABI of libsnappier_hip_buffers.so: device batch compress of buffers of ANY length, one Snappy block each.
 *
 * An extension of include/snappier_hip.h, in a library of its own that is linked against libsnappier_hip.so and takes that library's
 * contexts (snp_ctx).  It adds no status code and no option.  The drop-in surface of snappier_hip.h is unchanged; the C# side binds these
 * functions in csharp/Snappier.Gpu/NativeMethodsBuffers.cs.
 */
#ifndef SNAPPIER_HIP_BUFFERS_H
#define SNAPPIER_HIP_BUFFERS_H

#include "snappier_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* SnappyCompressor.TryCompress  SnappyCompressor.cs:24-83 over nbuffers independent inputs of ANY length < 2^32, on the device: buffer b reads
 * in[in_off[b] .. +in_len[b]) and becomes ONE Snappy block, varint(in_len[b]) || CompressFragment of each 65536-byte piece in order -- the
 * bytes snp_try_compress gives for it -- written at out[out_off[b] ..) when it fits in out_cap[b] bytes.  Per buffer: status[b] = SNP_OK with
 * out_len[b] = the block size, or SNP_ERR_OUTPUT_TOO_SMALL with out_len[b] = 0 when the block is larger than out_cap[b] (TryCompress returns
 * false) or when the buffer's fragments do not fit in max_fragments (fragments go to buffers in order: that buffer and every later one fail).
 * A buffer that is not OK has its out range left untouched.  d_result (device, 2 x u64): [0] = fragments the batch needs
 * (sum of ceil(in_len / 65536): grow max_fragments to it and retry), [1] = sum of out_len over the OK buffers.  d_work must hold
 * snp_compress_buffers_workspace(nbuffers, max_fragments) bytes (host arithmetic; 0 when nbuffers is 0) -- the fragment table and ~76.5 KB
 * of staging per fragment slot.  All arrays are device memory.
 * Stream capture: the call only enqueues, under the same rule as snp_compress_batch (snappier_hip.h): make the same call, with the same
 * max_fragments, once before the capture so that the compressor's workspaces exist.
 * How: an exclusive scan of the fragment counts plans max_fragments slots (those past the batch stay empty), ONE snp_compress_batch-style
 * launch compresses every slot without varint into the staging area, a scan of the compressed lengths places each fragment, and a copy of one
 * workgroup per fragment emits them (buffers.hip).  The compressor's layout follows max_fragments, not the fragments the batch holds: a loose
 * bound costs time, never a different result.
 * SNP_ERR_BAD_ARG for a null pointer (nbuffers == 0 needs only ctx and d_result, and still writes d_result), SNP_ERR_DEVICE for a runtime failure. */
uint64_t snp_compress_buffers_workspace(uint32_t nbuffers, uint32_t max_fragments);
snp_status snp_compress_buffers_batch(snp_ctx* ctx, const uint8_t* in, const uint64_t* in_off, const uint32_t* in_len,
                                      uint32_t nbuffers, uint32_t max_fragments, uint8_t* out, const uint64_t* out_off,
                                      const uint64_t* out_cap, uint64_t* out_len, int32_t* status,
                                      void* d_work, uint64_t* d_result);

#ifdef __cplusplus
}
#endif
#endif /* SNAPPIER_HIP_BUFFERS_H */

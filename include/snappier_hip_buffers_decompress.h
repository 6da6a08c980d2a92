/*
 * snappier_hip_buffers_decompress.h -- C-ABI of libsnappier_hip_buffers_decompress.so: device batch decompress that splits large blocks across
 * wavefronts, the decode-side sibling of snp_compress_buffers_batch (snappier_hip_buffers.h).
 *
 * An extension of include/snappier_hip.h in a library of its own, linked against libsnappier_hip.so and taking that library's contexts (snp_ctx).
 * It adds no status code and no option; the surfaces of snappier_hip.h and snappier_hip_buffers.h are unchanged.  The C# side binds these
 * functions in csharp/Snappier.Gpu/NativeMethodsBuffersDecompress.cs.
 */
#ifndef SNAPPIER_HIP_BUFFERS_DECOMPRESS_H
#define SNAPPIER_HIP_BUFFERS_DECOMPRESS_H

#include "snappier_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* snp_decompress_batch with the same arguments and the same results, for batches that hold LARGE blocks: every array has the type and meaning it
 * has there (all device memory), and per block status[b] and out_len[b] are what snp_decompress_batch gives, as are the bytes of every OK block.
 * A block that is not OK may have had its own range [out_off[b], +out_cap[b]) written (contents unspecified); nothing outside the ranges is ever
 * written.  While the call is in flight status[b] may transiently hold -1, as there.
 * Which blocks are split into 64 KiB output fragments, one wavefront each, is decided on the device, per block: a clean varint preamble,
 * par_min <= declared <= out_cap[b] (par_min = SNP_OPT_PARALLEL_DECODE_MIN of the context, 0 = never), hb < in_len[b] <= snp_max_compressed_length
 * (declared) -- and declared >= 2 * (sum of declared over those blocks) / (the device's persistent wavefront slots), so a batch of many mid-sized
 * blocks is left to one wavefront per block.  The chosen blocks are admitted in buffer order while their fragments fit in max_fragments; a
 * block that does not fit is decoded by one wavefront instead (same result, only slower).  No bound changes a result.
 * d_result (device, 4 x u64): [0] = fragments the blocks chosen for splitting need (grow max_fragments to it), [1] = blocks decoded by fragments,
 * [2] = blocks chosen and admitted that fell back to one wavefront (foreign streams whose copies cross fragments, malformed blocks), [3] = split
 * blocks whose tag index took the look-back pass.  The host-only snp_ctx_counter values are left alone.
 * d_work must hold snp_decompress_buffers_workspace(nbuffers, max_fragments) bytes (host arithmetic; 0 when nbuffers is 0; max_fragments counts
 * up to 2^26): ~3 KB per fragment slot and ~0.1 KB per buffer, plus 104 KB per tag-index scan workgroup (at most 256).
 * Stream capture: the call only enqueues, under the same rule as snp_decompress_batch: make the same call once before the capture.
 * SNP_ERR_BAD_ARG for a null pointer (nbuffers == 0 needs only ctx and d_result, and still writes d_result), SNP_ERR_DEVICE for a runtime failure. */
uint64_t snp_decompress_buffers_workspace(uint32_t nbuffers, uint32_t max_fragments);
snp_status snp_decompress_buffers_batch(snp_ctx* ctx, const uint8_t* in, const uint64_t* in_off, const uint32_t* in_len,
                                        uint32_t nbuffers, uint32_t max_fragments, uint8_t* out, const uint64_t* out_off,
                                        const uint32_t* out_cap, uint32_t* out_len, int32_t* status,
                                        void* d_work, uint64_t* d_result);

#ifdef __cplusplus
}
#endif
#endif /* SNAPPIER_HIP_BUFFERS_DECOMPRESS_H */

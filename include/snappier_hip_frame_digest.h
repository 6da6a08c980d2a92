/*
 * snappier_hip_frame_digest.h -- C-ABI of libsnappier_hip_frame_digest.so: device batch DIGEST of seekable Snappy framed streams -- the CRC-32C
 * of any number of windows of what the streams decode to, computed WITHOUT decoding them.  Every data chunk header of the framing format holds
 * the masked CRC-32C of the chunk's decoded bytes, and CRC is GF(2)-linear: the CRC of a concatenation is the XOR of the pieces' CRCs, each
 * multiplied by x^(8 x the bytes behind it) modulo the polynomial.  A window's digest takes one header read and one modular multiplication per
 * chunk inside it; only the at most two chunks the window cuts are decoded.  A whole-stream digest decodes nothing.  The digest depends on the
 * decoded bytes alone, not on the chunk grid or the compressed bytes: streams kept at different chunk sizes, or edited by the splice, rechunk
 * and compose calls, compare by content.
 *
 * An extension of include/snappier_hip.h in a library of its own, linked against libsnappier_hip.so and taking that library's contexts (snp_ctx).
 * It adds no status code and no option, keeps no state in the context and reads no environment variable; the surfaces of snappier_hip.h and the
 * other extension headers are unchanged.  The C# side binds these functions in csharp/Snappier.Gpu/NativeMethodsFrameDigest.cs.
 */
#ifndef SNAPPIER_HIP_FRAME_DIGEST_H
#define SNAPPIER_HIP_FRAME_DIGEST_H

#include "snappier_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Streams and index as snp_frame_read_indexed_batch takes them (snappier_hip_frame_index.h): stream b is in[in_off[b] .. +in_len[b]), its rows
 * are [idx_first[b], idx_first[b + 1]) of idx_start / idx_pos, nentries = the rows the index arrays hold.
 * nreq requests, independent of each other: request r names stream req_stream[r] and the window [req_off[r], req_off[r] + req_len[r]) of what
 * the stream decodes to, clipped to idx_total exactly as the read clips it -- req_off = 0, req_len = 2^64 - 1 is the whole stream.  Any number
 * of requests may name one stream, in any order.
 *
 * Result.  dig_len[r] = hi - lo, the clipped window's length; digest[r] = the plain (unmasked) CRC-32C of those bytes (what snp_crc32c gives
 * with masked = 0).  An empty window gives 0.  A request that is not SNP_OK has digest = 0 and dig_len = 0.
 *
 * Selection and checks are the indexed read's, with no capacity: the two binary searches, head edge / interior rows / tail edge, and the check
 * of EVERY owned row, interior or edge, against the header it points at (a data chunk that decodes to exactly end - start bytes; an interior
 * row inside the window).  THE INDEX IS UNTRUSTED INPUT: index reads are bounded by nentries, header reads by in_len[b], and nothing is written
 * outside digest, dig_len, status, d_result and d_work.  A stale index, one built from other bytes or one filled with anything at all gives
 * SNP_ERR_BAD_ARG per request, as in the read; so does req_stream[r] >= nstreams and an idx_tail that is no status of the walk.  A request on a
 * stream whose idx_tail is SNP_ERR_OUTPUT_TOO_SMALL (not indexed) gets that status.
 *
 * An interior row is never decoded: it adds shift(unmask(crc in its header), hi - end), shift(c, n) = c * x^(8n) mod P on reflected values,
 * P = 0x82F63B78.  A zero-length row adds nothing and its header CRC is not looked at.  An edge row (head, tail, or the one row that holds the
 * whole window) is decoded and verified whole into the scratch arena inside d_work, as the read does it; the part inside the window goes
 * through the library's CRC kernel and is shifted like the others.  An edge that fails to decode or verify gives the request the status the
 * read gives it.
 *
 * Status.  status[r] is what snp_frame_read_indexed_batch returns for the same request with out_cap = 2^64 - 1 and bounds that admit it, on
 * streams whose interior chunks are sound (the strict tail rule included: a stream whose walk ended in an error gives that error).
 * A CORRUPT BODY OF AN INTERIOR CHUNK IS NOT NOTICED: THE DIGEST IS THE CRC OF WHAT THE STREAM'S HEADERS DECLARE, NOT OF WHAT ITS BODIES
 * DECODE TO.  The calls that verify every chunk are the reads (snp_frame_read_indexed_batch, snp_frame_decode_buffers_batch) and
 * snp_frame_rechunk_indexed_batch with SNP_RECHUNK_REWRITE_ALL.
 *
 * Admission, in request order: the decoded bytes of a request's edges must fit edge_cap, counted with those of the requests before it.  The
 * first request that misses, and every later one, get SNP_ERR_OUTPUT_TOO_SMALL.
 * d_result (device, 4 x u64): [0] = interior rows combined into the digests of the OK requests, [1] = sum of dig_len over the OK requests,
 * [2] = edge scratch bytes needed, [3] = requests that are OK.  edge_cap = 0 is a real call for windows on chunk boundaries (whole streams
 * among them: they have no edges), and the sizing call for the rest.
 * d_work must hold snp_frame_digest_indexed_workspace(nreq, edge_cap) bytes (host arithmetic; 0 when nreq is 0): per-request words, two edge
 * rows per request and edge_cap bytes -- nothing per interior row.  nreq must be below 2^30, else SNP_ERR_BAD_ARG.  All arrays are device
 * memory; the call only reads `in` and the index.
 * How: one wavefront per 64 interior rows of a request, found by a search in the scan of the requests' row counts, so rows are balanced and not
 * requests; one atomic XOR per wavefront (frame_digest.hip).
 * Stream capture: the call only enqueues on the context's stream -- no allocation, no read-back, no synchronisation -- under the rule of
 * snp_decompress_batch: make the same call once before the capture.  No option changes a result.
 * SNP_ERR_BAD_ARG for a null pointer (nreq == 0 needs only ctx and d_result, and still writes d_result), SNP_ERR_DEVICE for a runtime failure. */
uint64_t snp_frame_digest_indexed_workspace(uint32_t nreq, uint64_t edge_cap);
snp_status snp_frame_digest_indexed_batch(snp_ctx* ctx, const uint8_t* in, const uint64_t* in_off, const uint64_t* in_len, uint32_t nstreams,
                                          const uint64_t* idx_first, const uint64_t* idx_start, const uint64_t* idx_pos,
                                          const uint64_t* idx_total, const int32_t* idx_tail, uint64_t nentries,
                                          const uint32_t* req_stream, const uint64_t* req_off, const uint64_t* req_len, uint32_t nreq,
                                          uint64_t edge_cap, uint32_t* digest, uint64_t* dig_len, int32_t* status, void* d_work,
                                          uint64_t* d_result);

/* Host arithmetic, no context and no device: the plain CRC-32C of A || B from the plain CRC-32Cs of A and of B and B's length in bytes --
 * shift(crc_a, len_b) ^ crc_b.  len_b may be any value; len_b = 0 gives crc_a ^ crc_b with crc_b = 0 for an empty B. */
uint32_t snp_crc32c_combine(uint32_t crc_a, uint32_t crc_b, uint64_t len_b);

#ifdef __cplusplus
}
#endif
#endif /* SNAPPIER_HIP_FRAME_DIGEST_H */

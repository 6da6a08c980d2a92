/*
 * snappier_hip_frame_diff.h -- C-ABI of libsnappier_hip_frame_diff.so: device batch DIFF of seekable Snappy framed streams -- the longest common
 * prefix and the longest common suffix of pairs of windows of what the streams decode to.  The digest (snappier_hip_frame_digest.h) says whether
 * two windows hold the same bytes; this call says WHERE they part, which is the one splice (off, del, ins) that turns one into the other
 * (snappier_hip_frame_splice.h applies it).  Every data chunk header holds the CRC-32C of the chunk's decoded bytes and CRC is GF(2)-linear, so
 * wherever both streams have a chunk boundary at the same decoded offset the span between two such COMMON CUTS is compared from the headers
 * alone; only the first span whose CRCs differ and the ragged pieces no common cut covers are decoded.  The two streams may be kept at
 * different chunk sizes or have been edited by different splice, rechunk and compose calls: the answer depends on the decoded bytes alone.
 *
 * An extension of include/snappier_hip.h in a library of its own, linked against libsnappier_hip.so and taking that library's contexts (snp_ctx).
 * It adds no status code and no option, keeps no state in the context and reads no environment variable; the surfaces of snappier_hip.h and the
 * other extension headers are unchanged.  The C# side binds these functions in csharp/Snappier.Gpu/NativeMethodsFrameDiff.cs.
 */
#ifndef SNAPPIER_HIP_FRAME_DIFF_H
#define SNAPPIER_HIP_FRAME_DIFF_H

#include "snappier_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SNP_DIFF_PREFIX 1u   /* find the longest common prefix */
#define SNP_DIFF_SUFFIX 2u   /* find the longest common suffix */
#define SNP_DIFF_EXACT 4u    /* use no header CRC: decode and compare both windows whole */

/* Sides.  Each of the sides A and B is a batch of streams with its index, exactly as snp_frame_read_indexed_batch takes them
 * (snappier_hip_frame_index.h): stream b is in[in_off[b] .. +in_len[b]), its rows are [idx_first[b], idx_first[b + 1]) of idx_start / idx_pos,
 * nentries = the rows the index arrays hold.  The same arrays may be passed for both sides (the call only reads them): that compares two
 * streams of one batch.
 * Requests.  Request r compares the window [req_off_a[r], req_off_a[r] + req_len_a[r]) of stream req_stream_a[r] of side A with the window
 * [req_off_b[r], +req_len_b[r]) of stream req_stream_b[r] of side B.  Each window is clipped to its stream's idx_total exactly as the read
 * clips it -- offset 0, length 2^64 - 1 is the whole stream.  The clipped lengths may differ; n = min(len_a[r], len_b[r]).  Any number of
 * requests may name one stream, in any order.
 * flags: SNP_DIFF_PREFIX | SNP_DIFF_SUFFIX | SNP_DIFF_EXACT; at least one of PREFIX and SUFFIX, and no other bit, else SNP_ERR_BAD_ARG.
 *
 * Result of a request that is SNP_OK.  len_a[r], len_b[r] = the clipped lengths.  prefix[r] = the largest p <= n with A[0, p) == B[0, p).
 * The raw suffix is the largest s <= n with A[len_a - s, len_a) == B[len_b - s, len_b).  With both flags suffix[r] = min(raw, n - prefix[r]):
 * the two never overlap, and (off = prefix, del = len_a - prefix - suffix, ins = B[prefix, len_b - suffix)) is a splice that turns window A
 * into window B.  With SNP_DIFF_SUFFIX alone suffix[r] is the raw value.  A direction that was not asked for gives 0.  The windows are equal
 * iff prefix == len_a == len_b.  A request that is not SNP_OK has all four outputs 0.
 *
 * How equality is decided.  Work in t = the distance from the windows' starts.  The common cuts are the t in [0, n] at which both sides have a
 * chunk boundary (a zero-length chunk is a boundary and adds nothing).  For the span between two consecutive common cuts each side XORs the
 * unmasked header CRCs of its chunks in the span, each shifted over the bytes behind it (the arithmetic of snappier_hip_frame_digest.h); spans
 * whose values agree are TAKEN AS EQUAL AND ARE NOT DECODED.  Decoded whole and verified, into the scratch arena inside d_work, and then
 * compared byte for byte are: the chunks that hold the bytes before the first common cut; the chunks of the first span whose values differ;
 * when no span differs, the chunks that hold the bytes after the last common cut; when there is no common cut, the chunks that hold [0, n).
 * The suffix is the mirror image, in t = the distance from the windows' ends, with decodes of its own -- except that on windows of one length
 * a suffix that needs the whole window compares what the prefix decoded when that needs the whole window too.  With SNP_DIFF_EXACT no cut
 * is used: the chunks that hold [0, n) are decoded and compared whole.
 * A CORRUPT BODY OF A CHUNK THAT IS NOT DECODED IS NOT NOTICED: WHAT IS COMPARED THERE IS WHAT THE STREAMS' HEADERS DECLARE, NOT WHAT THEIR
 * BODIES DECODE TO.
 * TWO DIFFERENT SPANS WHOSE HEADER CRCS COLLIDE (PROBABILITY 2^-32 PER SPAN) ARE TAKEN AS EQUAL, UNLESS SNP_DIFF_EXACT IS SET.
 * The calls that verify every chunk are the reads and snp_frame_rechunk_indexed_batch with SNP_RECHUNK_REWRITE_ALL.
 *
 * Checks and status.  BOTH INDEXES ARE UNTRUSTED INPUT, as in the read: index reads are bounded by nentries, header reads by in_len[b], every
 * row a request owns on either side (the rows the read would select for its window) is checked against the header it points at, and nothing
 * is written outside len_a, len_b, prefix, suffix, status, d_result and d_work.  A stale index, one built from other bytes or one filled with
 * anything at all gives SNP_ERR_BAD_ARG per request; so does req_stream >= nstreams and an idx_tail that is no status of the walk.  A
 * request on a stream that was not indexed gets its SNP_ERR_OUTPUT_TOO_SMALL.  A side's verdict is, in this order: what the read's plan
 * refuses; SNP_ERR_BAD_ARG for a row that fails its check (then nothing of the request is decoded); the status of the first chunk, in stream
 * order, that this call decodes on that side and that fails to decode or verify; the error that ended the stream's walk (the strict tail
 * rule).  status[r] is side A's verdict if that is not SNP_OK, else side B's.  When a side's plan refuses the request, the other side's rows
 * are not looked at.
 *
 * Admission, in request order.  A request is admitted if the rows it owns, summed over both sides, fit max_rows, and the decoded bytes of the
 * chunks it decodes, summed over both sides and both directions, fit scratch_cap (a run of consecutive chunks counts no less than one byte
 * per chunk: a zero-length chunk in it costs a byte) -- each counted together with the requests before it.  The
 * first request that misses a bound, and every later one, get SNP_ERR_OUTPUT_TOO_SMALL.  A request that is refused for another reason counts
 * no row (a refused plan) and no byte.
 * d_result (device, 4 x u64): [0] = rows needed, over all requests whatever was admitted; [1] = sum of n over the SNP_OK requests;
 * [2] = scratch bytes needed by the requests that passed the row bound (complete when [0] <= max_rows); [3] = requests that are SNP_OK.
 * SIZING TAKES TWO ROUNDS, because which chunks are decoded depends on the headers' content: call with max_rows = 0 (and scratch_cap = 0)
 * for [0], then with that max_rows and scratch_cap = 0 for [2].
 * d_work must hold snp_frame_diff_indexed_workspace(nreq, max_rows, scratch_cap) bytes (host arithmetic; 0 when nreq is 0): per-request words,
 * per owned row two words, per side min(2 x max_rows, scratch_cap) rows of a chunk table, and scratch_cap bytes.  nreq must be below 2^30 and max_rows below 2^31, else
 * SNP_ERR_BAD_ARG (the workspace function then gives 0).  All arrays are device memory; the call only reads the streams and the indexes.
 * How: one wavefront per request and direction walks the rows of both sides 64 at a time; the byte compare takes 16 bytes per lane
 * (frame_diff.hip).
 * Stream capture: the call only enqueues on the context's stream -- no allocation, no read-back, no synchronisation -- under the rule of
 * snp_decompress_batch: make the same call once before the capture.  No option changes a result.
 * SNP_ERR_BAD_ARG for a null pointer (nreq == 0 needs only ctx, d_result and legal flags, and still writes d_result), SNP_ERR_DEVICE for a
 * runtime failure. */
uint64_t snp_frame_diff_indexed_workspace(uint32_t nreq, uint64_t max_rows, uint64_t scratch_cap);
snp_status snp_frame_diff_indexed_batch(snp_ctx* ctx, const uint8_t* in_a, const uint64_t* in_off_a, const uint64_t* in_len_a, uint32_t nstreams_a,
                                        const uint64_t* idx_first_a, const uint64_t* idx_start_a, const uint64_t* idx_pos_a,
                                        const uint64_t* idx_total_a, const int32_t* idx_tail_a, uint64_t nentries_a, const uint8_t* in_b,
                                        const uint64_t* in_off_b, const uint64_t* in_len_b, uint32_t nstreams_b, const uint64_t* idx_first_b,
                                        const uint64_t* idx_start_b, const uint64_t* idx_pos_b, const uint64_t* idx_total_b,
                                        const int32_t* idx_tail_b, uint64_t nentries_b, const uint32_t* req_stream_a, const uint64_t* req_off_a,
                                        const uint64_t* req_len_a, const uint32_t* req_stream_b, const uint64_t* req_off_b,
                                        const uint64_t* req_len_b, uint32_t nreq, uint32_t flags, uint64_t max_rows, uint64_t scratch_cap,
                                        uint64_t* len_a, uint64_t* len_b, uint64_t* prefix, uint64_t* suffix, int32_t* status, void* d_work,
                                        uint64_t* d_result);

#ifdef __cplusplus
}
#endif
#endif /* SNAPPIER_HIP_FRAME_DIFF_H */

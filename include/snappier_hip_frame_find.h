/*
 * snappier_hip_frame_find.h -- C-ABI of libsnappier_hip_frame_find.so: device batch FIND in seekable Snappy framed streams -- where a byte
 * string occurs in windows of what the streams decode to.  The digest (snappier_hip_frame_digest.h) says whether two windows hold the same
 * bytes and the diff (snappier_hip_frame_diff.h) where they part; this call says WHERE IN THE DECODED BYTES A NEEDLE OCCURS: the offsets of
 * every record delimiter, the place of a key before an update, the number of matches for a filter -- with no decoded byte leaving the call.
 * The positions it gives are offsets into what the STREAM decodes to, so they go straight into req_off of snp_frame_read_indexed_batch
 * (snappier_hip_frame_index.h) and sp_off of the splice (snappier_hip_frame_splice.h).
 *
 * An extension of include/snappier_hip.h in a library of its own, linked against libsnappier_hip.so and taking that library's contexts (snp_ctx).
 * It adds no status code and no option, keeps no state in the context and reads no environment variable; the surfaces of snappier_hip.h and the
 * other extension headers are unchanged.  The C# side binds these functions in csharp/Snappier.Gpu/NativeMethodsFrameFind.cs.
 */
#ifndef SNAPPIER_HIP_FRAME_FIND_H
#define SNAPPIER_HIP_FRAME_FIND_H

#include "snappier_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SNP_FIND_MAX_NEEDLE 256u   /* the longest needle, in bytes */

/* Streams, index and requests are exactly those of snp_frame_read_indexed_batch (snappier_hip_frame_index.h): stream b is
 * in[in_off[b] .. +in_len[b]), its rows are [idx_first[b], idx_first[b + 1]) of idx_start / idx_pos, nentries = the rows the index arrays
 * hold; request r names the window [req_off[r], req_off[r] + req_len[r]) of stream req_stream[r], clipped to idx_total exactly as the read
 * clips it -- offset 0, length 2^64 - 1 is the whole stream.  Any number of requests may name one stream, in any order.
 * Needles.  Request r looks for the m = needle_len[r] bytes needles[needle_off[r] .. +m).  Two requests may share needle bytes, wholly or in
 * part.  m == 0 or m > SNP_FIND_MAX_NEEDLE is SNP_ERR_BAD_ARG for that request, which then owns no row and decodes nothing.
 *
 * Result of a request that is SNP_OK.  With [lo, hi) the clipped window, an OCCURRENCE is a decoded offset p with lo <= p, p + m <= hi and
 * decoded[p, p + m) == needle.  Occurrences may overlap each other: "aaa" occurs 3 times in "aaaaa".  win_len[r] = hi - lo; count[r] = the
 * number of all occurrences; nhits[r] = min(count[r], hit_cap[r]); hits[hit_off[r] .. +nhits[r]) = the first nhits[r] occurrences in
 * ascending order, AS OFFSETS INTO WHAT THE STREAM DECODES TO, NOT INTO THE WINDOW.  Nothing of hits beyond nhits[r] is written.  The hit
 * regions [hit_off[r], +hit_cap[r]) of different requests must not overlap.  hit_cap[r] = 0 makes a count-only request.  A window shorter
 * than m is SNP_OK with count 0 (if the read would be OK).  A request that is not SNP_OK has win_len = count = nhits = 0 and writes no hit.
 * The result is deterministic: no atomic decides an order.
 *
 * Checks and status.  THE INDEX IS UNTRUSTED INPUT, as in the read: index reads are bounded by nentries, header reads by in_len[b], every row
 * a request owns (the rows the read would select for its window) is checked against the header it points at, and nothing is written outside
 * hits[hit_off[r] .. +nhits[r]), win_len, count, nhits, status, d_result and d_work; nothing is read outside the streams, the index, the
 * needles and d_work.  status[r] is what snp_frame_read_indexed_batch gives for the same (stream, off, len) with an out_cap that holds the
 * window and bounds that admit it, in this order: SNP_ERR_BAD_ARG for a needle length that is not legal; what the read's plan refuses
 * (SNP_ERR_BAD_ARG for req_stream >= nstreams, for an idx_tail that is no status of the walk and for an index that does not hold the window;
 * SNP_ERR_OUTPUT_TOO_SMALL for a stream that was not indexed); SNP_ERR_BAD_ARG for a row that fails its check (then nothing of the request
 * is decoded); the status of the first chunk of the window, in stream order, that fails to decode or verify; the error that ended the
 * stream's walk (the strict tail rule).
 * EVERY CHUNK THE WINDOW MEETS IS DECODED WHOLE AND VERIFIED.  ZERO-LENGTH ROWS ARE NEVER DECODED.  A CORRUPT CHUNK OUTSIDE THE WINDOW IS NOT
 * NOTICED.
 *
 * Admission, in request order.  A request needs the rows it owns, which must fit max_rows, and the decoded bytes of those rows -- the edge
 * chunks whole -- which must fit scratch_cap, each counted together with the requests before it.  The first request that misses a bound, and
 * every later one, get SNP_ERR_OUTPUT_TOO_SMALL.  Both needs follow from the index's starts alone (a request's rows are consecutive: its
 * bytes are where its last row ends minus where its first begins), so SIZING TAKES ONE ROUND: call with max_rows = scratch_cap = 0; hits and
 * d_work may then be minimal (one element; the workspace of those bounds).  A request refused by its needle, its window or its plan counts
 * nothing; a request refused by a row check had its rows and bytes counted.  The sums saturate -- a request's rows count as no more than
 * 2^31 (max_rows is below that), the byte sum stops at 2^64 - 1 -- so an index filled with anything at all never wraps a sum into something
 * that passes admission.  scratch_cap above 2^40 - 1 counts as 2^40 - 1.
 * d_result (device, 4 x u64): [0] = rows needed, over all requests whatever was admitted; [1] = sum of count over the SNP_OK requests;
 * [2] = scratch bytes needed, over all requests; [3] = requests that are SNP_OK.
 * d_work must hold snp_frame_find_indexed_workspace(nreq, max_rows, scratch_cap) bytes (host arithmetic; 0 when nreq is 0): per-request words,
 * max_rows rows of a chunk table, per 16384 bytes of scratch_cap a tile's words, scratch_cap bytes and 32 more.  nreq must be below 2^30 and
 * max_rows below 2^31, else SNP_ERR_BAD_ARG (the workspace function then gives 0).  All arrays are device memory; the call only reads the
 * streams, the index and the needles.
 * How: each request's chunks are decoded one after the other into one run of the scratch arena, so a match across chunk boundaries is no
 * special case; the start positions of a window are cut into tiles of 16384 and workgroups take equal shares of consecutive tiles, 16 start
 * positions per lane and step, read 16 bytes at a time; a first pass counts, a scan ranks the tiles, a second pass over the tiles below
 * hit_cap writes the positions (frame_find.hip).
 * Stream capture: the call only enqueues on the context's stream -- no allocation, no read-back, no synchronisation -- under the rule of
 * snp_decompress_batch: make the same call once before the capture.  No option changes a result.
 * SNP_ERR_BAD_ARG for a null pointer (nreq == 0 needs only ctx and d_result, and still writes d_result), SNP_ERR_DEVICE for a runtime
 * failure. */
uint64_t snp_frame_find_indexed_workspace(uint32_t nreq, uint64_t max_rows, uint64_t scratch_cap);
snp_status snp_frame_find_indexed_batch(snp_ctx* ctx, const uint8_t* in, const uint64_t* in_off, const uint64_t* in_len, uint32_t nstreams,
                                        const uint64_t* idx_first, const uint64_t* idx_start, const uint64_t* idx_pos, const uint64_t* idx_total,
                                        const int32_t* idx_tail, uint64_t nentries, const uint32_t* req_stream, const uint64_t* req_off,
                                        const uint64_t* req_len, uint32_t nreq, const uint8_t* needles, const uint64_t* needle_off,
                                        const uint32_t* needle_len, uint64_t max_rows, uint64_t scratch_cap, uint64_t* hits,
                                        const uint64_t* hit_off, const uint64_t* hit_cap, uint64_t* win_len, uint64_t* count, uint64_t* nhits,
                                        int32_t* status, void* d_work, uint64_t* d_result);

#ifdef __cplusplus
}
#endif
#endif /* SNAPPIER_HIP_FRAME_FIND_H */

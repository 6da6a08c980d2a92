/*
 * snappier_hip_frame_verify.h -- C-ABI of libsnappier_hip_frame_verify.so: device batch VERIFY of seekable Snappy framed streams, chunk by
 * chunk, and the REPAIR PLAN that fetches the rotten chunks from a replica.  The calls that copy chunks they do not need to decode -- compose,
 * splice, edit, rechunk, recut, dedup, digest, diff -- copy a corrupt kept chunk as it is; a rechunk or recut with REWRITE_ALL is the scrub,
 * at compressor speed and with one status per stream.  snp_frame_verify_indexed_batch is the question on its own: every data chunk the index
 * lists is decoded and CRC-verified into a scratch of bounded size, NOTHING IS WRITTEN BUT VERDICTS, and the answer is one status per index
 * row.  snp_frame_repair_plan_batch turns those verdicts into the segment lists with which snp_frame_compose_indexed_batch
 * (snappier_hip_frame_compose.h) builds each stream again from its good chunks and a replica's bytes for the bad ones.
 *
 * An extension of include/snappier_hip.h in a library of its own, linked against libsnappier_hip.so and taking that library's contexts (snp_ctx).
 * It adds no status code and no option, keeps no state in the context and reads no environment; the surfaces of snappier_hip.h and the other
 * extension headers are unchanged.  The C# side binds these functions in csharp/Snappier.Gpu/NativeMethodsFrameVerify.cs.
 */
#ifndef SNAPPIER_HIP_FRAME_VERIFY_H
#define SNAPPIER_HIP_FRAME_VERIFY_H

#include "snappier_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SNP_VERIFY_NONE 0xffffffffffffffffull   /* first_bad of a stream with no bad row */
#define SNP_VERIFY_SKIPPED (-1)                 /* row_status of a row that was not looked at: no snp_status, all of which are >= 0 */

/* Stream s is in[in_off[s] .. +in_len[s]), as the sibling calls take it; idx_first, idx_start, idx_pos, idx_total, idx_tail and nentries are
 * the streams' index as snappier_hip_frame_index.h describes it, exactly as snp_frame_dedup_indexed_batch takes them.  Rows are numbered over
 * the whole index.  `in` and the index are only read.
 *
 * The verdict of a stream.  THE INDEX IS UNTRUSTED INPUT: idx_first values are clamped to nentries.  A stream whose idx_tail is not SNP_OK
 * gets that status; a value that is no status of the walk gives SNP_ERR_BAD_ARG.  SNP_ERR_BAD_ARG also for a stream whose idx_first runs
 * backwards: idx_first[s + 1] < idx_first[s], or idx_first[s] below the idx_first of a stream in front of it, as in the dedup.  A STREAM
 * THAT FAILS HERE IS NOT LOOKED AT: status[s] holds that verdict, nbad[s] = bad_bytes[s] = 0, first_bad[s] = SNP_VERIFY_NONE, and its rows
 * keep SNP_VERIFY_SKIPPED, as does every row that belongs to no stream that passed.  The other streams go on.
 *
 * row_status[nentries] (i32), for the rows of a stream that passed:
 *   SNP_ERR_BAD_ARG            the row fails the compose call's check of a kept row: the header at idx_pos is read again inside in_len and
 *                              must be a data chunk that decodes to exactly end - start bytes and ends inside the stream (a row ends where
 *                              the next one starts, the last at idx_total), and the next row's chunk lies at or behind the end of this
 *                              one's.  Such a row is not decoded.
 *   SNP_ERR_OUTPUT_TOO_SMALL   the row passed that check and is NOT VERIFIED: its length exceeds slot_bytes, or the call has no round (below).
 *                              A chunk that decodes to more than 65536 bytes -- legal in a foreign stream -- exceeds every slot_bytes: this
 *                              call never verifies it.
 *   anything else              what this library's framed decode gives that one chunk: the decoder's status, else SNP_ERR_CRC_MISMATCH when
 *                              the CRC-32C of what it decoded to is not the one its header carries, else SNP_OK.  A row of length 0 is
 *                              decoded and verified like any other (an uncompressed one must carry the CRC of nothing).
 * For an index that snp_frame_index_batch gave for the stream as it is now and chunks of at most slot_bytes, row_status is the status the
 * reference's frame decoder gives the identifier plus that chunk, and status[s] is SNP_OK exactly when it decodes the whole stream.
 * SKIPPABLE AND PADDING CHUNKS AND REPEATED IDENTIFIERS BETWEEN THE ROWS ARE NOT LOOKED AT, nor is anything behind the last row: the index
 * walk read their headers once, and they carry no CRC.
 *
 * Per stream (nstreams values each): status[s] = the stream's verdict if that is not SNP_OK, else the row_status of its first row in row
 * order that is not SNP_OK, else SNP_OK; nbad[s] = its rows that are not SNP_OK; first_bad[s] = the first of them (a global row number;
 * SNP_VERIFY_NONE when there is none); bad_bytes[s] = the sum of end - start over them (what a repair takes from a replica; a row that ends
 * below its start counts 0); flags[s] (u32): bit 0 is set when the stream's first 10 bytes are not the stream identifier -- for every
 * stream, whatever its verdict.
 *
 * Bounded scratch.  Decoded bytes go into the scratch at the end of d_work, in rounds: the slot stride is slot_bytes (1 .. 65536) rounded up
 * to 16, rows_per_round = min(scratch_cap / stride, nentries), rounds = ceil(nentries / rows_per_round), row i is decoded in round
 * i / rows_per_round into slot i % rows_per_round.  All of it is host arithmetic from the arguments: no read-back decides a launch count.
 * Results do not depend on scratch_cap (at or above the stride), on the context's decode layout options or on the run.  scratch_cap below
 * the stride, 0 in particular, is the SIZING CALL: it runs every check, decodes nothing and gives every row that passed its check
 * SNP_ERR_OUTPUT_TOO_SMALL; d_result[4] is then the slot_bytes to come again with.
 * d_result (device, 8 x u64): [0] = rows looked at (the rows of the streams that passed), [1] = those whose row_status is not SNP_OK,
 * [2] = decoded bytes verified (the lengths of the rows that are SNP_OK), [3] = streams whose status is SNP_OK, [4] = the largest length
 * among the rows that passed their check, [5] = rows left unverified (SNP_ERR_OUTPUT_TOO_SMALL), [6] = rounds, [7] = the sum of bad_bytes.
 * d_work must hold snp_frame_verify_indexed_workspace(nstreams, nentries, slot_bytes, scratch_cap) bytes (host arithmetic; 0 when nstreams is
 * 0 or >= 2^31, nentries >= 2^31 or slot_bytes is out of range): 46 bytes per row, 44 per stream, rows_per_round * stride of scratch, every
 * piece rounded up to 256.  All arrays are device memory.  Whatever the arrays hold, nothing is read outside a stream's bytes and nothing is
 * written outside the output arrays and d_work.
 * Stream capture: the call only enqueues on the context's stream -- no allocation, no read-back, no synchronisation -- under the rule of
 * snp_frame_read_indexed_batch.
 * How: frame_verify.hip -- a workgroup per stream checks its rows and fills one chunk table over all rows of the index, empty rows standing
 * in for rows that are skipped, failed or too long; a round is a slice of that table and one decode + CRC verify over it; one thread per row
 * folds the statuses into row_status; a workgroup per stream reduces its rows (sums, the minimum row number, a maximum).  No atomic is used.
 * SNP_ERR_BAD_ARG for slot_bytes outside 1 .. 65536, nstreams or nentries >= 2^31 and for a null pointer (nstreams == 0 needs only ctx and
 * d_result: it writes a zeroed d_result and nothing else; idx_start, idx_pos and row_status when nentries > 0), SNP_ERR_DEVICE for a
 * runtime failure. */
uint64_t snp_frame_verify_indexed_workspace(uint32_t nstreams, uint64_t nentries, uint32_t slot_bytes, uint64_t scratch_cap);
snp_status snp_frame_verify_indexed_batch(snp_ctx* ctx, const uint8_t* in, const uint64_t* in_off, const uint64_t* in_len, uint32_t nstreams,
                                          const uint64_t* idx_first, const uint64_t* idx_start, const uint64_t* idx_pos,
                                          const uint64_t* idx_total, const int32_t* idx_tail, uint64_t nentries, uint32_t slot_bytes,
                                          uint64_t scratch_cap, int32_t* row_status, int32_t* status, uint64_t* nbad, uint64_t* first_bad,
                                          uint64_t* bad_bytes, uint32_t* flags, void* d_work, uint64_t* d_result);

/* Row verdicts to compose recipes.  idx_first, idx_start, idx_total, idx_tail, nentries and nstreams are the streams' index (no positions:
 * the planner reads no stream), row_status what snp_frame_verify_indexed_batch gave for it; rep_total and rep_tail (nrep_streams values
 * each) are the idx_total and idx_tail of the replicas' index.  Pair j (nout of them) names stream rp_stream[j] and replica rp_replica[j].
 * Output j covers [0, idx_total[s]) of s = rp_stream[j]: a maximal run of rows whose row_status is SNP_OK is one segment of the stream
 * itself, a maximal run of rows with ANY other status (SNP_VERIFY_SKIPPED too) is one segment of the replica over the same decoded range.
 * Rows of length 0 (and rows that end below their start) are dropped.  A segment runs from its first row's idx_start to the idx_start of
 * the row that begins the next segment, the last to idx_total.  A stream with no bad row is one segment; one with no byte has none.
 * Source numbering: stream s is source s, replica t is source nstreams + t -- the caller composes from the streams followed by the
 * replicas.  THE INDEX AND row_status ARE UNTRUSTED INPUT: idx_first values are clamped to nentries, and the compose call checks every
 * segment against the sources.
 * plan_status[j] = SNP_ERR_BAD_ARG, and no segments, for a pair out of range (rp_stream[j] >= nstreams or rp_replica[j] >= nrep_streams), a
 * stream whose idx_tail is not SNP_OK or whose idx_first runs backwards (idx_first[s + 1] < idx_first[s]), a replica whose tail is not
 * SNP_OK and a replica whose total differs from the stream's.
 * The recipes are in the compose call's CSR form: seg_first[nout + 1], and seg_stream, seg_off, seg_len with max_segs values each.
 * Admission, in pair order over the pairs that passed: counted, each with the pairs before it, the segments against max_segs.  The first
 * pair that misses the bound, and every later one, get SNP_ERR_OUTPUT_TOO_SMALL and no segments.  max_segs = 0 is the
 * sizing call.  Every place in the CSR comes from a scan; results are the same in every run.
 * d_result (device, 4 x u64): [0] = segments needed, [2] = decoded bytes taken from replicas, [3] = decoded bytes kept -- these three over
 * the pairs that passed, admitted or not; [1] = pairs whose plan_status is SNP_OK.
 * d_work must hold snp_frame_repair_plan_workspace(nout) bytes (host arithmetic; 0 when nout is 0 or >= 2^31): 44 bytes per pair, every
 * piece rounded up to 256.  All arrays are device memory.  Stream capture: as above.
 * How: frame_verify.hip -- a workgroup per pair walks the stream's rows in tiles of 256; the row that takes part before a row comes from a
 * ballot, a segment's number from a scan; a second walk writes the admitted pairs' segments.  No atomic is used.
 * SNP_ERR_BAD_ARG for nout, nstreams, nrep_streams or nentries >= 2^31 and for a null pointer (nout == 0 needs only ctx and d_result: it
 * writes a zeroed d_result and nothing else; the index arrays when nstreams > 0, idx_start and row_status when also nentries > 0, rep_total
 * and rep_tail when nrep_streams > 0, seg_stream, seg_off and seg_len when max_segs > 0), SNP_ERR_DEVICE for a runtime failure. */
uint64_t snp_frame_repair_plan_workspace(uint32_t nout);
snp_status snp_frame_repair_plan_batch(snp_ctx* ctx, const uint64_t* idx_first, const uint64_t* idx_start, const uint64_t* idx_total,
                                       const int32_t* idx_tail, uint64_t nentries, uint32_t nstreams, const int32_t* row_status,
                                       const uint64_t* rep_total, const int32_t* rep_tail, uint32_t nrep_streams, const uint32_t* rp_stream,
                                       const uint32_t* rp_replica, uint32_t nout, uint32_t max_segs, uint64_t* seg_first,
                                       uint32_t* seg_stream, uint64_t* seg_off, uint64_t* seg_len, int32_t* plan_status, void* d_work,
                                       uint64_t* d_result);

#ifdef __cplusplus
}
#endif
#endif /* SNAPPIER_HIP_FRAME_VERIFY_H */

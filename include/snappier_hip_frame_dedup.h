/*
 * snappier_hip_frame_dedup.h -- C-ABI of libsnappier_hip_frame_dedup.so: device batch DEDUP of seekable Snappy framed streams by chunk.  One call
 * finds the duplicate chunks of a batch on the device, proves them equal byte for byte, writes the unique chunks of the new streams once into a
 * PACK -- a valid framed stream with its own chunk index -- and hands back, per new stream, the segment list (its RECIPE) with which
 * snp_frame_compose_indexed_batch (snappier_hip_frame_compose.h) rebuilds it from the base streams and the pack.  N versions of a buffer, a
 * batch of logs that share records, a backup that grew by an insert: with content-defined chunks (snappier_hip_frame_cuts.h) equal content is
 * equal chunks wherever it lies, and the compressor is deterministic, so equal pieces are equal chunk bytes.  Nothing is decoded.
 *
 * An extension of include/snappier_hip.h in a library of its own, linked against libsnappier_hip.so and taking that library's contexts (snp_ctx).
 * It adds no status code and no option, keeps no state in the context and reads no environment; the surfaces of snappier_hip.h and the other
 * extension headers are unchanged.  The C# side binds these functions in csharp/Snappier.Gpu/NativeMethodsFrameDedup.cs.
 */
#ifndef SNAPPIER_HIP_FRAME_DEDUP_H
#define SNAPPIER_HIP_FRAME_DEDUP_H

#include "snappier_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SNP_DEDUP_NONE 0xffffffffffffffffull    /* canon of a row that takes no part */

/* Stream s is in[in_off[s] .. +in_len[s]), as the sibling calls take it; idx_first, idx_start, idx_pos, idx_total, idx_tail and nentries are
 * the streams' index as snappier_hip_frame_index.h describes it.  Rows are numbered over the whole index.  The first nbase streams
 * (0 .. nstreams) are the BASE: data that is stored already, for example earlier packs; the other nnew = nstreams - nbase streams are NEW.
 * `in` and the index are only read; the pack goes to out[0 .. out_cap), which must not overlap `in`.
 *
 * The verdict of a stream.  THE INDEX IS UNTRUSTED INPUT: idx_first values are clamped to nentries.  A stream whose idx_tail is not SNP_OK gets
 * that status; a value that is no status of the walk gives SNP_ERR_BAD_ARG.  SNP_ERR_BAD_ARG also for a stream whose idx_first runs backwards
 * -- idx_first[s + 1] < idx_first[s], or idx_first[s] below the idx_first of a stream in front of it (it would share rows with that stream) --
 * and for one with a row that fails the compose call's check of a kept row: the header at idx_pos is read again inside in_len and must be a
 * data chunk that decodes to exactly end - start bytes and ends inside the stream (a row ends where the next one starts, the last at
 * idx_total), and the next row's chunk lies at or behind the end of this one's.  status[s] (nstreams values) holds the verdict.  A STREAM THAT
 * FAILS IS DEDUP'ED NOT AT ALL: it offers no row to any other stream and gets no recipe.  The other streams go on.  Whatever the arrays hold,
 * nothing is read outside a stream's bytes and nothing is written outside the output arrays.
 *
 * The map.  A row TAKES PART when its stream passed and it decodes to at least one byte.  Its KEY is the pair (decoded length, the CRC field of
 * its chunk header).  The LEADER of a key is the smallest row number among the rows that have it.  canon[r] (nentries values) is
 *   r itself                for a leader;
 *   the leader              for any other row whose chunk is BYTE-IDENTICAL to the leader's: the whole 4 + size bytes, header, CRC and payload;
 *   r itself                for any other row that is not: a key collision, or the same content in another encoding;
 *   SNP_DEDUP_NONE          for a row that takes no part (length 0, a failed stream, no stream).
 * NO PAIR IS EVER MERGED ON THE CRC ALONE.  canon is written in every call, the sizing call included, and does not depend on admission.
 * THE RULE IS ONE ROUND: two equal rows behind a different leader with the same key both stay unmerged.  That costs ratio, never data.  Two
 * rows of different content and equal length collide with probability 2^-32, so among n rows of one length about n^2 / 2^33 pairs do: one
 * expected pair at 93 000 rows of one length, and then the few rows equal to the loser are stored once each instead of once.
 * canon and everything derived from it are the same in every run.
 *
 * The pack is one framed stream: the 10-byte identifier, then the chunks of all rows with canon[r] == r that belong to ADMITTED NEW streams,
 * verbatim, in row order.  Base rows are never written.  out_len[0] is its length; with nothing to store it is the identifier alone
 * (out_len = 10); with out_cap < 10 nothing is written, out_len = 0 and pk_tail = SNP_ERR_OUTPUT_TOO_SMALL.  Its index comes with it:
 * pk_first[2] = {0, rows}, pk_start and pk_pos (max_entries rows each; rows at and above pk_first[1] are not written), pk_total[1],
 * pk_tail[1] -- array for array what snp_frame_index_batch gives for the pack, so the pack goes straight into the read, digest, diff, find
 * and compose calls, and into the next dedup as a base stream.
 *
 * The recipes are in the compose call's CSR form: seg_first[nnew + 1], and seg_stream, seg_off, seg_len with max_segs values each.  Source
 * numbering: base stream s is source s, the pack is source nbase; the caller composes from the base streams plus the pack.  A row that takes
 * part stands for its canonical row's decoded range: in a base stream from that row's idx_start, in the pack from the decoded bytes of the
 * packed rows before it.  Neighbouring rows of one new stream are one segment when they have the same source and their ranges are contiguous,
 * so a stream with no duplicate is one segment.  Rows of length 0 are dropped.  A new stream that is not admitted has no segment.
 * Composing a recipe at any chunk_bytes decodes to the original stream with nothing decoded on the way (every row is kept), and the framed
 * bytes are the original's byte for byte for a stream that is the identifier plus non-empty data chunks -- every stream this library's
 * encoders write.
 *
 * Admission, in stream order over the new streams that passed.  Counted, each with the streams before it: the unique rows against
 * max_entries, 10 + their chunk bytes against out_cap, the segments against max_segs.  The first stream that misses a bound, and every later
 * one, get SNP_ERR_OUTPUT_TOO_SMALL and no segments.  A canonical row is always an earlier row, so every admitted recipe is whole.
 * max_entries = max_segs = out_cap = 0 is the sizing call.
 * d_result (device, 8 x u64), [0] .. [2] and [4] .. [7] over the new streams that passed, admitted or not: [0] = unique rows, [1] = pack
 * bytes (10 + their chunk bytes), [2] = segments, [3] = streams whose status is SNP_OK (base streams too), [4] = rows that take part,
 * [5] = rows merged into a leader, [6] = rows with a leader's key but other bytes, [7] = the chunk bytes the merged rows would have taken.
 * d_work must hold snp_frame_dedup_indexed_workspace(nstreams, nentries) bytes (host arithmetic; 0 when nstreams is 0 or nentries >= 2^31):
 * 80 bytes per row, 12 per slot of a table of the next power of two at or above 2 * nentries (at least 64), 36 per stream, every piece
 * rounded up to 256.  All arrays are device memory.
 * Stream capture: the call only enqueues on the context's stream -- no allocation, no read-back, no synchronisation -- under the rule of
 * snp_frame_read_indexed_batch.
 * How: frame_dedup.hip -- a workgroup per stream walks its rows; one thread per row claims its key's slot in an open-addressing table by a
 * 64-bit compare-and-swap and lowers the slot's row by an atomic minimum, whose result does not depend on the order of arrival; a wavefront
 * per non-leader row compares the two chunks 16 bytes per lane; scans over the rows give every place in the pack and in the recipes; a
 * wavefront per unique row copies its chunk.  No atomic decides an order or a value of an output.
 * SNP_ERR_BAD_ARG for nbase > nstreams, nstreams or nentries >= 2^31 and for a null pointer (nstreams == 0 needs only ctx and d_result: it
 * writes a zeroed d_result and nothing else; idx_start, idx_pos and canon when nentries > 0, out when out_cap > 0, pk_start and pk_pos when
 * max_entries > 0, seg_stream, seg_off and seg_len when max_segs > 0), SNP_ERR_DEVICE for a runtime failure. */
uint64_t snp_frame_dedup_indexed_workspace(uint32_t nstreams, uint64_t nentries);
snp_status snp_frame_dedup_indexed_batch(snp_ctx* ctx, const uint8_t* in, const uint64_t* in_off, const uint64_t* in_len, uint32_t nstreams,
                                         const uint64_t* idx_first, const uint64_t* idx_start, const uint64_t* idx_pos,
                                         const uint64_t* idx_total, const int32_t* idx_tail, uint64_t nentries, uint32_t nbase,
                                         uint32_t max_entries, uint32_t max_segs, uint64_t out_cap, uint8_t* out, uint64_t* out_len,
                                         int32_t* status, uint64_t* canon, uint64_t* pk_first, uint64_t* pk_start, uint64_t* pk_pos,
                                         uint64_t* pk_total, int32_t* pk_tail, uint64_t* seg_first, uint32_t* seg_stream, uint64_t* seg_off,
                                         uint64_t* seg_len, void* d_work, uint64_t* d_result);

#ifdef __cplusplus
}
#endif
#endif /* SNAPPIER_HIP_FRAME_DEDUP_H */

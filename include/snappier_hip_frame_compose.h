/*
 * snappier_hip_frame_compose.h -- C-ABI of libsnappier_hip_frame_compose.so: device batch COMPOSE of seekable Snappy framed streams: new streams
 * made of windows of old ones, through the old streams' chunk index.  The read, update, append, splice and rechunk calls
 * (snappier_hip_frame_index.h, _update.h, _append.h, _splice.h, _rechunk.h) stay inside one stream, and the only bytes that enter a stream there
 * are raw bytes.  This call moves COMPRESSED data between streams: concatenating streams, splitting one at a record boundary, extracting a window
 * as a stream of its own, moving a record from one log to another, interleaving two streams.  A chunk that lies inside a window is copied
 * untouched; only the chunk a window cuts at its head and the one it cuts at its tail are decoded and the parts inside the window compressed
 * again.  Nothing is read back between the decode and the compress.
 *
 * An extension of include/snappier_hip.h in a library of its own, linked against libsnappier_hip.so and taking that library's contexts (snp_ctx).
 * It adds no status code and no option and keeps no state in the context; the surfaces of snappier_hip.h and the other extension headers are
 * unchanged.  The C# side binds these functions in csharp/Snappier.Gpu/NativeMethodsFrameCompose.cs.
 */
#ifndef SNAPPIER_HIP_FRAME_COMPOSE_H
#define SNAPPIER_HIP_FRAME_COMPOSE_H

#include "snappier_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Source stream s is in[in_off[s] .. +in_len[s]), as the sibling calls take it; idx_first, idx_start, idx_pos, idx_total, idx_tail and nentries
 * are the sources' index as snappier_hip_frame_index.h describes it.  Output stream j is made of the SEGMENTS [seg_first[j], seg_first[j + 1])
 * (seg_first holds nout + 1 values), one behind the other; segment g stands for the decoded bytes [seg_off[g], seg_off[g] + seg_len[g]) of
 * source seg_stream[g] (lo, hi below).  A source may be named any number of times, and segments of one output or of different outputs may
 * overlap.  chunk_bytes (1 .. 65536, cb below) holds for the whole call.  Out of place: `in`, the old index and the segment list are only read;
 * output j goes to out[out_off[j] .. +out_cap[j]), which must not overlap `in`.
 *
 * The rows of a segment.  The source's rows are [f0, f1) (clamped to nentries); a row ends where the next one starts, the last at idx_total.
 * r0 is the first row that ends above lo, r1 the first row at or behind r0 that starts at or above hi -- the read call's and the splice's rule.
 * A segment of length 0 contributes nothing, and nothing of the index is looked at for it beyond seg_stream[g] < nstreams.  So zero-length rows
 * at a border of a segment are never taken; zero-length rows strictly inside it are taken and copied like any kept row (a new row's old row
 * stays a subtraction, not a search; the rechunk is what drops them).
 *
 * Edges.  Row r0 is the HEAD EDGE when it starts below lo, row r1 - 1 the TAIL EDGE when it ends above hi.  Both may be the same row: it is
 * decoded once and its region is [lo, hi).  An edge's chunk is decoded and CRC-verified whole into staging; one that decodes to more than 65536
 * bytes gives SNP_ERR_BAD_ARG.  The part of the edge inside the segment is cut into pieces of cb bytes, the last one shorter; each piece is one
 * slot of snp_frame_encode_chunked_batch (snappier_hip_frame_chunked.h): what CompressBlock makes of it with the context's hash variant -- type
 * 0x00 with varint || fragment when that is smaller than the piece, else type 0x01 with the piece -- and the masked CRC-32C of the piece.  The
 * compressor reads a piece where its edge was decoded to, at lo - start + k cb: there is no assemble pass.
 * THE EDGES OF NEIGHBOURING SEGMENTS ARE NOT MERGED INTO ONE REGION: a segment is planned on its own, in one pass, so two segments that meet
 * inside a chunk leave two short chunks.  This fragmentation is what snp_frame_rechunk_indexed_batch is for.
 *
 * Kept rows.  Every other row of [r0, r1) is KEPT: its chunk in[pos .. pos + 4 + size) of the source is copied verbatim, never decoded; size
 * comes from its header, read again inside the source's in_len.
 *
 * The output stream is the 10-byte identifier, then for each segment in order its head pieces, its kept chunks and its tail pieces.
 * EVERYTHING THAT IS NOT A DATA CHUNK OF THE INDEX IS DROPPED: SKIPPABLE, PADDING AND REPEATED-IDENTIFIER CHUNKS.  An output with no segment, or
 * with only empty ones, is the identifier alone (out_len = 10, SNP_OK).
 * So, byte for byte:
 *   (a) with sources that snp_frame_encode_chunked_batch wrote with chunk_bytes = cb, every lo a multiple of cb, and every segment of an output
 *       but its last of a length that is a multiple of cb (also when it ends at its source's total): the output is exactly that encoder's output
 *       for the concatenated decoded bytes -- whole-stream concatenation of streams of k cb bytes, a split at a grid point, an aligned extract;
 *   (b) any compose followed by snp_frame_rechunk_indexed_batch to cb is that encoder's output for the concatenation: with
 *       SNP_RECHUNK_REWRITE_ALL for any source, without it for sources this library wrote with the context's hash variant;
 *   (c) any other compose decodes to the concatenation; short chunks are possible at the borders of segments.
 * A CORRUPT KEPT CHUNK IS COPIED AS IT IS, NOT NOTICED.  A RECHUNK WITH SNP_RECHUNK_REWRITE_ALL IS THE SCRUB.
 *
 * The new index.  new_first[nout + 1], new_total[nout] and new_tail[nout] are per OUTPUT; new_start and new_pos hold max_entries rows each.  An
 * output that was written gets one row per piece and per kept chunk: start is the running decoded offset in the output, pos where the chunk
 * lies (the first at 10); new_total[j] is the sum of its segments' lengths and new_tail[j] = SNP_OK.  The arrays are, array for array, what
 * snp_frame_index_batch gives for the new streams: they go straight into the read, update, append, splice and rechunk calls and into the next
 * compose.  AN OUTPUT IS COMPOSED WHOLE OR NOT AT ALL: one that fails has no rows, new_total[j] = 0, new_tail[j] = status[j], out_len[j] = 0 and
 * its out range untouched; the other outputs go on.  Rows at and above new_first[nout] are not written.
 *
 * THE INDEX AND THE SEGMENT LIST ARE UNTRUSTED INPUT.  seg_first values are clamped to nsegs, idx_first values to nentries.  SNP_ERR_BAD_ARG for
 * an output whose seg_first runs backwards, and for a segment with seg_stream >= nstreams, with lo + len wrapping or above idx_total, with
 * f1 < f0 for its source, or with decoded bytes and no row that holds them.  A source whose idx_tail is not SNP_OK gives that status to every
 * output that names it with a segment of positive length; a value that is no status of the walk gives SNP_ERR_BAD_ARG.  EVERY row a segment
 * touches, kept or edge, has its header read again inside the source's in_len and must be a data chunk that decodes to exactly end - start
 * bytes and ends inside the stream; within a segment each chunk lies at or behind the end of the chunk before it, and a kept row lies inside
 * [lo, hi).  Any failed check: SNP_ERR_BAD_ARG.  An output gets the status of its first failing segment in segment order.  An edge that fails to
 * decode or verify gives its output that chunk's status -- the first such edge in segment order, within a segment the head edge first.
 * Whatever the arrays hold, nothing is read outside a source's bytes, and nothing is written outside out[out_off[j] .. +out_cap[j]), the new
 * index arrays and the per-output arrays.
 *
 * Admission, in output order over the outputs that passed the checks above.  Counted, each with the outputs before it: the edge rows and the
 * pieces, each against max_slots (one bound serves the decode table and the compressor table, as in the rechunk); the decoded bytes of the
 * edges against stage_cap; the rows of the new index against max_entries.  The first output that misses a bound, and every later one, get
 * SNP_ERR_OUTPUT_TOO_SMALL; so does an output whose new size exceeds out_cap[j] (this can hit one output in the middle of a batch; the others
 * go on).
 * d_result (device, 6 x u64): [0] = the larger of the edge rows and the pieces needed, [1] = sum of out_len, [2] = staging bytes needed,
 * [3] = outputs written, [4] = rows of the new index needed, [5] = kept chunks copied (of the outputs written).  [0], [2] and [4] count the
 * outputs that passed the checks; a segment or an output that needs 2^32 rows or slots or more is counted as 2^32, an output that needs 2^48
 * staging bytes or more as 2^48.
 * max_slots = stage_cap = 0 is the sizing call: it decodes nothing.  out_bound (nullable, nout x u64): for an output that passed the checks, from
 * the headers alone, 10 + the sum of 4 + size over its kept chunks + the sum of 8 + piece over its pieces -- it always holds the new stream; 0
 * for the others (also for an output whose edge failed to decode in this call).
 * d_work must hold snp_frame_compose_indexed_workspace(nstreams, nout, nsegs, max_slots, stage_cap, chunk_bytes, max_entries) bytes (host
 * arithmetic; 0 when nout is 0 or chunk_bytes is out of range): about 170 bytes per segment, 130 per output, 90 per slot, 20 per new row,
 * stage_cap of staging and snp_max_compressed_length(chunk_bytes) + 32 of compressed staging per slot.  All arrays are device memory.
 * Stream capture: the call only enqueues on the context's stream -- no allocation, no read-back, no synchronisation -- under the rule of
 * snp_frame_encode_buffers_batch: make the same call, with the same max_slots, once before the capture.
 * How: frame_compose.hip -- a workgroup per segment walks its rows (the headers, edge or kept), scans over the segments (an output's share of a
 * count is a difference), a join per output, the admission scans, a decode table of max_slots rows (cleared, then one thread per edge) and ONE
 * decode over it, a slot table of max_slots rows (one thread per piece) with ONE compressor and ONE CRC launch, the verdicts, one thread per new
 * row (its output, its segment by a search over the row counts, then a subtraction: a kept chunk or a slot), a scan of the chunk sizes, and an
 * emit whose workgroups each take the chunks of 64 KiB of a new stream: a copy from `in`, or header plus payload from staging.
 * SNP_ERR_BAD_ARG for chunk_bytes of 0 or above 65536, for nout, nsegs or nstreams >= 2^31 and for a null pointer (nout == 0 needs only ctx and
 * d_result: it writes a zeroed d_result and nothing else; out_bound is optional, the segment arrays when nsegs > 0, in and the index when
 * nstreams > 0, idx_start / idx_pos when nentries > 0, new_start / new_pos when max_entries > 0), SNP_ERR_DEVICE for a runtime failure. */
uint64_t snp_frame_compose_indexed_workspace(uint32_t nstreams, uint32_t nout, uint32_t nsegs, uint32_t max_slots, uint64_t stage_cap,
                                             uint32_t chunk_bytes, uint32_t max_entries);
snp_status snp_frame_compose_indexed_batch(snp_ctx* ctx, const uint8_t* in, const uint64_t* in_off, const uint64_t* in_len, uint32_t nstreams,
                                           const uint64_t* idx_first, const uint64_t* idx_start, const uint64_t* idx_pos,
                                           const uint64_t* idx_total, const int32_t* idx_tail, uint64_t nentries,
                                           const uint64_t* seg_first, const uint32_t* seg_stream, const uint64_t* seg_off, const uint64_t* seg_len,
                                           uint32_t nout, uint32_t nsegs, uint32_t chunk_bytes, uint32_t max_slots, uint64_t stage_cap,
                                           uint32_t max_entries, uint8_t* out, const uint64_t* out_off, const uint64_t* out_cap, uint64_t* out_len,
                                           int32_t* status, uint64_t* new_first, uint64_t* new_start, uint64_t* new_pos, uint64_t* new_total,
                                           int32_t* new_tail, uint64_t* out_bound, void* d_work, uint64_t* d_result);

#ifdef __cplusplus
}
#endif
#endif /* SNAPPIER_HIP_FRAME_COMPOSE_H */

/*
 * snappier_hip_frame_recut.h -- C-ABI of libsnappier_hip_frame_recut.so: device batch RECUT of seekable Snappy framed streams -- rechunk to a
 * caller's cut list -- through their chunk index.  Content-defined chunks (snappier_hip_frame_cuts.h) sit where the content puts them only while
 * nothing edits the stream: the append writes a grid, the splice, edit, update and compose calls leave short chunks and grid pieces at their
 * edges, and the one canonicaliser there was (snappier_hip_frame_rechunk.h) goes to the grid k * chunk_bytes.  This call brings a stream to what
 * snp_frame_encode_cuts_batch writes for its decoded bytes and a given cut list -- the finder's for the edited bytes, the record boundaries, or a
 * grid -- and compresses again only the pieces that no old chunk already is.  After an edit of a content-defined stream that is a few chunks
 * around the edit; a grid store is converted with every piece rebuilt.  Nothing is read back between the decode and the compress.
 *
 * An extension of include/snappier_hip.h in a library of its own, linked against libsnappier_hip.so and taking that library's contexts (snp_ctx).
 * It adds no status code and no option, keeps no state in the context and reads no environment; the surfaces of snappier_hip.h and the other
 * extension headers are unchanged.  The C# side binds these functions in csharp/Snappier.Gpu/NativeMethodsFrameRecut.cs.
 */
#ifndef SNAPPIER_HIP_FRAME_RECUT_H
#define SNAPPIER_HIP_FRAME_RECUT_H

#include "snappier_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* flags bit 0: every row is dirty -- the whole stream is decoded, verified and compressed again.  The scrub. */
#define SNP_RECUT_REWRITE_ALL 1u

/* Stream b is in[in_off[b] .. +in_len[b]), as the sibling calls take it; idx_first, idx_start, idx_pos, idx_total, idx_tail and nentries are its
 * batch's index as snappier_hip_frame_index.h describes it -- the arguments of snp_frame_rechunk_indexed_batch, with the cut list in the place of
 * chunk_bytes.  flags holds for the whole call.  Out of place: `in`, the old index and the list are only read; the new stream of b goes to
 * out[out_off[b] .. +out_cap[b]), which must not overlap `in`.
 *
 * PIECES.  Stream b decodes to total = idx_total[b] bytes.  Its cuts are cuts[cut_first[b] .. cut_first[b + 1]) (cut_first: nstreams + 1 values,
 * cuts: ncuts values, as snp_frame_encode_cuts_batch takes them and snp_content_cuts_batch writes them), relative to the stream's first decoded
 * byte; its pieces are the intervals between neighbours of {0} + cuts + {total}.  A stream that decodes to nothing has no piece and no cut.
 *
 * The CANONICAL stream of b is what snp_frame_encode_cuts_batch writes for the stream's decoded bytes and that list: the 10-byte identifier,
 * then one data chunk per piece, back to back, and nothing else.  A stream that decodes to nothing is the identifier only, also when
 * in_len[b] == 0.
 *
 * KEPT AND REBUILT PIECES.  The stream's rows are [f0, f1) (clamped to nentries); a row ends where the next one starts, the last at idx_total.
 * A row [s, e) of positive length is CLEAN when s is 0 or a cut, e is a cut or total, and no cut lies strictly inside: one binary search in
 * the stream's list.  A piece is KEPT when a clean row starts where it starts -- the read call's search: the first row that ends above the
 * piece's start -- and then its chunk's bytes in[pos .. pos + 4 + size) are copied verbatim, never decoded.  Every other piece is REBUILT.
 * The rows that are not clean, the DIRTY rows (every zero-length row is one), cover exactly the rebuilt pieces, in order, because the clean rows
 * are whole pieces of a partition; they are decoded and CRC-verified whole into staging, one behind the other, which is where the rebuilt pieces
 * lie one behind the other.  Each rebuilt piece is one slot of the chunked encoder: what CompressBlock makes of it with the context's hash
 * variant -- type 0x00 with varint || fragment when that is smaller than the piece, else type 0x01 with the piece -- and the masked CRC-32C of
 * the piece.  A dirty row of more than 65536 decoded bytes gives SNP_ERR_BAD_ARG.  Zero-length rows vanish.  EVERYTHING THAT IS NOT A DATA
 * CHUNK OF THE INDEX IS DROPPED: SKIPPABLE, PADDING AND REPEATED-IDENTIFIER CHUNKS, WHEREVER THEY LIE.  flags & SNP_RECUT_REWRITE_ALL makes
 * every row dirty.
 * So, byte for byte:
 *   (a) with cuts = k * cb (every multiple of cb inside (0, total)), out, out_len, status, the five new-index arrays, out_bound and
 *       d_result[1], [3], [4], [5] are snp_frame_rechunk_indexed_batch's at chunk_bytes = cb, with and without the flag;
 *   (b) with SNP_RECUT_REWRITE_ALL, any indexed stream becomes exactly snp_frame_encode_cuts_batch's output for its decoded bytes and the list,
 *       index arrays included;
 *   (c) the same without the flag for a stream whose data chunks were all written by this library with the context's hash variant -- at any
 *       chunking, after any of the update, append, splice, edit, compose or rechunk calls: a chunk's bytes depend only on its piece;
 *   (d) any other stream decodes to the same bytes, with its data chunks at exactly the given cuts.
 * A CORRUPT KEPT CHUNK IS COPIED AS IT IS, NOT NOTICED.  SNP_RECUT_REWRITE_ALL IS THE SCRUB.
 *
 * A stream that is already canonical is LEFT ALONE, as the sibling calls leave a stream that is not named: SNP_OK, out_len[b] = 0, nothing
 * written, its old rows in the new index.  Without the flag "canonical" is structural, read from the index, the headers and the list alone: the
 * list is good; every row is clean (so there is no zero-length row); pos[f0] == 10 and in[0, 10) is the identifier; pos[r + 1] == pos[r] + 4 +
 * size for every row and the last chunk ends at in_len[b]; with idx_total[b] == 0, no row, no cut, in_len[b] == 10 and the identifier.  With
 * the flag every stream is written.
 *
 * The new index.  new_first[nstreams + 1], new_total[nstreams] and new_tail[nstreams] are per stream; new_start and new_pos hold max_entries
 * rows each.  A written stream gets one row per piece with start = where the piece starts and pos where the chunk lies (the first at 10);
 * new_total[b] = idx_total[b] and new_tail[b] = SNP_OK.  Any other stream keeps its old rows, total and tail.  When the old index is what
 * snp_frame_index_batch gives, the new arrays are, array for array, what it gives for the resulting streams (the old one where a stream is not
 * written): they go straight into the read, digest, diff, find, dedup, update, append, splice, edit and compose calls and into the next recut.
 * Rows at and above new_first[nstreams] are not written.
 *
 * BOTH THE INDEX AND THE LIST ARE UNTRUSTED INPUT.  The index checks are the rechunk's: idx_first values are clamped to nentries; a stream whose
 * idx_tail is not SNP_OK gets that status, a value that is no status of the walk gives SNP_ERR_BAD_ARG; the rows of a stream must partition
 * [0, idx_total): start[f0] == 0, no row ends below its start, no decoded bytes without a row; positions strictly increase and no chunk
 * overlaps the next; EVERY row, kept or dirty, has its header read again inside in_len[b] -- a kept chunk's size comes from there -- and must
 * be a data chunk that decodes to exactly end - start bytes.  Any failed check, and f1 < f0: SNP_ERR_BAD_ARG.  The list checks are the
 * encoder's (snp_frame_encode_cuts_batch), with idx_total[b] in the place of in_len[b]: cut_first[b] <= cut_first[b + 1] <= ncuts; the cuts
 * strictly ascending inside (0, total); no piece above 65536 bytes; every read of `cuts` is below ncuts.  A bad list is SNP_ERR_BAD_ARG for
 * that stream alone: it counts nothing towards admission and keeps its old rows.  A dirty chunk that fails to decode or verify gives its
 * stream the status of the first such chunk in stream order.  A stream is recut whole or not at all: one that fails has out_len[b] = 0, its
 * out range untouched and its old rows.  Whatever the arrays hold, nothing is read outside a stream's bytes or cuts[0, ncuts), and nothing is
 * written outside out[out_off[b] .. +out_cap[b]), the new index arrays and the per-stream arrays; with an idx_first that claims more rows than
 * max_entries holds, the rows of streams that are not written are cut off at max_entries and new_first stays at that.
 *
 * Admission, in stream order over the streams that passed the checks above and are not left alone.  Counted, each with the streams before it:
 * the dirty rows and the rebuilt pieces, each against max_slots (one bound serves the decode table and the compressor table); the staging
 * against stage_cap -- ONE budget for both stagings: what the stream's dirty rows decode to plus, over its rebuilt pieces, the compressed
 * staging of each, (38 + p + p / 6 + 15) / 16 * 16 + 16 bytes for a piece of p bytes (a fixed stride at the largest piece would cost several
 * times the input at content-defined sizes); 2 * dbytes + dbytes / 6 + 69 * rebuilt always holds it, with dbytes the decoded bytes of the dirty
 * rows; and the rows of the new index against max_entries -- here EVERY stream of the batch counts, one that is to be written with the larger
 * of its old and its new row count, any other with its old rows, so that the rows fit whatever becomes of a stream.  The first stream that
 * misses a bound, and every later one that needs work, get SNP_ERR_OUTPUT_TOO_SMALL; so does a stream whose new size exceeds out_cap[b] (this
 * can hit one stream in the middle of a batch; the others go on).
 * d_result (device, 8 x u64): [0] = the larger of the decode rows and the compressor slots needed, [1] = sum of out_len over the written
 * streams, [2] = staging bytes needed, as defined above, [3] = streams written, [4] = rows of the new index needed (counted as above),
 * [5] = streams left alone as canonical, [6] = chunks copied and [7] = pieces rebuilt, both over the written streams.  A stream that needs
 * 2^32 rows or slots or more is counted as 2^32, one that needs 2^48 staging bytes or more as 2^48.
 * max_slots = stage_cap = 0 is the sizing call: it decodes nothing.  out_bound (nullable, nstreams x u64): for a stream that passed the checks
 * and is not left alone, from the headers alone, 10 + the sum over its pieces of 4 + size (kept) or 8 + piece (rebuilt) -- it always holds the
 * new stream; 0 for the others (also for a stream whose dirty chunk failed to decode in this call).
 * d_work must hold snp_frame_recut_indexed_workspace(nstreams, max_slots, stage_cap, max_entries) bytes (host arithmetic; 0 when nstreams is
 * 0): about 250 bytes per stream, 120 per slot, 20 per new row, and stage_cap + 64 * max_slots + 256 of staging -- the 64 bytes are what the
 * compressor may touch of a slot that stays empty.  All arrays are device memory.
 * Stream capture: the call only enqueues on the context's stream -- no allocation, no read-back, no synchronisation -- under the rule of
 * snp_frame_encode_buffers_batch: make the same call, with the same max_slots, once before the capture.
 * How: frame_recut.hip -- a workgroup per stream gives the list its verdict and walks the rows (the partition, the headers, clean or dirty by a
 * search in the list), scans, a decode table of max_slots rows filled by a second walk (dirty row j of a stream at its j-th row, decoded behind
 * the dirty rows before it) and ONE decode over it, a slot table of max_slots rows (the m-th rebuilt piece of a stream: found through a scan of
 * the pieces that start in each dirty row, its length from the list) with ONE compressor and ONE CRC launch, the verdicts, one thread per new row
 * (kept: the old chunk; rebuilt: its slot), a scan of the chunk sizes, and an emit whose workgroups each take the pieces that start in 64 KiB
 * of what a new stream decodes to: a copy from `in`, or header plus payload from staging.  No atomic decides an order or a value of an output:
 * the outputs are the same in every run.
 * SNP_ERR_BAD_ARG for flags with any other bit, for nstreams >= 2^31 and for a null pointer (nstreams == 0 needs only ctx and d_result: it
 * writes a zeroed d_result and nothing else; out_bound is optional, idx_start / idx_pos are needed when nentries > 0, cuts when ncuts > 0,
 * new_start / new_pos when max_entries > 0), SNP_ERR_DEVICE for a runtime failure. */
uint64_t snp_frame_recut_indexed_workspace(uint32_t nstreams, uint32_t max_slots, uint64_t stage_cap, uint32_t max_entries);
snp_status snp_frame_recut_indexed_batch(snp_ctx* ctx, const uint8_t* in, const uint64_t* in_off, const uint64_t* in_len, uint32_t nstreams,
                                         const uint64_t* idx_first, const uint64_t* idx_start, const uint64_t* idx_pos,
                                         const uint64_t* idx_total, const int32_t* idx_tail, uint64_t nentries,
                                         const uint64_t* cut_first, const uint64_t* cuts, uint64_t ncuts,
                                         uint32_t flags, uint32_t max_slots, uint64_t stage_cap, uint32_t max_entries,
                                         uint8_t* out, const uint64_t* out_off, const uint64_t* out_cap, uint64_t* out_len, int32_t* status,
                                         uint64_t* new_first, uint64_t* new_start, uint64_t* new_pos, uint64_t* new_total, int32_t* new_tail,
                                         uint64_t* out_bound, void* d_work, uint64_t* d_result);

#ifdef __cplusplus
}
#endif
#endif /* SNAPPIER_HIP_FRAME_RECUT_H */

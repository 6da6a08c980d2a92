/*
 * snappier_hip_frame_edit.h -- C-ABI of libsnappier_hip_frame_edit.so: device batch EDIT of seekable Snappy framed streams through their chunk
 * index -- a sorted EDIT SCRIPT per stream, every edit an insert, a delete or a replacement, all of them in the OLD stream's coordinates, applied
 * in one call.  snp_frame_splice_indexed_batch (snappier_hip_frame_splice.h) takes one such edit per stream and call, and every call copies the
 * whole stream; whatever produces edits produces a list per stream -- every occurrence of a needle (snp_frame_find_indexed_batch), the hunks of a
 * patch.  This call decodes each touched chunk once, compresses each rewritten region once, copies every other byte once and returns the new
 * index.
 *
 * An extension of include/snappier_hip.h in a library of its own, linked against libsnappier_hip.so and taking that library's contexts (snp_ctx).
 * It adds no status code and no option and keeps no state in the context; the surfaces of snappier_hip.h and the other extension headers are
 * unchanged.  The C# side binds these functions in csharp/Snappier.Gpu/NativeMethodsFrameEdit.cs.
 */
#ifndef SNAPPIER_HIP_FRAME_EDIT_H
#define SNAPPIER_HIP_FRAME_EDIT_H

#include "snappier_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The stream and index arguments, `out`, out_off, out_cap, out_len, the new index arrays (new_start and new_pos hold nentries + max_slots rows),
 * out_bound, d_result[0..3], the sizing call (max_slots = stage_cap = 0) and the rules for null pointers and nstreams == 0 are those of
 * snp_frame_splice_indexed_batch, field for field; read them there.  What differs is said here.
 *
 * The edits.  Stream b has the edits [ed_first[b], ed_first[b + 1]) of the nedits of the call (the CSR form seg_first has in
 * snp_frame_compose_indexed_batch, and hit_off coming out of snp_frame_find_indexed_batch).  Edit e replaces the decoded bytes
 * [ed_off[e], ed_off[e] + ed_del[e]) of the OLD stream by src[src_off[e] .. +ed_ins[e]): the caller re-bases nothing.  The edits of a stream
 * must be ascending and disjoint: ed_off[e] >= ed_off[e - 1] + ed_del[e - 1].  Equality is legal; two inserts at one offset apply in list
 * order.  An edit with del == ins == 0 is SKIPPED: nothing of it is looked at, not its offset either, and the order rule runs over the others.
 * A stream with no edit, or only skipped ones, is not named: SNP_OK, out_len[b] = 0, nothing of the index looked at, as in the splice.
 * ed_first is untrusted: its values are clamped to nedits, and a list that runs backwards (ed_first[b + 1] < ed_first[b]) gives its stream
 * SNP_ERR_BAD_ARG, as a seg_first that runs backwards does in the compose call -- AND EVERY STREAM AFTER IT TOO: an edit belongs to one stream
 * here (its stream is found from ed_first, where a compose segment names its own), and behind a list that runs backwards two lists could
 * claim the same edit.  Edits that no stream's list holds are not looked at; their ed_status is SNP_OK.
 *
 * The new stream.  Per edit, the owned rows [r0, r1), the head H, the tail T, the hole, the probes of the untrusted index and every check are
 * those of the splice for that edit alone, header for header (one function plans both: fs_plan, csrc/frame_splice_device.h).  Two consecutive
 * edits of a stream are LINKED when both own rows and the last owned row of the first is the first owned row of the second.  A GROUP is a
 * maximal run of linked edits; an edit that owns no row is a group of its own.  A group has ONE region
 *   R = H(first) || ins_1 || G_1 || ins_2 || ... || ins_k || T(last),
 * G_i the kept decoded bytes [hi_i, lo_(i+1)), which lie inside the shared row, and ONE hole [P0, P1) = [pos[r0(first)], the end of the chunk
 * of row r1(last) - 1).  R is cut into pieces of chunk_bytes, each one slot of snp_frame_encode_chunked_batch, as in the splice.  The new stream
 * is the old bytes outside all holes, copied verbatim, with each group's new chunks in its hole's place; an empty stream (in_len == 0) gets
 * the identifier first.  Holes of successive groups are ordered and do not overlap -- P1(g) <= P0(g + 1), and r1(g) <= r0(g + 1) for the rows:
 * with a sound index this follows from the order of the edits; both are checked, and an index that breaks one gives SNP_ERR_BAD_ARG.
 * A ROW THAT TWO OR MORE EDITS TOUCH IS DECODED AND VERIFIED ONCE.  A wholly deleted row is never decoded; non-data chunks inside a hole go with
 * it, those between holes stay.  With one edit per stream every output array is what snp_frame_splice_indexed_batch writes.
 *
 * The new index.  Rows before the first hole are copied.  Each group's new rows follow in place, start = lo(first) - |H| + k * chunk_bytes in
 * the new stream's coordinates: the old value plus the sum of ins - del over the edits before the group.  Old rows between and behind holes are
 * moved: start by the running ins - del, pos by the running (new bytes - hole bytes).  new_total = total - sum(del) + sum(ins).
 *
 * Verdicts.  A stream is edited whole or not at all.  ed_status[e] (nedits x i32) is the edit's own verdict: what the splice gives that edit
 * alone before anything is decoded (an idx_tail that is not SNP_OK, lo + del above total, the index probes, ...); else SNP_ERR_BAD_ARG when it
 * is out of order with, or overlaps, the named edit before it; when its hole or its rows are not behind those of that edit (and they are not
 * linked); and when total - sum(del) + sum(ins) over the stream's edits up to it wraps.  SNP_OK for a skipped edit.  status[b] is the first
 * ed_status of the stream that is not SNP_OK; else, as in the splice: SNP_ERR_OUTPUT_TOO_SMALL by admission, the status of the first edge row
 * (in edit order, an edit's head row before its tail row) that failed to decode or verify, SNP_ERR_OUTPUT_TOO_SMALL by out_cap.
 * Admission, in stream order over the named streams that passed: the pieces of all groups against max_slots and the staging bytes -- the
 * decoded bytes of each DISTINCT edge row once, plus the sum of |R| -- against stage_cap, each with those of the streams before.  A group is
 * counted as at most 2^32 pieces and 2^48 + 2^18 bytes, and so is a stream.  out_bound[b] = in_len - sum(P1 - P0) + sum(8 * pieces + |R|)
 * (+ 10 for an empty stream), from the headers alone.
 * d_work must hold snp_frame_edit_indexed_workspace(nstreams, nedits, max_slots, stage_cap, chunk_bytes) bytes (host arithmetic; 0 when
 * nstreams is 0 or chunk_bytes is out of range): about 140 bytes per stream, 362 per edit (its two rows of the decode table among them), 45
 * per slot, stage_cap of staging and snp_max_compressed_length(chunk_bytes) + 32 of compressed staging per slot.
 * Stream capture: the call only enqueues on the context's stream -- no allocation, no read-back, no synchronisation -- under the rule of
 * snp_frame_encode_buffers_batch: make the same call, with the same max_slots and nedits, once before the capture.
 * How: frame_edit.hip -- a plan per edit, the named edits compacted, link flags and segmented sums by prefix scans (inserted bytes as two
 * half-word sums, so that no sum wraps), a plan per group and per stream, ONE decode over an edge table of 2 x nedits rows, an assemble kernel
 * over 64 KiB units of staging that finds its parts by a search over the running lengths, ONE compressor and ONE CRC launch over all pieces,
 * an emit over 64 KiB units of kept bytes (a unit that meets holes is several copies) and over the new chunks, and a merge of the index rows.
 * SNP_ERR_BAD_ARG for chunk_bytes of 0 or above 65536, for nstreams or nedits >= 2^31 and for a null pointer (nstreams == 0 needs only ctx and
 * d_result; out_bound is optional; ed_off, ed_del, ed_ins, src_off and ed_status when nedits > 0; idx_start / idx_pos when nentries > 0;
 * new_start / new_pos when nentries + max_slots > 0), SNP_ERR_DEVICE for a runtime failure. */
uint64_t snp_frame_edit_indexed_workspace(uint32_t nstreams, uint32_t nedits, uint32_t max_slots, uint64_t stage_cap, uint32_t chunk_bytes);
snp_status snp_frame_edit_indexed_batch(snp_ctx* ctx, const uint8_t* in, const uint64_t* in_off, const uint64_t* in_len, uint32_t nstreams,
                                        const uint64_t* idx_first, const uint64_t* idx_start, const uint64_t* idx_pos, const uint64_t* idx_total,
                                        const int32_t* idx_tail, uint64_t nentries, const uint8_t* src, const uint64_t* ed_first,
                                        const uint64_t* ed_off, const uint64_t* ed_del, const uint64_t* ed_ins, const uint64_t* src_off,
                                        uint32_t nedits, uint32_t chunk_bytes, uint32_t max_slots, uint64_t stage_cap, uint8_t* out,
                                        const uint64_t* out_off, const uint64_t* out_cap, uint64_t* out_len, int32_t* status, int32_t* ed_status,
                                        uint64_t* new_first, uint64_t* new_start, uint64_t* new_pos, uint64_t* new_total, int32_t* new_tail,
                                        uint64_t* out_bound, void* d_work, uint64_t* d_result);

#ifdef __cplusplus
}
#endif
#endif /* SNAPPIER_HIP_FRAME_EDIT_H */

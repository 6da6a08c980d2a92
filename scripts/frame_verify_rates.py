"""Verify and repair rates (libsnappier_hip_frame_verify.so): html-like data (snappier_amd/datagen.py) as 160 streams of 64 MiB and as 163 840
streams of 64 KiB, each encoded seekable at 4 096- and at 65 536-byte chunks.  Everything here is reported, nothing is gated.

Per store: snp_frame_verify_indexed_batch (slot_bytes = the chunk size, workspace allocated before the timing) at scratch_cap = 64 MiB, 256 MiB,
1 GiB and the full decoded size -- whether a scratch that fits the 256 MiB Infinity Cache beats a full-size one is what the sweep is there to
decide --, and in the same process, interleaved, what the library offered for the same question before: frame_read_indexed of every stream
whole into a full-size buffer, and a rechunk with RECHUNK_REWRITE_ALL (the scrub).  Then the repair of one damaged 4 KiB range per stream --
one chunk at 4 096, the chunk that holds it at 65 536 -- with frame_repair_streams from an undamaged copy, against a full re-encode of the
replica's decoded bytes (frame_encode_seekable).  ms from HIP events around each call (median of --reps after one warm-up); the repair, which
reads back and allocates, is wall-clock between two synchronisations.  One JSON line per measurement, appended to --out as it is made.  --gib
scales both shapes down (10: the shapes above).

    python scripts/frame_verify_rates.py --out profiles/r26a_frame_verify_rates.jsonl
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
from snappier_amd import batch as SB, datagen as SD, _native as N  # noqa: E402
from compress_buffers_rates import B  # noqa: E402
from frame_chunked_rates import i64, rec_ms, u8  # noqa: E402
from frame_splice_rates import timed  # noqa: E402

MIB = 1 << 20


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="64m,64k")
    ap.add_argument("--chunks", default="4096,65536")
    ap.add_argument("--gib", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--repair", type=int, default=1, help="time the repair of one damaged chunk per stream (0: skip)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    total = a.gib << 30
    html = open(os.path.join(ROOT, "tests", "golden", "testdata", "html"), "rb").read()
    raw = SD.html_like_blocks(html, 0, total // B, "cuda")
    cd = SB.BlockCodec(0, N.HASH_CRC32C)
    cd.ctx.reserve_compress(total // B)
    VL = N.frame_verify_lib()

    def emit(rec):
        rec["where"] = torch.cuda.get_device_name(0)
        print(json.dumps(rec), flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(json.dumps(rec) + "\n")

    for shape in a.shapes.split(","):
        n = 64 * MIB if shape == "64m" else B
        ns = total // n
        lens = np.full(ns, n)
        in_off, in_len = i64(np.cumsum(lens) - lens), i64(lens)
        for cb in [int(v) for v in a.chunks.split(",")]:
            out, out_off, out_len, est, _, index = cd.frame_encode_seekable(raw, in_off, in_len, chunk_bytes=cb)
            torch.cuda.synchronize()
            assert int((est != 0).sum()) == 0
            ne, framed_bytes = index.nentries, int(out_len.sum())
            common = {"shape": shape, "streams": ns, "stream_raw_bytes": int(n), "chunk_bytes": cb, "index_rows": int(index.first[ns]),
                      "framed_bytes": framed_bytes, "decoded_bytes": total}
            caps = [("64 MiB", 64 * MIB), ("256 MiB", 256 * MIB), ("1 GiB", 1024 * MIB), ("full", total)]
            works = [u8(VL.snp_frame_verify_indexed_workspace(ns, ne, cb, cap)) for _, cap in caps]
            got = {}

            def verify_at(k):
                def run():
                    got[k] = cd.frame_verify_indexed(out, out_off, out_len, index, cb, caps[k][1], works[k])
                return run

            # what the library offered before: the indexed read of every stream whole, and the scrub
            whole = u8(total)
            req = torch.arange(ns, dtype=torch.int32, device="cuda")
            zero = torch.zeros(ns, dtype=torch.int64, device="cuda")
            need = cd.frame_read_indexed(out, out_off, out_len, index, req, zero, in_len, whole, in_off, in_len, 0, 0)[2].tolist()      # the sizing call
            rwork = u8(N.frame_index_lib().snp_frame_read_indexed_workspace(ns, need[0], need[2]))

            def read():
                got["read"] = cd.frame_read_indexed(out, out_off, out_len, index, req, zero, in_len, whole, in_off, in_len, need[0], need[2], rwork)

            res = timed([verify_at(k) for k in range(len(caps))] + [read], a.reps)
            read_ms = res[len(caps)][0]
            assert int((got["read"][1] != 0).sum()) == 0
            del whole, rwork
            torch.cuda.empty_cache()
            t0 = time.perf_counter()
            scrub = cd.frame_rechunk_to_memory(out, out_off, out_len, index, cb, rewrite_all=True)
            torch.cuda.synchronize()
            scrub_first = (time.perf_counter() - t0) * 1e3
            ms = []
            for _ in range(a.reps):
                t0 = time.perf_counter()
                scrub = cd.frame_rechunk_to_memory(out, out_off, out_len, index, cb, rewrite_all=True)
                torch.cuda.synchronize()
                ms.append((time.perf_counter() - t0) * 1e3)
            scrub_ms = float(np.median(ms))
            assert int((scrub[3] != 0).sum()) == 0
            del scrub
            torch.cuda.empty_cache()
            for k, (name, cap) in enumerate(caps):
                r = got[k][6].tolist()
                emit({"what": "snp_frame_verify_indexed_batch", **common, "scratch_cap": name, "scratch_bytes": min(cap, total), **rec_ms(*res[k]),
                      "decoded_gb_per_s": round(total / res[k][0] / 1e6, 1), "result": r, "all_ok": int((got[k][1] != 0).sum()) == 0,
                      "workspace_bytes": works[k].numel(), "verify_over_read": round(res[k][0] / read_ms, 3),
                      "verify_over_scrub": round(res[k][0] / scrub_ms, 3)})
            emit({"what": "frame_read_indexed of every stream whole into a full-size buffer", **common, **rec_ms(*res[len(caps)]),
                  "decoded_gb_per_s": round(total / read_ms / 1e6, 1)})
            emit({"what": "frame_rechunk_to_memory with RECHUNK_REWRITE_ALL (the scrub; wall clock, sizing call and allocation included)", **common,
                  **rec_ms(scrub_ms, ms), "first_ms": round(scrub_first, 3)})
            del works, got
            torch.cuda.empty_cache()
            if a.repair:
                # one 4 KiB range per stream rots (a body byte of the chunk at one third of the stream); the replica is an undamaged copy
                replica = out.clone()
                first = index.first[:ns]
                rows = first + (index.first[1:ns + 1] - first) // 3
                at = out_off + index.pos[rows] + 40
                out[at] ^= 4
                t0 = time.perf_counter()
                damaged, fixed, f_off, f_len, fst, _ = cd.frame_repair_streams(out, out_off, out_len, index, replica, out_off, out_len, index, cb)
                torch.cuda.synchronize()
                repair_ms = (time.perf_counter() - t0) * 1e3
                same = len(damaged) == ns and int((fst != 0).sum()) == 0 and torch.equal(f_len, out_len)
                for j in np.linspace(0, ns - 1, 16).astype(int).tolist() if same else []:
                    o, p, k = int(f_off[j]), int(out_off[j]), int(f_len[j])
                    same = same and torch.equal(fixed[o:o + k], replica[p:p + k])
                del fixed
                torch.cuda.empty_cache()
                t0 = time.perf_counter()
                again = cd.frame_encode_seekable(raw, in_off, in_len, chunk_bytes=cb)
                torch.cuda.synchronize()
                encode_ms = (time.perf_counter() - t0) * 1e3
                emit({"what": "frame_repair_streams: one damaged chunk per stream, from an undamaged copy (wall clock, both verifies included)",
                      **common, "ms": round(repair_ms, 3), "damaged_streams": len(damaged), "repaired_byte_for_byte": bool(same),
                      "full_reencode_ms": round(encode_ms, 3), "repair_over_reencode": round(repair_ms / encode_ms, 3)})
                del again, replica
            del out
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()

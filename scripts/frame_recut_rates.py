"""Recut rates (libsnappier_hip_frame_recut.so): html-like data (snappier_amd/datagen.py), content-defined at (window, max_bytes) = (2048, 16384),
as 160 streams of 64 MiB and as 163 840 streams of 64 KiB.  Everything here is reported, nothing is gated.

Four stores per shape, each brought to the chunks frame_encode_content_defined writes for what it decodes to:
  * splice:    content-defined streams after one 4 KiB frame_splice insert at 1/3 of each;
  * append:    the same streams after a 64 KiB frame_append to each (written on the 16 384 grid);
  * grid:      a store written at 4 096-byte chunks (every piece is rebuilt);
  * canonical: content-defined streams as they were written (every stream is left alone).
Per store two sides, interleaved:
  * recut: frame_recut_content_defined -- the indexed read of every stream whole, content_cuts, the sizing call and the recut;
  * today: frame_decode_to_memory then frame_encode_content_defined, what a caller does with the calls there were before.
and the recut call alone with the cut list given and every bound sized beforehand (snp_frame_recut_indexed_batch: what is left when the
caller has the cuts), with d_result[6] chunks copied and d_result[7] pieces rebuilt.  After each store the two sides' outputs are compared:
every status, every length, every index row, the CRC-32C of every stream's framed bytes (snp_crc32c_batch over both sides, on the device), and
--sample streams byte for byte (all of them when there are no more).  ms from HIP events around each side
(median of --reps after one warm-up; both wrappers read sizes back, so host time between their launches is inside).  One JSON line per
measurement, appended to --out as it is made.  --gib scales the shapes down (10: the shapes above).  --recut-only makes the call alone and
nothing else, for a rocprofv3 --kernel-trace --stats run of its own (the plan and fill kernels take one workgroup per stream).

    python scripts/frame_recut_rates.py --out profiles/r25a_frame_recut_rates.jsonl
"""
import argparse
import json
import os
import sys

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
W, MX, INS, APP = 2048, 16384, 4096, 65536


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="64m,64k")
    ap.add_argument("--stores", default="splice,append,grid,canonical")
    ap.add_argument("--gib", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sample", type=int, default=64)
    ap.add_argument("--recut-only", action="store_true", help="the recut call alone, no other side and no check (a rocprofv3 --kernel-trace --stats run of its own)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    total = a.gib << 30
    html = open(os.path.join(ROOT, "tests", "golden", "testdata", "html"), "rb").read()
    raw = SD.html_like_blocks(html, 0, total // B, "cuda")
    cd = SB.BlockCodec(0, N.HASH_CRC32C)
    cd.ctx.reserve_compress(2 * total // B)
    RL = N.frame_recut_lib()
    gen = torch.Generator("cuda").manual_seed(7)

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
        for store in a.stores.split(","):
            # the store: framed bytes, their table and their index
            if store == "grid":
                framed, f_off, f_len, st, _, index = cd.frame_encode_seekable(raw, in_off, in_len, 4096)
            else:
                n_cut = in_len // (W + 1) + in_len // MX
                cap = 10 + 8 * (n_cut + 1) + in_len + (APP + 8 * (APP // MX + 2) + 64 if store == "append" else 0)
                framed, f_off, f_len, st, _, index = cd.frame_encode_content_defined(raw, in_off, in_len, W, MX, out_cap=cap)
            assert int((st != 0).sum()) == 0
            if store == "splice":
                ins = torch.randint(0, 256, (ns * INS,), dtype=torch.uint8, device="cuda", generator=gen)
                k = torch.arange(ns, dtype=torch.int64, device="cuda")
                s_out, s_off, s_len, s_st, s_ix = cd.frame_splice_to_memory(framed, f_off, f_len, index, torch.full_like(k, n // 3), torch.zeros_like(k),
                                                                            ins, k * INS, torch.full_like(k, INS), MX)
                assert int((s_st != 0).sum()) == 0
                framed, f_off, f_len, index = s_out, s_off, s_len, s_ix
                del ins
            elif store == "append":
                more = torch.randint(0, 256, (ns * APP,), dtype=torch.uint8, device="cuda", generator=gen)
                k = torch.arange(ns, dtype=torch.int64, device="cuda")
                new_len, a_st, a_ix = cd.frame_append_to_memory(framed, f_off, f_len, cap, index, more, k * APP, torch.full_like(k, APP), MX)
                assert int((a_st != 0).sum()) == 0
                f_len, index = new_len, a_ix
                del more
            torch.cuda.synchronize()
            torch.cuda.empty_cache()
            framed_bytes, rows = int(f_len.sum()), int(index.first[ns])
            got = {}

            def recut():
                got["r"] = cd.frame_recut_content_defined(framed, f_off, f_len, index, W, MX)

            def today():
                dec, d_off, d_len, d_st = cd.frame_decode_to_memory(framed, f_off, f_len)
                got["t"] = cd.frame_encode_content_defined(dec, d_off, d_len, W, MX)

            common = {"shape": shape, "store": store, "streams": ns, "stream_raw_bytes": int(n), "window": W, "max_bytes": MX, "index_rows": rows,
                      "framed_bytes": framed_bytes}
            if not a.recut_only:
                res = timed([recut, today], a.reps)
                out, o_off, o_len, status, new_ix = got["r"]
                want, w_off, w_len, w_st, _, w_ix = got["t"]
                r = new_ix.result.tolist()
                # the outputs: a stream that was left alone is its old bytes
                ok = int((status != 0).sum()) == 0 and int((w_st != 0).sum()) == 0
                new_len = torch.where(o_len > 0, o_len, f_len)
                same = ok and torch.equal(new_len, w_len) and torch.equal(new_ix.first, w_ix.first)
                used = int(w_ix.first[ns])
                same = same and torch.equal(new_ix.start[:used], w_ix.start[:used]) and torch.equal(new_ix.pos[:used], w_ix.pos[:used])
                # every stream's framed bytes on the device, by the CRC-32C of each (snp_crc32c_batch), then a sample of them byte for byte
                if same:
                    mine = torch.where(o_len > 0, cd.crc32c(out, o_off, o_len), cd.crc32c(framed, f_off, torch.where(o_len > 0, torch.zeros_like(f_len), f_len)))
                    same = torch.equal(mine, cd.crc32c(want, w_off, w_len))
                picks = np.unique(np.linspace(0, ns - 1, min(ns, a.sample)).astype(int)).tolist()
                for b in picks if same else []:
                    src, o = (out, int(o_off[b])) if int(o_len[b]) else (framed, int(f_off[b]))
                    p, ln = int(w_off[b]), int(w_len[b])
                    same = same and torch.equal(src[o:o + ln], want[p:p + ln])
                emit({"what": "frame_recut_content_defined (read, content_cuts, sizing, recut)", **common, **rec_ms(*res[0]), "result": r,
                      "chunks_copied": r[6], "pieces_rebuilt": r[7], "streams_written": r[3], "streams_left_alone": r[5],
                      "recut_over_today": round(res[0][0] / res[1][0], 3)})
                emit({"what": "frame_decode_to_memory + frame_encode_content_defined (today)", **common, **rec_ms(*res[1])})
                emit({"what": "outputs equal: every status, length and index row, the CRC-32C of every stream's framed bytes, %d streams byte for byte" % len(picks), **common, "same": bool(same)})
                del got, want, out
                torch.cuda.empty_cache()
            # the call alone: the cuts given (the finder's for the decoded bytes), every bound from one sizing call
            dec, d_off, d_len, d_st = cd.frame_decode_to_memory(framed, f_off, f_len)
            cut_first, cuts, _, _ = cd.content_cuts(dec, d_off, d_len, W, MX)
            del dec
            zero = torch.zeros(ns, dtype=torch.int64, device="cuda")
            _, _, _, sized, bound = cd.frame_recut_indexed(framed, f_off, f_len, index, cut_first, cuts, u8(0), zero, zero, 0, 0, 0, with_bound=True)
            need = sized.tolist()
            ends = torch.cumsum(bound, 0)
            arena = u8(int(ends[-1]))
            work = u8(RL.snp_frame_recut_indexed_workspace(ns, need[0], need[2], need[4]))

            def alone():
                got2["r"] = cd.frame_recut_indexed(framed, f_off, f_len, index, cut_first, cuts, arena, ends - bound, bound, need[0], need[2], need[4],
                                                   work=work)

            def copy():
                spare.copy_(framed[:spare.numel()])

            got2 = {}
            spare = u8(min(framed_bytes, framed.numel()))
            one = timed([alone, copy], a.reps)
            r2 = got2["r"][3].tolist()
            emit({"what": "snp_frame_recut_indexed_batch alone (cuts given, bounds sized before)", **common, **rec_ms(*one[0]), "result": r2,
                  "chunks_copied": r2[6], "pieces_rebuilt": r2[7], "max_slots": need[0], "stage_cap": need[2], "workspace_bytes": work.numel(),
                  "all_ok": int((got2["r"][1] != 0).sum()) == 0, "call_over_copy": round(one[0][0] / one[1][0], 2)})
            emit({"what": "device copy of the store's framed bytes (the floor)", **common, **rec_ms(*one[1])})
            del framed, arena, work, spare, got2, index
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()

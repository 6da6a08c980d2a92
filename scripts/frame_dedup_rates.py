"""Dedup rates (libsnappier_hip_frame_dedup.so): html-like data (snappier_amd/datagen.py), content-defined at (window, max_bytes) =
(2048, 16384), on two batches.  Everything here is reported, nothing is gated.

  * versions: 160 streams of 64 MiB (the base) and their copies after one 4 KiB insert at 1/3 of each, encoded from scratch (the new streams);
  * repeats: 163 840 streams of 64 KiB of which the second half repeats the first, no base.

Per batch four figures: snp_frame_dedup_indexed_batch (bounds and workspace sized by one sizing call before the timing); a device copy of the
batch's framed bytes, the floor of anything that reads them once; one frame_digest_streams call over the same streams, the other call that
works from the chunk headers; and the pack's bytes over the new streams' bytes.  The recipes are composed back once and compared with the new
streams byte for byte.  ms from HIP events around each call, interleaved (median of --reps after one warm-up).  One JSON line per measurement,
appended to --out as it is made.  --gib scales both batches down (10: the shapes above).

    python scripts/frame_dedup_rates.py --out profiles/r24a_frame_dedup_rates.jsonl
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
W, MX, INS = 2048, 16384, 4096


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="versions,repeats")
    ap.add_argument("--gib", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--check", type=int, default=1, help="compose the recipes back and compare (0: skip)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    total = a.gib << 30
    html = open(os.path.join(ROOT, "tests", "golden", "testdata", "html"), "rb").read()
    raw = SD.html_like_blocks(html, 0, total // B, "cuda")
    cd = SB.BlockCodec(0, N.HASH_CRC32C)
    cd.ctx.reserve_compress(2 * total // B)
    DL = N.frame_dedup_lib()

    def emit(rec):
        rec["where"] = torch.cuda.get_device_name(0)
        print(json.dumps(rec), flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(json.dumps(rec) + "\n")

    for batch in a.batches.split(","):
        if batch == "versions":
            n, nb = 64 * MIB, total // (64 * MIB)
            x = raw.view(nb, n)
            at = n // 3
            ins = torch.randint(0, 256, (nb, INS), dtype=torch.uint8, device="cuda", generator=torch.Generator("cuda").manual_seed(7))
            data = torch.cat([raw, torch.cat([x[:, :at], ins, x[:, at:]], dim=1).contiguous().view(-1)])
            lens = np.concatenate([np.full(nb, n), np.full(nb, n + INS)])
            nbase = nb
        else:
            n, nb = B, total // B
            half = raw[:(nb // 2) * n]
            data = torch.cat([half, half])
            lens = np.full(nb // 2 * 2, n)
            nbase = 0
        ns = len(lens)
        in_off, in_len = i64(np.cumsum(lens) - lens), i64(lens)
        out, out_off, out_len, est, _, index = cd.frame_encode_content_defined(data, in_off, in_len, W, MX)
        torch.cuda.synchronize()
        assert int((est != 0).sum()) == 0
        del data
        torch.cuda.empty_cache()
        framed_bytes, new_bytes = int(out_len.sum()), int(out_len[nbase:].sum())
        need = cd.frame_dedup_indexed(out, out_off, out_len, index, nbase, 0, 0, None)[5].tolist()     # the sizing call
        pack = u8(need[1])
        work = u8(DL.snp_frame_dedup_indexed_workspace(ns, index.nentries))
        spare = u8(framed_bytes)
        got = {}

        def dedup():
            got["r"] = cd.frame_dedup_indexed(out, out_off, out_len, index, nbase, need[0], need[2], pack, work)

        def copy():
            spare.copy_(out[:framed_bytes])

        def digest():
            got["d"] = cd.frame_digest_streams(out, out_off, out_len, index)

        res = timed([dedup, copy, digest], a.reps)
        _, status, canon, pindex, recipe, result = got["r"]
        r = result.tolist()
        common = {"batch": batch, "streams": ns, "base_streams": nbase, "stream_raw_bytes": int(n), "window": W, "max_bytes": MX,
                  "index_rows": int(index.first[ns]), "framed_bytes": framed_bytes}
        emit({"what": "snp_frame_dedup_indexed_batch", **common, **rec_ms(*res[0]), "framed_gb_per_s": round(framed_bytes / res[0][0] / 1e6, 1),
              "result": r, "all_ok": int((status != 0).sum()) == 0, "workspace_bytes": work.numel(),
              "call_over_copy": round(res[0][0] / res[1][0], 2), "call_over_digest": round(res[0][0] / res[2][0], 2)})
        emit({"what": "device copy of the batch's framed bytes (the floor)", **common, **rec_ms(*res[1]),
              "gb_per_s": round(framed_bytes / res[1][0] / 1e6, 1)})
        emit({"what": "frame_digest_streams over the same streams", **common, **rec_ms(*res[2]),
              "all_ok": int((got["d"][2] != 0).sum()) == 0})
        emit({"what": "pack bytes over the new streams' bytes", **common, "pack_bytes": r[1], "new_stream_bytes": new_bytes,
              "ratio": round(r[1] / new_bytes, 4), "unique_rows": r[0], "merged_rows": r[5], "rows_with_a_leader_s_key_but_other_bytes": r[6],
              "segments": r[2]})
        if a.check:
            del spare, work
            torch.cuda.empty_cache()
            back, b_off, b_len, bst, _ = cd.frame_restore_to_memory(out, out_off, out_len, index, nbase, pack[:r[1]], pindex, recipe)
            torch.cuda.synchronize()
            same = int((bst != 0).sum()) == 0 and torch.equal(b_len, out_len[nbase:])
            for j in np.linspace(0, ns - nbase - 1, 16).astype(int).tolist() if same else []:
                o, p, k = int(b_off[j]), int(out_off[nbase + j]), int(b_len[j])
                same = same and torch.equal(back[o:o + k], out[p:p + k])
            emit({"what": "recipes composed back: statuses, every length, 16 streams byte for byte", **common, "same": bool(same)})
            del back
        del out, pack, got
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()

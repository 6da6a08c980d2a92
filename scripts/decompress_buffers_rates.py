"""snp_decompress_buffers_batch rates: 10 GiB of html-like data (snappier_amd/datagen.py) in the four shapes of compress_buffers_rates.py, made into
one Snappy block per buffer by snp_compress_buffers_batch, then decoded by snp_decompress_batch (one wavefront per block) and by
snp_decompress_buffers_batch (large blocks split across wavefronts) on the same blocks.  Output GB/s from HIP events around each call (median of
--reps after one warm-up); every round trip is checked against the input.  max_fragments is exact: d_result[0] of a first call with 0.
One JSON line per measurement to --out.

    python scripts/decompress_buffers_rates.py --out profiles/r07b_decompress_buffers_rates.jsonl
    rocprofv3 --kernel-trace --stats -d DIR -o run -- python scripts/decompress_buffers_rates.py --shapes 64m --reps 2 --no-batch
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
from compress_buffers_rates import B, TOTAL, shapes, timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="64k,1m,64m,loguni")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-batch", action="store_true", help="skip the snp_decompress_batch comparison (profiling runs)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    html = open(os.path.join(ROOT, "tests", "golden", "testdata", "html"), "rb").read()
    raw = SD.html_like_blocks(html, 0, TOTAL // B, "cuda")
    cd = SB.BlockCodec(0, N.HASH_CRC32C)
    lines = []

    def emit(rec):
        rec["where"] = torch.cuda.get_device_name(0)
        print(json.dumps(rec), flush=True)
        lines.append(rec)

    back = torch.empty(TOTAL, dtype=torch.uint8, device="cuda")
    for name, lens in shapes(a.shapes.split(",")).items():
        nb = len(lens)
        in_off = torch.from_numpy(np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)).cuda()
        in_len = torch.from_numpy(lens.astype(np.uint32).view(np.int32)).cuda()
        # the blocks, made on the device
        comp, comp_off, comp_len, status, _ = cd.compress_buffers(raw, in_off, in_len)
        torch.cuda.synchronize()
        assert int((status != 0).sum()) == 0, name
        torch.cuda.empty_cache()                                  # (the compressor's staging goes)
        c_len = comp_len.to(torch.int32)
        ratio = float(comp_len.sum()) / float(lens.sum())
        out_off, out_cap = in_off, in_len                         # each block back where its buffer came from, capacity = its length
        res = {}

        def check(tag, out_len, st):
            ok = int((st != 0).sum()) == 0 and torch.equal(out_len.to(torch.int64) & 0xFFFFFFFF, torch.from_numpy(lens).cuda())
            return ok and torch.equal(back, raw[:back.numel()])

        med_b = None
        if not a.no_batch:
            def bcall():
                res["b"] = cd.decompress(comp, comp_off, c_len, back, out_off, out_cap)

            back.zero_()
            med_b, ms_b = timed(bcall, a.reps)
            emit({"what": "snp_decompress_batch", "shape": name, "blocks": nb, "output_bytes": int(lens.sum()), "ratio": round(ratio, 4),
                  "ms": round(med_b, 3), "ms_all": [round(x, 3) for x in ms_b], "output_GBps": round(lens.sum() / med_b / 1e6, 2),
                  "round_trip_ok": check("batch", *res["b"])})
        # exact max_fragments: d_result[0] of a call that splits nothing
        probe = cd.decompress_buffers(comp, comp_off, c_len, back, out_off, out_cap, max_fragments=0)[2]
        mf = int(probe[0].item())
        work = torch.empty(max(N.buffers_decompress_lib().snp_decompress_buffers_workspace(nb, mf), 1), dtype=torch.uint8, device="cuda")

        def call():
            res["d"] = cd.decompress_buffers(comp, comp_off, c_len, back, out_off, out_cap, max_fragments=mf, work=work)

        back.zero_()
        t0 = time.time()
        med, ms = timed(call, a.reps)
        out_len, st, result = res["d"]
        rec = {"what": "snp_decompress_buffers_batch", "shape": name, "blocks": nb, "output_bytes": int(lens.sum()), "max_fragments": mf,
               "workspace_bytes": work.numel(), "ms": round(med, 3), "ms_all": [round(x, 3) for x in ms], "output_GBps": round(lens.sum() / med / 1e6, 2),
               "result": result.cpu().tolist(), "round_trip_ok": check("buffers", out_len, st), "wall_s": round(time.time() - t0, 1)}
        if med_b is not None:
            rec["speedup_over_decompress_batch"] = round(med_b / med, 4)
        emit(rec)
        del comp, comp_off, comp_len, c_len, work, res
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "a") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()

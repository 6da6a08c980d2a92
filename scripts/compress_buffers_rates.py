"""snp_compress_buffers_batch rates: 10 GiB of html-like data (snappier_amd/datagen.py) in four shapes, each compressed as buffers of any length
(one Snappy block per buffer) and, beside it, the same bytes cut into 64 KiB pieces through snp_compress_batch.  Input GB/s from HIP events around
each call (median of --reps after one warm-up).  Also records snp_decompress_batch on the 64 MiB shape's blocks (one wavefront per block: the
known slow case) and checks that round trip.  One JSON line per measurement to --out.

    python scripts/compress_buffers_rates.py --out profiles/r07a_compress_buffers_rates.jsonl
    rocprofv3 --kernel-trace --stats -d DIR -o run -- python scripts/compress_buffers_rates.py --shapes 64k --reps 2 --no-batch
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
from snappier_amd import batch as SB, datagen as SD, _native as N  # noqa: E402

B = 65536
TOTAL = 10 << 30


def shapes(which):
    rng = np.random.default_rng(20261016)
    out = {}
    if "64k" in which:
        out["64k"] = np.full(TOTAL // B, B, dtype=np.int64)
    if "1m" in which:
        out["1m"] = np.full(TOTAL >> 20, 1 << 20, dtype=np.int64)
    if "64m" in which:
        out["64m"] = np.full(TOTAL >> 26, 64 << 20, dtype=np.int64)
    if "loguni" in which:                                        # lengths log-uniform in [1 B, 16 MiB], fixed seed, cut to 10 GiB in total
        lens = np.floor(np.exp(rng.uniform(0, np.log(16 << 20), 40000))).astype(np.int64)
        csum = np.cumsum(lens)
        k = int(np.searchsorted(csum, TOTAL))
        lens = lens[:k + 1].copy()
        lens[-1] -= int(csum[k] - TOTAL)
        out["loguni"] = lens[lens > 0]
    return out


def timed(fn, reps):
    fn()                                                         # warm-up: workspaces, hints
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms)), ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="64k,1m,64m,loguni")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-batch", action="store_true", help="skip the snp_compress_batch comparison and the decode (profiling runs)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    html = open(os.path.join(ROOT, "tests", "golden", "testdata", "html"), "rb").read()
    raw = SD.html_like_blocks(html, 0, TOTAL // B, "cuda")
    cd = SB.BlockCodec(0, N.HASH_CRC32C)
    cd.ctx.reserve_compress(TOTAL // B)                          # the table workspace before the buffers crowd the device (as bench.py)
    lines = []

    def emit(rec):
        rec["where"] = torch.cuda.get_device_name(0)
        print(json.dumps(rec), flush=True)
        lines.append(rec)

    out = work = None
    for name, lens in shapes(a.shapes.split(",")).items():
        nb = len(lens)
        in_off = torch.from_numpy(np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)).cuda()
        in_len = torch.from_numpy(lens.astype(np.uint32).view(np.int32)).cuda()
        cap = 32 + lens + lens // 6 + 1 + 5
        out_cap = torch.from_numpy(cap).cuda()
        out_off = torch.from_numpy(np.concatenate([[0], np.cumsum(cap)[:-1]]).astype(np.int64)).cuda()
        mf = int(((lens + B - 1) // B).sum())
        if out is None or out.numel() < int(cap.sum()):
            out = None
            torch.cuda.empty_cache()
            out = torch.empty(int(cap.sum()), dtype=torch.uint8, device="cuda")
        need = N.buffers_lib().snp_compress_buffers_workspace(nb, mf)
        if work is None or work.numel() < need:
            work = None
            torch.cuda.empty_cache()
            work = torch.empty(need, dtype=torch.uint8, device="cuda")
        res = {}

        def call():
            res["r"] = cd.compress_buffers(raw, in_off, in_len, out=out, out_off=out_off, out_cap=out_cap, max_fragments=mf, work=work)

        t0 = time.time()
        med, ms = timed(call, a.reps)
        _, _, out_len, status, result = res["r"]
        ok = int((status != 0).sum()) == 0
        r = result.cpu().tolist()
        emit({"what": "snp_compress_buffers_batch", "shape": name, "buffers": nb, "fragments": mf, "input_bytes": int(lens.sum()), "ms": round(med, 3),
              "ms_all": [round(x, 3) for x in ms], "input_GBps": round(lens.sum() / med / 1e6, 2), "all_ok": ok, "result": r,
              "ratio": round(r[1] / lens.sum(), 4), "wall_s": round(time.time() - t0, 1)})
        if a.no_batch:
            continue
        # the same bytes as 64 KiB pieces through snp_compress_batch (blocks with their own varint preambles, at a fixed stride)
        p_lens = []
        for n in lens:
            p_lens += [B] * (int(n) // B) + ([int(n) % B] if n % B else [])
        p_lens = np.array(p_lens, dtype=np.int64)
        p_off = torch.from_numpy(np.concatenate([[0], np.cumsum(p_lens)[:-1]]).astype(np.int64)).cuda()
        p_len = torch.from_numpy(p_lens.astype(np.int32)).cuda()
        comp = torch.empty(len(p_lens) * cd.comp_stride, dtype=torch.uint8, device="cuda")
        comp_off = torch.arange(len(p_lens), dtype=torch.int64, device="cuda") * cd.comp_stride
        bres = {}

        def bcall():
            bres["r"] = cd.compress(raw, p_off, p_len, out=comp, out_off=comp_off)

        med_b, ms_b = timed(bcall, a.reps)
        emit({"what": "snp_compress_batch (64 KiB pieces)", "shape": name, "pieces": len(p_lens), "input_bytes": int(p_lens.sum()), "ms": round(med_b, 3),
              "ms_all": [round(x, 3) for x in ms_b], "input_GBps": round(p_lens.sum() / med_b / 1e6, 2),
              "all_ok": int((bres["r"][3] != 0).sum()) == 0, "buffers_over_batch_time": round(med / med_b, 4)})
        del comp, comp_off, bres
        if name == "64m":
            back = torch.empty(int(lens.sum()), dtype=torch.uint8, device="cuda")
            dcap = in_len.clone()
            dres = {}

            def dcall():
                dres["r"] = cd.decompress(out, out_off, out_len.to(torch.int32), back, in_off, dcap)

            med_d, ms_d = timed(dcall, max(1, a.reps // 2))
            dlen, dst = dres["r"]
            same = int((dst != 0).sum()) == 0 and torch.equal(back, raw[:back.numel()])
            emit({"what": "snp_decompress_batch (one 64 MiB block per wavefront)", "shape": name, "blocks": nb, "output_bytes": int(lens.sum()),
                  "ms": round(med_d, 3), "ms_all": [round(x, 3) for x in ms_d], "output_GBps": round(lens.sum() / med_d / 1e6, 2), "round_trip_ok": same})
            del back
    if a.out:
        with open(a.out, "a") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()

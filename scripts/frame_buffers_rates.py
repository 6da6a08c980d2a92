"""snp_frame_encode_buffers_batch / snp_frame_decode_buffers_batch rates: 10 GiB of html-like data (snappier_amd/datagen.py) in the four shapes of
compress_buffers_rates.py, each buffer one framed stream, against snp_frame_encode_device / snp_frame_decode_device on the same bytes framed as ONE
stream.  Raw GB/s from HIP events around each call (median of --reps after one warm-up); every round trip is checked against the input.  Both
bounds are exact (max_chunks = sum of ceil(n / 65536), max_spans = sum of ceil(framed / 2^20)).  On the 1 MiB shape a loop of the single-stream
calls over every stream is timed once beside the batch (--no-loop skips it).  One JSON line per measurement to --out.

    python scripts/frame_buffers_rates.py --out profiles/r07c_frame_buffers_rates.jsonl
    rocprofv3 --kernel-trace --stats -d DIR -o run -- python scripts/frame_buffers_rates.py --shapes 64k --reps 2 --no-single --no-loop
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

SPAN = 1 << 20


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="64k,1m,64m,loguni")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-single", action="store_true", help="skip the one-stream baselines (profiling runs)")
    ap.add_argument("--no-loop", action="store_true", help="skip the per-stream loop on the 1 MiB shape")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    html = open(os.path.join(ROOT, "tests", "golden", "testdata", "html"), "rb").read()
    raw = SD.html_like_blocks(html, 0, TOTAL // B, "cuda")
    cd = SB.BlockCodec(0, N.HASH_CRC32C)
    cd.ctx.reserve_compress(TOTAL // B)                          # the table workspace before the buffers crowd the device (as bench.py)
    L, FL = N.lib(), N.frame_buffers_lib()
    lines = []

    def emit(rec):
        rec["where"] = torch.cuda.get_device_name(0)
        print(json.dumps(rec), flush=True)
        lines.append(rec)

    base = {}
    if not a.no_single:
        # the same 10 GiB as ONE framed stream: snp_frame_encode_device, then snp_frame_decode_device (span walk)
        cap = L.snp_frame_max_encoded_length(TOTAL)
        one = torch.empty(cap, dtype=torch.uint8, device="cuda")
        w = torch.empty(L.snp_frame_encode_workspace(TOTAL), dtype=torch.uint8, device="cuda")
        r = {}
        med, ms = timed(lambda: r.__setitem__("e", cd.frame_encode(raw, out=one, work=w)), a.reps)
        n1 = int(r["e"][1].item())
        base["enc"] = med
        emit({"what": "snp_frame_encode_device (one stream)", "input_bytes": TOTAL, "framed_bytes": n1, "ms": round(med, 3),
              "ms_all": [round(x, 3) for x in ms], "input_GBps": round(TOTAL / med / 1e6, 2)})
        del w
        torch.cuda.empty_cache()
        back = torch.empty(TOTAL, dtype=torch.uint8, device="cuda")
        dw = torch.empty(L.snp_frame_decode_workspace(TOTAL // B), dtype=torch.uint8, device="cuda")
        med, ms = timed(lambda: r.__setitem__("d", cd.frame_decode(one[:n1], n1, back, TOTAL // B, work=dw)), a.reps)
        res = r["d"].cpu().tolist()
        base["dec"] = med
        emit({"what": "snp_frame_decode_device (one stream)", "output_bytes": TOTAL, "ms": round(med, 3), "ms_all": [round(x, 3) for x in ms],
              "output_GBps": round(TOTAL / med / 1e6, 2), "round_trip_ok": res == [TOTAL, 0] and torch.equal(back, raw)})
        del one, dw, back, r
        torch.cuda.empty_cache()

    for name, lens in shapes(a.shapes.split(",")).items():
        nb = len(lens)
        in_off = torch.from_numpy(np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)).cuda()
        in_len = torch.from_numpy(lens).cuda()
        caps = 10 + 8 * ((lens + B - 1) // B) + lens
        out_cap = torch.from_numpy(caps).cuda()
        out_off = torch.from_numpy(np.concatenate([[0], np.cumsum(caps)[:-1]]).astype(np.int64)).cuda()
        mc = int(((lens + B - 1) // B).sum())
        framed = torch.empty(int(caps.sum()), dtype=torch.uint8, device="cuda")
        ew = torch.empty(FL.snp_frame_encode_buffers_workspace(nb, mc), dtype=torch.uint8, device="cuda")
        res = {}

        def ecall():
            res["e"] = cd.frame_encode_buffers(raw, in_off, in_len, out=framed, out_off=out_off, out_cap=out_cap, max_chunks=mc, work=ew)

        t0 = time.time()
        med, ms = timed(ecall, a.reps)
        batch_ms = {"encode": med}
        _, _, f_len, est, eres = res["e"]
        er = eres.cpu().tolist()
        rec = {"what": "snp_frame_encode_buffers_batch", "shape": name, "buffers": nb, "chunks": mc, "input_bytes": int(lens.sum()),
               "workspace_bytes": ew.numel(), "ms": round(med, 3), "ms_all": [round(x, 3) for x in ms], "input_GBps": round(lens.sum() / med / 1e6, 2),
               "all_ok": int((est != 0).sum()) == 0, "result": er, "ratio": round(er[1] / lens.sum(), 4), "wall_s": round(time.time() - t0, 1)}
        if "enc" in base:
            rec["over_one_stream_rate"] = round(base["enc"] / med, 4)
        emit(rec)
        del ew
        torch.cuda.empty_cache()
        fl = f_len.cpu().numpy()
        ms_ = int(((fl + SPAN - 1) // SPAN).sum())
        back = torch.empty(int(lens.sum()), dtype=torch.uint8, device="cuda")
        dw = torch.empty(max(FL.snp_frame_decode_buffers_workspace(nb, mc, ms_), 1), dtype=torch.uint8, device="cuda")

        def dcall():
            res["d"] = cd.frame_decode_buffers(framed, out_off, f_len, back, in_off, in_len, max_chunks=mc, max_spans=ms_, work=dw)

        back.zero_()
        t0 = time.time()
        med, ms = timed(dcall, a.reps)
        batch_ms["decode"] = med
        ol, dst, dres = res["d"]
        ok = int((dst != 0).sum()) == 0 and torch.equal(ol, in_len) and torch.equal(back, raw[:back.numel()])
        rec = {"what": "snp_frame_decode_buffers_batch", "shape": name, "streams": nb, "chunks": mc, "spans": ms_, "output_bytes": int(lens.sum()),
               "workspace_bytes": dw.numel(), "ms": round(med, 3), "ms_all": [round(x, 3) for x in ms], "output_GBps": round(lens.sum() / med / 1e6, 2),
               "result": dres.cpu().tolist(), "round_trip_ok": ok, "wall_s": round(time.time() - t0, 1)}
        if "dec" in base:
            rec["over_one_stream_rate"] = round(base["dec"] / med, 4)
        emit(rec)
        del dw
        if name == "1m" and not a.no_loop:
            # the same streams one call each: snp_frame_encode_device, then snp_frame_decode_device (timed once, after a few warm-up calls)
            lw = torch.empty(L.snp_frame_encode_workspace(1 << 20), dtype=torch.uint8, device="cuda")
            ldw = torch.empty(L.snp_frame_decode_workspace(16), dtype=torch.uint8, device="cuda")
            lo, lc = out_off.cpu().numpy(), caps
            loop_out = torch.empty_like(framed)
            io = in_off.cpu().numpy()

            def enc_loop(k):
                for b in range(k):
                    cd.frame_encode(raw[io[b]:io[b] + lens[b]], out=loop_out[lo[b]:lo[b] + lc[b]], work=lw)

            def dec_loop(k):
                for b in range(k):
                    cd.frame_decode(framed[lo[b]:lo[b] + fl[b]], int(fl[b]), back[io[b]:io[b] + lens[b]], 16, work=ldw)

            back.zero_()
            for fn, what, kind in ((enc_loop, "snp_frame_encode_device per stream", "encode"), (dec_loop, "snp_frame_decode_device per stream", "decode")):
                fn(4)
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0 = time.time()
                e0.record()
                fn(nb)
                e1.record()
                torch.cuda.synchronize()
                t = e0.elapsed_time(e1)
                emit({"what": what, "shape": name, "streams": nb, "bytes": int(lens.sum()), "ms": round(t, 1), "GBps": round(lens.sum() / t / 1e6, 3),
                      "wall_s": round(time.time() - t0, 1), "batch_speedup": round(t / batch_ms[kind], 1)})
            same = torch.equal(back, raw[:back.numel()])
            emit({"what": "per-stream loop round trip", "shape": name, "round_trip_ok": same})
            del lw, ldw, loop_out
        del framed, back, res
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "a") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()

"""snp_frame_decode_range_batch times beside snp_frame_decode_buffers_batch on the same streams in the same process: 10 GiB of html-like data
(snappier_amd/datagen.py) in the shapes of compress_buffers_rates.py (64 KiB, 1 MiB, 64 MiB items), framed on the device (frame_encode_buffers).
Per shape, the full decode of every stream (exact bounds), then four windows of every stream through the range call (exact bounds, from its own
sizing call, which is timed too: the walk and the selection alone):

  * 1 MiB starting on a chunk boundary in the middle of the stream (no edge chunk);
  * 1 MiB starting 12 345 bytes further (two edge chunks per stream);
  * 4 KiB in the middle of a chunk (one chunk per stream, an edge);
  * the whole stream (every chunk interior: the same chunks as the full decode, plus the selection).

A window is clipped to the stream, so on the 64 KiB shape the two 1 MiB windows are the whole stream and the part of it behind byte 12 345.
ms from HIP events around each call (median of --reps after one warm-up); every result is checked against the input.  One JSON line per
measurement to --out.  The line of the 64 MiB shape carries the sanity condition the design rests on: a 1 MiB window must take less time than
the full decode of the same streams -- if not, the select kernel is hopping spans it should skip.

    python scripts/frame_range_rates.py --out profiles/r10a_frame_range_rates.jsonl
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

SPAN = 1 << 20


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="64k,1m,64m")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch
    from snappier_amd import batch as SB, datagen as SD, _native as N
    from compress_buffers_rates import B, TOTAL, shapes, timed

    html = open(os.path.join(ROOT, "tests", "golden", "testdata", "html"), "rb").read()
    raw = SD.html_like_blocks(html, 0, TOTAL // B, "cuda")
    cd = SB.BlockCodec(0, N.HASH_CRC32C)
    cd.ctx.reserve_compress(TOTAL // B)
    FL, RL = N.frame_buffers_lib(), N.frame_range_lib()
    lines = []

    def emit(rec):
        rec["where"] = torch.cuda.get_device_name(0)
        print(json.dumps(rec), flush=True)
        lines.append(rec)

    def rec_ms(med, ms):
        return {"ms": round(med, 4), "ms_all": [round(x, 4) for x in ms], "spread_ms": round(max(ms) - min(ms), 4)}

    def u8(n):
        return torch.empty(max(int(n), 1), dtype=torch.uint8, device="cuda")

    def i64(x):
        return torch.from_numpy(np.ascontiguousarray(x, dtype=np.int64)).cuda()

    back = torch.empty(TOTAL, dtype=torch.uint8, device="cuda")
    for name, lens in shapes(a.shapes.split(",")).items():
        nb, n = len(lens), int(lens[0])
        assert (lens == n).all()
        total = int(lens.sum())
        in_off, in_len = i64(np.arange(nb) * n), i64(lens)
        caps = 10 + 8 * ((lens + B - 1) // B) + lens
        mc = int(((lens + B - 1) // B).sum())
        framed = u8(caps.sum())
        f_off = i64(np.concatenate([[0], np.cumsum(caps)[:-1]]))
        _, _, f_len, est, _ = cd.frame_encode_buffers(raw, in_off, in_len, out=framed, out_off=f_off, out_cap=i64(caps), max_chunks=mc)
        torch.cuda.synchronize()
        assert int((est != 0).sum()) == 0
        framed, f_off = cd.compact(framed, f_off, f_len.to(torch.int32))   # the streams back to back, as a batch read from storage would be
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        spans = int(((f_len.cpu().numpy() + SPAN - 1) // SPAN).sum())
        common = {"shape": name, "streams": nb, "stream_bytes": n, "framed_bytes": int(f_len.sum())}
        res = {}

        # ---- the full decode -----------------------------------------------------------------------------------------------------------------
        dw = u8(FL.snp_frame_decode_buffers_workspace(nb, mc, spans))

        def full():
            res["d"] = cd.frame_decode_buffers(framed, f_off, f_len, back, in_off, in_len, max_chunks=mc, max_spans=spans, work=dw)

        back.zero_()
        med_full, ms_full = timed(full, a.reps)
        ol, st, _ = res["d"]
        ok = int((st != 0).sum()) == 0 and torch.equal(ol, in_len) and torch.equal(back[:total], raw[:total])
        emit({"what": "snp_frame_decode_buffers_batch, every stream whole, exact bounds", **common, "max_chunks": mc, "max_spans": spans,
              "output_bytes": total, **rec_ms(med_full, ms_full), "output_GBps": round(total / med_full / 1e6, 2), "round_trip_ok": ok})
        del dw

        # ---- the windows ---------------------------------------------------------------------------------------------------------------------
        mid = n // 2 // B * B
        windows = {"1 MiB, chunk-aligned": (mid, 1 << 20), "1 MiB, unaligned": (mid + 12345, 1 << 20), "4 KiB": (mid + 777, 4096),
                   "whole stream": (0, n)}
        for wname, (ro, rl) in windows.items():
            lo, hi = min(ro, n), min(ro + rl, n)
            w = hi - lo
            r_off, r_len = i64(np.full(nb, ro)), i64(np.full(nb, rl))
            o_off, o_cap = i64(np.arange(nb) * w), i64(np.full(nb, w))
            zw = u8(RL.snp_frame_decode_range_workspace(nb, 0, spans, 0))

            def sizing():
                res["s"] = cd.frame_decode_range_buffers(framed, f_off, f_len, r_off, r_len, back, o_off, o_cap, max_chunks=0, max_spans=spans,
                                                         edge_cap=0, work=zw)

            med_s, ms_s = timed(sizing, a.reps)
            need = res["s"][2].cpu().tolist()
            rmc, rec_ = need[0], need[4]
            rw = u8(RL.snp_frame_decode_range_workspace(nb, rmc, spans, rec_))

            def ranged():
                res["r"] = cd.frame_decode_range_buffers(framed, f_off, f_len, r_off, r_len, back, o_off, o_cap, max_chunks=rmc, max_spans=spans,
                                                         edge_cap=rec_, work=rw)

            back[:nb * w].zero_()
            med_r, ms_r = timed(ranged, a.reps)
            ol, st, result = res["r"]
            ok = int((st != 0).sum()) == 0 and int((ol != w).sum()) == 0 and \
                torch.equal(back[:nb * w].view(nb, w), raw[:total].view(nb, n)[:, lo:hi])
            line = {"what": "snp_frame_decode_range_batch", "window": wname, "range_off": ro, "range_len": rl, **common, "max_chunks": rmc,
                    "max_spans": spans, "edge_cap": rec_, "workspace_bytes": rw.numel(), "result": result.cpu().tolist(), "output_bytes": nb * w,
                    **rec_ms(med_r, ms_r), "output_GBps": round(nb * w / med_r / 1e6, 2), "sizing_call_ms": round(med_s, 4),
                    "full_decode_ms": round(med_full, 4), "over_full_decode": round(med_r / med_full, 4), "window_ok": ok}
            if name == "64m" and wname.startswith("1 MiB"):
                line["narrow_window_takes_less_than_the_full_decode"] = med_r < med_full      # the sanity condition (by construction)
            emit(line)
            del zw, rw
            res.pop("s"), res.pop("r")
        del framed
        res.clear()
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "a") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()

"""snp_frame_index_batch / snp_frame_read_indexed_batch times beside snp_frame_decode_range_batch on the same streams in the same process: 10 GiB
of html-like data (snappier_amd/datagen.py) in the shapes of compress_buffers_rates.py (64 KiB, 1 MiB, 64 MiB items), framed on the device
(frame_encode_buffers) and compacted.  Per shape, the index build beside snp_frame_decode_layout_batch (the same walk, without the rows); then,
per window of scripts/frame_range_rates.py (1 MiB on a chunk boundary, 1 MiB 12 345 bytes further, 4 KiB inside a chunk, the whole stream):

  * the range call with exact bounds, and its sizing call alone (the walk and the selection);
  * the indexed read of the same windows, one request per stream, exact bounds from its own sizing call (timed too: the plan alone).

On the 64 MiB shape also 16 windows of 64 KiB in each of the 160 streams: ONE indexed call of 2 560 requests against 16 range calls.
ms from HIP events around each call (median of --reps after one warm-up); every window is compared with the input.  One JSON line per
measurement to --out.  The lines of the 64 MiB shape carry the condition the index rests on, for both 1 MiB windows and the 4 KiB window:
indexed read < range call - 1/2 x (range sizing call alone), all three measured in this run.

    python scripts/frame_index_rates.py --out profiles/r12a_frame_index_rates.jsonl
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
    LL, RL, IL = N.layout_lib(), N.frame_range_lib(), N.frame_index_lib()
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

        # ---- the index build beside the layout call --------------------------------------------------------------------------------------------
        lw = u8(LL.snp_frame_decode_layout_workspace(nb, spans))

        def layout():
            res["l"] = cd.frame_decode_layout(framed, f_off, f_len, max_spans=spans, work=lw)

        med_l, ms_l = timed(layout, a.reps)
        iw = u8(IL.snp_frame_index_workspace(nb, spans))

        def build():
            res["i"] = cd.frame_index_buffers(framed, f_off, f_len, max_spans=spans, max_entries=mc, work=iw)

        med_i, ms_i = timed(build, a.reps)
        ix = res["i"]
        nchunks = (n + B - 1) // B
        ok = ix.result.cpu().tolist()[:3] == [mc, total, spans] and int((ix.tail != 0).sum()) == 0 and \
            torch.equal(ix.first, i64(np.arange(nb + 1) * nchunks)) and torch.equal(ix.total, in_len) and \
            torch.equal(ix.start.view(nb, nchunks), i64(np.arange(nchunks) * B).expand(nb, nchunks)) and torch.equal(ix.total, res["l"][2])
        emit({"what": "snp_frame_index_batch", **common, "max_spans": spans, "rows": mc, "index_bytes": 16 * mc + 20 * nb + 8,
              "result": ix.result.cpu().tolist(), **rec_ms(med_i, ms_i), "frame_decode_layout_ms": round(med_l, 4),
              "frame_decode_layout_ms_all": [round(x, 4) for x in ms_l], "over_layout_call": round(med_i / med_l, 4), "index_ok": ok})
        del lw, iw
        res.pop("l")
        req_stream = torch.arange(nb, dtype=torch.int32, device="cuda")

        def indexed(r_stream, r_off, r_len, o_off, o_cap):
            """-> (median ms, all ms, sizing median ms, the call's tensors, max_chunks, edge_cap, workspace bytes), exact bounds from its sizing call."""
            nreq = r_stream.numel()
            zw = u8(IL.snp_frame_read_indexed_workspace(nreq, 0, 0))

            def sizing():
                res["xs"] = cd.frame_read_indexed(framed, f_off, f_len, ix, r_stream, r_off, r_len, back, o_off, o_cap, max_chunks=0, edge_cap=0, work=zw)

            med_s, _ = timed(sizing, a.reps)
            need = res["xs"][2].cpu().tolist()
            xw = u8(IL.snp_frame_read_indexed_workspace(nreq, need[0], need[2]))

            def read():
                res["x"] = cd.frame_read_indexed(framed, f_off, f_len, ix, r_stream, r_off, r_len, back, o_off, o_cap, max_chunks=need[0],
                                                 edge_cap=need[2], work=xw)

            med, ms = timed(read, a.reps)
            return med, ms, med_s, res["x"], need[0], need[2], xw.numel()

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
            ol, st, _ = res["r"]
            want = raw[:total].view(nb, n)[:, lo:hi]
            range_ok = int((st != 0).sum()) == 0 and int((ol != w).sum()) == 0 and torch.equal(back[:nb * w].view(nb, w), want)
            del zw, rw
            back[:nb * w].zero_()
            med_x, ms_x, med_xs, (ol, st, result), xmc, xec, xbytes = indexed(req_stream, r_off, r_len, o_off, o_cap)
            ok = int((st != 0).sum()) == 0 and int((ol != w).sum()) == 0 and torch.equal(back[:nb * w].view(nb, w), want)
            line = {"what": "snp_frame_read_indexed_batch", "window": wname, "req_off": ro, "req_len": rl, **common, "requests": nb, "max_chunks": xmc,
                    "edge_cap": xec, "workspace_bytes": xbytes, "result": result.cpu().tolist(), "output_bytes": nb * w, **rec_ms(med_x, ms_x),
                    "output_GBps": round(nb * w / med_x / 1e6, 2), "sizing_call_ms": round(med_xs, 4), "range_call_ms": round(med_r, 4),
                    "range_call_ms_all": [round(x, 4) for x in ms_r], "range_sizing_call_ms": round(med_s, 4),
                    "range_sizing_call_ms_all": [round(x, 4) for x in ms_s], "range_max_chunks": rmc, "range_edge_cap": rec_,
                    "over_range_call": round(med_x / med_r, 4), "window_ok": ok, "range_window_ok": range_ok}
            if name == "64m" and wname != "whole stream":
                line["indexed_read_below_range_call_less_half_its_walk"] = med_x < med_r - 0.5 * med_s      # the condition the index rests on
            emit(line)
            res.clear()
            res["i"] = ix

        # ---- 16 windows of 64 KiB in every stream: one indexed call against 16 range calls ------------------------------------------------------
        if name == "64m":
            k, w = 16, B
            offs = (np.arange(k) * (n // k) + 4321) // 7 * 7             # spread over the stream, on no chunk boundary
            r_stream = torch.arange(nb, dtype=torch.int32, device="cuda").repeat_interleave(k)
            r_off, r_len = i64(np.tile(offs, nb)), i64(np.full(nb * k, w))
            o_off, o_cap = i64(np.arange(nb * k) * w), i64(np.full(nb * k, w))
            back[:nb * k * w].zero_()
            med_x, ms_x, med_xs, (ol, st, result), xmc, xec, xbytes = indexed(r_stream, r_off, r_len, o_off, o_cap)
            want = torch.stack([raw[:total].view(nb, n)[:, o:o + w] for o in offs.tolist()], dim=1)
            ok = int((st != 0).sum()) == 0 and int((ol != w).sum()) == 0 and torch.equal(back[:nb * k * w].view(nb, k, w), want)
            # the same windows through the range call: one call per window number, window j of every stream
            calls = []
            for j, o in enumerate(offs.tolist()):
                ro_j, oo_j = i64(np.full(nb, o)), i64((np.arange(nb) * k + j) * w)
                rl_j, oc_j = i64(np.full(nb, w)), i64(np.full(nb, w))
                need = cd.frame_decode_range_buffers(framed, f_off, f_len, ro_j, rl_j, back, oo_j, oc_j, max_chunks=0, max_spans=spans, edge_cap=0)[2].cpu().tolist()
                calls.append((ro_j, rl_j, oo_j, oc_j, need[0], need[4], u8(RL.snp_frame_decode_range_workspace(nb, need[0], spans, need[4]))))

            def sixteen():
                for ro_j, rl_j, oo_j, oc_j, m, e, wk in calls:
                    res["r"] = cd.frame_decode_range_buffers(framed, f_off, f_len, ro_j, rl_j, back, oo_j, oc_j, max_chunks=m, max_spans=spans, edge_cap=e, work=wk)

            back[:nb * k * w].zero_()
            med_r, ms_r = timed(sixteen, a.reps)
            range_ok = torch.equal(back[:nb * k * w].view(nb, k, w), want)
            emit({"what": "16 windows of 64 KiB in every stream: one snp_frame_read_indexed_batch against 16 snp_frame_decode_range_batch", **common,
                  "requests": nb * k, "max_chunks": xmc, "edge_cap": xec, "workspace_bytes": xbytes, "result": result.cpu().tolist(),
                  "output_bytes": nb * k * w, **rec_ms(med_x, ms_x), "sizing_call_ms": round(med_xs, 4), "range_calls_ms": round(med_r, 4),
                  "range_calls_ms_all": [round(x, 4) for x in ms_r], "over_range_calls": round(med_x / med_r, 4), "window_ok": ok,
                  "range_window_ok": range_ok})
            del calls
        del framed, ix
        res.clear()
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "a") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()

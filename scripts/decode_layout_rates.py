"""snp_frame_decode_layout_batch / snp_decompress_layout_batch times: 10 GiB of html-like data (snappier_amd/datagen.py) in the shapes of
compress_buffers_rates.py (64 KiB, 1 MiB, 64 MiB items), framed (frame_encode_buffers) and as blocks (compress_buffers) on the device.  Per shape:

  * the decode alone with the sizes known on the host (what frame_buffers_rates.py / decompress_buffers_rates.py time), exact bounds;
  * the same decode with the bounds a caller without the sizes can give (max_chunks / max_fragments = arena bytes / 65536);
  * the layout call alone;
  * layout + decode chained on one stream, nothing read between them, and its ratio to the decode alone: the price of not knowing the sizes;
  * once, for context, the route a caller has without the layout call: the compressed batch copied to (pinned) host memory, snp_frame_decoded_length
    / snp_get_uncompressed_length per item in one thread, the layout built and uploaded.

ms from HIP events around each call (median of --reps after one warm-up); every decode is checked against the input.  One JSON line per
measurement to --out.

    python scripts/decode_layout_rates.py --out profiles/r07d_decode_layout_rates.jsonl
    rocprofv3 --kernel-trace --output-format csv -d DIR -o run -- python scripts/decode_layout_rates.py --profile --reps 3
    python scripts/decode_layout_rates.py --trace DIR --reps 3 --stats-out profiles/r07d_decode_layout_kernel_stats.csv

--profile issues, per shape, only: frame layout x reps, frame decode (sizes known) x reps, block layout x reps -- so that --trace can cut the
kernel trace into calls (a frame layout ends with k_fl_write, a frame decode with k_fd_verdict, a block layout with k_bl_write) and average each
kernel's time per call over the repetitions after the first.
"""
import argparse
import csv
import ctypes as C
import glob
import json
import os
import re
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

SPAN = 1 << 20
ALIGN = 256


def kernel_stats(trace_dir, reps, shapes_run, out_path):
    """Cut a rocprofv3 kernel trace of a --profile run into calls and write kernel, launches and us per call."""
    files = sorted(glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True))
    if not files:
        sys.exit(f"no *kernel_trace.csv under {trace_dir}")
    rows = []
    for f in files:
        with open(f) as fh:
            rows += [(int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]) for r in csv.DictReader(fh)]
    rows.sort()

    def short(name):
        name = re.sub(r"\(anonymous namespace\)::", "", name)
        name = re.sub(r"^void ", "", name)
        name = re.sub(r"\s*\[clone .*\]$", "", name)
        return re.sub(r"\(.*\)$", "", name).replace(".kd", "")

    ends = {"k_fl_write": "frame layout", "k_fd_verdict": "frame decode", "k_bl_write": "block layout", "k_fe_emit": None}
    calls, cur = {"frame layout": [], "frame decode": [], "block layout": []}, None
    for t0, t1, name in rows:
        k = short(name)
        if cur is None and (k == "k_scan_reduce<ScanPieces>" or k == "k_lay_result_init"):
            cur = []
        if cur is None:
            continue
        cur.append((k, (t1 - t0) / 1000.0))
        if k in ends:
            if ends[k]:
                calls[ends[k]].append(cur)
            cur = None
    with open(out_path, "w", newline="") as fh:
        w = csv.writer(fh)
        w.writerow(["shape", "call", "kernel", "launches", "total_us", "pct_of_call_kernel_time"])
        for kind, groups in calls.items():
            per = reps + 1                                       # one warm-up and `reps` timed calls per shape
            if len(groups) != per * len(shapes_run):
                sys.exit(f"{kind}: {len(groups)} calls in the trace, expected {per * len(shapes_run)}")
            for si, shape in enumerate(shapes_run):
                mine = groups[si * per + 1:(si + 1) * per]       # (the warm-up call is left out)
                order, launches, us = [], {}, {}
                for g in mine:
                    for k, t in g:
                        if k not in us:
                            order.append(k)
                            launches[k], us[k] = 0, 0.0
                        launches[k] += 1
                        us[k] += t
                total = sum(us.values())
                for k in order:
                    w.writerow([shape, kind, k, launches[k] // len(mine), round(us[k] / len(mine), 2), round(100 * us[k] / total, 3)])
                w.writerow([shape, kind, "(all kernels)", sum(launches.values()) // len(mine), round(total / len(mine), 2), 100.0])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="64k,1m,64m")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--profile", action="store_true", help="only the calls --trace knows how to cut apart (see above)")
    ap.add_argument("--no-host", action="store_true", help="skip the host route")
    ap.add_argument("--trace", default=None, help="directory of a rocprofv3 --kernel-trace run of --profile: write --stats-out and exit")
    ap.add_argument("--stats-out", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.trace:
        kernel_stats(a.trace, a.reps, a.shapes.split(","), a.stats_out)
        return

    import torch
    from snappier_amd import batch as SB, datagen as SD, _native as N
    from compress_buffers_rates import B, TOTAL, shapes, timed

    html = open(os.path.join(ROOT, "tests", "golden", "testdata", "html"), "rb").read()
    raw = SD.html_like_blocks(html, 0, TOTAL // B, "cuda")
    cd = SB.BlockCodec(0, N.HASH_CRC32C)
    cd.ctx.reserve_compress(TOTAL // B)
    L, FL, BL, LL = N.lib(), N.frame_buffers_lib(), N.buffers_decompress_lib(), N.layout_lib()
    lines = []

    def emit(rec):
        rec["where"] = torch.cuda.get_device_name(0)
        print(json.dumps(rec), flush=True)
        lines.append(rec)

    def rec_ms(med, ms):
        return {"ms": round(med, 4), "ms_all": [round(x, 4) for x in ms], "spread_ms": round(max(ms) - min(ms), 4)}

    def u8(n):
        return torch.empty(max(int(n), 1), dtype=torch.uint8, device="cuda")

    back = torch.empty(TOTAL, dtype=torch.uint8, device="cuda")
    bound = TOTAL // B                                            # what a caller who knows only its arena can say: arena bytes / 65536
    for name, lens in shapes(a.shapes.split(",")).items():
        nb = len(lens)
        total = int(lens.sum())
        in_off = torch.from_numpy(np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)).cuda()
        in_len = torch.from_numpy(lens).cuda()
        res = {}

        # ---- framed streams ------------------------------------------------------------------------------------------------------------------
        caps = 10 + 8 * ((lens + B - 1) // B) + lens
        f_cap = torch.from_numpy(caps).cuda()
        f_off = torch.from_numpy(np.concatenate([[0], np.cumsum(caps)[:-1]]).astype(np.int64)).cuda()
        mc = int(((lens + B - 1) // B).sum())
        framed = u8(caps.sum())
        _, _, f_len, est, _ = cd.frame_encode_buffers(raw, in_off, in_len, out=framed, out_off=f_off, out_cap=f_cap, max_chunks=mc)
        torch.cuda.synchronize()
        assert int((est != 0).sum()) == 0
        framed, f_off = cd.compact(framed, f_off, f_len.to(torch.int32))   # the streams back to back, as a batch read from storage would be
        torch.cuda.synchronize()
        torch.cuda.empty_cache()                                  # (the compressor's staging and the capacity-sized tensor go)
        fl = f_len.cpu().numpy()
        ms_ = int(((fl + SPAN - 1) // SPAN).sum())
        span_bound = nb + (framed.numel() >> 20)                  # no host lengths needed
        lw = u8(LL.snp_frame_decode_layout_workspace(nb, span_bound))
        dw = u8(FL.snp_frame_decode_buffers_workspace(nb, bound, span_bound))

        def flayout():
            res["l"] = cd.frame_decode_layout(framed, f_off, f_len, align=ALIGN, arena_cap=TOTAL, max_spans=span_bound, work=lw)

        def fdecode_known(chunks=mc, spans=ms_):
            res["d"] = cd.frame_decode_buffers(framed, f_off, f_len, back, in_off, in_len, max_chunks=chunks, max_spans=spans, work=dw)

        def fchain():
            flayout()
            oo, oc = res["l"][0], res["l"][1]
            res["d"] = cd.frame_decode_buffers(framed, f_off, f_len, back, oo, oc, max_chunks=bound, max_spans=span_bound, work=dw)

        def fcheck():
            ol, st, _ = res["d"]
            return int((st != 0).sum()) == 0 and torch.equal(ol, in_len) and torch.equal(back[:total], raw[:total])

        common = {"shape": name, "streams": nb, "framed_bytes": int(fl.sum()), "output_bytes": total}
        med_l, ms_l = timed(flayout, a.reps)
        oo, oc, dl, nch, lst, lres = res["l"]
        layout_ok = int((lst != 0).sum()) == 0 and torch.equal(oo, in_off) and torch.equal(oc, in_len) and torch.equal(dl, in_len)
        emit({"what": "snp_frame_decode_layout_batch", **common, "max_spans": span_bound, "workspace_bytes": lw.numel(), **rec_ms(med_l, ms_l),
              "us": round(med_l * 1000, 1), "result": lres.cpu().tolist(), "layout_ok": layout_ok})
        back.zero_()
        med_d, ms_d = timed(fdecode_known, a.reps)
        emit({"what": "snp_frame_decode_buffers_batch, sizes known on the host, exact bounds", **common, "max_chunks": mc, "max_spans": ms_,
              **rec_ms(med_d, ms_d), "output_GBps": round(total / med_d / 1e6, 2), "round_trip_ok": fcheck()})
        if not a.profile:
            back.zero_()
            med_b, ms_b = timed(lambda: fdecode_known(bound, span_bound), a.reps)
            emit({"what": "snp_frame_decode_buffers_batch, sizes known on the host, a caller's bounds", **common, "max_chunks": bound,
                  "max_spans": span_bound, **rec_ms(med_b, ms_b), "output_GBps": round(total / med_b / 1e6, 2), "round_trip_ok": fcheck()})
            back.zero_()
            med_c, ms_c = timed(fchain, a.reps)
            emit({"what": "frame layout + decode, one stream, nothing read back", **common, "max_chunks": bound, "max_spans": span_bound,
                  **rec_ms(med_c, ms_c), "output_GBps": round(total / med_c / 1e6, 2), "round_trip_ok": fcheck(),
                  "over_decode_alone_exact_bounds": round(med_c / med_d, 4), "over_decode_alone_same_bounds": round(med_c / med_b, 4)})
            if not a.no_host:
                pinned = torch.empty(framed.numel(), dtype=torch.uint8, pin_memory=True)
                h_off = f_off.cpu().numpy()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                pinned.copy_(framed, non_blocking=True)
                torch.cuda.synchronize()
                t1 = time.perf_counter()
                base = pinned.data_ptr()
                fn = L.snp_frame_decoded_length
                v = C.c_uint64(0)
                dec = np.empty(nb, dtype=np.int64)
                for b in range(nb):
                    assert fn(C.c_void_p(base + int(h_off[b])), int(fl[b]), C.byref(v)) == 0
                    dec[b] = v.value
                slot = (dec + ALIGN - 1) // ALIGN * ALIGN
                h_oo = np.cumsum(slot) - slot
                t2 = time.perf_counter()
                d_oo, d_oc = torch.from_numpy(h_oo).cuda(), torch.from_numpy(dec).cuda()
                torch.cuda.synchronize()
                t3 = time.perf_counter()
                emit({"what": "host route: copy framed batch to pinned host memory, snp_frame_decoded_length per stream, upload", **common,
                      "copy_ms": round((t1 - t0) * 1e3, 2), "copy_GBps": round(framed.numel() / (t1 - t0) / 1e9, 2), "walk_ms": round((t2 - t1) * 1e3, 2),
                      "upload_ms": round((t3 - t2) * 1e3, 3), "total_ms": round((t3 - t0) * 1e3, 2), "copied_bytes": framed.numel(),
                      "same_layout": torch.equal(d_oo, oo) and torch.equal(d_oc, oc), "over_layout_call": round((t3 - t0) * 1e3 / med_l, 1)})
                del pinned
        del framed, lw, dw, res["l"], res["d"]
        torch.cuda.empty_cache()

        # ---- blocks --------------------------------------------------------------------------------------------------------------------------
        b_len = torch.from_numpy(lens.astype(np.uint32).view(np.int32)).cuda()
        comp, c_off, comp_len, status, _ = cd.compress_buffers(raw, in_off, b_len)
        torch.cuda.synchronize()
        assert int((status != 0).sum()) == 0, name
        c_len = comp_len.to(torch.int32)
        comp, c_off = cd.compact(comp, c_off, c_len)              # the blocks back to back
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        blw = u8(LL.snp_decompress_layout_workspace(nb))

        def blayout():
            res["l"] = cd.decompress_layout(comp, c_off, c_len, align=ALIGN, arena_cap=TOTAL, work=blw)

        common = {"shape": name, "blocks": nb, "compressed_bytes": int(comp_len.sum()), "output_bytes": total}
        med_l, ms_l = timed(blayout, a.reps)
        oo, oc, decl, lst, lres = res["l"]
        layout_ok = int((lst != 0).sum()) == 0 and torch.equal(oo, in_off) and torch.equal(oc, b_len) and torch.equal(decl, b_len)
        emit({"what": "snp_decompress_layout_batch", **common, "workspace_bytes": blw.numel(), **rec_ms(med_l, ms_l), "us": round(med_l * 1000, 1),
              "result": lres.cpu().tolist(), "layout_ok": layout_ok})
        if not a.profile:
            mf = int(cd.decompress_buffers(comp, c_off, c_len, back, in_off, b_len, max_fragments=0)[2][0].item())   # exact, as decompress_buffers_rates.py
            bw = u8(BL.snp_decompress_buffers_workspace(nb, bound))

            def bdecode_known(frags=mf):
                res["d"] = cd.decompress_buffers(comp, c_off, c_len, back, in_off, b_len, max_fragments=frags, work=bw)

            def bchain():
                blayout()
                res["d"] = cd.decompress_buffers(comp, c_off, c_len, back, res["l"][0], res["l"][1], max_fragments=bound, work=bw)

            def bcheck():
                ol, st, _ = res["d"]
                return int((st != 0).sum()) == 0 and torch.equal(ol, b_len) and torch.equal(back[:total], raw[:total])

            back.zero_()
            med_d, ms_d = timed(bdecode_known, a.reps)
            emit({"what": "snp_decompress_buffers_batch, sizes known on the host, exact bound", **common, "max_fragments": mf, **rec_ms(med_d, ms_d),
                  "output_GBps": round(total / med_d / 1e6, 2), "round_trip_ok": bcheck()})
            back.zero_()
            med_b, ms_b = timed(lambda: bdecode_known(bound), a.reps)
            emit({"what": "snp_decompress_buffers_batch, sizes known on the host, a caller's bound", **common, "max_fragments": bound,
                  **rec_ms(med_b, ms_b), "output_GBps": round(total / med_b / 1e6, 2), "round_trip_ok": bcheck()})
            back.zero_()
            med_c, ms_c = timed(bchain, a.reps)
            emit({"what": "block layout + decode, one stream, nothing read back", **common, "max_fragments": bound, **rec_ms(med_c, ms_c),
                  "output_GBps": round(total / med_c / 1e6, 2), "round_trip_ok": bcheck(), "over_decode_alone_exact_bound": round(med_c / med_d, 4),
                  "over_decode_alone_same_bound": round(med_c / med_b, 4)})
            if not a.no_host:
                pinned = torch.empty(comp.numel(), dtype=torch.uint8, pin_memory=True)
                h_off, h_len = c_off.cpu().numpy(), comp_len.cpu().numpy()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                pinned.copy_(comp, non_blocking=True)
                torch.cuda.synchronize()
                t1 = time.perf_counter()
                base = pinned.data_ptr()
                fn = L.snp_get_uncompressed_length
                v, hb = C.c_uint32(0), C.c_uint32(0)
                dec = np.empty(nb, dtype=np.int64)
                for b in range(nb):
                    assert fn(C.c_void_p(base + int(h_off[b])), int(h_len[b]), C.byref(v), C.byref(hb)) == 0
                    dec[b] = v.value
                slot = (dec + ALIGN - 1) // ALIGN * ALIGN
                h_oo = np.cumsum(slot) - slot
                t2 = time.perf_counter()
                d_oo, d_oc = torch.from_numpy(h_oo).cuda(), torch.from_numpy(dec.astype(np.uint32).view(np.int32)).cuda()
                torch.cuda.synchronize()
                t3 = time.perf_counter()
                emit({"what": "host route: copy compressed batch to pinned host memory, snp_get_uncompressed_length per block, upload", **common,
                      "copy_ms": round((t1 - t0) * 1e3, 2), "copy_GBps": round(comp.numel() / (t1 - t0) / 1e9, 2), "walk_ms": round((t2 - t1) * 1e3, 2),
                      "upload_ms": round((t3 - t2) * 1e3, 3), "total_ms": round((t3 - t0) * 1e3, 2), "copied_bytes": comp.numel(),
                      "same_layout": torch.equal(d_oo, oo) and torch.equal(d_oc, oc), "over_layout_call": round((t3 - t0) * 1e3 / med_l, 1)})
                del pinned
            del bw
        del comp, c_off, comp_len, c_len, blw
        res.clear()
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "a") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()

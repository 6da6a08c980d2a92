"""snp_frame_encode_chunked_batch rates at the seek granularities: 10 GiB of html-like data (snappier_amd/datagen.py) in a uniform shape of
compress_buffers_rates.py (default 64k: 163 840 buffers of 64 KiB), each buffer one framed stream, at chunk sizes 65536, 16384, 4096, 1024, 256.
Per chunk size, in one process:

  * the call without and with the index, beside snp_compress_batch + snp_crc32c_batch over the same pieces (what the plan, the scans and the
    emit cost on top of the two codec launches), and beside snp_frame_index_batch over the emitted streams (the walk the caller no longer makes);
    the encoder's index is compared with that walk's, array for array, and the streams are decoded back and compared with the input
    (snp_frame_decode_buffers_batch: its time and d_result[3] are reported too);
  * at 65536 the call without an index INTERLEAVED with snp_frame_encode_buffers_batch: the condition is that its median is not above that
    call's median by more than that call's own min-to-max spread.

Then the payoff (--no-payoff skips it): one 4 KiB window per stream, off a chunk boundary, through snp_frame_read_indexed_batch over streams
encoded at 65536 and at 4096 with the encoder's index, and the compressed-size ratio of the two encodings.
ms from HIP events around each call (median of --reps after one warm-up).  One JSON line per measurement to --out.

    python scripts/frame_chunked_rates.py --out profiles/r12a_frame_chunked_rates.jsonl
    rocprofv3 --kernel-trace --stats -d DIR -o run -- python scripts/frame_chunked_rates.py --chunks 4096 --reps 2 --encode-only
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
from compress_buffers_rates import B, TOTAL, shapes, timed  # noqa: E402

SPAN = 1 << 20


def i64(x):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.int64)).cuda()


def u8(n):
    return torch.empty(max(int(n), 1), dtype=torch.uint8, device="cuda")


def rec_ms(med, ms, key="ms"):
    return {key: round(med, 3), key + "_all": [round(x, 3) for x in ms], key.replace("ms", "spread_ms"): round(max(ms) - min(ms), 3)}


def interleaved(f, g, reps):
    """f and g timed in turn, reps times each after one warm-up of both: -> ((median, all) of f, (median, all) of g)."""
    f()
    g()
    torch.cuda.synchronize()
    ms = ([], [])
    for _ in range(reps):
        for k, fn in enumerate((f, g)):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            ms[k].append(a.elapsed_time(b))
    return (float(np.median(ms[0])), ms[0]), (float(np.median(ms[1])), ms[1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="64k", help="64k | 1m | 64m (uniform buffers whose length every chunk size divides)")
    ap.add_argument("--chunks", default="65536,16384,4096,1024,256")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--encode-only", action="store_true", help="the call without an index only (profiling runs)")
    ap.add_argument("--no-payoff", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    html = open(os.path.join(ROOT, "tests", "golden", "testdata", "html"), "rb").read()
    raw = SD.html_like_blocks(html, 0, TOTAL // B, "cuda")
    cd = SB.BlockCodec(0, N.HASH_CRC32C)
    cd.ctx.reserve_compress(TOTAL // B)                          # the table workspace before the buffers crowd the device (as bench.py)
    CL, FL, IL = N.frame_chunked_lib(), N.frame_buffers_lib(), N.frame_index_lib()
    lines = []

    def emit(rec):
        rec["where"] = torch.cuda.get_device_name(0)
        print(json.dumps(rec), flush=True)
        lines.append(rec)

    lens = shapes([a.shape])[a.shape]
    nb, n, total = len(lens), int(lens[0]), int(lens.sum())
    in_off, in_len = i64(np.arange(nb) * n), i64(lens)
    sizes = {}

    def encoded(cb, with_index, framed=None, work=None):
        """-> (call, M, out_off, out_cap, framed, work): the call at chunk size cb with exact bounds and every buffer passed in."""
        assert n % cb == 0
        chunks = lens // cb
        caps = 10 + 8 * chunks + lens
        mc = int(chunks.sum())
        out_off, out_cap = i64(np.concatenate([[0], np.cumsum(caps)[:-1]])), i64(caps)
        framed = u8(caps.sum()) if framed is None else framed
        work = u8(CL.snp_frame_encode_chunked_workspace(nb, mc, cb)) if work is None else work
        res = {}

        def call():
            res["e"] = cd.frame_encode_seekable(raw, in_off, in_len, cb, with_index=with_index, out=framed, out_off=out_off, out_cap=out_cap,
                                                max_chunks=mc, work=work)
        return call, res, mc, out_off, out_cap, framed, work

    for cb in [int(x) for x in a.chunks.split(",")]:
        call, res, mc, out_off, out_cap, framed, work = encoded(cb, False)
        common = {"shape": a.shape, "buffers": nb, "chunk_bytes": cb, "chunks": mc, "input_bytes": total}
        med, ms = timed(call, a.reps)
        _, _, f_len, est, eres, _ = res["e"]
        er = eres.cpu().tolist()
        sizes[cb] = er[1]
        line = {"what": "snp_frame_encode_chunked_batch, no index", **common, "workspace_bytes": work.numel(), "workspace_over_input": round(work.numel() / total, 3),
                **rec_ms(med, ms), "input_GBps": round(total / med / 1e6, 2), "all_ok": er[3] == nb, "result": er, "ratio": round(er[1] / total, 4)}
        if cb == B and not a.encode_only:
            ew = u8(FL.snp_frame_encode_buffers_workspace(nb, mc))
            ref = u8(framed.numel())
            old = {}

            def old_call():
                old["e"] = cd.frame_encode_buffers(raw, in_off, in_len, out=ref, out_off=out_off, out_cap=out_cap, max_chunks=mc, work=ew)

            (m_old, ms_old), (m_new, ms_new) = interleaved(old_call, call, a.reps)
            same = torch.equal(ref, framed) and torch.equal(old["e"][2], res["e"][2]) and old["e"][4].cpu().tolist() == res["e"][4].cpu().tolist()[:2]
            spread = max(ms_old) - min(ms_old)
            line.update({"interleaved": {**rec_ms(m_new, ms_new), **rec_ms(m_old, ms_old, "frame_encode_buffers_ms")}, "same_bytes_as_frame_encode_buffers": same,
                         "not_slower_than_frame_encode_buffers_by_more_than_its_spread": m_new <= m_old + spread})
            del ew, ref, old
        emit(line)
        if a.encode_only:
            del framed, work, res, call
            torch.cuda.empty_cache()
            continue
        # with the index, next to the walk over the emitted streams
        call_i, res_i, *_ = encoded(cb, True, framed, work)
        med_i, ms_i = timed(call_i, a.reps)
        _, _, f_len, est, eres, index = res_i["e"]
        del work, call, call_i, res                              # (the closures hold the workspace)
        torch.cuda.empty_cache()
        spans = int(((f_len.cpu().numpy() + SPAN - 1) // SPAN).sum())
        iw = u8(IL.snp_frame_index_workspace(nb, spans))
        walk = {}

        def walked():
            walk["i"] = cd.frame_index_buffers(framed, out_off, f_len, max_spans=spans, max_entries=mc, work=iw)

        med_w, ms_w = timed(walked, a.reps)
        same = all(torch.equal(getattr(index, k), getattr(walk["i"], k)) for k in ("first", "start", "pos", "total", "tail"))
        emit({"what": "snp_frame_encode_chunked_batch, with index", **common, **rec_ms(med_i, ms_i), "input_GBps": round(total / med_i / 1e6, 2),
              "result": eres.cpu().tolist(), "index_price_ms": round(med_i - med, 3), "frame_index_batch_ms": round(med_w, 3),
              "frame_index_batch_ms_all": [round(x, 3) for x in ms_w], "index_equals_the_walks": same})
        del iw, walk, res_i
        # the two codec launches alone over the same pieces
        p_off, p_len = i64(np.arange(mc) * cb), torch.full((mc,), cb, dtype=torch.int32, device="cuda")
        stride = (N.lib().snp_max_compressed_length(cb) + 15) // 16 * 16 + 16    # the staging stride of the chunked call
        s_off, stage = i64(np.arange(mc) * stride), u8(mc * stride)

        def codec():
            cd.compress(raw, p_off, p_len, out=stage, out_off=s_off)
            cd.crc32c(raw, p_off, p_len, masked=True)

        med_c, ms_c = timed(codec, a.reps)
        emit({"what": "snp_compress_batch + snp_crc32c_batch over the same pieces", **common, **rec_ms(med_c, ms_c), "input_GBps": round(total / med_c / 1e6, 2),
              "chunked_call_over_codec_launches": round(med / med_c, 4), "plan_scans_emit_ms": round(med - med_c, 3)})
        del stage, s_off, p_off, p_len
        torch.cuda.empty_cache()
        # the round trip: every stream decoded back (the decode walk over many small chunks is reported, not tuned)
        back = u8(total)
        dw = u8(FL.snp_frame_decode_buffers_workspace(nb, mc, spans))
        dec = {}

        def decode():
            dec["d"] = cd.frame_decode_buffers(framed, out_off, f_len, back, in_off, in_len, max_chunks=mc, max_spans=spans, work=dw)

        back.zero_()
        med_d, ms_d = timed(decode, min(a.reps, 3))
        ol, dst, dres = dec["d"]
        ok = int((dst != 0).sum()) == 0 and torch.equal(ol, in_len) and torch.equal(back, raw[:total])
        emit({"what": "snp_frame_decode_buffers_batch over the chunked streams", **common, "spans": spans, **rec_ms(med_d, ms_d),
              "output_GBps": round(total / med_d / 1e6, 2), "result": dres.cpu().tolist(), "round_trip_ok": ok})
        del back, dw, dec, framed, index
        torch.cuda.empty_cache()

    if not a.no_payoff and not a.encode_only:
        # one 4 KiB window per stream, off a chunk boundary, through the encoder's index: streams of 65536-byte chunks against 4096-byte chunks
        ro, rl = n // 2 // B * B + 777, 4096
        want = raw[:total].view(nb, n)[:, ro:ro + rl]
        req_stream = torch.arange(nb, dtype=torch.int32, device="cuda")
        r_off, r_len = i64(np.full(nb, ro)), i64(np.full(nb, rl))
        o_off, o_cap = i64(np.arange(nb) * rl), i64(np.full(nb, rl))
        back = u8(nb * rl)
        got = {}
        for cb in (B, 4096):
            call, res, mc, out_off, out_cap, framed, work = encoded(cb, True)
            call()
            _, _, f_len, est, eres, index = res["e"]
            torch.cuda.synchronize()
            del work, call
            torch.cuda.empty_cache()
            need = cd.frame_read_indexed(framed, out_off, f_len, index, req_stream, r_off, r_len, back, o_off, o_cap, max_chunks=0, edge_cap=0)[2].cpu().tolist()
            xw = u8(IL.snp_frame_read_indexed_workspace(nb, need[0], need[2]))
            x = {}

            def read():
                x["r"] = cd.frame_read_indexed(framed, out_off, f_len, index, req_stream, r_off, r_len, back, o_off, o_cap, max_chunks=need[0],
                                               edge_cap=need[2], work=xw)

            back.zero_()
            med, ms = timed(read, a.reps)
            ol, st, result = x["r"]
            ok = int((st != 0).sum()) == 0 and int((ol != rl).sum()) == 0 and torch.equal(back.view(nb, rl), want)
            got[cb] = (med, eres.cpu().tolist()[1])
            emit({"what": "snp_frame_read_indexed_batch, one 4 KiB window per stream through the encoder's index", "shape": a.shape, "streams": nb,
                  "chunk_bytes": cb, "req_off": ro, "req_len": rl, "framed_bytes": got[cb][1], "max_chunks": need[0], "edge_cap": need[2],
                  **rec_ms(med, ms), "result": result.cpu().tolist(), "window_ok": ok})
            del framed, xw, index, x, res
            torch.cuda.empty_cache()
        emit({"what": "payoff of 4096-byte chunks for 4 KiB windows", "shape": a.shape, "read_ms_at_65536": round(got[B][0], 3),
              "read_ms_at_4096": round(got[4096][0], 3), "read_speedup": round(got[B][0] / got[4096][0], 2),
              "compressed_size_ratio_4096_over_65536": round(got[4096][1] / got[B][1], 4)})
    if a.out:
        with open(a.out, "a") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()

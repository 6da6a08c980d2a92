"""snp_frame_append_indexed_batch rates: html-like data (snappier_amd/datagen.py) kept as seekable framed streams with their index, each stream in a
region of an arena that it may grow into, and bytes appended to them in place:

  * a: 10 GiB as 160 streams of 64 MiB at 65536-byte chunks, 4 KiB appended to each -- beside it, interleaved in the same process, what a caller
       must do without the call: snp_frame_decode_buffers_batch of every stream plus snp_frame_encode_chunked_batch of every stream with its
       4 KiB behind it;
  * b: 163 840 streams of 62 KiB at 4096-byte chunks (a tail of 2048 bytes each), 1000 bytes appended to each: every stream reopens its tail;
  * c: bulk -- 1 GiB appended as 64 KiB to each of 16 384 streams of 96 KiB at 65536-byte chunks (a tail of 32 KiB each) -- beside it, interleaved,
       snp_frame_encode_chunked_batch of the same appended bytes alone.

A call that reopens tails changes the bytes it read, so the arena is put back (a device copy, outside the timed interval) before every call.
Every appended arena is checked: the appended ranges read back through the new index (a), the streams decoded whole against A || S (b, c), and
the new index against snp_frame_index_batch over the new streams.  ms from HIP events around each call (median of --reps after one warm-up).
One JSON line per measurement to --out.

    python scripts/frame_append_rates.py --out profiles/r15a_frame_append_rates.jsonl
    rocprofv3 --kernel-trace --stats -d DIR -o run -- python scripts/frame_append_rates.py --cases c --reps 2 --append-only
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
from compress_buffers_rates import B, TOTAL  # noqa: E402
from frame_chunked_rates import i64, rec_ms, u8  # noqa: E402

SPAN = 1 << 20
# name -> (streams, decoded bytes of each, chunk_bytes, appended bytes to each)
CASES = {"a": (TOTAL >> 26, 64 << 20, 65536, 4096), "b": (TOTAL // B, B - 2048, 4096, 1000), "c": (16384, B + B // 2, 65536, B)}


def timed_after(restore, fns, reps):
    """The calls of fns timed in turn, reps times each after one warm-up of all, restore() before each (outside the interval): -> [(median, all)]."""
    for fn in fns:
        restore()
        fn()
    torch.cuda.synchronize()
    ms = [[] for _ in fns]
    for _ in range(reps):
        for k, fn in enumerate(fns):
            restore()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            ms[k].append(a.elapsed_time(b))
    return [(float(np.median(m)), m) for m in ms]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="a,b,c")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--append-only", action="store_true", help="the append only, no comparison and no check (profiling runs)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    html = open(os.path.join(ROOT, "tests", "golden", "testdata", "html"), "rb").read()
    raw = SD.html_like_blocks(html, 0, TOTAL // B, "cuda")
    cd = SB.BlockCodec(0, N.HASH_CRC32C)
    cd.ctx.reserve_compress(TOTAL // B)
    AL, CL, FL = N.frame_append_lib(), N.frame_chunked_lib(), N.frame_buffers_lib()
    lines = []

    def emit(rec):
        rec["where"] = torch.cuda.get_device_name(0)
        print(json.dumps(rec), flush=True)
        lines.append(rec)

    for case in a.cases.split(","):
        nb, n, cb, add = CASES[case]
        stride = (n + B - 1) // B * B                                   # where stream b's bytes start in the generated data
        in_off, in_len = i64(np.arange(nb) * stride), i64(np.full(nb, n))
        mc = nb * ((n + cb - 1) // cb)
        cap = 10 + 8 * ((n + add + cb - 1) // cb + 1) + n + add         # room for A || S however it compresses
        r_off, r_cap = i64(np.arange(nb) * cap), i64(np.full(nb, cap))
        arena = u8(nb * cap)
        ework = u8(CL.snp_frame_encode_chunked_workspace(nb, mc, cb))
        _, _, f_len, est, eres, index = cd.frame_encode_seekable(raw, in_off, in_len, cb, out=arena, out_off=r_off, out_cap=r_cap, max_chunks=mc, work=ework)
        torch.cuda.synchronize()
        assert int((est != 0).sum()) == 0
        # the appended bytes: the data of the neighbouring stream (as compressible as what they follow), packed
        neighbour = torch.roll(torch.arange(nb, device="cuda"), 1)
        src = raw[:nb * stride].view(nb, stride)[neighbour, 777:777 + add].contiguous().view(-1)
        s_off, s_len = i64(np.arange(nb) * add), i64(np.full(nb, add))
        need = cd.frame_append_indexed(arena, r_off, f_len, r_cap, index, src, s_off, s_len, cb, 0, 0)[3].cpu().tolist()
        mt, ms = need[2], need[0]
        work = u8(AL.snp_frame_append_indexed_workspace(nb, mt, ms, cb))
        saved = arena.clone() if mt else None                           # (with no tail reopened the call writes what it wrote before)
        got = {}

        def restore():
            if saved is not None:
                arena.copy_(saved)

        def append():
            got["a"] = cd.frame_append_indexed(arena, r_off, f_len, r_cap, index, src, s_off, s_len, cb, mt, ms, work=work)

        common = {"case": case, "streams": nb, "chunk_bytes": cb, "decoded_bytes": nb * n, "framed_bytes": int(eres[1].item()), "appended_bytes": nb * add,
                  "reopened_tails": mt, "fresh_slots": ms, "workspace_bytes": work.numel()}
        fns, names = [append], []
        back = dwork = e2work = out2 = None
        if not a.append_only and case == "a":
            # what the caller does today: decode every stream, encode every stream with its appended bytes behind it
            spans = int(((f_len.cpu().numpy() + SPAN - 1) // SPAN).sum()) + nb
            b_off, b_len = i64(np.arange(nb) * (n + add)), i64(np.full(nb, n + add))
            back = u8(nb * (n + add))
            back.view(nb, n + add)[:, n:] = src.view(nb, add)
            dwork = u8(FL.snp_frame_decode_buffers_workspace(nb, mc, spans))
            mc2 = nb * ((n + add + cb - 1) // cb)
            e2work = u8(CL.snp_frame_encode_chunked_workspace(nb, mc2, cb))
            out2 = u8(nb * cap)

            def today():
                cd.frame_decode_buffers(arena, r_off, f_len, back, b_off, in_len, max_chunks=mc, max_spans=spans, work=dwork)
                cd.frame_encode_seekable(back, b_off, b_len, cb, out=out2, out_off=r_off, out_cap=r_cap, max_chunks=mc2, work=e2work)

            fns.append(today)
            names.append("frame_decode_buffers + frame_encode_seekable of every whole stream (what a caller does today)")
        if not a.append_only and case == "c":
            mc2 = nb * ((add + cb - 1) // cb)
            e2work = u8(CL.snp_frame_encode_chunked_workspace(nb, mc2, cb))
            out2 = u8(nb * cap)

            def alone():
                cd.frame_encode_seekable(src, s_off, s_len, cb, out=out2, out_off=r_off, out_cap=r_cap, max_chunks=mc2, work=e2work)

            fns.append(alone)
            names.append("snp_frame_encode_chunked_batch of the same appended bytes alone")
        res = timed_after(restore, fns, a.reps)
        restore()                                                       # the arena as one append leaves it, for the checks
        append()
        torch.cuda.synchronize()
        new_len, st, new_ix, result, _ = got["a"]
        line = {"what": "snp_frame_append_indexed_batch", **common, **rec_ms(*res[0]), "result": result.cpu().tolist(),
                "all_written": int((st != 0).sum()) == 0, "appended_GBps": round(nb * add / res[0][0] / 1e6, 2)}
        if not a.append_only:
            used = int(new_ix.first[-1].item())
            spans = int(((new_len.cpu().numpy() + SPAN - 1) // SPAN).sum()) + nb
            walked = cd.frame_index_buffers(arena, r_off, new_len, max_spans=spans, max_entries=used)
            line["new_index_equals_the_walks"] = bool(torch.equal(walked.first, new_ix.first) and torch.equal(walked.start, new_ix.start[:used]) and
                                                      torch.equal(walked.pos, new_ix.pos[:used]) and torch.equal(walked.total, new_ix.total) and
                                                      torch.equal(walked.tail, new_ix.tail))
            if case == "a":                                             # the appended ranges through the new index
                rd = u8(nb * add)
                rl, rs, _ = cd.frame_read_indexed(arena, r_off, new_len, new_ix, torch.arange(nb, dtype=torch.int32, device="cuda"), i64(np.full(nb, n)),
                                                  s_len, rd, s_off, s_len)
                line["appended_bytes_read_back"] = int((rs != 0).sum()) == 0 and bool(torch.equal(rd, src))
            else:                                                       # every stream decoded whole against A || S
                whole = u8(nb * (n + add))
                w_off, w_len = i64(np.arange(nb) * (n + add)), i64(np.full(nb, n + add))
                dw = u8(FL.snp_frame_decode_buffers_workspace(nb, used, spans))
                ol, dst, _ = cd.frame_decode_buffers(arena, r_off, new_len, whole, w_off, w_len, max_chunks=used, max_spans=spans, work=dw)
                v = whole.view(nb, n + add)
                line["round_trip_ok"] = int((dst != 0).sum()) == 0 and bool(torch.equal(v[:, :n], raw[:nb * stride].view(nb, stride)[:, :n]) and
                                                                            torch.equal(v[:, n:], src.view(nb, add)))
                del whole, dw, v
            for name, r in zip(names, res[1:]):
                emit({"what": name, **common, **rec_ms(*r)})
                spread = max(r[1]) - min(r[1])
                line.update({"other_ms": round(r[0], 3), "other_spread_ms": round(spread, 3), "other_over_append": round(r[0] / res[0][0], 2)})
        emit(line)
        del arena, saved, work, ework, index, got, src, back, dwork, e2work, out2
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "a") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()

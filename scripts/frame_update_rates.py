"""snp_frame_write_indexed_batch rates: 10 GiB of html-like data (snappier_amd/datagen.py) kept as seekable framed streams with their index, in two
shapes -- 160 streams of 64 MiB at 65536-byte chunks (64m) and 163 840 streams of 64 KiB at 4096-byte chunks (64k) -- and small writes into them:

  * one 4 KiB window per stream off a chunk boundary (both shapes);
  * one 1 MiB window per stream, and 16 windows of 64 KiB per stream (64m only).

Beside each write, in the same process: what a caller must do without the call -- snp_frame_decode_buffers_batch of every stream plus
snp_frame_encode_chunked_batch of every stream -- and a plain device copy of the framed arena, the floor of the emit's verbatim copy.  Every
updated arena is decoded back and compared with the patched data, and the returned positions with snp_frame_index_batch over the new streams.
ms from HIP events around each call (median of --reps after one warm-up).  One JSON line per measurement to --out.

    python scripts/frame_update_rates.py --out profiles/r13a_frame_update_rates.jsonl
    rocprofv3 --kernel-trace --stats -d DIR -o run -- python scripts/frame_update_rates.py --shapes 64k --reps 2 --update-only
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
from frame_chunked_rates import i64, rec_ms, u8  # noqa: E402

SPAN = 1 << 20
CHUNK = {"64m": 65536, "64k": 4096}


def writes_of(shape, n):
    """name -> (offsets within a stream, length): sorted, disjoint, off the chunk boundaries."""
    w = {"one 4 KiB window per stream": ([n // 2 + 777], 4096)}
    if shape == "64m":
        w["one 1 MiB window per stream"] = ([n // 2 + 777], 1 << 20)
        w["16 windows of 64 KiB per stream"] = ([k * (n // 16) + 4242 for k in range(16)], 65536)
    return w


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="64m,64k")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--update-only", action="store_true", help="the 4 KiB update only, no comparison (profiling runs)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    html = open(os.path.join(ROOT, "tests", "golden", "testdata", "html"), "rb").read()
    raw = SD.html_like_blocks(html, 0, TOTAL // B, "cuda")
    cd = SB.BlockCodec(0, N.HASH_CRC32C)
    cd.ctx.reserve_compress(TOTAL // B)
    UL, CL, FL = N.frame_update_lib(), N.frame_chunked_lib(), N.frame_buffers_lib()
    lines = []

    def emit(rec):
        rec["where"] = torch.cuda.get_device_name(0)
        print(json.dumps(rec), flush=True)
        lines.append(rec)

    for shape in a.shapes.split(","):
        cb = CHUNK[shape]
        lens = shapes([shape])[shape]
        nb, n, total = len(lens), int(lens[0]), int(lens.sum())
        in_off, in_len = i64(np.arange(nb) * n), i64(lens)
        chunks = lens // cb
        mc = int(chunks.sum())
        caps = 10 + 8 * chunks + lens
        f_off, f_cap = i64(np.concatenate([[0], np.cumsum(caps)[:-1]])), i64(caps)
        framed = u8(caps.sum())
        ework = u8(CL.snp_frame_encode_chunked_workspace(nb, mc, cb))
        _, _, f_len, est, eres, index = cd.frame_encode_seekable(raw, in_off, in_len, cb, out=framed, out_off=f_off, out_cap=f_cap, max_chunks=mc, work=ework)
        torch.cuda.synchronize()
        assert int((est != 0).sum()) == 0
        framed_bytes = int(eres[1].item())
        spans = int(((f_len.cpu().numpy() + SPAN - 1) // SPAN).sum())
        common = {"shape": shape, "streams": nb, "chunk_bytes": cb, "chunks": mc, "decoded_bytes": total, "framed_bytes": framed_bytes}
        out = u8(framed.numel() + 16 * nb * 16)
        todo = writes_of(shape, n)
        if a.update_only:
            todo = {k: v for k, v in todo.items() if "4 KiB" in k}
        base = None
        for name, (offs, ln) in todo.items():
            per = len(offs)
            nreq = nb * per
            req_stream = torch.arange(nb, dtype=torch.int32, device="cuda").repeat_interleave(per)
            req_off = i64(np.tile(np.array(offs, dtype=np.int64), nb))
            req_len = i64(np.full(nreq, ln))
            # the new bytes: the data of the neighbouring stream at the same place (as compressible as what they replace)
            neighbour = torch.roll(torch.arange(nb, device="cuda"), 1)
            src = raw[:total].view(nb, n)[neighbour, offs[0]:offs[0] + ln].repeat(1, per).reshape(-1).contiguous()
            src_off = i64(np.arange(nreq) * ln)
            sizing = cd.frame_write_indexed(framed, f_off, f_len, index, req_stream, req_off, src, src_off, req_len, out, f_off, torch.zeros_like(f_cap), 0, 0,
                                            with_bound=True)
            need, bound = sizing[4].cpu().tolist(), sizing[5]
            o_off = torch.cumsum(bound, 0) - bound
            assert int(bound.sum().item()) <= out.numel()
            work = u8(UL.snp_frame_write_indexed_workspace(nb, nreq, need[0], need[2]))
            got = {}

            def update():
                got["u"] = cd.frame_write_indexed(framed, f_off, f_len, index, req_stream, req_off, src, src_off, req_len, out, o_off, bound,
                                                  max_slots=need[0], stage_cap=need[2], work=work)

            med, ms = timed(update, a.reps)
            o_len, st, rst, new_ix, res, _ = got["u"]
            line = {"what": "snp_frame_write_indexed_batch: " + name, **common, "requests": nreq, "written_bytes": nreq * ln, "dirty_slots": need[0],
                    "staging_bytes": need[2], "workspace_bytes": work.numel(), **rec_ms(med, ms), "result": res.cpu().tolist(),
                    "all_written": int((st != 0).sum()) == 0 and int((rst != 0).sum()) == 0}
            if not a.update_only:
                # the round trip: the new streams decoded back against the patched data; the new positions against the walk
                back = u8(total)
                dwork = u8(FL.snp_frame_decode_buffers_workspace(nb, mc, spans + nb))
                ol, dst, _ = cd.frame_decode_buffers(out, o_off, o_len, back, in_off, in_len, max_chunks=mc, max_spans=spans + nb, work=dwork)
                want = raw[:total].clone().view(nb, n)
                for k, o in enumerate(offs):
                    want[:, o:o + ln] = src.view(nb, per, ln)[:, k]
                walked = cd.frame_index_buffers(out, o_off, o_len, max_spans=spans + nb, max_entries=mc)
                line.update({"round_trip_ok": int((dst != 0).sum()) == 0 and torch.equal(back.view(nb, n), want),
                             "new_pos_equals_the_walks": torch.equal(walked.pos, new_ix.pos[:mc])})
                del want, walked
                if base is None:
                    # what the caller does today: decode every stream, encode every stream (the patch itself is not even counted)
                    def today():
                        cd.frame_decode_buffers(framed, f_off, f_len, back, in_off, in_len, max_chunks=mc, max_spans=spans + nb, work=dwork)
                        cd.frame_encode_seekable(back, in_off, in_len, cb, out=out, out_off=f_off, out_cap=f_cap, max_chunks=mc, work=ework)

                    base = timed(today, a.reps)
                    arena = framed[:int(f_off[-1].item()) + int(f_len[-1].item())]

                    def copy():
                        out[:arena.numel()].copy_(arena)

                    floor = timed(copy, a.reps)
                    emit({"what": "frame_decode_buffers + frame_encode_seekable of every stream (what a caller does today)", **common, **rec_ms(*base)})
                    emit({"what": "plain device copy of the framed arena (the floor of the emit's verbatim copy)", **common, "bytes": arena.numel(),
                          **rec_ms(*floor), "GBps": round(arena.numel() / floor[0] / 1e6, 1)})
                spread = max(base[1]) - min(base[1])
                line.update({"decode_plus_encode_ms": round(base[0], 3), "decode_plus_encode_spread_ms": round(spread, 3), "speedup": round(base[0] / med, 2),
                             "faster_than_decode_plus_encode_by_more_than_its_spread": med < base[0] - spread})
                del back, dwork
            emit(line)
            del work, got
            torch.cuda.empty_cache()
        del framed, ework, out, index
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "a") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()

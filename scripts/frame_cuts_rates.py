"""Content-defined chunking rates (libsnappier_hip_frame_cuts.so): html-like data (snappier_amd/datagen.py) on the seekable line's two shapes --
10 GiB as 160 buffers of 64 MiB and as 163 840 buffers of 64 KiB.  Everything here is reported, nothing is gated.

  * finder: snp_content_cuts_batch at (window, max_bytes) = (2048, 16384) beside the CRC-32C kernel (snp_crc32c_batch) over the same bytes, in
    the same process, interleaved -- both read every byte once or a few times and write next to nothing;
  * encode: BlockCodec.frame_encode_content_defined at (2048, 16384) beside BlockCodec.frame_encode_seekable at 4096-byte chunks, interleaved,
    with the output sizes of both;
  * diff: BlockCodec.frame_diff_indexed with DIFF_PREFIX | DIFF_SUFFIX, every stream whole, between the batch and a re-encode FROM SCRATCH of
    the same buffers with 37 bytes inserted at 1/3 of each -- both sides on the 4096 grid, and both content-defined.  On the grid the two sides
    share no cut behind the insert, so the suffix direction decodes; content-defined they fall back into step.  (--diff-streams bounds the
    streams of this part: the grid pair decodes two thirds of both sides into scratch.)

ms from HIP events around each call (median of --reps after one warm-up); bounds, workspaces and outputs are sized before the timing where the
call allows it.  One JSON line per measurement, appended to --out as it is made.

    python scripts/frame_cuts_rates.py --out profiles/r23a_frame_cuts_rates.jsonl
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
from frame_splice_rates import timed  # noqa: E402

MIB = 1 << 20
CB, W, MX, INS = 4096, 2048, 16384, 37
SHAPES = {"64m": (TOTAL >> 26, 64 * MIB), "64k": (TOTAL // B, B)}                   # name -> (buffers, bytes of each)


def gbps(nbytes, ms):
    return round(nbytes / ms / 1e6, 2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="64m,64k")
    ap.add_argument("--parts", default="finder,encode,diff")
    ap.add_argument("--diff-streams", type=int, default=None, help="streams of the diff part (default: the whole shape)")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    html = open(os.path.join(ROOT, "tests", "golden", "testdata", "html"), "rb").read()
    raw = SD.html_like_blocks(html, 0, TOTAL // B, "cuda")
    cd = SB.BlockCodec(0, N.HASH_CRC32C)
    cd.ctx.reserve_compress(TOTAL // B)
    CL = N.frame_cuts_lib()

    def emit(rec):
        rec["where"] = torch.cuda.get_device_name(0)
        print(json.dumps(rec), flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(json.dumps(rec) + "\n")

    for shape in a.shapes.split(","):
        nb, n = SHAPES[shape]
        in_off, in_len = i64(np.arange(nb) * n), i64(np.full(nb, n))
        common = {"shape": shape, "buffers": nb, "buffer_bytes": n, "window": W, "max_bytes": MX}
        if "finder" in a.parts:
            max_cuts = nb * (n // (W + 1) + n // MX)
            work = u8(CL.snp_content_cuts_workspace(nb, nb * n, W))
            len32 = torch.full((nb,), n, dtype=torch.int32, device="cuda")
            got = {}

            def find():
                got["r"] = cd.content_cuts(raw, in_off, in_len, W, MX, max_cuts=max_cuts, work=work, span_bytes=nb * n)

            def crc():
                got["c"] = cd.crc32c(raw, in_off, len32)

            res = timed([find, crc], a.reps)
            r = got["r"][3].cpu().tolist()
            emit({"what": "snp_content_cuts_batch", **common, **rec_ms(*res[0]), "gb_per_s": gbps(nb * n, res[0][0]), "result": r,
                  "mean_piece": round(nb * n / (r[1] + nb), 1), "max_cuts": max_cuts, "workspace_bytes": work.numel(),
                  "all_ok": int((got["r"][2] != 0).sum()) == 0})
            emit({"what": "snp_crc32c_batch over the same bytes (the memory-speed yardstick)", **common, **rec_ms(*res[1]),
                  "gb_per_s": gbps(nb * n, res[1][0]), "finder_over_crc": round(res[0][0] / res[1][0], 2)})
            del work, got
            torch.cuda.empty_cache()
        if "encode" in a.parts:
            got = {}
            mc = nb * ((n + CB - 1) // CB)
            cap = 10 + 8 * ((n + CB - 1) // CB) + n
            g_off, g_cap, g_out = i64(np.arange(nb) * cap), i64(np.full(nb, cap)), u8(nb * cap)
            g_work = u8(N.frame_chunked_lib().snp_frame_encode_chunked_workspace(nb, mc, CB))
            ccap = 10 + 8 * (n // (W + 1) + n // MX + 1) + n
            c_off, c_cap, c_out = i64(np.arange(nb) * ccap), i64(np.full(nb, ccap)), u8(nb * ccap)

            def grid():
                got["g"] = cd.frame_encode_seekable(raw, in_off, in_len, CB, out=g_out, out_off=g_off, out_cap=g_cap, max_chunks=mc, work=g_work)

            def defined():
                got["d"] = cd.frame_encode_content_defined(raw, in_off, in_len, W, MX, out=c_out, out_off=c_off, out_cap=c_cap)

            res = timed([defined, grid], a.reps)
            rd, rg = got["d"][4].cpu().tolist(), got["g"][4].cpu().tolist()
            emit({"what": "frame_encode_content_defined (finder + encode at cuts, workspaces allocated inside)", **common, **rec_ms(*res[0]),
                  "gb_per_s": gbps(nb * n, res[0][0]), "result": rd, "out_bytes": rd[1], "chunks": rd[2],
                  "all_ok": int((got["d"][3] != 0).sum()) == 0})
            emit({"what": "frame_encode_seekable at 4096-byte chunks", **common, "chunk_bytes": CB, **rec_ms(*res[1]), "gb_per_s": gbps(nb * n, res[1][0]),
                  "result": rg, "out_bytes": rg[1], "chunks": rg[2], "all_ok": int((got["g"][3] != 0).sum()) == 0,
                  "content_defined_over_grid_ms": round(res[0][0] / res[1][0], 2), "content_defined_over_grid_bytes": round(rd[1] / max(rg[1], 1), 4)})
            del got, g_out, g_work, c_out
            torch.cuda.empty_cache()
        if "diff" in a.parts:
            ns = min(nb, a.diff_streams or nb)
            x = raw[:ns * n].view(ns, n)
            at = n // 3
            ins = torch.randint(0, 256, (ns, INS), dtype=torch.uint8, device="cuda", generator=torch.Generator("cuda").manual_seed(7))
            raw2 = torch.cat([x[:, :at], ins, x[:, at:]], dim=1).contiguous().view(-1)
            off1, len1 = i64(np.arange(ns) * n), i64(np.full(ns, n))
            off2, len2 = i64(np.arange(ns) * (n + INS)), i64(np.full(ns, n + INS))
            rs = torch.arange(ns, dtype=torch.int32, device="cuda")
            zero, whole = i64(np.zeros(ns)), i64(np.full(ns, -1))
            flags = SB.DIFF_PREFIX | SB.DIFF_SUFFIX
            for kind in ("grid", "content-defined"):
                sides = []
                for data, off, ln in ((raw[:ns * n], off1, len1), (raw2, off2, len2)):
                    if kind == "grid":
                        e = cd.frame_encode_seekable(data, off, ln, CB)
                    else:
                        e = cd.frame_encode_content_defined(data, off, ln, W, MX)
                    torch.cuda.synchronize()
                    assert int((e[3] != 0).sum()) == 0
                    sides.append((e[0], e[1], e[2], e[5]))
                need = cd.frame_diff_indexed(sides[0], sides[1], rs, zero, whole, rs, zero, whole, flags)[5].cpu().tolist()   # the sizing rounds
                mr, sc = need[0], need[2]
                work = u8(N.frame_diff_lib().snp_frame_diff_indexed_workspace(ns, mr, sc))
                got = {}

                def diff():
                    got["r"] = cd.frame_diff_indexed(sides[0], sides[1], rs, zero, whole, rs, zero, whole, flags, mr, sc, work)

                res = timed([diff], a.reps)
                pre, suf, _, _, st, result = got["r"]
                emit({"what": "frame_diff_indexed, whole streams, against a re-encode with %d bytes inserted at 1/3" % INS, **common, "encoding": kind,
                      "streams": ns, **rec_ms(*res[0]), "gb_per_s": gbps(ns * n, res[0][0]), "max_rows": mr, "scratch_bytes": sc,
                      "workspace_bytes": work.numel(), "result": result.cpu().tolist(), "all_ok": int((st != 0).sum()) == 0,
                      # (an inserted byte may equal its neighbour: the prefix ends inside the insert, the two cover all but at most the insert)
                      "true_answer": bool((pre >= at).all()) and bool((pre <= at + INS).all()) and bool((pre + suf >= n - INS).all())})
                del sides, work, got
                torch.cuda.empty_cache()
            del raw2
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()

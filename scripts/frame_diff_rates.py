"""snp_frame_diff_indexed_batch rates: html-like data (snappier_amd/datagen.py) kept as seekable framed streams with 4096-byte chunks and their
index, on the seekable line's two shapes -- 10 GiB as 160 streams of 64 MiB and as 163 840 streams of 64 KiB -- every stream whole against:

  * a: an identical replica (the same arrays passed for both sides);
  * b: a replica kept at 65536-byte chunks (64m only);
  * c: the stream after ONE insert of 4 KiB at 3/4 of its length (snp_frame_splice_indexed_batch), the splice's benchmark case;
  * d: itself one byte on (off_b = off_a + 1): no common cut, everything is decoded -- a window of --ragged bytes per stream, what scratch
       allows (64m only);

each once more with SNP_DIFF_EXACT.  Beside each, interleaved in the same process, what a caller does without the call:
BlockCodec.frame_read_indexed of both windows into arenas sized beforehand, then a first and a last mismatch per stream in torch over the two
arenas (timed apart: the read, and the comparison).  After each case prefix and suffix are compared with that path's answer.  ms from HIP
events around each call (median of --reps after one warm-up); bounds, workspaces and outputs are sized before the timing, so all sides only
enqueue.  One JSON line per measurement to --out.

    python scripts/frame_diff_rates.py --out profiles/r20a_frame_diff_rates.jsonl
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
CB = 4096
SHAPES = {"64m": (TOTAL >> 26, 64 * MIB), "64k": (TOTAL // B, B)}                   # name -> (streams, decoded bytes of each)
CASES = {"64m": "a,b,c,d", "64k": "a,c"}


def encode(cd, raw, nb, n, cb):
    """nb streams of n bytes of raw at chunk size cb: -> (framed, in_off, in_len, index)."""
    in_off, in_len = i64(np.arange(nb) * n), i64(np.full(nb, n))
    mc = nb * ((n + cb - 1) // cb)
    cap = 10 + 8 * ((n + cb - 1) // cb) + n
    r_off, r_cap = i64(np.arange(nb) * cap), i64(np.full(nb, cap))
    arena = u8(nb * cap)
    work = u8(N.frame_chunked_lib().snp_frame_encode_chunked_workspace(nb, mc, cb))
    _, _, f_len, est, _, index = cd.frame_encode_seekable(raw, in_off, in_len, cb, out=arena, out_off=r_off, out_cap=r_cap, max_chunks=mc, work=work)
    torch.cuda.synchronize()
    assert int((est != 0).sum()) == 0
    return arena, r_off, f_len, index


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="64m,64k")
    ap.add_argument("--cases", default=None, help="default: a,b,c,d on 64m and a,c on 64k")
    ap.add_argument("--modes", default="headers,exact")
    ap.add_argument("--ragged", type=int, default=16 * MIB, help="window bytes per stream in case d")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--diff-only", action="store_true", help="the diff only, no comparison and no check (profiling runs)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    html = open(os.path.join(ROOT, "tests", "golden", "testdata", "html"), "rb").read()
    raw = SD.html_like_blocks(html, 0, TOTAL // B, "cuda")
    cd = SB.BlockCodec(0, N.HASH_CRC32C)
    cd.ctx.reserve_compress(TOTAL // B)
    DL, IL = N.frame_diff_lib(), N.frame_index_lib()
    lines = []

    def emit(rec):
        rec["where"] = torch.cuda.get_device_name(0)
        print(json.dumps(rec), flush=True)
        lines.append(rec)

    for shape in a.shapes.split(","):
        nb, n = SHAPES[shape]
        side_a = encode(cd, raw, nb, n, CB)
        rs = torch.arange(nb, dtype=torch.int32, device="cuda")
        for case in (a.cases or CASES[shape]).split(","):
            off_a, off_b, ln = 0, 0, -1
            if case == "a":
                side_b = side_a
            elif case == "b":
                side_b = encode(cd, raw, nb, n, B)
            elif case == "c":
                at = n // 4 * 3 + 100                                   # mid-chunk, as in the splice's benchmark
                src = raw[:nb * CB].clone()
                sp = cd.frame_splice_to_memory(*side_a, i64(np.full(nb, at)), i64(np.zeros(nb)), src, i64(np.arange(nb) * CB), i64(np.full(nb, CB)), CB)
                torch.cuda.synchronize()
                assert int((sp[3] != 0).sum()) == 0
                side_b = (sp[0], sp[1], sp[2], sp[4])
            else:
                side_b, off_b, ln = side_a, 1, a.ragged
            roa, rob, rl = i64(np.full(nb, off_a)), i64(np.full(nb, off_b)), i64(np.full(nb, ln))
            la = n if ln < 0 else min(ln, n)
            lb = (n + CB if case == "c" else n) if ln < 0 else min(ln, n - off_b)
            m = min(la, lb)
            for mode in a.modes.split(","):
                flags = SB.DIFF_PREFIX | SB.DIFF_SUFFIX | (SB.DIFF_EXACT if mode == "exact" else 0)
                need = cd.frame_diff_indexed(side_a, side_b, rs, roa, rl, rs, rob, rl, flags)[5].cpu().tolist()      # the two sizing rounds
                mr, sc = need[0], need[2]
                work = u8(DL.snp_frame_diff_indexed_workspace(nb, mr, sc))
                got, other = {}, {}

                def diff():
                    got["r"] = cd.frame_diff_indexed(side_a, side_b, rs, roa, rl, rs, rob, rl, flags, mr, sc, work)

                fns = [diff]
                if not a.diff_only:
                    stride = max(la, lb)
                    o_off = i64(np.arange(nb) * stride)
                    xs, ys = u8(nb * stride), u8(nb * stride)
                    ne = u8(nb * m)
                    reads = []
                    for side, ro, cap in ((side_a, roa, la), (side_b, rob, lb)):
                        o_cap = i64(np.full(nb, cap))
                        rneed = cd.frame_read_indexed(*side, rs, ro, rl, xs, o_off, o_cap, 0, 0)[2].cpu().tolist()
                        reads.append((side, ro, o_cap, rneed[0], rneed[2], u8(IL.snp_frame_read_indexed_workspace(nb, rneed[0], rneed[2]))))

                    def read_both():
                        for (side, ro, o_cap, rmc, rec, rwork), out in zip(reads, (xs, ys)):
                            other["read"] = cd.frame_read_indexed(*side, rs, ro, rl, out, o_off, o_cap, rmc, rec, work=rwork)

                    def compare():
                        x, y, d = xs.view(nb, stride), ys.view(nb, stride), ne.view(nb, m)
                        torch.ne(x[:, :m], y[:, :m], out=d.view(torch.bool))
                        hit, first = d.max(dim=1)                       # (the index of the first maximal value)
                        other["prefix"] = torch.where(hit > 0, first, torch.full_like(first, m))
                        torch.ne(x[:, la - m:la].flip(1), y[:, lb - m:lb].flip(1), out=d.view(torch.bool))
                        hit, first = d.max(dim=1)
                        other["suffix"] = torch.minimum(torch.where(hit > 0, first, torch.full_like(first, m)), m - other["prefix"])

                    fns += [read_both, compare]
                res = timed(fns, a.reps)
                pre, suf, len_a, len_b, st, result = got["r"]
                r = result.cpu().tolist()
                common = {"shape": shape, "case": case, "mode": mode, "streams": nb, "stream_bytes": n, "chunk_bytes": CB, "requests": nb,
                          "len_a": la, "len_b": lb, "max_rows": mr, "scratch_bytes": sc, "workspace_bytes": work.numel()}
                line = {"what": "snp_frame_diff_indexed_batch", **common, **rec_ms(*res[0]), "result": r, "all_ok": int((st != 0).sum()) == 0,
                        "prefix_min_max": [int(pre.min()), int(pre.max())], "suffix_min_max": [int(suf.min()), int(suf.max())]}
                if not a.diff_only:
                    line["equals_read_then_compare"] = bool(torch.equal(pre, other["prefix"])) and bool(torch.equal(suf, other["suffix"])) and \
                        int((other["read"][1] != 0).sum()) == 0
                    emit({"what": "frame_read_indexed of both windows (what a caller does without the call, 1 of 2)", **common, **rec_ms(*res[1])})
                    emit({"what": "torch first and last mismatch over the two arenas (what a caller does without the call, 2 of 2)", **common, **rec_ms(*res[2])})
                    both = res[1][0] + res[2][0]
                    line.update({"other_ms": round(both, 3), "other_over_diff": round(both / res[0][0], 2)})
                    del xs, ys, ne, reads
                emit(line)
                other.clear()
                got.clear()
                del work
                torch.cuda.empty_cache()
            if side_b is not side_a:
                del side_b
            torch.cuda.empty_cache()
        del side_a
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "a") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()

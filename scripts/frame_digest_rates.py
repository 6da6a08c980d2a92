"""snp_frame_digest_indexed_batch rates: html-like data (snappier_amd/datagen.py) kept as seekable framed streams with 4096-byte chunks and
their index, on the seekable line's two shapes -- 10 GiB as 160 streams of 64 MiB and as 163 840 streams of 64 KiB:

  * whole:   the digest of every stream whole (edge_cap = 0: nothing is decoded);
  * w1m_on:  one window of 1 MiB per stream from a chunk boundary (on the short shape it is clipped at the stream's end: 44 KiB, no cut chunk);
  * w1m_off: the same 777 bytes off the boundary: both ends cut a chunk (on the short shape the window is clipped: one cut chunk);
  * w4k:     one window of 4 KiB per stream, off the boundary: two cut chunks and nothing between.

Beside each, interleaved in the same process, what a caller does without the call: BlockCodec.frame_read_indexed of the same windows into
an arena sized beforehand, then BlockCodec.crc32c over what it read.  After each case the digests are compared with those CRCs.  ms from HIP
events around each call (median of --reps after one warm-up); bounds, workspaces and outputs are sized before the timing, so both sides
only enqueue.  One JSON line per measurement to --out.

    python scripts/frame_digest_rates.py --out profiles/r19a_frame_digest_rates.jsonl
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
CASES = {"whole": (0, -1), "w1m_on": (5 * CB, MIB), "w1m_off": (5 * CB + 777, MIB), "w4k": (9 * CB + 777, CB)}   # name -> (req_off, req_len)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="64m,64k")
    ap.add_argument("--cases", default="whole,w1m_on,w1m_off,w4k")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--digest-only", action="store_true", help="the digest only, no comparison and no check (profiling runs)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    html = open(os.path.join(ROOT, "tests", "golden", "testdata", "html"), "rb").read()
    raw = SD.html_like_blocks(html, 0, TOTAL // B, "cuda")
    cd = SB.BlockCodec(0, N.HASH_CRC32C)
    cd.ctx.reserve_compress(TOTAL // B)
    DL, CL, IL = N.frame_digest_lib(), N.frame_chunked_lib(), N.frame_index_lib()
    lines = []

    def emit(rec):
        rec["where"] = torch.cuda.get_device_name(0)
        print(json.dumps(rec), flush=True)
        lines.append(rec)

    for shape in a.shapes.split(","):
        nb, n = SHAPES[shape]
        in_off, in_len = i64(np.arange(nb) * n), i64(np.full(nb, n))
        mc = nb * ((n + CB - 1) // CB)
        cap = 10 + 8 * ((n + CB - 1) // CB) + n
        r_off, r_cap = i64(np.arange(nb) * cap), i64(np.full(nb, cap))
        arena = u8(nb * cap)
        ework = u8(CL.snp_frame_encode_chunked_workspace(nb, mc, CB))
        _, _, f_len, est, _, index = cd.frame_encode_seekable(raw, in_off, in_len, CB, out=arena, out_off=r_off, out_cap=r_cap, max_chunks=mc, work=ework)
        torch.cuda.synchronize()
        assert int((est != 0).sum()) == 0
        del ework
        rs = torch.arange(nb, dtype=torch.int32, device="cuda")
        for case in a.cases.split(","):
            off, ln = CASES[case]
            ro, rl = i64(np.full(nb, off)), i64(np.full(nb, ln))
            lo, hi = min(off, n), (n if ln < 0 else min(off + ln, n))
            need = cd.frame_digest_indexed(arena, r_off, f_len, index, rs, ro, rl, edge_cap=0)[3].cpu().tolist()
            ec = need[2]
            work = u8(DL.snp_frame_digest_indexed_workspace(nb, ec))
            got, other = {}, {}

            def digest():
                got["r"] = cd.frame_digest_indexed(arena, r_off, f_len, index, rs, ro, rl, edge_cap=ec, work=work)

            fns = [digest]
            if not a.digest_only:
                o_cap = i64(np.full(nb, hi - lo))
                o_off = i64(np.arange(nb) * (hi - lo))
                out = u8(nb * (hi - lo))
                rneed = cd.frame_read_indexed(arena, r_off, f_len, index, rs, ro, rl, out, o_off, o_cap, 0, 0)[2].cpu().tolist()
                rmc, rec = rneed[0], rneed[2]
                rwork = u8(IL.snp_frame_read_indexed_workspace(nb, rmc, rec))
                o_len32 = torch.full((nb,), hi - lo, dtype=torch.int32, device="cuda")

                def today():
                    other["read"] = cd.frame_read_indexed(arena, r_off, f_len, index, rs, ro, rl, out, o_off, o_cap, rmc, rec, work=rwork)
                    other["crc"] = cd.crc32c(out, o_off, o_len32)

                fns.append(today)
            res = timed(fns, a.reps)
            digest_t, dig_len, st, result = got["r"]
            r = result.cpu().tolist()
            common = {"shape": shape, "case": case, "streams": nb, "stream_bytes": n, "chunk_bytes": CB, "requests": nb, "window": [lo, hi],
                      "decoded_bytes": nb * (hi - lo), "edge_bytes": ec, "workspace_bytes": work.numel()}
            line = {"what": "snp_frame_digest_indexed_batch", **common, **rec_ms(*res[0]), "result": r, "all_ok": int((st != 0).sum()) == 0,
                    "digested_GBps": round(r[1] / res[0][0] / 1e6, 2), "rows_per_us": round(r[0] / res[0][0] / 1e3, 2)}
            if not a.digest_only:
                rlen, rst, _ = other["read"]
                line["equals_read_then_crc"] = bool(torch.equal(digest_t, other["crc"])) and bool(torch.equal(dig_len, rlen)) and int((rst != 0).sum()) == 0
                emit({"what": "frame_read_indexed of the windows + crc32c over the output (what a caller does without the call)", **common,
                      "read_slots": rmc, "read_workspace_bytes": rwork.numel(), **rec_ms(*res[1])})
                line.update({"other_ms": round(res[1][0], 3), "other_spread_ms": round(max(res[1][1]) - min(res[1][1]), 3),
                             "other_over_digest": round(res[1][0] / res[0][0], 2)})
                del out, rwork
            emit(line)
            other.clear()
            got.clear()
            del work
            torch.cuda.empty_cache()
        del arena, index
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "a") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()

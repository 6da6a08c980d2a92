"""snp_frame_find_indexed_batch rates: html-like data (snappier_amd/datagen.py) kept as seekable framed streams with their index, on the seekable
line's two shapes -- 10 GiB as 160 streams of 64 MiB and as 163 840 streams of 64 KiB -- at 4096- and 65536-byte chunks, every stream whole,
one request per stream, for needles of 1, 8 and 64 bytes with few hits (0xff bytes, which the data all but lacks) and with many (`\\n`, and
pieces of the corpus that every block repeats), and for the 1-byte needle ` ` (dense: half a billion hits).  Per case, interleaved in the same process:

  * a: the find call, with room for --hit-cap hits per request;
  * b: BlockCodec.frame_read_indexed of the same windows into an arena sized beforehand: the decode the call cannot do without;
  * d2 (1-byte needles): (arena == c).nonzero() over the arena that b filled, 1 GiB at a time: torch's only search, a mask as large as
       what it looks at;

and once per shape and chunk size, d1: what a caller has today -- the arena of b copied to the host and bytes.find in a loop, the loop over
the first --host-bytes of it and scaled to the whole (10 GiB of bytes.find with many hits takes minutes).  After each case the counts are
compared with a count of the arena in torch (1-byte needles) or with bytes.find over the first stream (longer ones).  ms from HIP events around
each call (median of --reps after one warm-up); bounds, workspaces and outputs are sized before the timing, so all sides only enqueue.
One JSON line per measurement to --out.

c, the search kernels alone: the call has no entry point that skips the decode, so their time comes from a run of its own under
`rocprofv3 --kernel-trace --stats` with --find-only (one sizing call, one warm-up and --reps calls of ONE case); --kernel-stats reads that
run's CSV and writes the rates of k_fd_search<false> (count) and k_fd_search<true> (emit) over --bytes decoded bytes.

    python scripts/frame_find_rates.py --out profiles/r21a_frame_find_rates.jsonl
"""
import argparse
import csv
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
from compress_buffers_rates import B, TOTAL  # noqa: E402
from frame_chunked_rates import i64, rec_ms, u8  # noqa: E402
from frame_diff_rates import encode  # noqa: E402
from frame_splice_rates import timed  # noqa: E402

MIB = 1 << 20
SHAPES = {"64m": (TOTAL >> 26, 64 * MIB), "64k": (TOTAL // B, B)}                   # name -> (streams, decoded bytes of each)


def kernel_stats(path, nbytes, calls, out):
    """The c rows from a rocprofv3 kernel-stats CSV of a --find-only run."""
    lines = []
    with open(path) as f:
        rows = list(csv.DictReader(x for x in f if not x.startswith("#")))
    for row in rows:
        low = {k.lower(): v for k, v in row.items()}
        name = low.get("name") or low.get("kernel") or ""
        if "k_fd_search" not in name:
            continue
        total = float(low.get("totaldurationns") or low.get("total_ns"))
        per_call = total / calls
        lines.append({"what": "c: search kernel alone (rocprofv3 --kernel-trace --stats, a run of its own)", "kernel": name, "launches": int(low["calls"]),
                      "find_calls_with_tiles": calls, "total_ns": total, "ms_per_call": round(per_call / 1e6, 3), "bytes": nbytes,
                      "GBps": round(nbytes / per_call, 1)})
    for rec in lines:
        print(json.dumps(rec), flush=True)
    if out:
        with open(out, "a") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="64m,64k")
    ap.add_argument("--chunks", default="4096,65536")
    ap.add_argument("--needles", default="1,8,64")
    ap.add_argument("--hits", default="few,many,dense")
    ap.add_argument("--hit-cap", type=int, default=None, help="hits kept per request (default: 2^22 per 64 MiB stream, 4096 per 64 KiB stream)")
    ap.add_argument("--host-bytes", type=int, default=256 * MIB)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--find-only", action="store_true", help="the find only, no comparison and no check (profiling runs)")
    ap.add_argument("--kernel-stats", default=None, help="a rocprofv3 kernel-stats CSV of a --find-only run: write the c rows and stop")
    ap.add_argument("--bytes", type=int, default=TOTAL)
    ap.add_argument("--calls", type=int, default=None, help="find calls with tiles in that run (warm-up + reps)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.kernel_stats:
        return kernel_stats(a.kernel_stats, a.bytes, a.calls or a.reps + 1, a.out)
    html = open(os.path.join(ROOT, "tests", "golden", "testdata", "html"), "rb").read()
    raw = SD.html_like_blocks(html, 0, TOTAL // B, "cuda")
    cd = SB.BlockCodec(0, N.HASH_CRC32C)
    cd.ctx.reserve_compress(TOTAL // B)
    FL, IL = N.frame_find_lib(), N.frame_index_lib()
    lines = []
    first = bytes(raw[:B].cpu().numpy())
    # many hits: the delimiter, and pieces every block of the corpus repeats; few: bytes the corpus does not hold
    common = max((first[p:p + 64] for p in range(0, 4096, 64)), key=lambda s: len(first.split(s)))
    needles = {("few", m): b"\xff" * m for m in (1, 8, 64)}
    needles.update({("many", 1): b"\n", ("many", 8): common[:8], ("many", 64): common, ("dense", 1): b" "})

    def emit(rec):
        rec["where"] = torch.cuda.get_device_name(0)
        print(json.dumps(rec), flush=True)
        lines.append(rec)

    for shape in a.shapes.split(","):
        nb, n = SHAPES[shape]
        cap = a.hit_cap if a.hit_cap is not None else (1 << 22 if shape == "64m" else 4096)
        rs = torch.arange(nb, dtype=torch.int32, device="cuda")
        ro, rl = i64(np.zeros(nb)), i64(np.full(nb, -1))
        for cb in [int(x) for x in a.chunks.split(",")]:
            side = encode(cd, raw, nb, n, cb)
            arena, o_off, o_cap = (None, None, None) if a.find_only else (u8(nb * n), i64(np.arange(nb) * n), i64(np.full(nb, n)))
            if not a.find_only:
                rneed = cd.frame_read_indexed(*side, rs, ro, rl, arena, o_off, o_cap, 0, 0)[2].cpu().tolist()
                rwork = u8(IL.snp_frame_read_indexed_workspace(nb, rneed[0], rneed[2]))
            host_done = False
            for kind in a.hits.split(","):
                for m in [int(x) for x in a.needles.split(",")]:
                    if (kind, m) not in needles:
                        continue
                    needle = needles[(kind, m)]
                    nd = cd._needle_tensors(needle, nb)
                    need = cd.frame_find_indexed_result(*side, rs, ro, rl, nd, cap, 0, 0)[6].cpu().tolist()          # the one sizing round
                    mr, sc = need[0], need[2]
                    work = u8(FL.snp_frame_find_indexed_workspace(nb, mr, sc))
                    got, other = {}, {}

                    def find():
                        got["r"] = cd.frame_find_indexed_result(*side, rs, ro, rl, nd, cap, mr, sc, work)

                    fns = [find]
                    if not a.find_only:
                        def read():
                            other["read"] = cd.frame_read_indexed(*side, rs, ro, rl, arena, o_off, o_cap, rneed[0], rneed[2], work=rwork)

                        fns.append(read)
                        if m == 1:
                            def nonzero():
                                # (1 GiB at a time: nonzero() of more than 2^31 elements is not supported)
                                other["nz"] = torch.cat([(arena[at:at + (1 << 30)] == needle[0]).nonzero() + at for at in range(0, arena.numel(), 1 << 30)])

                            fns.append(nonzero)
                    res = timed(fns, a.reps)
                    st, wl, cnt, nh, hits, hit_off, result = got["r"]
                    r = result.cpu().tolist()
                    base = {"shape": shape, "streams": nb, "stream_bytes": n, "chunk_bytes": cb, "requests": nb, "needle_bytes": m, "hits": kind,
                            "needle": needle.hex(), "hit_cap": cap, "max_rows": mr, "scratch_bytes": sc, "workspace_bytes": work.numel()}
                    line = {"what": "a: snp_frame_find_indexed_batch", **base, **rec_ms(*res[0]), "result": r, "all_ok": int((st != 0).sum()) == 0,
                            "GBps": round(nb * n / res[0][0] / 1e6, 1), "count": r[1], "hits_kept": int(nh.sum())}
                    if not a.find_only:
                        torch.cuda.synchronize()
                        if m == 1:
                            line["equals_torch_count"] = int((arena == needle[0]).sum()) == r[1]
                        else:
                            s0 = bytes(arena[:n].cpu().numpy())             # stream 0, by bytes.find in a loop
                            found, p = 0, s0.find(needle)
                            while p >= 0:
                                found += 1
                                p = s0.find(needle, p + 1)
                            line["equals_bytes_find_on_stream_0"] = found == int(cnt[0])
                        emit({"what": "b: frame_read_indexed of the same windows (the decode floor)", **base, **rec_ms(*res[1]),
                              "GBps": round(nb * n / res[1][0] / 1e6, 1)})
                        line.update({"read_ms": round(res[1][0], 3), "find_over_read": round(res[0][0] / res[1][0], 3)})
                        if m == 1:
                            emit({"what": "d2: (arena == c).nonzero() over the arena b filled (without the read)", **base, **rec_ms(*res[2]),
                                  "positions": int(other["nz"].shape[0])})
                            line["read_plus_nonzero_over_find"] = round((res[1][0] + res[2][0]) / res[0][0], 2)
                        if not host_done:                               # d1, once per shape and chunk size
                            host_done = True
                            t0 = time.perf_counter()
                            host = arena.cpu()
                            t1 = time.perf_counter()
                            piece = bytes(host[:a.host_bytes].numpy())
                            t2 = time.perf_counter()
                            found, p = 0, piece.find(needle)
                            while p >= 0:
                                found += 1
                                p = piece.find(needle, p + 1)
                            t3 = time.perf_counter()
                            scale = nb * n / len(piece)
                            emit({"what": "d1: the arena of b copied to the host, then bytes.find in a loop (loop over host_bytes, scaled to all)", **base,
                                  "copy_ms": round((t1 - t0) * 1e3, 1), "host_bytes": len(piece), "find_loop_ms_on_host_bytes": round((t3 - t2) * 1e3, 1),
                                  "found_in_host_bytes": found, "find_loop_ms_scaled": round((t3 - t2) * 1e3 * scale, 1),
                                  "total_ms_with_read": round(res[1][0] + (t1 - t0) * 1e3 + (t3 - t2) * 1e3 * scale, 1)})
                            del host, piece
                    emit(line)
                    other.clear()
                    got.clear()
                    del work
                    torch.cuda.empty_cache()
            del side, arena
            torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "a") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()

"""snp_frame_compose_indexed_batch rates: html-like data (snappier_amd/datagen.py) kept as seekable framed streams with their index, composed
into new streams out of place:

  * join:   10 GiB as 160 streams of 64 MiB at 65536-byte chunks, joined pairwise into 80 streams: every chunk is copied, nothing is decoded;
  * split:  each of the 160 split at 3/4 + 1000 bytes into two outputs: two chunks per source are cut, the rest is copied;
  * window: a 1 MiB window off the grid of each of the 160, as a stream of its own;
  * join16: 163 840 streams of 64 KiB at 4096-byte chunks joined 16 at a time: copy only;
  * cut16:  the same with every window cut mid-chunk on both sides (100 bytes off each end of every source).

Beside each, interleaved in the same process, what a caller does without the call: BlockCodec.frame_read_to_memory of the windows (one call
per window of a source), then BlockCodec.frame_encode_seekable of what it read (with their synchronising size reads).  After each case the
call's outputs are compared with that path's, byte for byte and length for length -- directly where the segments lie on the grid, after a
rechunk (BlockCodec.frame_rechunk_to_memory) of the call's outputs where they do not.  ms from HIP events around each call (median of --reps
after one warm-up).  One JSON line per measurement to --out.

    python scripts/frame_compose_rates.py --out profiles/r18a_frame_compose_rates.jsonl
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
# name -> (sources, decoded bytes of each, chunk_bytes, the windows of source b as (offset, length) in the order of the outputs' segments,
#          sources per output or None when every window is an output of its own, the outputs are the chunked encoder's as they are)
CASES = {
    "join": (TOTAL >> 26, 64 * MIB, 65536, [(0, 64 * MIB)], 2, True),
    "split": (TOTAL >> 26, 64 * MIB, 65536, [(0, 48 * MIB + 1000), (48 * MIB + 1000, 16 * MIB - 1000)], None, False),
    "window": (TOTAL >> 26, 64 * MIB, 65536, [(5 * MIB + 777, MIB)], None, False),
    "join16": (TOTAL // B, B, 4096, [(0, B)], 16, True),
    "cut16": (TOTAL // B, B, 4096, [(100, B - 200)], 16, False),
}


def dense(buf, off, lens, step=256 * MIB):
    """The bytes [off[j], off[j] + lens[j]) of every j, one behind the other, in pieces of about `step` bytes."""
    ends = torch.cumsum(lens, 0)
    total, j0 = int(ends[-1].item()) if lens.numel() else 0, 0
    while j0 < lens.numel():
        base = int(ends[j0 - 1].item()) if j0 else 0
        j1 = max(int(torch.searchsorted(ends, torch.tensor([base + step], device="cuda")).item()), j0 + 1)
        n = lens[j0:j1]
        begin = torch.cumsum(n, 0) - n
        idx = torch.repeat_interleave(off[j0:j1] - begin, n) + torch.arange(int(n.sum().item()), device="cuda")
        yield buf[idx]
        j0 = j1
    assert total >= 0


def same_bytes(x, x_off, y, y_off, lens):
    return all(bool(torch.equal(a, b)) for a, b in zip(dense(x, x_off, lens), dense(y, y_off, lens)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="join,split,window,join16,cut16")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--compose-only", action="store_true", help="the compose only, no comparison and no check (profiling runs)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    html = open(os.path.join(ROOT, "tests", "golden", "testdata", "html"), "rb").read()
    raw = SD.html_like_blocks(html, 0, TOTAL // B, "cuda")
    cd = SB.BlockCodec(0, N.HASH_CRC32C)
    cd.ctx.reserve_compress(TOTAL // B)
    PL, CL = N.frame_compose_lib(), N.frame_chunked_lib()
    lines = []

    def emit(rec):
        rec["where"] = torch.cuda.get_device_name(0)
        print(json.dumps(rec), flush=True)
        lines.append(rec)

    for case in a.cases.split(","):
        nb, n, cb, windows, per, on_grid = CASES[case]
        in_off, in_len = i64(np.arange(nb) * n), i64(np.full(nb, n))
        mc = nb * ((n + cb - 1) // cb)
        cap = 10 + 8 * ((n + cb - 1) // cb) + n
        r_off, r_cap = i64(np.arange(nb) * cap), i64(np.full(nb, cap))
        arena = u8(nb * cap)
        ework = u8(CL.snp_frame_encode_chunked_workspace(nb, mc, cb))
        _, _, f_len, est, _, index = cd.frame_encode_seekable(raw, in_off, in_len, cb, out=arena, out_off=r_off, out_cap=r_cap, max_chunks=mc, work=ework)
        torch.cuda.synchronize()
        assert int((est != 0).sum()) == 0
        del ework
        # the segment list: window w of source b is segment w * nb + b when every window is an output, else segment b (one window per source)
        nw = len(windows)
        src = torch.arange(nb, dtype=torch.int32, device="cuda").repeat(nw)
        seg_off = torch.cat([i64(np.full(nb, w[0])) for w in windows])
        seg_len = torch.cat([i64(np.full(nb, w[1])) for w in windows])
        nsegs = nb * nw
        group = per or 1
        nout = nsegs // group
        seg_first = i64(np.arange(nout + 1) * group)
        need, bound = [cd.frame_compose_indexed(arena, r_off, f_len, index, cb, u8(0), i64(np.zeros(nout)), i64(np.zeros(nout)), 0, 0, 0, seg_first,
                                                src, seg_off, seg_len, with_bound=True)[k] for k in (3, 4)]
        need = need.cpu().tolist()
        ms, sc, me = need[0], need[2], max(need[4], 1)
        o_off = torch.cumsum(bound, 0) - bound
        out = u8(int(bound.sum().item()))
        work = u8(PL.snp_frame_compose_indexed_workspace(nb, nout, nsegs, ms, sc, cb, me))
        got, other = {}, {}

        def compose():
            got["r"] = cd.frame_compose_indexed(arena, r_off, f_len, index, cb, out, o_off, bound, ms, sc, me, seg_first, src, seg_off, seg_len, work=work)

        def today():
            # one read per window of a source; the windows of an output lie one behind the other in what the read returns
            other["e"] = []
            for w in windows:
                dec, d_off, d_len, dst = cd.frame_read_to_memory(arena, r_off, f_len, i64(np.full(nb, w[0])), i64(np.full(nb, w[1])))
                b_off, b_len = d_off.view(-1, group)[:, 0].contiguous(), d_len.view(-1, group).sum(1)
                other["e"].append((cd.frame_encode_seekable(dec, b_off, b_len, cb), dst))

        common = {"case": case, "sources": nb, "outputs": nout, "segments": nsegs, "chunk_bytes": cb, "source_bytes": nb * n,
                  "decoded_bytes": int(seg_len.sum().item()), "slots": ms, "staging_bytes": sc, "index_rows": me, "workspace_bytes": work.numel()}
        res = timed([compose] if a.compose_only else [compose, today], a.reps)
        out_len, st, new_ix, result = got["r"]
        r = result.cpu().tolist()
        line = {"what": "snp_frame_compose_indexed_batch", **common, **rec_ms(*res[0]), "result": r, "all_ok": int((st != 0).sum()) == 0,
                "written_GBps": round(r[1] / res[0][0] / 1e6, 2), "kept_fraction_of_chunks": round(r[5] / max(r[4], 1), 4)}
        if not a.compose_only:
            fin, fin_off, fin_len = out, o_off, out_len
            alone = torch.ones_like(out_len, dtype=torch.bool)
            if not on_grid:                                             # claim (b): after a rechunk the outputs are the chunked encoder's
                used = int(new_ix.first[-1].item())
                new_ix.start, new_ix.pos = new_ix.start[:used], new_ix.pos[:used]
                fin, fin_off, fin_len, rst, _ = cd.frame_rechunk_to_memory(out, o_off, out_len, new_ix, cb)
                assert int((rst != 0).sum()) == 0
                alone = fin_len == 0                                    # canonical already: the compose's own bytes
            e_out = [e[0][0] for e in other["e"]]
            e_off = torch.cat([e[0][1] for e in other["e"]])
            e_len = torch.cat([e[0][2] for e in other["e"]])
            ok = all(int((e[0][3] != 0).sum()) == 0 and int((e[1] != 0).sum()) == 0 for e in other["e"])
            per_read = nout // nw
            zero = torch.zeros_like(out_len)
            ok = ok and bool(torch.equal(torch.where(alone, out_len, fin_len), e_len))
            for k, eb in enumerate(e_out):
                rows = slice(k * per_read, (k + 1) * per_read)
                ok = ok and same_bytes(out, o_off[rows], eb, e_off[rows], torch.where(alone, out_len, zero)[rows])
                ok = ok and same_bytes(fin, fin_off[rows], eb, e_off[rows], torch.where(alone, zero, fin_len)[rows])
            line["equals_read_then_encode" if on_grid else "equals_read_then_encode_after_a_rechunk"] = ok
            emit({"what": "frame_read_to_memory of the windows + frame_encode_seekable (what a caller does without the call)", **common, **rec_ms(*res[1])})
            line.update({"other_ms": round(res[1][0], 3), "other_spread_ms": round(max(res[1][1]) - min(res[1][1]), 3),
                         "other_over_compose": round(res[1][0] / res[0][0], 2)})
        emit(line)
        other.clear()
        got.clear()
        del arena, out, work, index
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "a") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()

"""snp_frame_rechunk_indexed_batch rates: html-like data (snappier_amd/datagen.py) kept as seekable framed streams with their index, brought to
canonical form out of place:

  * 1: 10 GiB as 160 streams of 64 MiB at 65536-byte chunks, after ONE 4 KiB insert (snp_frame_splice_indexed_batch) at 3/4 of each stream: the
       chunks before the insert are clean and copied, the quarter behind it is off the grid and rebuilt;
  * 2: the same streams with the insert at offset 0: every chunk is off the grid, everything is rebuilt;
  * 3: 163 840 streams of 64 KiB from 4096-byte chunks to 65536-byte chunks, and back;
  * 4: the streams of 1 before the insert: canonical already, the plan alone.

Beside each of 1 .. 3, interleaved in the same process, what a caller does without the call: BlockCodec.frame_decode_to_memory of every stream,
then BlockCodec.frame_encode_seekable of what it decoded (two calls, with their synchronising size reads).  After each case the call's output
is compared with that path's, byte for byte and length for length, and the new index with the encoder's.  ms from HIP events around each call
(median of --reps after one warm-up).  One JSON line per measurement to --out.

    python scripts/frame_rechunk_rates.py --out profiles/r17a_frame_rechunk_rates.jsonl
    rocprofv3 --kernel-trace --stats -d DIR -o run -- python scripts/frame_rechunk_rates.py --cases 2 --reps 2 --rechunk-only
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

# name -> (streams, decoded bytes of each, chunk_bytes the streams are written with, chunk_bytes of the rechunk, offset of a 4 KiB insert or None)
CASES = {"1": (TOTAL >> 26, 64 << 20, 65536, 65536, 48 << 20), "2": (TOTAL >> 26, 64 << 20, 65536, 65536, 0),
         "3up": (TOTAL // B, B, 4096, 65536, None), "3down": (TOTAL // B, B, 65536, 4096, None), "4": (TOTAL >> 26, 64 << 20, 65536, 65536, None)}
INS = 4096


def same_streams(x, y, lens, nb, cap):
    """The first lens[b] bytes of slot b (cap bytes each) of x and of y are equal, for every b; in slices of at most 1 GiB."""
    step = max((1 << 30) // cap, 1)
    col = torch.arange(cap, device="cuda")
    for b0 in range(0, nb, step):
        b1 = min(b0 + step, nb)
        live = col[None, :] < lens[b0:b1, None]
        if not bool(((x[b0 * cap:b1 * cap].view(b1 - b0, cap) == y[b0 * cap:b1 * cap].view(b1 - b0, cap)) | ~live).all()):
            return False
    return True


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="1,2,3up,3down,4")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rechunk-only", action="store_true", help="the rechunk only, no comparison and no check (profiling runs)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    html = open(os.path.join(ROOT, "tests", "golden", "testdata", "html"), "rb").read()
    raw = SD.html_like_blocks(html, 0, TOTAL // B, "cuda")
    cd = SB.BlockCodec(0, N.HASH_CRC32C)
    cd.ctx.reserve_compress(TOTAL // B)
    RL, CL = N.frame_rechunk_lib(), N.frame_chunked_lib()
    lines = []

    def emit(rec):
        rec["where"] = torch.cuda.get_device_name(0)
        print(json.dumps(rec), flush=True)
        lines.append(rec)

    for case in a.cases.split(","):
        nb, n, cb0, cb, ins_at = CASES[case]
        m = n + (INS if ins_at is not None else 0)                     # what a stream decodes to when it is rechunked
        small = min(cb0, cb)
        stride = (n + B - 1) // B * B                                   # where stream b's bytes start in the generated data
        in_off, in_len = i64(np.arange(nb) * stride), i64(np.full(nb, n))
        mc = nb * ((n + cb0 - 1) // cb0)
        cap = 10 + 8 * ((m + small - 1) // small + 2) + m               # room for any of the streams however it compresses
        r_off, r_cap = i64(np.arange(nb) * cap), i64(np.full(nb, cap))
        arena = u8(nb * cap)
        ework = u8(CL.snp_frame_encode_chunked_workspace(nb, mc, cb0))
        _, _, f_len, est, eres, index = cd.frame_encode_seekable(raw, in_off, in_len, cb0, out=arena, out_off=r_off, out_cap=r_cap, max_chunks=mc, work=ework)
        torch.cuda.synchronize()
        assert int((est != 0).sum()) == 0
        del ework
        if ins_at is not None:
            # one insert per stream: the bytes of the neighbouring stream; the spliced streams and their index are what the rechunk takes
            rawv = raw[:nb * stride].view(nb, stride)
            src = rawv[torch.roll(torch.arange(nb, device="cuda"), 1), 777:777 + INS].contiguous().view(-1)
            s_off, s_len = i64(np.arange(nb) * INS), i64(np.full(nb, INS))
            sp_off, sp_del = i64(np.full(nb, ins_at)), i64(np.zeros(nb))
            spliced = u8(nb * cap)
            need = cd.frame_splice_indexed(arena, r_off, f_len, index, sp_off, sp_del, src, s_off, s_len, cb0, spliced, r_off, r_cap, 0, 0)[3].cpu().tolist()
            f_len, sst, index, _ = cd.frame_splice_indexed(arena, r_off, f_len, index, sp_off, sp_del, src, s_off, s_len, cb0, spliced, r_off, r_cap,
                                                           need[0], need[2])
            torch.cuda.synchronize()
            assert int((sst != 0).sum()) == 0
            arena = spliced
            del spliced, src, rawv
        out = u8(nb * cap)
        need = cd.frame_rechunk_indexed(arena, r_off, f_len, index, cb, out, r_off, r_cap, 0, 0, 0)[3].cpu().tolist()
        ms, sc, me = need[0], need[2], max(need[4], 1)
        work = u8(RL.snp_frame_rechunk_indexed_workspace(nb, ms, sc, cb, me))
        got = {}

        def rechunk():
            got["r"] = cd.frame_rechunk_indexed(arena, r_off, f_len, index, cb, out, r_off, r_cap, ms, sc, me, work=work)

        common = {"case": case, "streams": nb, "from_chunk_bytes": cb0, "chunk_bytes": cb, "decoded_bytes": nb * m, "framed_bytes": int(f_len.sum().item()),
                  "insert_at": ins_at, "slots": ms, "staging_bytes": sc, "index_rows": me, "workspace_bytes": work.numel()}
        fns = [rechunk]
        other = {}
        if not a.rechunk_only and case != "4":
            out2 = u8(nb * cap)

            def today():
                dec, d_off, d_len, dst = cd.frame_decode_to_memory(arena, r_off, f_len)
                other["e"] = cd.frame_encode_seekable(dec, d_off, d_len, cb, out=out2, out_off=r_off, out_cap=r_cap)
                other["dst"] = dst

            fns.append(today)
        res = timed(fns, a.reps)
        out_len, st, new_ix, result = got["r"]
        r = result.cpu().tolist()
        line = {"what": "snp_frame_rechunk_indexed_batch", **common, **rec_ms(*res[0]), "result": r, "all_ok": int((st != 0).sum()) == 0,
                "written_GBps": round(r[1] / res[0][0] / 1e6, 2), "kept_fraction_of_chunks": round(1 - ms / max(me, 1), 4)}
        if case == "4":
            line["all_left_alone"] = r[5] == nb and r[3] == 0 and int(out_len.sum().item()) == 0
        elif not a.rechunk_only:
            _, _, e_len, est, _, e_ix = other["e"]
            used = int(new_ix.first[-1].item())
            line["equals_decode_then_encode"] = int((est != 0).sum()) == 0 and int((other["dst"] != 0).sum()) == 0 and bool(torch.equal(e_len, out_len)) and \
                same_streams(out, out2, out_len, nb, cap)
            line["new_index_equals_the_encoders"] = bool(torch.equal(e_ix.first, new_ix.first) and torch.equal(e_ix.start[:used], new_ix.start[:used]) and
                                                         torch.equal(e_ix.pos[:used], new_ix.pos[:used]) and torch.equal(e_ix.total, new_ix.total) and
                                                         torch.equal(e_ix.tail, new_ix.tail))
            emit({"what": "frame_decode_to_memory + frame_encode_seekable of every stream (what a caller does without the call)", **common, **rec_ms(*res[1])})
            line.update({"other_ms": round(res[1][0], 3), "other_spread_ms": round(max(res[1][1]) - min(res[1][1]), 3),
                         "other_over_rechunk": round(res[1][0] / res[0][0], 2)})
            del out2
        emit(line)
        other.clear()
        del arena, out, work, index, got
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "a") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()

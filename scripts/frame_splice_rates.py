"""snp_frame_splice_indexed_batch rates: html-like data (snappier_amd/datagen.py) kept as seekable framed streams with their index, and ONE splice per
stream, out of place:

  * a: 10 GiB as 160 streams of 64 MiB at 65536-byte chunks, 4 KiB inserted mid-chunk in each -- beside it, interleaved in the same process, what a
       caller must do without the call: snp_frame_decode_buffers_batch of every stream, the edited buffer put together by device copies, and
       snp_frame_encode_chunked_batch of it; and snp_frame_write_indexed_batch writing 4 KiB at the same place of the same streams (both calls
       copy every stream, so their ratio says what the plan, the assembly and the row merge cost);
  * b: 163 840 streams of 64 KiB at 4096-byte chunks, 1000 bytes deleted mid-stream in each;
  * c: the streams of a truncated to half;
  * d: bulk -- 1 GiB inserted as 64 KiB into each of 16 384 streams of 96 KiB at 65536-byte chunks -- beside it, interleaved,
       snp_frame_encode_chunked_batch of the same inserted bytes alone.

After each case the new streams are decoded whole against the edited buffers and the new index is compared with snp_frame_index_batch over the
new streams.  ms from HIP events around each call (median of --reps after one warm-up).  One JSON line per measurement to --out.

    python scripts/frame_splice_rates.py --out profiles/r16a_frame_splice_rates.jsonl
    rocprofv3 --kernel-trace --stats -d DIR -o run -- python scripts/frame_splice_rates.py --cases d --reps 2 --splice-only
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
# name -> (streams, decoded bytes of each, chunk_bytes, off, del, ins)
CASES = {"a": (TOTAL >> 26, 64 << 20, 65536, (32 << 20) + 777, 0, 4096), "b": (TOTAL // B, B, 4096, 30000, 1000, 0),
         "c": (TOTAL >> 26, 64 << 20, 65536, 32 << 20, 32 << 20, 0), "d": (16384, B + B // 2, 65536, 40000, 0, B)}


def timed(fns, reps):
    """The calls of fns timed in turn, reps times each after one warm-up of all: -> [(median, all)]."""
    for fn in fns:
        fn()
    torch.cuda.synchronize()
    ms = [[] for _ in fns]
    for _ in range(reps):
        for k, fn in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            ms[k].append(a.elapsed_time(b))
    return [(float(np.median(m)), m) for m in ms]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="a,b,c,d")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--splice-only", action="store_true", help="the splice only, no comparison and no check (profiling runs)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    html = open(os.path.join(ROOT, "tests", "golden", "testdata", "html"), "rb").read()
    raw = SD.html_like_blocks(html, 0, TOTAL // B, "cuda")
    cd = SB.BlockCodec(0, N.HASH_CRC32C)
    cd.ctx.reserve_compress(TOTAL // B)
    PL, CL, FL, UL = N.frame_splice_lib(), N.frame_chunked_lib(), N.frame_buffers_lib(), N.frame_update_lib()
    lines = []

    def emit(rec):
        rec["where"] = torch.cuda.get_device_name(0)
        print(json.dumps(rec), flush=True)
        lines.append(rec)

    for case in a.cases.split(","):
        nb, n, cb, off, dele, ins = CASES[case]
        m = n - dele + ins                                              # what an edited stream decodes to
        stride = (n + B - 1) // B * B                                   # where stream b's bytes start in the generated data
        in_off, in_len = i64(np.arange(nb) * stride), i64(np.full(nb, n))
        mc = nb * ((n + cb - 1) // cb)
        cap = 10 + 8 * ((max(n, m) + cb - 1) // cb + 2) + max(n, m)     # room for either stream however it compresses
        r_off, r_cap = i64(np.arange(nb) * cap), i64(np.full(nb, cap))
        arena = u8(nb * cap)
        ework = u8(CL.snp_frame_encode_chunked_workspace(nb, mc, cb))
        _, _, f_len, est, eres, index = cd.frame_encode_seekable(raw, in_off, in_len, cb, out=arena, out_off=r_off, out_cap=r_cap, max_chunks=mc, work=ework)
        torch.cuda.synchronize()
        assert int((est != 0).sum()) == 0
        del ework
        # the inserted bytes: the data of the neighbouring stream (as compressible as what they go into), packed
        rawv = raw[:nb * stride].view(nb, stride)
        neighbour = torch.roll(torch.arange(nb, device="cuda"), 1)
        src = rawv[neighbour, 777:777 + ins].contiguous().view(-1) if ins else u8(1)
        s_off, s_len = i64(np.arange(nb) * ins), i64(np.full(nb, ins))
        sp_off, sp_del = i64(np.full(nb, off)), i64(np.full(nb, dele))
        out = u8(nb * cap)
        need = cd.frame_splice_indexed(arena, r_off, f_len, index, sp_off, sp_del, src, s_off, s_len, cb, out, r_off, r_cap, 0, 0)[3].cpu().tolist()
        ms, sc = need[0], need[2]
        work = u8(PL.snp_frame_splice_indexed_workspace(nb, ms, sc, cb))
        got = {}

        def splice():
            got["s"] = cd.frame_splice_indexed(arena, r_off, f_len, index, sp_off, sp_del, src, s_off, s_len, cb, out, r_off, r_cap, ms, sc, work=work)

        common = {"case": case, "streams": nb, "chunk_bytes": cb, "decoded_bytes": nb * n, "framed_bytes": int(eres[1].item()), "off": off, "del": dele,
                  "ins": ins, "slots": ms, "staging_bytes": sc, "workspace_bytes": work.numel()}
        fns, names = [splice], []
        back = edit = dwork = e2work = out2 = uwork = uout = None
        if not a.splice_only and case == "a":
            # what the caller does today: decode every stream, put the edited buffer together, encode it
            spans = int(((f_len.cpu().numpy() + SPAN - 1) // SPAN).sum()) + nb
            back, edit = u8(nb * n), u8(nb * m)
            b_off, e_off, e_len = i64(np.arange(nb) * n), i64(np.arange(nb) * m), i64(np.full(nb, m))
            dwork = u8(FL.snp_frame_decode_buffers_workspace(nb, mc, spans))
            mc2 = nb * ((m + cb - 1) // cb)
            e2work = u8(CL.snp_frame_encode_chunked_workspace(nb, mc2, cb))
            out2 = u8(nb * cap)

            def today():
                cd.frame_decode_buffers(arena, r_off, f_len, back, b_off, in_len, max_chunks=mc, max_spans=spans, work=dwork)
                bv, ev = back.view(nb, n), edit.view(nb, m)
                ev[:, :off] = bv[:, :off]
                ev[:, off:off + ins] = src.view(nb, ins)
                ev[:, off + ins:] = bv[:, off + dele:]
                cd.frame_encode_seekable(edit, e_off, e_len, cb, out=out2, out_off=r_off, out_cap=r_cap, max_chunks=mc2, work=e2work)

            fns.append(today)
            names.append("frame_decode_buffers + device copies + frame_encode_seekable of every edited stream (what a caller does today)")
            # the update call writing the same bytes over what is there: it copies every stream too, and changes no length
            who = torch.arange(nb, dtype=torch.int32, device="cuda")
            uout = u8(nb * cap)
            uneed = cd.frame_write_indexed(arena, r_off, f_len, index, who, sp_off, src, s_off, s_len, uout, r_off, r_cap, 0, 0)[4].cpu().tolist()
            uwork = u8(UL.snp_frame_write_indexed_workspace(nb, nb, uneed[0], uneed[2]))

            def update():
                cd.frame_write_indexed(arena, r_off, f_len, index, who, sp_off, src, s_off, s_len, uout, r_off, r_cap, uneed[0], uneed[2], work=uwork)

            fns.append(update)
            names.append("snp_frame_write_indexed_batch writing the same 4 KiB over the bytes at the same place")
        if not a.splice_only and case == "d":
            mc2 = nb * ((ins + cb - 1) // cb)
            e2work = u8(CL.snp_frame_encode_chunked_workspace(nb, mc2, cb))
            out2 = u8(nb * cap)

            def alone():
                cd.frame_encode_seekable(src, s_off, s_len, cb, out=out2, out_off=r_off, out_cap=r_cap, max_chunks=mc2, work=e2work)

            fns.append(alone)
            names.append("snp_frame_encode_chunked_batch of the same inserted bytes alone")
        res = timed(fns, a.reps)
        out_len, st, new_ix, result = got["s"]
        line = {"what": "snp_frame_splice_indexed_batch", **common, **rec_ms(*res[0]), "result": result.cpu().tolist(),
                "all_written": int((st != 0).sum()) == 0, "copied_GBps": round(float(result[1].item()) / res[0][0] / 1e6, 2)}
        if not a.splice_only:
            del back, edit, dwork, e2work, out2, uwork, uout
            back = edit = dwork = e2work = out2 = uwork = uout = None
            torch.cuda.empty_cache()
            used = int(new_ix.first[-1].item())
            spans = int(((out_len.cpu().numpy() + SPAN - 1) // SPAN).sum()) + nb
            walked = cd.frame_index_buffers(out, r_off, out_len, max_spans=spans, max_entries=used)
            line["new_index_equals_the_walks"] = bool(torch.equal(walked.first, new_ix.first) and torch.equal(walked.start, new_ix.start[:used]) and
                                                      torch.equal(walked.pos, new_ix.pos[:used]) and torch.equal(walked.total, new_ix.total) and
                                                      torch.equal(walked.tail, new_ix.tail))
            # every new stream decoded whole against the edited buffer
            whole = u8(nb * m)
            w_off, w_len = i64(np.arange(nb) * m), i64(np.full(nb, m))
            dw = u8(FL.snp_frame_decode_buffers_workspace(nb, used, spans))
            ol, dst, _ = cd.frame_decode_buffers(out, r_off, out_len, whole, w_off, w_len, max_chunks=used, max_spans=spans, work=dw)
            v = whole.view(nb, m)
            line["round_trip_ok"] = int((dst != 0).sum()) == 0 and bool(torch.equal(ol, w_len)) and bool(
                torch.equal(v[:, :off], rawv[:, :off]) and (ins == 0 or torch.equal(v[:, off:off + ins], src.view(nb, ins))) and
                torch.equal(v[:, off + ins:], rawv[:, off + dele:n]))
            del whole, dw, v
            for k, (name, r) in enumerate(zip(names, res[1:])):
                emit({"what": name, **common, **rec_ms(*r)})
                key = "other" if k == 0 else "update"
                line.update({key + "_ms": round(r[0], 3), key + "_spread_ms": round(max(r[1]) - min(r[1]), 3), key + "_over_splice": round(r[0] / res[0][0], 2)})
        emit(line)
        del arena, out, work, index, got, src, rawv
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "a") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()

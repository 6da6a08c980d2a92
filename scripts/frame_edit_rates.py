"""snp_frame_edit_indexed_batch rates: html-like data (snappier_amd/datagen.py) kept as seekable framed streams with their index, and a sorted edit
script per stream, out of place, on the 10 GiB shapes of frame_splice_rates.py:

  * a: 160 streams of 64 MiB at 65536-byte chunks, K = 1, 16 and 1024 edits per stream of 4 KiB inserted mid-chunk, evenly spread -- beside it,
       interleaved in the same process: the same edits as K calls of snp_frame_splice_indexed_batch, each on what the one before wrote (the
       caller re-bases the offsets; every K is run unless --max-splices lowers the cap); the route over the other seekable calls:
       snp_frame_encode_chunked_batch of the inserted bytes as one stream per old stream with a chunk per edit (so that compose copies
       them whole), into the old streams' arena, the two indexes
       joined, snp_frame_compose_indexed_batch of 2 K + 1 segments per output, and snp_frame_rechunk_indexed_batch of what it wrote (sized
       beforehand, untimed: the three calls only enqueue); and what a caller does without any of them: snp_frame_decode_buffers_batch of every
       stream, the edited buffer put together by device copies, and snp_frame_encode_chunked_batch of it;
  * b: 163 840 streams of 64 KiB at 4096-byte chunks, ONE edit per stream (1000 bytes deleted mid-stream) -- beside it snp_frame_splice_indexed_batch
       on the same inputs: the price of the general plan; the same ratio on the streams of a with K = 1;
  * r: BlockCodec.frame_replace_streams of an 8-byte needle on the first --replace-streams streams of a -- beside it the read + host route: the
       streams decoded, copied to the host, bytes.replace, copied back and encoded.  Wall-clock, synchronised: neither side only enqueues.

After each case every new stream is decoded whole against the edited buffer and the new index is compared with snp_frame_index_batch over the
new streams.  ms from HIP events around each call (median of --reps after one warm-up).  One JSON line per measurement to --out.

    python scripts/frame_edit_rates.py --out profiles/r22a_frame_edit_rates.jsonl
"""
import argparse
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
from frame_splice_rates import SPAN, timed  # noqa: E402

INS = 4096


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="a,b,r")
    ap.add_argument("--edits", default="1,16,1024")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--max-splices", type=int, default=None, help="skip the K splice calls where K is above this (default: run every K)")
    ap.add_argument("--replace-streams", type=int, default=16)
    ap.add_argument("--edit-only", action="store_true", help="the edit only, no comparison and no check (profiling runs)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    html = open(os.path.join(ROOT, "tests", "golden", "testdata", "html"), "rb").read()
    raw = SD.html_like_blocks(html, 0, TOTAL // B, "cuda")
    cd = SB.BlockCodec(0, N.HASH_CRC32C)
    cd.ctx.reserve_compress(TOTAL // B)
    EL, PL, CL, FL = N.frame_edit_lib(), N.frame_splice_lib(), N.frame_chunked_lib(), N.frame_buffers_lib()
    lines = []

    def emit(rec):
        rec["where"] = torch.cuda.get_device_name(0)
        print(json.dumps(rec), flush=True)
        lines.append(rec)

    def encoded(nb, n, cb, cap, extra=0):
        """nb streams of n decoded bytes each, encoded at cb into regions of cap bytes of an arena with `extra` bytes behind them:
        -> (arena, r_off, r_cap, f_len, index, in_len, stride)."""
        stride = (n + B - 1) // B * B
        in_off, in_len = i64(np.arange(nb) * stride), i64(np.full(nb, n))
        mc = nb * ((n + cb - 1) // cb)
        r_off, r_cap = i64(np.arange(nb) * cap), i64(np.full(nb, cap))
        arena = u8(nb * cap + extra)
        ework = u8(CL.snp_frame_encode_chunked_workspace(nb, mc, cb))
        _, _, f_len, est, _, index = cd.frame_encode_seekable(raw, in_off, in_len, cb, out=arena, out_off=r_off, out_cap=r_cap, max_chunks=mc, work=ework)
        torch.cuda.synchronize()
        assert int((est != 0).sum()) == 0
        return arena, r_off, r_cap, f_len, index, in_len, stride

    def verify(line, out, r_off, out_len, new_ix, nb, m, want_rows):
        """The new index against the walk, every new stream decoded whole against want_rows (nb x m)."""
        used = int(new_ix.first[-1].item())
        spans = int(((out_len.cpu().numpy() + SPAN - 1) // SPAN).sum()) + nb
        walked = cd.frame_index_buffers(out, r_off, out_len, max_spans=spans, max_entries=used)
        line["new_index_equals_the_walks"] = bool(torch.equal(walked.first, new_ix.first) and torch.equal(walked.start, new_ix.start[:used]) and
                                                  torch.equal(walked.pos, new_ix.pos[:used]) and torch.equal(walked.total, new_ix.total) and
                                                  torch.equal(walked.tail, new_ix.tail))
        whole = u8(nb * m)
        w_off, w_len = i64(np.arange(nb) * m), i64(np.full(nb, m))
        dw = u8(FL.snp_frame_decode_buffers_workspace(nb, used, spans))
        ol, dst, _ = cd.frame_decode_buffers(out, r_off, out_len, whole, w_off, w_len, max_chunks=used, max_spans=spans, work=dw)
        line["round_trip_ok"] = int((dst != 0).sum()) == 0 and bool(torch.equal(ol, w_len)) and bool(torch.equal(whole.view(nb, m), want_rows))

    for case in a.cases.split(","):
        if case == "a":
            nb, n, cb = TOTAL >> 26, 64 << 20, 65536
            for K in [int(v) for v in a.edits.split(",")]:
                P = n // K                                              # an edit every P bytes, at h inside each period
                h = P // 2 + 777
                m = n + K * INS
                cap = 10 + 8 * ((m + cb - 1) // cb + 2 * K + 2) + m
                icap = 10 + 8 * K + K * INS                             # the inserted bytes of a stream as a stream of their own (a chunk per edit), behind the arena
                arena, r_off, r_cap, f_len, index, in_len, stride = encoded(nb, n, cb, cap, extra=nb * icap)
                rawv = raw[:nb * stride].view(nb, stride)
                neighbour = torch.roll(torch.arange(nb, device="cuda"), 1)
                src = rawv[neighbour, 777:777 + K * INS].contiguous().view(-1)
                ne = nb * K
                ed_first = i64(np.arange(nb + 1) * K)
                ed_off = i64(np.tile(np.arange(K) * P + h, nb))
                ed_del = i64(np.zeros(ne))
                s_off, s_len = i64(np.arange(ne) * INS), i64(np.full(ne, INS))
                out = u8(nb * cap)
                need = cd.frame_edit_indexed(arena, r_off, f_len, index, ed_first, ed_off, ed_del, src, s_off, s_len, cb, out, r_off, r_cap, 0, 0)[4].cpu().tolist()
                ms, sc = need[0], need[2]
                work = u8(EL.snp_frame_edit_indexed_workspace(nb, ne, ms, sc, cb))
                got = {}

                def edit():
                    got["e"] = cd.frame_edit_indexed(arena, r_off, f_len, index, ed_first, ed_off, ed_del, src, s_off, s_len, cb, out, r_off, r_cap, ms, sc, work=work)

                common = {"case": case, "streams": nb, "chunk_bytes": cb, "decoded_bytes": nb * n, "edits_per_stream": K, "ins": INS, "slots": ms,
                          "staging_bytes": sc, "workspace_bytes": work.numel()}
                if a.edit_only:
                    res = timed([edit], a.reps)
                    emit({"what": "snp_frame_edit_indexed_batch", **common, **rec_ms(*res[0])})
                    continue
                # Two arenas every other route writes to.  Each route is timed interleaved with the edit and checked on its own, and gives its
                # buffers back before the next one: together they do not fit the device at K = 1024.
                ping, pong = u8(nb * cap), u8(nb * cap)
                edited = u8(nb * m)                                     # the edited buffer: the decode-and-encode route puts it together, every check reads it
                mc = nb * ((n + cb - 1) // cb)
                mc2 = nb * ((m + cb - 1) // cb)
                spans = int(((f_len.cpu().numpy() + SPAN - 1) // SPAN).sum()) + nb

                def route_today():
                    back = u8(nb * n)
                    b_off, e_off, e_len = i64(np.arange(nb) * n), i64(np.arange(nb) * m), i64(np.full(nb, m))
                    dwork = u8(FL.snp_frame_decode_buffers_workspace(nb, mc, spans))
                    e2work = u8(CL.snp_frame_encode_chunked_workspace(nb, mc2, cb))

                    def today():
                        cd.frame_decode_buffers(arena, r_off, f_len, back, b_off, in_len, max_chunks=mc, max_spans=spans, work=dwork)
                        bv, ev = back.view(nb, K, P), edited.view(nb, K, P + INS)
                        ev[:, :, :h] = bv[:, :, :h]
                        ev[:, :, h:h + INS] = src.view(nb, K, INS)
                        ev[:, :, h + INS:] = bv[:, :, h:]
                        got["t"] = cd.frame_encode_seekable(edited, e_off, e_len, cb, out=ping, out_off=r_off, out_cap=r_cap, max_chunks=mc2, work=e2work)

                    def check(line):
                        _, _, t_len, t_st, _, t_ix = got["t"]
                        verify(line, ping, r_off, t_len, t_ix, nb, m, edited.view(nb, m))
                        got["canonical_len"] = t_len.clone()

                    return today, check

                def route_splices():
                    # the same edits as K splice calls, each on what the one before wrote: two arenas in turn, the offsets re-based by the caller
                    z = i64(np.zeros(nb))
                    ins_len = i64(np.full(nb, INS))
                    pneed = cd.frame_splice_indexed(arena, r_off, f_len, index, i64(np.full(nb, h)), z, src, z, ins_len, cb, ping, r_off, r_cap, 0, 0)[3].cpu().tolist()
                    pwork = u8(PL.snp_frame_splice_indexed_workspace(nb, pneed[0], pneed[2], cb))
                    steps = [(i64(np.full(nb, i * (P + INS) + h)), i64(np.arange(nb) * K * INS + i * INS)) for i in range(K)]

                    def splices():
                        cur, cur_len, ix = arena, f_len, index
                        for i, (off_i, so) in enumerate(steps):
                            dst = ping if i % 2 == 0 else pong
                            cur_len, _, ix, _ = cd.frame_splice_indexed(cur, r_off, cur_len, ix, off_i, z, src, so, ins_len, cb, dst, r_off, r_cap, pneed[0], pneed[2], work=pwork)
                            cur = dst
                        got["p"] = (cur, cur_len, ix)

                    def check(line):
                        cur, cur_len, ix = got["p"]
                        verify(line, cur, r_off, cur_len, ix, nb, m, edited.view(nb, m))

                    return splices, check

                def route_composed():
                    # the inserted bytes encoded as streams (a chunk per edit) behind the old streams, the two indexes joined, compose, rechunk
                    RL, ML = N.frame_rechunk_lib(), N.frame_compose_lib()
                    si_off, si_len = i64(np.arange(nb) * K * INS), i64(np.full(nb, K * INS))
                    i_off, i_cap = i64(nb * cap + np.arange(nb) * icap), i64(np.full(nb, icap))
                    imc = nb * K
                    iwork = u8(CL.snp_frame_encode_chunked_workspace(nb, imc, INS))
                    all_off = torch.cat([r_off, i_off])
                    nseg = 2 * K + 1
                    cuts = np.arange(K) * P + h                         # output b: old [0, cut_0), ins_0, old [cut_0, cut_1), ..., old [cut_(K-1), n)
                    so, sl, ss = np.zeros(nseg, dtype=np.int64), np.zeros(nseg, dtype=np.int64), np.zeros(nseg, dtype=np.int64)
                    so[0::2], sl[0::2] = np.concatenate([[0], cuts]), np.diff(np.concatenate([[0], cuts, [n]]))
                    so[1::2], sl[1::2], ss[1::2] = np.arange(K) * INS, INS, 1
                    seg_first = i64(np.arange(nb + 1) * nseg)
                    seg_stream = torch.from_numpy((np.arange(nb)[:, None] + ss[None, :] * nb).astype(np.int32).reshape(-1)).cuda()
                    seg_off, seg_len = i64(np.tile(so, nb)), i64(np.tile(sl, nb))
                    size = {}

                    def composed():
                        _, _, i_len, _, _, iix = cd.frame_encode_seekable(src, si_off, si_len, INS, out=arena, out_off=i_off, out_cap=i_cap, max_chunks=imc, work=iwork)
                        both = SB.FrameIndex(torch.cat([index.first, iix.first[1:] + index.first[-1]]), torch.cat([index.start, iix.start]),
                                             torch.cat([index.pos, iix.pos]), torch.cat([index.total, iix.total]), torch.cat([index.tail, iix.tail]))
                        lens = torch.cat([f_len, i_len])
                        if "c" not in size:                             # the first pass (the warm-up, untimed) sizes both calls
                            cn = cd.frame_compose_indexed(arena, all_off, lens, both, cb, ping, r_off, r_cap, 0, 0, 0, seg_first, seg_stream, seg_off, seg_len)[3].cpu().tolist()
                            size["c"] = (cn[0], cn[2], cn[4])
                            size["cw"] = u8(ML.snp_frame_compose_indexed_workspace(2 * nb, nb, nb * nseg, cn[0], cn[2], cb, cn[4]))
                        c_len, c_st, c_ix, _ = cd.frame_compose_indexed(arena, all_off, lens, both, cb, ping, r_off, r_cap, *size["c"], seg_first, seg_stream,
                                                                        seg_off, seg_len, work=size["cw"])
                        if "r" not in size:
                            rn = cd.frame_rechunk_indexed(ping, r_off, c_len, c_ix, cb, pong, r_off, r_cap, 0, 0, 0)[3].cpu().tolist()
                            size["r"] = (rn[0], rn[2], rn[4])
                            size["rw"] = u8(RL.snp_frame_rechunk_indexed_workspace(nb, rn[0], rn[2], cb, rn[4]))
                        got["c"] = (c_st,) + tuple(cd.frame_rechunk_indexed(ping, r_off, c_len, c_ix, cb, pong, r_off, r_cap, *size["r"], work=size["rw"]))

                    def check(line):
                        c_st, r_len, r_st, r_ix, _ = got["c"]
                        verify(line, pong, r_off, r_len, r_ix, nb, m, edited.view(nb, m))
                        line["all_written"] = int((c_st != 0).sum()) == 0 and int((r_st != 0).sum()) == 0
                        line["equals_the_encoders_output"] = bool(torch.equal(r_len, got["canonical_len"]))
                        line["workspace_bytes"] = size["cw"].numel() + size["rw"].numel() + iwork.numel()

                    return composed, check

                routes = [("frame_decode_buffers + device copies + frame_encode_seekable of every edited stream", route_today)]
                if a.max_splices is None or K <= a.max_splices:
                    routes.append(("the same edits as %d calls of snp_frame_splice_indexed_batch" % K, route_splices))
                routes.append(("frame_encode_seekable of the inserted bytes + frame_compose_indexed + frame_rechunk_indexed", route_composed))
                edit_ms = []
                for name, make in routes:
                    fn, check = make()
                    res = timed([edit, fn], a.reps)
                    edit_ms += res[0][1]
                    rec = {"what": name, **common, **rec_ms(*res[1]), "edit_ms_beside_it": round(res[0][0], 3), "over_edit": round(res[1][0] / res[0][0], 2)}
                    check(rec)
                    emit(rec)
                    del fn, check
                    torch.cuda.empty_cache()
                out_len, st, ed_st, new_ix, result = got["e"]
                line = {"what": "snp_frame_edit_indexed_batch", **common, **rec_ms(float(np.median(edit_ms)), edit_ms), "result": result.cpu().tolist(),
                        "all_written": int((st != 0).sum()) == 0, "copied_GBps": round(float(result[1].item()) / float(np.median(edit_ms)) / 1e6, 2)}
                verify(line, out, r_off, out_len, new_ix, nb, m, edited.view(nb, m))
                emit(line)
                del arena, out, work, index, got, src, rawv, ping, pong, edited, routes
                torch.cuda.empty_cache()
        if case == "b":
            for nb, n, cb, off, dele, ins in ((TOTAL // B, B, 4096, 30000, 1000, 0), (TOTAL >> 26, 64 << 20, 65536, (32 << 20) + 777, 0, INS)):
                m = n - dele + ins
                cap = 10 + 8 * ((max(n, m) + cb - 1) // cb + 2) + max(n, m)
                arena, r_off, r_cap, f_len, index, in_len, stride = encoded(nb, n, cb, cap)
                rawv = raw[:nb * stride].view(nb, stride)
                src = rawv[torch.roll(torch.arange(nb, device="cuda"), 1), 777:777 + ins].contiguous().view(-1) if ins else u8(1)
                s_off, s_len = i64(np.arange(nb) * ins), i64(np.full(nb, ins))
                sp_off, sp_del = i64(np.full(nb, off)), i64(np.full(nb, dele))
                ed_first = i64(np.arange(nb + 1))
                out, out_s = u8(nb * cap), u8(nb * cap)
                out.zero_()                                             # (the arenas are compared whole below)
                out_s.zero_()
                need = cd.frame_splice_indexed(arena, r_off, f_len, index, sp_off, sp_del, src, s_off, s_len, cb, out, r_off, r_cap, 0, 0)[3].cpu().tolist()
                ms, sc = need[0], need[2]
                ework, pwork = u8(EL.snp_frame_edit_indexed_workspace(nb, nb, ms, sc, cb)), u8(PL.snp_frame_splice_indexed_workspace(nb, ms, sc, cb))
                got = {}

                def edit():
                    got["e"] = cd.frame_edit_indexed(arena, r_off, f_len, index, ed_first, sp_off, sp_del, src, s_off, s_len, cb, out, r_off, r_cap, ms, sc, work=ework)

                def splice():
                    got["s"] = cd.frame_splice_indexed(arena, r_off, f_len, index, sp_off, sp_del, src, s_off, s_len, cb, out_s, r_off, r_cap, ms, sc, work=pwork)

                res = timed([edit, splice], a.reps)
                (e_len, e_st, _, e_ix, e_res), (s_len2, s_st, s_ix, s_res) = got["e"], got["s"]
                used = int(s_ix.first[-1].item())
                emit({"what": "snp_frame_edit_indexed_batch, ONE edit per stream, beside snp_frame_splice_indexed_batch on the same inputs", "case": case,
                      "streams": nb, "chunk_bytes": cb, "decoded_bytes": nb * n, "off": off, "del": dele, "ins": ins, **rec_ms(*res[0]),
                      "splice_ms": round(res[1][0], 3), "splice_spread_ms": round(max(res[1][1]) - min(res[1][1]), 3),
                      "edit_over_splice": round(res[0][0] / res[1][0], 3),
                      "same_bytes_and_index": bool(torch.equal(out, out_s) and torch.equal(e_len, s_len2) and torch.equal(e_st, s_st) and
                                                   torch.equal(e_res, s_res) and torch.equal(e_ix.first, s_ix.first) and
                                                   torch.equal(e_ix.start[:used], s_ix.start[:used]) and torch.equal(e_ix.pos[:used], s_ix.pos[:used]) and
                                                   torch.equal(e_ix.total, s_ix.total))})
                del arena, out, out_s, ework, pwork, index, got, src, rawv
                torch.cuda.empty_cache()
        if case == "r":
            nb, n, cb = a.replace_streams, 64 << 20, 65536
            needle, repl = b"<a href=", b"<a rel=nofollow href="
            cap = 10 + 8 * ((n + cb - 1) // cb + 2) + n
            arena, r_off, r_cap, f_len, index, in_len, stride = encoded(nb, n, cb, cap)

            def wall(fn):
                ms = []
                for _ in range(3):                                      # (seconds a round: one warm-up, two measured)
                    torch.cuda.synchronize()
                    t = time.perf_counter()
                    r = fn()
                    torch.cuda.synchronize()
                    ms.append((time.perf_counter() - t) * 1e3)
                return (float(np.median(ms[1:])), ms[1:]), r

            def host():
                back = u8(nb * n)
                mc = nb * ((n + cb - 1) // cb)
                cd.frame_decode_buffers(arena, r_off, f_len, back, i64(np.arange(nb) * n), in_len, max_chunks=mc,
                                        max_spans=int(((f_len.cpu().numpy() + SPAN - 1) // SPAN).sum()) + nb)
                new = [bytes(x).replace(needle, repl) for x in back.view(nb, n).cpu().numpy()]
                lens = np.array([len(x) for x in new], dtype=np.int64)
                offs = np.cumsum(lens) - lens
                dev = torch.from_numpy(np.frombuffer(b"".join(new), dtype=np.uint8).copy()).cuda()
                big = 10 + 8 * ((int(lens.max()) + cb - 1) // cb + 2) + int(lens.max())
                cd.frame_encode_seekable(dev, i64(offs), i64(lens), cb, out=u8(nb * big), out_off=i64(np.arange(nb) * big), out_cap=i64(np.full(nb, big)),
                                         max_chunks=int(((lens + cb - 1) // cb).sum()))
                return new

            (r_ms, r_all), got = wall(lambda: cd.frame_replace_streams(arena, r_off, f_len, index, needle, repl, cb))
            (h_ms, h_all), new = wall(host)
            out, out_off, out_len, st, new_ix, count = got
            line = {"what": "BlockCodec.frame_replace_streams, an 8-byte needle, wall-clock", "case": case, "streams": nb, "chunk_bytes": cb, "decoded_bytes": nb * n,
                    "needle": needle.decode(), "replacement": repl.decode(), "replacements": int(count.sum().item()), **rec_ms(r_ms, r_all),
                    "host_ms": round(h_ms, 1), "host_over_replace": round(h_ms / r_ms, 2), "all_written": int((st != 0).sum()) == 0}
            back = u8(int(new_ix.total.sum().item()))
            lens = new_ix.total.clone()
            offs = torch.cumsum(lens, 0) - lens
            used = int(new_ix.first[-1].item())
            ol, dst, _ = cd.frame_decode_buffers(out, out_off, out_len, back, offs, lens, max_chunks=used,
                                                 max_spans=int(((out_len.cpu().numpy() + SPAN - 1) // SPAN).sum()) + nb)
            h = back.cpu().numpy()
            line["equals_bytes_replace"] = int((dst != 0).sum()) == 0 and all(
                h[o:o + k].tobytes() == x for o, k, x in zip(offs.tolist(), lens.tolist(), new))
            emit(line)
    if a.out:
        with open(a.out, "a") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()

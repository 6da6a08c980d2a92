"""snp_frame_recut_indexed_batch (BlockCodec.frame_recut_indexed / frame_recut_to_memory / frame_recut_content_defined): every new stream, status,
length, size bound, index array and d_result against the model (frame_recut_model.py), with canary bytes around every output range, guard words
around every array and the workspace, and the inputs compared with their copies after the call (recut_harness.Recut): a grid list against the
model and against the device's own rechunk (guarantee (a)); the encoder's output at the list (b, c); directed lists; foreign streams; every
rejection of a list; unsound indexes; admission; corruption; the new index against snp_frame_index_batch, under the read, digest, find and dedup
calls and under a second recut; the end-to-end property through the wrappers, and the dedup of the result; a splice and a recut without
synchronisation; graph capture; the launch tiers of the compressor and the decoder by bound and by real count; every layout; a kept chunk past
position 2^32 of both streams.  Needs an MI355X."""
import numpy as np
import pytest
import torch

import frame_buffers_helpers as H
import frame_buffers_model as M
import frame_chunked_model as K
import frame_cuts_model as CM
import frame_index_model as X
import frame_range_model as R
import frame_rechunk_model as RC
import frame_recut_model as RX
import frame_splice_model as S
import layouts
import oracle as O
from conftest import read_testdata
from rechunk_harness import Rechunked
from recut_harness import Recut, new_table
from seekable_harness import CANARY, Guarded, index_call, index_tensors
from test_frame_rechunk_model import fragmented

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from snappier_amd import batch as SB, _native as N

VARIANTS = [O.HASH_CRC32C, O.HASH_MUL]
ALL = RX.REWRITE_ALL


@pytest.fixture(scope="module")
def html():
    return read_testdata("html") * 5


@pytest.fixture(scope="module")
def named():
    cases = X.named_streams()
    streams = list(cases.values())
    return list(cases), streams, X.build_index(streams)


def device_index(ix, ns):
    index = SB.FrameIndex(*index_tensors(ix, ns)[0])
    index.start, index.pos = index.start[:len(ix["start"])], index.pos[:len(ix["pos"])]
    return index


def walked_like(cd, rc):
    """The new index is what snp_frame_index_batch gives for the resulting streams."""
    assert index_call(cd, rc.after()) == {**rc.got["index"], "result": X.build_index(rc.after())["result"]}


def streams_of(out, off, lens, old=None):
    h = out.cpu().numpy()
    return [h[o:o + n].tobytes() if n or old is None else old[b] for b, (o, n) in enumerate(zip(off.tolist(), lens.tolist()))]


# ---- 1: a grid list is the rechunk (a); the encoder's output at the list (b), (c) ------------------------------------------------------------------
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("cb", RC.CHUNK_SIZES)
def test_a_grid_list_gives_what_the_rechunk_gives(html, cb, variant):
    cd = SB.BlockCodec(0, variant)
    names, raws, streams = fragmented(html, cb, variant)
    streams, raws = streams + [K.stream_of(raws[0], cb, variant), M.STREAM_ID, b""], raws + [raws[0], b"", b""]
    ix = X.build_index(streams)
    first, cuts = CM.regular_cuts([len(a) for a in raws], cb)
    want = CM.encode_at_cuts(raws, first, cuts, variant)["streams"]
    for flags in (0, ALL):
        rc = Recut(cd, streams, ix, first, cuts, flags, variant=variant).check()
        grid = Rechunked(cd, streams, ix, cb, flags, variant=variant)     # the device's own rechunk
        for key in ("status", "out_len", "streams", "index", "out_bound"):
            assert rc.got[key] == grid.got[key], (key, flags)
        assert [rc.got["result"][i] for i in (0, 1, 3, 4, 5)] == [grid.got["result"][i] for i in (0, 1, 3, 4, 5)]
        assert rc.after() == want
        walked_like(cd, rc)
    # fed to a second recut, every stream is left alone
    rc = Recut(cd, streams, ix, first, cuts, variant=variant)
    again = Recut(cd, rc.after(), rc.got["index"], first, cuts, variant=variant).check()
    assert again.got["streams"] == [None] * len(streams) and again.got["result"] == [0, 0, 0, 0, len(rc.got["index"]["start"]), len(streams), 0, 0]
    assert again.got["index"] == rc.got["index"]
    # another grid and the content's own cuts, at once
    for first2, cuts2 in (CM.regular_cuts([len(a) for a in raws], min(cb + 1, 65536)), RX.content_lists(raws, 32, min(max(cb, 33), 4096))):
        other = Recut(cd, streams, ix, first2, cuts2, variant=variant).check()
        enc = CM.encode_at_cuts(raws, first2, cuts2, variant)
        assert other.after() == enc["streams"] and all(other.got["index"][k] == enc[k] for k in ("first", "start", "pos", "total", "tail"))


def test_directed_lists(html):
    cd = SB.BlockCodec(0, O.HASH_CRC32C)
    cases = RX.directed(read_testdata("html"))
    names = list(cases)
    streams, raws = [cases[n][0] for n in names], [cases[n][1] for n in names]
    first, cuts = RX.lists([cases[n][2] for n in names])
    ix = X.build_index(streams)
    rc = Recut(cd, streams, ix, first, cuts).check()
    assert rc.got["status"] == [O.OK] * len(names) and rc.after() == CM.encode_at_cuts(raws, first, cuts)["streams"]
    assert rc.got["result"][6] > 10 and rc.got["result"][7] > 10 and rc.got["result"][5] == 2
    walked_like(cd, rc)
    every = Recut(cd, streams, ix, first, cuts, ALL).check()
    assert every.got["streams"] == CM.encode_at_cuts(raws, first, cuts)["streams"] and every.got["result"][6] == 0
    sizing = Recut(cd, streams, ix, first, cuts, caps=[0] * len(names), max_slots=0, stage_cap=0, max_entries=0).check()
    assert sizing.got["streams"] == [None] * len(names) and sizing.got["out_bound"] == rc.got["out_bound"]
    assert [sizing.got["result"][i] for i in (0, 2, 4)] == [rc.ms, rc.sc, rc.me]


def test_foreign_and_named_streams_with_and_without_rewrite_all(html, named):
    cd = SB.BlockCodec(0, O.HASH_CRC32C)
    cases = RC.foreign_streams(html)
    streams, raws = [c[0] for c in cases.values()], [c[1] for c in cases.values()]
    ix = X.build_index(streams)
    for first, cuts in (RX.content_lists(raws, 32, 256), CM.regular_cuts([len(a) for a in raws], 500)):
        every = Recut(cd, streams, ix, first, cuts, ALL).check()
        assert every.got["streams"] == CM.encode_at_cuts(raws, first, cuts)["streams"]                  # (b)
        rc = Recut(cd, streams, ix, first, cuts).check()
        assert rc.got["status"] == [O.OK] * len(streams)
        for b, (new, a) in enumerate(zip(rc.after(), raws)):            # (d)
            assert O.frame_decode(new) == a and X.build_index([new])["start"] == [0] * bool(a) + cuts[first[b]:first[b + 1]], b
        walked_like(cd, rc)
    names, streams, ix = named
    first, cuts = RX.lists([list(range(300, t, 300)) for t in ix["total"]])
    for flags in (0, ALL):
        rc = Recut(cd, streams, ix, first, cuts, flags).check()
        assert sum(1 for x in rc.got["streams"] if x is not None) >= 8 and len(set(rc.got["status"])) >= 3
        walked_like(cd, rc)


def mixed_batch(html, variant=O.HASH_CRC32C):
    """Content-defined streams after edits, grid streams, foreign, broken and empty streams, compressed and raw chunks, under the content's own
    cuts, a grid, and a list that is bad: -> (streams, index, cut_first, cuts)."""
    rnd = bytes(np.random.default_rng(3).integers(0, 256, 3 * 4096 + 77, dtype=np.uint8))
    e2e = RX.end_to_end(read_testdata("html"), 32, 256, variant)
    foreign = [c for c in RC.foreign_streams(html).values()]
    broken = R.uniform_stream(3, 1)[0][:-5]
    ch = M.data_chunk
    streams = [c[0] for c in e2e.values()] + [K.stream_of(html[:3500], 1000, variant), K.stream_of(rnd, 4096, variant), foreign[0][0], broken, b"",
                                              foreign[2][0], M.STREAM_ID + ch(rnd[:700], False) + ch(html[:300]) + ch(rnd[700:1400], False),
                                              K.stream_of(html[:70000], 65536, variant), K.stream_of(html[:5000], 1000, variant)]
    raws = [c[1] for c in e2e.values()] + [html[:3500], rnd, foreign[0][1], b"", b"", foreign[2][1], rnd[:700] + html[:300] + rnd[700:1400], html[:70000],
                                           html[:5000]]
    per = [CM.cuts_of(a, 32, 256)[0] for a in raws[:4]] + [[1000, 2000, 3000], [5000, 9000], CM.cuts_of(raws[6], 32, 256)[0], [], [],
                                                           CM.cuts_of(raws[9], 64, 1024)[0], [700, 1000], [4464, 70000 - 100], [1000, 900]]
    first, cuts = RX.lists(per)
    return streams, X.build_index(streams), first, cuts


def test_a_mixed_batch_written_left_alone_refused_and_broken(html):
    cd = SB.BlockCodec(0, O.HASH_MUL)
    streams, ix, first, cuts = mixed_batch(html, O.HASH_MUL)
    free = RX.recut_plan(streams, ix, first, cuts, variant=O.HASH_MUL)
    caps = list(free["out_bound"])
    caps[1] = free["out_len"][1] - 1                                    # refused: its range is one byte short
    rc = Recut(cd, streams, ix, first, cuts, caps=caps, variant=O.HASH_MUL).check()
    assert rc.got["status"][1] == O.ERR_OUTPUT_TOO_SMALL and rc.got["status"][7] == ix["tail"][7] != O.OK and rc.got["status"][12] == O.ERR_BAD_ARG
    assert rc.got["streams"][4] is None and rc.got["status"][4] == O.OK and rc.got["streams"][10] is None and rc.got["result"][5] == 2
    assert rc.got["result"][3] == len(streams) - 5 and rc.got["result"][6] > 100 and rc.got["result"][7] > 20
    walked_like(cd, rc)


# ---- 2: the new index under the sibling calls -----------------------------------------------------------------------------------------------------
def test_the_new_index_serves_the_read_digest_find_dedup_and_a_second_recut(html):
    cd = SB.BlockCodec(0, O.HASH_CRC32C)
    cases = RX.end_to_end(read_testdata("html"))
    streams, now = [c[0] for c in cases.values()], [c[1] for c in cases.values()]
    first, cuts = RX.content_lists(now, 32, 256)
    rc = Recut(cd, streams, X.build_index(streams), first, cuts).check()
    ns = len(now)
    assert rc.got["result"][3] == ns
    framed, off, lens = new_table(rc)
    index = rc.frame_index()
    stream_no = torch.arange(ns, dtype=torch.int32, device="cuda")
    out, out_off, out_len, status = cd.frame_gather_to_memory(framed, off, lens, index, stream_no, H.dev([0] * ns), H.dev([len(x) for x in now]))
    assert status.tolist() == [O.OK] * ns and streams_of(out, out_off, out_len) == now
    digest, dig_len, dst = cd.frame_digest_streams(framed, off, lens, index)
    assert dst.tolist() == [O.OK] * ns and dig_len.tolist() == [len(x) for x in now]
    assert [d & 0xFFFFFFFF for d in digest.tolist()] == [O.crc32c(x) for x in now]
    needle = now[0][4000:4009]
    count, hits, fst = cd.frame_find_streams(framed, off, lens, index, needle)
    assert fst.tolist() == [O.OK] * ns and count.tolist() == [x.count(needle) for x in now] and hits[0].tolist()[0] == now[0].find(needle)
    # dedup: the recut streams against freshly encoded ones -- every row merges
    fresh = CM.encode_at_cuts(now, first, cuts)["streams"]
    both, boff, blen = H.pack(fresh + rc.after())
    bix = device_index(X.build_index(fresh + rc.after()), 2 * ns)
    pack, _, _, _, dstatus, dres = cd.frame_dedup_to_memory(both, H.dev(boff), H.dev(blen), bix, ns)
    assert dstatus.tolist() == [O.OK] * (2 * ns) and dres.tolist()[5] == len(cuts) + ns
    # a second recut, through the wrapper that sizes it: every stream is left alone
    out2, off2, len2, st2, ix2 = cd.frame_recut_to_memory(framed, off, lens, index, H.dev(first), H.dev(cuts))
    assert st2.tolist() == [O.OK] * ns and len2.tolist() == [0] * ns and out2.numel() == 0 and ix2.result.tolist() == [0, 0, 0, 0, len(cuts) + ns, ns, 0, 0]
    assert ix2.pos.tolist() == rc.got["index"]["pos"]


# ---- 3: the end-to-end property through the wrappers, and what the dedup makes of it -------------------------------------------------------------
@pytest.mark.parametrize("variant", VARIANTS)
def test_content_defined_streams_after_edits_come_back_to_the_encoders_chunks(variant):
    cd = SB.BlockCodec(0, variant)
    text = read_testdata("html") * 2
    rng = np.random.default_rng(9)
    raws = [bytes(rng.integers(0, 64, 9000, dtype=np.uint8)), text[:20000], text[300:9000], b"", text[:50]]
    ns = len(raws)
    data, doff, dlen = H.pack(raws)
    base, base_off, base_len, st, _, base_ix = cd.frame_encode_content_defined(data, H.dev(doff), H.dev(dlen), 32, 256)
    assert st.tolist() == [O.OK] * ns
    # one splice per stream (an insert mid-chunk, a delete across chunks, a truncate, nothing, an insert in front), then an append to each
    edits = [(4000, 0), (7000, 900), (5000, 3700), (0, 0), (0, 0)]
    ins = [text[100:137], b"", b"", b"", text[:3]]
    isrc, ioff, ilen = H.pack(ins)
    s_out, s_off, s_len, s_st, s_ix = cd.frame_splice_to_memory(base, base_off, base_len, base_ix, H.dev([q[0] for q in edits]),
                                                                H.dev([q[1] for q in edits]), isrc, H.dev(ioff), H.dev(ilen), 256)
    assert s_st.tolist() == [O.OK] * ns
    spliced = streams_of(s_out, s_off, s_len, streams_of(base, base_off, base_len))
    more = [text[777:777 + n] for n in (700, 1, 0, 300, 65)]
    caps = [len(s) + len(m) + 8 * (len(m) // 256 + 2) + 64 for s, m in zip(spliced, more)]
    from append_harness import arena_of
    buf, boff = arena_of(spliced, caps)
    asrc, aoff, alen = H.pack(more)
    new_len, a_st, a_ix = cd.frame_append_to_memory(buf, H.dev(boff), H.dev([len(s) for s in spliced]), H.dev(caps), s_ix, asrc, H.dev(aoff), H.dev(alen), 256)
    assert a_st.tolist() == [O.OK] * ns
    edited = [(x[:q[0]] + i + x[q[0] + q[1]:]) + m for x, q, i, m in zip(raws, edits, ins, more)]
    grown = streams_of(buf, H.dev(boff), new_len)
    assert [O.frame_decode(s) for s in grown] == edited
    # the recut to the content's own cuts, against the encoder from scratch: bytes and index
    out, off, lens, status, new_ix = cd.frame_recut_content_defined(buf, H.dev(boff), new_len, a_ix, 32, 256)
    edata, eoff, elen = H.pack(edited)
    want, want_off, want_len, wst, _, want_ix = cd.frame_encode_content_defined(edata, H.dev(eoff), H.dev(elen), 32, 256)
    fresh = streams_of(want, want_off, want_len)
    assert status.tolist() == [O.OK] * ns and streams_of(out, off, lens, grown) == fresh
    used = int(new_ix.first[-1])
    assert new_ix.first.tolist() == want_ix.first.tolist() and new_ix.start[:used].tolist() == want_ix.start[:used].tolist()
    assert new_ix.pos[:used].tolist() == want_ix.pos[:used].tolist() and new_ix.total.tolist() == want_ix.total.tolist() and new_ix.tail.tolist() == [0] * ns
    res = new_ix.result.tolist()
    assert res[3] + res[5] == ns and res[6] > 4 * res[7] > 0            # almost every chunk was copied
    model = RX.recut_plan(grown, X.build_index(grown), *RX.content_lists(edited, 32, 256), variant=variant)
    assert model["result"] == res and RX.after(grown, model) == fresh
    # the dedup of (base, recut stream) reports what the dedup of (base, freshly encoded stream) reports
    bases = streams_of(base, base_off, base_len)
    reports = []
    for news in (streams_of(out, off, lens, grown), fresh):
        both, o, n = H.pack(bases + news)
        r = cd.frame_dedup_to_memory(both, H.dev(o), H.dev(n), device_index(X.build_index(bases + news), 2 * ns), ns)[-1].tolist()
        reports.append((r[0], r[5]))
    assert reports[0] == reports[1] and reports[0][1] > 100


# ---- 4: a splice and a recut on one context, no synchronisation between them; graph capture ------------------------------------------------------
def test_a_splice_and_a_recut_in_a_row(html):
    cd = SB.BlockCodec(0, O.HASH_CRC32C)
    cases = RX.end_to_end(read_testdata("html"))
    raws = [c[1] for c in cases.values()][:3]
    streams = [RX.stream_at(a, CM.cuts_of(a, 32, 256)[0]) for a in raws]
    ix = X.build_index(streams)
    step = [(3000, 0, 40), (100, 2000, 0), (len(raws[2]), 0, 333)]
    srcs = [html[17 * b:17 * b + q[2]] for b, q in enumerate(step)]
    w = S.splice_plan(streams, ix, [q[:2] for q in step], srcs, 256)        # the model runs ahead: every call is sized without a read-back
    assert w["status"] == [O.OK] * 3
    raws = [S.edited(x, q[0], q[1], s) for x, q, s in zip(raws, step, srcs)]
    first, cuts = RX.content_lists(raws, 32, 256)
    want = RX.recut_plan(w["streams"], w["index"], first, cuts)
    assert RX.after(w["streams"], want) == CM.encode_at_cuts(raws, first, cuts)["streams"] and want["result"][6] > want["result"][7] > 0
    framed, in_off, in_len = H.pack(streams)
    src, src_off, src_len = H.pack(srcs)
    out_off, total = H.out_layout(np.array(w["out_bound"], dtype=np.int64))
    mid = torch.full((total,), CANARY, dtype=torch.uint8, device="cuda")
    mid_len, _, index, _ = cd.frame_splice_indexed(framed, H.dev(in_off), H.dev(in_len), device_index(ix, 3), H.dev([q[0] for q in step]),
                                                   H.dev([q[1] for q in step]), src, H.dev(src_off), H.dev(src_len), 256, mid, H.dev(out_off),
                                                   H.dev(w["out_bound"]), w["result"][0], w["result"][2])
    off2, total2 = H.out_layout(np.array(want["out_bound"], dtype=np.int64))
    out = torch.full((total2,), CANARY, dtype=torch.uint8, device="cuda")
    out_len, status, index, result = cd.frame_recut_indexed(mid, H.dev(out_off), mid_len, index, H.dev(first), H.dev(cuts), out, H.dev(off2),
                                                            H.dev(want["out_bound"]), want["result"][0], want["result"][2], want["result"][4])
    torch.cuda.synchronize()
    assert status.tolist() == [O.OK] * 3 and out_len.tolist() == want["out_len"] and result.tolist() == want["result"]
    h = out.cpu().numpy()
    assert [h[o:o + n].tobytes() if n else None for o, n in zip(off2.tolist(), out_len.tolist())] == want["streams"]
    assert (H.outside_ranges(h, off2.tolist(), out_len.tolist()) == CANARY).all()
    used = want["index"]["first"][-1]
    assert index.first.tolist() == want["index"]["first"] and index.start[:used].tolist() == want["index"]["start"]
    assert index.pos[:used].tolist() == want["index"]["pos"] and index.total.tolist() == want["index"]["total"] and index.tail.tolist() == [0] * 3


def test_graph_capture_replays_the_call_twice(html):
    cd = SB.BlockCodec(0, O.HASH_CRC32C)
    streams, ix, first, cuts = mixed_batch(html)
    ns = len(streams)
    want = RX.recut_plan(streams, ix, first, cuts)
    ms, sc, me = want["result"][0], want["result"][2], want["result"][4]
    framed, in_off, in_len = H.pack(streams)
    out_off, total = H.out_layout(np.array(want["out_bound"], dtype=np.int64))
    out = torch.full((total,), CANARY, dtype=torch.uint8, device="cuda")
    index = device_index(ix, ns)
    tabs = [H.dev(in_off), H.dev(in_len), H.dev(out_off), H.dev(want["out_bound"]), H.dev(first), H.dev(cuts)]
    work = torch.empty(N.frame_recut_lib().snp_frame_recut_indexed_workspace(ns, ms, sc, me), dtype=torch.uint8, device="cuda")

    def call():
        return cd.frame_recut_indexed(framed, tabs[0], tabs[1], index, tabs[4], tabs[5], out, tabs[2], tabs[3], ms, sc, me, work=work)

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        call()                                                          # the same call once before the capture
        torch.cuda.synchronize()
        plain = out.clone()
        out.fill_(CANARY)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        out_len, status, new_ix, result = call()
    for _ in range(2):
        out.fill_(CANARY)
        work.fill_(CANARY)
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, plain)
        assert status.tolist() == want["status"] and out_len.tolist() == want["out_len"] and result.tolist() == want["result"]
        used = want["index"]["first"][-1]
        assert new_ix.first.tolist() == want["index"]["first"] and new_ix.pos[:used].tolist() == want["index"]["pos"]
    h = out.cpu().numpy()
    for b, x in enumerate(want["streams"]):
        if x is not None:
            assert h[out_off[b]:out_off[b] + len(x)].tobytes() == x, b


# ---- 5: admission; every rejection of a list; corruption; the index is untrusted; empty calls ------------------------------------------------------
def test_admission_by_each_bound_and_by_out_cap(html):
    cd = SB.BlockCodec(0, O.HASH_CRC32C)
    blobs = [html[:700], html[50:50 + 1024], html[9:9 + 1300], html[:100], html[:2000]]
    streams = [K.stream_of(x, 500) for x in blobs[:3]] + [K.stream_of(blobs[3], 512), K.stream_of(blobs[4], 300)]
    ix = X.build_index(streams)
    first, cuts = RX.lists([[512], [512], [500, 1012], [], [300, 700, 1200, 1500]])
    full = Recut(cd, streams, ix, first, cuts).check()
    assert full.got["status"] == [O.OK] * 5
    sizing = Recut(cd, streams, ix, first, cuts, caps=[0] * 5, max_slots=0, stage_cap=0, max_entries=0).check()
    ms, _, sc, _, me, alone, _, _ = sizing.got["result"]
    assert (ms, me, alone) == (12, 16, 1) and sc == full.sc and sizing.got["streams"] == [None] * 5 and sizing.got["out_bound"] == full.got["out_bound"]
    late = [O.OK, O.OK, O.OK, O.OK, O.ERR_OUTPUT_TOO_SMALL]
    mid = [O.OK, O.ERR_OUTPUT_TOO_SMALL, O.ERR_OUTPUT_TOO_SMALL, O.OK, O.ERR_OUTPUT_TOO_SMALL]
    assert Recut(cd, streams, ix, first, cuts, max_slots=ms - 1).check().got["status"] == late
    assert Recut(cd, streams, ix, first, cuts, stage_cap=sc - 1).check().got["status"] == late
    assert Recut(cd, streams, ix, first, cuts, max_entries=me - 1).check().got["status"] == late
    assert Recut(cd, streams, ix, first, cuts, max_slots=4).check().got["status"] == mid
    two = 700 + 1024 + K.stride(512) * 3 + K.stride(188)
    assert Recut(cd, streams, ix, first, cuts, stage_cap=two - 1).check().got["status"] == mid
    assert Recut(cd, streams, ix, first, cuts, stage_cap=two).check().got["status"][:2] == [O.OK, O.OK]
    assert Recut(cd, streams, ix, first, cuts, max_entries=4).check().got["status"] == mid
    caps = list(full.got["out_len"])
    caps[2] -= 1                                                        # one byte short, in the middle of the batch
    one = Recut(cd, streams, ix, first, cuts, caps=caps).check()
    assert one.got["status"] == [O.OK, O.OK, O.ERR_OUTPUT_TOO_SMALL, O.OK, O.OK] and one.got["result"][3] == 3
    walked_like(cd, one)
    assert Recut(cd, streams, ix, first, cuts, caps=full.got["out_len"]).check().got == full.got


def test_every_list_rejection_fails_its_stream_alone(html):
    cd = SB.BlockCodec(0, O.HASH_CRC32C)
    raws = [html[:2500], html[100:3300], html[7:1800]]
    streams = [K.stream_of(a, 900) for a in raws]
    ix = X.build_index(streams)
    good = [[1000, 2000], [500], [900]]
    total = len(raws[1])
    for bc in ([0, 1000], [1000, total], [1000, total + 5], [1000, 1000, 2000], [2000, 1000, 2500], [1000, 2000, 1999], [1 << 63, 5]):
        rc = Recut(cd, streams, ix, *RX.lists([good[0], bc, good[2]])).check()
        assert rc.got["status"] == [O.OK, O.ERR_BAD_ARG, O.OK] and rc.got["result"][3] == 1 and rc.got["result"][5] == 1, bc
    flat = good[0] + good[1] + good[2] + [1000, 1200]
    for first, ncuts in (([0, 2, 3, 1], None), ([0, 2, 3, 7], None), ([0, 2, 3, 4], 3), ([0, 2, 3, 1 << 63], None), ([0, 2, (1 << 64) - 1, 4], None)):
        rc = Recut(cd, streams, ix, first, flat, ncuts=ncuts).check()
        assert rc.got["status"][0] == O.OK and rc.got["status"][2] == O.ERR_BAD_ARG, first
    big = (html * 3)[:140000]
    s = K.stream_of(big, 65536)
    for cuts, ok in (([65536, 131072], True), ([65537, 131072], False), ([65536], False), ([4464, 70000, 135536], True), ([4463, 70000], False)):
        assert Recut(cd, [s], X.build_index([s]), [0, len(cuts)], cuts).check().got["status"] == [O.OK if ok else O.ERR_BAD_ARG], cuts
    for e in (M.STREAM_ID, b""):
        assert Recut(cd, [e], X.build_index([e]), [0, 1], [1]).check().got["status"] == [O.ERR_BAD_ARG]
        assert Recut(cd, [e], X.build_index([e]), [0, 0], []).check().got["status"] == [O.OK]


def test_corruption_in_a_dirty_chunk_in_a_kept_chunk_and_the_scrub(html):
    cd = SB.BlockCodec(0, O.HASH_CRC32C)
    raw = html[:9000]
    cuts = [1000, 3000, 4000, 6500]
    s = RX.stream_at(raw, [1000, 3000, 5000, 6500])
    rows = R.walk(s)[0]
    bad = [R.corrupt_chunk(s, rows[i]) for i in (0, 2, 3)]
    both = R.corrupt_chunk(bad[1], rows[3])
    want2, want3 = M.chunk_status(bad[1], rows[2]), M.chunk_status(bad[2], rows[3])
    ix = X.build_index([s] * 5)
    first, flat = RX.lists([cuts] * 5)
    rc = Recut(cd, bad + [s, both], ix, first, flat).check()
    assert rc.got["status"] == [O.OK, want2, want3, O.OK, want2] and want2 != O.OK != want3
    assert rc.got["streams"][0] != rc.got["streams"][3] and rc.got["result"][3] == 2 and rc.got["result"][6:] == [6, 4]
    scrub = Recut(cd, bad + [s, both], ix, first, flat, ALL).check()
    assert scrub.got["status"][0] != O.OK and scrub.got["result"][3] == 1


def test_unsound_indexes_and_lists_keep_every_guard_and_canary(named):
    names, streams, ix = named
    cd = SB.BlockCodec(0, O.HASH_CRC32C)
    rng = np.random.default_rng(5)
    bad = RC.unsound_indexes(ix, streams, rng)
    assert len(bad) == 13
    ns = len(streams)
    first, cuts = RX.lists([list(range(300, t, 300)) for t in ix["total"]])
    refused = 0
    for k, index in enumerate(bad):
        ne = min(len(index["start"]), len(index["pos"]))
        rc = Recut(cd, streams, index, first, cuts, ALL * (k & 1), caps=[len(s) + 70000 for s in streams], max_slots=1 << 12, stage_cap=1 << 25,
                   max_entries=ne + 64)
        rc.check()                                                      # guards and canaries held inside; every status is the model's
        refused += sum(1 for s in rc.got["status"] if s == O.ERR_BAD_ARG)
    assert refused > 40
    # a sound index under lists filled with anything at all
    for k in range(4):
        nc = int(rng.integers(ns, 4 * ns))
        anyc = [int(v) for v in rng.integers(0, 6000, nc)]
        anyf = sorted(int(v) for v in rng.integers(0, nc + 1, ns + 1))
        Recut(cd, streams, ix, anyf if k < 2 else [int(v) for v in rng.integers(0, nc + 3, ns + 1)], sorted(anyc) if k % 2 else anyc,
              caps=[len(s) + 70000 for s in streams], max_slots=1 << 12, stage_cap=1 << 25, max_entries=len(ix["start"]) + 4096).check()


def test_empty_calls_and_a_batch_that_is_canonical(html):
    cd = SB.BlockCodec(0, O.HASH_CRC32C)
    cd._bind()
    call = N.frame_recut_lib().snp_frame_recut_indexed_batch
    result = Guarded(8, torch.int64)
    assert call(cd.ctx.handle, *[None] * 3, 0, *[None] * 5, 0, None, None, 0, 0, 0, 0, 0, *[None] * 5, *[None] * 5, None, None, result.ptr()) == O.OK
    torch.cuda.synchronize()
    assert result.read() == [0] * 8
    raws = [html[:2500], b"", html[:1000]]
    per = [CM.cuts_of(a, 32, 256)[0] for a in raws]
    streams = [RX.stream_at(a, c) for a, c in zip(raws, per)]
    ix = X.build_index(streams)
    rc = Recut(cd, streams, ix, *RX.lists(per), max_slots=3, stage_cap=5000, max_entries=len(ix["start"]) + 5).check()
    assert rc.got["status"] == [O.OK] * 3 and rc.got["result"] == [0, 0, 0, 0, len(ix["start"]), 3, 0, 0] and RX.same_index(rc.got["index"], ix)
    rc = Recut(cd, [b"", b""], X.build_index([b"", b""]), [0, 0, 0], []).check()            # in_len == 0: the identifier
    assert rc.got["streams"] == [M.STREAM_ID] * 2 and rc.got["result"] == [0, 20, 0, 2, 0, 0, 0, 0]


# ---- 6: launch tiers ----------------------------------------------------------------------------------------------------------------------------------
def test_the_slot_bound_picks_the_tier_of_both_tables_and_changes_nothing(html):
    cd = SB.BlockCodec(0, O.HASH_CRC32C)
    streams, ix, first, cuts = mixed_batch(html)
    exact = Recut(cd, streams, ix, first, cuts).check()
    tiers = [cd.ctx.get_option(getattr(N, o)) for o in ("OPT_COMPRESS_WINDOW_DUAL_MIN_BATCH", "OPT_COMPRESS_WINDOW_GLOBAL_MIN_BATCH",
                                                        "OPT_SMALL_BLOCK_MIN_BATCH", "OPT_COMPRESS_WINDOW_MAX_BATCH")]
    assert tiers[0] == 1536 and tiers[2:] == [4096, 32768]
    for ms in [t - d for t in tiers for d in (1, 0)]:
        rc = Recut(cd, streams, ix, first, cuts, caps=exact.caps, max_slots=ms).check()
        assert np.array_equal(rc.h, exact.h) and rc.got == exact.got, ms


def test_real_rows_and_slots_past_the_decoders_list_threshold(html):
    """4 100 one-byte pieces from 41 streams of 100 one-byte chunks' worth of bytes, kept as 50-byte chunks: 82 dirty rows, 4 100 slots; and back:
    4 100 dirty rows on the decoder's list path, 82 slots."""
    cd = SB.BlockCodec(0, O.HASH_CRC32C)
    raws = [html[b:b + 100] for b in range(41)]
    streams = [K.stream_of(x, 50) for x in raws]
    first, cuts = CM.regular_cuts([100] * 41, 1)
    rc = Recut(cd, streams, X.build_index(streams), first, cuts).check()
    assert rc.got["result"][0] == 4100 >= cd.ctx.get_option(N.OPT_SMALL_BLOCK_MIN_BATCH) and rc.got["result"][3] == 41 and rc.got["result"][7] == 4100
    assert rc.after() == [K.stream_of(x, 1) for x in raws]
    first2, cuts2 = CM.regular_cuts([100] * 41, 50)
    back = Recut(cd, rc.after(), rc.got["index"], first2, cuts2).check()
    assert back.got["result"][0] == 4100 and back.got["result"][7] == 82 and back.after() == streams


# ---- 7: every layout --------------------------------------------------------------------------------------------------------------------------------------
_default = {}


def default_run(html, variant):
    if variant not in _default:
        streams, ix, first, cuts = mixed_batch(html, variant)
        _default[variant] = (streams, ix, first, cuts, Recut(SB.BlockCodec(0, variant), streams, ix, first, cuts, variant=variant).check())
    return _default[variant]


@pytest.mark.parametrize("crc", [0, 1, 2])
@pytest.mark.parametrize("layout", layouts.COMPRESS_LAYOUTS)
def test_every_compress_layout_and_crc_kernel(html, layout, crc):
    for variant in VARIANTS:
        streams, ix, first, cuts, base = default_run(html, variant)
        cd = SB.BlockCodec(0, variant)
        layouts.set_compress_layout(cd.ctx, layout)
        cd.ctx.set_option(N.OPT_CRC_KERNEL, crc)
        rc = Recut(cd, streams, ix, first, cuts, caps=base.caps, max_slots=base.ms, stage_cap=base.sc, max_entries=base.me, variant=variant, model=False)
        rc.want = base.want
        rc.check()
        assert np.array_equal(rc.h, base.h)


@pytest.mark.parametrize("fenced", [0, 1])
@pytest.mark.parametrize("decode", layouts.DECODE_LAYOUTS)
def test_every_decode_layout(html, decode, fenced):
    streams, ix, first, cuts, base = default_run(html, O.HASH_CRC32C)
    cd = SB.BlockCodec(0, O.HASH_CRC32C)
    layouts.set_decode_layout(cd.ctx, decode, fenced)
    rc = Recut(cd, streams, ix, first, cuts, caps=base.caps, max_slots=base.ms, stage_cap=base.sc, max_entries=base.me, model=False)
    rc.want = base.want
    rc.check()
    assert np.array_equal(rc.h, base.h)


# ---- 8: past 4 GiB -----------------------------------------------------------------------------------------------------------------------------------------
def test_a_kept_chunk_past_position_2_to_the_32_of_both_streams(html):
    """One stream of 66 000 uncompressed chunks of 65 536 bytes -- clean rows that are copied, 4.03 GiB of them -- then two chunks that make one
    piece, which is rebuilt, and a last chunk that is a piece already: kept, behind position 2^32 of the old and of the new stream."""
    cb, nkept = 65536, 66000
    free = torch.cuda.mem_get_info()[0]
    if free < 20 << 30:
        pytest.skip(f"needs 20 GiB of free device memory, {free >> 30} GiB free")
    cd = SB.BlockCodec(0, O.HASH_CRC32C)
    one = M.data_chunk(html[:cb], compressed=False)
    tail_raw = html[100:100 + 1000] + html[5000:5000 + 3000] + html[9000:9000 + 700]
    last = K.chunks_of(tail_raw[4000:], 700)[0]
    tail = M.data_chunk(tail_raw[:1000]) + M.data_chunk(tail_raw[1000:4000]) + last
    kept_bytes = nkept * len(one)
    n = 10 + kept_bytes + len(tail)
    assert 10 + kept_bytes > 1 << 32
    buf = torch.empty(n, dtype=torch.uint8, device="cuda")
    buf[:10] = torch.from_numpy(np.frombuffer(M.STREAM_ID, dtype=np.uint8).copy()).cuda()
    buf[10:10 + kept_bytes].view(nkept, len(one))[:] = torch.from_numpy(np.frombuffer(one, dtype=np.uint8).copy()).cuda()
    buf[10 + kept_bytes:] = torch.from_numpy(np.frombuffer(tail, dtype=np.uint8).copy()).cuda()
    tix = X.build_index([M.STREAM_ID + tail])
    start = torch.cat([torch.arange(nkept, dtype=torch.int64, device="cuda") * cb, H.dev([nkept * cb + v for v in tix["start"]])])
    pos = torch.cat([10 + torch.arange(nkept, dtype=torch.int64, device="cuda") * len(one), H.dev([kept_bytes + p for p in tix["pos"]])])
    total = nkept * cb + len(tail_raw)
    index = SB.FrameIndex(H.dev([0, nkept + 3]), start, pos, H.dev([total]), torch.zeros(1, dtype=torch.int32, device="cuda"))
    cuts = torch.cat([torch.arange(1, nkept + 1, dtype=torch.int64, device="cuda") * cb, H.dev([nkept * cb + 4000])])
    fresh = K.chunks_of(tail_raw[:4000], 4000)[0]
    want_len = 10 + kept_bytes + len(fresh) + len(last)
    cap = 10 + kept_bytes + 8 + 4000 + len(last)
    out = torch.full((cap + 64,), CANARY, dtype=torch.uint8, device="cuda")
    out_len, status, new_ix, result, bound = cd.frame_recut_indexed(buf, H.dev([0]), H.dev([n]), index, H.dev([0, nkept + 1]), cuts, out, H.dev([0]),
                                                                    H.dev([cap]), 2, 4000 + K.stride(4000), nkept + 3, with_bound=True)
    assert status.tolist() == [O.OK] and out_len.tolist() == [want_len] and bound.tolist() == [cap]
    assert result.tolist() == [2, want_len, 4000 + K.stride(4000), 1, nkept + 3, 0, nkept + 1, 1]
    assert torch.equal(out[:10 + kept_bytes], buf[:10 + kept_bytes]) and bool((out[want_len:] == CANARY).all())
    assert out[10 + kept_bytes:want_len].cpu().numpy().tobytes() == fresh + last
    used = nkept + 2
    assert new_ix.first.tolist() == [0, used] and torch.equal(new_ix.start[:nkept + 1], torch.arange(nkept + 1, dtype=torch.int64, device="cuda") * cb)
    assert new_ix.start[nkept + 1:used].tolist() == [nkept * cb + 4000]
    assert torch.equal(new_ix.pos[:nkept], pos[:nkept]) and new_ix.pos[nkept:used].tolist() == [10 + kept_bytes, 10 + kept_bytes + len(fresh)]
    back = torch.empty(len(tail_raw), dtype=torch.uint8, device="cuda")
    rl, rs, _ = cd.frame_read_indexed(out, H.dev([0]), out_len, new_ix, torch.zeros(1, dtype=torch.int32, device="cuda"), H.dev([nkept * cb]),
                                      H.dev([len(tail_raw)]), back, H.dev([0]), H.dev([len(tail_raw)]))
    assert rs.tolist() == [O.OK] and rl.tolist() == [len(tail_raw)] and back.cpu().numpy().tobytes() == tail_raw

"""snp_frame_splice_indexed_batch (BlockCodec.frame_splice_indexed / frame_splice_to_memory): every new stream, status, length, size bound, index
array and d_result against the model (frame_splice_model.py), with canary bytes around every output range, guard words around every array and
the workspace, and the inputs compared with their copies after the call (splice_harness.Spliced); the named splices at the seam chunk sizes;
foreign streams and mixed batches; the new index against snp_frame_index_batch and under the read, update, append and splice calls; sequences
of splices without synchronisation; graph capture; admission; corruption; unsound indexes; empty calls; the launch tiers of the compressor and
the decoder by bound and by real count; a hole past position 2^32.  Needs an MI355X."""
import numpy as np
import pytest
import torch

import frame_buffers_helpers as H
import frame_buffers_model as M
import frame_chunked_model as K
import frame_index_model as X
import frame_range_model as R
import frame_splice_model as S
import oracle as O
import seekable_cases as SC
from append_harness import arena_of
from conftest import read_testdata
from seekable_harness import CANARY, Guarded, index_call, index_tensors
from splice_harness import Spliced, new_table

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from snappier_amd import batch as SB, _native as N

VARIANTS = [O.HASH_CRC32C, O.HASH_MUL]


@pytest.fixture(scope="module")
def html():
    return read_testdata("html") * 5


@pytest.fixture(scope="module")
def named():
    cases = X.named_streams()
    streams = list(cases.values())
    return list(cases), streams, X.build_index(streams)


def named_batch(html, cb, variant):
    """One stream of at most 5 chunks of cb bytes per named case: -> (names, raws, streams, reqs, srcs)."""
    cases = S.named_cases(cb)
    raws = [html[7 + i:7 + i + n] for i, (n, _, _, _) in enumerate(cases.values())]
    streams = [K.stream_of(a, cb, variant) if a else b"" for a in raws]
    reqs = [(off, dele) for _, off, dele, _ in cases.values()]
    srcs = [html[3001 + 5 * i:3001 + 5 * i + ins] for i, (_, _, _, ins) in enumerate(cases.values())]
    return list(cases), raws, streams, reqs, srcs


def device_index(ix, ns):
    index = SB.FrameIndex(*index_tensors(ix, ns)[0])
    index.start, index.pos = index.start[:len(ix["start"])], index.pos[:len(ix["pos"])]
    return index


# ---- 1: the named splices at every seam chunk size; the new index is the walk's ---------------------------------------------------------------------
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("cb", S.CHUNK_SIZES)
def test_named_splices_are_the_models_byte_for_byte(html, cb, variant):
    cd = SB.BlockCodec(0, variant)
    names, raws, streams, reqs, srcs = named_batch(html, cb, variant)
    ix = X.build_index(streams)
    sp = Spliced(cd, streams, ix, reqs, srcs, cb, variant=variant).check()
    assert set(sp.got["status"]) == {O.OK}
    for b, name in enumerate(names):
        if sp.got["streams"][b] is not None:
            assert O.frame_decode(sp.got["streams"][b]) == S.edited(raws[b], reqs[b][0], reqs[b][1], srcs[b]), name
    assert sp.got["result"][3] == sum(1 for r, s in zip(reqs, srcs) if r[1] or s) >= len(names) - 4
    walked = index_call(cd, sp.after())
    assert walked == {**sp.got["index"], "result": X.build_index(sp.after())["result"]}
    # a truncate and a delete to the end with an insert: the chunked encoder's own bytes
    for name in ("truncate_mid_chunk", "delete_everything_and_insert"):
        b = names.index(name)
        assert sp.got["streams"][b] == K.stream_of(raws[b][:reqs[b][0]] + srcs[b], cb, variant), name


def test_an_incompressible_edge_and_a_stream_written_with_larger_chunks(html):
    cd = SB.BlockCodec(0, O.HASH_CRC32C)
    rnd = bytes(np.random.default_rng(3).integers(0, 256, 3 * 4096, dtype=np.uint8))
    a = html[:2 * 65536 + 1000]
    streams = [K.stream_of(rnd, 4096), K.stream_of(a, 65536)]
    assert streams[0][10] == 1
    reqs, srcs = [(100, 5000), (70000, 10)], [html[:33], html[:4096 + 5]]
    sp = Spliced(cd, streams, X.build_index(streams), reqs, srcs, 4096).check()
    assert sp.got["status"] == [O.OK, O.OK]
    assert [O.frame_decode(x) for x in sp.got["streams"]] == [S.edited(rnd, 100, 5000, srcs[0]), S.edited(a, 70000, 10, srcs[1])]
    assert index_call(cd, sp.after())["pos"] == sp.got["index"]["pos"]


# ---- 2: foreign streams; a mixed batch -----------------------------------------------------------------------------------------------------------------
def test_foreign_streams_drop_what_lies_in_the_hole(html):
    cd = SB.BlockCodec(0, O.HASH_CRC32C)
    cases = S.foreign_streams(html)
    streams = [c[0] for c in cases.values()]
    reqs = [(c[2][0], c[2][1]) for c in cases.values()]
    srcs = [html[4000:4000 + c[2][2]] for c in cases.values()]
    for cb in (64, 65536):
        sp = Spliced(cd, streams, X.build_index(streams), reqs, srcs, cb).check()
        assert sp.got["status"] == [O.OK] * len(streams)
        for b, (name, (s, raw, (off, dele, _), _)) in enumerate(cases.items()):
            assert O.frame_decode(sp.got["streams"][b]) == S.edited(raw, off, dele, srcs[b]), name
        assert index_call(cd, sp.after()) == {**sp.got["index"], "result": X.build_index(sp.after())["result"]}


def middle_splices(ix, ns):
    out = []
    for b in range(ns):
        t = ix["total"][b]
        out.append((t // 2, min(t - t // 2, 300 + 7 * b), 100 + b))
    return out


def test_named_foreign_streams(html, named):
    names, streams, ix = named
    cd = SB.BlockCodec(0, O.HASH_CRC32C)
    reqs3 = middle_splices(ix, len(streams))
    srcs = [html[b:b + r[2]] for b, r in enumerate(reqs3)]
    sp = Spliced(cd, streams, ix, [r[:2] for r in reqs3], srcs, 4096).check()
    written = sum(1 for x in sp.got["streams"] if x is not None)
    assert written >= 10 and len(set(sp.got["status"])) >= 3          # (the floor the model meets on the CPU)
    assert index_call(cd, sp.after()) == {**sp.got["index"], "result": X.build_index(sp.after())["result"]}


def test_a_mixed_batch_written_refused_broken_and_unnamed(html, named):
    names, streams, ix = named
    cd = SB.BlockCodec(0, O.HASH_MUL)
    cb = 512
    mine = [K.stream_of(html[:n], cb, O.HASH_MUL) for n in (700, 1024, 1300, 100)] + [b""]
    broken = [s for s, t in zip(streams, ix["tail"]) if t != O.OK][:3]
    batch = [mine[0], broken[0], mine[1], mine[2], broken[1], mine[3], mine[4], broken[2]]
    reqs = [(100, 50), (0, 1), (512, 512), (600, 0), (0, 0), (5, 0), (0, 0), (3, 0)]
    srcs = [html[3000:3000 + n] for n in (1000, 50, 0, 100, 0, 0, 2000, 7)]
    bix = X.build_index(batch)
    free = S.splice_plan(batch, bix, reqs, srcs, cb, variant=O.HASH_MUL)
    caps = list(free["out_bound"])
    caps[3] = free["out_len"][3] - 1                                    # refused: its range is one byte short
    sp = Spliced(cd, batch, bix, reqs, srcs, cb, caps=caps, variant=O.HASH_MUL).check()
    assert sp.got["status"] == [O.OK, bix["tail"][1], O.OK, O.ERR_OUTPUT_TOO_SMALL, O.OK, O.OK, O.OK, bix["tail"][7]]
    assert [x is not None for x in sp.got["streams"]] == [True, False, True, False, False, False, True, False]
    assert index_call(cd, sp.after())["pos"] == sp.got["index"]["pos"]


# ---- 3: the new index under the sibling calls --------------------------------------------------------------------------------------------------------------
def test_the_new_index_serves_the_read_update_append_and_a_second_splice(html):
    cd = SB.BlockCodec(0, O.HASH_CRC32C)
    cb = 4096
    raws = [html[:3 * cb + 100], html[5:5 + cb], html[9:9 + 5 * cb]]
    reqs, srcs = [(cb + 7, 2 * cb), (cb, 0), (0, 2 * cb + 1)], [html[30000:30000 + 50], html[9:9 + 3 * cb + 1], b""]
    streams = [K.stream_of(x, cb) for x in raws]
    sp = Spliced(cd, streams, X.build_index(streams), reqs, srcs, cb).check()
    now = [S.edited(x, r[0], r[1], s) for x, r, s in zip(raws, reqs, srcs)]
    framed, off, lens = new_table(sp)
    index = sp.frame_index()
    ns = len(now)
    stream_no = torch.arange(ns, dtype=torch.int32, device="cuda")
    # read: every stream whole
    out, out_off, out_len, status = cd.frame_gather_to_memory(framed, off, lens, index, stream_no, H.dev([0] * ns), H.dev([len(x) for x in now]))
    assert status.tolist() == [O.OK] * ns and out_len.tolist() == [len(x) for x in now]
    h = out.cpu().numpy()
    assert [h[o:o + n].tobytes() for o, n in zip(out_off.tolist(), out_len.tolist())] == now
    # update: ten bytes across the front seam of every splice
    ureq = [(b, max(r[0] - 5, 0), 10) for b, r in enumerate(reqs)]
    data = [bytes([65 + b]) * 10 for b in range(ns)]
    src, src_off, src_len = H.pack(data)
    uout, uoff, ulen, ust, ureq_st, _ = cd.frame_update_to_memory(framed, off, lens, index, stream_no, H.dev([q[1] for q in ureq]), src, H.dev(src_off),
                                                                   H.dev(src_len))
    assert ust.tolist() == [O.OK] * ns and ureq_st.tolist() == [O.OK] * ns
    h = uout.cpu().numpy()
    for b, (_, o, ln) in enumerate(ureq):
        assert O.frame_decode(h[int(uoff[b]):int(uoff[b]) + int(ulen[b])].tobytes()) == now[b][:o] + data[b] + now[b][o + ln:], b
    # append, in place in an arena of its own
    more = [html[777:777 + n] for n in (cb + 3, 1, 2 * cb)]
    caps = [len(s) + len(m) + 64 for s, m in zip(sp.after(), more)]
    buf, boff = arena_of(sp.after(), caps)
    asrc, asrc_off, asrc_len = H.pack(more)
    new_len, ast, aix = cd.frame_append_to_memory(buf, H.dev(boff), lens, H.dev(caps), index, asrc, H.dev(asrc_off), H.dev(asrc_len), cb)
    assert ast.tolist() == [O.OK] * ns
    h = buf.cpu().numpy()
    grown = [h[o:o + n].tobytes() for o, n in zip(boff, new_len.tolist())]
    assert [O.frame_decode(x) for x in grown] == [x + m for x, m in zip(now, more)]
    assert X.build_index(grown)["pos"] == aix.pos[:int(aix.first[-1])].tolist()
    # a second splice, through the wrapper that sizes it
    again = [(5, 10), (len(now[1]), 0), (cb // 2, cb)]
    ins = [b"", html[:99], html[50:50 + 2 * cb]]
    isrc, isrc_off, isrc_len = H.pack(ins)
    out2, off2, len2, st2, ix2 = cd.frame_splice_to_memory(framed, off, lens, index, H.dev([q[0] for q in again]), H.dev([q[1] for q in again]), isrc,
                                                           H.dev(isrc_off), H.dev(isrc_len), cb)
    assert st2.tolist() == [O.OK] * ns
    h = out2.cpu().numpy()
    second = [h[o:o + n].tobytes() for o, n in zip(off2.tolist(), len2.tolist())]
    assert [O.frame_decode(x) for x in second] == [S.edited(x, q[0], q[1], s) for x, q, s in zip(now, again, ins)]
    want = S.splice_plan(sp.after(), sp.got["index"], again, ins, cb)
    assert second == want["streams"] and ix2.first.tolist() == want["index"]["first"]
    used = want["index"]["first"][-1]
    assert ix2.start[:used].tolist() == want["index"]["start"] and ix2.pos[:used].tolist() == want["index"]["pos"] and ix2.total.tolist() == want["index"]["total"]


# ---- 4: five splices on one context, no synchronisation between them ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("cb", [100, 65536])
def test_five_splices_in_a_row(html, cb):
    cd = SB.BlockCodec(0, O.HASH_CRC32C)
    raws = [html[:2 * cb + cb // 3], html[3:3 + cb], html[:4 * cb]]
    streams = [K.stream_of(x, cb) for x in raws]
    ix = X.build_index(streams)
    steps = [[(cb // 2, 0, cb + 1), (0, cb // 2, 0), (cb, 2 * cb, 5)], [(0, 10, 0), (1, 0, 3 * cb), (7, 0, 1)], [(cb, cb // 2, cb // 2), (cb, cb, 0), (0, cb, cb)],
             [(3, 0, 2), (0, 0, 9), (cb + 9, 1, 0)], [(20, cb, 0), (5, cb, 7), (1, cb - 1, 2 * cb)]]
    # the model runs ahead, so that every call is sized without reading anything back
    plans, ms, mix = [], streams, ix
    for k, step in enumerate(steps):
        srcs = [html[1000 * k + 17 * b:1000 * k + 17 * b + q[2]] for b, q in enumerate(step)]
        w = S.splice_plan(ms, mix, [q[:2] for q in step], srcs, cb)
        assert w["status"] == [O.OK] * 3
        plans.append((step, srcs, w))
        raws = [S.edited(x, q[0], q[1], s) for x, q, s in zip(raws, step, srcs)]
        ms, mix = w["streams"], w["index"]
    framed, in_off, in_len = H.pack(streams)
    in_off, in_len = H.dev(in_off), H.dev(in_len)
    index = device_index(ix, 3)
    keep = []
    for step, srcs, w in plans:
        src, src_off, src_len = H.pack(srcs)
        out_off, total = H.out_layout(np.array(w["out_bound"], dtype=np.int64))
        out = torch.full((total,), CANARY, dtype=torch.uint8, device="cuda")
        keep += [src, framed]
        out_len, status, index, _ = cd.frame_splice_indexed(framed, in_off, in_len, index, H.dev([q[0] for q in step]), H.dev([q[1] for q in step]), src,
                                                           H.dev(src_off), H.dev(src_len), cb, out, H.dev(out_off), H.dev(w["out_bound"]),
                                                           w["result"][0], w["result"][2])
        framed, in_off, in_len = out, H.dev(out_off), out_len
    torch.cuda.synchronize()
    assert status.tolist() == [O.OK] * 3 and in_len.tolist() == [len(x) for x in ms]
    h = framed.cpu().numpy()
    got = [h[o:o + n].tobytes() for o, n in zip(in_off.tolist(), in_len.tolist())]
    assert got == ms and [O.frame_decode(x) for x in got] == raws
    assert (H.outside_ranges(h, in_off.tolist(), in_len.tolist()) == CANARY).all()
    after = X.build_index(got)
    used = after["first"][-1]
    assert index.first.tolist() == after["first"] and index.start[:used].tolist() == after["start"] and index.pos[:used].tolist() == after["pos"]
    assert index.total.tolist() == after["total"] and index.tail.tolist() == after["tail"]


# ---- 5: graph capture ------------------------------------------------------------------------------------------------------------------------------------------
def test_graph_capture_replays_the_call(html):
    cd = SB.BlockCodec(0, O.HASH_CRC32C)
    cb = 4096
    raws = [html[:3 * cb + 700], html[11:11 + cb], b"", html[5:5 + 9000]]
    reqs, srcs = [(cb + 5, cb), (0, 100), (0, 0), (0, 0)], [html[40000:40000 + 2 * cb + 3], b"", html[7:7 + cb], b""]
    streams = [K.stream_of(x, cb) if x else b"" for x in raws]
    ix = X.build_index(streams)
    want = S.splice_plan(streams, ix, reqs, srcs, cb)
    ms, sc = want["result"][0], want["result"][2]
    framed, in_off, in_len = H.pack(streams)
    out_off, total = H.out_layout(np.array(want["out_bound"], dtype=np.int64))
    out = torch.full((total,), CANARY, dtype=torch.uint8, device="cuda")
    index = device_index(ix, 4)
    src, src_off, src_len = H.pack(srcs)
    tabs = [H.dev(in_off), H.dev(in_len), H.dev([q[0] for q in reqs]), H.dev([q[1] for q in reqs]), H.dev(src_off), H.dev(src_len), H.dev(out_off),
            H.dev(want["out_bound"])]
    work = torch.empty(N.frame_splice_lib().snp_frame_splice_indexed_workspace(4, ms, sc, cb), dtype=torch.uint8, device="cuda")

    def call():
        return cd.frame_splice_indexed(framed, tabs[0], tabs[1], index, tabs[2], tabs[3], src, tabs[4], tabs[5], cb, out, tabs[6], tabs[7], ms, sc, work=work)

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
    out.fill_(CANARY)
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


# ---- 6: admission; corruption; the index is untrusted; empty calls ------------------------------------------------------------------------------------------
def test_admission_by_each_bound_and_by_out_cap(html):
    cd = SB.BlockCodec(0, O.HASH_CRC32C)
    cb = 512
    streams = [K.stream_of(x, cb) for x in (html[:700], html[50:50 + 1024], html[9:9 + 1300], html[:100], html[:2000])]
    ix = X.build_index(streams)
    reqs = [(100, 50), (512, 512), (600, 0), (5, 0), (1000, 1000)]
    srcs = [html[3000:3000 + n] for n in (1000, 0, 100, 0, 2000)]
    full = Spliced(cd, streams, ix, reqs, srcs, cb).check()
    assert full.got["status"] == [O.OK] * 5
    sizing = Spliced(cd, streams, ix, reqs, srcs, cb, caps=[0] * 5, max_slots=0, stage_cap=0).check()
    slots, _, stage, _ = sizing.got["result"]
    assert (slots, stage) == (10, 6098) and sizing.got["streams"] == [None] * 5 and sizing.got["out_bound"] == full.got["out_bound"]
    assert all(bd >= n for bd, n in zip(sizing.got["out_bound"], full.got["out_len"]))
    short = Spliced(cd, streams, ix, reqs, srcs, cb, max_slots=slots - 1).check()
    assert short.got["status"] == [O.OK, O.OK, O.OK, O.OK, O.ERR_OUTPUT_TOO_SMALL]
    short = Spliced(cd, streams, ix, reqs, srcs, cb, stage_cap=1974 + 1123).check()
    assert short.got["status"] == [O.OK, O.OK, O.ERR_OUTPUT_TOO_SMALL, O.OK, O.ERR_OUTPUT_TOO_SMALL]
    caps = list(full.got["out_len"])
    caps[2] -= 1                                                        # one byte short, in the middle of the batch
    mid = Spliced(cd, streams, ix, reqs, srcs, cb, caps=caps).check()
    assert mid.got["status"] == [O.OK, O.OK, O.ERR_OUTPUT_TOO_SMALL, O.OK, O.OK] and mid.got["result"][3] == 3


def test_corruption_in_an_edge_in_a_deleted_chunk_and_outside_the_hole(html):
    cd = SB.BlockCodec(0, O.HASH_CRC32C)
    cb = 4096
    s = K.stream_of(html[:5 * cb], cb)
    rows = R.walk(s)[0]
    bad = [R.corrupt_chunk(s, rows[i]) for i in (1, 2, 3, 4)]
    both = R.corrupt_chunk(bad[0], rows[3])
    want1, want3 = M.chunk_status(bad[0], rows[1]), M.chunk_status(bad[2], rows[3])
    sp = Spliced(cd, bad + [s, both], X.build_index([s] * 6), [(cb + 100, 2 * cb)] * 6, [html[9000:9050]] * 6, cb).check()
    assert sp.got["status"] == [want1, O.OK, want3, O.OK, O.OK, want1] and want1 != O.OK != want3
    assert sp.got["streams"][1] == sp.got["streams"][4] and sp.got["streams"][3] != sp.got["streams"][4] and sp.got["result"][3] == 3


def test_unsound_indexes_keep_every_guard_and_canary(html, named):
    names, streams, ix = named
    cd = SB.BlockCodec(0, O.HASH_CRC32C)
    rng = np.random.default_rng(5)
    reqs3 = middle_splices(ix, len(streams))
    srcs = [html[b:b + r[2]] for b, r in enumerate(reqs3)]
    reqs = [r[:2] for r in reqs3]
    ns = len(streams)
    bad = S.unsound_indexes(ix, streams, rng)
    assert len(bad) == 13
    refused = 0
    for index in bad:
        sp = Spliced(cd, streams, index, reqs, srcs, 4096, caps=[len(s) + 70000 for s in streams], max_slots=3 * ns, stage_cap=1 << 24)
        sp.check()                                                      # guards and canaries held inside; every status is the model's
        refused += sum(1 for s in sp.got["status"] if s == O.ERR_BAD_ARG)
    assert refused > 40


def test_empty_calls_and_streams_that_are_not_named(html):
    cd = SB.BlockCodec(0, O.HASH_CRC32C)
    cd._bind()
    call = N.frame_splice_lib().snp_frame_splice_indexed_batch
    result = Guarded(4, torch.int64)
    assert call(cd.ctx.handle, *[None] * 3, 0, *[None] * 5, 0, *[None] * 5, 4096, 0, 0, *[None] * 5, *[None] * 5, None, None, result.ptr()) == O.OK
    torch.cuda.synchronize()
    assert result.read() == [0, 0, 0, 0]
    streams = [K.stream_of(html[:n], 1000) for n in (2500, 0, 1000)]
    ix = X.build_index(streams)
    sp = Spliced(cd, streams, ix, [(5, 0)] * 3, [b""] * 3, 1000, max_slots=3, stage_cap=5000).check()
    assert sp.got["status"] == [O.OK] * 3 and sp.got["result"] == [0, 0, 0, 0] and S.same_index(sp.got["index"], ix)
    # ... whatever the index holds: nothing of it is trusted for a stream that is not named
    sp = Spliced(cd, streams, {**ix, "tail": [5, 77, -3]}, [(1 << 63, 0)] * 3, [b""] * 3, 1000, max_slots=0, stage_cap=0).check()
    assert sp.got["status"] == [O.OK] * 3 and sp.got["index"]["tail"] == [5, 77, -3]


# ---- 7: launch tiers ---------------------------------------------------------------------------------------------------------------------------------------------
def test_the_slot_bound_picks_the_compressors_tier_and_changes_nothing(html):
    cd = SB.BlockCodec(0, O.HASH_CRC32C)
    cb = 1000
    raws = [html[:2 * cb + 300], html[7:7 + cb], b"", html[3:3 + 10], html[:5 * cb]]
    reqs, srcs = [(cb + 1, cb), (0, 0), (0, 0), (2, 3), (cb // 2, 3 * cb)], [html[20000:20000 + 2 * cb], html[:cb // 2], html[9:9 + 3 * cb + 1], b"", html[100:100 + cb]]
    streams = [K.stream_of(x, cb) if x else b"" for x in raws]
    ix = X.build_index(streams)
    exact = Spliced(cd, streams, ix, reqs, srcs, cb).check()
    compress = [cd.ctx.get_option(getattr(N, o)) for o in ("OPT_COMPRESS_WINDOW_DUAL_MIN_BATCH", "OPT_COMPRESS_WINDOW_MAX_BATCH")]
    assert compress == [1536, 32768]
    rows = len(ix["start"])
    for ms in [t - d for t in compress for d in (1, 0)]:
        sp = Spliced(cd, streams, ix, reqs, srcs, cb, caps=exact.caps, max_slots=ms).check()
        assert np.array_equal(sp.h, exact.h) and sp.got == exact.got, ms
        assert sp.new[1].n == rows + ms


@pytest.mark.parametrize("ns", [2047, 2048])
def test_the_edge_table_crosses_the_decoders_list_threshold(html, ns):
    """The edge table holds 2 x nstreams rows, an even number: 4 094 rows lie below the decoder's threshold of 4 096 and 4 096 rows on it.  Five
    streams do real work, the rest are not named."""
    cd = SB.BlockCodec(0, O.HASH_CRC32C)
    assert cd.ctx.get_option(N.OPT_SMALL_BLOCK_MIN_BATCH) == 4096
    cb = 64
    one = K.stream_of(html[:3 * cb + 9], cb)
    streams = [one] * ns
    busy = {0: (10, 100, 7), 1: (cb, 0, 5), ns // 2: (70, 0, 200), ns - 2: (0, 3 * cb + 9, 1), ns - 1: (cb + 1, 2, 0)}
    reqs = [busy.get(b, (0, 0, 0))[:2] for b in range(ns)]
    srcs = [html[500 + b:500 + b + busy.get(b, (0, 0, 0))[2]] for b in range(ns)]
    ix = X.build_index([one])
    rows = len(ix["start"])
    batch_ix = dict(first=[rows * b for b in range(ns + 1)], start=ix["start"] * ns, pos=ix["pos"] * ns, total=ix["total"] * ns, tail=ix["tail"] * ns)
    sp = Spliced(cd, streams, batch_ix, reqs, srcs, cb).check()
    assert sp.got["result"][3] == 5 and sp.got["status"] == [O.OK] * ns


def test_real_slots_on_the_lane_compressor(html):
    """33 000 new chunks of one byte: past the window compressor's range."""
    cd = SB.BlockCodec(0, O.HASH_CRC32C)
    cb, ns, per = 1, 33, 1000
    raws = [html[b:b + 3 + b % 4] for b in range(ns)]
    streams = [K.stream_of(x, cb) for x in raws]
    reqs = [(b % 3, 0) for b in range(ns)]
    srcs = [html[1000 + 7 * b:1000 + 7 * b + per] for b in range(ns)]
    sp = Spliced(cd, streams, X.build_index(streams), reqs, srcs, cb).check()
    assert sp.got["result"][0] == 33000 >= cd.ctx.get_option(N.OPT_COMPRESS_WINDOW_MAX_BATCH) and sp.got["result"][3] == ns
    assert sp.after() == [K.stream_of(S.edited(x, r[0], 0, s), cb) for x, r, s in zip(raws, reqs, srcs)]


def test_real_edges_on_the_decoders_list_path(html):
    """2 100 streams with two real edges each: 4 200 rows to decode."""
    cd = SB.BlockCodec(0, O.HASH_CRC32C)
    cb, ns = 64, 2100
    raws = [html[b:b + 3 * cb + b % 50] for b in range(ns)]
    streams = [K.stream_of(x, cb) for x in raws]
    reqs = [(10 + b % 40, 2 * cb) for b in range(ns)]                   # from inside chunk 0 to inside chunk 2
    srcs = [html[5 * b:5 * b + b % 3] for b in range(ns)]
    sp = Spliced(cd, streams, X.build_index(streams), reqs, srcs, cb).check()
    assert sp.got["result"][3] == ns and sp.got["result"][2] >= 2 * cb * ns and 2 * ns >= cd.ctx.get_option(N.OPT_SMALL_BLOCK_MIN_BATCH)
    assert [O.frame_decode(x) for x in sp.after()[::97]] == [S.edited(x, r[0], r[1], s) for x, r, s in list(zip(raws, reqs, srcs))[::97]]


# ---- 8: past 4 GiB ---------------------------------------------------------------------------------------------------------------------------------------------------
def test_a_hole_past_position_2_to_the_32(html):
    cb, pad = 65536, (1 << 24) - 1
    npad = -(-((1 << 32) + 200_000 - 10) // (pad + 4))
    p0 = 10 + npad * (pad + 4)
    free = torch.cuda.mem_get_info()[0]
    if free < 20 << 30:
        pytest.skip(f"needs 20 GiB of free device memory, {free >> 30} GiB free")
    cd = SB.BlockCodec(0, O.HASH_CRC32C)
    old = html[:3 * cb + 30000]
    src = html[70000:170000]
    small = K.stream_of(old, cb)                                        # the data chunks alone: the same chunks behind the identifier
    six = X.build_index([small])
    req = (cb + 500, cb)                                                # from inside chunk 1 to inside chunk 2
    want = S.splice_plan([small], six, [req], [src], cb)
    assert want["status"] == [O.OK]
    delta = p0 - 10
    n = delta + len(small)
    buf = torch.zeros(n, dtype=torch.uint8, device="cuda")               # the bodies of the padding chunks are never looked at
    buf[:10] = torch.from_numpy(np.frombuffer(M.STREAM_ID, dtype=np.uint8).copy()).cuda()
    head = torch.from_numpy(np.frombuffer(bytes([0xFE]) + pad.to_bytes(3, "little"), dtype=np.uint8).copy()).cuda()
    for k in range(npad):
        buf[10 + k * (pad + 4):14 + k * (pad + 4)] = head
    buf[16 + 3 * (pad + 4)] = 77                                        # a byte in a padding body, to see the copy
    buf[p0:n] = torch.from_numpy(np.frombuffer(small[10:], dtype=np.uint8).copy()).cuda()
    index = SB.FrameIndex(H.dev(six["first"]), H.dev(six["start"]), H.dev([p + delta for p in six["pos"]]), H.dev(six["total"]),
                          torch.tensor(six["tail"], dtype=torch.int32, device="cuda"))
    cap = want["out_bound"][0] + delta
    out = torch.full((cap + 64,), CANARY, dtype=torch.uint8, device="cuda")
    data = torch.from_numpy(np.frombuffer(src, dtype=np.uint8).copy()).cuda()
    out_len, status, new_ix, result, bound = cd.frame_splice_indexed(buf, H.dev([0]), H.dev([n]), index, H.dev([req[0]]), H.dev([req[1]]), data, H.dev([0]),
                                                                     H.dev([len(src)]), cb, out, H.dev([0]), H.dev([cap]), want["result"][0],
                                                                     want["result"][2], with_bound=True)
    assert status.tolist() == [O.OK] and out_len.tolist() == [want["out_len"][0] + delta] and bound.tolist() == [cap]
    assert result.tolist() == [want["result"][0], want["out_len"][0] + delta, want["result"][2], 1]
    h0, h1 = want["hole"][0]
    assert h0 + delta > 1 << 32
    end = want["out_len"][0] + delta
    assert torch.equal(out[:h0 + delta], buf[:h0 + delta]) and bool((out[end:] == CANARY).all())
    assert out[h0 + delta:end].cpu().numpy().tobytes() == want["streams"][0][h0:]
    used = want["index"]["first"][-1]
    assert new_ix.first.tolist() == want["index"]["first"] and new_ix.pos[:used].tolist() == [p + delta for p in want["index"]["pos"]]
    assert new_ix.start[:used].tolist() == want["index"]["start"] and new_ix.total.tolist() == want["index"]["total"]
    # the inserted bytes, past position 2^32 of the new stream, read back through the new index
    back = torch.empty(len(src), dtype=torch.uint8, device="cuda")
    rl, rs, _ = cd.frame_read_indexed(out, H.dev([0]), out_len, new_ix, torch.zeros(1, dtype=torch.int32, device="cuda"), H.dev([req[0]]),
                                      H.dev([len(src)]), back, H.dev([0]), H.dev([len(src)]))
    assert rs.tolist() == [O.OK] and rl.tolist() == [len(src)] and torch.equal(back, data)


# ---- rebuilt chunks stored compressed and stored raw, at the chunk sizes whose emit teams are 64, 128 and 256 threads --------------------------------
@pytest.mark.parametrize("cb", SC.TEAM_CHUNK_SIZES)
def test_rebuilt_chunks_raw_and_compressed_at_every_team_size(cb):
    cd = SB.BlockCodec(0, O.HASH_CRC32C)
    blobs = SC.team_blobs(cb)
    streams = [K.stream_of(x, cb) for x in blobs]
    reqs = [(cb - 3, 10)] * 3                                           # a hole across the first chunk boundary: a head and a tail edge
    srcs = [x[5:5 + cb + 5] for x in blobs]                             # each stream's own kind of bytes
    sp = Spliced(cd, streams, X.build_index(streams), reqs, srcs, cb).check()
    assert sp.got["status"] == [O.OK] * 3 and sp.got["result"][3] == 3
    assert [O.frame_decode(s) for s in sp.got["streams"]] == [S.edited(x, off, dele, src) for x, (off, dele), src in zip(blobs, reqs, srcs)]
    assert [SC.chunk_types(s) for s in sp.got["streams"][:2]] == [{1}, {0}]

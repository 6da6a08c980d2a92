"""snp_frame_edit_indexed_batch (BlockCodec.frame_edit_indexed / frame_edit_to_memory / frame_replace_streams): every new stream, status, edit
status, length, size bound, index array and d_result against the model (frame_edit_model.py), with canary bytes around every output range,
guard words around every array and the workspace, and the inputs compared with their copies after the call (edit_harness.Edited); the directed
edit scripts at the seam chunk sizes; groups with more edits than a workgroup has threads and with a region across assemble units; foreign
streams; one edit per stream against the splice call on the device; every refusal; the new index against snp_frame_index_batch and under the
read, the splice and a second edit without synchronisation; graph capture; the launch tiers of the decoder and the compressor; replace against
bytes.replace.  Needs an MI355X."""
import numpy as np
import pytest
import torch

import frame_buffers_helpers as H
import frame_buffers_model as M
import frame_chunked_model as K
import frame_edit_model as E
import frame_index_model as X
import frame_range_model as R
import frame_splice_model as S
import oracle as O
from conftest import read_testdata
from edit_harness import Edited
from seekable_harness import CANARY, Guarded, index_call, index_tensors
from splice_harness import Spliced

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


def device_index(ix, ns):
    index = SB.FrameIndex(*index_tensors(ix, ns)[0])
    index.start, index.pos = index.start[:len(ix["start"])], index.pos[:len(ix["pos"])]
    return index


def walked_is(cd, ed):
    """The new index is what snp_frame_index_batch gives for the batch after the call."""
    assert index_call(cd, ed.after()) == {**ed.got["index"], "result": X.build_index(ed.after())["result"]}


# ---- 1: the directed scripts at every seam chunk size ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("cb", S.CHUNK_SIZES)
def test_directed_scripts_are_the_models_byte_for_byte(html, cb, variant):
    cd = SB.BlockCodec(0, variant)
    names, raws, streams, scripts = E.scripts_batch(html, cb, variant)
    ed = Edited(cd, streams, X.build_index(streams), scripts, cb, variant=variant).check()
    assert set(ed.got["status"]) == {O.OK} and set(ed.got["ed_status"]) == {O.OK}
    for b, name in enumerate(names):
        if ed.got["streams"][b] is not None:
            assert O.frame_decode(ed.got["streams"][b]) == E.applied(raws[b], scripts[b]), name
    named = [any(d or x for _, d, x in sc) for sc in scripts]       # a script with no edit, or skipped ones only, is not named
    assert [x is not None for x in ed.got["streams"]] == named and ed.got["result"][3] == sum(named)
    walked_is(cd, ed)


def test_a_group_with_more_edits_than_a_workgroup_has_threads_and_a_region_across_assemble_units(html):
    cd = SB.BlockCodec(0, O.HASH_CRC32C)
    cb = 4096
    raws = [html[3:3 + 3 * cb + 77], html[9:9 + 2 * cb + 5], html[1:1 + 4 * cb]]
    streams = [K.stream_of(x, cb) for x in raws]
    scripts = [[(cb + 10 + 13 * i, 1, bytes([65 + i % 26])) for i in range(300)],              # 300 one-byte replacements inside chunk 1
               [(cb + 100 + 7 * i, 3, html[50000 + 30000 * i:50000 + 30000 * (i + 1)]) for i in range(5)],    # one group, a region of 150 KB
               [(5 + 3 * i, 1, b"") for i in range(1200)] + [(3 * cb + 9, 0, html[:70000])]]    # 1 200 deletes inside chunk 0, a second group
    ed = Edited(cd, streams, X.build_index(streams), scripts, cb).check()
    assert ed.got["status"] == [O.OK] * 3
    assert [O.frame_decode(x) for x in ed.got["streams"]] == [E.applied(x, sc) for x, sc in zip(raws, scripts)]
    assert [len(h) for h in ed.want["holes"]] == [1, 1, 2]
    assert ed.got["result"][2] == 2 * cb + (2 * cb + 5 * 30000 - 15) + (2 * cb - 1200) + (2 * cb + 70000)     # every edge row once, every region
    walked_is(cd, ed)


# ---- 2: foreign streams, with a second edit behind the splice model's one -------------------------------------------------------------------------------
def test_foreign_streams_non_data_chunks_inside_and_between_holes(html):
    cd = SB.BlockCodec(0, O.HASH_CRC32C)
    cases = S.foreign_streams(html)
    streams = [c[0] for c in cases.values()]
    scripts = []
    for i, (s, raw, (off, dele, ins), _) in enumerate(cases.values()):
        at = min(off + dele + 150, len(raw))
        scripts.append([(off, dele, html[4000:4000 + ins]), (at, min(25, len(raw) - at), html[6000 + i:6006 + i])])
    for cb in (64, 65536):
        ed = Edited(cd, streams, X.build_index(streams), scripts, cb).check()
        assert ed.got["status"] == [O.OK] * len(streams)
        for b, (name, (s, raw, _, _)) in enumerate(cases.items()):
            assert O.frame_decode(ed.got["streams"][b]) == E.applied(raw, scripts[b]), name
        walked_is(cd, ed)


# ---- 3: one edit per stream is the splice -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cb", [1, 65, 4096])
def test_one_edit_per_stream_equals_the_splice_call_in_every_output_array(html, cb):
    cd = SB.BlockCodec(0, O.HASH_CRC32C)
    cases = S.named_cases(cb)
    raws = [html[7 + i:7 + i + n] for i, (n, _, _, _) in enumerate(cases.values())]
    streams = [K.stream_of(a, cb) if a else b"" for a in raws]
    reqs = [(off, dele) for _, off, dele, _ in cases.values()]
    srcs = [html[3001 + 5 * i:3001 + 5 * i + ins] for i, (_, _, _, ins) in enumerate(cases.values())]
    ix = X.build_index(streams)
    sp = Spliced(cd, streams, ix, reqs, srcs, cb).check()
    ed = Edited(cd, streams, ix, [[(r[0], r[1], s)] for r, s in zip(reqs, srcs)], cb).check()
    for key in ("status", "out_len", "streams", "index", "out_bound", "result"):
        assert ed.got[key] == sp.got[key], key
    assert np.array_equal(ed.h, sp.h)                                   # the whole arena, canaries included


# ---- 4: refusals ------------------------------------------------------------------------------------------------------------------------------------------------
def test_edits_out_of_order_overlapping_and_past_the_total_are_refused_with_their_own_status(html):
    cd = SB.BlockCodec(0, O.HASH_CRC32C)
    cb = 1000
    raw = html[:3500]
    s = K.stream_of(raw, cb)
    x = html[9000:9010]
    scripts = [[(100, 10, x), (50, 5, x)],                              # out of order
               [(100, 10, x), (109, 5, x)],                             # overlapping
               [(100, 10, x), (110, 5, x)],                             # touching: legal
               [(100, 10, x), (3490, 11, x)],                           # hi > total
               [(3500, 0, x), (3500, 0, x)],                            # two inserts at total: legal
               [(3501, 0, x)],
               [(200, 0, x), (100, 0, b""), (300, 1, b"")]]             # a skipped edit is not looked at
    ed = Edited(cd, [s] * len(scripts), X.build_index([s] * len(scripts)), scripts, cb).check()
    B = O.ERR_BAD_ARG
    assert ed.got["status"] == [B, B, O.OK, B, O.OK, B, O.OK]
    assert ed.got["ed_status"] == [0, B, 0, B, 0, 0, 0, B, 0, 0, B, 0, 0, 0]
    assert [x is not None for x in ed.got["streams"]] == [False, False, True, False, True, False, True]


def test_a_corrupt_shared_edge_row_refuses_its_stream_once_and_a_corrupt_deleted_chunk_is_not_noticed(html):
    cd = SB.BlockCodec(0, O.HASH_CRC32C)
    cb = 4096
    s = K.stream_of(html[:5 * cb], cb)
    rows = R.walk(s)[0]
    bad = [R.corrupt_chunk(s, rows[i]) for i in (1, 2, 3)]
    both = R.corrupt_chunk(bad[0], rows[3])
    x = html[9000:9050]
    # chunk 1 is shared by two edits (the tail row of the first, the head row of the second), chunk 2 is wholly deleted, chunk 3 a tail row
    script = [(100, cb, x), (cb + 200, 2 * cb, x)]
    streams = bad + [s, both]
    ed = Edited(cd, streams, X.build_index([s] * 5), [script] * 5, cb).check()
    want1, want3 = M.chunk_status(bad[0], rows[1]), M.chunk_status(bad[2], rows[3])
    assert want1 != O.OK != want3
    assert ed.got["status"] == [want1, O.OK, want3, O.OK, want1] and set(ed.got["ed_status"]) == {O.OK}
    assert ed.got["streams"][1] == ed.got["streams"][3] and ed.got["result"][3] == 2
    assert ed.want["result"][2] == 5 * (3 * cb + 100 + 50 + 100 + 50 + cb - 200)           # rows 0, 1 and 3 once each, and the one region


def test_out_cap_short_in_the_middle_and_admission_in_stream_order(html):
    cd = SB.BlockCodec(0, O.HASH_CRC32C)
    cb = 512
    raws = [html[:700], html[50:50 + 1024], html[9:9 + 1300], html[:100], html[:2000]]
    streams = [K.stream_of(x, cb) for x in raws]
    ix = X.build_index(streams)
    scripts = [[(100, 50, html[3000:4000]), (600, 0, html[:9])], [(512, 512, b"")], [(10, 1, b"ab"), (600, 0, html[3000:3100])], [],
               [(1000, 500, html[:2000]), (1500, 500, b"")]]
    full = Edited(cd, streams, ix, scripts, cb).check()
    assert full.got["status"] == [O.OK] * 5
    sizing = Edited(cd, streams, ix, scripts, cb, caps=[0] * 5, max_slots=0, stage_cap=0).check()
    slots, _, stage, _ = sizing.got["result"]
    assert sizing.got["streams"] == [None] * 5 and sizing.got["out_bound"] == full.got["out_bound"] and S.same_index(sizing.got["index"], ix)
    per = [E.needs([s], X.build_index([s]), *E.flat([sc]), cb) for s, sc in zip(streams, scripts)]
    assert (slots, stage) == (sum(p[0] for p in per), sum(p[1] for p in per)) and per[1] == (0, 0)
    short = Edited(cd, streams, ix, scripts, cb, max_slots=slots - 1).check()
    assert short.got["status"] == [O.OK, O.OK, O.OK, O.OK, O.ERR_OUTPUT_TOO_SMALL]
    short = Edited(cd, streams, ix, scripts, cb, stage_cap=per[0][1] + per[2][1] - 1).check()
    assert short.got["status"] == [O.OK, O.OK, O.ERR_OUTPUT_TOO_SMALL, O.OK, O.ERR_OUTPUT_TOO_SMALL]
    caps = list(full.got["out_len"])
    caps[2] -= 1                                                        # one byte short, in the middle of the batch
    mid = Edited(cd, streams, ix, scripts, cb, caps=caps).check()
    assert mid.got["status"] == [O.OK, O.OK, O.ERR_OUTPUT_TOO_SMALL, O.OK, O.OK] and mid.got["result"][3] == 3
    walked_is(cd, mid)


def two_middle_edits(ix, ns, html):
    out = []
    for b in range(ns):
        t = ix["total"][b]
        a = t // 2
        d = min(t - a, 300 + 7 * b)
        c = min(a + d + 40, t)
        out.append([(a, d, html[b:b + 100 + b]), (c, min(t - c, 5000), html[7 * b:7 * b + 3])])
    return out


def test_unsound_indexes_keep_every_guard_and_canary(html, named):
    names, streams, ix = named
    cd = SB.BlockCodec(0, O.HASH_CRC32C)
    rng = np.random.default_rng(5)
    ns = len(streams)
    scripts = two_middle_edits(ix, ns, html)
    bad = S.unsound_indexes(ix, streams, rng)
    assert len(bad) == 13
    refused = 0
    for index in bad:
        ed = Edited(cd, streams, index, scripts, 4096, caps=[len(s) + 80000 for s in streams], max_slots=6 * ns, stage_cap=1 << 24)
        ed.check()                                                      # guards and canaries held inside; every status is the model's
        refused += sum(1 for s in ed.got["status"] if s == O.ERR_BAD_ARG)
    assert refused > 40


def test_a_malformed_ed_first(html):
    cd = SB.BlockCodec(0, O.HASH_CRC32C)
    cb = 1000
    s = K.stream_of(html[:2500], cb)
    edits = [(10 * i, 3) for i in range(8)]
    srcs = [html[i:i + 5] for i in range(8)]
    ix = X.build_index([s] * 4)
    B = O.ERR_BAD_ARG
    for first, want in (([0, 2, 4, 6, 8], [0] * 4), ([0, 4, 2, 6, 8], [0, B, B, B]), ([2, 4, 4, 99, 1 << 63], [0, 0, 0, 0]), ([0, 2, 4, 9, 7], [0, 0, 0, B]),
                        ([5, 0, 0, 0, 0], [B] * 4), ([8, 8, 8, 8, 8], [0] * 4)):
        ed = Edited(cd, [s] * 4, ix, None, cb, flat=(first, edits, srcs)).check()
        assert ed.got["status"] == want, first
    assert ed.got["streams"] == [None] * 4


def test_empty_calls_and_streams_that_are_not_named(html):
    cd = SB.BlockCodec(0, O.HASH_CRC32C)
    cd._bind()
    call = N.frame_edit_lib().snp_frame_edit_indexed_batch
    result = Guarded(4, torch.int64)
    assert call(cd.ctx.handle, *[None] * 3, 0, *[None] * 5, 0, *[None] * 6, 0, 4096, 0, 0, *[None] * 6, *[None] * 5, None, None, result.ptr()) == O.OK
    torch.cuda.synchronize()
    assert result.read() == [0, 0, 0, 0]
    streams = [K.stream_of(html[:n], 1000) for n in (2500, 0, 1000)]
    ix = X.build_index(streams)
    ed = Edited(cd, streams, ix, [[], [], []], 1000, max_slots=3, stage_cap=5000).check()               # no edit at all
    assert ed.got["status"] == [O.OK] * 3 and ed.got["result"] == [0, 0, 0, 0] and S.same_index(ed.got["index"], ix)
    # ... whatever the index holds: nothing of it is trusted for a stream that is not named
    ed = Edited(cd, streams, {**ix, "tail": [5, 77, -3]}, [[(1 << 63, 0, b"")], [], [(7, 0, b""), (3, 0, b"")]], 1000, max_slots=0, stage_cap=0).check()
    assert ed.got["status"] == [O.OK] * 3 and ed.got["index"]["tail"] == [5, 77, -3]


# ---- 5: the new index under the sibling calls, no synchronisation between them ----------------------------------------------------------------------------
def test_the_new_index_serves_a_second_edit_the_splice_and_the_read_without_synchronisation(html):
    cd = SB.BlockCodec(0, O.HASH_CRC32C)
    cb = 4096
    raws = [html[:3 * cb + 100], html[5:5 + cb], html[9:9 + 5 * cb]]
    streams = [K.stream_of(x, cb) for x in raws]
    ix = X.build_index(streams)
    step1 = [[(7, 3, html[100:150]), (cb + 7, 2 * cb, b""), (3 * cb + 50, 0, html[:9])], [(cb, 0, html[9:9 + 3 * cb + 1])], [(0, 2 * cb + 1, b""), (3 * cb, 5, b"x")]]
    w1 = E.edit_plan(streams, ix, *E.flat(step1), cb)
    now1 = [E.applied(x, sc) for x, sc in zip(raws, step1)]
    step2 = [[(0, 1, b""), (1, 1, b"yy"), (len(now1[0]), 0, html[:cb + 1])], [(5, 10, b""), (cb + 5, 10, b"")], []]
    w2 = E.edit_plan(w1["streams"], w1["index"], *E.flat(step2), cb)
    now2 = [E.applied(x, sc) for x, sc in zip(now1, step2)]
    after2 = [n if n is not None else s for s, n in zip(w1["streams"], w2["streams"])]
    step3 = [(10, 0), (0, 0), (cb, cb)]
    ins3 = [html[:33], b"", html[40:40 + 2 * cb]]
    w3 = S.splice_plan(after2, w2["index"], step3, ins3, cb)
    assert w1["status"] == w2["status"] == w3["status"] == [O.OK] * 3
    framed, in_off, in_len = H.pack(streams)
    in_off, in_len = H.dev(in_off), H.dev(in_len)
    index = device_index(ix, 3)
    keep = []

    def arena(w):
        off, total = H.out_layout(np.array(w["out_bound"], dtype=np.int64))
        return torch.full((total,), CANARY, dtype=torch.uint8, device="cuda"), off

    def run_edit(script, w, framed, in_off, in_len, index):
        first, edits, srcs = E.flat(script)
        src, src_off, src_len = H.pack(srcs)
        out, off = arena(w)
        keep.extend([src, framed])
        out_len, status, ed_status, new_index, _ = cd.frame_edit_indexed(framed, in_off, in_len, index, H.dev(first), H.dev([e[0] for e in edits]),
                                                                         H.dev([e[1] for e in edits]), src, H.dev(src_off), H.dev(src_len), cb, out,
                                                                         H.dev(off), H.dev(w["out_bound"]), w["result"][0], w["result"][2])
        return out, H.dev(off), out_len, status, new_index

    out1, off1, len1, st1, index1 = run_edit(step1, w1, framed, in_off, in_len, index)
    out2, off2, len2, st2, index2 = run_edit(step2, w2, out1, off1, len1, index1)
    # stream 2 was not named in the second call: it still lies in the first call's arena, with its old rows in the new index
    both = torch.cat([out2, out1])
    off2b = torch.where(len2 > 0, off2, off1 + out2.numel())
    len2b = torch.where(len2 > 0, len2, len1)
    src3, src3_off, src3_len = H.pack(ins3)
    out3, off3 = arena(w3)
    len3, st3, index3, _ = cd.frame_splice_indexed(both, off2b, len2b, index2, H.dev([q[0] for q in step3]), H.dev([q[1] for q in step3]), src3, H.dev(src3_off),
                                                   H.dev(src3_len), cb, out3, H.dev(off3), H.dev(w3["out_bound"]), w3["result"][0], w3["result"][2])
    back = torch.full((len(now2[1]),), CANARY, dtype=torch.uint8, device="cuda")
    rl, rs, _ = cd.frame_read_indexed(both, off2b, len2b, index2, torch.ones(1, dtype=torch.int32, device="cuda"), H.dev([0]), H.dev([len(now2[1])]), back,
                                      H.dev([0]), H.dev([len(now2[1])]))
    torch.cuda.synchronize()
    assert st1.tolist() == st2.tolist() == st3.tolist() == [O.OK] * 3
    assert rs.tolist() == [O.OK] and back.cpu().numpy().tobytes() == now2[1]
    for out, off, lens, w in ((out1, off1, len1, w1), (out2, off2, len2, w2), (out3, H.dev(off3), len3, w3)):
        h = out.cpu().numpy()
        got = [h[o:o + n].tobytes() if n else None for o, n in zip(off.tolist(), lens.tolist())]
        assert got == w["streams"]
    used = w2["index"]["first"][-1]
    assert index2.first.tolist() == w2["index"]["first"] and index2.start[:used].tolist() == w2["index"]["start"]
    assert index2.pos[:used].tolist() == w2["index"]["pos"] and index2.total.tolist() == w2["index"]["total"]
    final = [n if n is not None else s for s, n in zip(after2, w3["streams"])]
    assert [O.frame_decode(x) for x in final] == [S.edited(x, q[0], q[1], s) for x, q, s in zip(now2, step3, ins3)]


def test_the_wrapper_that_sizes_the_call(html):
    cd = SB.BlockCodec(0, O.HASH_CRC32C)
    cb = 4096
    raws = [html[:3 * cb + 100], html[5:5 + cb], b""]
    streams = [K.stream_of(x, cb) if x else b"" for x in raws]
    scripts = [[(7, 3, html[100:150]), (cb + 7, cb, b"")], [], [(0, 0, html[:70000])]]
    first, edits, srcs = E.flat(scripts)
    want = E.edit_plan(streams, X.build_index(streams), first, edits, srcs, cb)
    framed, in_off, in_len = H.pack(streams)
    src, src_off, src_len = H.pack(srcs)
    index = cd.frame_index_buffers(framed, H.dev(in_off), H.dev(in_len))
    out, out_off, out_len, status, ed_status, new_index = cd.frame_edit_to_memory(framed, H.dev(in_off), H.dev(in_len), index, H.dev(first),
                                                                                  H.dev([e[0] for e in edits]), H.dev([e[1] for e in edits]), src,
                                                                                  H.dev(src_off), H.dev(src_len), cb)
    assert status.tolist() == want["status"] and ed_status.tolist() == want["ed_status"] and out_len.tolist() == want["out_len"]
    h = out.cpu().numpy()
    assert [h[o:o + n].tobytes() if n else None for o, n in zip(out_off.tolist(), out_len.tolist())] == want["streams"]
    assert new_index.first.tolist() == want["index"]["first"] and new_index.total.tolist() == want["index"]["total"]


# ---- 6: graph capture ------------------------------------------------------------------------------------------------------------------------------------------
def test_graph_capture_replays_the_call(html):
    cd = SB.BlockCodec(0, O.HASH_CRC32C)
    cb = 4096
    raws = [html[:3 * cb + 700], html[11:11 + cb], b"", html[5:5 + 9000]]
    scripts = [[(5, 1, b"q"), (cb + 5, cb, html[40000:40000 + 2 * cb + 3]), (2 * cb + 9, 0, b"zz")], [(0, 100, b""), (200, 0, html[:5])], [(0, 0, html[7:7 + cb])], []]
    streams = [K.stream_of(x, cb) if x else b"" for x in raws]
    ix = X.build_index(streams)
    first, edits, srcs = E.flat(scripts)
    want = E.edit_plan(streams, ix, first, edits, srcs, cb)
    ms, sc = want["result"][0], want["result"][2]
    framed, in_off, in_len = H.pack(streams)
    out_off, total = H.out_layout(np.array(want["out_bound"], dtype=np.int64))
    out = torch.full((total,), CANARY, dtype=torch.uint8, device="cuda")
    index = device_index(ix, 4)
    src, src_off, src_len = H.pack(srcs)
    tabs = [H.dev(in_off), H.dev(in_len), H.dev(first), H.dev([e[0] for e in edits]), H.dev([e[1] for e in edits]), H.dev(src_off), H.dev(src_len),
            H.dev(out_off), H.dev(want["out_bound"])]
    work = torch.empty(N.frame_edit_lib().snp_frame_edit_indexed_workspace(4, len(edits), ms, sc, cb), dtype=torch.uint8, device="cuda")

    def call():
        return cd.frame_edit_indexed(framed, tabs[0], tabs[1], index, tabs[2], tabs[3], tabs[4], src, tabs[5], tabs[6], cb, out, tabs[7], tabs[8], ms, sc,
                                     work=work)

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
        out_len, status, ed_status, new_ix, result = call()
    out.fill_(CANARY)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, plain)
    assert status.tolist() == want["status"] and out_len.tolist() == want["out_len"] and result.tolist() == want["result"]
    assert ed_status.tolist() == want["ed_status"]
    used = want["index"]["first"][-1]
    assert new_ix.first.tolist() == want["index"]["first"] and new_ix.pos[:used].tolist() == want["index"]["pos"]
    h = out.cpu().numpy()
    for b, x in enumerate(want["streams"]):
        if x is not None:
            assert h[out_off[b]:out_off[b] + len(x)].tobytes() == x, b


# ---- 7: launch tiers -------------------------------------------------------------------------------------------------------------------------------------------
def test_real_edges_on_the_decoders_list_path(html):
    """1 100 streams with two edits each: rows 0 and 1 for the first, row 3 for the second, whose head row is the shared row 1 and stays empty --
    3 300 real rows in an edge table of 2 x nedits = 4 400, and it is the table's size the decoder picks its list path by."""
    cd = SB.BlockCodec(0, O.HASH_CRC32C)
    cb, ns = 64, 1100
    raws = [html[b:b + 4 * cb + b % 50] for b in range(ns)]
    streams = [K.stream_of(x, cb) for x in raws]
    scripts = [[(10 + b % 40, cb, html[5 * b:5 * b + b % 3]), (cb + 60, 2 * cb, b"")] for b in range(ns)]     # rows 0-1, then rows 1-3
    ed = Edited(cd, streams, X.build_index(streams), scripts, cb).check()
    assert ed.got["result"][3] == ns and ed.got["result"][2] >= 3 * cb * ns and 4 * ns >= cd.ctx.get_option(N.OPT_SMALL_BLOCK_MIN_BATCH)
    assert [O.frame_decode(x) for x in ed.after()[::97]] == [E.applied(x, sc) for x, sc in list(zip(raws, scripts))[::97]]


def test_real_slots_on_the_lane_compressor(html):
    """33 000 new chunks of one byte: past the window compressor's range."""
    cd = SB.BlockCodec(0, O.HASH_CRC32C)
    cb, ns, per = 1, 33, 500
    raws = [html[b:b + 4 + b % 4] for b in range(ns)]
    streams = [K.stream_of(x, cb) for x in raws]
    scripts = [[(b % 3, 0, html[1000 + 7 * b:1000 + 7 * b + per]), (3, 1, html[9000 + 7 * b:9000 + 7 * b + per])] for b in range(ns)]
    ed = Edited(cd, streams, X.build_index(streams), scripts, cb).check()
    assert ed.got["result"][0] == 33000 >= cd.ctx.get_option(N.OPT_COMPRESS_WINDOW_MAX_BATCH) and ed.got["result"][3] == ns
    assert ed.after() == [K.stream_of(E.applied(x, sc), cb) for x, sc in zip(raws, scripts)]


# ---- 8: replace ------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("needle,repl", [(b"aa", b"b"), (b"aa", b"aaa"), (b"aa", b""), (b"<div", b"<section"), (b"href", b""), (b"abab", b"ab")])
def test_replace_streams_is_bytes_replace(html, needle, repl):
    cd = SB.BlockCodec(0, O.HASH_CRC32C)
    cb = 4096
    raws = [b"a" * 9001 + b"xaay" + b"a" * 4097, html[:40000], b"ab" * 3000 + b"a", b"", html[100:5000].replace(needle, b"#")]
    streams = [K.stream_of(x, cb) if x else b"" for x in raws]
    framed, in_off, in_len = H.pack(streams)
    in_off, in_len = H.dev(in_off), H.dev(in_len)
    index = cd.frame_index_buffers(framed, in_off, in_len)
    out, out_off, out_len, status, new_index, count = cd.frame_replace_streams(framed, in_off, in_len, index, needle, repl, cb)
    assert status.tolist() == [O.OK] * len(raws)
    assert count.tolist() == [x.count(needle) for x in raws] and count.tolist()[-1] == 0
    h = out.cpu().numpy()
    for b, x in enumerate(raws):
        got = h[int(out_off[b]):int(out_off[b]) + int(out_len[b])].tobytes()
        if x.count(needle):
            assert O.frame_decode(got) == x.replace(needle, repl), b
        else:
            assert got == b""
    assert new_index.total.tolist() == [len(x.replace(needle, repl)) for x in raws]

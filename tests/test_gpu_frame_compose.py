"""snp_frame_compose_indexed_batch (BlockCodec.frame_compose_indexed / frame_compose_to_memory): every new stream, status, length, size bound,
index array and d_result against the model (frame_compose_model.py), with canary bytes around every output range, guard words around every
array and the workspace, and the inputs compared with their copies after the call (compose_harness.Composed): one mixed batch per chunk size
with every shape of a segment list; the new index against snp_frame_index_batch and under the read, update, append, splice and rechunk calls
and a second compose; compose then rechunk byte for byte the chunked encoder's output; a splice, a compose and a rechunk without
synchronisation; graph capture replayed on changed segment lists; admission; corruption; rejections and unsound indexes; empty calls; the
launch tiers of the compressor and the decoder by bound and by real count; every layout; a kept chunk past position 2^32 of its source; a
segment of 70 000 rows.  Needs an MI355X."""
import numpy as np
import pytest
import torch

import frame_buffers_helpers as H
import frame_buffers_model as M
import frame_chunked_model as K
import frame_compose_model as CM
import frame_index_model as X
import frame_range_model as R
import frame_rechunk_model as RC
import frame_splice_model as S
import layouts
import oracle as O
import seekable_cases as SC
from append_harness import arena_of
from compose_harness import Composed, seg_tensors
from conftest import read_testdata
from rechunk_harness import Rechunked
from seekable_harness import CANARY, Guarded, index_call, index_tensors

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from snappier_amd import batch as SB, _native as N

VARIANTS = [O.HASH_CRC32C, O.HASH_MUL]


@pytest.fixture(scope="module")
def html():
    return read_testdata("html") * 5


def device_index(ix, ns):
    index = SB.FrameIndex(*index_tensors(ix, ns)[0])
    index.start, index.pos = index.start[:len(ix["start"])], index.pos[:len(ix["pos"])]
    return index


def walked_like(cd, cp):
    """The new index is what snp_frame_index_batch gives for the new streams (every output written)."""
    outs = cp.written()
    assert None not in outs
    assert index_call(cd, outs) == {**cp.got["index"], "result": X.build_index(outs)["result"]}


# ---- 1: one mixed batch per chunk size: (a), (b), (c), the new index ----------------------------------------------------------------------------
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("cb", CM.CHUNK_SIZES)
def test_a_mixed_batch_of_every_shape(html, cb, variant):
    cd = SB.BlockCodec(0, variant)
    streams, raws, ix, outputs, claims = CM.mixed_batch(html, cb, variant)
    cp = Composed(cd, streams, ix, CM.seg_lists(outputs), cb, variant=variant).check()
    assert cp.got["status"] == [O.OK] * len(outputs) and cp.got["result"][3] == len(outputs)
    want = [CM.concat(raws, segments) for segments in outputs]
    for j, (new, raw, claim) in enumerate(zip(cp.written(), want, claims)):
        assert O.frame_decode(new) == raw, j                            # (c)
        if claim == "a":
            assert new == K.stream_of(raw, cb, variant), j              # (a)
    walked_like(cd, cp)
    # (b): a rechunk of the outputs with their new index is the chunked encoder's output for the concatenation
    foreign = len(outputs) - len(CM.foreign_outputs())
    rc = Rechunked(cd, cp.written(), cp.got["index"], cb, variant=variant).check()
    assert rc.after()[:foreign] == [K.stream_of(raw, cb, variant) for raw in want[:foreign]]
    every = Rechunked(cd, cp.written(), cp.got["index"], cb, RC.REWRITE_ALL, variant=variant).check()
    assert every.got["streams"] == [K.stream_of(raw, cb, variant) for raw in want]


# ---- 2: the new index under the sibling calls ------------------------------------------------------------------------------------------------------
def test_the_outputs_serve_the_read_update_append_splice_rechunk_and_a_second_compose(html):
    cd = SB.BlockCodec(0, O.HASH_CRC32C)
    cb = 4096
    streams, raws, ix, _, _ = CM.mixed_batch(html, cb)
    outputs = [[(0, cb // 2, 3 * cb), (1, 7, 2 * cb)], [(2, 0, len(raws[2]))], [(1, cb, 2 * cb), (0, 100, 50)]]
    now = [CM.concat(raws, segments) for segments in outputs]
    segs = CM.seg_lists(outputs)
    framed0, off0, len0 = H.pack(streams)
    dsegs, _ = seg_tensors(segs)
    framed, off, lens, status, index = cd.frame_compose_to_memory(framed0, H.dev(off0), H.dev(len0), device_index(ix, len(streams)), *dsegs, cb)
    ns = len(now)
    assert status.tolist() == [O.OK] * ns
    want = CM.compose_plan(streams, ix, segs, cb)
    h = framed.cpu().numpy()
    assert [h[o:o + n].tobytes() for o, n in zip(off.tolist(), lens.tolist())] == want["streams"]
    used = want["index"]["first"][-1]
    assert index.first.tolist() == want["index"]["first"] and index.start[:used].tolist() == want["index"]["start"]
    assert index.pos[:used].tolist() == want["index"]["pos"] and index.total.tolist() == want["index"]["total"] and index.tail.tolist() == [0] * ns
    index.start, index.pos = index.start[:used], index.pos[:used]
    stream_no = torch.arange(ns, dtype=torch.int32, device="cuda")
    # read: every output whole
    out, out_off, out_len, st = cd.frame_gather_to_memory(framed, off, lens, index, stream_no, H.dev([0] * ns), H.dev([len(x) for x in now]))
    assert st.tolist() == [O.OK] * ns and out_len.tolist() == [len(x) for x in now]
    h = out.cpu().numpy()
    assert [h[o:o + n].tobytes() for o, n in zip(out_off.tolist(), out_len.tolist())] == now
    # update: ten bytes across the first border between two segments or chunks
    data = [bytes([65 + b]) * 10 for b in range(ns)]
    src, src_off, src_len = H.pack(data)
    at = [3 * cb - 5, cb - 5, cb - 5]
    uout, uoff, ulen, ust, ureq_st, _ = cd.frame_update_to_memory(framed, off, lens, index, stream_no, H.dev(at), src, H.dev(src_off), H.dev(src_len))
    assert ust.tolist() == [O.OK] * ns and ureq_st.tolist() == [O.OK] * ns
    h = uout.cpu().numpy()
    for b in range(ns):
        assert O.frame_decode(h[int(uoff[b]):int(uoff[b]) + int(ulen[b])].tobytes()) == now[b][:at[b]] + data[b] + now[b][at[b] + 10:], b
    # append, in place in an arena of its own
    more = [html[777:777 + n] for n in (cb + 3, 1, 2 * cb)]
    caps = [len(s) + len(m) + 64 for s, m in zip(want["streams"], more)]
    buf, boff = arena_of(want["streams"], caps)
    asrc, asrc_off, asrc_len = H.pack(more)
    new_len, ast, _ = cd.frame_append_to_memory(buf, H.dev(boff), lens, H.dev(caps), index, asrc, H.dev(asrc_off), H.dev(asrc_len), cb)
    assert ast.tolist() == [O.OK] * ns
    h = buf.cpu().numpy()
    for o, n, x, m in zip(boff, new_len.tolist(), now, more):
        assert O.frame_decode(h[o:o + n].tobytes()) == x + m
    # a splice, through the wrapper that sizes it
    edits = [(5, 10), (len(now[1]), 0), (cb // 2, cb)]
    ins = [b"", html[:99], html[50:50 + 2 * cb]]
    isrc, isrc_off, isrc_len = H.pack(ins)
    out2, off2, len2, st2, ix2 = cd.frame_splice_to_memory(framed, off, lens, index, H.dev([q[0] for q in edits]), H.dev([q[1] for q in edits]), isrc,
                                                           H.dev(isrc_off), H.dev(isrc_len), cb)
    assert st2.tolist() == [O.OK] * ns
    h = out2.cpu().numpy()
    spliced = [h[o:o + n].tobytes() for o, n in zip(off2.tolist(), len2.tolist())]
    assert spliced == S.splice_plan(want["streams"], want["index"], edits, ins, cb)["streams"]
    # the rechunk through the wrapper that sizes it: the chunked encoder's output for the concatenation, (b)
    out3, off3, len3, st3, _ = cd.frame_rechunk_to_memory(framed, off, lens, index, cb)
    assert st3.tolist() == [O.OK] * ns
    h = out3.cpu().numpy()
    assert [h[o:o + n].tobytes() if n else s for o, n, s in zip(off3.tolist(), len3.tolist(), want["streams"])] == [K.stream_of(x, cb) for x in now]
    # a second compose over the outputs: the outputs swapped and cut
    again = [[(1, 3, len(now[1]) - 3), (0, 0, len(now[0]))], [(2, cb - 1, 2)]]
    dsegs2, _ = seg_tensors(CM.seg_lists(again))
    out4, off4, len4, st4, _ = cd.frame_compose_to_memory(framed, off, lens, index, *dsegs2, cb)
    assert st4.tolist() == [O.OK] * 2
    h = out4.cpu().numpy()
    got = [h[o:o + n].tobytes() for o, n in zip(off4.tolist(), len4.tolist())]
    assert got == CM.compose_plan(want["streams"], want["index"], CM.seg_lists(again), cb)["streams"]
    assert [O.frame_decode(x) for x in got] == [CM.concat(now, segments) for segments in again]


def test_compose_then_rechunk_equals_frame_encode_seekable(html):
    cd = SB.BlockCodec(0, O.HASH_CRC32C)
    cb = 1000
    raws = [html[:7300], html[11:11 + 5000]]
    src, src_off, src_len = H.pack(raws)
    framed, off, lens, st, _, index = cd.frame_encode_seekable(src, H.dev(src_off), H.dev(src_len), cb)
    assert st.tolist() == [O.OK] * 2
    outputs = [[(0, 333, 4000), (1, 1, 4999), (0, 0, 7300)], [(1, 2500, 1000)]]
    dsegs, _ = seg_tensors(CM.seg_lists(outputs))
    out, ooff, olen, st, oix = cd.frame_compose_to_memory(framed, off, lens, index, *dsegs, cb)
    assert st.tolist() == [O.OK] * 2
    used = int(oix.first[-1])
    oix.start, oix.pos = oix.start[:used], oix.pos[:used]
    out2, off2, len2, st2, _ = cd.frame_rechunk_to_memory(out, ooff, olen, oix, cb)
    assert st2.tolist() == [O.OK] * 2
    want = [CM.concat(raws, segments) for segments in outputs]
    wsrc, wsrc_off, wsrc_len = H.pack(want)
    enc, eoff, elen, est = cd.frame_encode_seekable(wsrc, H.dev(wsrc_off), H.dev(wsrc_len), cb)[:4]
    h, e = out2.cpu().numpy(), enc.cpu().numpy()
    assert len2.tolist() == elen.tolist() and min(len2.tolist()) > 0
    for a, b, n, raw in zip(off2.tolist(), eoff.tolist(), elen.tolist(), want):
        assert h[a:a + n].tobytes() == e[b:b + n].tobytes() == K.stream_of(raw, cb)


# ---- 3: splice, compose, rechunk on one context, no synchronisation between them -----------------------------------------------------------------
@pytest.mark.parametrize("cb", [100, 65536])
def test_a_splice_a_compose_and_a_rechunk_in_a_row(html, cb):
    cd = SB.BlockCodec(0, O.HASH_CRC32C)
    raws = [html[:2 * cb + cb // 3], html[3:3 + cb], html[:4 * cb]]
    streams = [K.stream_of(x, cb) for x in raws]
    ix = X.build_index(streams)
    step = [(cb // 2, 0, cb + 1), (0, cb // 2, 0), (cb, 2 * cb, 5)]
    srcs = [html[17 * b:17 * b + q[2]] for b, q in enumerate(step)]
    # the model runs ahead, so that every call is sized without reading anything back
    w1 = S.splice_plan(streams, ix, [q[:2] for q in step], srcs, cb)
    assert w1["status"] == [O.OK] * 3
    raws = [S.edited(x, q[0], q[1], s) for x, q, s in zip(raws, step, srcs)]
    outputs = [[(0, 0, len(raws[0])), (2, 0, len(raws[2]))], [(1, 1, len(raws[1]) - 2), (0, cb, cb)], []]
    segs = CM.seg_lists(outputs)
    w2 = CM.compose_plan(w1["streams"], w1["index"], segs, cb)
    assert w2["status"] == [O.OK] * 3
    w3 = RC.rechunk_plan(w2["streams"], w2["index"], cb)
    assert RC.after(w2["streams"], w3) == [K.stream_of(CM.concat(raws, segments), cb) for segments in outputs]
    framed, in_off, in_len = H.pack(streams)
    src, src_off, src_len = H.pack(srcs)
    off1, total = H.out_layout(np.array(w1["out_bound"], dtype=np.int64))
    out1 = torch.full((total,), CANARY, dtype=torch.uint8, device="cuda")
    len1, _, index1, _ = cd.frame_splice_indexed(framed, H.dev(in_off), H.dev(in_len), device_index(ix, 3), H.dev([q[0] for q in step]),
                                                H.dev([q[1] for q in step]), src, H.dev(src_off), H.dev(src_len), cb, out1, H.dev(off1),
                                                H.dev(w1["out_bound"]), w1["result"][0], w1["result"][2])
    off2, total = H.out_layout(np.array(w2["out_bound"], dtype=np.int64))
    out2 = torch.full((total,), CANARY, dtype=torch.uint8, device="cuda")
    dsegs, _ = seg_tensors(segs)
    len2, _, index2, _ = cd.frame_compose_indexed(out1, H.dev(off1), len1, index1, cb, out2, H.dev(off2), H.dev(w2["out_bound"]), w2["result"][0],
                                                  w2["result"][2], w2["result"][4], *dsegs)
    off3, total = H.out_layout(np.array(w3["out_bound"], dtype=np.int64))
    out3 = torch.full((total,), CANARY, dtype=torch.uint8, device="cuda")
    len3, status, index3, result = cd.frame_rechunk_indexed(out2, H.dev(off2), len2, index2, cb, out3, H.dev(off3), H.dev(w3["out_bound"]),
                                                            w3["result"][0], w3["result"][2], w3["result"][4])
    torch.cuda.synchronize()
    assert status.tolist() == [O.OK] * 3 and len3.tolist() == w3["out_len"] and result.tolist() == w3["result"]
    h = out3.cpu().numpy()
    assert [h[o:o + n].tobytes() if n else None for o, n in zip(off3.tolist(), len3.tolist())] == w3["streams"]
    assert (H.outside_ranges(h, off3.tolist(), len3.tolist()) == CANARY).all()
    h = out2.cpu().numpy()
    assert [h[o:o + n].tobytes() for o, n in zip(off2.tolist(), len2.tolist())] == w2["streams"]
    used = w3["index"]["first"][-1]
    assert index3.first.tolist() == w3["index"]["first"] and index3.pos[:used].tolist() == w3["index"]["pos"]


# ---- 4: graph capture ------------------------------------------------------------------------------------------------------------------------------
def test_graph_capture_replays_the_call_on_changed_segment_lists(html):
    cd = SB.BlockCodec(0, O.HASH_CRC32C)
    cb = 4096
    streams, raws, ix, _, _ = CM.mixed_batch(html, cb)
    ns = len(streams)
    lists = [[[(0, 100, 3 * cb), (1, cb, cb)], [(2, 5, 2 * cb)], [(3, 0, 3400)]],
             [[(1, 0, 2 * cb), (0, 1, cb + 7)], [(4, 1000, 700)], [(2, cb, cb)]]]
    wants = [CM.compose_plan(streams, ix, CM.seg_lists(o), cb) for o in lists]
    ms, sc, me = [max(w["result"][k] for w in wants) for k in (0, 2, 4)]
    caps = [max(a, b) for a, b in zip(wants[0]["out_bound"], wants[1]["out_bound"])]
    framed, in_off, in_len = H.pack(streams)
    out_off, total = H.out_layout(np.array(caps, dtype=np.int64))
    out = torch.full((total,), CANARY, dtype=torch.uint8, device="cuda")
    index = device_index(ix, ns)
    tabs = [H.dev(in_off), H.dev(in_len), H.dev(out_off), H.dev(caps)]
    dsegs = [seg_tensors(CM.seg_lists(o))[0] for o in lists]
    live = [t.clone() for t in dsegs[0]]
    work = torch.empty(N.frame_compose_lib().snp_frame_compose_indexed_workspace(ns, 3, live[1].numel(), ms, sc, cb, me), dtype=torch.uint8, device="cuda")

    def call():
        return cd.frame_compose_indexed(framed, tabs[0], tabs[1], index, cb, out, tabs[2], tabs[3], ms, sc, me, *live, work=work)

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        call()                                                          # the same call once before the capture
        torch.cuda.synchronize()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        out_len, status, new_ix, result = call()
    for k in (0, 1, 0):
        for t, v in zip(live, dsegs[k]):
            t.copy_(v)
        out.fill_(CANARY)
        g.replay()
        torch.cuda.synchronize()
        want = CM.compose_plan(streams, ix, CM.seg_lists(lists[k]), cb, caps, ms, sc, me)
        assert status.tolist() == want["status"] == [O.OK] * 3 and out_len.tolist() == want["out_len"] and result.tolist() == want["result"]
        used = want["index"]["first"][-1]
        assert new_ix.first.tolist() == want["index"]["first"] and new_ix.pos[:used].tolist() == want["index"]["pos"]
        assert new_ix.start[:used].tolist() == want["index"]["start"]
        h = out.cpu().numpy()
        assert [h[o:o + n].tobytes() for o, n in zip(out_off.tolist(), out_len.tolist())] == want["streams"]
        assert (H.outside_ranges(h, out_off.tolist(), out_len.tolist()) == CANARY).all()


# ---- 5: admission; corruption; the inputs are untrusted; empty calls -----------------------------------------------------------------------------
def test_admission_by_each_bound_and_by_out_cap(html):
    cd = SB.BlockCodec(0, O.HASH_CRC32C)
    cb = 512
    raws = [html[:3000], html[50:50 + 2048]]
    streams = [K.stream_of(raws[0], 500), K.stream_of(raws[1], cb)]
    ix = X.build_index(streams)
    outputs = [[(0, 250, 1000)], [(1, 0, 1024)], [(0, 100, 50), (1, 5, 1000)], [], [(0, 1400, 1300)]]
    segs = CM.seg_lists(outputs)
    full = Composed(cd, streams, ix, segs, cb).check()
    assert full.got["status"] == [O.OK] * 5
    sizing = Composed(cd, streams, ix, segs, cb, caps=[0] * 5, max_slots=0, stage_cap=0, max_entries=0).check()
    ms, _, sc, _, me, _ = sizing.got["result"]
    assert (ms, sc, me) == (7, 3524, 12) and sizing.got["streams"] == [None] * 5 and sizing.got["out_bound"] == full.got["out_bound"]
    late = [O.OK, O.OK, O.OK, O.OK, O.ERR_OUTPUT_TOO_SMALL]
    mid = [O.OK, O.OK] + [O.ERR_OUTPUT_TOO_SMALL] * 3
    assert Composed(cd, streams, ix, segs, cb, max_slots=ms - 1).check().got["status"] == late
    assert Composed(cd, streams, ix, segs, cb, stage_cap=sc - 1).check().got["status"] == late
    assert Composed(cd, streams, ix, segs, cb, max_entries=me - 1).check().got["status"] == late
    assert Composed(cd, streams, ix, segs, cb, max_slots=4).check().got["status"] == mid
    assert Composed(cd, streams, ix, segs, cb, stage_cap=1000 + 999).check().got["status"] == mid
    assert Composed(cd, streams, ix, segs, cb, max_entries=5).check().got["status"] == mid
    caps = list(full.got["out_len"])
    caps[2] -= 1                                                        # one byte short, in the middle of the batch
    one = Composed(cd, streams, ix, segs, cb, caps=caps).check()
    assert one.got["status"] == [O.OK, O.OK, O.ERR_OUTPUT_TOO_SMALL, O.OK, O.OK] and one.got["result"][3] == 4
    assert one.got["index"]["tail"][2] == O.ERR_OUTPUT_TOO_SMALL and one.got["index"]["total"][2] == 0


def test_corruption_in_an_edge_chunk_and_in_a_kept_chunk(html):
    cd = SB.BlockCodec(0, O.HASH_CRC32C)
    cb = 4096
    s = K.stream_of(html[:5 * cb], cb)
    rows = R.walk(s)[0]
    bad1, bad3 = R.corrupt_chunk(s, rows[1]), R.corrupt_chunk(s, rows[3])
    want1, want3 = M.chunk_status(bad1, rows[1]), M.chunk_status(bad3, rows[3])
    assert want1 != O.OK != want3
    streams = [s, bad1, bad3, R.corrupt_chunk(bad1, rows[3])]
    ix = X.build_index([s] * 4)
    # per source: chunk 1 cut at the head, chunk 2 kept, chunk 3 cut at the tail; then chunk 1 kept
    outputs = [[(b, cb + 9, 2 * cb)] for b in range(4)] + [[(1, cb, 2 * cb)], [(0, 5, 10), (3, cb + 9, 2 * cb), (2, cb + 9, 2 * cb)]]
    cp = Composed(cd, streams, ix, CM.seg_lists(outputs), cb).check()
    assert cp.got["status"] == [O.OK, want1, want3, want1, O.OK, want1] and cp.got["result"][3] == 2
    assert cp.written()[4] != K.stream_of(html[cb:3 * cb], cb) and O.frame_decode(cp.written()[0]) == html[cb + 9:3 * cb + 9]   # A CORRUPT KEPT CHUNK IS COPIED


def rejections(streams, ix):
    """name -> (index, segment list): every rejection of the header, each beside outputs that go on."""
    t = ix["total"]
    good = [(0, 1, 100)]
    lists = {
        "stream_out_of_range": [good, [(len(streams), 0, 1)], good],
        "stream_out_of_range_in_an_empty_segment": [[(len(streams), 0, 0)], good],
        "past_the_total": [good, [(0, t[0] - 5, 6)], [(0, t[0], 0)], [(0, t[0] + 1, 0)]],
        "wrapping": [[(0, (1 << 64) - 2, 5)], good, [(1, 1 << 63, 1 << 63)]],
        "second_segment_fails": [[(0, 0, 10), (1, t[1], 1), (len(streams), 0, 1)], good],
    }
    got = {k: (ix, CM.seg_lists(v)) for k, v in lists.items()}
    backwards = CM.seg_lists([good, good, good])
    backwards["first"] = [0, 2, 1, 3]
    got["seg_first_runs_backwards"] = (ix, backwards)
    beyond = CM.seg_lists([good, good])
    beyond["first"] = [0, 1, 1 << 40]
    got["seg_first_beyond_nsegs"] = (ix, beyond)
    for name, tail in (("a_broken_source", O.ERR_CRC_MISMATCH), ("an_unindexed_source", O.ERR_OUTPUT_TOO_SMALL), ("no_status_of_the_walk", 77),
                       ("a_negative_tail", -3)):
        other = {**ix, "tail": [ix["tail"][0], tail] + list(ix["tail"][2:])}
        got[name] = (other, CM.seg_lists([good, [(1, 0, 5)], [(1, 0, 0)], [(0, 0, 3), (1, 1, 1)]]))
    flipped = {**ix, "first": [ix["first"][1], ix["first"][0]] + list(ix["first"][2:])}
    got["f1_below_f0"] = (flipped, CM.seg_lists([[(0, 0, 5)], [(1, 0, 5)]]))
    norows = {**ix, "first": [0, 0] + list(ix["first"][2:])}
    got["bytes_and_no_row"] = (norows, CM.seg_lists([[(0, 0, 5)], [(1, 0, 5)]]))
    return got


def test_every_rejection_beside_outputs_that_go_on(html):
    cd = SB.BlockCodec(0, O.HASH_CRC32C)
    streams = [K.stream_of(html[:3000], 500), K.stream_of(html[9:2009], 700)]
    ix = X.build_index(streams)
    seen = set()
    for name, (index, segs) in rejections(streams, ix).items():
        cp = Composed(cd, streams, index, segs, 512).check()
        seen |= set(cp.got["status"])                                   # (every status is the model's)
    assert seen == {O.OK, O.ERR_BAD_ARG, O.ERR_CRC_MISMATCH, O.ERR_OUTPUT_TOO_SMALL}


def test_unsound_indexes_keep_every_guard_and_canary():
    cases = X.named_streams()
    streams = list(cases.values())
    ix = X.build_index(streams)
    cd = SB.BlockCodec(0, O.HASH_CRC32C)
    rng = np.random.default_rng(5)
    bad = RC.unsound_indexes(ix, streams, rng)
    assert len(bad) == 13
    outputs = []
    for b in range(len(streams)):
        t = ix["total"][b]
        outputs += [[(b, 0, t)], [(b, t // 3, t // 2), (b, 1, 1)]]
    segs = CM.seg_lists(outputs)
    refused = 0
    for index in bad:
        ne = min(len(index["start"]), len(index["pos"]))
        cp = Composed(cd, streams, index, segs, 4096, caps=[2 * len(s) + 70000 for s in streams for _ in (0, 1)], max_slots=1 << 12, stage_cap=1 << 25,
                      max_entries=2 * ne + 256)
        cp.check()                                                      # guards and canaries held inside; every status is the model's
        refused += sum(1 for s in cp.got["status"] if s == O.ERR_BAD_ARG)
    assert refused > 40


def test_empty_calls(html):
    cd = SB.BlockCodec(0, O.HASH_CRC32C)
    cd._bind()
    call = N.frame_compose_lib().snp_frame_compose_indexed_batch
    result = Guarded(6, torch.int64)
    assert call(cd.ctx.handle, *[None] * 3, 0, *[None] * 5, 0, *[None] * 4, 0, 0, 4096, 0, 0, 0, *[None] * 5, *[None] * 5, None, None, result.ptr()) == O.OK
    torch.cuda.synchronize()
    assert result.read() == [0] * 6
    streams = [K.stream_of(html[:2500], 1000)]
    ix = X.build_index(streams)
    cp = Composed(cd, streams, ix, CM.seg_lists([[], [(0, 5, 0)], []]), 1000).check()      # no segment, an empty one: the identifier
    assert cp.written() == [M.STREAM_ID] * 3 and cp.got["result"] == [0, 30, 0, 3, 0, 0]
    cp = Composed(cd, [], X.build_index([]), CM.seg_lists([[]]), 1000).check()            # no source at all
    assert cp.written() == [M.STREAM_ID]


# ---- 6: launch tiers -------------------------------------------------------------------------------------------------------------------------------
def test_the_slot_bound_picks_the_tier_of_both_tables_and_changes_nothing(html):
    cd = SB.BlockCodec(0, O.HASH_CRC32C)
    streams, raws, ix, outputs, _ = CM.mixed_batch(html, 1000)
    segs = CM.seg_lists(outputs)
    exact = Composed(cd, streams, ix, segs, 1000).check()
    tiers = [cd.ctx.get_option(getattr(N, o)) for o in ("OPT_COMPRESS_WINDOW_DUAL_MIN_BATCH", "OPT_COMPRESS_WINDOW_GLOBAL_MIN_BATCH",
                                                        "OPT_SMALL_BLOCK_MIN_BATCH", "OPT_COMPRESS_WINDOW_MAX_BATCH")]
    assert tiers[0] == 1536 and tiers[2:] == [4096, 32768]
    for ms in [t - d for t in tiers for d in (1, 0)]:
        cp = Composed(cd, streams, ix, segs, 1000, caps=exact.caps, max_slots=ms).check()
        assert np.array_equal(cp.h, exact.h) and cp.got == exact.got, ms


def one_byte_chunks(raw: bytes) -> bytes:
    """The stream of raw at one-byte chunks (what the chunked encoder writes: a one-byte piece does not shrink), built from 256 chunks."""
    chunk = [M.data_chunk(bytes([v]), compressed=False) for v in range(256)]
    return M.STREAM_ID + b"".join(chunk[v] for v in raw)


def one_byte_index(lens):
    first, start, pos = [0], [], []
    for n in lens:
        start += range(n)
        pos += range(10, 10 + 9 * n, 9)
        first.append(len(start))
    return dict(first=first, start=start, pos=pos, total=list(lens), tail=[O.OK] * len(lens))


def test_real_rows_copy_only(html):
    """33 000 kept one-byte chunks from three sources in one output: no edge, copy only, past the window compressor's range in rows."""
    cd = SB.BlockCodec(0, O.HASH_CRC32C)
    raws = [html[b:b + 11000] for b in range(3)]
    streams = [one_byte_chunks(x) for x in raws]
    assert streams[0][:1000] == K.stream_of(raws[0][:110], 1)[:1000]
    ix = one_byte_index([11000] * 3)
    cap = 10 + 9 * 33000
    cp = Composed(cd, streams, ix, CM.seg_lists([[(b, 0, 11000) for b in range(3)]]), 1, caps=[cap], max_slots=0, stage_cap=0, max_entries=33000,
                  model=False)
    assert cp.got["result"] == [0, cap, 0, 1, 33000, 33000] and 33000 >= cd.ctx.get_option(N.OPT_COMPRESS_WINDOW_MAX_BATCH)
    assert cp.got["status"] == [O.OK] and cp.written() == [one_byte_chunks(b"".join(raws))] and cp.got["out_bound"] == [cap]
    assert cp.got["index"] == one_byte_index([33000])


def test_real_rows_on_the_decoders_list_path(html):
    """4 100 segments that each cut one chunk on both sides: 4 100 decode rows and 4 100 pieces."""
    cd = SB.BlockCodec(0, O.HASH_CRC32C)
    raws = [html[b:b + 6400] for b in range(41)]
    streams = [K.stream_of(x, 64) for x in raws]
    outputs = [[(b, 64 * k + 1, 62) for k in range(100)] for b in range(41)]
    cp = Composed(cd, streams, X.build_index(streams), CM.seg_lists(outputs), 100).check()
    assert cp.got["result"][0] == 4100 >= cd.ctx.get_option(N.OPT_SMALL_BLOCK_MIN_BATCH) and cp.got["result"][3:] == [41, 4100, 0]
    assert [O.frame_decode(x) for x in cp.written()] == [CM.concat(raws, segments) for segments in outputs]


def test_a_segment_of_70000_rows(html):
    """The plan kernel's long walk: more than one round of its workgroup over the rows of one segment.  The window cuts nothing."""
    cd = SB.BlockCodec(0, O.HASH_CRC32C)
    raw = (html * 2)[:70000]
    stream = one_byte_chunks(raw)
    ix = one_byte_index([70000])
    n = 69995
    cap = 10 + 9 * n
    cp = Composed(cd, [stream], ix, CM.seg_lists([[(0, 3, n)]]), 1, caps=[cap], max_slots=0, stage_cap=0, max_entries=n, model=False)
    assert cp.got["status"] == [O.OK] and cp.got["result"] == [0, cap, 0, 1, n, n]
    assert cp.written() == [one_byte_chunks(raw[3:3 + n])] and cp.got["index"] == one_byte_index([n])


# ---- 7: every layout -------------------------------------------------------------------------------------------------------------------------------
_default = {}


def default_run(html, variant):
    if variant not in _default:
        streams, raws, ix, outputs, _ = CM.mixed_batch(html, 1000, variant)
        segs = CM.seg_lists(outputs)
        _default[variant] = (streams, ix, segs, Composed(SB.BlockCodec(0, variant), streams, ix, segs, 1000, variant=variant).check())
    return _default[variant]


@pytest.mark.parametrize("crc", [0, 1, 2])
@pytest.mark.parametrize("layout", layouts.COMPRESS_LAYOUTS)
def test_every_compress_layout_and_crc_kernel(html, layout, crc):
    for variant in VARIANTS:
        streams, ix, segs, base = default_run(html, variant)
        cd = SB.BlockCodec(0, variant)
        layouts.set_compress_layout(cd.ctx, layout)
        cd.ctx.set_option(N.OPT_CRC_KERNEL, crc)
        cp = Composed(cd, streams, ix, segs, 1000, caps=base.caps, max_slots=base.ms, stage_cap=base.sc, max_entries=base.me, variant=variant, model=False)
        cp.want = base.want
        cp.check()
        assert np.array_equal(cp.h, base.h)


@pytest.mark.parametrize("fenced", [0, 1])
@pytest.mark.parametrize("decode", layouts.DECODE_LAYOUTS)
def test_every_decode_layout(html, decode, fenced):
    streams, ix, segs, base = default_run(html, O.HASH_CRC32C)
    cd = SB.BlockCodec(0, O.HASH_CRC32C)
    layouts.set_decode_layout(cd.ctx, decode, fenced)
    cp = Composed(cd, streams, ix, segs, 1000, caps=base.caps, max_slots=base.ms, stage_cap=base.sc, max_entries=base.me, model=False)
    cp.want = base.want
    cp.check()
    assert np.array_equal(cp.h, base.h)


# ---- 8: past 4 GiB ---------------------------------------------------------------------------------------------------------------------------------
def test_a_kept_chunk_whose_source_position_lies_past_2_to_the_32(html):
    """One source of 66 000 uncompressed chunks of 65 536 bytes, 4.03 GiB of them, then a short chunk: a window over its end cuts the last but
    one of them at the head, keeps the last one -- copied from behind position 2^32 -- and cuts the short chunk at the tail."""
    cb, nkept = 65536, 66000
    free = torch.cuda.mem_get_info()[0]
    if free < 8 << 30:
        pytest.skip(f"needs 8 GiB of free device memory, {free >> 30} GiB free")
    cd = SB.BlockCodec(0, O.HASH_CRC32C)
    piece = html[:cb]
    one = M.data_chunk(piece, compressed=False)
    tail_raw = html[100:100 + 1000]
    tail = M.data_chunk(tail_raw)
    kept_bytes = nkept * len(one)
    n = 10 + kept_bytes + len(tail)
    assert 10 + kept_bytes - 2 * len(one) > 1 << 32
    buf = torch.empty(n, dtype=torch.uint8, device="cuda")
    buf[:10] = torch.from_numpy(np.frombuffer(M.STREAM_ID, dtype=np.uint8).copy()).cuda()
    buf[10:10 + kept_bytes].view(nkept, len(one))[:] = torch.from_numpy(np.frombuffer(one, dtype=np.uint8).copy()).cuda()
    buf[10 + kept_bytes:] = torch.from_numpy(np.frombuffer(tail, dtype=np.uint8).copy()).cuda()
    start = torch.arange(nkept + 1, dtype=torch.int64, device="cuda") * cb
    pos = 10 + torch.arange(nkept + 1, dtype=torch.int64, device="cuda") * len(one)
    index = SB.FrameIndex(H.dev([0, nkept + 1]), start, pos, H.dev([nkept * cb + 1000]), torch.zeros(1, dtype=torch.int32, device="cuda"))
    want = M.STREAM_ID + K.chunks_of(piece[100:], cb)[0] + one + K.chunks_of(tail_raw[:100], cb)[0]
    cap = 10 + len(one) + 16 + cb
    out = torch.full((cap + 64,), CANARY, dtype=torch.uint8, device="cuda")
    dsegs, _ = seg_tensors(CM.seg_lists([[(0, (nkept - 2) * cb + 100, 2 * cb)]]))
    out_len, status, new_ix, result, bound = cd.frame_compose_indexed(buf, H.dev([0]), H.dev([n]), index, cb, out, H.dev([0]), H.dev([cap]), 2,
                                                                      cb + 1000, 3, *dsegs, with_bound=True)
    assert status.tolist() == [O.OK] and out_len.tolist() == [len(want)] and bound.tolist() == [cap]
    assert result.tolist() == [2, len(want), cb + 1000, 1, 3, 1]
    assert out[:len(want)].cpu().numpy().tobytes() == want and bool((out[len(want):] == CANARY).all())
    first = len(K.chunks_of(piece[100:], cb)[0])
    assert new_ix.first.tolist() == [0, 3] and new_ix.start[:3].tolist() == [0, cb - 100, 2 * cb - 100]
    assert new_ix.pos[:3].tolist() == [10, 10 + first, 10 + first + len(one)] and new_ix.total.tolist() == [2 * cb]


# ---- rebuilt chunks stored compressed and stored raw, at the chunk sizes whose emit teams are 64, 128 and 256 threads --------------------------------
@pytest.mark.parametrize("cb", SC.TEAM_CHUNK_SIZES)
def test_rebuilt_chunks_raw_and_compressed_at_every_team_size(cb):
    cd = SB.BlockCodec(0, O.HASH_CRC32C)
    blobs = SC.team_blobs(cb)
    streams = [K.stream_of(x, cb) for x in blobs]
    outputs = [[(b, 5, len(x) - 9)] for b, x in enumerate(blobs)]       # a segment that cuts its first and its last chunk: two pieces, kept chunks between
    cp = Composed(cd, streams, X.build_index(streams), CM.seg_lists(outputs), cb).check()
    assert cp.got["status"] == [O.OK] * 3 and cp.got["result"][3] == 3
    assert [O.frame_decode(s) for s in cp.written()] == [x[5:len(x) - 4] for x in blobs]
    assert [SC.chunk_types(s) for s in cp.written()[:2]] == [{1}, {0}]

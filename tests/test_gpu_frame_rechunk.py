"""snp_frame_rechunk_indexed_batch (BlockCodec.frame_rechunk_indexed / frame_rechunk_to_memory): every new stream, status, length, size bound,
index array and d_result against the model (frame_rechunk_model.py), with canary bytes around every output range, guard words around every
array and the workspace, and the inputs compared with their copies after the call (rechunk_harness.Rechunked): fragmented streams at the seam
chunk sizes byte for byte the chunked encoder's output; a change of the chunk size and back; foreign streams with and without
SNP_RECHUNK_REWRITE_ALL; the new index against snp_frame_index_batch, under the read, update, append and splice calls and under a second
rechunk; splices and a rechunk without synchronisation; graph capture; admission; corruption; unsound indexes; empty calls; the launch tiers of
the compressor and the decoder by bound and by real count; every layout; a kept prefix past position 2^32.  Needs an MI355X."""
import numpy as np
import pytest
import torch

import frame_buffers_helpers as H
import frame_buffers_model as M
import frame_chunked_model as K
import frame_index_model as X
import frame_range_model as R
import frame_rechunk_model as RC
import frame_splice_model as S
import layouts
import oracle as O
import seekable_cases as SC
from append_harness import arena_of
from conftest import read_testdata
from rechunk_harness import Rechunked, new_table
from seekable_harness import CANARY, Guarded, index_call, index_tensors
from test_frame_rechunk_model import fragmented

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from snappier_amd import batch as SB, _native as N

VARIANTS = [O.HASH_CRC32C, O.HASH_MUL]
ALL = RC.REWRITE_ALL


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


# ---- 1: fragmented streams become the chunked encoder's output, (b) and (a) -------------------------------------------------------------------------
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("cb", RC.CHUNK_SIZES)
def test_fragmented_streams_become_the_chunked_encoders_output(html, cb, variant):
    cd = SB.BlockCodec(0, variant)
    names, raws, streams = fragmented(html, cb, variant)
    ix = X.build_index(streams)
    want = [K.stream_of(a, cb, variant) for a in raws]
    rc = Rechunked(cd, streams, ix, cb, variant=variant).check()
    assert set(rc.got["status"]) == {O.OK} and rc.after() == want       # (b)
    assert rc.got["result"][3] + rc.got["result"][5] == len(streams) and (cb == 1 or rc.got["result"][3] >= 4)
    walked_like(cd, rc)
    every = Rechunked(cd, streams, ix, cb, ALL, variant=variant).check()
    assert every.got["streams"] == want and every.got["result"][3] == len(streams)       # (a)
    # fed to a second rechunk, every stream is left alone
    again = Rechunked(cd, rc.after(), rc.got["index"], cb, variant=variant).check()
    assert again.got["streams"] == [None] * len(streams) and again.got["result"] == [0, 0, 0, 0, len(rc.got["index"]["start"]), len(streams)]
    assert again.got["index"] == rc.got["index"]


def test_the_chunk_size_changed_and_back(html):
    cd = SB.BlockCodec(0, O.HASH_CRC32C)
    raws = [html[:300000], html[5:5 + 65536], html[9:9 + 65537], html[:4096], html[:1], b""]
    small = [K.stream_of(a, 4096) for a in raws]
    big = [K.stream_of(a, 65536) for a in raws]
    up = Rechunked(cd, small, X.build_index(small), 65536).check()
    assert up.after() == big and up.got["result"][3] == 3 and up.got["result"][5] == 3
    walked_like(cd, up)
    down = Rechunked(cd, big, up.got["index"], 4096).check()
    assert down.after() == small
    walked_like(cd, down)


# ---- 2: foreign streams; the named streams; a mixed batch -----------------------------------------------------------------------------------------------
def test_foreign_streams_with_and_without_rewrite_all(html):
    cd = SB.BlockCodec(0, O.HASH_CRC32C)
    cases = RC.foreign_streams(html)
    streams, raws = [c[0] for c in cases.values()], [c[1] for c in cases.values()]
    ix = X.build_index(streams)
    for cb in (1, 500, 65536):
        every = Rechunked(cd, streams, ix, cb, ALL).check()
        assert every.got["streams"] == [K.stream_of(a, cb) for a in raws], cb                # (a)
        rc = Rechunked(cd, streams, ix, cb).check()
        assert rc.got["status"] == [O.OK] * len(streams)
        for name, new, a in zip(cases, rc.after(), raws):                # (c)
            assert O.frame_decode(new) == a and RC.data_chunk_lengths(new) == [cb] * (len(a) // cb) + ([len(a) % cb] if len(a) % cb else []), (cb, name)
        walked_like(cd, rc)


def test_named_foreign_streams(named):
    names, streams, ix = named
    cd = SB.BlockCodec(0, O.HASH_CRC32C)
    for flags in (0, ALL):
        rc = Rechunked(cd, streams, ix, 4096, flags).check()
        written = sum(1 for x in rc.got["streams"] if x is not None)
        assert written >= 8 and len(set(rc.got["status"])) >= 3       # (the floor the model meets on the CPU)
        walked_like(cd, rc)


def mixed_batch(html, variant=O.HASH_CRC32C):
    """Fragmented, canonical, foreign, broken and empty streams, compressed and raw chunks: -> (streams, index)."""
    rnd = bytes(np.random.default_rng(3).integers(0, 256, 3 * 4096 + 77, dtype=np.uint8))
    frag = fragmented(html, 1000, variant)[2]
    foreign = [c[0] for c in RC.foreign_streams(html).values()]
    broken = R.uniform_stream(3, 1)[0][:-5]
    ch = M.data_chunk
    streams = [frag[0]] + frag[2:5] + [K.stream_of(html[:3500], 1000, variant), K.stream_of(rnd, 4096, variant), foreign[0], broken, b"", foreign[2],
                          M.STREAM_ID + ch(rnd[:700], False) + ch(html[:300]) + ch(rnd[700:1400], False), K.stream_of(html[:70000], 65536, variant)]
    return streams, X.build_index(streams)


def test_a_mixed_batch_written_left_alone_refused_and_broken(html):
    cd = SB.BlockCodec(0, O.HASH_MUL)
    streams, ix = mixed_batch(html, O.HASH_MUL)
    free = RC.rechunk_plan(streams, ix, 1000, variant=O.HASH_MUL)
    caps = list(free["out_bound"])
    caps[1] = free["out_len"][1] - 1                                    # refused: its range is one byte short
    rc = Rechunked(cd, streams, ix, 1000, caps=caps, variant=O.HASH_MUL).check()
    assert rc.got["status"][1] == O.ERR_OUTPUT_TOO_SMALL and rc.got["status"][7] == ix["tail"][7] != O.OK
    assert rc.got["streams"][4] is None and rc.got["status"][4] == O.OK and rc.got["result"][5] == 1
    assert rc.got["result"][3] == len(streams) - 3
    walked_like(cd, rc)


# ---- 3: the new index under the sibling calls --------------------------------------------------------------------------------------------------------------
def test_the_new_index_serves_the_read_update_append_splice_and_a_second_rechunk(html):
    cd = SB.BlockCodec(0, O.HASH_CRC32C)
    cb = 4096
    names, now, streams = fragmented(html, cb, O.HASH_CRC32C)
    pick = [names.index(x) for x in ("insert_mid_chunk", "drop_prefix_of_a_non_multiple", "several_edits")]
    now, streams = [now[i] for i in pick], [streams[i] for i in pick]
    rc = Rechunked(cd, streams, X.build_index(streams), cb).check()
    assert rc.got["result"][3] == 3
    framed, off, lens = new_table(rc)
    index = rc.frame_index()
    ns = len(now)
    stream_no = torch.arange(ns, dtype=torch.int32, device="cuda")
    # read: every stream whole
    out, out_off, out_len, status = cd.frame_gather_to_memory(framed, off, lens, index, stream_no, H.dev([0] * ns), H.dev([len(x) for x in now]))
    assert status.tolist() == [O.OK] * ns and out_len.tolist() == [len(x) for x in now]
    h = out.cpu().numpy()
    assert [h[o:o + n].tobytes() for o, n in zip(out_off.tolist(), out_len.tolist())] == now
    # update: ten bytes across the first chunk boundary
    data = [bytes([65 + b]) * 10 for b in range(ns)]
    src, src_off, src_len = H.pack(data)
    uout, uoff, ulen, ust, ureq_st, _ = cd.frame_update_to_memory(framed, off, lens, index, stream_no, H.dev([cb - 5] * ns), src, H.dev(src_off),
                                                                   H.dev(src_len))
    assert ust.tolist() == [O.OK] * ns and ureq_st.tolist() == [O.OK] * ns
    h = uout.cpu().numpy()
    for b in range(ns):
        assert O.frame_decode(h[int(uoff[b]):int(uoff[b]) + int(ulen[b])].tobytes()) == now[b][:cb - 5] + data[b] + now[b][cb + 5:], b
    # append, in place in an arena of its own
    more = [html[777:777 + n] for n in (cb + 3, 1, 2 * cb)]
    caps = [len(s) + len(m) + 64 for s, m in zip(rc.after(), more)]
    buf, boff = arena_of(rc.after(), caps)
    asrc, asrc_off, asrc_len = H.pack(more)
    new_len, ast, aix = cd.frame_append_to_memory(buf, H.dev(boff), lens, H.dev(caps), index, asrc, H.dev(asrc_off), H.dev(asrc_len), cb)
    assert ast.tolist() == [O.OK] * ns
    h = buf.cpu().numpy()
    grown = [h[o:o + n].tobytes() for o, n in zip(boff, new_len.tolist())]
    assert grown == [K.stream_of(x + m, cb) for x, m in zip(now, more)]
    # a splice, through the wrapper that sizes it
    edits = [(5, 10), (len(now[1]), 0), (cb // 2, cb)]
    ins = [b"", html[:99], html[50:50 + 2 * cb]]
    isrc, isrc_off, isrc_len = H.pack(ins)
    out2, off2, len2, st2, ix2 = cd.frame_splice_to_memory(framed, off, lens, index, H.dev([q[0] for q in edits]), H.dev([q[1] for q in edits]), isrc,
                                                           H.dev(isrc_off), H.dev(isrc_len), cb)
    assert st2.tolist() == [O.OK] * ns
    h = out2.cpu().numpy()
    spliced = [h[o:o + n].tobytes() for o, n in zip(off2.tolist(), len2.tolist())]
    assert spliced == S.splice_plan(rc.after(), rc.got["index"], edits, ins, cb)["streams"]
    # ... and the spliced streams with the splice's index through the wrapper that sizes the rechunk: canonical again, and then left alone
    out3, off3, len3, st3, ix3 = cd.frame_rechunk_to_memory(out2, off2, len2, ix2, cb)
    assert st3.tolist() == [O.OK] * ns
    h = out3.cpu().numpy()
    final = [h[o:o + n].tobytes() if n else s for o, n, s in zip(off3.tolist(), len3.tolist(), spliced)]
    assert final == [K.stream_of(S.edited(x, q[0], q[1], s), cb) for x, q, s in zip(now, edits, ins)]
    want = X.build_index(final)
    used = int(ix3.first[-1])
    assert ix3.first.tolist() == want["first"] and ix3.start[:used].tolist() == want["start"] and ix3.pos[:used].tolist() == want["pos"]
    fin, foff, flen = H.pack(final)
    out4, off4, len4, st4, ix4 = cd.frame_rechunk_to_memory(fin, H.dev(foff), H.dev(flen), ix3, cb)
    assert st4.tolist() == [O.OK] * ns and len4.tolist() == [0] * ns and out4.numel() == 0 and ix4.pos[:used].tolist() == want["pos"]
    assert ix4.result.tolist()[5] == ns


# ---- 4: splice, splice, rechunk on one context, no synchronisation between them ------------------------------------------------------------------------------
@pytest.mark.parametrize("cb", [100, 65536])
def test_two_splices_and_a_rechunk_in_a_row(html, cb):
    cd = SB.BlockCodec(0, O.HASH_CRC32C)
    raws = [html[:2 * cb + cb // 3], html[3:3 + cb], html[:4 * cb]]
    streams = [K.stream_of(x, cb) for x in raws]
    ix = X.build_index(streams)
    steps = [[(cb // 2, 0, cb + 1), (0, cb // 2, 0), (cb, 2 * cb, 5)], [(0, 10, 0), (1, 0, 3 * cb), (7, 0, 1)]]
    # the model runs ahead, so that every call is sized without reading anything back
    plans, ms, mix = [], streams, ix
    for k, step in enumerate(steps):
        srcs = [html[1000 * k + 17 * b:1000 * k + 17 * b + q[2]] for b, q in enumerate(step)]
        w = S.splice_plan(ms, mix, [q[:2] for q in step], srcs, cb)
        assert w["status"] == [O.OK] * 3
        plans.append((step, srcs, w))
        raws = [S.edited(x, q[0], q[1], s) for x, q, s in zip(raws, step, srcs)]
        ms, mix = w["streams"], w["index"]
    want = RC.rechunk_plan(ms, mix, cb)
    assert RC.after(ms, want) == [K.stream_of(x, cb) for x in raws] and sum(1 for x in want["streams"] if x is not None) >= 2
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
    out_off, total = H.out_layout(np.array(want["out_bound"], dtype=np.int64))
    out = torch.full((total,), CANARY, dtype=torch.uint8, device="cuda")
    out_len, status, index, result = cd.frame_rechunk_indexed(framed, in_off, in_len, index, cb, out, H.dev(out_off), H.dev(want["out_bound"]),
                                                              want["result"][0], want["result"][2], want["result"][4])
    torch.cuda.synchronize()
    assert status.tolist() == [O.OK] * 3 and out_len.tolist() == want["out_len"] and result.tolist() == want["result"]
    h = out.cpu().numpy()
    assert [h[o:o + n].tobytes() if n else None for o, n in zip(out_off.tolist(), out_len.tolist())] == want["streams"]
    assert (H.outside_ranges(h, out_off.tolist(), out_len.tolist()) == CANARY).all()
    used = want["index"]["first"][-1]
    assert index.first.tolist() == want["index"]["first"] and index.start[:used].tolist() == want["index"]["start"]
    assert index.pos[:used].tolist() == want["index"]["pos"] and index.total.tolist() == want["index"]["total"] and index.tail.tolist() == [0] * 3
    assert X.build_index(RC.after(ms, want))["pos"] == want["index"]["pos"]


# ---- 5: graph capture ------------------------------------------------------------------------------------------------------------------------------------------
def test_graph_capture_replays_the_call(html):
    cd = SB.BlockCodec(0, O.HASH_CRC32C)
    cb = 4096
    streams, ix = mixed_batch(html)
    ns = len(streams)
    want = RC.rechunk_plan(streams, ix, cb)
    ms, sc, me = want["result"][0], want["result"][2], want["result"][4]
    framed, in_off, in_len = H.pack(streams)
    out_off, total = H.out_layout(np.array(want["out_bound"], dtype=np.int64))
    out = torch.full((total,), CANARY, dtype=torch.uint8, device="cuda")
    index = device_index(ix, ns)
    tabs = [H.dev(in_off), H.dev(in_len), H.dev(out_off), H.dev(want["out_bound"])]
    work = torch.empty(N.frame_rechunk_lib().snp_frame_rechunk_indexed_workspace(ns, ms, sc, cb, me), dtype=torch.uint8, device="cuda")

    def call():
        return cd.frame_rechunk_indexed(framed, tabs[0], tabs[1], index, cb, out, tabs[2], tabs[3], ms, sc, me, work=work)

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
    blobs = [html[:700], html[50:50 + 1024], html[9:9 + 1300], html[:100], html[:2000]]
    streams = [K.stream_of(x, 500) for x in blobs[:3]] + [K.stream_of(blobs[3], cb), K.stream_of(blobs[4], 300)]
    ix = X.build_index(streams)
    full = Rechunked(cd, streams, ix, cb).check()
    assert full.got["status"] == [O.OK] * 5
    sizing = Rechunked(cd, streams, ix, cb, caps=[0] * 5, max_slots=0, stage_cap=0, max_entries=0).check()
    ms, _, sc, _, me, alone = sizing.got["result"]
    assert (ms, sc, me, alone) == (15, 5024, 16, 1) and sizing.got["streams"] == [None] * 5 and sizing.got["out_bound"] == full.got["out_bound"]
    late = [O.OK, O.OK, O.OK, O.OK, O.ERR_OUTPUT_TOO_SMALL]
    mid = [O.OK, O.ERR_OUTPUT_TOO_SMALL, O.ERR_OUTPUT_TOO_SMALL, O.OK, O.ERR_OUTPUT_TOO_SMALL]
    assert Rechunked(cd, streams, ix, cb, max_slots=ms - 1).check().got["status"] == late
    assert Rechunked(cd, streams, ix, cb, stage_cap=sc - 1).check().got["status"] == late
    assert Rechunked(cd, streams, ix, cb, max_entries=me - 1).check().got["status"] == late
    assert Rechunked(cd, streams, ix, cb, max_slots=4).check().got["status"] == mid
    assert Rechunked(cd, streams, ix, cb, stage_cap=700 + 1023).check().got["status"] == mid
    assert Rechunked(cd, streams, ix, cb, max_entries=4).check().got["status"] == mid
    caps = list(full.got["out_len"])
    caps[2] -= 1                                                        # one byte short, in the middle of the batch
    one = Rechunked(cd, streams, ix, cb, caps=caps).check()
    assert one.got["status"] == [O.OK, O.OK, O.ERR_OUTPUT_TOO_SMALL, O.OK, O.OK] and one.got["result"][3] == 3
    walked_like(cd, one)


def test_corruption_in_a_dirty_chunk_in_a_kept_chunk_and_the_scrub(html):
    cd = SB.BlockCodec(0, O.HASH_CRC32C)
    cb = 4096
    s0 = K.stream_of(html[:5 * cb], cb)
    s = S.splice_plan([s0], X.build_index([s0]), [(cb + 100, 50)], [b""], cb)["streams"][0]
    rows = R.walk(s)[0]
    bad = [R.corrupt_chunk(s, rows[i]) for i in (0, 1, 3)]
    both = R.corrupt_chunk(bad[1], rows[3])
    want1, want3 = M.chunk_status(bad[1], rows[1]), M.chunk_status(bad[2], rows[3])
    ix = X.build_index([s] * 5)
    rc = Rechunked(cd, bad + [s, both], ix, cb).check()
    assert rc.got["status"] == [O.OK, want1, want3, O.OK, want1] and want1 != O.OK != want3
    assert rc.got["streams"][0] != rc.got["streams"][3] and rc.got["result"][3] == 2
    scrub = Rechunked(cd, bad + [s, both], ix, cb, ALL).check()
    assert scrub.got["status"][0] != O.OK and scrub.got["result"][3] == 1


def test_unsound_indexes_keep_every_guard_and_canary(named):
    names, streams, ix = named
    cd = SB.BlockCodec(0, O.HASH_CRC32C)
    rng = np.random.default_rng(5)
    bad = RC.unsound_indexes(ix, streams, rng)
    assert len(bad) == 13
    refused = 0
    for k, index in enumerate(bad):
        ne = min(len(index["start"]), len(index["pos"]))
        rc = Rechunked(cd, streams, index, 4096, ALL * (k & 1), caps=[len(s) + 70000 for s in streams], max_slots=1 << 12, stage_cap=1 << 25,
                       max_entries=ne + 64)
        rc.check()                                                      # guards and canaries held inside; every status is the model's
        refused += sum(1 for s in rc.got["status"] if s == O.ERR_BAD_ARG)
    assert refused > 40


def test_empty_calls_and_a_batch_that_is_canonical(html):
    cd = SB.BlockCodec(0, O.HASH_CRC32C)
    cd._bind()
    call = N.frame_rechunk_lib().snp_frame_rechunk_indexed_batch
    result = Guarded(6, torch.int64)
    assert call(cd.ctx.handle, *[None] * 3, 0, *[None] * 5, 0, 4096, 0, 0, 0, 0, *[None] * 5, *[None] * 5, None, None, result.ptr()) == O.OK
    torch.cuda.synchronize()
    assert result.read() == [0] * 6
    streams = [K.stream_of(html[:n], 1000) for n in (2500, 0, 1000)]
    ix = X.build_index(streams)
    rc = Rechunked(cd, streams, ix, 1000, max_slots=3, stage_cap=5000, max_entries=9).check()
    assert rc.got["status"] == [O.OK] * 3 and rc.got["result"] == [0, 0, 0, 0, 4, 3] and RC.same_index(rc.got["index"], ix)
    rc = Rechunked(cd, [b"", b""], X.build_index([b"", b""]), 1000).check()               # in_len == 0: the identifier
    assert rc.got["streams"] == [M.STREAM_ID] * 2 and rc.got["result"] == [0, 20, 0, 2, 0, 0]


# ---- 7: launch tiers ---------------------------------------------------------------------------------------------------------------------------------------------
def test_the_slot_bound_picks_the_tier_of_both_tables_and_changes_nothing(html):
    cd = SB.BlockCodec(0, O.HASH_CRC32C)
    streams, ix = mixed_batch(html)
    exact = Rechunked(cd, streams, ix, 1000).check()
    tiers = [cd.ctx.get_option(getattr(N, o)) for o in ("OPT_COMPRESS_WINDOW_DUAL_MIN_BATCH", "OPT_COMPRESS_WINDOW_GLOBAL_MIN_BATCH",
                                                        "OPT_SMALL_BLOCK_MIN_BATCH", "OPT_COMPRESS_WINDOW_MAX_BATCH")]
    assert tiers[0] == 1536 and tiers[2:] == [4096, 32768]
    for ms in [t - d for t in tiers for d in (1, 0)]:
        rc = Rechunked(cd, streams, ix, 1000, caps=exact.caps, max_slots=ms).check()
        assert np.array_equal(rc.h, exact.h) and rc.got == exact.got, ms


def test_real_slots_on_the_lane_compressor(html):
    """33 000 one-byte chunks from three streams of 11 000 bytes at 1 000-byte chunks: past the window compressor's range."""
    cd = SB.BlockCodec(0, O.HASH_CRC32C)
    raws = [html[b:b + 11000] for b in range(3)]
    streams = [K.stream_of(x, 1000) for x in raws]
    ix = X.build_index(streams)
    caps = [10 + 9 * 11000] * 3
    rc = Rechunked(cd, streams, ix, 1, caps=caps, max_slots=33000, stage_cap=33000, max_entries=33000, model=False)
    assert rc.got["result"] == [33000, 3 * caps[0], 33000, 3, 33000, 0] and 33000 >= cd.ctx.get_option(N.OPT_COMPRESS_WINDOW_MAX_BATCH)
    assert rc.got["status"] == [O.OK] * 3 and rc.after() == [K.stream_of(x, 1) for x in raws]
    assert rc.got["index"]["start"] == list(range(11000)) * 3 and rc.got["index"]["pos"] == [10 + 9 * k for k in range(11000)] * 3
    # ... and back: 33 000 dirty rows on the decoder's list path, 33 slots
    back = Rechunked(cd, rc.after(), rc.got["index"], 1000, caps=[len(s) for s in streams], max_slots=33000, stage_cap=33000, max_entries=33000,
                     model=False)
    assert back.got["status"] == [O.OK] * 3 and back.after() == streams and back.got["result"][0] == 33000 and back.got["result"][4] == 33000


def test_real_rows_on_the_decoders_list_path(html):
    """4 100 dirty rows: 41 streams of 100 chunks of 64 bytes, rechunked to 100-byte chunks."""
    cd = SB.BlockCodec(0, O.HASH_CRC32C)
    raws = [html[b:b + 6400] for b in range(41)]
    streams = [K.stream_of(x, 64) for x in raws]
    rc = Rechunked(cd, streams, X.build_index(streams), 100).check()
    assert rc.got["result"][0] == 4100 >= cd.ctx.get_option(N.OPT_SMALL_BLOCK_MIN_BATCH) and rc.got["result"][3] == 41
    assert rc.after() == [K.stream_of(x, 100) for x in raws]


# ---- 8: every layout -------------------------------------------------------------------------------------------------------------------------------------------------
_default = {}


def default_run(html, variant):
    if variant not in _default:
        streams, ix = mixed_batch(html, variant)
        _default[variant] = (streams, ix, Rechunked(SB.BlockCodec(0, variant), streams, ix, 1000, variant=variant).check())
    return _default[variant]


@pytest.mark.parametrize("crc", [0, 1, 2])
@pytest.mark.parametrize("layout", layouts.COMPRESS_LAYOUTS)
def test_every_compress_layout_and_crc_kernel(html, layout, crc):
    for variant in VARIANTS:
        streams, ix, base = default_run(html, variant)
        cd = SB.BlockCodec(0, variant)
        layouts.set_compress_layout(cd.ctx, layout)
        cd.ctx.set_option(N.OPT_CRC_KERNEL, crc)
        rc = Rechunked(cd, streams, ix, 1000, caps=base.caps, max_slots=base.ms, stage_cap=base.sc, max_entries=base.me, variant=variant, model=False)
        rc.want = base.want
        rc.check()
        assert np.array_equal(rc.h, base.h)


@pytest.mark.parametrize("fenced", [0, 1])
@pytest.mark.parametrize("decode", layouts.DECODE_LAYOUTS)
def test_every_decode_layout(html, decode, fenced):
    streams, ix, base = default_run(html, O.HASH_CRC32C)
    cd = SB.BlockCodec(0, O.HASH_CRC32C)
    layouts.set_decode_layout(cd.ctx, decode, fenced)
    rc = Rechunked(cd, streams, ix, 1000, caps=base.caps, max_slots=base.ms, stage_cap=base.sc, max_entries=base.me, model=False)
    rc.want = base.want
    rc.check()
    assert np.array_equal(rc.h, base.h)


# ---- 9: past 4 GiB ---------------------------------------------------------------------------------------------------------------------------------------------------
def test_a_kept_prefix_that_ends_past_position_2_to_the_32(html):
    """One stream of 66 000 uncompressed chunks of 65 536 bytes -- clean rows that are copied, 4.03 GiB of them -- then a short chunk and a tail off
    the grid, which are rebuilt behind position 2^32 of both streams."""
    cb, nkept = 65536, 66000
    free = torch.cuda.mem_get_info()[0]
    if free < 20 << 30:
        pytest.skip(f"needs 20 GiB of free device memory, {free >> 30} GiB free")
    cd = SB.BlockCodec(0, O.HASH_CRC32C)
    piece = np.frombuffer(html[:cb], dtype=np.uint8)
    one = M.data_chunk(piece.tobytes(), compressed=False)
    tail_raw = html[100:100 + 1000] + html[5000:5000 + cb + 300]
    tail = M.data_chunk(tail_raw[:1000]) + M.data_chunk(tail_raw[1000:1000 + cb]) + M.data_chunk(tail_raw[1000 + cb:])
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
    fresh = K.chunks_of(tail_raw, cb)
    want_len = 10 + kept_bytes + sum(len(c) for c in fresh)
    cap = 10 + kept_bytes + 8 * len(fresh) + len(tail_raw)
    out = torch.full((cap + 64,), CANARY, dtype=torch.uint8, device="cuda")
    out_len, status, new_ix, result, bound = cd.frame_rechunk_indexed(buf, H.dev([0]), H.dev([n]), index, cb, out, H.dev([0]), H.dev([cap]), 3,
                                                                      len(tail_raw), nkept + 3, with_bound=True)
    assert status.tolist() == [O.OK] and out_len.tolist() == [want_len] and bound.tolist() == [cap]
    assert result.tolist() == [3, want_len, len(tail_raw), 1, nkept + 3, 0]
    assert torch.equal(out[:10 + kept_bytes], buf[:10 + kept_bytes]) and bool((out[want_len:] == CANARY).all())
    assert out[10 + kept_bytes:want_len].cpu().numpy().tobytes() == b"".join(fresh)
    used = nkept + len(fresh)
    assert new_ix.first.tolist() == [0, used] and torch.equal(new_ix.start[:used], torch.arange(used, dtype=torch.int64, device="cuda") * cb)
    assert torch.equal(new_ix.pos[:nkept], pos[:nkept]) and new_ix.pos[nkept:used].tolist() == [10 + kept_bytes, 10 + kept_bytes + len(fresh[0])]
    # the rebuilt bytes, past position 2^32 of the new stream, read back through the new index
    back = torch.empty(len(tail_raw), dtype=torch.uint8, device="cuda")
    rl, rs, _ = cd.frame_read_indexed(out, H.dev([0]), out_len, new_ix, torch.zeros(1, dtype=torch.int32, device="cuda"), H.dev([nkept * cb]),
                                      H.dev([len(tail_raw)]), back, H.dev([0]), H.dev([len(tail_raw)]))
    assert rs.tolist() == [O.OK] and rl.tolist() == [len(tail_raw)] and back.cpu().numpy().tobytes() == tail_raw


# ---- rebuilt chunks stored compressed and stored raw, at the chunk sizes whose emit teams are 64, 128 and 256 threads --------------------------------
@pytest.mark.parametrize("cb", SC.TEAM_CHUNK_SIZES)
def test_rebuilt_chunks_raw_and_compressed_at_every_team_size(cb):
    cd = SB.BlockCodec(0, O.HASH_CRC32C)
    blobs = SC.team_blobs(cb)
    streams = [K.stream_of(x, cb // 2 + 1) for x in blobs]              # no old chunk but the first ends on a boundary of the new ones
    rc = Rechunked(cd, streams, X.build_index(streams), cb).check()
    assert rc.got["status"] == [O.OK] * 3 and rc.got["result"][3] == 3
    assert rc.after() == [K.stream_of(x, cb) for x in blobs]
    assert [SC.chunk_types(s) for s in rc.after()[:2]] == [{1}, {0}]

"""snp_frame_append_indexed_batch (BlockCodec.frame_append_indexed / frame_append_to_memory): every new stream, status, length, size bound, index
array and d_result against the model (frame_append_model.py), with every stream in a canary-filled region and guard words around every array and
the workspace (append_harness.Appended); whole-arena equality with snp_frame_encode_chunked_batch of A || S; the new index against
snp_frame_index_batch, through snp_frame_read_indexed_batch and under snp_frame_write_indexed_batch; sequences of appends without
synchronisation; graph capture; foreign streams and mixed batches; admission; unsound indexes; a corrupt reopened tail; empty calls; the launch
tiers of the compressor and the decoder by bound and by real count; a stream past 4 GiB.  Needs an MI355X."""
import numpy as np
import pytest
import torch

import frame_append_model as A
import frame_buffers_helpers as H
import frame_buffers_model as M
import frame_chunked_model as K
import frame_index_model as X
import frame_range_model as R
import oracle as O
import seekable_cases as SC
from append_harness import Appended, arena_of
from conftest import read_testdata
from seekable_harness import CANARY, Guarded, index_call, index_tensors

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from snappier_amd import batch as SB, _native as N

VARIANTS = [O.HASH_CRC32C, O.HASH_MUL]


@pytest.fixture(scope="module")
def html():
    return read_testdata("html") * 4


@pytest.fixture(scope="module")
def named():
    cases = X.named_streams()
    streams = list(cases.values())
    return list(cases), streams, X.build_index(streams)


def grid(html, cb, variant):
    """Every A-length against every S-length: -> (blobs, streams, srcs)."""
    blobs = [html[7:7 + na] for na in A.a_lengths(cb) for _ in A.s_lengths(cb)]
    srcs = [html[11 + na:11 + na + n] for na in A.a_lengths(cb) for n in A.s_lengths(cb)]
    return blobs, [K.stream_of(x, cb, variant) for x in blobs], srcs


def read_back(cd, a, windows):
    """(stream, off, len) windows read through the index the append wrote: -> bytes per window."""
    buf, buf_off, new_len = a.table()
    lens = [w[2] for w in windows]
    out_off = np.cumsum([0] + lens[:-1])
    out = torch.full((max(sum(lens), 1),), CANARY, dtype=torch.uint8, device="cuda")
    rl, rs, _ = cd.frame_read_indexed(buf, buf_off, new_len, a.frame_index(), torch.tensor([w[0] for w in windows], dtype=torch.int32, device="cuda"),
                                      H.dev([w[1] for w in windows]), H.dev(lens), out, H.dev(out_off), H.dev(lens))
    assert rs.tolist() == [O.OK] * len(windows) and rl.tolist() == lens
    h = out.cpu().numpy()
    return [h[o:o + n].tobytes() for o, n in zip(out_off, lens)]


# ---- 1: chunk sizes x A-lengths x S-lengths; the whole arena is the chunked encode's; the new index is the walk's and the encoder's -------------
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("cb", [1, 64, 4096, 65536])
def test_append_leaves_the_chunked_encode_of_the_concatenation(html, cb, variant):
    cd = SB.BlockCodec(0, variant)
    blobs, streams, srcs = grid(html, cb, variant)
    ix = X.build_index(streams)
    a = Appended(cd, streams, ix, srcs, cb, variant=variant).check()
    assert set(a.got["status"]) == {O.OK}
    whole = [x + s for x, s in zip(blobs, srcs)]
    for b, x in enumerate(whole):
        assert a.after()[b] == K.stream_of(x, cb, variant), b
    # the encoder on A || S, into an arena of the same offsets and caps: the same bytes, canaries included, and the same index
    data, in_off, lens = H.pack(whole)
    out = torch.full_like(a.buf, CANARY)
    mc = sum(K.nchunks(len(x), cb) for x in whole)
    _, _, e_len, e_st, _, e_ix = cd.frame_encode_seekable(data, H.dev(in_off), H.dev(lens), cb, out=out, out_off=a.tabs[0], out_cap=a.tabs[2], max_chunks=mc,
                                                          work=torch.empty(N.frame_chunked_lib().snp_frame_encode_chunked_workspace(len(whole), mc, cb),
                                                                           dtype=torch.uint8, device="cuda"))
    assert e_st.tolist() == [O.OK] * len(whole) and torch.equal(e_len, a.new_len.mid)
    assert torch.equal(out, a.buf)
    new = a.frame_index()
    used = int(new.first[-1].item())
    assert used == mc and torch.equal(new.first, e_ix.first) and torch.equal(new.total, e_ix.total) and torch.equal(new.tail, e_ix.tail)
    assert torch.equal(new.start[:used], e_ix.start[:used]) and torch.equal(new.pos[:used], e_ix.pos[:used])
    walked = cd.frame_index_buffers(*a.table())
    assert torch.equal(walked.first, new.first) and torch.equal(walked.start, new.start[:used]) and torch.equal(walked.pos, new.pos[:used])
    assert torch.equal(walked.total, new.total) and torch.equal(walked.tail, new.tail)
    # every appended byte range read back through the new index
    windows = [(b, len(x), len(s)) for b, (x, s) in enumerate(zip(blobs, srcs)) if s]
    assert read_back(cd, a, windows) == [s for s in srcs if s]


# ---- 2: an update made through the new index ------------------------------------------------------------------------------------------------------
def test_an_update_through_the_new_index_succeeds(html):
    cd = SB.BlockCodec(0, O.HASH_CRC32C)
    cb = 4096
    blobs = [html[:3 * cb + 100], html[5:5 + cb], b""]
    srcs = [html[30000:30000 + 2 * cb], html[9:9 + 10], html[:cb + 1]]
    streams = [K.stream_of(x, cb) for x in blobs]
    a = Appended(cd, streams, X.build_index(streams), srcs, cb).check()
    whole = [x + s for x, s in zip(blobs, srcs)]
    # one request per stream, across the seam between the old bytes and the appended ones
    reqs = [(b, max(len(x) - 5, 0), min(10, len(w))) for b, (x, w) in enumerate(zip(blobs, whole))]
    data = [bytes([65 + b]) * ln for b, _, ln in reqs]
    src, src_off, src_len = H.pack(data)
    buf, buf_off, new_len = a.table()
    out, out_off, out_len, status, req_status, _ = cd.frame_update_to_memory(buf, buf_off, new_len, a.frame_index(),
                                                                             torch.tensor([q[0] for q in reqs], dtype=torch.int32, device="cuda"),
                                                                             H.dev([q[1] for q in reqs]), src, H.dev(src_off), H.dev(src_len))
    assert status.tolist() == [O.OK] * 3 and req_status.tolist() == [O.OK] * 3
    h = out.cpu().numpy()
    for b, (_, off, ln) in enumerate(reqs):
        patched = whole[b][:off] + data[b] + whole[b][off + ln:]
        o, n = int(out_off[b]), int(out_len[b])
        assert h[o:o + n].tobytes() == K.stream_of(patched, cb), b


# ---- 3: five appends on one context, no synchronisation between them --------------------------------------------------------------------------------
@pytest.mark.parametrize("cb", [100, 65536])
def test_five_appends_in_a_row_leave_the_encode_of_the_concatenation(html, cb):
    cd = SB.BlockCodec(0, O.HASH_CRC32C)
    blobs = [html[:2 * cb + cb // 3], b"", html[3:3 + cb], html[:1]]
    parts = [[html[1000 * k + 17 * b:1000 * k + 17 * b + n] for b, n in enumerate((cb // 2, 3 * cb + 1, 1, (k % 2) * (cb + 5)))] for k in range(5)]
    whole = [x + b"".join(p[b] for p in parts) for b, x in enumerate(blobs)]
    streams = [K.stream_of(x, cb) for x in blobs]
    caps = [len(K.stream_of(x, cb)) + 64 for x in whole]
    buf, off = arena_of(streams, caps)
    ix = X.build_index(streams)
    index = SB.FrameIndex(*index_tensors(ix, 4)[0])
    index.start, index.pos = index.start[:len(ix["start"])], index.pos[:len(ix["pos"])]
    buf_off, buf_cap, buf_len = H.dev(off), H.dev(caps), H.dev([len(s) for s in streams])
    keep = []
    for p in parts:                                                     # sized by the model, so that nothing is read back between the calls
        src, src_off, src_len = H.pack(p)
        keep.append(src)
        mt, ms = 4, sum(K.nchunks(len(x), cb) for x in p)
        buf_len, status, index, _, _ = cd.frame_append_indexed(buf, buf_off, buf_len, buf_cap, index, src, H.dev(src_off), H.dev(src_len), cb, mt, ms)
    torch.cuda.synchronize()
    assert status.tolist() == [O.OK] * 4
    want = [K.stream_of(x, cb) for x in whole]
    assert buf_len.tolist() == [len(w) for w in want]
    h = buf.cpu().numpy()
    for b, w in enumerate(want):
        assert h[off[b]:off[b] + len(w)].tobytes() == w, b
    assert (H.outside_ranges(h, off, [len(w) for w in want]) == CANARY).all()
    after = X.build_index(want)
    used = after["first"][-1]
    assert index.first.tolist() == after["first"] and index.start[:used].tolist() == after["start"] and index.pos[:used].tolist() == after["pos"]
    assert index.total.tolist() == after["total"] and index.tail.tolist() == after["tail"]


# ---- 4: graph capture ------------------------------------------------------------------------------------------------------------------------------
def test_graph_capture_replays_the_call(html):
    cd = SB.BlockCodec(0, O.HASH_CRC32C)
    cb = 4096
    blobs = [html[:3 * cb + 700], html[11:11 + cb], b"", html[5:5 + 9000]]
    srcs = [html[40000:40000 + 2 * cb + 3], html[:50], html[7:7 + cb], b""]
    streams = [K.stream_of(x, cb) for x in blobs]
    ix = X.build_index(streams)
    want = A.append_plan(streams, ix, srcs, cb)
    caps = [len(x or s) + 64 for x, s in zip(want["streams"], streams)]
    mt, ms = want["result"][2], want["result"][0]
    start_buf, off = arena_of(streams, caps)
    buf = start_buf.clone()
    index = SB.FrameIndex(*index_tensors(ix, 4)[0])
    index.start, index.pos = index.start[:len(ix["start"])], index.pos[:len(ix["pos"])]
    src, src_off, src_len = H.pack(srcs)
    tabs = [H.dev(off), H.dev([len(s) for s in streams]), H.dev(caps), H.dev(src_off), H.dev(src_len)]
    work = torch.empty(N.frame_append_lib().snp_frame_append_indexed_workspace(4, mt, ms, cb), dtype=torch.uint8, device="cuda")

    def call():
        return cd.frame_append_indexed(buf, tabs[0], tabs[1], tabs[2], index, src, tabs[3], tabs[4], cb, mt, ms, work=work)

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        call()                                                          # the warm-up call, and the call whose bytes the replay must leave
        torch.cuda.synchronize()
        plain = buf.clone()
        buf.copy_(start_buf)
        call()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    assert torch.equal(buf, plain)
    buf.copy_(start_buf)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        new_len, status, new_ix, result, _ = call()
    buf.copy_(start_buf)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(buf, plain)
    assert status.tolist() == want["status"] and new_len.tolist() == want["new_len"] and result.tolist() == want["result"]
    used = want["index"]["first"][-1]
    assert new_ix.first.tolist() == want["index"]["first"] and new_ix.pos[:used].tolist() == want["index"]["pos"]
    h = buf.cpu().numpy()
    for b, x in enumerate(want["streams"]):
        if x is not None:
            assert h[off[b]:off[b] + len(x)].tobytes() == x, b


# ---- 5: foreign streams; a mixed batch ---------------------------------------------------------------------------------------------------------------
def test_named_foreign_streams(html, named):
    names, streams, ix = named
    cd = SB.BlockCodec(0, O.HASH_CRC32C)
    srcs = [html[b:b + 5000 + 13 * b] for b in range(len(streams))]
    a = Appended(cd, streams, ix, srcs, 4096).check()
    written = sum(1 for x in a.got["streams"] if x is not None)
    assert written >= 10 and len(streams) - written >= 5 and len(set(a.got["status"])) >= 4      # (the floor the model meets on the CPU)
    assert index_call(cd, a.after()) == {**a.got["index"], "result": X.build_index(a.after())["result"]}
    windows = [(b, ix["total"][b], len(srcs[b])) for b, x in enumerate(a.got["streams"]) if x is not None]
    assert read_back(cd, a, windows) == [srcs[b] for b, _, _ in windows]


def test_the_tails_the_contract_tells_apart(html):
    cd = SB.BlockCodec(0, O.HASH_CRC32C)
    cb = 1000
    shapes = A.tail_shapes(html, cb)
    streams = [s for s, _ in shapes.values()]
    src = html[5000:5000 + 2 * cb + 17]
    a = Appended(cd, streams, X.build_index(streams), [src] * len(streams), cb).check()
    assert a.got["status"] == [O.OK] * len(streams) and a.got["result"][2] == 2
    for b, (name, (s, reopened)) in enumerate(shapes.items()):
        assert (a.got["streams"][b][:len(s)] == s) == (not reopened), name
        assert O.frame_decode(a.got["streams"][b]) == O.frame_decode(s) + src, name


def test_a_mixed_batch_written_refused_broken_and_unnamed(html, named):
    names, streams, ix = named
    cd = SB.BlockCodec(0, O.HASH_MUL)
    cb = 512
    mine = [K.stream_of(html[:n], cb, O.HASH_MUL) for n in (700, 1024, 1300, 100)] + [b""]
    broken = [s for s, t in zip(streams, ix["tail"]) if t != O.OK][:3]
    batch = [mine[0], broken[0], mine[1], mine[2], broken[1], mine[3], mine[4], broken[2]]
    srcs = [html[3000:3000 + n] for n in (1000, 50, 513, 100, 0, 0, 2000, 7)]
    bix = X.build_index(batch)
    free = A.append_plan(batch, bix, srcs, cb, variant=O.HASH_MUL)
    caps = [max(bd, len(s)) for bd, s in zip(free["out_bound"], batch)]
    caps[2] = free["new_len"][2] - 1                                    # refused: its region is one byte short
    a = Appended(cd, batch, bix, srcs, cb, caps=caps, variant=O.HASH_MUL).check()
    assert a.got["status"] == [O.OK, bix["tail"][1], O.ERR_OUTPUT_TOO_SMALL, O.OK, O.OK, O.OK, O.OK, bix["tail"][7]]
    assert [x is not None for x in a.got["streams"]] == [True, False, False, True, False, False, True, False]
    assert index_call(cd, a.after())["pos"] == a.got["index"]["pos"]


# ---- 6: admission ------------------------------------------------------------------------------------------------------------------------------------
def test_admission_by_each_bound_and_by_buf_cap(html):
    cd = SB.BlockCodec(0, O.HASH_CRC32C)
    cb = 512
    streams = [K.stream_of(x, cb) for x in (html[:700], html[50:50 + 1024], html[9:9 + 1300], html[:100], b"")]
    ix = X.build_index(streams)
    srcs = [html[3000:3000 + n] for n in (1000, 513, 100, 0, 2000)]
    full = Appended(cd, streams, ix, srcs, cb).check()
    # the sizing call: nothing written, the needs and the bounds reported
    sizing = Appended(cd, streams, ix, srcs, cb, max_tails=0, max_slots=0).check()
    slots, _, tails, _ = sizing.got["result"]
    assert (tails, slots) == (2, 8) and sizing.got["streams"] == [None] * 5 and sizing.got["out_bound"] == full.got["out_bound"]
    assert all(bd >= n for bd, n in zip(sizing.got["out_bound"], full.got["new_len"]))
    short = Appended(cd, streams, ix, srcs, cb, max_slots=slots - 1).check()
    assert short.got["status"] == [O.OK, O.OK, O.OK, O.OK, O.ERR_OUTPUT_TOO_SMALL]
    short = Appended(cd, streams, ix, srcs, cb, max_tails=tails - 1).check()
    assert short.got["status"] == [O.OK, O.OK, O.ERR_OUTPUT_TOO_SMALL, O.OK, O.ERR_OUTPUT_TOO_SMALL]
    caps = list(full.got["new_len"])
    caps[1] -= 1                                                        # one byte short, in the middle of the batch
    mid = Appended(cd, streams, ix, srcs, cb, caps=caps).check()
    assert mid.got["status"] == [O.OK, O.ERR_OUTPUT_TOO_SMALL, O.OK, O.OK, O.OK] and mid.got["result"][3] == 3
    # max_tails = 0 with only short appends: every stream needs its tail, none is written; with room for the tails no fresh slot is needed
    tails_only = [K.stream_of(html[:n], cb) for n in (700, 100, 513)]
    tix = X.build_index(tails_only)
    few = [html[:5], html[:1], html[:200]]
    none = Appended(cd, tails_only, tix, few, cb, max_tails=0, max_slots=4).check()
    assert none.got["status"] == [O.ERR_OUTPUT_TOO_SMALL] * 3 and none.got["result"] == [0, 0, 3, 0]
    assert Appended(cd, tails_only, tix, few, cb, max_tails=3, max_slots=0).check().got["status"] == [O.OK] * 3


# ---- 7: the index is untrusted ---------------------------------------------------------------------------------------------------------------------
def test_unsound_indexes_keep_every_guard_and_canary(html, named):
    names, streams, ix = named
    cd = SB.BlockCodec(0, O.HASH_CRC32C)
    rng = np.random.default_rng(5)
    srcs = [html[b:b + 3000] for b in range(len(streams))]
    ns = len(streams)
    bad = A.unsound_indexes(ix, streams, rng)
    assert len(bad) == 13
    refused = 0
    for k, index in enumerate(bad):
        a = Appended(cd, streams, index, srcs, 4096, caps=[len(s) + 3100 for s in streams], max_tails=ns, max_slots=2 * ns)
        a.check()                                                       # guards and canaries held inside; every status is the model's
        refused += sum(1 for s in a.got["status"] if s == O.ERR_BAD_ARG)
    assert refused > 40


def test_a_corrupt_reopened_tail_gives_its_stream_the_chunks_status(html):
    cd = SB.BlockCodec(0, O.HASH_CRC32C)
    cb = 4096
    s = K.stream_of(html[:3 * cb + 100], cb)
    rows = R.walk(s)[0]
    bad_tail, bad_early = R.corrupt_chunk(s, rows[3]), R.corrupt_chunk(s, rows[1])
    want = M.chunk_status(bad_tail, rows[3])
    assert want != O.OK
    a = Appended(cd, [bad_tail, bad_early, s], X.build_index([s] * 3), [html[20000:20000 + cb]] * 3, cb).check()
    assert a.got["status"] == [want, O.OK, O.OK] and a.got["streams"][0] is None and a.got["result"][3] == 2


# ---- 8: empty calls ----------------------------------------------------------------------------------------------------------------------------------
def test_empty_calls(html):
    cd = SB.BlockCodec(0, O.HASH_CRC32C)
    cd._bind()
    call = N.frame_append_lib().snp_frame_append_indexed_batch
    result = Guarded(4, torch.int64)
    assert call(cd.ctx.handle, *[None] * 4, 0, *[None] * 5, 0, *[None] * 3, 4096, 0, 0, *[None] * 7, None, None, result.ptr()) == O.OK
    torch.cuda.synchronize()
    assert result.read() == [0, 0, 0, 0]
    streams = [K.stream_of(html[:n], 1000) for n in (2500, 0, 1000)]
    ix = X.build_index(streams)
    a = Appended(cd, streams, ix, [b""] * 3, 1000, max_tails=2, max_slots=3).check()
    assert a.got["status"] == [O.OK] * 3 and a.got["result"] == [0, 0, 0, 0] and A.same_index(a.got["index"], ix)
    # ... whatever the index holds: nothing of it is trusted for a stream that takes nothing
    a = Appended(cd, streams, {**ix, "tail": [5, 77, -3]}, [b""] * 3, 1000, max_tails=0, max_slots=0).check()
    assert a.got["status"] == [O.OK] * 3 and a.got["index"]["tail"] == [5, 77, -3]


def test_the_wrapper_sizes_and_appends(html):
    cd = SB.BlockCodec(0, O.HASH_CRC32C)
    cb = 1000
    blobs = [html[:2500], b"", html[:1000]]
    srcs = [html[9000:9000 + n] for n in (700, 2001, 1)]
    streams = [K.stream_of(x, cb) for x in blobs]
    want = [K.stream_of(x + s, cb) for x, s in zip(blobs, srcs)]
    buf, off = arena_of(streams, [len(w) + 9 for w in want])
    index = cd.frame_index_buffers(buf, H.dev(off), H.dev([len(s) for s in streams]))
    src, src_off, src_len = H.pack(srcs)
    new_len, status, new_ix = cd.frame_append_to_memory(buf, H.dev(off), H.dev([len(s) for s in streams]), H.dev([len(w) + 9 for w in want]), index, src,
                                                        H.dev(src_off), H.dev(src_len), cb)
    assert status.tolist() == [O.OK] * 3 and new_len.tolist() == [len(w) for w in want]
    h = buf.cpu().numpy()
    assert [h[o:o + len(w)].tobytes() for o, w in zip(off, want)] == want
    after = X.build_index(want)
    assert new_ix.first.tolist() == after["first"] and new_ix.pos.tolist() == after["pos"] and new_ix.start.tolist() == after["start"]


# ---- 9: launch tiers ---------------------------------------------------------------------------------------------------------------------------------
def tier_batch(html, cb=1000):
    """A dozen chunks of real work: tails reopened and not, fresh chunks, an empty stream."""
    blobs = [html[:2 * cb + 300], html[7:7 + cb], b"", html[3:3 + 10], html[:5 * cb]]
    srcs = [html[20000:20000 + 2 * cb], html[:cb // 2], html[9:9 + 3 * cb + 1], html[:1], html[100:100 + cb]]
    streams = [K.stream_of(x, cb) for x in blobs]
    return streams, X.build_index(streams), srcs


def test_the_bounds_pick_the_tier_and_change_nothing(html):
    cd = SB.BlockCodec(0, O.HASH_CRC32C)
    cb = 1000
    streams, ix, srcs = tier_batch(html, cb)
    exact = Appended(cd, streams, ix, srcs, cb).check()
    compress = [cd.ctx.get_option(getattr(N, o)) for o in ("OPT_COMPRESS_WINDOW_DUAL_MIN_BATCH", "OPT_COMPRESS_WINDOW_MAX_BATCH")]
    decode = cd.ctx.get_option(N.OPT_SMALL_BLOCK_MIN_BATCH)
    assert compress == [1536, 32768] and decode == 4096
    rows = len(ix["start"])
    for mt, ms in [(exact.mt, t - d) for t in compress for d in (1, 0)] + [(decode - d, exact.ms) for d in (1, 0)] + [(t - d, exact.ms) for t in compress for d in (1, 0)]:
        a = Appended(cd, streams, ix, srcs, cb, caps=exact.caps, max_tails=mt, max_slots=ms).check()
        assert np.array_equal(a.h, exact.h) and a.got == exact.got, (mt, ms)
        assert a.new[1].n == rows + ms


def test_real_rows_on_the_lane_compressor(html):
    """33 000 fresh slots of 64 bytes: past the window compressor's range."""
    cd = SB.BlockCodec(0, O.HASH_CRC32C)
    cb, ns, per = 64, 330, 100
    blobs = [html[b:b + (b % 3) * 50] for b in range(ns)]                # empty streams, streams with a short tail, streams with a tail of 36 bytes
    streams = [K.stream_of(x, cb) if x else b"" for x in blobs]
    srcs = [html[1000 + 7 * b:1000 + 7 * b + (cb - len(x) % cb) % cb + per * cb] for b, x in enumerate(blobs)]
    ix = X.build_index(streams)
    a = Appended(cd, streams, ix, srcs, cb).check()
    assert a.got["result"][0] == 33000 >= cd.ctx.get_option(N.OPT_COMPRESS_WINDOW_MAX_BATCH) and a.got["result"][3] == ns
    assert a.after() == [K.stream_of(x + s, cb) for x, s in zip(blobs, srcs)]


def test_real_rows_on_the_decoders_list_path(html):
    """4 100 reopened tails, one byte appended to each."""
    cd = SB.BlockCodec(0, O.HASH_CRC32C)
    cb, ns = 64, 4100
    blobs = [html[b:b + 70 + b % 50] for b in range(ns)]
    streams = [K.stream_of(x, cb) for x in blobs]
    srcs = [html[5 * b:5 * b + 1] for b in range(ns)]
    a = Appended(cd, streams, X.build_index(streams), srcs, cb).check()
    assert a.got["result"][2] == ns >= cd.ctx.get_option(N.OPT_SMALL_BLOCK_MIN_BATCH) and a.got["result"][0] == 0 and a.got["result"][3] == ns
    assert a.after() == [K.stream_of(x + s, cb) for x, s in zip(blobs, srcs)]


# ---- 10: past 4 GiB ------------------------------------------------------------------------------------------------------------------------------------
def test_one_stream_past_4_gib(html):
    cb, pad = 65536, (1 << 24) - 1
    npad = -(-((1 << 32) + 200_000 - 10) // (pad + 4))
    p0 = 10 + npad * (pad + 4)
    free = torch.cuda.mem_get_info()[0]
    if free < 12 << 30:
        pytest.skip(f"needs 12 GiB of free device memory, {free >> 30} GiB free")
    cd = SB.BlockCodec(0, O.HASH_CRC32C)
    old = html[:2 * cb + 30000]
    src = html[70000:170000]
    small = K.stream_of(old, cb)                                        # the tail alone: the same chunks behind the identifier
    six = X.build_index([small])
    want = A.append_plan([small], six, [src], cb)
    delta = p0 - 10
    n, room = delta + len(small), 200_000
    buf = torch.zeros(n + room, dtype=torch.uint8, device="cuda")        # the bodies of the padding chunks are never looked at
    buf[n:] = CANARY
    buf[:10] = torch.from_numpy(np.frombuffer(M.STREAM_ID, dtype=np.uint8).copy()).cuda()
    head = torch.from_numpy(np.frombuffer(bytes([0xFE]) + pad.to_bytes(3, "little"), dtype=np.uint8).copy()).cuda()
    for k in range(npad):
        buf[10 + k * (pad + 4):14 + k * (pad + 4)] = head
    buf[p0:n] = torch.from_numpy(np.frombuffer(small[10:], dtype=np.uint8).copy()).cuda()
    index = SB.FrameIndex(H.dev(six["first"]), H.dev(six["start"]), H.dev([p + delta for p in six["pos"]]), H.dev(six["total"]),
                          torch.tensor(six["tail"], dtype=torch.int32, device="cuda"))
    assert p0 > (1 << 32) + 200_000 and want["result"] == [1, want["new_len"][0] - len(small), 1, 1]
    data = torch.from_numpy(np.frombuffer(src, dtype=np.uint8).copy()).cuda()
    before = buf[p0:want["cut"][0] + delta].clone()
    new_len, status, new_ix, result, bound = cd.frame_append_indexed(buf, H.dev([0]), H.dev([n]), H.dev([n + room]), index, data, H.dev([0]),
                                                                     H.dev([len(src)]), cb, 1, 1, with_bound=True)
    assert status.tolist() == [O.OK] and new_len.tolist() == [want["new_len"][0] + delta] and result.tolist() == want["result"]
    assert bound.tolist() == [want["out_bound"][0] + delta]
    cut, end = want["cut"][0] + delta, want["new_len"][0] + delta
    assert cut > 1 << 32 and buf[cut:end].cpu().numpy().tobytes() == want["streams"][0][want["cut"][0]:]
    assert torch.equal(buf[p0:cut], before) and buf[:10].cpu().numpy().tobytes() == M.STREAM_ID and bool((buf[end:] == CANARY).all())
    assert new_ix.first.tolist() == want["index"]["first"] and new_ix.pos.tolist() == [p + delta for p in want["index"]["pos"]]
    assert new_ix.start.tolist() == want["index"]["start"] and new_ix.total.tolist() == want["index"]["total"]
    # the appended bytes, past position 2^32, read back through the new index
    back = torch.empty(len(src), dtype=torch.uint8, device="cuda")
    rl, rs, _ = cd.frame_read_indexed(buf, H.dev([0]), new_len, new_ix, torch.zeros(1, dtype=torch.int32, device="cuda"), H.dev([len(old)]),
                                      H.dev([len(src)]), back, H.dev([0]), H.dev([len(src)]))
    assert rs.tolist() == [O.OK] and rl.tolist() == [len(src)] and torch.equal(back, data)


# ---- rebuilt chunks stored compressed and stored raw, at the chunk sizes whose emit teams are 64, 128 and 256 threads --------------------------------
@pytest.mark.parametrize("cb", SC.TEAM_CHUNK_SIZES)
def test_rebuilt_chunks_raw_and_compressed_at_every_team_size(cb):
    cd = SB.BlockCodec(0, O.HASH_CRC32C)
    blobs = SC.team_blobs(cb)
    streams = [K.stream_of(x, cb) for x in blobs]
    srcs = [x[5:5 + cb + cb // 2] for x in blobs]                       # each stream's own kind of bytes: a reopened tail (0, 2) and fresh chunks
    a = Appended(cd, streams, X.build_index(streams), srcs, cb).check()
    assert a.got["status"] == [O.OK] * 3 and a.got["result"][2] == 2
    assert a.after() == [K.stream_of(x + s, cb) for x, s in zip(blobs, srcs)]
    assert [SC.chunk_types(s) for s in a.after()[:2]] == [{1}, {0}]

"""snp_frame_write_indexed_batch (BlockCodec.frame_write_indexed / frame_update_to_memory): every new stream, status, length, request status,
new position, size bound and d_result against the model (frame_update_model.py), with canary bytes around every output range and guard words
around every array and the workspace; whole-arena equality with snp_frame_encode_chunked_batch of the patched buffers; the new index against
snp_frame_index_batch and through snp_frame_read_indexed_batch; foreign streams; mixed batches; admission; corruption in an edge and in a
covered chunk; every request error; stale and unsound indexes; the seams of the emit's workgroups; a stream past 4 GiB; graph capture; empty
calls.  Needs an MI355X."""
import numpy as np
import pytest
import torch

import frame_buffers_helpers as H
import frame_buffers_model as M
import frame_chunked_model as K
import frame_index_model as X
import frame_range_model as R
import frame_update_model as U
import oracle as O
import seekable_cases as SC
from conftest import read_testdata
from seekable_harness import CANARY, Guarded, Updated, index_tensors

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from snappier_amd import batch as SB, _native as N

VARIANTS = [O.HASH_CRC32C, O.HASH_MUL]


def batch_of(blobs, cb, variant):
    streams = [K.stream_of(x, cb, variant) for x in blobs]
    return streams, X.build_index(streams)


def requests_for(blobs, cb, shape: int, rng):
    reqs = [(b, off, ln) for b, x in enumerate(blobs) for off, ln in U.request_shapes(len(x), cb)[shape] if x or not ln]
    return reqs, [U.fresh(rng, ln) for _, _, ln in reqs]


@pytest.fixture(scope="module")
def html():
    return read_testdata("html") * 3


@pytest.fixture(scope="module")
def named():
    cases = X.named_streams()
    streams = list(cases.values())
    return list(cases), streams, X.build_index(streams)


# ---- 1: chunk sizes x lengths x request shapes ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("cb", U.CHUNK_SIZES)
def test_chunk_sizes_lengths_and_request_shapes(html, cb, variant):
    cd = SB.BlockCodec(0, variant)
    blobs = [html[7:7 + n] for n in U.lengths(cb)]
    streams, ix = batch_of(blobs, cb, variant)
    rng = np.random.default_rng(cb + variant)
    for shape in range(10):
        reqs, srcs = requests_for(blobs, cb, shape, rng)
        u = Updated(cd, streams, ix, reqs, srcs, variant=variant).check()
        assert set(u.got["req_status"]) == {O.OK}, shape
        for b, x in enumerate(blobs):                                   # the consequence: the chunked encode of the patched buffer
            if u.got["streams"][b] is not None:
                assert u.got["streams"][b] == K.stream_of(U.patched(x, reqs, srcs, b), cb, variant), (shape, b)


# ---- 2: the whole arena is the chunked encode's; the new index is the walk's; the windows read back -----------------------------------------------
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("cb", [64, 4096, 65536])
def test_arena_equals_frame_encode_seekable_of_the_patched_buffers(html, cb, variant):
    cd = SB.BlockCodec(0, variant)
    blobs = [html[3:3 + n] for n in U.lengths(cb)[2:]]
    streams, ix = batch_of(blobs, cb, variant)
    rng = np.random.default_rng(cb)
    reqs, srcs = requests_for(blobs, cb, 2, rng)                        # head edge + interiors + tail edge, in every stream
    u = Updated(cd, streams, ix, reqs, srcs, variant=variant).check()
    assert u.got["status"] == [O.OK] * len(blobs) and all(x is not None for x in u.got["streams"])
    patched = [U.patched(x, reqs, srcs, b) for b, x in enumerate(blobs)]
    data, in_off, lens = H.pack(patched)
    arena = torch.full_like(u.out, CANARY)
    d_off, d_cap = H.dev(u.out_off), H.dev(u.caps)
    _, _, e_len, e_st, _, e_ix = cd.frame_encode_seekable(data, H.dev(in_off), H.dev(lens), cb, out=arena, out_off=d_off, out_cap=d_cap)
    torch.cuda.synchronize()
    assert e_st.tolist() == [O.OK] * len(blobs) and torch.equal(arena, u.out) and e_len.tolist() == u.got["out_len"]
    # the old index with new_pos is the index of the new streams, array for array
    walked = cd.frame_index_buffers(u.out, d_off, u.out_len.mid)
    ne = len(ix["start"])
    assert torch.equal(walked.pos, u.new_pos.mid) and torch.equal(walked.pos, e_ix.pos[:ne])
    for key, t in zip(("first", "start", "total", "tail"), (u.ix[0], u.ix[1], u.ix[3], u.ix[4])):
        assert torch.equal(getattr(walked, key), t[:getattr(walked, key).numel()]), key
    # the written windows read back through the new index
    live = [(q, s) for q, s in zip(reqs, srcs) if q[2]]
    caps = np.array([q[2] for q, _ in live], dtype=np.int64)
    r_off, total = H.out_layout(caps)
    back = torch.full((total,), CANARY, dtype=torch.uint8, device="cuda")
    new_ix = SB.FrameIndex(u.ix[0], u.ix[1][:ne], u.new_pos.mid, u.ix[3], u.ix[4])
    ol, st, _ = cd.frame_read_indexed(u.out, d_off, u.out_len.mid, new_ix, torch.tensor([q[0] for q, _ in live], dtype=torch.int32, device="cuda"),
                                      H.dev([q[1] for q, _ in live]), H.dev(caps), back, H.dev(r_off), H.dev(caps))
    torch.cuda.synchronize()
    assert st.tolist() == [O.OK] * len(live) and ol.tolist() == caps.tolist()
    h = back.cpu().numpy()
    for (q, s), o in zip(live, r_off.tolist()):
        assert h[o:o + q[2]].tobytes() == s


# ---- 3: foreign streams --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", range(7))
def test_foreign_streams(named, kind):
    names, streams, ix = named
    cd = SB.BlockCodec(0, O.HASH_CRC32C)
    rng = np.random.default_rng(kind)
    reqs = [(b, off, ln) for b, s in enumerate(streams) for off, ln in U.row_requests(s)[min(kind, len(U.row_requests(s)) - 1)]]
    srcs = [U.fresh(rng, ln) for _, _, ln in reqs]
    u = Updated(cd, streams, ix, reqs, srcs).check()
    written = [b for b, x in enumerate(u.got["streams"]) if x is not None]
    assert len(written) >= 10 and len(set(u.got["status"])) >= 3         # written streams, broken streams and refused requests in one batch
    for b in written:                                                   # skippable and padding chunks, identifiers, clean chunks: verbatim, in order
        s, new, at, out = streams[b], u.got["streams"][b], 0, 0
        for p, o, c in u.want["dirty"][b]:
            assert new[out:out + (p - at)] == s[at:p]
            out += p - at + len(c)
            at = p + o
        assert new[out:] == s[at:]


# ---- 4: each stream gets its own verdict ---------------------------------------------------------------------------------------------------------
def test_a_batch_with_unnamed_refused_and_short_streams(html):
    cd = SB.BlockCodec(0, O.HASH_CRC32C)
    cb = 1000
    blobs = [html[:5000], html[100:4100], html[7:3007], html[:2500], html[9:9 + 6001], html[:1]]
    streams, ix = batch_of(blobs, cb, O.HASH_CRC32C)
    reqs = [(0, 10, 20), (0, 990, 20), (0, 4999, 1), (2, 0, 3000), (3, 100, 10), (3, 105, 10), (4, 500, 3000), (5, 0, 0)]
    rng = np.random.default_rng(2)
    srcs = [U.fresh(rng, ln) for _, _, ln in reqs]
    free = U.write_plan(streams, ix, reqs, srcs)
    caps = [bd or len(s) for bd, s in zip(free["out_bound"], streams)]
    caps[4] = free["out_len"][4] - 1
    u = Updated(cd, streams, ix, reqs, srcs, caps=caps).check()
    assert u.got["status"] == [O.OK, O.OK, O.OK, O.ERR_BAD_ARG, O.ERR_OUTPUT_TOO_SMALL, O.OK] and u.got["out_len"][1] == 0
    assert u.got["req_status"] == [O.OK] * 4 + [O.ERR_BAD_ARG, O.ERR_BAD_ARG, O.ERR_OUTPUT_TOO_SMALL, O.OK]
    f = ix["first"]
    for b in (1, 3, 4):                                                 # their rows keep the old positions (their out ranges: checked by the call)
        assert u.got["new_pos"][f[b]:f[b + 1]] == ix["pos"][f[b]:f[b + 1]]
    assert u.got["streams"][5] == streams[5]


# ---- 5: admission; the sizing call admits the real call exactly ----------------------------------------------------------------------------------
def test_admission_by_each_bound_and_the_sizing_call(html):
    cd = SB.BlockCodec(0, O.HASH_CRC32C)
    cb = 512
    blobs = [html[:3000], html[50:2050], html[9:9 + 4000], html[:700]]
    streams, ix = batch_of(blobs, cb, O.HASH_CRC32C)
    reqs = [(0, 100, 1000), (1, 0, 512), (1, 600, 10), (2, 511, 2), (3, 0, 0)]
    srcs = [bytes([7]) * ln for _, _, ln in reqs]
    sizing = Updated(cd, streams, ix, reqs, srcs, caps=[0] * 4, max_slots=0, stage_cap=0).check()
    slots, _, stage, _ = sizing.got["result"]
    assert (slots, stage) == (7, 3584) and sizing.got["status"] == [O.ERR_OUTPUT_TOO_SMALL] * 4
    full = Updated(cd, streams, ix, reqs, srcs, caps=sizing.got["out_bound"], max_slots=slots, stage_cap=stage).check()
    assert full.got["status"] == [O.OK] * 4 and full.got["result"][3] == 4
    short = Updated(cd, streams, ix, reqs, srcs, max_slots=slots - 1).check()
    assert short.got["status"] == [O.OK, O.OK, O.ERR_OUTPUT_TOO_SMALL, O.ERR_OUTPUT_TOO_SMALL] and short.got["streams"][:2] == full.got["streams"][:2]
    short = Updated(cd, streams, ix, reqs, srcs, stage_cap=1536 + 1023).check()
    assert short.got["status"] == [O.OK] + [O.ERR_OUTPUT_TOO_SMALL] * 3 and short.got["result"][::2] == [slots, stage]
    loose = Updated(cd, streams, ix, reqs, srcs, max_slots=slots + 300, stage_cap=stage + 100000).check()
    assert loose.got["streams"] == full.got["streams"]


# ---- 6: corruption ---------------------------------------------------------------------------------------------------------------------------------
def test_a_corrupt_edge_fails_the_stream_and_a_corrupt_covered_chunk_is_repaired(html):
    cd = SB.BlockCodec(0, O.HASH_CRC32C)
    cb = 4096
    raw = html[:5 * cb]
    s = K.stream_of(raw, cb)
    good = K.stream_of(html[5:5 + 3 * cb], cb)
    rows = R.walk(s)[0]
    bad = R.corrupt_chunk(s, rows[2])
    streams = [good, bad]
    ix = X.build_index(streams)
    want = M.chunk_status(bad, rows[2])
    src = bytes(range(256)) * 40
    edge = Updated(cd, streams, ix, [(0, 5, 10), (1, 2 * cb + 5, cb)], [src[:10], src[:cb]]).check()
    assert edge.got["status"] == [O.OK, want] and edge.got["req_status"] == [O.OK, want] and want != O.OK
    both = Updated(cd, streams, ix, [(1, cb, 10), (1, 2 * cb - 5, 10)], [src[:10], src[:10]]).check()
    assert both.got["status"] == [O.OK, want] and both.got["req_status"] == [want, want]
    whole = Updated(cd, streams, ix, [(1, 2 * cb - 1, cb + 2)], [src[:cb + 2]]).check()
    assert whole.got["status"] == [O.OK, O.OK]
    assert O.frame_decode(whole.got["streams"][1]) == raw[:2 * cb - 1] + src[:cb + 2] + raw[3 * cb + 1:]


# ---- 7: request errors ---------------------------------------------------------------------------------------------------------------------------
def test_each_request_error_gets_its_status(html):
    cd = SB.BlockCodec(0, O.HASH_CRC32C)
    cb = 1000
    streams = [K.stream_of(html[:n], cb) for n in (5000, 4000, 3000)] + [R.big_chunk_stream()[0], R.uniform_stream(3, 1)[0][:-5]]
    ix = X.build_index(streams)
    big = next(r for r in R.walk(streams[3])[0] if r[5] > 65536)
    unindexed = {**ix, "tail": ix["tail"][:2] + [O.ERR_OUTPUT_TOO_SMALL] + ix["tail"][3:]}
    cases = [([(0, 10, 5), (0, 12, 5)], ix, [O.ERR_BAD_ARG] * 2), ([(0, 10, 5), (0, 15, 5)], ix, [O.OK] * 2), ([(0, 20, 5), (0, 10, 5)], ix, [O.ERR_BAD_ARG] * 2),
             ([(1, 0, 5), (0, 0, 5), (2, 0, 5)], ix, None),
             ([(0, 0, 5), (2, 0, 5), (1, 0, 5), (2, 9, 5)], ix, None),
             ([(5, 0, 1)], ix, [O.ERR_BAD_ARG]), ([(0xFFFFFFFF, 0, 0)], ix, [O.ERR_BAD_ARG]), ([(0, 4999, 2)], ix, [O.ERR_BAD_ARG]),
             ([(0, 5000, 1)], ix, [O.ERR_BAD_ARG]), ([(0, 5000, 0)], ix, [O.OK]), ([(0, 5001, 0)], ix, [O.ERR_BAD_ARG]),
             ([(0, U.U64, 2)], ix, [O.ERR_BAD_ARG]), ([(0, 1, U.U64)], ix, [O.ERR_BAD_ARG]),
             ([(3, big[4] + 1, 1)], ix, [O.ERR_BAD_ARG]), ([(3, big[4], big[5])], ix, [O.ERR_BAD_ARG]), ([(3, big[4] - 1, 1)], ix, [O.OK]),
             ([(4, 0, 1)], ix, [O.ERR_TRUNCATED_STREAM]), ([(2, 0, 1)], unindexed, [O.ERR_OUTPUT_TOO_SMALL]),
             ([(2, 0, 1)], {**ix, "tail": [0, 0, 77, 0, 0]}, [O.ERR_BAD_ARG])]
    for reqs, index, expect in cases:
        srcs = [bytes([9]) * min(ln, 1 << 17) for _, _, ln in reqs]
        u = Updated(cd, streams, index, reqs, srcs).check()             # (the guards and the canaries are checked by the call)
        assert expect is None or u.got["req_status"] == expect, reqs


# ---- 8: stale and unsound indexes ------------------------------------------------------------------------------------------------------------------
def test_stale_and_unsound_indexes_give_the_models_statuses(named):
    names, streams, ix = named
    cd = SB.BlockCodec(0, O.HASH_CRC32C)
    rng = np.random.default_rng(11)
    reqs = U.sound_lists(streams, ix)
    srcs = [U.fresh(rng, ln) for _, _, ln in reqs]
    clean = Updated(cd, streams, ix, reqs, srcs).check()
    assert O.OK in clean.got["req_status"] and clean.got["result"][3] >= 10        # (some named streams hold a corrupt chunk: their edges say so)
    refused = written = 0
    for bad in U.unsound_indexes(ix, streams, rng):
        u = Updated(cd, streams, bad, reqs, srcs).check()
        refused += sum(1 for s in u.got["req_status"] if s != O.OK)
        written += u.got["result"][3]
    assert refused > 100 and written > 5                               # both outcomes, on the unsound indexes
    # stale: the index of other streams of the same shape at the same place
    other = [K.stream_of(read_testdata("html")[3:3 + 9000], 1000), K.stream_of(read_testdata("html")[:9000], 1000)]
    stale = X.build_index([other[1], other[0]])
    u = Updated(cd, other, stale, [(0, 1500, 2000), (1, 10, 5)], [bytes(2000), bytes(5)]).check()
    assert O.ERR_BAD_ARG in u.got["req_status"]


# ---- 9: the seams of the emit's workgroups ---------------------------------------------------------------------------------------------------------
def test_emit_workgroup_seams(html):
    cd = SB.BlockCodec(0, O.HASH_CRC32C)
    rnd = np.random.default_rng(3).integers(0, 256, 300000, dtype=np.uint8).tobytes()
    # 4 096-byte raw chunks of 4 104 bytes: chunk 15 lies across byte 65 536 of the old stream, and the new one (compressible) is shorter
    s, = batch = [K.stream_of(rnd[:40 * 4096], 4096)]
    ix = X.build_index(batch)
    across = next(i for i, p in enumerate(ix["pos"]) if p < 65536 < p + 4104)
    reqs = [(0, across * 4096 + 7, 4096), (0, (across + 3) * 4096, 100)]
    u = Updated(cd, batch, ix, reqs, [b"ab" * 2048, b"z" * 100]).check()
    assert u.got["out_len"][0] < len(s)
    u = Updated(cd, batch, ix, reqs, [rnd[5:5 + 4096], rnd[:100]]).check()
    assert u.got["out_len"][0] == len(s)
    # 64-byte chunks across the boundary: every chunk of a run around byte 65 536 of the old stream is dirty
    blobs = [html[:63], (html + rnd[:30000])[7:7 + 140001], rnd[:129]]
    streams, ix = batch_of(blobs, 64, O.HASH_CRC32C)
    f = ix["first"][1]
    row = next(i for i in range(f, ix["first"][2]) if ix["pos"][i] > 65536) - f
    reqs = [(1, (row - 40) * 64 + 3, 80 * 64), (1, (row + 900) * 64, 64 * 200 + 1)]
    Updated(cd, streams, ix, reqs, [U.fresh(np.random.default_rng(1), ln) for _, _, ln in reqs]).check()
    # two dirty chunks (and three requests) in one workgroup's range, clean chunks between them
    reqs = [(0, 1, 2), (1, 64 * 3 + 1, 2), (1, 64 * 9, 64), (1, 64 * 11 + 5, 1), (2, 128, 1)]
    Updated(cd, streams, ix, reqs, [b"q" * ln for _, _, ln in reqs]).check()


# ---- 10: past 4 GiB --------------------------------------------------------------------------------------------------------------------------------
def test_one_stream_past_4_gib():
    n, cb = (1 << 32) + 70001, 65536
    free = torch.cuda.mem_get_info()[0]
    if free < 40 << 30:
        pytest.skip(f"needs 40 GiB of free device memory, {free >> 30} GiB free")
    cd = SB.BlockCodec(0, O.HASH_CRC32C)
    src = torch.randint(0, 256, (n,), dtype=torch.uint8, device="cuda", generator=torch.Generator("cuda").manual_seed(5))
    in_off, in_len = H.dev([0]), H.dev([n])
    mc = K.nchunks(n, cb)
    framed, f_off, f_len, status, _, index = cd.frame_encode_seekable(src, in_off, in_len, cb, max_chunks=mc)
    size = int(f_len.item())
    assert status.tolist() == [O.OK] and size == 10 + n + 8 * mc         # raw chunks: the stream outgrows its input
    # one window past position 2^32, off the chunk boundaries: compressible bytes, so three chunks shrink and everything behind them moves
    off, ln = (1 << 32) - 3 * cb + 11, 2 * cb
    first = off // cb
    data = torch.from_numpy(np.frombuffer((b"snappier " * 20000)[:ln], dtype=np.uint8).copy()).cuda()
    old = src[first * cb:(first + 3) * cb].cpu().numpy().tobytes()
    new = bytearray(old)
    new[off - first * cb:off - first * cb + ln] = data.cpu().numpy().tobytes()
    chunks = K.chunks_of(bytes(new), cb)
    shift = sum(len(c) for c in chunks) - 3 * (cb + 8)
    out = torch.empty(size, dtype=torch.uint8, device="cuda")
    ol, st, rst, new_ix, res, _ = cd.frame_write_indexed(framed, f_off, f_len, index, torch.zeros(1, dtype=torch.int32, device="cuda"), H.dev([off]),
                                                         data, H.dev([0]), H.dev([ln]), out, H.dev([0]), H.dev([size]))
    assert st.tolist() == [O.OK] and rst.tolist() == [O.OK] and ol.tolist() == [size + shift] and res.tolist() == [3, size + shift, 3 * cb, 1]
    p0 = 10 + first * (cb + 8)
    assert int(index.pos[first].item()) == p0 > (1 << 32) - 4 * (cb + 8)
    assert torch.equal(new_ix.pos[:first + 1], index.pos[:first + 1]) and torch.equal(new_ix.pos[first + 3:], index.pos[first + 3:] + shift)
    assert int(new_ix.pos[-1].item()) > 1 << 32
    assert out[p0:p0 + len(chunks[0])].cpu().numpy().tobytes() == chunks[0]
    assert torch.equal(out[:p0], framed[:p0]) and torch.equal(out[p0 + 3 * (cb + 8) + shift:size + shift], framed[p0 + 3 * (cb + 8):size])
    # the window, and the stream's last bytes (past 2^32 in both streams), read back through the new index
    back = torch.empty(ln + 70001, dtype=torch.uint8, device="cuda")
    rl, rs, _ = cd.frame_read_indexed(out, H.dev([0]), ol, new_ix, torch.zeros(2, dtype=torch.int32, device="cuda"), H.dev([off, n - 70001]),
                                      H.dev([ln, 70001]), back, H.dev([0, ln]), H.dev([ln, 70001]))
    assert rs.tolist() == [O.OK, O.OK] and rl.tolist() == [ln, 70001]
    assert torch.equal(back[:ln], data) and torch.equal(back[ln:], src[n - 70001:])


# ---- 11: graph capture -----------------------------------------------------------------------------------------------------------------------------
def test_graph_capture_replays_on_new_request_contents(html):
    cd = SB.BlockCodec(0, O.HASH_CRC32C)
    cb = 4096
    blobs = [html[:50000], html[11:11 + 30000], html[5:5 + 9000]]
    streams, ix = batch_of(blobs, cb, O.HASH_CRC32C)
    reqs = [(0, 4000, 9000), (0, 20000, 10), (2, 8999, 1)]
    lens = [q[2] for q in reqs]
    framed, in_off, in_len = H.pack(streams)
    index = SB.FrameIndex(*index_tensors(ix, 3)[0])
    src = torch.zeros(sum(lens), dtype=torch.uint8, device="cuda")
    src_off = H.dev(np.cumsum([0] + lens[:-1]))
    rs, ro, rl = torch.tensor([q[0] for q in reqs], dtype=torch.int32, device="cuda"), H.dev([q[1] for q in reqs]), H.dev(lens)
    caps = [len(s) + 64 for s in streams]
    out_off, total = H.out_layout(np.array(caps, dtype=np.int64))
    out = torch.zeros(total, dtype=torch.uint8, device="cuda")
    d_in_off, d_in_len, d_out_off, d_caps = H.dev(in_off), H.dev(in_len), H.dev(out_off), H.dev(caps)
    free = U.write_plan(streams, ix, reqs, [bytes(n) for n in lens])
    ms, sc = free["result"][0], free["result"][2]
    work = torch.empty(N.frame_update_lib().snp_frame_write_indexed_workspace(3, 3, ms, sc), dtype=torch.uint8, device="cuda")

    def fill(seed):
        srcs = [U.fresh(np.random.default_rng(seed + i), n) for i, n in enumerate(lens)]
        src.copy_(torch.from_numpy(np.frombuffer(b"".join(srcs), dtype=np.uint8).copy()).cuda())
        return srcs

    def call():
        return cd.frame_write_indexed(framed, d_in_off, d_in_len, index, rs, ro, src, src_off, rl, out, d_out_off, d_caps, max_slots=ms, stage_cap=sc,
                                      work=work)

    fill(0)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        call()
        torch.cuda.synchronize()
        call()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        ol, st, rst, new_ix, res, _ = call()
    srcs = fill(777)
    out.zero_()
    g.replay()
    torch.cuda.synchronize()
    want = U.write_plan(streams, ix, reqs, srcs, caps, ms, sc)
    assert st.tolist() == want["status"] and ol.tolist() == want["out_len"] and rst.tolist() == want["req_status"] and res.tolist() == want["result"]
    assert new_ix.pos.tolist() == want["new_pos"]
    h = out.cpu().numpy()
    for b, x in enumerate(want["streams"]):
        if x is not None:
            assert h[out_off[b]:out_off[b] + len(x)].tobytes() == x, b


# ---- 12: empty calls, and the wrapper ----------------------------------------------------------------------------------------------------------------
def test_empty_calls_write_a_zeroed_result():
    cd = SB.BlockCodec(0, O.HASH_CRC32C)
    cd._bind()
    call = N.frame_update_lib().snp_frame_write_indexed_batch
    for ns, nreq in ((0, 0), (3, 0), (0, 2)):
        result = Guarded(4, torch.int64)
        assert call(cd.ctx.handle, None, None, None, ns, *[None] * 5, 0, *[None] * 5, nreq, 0, 0, *[None] * 6, None, None, None, result.ptr()) == O.OK
        torch.cuda.synchronize()
        assert result.read() == [0, 0, 0, 0]


def test_update_to_memory(html):
    cd = SB.BlockCodec(0, O.HASH_CRC32C)
    cb = 4096
    blobs = [html[:20000], html[3:3 + 4097], b"", html[:9000]]
    data, in_off, lens = H.pack(blobs)
    framed, f_off, f_len, _, _, index = cd.frame_encode_seekable(data, H.dev(in_off), H.dev(lens), cb)
    reqs = [(0, 4000, 8300), (0, 19999, 1), (1, 4096, 1), (3, 100, 9000)]     # the last one runs past its stream's end
    rng = np.random.default_rng(4)
    srcs = [U.fresh(rng, ln) for _, _, ln in reqs]
    src, src_off, _ = H.pack(srcs)
    out, out_off, out_len, status, req_status, new_ix = cd.frame_update_to_memory(
        framed, f_off, f_len, index, torch.tensor([q[0] for q in reqs], dtype=torch.int32, device="cuda"), H.dev([q[1] for q in reqs]), src,
        H.dev(src_off), H.dev([q[2] for q in reqs]))
    assert status.tolist() == [O.OK, O.OK, O.OK, O.ERR_BAD_ARG] and req_status.tolist() == [O.OK, O.OK, O.OK, O.ERR_BAD_ARG]
    h = out.cpu().numpy()
    for b in (0, 1):
        new = h[int(out_off[b]):int(out_off[b]) + int(out_len[b])].tobytes()
        assert new == K.stream_of(U.patched(blobs[b], reqs, srcs, b), cb)
    assert out_len.tolist()[2:] == [0, 0]
    # the streams that were written, read through the returned index
    got, g_off, g_len, g_st = cd.frame_gather_to_memory(out, out_off[:2], out_len[:2], SB.FrameIndex(new_ix.first[:3], new_ix.start, new_ix.pos,
                                                                                                      new_ix.total[:2], new_ix.tail[:2]),
                                                        torch.tensor([0, 1], dtype=torch.int32, device="cuda"), H.dev([4000, 4096]), H.dev([8300, 1]))
    assert g_st.tolist() == [O.OK, O.OK]
    g = got.cpu().numpy()
    assert g[:8300].tobytes() == srcs[0] and g[int(g_off[1]):int(g_off[1]) + 1].tobytes() == srcs[2]


# ---- rebuilt chunks stored compressed and stored raw, at the chunk sizes whose emit teams are 64, 128 and 256 threads --------------------------------
@pytest.mark.parametrize("cb", SC.TEAM_CHUNK_SIZES)
def test_rebuilt_chunks_raw_and_compressed_at_every_team_size(cb):
    cd = SB.BlockCodec(0, O.HASH_CRC32C)
    blobs = SC.team_blobs(cb)
    streams, ix = batch_of(blobs, cb, O.HASH_CRC32C)
    reqs = [(b, cb - 3, cb + 10) for b in range(3)]                    # a tail edge, a whole chunk and a head edge in every stream
    srcs = [x[5:5 + cb + 10] for x in blobs]                            # each stream's own kind of bytes
    u = Updated(cd, streams, ix, reqs, srcs).check()
    assert u.got["status"] == [O.OK] * 3 and u.got["result"][0] == 9
    assert u.got["streams"] == [K.stream_of(U.patched(x, reqs, srcs, b), cb) for b, x in enumerate(blobs)]
    assert [SC.chunk_types(s) for s in u.got["streams"][:2]] == [{1}, {0}]

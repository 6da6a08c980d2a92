"""libsnappier_hip_frame_dedup.so on the GPU: snp_frame_dedup_indexed_batch against the model (frame_dedup_model.py) element for element --
canon, status, the pack's bytes and index, the recipes, d_result -- where the call can go wrong: the tails of the chunk compare at every
alignment, forged CRC collisions, one key under contention, a table that probes, the shapes of run merging, foreign and corrupt input with
indexes filled with anything, admission at every bound, and end to end through the wrappers (content-defined versions of html, a restore, a
read through the pack's index, the incremental form); two runs; graph capture.  The call is made directly, every array and the workspace
between guard words, the pack arena canary-filled.  Needs an MI355X."""
import numpy as np
import pytest
import torch

import frame_buffers_helpers as H
import frame_buffers_model as M
import frame_dedup_model as D
import frame_index_model as X
import oracle as O
from conftest import read_testdata
from seekable_harness import CANARY, UNTOUCHED, Guarded, _p, dev_u64, index_tensors, s64

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from snappier_amd import batch as SB, _native as N

VARIANTS = [O.HASH_CRC32C, O.HASH_MUL]
KEYS = ("first", "start", "pos", "total", "tail")
ARENA_LEAD = 3


@pytest.fixture(scope="module")
def html():
    return read_testdata("html")


def cd_of(variant=O.HASH_CRC32C):
    return SB.BlockCodec(0, variant)


# ---- the call, made directly ---------------------------------------------------------------------------------------------------------------------
def dedup_call(cd, streams, ix, nbase=0, max_entries=None, max_segs=None, out_cap=None, lead=1, gap=3):
    """snp_frame_dedup_indexed_batch with every array guarded and the pack arena canary-filled: -> the dict the model's dedup_plan gives.
    None: what the model says the batch needs."""
    ns = len(streams)
    DL = N.frame_dedup_lib()
    cd._bind()
    if None in (max_entries, max_segs, out_cap):
        me, ms, cap = D.needs(streams, ix, nbase)
        max_entries = me if max_entries is None else max_entries
        max_segs = ms if max_segs is None else max_segs
        out_cap = cap if out_cap is None else out_cap
    framed, in_off, in_len = H.pack(streams, lead, gap) if ns else (torch.zeros(16, dtype=torch.uint8, device="cuda"), [], [])
    ixt, ne = index_tensors(ix, ns) if ns else ([torch.zeros(1, dtype=torch.int64, device="cuda")] * 4 + [torch.zeros(1, dtype=torch.int32, device="cuda")], 0)
    nnew = ns - nbase
    arena = torch.full((out_cap + 2 * ARENA_LEAD + 5,), CANARY, dtype=torch.uint8, device="cuda")
    out_len, status, canon, result = Guarded(1, torch.int64), Guarded(ns, torch.int32), Guarded(ne, torch.int64), Guarded(8, torch.int64)
    pk = [Guarded(2, torch.int64), Guarded(max_entries, torch.int64), Guarded(max_entries, torch.int64), Guarded(1, torch.int64), Guarded(1, torch.int32)]
    seg = [Guarded(nnew + 1, torch.int64), Guarded(max_segs, torch.int32), Guarded(max_segs, torch.int64), Guarded(max_segs, torch.int64)]
    work = Guarded(DL.snp_frame_dedup_indexed_workspace(ns, ne), torch.uint8)
    tabs = [dev_u64(in_off), dev_u64(in_len)]
    import ctypes as C
    st = DL.snp_frame_dedup_indexed_batch(cd.ctx.handle, _p(framed), _p(tabs[0]), _p(tabs[1]), ns, *[_p(t) for t in ixt], ne, nbase, max_entries,
                                          max_segs, out_cap, C.c_void_p(arena.data_ptr() + ARENA_LEAD), out_len.ptr(), status.ptr(), canon.ptr(),
                                          *[g.ptr() for g in pk], *[g.ptr() for g in seg], work.ptr(), result.ptr())
    assert st == O.OK
    torch.cuda.synchronize()
    work.read()
    h = arena.cpu().numpy()
    got = dict(status=status.read(), canon=[v & D.U64 for v in canon.read()], out_len=out_len.read()[0], result=result.read())
    if ns == 0:                                                         # a zeroed d_result and nothing else
        assert (h == CANARY).all() and got["out_len"] == UNTOUCHED and all(v == UNTOUCHED for g in pk[:1] + seg[:1] for v in g.read())
        return got
    n = got["out_len"]
    assert 0 <= n <= out_cap and (h[:ARENA_LEAD] == CANARY).all() and (h[ARENA_LEAD + n:] == CANARY).all(), "a write outside the pack"
    got["pack"] = h[ARENA_LEAD:ARENA_LEAD + n].tobytes() if n or out_cap >= 10 else None
    index = [g.read() for g in pk]
    used = index[0][1]
    assert index[0][0] == 0 and 0 <= used <= max_entries and all(v == UNTOUCHED for v in index[1][used:] + index[2][used:]), "a row beyond the pack's index"
    index[1], index[2] = index[1][:used], index[2][:used]
    got["index"] = dict(zip(KEYS, index))
    segs = [g.read() for g in seg]
    nsegs = segs[0][nnew]
    assert 0 <= nsegs <= max_segs and all(v == UNTOUCHED for v in segs[2][nsegs:] + segs[3][nsegs:]), "a segment beyond seg_first[nnew]"
    got["segs"] = dict(first=segs[0], stream=segs[1][:nsegs], off=[v & D.U64 for v in segs[2][:nsegs]], len=[v & D.U64 for v in segs[3][:nsegs]])
    return got


def check(cd, streams, ix, nbase=0, **kw):
    got = dedup_call(cd, streams, ix, nbase, **kw)
    want = D.dedup_plan(streams, ix, nbase, kw.get("max_entries"), kw.get("max_segs"), kw.get("out_cap"))
    for key in ("status", "canon", "result", "out_len", "pack", "index", "segs"):
        assert got[key] == want[key], key
    return want


# ---- 1: the tails of the compare -----------------------------------------------------------------------------------------------------------------
def test_compare_tails_at_every_alignment():
    cd = cd_of()
    rng = np.random.default_rng(31)
    lens = [1, 15, 16, 17, 63, 64, 65, 255, 4096, 65536]
    base, new, merged, coll = [], [], 0, 0
    for k, n in enumerate(lens):
        raw = bytes(rng.integers(0, 200, n, dtype=np.uint8)) if n < 4096 else bytes(rng.integers(0, 4, n, dtype=np.uint8))
        plain, comp = D.raw_chunk(raw), M.data_chunk(raw)
        first, last = bytearray(plain), bytearray(plain)
        first[8] ^= 0x10
        last[-1] ^= 0x01
        base.append(plain)
        pad = [M.chunk(0x80, bytes(k % 2))]                             # shifts what follows by one byte: odd and even positions
        new += [plain] + pad + [bytes(last), plain, bytes(first)] + pad + [comp, plain]
        merged += 3
        coll += 3                                                       # another last byte, another first byte, another encoding
    streams = [D.stream_of_chunks(base), D.stream_of_chunks(new)]
    for nbase, lead in ((0, 1), (1, 2)):
        want = check(cd, streams, X.build_index(streams), nbase, lead=lead)
        assert want["result"][5] == merged and want["result"][6] == coll
    # the leader in the same stream as its copies, the copies first in another order
    both = [D.stream_of_chunks(new[::-1] + base)]
    check(cd, both, X.build_index(both))


# ---- 2: forged CRC collisions ----------------------------------------------------------------------------------------------------------------------
def test_forged_collisions_follow_the_leader_rule(html):
    cd = cd_of()
    a = html[:4097]
    b = D.forge_collision(a, at=4000, flip=0x08)
    assert a != b and O.crc32c(a) == O.crc32c(b)
    A, B = D.raw_chunk(a), D.raw_chunk(b)
    for order, canon, coll in (([A, B, B], [0, 1, 2], 2), ([B, A, B], [0, 1, 0], 1)):
        for streams in ([D.stream_of_chunks(order)], [D.stream_of_chunks([c]) for c in order]):
            want = check(cd, streams, X.build_index(streams))
            assert want["canon"] == canon and want["result"][6] == coll


# ---- 3: one key under contention ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nstreams", [1, 50])
def test_contention_on_one_key(html, nstreams):
    cd = cd_of()
    c = M.data_chunk(html[:1000])
    per = 5000 // nstreams
    streams = [D.stream_of_chunks([c] * per)] * nstreams
    want = check(cd, streams, X.build_index(streams))
    assert want["canon"] == [0] * 5000 and want["pack"] == M.STREAM_ID + c and want["result"][:3] == [1, 10 + len(c), 5000]
    assert want["segs"]["first"] == [per * j for j in range(nstreams + 1)] and want["segs"]["off"] == [0] * 5000   # none can merge


# ---- 4: a table that probes ----------------------------------------------------------------------------------------------------------------------------
def test_probing_finds_every_row_of_a_large_table():
    cd = cd_of()
    rng = np.random.default_rng(32)
    raws = rng.integers(0, 256, (20000, 64), dtype=np.uint8)
    chunks = [D.raw_chunk(r.tobytes()) for r in raws]
    assert len(set(chunks)) == 20000
    streams = [D.stream_of_chunks(chunks), D.stream_of_chunks(chunks[::-1])]
    want = check(cd, streams, X.build_index(streams))
    assert want["canon"][20000:] == list(range(19999, -1, -1)) and want["result"][5] == 20000 and want["result"][6] == 0
    assert want["segs"]["first"] == [0, 1, 20001] and want["pack"] == streams[0]


# ---- 5: run merging ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", VARIANTS)
def test_run_merging_shapes(variant):
    cd = cd_of(variant)
    per = {}
    for name, (streams, nbase) in D.run_cases(np.random.default_rng(21), variant).items():
        want = check(cd, streams, X.build_index(streams), nbase)
        f = want["segs"]["first"]
        per[name] = [b - a for a, b in zip(f, f[1:])]
    assert per == {"all_unique_is_one_segment": [1], "abab": [2], "run_continues_from_the_previous_stream": [1, 2],
                   "run_passes_from_base_into_pack": [2], "duplicate_of_the_middle_of_a_base_stream": [4], "base_only": []}


# ---- 6: foreign and corrupt input -------------------------------------------------------------------------------------------------------------------
def test_foreign_streams(html):
    cd = cd_of()
    streams = D.foreign_streams(html)
    want = check(cd, streams, X.build_index(streams))
    assert want["status"] == [O.OK] * 3 and want["result"][0] == 3 and want["canon"].count(D.NONE) == 5
    check(cd, streams, X.build_index(streams), 1)


def test_a_corrupt_stream_fails_alone_and_the_next_one_leads(html):
    cd = cd_of()
    a, b = M.data_chunk(html[:900]), M.data_chunk(html[900:2000])
    streams = [D.stream_of_chunks([a, b]), D.stream_of_chunks([b, a]), D.stream_of_chunks([a, b])]
    ix = X.build_index(streams)
    broken = bytearray(streams[0])
    broken[10] = 0x02                                                   # the first chunk's type: no data chunk
    want = check(cd, [bytes(broken)] + streams[1:], ix)
    assert want["status"] == [O.ERR_BAD_ARG, O.OK, O.OK] and want["canon"] == [D.NONE, D.NONE, 2, 3, 3, 2]
    short = [streams[0][:-1]] + streams[1:]                             # the last chunk ends outside the stream
    assert check(cd, short, ix)["status"] == [O.ERR_BAD_ARG, O.OK, O.OK]
    other = [streams[1], streams[0], streams[2]]                        # an index from other bytes
    check(cd, other, ix)
    check(cd, [html[:500], html[500:900], streams[2]], ix)


def test_unsound_indexes_write_nothing_outside_the_guards(html):
    cd = cd_of()
    a, b = M.data_chunk(html[:900]), M.data_chunk(html[900:2000])
    streams = [D.stream_of_chunks([a, b]), D.stream_of_chunks([b, a]), D.stream_of_chunks([a, b])] + D.foreign_streams(html)[1:2]
    ix = X.build_index(streams)
    rng = np.random.default_rng(2)
    cases = D.unsound_indexes(ix, streams, rng)
    assert {"a_tail_that_is_not_ok", "first_runs_backwards", "a_position_outside_in_len", "random_words"} <= set(cases)
    failed = 0
    for name, bad in cases.items():
        for nbase in (0, 2):
            want = check(cd, streams, bad, nbase)
            failed += sum(1 for s in want["status"] if s != O.OK)
    assert failed > 10
    for _ in range(3):                                                  # an index filled with random words, others
        bad = D.unsound_indexes(ix, streams, rng)["random_words"]
        check(cd, streams, bad, max_entries=7, max_segs=9, out_cap=5000)


# ---- 7: admission ------------------------------------------------------------------------------------------------------------------------------------
def test_admission_at_every_bound_and_the_sizing_round():
    cd = cd_of()
    rng = np.random.default_rng(4)
    chunks = [M.data_chunk(bytes(rng.integers(0, 256, int(n), dtype=np.uint8))) for n in rng.integers(50, 400, 9)]
    streams = [D.stream_of_chunks([chunks[0], chunks[1], chunks[2]]), D.stream_of_chunks([chunks[1], chunks[3], chunks[0], chunks[4]]),
               D.stream_of_chunks([chunks[5], chunks[3], chunks[6], chunks[7]])]
    ix = X.build_index(streams)
    sizing = dedup_call(cd, streams, ix, 0, 0, 0, 0)
    me, cap, ms = sizing["result"][:3]
    assert sizing["status"] == [O.ERR_OUTPUT_TOO_SMALL] * 3 and sizing["out_len"] == 0
    free = check(cd, streams, ix, 0, max_entries=me, max_segs=ms, out_cap=cap)      # the exact fit
    assert free["status"] == [O.OK] * 3 and sizing["canon"] == free["canon"] and len(free["pack"]) == cap
    check(cd, streams, ix, 0, max_entries=0, max_segs=0, out_cap=0)
    per = [D.dedup_plan(streams[:k + 1], X.build_index(streams[:k + 1]))["result"][:3] for k in range(3)]
    for bound in range(3):
        for miss in range(3):
            b = [me, cap, ms]
            b[bound] = per[miss][bound] - 1                             # stream `miss` is the first that does not fit
            want = check(cd, streams, ix, 0, max_entries=b[0], max_segs=b[2], out_cap=b[1])
            assert want["status"] == [O.OK] * miss + [O.ERR_OUTPUT_TOO_SMALL] * (3 - miss), (bound, miss)
    for cap in (9, 10, 11):
        check(cd, streams, ix, 0, max_entries=me, max_segs=ms, out_cap=cap)
    for nbase in (1, 2, 3):
        want = check(cd, streams, ix, nbase)
        assert want["canon"] == free["canon"]
    assert check(cd, streams, ix, 3)["pack"] == M.STREAM_ID
    none = dedup_call(cd, [], dict(first=[0], start=[], pos=[], total=[], tail=[]))
    assert none["result"] == [0] * 8


# ---- 8: end to end ------------------------------------------------------------------------------------------------------------------------------------
def index_of(index, b):
    """Stream b of a batch index as an index of its own."""
    f0, f1 = int(index.first[b]), int(index.first[b + 1])
    first = torch.tensor([0, f1 - f0], dtype=torch.int64, device="cuda")
    return SB.FrameIndex(first, index.start[f0:f1].contiguous(), index.pos[f0:f1].contiguous(), index.total[b:b + 1].contiguous(),
                         index.tail[b:b + 1].contiguous(), None)


@pytest.mark.parametrize("variant", VARIANTS)
def test_versions_of_html_end_to_end(html, variant):
    cd = cd_of(variant)
    at = len(html) // 3
    raws = [html, html[:at] + bytes(np.random.default_rng(11).integers(0, 256, 1001, dtype=np.uint8)) + html[at:]]
    data, in_off, lens = H.pack(raws)
    out, out_off, out_len, est, _, index = cd.frame_encode_content_defined(data, H.dev(in_off), H.dev(lens), 64, 1024)
    torch.cuda.synchronize()
    assert est.tolist() == [O.OK, O.OK]
    h, off, n = out.cpu().numpy(), out_off.tolist(), out_len.tolist()
    streams = [h[o:o + k].tobytes() for o, k in zip(off, n)]
    assert streams == D.content_defined(raws, 64, 1024, variant)
    pack, pindex, recipe, canon, status, result = cd.frame_dedup_to_memory(out, out_off, out_len, index)
    torch.cuda.synchronize()
    want = D.dedup_plan(streams, X.build_index(streams))
    res = result.tolist()
    assert status.tolist() == [O.OK, O.OK] and res == want["result"] and res[6] == 0
    assert pack.numel() == res[1] < 0.6 * sum(n)
    rows = len(want["canon"])                                           # (the encoder's index arrays hold more rows than the streams have)
    assert pack.cpu().numpy().tobytes() == want["pack"] and [v & D.U64 for v in canon[:rows].tolist()] == want["canon"]
    assert all(v == -1 for v in canon[rows:].tolist())
    assert [t.tolist() for t in recipe] == [want["segs"][k] for k in ("first", "stream", "off", "len")]
    for key in KEYS:
        assert getattr(pindex, key).tolist() == want["index"][key], key
    # both streams again, byte for byte
    back, b_off, b_len, bst, _ = cd.frame_restore_to_memory(out, out_off, out_len, index, 0, pack, pindex, recipe, chunk_bytes=4096)
    torch.cuda.synchronize()
    assert bst.tolist() == [O.OK, O.OK]
    hb = back.cpu().numpy()
    assert [hb[o:o + k].tobytes() for o, k in zip(b_off.tolist(), b_len.tolist())] == streams
    # the pack is a seekable stream: its chunks through its own index
    p_off, p_len = H.dev([0]), H.dev([pack.numel()])
    rows = pindex.start.tolist()
    reqs = [0, len(rows) // 2, len(rows) - 1]
    ends = rows[1:] + [int(pindex.total[0])]
    req = [H.dev([0] * len(reqs)).to(torch.int32), H.dev([rows[r] for r in reqs]), H.dev([ends[r] - rows[r] for r in reqs])]
    caps = H.dev([ends[r] - rows[r] for r in reqs])
    r_off = torch.cumsum(caps, 0) - caps
    dec = torch.zeros(int(caps.sum()), dtype=torch.uint8, device="cuda")
    got = cd.frame_read_indexed(pack, p_off, p_len, pindex, req[0], req[1], req[2], dec, r_off, caps)
    torch.cuda.synchronize()
    whole = O.frame_decode(want["pack"])
    assert dec.cpu().numpy().tobytes() == b"".join(whole[rows[r]:ends[r]] for r in reqs) and got[1].tolist() == [O.OK] * 3
    # incremental: version 1 alone into pack 1, version 2 against pack 1 into pack 2, version 2 back from the two packs
    one = cd.frame_dedup_to_memory(out, out_off[:1], out_len[:1], index_of(index, 0))
    torch.cuda.synchronize()
    assert one[4].tolist() == [O.OK]
    both = torch.cat([one[0], out])
    boff = torch.cat([H.dev([0]), out_off[1:] + one[0].numel()])
    blen = torch.cat([H.dev([one[0].numel()]), out_len[1:]])
    i1, i2 = one[1], index_of(index, 1)
    r1 = int(i1.first[1])
    bindex = SB.FrameIndex(torch.cat([i1.first, i2.first[1:] + r1]), torch.cat([i1.start[:r1], i2.start]), torch.cat([i1.pos[:r1], i2.pos]),
                           torch.cat([i1.total, i2.total]), torch.cat([i1.tail, i2.tail]))
    two = cd.frame_dedup_to_memory(both, boff, blen, bindex, nbase=1)
    torch.cuda.synchronize()
    assert two[4].tolist() == [O.OK, O.OK] and one[0].numel() + two[0].numel() == pack.numel() + 10
    back, b_off, b_len, bst, _ = cd.frame_restore_to_memory(both, boff, blen, bindex, 1, two[0], two[1], two[2])
    torch.cuda.synchronize()
    assert bst.tolist() == [O.OK] and back.cpu().numpy()[int(b_off[0]):int(b_off[0]) + int(b_len[0])].tobytes() == streams[1]


# ---- 9: two runs; graph capture --------------------------------------------------------------------------------------------------------------------------
def batch_of(html, shift):
    rng = np.random.default_rng(40 + shift)
    chunks = [M.data_chunk(html[o + shift:o + shift + int(n)]) for o, n in zip(range(0, 60000, 1500), rng.integers(1, 1500, 40))]
    order = rng.integers(0, 40, (4, 60))
    return [D.stream_of_chunks([chunks[i] for i in row]) for row in order]


def wrapper_arrays(got):
    out_len, status, canon, pindex, recipe, result = got
    used, nsegs = int(pindex.first[1]), int(recipe[0][-1])
    return [out_len.tolist(), status.tolist(), canon.tolist(), pindex.first.tolist(), pindex.start[:used].tolist(), pindex.pos[:used].tolist(),
            pindex.total.tolist(), pindex.tail.tolist(), recipe[0].tolist()] + [t[:nsegs].tolist() for t in recipe[1:]] + [result.tolist()]


def test_two_runs_and_graph_capture_give_the_same_arrays(html):
    cd = cd_of()
    sets = [batch_of(html, 0), batch_of(html, 7)]
    size = max(sum(len(s) for s in b) for b in sets)
    lens = [[len(s) for s in b] for b in sets]
    ixs = [X.build_index(b) for b in sets]
    ne = max(D.nentries_of(ix) for ix in ixs)
    assert all(D.nentries_of(ix) == ne for ix in ixs)
    framed = torch.zeros(size + 64, dtype=torch.uint8, device="cuda")
    d_off, d_len = torch.zeros(4, dtype=torch.int64, device="cuda"), torch.zeros(4, dtype=torch.int64, device="cuda")
    index = SB.FrameIndex(torch.zeros(5, dtype=torch.int64, device="cuda"), torch.zeros(ne, dtype=torch.int64, device="cuda"),
                          torch.zeros(ne, dtype=torch.int64, device="cuda"), torch.zeros(4, dtype=torch.int64, device="cuda"),
                          torch.zeros(4, dtype=torch.int32, device="cuda"))
    needs = [D.needs(b, ix, 1) for b, ix in zip(sets, ixs)]
    me, ms, cap = (max(v[k] for v in needs) for k in range(3))
    pack = torch.zeros(cap, dtype=torch.uint8, device="cuda")
    work = torch.zeros(N.frame_dedup_lib().snp_frame_dedup_indexed_workspace(4, ne), dtype=torch.uint8, device="cuda")

    def fill(k):
        off = np.concatenate([[0], np.cumsum(lens[k])[:-1]]).astype(np.int64)
        framed[:sum(lens[k])].copy_(torch.from_numpy(np.frombuffer(b"".join(sets[k]), dtype=np.uint8).copy()).cuda())
        d_off.copy_(H.dev(off))
        d_len.copy_(H.dev(lens[k]))
        for key, t in zip(KEYS, index_tensors(ixs[k], 4)[0]):
            getattr(index, key).copy_(t)

    def call():
        return cd.frame_dedup_indexed(framed, d_off, d_len, index, 1, me, ms, pack, work)

    def expect(k, arrays, h):
        want = D.dedup_plan(sets[k], ixs[k], 1, me, ms, cap)
        assert arrays[0] == [want["out_len"]] and arrays[1] == want["status"] and [v & D.U64 for v in arrays[2]] == want["canon"]
        assert arrays[3:8] == [want["index"][key] for key in KEYS]
        assert arrays[8:12] == [want["segs"][key] for key in ("first", "stream", "off", "len")] and arrays[12] == want["result"]
        assert h[:want["out_len"]].tobytes() == want["pack"]

    fill(0)
    first = wrapper_arrays(call())
    h1 = pack.cpu().numpy().copy()
    pack.zero_()
    second = wrapper_arrays(call())
    torch.cuda.synchronize()
    assert first == second and (pack.cpu().numpy() == h1).all()         # two runs of the same call
    expect(0, first, h1)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        call()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        got = call()
    fill(1)
    pack.zero_()
    g.replay()
    torch.cuda.synchronize()
    replayed = wrapper_arrays(got)
    expect(1, replayed, pack.cpu().numpy())
    eager = wrapper_arrays(call())
    torch.cuda.synchronize()
    assert eager == replayed

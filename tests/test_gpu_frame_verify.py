"""libsnappier_hip_frame_verify.so on the GPU: snp_frame_verify_indexed_batch and snp_frame_repair_plan_batch against the model
(frame_verify_model.py) array for array -- row_status, status, nbad, first_bad, bad_bytes, flags, d_result; plan_status, the recipes, d_result
-- where the calls can go wrong: every shape of stream and row, round borders inside and between streams, the sizing call, a slot below the
largest row, every scratch size and decode layout, every single-bit flip of a short chunk, damage at round borders, indexes filled with
anything, run merging for every pattern of 1 to 8 rows, every rejection, admission; and end to end through the wrappers: repair from a copy
(byte for byte), from a replica at another chunking (same bytes, same digest), damage on both sides; two runs; graph capture.  The calls are
made directly, every array and the workspace between guard words.  Needs an MI355X."""
import ctypes as C

import numpy as np
import pytest
import torch

import frame_buffers_helpers as H
import frame_buffers_model as M
import frame_index_model as X
import frame_verify_model as V
import oracle as O
from conftest import read_testdata
from layouts import DECODE_LAYOUTS, set_decode_layout
from seekable_harness import Guarded, _p, dev_u64, index_tensors, s32

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from snappier_amd import batch as SB, _native as N

VARIANTS = [O.HASH_CRC32C, O.HASH_MUL]
KEYS = ("first", "start", "pos", "total", "tail")
VERIFY_KEYS = ("row_status", "status", "nbad", "first_bad", "bad_bytes", "flags", "result")


@pytest.fixture(scope="module")
def html():
    return read_testdata("html")


def cd_of(variant=O.HASH_CRC32C):
    return SB.BlockCodec(0, variant)


def u64s(vals):
    return [v & V.U64 for v in vals]


# ---- the calls, made directly ----------------------------------------------------------------------------------------------------------------------
def verify_call(cd, streams, ix, slot_bytes=65536, scratch_cap=1 << 22, lead=1, gap=3):
    """snp_frame_verify_indexed_batch with every array and the workspace guarded: -> the dict the model's verify_plan gives."""
    ns = len(streams)
    VL = N.frame_verify_lib()
    cd._bind()
    framed, in_off, in_len = H.pack(streams, lead, gap) if ns else (torch.zeros(16, dtype=torch.uint8, device="cuda"), [], [])
    ixt, ne = index_tensors(ix, ns) if ns else ([torch.zeros(1, dtype=torch.int64, device="cuda")] * 4 + [torch.zeros(1, dtype=torch.int32, device="cuda")], 0)
    row_status, status, flags = Guarded(ne, torch.int32), Guarded(ns, torch.int32), Guarded(ns, torch.int32)
    nbad, first_bad, bad_bytes, result = Guarded(ns, torch.int64), Guarded(ns, torch.int64), Guarded(ns, torch.int64), Guarded(8, torch.int64)
    work = Guarded(VL.snp_frame_verify_indexed_workspace(ns, ne, slot_bytes, scratch_cap), torch.uint8)
    tabs = [dev_u64(in_off), dev_u64(in_len)]
    st = VL.snp_frame_verify_indexed_batch(cd.ctx.handle, _p(framed), _p(tabs[0]), _p(tabs[1]), ns, *[_p(t) for t in ixt], ne, slot_bytes, scratch_cap,
                                           row_status.ptr(), status.ptr(), nbad.ptr(), first_bad.ptr(), bad_bytes.ptr(), flags.ptr(), work.ptr(),
                                           result.ptr())
    assert st == O.OK
    torch.cuda.synchronize()
    work.read()
    return dict(row_status=row_status.read(), status=status.read(), nbad=nbad.read(), first_bad=u64s(first_bad.read()),
                bad_bytes=u64s(bad_bytes.read()), flags=flags.read(), result=u64s(result.read()))


def check(cd, streams, ix, slot_bytes=65536, scratch_cap=1 << 22, **kw):
    got = verify_call(cd, streams, ix, slot_bytes, scratch_cap, **kw)
    want = V.verify_plan(streams, ix, slot_bytes, scratch_cap)
    for key in VERIFY_KEYS:
        assert got[key] == want[key], key
    return want


def plan_call(cd, ix, ns, row_status, rep_total, rep_tail, rp_stream, rp_replica, max_segs=None):
    """snp_frame_repair_plan_batch with every array guarded: -> the dict the model's repair_plan gives.  None: what the model says the pairs need."""
    VL = N.frame_verify_lib()
    cd._bind()
    if max_segs is None:
        max_segs = V.repair_plan(ix, ns, row_status, rep_total, rep_tail, rp_stream, rp_replica)["result"][0]
    ne, nrep, nout = min(len(ix["start"]), len(row_status)), len(rep_total), len(rp_stream)
    one = [0]
    arrays = [dev_u64(ix["first"][:ns + 1] or one), dev_u64(ix["start"][:ne] or one), dev_u64(ix["total"][:ns] or one),
              torch.tensor([s32(v) for v in ix["tail"][:ns]] or one, dtype=torch.int32, device="cuda"),
              torch.tensor([s32(v) for v in row_status[:ne]] or one, dtype=torch.int32, device="cuda"), dev_u64(rep_total or one),
              torch.tensor([s32(v) for v in rep_tail] or one, dtype=torch.int32, device="cuda"),
              torch.tensor(list(rp_stream) or one, dtype=torch.int64, device="cuda").to(torch.int32),
              torch.tensor(list(rp_replica) or one, dtype=torch.int64, device="cuda").to(torch.int32)]
    seg = [Guarded(nout + 1, torch.int64), Guarded(max_segs, torch.int32), Guarded(max_segs, torch.int64), Guarded(max_segs, torch.int64)]
    plan_status, result = Guarded(nout, torch.int32), Guarded(4, torch.int64)
    work = Guarded(VL.snp_frame_repair_plan_workspace(nout), torch.uint8)
    a = [_p(t) for t in arrays]
    st = VL.snp_frame_repair_plan_batch(cd.ctx.handle, *a[:4], ne, ns, *a[4:7], nrep, *a[7:9], nout, max_segs, *[g.ptr() for g in seg],
                                        plan_status.ptr(), work.ptr(), result.ptr())
    assert st == O.OK
    torch.cuda.synchronize()
    work.read()
    got = dict(plan_status=plan_status.read(), result=u64s(result.read()))
    segs = [g.read() for g in seg]
    if nout == 0:
        return got
    nsegs = segs[0][nout]
    assert 0 <= nsegs <= max_segs and all(v & 0xFF == H.CANARY for v in segs[2][nsegs:] + segs[3][nsegs:]), "a segment beyond seg_first[nout]"
    got["segs"] = dict(first=segs[0], stream=segs[1][:nsegs], off=u64s(segs[2][:nsegs]), len=u64s(segs[3][:nsegs]))
    return got


def check_plan(cd, ix, ns, row_status, rep_total, rep_tail, rp_stream, rp_replica, max_segs=None):
    got = plan_call(cd, ix, ns, row_status, rep_total, rep_tail, rp_stream, rp_replica, max_segs)
    want = V.repair_plan(ix, ns, row_status, rep_total, rep_tail, rp_stream, rp_replica, max_segs)
    for key in ("plan_status", "result", "segs"):
        assert got[key] == want[key], key
    return want


# ---- 1: shapes -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", VARIANTS)
def test_every_shape_of_stream_and_row(html, variant):
    cd = cd_of(variant)
    shapes = V.shape_streams(html, variant)
    streams = list(shapes.values()) + V.seven_by_three(html)
    want = check(cd, streams, X.build_index(streams))
    assert want["status"] == [O.OK] * len(streams) and want["result"][4] == 65536 and want["result"][1] == 0
    for s in shapes.values():                                           # each alone: 0 rows, 1 row, ...
        check(cd, [s], X.build_index([s]), lead=2)


def test_foreign_streams_of_the_grammar_corpus():
    import stream_grammar as G
    cd = cd_of()
    streams = [s for _, s, _ in G.frame_corpus()]
    want = check(cd, streams, X.build_index(streams))
    assert O.OK in want["status"] and any(v not in (O.OK, V.SKIPPED) for v in want["row_status"])     # the corpus has good and bad chunks
    for b, s in enumerate(streams):                                     # guarantee (a): OK exactly when the oracle decodes the whole stream
        assert (want["status"][b] == O.OK) == (V.chunk_status(s[10:]) == O.OK)


@pytest.mark.parametrize("variant", VARIANTS)
def test_streams_after_splice_and_append(variant):
    from append_harness import arena_of
    cd = cd_of(variant)
    text = read_testdata("html") * 2
    raws = [text[:20000], text[300:9000], b"", text[:50]]
    ns = len(raws)
    data, doff, dlen = H.pack(raws)
    base, base_off, base_len, st, _, base_ix = cd.frame_encode_seekable(data, H.dev(doff), H.dev(dlen), chunk_bytes=1024)
    edits, ins = [(4000, 0), (7000, 900), (0, 0), (0, 0)], [text[100:137], b"", b"", text[:3]]
    isrc, ioff, ilen = H.pack(ins)
    s_out, s_off, s_len, s_st, s_ix = cd.frame_splice_to_memory(base, base_off, base_len, base_ix, H.dev([q[0] for q in edits]),
                                                                H.dev([q[1] for q in edits]), isrc, H.dev(ioff), H.dev(ilen), 1024)
    assert st.tolist() == s_st.tolist() == [O.OK] * ns
    hb, hs = base.cpu().numpy(), s_out.cpu().numpy()
    spliced = [(hs[o:o + n] if n else hb[bo:bo + bn]).tobytes() for o, n, bo, bn in zip(s_off.tolist(), s_len.tolist(), base_off.tolist(), base_len.tolist())]
    more = [text[777:777 + n] for n in (700, 1, 0, 300)]
    caps = [len(s) + len(m) + 8 * (len(m) // 1024 + 2) + 64 for s, m in zip(spliced, more)]
    buf, boff = arena_of(spliced, caps)
    asrc, aoff, alen = H.pack(more)
    new_len, a_st, a_ix = cd.frame_append_to_memory(buf, H.dev(boff), H.dev([len(s) for s in spliced]), H.dev(caps), s_ix, asrc, H.dev(aoff), H.dev(alen), 1024)
    assert a_st.tolist() == [O.OK] * ns
    got = cd.frame_verify_indexed(buf, H.dev(boff), new_len, a_ix)      # the wrapper, over the index the append handed back
    torch.cuda.synchronize()
    hbuf = buf.cpu().numpy()
    grown = [hbuf[o:o + n].tobytes() for o, n in zip(boff, new_len.tolist())]
    want = V.verify_plan(grown, X.build_index(grown))
    rows = len(want["row_status"])
    assert got[0].tolist()[:rows] == want["row_status"] and got[1].tolist() == want["status"] == [O.OK] * ns
    assert got[6].tolist()[:6] == want["result"][:6]
    check(cd, grown, X.build_index(grown), 1024, 5 * 1024)


# ---- 2: rounds -------------------------------------------------------------------------------------------------------------------------------------
def test_round_borders_inside_and_between_streams_and_every_layout(html):
    cd = cd_of()
    streams = V.seven_by_three(html)
    ix = X.build_index(streams)
    stride = 2512                                                       # the longest row is 2500
    base = None
    for per, rounds in ((1, 21), (2, 11), (3, 7), (7, 3), (8, 3), (21, 1), (1000, 1)):
        want = check(cd, streams, ix, 2500, per * stride + 5)
        assert want["result"][6] == rounds and want["status"] == [O.OK] * 3
        base = base or want
        assert {k: want[k] for k in VERIFY_KEYS[:6]} == {k: base[k] for k in VERIFY_KEYS[:6]}      # (b): nothing depends on scratch_cap
    # one byte below the stride: the sizing call
    sizing = check(cd, streams, ix, 2500, stride - 1)
    assert sizing["row_status"] == [O.ERR_OUTPUT_TOO_SMALL] * 21 and sizing["result"][4:7] == [2500, 21, 0]
    check(cd, streams, ix, 65536, 0)
    # a slot below the largest row: those rows are left unverified, the rest verified
    small = check(cd, streams, ix, 1000, 3 * 1008)
    assert small["result"][5] == sum(1 for v in small["row_status"] if v == O.ERR_OUTPUT_TOO_SMALL) == 12 and small["row_status"].count(O.OK) == 9
    # (b): every decode layout
    for layout in DECODE_LAYOUTS:
        other = cd_of()
        set_decode_layout(other.ctx, layout)
        got = verify_call(other, streams, ix, 2500, 3 * stride)
        assert {k: got[k] for k in VERIFY_KEYS[:6]} == {k: base[k] for k in VERIFY_KEYS[:6]}, layout


# ---- 3: damage -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("compressed", [False, True])
def test_every_single_bit_flip_of_a_short_chunk(html, compressed):
    """Every flip, in turn, in one batch of one stream each: type byte, length bytes, CRC bytes, body.  An uncompressed chunk: every flip
    is a bad row.  A compressed one: every flip but those after which the reference's own decoder still gives the chunk's bytes
    (V.same_bytes_flips: test_frame_verify_model.py says why)."""
    cd = cd_of()
    s, ix1, lo, n = V.flip_stream(html, compressed)
    harmless = V.same_bytes_flips(s, lo, n)
    assert not harmless if not compressed else len(harmless) < 8
    flips = [(at, bit) for at in range(lo, lo + n) for bit in range(8)]
    streams = [V.flip(s, at, bit) for at, bit in flips]
    ix = dict(first=[3 * k for k in range(len(flips) + 1)], start=ix1["start"] * len(flips), pos=ix1["pos"] * len(flips),
              total=ix1["total"] * len(flips), tail=[O.OK] * len(flips))
    want = check(cd, streams, ix, 512, 64 * 512)
    for k, f in enumerate(flips):
        assert (want["row_status"][3 * k + 1] == O.OK) == (f in harmless), f
        assert want["row_status"][3 * k] == want["row_status"][3 * k + 2] == O.OK
    assert {O.ERR_BAD_ARG, O.ERR_CRC_MISMATCH} <= set(want["row_status"])


def test_damage_in_first_and_last_rows_at_round_borders_and_everywhere(html):
    cd = cd_of()
    streams = V.seven_by_three(html)
    ix = X.build_index(streams)
    for rows in ([0], [20], [0, 20], [5, 6], [6, 7], [8, 9], list(range(21))):
        bad = list(streams)
        for r in rows:
            bad[r // 7] = V.flip(bad[r // 7], ix["pos"][r] + 9, 3)      # a body byte
        want = check(cd, bad, ix, 2500, 3 * 2512)                       # rounds of 3 rows: borders at rows 3, 6, 9, ...
        assert [i for i, v in enumerate(want["row_status"]) if v != O.OK] == rows and want["result"][1] == len(rows)
    # a truncated last chunk
    want = check(cd, [streams[0], streams[1][:-1], streams[2]], ix)
    assert want["row_status"][13] == O.ERR_BAD_ARG and want["status"] == [O.OK, O.ERR_BAD_ARG, O.OK] and want["first_bad"][1] == 13
    # a damaged identifier: flags alone
    want = check(cd, [V.flip(streams[0], 4, 0)] + streams[1:], ix)
    assert want["flags"] == [1, 0, 0] and want["status"] == [O.OK] * 3
    # a stream with a broken idx_tail is skipped alone
    k = {key: list(v) for key, v in ix.items()}
    k["tail"][1] = O.ERR_CRC_MISMATCH
    want = check(cd, streams, k)
    assert want["status"] == [O.OK, O.ERR_CRC_MISMATCH, O.OK] and want["row_status"][7:14] == [V.SKIPPED] * 7 and want["result"][0] == 14


# ---- 4: unsound indexes ----------------------------------------------------------------------------------------------------------------------------
def test_unsound_indexes_write_nothing_outside_the_guards(html):
    cd = cd_of()
    streams = V.seven_by_three(html) + [V.shape_streams(html)["sizes"], V.shape_streams(html)["skippable_between"]]
    ix = X.build_index(streams)
    rng = np.random.default_rng(2)
    cases = V.unsound_indexes(ix, streams, rng)
    assert {"a_tail_that_is_not_ok", "first_runs_backwards", "a_position_outside_in_len", "random_words"} <= set(cases)
    failed = 0
    for name, bad in cases.items():
        want = check(cd, streams, bad, 65536, 4 * 65536)
        failed += sum(1 for s in want["status"] if s != O.OK)
    assert failed > 10
    for k in range(3):                                                  # an index filled with random words, others
        bad = V.unsound_indexes(ix, streams, rng)["random_words"]
        check(cd, streams, bad, (1000, 65536, 17)[k], (1 << 20, 70000, 16)[k])


# ---- 5: the planner ----------------------------------------------------------------------------------------------------------------------------------
def test_planner_merges_runs_for_every_pattern_of_1_to_8_rows():
    """All 510 patterns as the streams of ONE index, one pair each, in one call; zero-length rows at run borders."""
    cd = cd_of()
    lens = [5, 0, 3, 7, 0, 0, 2, 9]
    ix, rs = dict(first=[0], start=[], pos=[], total=[], tail=[]), []
    for n in range(1, 9):
        for mask in range(1 << n):
            ix["start"] += [sum(lens[:i]) for i in range(n)]
            ix["first"].append(len(ix["start"]))
            ix["total"].append(sum(lens[:n]))
            ix["tail"].append(O.OK)
            rs += [O.OK if mask >> i & 1 else (O.ERR_CRC_MISMATCH, V.SKIPPED, O.ERR_BAD_ARG, O.ERR_OUTPUT_TOO_SMALL)[i % 4] for i in range(n)]
    ns = len(ix["total"])
    assert ns == 510
    ix["pos"] = [0] * len(ix["start"])
    pairs = list(range(ns))
    want = check_plan(cd, ix, ns, rs, ix["total"], [O.OK] * ns, pairs, pairs)
    assert want["plan_status"] == [O.OK] * ns and want["result"][1] == ns
    # a long stream: runs that cross the tiles of the walk (256 rows), a run of exactly one tile, zero-length rows on a tile's border
    rng = np.random.default_rng(8)
    n = 2000
    ln = [int(v) for v in rng.integers(0, 4, n)]
    ln[255] = ln[256] = ln[511] = 0
    good = [bool(v) for v in rng.integers(0, 2, n)]
    good[600:856] = [True] * 256
    good[1000:1700] = [False] * 700
    long_ix = dict(first=[0, n], start=[sum(ln[:i]) for i in range(n)], pos=[0] * n, total=[sum(ln)], tail=[O.OK])
    check_plan(cd, long_ix, 1, [O.OK if g else O.ERR_CRC_MISMATCH for g in good], [sum(ln)] * 2, [O.OK] * 2, [0, 0], [0, 1])


def test_planner_rejections_admission_and_the_sizing_call():
    cd = cd_of()
    ix = dict(first=[0, 2, 2, 5], start=[0, 10, 0, 6, 9], pos=[0] * 5, total=[30, 0, 12], tail=[O.OK, O.OK, O.OK])
    rs = [O.OK, O.ERR_CRC_MISMATCH, O.ERR_CRC_MISMATCH, O.OK, O.ERR_BAD_ARG]
    rep_total, rep_tail = [30, 0, 12, 12, 13], [O.OK, O.OK, O.OK, O.ERR_TRUNCATED_STREAM, O.OK]
    # every rejection, in one call, among pairs that pass
    want = check_plan(cd, ix, 3, rs, rep_total, rep_tail, [0, 3, 0, 2, 2, 0, 2, 1], [0, 0, 5, 3, 4, 2, 2, 1])
    assert want["plan_status"] == [O.OK] + [O.ERR_BAD_ARG] * 5 + [O.OK, O.OK]
    for tail in (O.ERR_CRC_MISMATCH, 77, -1):
        assert check_plan(cd, dict(ix, tail=[tail, O.OK, O.OK]), 3, rs, rep_total, rep_tail, [0, 2], [0, 2])["plan_status"] == [O.ERR_BAD_ARG, O.OK]
    assert check_plan(cd, dict(ix, first=[3, 2, 2, 5]), 3, rs, rep_total, rep_tail, [0], [0])["plan_status"] == [O.ERR_BAD_ARG]
    # admission at max_segs - 1, max_segs, max_segs + 1 of every pair's need, and the sizing call
    for ms in (0, 1, 2, 3, 4, 5, 6):
        want = check_plan(cd, ix, 3, rs, rep_total, rep_tail, [0, 1, 2], [0, 1, 2], ms)
        assert want["result"][0] == 5 and want["plan_status"] == [O.OK if need <= ms else O.ERR_OUTPUT_TOO_SMALL for need in (2, 2, 5)]
    none = plan_call(cd, ix, 3, rs, rep_total, rep_tail, [], [], 4)
    assert none == dict(plan_status=[], result=[0] * 4)
    # arrays filled with anything
    rng = np.random.default_rng(5)
    for _ in range(4):
        words = lambda n: [int(v) for v in rng.integers(0, 1 << 63, n, dtype=np.uint64) * 2 + rng.integers(0, 2, n, dtype=np.uint64)]      # noqa: E731
        wild = dict(first=words(4), start=words(9), pos=[0] * 9, total=words(3), tail=[O.OK, int(rng.integers(-5, 15)), O.OK])
        wild["first"][0] = 0
        check_plan(cd, wild, 3, [int(v) for v in rng.integers(-1, 2, 9)], wild["total"], [O.OK] * 3, [0, 1, 2, 7], [0, 1, 2, 0], 5)


# ---- 6: end to end --------------------------------------------------------------------------------------------------------------------------------
def encoded(cd, raws, cb=None, window=None):
    data, off, lens = H.pack(raws)
    if window:
        out, out_off, out_len, st, _, index = cd.frame_encode_content_defined(data, H.dev(off), H.dev(lens), window, 2048)
    else:
        out, out_off, out_len, st, _, index = cd.frame_encode_seekable(data, H.dev(off), H.dev(lens), chunk_bytes=cb)
    assert st.tolist() == [O.OK] * len(raws)
    return out.clone(), out_off, out_len, index


def streams_of(out, off, lens):
    h = out.cpu().numpy()
    return [h[o:o + n].tobytes() for o, n in zip(off.tolist(), lens.tolist())]


def damage(store, rows, byte=9):
    """One bit of a body byte of every named row, on the device."""
    out, out_off, _, index = store
    first, pos = index.first.tolist(), index.pos.tolist()
    for r in rows:
        b = max(k for k in range(len(first) - 1) if first[k] <= r)
        out[int(out_off[b]) + pos[r] + byte] ^= 4


@pytest.mark.parametrize("window", [0, 64])
@pytest.mark.parametrize("nbad", [1, 2, "all"])
def test_repair_from_an_identical_copy_is_byte_for_byte(html, window, nbad):
    """Guarantee (c), on seekable (4096) and content-defined stores of html; 1, 2 and all chunks of the first stream damaged."""
    cd = cd_of()
    raws = [html[:30000], html[30000:31000], html[40000:65000]]
    store = encoded(cd, raws, 4096, window)
    copy = (store[0].clone(), store[1], store[2], store[3])
    good = streams_of(*store[:3])
    rows0 = int(store[3].first[1])
    rows = {1: [3], 2: [0, rows0 - 1], "all": list(range(rows0))}[nbad] + [int(store[3].first[2]) + 1]
    damage(store, rows)
    damaged, out, out_off, out_len, status, new_index = cd.frame_repair_streams(*store, *copy)
    torch.cuda.synchronize()
    assert damaged == [0, 2] and status.tolist() == [O.OK, O.OK]
    assert streams_of(out, out_off, out_len) == [good[0], good[2]]
    bad = streams_of(*store[:3])
    want = V.verify_plan(bad, X.build_index(good))                      # the wrapper's first verify, against the model
    got = cd.frame_verify_indexed(*store)
    torch.cuda.synchronize()
    n = len(want["row_status"])
    assert got[0].tolist()[:n] == want["row_status"] and got[1].tolist() == want["status"] and got[2].tolist() == want["nbad"]
    assert [i for i, v in enumerate(want["row_status"]) if v != O.OK] == rows


def test_repair_from_a_replica_at_another_chunking_and_damage_on_both_sides(html):
    """Guarantee (d): the same decoded bytes, a clean verify, the replica's digest.  Then damage on both sides in the same range."""
    cd = cd_of()
    raws = [html[:70000], html[70000:90000]]
    store, replica = encoded(cd, raws, 4096), encoded(cd, raws, 65536)
    damage(store, [2, 9, int(store[3].first[1])])
    damaged, out, out_off, out_len, status, new_index = cd.frame_repair_streams(*store, *replica, chunk_bytes=4096)
    torch.cuda.synchronize()
    assert damaged == [0, 1] and status.tolist() == [O.OK, O.OK]
    assert [O.frame_decode(s) for s in streams_of(out, out_off, out_len)] == raws
    dig, dlen, dst = cd.frame_digest_streams(out, out_off, out_len, new_index)
    rdig, rlen, rst = cd.frame_digest_streams(*replica)
    torch.cuda.synchronize()
    assert dig.tolist() == rdig.tolist() and dlen.tolist() == rlen.tolist() and dst.tolist() == rst.tolist() == [O.OK, O.OK]
    assert [v & 0xFFFFFFFF for v in dig.tolist()] == [O.crc32c(x) for x in raws]
    # the replica's first chunk rots too: stream 0 is reported still bad, stream 1 is repaired
    damage(replica, [0], byte=50)
    damaged, out, out_off, out_len, status, _ = cd.frame_repair_streams(*store, *replica, chunk_bytes=4096)
    torch.cuda.synchronize()
    assert damaged == [0, 1] and status.tolist()[0] != O.OK and status.tolist()[1] == O.OK
    # ... and from a byte-identical copy with the SAME chunks rotten deep in their bodies the compose copies the bad chunks as they are:
    # only the second verify can tell
    again = encoded(cd, raws, 4096)
    damage(again, [2, 9, int(again[3].first[1])], byte=50)
    twin = (again[0].clone(), again[1], again[2], again[3])
    damaged, out, out_off, out_len, status, _ = cd.frame_repair_streams(*again, *twin)
    torch.cuda.synchronize()
    assert damaged == [0, 1] and all(v != O.OK for v in status.tolist())
    assert streams_of(out, out_off, out_len) == streams_of(*again[:3])  # (the compose did copy them)
    # nothing damaged: nothing to do
    clean = encoded(cd, raws, 4096)
    assert cd.frame_repair_streams(*clean, *replica)[0] == []


# ---- 7: two runs; graph capture; the ABI ------------------------------------------------------------------------------------------------------------
def wrapper_arrays(got):
    return [t.tolist() for t in got]


def test_two_runs_and_graph_capture_give_the_same_arrays(html):
    cd = cd_of()
    sets = [V.seven_by_three(html), V.seven_by_three(html[5000:])]
    ixs = [X.build_index(b) for b in sets]                              # (the caller's index: it survives the damage)
    sets[1][1] = V.flip(sets[1][1], ixs[1]["pos"][9] + 12, 2)           # a body byte of the stream's third row
    sets[1][2] = V.flip(sets[1][2], 4, 2)                               # the identifier
    ne = 21
    size = max(sum(len(s) for s in b) for b in sets)
    lens = [[len(s) for s in b] for b in sets]
    framed = torch.zeros(size + 64, dtype=torch.uint8, device="cuda")
    d_off, d_len = torch.zeros(3, dtype=torch.int64, device="cuda"), torch.zeros(3, dtype=torch.int64, device="cuda")
    index = SB.FrameIndex(torch.zeros(4, dtype=torch.int64, device="cuda"), torch.zeros(ne, dtype=torch.int64, device="cuda"),
                          torch.zeros(ne, dtype=torch.int64, device="cuda"), torch.zeros(3, dtype=torch.int64, device="cuda"),
                          torch.zeros(3, dtype=torch.int32, device="cuda"))
    slot, cap = 2500, 4 * 2512
    work = torch.zeros(N.frame_verify_lib().snp_frame_verify_indexed_workspace(3, ne, slot, cap), dtype=torch.uint8, device="cuda")
    pwork = torch.zeros(N.frame_verify_lib().snp_frame_repair_plan_workspace(3), dtype=torch.uint8, device="cuda")
    pairs = torch.arange(3, dtype=torch.int32, device="cuda")

    def fill(k):
        off = np.concatenate([[0], np.cumsum(lens[k])[:-1]]).astype(np.int64)
        framed[:sum(lens[k])].copy_(torch.from_numpy(np.frombuffer(b"".join(sets[k]), dtype=np.uint8).copy()).cuda())
        d_off.copy_(H.dev(off))
        d_len.copy_(H.dev(lens[k]))
        for key, t in zip(KEYS, index_tensors(ixs[k], 3)[0]):
            getattr(index, key).copy_(t)

    def call():
        got = cd.frame_verify_indexed(framed, d_off, d_len, index, slot, cap, work)
        plan_status, recipe, result = cd.frame_repair_plan(index, got[0], index, pairs, pairs, 9, pwork)
        return list(got) + [plan_status, *recipe, result]

    def expect(k, arrays):
        want = V.verify_plan(sets[k], ixs[k], slot, cap)
        assert [arrays[0], arrays[1], arrays[2], u64s(arrays[3]), u64s(arrays[4]), arrays[5], u64s(arrays[6])] == [want[key] for key in VERIFY_KEYS]
        plan = V.repair_plan(ixs[k], 3, want["row_status"], ixs[k]["total"], ixs[k]["tail"], [0, 1, 2], [0, 1, 2], 9)
        nsegs = plan["segs"]["first"][-1]
        assert arrays[7] == plan["plan_status"] and arrays[8] == plan["segs"]["first"] and arrays[12] == plan["result"]
        assert [a[:nsegs] for a in arrays[9:12]] == [plan["segs"][key] for key in ("stream", "off", "len")]
        return want

    fill(0)
    first = wrapper_arrays(call())
    second = wrapper_arrays(call())
    torch.cuda.synchronize()
    assert first == second                                              # two runs of the same calls
    assert expect(0, first)["status"] == [O.OK] * 3
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
    g.replay()
    torch.cuda.synchronize()
    replayed = wrapper_arrays(got)
    want = expect(1, replayed)
    assert want["status"][0] == O.OK and want["status"][1] != O.OK and want["flags"] == [0, 0, 1]
    eager = wrapper_arrays(call())
    torch.cuda.synchronize()
    assert eager == replayed


def test_abi_null_pointers_ranges_and_an_empty_batch(html):
    cd = cd_of()
    VL = N.frame_verify_lib()
    cd._bind()
    none = verify_call(cd, [], dict(first=[0], start=[], pos=[], total=[], tail=[]))
    assert none["result"] == [0] * 8 and none["row_status"] == [] and none["status"] == []
    streams = V.seven_by_three(html)[:1]
    ix = X.build_index(streams)
    framed, in_off, in_len = H.pack(streams)
    ixt, ne = index_tensors(ix, 1)
    outs = [torch.zeros(8, dtype=torch.int64, device="cuda") for _ in range(6)]
    work = torch.zeros(VL.snp_frame_verify_indexed_workspace(1, ne, 4096, 1 << 20), dtype=torch.uint8, device="cuda")
    result = torch.zeros(8, dtype=torch.int64, device="cuda")
    full = [_p(framed), _p(dev_u64(in_off)), _p(dev_u64(in_len))] + [_p(t) for t in ixt] + [_p(t) for t in outs] + [_p(work)]

    def call(null=(), ns=1, nent=ne, slot=4096, cap=1 << 20, res=result, ctx=cd.ctx.handle):
        p = [C.c_void_p(None) if i in null else v for i, v in enumerate(full)]
        return VL.snp_frame_verify_indexed_batch(ctx, *p[:3], ns, *p[3:8], nent, slot, cap, *p[8:15], _p(res) if res is not None else None)

    assert call() == O.OK
    for i in range(15):
        assert call(null=(i,)) == O.ERR_BAD_ARG, i
    assert call(slot=0) == call(slot=65537) == call(ns=1 << 31) == call(nent=1 << 31) == call(res=None) == call(ctx=None) == O.ERR_BAD_ARG
    assert VL.snp_frame_verify_indexed_workspace(1, ne, 0, 1 << 20) == 0 and VL.snp_frame_repair_plan_workspace(0) == 0
    torch.cuda.synchronize()
    with pytest.raises(ValueError):
        cd.frame_verify_indexed(framed, dev_u64(in_off), dev_u64(in_len), SB.FrameIndex(*ixt), 65537)

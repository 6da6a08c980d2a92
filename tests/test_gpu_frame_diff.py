"""snp_frame_diff_indexed_batch (BlockCodec.frame_diff_indexed / frame_diff_streams / frame_delta_streams): prefix, suffix, lengths, status and
d_result against the model (tests/frame_diff_model.py) and, where the model is not blind, against the ground truth (plain comparison of the
oracle's decodes), with guard words around every output array and the workspace (diff_call): every difference position under four pairs of
chunk grids; windows with no common cut; windows of every kind; the splice found again after splice and rechunk; foreign streams; unsound
indexes on either side; corruption and a constructed CRC collision; 70 000 rows under one request beside 70 000 requests of one row; admission
by both bounds and the two sizing rounds; windows past 2^32 bytes; graph capture.  Each check runs with PREFIX, SUFFIX, both, and EXACT.
Needs an MI355X."""
import ctypes as C

import numpy as np
import pytest
import torch

import frame_buffers_helpers as H
import frame_chunked_model as K
import frame_diff_model as F
import frame_index_model as X
import frame_range_model as R
import oracle as O
import stream_grammar as G
from conftest import read_testdata
from seekable_harness import Guarded, dev_i32, dev_u64
from test_frame_diff_model import collide, side_of, tiled, unsound_indexes, whole

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from snappier_amd import batch as SB, _native as N

U64 = F.U64
P, S, E = F.PREFIX, F.SUFFIX, F.EXACT
MODES = [P, S, P | S, P | S | E]
B = 65536


def codec():
    return SB.BlockCodec(0, O.HASH_CRC32C)


def _p(t):
    return C.c_void_p(t.data_ptr()) if t.numel() else C.c_void_p(None)


def side_tensors(sd: F.Side, lead=1, gap=3):
    ns, ix = len(sd.streams), sd.ix
    framed, in_off, in_len = H.pack(sd.streams, lead, gap) if ns else (torch.zeros(16, dtype=torch.uint8, device="cuda"), [], [])
    ne = min(len(ix["start"]), len(ix["pos"]))
    tabs = [framed] + [dev_u64(x) for x in (in_off, in_len, ix["first"], ix["start"] or [0], ix["pos"] or [0], ix["total"])] + [dev_i32(ix["tail"])]
    return tabs, ns, ne


def diff_call(cd, a: F.Side, b: F.Side, requests, flags, max_rows, scratch_cap):
    """snp_frame_diff_indexed_batch called directly, the five outputs, d_result and the workspace between guard elements (one set of arrays
    for both sides when they are one): -> what F.diff_plan returns."""
    nreq = len(requests)
    DL = N.frame_diff_lib()
    cd._bind()
    ta, nsa, nea = side_tensors(a)
    tb, nsb, neb = (ta, nsa, nea) if b is a else side_tensors(b, 2, 5)
    outs = [Guarded(nreq, torch.int64) for _ in range(4)]
    status, result = Guarded(nreq, torch.int32), Guarded(4, torch.int64)
    work = Guarded(DL.snp_frame_diff_indexed_workspace(nreq, max_rows, scratch_cap), torch.uint8)
    s32 = lambda v: v - (1 << 32) if v >= 1 << 31 else v
    req = [dev_i32([s32(q[0]) for q in requests]), dev_u64([q[1] for q in requests]), dev_u64([q[2] for q in requests]),
           dev_i32([s32(q[3]) for q in requests]), dev_u64([q[4] for q in requests]), dev_u64([q[5] for q in requests])]
    st = DL.snp_frame_diff_indexed_batch(cd.ctx.handle, *[_p(t) for t in ta[:3]], nsa, *[_p(t) for t in ta[3:]], nea,
                                         *[_p(t) for t in tb[:3]], nsb, *[_p(t) for t in tb[3:]], neb, *[_p(t) for t in req], nreq, flags, max_rows,
                                         scratch_cap, *[g.ptr() for g in outs], status.ptr(), work.ptr(), result.ptr())
    assert st == O.OK
    torch.cuda.synchronize()
    work.read()
    len_a, len_b, prefix, suffix = [g.read() for g in outs]
    return status.read(), len_a, len_b, prefix, suffix, result.read()


def check(cd, a, b, requests, flags, max_rows=None, scratch_cap=None):
    """The call against the model under the same bounds (default: what admits every request)."""
    if max_rows is None or scratch_cap is None:
        rows, scratch = F.needs(a, b, requests, flags)
        max_rows = rows if max_rows is None else max_rows
        scratch_cap = scratch if scratch_cap is None else scratch_cap
    got = diff_call(cd, a, b, requests, flags, max_rows, scratch_cap)
    want = F.diff_plan(a, b, requests, flags, max_rows, scratch_cap)
    assert got[0] == want[0], [(r, requests[r], g, w) for r, (g, w) in enumerate(zip(got[0], want[0])) if g != w][:10]
    for k, name in ((1, "len_a"), (2, "len_b"), (3, "prefix"), (4, "suffix")):
        assert got[k] == want[k], (name, flags, [(r, requests[r], g, w) for r, (g, w) in enumerate(zip(got[k], want[k])) if g != w][:10])
    assert got[5] == want[5], (got[5], want[5])
    return got


def check_truth(a, b, requests, flags, got):
    for r, (ba, oa, la, bb, ob, lb) in enumerate(requests):
        if got[0][r] != O.OK:
            continue
        x, y = F.window_bytes(a.streams[ba], oa, la), F.window_bytes(b.streams[bb], ob, lb)
        assert (got[1][r], got[2][r]) == (len(x), len(y)) and (got[3][r], got[4][r]) == F.truth(x, y, flags), (r, flags, requests[r])


@pytest.fixture(scope="module")
def html():
    return read_testdata("html") * 3


# ---- 1. every difference position ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ca, cb", [(1, 7), (7, 21), (5, 7), (7, 7)])
def test_every_difference_position_of_a_small_buffer(ca, cb):
    cd = codec()
    raw = bytes(np.random.default_rng(ca * 100 + cb).integers(0, 256, 300, dtype=np.uint8))
    a = side_of([K.stream_of(raw, ca)])
    b = side_of([K.stream_of(raw[:p] + bytes([raw[p] ^ 0x40]) + raw[p + 1:], cb) for p in range(300)] + [K.stream_of(raw, cb)])
    reqs = [whole(0, p) for p in range(301)]
    for flags in MODES:
        got = check(cd, a, b, reqs, flags)                              # one call
        assert got[0] == [O.OK] * 301
        assert got[3] == ([*range(300), 300] if flags & P else [0] * 301)
        assert got[4] == ([299 - p for p in range(300)] + [0] if flags & P and flags & S else [299 - p for p in range(300)] + [300] if flags & S else [0] * 301)


@pytest.mark.parametrize("ca, cb", [(4096, 65536), (4096, 4096)])
def test_every_difference_position_class_of_200_kib(ca, cb, html):
    cd = codec()
    raw = html[:200 * 1024]
    n = len(raw)
    rng = np.random.default_rng(cb)
    places = sorted({p for c in range(0, n + 1, 4096) for p in (c - 1, c, c + 1) if 0 <= p < n} | {int(v) for v in rng.integers(0, n, 64)})
    a = side_of([K.stream_of(raw, ca)])
    b = side_of([K.stream_of(raw[:p] + bytes([raw[p] ^ 1]) + raw[p + 1:], cb) for p in places] + [K.stream_of(raw, cb)])
    reqs = [whole(0, i) for i in range(len(places) + 1)]
    for flags in MODES:
        got = check(cd, a, b, reqs, flags)
        assert got[3] == ([*places, n] if flags & P else [0] * len(reqs))
        if flags & S:
            assert got[4][:-1] == [n - 1 - p for p in places]
        if not flags & E:                                               # (the model says so first: only the spans around the differences)
            assert got[5][2] <= 2 * len(places) * (cb + max(ca, cb)) and F.diff_plan(a, b, reqs[-1:], flags, 1 << 20, 0)[5][2:] == [0, 1]


# ---- 2. no common cut ------------------------------------------------------------------------------------------------------------------------------
def test_windows_with_no_common_cut(html):
    cd = codec()
    ragged = html[1000:1000 + 5 * 777 + 31]
    period1 = b"\x55" * 3000
    a = side_of([K.stream_of(ragged, 777), K.stream_of(period1, 512), tiled(ragged, [100, 900, 2000])])
    n = len(ragged)
    reqs = [(0, 0, n - 1, 0, 1, n - 1), (1, 0, 2999, 1, 1, 2999), (1, 5, 1000, 1, 6, 1000),       # off_b = off_a + 1
            (0, 777, 777 * 2, 0, 777 + 300, 777 * 2), (0, 300, 1000, 0, 300, 1000),                 # one window, or both, from mid-chunk
            (0, 0, 777, 2, 0, 777), (0, 777, 50, 2, 777, 50), (2, 100, 800, 0, 100, 800)]
    for flags in MODES:
        got = check(cd, a, a, reqs, flags)
        check_truth(a, a, reqs, flags, got)
        assert got[0] == [O.OK] * len(reqs)
    got = check(cd, a, a, reqs, P | S)
    assert (got[3][1], got[4][1]) == (2999, 0) and (got[3][2], got[4][2]) == (1000, 0) and got[3][0] < 20


# ---- 3. windows ------------------------------------------------------------------------------------------------------------------------------------
def test_windows_of_every_kind_in_any_order(html):
    cd = codec()
    raw = html[50:50 + 9 * 4096 + 123]
    other = raw[:20000] + b"#" + raw[20001:30000] + raw[30010:]
    a, b = side_of([K.stream_of(raw, 4096), K.stream_of(b"", 4096)]), side_of([K.stream_of(other, 1024), K.stream_of(raw + b"more", 4096)])
    n = len(raw)
    reqs = [whole(0, 0), whole(0, 1), whole(1, 0), whole(1, 1), (0, 0, 0, 0, 0, 0), (0, n, 5, 1, n, 5), (0, n - 10, 100, 1, n - 10, 100),
            (0, 5000, 10, 0, 5, 10), (0, 4096, 4096, 0, 4096, 4096), (0, 4096, 8192, 1, 4096, 4096), (0, 19000, 3000, 0, 19000, 2000),
            (0, 1, n, 1, 0, U64), (0, U64, U64, 0, U64 - 1, 2), (0, 30000, 5000, 0, 29990, 5000), (0, 20001, 100, 0, 20001, 100)]
    rng = np.random.default_rng(4)
    for _ in range(40):
        oa = int(rng.integers(0, n))
        reqs.append((0, oa, int(rng.integers(0, 9000)), int(rng.integers(0, 2)), oa + int(rng.integers(0, 2)) * int(rng.integers(0, 50)), int(rng.integers(0, 9000))))
    order = [int(v) for v in rng.permutation(len(reqs))]
    reqs = [reqs[i] for i in order]
    for flags in MODES:
        got = check(cd, a, b, reqs, flags)
        assert got[0] == [O.OK] * len(reqs)
        check_truth(a, b, reqs, flags, got)


# ---- 4. the use case -------------------------------------------------------------------------------------------------------------------------------
def pack_raw(raws):
    data = torch.from_numpy(np.frombuffer(b"".join(raws) or b"\0", dtype=np.uint8).copy()).cuda()
    lens = np.array([len(x) for x in raws], dtype=np.int64)
    return data, H.dev(np.cumsum(lens) - lens), H.dev(lens)


def test_the_splice_is_found_again_and_repairs_the_replica(html):
    cd = codec()
    cb = 4096
    raw = html[7:7 + 12 * cb + 300]
    n = len(raw)
    edits = [(5000, 0, 4096), (5000, 3000, 0), (8192, 100, 5000), (9000, 6000, 10), (10000, n - 10000, 0), (0, 7000, 0)]
    names = ["insert", "delete", "longer", "shorter", "truncate", "drop-prefix"]
    ns = len(edits)
    ins = [html[200000 + 1000 * i:200000 + 1000 * i + ln] for i, (_, _, ln) in enumerate(edits)]
    data, in_off, in_len = pack_raw([raw] * ns)
    old, old_off, old_len, status, _, old_ix = cd.frame_encode_seekable(data, in_off, in_len, chunk_bytes=cb)
    assert status.tolist() == [O.OK] * ns
    A = (old, old_off, old_len, old_ix)
    src, src_off, src_len = pack_raw(ins)
    sp = cd.frame_splice_to_memory(*A, dev_u64([e[0] for e in edits]), dev_u64([e[1] for e in edits]), src, src_off, src_len, cb)
    assert sp[3].tolist() == [O.OK] * ns
    spliced = (sp[0], sp[1], sp[2], sp[4])
    rc = cd.frame_rechunk_to_memory(*spliced, 1024)                     # ... and B is also rechunked, to another grid
    assert rc[3].tolist() == [O.OK] * ns and int(rc[2].min()) > 0
    rechunked = (rc[0], rc[1], rc[2], rc[4])
    want_dg = cd.frame_digest_streams(*spliced)
    req_stream = torch.arange(ns, dtype=torch.int32, device="cuda")
    for Bside in (spliced, rechunked):
        off, dele, ins_off, ins_len, dstatus = cd.frame_delta_streams(A, Bside)
        assert dstatus.tolist() == [O.OK] * ns
        for i, (eo, ed, el) in enumerate(edits):
            o, d, ln = int(off[i]), int(dele[i]), int(ins_len[i])
            assert d <= ed and ln <= el and d - ln == ed - el, names[i]  # the hole is no larger than the one applied
            assert int(ins_off[i]) == o and d + ln > 0, names[i]
        # the repair: read B[ins_off, +ins_len), splice it into A
        data_off = torch.cumsum(ins_len, 0) - ins_len
        fetched = torch.empty(max(int(ins_len.sum()), 1), dtype=torch.uint8, device="cuda")
        rd = cd.frame_read_indexed(*Bside, req_stream, ins_off, ins_len, fetched, data_off, ins_len)
        assert rd[1].tolist() == [O.OK] * ns
        fx = cd.frame_splice_to_memory(*A, off, dele, fetched, data_off, ins_len, cb)
        assert fx[3].tolist() == [O.OK] * ns
        fixed = (fx[0], fx[1], fx[2], fx[4])
        got_dg = cd.frame_digest_streams(*fixed)
        assert all(torch.equal(x, y) for x, y in zip(got_dg, want_dg))
        for exact in (False, True):
            pre, suf, la, lb, st = cd.frame_diff_streams(fixed, Bside, exact=exact)
            assert st.tolist() == [O.OK] * ns and torch.equal(pre, la) and torch.equal(la, lb) and int(suf.sum()) == 0


# ---- 5. foreign streams ----------------------------------------------------------------------------------------------------------------------------
def test_foreign_streams_of_the_stream_grammar():
    cd = codec()
    frames = G.frame_corpus()
    streams = [s for _n, s, _r in frames] + [R.tiny_chunk_stream(1)[0], R.zero_length_chunk_stream()[0], R.big_chunk_stream()[0]]
    streams.append(streams[0] + streams[2])                             # a repeated identifier between data chunks
    raws = [b"".join(r) for _n, _s, r in frames] + [R.tiny_chunk_stream(1)[1], R.zero_length_chunk_stream()[1], R.big_chunk_stream()[1]]
    unsound = {b for b, (name, _s, _r) in enumerate(frames) if name in ("mutated-chunk", "wrong-crc")}
    a = side_of(streams)
    clean = [K.stream_of(r, 100) for r in raws]                         # the same bytes in the project's own framing, at another grid
    b = side_of(clean)
    reqs = [whole(i, i) for i in range(len(raws))] + [(i, 3, 500, i, 3, 500) for i in range(len(raws))] + [(i, 1, 400, i, 0, 400) for i in range(len(raws))]
    reqs += [(q[0], q[1], q[2], q[0], q[1], q[2]) for q in [(bb, ro & U64, rl & U64) for bb, ro, rl in X.all_windows(streams)][::9]]
    for flags in MODES:
        got = check(cd, a, b, reqs, flags)
        sound = 0
        for r, q in enumerate(reqs):
            if got[0][r] == O.OK and q[0] not in unsound:
                x, y = raws[q[0]][R.clip(len(raws[q[0]]), q[1], q[2])[0]:R.clip(len(raws[q[0]]), q[1], q[2])[1]], F.window_bytes(clean[q[3]], q[4], q[5])
                assert (got[3][r], got[4][r]) == F.truth(x, y, flags), (r, q)
                sound += 1
        assert sound > 60
        same = check(cd, a, a, reqs[:len(raws)], flags)                 # skippable and padding chunks between data chunks: every cut is common
        assert same[5][2] == 0 or flags & E


# ---- 6. the indexes are untrusted ------------------------------------------------------------------------------------------------------------------
def test_unsound_indexes_on_either_side_give_the_models_statuses_and_write_nowhere_else():
    cd = codec()
    streams = list(X.named_streams().values())
    ns = len(streams)
    ix = X.build_index(streams)
    a = F.Side(streams, ix)
    windows = [(b, ro & U64, rl & U64) for b, ro, rl in X.all_windows(streams)]
    reqs = [(b, ro, rl, b, ro, rl) for b, ro, rl in windows[::9]] + [(b, ro, rl, b, (ro + 1) & U64, rl) for b, ro, rl in windows[4::23]] + \
        [(ns, 0, 10, 0, 0, 10), (0, 5, 5, 0xFFFFFFFF, 5, 5)]
    rng = np.random.default_rng(11)
    refused = 0
    check(cd, a, a, reqs, P | S)
    for c, index in enumerate(unsound_indexes(ix, streams, rng)):
        bad = F.Side(streams, index)
        for x, y, flags in ((bad, a, P | S), (a, bad, MODES[c % 4]), (bad, bad, S)):
            got = check(cd, x, y, reqs, flags)                          # (diff_call checks the guard words around outputs and workspace)
            refused += got[0].count(O.ERR_BAD_ARG)
    assert refused > 1000


# ---- 7. corruption ---------------------------------------------------------------------------------------------------------------------------------
def test_corruption_in_a_decoded_span_a_skipped_body_a_header_crc_and_a_crc_collision():
    cd = codec()
    raw = bytes(np.random.default_rng(8).integers(0, 256, 64 * 6, dtype=np.uint8))
    s = K.stream_of(raw, 64)
    rows = R.walk(s)[0]
    ix = X.build_index([s])
    a = F.Side([s], ix)
    other = raw[:130] + bytes([raw[130] ^ 0xFF]) + raw[131:]            # chunk 2 differs: it is the span that is decoded
    t = K.stream_of(other, 64)
    trows = R.walk(t)[0]
    tix = X.build_index([t])
    good = check(cd, a, F.Side([t], tix), [whole(0, 0)], P | S)
    assert good[0] == [O.OK] and (good[3], good[4]) == ([130], [253]) and good[5][2] == 4 * 64
    bad = R.corrupt_chunk(t, trows[2])                                  # ... in a decoded span: the read's status
    got = check(cd, a, F.Side([bad], tix), [whole(0, 0)], P | S)
    assert got[0] == [R.chunk_result(bad, trows[2])[0]] and got[0] != [O.OK] and got[3] == [0]
    got = check(cd, F.Side([bad], tix), a, [whole(0, 0)], P)
    assert got[0] == [R.chunk_result(bad, trows[2])[0]]
    inner = R.corrupt_chunk(s, rows[4])                                 # ... in a body inside a CRC-equal span
    for flags in MODES:
        got = check(cd, a, F.Side([inner], ix), [whole(0, 0)], flags)
        if flags & E:
            assert got[0] == [R.chunk_result(inner, rows[4])[0]] and got[0] != [O.OK]
        else:
            assert got[0] == [O.OK] and got[5][2] == 0 and (got[3], got[4]) == ([384] if flags & P else [0], [384] if flags == S else [0])
    p = ix["pos"][3] + 4                                                # ... in a header CRC: the span is decoded and fails to verify
    flipped = s[:p] + bytes([s[p] ^ 0x10]) + s[p + 1:]
    for flags in MODES:
        got = check(cd, a, F.Side([flipped], ix), [whole(0, 0)], flags)
        assert got[0] == [O.ERR_CRC_MISMATCH]
    twin = collide(raw, 64 * 4 + 9)                                     # the constructed collision of the CPU test
    assert twin != raw and O.crc32c(twin[256:320]) == O.crc32c(raw[256:320])
    tw = side_of([K.stream_of(twin, 64)])
    for flags in MODES:
        got = check(cd, a, tw, [whole(0, 0)], flags)
        assert got[0] == [O.OK]
        if flags & E:
            assert (got[3][0], got[4][0]) == F.truth(raw, twin, flags) and got[3][0] < 384
        else:
            assert got[5][2] == 0 and got[3] == ([384] if flags & P else [0])


# ---- 8. balance ------------------------------------------------------------------------------------------------------------------------------------
def test_one_request_of_70000_rows_beside_70000_requests_of_one_row(html):
    cd = codec()
    n = 70000
    raw = html[3:3 + n]
    data, in_off, in_len = pack_raw([raw])
    a1 = cd.frame_encode_seekable(data, in_off, in_len, chunk_bytes=1)
    b7 = cd.frame_encode_seekable(data, in_off, in_len, chunk_bytes=7)
    assert a1[5].nentries == n and b7[5].nentries == n // 7
    A, Bs = (a1[0], a1[1], a1[2], a1[5]), (b7[0], b7[1], b7[2], b7[5])
    # the model first, on a sample: equal bytes on boundaries decode nothing; a one-byte window owns one row on each side, and side B's is cut
    host = lambda t: t.cpu().numpy().tobytes()
    sa, sb = side_of([host(a1[0])[int(a1[1][0]):int(a1[1][0]) + int(a1[2][0])]]), side_of([host(b7[0])[int(b7[1][0]):int(b7[1][0]) + int(b7[2][0])]])
    sample = [(0, i, 1, 0, i, 1) for i in (0, 1, 6, 7, 500, n - 1)] + [(0, 0, 700, 0, 0, 700)]
    for flags in MODES:
        want = F.diff_plan(sa, sb, sample, flags, 1 << 20, 1 << 20)
        assert want[0] == [O.OK] * 7 and want[5][0] == 6 * 2 + 800 and want[5][2] == 6 * 8 + (1400 if flags & E else 0)
        assert want[3] == ([1] * 6 + [700] if flags & P else [0] * 7)
    ro, rl = dev_u64([0] + list(range(n))), dev_u64([U64] + [1] * n)
    rs = torch.zeros(n + 1, dtype=torch.int32, device="cuda")
    for flags in MODES:
        rows, scratch = n + n // 7 + 2 * n, 8 * n + (2 * n if flags & E else 0)
        pre, suf, la, lb, st, res = cd.frame_diff_indexed(A, Bs, rs, ro, rl, rs, ro, rl, flags, rows, scratch)
        torch.cuda.synchronize()
        assert int((st != 0).sum()) == 0
        assert la.tolist() == [n] + [1] * n and lb.tolist() == la.tolist()
        assert pre.tolist() == ([n] + [1] * n if flags & P else [0] * (n + 1))
        assert suf.tolist() == ([n] + [1] * n if not flags & P else [0] * (n + 1))
        assert res.tolist() == [rows, 2 * n, scratch, n + 1]
        short = cd.frame_diff_indexed(A, Bs, rs, ro, rl, rs, ro, rl, flags, rows, scratch - 1)
        assert short[4].tolist() == [O.OK] * n + [O.ERR_OUTPUT_TOO_SMALL]


# ---- 9. admission ----------------------------------------------------------------------------------------------------------------------------------
def test_each_bound_admits_exactly_the_first_k_requests_and_sizing_fits_exactly(html):
    cd = codec()
    raw = html[:700 * 9]
    other = raw[:3333] + b"\x00" + raw[3334:]
    a, b = side_of([K.stream_of(raw, 500)]), side_of([K.stream_of(other, 700), K.stream_of(raw, 700)])
    reqs = [whole(0, 0), whole(0, 1), (0, 10, 1000, 0, 10, 1000), whole(0, 0), (0, 0, 0, 1, 0, 0), whole(0, 0), (0, 3000, 800, 0, 3000, 900)]
    nreq = len(reqs)
    for flags in MODES:
        rows, scratch = F.needs(a, b, reqs, flags)
        per_rows = [F.diff_plan(a, b, [q], flags, 1 << 20, 1 << 30)[5][0] for q in reqs]
        per_bytes = [F.diff_plan(a, b, [q], flags, 1 << 20, 1 << 30)[5][2] for q in reqs]
        assert sum(per_rows) == rows and sum(per_bytes) == scratch and per_bytes[0] > 0
        # the two sizing rounds, on the device, report the needs that the real call then fits exactly
        assert diff_call(cd, a, b, reqs, flags, 0, 0)[5][0] == rows
        assert diff_call(cd, a, b, reqs, flags, rows, 0)[5][::2] == [rows, scratch]
        full = check(cd, a, b, reqs, flags, rows, scratch)
        assert full[0] == [O.OK] * nreq
        for bounds in ((rows - 1, scratch), (rows, scratch - 1)):       # with need - 1 the last request is refused
            got = check(cd, a, b, reqs, flags, *bounds)
            assert got[0] == [O.OK] * (nreq - 1) + [O.ERR_OUTPUT_TOO_SMALL]
        for k in range(nreq + 1):
            for cap_rows, cap_bytes, per, cap in ((sum(per_rows[:k]), scratch, per_rows, sum(per_rows[:k])), (rows, sum(per_bytes[:k]), per_bytes, sum(per_bytes[:k]))):
                got = check(cd, a, b, reqs, flags, cap_rows, cap_bytes)
                admitted = max(i for i in range(nreq + 1) if sum(per[:i]) <= cap)
                assert got[0] == [O.OK] * admitted + [O.ERR_OUTPUT_TOO_SMALL] * (nreq - admitted)
    # the wrapper sizes the call itself
    ta, tb = side_tensors(a)[0], side_tensors(b)[0]
    ia, ib = SB.FrameIndex(*ta[3:]), SB.FrameIndex(*tb[3:])
    rq = [dev_i32([q[0] for q in reqs]), dev_u64([q[1] for q in reqs]), dev_u64([q[2] for q in reqs]),
          dev_i32([q[3] for q in reqs]), dev_u64([q[4] for q in reqs]), dev_u64([q[5] for q in reqs])]
    pre, suf, la, lb, st, res = cd.frame_diff_indexed((ta[0], ta[1], ta[2], ia), (tb[0], tb[1], tb[2], ib), *rq)
    want = F.diff_plan(a, b, reqs, P | S, *F.needs(a, b, reqs, P | S))
    assert (st.tolist(), la.tolist(), lb.tolist(), pre.tolist(), suf.tolist(), res.tolist()) == tuple(want)


# ---- 10. windows past 2^32 bytes -------------------------------------------------------------------------------------------------------------------
def test_past_4_gib_with_no_large_buffer():
    count = 65537
    k = 12345
    cd = codec()
    zeros = torch.zeros(B, dtype=torch.uint8, device="cuda")
    marked = zeros.clone()
    marked[k] = 1
    ident, chunks = None, []
    for buf in (zeros, marked):
        one = cd.frame_encode_seekable(buf, dev_u64([0]), dev_u64([B]), chunk_bytes=B)
        n1 = int(one[2].item())
        ident, chunk = one[0][:10], one[0][10:n1]
        chunks.append(chunk)
    sides = []
    for last in chunks:
        framed = torch.cat([ident, chunks[0].repeat(count - 1), last])
        in_off, in_len = dev_u64([0]), dev_u64([framed.numel()])
        index = cd.frame_index_buffers(framed, in_off, in_len)
        assert index.total.tolist() == [count * B] and index.tail.tolist() == [O.OK] and index.nentries == count
        sides.append((framed, in_off, in_len, index))
    total = count * B
    assert total - B == 1 << 32
    for exact in (False,):                                              # (EXACT would decode 2 x 4 GiB: the header path is what reaches past 2^32 here)
        pre, suf, la, lb, st = cd.frame_diff_streams(sides[0], sides[1], exact=exact)
        assert st.tolist() == [O.OK] and la.tolist() == [total] and lb.tolist() == [total]
        assert pre.tolist() == [(1 << 32) + k] and suf.tolist() == [B - 1 - k]
    rs = torch.zeros(2, dtype=torch.int32, device="cuda")
    ro, rl = dev_u64([(1 << 32) - 5, 7]), dev_u64([U64, (1 << 32) + 100])
    for flags in (P, S, P | S):
        pre, suf, la, lb, st, res = cd.frame_diff_indexed(sides[0], sides[1], rs, ro, rl, rs, ro, rl, flags)
        assert st.tolist() == [O.OK, O.OK] and la.tolist() == [B + 5, (1 << 32) + 100]
        assert pre.tolist() == ([5 + k, (1 << 32) + 100] if flags & P else [0, 0])
        assert suf.tolist() == ([B - 1 - k, 0 if flags & P else (1 << 32) + 100] if flags & S else [0, 0])
        assert res.tolist()[0] == 2 * (2 + count)


# ---- 11. graph capture -----------------------------------------------------------------------------------------------------------------------------
def test_graph_capture_replays_the_call_on_changed_requests(html):
    cd = codec()
    cb = 4096
    raws = [html[:5 * cb + 9], html[100:100 + 3 * cb]]
    others = [raws[0][:9000] + b"!" + raws[0][9001:], raws[1]]
    a, b = side_of([K.stream_of(r, cb) for r in raws]), side_of([K.stream_of(r, 1000) for r in others])
    lists = [[whole(0, 0), whole(1, 1), (0, cb, cb, 0, cb, cb), (1, cb - 1, 2, 1, cb - 1, 2)], [(1, 7, 2 * cb, 1, 8, 2 * cb), whole(0, 0), (0, 0, 0, 0, 0, 0), (0, 9001, 5, 0, 9001, 5)]]
    nreq = 4
    mr, sc = 256, 1 << 18
    ta, tb = side_tensors(a)[0], side_tensors(b)[0]
    A, Bs = (ta[0], ta[1], ta[2], SB.FrameIndex(*ta[3:])), (tb[0], tb[1], tb[2], SB.FrameIndex(*tb[3:]))
    live = [torch.zeros(nreq, dtype=torch.int32, device="cuda"), dev_u64([0] * nreq), dev_u64([0] * nreq),
            torch.zeros(nreq, dtype=torch.int32, device="cuda"), dev_u64([0] * nreq), dev_u64([0] * nreq)]
    tens = [[dev_i32([q[0] for q in lst]), dev_u64([q[1] for q in lst]), dev_u64([q[2] for q in lst]),
             dev_i32([q[3] for q in lst]), dev_u64([q[4] for q in lst]), dev_u64([q[5] for q in lst])] for lst in lists]
    work = torch.empty(N.frame_diff_lib().snp_frame_diff_indexed_workspace(nreq, mr, sc), dtype=torch.uint8, device="cuda")

    def call():
        return cd.frame_diff_indexed(A, Bs, *live, P | S, mr, sc, work)

    for t, v in zip(live, tens[0]):
        t.copy_(v)
    plain = [x.clone() for x in call()]                                  # one plain call
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        call()                                                          # the same call once before the capture, on the capture's stream
        torch.cuda.synchronize()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        outs = call()
    for k in (0, 1, 0):
        for t, v in zip(live, tens[k]):
            t.copy_(v)
        outs[0].fill_(-1)
        g.replay()
        torch.cuda.synchronize()
        want = F.diff_plan(a, b, lists[k], P | S, mr, sc)
        pre, suf, la, lb, st, res = [x.tolist() for x in outs]
        assert (st, la, lb, pre, suf, res) == tuple(want) and st == [O.OK] * nreq
        if k == 0:
            assert all(torch.equal(x, y) for x, y in zip(plain, outs))

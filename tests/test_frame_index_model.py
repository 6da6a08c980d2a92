"""snp_frame_index_batch / snp_frame_read_indexed_batch (libsnappier_hip_frame_index.so) without a GPU: the declarations and their C# binding, the
workspace arithmetic, argument rejection; the Python model of the contract (frame_index_model.py) against the model of the range call
(frame_range_model.py) on every window of the named streams; admission by each bound, unindexed streams, bad stream numbers, corruption inside
and outside the window, stale rows; and the planning header (csrc/frame_index_device.h) itself, compiled for the CPU under AddressSanitizer
and UBSan into a stand-alone program (tests/abi/frame_index_plan_check.hip) and run over the same windows and over indexes filled with
anything at all."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import decode_layout_model as L
import frame_buffers_model as M
import frame_index_model as X
import frame_range_model as R
import oracle as O
from conftest import ROOT

NAMES = ["snp_frame_index_batch", "snp_frame_index_workspace", "snp_frame_read_indexed_batch", "snp_frame_read_indexed_workspace"]
BIG = 1 << 62


def _lib():
    from snappier_amd import _native as N
    return N.frame_index_lib()


# ---- the surface -----------------------------------------------------------------------------------------------------------------------------
def test_header_and_binding_declare_the_new_functions():
    from snappier_amd import _native as N
    declared = N.frame_index_declared_symbols()
    assert declared == NAMES
    others = set(N.declared_symbols()) | set(N.buffers_declared_symbols()) | set(N.buffers_decompress_declared_symbols()) | \
        set(N.frame_buffers_declared_symbols()) | set(N.layout_declared_symbols()) | set(N.frame_range_declared_symbols())
    assert not set(declared) & others                                  # the other headers' surfaces are left as they are
    lib = _lib()
    assert lib.snp_frame_index_batch.restype is C.c_int and len(lib.snp_frame_index_batch.argtypes) == 14
    assert lib.snp_frame_read_indexed_batch.restype is C.c_int and len(lib.snp_frame_read_indexed_batch.argtypes) == 24
    assert lib.snp_frame_index_workspace.restype is C.c_uint64 and len(lib.snp_frame_index_workspace.argtypes) == 2
    assert lib.snp_frame_read_indexed_workspace.restype is C.c_uint64 and len(lib.snp_frame_read_indexed_workspace.argtypes) == 3


def test_extension_library_exports_exactly_its_header():
    from layouts import exported
    from snappier_amd import _native as N

    ext = exported(N.FRAME_INDEX_PATH)
    assert ext == set(NAMES)
    for other in (N.PRODUCT_PATH, N.BUFFERS_PATH, N.BUFFERS_DECOMPRESS_PATH, N.FRAME_BUFFERS_PATH, N.LAYOUT_PATH, N.FRAME_RANGE_PATH):
        assert not exported(other) & ext


def test_workspace_functions_are_host_arithmetic():
    from snappier_amd import _native as N
    iw, rw = _lib().snp_frame_index_workspace, _lib().snp_frame_read_indexed_workspace
    layout_ws = N.layout_lib().snp_frame_decode_layout_workspace
    assert iw(0, 0) == 0 and iw(0, 5000) == 0                           # nothing when there is no stream
    for ns in (1, 2, 255, 1024, 1025, 300000):
        for sp in (0, 1, 5000):
            w = iw(ns, sp)
            assert w % 256 == 0 and w == layout_ws(ns, sp)              # the span walk, a second per-stream scan and its tile sums: the layout call's pieces
            assert iw(ns + 1, sp) >= w and iw(ns, sp + 1) >= w
    assert iw(0x7FFFFFFF, 0xFFFFFFFF) > 0xFFFFFFFF * 100                # (64-bit arithmetic)
    assert rw(0, 0, 0) == 0 and rw(0, 1000, 1 << 30) == 0               # nothing when there is no request
    for nr in (1, 2, 255, 1024, 1025, 300000):
        for mc in (0, 1, 70000):
            for ec in (0, 1, 65536, 200001, 5 << 30):
                w = rw(nr, mc, ec)
                assert w % 256 == 0
                assert w >= ec + mc * 41 + nr * 2 * 45 + nr * 44        # the scratch, the interior table, the edge slots and rows, the request's words
                assert rw(nr + 1, mc, ec) >= w and rw(nr, mc + 1, ec) >= w and rw(nr, mc, ec + 1) >= w
    assert rw(1, 0, 256) - rw(1, 0, 0) == 256 and rw(1, 0, 257) - rw(1, 0, 0) == 512    # the scratch is a 256-byte piece like the others
    assert rw(0x3FFFFFFF, 0xFFFFFFFF, 1 << 40) > 0xFFFFFFFF * 41 + (1 << 40)            # (64-bit arithmetic)


def test_batch_calls_reject_bad_arguments_without_a_device():
    lib = _lib()
    fake = C.c_void_p(64)                                               # (never dereferenced: the arguments are refused first)
    index, read = lib.snp_frame_index_batch, lib.snp_frame_read_indexed_batch
    assert index(None, None, None, None, 0, 0, 0, *[None] * 7) == O.ERR_BAD_ARG
    assert index(fake, None, None, None, 0, 0, 0, *[None] * 7) == O.ERR_BAD_ARG                                   # no d_result
    assert index(fake, None, None, None, 1, 0, 0, *[None] * 6, fake) == O.ERR_BAD_ARG                             # streams, no arrays
    assert index(fake, fake, fake, fake, 1, 1, 5, fake, None, None, fake, fake, fake, fake) == O.ERR_BAD_ARG      # rows to write, no row arrays
    n3, n5, f3, f5 = [None] * 3, [None] * 5, [fake] * 3, [fake] * 5
    # ctx, in / in_off / in_len, nstreams, the five index arrays, nentries, the three request arrays, nreq, max_chunks, edge_cap, seven more
    assert read(None, *n3, 0, *n5, 0, *n3, 0, 0, 0, *[None] * 7) == O.ERR_BAD_ARG
    assert read(fake, *n3, 0, *n5, 0, *n3, 0, 0, 0, *[None] * 7) == O.ERR_BAD_ARG                                 # no d_result
    assert read(fake, *n3, 0, *n5, 0, *n3, 1, 0, 0, *[None] * 6, fake) == O.ERR_BAD_ARG                           # requests, no arrays
    assert read(fake, *f3, 1, *f5, 8, *f3, 0x40000000, 0, 0, *[fake] * 7) == O.ERR_BAD_ARG                        # nreq >= 2^30
    assert read(fake, *f3, 1, None, *[fake] * 4, 8, *f3, 1, 0, 0, *[fake] * 7) == O.ERR_BAD_ARG                   # streams, no index
    assert read(fake, *f3, 1, fake, None, None, fake, fake, 8, *f3, 1, 0, 0, *[fake] * 7) == O.ERR_BAD_ARG        # rows, no row arrays


def test_csharp_binding_matches_the_extension_header():
    import test_csharp_signatures as T
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "snappier_hip_frame_index.h")).read(), flags=re.S)
    protos = {}
    for m in re.finditer(r"([A-Za-z_][A-Za-z0-9_ ]*?[\s\*]+)(snp_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", text):
        params = [re.match(r"(.*?[\s\*])([A-Za-z_][A-Za-z0-9_]*)$", q.strip()).group(1) for q in m.group(3).split(",") if q.strip() not in ("", "void")]
        protos[m.group(2)] = (T.c_class(m.group(1)), [T.c_class(q) for q in params])
    cs = re.sub(r"//.*", "", open(os.path.join(ROOT, "csharp", "Snappier.Gpu", "NativeMethodsFrameIndex.cs")).read())
    assert 'const string Lib = "snappier_hip_frame_index"' in cs
    imps = {}
    for m in re.finditer(r"\[DllImport\(Lib, CallingConvention = Cc\)\]\s*internal static extern ([A-Za-z\*]+) (snp_[a-z0-9_]+)\(([^)]*)\);", cs):
        params = [re.match(r"(.*?)\s+([A-Za-z_][A-Za-z0-9_]*)$", q.strip()).group(1) for q in m.group(3).split(",") if q.strip()]
        imps[m.group(2)] = (T.cs_class(m.group(1)), [T.cs_class(q) for q in params])
    assert set(protos) == set(imps) == set(NAMES)
    for name, (ret, params) in protos.items():
        cret, cparams = imps[name]
        assert T.compatible(ret, cret), (name, ret, cret)
        assert len(params) == len(cparams) and all(T.compatible(a, b) for a, b in zip(params, cparams)), (name, params, cparams)
    proj = open(os.path.join(ROOT, "csharp", "Snappier.Gpu", "Snappier.Gpu.csproj")).read()
    assert 'Include="../../snappier_amd/libsnappier_hip_frame_index.so"' in proj


# ---- the model -------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def named():
    """(names, streams, the model's index of the batch, every window of every stream as a request)."""
    cases = X.named_streams()
    streams = list(cases.values())
    return list(cases), streams, X.build_index(streams), X.all_windows(streams)


def exact_caps(streams, requests, slack=0):
    out = []
    for r, (b, ro, rl) in enumerate(requests):
        lo, hi = R.clip(R.walk(streams[b])[1], ro, rl)
        out.append(hi - lo + (slack and r % 3))
    return out


def alone(streams, requests, caps):
    """What snp_frame_decode_range_batch gives each request's stream alone, with bounds that admit it: -> (status, out_len, bytes)."""
    ss, wins = [streams[b] for b, _, _ in requests], [(ro, rl) for _, ro, rl in requests]
    mc, sp, ec = R.needs(ss, wins, caps)
    return R.range_plan(ss, wins, caps, mc, sp, ec)[:3]


def test_the_index_lists_the_rows_of_the_walk(named):
    names, streams, ix, _ = named
    assert len(streams) == 28
    for b, s in enumerate(streams):
        rows, total, tail, _ = R.walk(s)
        tail_l, total_l, nchunks = L.stream_item(s)
        f0, f1 = ix["first"][b], ix["first"][b + 1]
        assert f1 - f0 == len(rows) == nchunks and ix["total"][b] == total == total_l and ix["tail"][b] == tail == tail_l, names[b]
        start, pos = ix["start"][f0:f1], ix["pos"][f0:f1]
        assert start == sorted(start) and start == [r[4] for r in rows]
        for p, r in zip(pos, rows):                                     # the position names the chunk's 4-byte header, inside the stream
            h = M.hop(s, p)
            assert h.kind == "data" and (h.type, p + 8, h.body_len, h.crc, h.dec) == r[:4] + (r[5],)
    assert ix["result"] == [len(ix["start"]), sum(R.walk(s)[1] for s in streams), sum((len(s) + R.SPAN - 1) // R.SPAN for s in streams), 1]
    assert any(r[5] == 0 for s in streams for r in R.walk(s)[0])          # zero-length chunks have rows too


def test_every_window_reads_what_the_range_call_gives_for_the_stream_alone(named):
    names, streams, ix, requests = named
    assert len(requests) == 802
    for caps in (exact_caps(streams, requests, slack=1), [BIG] * len(requests)):
        mc, ec = X.read_needs(streams, ix, requests, caps)
        got = X.read_plan(streams, ix, requests, caps, mc, ec)
        want = alone(streams, requests, caps)
        for r, (b, ro, rl) in enumerate(requests):
            assert (got[0][r], got[1][r], got[2][r]) == (want[0][r], want[1][r], want[2][r]), (names[b], ro, rl)
        assert got[3] == [mc, sum(want[1]), ec, sum(1 for s in want[0] if s == O.OK)]
        assert {O.OK, O.ERR_TRUNCATED_STREAM, O.ERR_CHUNK_TYPE, O.ERR_BAD_LENGTH, O.ERR_INCOMPLETE, O.ERR_CRC_MISMATCH} <= set(got[0])
        assert X.read_plan(streams, ix, requests, caps, mc + 300, ec + 1000)[:3] == got[:3]       # looser bounds change nothing
    # the searches select the chunks the range call's rule selects, everywhere; a zero-length row falls inside a slot range now and then
    empties = 0
    for b, ro, rl in requests:
        s = streams[b]
        rows, total, _, _ = R.walk(s)
        k, head, tail, cnt, _ = X.planned(ix, streams, b, ro, rl, BIG)
        sel, edges = R.select(rows, *R.clip(total, ro, rl))
        mine = ([head] if head else []) + X.interior_rows(ix, s, k) + ([tail] if tail else [])
        assert [x for x in mine if x[5] > 0] == sel and [x for x in (head, tail) if x] == edges
        empties += any(x[5] == 0 for x in mine)
    assert empties == 19                                                # (of the 802)
    # a window that does not fit its capacity decodes nothing and takes nothing
    tight = [max(c - 1, 0) for c in exact_caps(streams, requests)]
    got = X.read_plan(streams, ix, requests, tight, *X.read_needs(streams, ix, requests, tight))
    assert got[:3] == alone(streams, requests, tight)


def test_requests_are_independent_of_their_order_and_may_repeat(named):
    _, streams, ix, requests = named
    caps = exact_caps(streams, requests)
    rng = np.random.default_rng(5)
    order = rng.permutation(len(requests))[:200].tolist()
    order += order[:20]                                                 # duplicates
    reqs, cps = [requests[i] for i in order], [caps[i] for i in order]
    mc, ec = X.read_needs(streams, ix, reqs, cps)
    got = X.read_plan(streams, ix, reqs, cps, mc, ec)
    assert got[:3] == alone(streams, reqs, cps)


def test_index_admission_is_in_stream_order_by_each_bound():
    a, b, c = R.uniform_stream(3, 1)[0], R.tiny_chunk_stream(3)[0], R.uniform_stream(2, 2, 500)[0]
    long_s = R.long_stream_with_a_skippable_chunk_across_the_span_boundary()[0]
    streams = [a, b, b"", long_s, c, a, R.ID]
    full = X.build_index(streams)
    rows = [len(R.walk(s)[0]) for s in streams]
    need, spans = sum(rows), 7
    assert full["result"] == [need, sum(R.walk(s)[1] for s in streams), spans, 1] and full["first"][-1] == need
    assert X.build_index(streams, spans, need) == full and X.build_index(streams, spans + 9, need + 9) == full

    def first_rejected(ix):
        f = next(i for i, t in enumerate(ix["tail"]) if t == O.ERR_OUTPUT_TOO_SMALL)
        n = len(streams)
        assert ix["tail"][f:] == [O.ERR_OUTPUT_TOO_SMALL] * (n - f) and ix["total"][f:] == [0] * (n - f)
        assert ix["first"][f:] == [ix["first"][f]] * (n + 1 - f)                                   # no rows
        assert ix["first"][:f + 1] == full["first"][:f + 1] and ix["tail"][:f] == full["tail"][:f] and ix["total"][:f] == full["total"][:f]
        assert ix["start"] == full["start"][:ix["first"][f]] and ix["pos"] == full["pos"][:ix["first"][f]]
        return f

    short = X.build_index(streams, spans, need - 1)
    assert first_rejected(short) == 5 and short["result"][0] == need                               # the last stream with a row
    short = X.build_index(streams, spans - 1, need)
    assert first_rejected(short) == 6 and short["result"][0] == need and short["result"][2] == spans   # the last stream with a span (it has no chunk)
    short = X.build_index(streams, spans - 2, need)
    assert first_rejected(short) == 5 and short["result"][0] == need - rows[5]                     # not walked: its rows are not counted
    sizing = X.build_index(streams, spans, 0)
    assert sizing["result"] == full["result"][:1] + [0] + full["result"][2:] and first_rejected(sizing) == 0
    assert X.build_index([b"", b""], 0, 0)["tail"] == [O.OK, O.OK]                                 # empty streams need neither
    assert X.build_index([], 0, 0)["result"] == [0] * 4


def test_read_admission_is_in_request_order_by_each_bound():
    a, b, c = R.uniform_stream(3, 1)[0], R.tiny_chunk_stream(3)[0], R.uniform_stream(2, 2, 500)[0]
    streams = [a, b, c]
    ix = X.build_index(streams)
    B = R.B
    requests = [(0, 10, 2 * B), (1, 0, R.U64), (2, B - 1, 2), (0, 0, 3 * B), (1, 5, 0), (2, 7, 10), (0, 0, 0)]
    caps = [BIG] * len(requests)
    mc, ec = X.read_needs(streams, ix, requests, caps)
    full = X.read_plan(streams, ix, requests, caps, mc, ec)
    assert full[0] == [O.OK] * len(requests) and full[3] == [mc, sum(full[1]), ec, len(requests)]
    assert full[:3] == alone(streams, requests, caps)

    def first_rejected(plan):
        st = plan[0]
        f = next(i for i, x in enumerate(st) if x == O.ERR_OUTPUT_TOO_SMALL)
        assert st[f:] == [O.ERR_OUTPUT_TOO_SMALL] * (len(st) - f) and plan[1][f:] == [0] * (len(st) - f)
        assert st[:f] == full[0][:f] and plan[2][:f] == full[2][:f]     # earlier requests are what they were
        assert plan[3][0] == mc and plan[3][2] == ec                    # what the call needs is reported whatever it was given
        return f

    assert first_rejected(X.read_plan(streams, ix, requests, caps, mc - 1, ec)) == 3               # the last request with an interior slot
    assert first_rejected(X.read_plan(streams, ix, requests, caps, mc, ec - 1)) == 5               # the last request with an edge
    assert first_rejected(X.read_plan(streams, ix, requests, caps, 0, 0)) == 0                     # the sizing call
    # a request that needs nothing is admitted by a sizing call
    assert X.read_plan(streams, ix, [(0, 0, 0), (1, 0, 5)], [0, 5], 0, 0)[0] == [O.OK, O.ERR_OUTPUT_TOO_SMALL]
    assert X.read_plan(streams, ix, [], [], 0, 0)[3] == [0] * 4


def test_an_unindexed_stream_and_a_bad_stream_number():
    a, b = R.uniform_stream(3, 1)[0], R.tiny_chunk_stream(3)[0]
    streams = [a, b, a]
    ix = X.build_index(streams, max_entries=len(R.walk(a)[0]) + len(R.walk(b)[0]))                 # the third stream is not indexed
    assert ix["tail"][2] == O.ERR_OUTPUT_TOO_SMALL
    requests = [(0, 5, 100), (2, 5, 100), (3, 5, 100), (0xFFFFFFFF, 0, 0), (1, 0, 50), (2, 0, 0)]
    caps = [BIG] * len(requests)
    got = X.read_plan(streams, ix, requests, caps, *X.read_needs(streams, ix, requests, caps))
    assert got[0] == [O.OK, O.ERR_OUTPUT_TOO_SMALL, O.ERR_BAD_ARG, O.ERR_BAD_ARG, O.OK, O.ERR_OUTPUT_TOO_SMALL]
    assert got[1] == [100, 0, 0, 0, 50, 0] and got[3][3] == 2


def test_a_corrupt_chunk_is_noticed_iff_the_request_meets_it():
    for s in (R.uniform_stream(4, 5)[0], R.tiny_chunk_stream(2)[0], R.big_chunk_stream()[0]):
        rows, total, tail, _ = R.walk(s)
        full = [r for r in rows if r[5] > 0]
        victim = full[len(full) // 2]
        bad = R.corrupt_chunk(s, victim)
        ix = X.build_index([bad])
        assert ix == X.build_index([s])                                 # the header walk does not see it
        requests = [(0, ro, rl) for ro, rl in R.windows(rows, total)]
        caps = [BIG] * len(requests)
        got = X.read_plan([bad], ix, requests, caps, *X.read_needs([bad], ix, requests, caps))
        assert got[:3] == alone([bad], requests, caps)
        want = M.chunk_status(bad, victim)
        hit = [victim in R.select(rows, *R.clip(total, ro, rl))[0] for _, ro, rl in requests]
        assert [st != O.OK for st in got[0]] == hit and all(st == want for st, h in zip(got[0], hit) if h)
        assert sum(hit) > 3 and len(hit) - sum(hit) > 3


def test_a_stale_index_gives_bad_arg_per_request():
    B = R.B
    s = R.uniform_stream(5, last=777)[0]
    other = R.uniform_stream(5, 3, 777)[0]
    rows = R.walk(s)[0]
    ix = X.build_index([s])
    requests = [(0, 10, 100), (0, B + 5, 2 * B), (0, B, 2 * B), (0, 3 * B - 1, 2), (0, 0, R.U64), (0, 4 * B + 1, 10), (0, 2 * B, 0)]
    caps = [BIG] * len(requests)

    def read(streams, index):
        return X.read_plan(streams, index, requests, caps, *X.read_needs(streams, index, requests, caps))

    good = read([s], ix)
    assert good[0] == [O.OK] * len(requests)
    total = R.walk(s)[1]
    uses = [[rows.index(x) for x in R.select(rows, *R.clip(total, ro, rl))[0]] for _, ro, rl in requests]     # the rows each request meets

    def stale(index, row, streams=None):
        got = read(streams or [s], index)
        for r, st in enumerate(got[0]):
            touched = row in uses[r]
            assert st == (O.ERR_BAD_ARG if touched else O.OK) and (got[2][r] is None) == touched, (row, r)
            if not touched:
                assert got[2][r] == good[2][r]
        return got

    # a wrong position: the header of another chunk (its size differs), bytes inside a payload, a position beyond the stream
    for pos in (ix["pos"][4], ix["pos"][2] + 9, len(s) + 5, len(s) - 2):
        stale({**ix, "pos": ix["pos"][:2] + [pos] + ix["pos"][3:]}, 2)
    # a wrong size: the row's start moved by one (the row before it and the row itself no longer match their headers)
    moved = {**ix, "start": ix["start"][:2] + [ix["start"][2] + 1] + ix["start"][3:]}
    got = read([s], moved)
    assert [st for st in got[0]] == [O.OK, O.ERR_BAD_ARG, O.ERR_BAD_ARG, O.ERR_BAD_ARG, O.ERR_BAD_ARG, O.OK, O.ERR_BAD_ARG]
    # not a data chunk: the position of the stream identifier
    stale({**ix, "pos": [0] + ix["pos"][1:]}, 0)
    # the stream changed under the index: the size field of a raw chunk's header altered (it now declares another size than its row)
    assert rows[2][0] == 1
    p = ix["pos"][2]
    stale(ix, 2, [s[:p + 1] + bytes([s[p + 1] ^ 1]) + s[p + 2:]])
    # another stream at the same place: its chunks have other sizes, so other positions (only chunk 0 is where the index says)
    assert [r[1] for r in R.walk(other)[0]][1:] != [r[1] for r in rows][1:]
    got = read([other], ix)
    assert got[0][0] == O.OK and got[2][0] == R.uniform_stream(5, 3, 777)[1][10:110] and set(got[0][1:6]) == {O.ERR_BAD_ARG}
    # a start moved before the window: the row no longer decodes to end - start bytes
    shifted = {**ix, "start": [0, B - 1] + ix["start"][2:]}
    assert read([s], shifted)[0][2] == O.ERR_BAD_ARG
    # first beyond the arrays, a total that no row reaches, a tail that is no status
    assert set(read([s], {**ix, "first": [0, 1 << 40]})[0]) == {O.OK}   # clamped to the rows there are
    assert set(read([s], {**ix, "first": [3, 1]})[0]) == {O.ERR_BAD_ARG}
    assert read([s], {**ix, "total": [1 << 40]})[0][4:6] == [O.ERR_BAD_ARG, O.ERR_BAD_ARG]
    assert set(read([s], {**ix, "tail": [77]})[0]) == {O.ERR_BAD_ARG}
    assert set(read([s], {**ix, "start": [], "pos": []})[0]) == {O.ERR_BAD_ARG, O.OK}


# ---- the planning header on the CPU, under sanitizers ------------------------------------------------------------------------------------------
def test_planning_header_under_sanitizers_matches_the_model(named, tmp_path):
    names, streams, ix, requests = named
    ns = len(streams)
    rng = np.random.default_rng(11)
    ne = len(ix["start"])
    caps = exact_caps(streams, requests, slack=1)
    sound = [(b, ro & R.U64, rl & R.U64, c) for (b, ro, rl), c in zip(requests, caps)]      # (as 64-bit words)
    some = sound[::3] + [(ns, 0, 10, 10), (0xFFFFFFFF, 5, 5, 5)]

    def rnd(n, hi=1 << 64):
        return [int(v) % hi for v in rng.integers(0, 1 << 63, n, dtype=np.uint64) * 2 + rng.integers(0, 2, n, dtype=np.uint64)]

    lens = [len(s) for s in streams]
    cases = [(ix, sound + [(ns, 0, 10, 10)]),                                                  # the 802 windows over the sound index
             ({**ix, "start": rnd(ne), "pos": rnd(ne)}, some),                                 # rows filled with random u64
             ({**ix, "first": rnd(ns + 1), "total": rnd(ns), "start": rnd(ne), "pos": rnd(ne)}, some),
             ({**ix, "start": rnd(ne, 1 << 17), "pos": rnd(ne, 1 << 12), "total": rnd(ns, 1 << 18)}, some),   # small random values: searches go everywhere
             ({**ix, "first": [f + (1 << 33) * (i % 2) for i, f in enumerate(ix["first"])]}, some),        # idx_first beyond nentries
             ({**ix, "first": list(reversed(ix["first"]))}, some),
             ({**ix, "pos": [p + lens[i % ns] for i, p in enumerate(ix["pos"])]}, some),       # positions beyond in_len
             ({**ix, "pos": [max(lens) - 1 - (i % 20) for i in range(ne)]}, some),             # ... and within a few bytes of a stream's end
             ({**ix, "start": list(reversed(ix["start"]))}, some),                             # non-monotone starts
             ({**ix, "start": [v ^ ((i % 3 == 0) << 9) for i, v in enumerate(ix["start"])]}, some),
             ({**ix, "tail": [int(v) % 40 - 20 for v in rng.integers(0, 1000, ns)]}, some),    # tails that are no status
             ({**ix, "start": ix["start"][:ne // 2], "pos": ix["pos"][:ne // 2]}, some),       # fewer rows than idx_first says
             ({**ix, "start": [], "pos": []}, some)]
    path = str(tmp_path / "cases.bin")
    X.write_cases(path, streams, cases)
    exe = str(tmp_path / "frame_index_plan_check")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host",
                    "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "abi", "frame_index_plan_check.hip"), "-o", exe,
                    "-Wl,-rpath,/opt/rocm/lib"], check=True)
    env = {**os.environ, "ASAN_OPTIONS": "detect_leaks=1:abort_on_error=0", "UBSAN_OPTIONS": "print_stacktrace=1:halt_on_error=1"}
    run = subprocess.run([exe, path], capture_output=True, text=True, env=env)
    assert run.returncode == 0 and run.stderr == "", run.stderr[-3000:]      # the sanitizers are silent
    lines = run.stdout.splitlines()
    assert len(lines) == sum(len(reqs) for _, reqs in cases)
    at = refused = planned = 0
    for c, (index, reqs) in enumerate(cases):
        for b, ro, rl, cap in reqs:
            want = X.plan_line(index, streams, (b, ro, rl), cap)
            assert lines[at] == want, (c, names[b] if b < ns else b, ro, rl, cap)
            refused += c > 0 and (want.startswith("%d " % O.ERR_BAD_ARG) or not want.endswith(" 0"))
            planned += c > 0 and want.startswith("0 ") and want.endswith(" 0")
            at += 1
    assert refused > 500 and planned > 100                            # both outcomes, on the unsound indexes
    # over the sound index the plans are the selection of the range call (the model's, checked above), with no row refused
    assert all(line.endswith(" 0") and not line.startswith("%d " % O.ERR_BAD_ARG) for line in lines[:len(sound)])

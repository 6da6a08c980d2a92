"""snp_frame_recut_indexed_batch (libsnappier_hip_frame_recut.so) without a GPU: the declarations and their C# binding, the workspace arithmetic,
argument rejection; the Python model of the contract (frame_recut_model.py) checked against the rechunk model (guarantee (a): a grid list is the
rechunk, array for array), the model of the encoder at given cuts (guarantees (b) and (c)), the oracle's frame decode and the index model:
directed lists, every rejection of a list, unsound indexes, admission by each bound and out_cap, the end-to-end property on content-defined
streams after edits; and the planning header (csrc/frame_recut_device.h) itself, compiled for the CPU under AddressSanitizer and UBSan into a
stand-alone program (tests/abi/frame_recut_plan_check.hip) and run over the same cases, over indexes and lists filled with anything at all and
over streams and cuts past 4 GiB given as numbers."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import frame_buffers_model as M
import frame_chunked_model as K
import frame_cuts_model as CM
import frame_index_model as X
import frame_range_model as R
import frame_rechunk_model as RC
import frame_recut_model as RX
import oracle as O
from conftest import ROOT, read_testdata
from test_frame_rechunk_model import fragmented

NAMES = ["snp_frame_recut_indexed_batch", "snp_frame_recut_indexed_workspace"]
ALL = RX.REWRITE_ALL


def _lib():
    from snappier_amd import _native as N
    return N.frame_recut_lib()


# ---- the surface -----------------------------------------------------------------------------------------------------------------------------
def test_header_and_binding_declare_the_new_functions():
    from snappier_amd import _native as N
    declared = N.frame_recut_declared_symbols()
    assert sorted(declared) == NAMES
    others = set()
    for name in dir(N):
        if name.endswith("declared_symbols") and name not in ("frame_recut_declared_symbols",):
            others |= set(getattr(N, name)())
    assert len(others) > 40 and not set(declared) & others             # the other headers' surfaces are left as they are
    lib = _lib()
    assert lib.snp_frame_recut_indexed_batch.restype is C.c_int and len(lib.snp_frame_recut_indexed_batch.argtypes) == 31
    assert lib.snp_frame_recut_indexed_workspace.restype is C.c_uint64 and len(lib.snp_frame_recut_indexed_workspace.argtypes) == 4
    header = open(os.path.join(ROOT, "include", "snappier_hip_frame_recut.h")).read()
    assert re.search(r"#define SNP_RECUT_REWRITE_ALL 1u\b", header) and N.RECUT_REWRITE_ALL == ALL == 1
    import snappier_amd
    from snappier_amd import batch as SB
    assert snappier_amd.RECUT_REWRITE_ALL == 1
    assert callable(SB.BlockCodec.frame_recut_indexed) and callable(SB.BlockCodec.frame_recut_to_memory)
    assert callable(SB.BlockCodec.frame_recut_content_defined)


def test_extension_library_exports_exactly_its_header():
    from layouts import exported
    from snappier_amd import _native as N

    ext = exported(N.FRAME_RECUT_PATH)
    assert ext == set(NAMES)
    for other in (N.PRODUCT_PATH, N.FRAME_RECHUNK_PATH, N.FRAME_CUTS_PATH, N.FRAME_DEDUP_PATH, N.FRAME_COMPOSE_PATH, N.FRAME_EDIT_PATH):
        assert not exported(other) & ext


def test_workspace_is_host_arithmetic():
    ws = _lib().snp_frame_recut_indexed_workspace
    assert ws(0, 10, 1000, 50) == 0                                     # nothing when there is no stream
    for ns in (1, 255, 1025, 300000):
        for ms in (0, 1, 33000):
            for sc in (0, 1, 70000, 1 << 33):
                for me in (0, 7, 100000):
                    w = ws(ns, ms, sc, me)
                    assert w % 256 == 0
                    # ONE staging and the 64 bytes an empty slot may touch; the slot table (32), the decode table (41) with where a row starts and
                    # the pieces before it (16) and the two scans (16); the streams' words (15 + 7 of 8 bytes, 1 of 4); the new rows' (8 + 4 + 8)
                    assert w >= sc + ms * (64 + 105) + ns * 180 + me * 20
                    assert w <= sc + 512 + ms * (64 + 105) + ns * 180 + me * 20 + 64 * 256 + (ns + ms + me) // 50
                    assert ws(ns + 1, ms, sc, me) >= w and ws(ns, ms + 1, sc, me) >= w and ws(ns, ms, sc + 16, me) >= w and ws(ns, ms, sc, me + 1) >= w
    assert ws(0x7FFFFFFF, 0xFFFFFFFF, 1 << 40, 0xFFFFFFFF) > 0xFFFFFFFF * 64 + (1 << 40)       # (64-bit arithmetic)
    # the workspace does not grow with the largest piece: it is the caller's budget, not slots * 76 512
    assert ws(1, 1000, 1 << 20, 1000) < (1 << 20) + 1000 * 300 + 64 * 256


def test_batch_call_rejects_bad_arguments_without_a_device():
    call = _lib().snp_frame_recut_indexed_batch
    fake = C.c_void_p(64)                                               # (never dereferenced: the arguments are refused first)
    # ctx; in, in_off, in_len; nstreams; five index arrays; nentries; cut_first, cuts, ncuts; flags, max_slots, stage_cap, max_entries;
    # out, out_off, out_cap, out_len, status; five new index arrays; out_bound; d_work, d_result
    def args(ctx=fake, ins=(fake,) * 3, ns=1, idx=(fake,) * 5, ne=8, cf=fake, cuts=fake, nc=4, flags=0, ms=0, sc=0, me=8, outs=(fake,) * 5,
             new=(fake,) * 5, bound=None, work=fake, result=fake):
        return (ctx, *ins, ns, *idx, ne, cf, cuts, nc, flags, ms, sc, me, *outs, *new, bound, work, result)

    assert call(*args(ctx=None)) == O.ERR_BAD_ARG
    assert call(*args(result=None)) == O.ERR_BAD_ARG
    assert call(*args(ns=0, result=None)) == O.ERR_BAD_ARG             # an empty call still needs d_result
    assert call(*args(flags=2)) == O.ERR_BAD_ARG and call(*args(flags=3)) == O.ERR_BAD_ARG and call(*args(flags=1 << 31)) == O.ERR_BAD_ARG
    assert call(*args(ns=0, flags=2)) == O.ERR_BAD_ARG                 # ... also when there is no stream
    assert call(*args(ns=1 << 31)) == O.ERR_BAD_ARG
    assert call(*args(work=None)) == O.ERR_BAD_ARG
    assert call(*args(cf=None)) == O.ERR_BAD_ARG and call(*args(cf=None, nc=0)) == O.ERR_BAD_ARG      # cut_first: always
    assert call(*args(cuts=None)) == O.ERR_BAD_ARG                      # cuts: when there is one
    for group, n in (("ins", 3), ("outs", 5)):
        for i in range(n):
            a = [fake] * n
            a[i] = None
            assert call(*args(**{group: tuple(a)})) == O.ERR_BAD_ARG, (group, i)
    for i in (0, 3, 4):                                                 # idx_first, idx_total, idx_tail; new_first, new_total, new_tail
        a = [fake] * 5
        a[i] = None
        assert call(*args(idx=tuple(a))) == O.ERR_BAD_ARG, i
        assert call(*args(new=tuple(a))) == O.ERR_BAD_ARG, i
    for i in (1, 2):                                                    # rows, no row arrays
        a = [fake] * 5
        a[i] = None
        assert call(*args(idx=tuple(a))) == O.ERR_BAD_ARG and call(*args(new=tuple(a))) == O.ERR_BAD_ARG
        assert call(*args(new=tuple(a), ne=0, me=1)) == O.ERR_BAD_ARG   # no old rows, room for new ones


def test_csharp_binding_matches_the_extension_header():
    import test_csharp_signatures as T
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "snappier_hip_frame_recut.h")).read(), flags=re.S)
    protos = {}
    for m in re.finditer(r"([A-Za-z_][A-Za-z0-9_ ]*?[\s\*]+)(snp_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", text):
        params = [re.match(r"(.*?[\s\*])([A-Za-z_][A-Za-z0-9_]*)$", q.strip()).group(1) for q in m.group(3).split(",") if q.strip() not in ("", "void")]
        protos[m.group(2)] = (T.c_class(m.group(1)), [T.c_class(q) for q in params])
    cs = re.sub(r"//.*", "", open(os.path.join(ROOT, "csharp", "Snappier.Gpu", "NativeMethodsFrameRecut.cs")).read())
    assert 'const string Lib = "snappier_hip_frame_recut"' in cs and "const uint RewriteAll = 1;" in cs
    imps = {}
    for m in re.finditer(r"\[DllImport\(Lib, CallingConvention = Cc\)\]\s*internal static extern ([A-Za-z\*]+) (snp_[a-z0-9_]+)\(([^)]*)\);", cs):
        params = [re.match(r"(.*?)\s+([A-Za-z_][A-Za-z0-9_]*)$", q.strip()).group(1) for q in m.group(3).split(",") if q.strip()]
        imps[m.group(2)] = (T.cs_class(m.group(1)), [T.cs_class(q) for q in params])
    assert set(protos) == set(imps) == set(NAMES)
    for name, (ret, params) in protos.items():
        cret, cparams = imps[name]
        assert T.compatible(ret, cret), (name, ret, cret)
        assert len(params) == len(cparams) and all(T.compatible(a, b) for a, b in zip(params, cparams)), (name, params, cparams)
    assert len(protos["snp_frame_recut_indexed_batch"][1]) == 31 and len(protos["snp_frame_recut_indexed_workspace"][1]) == 4
    proj = open(os.path.join(ROOT, "csharp", "Snappier.Gpu", "Snappier.Gpu.csproj")).read()
    assert 'Include="../../snappier_amd/libsnappier_hip_frame_recut.so"' in proj


# ---- guarantee (a): a grid list is the rechunk -----------------------------------------------------------------------------------------------------
def same_as_rechunk(got, want):
    assert got["status"] == want["status"] and got["out_len"] == want["out_len"] and got["streams"] == want["streams"]
    assert RX.same_index(got["index"], want["index"]) and got["out_bound"] == want["out_bound"] and got["alone"] == want["alone"]
    assert [got["result"][i] for i in (0, 1, 3, 4, 5)] == [want["result"][i] for i in (0, 1, 3, 4, 5)]


@pytest.mark.parametrize("cb", RC.CHUNK_SIZES)
def test_a_grid_list_gives_what_the_rechunk_gives(cb):
    html = read_testdata("html") * 5
    for variant in (O.HASH_CRC32C, O.HASH_MUL):
        names, raws, streams = fragmented(html, cb, variant)
        streams = streams + [K.stream_of(raws[0], cb, variant), M.STREAM_ID, b""]
        raws = raws + [raws[0], b"", b""]
        ix = X.build_index(streams)
        first, cuts = CM.regular_cuts([len(a) for a in raws], cb)
        for flags in (0, ALL):
            got = RX.recut_plan(streams, ix, first, cuts, flags, variant=variant)
            same_as_rechunk(got, RC.rechunk_plan(streams, ix, cb, flags, variant=variant))
            assert got["result"][6] + got["result"][7] == sum(len(x["start"]) for x in [X.build_index([s]) for s in got["streams"] if s is not None])
            assert got["result"][2] >= got["result"][7] * 64 and (flags == 0 or got["result"][6] == 0)
        # (b) and (c): the encoder's output at the same list
        want = CM.encode_at_cuts(raws, first, cuts, variant)["streams"]
        assert RX.after(streams, RX.recut_plan(streams, ix, first, cuts, variant=variant)) == want
        assert RX.recut_plan(streams, ix, first, cuts, ALL, variant=variant)["streams"] == want
        # ... and at another grid and at the content's own cuts, at once
        for first2, cuts2 in (CM.regular_cuts([len(a) for a in raws], min(cb + 1, 65536)), RX.content_lists(raws, 32, min(max(cb, 33), 4096))):
            enc = CM.encode_at_cuts(raws, first2, cuts2, variant)
            got = RX.recut_plan(streams, ix, first2, cuts2, variant=variant)
            assert got["status"] == [O.OK] * len(streams) and RX.after(streams, got) == enc["streams"]
            new_ix = X.build_index(RX.after(streams, got))
            assert RX.same_index(got["index"], new_ix)
            assert RX.same_index(got["index"], {k: enc[k] for k in ("first", "start", "pos", "total", "tail")})    # index arrays included


# ---- directed lists ------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def directed():
    cases = RX.directed(read_testdata("html"))
    names = list(cases)
    streams, raws = [cases[n][0] for n in names], [cases[n][1] for n in names]
    first, cuts = RX.lists([cases[n][2] for n in names])
    assert all(O.frame_decode(s) == a for s, a in zip(streams, raws) if s)
    return names, streams, raws, first, cuts, X.build_index(streams)


def test_directed_lists(directed):
    names, streams, raws, first, cuts, ix = directed
    want = CM.encode_at_cuts(raws, first, cuts)
    assert want["status"] == [O.OK] * len(names)
    got = RX.recut_plan(streams, ix, first, cuts)
    assert got["status"] == [O.OK] * len(names)
    assert RX.after(streams, got) == want["streams"]                                    # (c): every chunk here is the oracle's
    assert RX.same_index(got["index"], X.build_index(RX.after(streams, got)))
    assert [n for n, x in zip(names, got["alone"]) if x] == ["empty_in_len_10", "canonical_already"]
    plans = dict(zip(names, got["plans"]))
    shape = {n: (k["dirty"], k["rebuilt"], k["copied"]) for n, k in plans.items()}
    assert shape["dirty_row_spans_pieces"] == (1, 4, 1)                 # the row [0, 3000) is four pieces; [3000, 4000) is one already
    assert shape["dirty_rows_make_one_piece"] == (3, 1, 2)              # three rows make [0, 1900); [1900, 2600) and [2600, 4000) are kept
    assert shape["clean_between_dirty"] == (4, 4, 1)
    assert shape["start_matches_end_does_not"] == (2, 2, 3) and shape["end_matches_start_does_not"] == (2, 2, 3)
    assert shape["one_byte_pieces"] == (3, 7, 2)
    assert shape["a_full_size_piece"] == (2, 1, 2) and shape["a_full_size_piece_kept"] == (2, 1, 2)
    assert shape["short_last_piece_kept"] == (4, 2, 1)
    assert shape["zero_length_rows"] == (6, 2, 3)                       # the four zero-length rows are dirty and vanish
    assert shape["skippable_and_padding_dropped"] == (0, 0, 5) and shape["one_piece"] == (5, 1, 0)
    assert shape["empty_in_len_0"] == (0, 0, 0) and shape["only_zero_length_rows"] == (2, 0, 0)
    assert got["streams"][names.index("empty_in_len_0")] == M.STREAM_ID == got["streams"][names.index("only_zero_length_rows")]
    big = names.index("a_full_size_piece_kept")
    assert 65536 in RC.data_chunk_lengths(got["streams"][big]) and 1 in RC.data_chunk_lengths(got["streams"][big])
    k = names.index("skippable_and_padding_dropped")
    assert got["out_len"][k] == got["out_bound"][k] and got["result"][6] == sum(v[2] for n, v in shape.items() if plans[n]["work"])
    # the flag: every stream written, nothing copied, the same bytes
    every = RX.recut_plan(streams, ix, first, cuts, ALL)
    assert every["streams"] == want["streams"] and every["result"][5] == 0 and every["result"][6] == 0
    assert every["result"][7] == sum(len(CM.list_verdict(len(a), first[b], first[b + 1], cuts)[1]) for b, a in enumerate(raws))
    # the sizing call and the exact bounds
    ms, sc, me = RX.needs(streams, ix, first, cuts)
    assert (ms, sc, me) == (got["result"][0], got["result"][2], got["result"][4])
    assert RX.recut_plan(streams, ix, first, cuts, max_slots=ms, stage_cap=sc, max_entries=me) == got
    assert sc == sum(k["dbytes"] + k["cbytes"] for k in got["plans"]) <= sum(RX.stage_bound(k["dbytes"], k["rebuilt"]) for k in got["plans"])


def test_foreign_streams_with_and_without_rewrite_all():
    html = read_testdata("html")
    cases = RC.foreign_streams(html)
    streams, raws = [c[0] for c in cases.values()], [c[1] for c in cases.values()]
    ix = X.build_index(streams)
    for first, cuts in (RX.content_lists(raws, 32, 256), CM.regular_cuts([len(a) for a in raws], 500), RX.lists([[1000, 1700, 3000][:max(0, len(a) // 1000)] for a in raws])):
        enc = CM.encode_at_cuts(raws, first, cuts)
        assert enc["status"] == [O.OK] * len(streams)
        every = RX.recut_plan(streams, ix, first, cuts, ALL)
        assert every["status"] == [O.OK] * len(streams) and every["streams"] == enc["streams"]                           # (b)
        assert RX.same_index(every["index"], {k: enc[k] for k in ("first", "start", "pos", "total", "tail")})
        got = RX.recut_plan(streams, ix, first, cuts)
        assert got["status"] == [O.OK] * len(streams)
        for name, new, a, b in zip(cases, RX.after(streams, got), raws, range(len(raws))):                               # (d)
            assert O.frame_decode(new) == a, name
            nix = X.build_index([new])
            assert nix["tail"] == [O.OK] and nix["start"] == [0] * bool(a) + cuts[first[b]:first[b + 1]], name
            assert new[:10] == M.STREAM_ID and sum(len(new[r[1] - 8:r[1] + r[2]]) for r in R.walk(new)[0]) == len(new) - 10     # data chunks and nothing else
        assert RX.same_index(got["index"], X.build_index(RX.after(streams, got)))
    # at the cuts the foreign chunks lie at, they are kept as they are: uncompressed ones stay uncompressed, which no encoder writes for html
    g = list(cases).index("on_the_grid_with_a_skippable_chunk")
    first, cuts = CM.regular_cuts([len(a) for a in raws], 500)
    got = RX.recut_plan(streams, ix, first, cuts)
    assert got["streams"][g] == streams[g].replace(M.chunk(0x80, b"note"), b"") != CM.encode_at_cuts(raws, first, cuts)["streams"][g]


def test_corruption_in_a_dirty_chunk_is_noticed_in_a_kept_chunk_copied_and_rewrite_all_is_the_scrub():
    html = read_testdata("html") * 2
    raw = html[:9000]
    cuts = [1000, 3000, 4000, 6500]
    s = RX.stream_at(raw, [1000, 3000, 5000, 6500])                     # rows 2 and 3 are dirty for `cuts`, rows 0, 1 and 4 clean
    rows = R.walk(s)[0]
    bad = [R.corrupt_chunk(s, rows[i]) for i in (0, 2, 3)]
    ix = X.build_index([s] * 4)
    first, flat = RX.lists([cuts] * 4)
    got = RX.recut_plan(bad + [s], ix, first, flat)
    want2, want3 = M.chunk_status(bad[1], rows[2]), M.chunk_status(bad[2], rows[3])
    assert want2 != O.OK and want3 != O.OK
    assert got["status"] == [O.OK, want2, want3, O.OK]
    assert got["streams"][1] is None and got["out_len"][1] == 0 and got["out_bound"][1] == 0 and got["out_bound"][3] > 0
    assert got["streams"][3] == RX.stream_at(raw, cuts)
    c0 = rows[1][1] - 8                                                 # chunk 0 ends where chunk 1's header starts
    assert got["streams"][0][:c0] == bad[0][:c0] != s[:c0] and got["streams"][0][c0:] == got["streams"][3][c0:]      # copied as it is
    with pytest.raises(O.OracleError):
        O.frame_decode(got["streams"][0])
    assert got["result"][3] == 2 and got["result"][6:] == [6, 4] and got["index"]["tail"] == [0] * 4
    scrub = RX.recut_plan(bad + [s], ix, first, flat, ALL)
    assert scrub["status"] == [M.chunk_status(bad[0], rows[0]), want2, want3, O.OK] and scrub["status"][0] != O.OK
    both = R.corrupt_chunk(bad[1], rows[3])                             # two dirty chunks corrupt: the first one's status
    assert RX.recut_plan([both], X.build_index([s]), [0, 4], cuts)["status"] == [want2]


# ---- every rejection of the list ------------------------------------------------------------------------------------------------------------------
def test_every_list_rejection_fails_its_stream_alone():
    html = read_testdata("html")
    raws = [html[:2500], html[100:3300], html[7:1800]]
    streams = [K.stream_of(a, 900) for a in raws]
    ix = X.build_index(streams)
    good = [[1000, 2000], [500], [900]]
    sound = RX.recut_plan(streams, ix, *RX.lists(good))
    assert sound["status"] == [O.OK] * 3 and sound["alone"] == [False, False, True]
    total = len(raws[1])

    def refused_alone(got, b, name):
        assert got["status"][b] == O.ERR_BAD_ARG and got["streams"][b] is None and got["out_len"][b] == 0 and got["out_bound"][b] == 0, name
        for o in range(3):
            if o != b:
                assert got["status"][o] == O.OK and got["streams"][o] == sound["streams"][o] and got["alone"][o] == sound["alone"][o], (name, o)
        f0, f1, g0, g1 = ix["first"][b], ix["first"][b + 1], got["index"]["first"][b], got["index"]["first"][b + 1]
        assert got["index"]["start"][g0:g1] == ix["start"][f0:f1] and got["index"]["pos"][g0:g1] == ix["pos"][f0:f1], name      # its old rows
        k = got["plans"][b]
        assert RX.counts(k) == (0, 0, 0, 0, k["rows"]), name                # it counts nothing but its old rows
        others = RX.recut_plan([s for o, s in enumerate(streams) if o != b], X.build_index([s for o, s in enumerate(streams) if o != b]),
                               *RX.lists([c for o, c in enumerate(good) if o != b]))
        assert got["result"][:4] == others["result"][:4] and got["result"][5:] == others["result"][5:], name

    # what a cut may not be: the stream in the middle fails alone
    for name, bc in {"a_cut_of_zero": [0, 1000], "a_cut_at_total": [1000, total], "a_cut_past_total": [1000, total + 5],
                     "repeated_cuts": [1000, 1000, 2000], "descending_cuts": [2000, 1000, 2500], "descending_at_the_end": [1000, 2000, 1999]}.items():
        refused_alone(RX.recut_plan(streams, ix, *RX.lists([good[0], bc, good[2]])), 1, name)
    # what cut_first may not be: the last stream's range decreases, ends past ncuts, and a list that the call is told is shorter than it is
    flat = good[0] + good[1] + good[2] + [1000, 1200]
    refused_alone(RX.recut_plan(streams, ix, [0, 2, 3, 1], flat), 2, "cut_first_decreasing")
    refused_alone(RX.recut_plan(streams, ix, [0, 2, 3, 7], flat), 2, "cut_first_past_ncuts")
    refused_alone(RX.recut_plan(streams, ix, [0, 2, 3, 4], flat, ncuts=3), 2, "a_cut_at_or_above_ncuts")
    assert RX.recut_plan(streams, ix, [0, 2, 3, 4], flat, ncuts=4) == sound
    # a piece of 65 537 bytes, between cuts and behind the last; 65 536 passes
    big = (html * 3)[:140000]
    s = K.stream_of(big, 65536)
    bix = X.build_index([s])
    for cuts, ok in (([65536, 131072], True), ([65537, 131072], False), ([65536], False), ([4464, 70000, 135536], True), ([4463, 70000], False)):
        got = RX.recut_plan([s], bix, [0, len(cuts)], cuts)
        assert got["status"] == [O.OK if ok else O.ERR_BAD_ARG], cuts
    # a cut for an empty stream
    for e in (M.STREAM_ID, b""):
        assert RX.recut_plan([e], X.build_index([e]), [0, 1], [1])["status"] == [O.ERR_BAD_ARG]
        assert RX.recut_plan([e], X.build_index([e]), [0, 1], [0])["status"] == [O.ERR_BAD_ARG]
        assert RX.recut_plan([e], X.build_index([e]), [0, 0], [])["status"] == [O.OK]
    # the index's own verdict comes first: a stream that was not indexed keeps that status whatever its list holds
    trunc = R.uniform_stream(3, 1)[0][:-5]
    tix = X.build_index([trunc])
    assert RX.recut_plan([trunc], tix, [0, 2], [5, 5])["status"] == [O.ERR_TRUNCATED_STREAM]


# ---- unsound indexes ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def named():
    cases = X.named_streams()
    streams = list(cases.values())
    return list(cases), streams, X.build_index(streams)


def test_unsound_indexes_get_the_models_verdicts(named):
    names, streams, ix = named
    rng = np.random.default_rng(5)
    first, cuts = CM.regular_cuts(ix["total"], 4096)
    sound = RX.recut_plan(streams, ix, first, cuts)
    same_as_rechunk(sound, RC.rechunk_plan(streams, ix, 4096))
    refused = kept = 0
    for bad in RC.unsound_indexes(ix, streams, rng):
        ne = min(len(bad["start"]), len(bad["pos"]))
        me = ne + 64
        bfirst, bcuts = CM.regular_cuts(bad["total"], 4096) if max(bad["total"]) < (1 << 30) else (first, cuts)
        got = RX.recut_plan(streams, bad, bfirst, bcuts, max_slots=1 << 20, stage_cap=1 << 28, max_entries=me)
        same_as_rechunk(got, RC.rechunk_plan(streams, bad, 4096, max_slots=1 << 20, stage_cap=1 << 28, max_entries=me)) if bfirst is not first else None
        assert len(got["index"]["start"]) == len(got["index"]["pos"]) <= me                # the new arrays stay inside max_entries
        assert got["index"]["first"][-1] == len(got["index"]["start"]) and got["index"]["first"] == sorted(got["index"]["first"])
        for b, s in enumerate(streams):
            if got["streams"][b] is None:
                assert got["out_len"][b] == 0
                refused += got["status"][b] != sound["status"][b]
            else:
                kept += 1
    assert refused > 40 and kept > 10, (refused, kept)


# ---- admission ----------------------------------------------------------------------------------------------------------------------------------------
def test_admission_is_in_stream_order_by_each_bound_and_out_cap_hits_one_stream():
    html = read_testdata("html")
    blobs = [html[:700], html[50:50 + 1024], html[9:9 + 1300], html[:100], html[:2000]]
    streams = [K.stream_of(x, 500) for x in blobs[:3]] + [K.stream_of(blobs[3], 512), K.stream_of(blobs[4], 300)]
    ix = X.build_index(streams)
    first, cuts = RX.lists([[512], [512], [500, 1012], [], [300, 700, 1200, 1500]])
    full = RX.recut_plan(streams, ix, first, cuts)
    assert full["status"] == [O.OK] * 5 and full["alone"] == [False, False, False, True, False]
    dirty = [2, 3, 2, 0, 5]                                             # stream 2 keeps [0, 500), stream 4 keeps [0, 300) and [1200, 1500)
    slots = [2, 2, 2, 0, 3]
    dec = [700, 1024, 800, 0, 1400]
    comp = [K.stride(512) + K.stride(188), 2 * K.stride(512), K.stride(512) + K.stride(288), 0, K.stride(400) + 2 * K.stride(500)]
    rows = [2, 3, 3, 1, 7]
    assert full["result"] == [max(sum(dirty), sum(slots)), sum(full["out_len"]), sum(dec) + sum(comp), 4, sum(rows), 1, 3, sum(slots)]
    ms, sc, me = full["result"][0], full["result"][2], full["result"][4]
    assert RX.recut_plan(streams, ix, first, cuts, max_slots=ms, stage_cap=sc, max_entries=me) == full
    late = [O.OK, O.OK, O.OK, O.OK, O.ERR_OUTPUT_TOO_SMALL]
    for bounds in (dict(max_slots=ms - 1, stage_cap=sc, max_entries=me), dict(max_slots=ms, stage_cap=sc - 1, max_entries=me),
                   dict(max_slots=ms, stage_cap=sc, max_entries=me - 1)):
        short = RX.recut_plan(streams, ix, first, cuts, **bounds)
        assert short["status"] == late and short["streams"][:3] == full["streams"][:3] and short["streams"][4] is None, bounds
        assert short["result"] == [ms, sum(short["out_len"]), sc, 3, me, 1, 1, 6]
        assert RX.same_index(short["index"], X.build_index(RX.after(streams, short)))
    # in the middle: stream 1 misses, and every later one that needs work; the one that needs none is left alone all the same
    mid = [O.OK, O.ERR_OUTPUT_TOO_SMALL, O.ERR_OUTPUT_TOO_SMALL, O.OK, O.ERR_OUTPUT_TOO_SMALL]
    assert RX.recut_plan(streams, ix, first, cuts, max_slots=4, stage_cap=sc, max_entries=me)["status"] == mid            # 2 + 3 dirty rows
    one_more = dec[0] + comp[0] + dec[1] + comp[1]
    assert RX.recut_plan(streams, ix, first, cuts, max_slots=ms, stage_cap=one_more - 1, max_entries=me)["status"] == mid
    assert RX.recut_plan(streams, ix, first, cuts, max_slots=ms, stage_cap=one_more, max_entries=me)["status"][:2] == [O.OK, O.OK]
    assert RX.recut_plan(streams, ix, first, cuts, max_slots=ms, stage_cap=sc, max_entries=4)["status"] == mid
    sizing = RX.recut_plan(streams, ix, first, cuts, caps=[0] * 5, max_slots=0, stage_cap=0, max_entries=0)
    assert sizing["result"] == [ms, 0, sc, 0, me, 1, 0, 0] and sizing["out_bound"] == full["out_bound"]
    assert sizing["status"] == [O.ERR_OUTPUT_TOO_SMALL] * 3 + [O.OK, O.ERR_OUTPUT_TOO_SMALL]
    assert all(b >= n for b, n in zip(sizing["out_bound"], full["out_len"]))
    caps = list(full["out_len"])
    caps[2] -= 1                                                        # one byte short, in the middle
    one = RX.recut_plan(streams, ix, first, cuts, caps=caps)
    assert one["status"] == [O.OK, O.OK, O.ERR_OUTPUT_TOO_SMALL, O.OK, O.OK] and one["streams"][2] is None and one["out_len"][2] == 0
    assert RX.same_index(one["index"], X.build_index(RX.after(streams, one)))
    assert one["result"] == [ms, sum(one["out_len"]), sc, 3, me, 1, 2, 7]
    assert RX.recut_plan(streams, ix, first, cuts, caps=full["out_len"]) == full


# ---- the end-to-end property -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", [O.HASH_CRC32C, O.HASH_MUL])
def test_content_defined_streams_after_edits_come_back_to_the_encoders_chunks(variant):
    cases = RX.end_to_end(read_testdata("html"), 32, 256, variant)
    assert list(cases) == ["insert_mid_chunk", "delete_across_chunks", "append", "three_edits"]
    for name, (s, raw) in cases.items():
        assert O.frame_decode(s) == raw, name
        cuts = CM.cuts_of(raw, 32, 256)[0]
        assert 60 <= len(cuts) <= 250, (name, len(cuts))                # roughly a hundred pieces
        want = CM.encode_at_cuts([raw], [0, len(cuts)], cuts, variant)
        assert s != want["streams"][0], name                            # the edit left the cuts
        got = RX.recut_plan([s], X.build_index([s]), [0, len(cuts)], cuts, variant=variant)
        # the condition on the inputs: the model alone yields kept and rebuilt pieces
        assert got["result"][6] >= 1 and got["result"][7] >= 1, (name, got["result"])
        assert got["result"][6] > 4 * got["result"][7] or name == "three_edits", (name, got["result"])     # almost every chunk is copied
        assert got["status"] == [O.OK] and got["streams"] == want["streams"], name
        assert RX.same_index(got["index"], {k: want[k] for k in ("first", "start", "pos", "total", "tail")}), name
        again = RX.recut_plan(got["streams"], got["index"], [0, len(cuts)], cuts, variant=variant)
        assert again["alone"] == [True] and again["result"] == [0, 0, 0, 0, len(cuts) + 1, 1, 0, 0], name


# ---- the planning header on the CPU, under sanitizers ------------------------------------------------------------------------------------------
def test_planning_header_under_sanitizers_matches_the_model(named, directed, tmp_path):
    _, nstreams, _ = named
    dnames, dstreams, draws, dfirst, dcuts, _ = directed
    html = read_testdata("html") * 5
    foreign = [c[0] for c in RC.foreign_streams(html).values()]
    e2e = [c[0] for c in RX.end_to_end(read_testdata("html")).values()]
    shaped = fragmented(html, 1000, O.HASH_CRC32C)[2] + [K.stream_of(html[:n], 1000) for n in (0, 1, 1000, 3500)]
    streams = dstreams + nstreams + foreign + e2e + shaped
    ix = X.build_index(streams)
    ns = len(streams)
    rng = np.random.default_rng(11)
    totals = ix["total"]
    pad = [[] for _ in range(ns - len(dstreams))]
    lists = {"directed": RX.lists([dcuts[dfirst[b]:dfirst[b + 1]] for b in range(len(dstreams))] + pad)}
    for cb in (1000, 4096, 65536):
        lists["grid %d" % cb] = CM.regular_cuts(totals, cb)
    per = []
    for b, s in enumerate(streams):
        try:
            per.append(CM.cuts_of(O.frame_decode(s), 32, 256)[0])
        except O.OracleError:
            per.append(list(range(200, totals[b], 200)))
    lists["content"] = RX.lists(per)
    cases = [(ix, f, c, len(c), flags) for f, c in lists.values() for flags in (0, ALL)]
    nsound = len(cases)
    cfirst, ccuts = lists["content"]
    cases += [(bad, cfirst, ccuts, len(ccuts), flags) for bad in RC.unsound_indexes(ix, streams, rng) for flags in (0, ALL)]
    # every rejection of the list, for every stream at once; ncuts that cuts the list short
    for name, (bf, bc, nc) in RX.bad_lists(3000).items():
        cases.append((ix, [bf[0]] + [bf[1]] * ns, bc + [0] * 8, nc, 0))
    cases.append((ix, cfirst, ccuts, len(ccuts) // 2, 0))
    # random indexes and lists: arrays filled with anything
    for _ in range(8):
        ne, nc = int(rng.integers(0, 40)), int(rng.integers(0, 60))
        cases.append((dict(first=[int(v) for v in rng.integers(0, ne + 3, ns + 1)], start=[int(v) for v in rng.integers(0, 5000, ne)],
                           pos=[int(v) for v in rng.integers(0, 3000, ne)], total=[int(v) for v in rng.integers(0, 9000, ns)],
                           tail=[int(v) for v in rng.integers(-1, 3, ns)]),
                      [int(v) for v in rng.integers(0, nc + 3, ns + 1)], [int(v) for v in rng.integers(0, 9000, nc)], nc, int(rng.integers(0, 2))))
    for _ in range(4):                                                  # a sound index under lists filled with anything, sorted or not
        nc = int(rng.integers(ns, 4 * ns))
        anyc = [int(v) for v in rng.integers(0, 6000, nc)]
        cases.append((ix, sorted(int(v) for v in rng.integers(0, nc + 1, ns + 1)), anyc if _ % 2 else sorted(anyc), nc, 0))
    # streams past 4 GiB, as numbers: two rows behind positions past 4 GiB with cuts past 4 GiB -- both kept; the same with the flag (a dirty row
    # above 65536: refused) and with rows of 65536; a cut that splits the second row; a cut equal to the total; a cut past it; descending cuts;
    # a piece of 65537 between cuts past 4 GiB; a skippable chunk at the second row; one row and a total past 4 GiB that no row holds; no row and
    # nothing decoded: the identifier is missing, present; a cut for it
    G = 1 << 32
    base = dict(n=3 * G, flags=0, total=5 * G + 65536 + 3000, tail=0, rows=2, ident=1, start0=0, pos0=2 * G + 10, kind0=0, size0=4 + 65536, dec0=65536,
                start1=65536, pos1=2 * G + 10 + 65544, kind1=0, size1=4 + 3000, dec1=3000, ncuts=1, cut0=65536, cut1=0, cut2=0)
    small = {**base, "total": 65536 + 3000}
    far = {**base, "start0": 0, "dec0": 65536, "total": 65536 + 3000}
    numeric = [small, {**small, "flags": ALL}, {**small, "ncuts": 2, "cut1": 65536 + 1000}, {**small, "ncuts": 2, "cut1": 65536 + 3000},
               {**small, "ncuts": 2, "cut1": 5 * G}, {**small, "ncuts": 2, "cut0": 65536 + 5, "cut1": 65536}, {**small, "cut0": 2999},
               {**small, "kind1": 1}, {**base, "rows": 1}, {**base, "rows": 0, "total": 0, "n": 0, "ident": 0, "ncuts": 0},
               {**base, "rows": 0, "total": 0, "n": 10, "ncuts": 0}, {**base, "rows": 0, "total": 0, "n": 10, "ncuts": 1, "cut0": 0},
               {**far, "pos0": 10, "pos1": 10 + 65544, "n": 10 + 65544 + 3008},
               # decoded offsets past 4 GiB: a one-row stream is refused (no chunk decodes to 5 GiB), a list past 4 GiB with pieces above 65536 too
               {**base, "rows": 1, "dec0": 65536, "total": 65536, "ncuts": 0},
               {**base, "rows": 2, "start1": 5 * G, "dec0": 65536, "total": 5 * G + 3000, "ncuts": 1, "cut0": 5 * G}]
    path = str(tmp_path / "cases.bin")
    RX.write_cases(path, streams, cases, numeric)
    exe = str(tmp_path / "frame_recut_plan_check")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host",
                    "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "abi", "frame_recut_plan_check.hip"), "-o", exe,
                    "-Wl,-rpath,/opt/rocm/lib"], check=True)
    env = {**os.environ, "ASAN_OPTIONS": "detect_leaks=1:abort_on_error=0", "UBSAN_OPTIONS": "print_stacktrace=1:halt_on_error=1"}
    run = subprocess.run([exe, path], capture_output=True, text=True, env=env)
    assert run.returncode == 0 and run.stderr == "", run.stderr[-3000:]      # the sanitizers are silent
    lines = run.stdout.splitlines()
    assert len(lines) == ns * len(cases) + len(numeric)
    at = passed = refused = kept = 0
    for c, (index, cf, cu, nc, flags) in enumerate(cases):
        for b, w in enumerate(RX.plan_lines(index, streams, cf, cu, nc, flags)):
            assert lines[at] == w, (c, b, flags)
            unsound = c >= nsound
            passed += unsound and w.startswith("0 1 ")
            refused += unsound and not w.startswith("0 ")
            kept += w.startswith("0 1 ") and int(w.split()[8]) > 0 and int(w.split()[7]) > 0
            at += 1
    assert passed > 50 and refused > 200 and kept > 20, (passed, refused, kept)    # both outcomes on the unsound inputs; plans with kept and rebuilt pieces
    want = [RX.numeric_line(c) for c in numeric]
    assert lines[at:] == want
    f = [[int(v) for v in w.replace("|", " ").split()] for w in want]
    assert f[0][:2] == [0, 1] and f[0][4:10] == [0, 0, 2, 0, 2, 65544 + 3008]          # not canonical by position alone: both rows kept
    assert f[1][:2] == [0, 1] and f[1][4:9] == [2, 65536 + 3000, 2, 2, 0] and f[1][25:31] == [0, 0, 65536, 1, 65536, 3000]
    assert f[2][:2] == [0, 1] and f[2][4:9] == [1, 3000, 3, 2, 1] and f[2][25:31] == [1, 0, 1000, 2, 1000, 2000]
    for i in (3, 4, 5, 6, 7, 8, 11, 14):
        assert f[i][0] == O.ERR_BAD_ARG, i
    assert f[9][:2] == [0, 1] and f[9][11] == 10 and f[10][:2] == [0, 0]
    assert f[12][:2] == [0, 0]                                          # canonical
    assert f[13][:2] == [0, 1] and f[13][6:9] == [1, 0, 1]              # one row that is the one piece, behind a position past 4 GiB: kept

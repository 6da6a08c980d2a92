"""snp_frame_compose_indexed_batch (libsnappier_hip_frame_compose.so) without a GPU: the declarations and their C# binding, the workspace
arithmetic, argument rejection; the Python model of the contract (frame_compose_model.py) checked against the oracle's frame decode, the index
model, the chunked encoder's model and the rechunk model: sources written at the seam chunk sizes with both hash variants and sources
fragmented through the splice, update and append models; claims (a), (b) and (c) of the header on every shape of a segment list; sources with
skippable and padding chunks and zero-length rows; corruption in an edge and in a kept chunk; every rejection; unsound indexes; admission by
each bound and out_cap; the sizing call; and the planning header (csrc/frame_compose_device.h) itself, compiled for the CPU under
AddressSanitizer and UBSan into a stand-alone program (tests/abi/frame_compose_plan_check.hip) and run over the same cases, over indexes and
segment lists filled with anything at all and over sources past 4 GiB given as numbers."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import frame_buffers_model as M
import frame_chunked_model as K
import frame_compose_model as CM
import frame_index_model as X
import frame_range_model as R
import frame_rechunk_model as RC
import oracle as O
from conftest import ROOT, read_testdata
from test_frame_rechunk_model import fragmented

NAMES = ["snp_frame_compose_indexed_batch", "snp_frame_compose_indexed_workspace"]


def _lib():
    from snappier_amd import _native as N
    return N.frame_compose_lib()


# ---- the surface -----------------------------------------------------------------------------------------------------------------------------
def test_header_and_binding_declare_the_new_functions():
    from snappier_amd import _native as N
    declared = N.frame_compose_declared_symbols()
    assert sorted(declared) == NAMES
    others = set(N.declared_symbols()) | set(N.buffers_declared_symbols()) | set(N.buffers_decompress_declared_symbols()) | \
        set(N.frame_buffers_declared_symbols()) | set(N.layout_declared_symbols()) | set(N.frame_range_declared_symbols()) | \
        set(N.frame_index_declared_symbols()) | set(N.frame_chunked_declared_symbols()) | set(N.frame_update_declared_symbols()) | \
        set(N.frame_append_declared_symbols()) | set(N.frame_splice_declared_symbols()) | set(N.frame_rechunk_declared_symbols())
    assert not set(declared) & others                                  # the other headers' surfaces are left as they are
    lib = _lib()
    assert lib.snp_frame_compose_indexed_batch.restype is C.c_int and len(lib.snp_frame_compose_indexed_batch.argtypes) == 34
    assert lib.snp_frame_compose_indexed_workspace.restype is C.c_uint64 and len(lib.snp_frame_compose_indexed_workspace.argtypes) == 7
    from snappier_amd import batch as SB
    assert callable(SB.BlockCodec.frame_compose_indexed) and callable(SB.BlockCodec.frame_compose_to_memory)


def test_extension_library_exports_exactly_its_header():
    from layouts import exported
    from snappier_amd import _native as N

    ext = exported(N.FRAME_COMPOSE_PATH)
    assert ext == set(NAMES)
    for other in (N.PRODUCT_PATH, N.BUFFERS_PATH, N.BUFFERS_DECOMPRESS_PATH, N.FRAME_BUFFERS_PATH, N.LAYOUT_PATH, N.FRAME_RANGE_PATH, N.FRAME_INDEX_PATH,
                  N.FRAME_CHUNKED_PATH, N.FRAME_UPDATE_PATH, N.FRAME_APPEND_PATH, N.FRAME_SPLICE_PATH, N.FRAME_RECHUNK_PATH):
        assert not exported(other) & ext


def test_workspace_is_host_arithmetic():
    ws = _lib().snp_frame_compose_indexed_workspace
    assert ws(3, 0, 10, 10, 1000, 4096, 50) == 0                        # nothing when there is no output
    assert ws(3, 5, 10, 10, 1000, 0, 50) == 0 and ws(3, 5, 10, 10, 1000, 65537, 50) == 0     # ... or no chunk size the call takes
    for no in (1, 255, 1025, 300000):
        for ng in (0, 1, 4100, 300001):
            for ms in (0, 1, 33000):
                for sc in (0, 70000, 1 << 33):
                    for cb in (1, 4096, 65536):
                        for me in (0, 7, 100000):
                            w = ws(9, no, ng, ms, sc, cb, me)
                            stride = K.stride(cb)
                            assert w % 256 == 0 and w == ws(0, no, ng, ms, sc, cb, me)      # nothing is kept per source
                            # the staging, the compressed staging, the slot table (32) and the decode table (41) with the size scan (8), the
                            # outputs' words (9 + 6 of 8 bytes, 1 of 4), the segments' (10 + 8 of 8 bytes, 5 of 4), the new rows' (8 + 4 + 8)
                            assert w >= sc + ms * (stride + 81) + no * 124 + ng * 164 + me * 20
                            assert w <= sc + 256 + ms * (stride + 81) + no * 124 + ng * 164 + me * 20 + 80 * 256 + (no + ng + ms + me) // 50
                            assert ws(9, no + 1, ng, ms, sc, cb, me) >= w and ws(9, no, ng + 1, ms, sc, cb, me) >= w
                            assert ws(9, no, ng, ms + 1, sc, cb, me) >= w and ws(9, no, ng, ms, sc + 1, cb, me) >= w
                            assert ws(9, no, ng, ms, sc, cb, me + 1) >= w
    assert ws(1, 0x7FFFFFFF, 0x7FFFFFFF, 0xFFFFFFFF, 1 << 40, 65536, 0xFFFFFFFF) > 0xFFFFFFFF * 76496 + (1 << 40)      # (64-bit arithmetic)


def test_batch_call_rejects_bad_arguments_without_a_device():
    call = _lib().snp_frame_compose_indexed_batch
    fake = C.c_void_p(64)                                               # (never dereferenced: the arguments are refused first)
    # ctx; in, in_off, in_len; nstreams; five index arrays; nentries; four segment arrays; nout, nsegs, chunk_bytes, max_slots, stage_cap,
    # max_entries; out, out_off, out_cap, out_len, status; five new index arrays; out_bound; d_work, d_result
    def args(ctx=fake, ins=(fake,) * 3, ns=1, idx=(fake,) * 5, ne=8, segs=(fake,) * 4, no=1, ng=1, cb=4096, ms=0, sc=0, me=8, outs=(fake,) * 5,
             new=(fake,) * 5, bound=None, work=fake, result=fake):
        return (ctx, *ins, ns, *idx, ne, *segs, no, ng, cb, ms, sc, me, *outs, *new, bound, work, result)

    assert call(*args(ctx=None)) == O.ERR_BAD_ARG
    assert call(*args(result=None)) == O.ERR_BAD_ARG
    assert call(*args(no=0, result=None)) == O.ERR_BAD_ARG             # an empty call still needs d_result
    assert call(*args(cb=0)) == O.ERR_BAD_ARG and call(*args(cb=65537)) == O.ERR_BAD_ARG
    assert call(*args(no=0, cb=0)) == O.ERR_BAD_ARG                    # ... also when there is no output
    assert call(*args(no=1 << 31)) == O.ERR_BAD_ARG and call(*args(ng=1 << 31)) == O.ERR_BAD_ARG and call(*args(ns=1 << 31)) == O.ERR_BAD_ARG
    assert call(*args(work=None)) == O.ERR_BAD_ARG
    for group, n in (("ins", 3), ("outs", 5), ("segs", 4)):
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
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "snappier_hip_frame_compose.h")).read(), flags=re.S)
    protos = {}
    for m in re.finditer(r"([A-Za-z_][A-Za-z0-9_ ]*?[\s\*]+)(snp_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", text):
        params = [re.match(r"(.*?[\s\*])([A-Za-z_][A-Za-z0-9_]*)$", q.strip()).group(1) for q in m.group(3).split(",") if q.strip() not in ("", "void")]
        protos[m.group(2)] = (T.c_class(m.group(1)), [T.c_class(q) for q in params])
    cs = re.sub(r"//.*", "", open(os.path.join(ROOT, "csharp", "Snappier.Gpu", "NativeMethodsFrameCompose.cs")).read())
    assert 'const string Lib = "snappier_hip_frame_compose"' in cs
    imps = {}
    for m in re.finditer(r"\[DllImport\(Lib, CallingConvention = Cc\)\]\s*internal static extern ([A-Za-z\*]+) (snp_[a-z0-9_]+)\(([^)]*)\);", cs):
        params = [re.match(r"(.*?)\s+([A-Za-z_][A-Za-z0-9_]*)$", q.strip()).group(1) for q in m.group(3).split(",") if q.strip()]
        imps[m.group(2)] = (T.cs_class(m.group(1)), [T.cs_class(q) for q in params])
    assert set(protos) == set(imps) == set(NAMES)
    for name, (ret, params) in protos.items():
        cret, cparams = imps[name]
        assert T.compatible(ret, cret), (name, ret, cret)
        assert len(params) == len(cparams) and all(T.compatible(a, b) for a, b in zip(params, cparams)), (name, params, cparams)
    assert len(protos["snp_frame_compose_indexed_batch"][1]) == 34 and len(protos["snp_frame_compose_indexed_workspace"][1]) == 7
    proj = open(os.path.join(ROOT, "csharp", "Snappier.Gpu", "Snappier.Gpu.csproj")).read()
    assert 'Include="../../snappier_amd/libsnappier_hip_frame_compose.so"' in proj


# ---- the model against the oracle ----------------------------------------------------------------------------------------------------------------
def check_outputs(streams, raws, ix, outputs, claims, cb, variant):
    """Claims (a), (b) and (c), the new index, the size bound and the sizing call, for a batch whose outputs are all written."""
    segs = CM.seg_lists(outputs)
    got = CM.compose_plan(streams, ix, segs, cb, variant=variant)
    assert got["status"] == [O.OK] * len(outputs)
    want = [CM.concat(raws, segments) for segments in outputs]
    for j, (new, raw) in enumerate(zip(got["streams"], want)):
        assert O.frame_decode(new) == raw, (cb, j)                     # (c)
        assert got["out_len"][j] == len(new) <= got["out_bound"][j] and new[:10] == M.STREAM_ID
        assert sum(len(c) for c in [new[:10]] + [new[r[1] - 8:r[1] + r[2]] for r in R.walk(new)[0]]) == len(new)    # data chunks and nothing else
        if claims[j] == "a":
            assert new == K.stream_of(raw, cb, variant), (cb, j)       # (a)
    nix = X.build_index(got["streams"])
    assert CM.same_index(got["index"], nix) and got["index"]["total"] == [len(x) for x in want]
    ms, sc, me = CM.needs(streams, ix, segs, cb)
    assert (ms, sc, me) == (got["result"][0], got["result"][2], got["result"][4]) and got["result"][1] == sum(got["out_len"])
    assert CM.compose_plan(streams, ix, segs, cb, max_slots=ms, stage_cap=sc, max_entries=me, variant=variant) == got
    return got, want


@pytest.mark.parametrize("cb", CM.CHUNK_SIZES)
def test_every_shape_on_sources_of_every_chunk_size(cb):
    html = read_testdata("html") * 5
    for variant in (O.HASH_CRC32C, O.HASH_MUL):
        streams, raws, ix, outputs, claims = CM.mixed_batch(html, cb, variant)
        assert all(O.frame_decode(s) == a for s, a in zip(streams, raws))
        got, want = check_outputs(streams, raws, ix, outputs, claims, cb, variant)
        # (b): the rechunk of an output is the chunked encoder's output for the concatenation -- with the flag for any source, without it for
        # sources this library wrote (all but the foreign ones)
        ours = len(outputs) - len(CM.foreign_outputs())
        rc = RC.rechunk_plan(got["streams"], got["index"], cb, variant=variant)
        assert RC.after(got["streams"], rc)[:ours] == [K.stream_of(raw, cb, variant) for raw in want[:ours]]
        every = RC.rechunk_plan(got["streams"], got["index"], cb, RC.REWRITE_ALL, variant=variant)
        assert every["streams"] == [K.stream_of(raw, cb, variant) for raw in want]
        # no segment, only empty ones: the identifier alone
        names = list(CM.shapes([len(raws[0]), len(raws[1])], cb))
        for name in ("no_segment", "only_empty_segments"):
            assert got["streams"][names.index(name)] == M.STREAM_ID and got["out_bound"][names.index(name)] == 10
        # a whole-stream concatenation rebuilds nothing
        whole = CM.compose_plan(streams, ix, CM.seg_lists([[(0, 0, len(raws[0])), (1, 0, len(raws[1]))]]), cb, variant=variant)
        assert whole["result"][0] == 0 and whole["result"][2] == 0 and whole["result"][5] == whole["result"][4] == len(ix["start"][:ix["first"][2]])
        assert whole["out_bound"] == whole["out_len"]


@pytest.mark.parametrize("cb", [64, 4096])
def test_sources_fragmented_through_the_splice_update_and_append_models(cb):
    html = read_testdata("html") * 5
    for variant in (O.HASH_CRC32C, O.HASH_MUL):
        names, raws, streams = fragmented(html, cb, variant)
        ix = X.build_index(streams)
        n = len(streams)
        outputs = [[(b, 0, len(raws[b]))] for b in range(n)] + [[(b, cb // 2, 2 * cb) for b in range(n)]] + \
                  [[(b, 1, len(raws[b]) - 2), ((b + 1) % n, cb, cb)] for b in range(n)]
        got, want = check_outputs(streams, raws, ix, outputs, ["c"] * len(outputs), cb, variant)
        assert got["streams"][:n] == streams                            # a whole stream of data chunks only: copied chunk for chunk
        rc = RC.rechunk_plan(got["streams"], got["index"], cb, variant=variant)
        assert RC.after(got["streams"], rc) == [K.stream_of(raw, cb, variant) for raw in want]     # (b), without the flag


def test_foreign_sources_drop_what_is_no_data_chunk_and_zero_length_rows_at_a_border():
    html = read_testdata("html")
    streams, raws = CM.foreign_sources(html)
    ix = X.build_index(streams)
    outputs = CM.foreign_outputs()
    zero = M.data_chunk(b"", compressed=False)
    for cb in (1, 300, 1000, 65536):
        got, want = check_outputs(streams, raws, ix, outputs, ["c"] * len(outputs), cb, O.HASH_CRC32C)
        assert b"note" not in b"".join(got["streams"]) and got["streams"][0].count(M.STREAM_ID) == 1
        # source 1: rows  z a z z b c z d z.  [1000, 1700) is row b alone: the zero-length rows at its borders are not taken
        assert got["streams"][3] == M.STREAM_ID + M.data_chunk(raws[1][1000:1700]) and got["result"][0] > 0
        # [0, 1700): the leading zero-length row lies at the border, the two between a and b lie inside and are copied
        assert got["streams"][4] == M.STREAM_ID + M.data_chunk(raws[1][:1000]) + zero + zero + M.data_chunk(raws[1][1000:1700])
        # [1000, 3400): the one between c and d is inside, the one behind d at the border
        assert got["streams"][5] == M.STREAM_ID + M.data_chunk(raws[1][1000:1700]) + M.data_chunk(raws[1][1700:3000]) + zero + M.data_chunk(raws[1][3000:])
        # [999, 1701): a cut on both sides; the two zero-length rows between a and b lie inside
        lens = RC.data_chunk_lengths(got["streams"][6])
        assert lens[0] == 1 and lens[-1] == 1 and lens.count(0) == 2 and 700 in lens or cb < 700


def test_corruption_in_an_edge_chunk_fails_its_output_and_in_a_kept_chunk_is_copied():
    html = read_testdata("html") * 2
    cb = 4096
    s = K.stream_of(html[:5 * cb], cb)
    rows = R.walk(s)[0]
    bad1, bad2, bad3 = [R.corrupt_chunk(s, rows[i]) for i in (1, 2, 3)]
    want1, want3 = M.chunk_status(bad1, rows[1]), M.chunk_status(bad3, rows[3])
    assert want1 != O.OK != want3
    streams = [s, bad1, bad2, bad3, R.corrupt_chunk(bad1, rows[3])]
    ix = X.build_index([s] * 5)
    # per source: chunk 1 cut at the head, chunk 2 kept, chunk 3 cut at the tail
    outputs = [[(b, cb + 9, 2 * cb)] for b in range(5)] + [[(0, 5, 10), (4, cb + 9, 2 * cb), (3, cb + 9, 2 * cb)]]
    got = CM.compose_plan(streams, ix, CM.seg_lists(outputs), cb)
    assert got["status"] == [O.OK, want1, O.OK, want3, want1, want1]   # the head edge's status comes first; the first failing segment's
    assert got["streams"][1] is None and got["out_len"][1] == 0 and got["out_bound"][1] == 0 and got["out_bound"][0] > 0
    assert got["index"]["tail"] == got["status"] and got["index"]["total"] == [2 * cb, 0, 2 * cb, 0, 0, 0]
    assert got["index"]["first"] == [0, 3, 3, 6, 6, 6, 6] and got["result"][3] == 2
    assert O.frame_decode(got["streams"][0]) == html[cb + 9:3 * cb + 9]
    with pytest.raises(O.OracleError):                                  # A CORRUPT KEPT CHUNK IS COPIED AS IT IS
        O.frame_decode(got["streams"][2])
    mid = got["index"]["pos"][4] - 10
    assert got["streams"][2][:10 + mid] == got["streams"][0][:10 + mid] and got["streams"][2] != got["streams"][0]


def test_every_rejection():
    html = read_testdata("html")
    cb = 1000
    streams = [K.stream_of(html[:n], 900) for n in (2500, 2000)] + [R.uniform_stream(3, 1)[0][:-5]]
    ix = X.build_index(streams)
    assert ix["tail"][2] == O.ERR_TRUNCATED_STREAM

    def statuses(outputs, segs=None, **change):
        return CM.compose_plan(streams, {**ix, **change}, segs or CM.seg_lists(outputs), cb)["status"]

    good = [(0, 1, 100)]
    assert statuses([good, [(3, 0, 1)], [(3, 0, 0)], [(1 << 31, 0, 0)], good]) == [O.OK] + [O.ERR_BAD_ARG] * 3 + [O.OK]      # seg_stream >= nstreams
    assert statuses([[(0, 2499, 2)], [(0, 2500, 0)], [(0, 2501, 0)], [(0, 0, 2500)]]) == [O.ERR_BAD_ARG, O.OK, O.OK, O.OK]      # above idx_total
    assert statuses([[(0, (1 << 64) - 1, 2)], [(0, 1 << 63, 1 << 63)]]) == [O.ERR_BAD_ARG] * 2                            # lo + len wraps
    assert statuses([[(2, 0, 10)], [(2, 0, 0)], good + [(2, 5, 1)]]) == [O.ERR_TRUNCATED_STREAM, O.OK, O.ERR_TRUNCATED_STREAM]   # a broken source
    assert statuses([[(1, 0, 5)], good], tail=[0, O.ERR_OUTPUT_TOO_SMALL, 0]) == [O.ERR_OUTPUT_TOO_SMALL, O.OK]
    assert statuses([[(1, 0, 5)], [(0, 0, 5)]], tail=[-1, 77, 0]) == [O.ERR_BAD_ARG] * 2                                   # no status of the walk
    assert statuses([good, [(1, 0, 5)]], first=[3, 0, 6, 7]) == [O.ERR_BAD_ARG, O.ERR_BAD_ARG]                             # f1 < f0; rows of another stream
    assert statuses([good, [(1, 0, 5)]], first=[0, 0, 6, 7])[0] == O.ERR_BAD_ARG                                           # bytes and no row
    assert statuses([good], total=[2501, 2000, 0]) == [O.OK] and statuses([[(0, 2000, 501)]], total=[2501, 2000, 0]) == [O.ERR_BAD_ARG]
    assert statuses([good], pos=[p + 1 for p in ix["pos"]]) == [O.ERR_BAD_ARG]
    assert statuses([[(0, 0, 2500)]], start=list(reversed(ix["start"]))) == [O.ERR_BAD_ARG]
    swapped = list(ix["pos"])
    swapped[0], swapped[1] = swapped[1], swapped[0]                     # each chunk at or behind the end of the chunk before it
    assert statuses([[(0, 0, 2500)]], pos=swapped) == [O.ERR_BAD_ARG] and statuses([[(0, 1800, 700)]], pos=swapped) == [O.OK]
    past = list(ix["pos"])
    past[2] = len(streams[0])                                           # pos past in_len
    assert statuses([[(0, 0, 2500)]], pos=past) == [O.ERR_BAD_ARG] and statuses([[(0, 0, 1800)]], pos=past) == [O.OK]
    # the first failing segment in segment order
    assert statuses([[(0, 0, 5), (2, 0, 1), (3, 0, 1)], [(0, 0, 5), (3, 0, 1), (2, 0, 1)]]) == [O.ERR_TRUNCATED_STREAM, O.ERR_BAD_ARG]
    # the segment list is untrusted: seg_first runs backwards; beyond nsegs it is clamped
    segs = CM.seg_lists([good, good, good])
    assert statuses(None, {**segs, "first": [0, 2, 1, 3]}) == [O.OK, O.ERR_BAD_ARG, O.OK]
    assert statuses(None, {**segs, "first": [0, 1, 1 << 40, 1 << 50]}) == [O.OK, O.OK, O.OK]
    assert CM.compose_plan(streams, ix, {**segs, "first": [0, 1, 1 << 40, 1 << 50]}, cb)["out_len"][2] == 10
    # a row at a skippable chunk; an edge above 65536 bytes
    skip = M.STREAM_ID + M.data_chunk(html[:100]) + M.chunk(0x80, b"note") + M.data_chunk(html[100:200])
    six = X.build_index([skip])
    moved = {**six, "pos": [six["pos"][0], six["pos"][1] - 8]}
    assert CM.compose_plan([skip], six, CM.seg_lists([[(0, 0, 200)]]), cb)["status"] == [O.OK]
    assert CM.compose_plan([skip], moved, CM.seg_lists([[(0, 0, 200)], [(0, 0, 100)]]), cb)["status"] == [O.ERR_BAD_ARG, O.OK]
    big = R.big_chunk_stream()[0]
    bix = X.build_index([big])
    over = next(i for i, n in enumerate(RC.data_chunk_lengths(big)) if n > 65536)
    at = bix["start"][over]
    assert CM.compose_plan([big], bix, CM.seg_lists([[(0, at + 1, 5)], [(0, 0, bix["total"][0])]]), cb)["status"] == [O.ERR_BAD_ARG, O.OK]


def test_unsound_indexes_get_verdicts_and_what_passes_is_data_chunks():
    cases = X.named_streams()
    streams = list(cases.values())
    ix = X.build_index(streams)
    rng = np.random.default_rng(5)
    outputs = []
    for b in range(len(streams)):
        t = ix["total"][b]
        outputs += [[(b, 0, t)], [(b, t // 3, t // 2), (b, 1, 1)]]
    segs = CM.seg_lists(outputs)
    sound = CM.compose_plan(streams, ix, segs, 4096)
    refused = kept = 0
    for bad in RC.unsound_indexes(ix, streams, rng):
        me = 2 * min(len(bad["start"]), len(bad["pos"])) + 256
        got = CM.compose_plan(streams, bad, segs, 4096, max_slots=1 << 20, stage_cap=1 << 28, max_entries=me)
        assert len(got["index"]["start"]) == len(got["index"]["pos"]) <= me
        assert got["index"]["first"][-1] == len(got["index"]["start"]) and got["index"]["first"] == sorted(got["index"]["first"])
        for j, new in enumerate(got["streams"]):
            if new is None:
                assert got["out_len"][j] == 0 and got["index"]["tail"][j] == got["status"][j] != O.OK
                refused += got["status"][j] != sound["status"][j]
            else:                                                       # whatever passed the checks is the identifier and data chunks
                assert got["out_len"][j] == len(new) <= got["out_bound"][j] and new[:10] == M.STREAM_ID
                rows = R.walk(new)[0]
                assert sum(len(c) for c in [new[:10]] + [new[r[1] - 8:r[1] + r[2]] for r in rows]) == len(new)
                assert sum(r[5] for r in rows) == got["index"]["total"][j] == sum(bad_len for bad_len in segs["len"][segs["first"][j]:segs["first"][j + 1]])
                kept += 1
    assert refused > 40 and kept > 10, (refused, kept)


def test_admission_is_in_output_order_by_each_bound_and_out_cap_hits_one_output():
    html = read_testdata("html")
    cb = 512
    raws = [html[:3000], html[50:50 + 2048]]
    streams = [K.stream_of(raws[0], 500), K.stream_of(raws[1], cb)]
    ix = X.build_index(streams)
    outputs = [[(0, 250, 1000)], [(1, 0, 1024)], [(0, 100, 50), (1, 5, 1000)], [], [(0, 1400, 1300)]]
    segs = CM.seg_lists(outputs)
    full = CM.compose_plan(streams, ix, segs, cb)
    assert full["status"] == [O.OK] * 5
    # [250, 1250): rows 0 and 2 cut, row 1 kept.  [0, 1024) of the 512 grid: two rows kept.  [100, 150): inside row 0; [5, 1005): row 0 cut at
    # the head, row 1 at the tail.  [1400, 2700): rows 2 and 5 cut, rows 3 and 4 kept
    edges = [2, 0, 3, 0, 2]
    slots = [2, 0, 3, 0, 2]
    stage = [1000, 0, 500 + 1024, 0, 1000]
    rows = [3, 2, 3, 0, 4]
    assert full["result"] == [sum(edges), sum(full["out_len"]), sum(stage), 5, sum(rows), 1 + 2 + 0 + 0 + 2]
    assert full["index"]["first"] == [0, 3, 5, 8, 8, 12] and full["out_len"][3] == 10
    ms, sc, me = full["result"][0], full["result"][2], full["result"][4]
    late = [O.OK, O.OK, O.OK, O.OK, O.ERR_OUTPUT_TOO_SMALL]
    for bounds in (dict(max_slots=ms - 1, stage_cap=sc, max_entries=me), dict(max_slots=ms, stage_cap=sc - 1, max_entries=me),
                   dict(max_slots=ms, stage_cap=sc, max_entries=me - 1)):
        short = CM.compose_plan(streams, ix, segs, cb, **bounds)
        assert short["status"] == late and short["streams"][:4] == full["streams"][:4] and short["streams"][4] is None, bounds
        assert short["result"] == [ms, sum(short["out_len"]), sc, 4, me, 3]
        assert short["index"]["first"] == [0, 3, 5, 8, 8, 8] and short["index"]["tail"][4] == O.ERR_OUTPUT_TOO_SMALL
        assert short["out_bound"] == full["out_bound"]
    # in the middle: output 2 misses, and every later one -- also the one with no segment
    mid = [O.OK, O.OK] + [O.ERR_OUTPUT_TOO_SMALL] * 3
    assert CM.compose_plan(streams, ix, segs, cb, max_slots=4)["status"] == mid
    assert CM.compose_plan(streams, ix, segs, cb, stage_cap=1000 + 1523)["status"] == mid
    assert CM.compose_plan(streams, ix, segs, cb, max_entries=7)["status"] == mid
    sizing = CM.compose_plan(streams, ix, segs, cb, caps=[0] * 5, max_slots=0, stage_cap=0, max_entries=0)
    assert sizing["result"] == [ms, 0, sc, 0, me, 0] and sizing["out_bound"] == full["out_bound"] and sizing["streams"] == [None] * 5
    assert sizing["status"] == [O.ERR_OUTPUT_TOO_SMALL] * 5 and sizing["index"]["first"] == [0] * 6 and sizing["index"]["total"] == [0] * 5
    assert all(b >= n for b, n in zip(sizing["out_bound"], full["out_len"]))
    caps = list(full["out_len"])
    caps[2] -= 1                                                        # one byte short, in the middle
    one = CM.compose_plan(streams, ix, segs, cb, caps=caps)
    assert one["status"] == [O.OK, O.OK, O.ERR_OUTPUT_TOO_SMALL, O.OK, O.OK] and one["streams"][2] is None and one["out_len"][2] == 0
    assert one["index"]["first"] == [0, 3, 5, 5, 5, 9] and one["result"] == [ms, sum(one["out_len"]), sc, 4, me, 5]
    left = [x for x in one["streams"] if x is not None]
    assert one["index"]["pos"] == X.build_index(left)["pos"]


# ---- the planning header on the CPU, under sanitizers ------------------------------------------------------------------------------------------
def test_planning_header_under_sanitizers_matches_the_model(tmp_path):
    html = read_testdata("html") * 5
    streams, raws, ix, outputs, _ = CM.mixed_batch(html, 1000)
    named = list(X.named_streams().values())
    streams = streams + named
    ix = X.build_index(streams)
    ns = len(streams)
    for b in range(len(raws), ns):
        t = ix["total"][b]
        outputs = outputs + [[(b, 0, t)], [(b, t // 3, t // 2), (b, 1, 1)]]
    segs = CM.seg_lists(outputs + [[(ns, 0, 1)], [(0, 1 << 63, 1 << 63), (1, 5, 0)]])
    rng = np.random.default_rng(11)
    cases = [(ix, segs, cb) for cb in (1, 500, 1000, 4096, 65536)]
    nsound = len(cases)
    cases += [(bad, segs, cb) for bad in RC.unsound_indexes(ix, streams, rng) for cb in (1000, 65536)]
    # random indexes and segment lists: filled with anything
    for _ in range(8):
        ne, ng, no = int(rng.integers(0, 40)), int(rng.integers(0, 30)), int(rng.integers(0, 6))
        index = dict(first=[int(v) for v in rng.integers(0, ne + 3, ns + 1)], start=[int(v) for v in rng.integers(0, 5000, ne)],
                     pos=[int(v) for v in rng.integers(0, 3000, ne)], total=[int(v) for v in rng.integers(0, 9000, ns)],
                     tail=[int(v) for v in rng.integers(-1, 3, ns)])
        anything = dict(first=[int(v) for v in rng.integers(0, ng + 3, no + 1)], stream=[int(v) for v in rng.integers(0, ns + 2, ng)],
                        off=[int(v) for v in rng.integers(0, 6000, ng)], len=[int(v) for v in rng.integers(0, 4000, ng)])
        cases.append((index, anything, int(rng.integers(1, 5000))))
        cases.append((ix, anything, int(rng.integers(1, 5000))))
    # sources past 4 GiB, as numbers: two rows of 65536 and 3000 bytes whose chunks lie behind position 2^33.  Both rows whole (kept, no edge);
    # a window that cuts both; rows that start past 2^34 decoded bytes, cut; a window inside the first row; a skippable chunk at the second row;
    # the second header inside the first chunk; a position at the end of the source; an edge above 65536 bytes; a tail that is an error; one
    # row, and a total past 4 GiB that no row holds; lo + len wraps; a segment of no bytes of a source with no rows
    G = 1 << 32
    base = dict(n=2 * G + 2 * 65544 + 10, cb=4096, off=0, len=65536 + 3000, total=65536 + 3000, tail=0, rows=2,
                start0=0, pos0=2 * G + 10, kind0=0, size0=4 + 65536, dec0=65536, start1=65536, pos1=2 * G + 10 + 65544, kind1=0, size1=4 + 65536,
                dec1=3000)
    far = {**base, "start0": 4 * G, "start1": 4 * G + 65536, "total": 4 * G + 65536 + 3000, "off": 4 * G + 100, "len": 65536}
    numeric = [base, {**base, "off": 60000, "len": 6000}, far, {**base, "off": 10, "len": 100, "cb": 64}, {**base, "kind1": 1},
               {**base, "pos1": base["pos0"] + 100}, {**base, "pos1": base["n"]}, {**base, "off": 1, "dec0": 65537, "start1": 65537, "total": 65537 + 3000},
               {**base, "tail": O.ERR_CRC_MISMATCH}, {**base, "rows": 1, "total": 5 * G, "len": 5 * G}, {**base, "off": (1 << 64) - 5, "len": 10},
               {**base, "rows": 0, "total": 0, "len": 0}]
    path = str(tmp_path / "cases.bin")
    CM.write_cases(path, streams, cases, numeric)
    exe = str(tmp_path / "frame_compose_plan_check")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host",
                    "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "abi", "frame_compose_plan_check.hip"), "-o", exe,
                    "-Wl,-rpath,/opt/rocm/lib"], check=True)
    env = {**os.environ, "ASAN_OPTIONS": "detect_leaks=1:abort_on_error=0", "UBSAN_OPTIONS": "print_stacktrace=1:halt_on_error=1"}
    run = subprocess.run([exe, path], capture_output=True, text=True, env=env)
    assert run.returncode == 0 and run.stderr == "", run.stderr[-3000:]      # the sanitizers are silent
    lines = run.stdout.splitlines()
    at = passed = refused = 0
    for c, (index, sg, cb) in enumerate(cases):
        for g, w in enumerate(CM.plan_lines(index, streams, sg, cb)):
            assert lines[at] == w, (c, g, cb)
            unsound = c >= nsound and " " in w[2:6]
            passed += unsound and w.startswith("0 ")
            refused += unsound and not w.startswith("0 ")
            at += 1
    assert passed > 50 and refused > 200, (passed, refused)            # both outcomes, on the unsound inputs
    want = [CM.numeric_line(c) for c in numeric]
    assert lines[at:] == want
    # the numbers themselves: status head tail r0 r1 hdec tdec hlen tlen hskip hp tp kept kbytes | edges pieces stage rows bytes bound | ...
    f = [[int(v) for v in w.replace("|", " ").split()] for w in want]
    assert f[0][:5] == [0, 0, 0, 0, 2] and f[0][12:20] == [2, 2 * 65544, 0, 0, 0, 2, 65536 + 3000, 2 * 65544]
    assert f[1][:14] == [0, 1, 1, 0, 2, 65536, 3000, 5536, 464, 60000, 2, 1, 0, 0] and f[1][14:20] == [2, 3, 68536, 3, 6000, 24 + 6000]
    assert f[1][20:27] == [0, 0, 0, 0, 60000, 4096, 0] and f[1][27:34] == [0, 1, 0, 2, 0, 464, 5536]
    assert f[2][:14] == [0, 1, 1, 0, 2, 65536, 3000, 65436, 100, 100, 16, 1, 0, 0] and f[2][33] == 65436
    assert f[3][:14] == [0, 1, 0, 0, 1, 65536, 0, 100, 0, 10, 2, 0, 0, 0] and f[3][27:34] == [0, 0, 0, 1, 74, 36, 64]
    for i in (4, 5, 6, 7, 9, 10):
        assert f[i][0] == O.ERR_BAD_ARG and not any(f[i][1:]), i
    assert f[8][0] == O.ERR_CRC_MISMATCH and f[11] == [0] * 34

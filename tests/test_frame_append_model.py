"""snp_frame_append_indexed_batch (libsnappier_hip_frame_append.so) without a GPU: the declarations and their C# binding, the workspace arithmetic,
argument rejection; the Python model of the contract (frame_append_model.py) checked against the chunked encoder's model, the index model and the
oracle's frame decode at the seam sizes, over sequences of appends and over the named streams; which tails are reopened; corruption in a
reopened tail and before the cut; admission and buf_cap; unsound indexes; and the planning header (csrc/frame_append_device.h) itself, compiled
for the CPU under AddressSanitizer and UBSan into a stand-alone program (tests/abi/frame_append_plan_check.hip) and run over the same cases, over
indexes filled with anything at all and over streams past 4 GiB given as numbers."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import frame_append_model as A
import frame_buffers_model as M
import frame_chunked_model as K
import frame_index_model as X
import frame_range_model as R
import oracle as O
from conftest import ROOT, read_testdata

NAMES = ["snp_frame_append_indexed_batch", "snp_frame_append_indexed_workspace"]
BIG = 1 << 62


def _lib():
    from snappier_amd import _native as N
    return N.frame_append_lib()


# ---- the surface -----------------------------------------------------------------------------------------------------------------------------
def test_header_and_binding_declare_the_new_functions():
    from snappier_amd import _native as N
    declared = N.frame_append_declared_symbols()
    assert sorted(declared) == NAMES
    others = set(N.declared_symbols()) | set(N.buffers_declared_symbols()) | set(N.buffers_decompress_declared_symbols()) | \
        set(N.frame_buffers_declared_symbols()) | set(N.layout_declared_symbols()) | set(N.frame_range_declared_symbols()) | \
        set(N.frame_index_declared_symbols()) | set(N.frame_chunked_declared_symbols()) | set(N.frame_update_declared_symbols())
    assert not set(declared) & others                                  # the other headers' surfaces are left as they are
    lib = _lib()
    assert lib.snp_frame_append_indexed_batch.restype is C.c_int and len(lib.snp_frame_append_indexed_batch.argtypes) == 28
    assert lib.snp_frame_append_indexed_workspace.restype is C.c_uint64 and len(lib.snp_frame_append_indexed_workspace.argtypes) == 4


def test_extension_library_exports_exactly_its_header():
    from layouts import exported
    from snappier_amd import _native as N

    ext = exported(N.FRAME_APPEND_PATH)
    assert ext == set(NAMES)
    for other in (N.PRODUCT_PATH, N.BUFFERS_PATH, N.BUFFERS_DECOMPRESS_PATH, N.FRAME_BUFFERS_PATH, N.LAYOUT_PATH, N.FRAME_RANGE_PATH, N.FRAME_INDEX_PATH,
                  N.FRAME_CHUNKED_PATH, N.FRAME_UPDATE_PATH):
        assert not exported(other) & ext


def test_workspace_is_host_arithmetic():
    ws = _lib().snp_frame_append_indexed_workspace
    assert ws(0, 5, 10, 4096) == 0                                      # nothing when there is no stream
    assert ws(5, 5, 10, 0) == 0 and ws(5, 5, 10, 65537) == 0            # ... or no chunk size the call takes
    for ns in (1, 255, 1025, 300000):
        for mt in (0, 1, 4100, 70000):
            for ms in (0, 1, 33000):
                for cb in (1, 64, 4096, 65536):
                    w = ws(ns, mt, ms, cb)
                    stride = K.stride(cb)
                    assert w % 256 == 0
                    # the raw staging of the tails, the compressed staging of both tables, the two slot tables, the tails' decode rows, the streams' words
                    assert w >= mt * cb + (mt + ms) * stride + (mt + ms) * 36 + mt * 41 + ms * 8 + ns * 112
                    assert w <= mt * cb + (mt + ms) * (stride + 100) + ns * 120 + 60 * 256 + (ns + mt + ms) // 100
                    assert ws(ns + 1, mt, ms, cb) >= w and ws(ns, mt + 1, ms, cb) >= w and ws(ns, mt, ms + 1, cb) >= w
    assert ws(0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF, 65536) > 0xFFFFFFFF * (65536 + 2 * 76496)      # (64-bit arithmetic)


def test_batch_call_rejects_bad_arguments_without_a_device():
    call = _lib().snp_frame_append_indexed_batch
    fake = C.c_void_p(64)                                               # (never dereferenced: the arguments are refused first)
    # ctx; buf, buf_off, buf_len, buf_cap; nstreams; five index arrays; nentries; src, src_off, src_len; chunk_bytes, max_tails, max_slots;
    # new_len, status; five new index arrays; out_bound; d_work, d_result
    def args(ctx=fake, bufs=(fake,) * 4, ns=1, idx=(fake,) * 5, ne=8, srcs=(fake,) * 3, cb=4096, mt=0, ms=0, outs=(fake,) * 2, new=(fake,) * 5,
             bound=None, work=fake, result=fake):
        return (ctx, *bufs, ns, *idx, ne, *srcs, cb, mt, ms, *outs, *new, bound, work, result)

    assert call(*args(ctx=None)) == O.ERR_BAD_ARG
    assert call(*args(result=None)) == O.ERR_BAD_ARG
    assert call(*args(ns=0, result=None)) == O.ERR_BAD_ARG             # an empty call still needs d_result
    assert call(*args(cb=0)) == O.ERR_BAD_ARG and call(*args(cb=65537)) == O.ERR_BAD_ARG
    assert call(*args(ns=0, cb=0)) == O.ERR_BAD_ARG                    # ... also when there is no stream
    assert call(*args(work=None)) == O.ERR_BAD_ARG
    for group, n in (("bufs", 4), ("srcs", 3), ("outs", 2)):
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
        assert call(*args(new=tuple(a), ne=0, ms=1)) == O.ERR_BAD_ARG   # no old rows, room for fresh ones


def test_csharp_binding_matches_the_extension_header():
    import test_csharp_signatures as T
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "snappier_hip_frame_append.h")).read(), flags=re.S)
    protos = {}
    for m in re.finditer(r"([A-Za-z_][A-Za-z0-9_ ]*?[\s\*]+)(snp_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", text):
        params = [re.match(r"(.*?[\s\*])([A-Za-z_][A-Za-z0-9_]*)$", q.strip()).group(1) for q in m.group(3).split(",") if q.strip() not in ("", "void")]
        protos[m.group(2)] = (T.c_class(m.group(1)), [T.c_class(q) for q in params])
    cs = re.sub(r"//.*", "", open(os.path.join(ROOT, "csharp", "Snappier.Gpu", "NativeMethodsFrameAppend.cs")).read())
    assert 'const string Lib = "snappier_hip_frame_append"' in cs
    imps = {}
    for m in re.finditer(r"\[DllImport\(Lib, CallingConvention = Cc\)\]\s*internal static extern ([A-Za-z\*]+) (snp_[a-z0-9_]+)\(([^)]*)\);", cs):
        params = [re.match(r"(.*?)\s+([A-Za-z_][A-Za-z0-9_]*)$", q.strip()).group(1) for q in m.group(3).split(",") if q.strip()]
        imps[m.group(2)] = (T.cs_class(m.group(1)), [T.cs_class(q) for q in params])
    assert set(protos) == set(imps) == set(NAMES)
    for name, (ret, params) in protos.items():
        cret, cparams = imps[name]
        assert T.compatible(ret, cret), (name, ret, cret)
        assert len(params) == len(cparams) and all(T.compatible(a, b) for a, b in zip(params, cparams)), (name, params, cparams)
    assert len(protos["snp_frame_append_indexed_batch"][1]) == 28 and len(protos["snp_frame_append_indexed_workspace"][1]) == 4
    proj = open(os.path.join(ROOT, "csharp", "Snappier.Gpu", "Snappier.Gpu.csproj")).read()
    assert 'Include="../../snappier_amd/libsnappier_hip_frame_append.so"' in proj


# ---- the model -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cb", A.CHUNK_SIZES)
def test_append_equals_the_chunked_encode_of_the_concatenation(cb):
    html = read_testdata("html") * 4
    for variant in (O.HASH_CRC32C, O.HASH_MUL):
        for na in A.a_lengths(cb):
            a = html[7:7 + na]
            streams = [K.stream_of(a, cb, variant)] * len(A.s_lengths(cb))
            srcs = [html[11 + na:11 + na + n] for n in A.s_lengths(cb)]
            ix = X.build_index(streams)
            got = A.append_plan(streams, ix, srcs, cb, variant=variant)
            assert got["status"] == [O.OK] * len(srcs), (cb, na, got["status"])
            for b, s in enumerate(srcs):
                if not s:                                               # (cb = 1: cb - 1 bytes are none) nothing to append, nothing touched
                    assert got["streams"][b] is None and got["new_len"][b] == len(streams[b])
                    continue
                assert got["streams"][b] == K.stream_of(a + s, cb, variant), (cb, na, len(s))
                assert got["new_len"][b] == len(got["streams"][b]) <= got["out_bound"][b]
                assert got["streams"][b][:got["cut"][b]] == streams[b][:got["cut"][b]]
            assert A.same_index(got["index"], X.build_index(A.after(streams, got)))
            tails, slots = A.needs(streams, ix, srcs, cb)
            busy = sum(1 for s in srcs if s)
            assert tails == (busy if 0 < na % cb else 0)
            assert got["result"] == [slots, sum(got["new_len"]) - sum(map(len, streams)), tails, busy]


def test_three_appends_in_a_row_equal_the_encode_of_the_concatenation():
    html = read_testdata("html") * 4
    for cb, parts in ((100, (250, 30, 20, 331)), (4096, (0, 1, 4095, 9000)), (65536, (70000, 1, 65535, 5)), (1, (0, 3, 2, 1))):
        blobs = [html[9:9 + parts[0]], html[:parts[0] // 2]]
        streams = [K.stream_of(x, cb) for x in blobs]
        ix = X.build_index(streams)
        at = 1000
        for n in parts[1:]:
            srcs = [html[at:at + n], html[at + 7:at + 7 + 2 * n]]
            got = A.append_plan(streams, ix, srcs, cb)
            assert got["status"] == [O.OK, O.OK]
            streams, ix = got["streams"], got["index"]                  # the new index goes straight into the next call
            blobs = [x + s for x, s in zip(blobs, srcs)]
            at += 3 * n
        assert streams == [K.stream_of(x, cb) for x in blobs]
        assert A.same_index(ix, X.build_index(streams))


@pytest.fixture(scope="module")
def named():
    cases = X.named_streams()
    streams = list(cases.values())
    return list(cases), streams, X.build_index(streams)


def test_named_streams_append_as_the_contract_says(named):
    names, streams, ix = named
    html = read_testdata("html")
    cb = 4096
    srcs = [html[b:b + 5000 + 13 * b] for b in range(len(streams))]
    got = A.append_plan(streams, ix, srcs, cb)
    written = sick = 0
    for b, s in enumerate(streams):
        if ix["tail"][b] == O.OK:                                       # appended, and it decodes to old || S by the oracle's frame decode
            assert got["status"][b] == O.OK, names[b]
            try:
                old = O.frame_decode(s)
            except O.OracleError:                                       # (a corrupt chunk before the cut: not noticed, and it stays)
                old = None
                sick += 1
            if old is not None:
                assert O.frame_decode(got["streams"][b]) == old + srcs[b], names[b]
            assert got["streams"][b][:got["cut"][b]] == s[:got["cut"][b]] and got["cut"][b] <= len(s)
            written += 1
        else:                                                           # a broken stream keeps every byte and gets the walk's status
            assert got["status"][b] == ix["tail"][b] and got["streams"][b] is None and got["new_len"][b] == len(s), names[b]
    assert A.same_index(got["index"], X.build_index(A.after(streams, got)))
    assert got["result"][3] == written and sick < written // 2
    # both outcomes, and several statuses: the floor the GPU test asserts on the same batch
    assert written >= 10 and len(streams) - written >= 5 and len(set(got["status"])) >= 4, (written, len(streams), set(got["status"]))


def test_only_a_short_tail_that_is_physically_last_is_reopened():
    html = read_testdata("html")
    cb = 1000
    shapes = A.tail_shapes(html, cb)
    streams = [s for s, _ in shapes.values()]
    ix = X.build_index(streams)
    src = html[5000:5000 + 2 * cb + 17]
    got = A.append_plan(streams, ix, [src] * len(streams), cb)
    assert got["status"] == [O.OK] * len(streams)
    for b, (name, (s, reopened)) in enumerate(shapes.items()):
        assert (got["cut"][b] < len(s)) == reopened, name
        if not reopened:
            assert got["cut"][b] == len(s) and got["streams"][b][:len(s)] == s, name
        assert O.frame_decode(got["streams"][b]) == O.frame_decode(s) + src, name
    assert got["streams"][list(shapes).index("empty")] == K.stream_of(src, cb)       # the identifier first
    assert got["result"][2] == sum(r for _, r in shapes.values()) == 2
    assert A.same_index(got["index"], X.build_index(got["streams"]))
    # a source no longer than the room in the tail: one chunk, no fresh slot
    small = A.append_plan(streams[:1], X.build_index(streams[:1]), [src[:cb // 2]], cb)
    assert small["result"] == [0, small["new_len"][0] - len(streams[0]), 1, 1] and small["streams"][0] == K.stream_of(html[:2 * cb + cb // 2] + src[:cb // 2], cb)


def test_a_corrupt_reopened_tail_is_noticed_and_corruption_before_the_cut_is_not():
    html = read_testdata("html")
    cb = 4096
    raw = html[:3 * cb + 100]
    s = K.stream_of(raw, cb)
    rows = R.walk(s)[0]
    src = html[20000:20000 + cb]
    bad_tail, bad_early = R.corrupt_chunk(s, rows[3]), R.corrupt_chunk(s, rows[1])
    ix = X.build_index([s])
    assert ix == X.build_index([bad_tail]) == X.build_index([bad_early])
    want = M.chunk_status(bad_tail, rows[3])
    assert want != O.OK
    got = A.append_plan([bad_tail, bad_early, s], X.build_index([s] * 3), [src] * 3, cb)
    assert got["status"] == [want, O.OK, O.OK] and got["streams"][0] is None and got["new_len"][0] == len(s) and got["out_bound"][0] == len(s)
    assert got["streams"][1][:got["cut"][1]] == bad_early[:got["cut"][1]] and got["streams"][1][got["cut"][1]:] == got["streams"][2][got["cut"][2]:]
    assert got["result"] == [3, 2 * (got["new_len"][2] - len(s)), 3, 2]      # (the failing tail was admitted: it took its slots)
    full = A.append_plan([K.stream_of(raw[:3 * cb], cb)[:-1] + b"\x00"], X.build_index([K.stream_of(raw[:3 * cb], cb)]), [src], cb)
    assert full["status"] == [O.OK]                                     # a corrupt full tail is not reopened, so it is not looked at


def test_admission_is_in_stream_order_by_each_bound_and_buf_cap_hits_one_stream():
    html = read_testdata("html")
    cb = 512
    blobs = [html[:700], html[50:50 + 1024], html[9:9 + 1300], html[:100], b""]
    streams = [K.stream_of(x, cb) for x in blobs]
    ix = X.build_index(streams)
    srcs = [html[3000:3000 + n] for n in (1000, 513, 100, 0, 2000)]
    full = A.append_plan(streams, ix, srcs, cb)
    tails, slots = full["result"][2], full["result"][0]
    assert full["status"] == [O.OK] * 5 and (tails, slots) == (2, 2 + 2 + 0 + 0 + 4)
    assert A.append_plan(streams, ix, srcs, cb, max_tails=tails, max_slots=slots) == full
    short = A.append_plan(streams, ix, srcs, cb, max_tails=tails, max_slots=slots - 1)
    assert short["status"] == [O.OK, O.OK, O.OK, O.OK, O.ERR_OUTPUT_TOO_SMALL] and short["streams"][:3] == full["streams"][:3]
    short = A.append_plan(streams, ix, srcs, cb, max_tails=tails - 1, max_slots=slots)
    assert short["status"] == [O.OK, O.OK, O.ERR_OUTPUT_TOO_SMALL, O.OK, O.ERR_OUTPUT_TOO_SMALL]      # the stream that misses, every later appended one; an empty append is OK
    assert short["result"] == [slots, short["new_len"][0] + short["new_len"][1] - len(streams[0]) - len(streams[1]), tails, 2]
    assert short["index"]["total"] == [700 + 1000, 1024 + 513, 1300, 100, 0] and short["index"]["tail"] == [0] * 5
    none = A.append_plan(streams, ix, srcs, cb, max_tails=0, max_slots=slots)
    assert none["status"] == [O.ERR_OUTPUT_TOO_SMALL] * 3 + [O.OK, O.ERR_OUTPUT_TOO_SMALL] and none["streams"] == [None] * 5
    sizing = A.append_plan(streams, ix, srcs, cb, caps=[0] * 5, max_tails=0, max_slots=0)
    assert sizing["result"] == [slots, 0, tails, 0] and sizing["out_bound"] == full["out_bound"]
    assert all(b >= n for b, n in zip(sizing["out_bound"], full["new_len"])) and A.same_index(sizing["index"], ix)
    caps = list(full["new_len"])
    caps[1] -= 1                                                        # one byte short, in the middle
    mid = A.append_plan(streams, ix, srcs, cb, caps=caps)
    assert mid["status"] == [O.OK, O.ERR_OUTPUT_TOO_SMALL, O.OK, O.OK, O.OK] and mid["streams"][1] is None and mid["new_len"][1] == len(streams[1])
    assert A.same_index(mid["index"], X.build_index(A.after(streams, mid)))
    assert mid["result"] == [slots, sum(mid["new_len"]) - sum(map(len, streams)), tails, 3]


def test_verdicts_of_the_index():
    html = read_testdata("html")
    cb = 1000
    streams = [K.stream_of(html[:n], cb) for n in (2500, 2000, 300)] + [R.uniform_stream(3, 1)[0][:-5]]
    ix = X.build_index(streams)
    assert ix["tail"][3] == O.ERR_TRUNCATED_STREAM
    src = [html[:700]] * 4

    def statuses(**change):
        return A.append_plan(streams, {**ix, **change}, src, cb)["status"]

    assert statuses() == [O.OK, O.OK, O.OK, O.ERR_TRUNCATED_STREAM]
    assert statuses(tail=[O.ERR_OUTPUT_TOO_SMALL, 0, 77, -1]) == [O.ERR_OUTPUT_TOO_SMALL, O.OK, O.ERR_BAD_ARG, O.ERR_BAD_ARG]
    assert statuses(total=[2501, 2000, 299, 0])[:3] == [O.ERR_BAD_ARG, O.OK, O.ERR_BAD_ARG]        # the tail does not decode to d bytes
    assert statuses(total=[A.U64, 2000, 300, 0])[0] == O.ERR_BAD_ARG            # total + src_len wraps
    assert statuses(pos=[p + 1 for p in ix["pos"]])[:3] == [O.ERR_BAD_ARG] * 3
    assert statuses(first=[0, 0, 5, 6, 6])[:2] == [O.ERR_BAD_ARG, O.OK]                            # decoded bytes and no row; the next stream's rows are its own
    assert A.append_plan(streams, {**ix, "tail": [5, 77, -3, 9]}, [b""] * 4, cb)["status"] == [O.OK] * 4      # nothing to append: nothing is looked at


def test_unsound_indexes_get_the_models_verdicts(named):
    names, streams, ix = named
    rng = np.random.default_rng(5)
    html = read_testdata("html")
    srcs = [html[b:b + 3000] for b in range(len(streams))]
    sound = A.append_plan(streams, ix, srcs, 4096)
    refused = kept = 0
    for bad in A.unsound_indexes(ix, streams, rng):
        got = A.append_plan(streams, bad, srcs, 4096, max_tails=len(streams), max_slots=2 * len(streams))
        ne = min(len(bad["start"]), len(bad["pos"]))
        assert len(got["index"]["start"]) == len(got["index"]["pos"]) <= ne + 2 * len(streams)
        assert got["index"]["first"][-1] == len(got["index"]["start"]) and got["index"]["first"] == sorted(got["index"]["first"])
        for b, s in enumerate(streams):
            if got["streams"][b] is None:
                assert got["new_len"][b] == len(s)
                refused += got["status"][b] != sound["status"][b]
            else:                                                       # whatever passed the check of its last row is appended to soundly
                assert got["streams"][b][:got["cut"][b]] == s[:got["cut"][b]] and got["cut"][b] <= len(s)
                kept += 1
    assert refused > 40 and kept > 20, (refused, kept)


# ---- the planning header on the CPU, under sanitizers ------------------------------------------------------------------------------------------
def test_planning_header_under_sanitizers_matches_the_model(named, tmp_path):
    names, streams, ix = named
    html = read_testdata("html")
    shapes = A.tail_shapes(html, 1000)
    streams = streams + [s for s, _ in shapes.values()]
    ix = X.build_index(streams)
    ns = len(streams)
    rng = np.random.default_rng(11)
    lens = [[int(v) for v in rng.integers(0, 200000, ns)], [1] * ns, [0] * ns, [65536 * 3 + 1] * ns, [(1 << 32) + 5 + b for b in range(ns)],
            [A.U64 - b for b in range(ns)]]
    cases = [(ix, cb, ln) for cb in (1, 1000, 4096, 65536) for ln in lens]
    cases += [(bad, cb, lens[0]) for bad in A.unsound_indexes(ix, streams, rng) for cb in (1000, 65536)]
    # streams past 4 GiB, as numbers: a short tail that is last (reopened), one followed by more bytes, a full one, a skippable chunk at the row,
    # a position at the end, an appended length past 4 GiB, a total that wraps
    G = 1 << 32
    base = dict(n=G + 200_000, src_len=100_000, cb=65536, total=3 * G + 140_000, start=3 * G + 131_072, pos=G + 200_000 - 4 - 4 - 8928, tail=0, rows=1,
                kind=0, size=4 + 8928, dec=8928)
    numeric = [base, {**base, "n": base["n"] + 9}, {**base, "start": base["total"] - 65536, "dec": 65536, "size": 65540, "pos": base["n"] - 65544},
               {**base, "kind": 1}, {**base, "pos": base["n"]}, {**base, "src_len": 5 * G + 3}, {**base, "src_len": A.U64 - base["total"] + 1},
               {**base, "cb": 1, "src_len": 2 * G + 1}, {**base, "rows": 0}, {**base, "rows": 0, "total": 0, "n": 0, "src_len": G + 1},
               {**base, "tail": O.ERR_CRC_MISMATCH}, {**base, "dec": 8927}, {**base, "start": base["total"] + 1}]
    path = str(tmp_path / "cases.bin")
    A.write_cases(path, streams, cases, numeric)
    exe = str(tmp_path / "frame_append_plan_check")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host",
                    "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "abi", "frame_append_plan_check.hip"), "-o", exe,
                    "-Wl,-rpath,/opt/rocm/lib"], check=True)
    env = {**os.environ, "ASAN_OPTIONS": "detect_leaks=1:abort_on_error=0", "UBSAN_OPTIONS": "print_stacktrace=1:halt_on_error=1"}
    run = subprocess.run([exe, path], capture_output=True, text=True, env=env)
    assert run.returncode == 0 and run.stderr == "", run.stderr[-3000:]      # the sanitizers are silent
    lines = run.stdout.splitlines()
    assert len(lines) == ns * len(cases) + len(numeric)
    at = passed = refused = 0
    for c, (index, cb, ln) in enumerate(cases):
        for b, w in enumerate(A.plan_lines(index, streams, ln, cb)):
            assert lines[at] == w, (c, b, cb, ln[b])
            unsound = c >= 4 * len(lens)
            passed += unsound and w.startswith("0 1 ")
            refused += unsound and not w.startswith("0 ")
            at += 1
    assert passed > 50 and refused > 200, (passed, refused)            # both outcomes, on the unsound indexes
    want = [A.numeric_line(c) for c in numeric]
    assert lines[at:] == want
    # the numbers themselves: the reopened tail past 4 GiB, its fill, its fresh slots; a length past 4 GiB at one byte per chunk
    first = want[0].split()
    assert first[:6] == ["0", "1", "1", "0", "8928", str(65536 - 8928)] and int(first[8]) == base["pos"] > G and int(first[10]) == 1
    assert want[1].split()[2] == "0" and want[2].split()[2] == "0" and want[3].split()[0] == str(O.ERR_BAD_ARG) and want[4].split()[0] == str(O.ERR_BAD_ARG)
    assert int(want[5].split()[10]) == (5 * G + 3 - (65536 - 8928) + 65535) // 65536 and want[6].split()[0] == str(O.ERR_BAD_ARG)
    assert int(want[7].split()[10]) == 2 * G + 1 and want[7].split()[2] == "0"
    assert want[8].split()[0] == str(O.ERR_BAD_ARG) and want[9].split()[:4] == ["0", "1", "0", "1"] and want[10].split()[0] == str(O.ERR_CRC_MISMATCH)
    assert want[11].split()[0] == str(O.ERR_BAD_ARG) and want[12].split()[0] == str(O.ERR_BAD_ARG)

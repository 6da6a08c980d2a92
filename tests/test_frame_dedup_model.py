"""libsnappier_hip_frame_dedup.so without a GPU: the declarations and their C# binding, argument rejection, the workspace arithmetic; the model
of the call (frame_dedup_model.py) against an independent brute-force statement -- every chunk decoded with the oracle, grouped by content and
by chunk bytes --, its recipes through the compose model back to the original streams, admission at every bound, the forged CRC collisions
against the oracle's CRC; and the rule header (csrc/frame_dedup_device.h) itself, compiled for the CPU under AddressSanitizer and UBSan into a
stand-alone program (tests/abi/frame_dedup_plan_check.hip) and run over cases the model writes out."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import frame_buffers_model as M
import frame_compose_model as CM
import frame_dedup_model as D
import frame_index_model as X
import oracle as O
from conftest import ROOT, read_testdata

NAMES = ["snp_frame_dedup_indexed_batch", "snp_frame_dedup_indexed_workspace"]


def _lib():
    from snappier_amd import _native as N
    return N.frame_dedup_lib()


_lib()                                                                  # every test here is about this library: without it the module does not load


@pytest.fixture(scope="module")
def html():
    return read_testdata("html")


@pytest.fixture(scope="module")
def versions(html):
    """html and an edited copy (1 001 bytes inserted at one third), content-defined at window 64: -> (raws, streams, index)."""
    at = len(html) // 3
    raws = [html, html[:at] + bytes(np.random.default_rng(11).integers(0, 256, 1001, dtype=np.uint8)) + html[at:]]
    streams = D.content_defined(raws, 64, 1024)
    return raws, streams, X.build_index(streams)


# ---- the surface -----------------------------------------------------------------------------------------------------------------------------
def test_header_binding_and_library_declare_the_new_functions():
    from layouts import exported
    from snappier_amd import _native as N
    import snappier_amd as S
    assert N.frame_dedup_declared_symbols() == NAMES
    others = set(N.declared_symbols())
    for name in N._EXTENSIONS:
        if name != "frame_dedup":
            others |= set(N.declared_symbols(N._extension_header(name)))
            assert not exported(N._extension_path(name)) & set(NAMES)
    assert not set(NAMES) & others                                      # the other headers' surfaces are left as they are
    assert exported(N.FRAME_DEDUP_PATH) == set(NAMES) and not exported(N.PRODUCT_PATH) & set(NAMES)
    lib = _lib()
    assert lib.snp_frame_dedup_indexed_batch.restype is C.c_int and len(lib.snp_frame_dedup_indexed_batch.argtypes) == 30
    assert S.DEDUP_NONE == D.NONE == (1 << 64) - 1
    text = open(os.path.join(ROOT, "include", "snappier_hip_frame_dedup.h")).read()
    assert re.search(r"#define SNP_DEDUP_NONE 0xffffffffffffffffull", text)


def test_csharp_binding_matches_the_extension_header():
    import test_csharp_signatures as T
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "snappier_hip_frame_dedup.h")).read(), flags=re.S)
    protos = {}
    for m in re.finditer(r"([A-Za-z_][A-Za-z0-9_ ]*?[\s\*]+)(snp_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", text):
        params = [re.match(r"(.*?[\s\*])([A-Za-z_][A-Za-z0-9_]*)$", q.strip()).group(1) for q in m.group(3).split(",") if q.strip() not in ("", "void")]
        protos[m.group(2)] = (T.c_class(m.group(1)), [T.c_class(q) for q in params])
    cs = re.sub(r"//.*", "", open(os.path.join(ROOT, "csharp", "Snappier.Gpu", "NativeMethodsFrameDedup.cs")).read())
    assert 'const string Lib = "snappier_hip_frame_dedup"' in cs
    imps = {}
    for m in re.finditer(r"\[DllImport\(Lib, CallingConvention = Cc\)\]\s*internal static extern ([A-Za-z\*]+) (snp_[a-z0-9_]+)\(([^)]*)\);", cs):
        params = [re.match(r"(.*?)\s+([A-Za-z_][A-Za-z0-9_]*)$", q.strip()).group(1) for q in m.group(3).split(",") if q.strip()]
        imps[m.group(2)] = (T.cs_class(m.group(1)), [T.cs_class(q) for q in params])
    assert set(protos) == set(imps) == set(NAMES)
    for name, (ret, params) in protos.items():
        cret, cparams = imps[name]
        assert T.compatible(ret, cret), (name, ret, cret)
        assert len(params) == len(cparams) and all(T.compatible(a, b) for a, b in zip(params, cparams)), (name, params, cparams)
    assert [len(protos[n][1]) for n in NAMES] == [30, 2]
    proj = open(os.path.join(ROOT, "csharp", "Snappier.Gpu", "Snappier.Gpu.csproj")).read()
    assert 'Include="../../snappier_amd/libsnappier_hip_frame_dedup.so"' in proj


def test_workspace_is_host_arithmetic_within_the_documented_bound():
    ws = _lib().snp_frame_dedup_indexed_workspace
    assert ws(0, 1000) == 0 and ws(1, 1 << 31) == 0 and ws(1, 1 << 40) == 0
    for ns in (1, 2, 1000, 163840):
        for ne in (0, 1, 31, 32, 33, 5000, 40000, (1 << 20) + 1, (1 << 31) - 1):
            size = ws(ns, ne)
            slots = D.slots_of(ne)
            assert slots >= 64 and slots >= 2 * ne and (ne <= 32 or slots < 4 * ne) and slots & (slots - 1) == 0
            assert size % 256 == 0 and ws(ns + 1, ne) >= size and ws(ns, min(ne + 1, (1 << 31) - 1)) >= size
            assert 80 * ne + 12 * slots + 36 * ns <= size <= 80 * ne + 12 * slots + 36 * ns + 8 * (ns + ne) // 1024 + 24 * 256 + 64


def test_batch_call_rejects_bad_arguments_without_a_device():
    call = _lib().snp_frame_dedup_indexed_batch
    fake = C.c_void_p(64)                                               # (never dereferenced: the arguments are refused first)

    def args(ns=1, ne=4, nbase=0, me=4, ms=4, cap=100, null=(), ctx=fake, result=fake):
        # in, in_off, in_len | idx_first, idx_start, idx_pos, idx_total, idx_tail | out, out_len, status, canon, pk_first, pk_start, pk_pos,
        # pk_total, pk_tail, seg_first, seg_stream, seg_off, seg_len, d_work
        p = [None if i in null else fake for i in range(22)]
        return (ctx, *p[:3], ns, *p[3:8], ne, nbase, me, ms, cap, *p[8:22], result)

    assert call(*args(ctx=None)) == O.ERR_BAD_ARG
    assert call(*args(result=None)) == O.ERR_BAD_ARG
    assert call(*args(ns=0, ne=0, null=range(22), result=None)) == O.ERR_BAD_ARG
    assert call(*args(ns=1, nbase=2)) == O.ERR_BAD_ARG                  # more base streams than streams
    assert call(*args(ns=0, nbase=1, null=range(22))) == O.ERR_BAD_ARG
    assert call(*args(ns=1 << 31)) == O.ERR_BAD_ARG
    assert call(*args(ne=1 << 31)) == O.ERR_BAD_ARG
    for i in range(22):                                                 # any one null among the arrays of a full call
        assert call(*args(null=(i,))) == O.ERR_BAD_ARG, i


# ---- the model against brute force ---------------------------------------------------------------------------------------------------------------
def brute_force(streams, nbase):
    """Every data chunk of every stream (all of them sound here) decoded with the oracle: -> per row (stream, content, chunk bytes)."""
    rows = []
    for b, s in enumerate(streams):
        ip = 0
        while ip < len(s):
            h = M.hop(s, ip)
            assert h.kind in ("data", "skip")
            if h.kind == "data":
                body = s[ip + 8:h.next]
                raw = O.decompress(body) if h.type == 0 else body
                assert O.crc32c(raw, masked=True) == h.crc
                rows.append((b, raw, s[ip:h.next]))
            ip = h.next
    return rows


def check_against_brute_force(streams, nbase, got):
    rows = brute_force(streams, nbase)
    canon = got["canon"]
    assert len(canon) == len(rows)
    by_bytes = {}
    for r, (b, raw, chunk) in enumerate(rows):
        if not raw:
            assert canon[r] == D.NONE
            continue
        c = canon[r]
        assert c <= r and rows[c][2] == chunk and canon[c] == c        # a row is only ever mapped to the same bytes, and to a fixed point
        first = by_bytes.setdefault(chunk, r)
        # merged exactly when an earlier row has the same bytes -- unless that row lost its key to other content (never in these cases:
        # the caller says so through [6] == 0) -- and then into the first such row
        if got["result"][6] == 0:
            assert c == first, r
    # the pack: the unique chunks of the new streams, in row order; every new stream back from its recipe
    new_rows = [r for r, (b, raw, _) in enumerate(rows) if b >= nbase and raw]
    assert got["pack"] == M.STREAM_ID + b"".join(rows[r][2] for r in new_rows if canon[r] == r)
    assert got["result"][4] == len(new_rows) and got["result"][0] == sum(1 for r in new_rows if canon[r] == r)
    assert got["result"][5] == sum(1 for r in new_rows if canon[r] != r)
    assert got["result"][7] == sum(len(rows[r][2]) for r in new_rows if canon[r] != r)
    assert got["result"][1] == len(got["pack"])


def restored(streams, ix, nbase, got, cb=65536):
    """The recipes through the compose model: -> the new streams again, and how many rows were kept."""
    src, six = D.sources(streams, ix, nbase, got["pack"], got["index"])
    back = CM.compose_plan(src, six, got["segs"], cb)
    assert back["status"] == [O.OK] * (len(streams) - nbase)
    assert back["result"][0] == 0 and back["result"][2] == 0            # no edge, no piece: nothing decoded on the way
    return back["streams"], back["result"][5]


def test_model_against_brute_force_and_through_compose(html):
    rng = np.random.default_rng(21)
    for name, (streams, nbase) in D.run_cases(rng).items():
        ix = X.build_index(streams)
        got = D.dedup_plan(streams, ix, nbase)
        assert got["result"][6] == 0
        check_against_brute_force(streams, nbase, got)
        assert X.build_index([got["pack"]])["start"] == got["index"]["start"] and X.build_index([got["pack"]])["pos"] == got["index"]["pos"]
        back, kept = restored(streams, ix, nbase, got)
        assert back == streams[nbase:], name
        assert kept == got["result"][4]
    want = {"all_unique_is_one_segment": [1], "abab": [2], "run_continues_from_the_previous_stream": [1, 2], "run_passes_from_base_into_pack": [2],
            "duplicate_of_the_middle_of_a_base_stream": [4], "base_only": []}
    for name, (streams, nbase) in D.run_cases(np.random.default_rng(21)).items():
        f = D.dedup_plan(streams, X.build_index(streams), nbase)["segs"]["first"]
        assert [b - a for a, b in zip(f, f[1:])] == want[name], name


def test_pack_index_is_the_index_call_s(versions):
    raws, streams, ix = versions
    got = D.dedup_plan(streams, ix)
    px = X.build_index([got["pack"]])
    for key in ("first", "start", "pos", "total", "tail"):
        assert px[key] == got["index"][key], key


def test_end_to_end_on_versions_of_html(versions):
    raws, streams, ix = versions
    got = D.dedup_plan(streams, ix)
    assert got["status"] == [O.OK, O.OK] and got["result"][6] == 0
    assert len(got["pack"]) < 0.6 * (len(streams[0]) + len(streams[1]))  # the input stays under the cap the GPU test asserts
    check_against_brute_force(streams, 0, got)
    back, kept = restored(streams, ix, 0, got, cb=4096)
    assert back == streams and kept == got["result"][4]
    assert [O.frame_decode(s) for s in back] == raws
    # incremental: version 1 alone, then version 2 against pack 1 as the base
    one = D.dedup_plan(streams[:1], X.build_index(streams[:1]))
    assert len(one["pack"]) <= len(streams[0]) and restored(streams[:1], X.build_index(streams[:1]), 0, one)[0] == streams[:1]
    both = [one["pack"], streams[1]]
    bix = X.build_index(both)
    two = D.dedup_plan(both, bix, 1)
    assert two["status"] == [O.OK, O.OK] and len(one["pack"]) + len(two["pack"]) == len(got["pack"]) + 10
    back, _ = restored(both, bix, 1, two)
    assert back == [streams[1]]


def test_foreign_streams_zero_length_rows_and_skippable_chunks(html):
    streams = D.foreign_streams(html)
    ix = X.build_index(streams)
    got = D.dedup_plan(streams, ix)
    assert got["status"] == [O.OK] * 3 and got["result"][4] == 8 and got["result"][0] == 3 and got["result"][6] == 0
    check_against_brute_force(streams, 0, got)
    back, _ = restored(streams, ix, 0, got)
    assert [O.frame_decode(s) for s in back] == [O.frame_decode(s) for s in streams]
    assert back[0] != streams[0]                                        # everything that is no non-empty data chunk is dropped


def test_a_failed_stream_offers_no_row_and_the_next_one_leads(html):
    a, b = M.data_chunk(html[:900]), M.data_chunk(html[900:2000])
    streams = [D.stream_of_chunks([a, b]), D.stream_of_chunks([b, a]), D.stream_of_chunks([a, b])]
    ix = X.build_index(streams)
    for name, bad in D.unsound_indexes(ix, streams, np.random.default_rng(2)).items():
        got = D.dedup_plan(streams, bad)
        ne = D.nentries_of(bad)
        for s, st in enumerate(got["status"]):
            f0, f1 = min(bad["first"][s], ne), min(bad["first"][s + 1], ne)
            if st != O.OK:
                assert got["segs"]["first"][s] == got["segs"]["first"][s + 1], name
        owned = set()
        for s, st in enumerate(got["status"]):
            if st == O.OK:
                rows = set(range(min(bad["first"][s], ne), min(bad["first"][s + 1], ne)))
                assert not rows & owned, name                           # streams that passed share no row
                owned |= rows
        assert all((c == D.NONE) == (r not in owned) for r, c in enumerate(got["canon"])), name
        assert all(c == D.NONE or (c in owned and c <= r) for r, c in enumerate(got["canon"])), name
    got = D.dedup_plan(streams, D.unsound_indexes(ix, streams, np.random.default_rng(2))["a_tail_that_is_not_ok"])
    assert got["status"] == [O.ERR_CRC_MISMATCH, O.OK, O.OK] and got["canon"] == [D.NONE, D.NONE, 2, 3, 3, 2]
    # a corrupt header fails its stream alone
    broken = bytearray(streams[0])
    broken[10] = 0x02
    got = D.dedup_plan([bytes(broken)] + streams[1:], ix)
    assert got["status"] == [O.ERR_BAD_ARG, O.OK, O.OK] and got["canon"] == [D.NONE, D.NONE, 2, 3, 3, 2]


def test_forged_collisions_and_the_leader_rule(html):
    a = html[:600]
    b = D.forge_collision(a, at=5, flip=0x40)
    assert a != b and len(a) == len(b) and O.crc32c(a) == O.crc32c(b) and O.crc32c(a, masked=True) == O.crc32c(b, masked=True)
    for n in (5, 6, 64, 65536):
        x = bytes(np.random.default_rng(n).integers(0, 256, n, dtype=np.uint8))
        for at in {0, (n - 5) // 2, n - 5}:
            y = D.forge_collision(x, at, 0x81)
            assert x != y and len(y) == n and O.crc32c(x) == O.crc32c(y)
    A, B = D.raw_chunk(a), D.raw_chunk(b)
    assert A[:8] == B[:8] and A != B                                    # the same header and CRC field, another payload
    for order, canon, coll in (([A, B, B], [0, 1, 2], 2), ([B, A, B], [0, 1, 0], 1)):
        for streams in ([D.stream_of_chunks(order)], [D.stream_of_chunks([c]) for c in order]):
            got = D.dedup_plan(streams, X.build_index(streams))
            assert got["canon"] == canon and got["result"][6] == coll and got["result"][5] == 3 - len(set(canon))
            back, _ = restored(streams, X.build_index(streams), 0, got)
            assert back == streams
    # the same content in another encoding: the same key, never merged
    comp, plain = M.data_chunk(a), D.raw_chunk(a)
    streams = [D.stream_of_chunks([comp, plain, comp])]
    got = D.dedup_plan(streams, X.build_index(streams))
    assert got["canon"] == [0, 1, 0] and got["result"][6] == 1


def test_admission_in_stream_order_at_every_bound(html):
    rng = np.random.default_rng(4)
    chunks = [M.data_chunk(bytes(rng.integers(0, 256, int(n), dtype=np.uint8))) for n in rng.integers(50, 400, 9)]
    streams = [D.stream_of_chunks([chunks[0], chunks[1], chunks[2]]), D.stream_of_chunks([chunks[1], chunks[3], chunks[0], chunks[4]]),
               D.stream_of_chunks([chunks[5], chunks[3], chunks[6], chunks[7]])]
    ix = X.build_index(streams)
    free = D.dedup_plan(streams, ix)
    me, ms, cap = D.needs(streams, ix)
    assert (me, ms, cap) == (free["result"][0], free["result"][2], free["result"][1]) == (8, 8, len(free["pack"]))
    exact = D.dedup_plan(streams, ix, 0, me, ms, cap)
    assert exact == free
    per = [D.dedup_plan(streams[:k + 1], X.build_index(streams[:k + 1]))["result"][:3] for k in range(3)]
    for bound in range(3):
        for miss in range(3):
            b = [me, cap, ms]
            b[bound] = per[miss][bound] - 1                             # stream `miss` is the first that does not fit
            got = D.dedup_plan(streams, ix, 0, b[0], b[2], b[1])
            assert got["status"] == [O.OK] * miss + [O.ERR_OUTPUT_TOO_SMALL] * (3 - miss), (bound, miss)
            assert got["canon"] == free["canon"] and got["result"][:3] == free["result"][:3] and got["result"][3] == miss
            assert got["segs"]["first"] == free["segs"]["first"][:miss + 1] + [free["segs"]["first"][miss]] * (3 - miss)
            if got["pack"] is not None:
                assert free["pack"].startswith(got["pack"]) and X.build_index([got["pack"]])["pos"] == got["index"]["pos"]
    sizing = D.dedup_plan(streams, ix, 0, 0, 0, 0)
    assert sizing["pack"] is None and sizing["out_len"] == 0 and sizing["canon"] == free["canon"] and sizing["index"]["tail"] == [O.ERR_OUTPUT_TOO_SMALL]
    empty = D.dedup_plan([], dict(first=[0], start=[], pos=[], total=[], tail=[]))
    assert empty["pack"] == M.STREAM_ID and empty["result"] == [0, 10, 0, 0, 0, 0, 0, 0]
    base = D.dedup_plan(streams, ix, 3)
    assert base["pack"] == M.STREAM_ID and base["segs"]["first"] == [0] and base["canon"] == free["canon"] and base["result"][3] == 3


# ---- the rule header on the CPU ------------------------------------------------------------------------------------------------------------------
def test_device_header_under_sanitizers_against_brute_force(html, tmp_path):
    keys = [(1, 0, 0), (65536, 0xFFFFFFFF, 1), (0x7FFFFFFF, 0x12345678, 31), (1000, 0xA282EAD8, 32), (1000, 0xA282EAD9, 33), (4096, 7, 5000),
            (4096, 8, (1 << 31) - 1), (17, 0xDEADBEEF, 1 << 20)]
    runs = [(1, 0, 1, 5, 9, 0, 0, 0), (0, 0, 1, 100, 9, 0, 40, 60), (0, 0, 1, 100, 9, 0, 40, 59), (0, 2, 1, 100, 70, 1, 30, 40),
            (0, 2, 1, 100, 70, 0, 30, 40), (0, 3, 3, 100, 70, 3, 70, 0), (0, 1, 5, (1 << 40) + 7, 3, 1, (1 << 40), 7),
            (0, 1, 5, 6, 3, 1, D.U64, 7), (0, 9, 5, 6, 1 << 33, 5, (1 << 33) - 9, 9)]
    a, b, c = M.data_chunk(html[:900]), M.data_chunk(html[900:2000]), M.data_chunk(b"", compressed=False)
    streams = [D.stream_of_chunks([a, b, c]), D.stream_of_chunks([b, M.chunk(0x80, b"skip"), a]), D.stream_of_chunks([a, c, c, b])] + \
        D.foreign_streams(html)
    ix = X.build_index(streams)
    rng = np.random.default_rng(13)
    indexes = [ix] + list(D.unsound_indexes(ix, streams, rng).values())
    for _ in range(30):                                                 # one word of a sound index replaced by another value near it, or by anything
        k = {key: list(v) for key, v in ix.items() if key != "result"}
        key = ("first", "start", "pos", "total", "tail")[int(rng.integers(0, 5))]
        i = int(rng.integers(0, len(k[key])))
        k[key][i] = int(rng.integers(0, 12)) if key == "tail" else max(0, k[key][i] + int(rng.integers(-3, 4))) if rng.integers(0, 2) else int(rng.integers(0, 1 << 62))
        indexes.append(k)
    path = str(tmp_path / "cases.bin")
    D.write_cases(path, keys, runs, streams, indexes)
    exe = str(tmp_path / "frame_dedup_plan_check")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host",
                    "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "abi", "frame_dedup_plan_check.hip"), "-o", exe,
                    "-Wl,-rpath,/opt/rocm/lib"], check=True)
    env = {**os.environ, "ASAN_OPTIONS": "detect_leaks=1:abort_on_error=0", "UBSAN_OPTIONS": "print_stacktrace=1:halt_on_error=1"}
    run = subprocess.run([exe, path], capture_output=True, text=True, env=env)
    assert run.returncode == 0 and run.stderr == "", run.stderr[-3000:]      # the sanitizers are silent
    lines = run.stdout.splitlines()
    assert lines[0].startswith("C ok ") and int(lines[0].split()[2]) > 10000 and lines[1].startswith("T ok ")
    want = D.check_lines(keys, runs, streams, indexes)
    assert len(lines) == len(want) + 2
    for i, (got, exp) in enumerate(zip(lines[2:], want)):
        assert got == exp, (i, got[:200], exp[:200])
    # the cases reach what they are for: a sound index passes whole, unsound ones fail streams and leave others standing
    sound = want[len(keys) + len(runs)].split()[1:]
    assert all(v.startswith("0:") for v in sound)
    assert any(" 9:0:0" in v and " 0:" in v for v in want[len(keys) + len(runs) + 1:])

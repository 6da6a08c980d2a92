"""CPU tests of the batch find (include/snappier_hip_frame_find.h): the surface of libsnappier_hip_frame_find.so -- symbols, workspace arithmetic,
argument rejection, the C# binding, the sentences in capitals -- the model of the call (tests/frame_find_model.py) against the ground truth
(bytes.find over the oracle's decode) on overlapping occurrences, clipped windows, the cap, both admission bounds and an index whose sums
saturate, and the planning header csrc/frame_find_device.h compiled for the CPU under sanitizers (tests/abi/frame_find_plan_check.hip) and run
over the same requests, over indexes filled with anything at all and over windows beyond 2^32 bytes.  No GPU is touched."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

import frame_chunked_model as K
import frame_find_model as F
import frame_index_model as X
import oracle as O
from conftest import ROOT
from test_frame_diff_model import huge_side, unsound_indexes

NAMES = ["snp_frame_find_indexed_batch", "snp_frame_find_indexed_workspace"]
U64 = F.U64
WHOLE = (0, U64)


def _lib():
    from snappier_amd import _native as N
    return N.frame_find_lib()


def batch_of(streams):
    return streams, X.build_index(streams)


def full_run(streams, ix, requests, needles, caps):
    """The model with bounds that admit everything."""
    return F.find_plan(streams, ix, requests, needles, caps, *F.needs(streams, ix, requests, needles))


def check_truth(streams, ix, requests, needles, caps, got=None):
    """Every OK request of a model run gives the ground truth.  -> the run."""
    got = got or full_run(streams, ix, requests, needles, caps)
    status, win_len, count, nhits, hits, _ = got
    for r, ((b, ro, rl), needle) in enumerate(zip(requests, F.per_request(needles, len(requests)))):
        assert status[r] == O.OK, (r, status[r])
        wl, n, want = F.truth(streams[b], ro, rl, needle, caps[r])
        assert (win_len[r], count[r], nhits[r], hits[r]) == (wl, n, len(want), want), (r, requests[r], needle)
    return got


# ---- the surface -----------------------------------------------------------------------------------------------------------------------------
def test_header_and_binding_declare_the_new_functions():
    from snappier_amd import _native as N
    import snappier_amd
    declared = N.frame_find_declared_symbols()
    assert sorted(declared) == NAMES
    others = set(N.declared_symbols())
    for name in N._EXTENSIONS:
        if name != "frame_find":
            others |= set(N.declared_symbols(N._extension_header(name)))
    assert not set(declared) & others                                  # the other headers' surfaces are left as they are
    lib = _lib()
    assert lib.snp_frame_find_indexed_batch.restype is C.c_int and len(lib.snp_frame_find_indexed_batch.argtypes) == 29
    assert lib.snp_frame_find_indexed_workspace.restype is C.c_uint64 and len(lib.snp_frame_find_indexed_workspace.argtypes) == 3
    text = open(os.path.join(ROOT, "include", "snappier_hip_frame_find.h")).read()
    assert re.search(r"#define SNP_FIND_MAX_NEEDLE %du\b" % snappier_amd.FIND_MAX_NEEDLE, text) and snappier_amd.FIND_MAX_NEEDLE == F.MAX_NEEDLE == 256
    assert snappier_amd.FIND_TILE == F.TILE                             # (the model reads kFindTile from csrc/frame_find_device.h)
    assert str(F.TILE) in text


def test_extension_library_exports_exactly_its_header():
    from layouts import exported
    from snappier_amd import _native as N

    ext = exported(N.FRAME_FIND_PATH)
    assert ext == set(NAMES)
    for name in N._EXTENSIONS:
        if name != "frame_find":
            assert not exported(N._extension_path(name)) & ext
    assert not exported(N.PRODUCT_PATH) & ext


def test_workspace_is_monotone_host_arithmetic():
    ws = _lib().snp_frame_find_indexed_workspace
    assert ws(0, 0, 0) == 0 and ws(0, 1 << 20, 1 << 40) == 0           # nothing when there is no request
    for nreq in (1, 2, 255, 256, 257, 70000):
        base = ws(nreq, 0, 0)
        assert 0 < base <= 128 * nreq + 64 * 256                        # per-request words, and a tile's words per request
        grown = ws(nreq, 0, 1 << 20) - base                             # + scratch_cap bytes, a tile's 12 bytes per kFindTile of it (and alignment)
        assert (1 << 20) <= grown <= (1 << 20) + 12 * ((1 << 20) // F.TILE) + 8 * 256
        rows = ws(nreq, 1000, 0) - base
        assert 0 < rows <= 1000 * 41 + 16 * 256                         # per row of the chunk table 41 bytes
        assert ws(nreq + 1, 1000, 12345) >= ws(nreq, 1000, 12345) >= ws(nreq, 999, 12345) >= ws(nreq, 999, 12344)
    assert ws(1, 1 << 31, 0) == 0 and ws(1 << 30, 0, 0) == 0            # counts the call refuses
    assert ws(1, 0, 1 << 50) == ws(1, 0, (1 << 40) - 1)                 # scratch_cap counts as no more than 2^40 - 1


def test_null_pointers_and_counts_are_rejected_before_any_device_work():
    call = _lib().snp_frame_find_indexed_batch
    fake = C.c_void_p(0x1000)

    def args(ctx=fake, ins=(fake,) * 3, idx=(fake,) * 5, ns=1, ne=1, req=(fake,) * 3, nreq=1, needles=(fake,) * 3, mr=0, sc=0, hits=(fake,) * 3,
             outs=(fake,) * 4, work=fake, result=fake):
        return (ctx, *ins, ns, *idx, ne, *req, nreq, *needles, mr, sc, *hits, *outs, work, result)

    assert call(*args(ctx=None)) == O.ERR_BAD_ARG
    assert call(*args(result=None)) == O.ERR_BAD_ARG
    assert call(*args(nreq=0, result=None)) == O.ERR_BAD_ARG           # an empty call still needs d_result
    assert call(*args(nreq=1 << 30)) == O.ERR_BAD_ARG
    assert call(*args(mr=1 << 31)) == O.ERR_BAD_ARG
    assert call(*args(work=None)) == O.ERR_BAD_ARG
    for group, n in (("ins", 3), ("req", 3), ("needles", 3), ("hits", 3), ("outs", 4), ("idx", 5)):
        for i in range(n):
            a = [fake] * n
            a[i] = None
            assert call(*args(**{group: tuple(a)})) == O.ERR_BAD_ARG, (group, i)


def test_csharp_binding_matches_the_extension_header():
    import test_csharp_signatures as T
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "snappier_hip_frame_find.h")).read(), flags=re.S)
    protos = {}
    for m in re.finditer(r"([A-Za-z_][A-Za-z0-9_ ]*?[\s\*]+)(snp_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", text):
        params = [re.match(r"(.*?[\s\*])([A-Za-z_][A-Za-z0-9_]*)$", q.strip()).group(1) for q in m.group(3).split(",") if q.strip() not in ("", "void")]
        protos[m.group(2)] = (T.c_class(m.group(1)), [T.c_class(q) for q in params])
    cs = re.sub(r"//.*", "", open(os.path.join(ROOT, "csharp", "Snappier.Gpu", "NativeMethodsFrameFind.cs")).read())
    assert 'const string Lib = "snappier_hip_frame_find"' in cs
    imps = {}
    for m in re.finditer(r"\[DllImport\(Lib, CallingConvention = Cc\)\]\s*internal static extern ([A-Za-z\*]+) (snp_[a-z0-9_]+)\(([^)]*)\);", cs):
        params = [re.match(r"(.*?)\s+([A-Za-z_][A-Za-z0-9_]*)$", q.strip()).group(1) for q in m.group(3).split(",") if q.strip()]
        imps[m.group(2)] = (T.cs_class(m.group(1)), [T.cs_class(q) for q in params])
    assert set(protos) == set(imps) == set(NAMES)
    for name, (ret, params) in protos.items():
        cret, cparams = imps[name]
        assert T.compatible(ret, cret), (name, ret, cret)
        assert len(params) == len(cparams) and all(T.compatible(a, b) for a, b in zip(params, cparams)), (name, params, cparams)
    assert len(protos["snp_frame_find_indexed_batch"][1]) == 29
    assert "SNP_FIND_MAX_NEEDLE = 256" in cs
    proj = open(os.path.join(ROOT, "csharp", "Snappier.Gpu", "Snappier.Gpu.csproj")).read()
    assert 'Include="../../snappier_amd/libsnappier_hip_frame_find.so"' in proj


def test_header_says_in_capitals_what_is_decoded_and_what_is_not_noticed():
    text = " ".join(open(os.path.join(ROOT, "include", "snappier_hip_frame_find.h")).read().replace(" * ", " ").split())
    assert "EVERY CHUNK THE WINDOW MEETS IS DECODED WHOLE AND VERIFIED" in text and "ZERO-LENGTH ROWS ARE NEVER DECODED" in text
    assert "A CORRUPT CHUNK OUTSIDE THE WINDOW IS NOT NOTICED" in text
    assert "THE INDEX IS UNTRUSTED INPUT" in text and "SIZING TAKES ONE ROUND" in text
    assert "AS OFFSETS INTO WHAT THE STREAM DECODES TO, NOT INTO THE WINDOW" in text


# ---- the model against the ground truth ----------------------------------------------------------------------------------------------------------
def test_overlapping_occurrences_are_all_counted():
    assert F.occurrences(b"aaaaa", b"aaa") == [0, 1, 2] and F.occurrences(b"ababab", b"abab") == [0, 2] and F.occurrences(b"abc", b"abcd") == []
    streams, ix = batch_of([K.stream_of(b"a" * 1000, 7), K.stream_of(b"ab" * 500, 7)])
    reqs = [(0, *WHOLE), (0, *WHOLE), (1, *WHOLE), (0, 10, 5), (1, 1, 6)]
    needles = [b"aaa", b"aa", b"abab", b"aaa", b"abab"]
    got = check_truth(streams, ix, reqs, needles, [2000] * 5)
    assert got[2] == [998, 999, 499, 3, 1] and got[4][3] == [10, 11, 12] and got[4][4] == [2]
    assert got[5][1] == sum(got[2]) and got[5][3] == 5


def test_windows_are_clipped_and_positions_are_stream_offsets():
    raw = bytes(np.random.default_rng(5).integers(0, 256, 1000, dtype=np.uint8))
    streams, ix = batch_of([K.stream_of(raw, 64), K.stream_of(b"", 64)])
    n = raw[500:503]
    reqs = [(0, *WHOLE), (0, 500, 3), (0, 501, 3), (0, 499, 3), (0, 498, 5), (0, 500, 2), (0, 990, 500), (0, 1000, 5), (0, 5000, 10), (0, U64, U64),
            (0, 0, 0), (1, *WHOLE), (0, 997, U64)]
    got = check_truth(streams, ix, reqs, n, [10] * len(reqs))
    assert got[4][0] == [500] and got[4][1] == [500] and got[2][2] == 0 and got[2][3] == 0 and got[4][4] == [500]
    assert got[1][5] == 2 and got[2][5] == 0                            # a window shorter than the needle: OK, nothing
    assert got[1][6] == 10 and got[1][7:12] == [0] * 5
    got = check_truth(streams, ix, [(0, 997, U64)], raw[997:], [10])
    assert got[4][0] == [997]


def test_the_cap_keeps_the_first_occurrences_and_the_count_is_of_all():
    streams, ix = batch_of([K.stream_of(b"a" * 100, 7)])
    for cap in (0, 1, 97, 98, 99):
        got = check_truth(streams, ix, [(0, *WHOLE)], b"aaa", [cap])
        assert got[2] == [98] and got[3] == [min(cap, 98)] and got[4][0] == list(range(min(cap, 98)))


def test_needle_lengths_that_are_not_legal_own_nothing():
    streams, ix = batch_of([K.stream_of(b"a" * 100, 7)])
    reqs = [(0, *WHOLE)] * 4
    needles = [b"a", b"", b"a" * 257, b"a" * 256]
    got = full_run(streams, ix, reqs, needles, [5] * 4)
    assert got[0] == [O.OK, O.ERR_BAD_ARG, O.ERR_BAD_ARG, O.OK] and got[2] == [100, 0, 0, 0]
    assert got[5] == [2 * 15, 100, 2 * 100, 2]                          # ... and count no row and no byte


def test_admission_by_rows_and_by_scratch_is_in_request_order():
    raw = bytes(np.random.default_rng(6).integers(0, 256, 700, dtype=np.uint8))
    streams, ix = batch_of([K.stream_of(raw, 50), K.stream_of(raw, 70)])
    reqs = [(0, *WHOLE), (1, *WHOLE), (0, 10, 100), (0, 0, 0), (5, 0, 1), (1, 69, 2), (0, 55, 30)]
    nreq = len(reqs)
    needle = raw[60:62]
    rows, scratch = F.needs(streams, ix, reqs, needle)
    per_rows, per_bytes = [14, 10, 3, 0, 0, 2, 1], [700, 700, 150, 0, 0, 140, 50]   # edge chunks whole
    assert [F.needs(streams, ix, [q], needle) for q in reqs] == list(zip(per_rows, per_bytes))
    assert (rows, scratch) == (sum(per_rows), sum(per_bytes))
    free = F.find_plan(streams, ix, reqs, needle, [9] * nreq, rows, scratch)
    assert free[0] == [O.OK] * 4 + [O.ERR_BAD_ARG] + [O.OK] * 2 and free[5] == [rows, sum(free[2]), scratch, 6]
    for k in range(nreq + 1):
        for bound, per in ((0, per_rows), (1, per_bytes)):
            for delta in (-1, 0, 1):
                cap = sum(per[:k]) + delta
                if cap < 0:
                    continue
                got = F.find_plan(streams, ix, reqs, needle, [9] * nreq, cap if bound == 0 else rows, scratch if bound == 0 else cap)
                admitted = max(i for i in range(nreq + 1) if sum(per[:i]) <= cap)
                assert got[0] == free[0][:admitted] + [O.ERR_OUTPUT_TOO_SMALL] * (nreq - admitted)
                assert got[4][:admitted] == free[4][:admitted] and got[2][admitted:] == [0] * (nreq - admitted)
                assert got[5][0] == rows and got[5][2] == scratch and got[5][3] == sum(1 for s in got[0] if s == O.OK)


def test_sums_saturate_on_an_index_filled_with_anything():
    s = K.stream_of(b"x" * 100, 10)
    good = X.build_index([s])
    big = 1 << 63
    # the rows' starts say that a request's run holds 2^63 + 5 bytes: two of them wrap a plain sum to 10, which any scratch_cap admits
    ix = {**good, "start": [0] + [big] * 9, "total": [big + 5]}
    reqs = [(0, 0, big + 5)] * 2
    assert F.needs_of(ix, 1, reqs[0], 1) == (O.OK, 10, big + 5) and (2 * (big + 5)) & U64 == 10
    got = F.find_plan([s], ix, reqs, b"x", [1] * 2, 1 << 30, 1 << 20)
    assert got[5] == [20, 0, U64, 0] and got[0] == [O.ERR_OUTPUT_TOO_SMALL] * 2
    got = F.find_plan([s], ix, reqs, b"x", [1] * 2, 1 << 30, U64)        # scratch_cap counts as no more than 2^40 - 1
    assert got[0] == [O.ERR_OUTPUT_TOO_SMALL] * 2
    # a request that claims 2^40 rows counts as 2^31 of them
    many = {**good, "first": [0, 1 << 40]}
    assert F.find_plan([s], many, [(0, *WHOLE)], b"x", [1], 1 << 30, 1 << 30)[5][0] == 10   # (idx_first is clamped to nentries)
    assert F.ROW_CLAMP == 1 << 31 and F.CAP_MAX == (1 << 40) - 1
    got = F.find_plan([s], good, [(0, *WHOLE)], b"x", [1], 10, 1 << 50)
    assert got[0] == [O.OK] and got[2] == [100]


def test_named_streams_and_unsound_indexes_give_a_status_per_request():
    streams = list(X.named_streams().values())
    ix = X.build_index(streams)
    windows = [(b, ro & U64, rl & U64) for b, ro, rl in X.all_windows(streams)]
    reqs = windows[::7]
    needles = [bytes([r % 251]) * (1 + r % 3) for r in range(len(reqs))]
    got = full_run(streams, ix, reqs, needles, [4] * len(reqs))
    oks = 0
    for r, (b, ro, rl) in enumerate(reqs):
        if got[0][r] != O.OK:
            assert (got[1][r], got[2][r], got[3][r], got[4][r]) == (0, 0, 0, [])
            continue
        oks += 1
        assert got[0][r] == X.read_plan(streams, ix, [reqs[r]], [U64], 1 << 62, 1 << 62)[0][0]
    assert 30 < oks < len(reqs)
    rng = np.random.default_rng(3)
    refused = 0
    for index in unsound_indexes(ix, streams, rng):
        status = full_run(streams, index, reqs[::3], b"\n", [4] * len(reqs[::3]))[0]
        refused += status.count(O.ERR_BAD_ARG)
    assert refused > 150


# ---- the header on the CPU, under sanitizers -----------------------------------------------------------------------------------------------------
def test_header_under_sanitizers_matches_the_model(tmp_path):
    streams = list(X.named_streams().values())
    ns = len(streams)
    ix = X.build_index(streams)
    windows = [(b, ro & U64, rl & U64) for b, ro, rl in X.all_windows(streams)]
    rng = np.random.default_rng(11)
    lens = [1, 2, 3, 15, 16, 17, 33, 256, 0, 257]
    sound = [(*w, lens[i % len(lens)]) for i, w in enumerate(windows[::2])]
    # windows around the tile borders of the long stream: the last tile ends at the window's last start position
    long_b = max(range(ns), key=lambda b: ix["total"][b])
    total = ix["total"][long_b]
    assert total > 3 * F.TILE
    tiles = [(long_b, lo, F.TILE * k + d + m - 1, m) for lo in (0, 5) for k in (1, 2) for d in (-1, 0, 1) for m in (1, 2, 256)] + \
        [(long_b, 0, U64, 1), (long_b, 7, U64, 256), (long_b, total - 300, U64, 256), (long_b, total - 255, U64, 256)]
    some = sound[::4] + [(ns, 0, 10, 1), (0xFFFFFFFF, 5, 5, 2)]
    cases = [(ix, sound), (ix, tiles)]
    nsound = len(cases)
    for index in unsound_indexes(ix, streams, rng):
        cases.append((index, some))
    huge = huge_side()
    cpath, hpath = str(tmp_path / "cases.bin"), str(tmp_path / "huge.bin")
    F.write_cases(cpath, streams, cases)
    big = [(0, 0, U64, 1), (0, 65536 * 3 + 5, 1 << 33, 17), (0, 1 << 32, U64, 256), (0, (1 << 32) - (1 << 20) + 7, 1 << 20, 3)]
    F.write_cases(hpath, huge.streams, [(huge.ix, big)])
    exe = str(tmp_path / "frame_find_plan_check")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host",
                    "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "abi", "frame_find_plan_check.hip"), "-o", exe,
                    "-Wl,-rpath,/opt/rocm/lib"], check=True)
    env = {**os.environ, "ASAN_OPTIONS": "detect_leaks=1:abort_on_error=0", "UBSAN_OPTIONS": "print_stacktrace=1:halt_on_error=1"}
    run = subprocess.run([exe, cpath], capture_output=True, text=True, env=env)
    assert run.returncode == 0 and run.stderr == "", run.stderr[-3000:]      # the sanitizers are silent
    lines = run.stdout.splitlines()
    assert len(lines) == sum(len(c[1]) for c in cases)
    at = refused = planned = 0
    for c, (index, reqs) in enumerate(cases):
        for b, ro, rl, m in reqs:
            want = F.plan_line(index, streams, (b, ro, rl), m)
            assert lines[at] == want, (c, (b, ro, rl, m))
            if c >= nsound:
                f = want.split()
                bad = f[0] != "0" or f[-1] != "0"
                refused += bad
                planned += not bad
            at += 1
    assert refused > 150 and planned > 20                               # both outcomes, on the unsound indexes
    # the tiles: what the model says, spelt out for one window -- 2 * TILE + 1 start positions make three tiles, the last of one position
    line = F.plan_line(ix, streams, (long_b, 5, 2 * F.TILE + 1 + 255), 256).split()
    assert line[3:10] == [str(v) for v in (2 * F.TILE + 1, 3, 5, 5 + F.TILE, 5 + 2 * F.TILE, 5 + 2 * F.TILE + 1, 0)]
    run = subprocess.run([exe, hpath], capture_output=True, text=True, env=env)
    assert run.returncode == 0 and run.stderr == "", run.stderr[-3000:]
    hl = run.stdout.splitlines()
    assert hl == [F.plan_line(huge.ix, huge.streams, q[:3], q[3]) for q in big]
    assert hl[0].split()[:4] == ["0", "65537", str(65537 * 65536), str(65537 * 65536)] and hl[3].split()[1:3] == ["17", str(17 * 65536)]

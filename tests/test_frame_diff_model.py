"""CPU tests of the batch diff (include/snappier_hip_frame_diff.h): the surface of libsnappier_hip_frame_diff.so -- symbols, workspace arithmetic,
argument rejection, the C# binding, the two sentences in capitals -- the model of the call (tests/frame_diff_model.py) against the ground truth
(plain byte comparison of the oracle's decodes) on random tilings, every single-byte difference position, windows of different length, empty and
clipped windows, the model's documented blindness (a corrupt body inside a CRC-equal span, a constructed CRC collision), and the planning header
csrc/frame_diff_device.h compiled for the CPU under sanitizers (tests/abi/frame_diff_plan_check.hip) and run over the same requests, over
indexes filled with anything at all and over windows beyond 2^32 bytes.  No GPU is touched."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import frame_chunked_model as K
import frame_diff_model as F
import frame_index_model as X
import frame_range_model as R
import oracle as O
from conftest import ROOT

NAMES = ["snp_frame_diff_indexed_batch", "snp_frame_diff_indexed_workspace"]
U64 = F.U64
P, S, E = F.PREFIX, F.SUFFIX, F.EXACT
MODES = [P, S, P | S, P | E, S | E, P | S | E]
WHOLE = (0, U64)


def _lib():
    from snappier_amd import _native as N
    return N.frame_diff_lib()


def side_of(streams):
    return F.Side(streams, X.build_index(streams))


def whole(ba: int, bb: int):
    return (ba, *WHOLE, bb, *WHOLE)


def full_run(a: F.Side, b: F.Side, requests, flags: int):
    """The model with bounds that admit everything."""
    return F.diff_plan(a, b, requests, flags, *F.needs(a, b, requests, flags))


def check_truth(a: F.Side, b: F.Side, requests, flags: int, got=None):
    """Every OK request of a model run gives the ground truth.  -> the run."""
    got = got or full_run(a, b, requests, flags)
    status, len_a, len_b, prefix, suffix, _ = got
    for r, (ba, oa, la, bb, ob, lb) in enumerate(requests):
        assert status[r] == O.OK, (r, status[r])
        x, y = F.window_bytes(a.streams[ba], oa, la), F.window_bytes(b.streams[bb], ob, lb)
        assert (len_a[r], len_b[r]) == (len(x), len(y)), r
        assert (prefix[r], suffix[r]) == F.truth(x, y, flags), (r, flags, requests[r])
    return got


# ---- the surface -----------------------------------------------------------------------------------------------------------------------------
def test_header_and_binding_declare_the_new_functions():
    from snappier_amd import _native as N
    import snappier_amd
    declared = N.frame_diff_declared_symbols()
    assert sorted(declared) == NAMES
    others = set(N.declared_symbols())
    for name in N._EXTENSIONS:
        if name != "frame_diff":
            others |= set(N.declared_symbols(N._extension_header(name)))
    assert not set(declared) & others                                  # the other headers' surfaces are left as they are
    lib = _lib()
    assert lib.snp_frame_diff_indexed_batch.restype is C.c_int and len(lib.snp_frame_diff_indexed_batch.argtypes) == 38
    assert lib.snp_frame_diff_indexed_workspace.restype is C.c_uint64 and len(lib.snp_frame_diff_indexed_workspace.argtypes) == 3
    assert (snappier_amd.DIFF_PREFIX, snappier_amd.DIFF_SUFFIX, snappier_amd.DIFF_EXACT) == (1, 2, 4)
    text = open(os.path.join(ROOT, "include", "snappier_hip_frame_diff.h")).read()
    for name, value in (("SNP_DIFF_PREFIX", 1), ("SNP_DIFF_SUFFIX", 2), ("SNP_DIFF_EXACT", 4)):
        assert re.search(r"#define %s %du\b" % (name, value), text)


def test_extension_library_exports_exactly_its_header():
    from layouts import exported
    from snappier_amd import _native as N

    ext = exported(N.FRAME_DIFF_PATH)
    assert ext == set(NAMES)
    for name in N._EXTENSIONS:
        if name != "frame_diff":
            assert not exported(N._extension_path(name)) & ext
    assert not exported(N.PRODUCT_PATH) & ext


def test_workspace_is_monotone_host_arithmetic():
    ws = _lib().snp_frame_diff_indexed_workspace
    assert ws(0, 0, 0) == 0 and ws(0, 1 << 20, 1 << 40) == 0           # nothing when there is no request
    for nreq in (1, 2, 255, 256, 257, 70000):
        base = ws(nreq, 0, 0)
        assert 0 < base <= 1024 * nreq + 64 * 256                       # per-request and per-piece words
        assert ws(nreq, 0, 12345) - base in range(12345, 12345 + 256)   # + scratch_cap bytes (and alignment)
        rows = ws(nreq, 1000, 0) - base
        assert 0 < rows <= 1000 * 8 + 64 * 256                          # per owned row: two words
        rows = ws(nreq, 1000, 1 << 20) - ws(nreq, 0, 1 << 20)
        assert 0 < rows <= 1000 * (8 + 4 * 41) + 64 * 256               # ... and, per side, two chunk table rows of 41 bytes where scratch_cap allows as many
        assert ws(nreq + 1, 1000, 12345) >= ws(nreq, 1000, 12345) >= ws(nreq, 999, 12345) >= ws(nreq, 999, 12344)
    assert ws(1, 1 << 31, 0) == 0 and ws(1 << 30, 0, 0) == 0            # counts the call refuses


def test_null_pointers_counts_and_flags_are_rejected_before_any_device_work():
    call = _lib().snp_frame_diff_indexed_batch
    fake = C.c_void_p(0x1000)

    def args(ctx=fake, ins_a=(fake,) * 3, idx_a=(fake,) * 5, ins_b=(fake,) * 3, idx_b=(fake,) * 5, ns=1, ne=1, req=(fake,) * 6, nreq=1, flags=3, mr=0,
             sc=0, outs=(fake,) * 5, work=fake, result=fake):
        return (ctx, *ins_a, ns, *idx_a, ne, *ins_b, ns, *idx_b, ne, *req, nreq, flags, mr, sc, *outs, work, result)

    assert call(*args(ctx=None)) == O.ERR_BAD_ARG
    assert call(*args(result=None)) == O.ERR_BAD_ARG
    assert call(*args(nreq=0, result=None)) == O.ERR_BAD_ARG           # an empty call still needs d_result
    assert call(*args(nreq=1 << 30)) == O.ERR_BAD_ARG
    assert call(*args(mr=1 << 31)) == O.ERR_BAD_ARG
    assert call(*args(work=None)) == O.ERR_BAD_ARG
    for flags in (0, E, 8, P | 8, P | S | E | 16, 1 << 31):             # neither direction, or a bit that is no flag
        assert call(*args(flags=flags)) == O.ERR_BAD_ARG, flags
        assert call(*args(flags=flags, nreq=0)) == O.ERR_BAD_ARG, flags
    for group, n in (("ins_a", 3), ("ins_b", 3), ("req", 6), ("outs", 5), ("idx_a", 5), ("idx_b", 5)):
        for i in range(n):
            a = [fake] * n
            a[i] = None
            assert call(*args(**{group: tuple(a)})) == O.ERR_BAD_ARG, (group, i)


def test_csharp_binding_matches_the_extension_header():
    import test_csharp_signatures as T
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "snappier_hip_frame_diff.h")).read(), flags=re.S)
    protos = {}
    for m in re.finditer(r"([A-Za-z_][A-Za-z0-9_ ]*?[\s\*]+)(snp_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", text):
        params = [re.match(r"(.*?[\s\*])([A-Za-z_][A-Za-z0-9_]*)$", q.strip()).group(1) for q in m.group(3).split(",") if q.strip() not in ("", "void")]
        protos[m.group(2)] = (T.c_class(m.group(1)), [T.c_class(q) for q in params])
    cs = re.sub(r"//.*", "", open(os.path.join(ROOT, "csharp", "Snappier.Gpu", "NativeMethodsFrameDiff.cs")).read())
    assert 'const string Lib = "snappier_hip_frame_diff"' in cs
    imps = {}
    for m in re.finditer(r"\[DllImport\(Lib, CallingConvention = Cc\)\]\s*internal static extern ([A-Za-z\*]+) (snp_[a-z0-9_]+)\(([^)]*)\);", cs):
        params = [re.match(r"(.*?)\s+([A-Za-z_][A-Za-z0-9_]*)$", q.strip()).group(1) for q in m.group(3).split(",") if q.strip()]
        imps[m.group(2)] = (T.cs_class(m.group(1)), [T.cs_class(q) for q in params])
    assert set(protos) == set(imps) == set(NAMES)
    for name, (ret, params) in protos.items():
        cret, cparams = imps[name]
        assert T.compatible(ret, cret), (name, ret, cret)
        assert len(params) == len(cparams) and all(T.compatible(a, b) for a, b in zip(params, cparams)), (name, params, cparams)
    assert len(protos["snp_frame_diff_indexed_batch"][1]) == 38
    assert "SNP_DIFF_PREFIX = 1, SNP_DIFF_SUFFIX = 2, SNP_DIFF_EXACT = 4" in cs
    proj = open(os.path.join(ROOT, "csharp", "Snappier.Gpu", "Snappier.Gpu.csproj")).read()
    assert 'Include="../../snappier_amd/libsnappier_hip_frame_diff.so"' in proj


def test_header_says_in_capitals_what_is_not_noticed():
    text = " ".join(open(os.path.join(ROOT, "include", "snappier_hip_frame_diff.h")).read().replace(" * ", " ").split())
    assert "A CORRUPT BODY OF A CHUNK THAT IS NOT DECODED IS NOT NOTICED" in text
    assert "TWO DIFFERENT SPANS WHOSE HEADER CRCS COLLIDE (PROBABILITY 2^-32 PER SPAN) ARE TAKEN AS EQUAL, UNLESS SNP_DIFF_EXACT IS SET" in text
    assert "BOTH INDEXES ARE UNTRUSTED INPUT" in text and "SIZING TAKES TWO ROUNDS" in text


# ---- the model against the ground truth ----------------------------------------------------------------------------------------------------------
def tiled(raw: bytes, cuts) -> bytes:
    """A framed stream whose data chunks end at the given offsets of raw (and at its end)."""
    out, at = [K.stream_of(b"", 1)], 0
    for c in sorted(set(cuts) | {len(raw)}):
        if c > at:
            out.append(K.stream_of(raw[at:c], 65536)[len(out[0]):])
            at = c
    return b"".join(out)


def test_tiled_is_a_stream_of_its_bytes():
    raw = bytes(range(200))
    s = tiled(raw, [3, 50, 51])
    assert O.frame_decode(s) == raw and X.index_of(s)[0] == [0, 3, 50, 51]


@pytest.mark.parametrize("flags", MODES)
def test_random_tilings_give_the_ground_truth(flags):
    rng = np.random.default_rng(flags)
    for trial in range(12):
        n = int(rng.integers(1, 400))
        raw = bytes(rng.integers(0, 4, n, dtype=np.uint8))              # few symbols: long accidental matches around a difference
        other = bytearray(raw)
        for _ in range(int(rng.integers(0, 4))):
            other[int(rng.integers(0, n))] ^= 1
        other = bytes(other)
        if trial % 3 == 0:
            at = int(rng.integers(0, n + 1))
            other = other[:at] + bytes(rng.integers(0, 4, int(rng.integers(1, 30)), dtype=np.uint8)) + other[at + int(rng.integers(0, 20)):]
        cuts_a = [int(v) for v in rng.integers(0, n + 1, int(rng.integers(0, 12)))]
        cuts_b = [int(v) for v in rng.integers(0, len(other) + 1, int(rng.integers(0, 12)))] + cuts_a[:trial % 4]
        a, b = side_of([tiled(raw, cuts_a), tiled(raw, cuts_b)]), side_of([tiled(other, cuts_b), tiled(raw, cuts_a)])
        reqs = [whole(0, 0), whole(1, 0), whole(0, 1), whole(1, 1)]
        for _ in range(6):                                              # windows, of the same and of different lengths
            oa, ob = int(rng.integers(0, n)), int(rng.integers(0, n))
            reqs += [(0, oa, int(rng.integers(0, n)), 0, ob, int(rng.integers(0, n))), (1, oa, 40, 1, oa, 40), (0, oa, 0, 0, ob, 5), (0, n - 3, 10, 0, 1, U64)]
        check_truth(a, b, reqs, flags)


@pytest.mark.parametrize("ca, cb", [(1, 7), (7, 21), (5, 7), (7, 7)])
def test_every_single_byte_difference_position(ca, cb):
    rng = np.random.default_rng(ca * 100 + cb)
    raw = bytes(rng.integers(0, 256, 300, dtype=np.uint8))
    a = side_of([K.stream_of(raw, ca)])
    b = side_of([K.stream_of(raw[:p] + bytes([raw[p] ^ 0x40]) + raw[p + 1:], cb) for p in range(300)] + [K.stream_of(raw, cb)])
    reqs = [whole(0, p) for p in range(301)]
    for flags in (P | S, P | S | E):
        status, len_a, len_b, prefix, suffix, result = check_truth(a, b, reqs, flags)
        assert prefix == list(range(300)) + [300] and suffix == [299 - p for p in range(300)] + [0]
        assert result[3] == 301 and result[1] == 301 * 300
    # from the headers alone: an equal pair decodes nothing, a differing pair the span around the difference in each direction
    need = [F.diff_plan(a, b, [q], P | S, 1 << 20, 0)[5][2] for q in reqs]
    lcm = ca * cb // int(np.gcd(ca, cb))
    assert need[300] == 0
    assert all(0 < v <= 4 * lcm for v in need[:300])


def test_empty_clipped_and_unequal_windows():
    raw = bytes(np.random.default_rng(5).integers(0, 256, 1000, dtype=np.uint8))
    a, b = side_of([K.stream_of(raw, 64), K.stream_of(b"", 64)]), side_of([K.stream_of(raw + b"tail", 100)])
    reqs = [(0, 0, 0, 0, 0, 0), (1, *WHOLE, 0, *WHOLE), (0, *WHOLE, 0, *WHOLE), (0, 990, 500, 0, 990, 500), (0, 5000, 10, 0, 5, 10),
            (0, 64, 64, 0, 64, 64), (0, 64, 128, 0, 64, 64), (0, 100, 200, 0, 100, 200), (0, 1, 999, 0, 0, 1000), (0, U64, U64, 0, U64 - 1, 2)]
    for flags in MODES:
        status, len_a, len_b, prefix, suffix, _ = check_truth(a, b, reqs, flags)
        assert (len_a[2], len_b[2]) == (1000, 1004) and len_a[3] == 10 and len_b[3] == 14
    status, len_a, len_b, prefix, suffix, _ = full_run(a, b, reqs, P | S)
    assert prefix[2] == 1000 and suffix[2] == 0                         # an append: prefix == len_a
    assert (prefix[5], suffix[5]) == (64, 0) and (prefix[6], suffix[6]) == (64, 0)


def test_admission_by_rows_and_by_scratch_is_in_request_order():
    raw = bytes(np.random.default_rng(6).integers(0, 256, 700, dtype=np.uint8))
    other = raw[:333] + b"\x00" + raw[334:]
    a, b = side_of([K.stream_of(raw, 50)]), side_of([K.stream_of(other, 70), K.stream_of(raw, 70)])
    reqs = [whole(0, 0), whole(0, 1), (0, 10, 100, 0, 10, 100), whole(0, 0), (0, 0, 0, 1, 0, 0), whole(0, 0)]
    rows, scratch = F.needs(a, b, reqs, P | S)
    free = F.diff_plan(a, b, reqs, P | S, rows, scratch)
    assert free[0] == [O.OK] * 6 and free[5] == [rows, free[5][1], scratch, 6]
    per_rows = [F.diff_plan(a, b, [q], P | S, 1 << 20, 1 << 30)[5][0] for q in reqs]
    per_bytes = [F.diff_plan(a, b, [q], P | S, 1 << 20, 1 << 30)[5][2] for q in reqs]
    assert sum(per_rows) == rows and sum(per_bytes) == scratch and per_bytes[1] == 0 and per_bytes[0] > 0 and per_rows[4] == 0
    for k in range(7):
        for bound, per in ((0, per_rows), (1, per_bytes)):
            cap = sum(per[:k])
            got = F.diff_plan(a, b, reqs, P | S, cap if bound == 0 else rows, scratch if bound == 0 else cap)
            admitted = max(i for i in range(7) if sum(per[:i]) <= cap)
            assert got[0] == [O.OK] * admitted + [O.ERR_OUTPUT_TOO_SMALL] * (6 - admitted)
            assert got[3][:admitted] == free[3][:admitted] and got[3][admitted:] == [0] * (6 - admitted)
            assert got[5][0] == rows and got[5][3] == admitted
            if bound == 1:
                assert got[5][2] == scratch


# ---- the model's documented blindness --------------------------------------------------------------------------------------------------------------
def collide(data: bytes, at: int) -> bytes:
    """data with the 33 bits of the generator polynomial XORed in from byte `at` on: other bytes, the same CRC-32C."""
    poly = (1 << 32) | 0x1EDC6F41                                       # x^32 + ..., highest power first
    # CRC-32C processes each byte's LOWEST bit first: lay the polynomial out in that bit order over five bytes
    word = 0
    for i in range(33):
        if (poly >> (32 - i)) & 1:
            byte, bit = divmod(i, 8)
            word |= 1 << (8 * (4 - byte) + bit)
    mask = word.to_bytes(5, "big")
    return data[:at] + bytes(x ^ m for x, m in zip(data[at:at + 5], mask)) + data[at + 5:]


def test_corrupt_body_and_crc_collision_are_seen_only_with_exact():
    rng = np.random.default_rng(8)
    raw = bytes(rng.integers(0, 256, 64 * 6, dtype=np.uint8))
    s = K.stream_of(raw, 64)
    rows = R.walk(s)[0]
    ix = X.build_index([s])
    # a corrupt body inside a CRC-equal span
    bad = R.corrupt_chunk(s, rows[2])
    a, b = F.Side([s], ix), F.Side([bad], ix)
    blind = full_run(a, b, [whole(0, 0)], P | S)
    assert blind[0] == [O.OK] and (blind[3], blind[4]) == ([384], [0]) and blind[5][2] == 0
    seen = full_run(a, b, [whole(0, 0)], P | S | E)
    assert seen[0] == [R.chunk_result(bad, rows[2])[0]] and seen[0] != [O.OK] and (seen[3], seen[4]) == ([0], [0])
    # a corrupt header CRC: the span is decoded and fails to verify
    p = ix["pos"][3] + 4
    flipped = s[:p] + bytes([s[p] ^ 0x10]) + s[p + 1:]
    got = full_run(a, F.Side([flipped], ix), [whole(0, 0)], P | S)
    assert got[0] == [R.chunk_result(flipped, X.row_check(ix, flipped, dict(f1=6, total=384, lo=0, hi=384), 3, False))[0]] and got[0] != [O.OK]
    # a constructed collision
    twin = collide(raw, 64 * 4 + 9)
    assert twin != raw and O.crc32c(twin[256:320]) == O.crc32c(raw[256:320]) and sum(x != y for x, y in zip(raw, twin)) <= 5
    t = side_of([K.stream_of(twin, 64)])
    a = side_of([s])
    blind = full_run(a, t, [whole(0, 0)], P | S)
    assert blind[0] == [O.OK] and (blind[3], blind[4]) == ([384], [0])  # taken as equal
    check_truth(a, t, [whole(0, 0)], P | S | E)                         # found
    assert full_run(a, t, [whole(0, 0)], P | S | E)[3] != [384]
    # ... and seen without EXACT where the grids share no cut around it
    check_truth(a, side_of([K.stream_of(twin, 384)]), [(0, 1, U64, 0, 1, U64)], P | S)


def unsound_indexes(ix, streams, rng):
    ns, ne = len(streams), len(ix["start"])

    def rnd(n, hi=1 << 64):
        return [int(v) % hi for v in rng.integers(0, 1 << 63, n, dtype=np.uint64) * 2 + rng.integers(0, 2, n, dtype=np.uint64)]

    lens = [len(s) for s in streams]
    return [{**ix, "start": rnd(ne), "pos": rnd(ne)},                                    # rows filled with random u64
            {**ix, "first": rnd(ns + 1), "total": rnd(ns), "start": rnd(ne), "pos": rnd(ne)},
            {**ix, "start": rnd(ne, 1 << 17), "pos": rnd(ne, 1 << 12), "total": rnd(ns, 1 << 18)},   # small random values: searches go everywhere
            {**ix, "first": [f + (1 << 33) * (i % 2) for i, f in enumerate(ix["first"])]},       # idx_first beyond nentries
            {**ix, "first": list(reversed(ix["first"]))},
            {**ix, "pos": [p + lens[i % ns] for i, p in enumerate(ix["pos"])]},                  # positions beyond in_len
            {**ix, "pos": [max(lens) - 1 - (i % 20) for i in range(ne)]},                        # ... and within a few bytes of a stream's end
            {**ix, "start": list(reversed(ix["start"]))},                                        # non-monotone starts
            {**ix, "start": [v ^ ((i % 3 == 0) << 9) for i, v in enumerate(ix["start"])]},
            {**ix, "pos": [p + 1 for p in ix["pos"]]},                                           # stale: every header moved
            {**ix, "total": [t + (1 << 40) for t in ix["total"]]},                               # totals no row reaches
            {**ix, "tail": [int(v) % 40 - 20 for v in rng.integers(0, 1000, ns)]},               # tails that are no status
            {**ix, "start": ix["start"][:ne // 2], "pos": ix["pos"][:ne // 2]},                  # fewer rows than idx_first says
            {**ix, "start": [], "pos": []}]


@pytest.fixture(scope="module")
def named():
    cases = X.named_streams()
    streams = list(cases.values())
    return list(cases), streams, X.build_index(streams), X.all_windows(streams)


def test_named_streams_against_themselves_and_unsound_indexes(named):
    names, streams, ix, windows = named
    a = F.Side(streams, ix)
    reqs = [(b, ro, rl, b, ro, rl) for b, ro, rl in windows[::7]] + [(b, ro, rl, b, ro + 1, rl) for b, ro, rl in windows[3::11]]
    for flags in (P | S, S | E):
        status, len_a, len_b, prefix, suffix, _ = full_run(a, a, reqs, flags)
        oks = 0
        for r, q in enumerate(reqs):
            if status[r] != O.OK:
                assert (len_a[r], len_b[r], prefix[r], suffix[r]) == (0, 0, 0, 0)
                continue
            oks += 1
            if q[1] == q[4]:
                assert len_a[r] == len_b[r] and (prefix[r], suffix[r]) == ((len_a[r], 0) if flags & P else (0, len_a[r])), (r, q)
        assert oks > 30 and oks < len(reqs)
    rng = np.random.default_rng(3)
    refused = 0
    for index in unsound_indexes(ix, streams, rng):
        bad = F.Side(streams, index)
        for x, y in ((bad, a), (a, bad)):
            status = full_run(x, y, reqs[::3], P | S)[0]
            refused += status.count(O.ERR_BAD_ARG)
    assert refused > 300


# ---- the header on the CPU, under sanitizers -----------------------------------------------------------------------------------------------------
def huge_side():
    """Two streams whose indexes claim 65 537 rows of 65 536 bytes over ONE real chunk each: windows beyond 2^32 with no large buffer (the row
    check reads the header every row points at, and every row points at the same one)."""
    rng = np.random.default_rng(9)
    one = bytes(rng.integers(0, 256, 65536, dtype=np.uint8))
    s = K.stream_of(one, 65536)
    pos = X.index_of(s)[1][0]
    n = 65537
    ix = {"first": [0, n], "start": [i * 65536 for i in range(n)], "pos": [pos] * n, "total": [n * 65536], "tail": [0]}
    return F.Side([s], ix)


def test_header_under_sanitizers_matches_the_model(named, tmp_path):
    names, streams, ix, windows = named
    ns = len(streams)
    rng = np.random.default_rng(11)
    a = F.Side(streams, ix)
    sound = [(b, ro & U64, rl & U64, b, ro & U64, rl & U64) for b, ro, rl in windows[::2]] + \
        [(b, ro & U64, rl & U64, b, (ro + 1) & U64, rl & U64) for b, ro, rl in windows[1::4]]
    some = sound[::4] + [(ns, 0, 10, 0, 0, 10), (0, 5, 5, 0xFFFFFFFF, 5, 5)]
    raw = bytes(rng.integers(0, 256, 3000, dtype=np.uint8))
    other = raw[:1500] + b"!" + raw[1501:]
    g1, g2 = side_of([K.stream_of(raw, 64), K.stream_of(raw, 7)]), side_of([K.stream_of(other, 96), K.stream_of(other[:2000], 64), tiled(other, [5, 77, 1499, 1502])])
    grids = [(i, *WHOLE, j, *WHOLE) for i in range(2) for j in range(3)] + [(0, 10, 1000, 2, 10, 1200), (1, 64, 640, 1, 64, 640), (0, 0, 0, 0, 0, 0)]
    huge = huge_side()
    big = [whole(0, 0), (0, 65536 * 3 + 5, 1 << 33, 0, 65536 * 3 + 5, 1 << 33), (0, 1 << 32, U64, 0, (1 << 32) + 65536, U64), (0, 1, U64, 0, 0, U64)]
    cases = [(a, a, P | S, sound), (a, a, S | E, some), (g1, g2, P | S, grids), (g1, g2, P, grids), (g1, g2, S, grids), (g1, g2, P | S | E, grids),
             (g2, g1, P | S, [(q[3], q[4], q[5], q[0], q[1], q[2]) for q in grids]), (huge, huge, P | S, big), (huge, huge, P | E, big[:1])]
    for index in unsound_indexes(ix, streams, rng):
        cases += [(F.Side(streams, index), a, P | S, some), (a, F.Side(streams, index), P | S, some)]
    cpath = str(tmp_path / "cases.bin")
    F.write_cases(cpath, cases)
    exe = str(tmp_path / "frame_diff_plan_check")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host",
                    "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "abi", "frame_diff_plan_check.hip"), "-o", exe,
                    "-Wl,-rpath,/opt/rocm/lib"], check=True)
    env = {**os.environ, "ASAN_OPTIONS": "detect_leaks=1:abort_on_error=0", "UBSAN_OPTIONS": "print_stacktrace=1:halt_on_error=1"}
    run = subprocess.run([exe, cpath], capture_output=True, text=True, env=env)
    assert run.returncode == 0 and run.stderr == "", run.stderr[-3000:]      # the sanitizers are silent
    lines = run.stdout.splitlines()
    assert len(lines) == sum(len(c[3]) for c in cases)
    at = refused = planned = 0
    for c, (x, y, flags, reqs) in enumerate(cases):
        for q in reqs:
            want = F.plan_line(x, y, q, flags)
            assert lines[at] == want, (c, q)
            f = want.split()
            if c >= 9:
                bad = f[:2] != ["0", "0"] or f[3:5] != ["0", "0"]
                refused += bad
                planned += not bad
            at += 1
    assert refused > 300 and planned > 50                               # both outcomes, on the unsound indexes
    # windows beyond 2^32: every row points at one chunk, so every span's CRCs agree and nothing but ragged ends is decoded
    hl = [line.split() for line in lines[sum(len(c[3]) for c in cases[:7]):][:4]]
    assert hl[0][2] == str(65537 * 65536) and hl[0][5:7] == ["1", "0"] and hl[1][2] == str(65537 * 65536 - 65536 * 3 - 5)

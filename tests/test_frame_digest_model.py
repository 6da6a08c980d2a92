"""snp_frame_digest_indexed_batch / snp_crc32c_combine (libsnappier_hip_frame_digest.so) without a GPU: the declarations and their C# binding,
the workspace arithmetic, argument rejection; the combine of the Python model (frame_digest_model.py) against the oracle's CRC-32C of the
concatenation, the group law of the shift, the library's host combine against the model; the model of the whole call against the oracle's CRC of
the decoded window on every window of the named streams, admission by edge_cap, corruption inside and at the edge of a window, a stale index;
and the header (csrc/frame_digest_device.h) itself, compiled for the CPU under AddressSanitizer and UBSan into a stand-alone program
(tests/abi/frame_digest_plan_check.hip) and run over the same requests, over indexes filled with anything at all and over shifts of 2^32
bytes and more."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import frame_digest_model as D
import frame_index_model as X
import frame_range_model as R
import oracle as O
from conftest import ROOT

NAMES = ["snp_crc32c_combine", "snp_frame_digest_indexed_batch", "snp_frame_digest_indexed_workspace"]
PIECES = [0, 1, 3, 4, 63, 64, 65, 4095, 4096, 65535, 65536]
U64 = D.U64


def _lib():
    from snappier_amd import _native as N
    return N.frame_digest_lib()


# ---- the surface -----------------------------------------------------------------------------------------------------------------------------
def test_header_and_binding_declare_the_new_functions():
    from snappier_amd import _native as N
    declared = N.frame_digest_declared_symbols()
    assert declared == NAMES
    others = set(N.declared_symbols())
    for name in N._EXTENSIONS:
        if name != "frame_digest":
            others |= set(N.declared_symbols(N._extension_header(name)))
    assert not set(declared) & others                                  # the other headers' surfaces are left as they are
    lib = _lib()
    assert lib.snp_frame_digest_indexed_batch.restype is C.c_int and len(lib.snp_frame_digest_indexed_batch.argtypes) == 21
    assert lib.snp_frame_digest_indexed_workspace.restype is C.c_uint64 and len(lib.snp_frame_digest_indexed_workspace.argtypes) == 2
    assert lib.snp_crc32c_combine.restype is C.c_uint32 and len(lib.snp_crc32c_combine.argtypes) == 3


def test_extension_library_exports_exactly_its_header():
    from layouts import exported
    from snappier_amd import _native as N

    ext = exported(N.FRAME_DIGEST_PATH)
    assert ext == set(NAMES)
    for name in N._EXTENSIONS:
        if name != "frame_digest":
            assert not exported(N._extension_path(name)) & ext
    assert not exported(N.PRODUCT_PATH) & ext


def test_workspace_is_host_arithmetic_with_nothing_per_row():
    from snappier_amd import _native as N
    ws, rw = _lib().snp_frame_digest_indexed_workspace, N.frame_index_lib().snp_frame_read_indexed_workspace
    assert ws(0, 0) == 0 and ws(0, 1 << 40) == 0                        # nothing when there is no request
    for nreq in (1, 2, 255, 256, 257, 70000):
        base = ws(nreq, 0)
        assert 0 < base <= 256 * nreq + 64 * 256                        # per-request words and two edge rows (each piece on a 256-byte boundary): no term per interior row
        assert ws(nreq, 12345) - base in range(12345, 12345 + 256)      # + edge_cap bytes (and alignment)
        assert base <= rw(nreq, 0, 0) + 32 * nreq + 1024                # the read's workspace without its chunk slots, + a CRC range and a CRC per edge


def test_null_pointers_and_counts_are_rejected_before_any_device_work():
    call = _lib().snp_frame_digest_indexed_batch
    fake = C.c_void_p(0x1000)

    def args(ctx=fake, ins=(fake,) * 3, ns=1, idx=(fake,) * 5, ne=1, req=(fake,) * 3, nreq=1, ec=0, outs=(fake,) * 3, work=fake, result=fake):
        return (ctx, *ins, ns, *idx, ne, *req, nreq, ec, *outs, work, result)

    assert call(*args(ctx=None)) == O.ERR_BAD_ARG
    assert call(*args(result=None)) == O.ERR_BAD_ARG
    assert call(*args(nreq=0, result=None)) == O.ERR_BAD_ARG           # an empty call still needs d_result
    assert call(*args(nreq=1 << 30)) == O.ERR_BAD_ARG
    assert call(*args(work=None)) == O.ERR_BAD_ARG
    for group, n in (("ins", 3), ("req", 3), ("outs", 3)):
        for i in range(n):
            a = [fake] * n
            a[i] = None
            assert call(*args(**{group: tuple(a)})) == O.ERR_BAD_ARG, (group, i)
    for i in range(5):                                                  # idx_first, idx_total, idx_tail always; the row arrays when there are rows
        a = [fake] * 5
        a[i] = None
        assert call(*args(idx=tuple(a))) == O.ERR_BAD_ARG, i


def test_csharp_binding_matches_the_extension_header():
    import test_csharp_signatures as T
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "snappier_hip_frame_digest.h")).read(), flags=re.S)
    protos = {}
    for m in re.finditer(r"([A-Za-z_][A-Za-z0-9_ ]*?[\s\*]+)(snp_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", text):
        params = [re.match(r"(.*?[\s\*])([A-Za-z_][A-Za-z0-9_]*)$", q.strip()).group(1) for q in m.group(3).split(",") if q.strip() not in ("", "void")]
        protos[m.group(2)] = (T.c_class(m.group(1)), [T.c_class(q) for q in params])
    cs = re.sub(r"//.*", "", open(os.path.join(ROOT, "csharp", "Snappier.Gpu", "NativeMethodsFrameDigest.cs")).read())
    assert 'const string Lib = "snappier_hip_frame_digest"' in cs
    imps = {}
    for m in re.finditer(r"\[DllImport\(Lib, CallingConvention = Cc\)\]\s*internal static extern ([A-Za-z\*]+) (snp_[a-z0-9_]+)\(([^)]*)\);", cs):
        params = [re.match(r"(.*?)\s+([A-Za-z_][A-Za-z0-9_]*)$", q.strip()).group(1) for q in m.group(3).split(",") if q.strip()]
        imps[m.group(2)] = (T.cs_class(m.group(1)), [T.cs_class(q) for q in params])
    assert set(protos) == set(imps) == set(NAMES)
    for name, (ret, params) in protos.items():
        cret, cparams = imps[name]
        assert T.compatible(ret, cret), (name, ret, cret)
        assert len(params) == len(cparams) and all(T.compatible(a, b) for a, b in zip(params, cparams)), (name, params, cparams)
    assert len(protos["snp_frame_digest_indexed_batch"][1]) == 21
    proj = open(os.path.join(ROOT, "csharp", "Snappier.Gpu", "Snappier.Gpu.csproj")).read()
    assert 'Include="../../snappier_amd/libsnappier_hip_frame_digest.so"' in proj


def test_header_says_in_capitals_what_is_not_noticed():
    text = open(os.path.join(ROOT, "include", "snappier_hip_frame_digest.h")).read()
    assert "A CORRUPT BODY OF AN INTERIOR CHUNK IS NOT NOTICED" in text and "THE INDEX IS UNTRUSTED INPUT" in text


# ---- the arithmetic ----------------------------------------------------------------------------------------------------------------------------
def test_shift_table_and_unmask():
    assert D.SHIFT[0] == 0x00800000 and D.crc_shift(0x80000000, 1) == 0x00800000     # 1 * x^8
    assert all(D.SHIFT[k + 1] == D.gf2_mul(D.SHIFT[k], D.SHIFT[k]) for k in range(63))
    for k in range(64):
        assert D.crc_shift(0x80000000, 1 << k) == D.SHIFT[k]
    for c in (0, 1, 0xDEADBEEF, 0xFFFFFFFF, 0xA282EAD8):
        assert D.crc_shift(c, 0) == c and D.gf2_mul(0x80000000, c) == c
        assert D.crc_unmask(O.crc32c(c.to_bytes(4, "little"), masked=True)) == O.crc32c(c.to_bytes(4, "little"), masked=False)
    assert D.crc_shift(0, 12345) == 0
    # a shift is n zero bytes through the raw register: crc(A || 0^n) without the final xor and the init
    a = b"shift me"
    assert D.crc_combine(O.crc32c(a), O.crc32c(bytes(777)), 777) == O.crc32c(a + bytes(777))


def test_combine_matches_the_oracle_on_random_tilings():
    rng = np.random.default_rng(7)
    blob = rng.integers(0, 256, 1 << 20, dtype=np.uint8).tobytes()
    for t in range(60):
        n = int(rng.integers(1, 9))
        lens = [PIECES[int(i)] for i in rng.integers(0, len(PIECES), n)]
        if t < len(PIECES):
            lens[0] = PIECES[t]                                         # every length leads a tiling at least once ...
            lens.append(PIECES[-1 - t])                                 # ... and ends one
        at = int(rng.integers(0, len(blob) - sum(lens) + 1))
        parts, p = [], at
        for m in lens:
            parts.append(blob[p:p + m])
            p += m
        whole = O.crc32c(blob[at:p])
        assert D.combine_all([(O.crc32c(x), len(x)) for x in parts]) == whole, lens
        acc = 0
        for x in parts:                                                 # ... and pairwise, left to right
            acc = D.crc_combine(acc, O.crc32c(x), len(x))
        assert acc == whole, lens


def test_shift_is_a_group_action_up_to_2_63():
    rng = np.random.default_rng(8)
    big = [0, 1, 2, 255, (1 << 32) - 1, 1 << 32, (1 << 32) + 1, (1 << 63) - 1, 1 << 63]
    vals = big + [int(v) >> int(s) for v, s in zip(rng.integers(0, 1 << 63, 40, dtype=np.uint64), rng.integers(0, 63, 40))]
    for i, a in enumerate(vals):
        b = vals[(i * 7 + 3) % len(vals)]
        c = int(rng.integers(0, 1 << 32))
        assert a <= 1 << 63 and b <= 1 << 63
        if a + b <= U64:
            assert D.crc_shift(D.crc_shift(c, a), b) == D.crc_shift(c, a + b), (a, b)
        assert D.crc_shift(D.crc_shift(c, a), b) == D.crc_shift(D.crc_shift(c, b), a)
    # P = (x + 1) * (a primitive polynomial of degree 31): x has order 2^31 - 1 modulo P, so 2^31 - 1 bytes shift nothing
    assert D.crc_shift(0x12345678, (1 << 31) - 1) == 0x12345678 and D.crc_shift(0x12345678, (1 << 32) - 1) != 0x12345678


def test_library_combine_matches_the_model():
    import snappier_amd as S
    comb = _lib().snp_crc32c_combine
    rng = np.random.default_rng(9)
    lens = PIECES + [(1 << 32) - 1, 1 << 32, (1 << 32) + 5, (1 << 40) + 3, (1 << 63), U64]
    for n in lens:
        for _ in range(3):
            a, b = int(rng.integers(0, 1 << 32)), int(rng.integers(0, 1 << 32))
            assert comb(a, b, n) == D.crc_combine(a, b, n) == S.crc32c_combine(a, b, n), n
    x, y = b"left half, ", b"right half"
    assert S.crc32c_combine(O.crc32c(x), O.crc32c(y), len(y)) == O.crc32c(x + y)


# ---- the model of the call ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def named():
    """(names, streams, the model's index of the batch, every window of every stream as a request)."""
    cases = X.named_streams()
    streams = list(cases.values())
    return list(cases), streams, X.build_index(streams), X.all_windows(streams)


@pytest.fixture(scope="module")
def decoded(named):
    """What every stream decodes to, chunk by chunk, up to the first chunk that fails (None from there on is never asked for)."""
    _, streams, _, _ = named
    out = []
    for s in streams:
        parts = []
        for row in R.walk(s)[0]:
            st, data = R.chunk_result(s, row)
            parts.append(data if st == O.OK else None)
        out.append(parts)
    return out


def test_model_is_the_crc_of_the_decoded_window_and_the_reads_status(named, decoded):
    names, streams, ix, requests = named
    need = D.edge_need(streams, ix, requests)
    status, dig_len, digest, result = D.digest_plan(streams, ix, requests, need)
    caps = [U64] * len(requests)
    rstatus, rlen, rdata, _ = X.read_plan(streams, ix, requests, caps, *X.read_needs(streams, ix, requests, caps))
    seen_ok = seen_err = sound_differs = 0
    for r, (b, ro, rl) in enumerate(requests):
        if rstatus[r] == O.OK:
            assert status[r] == O.OK and dig_len[r] == rlen[r] and digest[r] == O.crc32c(rdata[r]), (names[b], ro, rl)
            seen_ok += 1
        elif status[r] != rstatus[r]:
            # the one licensed difference: the read met a corrupt INTERIOR chunk, which the digest never decodes
            k, head, tail, inner, _ = D.request_plan(ix, streams, b, ro, rl)
            assert any(R.chunk_result(streams[b], x)[0] == rstatus[r] for x in inner if x and x[5]), (names[b], ro, rl)
            sound_differs += 1
        else:
            assert digest[r] == 0 and dig_len[r] == 0
            seen_err += 1
    assert seen_ok > 400 and seen_err > 20
    assert result == [result[0], sum(dig_len), need, sum(1 for s in status if s == O.OK)] and result[0] > 0
    # whole streams: no edge, whatever the chunks
    whole = [(b, 0, U64) for b in range(len(streams))]
    st, ln, dg, res = D.digest_plan(streams, ix, whole, 0)
    assert res[2] == 0
    sound = 0
    for b, s in enumerate(streams):
        if st[b] == O.OK and all(x is not None for x in decoded[b]):    # (a stream with a corrupt body is OK too: no chunk of it is decoded)
            assert dg[b] == O.crc32c(b"".join(decoded[b])) and ln[b] == R.walk(s)[1]
            sound += 1
    assert sound > 8


def test_admission_by_edge_cap_is_in_request_order():
    s = R.uniform_stream(5, last=777)[0]
    raw = R.uniform_stream(5, last=777)[1]
    ix = X.build_index([s])
    B = R.B
    requests = [(0, 0, B), (0, 5, 10), (0, B, B), (0, B + 1, 2 * B), (0, 0, U64), (0, 4 * B + 1, 5)]
    edges = [0, B, 0, 2 * B, 0, 777]
    assert D.edge_need([s], ix, requests) == sum(edges)
    for k in range(len(requests) + 1):
        cap = sum(edges[:k])
        status, dig_len, digest, result = D.digest_plan([s], ix, requests, cap)
        admitted = max(i for i in range(len(requests) + 1) if sum(edges[:i]) <= cap)
        for r, (_, ro, rl) in enumerate(requests):
            lo, hi = R.clip(len(raw), ro, rl)
            if r < admitted:
                assert (status[r], dig_len[r], digest[r]) == (O.OK, hi - lo, O.crc32c(raw[lo:hi]))
            else:
                assert (status[r], dig_len[r], digest[r]) == (O.ERR_OUTPUT_TOO_SMALL, 0, 0)
        assert result[2] == sum(edges) and result[3] == admitted


def test_corruption_at_an_edge_is_the_reads_status_and_inside_is_not_noticed():
    B = R.B
    s, raw = R.uniform_stream(5, last=777)
    rows = R.walk(s)[0]
    ix = X.build_index([s])
    req = [(0, B + 5, 2 * B)]                                           # head edge: chunk 1, interior: chunk 2, tail edge: chunk 3
    good = D.digest_plan([s], ix, req, 2 * B)
    assert good[0] == [O.OK] and good[2] == [O.crc32c(raw[B + 5:3 * B + 5])]
    for edge in (1, 3):
        bad = R.corrupt_chunk(s, rows[edge])
        got = D.digest_plan([bad], ix, req, 2 * B)
        want = X.read_plan([bad], ix, req, [U64], 1, 2 * B)[0]
        assert got[0] == want and want[0] != O.OK and got[1] == [0] and got[2] == [0]
    inner = R.corrupt_chunk(s, rows[2])
    assert X.read_plan([inner], ix, req, [U64], 1, 2 * B)[0] != [O.OK]
    assert D.digest_plan([inner], ix, req, 2 * B)[:3] == good[:3]       # never decoded: status OK, digest unchanged
    p = ix["pos"][2] + 4                                                # the header CRC of the interior chunk
    flipped = s[:p] + bytes([s[p] ^ 0x10]) + s[p + 1:]
    got = D.digest_plan([flipped], ix, req, 2 * B)
    assert got[0] == [O.OK] and got[1] == good[1] and got[2] != good[2]


def test_a_stale_index_gives_the_reads_statuses(named):
    names, streams, ix, requests = named
    some = requests[::5]
    caps = [U64] * len(some)
    ne = len(ix["start"])
    rng = np.random.default_rng(3)
    rnd = [int(v) for v in rng.integers(0, 1 << 20, ne)]
    refused = 0
    for index in ({**ix, "pos": [p + 1 for p in ix["pos"]]}, {**ix, "start": [v ^ ((i % 3 == 0) << 9) for i, v in enumerate(ix["start"])]},
                  {**ix, "start": rnd, "pos": list(reversed(rnd))}, {**ix, "first": list(reversed(ix["first"]))},
                  {**ix, "tail": [77] * len(streams)}, {**ix, "start": [], "pos": []}):
        need = D.edge_need(streams, index, some)
        status = D.digest_plan(streams, index, some, need)[0]
        rstatus = X.read_plan(streams, index, some, caps, *X.read_needs(streams, index, some, caps))[0]
        for r, (a, b) in enumerate(zip(status, rstatus)):
            assert a == b or (a == O.OK and b not in (O.OK, O.ERR_BAD_ARG, O.ERR_OUTPUT_TOO_SMALL)), (r, a, b)   # (a corrupt interior chunk of a named stream)
        refused += status.count(O.ERR_BAD_ARG)
    assert refused > 300


# ---- the header on the CPU, under sanitizers -----------------------------------------------------------------------------------------------------
def test_header_under_sanitizers_matches_the_model(named, tmp_path):
    names, streams, ix, requests = named
    ns = len(streams)
    rng = np.random.default_rng(11)
    ne = len(ix["start"])
    sound = [(b, ro & U64, rl & U64, 0) for b, ro, rl in requests]     # (as 64-bit words; the fourth word is the read's capacity: unused)
    some = sound[::3] + [(ns, 0, 10, 0), (0xFFFFFFFF, 5, 5, 0)]

    def rnd(n, hi=1 << 64):
        return [int(v) % hi for v in rng.integers(0, 1 << 63, n, dtype=np.uint64) * 2 + rng.integers(0, 2, n, dtype=np.uint64)]

    lens = [len(s) for s in streams]
    cases = [(ix, sound + [(ns, 0, 10, 0)]),
             ({**ix, "start": rnd(ne), "pos": rnd(ne)}, some),                                 # rows filled with random u64
             ({**ix, "first": rnd(ns + 1), "total": rnd(ns), "start": rnd(ne), "pos": rnd(ne)}, some),
             ({**ix, "start": rnd(ne, 1 << 17), "pos": rnd(ne, 1 << 12), "total": rnd(ns, 1 << 18)}, some),   # small random values: searches go everywhere
             ({**ix, "first": [f + (1 << 33) * (i % 2) for i, f in enumerate(ix["first"])]}, some),        # idx_first beyond nentries
             ({**ix, "first": list(reversed(ix["first"]))}, some),
             ({**ix, "pos": [p + lens[i % ns] for i, p in enumerate(ix["pos"])]}, some),       # positions beyond in_len
             ({**ix, "pos": [max(lens) - 1 - (i % 20) for i in range(ne)]}, some),             # ... and within a few bytes of a stream's end
             ({**ix, "start": list(reversed(ix["start"]))}, some),                             # non-monotone starts
             ({**ix, "start": [v ^ ((i % 3 == 0) << 9) for i, v in enumerate(ix["start"])]}, some),
             ({**ix, "total": [t + (1 << 40) for t in ix["total"]]}, some),                    # totals no row reaches
             ({**ix, "tail": [int(v) % 40 - 20 for v in rng.integers(0, 1000, ns)]}, some),    # tails that are no status
             ({**ix, "start": ix["start"][:ne // 2], "pos": ix["pos"][:ne // 2]}, some),       # fewer rows than idx_first says
             ({**ix, "start": [], "pos": []}, some)]
    shifts = [(c, n) for c in (0, 1, 0x80000000, 0xFFFFFFFF, 0x9E3779B9)
              for n in PIECES + [(1 << 32) - 1, 1 << 32, (1 << 32) + 1, 65537 * 65536, (1 << 40) + 7, (1 << 63) - 1, 1 << 63, U64]]
    spath, cpath = str(tmp_path / "shifts.bin"), str(tmp_path / "cases.bin")
    D.write_shifts(spath, shifts)
    X.write_cases(cpath, streams, cases)
    exe = str(tmp_path / "frame_digest_plan_check")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host",
                    "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "abi", "frame_digest_plan_check.hip"), "-o", exe,
                    "-Wl,-rpath,/opt/rocm/lib"], check=True)
    env = {**os.environ, "ASAN_OPTIONS": "detect_leaks=1:abort_on_error=0", "UBSAN_OPTIONS": "print_stacktrace=1:halt_on_error=1"}
    run = subprocess.run([exe, spath, cpath], capture_output=True, text=True, env=env)
    assert run.returncode == 0 and run.stderr == "", run.stderr[-3000:]      # the sanitizers are silent
    lines = run.stdout.splitlines()
    assert len(lines) == len(shifts) + sum(len(reqs) for _, reqs in cases)
    for line, (c, n) in zip(lines, shifts):
        assert int(line) == D.crc_shift(c, n), (c, n)
    at = len(shifts)
    refused = planned = 0
    for c, (index, reqs) in enumerate(cases):
        for b, ro, rl, _ in reqs:
            want = D.plan_line(index, streams, (b, ro, rl))
            assert lines[at] == want, (c, names[b] if b < ns else b, ro, rl)
            f = want.split()
            refused += c > 0 and (f[0] == str(O.ERR_BAD_ARG) or f[5] != "0")
            planned += c > 0 and f[0] == "0" and f[5] == "0"
            at += 1
    assert refused > 500 and planned > 100                            # both outcomes, on the unsound indexes
    first = [line.split() for line in lines[len(shifts):len(shifts) + len(sound)]]
    assert all(f[5] == "0" and f[0] != str(O.ERR_BAD_ARG) for f in first) and sum(1 for f in first if f[6] != "0") > 200

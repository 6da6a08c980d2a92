"""snp_frame_encode_chunked_batch (libsnappier_hip_frame_chunked.so) without a GPU: the declarations and their C# binding, the workspace
arithmetic and the staging stride, argument rejection; the Python model of the contract (frame_chunked_model.py) checked against the oracle's
whole-stream encoder and decoder and against the index model's walk of its own streams; the admission and out_cap plans; and the planning
header (csrc/frame_chunked_device.h) itself, compiled for the CPU under AddressSanitizer and UBSan into a stand-alone program
(tests/abi/frame_chunked_plan_check.hip) and run over cases the model writes out, buffers past 4 GiB among them."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import frame_chunked_model as K
import frame_index_model as X
import oracle as O
from conftest import ROOT, read_testdata

NAMES = ["snp_frame_encode_chunked_batch", "snp_frame_encode_chunked_workspace"]


def _lib():
    from snappier_amd import _native as N
    return N.frame_chunked_lib()


# ---- the surface -----------------------------------------------------------------------------------------------------------------------------
def test_header_and_binding_declare_the_new_functions():
    from snappier_amd import _native as N
    declared = N.frame_chunked_declared_symbols()
    assert declared == NAMES
    others = set(N.declared_symbols()) | set(N.buffers_declared_symbols()) | set(N.buffers_decompress_declared_symbols()) | \
        set(N.frame_buffers_declared_symbols()) | set(N.layout_declared_symbols()) | set(N.frame_range_declared_symbols()) | \
        set(N.frame_index_declared_symbols())
    assert not set(declared) & others                                  # the other headers' surfaces are left as they are
    lib = _lib()
    assert lib.snp_frame_encode_chunked_batch.restype is C.c_int and len(lib.snp_frame_encode_chunked_batch.argtypes) == 19
    assert lib.snp_frame_encode_chunked_workspace.restype is C.c_uint64 and len(lib.snp_frame_encode_chunked_workspace.argtypes) == 3


def test_extension_library_exports_exactly_its_header():
    from layouts import exported
    from snappier_amd import _native as N

    ext = exported(N.FRAME_CHUNKED_PATH)
    assert ext == set(NAMES)
    for other in (N.PRODUCT_PATH, N.BUFFERS_PATH, N.BUFFERS_DECOMPRESS_PATH, N.FRAME_BUFFERS_PATH, N.LAYOUT_PATH, N.FRAME_RANGE_PATH, N.FRAME_INDEX_PATH):
        assert not exported(other) & ext


def test_workspace_is_host_arithmetic_and_the_stride_follows_the_rule():
    from snappier_amd import _native as N
    ws = _lib().snp_frame_encode_chunked_workspace
    old = N.frame_buffers_lib().snp_frame_encode_buffers_workspace
    assert ws(0, 0, 4096) == 0 and ws(0, 5000, 65536) == 0              # nothing when there is no buffer
    for cb in K.CHUNK_SIZES + [1024, 40000]:
        # the stride: snp_max_compressed_length(cb) rounded up to 16, plus 16 -- the staging is one 256-byte piece of max_chunks strides
        rule = (N.lib().snp_max_compressed_length(cb) + 15) // 16 * 16 + 16
        assert K.stride(cb) == rule
        for nb in (1, 2, 255, 1024, 1025, 300000):
            for mc in (0, 1, 255, 4096, 70001):
                w = ws(nb, mc, cb)
                assert w % 256 == 0
                assert ws(nb, mc + 1, cb) >= w and ws(nb + 1, mc, cb) >= w              # monotone
                staging = (mc * rule + 255) // 256 * 256
                assert w - staging == ws(nb, mc, 1) - (mc * K.stride(1) + 255) // 256 * 256    # everything else does not depend on the chunk size
                if cb == 65536:
                    assert w == old(nb, mc)                                             # the pieces of snp_frame_encode_buffers_batch
    assert K.stride(65536) == 76496 + 16 and K.stride(4096) == 4832 and K.stride(1) == 64
    # 4 KiB chunks: the workspace of n bytes of input is about 1.2 x n, as at 64 KiB (a fixed 64 KiB stride would make it 19 x)
    n = 10 << 30
    for cb in (65536, 16384, 4096):
        assert 1.16 < ws(1, n // cb, cb) / n < 1.25, cb
    assert ws(1, n // 1024, 1024) / n < 1.3 and ws(1, n // 256, 256) / n < 1.6         # (the 32 + 16 + 16 bytes per slot begin to show)
    assert ws(0x7FFFFFFF, 0xFFFFFFFF, 65536) > 0xFFFFFFFF * 76496        # (64-bit arithmetic)


def test_batch_call_rejects_bad_arguments_without_a_device():
    enc = _lib().snp_frame_encode_chunked_batch
    fake = C.c_void_p(64)                                               # (never dereferenced: the arguments are refused first)
    n3, n5, f3, f5 = [None] * 3, [None] * 5, [fake] * 3, [fake] * 5
    # ctx, in / in_off / in_len, nbuffers, chunk_bytes, max_chunks, out / out_off / out_cap / out_len / status, the five index arrays, d_work, d_result
    assert enc(None, *n3, 0, 4096, 0, *n5, *n5, None, None) == O.ERR_BAD_ARG
    assert enc(fake, *n3, 0, 4096, 0, *n5, *n5, None, None) == O.ERR_BAD_ARG                       # no d_result
    assert enc(fake, *n3, 1, 4096, 0, *n5, *n5, None, fake) == O.ERR_BAD_ARG                       # buffers, no arrays
    assert enc(fake, *f3, 1, 4096, 1, *f5, *n5, None, fake) == O.ERR_BAD_ARG                       # no d_work
    assert enc(fake, *f3, 1, 0, 1, *f5, *f5, fake, fake) == O.ERR_BAD_ARG                          # chunk_bytes 0
    assert enc(fake, *f3, 1, 65537, 1, *f5, *f5, fake, fake) == O.ERR_BAD_ARG                      # ... and above what a chunk may hold
    assert enc(fake, *f3, 1, 65537, 1, *f5, *n5, fake, fake) == O.ERR_BAD_ARG
    assert enc(fake, *n3, 0, 0, 0, *n5, *n5, None, fake) == O.ERR_BAD_ARG                          # ... also in an empty batch
    for given in range(1, 31):                                                                     # an index given in part
        ix = [fake if given >> i & 1 else None for i in range(5)]
        assert enc(fake, *f3, 1, 4096, 1, *f5, *ix, fake, fake) == O.ERR_BAD_ARG, given
        assert enc(fake, *n3, 0, 4096, 0, *n5, *ix, None, fake) == O.ERR_BAD_ARG, given
    for i in range(9):                                                                             # any one null among the nine arrays of a batch
        a = [fake] * 9
        a[i] = None
        assert enc(fake, *a[:3], 1, 4096, 1, *a[3:8], *f5, a[8], fake) == O.ERR_BAD_ARG, i


def test_csharp_binding_matches_the_extension_header():
    import test_csharp_signatures as T
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "snappier_hip_frame_chunked.h")).read(), flags=re.S)
    protos = {}
    for m in re.finditer(r"([A-Za-z_][A-Za-z0-9_ ]*?[\s\*]+)(snp_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", text):
        params = [re.match(r"(.*?[\s\*])([A-Za-z_][A-Za-z0-9_]*)$", q.strip()).group(1) for q in m.group(3).split(",") if q.strip() not in ("", "void")]
        protos[m.group(2)] = (T.c_class(m.group(1)), [T.c_class(q) for q in params])
    cs = re.sub(r"//.*", "", open(os.path.join(ROOT, "csharp", "Snappier.Gpu", "NativeMethodsFrameChunked.cs")).read())
    assert 'const string Lib = "snappier_hip_frame_chunked"' in cs
    imps = {}
    for m in re.finditer(r"\[DllImport\(Lib, CallingConvention = Cc\)\]\s*internal static extern ([A-Za-z\*]+) (snp_[a-z0-9_]+)\(([^)]*)\);", cs):
        params = [re.match(r"(.*?)\s+([A-Za-z_][A-Za-z0-9_]*)$", q.strip()).group(1) for q in m.group(3).split(",") if q.strip()]
        imps[m.group(2)] = (T.cs_class(m.group(1)), [T.cs_class(q) for q in params])
    assert set(protos) == set(imps) == set(NAMES)
    for name, (ret, params) in protos.items():
        cret, cparams = imps[name]
        assert T.compatible(ret, cret), (name, ret, cret)
        assert len(params) == len(cparams) and all(T.compatible(a, b) for a, b in zip(params, cparams)), (name, params, cparams)
    assert len(protos["snp_frame_encode_chunked_batch"][1]) == 19 and len(protos["snp_frame_encode_chunked_workspace"][1]) == 3
    proj = open(os.path.join(ROOT, "csharp", "Snappier.Gpu", "Snappier.Gpu.csproj")).read()
    assert 'Include="../../snappier_amd/libsnappier_hip_frame_chunked.so"' in proj


# ---- the model checks itself ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def content():
    html = read_testdata("html")
    rnd = np.random.default_rng(3).integers(0, 256, 200000, dtype=np.uint8).tobytes()
    return html, rnd


def test_at_65536_the_model_is_the_oracles_frame_encoder(content):
    html, rnd = content
    for variant in (O.HASH_CRC32C, O.HASH_MUL):
        for raw in (b"", b"a", html[:65535], html[:65536], html[:65537], html, rnd[:70001], html[:50000] + rnd[:100000]):
            assert K.stream_of(raw, 65536, variant) == O.frame_encode(raw, variant)


def test_every_chunk_size_decodes_to_the_input_and_indexes_like_the_walk(content):
    html, rnd = content
    kinds = set()
    for cb in K.CHUNK_SIZES + [1000]:
        blobs = [html[:n] for n in K.buffer_lengths(cb)] + [rnd[:min(2 * cb + 3, 70001)]]
        for variant in (O.HASH_CRC32C, O.HASH_MUL):
            m = K.encode(blobs, cb, variant)
            assert m["status"] == [O.OK] * len(blobs) and m["result"][3] == len(blobs)
            for raw, s in zip(blobs, m["streams"]):
                assert O.frame_decode(s) == raw and len(s) <= K.frame_cap(len(raw), cb)
                kinds |= {(cb, s[p]) for p in X.index_of(s)[1]}
            # the index of an all-OK batch is what snp_frame_index_batch's model gives over the emitted streams
            ix = X.build_index(m["streams"])
            assert [m[k] for k in ("first", "start", "pos", "total", "tail")] == [ix[k] for k in ("first", "start", "pos", "total", "tail")]
            assert m["result"] == [sum(K.nchunks(len(x), cb) for x in blobs), sum(len(s) for s in m["streams"]), len(ix["start"]), len(blobs)]
            assert m["result"][:2] == [ix["result"][0], sum(m["out_len"])]
    # both chunk types at every size that can have both: a piece of up to 16 bytes is varint + one literal, two bytes MORE than the piece
    # (the scan's first probe needs 17), so below 17 every chunk is type 0x01
    for cb in K.CHUNK_SIZES:
        assert (cb, 1) in kinds and ((cb, 0) in kinds if cb > 17 else cb == 17 or (cb, 0) not in kinds), cb


def test_admission_is_a_prefix_and_out_cap_fails_a_buffer_alone(content):
    html, rnd = content
    cb = 1000
    blobs = [html[:2500], rnd[:999], b"", html[:7001], rnd[:1000], html[:1]]
    full = K.encode(blobs, cb)
    need = full["result"][0]
    assert need == 3 + 1 + 0 + 8 + 1 + 1 and full["first"] == [0, 3, 4, 4, 12, 13, 14]
    assert K.encode(blobs, cb, max_chunks=need + 7) == full             # a loose bound changes nothing
    short = K.encode(blobs, cb, max_chunks=need - 3)                    # three short: the 8-chunk buffer and every later one
    assert short["status"] == [O.OK] * 3 + [O.ERR_OUTPUT_TOO_SMALL] * 3 and short["out_len"][3:] == [0, 0, 0]
    assert short["streams"][:3] == full["streams"][:3] and short["streams"][3:] == [None] * 3
    assert short["first"] == [0, 3, 4, 4, 4, 4, 4] and short["tail"][3:] == [O.ERR_OUTPUT_TOO_SMALL] * 3 and short["total"][3:] == [0] * 3
    assert short["result"] == [need, sum(full["out_len"][:3]), 4, 3]
    sizing = K.encode(blobs, cb, max_chunks=0)                          # the empty buffer needs no slot, but comes after one that does
    assert sizing["status"] == [O.ERR_OUTPUT_TOO_SMALL] * 6 and sizing["result"] == [need, 0, 0, 0]
    assert K.encode([b"", b""], cb, max_chunks=0)["status"] == [O.OK, O.OK]
    # out_cap: exact fits, one byte short fails that buffer alone; its rows are taken out, the later buffers' rows move down
    caps = list(full["out_len"])
    assert K.encode(blobs, cb, caps=caps) == full
    caps[3] -= 1
    mid = K.encode(blobs, cb, caps=caps)
    assert mid["status"] == [O.OK] * 3 + [O.ERR_OUTPUT_TOO_SMALL] + [O.OK] * 2
    assert mid["first"] == [0, 3, 4, 4, 4, 5, 6] and mid["result"] == [need, sum(full["out_len"]) - full["out_len"][3], 6, 5]
    assert mid["start"] == full["start"][:4] + full["start"][12:] and mid["pos"] == full["pos"][:4] + full["pos"][12:]
    assert mid["total"] == [2500, 999, 0, 0, 1000, 1] and mid["tail"][3] == O.ERR_OUTPUT_TOO_SMALL
    assert K.encode([], cb)["result"] == [0] * 4 and K.encode([], cb)["first"] == [0]
    none = K.encode(blobs, cb, caps=caps, with_index=False)             # without an index nothing but result[2] differs
    assert (none["status"], none["out_len"], none["streams"]) == (mid["status"], mid["out_len"], mid["streams"])
    assert none["result"] == mid["result"][:2] + [0] + mid["result"][3:] and none["first"] == []


# ---- the planning header on the CPU, under sanitizers ------------------------------------------------------------------------------------------
def test_planning_header_under_sanitizers_matches_the_model(tmp_path):
    OKS, BAD = O.OK, O.ERR_OUTPUT_TOO_SMALL
    big = (1 << 32) + 5
    cases = []

    def case(in_len, cb, max_chunks=None, status=None):
        first = K.first_slots(in_len, cb)
        mc = min(first[-1], 0xFFFFFFFF) if max_chunks is None else max_chunks
        st = [OKS if first[b + 1] <= mc else BAD for b in range(len(in_len))] if status is None else status
        cases.append((in_len, st, cb, mc, K.interesting_slots(first, mc)))

    case([big], 4096)                                                   # 1 048 577 slots: k * cb passes 2^32 at the last ones
    case([7, big, 4097], 4096)
    case([big], 1)                                                      # 2^32 + 5 chunks: more than a buffer may hold, it is never admitted
    case([3, big, 2], 1, 0xFFFFFFFF)
    case([(1 << 40) + 1], 65536)
    case([(1 << 40) + 1], 256, 0xFFFFFFFF)                              # 2^32 + 1 chunks of 256 bytes
    case([(1 << 40) - 511], 256, 0xFFFFFFFF)                            # 2^32 - 1 chunks: admitted, the last slot (one byte) is u32's last but one
    case([2500, 999, 0, 7001, 1000, 1], 1000, status=[OKS, OKS, OKS, BAD, OKS, OKS])     # the middle buffer failed out_cap
    case([2500, 999, 0, 7001, 1000, 1], 1000, 11)                       # three short
    case([2500, 999, 0, 7001, 1000, 1], 1000, 20)                       # loose
    case([63, 70001, 129], 64)
    case([0, 0, 0], 17)
    case([], 4096)
    for cb in K.CHUNK_SIZES + [32768, 32769, 21846, 21845]:
        case(K.buffer_lengths(cb), cb)
    path = str(tmp_path / "cases.bin")
    K.write_cases(path, cases)
    exe = str(tmp_path / "frame_chunked_plan_check")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host",
                    "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "abi", "frame_chunked_plan_check.hip"), "-o", exe,
                    "-Wl,-rpath,/opt/rocm/lib"], check=True)
    env = {**os.environ, "ASAN_OPTIONS": "detect_leaks=1:abort_on_error=0", "UBSAN_OPTIONS": "print_stacktrace=1:halt_on_error=1"}
    run = subprocess.run([exe, path], capture_output=True, text=True, env=env)
    assert run.returncode == 0 and run.stderr == "", run.stderr[-3000:]      # the sanitizers are silent
    lines = run.stdout.splitlines()
    want = [line for in_len, st, cb, mc, slots in cases for line in K.plan_lines(in_len, st, cb, mc, slots)]
    assert len(lines) == len(want)
    for i, (got, exp) in enumerate(zip(lines, want)):
        assert got == exp, i
    # the cases reach what they are for: offsets and starts past 2^32, a buffer that is never admitted, rows that moved down
    first = K.plan_lines([big], [OKS], 4096, 1048577, [1048576])
    assert first == ["1048577 1048577 16 64", "0 5 1048576 4294967296 %d 1048576 4294967296" % (1048576 * 4832)]
    assert K.plan_lines([big], [BAD], 1, 0xFFFFFFFF, [0, 0xFFFFFFFF]) == ["4294967301 0 65536 64", "-1 0 0 0 0 0 0", "-1 0 0 0 %d 0 0" % (0xFFFFFFFF * 64)]
    moved = K.plan_lines([2500, 999, 0, 7001, 1000, 1], [OKS, OKS, OKS, BAD, OKS, OKS], 1000, 14, [3, 4, 12, 13])
    assert moved == ["14 6 66 64", "1 999 0 0 %d 3 0" % (3 * K.stride(1000)), "3 1000 0 0 %d 0 0" % (4 * K.stride(1000)),
                     "4 1000 0 0 %d 4 0" % (12 * K.stride(1000)), "5 1 0 0 %d 5 0" % (13 * K.stride(1000))]

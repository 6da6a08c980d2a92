"""snp_compress_buffers_batch (libsnappier_hip_buffers.so) without a GPU: the workspace arithmetic, the declarations and their C# binding, and a NumPy statement of the plan / scan / emit
arithmetic of csrc/buffers.hip checked against the oracle -- the concatenation that the device kernels perform, pinned on the CPU."""
import ctypes as C

import numpy as np
import pytest

import oracle as O
from conftest import read_testdata

B = 65536
STAGE_STRIDE = 76512          # kSnpCompStride (capi_internal.h): staging bytes per fragment slot


def varint_len(n: int) -> int:
    return 1 if n < 1 << 7 else 2 if n < 1 << 14 else 3 if n < 1 << 21 else 4 if n < 1 << 28 else 5


def fragment_body(piece: bytes, variant: int) -> bytes:
    """CompressFragment of one <= 64 KiB piece: the oracle's block minus its varint (what the compressor writes with emit_varint = 0)."""
    return O.compress(piece, variant)[varint_len(len(piece)):]


def model(data: bytes, in_off, in_len, max_fragments: int, out_off, out_cap, variant: int, out_size: int, sentinel: int = 0xA5):
    """The device pipeline in NumPy: -> (out bytes, out_len, status, result)."""
    nb = len(in_len)
    nf = np.array([(n + B - 1) // B for n in in_len], dtype=np.uint64)
    first = np.zeros(nb + 1, dtype=np.uint64)
    first[1:] = np.cumsum(nf)                                   # k_scan_*<FRAGS>: exclusive scan, first[nb] = fragments needed
    # plan: slot f -> owner, input range (empty slots past the batch and for buffers that do not fit)
    owner = np.full(max_fragments, -1, dtype=np.int64)
    comp_len = np.zeros(max_fragments, dtype=np.uint64)
    stage = {}
    for f in range(max_fragments):
        if f >= first[nb]:
            continue
        b = int(np.searchsorted(first, f, side="right") - 1)
        if first[b + 1] > max_fragments:
            continue
        k = f - int(first[b])
        o, n = in_off[b] + k * B, min(B, in_len[b] - k * B)
        owner[f] = b
        stage[f] = fragment_body(data[o:o + n], variant)
        assert len(stage[f]) <= STAGE_STRIDE
        comp_len[f] = len(stage[f])
    scan = np.zeros(max_fragments + 1, dtype=np.uint64)
    scan[1:] = np.cumsum(comp_len)
    # sizes
    out = bytearray([sentinel]) * out_size
    out_len = np.zeros(nb, dtype=np.int64)
    status = np.full(nb, O.ERR_OUTPUT_TOO_SMALL, dtype=np.int32)
    for b in range(nb):
        if first[b + 1] <= max_fragments:
            size = varint_len(in_len[b]) + int(scan[first[b + 1]] - scan[first[b]])
            if size <= out_cap[b]:
                out_len[b], status[b] = size, O.OK
                out[out_off[b]:out_off[b] + varint_len(in_len[b])] = O.varint_write(in_len[b])
    # emit: one copy per fragment slot
    for f in range(max_fragments):
        b = owner[f]
        if b < 0 or status[b] != O.OK:
            continue
        o = out_off[b] + varint_len(in_len[b]) + int(scan[f] - scan[first[b]])
        out[o:o + len(stage[f])] = stage[f]
    return bytes(out), out_len, status, (int(first[nb]), int(out_len[status == O.OK].sum()))


def _lib():
    from snappier_amd import _native as N
    return N.buffers_lib()


def test_workspace_arithmetic():
    L = _lib()
    ws = L.snp_compress_buffers_workspace
    assert ws(0, 0) == 0 and ws(0, 1000) == 0
    prev = 0
    for nb in (1, 2, 255, 256, 1023, 1024, 1025, 100000):
        for nf in (0, 1, 1023, 1024, 1025, 163840):
            w = ws(nb, nf)
            assert w % 256 == 0 and w >= nf * STAGE_STRIDE + (nb + 1) * 8
            assert ws(nb, nf + 1) >= w and ws(nb + 1, nf) >= w
        assert ws(nb, 0) >= prev
        prev = ws(nb, 0)
    assert ws(0xFFFFFFFF, 0xFFFFFFFF) > 0xFFFFFFFF * STAGE_STRIDE      # (64-bit arithmetic)


def test_header_and_binding_declare_the_new_functions():
    from snappier_amd import _native as N
    declared = N.buffers_declared_symbols()
    assert declared == ["snp_compress_buffers_batch", "snp_compress_buffers_workspace"]
    assert not set(declared) & set(N.declared_symbols())               # the extension leaves snappier_hip.h's surface as it is
    L = _lib()
    assert L.snp_compress_buffers_batch.restype is C.c_int and len(L.snp_compress_buffers_batch.argtypes) == 13
    assert L.snp_compress_buffers_workspace.restype is C.c_uint64


def test_extension_library_exports_exactly_its_header():
    """libsnappier_hip_buffers.so exports the functions of include/snappier_hip_buffers.h, nothing else of the snp_ namespace; the product
    library does not export them."""
    from layouts import exported
    from snappier_amd import _native as N

    ext = exported(N.BUFFERS_PATH)
    assert ext == set(N.buffers_declared_symbols())
    assert not exported(N.PRODUCT_PATH) & ext


def test_csharp_binding_matches_the_extension_header():
    """csharp/Snappier.Gpu/NativeMethodsBuffers.cs against include/snappier_hip_buffers.h, by ABI class, as test_csharp_signatures.py does for
    NativeMethods.cs and snappier_hip.h."""
    import os
    import re
    import test_csharp_signatures as T
    from conftest import ROOT
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "snappier_hip_buffers.h")).read(), flags=re.S)
    protos = {}
    for m in re.finditer(r"([A-Za-z_][A-Za-z0-9_ ]*?[\s\*]+)(snp_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", text):
        params = [re.match(r"(.*?[\s\*])([A-Za-z_][A-Za-z0-9_]*)$", q.strip()).group(1) for q in m.group(3).split(",") if q.strip() not in ("", "void")]
        protos[m.group(2)] = (T.c_class(m.group(1)), [T.c_class(q) for q in params])
    cs = re.sub(r"//.*", "", open(os.path.join(ROOT, "csharp", "Snappier.Gpu", "NativeMethodsBuffers.cs")).read())
    assert 'const string Lib = "snappier_hip_buffers"' in cs
    imps = {}
    for m in re.finditer(r"\[DllImport\(Lib, CallingConvention = Cc\)\]\s*internal static extern ([A-Za-z\*]+) (snp_[a-z0-9_]+)\(([^)]*)\);", cs):
        params = [re.match(r"(.*?)\s+([A-Za-z_][A-Za-z0-9_]*)$", q.strip()).group(1) for q in m.group(3).split(",") if q.strip()]
        imps[m.group(2)] = (T.cs_class(m.group(1)), [T.cs_class(q) for q in params])
    assert set(protos) == set(imps) == {"snp_compress_buffers_batch", "snp_compress_buffers_workspace"}
    for name, (ret, params) in protos.items():
        cret, cparams = imps[name]
        assert T.compatible(ret, cret), (name, ret, cret)
        assert len(params) == len(cparams) and all(T.compatible(a, b) for a, b in zip(params, cparams)), (name, params, cparams)


def test_batch_call_rejects_null_pointers_without_a_device():
    L = _lib()
    assert L.snp_compress_buffers_batch(None, None, None, None, 0, 0, None, None, None, None, None, None, None) == O.ERR_BAD_ARG


@pytest.mark.parametrize("variant", [O.HASH_CRC32C, O.HASH_MUL])
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_plan_and_emit_model_concatenates_to_the_oracle(variant, seed):
    rng = np.random.default_rng(seed)
    html = read_testdata("html") * 8 + read_testdata("kppkn.gtb")
    lens = [0, 1, 15, 65535, 65536, 65537, 131073, 3] + [int(x) for x in rng.integers(0, 300000, 6)]
    rng.shuffle(lens)
    in_off = [int(rng.integers(0, len(html) - n + 1)) for n in lens]
    cap = [32 + n + n // 6 + 1 + 5 for n in lens]
    out_off, o = [], 7
    for c in cap:
        out_off.append(o)
        o += c + 13                                            # gaps the emit must leave alone
    exact = sum((n + B - 1) // B for n in lens)
    assert _lib().snp_compress_buffers_workspace(len(lens), exact) >= exact * STAGE_STRIDE   # the staging the model uses fits the declared workspace
    out, out_len, status, result = model(html, in_off, lens, exact, out_off, cap, variant, o)
    assert (status == O.OK).all() and result == (exact, int(out_len.sum()))
    for b, n in enumerate(lens):
        assert out[out_off[b]:out_off[b] + out_len[b]] == O.compress(html[in_off[b]:in_off[b] + n], variant)
        end = out_off[b + 1] if b + 1 < len(lens) else o
        assert set(out[out_off[b] + out_len[b]:end]) <= {0xA5}
    # a loose bound gives the same bytes; a short one fails the buffer that does not fit and every later one, and says what was needed
    assert model(html, in_off, lens, exact + 5, out_off, cap, variant, o)[0] == out
    short = exact - 1
    out2, len2, st2, res2 = model(html, in_off, lens, short, out_off, cap, variant, o)
    assert res2[0] == exact
    firsts = np.concatenate([[0], np.cumsum([(n + B - 1) // B for n in lens])])
    for b in range(len(lens)):
        fits = firsts[b + 1] <= short
        assert st2[b] == (O.OK if fits else O.ERR_OUTPUT_TOO_SMALL)
        if fits:
            assert out2[out_off[b]:out_off[b] + len2[b]] == out[out_off[b]:out_off[b] + out_len[b]]
        else:
            assert len2[b] == 0 and set(out2[out_off[b]:out_off[b] + cap[b]]) == {0xA5}
    # exact capacity fits, one byte less does not and leaves the range alone
    cap3 = list(cap)
    cap3[0] = int(out_len[0]) - 1
    _, len3, st3, _ = model(html, in_off, lens, exact, out_off, cap3, variant, o)
    assert st3[0] == O.ERR_OUTPUT_TOO_SMALL and len3[0] == 0 and (st3[1:] == O.OK).all()

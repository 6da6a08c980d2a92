"""snp_decompress_buffers_batch (libsnappier_hip_buffers_decompress.so) without a GPU: the workspace arithmetic, null-pointer checks, the
declarations and their C# binding, and a NumPy statement of the plan of csrc/buffers_decode.hip -- classification, the makespan rule, admission in
buffer order, the chunk bound that sizes the workspace from max_fragments alone, and the ticket -> (block, chunk) map -- checked against a serial
walk."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import oracle as O
from conftest import ROOT

B = 65536
CHUNK = 16384
SPLIT_FACTOR = 2            # kSplitFactor (buffers_decode.hip)
SLOTS_PER_FRAGMENT = 7      # kSlotsPerFragment


def _lib():
    from snappier_amd import _native as N
    return N.buffers_decompress_lib()


def varint(v: int) -> bytes:
    out = bytearray()
    while v >= 128:
        out.append((v & 0x7F) | 0x80)
        v >>= 7
    out.append(v)
    return bytes(out)


def max_compressed(n: int) -> int:
    """snp_max_compressed_length: -1 above 2^31 - 1."""
    v = 32 + n + n // 6 + 1 + 5
    return -1 if v > 0x7FFFFFFF else v


def preamble(block: bytes):
    """-> (clean, declared, hb) as decompress_spans and k_bd_classify read the varint."""
    expected = hb = shift = 0
    for i in range(min(5, len(block))):
        ch = block[i]
        val = ch & 0x7F
        if val & ~(0xFFFFFFFF >> shift) & 0xFFFFFFFF:
            break
        expected |= val << shift
        shift += 7
        hb = i + 1
        if ch < 128:
            return True, expected, hb
    return False, expected, hb


def plan(blocks, out_cap, par_min, wave_slots, max_fragments):
    """The device plan in NumPy: -> dict of per-block arrays and the totals."""
    nb = len(blocks)
    decl = np.zeros(nb, np.uint64)
    hbv = np.zeros(nb, np.uint64)
    for b, blk in enumerate(blocks):
        clean, d, hb = preamble(blk)
        mc = max_compressed(d)
        cand = clean and par_min and d >= par_min and d <= out_cap[b] and len(blk) > hb and mc >= 0 and len(blk) <= mc
        decl[b] = d if cand else 0
        hbv[b] = hb
    total = int(decl.sum())
    chosen_frags = np.array([(int(d) + B - 1) // B if d and int(d) * wave_slots >= SPLIT_FACTOR * total else 0 for d in decl], np.uint64)
    first = np.zeros(nb + 1, np.uint64)
    first[1:] = np.cumsum(chosen_frags)
    adm = (first[1:] > first[:-1]) & (first[1:] <= max_fragments)
    chunks = np.array([(len(blk) - int(h) + CHUNK - 1) // CHUNK if a else 0 for blk, h, a in zip(blocks, hbv, adm)], np.uint64)
    chunk_first = np.zeros(nb + 1, np.uint64)
    chunk_first[1:] = np.cumsum(chunks)
    rank = np.zeros(nb + 1, np.uint64)
    rank[1:] = np.cumsum(adm.astype(np.uint64))
    slot = chunk_first + 2 * rank
    return dict(decl=decl, first=first, admitted=adm, chunks=chunks, chunk_first=chunk_first, rank=rank, slot=slot,
                needed=int(first[nb]))


def find_block(key, nb, t):
    """owner_of of scan_tiles.h (buffers_decode.hip calls it with key functors): the last b in [0, nb) with key[b] <= t."""
    lo, hi = 0, nb
    while hi - lo > 1:
        mid = lo + (hi - lo) // 2
        if key[mid] <= t:
            lo = mid
        else:
            hi = mid
    return lo


def test_workspace_arithmetic():
    ws = _lib().snp_decompress_buffers_workspace
    assert ws(0, 0) == 0 and ws(0, 1000) == 0
    assert ws(1, 0) > 0                                              # (0 fragments: the per-block arrays only)
    for nb in (1, 2, 255, 256, 1023, 1024, 1025, 100000):
        for nf in (0, 1, 255, 256, 257, 1024, 163840):
            w = ws(nb, nf)
            assert w % 256 == 0 and w >= nb * 4 * 5 + nf * 40
            assert ws(nb, nf + 1) >= w and ws(nb + 1, nf) >= w
    assert ws(0xFFFFFFFF, 0xFFFFFFFF) > 0xFFFFFFFF * 64             # (64-bit arithmetic)
    assert ws(10, 0xFFFFFFFF) == ws(10, 1 << 26)                     # (max_fragments counts up to 2^26)


def test_batch_call_rejects_null_pointers_without_a_device():
    L = _lib()
    assert L.snp_decompress_buffers_batch(None, None, None, None, 0, 0, None, None, None, None, None, None, None) == O.ERR_BAD_ARG
    assert L.snp_decompress_buffers_batch(None, None, None, None, 4, 16, None, None, None, None, None, None, None) == O.ERR_BAD_ARG


def test_header_binding_and_exports():
    """The new library exports exactly its header's functions under snp_; the product and compress-side libraries export neither."""
    from layouts import exported
    from snappier_amd import _native as N
    declared = N.buffers_decompress_declared_symbols()
    assert declared == ["snp_decompress_buffers_batch", "snp_decompress_buffers_workspace"]
    assert not set(declared) & set(N.declared_symbols()) and not set(declared) & set(N.buffers_declared_symbols())
    L = _lib()
    assert L.snp_decompress_buffers_batch.restype is C.c_int and len(L.snp_decompress_buffers_batch.argtypes) == 13
    assert exported(N.BUFFERS_DECOMPRESS_PATH) == set(declared)
    assert not exported(N.PRODUCT_PATH) & set(declared) and not exported(N.BUFFERS_PATH) & set(declared)


def test_csharp_binding_matches_the_header():
    import test_csharp_signatures as T
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "snappier_hip_buffers_decompress.h")).read(), flags=re.S)
    protos = {}
    for m in re.finditer(r"([A-Za-z_][A-Za-z0-9_ ]*?[\s\*]+)(snp_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", text):
        params = [re.match(r"(.*?[\s\*])([A-Za-z_][A-Za-z0-9_]*)$", q.strip()).group(1) for q in m.group(3).split(",") if q.strip() not in ("", "void")]
        protos[m.group(2)] = (T.c_class(m.group(1)), [T.c_class(q) for q in params])
    cs = re.sub(r"//.*", "", open(os.path.join(ROOT, "csharp", "Snappier.Gpu", "NativeMethodsBuffersDecompress.cs")).read())
    assert 'const string Lib = "snappier_hip_buffers_decompress"' in cs
    imps = {}
    for m in re.finditer(r"\[DllImport\(Lib, CallingConvention = Cc\)\]\s*internal static extern ([A-Za-z\*]+) (snp_[a-z0-9_]+)\(([^)]*)\);", cs):
        params = [re.match(r"(.*?)\s+([A-Za-z_][A-Za-z0-9_]*)$", q.strip()).group(1) for q in m.group(3).split(",") if q.strip()]
        imps[m.group(2)] = (T.cs_class(m.group(1)), [T.cs_class(q) for q in params])
    assert list(protos) == list(imps) == ["snp_decompress_buffers_workspace", "snp_decompress_buffers_batch"]   # (header order)
    for name, (ret, params) in protos.items():
        cret, cparams = imps[name]
        assert T.compatible(ret, cret), (name, ret, cret)
        assert len(params) == len(cparams) and all(T.compatible(a, b) for a, b in zip(params, cparams)), (name, params, cparams)


def _random_batch(seed):
    """Blocks with real Snappy streams of html-like content, a few malformed or foreign preambles, and empty ones."""
    rng = np.random.default_rng(seed)
    html = open(os.path.join(ROOT, "tests", "golden", "testdata", "html"), "rb").read()
    blocks, caps = [], []
    for b in range(int(rng.integers(8, 40))):
        kind = rng.integers(0, 6)
        n = int(np.exp(rng.uniform(0, np.log(3 << 20))))
        raw = (html * (n // len(html) + 1))[:n]
        if kind == 0:
            blk = b""
        elif kind == 1:
            blk = b"\xff\xff\xff\xff\xff\x01" + raw[:100]                # a varint that overflows
        elif kind == 2:
            blk = varint(n)                                              # nothing after the preamble
        else:
            blk = O.compress(raw, O.HASH_CRC32C)
        blocks.append(blk)
        caps.append(n + int(rng.integers(-1, 3)) if kind != 4 else n // 2)
    return blocks, [max(c, 0) for c in caps]


@pytest.mark.parametrize("seed", [1, 2, 3, 4])
@pytest.mark.parametrize("par_min", [0, 1, 262144])
def test_plan_model_against_a_serial_walk(seed, par_min):
    blocks, caps = _random_batch(seed)
    nb = len(blocks)
    for wave_slots in (8192, 64):
        for max_fragments in (0, 7, 1 << 20):
            P = plan(blocks, caps, par_min, wave_slots, max_fragments)
            # serial walk: candidates, the makespan rule, admission in buffer order while the fragments fit
            cands = []
            for b, blk in enumerate(blocks):
                clean, d, hb = preamble(blk)
                if clean and par_min and par_min <= d <= caps[b] and hb < len(blk) <= max_compressed(d):
                    cands.append((b, d, hb))
            total = sum(d for _, d, _ in cands)
            used, adm, need = 0, [], 0
            for b, d, hb in cands:
                if d * wave_slots < SPLIT_FACTOR * total:
                    continue
                need += (d + B - 1) // B
                if need <= max_fragments:                                # (once one does not fit, no later one does)
                    adm.append(b)
                    used = need
            assert P["needed"] == need
            assert [b for b in range(nb) if P["admitted"][b]] == adm
            # the chunk bound that sizes the workspace: chunks + 2 per split block within 7 slots per fragment
            assert int(P["slot"][nb]) <= SLOTS_PER_FRAGMENT * max(used, 0)
            for b in adm:
                f = int(P["first"][b + 1] - P["first"][b])
                assert int(P["chunks"][b]) <= 5 * f
            # ticket -> (block, chunk): block-major order, every chunk of every split block exactly once
            walk = [(b, k) for b in adm for k in range(int(P["chunks"][b]))]
            got = []
            for t in range(int(P["chunk_first"][nb])):
                b = find_block(P["chunk_first"], nb, t)
                got.append((b, t - int(P["chunk_first"][b])))
            assert got == walk
            # scan tickets -> the i-th split block
            assert [find_block(P["rank"], nb, i) for i in range(len(adm))] == adm


def test_makespan_rule_keeps_small_batches_whole():
    """Batches of <= 64 MiB in all split every candidate (c * 64 MiB / 8192 wave slots = 16 KiB < the smallest par_min of 256 KiB),
    and 10 GiB of 1 MiB blocks split none."""
    assert SPLIT_FACTOR * (64 << 20) // 8192 <= 262144
    assert (1 << 20) * 8192 < SPLIT_FACTOR * (10 << 30)
    assert (64 << 20) * 8192 >= SPLIT_FACTOR * (10 << 30)

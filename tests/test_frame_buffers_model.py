"""snp_frame_encode_buffers_batch / snp_frame_decode_buffers_batch (libsnappier_hip_frame_buffers.so) without a GPU: the workspace arithmetic, the
declarations and their C# binding, null-pointer rejection, and the NumPy / Python model of both plans (frame_buffers_model.py): encode emit positions
that concatenate the oracle's chunks into its framed stream, and the per-stream span walk with small spans against a serial walk."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import frame_buffers_model as M
import oracle as O
from conftest import ROOT, read_testdata

B = 65536
STAGE_STRIDE = 76512          # kSnpCompStride (capi_internal.h): staging bytes per chunk slot
NAMES = ["snp_frame_decode_buffers_batch", "snp_frame_decode_buffers_workspace", "snp_frame_encode_buffers_batch", "snp_frame_encode_buffers_workspace"]


def _lib():
    from snappier_amd import _native as N
    return N.frame_buffers_lib()


def test_workspace_arithmetic():
    L = _lib()
    ew, dw = L.snp_frame_encode_buffers_workspace, L.snp_frame_decode_buffers_workspace
    assert ew(0, 0) == 0 and ew(0, 1000) == 0 and dw(0, 0, 0) == 0 and dw(0, 1000, 1000) == 0
    for nb in (1, 2, 255, 1023, 1024, 1025, 300000):
        for nc in (0, 1, 1023, 1024, 1025, 163840):
            w = ew(nb, nc)
            assert w % 256 == 0 and w >= nc * STAGE_STRIDE + (nb + 1) * 8
            assert ew(nb, nc + 1) >= w and ew(nb + 1, nc) >= w
            for ns in (0, 1, 5000):
                d = dw(nb, nc, ns)
                assert d % 256 == 0 and d >= nc * 41 + ns * 136 + (nb + 1) * 16
                assert dw(nb, nc + 1, ns) >= d and dw(nb, nc, ns + 1) >= d and dw(nb + 1, nc, ns) >= d
    assert ew(0xFFFFFFFF, 0xFFFFFFFF) > 0xFFFFFFFF * STAGE_STRIDE      # (64-bit arithmetic)
    assert dw(0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF) > 0xFFFFFFFF * 177


def test_header_and_binding_declare_the_new_functions():
    from snappier_amd import _native as N
    declared = N.frame_buffers_declared_symbols()
    assert declared == NAMES
    others = set(N.declared_symbols()) | set(N.buffers_declared_symbols()) | set(N.buffers_decompress_declared_symbols())
    assert not set(declared) & others                                  # the other headers' surfaces are left as they are
    L = _lib()
    assert L.snp_frame_encode_buffers_batch.restype is C.c_int and len(L.snp_frame_encode_buffers_batch.argtypes) == 13
    assert L.snp_frame_decode_buffers_batch.restype is C.c_int and len(L.snp_frame_decode_buffers_batch.argtypes) == 14
    assert L.snp_frame_encode_buffers_workspace.restype is C.c_uint64 and L.snp_frame_decode_buffers_workspace.restype is C.c_uint64


def test_extension_library_exports_exactly_its_header():
    from layouts import exported
    from snappier_amd import _native as N

    ext = exported(N.FRAME_BUFFERS_PATH)
    assert ext == set(NAMES)
    assert not exported(N.PRODUCT_PATH) & ext


def test_csharp_binding_matches_the_extension_header():
    import test_csharp_signatures as T
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "snappier_hip_frame_buffers.h")).read(), flags=re.S)
    protos = {}
    for m in re.finditer(r"([A-Za-z_][A-Za-z0-9_ ]*?[\s\*]+)(snp_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", text):
        params = [re.match(r"(.*?[\s\*])([A-Za-z_][A-Za-z0-9_]*)$", q.strip()).group(1) for q in m.group(3).split(",") if q.strip() not in ("", "void")]
        protos[m.group(2)] = (T.c_class(m.group(1)), [T.c_class(q) for q in params])
    cs = re.sub(r"//.*", "", open(os.path.join(ROOT, "csharp", "Snappier.Gpu", "NativeMethodsFrameBuffers.cs")).read())
    assert 'const string Lib = "snappier_hip_frame_buffers"' in cs
    imps = {}
    for m in re.finditer(r"\[DllImport\(Lib, CallingConvention = Cc\)\]\s*internal static extern ([A-Za-z\*]+) (snp_[a-z0-9_]+)\(([^)]*)\);", cs):
        params = [re.match(r"(.*?)\s+([A-Za-z_][A-Za-z0-9_]*)$", q.strip()).group(1) for q in m.group(3).split(",") if q.strip()]
        imps[m.group(2)] = (T.cs_class(m.group(1)), [T.cs_class(q) for q in params])
    assert set(protos) == set(imps) == set(NAMES)
    for name, (ret, params) in protos.items():
        cret, cparams = imps[name]
        assert T.compatible(ret, cret), (name, ret, cret)
        assert len(params) == len(cparams) and all(T.compatible(a, b) for a, b in zip(params, cparams)), (name, params, cparams)
    proj = open(os.path.join(ROOT, "csharp", "Snappier.Gpu", "Snappier.Gpu.csproj")).read()
    assert 'Include="../../snappier_amd/libsnappier_hip_frame_buffers.so"' in proj


def test_batch_calls_reject_null_pointers_without_a_device():
    L = _lib()
    assert L.snp_frame_encode_buffers_batch(None, None, None, None, 0, 0, None, None, None, None, None, None, None) == O.ERR_BAD_ARG
    assert L.snp_frame_decode_buffers_batch(None, None, None, None, 0, 0, 0, None, None, None, None, None, None, None) == O.ERR_BAD_ARG


# ---- encode plan -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", [O.HASH_CRC32C, O.HASH_MUL])
@pytest.mark.parametrize("seed", [1, 2])
def test_encode_emit_positions_concatenate_to_the_oracle(variant, seed):
    rng = np.random.default_rng(seed)
    pool = read_testdata("html") * 6 + rng.integers(0, 256, 200000, dtype=np.uint8).tobytes()
    lens = [0, 1, 65535, 65536, 65537, 3] + [int(x) for x in rng.integers(0, 250000, 6)]
    rng.shuffle(lens)
    offs = [int(rng.integers(0, len(pool) - n + 1)) for n in lens]
    bufs = [pool[o:o + n] for o, n in zip(offs, lens)]
    chunks = [M.oracle_chunks(x, variant) for x in bufs]
    size = lambda b, k: len(chunks[b][k])                               # noqa: E731
    cap = [10 + 8 * ((n + B - 1) // B) + n for n in lens]
    exact = sum((n + B - 1) // B for n in lens)

    def emit(max_chunks, caps):
        status, out_len, pos, result = M.encode_plan(lens, max_chunks, size, caps)
        outs = []
        for b in range(len(lens)):
            o = bytearray(b"\xa5" * caps[b])
            if status[b] == O.OK:
                o[:10] = M.STREAM_ID
                for k, c in enumerate(chunks[b]):
                    o[pos[(b, k)]:pos[(b, k)] + len(c)] = c
            outs.append(bytes(o))
        return status, out_len, outs, result

    status, out_len, outs, result = emit(exact, cap)
    assert (status == O.OK).all() and result == [exact, int(out_len.sum())]
    for b, x in enumerate(bufs):
        assert outs[b][:out_len[b]] == O.frame_encode(x, variant)
    assert any(c[0] == 1 for cs in chunks for c in cs)                 # random content: raw chunks
    assert emit(exact + 7, cap)[2] == outs                              # a loose bound: the same bytes
    short = exact - 2
    st2, len2, outs2, res2 = emit(short, cap)
    first = np.concatenate([[0], np.cumsum([(n + B - 1) // B for n in lens])])
    assert res2[0] == exact
    for b in range(len(lens)):
        if first[b + 1] <= short:
            assert st2[b] == O.OK and outs2[b] == outs[b]
        else:
            assert st2[b] == O.ERR_OUTPUT_TOO_SMALL and len2[b] == 0 and set(outs2[b]) <= {0xA5}
    cap3 = list(cap)
    cap3[2] = int(out_len[2]) - 1
    st3, len3, _, _ = emit(exact, cap3)
    assert st3[2] == O.ERR_OUTPUT_TOO_SMALL and len3[2] == 0 and (np.delete(st3, 2) == O.OK).all()


# ---- decode: the span walk with small spans --------------------------------------------------------------------------------------------------
def hand_streams():
    html = read_testdata("html") * 4
    ID = M.STREAM_ID
    rng = np.random.default_rng(4)
    s = {}
    s["plain"] = O.frame_encode(html[:200000])
    s["raw"] = ID + b"".join(M.data_chunk(html[i:i + 700], compressed=False) for i in range(0, 7000, 700))
    s["skip_big"] = ID + M.data_chunk(html[:300]) + M.chunk(0x85, bytes(rng.integers(0, 256, 1500, dtype=np.uint8))) + \
        M.chunk(0xFE, b"\0" * 900) + M.data_chunk(html[300:900])
    s["ids"] = ID + M.data_chunk(html[:100]) + ID + ID + M.data_chunk(html[100:500]) + ID
    s["concat"] = O.frame_encode(html[:1000]) + O.frame_encode(html[5:5000])
    s["mid_header"] = ID + M.data_chunk(html[:600]) + b"\x00\x10"
    s["mid_body"] = (ID + M.data_chunk(html[:600]))[:-9]
    s["type"] = ID + M.data_chunk(html[:80]) + M.chunk(0x33, b"zz") + M.data_chunk(html[:80])
    s["crc"] = ID + M.data_chunk(html[:500])[:5] + b"\x00" + M.data_chunk(html[:500])[6:] + M.data_chunk(html[:50])
    s["varint"] = ID + M.chunk(0x00, b"\1\2\3\4" + b"\xff" * 6)
    s["empty"] = b""
    s["id_only"] = ID
    # an entry that is no candidate: the chain enters span 1 at a data chunk larger than 65536 raw bytes
    s["huge_raw"] = ID + M.chunk(0xFE, b"\0" * 400) + M.data_chunk(bytes(70000), compressed=False) + M.data_chunk(html[:300])
    return s


def test_host_walk_equals_the_serial_walk():
    """snp_frame_decoded_length (the host walk of capi_frame.hip) gives the status and the total of the model's serial walk on every hand stream
    and on each of them cut short by 1 to 12 bytes: a cut inside the last header, CRC, preamble or body."""
    import ctypes as C
    from snappier_amd import _native as N
    fn = N.lib().snp_frame_decoded_length
    for name, x in hand_streams().items():
        for cut in range(0, min(12, len(x)) + 1):
            s = x[:len(x) - cut]
            _rows, total, tail = M.serial_walk(s, cap=2 ** 63)
            v = C.c_uint64(0)
            assert (fn(s, len(s), C.byref(v)), v.value) == (tail, total), (name, cut)


@pytest.mark.parametrize("span,window", [(256, 256), (256, 40), (333, 333), (1024, 200)])
def test_span_walk_equals_the_serial_walk(span, window):
    for name, x in hand_streams().items():
        for cap in (1 << 40, max(M.serial_walk(x, 1 << 40)[1] - 1, 0)):
            rows, total, tail = M.serial_walk(x, cap)
            r2, t2, tail2, missed = M.span_walk(x, cap, span, window)
            assert (r2, t2, tail2) == (rows, total, tail), (name, cap)
            assert M.verdict(x, r2, t2, tail2) == M.verdict(x, rows, total, tail)


def test_span_walk_meets_entries_that_are_no_candidate():
    s = hand_streams()
    assert M.span_walk(s["skip_big"], 1 << 40, 256, 256)[3] > 0
    assert M.span_walk(s["huge_raw"], 1 << 40, 256, 256)[3] > 0
    assert M.span_walk(s["plain"], 1 << 40, 256, 40)[3] > 0             # a window shorter than a chunk: every entry is walked on the spot


def test_verdicts_of_the_hand_streams():
    s = hand_streams()
    v = {name: M.verdict(x, *M.serial_walk(x, 1 << 40)) for name, x in s.items()}
    assert v["plain"] == (O.OK, 200000) and v["empty"] == (O.OK, 0) and v["id_only"] == (O.OK, 0)
    assert v["mid_header"][0] == v["mid_body"][0] == O.ERR_TRUNCATED_STREAM
    assert v["type"][0] == O.ERR_CHUNK_TYPE and v["crc"][0] == O.ERR_CRC_MISMATCH and v["varint"][0] == O.ERR_BAD_LENGTH
    assert v["ids"] == (O.OK, 500) and v["concat"] == (O.OK, 5995) and v["skip_big"] == (O.OK, 900)


@pytest.mark.parametrize("span,window", [(256, 256), (512, 100)])
def test_batch_plan_rows_and_both_admission_bounds(span, window):
    streams = list(hand_streams().values())
    caps = [M.serial_walk(x, 1 << 40)[1] for x in streams]
    caps[3] -= 1                                                        # one stream over its capacity: it lists nothing
    nspans = [(len(x) + span - 1) // span for x in streams]
    serial = [M.serial_walk(x, c) for x, c in zip(streams, caps)]
    nchunks = [len(w[0]) for w in serial]
    sfirst, cfirst = np.cumsum(nspans), np.cumsum(nchunks)
    for max_spans, max_chunks in ((sfirst[-1], cfirst[-1]), (sfirst[-1] + 3, cfirst[-1] + 5), (sfirst[6] - 1, cfirst[-1]),
                                  (sfirst[-1], cfirst[4] - 1), (0, 0), (sfirst[-1], 0)):
        status, out_len, slots, result, _ = M.decode_plan(streams, caps, int(max_chunks), int(max_spans), span, window)
        walked = sfirst <= max_spans
        assert result[2] == sfirst[-1] and result[0] == (int(cfirst[walked].max()) if walked.any() else 0)
        for b, x in enumerate(streams):
            if walked[b] and cfirst[b] <= max_chunks:
                assert (status[b], out_len[b]) == M.verdict(x, *serial[b])
                base = int(cfirst[b]) - nchunks[b]
                assert [slots[base + i][1] for i in range(nchunks[b])] == serial[b][0]
            else:
                assert (status[b], out_len[b]) == (O.ERR_OUTPUT_TOO_SMALL, 0)
        assert result[1] == int(out_len[status == O.OK].sum())
        assert all(c < max_chunks for c in slots)


def _random_windows(seed: int):
    """Random bytes with data, raw, identifier and skippable chunks (some cut short, some with a body lying about its length) at random places."""
    rng = np.random.default_rng(seed)
    html = read_testdata("html")
    out = []
    for _ in range(6):
        s = bytearray(rng.integers(0, 256, int(rng.integers(2000, 9000)), dtype=np.uint8).tobytes())
        for _ in range(int(rng.integers(3, 12))):
            c = b""
            for _ in range(int(rng.integers(1, 4))):                 # a run of chunks: its first header is a plausible start
                o = int(rng.integers(0, len(html) - 2000))
                piece = html[o:o + int(rng.integers(1, 1500))]
                c += [M.data_chunk(piece), M.data_chunk(piece, compressed=False), M.STREAM_ID, M.chunk(0xFE, b"\0" * len(piece))][int(rng.integers(0, 4))]
            if rng.integers(0, 4) == 0:
                c = c[:int(rng.integers(1, len(c) + 1))]
            at = int(rng.integers(0, len(s)))
            s[at:at] = c
        for _ in range(int(rng.integers(0, 30))):                   # loose type bytes in front of lengths that may or may not fit
            at = int(rng.integers(0, len(s) - 4))
            s[at] = int(rng.choice([0x00, 0x01, 0xFF]))
        out.append(bytes(s))
    return out


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_candidate_prefilter_equals_the_scalar_search(seed):
    """candidates() runs plausible_start only where shape_prefilter lets a position through: the same kept candidates and chains as the scalar
    search, on the model's hand streams and on seeded random windows; and the prefilter never drops a position chunk_shape accepts."""
    streams = list(hand_streams().values()) + _random_windows(seed)
    for span, window in ((256, 256), (333, 333), (1024, 200), (4096, 4096)):
        for x in streams:
            for k in range((len(x) + span - 1) // span):
                assert M.candidates(x, k, span, window) == M.candidates_scalar(x, k, span, window), (span, window, k)
    for x in streams:
        kept = set(M.shape_prefilter(x, 0, len(x)).tolist())
        assert {p for p in range(len(x)) if M.chunk_shape(x, p)[0]} <= kept
        assert kept <= set(range(max(len(x) - 7, 0)))

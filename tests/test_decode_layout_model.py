"""snp_decompress_layout_batch / snp_frame_decode_layout_batch (libsnappier_hip_layout.so) without a GPU: the declarations and their C# binding,
the workspace arithmetic, argument rejection, and the Python model of both contracts (decode_layout_model.py): its per-item part against the host
functions snp_get_uncompressed_length / snp_frame_decoded_length and the oracle, the claim the header makes about the expansion rule, and the
placement rule against a brute-force loop."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import decode_layout_model as L
import frame_buffers_model as M
import oracle as O
from conftest import ROOT

NAMES = ["snp_decompress_layout_batch", "snp_decompress_layout_workspace", "snp_frame_decode_layout_batch", "snp_frame_decode_layout_workspace"]


def _lib():
    from snappier_amd import _native as N
    return N.layout_lib()


# ---- the surface -----------------------------------------------------------------------------------------------------------------------------
def test_header_and_binding_declare_the_new_functions():
    from snappier_amd import _native as N
    declared = N.layout_declared_symbols()
    assert declared == NAMES
    others = set(N.declared_symbols()) | set(N.buffers_declared_symbols()) | set(N.buffers_decompress_declared_symbols()) | \
        set(N.frame_buffers_declared_symbols())
    assert not set(declared) & others                                  # the other headers' surfaces are left as they are
    lib = _lib()
    assert lib.snp_decompress_layout_batch.restype is C.c_int and len(lib.snp_decompress_layout_batch.argtypes) == 13
    assert lib.snp_frame_decode_layout_batch.restype is C.c_int and len(lib.snp_frame_decode_layout_batch.argtypes) == 15
    assert lib.snp_decompress_layout_workspace.restype is C.c_uint64 and lib.snp_frame_decode_layout_workspace.restype is C.c_uint64


def test_extension_library_exports_exactly_its_header():
    from layouts import exported
    from snappier_amd import _native as N

    ext = exported(N.LAYOUT_PATH)
    assert ext == set(NAMES)
    for other in (N.PRODUCT_PATH, N.BUFFERS_PATH, N.BUFFERS_DECOMPRESS_PATH, N.FRAME_BUFFERS_PATH, N.FRAME_RANGE_PATH):
        assert not exported(other) & ext


def test_workspace_functions_are_host_arithmetic():
    lib = _lib()
    bw, fw = lib.snp_decompress_layout_workspace, lib.snp_frame_decode_layout_workspace
    assert bw(0) == 0 and fw(0, 0) == 0 and fw(0, 1000) == 0
    for nb in (1, 2, 255, 1023, 1024, 1025, 300000):
        w = bw(nb)
        assert w % 256 == 0 and w >= (nb + 1) * 8 + ((nb + 1023) // 1024 + 1) * 8 and bw(nb + 1) >= w
        for ns in (0, 1, 5000):
            d = fw(nb, ns)
            assert d % 256 == 0 and d >= ns * 136 + (nb + 1) * 16 + nb * 20
            assert fw(nb, ns + 1) >= d and fw(nb + 1, ns) >= d
    assert bw(0xFFFFFFFF) > 0xFFFFFFFF * 8 and fw(0xFFFFFFFF, 0xFFFFFFFF) > 0xFFFFFFFF * 170      # (64-bit arithmetic)
    # the frame layout needs no chunk table: less than the decode call's workspace with the same spans and no chunk slot
    from snappier_amd import _native as N
    assert fw(1000, 5000) <= N.frame_buffers_lib().snp_frame_decode_buffers_workspace(1000, 0, 5000)


def test_workspace_sizes_of_the_four_extensions_are_pinned():
    """Every *_workspace function of the batch extensions returns these values: the order and the sizes of the pieces their layout functions
    carve (work_carver.h, 256-byte pieces) are part of what a caller that sizes d_work once relies on."""
    from snappier_amd import _native as N
    B, D, F, Y = N.buffers_lib(), N.buffers_decompress_lib(), N.frame_buffers_lib(), N.layout_lib()
    two = {(0, 0): (0, 0, 0, 0),
           (1, 1): (79104, 115456, 79360, 4096),
           (1000, 5000): (382770176, 42555136, 382790400, 718336),
           (300000, 300000): (22968006144, 970468864, 22969206272, 51603712),
           (7, 4294967295): (328788369922304, 203769777920, 328805549791488, 584115554048)}
    for args, want in two.items():
        got = (B.snp_compress_buffers_workspace(*args), D.snp_decompress_buffers_workspace(*args), F.snp_frame_encode_buffers_workspace(*args),
               Y.snp_frame_decode_layout_workspace(*args))
        assert got == want, (args, got)
    for args, want in {(0, 0, 0): 0, (1, 1, 1): 6400, (1000, 70000, 5000): 3589120, (163840, 163840, 163840): 34899968}.items():
        assert F.snp_frame_decode_buffers_workspace(*args) == want, args
    for nb, want in {0: 0, 1: 512, 1000: 8448, 300000: 2402816}.items():
        assert Y.snp_decompress_layout_workspace(nb) == want, nb


def test_workspace_sizes_of_the_framed_decode_calls_are_pinned():
    """The same for the range decode's workspace, and for snp_frame_decode_workspace of the product library: a 64-byte header, the packed chunk
    table of 37 bytes a row (two u64, five 32-bit words, one byte) rounded up to 16, and 16 bytes."""
    from snappier_amd import _native as N
    R, P = N.frame_range_lib(), N.lib()
    for args, want in {(0, 0, 0, 0): 0, (1, 1, 1, 1): 12288, (1000, 70000, 5000, 1 << 20): 4893184, (163840, 163840, 163840, 0): 68325120}.items():
        assert R.snp_frame_decode_range_workspace(*args) == want, args
    for n, want in {0: 80, 1: 128, 8: 384, 163848: 6062464}.items():
        assert P.snp_frame_decode_workspace(n) == want == 64 + (37 * n + 15) // 16 * 16 + 16, n


def test_csharp_binding_matches_the_extension_header():
    import test_csharp_signatures as T
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "snappier_hip_layout.h")).read(), flags=re.S)
    protos = {}
    for m in re.finditer(r"([A-Za-z_][A-Za-z0-9_ ]*?[\s\*]+)(snp_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", text):
        params = [re.match(r"(.*?[\s\*])([A-Za-z_][A-Za-z0-9_]*)$", q.strip()).group(1) for q in m.group(3).split(",") if q.strip() not in ("", "void")]
        protos[m.group(2)] = (T.c_class(m.group(1)), [T.c_class(q) for q in params])
    cs = re.sub(r"//.*", "", open(os.path.join(ROOT, "csharp", "Snappier.Gpu", "NativeMethodsLayout.cs")).read())
    assert 'const string Lib = "snappier_hip_layout"' in cs
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
    assert 'Include="../../snappier_amd/libsnappier_hip_layout.so"' in proj


def test_batch_calls_reject_bad_arguments_without_a_device():
    lib = _lib()
    assert lib.snp_decompress_layout_batch(None, None, None, None, 0, 1, 0, None, None, None, None, None, None) == O.ERR_BAD_ARG
    assert lib.snp_frame_decode_layout_batch(None, None, None, None, 0, 0, 1, 0, None, None, None, None, None, None, None) == O.ERR_BAD_ARG
    # a bad align is refused before the context is touched (the pointers below are never dereferenced)
    fake = C.c_void_p(64)
    for align in (0, 3, 6, 1000, (1 << 20) + 1, 1 << 21, 0xFFFFFFFF):
        assert lib.snp_decompress_layout_batch(fake, None, None, None, 0, align, 0, None, None, None, None, None, fake) == O.ERR_BAD_ARG
        assert lib.snp_frame_decode_layout_batch(fake, None, None, None, 0, 0, align, 0, None, None, None, None, None, None, fake) == O.ERR_BAD_ARG


# ---- one item: the model against the host functions and the oracle ---------------------------------------------------------------------------
def host_block(buf: bytes):
    """snp_get_uncompressed_length of libsnappier_hip.so: -> (status, value, header bytes)."""
    from snappier_amd import _native as N
    v, hb = C.c_uint32(0), C.c_uint32(0)
    st = N.lib().snp_get_uncompressed_length(buf, len(buf), C.byref(v), C.byref(hb))
    return (st, v.value, hb.value) if st == O.OK else (st, 0, 0)


def host_stream(s: bytes):
    """snp_frame_decoded_length of libsnappier_hip.so: -> (status, decoded_len)."""
    from snappier_amd import _native as N
    v = C.c_uint64(0)
    st = N.lib().snp_frame_decoded_length(s, len(s), C.byref(v))
    return st, v.value


def test_block_items_equal_the_host_function_and_cover_every_status():
    seen = set()
    for name, buf in {**L.corpus_blocks(), **L.block_cases()}.items():
        st, v, hb = host_block(buf)
        assert L.read_preamble(buf) == (st, v, hb), name
        got = L.block_item(buf)
        want = (st, 0) if st != O.OK else (O.ERR_INCOMPLETE, 0) if v > (((len(buf) - hb) // 3) + 1) * 64 else (O.OK, v)
        assert got == want, name
        seen.add(got[0])
    assert seen == {O.OK, O.ERR_BAD_LENGTH, O.ERR_INCOMPLETE}
    cases = L.block_cases()
    for k in (0, 1, 2, 3, 10, 299):                                     # the bound itself passes, one more does not
        assert L.block_item(cases[f"at_bound_{k}"]) == (O.OK, L.expansion_bound(k))
        assert L.block_item(cases[f"over_bound_{k}"]) == (O.ERR_INCOMPLETE, 0)
    for name in ("empty", "unterminated_1", "unterminated_2", "unterminated_4", "bits_above_2_32", "six_bytes_zero_tail", "six_bytes"):
        assert L.block_item(cases[name]) == (O.ERR_BAD_LENGTH, 0), name
    assert L.block_item(cases["u32_max_short_body"]) == (O.ERR_INCOMPLETE, 0) and host_block(cases["u32_max_short_body"])[1] == 0xFFFFFFFF
    assert L.block_item(b"\xff\xff\xff\xff\x0f", in_len=1 << 28) == (O.OK, 0xFFFFFFFF)   # (a table length: the body is never read)


def test_well_formed_blocks_equal_the_oracle():
    for name, buf in L.corpus_blocks().items():
        st, v, br = O.varint_read(buf)
        assert st == O.OK and L.block_item(buf) == (O.OK, v) and L.read_preamble(buf)[2] == br, name
        assert v == O.get_uncompressed_length(buf)
    for m in (1, 7, 100):
        buf = L.block_cases()[f"max_expansion_{m}"]
        assert L.block_item(buf) == (O.OK, 1 + 64 * m) and O.decompress(buf) == b"a" * (1 + 64 * m)


def test_every_block_the_expansion_rule_rejects_fails_in_the_decoder():
    """The header's claim: declared > ((in_len - header_bytes) / 3 + 1) * 64 cannot decode, whatever the tags are and with room for all of it."""
    rng = np.random.default_rng(11)
    blocks = [b for b in L.block_cases().values()]
    html = O.compress(L.read_testdata("html")[:3000])
    hb = L.read_preamble(html)[2]
    for m in range(0, 40):                                              # bodies that expand the most, cut to every length mod 3
        body = L.max_expansion_body(m)
        for cut in (0, 1, 2):
            body2 = body[:len(body) - cut]
            blocks += [L.varint(L.expansion_bound(len(body2)) + extra) + body2 for extra in (1, 2, 64)]
    for _ in range(300):                                                # random tags, and a real body under a larger preamble
        body = rng.integers(0, 256, int(rng.integers(0, 200)), dtype=np.uint8).tobytes()
        blocks.append(L.varint(L.expansion_bound(len(body)) + int(rng.integers(1, 1000))) + body)
    blocks.append(L.varint(L.expansion_bound(len(html) - hb) + 1) + html[hb:])
    rejected = 0
    for buf in blocks:
        st, declared, _ = L.read_preamble(buf)
        if st == O.OK and L.block_item(buf)[0] == O.ERR_INCOMPLETE:
            rejected += 1
            assert O.decompress_status(buf, cap=declared) != O.OK, buf[:16]
    assert rejected > 400


def test_stream_items_equal_the_host_function_and_cover_every_status():
    seen = set()
    cases = L.stream_cases()
    for name, s in {**L.corpus_streams(), **cases}.items():
        st, total, nc = L.stream_item(s)
        assert (st, total) == host_stream(s), name
        assert nc == len(M.serial_walk(s, 1 << 64)[0])
        seen.add(st)
    assert seen == {O.OK, O.ERR_BAD_LENGTH, O.ERR_INCOMPLETE, O.ERR_TRUNCATED_STREAM, O.ERR_CHUNK_TYPE}
    want = {"empty": (O.OK, 0, 0), "id_only": (O.OK, 0, 0), "plain": (O.OK, 200000, 4), "concat": (O.OK, 5995, 2),
            "cut_in_header_1": (O.ERR_TRUNCATED_STREAM, 5000, 2), "cut_in_header_3": (O.ERR_TRUNCATED_STREAM, 5000, 2),
            "cut_in_body": (O.ERR_TRUNCATED_STREAM, 5000, 2), "cut_in_first_body": (O.ERR_TRUNCATED_STREAM, 0, 0),
            "cut_in_id": (O.ERR_TRUNCATED_STREAM, 0, 0), "size_3_compressed": (O.ERR_TRUNCATED_STREAM, 5000, 2),
            "size_0_raw": (O.ERR_TRUNCATED_STREAM, 5000, 2), "type_02": (O.ERR_CHUNK_TYPE, 5000, 2), "type_7f": (O.ERR_CHUNK_TYPE, 5000, 2),
            "type_02_first": (O.ERR_CHUNK_TYPE, 0, 0), "skippable": (O.OK, 1000, 3), "bad_varint_after_good": (O.ERR_BAD_LENGTH, 5000, 2),
            "unterminated_varint": (O.ERR_BAD_LENGTH, 5000, 2), "varint_2_31": (O.ERR_BAD_LENGTH, 5000, 2),
            "over_bound": (O.ERR_INCOMPLETE, 5000, 2), "at_bound": (O.OK, 5000 + L.expansion_bound(10) + 80, 4), "bad_crc": (O.OK, 550, 2)}
    for name, w in want.items():
        assert L.stream_item(cases[name]) == w, name


def test_well_formed_streams_equal_the_oracle():
    for name, s in L.corpus_streams().items():
        st, total, nc = L.stream_item(s)
        raw = O.frame_decode(s)
        assert st == O.OK and total == O.frame_decoded_length(s) == len(raw) and nc == (len(raw) + L.B - 1) // L.B, name


# ---- placement -------------------------------------------------------------------------------------------------------------------------------
def brute_force(lengths, takes_part, align, arena_cap):
    """The placement as a caller would do it by hand: -> (ranges of the placed items {index: (start, end)}, first not placed or None, need)."""
    cursor, ranges, stopped, need = 0, {}, None, 0
    for b, (n, t) in enumerate(zip(lengths, takes_part)):
        if not t:
            continue
        cursor += -cursor % align                                          # the next multiple of align
        need = cursor + n
        if stopped is None and need > arena_cap:
            stopped = b
        if stopped is None:
            ranges[b] = (cursor, cursor + n)
        cursor += n
    return ranges, stopped, need


def check_placement(out, lengths, takes_part, align, arena_cap):
    ranges, stopped, need = brute_force(lengths, takes_part, align, arena_cap)
    n = len(lengths)
    prev_end = 0
    for b in range(n):
        assert out["out_off"][b] % align == 0
        if b in ranges:
            assert (out["out_off"][b], out["out_off"][b] + out["out_cap"][b]) == ranges[b]
            assert out["out_off"][b] >= prev_end and ranges[b][1] <= arena_cap      # disjoint, in order, inside the arena
            prev_end = ranges[b][1]
        else:
            assert out["out_cap"][b] == 0
            if takes_part[b]:
                assert out["status"][b] == O.ERR_OUTPUT_TOO_SMALL and b >= stopped
    assert out["result"][0] == need
    return ranges, stopped


ALIGNS = (1, 2, 64, 4096, 1 << 20)


@pytest.mark.parametrize("align", ALIGNS)
def test_block_placement_against_a_brute_force_loop(align):
    rng = np.random.default_rng(align)
    bad = [(O.ERR_BAD_LENGTH, 0), (O.ERR_INCOMPLETE, 0)]
    good = [(O.OK, int(x)) for x in [0, 1, 63, 64, 65, 4095, 4096, 4097, 65536, 65537, (1 << 20) - 1, 1 << 20, 3 << 20, 0xFFFFFFFF, 0]]
    # not-OK buffers in front of, between and after the placed ones
    items = [bad[0], bad[1]] + good[:5] + [bad[1]] + good[5:9] + [bad[0], bad[0]] + good[9:] + [bad[1]]
    for trial in range(4):
        if trial:
            items = [items[i] for i in rng.permutation(len(items))]
        ok = [st == O.OK for st, _ in items]
        lengths = [d for _, d in items]
        full = L.block_layout(items, align)
        need = full["result"][0]
        assert check_placement(full, lengths, ok, align, L.UNBOUNDED)[1] is None
        assert full["result"] == [need, len(items), sum((d + L.B - 1) // L.B for d in lengths), sum(lengths)]
        assert full["status"] == [st for st, _ in items] and full["declared"] == lengths
        assert L.block_layout(items, align, need) == full                  # exactly enough
        for cap in (need - 1, 0, need // 2, need // 3 + 1):
            out = L.block_layout(items, align, cap)
            ranges, stopped = check_placement(out, lengths, ok, align, cap)
            assert stopped is not None and out["result"][1] == stopped and out["result"][0] == need
            assert out["out_off"] == full["out_off"] and out["declared"] == lengths
            for b, (st, _) in enumerate(items):
                assert out["status"][b] == (st if st != O.OK or b < stopped else O.ERR_OUTPUT_TOO_SMALL)
            assert out["result"][2] == sum((e - s + L.B - 1) // L.B for s, e in ranges.values())
            assert out["result"][3] == sum(e - s for s, e in ranges.values())
    assert L.block_layout([], align)["result"] == [0, 0, 0, 0]
    assert L.block_layout([bad[0], bad[1]], align, 0)["result"] == [0, 2, 0, 0]
    assert L.block_layout([(O.OK, 0), bad[0], (O.OK, 0)], align, 0)["result"] == [0, 3, 0, 0]   # empty outputs fit an empty arena


@pytest.mark.parametrize("align", ALIGNS)
def test_stream_placement_and_span_admission(align):
    rng = np.random.default_rng(100 + align)
    statuses = [O.OK, O.ERR_TRUNCATED_STREAM, O.ERR_BAD_LENGTH, O.ERR_INCOMPLETE, O.ERR_CHUNK_TYPE]
    items, in_len = [], []
    for i in range(24):
        total = int(rng.choice([0, 1, 4097, 65536, 200000, 5 << 20]))
        items.append((statuses[i % 5], total, (total + L.B - 1) // L.B))
        in_len.append(int(rng.choice([0, 10, 70000, (1 << 20), (1 << 20) + 1, 3 << 20])))
    spans = [(x + L.SPAN - 1) // L.SPAN for x in in_len]
    sfirst = np.cumsum(spans)
    lengths = [t for _, t, _ in items]
    for max_spans in (int(sfirst[-1]), int(sfirst[-1]) + 5, int(sfirst[11]) - 1, 0):
        walked = [bool(s <= max_spans) for s in sfirst]
        full = L.stream_layout(items, in_len, max_spans, align, missed=3)
        need = full["result"][0]
        check_placement(full, lengths, walked, align, L.UNBOUNDED)
        nw = walked.index(False) if False in walked else len(items)
        assert all(walked[:nw]) and not any(walked[nw:])                  # every stream behind the first that does not fit
        assert full["result"] == [need, nw, int(sfirst[-1]), sum(it[2] for it in items[:nw]), 3]
        for b, (st, total, nc) in enumerate(items):
            got = tuple(full[k][b] for k in ("out_cap", "decoded_len", "nchunks", "status"))
            assert got == ((total, total, nc, st) if walked[b] else (0, 0, 0, O.ERR_OUTPUT_TOO_SMALL))   # out_cap whatever the tail is
            assert walked[b] or full["out_off"][b] == 0
        assert L.stream_layout(items, in_len, max_spans, align, need, missed=3) == full
        for cap in (need - 1, 0, need // 2):
            if cap < 0:
                continue
            out = L.stream_layout(items, in_len, max_spans, align, cap)
            ranges, stopped = check_placement(out, lengths, walked, align, cap)
            first = min(nw, len(items) if stopped is None else stopped)
            assert out["result"][:4] == [need, first, int(sfirst[-1]), sum(items[b][2] for b in ranges)]
            for b, (st, total, nc) in enumerate(items):
                if walked[b]:
                    assert (out["decoded_len"][b], out["nchunks"][b]) == (total, nc)
                    assert out["status"][b] == (st if b in ranges else O.ERR_OUTPUT_TOO_SMALL)
    assert L.stream_layout([], [], 0, align)["result"] == [0, 0, 0, 0, 0]


def test_layout_of_the_case_lists_chains_into_the_decode_model():
    """The layout of the constructed streams, given to the decode plan as out_cap: every stream keeps the verdict it has alone with room for all it
    lists (the reason out_cap = decoded_len whatever the tail status is)."""
    cases = L.stream_cases()
    streams = list(cases.values())
    items = [L.stream_item(s) for s in streams]
    spans = sum((len(s) + L.SPAN - 1) // L.SPAN for s in streams)
    out = L.stream_layout(items, [len(s) for s in streams], spans, 64)
    status, out_len, _, result, _ = M.decode_plan(streams, out["out_cap"], out["result"][3], spans)
    assert result[0] == out["result"][3] and result[2] == out["result"][2]
    for b, s in enumerate(streams):
        assert (status[b], out_len[b]) == M.verdict(s, *M.serial_walk(s, 1 << 64)), list(cases)[b]
    names = list(cases)
    assert status[names.index("bad_crc")] == O.ERR_CRC_MISMATCH and status[names.index("type_02")] == O.ERR_CHUNK_TYPE
    assert status[names.index("at_bound")] != O.OK and status[names.index("skippable")] == O.OK

"""libsnappier_hip_frame_cuts.so without a GPU: the declarations and their C# binding, argument rejection, the workspace arithmetic; the model
of the cut rule (frame_cuts_model.py) against every pinned value, its invariants and the re-synchronisation behind an edit; the model of the
encoder at given cuts against frame_chunked_model at regular cuts and on bad lists; and the rule header (csrc/frame_cuts_device.h) itself,
compiled for the CPU under AddressSanitizer and UBSan into a stand-alone program (tests/abi/frame_cuts_rule_check.hip) and run over cases the
model writes out, offsets past 2^32 among them."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import frame_chunked_model as K
import frame_cuts_model as F
import oracle as O
from conftest import ROOT, read_testdata

NAMES = ["snp_content_cuts_batch", "snp_content_cuts_workspace", "snp_frame_encode_cuts_batch", "snp_frame_encode_cuts_workspace"]
U64 = (1 << 64) - 1


def _lib():
    from snappier_amd import _native as N
    return N.frame_cuts_lib()


@pytest.fixture(scope="module")
def content():
    html = read_testdata("html")
    rnd = np.random.default_rng(3).integers(0, 256, 200000, dtype=np.uint8).tobytes()
    period = np.random.default_rng(1).integers(0, 256, 64, dtype=np.uint8).tobytes()
    return html, rnd, period


# ---- the surface -----------------------------------------------------------------------------------------------------------------------------
def test_header_binding_and_library_declare_the_new_functions():
    from layouts import exported
    from snappier_amd import _native as N
    import snappier_amd as S
    assert N.frame_cuts_declared_symbols() == NAMES
    others = set(N.declared_symbols())
    for name in N._EXTENSIONS:
        if name != "frame_cuts":
            others |= set(N.declared_symbols(N._extension_header(name)))
            assert not exported(N._extension_path(name)) & set(NAMES)
    assert not set(NAMES) & others                                      # the other headers' surfaces are left as they are
    assert exported(N.FRAME_CUTS_PATH) == set(NAMES) and not exported(N.PRODUCT_PATH) & set(NAMES)
    lib = _lib()
    assert lib.snp_content_cuts_batch.restype is C.c_int and len(lib.snp_content_cuts_batch.argtypes) == 14
    assert lib.snp_frame_encode_cuts_batch.restype is C.c_int and len(lib.snp_frame_encode_cuts_batch.argtypes) == 22
    assert (S.CUTS_MIN_WINDOW, S.CUTS_MAX_WINDOW) == (F.MIN_WINDOW, F.MAX_WINDOW) == (32, 32767)
    dev = open(os.path.join(ROOT, "snappier_amd", "csrc", "frame_cuts_device.h")).read()
    for name, value in (("kCutsTile", S.CUTS_TILE), ("kCutsBlock", S.CUTS_BLOCK), ("kCutsRun", S.CUTS_RUN)):
        assert re.search(r"constexpr u32 %s = %d;" % (name, value), dev), name


def test_csharp_binding_matches_the_extension_header():
    import test_csharp_signatures as T
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "snappier_hip_frame_cuts.h")).read(), flags=re.S)
    protos = {}
    for m in re.finditer(r"([A-Za-z_][A-Za-z0-9_ ]*?[\s\*]+)(snp_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", text):
        params = [re.match(r"(.*?[\s\*])([A-Za-z_][A-Za-z0-9_]*)$", q.strip()).group(1) for q in m.group(3).split(",") if q.strip() not in ("", "void")]
        protos[m.group(2)] = (T.c_class(m.group(1)), [T.c_class(q) for q in params])
    cs = re.sub(r"//.*", "", open(os.path.join(ROOT, "csharp", "Snappier.Gpu", "NativeMethodsFrameCuts.cs")).read())
    assert 'const string Lib = "snappier_hip_frame_cuts"' in cs
    imps = {}
    for m in re.finditer(r"\[DllImport\(Lib, CallingConvention = Cc\)\]\s*internal static extern ([A-Za-z\*]+) (snp_[a-z0-9_]+)\(([^)]*)\);", cs):
        params = [re.match(r"(.*?)\s+([A-Za-z_][A-Za-z0-9_]*)$", q.strip()).group(1) for q in m.group(3).split(",") if q.strip()]
        imps[m.group(2)] = (T.cs_class(m.group(1)), [T.cs_class(q) for q in params])
    assert set(protos) == set(imps) == set(NAMES)
    for name, (ret, params) in protos.items():
        cret, cparams = imps[name]
        assert T.compatible(ret, cret), (name, ret, cret)
        assert len(params) == len(cparams) and all(T.compatible(a, b) for a, b in zip(params, cparams)), (name, params, cparams)
    assert [len(protos[n][1]) for n in NAMES] == [14, 3, 22, 3]
    proj = open(os.path.join(ROOT, "csharp", "Snappier.Gpu", "Snappier.Gpu.csproj")).read()
    assert 'Include="../../snappier_amd/libsnappier_hip_frame_cuts.so"' in proj


def test_workspaces_are_host_arithmetic_within_the_documented_bounds():
    lib = _lib()
    cw, ew = lib.snp_content_cuts_workspace, lib.snp_frame_encode_cuts_workspace
    assert cw(0, 1 << 30, 64) == 0 and ew(0, 100, 1000) == 0            # nothing when there is no buffer
    assert cw(1, 1 << 20, 31) == 0 and cw(1, 1 << 20, 32768) == 0       # no workspace for a window outside the rule
    for span in (0, 1, 4096, 1 << 20, (1 << 30) + 5, 10 << 30):
        for nb in (1, 2, 1000, 100000):
            sizes = {cw(nb, span, w) for w in (32, 33, 2048, 32767)}
            assert len(sizes) == 1                                      # the same at every window
            size = sizes.pop()
            assert size % 256 == 0 and cw(nb + 1, span, 64) >= size and cw(nb, span + 4096, 64) >= size
            # no hash word per byte: below one eighth of the span, plus per-buffer words and the rounding of the pieces
            assert size <= span // 13 + 332 * nb + 16 * 256 + 8 * 1024
            assert size < span // 8 + 332 * nb + 16 * 256 + 8 * 1024
    assert cw(1, 1 << 62, 64) == cw(1, 1 << 40, 64)                     # the span is clamped
    for nb in (1, 7, 1000):
        for mc in (0, 1, 255, 70001):
            for sc in (0, 1, 5000, 1 << 32):
                size = ew(nb, mc, sc)
                assert size % 256 == 0 and ew(nb, mc + 1, sc) >= size and ew(nb + 1, mc, sc) >= size and ew(nb, mc, sc + 256) >= size
                assert sc + 64 * mc <= size <= sc + (56 + 64) * mc + 56 * nb + 20 * 256 + 8 * 1024
    # the bound for stage_cap: no batch of pieces needs more
    rng = np.random.default_rng(5)
    for _ in range(50):
        pieces = [int(v) for v in rng.integers(1, 65537, int(rng.integers(1, 40)))]
        assert sum(F.stride(p) for p in pieces) <= F.stage_bound(sum(pieces), len(pieces))
    assert F.stride(65536) == 76496 + 16 and F.stride(1) == 64 and all(F.stride(p) <= p + p // 6 + 69 for p in range(0, 70000, 7))


def test_batch_calls_reject_bad_arguments_without_a_device():
    lib = _lib()
    find, enc = lib.snp_content_cuts_batch, lib.snp_frame_encode_cuts_batch
    fake = C.c_void_p(64)                                               # (never dereferenced: the arguments are refused first)
    n3, f3 = [None] * 3, [fake] * 3
    # ctx, in / in_off / in_len, nbuffers, window, max_bytes, span_bytes, max_cuts, cut_first, cuts, status, d_work, d_result
    assert find(None, *n3, 0, 64, 1024, 0, 0, None, None, None, None, fake) == O.ERR_BAD_ARG
    assert find(fake, *n3, 0, 64, 1024, 0, 0, None, None, None, None, None) == O.ERR_BAD_ARG          # no d_result
    for w, mx in ((31, 1024), (32768, 65536), (64, 64), (64, 63), (64, 65537), (0, 1)):
        assert find(fake, *f3, 1, w, mx, 100, 10, fake, fake, fake, fake, fake) == O.ERR_BAD_ARG, (w, mx)
        assert find(fake, *n3, 0, w, mx, 0, 0, None, None, None, None, fake) == O.ERR_BAD_ARG, (w, mx)   # ... also in an empty batch
    assert find(fake, *f3, 1 << 30, 64, 1024, 100, 10, fake, fake, fake, fake, fake) == O.ERR_BAD_ARG
    for i in range(7):                                                  # any one null among the seven arrays of a batch
        a = [fake] * 7
        a[i] = None
        assert find(fake, *a[:3], 1, 64, 1024, 100, 10, a[3], a[4], a[5], a[6], fake) == O.ERR_BAD_ARG, i
    # ctx, in / in_off / in_len, nbuffers, cut_first, cuts, ncuts, max_chunks, stage_cap, out / out_off / out_cap / out_len / status, the index, d_work, d_result
    n5, f5 = [None] * 5, [fake] * 5
    assert enc(None, *n3, 0, None, None, 0, 0, 0, *n5, *n5, None, fake) == O.ERR_BAD_ARG
    assert enc(fake, *n3, 0, None, None, 0, 0, 0, *n5, *n5, None, None) == O.ERR_BAD_ARG              # no d_result
    assert enc(fake, *n3, 1, None, None, 0, 0, 0, *n5, *n5, None, fake) == O.ERR_BAD_ARG              # buffers, no arrays
    assert enc(fake, *f3, 1, fake, None, 1, 1, 100, *f5, *n5, fake, fake) == O.ERR_BAD_ARG            # cuts counted, none given
    for given in range(1, 31):                                          # an index given in part
        ix = [fake if given >> i & 1 else None for i in range(5)]
        assert enc(fake, *f3, 1, fake, fake, 1, 1, 100, *f5, *ix, fake, fake) == O.ERR_BAD_ARG, given
        assert enc(fake, *n3, 0, None, None, 0, 0, 0, *n5, *ix, None, fake) == O.ERR_BAD_ARG, given
    for i in range(10):                                                 # any one null among the ten arrays of a batch
        a = [fake] * 10
        a[i] = None
        assert enc(fake, *a[:3], 1, a[3], fake, 1, 1, 100, *a[4:9], *f5, a[9], fake) == O.ERR_BAD_ARG, i


# ---- the rule: every pin ---------------------------------------------------------------------------------------------------------------------------
def test_gear_and_hash_pins():
    assert [int(F.GEAR[b]) for b in (0, 1, 2, 97, 255)] == [0x92CA2F0E, 0x3CD6E3F3, 0x1B147DCC, 0xF2EBE3A2, 0x7970D887]
    g = F.hashes(bytes(range(32)))
    assert int(g[32]) == 0x16AF8A9F and int(g[0]) == 0
    # the recurrence, step by step, is what hashes() unrolls; g(c) depends on the 32 bytes before c only
    x = np.random.default_rng(9).integers(0, 256, 300, dtype=np.uint8).tobytes()
    h, want = 0, [0]
    for b in x:
        h = ((h << 1) + int(F.GEAR[b])) & F.M32
        want.append(h)
    assert F.hashes(x).tolist() == want
    assert F.hashes(x[100:132])[32] == F.hashes(x)[132]


def test_pins_on_html(content):
    html = content[0]
    assert len(html) == 102400
    c, forced = F.cuts_of(html[:20000], 64, 1024)
    assert (len(c), forced, c[:6], c[-2:], sum(c)) == (146, 0, [160, 285, 369, 476, 691, 781], [19521, 19809], 1426291)
    c, _ = F.cuts_of(html[:20000], 32, 65536)
    assert (len(c), c[:6], sum(c)) == (301, [160, 201, 285, 369, 476, 540], 3077701)
    c, forced = F.cuts_of(html, 1000, 4096)
    assert (len(c), forced, c[:3], sum(c)) == (50, 3, [2212, 4476, 5648], 2379270)
    c, _ = F.cuts_of(html, 4096, 65536)
    assert (len(c), c[0], c[-1], sum(c)) == (11, 9017, 91920, 533131)


def test_pins_on_synthetic_inputs(content):
    period = content[2]
    assert F.cuts_of(bytes(200000), 32, 65536) == ([65536, 131072, 196608], 3)
    x = period * 200
    c, forced = F.cuts_of(x, 100, 4096)                                 # the period is shorter than the window: every value ties to its left
    assert forced == len(c) == (len(x) - 1) // 4096 and c == list(range(4096, len(x), 4096)) and F.content_cuts(x, 100) == []
    c, forced = F.cuts_of(x, 40, 4096)                                  # content cuts 64 apart
    assert forced == 0 and len(c) > 190 and {b - a for a, b in zip(c, c[1:])} == {64}


def test_mean_piece_is_about_two_windows(content):
    html, rnd, _ = content
    for x in (rnd, html):
        for w, lo, hi in ((64, 120, 135), (512, 940, 1100)):
            c, _ = F.cuts_of(x, w, 65536)
            assert lo < len(x) / (len(c) + 1) < hi, (w, len(x) / (len(c) + 1))


# ---- the rule: invariants ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,mx", [(32, 33), (33, 100), (64, 1024), (1000, 1001), (1000, 4096), (4096, 65536), (32767, 32768)])
def test_cuts_are_far_apart_pieces_are_short_and_the_bound_holds(content, w, mx):
    html, rnd, period = content
    for x in (html, rnd[:70001], bytes(70000), period * 1100, html[:2 * w + 3], b"", b"a"):
        cc = F.content_cuts(x, w)
        assert all(b - a > w for a, b in zip(cc, cc[1:])) and all(w < c < len(x) - w for c in cc)
        c, forced = F.cuts_of(x, w, mx)
        assert c == sorted(set(c)) and all(0 < v < len(x) for v in c) and set(cc) <= set(c) and forced == len(c) - len(cc)
        assert all(1 <= b - a <= mx for a, b in zip([0] + c, c + [len(x)])) or not x
        assert len(c) <= F.cut_bound(len(x), w, mx)
    for n in (0, 1, w, 2 * w, 2 * w + 1):                               # too short for a content cut: forced cuts only
        x = rnd[:n]
        assert F.content_cuts(x, w) == [] and F.cuts_of(x, w, mx)[0] == list(range(mx, n, mx))
    assert not F.params_ok(31, 1000) and not F.params_ok(32768, 65536) and not F.params_ok(64, 64) and not F.params_ok(64, 65537)
    assert F.params_ok(32, 33) and F.params_ok(32767, 65536)


@pytest.mark.parametrize("w", [64, 512])
def test_cuts_fall_back_into_step_behind_an_edit(content, w):
    html, rnd, _ = content
    a = html + rnd[:50000]
    ins = rnd[60000:60037]
    cc = F.content_cuts(a, w)
    for at in (len(a) // 3, 5, 40000, len(a) - 7, cc[10], cc[10] - w - 31):
        for name, b, end, shift in (("insert", a[:at] + ins + a[at:], at, 37), ("delete", a[:at] + a[at + 37:], at + 37, -37),
                                    ("replace", a[:at] + ins + a[at + 37:], at + 37, 0)):
            cb = F.content_cuts(b, w)
            assert [c for c in cc if c < at - w] == [c for c in cb if c < at - w], (name, at)      # before at - w: unchanged
            # beyond w + 32 of the edit: the same content cuts, shifted -- except within w of the end, where the other end decides
            behind = [c + shift for c in cc if c > end + w + 32]
            assert behind == [c for c in cb if c > end + shift + w + 32], (name, at)
            # the forced cuts follow from the content cuts: all cuts before the last unchanged content cut are equal too
            ca, cbb = F.cuts_of(a, w, 4 * w)[0], F.cuts_of(b, w, 4 * w)[0]
            last = max([c for c in cc if c < at - w], default=0)
            assert [c for c in ca if c <= last] == [c for c in cbb if c <= last]


# ---- the finder's plan -----------------------------------------------------------------------------------------------------------------------------
def test_finder_admission_in_the_model(content):
    html, rnd, _ = content
    blobs = [html[:9000], rnd[:5000], b"", html[3:3 + 20000], rnd[:100]]
    full = F.find(blobs, 64, 1024)
    need = full["result"][0]
    assert full["status"] == [O.OK] * 5 and full["result"] == [need, need, 34100, 5] and full["cut_first"][-1] == need == len(full["cuts"])
    assert full["cut_first"][2] == full["cut_first"][3] and full["cut_first"][4] == full["cut_first"][5]    # 0 and 100 bytes: no cut
    assert F.find(blobs, 64, 1024, max_cuts=need + 3) == full
    sizing = F.find(blobs, 64, 1024, max_cuts=0)
    assert sizing["status"] == [O.ERR_OUTPUT_TOO_SMALL] * 5 and sizing["result"] == [need, 0, 34100, 0] and sizing["cut_first"] == [0] * 6
    span = F.find(blobs, 64, 1024, span_bytes=14000)
    assert span["status"] == [O.OK] * 3 + [O.ERR_OUTPUT_TOO_SMALL] * 2 and span["result"] == [full["cut_first"][3]] * 2 + [34100, 3]
    assert F.find([], 64, 1024)["result"] == [0] * 4 and F.find([b"", b""], 64, 1024, 0, 0)["status"] == [O.OK] * 2


# ---- the encoder's model ---------------------------------------------------------------------------------------------------------------------------
def test_regular_cuts_are_the_chunked_model(content):
    html, rnd, _ = content
    for cb in (1000, 4096, 65536):
        blobs = [html[:n] for n in K.buffer_lengths(cb)[:6]] + [rnd[:min(2 * cb + 3, 70001)]]
        first, cuts = F.regular_cuts([len(x) for x in blobs], cb)
        for variant in (O.HASH_CRC32C, O.HASH_MUL):
            caps = [K.frame_cap(len(x), cb) for x in blobs]
            assert F.encode_at_cuts(blobs, first, cuts, variant, caps=caps) == K.encode(blobs, cb, variant)
        need = sum(K.nchunks(len(x), cb) for x in blobs)
        assert F.encode_at_cuts(blobs, first, cuts, max_chunks=need - 2, caps=caps) == K.encode(blobs, cb, max_chunks=need - 2)
        exact = K.encode(blobs, cb)["out_len"]
        exact[3] -= 1
        assert F.encode_at_cuts(blobs, first, cuts, caps=exact) == K.encode(blobs, cb, caps=exact)
        assert F.encode_at_cuts(blobs, first, cuts, caps=caps, with_index=False) == K.encode(blobs, cb, with_index=False)
    assert F.encode_at_cuts([], [0], []) == K.encode([], 4096)


def test_found_cuts_encode_to_streams_that_decode_and_index(content):
    import frame_index_model as X
    html, rnd, _ = content
    blobs = [html[:30000], b"", rnd[:9000] + html[:9000], html[:1]]
    f = F.find(blobs, 64, 1024)
    m = F.encode_at_cuts(blobs, f["cut_first"], f["cuts"])
    assert m["status"] == [O.OK] * 4 and m["result"][0] == len(f["cuts"]) + 3
    for raw, s in zip(blobs, m["streams"]):
        assert O.frame_decode(s) == raw
    ix = X.build_index(m["streams"])
    assert [m[k] for k in ("first", "start", "pos", "total", "tail")] == [ix[k] for k in ("first", "start", "pos", "total", "tail")]


def test_bad_cut_lists_get_their_verdicts(content):
    html = content[0]
    n = 5000
    good = [1000, 2000, 4999]
    for bad in ([1000, 3000, 2000], [1000, 1000], [0, 1000], [1000, n], [1000, n + 1], [1000, U64], [U64, 1000]):
        m = F.encode_at_cuts([html[:n]] * 3, [0, 3, 3 + len(bad), 6 + len(bad)], good + bad + good)
        assert m["status"] == [O.OK, O.ERR_BAD_ARG, O.OK] and m["first"] == [0, 4, 4, 8] and m["result"] == [8, 2 * m["out_len"][0], 8, 2], bad
        assert m["streams"][1] is None and m["tail"] == [O.OK, O.ERR_BAD_ARG, O.OK] and m["total"] == [n, 0, n]
    long = html * 2
    assert F.list_verdict(140000, 0, 1, [65537])[0] is False and F.list_verdict(140000, 0, 2, [65536, 131072])[0] is True
    assert F.list_verdict(65537, 0, 0, [])[0] is False and F.list_verdict(65536, 0, 0, []) == (True, [(0, 65536)])
    assert F.list_verdict(140000, 0, 2, [10, 65547])[0] is False and F.list_verdict(140000, 0, 1, [140000 - 65537])[0] is False
    assert F.list_verdict(0, 0, 0, []) == (True, []) and F.list_verdict(0, 0, 1, [1])[0] is False
    assert F.list_verdict(n, 3, 2, good + good)[0] is False and F.list_verdict(n, 3, 7, good + good)[0] is False     # decreasing; beyond ncuts
    assert F.list_verdict(n, 0, 3, good + good, ncuts=2)[0] is False
    m = F.encode_at_cuts([long[:140000], html[:n]], [0, 1, 4], [65537] + good)
    assert m["status"] == [O.ERR_BAD_ARG, O.OK] and m["result"][0] == 4 and m["first"] == [0, 0, 4]       # a bad list counts nothing
    # admission by stage_cap is a prefix over the good buffers
    blobs = [html[:2500], html[:7001], html[:77]]
    first, cuts = F.regular_cuts([len(x) for x in blobs], 1000)
    s0 = 2 * F.stride(1000) + F.stride(500)
    m = F.encode_at_cuts(blobs, first, cuts, stage_cap=s0)
    assert m["status"] == [O.OK, O.ERR_OUTPUT_TOO_SMALL, O.ERR_OUTPUT_TOO_SMALL] and m["result"][0] == 12
    assert F.encode_at_cuts(blobs, first, cuts, stage_cap=s0 - 1)["status"] == [O.ERR_OUTPUT_TOO_SMALL] * 3


# ---- the rule header on the CPU, under sanitizers ------------------------------------------------------------------------------------------------
def test_rule_header_under_sanitizers_matches_the_model(content, tmp_path):
    html, rnd, period = content
    rule = [(64, 1024, html[:20000]), (32, 65536, html[:6000]), (32, 33, rnd[:3000]), (33, 34, html[:70]), (100, 4096, period * 150),
            (40, 4096, period * 150), (32, 65536, bytes(70000)), (1000, 1001, html[:9000]), (64, 100, b""), (64, 100, b"a"),
            (64, 100, rnd[:129]), (64, 100, rnd[:130]), (64, 100, rnd[:131]), (31, 100, rnd[:500]), (64, 64, rnd[:500])]
    rule = [r for r in rule if F.params_ok(r[0], r[1])] + [(64, 65536, rnd[:2000])]
    n = 5000
    good = [1000, 2000, 4999]
    big = (1 << 32) + 100000                                            # a synthetic length: no such buffer is allocated
    grid = list(range(65536, big, 65536))
    lists = [(n, 0, 3, 6, good + good, [0, 1, 2, 3], [0, 1, 999, 1000, 1001, 4999, 5000]),
             (n, 3, 6, 6, good + good, [0, 3], [0, 2000, 2001]),
             (n, 0, 3, 3, [1000, 3000, 2000], [], []), (n, 0, 2, 2, [1000, 1000], [], []), (n, 0, 2, 2, [0, 1000], [], []),
             (n, 0, 2, 2, [1000, n], [], []), (n, 0, 2, 2, [1000, U64], [], []), (n, 0, 2, 2, [U64, 1000], [], []),
             (n, 3, 2, 6, good + good, [], []), (n, 3, 7, 6, good + good + [1], [], []), (n, 0, U64, 6, good + good, [], []),
             (n, U64, 3, 6, good + good, [], []), (n, 0, 3, 2, good, [], []),
             (140000, 0, 1, 1, [65537], [], []), (140000, 0, 2, 2, [65536, 131072], [0, 1, 2], [65536, 65537, 131072, 139999]),
             (65537, 0, 0, 0, [], [], []), (65536, 0, 0, 0, [], [0], [0, 1]), (0, 0, 0, 0, [], [], [0]), (0, 0, 1, 1, [1], [], []),
             (big, 0, len(grid), len(grid), grid, [0, 1, 65535, 65536, len(grid)], [0, 1, 65536, (1 << 32) - 1, 1 << 32, (1 << 32) + 1, big - 1]),
             (big + 65536, 0, len(grid), len(grid), grid, [], []),     # the last piece: 65 536 + 34 464 bytes
             (1 << 63, 0, 1, 1, [(1 << 63) - 5], [], [])]
    forced = [(0, 0, 200000, 65536), (0, 4096, 8192, 4096), (0, 4097, 8192, 4096), (100, 100, 101, 33), (100, 100, 133, 33), (100, 100, 134, 33),
              (5, 4096, 8192, 33), ((1 << 32) - 7, 1 << 32, (1 << 32) + 4096, 65536), ((1 << 32) - 7, 1 << 32, (1 << 32) + 4096, 33),
              (0, 1 << 40, (1 << 40) + 4096, 65536), (7, 7, 7, 100), (9, 4, 9, 100)]
    forced = [q for q in forced if q[1] >= q[0] or q[2] <= q[0]]
    joins = [(0, 0), (0, 5), (1, 5), (0, (1 << 33) + 3), ((1 << 32) - 1, (1 << 32) - 1), ((1 << 32) - 1, 1 << 32), (1 << 32, 0), (U64 >> 1, 7)]
    path = str(tmp_path / "cases.bin")
    F.write_cases(path, rule, lists, forced, joins)
    exe = str(tmp_path / "frame_cuts_rule_check")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host",
                    "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "abi", "frame_cuts_rule_check.hip"), "-o", exe,
                    "-Wl,-rpath,/opt/rocm/lib"], check=True)
    env = {**os.environ, "ASAN_OPTIONS": "detect_leaks=1:abort_on_error=0", "UBSAN_OPTIONS": "print_stacktrace=1:halt_on_error=1"}
    run = subprocess.run([exe, path], capture_output=True, text=True, env=env)
    assert run.returncode == 0 and run.stderr == "", run.stderr[-3000:]      # the sanitizers are silent
    lines = run.stdout.splitlines()
    want = F.check_lines(rule, lists, forced, joins)
    assert len(lines) == len(want)
    for i, (got, exp) in enumerate(zip(lines, want)):
        assert got == exp, (i, got[:200], exp[:200])
    # the cases reach what they are for: the pins, pieces and offsets past 2^32, a saturated sum
    assert want[0] == "92ca2f0e 3cd6e3f3 1b147dcc f2ebe3a2 7970d887 16af8a9f"
    assert want[1].startswith("R 1 146 0 326 160 285 369 476 691 781 ") and want[7].startswith("R 1 1 1 ") and want[7].endswith(" 65536")
    past = [w for w in want if w.startswith("P ") and "4294967296:65536" in w]
    assert len(past) == 1 and past[0] == "P 0:65536 65536:65536 4294901760:65536 4294967296:65536 4295032832:34464"
    assert "A 0 1 1 65536 65536 65537 65538" in want and "V 1 65538 %d" % (65537 * F.stride(65536) + F.stride(34464)) in want
    assert "J 18446744073709551615" in want and "F 3 1" in want

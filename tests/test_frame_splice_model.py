"""snp_frame_splice_indexed_batch (libsnappier_hip_frame_splice.so) without a GPU: the declarations and their C# binding, the workspace arithmetic,
argument rejection; the Python model of the contract (frame_splice_model.py) checked against the oracle's frame decode, the index model, the
chunked encoder's model and the update call's model over the named splices at the seam chunk sizes and on foreign streams; corruption in an
edge, in a wholly deleted chunk and outside the hole; admission and out_cap; every rejection; unsound indexes; and the planning header
(csrc/frame_splice_device.h) itself, compiled for the CPU under AddressSanitizer and UBSan into a stand-alone program
(tests/abi/frame_splice_plan_check.hip) and run over the same cases, over indexes filled with anything at all and over streams past 4 GiB given
as numbers."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import frame_buffers_model as M
import frame_chunked_model as K
import frame_index_model as X
import frame_range_model as R
import frame_splice_model as S
import frame_update_model as U
import oracle as O
from conftest import ROOT, read_testdata

NAMES = ["snp_frame_splice_indexed_batch", "snp_frame_splice_indexed_workspace"]
BIG = 1 << 62


def _lib():
    from snappier_amd import _native as N
    return N.frame_splice_lib()


# ---- the surface -----------------------------------------------------------------------------------------------------------------------------
def test_header_and_binding_declare_the_new_functions():
    from snappier_amd import _native as N
    declared = N.frame_splice_declared_symbols()
    assert sorted(declared) == NAMES
    others = set(N.declared_symbols()) | set(N.buffers_declared_symbols()) | set(N.buffers_decompress_declared_symbols()) | \
        set(N.frame_buffers_declared_symbols()) | set(N.layout_declared_symbols()) | set(N.frame_range_declared_symbols()) | \
        set(N.frame_index_declared_symbols()) | set(N.frame_chunked_declared_symbols()) | set(N.frame_update_declared_symbols()) | \
        set(N.frame_append_declared_symbols())
    assert not set(declared) & others                                  # the other headers' surfaces are left as they are
    lib = _lib()
    assert lib.snp_frame_splice_indexed_batch.restype is C.c_int and len(lib.snp_frame_splice_indexed_batch.argtypes) == 32
    assert lib.snp_frame_splice_indexed_workspace.restype is C.c_uint64 and len(lib.snp_frame_splice_indexed_workspace.argtypes) == 4
    from snappier_amd import batch as SB
    assert callable(SB.BlockCodec.frame_splice_indexed) and callable(SB.BlockCodec.frame_splice_to_memory)


def test_extension_library_exports_exactly_its_header():
    from layouts import exported
    from snappier_amd import _native as N

    ext = exported(N.FRAME_SPLICE_PATH)
    assert ext == set(NAMES)
    for other in (N.PRODUCT_PATH, N.BUFFERS_PATH, N.BUFFERS_DECOMPRESS_PATH, N.FRAME_BUFFERS_PATH, N.LAYOUT_PATH, N.FRAME_RANGE_PATH, N.FRAME_INDEX_PATH,
                  N.FRAME_CHUNKED_PATH, N.FRAME_UPDATE_PATH, N.FRAME_APPEND_PATH):
        assert not exported(other) & ext


def test_workspace_is_host_arithmetic():
    ws = _lib().snp_frame_splice_indexed_workspace
    assert ws(0, 10, 1000, 4096) == 0                                   # nothing when there is no stream
    assert ws(5, 10, 1000, 0) == 0 and ws(5, 10, 1000, 65537) == 0      # ... or no chunk size the call takes
    for ns in (1, 255, 1025, 300000):
        for ms in (0, 1, 33000):
            for sc in (0, 1, 70000, 1 << 33):
                for cb in (1, 64, 4096, 65536):
                    w = ws(ns, ms, sc, cb)
                    stride = K.stride(cb)
                    assert w % 256 == 0
                    # the staging, the compressed staging and the slot table, the streams' words (14 + 4 of 8 bytes, 6 of 4) and their two decode rows of 41 bytes
                    assert w >= sc + ms * (stride + 44) + ns * (168 + 82)
                    assert w <= sc + 256 + ms * (stride + 44) + ns * 250 + 70 * 256 + (2 * ns + ms) // 50
                    assert ws(ns + 1, ms, sc, cb) >= w and ws(ns, ms + 1, sc, cb) >= w and ws(ns, ms, sc + 1, cb) >= w
    assert ws(0x7FFFFFFF, 0xFFFFFFFF, 1 << 40, 65536) > 0xFFFFFFFF * 76496 + (1 << 40)      # (64-bit arithmetic)


def test_batch_call_rejects_bad_arguments_without_a_device():
    call = _lib().snp_frame_splice_indexed_batch
    fake = C.c_void_p(64)                                               # (never dereferenced: the arguments are refused first)
    # ctx; in, in_off, in_len; nstreams; five index arrays; nentries; src, sp_off, sp_del, sp_ins, src_off; chunk_bytes, max_slots, stage_cap;
    # out, out_off, out_cap, out_len, status; five new index arrays; out_bound; d_work, d_result
    def args(ctx=fake, ins=(fake,) * 3, ns=1, idx=(fake,) * 5, ne=8, srcs=(fake,) * 5, cb=4096, ms=0, sc=0, outs=(fake,) * 5, new=(fake,) * 5,
             bound=None, work=fake, result=fake):
        return (ctx, *ins, ns, *idx, ne, *srcs, cb, ms, sc, *outs, *new, bound, work, result)

    assert call(*args(ctx=None)) == O.ERR_BAD_ARG
    assert call(*args(result=None)) == O.ERR_BAD_ARG
    assert call(*args(ns=0, result=None)) == O.ERR_BAD_ARG             # an empty call still needs d_result
    assert call(*args(cb=0)) == O.ERR_BAD_ARG and call(*args(cb=65537)) == O.ERR_BAD_ARG
    assert call(*args(ns=0, cb=0)) == O.ERR_BAD_ARG                    # ... also when there is no stream
    assert call(*args(ns=1 << 31)) == O.ERR_BAD_ARG
    assert call(*args(work=None)) == O.ERR_BAD_ARG
    for group, n in (("ins", 3), ("srcs", 5), ("outs", 5)):
        for i in range(n):
            a = [fake] * n
            a[i] = None
            assert call(*args(**{group: tuple(a)})) == O.ERR_BAD_ARG, (group, i)
    for i in (0, 3, 4):                                                 # idx_first, idx_total, idx_tail; new_first, new_total, new_tail
        a = [fake] * 5
        a[i] = None
        assert call(*args(idx=tuple(a))) == O.ERR_BAD_ARG, i
        assert call(*args(new=tuple(a))) == O.ERR_BAD_ARG, i
    for i in (1, 2):                                                    # rows, no row arrays
        a = [fake] * 5
        a[i] = None
        assert call(*args(idx=tuple(a))) == O.ERR_BAD_ARG and call(*args(new=tuple(a))) == O.ERR_BAD_ARG
        assert call(*args(new=tuple(a), ne=0, ms=1)) == O.ERR_BAD_ARG   # no old rows, room for new ones


def test_csharp_binding_matches_the_extension_header():
    import test_csharp_signatures as T
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "snappier_hip_frame_splice.h")).read(), flags=re.S)
    protos = {}
    for m in re.finditer(r"([A-Za-z_][A-Za-z0-9_ ]*?[\s\*]+)(snp_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", text):
        params = [re.match(r"(.*?[\s\*])([A-Za-z_][A-Za-z0-9_]*)$", q.strip()).group(1) for q in m.group(3).split(",") if q.strip() not in ("", "void")]
        protos[m.group(2)] = (T.c_class(m.group(1)), [T.c_class(q) for q in params])
    cs = re.sub(r"//.*", "", open(os.path.join(ROOT, "csharp", "Snappier.Gpu", "NativeMethodsFrameSplice.cs")).read())
    assert 'const string Lib = "snappier_hip_frame_splice"' in cs
    imps = {}
    for m in re.finditer(r"\[DllImport\(Lib, CallingConvention = Cc\)\]\s*internal static extern ([A-Za-z\*]+) (snp_[a-z0-9_]+)\(([^)]*)\);", cs):
        params = [re.match(r"(.*?)\s+([A-Za-z_][A-Za-z0-9_]*)$", q.strip()).group(1) for q in m.group(3).split(",") if q.strip()]
        imps[m.group(2)] = (T.cs_class(m.group(1)), [T.cs_class(q) for q in params])
    assert set(protos) == set(imps) == set(NAMES)
    for name, (ret, params) in protos.items():
        cret, cparams = imps[name]
        assert T.compatible(ret, cret), (name, ret, cret)
        assert len(params) == len(cparams) and all(T.compatible(a, b) for a, b in zip(params, cparams)), (name, params, cparams)
    assert len(protos["snp_frame_splice_indexed_batch"][1]) == 32 and len(protos["snp_frame_splice_indexed_workspace"][1]) == 4
    proj = open(os.path.join(ROOT, "csharp", "Snappier.Gpu", "Snappier.Gpu.csproj")).read()
    assert 'Include="../../snappier_amd/libsnappier_hip_frame_splice.so"' in proj


# ---- the model against the oracle ----------------------------------------------------------------------------------------------------------------
def named_batch(html: bytes, cb: int, variant: int):
    """One stream per named case: -> (names, raws, streams, reqs, srcs)."""
    cases = S.named_cases(cb)
    raws = [html[7 + i:7 + i + n] for i, (n, _, _, _) in enumerate(cases.values())]
    streams = [K.stream_of(a, cb, variant) if a else b"" for a in raws]
    reqs = [(off, dele) for _, off, dele, _ in cases.values()]
    srcs = [html[3001 + 5 * i:3001 + 5 * i + ins] for i, (_, _, _, ins) in enumerate(cases.values())]
    return list(cases), raws, streams, reqs, srcs


@pytest.mark.parametrize("cb", S.CHUNK_SIZES)
def test_named_splices_decode_to_the_edited_buffer_with_the_index_of_the_new_streams(cb):
    html = read_testdata("html") * 5
    for variant in (O.HASH_CRC32C, O.HASH_MUL):
        names, raws, streams, reqs, srcs = named_batch(html, cb, variant)
        ix = X.build_index(streams)
        got = S.splice_plan(streams, ix, reqs, srcs, cb, variant=variant)
        for b, name in enumerate(names):
            assert got["status"][b] == O.OK, name
            new, (off, dele) = got["streams"][b], reqs[b]
            if dele == 0 and not srcs[b]:                                # not named (at one byte per chunk, so are the splices of half a chunk)
                assert new is None and got["out_len"][b] == 0 and got["out_bound"][b] == 0 and (name == "not_named" or cb == 1)
                continue
            assert O.frame_decode(new) == S.edited(raws[b], off, dele, srcs[b]), (cb, name)
            assert got["out_len"][b] == len(new) <= got["out_bound"][b]
            p0, p1 = got["hole"][b]
            assert new[:p0] == streams[b][:p0] and (p1 == len(streams[b]) or new[-(len(streams[b]) - p1):] == streams[b][p1:]), name
        assert S.same_index(got["index"], X.build_index(S.after(streams, got))), cb
        slots, stage = S.needs(streams, ix, reqs, srcs, cb)
        assert got["result"] == [slots, sum(got["out_len"]), stage, sum(1 for r, s in zip(reqs, srcs) if r[1] or s)]
        assert S.splice_plan(streams, ix, reqs, srcs, cb, max_slots=slots, stage_cap=stage, variant=variant) == got
        whole = names.index("delete_whole_chunks")                      # exactly whole chunks: no new chunk, nothing staged
        assert got["index"]["first"][whole + 1] - got["index"]["first"][whole] == ix["first"][whole + 1] - ix["first"][whole] - 2
        assert got["out_bound"][whole] == got["out_len"][whole]


@pytest.mark.parametrize("cb", S.CHUNK_SIZES)
def test_byte_exact_consequences_against_the_chunked_encoder(cb):
    html = read_testdata("html") * 5
    a = html[11:11 + 4 * cb + (cb + 1) // 2]
    n = len(a)
    ins = [b"", html[5000:5000 + 1], html[5000:5000 + cb], html[5000:5000 + 2 * cb + 3]]
    # deletes to the end (hi == total): the encoder's output for A[:lo] || INS, whatever lo is; a pure truncate is the empty INS
    for lo in (0, 1, cb - 1, cb, cb + 1, 2 * cb + cb // 2, n - 1, n):
        lo = min(lo, n)
        reqs = [(lo, n - lo)] * len(ins)
        streams = [K.stream_of(a, cb)] * len(ins)
        got = S.splice_plan(streams, X.build_index(streams), reqs, ins, cb)
        for b, src in enumerate(ins):
            if n - lo == 0:                                             # nothing deleted: not named, or an insert at total, which owns no row --
                assert (got["streams"][b] is None) == (not src)         # fresh chunks behind the short tail (only the append call fills it up)
                assert not src or O.frame_decode(got["streams"][b]) == a + src
                continue
            assert got["status"][b] == O.OK and got["streams"][b] == K.stream_of(a[:lo] + src, cb), (cb, lo, len(src))
    # lo, hi and ins multiples of c (or hi == total): the encoder's output for the edited buffer
    aligned = [(0, cb, 2 * cb), (cb, 2 * cb, 0), (2 * cb, 0, cb), (cb, cb, 3 * cb), (3 * cb, n - 3 * cb, cb + 5), (0, 0, cb), (4 * cb, 0, 2 * cb)]
    streams = [K.stream_of(a, cb)] * len(aligned)
    srcs = [html[9000:9000 + k] for _, _, k in aligned]
    got = S.splice_plan(streams, X.build_index(streams), [(o, d) for o, d, _ in aligned], srcs, cb)
    for b, (off, dele, _) in enumerate(aligned):
        assert got["status"][b] == O.OK and got["streams"][b] == K.stream_of(S.edited(a, off, dele, srcs[b]), cb), (cb, off, dele)


def test_a_splice_that_keeps_the_length_decodes_to_what_the_update_writes():
    html = read_testdata("html") * 3
    for cb in (64, 4096):
        a = html[3:3 + 4 * cb + 9]
        s = K.stream_of(a, cb)
        ix = X.build_index([s])
        for off, ln in ((cb // 3, cb // 2), (cb, cb), (cb // 2, 2 * cb + 1), (len(a) - 1, 1), (0, len(a))):
            src = html[7777:7777 + ln]
            up = U.write_plan([s], ix, [(0, off, ln)], [src])
            sp = S.splice_plan([s], ix, [(off, ln)], [src], cb)
            assert up["status"] == sp["status"] == [O.OK]
            assert O.frame_decode(sp["streams"][0]) == O.frame_decode(up["streams"][0]) == S.edited(a, off, ln, src)
            assert sp["index"]["total"] == ix["total"]


def test_an_incompressible_edge_and_a_stream_written_with_larger_chunks():
    html = read_testdata("html") * 5
    rnd = bytes(np.random.default_rng(3).integers(0, 256, 3 * 4096, dtype=np.uint8))
    s = K.stream_of(rnd, 4096)
    assert s[10] == 1                                                   # type 0x01: stored as it is
    got = S.splice_plan([s], X.build_index([s]), [(100, 5000)], [html[:33]], 4096)
    assert got["status"] == [O.OK] and O.frame_decode(got["streams"][0]) == S.edited(rnd, 100, 5000, html[:33])
    assert got["result"][2] == 2 * 4096 + 100 + 33 + (2 * 4096 - 5100)   # both edges decoded whole, and the region
    a = html[:2 * 65536 + 1000]
    big = K.stream_of(a, 65536)
    ix = X.build_index([big])
    got = S.splice_plan([big], ix, [(70000, 10)], [html[:4096 + 5]], 4096)
    want = S.edited(a, 70000, 10, html[:4096 + 5])
    assert got["status"] == [O.OK] and O.frame_decode(got["streams"][0]) == want
    new = X.build_index(got["streams"])
    assert S.same_index(got["index"], new) and len(new["start"]) == 2 + (65536 - 10 + 4101 + 4095) // 4096
    assert got["streams"][0][:got["hole"][0][0]] == big[:got["hole"][0][0]]      # chunk 0 and chunk 2 are copies
    assert got["streams"][0].endswith(big[got["hole"][0][1]:])


def test_foreign_streams_drop_what_lies_in_the_hole_and_keep_what_lies_outside():
    html = read_testdata("html")
    cases = S.foreign_streams(html)
    streams = [c[0] for c in cases.values()]
    ix = X.build_index(streams)
    assert ix["tail"] == [O.OK] * len(streams)
    reqs = [(c[2][0], c[2][1]) for c in cases.values()]
    srcs = [html[4000:4000 + c[2][2]] for c in cases.values()]
    for cb in (64, 1000, 65536):
        got = S.splice_plan(streams, ix, reqs, srcs, cb)
        assert got["status"] == [O.OK] * len(streams)
        for b, (name, (s, raw, (off, dele, _), dropped)) in enumerate(cases.items()):
            new, (p0, p1) = got["streams"][b], got["hole"][b]
            assert O.frame_decode(new) == S.edited(raw, off, dele, srcs[b]), name
            assert new[:p0] == s[:p0] and new[len(new) - (len(s) - p1):] == s[p1:], name

            def non_data(x):                                            # every chunk that is no data chunk, in order
                out, ip = [], 0
                while ip < len(x):
                    h = M.hop(x, ip)
                    if h.kind == "skip":
                        out.append(x[ip:h.next])
                    ip = h.next
                return out
            assert (non_data(new) != non_data(s)) == dropped, name
            zero = lambda x: sum(1 for r in R.walk(x)[0] if r[5] == 0)
            if name == "zero_length_at_both_borders":
                assert zero(new) == zero(s) == 4
            if name == "zero_length_inside":
                assert zero(new) == 2
        assert S.same_index(got["index"], X.build_index(got["streams"]))


def test_corruption_in_an_edge_is_noticed_in_a_deleted_chunk_not_and_outside_the_hole_copied():
    html = read_testdata("html") * 2
    cb = 4096
    raw = html[:5 * cb]
    s = K.stream_of(raw, cb)
    rows = R.walk(s)[0]
    ix = X.build_index([s] * 5)
    bad = [R.corrupt_chunk(s, rows[i]) for i in (1, 2, 3, 4)]
    assert all(X.build_index([x])["pos"] == X.build_index([s])["pos"] for x in bad)
    req, src = (cb + 100, 2 * cb), html[9000:9050]                       # head edge: chunk 1, chunk 2 wholly deleted, tail edge: chunk 3
    got = S.splice_plan(bad + [s], ix, [req] * 5, [src] * 5, cb)
    want1, want3 = M.chunk_status(bad[0], rows[1]), M.chunk_status(bad[2], rows[3])
    assert want1 != O.OK and want3 != O.OK
    assert got["status"] == [want1, O.OK, want3, O.OK, O.OK]
    assert got["streams"][0] is None and got["out_len"][0] == 0 and got["out_bound"][0] == 0 and got["out_bound"][4] > 0
    assert got["streams"][1] == got["streams"][4]                       # the corrupt chunk is gone, not noticed
    p0, p1 = got["hole"][3]
    assert got["streams"][3][-(len(s) - p1):] == bad[3][p1:] != s[p1:]   # copied as it is
    with pytest.raises(O.OracleError):
        O.frame_decode(got["streams"][3])
    assert O.frame_decode(got["streams"][4]) == S.edited(raw, req[0], req[1], src)
    assert got["result"][3] == 3 and got["index"]["total"] == [5 * cb, 5 * cb - 2 * cb + 50, 5 * cb, 5 * cb - 2 * cb + 50, 5 * cb - 2 * cb + 50]
    # both edges corrupt: the head edge's status
    both = R.corrupt_chunk(bad[0], rows[3])
    assert S.splice_plan([both], X.build_index([s]), [req], [src], cb)["status"] == [want1]


def test_admission_is_in_stream_order_by_each_bound_and_out_cap_hits_one_stream():
    html = read_testdata("html")
    cb = 512
    blobs = [html[:700], html[50:50 + 1024], html[9:9 + 1300], html[:100], html[:2000]]
    streams = [K.stream_of(x, cb) for x in blobs]
    ix = X.build_index(streams)
    reqs = [(100, 50), (512, 512), (600, 0), (5, 0), (1000, 1000)]
    srcs = [html[3000:3000 + n] for n in (1000, 0, 100, 0, 2000)]
    full = S.splice_plan(streams, ix, reqs, srcs, cb)
    slots, stage = full["result"][0], full["result"][2]
    assert full["status"] == [O.OK] * 5
    # stream 0: row 0 split (512 decoded, region 512 - 50 + 1000); 1: a whole chunk, nothing; 2: row 1 split; 3: not named; 4: rows 1 .. 3,
    # a head edge of 512 bytes of which 488 stay, no tail edge
    assert slots == 3 + 0 + 2 + 0 + 5 and stage == (512 + 1462) + 0 + (512 + 612) + 0 + (512 + 488 + 2000)
    assert S.splice_plan(streams, ix, reqs, srcs, cb, max_slots=slots, stage_cap=stage) == full
    short = S.splice_plan(streams, ix, reqs, srcs, cb, max_slots=slots - 1, stage_cap=stage)
    assert short["status"] == [O.OK, O.OK, O.OK, O.OK, O.ERR_OUTPUT_TOO_SMALL] and short["streams"][:3] == full["streams"][:3]
    short = S.splice_plan(streams, ix, reqs, srcs, cb, max_slots=slots, stage_cap=512 + 1462 + 1123)
    assert short["status"] == [O.OK, O.OK, O.ERR_OUTPUT_TOO_SMALL, O.OK, O.ERR_OUTPUT_TOO_SMALL]      # the stream that misses, every later named one
    assert short["result"] == [slots, short["out_len"][0] + short["out_len"][1], stage, 2]
    assert short["index"]["total"] == [700 - 50 + 1000, 512, 1300, 100, 2000] and short["index"]["tail"] == [0] * 5
    none = S.splice_plan(streams, ix, reqs, srcs, cb, max_slots=2, stage_cap=stage)
    assert none["status"] == [O.ERR_OUTPUT_TOO_SMALL] * 3 + [O.OK, O.ERR_OUTPUT_TOO_SMALL] and none["streams"] == [None] * 5
    sizing = S.splice_plan(streams, ix, reqs, srcs, cb, caps=[0] * 5, max_slots=0, stage_cap=0)
    assert sizing["result"] == [slots, 0, stage, 0] and sizing["out_bound"] == full["out_bound"]
    assert all(b >= n for b, n in zip(sizing["out_bound"], full["out_len"])) and S.same_index(sizing["index"], ix)
    caps = list(full["out_len"])
    caps[2] -= 1                                                        # one byte short, in the middle
    mid = S.splice_plan(streams, ix, reqs, srcs, cb, caps=caps)
    assert mid["status"] == [O.OK, O.OK, O.ERR_OUTPUT_TOO_SMALL, O.OK, O.OK] and mid["streams"][2] is None and mid["out_len"][2] == 0
    assert S.same_index(mid["index"], X.build_index(S.after(streams, mid)))
    assert mid["result"] == [slots, sum(mid["out_len"]), stage, 3]


def test_every_rejection():
    html = read_testdata("html")
    cb = 1000
    streams = [K.stream_of(html[:n], cb) for n in (2500, 2000, 300)] + [R.uniform_stream(3, 1)[0][:-5]]
    ix = X.build_index(streams)
    assert ix["tail"][3] == O.ERR_TRUNCATED_STREAM
    src = [html[:700]] * 4

    def statuses(reqs=((10, 20),) * 4, srcs=src, **change):
        return S.splice_plan(streams, {**ix, **change}, list(reqs), srcs, cb)["status"]

    assert statuses() == [O.OK, O.OK, O.OK, O.ERR_TRUNCATED_STREAM]
    assert statuses(tail=[O.ERR_OUTPUT_TOO_SMALL, 0, 77, -1]) == [O.ERR_OUTPUT_TOO_SMALL, O.OK, O.ERR_BAD_ARG, O.ERR_BAD_ARG]
    assert statuses(reqs=[(2500, 1), (1999, 2), (S.U64, 2), (0, 0)])[:3] == [O.ERR_BAD_ARG] * 3        # above total; lo + del wraps
    assert statuses(reqs=[(2500, 0), (0, 2000), (300, 0), (0, 0)])[:3] == [O.OK] * 3                   # at total, everything
    assert statuses(total=[S.U64, 2000, 300, 0], reqs=[(0, 0)] * 4)[0] == O.ERR_BAD_ARG                # total - del + ins wraps
    assert statuses(total=[2501, 2000, 299, 0], reqs=[(2400, 10)] * 3 + [(0, 0)], srcs=[b""] * 4)[:3] == [O.ERR_BAD_ARG, O.ERR_BAD_ARG, O.ERR_BAD_ARG]
    assert statuses(pos=[p + 1 for p in ix["pos"]])[:3] == [O.ERR_BAD_ARG] * 3
    assert statuses(first=[0, 0, 3, 6, 6])[:3] == [O.ERR_BAD_ARG, O.OK, O.ERR_BAD_ARG]        # decoded bytes and no row; rows of a twin stream that fit the headers; rows that run backwards
    assert statuses(first=[0, 3, 5, 5, 6])[:3] == [O.OK, O.OK, O.ERR_BAD_ARG]
    assert statuses(first=[3, 0, 5, 6, 6])[0] == O.ERR_BAD_ARG                                         # f1 < f0
    assert statuses(start=list(reversed(ix["start"])))[0] == O.ERR_BAD_ARG                            # rows backwards
    assert statuses(reqs=[(0, 0)] * 4, srcs=[b""] * 4, tail=[5, 77, -3, 9]) == [O.OK] * 4              # not named: nothing is looked at
    # an insertion point on a row boundary must be a data chunk's header; one inside a wholly deleted row is checked as well
    skip = M.STREAM_ID + M.data_chunk(html[:100]) + M.chunk(0x80, b"note") + M.data_chunk(html[100:200])
    six = X.build_index([skip])
    assert S.splice_plan([skip], six, [(100, 0)], [b"x"], cb)["status"] == [O.OK]
    moved = {**six, "pos": [six["pos"][0], six["pos"][1] - 8]}          # at the skippable chunk
    assert S.splice_plan([skip], moved, [(100, 0)], [b"x"], cb)["status"] == [O.ERR_BAD_ARG]
    assert S.splice_plan([skip], moved, [(100, 100)], [b""], cb)["status"] == [O.ERR_BAD_ARG]
    # an edge chunk above 65536 bytes; the same chunk wholly deleted is fine
    big = R.big_chunk_stream()[0]
    bix = X.build_index([big])
    i = max(range(len(bix["start"])), key=lambda j: X.row_end(bix, len(bix["start"]), bix["total"][0], j) - bix["start"][j])
    s0, e0 = bix["start"][i], X.row_end(bix, len(bix["start"]), bix["total"][0], i)
    assert e0 - s0 > 65536
    assert S.splice_plan([big], bix, [(s0 + 1, 5)], [b""], 65536)["status"] == [O.ERR_BAD_ARG]
    assert S.splice_plan([big], bix, [(s0, e0 - s0)], [b""], 65536)["status"] == [O.OK]


@pytest.fixture(scope="module")
def named():
    cases = X.named_streams()
    streams = list(cases.values())
    return list(cases), streams, X.build_index(streams)


def middle_splices(ix, ns):
    """(off, del, ins) per stream: around the middle of what it decodes to, across a few hundred bytes."""
    out = []
    for b in range(ns):
        t = ix["total"][b]
        out.append((t // 2, min(t - t // 2, 300 + 7 * b), 100 + b))
    return out


def test_named_streams_splice_as_the_contract_says(named):
    names, streams, ix = named
    html = read_testdata("html")
    reqs3 = middle_splices(ix, len(streams))
    srcs = [html[b:b + r[2]] for b, r in enumerate(reqs3)]
    got = S.splice_plan(streams, ix, [r[:2] for r in reqs3], srcs, 4096)
    written = 0
    for b, s in enumerate(streams):
        if got["streams"][b] is not None:
            try:
                old = O.frame_decode(s)
            except O.OracleError:                                       # (a corrupt chunk outside the hole: copied)
                old = None
            if old is not None:
                assert O.frame_decode(got["streams"][b]) == S.edited(old, reqs3[b][0], reqs3[b][1], srcs[b]), names[b]
            written += 1
        else:
            assert got["out_len"][b] == 0 and got["status"][b] != O.OK, names[b]
            if ix["tail"][b] != O.OK:
                assert got["status"][b] == ix["tail"][b]
    assert S.same_index(got["index"], X.build_index(S.after(streams, got)))
    assert got["result"][3] == written >= 10 and len(set(got["status"])) >= 3, (written, set(got["status"]))


def test_unsound_indexes_get_the_models_verdicts(named):
    names, streams, ix = named
    rng = np.random.default_rng(5)
    html = read_testdata("html")
    reqs3 = middle_splices(ix, len(streams))
    srcs = [html[b:b + r[2]] for b, r in enumerate(reqs3)]
    reqs = [r[:2] for r in reqs3]
    sound = S.splice_plan(streams, ix, reqs, srcs, 4096)
    refused = kept = 0
    for bad in S.unsound_indexes(ix, streams, rng):
        ms = 3 * len(streams)
        got = S.splice_plan(streams, bad, reqs, srcs, 4096, max_slots=ms, stage_cap=1 << 24)
        ne = min(len(bad["start"]), len(bad["pos"]))
        assert len(got["index"]["start"]) == len(got["index"]["pos"]) <= ne + ms          # the new arrays stay inside nentries + max_slots
        assert got["index"]["first"][-1] == len(got["index"]["start"]) and got["index"]["first"] == sorted(got["index"]["first"])
        for b, s in enumerate(streams):
            if got["streams"][b] is None:
                assert got["out_len"][b] == 0
                refused += got["status"][b] != sound["status"][b]
            else:                                                       # whatever passed the checks keeps the bytes around its hole
                p0, p1 = got["hole"][b]
                assert p0 <= p1 <= len(s) and got["streams"][b][:p0] == s[:p0] and got["streams"][b].endswith(s[p1:])
                assert got["out_len"][b] == len(got["streams"][b]) <= got["out_bound"][b]
                kept += 1
    assert refused > 40 and kept > 20, (refused, kept)
    # a stale index: that of other bytes with the same shape
    a, b2 = K.stream_of(html[:9000], 4096), K.stream_of(html[500:9500][::-1], 4096)
    stale = S.splice_plan([b2], X.build_index([a]), [(100, 5000)], [b"abc"], 4096)
    fresh = S.splice_plan([b2], X.build_index([b2]), [(100, 5000)], [b"abc"], 4096)
    assert stale["status"] == [O.OK if X.build_index([a])["pos"] == X.build_index([b2])["pos"] else O.ERR_BAD_ARG] and fresh["status"] == [O.OK]


# ---- the planning header on the CPU, under sanitizers ------------------------------------------------------------------------------------------
def test_planning_header_under_sanitizers_matches_the_model(named, tmp_path):
    names, streams, ix = named
    html = read_testdata("html") * 5
    foreign = [c[0] for c in S.foreign_streams(html).values()]
    cb0 = 1000
    shaped = [K.stream_of(html[5:5 + n], cb0) if n else b"" for n, _, _, _ in S.named_cases(cb0).values()]
    streams = streams + foreign + shaped
    ix = X.build_index(streams)
    ns = len(streams)
    rng = np.random.default_rng(11)
    mid = middle_splices(ix, ns)
    shapes = list(S.named_cases(cb0).values())
    # around the middle; the named splices on the named shapes (anything at all on the rest); inserts at the end; everything deleted; nothing;
    # lengths past 4 GiB and at the top of 64 bits
    lists = [mid,
             [(0, 0, 0)] * (ns - len(shaped)) + [(off, dele, ins) for _, off, dele, ins in shapes],
             [(int(rng.integers(0, t + 2)), int(rng.integers(0, t + 2)), int(rng.integers(0, 200000))) for t in ix["total"]],
             [(t, 0, 1) for t in ix["total"]], [(0, t, 0) for t in ix["total"]], [(0, 0, 0)] * ns,
             [(t // 2, 0, (1 << 32) + 5 + b) for b, t in enumerate(ix["total"])], [(1, 1, S.U64 - b) for b in range(ns)],
             [(S.U64 - b, 2 + b, 0) for b in range(ns)]]
    cases = [(ix, cb, ln) for cb in (1, 1000, 4096, 65536) for ln in lists]
    nsound = len(cases)
    cases += [(bad, cb, lists[0]) for bad in S.unsound_indexes(ix, streams, rng) for cb in (1000, 65536)]
    # streams past 4 GiB, as numbers: two rows around a hole past 4 GiB with both edges; the same rows wholly deleted; an insert on the second
    # row's boundary; a skippable chunk at the first row, at the second; the second header inside the first chunk; a position at the end; an
    # insert past 4 GiB, at one byte per chunk; a new length that wraps; an insert at the end of a stream without rows; an edge above 65536 bytes
    G = 1 << 32
    base = dict(n=3 * G, off=5 * G + 100, ins=5000, cb=65536, total=5 * G + 70000 + 9000, tail=0, rows=2,
                start0=5 * G, pos0=2 * G, kind0=0, size0=4 + 65536, dec0=65536, start1=5 * G + 65536, pos1=2 * G + 8 + 65536 + 77, kind1=0, size1=4 + 3000,
                dec1=70000 + 9000 - 65536)
    base["del"] = 65536 + 1000 - 100
    numeric = [base, {**base, "off": 5 * G, "del": 70000 + 9000}, {**base, "off": 5 * G + 65536, "del": 0}, {**base, "kind0": 1}, {**base, "kind1": 1},
               {**base, "pos1": base["pos0"] + 100}, {**base, "pos1": base["n"]}, {**base, "ins": 5 * G + 3}, {**base, "cb": 1, "ins": 2 * G + 1},
               {**base, "ins": S.U64 - 5 * G}, {**base, "rows": 0, "total": 0, "n": 0, "off": 0, "del": 0, "ins": G + 1},
               {**base, "dec0": 65537, "size0": 65541, "start1": 5 * G + 65537, "dec1": 70000 + 9000 - 65537}, {**base, "tail": O.ERR_CRC_MISMATCH},
               {**base, "dec1": base["dec1"] - 1}, {**base, "rows": 1}]
    path = str(tmp_path / "cases.bin")
    S.write_cases(path, streams, cases, numeric)
    exe = str(tmp_path / "frame_splice_plan_check")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host",
                    "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "abi", "frame_splice_plan_check.hip"), "-o", exe,
                    "-Wl,-rpath,/opt/rocm/lib"], check=True)
    env = {**os.environ, "ASAN_OPTIONS": "detect_leaks=1:abort_on_error=0", "UBSAN_OPTIONS": "print_stacktrace=1:halt_on_error=1"}
    run = subprocess.run([exe, path], capture_output=True, text=True, env=env)
    assert run.returncode == 0 and run.stderr == "", run.stderr[-3000:]      # the sanitizers are silent
    lines = run.stdout.splitlines()
    assert len(lines) == ns * len(cases) + len(numeric)
    at = passed = refused = 0
    for c, (index, cb, ln) in enumerate(cases):
        for b, w in enumerate(S.plan_lines(index, streams, ln, cb)):
            assert lines[at] == w, (c, b, cb, ln[b])
            unsound = c >= nsound
            passed += unsound and w.startswith("0 1 ")
            refused += unsound and not w.startswith("0 ")
            at += 1
    assert passed > 50 and refused > 200, (passed, refused)            # both outcomes, on the unsound indexes
    want = [S.numeric_line(c) for c in numeric]
    assert lines[at:] == want
    # the numbers themselves: the hole past 4 GiB with both edges, its region and its pieces; the same rows wholly deleted: nothing staged
    f = [int(v) for v in want[0].split("|")[0].split()]
    assert f[:9] == [0, 1, 0, 1, 1, 100, 70000 + 9000 - 65536 - 1000, 65536, base["dec1"]] and f[13:15] == [2 * G, base["pos1"] + 4 + base["size1"]]
    assert f[16] == 100 + 5000 + f[6] and f[17] == (f[16] + 65535) // 65536 and f[18] == f[7] + f[8] + f[16]
    assert f[19] == 3 * G - (f[14] - f[13]) + 8 * f[17] + f[16]
    w1 = [int(v) for v in want[1].split("|")[0].split()]
    assert w1[:5] == [0, 1, 0, 0, 0] and w1[16:19] == [5000, 1, 5000] and w1[11:13] == [0, 2]
    w2 = [int(v) for v in want[2].split("|")[0].split()]
    assert w2[:5] == [0, 1, 0, 0, 0] and w2[11:15] == [1, 1, base["pos1"], base["pos1"]]
    for i in (3, 4, 5, 6, 9, 11, 13, 14):
        assert want[i].split()[0] == str(O.ERR_BAD_ARG), i
    assert int(want[7].split("|")[0].split()[17]) == (5 * G + 3 + f[5] + f[6] + 65535) // 65536
    assert int(want[8].split("|")[0].split()[17]) == 2 * G + 1 + f[5] + f[6]
    assert want[10].split()[:3] == ["0", "1", "1"] and want[12].split()[0] == str(O.ERR_CRC_MISMATCH)

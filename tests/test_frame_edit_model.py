"""snp_frame_edit_indexed_batch (libsnappier_hip_frame_edit.so) without a GPU: the declarations and their C# binding, the workspace arithmetic,
argument rejection; the Python model of the contract (frame_edit_model.py) checked against the oracle's frame decode, the splice's model (one
edit per stream: every returned field), the index model and the chunked encoder's model over the directed scripts at the seam chunk sizes and
both hash variants; verdicts; and the planning header (csrc/frame_edit_device.h over fs_plan) itself, compiled for the CPU under
AddressSanitizer and UBSan into a stand-alone program (tests/abi/frame_edit_plan_check.hip) and run over the same cases, over indexes and edit
lists filled with anything at all and over streams past 4 GiB given as numbers."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import frame_chunked_model as K
import frame_edit_model as E
import frame_index_model as X
import frame_splice_model as S
import oracle as O
from conftest import ROOT, read_testdata

NAMES = ["snp_frame_edit_indexed_batch", "snp_frame_edit_indexed_workspace"]


def _lib():
    from snappier_amd import _native as N
    return N.frame_edit_lib()


# ---- the surface -----------------------------------------------------------------------------------------------------------------------------
def test_header_and_binding_declare_the_new_functions():
    from snappier_amd import _native as N
    declared = N.frame_edit_declared_symbols()
    assert sorted(declared) == NAMES
    others = set(N.declared_symbols())
    for name in ("buffers", "buffers_decompress", "frame_buffers", "layout", "frame_range", "frame_index", "frame_chunked", "frame_update",
                 "frame_append", "frame_splice", "frame_rechunk", "frame_compose", "frame_digest", "frame_diff", "frame_find"):
        others |= set(getattr(N, name + "_declared_symbols")())
    assert not set(declared) & others                                  # the other headers' surfaces are left as they are
    lib = _lib()
    assert lib.snp_frame_edit_indexed_batch.restype is C.c_int and len(lib.snp_frame_edit_indexed_batch.argtypes) == 35
    assert lib.snp_frame_edit_indexed_workspace.restype is C.c_uint64 and len(lib.snp_frame_edit_indexed_workspace.argtypes) == 5
    from snappier_amd import batch as SB
    assert all(callable(getattr(SB.BlockCodec, m)) for m in ("frame_edit_indexed", "frame_edit_to_memory", "frame_replace_streams"))


def test_extension_library_exports_exactly_its_header():
    from layouts import exported
    from snappier_amd import _native as N

    ext = exported(N.FRAME_EDIT_PATH)
    assert ext == set(NAMES)
    for other in (N.PRODUCT_PATH, N.FRAME_SPLICE_PATH, N.FRAME_COMPOSE_PATH, N.FRAME_FIND_PATH, N.FRAME_RECHUNK_PATH):
        assert not exported(other) & ext


def test_workspace_is_host_arithmetic():
    ws = _lib().snp_frame_edit_indexed_workspace
    assert ws(0, 7, 10, 1000, 4096) == 0                                # nothing when there is no stream
    assert ws(5, 7, 10, 1000, 0) == 0 and ws(5, 7, 10, 1000, 65537) == 0    # ... or no chunk size the call takes
    for ns in (1, 255, 300000):
        for ne in (0, 1, 1025, 300000):
            for ms in (0, 1, 33000):
                for sc in (0, 70000, 1 << 33):
                    for cb in (1, 4096, 65536):
                        w = ws(ns, ne, ms, sc, cb)
                        stride = K.stride(cb)
                        assert w % 256 == 0
                        # the staging, the compressed staging and the slot table; per edit 31 words of 8 bytes, 8 of 4 and two decode rows of
                        # 41; per stream 17 words of 8 bytes and one of 4
                        assert w >= sc + ms * (stride + 44) + ne * (248 + 32 + 82) + ns * 140
                        assert w <= sc + 256 + ms * (stride + 44) + ne * 362 + ns * 140 + 90 * 256 + (ns + ne + ms) // 50
                        assert ws(ns + 1, ne, ms, sc, cb) >= w and ws(ns, ne + 1, ms, sc, cb) >= w and ws(ns, ne, ms + 1, sc, cb) >= w
    assert ws(0x7FFFFFFF, 0x7FFFFFFF, 0xFFFFFFFF, 1 << 40, 65536) > 0xFFFFFFFF * 76496 + (1 << 40)      # (64-bit arithmetic)


def test_batch_call_rejects_bad_arguments_without_a_device():
    call = _lib().snp_frame_edit_indexed_batch
    fake = C.c_void_p(64)                                               # (never dereferenced: the arguments are refused first)
    # ctx; in, in_off, in_len; nstreams; five index arrays; nentries; src, ed_first, ed_off, ed_del, ed_ins, src_off; nedits, chunk_bytes,
    # max_slots, stage_cap; out, out_off, out_cap, out_len, status, ed_status; five new index arrays; out_bound; d_work, d_result
    def args(ctx=fake, ins=(fake,) * 3, ns=1, idx=(fake,) * 5, ne=8, eds=(fake,) * 6, nedits=3, cb=4096, ms=0, sc=0, outs=(fake,) * 6, new=(fake,) * 5,
             bound=None, work=fake, result=fake):
        return (ctx, *ins, ns, *idx, ne, *eds, nedits, cb, ms, sc, *outs, *new, bound, work, result)

    assert call(*args(ctx=None)) == O.ERR_BAD_ARG
    assert call(*args(result=None)) == O.ERR_BAD_ARG
    assert call(*args(ns=0, result=None)) == O.ERR_BAD_ARG             # an empty call still needs d_result
    assert call(*args(cb=0)) == O.ERR_BAD_ARG and call(*args(cb=65537)) == O.ERR_BAD_ARG
    assert call(*args(ns=0, cb=0)) == O.ERR_BAD_ARG                    # ... also when there is no stream
    assert call(*args(ns=1 << 31)) == O.ERR_BAD_ARG and call(*args(nedits=1 << 31)) == O.ERR_BAD_ARG
    assert call(*args(work=None)) == O.ERR_BAD_ARG
    for group, n in (("ins", 3), ("eds", 6), ("outs", 6)):
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
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "snappier_hip_frame_edit.h")).read(), flags=re.S)
    protos = {}
    for m in re.finditer(r"([A-Za-z_][A-Za-z0-9_ ]*?[\s\*]+)(snp_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", text):
        params = [re.match(r"(.*?[\s\*])([A-Za-z_][A-Za-z0-9_]*)$", q.strip()).group(1) for q in m.group(3).split(",") if q.strip() not in ("", "void")]
        protos[m.group(2)] = (T.c_class(m.group(1)), [T.c_class(q) for q in params])
    cs = re.sub(r"//.*", "", open(os.path.join(ROOT, "csharp", "Snappier.Gpu", "NativeMethodsFrameEdit.cs")).read())
    assert 'const string Lib = "snappier_hip_frame_edit"' in cs
    imps = {}
    for m in re.finditer(r"\[DllImport\(Lib, CallingConvention = Cc\)\]\s*internal static extern ([A-Za-z\*]+) (snp_[a-z0-9_]+)\(([^)]*)\);", cs):
        params = [re.match(r"(.*?)\s+([A-Za-z_][A-Za-z0-9_]*)$", q.strip()).group(1) for q in m.group(3).split(",") if q.strip()]
        imps[m.group(2)] = (T.cs_class(m.group(1)), [T.cs_class(q) for q in params])
    assert set(protos) == set(imps) == set(NAMES)
    for name, (ret, params) in protos.items():
        cret, cparams = imps[name]
        assert T.compatible(ret, cret), (name, ret, cret)
        assert len(params) == len(cparams) and all(T.compatible(a, b) for a, b in zip(params, cparams)), (name, params, cparams)
    assert len(protos["snp_frame_edit_indexed_batch"][1]) == 35 and len(protos["snp_frame_edit_indexed_workspace"][1]) == 5
    proj = open(os.path.join(ROOT, "csharp", "Snappier.Gpu", "Snappier.Gpu.csproj")).read()
    assert 'Include="../../snappier_amd/libsnappier_hip_frame_edit.so"' in proj


# ---- the model -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cb", S.CHUNK_SIZES)
def test_directed_scripts_decode_to_the_edits_applied_from_last_to_first_with_the_index_of_the_new_streams(cb):
    html = read_testdata("html") * 5
    for variant in (O.HASH_CRC32C, O.HASH_MUL):
        names, raws, streams, scripts = E.scripts_batch(html, cb, variant)
        assert all(len(K.chunks_of(a, cb, variant)) <= 5 for a in raws)
        ix = X.build_index(streams)
        first, edits, srcs = E.flat(scripts)
        got = E.edit_plan(streams, ix, first, edits, srcs, cb, variant=variant)
        assert set(got["ed_status"]) == {O.OK}
        for b, name in enumerate(names):
            assert got["status"][b] == O.OK, name
            new = got["streams"][b]
            if not any(d or x for _, d, x in scripts[b]):               # no edit, or skipped ones only: not named
                assert new is None and got["out_len"][b] == 0 and got["out_bound"][b] == 0, name
                continue
            assert O.frame_decode(new) == E.applied(raws[b], scripts[b]), (cb, name)
            assert got["out_len"][b] == len(new) <= got["out_bound"][b]
            at = 0
            for p0, p1 in got["holes"][b]:                              # the holes in order; everything outside them is a copy
                assert at <= p0 <= p1 <= len(streams[b])
                assert streams[b][at:p0] in new
                at = p1
        after = [n if n is not None else s for s, n in zip(streams, got["streams"])]
        assert S.same_index(got["index"], X.build_index(after)), cb
        slots, stage = E.needs(streams, ix, first, edits, srcs, cb)
        assert got["result"][0] == slots and got["result"][2] == stage and got["result"][1] == sum(got["out_len"])
        assert E.edit_plan(streams, ix, first, edits, srcs, cb, max_slots=slots, stage_cap=stage, variant=variant) == got
        # what the groups are: two edits inside one chunk are one hole; the chain is one; separate chunks are three
        if cb >= 63:
            holes = dict(zip(names, got["holes"]))
            assert len(holes["two_edits_inside_one_chunk"]) == 1 and len(holes["chain_each_tail_row_is_the_next_head_row"]) == 1
            assert len(holes["separate_chunks_untouched_between"]) == 3 and len(holes["two_inserts_at_one_boundary"]) == 2
            assert len(holes["two_inserts_at_one_offset_mid_chunk"]) == 1 and len(holes["skipped_edits_between_linked_ones"]) == 1
            # a row that two edits touch is staged once: chunk 1 whole, and the region
            b = names.index("two_edits_inside_one_chunk")
            one = E.needs([streams[b]], X.build_index([streams[b]]), *E.flat([scripts[b]]), cb)
            assert one[1] == cb + cb - (cb // 8 + 1) + 5 + cb + 2


@pytest.mark.parametrize("cb", S.CHUNK_SIZES)
def test_one_edit_per_stream_equals_the_splice_model_in_every_returned_field(cb):
    html = read_testdata("html") * 5
    for variant in (O.HASH_CRC32C, O.HASH_MUL):
        cases = S.named_cases(cb)
        raws = [html[7 + i:7 + i + n] for i, (n, _, _, _) in enumerate(cases.values())]
        streams = [K.stream_of(a, cb, variant) if a else b"" for a in raws]
        reqs = [(off, dele) for _, off, dele, _ in cases.values()]
        srcs = [html[3001 + 5 * i:3001 + 5 * i + ins] for i, (_, _, _, ins) in enumerate(cases.values())]
        ix = X.build_index(streams)
        for bounds in (dict(), dict(max_slots=7, stage_cap=3 * cb + 50), dict(caps=[len(s) + 20 for s in streams])):
            want = S.splice_plan(streams, ix, reqs, srcs, cb, variant=variant, **bounds)
            got = E.edit_plan(streams, ix, list(range(len(streams) + 1)), reqs, srcs, cb, variant=variant, **bounds)
            for key in want:
                assert got[key] == want[key], (cb, key)
            assert got["ed_status"] == [O.OK] * len(streams)
    # ... also where the splice refuses: the verdict is the edit's
    streams = [K.stream_of(html[:2500], 1000)] * 3
    ix = {**X.build_index(streams), "tail": [0, O.ERR_CRC_MISMATCH, 77]}
    reqs, srcs = [(2500, 1), (0, 1), (0, 1)], [b"x"] * 3
    want = S.splice_plan(streams, ix, reqs, srcs, 1000)
    got = E.edit_plan(streams, ix, [0, 1, 2, 3], reqs, srcs, 1000)
    assert got["status"] == got["ed_status"] == want["status"] == [O.ERR_BAD_ARG, O.ERR_CRC_MISMATCH, O.ERR_BAD_ARG]
    assert all(got[key] == want[key] for key in want)


@pytest.mark.parametrize("cb", S.CHUNK_SIZES)
def test_edits_on_multiples_of_chunk_bytes_give_the_chunked_encoders_output(cb):
    html = read_testdata("html") * 5
    a = html[11:11 + 4 * cb + (cb + 1) // 2]
    n = len(a)

    def s(k, at=9000):
        return html[at:at + k]

    scripts = [[(0, cb, s(2 * cb)), (2 * cb, cb, s(0)), (3 * cb, 0, s(cb, 100))],
               [(cb, 0, s(cb)), (cb, cb, s(0)), (4 * cb, n - 4 * cb, s(cb + 5, 7))],
               [(0, 0, s(cb)), (0, 0, s(cb, 50)), (cb, 2 * cb, s(3 * cb, 99))],
               [(0, 2 * cb, s(0)), (2 * cb, n - 2 * cb, s(0))]]
    for variant in (O.HASH_CRC32C, O.HASH_MUL):
        streams = [K.stream_of(a, cb, variant)] * len(scripts)
        got = E.edit_plan(streams, X.build_index(streams), *E.flat(scripts), cb, variant=variant)
        for b, sc in enumerate(scripts):
            assert got["status"][b] == O.OK and got["streams"][b] == K.stream_of(E.applied(a, sc), cb, variant), (cb, b)
        assert got["result"][2] == sum(len(x) for sc in scripts for _, _, x in sc)       # no edge: only the inserted bytes are staged


def test_verdicts_of_edits_and_of_streams():
    html = read_testdata("html")
    cb = 1000
    s = K.stream_of(html[:3500], cb)
    x = html[9000:9010]
    B = O.ERR_BAD_ARG
    scripts = [[(100, 10, x), (50, 5, x)], [(100, 10, x), (109, 5, x)], [(100, 10, x), (110, 5, x)], [(100, 10, x), (3490, 11, x)],
               [(3500, 0, x), (3500, 0, x)], [(3501, 0, x)], [(200, 0, x), (100, 0, b""), (300, 1, b"")], [(S.U64, 2, x), (5, 1, x)]]
    got = E.edit_plan([s] * len(scripts), X.build_index([s] * len(scripts)), *E.flat(scripts), cb)
    assert got["status"] == [B, B, O.OK, B, O.OK, B, O.OK, B]
    assert got["ed_status"] == [0, B, 0, B, 0, 0, 0, B, 0, 0, B, 0, 0, 0, B, 0]       # (behind an edit whose end wraps, the order is not checked)
    # the running length wraps at the second edit, not at the first
    huge = {**X.build_index([s]), "total": [S.U64 - 5]}
    got = E.edit_plan([s], huge, [0, 2], [(0, 0), (1, 0)], [b"abc", b"abcd"], cb)
    assert got["ed_status"] == [O.OK, B] and got["status"] == [B]
    # a malformed ed_first: clamped; from the first list that runs backwards on, every stream is refused
    edits, srcs = [(10 * i, 3) for i in range(8)], [html[i:i + 5] for i in range(8)]
    ix = X.build_index([s] * 4)
    for first, want in (([0, 2, 4, 6, 8], [0] * 4), ([0, 4, 2, 6, 8], [0, B, B, B]), ([2, 4, 4, 99, 1 << 63], [0] * 4), ([0, 2, 4, 9, 7], [0, 0, 0, B]),
                        ([5, 0, 0, 0, 0], [B] * 4)):
        assert E.edit_plan([s] * 4, ix, first, edits, srcs, cb)["status"] == want, first
    # hole order with an unsound index: two rows swapped in pos -- the second group's hole lies before the first's
    one = X.build_index([s])
    swapped = {**one, "pos": [one["pos"][0], one["pos"][2], one["pos"][1], one["pos"][3]]}
    got = E.edit_plan([s], swapped, [0, 2], [(1000, 1000), (2000, 1000)], [b"", b""], cb)
    assert got["ed_status"] == [O.OK, B] and got["status"] == [B]


# ---- the planning header on the CPU, under sanitizers ------------------------------------------------------------------------------------------
def test_planning_header_under_sanitizers_matches_the_model(tmp_path):
    html = read_testdata("html") * 5
    named = list(X.named_streams().values())
    foreign = [c[0] for c in S.foreign_streams(html).values()]
    cb0 = 1000
    _, _, shaped, scripts = E.scripts_batch(html, cb0)
    streams = named + foreign + shaped
    ix = X.build_index(streams)
    ns = len(streams)
    rng = np.random.default_rng(11)

    def around_the_middle(b):
        t = ix["total"][b]
        a = t // 2
        d = min(t - a, 300 + 7 * b)
        c = min(a + d + 40, t)
        return [(a, d, 100 + b), (c, min(t - c, 5000), 3), (t, 0, 9)]

    def anything(b):
        t = ix["total"][b]
        return sorted((int(rng.integers(0, t + 2)), int(rng.integers(0, 200)), int(rng.integers(0, 2000))) for _ in range(int(rng.integers(0, 6))))

    def flat3(lists):
        first, edits3 = [0], []
        for ln in lists:
            edits3 += ln
            first.append(len(edits3))
        return first, edits3

    directed = [[(0, 0, 0)] for _ in range(ns - len(shaped))] + [[(o, d, len(x)) for o, d, x in sc] for sc in scripts]
    lists = [flat3([around_the_middle(b) for b in range(ns)]), flat3(directed), flat3([anything(b) for b in range(ns)]),
             flat3([[(t // 3, 0, (1 << 32) + 5), (t // 3, 1, S.U64 - (1 << 32))] for t in ix["total"]]),                # the inserted bytes wrap
             flat3([[(S.U64 - b, 2 + b, 0), (1, 1, 1)] for b in range(ns)])]
    cases = [(ix, cb, first, edits3) for cb in (1, 1000, 4096, 65536) for first, edits3 in lists]
    # ed_first filled with anything at all
    first, edits3 = lists[0]
    cases += [(ix, 1000, [int(v) for v in rng.integers(0, len(edits3) + 3, ns + 1)], edits3), (ix, 1000, list(reversed(first)), edits3),
              (ix, 1000, [S.U64 - v for v in first], edits3), (ix, 1000, first[:ns // 2] + [3] + first[ns // 2 + 1:], edits3)]
    nsound = len(cases)
    cases += [(bad, cb, *lists[0]) for bad in S.unsound_indexes(ix, streams, rng) for cb in (1000, 65536)]
    # streams past 4 GiB, as numbers: two rows behind 5 * 2^32 decoded bytes and 2 * 2^32 stream bytes; three edits in the first row and across
    # into the second (one group); the same with the second edit out of order; an insert past 4 GiB between two others (the running sums)
    G = 1 << 32
    base = dict(n=3 * G, cb=65536, total=5 * G + 70000 + 9000, tail=0, rows=2, start0=5 * G, pos0=2 * G, kind0=0, size0=4 + 65536, dec0=65536,
                start1=5 * G + 65536, pos1=2 * G + 8 + 65536 + 77, kind1=0, size1=4 + 3000, dec1=70000 + 9000 - 65536, nedits=3,
                off0=5 * G + 100, del0=50, ins0=7, off1=5 * G + 900, del1=0, ins1=5000, off2=5 * G + 65000, del2=1000, ins2=0)
    numeric = [base, {**base, "off1": 5 * G + 120}, {**base, "ins1": 5 * G + 3}, {**base, "ins0": S.U64 - 7 * G, "ins1": G, "ins2": 5 * G},
               {**base, "off2": 5 * G + 65536, "del2": 0, "ins2": 1}, {**base, "kind1": 1}, {**base, "nedits": 1, "del0": 0, "ins0": 0}]
    path = str(tmp_path / "cases.bin")
    E.write_cases(path, streams, cases, numeric)
    exe = str(tmp_path / "frame_edit_plan_check")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host",
                    "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "abi", "frame_edit_plan_check.hip"), "-o", exe,
                    "-Wl,-rpath,/opt/rocm/lib"], check=True)
    env = {**os.environ, "ASAN_OPTIONS": "detect_leaks=1:abort_on_error=0", "UBSAN_OPTIONS": "print_stacktrace=1:halt_on_error=1"}
    run = subprocess.run([exe, path], capture_output=True, text=True, env=env)
    assert run.returncode == 0 and run.stderr == "", run.stderr[-3000:]      # the sanitizers are silent
    lines = run.stdout.splitlines()
    want = []
    marks = []
    for index, cb, first, edits3 in cases:
        marks.append(len(want))
        want += E.check_lines(index, streams, first, edits3, cb)
    marks.append(len(want))
    for c in numeric:
        want += E.numeric_lines(c)
    assert len(lines) == len(want)
    for i, (g, w) in enumerate(zip(lines, want)):
        assert g == w, (i, g, w)
    sound = [w.split() for w in want[:marks[nsound]] if w.startswith("E")]
    unsound = [w.split() for w in want[marks[nsound]:marks[-1]] if w.startswith("E")]
    assert sum(1 for f in sound if f[2] == "0" and f[3] == "1") > 50 and sum(1 for f in sound if f[2] != "0") > 50     # linked; refused
    assert sum(1 for f in unsound if f[2] == "0") > 100 and sum(1 for f in unsound if f[2] != "0") > 200
    assert sum(1 for w in want if w.startswith("S") and w.endswith(" 0")) > ns                                         # lists that run backwards
    # the numbers themselves: one group across both rows past 4 GiB; the second edit out of order; the inserted bytes wrap at the third edit
    num = [[ln.split() for ln in E.numeric_lines(c)] for c in numeric]
    assert [f[2:4] for f in num[0][1:]] == [["0", "0"], ["0", "1"], ["0", "1"]] and num[0][1][4] == "100" and num[0][3][5] == str(70000 + 9000 - 66000)
    assert [f[2] for f in num[1][1:]] == ["0", str(O.ERR_BAD_ARG), "0"]
    assert [f[2] for f in num[2][1:]] == ["0", "0", "0"] and [f[2] for f in num[3][1:]] == ["0", "0", str(O.ERR_BAD_ARG)]
    assert [f[2:4] for f in num[4][1:]] == [["0", "0"], ["0", "1"], ["0", "0"]]          # an insert on the second row's boundary: a group of its own
    assert num[5][3][2] == str(O.ERR_BAD_ARG) and len(num[6]) == 1

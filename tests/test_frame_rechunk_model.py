"""snp_frame_rechunk_indexed_batch (libsnappier_hip_frame_rechunk.so) without a GPU: the declarations and their C# binding, the workspace
arithmetic, argument rejection; the Python model of the contract (frame_rechunk_model.py) checked against the oracle's frame decode, the index
model and the chunked encoder's model: streams written at the seam chunk sizes with both hash variants, fragmented through the splice, update
and append models and rechunked -- byte for byte the chunked encoder's output; a change of the chunk size and back; canonical streams left
alone; foreign streams with and without SNP_RECHUNK_REWRITE_ALL; the length cases; corruption in a dirty and in a kept chunk; admission by each
bound and out_cap; every rejection; unsound indexes; and the planning header (csrc/frame_rechunk_device.h) itself, compiled for the CPU under
AddressSanitizer and UBSan into a stand-alone program (tests/abi/frame_rechunk_plan_check.hip) and run over the same cases, over indexes filled
with anything at all and over streams past 4 GiB given as numbers."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import frame_append_model as A
import frame_buffers_model as M
import frame_chunked_model as K
import frame_index_model as X
import frame_range_model as R
import frame_rechunk_model as RC
import frame_splice_model as S
import frame_update_model as U
import oracle as O
from conftest import ROOT, read_testdata

NAMES = ["snp_frame_rechunk_indexed_batch", "snp_frame_rechunk_indexed_workspace"]
ALL = RC.REWRITE_ALL


def _lib():
    from snappier_amd import _native as N
    return N.frame_rechunk_lib()


# ---- the surface -----------------------------------------------------------------------------------------------------------------------------
def test_header_and_binding_declare_the_new_functions():
    from snappier_amd import _native as N
    declared = N.frame_rechunk_declared_symbols()
    assert sorted(declared) == NAMES
    others = set(N.declared_symbols()) | set(N.buffers_declared_symbols()) | set(N.buffers_decompress_declared_symbols()) | \
        set(N.frame_buffers_declared_symbols()) | set(N.layout_declared_symbols()) | set(N.frame_range_declared_symbols()) | \
        set(N.frame_index_declared_symbols()) | set(N.frame_chunked_declared_symbols()) | set(N.frame_update_declared_symbols()) | \
        set(N.frame_append_declared_symbols()) | set(N.frame_splice_declared_symbols())
    assert not set(declared) & others                                  # the other headers' surfaces are left as they are
    lib = _lib()
    assert lib.snp_frame_rechunk_indexed_batch.restype is C.c_int and len(lib.snp_frame_rechunk_indexed_batch.argtypes) == 29
    assert lib.snp_frame_rechunk_indexed_workspace.restype is C.c_uint64 and len(lib.snp_frame_rechunk_indexed_workspace.argtypes) == 5
    header = open(os.path.join(ROOT, "include", "snappier_hip_frame_rechunk.h")).read()
    assert re.search(r"#define SNP_RECHUNK_REWRITE_ALL 1u\b", header) and N.RECHUNK_REWRITE_ALL == ALL == 1
    from snappier_amd import batch as SB
    assert callable(SB.BlockCodec.frame_rechunk_indexed) and callable(SB.BlockCodec.frame_rechunk_to_memory)


def test_extension_library_exports_exactly_its_header():
    from layouts import exported
    from snappier_amd import _native as N

    ext = exported(N.FRAME_RECHUNK_PATH)
    assert ext == set(NAMES)
    for other in (N.PRODUCT_PATH, N.BUFFERS_PATH, N.BUFFERS_DECOMPRESS_PATH, N.FRAME_BUFFERS_PATH, N.LAYOUT_PATH, N.FRAME_RANGE_PATH, N.FRAME_INDEX_PATH,
                  N.FRAME_CHUNKED_PATH, N.FRAME_UPDATE_PATH, N.FRAME_APPEND_PATH, N.FRAME_SPLICE_PATH):
        assert not exported(other) & ext


def test_workspace_is_host_arithmetic():
    ws = _lib().snp_frame_rechunk_indexed_workspace
    assert ws(0, 10, 1000, 4096, 50) == 0                               # nothing when there is no stream
    assert ws(5, 10, 1000, 0, 50) == 0 and ws(5, 10, 1000, 65537, 50) == 0      # ... or no chunk size the call takes
    for ns in (1, 255, 1025, 300000):
        for ms in (0, 1, 33000):
            for sc in (0, 1, 70000, 1 << 33):
                for cb in (1, 64, 4096, 65536):
                    for me in (0, 7, 100000):
                        w = ws(ns, ms, sc, cb, me)
                        stride = K.stride(cb)
                        assert w % 256 == 0
                        # the staging, the compressed staging, the slot table (32) and the decode table (41 + 8) with the size scan (8), the
                        # streams' words (13 + 6 of 8 bytes, 1 of 4), the new rows' (8 + 4 + 8)
                        assert w >= sc + ms * (stride + 89) + ns * 156 + me * 20
                        assert w <= sc + 256 + ms * (stride + 89) + ns * 156 + me * 20 + 60 * 256 + (ns + ms + me) // 50
                        assert ws(ns + 1, ms, sc, cb, me) >= w and ws(ns, ms + 1, sc, cb, me) >= w and ws(ns, ms, sc + 1, cb, me) >= w
                        assert ws(ns, ms, sc, cb, me + 1) >= w
    assert ws(0x7FFFFFFF, 0xFFFFFFFF, 1 << 40, 65536, 0xFFFFFFFF) > 0xFFFFFFFF * 76496 + (1 << 40)      # (64-bit arithmetic)


def test_batch_call_rejects_bad_arguments_without_a_device():
    call = _lib().snp_frame_rechunk_indexed_batch
    fake = C.c_void_p(64)                                               # (never dereferenced: the arguments are refused first)
    # ctx; in, in_off, in_len; nstreams; five index arrays; nentries; chunk_bytes, flags, max_slots, stage_cap, max_entries;
    # out, out_off, out_cap, out_len, status; five new index arrays; out_bound; d_work, d_result
    def args(ctx=fake, ins=(fake,) * 3, ns=1, idx=(fake,) * 5, ne=8, cb=4096, flags=0, ms=0, sc=0, me=8, outs=(fake,) * 5, new=(fake,) * 5,
             bound=None, work=fake, result=fake):
        return (ctx, *ins, ns, *idx, ne, cb, flags, ms, sc, me, *outs, *new, bound, work, result)

    assert call(*args(ctx=None)) == O.ERR_BAD_ARG
    assert call(*args(result=None)) == O.ERR_BAD_ARG
    assert call(*args(ns=0, result=None)) == O.ERR_BAD_ARG             # an empty call still needs d_result
    assert call(*args(cb=0)) == O.ERR_BAD_ARG and call(*args(cb=65537)) == O.ERR_BAD_ARG
    assert call(*args(ns=0, cb=0)) == O.ERR_BAD_ARG                    # ... also when there is no stream
    assert call(*args(flags=2)) == O.ERR_BAD_ARG and call(*args(flags=3)) == O.ERR_BAD_ARG and call(*args(flags=1 << 31)) == O.ERR_BAD_ARG
    assert call(*args(ns=1 << 31)) == O.ERR_BAD_ARG
    assert call(*args(work=None)) == O.ERR_BAD_ARG
    for group, n in (("ins", 3), ("outs", 5)):
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
        assert call(*args(new=tuple(a), ne=0, me=1)) == O.ERR_BAD_ARG   # no old rows, room for new ones


def test_csharp_binding_matches_the_extension_header():
    import test_csharp_signatures as T
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "snappier_hip_frame_rechunk.h")).read(), flags=re.S)
    protos = {}
    for m in re.finditer(r"([A-Za-z_][A-Za-z0-9_ ]*?[\s\*]+)(snp_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", text):
        params = [re.match(r"(.*?[\s\*])([A-Za-z_][A-Za-z0-9_]*)$", q.strip()).group(1) for q in m.group(3).split(",") if q.strip() not in ("", "void")]
        protos[m.group(2)] = (T.c_class(m.group(1)), [T.c_class(q) for q in params])
    cs = re.sub(r"//.*", "", open(os.path.join(ROOT, "csharp", "Snappier.Gpu", "NativeMethodsFrameRechunk.cs")).read())
    assert 'const string Lib = "snappier_hip_frame_rechunk"' in cs and "const uint RewriteAll = 1;" in cs
    imps = {}
    for m in re.finditer(r"\[DllImport\(Lib, CallingConvention = Cc\)\]\s*internal static extern ([A-Za-z\*]+) (snp_[a-z0-9_]+)\(([^)]*)\);", cs):
        params = [re.match(r"(.*?)\s+([A-Za-z_][A-Za-z0-9_]*)$", q.strip()).group(1) for q in m.group(3).split(",") if q.strip()]
        imps[m.group(2)] = (T.cs_class(m.group(1)), [T.cs_class(q) for q in params])
    assert set(protos) == set(imps) == set(NAMES)
    for name, (ret, params) in protos.items():
        cret, cparams = imps[name]
        assert T.compatible(ret, cret), (name, ret, cret)
        assert len(params) == len(cparams) and all(T.compatible(a, b) for a, b in zip(params, cparams)), (name, params, cparams)
    assert len(protos["snp_frame_rechunk_indexed_batch"][1]) == 29 and len(protos["snp_frame_rechunk_indexed_workspace"][1]) == 5
    proj = open(os.path.join(ROOT, "csharp", "Snappier.Gpu", "Snappier.Gpu.csproj")).read()
    assert 'Include="../../snappier_amd/libsnappier_hip_frame_rechunk.so"' in proj


# ---- the model against the oracle ----------------------------------------------------------------------------------------------------------------
def fragmented(html: bytes, cb: int, variant: int):
    """One stream per fragmenting edit, written at cb and edited through the splice model (the append at total through the append model), and
    one that the update model patched: -> (names, edited buffers, streams)."""
    n = 5 * cb + (cb + 1) // 2
    names, raws, streams = [], [], []
    for i, (name, edits) in enumerate(RC.fragmenting_edits(cb, n).items()):
        raw = html[13 + i:13 + i + n]
        s = K.stream_of(raw, cb, variant)
        for j, (off, dele, ins) in enumerate(edits):
            src = html[4001 + 3 * j:4001 + 3 * j + ins]
            if name == "append_at_total":
                got = A.append_plan([s], X.build_index([s]), [src], cb, variant=variant)
            else:
                got = S.splice_plan([s], X.build_index([s]), [(off, dele)], [src], cb, variant=variant)
            assert got["status"] == [O.OK]
            s, raw = got["streams"][0], S.edited(raw, off, dele, src)
        names.append(name)
        raws.append(raw)
        streams.append(s)
    raw = html[77:77 + n]
    s = K.stream_of(raw, cb, variant)
    src = html[9000:9000 + cb + 3]
    up = U.write_plan([s], X.build_index([s]), [(0, cb // 2, len(src))], [src], variant=variant)
    assert up["status"] == [O.OK]
    return names + ["updated"], raws + [S.edited(raw, cb // 2, len(src), src)], streams + [up["streams"][0]]


@pytest.mark.parametrize("cb", RC.CHUNK_SIZES)
def test_fragmented_streams_become_the_chunked_encoders_output(cb):
    html = read_testdata("html") * 5
    for variant in (O.HASH_CRC32C, O.HASH_MUL):
        names, raws, streams = fragmented(html, cb, variant)
        assert all(O.frame_decode(s) == a for s, a in zip(streams, raws))
        ix = X.build_index(streams)
        got = RC.rechunk_plan(streams, ix, cb, variant=variant)
        want = [K.stream_of(a, cb, variant) for a in raws]
        for b, name in enumerate(names):
            if streams[b] == want[b]:                                   # (one byte per chunk: no edit fragments; the update keeps the grid, and so do
                assert got["alone"][b] and got["streams"][b] is None and got["out_len"][b] == 0, (cb, name)     # a delete whose edges make one whole
                assert cb == 1 or name in ("updated", "delete_across_chunks", "append_at_total"), (cb, name)   # chunk and an append, which fills the tail)
                continue
            assert got["status"][b] == O.OK and got["streams"][b] == want[b], (cb, name)        # (b)
            assert got["out_len"][b] == len(want[b]) <= got["out_bound"][b]
        assert RC.same_index(got["index"], X.build_index(RC.after(streams, got))), cb
        assert got["result"][3] + got["result"][5] == len(streams) and got["result"][1] == sum(got["out_len"])
        ms, sc, me = RC.needs(streams, ix, cb)
        assert got["result"][0] == ms and got["result"][2] == sc and got["result"][4] == me
        assert RC.rechunk_plan(streams, ix, cb, max_slots=ms, stage_cap=sc, max_entries=me, variant=variant) == got
        # the edit near the end keeps a long clean prefix: the 5-byte chunk the split left and the short tail are one rebuilt piece, the rest is copied
        if cb > 1:
            end = names.index("edit_near_the_end")
            k = RC.plan(ix, end, len(streams[end]), cb, False, True, lambda pos, s=streams[end]: M.hop(s, pos))
            assert k["work"] and k["rebuilt"] == 1 and k["pieces"] - k["rebuilt"] == 5 and k["dirty"] == 2
        # another chunk size, at once: the encoder's output at that size; with the flag the same
        for cb2 in (cb + 1, max(cb // 2, 1)):
            if cb2 <= 65536:
                other = RC.rechunk_plan(streams, ix, cb2, variant=variant)
                assert RC.after(streams, other) == [K.stream_of(a, cb2, variant) for a in raws]
        assert RC.rechunk_plan(streams, ix, cb, ALL, variant=variant)["streams"] == want


def test_the_chunk_size_changed_and_back():
    html = read_testdata("html") * 8
    raws = [html[:300000], html[5:5 + 65536], html[9:9 + 65537], html[:4096], html[:1], b""]
    small = [K.stream_of(a, 4096) for a in raws]
    big = [K.stream_of(a, 65536) for a in raws]
    up = RC.rechunk_plan(small, X.build_index(small), 65536)
    assert RC.after(small, up) == big and up["status"] == [O.OK] * 6
    assert up["alone"] == [False, False, False, True, True, True]       # one chunk at most, on both grids
    assert all(k is None or len(k) == n for k, n in zip(up["streams"], up["out_len"]))
    assert RC.same_index(up["index"], X.build_index(big))
    down = RC.rechunk_plan(big, up["index"], 4096)
    assert RC.after(big, down) == small and RC.same_index(down["index"], X.build_index(small))
    # every row is dirty on the way up (no 4096-byte row is a 65536-byte piece) but the one-byte last row of the 65537-byte stream, which
    # starts on the 65536 grid and ends the stream
    assert up["result"][0] == sum(K.nchunks(len(a), 4096) for a in raws[:3]) - 1 and up["result"][2] == sum(len(a) for a in raws[:3]) - 1


def test_a_canonical_stream_is_left_alone_and_rewrite_all_writes_it_identically():
    html = read_testdata("html") * 3
    for cb in (64, 4096, 65536):
        raws = [html[:3 * cb + 5], html[:2 * cb], html[:1], b""]
        streams = [K.stream_of(a, cb) for a in raws]
        ix = X.build_index(streams)
        got = RC.rechunk_plan(streams, ix, cb)
        assert got["status"] == [O.OK] * 4 and got["alone"] == [True] * 4 and got["streams"] == [None] * 4 and got["out_len"] == [0] * 4
        assert got["out_bound"] == [0] * 4 and got["result"] == [0, 0, 0, 0, len(ix["start"]), 4] and RC.same_index(got["index"], ix)
        every = RC.rechunk_plan(streams, ix, cb, ALL)
        assert every["streams"] == streams and every["alone"] == [False] * 4 and every["result"][3] == 4 and every["result"][5] == 0
        assert RC.same_index(every["index"], ix)


def test_foreign_streams_with_and_without_rewrite_all():
    html = read_testdata("html")
    cases = RC.foreign_streams(html)
    streams, raws = [c[0] for c in cases.values()], [c[1] for c in cases.values()]
    assert all(O.frame_decode(s) == a for s, a in zip(streams, raws))
    ix = X.build_index(streams)
    for cb in (1, 300, 500, 1000, 65536):
        every = RC.rechunk_plan(streams, ix, cb, ALL)
        assert every["status"] == [O.OK] * len(streams) and every["streams"] == [K.stream_of(a, cb) for a in raws], cb      # (a)
        got = RC.rechunk_plan(streams, ix, cb)
        assert got["status"] == [O.OK] * len(streams), cb
        assert [n for n, x in zip(cases, got["alone"]) if x] == ["identifier_only"] + (["on_the_grid_uncompressed"] if cb == 500 else []), cb
        for name, new, a in zip(cases, RC.after(streams, got), raws):    # (c)
            assert O.frame_decode(new) == a, (cb, name)
            lens = RC.data_chunk_lengths(new)
            assert lens == [cb] * (len(a) // cb) + ([len(a) % cb] if len(a) % cb else []), (cb, name)
            assert new[:10] == M.STREAM_ID and len(R.walk(new)[0]) == K.nchunks(len(a), cb)
            assert sum(len(c) for c in [new[:10]] + [new[r[1] - 8:r[1] + r[2]] for r in R.walk(new)[0]]) == len(new)    # data chunks and nothing else
        assert RC.same_index(got["index"], X.build_index(RC.after(streams, got)))
    # on the 500-byte grid the foreign chunks are kept as they are: uncompressed ones stay uncompressed, which no encoder writes for html
    got = RC.rechunk_plan(streams, ix, 500)
    g = list(cases).index("on_the_grid_with_a_skippable_chunk")
    assert got["streams"][g] == streams[g].replace(M.chunk(0x80, b"note"), b"") != K.stream_of(raws[g], 500)
    assert got["result"][0] > 0 and got["out_bound"][g] == got["out_len"][g] == len(got["streams"][g])


def test_length_cases():
    html = read_testdata("html") * 2
    cb = 1000
    ch = M.data_chunk
    empty = RC.rechunk_plan([M.STREAM_ID, b""], X.build_index([M.STREAM_ID, b""]), cb)
    assert empty["status"] == [O.OK, O.OK] and empty["alone"] == [True, False] and empty["streams"] == [None, M.STREAM_ID]     # in_len == 0
    assert empty["out_len"] == [0, 10] and empty["out_bound"] == [0, 10] and empty["result"] == [0, 10, 0, 1, 0, 1]
    assert RC.rechunk_plan([M.STREAM_ID], X.build_index([M.STREAM_ID]), cb, ALL)["streams"] == [M.STREAM_ID]
    # a short last row that is kept (behind a dirty first row) and a last row longer than cb
    a, b, c = html[:700], html[700:1000], html[1000:1400]
    short = M.STREAM_ID + ch(a) + ch(b) + ch(c)
    long_ = M.STREAM_ID + ch(html[:1000]) + ch(html[1000:2700])
    got = RC.rechunk_plan([short, long_], X.build_index([short, long_]), cb)
    assert got["streams"] == [K.stream_of(html[:1400], cb), K.stream_of(html[:2700], cb)]
    assert got["streams"][0].endswith(ch(c)) and got["streams"][1].startswith(M.STREAM_ID + ch(html[:1000]))
    assert got["result"][0] == 3 and got["result"][2] == 1000 + 1700       # rows a and b for one slot; the long row for two
    assert got["out_bound"] == [10 + 8 + 1000 + len(ch(c)), 10 + len(ch(html[:1000])) + 16 + 1700]


def test_corruption_in_a_dirty_chunk_is_noticed_in_a_kept_chunk_copied_and_rewrite_all_is_the_scrub():
    html = read_testdata("html") * 2
    cb = 4096
    raw = html[:5 * cb]
    s0 = K.stream_of(raw, cb)
    sp = S.splice_plan([s0], X.build_index([s0]), [(cb + 100, 50)], [b""], cb)        # chunk 1 is short now, 2 .. 4 off the grid, chunk 0 clean
    s, raw = sp["streams"][0], S.edited(raw, cb + 100, 50, b"")
    rows = R.walk(s)[0]
    bad = [R.corrupt_chunk(s, rows[i]) for i in (0, 1, 3)]
    ix = X.build_index([s] * 4)
    assert all(X.build_index([x])["pos"] == X.build_index([s])["pos"] for x in bad)
    got = RC.rechunk_plan(bad + [s], ix, cb)
    want1, want3 = M.chunk_status(bad[1], rows[1]), M.chunk_status(bad[2], rows[3])
    assert want1 != O.OK and want3 != O.OK
    assert got["status"] == [O.OK, want1, want3, O.OK]
    assert got["streams"][1] is None and got["out_len"][1] == 0 and got["out_bound"][1] == 0 and got["out_bound"][3] > 0
    assert got["streams"][3] == K.stream_of(raw, cb)
    c0 = rows[1][1] - 8                                                 # chunk 0 ends where chunk 1's header starts
    assert got["streams"][0][:c0] == bad[0][:c0] != s[:c0] and got["streams"][0][c0:] == got["streams"][3][c0:]      # copied as it is
    with pytest.raises(O.OracleError):
        O.frame_decode(got["streams"][0])
    assert got["result"][3] == 2 and got["index"]["tail"] == [0] * 4
    scrub = RC.rechunk_plan(bad + [s], ix, cb, ALL)
    assert scrub["status"] == [M.chunk_status(bad[0], rows[0]), want1, want3, O.OK] and scrub["status"][0] != O.OK
    both = R.corrupt_chunk(bad[1], rows[3])                             # two dirty chunks corrupt: the first one's status
    assert RC.rechunk_plan([both], X.build_index([s]), cb)["status"] == [want1]


def test_admission_is_in_stream_order_by_each_bound_and_out_cap_hits_one_stream():
    html = read_testdata("html")
    cb = 512
    blobs = [html[:700], html[50:50 + 1024], html[9:9 + 1300], html[:100], html[:2000]]
    streams = [K.stream_of(x, 500) for x in blobs[:3]] + [K.stream_of(blobs[3], cb), K.stream_of(blobs[4], 300)]
    ix = X.build_index(streams)
    full = RC.rechunk_plan(streams, ix, cb)
    assert full["status"] == [O.OK] * 5 and full["alone"] == [False, False, False, True, False]
    # every row of the 500- and 300-byte streams is dirty; stream 3 is canonical.  rows: max(old, new) per written stream
    dirty = [2, 3, 3, 0, 7]
    slots = [2, 2, 3, 0, 4]
    stage = [700, 1024, 1300, 0, 2000]
    rows = [2, 3, 3, 1, 7]
    assert full["result"] == [max(sum(dirty), sum(slots)), sum(full["out_len"]), sum(stage), 4, sum(rows), 1]
    assert full["streams"][:3] == [K.stream_of(x, cb) for x in blobs[:3]]
    ms, sc, me = full["result"][0], full["result"][2], full["result"][4]
    assert RC.rechunk_plan(streams, ix, cb, max_slots=ms, stage_cap=sc, max_entries=me) == full
    late = [O.OK, O.OK, O.OK, O.OK, O.ERR_OUTPUT_TOO_SMALL]
    for bounds in (dict(max_slots=ms - 1, stage_cap=sc, max_entries=me), dict(max_slots=ms, stage_cap=sc - 1, max_entries=me),
                   dict(max_slots=ms, stage_cap=sc, max_entries=me - 1)):
        short = RC.rechunk_plan(streams, ix, cb, **bounds)
        assert short["status"] == late and short["streams"][:3] == full["streams"][:3] and short["streams"][4] is None, bounds
        assert short["result"] == [ms, sum(short["out_len"]), sc, 3, me, 1]
        assert RC.same_index(short["index"], X.build_index(RC.after(streams, short)))
    # in the middle: stream 1 misses, and every later one that needs work; the canonical one is left alone all the same
    mid = [O.OK, O.ERR_OUTPUT_TOO_SMALL, O.ERR_OUTPUT_TOO_SMALL, O.OK, O.ERR_OUTPUT_TOO_SMALL]
    assert RC.rechunk_plan(streams, ix, cb, max_slots=4, stage_cap=sc, max_entries=me)["status"] == mid           # 2 + 3 dirty rows
    assert RC.rechunk_plan(streams, ix, cb, max_slots=ms, stage_cap=700 + 1023, max_entries=me)["status"] == mid
    assert RC.rechunk_plan(streams, ix, cb, max_slots=ms, stage_cap=sc, max_entries=4)["status"] == mid
    sizing = RC.rechunk_plan(streams, ix, cb, caps=[0] * 5, max_slots=0, stage_cap=0, max_entries=0)
    assert sizing["result"] == [ms, 0, sc, 0, me, 1] and sizing["out_bound"] == full["out_bound"]
    assert sizing["status"] == [O.ERR_OUTPUT_TOO_SMALL] * 3 + [O.OK, O.ERR_OUTPUT_TOO_SMALL]
    assert all(b >= n for b, n in zip(sizing["out_bound"], full["out_len"]))
    assert sizing["index"]["first"] == [0] * 6 and sizing["index"]["total"] == ix["total"]        # (no room for a row)
    caps = list(full["out_len"])
    caps[2] -= 1                                                        # one byte short, in the middle
    one = RC.rechunk_plan(streams, ix, cb, caps=caps)
    assert one["status"] == [O.OK, O.OK, O.ERR_OUTPUT_TOO_SMALL, O.OK, O.OK] and one["streams"][2] is None and one["out_len"][2] == 0
    assert RC.same_index(one["index"], X.build_index(RC.after(streams, one)))
    assert one["result"] == [ms, sum(one["out_len"]), sc, 3, me, 1]


def test_every_rejection():
    html = read_testdata("html")
    cb = 1000
    streams = [K.stream_of(html[:n], 900) for n in (2500, 2000, 300)] + [R.uniform_stream(3, 1)[0][:-5]]
    ix = X.build_index(streams)
    assert ix["tail"][3] == O.ERR_TRUNCATED_STREAM and ix["first"] == [0, 3, 6, 7, ix["first"][4]]

    def statuses(flags=0, **change):
        return RC.rechunk_plan(streams, {**ix, **change}, cb, flags)["status"]

    assert statuses() == statuses(ALL) == [O.OK, O.OK, O.OK, O.ERR_TRUNCATED_STREAM]
    assert statuses(tail=[O.ERR_OUTPUT_TOO_SMALL, 0, 77, -1]) == [O.ERR_OUTPUT_TOO_SMALL, O.OK, O.ERR_BAD_ARG, O.ERR_BAD_ARG]
    assert statuses(total=[2501, 1999, 0, 0])[:3] == [O.ERR_BAD_ARG] * 3                              # lengths that disagree with headers
    assert statuses(pos=[p + 1 for p in ix["pos"]])[:3] == [O.ERR_BAD_ARG] * 3
    assert statuses(first=[0, 0, 3, 6, 6])[:3] == [O.ERR_BAD_ARG, O.OK, O.ERR_BAD_ARG]      # bytes and no row; rows of a twin stream that fit the headers; the rows of a longer stream
    assert statuses(first=[3, 0, 5, 6, 6])[0] == O.ERR_BAD_ARG                                        # f1 < f0
    assert statuses(first=[1, 3, 6, 7, 7])[0] == O.ERR_BAD_ARG                                        # the first row does not start at 0
    assert statuses(start=list(reversed(ix["start"])))[0] == O.ERR_BAD_ARG                           # rows backwards
    gap = list(ix["start"])
    gap[1] += 1                                                         # a gap behind row 0 / an overlap of rows 0 and 1
    assert statuses(start=gap)[0] == O.ERR_BAD_ARG
    gap[1] -= 2
    assert statuses(start=gap)[0] == O.ERR_BAD_ARG
    swapped = list(ix["pos"])
    swapped[0], swapped[1] = swapped[1], swapped[0]                     # positions that do not increase
    assert statuses(pos=swapped)[0] == O.ERR_BAD_ARG
    same = list(ix["pos"])
    same[1] = same[0]
    assert statuses(pos=same)[0] == O.ERR_BAD_ARG
    past = list(ix["pos"])
    past[2] = len(streams[0])                                           # pos past in_len
    assert statuses(pos=past)[0] == O.ERR_BAD_ARG
    # a row at a skippable chunk
    skip = M.STREAM_ID + M.data_chunk(html[:100]) + M.chunk(0x80, b"note") + M.data_chunk(html[100:200])
    six = X.build_index([skip])
    assert RC.rechunk_plan([skip], six, cb)["status"] == [O.OK]
    moved = {**six, "pos": [six["pos"][0], six["pos"][1] - 8]}
    assert RC.rechunk_plan([skip], moved, cb)["status"] == [O.ERR_BAD_ARG]
    # a dirty chunk above 65536 bytes
    big = R.big_chunk_stream()[0]
    bix = X.build_index([big])
    assert max(RC.data_chunk_lengths(big)) > 65536
    assert RC.rechunk_plan([big], bix, 65536)["status"] == [O.ERR_BAD_ARG] == RC.rechunk_plan([big], bix, 4096, ALL)["status"]


@pytest.fixture(scope="module")
def named():
    cases = X.named_streams()
    streams = list(cases.values())
    return list(cases), streams, X.build_index(streams)


def test_named_streams_rechunk_as_the_contract_says(named):
    names, streams, ix = named
    for flags in (0, ALL):
        got = RC.rechunk_plan(streams, ix, 4096, flags)
        written = 0
        for b, s in enumerate(streams):
            if got["streams"][b] is not None:
                try:
                    old = O.frame_decode(s)
                except O.OracleError:                                   # (a corrupt kept chunk: copied)
                    assert flags == 0
                    old = None
                if old is not None:
                    assert O.frame_decode(got["streams"][b]) == old, names[b]
                    if flags:
                        assert got["streams"][b] == K.stream_of(old, 4096), names[b]
                written += 1
            else:
                assert got["out_len"][b] == 0 and (got["status"][b] != O.OK or got["alone"][b]), names[b]
                if ix["tail"][b] != O.OK:
                    assert got["status"][b] == ix["tail"][b]
        assert RC.same_index(got["index"], X.build_index(RC.after(streams, got)))
        assert got["result"][3] == written >= 8 and len(set(got["status"])) >= 3, (written, set(got["status"]))


def test_unsound_indexes_get_the_models_verdicts(named):
    names, streams, ix = named
    rng = np.random.default_rng(5)
    sound = RC.rechunk_plan(streams, ix, 4096)
    refused = kept = 0
    for bad in RC.unsound_indexes(ix, streams, rng):
        ne = min(len(bad["start"]), len(bad["pos"]))
        me = ne + 64
        got = RC.rechunk_plan(streams, bad, 4096, max_slots=1 << 20, stage_cap=1 << 28, max_entries=me)
        assert len(got["index"]["start"]) == len(got["index"]["pos"]) <= me                # the new arrays stay inside max_entries
        assert got["index"]["first"][-1] == len(got["index"]["start"]) and got["index"]["first"] == sorted(got["index"]["first"])
        for b, s in enumerate(streams):
            if got["streams"][b] is None:
                assert got["out_len"][b] == 0
                refused += got["status"][b] != sound["status"][b]
            else:                                                       # whatever passed the checks is data chunks on the grid
                new = got["streams"][b]
                assert got["out_len"][b] == len(new) <= got["out_bound"][b] and new[:10] == M.STREAM_ID
                nix = X.build_index([new])
                assert nix["tail"] == [O.OK] and nix["start"] == [4096 * k for k in range(len(nix["start"]))] and nix["total"] == [bad["total"][b]]
                kept += 1
    assert refused > 40 and kept > 10, (refused, kept)
    # a stale index: that of other bytes with the same shape
    html = read_testdata("html")
    a, b2 = K.stream_of(html[:9000], 4000), K.stream_of(html[500:9500][::-1], 4000)
    stale = RC.rechunk_plan([b2], X.build_index([a]), 4096)
    assert stale["status"] == [O.OK if X.build_index([a])["pos"] == X.build_index([b2])["pos"] else O.ERR_BAD_ARG]


# ---- the planning header on the CPU, under sanitizers ------------------------------------------------------------------------------------------
def test_planning_header_under_sanitizers_matches_the_model(named, tmp_path):
    names, streams, ix = named
    html = read_testdata("html") * 5
    foreign = [c[0] for c in RC.foreign_streams(html).values()]
    shaped = fragmented(html, 1000, O.HASH_CRC32C)[2] + [K.stream_of(html[:n], 1000) for n in (0, 1, 1000, 3500)]
    streams = streams + foreign + shaped
    ix = X.build_index(streams)
    ns = len(streams)
    rng = np.random.default_rng(11)
    cases = [(ix, cb, flags) for cb in (1, 500, 1000, 4096, 65536) for flags in (0, ALL)]
    nsound = len(cases)
    cases += [(bad, cb, flags) for bad in RC.unsound_indexes(ix, streams, rng) for cb, flags in ((1000, 0), (65536, ALL))]
    # random indexes: rows filled with anything
    for _ in range(6):
        ne = int(rng.integers(0, 40))
        cases.append((dict(first=[int(v) for v in rng.integers(0, ne + 3, ns + 1)], start=[int(v) for v in rng.integers(0, 5000, ne)],
                           pos=[int(v) for v in rng.integers(0, 3000, ne)], total=[int(v) for v in rng.integers(0, 9000, ns)],
                           tail=[int(v) for v in rng.integers(-1, 3, ns)]), int(rng.integers(1, 5000)), int(rng.integers(0, 2))))
    # streams past 4 GiB, as numbers: two clean rows on the 65536 grid behind 5 GiB of ... nothing (the first must start at 0: refused); two rows
    # from 0 with positions past 4 GiB, canonical but for the position of the first; the same with the flag; the second row dirty (off the
    # grid); a skippable chunk at the second; the second header inside the first chunk; a position at the end; a dirty row above 65536 bytes;
    # a tail that is an error; one row, and a total past 4 GiB that no row holds; no row and nothing decoded: the identifier is missing, present
    G = 1 << 32
    base = dict(n=2 * G + 2 * 65544 + 10, cb=65536, flags=0, total=65536 + 3000, tail=0, rows=2, ident=1,
                start0=0, pos0=2 * G + 10, kind0=0, size0=4 + 65536, dec0=65536, start1=65536, pos1=2 * G + 10 + 65544, kind1=0, size1=4 + 65536,
                dec1=3000)
    numeric = [{**base, "start0": 5 * G, "start1": 5 * G + 65536, "total": 5 * G + 65536 + 3000}, base, {**base, "flags": ALL},
               {**base, "cb": 4096}, {**base, "kind1": 1}, {**base, "pos1": base["pos0"] + 100}, {**base, "pos1": base["n"]},
               {**base, "cb": 1000, "dec0": 65537, "start1": 65537, "dec1": 2999}, {**base, "tail": O.ERR_CRC_MISMATCH},
               {**base, "rows": 1, "total": 5 * G}, {**base, "rows": 0, "total": 0, "n": 0, "ident": 0}, {**base, "rows": 0, "total": 0, "n": 10},
               {**base, "pos0": 10, "pos1": 10 + 65544, "n": 10 + 2 * 65544}, {**base, "cb": 1, "flags": ALL, "dec0": 65536}]
    path = str(tmp_path / "cases.bin")
    RC.write_cases(path, streams, cases, numeric)
    exe = str(tmp_path / "frame_rechunk_plan_check")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host",
                    "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "abi", "frame_rechunk_plan_check.hip"), "-o", exe,
                    "-Wl,-rpath,/opt/rocm/lib"], check=True)
    env = {**os.environ, "ASAN_OPTIONS": "detect_leaks=1:abort_on_error=0", "UBSAN_OPTIONS": "print_stacktrace=1:halt_on_error=1"}
    run = subprocess.run([exe, path], capture_output=True, text=True, env=env)
    assert run.returncode == 0 and run.stderr == "", run.stderr[-3000:]      # the sanitizers are silent
    lines = run.stdout.splitlines()
    assert len(lines) == ns * len(cases) + len(numeric)
    at = passed = refused = 0
    for c, (index, cb, flags) in enumerate(cases):
        for b, w in enumerate(RC.plan_lines(index, streams, cb, flags)):
            assert lines[at] == w, (c, b, cb, flags)
            unsound = c >= nsound
            passed += unsound and w.startswith("0 1 ")
            refused += unsound and not w.startswith("0 ")
            at += 1
    assert passed > 50 and refused > 200, (passed, refused)            # both outcomes, on the unsound indexes
    want = [RC.numeric_line(c) for c in numeric]
    assert lines[at:] == want
    # the numbers themselves
    f = [[int(v) for v in w.replace("|", " ").split()] for w in want]
    assert f[0][0] == O.ERR_BAD_ARG
    assert f[1][:3] == [0, 1, 0] and f[1][5:11] == [0, 0, 2, 0, 2 * 65544, 10 + 2 * 65544]         # not canonical by position alone: both rows kept
    assert f[1][15:23] == [1, 0, 0, 65536, 1, 1, 65536, 3000]
    assert f[2][:3] == [0, 1, 1] and f[2][5:11] == [2, 65536 + 3000, 2, 2, 0, 10 + 16 + 65536 + 3000] and f[2][23] == 3000
    assert f[3][:3] == [0, 1, 0] and f[3][5:9] == [1, 65536, 17, 16] and f[3][19:24] == [1, 1, 65536, 3000, 4096]     # the short last row is on the 4096 grid: kept
    for i in (4, 5, 6, 7, 9):
        assert f[i][0] == O.ERR_BAD_ARG, i
    assert f[8][0] == O.ERR_CRC_MISMATCH
    assert f[10][:2] == [0, 1] and f[10][10] == 10 and f[11][:2] == [0, 0]
    assert f[12][:2] == [0, 0]                                          # canonical
    assert f[13][:3] == [0, 1, 1] and f[13][7:9] == [65536 + 3000] * 2 and f[13][23] == 1

"""snp_frame_write_indexed_batch (libsnappier_hip_frame_update.so) without a GPU: the declarations and their C# binding, the workspace arithmetic,
argument rejection; the Python model of the contract (frame_update_model.py) checked against the oracle, the index model and the chunked
encoder's model over the named streams and over chunked streams at the seam sizes; every request error, admission, corruption inside an edge
and inside a wholly covered chunk, stale and unsound indexes; and the planning header (csrc/frame_update_device.h) itself, compiled for the CPU
under AddressSanitizer and UBSan into a stand-alone program (tests/abi/frame_update_plan_check.hip) and run over the same cases and over
indexes and request lists filled with anything at all."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import frame_chunked_model as K
import frame_index_model as X
import frame_range_model as R
import frame_update_model as U
import oracle as O
from conftest import ROOT, read_testdata

NAMES = ["snp_frame_write_indexed_batch", "snp_frame_write_indexed_workspace"]
BIG = 1 << 62


def _lib():
    from snappier_amd import _native as N
    return N.frame_update_lib()


# ---- the surface -----------------------------------------------------------------------------------------------------------------------------
def test_header_and_binding_declare_the_new_functions():
    from snappier_amd import _native as N
    declared = N.frame_update_declared_symbols()
    assert declared == NAMES
    others = set(N.declared_symbols()) | set(N.buffers_declared_symbols()) | set(N.buffers_decompress_declared_symbols()) | \
        set(N.frame_buffers_declared_symbols()) | set(N.layout_declared_symbols()) | set(N.frame_range_declared_symbols()) | \
        set(N.frame_index_declared_symbols()) | set(N.frame_chunked_declared_symbols())
    assert not set(declared) & others                                  # the other headers' surfaces are left as they are
    lib = _lib()
    assert lib.snp_frame_write_indexed_batch.restype is C.c_int and len(lib.snp_frame_write_indexed_batch.argtypes) == 29
    assert lib.snp_frame_write_indexed_workspace.restype is C.c_uint64 and len(lib.snp_frame_write_indexed_workspace.argtypes) == 4


def test_extension_library_exports_exactly_its_header():
    from layouts import exported
    from snappier_amd import _native as N

    ext = exported(N.FRAME_UPDATE_PATH)
    assert ext == set(NAMES)
    for other in (N.PRODUCT_PATH, N.BUFFERS_PATH, N.BUFFERS_DECOMPRESS_PATH, N.FRAME_BUFFERS_PATH, N.LAYOUT_PATH, N.FRAME_RANGE_PATH, N.FRAME_INDEX_PATH,
                  N.FRAME_CHUNKED_PATH):
        assert not exported(other) & ext


def test_workspace_is_host_arithmetic():
    ws = _lib().snp_frame_write_indexed_workspace
    assert ws(0, 5, 10, 1000) == 0 and ws(5, 0, 10, 1000) == 0          # nothing when there is no stream or no request
    for ns in (1, 255, 1025, 300000):
        for nr in (1, 2, 1024, 1025, 300000):
            for ms in (0, 1, 70000):
                for sc in (0, 1, 65536, 200001, 5 << 30):
                    w = ws(ns, nr, ms, sc)
                    assert w % 256 == 0
                    # the raw staging, the compressed staging (raw + raw / 6, 96 + 64 bytes per slot), the slot table and its decode rows, the
                    # request's and the stream's words
                    assert w >= sc + sc + sc // 6 + ms * 160 + ms * (76 + 41) + nr * 68 + ns * 84
                    assert w <= 2.2 * sc + ms * 300 + nr * 80 + ns * 100 + 50 * 256 + (ns + nr + ms) // 100
                    assert ws(ns + 1, nr, ms, sc) >= w and ws(ns, nr + 1, ms, sc) >= w and ws(ns, nr, ms + 1, sc) >= w and ws(ns, nr, ms, sc + 1) >= w
    assert ws(0xFFFFFFFF, 0x7FFFFFFF, 0xFFFFFFFF, 1 << 40) > 0xFFFFFFFF * 160 + (2 << 40)      # (64-bit arithmetic)


def test_batch_call_rejects_bad_arguments_without_a_device():
    call = _lib().snp_frame_write_indexed_batch
    fake = C.c_void_p(64)                                               # (never dereferenced: the arguments are refused first)
    # ctx; in, in_off, in_len; nstreams; five index arrays; nentries; src, req_stream, req_off, req_len, src_off; nreq, max_slots, stage_cap;
    # out, out_off, out_cap, out_len, status, req_status; new_pos, out_bound; d_work, d_result
    def args(ctx=fake, ins=(fake,) * 3, ns=1, idx=(fake,) * 5, ne=8, reqs=(fake,) * 5, nreq=1, outs=(fake,) * 6, opt=(None, None), work=fake, result=fake):
        return (ctx, *ins, ns, *idx, ne, *reqs, nreq, 0, 0, *outs, *opt, work, result)

    assert call(*args(ctx=None)) == O.ERR_BAD_ARG
    assert call(*args(result=None)) == O.ERR_BAD_ARG
    assert call(*args(ns=0, nreq=0, result=None)) == O.ERR_BAD_ARG      # an empty call still needs d_result
    assert call(*args(nreq=0x80000000)) == O.ERR_BAD_ARG                # nreq >= 2^31
    assert call(*args(work=None)) == O.ERR_BAD_ARG
    for group, n in (("ins", 3), ("reqs", 5), ("outs", 6)):
        for i in range(n):
            a = [fake] * n
            a[i] = None
            assert call(*args(**{group: tuple(a)})) == O.ERR_BAD_ARG, (group, i)
    for i in (0, 3, 4):                                                 # idx_first, idx_total, idx_tail
        a = [fake] * 5
        a[i] = None
        assert call(*args(idx=tuple(a))) == O.ERR_BAD_ARG, i
    assert call(*args(idx=(fake, None, fake, fake, fake))) == O.ERR_BAD_ARG     # rows, no row arrays
    assert call(*args(idx=(fake, fake, None, fake, fake))) == O.ERR_BAD_ARG


def test_csharp_binding_matches_the_extension_header():
    import test_csharp_signatures as T
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "snappier_hip_frame_update.h")).read(), flags=re.S)
    protos = {}
    for m in re.finditer(r"([A-Za-z_][A-Za-z0-9_ ]*?[\s\*]+)(snp_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", text):
        params = [re.match(r"(.*?[\s\*])([A-Za-z_][A-Za-z0-9_]*)$", q.strip()).group(1) for q in m.group(3).split(",") if q.strip() not in ("", "void")]
        protos[m.group(2)] = (T.c_class(m.group(1)), [T.c_class(q) for q in params])
    cs = re.sub(r"//.*", "", open(os.path.join(ROOT, "csharp", "Snappier.Gpu", "NativeMethodsFrameUpdate.cs")).read())
    assert 'const string Lib = "snappier_hip_frame_update"' in cs
    imps = {}
    for m in re.finditer(r"\[DllImport\(Lib, CallingConvention = Cc\)\]\s*internal static extern ([A-Za-z\*]+) (snp_[a-z0-9_]+)\(([^)]*)\);", cs):
        params = [re.match(r"(.*?)\s+([A-Za-z_][A-Za-z0-9_]*)$", q.strip()).group(1) for q in m.group(3).split(",") if q.strip()]
        imps[m.group(2)] = (T.cs_class(m.group(1)), [T.cs_class(q) for q in params])
    assert set(protos) == set(imps) == set(NAMES)
    for name, (ret, params) in protos.items():
        cret, cparams = imps[name]
        assert T.compatible(ret, cret), (name, ret, cret)
        assert len(params) == len(cparams) and all(T.compatible(a, b) for a, b in zip(params, cparams)), (name, params, cparams)
    assert len(protos["snp_frame_write_indexed_batch"][1]) == 29 and len(protos["snp_frame_write_indexed_workspace"][1]) == 4
    proj = open(os.path.join(ROOT, "csharp", "Snappier.Gpu", "Snappier.Gpu.csproj")).read()
    assert 'Include="../../snappier_amd/libsnappier_hip_frame_update.so"' in proj


# ---- the model -------------------------------------------------------------------------------------------------------------------------------
def decoded_rows(s: bytes):
    """-> (rows of the walk, what each decodes to: None for a corrupt one)."""
    rows = R.walk(s)[0]
    return rows, [R.chunk_result(s, r)[1] if r[5] else b"" for r in rows]


def check_one(streams, ix, b: int, lst, rng, variant=O.HASH_CRC32C):
    """One request list on stream b of a batch, against everything the contract promises.  -> the model's answer."""
    reqs = [(b, off, ln) for off, ln in lst]
    srcs = [U.fresh(rng, ln) for _, _, ln in reqs]
    got = U.write_plan(streams, ix, reqs, srcs, variant=variant)
    s = streams[b]
    rows, parts = decoded_rows(s)
    touched = [any(off < r[4] + r[5] and off + ln > r[4] and ln for _, off, ln in reqs) for r in rows]
    covered = [any(off <= r[4] and off + ln >= r[4] + r[5] for _, off, ln in reqs) for r in rows]
    broken = [r for r, p, t, c in zip(rows, parts, touched, covered) if p is None and t and not c]
    if broken:                                                          # a corrupt chunk written in part: its status, and nothing is written
        import frame_buffers_model as M
        want = M.chunk_status(s, broken[0])
        assert got["status"][b] == want and got["streams"] == [None] * len(streams) and set(got["req_status"]) == {want}
        return got
    assert got["status"][b] == O.OK and got["req_status"] == [O.OK] * len(reqs), (b, lst, got["status"])
    new = got["streams"][b]
    flat = U.patched(b"".join(bytes(r[5]) if p is None else p for r, p in zip(rows, parts)), reqs, srcs, b)
    new_rows, new_parts = decoded_rows(new)
    assert len(new_rows) == len(rows) and R.walk(new)[1:3] == R.walk(s)[1:3]
    for r, p, t, q in zip(rows, parts, touched, new_parts):
        assert q == (None if p is None and not t else flat[r[4]:r[4] + r[5]])      # (a corrupt chunk nobody touches stays as it is; a covered one is repaired)
    assert len(new) == got["out_len"][b] <= got["out_bound"][b]
    # every other stream is left alone; the index of the new streams is the old one with new_pos
    others = [x for i, x in enumerate(got["streams"]) if i != b]
    assert others == [None] * (len(streams) - 1) and [got["out_len"][i] for i in range(len(streams)) if i != b] == [0] * (len(streams) - 1)
    after = X.build_index([new if i == b else x for i, x in enumerate(streams)])
    assert after == {**ix, "pos": got["new_pos"], "result": after["result"]}
    # the bytes outside the dirty chunks are verbatim, in order
    at = out = 0
    for p, o, c in got["dirty"][b]:
        assert new[out:out + (p - at)] == s[at:p] and new[out + (p - at):out + (p - at) + len(c)] == c
        out += p - at + len(c)
        at = p + o
    assert new[out:] == s[at:]
    # a chunk is dirty iff a request writes a byte of it
    rows = R.walk(s)[0]
    hit = {r[1] - 8 for r in rows if r[5] and any(off < r[4] + r[5] and off + ln > r[4] and ln for _, off, ln in reqs)}
    assert {p for p, _, _ in got["dirty"][b]} == hit
    return got


@pytest.fixture(scope="module")
def named():
    cases = X.named_streams()
    streams = list(cases.values())
    return list(cases), streams, X.build_index(streams)


def test_named_streams_update_as_the_contract_says(named):
    names, streams, ix = named
    rng = np.random.default_rng(1)
    done = refused = 0
    for b, s in enumerate(streams):
        tail = ix["tail"][b]
        for lst in U.row_requests(s):
            reqs = [(b, off, ln) for off, ln in lst]
            srcs = [U.fresh(rng, ln) for _, _, ln in reqs]
            rows = R.walk(s)[0]
            big = any(r[5] > 65536 and any(off < r[4] + r[5] and off + ln > r[4] and ln for _, off, ln in reqs) for r in rows)
            if tail != O.OK or big:                                     # a broken stream gives its walk's status, a dirty chunk above 65536 BAD_ARG
                got = U.write_plan(streams, ix, reqs, srcs)
                want = tail if tail != O.OK else O.ERR_BAD_ARG
                assert got["status"][b] == want and got["req_status"] == [want] * len(reqs) and got["streams"] == [None] * len(streams), names[b]
                assert got["new_pos"] == ix["pos"] and got["result"][1] == got["result"][3] == 0
                refused += 1
                continue
            check_one(streams, ix, b, lst, rng)
            done += 1
    assert done > 50 and refused > 20, (done, refused)                  # both outcomes


@pytest.mark.parametrize("cb", U.CHUNK_SIZES)
def test_chunked_streams_update_to_the_chunked_encode_of_the_patched_buffer(cb):
    html = read_testdata("html")
    rng = np.random.default_rng(cb)
    for variant in (O.HASH_CRC32C, O.HASH_MUL):
        blobs = [(html * 3)[7:7 + n] for n in U.lengths(cb)]
        streams = [K.stream_of(x, cb, variant) for x in blobs]
        ix = X.build_index(streams)
        for b, raw in enumerate(blobs):
            for lst in U.request_shapes(len(raw), cb):
                if not raw and any(ln for _, ln in lst):
                    continue
                got = check_one(streams, ix, b, lst, rng, variant)
                reqs = [(b, off, ln) for off, ln in lst]
                # the update equals the chunked encode of the patched buffer, byte for byte (so do the positions)
                patched = O.frame_decode(got["streams"][b])
                assert got["streams"][b] == K.stream_of(patched, cb, variant), (cb, b, lst)
                assert len(reqs) == len(lst)


def test_several_streams_each_get_their_own_verdict(named):
    html = read_testdata("html")
    cb = 1000
    blobs = [html[:5000], html[100:4100], html[7:3007], html[:2500], html[9:9 + 6001], html[:1]]
    streams = [K.stream_of(x, cb) for x in blobs]
    ix = X.build_index(streams)
    reqs = [(0, 10, 20), (0, 990, 20), (0, 4999, 1),       # stream 0: three requests, two chunks shared by none
            (2, 0, 3000),                                  # stream 2: whole
            (3, 100, 10), (3, 105, 10),                    # stream 3: the second overlaps the first
            (4, 500, 3000),                                # stream 4: out_cap one byte short
            (5, 0, 0)]                                     # stream 5: named by an empty request only: a copy
    rng = np.random.default_rng(2)
    srcs = [U.fresh(rng, ln) for _, _, ln in reqs]
    free = U.write_plan(streams, ix, reqs, srcs)
    assert free["status"] == [O.OK, O.OK, O.OK, O.ERR_BAD_ARG, O.OK, O.OK] and free["out_len"][1] == 0 and free["streams"][5] == streams[5]
    caps = [BIG] * 6
    caps[4] = free["out_len"][4] - 1
    got = U.write_plan(streams, ix, reqs, srcs, caps)
    assert got["status"] == [O.OK, O.OK, O.OK, O.ERR_BAD_ARG, O.ERR_OUTPUT_TOO_SMALL, O.OK]
    assert got["req_status"] == [O.OK] * 4 + [O.ERR_BAD_ARG, O.ERR_BAD_ARG, O.ERR_OUTPUT_TOO_SMALL, O.OK]    # a fine request of a refused stream gets its stream's status
    assert got["streams"][1] is None and got["streams"][3] is None and got["streams"][4] is None
    assert got["result"] == [3 + 3 + 4, sum(got["out_len"]), 1000 * 3 + 3000 + 4000, 3]
    assert got["out_bound"][1] == got["out_bound"][3] == 0 and got["out_bound"][4] >= free["out_len"][4]
    for b in (0, 2):
        assert O.frame_decode(got["streams"][b]) == U.patched(blobs[b], reqs, srcs, b)
    f = ix["first"]
    assert got["new_pos"][f[1]:f[2]] == ix["pos"][f[1]:f[2]] and got["new_pos"][f[3]:f[5]] == ix["pos"][f[3]:f[5]]      # rows of streams not written
    assert X.build_index([got["streams"][b] or streams[b] for b in range(6)])["pos"] == got["new_pos"]


def test_admission_is_in_stream_order_by_each_bound():
    html = read_testdata("html")
    cb = 512
    blobs = [html[:3000], html[50:2050], html[9:9 + 4000], html[:700]]
    streams = [K.stream_of(x, cb) for x in blobs]
    ix = X.build_index(streams)
    reqs = [(0, 100, 1000), (1, 0, 512), (1, 600, 10), (2, 511, 2), (3, 0, 0)]
    srcs = [bytes(ln) for _, _, ln in reqs]
    full = U.write_plan(streams, ix, reqs, srcs)
    slots, stage = full["result"][0], full["result"][2]
    assert full["status"] == [O.OK] * 4 and (slots, stage) == (3 + 2 + 2, 1536 + 1024 + 1024)
    assert U.write_plan(streams, ix, reqs, srcs, max_slots=slots, stage_cap=stage) == full
    short = U.write_plan(streams, ix, reqs, srcs, max_slots=slots - 1, stage_cap=stage)
    assert short["status"] == [O.OK, O.OK, O.ERR_OUTPUT_TOO_SMALL, O.ERR_OUTPUT_TOO_SMALL]        # the stream that misses, and every later named one
    assert short["req_status"] == [O.OK, O.OK, O.OK, O.ERR_OUTPUT_TOO_SMALL, O.ERR_OUTPUT_TOO_SMALL] and short["streams"][:2] == full["streams"][:2]
    short = U.write_plan(streams, ix, reqs, srcs, max_slots=slots, stage_cap=1536 + 1023)
    assert short["status"] == [O.OK] + [O.ERR_OUTPUT_TOO_SMALL] * 3 and short["result"][::2] == [slots, stage]
    sizing = U.write_plan(streams, ix, reqs, srcs, caps=[0] * 4, max_slots=0, stage_cap=0)
    assert sizing["status"] == [O.ERR_OUTPUT_TOO_SMALL] * 4 and sizing["result"] == [slots, 0, stage, 0]
    assert all(b >= n for b, n in zip(sizing["out_bound"], full["out_len"])) and sizing["out_bound"] == full["out_bound"]


def test_request_errors():
    html = read_testdata("html")
    cb = 1000
    streams = [K.stream_of(html[:n], cb) for n in (5000, 4000, 3000)] + [R.big_chunk_stream()[0], R.uniform_stream(3, 1)[0][:-5]]
    ix = X.build_index(streams)
    assert ix["tail"][4] == O.ERR_TRUNCATED_STREAM
    unindexed = {**ix, "tail": ix["tail"][:2] + [O.ERR_OUTPUT_TOO_SMALL] + ix["tail"][3:]}
    big = next(r for r in R.walk(streams[3])[0] if r[5] > 65536)

    def statuses(reqs, index=ix):
        got = U.write_plan(streams, index, reqs, [bytes(min(ln, 1 << 20)) for _, _, ln in reqs])
        return got["req_status"], got["status"]

    assert statuses([(0, 10, 5), (0, 12, 5)])[0] == [O.ERR_BAD_ARG, O.ERR_BAD_ARG]                 # overlap: the second fails, the stream with it
    assert statuses([(0, 10, 5), (0, 15, 5)])[0] == [O.OK, O.OK]                                  # touching is disjoint
    assert statuses([(0, 20, 5), (0, 10, 5)])[0] == [O.ERR_BAD_ARG, O.ERR_BAD_ARG]                 # offsets out of order
    rq, st = statuses([(1, 0, 5), (0, 0, 5), (2, 0, 5)])                                           # streams out of order
    assert rq[1] == O.ERR_BAD_ARG and st[0] == O.ERR_BAD_ARG and st[2] == O.OK
    rq, st = statuses([(0, 0, 5), (2, 0, 5), (1, 0, 5), (2, 9, 5)])                                # a stream's requests apart: it is not written
    assert st[2] == O.ERR_BAD_ARG and st[1] == O.ERR_BAD_ARG and st[0] == O.OK and rq[0] == O.OK
    assert statuses([(5, 0, 1)])[0] == [O.ERR_BAD_ARG] and statuses([(0xFFFFFFFF, 0, 0)])[0] == [O.ERR_BAD_ARG]
    assert statuses([(0, 4999, 2)])[0] == [O.ERR_BAD_ARG] and statuses([(0, 5000, 1)])[0] == [O.ERR_BAD_ARG]     # past the end
    assert statuses([(0, 5000, 0)])[0] == [O.OK] and statuses([(0, 5001, 0)])[0] == [O.ERR_BAD_ARG]
    assert statuses([(0, U.U64, 2)])[0] == [O.ERR_BAD_ARG] and statuses([(0, 1, U.U64)])[0] == [O.ERR_BAD_ARG]   # wrapping
    assert statuses([(3, big[4] + 1, 1)])[0] == [O.ERR_BAD_ARG] and statuses([(3, big[4], big[5])])[0] == [O.ERR_BAD_ARG]   # a dirty chunk above 65536
    assert statuses([(3, big[4] - 1, 1)])[0] == [O.OK]                                             # ... its neighbour is fine
    assert statuses([(4, 0, 1)])[0] == [O.ERR_TRUNCATED_STREAM]                                    # a broken stream
    assert statuses([(2, 0, 1)], unindexed)[0] == [O.ERR_OUTPUT_TOO_SMALL]
    assert statuses([(2, 0, 1)], {**ix, "tail": [0, 0, 77, 0, 0]})[0] == [O.ERR_BAD_ARG]


def test_a_corrupt_edge_is_noticed_and_a_corrupt_covered_chunk_is_repaired():
    html = read_testdata("html")
    cb = 4096
    raw = html[:5 * cb]
    s = K.stream_of(raw, cb)
    rows = R.walk(s)[0]
    bad = R.corrupt_chunk(s, rows[2])
    ix = X.build_index([bad])
    assert ix == X.build_index([s])
    import frame_buffers_model as M
    want = M.chunk_status(bad, rows[2])
    assert want != O.OK
    src = bytes(range(256)) * 40
    edge = U.write_plan([bad], ix, [(0, 2 * cb + 5, cb)], [src[:cb]])                             # chunk 2 is the head edge
    assert edge["status"] == [want] and edge["req_status"] == [want] and edge["streams"] == [None] and edge["new_pos"] == ix["pos"]
    both = U.write_plan([bad], ix, [(0, cb, 10), (0, 2 * cb - 5, 10)], [src[:10], src[:10]])       # ... the tail edge of the second request
    assert both["status"] == [want] and both["req_status"] == [want, want]
    whole = U.write_plan([bad], ix, [(0, 2 * cb - 1, cb + 2)], [src[:cb + 2]])                     # wholly covered: never looked at
    assert whole["status"] == [O.OK]
    assert O.frame_decode(whole["streams"][0]) == raw[:2 * cb - 1] + src[:cb + 2] + raw[3 * cb + 1:]
    elsewhere = U.write_plan([bad], ix, [(0, 5, 10)], [src[:10]])                                  # untouched: copied as it is
    assert elsewhere["status"] == [O.OK] and bad[ix["pos"][2]:ix["pos"][3]] in elsewhere["streams"][0]


def test_rows_that_point_at_one_header_twice_are_refused(named):
    names, streams, ix = named
    b = names.index("uniform_5")
    f0 = ix["first"][b]
    pos = list(ix["pos"])
    pos[f0 + 2] = pos[f0 + 1]                                           # row 2 claims row 1's header; both are raw chunks of 65536 bytes there?
    B = R.B
    got = U.write_plan(streams, {**ix, "pos": pos}, [(b, B + 5, 2 * B)], [bytes(2 * B)])
    assert got["status"][b] == O.ERR_BAD_ARG and got["streams"][b] is None
    assert U.write_plan(streams, ix, [(b, B + 5, 2 * B)], [bytes(2 * B)])["status"][b] == O.OK


# ---- the planning header on the CPU, under sanitizers ------------------------------------------------------------------------------------------
def test_planning_header_under_sanitizers_matches_the_model(named, tmp_path):
    names, streams, ix = named
    ns = len(streams)
    rng = np.random.default_rng(11)
    sound = U.sound_lists(streams, ix)
    u5 = names.index("uniform_5")
    B = R.B
    lists = [sound,
             [(b, off, ln) for b, s in enumerate(streams) for lst in U.row_requests(s)[:3] for off, ln in lst],      # unsorted within a stream: overlaps, order
             [(u5, 10, 5), (u5, 12, 5), (u5, 30, 5), (u5, 20, 5), (u5, B - 1, 2), (u5, B + 1, 10), (u5, B + 11, 2 * B), (u5, 5 * B, 1),   # overlapping, out of
              (u5, 4 * B + 776, 1), (u5, 4 * B + 777, 0), (u5, 4 * B + 777, 1), (u5, U.U64, 2)],                                         # order, past the end, one chunk, a shared edge
             [(u5, 0, 5), (ns, 0, 1), (u5 - 1, 0, 1), (u5, 9, 1), (0xFFFFFFFF, 0, 0)],                               # streams out of order and beyond
             [(int(v) % (ns + 2), int(o) % 200000, int(n) % 70000) for v, o, n in rng.integers(0, 1 << 40, (300, 3))],   # a list filled with anything
             sorted((int(v) % ns, int(o) % 200000, int(n) % 3000) for v, o, n in rng.integers(0, 1 << 40, (300, 3)))]
    cases = [(ix, lst) for lst in lists] + [(bad, lst) for bad in U.unsound_indexes(ix, streams, rng) for lst in (sound, lists[5])]
    path = str(tmp_path / "cases.bin")
    U.write_cases(path, streams, cases)
    exe = str(tmp_path / "frame_update_plan_check")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host",
                    "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "abi", "frame_update_plan_check.hip"), "-o", exe,
                    "-Wl,-rpath,/opt/rocm/lib"], check=True)
    env = {**os.environ, "ASAN_OPTIONS": "detect_leaks=1:abort_on_error=0", "UBSAN_OPTIONS": "print_stacktrace=1:halt_on_error=1"}
    run = subprocess.run([exe, path], capture_output=True, text=True, env=env)
    assert run.returncode == 0 and run.stderr == "", run.stderr[-3000:]      # the sanitizers are silent
    lines = run.stdout.splitlines()
    assert len(lines) == sum(len(reqs) for _, reqs in cases)
    at = refused = planned = 0
    for c, (index, reqs) in enumerate(cases):
        want = U.plan_lines(index, streams, reqs)
        for r, w in enumerate(want):
            assert lines[at] == w, (c, r, reqs[r])
            refused += c >= len(lists) and (not w.startswith("0 ") or not w.endswith(" 0"))
            planned += c >= len(lists) and w.startswith("0 ") and w.endswith(" 0")
            at += 1
    assert refused > 500 and planned > 100                              # both outcomes, on the unsound indexes
    # over the sound index the sorted list is planned whole, with no row refused
    assert all(line.startswith("0 ") and line.endswith(" 0") for line in lines[:len(sound)])

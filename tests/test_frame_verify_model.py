"""libsnappier_hip_frame_verify.so without a GPU: the declarations and their C# binding, argument rejection, the workspace arithmetic; the model
of both calls (frame_verify_model.py) against brute force -- every chunk decoded alone with the oracle's block decoder and CRC, every stream
decoded whole with its frame decoder, every single-bit flip of a short chunk, the planner's segments against a byte-by-byte labelling for all
good / bad patterns of 1 to 8 rows --, its recipes through the compose model (repair from a copy gives the stream back byte for byte, repair
from a replica at another chunking the same decoded bytes); and the rule header (csrc/frame_verify_device.h) itself, compiled for the CPU
under AddressSanitizer and UBSan into a stand-alone program (tests/abi/frame_verify_plan_check.hip) and run over cases the model writes out."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import frame_buffers_model as M
import frame_chunked_model as FC
import frame_compose_model as CM
import frame_index_model as X
import frame_verify_model as V
import oracle as O
from conftest import ROOT, read_testdata

NAMES = ["snp_frame_repair_plan_batch", "snp_frame_repair_plan_workspace", "snp_frame_verify_indexed_batch", "snp_frame_verify_indexed_workspace"]


def _lib():
    from snappier_amd import _native as N
    return N.frame_verify_lib()


_lib()                                                                  # every test here is about this library: without it the module does not load


@pytest.fixture(scope="module")
def html():
    return read_testdata("html")


# ---- the surface -----------------------------------------------------------------------------------------------------------------------------
def test_header_binding_and_library_declare_the_new_functions():
    from layouts import exported
    from snappier_amd import _native as N
    import snappier_amd as S
    assert N.frame_verify_declared_symbols() == NAMES
    others = set(N.declared_symbols())
    for name in N._EXTENSIONS:
        if name != "frame_verify":
            others |= set(N.declared_symbols(N._extension_header(name)))
            assert not exported(N._extension_path(name)) & set(NAMES)
    assert not set(NAMES) & others                                      # the other headers' surfaces are left as they are
    assert exported(N.FRAME_VERIFY_PATH) == set(NAMES) and not exported(N.PRODUCT_PATH) & set(NAMES)
    lib = _lib()
    assert lib.snp_frame_verify_indexed_batch.restype is C.c_int and len(lib.snp_frame_verify_indexed_batch.argtypes) == 21
    assert lib.snp_frame_repair_plan_batch.restype is C.c_int and len(lib.snp_frame_repair_plan_batch.argtypes) == 22
    assert S.VERIFY_NONE == V.NONE == (1 << 64) - 1 and S.VERIFY_SKIPPED == V.SKIPPED == -1
    text = open(os.path.join(ROOT, "include", "snappier_hip_frame_verify.h")).read()
    assert re.search(r"#define SNP_VERIFY_NONE 0xffffffffffffffffull", text) and re.search(r"#define SNP_VERIFY_SKIPPED \(-1\)", text)
    assert V.SKIPPED < O.OK                                             # outside the snp_status range: every status is >= 0


def test_csharp_binding_matches_the_extension_header():
    import test_csharp_signatures as T
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "snappier_hip_frame_verify.h")).read(), flags=re.S)
    protos = {}
    for m in re.finditer(r"([A-Za-z_][A-Za-z0-9_ ]*?[\s\*]+)(snp_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", text):
        params = [re.match(r"(.*?[\s\*])([A-Za-z_][A-Za-z0-9_]*)$", q.strip()).group(1) for q in m.group(3).split(",") if q.strip() not in ("", "void")]
        protos[m.group(2)] = (T.c_class(m.group(1)), [T.c_class(q) for q in params])
    cs = re.sub(r"//.*", "", open(os.path.join(ROOT, "csharp", "Snappier.Gpu", "NativeMethodsFrameVerify.cs")).read())
    assert 'const string Lib = "snappier_hip_frame_verify"' in cs
    imps = {}
    for m in re.finditer(r"\[DllImport\(Lib, CallingConvention = Cc\)\]\s*internal static extern ([A-Za-z\*]+) (snp_[a-z0-9_]+)\(([^)]*)\);", cs):
        params = [re.match(r"(.*?)\s+([A-Za-z_][A-Za-z0-9_]*)$", q.strip()).group(1) for q in m.group(3).split(",") if q.strip()]
        imps[m.group(2)] = (T.cs_class(m.group(1)), [T.cs_class(q) for q in params])
    assert set(protos) == set(imps) == set(NAMES)
    for name, (ret, params) in protos.items():
        cret, cparams = imps[name]
        assert T.compatible(ret, cret), (name, ret, cret)
        assert len(params) == len(cparams) and all(T.compatible(a, b) for a, b in zip(params, cparams)), (name, params, cparams)
    assert [len(protos[n][1]) for n in NAMES] == [22, 1, 21, 4]
    proj = open(os.path.join(ROOT, "csharp", "Snappier.Gpu", "Snappier.Gpu.csproj")).read()
    assert 'Include="../../snappier_amd/libsnappier_hip_frame_verify.so"' in proj


def test_workspaces_are_host_arithmetic_within_the_documented_bounds():
    ws, pws = _lib().snp_frame_verify_indexed_workspace, _lib().snp_frame_repair_plan_workspace
    assert ws(0, 1000, 4096, 1 << 20) == 0 and ws(1, 1 << 31, 4096, 1 << 20) == 0 and ws(1 << 31, 5, 4096, 1 << 20) == 0
    assert ws(1, 1000, 0, 1 << 20) == 0 and ws(1, 1000, 65537, 1 << 20) == 0
    for ns in (1, 2, 1000, 163840):
        for ne in (0, 1, 33, 5000, (1 << 20) + 1, (1 << 31) - 1):
            for slot in (1, 16, 17, 4096, 65536):
                for cap in (0, 15, slot, 1 << 20, 256 << 20, (1 << 64) - 1):
                    size = ws(ns, ne, slot, cap)
                    stride, per, _ = V.rounds_of(slot, cap, ne)
                    scratch = per * stride
                    assert scratch <= cap and size % 256 == 0 and ws(ns + 1, ne, slot, cap) >= size
                    assert 46 * ne + 44 * ns + scratch <= size <= 46 * ne + 44 * ns + scratch + 17 * 256
    assert pws(0) == 0 and pws(1 << 31) == 0
    for nout in (1, 2, 1000, 163840, (1 << 31) - 1):
        assert pws(nout) % 256 == 0 and 44 * nout <= pws(nout) <= 44 * nout + 8 * nout // 1024 + 8 * 256 + 64


def test_batch_calls_reject_bad_arguments_without_a_device():
    call = _lib().snp_frame_verify_indexed_batch
    fake = C.c_void_p(64)                                               # (never dereferenced: the arguments are refused first)

    def args(ns=1, ne=4, slot=4096, cap=1 << 20, null=(), ctx=fake, result=fake):
        # in, in_off, in_len | idx_first, idx_start, idx_pos, idx_total, idx_tail | row_status, status, nbad, first_bad, bad_bytes, flags, d_work
        p = [None if i in null else fake for i in range(15)]
        return (ctx, *p[:3], ns, *p[3:8], ne, slot, cap, *p[8:15], result)

    assert call(*args(ctx=None)) == O.ERR_BAD_ARG
    assert call(*args(result=None)) == O.ERR_BAD_ARG
    assert call(*args(ns=0, ne=0, null=range(15), result=None)) == O.ERR_BAD_ARG
    assert call(*args(slot=0)) == O.ERR_BAD_ARG and call(*args(slot=65537)) == O.ERR_BAD_ARG
    assert call(*args(ns=0, ne=0, slot=0, null=range(15))) == O.ERR_BAD_ARG
    assert call(*args(ns=1 << 31)) == O.ERR_BAD_ARG
    assert call(*args(ne=1 << 31)) == O.ERR_BAD_ARG
    for i in range(15):                                                 # any one null among the arrays of a full call
        assert call(*args(null=(i,))) == O.ERR_BAD_ARG, i

    plan = _lib().snp_frame_repair_plan_batch

    def pargs(ne=4, ns=1, nrep=1, nout=1, ms=4, null=(), ctx=fake, result=fake):
        # idx_first, idx_start, idx_total, idx_tail | row_status, rep_total, rep_tail | rp_stream, rp_replica | seg_first, seg_stream, seg_off,
        # seg_len, plan_status, d_work
        p = [None if i in null else fake for i in range(15)]
        return (ctx, *p[:4], ne, ns, *p[4:7], nrep, *p[7:9], nout, ms, *p[9:15], result)

    assert plan(*pargs(ctx=None)) == O.ERR_BAD_ARG
    assert plan(*pargs(result=None)) == O.ERR_BAD_ARG
    assert plan(*pargs(nout=0, null=range(15), result=None)) == O.ERR_BAD_ARG
    for big in ("ne", "ns", "nrep", "nout"):
        assert plan(*pargs(**{big: 1 << 31})) == O.ERR_BAD_ARG, big
    for i in range(15):
        assert plan(*pargs(null=(i,))) == O.ERR_BAD_ARG, i


# ---- the verify model against brute force ------------------------------------------------------------------------------------------------------
def brute_force_rows(s: bytes):
    """Every data chunk of a stream whose headers walk, decoded ALONE with the oracle's block decoder and CRC: -> [status per data chunk]."""
    rows, _, tail = M.serial_walk(s, 1 << 62)
    assert tail == O.OK
    return [M.chunk_status(s, r) for r in rows]


def whole_status(s: bytes) -> int:
    try:
        O.frame_decode(s)
        return O.OK
    except O.OracleError as e:
        return e.status


def check_against_brute_force(streams):
    """Guarantee (a) over an index of the streams as they are: the model's row_status is the chunks' own status, and a stream is OK exactly
    when the oracle decodes it whole."""
    ix = X.build_index(streams)
    got = V.verify_plan(streams, ix)
    at = 0
    for b, s in enumerate(streams):
        if ix["tail"][b] != O.OK:
            assert got["status"][b] == ix["tail"][b] and whole_status(s) != O.OK
            continue
        rows = brute_force_rows(s)
        assert got["row_status"][at:at + len(rows)] == rows, b
        assert (got["status"][b] == O.OK) == (whole_status(s) == O.OK) == all(r == O.OK for r in rows)
        if got["status"][b] != O.OK:
            assert got["status"][b] == whole_status(s)                  # the first bad chunk in stream order is where the whole decode stops
            assert got["first_bad"][b] == at + [i for i, r in enumerate(rows) if r != O.OK][0]
        assert got["nbad"][b] == sum(1 for r in rows if r != O.OK)
        at += len(rows)
    assert at == V.nentries_of(ix)
    return got


@pytest.mark.parametrize("variant", [O.HASH_CRC32C, O.HASH_MUL])
def test_model_against_brute_force_on_sound_streams(html, variant):
    streams = list(V.shape_streams(html, variant).values()) + V.seven_by_three(html)
    got = check_against_brute_force(streams)
    assert got["status"] == [O.OK] * len(streams) and got["result"][1] == 0 and got["result"][4] == 65536
    assert got["result"][2] == sum(len(O.frame_decode(s)) for s in streams)


def test_every_single_bit_flip_of_a_short_chunk_is_a_bad_row(html):
    """CRC-32C catches every single-bit error in body or CRC; the row check or the decoder catches the header.  Every flip over an
    uncompressed chunk is a bad row, none left out.  In a COMPRESSED chunk the body is elements, not data, and the reference's decoder itself
    takes some flipped bodies for the same bytes (a literal whose tag says more than the block holds is cut at the declared length): those
    flips -- V.same_bytes_flips, from the oracle alone -- are no damage to anything the CRC covers, and every other flip is a bad row."""
    for comp in (False, True):
        s, ix, lo, n = V.flip_stream(html, comp)
        harmless = V.same_bytes_flips(s, lo, n)
        assert not harmless if not comp else len(harmless) < 8
        whole = O.frame_decode(s)
        seen = set()
        for at in range(lo, lo + n):
            for bit in range(8):
                bad = V.flip(s, at, bit)
                got = V.verify_plan([bad], ix)                          # the index is the caller's: it survives the damage
                if (at, bit) in harmless:
                    assert got["status"] == [O.OK] and O.frame_decode(bad) == whole
                    continue
                assert got["row_status"][1] != O.OK and got["status"] != [O.OK], (at, bit)
                assert got["row_status"][0] == got["row_status"][2] == O.OK and got["first_bad"] == [1] and got["nbad"] == [1]
                assert whole_status(bad) != O.OK or O.frame_decode(bad) != whole     # (a type byte turned skippable drops the chunk: only the index notices)
                seen.add(got["row_status"][1])
        assert {O.ERR_BAD_ARG, O.ERR_CRC_MISMATCH} <= seen


def test_damage_and_unsound_indexes_in_the_model(html):
    streams = V.seven_by_three(html)
    ix = X.build_index(streams)
    pos = ix["pos"]
    for rows in ([0], [20], [6, 7], [0, 20], list(range(21))):
        bad = list(streams)
        for r in rows:
            b = r // 7
            bad[b] = V.flip(bad[b], pos[r] + 9, 3)                      # a body byte
        got = V.verify_plan(bad, ix)
        assert [i for i, v in enumerate(got["row_status"]) if v != O.OK] == rows
        assert got["result"][1] == len(rows) and got["result"][0] == 21
        check_against_brute_force(bad)
    # a truncated last chunk; a damaged identifier; a broken idx_tail skips its stream alone
    cut = [streams[0], streams[1][:-1], streams[2]]
    got = V.verify_plan(cut, ix)
    assert got["row_status"][13] == O.ERR_BAD_ARG and got["status"] == [O.OK, O.ERR_BAD_ARG, O.OK]
    got = V.verify_plan([V.flip(streams[0], 4, 0)] + streams[1:], ix)
    assert got["flags"] == [1, 0, 0] and got["status"] == [O.OK] * 3
    k = {key: list(v) for key, v in ix.items()}
    k["tail"][1] = O.ERR_CRC_MISMATCH
    got = V.verify_plan(streams, k)
    assert got["status"] == [O.OK, O.ERR_CRC_MISMATCH, O.OK] and got["row_status"][7:14] == [V.SKIPPED] * 7 and got["result"][0] == 14
    assert got["first_bad"][1] == V.NONE and got["nbad"][1] == 0
    # the sizing call and a slot below the largest row
    sizing = V.verify_plan(streams, ix, 65536, 0)
    assert sizing["row_status"] == [O.ERR_OUTPUT_TOO_SMALL] * 21 and sizing["result"][4] == 2500 and sizing["result"][5] == 21 and sizing["result"][6] == 0
    small = V.verify_plan(streams, ix, 1000, 1 << 20)
    assert sorted(set(small["row_status"])) == [O.OK, O.ERR_OUTPUT_TOO_SMALL] and small["result"][5] == sum(1 for v in small["row_status"] if v)
    for per, rounds in ((1, 21), (2, 11), (3, 7), (7, 3), (8, 3), (21, 1), (50, 1)):
        assert V.verify_plan(streams, ix, 2512, per * 2512)["result"][6] == rounds and V.rounds_of(2500, per * 2512, 21)[1] == min(per, 21)


# ---- the planner model against brute force -------------------------------------------------------------------------------------------------------
def labels_of(segs, total):
    """Byte by byte: the source of every decoded byte the segments cover, in order."""
    out = []
    for src, off, ln in segs:
        assert off == len(out) and ln > 0
        out += [src] * ln
    assert len(out) == total
    return out


def test_planner_merges_runs_for_every_pattern_of_1_to_8_rows():
    lens = [5, 0, 3, 7, 0, 0, 2, 9]
    for n in range(1, 9):
        start = [sum(lens[:i]) for i in range(n)]
        total = sum(lens[:n])
        ix = dict(first=[0, n], start=start, pos=[0] * n, total=[total], tail=[O.OK])
        for mask in range(1 << n):
            rs = [O.OK if mask >> i & 1 else (O.ERR_CRC_MISMATCH, V.SKIPPED, O.ERR_BAD_ARG, O.ERR_OUTPUT_TOO_SMALL)[i % 4] for i in range(n)]
            got = V.repair_plan(ix, 1, rs, [total], [O.OK], [0], [0])
            segs = list(zip(got["segs"]["stream"], got["segs"]["off"], got["segs"]["len"]))
            want = [0 if rs[i] == O.OK else 1 for i in range(n) for _ in range(lens[i])]
            assert labels_of(segs, total) == want
            assert all(a[0] != b[0] for a, b in zip(segs, segs[1:]))   # maximal runs: neighbours differ
            assert got["result"] == [len(segs), 1, want.count(1), want.count(0)] and got["plan_status"] == [O.OK]
    clean = V.repair_plan(dict(first=[0, 3], start=[0, 4, 9], pos=[0] * 3, total=[20], tail=[O.OK]), 1, [O.OK] * 3, [20], [O.OK], [0], [0])
    assert clean["segs"] == dict(first=[0, 1], stream=[0], off=[0], len=[20])                       # no bad row: one segment


def test_planner_rejections_and_admission():
    ix = dict(first=[0, 2, 2, 5], start=[0, 10, 0, 6, 9], pos=[0] * 5, total=[30, 0, 12], tail=[O.OK, O.OK, O.OK])
    rs = [O.OK, O.ERR_CRC_MISMATCH, O.ERR_CRC_MISMATCH, O.OK, O.ERR_BAD_ARG]
    rep_total, rep_tail = [30, 0, 12, 12, 13], [O.OK, O.OK, O.OK, O.ERR_TRUNCATED_STREAM, O.OK]
    free = V.repair_plan(ix, 3, rs, rep_total, rep_tail, [0, 1, 2], [0, 1, 2])
    assert free["plan_status"] == [O.OK] * 3 and free["segs"]["first"] == [0, 2, 2, 5] and free["segs"]["stream"] == [0, 3, 5, 2, 5]
    assert free["result"] == [5, 3, 20 + 6 + 3, 10 + 3]
    for s, t in ((3, 0), (0, 5), (2, 3), (2, 4), (0, 2)):               # out of range twice, a replica's tail, totals that differ twice
        assert V.repair_plan(ix, 3, rs, rep_total, rep_tail, [s], [t])["plan_status"] == [O.ERR_BAD_ARG]
    for tail in (O.ERR_CRC_MISMATCH, 77, -1):
        k = dict(ix, tail=[tail, O.OK, O.OK])
        assert V.repair_plan(k, 3, rs, rep_total, rep_tail, [0, 2], [0, 2])["plan_status"] == [O.ERR_BAD_ARG, O.OK]
    k = dict(ix, first=[3, 2, 2, 5])
    assert V.repair_plan(k, 3, rs, rep_total, rep_tail, [0], [0])["plan_status"] == [O.ERR_BAD_ARG]
    for ms, want in ((0, [1, 1, 1]), (1, [1, 1, 1]), (2, [0, 0, 1]), (4, [0, 0, 1]), (5, [0, 0, 0]), (6, [0, 0, 0])):
        got = V.repair_plan(ix, 3, rs, rep_total, rep_tail, [0, 1, 2], [0, 1, 2], ms)
        assert [int(v == O.ERR_OUTPUT_TOO_SMALL) for v in got["plan_status"]] == want and got["result"][0] == 5
        assert got["segs"]["first"][-1] == len(got["segs"]["stream"]) <= ms
    # the same stream in two pairs, against two replicas
    twice = V.repair_plan(ix, 3, rs, rep_total, rep_tail, [2, 2], [2, 2])
    assert twice["segs"]["stream"] == [5, 2, 5] * 2


# ---- through the compose model: guarantees (c) and (d) ----------------------------------------------------------------------------------------------
def repaired(streams, ix, reps, rep_ix, damaged_streams, cb=65536):
    got = V.verify_plan(damaged_streams, ix)
    pairs = [b for b, st in enumerate(got["status"]) if st != O.OK]
    plan = V.repair_plan(ix, len(streams), got["row_status"], rep_ix["total"], rep_ix["tail"], pairs, pairs)
    assert plan["plan_status"] == [O.OK] * len(pairs)
    src, six = V.joined(damaged_streams, ix, reps, rep_ix)
    back = CM.compose_plan(src, six, plan["segs"], cb)
    assert back["status"] == [O.OK] * len(pairs)
    return pairs, back["streams"], plan


def test_repair_from_a_copy_gives_the_stream_back_byte_for_byte(html):
    streams = V.seven_by_three(html) + [V.shape_streams(html)["raw_chunks"]]
    ix = X.build_index(streams)
    for rows in ([3], [0, 6], [7, 8, 9, 10, 11, 12, 13], [20, 23], [2, 4, 16]):
        bad = list(streams)
        for r in rows:
            b = max(k for k in range(4) if ix["first"][k] <= r)
            bad[b] = V.flip(bad[b], ix["pos"][r] + 8 + (r % 3), r % 8)
        pairs, back, plan = repaired(streams, ix, streams, ix, bad)
        assert back == [streams[b] for b in pairs]                      # (c)
        assert plan["result"][2] == sum(X.row_end(ix, ix["first"][b + 1], ix["total"][b], r) - ix["start"][r]
                                        for r in rows for b in [max(k for k in range(4) if ix["first"][k] <= r)])
        assert V.verify_plan(back, X.build_index(back))["status"] == [O.OK] * len(pairs)


def test_repair_from_a_replica_at_another_chunking_decodes_to_the_same_bytes(html):
    raws = [html[:70000], html[70000:90000]]
    streams = [M.STREAM_ID + b"".join(FC.chunks_of(x, 4096, O.HASH_CRC32C)) for x in raws]
    reps = [M.STREAM_ID + b"".join(FC.chunks_of(x, 65536, O.HASH_CRC32C)) for x in raws]
    ix, rep_ix = X.build_index(streams), X.build_index(reps)
    bad = [V.flip(V.flip(streams[0], ix["pos"][2] + 20, 1), ix["pos"][9] + 30, 6), V.flip(streams[1], ix["pos"][ix["first"][1]] + 11, 0)]
    pairs, back, plan = repaired(streams, ix, reps, rep_ix, bad, cb=4096)
    assert pairs == [0, 1] and [O.frame_decode(s) for s in back] == raws                            # (d)
    assert plan["result"][2] == 3 * 4096 and V.verify_plan(back, X.build_index(back))["status"] == [O.OK, O.OK]
    # damage on both sides in the same range: the second verify says so
    rep_bad = [V.flip(reps[0], rep_ix["pos"][0] + 50, 2), reps[1]]
    got = V.verify_plan(bad, ix)
    plan = V.repair_plan(ix, 2, got["row_status"], rep_ix["total"], rep_ix["tail"], [0, 1], [0, 1])
    src, six = V.joined(bad, ix, rep_bad, rep_ix)
    back = CM.compose_plan(src, six, plan["segs"], 4096)
    again = V.verify_plan(back["streams"], X.build_index(back["streams"])) if back["status"] == [O.OK, O.OK] else None
    assert back["status"][0] != O.OK or again["status"][0] != O.OK      # never silent success


# ---- the rule header on the CPU ------------------------------------------------------------------------------------------------------------------
def test_device_header_under_sanitizers_against_the_model(html, tmp_path):
    rounds = [(1, 0, 0), (1, 15, 9), (1, 16, 9), (16, 16, 9), (17, 64, 9), (4096, 256 << 20, 2621440), (65536, 256 << 20, 163840),
              (65536, (1 << 64) - 1, (1 << 31) - 1), (65535, 65535, 7), (4000, 4000 * 21 + 500, 21), (2500, 2512 * 8, 21)]
    streams = V.seven_by_three(html) + [V.shape_streams(html)[k] for k in ("no_rows", "sizes", "skippable_between")]
    ix = X.build_index(streams)
    rng = np.random.default_rng(17)
    streams[1] = V.flip(streams[1], 4, 5)                               # an identifier that is none
    indexes = [(ix, 65536, 1 << 30), (ix, 65536, 0), (ix, 1000, 1 << 20), (ix, 2500, 2512 * 2), (ix, 1, 16)]
    indexes += [(k, 65536, 1 << 24) for k in V.unsound_indexes(ix, streams, rng).values()]
    for _ in range(30):                                                 # one word of a sound index replaced by another value near it, or by anything
        k = {key: list(v) for key, v in ix.items() if key != "result"}
        key = ("first", "start", "pos", "total", "tail")[int(rng.integers(0, 5))]
        i = int(rng.integers(0, len(k[key])))
        k[key][i] = int(rng.integers(0, 12)) if key == "tail" else max(0, k[key][i] + int(rng.integers(-3, 4))) if rng.integers(0, 2) else int(rng.integers(0, 1 << 62))
        indexes.append((k, int(rng.integers(1, 65537)), int(rng.integers(0, 1 << 22))))
    # the planner: numbers alone -- every mask of 6 rows, totals past 4 GiB, arrays filled with anything
    G = 1 << 32
    big = dict(first=[0, 3, 6], start=[0, 5 * G, 5 * G + 7, 0, G, 3 * G], total=[9 * G, 4 * G], tail=[O.OK, O.OK])
    plans = [(big, 2, [O.OK, O.ERR_CRC_MISMATCH, O.OK, V.SKIPPED, V.SKIPPED, O.OK], [9 * G, 4 * G, 4 * G + 1], [O.OK, O.OK, O.OK],
              [(0, 0), (1, 1), (1, 2), (1, 0), (2, 0), (0, 3), (0, 0)])]
    six = dict(first=[0, 6], start=[0, 5, 5, 8, 15, 15], total=[17], tail=[O.OK])
    plans += [(six, 1, [O.OK if mask >> i & 1 else O.ERR_BAD_OFFSET for i in range(6)], [17], [O.OK], [(0, 0)]) for mask in range(64)]
    for _ in range(40):
        pns, ne, nrep = int(rng.integers(1, 5)), int(rng.integers(0, 12)), int(rng.integers(0, 4))
        words = lambda n, hi: [int(v) for v in rng.integers(0, hi, n, dtype=np.uint64)]      # noqa: E731
        wild = rng.integers(0, 2)
        k = dict(first=words(pns + 1, 1 << 63) if wild else sorted(words(pns + 1, ne + 2)), start=words(ne, 1 << 63) if wild else sorted(words(ne, 50)),
                 total=words(pns, 60), tail=[int(v) for v in rng.integers(-2, 13, pns)] if wild else [O.OK] * pns)
        rs = [int(v) for v in rng.integers(-1, 3, ne)] if rng.integers(0, 2) else [int(v) - (1 << 31) for v in rng.integers(0, 1 << 32, ne, dtype=np.uint64)]
        rep_total = list(k["total"][:nrep]) + words(max(nrep - pns, 0), 60)
        plans.append((k, pns, rs, rep_total, [int(v) for v in rng.integers(0, 2, nrep)], [(int(rng.integers(0, pns + 1)), int(rng.integers(0, nrep + 1))) for _ in range(6)]))
    path = str(tmp_path / "cases.bin")
    V.write_cases(path, rounds, streams, indexes, plans)
    exe = str(tmp_path / "frame_verify_plan_check")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host",
                    "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "abi", "frame_verify_plan_check.hip"), "-o", exe,
                    "-Wl,-rpath,/opt/rocm/lib"], check=True)
    env = {**os.environ, "ASAN_OPTIONS": "detect_leaks=1:abort_on_error=0", "UBSAN_OPTIONS": "print_stacktrace=1:halt_on_error=1"}
    run = subprocess.run([exe, path], capture_output=True, text=True, env=env)
    assert run.returncode == 0 and run.stderr == "", run.stderr[-3000:]      # the sanitizers are silent
    lines = run.stdout.splitlines()
    assert lines[0].startswith("G ok ") and int(lines[0].split()[2]) == 4000
    want = V.check_lines(rounds, streams, indexes, plans)
    assert len(lines) == len(want) + 1
    for i, (got, exp) in enumerate(zip(lines[1:], want)):
        assert got == exp, (i, got[:300], exp[:300])
    # the cases reach what they are for: a sound index passes whole, unsound ones fail streams and rows and leave others standing
    sound = want[len(rounds)].split()[1:]
    assert set(sound) == {"0"} and want[len(rounds) + 1].split(" | ")[1].split()[1] == "0"
    verdicts = [w for w in want if w.startswith("S")]
    assert any(" 9:0:" in w and " 0:0:" in w for w in verdicts) and any(w.startswith("V") and " 9" in w and " 0" in w for w in want)
    assert sum(1 for w in want if w.startswith("P") and " 9 ;" in w) > 5 and sum(1 for w in want if w.startswith("P") and ":" in w) > 60

"""snp_frame_decode_range_batch (libsnappier_hip_frame_range.so) without a GPU: the declarations and their C# binding, the workspace arithmetic,
argument rejection, and the Python model of the contract (frame_range_model.py) against the oracle: the bytes of every window, the status of a
window that covers the stream against the whole-stream decode plan, corruption inside and outside the window, the strict tail rule, the window
that does not fit its capacity, and the in-order admission by each of the three bounds."""
import ctypes as C
import os
import re

import decode_layout_model as L
import frame_buffers_model as M
import frame_range_model as R
import oracle as O
from conftest import ROOT

NAMES = ["snp_frame_decode_range_batch", "snp_frame_decode_range_workspace"]
BIG = 1 << 62


def _lib():
    from snappier_amd import _native as N
    return N.frame_range_lib()


# ---- the surface -----------------------------------------------------------------------------------------------------------------------------
def test_header_and_binding_declare_the_new_functions():
    from snappier_amd import _native as N
    declared = N.frame_range_declared_symbols()
    assert declared == NAMES
    others = set(N.declared_symbols()) | set(N.buffers_declared_symbols()) | set(N.buffers_decompress_declared_symbols()) | \
        set(N.frame_buffers_declared_symbols()) | set(N.layout_declared_symbols())
    assert not set(declared) & others                                  # the other headers' surfaces are left as they are
    lib = _lib()
    assert lib.snp_frame_decode_range_batch.restype is C.c_int and len(lib.snp_frame_decode_range_batch.argtypes) == 17
    assert lib.snp_frame_decode_range_workspace.restype is C.c_uint64 and len(lib.snp_frame_decode_range_workspace.argtypes) == 4


def test_extension_library_exports_exactly_its_header():
    from layouts import exported
    from snappier_amd import _native as N

    ext = exported(N.FRAME_RANGE_PATH)
    assert ext == set(NAMES)
    for other in (N.PRODUCT_PATH, N.BUFFERS_PATH, N.BUFFERS_DECOMPRESS_PATH, N.FRAME_BUFFERS_PATH, N.LAYOUT_PATH):
        assert not exported(other) & ext


def test_workspace_function_is_host_arithmetic():
    from snappier_amd import _native as N
    ws = _lib().snp_frame_decode_range_workspace
    layout_ws = N.layout_lib().snp_frame_decode_layout_workspace
    assert ws(0, 0, 0, 0) == 0 and ws(0, 1000, 1000, 1 << 30) == 0      # nothing when there is no stream
    for ns in (1, 2, 255, 1024, 1025, 300000):
        for mc in (0, 1, 70000):
            for sp in (0, 1, 5000):
                for ec in (0, 1, 65536, 200001, 5 << 30):
                    w = ws(ns, mc, sp, ec)
                    assert w % 256 == 0
                    assert w >= layout_ws(ns, sp)                       # the span walk's share, and more
                    assert w >= ec and w >= layout_ws(ns, sp) + ec + mc * 41 + ns * 2 * 45
                    # monotone in each argument
                    assert ws(ns + 1, mc, sp, ec) >= w and ws(ns, mc + 1, sp, ec) >= w and ws(ns, mc, sp + 1, ec) >= w and ws(ns, mc, sp, ec + 1) >= w
    assert ws(1, 0, 0, 256) - ws(1, 0, 0, 0) == 256 and ws(1, 0, 0, 257) - ws(1, 0, 0, 0) == 512    # the scratch is a 256-byte piece like the others
    assert ws(0x7FFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF, 1 << 40) > 0xFFFFFFFF * 170 + (1 << 40)          # (64-bit arithmetic)


def test_batch_call_rejects_bad_arguments_without_a_device():
    lib = _lib()
    none = [None] * 3
    assert lib.snp_frame_decode_range_batch(None, *none, 0, None, None, 0, 0, 0, None, None, None, None, None, None, None) == O.ERR_BAD_ARG
    fake = C.c_void_p(64)                                               # (never dereferenced: the arguments are refused first)
    assert lib.snp_frame_decode_range_batch(fake, *none, 0, None, None, 0, 0, 0, None, None, None, None, None, None, None) == O.ERR_BAD_ARG   # no d_result
    assert lib.snp_frame_decode_range_batch(fake, *none, 1, None, None, 0, 0, 0, None, None, None, None, None, None, fake) == O.ERR_BAD_ARG   # streams, no arrays
    assert lib.snp_frame_decode_range_batch(fake, fake, fake, fake, 0x40000000, fake, fake, 0, 0, 0, fake, fake, fake, fake, fake, fake, fake) == O.ERR_BAD_ARG


def test_csharp_binding_matches_the_extension_header():
    import test_csharp_signatures as T
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "snappier_hip_frame_range.h")).read(), flags=re.S)
    protos = {}
    for m in re.finditer(r"([A-Za-z_][A-Za-z0-9_ ]*?[\s\*]+)(snp_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", text):
        params = [re.match(r"(.*?[\s\*])([A-Za-z_][A-Za-z0-9_]*)$", q.strip()).group(1) for q in m.group(3).split(",") if q.strip() not in ("", "void")]
        protos[m.group(2)] = (T.c_class(m.group(1)), [T.c_class(q) for q in params])
    cs = re.sub(r"//.*", "", open(os.path.join(ROOT, "csharp", "Snappier.Gpu", "NativeMethodsFrameRange.cs")).read())
    assert 'const string Lib = "snappier_hip_frame_range"' in cs
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
    assert 'Include="../../snappier_amd/libsnappier_hip_frame_range.so"' in proj


# ---- the model against the oracle ------------------------------------------------------------------------------------------------------------
def all_streams():
    extra = {"long_two_spans": R.long_stream_with_a_skippable_chunk_across_the_span_boundary()[0], "tiny_chunks": R.tiny_chunk_stream(1)[0],
             "big_chunk": R.big_chunk_stream()[0], "zero_length_chunks": R.zero_length_chunk_stream()[0], "uniform_5": R.uniform_stream(5, 2, 777)[0]}
    return {**L.stream_cases(), **L.corpus_streams(), **extra}


def plan_windows(s, wins, cap=None):
    """Every window of `wins` over the one stream s, as one batch with room for everything."""
    streams = [s] * len(wins)
    caps = [BIG if cap is None else cap] * len(wins)
    mc, sp, ec = R.needs(streams, wins, caps)
    return R.range_plan(streams, wins, caps, mc, sp, ec)


def test_bytes_of_every_window_equal_the_oracle_slice():
    checked = 0
    for name, s in all_streams().items():
        rows, total, tail, _ = R.walk(s)
        if M.verdict(s, rows, total, tail)[0] != O.OK:
            continue
        raw = O.frame_decode(s)
        assert len(raw) == total
        wins = R.windows(rows, total)
        status, out_len, data, result = plan_windows(s, wins)
        for (ro, rl), st, n, got in zip(wins, status, out_len, data):
            lo, hi = R.clip(total, ro, rl)
            assert st == O.OK and n == hi - lo and got == raw[lo:hi], (name, ro, rl)
            checked += 1
        assert result[1] == sum(out_len) and result[5] >= result[0]
    assert checked > 500


def test_a_window_over_the_whole_stream_has_the_status_of_the_whole_decode():
    streams = list(all_streams().values())
    names = list(all_streams())
    walks = [R.walk(s) for s in streams]
    spans = sum((len(s) + R.SPAN - 1) // R.SPAN for s in streams)
    caps = [w[1] for w in walks]                                        # cap = total exactly
    seen = set()
    for rl in (None, R.U64):
        ranges = [(0, w[1] if rl is None else rl) for w in walks]
        mc, sp, ec = R.needs(streams, ranges, caps)
        assert sp == spans and ec == 0                                  # no edge: every selected chunk is interior
        status, out_len, data, result = R.range_plan(streams, ranges, caps, mc, sp, ec)
        want_status, want_len, _, want_result, _ = M.decode_plan(streams, caps, sum(len(w[0]) for w in walks), spans)
        assert status == want_status.tolist() and out_len == want_len.tolist(), [n for n, a, b in zip(names, status, want_status) if a != b]
        assert result[1:4] == want_result[1:4]
        assert result[0] == result[5] == sum(1 for w in walks for r in w[0] if r[5] > 0)    # (an empty chunk is never selected)
        seen |= set(status)
    assert {O.OK, O.ERR_TRUNCATED_STREAM, O.ERR_CHUNK_TYPE, O.ERR_BAD_LENGTH, O.ERR_INCOMPLETE, O.ERR_CRC_MISMATCH} <= seen


def test_selection_interior_and_edges():
    s, raw = R.uniform_stream(5, 1, 1000)
    rows, total, tail, _ = R.walk(s)
    assert [r[5] for r in rows] == [R.B] * 4 + [1000] and total == 4 * R.B + 1000
    B = R.B
    # window -> (selected chunks, edges among them, decoded bytes of those edges)
    cases = {(0, 0): (0, 0, 0), (B, 0): (0, 0, 0), (B + 1, 0): (1, 1, B),   # an empty window strictly inside a chunk selects it, on a boundary none
             (0, B): (1, 0, 0), (B, 2 * B): (2, 0, 0), (B - 1, 2): (2, 2, 2 * B), (B, 1): (1, 1, B), (2 * B - 1, 1): (1, 1, B), (10, 20): (1, 1, B),
             (1, 4 * B): (5, 2, B + 1000), (B, 3 * B + 1): (4, 1, 1000), (B - 1, 3 * B + 1): (4, 1, B), (0, R.U64): (5, 0, 0),
             (total - 1, 5): (1, 1, 1000), (total, 5): (0, 0, 0)}
    for (ro, rl), (nsel, nedge, ebytes) in cases.items():
        sel, edges = R.select(rows, *R.clip(total, ro, rl))
        assert (len(sel), len(edges), sum(r[5] for r in edges)) == (nsel, nedge, ebytes), (ro, rl)
    # d_result: interior rows, edge bytes, selected chunks
    _, _, _, result = plan_windows(s, list(cases))
    assert result[0] == sum(a - b for a, b, _ in cases.values()) and result[5] == sum(a for a, _, _ in cases.values())
    assert result[4] == sum(e for _, _, e in cases.values())


def test_a_corrupt_chunk_is_noticed_iff_it_is_selected():
    for s in (R.uniform_stream(4, 5)[0], R.tiny_chunk_stream(2)[0], R.big_chunk_stream()[0]):
        rows, total, tail, _ = R.walk(s)
        full = [r for r in rows if r[5] > 0]
        for victim in (full[0], full[len(full) // 2], full[-1]):
            bad = R.corrupt_chunk(s, victim)
            assert R.walk(bad)[:3] == (rows, total, tail)               # the header walk does not see it
            want = M.chunk_status(bad, victim)
            assert want != O.OK
            wins = R.windows(rows, total)
            status, out_len, data, _ = plan_windows(bad, wins)
            good = plan_windows(s, wins)
            hit = miss = 0
            for k, (ro, rl) in enumerate(wins):
                sel, _ = R.select(rows, *R.clip(total, ro, rl))
                if victim in sel:
                    assert status[k] == want and out_len[k] == 0 and data[k] is None, (ro, rl)
                    hit += 1
                else:
                    assert status[k] == O.OK and data[k] == good[2][k], (ro, rl)
                    miss += 1
            assert hit > 3 and miss > 3
    # the first failing chunk in stream order wins: head edge, interior, tail edge
    s = R.uniform_stream(4, 6)[0]
    rows = R.walk(s)[0]
    bad_crc = s[:rows[1][1] - 4] + bytes([s[rows[1][1] - 4] ^ 1]) + s[rows[1][1] - 3:]   # chunk 1: its CRC field
    cut = rows[2][1] + rows[2][2] - 1
    both = R.corrupt_chunk(bad_crc, rows[2])
    assert M.chunk_status(both, R.walk(both)[0][1]) == O.ERR_CRC_MISMATCH
    st2 = M.chunk_status(both, R.walk(both)[0][2])
    assert cut and st2 != O.OK
    status = plan_windows(both, [(R.B + 5, 2 * R.B), (R.B, 2 * R.B), (2 * R.B, R.B), (2 * R.B + 1, 10), (0, R.B), (3 * R.B, 7)])[0]
    assert status == [O.ERR_CRC_MISMATCH, O.ERR_CRC_MISMATCH, st2, st2, O.OK, O.OK]


def test_a_damaged_tail_fails_every_window_the_strict_rule():
    cases = L.stream_cases()
    for name, err in (("cut_in_body", O.ERR_TRUNCATED_STREAM), ("cut_in_header_1", O.ERR_TRUNCATED_STREAM), ("type_02", O.ERR_CHUNK_TYPE),
                      ("bad_varint_after_good", O.ERR_BAD_LENGTH), ("over_bound", O.ERR_INCOMPLETE)):
        s = cases[name]
        rows, total, tail, _ = R.walk(s)
        assert tail == err and total == 5000
        wins = R.windows(rows, total)
        status, out_len, data, result = plan_windows(s, wins)
        assert status == [err] * len(wins) and out_len == [0] * len(wins) and result[1] == 0, name
    # a truncated stream of the project's own encoder: a window in the intact first chunk
    s = R.uniform_stream(3, 4)[0][:-100]
    assert plan_windows(s, [(10, 100), (0, R.B)])[0] == [O.ERR_TRUNCATED_STREAM] * 2
    # a failing selected chunk comes before the tail
    s = L.stream_cases()["cut_in_body"]
    rows = R.walk(s)[0]
    assert plan_windows(R.corrupt_chunk(s, rows[1]), [(0, 100), (700, 100)])[0] == [O.ERR_TRUNCATED_STREAM, O.ERR_CRC_MISMATCH]


def test_a_window_that_does_not_fit_its_capacity_decodes_nothing():
    s, raw = R.uniform_stream(3, 7)
    rows = R.walk(s)[0]
    ranges = [(5, 1000), (R.B - 10, R.B + 20), (0, R.U64), (100, 0)]
    fit = [1000, R.B + 20, 3 * R.B, 0]
    streams = [s] * 4
    mc, sp, ec = R.needs(streams, ranges, fit)
    assert (mc, ec) == (1 + 3, R.B + 2 * R.B + R.B)                     # (the empty window lies strictly inside chunk 0: an edge)
    status, out_len, data, result = R.range_plan(streams, ranges, fit, mc, sp, ec)
    assert status == [O.OK] * 4 and data == [raw[5:1005], raw[R.B - 10:2 * R.B + 10], raw, b""]
    for k in range(3):
        caps = list(fit)
        caps[k] -= 1
        st, ol, dt, res = R.range_plan(streams, ranges, caps, mc, sp, ec)
        assert st == [O.ERR_OUTPUT_TOO_SMALL if j == k else O.OK for j in range(4)] and ol[k] == 0
        assert [dt[j] for j in range(4) if j != k] == [data[j] for j in range(4) if j != k]    # that stream alone
        assert res[0] < result[0] or res[4] < result[4]                 # it takes no slot and no scratch
    # the tail error comes before the capacity; a corrupt chunk is not seen, because nothing is decoded
    cut = s[:-50]
    assert R.range_plan([cut], [(0, 1000)], [999], 8, 8, 1 << 20)[0] == [O.ERR_TRUNCATED_STREAM]
    bad = R.corrupt_chunk(s, rows[0])
    assert R.range_plan([bad], [(0, 1000)], [999], 8, 8, 1 << 20)[0] == [O.ERR_OUTPUT_TOO_SMALL]
    assert R.range_plan([bad], [(0, 1000)], [1000], 8, 8, 1 << 20)[0] == [O.ERR_CRC_MISMATCH]


def test_admission_is_in_stream_order_by_each_of_the_three_bounds():
    a, b, c = R.uniform_stream(3, 1)[0], R.tiny_chunk_stream(3)[0], R.uniform_stream(2, 2, 500)[0]
    long_s = R.long_stream_with_a_skippable_chunk_across_the_span_boundary()[0]
    streams = [a, b, b"", long_s, c, a, R.ID]
    ranges = [(10, 2 * R.B), (0, R.U64), (0, 5), (1_000_000, 300_000), (R.B - 1, 2), (0, 3 * R.B), (0, 1)]
    caps = [BIG] * len(streams)
    mc, sp, ec = R.needs(streams, ranges, caps)
    full = R.range_plan(streams, ranges, caps, mc, sp, ec)
    assert full[0] == [O.OK] * len(streams) and full[3][0] == mc and full[3][2] == sp and full[3][4] == ec and sp == 7
    assert R.range_plan(streams, ranges, caps, mc + 9, sp + 9, ec + 9)[:3] == full[:3]

    def first_rejected(plan):
        st = plan[0]
        f = next(i for i, x in enumerate(st) if x == O.ERR_OUTPUT_TOO_SMALL)
        assert st[f:] == [O.ERR_OUTPUT_TOO_SMALL] * (len(st) - f) and plan[1][f:] == [0] * (len(st) - f)
        assert plan[0][:f] == full[0][:f] and plan[2][:f] == full[2][:f]                 # earlier streams are what they were
        return f

    short = R.range_plan(streams, ranges, caps, mc - 1, sp, ec)
    assert first_rejected(short) == 5 and short[3][0] == mc and short[3][4] == ec         # the last stream with an interior chunk
    short = R.range_plan(streams, ranges, caps, mc, sp, ec - 1)
    assert first_rejected(short) == 4 and short[3][4] == ec                               # the last stream with an edge
    short = R.range_plan(streams, ranges, caps, mc, sp - 1, ec)
    assert first_rejected(short) == 6 and short[3][2] == sp and short[3][0] == mc         # the last stream with a span (it has no chunk)
    short = R.range_plan(streams, ranges, caps, mc, sp - 2, ec)
    assert first_rejected(short) == 5 and short[3][2] == sp and short[3][0] == mc - 3     # not walked: its chunks are not counted
    none = R.range_plan(streams, ranges, caps, 0, sp, 0)                                  # the sizing call: decodes nothing, says what is needed
    assert none[3][0] == mc and none[3][4] == ec and first_rejected(none) == 0
    assert R.range_plan(streams, ranges, caps, 0, 0, 0)[0] == [O.ERR_OUTPUT_TOO_SMALL] * len(streams)
    assert R.range_plan([b"", R.ID[:0]], [(0, 1)] * 2, [0, 0], 0, 0, 0)[0] == [O.OK, O.OK]   # empty streams need no span
    assert R.range_plan([], [], [], 0, 0, 0)[3] == [0] * 6


def test_the_model_does_not_depend_on_the_span_size():
    s, raw = R.tiny_chunk_stream(4, 60)
    rows, total, _, _ = R.walk(s)
    wins = R.windows(rows, total)
    streams = [s] * len(wins)
    want = plan_windows(s, wins)
    spans = len(wins) * ((len(s) + 699) // 700)
    got = R.range_plan(streams, wins, [BIG] * len(wins), want[3][0], spans, want[3][4], span=700, window=200)
    assert got[:3] == want[:3] and got[3][0] == want[3][0] and got[3][4:] == want[3][4:] and got[3][2] == spans
    assert all(d == raw[R.clip(total, *w)[0]:R.clip(total, *w)[1]] for d, w in zip(got[2], wins))

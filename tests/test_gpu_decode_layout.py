"""snp_decompress_layout_batch / snp_frame_decode_layout_batch (BlockCodec.decompress_layout / frame_decode_layout, decompress_to_memory /
frame_decode_to_memory): every output and d_result against the model (decode_layout_model.py) on the inputs the CPU tests use, guard words around
every output array; layout -> decode chained on one stream against snp_decompress_batch / snp_frame_decode_device and the oracle; admission by
arena_cap and max_spans; the to_memory round trips; graph capture; offsets past 4 GiB.  Needs an MI355X."""
import ctypes as C

import numpy as np
import pytest
import torch

import datagen
import decode_layout_model as L
import frame_buffers_helpers as H
import frame_buffers_model as M
import oracle as O
from conftest import CORPUS, read_testdata

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from snappier_amd import batch as SB, _native as N

B = 65536
GUARD = 16                 # guard elements on each side of every output array
CANARY = 0x5A


def dev(a, dtype=np.int64):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=dtype))).cuda()


def dev_u32(a):
    return torch.from_numpy(np.asarray(a, dtype=np.int64).astype(np.uint32).view(np.int32)).cuda()


class Guarded:
    """An output array between guard elements: the call gets the middle, the test checks the rims."""

    def __init__(self, n: int, dtype):
        self.n = n
        self.t = torch.empty(n + 2 * GUARD, dtype=dtype, device="cuda")
        self.t.view(torch.uint8).fill_(CANARY)
        self.mid = self.t[GUARD:GUARD + n]

    def ptr(self):
        return C.c_void_p(self.mid.data_ptr())                          # (valid for n == 0 too: nothing is written there)

    def read(self, unsigned_bits: int = 0):
        h = self.t.cpu().numpy()
        rim = np.concatenate([h[:GUARD], h[GUARD + self.n:]])
        assert (rim.view(np.uint8) == CANARY).all(), "a write outside an output array"
        mid = h[GUARD:GUARD + self.n].astype(np.int64)
        return (mid & ((1 << unsigned_bits) - 1) if unsigned_bits else mid).tolist()


def _p(t):
    return C.c_void_p(t.data_ptr())


def block_layout(cd, comp, in_off, in_len, align=1, arena_cap=L.UNBOUNDED):
    """snp_decompress_layout_batch called directly, every output guarded: -> the model's dict."""
    nb = len(in_off)
    LL = N.layout_lib()
    cd._bind()
    out_off, out_cap, declared = Guarded(nb, torch.int64), Guarded(nb, torch.int32), Guarded(nb, torch.int32)
    status, result = Guarded(nb, torch.int32), Guarded(4, torch.int64)
    work = Guarded(LL.snp_decompress_layout_workspace(nb), torch.uint8)
    d_off, d_len = dev(in_off), dev_u32(in_len)                         # (named: they must outlive the call)
    st = LL.snp_decompress_layout_batch(cd.ctx.handle, _p(comp), _p(d_off), _p(d_len), nb, align, arena_cap, out_off.ptr(),
                                        out_cap.ptr(), declared.ptr(), status.ptr(), work.ptr(), result.ptr())
    assert st == O.OK
    torch.cuda.synchronize()
    work.read()
    return {"out_off": out_off.read(), "out_cap": out_cap.read(32), "declared": declared.read(32), "status": status.read(), "result": result.read()}


def stream_layout(cd, framed, in_off, in_len, max_spans, align=1, arena_cap=L.UNBOUNDED):
    ns = len(in_off)
    LL = N.layout_lib()
    cd._bind()
    out_off, out_cap, decoded = Guarded(ns, torch.int64), Guarded(ns, torch.int64), Guarded(ns, torch.int64)
    nchunks, status, result = Guarded(ns, torch.int32), Guarded(ns, torch.int32), Guarded(5, torch.int64)
    work = Guarded(LL.snp_frame_decode_layout_workspace(ns, max_spans), torch.uint8)
    d_off, d_len = dev(in_off), dev(in_len)
    st = LL.snp_frame_decode_layout_batch(cd.ctx.handle, _p(framed), _p(d_off), _p(d_len), ns, max_spans, align, arena_cap,
                                          out_off.ptr(), out_cap.ptr(), decoded.ptr(), nchunks.ptr(), status.ptr(), work.ptr(), result.ptr())
    assert st == O.OK
    torch.cuda.synchronize()
    work.read()
    return {"out_off": out_off.read(), "out_cap": out_cap.read(), "decoded_len": decoded.read(), "nchunks": nchunks.read(32),
            "status": status.read(), "result": result.read()}


def spans_of(streams):
    return [(len(s) + L.SPAN - 1) // L.SPAN for s in streams]


def long_stream_with_a_skippable_chunk_across_the_span_boundary():
    """More than one span; a skippable chunk crosses byte 2^20 and is followed by another one, so span 1 is entered at a header that is no
    candidate (the resolver walks it on the spot)."""
    rnd = np.random.default_rng(3).integers(0, 256, 1_040_000, dtype=np.uint8).tobytes()
    html = read_testdata("html")
    s = O.frame_encode(rnd)
    assert len(s) < L.SPAN - 100
    s += M.chunk(0xFE, bytes(20000)) + M.chunk(0x80, b"x" * 100) + O.frame_encode(html * 12)[10:] + M.data_chunk(rnd[:50000], compressed=False)
    assert L.SPAN < len(s) < 2 * L.SPAN
    return s, rnd + html * 12 + rnd[:50000]


# ---- the outputs against the model -----------------------------------------------------------------------------------------------------------
def test_block_layout_equals_the_model_on_the_constructed_inputs():
    cd = SB.BlockCodec(0, O.HASH_CRC32C)
    cases = {**L.block_cases(), **L.corpus_blocks()}
    names = list(cases)
    order = np.random.default_rng(1).permutation(len(names))            # not-OK buffers in front of, between and after the OK ones
    bufs = [cases[names[i]] for i in order]
    comp, in_off, in_len = H.pack(bufs)
    items = [L.block_item(x) for x in bufs]
    assert {st for st, _ in items} == {O.OK, O.ERR_BAD_LENGTH, O.ERR_INCOMPLETE}
    need = L.block_layout(items, 1)["result"][0]
    for align, cap in ((1, L.UNBOUNDED), (1, need), (1, need - 1), (1, 0), (2, need // 2), (64, L.UNBOUNDED), (4096, need // 3),
                       (1 << 20, L.UNBOUNDED), (1 << 20, need), (1, (1 << 64) - 1)):
        got = block_layout(cd, comp, in_off, in_len, align, cap)
        assert got == L.block_layout(items, align, cap), (align, cap)
    # one buffer, and none (d_result is still written)
    assert block_layout(cd, comp, in_off[:1], in_len[:1]) == L.block_layout(items[:1])
    assert block_layout(cd, comp, [], [])["result"] == [0, 0, 0, 0]
    # more than one scan tile, every thread of the last workgroup partly idle
    small = [x for x in bufs if len(x) < 70000]
    many = [small[i % len(small)] for i in range(2500)]
    comp, in_off, in_len = H.pack(many)
    items = [L.block_item(x) for x in many]
    need = L.block_layout(items, 64)["result"][0]
    for cap in (L.UNBOUNDED, need * 2 // 3):
        assert block_layout(cd, comp, in_off, in_len, 64, cap) == L.block_layout(items, 64, cap)


def test_stream_layout_equals_the_model_on_the_constructed_inputs():
    cd = SB.BlockCodec(0, O.HASH_CRC32C)
    cases = {**L.stream_cases(), **L.corpus_streams()}
    long_s, _ = long_stream_with_a_skippable_chunk_across_the_span_boundary()
    names = list(cases)
    order = np.random.default_rng(2).permutation(len(names))
    streams = [cases[names[i]] for i in order]
    mid = len(streams) // 2
    streams.insert(mid, long_s)
    framed, in_off, in_len = H.pack(streams)
    items = [L.stream_item(s) for s in streams]
    assert {st for st, _, _ in items} == {O.OK, O.ERR_BAD_LENGTH, O.ERR_INCOMPLETE, O.ERR_TRUNCATED_STREAM, O.ERR_CHUNK_TYPE}
    sfirst = np.cumsum(spans_of(streams))
    total_spans = int(sfirst[-1])
    missed = {ms: L.missed_spans(streams, ms) for ms in (total_spans, total_spans + 7, int(sfirst[mid]) - 1, 0)}
    assert missed[total_spans] > 0                                      # the long stream's second span
    need = L.stream_layout(items, in_len, total_spans, 1)["result"][0]
    for max_spans, align, cap in ((total_spans, 1, L.UNBOUNDED), (total_spans, 1, need), (total_spans, 1, need - 1), (total_spans, 64, need // 2),
                                  (total_spans + 7, 4096, L.UNBOUNDED), (total_spans, 1 << 20, L.UNBOUNDED), (total_spans, 2, 0),
                                  (int(sfirst[mid]) - 1, 64, L.UNBOUNDED), (int(sfirst[mid]) - 1, 1, 1000), (0, 1, L.UNBOUNDED)):
        got = stream_layout(cd, framed, in_off, in_len, max_spans, align, cap)
        assert got == L.stream_layout(items, in_len, max_spans, align, cap, missed[max_spans]), (max_spans, align, cap)
    assert stream_layout(cd, framed, [], [], 0)["result"] == [0, 0, 0, 0, 0]
    # the long stream alone: result[4] counts its second span
    got = stream_layout(cd, framed, in_off[mid:mid + 1], in_len[mid:mid + 1], 2)
    assert got["result"][4] > 0 and got["status"] == [O.OK] and got["result"][2] == 2


# ---- layout -> decode on one stream, no host step between them -----------------------------------------------------------------------------------
def test_block_layout_chains_into_decompress_buffers():
    cd = SB.BlockCodec(0, O.HASH_CRC32C)
    html = read_testdata("html")
    corpus = b"".join(read_testdata(f) for f in CORPUS)
    raws = [html[:1], html[:100], corpus[:B - 1], corpus[7:7 + B], corpus[:B + 1], corpus[:3 * B + 1], (corpus * 3)[:9 << 20],
            bytes(np.random.default_rng(5).integers(0, 256, 100000, dtype=np.uint8)), b""]
    good = [O.compress(x, O.HASH_CRC32C if i % 2 else O.HASH_MUL) for i, x in enumerate(raws)]
    bc = L.block_cases()
    big = good[5]
    bad = [b"", bc["unterminated_2"], bc["six_bytes"], bc["over_bound_10"], bc["max_expansion_over_7"], bc["at_bound_299"],   # (the last: OK for the layout, fails in the decoder)
           big[:len(big) - 300], L.varint(len(raws[5]) + 5) + big[L.read_preamble(big)[2]:]]
    bufs = [bad[0], good[0], bad[1], good[1], good[2], bad[2], good[3], good[4], bad[3], good[5], good[6], bad[4], bad[5], good[7], bad[6],
            good[8], bad[7]]
    comp, in_off, in_len = H.pack(bufs)
    d_in_off, d_in_len = dev(in_off), dev_u32(in_len)
    items = [L.block_item(x) for x in bufs]
    want = L.block_layout(items, 64)
    arena = want["result"][0]
    out = torch.full((arena + 64,), CANARY, dtype=torch.uint8, device="cuda")
    BL = N.buffers_decompress_lib()
    frag_bound = want["result"][2]
    work = torch.empty(BL.snp_decompress_buffers_workspace(len(bufs), frag_bound), dtype=torch.uint8, device="cuda")
    lwork = torch.empty(N.layout_lib().snp_decompress_layout_workspace(len(bufs)), dtype=torch.uint8, device="cuda")
    # two enqueues, nothing read between them
    out_off, out_cap, declared, lstatus, lres = cd.decompress_layout(comp, d_in_off, d_in_len, align=64, arena_cap=arena, work=lwork)
    out_len, status, dres = cd.decompress_buffers(comp, d_in_off, d_in_len, out, out_off, out_cap, max_fragments=frag_bound, work=work)
    torch.cuda.synchronize()
    assert out_off.dtype == torch.int64 and out_cap.dtype == declared.dtype == lstatus.dtype == torch.int32 and lres.dtype == torch.int64
    h_off, h_cap = out_off.cpu().tolist(), (out_cap.cpu().numpy().astype(np.int64) & 0xFFFFFFFF).tolist()
    assert (h_off, h_cap, lstatus.cpu().tolist(), lres.cpu().tolist()) == (want["out_off"], want["out_cap"], want["status"], want["result"])
    assert lres.cpu().tolist()[1] == len(bufs)                          # everything placed
    assert int(dres[1]) >= 1                                            # the 9 MiB block was decoded by fragments
    # snp_decompress_batch given cap = declared, into an arena of its own
    ref = torch.full((arena + 64,), CANARY, dtype=torch.uint8, device="cuda")
    r_len, r_status = cd.decompress(comp, d_in_off, d_in_len, ref, out_off, declared)
    torch.cuda.synchronize()
    h, r = out.cpu().numpy(), ref.cpu().numpy()
    st, ol = status.cpu().tolist(), (out_len.cpu().numpy().astype(np.int64) & 0xFFFFFFFF).tolist()
    assert st == r_status.cpu().tolist() and ol == (r_len.cpu().numpy().astype(np.int64) & 0xFFFFFFFF).tolist()
    mask = np.ones(h.size, dtype=bool)
    n_ok = 0
    for b, x in enumerate(bufs):
        o, c = h_off[b], h_cap[b]
        mask[o:o + c] = False
        if st[b] == O.OK:
            n_ok += 1
            assert ol[b] == c and h[o:o + c].tobytes() == r[o:o + c].tobytes() == O.decompress(x), f"buffer {b}"
    assert n_ok == len(good) and (h[mask] == CANARY).all()
    assert st[bufs.index(bad[5])] != O.OK and st[bufs.index(bad[6])] != O.OK and st[bufs.index(bad[7])] != O.OK


def test_stream_layout_chains_into_frame_decode_buffers():
    cd = SB.BlockCodec(0, O.HASH_CRC32C)
    cases = L.stream_cases()
    long_s, long_raw = long_stream_with_a_skippable_chunk_across_the_span_boundary()
    html = read_testdata("html") * 8
    streams = list(cases.values()) + [long_s, O.frame_encode(html[:400000], O.HASH_MUL)]
    framed, in_off, in_len = H.pack(streams)
    d_in_off, d_in_len = dev(in_off), dev(in_len)
    items = [L.stream_item(s) for s in streams]
    spans = sum(spans_of(streams))
    want = L.stream_layout(items, in_len, spans, 4096, missed=L.missed_spans(streams, spans))
    arena, chunks = want["result"][0], want["result"][3]
    out = torch.full((arena + 64,), CANARY, dtype=torch.uint8, device="cuda")
    lwork = torch.empty(N.layout_lib().snp_frame_decode_layout_workspace(len(streams), spans), dtype=torch.uint8, device="cuda")
    dwork = torch.empty(N.frame_buffers_lib().snp_frame_decode_buffers_workspace(len(streams), chunks, spans), dtype=torch.uint8, device="cuda")
    out_off, out_cap, decoded, nchunks, lstatus, lres = cd.frame_decode_layout(framed, d_in_off, d_in_len, align=4096, arena_cap=arena,
                                                                                max_spans=spans, work=lwork)
    out_len, status, dres = cd.frame_decode_buffers(framed, d_in_off, d_in_len, out, out_off, out_cap, max_chunks=chunks, max_spans=spans, work=dwork)
    torch.cuda.synchronize()
    assert out_off.dtype == out_cap.dtype == decoded.dtype == lres.dtype == torch.int64 and nchunks.dtype == lstatus.dtype == torch.int32
    got = {"out_off": out_off.cpu().tolist(), "out_cap": out_cap.cpu().tolist(), "decoded_len": decoded.cpu().tolist(),
           "nchunks": nchunks.cpu().tolist(), "status": lstatus.cpu().tolist(), "result": lres.cpu().tolist()}
    assert got == want
    assert got["result"][4] > 0 and got["result"][1] == len(streams)
    assert dres.cpu().tolist()[0] == chunks and dres.cpu().tolist()[2] == spans     # the decode call's own d_result[0]: what the layout promised
    h = out.cpu().numpy()
    st, ol = status.cpu().tolist(), out_len.cpu().tolist()
    mask = np.ones(h.size, dtype=bool)
    seen = set()
    for b, x in enumerate(streams):
        o, c = got["out_off"][b], got["out_cap"][b]
        mask[o:o + c] = False
        s_st, s_len, s_bytes = H.single_decode(cd, x, max(c, 1))
        assert (st[b], ol[b]) == (s_st, s_len), f"stream {b}: batch {(st[b], ol[b])} single {(s_st, s_len)}"
        assert (st[b], ol[b]) == tuple(int(v) for v in M.verdict(x, *M.serial_walk(x, 1 << 64))), f"stream {b}"
        seen.add(st[b])
        if st[b] == O.OK:
            assert ol[b] == c and h[o:o + c].tobytes() == s_bytes == O.frame_decode(x), f"stream {b}"
    assert (h[mask] == CANARY).all()
    assert {O.OK, O.ERR_TRUNCATED_STREAM, O.ERR_CHUNK_TYPE, O.ERR_BAD_LENGTH, O.ERR_INCOMPLETE, O.ERR_CRC_MISMATCH} <= seen
    b = streams.index(long_s)
    assert h[got["out_off"][b]:got["out_off"][b] + ol[b]].tobytes() == long_raw
    # a tail error after good chunks: the chunks were given room, the tail is what the decode reports
    b = streams.index(cases["type_02"])
    assert got["out_cap"][b] == 5000 and st[b] == O.ERR_CHUNK_TYPE


# ---- admission ---------------------------------------------------------------------------------------------------------------------------------
def test_arena_cap_and_max_spans_admission_and_growing_them():
    cd = SB.BlockCodec(0, O.HASH_CRC32C)
    html = read_testdata("html") * 30
    rng = np.random.default_rng(9)
    raws = [html[o:o + n] for o, n in zip(rng.integers(0, 1000, 12).tolist(), [5, 70000, 0, 300000, 1, 65536, 2 << 20, 9, 100000, 3, 1 << 20, 77])]
    # blocks
    bufs = [O.compress(x) for x in raws]
    bufs.insert(4, b"\xff")                                              # a not-OK buffer keeps its own status behind f
    bufs.insert(9, b"")
    comp, in_off, in_len = H.pack(bufs)
    full = block_layout(cd, comp, in_off, in_len, 64)
    need = full["result"][0]
    assert full["result"][1] == len(bufs) and full["status"].count(O.OK) == len(raws)
    short = block_layout(cd, comp, in_off, in_len, 64, need // 2)
    f = short["result"][1]
    assert 0 < f < len(bufs) and short["result"][0] == need
    for b in range(len(bufs)):
        ok = full["status"][b] == O.OK
        assert short["status"][b] == (full["status"][b] if b < f or not ok else O.ERR_OUTPUT_TOO_SMALL)
        assert short["out_cap"][b] == (full["out_cap"][b] if b < f else 0) and short["declared"][b] == full["declared"][b]
    assert block_layout(cd, comp, in_off, in_len, 64, short["result"][0]) == full
    # framed streams: arena_cap, then max_spans
    streams = [O.frame_encode(x) for x in raws]
    streams.insert(4, L.stream_cases()["type_02"])
    framed, s_off, s_len = H.pack(streams)
    spans = sum(spans_of(streams))
    full = stream_layout(cd, framed, s_off, s_len, spans, 64)
    need = full["result"][0]
    assert full["result"][1:3] == [len(streams), spans] and full["result"][3] == sum(full["nchunks"])
    short = stream_layout(cd, framed, s_off, s_len, spans, 64, need // 2)
    f = short["result"][1]
    assert 0 < f < len(streams) and short["result"][0] == need
    for b in range(len(streams)):
        assert short["status"][b] == (full["status"][b] if b < f else O.ERR_OUTPUT_TOO_SMALL)
        assert short["out_cap"][b] == (full["out_cap"][b] if b < f else 0)
        assert (short["decoded_len"][b], short["nchunks"][b]) == (full["decoded_len"][b], full["nchunks"][b])
    assert stream_layout(cd, framed, s_off, s_len, spans, 64, short["result"][0]) == full
    few = stream_layout(cd, framed, s_off, s_len, spans - 1, 64)
    f = few["result"][1]
    assert few["result"][2] == spans and f == max(b for b in range(len(streams)) if len(streams[b]))   # the last stream that has a span
    for b in range(len(streams)):
        if b < f:
            assert all(few[k][b] == full[k][b] for k in ("out_off", "out_cap", "decoded_len", "nchunks", "status"))
        else:
            assert [few[k][b] for k in ("out_off", "out_cap", "decoded_len", "nchunks", "status")] == [0, 0, 0, 0, O.ERR_OUTPUT_TOO_SMALL]
    assert stream_layout(cd, framed, s_off, s_len, few["result"][2], 64) == full


# ---- to_memory: nothing but the compressed tensor and its table --------------------------------------------------------------------------------
def content(kind: str, n: int, seed: int) -> bytes:
    if kind == "corpus":
        files = [read_testdata(name) for name in CORPUS]
        out = bytearray()
        while len(out) < n:
            out += files[seed % len(files)]
            seed += 1
        return bytes(out[:n])
    if kind == "low":
        return b"".join(datagen.low_entropy_block(seed + b, B).tobytes() for b in range((n + B - 1) // B))[:n]
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes()


def ragged_raws(seed: int, count: int, top: int):
    rng = np.random.default_rng(seed)
    sizes = [0, 1, B - 1, B, B + 1, 3 * B + 1] + [int(np.exp(rng.uniform(0, np.log(top)))) for _ in range(count)]
    rng.shuffle(sizes)
    return [content(("corpus", "low", "random")[i % 3], n, seed + i) for i, n in enumerate(sizes)]


@pytest.mark.parametrize("seed,align", [(1, 1), (2, 256)])
def test_decompress_to_memory_round_trips_a_ragged_batch(seed, align):
    cd = SB.BlockCodec(0, O.HASH_CRC32C)
    raws = ragged_raws(seed, 20, 4 << 20) + [content("corpus", 9 << 20, seed)]
    bufs = [O.compress(x, O.HASH_CRC32C if i % 2 else O.HASH_MUL) for i, x in enumerate(raws)]
    bufs.insert(3, b"\x80")
    raws.insert(3, None)
    comp, in_off, in_len = H.pack(bufs)
    d_off, d_len = dev(in_off), dev_u32(in_len)
    out, out_off, out_len, status = cd.decompress_to_memory(comp, d_off, d_len, align=align)
    torch.cuda.synchronize()
    need = L.block_layout([L.block_item(x) for x in bufs], align)["result"][0]
    assert out.numel() == need and out.dtype == torch.uint8
    h, oo, ol, st = out.cpu().numpy(), out_off.cpu().tolist(), (out_len.cpu().numpy().astype(np.int64) & 0xFFFFFFFF).tolist(), status.cpu().tolist()
    for b, x in enumerate(raws):
        if x is None:
            assert st[b] == O.ERR_BAD_LENGTH and ol[b] == 0
        else:
            assert st[b] == O.OK and oo[b] % align == 0 and h[oo[b]:oo[b] + ol[b]].tobytes() == x, f"buffer {b}"
    with pytest.raises(ValueError):
        cd.decompress_to_memory(comp, d_off, d_len, align=align, max_bytes=need - 1)
    assert cd.decompress_to_memory(comp, d_off, d_len, align=align, max_bytes=need)[0].numel() == need
    empty = torch.empty(0, dtype=torch.int64, device="cuda")
    assert cd.decompress_to_memory(comp, empty, empty.to(torch.int32))[0].numel() == 0


@pytest.mark.parametrize("seed,align", [(3, 1), (4, 4096)])
def test_frame_decode_to_memory_round_trips_a_ragged_batch(seed, align):
    cd = SB.BlockCodec(0, O.HASH_CRC32C)
    raws = ragged_raws(seed, 14, 3 << 20) + [content("random", 5 << 19, seed)]      # (the last: three spans)
    streams = [O.frame_encode(x, O.HASH_CRC32C if i % 2 else O.HASH_MUL) for i, x in enumerate(raws)]
    streams.insert(2, L.stream_cases()["cut_in_body"])
    raws.insert(2, None)
    framed, in_off, in_len = H.pack(streams)
    d_off, d_len = dev(in_off), dev(in_len)
    out, out_off, out_len, status = cd.frame_decode_to_memory(framed, d_off, d_len, align=align)
    torch.cuda.synchronize()
    need = L.stream_layout([L.stream_item(s) for s in streams], in_len, 1 << 30, align)["result"][0]
    assert out.numel() == need
    h, oo, ol, st = out.cpu().numpy(), out_off.cpu().tolist(), out_len.cpu().tolist(), status.cpu().tolist()
    for b, x in enumerate(raws):
        if x is None:
            assert st[b] == O.ERR_TRUNCATED_STREAM and ol[b] == 0
        else:
            assert st[b] == O.OK and oo[b] % align == 0 and h[oo[b]:oo[b] + ol[b]].tobytes() == x, f"stream {b}"
    with pytest.raises(ValueError):
        cd.frame_decode_to_memory(framed, d_off, d_len, align=align, max_bytes=need - 1)
    # a table whose ranges overlap (every stream listed k times): more spans than the wrapper's first bound, so the layout is made again
    ns, spans = len(streams), sum(spans_of(streams))
    k = (framed.numel() >> 20) // (spans - ns) + 1
    assert k * spans > k * ns + (framed.numel() >> 20)
    t_off, t_len = dev(np.tile(in_off, k)), dev(np.tile(in_len, k))
    out3, off3, len3, st3 = cd.frame_decode_to_memory(framed, t_off, t_len, align=align)
    torch.cuda.synchronize()
    assert st3.cpu().tolist() == st * k and len3.cpu().tolist() == ol * k
    h3, o3 = out3.cpu().numpy(), off3.cpu().tolist()
    for b, x in enumerate(raws * k):
        if x is not None:
            assert h3[o3[b]:o3[b] + len(x)].tobytes() == x


# ---- graph capture -----------------------------------------------------------------------------------------------------------------------------
def test_layout_and_decode_replay_from_a_graph_on_new_inputs():
    cd = SB.BlockCodec(0, O.HASH_CRC32C)
    html = read_testdata("html") * 12
    alice = read_testdata("alice29.txt") * 8
    sizes = {"a": [5, 70000, 0, 300000, 65536, 1 << 20], "b": [200001, 1, 65537, 9, 600000, 0]}
    raws = {"a": [html[i:i + n] for i, n in enumerate(sizes["a"])], "b": [alice[3 * i:3 * i + n] for i, n in enumerate(sizes["b"])]}
    nb = 6
    stride = 1 << 21                                                    # every item's input slot: the same table of offsets for both batches
    in_off = dev(np.arange(nb) * stride + 1)
    arena = 4 << 20
    frag_bound, chunk_bound, span_bound = 64, 64, 2 * nb
    LL, BL, FL = N.layout_lib(), N.buffers_decompress_lib(), N.frame_buffers_lib()
    comp = torch.zeros(nb * stride + 64, dtype=torch.uint8, device="cuda")
    framed = torch.zeros(nb * stride + 64, dtype=torch.uint8, device="cuda")
    b_len = torch.zeros(nb, dtype=torch.int32, device="cuda")
    s_len = torch.zeros(nb, dtype=torch.int64, device="cuda")
    b_out = torch.zeros(arena, dtype=torch.uint8, device="cuda")
    s_out = torch.zeros(arena, dtype=torch.uint8, device="cuda")
    w1 = torch.empty(LL.snp_decompress_layout_workspace(nb), dtype=torch.uint8, device="cuda")
    w2 = torch.empty(BL.snp_decompress_buffers_workspace(nb, frag_bound), dtype=torch.uint8, device="cuda")
    w3 = torch.empty(LL.snp_frame_decode_layout_workspace(nb, span_bound), dtype=torch.uint8, device="cuda")
    w4 = torch.empty(FL.snp_frame_decode_buffers_workspace(nb, chunk_bound, span_bound), dtype=torch.uint8, device="cuda")

    def load(which):
        hc, hf = np.zeros(comp.numel(), dtype=np.uint8), np.zeros(framed.numel(), dtype=np.uint8)
        bl, sl = [], []
        for i, x in enumerate(raws[which]):
            c, f = O.compress(x), O.frame_encode(x)
            hc[i * stride + 1:i * stride + 1 + len(c)] = np.frombuffer(c, dtype=np.uint8)
            hf[i * stride + 1:i * stride + 1 + len(f)] = np.frombuffer(f, dtype=np.uint8)
            bl.append(len(c))
            sl.append(len(f))
        comp.copy_(torch.from_numpy(hc).cuda())
        framed.copy_(torch.from_numpy(hf).cuda())
        b_len.copy_(dev_u32(bl))
        s_len.copy_(dev(sl))

    def call():
        oo, oc, dec, lst, lres = cd.decompress_layout(comp, in_off, b_len, align=256, arena_cap=arena, work=w1)
        ol, st, _ = cd.decompress_buffers(comp, in_off, b_len, b_out, oo, oc, max_fragments=frag_bound, work=w2)
        so, sc, sd, snc, slst, slres = cd.frame_decode_layout(framed, in_off, s_len, align=256, arena_cap=arena, max_spans=span_bound, work=w3)
        sol, sst, _ = cd.frame_decode_buffers(framed, in_off, s_len, s_out, so, sc, max_chunks=chunk_bound, max_spans=span_bound, work=w4)
        return oo, oc, dec, lst, lres, ol, st, so, sc, sd, snc, slst, slres, sol, sst

    def snapshot(tensors):
        torch.cuda.synchronize()
        return [t.cpu().tolist() for t in tensors] + [b_out.cpu().numpy().copy(), s_out.cpu().numpy().copy()]

    load("b")
    eager_b = snapshot(call())                                          # (also the call before the capture)
    load("a")
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        eager_a = snapshot(call())
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        captured = call()
    for which, eager in (("b", eager_b), ("a", eager_a), ("b", eager_b)):
        load(which)
        b_out.zero_(); s_out.zero_()
        g.replay()
        got = snapshot(captured)
        for k in range(len(captured)):
            assert got[k] == eager[k], (which, k)
        oo, ol, st, so, sol, sst = got[0], got[5], got[6], got[7], got[13], got[14]
        assert st == [O.OK] * nb and sst == [O.OK] * nb
        for i, x in enumerate(raws[which]):
            assert ol[i] == sol[i] == len(x) and oo[i] % 256 == 0 and so[i] % 256 == 0
            assert got[-2][oo[i]:oo[i] + len(x)].tobytes() == x and got[-1][so[i]:so[i] + len(x)].tobytes() == x


# ---- offsets that need all 64 bits -------------------------------------------------------------------------------------------------------------
def test_block_layout_past_4_gib():
    """Layout only: ten preambles that declare about 1 GiB each.  Each buffer's table length is large enough for the expansion rule (the body is
    never read), and all the ranges overlap in one 64 MiB tensor."""
    cd = SB.BlockCodec(0, O.HASH_CRC32C)
    size = 64 << 20
    declared = [1 << 30, (1 << 30) + 12345, 1_200_000_000, 0xFFFFFFFF, 1 << 30, 999_999_999, 1_300_000_001, (1 << 30) - 1, 1 << 30, 1_111_111_111]
    h = np.zeros(size, dtype=np.uint8)
    in_off, in_len, heads = [], [], []
    for k, d in enumerate(declared):
        v = L.varint(d)
        o = 3 + 17 * k
        h[o:o + len(v)] = np.frombuffer(v, dtype=np.uint8)
        in_off.append(o)
        in_len.append(size - 1024 - o)
        heads.append(bytes(h[o:o + 8]))
    comp = torch.from_numpy(h).cuda()
    items = [L.block_item(x, n) for x, n in zip(heads, in_len)]
    assert [st for st, _ in items].count(O.OK) == 9 and items[3] == (O.ERR_INCOMPLETE, 0)
    for align, cap in ((1, L.UNBOUNDED), (1 << 20, L.UNBOUNDED), (4096, 5 << 30), (1, (1 << 32) - 1)):
        want = L.block_layout(items, align, cap)
        assert want["result"][0] > (9 << 30) and max(want["out_off"]) > (1 << 33)
        assert block_layout(cd, comp, in_off, in_len, align, cap) == want, (align, cap)

"""snp_frame_decode_range_batch (BlockCodec.frame_decode_range_buffers / frame_read_to_memory): every output and d_result against the model
(frame_range_model.py) on the inputs the CPU tests use, guard words around every output array and the workspace, a canary-filled arena; the
smallest shapes that can go wrong (1-5 chunks, tiny foreign chunks, a chunk above 65536 bytes as an edge, a window in the second span); equality
with frame_decode_buffers sliced on the host; admission by each bound; the capacity; corruption inside and outside the window; the read_to_memory
round trips; graph capture; an empty batch.  Needs an MI355X."""
import numpy as np
import pytest
import torch

import decode_layout_model as L
import frame_buffers_helpers as H
import frame_buffers_model as M
import frame_range_model as R
import oracle as O
from seekable_harness import CANARY, Guarded, dev_u64, range_call

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from snappier_amd import batch as SB, _native as N

B = 65536


def check(cd, streams, ranges, caps, mc=None, sp=None, ec=None):
    """The call against the model under the same bounds (default: what admits the whole batch)."""
    need = R.needs(streams, ranges, caps)
    mc, sp, ec = (need[0] if mc is None else mc), (need[1] if sp is None else sp), (need[2] if ec is None else ec)
    got = range_call(cd, streams, ranges, caps, mc, sp, ec)
    want = R.range_plan(streams, ranges, caps, mc, sp, ec)
    assert got[0] == want[0], [(b, g, w) for b, (g, w) in enumerate(zip(got[0], want[0])) if g != w]
    assert got[1] == want[1] and got[3] == want[3], (got[3], want[3])
    for b in range(len(streams)):
        assert got[2][b] == want[2][b], f"stream {b}: window {ranges[b]}"
    return got


def exact_caps(streams, ranges, slack=0):
    return [R.clip(R.walk(s)[1], *w)[1] - R.clip(R.walk(s)[1], *w)[0] + (slack and b % 3) for b, (s, w) in enumerate(zip(streams, ranges))]


def entries(named, every=1):
    """(stream, window) for every `every`-th window of each stream, the phase turning from stream to stream."""
    out = []
    for k, s in enumerate(named.values()):
        rows, total, _, _ = R.walk(s)
        out += [(s, w) for i, w in enumerate(R.windows(rows, total)) if (i + k) % every == 0]
    return out


# ---- against the model -----------------------------------------------------------------------------------------------------------------------
def test_range_equals_the_model_on_the_constructed_streams():
    cd = SB.BlockCodec(0, O.HASH_CRC32C)
    named = {**L.stream_cases(), "tiny": R.tiny_chunk_stream(1)[0], "zero": R.zero_length_chunk_stream()[0], "big": R.big_chunk_stream()[0]}
    pairs = entries(named)
    streams, ranges = [p[0] for p in pairs], [p[1] for p in pairs]
    got = check(cd, streams, ranges, exact_caps(streams, ranges, slack=1))
    assert {O.OK, O.ERR_TRUNCATED_STREAM, O.ERR_CHUNK_TYPE, O.ERR_BAD_LENGTH, O.ERR_INCOMPLETE, O.ERR_CRC_MISMATCH} <= set(got[0])
    assert got[3][4] > 0 and got[3][0] > 0 and got[3][5] > got[3][0]
    # looser bounds change nothing
    need = R.needs(streams, ranges, exact_caps(streams, ranges, slack=1))
    assert range_call(cd, streams, ranges, exact_caps(streams, ranges, slack=1), need[0] + 300, need[1] + 7, need[2] + 1000)[:3] == got[:3]


def test_range_equals_the_model_on_corpus_streams():
    cd = SB.BlockCodec(0, O.HASH_CRC32C)
    corpus = L.corpus_streams()
    named = {k: corpus[k] for k in list(corpus)[::3]}
    pairs = entries(named, every=3)
    streams, ranges = [p[0] for p in pairs], [p[1] for p in pairs]
    got = check(cd, streams, ranges, exact_caps(streams, ranges))
    assert got[0] == [O.OK] * len(streams)
    for s, w, d in zip(streams, ranges, got[2]):
        lo, hi = R.clip(R.walk(s)[1], *w)
        assert d == O.frame_decode(s)[lo:hi]


@pytest.mark.parametrize("nchunks", [1, 2, 3, 5])
def test_streams_of_a_few_whole_chunks(nchunks):
    cd = SB.BlockCodec(0, O.HASH_CRC32C if nchunks % 2 else O.HASH_MUL)
    last = {1: B, 2: 1, 3: B - 1, 5: 777}[nchunks]
    s, raw = R.uniform_stream(nchunks, nchunks, last)
    rows, total, _, _ = R.walk(s)
    wins = R.windows(rows, total)
    got = check(cd, [s] * len(wins), wins, exact_caps([s] * len(wins), wins))
    assert got[0] == [O.OK] * len(wins) and all(d == raw[R.clip(total, *w)[0]:R.clip(total, *w)[1]] for d, w in zip(got[2], wins))


def test_foreign_streams_tiny_chunks_and_a_chunk_above_65536_as_an_edge():
    cd = SB.BlockCodec(0, O.HASH_CRC32C)
    named = {f"tiny{k}": R.tiny_chunk_stream(10 + k, 25 + 30 * k)[0] for k in range(3)}
    pairs = entries(named)
    big, big_raw = R.big_chunk_stream()
    rows = R.walk(big)[0]
    assert rows[1][5] == 200_000 and rows[1][4] == 5000
    # the 200 000-byte chunk as the head edge, the tail edge, both ends at once, interior, and twice in one batch (the arena is in bytes)
    pairs += [(big, w) for w in ((5001, 250_000), (100, 5000), (100_000, 10), (5000, 200_000), (4999, 200_002), (204_999, 70_000), (0, R.U64))]
    streams, ranges = [p[0] for p in pairs], [p[1] for p in pairs]
    got = check(cd, streams, ranges, exact_caps(streams, ranges))
    assert got[0] == [O.OK] * len(streams) and got[3][4] > 4 * 200_000
    assert got[2][-7] == big_raw[5001:255_001] and got[2][-5] == big_raw[100_000:100_010]


def test_a_window_in_the_second_span_and_one_that_ends_at_its_first_chunk():
    cd = SB.BlockCodec(0, O.HASH_CRC32C)
    s, raw = R.long_stream_with_a_skippable_chunk_across_the_span_boundary()
    rows, total, _, missed = R.walk(s)
    first = next(r for r in rows if r[1] >= R.SPAN)                     # the first chunk whose header lies in span 1
    s1, d1 = first[4], first[5]
    assert missed == 1 and 0 < s1 < total
    wins = [(s1 + 10, 1000), (s1, d1), (s1 + d1, 3 * B), (s1 + 5, total), (s1 - 100, 100), (s1 - 100, 101), (s1 - 1, 2), (0, s1), (0, 10),
            (total - 10, 100), (s1 - B, 2 * B + 7), (0, R.U64)]
    streams = [s] * len(wins)
    got = check(cd, streams, wins, exact_caps(streams, wins))
    assert got[0] == [O.OK] * len(wins) and got[3][3] == len(wins) and got[3][2] == 2 * len(wins)
    assert all(d == raw[R.clip(total, *w)[0]:R.clip(total, *w)[1]] for d, w in zip(got[2], wins))


# ---- against the existing path ---------------------------------------------------------------------------------------------------------------
def test_bytes_equal_frame_decode_buffers_sliced_on_the_host():
    cd = SB.BlockCodec(0, O.HASH_CRC32C)
    rng = np.random.default_rng(21)
    raws = H.ragged(rng, 40, 400 * 1024) + [b"", b"x"]
    streams = [O.frame_encode(x, O.HASH_CRC32C if i % 2 else O.HASH_MUL) for i, x in enumerate(raws)]
    streams[7] = streams[7][:-3]                                        # truncated
    rows9 = R.walk(streams[9])[0]
    if rows9:
        streams[9] = R.corrupt_chunk(streams[9], rows9[len(rows9) // 2])
    totals = [R.walk(s)[1] for s in streams]
    h, f_off, f_len, f_st, _ = H.decode(cd, streams, totals)
    ranges = []
    for b, t in enumerate(totals):
        kind = b % 5
        lo = int(rng.integers(0, t + 1))
        ranges.append([(0, R.U64), (lo, int(rng.integers(0, t - lo + 2))), (lo // B * B, B), (lo, 4096), (0, t)][kind])
    caps = exact_caps(streams, ranges)
    st, ol, data, res = check(cd, streams, ranges, caps)
    n_ok = 0
    for b, (ro, rl) in enumerate(ranges):
        lo, hi = R.clip(totals[b], ro, rl)
        if (lo, hi) == (0, totals[b]):
            assert st[b] == f_st[b], f"stream {b}"                      # the window covers the stream: the status of the whole decode
        if st[b] == O.OK:
            assert f_st[b] == O.OK and data[b] == h[f_off[b] + lo:f_off[b] + hi].tobytes(), f"stream {b}"
            n_ok += 1
    assert n_ok >= 38 and st[7] == O.ERR_TRUNCATED_STREAM


# ---- admission, capacity, corruption -----------------------------------------------------------------------------------------------------------
def test_admission_by_each_bound_one_short_and_growing_to_d_result():
    cd = SB.BlockCodec(0, O.HASH_CRC32C)
    a, b, c = R.uniform_stream(3, 1)[0], R.tiny_chunk_stream(3)[0], R.uniform_stream(2, 2, 500)[0]
    long_s = R.long_stream_with_a_skippable_chunk_across_the_span_boundary()[0]
    streams = [a, b, b"", long_s, c, a, R.ID]
    ranges = [(10, 2 * B), (0, R.U64), (0, 5), (1_000_000, 300_000), (B - 1, 2), (0, 3 * B), (0, 1)]
    caps = exact_caps(streams, ranges)
    mc, sp, ec = R.needs(streams, ranges, caps)
    full = check(cd, streams, ranges, caps)
    assert full[0] == [O.OK] * len(streams) and (full[3][0], full[3][2], full[3][4]) == (mc, sp, ec)
    for bounds, first in (((mc - 1, sp, ec), 5), ((mc, sp - 1, ec), 6), ((mc, sp - 2, ec), 5), ((mc, sp, ec - 1), 4), ((0, sp, 0), 0)):
        short = check(cd, streams, ranges, caps, *bounds)
        assert short[0][first:] == [O.ERR_OUTPUT_TOO_SMALL] * (len(streams) - first) and short[1][first:] == [0] * (len(streams) - first)
        assert short[0][:first] == full[0][:first] and short[2][:first] == full[2][:first]     # earlier streams are bit-identical
        grown = range_call(cd, streams, ranges, caps, max(bounds[0], short[3][0]), max(bounds[1], short[3][2]), max(bounds[2], short[3][4]))
        if bounds[1] == sp:
            assert grown == full                                        # d_result[0], [2] and [4] are what the call needs
        else:
            assert grown[3][2] == sp                                    # spans first: the chunks of a stream that was not walked are not counted


def test_a_capacity_one_short_fails_that_stream_alone():
    cd = SB.BlockCodec(0, O.HASH_CRC32C)
    s, raw = R.uniform_stream(3, 7)
    ranges = [(5, 1000), (B - 10, B + 20), (0, R.U64), (100, 0), (2 * B, B)]
    streams = [s] * len(ranges)
    fit = exact_caps(streams, ranges)
    mc, sp, ec = R.needs(streams, ranges, fit)
    full = check(cd, streams, ranges, fit)
    assert full[0] == [O.OK] * 5
    for k in (0, 1, 2, 4):
        caps = list(fit)
        caps[k] -= 1
        got = check(cd, streams, ranges, caps, mc, sp, ec)              # (the arena check: nothing of stream k's range need be written, nothing outside is)
        assert got[0] == [O.ERR_OUTPUT_TOO_SMALL if j == k else O.OK for j in range(5)] and got[1][k] == 0
        assert [got[2][j] for j in range(5) if j != k] == [full[2][j] for j in range(5) if j != k]
    cut = s[:-50]
    assert check(cd, [cut, s], [(0, 1000), (0, 10)], [999, 10])[0] == [O.ERR_TRUNCATED_STREAM, O.OK]   # the tail comes before the capacity


def test_a_corrupt_chunk_inside_and_outside_the_window():
    cd = SB.BlockCodec(0, O.HASH_CRC32C)
    pairs = []
    for s in (R.uniform_stream(4, 5)[0], R.tiny_chunk_stream(2)[0], R.big_chunk_stream()[0]):
        rows, total, _, _ = R.walk(s)
        full = [r for r in rows if r[5] > 0]
        for victim in (full[0], full[len(full) // 2], full[-1]):
            bad = R.corrupt_chunk(s, victim)
            pairs += [(bad, w, victim in R.select(rows, *R.clip(total, *w))[0]) for w in R.windows(rows, total)[::2]]
    streams, ranges = [p[0] for p in pairs], [p[1] for p in pairs]
    got = check(cd, streams, ranges, exact_caps(streams, ranges))
    for (bad, w, hit), st in zip(pairs, got[0]):
        assert (st != O.OK) == hit, w
    assert sum(p[2] for p in pairs) > 20 and sum(not p[2] for p in pairs) > 20
    # two failing chunks: the first in stream order gives the status, whether it is an edge or interior
    s = R.uniform_stream(4, 6)[0]
    rows = R.walk(s)[0]
    p = rows[1][1] - 4
    both = R.corrupt_chunk(s[:p] + bytes([s[p] ^ 1]) + s[p + 1:], rows[2])
    st2 = M.chunk_status(both, R.walk(both)[0][2])
    wins = [(B + 5, 2 * B), (B, 2 * B), (2 * B, B), (2 * B + 1, 10), (0, B), (3 * B, 7), (B + 5, B + 5), (0, R.U64)]
    got = check(cd, [both] * len(wins), wins, exact_caps([both] * len(wins), wins))
    assert got[0] == [O.ERR_CRC_MISMATCH, O.ERR_CRC_MISMATCH, st2, st2, O.OK, O.OK, O.ERR_CRC_MISMATCH, O.ERR_CRC_MISMATCH]


# ---- the Python conveniences -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("align", [1, 256])
def test_frame_read_to_memory_round_trips(align):
    cd = SB.BlockCodec(0, O.HASH_CRC32C)
    rng = np.random.default_rng(align)
    raws = H.ragged(rng, 14, 300 * 1024) + [b""]
    streams = [O.frame_encode(x) for x in raws] + [L.stream_cases()["cut_in_body"]]
    raws.append(None)
    ranges = []
    for b, x in enumerate(raws):
        t = len(x) if x is not None else 5000
        lo = int(rng.integers(0, t + 1))
        ranges.append([(lo, int(rng.integers(0, t - lo + 2))), (0, R.U64 >> 1), (lo, 70000), (t + 3, 9)][b % 4])
    framed, in_off, in_len = H.pack(streams)
    tabs = [dev_u64(x) for x in (in_off, in_len, [r[0] for r in ranges], [r[1] for r in ranges])]
    out, out_off, out_len, status = cd.frame_read_to_memory(framed, *tabs, align=align)
    torch.cuda.synchronize()
    h, oo, ol, st = out.cpu().numpy(), out_off.cpu().tolist(), out_len.cpu().tolist(), status.cpu().tolist()
    slots = [(min(rl, 22 * len(s)) + align - 1) // align * align for s, (_, rl) in zip(streams, ranges)]
    assert out.numel() == sum(slots) and oo == [sum(slots[:b]) for b in range(len(slots))]
    for b, x in enumerate(raws):
        if x is None:
            assert st[b] == O.ERR_TRUNCATED_STREAM and ol[b] == 0
        else:
            lo, hi = R.clip(len(x), *ranges[b])
            assert st[b] == O.OK and ol[b] == hi - lo and oo[b] % align == 0 and h[oo[b]:oo[b] + ol[b]].tobytes() == x[lo:hi], f"stream {b}"
    with pytest.raises(ValueError):
        cd.frame_read_to_memory(framed, *tabs, align=align, max_bytes=sum(slots) - 1)
    assert cd.frame_read_to_memory(framed, *tabs, align=align, max_bytes=sum(slots))[0].numel() == sum(slots)
    empty = torch.empty(0, dtype=torch.int64, device="cuda")
    assert cd.frame_read_to_memory(framed, empty, empty, empty, empty)[0].numel() == 0
    # the defaults of frame_decode_range_buffers size the call themselves
    caps = exact_caps(streams, ranges)
    o_off, total = H.out_layout(caps)
    arena = torch.full((total,), CANARY, dtype=torch.uint8, device="cuda")
    ol2, st2, res = cd.frame_decode_range_buffers(framed, *tabs, arena, dev_u64(o_off), dev_u64(caps))
    torch.cuda.synchronize()
    assert ol2.cpu().tolist() == ol and st2.cpu().tolist() == st and res.cpu().tolist()[1] == sum(ol)
    a = arena.cpu().numpy()
    assert all(a[o:o + n].tobytes() == h[p:p + n].tobytes() for o, p, n in zip(o_off.tolist(), oo, ol))
    assert (H.outside_ranges(a, o_off, caps) == CANARY).all()


# ---- graph capture -----------------------------------------------------------------------------------------------------------------------------
def test_range_call_replays_from_a_graph_on_new_streams_and_windows():
    cd = SB.BlockCodec(0, O.HASH_CRC32C)
    batches = {"a": ([R.uniform_stream(3, 1)[0], R.tiny_chunk_stream(5)[0], b"", R.big_chunk_stream()[0], R.uniform_stream(2, 3, 9)[0]],
                     [(10, 2 * B), (100, 3000), (0, 5), (5001, 250_000), (B - 1, 2)]),
               "b": ([R.tiny_chunk_stream(6)[0], R.uniform_stream(5, 4, 100)[0], R.zero_length_chunk_stream()[0], L.stream_cases()["cut_in_body"], R.uniform_stream(1, 5)[0]],
                     [(0, R.U64), (B + 7, 3 * B), (650, 200), (0, 10), (B - 1, 9)])}
    ns, stride, cap = 5, 1 << 19, 300_000
    mc, sp, ec = 16, 2 * ns, 600_000                                    # bounds that hold both batches
    RL = N.frame_range_lib()
    framed = torch.zeros(ns * stride + 64, dtype=torch.uint8, device="cuda")
    in_off, out_off = dev_u64(np.arange(ns) * stride + 1), dev_u64(np.arange(ns) * cap)
    in_len, r_off, r_len = (torch.zeros(ns, dtype=torch.int64, device="cuda") for _ in range(3))
    out_cap = dev_u64([cap] * ns)
    out = torch.zeros(ns * cap, dtype=torch.uint8, device="cuda")
    work = torch.empty(RL.snp_frame_decode_range_workspace(ns, mc, sp, ec), dtype=torch.uint8, device="cuda")

    def load(which):
        streams, ranges = batches[which]
        h = np.zeros(framed.numel(), dtype=np.uint8)
        for i, x in enumerate(streams):
            h[i * stride + 1:i * stride + 1 + len(x)] = np.frombuffer(x, dtype=np.uint8)
        framed.copy_(torch.from_numpy(h).cuda())
        in_len.copy_(dev_u64([len(x) for x in streams]))
        r_off.copy_(dev_u64([r[0] for r in ranges]))
        r_len.copy_(dev_u64([r[1] for r in ranges]))

    def call():
        return cd.frame_decode_range_buffers(framed, in_off, in_len, r_off, r_len, out, out_off, out_cap, max_chunks=mc, max_spans=sp, edge_cap=ec, work=work)

    def verify(which, tensors):
        torch.cuda.synchronize()
        ol, st, res = (t.cpu().tolist() for t in tensors)
        streams, ranges = batches[which]
        want = R.range_plan(streams, ranges, [cap] * ns, mc, sp, ec)
        assert (st, ol, res) == (want[0], want[1], want[3]), which
        h = out.cpu().numpy()
        for b in range(ns):
            if st[b] == O.OK:
                assert h[b * cap:b * cap + ol[b]].tobytes() == want[2][b], (which, b)

    load("b")
    verify("b", call())                                                 # (also the call before the capture)
    load("a")
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        verify("a", call())
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        captured = call()
    for which in ("b", "a", "b"):
        load(which)
        out.zero_()
        g.replay()
        verify(which, captured)


def test_an_empty_batch_writes_a_zeroed_d_result():
    cd = SB.BlockCodec(0, O.HASH_CRC32C)
    assert range_call(cd, [], [], [], 0, 0, 0)[3] == [0] * 6
    assert range_call(cd, [], [], [], 100, 100, 1 << 20)[3] == [0] * 6
    RL = N.frame_range_lib()
    result = Guarded(6, torch.int64)
    assert RL.snp_frame_decode_range_batch(cd.ctx.handle, *[None] * 3, 0, None, None, 0, 0, 0, *[None] * 6, result.ptr()) == O.OK   # ctx and d_result only
    torch.cuda.synchronize()
    assert result.read() == [0] * 6

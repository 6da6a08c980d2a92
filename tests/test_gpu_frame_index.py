"""snp_frame_index_batch / snp_frame_read_indexed_batch (BlockCodec.frame_index_buffers / frame_read_indexed / frame_gather_to_memory): the index
arrays, every output and both d_results against the model (frame_index_model.py) on the streams the CPU tests use (the largest is 1.4 MB), guard
words around every output array, the index arrays and both workspaces, a canary-filled arena; all windows of all streams as the requests of one
call; equality with the device range call; many requests on one stream; the same index after the streams moved; admission by each bound;
corruption inside and outside the window; a stale index; the empty calls, the gather round trip and graph capture.  Needs an MI355X."""
import numpy as np
import pytest
import torch

import frame_buffers_helpers as H
import frame_index_model as X
import frame_range_model as R
import oracle as O
from seekable_harness import CANARY, Guarded, dev_i32, dev_u64, index_call, read_call

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from snappier_amd import batch as SB, _native as N

B = 65536
BIG = 1 << 62


def codec():
    return SB.BlockCodec(0, O.HASH_CRC32C)


def check(cd, streams, ix, requests, caps, mc=None, ec=None, **where):
    """The call against the model under the same bounds (default: what admits every request)."""
    need = X.read_needs(streams, ix, requests, caps)
    mc, ec = (need[0] if mc is None else mc), (need[1] if ec is None else ec)
    got = read_call(cd, streams, ix, requests, caps, mc, ec, **where)
    want = X.read_plan(streams, ix, requests, caps, mc, ec)
    assert got[0] == want[0], [(r, requests[r], g, w) for r, (g, w) in enumerate(zip(got[0], want[0])) if g != w][:10]
    assert got[1] == want[1] and got[3] == want[3], (got[3], want[3])
    for r in range(len(requests)):
        assert got[2][r] == want[2][r], f"request {r}: {requests[r]}"
    return got


def exact_caps(streams, requests, slack=0):
    out = []
    for r, (b, ro, rl) in enumerate(requests):
        lo, hi = R.clip(R.walk(streams[b])[1], ro, rl) if b < len(streams) else (0, 0)
        out.append(hi - lo + (slack and r % 3))
    return out


def interleaved(requests):
    """The requests in an order in which consecutive ones name different streams (round robin over the streams, as far as their counts allow)."""
    by = {}
    for q in requests:
        by.setdefault(q[0], []).append(q)
    rng = np.random.default_rng(9)
    for v in by.values():
        rng.shuffle(v)
    out, k = [], 0
    while by:
        for b in sorted(by, key=lambda b: (b * 7 + k) % 29):
            out.append(tuple(int(x) for x in by[b].pop()))
            if not by[b]:
                del by[b]
        k += 1
    return out


_named = {}


def named():
    """(streams, the model's index, every window of every stream as a request) -- computed once."""
    if not _named:
        streams = list(X.named_streams().values())
        _named["v"] = (streams, X.build_index(streams), X.all_windows(streams))
    return _named["v"]


# ---- 1. the index ------------------------------------------------------------------------------------------------------------------------------
def test_index_equals_the_model_on_the_named_streams():
    cd = codec()
    streams, want, _ = named()
    got = index_call(cd, streams)
    assert got == want
    assert got["result"][3] == 1 and got["result"][0] == len(got["start"]) == 141
    assert index_call(cd, streams, want["result"][2] + 7, want["result"][0] + 300) == want        # looser bounds change nothing
    # ... and through the convenience, which sizes the call itself
    framed, in_off, in_len = H.pack(streams)
    ix = cd.frame_index_buffers(framed, dev_u64(in_off), dev_u64(in_len))
    torch.cuda.synchronize()
    assert {k: getattr(ix, k).cpu().tolist() for k in ("first", "start", "pos", "total", "tail", "result")} == want and ix.nentries == 141


# ---- 2. reads against the model ------------------------------------------------------------------------------------------------------------------
def test_all_windows_of_all_streams_as_the_requests_of_one_call():
    cd = codec()
    streams, _, requests = named()
    ix = index_call(cd, streams)
    reqs = interleaved(requests)
    assert len(reqs) == 802 and sum(a[0] != b[0] for a, b in zip(reqs, reqs[1:])) > 0.9 * len(reqs)
    got = check(cd, streams, ix, reqs, exact_caps(streams, reqs, slack=1))
    assert {O.OK, O.ERR_TRUNCATED_STREAM, O.ERR_CHUNK_TYPE, O.ERR_BAD_LENGTH, O.ERR_INCOMPLETE, O.ERR_CRC_MISMATCH} <= set(got[0])
    assert got[3][0] > 0 and got[3][2] > 0 and 0 < got[3][3] < len(reqs)
    # looser bounds change nothing
    caps = exact_caps(streams, reqs, slack=1)
    need = X.read_needs(streams, ix, reqs, caps)
    assert read_call(cd, streams, ix, reqs, caps, need[0] + 300, need[1] + 1000)[:3] == got[:3]


# ---- 3. against the device range call ------------------------------------------------------------------------------------------------------------
def test_one_request_per_stream_equals_the_device_range_call():
    cd = codec()
    streams, _, _ = named()
    ix = index_call(cd, streams)
    rng = np.random.default_rng(3)
    ranges = []
    for b, s in enumerate(streams):
        rows, total, _, _ = R.walk(s)
        w = R.windows(rows, total)
        ranges.append(w[int(rng.integers(0, len(w)))] if b % 4 else (total // 3, total // 2 + 1))
    ranges = [(ro & R.U64, rl & R.U64) for ro, rl in ranges]
    requests = [(b, ro, rl) for b, (ro, rl) in enumerate(ranges)]
    caps = exact_caps(streams, requests)
    got = check(cd, streams, ix, requests, caps)
    framed, in_off, in_len = H.pack(streams)
    out_off, total = H.out_layout(caps)
    arena = torch.full((total,), CANARY, dtype=torch.uint8, device="cuda")
    ol, st, _ = cd.frame_decode_range_buffers(framed, dev_u64(in_off), dev_u64(in_len), dev_u64([r[0] for r in ranges]), dev_u64([r[1] for r in ranges]),
                                              arena, dev_u64(out_off), dev_u64(caps))
    torch.cuda.synchronize()
    a, st, ol = arena.cpu().numpy(), st.cpu().tolist(), ol.cpu().tolist()
    assert (st, ol) == (got[0], got[1]) and len(set(st)) > 3
    assert [a[o:o + n].tobytes() if s == O.OK else None for s, n, o in zip(st, ol, out_off.tolist())] == got[2]


# ---- 4. many requests on one stream --------------------------------------------------------------------------------------------------------------
def test_many_requests_on_one_stream():
    cd = codec()
    s, raw = R.uniform_stream(5, last=777)
    other = R.tiny_chunk_stream(1)[0]
    streams = [other, s]
    ix = index_call(cd, streams)
    rng = np.random.default_rng(4)
    total = len(raw)
    reqs = [(1, int(o), int(n)) for o, n in zip(rng.integers(0, total, 40), rng.integers(0, 3 * B, 40))]
    reqs += [(1, 2 * B + 100, 50), (1, 2 * B + 100, 50), (1, 2 * B + 120, 10), (1, B, B), (1, B, B), (1, 0, R.U64), (1, 0, R.U64), (1, 4 * B, 777)]   # duplicates, windows inside one chunk
    reqs += [(1, int(o), int(n)) for o, n in zip(rng.integers(0, total, 16), rng.integers(0, 200, 16))]
    assert len(reqs) == 64
    got = check(cd, streams, ix, reqs, exact_caps(streams, reqs))
    assert got[0] == [O.OK] * 64 and all(d == raw[o:o + n] for d, (_, o, n) in zip(got[2], reqs))


def test_windows_in_the_second_span_of_the_long_stream():
    cd = codec()
    s, raw = R.long_stream_with_a_skippable_chunk_across_the_span_boundary()
    ix = index_call(cd, [s])
    rows, total, _, _ = R.walk(s)
    first = next(r for r in rows if r[1] >= R.SPAN)                     # the first chunk whose header lies in span 1
    s1, d1 = first[4], first[5]
    assert ix["result"][3] == 1 and ix["result"][2] == 2 and max(ix["pos"]) > R.SPAN
    wins = [(s1 + 10, 1000), (s1, d1), (s1 + d1, 3 * B), (s1 + 5, total), (s1 - 100, 100), (s1 - 100, 101), (s1 - 1, 2), (0, s1), (total - 10, 100),
            (s1 - B, 2 * B + 7)]
    reqs = [(0, ro, rl) for ro, rl in wins]
    got = check(cd, [s], ix, reqs, exact_caps([s], reqs))
    assert got[0] == [O.OK] * len(wins) and all(d == raw[R.clip(total, *w)[0]:R.clip(total, *w)[1]] for d, w in zip(got[2], wins))


# ---- 5. position independence --------------------------------------------------------------------------------------------------------------------
def test_the_same_index_after_the_streams_are_repacked_at_other_offsets():
    cd = codec()
    streams, _, requests = named()
    ix = index_call(cd, streams, lead=1, gap=3)
    reqs = interleaved(requests)[::4]
    caps = exact_caps(streams, reqs)
    here = check(cd, streams, ix, reqs, caps, lead=1, gap=3)
    there = check(cd, streams, ix, reqs, caps, lead=777, gap=130)
    assert here == there
    assert index_call(cd, streams, lead=4099, gap=1) == ix              # and the index itself does not depend on where the streams lie


# ---- 6. admission --------------------------------------------------------------------------------------------------------------------------------
def test_index_admission_by_each_bound():
    cd = codec()
    a, b, c = R.uniform_stream(3, 1)[0], R.tiny_chunk_stream(3)[0], R.uniform_stream(2, 2, 500)[0]
    long_s = R.long_stream_with_a_skippable_chunk_across_the_span_boundary()[0]
    streams = [a, b, b"", long_s, c, a, R.ID]
    full = X.build_index(streams)
    need, spans = full["result"][0], full["result"][2]
    assert spans == 7
    for ms, me, first in ((spans, need, 7), (spans, need - 1, 5), (spans - 1, need, 6), (spans - 2, need, 5), (spans, 0, 0), (0, 0, 0), (1, 3, 1)):
        got = index_call(cd, streams, ms, me)
        assert got == X.build_index(streams, ms, me), (ms, me)
        assert got["tail"][first:] == [O.ERR_OUTPUT_TOO_SMALL] * (7 - first) and O.ERR_OUTPUT_TOO_SMALL not in got["tail"][:first]
        assert got["first"][:first + 1] == full["first"][:first + 1] and got["start"] == full["start"][:got["first"][-1]]


def test_read_admission_by_each_bound_an_unindexed_stream_and_a_bad_stream_number():
    cd = codec()
    a, b, c = R.uniform_stream(3, 1)[0], R.tiny_chunk_stream(3)[0], R.uniform_stream(2, 2, 500)[0]
    streams = [a, b, c]
    ix = index_call(cd, streams)
    requests = [(0, 10, 2 * B), (1, 0, R.U64), (2, B - 1, 2), (0, 0, 3 * B), (1, 5, 0), (2, 7, 10), (0, 0, 0)]
    caps = exact_caps(streams, requests)
    mc, ec = X.read_needs(streams, ix, requests, caps)
    full = check(cd, streams, ix, requests, caps)
    assert full[0] == [O.OK] * 7 and full[3] == [mc, sum(full[1]), ec, 7]
    for bounds, first in (((mc - 1, ec), 3), ((mc, ec - 1), 5), ((0, 0), 0), ((mc, 0), 0), ((0, ec), 0)):
        short = check(cd, streams, ix, requests, caps, *bounds)
        assert short[0][first:] == [O.ERR_OUTPUT_TOO_SMALL] * (7 - first) and short[1][first:] == [0] * (7 - first)
        assert short[0][:first] == full[0][:first] and short[2][:first] == full[2][:first]     # earlier requests are bit-identical
        assert read_call(cd, streams, ix, requests, caps, short[3][0], short[3][2]) == full     # d_result[0] and [2] are what the call needs
    # the third stream not indexed; stream numbers beyond the batch
    part = index_call(cd, streams, max_entries=ix["first"][2])
    assert part["tail"] == [O.OK, O.OK, O.ERR_OUTPUT_TOO_SMALL]
    requests = [(0, 5, 100), (2, 5, 100), (3, 5, 100), (0xFFFFFFFF, 0, 0), (1, 0, 50), (2, 0, 0), (0x80000000, 1, 1)]
    got = check(cd, streams, part, requests, [100, 100, 100, 0, 50, 0, 1])
    assert got[0] == [O.OK, O.ERR_OUTPUT_TOO_SMALL, O.ERR_BAD_ARG, O.ERR_BAD_ARG, O.OK, O.ERR_OUTPUT_TOO_SMALL, O.ERR_BAD_ARG] and got[3][3] == 2


# ---- 7. corruption -------------------------------------------------------------------------------------------------------------------------------
def test_a_corrupt_chunk_inside_and_outside_the_window():
    cd = codec()
    streams, requests, hits = [], [], []
    for s in (R.uniform_stream(4, 5)[0], R.tiny_chunk_stream(2)[0], R.big_chunk_stream()[0]):
        rows, total, _, _ = R.walk(s)
        full = [r for r in rows if r[5] > 0]
        for victim in (full[0], full[len(full) // 2], full[-1]):
            streams.append(R.corrupt_chunk(s, victim))
            wins = R.windows(rows, total)[::2]
            requests += [(len(streams) - 1, ro & R.U64, rl & R.U64) for ro, rl in wins]
            hits += [victim in R.select(rows, *R.clip(total, ro, rl))[0] for ro, rl in wins]
    ix = index_call(cd, streams)
    got = check(cd, streams, ix, requests, exact_caps(streams, requests))
    assert [st != O.OK for st in got[0]] == hits and sum(hits) > 20 and len(hits) - sum(hits) > 20


# ---- 8. a stale index ----------------------------------------------------------------------------------------------------------------------------
def test_a_stale_index_gives_the_models_statuses_and_writes_nowhere_else():
    cd = codec()
    s = R.uniform_stream(5, last=777)[0]
    other = R.uniform_stream(5, 3, 777)[0]
    ix = index_call(cd, [s])
    rows = R.walk(s)[0]
    assert rows[2][0] == 1
    p = ix["pos"][2]
    altered = s[:p + 1] + bytes([s[p + 1] ^ 1]) + s[p + 2:]             # the size field of chunk 2's header
    requests = [(0, 10, 100), (0, B + 5, 2 * B), (0, B, 2 * B), (0, 3 * B - 1, 2), (0, 0, R.U64), (0, 4 * B + 1, 10), (0, 2 * B, 0), (0, 2 * B + 7, 9)]
    caps = exact_caps([s], requests)
    good = check(cd, [s], ix, requests, caps)
    assert good[0] == [O.OK] * len(requests)
    got = check(cd, [altered], ix, requests, caps)
    assert got[0] == [O.OK, O.ERR_BAD_ARG, O.ERR_BAD_ARG, O.ERR_BAD_ARG, O.ERR_BAD_ARG, O.OK, O.OK, O.ERR_BAD_ARG]
    got = check(cd, [other], ix, requests, caps)                        # a different stream at the same place
    assert got[0][0] == O.OK and set(got[0][1:6]) == {O.ERR_BAD_ARG}


# ---- 9. the remaining cases ----------------------------------------------------------------------------------------------------------------------
def test_empty_calls_write_a_zeroed_d_result():
    cd = codec()
    IL = N.frame_index_lib()
    s = R.uniform_stream(2, 1)[0]
    ix = index_call(cd, [s])
    assert read_call(cd, [s], ix, [], [], 0, 0)[3] == [0] * 4 and read_call(cd, [s], ix, [], [], 100, 1 << 20)[3] == [0] * 4
    assert index_call(cd, [])["result"] == [0] * 4
    none = {"first": [0], "start": [], "pos": [], "total": [], "tail": []}
    assert read_call(cd, [], none, [(0, 0, 10), (5, 1, 1)], [10, 1], 0, 0)[0] == [O.ERR_BAD_ARG] * 2        # no stream at all
    result = Guarded(4, torch.int64)
    assert IL.snp_frame_index_batch(cd.ctx.handle, None, None, None, 0, 0, 0, *[None] * 6, result.ptr()) == O.OK   # ctx and d_result only
    torch.cuda.synchronize()
    assert result.read() == [0] * 4
    result = Guarded(4, torch.int64)
    assert IL.snp_frame_read_indexed_batch(cd.ctx.handle, *[None] * 3, 0, *[None] * 5, 0, *[None] * 3, 0, 0, 0, *[None] * 6, result.ptr()) == O.OK
    torch.cuda.synchronize()
    assert result.read() == [0] * 4


@pytest.mark.parametrize("align", [1, 256])
def test_frame_gather_to_memory_round_trips(align):
    cd = codec()
    rng = np.random.default_rng(align)
    raws = H.ragged(rng, 6, 300 * 1024) + [b""]
    streams = [O.frame_encode(x) for x in raws]
    framed, in_off, in_len = H.pack(streams)
    tabs = [dev_u64(in_off), dev_u64(in_len)]
    ix = cd.frame_index_buffers(framed, *tabs)
    reqs = []
    for k in range(40):
        b = int(rng.integers(0, len(raws)))
        t = len(raws[b])
        lo = int(rng.integers(0, t + 1))
        reqs.append([(b, lo, int(rng.integers(0, t - lo + 2))), (b, 0, R.U64 >> 1), (b, lo, 70000), (b, t + 3, 9)][k % 4])
    reqs.append((len(raws), 0, 10))                                     # no such stream
    rs, ro, rl = dev_i32([q[0] for q in reqs]), dev_u64([q[1] for q in reqs]), dev_u64([q[2] for q in reqs])
    out, out_off, out_len, status = cd.frame_gather_to_memory(framed, *tabs, ix, rs, ro, rl, align=align)
    torch.cuda.synchronize()
    h, oo, ol, st = out.cpu().numpy(), out_off.cpu().tolist(), out_len.cpu().tolist(), status.cpu().tolist()
    slots = [(min(n, 22 * len(streams[b])) + align - 1) // align * align if b < len(raws) else 0 for b, _, n in reqs]
    assert out.numel() == sum(slots) and oo == [sum(slots[:r]) for r in range(len(slots))]
    for r, (b, o, n) in enumerate(reqs[:-1]):
        lo, hi = R.clip(len(raws[b]), o, n)
        assert st[r] == O.OK and ol[r] == hi - lo and oo[r] % align == 0 and h[oo[r]:oo[r] + ol[r]].tobytes() == raws[b][lo:hi], f"request {r}"
    assert st[-1] == O.ERR_BAD_ARG and ol[-1] == 0
    with pytest.raises(ValueError):
        cd.frame_gather_to_memory(framed, *tabs, ix, rs, ro, rl, align=align, max_bytes=sum(slots) - 1)
    empty = torch.empty(0, dtype=torch.int64, device="cuda")
    assert cd.frame_gather_to_memory(framed, *tabs, ix, torch.empty(0, dtype=torch.int32, device="cuda"), empty, empty)[0].numel() == 0
    # the defaults of frame_read_indexed size the call themselves
    caps = [hi - lo for lo, hi in (R.clip(len(raws[b]), o, n) if b < len(raws) else (0, 0) for b, o, n in reqs)]
    o_off, total = H.out_layout(caps)
    arena = torch.full((total,), CANARY, dtype=torch.uint8, device="cuda")
    ol2, st2, res = cd.frame_read_indexed(framed, *tabs, ix, rs, ro, rl, arena, dev_u64(o_off), dev_u64(caps))
    torch.cuda.synchronize()
    assert ol2.cpu().tolist() == ol and st2.cpu().tolist() == st and res.cpu().tolist()[1] == sum(ol) and res.cpu().tolist()[3] == len(reqs) - 1
    a = arena.cpu().numpy()
    assert all(a[o:o + n].tobytes() == h[p:p + n].tobytes() for o, p, n in zip(o_off.tolist(), oo, ol))
    assert (H.outside_ranges(a, o_off, caps) == CANARY).all()


def test_read_call_replays_from_a_graph_on_new_requests():
    cd = codec()
    streams = [R.uniform_stream(3, 1)[0], R.tiny_chunk_stream(5)[0], R.big_chunk_stream()[0], R.zero_length_chunk_stream()[0]]
    model = X.build_index(streams)
    batches = {"a": [(0, 10, 2 * B), (1, 100, 3000), (2, 5001, 250_000), (0, B - 1, 2), (3, 650, 200), (9, 0, 5)],
               "b": [(2, 0, R.U64), (2, 100_000, 10), (1, 0, R.U64), (0, B + 7, B), (3, 0, 1600), (1, 7, 0)]}
    nreq, cap = 6, 300_000
    mc, ec = 64, 600_000                                                # bounds that hold both batches
    IL = N.frame_index_lib()
    framed, in_off, in_len = H.pack(streams)
    tabs = [dev_u64(in_off), dev_u64(in_len)]
    ix = cd.frame_index_buffers(framed, *tabs)
    out_off, out_cap = dev_u64(np.arange(nreq) * cap), dev_u64([cap] * nreq)
    rs = torch.zeros(nreq, dtype=torch.int32, device="cuda")
    ro, rl = (torch.zeros(nreq, dtype=torch.int64, device="cuda") for _ in range(2))
    out = torch.zeros(nreq * cap, dtype=torch.uint8, device="cuda")
    work = torch.empty(IL.snp_frame_read_indexed_workspace(nreq, mc, ec), dtype=torch.uint8, device="cuda")

    def load(which):
        reqs = batches[which]
        rs.copy_(dev_i32([q[0] for q in reqs]))
        ro.copy_(dev_u64([q[1] for q in reqs]))
        rl.copy_(dev_u64([q[2] for q in reqs]))

    def call():
        return cd.frame_read_indexed(framed, *tabs, ix, rs, ro, rl, out, out_off, out_cap, max_chunks=mc, edge_cap=ec, work=work)

    def verify(which, tensors):
        torch.cuda.synchronize()
        ol, st, res = (t.cpu().tolist() for t in tensors)
        want = X.read_plan(streams, model, batches[which], [cap] * nreq, mc, ec)
        assert (st, ol, res) == (want[0], want[1], want[3]), which
        h = out.cpu().numpy()
        for r in range(nreq):
            if st[r] == O.OK:
                assert h[r * cap:r * cap + ol[r]].tobytes() == want[2][r], (which, r)

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

"""snp_frame_digest_indexed_batch (BlockCodec.frame_digest_indexed / frame_digest_streams): digest, dig_len and status against the oracle's
CRC-32C of the decoded window and the status of the indexed read, with guard words around every output array and the workspace
(digest_call): every window at and around every chunk boundary at four chunk sizes; the same bytes under four chunk grids; foreign streams;
unsound indexes; corruption at an edge, inside a window and in a header CRC; 70 000 rows under one request, 70 000 requests of one row,
both at once, admission by edge_cap; shifts past 2^32 bytes; graph capture.  Needs an MI355X."""
import ctypes as C

import numpy as np
import pytest
import torch

import frame_buffers_helpers as H
import frame_digest_model as D
import frame_index_model as X
import frame_range_model as R
import oracle as O
import stream_grammar as G
from conftest import read_testdata
from seekable_harness import Guarded, dev_i32, dev_u64, read_call

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from snappier_amd import batch as SB, _native as N

B = 65536
U64 = D.U64


def codec():
    return SB.BlockCodec(0, O.HASH_CRC32C)


def _p(t):
    return C.c_void_p(t.data_ptr()) if t.numel() else C.c_void_p(None)


def u32s(t):
    return [int(v) & 0xFFFFFFFF for v in t.tolist()]


def digest_call(cd, streams, ix, requests, ec, lead=1, gap=3):
    """snp_frame_digest_indexed_batch called directly, the three outputs, d_result and the workspace between guard elements:
    -> (status, dig_len, digest, d_result)."""
    ns, nreq = len(streams), len(requests)
    DL = N.frame_digest_lib()
    cd._bind()
    framed, in_off, in_len = H.pack(streams, lead, gap) if ns else (torch.zeros(16, dtype=torch.uint8, device="cuda"), [], [])
    digest, dig_len, status, result = Guarded(nreq, torch.int32), Guarded(nreq, torch.int64), Guarded(nreq, torch.int32), Guarded(4, torch.int64)
    work = Guarded(DL.snp_frame_digest_indexed_workspace(nreq, ec), torch.uint8)
    ne = min(len(ix["start"]), len(ix["pos"]))
    tabs = [dev_u64(x) for x in (in_off, in_len, ix["first"], ix["start"] or [0], ix["pos"] or [0], ix["total"])] + [dev_i32(ix["tail"])] + \
        [dev_i32([b - (1 << 32) if b >= 1 << 31 else b for b, _, _ in requests])] + \
        [dev_u64(x) for x in ([r[1] for r in requests], [r[2] for r in requests])]      # (named: they outlive the call)
    st = DL.snp_frame_digest_indexed_batch(cd.ctx.handle, _p(framed), _p(tabs[0]), _p(tabs[1]), ns, *[_p(t) for t in tabs[2:7]], ne,
                                           _p(tabs[7]), _p(tabs[8]), _p(tabs[9]), nreq, ec, digest.ptr(), dig_len.ptr(), status.ptr(),
                                           work.ptr(), result.ptr())
    assert st == O.OK
    torch.cuda.synchronize()
    work.read()
    return status.read(), dig_len.read(), [v & 0xFFFFFFFF for v in digest.read()], result.read()


def check(cd, streams, ix, requests, ec=None):
    """The call against the model under the same bound (default: what admits every request)."""
    ec = D.edge_need(streams, ix, requests) if ec is None else ec
    got = digest_call(cd, streams, ix, requests, ec)
    want = D.digest_plan(streams, ix, requests, ec)
    assert got[0] == want[0], [(r, requests[r], g, w) for r, (g, w) in enumerate(zip(got[0], want[0])) if g != w][:10]
    assert got[1] == want[1] and got[2] == want[2] and got[3] == want[3], (got[3], want[3])
    return got


def pack_raw(raws):
    data = torch.from_numpy(np.frombuffer(b"".join(raws) or b"\0", dtype=np.uint8).copy()).cuda()
    lens = np.array([len(x) for x in raws], dtype=np.int64)
    return data, H.dev(np.cumsum(lens) - lens), H.dev(lens)


@pytest.fixture(scope="module")
def html():
    return read_testdata("html") * 3


# ---- 1. windows ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cb", [1, 7, 4096, 65536])
def test_every_window_at_and_around_every_chunk_boundary(cb, html):
    cd = codec()
    raws = [html[11:11 + n] for n in (0, 1, cb - 1, cb, cb + 1, 3 * cb + 5)]
    data, in_off, in_len = pack_raw(raws)
    out, out_off, out_len, status, _, index = cd.frame_encode_seekable(data, in_off, in_len, chunk_bytes=cb)
    assert status.tolist() == [O.OK] * len(raws)
    requests = []
    for b, raw in enumerate(raws):
        n = len(raw)
        bounds = sorted(set(range(0, n + 1, cb)) | {n})
        points = sorted({p + d for p in bounds for d in (-1, 0, 1) if 0 <= p + d <= n + 1})
        requests += [(b, lo, hi - lo) for lo in points for hi in points if hi >= lo] + [(b, 0, U64)]
    rs = torch.tensor([q[0] for q in requests], dtype=torch.int32, device="cuda")
    ro, rl = dev_u64([q[1] for q in requests]), dev_u64([q[2] for q in requests])
    digest, dig_len, dstatus, result = cd.frame_digest_indexed(out, out_off, out_len, index, rs, ro, rl)
    want = [raws[b][lo:min(lo + ln, U64)] for b, lo, ln in requests]
    caps = dev_u64([len(w) for w in want])
    offs = dev_u64(np.cumsum([0] + [len(w) for w in want[:-1]]).tolist())
    arena = torch.empty(max(sum(len(w) for w in want), 1), dtype=torch.uint8, device="cuda")
    rlen, rstatus, _ = cd.frame_read_indexed(out, out_off, out_len, index, rs, ro, rl, arena, offs, caps)
    torch.cuda.synchronize()
    assert dstatus.tolist() == rstatus.tolist() == [O.OK] * len(requests)
    assert dig_len.tolist() == rlen.tolist() == [len(w) for w in want]
    got = u32s(digest)
    for r, w in enumerate(want):
        assert got[r] == O.crc32c(w), (cb, requests[r])
    res = result.tolist()
    assert res[1] == sum(len(w) for w in want) and res[3] == len(requests)
    assert len(requests) > 60


# ---- 2. chunking does not matter ---------------------------------------------------------------------------------------------------------------------
def test_the_digest_does_not_depend_on_the_chunk_grid(html):
    cd = codec()
    raws = [html[:200000], html[777:777 + 65536 * 2], html[5:5 + 4096 * 3 + 100]]
    ns = len(raws)
    data, in_off, in_len = pack_raw(raws)
    small = cd.frame_encode_seekable(data, in_off, in_len, chunk_bytes=4096)
    big = cd.frame_encode_seekable(data, in_off, in_len, chunk_bytes=65536)
    # a third copy: 100 bytes inserted in the middle of a chunk, then deleted again -- the chunks around the hole are cut differently now
    ins = torch.from_numpy(np.frombuffer(bytes(range(100)) * ns, dtype=np.uint8).copy()).cuda()
    at, zero, hundred = dev_u64([4096 + 1000] * ns), dev_u64([0] * ns), dev_u64([100] * ns)
    s1 = cd.frame_splice_to_memory(small[0], small[1], small[2], small[5], at, zero, ins, dev_u64([100 * b for b in range(ns)]), hundred, chunk_bytes=4096)
    s2 = cd.frame_splice_to_memory(s1[0], s1[1], s1[2], s1[4], at, hundred, ins, zero, zero, chunk_bytes=4096)
    assert s1[3].tolist() == s2[3].tolist() == [O.OK] * ns
    # a fourth: that one rechunked to 8192
    r4 = cd.frame_rechunk_to_memory(s2[0], s2[1], s2[2], s2[4], 8192)
    assert r4[3].tolist() == [O.OK] * ns and all(n > 0 for n in r4[2].tolist())
    want = [O.crc32c(x) for x in raws]
    DL = N.frame_digest_lib()
    for framed, off, ln, index in ((small[0], small[1], small[2], small[5]), (big[0], big[1], big[2], big[5]), (s2[0], s2[1], s2[2], s2[4]),
                                   (r4[0], r4[1], r4[2], r4[4])):
        digest, dig_len, status = cd.frame_digest_streams(framed, off, ln, index)
        assert status.tolist() == [O.OK] * ns and dig_len.tolist() == [len(x) for x in raws] and u32s(digest) == want
        # ... the direct call with edge_cap = 0 and a workspace sized for that
        rs = torch.arange(ns, dtype=torch.int32, device="cuda")
        work = torch.empty(DL.snp_frame_digest_indexed_workspace(ns, 0), dtype=torch.uint8, device="cuda")
        digest, dig_len, status, result = cd.frame_digest_indexed(framed, off, ln, index, rs, dev_u64([0] * ns), dev_u64([U64] * ns), edge_cap=0, work=work)
        assert status.tolist() == [O.OK] * ns and u32s(digest) == want
        res = result.tolist()
        assert res[2] == 0 and res[3] == ns and res[1] == sum(len(x) for x in raws) and res[0] > 0


# ---- 3. foreign streams --------------------------------------------------------------------------------------------------------------------------
def test_foreign_streams_of_the_stream_grammar():
    cd = codec()
    frames = G.frame_corpus()
    streams = [s for _n, s, _r in frames] + [R.tiny_chunk_stream(1)[0], R.zero_length_chunk_stream()[0], R.big_chunk_stream()[0]]
    streams.append(streams[0] + streams[2])                             # a repeated identifier between data chunks
    raws = [b"".join(r) for _n, _s, r in frames] + [R.tiny_chunk_stream(1)[1], R.zero_length_chunk_stream()[1], R.big_chunk_stream()[1]]
    raws.append(raws[0] + raws[2])
    ix = X.build_index(streams)
    requests = [(b, ro & U64, rl & U64) for b, ro, rl in X.all_windows(streams)]          # (as the 64-bit words the call gets)
    got = check(cd, streams, ix, requests)
    unsound = {b for b, (name, _s, _r) in enumerate(frames) if name in ("mutated-chunk", "wrong-crc")}
    sound = 0
    for r, (b, ro, rl) in enumerate(requests):
        if got[0][r] == O.OK and b not in unsound:
            lo, hi = R.clip(len(raws[b]), ro, rl)
            assert got[1][r] == hi - lo and got[2][r] == O.crc32c(raws[b][lo:hi]), (b, ro, rl)
            sound += 1
    assert sound > 250 and {O.OK, O.ERR_CRC_MISMATCH} <= set(got[0])
    whole = [(b, 0, U64) for b in range(len(streams))]
    got = check(cd, streams, ix, whole, 0)
    assert got[3][2] == 0 and got[0] == [O.OK] * len(streams)           # (no chunk of a whole stream is decoded: the two bad ones are OK too)
    for b in range(len(streams)):
        if b not in unsound:
            assert got[2][b] == O.crc32c(raws[b]), b


# ---- 4. the index is untrusted ---------------------------------------------------------------------------------------------------------------------
def test_unsound_indexes_give_the_reads_statuses_and_write_nowhere_else():
    cd = codec()
    streams = list(X.named_streams().values())
    ns = len(streams)
    ix = X.build_index(streams)
    requests = [(b, ro & U64, rl & U64) for b, ro, rl in X.all_windows(streams)[::3]] + [(ns, 0, 10), (0xFFFFFFFF, 5, 5)]
    rng = np.random.default_rng(11)
    ne = len(ix["start"])

    def rnd(n, hi=1 << 64):
        return [int(v) % hi for v in rng.integers(0, 1 << 63, n, dtype=np.uint64) * 2 + rng.integers(0, 2, n, dtype=np.uint64)]

    lens = [len(s) for s in streams]
    indexes = [ix,
               {**ix, "start": rnd(ne), "pos": rnd(ne)},
               {**ix, "first": rnd(ns + 1), "total": rnd(ns), "start": rnd(ne), "pos": rnd(ne)},
               {**ix, "start": rnd(ne, 1 << 17), "pos": rnd(ne, 1 << 12), "total": rnd(ns, 1 << 18)},
               {**ix, "first": [f + (1 << 33) * (i % 2) for i, f in enumerate(ix["first"])]},
               {**ix, "first": list(reversed(ix["first"]))},
               {**ix, "pos": [p + lens[i % ns] for i, p in enumerate(ix["pos"])]},
               {**ix, "pos": [max(lens) - 1 - (i % 20) for i in range(ne)]},
               {**ix, "start": list(reversed(ix["start"]))},
               {**ix, "start": [v ^ ((i % 3 == 0) << 9) for i, v in enumerate(ix["start"])]},
               {**ix, "pos": [p + 1 for p in ix["pos"]]},                # stale: every position off by one
               {**ix, "tail": [int(v) % 40 - 20 for v in rng.integers(0, 1000, ns)]},
               {**ix, "start": ix["start"][:ne // 2], "pos": ix["pos"][:ne // 2]},
               {**ix, "start": [], "pos": []}]
    refused = 0
    caps = [U64] * len(requests)
    for c, index in enumerate(indexes):
        got = check(cd, streams, index, requests)                       # (digest_call checks the guard words around outputs and workspace)
        if c in (0, 9, 10):                                             # the read itself, on the device, where the totals are the streams' own
            mc, ec = X.read_needs(streams, index, requests, caps)
            exact = [R.clip(index["total"][b], ro, rl)[1] - R.clip(index["total"][b], ro, rl)[0] if b < ns else 0 for b, ro, rl in requests]
            rstatus = read_call(cd, streams, index, requests, exact, mc, ec)[0]
            for r, (a, b) in enumerate(zip(got[0], rstatus)):
                assert a == b or (a == O.OK and b not in (O.OK, O.ERR_BAD_ARG)), (c, r, a, b)
        refused += c > 0 and got[0].count(O.ERR_BAD_ARG)
    assert refused > 500


# ---- 5. corruption -------------------------------------------------------------------------------------------------------------------------------
def test_corruption_at_an_edge_inside_a_window_and_in_a_header_crc():
    cd = codec()
    s, raw = R.uniform_stream(5, last=777)
    rows = R.walk(s)[0]
    ix = X.build_index([s])
    req = [(0, B + 5, 2 * B)]                                           # head edge: chunk 1, interior: chunk 2, tail edge: chunk 3
    good = check(cd, [s], ix, req)
    assert good[0] == [O.OK] and good[2] == [O.crc32c(raw[B + 5:3 * B + 5])] and good[3] == [1, 2 * B, 2 * B, 1]
    for edge in (1, 3):
        bad = R.corrupt_chunk(s, rows[edge])
        got = check(cd, [bad], ix, req)
        rstatus = read_call(cd, [bad], ix, req, [2 * B], 1, 2 * B)[0]
        assert got[0] == rstatus and rstatus[0] != O.OK and got[1] == [0] and got[2] == [0]
    inner = R.corrupt_chunk(s, rows[2])
    assert read_call(cd, [inner], ix, req, [2 * B], 1, 2 * B)[0] != [O.OK]
    assert check(cd, [inner], ix, req)[:3] == good[:3]                  # never decoded
    p = ix["pos"][2] + 4
    flipped = s[:p] + bytes([s[p] ^ 0x10]) + s[p + 1:]
    got = check(cd, [flipped], ix, req)
    assert got[0] == [O.OK] and got[1] == good[1] and got[2] != good[2]


# ---- 6. tiers --------------------------------------------------------------------------------------------------------------------------------------
def test_rows_are_balanced_not_requests(html):
    cd = codec()
    n = 70000
    raw = html[3:3 + n]
    data, in_off, in_len = pack_raw([raw])
    out, out_off, out_len, status, _, index = cd.frame_encode_seekable(data, in_off, in_len, chunk_bytes=1)
    assert status.tolist() == [O.OK] and index.nentries == n
    byte_crc = [O.crc32c(bytes([v])) for v in range(256)]
    singles = [(0, i, 1) for i in range(n)]
    wide = [(0, 0, U64), (0, 1, n - 2), (0, 64, 64 * 1000), (0, 63, 65), (0, n - 1, 5), (0, n, 1)]
    for requests in ([(0, 0, U64)], singles, wide + singles[::7] + wide[::-1]):
        rs = torch.zeros(len(requests), dtype=torch.int32, device="cuda")
        ro, rl = dev_u64([q[1] for q in requests]), dev_u64([q[2] for q in requests])
        digest, dig_len, dstatus, result = cd.frame_digest_indexed(out, out_off, out_len, index, rs, ro, rl, edge_cap=0)
        torch.cuda.synchronize()
        assert int((dstatus != 0).sum()) == 0
        got, lens = u32s(digest), dig_len.tolist()
        for r, (_, lo, ln) in enumerate(requests):
            w = raw[lo:min(lo + ln, n)]
            assert lens[r] == len(w) and got[r] == (byte_crc[w[0]] if len(w) == 1 else O.crc32c(w)), requests[r]
        res = result.tolist()
        assert res == [sum(lens), sum(lens), 0, len(requests)]          # every chunk is one byte and every window is on chunk boundaries


def test_edge_cap_admits_exactly_the_first_k_requests(html):
    cd = codec()
    cb = 4096
    raw = html[:10 * cb + 77]
    data, in_off, in_len = pack_raw([raw])
    out, out_off, out_len, status, _, index = cd.frame_encode_seekable(data, in_off, in_len, chunk_bytes=cb)
    requests = [(0, 0, cb), (0, 5, 10), (0, cb, 3 * cb), (0, cb + 1, 2 * cb), (0, 0, U64), (0, 10 * cb + 1, 5), (0, 3, 9 * cb)]
    edges = [0, cb, 0, 2 * cb, 0, 77, 2 * cb]
    rs = torch.zeros(len(requests), dtype=torch.int32, device="cuda")
    ro, rl = dev_u64([q[1] for q in requests]), dev_u64([q[2] for q in requests])
    for k in range(len(requests) + 1):
        cap = sum(edges[:k])
        admitted = max(i for i in range(len(requests) + 1) if sum(edges[:i]) <= cap)
        digest, dig_len, dstatus, result = cd.frame_digest_indexed(out, out_off, out_len, index, rs, ro, rl, edge_cap=cap)
        got, lens, st = u32s(digest), dig_len.tolist(), dstatus.tolist()
        for r, (_, lo, ln) in enumerate(requests):
            w = raw[lo:min(lo + ln, len(raw))]
            assert (st[r], lens[r], got[r]) == ((O.OK, len(w), O.crc32c(w)) if r < admitted else (O.ERR_OUTPUT_TOO_SMALL, 0, 0)), (k, r)
        assert result.tolist()[2:] == [sum(edges), admitted]
    # the wrapper sizes the call itself
    digest, dig_len, dstatus, result = cd.frame_digest_indexed(out, out_off, out_len, index, rs, ro, rl)
    assert dstatus.tolist() == [O.OK] * len(requests) and result.tolist()[2] == sum(edges)


# ---- 7. shifts past 2^32 bytes -----------------------------------------------------------------------------------------------------------------------
def test_shifts_past_4_gib_with_no_large_buffer():
    count = 65537
    free = torch.cuda.mem_get_info()[0]
    if free < 2 << 30:
        pytest.skip(f"needs 2 GiB of free device memory, {free >> 30} GiB free")
    cd = codec()
    zeros = torch.zeros(B, dtype=torch.uint8, device="cuda")
    one = cd.frame_encode_seekable(zeros, dev_u64([0]), dev_u64([B]), chunk_bytes=B)
    n1 = int(one[2].item())
    chunk = one[0][10:n1]                                               # the one data chunk behind the identifier
    framed = torch.cat([one[0][:10], chunk.repeat(count)])
    assert 150_000_000 < framed.numel() < 300_000_000
    in_off, in_len = dev_u64([0]), dev_u64([framed.numel()])
    index = cd.frame_index_buffers(framed, in_off, in_len)
    total = count * B
    assert index.total.tolist() == [total] and index.tail.tolist() == [O.OK] and index.nentries == count and total > 1 << 32
    c = O.crc32c(bytes(B))
    rs = torch.zeros(3, dtype=torch.int32, device="cuda")
    digest, dig_len, status, result = cd.frame_digest_indexed(framed, in_off, in_len, index, rs, dev_u64([0, 5, B]), dev_u64([U64, U64, total - 2 * B]))
    want = [D.repeat_digest(c, B, count),
            D.crc_combine(O.crc32c(bytes(B - 5)), D.repeat_digest(c, B, count - 1), (count - 1) * B),
            D.repeat_digest(c, B, count - 2)]
    assert status.tolist() == [O.OK] * 3 and dig_len.tolist() == [total, total - 5, total - 2 * B]
    assert u32s(digest) == want
    assert result.tolist() == [3 * count - 3, 3 * total - 5 - 2 * B, B, 3]
    assert want[0] == D.crc_combine(want[2], D.repeat_digest(c, B, 2), 2 * B) and len(set(want)) == 3      # (the model's own consistency, past 2^32)


# ---- 8. graph capture ------------------------------------------------------------------------------------------------------------------------------
def test_graph_capture_replays_the_call(html):
    cd = codec()
    cb = 4096
    raws = [html[:5 * cb + 9], html[100:100 + 3 * cb]]
    data, in_off, in_len = pack_raw(raws)
    out, out_off, out_len, status, _, index = cd.frame_encode_seekable(data, in_off, in_len, chunk_bytes=cb)
    lists = [[(0, 5, 3 * cb), (1, 0, U64), (0, cb, cb), (1, cb - 1, 2)], [(1, 7, 2 * cb), (0, 0, U64), (0, 0, 0), (1, 3, 5)]]
    nreq = 4
    ec = 4 * cb
    live = [torch.zeros(nreq, dtype=torch.int32, device="cuda"), dev_u64([0] * nreq), dev_u64([0] * nreq)]
    tens = [[torch.tensor([q[0] for q in lst], dtype=torch.int32, device="cuda"), dev_u64([q[1] for q in lst]), dev_u64([q[2] for q in lst])]
            for lst in lists]
    work = torch.empty(N.frame_digest_lib().snp_frame_digest_indexed_workspace(nreq, ec), dtype=torch.uint8, device="cuda")

    def call():
        return cd.frame_digest_indexed(out, out_off, out_len, index, *live, edge_cap=ec, work=work)

    for t, v in zip(live, tens[0]):
        t.copy_(v)
    plain = [x.clone() for x in call()]                                  # one plain call
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        call()                                                          # the same call once before the capture, on the capture's stream
        torch.cuda.synchronize()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        digest, dig_len, dstatus, result = call()
    for k in (0, 1, 0):
        for t, v in zip(live, tens[k]):
            t.copy_(v)
        digest.fill_(-1)
        g.replay()
        torch.cuda.synchronize()
        want = [raws[b][lo:min(lo + ln, len(raws[b]))] for b, lo, ln in lists[k]]
        assert dstatus.tolist() == [O.OK] * nreq and dig_len.tolist() == [len(w) for w in want] and u32s(digest) == [O.crc32c(w) for w in want]
        if k == 0:
            assert all(torch.equal(a, b) for a, b in zip(plain, (digest, dig_len, dstatus, result)))

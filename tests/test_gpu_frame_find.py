"""snp_frame_find_indexed_batch (BlockCodec.frame_find_indexed / frame_find_streams): status, win_len, count, nhits, hits and d_result against the
model (tests/frame_find_model.py) and, where the status is OK, count and hits against the ground truth (bytes.find over the decoded bytes),
with guard words around every output array, hits and the workspace (find_call): a needle at every position of a small buffer under four chunk
sizes and eight needle lengths; overlapping occurrences and every interesting hit_cap; windows of every kind and needles that straddle their
edges; tile borders and runs that begin at odd scratch addresses; 70 000 requests of one row beside one request of 70 000 rows; requests that
share needle bytes; unsound indexes, corruption inside and outside the window, foreign streams; admission by both bounds and the one sizing
round; a window past 2^32 bytes; graph capture; the wrappers.  Needs an MI355X."""
import ctypes as C

import numpy as np
import pytest
import torch

import frame_buffers_helpers as H
import frame_chunked_model as K
import frame_find_model as F
import frame_index_model as X
import frame_range_model as R
import oracle as O
import stream_grammar as G
from conftest import read_testdata
from seekable_harness import Guarded, UNTOUCHED, dev_i32, dev_u64, s32
from test_frame_diff_model import unsound_indexes

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from snappier_amd import batch as SB, _native as N

U64 = F.U64
WHOLE = (0, U64)
B = 65536


def codec():
    return SB.BlockCodec(0, O.HASH_CRC32C)


def _p(t):
    return C.c_void_p(t.data_ptr()) if t.numel() else C.c_void_p(None)


def stream_tensors(streams, ix, lead=1, gap=3):
    ns = len(streams)
    framed, in_off, in_len = H.pack(streams, lead, gap) if ns else (torch.zeros(16, dtype=torch.uint8, device="cuda"), [], [])
    ne = min(len(ix["start"]), len(ix["pos"]))
    tabs = [framed] + [dev_u64(x) for x in (in_off, in_len, ix["first"], ix["start"] or [0], ix["pos"] or [0], ix["total"])] + \
        [dev_i32([s32(v) for v in ix["tail"]])]
    return tabs, ns, ne


def find_call(cd, streams, ix, requests, needles, caps, max_rows, scratch_cap, layout=None):
    """snp_frame_find_indexed_batch called directly, the five outputs, hits, d_result and the workspace between guard elements; no slot of hits
    beyond nhits[r] is written.  layout: (buffer, needle_off, needle_len) when the needles share bytes.  -> what F.find_plan returns."""
    nreq = len(requests)
    FL = N.frame_find_lib()
    cd._bind()
    tabs, ns, ne = stream_tensors(streams, ix)
    buf, noff, nlen = layout or F.pack_needles(F.per_request(needles, nreq))
    nd = [torch.from_numpy(np.frombuffer(buf, dtype=np.uint8).copy()).cuda(), dev_u64(noff), dev_i32(nlen)]
    hit_off = [sum(caps[:r]) for r in range(nreq)] if nreq < 2000 else (np.cumsum(caps) - np.array(caps)).tolist()
    hits = Guarded(sum(caps), torch.int64)
    outs = [Guarded(nreq, torch.int64) for _ in range(3)]
    status, result = Guarded(nreq, torch.int32), Guarded(4, torch.int64)
    work = Guarded(FL.snp_frame_find_indexed_workspace(nreq, max_rows, scratch_cap), torch.uint8)
    req = [dev_i32([s32(q[0]) for q in requests]), dev_u64([q[1] for q in requests]), dev_u64([q[2] for q in requests])]
    hit = [dev_u64(hit_off), dev_u64(caps)]
    st = FL.snp_frame_find_indexed_batch(cd.ctx.handle, *[_p(t) for t in tabs[:3]], ns, *[_p(t) for t in tabs[3:]], ne, *[_p(t) for t in req], nreq,
                                         *[_p(t) for t in nd], max_rows, scratch_cap, hits.ptr(), *[_p(t) for t in hit],
                                         *[g.ptr() for g in outs], status.ptr(), work.ptr(), result.ptr())
    assert st == O.OK
    torch.cuda.synchronize()
    work.read()
    win_len, count, nhits = [g.read() for g in outs]
    flat = hits.read()
    per = []
    for r in range(nreq):
        assert 0 <= nhits[r] <= caps[r]
        per.append(flat[hit_off[r]:hit_off[r] + nhits[r]])
        assert all(v == UNTOUCHED for v in flat[hit_off[r] + nhits[r]:hit_off[r] + caps[r]]), ("a hit beyond nhits", r)
    return status.read(), win_len, count, nhits, per, [v & U64 for v in result.read()]


def check(cd, streams, ix, requests, needles, caps, max_rows=None, scratch_cap=None, layout=None):
    """The call against the model under the same bounds (default: what admits every request)."""
    if max_rows is None or scratch_cap is None:
        rows, scratch = F.needs(streams, ix, requests, needles)
        max_rows = rows if max_rows is None else max_rows
        scratch_cap = scratch if scratch_cap is None else scratch_cap
    got = find_call(cd, streams, ix, requests, needles, caps, max_rows, scratch_cap, layout)
    want = F.find_plan(streams, ix, requests, needles, caps, max_rows, scratch_cap)
    assert got[0] == want[0], [(r, requests[r], g, w) for r, (g, w) in enumerate(zip(got[0], want[0])) if g != w][:10]
    for k, name in ((1, "win_len"), (2, "count"), (3, "nhits"), (4, "hits")):
        assert got[k] == want[k], (name, [(r, requests[r], g, w) for r, (g, w) in enumerate(zip(got[k], want[k])) if g != w][:5])
    assert got[5] == want[5], (got[5], want[5])
    return got


def check_truth(raws, requests, needles, caps, got):
    """Where the status is OK: count and hits against bytes.find over the decoded bytes (raws: what every stream decodes to)."""
    for r, ((b, ro, rl), needle) in enumerate(zip(requests, F.per_request(needles, len(requests)))):
        if got[0][r] != O.OK:
            continue
        lo, hi = R.clip(len(raws[b]), ro, rl)
        occ = [lo + p for p in F.occurrences(raws[b][lo:hi], needle)]
        assert (got[1][r], got[2][r], got[4][r]) == (hi - lo, len(occ), occ[:caps[r]]), (r, requests[r], needle)


@pytest.fixture(scope="module")
def html():
    return read_testdata("html") * 3


# ---- 1. every position -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [1, 2, 3, 15, 16, 17, 33, 256])
@pytest.mark.parametrize("cs", [1, 7, 21, 300])
def test_a_needle_at_every_position_of_a_small_buffer(cs, m):
    cd = codec()
    rng = np.random.default_rng(cs * 1000 + m)
    # the buffer holds no 0xA5 and no 0x5A; the needle begins with them: its first two bytes occur only where it is planted
    buf = bytes(int(v) for v in rng.choice([v for v in range(256) if v not in (0xA5, 0x5A)], 300))
    needle = (b"\xa5\x5a" + bytes(int(v) for v in rng.choice([v for v in range(256) if v not in (0xA5, 0x5A)], 256)))[:m]
    raws = [buf[:p] + needle + buf[p + m:] for p in range(300 - m + 1)] + [buf]
    for p, raw in enumerate(raws[:-1]):
        assert len(raw) == 300 and F.occurrences(raw, needle[:2]) == [p]    # no accidental second match of the first two bytes
    assert F.occurrences(buf, needle[:1]) == []
    streams = [K.stream_of(raw, cs) for raw in raws]
    ix = X.build_index(streams)
    reqs = [(b, *WHOLE) for b in range(len(streams))]
    got = check(cd, streams, ix, reqs, needle, [3] * len(reqs))          # one call
    assert got[0] == [O.OK] * len(reqs)
    assert got[4] == [[p] for p in range(300 - m + 1)] + [[]] and got[2] == [1] * (300 - m + 1) + [0]
    check_truth(raws, reqs, needle, [3] * len(reqs), got)


# ---- 2. overlap and period -------------------------------------------------------------------------------------------------------------------------
def test_overlapping_occurrences_and_every_interesting_cap():
    cd = codec()
    raws = [b"a" * 1000, b"ab" * 500]
    streams = [K.stream_of(raw, 7) for raw in raws]
    ix = X.build_index(streams)
    for b, needle, n in ((0, b"aaa", 998), (0, b"aa", 999), (1, b"abab", 499)):
        caps = [0, 1, n - 1, n, n + 1]
        reqs = [(b, *WHOLE)] * len(caps)
        got = check(cd, streams, ix, reqs, needle, caps)                # (find_call: untouched slots of hits keep the guard pattern)
        assert got[0] == [O.OK] * 5 and got[2] == [n] * 5 and got[3] == [0, 1, n - 1, n, n]
        step = 2 if b else 1
        assert got[4][4] == list(range(0, step * n, step))
        check_truth(raws, reqs, needle, caps, got)


# ---- 3. window edges -------------------------------------------------------------------------------------------------------------------------------
def test_needles_that_straddle_a_windows_edges_are_not_reported(html):
    cd = codec()
    names = ["long_two_spans", "tiny_chunks", "zero_length_chunks", "big_chunk", "uniform_5"]
    cases = X.named_streams()
    streams = [cases[n] for n in names]
    raws = [O.frame_decode(s) for s in streams]
    ix = X.build_index(streams)
    reqs, needles = [], []
    for b, ro, rl in X.all_windows(streams)[::3]:
        ro, rl = ro & U64, rl & U64
        lo, hi = R.clip(len(raws[b]), ro, rl)
        for m in (1, 2, 17):
            for at in (lo - 1, lo, hi - m + 1, hi - m):                  # across lo, just inside; across hi, just inside
                if 0 <= at and at + m <= len(raws[b]):
                    reqs.append((b, ro, rl))
                    needles.append(raws[b][at:at + m])
    n = len(raws[4])
    extra = [((4, 100, 16), raws[4][100:117]), ((4, 100, 17), raws[4][100:117]), ((4, 100, 0), b"x"), ((4, n, 5), b"x"), ((4, n + 9, 5), b"x"),
             ((4, n - 3, 100), raws[4][n - 3:]), ((4, n - 3, 100), raws[4][n - 4:n - 1]), ((4, U64, U64), b"x")]
    reqs += [q for q, _ in extra]
    needles += [nd for _, nd in extra]
    caps = [64] * len(reqs)
    got = check(cd, streams, ix, reqs, needles, caps)
    assert got[0] == [O.OK] * len(reqs)
    check_truth(raws, reqs, needles, caps, got)
    for r, ((b, ro, rl), nd) in enumerate(zip(reqs, needles)):
        lo, hi = R.clip(len(raws[b]), ro, rl)
        assert all(lo <= p and p + len(nd) <= hi for p in got[4][r])
    k = len(reqs) - len(extra)
    assert got[2][k:k + 2] == [0, 1] and got[1][k:k + 6] == [16, 17, 0, 0, 0, 3] and got[4][k + 5] == [n - 3] and got[2][k + 6] == 0


# ---- 4. tile borders and alignment -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cb", [4096, 65536])
def test_tile_borders_and_runs_at_odd_scratch_addresses(cb):
    cd = codec()
    T = N.FIND_TILE
    assert T == F.TILE
    n = 3 * T + 5
    rng = np.random.default_rng(cb)
    base = bytearray(int(v) for v in rng.integers(0, 200, n))            # no byte above 199
    streams = [K.stream_of(b"\xc8", cb), K.stream_of(b"\xc9\xca\xcb", cb), K.stream_of(bytes(range(201, 214)), cb)]
    raws = [b"\xc8", b"\xc9\xca\xcb", bytes(range(201, 214))]
    reqs, needles = [(0, *WHOLE), (1, *WHOLE), (2, *WHOLE)], [b"\xc8", b"\xca\xcb", bytes(range(205, 214))]
    for m in (1, 2, 17, 256):
        needle = bytes(250 - (i % 40) for i in range(m))                 # bytes above 210: only where planted
        raw = bytearray(base)
        places = []
        for border in (T, 2 * T, 3 * T):
            for p in range(border - m, border + 2):
                if p + m <= n and (not places or p >= places[-1] + m):   # planted needles do not overlap
                    raw[p:p + m] = needle
                    places.append(p)
        raws.append(bytes(raw))
        streams.append(K.stream_of(bytes(raw), cb))
        reqs.append((len(streams) - 1, *WHOLE))
        needles.append(needle)
    # every offset around every border, one stream per offset, for the needle of 17 bytes
    needle = bytes(250 - i for i in range(17))
    for border in (T, 2 * T, 3 * T):
        for p in range(border - 17, border + 2):
            if p + 17 <= n:
                raw = bytes(base[:p]) + needle + bytes(base[p + 17:])
                raws.append(raw)
                streams.append(K.stream_of(raw, cb))
                reqs.append((len(streams) - 1, *WHOLE))
                needles.append(needle)
    # two runs side by side: the last bytes of one and the first of the next form the needle, which is in neither
    left, right = bytes(base[:1000]) + b"\xfa\xfb", b"\xfc\xfd" + bytes(base[:1000])
    for raw in (left, right):
        raws.append(raw)
        streams.append(K.stream_of(raw, cb))
        reqs.append((len(streams) - 1, *WHOLE))
        needles.append(b"\xfa\xfb\xfc\xfd")
    ix = X.build_index(streams)
    caps = [40] * len(reqs)
    got = check(cd, streams, ix, reqs, needles, caps)
    assert got[0] == [O.OK] * len(reqs) and got[2][-2:] == [0, 0] and got[2][:3] == [1, 1, 1]
    assert all(c >= 1 for c in got[2][3:-2])
    check_truth(raws, reqs, needles, caps, got)
    # Tiles are cut from the window's first byte, so windows that begin at lo put the borders at lo + k T: with lo = 0 .. m the needle planted at
    # k T lies at every offset in [border - m, border] of border k, and with lo = T - 1 the one at (k + 1) T lies at border + 1
    for i, m in enumerate((1, 2, 17, 256)):
        wins = [(3 + i, lo, U64) for lo in [*range(m + 1), T - 1, T, T + 1]] + [(3 + i, lo, ln) for lo in (0, 1, 15, 16, 17) for ln in (T - 1, T, T + 1, 2 * T + 16)]
        got = check(cd, streams, ix, wins, needles[3 + i], [64] * len(wins))
        assert got[0] == [O.OK] * len(wins)
        check_truth(raws, wins, needles[3 + i], [64] * len(wins), got)


# ---- 5. many requests ------------------------------------------------------------------------------------------------------------------------------
def pack_raw(raws):
    data = torch.from_numpy(np.frombuffer(b"".join(raws) or b"\0", dtype=np.uint8).copy()).cuda()
    lens = np.array([len(x) for x in raws], dtype=np.int64)
    return data, H.dev(np.cumsum(lens) - lens), H.dev(lens)


def test_one_request_of_70000_rows_beside_70000_requests_of_one_row(html):
    cd = codec()
    n = 70000
    raw = html[3:3 + n]
    data, in_off, in_len = pack_raw([raw])
    enc = cd.frame_encode_seekable(data, in_off, in_len, chunk_bytes=1)
    assert enc[5].nentries == n
    A = (enc[0], enc[1], enc[2], enc[5])
    big = F.occurrences(raw, b"</")
    arr = np.frombuffer(raw, dtype=np.uint8)
    rs = torch.zeros(n + 1, dtype=torch.int32, device="cuda")
    ro, rl = dev_u64([0] + list(range(n))), dev_u64([U64] + [1] * n)
    needles = [b"</"] + [b"<" if i % 2 else b"e" for i in range(n)]
    cap = dev_u64([len(big)] + [1] * n)
    st, wl, count, nhits, hits, hit_off, res = cd.frame_find_indexed_result(*A, rs, ro, rl, needles, cap)
    torch.cuda.synchronize()
    assert int((st != 0).sum()) == 0 and wl.tolist() == [n] + [1] * n
    want = [len(big)] + [int(arr[i] == (0x3C if i % 2 else 0x65)) for i in range(n)]
    assert count.tolist() == want and nhits.tolist() == want
    assert hits[:len(big)].tolist() == big
    off = hit_off.tolist()
    h = hits.tolist()
    assert all(h[off[1 + i]] == i for i in range(n) if want[1 + i])
    assert res.tolist() == [2 * n, sum(want), 2 * n, n + 1]
    short = cd.frame_find_indexed(*A, rs, ro, rl, needles, cap, 2 * n, 2 * n - 1)
    assert short[0].tolist() == [O.OK] * n + [O.ERR_OUTPUT_TOO_SMALL] and short[2].tolist() == want[:n] + [0]


def test_many_requests_on_one_stream_share_needle_bytes_in_descending_stream_order(html):
    cd = codec()
    raws = [html[100:100 + 9000], html[5000:5000 + 777], html[:300]]
    streams = [K.stream_of(raws[0], 1000), K.stream_of(raws[1], 64), K.stream_of(raws[2], 300)]
    ix = X.build_index(streams)
    buf = b"<td></td>\n"                                                 # every needle is a piece of this one buffer
    pieces = [(0, 1), (0, 4), (1, 2), (4, 5), (0, 9), (3, 2), (9, 1), (5, 4), (2, 6)]
    reqs, layout_off, layout_len, needles = [], [], [], []
    for b in (2, 1, 0):                                                 # descending stream order
        for k, (o, ln) in enumerate(pieces):
            reqs.append((b, *WHOLE) if k % 2 else (b, 50 * k, 4000))
            layout_off.append(o)
            layout_len.append(ln)
            needles.append(buf[o:o + ln])
    caps = [500] * len(reqs)
    got = check(cd, streams, ix, reqs, needles, caps, layout=(buf, layout_off, layout_len))
    assert got[0] == [O.OK] * len(reqs) and sum(got[2]) > 100
    check_truth(raws, reqs, needles, caps, got)


# ---- 6. statuses -----------------------------------------------------------------------------------------------------------------------------------
def test_unsound_indexes_give_the_models_statuses_and_write_nowhere_else():
    cd = codec()
    streams = list(X.named_streams().values())
    ns = len(streams)
    ix = X.build_index(streams)
    windows = [(b, ro & U64, rl & U64) for b, ro, rl in X.all_windows(streams)]
    reqs = windows[::9] + [(ns, 0, 10), (0xFFFFFFFF, 5, 5)]
    needles = [(b"\n", b"<a", b"e", b"the ")[r % 4] for r in range(len(reqs))]
    caps = [8] * len(reqs)
    rng = np.random.default_rng(11)
    refused = 0
    check(cd, streams, ix, reqs, needles, caps)
    for index in unsound_indexes(ix, streams, rng):
        rows, scratch = F.needs(streams, index, reqs, needles)
        got = check(cd, streams, index, reqs, needles, caps, min(rows, 1 << 20), min(scratch, 1 << 24))   # (find_call checks the guard words)
        refused += got[0].count(O.ERR_BAD_ARG)
    assert refused > 300


def test_corruption_inside_the_window_is_the_reads_status_and_outside_it_is_not_noticed():
    cd = codec()
    raw = bytes(np.random.default_rng(8).integers(0, 256, 64 * 6, dtype=np.uint8))
    s = K.stream_of(raw, 64)
    rows = R.walk(s)[0]
    ix = X.build_index([s])
    needle = raw[200:203]
    body = R.corrupt_chunk(s, rows[2])                                  # a corrupt body in chunk 2: bytes [128, 192)
    p = ix["pos"][4] + 4
    crc = s[:p] + bytes([s[p] ^ 0x10]) + s[p + 1:]                       # a corrupt CRC in the header of chunk 4: bytes [256, 320)
    cut = s[:-5]                                                        # a truncated tail: the last chunk's body is short
    tix = X.build_index([cut])
    assert tix["tail"] == [O.ERR_TRUNCATED_STREAM] and len(tix["start"]) == 5
    reqs = [(0, *WHOLE), (0, 192, 64), (0, 190, 10), (0, 100, 28), (0, 320, 64), (0, 250, 10), (0, 0, 128), (0, 200, 3)]
    for stream, index, bad_rows in ((body, ix, {2}), (crc, ix, {4}), (cut, tix, None)):
        got = check(cd, [stream], index, reqs, needle, [4] * len(reqs))
        for r, (_, ro, rl) in enumerate(reqs):
            lo, hi = R.clip(index["total"][0], ro, rl)
            if bad_rows is None:
                assert got[0][r] == O.ERR_TRUNCATED_STREAM               # the strict tail rule: every window of the stream
                continue
            meets = any(lo < 64 * (k + 1) and hi > 64 * k for k in bad_rows)
            assert (got[0][r] != O.OK) == meets, (r, got[0][r])
        if bad_rows is not None:
            check_truth([raw], [q for q in reqs], needle, [4] * len(reqs), got)
            assert got[4][7] == [200]                                   # a failing request beside OK ones leaves theirs intact


def test_foreign_streams_bad_needles_and_streams_that_were_not_indexed():
    cd = codec()
    frames = G.frame_corpus()
    streams = [s for _n, s, _r in frames] + [R.tiny_chunk_stream(1)[0], R.zero_length_chunk_stream()[0], R.big_chunk_stream()[0]]
    raws = [b"".join(r) for _n, _s, r in frames] + [R.tiny_chunk_stream(1)[1], R.zero_length_chunk_stream()[1], R.big_chunk_stream()[1]]
    unsound = {b for b, (name, _s, _r) in enumerate(frames) if name in ("mutated-chunk", "wrong-crc")}
    ns = len(streams)
    ix = X.build_index(streams)
    reqs, needles = [], []
    for b in range(ns):
        nd = raws[b][len(raws[b]) // 2:len(raws[b]) // 2 + 3] or b"x"
        reqs += [(b, *WHOLE), (b, 3, 500), (b, 1, 400)]
        needles += [nd, nd[:1], nd[:2] or b"y"]
    reqs += [(ns, 0, 10), (0, *WHOLE), (0, *WHOLE), (ns - 1, *WHOLE), (0xFFFFFFFF, 0, 1)]
    needles += [b"x", b"", b"x" * 257, b"x" * 256, b"x"]
    caps = [16] * len(reqs)
    got = check(cd, streams, ix, reqs, needles, caps)
    assert got[0][-5:] == [O.ERR_BAD_ARG, O.ERR_BAD_ARG, O.ERR_BAD_ARG, O.OK, O.ERR_BAD_ARG]
    sound = [r for r, q in enumerate(reqs) if q[0] < ns and q[0] not in unsound and got[0][r] == O.OK]
    assert len(sound) > 15
    check_truth(raws, [reqs[r] for r in sound], [needles[r] for r in sound], [16] * len(sound), [[x[r] for r in sound] for x in got[:5]])
    # an index that holds only the first streams: the others were not indexed
    part = X.build_index(streams, max_entries=ix["first"][ns // 2])
    assert O.ERR_OUTPUT_TOO_SMALL in part["tail"]
    got = check(cd, streams, part, reqs, needles, caps)
    assert all(got[0][r] == O.ERR_OUTPUT_TOO_SMALL for r, q in enumerate(reqs[:-5]) if part["tail"][q[0]] == O.ERR_OUTPUT_TOO_SMALL)


# ---- 7. admission and sizing -----------------------------------------------------------------------------------------------------------------------
def test_each_bound_admits_exactly_the_first_k_requests_and_one_sizing_round_fits_exactly(html):
    cd = codec()
    raw = html[:700 * 9]
    streams = [K.stream_of(raw, 500), K.stream_of(raw, 700)]
    ix = X.build_index(streams)
    reqs = [(0, *WHOLE), (1, *WHOLE), (0, 10, 1000), (0, 0, 0), (7, 0, 1), (1, 699, 2), (0, 3000, 800)]
    nreq = len(reqs)
    needle = b"<"
    caps = [5] * nreq
    per = [F.needs(streams, ix, [q], needle) for q in reqs]
    per_rows, per_bytes = [p[0] for p in per], [p[1] for p in per]
    rows, scratch = sum(per_rows), sum(per_bytes)
    sizing = find_call(cd, streams, ix, reqs, needle, caps, 0, 0)        # the one sizing round
    assert sizing[5][0] == rows and sizing[5][2] == scratch and (rows, scratch) == F.needs(streams, ix, reqs, needle)
    full = check(cd, streams, ix, reqs, needle, caps, rows, scratch)
    assert full[0] == [O.OK] * 4 + [O.ERR_BAD_ARG] + [O.OK] * 2 and full[5] == [rows, sum(full[2]), scratch, nreq - 1]
    check_truth([raw, raw], reqs[:4] + reqs[5:], needle, caps[1:], [x[:4] + x[5:] for x in full[:5]])
    for k in range(nreq + 1):
        for bound, each in ((0, per_rows), (1, per_bytes)):
            for delta in (-1, 0, 1):                                    # one below what is needed, exactly at it, one above
                cap = sum(each[:k]) + delta
                if cap < 0:
                    continue
                got = check(cd, streams, ix, reqs, needle, caps, cap if bound == 0 else rows, scratch if bound == 0 else cap)
                admitted = max(i for i in range(nreq + 1) if sum(each[:i]) <= cap)
                assert got[0] == full[0][:admitted] + [O.ERR_OUTPUT_TOO_SMALL] * (nreq - admitted)
                assert got[5][0] == rows and got[5][2] == scratch
    # no request at all: d_result is still written
    FL = N.frame_find_lib()
    result = Guarded(4, torch.int64)
    assert FL.snp_frame_find_indexed_batch(cd.ctx.handle, *[None] * 3, 0, *[None] * 5, 0, *[None] * 3, 0, *[None] * 3, 0, 0, *[None] * 3,
                                           *[None] * 4, None, result.ptr()) == O.OK
    torch.cuda.synchronize()
    assert result.read() == [0, 0, 0, 0]


# ---- 8. past 2^32 ----------------------------------------------------------------------------------------------------------------------------------
def test_a_window_past_4_gib_gives_64_bit_positions():
    if torch.cuda.mem_get_info()[0] < (3 << 30):
        pytest.skip("needs 3 GiB of free device memory")
    cd = codec()
    needle = b"NEEDLE!"
    zeros = np.zeros(B, dtype=np.uint8)
    variants = {"Z": zeros.copy(), "A": zeros.copy(), "L": zeros.copy(), "R": zeros.copy()}
    variants["A"][100:107] = np.frombuffer(needle, dtype=np.uint8)
    variants["L"][B - 3:] = np.frombuffer(needle[:3], dtype=np.uint8)    # ... on a chunk border: three bytes here, four in the next chunk
    variants["R"][:4] = np.frombuffer(needle[3:], dtype=np.uint8)
    ident, chunk = None, {}
    for name, buf in variants.items():
        one = cd.frame_encode_seekable(torch.from_numpy(buf).cuda(), dev_u64([0]), dev_u64([B]), chunk_bytes=B)
        n1 = int(one[2].item())
        ident, chunk[name] = one[0][:10], one[0][10:n1]
    first = 65536                                                       # the chunk that begins at 2^32
    count = first + 24
    special = {first + 2: "A", first + 4: "L", first + 5: "R", first + 14: "A"}
    framed = torch.cat([ident, chunk["Z"].repeat(first + 2)] + [chunk[special.get(k, "Z")] for k in range(first + 2, count)])
    in_off, in_len = dev_u64([0]), dev_u64([framed.numel()])
    index = cd.frame_index_buffers(framed, in_off, in_len)
    assert index.total.tolist() == [count * B] and index.tail.tolist() == [O.OK] and index.nentries == count
    want = [(first + 2) * B + 100, (first + 5) * B - 3, (first + 14) * B + 100]
    assert all(p > 1 << 32 for p in want)
    rs = torch.zeros(2, dtype=torch.int32, device="cuda")
    ro, rl = dev_u64([(1 << 32) + 5] * 2), dev_u64([1 << 20] * 2)
    st, wl, cnt, nhits, hits, hit_off, res = cd.frame_find_indexed_result(framed, in_off, in_len, index, rs, ro, rl, [needle, b"\0"], dev_u64([8, 0]))
    assert st.tolist() == [O.OK, O.OK] and wl.tolist() == [1 << 20] * 2
    assert cnt.tolist() == [3, (1 << 20) - 3 * len(needle)] and nhits.tolist() == [3, 0] and hits[:3].tolist() == want
    assert res.tolist() == [2 * 17, 3 + (1 << 20) - 21, 2 * 17 * B, 2]


# ---- 9. graph capture ------------------------------------------------------------------------------------------------------------------------------
def test_graph_capture_replays_the_call_on_changed_needle_bytes(html):
    cd = codec()
    cb = 4096
    raws = [html[:5 * cb + 9], html[100:100 + 3 * cb]]
    streams = [K.stream_of(r, cb) for r in raws]
    ix = X.build_index(streams)
    reqs = [(0, *WHOLE), (1, *WHOLE), (0, cb - 1, cb + 2), (1, 7, 2 * cb)]
    nreq, cap = 4, 50
    sets = [[b"<td", b"\n", b"</", b"e"], [b"the", b"<", b"ab", b"\n"]]   # the same lengths: only the bytes change
    mr, sc = 64, 1 << 17
    tabs = stream_tensors(streams, ix)[0]
    index = SB.FrameIndex(*tabs[3:])
    rq = [dev_i32([q[0] for q in reqs]), dev_u64([q[1] for q in reqs]), dev_u64([q[2] for q in reqs])]
    packed = [F.pack_needles(s) for s in sets]
    assert packed[0][1:] == packed[1][1:]
    live = (torch.zeros(len(packed[0][0]), dtype=torch.uint8, device="cuda"), dev_u64(packed[0][1]), dev_i32(packed[0][2]))
    bufs = [torch.from_numpy(np.frombuffer(p[0], dtype=np.uint8).copy()).cuda() for p in packed]
    work = torch.empty(N.frame_find_lib().snp_frame_find_indexed_workspace(nreq, mr, sc), dtype=torch.uint8, device="cuda")

    def call():
        return cd.frame_find_indexed_result(tabs[0], tabs[1], tabs[2], index, *rq, live, cap, mr, sc, work)

    live[0].copy_(bufs[0])
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
        outs = call()
    for k in (0, 1, 0):
        live[0].copy_(bufs[k])
        outs[0].fill_(-1)
        g.replay()
        torch.cuda.synchronize()
        want = F.find_plan(streams, ix, reqs, sets[k], [cap] * nreq, mr, sc)
        st, wl, cnt, nh, hits, off, res = [x.tolist() for x in outs]
        assert (st, wl, cnt, nh, res) == (want[0], want[1], want[2], want[3], want[5]) and st == [O.OK] * nreq
        assert [hits[off[r]:off[r] + nh[r]] for r in range(nreq)] == want[4]
        if k == 0:
            assert all(torch.equal(x, y) for x, y in zip(plain[:4], outs[:4]))


# ---- 10. the wrappers ------------------------------------------------------------------------------------------------------------------------------
def test_wrappers_size_the_call_and_cut_streams_into_windows(html):
    cd = codec()
    raws = [html[:300000], html[1000:1000 + 70000], b"", html[:100], b"ab" * 100000]
    needle = b"</td>"
    T = 65536                                                           # the windows of scratch_bytes = 2 * 65536
    raws[0] = raws[0][:T - 2] + needle + raws[0][T + 3:2 * T - 4] + needle + raws[0][2 * T + 1:]    # occurrences across the windows' seams
    data, in_off, in_len = pack_raw(raws)
    enc = cd.frame_encode_seekable(data, in_off, in_len, chunk_bytes=4096)
    A = (enc[0], enc[1], enc[2], enc[5])
    truth = [F.occurrences(r, needle) for r in raws]
    assert T - 2 in truth[0] and 2 * T - 4 in truth[0] and len(truth[0]) > 200
    ns = len(raws)
    rs = torch.arange(ns, dtype=torch.int32, device="cuda")
    ro, rl = dev_u64([0] * ns), dev_u64([U64] * ns)
    st, wl, cnt, nh, hits, off = cd.frame_find_indexed(*A, rs, ro, rl, needle, 10000)       # default bounds: the wrapper sizes the call
    assert st.tolist() == [O.OK] * ns and wl.tolist() == [len(r) for r in raws] and cnt.tolist() == [len(t) for t in truth]
    assert [hits[o:o + k].tolist() for o, k in zip(off.tolist(), nh.tolist())] == truth
    count, found, status = cd.frame_find_streams(*A, needle, scratch_bytes=2 * T)
    assert status.tolist() == [O.OK] * ns and count.tolist() == [len(t) for t in truth] and [f.tolist() for f in found] == truth
    cut = len([p for p in truth[0] if p < T]) + 3                       # max_hits cuts inside a later window
    count, found, status = cd.frame_find_streams(*A, needle, max_hits=cut, scratch_bytes=2 * T)
    assert count.tolist() == [len(t) for t in truth] and [f.tolist() for f in found] == [t[:cut] for t in truth]
    count, found, status = cd.frame_find_streams(*A, b"ab", scratch_bytes=3 * T)          # more hits than the wrapper's first guess
    assert count.tolist()[4] == 100000 and found[4].tolist() == list(range(0, 200000, 2))
    assert [f.tolist() for f in found[:4]] == [F.occurrences(r, b"ab") for r in raws[:4]]

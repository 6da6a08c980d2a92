"""libsnappier_hip_frame_cuts.so on the GPU: snp_content_cuts_batch against the model (frame_cuts_model.py) element for element at the windows,
lengths and contents where the finder changes path -- its tile, its blocks, a lane's run, ties, the ends of the eligible range; its admission,
sizing round and bounds; one buffer past 4 GiB; snp_frame_encode_cuts_batch against the model and, at regular cuts, against
snp_frame_encode_chunked_batch byte for byte; untrusted cut lists; content-defined streams of a buffer and of its edited copy end to end; graph
capture of both calls.  The calls are made directly, every array and the workspace between guard words, the output arena canary-filled.
Needs an MI355X."""
import numpy as np
import pytest
import torch

import frame_buffers_helpers as H
import frame_chunked_model as K
import frame_cuts_model as F
import oracle as O
from conftest import read_testdata
from seekable_harness import CANARY, KEYS, UNTOUCHED, Encoded, Guarded, _p, dev_u64

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from snappier_amd import batch as SB, _native as N

VARIANTS = [O.HASH_CRC32C, O.HASH_MUL]
U64 = (1 << 64) - 1


@pytest.fixture(scope="module")
def content():
    html = read_testdata("html") * 4
    rnd = np.random.default_rng(3).integers(0, 256, 400000, dtype=np.uint8).tobytes()
    period = np.random.default_rng(1).integers(0, 256, 64, dtype=np.uint8).tobytes() * 4096
    return html, rnd, period


def cd_of(variant=O.HASH_CRC32C):
    return SB.BlockCodec(0, variant)


# ---- the two calls, made directly ------------------------------------------------------------------------------------------------------------------
def found(cd, blobs, w, mx, span=None, max_cuts=None, lead=1, gap=3):
    """snp_content_cuts_batch with every array guarded: -> the dict the model's find() gives."""
    nb = len(blobs)
    CL = N.frame_cuts_lib()
    cd._bind()
    data, in_off, lens = H.pack(blobs, lead, gap)
    span = sum(len(x) for x in blobs) if span is None else span
    mc = F.find(blobs, w, mx, span)["result"][0] if max_cuts is None else max_cuts
    first, cuts, status, result = Guarded(nb + 1, torch.int64), Guarded(mc, torch.int64), Guarded(nb, torch.int32), Guarded(4, torch.int64)
    work = Guarded(CL.snp_content_cuts_workspace(nb, span, w), torch.uint8)
    tabs = [H.dev(in_off), H.dev(lens)]
    st = CL.snp_content_cuts_batch(cd.ctx.handle, _p(data), _p(tabs[0]), _p(tabs[1]), nb, w, mx, span, mc, first.ptr(), cuts.ptr(), status.ptr(),
                                   work.ptr(), result.ptr())
    assert st == O.OK
    torch.cuda.synchronize()
    work.read()
    got = {"cut_first": first.read(), "cuts": cuts.read(), "status": status.read(), "result": result.read()}
    used = got["cut_first"][nb]
    assert 0 <= used <= mc and all(v == UNTOUCHED for v in got["cuts"][used:]), "a cut beyond cut_first[nbuffers]"
    got["cuts"] = got["cuts"][:used]
    return got


def check_found(cd, blobs, w, mx, **kw):
    got = found(cd, blobs, w, mx, **kw)
    want = F.find(blobs, w, mx, kw.get("span"), kw.get("max_cuts"))
    for key in ("status", "cut_first", "result", "cuts"):
        assert got[key] == want[key], (w, mx, key, [len(x) for x in blobs])
    for b, x in enumerate(blobs):                                       # the documented bound that spares the sizing round
        if want["status"][b] == O.OK:
            assert want["cut_first"][b + 1] - want["cut_first"][b] <= F.cut_bound(len(x), w, mx)
    return want


class EncodedAt:
    """snp_frame_encode_cuts_batch made directly, as seekable_harness.Encoded makes the chunked call: .got is what the model's encode_at_cuts gives."""

    def __init__(self, cd, blobs, cut_first, cuts, max_chunks=None, stage_cap=None, caps=None, with_index=True, ncuts=None):
        nb = len(blobs)
        CL = N.frame_cuts_lib()
        cd._bind()
        self.data, in_off, lens = H.pack(blobs)
        free = F.encode_at_cuts(blobs, cut_first, cuts, ncuts=ncuts, with_index=False) if max_chunks is None or stage_cap is None else None
        mc = free["result"][0] if max_chunks is None else max_chunks
        if stage_cap is None:
            sc = sum(F.stride(ln) for b in range(nb) for _, ln in F.list_verdict(len(blobs[b]), cut_first[b], cut_first[b + 1], cuts, ncuts)[1])
        else:
            sc = stage_cap
        pieces = [max(0, min(cut_first[b + 1], len(cuts)) - min(cut_first[b], len(cuts))) + 1 for b in range(nb)]
        caps = np.array([10 + 8 * p + len(x) for p, x in zip(pieces, blobs)] if caps is None else caps, dtype=np.int64)
        self.out_off, total = H.out_layout(caps)
        self.out = torch.full((total,), CANARY, dtype=torch.uint8, device="cuda")
        self.mc, self.sc = mc, sc
        self.out_len, self.status, self.result = Guarded(nb, torch.int64), Guarded(nb, torch.int32), Guarded(4, torch.int64)
        self.ix = [Guarded(nb + 1, torch.int64), Guarded(mc, torch.int64), Guarded(mc, torch.int64), Guarded(nb, torch.int64), Guarded(nb, torch.int32)]
        work = Guarded(CL.snp_frame_encode_cuts_workspace(nb, mc, sc), torch.uint8)
        nc = len(cuts) if ncuts is None else ncuts
        d_cuts = Guarded(len(cuts), torch.int64)
        if cuts:
            d_cuts.mid.copy_(dev_u64(cuts))
        self.tabs = [H.dev(in_off), H.dev(lens), H.dev(self.out_off), H.dev(caps), dev_u64(cut_first)]
        ixp = [g.ptr() for g in self.ix] if with_index else [None] * 5
        st = CL.snp_frame_encode_cuts_batch(cd.ctx.handle, _p(self.data), _p(self.tabs[0]), _p(self.tabs[1]), nb, _p(self.tabs[4]),
                                            d_cuts.ptr() if nc else None, nc, mc, sc, _p(self.out), _p(self.tabs[2]), _p(self.tabs[3]),
                                            self.out_len.ptr(), self.status.ptr(), *ixp, work.ptr(), self.result.ptr())
        assert st == O.OK
        torch.cuda.synchronize()
        work.read()
        d_cuts.read()
        status, out_len = self.status.read(), self.out_len.read()
        self.h = self.out.cpu().numpy()
        assert (H.outside_ranges(self.h, self.out_off, out_len) == CANARY).all(), "a write outside the output ranges"
        streams = [self.h[o:o + n].tobytes() if s == O.OK else None for s, n, o in zip(status, out_len, self.out_off.tolist())]
        self.got = {"status": status, "out_len": out_len, "streams": streams, "result": self.result.read(), **{k: [] for k in KEYS}}
        index = [g.read() for g in self.ix]
        if with_index:
            used = index[0][nb]
            assert 0 <= used <= mc and all(v == UNTOUCHED for v in index[1][used:] + index[2][used:]), "a row beyond the index"
            index[1], index[2] = index[1][:used], index[2][:used]
            self.got.update(zip(KEYS, index))
        else:
            assert all((g.t.view(torch.uint8) == CANARY).all() for g in self.ix), "an index array written without an index"

    def frame_index(self):
        return SB.FrameIndex(*[g.mid for g in self.ix], None)


def check_encoded(cd, blobs, cut_first, cuts, variant, read=True, **kw):
    e = EncodedAt(cd, blobs, cut_first, cuts, **kw)
    want = F.encode_at_cuts(blobs, cut_first, cuts, variant, kw.get("max_chunks"), kw.get("stage_cap"), kw.get("caps"), ncuts=kw.get("ncuts"))
    for key in want:
        assert e.got[key] == want[key], key
    if want["status"] != [O.OK] * len(blobs) or not blobs:
        return e, want
    d_off, d_len = H.dev(e.out_off), e.out_len.mid
    walked = cd.frame_index_buffers(e.out, d_off, d_len)               # the emitted index is the walk's
    for key, g in zip(KEYS, e.ix):
        used = want["result"][2] if key in ("start", "pos") else g.n
        assert torch.equal(getattr(walked, key)[:used], g.mid[:used]), key
    if read:                                                            # every buffer whole, and a window across its second cut, through the emitted index
        reqs = [(b, 0, len(x)) for b, x in enumerate(blobs)]
        reqs += [(b, max(cuts[cut_first[b] + 1] - 3, 0), 7) for b in range(len(blobs)) if cut_first[b + 1] - cut_first[b] > 1]
        expect = [blobs[b][ro:ro + rl] for b, ro, rl in reqs]
        caps = np.array([len(x) for x in expect], dtype=np.int64)
        r_off, total = H.out_layout(caps)
        arena = torch.full((total,), CANARY, dtype=torch.uint8, device="cuda")
        ol, st, _ = cd.frame_read_indexed(e.out, d_off, d_len, e.frame_index(), torch.tensor([r[0] for r in reqs], dtype=torch.int32, device="cuda"),
                                          H.dev([r[1] for r in reqs]), H.dev([r[2] for r in reqs]), arena, H.dev(r_off), H.dev(caps))
        torch.cuda.synchronize()
        assert st.tolist() == [O.OK] * len(reqs) and ol.tolist() == caps.tolist()
        h = arena.cpu().numpy()
        for x, o in zip(expect, r_off.tolist()):
            assert h[o:o + len(x)].tobytes() == x
        assert (H.outside_ranges(h, r_off, caps) == CANARY).all()
    return e, want


# ---- 1: the finder against the model ---------------------------------------------------------------------------------------------------------------
def peaks(w: int, n: int):
    """n bytes whose largest hash sits at the first and at the last eligible position, w + 1 and n - w - 1: zeros, and one 32-byte string in
    front of either position, chosen so that the model agrees."""
    assert n - w - 1 - (w + 1) > w
    rng = np.random.default_rng(w)
    strings = [rng.integers(0, 256, 32, dtype=np.uint8).tobytes() for _ in range(2000)]
    for s in sorted(strings, key=lambda s: -int(F.hashes(s)[32]))[:20]:
        x = bytearray(n)
        x[w + 1 - 32:w + 1] = s
        x[n - w - 1 - 32:n - w - 1] = s
        got = F.content_cuts(bytes(x), w)
        if got and got[0] == w + 1 and got[-1] == n - w - 1:
            return bytes(x)
    raise AssertionError("no string found")


WINDOWS = [(32, 33), (32, 65536), (33, 34), (33, 4096), (64, 65), (64, 1024), (1000, 1001), (1000, 4096), (4096, 4097), (4096, 65536),
           (32767, 32768), (32767, 65536)]


@pytest.mark.parametrize("w,mx", WINDOWS)
def test_finder_against_the_model(content, w, mx):
    html, rnd, period = content
    T, R = N.CUTS_TILE, N.CUTS_RUN
    ends = [0, 1, 2 * w + 1, 2 * w + 2, 2 * w + 3]
    # w, n - w and the buffer's end on either side of a tile seam, of a block seam and of a lane's run
    ends += [w + T - 1, w + T, w + T + 1, w + 2 * T + 64, 2 * T - 1, 2 * T, 2 * T + 1, 2 * T + R, 3 * T - 64 + R - 1, w + T + 63, w + T + 65]
    if w > 4096:                                                        # (every length is tens of KiB here: fewer of them)
        ends = [0, 1, 2 * w + 1, 2 * w + 2, 2 * w + 3, w + T - 1, w + T + 1, 2 * T + R]
    big = max(4 * w + 2 * T + 5, 50000)
    blobs = [html[7:7 + n] for n in ends] + [rnd[3:3 + n] for n in ends[2:] if w <= 4096]
    blobs += [html[:big], rnd[:2 * w + T + 100], bytes(big), period[:big], peaks(w, 3 * w + 40), peaks(w, 3 * w + T + 64)]
    if 2 * w < T - 1:                                                   # the last maximum just before, at and just behind the first tile seam
        blobs += [peaks(w, T + w + d) for d in (0, 1, 2)]
    assert sum(len(x) for x in blobs) < (1 << 20) + (1 << 18)
    want = check_found(cd_of(), blobs, w, mx)
    assert want["status"] == [O.OK] * len(blobs) and want["result"][1] > 0


@pytest.mark.parametrize("w", [40, 100])
def test_finder_on_a_period_shorter_and_longer_than_the_window(content, w):
    """A 64-byte period: at w = 100 every value ties with one to its left, so every cut is forced; at w = 40 the cuts are content cuts 64 apart."""
    _, _, period = content
    blobs = [period[:200000], period[5:5 + 3 * N.CUTS_TILE + 1], period[63:63 + 2 * w + 3]]
    want = check_found(cd_of(), blobs, w, 4096)
    c = want["cuts"][:want["cut_first"][1]]
    steps = {b - a for a, b in zip(c, c[1:])}
    assert steps == ({4096} if w == 100 else {64}) and len(c) > 40


def test_finder_on_many_buffers_at_unaligned_offsets(content):
    html, rnd, _ = content
    rng = np.random.default_rng(11)
    blobs = []
    for i in range(300):
        n = int(rng.integers(0, 9000))
        o = int(rng.integers(0, 100000))
        blobs.append((html if i % 3 else rnd)[o:o + n])
    for lead, gap in ((1, 3), (16, 0), (7, 1)):
        check_found(cd_of(), blobs, 64, 1024, lead=lead, gap=gap)
    check_found(cd_of(), blobs, 1000, 4096)


# ---- 2: the finder's admission ---------------------------------------------------------------------------------------------------------------------
def test_finder_admission_sizing_and_bad_arguments(content):
    html, rnd, _ = content
    cd = cd_of()
    w, mx = 64, 1024
    blobs = [html[:9000], rnd[:5000], b"", html[3:3 + 20000], rnd[:100], b"", html[:4097]]
    full = check_found(cd, blobs, w, mx)
    need, nbytes = full["result"][0], sum(len(x) for x in blobs)
    assert full["result"] == [need, need, nbytes, len(blobs)]
    sizing = check_found(cd, blobs, w, mx, max_cuts=0)                  # the sizing round: every count, no cut written
    assert sizing["result"] == [need, 0, nbytes, 0] and sizing["status"] == [O.ERR_OUTPUT_TOO_SMALL] * len(blobs)
    check_found(cd, blobs, w, mx, max_cuts=need + 5)
    short = check_found(cd, blobs, w, mx, max_cuts=need - 1)            # one short: the last buffer, which has cuts
    assert short["status"] == [O.OK] * 6 + [O.ERR_OUTPUT_TOO_SMALL] and short["result"] == [need, full["cut_first"][6], nbytes, 6]
    mid = check_found(cd, blobs, w, mx, max_cuts=full["cut_first"][3])  # exactly the first three
    assert mid["status"] == [O.OK] * 3 + [O.ERR_OUTPUT_TOO_SMALL] * 4 and mid["cut_first"][3:] == [full["cut_first"][3]] * 5
    span = check_found(cd, blobs, w, mx, span=14000 + 19999)            # bytes: the 20 000-byte buffer misses by one
    assert span["status"] == [O.OK] * 3 + [O.ERR_OUTPUT_TOO_SMALL] * 4 and span["result"] == [full["cut_first"][3], full["cut_first"][3], nbytes, 3]
    check_found(cd, blobs, w, mx, span=0)
    check_found(cd, [b"", b""], w, mx, span=0, max_cuts=0)              # empty buffers are OK with no cut
    # nbuffers == 0: only ctx and d_result, and cut_first[0] when given
    CL = N.frame_cuts_lib()
    cd._bind()
    for given in (False, True):
        result, first = Guarded(4, torch.int64), Guarded(1, torch.int64)
        assert CL.snp_content_cuts_batch(cd.ctx.handle, None, None, None, 0, w, mx, 0, 0, first.ptr() if given else None, None, None, None,
                                         result.ptr()) == O.OK
        torch.cuda.synchronize()
        assert result.read() == [0] * 4 and first.read() == ([0] if given else [UNTOUCHED])
    result = Guarded(4, torch.int64)
    for bw, bmx in ((31, 1024), (32768, 65536), (64, 64), (64, 65537), (0, 0), (100, 50)):
        assert CL.snp_content_cuts_batch(cd.ctx.handle, None, None, None, 0, bw, bmx, 0, 0, None, None, None, None, result.ptr()) == O.ERR_BAD_ARG
    assert result.read() == [UNTOUCHED] * 4


# ---- 3: past 4 GiB ---------------------------------------------------------------------------------------------------------------------------------
def test_finder_on_one_buffer_past_4_gib():
    n = (1 << 32) + 100000
    free = torch.cuda.mem_get_info()[0]
    if free < 6 << 30:
        pytest.skip(f"needs 6 GiB of free device memory, {free >> 30} GiB free")
    cd = cd_of()
    src = torch.zeros(n, dtype=torch.uint8, device="cuda")
    cut_first, cuts, status, result = cd.content_cuts(src, H.dev([0]), H.dev([n]), 32, 65536)
    want = (n - 1) // 65536
    assert status.tolist() == [O.OK] and cut_first.tolist() == [0, want] and result.tolist() == [want, want, n, 1]
    assert torch.equal(cuts[:want], torch.arange(1, want + 1, dtype=torch.int64, device="cuda") * 65536)
    assert int(cuts[want - 2]) == 1 << 32 and int(cuts[want - 1]) == (1 << 32) + 65536            # (the cuts go on past 2^32)


# ---- 4: encode at cuts against the model -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", VARIANTS)
def test_encode_at_found_and_hand_made_cuts(content, variant):
    html, rnd, _ = content
    cd = cd_of(variant)
    blobs = [html[:70000], b"", rnd[:9000] + html[:30000], html[5:6], html[100:100 + 200001]]
    f = found(cd, blobs, 64, 1024)
    check_encoded(cd, blobs, f["cut_first"], f["cuts"], variant)
    f = found(cd, blobs, 2048, 16384)
    check_encoded(cd, blobs, f["cut_first"], f["cuts"], variant)
    # hand-made: pieces of 1 byte, of 65 536, and of the sizes where the compressor changes path
    sizes = [1, 1, 65536, 1] + K.CHUNK_SIZES + [65536, 3, 65535]
    first, cuts, big = [0], [], html[:sum(sizes)]
    at = 0
    for s in sizes[:-1]:
        at += s
        cuts.append(at)
    first.append(len(cuts))
    ones = list(range(1, 300))
    check_encoded(cd, [big, html[:300], rnd[:65536], b""], first + [len(cuts) + len(ones)] * 3, cuts + ones, variant)


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("cb", [1000, 4096, 65536])
def test_regular_cuts_give_the_chunked_call_byte_for_byte(content, cb, variant):
    html, rnd, _ = content
    cd = cd_of(variant)
    blobs = [html[:n] for n in K.buffer_lengths(cb)] + [rnd[:min(2 * cb + 3, 70001)], (html + rnd[:50000])[:300000]]
    first, cuts = F.regular_cuts([len(x) for x in blobs], cb)
    for with_index in (True, False):
        ref = Encoded(cd, blobs, cb, with_index=with_index)
        e = EncodedAt(cd, blobs, first, cuts, caps=[K.frame_cap(len(x), cb) for x in blobs], with_index=with_index)
        assert np.array_equal(e.out_off, ref.out_off) and np.array_equal(e.h, ref.h)      # the whole arena, canaries included
        assert e.got == ref.got
    assert ref.got == K.encode(blobs, cb, variant, with_index=False)
    check_encoded(cd, blobs, first, cuts, variant, caps=[K.frame_cap(len(x), cb) for x in blobs])


# ---- 5: untrusted cuts, and the bounds ---------------------------------------------------------------------------------------------------------------
def test_bad_cut_lists_fail_their_buffer_alone(content):
    html, rnd, _ = content
    cd = cd_of()
    n = 5000
    good = [1000, 2000, 4999]
    lists = {"unsorted": [1000, 3000, 2000], "repeated": [1000, 2000, 2000], "zero": [0, 1000], "at n": [1000, n], "past n": [1000, n + 1],
             "all ones": [1000, U64], "wrapped": [U64 - 5, 1000]}
    for name, bad in lists.items():
        blobs = [html[:n], rnd[:n], html[7:7 + n]]
        first, cuts = [0, 3, 3 + len(bad), 6 + len(bad)], good + bad + good
        e, want = check_encoded(cd, blobs, first, cuts, O.HASH_CRC32C)
        assert want["status"] == [O.OK, O.ERR_BAD_ARG, O.OK] and want["first"] == [0, 4, 4, 8] and want["result"][0] == 8, name
        assert want["tail"][1] == O.ERR_BAD_ARG and want["total"][1] == 0
    # a piece of 65 537 bytes: in front, in the middle, behind, and the whole buffer
    long = html[:140000]
    for bad in ([65537], [10, 65547], [140000 - 65537], []):
        blobs = [html[:n], long if bad else long[:65537], rnd[:n]]
        e, want = check_encoded(cd, blobs, [0, 3, 3 + len(bad), 6 + len(bad)], good + bad + good, O.HASH_CRC32C)
        assert want["status"] == [O.OK, O.ERR_BAD_ARG, O.OK], bad
    check_encoded(cd, [long[:65536], long[:65537]], [0, 0, 1], [1], O.HASH_CRC32C)       # (65 536 is good)
    # cut_first decreasing, and beyond ncuts: the buffers whose own range is bad
    blobs = [html[:n], rnd[:n], html[7:7 + n], rnd[9:9 + n]]
    e, want = check_encoded(cd, blobs, [0, 3, 2, 3, 6], good + good, O.HASH_CRC32C)
    assert want["status"] == [O.OK, O.ERR_BAD_ARG, O.OK, O.OK]                            # (3 > 2 at buffer 1 alone; buffer 2 has cuts[2:3] = [4999])
    e, want = check_encoded(cd, blobs, [0, 3, 6, 7, 7], good + good + [1000, 2000], O.HASH_CRC32C, ncuts=6)
    assert want["status"] == [O.OK, O.OK, O.ERR_BAD_ARG, O.ERR_BAD_ARG]                   # (7 > ncuts = 6, at both)
    e, want = check_encoded(cd, blobs, [0, U64, 3, 3, 6], good + good, O.HASH_CRC32C)
    assert want["status"] == [O.ERR_BAD_ARG, O.ERR_BAD_ARG, O.OK, O.OK]
    # an empty buffer with a cut is bad; without one it is the identifier
    e, want = check_encoded(cd, [b"", b"", html[:n]], [0, 0, 1, 4], [1] + good, O.HASH_CRC32C)
    assert want["status"] == [O.OK, O.ERR_BAD_ARG, O.OK] and want["out_len"][0] == 10


def test_out_cap_max_chunks_and_stage_cap_fail_in_the_middle(content):
    html, rnd, _ = content
    cd = cd_of()
    blobs = [html[:2500], html[9:9 + 7001], rnd[:1999] + html[:500], b"", html[:77]]
    first, cuts = F.regular_cuts([len(x) for x in blobs], 1000)
    cuts[1] = 1777                                                      # (no longer the grid)
    full = F.encode_at_cuts(blobs, first, cuts)
    exact = full["out_len"]
    check_encoded(cd, blobs, first, cuts, O.HASH_CRC32C, caps=exact)
    short = list(exact)
    short[1] -= 1
    e, want = check_encoded(cd, blobs, first, cuts, O.HASH_CRC32C, caps=short)
    assert want["status"] == [O.OK, O.ERR_OUTPUT_TOO_SMALL, O.OK, O.OK, O.OK] and want["first"] == [0, 3, 3, 6, 6, 7]
    need = full["result"][0]
    e, want = check_encoded(cd, blobs, first, cuts, O.HASH_CRC32C, max_chunks=need - 2)
    assert want["status"] == [O.OK, O.OK, O.ERR_OUTPUT_TOO_SMALL, O.ERR_OUTPUT_TOO_SMALL, O.ERR_OUTPUT_TOO_SMALL] and want["result"][0] == need
    check_encoded(cd, blobs, first, cuts, O.HASH_CRC32C, max_chunks=need + 9)
    stage = [sum(F.stride(ln) for _, ln in F.list_verdict(len(x), first[b], first[b + 1], cuts)[1]) for b, x in enumerate(blobs)]
    assert sum(stage) <= F.stage_bound(sum(len(x) for x in blobs), need)
    e, want = check_encoded(cd, blobs, first, cuts, O.HASH_CRC32C, stage_cap=stage[0] + stage[1] - 1)
    assert want["status"] == [O.OK] + [O.ERR_OUTPUT_TOO_SMALL] * 4
    e, want = check_encoded(cd, blobs, first, cuts, O.HASH_CRC32C, stage_cap=stage[0] + stage[1])
    assert want["status"] == [O.OK, O.OK] + [O.ERR_OUTPUT_TOO_SMALL] * 3
    check_encoded(cd, blobs, first, cuts, O.HASH_CRC32C, stage_cap=F.stage_bound(sum(len(x) for x in blobs), need))
    # the empty batch
    CL = N.frame_cuts_lib()
    cd._bind()
    for with_index in (False, True):
        result, ix0 = Guarded(4, torch.int64), Guarded(1, torch.int64)
        others = [Guarded(0, torch.int64) for _ in range(3)] + [Guarded(0, torch.int32)]
        ix = [ix0.ptr()] + [g.ptr() for g in others] if with_index else [None] * 5
        assert CL.snp_frame_encode_cuts_batch(cd.ctx.handle, None, None, None, 0, None, None, 0, 0, 0, None, None, None, None, None, *ix, None,
                                              result.ptr()) == O.OK
        torch.cuda.synchronize()
        assert result.read() == [0] * 4 and ix0.read() == ([0] if with_index else [UNTOUCHED])


# ---- 6: end to end ---------------------------------------------------------------------------------------------------------------------------------
def test_content_defined_streams_of_a_buffer_and_its_edited_copy(content):
    html, rnd, _ = content
    cd = cd_of()
    w, mx = 512, 8192
    a = (html + rnd[:60000] + html)[:700000]
    at = len(a) // 3
    ins = rnd[100000:100037]
    a2 = a[:at] + ins + a[at:]
    blobs = [a, a2]
    data, in_off, lens = H.pack(blobs)
    out, out_off, out_len, status, result, index = cd.frame_encode_content_defined(data, H.dev(in_off), H.dev(lens), w, mx)
    torch.cuda.synchronize()
    assert status.tolist() == [O.OK, O.OK]
    f = F.find(blobs, w, mx)
    want = F.encode_at_cuts(blobs, f["cut_first"], f["cuts"])
    h = out.cpu().numpy()
    streams = [h[o:o + n].tobytes() for o, n in zip(out_off.tolist(), out_len.tolist())]
    assert streams == want["streams"] and result.tolist() == want["result"]
    used = want["result"][2]
    assert [getattr(index, k)[:used].tolist() if k in ("start", "pos") else getattr(index, k).tolist() for k in KEYS] == [want[k] for k in KEYS]
    # every framed chunk of A whose piece lies before at - w, or beyond at + w + 32 between content cuts that survive, is among the chunks of A'
    def chunks(b):
        r0, r1 = want["first"][b], want["first"][b + 1]
        pos = want["pos"][r0:r1] + [len(streams[b])]
        return [(s, streams[b][p:q]) for s, p, q in zip(want["start"][r0:r1], pos, pos[1:])]
    cc_a, cc_b = set(F.content_cuts(a, w)) | {0, len(a)}, set(F.content_cuts(a2, w)) | {0, len(a2)}
    theirs = {c for _, c in chunks(1)}
    ends = [s for s, _ in chunks(0)][1:] + [len(a)]
    kept = 0
    for (s, c), e in zip(chunks(0), ends):
        before = e <= at - w
        behind = s >= at + w + 32 and max(x for x in cc_a if x <= s) + 37 in cc_b and min(x for x in cc_a if x >= e) + 37 in cc_b
        if before or behind:
            assert c in theirs, s
            kept += 1
    assert kept > 0.9 * len(ends)
    # the diff of the pair: the true prefix and suffix; the digest: the plain CRC-32C
    sa = (out, out_off[:1].contiguous(), out_len[:1].contiguous(), index_of(index, 0))
    sb = (out, out_off[1:].contiguous(), out_len[1:].contiguous(), index_of(index, 1))
    d = cd.frame_diff_streams(sa, sb)
    torch.cuda.synchronize()
    assert d[4].tolist() == [O.OK] and d[2].tolist() == [len(a)] and d[3].tolist() == [len(a2)]
    true_pre = next(i for i in range(len(a)) if a[i] != a2[i])
    true_suf = next(i for i in range(len(a)) if a[-1 - i] != a2[-1 - i])
    assert (d[0].tolist(), d[1].tolist()) == ([true_pre], [min(true_suf, len(a) - true_pre)])   # (with both flags the two never overlap)
    assert at <= true_pre and true_suf >= len(a) - at - 37
    digest, dig_len, dst = cd.frame_digest_streams(out, out_off, out_len, index)
    torch.cuda.synchronize()
    assert dst.tolist() == [O.OK, O.OK] and dig_len.tolist() == [len(a), len(a2)]
    assert [int(v) & 0xFFFFFFFF for v in digest.tolist()] == [O.crc32c(a), O.crc32c(a2)]


def index_of(index, b):
    """Stream b of a batch index as an index of its own."""
    f0, f1 = int(index.first[b]), int(index.first[b + 1])
    first = torch.tensor([0, f1 - f0], dtype=torch.int64, device="cuda")
    return SB.FrameIndex(first, index.start[f0:f1].contiguous(), index.pos[f0:f1].contiguous(), index.total[b:b + 1].contiguous(),
                         index.tail[b:b + 1].contiguous(), None)


# ---- 7: graph capture ------------------------------------------------------------------------------------------------------------------------------
def test_graph_capture_of_both_calls(content):
    html, rnd, _ = content
    cd = cd_of()
    w, mx = 256, 4096
    lens = [0, 50000, 123457, 9]
    src = [html, rnd + html]
    nb, nbytes = len(lens), sum(lens)
    in_off = np.concatenate([[1], 1 + np.cumsum(lens)[:-1]]).astype(np.int64)
    data = torch.zeros(nbytes + 64, dtype=torch.uint8, device="cuda")
    max_cuts = sum(F.cut_bound(n, w, mx) for n in lens)
    mc = max_cuts + nb
    sc = F.stage_bound(nbytes, mc)
    caps = np.array([10 + 8 * (F.cut_bound(n, w, mx) + 1) + n for n in lens], dtype=np.int64)
    f_off, total = H.out_layout(caps)
    framed = torch.zeros(total, dtype=torch.uint8, device="cuda")
    CL = N.frame_cuts_lib()
    work1 = torch.empty(CL.snp_content_cuts_workspace(nb, nbytes, w), dtype=torch.uint8, device="cuda")
    work2 = torch.empty(CL.snp_frame_encode_cuts_workspace(nb, mc, sc), dtype=torch.uint8, device="cuda")
    d_off, d_len, d_f_off, d_caps = H.dev(in_off), H.dev(lens), H.dev(f_off), H.dev(caps)

    def blobs(k):
        return [src[k][7 * b:7 * b + n] for b, n in enumerate(lens)]

    def fill(k):
        for o, x in zip(in_off.tolist(), blobs(k)):
            if x:
                data[o:o + len(x)].copy_(torch.from_numpy(np.frombuffer(x, dtype=np.uint8).copy()).cuda())

    def call():
        cut_first, cuts, st, res = cd.content_cuts(data, d_off, d_len, w, mx, max_cuts=max_cuts, work=work1, span_bytes=nbytes)
        enc = cd.frame_encode_at_cuts(data, d_off, d_len, cut_first, cuts, True, framed, d_f_off, d_caps, mc, sc, work2)
        return cut_first, cuts, st, res, enc

    fill(0)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        call()
        torch.cuda.synchronize()
        call()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        cut_first, cuts, st, res, enc = call()
    fill(1)
    framed.zero_()
    g.replay()
    torch.cuda.synchronize()
    f = F.find(blobs(1), w, mx)
    assert cut_first.tolist() == f["cut_first"] and cuts[:f["result"][1]].tolist() == f["cuts"] and st.tolist() == f["status"]
    assert res.tolist() == f["result"]
    want = F.encode_at_cuts(blobs(1), f["cut_first"], f["cuts"])
    _, _, out_len, est, eres, index = enc
    h, fl = framed.cpu().numpy(), out_len.tolist()
    assert est.tolist() == want["status"] and fl == want["out_len"] and eres.tolist() == want["result"]
    for b, x in enumerate(want["streams"]):
        assert h[f_off[b]:f_off[b] + fl[b]].tobytes() == x, b
    direct = call()                                                     # the direct call gives what the replay gave
    torch.cuda.synchronize()
    assert torch.equal(direct[0], cut_first) and np.array_equal(framed.cpu().numpy(), h)

"""The five seekable-stream calls (snp_frame_encode_chunked_batch, snp_frame_index_batch, snp_frame_read_indexed_batch,
snp_frame_decode_range_batch, snp_frame_write_indexed_batch) at every launch tier and layout of the two routines they share
(snp_ctx::launch_compress, snp_ctx::decode_chunks): the tier picked by the caller's row bound (a), by the real row count (b), by the context's
options (c) and by what the previous batch on the context looked like (d), and the three calls in one captured graph (e).  Every comparison
is byte-exact against the Python models (frame_*_model.py) and the C oracle; where frame_update_model.write_plan is too slow (from ten thousand
slots on) the indexed write is checked by its consequence: the chunked encode of the patched buffers, the walk's index of the new streams,
and d_result by arithmetic.  In every case each output array and workspace lies between guard elements and every arena is canary-filled:
(a)-(c) through seekable_harness.py, whose calls synchronise; (d) and (e) need calls that only enqueue, so they make the same direct calls
on guarded arrays of their own and read them afterwards.  The LDS throttle values: the 256 and 65536 of test_decode_under_the_lds_throttle
and the 32768 that test_decode_lds_throttle_changes_nothing adds.  Bytes cannot
show which kernel ran, and no snp_ctx_counter reports these paths (0, 1 and 6 count the host calls' large blocks, 2-5 the table workspace
search): profiles/r14a_seekable_tier_kernels.csv is the kernel trace of this file.  The batches: seekable_cases.py.  Needs an MI355X."""
import functools

import numpy as np
import pytest
import torch

import frame_buffers_helpers as H
import frame_chunked_model as K
import frame_index_model as X
import frame_range_model as R
import frame_update_model as U
import layouts
import oracle as O
import seekable_cases as SC
from seekable_harness import (CANARY, KEYS, UNTOUCHED, Encoded, Guarded, Updated, _p, dev_i32, dev_u64, index_call, index_tensors, range_call,
                              read_call)

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from snappier_amd import batch as SB, _native as N

CRC = O.HASH_CRC32C
VARIANTS = [O.HASH_CRC32C, O.HASH_MUL]
BIG = 1 << 62


def codec(variant=CRC, compress=None, decode=None, fenced=None, **options):
    cd = SB.BlockCodec(0, variant)
    if compress is not None:
        layouts.set_compress_layout(cd.ctx, compress)
    if decode is not None:
        layouts.set_decode_layout(cd.ctx, decode, fenced)
    for name, value in options.items():
        cd.ctx.set_option(getattr(N, name), value)
    return cd


# ---- the models, computed once per batch ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def enc_model(batch, variant):
    return K.encode(batch.blobs, batch.cb, variant)


@functools.lru_cache(maxsize=None)
def dec_case(batch, variant=CRC):
    """(streams, their index): the batch's streams and the corrupt copy of the last one."""
    streams = SC.decode_streams(batch, variant)
    return streams, X.build_index(streams)


def exact_caps(lens, reqs):
    return [R.clip(lens[b], ro, rl)[1] - R.clip(lens[b], ro, rl)[0] for b, ro, rl in reqs]


@functools.lru_cache(maxsize=None)
def read_model(batch, variant=CRC):
    streams, ix = dec_case(batch, variant)
    caps = exact_caps(ix["total"], batch.reads)
    return caps, X.read_plan(streams, ix, batch.reads, caps, BIG, BIG)


@functools.lru_cache(maxsize=None)
def range_model(batch, variant=CRC):
    streams, ix = dec_case(batch, variant)
    caps = [R.clip(n, *w)[1] - R.clip(n, *w)[0] for n, w in zip(ix["total"], batch.ranges)]
    need = R.needs(streams, batch.ranges, caps)
    return caps, need, R.range_plan(streams, batch.ranges, caps, *need)


@functools.lru_cache(maxsize=None)
def write_model(batch, variant, kind):
    """kind "own": the batch's request list; "edges": a 3-byte request across every second chunk boundary, and one in the corrupt chunk."""
    streams, ix = dec_case(batch, variant)
    reqs = batch.writes if kind == "own" else SC.boundary_writes(batch, corrupt=True)
    rng = np.random.default_rng(len(reqs))
    srcs = [U.fresh(rng, ln) for _, _, ln in reqs]
    free = U.write_plan(streams, ix, reqs, srcs, variant=variant)
    caps = [bd or len(s) for bd, s in zip(free["out_bound"], streams)]
    return reqs, srcs, caps, U.write_plan(streams, ix, reqs, srcs, caps, free["result"][0], free["result"][2], variant)


# ---- one guarded call against its model; a looser bound changes no field of any model -------------------------------------------------------------
def run_encode(cd, batch, variant, bound=None):
    e = Encoded(cd, batch.blobs, batch.cb, max_chunks=bound)
    want = enc_model(batch, variant)
    for key in want:
        assert e.got[key] == want[key], (batch.cb, key)
    return e


def run_index(cd, batch, variant, bound=None):
    streams, want = dec_case(batch)
    got = index_call(cd, streams, want["result"][2] if bound is None else bound, want["result"][0] if bound is None else bound)
    assert got == want
    return got


def same_tuple(got, want, what):
    assert got[0] == want[0], [(r, g, w) for r, (g, w) in enumerate(zip(got[0], want[0])) if g != w][:10]
    assert got[1] == want[1] and got[3] == want[3], (what, got[3], want[3])
    for r, (g, w) in enumerate(zip(got[2], want[2])):
        assert g == w, (what, r)
    return got


def run_read(cd, batch, variant=CRC, bound=None):
    streams, ix = dec_case(batch, variant)
    caps, want = read_model(batch, variant)
    return same_tuple(read_call(cd, streams, ix, batch.reads, caps, want[3][0] if bound is None else bound, want[3][2]), want, "read")


def run_range(cd, batch, variant=CRC, bound=None):
    streams, _ = dec_case(batch, variant)
    caps, need, want = range_model(batch, variant)
    return same_tuple(range_call(cd, streams, batch.ranges, caps, need[0] if bound is None else bound, need[1], need[2]), want, "range")


def run_write(cd, batch, variant, bound=None, kind="own"):
    streams, ix = dec_case(batch, variant)
    reqs, srcs, caps, want = write_model(batch, variant, kind)
    u = Updated(cd, streams, ix, reqs, srcs, caps=caps, max_slots=want["result"][0] if bound is None else bound, stage_cap=want["result"][2],
                variant=variant, model=False)
    u.want = want
    return u.check()


def same(a, b):
    """Two runs of one call: every array and (encode, write) the whole arena, canaries included."""
    return (np.array_equal(a.h, b.h) and a.got == b.got) if hasattr(a, "h") else a == b


CALLS = {"encode": (run_encode, True), "index": (run_index, False), "read": (run_read, False), "range": (run_range, False),
         "write": (run_write, True)}                                    # (the call, whether a compressor runs in it)


# ---- a. the bound picks the tier -----------------------------------------------------------------------------------------------------------------
TIER_OPTIONS = {"dual": "OPT_COMPRESS_WINDOW_DUAL_MIN_BATCH", "global": "OPT_COMPRESS_WINDOW_GLOBAL_MIN_BATCH", "max": "OPT_COMPRESS_WINDOW_MAX_BATCH",
                "small": "OPT_SMALL_BLOCK_MIN_BATCH", "slice": "OPT_COMPRESS_SLICE"}
# t - 1 and t for each threshold t: the five a context states as options, and the fragment counts at which the lane compressor's launch shape
# changes (seekable_cases.LANE_TIERS: no option states them; its middle one is the default of "max").  The bounds from 131 072 on at 64-byte
# chunks only: their staging is max_chunks strides of the chunk size.
SMALL_BOUNDS = ["exact"] + [t + d for t in ("dual", "global", "small", "lane8192", "max") for d in ("-1", "")] + ["40000"]
LARGE_BOUNDS = [t + d for t in ("lane131072", "slice") for d in ("-1", "")]
SWEEP = [(cb, b) for cb in (1000, 64) for b in SMALL_BOUNDS] + [(64, b) for b in LARGE_BOUNDS]


def bound_of(cd, name):
    if name == "exact":
        return None
    if name.isdigit():
        return int(name)
    t, below = (name[:-2], 1) if name.endswith("-1") else (name, 0)
    return (int(t[4:]) if t.startswith("lane") else cd.ctx.get_option(getattr(N, TIER_OPTIONS[t]))) - below


def test_the_thresholds_are_the_defaults_the_batches_were_built_for():
    cd = codec()
    got = [cd.ctx.get_option(getattr(N, TIER_OPTIONS[t])) for t in ("dual", "global", "max", "small", "slice")]
    assert got == [SC.WIN_DUAL_MIN, SC.WIN_GLOBAL_MIN, SC.WIN_MAX, SC.SMALL_MIN_BATCH, SC.SLICE]
    assert SC.LANE_TIERS[1] == SC.WIN_MAX and [bound_of(cd, "lane8192-1"), bound_of(cd, "slice")] == [8191, SC.SLICE]


_exact = {}


def exact_run(call, cb, variant):
    if (call, cb, variant) not in _exact:
        _exact[call, cb, variant] = CALLS[call][0](codec(variant), SC.small_batch(cb), variant)
    return _exact[call, cb, variant]


@pytest.mark.parametrize("cb,bound", SWEEP)
@pytest.mark.parametrize("call", list(CALLS))
def test_the_bound_picks_the_tier(call, cb, bound):
    run, compresses = CALLS[call]
    for variant in VARIANTS if compresses else [CRC]:
        cd = codec(variant)
        got = run(cd, SC.small_batch(cb), variant, bound_of(cd, bound))   # (against the model)
        assert same(got, exact_run(call, cb, variant)), (call, cb, bound, variant)


@pytest.mark.parametrize("cb", [1000, 64])
def test_a_sliced_launch_whose_later_slices_hold_only_empty_slots(cb):
    """4 096 fragments per lane-compressor launch and a bound of 9 000: three launches, the real slots all in the first."""
    for variant in VARIANTS:
        cd = codec(variant, compress="lanes", OPT_COMPRESS_SLICE=4096)
        for call in ("encode", "write"):
            assert same(CALLS[call][0](cd, SC.small_batch(cb), variant, 9000), exact_run(call, cb, variant)), (call, variant)


# ---- b. the real count picks the tier ------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def sound_index(batch, variant):
    return X.build_index(batch.streams(variant))


def where_streams_differ(got, want, cb):
    """For the message of a failed comparison: the first chunk in which two streams differ -- its number, both headers, whether both chunks
    decode to the same bytes (a different compression of the right bytes) or not (wrong bytes) -- and how many chunks differ in all."""
    if got is None or want is None:
        return "one stream is missing"
    g, w = R.walk(got)[0], R.walk(want)[0]
    if len(g) != len(w):
        return f"{len(g)} chunks against {len(w)}"
    diff = [k for k, (a, b) in enumerate(zip(g, w)) if got[a[1] - 8:a[1] + a[2]] != want[b[1] - 8:b[1] + b[2]]]
    if not diff:
        return "no data chunk differs"
    k = diff[0]
    a, b = R.chunk_result(got, g[k]), R.chunk_result(want, w[k])
    return dict(chunk=k, differing=len(diff), got_row=g[k][:3] + g[k][4:], want_row=w[k][:3] + w[k][4:], got_status=a[0], same_bytes=a[1] == b[1],
                first_byte=next((i for i, (x, y) in enumerate(zip(a[1] or b"", b[1] or b"")) if x != y), None))


def consequence_write(cd, batch, variant, reqs, seed=1):
    """An indexed write too large for write_plan: every new stream is the chunked encode of the patched buffer, new_pos the walk's index of the
    new streams, d_result by arithmetic; then the written windows read back through the new index."""
    cb, blobs, streams, ix = batch.cb, batch.blobs, batch.streams(variant), sound_index(batch, variant)
    rng = np.random.default_rng(seed)
    srcs = [U.fresh(rng, ln) for _, _, ln in reqs]
    named = {b for b, _, _ in reqs}
    caps = [K.frame_cap(len(x), cb) if b in named else len(s) for b, (x, s) in enumerate(zip(blobs, streams))]
    slots, stage = SC.write_needs([len(x) for x in blobs], cb, reqs)
    u = Updated(cd, streams, ix, reqs, srcs, caps=caps, max_slots=slots, stage_cap=stage, variant=variant, model=False)
    new = [K.stream_of(U.patched(x, reqs, srcs, b), cb, variant) if b in named else None for b, x in enumerate(blobs)]
    assert u.got["status"] == [O.OK] * len(blobs) and u.got["req_status"] == [O.OK] * len(reqs)
    for b, (g, w) in enumerate(zip(u.got["streams"], new)):
        assert g == w, (b, where_streams_differ(g, w, cb))
    assert u.got["out_len"] == [len(x) if x else 0 for x in new]
    assert u.got["new_pos"] == X.build_index([x or s for x, s in zip(new, streams)])["pos"]
    assert u.got["result"] == [slots, sum(u.got["out_len"]), stage, len(named)]
    assert all((bd >= n > 0) if b in named else bd == 0 for b, (bd, n) in enumerate(zip(u.got["out_bound"], u.got["out_len"])))
    live = [(q, s) for q, s in zip(reqs, srcs) if q[2]]
    lens = np.array([q[2] for q, _ in live], dtype=np.int64)
    r_off, total = H.out_layout(lens)
    back = torch.full((total,), CANARY, dtype=torch.uint8, device="cuda")
    ol, st, _ = cd.frame_read_indexed(u.out, H.dev(u.out_off), u.out_len.mid, u.frame_index(), dev_i32([q[0] for q, _ in live]),
                                      H.dev([q[1] for q, _ in live]), H.dev(lens), back, H.dev(r_off), H.dev(lens))
    torch.cuda.synchronize()
    assert st.tolist() == [O.OK] * len(live) and ol.tolist() == lens.tolist()
    h = back.cpu().numpy()
    assert (H.outside_ranges(h, r_off, lens) == CANARY).all()
    for (q, s), o in zip(live, r_off.tolist()):
        assert h[o:o + q[2]].tobytes() == s, q
    return u


@functools.lru_cache(maxsize=None)
def tail_model(batch, variant):
    """The ragged tail 234 times over: 2 106 streams, so that the edge table (two rows per stream) reaches the small-block pre-pass."""
    copies = 234
    streams, ranges = batch.streams(variant)[1:] * copies, batch.ranges[1:len(batch.blobs)] * copies
    lens = [len(x) for x in batch.blobs[1:]] * copies
    caps = [R.clip(n, *w)[1] - R.clip(n, *w)[0] for n, w in zip(lens, ranges)]
    need = R.needs(streams, ranges, caps)
    return streams, ranges, caps, need, R.range_plan(streams, ranges, caps, *need)


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("cb,slots", SC.COUNT_PAIRS)
def test_the_real_count_picks_the_tier(cb, slots, variant):
    batch = SC.count_batch(cb, slots)
    cd = codec(variant)
    e = run_encode(cd, batch, variant)                                  # 1: against K.encode
    want = enc_model(batch, variant)
    walked = cd.frame_index_buffers(e.out, H.dev(e.out_off), e.out_len.mid)            # 2: the walk's index is the encoder's
    for key, g in zip(KEYS, e.ix):
        used = want["result"][2] if key in ("start", "pos") else g.n
        assert torch.equal(getattr(walked, key)[:used], g.mid[:used]), key
    if variant == CRC:                                                  # (the decoders do not know the variant)
        got = run_read(cd, batch)                                       # 3: a window across every chunk boundary, and every chunk whole
        assert got[3][0] >= slots and 2 * len(batch.reads) >= 2 * slots
        streams, ranges, caps, need, plan = tail_model(batch, variant)  # 4: the ragged tail, 2 106 streams
        assert 2 * len(streams) >= cd.ctx.get_option(N.OPT_SMALL_BLOCK_MIN_BATCH)
        same_tuple(range_call(cd, streams, ranges, caps, *need), plan, "tail")
        run_range(cd, batch)
    consequence_write(cd, batch, variant, batch.writes)                 # 5: every slot dirty; then every live row an edge among empty rows
    consequence_write(cd, batch, variant, SC.boundary_writes(batch), seed=2)


# ---- c. every layout -----------------------------------------------------------------------------------------------------------------------------
def layout_batches():
    return SC.count_batch(1000, 3000), SC.small_batch(64)


@functools.lru_cache(maxsize=None)
def default_run(call, batch, variant):
    return CALLS[call][0](codec(variant), batch, variant)


@pytest.mark.parametrize("crc", [0, 1, 2])
@pytest.mark.parametrize("layout", layouts.COMPRESS_LAYOUTS)
def test_every_compress_layout_and_crc_kernel(layout, crc):
    for batch in layout_batches():
        for variant in VARIANTS:
            cd = codec(variant, compress=layout, OPT_CRC_KERNEL=crc)
            for call in ("encode", "write"):                            # (the write: the batch's own list -- the whole long stream)
                assert same(CALLS[call][0](cd, batch, variant), default_run(call, batch, variant)), (call, batch.cb, variant)


DECODE_CASES = [(d, f, 0) for d in layouts.DECODE_LAYOUTS for f in (0, 1)] + [("chains", None, t) for t in (256, 32768, 65536)]


@pytest.mark.parametrize("decode,fenced,throttle", DECODE_CASES)
def test_every_decode_layout_fence_and_lds_throttle(decode, fenced, throttle):
    """A corrupt chunk lies inside a window of every call (the last stream of decode_streams), so the status path runs under each layout."""
    for batch in layout_batches():
        cd = codec(decode=decode, fenced=fenced, OPT_DECODE_LDS_THROTTLE=throttle)
        got = run_read(cd, batch), run_range(cd, batch), run_write(cd, batch, CRC, kind="edges")
        bad = [max(got[0][0]), got[1][0][-1], got[2].got["status"][-1]]  # (the statuses themselves: the models')
        assert O.OK not in bad and got[2].got["result"][3] == 1 and got[0][0].count(O.OK) >= len(batch.reads) - 4


# ---- d. the previous batch picks the form --------------------------------------------------------------------------------------------------------
class EncodeJob:
    """snp_frame_encode_chunked_batch called directly with every array guarded, as seekable_harness.Encoded calls it -- but launch() only
    enqueues, and verify() reads everything afterwards."""

    def __init__(self, cd, batch, variant):
        self.cd, self.batch, self.want = cd, batch, enc_model(batch, variant)
        self.nb = nb = len(batch.blobs)
        self.data, in_off, lens = H.pack(batch.blobs)
        caps = np.array([K.frame_cap(len(x), batch.cb) for x in batch.blobs], dtype=np.int64)
        self.out_off, total = H.out_layout(caps)
        self.out = torch.full((total,), CANARY, dtype=torch.uint8, device="cuda")
        self.mc = mc = batch.slots()
        self.out_len, self.status, self.result = Guarded(nb, torch.int64), Guarded(nb, torch.int32), Guarded(4, torch.int64)
        self.ix = [Guarded(nb + 1, torch.int64), Guarded(mc, torch.int64), Guarded(mc, torch.int64), Guarded(nb, torch.int64), Guarded(nb, torch.int32)]
        self.work = Guarded(N.frame_chunked_lib().snp_frame_encode_chunked_workspace(nb, mc, batch.cb), torch.uint8)
        self.tabs = [H.dev(in_off), H.dev(lens), H.dev(self.out_off), H.dev(caps)]

    def launch(self):
        self.cd._bind()
        st = N.frame_chunked_lib().snp_frame_encode_chunked_batch(
            self.cd.ctx.handle, _p(self.data), _p(self.tabs[0]), _p(self.tabs[1]), self.nb, self.batch.cb, self.mc, _p(self.out), _p(self.tabs[2]),
            _p(self.tabs[3]), self.out_len.ptr(), self.status.ptr(), *[g.ptr() for g in self.ix], self.work.ptr(), self.result.ptr())
        assert st == O.OK

    def verify(self):
        want, cb = self.want, self.batch.cb
        self.work.read()
        status, ol, index = self.status.read(), self.out_len.read(), [g.read() for g in self.ix]
        assert status == want["status"] and ol == want["out_len"] and self.result.read() == want["result"], cb
        used = index[0][self.nb]
        assert 0 <= used <= self.mc and all(v == UNTOUCHED for v in index[1][used:] + index[2][used:]), "a row beyond the index"
        index[1], index[2] = index[1][:used], index[2][:used]
        for key, got in zip(KEYS, index):
            assert got == want[key], (cb, key)
        h = self.out.cpu().numpy()
        assert (H.outside_ranges(h, self.out_off, ol) == CANARY).all(), "a write outside the output ranges"
        for b, (o, x) in enumerate(zip(self.out_off.tolist(), want["streams"])):
            assert h[o:o + ol[b]].tobytes() == x, (cb, b)


@functools.lru_cache(maxsize=None)
def sequence_reads(cb, rows):
    """At least `rows` interior rows: a window across every boundary and every chunk whole; at 65 536-byte chunks, 64 chunks read whole `rows`
    times over.  -> (batch, reads, caps, the model's plan)."""
    batch = SC.count_batch(cb, 64 if cb == 65536 else rows)
    reads = [(0, (k % 64) * cb, cb) for k in range(rows)] if cb == 65536 else batch.reads[:-4]
    streams, ix = batch.streams(CRC), sound_index(batch, CRC)
    caps = exact_caps(ix["total"], reads)
    return batch, reads, caps, X.read_plan(streams, ix, reads, caps, BIG, BIG)


class ReadJob:
    """snp_frame_read_indexed_batch called directly with every output guarded, as seekable_harness.read_call calls it -- but launch() only
    enqueues, and verify() reads everything afterwards."""

    def __init__(self, cd, cb):
        self.cd, self.cb = cd, cb
        small_min = cd.ctx.get_option(N.OPT_SMALL_BLOCK_MIN_BATCH)
        batch, reads, self.caps, self.want = sequence_reads(cb, SC.hint_rows(small_min))
        streams = batch.streams(CRC)
        self.ns, self.nreq = len(streams), len(reads)
        self.framed, in_off, in_len = H.pack(streams)
        self.index, self.ne = index_tensors(sound_index(batch, CRC), self.ns)
        self.out_off, total = H.out_layout(self.caps)
        self.out = torch.full((total,), CANARY, dtype=torch.uint8, device="cuda")
        self.mc, self.ec = self.want[3][0], self.want[3][2]
        assert self.mc >= small_min                                     # the interior table reaches the pre-pass
        self.out_len, self.status, self.result = Guarded(self.nreq, torch.int64), Guarded(self.nreq, torch.int32), Guarded(4, torch.int64)
        self.work = Guarded(N.frame_index_lib().snp_frame_read_indexed_workspace(self.nreq, self.mc, self.ec), torch.uint8)
        self.tabs = [H.dev(in_off), H.dev(in_len), dev_i32([q[0] for q in reads]), dev_u64([q[1] for q in reads]), dev_u64([q[2] for q in reads]),
                     H.dev(self.out_off), H.dev(self.caps)]

    def launch(self):
        self.cd._bind()
        st = N.frame_index_lib().snp_frame_read_indexed_batch(
            self.cd.ctx.handle, _p(self.framed), _p(self.tabs[0]), _p(self.tabs[1]), self.ns, *[_p(t) for t in self.index], self.ne, _p(self.tabs[2]),
            _p(self.tabs[3]), _p(self.tabs[4]), self.nreq, self.mc, self.ec, _p(self.out), _p(self.tabs[5]), _p(self.tabs[6]), self.out_len.ptr(),
            self.status.ptr(), self.work.ptr(), self.result.ptr())
        assert st == O.OK

    def verify(self):
        st, ol, data, res = self.want
        self.work.read()
        assert self.status.read() == st == [O.OK] * len(st) and self.out_len.read() == ol and self.result.read() == res, self.cb
        h = self.out.cpu().numpy()
        assert (H.outside_ranges(h, self.out_off, ol) == CANARY).all(), "a write outside the output ranges"
        for r, (o, x) in enumerate(zip(self.out_off.tolist(), data)):
            assert h[o:o + len(x)].tobytes() == x, (self.cb, r)


def run_sequence(jobs, sync):
    torch.cuda.synchronize()
    for j in jobs:
        j.launch()
        if sync:
            torch.cuda.synchronize()                                    # the hint this call left has landed when the next one looks
    torch.cuda.synchronize()
    for j in jobs:
        j.verify()


COMPRESS_SEQUENCE = [64, 64, 300, 300, 700, 4096, 96, 65536, 256]      # longest fragments: tiny, small, mid, large -- and back
DECODE_SEQUENCE = [32, 100, 400, 65536, 32, 400]


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("sync", [True, False])
def test_the_lane_compressor_after_every_kind_of_previous_batch(sync, variant):
    """The lane compressor picks its launch form (input in LDS first, fragments per wavefront, probes) by the longest fragment of the previous
    batch on the context, once that has come back; without a synchronisation between the calls the older hint applies."""
    cd = codec(variant, compress="lanes")
    slots = dict(SC.COMPRESS_SEQUENCE)                                  # (the batches test_seekable_cases.py checks)
    run_sequence([EncodeJob(cd, SC.count_batch(cb, slots[cb]), variant) for cb in COMPRESS_SEQUENCE], sync)
    consequence_write(cd, SC.count_batch(1000, 3000), variant, SC.count_batch(1000, 3000).writes)


@pytest.mark.parametrize("sync", [True, False])
def test_the_decoder_after_every_kind_of_previous_batch(sync):
    """The decoder picks the pre-pass (a lane, 4 or 8 lanes per block, its LDS budget) or one block per wavefront by the previous batch, in
    batches of at least OPT_SMALL_BLOCK_MIN_BATCH rows only.  With the hints landed: the pre-pass by lane (first batch), by lane (mean 32),
    by 4 lanes (100), by 8 lanes with a budget (400; its leftovers, every 65 536-byte row, say "mostly large"), one block per wavefront and a
    sample of the capacities (the second 32), and -- the sample having said "small" again -- the pre-pass by lane once more: the last batch is
    the launch after the flip back."""
    cd = codec()
    assert set(DECODE_SEQUENCE) == set(SC.DECODE_SEQUENCE)
    run_sequence([ReadJob(cd, cb) for cb in DECODE_SEQUENCE], sync)
    batch = SC.count_batch(1000, 3000)
    run_range(cd, batch)
    run_write(cd, batch, CRC, kind="edges")


# ---- e. the three calls in one captured graph ----------------------------------------------------------------------------------------------------
def test_encode_write_and_read_in_one_captured_graph():
    """Chunked encode -> indexed write of its output through its index -> indexed read through the new index, 4 096 rows of bound each, on one
    context in one capture, each call made directly with guarded arrays and a canary-filled arena; replayed on new buffer contents and new
    request bytes, the guards and canaries restored before each replay."""
    cb, rows = 1000, 4096
    cd = codec()
    shape = SC.small_batch(cb)
    lens = [len(x) for x in shape.blobs]
    ns = len(lens)
    writes = [q for q in shape.writes if q[0] < ns]
    reads = [q for q in shape.reads if q[0] < ns]
    nw, nr = len(writes), len(reads)
    in_off = np.concatenate([[1], 1 + np.cumsum(np.array(lens) + 3)[:-1]]).astype(np.int64)
    src = torch.zeros(int(in_off[-1]) + lens[-1] + 8, dtype=torch.uint8, device="cuda")
    caps = np.array([K.frame_cap(n, cb) for n in lens], dtype=np.int64)
    f_off, f_total = H.out_layout(caps)
    wlen = [q[2] for q in writes]
    w_off = np.concatenate([[0], np.cumsum(wlen)[:-1]]).astype(np.int64)
    wdata = torch.zeros(sum(wlen) + 8, dtype=torch.uint8, device="cuda")
    rcaps = exact_caps(lens, reads)
    r_off, r_total = H.out_layout(rcaps)
    framed, updated, back = (torch.full((n,), CANARY, dtype=torch.uint8, device="cuda") for n in (f_total, f_total, r_total))
    stage, edge = rows * cb, 2 * nr * cb
    CL, UL, IL = N.frame_chunked_lib(), N.frame_update_lib(), N.frame_index_lib()
    i64, i32 = torch.int64, torch.int32
    # encode: out_len, status, d_result and the index; write: out_len, status, req_status, new_pos, out_bound, d_result; read: out_len, status, d_result
    e_len, e_st, e_res = Guarded(ns, i64), Guarded(ns, i32), Guarded(4, i64)
    e_ix = [Guarded(ns + 1, i64), Guarded(rows, i64), Guarded(rows, i64), Guarded(ns, i64), Guarded(ns, i32)]
    u_len, u_st, q_st, u_pos, u_bound, u_res = Guarded(ns, i64), Guarded(ns, i32), Guarded(nw, i32), Guarded(rows, i64), Guarded(ns, i64), Guarded(4, i64)
    r_len, r_st, r_res = Guarded(nr, i64), Guarded(nr, i32), Guarded(4, i64)
    works = [Guarded(n, torch.uint8) for n in (CL.snp_frame_encode_chunked_workspace(ns, rows, cb),
                                               UL.snp_frame_write_indexed_workspace(ns, nw, rows, stage),
                                               IL.snp_frame_read_indexed_workspace(nr, rows, edge))]
    guarded = [e_len, e_st, e_res, *e_ix, u_len, u_st, q_st, u_pos, u_bound, u_res, r_len, r_st, r_res, *works]
    tabs = dict(in_off=H.dev(in_off), lens=H.dev(lens), f_off=H.dev(f_off), caps=H.dev(caps), ws=dev_i32([q[0] for q in writes]),
                wo=H.dev([q[1] for q in writes]), wl=H.dev(wlen), w_off=H.dev(w_off), rs=dev_i32([q[0] for q in reads]),
                ro=dev_u64([q[1] for q in reads]), rl=dev_u64([q[2] for q in reads]), r_off=H.dev(r_off), rcaps=H.dev(rcaps))

    def fill(seed):
        blobs = [SC.content(n, cb, seed + b) for b, n in enumerate(lens)]
        h = np.zeros(src.numel(), dtype=np.uint8)
        for o, x in zip(in_off, blobs):
            h[o:o + len(x)] = np.frombuffer(x, dtype=np.uint8)
        src.copy_(torch.from_numpy(h).cuda())
        rng = np.random.default_rng(seed)
        srcs = [U.fresh(rng, n) for n in wlen]
        wdata[:sum(wlen)].copy_(torch.from_numpy(np.frombuffer(b"".join(srcs), dtype=np.uint8).copy()).cuda())
        for t in (framed, updated, back):
            t.fill_(CANARY)
        for g in guarded:
            g.t.view(torch.uint8).fill_(CANARY)
        return blobs, srcs

    def call():
        cd._bind()
        h = cd.ctx.handle
        assert CL.snp_frame_encode_chunked_batch(h, _p(src), _p(tabs["in_off"]), _p(tabs["lens"]), ns, cb, rows, _p(framed), _p(tabs["f_off"]),
                                                 _p(tabs["caps"]), e_len.ptr(), e_st.ptr(), *[g.ptr() for g in e_ix], works[0].ptr(),
                                                 e_res.ptr()) == O.OK
        u_pos.mid.copy_(e_ix[2].mid)                                    # (as the wrapper does: new_pos starts as the old positions)
        assert UL.snp_frame_write_indexed_batch(h, _p(framed), _p(tabs["f_off"]), e_len.ptr(), ns, *[g.ptr() for g in e_ix], rows, _p(wdata),
                                                _p(tabs["ws"]), _p(tabs["wo"]), _p(tabs["wl"]), _p(tabs["w_off"]), nw, rows, stage, _p(updated),
                                                _p(tabs["f_off"]), _p(tabs["caps"]), u_len.ptr(), u_st.ptr(), q_st.ptr(), u_pos.ptr(),
                                                u_bound.ptr(), works[1].ptr(), u_res.ptr()) == O.OK
        assert IL.snp_frame_read_indexed_batch(h, _p(updated), _p(tabs["f_off"]), u_len.ptr(), ns, e_ix[0].ptr(), e_ix[1].ptr(), u_pos.ptr(),
                                               e_ix[3].ptr(), e_ix[4].ptr(), rows, _p(tabs["rs"]), _p(tabs["ro"]), _p(tabs["rl"]), nr, rows, edge,
                                               _p(back), _p(tabs["r_off"]), _p(tabs["rcaps"]), r_len.ptr(), r_st.ptr(), works[2].ptr(),
                                               r_res.ptr()) == O.OK

    def verify(blobs, srcs):
        torch.cuda.synchronize()
        for w in works:
            w.read()
        # the encode
        want = K.encode(blobs, cb, CRC, rows)
        fl = e_len.read()
        assert e_st.read() == want["status"] and fl == want["out_len"] and e_res.read() == want["result"]
        index = [g.read() for g in e_ix]
        used = index[0][ns]
        assert used == want["result"][2] and all(v == UNTOUCHED for v in index[1][used:] + index[2][used:]), "a row beyond the index"
        assert [index[0], index[1][:used], index[2][:used], index[3], index[4]] == [want[k] for k in KEYS]
        h = framed.cpu().numpy()
        assert (H.outside_ranges(h, f_off, fl) == CANARY).all(), "a write outside the encoder's output ranges"
        for o, x in zip(f_off.tolist(), want["streams"]):
            assert h[o:o + len(x)].tobytes() == x
        # the write
        ix = {k: want[k] for k in KEYS}
        plan = U.write_plan(want["streams"], ix, writes, srcs, caps.tolist(), rows, stage)
        ul, pos = u_len.read(), u_pos.read()
        assert u_st.read() == plan["status"] and ul == plan["out_len"] and q_st.read() == plan["req_status"] and u_res.read() == plan["result"]
        assert pos[:used] == plan["new_pos"] and all(v == UNTOUCHED for v in pos[used:]) and u_bound.read() == plan["out_bound"]
        h = updated.cpu().numpy()
        assert (H.outside_ranges(h, f_off, ul) == CANARY).all(), "a write outside the update's output ranges"
        new = [x if x is not None else b"" for x in plan["streams"]]
        for b, (o, x) in enumerate(zip(f_off.tolist(), new)):
            assert h[o:o + len(x)].tobytes() == x, b
            assert plan["streams"][b] is None or x == K.stream_of(U.patched(blobs[b], writes, srcs, b), cb)
        # the read goes through the new index over what the write left: a stream no request named has out_len 0 there, and its requests say so
        st, ol, data, res = X.read_plan(new, {**ix, "pos": plan["new_pos"]}, reads, rcaps, rows, edge)
        got_st, got_ol = r_st.read(), r_len.read()
        assert got_st == st and got_ol == ol and r_res.read() == res
        h = back.cpu().numpy()
        assert (H.outside_ranges(h, r_off, [n if s == O.OK else c for s, n, c in zip(got_st, got_ol, rcaps)]) == CANARY).all(), \
            "a write outside the read's output ranges"
        for r, (o, x) in enumerate(zip(r_off.tolist(), data)):
            assert x is None or h[o:o + len(x)].tobytes() == x, r
        assert st.count(O.OK) > nr // 2

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        fill(50)
        call()
        torch.cuda.synchronize()
        first = fill(100)
        call()
        verify(*first)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        call()
    for seed in (200, 300):
        new = fill(seed)
        torch.cuda.synchronize()
        g.replay()
        verify(*new)

"""Every block decoder on the foreign dialect of tests/stream_grammar.py: streams built from the whole tag grammar (copy-4, offsets of 65536 and
more, literals under longer length fields than they need, 65..128-byte literals in all four long encodings) and grammar-aware near-misses of them,
through (a) every batch decode layout, (b) every input / output alignment, (c) the small-block layouts on blocks of 1..512 bytes, (d) large
single blocks through the host API, (e) snp_decompress_buffers_batch and (f) the framed calls.  Every comparison is exact -- status, length and
bytes against the oracle, with the generator's own output as a cross-check -- and every output buffer is canary-filled: nothing may be written
outside [out_off, out_off + out_len) of an OK block, nor outside [out_off, out_off + cap) of any other.  Needs an MI355X."""
import json
from functools import lru_cache

import numpy as np
import pytest
import torch

import frame_buffers_helpers as H
import frame_index_model as X
import frame_range_model as R
import layouts
import oracle as O
import stream_grammar as G
import test_gpu_decompress_buffers as DB
import test_gpu_frame_index as FI
import test_gpu_frame_range as FR

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    import snappier_amd as S
    from snappier_amd import batch as SB, _native as N
    from snappier_amd.errors import InvalidDataException

CANARY = 0xA5
THREADS = 16


def log(**kw):
    """One JSON line per test on standard output: what was compared (pytest -s, or the captured output of a failing test, shows it)."""
    print(json.dumps(kw))


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def declared_of(stream: bytes) -> int:
    return DB.declared_of(stream)


def capacities(cases):
    """Mostly the declared length; some 1..40 bytes more (the slack must stay canary); some one byte less (OUTPUT_TOO_SMALL, nothing written).
    (A capacity of zero is an argument error at the boundary: an empty block gets one byte.)"""
    caps = []
    for i, c in enumerate(cases):
        d = declared_of(c.stream)
        caps.append(d + 1 + i % 40 if i % 10 == 7 else d - 1 if i % 10 == 3 and d >= 2 else max(d, 1))
    return np.array(caps, dtype=np.int64)


class Placed:
    """Streams and output ranges at chosen alignments, the oracle's answer for exactly this placement (computed once), canary gaps between
    the output ranges."""

    def __init__(self, cases, caps, in_mod=None, out_mod=None):
        self.cases, self.caps = cases, caps
        nb = len(cases)
        in_off, out_off, ip, op = np.zeros(nb, np.int64), np.zeros(nb, np.int64), 0, 24
        for b, c in enumerate(cases):
            if in_mod is not None:
                ip += (in_mod[b] - ip) % 4
            if out_mod is not None:
                op += (out_mod[b] - op) % 16
            in_off[b], out_off[b] = ip, op
            ip += len(c.stream)
            op += int(caps[b]) + 24
        self.in_off, self.out_off, self.total = in_off, out_off, op
        self.in_len = np.array([len(c.stream) for c in cases], dtype=np.int32)
        data = np.zeros(ip + 64, dtype=np.uint8)
        for b, c in enumerate(cases):
            data[in_off[b]:in_off[b] + len(c.stream)] = np.frombuffer(c.stream, dtype=np.uint8)
        self.data = data
        self.ref, self.ref_len, self.ref_st = O.decompress_batch(data, in_off.astype(np.uint64), self.in_len.astype(np.uint32), out_off.astype(np.uint64),
                                                                 caps.astype(np.uint32), self.total, THREADS)
        # what may be written: the out_len bytes of an OK block, the capacity of a failed one -- but nothing at all of one that is too small
        allowed = np.zeros(self.total, dtype=bool)
        for b in range(nb):
            n = int(self.ref_len[b]) if self.ref_st[b] == O.OK else 0 if self.ref_st[b] == O.ERR_OUTPUT_TOO_SMALL else int(caps[b])
            allowed[out_off[b]:out_off[b] + n] = True
        self.allowed = allowed
        self.ok = np.nonzero(self.ref_st == O.OK)[0]
        self.ok_idx = np.concatenate([np.arange(out_off[b], out_off[b] + self.ref_len[b]) for b in self.ok]) if self.ok.size else np.zeros(0, np.int64)
        for b in self.ok:                                              # the generator's own output, where the stream is as built
            c = cases[b]
            if c.mutation is None:
                assert self.ref[out_off[b]:out_off[b] + len(c.raw)].tobytes() == c.raw and self.ref_len[b] == len(c.raw)
        self.d = [dev(self.data), dev(in_off), dev(self.in_len), dev(out_off), dev(caps.astype(np.int32))]

    def run(self, cd, what):
        out = torch.full((self.total,), CANARY, dtype=torch.uint8, device="cuda")
        dlen, dst = cd.decompress(self.d[0], self.d[1], self.d[2], out, self.d[3], self.d[4])
        torch.cuda.synchronize()
        dlen, dst, out = dlen.cpu().numpy(), dst.cpu().numpy(), out.cpu().numpy()
        bad = np.nonzero(dst != self.ref_st)[0]
        assert bad.size == 0, (f"{what}: status differs at blocks {bad[:8]}: got {dst[bad[:8]]} want {self.ref_st[bad[:8]]}; "
                               f"{[(self.cases[b].profile, self.cases[b].total, self.cases[b].mutation) for b in bad[:8]]}")
        assert (dlen[self.ok] == self.ref_len[self.ok]).all(), f"{what}: lengths differ"
        if not np.array_equal(out[self.ok_idx], self.ref[self.ok_idx]):
            for b in self.ok:
                o, n = int(self.out_off[b]), int(self.ref_len[b])
                if not np.array_equal(out[o:o + n], self.ref[o:o + n]):
                    at = int(np.nonzero(out[o:o + n] != self.ref[o:o + n])[0][0])
                    c = self.cases[b]
                    raise AssertionError(f"{what}: block {b} ({c.profile}, {c.total} bytes, {c.mutation}) differs from the oracle at byte {at}; "
                                         f"stream {c.stream.hex() if len(c.stream) <= 400 else c.stream[:400].hex() + '...'}")
        stray = np.nonzero((out != CANARY) & ~self.allowed)[0]
        assert stray.size == 0, f"{what}: bytes written outside the output ranges, first at {stray[:4]} (out_off {self.out_off[np.searchsorted(self.out_off, stray[:4], 'right') - 1]})"

    def summary(self):
        st, n = np.unique(self.ref_st, return_counts=True)
        return dict(blocks=len(self.cases), mutated=sum(c.mutation is not None for c in self.cases), statuses={int(s): int(k) for s, k in zip(st, n)})


# ---- (a) every batch decode layout ---------------------------------------------------------------------------------------------------------
@lru_cache(maxsize=None)
def corpus_placed():
    cases = G.batch_corpus()
    return Placed(cases, capacities(cases))


@pytest.mark.parametrize("decode,fenced", [(d, f) for d in layouts.DECODE_LAYOUTS for f in ((0, 1) if d in ("chains", "serial") else (None,))])
def test_every_decode_layout_on_the_grammar_corpus(decode, fenced):
    p = corpus_placed()
    assert len(p.cases) == 1500 and {c.profile for c in p.cases} == set(G.PROFILES)
    assert {O.OK, O.ERR_OUTPUT_TOO_SMALL, O.ERR_BAD_OFFSET, O.ERR_TOO_LONG, O.ERR_INCOMPLETE} <= set(p.ref_st.tolist())
    cd = SB.BlockCodec(0, O.HASH_CRC32C)
    layouts.set_decode_layout(cd.ctx, decode, fenced=fenced)
    for call in range(2):                                              # the second call runs under the policy the first one taught the context
        p.run(cd, f"{decode} fenced={fenced} call {call}")
    log(test="a", decode=decode, fenced=fenced, calls=2, **p.summary())


# ---- (b) placement -------------------------------------------------------------------------------------------------------------------------
@lru_cache(maxsize=None)
def corpus_aligned():
    cases = G.batch_corpus()
    seen, in_mod, out_mod = {p: 0 for p in G.PROFILES}, [], []
    for c in cases:                                                    # the k-th stream of a profile: combination k mod 64
        k = seen[c.profile]
        seen[c.profile] += 1
        in_mod.append(k % 4)
        out_mod.append(k // 4 % 16)
    return Placed(cases, capacities(cases), in_mod, out_mod)


@pytest.mark.parametrize("decode", layouts.DECODE_LAYOUTS)
def test_every_input_alignment_meets_every_output_alignment(decode):
    p = corpus_aligned()
    met = {(c.profile, int(i) % 4, int(o) % 16) for c, i, o in zip(p.cases, p.in_off, p.out_off)}
    assert met == {(prof, i, o) for prof in G.PROFILES for i in range(4) for o in range(16)}
    ok = {(c.profile, int(p.in_off[b]) % 4, int(p.out_off[b]) % 16) for b, c in enumerate(p.cases) if p.ref_st[b] == O.OK and c.mutation is None}
    assert len(ok) > 0.9 * len(met)
    cd = SB.BlockCodec(0, O.HASH_CRC32C)
    layouts.set_decode_layout(cd.ctx, decode)
    p.run(cd, f"{decode} aligned")
    log(test="b", decode=decode, combinations=len(met), **p.summary())


# ---- (c) the small-block layouts on their own ground -------------------------------------------------------------------------------------------
@lru_cache(maxsize=None)
def small_placed():
    cases = G.batch_corpus(4200, seed=1, lo=1, small=512, big=512, full=0)
    return Placed(cases, capacities(cases))


@pytest.mark.parametrize("layout", ["lanes", "team4", "team8", "team16"])
def test_small_block_layouts_on_grammar_blocks(layout):
    p = small_placed()
    assert len(p.cases) >= 4096 and all(1 <= c.total <= 512 for c in p.cases) and 3 * sum(c.mutation is not None for c in p.cases) >= len(p.cases) - 3
    cd = SB.BlockCodec(0, O.HASH_CRC32C)
    layouts.set_decode_layout(cd.ctx, "small-" + layout, small_max=512)
    for call in range(2):
        p.run(cd, f"small-{layout} call {call}")
    log(test="c", layout=layout, calls=2, **p.summary())


# ---- (d) large single blocks through the host API ------------------------------------------------------------------------------------------
@pytest.fixture(params=["default", "min1", "off"])
def ctx(request):
    """The contexts of test_gpu_big_blocks.py: the parallel path from 256 KiB, for every block, never."""
    par_min = {"default": 262144, "min1": 1, "off": 0}[request.param]
    c = S.Context(0, O.HASH_CRC32C)
    c.set_option(N.OPT_PARALLEL_DECODE_MIN, par_min)
    c.par_min = par_min
    return c


def test_large_fragment_local_streams_decode_by_fragments(ctx):
    seen = {}
    for profile in G.PROFILES:
        c = G.large_local(profile)
        before = [ctx.counter(k) for k in (0, 1, 6)]
        assert S.Snappy.DecompressToArray(c.stream, ctx) == c.raw, profile
        after = [ctx.counter(k) for k in (0, 1, 6)]
        took = ctx.par_min != 0 and c.total >= ctx.par_min
        seen[profile] = [a - b for a, b in zip(after, before)]
        # a fragment_local stream is what the fragment decoder takes with no fallback (decode_common.h: no tag straddles a fragment start,
        # no copy reaches before it); the tag index's look-back decision is the model's (stream_grammar.LARGE_LOOK_BACK)
        assert seen[profile][:2] == ([1, 0] if took else [0, 0]), (profile, seen[profile])
        if took:
            assert seen[profile][2] == G.LARGE_LOOK_BACK[profile], (profile, seen[profile])
    out = np.full(G.LARGE_LOCAL["copy4"] + 4096, CANARY, dtype=np.uint8)
    c = G.large_local("copy4")
    ok, written = S.Snappy.TryDecompress(c.stream, out, ctx)
    assert ok and written == c.total and out[:written].tobytes() == c.raw and (out[written:] == CANARY).all()
    log(test="d-local", par_min=ctx.par_min, streams=len(G.PROFILES), mutated=0, counters_0_1_6=seen)


def test_large_streams_the_fragment_decoder_cannot_take_fall_back(ctx):
    seen = []
    for k in range(len(G.LARGE_FOREIGN)):
        c = G.large_foreign(k)
        before = ctx.counter(1)
        assert S.Snappy.DecompressToArray(c.stream, ctx) == c.raw, G.LARGE_FOREIGN[k]
        seen.append(ctx.counter(1) - before)
        assert seen[-1] == (1 if ctx.par_min != 0 and c.total >= ctx.par_min else 0), (G.LARGE_FOREIGN[k], seen)
    log(test="d-foreign", par_min=ctx.par_min, streams=len(seen), mutated=0, counter_1=seen)


def test_large_near_misses_raise_the_oracle_status(ctx):
    seen = []
    for k in range(8):
        c = G.large_mutated(k)
        want = O.decompress_status(c.stream)
        assert c.mutation is not None and want != O.OK, (k, c.mutation)
        with pytest.raises(InvalidDataException) as ei:
            S.Snappy.DecompressToArray(c.stream, ctx)
        assert ei.value.status == want, (k, c.profile, c.mutation)
        seen.append((c.mutation, want))
    log(test="d-mutated", par_min=ctx.par_min, streams=8, mutated=8, statuses=seen)


# ---- (e) decompress_buffers ----------------------------------------------------------------------------------------------------------------
def test_decompress_buffers_on_grammar_streams_among_good_blocks():
    par_min = 131072
    good = [O.compress(DB.corpus_bytes(n, n), O.HASH_CRC32C) for n in (300000, 77777)]
    local = [G.large_local(p, True) for p in G.PROFILES if p != "dense"]
    dense = G.large_local("dense")
    foreign = [G.large_foreign(k) for k in range(len(G.LARGE_FOREIGN))]
    bad = [G.large_mutated(k) for k in range(4)]
    order = [good[0]] + [x.stream for pair in zip(local[:4], foreign) for x in pair] + [dense.stream] + [x.stream for x in bad] + [x.stream for x in local[4:]] + [good[1]]
    kinds = ["good"] + ["local", "foreign"] * 4 + ["dense"] + ["bad"] * 4 + ["local"] * len(local[4:]) + ["good"]
    batch = DB.Batch(order, [declared_of(s) + 7 for s in order])
    cd = SB.BlockCodec(0, O.HASH_CRC32C)
    cd.ctx.set_option(N.OPT_PARALLEL_DECODE_MIN, par_min)
    ref = batch.run(cd, False)
    cand = batch.candidates(par_min)
    got = batch.run(cd, True, max_fragments=DB.nfrags(batch, cand))
    DB.check("grammar", batch, got, ref)
    for b, s in enumerate(order):
        assert got[2][b] == O.decompress_status(s), (b, kinds[b])
    for c in local + [dense] + foreign:
        assert got[0][batch.out_off[order.index(c.stream)]:][:c.total].tobytes() == c.raw
    # the bounded fragment_local streams and the foreign ones are candidates; a dense stream is several times its output: over the bound, none
    assert {b for b, k in enumerate(kinds) if k in ("local", "foreign", "bad")} | {0} <= set(cand)
    assert kinds.index("dense") not in cand and len(order) - 1 not in cand         # (77777 bytes: below par_min)
    fell_back = {b for b, k in enumerate(kinds) if k in ("foreign", "bad")}
    res = got[3]
    assert res[0] == DB.nfrags(batch, cand) and res[1] == len(cand) - len(fell_back) and res[2] == len(fell_back), (res.tolist(), cand, sorted(fell_back))
    log(test="e", blocks=len(order), mutated=len(bad), statuses=sorted(set(int(x) for x in got[2])), candidates=len(cand), d_result=[int(x) for x in res])


# ---- (f) the framed calls ------------------------------------------------------------------------------------------------------------------
def frame_statuses():
    out = []
    for _name, s, _raws in G.frame_corpus():
        try:
            O.frame_decode(s)
            out.append(O.OK)
        except O.OracleError as e:
            out.append(e.status)
    return out


def test_frame_decode_buffers_on_foreign_chunks():
    frames = G.frame_corpus()
    streams = [s for _n, s, _r in frames]
    assert len(streams) == 8 and {len(r) for _n, _s, r in frames} == {1, 2, 3, 4, 5}
    caps = [O.frame_decoded_length(s) + b % 3 for b, s in enumerate(streams)]
    cd = SB.BlockCodec(0, O.HASH_CRC32C)
    got = H.decode(cd, streams, caps)
    H.check_decode(cd, streams, caps, got)
    h, out_off, ol, st, _res = got
    assert st.tolist() == frame_statuses() and sorted(set(st.tolist())) == [O.OK, O.ERR_BAD_OFFSET, O.ERR_CRC_MISMATCH]
    for b, (_name, _s, raws) in enumerate(frames):
        if st[b] == O.OK:
            assert h[out_off[b]:out_off[b] + ol[b]].tobytes() == b"".join(raws)
    log(test="f-decode", streams=8, chunks=sum(len(r) for _n, _s, r in frames), mutated=2, statuses=st.tolist())


def frame_windows():
    """(stream, window) for every window shape of frame_range_model.windows over every framed stream: inside, across and at the ends of chunks."""
    out = []
    for b, (_name, s, _raws) in enumerate(G.frame_corpus()):
        rows, total, _, _ = R.walk(s)
        out += [(b, w) for w in R.windows(rows, total)]
    return out


def test_frame_decode_range_buffers_on_foreign_chunks():
    frames = G.frame_corpus()
    pairs = frame_windows()
    streams, ranges = [frames[b][1] for b, _w in pairs], [w for _b, w in pairs]
    cd = SB.BlockCodec(0, O.HASH_CRC32C)
    got = FR.check(cd, streams, ranges, FR.exact_caps(streams, ranges, slack=1))
    good = 0
    for (b, w), st, data in zip(pairs, got[0], got[2]):
        if frame_statuses()[b] == O.OK:
            whole = b"".join(frames[b][2])
            lo, hi = R.clip(len(whole), *w)
            assert st == O.OK and data == whole[lo:hi], (frames[b][0], w)
            good += 1
    assert good > 100 and sorted(set(got[0])) == [O.OK, O.ERR_BAD_OFFSET, O.ERR_CRC_MISMATCH]
    log(test="f-range", windows=len(pairs), ok_windows=got[0].count(O.OK), statuses=sorted(set(got[0])), d_result=got[3])


def test_frame_index_and_indexed_reads_on_foreign_chunks():
    frames = G.frame_corpus()
    streams = [s for _n, s, _r in frames]
    cd = SB.BlockCodec(0, O.HASH_CRC32C)
    ix = FI.index_call(cd, streams)
    assert ix == X.build_index(streams)
    reqs = FI.interleaved([(b, w[0], w[1]) for b, w in frame_windows()])
    got = FI.check(cd, streams, ix, reqs, FI.exact_caps(streams, reqs, slack=1))
    for (b, ro, rl), st, data in zip(reqs, got[0], got[2]):
        if frame_statuses()[b] == O.OK:
            whole = b"".join(frames[b][2])
            lo, hi = R.clip(len(whole), ro, rl)
            assert st == O.OK and data == whole[lo:hi], (frames[b][0], ro, rl)
    assert sorted(set(got[0])) == [O.OK, O.ERR_BAD_OFFSET, O.ERR_CRC_MISMATCH]
    log(test="f-index", requests=len(reqs), ok_requests=got[0].count(O.OK), rows=len(ix["start"]), statuses=sorted(set(got[0])), d_result=got[3])

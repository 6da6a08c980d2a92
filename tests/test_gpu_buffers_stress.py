"""snp_decompress_buffers_batch at scale, on corrupt streams and under every decode option: the batched tag index (k_bd_tag_cand, k_bd_tag_scan,
k_bd_tag_look_back -- drivers of the per-chunk code that tag_index.hip's kernels run), the makespan rule, admission by max_fragments, the plan scans
past 256 tiles (and the two scans of snp_compress_buffers_batch), the fallback list.  References: the oracle for bytes and statuses,
snp_decompress_batch on the same arguments, the NumPy plan() of tests/test_decompress_buffers_model.py for d_result[0..2], and the
single-block path (snp_try_decompress) for each stream's look-back decision, d_result[3].  Needs an MI355X."""
import numpy as np
import pytest
import torch

import layouts
import oracle as O
import shaped_streams as SS
from conftest import CORPUS, read_testdata
from test_decompress_buffers_model import plan
from test_gpu_decompress_buffers import CANARY, declared_of, foreign_streams, malformed_streams, preamble, ragged_batch, varint

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    import snappier_amd as S
    from snappier_amd import batch as SB, _native as N

B = 65536
PAR_MIN = 262144
SCAN_TILES = 256 * 1024                     # values k_scan_partials carries in its first round (256 tiles of SNP_SCAN_TILE)


def dev(a: np.ndarray):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def wave_slots() -> int:
    return torch.cuda.get_device_properties(0).multi_processor_count * 32


def codec(par_min=None):
    cd = SB.BlockCodec(0, O.HASH_CRC32C)
    if par_min is not None:
        cd.ctx.set_option(N.OPT_PARALLEL_DECODE_MIN, par_min)
    return cd


def frags(n: int) -> int:
    return (n + B - 1) // B


def covered(size: int, starts: np.ndarray, lens: np.ndarray) -> np.ndarray:
    """Bytes inside any of the ranges [start, start + len)."""
    d = np.zeros(size + 1, np.int64)
    np.add.at(d, starts, 1)
    np.add.at(d, starts + lens, -1)
    return np.cumsum(d[:-1]) > 0


def groups(which: np.ndarray, mask: np.ndarray):
    """-> [(value, indices of the masked positions holding it)]."""
    idx = np.nonzero(mask)[0]
    order = idx[np.argsort(which[idx], kind="stable")]
    vals, starts = np.unique(which[order], return_index=True)
    return zip(vals.tolist(), np.split(order, starts[1:]))


_corpus = None


def corpus_all() -> bytes:
    global _corpus
    if _corpus is None:
        _corpus = b"".join(read_testdata(n) for n in CORPUS)
    return _corpus


class Aliased:
    """Blocks that point at a few distinct streams (blocks of one stream share its in_off: aliased inputs), packed at odd and even offsets;
    every block has its own output range, canary gaps between them."""

    def __init__(self, streams, which, caps, gap=7):
        self.streams = list(streams)
        self.which = np.asarray(which, dtype=np.int64)
        s_off, pos = [], 3
        for s in self.streams:
            s_off.append(pos)
            pos += len(s) + 5
        buf = np.zeros(pos + 16, dtype=np.uint8)
        for o, s in zip(s_off, self.streams):
            buf[o:o + len(s)] = np.frombuffer(s, dtype=np.uint8)
        self.comp = dev(buf)
        self.in_off = np.asarray(s_off, np.int64)[self.which]
        self.in_len = np.array([len(s) for s in self.streams], np.int64)[self.which]
        self.caps = np.asarray(caps, dtype=np.int64)
        self.decl = np.array([declared_of(s) for s in self.streams], np.int64)[self.which]
        self.out_off = (gap + np.concatenate([[0], np.cumsum(self.caps + gap)[:-1]])).astype(np.int64)
        self.out_size = int(self.out_off[-1] + self.caps[-1] + gap)
        self.d = dict(in_off=dev(self.in_off), in_len=dev(self.in_len.astype(np.uint32).view(np.int32)), out_off=dev(self.out_off),
                      out_cap=dev(self.caps.astype(np.uint32).view(np.int32)))
        self._want = None

    def blocks(self):
        return [self.streams[w] for w in self.which]

    def plan(self, par_min, max_fragments):
        return plan(self.blocks(), self.caps, par_min, wave_slots(), max_fragments)

    def run(self, cd, buffers: bool, max_fragments=None):
        out = torch.full((self.out_size,), CANARY, dtype=torch.uint8, device="cuda")
        if buffers:
            ol, st, res = cd.decompress_buffers(self.comp, self.d["in_off"], self.d["in_len"], out, self.d["out_off"], self.d["out_cap"],
                                                max_fragments=max_fragments)
        else:
            ol, st = cd.decompress(self.comp, self.d["in_off"], self.d["in_len"], out, self.d["out_off"], self.d["out_cap"])
            res = None
        torch.cuda.synchronize()
        return out.cpu().numpy(), ol.cpu().numpy(), st.cpu().numpy(), None if res is None else res.cpu().numpy()

    def oracle(self):
        """Per distinct stream: (status, bytes or None), computed once."""
        if self._want is None:
            self._want = []
            for s in self.streams:
                st = O.decompress_status(s)
                self._want.append((st, O.decompress(s) if st == O.OK else None))
        return self._want

    def compared(self, st, ol):
        """-> (mask of the bytes every run must agree on: the OK blocks' bytes and everything outside the output ranges, expected bytes)."""
        want = self.oracle()
        ok = st == O.OK
        mask = ~covered(self.out_size, self.out_off, self.caps)
        exp = np.full(self.out_size, CANARY, dtype=np.uint8)
        for w, blks in groups(self.which, ok):
            data = np.frombuffer(want[w][1], dtype=np.uint8)
            if data.size > 4096:
                for o in self.out_off[blks]:
                    exp[o:o + data.size] = data
                    mask[o:o + data.size] = True
            elif data.size:
                at = self.out_off[blks][:, None] + np.arange(data.size)[None, :]
                exp[at] = data
                mask[at] = True
        return mask, exp

    def check(self, tag, got, ref):
        """snp_decompress_batch's statuses, out_len and bytes; the oracle's status (or a capacity below the declared length) and bytes; canaries."""
        out, ol, st, _ = got
        r_out, r_ol, r_st, _ = ref
        diff = np.nonzero(st != r_st)[0]
        assert diff.size == 0, f"{tag}: statuses differ from snp_decompress_batch at blocks {diff[:8].tolist()}: {st[diff[:8]].tolist()} vs {r_st[diff[:8]].tolist()}"
        diff = np.nonzero(ol != r_ol)[0]
        assert diff.size == 0, f"{tag}: out_len differs from snp_decompress_batch at blocks {diff[:8].tolist()}"
        want = self.oracle()
        w_st = np.array([w[0] for w in want])[self.which]
        bad = np.nonzero((st != w_st) & ~(self.caps < self.decl))[0]
        assert bad.size == 0, f"{tag}: status differs from the oracle at blocks {bad[:8].tolist()}: {st[bad[:8]].tolist()} vs {w_st[bad[:8]].tolist()}"
        w_len = np.array([len(w[1]) if w[1] is not None else -1 for w in want])[self.which]
        ok = st == O.OK
        bad = np.nonzero(ok & (ol != w_len))[0]
        assert bad.size == 0, f"{tag}: out_len differs from the oracle at blocks {bad[:8].tolist()}"
        mask, exp = self.compared(st, ol)
        for name, arr in (("the batched call", out), ("snp_decompress_batch", r_out)):
            wrong = np.nonzero(arr[mask] != exp[mask])[0]
            if wrong.size:
                pos = int(np.nonzero(mask)[0][wrong[0]])
                b = int(np.searchsorted(self.out_off, pos, side="right")) - 1
                inside = b >= 0 and pos < self.out_off[b] + self.caps[b]
                raise AssertionError(f"{tag}: {name}: byte {pos} " + (f"of block {b} differs from the oracle" if inside else "outside the output ranges was written"))


def single_block_look_back(streams, par_min):
    """The single-block path's decision per stream: the ctx.counter(6) delta of Snappy.DecompressToArray (and the bytes)."""
    ctx = S.Context(0, O.HASH_CRC32C)
    ctx.set_option(N.OPT_PARALLEL_DECODE_MIN, par_min)
    got = []
    for s in streams:
        before, frag_before = ctx.counter(6), ctx.counter(0)
        assert S.Snappy.DecompressToArray(s, ctx) == O.decompress(s)
        assert ctx.counter(0) == frag_before + 1                           # (decoded by fragments)
        got.append(ctx.counter(6) - before)
    ctx.close()
    return got


# ---- 1. scale and plan boundaries ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("extra", [0, 1])
def test_makespan_boundary_splits_every_block_or_none(extra):
    """N = wave slots / 2 blocks of one declared length: d * slots >= 2 * N * d splits every one of them; one block more splits none.  The
    N-block batch also gives each of the 256 scan workgroups N / 256 blocks in turn: RunCache slots and tickets are reused across blocks."""
    slots = wave_slots()
    nb = slots // 2 + extra
    d = 20000
    corpus = corpus_all()
    stride = len(corpus) // 64
    streams = [O.compress(corpus[k * stride:k * stride + d], O.HASH_CRC32C if k % 2 else O.HASH_MUL) for k in range(64)]
    which = np.arange(nb) % 64
    rng = np.random.default_rng(nb)
    batch = Aliased(streams, which, d + rng.integers(0, 64, nb))
    cd = codec(1)
    ref = batch.run(cd, False)
    got = batch.run(cd, True, max_fragments=nb)
    batch.check(f"{nb} blocks", got, ref)
    assert (got[2] == O.OK).all()
    P = batch.plan(1, nb)
    lbo = np.array([SS.look_back_only(s, d) for s in streams])[which]
    if extra == 0:
        assert P["needed"] == nb and P["admitted"].all()
        assert 0 < lbo.sum() < nb                                           # (one-chunk streams take the look-back pass by the 85 % rule only)
        assert got[3].tolist() == [nb, nb, 0, int(lbo.sum())], got[3]
    else:
        assert P["needed"] == 0
        assert got[3].tolist() == [0, 0, 0, 0], got[3]


def tiles_mix(rng, nb):
    """-> (distinct streams, block -> stream, caps, indices of the big streams): every 97th block a 66 536-byte stream (2 fragments), the
    rest 0-200-byte streams, empty and malformed ones among them."""
    corpus = corpus_all()
    big = []
    for k in range(24):
        n = 66536
        data = (SS.low_entropy_bytes(n, 300 + k) if k % 3 == 0 else SS.random_bytes(n, 300 + k) if k % 3 == 1
                else corpus[k * 97001:k * 97001 + n])
        big.append(O.compress(data, O.HASH_CRC32C if k % 2 else O.HASH_MUL))
    small = [b""]
    for k in range(400):
        n = int(rng.integers(0, 201))
        o = int(rng.integers(0, len(corpus) - n))
        small.append(O.compress(corpus[o:o + n], O.HASH_CRC32C if k % 2 else O.HASH_MUL))
    good = O.compress(corpus[5000:5150])
    malformed = [b"\xff\xff\xff\xff\xff\x01" + good[3:], varint(150), good[:-7], varint(140) + good[2:], good[:40] + bytes(8) + good[48:]]
    streams = big + small + malformed
    n_small = len(small) + len(malformed)
    which = len(big) + rng.integers(0, n_small, nb)
    which[rng.random(nb) < 0.01] = len(big)                                 # ~1 % empty blocks
    which[rng.random(nb) < 0.01] = len(big) + len(small) + rng.integers(0, len(malformed))
    big_at = np.arange(0, nb, 97)
    which[big_at] = big_at // 97 % len(big)
    caps = np.empty(nb, np.int64)
    for w, blks in groups(which, np.ones(nb, bool)):
        clean, dcl, _ = preamble(streams[w])
        caps[blks] = (dcl if clean and dcl <= 66536 else 256) + rng.integers(0, 64, blks.size)
    return streams, which, caps, list(range(len(big)))


def test_decompress_plan_scans_past_256_tiles():
    """~300 000 blocks: every plan scan (decl, first, packed) runs k_scan_partials' carry past its first 256 tiles with non-zero values there.
    Admission by max_fragments: exact, then 5 short -- the last three chosen blocks (in the final tile group) are cut off."""
    rng = np.random.default_rng(300000)
    nb = 300_000
    streams, which, caps, big = tiles_mix(rng, nb)
    batch = Aliased(streams, which, caps, gap=3)
    par_min = 65537
    cd = codec(par_min)
    ref = batch.run(cd, False)
    need = batch.plan(par_min, 1 << 26)["needed"]
    n_big = len(range(0, nb, 97))
    assert need == 2 * n_big                                                # (every big block is chosen)
    look_back = dict(zip(big, single_block_look_back([streams[w] for w in big], par_min)))
    for mf in (need, need - 5):
        P = batch.plan(par_min, mf)
        chosen = np.nonzero(P["first"][1:] > P["first"][:-1])[0]
        adm = np.nonzero(P["admitted"])[0]
        assert chosen[-1] >= SCAN_TILES and adm[-1] >= SCAN_TILES and P["decl"][SCAN_TILES:].any()
        if mf < need:
            assert adm.tolist() == chosen[:-3].tolist()
        got = batch.run(cd, True, max_fragments=mf)
        batch.check(f"max_fragments={mf}", got, ref)
        lb = sum(look_back[int(w)] for w in which[adm])
        assert got[3].tolist() == [P["needed"], len(adm), 0, lb], (mf, got[3].tolist())
    assert (ref[2] == O.OK).sum() > nb * 0.9


def test_compress_buffers_scans_past_256_tiles():
    """snp_compress_buffers_batch on ~300 000 buffers of the same length mix (> 262 144 fragments): both of its scans carry past 256 tiles.
    Every buffer's bytes are the oracle's (computed once per distinct input)."""
    from test_gpu_compress_buffers import SENTINEL, cap_of, nfrag, run
    from snappier_amd import datagen as SD
    rng = np.random.default_rng(262145)
    nb = 300_000
    html = read_testdata("html")
    data = torch.cat([SD.html_like_blocks(html, 3, 64, "cuda"), torch.randint(0, 256, (1 << 20,), dtype=torch.uint8, device="cuda")])
    h = data.cpu().numpy()
    pairs = [(int(rng.integers(0, h.size - 66536)), 66536) for _ in range(32)]
    pairs += [(int(rng.integers(0, h.size - 200)) | int(rng.integers(0, 2)), int(rng.integers(0, 201))) for _ in range(400)]
    which = 32 + rng.integers(0, 400, nb)
    big_at = np.arange(0, nb, 97)
    which[big_at] = big_at // 97 % 32
    p_off = np.array([p[0] for p in pairs], np.int64)
    p_len = np.array([p[1] for p in pairs], np.int64)
    in_off, lens = p_off[which], p_len[which]
    nf = nfrag(lens)
    assert nf > SCAN_TILES and nb > SCAN_TILES
    cd = codec()
    out, out_off, out_len, status, result = run(cd, data, in_off, lens, max_fragments=nf, gap=1)
    assert (status == 0).all()
    exp = np.full(out.size, SENTINEL, dtype=np.uint8)
    for p, blks in groups(which, np.ones(nb, bool)):
        o, n = pairs[p]
        ref = np.frombuffer(O.compress(h[o:o + n].tobytes(), O.HASH_CRC32C), dtype=np.uint8)
        bad = np.nonzero(out_len[blks] != ref.size)[0]
        assert bad.size == 0, f"buffer {int(blks[bad[0]])}: out_len {int(out_len[blks[bad[0]]])}, the oracle {ref.size}"
        exp[out_off[blks][:, None] + np.arange(ref.size)[None, :]] = ref
    wrong = np.nonzero(out != exp)[0]
    assert wrong.size == 0, f"byte {int(wrong[0])} (buffer {int(np.searchsorted(out_off, wrong[0], side='right')) - 1}) differs"
    assert result.tolist() == [nf, int(out_len.sum())]


# ---- 2. the tag-index decision: the batched copy and the single-block copy agree -------------------------------------------------------------

@pytest.fixture(scope="module")
def shaped():
    """S1..S5 (tests/shaped_streams.py) and the single-block path's look-back decision for each."""
    streams = [SS.stream(name) for name in SS.SHAPES]
    return streams, dict(zip(SS.SHAPES, single_block_look_back(streams, PAR_MIN)))


@pytest.mark.parametrize("name", SS.SHAPES)
def test_shaped_stream_alone_takes_the_single_block_decision(shaped, name):
    streams, single = shaped
    s = streams[SS.SHAPES.index(name)]
    assert single[name] == SS.LOOK_BACK[name], (name, single[name])       # the single-block kernels agree with the model (test_tag_index_model.py)
    d = declared_of(s)
    batch = Aliased([s], [0], [d + 3])
    cd = codec(PAR_MIN)
    got = batch.run(cd, True, max_fragments=frags(d))
    batch.check(name, got, batch.run(cd, False))
    assert got[3].tolist() == [frags(d), 1, 0, single[name]], (name, got[3].tolist())


def test_shaped_streams_in_one_batch_each_decode_from_their_own_entries(shaped):
    """S1..S5 twice each, interleaved: the flagged blocks (S3 by the 85 % rule, S5 by the scan giving up) take the look-back pass while the
    others keep their scanned entries."""
    streams, single = shaped
    order = ["S1", "S3", "S2", "S5", "S4", "S3", "S1", "S5", "S2", "S4"]
    which = [SS.SHAPES.index(n) for n in order]
    caps = [declared_of(streams[w]) + 1 + 2 * i for i, w in enumerate(which)]
    batch = Aliased(streams, which, caps, gap=11)
    cd = codec(PAR_MIN)
    need = sum(frags(declared_of(streams[w])) for w in which)
    P = batch.plan(PAR_MIN, need)
    assert P["needed"] == need and P["admitted"].all()
    got = batch.run(cd, True, max_fragments=need)
    batch.check("shaped", got, batch.run(cd, False))
    assert got[3].tolist() == [need, len(order), 0, sum(single[n] for n in order)] == [need, 10, 0, 4], got[3].tolist()


# ---- 3. corrupted streams in batches --------------------------------------------------------------------------------------------------------

_low = None


def low_entropy_pool() -> bytes:
    global _low
    if _low is None:
        _low = SS.low_entropy_bytes(3 << 20, 77)
    return _low


@pytest.mark.parametrize("seed,mf_kind", [(1, "exact"), (2, "half"), (3, "default")])
def test_corrupted_blocks_in_batches(seed, mf_kind):
    import test_gpu_fuzz as F
    rng = np.random.default_rng(4242 + seed)
    corpus, low = corpus_all(), low_entropy_pool()
    sizes = [int(rng.integers(200000, 1500000)) for _ in range(64)] + [int(np.exp(rng.uniform(0, np.log(400000)))) for _ in range(16)]
    streams = []
    for i, n in enumerate(sizes):
        src = corpus if i % 2 == 0 else low
        o = int(rng.integers(0, len(src) - n))
        z = np.frombuffer(O.compress(src[o:o + n], O.HASH_CRC32C if i % 4 < 2 else O.HASH_MUL), dtype=np.uint8)
        streams.append(F.corrupt(rng, z).tobytes())
    caps = []
    for s in streams:
        clean, d, _ = preamble(s)
        caps.append(max(d + int(rng.integers(-1, 65)), 1) if clean and d <= (2 << 20) else 1 << 20)
    order = rng.permutation(len(streams))
    streams = [streams[i] for i in order]
    caps = [caps[i] for i in order]
    batch = Aliased(streams, np.arange(len(streams)), caps, gap=5)
    cd = codec()
    need = batch.plan(PAR_MIN, 1 << 26)["needed"]
    mf = {"exact": need, "half": need // 2, "default": None}[mf_kind]
    used = mf if mf is not None else int(sum(frags(int(c)) for c in caps))   # (the wrapper's default: sum of ceil(out_cap / 65536))
    P = batch.plan(PAR_MIN, used)
    ref = batch.run(cd, False)
    got = batch.run(cd, True, max_fragments=mf)
    batch.check(f"seed {seed}", got, ref)
    res = got[3]
    assert res[0] == P["needed"] == need, res
    assert res[1] + res[2] == P["admitted"].sum(), res
    st = got[2]
    assert (st == O.OK).any() and (st != O.OK).any() and P["admitted"].sum() > 0


# ---- 4. every decode option through the batched call ---------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def mixed():
    """The ragged batch, the foreign and malformed streams, S3 and S5, and ~300 blocks of <= 4 KiB: with its default run."""
    rb = ragged_batch(5)
    streams = list(rb.streams) + foreign_streams() + list(malformed_streams().values()) + [SS.stream("S3"), SS.stream("S5")]
    rng = np.random.default_rng(17)
    corpus = corpus_all()
    for k in range(300):
        n = int(rng.integers(0, 4097))
        o = int(rng.integers(0, len(corpus) - n))
        streams.append(O.compress(corpus[o:o + n], O.HASH_MUL if k % 3 else O.HASH_CRC32C))
    rng.shuffle(streams)
    caps = [declared_of(s) + int(rng.integers(0, 50)) if preamble(s)[0] else 1 << 20 for s in streams]
    batch = Aliased(streams, np.arange(len(streams)), caps, gap=13)
    cd = codec()
    P = batch.plan(PAR_MIN, 1 << 26)
    mf = P["needed"]
    base = batch.run(cd, True, max_fragments=mf)
    batch.check("defaults", base, batch.run(cd, False))
    res = base[3]
    assert res[0] == mf and res[1] + res[2] == P["admitted"].sum(), res
    assert res[1] and res[2] and res[3], res                               # (fragments, fallbacks and look-back passes all in play)
    return batch, mf, base


def same_as_default(tag, batch, got, base):
    out, ol, st, res = got
    b_out, b_ol, b_st, b_res = base
    assert res.tolist() == b_res.tolist(), f"{tag}: d_result {res.tolist()} vs {b_res.tolist()}"
    assert np.array_equal(st, b_st), f"{tag}: statuses differ at blocks {np.nonzero(st != b_st)[0][:8].tolist()}"
    assert np.array_equal(ol, b_ol), f"{tag}: out_len differs at blocks {np.nonzero(ol != b_ol)[0][:8].tolist()}"
    mask, exp = batch.compared(b_st, b_ol)
    wrong = np.nonzero(out[mask] != exp[mask])[0]
    assert wrong.size == 0, f"{tag}: byte {int(np.nonzero(mask)[0][wrong[0]])} differs from the default run (the oracle's bytes and canaries)"


@pytest.mark.parametrize("fenced", [0, 1])
@pytest.mark.parametrize("decode", layouts.DECODE_LAYOUTS)
def test_every_decode_layout_changes_nothing(mixed, decode, fenced):
    batch, mf, base = mixed
    cd = codec()
    layouts.set_decode_layout(cd.ctx, decode, fenced)
    same_as_default(f"{decode} fenced={fenced}", batch, batch.run(cd, True, max_fragments=mf), base)


@pytest.mark.parametrize("throttle", [256, 32768, 65536])
def test_decode_lds_throttle_changes_nothing(mixed, throttle):
    batch, mf, base = mixed
    cd = codec()
    cd.ctx.set_option(N.OPT_DECODE_LDS_THROTTLE, throttle)
    assert cd.ctx.get_option(N.OPT_DECODE_LDS_THROTTLE) == throttle
    same_as_default(f"throttle {throttle}", batch, batch.run(cd, True, max_fragments=mf), base)

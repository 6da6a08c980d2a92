"""Every compressor configuration on directed and fuzzed inputs, every block compared with the oracle.

snp_launch_compress_lanes picks the lane kernel's launch form from the batch size (compress_lanes.hip:717-747; layouts.COMPRESS_TIERS names the four
forms), so the forms the large batches of the benchmark run on -- output staged in LDS, one exchange probe per trip, the 16-byte input register window --
never met ragged structured input with every block compared.  Here every entry of layouts.COMPRESS_LAYOUTS, both hashes:
  (a) the directed set of compress_inputs.py (every event class of the reference parse, confirmed by its tracer) plus one round of fuzz blocks, in the
      tight output layout with 24-byte gaps filled with 0xA5: length and bytes of every block, nothing written outside a block's own area, and back;
  (b) the directed set at every input and every output residue mod 16;
  (c) every directed fragment followed by bytes that would continue its last match, by 0xFF and by zeros: the output may not depend on them;
  (d) the policy as shipped (no lane option set) on 131 072 and 32 768 fragments of up to 4 096 bytes.
Needs an MI355X."""
import functools

import numpy as np
import pytest
import torch

import oracle as O
from conftest import read_testdata
import compress_inputs as CI
import layouts
from test_gpu_fuzz import THREADS, _compare_batch, dev

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from snappier_amd import batch as SB, _native as N

VARIANTS = [O.HASH_CRC32C, O.HASH_MUL]
PLACED_LAYOUTS = ["win", "wing", "lanes-opts215-slots1-per64", "lanes-opts87-slots2-per32"]
FUZZ_BLOCKS = 768
GAP = 24
FILL = 0xA5


def _text():
    return np.frombuffer(read_testdata("html") + read_testdata("alice29.txt"), dtype=np.uint8)


def max_compressed_length(lens: np.ndarray) -> np.ndarray:
    lens = lens.astype(np.int64)
    return 32 + lens + lens // 6 + 1 + 5                                # Snappy.GetMaxCompressedLength  Snappy.cs:20-24 (as _compare_batch)


class Batch:
    """Fragments laid out in one input buffer (at in_off, whatever lies between them), their tight output layout (every block exactly
    snp_max_compressed_length of its length, GAP bytes between the areas, or the residues asked for) and the oracle's stream of every block."""

    def __init__(self, data: np.ndarray, in_off: np.ndarray, lens: np.ndarray, variant: int, out_residue: np.ndarray | None = None):
        self.data, self.in_off, self.lens, self.variant = data, in_off.astype(np.int64), lens.astype(np.int32), variant
        nb = len(lens)
        self.caps = max_compressed_length(self.lens)
        self.out_off = np.zeros(nb, dtype=np.int64)
        at = GAP
        for b in range(nb):
            if out_residue is not None:
                at += (int(out_residue[b]) - at) % 16
            self.out_off[b] = at
            at += int(self.caps[b]) + GAP
        self.out_size = at + 64
        ref, ref_off, ref_len, ref_st = O.compress_batch(data, self.in_off.astype(np.uint64), self.lens.astype(np.uint32), variant, THREADS)
        assert (ref_st == 0).all()
        self.ref, self.ref_off, self.ref_len = ref, ref_off.astype(np.int64), ref_len.astype(np.int64)
        edge = np.zeros(self.out_size + 1, dtype=np.int32)              # which output bytes belong to no block
        np.add.at(edge, self.out_off, 1)
        np.add.at(edge, self.out_off + self.caps, -1)
        self.outside = np.cumsum(edge[:-1]) == 0
        self.dev = None

    def on_device(self):
        if self.dev is None:
            self.dev = (dev(self.data), dev(self.in_off), dev(self.lens), dev(self.out_off))
        return self.dev

    def check(self, cd, what: str) -> np.ndarray:
        """Compress on the device; length and bytes of every block against the oracle; the bytes of no block untouched; decompress back.  -> the output."""
        d_data, d_off, d_lens, d_coff = self.on_device()
        out = torch.full((self.out_size,), FILL, dtype=torch.uint8, device="cuda")
        _o, _oo, out_len, status = cd.compress(d_data, d_off, d_lens, out=out, out_off=d_coff)
        torch.cuda.synchronize()
        assert int((status != 0).sum()) == 0, what
        h_len, h_out = out_len.cpu().numpy().astype(np.int64), out.cpu().numpy()
        bad = np.nonzero(h_len != self.ref_len)[0]
        assert bad.size == 0, f"{what}: lengths differ at blocks {bad[:8]} (input lengths {self.lens[bad[:8]]}): got {h_len[bad[:8]]} want {self.ref_len[bad[:8]]}"
        for b in range(len(self.lens)):
            o, r, l = self.out_off[b], self.ref_off[b], self.ref_len[b]
            if not np.array_equal(h_out[o: o + l], self.ref[r: r + l]):
                f = self.data[self.in_off[b]: self.in_off[b] + self.lens[b]].tobytes()
                events = sorted(k for k, v in CI.trace(f, self.variant)[1].items() if v)
                raise AssertionError(f"{what}: block {b} (len {self.lens[b]}) differs from the oracle; events {events}; fragment {f[:96].hex()}")
        touched = np.nonzero(self.outside & (h_out != FILL))[0]
        assert touched.size == 0, f"{what}: bytes outside every block's area were written, first at {touched[:8]}"
        back = torch.zeros(self.data.size, dtype=torch.uint8, device="cuda")
        dlen, dst = cd.decompress(out, d_coff, out_len, back, d_off, d_lens)
        torch.cuda.synchronize()
        assert int((dst != 0).sum()) == 0 and bool((dlen == d_lens).all()), what
        h_back = back.cpu().numpy()
        for b in np.nonzero(self.lens)[0]:
            i, l = self.in_off[b], self.lens[b]
            assert np.array_equal(h_back[i: i + l], self.data[i: i + l]), f"{what}: block {b} does not decode to its input"
        return h_out


def packed(blocks, variant, in_residue=None, out_residue=None, between=0xEE) -> Batch:
    """One input buffer: the blocks back to back (or each at the input residue mod 16 asked for, `between` in the holes), 64 zero bytes behind the last."""
    parts, off, at = [], [], 0
    for i, b in enumerate(blocks):
        if in_residue is not None:
            pad = (int(in_residue[i]) - at) % 16
            parts.append(np.full(pad, between, dtype=np.uint8))
            at += pad
        off.append(at)
        parts.append(np.frombuffer(bytes(b), dtype=np.uint8))
        at += len(b)
    data = np.concatenate(parts + [np.zeros(64, dtype=np.uint8)])
    return Batch(data, np.array(off, dtype=np.int64), np.array([len(b) for b in blocks], dtype=np.int32), variant, out_residue)


def codec(layout, variant):
    cd = SB.BlockCodec(0, variant)
    layouts.set_compress_layout(cd.ctx, layout)
    return cd


# ---- (a) every layout ----------------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def matrix_batch(variant) -> Batch:
    rng = np.random.default_rng(13000 + variant)
    text = _text()
    return packed(CI.directed(variant) + [CI.make_block(rng, text).tobytes() for _ in range(FUZZ_BLOCKS)], variant)


@pytest.mark.parametrize("layout", layouts.COMPRESS_LAYOUTS)
@pytest.mark.parametrize("variant", VARIANTS)
def test_every_layout_on_directed_and_fuzz_blocks(layout, variant):
    matrix_batch(variant).check(codec(layout, variant), f"{layout} v{variant}")


# ---- (b) placement -------------------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def placed_batch(variant) -> Batch:
    """The directed set sixteen times over: in repetition r fragment i lies at input residue (i + r) mod 16 and writes at output residue (3 i + 5 r) mod 16,
    so every fragment meets every input residue and every output residue."""
    frags = CI.directed(variant)
    blocks, in_res, out_res = [], [], []
    for r in range(16):
        for i, f in enumerate(frags):
            blocks.append(f)
            in_res.append((i + r) % 16)
            out_res.append((3 * i + 5 * r) % 16)
    batch = packed(blocks, variant, np.array(in_res), np.array(out_res))
    assert all(len(set(res[i::len(frags)])) == 16 for res in (batch.in_off % 16, batch.out_off % 16) for i in range(0, len(frags), 37))
    return batch


@pytest.mark.parametrize("layout", PLACED_LAYOUTS)
@pytest.mark.parametrize("variant", VARIANTS)
def test_directed_set_at_every_input_and_output_residue(layout, variant):
    placed_batch(variant).check(codec(layout, variant), f"{layout} v{variant}, placed")


# ---- (c) neighbour independence ------------------------------------------------------------------------------------------------------------------

def continuation(f: bytes, variant: int, count: int = 64) -> bytes:
    """The bytes that would continue the fragment's last match beyond its end (a fragment without a copy: its own start, as an offset-n match would)."""
    offsets = [a for kind, a, _l in CI.trace(f, variant)[0] if kind == "copy"]
    off = offsets[-1] if offsets else len(f)
    ext = bytearray(f)
    for _ in range(count):
        ext.append(ext[-off])
    return bytes(ext[len(f):])


@functools.lru_cache(maxsize=None)
def neighbour_batch(variant) -> Batch:
    """Every directed fragment three times: followed by the continuation of its last match, by 0xFF bytes, and by zeros -- what the 64-byte pad at the end of
    the buffer holds (the batch's last fragment is followed by that pad itself)."""
    frags = [f for f in CI.directed(variant) if f]
    parts, off, lens, at = [], [], [], 0
    for follow in (lambda f: continuation(f, variant), lambda f: b"\xff" * 64, lambda f: b""):
        for f in frags:
            tail = follow(f) or bytes(64)
            off.append(at)
            lens.append(len(f))
            parts += [np.frombuffer(f, dtype=np.uint8), np.frombuffer(tail, dtype=np.uint8)]
            at += len(f) + len(tail)
    return Batch(np.concatenate(parts), np.array(off, dtype=np.int64), np.array(lens, dtype=np.int32), variant)


@pytest.mark.parametrize("layout", PLACED_LAYOUTS)
@pytest.mark.parametrize("variant", VARIANTS)
def test_output_does_not_depend_on_the_bytes_behind_a_fragment(layout, variant):
    batch = neighbour_batch(variant)
    k = len(batch.lens) // 3
    assert np.array_equal(batch.lens[:k], batch.lens[k: 2 * k]) and np.array_equal(batch.lens[:k], batch.lens[2 * k:])
    for b in range(k):                                                  # the oracle itself gives one stream for the three
        streams = {batch.ref[batch.ref_off[j]: batch.ref_off[j] + batch.ref_len[j]].tobytes() for j in (b, b + k, b + 2 * k)}
        assert len(streams) == 1
    batch.check(codec(layout, variant), f"{layout} v{variant}, neighbours")     # ... and every device stream equals the oracle's: the three are identical


# ---- (d) the policy as shipped -------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _pool():
    """make_block blocks back to back: the fragments of the large batches are windows of it (so mostly of one kind, some across two)."""
    rng = np.random.default_rng(4096)
    text = _text()
    return np.concatenate([CI.make_block(rng, text) for _ in range(1024)])


@pytest.mark.parametrize("nb", [131072, 32768])
def test_shipped_policy_on_large_batches_of_ragged_fragments(nb):
    """No lane option set: the launch form comes from the batch size (>= 131 072: exchange probe, input window, staged output, 64 per wavefront; 32 768: staged
    output, two probes, 32 per wavefront).  Lengths: EDGE_LENGTHS up to 4 096 mixed with uniform 0 .. 4 096; the longest is exactly 4 096, so neither the
    small-input launch nor full-size tables are involved.  About 270 MB of input for the larger batch."""
    free, _total = torch.cuda.mem_get_info()
    need = nb * 65536 * 2 + (6 << 30)                                   # twice the table workspace (snp_compress_lanes_workspace: 64 KiB per fragment) + buffers
    if free < need:
        pytest.skip(f"{nb} fragments need about {need >> 30} GiB of device memory, {free >> 30} GiB are free")
    pool = _pool()
    rng = np.random.default_rng(nb)
    edges = np.array([v for v in CI.EDGE_LENGTHS if v <= 4096], dtype=np.int32)
    lens = np.where(rng.integers(0, 3, nb) == 0, rng.choice(edges, nb), rng.integers(0, 4097, nb)).astype(np.int32)
    assert lens.max() == 4096
    start = rng.integers(0, pool.size - 4096, nb)
    off = np.zeros(nb, dtype=np.int64)
    off[1:] = np.cumsum(lens[:-1].astype(np.int64))
    data = np.zeros(int(off[-1] + lens[-1]) + 64, dtype=np.uint8)
    for b in range(nb):
        data[off[b]: off[b] + lens[b]] = pool[start[b]: start[b] + lens[b]]
    cd = SB.BlockCodec(0, O.HASH_CRC32C)
    cd.ctx.set_option(N.OPT_COMPRESS_LAYOUT, N.COMPRESS_LANES)
    cd.ctx.set_option(N.OPT_TABLE_PROBE_TRIES, 1)
    assert _compare_batch(cd, data, off, lens, O.HASH_CRC32C, f"{nb} ragged fragments, shipped policy") == nb
    cd.ctx.close()

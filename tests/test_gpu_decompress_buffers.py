"""snp_decompress_buffers_batch (BlockCodec.decompress_buffers): per block the status, out_len and OK bytes of snp_decompress_batch and of the
oracle, with the large blocks decoded by fragments (d_result proves which path ran) -- a seeded ragged batch, foreign and malformed streams among
good blocks, guard bytes and exact capacities, max_fragments and SNP_OPT_PARALLEL_DECODE_MIN that change nothing but the path, graph capture and
the wrapper's defaults.  Needs an MI355X."""
import numpy as np
import pytest
import torch

import datagen
import oracle as O
from conftest import CORPUS, read_testdata

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from snappier_amd import batch as SB, _native as N

B = 65536
PAR_MIN = 262144
CANARY = 0x5C


def varint(v):
    out = bytearray()
    while v >= 128:
        out.append((v & 0x7F) | 0x80)
        v >>= 7
    out.append(v)
    return bytes(out)


def literal(data: bytes) -> bytes:
    k = len(data) - 1
    if k < 60:
        return bytes([k << 2]) + data
    nb = (k.bit_length() + 7) // 8
    return bytes([(59 + nb) << 2]) + k.to_bytes(nb, "little") + data


def copy2(off: int, ln: int) -> bytes:
    return bytes([2 | ((ln - 1) << 2)]) + off.to_bytes(2, "little")


def corpus_bytes(n: int, start: int = 0) -> bytes:
    files = [read_testdata(name) for name in CORPUS]
    out = bytearray()
    i = start
    while len(out) < n:
        out += files[i % len(files)]
        i += 1
    return bytes(out[:n])


def low_entropy_bytes(n: int, seed: int = 7) -> bytes:
    return b"".join(datagen.low_entropy_block(seed + b, 65536).tobytes() for b in range((n + 65535) // 65536))[:n]


def random_bytes(n: int, seed: int) -> bytes:
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes()


def content(kind: str, n: int, seed: int) -> bytes:
    return corpus_bytes(n, seed) if kind == "corpus" else low_entropy_bytes(n, seed) if kind == "low" else random_bytes(n, seed)


def foreign_streams():
    """The three foreign streams of test_gpu_big_blocks.py: each decodes fine serially, but not fragment by fragment."""
    rng = np.random.default_rng(5)
    head = rng.integers(0, 256, 65536, dtype=np.uint8).tobytes()
    s_a = varint(65536 + 3200 * 64) + literal(head) + b"".join(copy2(60000 + (i % 5000), 64) for i in range(3200))
    lit = rng.integers(0, 256, 65536 + 100, dtype=np.uint8).tobytes()
    s_b = varint(len(lit) + 3200 * 64) + literal(lit) + b"".join(copy2(1 + (i % 90), 64) for i in range(3200))
    lit_c = rng.integers(0, 256, 65536 - 32, dtype=np.uint8).tobytes()
    s_c = varint(len(lit_c) + 4000 * 64) + literal(lit_c) + b"".join(copy2(1000 + i, 64) for i in range(4000))
    return [s_a, s_b, s_c]


def malformed_streams():
    """The malformed cases of test_gpu_big_blocks.py (each large enough to be a candidate, or not a candidate at all)."""
    data = corpus_bytes(600000)
    comp = O.compress(data, O.HASH_CRC32C)
    h = len(varint(len(data)))
    return {
        "truncated": comp[: len(comp) - 1000],                         # candidate: fragments fail
        "declared too long": varint(len(data) + 5) + comp[h:],          # candidate: fragments fail
        "declared too short": varint(len(data) - 5) + comp[h:],         # candidate: the stream does not end at the declared length
        "garbage in the middle": comp[:40000] + copy2(0, 8) + comp[40000:],   # candidate: a copy with offset 0
        "bad varint": b"\xff\xff\xff\xff\xff\x01" + comp[3:],           # no candidate (the preamble is not clean)
    }


def preamble(block: bytes):
    """-> (clean, declared, hb): the varint as snp_try_decompress reads it."""
    expected = hb = shift = 0
    for i in range(min(5, len(block))):
        val = block[i] & 0x7F
        if val & ~(0xFFFFFFFF >> shift) & 0xFFFFFFFF:
            break
        expected |= val << shift
        shift += 7
        hb = i + 1
        if block[i] < 128:
            return True, expected, hb
    return False, expected, hb


def declared_of(stream: bytes) -> int:
    v = shift = 0
    for ch in stream[:5]:
        v |= (ch & 0x7F) << shift
        shift += 7
        if ch < 128:
            break
    return v


class Batch:
    """Blocks packed at odd offsets into one device tensor; output ranges separated by canary gaps."""

    def __init__(self, streams, caps, gap=19):
        self.streams = streams
        self.caps = np.asarray(caps, dtype=np.int64)
        in_off, pos = [], 3
        for s in streams:
            in_off.append(pos)
            pos += len(s) + 5
        self.in_off = np.asarray(in_off, dtype=np.int64)
        buf = np.zeros(pos + 16, dtype=np.uint8)
        for o, s in zip(in_off, streams):
            buf[o:o + len(s)] = np.frombuffer(s, dtype=np.uint8)
        self.comp = torch.from_numpy(buf).cuda()
        self.in_len = np.array([len(s) for s in streams], dtype=np.int64)
        self.out_off = np.concatenate([[gap], np.cumsum(self.caps + gap)[:-1] + gap]).astype(np.int64) if len(streams) else np.zeros(0, np.int64)
        self.out_size = int(self.out_off[-1] + self.caps[-1] + gap) if len(streams) else 16
        self.d = dict(in_off=dev(self.in_off), in_len=dev(self.in_len.astype(np.uint32).view(np.int32)), out_off=dev(self.out_off),
                      out_cap=dev(self.caps.astype(np.uint32).view(np.int32)))

    def run(self, cd, buffers: bool, max_fragments=None, work=None):
        out = torch.full((self.out_size,), CANARY, dtype=torch.uint8, device="cuda")
        if buffers:
            ol, st, res = cd.decompress_buffers(self.comp, self.d["in_off"], self.d["in_len"], out, self.d["out_off"], self.d["out_cap"],
                                                max_fragments=max_fragments, work=work)
        else:
            ol, st = cd.decompress(self.comp, self.d["in_off"], self.d["in_len"], out, self.d["out_off"], self.d["out_cap"])
            res = None
        torch.cuda.synchronize()
        return out.cpu().numpy(), ol.cpu().numpy(), st.cpu().numpy(), None if res is None else res.cpu().numpy()

    def candidates(self, par_min=PAR_MIN):
        """The blocks the call splits: the candidate rule, then the makespan rule (declared >= 2 * sum / wave slots)."""
        cand = []
        for b, s in enumerate(self.streams):
            clean, d, h = preamble(s)
            if clean and par_min and par_min <= d <= self.caps[b] and h < len(s) <= 38 + d + d // 6:
                cand.append(b)
        total = sum(declared_of(self.streams[b]) for b in cand)
        slots = torch.cuda.get_device_properties(0).multi_processor_count * 32
        return [b for b in cand if declared_of(self.streams[b]) * slots >= 2 * total]


def dev(a: np.ndarray):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def nfrags(batch: Batch, blocks) -> int:
    return sum((declared_of(batch.streams[b]) + B - 1) // B for b in blocks)


def check(tag, batch: Batch, got, ref, oracle=True):
    out, ol, st, _ = got
    r_out, r_ol, r_st, _ = ref
    assert st.tolist() == r_st.tolist(), f"{tag}: statuses differ from snp_decompress_batch"
    assert ol.tolist() == r_ol.tolist(), f"{tag}: out_len differs from snp_decompress_batch"
    mask = np.ones(out.size, dtype=bool)
    for b, s in enumerate(batch.streams):
        o, c, n = int(batch.out_off[b]), int(batch.caps[b]), int(ol[b])
        mask[o:o + c] = False
        if st[b] == O.OK:
            assert out[o:o + n].tobytes() == r_out[o:o + int(r_ol[b])].tobytes(), f"{tag}: block {b} bytes differ from snp_decompress_batch"
            if oracle:
                assert out[o:o + n].tobytes() == O.decompress(s), f"{tag}: block {b} differs from the oracle"
        elif oracle:
            assert O.decompress_status(s) == st[b] or c < declared_of(s), f"{tag}: block {b} status {st[b]}"
    assert (out[mask] == CANARY).all(), f"{tag}: bytes outside the output ranges were written"


def ragged_batch(seed):
    rng = np.random.default_rng(seed)
    sizes = [0, 1, 14, 65536, 65537, 262143, 262144, 262145, 1000000, 4 << 20, 40 << 20]
    sizes += [int(np.exp(rng.uniform(0, np.log(8 << 20)))) for _ in range(24)]
    rng.shuffle(sizes)
    streams = []
    for i, n in enumerate(sizes):
        kind = ("corpus", "low", "random")[i % 3]
        streams.append(O.compress(content(kind, n, seed + i), O.HASH_CRC32C if i % 2 else O.HASH_MUL))
    caps = [declared_of(s) + int(rng.integers(0, 100)) for s in streams]
    return Batch(streams, caps)


@pytest.mark.parametrize("seed", [1, 2])
def test_seeded_ragged_batch_equals_decompress_batch_and_the_oracle(seed):
    batch = ragged_batch(seed)
    cd = SB.BlockCodec(0, O.HASH_CRC32C)
    ref = batch.run(cd, False)
    cand = batch.candidates()
    got = batch.run(cd, True, max_fragments=nfrags(batch, cand))
    check("ragged", batch, got, ref)
    res = got[3]
    assert res[0] == nfrags(batch, cand) and res[1] == len(cand) and res[2] == 0, res


def test_blocks_made_by_compress_buffers():
    """Blocks of any length made on the device by snp_compress_buffers_batch, decoded back."""
    cd = SB.BlockCodec(0, O.HASH_CRC32C)
    lens = np.array([3 << 20, 70000, 0, 9 << 20, 262144, 5], dtype=np.int64)
    raw = b"".join(corpus_bytes(int(n), i) for i, n in enumerate(lens))
    data = dev(np.frombuffer(raw, dtype=np.uint8).copy())
    in_off = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
    out, out_off, out_len, status, _ = cd.compress_buffers(data, dev(in_off), dev(lens.astype(np.int32)))
    torch.cuda.synchronize()
    h_out, h_oo, h_ol = out.cpu().numpy(), out_off.cpu().numpy(), out_len.cpu().numpy()
    streams = [h_out[int(h_oo[b]):int(h_oo[b]) + int(h_ol[b])].tobytes() for b in range(len(lens))]
    batch = Batch(streams, lens)
    got = batch.run(cd, True)
    check("compress_buffers", batch, got, batch.run(cd, False))
    assert got[2].tolist() == [O.OK] * len(lens) and got[3][1] == 3


def test_foreign_and_malformed_streams_among_good_blocks():
    good = [O.compress(corpus_bytes(n, n), O.HASH_CRC32C) for n in (300000, 1 << 20, 77777)]
    foreign = foreign_streams()
    bad = malformed_streams()
    rnd = O.compress(random_bytes(4 << 20, 9), O.HASH_CRC32C)        # 4 MiB of random bytes: the tag index takes the look-back pass
    streams = [good[0], foreign[0], bad["truncated"], good[1], foreign[1], bad["declared too long"], bad["declared too short"], rnd,
               foreign[2], bad["garbage in the middle"], bad["bad varint"], good[2]]
    caps = [declared_of(s) + 7 if preamble(s)[0] else 1 << 20 for s in streams]   # (the bad varint declares ~2^35 bytes)
    batch = Batch(streams, caps)
    cd = SB.BlockCodec(0, O.HASH_CRC32C)
    ref = batch.run(cd, False)
    cand = batch.candidates()
    got = batch.run(cd, True, max_fragments=nfrags(batch, cand))
    check("foreign", batch, got, ref)
    for b, s in enumerate(streams):
        assert got[2][b] == O.decompress_status(s), b
    fell_back = {1, 2, 4, 5, 6, 8, 9}                                  # the foreign streams and the malformed candidates
    assert fell_back <= set(cand)
    res = got[3]
    assert res[1] == len(cand) - len(fell_back) and res[2] == len(fell_back), res
    assert res[3] >= 1, res


def test_guard_bytes_and_exact_capacities():
    streams = [O.compress(corpus_bytes(n, 3), O.HASH_CRC32C) for n in (1 << 20, 1 << 20, 600001, 600001, 262144)]
    d = [declared_of(s) for s in streams]
    caps = [d[0], d[1] - 1, d[2], d[3] - 1, d[4]]                    # exactly the declared length, and one byte less
    batch = Batch(streams, caps, gap=33)
    cd = SB.BlockCodec(0, O.HASH_CRC32C)
    ref = batch.run(cd, False)
    got = batch.run(cd, True, max_fragments=64)
    check("caps", batch, got, ref)
    assert got[2].tolist() == [O.OK, O.ERR_OUTPUT_TOO_SMALL, O.OK, O.ERR_OUTPUT_TOO_SMALL, O.OK]
    assert got[3][1] == 3 and got[3][2] == 0


def test_max_fragments_changes_only_the_path():
    batch = ragged_batch(3)
    cd = SB.BlockCodec(0, O.HASH_CRC32C)
    ref = batch.run(cd, False)
    cand = batch.candidates()
    need = nfrags(batch, cand)
    split = []
    for mf in (0, need // 3, need - 1, need, need * 4 + 1000):
        got = batch.run(cd, True, max_fragments=mf)
        check(f"max_fragments={mf}", batch, got, ref, oracle=False)
        assert got[3][0] == need and got[3][2] == 0
        split.append(int(got[3][1]))
    # admitted in buffer order while the fragments fit
    def fit(mf):
        used, k = 0, 0
        for b in cand:
            used += (declared_of(batch.streams[b]) + B - 1) // B
            if used > mf:
                break
            k += 1
        return k
    assert split == [fit(mf) for mf in (0, need // 3, need - 1, need, need * 4 + 1000)]
    assert split[0] == 0 and split[-1] == split[-2] == len(cand)


@pytest.mark.parametrize("par_min", [0, 1, None])
def test_parallel_decode_min_changes_only_the_path(par_min):
    batch = ragged_batch(4)
    cd = SB.BlockCodec(0, O.HASH_CRC32C)
    if par_min is not None:
        cd.ctx.set_option(N.OPT_PARALLEL_DECODE_MIN, par_min)
    ref = batch.run(cd, False)
    cand = batch.candidates(PAR_MIN if par_min is None else par_min)
    got = batch.run(cd, True, max_fragments=nfrags(batch, cand) + 5)
    check(f"par_min={par_min}", batch, got, ref, oracle=False)
    assert got[3][1] == len(cand)


def test_graph_capture_replays_on_new_inputs():
    sizes = [300000, 2 << 20, 1000, 5 << 20, 65536]
    mk = lambda seed: [O.compress(corpus_bytes(n, seed + i), O.HASH_CRC32C) for i, n in enumerate(sizes)]
    first, second = mk(0), mk(7)
    n_max = [max(len(a), len(b)) for a, b in zip(first, second)]
    pad = lambda ss: [s + bytes(m - len(s)) for s, m in zip(ss, n_max)]   # same offsets; the zero tail is past in_len
    caps = [declared_of(s) for s in first]
    assert caps == [declared_of(s) for s in second]
    batch = Batch(pad(first), caps)
    lens = [np.array([len(s) for s in ss], dtype=np.int64) for ss in (first, second)]
    in_len = dev(lens[0].astype(np.int32))
    cd = SB.BlockCodec(0, O.HASH_CRC32C)
    mf = nfrags(batch, [0, 1, 3])                                       # (the blocks of >= 256 KiB)
    work = torch.empty(N.buffers_decompress_lib().snp_decompress_buffers_workspace(len(sizes), mf), dtype=torch.uint8, device="cuda")
    out = torch.zeros(batch.out_size, dtype=torch.uint8, device="cuda")

    def call():
        return cd.decompress_buffers(batch.comp, batch.d["in_off"], in_len, out, batch.d["out_off"], batch.d["out_cap"], max_fragments=mf, work=work)

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        call()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        out_len, status, result = call()
    for ss, ln in ((second, lens[1]), (first, lens[0]), (second, lens[1])):
        padded = pad(ss)
        buf = batch.comp.cpu().numpy()
        for o, blk in zip(batch.in_off, padded):
            buf[o:o + len(blk)] = np.frombuffer(blk, dtype=np.uint8)
        batch.comp.copy_(torch.from_numpy(buf))
        in_len.copy_(dev(ln.astype(np.int32)))
        out.zero_()
        g.replay()
        torch.cuda.synchronize()
        h, ol, st = out.cpu().numpy(), out_len.cpu().numpy(), status.cpu().numpy()
        for b, blk in enumerate(ss):
            o = int(batch.out_off[b])
            assert st[b] == O.OK and h[o:o + int(ol[b])].tobytes() == O.decompress(blk), b
        assert result.cpu().tolist()[:3] == [mf, 3, 0]


def test_wrapper_defaults():
    streams = [O.compress(corpus_bytes(n, 1), O.HASH_CRC32C) for n in (0, 5, 65536, 1 << 20, 3 << 20)]
    batch = Batch(streams, [declared_of(s) for s in streams])
    cd = SB.BlockCodec(0, O.HASH_CRC32C)
    got = batch.run(cd, True)
    check("defaults", batch, got, batch.run(cd, False))
    out_len, status, result = cd.decompress_buffers(batch.comp, batch.d["in_off"], batch.d["in_len"],
                                                    torch.empty(batch.out_size, dtype=torch.uint8, device="cuda"), batch.d["out_off"], batch.d["out_cap"])
    torch.cuda.synchronize()
    assert out_len.dtype == torch.int32 and status.dtype == torch.int32 and result.dtype == torch.int64 and result.numel() == 4
    assert got[3].tolist()[:3] == [nfrags(batch, [3, 4]), 2, 0]
    # no buffers: OK, and d_result is still written
    e = torch.zeros(0, dtype=torch.int64, device="cuda")
    e_len, e_st, e_res = cd.decompress_buffers(batch.comp, e, e.to(torch.int32), torch.empty(16, dtype=torch.uint8, device="cuda"), e, e.to(torch.int32))
    torch.cuda.synchronize()
    assert e_len.numel() == 0 and e_res.cpu().tolist() == [0, 0, 0, 0]
    with pytest.raises(ValueError):
        cd.decompress_buffers(batch.comp, batch.d["in_off"], batch.d["in_len"], torch.empty(batch.out_size, dtype=torch.uint8, device="cuda"),
                              batch.d["out_off"], batch.d["out_cap"], max_fragments=100, work=torch.empty(16, dtype=torch.uint8, device="cuda"))

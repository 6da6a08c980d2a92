"""snp_compress_buffers_batch (BlockCodec.compress_buffers): device buffers of ANY length, each one Snappy block, against the oracle byte for byte --
edge lengths, a seeded ragged batch of mixed content at aliased offsets, capacities, a short / loose max_fragments, every compressor layout,
round trips, graph capture and the wrapper's defaults.  Needs an MI355X."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest
import torch

import layouts
import oracle as O
from conftest import CORPUS, read_testdata

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    import snappier_amd as S
    from snappier_amd import batch as SB, datagen as SD, _native as N

B = 65536
VARIANTS = [O.HASH_CRC32C, O.HASH_MUL]
SENTINEL = 0xA5
_pool = ThreadPoolExecutor(16)            # the oracle on at most 16 threads (ctypes releases the GIL)


def oracle_all(chunks, variant):
    return list(_pool.map(lambda c: O.compress(c, variant), chunks))


def cap_of(n):
    return 32 + n + n // 6 + 1 + 5


def nfrag(lens):
    return sum((int(n) + B - 1) // B for n in lens)


def dev(a: np.ndarray):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def run(cd, data: torch.Tensor, in_off, lens, max_fragments=None, gap=0, out_cap=None, sentinel=True):
    """Buffers at caller offsets with `gap` sentinel bytes between them: -> (out (host), out_off, out_len, status, result) as numpy."""
    lens = np.asarray(lens, dtype=np.int64)
    cap = np.array([cap_of(int(n)) for n in lens], dtype=np.int64) if out_cap is None else np.asarray(out_cap, dtype=np.int64)
    out_off = np.concatenate([[gap], np.cumsum(cap + gap)[:-1] + gap]).astype(np.int64) if len(lens) else np.zeros(0, np.int64)
    total = int(out_off[-1] + cap[-1] + gap) if len(lens) else 1
    out = torch.full((total,), SENTINEL if sentinel else 0, dtype=torch.uint8, device="cuda")
    mf = nfrag(lens) if max_fragments is None else max_fragments
    res = cd.compress_buffers(data, dev(np.asarray(in_off, dtype=np.int64)), dev(lens.astype(np.uint32).view(np.int32)), out=out,
                              out_off=dev(out_off), out_cap=dev(cap), max_fragments=mf)
    torch.cuda.synchronize()
    _, _, out_len, status, result = res
    return out.cpu().numpy(), out_off, out_len.cpu().numpy(), status.cpu().numpy(), result.cpu().numpy()


def check_against_oracle(tag, h_data, in_off, lens, out, out_off, out_len, status, variant, gap_check=True, cap=None):
    refs = oracle_all([h_data[o:o + n].tobytes() for o, n in zip(in_off, lens)], variant)
    for b, ref in enumerate(refs):
        assert status[b] == O.OK, f"{tag}: buffer {b} ({lens[b]} B) status {status[b]}"
        got = out[out_off[b]:out_off[b] + out_len[b]].tobytes()
        assert out_len[b] == len(ref) and got == ref, f"{tag}: buffer {b} ({lens[b]} B) differs from the oracle"
    if gap_check:
        mask = np.ones(out.size, dtype=bool)
        for b in range(len(lens)):
            mask[out_off[b]:out_off[b] + out_len[b]] = False
        assert (out[mask] == SENTINEL).all(), f"{tag}: bytes outside the blocks were written"
    return refs


EDGE = [0, 1, 15, 16, 65535, 65536, 65537, 131072, 131073, 3 * 65536 + 7, 1 << 20, (16 << 20) + 3]


@pytest.mark.parametrize("variant", VARIANTS)
def test_edge_lengths_equal_the_oracle(variant):
    html = read_testdata("html")
    cd = SB.BlockCodec(0, variant)
    data = SD.html_like_blocks(html, 3, 260, "cuda")
    h = data.cpu().numpy()
    in_off = [(977 * i) % 4096 + (i & 1) for i in range(len(EDGE))]
    out, out_off, out_len, status, result = run(cd, data, in_off, EDGE, gap=5)
    check_against_oracle("edge", h, in_off, EDGE, out, out_off, out_len, status, variant)
    assert out[out_off[0]:out_off[0] + out_len[0]].tobytes() == b"\x00"
    assert result[0] == nfrag(EDGE) and result[1] == out_len.sum()


def test_a_buffer_with_a_five_byte_varint():
    n = (1 << 28) + 1
    free, _ = torch.cuda.mem_get_info()
    if free < 4 * n + nfrag([n]) * 80000 + (2 << 30):
        pytest.skip(f"needs ~{(4 * n + nfrag([n]) * 80000) >> 30} GiB of free device memory, {free >> 30} GiB free")
    html = read_testdata("html")
    data = SD.html_like_blocks(html, 0, nfrag([n]), "cuda")
    h = data.cpu().numpy()[:n].tobytes()
    for variant in VARIANTS:
        cd = SB.BlockCodec(0, variant)
        cd.ctx.set_option(N.OPT_TABLE_PROBE_TRIES, 1)
        out, out_off, out_len, status, _ = run(cd, data, [0], [n], sentinel=False)
        assert status[0] == O.OK
        got = out[:out_len[0]].tobytes()
        assert got[:5] == O.varint_write(n) and len(O.varint_write(n)) == 5
        assert got == O.compress(h, variant)


def mixed_pool(seed: int):
    """html-like, random, zeros and the corpus files, one device tensor: -> (tensor, [(start, length) of each kind])."""
    html = read_testdata("html")
    g = torch.Generator(device="cuda").manual_seed(seed)
    parts = [SD.html_like_blocks(html, 40, 96, "cuda"),
             torch.randint(0, 256, (16 << 20,), dtype=torch.uint8, device="cuda", generator=g),
             torch.zeros(8 << 20, dtype=torch.uint8, device="cuda"),
             torch.from_numpy(np.frombuffer(b"".join(read_testdata(n) for n in CORPUS) * 2, dtype=np.uint8).copy()).cuda()]
    spans, o = [], 0
    for p in parts:
        spans.append((o, p.numel()))
        o += p.numel()
    return torch.cat(parts), spans


def ragged_batch(rng, spans, nb, max_len):
    lens = np.minimum(np.floor(np.exp(rng.uniform(0, np.log(max_len + 1), nb))) - 1, max_len).astype(np.int64)
    lens[rng.integers(0, nb, nb // 50)] = 0
    in_off = []
    for n in lens:
        s, ln = spans[rng.integers(0, len(spans))]
        room = ln - n
        if room < 2:
            s, ln = spans[0]
            room = ln - n
        o = int(rng.integers(0, room))
        in_off.append(s + (o | 1 if rng.integers(0, 2) else o & ~1))        # odd and even input offsets; buffers overlap each other freely
    return np.array(in_off, dtype=np.int64), lens


@pytest.mark.parametrize("variant", VARIANTS)
def test_seeded_ragged_batch_of_mixed_content(variant):
    rng = np.random.default_rng(20261016 + variant)
    data, spans = mixed_pool(7 + variant)
    h = data.cpu().numpy()
    in_off, lens = ragged_batch(rng, spans, 2000, 4 << 20)
    cd = SB.BlockCodec(0, variant)
    out, out_off, out_len, status, result = run(cd, data, in_off, lens, gap=37)
    check_against_oracle("ragged", h, in_off, lens, out, out_off, out_len, status, variant)
    assert result[0] == nfrag(lens) and result[1] == out_len.sum()
    # buffers of <= 64 KiB: the same bytes as snp_compress_batch
    small = np.nonzero(lens <= B)[0]
    bo, bof, blen, bst = cd.compress(data, dev(in_off[small]), dev(lens[small].astype(np.int32)))
    torch.cuda.synchronize()
    bo, bof, blen = bo.cpu().numpy(), bof.cpu().numpy(), blen.cpu().numpy()
    assert (bst.cpu().numpy() == 0).all()
    for i, b in enumerate(small):
        assert bo[bof[i]:bof[i] + blen[i]].tobytes() == out[out_off[b]:out_off[b] + out_len[b]].tobytes(), f"buffer {b}"


def test_capacity_exact_fits_one_byte_less_fails_alone():
    html = read_testdata("html")
    data = SD.html_like_blocks(html, 9, 8, "cuda")
    h = data.cpu().numpy()
    lens = [300000, 0, 70000, 5, 65536]
    in_off = [1, 3, 200001, 17, 40000]
    cd = SB.BlockCodec(0, O.HASH_CRC32C)
    refs = [O.compress(h[o:o + n].tobytes(), O.HASH_CRC32C) for o, n in zip(in_off, lens)]
    exact = [len(r) for r in refs]
    out, out_off, out_len, status, result = run(cd, data, in_off, lens, out_cap=exact, gap=11)
    check_against_oracle("exact cap", h, in_off, lens, out, out_off, out_len, status, O.HASH_CRC32C)
    for b in (0, 1, 2):
        cap = list(exact)
        cap[b] -= 1
        out, out_off, out_len, status, result = run(cd, data, in_off, lens, out_cap=cap, gap=11)
        assert status[b] == O.ERR_OUTPUT_TOO_SMALL and out_len[b] == 0
        assert (out[out_off[b]:out_off[b] + exact[b]] == SENTINEL).all(), "a buffer that is not OK was written"
        for k in range(len(lens)):
            if k != b:
                assert status[k] == O.OK and out[out_off[k]:out_off[k] + out_len[k]].tobytes() == refs[k]
        assert result[0] == nfrag(lens) and result[1] == sum(exact) - exact[b]


def test_max_fragments_short_and_loose():
    html = read_testdata("html")
    data = SD.html_like_blocks(html, 21, 40, "cuda")
    h = data.cpu().numpy()
    lens = [70000, 10, 200000, 0, 65536, 131073, 7]        # fragments 2, 1, 4, 0, 1, 3, 1 -> 12
    in_off = [5, 99, 1000, 0, 300000, 600001, 42]
    need = nfrag(lens)
    cd = SB.BlockCodec(0, O.HASH_MUL)
    ref = run(cd, data, in_off, lens, max_fragments=need, gap=3)
    check_against_oracle("exact", h, in_off, lens, *ref[:4], O.HASH_MUL)
    loose = run(cd, data, in_off, lens, max_fragments=need + 1000, gap=3)
    assert np.array_equal(loose[0], ref[0]) and np.array_equal(loose[2], ref[2]) and (loose[3] == 0).all() and loose[4][0] == need
    firsts = np.concatenate([[0], np.cumsum([(n + B - 1) // B for n in lens])])
    for short in (0, 1, 6, 7, 10, need - 1):
        out, out_off, out_len, status, result = run(cd, data, in_off, lens, max_fragments=short, gap=3)
        assert result[0] == need
        for b in range(len(lens)):
            if firsts[b + 1] <= short:
                assert status[b] == O.OK and out[out_off[b]:out_off[b] + out_len[b]].tobytes() == ref[0][out_off[b]:out_off[b] + ref[2][b]].tobytes()
            else:
                assert status[b] == O.ERR_OUTPUT_TOO_SMALL and out_len[b] == 0
                assert (out[out_off[b]:out_off[b] + cap_of(lens[b])] == SENTINEL).all()
        assert result[1] == out_len.sum()


@pytest.mark.parametrize("layout", ["auto", "win", "wind", "lanes", "lanes-exact"])
def test_every_compressor_layout_with_padding_slots(layout):
    """The compressor runs over max_fragments slots, the empty padding slots included: every layout must write nothing for them."""
    rng = np.random.default_rng(5)
    data, spans = mixed_pool(3)
    h = data.cpu().numpy()
    in_off, lens = ragged_batch(rng, spans, 60, 600000)
    for variant in VARIANTS:
        cd = SB.BlockCodec(0, variant)
        cd.ctx.set_option(N.OPT_TABLE_PROBE_TRIES, 1)
        layouts.set_compress_layout(cd.ctx, layout)
        for mf in (nfrag(lens), nfrag(lens) + 517):
            out, out_off, out_len, status, result = run(cd, data, in_off, lens, max_fragments=mf, gap=9)
            check_against_oracle(f"{layout} mf {mf}", h, in_off, lens, out, out_off, out_len, status, variant)


def test_round_trip_through_the_decoders():
    html = read_testdata("html")
    lens = [0, 1, 100, 65536, 65537, 1 << 20, (16 << 20) + 3, 333333]
    data = SD.html_like_blocks(html, 77, 300, "cuda")
    in_off = [0, 1, 2, 3, 70001, 200000, 1000, 5000000]
    cd = SB.BlockCodec(0, O.HASH_CRC32C)
    out, out_off, out_len, status, _ = cd.compress_buffers(data, dev(np.array(in_off, np.int64)), dev(np.array(lens, np.int32)))
    assert int((status != 0).sum()) == 0
    dcap = torch.tensor(lens, dtype=torch.int32, device="cuda")
    doff = torch.cumsum(dcap.to(torch.int64), 0) - dcap.to(torch.int64)
    back = torch.zeros(int(sum(lens)), dtype=torch.uint8, device="cuda")
    dlen, dst = cd.decompress(out, out_off, out_len.to(torch.int32), back, doff, dcap)
    torch.cuda.synchronize()
    assert int((dst != 0).sum()) == 0 and dlen.cpu().tolist() == lens
    for b, (o, n) in enumerate(zip(in_off, lens)):
        assert torch.equal(back[int(doff[b]):int(doff[b]) + n], data[o:o + n]), f"buffer {b}"
    big = 6
    blk = out[int(out_off[big]):int(out_off[big]) + int(out_len[big])].cpu().numpy().tobytes()
    assert S.Snappy.DecompressToArray(blk) == data[in_off[big]:in_off[big] + lens[big]].cpu().numpy().tobytes()


@pytest.mark.parametrize("nbuf,maxlen", [(64, 300000), (3000, 80000)])
def test_graph_capture_replays_with_the_oracles_bytes(nbuf, maxlen):
    variant = O.HASH_CRC32C
    rng = np.random.default_rng(nbuf)
    data, spans = mixed_pool(11)
    in_off, lens = ragged_batch(rng, spans[:1], nbuf, maxlen)          # html-like region only: its contents are swapped between replays
    html = read_testdata("html")
    other = SD.html_like_blocks(html, 500, 96, "cuda")
    cd = SB.BlockCodec(0, variant)
    cd.ctx.set_option(N.OPT_TABLE_PROBE_TRIES, 1)
    mf = nfrag(lens)
    cap = np.array([cap_of(int(n)) for n in lens], dtype=np.int64)
    d_off, d_len, d_cap = dev(in_off), dev(lens.astype(np.int32)), dev(cap)
    d_oo = dev(np.concatenate([[0], np.cumsum(cap)[:-1]]).astype(np.int64))
    out = torch.zeros(int(cap.sum()), dtype=torch.uint8, device="cuda")
    work = torch.empty(N.buffers_lib().snp_compress_buffers_workspace(nbuf, mf), dtype=torch.uint8, device="cuda")
    src = data.clone()

    def call():
        return cd.compress_buffers(src, d_off, d_len, out=out, out_off=d_oo, out_cap=d_cap, max_fragments=mf, work=work)

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        call()                                                          # the call before the capture: workspaces exist from here on
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        _, _, out_len, status, result = call()
    html_len = spans[0][1]
    for contents in (other, data[:html_len], other):
        src[:html_len].copy_(contents)
        out.zero_()
        g.replay()
        torch.cuda.synchronize()
        h = src.cpu().numpy()
        ol, st, oo = out_len.cpu().numpy(), status.cpu().numpy(), d_oo.cpu().numpy()
        check_against_oracle("graph", h, in_off, lens, out.cpu().numpy(), oo, ol, st, variant, gap_check=False)
        assert result.cpu().tolist() == [mf, int(ol.sum())]


def test_wrapper_defaults():
    html = read_testdata("html")
    data = SD.html_like_blocks(html, 1, 20, "cuda")
    lens = np.array([0, 5, 65536, 65537, 1000000], dtype=np.int64)
    in_off = np.array([0, 1, 2, 3, 4], dtype=np.int64)
    cd = SB.BlockCodec(0, O.HASH_CRC32C)
    out, out_off, out_len, status, result = cd.compress_buffers(data, dev(in_off), dev(lens.astype(np.int32)))
    torch.cuda.synchronize()
    cap = np.array([N.lib().snp_max_compressed_length(int(n)) for n in lens], dtype=np.int64)
    assert cap.tolist() == [cap_of(int(n)) for n in lens]
    assert out_off.dtype == torch.int64 and out_off.cpu().tolist() == (np.cumsum(cap) - cap).tolist()
    assert out.numel() == int(cap.sum())
    assert out_len.dtype == torch.int64 and status.dtype == torch.int32 and result.dtype == torch.int64
    assert result.cpu().tolist() == [nfrag(lens), int(out_len.sum())]
    h = data.cpu().numpy()
    check_against_oracle("defaults", h, in_off, lens, out.cpu().numpy(), out_off.cpu().numpy(), out_len.cpu().numpy(), status.cpu().numpy(),
                         O.HASH_CRC32C, gap_check=False)
    # no buffers: OK, and d_result is still written
    e_out, _, e_len, e_st, e_res = cd.compress_buffers(data, dev(in_off[:0]), dev(lens[:0].astype(np.int32)))
    torch.cuda.synchronize()
    assert e_len.numel() == 0 and e_res.cpu().tolist() == [0, 0]
    # a work tensor that is too small is refused before anything is launched
    with pytest.raises(ValueError):
        cd.compress_buffers(data, dev(in_off), dev(lens.astype(np.int32)), max_fragments=nfrag(lens), work=torch.empty(16, dtype=torch.uint8, device="cuda"))

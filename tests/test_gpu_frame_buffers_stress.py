"""snp_frame_encode_buffers_batch / snp_frame_decode_buffers_batch at scale, on corrupt streams and under every option: streams of more than 64
spans behind streams whose first span slot is no multiple of 64 (k_fd_resolve's register batches), offsets and lengths past 2^32, a seeded
differential fuzz of corrupt streams under the max_chunks / max_spans admission prefix, every compressor and decoder layout, the raw-versus-
compressed edge of a chunk, and graph replays whose outcomes change.  References: the oracle for bytes, the single-stream device calls
(snp_frame_encode_device / snp_frame_decode_device) on each stream alone, and frame_buffers_model.py for statuses and d_result.  Needs an MI355X."""
import functools

import numpy as np
import pytest
import torch

import frame_buffers_model as M
import layouts
import oracle as O
from conftest import read_testdata
from frame_buffers_helpers import B, CANARY, check_decode, decode, dev, encode, frame_cap, nchunks, outside_ranges, pack, pool_bytes, ragged, \
    single_decode
from test_gpu_frame_buffers import hand_streams

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from snappier_amd import batch as SB, _native as N

SPAN = M.SPAN
G32 = 1 << 32


def spans_of(n: int) -> int:
    return (n + SPAN - 1) // SPAN


def to_dev(b: bytes):
    return torch.from_numpy(np.frombuffer(b, dtype=np.uint8).copy()).cuda()


@functools.lru_cache(maxsize=None)
def raw_chunks():
    """Raw chunk bodies of random bytes (their compressed form is longer) and compressed chunks of html, for the long streams."""
    rng = np.random.default_rng(64)
    rnd = rng.integers(0, 256, 2 * B, dtype=np.uint8).tobytes()
    html = read_testdata("html") * 4
    comp = [M.data_chunk(html[o:o + B]) for o in (0, 7919, 31337)]
    return rnd, M.data_chunk(rnd[:B], compressed=False), comp


class Long:
    """A framed stream built to put chunk headers at chosen stream offsets: full raw chunks (every fifth one a compressed html chunk), then one
    or two raw chunks that end exactly where the next header must start."""

    def __init__(self):
        self.parts, self.n, self.i = [M.STREAM_ID], 10, 0

    def add(self, c: bytes):
        self.parts.append(c)
        self.n += len(c)
        return self

    def fill_to(self, target: int):
        rnd, full, comp = raw_chunks()
        while target - self.n >= 2 * B + 16:
            self.add(comp[self.i % 3] if self.i % 5 == 4 else full)
            self.i += 1
        g = target - self.n - 8
        assert g >= 0
        if g > B:
            self.add(M.data_chunk(rnd[B:B + g // 2 - 8], compressed=False))
            g -= g // 2
        return self.add(M.data_chunk(rnd[:g], compressed=False))

    def bytes(self) -> bytes:
        return b"".join(self.parts)


def long_streams():
    """-> [(name, stream)]: headers at 64 MiB + d and 128 MiB + d (d = -3 .. 2), a skippable chunk from span 62 into span 67 (its exit inside
    span 67's candidate window, and past it), a stream that ends exactly on a span boundary."""
    html = read_testdata("html")
    out = []
    for d in (-3, -2, -1, 0, 1, 2):
        s = Long().fill_to((64 << 20) + d).fill_to((128 << 20) + d)
        s.add(M.data_chunk(html[:5000])).add(M.data_chunk(html[100:70000 - 4500], compressed=False))
        out.append((f"at_64_128_{d:+d}", s.bytes()))
    rng = np.random.default_rng(62)
    for name, land, body in (("skip_62_67", (67 << 20) + 1001, None), ("skip_62_67_far", (67 << 20) + 200003, "random")):
        s = Long().fill_to((62 << 20) + 333)
        pad = land - s.n - 4
        s.add(M.chunk(0x9A, bytes(pad) if body is None else rng.integers(0, 256, pad, dtype=np.uint8).tobytes()))
        s.fill_to(70 << 20).add(M.data_chunk(html[:777]))
        out.append((name, s.bytes()))
    out.append(("ends_on_span_66", Long().fill_to(66 << 20).bytes()))
    return out


def short_stream(rng, spans: int) -> bytes:
    return Long().fill_to(int(rng.integers((spans - 1) * SPAN + 1000, spans * SPAN - 1000))).bytes()


# ---- A: past 64 spans ------------------------------------------------------------------------------------------------------------------------
def test_streams_of_more_than_64_spans_behind_unaligned_first_slots():
    longs = long_streams()
    rng = np.random.default_rng(65)
    streams, names = [], []
    for name, s in longs:
        streams.append(short_stream(rng, int(rng.integers(1, 4))))
        names.append("short")
        if sum(spans_of(len(x)) for x in streams) % 64 == 0:
            streams.append(short_stream(rng, 1))
            names.append("short")
        streams.append(s)
        names.append(name)
    sfirst = np.concatenate([[0], np.cumsum([spans_of(len(x)) for x in streams])])
    for b, name in enumerate(names):
        if name != "short":
            assert sfirst[b] % 64 != 0 and spans_of(len(streams[b])) > 64, name
    assert len(longs[-1][1]) == 66 * SPAN
    for name, s in longs:                                               # the layout the stream promises
        if name.startswith("at_"):
            d = int(name.split("_")[-1])
            heads = {r[1] - 8 for r in M.serial_walk(s, 1 << 40)[0]}
            assert (64 << 20) + d in heads and (128 << 20) + d in heads, name
    caps = [O.frame_decoded_length(x) for x in streams]
    cd = SB.BlockCodec(0, O.HASH_CRC32C)
    got = decode(cd, streams, caps)
    check_decode(cd, streams, caps, got)                                # d_result[0], [2], [3] from the model; bytes = oracle = single call
    assert (got[3] == O.OK).all() and got[4][1] == sum(caps)
    # SNP_OPT_FRAME_SCAN 1: the single call walks the headers with one lane, and still agrees
    cd.ctx.set_option(N.OPT_FRAME_SCAN, 1)
    h, out_off, ol = got[0], got[1], got[2]
    for b, x in enumerate(streams):
        nrows = len(M.serial_walk(x, 1 << 40)[0])
        s_st, s_len, s_bytes = single_decode(cd, x, caps[b], max_chunks=nrows + 1)
        assert (s_st, s_len) == (O.OK, ol[b]) and s_bytes == h[out_off[b]:out_off[b] + ol[b]].tobytes(), names[b]


# ---- B: past 2^32 ----------------------------------------------------------------------------------------------------------------------------
def need_device_bytes(n: int):
    free = torch.cuda.mem_get_info()[0]
    if free < n:
        pytest.skip(f"needs {n >> 30} GiB of free device memory, {free >> 30} GiB free")


def high(blobs, lead: int):
    """Blobs packed (canaries between) from 2^32 + lead on, in a tensor of canaries: -> (tensor, offsets, lengths)."""
    small, off, lens = pack(blobs, lead=lead)
    big = torch.full((G32 + small.numel(),), CANARY, dtype=torch.uint8, device="cuda")
    big[G32:].copy_(small)
    del small
    return big, off + G32, lens


def below_g32_untouched(t) -> bool:
    return not bool((t[:G32] != CANARY).any().item())


def test_batch_offsets_past_4_gib():
    need_device_bytes(20 << 30)
    rng = np.random.default_rng(2 ** 32 + 1)
    blobs = ragged(rng, 20, 400000)
    lens = [len(x) for x in blobs]
    cd = SB.BlockCodec(0, O.HASH_CRC32C)
    # encode: every in_off and out_off at 2^32 + odd
    data, in_off, _ = high(blobs, 1)
    caps = np.array([frame_cap(n) for n in lens], dtype=np.int64)
    lo_off = np.concatenate([[3], 3 + np.cumsum(caps + 5)[:-1]]).astype(np.int64)
    out = torch.full((G32 + int(lo_off[-1] + caps[-1]) + 8,), CANARY, dtype=torch.uint8, device="cuda")
    _, _, ol, st, res = cd.frame_encode_buffers(data, dev(in_off), dev(lens), out=out, out_off=dev(lo_off + G32), out_cap=dev(caps),
                                                max_chunks=nchunks(lens))
    torch.cuda.synchronize()
    ol, st = ol.cpu().numpy(), st.cpu().numpy()
    assert (st == O.OK).all() and res.cpu().tolist() == [nchunks(lens), int(ol.sum())]
    assert below_g32_untouched(out)
    h = out[G32:].cpu().numpy()
    framed = []
    for b, x in enumerate(blobs):
        framed.append(O.frame_encode(x))
        assert h[lo_off[b]:lo_off[b] + ol[b]].tobytes() == framed[b], f"buffer {b}"
    assert (outside_ranges(h, lo_off, ol) == CANARY).all()
    assert below_g32_untouched(data)
    del data, out, h
    torch.cuda.empty_cache()
    # decode: the framed streams at 2^32 + odd, into outputs at 2^32 + odd
    src, f_off, f_len = high(framed, 5)
    d_off = np.concatenate([[7], 7 + np.cumsum(np.array(lens, dtype=np.int64) + 3)[:-1]]).astype(np.int64)
    out = torch.full((G32 + int(d_off[-1] + lens[-1]) + 8,), CANARY, dtype=torch.uint8, device="cuda")
    dcaps = np.array(lens, dtype=np.int64)
    ms = sum(spans_of(n) for n in f_len)
    dl, dst, dres = cd.frame_decode_buffers(src, dev(f_off), dev(f_len), out, dev(d_off + G32), dev(dcaps), max_chunks=nchunks(lens), max_spans=ms)
    torch.cuda.synchronize()
    _, _, _, mres, _ = M.decode_plan(framed, lens, nchunks(lens), ms, with_verdict=False)
    assert (dst.cpu().numpy() == O.OK).all() and np.array_equal(dl.cpu().numpy(), dcaps)
    assert dres.cpu().tolist() == [mres[0], sum(lens), mres[2], mres[3]]
    assert below_g32_untouched(out) and below_g32_untouched(src)
    h = out[G32:].cpu().numpy()
    for b, x in enumerate(blobs):
        assert h[d_off[b]:d_off[b] + lens[b]].tobytes() == x, f"stream {b}"
        assert single_decode(cd, framed[b], max(lens[b], 1)) == (O.OK, lens[b], x)
    assert (outside_ranges(h, d_off, dcaps) == CANARY).all()
    del src, out
    torch.cuda.empty_cache()


def periodic_content():
    """A period of 16 whole chunks (14 random, one of html, one of low entropy) and an odd-length tail: -> (period, tail, framed chunks of one
    period, framed tail chunk)."""
    rng = np.random.default_rng(4096)
    html = read_testdata("html") * 2
    pieces = [rng.integers(0, 256, B, dtype=np.uint8).tobytes() for _ in range(14)]
    pieces.insert(5, html[:B])
    pieces.insert(11, rng.integers(0, 4, B, dtype=np.uint8).tobytes())
    period = b"".join(pieces)
    tail = html[1000:1000 + 12345]
    chunks = b"".join(M.oracle_chunks(period, O.HASH_CRC32C))
    types = [c[0] for c in M.oracle_chunks(period, O.HASH_CRC32C)]
    assert types.count(0) == 2 and types.count(1) == 14
    return period, tail, chunks, M.oracle_chunks(tail, O.HASH_CRC32C)[0]


def test_encode_and_decode_a_buffer_longer_than_4_gib():
    """One buffer of 4.7 GB (a framed stream of 4.3 GB) between two small ones: the batch encode equals the oracle's chunks, built on the device;
    the batch decode gives the input back; the single-stream calls agree.  Peak device memory about 25 GB."""
    need_device_bytes(40 << 30)
    period, tail, chunks, tail_chunk = periodic_content()
    reps = (G32 + 64 * B - 10 - len(tail_chunk)) // len(chunks) + 1
    n = reps * len(period) + len(tail)
    flen = 10 + reps * len(chunks) + len(tail_chunk)
    assert n > G32 and flen > G32
    html = read_testdata("html")
    small = [html[:70001], html[3:3 + 999]]
    lens = np.array([len(small[0]), n, len(small[1])], dtype=np.int64)
    in_off = np.array([1, 1 + lens[0] + 3, 1 + lens[0] + 3 + n + 3], dtype=np.int64)
    data = torch.full((int(in_off[2] + lens[2]) + 4,), CANARY, dtype=torch.uint8, device="cuda")
    data[in_off[0]:in_off[0] + lens[0]].copy_(to_dev(small[0]))
    data[in_off[2]:in_off[2] + lens[2]].copy_(to_dev(small[1]))
    big = data[in_off[1]:in_off[1] + n]
    big[:reps * len(period)].view(reps, len(period))[:] = to_dev(period)
    big[reps * len(period):].copy_(to_dev(tail))
    cd = SB.BlockCodec(0, O.HASH_CRC32C)
    caps = np.array([frame_cap(int(x)) for x in lens], dtype=np.int64)
    f_off = np.concatenate([[3], 3 + np.cumsum(caps + 2)[:-1]]).astype(np.int64)
    framed = torch.full((int(f_off[-1] + caps[-1]) + 4,), CANARY, dtype=torch.uint8, device="cuda")
    mc = nchunks(lens)
    _, _, f_len, st, res = cd.frame_encode_buffers(data, dev(in_off), dev(lens), out=framed, out_off=dev(f_off), out_cap=dev(caps), max_chunks=mc)
    torch.cuda.synchronize()
    f_len = f_len.cpu().numpy()
    small_framed = [O.frame_encode(x) for x in small]
    assert st.cpu().tolist() == [O.OK] * 3 and f_len.tolist() == [len(small_framed[0]), flen, len(small_framed[1])]
    assert res.cpu().tolist() == [mc, int(f_len.sum())]
    torch.cuda.empty_cache()                                            # (the encode's 5.5 GB workspace)
    want = torch.empty(flen, dtype=torch.uint8, device="cuda")
    want[:10] = to_dev(M.STREAM_ID)
    want[10:10 + reps * len(chunks)].view(reps, len(chunks))[:] = to_dev(chunks)
    want[10 + reps * len(chunks):] = to_dev(tail_chunk)
    fb = framed[f_off[1]:f_off[1] + flen]
    assert torch.equal(fb, want)
    del want
    for b, ref in ((0, small_framed[0]), (2, small_framed[1])):
        assert framed[f_off[b]:f_off[b] + f_len[b]].cpu().numpy().tobytes() == ref
    gaps = [framed[:f_off[0]], framed[f_off[0] + f_len[0]:f_off[1]], framed[f_off[1] + flen:f_off[2]], framed[f_off[2] + f_len[2]:]]
    assert all(bool((g == CANARY).all().item()) for g in gaps)
    # batch decode back, next to the small ones
    o_off = np.array([5, 5 + lens[0] + 1, 5 + lens[0] + 1 + n + 1], dtype=np.int64)
    back = torch.full((int(o_off[2] + lens[2]) + 2,), CANARY, dtype=torch.uint8, device="cuda")
    ms = int(sum(spans_of(int(x)) for x in f_len))
    ol, dst, dres = cd.frame_decode_buffers(framed, dev(f_off), dev(f_len), back, dev(o_off), dev(lens), max_chunks=mc, max_spans=ms)
    torch.cuda.synchronize()
    assert dst.cpu().tolist() == [O.OK] * 3 and np.array_equal(ol.cpu().numpy(), lens)
    assert dres.cpu().tolist()[:3] == [mc, int(lens.sum()), ms]
    for b in range(3):
        assert torch.equal(back[o_off[b]:o_off[b] + lens[b]], data[in_off[b]:in_off[b] + lens[b]]), f"stream {b}"
    gaps = [back[:o_off[0]], back[o_off[0] + lens[0]:o_off[1]], back[o_off[1] + n:o_off[2]], back[o_off[2] + lens[2]:]]
    assert all(bool((g == CANARY).all().item()) for g in gaps)
    # the single-stream calls on the big buffer alone
    back.fill_(0)
    torch.cuda.empty_cache()
    r = cd.frame_decode(fb, flen, back[:n], mc + 1)
    torch.cuda.synchronize()
    assert r.cpu().tolist() == [n, O.OK] and torch.equal(back[:n], big)
    del back
    torch.cuda.empty_cache()
    so, sw = cd.frame_encode(big)
    torch.cuda.synchronize()
    assert int(sw.item()) == flen and torch.equal(so[:flen], fb)
    del so, sw, framed, fb, big, data
    torch.cuda.empty_cache()


# ---- C: corrupt streams, differential --------------------------------------------------------------------------------------------------------
MUTATIONS = ["type", "length", "crc", "body", "varint", "truncate", "reserved", "declared", "none"]


def fuzz_chunks(rng, pools, target: int):
    """-> (chunks, indices of the data chunks, indices of the compressed ones): compressed, raw, padding, skippable and repeated identifiers."""
    chunks = [M.STREAM_ID]
    n = 10

    def piece():
        src = pools[int(rng.integers(0, len(pools)))]
        ln = int(rng.integers(1, B + 1)) if rng.integers(0, 3) else int(rng.integers(1, 300))
        o = int(rng.integers(0, len(src) - ln))
        return src[o:o + ln]

    kinds = [0]                                                         # one compressed chunk first
    while n < target:
        k = kinds.pop() if kinds else int(rng.integers(0, 10))
        if k < 5:
            c = M.data_chunk(piece())
        elif k < 7:
            c = M.data_chunk(piece(), compressed=False)
        elif k == 7:
            c = M.chunk(0xFE, bytes(int(rng.integers(0, 3000))))
        elif k == 8:
            c = M.chunk(int(rng.integers(0x80, 0xFE)), rng.integers(0, 256, int(rng.integers(0, 5000)), dtype=np.uint8).tobytes())
        else:
            c = M.STREAM_ID
        chunks.append(c)
        n += len(c)
    data = [i for i, c in enumerate(chunks) if c[0] <= 1]
    comp = [i for i, c in enumerate(chunks) if c[0] == 0]
    return chunks, data, comp


def varint_len(b: bytes) -> int:
    return next(i for i, c in enumerate(b) if c < 128) + 1


def mutate(rng, chunks, data, comp, kind: str):
    """One mutation of the menu: -> the stream's bytes."""
    ch = list(chunks)

    def flip(i, lo, hi):                                                # one bit of chunk i's bytes [lo, hi)
        c = bytearray(ch[i])
        p = int(rng.integers(lo, hi))
        c[p] ^= 1 << int(rng.integers(0, 8))
        ch[i] = bytes(c)

    if kind == "type":
        flip(int(rng.choice(data)), 0, 1)
    elif kind == "length":
        flip(int(rng.integers(1, len(ch))), 1, 4)
    elif kind == "crc":
        flip(int(rng.choice(data)), 4, 8)
    elif kind == "body":
        i = int(rng.choice(data))
        lo = 8 + (varint_len(ch[i][8:]) if ch[i][0] == 0 else 0)
        if len(ch[i]) > lo:
            flip(i, lo, len(ch[i]))
        else:
            flip(i, 4, 8)
    elif kind == "varint":
        i = int(rng.choice(comp))
        flip(i, 8, 8 + varint_len(ch[i][8:]))
    elif kind == "reserved":
        ch.insert(int(rng.integers(1, len(ch) + 1)), M.chunk(int(rng.integers(0x02, 0x80)), rng.integers(0, 256, int(rng.integers(0, 40)), dtype=np.uint8).tobytes()))
    elif kind == "declared":                                            # the largest compressed chunk declares 5 000 .. 60 000 more bytes
        i = max(comp, key=lambda j: len(ch[j]))
        c = ch[i]
        v = varint_len(c[8:])
        dec = O.varint_read(c[8:8 + v])[0] + int(rng.integers(5000, 60000))
        body = c[4:8] + O.varint_write(dec) + c[8 + v:]
        ch[i] = M.chunk(0, body)
    s = b"".join(ch)
    if kind == "truncate":
        s = s[:int(rng.integers(1, len(s)))]
    return s


def expected(streams, caps, mc: int, ms: int):
    """statuses, out_len and d_result of a batch: the serial walk and k_fd_verdict's precedence per stream, the admission prefix over the batch,
    and the resolver's misses from the span walk."""
    ns = len(streams)
    serial = [M.serial_walk(x, c) for x, c in zip(streams, caps)]
    sfirst = np.concatenate([[0], np.cumsum([spans_of(len(x)) for x in streams])])
    cfirst = np.concatenate([[0], np.cumsum([len(w[0]) for w in serial])])
    status = np.full(ns, O.ERR_OUTPUT_TOO_SMALL, dtype=np.int32)
    out_len = np.zeros(ns, dtype=np.int64)
    missed = 0
    for b, x in enumerate(streams):
        if sfirst[b + 1] > ms:
            continue
        sw = M.span_walk(x, caps[b])
        assert sw[:3] == serial[b], f"model: span walk != serial walk, stream {b}"
        missed += sw[3]
        if cfirst[b + 1] <= mc:
            status[b], out_len[b] = M.verdict(x, *serial[b])
    walked = sfirst[1:] <= ms
    res = [int(cfirst[1:][walked].max()) if walked.any() else 0, int(out_len[status == O.OK].sum()), int(sfirst[ns]), missed]
    return status, out_len, res


def fuzz_batch(seed: int):
    rng = np.random.default_rng(1000 + seed)
    pools = pool_bytes()
    streams, caps, kinds = [], [], []
    for b in range(96):
        kind = MUTATIONS[b % len(MUTATIONS)]
        chunks, data, comp = fuzz_chunks(rng, pools, int(rng.integers(1 << 10, 3 << 20)))
        s = mutate(rng, chunks, data, comp, kind)
        total = M.serial_walk(b"".join(chunks) if kind == "declared" else s, 1 << 40)[1]
        cap = [total, total - 1, total + int(rng.integers(1, 5000))][int(rng.integers(0, 3))]
        streams.append(s)
        caps.append(max(cap, 1))
        kinds.append(kind)
    order = rng.permutation(len(streams))
    return [streams[i] for i in order], [caps[i] for i in order], [kinds[i] for i in order]


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_corrupt_streams_side_by_side_under_the_admission_prefix(seed):
    streams, caps, kinds = fuzz_batch(seed)
    cd = SB.BlockCodec(0, O.HASH_CRC32C)
    need_s = sum(spans_of(len(x)) for x in streams)
    need_c = sum(len(M.serial_walk(x, c)[0]) for x, c in zip(streams, caps))
    ok_bytes = {}
    for run, (mc, ms) in enumerate(((need_c, need_s), (need_c * 3 // 5, need_s), (need_c, need_s * 3 // 5), (need_c + 777, need_s + 5))):
        h, out_off, ol, st, res = decode(cd, streams, caps, max_chunks=mc, max_spans=ms)
        w_st, w_ol, w_res = expected(streams, caps, mc, ms)
        bad = np.nonzero(st != w_st)[0]
        assert bad.size == 0, f"run {run}: streams {bad[:8].tolist()} ({[kinds[i] for i in bad[:8]]}): {st[bad[:8]].tolist()} != {w_st[bad[:8]].tolist()}"
        assert np.array_equal(ol, w_ol) and res == w_res, (run, res, w_res)
        for b in np.flatnonzero(st == O.OK):
            if b not in ok_bytes:
                ok_bytes[b] = O.frame_decode(streams[b])
            assert h[out_off[b]:out_off[b] + ol[b]].tobytes() == ok_bytes[b], f"run {run}: stream {b} ({kinds[b]})"
        if run == 0:
            for b, x in enumerate(streams):
                s_st, s_len, s_bytes = single_decode(cd, x, caps[b])
                assert (s_st, s_len) == (st[b], ol[b]), f"stream {b} ({kinds[b]}): single {(s_st, s_len)} batch {(st[b], ol[b])}"
                if s_st == O.OK:
                    assert s_bytes == ok_bytes[b]
            assert (st == O.OK).any() and (st != O.OK).any()
            for kind in MUTATIONS[:-1]:
                assert any(st[b] != O.OK for b in range(len(streams)) if kinds[b] == kind), f"no {kind} mutation failed"


def precedence_streams():
    """Streams that fail in two places: two failing chunks of different statuses in both orders, a failing chunk then a tail error, and clean
    streams between them."""
    html = read_testdata("html") * 4
    ID = M.STREAM_ID
    good = M.data_chunk(html[:20000])
    crc = bytearray(M.data_chunk(html[100:9000]))
    crc[6] ^= 0x10
    crc = bytes(crc)
    offset = M.chunk(0x00, O.crc32c(b"ab" * 4, masked=True).to_bytes(4, "little") + b"\x08\x04ab\x09\x05")   # a copy before the output
    out = []
    for i in range(12):
        clean = O.frame_encode(html[i * 1000:i * 1000 + 30000 + i])
        out += [("clean", clean), ("crc_then_offset", ID + good + crc + good + offset), ("offset_then_crc", ID + offset + good + crc),
                ("crc_then_truncated", ID + good + crc + good[:-3 - i]), ("offset_then_type", ID + good + offset + M.chunk(0x02 + i, b"zz") + good),
                ("clean", clean[:10] + good + clean[10:])]
    return out


def test_verdict_takes_the_first_failing_chunk_before_the_tail():
    named = precedence_streams()
    streams = [s for _, s in named]
    caps = [max(M.serial_walk(x, 1 << 40)[1], 1) for x in streams]
    cd = SB.BlockCodec(0, O.HASH_CRC32C)
    got = decode(cd, streams, caps)
    check_decode(cd, streams, caps, got)
    w_st, w_ol, w_res = expected(streams, caps, 1 << 32, len(streams))
    assert np.array_equal(got[3], w_st) and np.array_equal(got[2], w_ol) and got[4] == w_res
    want = {"clean": O.OK, "crc_then_offset": O.ERR_CRC_MISMATCH, "crc_then_truncated": O.ERR_CRC_MISMATCH}
    for b, (name, _) in enumerate(named):
        if name in want:
            assert got[3][b] == want[name], (b, name)
        else:
            assert got[3][b] not in (O.OK, O.ERR_CRC_MISMATCH, O.ERR_CHUNK_TYPE, O.ERR_OUTPUT_TOO_SMALL), (b, name, got[3][b])


# ---- D: every layout -------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def layout_batch():
    rng = np.random.default_rng(13)
    html = read_testdata("html") * 8
    return [html[:n] for n in (0, 1, 65535, 65536, 65537)] + ragged(rng, 19, 250000)


@functools.lru_cache(maxsize=None)
def layout_batch_oracle(variant: int):
    return [O.frame_encode(x, variant) for x in layout_batch()]


@pytest.mark.parametrize("layout", layouts.COMPRESS_LAYOUTS)
def test_encode_under_every_compress_layout_and_crc_kernel(layout):
    blobs = layout_batch()
    for variant in (O.HASH_CRC32C, O.HASH_MUL):
        for crc_kernel in (0, 1):
            cd = SB.BlockCodec(0, variant)
            layouts.set_compress_layout(cd.ctx, layout)
            cd.ctx.set_option(N.OPT_CRC_KERNEL, crc_kernel)
            out, out_off, ol, st, res = encode(cd, blobs)
            assert (st == O.OK).all() and res == [nchunks([len(x) for x in blobs]), int(ol.sum())]
            for b, ref in enumerate(layout_batch_oracle(variant)):
                assert out[out_off[b]:out_off[b] + ol[b]].tobytes() == ref, f"{layout} variant {variant} crc kernel {crc_kernel}: buffer {b}"
            assert (outside_ranges(out, out_off, ol) == CANARY).all()


def test_encode_auto_policy_across_its_crossovers():
    """About 40 chunks with max_chunks = need, 1 536 (the dual form) and 32 769 (lanes): the same bytes."""
    rng = np.random.default_rng(40)
    blobs = ragged(rng, 16, 300000)
    need = nchunks([len(x) for x in blobs])
    assert 30 <= need <= 60
    cd = SB.BlockCodec(0, O.HASH_CRC32C)
    ref = encode(cd, blobs, max_chunks=need)
    assert (ref[3] == O.OK).all()
    for b, x in enumerate(blobs):
        assert ref[0][ref[1][b]:ref[1][b] + ref[2][b]].tobytes() == O.frame_encode(x)
    for mc in (1536, 32769):
        got = encode(cd, blobs, max_chunks=mc)
        assert np.array_equal(got[0], ref[0]) and np.array_equal(got[2], ref[2]) and np.array_equal(got[3], ref[3]) and got[4] == ref[4], mc


@functools.lru_cache(maxsize=None)
def mixed_decode_batch():
    """Clean, corrupt, tiny-chunk, raw-chunk and empty streams; capacities exact or loose; max_chunks loose, so pad slots exist."""
    rng = np.random.default_rng(17)
    html = read_testdata("html") * 4
    streams = [O.frame_encode(x) for x in ragged(rng, 12, 300000)]
    streams += [s for _, s in hand_streams()]
    streams.append(M.STREAM_ID + b"".join(M.data_chunk(html[i:i + 1 + i % 37], compressed=i % 2 == 0) for i in range(0, 3000, 13)))
    streams.append(O.frame_encode(rng.integers(0, 256, 300000, dtype=np.uint8).tobytes()))
    streams += [b"", M.STREAM_ID, b""]
    caps = [max(M.serial_walk(x, 1 << 40)[1] + (i % 3) * 17, 1) for i, x in enumerate(streams)]
    mc = sum(len(M.serial_walk(x, c)[0]) for x, c in zip(streams, caps)) + 300
    return streams, caps, mc


@functools.lru_cache(maxsize=None)
def mixed_default():
    streams, caps, mc = mixed_decode_batch()
    cd = SB.BlockCodec(0, O.HASH_CRC32C)
    got = decode(cd, streams, caps, max_chunks=mc)
    check_decode(cd, streams, caps, got, max_chunks=mc)
    st = got[3]
    assert (st == O.OK).any() and (st != O.OK).any()
    return got


def same_as_default(tag, got):
    ref = mixed_default()
    assert np.array_equal(got[3], ref[3]) and np.array_equal(got[2], ref[2]) and got[4] == ref[4], tag
    for b in np.flatnonzero(ref[3] == O.OK):
        o = ref[1][b]
        assert np.array_equal(got[0][o:o + ref[2][b]], ref[0][o:o + ref[2][b]]), f"{tag}: stream {b}"


@pytest.mark.parametrize("fenced", [0, 1])
@pytest.mark.parametrize("layout", layouts.DECODE_LAYOUTS)
def test_decode_under_every_decode_layout(layout, fenced):
    streams, caps, mc = mixed_decode_batch()
    mixed_default()
    cd = SB.BlockCodec(0, O.HASH_CRC32C)
    layouts.set_decode_layout(cd.ctx, layout, fenced)
    same_as_default(f"{layout} fenced={fenced}", decode(cd, streams, caps, max_chunks=mc))


@pytest.mark.parametrize("throttle", [256, 65536])
def test_decode_under_the_lds_throttle(throttle):
    streams, caps, mc = mixed_decode_batch()
    mixed_default()
    cd = SB.BlockCodec(0, O.HASH_CRC32C)
    cd.ctx.set_option(N.OPT_DECODE_LDS_THROTTLE, throttle)
    same_as_default(f"throttle {throttle}", decode(cd, streams, caps, max_chunks=mc))


def test_decode_after_batches_that_flip_the_previous_batch_hint():
    """snp_decompress_batch picks its layout by what the context's previous batch looked like: a frame decode right after thousands of tiny
    blocks, and right after 64 KiB blocks, gives the default run's results."""
    streams, caps, mc = mixed_decode_batch()
    mixed_default()
    cd = SB.BlockCodec(0, O.HASH_CRC32C)
    html = read_testdata("html") * 8
    for size, count in ((23, 4000), (B, 64)):
        blocks = [html[i * 97 % 500000:i * 97 % 500000 + size] for i in range(count)]
        comp, c_off, c_len = pack([O.compress(x) for x in blocks])
        o_off = np.arange(count, dtype=np.int64) * size
        out = torch.empty(count * size, dtype=torch.uint8, device="cuda")
        cap = torch.full((count,), size, dtype=torch.int32, device="cuda")
        ol, st = cd.decompress(comp, dev(c_off), dev(c_len).to(torch.int32), out, dev(o_off), cap)
        torch.cuda.synchronize()
        assert (st.cpu().numpy() == O.OK).all() and out.cpu().numpy().tobytes() == b"".join(blocks)
        same_as_default(f"after blocks of {size}", decode(cd, streams, caps, max_chunks=mc))


# ---- E: compressed versus raw ----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def edge_chunks(variant: int):
    """Chunks of 65 536 bytes whose compressed form (varint included) is raw - 1, raw and raw + 1 bytes long: random bytes with a repeat of
    tuned length near the start, found by search with the oracle."""
    rng = np.random.default_rng(700 + variant)
    found = {}
    for _ in range(400):
        a = int(rng.integers(40, 2000))
        head = rng.integers(0, 256, a, dtype=np.uint8).tobytes()
        rest = rng.integers(0, 256, B, dtype=np.uint8).tobytes()
        src = int(rng.integers(0, 32))
        for r in range(4, 40):
            x = (head + head[src:src + r] + rest)[:B]
            d = len(O.compress(x, variant)) - B
            if d in (-1, 0, 1) and d not in found:
                found[d] = x
        if len(found) == 3:
            return found
    raise AssertionError(f"no chunk found for {sorted({-1, 0, 1} - set(found))}")


@pytest.mark.parametrize("variant", [O.HASH_CRC32C, O.HASH_MUL])
def test_chunk_compressed_only_when_shorter_than_raw(variant):
    found = edge_chunks(variant)
    html = read_testdata("html")
    blobs = [found[-1], found[0], found[1], found[0] + html[:3000], html[:1000] + found[-1], found[1] + found[0]]
    cd = SB.BlockCodec(0, variant)
    out, out_off, ol, st, res = encode(cd, blobs)
    assert (st == O.OK).all()
    types = []
    for b, x in enumerate(blobs):
        ref = O.frame_encode(x, variant)
        got = out[out_off[b]:out_off[b] + ol[b]].tobytes()
        assert got == ref, f"buffer {b}"
        so, sw = cd.frame_encode(to_dev(x))
        assert so[:int(sw.item())].cpu().numpy().tobytes() == ref, f"buffer {b}: single call"
        types.append(got[10])
    assert types[:3] == [0, 1, 1] and [c[0] for c in M.oracle_chunks(blobs[5], variant)] == [1, 1]


# ---- F: graph replay with changing outcomes --------------------------------------------------------------------------------------------------
def test_graph_replays_follow_corruption_in_place():
    html = read_testdata("html") * 8
    plain = [html[:70000], html[5:5 + 200001], html[9:9 + 999], html[:1 << 20], html[77:77 + 65536]]
    streams = [O.frame_encode(x) for x in plain]
    lens = np.array([len(x) for x in plain], dtype=np.int64)
    framed, f_off, f_len = pack(streams)
    o_off, total = np.concatenate([[1], 1 + np.cumsum(lens + 2)[:-1]]).astype(np.int64), int(lens.sum()) + 2 * len(lens) + 4
    out = torch.full((total,), CANARY, dtype=torch.uint8, device="cuda")
    mc = nchunks(lens)
    ms = len(streams)
    cd = SB.BlockCodec(0, O.HASH_CRC32C)
    work = torch.empty(N.frame_buffers_lib().snp_frame_decode_buffers_workspace(len(streams), mc, ms), dtype=torch.uint8, device="cuda")
    d_f_off, d_f_len, d_o_off, d_caps = dev(f_off), dev(f_len), dev(o_off), dev(lens)

    def call():
        return cd.frame_decode_buffers(framed, d_f_off, d_f_len, out, d_o_off, d_caps, max_chunks=mc, max_spans=ms, work=work)

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        call()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        ol, st, res = call()
    clean = framed.clone()
    # stream 1: a flipped bit in its second chunk's body; stream 3: a flipped bit in its fifth chunk's CRC, and a flipped type byte of its
    # twelfth chunk (a reserved type: the walk stops there, but the CRC failure comes first)
    heads = [[r[1] - 8 for r in M.serial_walk(x, 1 << 40)[0]] for x in streams]
    edits = [(1, heads[1][1] + 8 + 200, 0x04), (3, heads[3][4] + 5, 0x20), (3, heads[3][11], 0x04)]
    for replay, corrupt in enumerate((False, True, False, True)):
        host = [bytearray(x) for x in streams]
        framed.copy_(clean)
        if corrupt:
            for b, p, bit in edits:
                framed[int(f_off[b]) + p] ^= bit
                host[b][p] ^= bit
        out.fill_(CANARY)
        g.replay()
        torch.cuda.synchronize()
        w_st, w_ol, w_res = expected([bytes(x) for x in host], lens, mc, ms)
        assert np.array_equal(st.cpu().numpy(), w_st) and np.array_equal(ol.cpu().numpy(), w_ol), replay
        assert res.cpu().tolist() == w_res, replay
        want = list(zip(w_st.tolist(), w_ol.tolist()))
        if corrupt:
            assert [w[0] for w in want] == [O.OK, want[1][0], O.OK, O.ERR_CRC_MISMATCH, O.OK] and want[1][0] != O.OK
            assert w_res[0] < mc                                        # (stream 3's walk stopped at the reserved type)
        else:
            assert w_res == [mc, int(lens.sum()), ms, 0]
        h = out.cpu().numpy()
        for b, x in enumerate(plain):
            if want[b][0] == O.OK:
                assert h[o_off[b]:o_off[b] + lens[b]].tobytes() == x, (replay, b)

"""snp_frame_encode_buffers_batch / snp_frame_decode_buffers_batch (BlockCodec.frame_encode_buffers / frame_decode_buffers): many framed streams per
call, each against the oracle and against the single-stream device calls (snp_frame_encode_device / snp_frame_decode_device) on that stream
alone.  Odd input and output offsets, canary bytes around every range, exact d_result.  Needs an MI355X."""
import numpy as np
import pytest
import torch

import frame_buffers_model as M
import oracle as O
from conftest import read_testdata
from frame_buffers_helpers import B, CANARY, check_decode, decode, dev, encode, frame_cap, nchunks, outside_ranges, pack, ragged

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from snappier_amd import batch as SB, _native as N


# ---- encode ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", [O.HASH_CRC32C, O.HASH_MUL])
def test_encode_edge_lengths_equal_the_oracle_and_the_single_call(variant):
    html = read_testdata("html") * 12
    lens = [0, 1, 65535, 65536, 65537, (1 << 20) + 3]
    blobs = [html[i:i + n] for i, n in enumerate(lens)]
    cd = SB.BlockCodec(0, variant)
    out, out_off, ol, st, res = encode(cd, blobs)
    assert (st == O.OK).all() and res == [nchunks(lens), int(ol.sum())]
    for b, x in enumerate(blobs):
        ref = O.frame_encode(x, variant)
        assert out[out_off[b]:out_off[b] + ol[b]].tobytes() == ref, f"buffer {b} ({len(x)} B)"
        raw = torch.from_numpy(np.frombuffer(x, dtype=np.uint8).copy()).cuda() if x else torch.empty(0, dtype=torch.uint8, device="cuda")
        so, sw = cd.frame_encode(raw)
        assert so[:int(sw.item())].cpu().numpy().tobytes() == ref
    assert (outside_ranges(out, out_off, ol) == CANARY).all()


@pytest.mark.parametrize("variant", [O.HASH_CRC32C, O.HASH_MUL])
def test_encode_seeded_ragged_batch_of_mixed_content(variant):
    rng = np.random.default_rng(11 + variant)
    blobs = ragged(rng, 48, 300000)
    cd = SB.BlockCodec(0, variant)
    out, out_off, ol, st, res = encode(cd, blobs)
    assert (st == O.OK).all() and res == [nchunks([len(x) for x in blobs]), int(ol.sum())]
    raw_chunks = 0
    for b, x in enumerate(blobs):
        got = out[out_off[b]:out_off[b] + ol[b]].tobytes()
        assert got == O.frame_encode(x, variant), f"buffer {b}"
        raw_chunks += sum(c[0] == 1 for c in M.oracle_chunks(x, variant))
    assert raw_chunks > 0                                               # random content: type 0x01 chunks
    assert (outside_ranges(out, out_off, ol) == CANARY).all()


def test_encode_capacity_exact_fits_one_byte_less_fails_alone():
    html = read_testdata("html") * 4
    blobs = [html[:70000], html[5:5 + 200000], html[9:9 + 17]]
    cd = SB.BlockCodec(0, O.HASH_CRC32C)
    exact = [len(O.frame_encode(x)) for x in blobs]
    out, out_off, ol, st, res = encode(cd, blobs, caps=exact)
    assert (st == O.OK).all() and ol.tolist() == exact
    short = list(exact)
    short[1] -= 1
    out, out_off, ol, st, res = encode(cd, blobs, caps=short)
    assert st.tolist() == [O.OK, O.ERR_OUTPUT_TOO_SMALL, O.OK] and ol[1] == 0
    assert (out[out_off[1]:out_off[1] + short[1]] == CANARY).all()
    assert res == [nchunks([len(x) for x in blobs]), exact[0] + exact[2]]


def test_encode_max_chunks_short_and_loose():
    rng = np.random.default_rng(3)
    blobs = ragged(rng, 12, 200000)
    lens = [len(x) for x in blobs]
    need = nchunks(lens)
    cd = SB.BlockCodec(0, O.HASH_CRC32C)
    ref = encode(cd, blobs)
    loose = encode(cd, blobs, max_chunks=need + 37)
    assert np.array_equal(loose[0], ref[0]) and loose[4] == ref[4]
    short = need - 3
    out, out_off, ol, st, res = encode(cd, blobs, max_chunks=short)
    first = np.concatenate([[0], np.cumsum([(n + B - 1) // B for n in lens])])
    assert res[0] == need
    for b in range(len(blobs)):
        if first[b + 1] <= short:
            assert st[b] == O.OK and out[out_off[b]:out_off[b] + ol[b]].tobytes() == ref[0][ref[1][b]:ref[1][b] + ref[2][b]].tobytes()
        else:
            assert st[b] == O.ERR_OUTPUT_TOO_SMALL and ol[b] == 0
    assert (outside_ranges(out, out_off, ol) == CANARY).all()


# ---- decode ----------------------------------------------------------------------------------------------------------------------------------
def hand_streams():
    html = read_testdata("html") * 8
    ID = M.STREAM_ID
    rng = np.random.default_rng(5)
    good = ID + M.data_chunk(html[:40000]) + M.chunk(0xFE, b"\0" * 100) + M.data_chunk(html[40000:60000], compressed=False) + M.chunk(0x80, b"x" * 9)
    concat = O.frame_encode(html[:70000]) + O.frame_encode(html[1000:1100])
    big_skip = ID + M.data_chunk(html[:1000]) + M.chunk(0x99, bytes(rng.integers(0, 2, (2 << 20) + 200000, dtype=np.uint8))) + \
        b"".join(M.data_chunk(html[i:i + 65536]) for i in range(0, 300000, 65536))
    crc_bad = bytearray(ID + M.data_chunk(html[:30000]) + M.data_chunk(html[30000:50000]))
    crc_bad[10 + 4 + len(M.data_chunk(html[:30000])) + 1] ^= 0x40
    bad_varint = ID + M.chunk(0x00, b"\1\2\3\4" + b"\xff" * 6 + b"abc")
    bad_offset = ID + M.data_chunk(html[:500]) + M.chunk(0x00, O.crc32c(b"ab" * 4, masked=True).to_bytes(4, "little") + b"\x08\x04ab\x09\x05")
    crc_then_trunc = bytes(crc_bad) + M.data_chunk(html[:100])[:-7]
    return [
        ("good", good), ("concat", concat), ("big_skip", big_skip), ("id_only", ID), ("empty", b""),
        ("crc", bytes(crc_bad)), ("type", ID + M.chunk(0x05, b"abc") + M.data_chunk(html[:10])),
        ("trunc_header", ID + M.data_chunk(html[:300]) + b"\x00\x10"), ("trunc_body", (ID + M.data_chunk(html[:3000]))[:-5]),
        ("bad_varint", bad_varint), ("bad_offset", bad_offset), ("crc_then_trunc", crc_then_trunc),
    ]


def straddling_streams():
    """Raw chunks behind a skippable chunk of d bytes: headers at 2^20 - 3 .. 2^20 + 2, and totals of 2^20 - 2 .. 2^20 + 2."""
    out = []
    raw = bytes(range(256)) * 256
    base = M.STREAM_ID + b"".join(M.data_chunk(raw, compressed=False) for _ in range(15))   # 10 + 15 * 65544
    for delta in (-3, -2, -1, 0, 1, 2):
        pad = (1 << 20) + delta - len(base) - 4
        out.append(base + M.chunk(0xFE, b"\0" * pad) + M.data_chunk(raw[:1000], compressed=False))
    for delta in (-2, -1, 0, 1, 2):
        body = (1 << 20) + delta - len(base) - 8
        out.append(base + M.data_chunk(raw[:body], compressed=False))
    return out


def test_decode_every_stream_equals_the_single_call():
    rng = np.random.default_rng(21)
    cd = SB.BlockCodec(0, O.HASH_CRC32C)
    plain = ragged(rng, 16, 300000)
    streams = [O.frame_encode(x) for x in plain] + [s for _, s in hand_streams()] + straddling_streams()
    caps = [max(O.frame_decoded_length(s) if _walk_ok(s) else len(s) * 4, 1) for s in streams]
    got = decode(cd, streams, caps)
    check_decode(cd, streams, caps, got)
    st = got[3]
    assert (st[:16] == O.OK).all()
    names = [n for n, _ in hand_streams()]
    for name, want in (("crc", O.ERR_CRC_MISMATCH), ("type", O.ERR_CHUNK_TYPE), ("trunc_header", O.ERR_TRUNCATED_STREAM),
                       ("trunc_body", O.ERR_TRUNCATED_STREAM), ("bad_varint", O.ERR_BAD_LENGTH), ("crc_then_trunc", O.ERR_CRC_MISMATCH)):
        assert st[16 + names.index(name)] == want, name
    assert st[16 + names.index("bad_offset")] not in (O.OK, O.ERR_OUTPUT_TOO_SMALL)
    assert got[4][3] > 0                                                # the 2 MiB skippable chunk: a span walked on the spot
    # SNP_OPT_FRAME_SCAN = 1 changes nothing
    cd.ctx.set_option(N.OPT_FRAME_SCAN, 1)
    again = decode(cd, streams, caps)
    assert again[4] == got[4] and np.array_equal(again[3], got[3]) and np.array_equal(again[2], got[2])
    for b in np.flatnonzero(st == O.OK):
        assert np.array_equal(again[0][got[1][b]:got[1][b] + got[2][b]], got[0][got[1][b]:got[1][b] + got[2][b]])


def _walk_ok(s):
    return M.serial_walk(s, 1 << 40)[2] == O.OK


def test_decode_capacity_exact_and_one_less():
    html = read_testdata("html") * 4
    streams = [O.frame_encode(html[:100000]), O.frame_encode(html[7:7 + 300]), O.frame_encode(html[:70000])]
    exact = [O.frame_decoded_length(s) for s in streams]
    cd = SB.BlockCodec(0, O.HASH_CRC32C)
    got = decode(cd, streams, exact)
    check_decode(cd, streams, exact, got)
    assert (got[3] == O.OK).all()
    caps = list(exact)
    caps[1] -= 1
    got = decode(cd, streams, caps)
    check_decode(cd, streams, caps, got)
    assert got[3].tolist() == [O.OK, O.ERR_OUTPUT_TOO_SMALL, O.OK] and got[2][1] == 0


def test_decode_max_spans_and_max_chunks_short_and_loose():
    rng = np.random.default_rng(8)
    html = read_testdata("html") * 40
    lens = [int(x) for x in rng.integers(0, 3 << 20, 10)]
    streams = [O.frame_encode(html[:n]) for n in lens]
    caps = [n for n in lens]
    cd = SB.BlockCodec(0, O.HASH_CRC32C)
    ref = decode(cd, streams, caps)
    check_decode(cd, streams, caps, ref)
    spans, chunks = ref[4][2], ref[4][0]
    sfirst = np.cumsum([(len(s) + M.SPAN - 1) // M.SPAN for s in streams])
    cfirst = np.cumsum([len(M.serial_walk(s, c)[0]) for s, c in zip(streams, caps)])
    for ms, mc in ((spans + 5, chunks + 9), (spans - 2, chunks), (spans, chunks - 4), (spans - 1, chunks - 1)):
        got = decode(cd, streams, caps, max_chunks=mc, max_spans=ms)
        check_decode(cd, streams, caps, got, max_chunks=mc, max_spans=ms)
        walked = sfirst <= ms
        assert got[4][2] == spans and got[4][0] == int(cfirst[walked].max()) if walked.any() else got[4][0] == 0
        for b in range(len(streams)):
            fits = walked[b] and cfirst[b] <= mc
            if fits:
                assert got[3][b] == O.OK and got[2][b] == ref[2][b]
            else:
                assert got[3][b] == O.ERR_OUTPUT_TOO_SMALL and got[2][b] == 0


def test_round_trip_of_the_encode_batch():
    rng = np.random.default_rng(31)
    blobs = ragged(rng, 40, 400000)
    cd = SB.BlockCodec(0, O.HASH_MUL)
    data, in_off, lens = pack(blobs)
    framed, f_off, f_len, st, res = cd.frame_encode_buffers(data, dev(in_off), dev(lens))
    assert (st.cpu().numpy() == O.OK).all()
    caps = dev(lens)
    o_off = torch.cumsum(caps, 0) - caps
    out = torch.empty(max(int(lens.sum()), 1), dtype=torch.uint8, device="cuda")
    ol, dst, dres = cd.frame_decode_buffers(framed, f_off, f_len, out, o_off, caps)
    torch.cuda.synchronize()
    assert (dst.cpu().numpy() == O.OK).all() and np.array_equal(ol.cpu().numpy(), lens)
    assert out[:int(lens.sum())].cpu().numpy().tobytes() == b"".join(blobs)
    assert dres.cpu().tolist() == [nchunks(lens), int(lens.sum()), sum((int(n) + M.SPAN - 1) // M.SPAN for n in f_len.cpu().numpy()), 0]


# ---- both ------------------------------------------------------------------------------------------------------------------------------------
def test_graph_capture_replays_on_new_inputs():
    cd = SB.BlockCodec(0, O.HASH_CRC32C)
    html = read_testdata("html") * 16
    lens = np.array([0, 5, 65536, 200001, 70000, 1 << 20], dtype=np.int64)
    src = torch.zeros(int(lens.sum()) + 64, dtype=torch.uint8, device="cuda")
    in_off = np.concatenate([[1], 1 + np.cumsum(lens)[:-1]]).astype(np.int64)
    caps = np.array([frame_cap(int(n)) for n in lens], dtype=np.int64)
    f_off = np.concatenate([[3], 3 + np.cumsum(caps)[:-1]]).astype(np.int64)
    framed = torch.zeros(int(caps.sum()) + 8, dtype=torch.uint8, device="cuda")
    back = torch.zeros(int(lens.sum()) + 64, dtype=torch.uint8, device="cuda")
    d_in_off, d_lens, d_caps, d_f_off = dev(in_off), dev(lens), dev(caps), dev(f_off)
    mc = nchunks(lens)
    ms = int(sum((int(c) + M.SPAN - 1) // M.SPAN for c in caps))
    FL = N.frame_buffers_lib()
    ew = torch.empty(FL.snp_frame_encode_buffers_workspace(len(lens), mc), dtype=torch.uint8, device="cuda")
    dw = torch.empty(FL.snp_frame_decode_buffers_workspace(len(lens), mc, ms), dtype=torch.uint8, device="cuda")

    def call():
        _, _, f_len, est, eres = cd.frame_encode_buffers(src, d_in_off, d_lens, out=framed, out_off=d_f_off, out_cap=d_caps, max_chunks=mc, work=ew)
        # the decode reads the lengths the encode wrote, on the device; each stream is walked with max_spans from its capacity
        ol, dst, dres = cd.frame_decode_buffers(framed, d_f_off, f_len, back, d_in_off, d_lens, max_chunks=mc, max_spans=ms, work=dw)
        return f_len, est, eres, ol, dst, dres

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        call()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        f_len, est, eres, ol, dst, dres = call()
    for seed in (1, 2):
        o = seed * 777
        for b, n in enumerate(lens):
            src[int(in_off[b]):int(in_off[b] + n)].copy_(torch.from_numpy(np.frombuffer(html[o + b:o + b + int(n)], dtype=np.uint8).copy()).cuda())
        back.zero_()
        g.replay()
        torch.cuda.synchronize()
        fl = f_len.cpu().numpy()
        h = framed.cpu().numpy()
        for b, n in enumerate(lens):
            x = html[o + b:o + b + int(n)]
            assert h[f_off[b]:f_off[b] + fl[b]].tobytes() == O.frame_encode(x)
            assert back[int(in_off[b]):int(in_off[b] + n)].cpu().numpy().tobytes() == x
        assert (est.cpu().numpy() == O.OK).all() and (dst.cpu().numpy() == O.OK).all()
        assert eres.cpu().tolist() == [mc, int(fl.sum())]
        assert dres.cpu().tolist() == [mc, int(lens.sum()), int(sum((int(n) + M.SPAN - 1) // M.SPAN for n in fl)), 0]


def test_wrapper_defaults():
    html = read_testdata("html") * 4
    blobs = [b"", html[:5], html[:65536], html[3:3 + 65537], html[:300000]]
    data, in_off, lens = pack(blobs)
    cd = SB.BlockCodec(0, O.HASH_CRC32C)
    out, out_off, out_len, status, result = cd.frame_encode_buffers(data, dev(in_off), dev(lens))
    torch.cuda.synchronize()
    cap = np.array([N.lib().snp_frame_max_encoded_length(int(n)) for n in lens], dtype=np.int64)
    assert out_off.dtype == torch.int64 and out_off.cpu().tolist() == (np.cumsum(cap) - cap).tolist() and out.numel() == int(cap.sum())
    assert out_len.dtype == torch.int64 and status.dtype == torch.int32 and result.dtype == torch.int64
    assert result.cpu().tolist() == [nchunks(lens), int(out_len.sum())]
    h, oo, ol = out.cpu().numpy(), out_off.cpu().numpy(), out_len.cpu().numpy()
    for b, x in enumerate(blobs):
        assert h[oo[b]:oo[b] + ol[b]].tobytes() == O.frame_encode(x)
    # decode with both bounds defaulted (a max_spans read-back, then a max_chunks = 0 call and a read of its d_result[0])
    dcap = dev(lens)
    doff = torch.cumsum(dcap, 0) - dcap
    back = torch.empty(int(lens.sum()), dtype=torch.uint8, device="cuda")
    dl, dst, dres = cd.frame_decode_buffers(out, out_off, out_len, back, doff, dcap)
    torch.cuda.synchronize()
    assert (dst.cpu().numpy() == O.OK).all() and np.array_equal(dl.cpu().numpy(), lens)
    assert back.cpu().numpy().tobytes() == b"".join(blobs)
    assert dres.cpu().tolist() == [nchunks(lens), int(lens.sum()), len(blobs), 0]   # (every framed stream holds at least its identifier)
    # no streams: OK, and d_result is still written
    _, _, e_len, _, e_res = cd.frame_encode_buffers(data, dev(in_off[:0]), dev(lens[:0]))
    e_dl, _, e_dres = cd.frame_decode_buffers(out, dev(in_off[:0]), dev(lens[:0]), back, dev(in_off[:0]), dev(lens[:0]))
    torch.cuda.synchronize()
    assert e_len.numel() == 0 and e_res.cpu().tolist() == [0, 0] and e_dl.numel() == 0 and e_dres.cpu().tolist() == [0, 0, 0, 0]
    with pytest.raises(ValueError):
        cd.frame_encode_buffers(data, dev(in_off), dev(lens), max_chunks=nchunks(lens), work=torch.empty(16, dtype=torch.uint8, device="cuda"))


def test_scale_300000_tiny_streams():
    """Every scan (buffers, chunk slots, spans, listed chunks) runs past 256 tiles of 1024."""
    nb = 300000
    rng = np.random.default_rng(99)
    lens = rng.integers(0, 40, nb).astype(np.int64)
    html = read_testdata("html")
    starts = rng.integers(0, len(html) - 64, nb)
    blobs = [html[int(s):int(s) + int(n)] for s, n in zip(starts, lens)]
    data, in_off, _ = pack(blobs, gap=1)
    cd = SB.BlockCodec(0, O.HASH_CRC32C)
    framed, f_off, f_len, st, res = cd.frame_encode_buffers(data, dev(in_off), dev(lens))
    torch.cuda.synchronize()
    fl = f_len.cpu().numpy()
    assert (st.cpu().numpy() == O.OK).all() and res.cpu().tolist() == [int((lens > 0).sum()), int(fl.sum())]
    h, fo = framed.cpu().numpy(), f_off.cpu().numpy()
    for b in range(0, nb, 997):
        assert h[fo[b]:fo[b] + fl[b]].tobytes() == O.frame_encode(blobs[b])
    caps = dev(lens)
    o_off = dev(np.concatenate([[1], 1 + np.cumsum(lens + 1)[:-1]]))
    out = torch.full((int(lens.sum()) + nb + 2,), CANARY, dtype=torch.uint8, device="cuda")
    nonempty = int((fl > 0).sum())
    ol, dst, dres = cd.frame_decode_buffers(framed, f_off, f_len, out, o_off, caps, max_chunks=int(res[0].item()), max_spans=nonempty)
    torch.cuda.synchronize()
    assert (dst.cpu().numpy() == O.OK).all() and np.array_equal(ol.cpu().numpy(), lens)
    assert dres.cpu().tolist() == [int((lens > 0).sum()), int(lens.sum()), nonempty, 0]
    ho, oo = out.cpu().numpy(), o_off.cpu().numpy()
    for b in range(0, nb, 997):
        assert ho[oo[b]:oo[b] + lens[b]].tobytes() == blobs[b]
    assert (outside_ranges(ho, oo, lens) == CANARY).all()

"""snp_frame_encode_chunked_batch (BlockCodec.frame_encode_seekable): every stream, status, length, index array and d_result against the model
(frame_chunked_model.py) at the chunk sizes where the compressor changes path, at the seams of the emit's workgroups, under both hash variants;
canary bytes around every output range and guard words around every array and the workspace; equality with snp_frame_encode_buffers_batch at
65536; the encoder's index against snp_frame_index_batch over the emitted streams and through snp_frame_read_indexed_batch; out_cap and
max_chunks failures; a buffer past 4 GiB; graph capture; the empty batch.  Needs an MI355X."""
import numpy as np
import pytest
import torch

import frame_buffers_helpers as H
import frame_chunked_model as K
import oracle as O
from conftest import read_testdata
from seekable_cases import windows
from seekable_harness import CANARY, KEYS, Encoded, Guarded

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from snappier_amd import batch as SB, _native as N

VARIANTS = [O.HASH_CRC32C, O.HASH_MUL]


@pytest.fixture(scope="module")
def content():
    html = read_testdata("html") * 4
    rnd = np.random.default_rng(3).integers(0, 256, 200000, dtype=np.uint8).tobytes()
    return html, rnd


def check(cd, blobs, cb, variant, read=True, **bounds):
    """The call against the model, field for field; when every buffer is OK, its index against snp_frame_index_batch over the emitted streams
    and (read) the input's bytes back through snp_frame_read_indexed_batch with the encoder's index."""
    e = Encoded(cd, blobs, cb, **bounds)
    want = K.encode(blobs, cb, variant, bounds.get("max_chunks"), bounds.get("caps"))
    for key in want:
        assert e.got[key] == want[key], (cb, key)
    if want["status"] != [O.OK] * len(blobs) or not blobs:
        return e, want
    d_off, d_len = H.dev(e.out_off), e.out_len.mid
    walked = cd.frame_index_buffers(e.out, d_off, d_len)
    for key, g in zip(KEYS, e.ix):
        used = want["result"][2] if key in ("start", "pos") else g.n
        assert torch.equal(getattr(walked, key)[:used], g.mid[:used]), (cb, key)
    assert walked.result.tolist()[:2] == [want["result"][2], sum(len(x) for x in blobs)]
    if read:
        reqs = [(b, ro, rl) for b, x in enumerate(blobs) for ro, rl in windows(len(x), cb)]
        expect = [blobs[b][ro:ro + rl] for b, ro, rl in reqs]
        caps = np.array([len(x) for x in expect], dtype=np.int64)
        r_off, total = H.out_layout(caps)
        arena = torch.full((total,), CANARY, dtype=torch.uint8, device="cuda")
        ol, st, res = cd.frame_read_indexed(e.out, d_off, d_len, e.frame_index(), torch.tensor([r[0] for r in reqs], dtype=torch.int32, device="cuda"),
                                            H.dev([r[1] for r in reqs]), H.dev([r[2] for r in reqs]), arena, H.dev(r_off), H.dev(caps))
        torch.cuda.synchronize()
        assert st.tolist() == [O.OK] * len(reqs) and ol.tolist() == caps.tolist() and res.tolist()[1::2] == [int(caps.sum()), len(reqs)]
        h = arena.cpu().numpy()
        for (b, ro, rl), x, o in zip(reqs, expect, r_off.tolist()):
            assert h[o:o + len(x)].tobytes() == x, (cb, b, ro, rl)
        assert (H.outside_ranges(h, r_off, caps) == CANARY).all()
    return e, want


# ---- 1: chunk sizes at the compressor's seams (and 4: their index) ---------------------------------------------------------------------------
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("cb", K.CHUNK_SIZES)
def test_chunk_sizes_at_the_compressors_seams(content, cb, variant):
    html, rnd = content
    blobs = [html[:n] for n in K.buffer_lengths(cb)] + [rnd[:min(3 * cb + 1, len(rnd))]]
    assert sum(len(x) for x in blobs) < 1 << 20
    _, want = check(SB.BlockCodec(0, variant), blobs, cb, variant)
    kinds = {s[p] for s, f0, f1 in zip(want["streams"], want["first"], want["first"][1:]) for p in want["pos"][f0:f1]}
    # both chunk types -- where both can be: a piece of up to 16 bytes is varint + one literal, two bytes more than the piece, so it stays raw
    assert kinds == ({0, 1} if cb > 17 else {1}) or (cb == 17 and 1 in kinds)


# ---- 2: 65536 is the existing call -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", VARIANTS)
def test_at_65536_the_output_is_that_of_frame_encode_buffers(variant):
    rng = np.random.default_rng(17 + variant)
    blobs = H.ragged(rng, 24, 300000) + [b"", b"x"]
    cd = SB.BlockCodec(0, variant)
    out, out_off, ol, st, res = H.encode(cd, blobs)
    for with_index in (False, True):
        e = Encoded(cd, blobs, 65536, with_index=with_index)
        assert np.array_equal(e.out_off, out_off) and np.array_equal(e.h, out)                      # the whole arena, canaries included
        assert e.got["out_len"] == ol.tolist() and e.got["status"] == st.tolist() and e.got["result"][:2] == res
        assert e.got["result"][2:] == [H.nchunks([len(x) for x in blobs]) if with_index else 0, len(blobs)]


# ---- 3: the seams of the emit's workgroups (and 4: their index) ----------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", VARIANTS)
def test_workgroup_seams(content, variant):
    html, rnd = content
    cd = SB.BlockCodec(0, variant)
    # 64-byte chunks: a workgroup takes 1 024 slots; the long buffer's 1 094 start in the first workgroup's second slot and end in the second
    check(cd, [html[:63], html[7:7 + 70001], rnd[:129]], 64, variant)
    check(cd, [(html + rnd[:50000])[:300000]], 1000, variant)           # 66 slots per workgroup, 300 slots


# ---- 4: without an index ---------------------------------------------------------------------------------------------------------------------
def test_without_an_index_only_the_row_count_differs(content):
    html, rnd = content
    cd = SB.BlockCodec(0, O.HASH_CRC32C)
    blobs = [html[:10000], b"", rnd[:5000], html[3:3 + 4097]]
    a, b = Encoded(cd, blobs, 4096), Encoded(cd, blobs, 4096, with_index=False)
    assert np.array_equal(a.h, b.h) and a.got["status"] == b.got["status"] and a.got["out_len"] == b.got["out_len"]
    assert b.got["result"] == a.got["result"][:2] + [0] + a.got["result"][3:] and a.got["result"][2] == 3 + 0 + 2 + 2
    assert b.got == K.encode(blobs, 4096, with_index=False)


# ---- 5: failures ---------------------------------------------------------------------------------------------------------------------------------
def test_out_cap_exact_fits_and_one_byte_short_fails_the_middle_buffer_alone(content):
    html, rnd = content
    cd = SB.BlockCodec(0, O.HASH_CRC32C)
    cb = 1000
    blobs = [html[:2500], html[9:9 + 7001], rnd[:1999] + html[:500]]
    exact = K.encode(blobs, cb)["out_len"]
    check(cd, blobs, cb, O.HASH_CRC32C, caps=exact)
    short = list(exact)
    short[1] -= 1
    e, want = check(cd, blobs, cb, O.HASH_CRC32C, caps=short)           # (the call checks that the failed buffer's range is still canary)
    assert e.got["status"] == [O.OK, O.ERR_OUTPUT_TOO_SMALL, O.OK] and e.got["first"] == [0, 3, 3, 6] and e.got["tail"][1] == O.ERR_OUTPUT_TOO_SMALL
    assert e.got["total"] == [2500, 0, 2499] and e.got["result"] == [14, exact[0] + exact[2], 6, 2]
    # an indexed read through this index: the buffers around it read back, the one that failed answers OUTPUT_TOO_SMALL
    reqs = [(0, 999, 1002), (1, 0, 10), (2, 1500, 999), (1, 5000, 0)]
    caps = np.array([r[2] for r in reqs], dtype=np.int64)
    r_off, total = H.out_layout(caps)
    arena = torch.full((total,), CANARY, dtype=torch.uint8, device="cuda")
    ol, st, _ = cd.frame_read_indexed(e.out, H.dev(e.out_off), e.out_len.mid, e.frame_index(), torch.tensor([r[0] for r in reqs], dtype=torch.int32, device="cuda"),
                                      H.dev([r[1] for r in reqs]), H.dev([r[2] for r in reqs]), arena, H.dev(r_off), H.dev(caps))
    torch.cuda.synchronize()
    assert st.tolist() == [O.OK, O.ERR_OUTPUT_TOO_SMALL, O.OK, O.ERR_OUTPUT_TOO_SMALL] and ol.tolist() == [1002, 0, 999, 0]
    h = arena.cpu().numpy()
    assert h[r_off[0]:r_off[0] + 1002].tobytes() == blobs[0][999:2001] and h[r_off[2]:r_off[2] + 999].tobytes() == blobs[2][1500:2499]


def test_max_chunks_three_short_and_loose(content):
    rng = np.random.default_rng(3)
    blobs = H.ragged(rng, 12, 200000)
    cd = SB.BlockCodec(0, O.HASH_CRC32C)
    cb = 16384
    need = sum(K.nchunks(len(x), cb) for x in blobs)
    ref, _ = check(cd, blobs, cb, O.HASH_CRC32C, read=False)
    loose, _ = check(cd, blobs, cb, O.HASH_CRC32C, read=False, max_chunks=need + 37)
    assert np.array_equal(loose.h, ref.h) and loose.got == ref.got      # a loose bound gives the same bytes
    short, want = check(cd, blobs, cb, O.HASH_CRC32C, max_chunks=need - 3)
    ok = sum(1 for s in want["status"] if s == O.OK)                    # prefix admission: the first buffer that does not fit and every later one
    assert 0 < ok < len(blobs) and want["status"] == [O.OK] * ok + [O.ERR_OUTPUT_TOO_SMALL] * (len(blobs) - ok)
    assert short.got["streams"][:ok] == ref.got["streams"][:ok] and short.got["result"][0] == need


# ---- 6: past 4 GiB -----------------------------------------------------------------------------------------------------------------------------
def test_one_buffer_past_4_gib_at_4096_byte_chunks():
    n, cb = (1 << 32) + 70001, 4096
    free = torch.cuda.mem_get_info()[0]
    if free < 40 << 30:
        pytest.skip(f"needs 40 GiB of free device memory, {free >> 30} GiB free")
    cd = SB.BlockCodec(0, O.HASH_CRC32C)
    # random bytes, so that the stream outgrows its input (raw chunks: 8 bytes each over it) and the last header lies past 2^32; 4 MiB of html in front
    src = torch.randint(0, 256, (n,), dtype=torch.uint8, device="cuda", generator=torch.Generator("cuda").manual_seed(5))
    html = torch.from_numpy(np.frombuffer(read_testdata("html"), dtype=np.uint8).copy()).cuda()
    src[:4 << 20].copy_(html.repeat((4 << 20) // html.numel() + 1)[:4 << 20])
    in_off, in_len = H.dev([0]), H.dev([n])
    mc = K.nchunks(n, cb)
    out, out_off, out_len, status, result, index = cd.frame_encode_seekable(src, in_off, in_len, cb, max_chunks=mc)
    size = int(out_len.item())
    assert status.tolist() == [O.OK] and result.tolist() == [mc, size, mc, 1] and n < size <= K.frame_cap(n, cb)
    spans = (size + (1 << 20) - 1) >> 20
    walked = cd.frame_index_buffers(out, out_off, out_len, max_spans=spans, max_entries=mc)
    for key in KEYS:
        assert torch.equal(getattr(walked, key), getattr(index, key)), key
    assert index.first.tolist() == [0, mc] and index.total.tolist() == [n] and int(index.pos[-1].item()) > 1 << 32
    assert int(index.start[-1].item()) == (mc - 1) * cb > 1 << 32
    del walked
    back = torch.empty(n, dtype=torch.uint8, device="cuda")
    ol, st, _ = cd.frame_decode_buffers(out, out_off, out_len, back, in_off, in_len, max_chunks=mc, max_spans=spans)
    assert st.tolist() == [O.OK] and ol.tolist() == [n] and torch.equal(back, src)


# ---- 7: graph capture ----------------------------------------------------------------------------------------------------------------------------
def test_graph_capture_replays_on_new_inputs():
    """256-byte chunks in a batch of more than 32 768 slots: the lane compressor, and -- the context having seen a batch whose longest fragment is
    256 bytes -- its small-fragment launch.  The hint arrives with the SECOND call (the first leaves it, the next one reads it), hence two calls
    before the capture, not one."""
    cd = SB.BlockCodec(0, O.HASH_CRC32C)
    cb = 256
    html = read_testdata("html") * 90
    lens = np.array([0, 5, cb * 20000 + 3, cb * 13000, 100], dtype=np.int64)
    mc = sum(K.nchunks(int(n), cb) for n in lens)
    assert mc > 32768
    src = torch.zeros(int(lens.sum()) + 64, dtype=torch.uint8, device="cuda")
    in_off = np.concatenate([[1], 1 + np.cumsum(lens)[:-1]]).astype(np.int64)
    caps = np.array([K.frame_cap(int(n), cb) for n in lens], dtype=np.int64)
    f_off = np.concatenate([[3], 3 + np.cumsum(caps)[:-1]]).astype(np.int64)
    framed = torch.zeros(int(caps.sum()) + 8, dtype=torch.uint8, device="cuda")
    d_in_off, d_lens, d_caps, d_f_off = H.dev(in_off), H.dev(lens), H.dev(caps), H.dev(f_off)
    work = torch.empty(N.frame_chunked_lib().snp_frame_encode_chunked_workspace(len(lens), mc, cb), dtype=torch.uint8, device="cuda")

    def fill(o):
        for b, n in enumerate(lens):
            src[int(in_off[b]):int(in_off[b] + n)].copy_(torch.from_numpy(np.frombuffer(html[o + b:o + b + int(n)], dtype=np.uint8).copy()).cuda())

    def call():
        return cd.frame_encode_seekable(src, d_in_off, d_lens, cb, out=framed, out_off=d_f_off, out_cap=d_caps, max_chunks=mc, work=work)[2:]

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
        f_len, est, eres, index = call()
    fill(777)
    framed.zero_()
    g.replay()
    torch.cuda.synchronize()
    want = K.encode([html[777 + b:777 + b + int(n)] for b, n in enumerate(lens)], cb)
    fl, h = f_len.tolist(), framed.cpu().numpy()
    assert est.tolist() == want["status"] and fl == want["out_len"] and eres.tolist() == want["result"]
    for b, x in enumerate(want["streams"]):
        assert h[f_off[b]:f_off[b] + fl[b]].tobytes() == x, b
    for key in KEYS:
        assert getattr(index, key).tolist() == want[key], key


# ---- 8: the empty batch, and the wrapper's defaults ----------------------------------------------------------------------------------------------
def test_empty_batch():
    cd = SB.BlockCodec(0, O.HASH_CRC32C)
    cd._bind()
    enc = N.frame_chunked_lib().snp_frame_encode_chunked_batch
    for with_index in (False, True):
        result, first = Guarded(4, torch.int64), Guarded(1, torch.int64)
        others = [Guarded(0, torch.int64) for _ in range(3)] + [Guarded(0, torch.int32)]
        ix = [first.ptr()] + [g.ptr() for g in others] if with_index else [None] * 5
        assert enc(cd.ctx.handle, None, None, None, 0, 4096, 0, None, None, None, None, None, *ix, None, result.ptr()) == O.OK
        torch.cuda.synchronize()
        assert result.read() == [0, 0, 0, 0]
        assert first.read() == ([0] if with_index else [int.from_bytes(bytes([CANARY]) * 8, "little", signed=True)])
        for g in others:
            g.read()
    empty = torch.empty(0, dtype=torch.int64, device="cuda")
    out, out_off, out_len, status, result, index = cd.frame_encode_seekable(torch.empty(0, dtype=torch.uint8, device="cuda"), empty, empty, 100)
    assert out_len.numel() == 0 and status.numel() == 0 and result.tolist() == [0] * 4 and index.first.tolist() == [0] and index.nentries == 0


def test_wrapper_defaults_and_gather(content):
    html, rnd = content
    blobs = [b"", html[:5], html[:4096], html[3:3 + 4097], rnd[:9000] + html[:30000]]
    data, in_off, lens = H.pack(blobs)
    cd = SB.BlockCodec(0, O.HASH_CRC32C)
    out, out_off, out_len, status, result, index = cd.frame_encode_seekable(data, H.dev(in_off), H.dev(lens), 4096)
    want = K.encode(blobs, 4096)
    assert status.tolist() == want["status"] and out_len.tolist() == want["out_len"] and result.tolist() == want["result"]
    assert [getattr(index, k).tolist() for k in KEYS] == [want[k] for k in KEYS]
    h = out.cpu().numpy()
    for o, n, x in zip(out_off.tolist(), out_len.tolist(), want["streams"]):
        assert h[o:o + n].tobytes() == x
    reqs = [(4, 4000, 8300), (2, 4095, 1), (3, 4096, 1), (1, 0, 99), (0, 0, 5)]
    got, g_off, g_len, g_st = cd.frame_gather_to_memory(out, out_off, out_len, index, torch.tensor([r[0] for r in reqs], dtype=torch.int32, device="cuda"),
                                                        H.dev([r[1] for r in reqs]), H.dev([r[2] for r in reqs]))
    assert g_st.tolist() == [O.OK] * len(reqs)
    g = got.cpu().numpy()
    for (b, ro, rl), o, n in zip(reqs, g_off.tolist(), g_len.tolist()):
        assert g[o:o + n].tobytes() == blobs[b][ro:ro + rl]
    assert cd.frame_encode_seekable(data, H.dev(in_off), H.dev(lens), 4096, with_index=False)[5] is None
    with pytest.raises(ValueError):
        cd.frame_encode_seekable(data, H.dev(in_off), H.dev(lens), 65537)

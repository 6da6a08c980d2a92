"""Shared by the GPU tests of snp_frame_encode_buffers_batch / snp_frame_decode_buffers_batch (test_gpu_frame_buffers.py,
test_gpu_frame_buffers_stress.py): streams packed at odd offsets between canary bytes, output layouts, the single-stream device decode, the check
of a batch decode against the model, the oracle and the single call, and the content pools."""
import numpy as np
import torch

import frame_buffers_model as M
import oracle as O
from conftest import CORPUS, read_testdata

B = 65536
CANARY = 0xA5


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.int64))).cuda()


def pack(blobs, lead=1, gap=3):
    """Blobs at odd offsets with canary bytes between them: -> (device tensor, offsets, lengths)."""
    off, o = [], lead
    for x in blobs:
        off.append(o)
        o += len(x) + gap
    h = np.full(o + gap, CANARY, dtype=np.uint8)
    for x, p in zip(blobs, off):
        h[p:p + len(x)] = np.frombuffer(x, dtype=np.uint8)
    return torch.from_numpy(h).cuda(), np.array(off, dtype=np.int64), np.array([len(x) for x in blobs], dtype=np.int64)


def out_layout(caps, lead=3, gap=5):
    off, o = [], lead
    for c in caps:
        off.append(o)
        o += int(c) + gap
    return np.array(off, dtype=np.int64), o + gap


def outside_ranges(out, off, lens):
    mask = np.ones(len(out), dtype=bool)
    for o, n in zip(off, lens):
        mask[int(o):int(o) + int(n)] = False
    return out[mask]


def frame_cap(n):
    return 10 + 8 * ((n + B - 1) // B) + n


def nchunks(lens):
    return int(sum((int(n) + B - 1) // B for n in lens))


def encode(cd, blobs, max_chunks=None, caps=None):
    data, in_off, lens = pack(blobs)
    caps = np.array([frame_cap(int(n)) for n in lens], dtype=np.int64) if caps is None else np.asarray(caps, dtype=np.int64)
    out_off, total = out_layout(caps)
    out = torch.full((total,), CANARY, dtype=torch.uint8, device="cuda")
    mc = nchunks(lens) if max_chunks is None else max_chunks
    _, _, ol, st, res = cd.frame_encode_buffers(data, dev(in_off), dev(lens), out=out, out_off=dev(out_off), out_cap=dev(caps), max_chunks=mc)
    torch.cuda.synchronize()
    return out.cpu().numpy(), out_off, ol.cpu().numpy(), st.cpu().numpy(), res.cpu().tolist()


def decode(cd, streams, caps, max_chunks=None, max_spans=None):
    data, in_off, lens = pack(streams)
    caps = np.asarray(caps, dtype=np.int64)
    out_off, total = out_layout(caps)
    out = torch.full((max(total, 1),), CANARY, dtype=torch.uint8, device="cuda")
    ol, st, res = cd.frame_decode_buffers(data, dev(in_off), dev(lens), out, dev(out_off), dev(caps), max_chunks=max_chunks, max_spans=max_spans)
    torch.cuda.synchronize()
    h = out.cpu().numpy()
    assert (outside_ranges(h, out_off, caps) == CANARY).all(), "a write outside the output ranges"
    return h, out_off, ol.cpu().numpy(), st.cpu().numpy(), res.cpu().tolist()


def single_decode(cd, blob, cap, max_chunks=None):
    """snp_frame_decode_device on this stream alone: -> (status, out_len, bytes)."""
    framed = torch.from_numpy(np.frombuffer(blob, dtype=np.uint8).copy()).cuda() if blob else torch.empty(0, dtype=torch.uint8, device="cuda")
    out = torch.empty(cap, dtype=torch.uint8, device="cuda")
    r = cd.frame_decode(framed, len(blob), out, len(blob) // 8 + 1 if max_chunks is None else max_chunks).cpu().tolist()
    return int(r[1]), int(r[0]), out[:int(r[0])].cpu().numpy().tobytes()


def check_decode(cd, streams, caps, got, max_chunks=None, max_spans=None):
    h, out_off, ol, st, res = got
    need_spans = sum((len(x) + M.SPAN - 1) // M.SPAN for x in streams)
    ms = need_spans if max_spans is None else max_spans
    _, _, _, mres, _ = M.decode_plan(streams, caps, 1 << 32 if max_chunks is None else max_chunks, ms, with_verdict=False)
    assert res[0] == mres[0] and res[2] == mres[2] and res[3] == mres[3], (res, mres)
    assert res[1] == int(ol[st == O.OK].sum())
    for b, x in enumerate(streams):
        s_st, s_len, s_bytes = single_decode(cd, x, int(caps[b]))
        if max_chunks is None and max_spans is None:
            assert (st[b], ol[b]) == (s_st, s_len), f"stream {b}: batch {(st[b], ol[b])} single {(s_st, s_len)}"
        if st[b] == O.OK:
            assert (s_st, s_len) == (O.OK, ol[b])
            got_b = h[out_off[b]:out_off[b] + ol[b]].tobytes()
            assert got_b == s_bytes == O.frame_decode(x), f"stream {b}: bytes differ"


# ---- content ---------------------------------------------------------------------------------------------------------------------------------
def pool_bytes():
    html = read_testdata("html")
    corpus = b"".join(read_testdata(f) for f in CORPUS if f in ("alice29.txt", "kppkn.gtb", "geo.protodata", "fireworks.jpeg"))
    rng = np.random.default_rng(7)
    low = bytes(rng.integers(0, 4, 400000, dtype=np.uint8))
    rnd = rng.integers(0, 256, 400000, dtype=np.uint8).tobytes()
    return [html * 30, corpus, low, rnd]


def ragged(rng, n, maxlen):
    pools = pool_bytes()
    blobs = []
    for i in range(n):
        src = pools[i % 4]
        ln = int(rng.integers(0, maxlen))
        ln = min(ln, len(src))
        o = int(rng.integers(0, len(src) - ln + 1))
        blobs.append(src[o:o + ln])
    return blobs

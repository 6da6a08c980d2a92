"""snp_launch_crc32c (csrc/crc32c.hip), the routine every framed call shares, on each of its three kernels: the direct call
(snp_crc32c_batch) over every length residue and input alignment, at the range counts where the launch policy changes kernel and where the list
ends at each position of a wavefront's four ranges and a workgroup's sixteen (1); the same call captured into a graph and replayed (2); the
verifying form of the launch (expect / status) behind the batch frame decode, on foreign streams of ragged chunks, clean and corrupt, a wrong
stored CRC at each position of a wavefront's four alone, and under chunk bounds on either side of the kernel threshold (3); the
encoding form behind the chunked frame encode on ragged buffers (4); and single ranges of 2 GiB and more, whose byte offsets leave 32 bits (5).
Every comparison is exact against the C oracle (O.crc32c_batch, O.frame_decode) or the models built on it; every output array of a direct call
lies between guard elements.  SNP_OPT_CRC_KERNEL = 0 runs k_crc32c<2> (three LDS tables of 11 + 11 + 10 bits, four ranges per wavefront) from
crc_cases.THREE_TABLE_MIN ranges on and k_crc32c<0> (four 8-bit tables) below; 1 runs k_crc32c<1> (no table), 2 k_crc32c<0>.  Bytes cannot
show which kernel ran: profiles/r15a_crc_kernels.csv is the kernel trace of this file, with all three instantiations in it.  The ranges:
crc_cases.py (checked without a GPU by test_crc_cases.py).  Needs an MI355X."""
import functools

import numpy as np
import pytest
import torch

import crc_cases as CC
import frame_buffers_helpers as H
import oracle as O
from seekable_harness import CANARY, GUARD, Encoded, Guarded, _p

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    import snappier_amd as S
    from snappier_amd import batch as SB, _native as N

KERNELS = [0, 1, 2]
T = CC.THREE_TABLE_MIN
UNTOUCHED = int.from_bytes(bytes([CANARY]) * 4, "little")


def codec(kernel=0):
    cd = SB.BlockCodec(0, O.HASH_CRC32C)
    cd.ctx.set_option(N.OPT_CRC_KERNEL, kernel)
    assert cd.ctx.get_option(N.OPT_CRC_KERNEL) == kernel
    return cd


def crc_call(cd, data, in_off, in_len, nblocks, masked, out):
    """snp_crc32c_batch called directly: only enqueues."""
    cd._bind()
    assert cd.ctx.lib.snp_crc32c_batch(cd.ctx.handle, _p(data), _p(in_off), _p(in_len), nblocks, int(masked), out.ptr()) == O.OK


def read_crcs(out, nblocks):
    """The first nblocks elements; the guards and every element past nblocks must have kept their canary."""
    h = out.t.cpu().numpy().view(np.uint32)
    assert (h[:GUARD] == UNTOUCHED).all() and (h[GUARD + nblocks:] == UNTOUCHED).all(), "a write outside the first nblocks CRCs"
    return h[GUARD:GUARD + nblocks]


def same_crcs(got, want, what):
    bad = np.nonzero(got != want)[0]
    off, ln, _ = CC.ranges()
    assert bad.size == 0, (what, bad.size, [(int(k), int(ln[k]), int(off[k]) % 16, hex(got[k]), hex(want[k])) for k in bad[:8]])


# ---- 1. every length, alignment and prefix, on every kernel --------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def device_ranges():
    off, ln, _ = CC.ranges()
    return torch.from_numpy(off.astype(np.int64)).cuda(), torch.from_numpy(ln.view(np.int32).copy()).cuda()


@functools.lru_cache(maxsize=None)
def device_contents(name):
    return torch.from_numpy(CC.contents()[name].copy()).cuda()


@pytest.mark.parametrize("kernel", KERNELS)
def test_every_length_alignment_and_list_end(kernel):
    """Under option 0 the first prefix runs the 8-bit tables and every other one the three tables; options 1 and 2 run one kernel throughout."""
    cd = codec(kernel)
    in_off, in_len = device_ranges()
    out = Guarded(CC.COUNT, torch.int32)
    for name in ("random", "zeros"):
        data = device_contents(name)
        for masked in (False, True):
            want = CC.expected(name, masked)
            for n in CC.PREFIXES:
                out.t.view(torch.uint8).fill_(CANARY)
                crc_call(cd, data, in_off, in_len, n, masked, out)
                torch.cuda.synchronize()
                same_crcs(read_crcs(out, n), want[:n], (kernel, name, masked, n))


# ---- 2. capture and replay -----------------------------------------------------------------------------------------------------------------------
def test_the_direct_call_replays_from_a_graph():
    """include/snappier_hip.h lists snp_crc32c_batch among the calls that only enqueue: the T + 5 call (the three-table kernel, the list ending
    one range into a wavefront's four), masked and unmasked, captured once and replayed on the other contents and back."""
    n = T + 5
    cd = codec(0)
    in_off, in_len = device_ranges()
    data = device_contents("random").clone()
    outs = {masked: Guarded(CC.COUNT, torch.int32) for masked in (False, True)}

    def call():
        for masked, out in outs.items():
            crc_call(cd, data, in_off, in_len, n, masked, out)

    def check(name):
        torch.cuda.synchronize()
        for masked, out in outs.items():
            same_crcs(read_crcs(out, n), CC.expected(name, masked)[:n], (name, masked))
            out.t.view(torch.uint8).fill_(CANARY)

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        call()
    torch.cuda.current_stream().wait_stream(s)
    check("random")
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        call()
    for name in ("zeros", "random", "zeros"):
        data.copy_(device_contents(name))
        torch.cuda.synchronize()
        g.replay()
        check(name)
    data.copy_(device_contents("random"))                               # and outside the graph again
    call()
    check("random")


# ---- 3. the verifying launch, on foreign streams -------------------------------------------------------------------------------------------------
def decode_against_the_oracle(cd, streams, caps, want, max_chunks=None):
    got = H.decode(cd, streams, caps, max_chunks=max_chunks)            # (asserts that nothing is written outside the output ranges)
    H.check_decode(cd, streams, caps, got, max_chunks=max_chunks)
    h, out_off, ol, st, _ = got
    for b, (status, raw) in enumerate(want):
        assert st[b] == status and ol[b] == (len(raw) if status == O.OK else 0), (b, st[b], status, ol[b])
        if status == O.OK:
            assert h[out_off[b]:out_off[b] + ol[b]].tobytes() == raw, b
    return got


@pytest.mark.parametrize("kernel", KERNELS)
def test_the_verifying_launch_on_foreign_streams(kernel):
    streams, caps, want = CC.foreign_batch()
    got = decode_against_the_oracle(codec(kernel), streams, caps, want)
    assert got[4][0] >= T + 5                                           # chunk slots: under option 0 the three-table kernel verifies them


@pytest.mark.parametrize("chunk", CC.BAD_CRC)
def test_one_bad_crc_alone_at_each_position_of_a_group_of_four(chunk):
    """The three-table kernel's wavefront verifies four slots in a row: one wrong CRC at each of the four positions, and in the last chunk."""
    streams, caps, want = CC.single_bad_crc_batch(chunk)
    h, out_off, ol, st, res = H.decode(codec(0), streams, caps)
    assert res[0] >= T + 5 and st.tolist() == [s for s, _ in want] and st[5] == O.ERR_CRC_MISMATCH
    assert ol.tolist() == [len(raw) if s == O.OK else 0 for s, raw in want]


@pytest.mark.parametrize("kernel", KERNELS)
def test_a_loose_chunk_bound_crosses_the_kernel_threshold_and_changes_nothing(kernel):
    """The verifying launch runs over max_chunks slots, real or not: 40 real chunks under bounds on either side of the threshold."""
    streams, caps, want = CC.small_batch()
    cd = codec(kernel)
    exact = decode_against_the_oracle(cd, streams, caps, want, max_chunks=40)
    for bound in (T - 1, T):
        got = decode_against_the_oracle(cd, streams, caps, want, max_chunks=bound)
        assert np.array_equal(got[0], exact[0]) and np.array_equal(got[2], exact[2]) and np.array_equal(got[3], exact[3]) and got[4] == exact[4], bound


# ---- 4. the encoding launch, ragged --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel", KERNELS)
def test_the_encoding_launch_on_ragged_chunks(kernel):
    """snp_frame_encode_chunked_batch (what frame_encode_seekable calls) with every array guarded: streams and index equal the model's."""
    blobs, want = CC.ragged_buffers()
    assert len(blobs) == 64 and want["result"][0] == T + 3 and want["status"] == [O.OK] * 64
    got = Encoded(codec(kernel), blobs, CC.CHUNK).got
    for key in want:
        assert got[key] == want[key], key


# ---- 5. single ranges of 2 GiB and more ----------------------------------------------------------------------------------------------------------
BIG = (1 << 32) + 64
BIG_RANGES = [(3, (1 << 31) - 1), (1, (1 << 31) + 1029), (0, (1 << 32) - 1)]      # (in_off, length)
EMPTY_MASKED = 0xA282EAD8                                                          # the masked CRC of no bytes


def test_single_ranges_of_2_gib_and_more():
    """A lane's byte offset inside a range passes 2^31, and n + pad reaches 2^32: the three ranges side by side in one call, lengths as the
    uint32 bit pattern.  Unmasked as a list of three (k_crc32c<0>); masked as ranges 0, 4 and 8 -- a wavefront each -- of a list of
    THREE_TABLE_MIN whose other ranges are empty (k_crc32c<2>); and the host call on the 2^31 + 1029 range with the table-free kernel.
    One wavefront reads 1.9 GB/s (1.35 GB/s table-free): 2.3 s for the longest range."""
    import psutil
    free = torch.cuda.mem_get_info()[0]
    if free < BIG + (4 << 30):
        pytest.skip(f"needs {(BIG + (4 << 30)) >> 30} GiB of free device memory, {free >> 30} GiB free")
    if psutil.virtual_memory().available < (16 << 30):
        pytest.skip("needs ~8 GiB of host memory")
    gen = torch.Generator(device="cuda").manual_seed(1514)
    data = torch.empty(BIG, dtype=torch.uint8, device="cuda")
    for o in range(0, BIG, 1 << 30):
        data[o:o + (1 << 30)].random_(0, 256, generator=gen)
    off = np.zeros(T, dtype=np.uint64)
    ln = np.zeros(T, dtype=np.uint32)
    off[0:12:4], ln[0:12:4] = [o for o, _ in BIG_RANGES], [n for _, n in BIG_RANGES]
    cd = codec(0)
    tables = {3: (torch.from_numpy(off[0:12:4].astype(np.int64)).cuda(), torch.from_numpy(ln[0:12:4].view(np.int32).copy()).cuda()),
              T: (torch.from_numpy(off.astype(np.int64)).cuda(), torch.from_numpy(ln.view(np.int32).copy()).cuda())}
    outs = {3: Guarded(3, torch.int32), T: Guarded(T, torch.int32)}
    for count, out in outs.items():
        crc_call(cd, data, *tables[count], count, count == T, out)      # (they run while the host copies and the oracle works)
    host = data.cpu().numpy()
    want = {masked: O.crc32c_batch(host, off[0:12:4], ln[0:12:4], masked, threads=3) for masked in (False, True)}
    torch.cuda.synchronize()
    got = read_crcs(outs[3], 3)
    assert got.tolist() == want[False].tolist(), ([hex(x) for x in got], [hex(x) for x in want[False]])
    got = read_crcs(outs[T], T)
    assert got[0:12:4].tolist() == want[True].tolist(), ([hex(x) for x in got[0:12:4]], [hex(x) for x in want[True]])
    rest = np.ones(T, dtype=bool)
    rest[0:12:4] = False
    assert (got[rest] == EMPTY_MASKED).all()
    o, n = BIG_RANGES[1]
    assert S.crc32c(host[o:o + n], masked=True, ctx=codec(1).ctx) == int(want[True][1])

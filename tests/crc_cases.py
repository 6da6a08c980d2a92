"""The byte ranges of the CRC-32C kernel tests (test_gpu_crc32c_kernels.py; checked for what they claim, without a GPU and without torch, by
test_crc_cases.py): one list of ranges that holds every length 0 .. 2100 (every residue mod 1024 in ranges of one, two and three 1 KiB rows,
so the two-row prefetch is met on both sides) and the lengths around 3, 4, 5 and 64 KiB at every one of the 16 values of in_off % 16, over two
content buffers; and the prefixes of that list at which the launch policy of csrc/crc32c.hip changes kernel and at which the list ends at each
position of a wavefront's group of four ranges and of a workgroup's sixteen.  Then the framed streams of ragged chunks, clean and faulty, for the
verifying launch, and the ragged buffers for the encoding launch."""
import functools

import numpy as np

import frame_buffers_model as M
import frame_chunked_model as K
import kats
import oracle as O
import seekable_cases as SC
import stream_grammar as G
from conftest import read_testdata

# Below this many byte ranges SNP_OPT_CRC_KERNEL = 0 runs the four 8-bit tables (k_crc32c<0>), from it on the three tables of 11 + 11 + 10 bits
# (k_crc32c<2>).  Owner: snp_launch_crc32c, csrc/crc32c.hip:240 (`nblocks < 16u * 256u * kWaves11`); no option states it, so this copy is kept in
# step by hand, like layouts.COMPRESS_TIERS.
THREE_TABLE_MIN = 16 * 256 * 4
PER_WAVEFRONT, PER_WORKGROUP = 4, 16       # ranges a wavefront / a workgroup of k_crc32c<2> takes (kPer11, kPer11 * kWaves11)

LENGTHS = list(range(2101)) + [3071, 3072, 3073, 4095, 4096, 4097, 5119, 5120, 5121, 65535, 65536, 65537, 70000]
ALIGNMENTS = 16
COUNT = len(LENGTHS) * ALIGNMENTS          # 33 824 ranges
STEP = 131                                 # the lengths of one group of 16 ranges lie this far apart in LENGTHS: short and long ones side by side
# The prefixes of the list that the GPU tests run: the last count on the 8-bit tables, the first on the three tables, then a list that ends at
# each position of a wavefront's four (+1, +3, +4, +5) and inside a workgroup's sixteen (+15), and the whole list.
PREFIXES = [THREE_TABLE_MIN - 1, THREE_TABLE_MIN, THREE_TABLE_MIN + 1, THREE_TABLE_MIN + 3, THREE_TABLE_MIN + 4, THREE_TABLE_MIN + 5,
            THREE_TABLE_MIN + 15, COUNT]
SEED = 1511


def length_of(k: int) -> int:
    """Range k = 16 q + a lies at in_off % 16 == a and has length LENGTHS[(q + STEP a) % len]: for each a, q walks every length once, and the
    lengths cycle, so every prefix of 16 q ranges holds q lengths at every alignment."""
    q, a = divmod(k, ALIGNMENTS)
    return LENGTHS[(q + STEP * a) % len(LENGTHS)]


@functools.lru_cache(maxsize=None)
def ranges():
    """-> (in_off uint64[COUNT], in_len uint32[COUNT], bytes the buffer needs): the ranges in list order, 1 .. 16 bytes apart."""
    off = np.zeros(COUNT, dtype=np.uint64)
    ln = np.array([length_of(k) for k in range(COUNT)], dtype=np.uint32)
    pos = 0
    for k in range(COUNT):
        pos += 1 + (k % ALIGNMENTS - (pos + 1)) % ALIGNMENTS            # the next offset past pos with offset % 16 == k % 16
        off[k] = pos
        pos += int(ln[k])
    off.setflags(write=False)
    ln.setflags(write=False)
    return off, ln, pos + 16


@functools.lru_cache(maxsize=None)
def kat_ranges():
    """[(range, bytes, CRC)]: the first range of the list of each KAT's length, for three of kats.CRC32C (lengths 9, 16 and 30)."""
    _, ln, _ = ranges()
    return [(int(np.nonzero(ln == len(data))[0][0]), data, crc) for data, crc in kats.CRC32C[:3]]


@functools.lru_cache(maxsize=None)
def contents():
    """-> {"random": seeded random bytes with the three KATs written into their ranges, "zeros": all zeros -- there a CRC depends on the length
    alone, so a range taken one byte long or short, or at the wrong place, shows}."""
    off, _, size = ranges()
    rnd = np.random.default_rng(SEED).integers(0, 256, size, dtype=np.uint8)
    for k, data, _ in kat_ranges():
        rnd[int(off[k]):int(off[k]) + len(data)] = np.frombuffer(data, dtype=np.uint8)
    zeros = np.zeros(size, dtype=np.uint8)
    rnd.setflags(write=False)
    zeros.setflags(write=False)
    return {"random": rnd, "zeros": zeros}


@functools.lru_cache(maxsize=None)
def expected(name: str, masked: bool):
    """The oracle's CRC of every range of one content buffer (computed once, shared, read-only)."""
    off, ln, _ = ranges()
    want = O.crc32c_batch(contents()[name], off, ln, masked)
    want.setflags(write=False)
    return want


# ---- framed streams for the verifying launch: 1 .. 2100-byte chunks, both chunk types, foreign bodies ---------------------------------------------
ID = M.STREAM_ID
PER_STREAM = 2050                                                      # data chunks per stream: eight streams hold 16 400 >= THREE_TABLE_MIN + 5
GRAMMAR_EVERY = 16                                                     # every sixteenth chunk's body is a grammar-built stream (stream_grammar.build)
BAD_CRC = (100, 101, 102, 103, PER_STREAM - 1)                         # four neighbours: every position of a group of four, wherever the stream's slots start
CORRUPT_AT = 1001


@functools.lru_cache(maxsize=None)
def _pools():
    corpus = read_testdata("html") + read_testdata("alice29.txt")
    return corpus, np.random.default_rng(1512).integers(0, 256, 1 << 20, dtype=np.uint8).tobytes()


@functools.lru_cache(maxsize=None)
def pairs(seed, count):
    """count chunks as stream_grammar.framed takes them, (body, raw) with body None for an uncompressed chunk: 1 .. 2100 bytes each, corpus
    and random bytes, types 0x00 and 0x01 mixed; the compressed bodies are the oracle's and, every sixteenth, a grammar-built foreign one."""
    corpus, rnd = _pools()
    rng = np.random.default_rng(seed)
    out = []
    for k in range(count):
        n = int(rng.integers(1, 2101))
        if k % GRAMMAR_EVERY == 3:
            out.append(G.build(seed * 100000 + k, n, G.PROFILES[(k // GRAMMAR_EVERY) % len(G.PROFILES)])[:2])
            continue
        src = rnd if k % 3 == 1 else corpus
        o = int(rng.integers(0, len(src) - n))
        raw = src[o:o + n]
        out.append((None, raw) if k % 8 in (1, 5) else (O.compress(raw), raw))
    return tuple(out)


def clean_stream(chunks):
    """The identifier and one chunk per pair: frame_buffers_model.data_chunk's for the oracle's bodies and the raw chunks, stream_grammar.framed's
    for a foreign body."""
    out = [ID]
    for k, (body, raw) in enumerate(chunks):
        out.append(G.framed([(body, raw)])[len(ID):] if k % GRAMMAR_EVERY == 3 else M.data_chunk(raw, compressed=body is not None))
    return b"".join(out)


def corrupt_pair(seed, n):
    """A compressed chunk whose body does not decode (a copy that reaches before the start of the output) under the CRC of what it was built for."""
    stream, raw, tags = G.build(seed, n, "uniform")
    bad = G.mutate(stream, tags, "offset-past")
    assert bad is not None and O.decompress_status(bad, n) not in (O.OK, O.ERR_CRC_MISMATCH)
    return bad, raw


def faulty_streams(seed, count, bad_crc, corrupt_at):
    """-> three streams of `count` data chunks each: stored CRCs off by a bit in the chunks bad_crc; one compressed chunk with a corrupt body;
    and a chunk too short to hold a CRC (3 body bytes) followed by a chunk with a bad CRC, both behind count - 1 sound chunks."""
    a, b, c = pairs(seed, count), list(pairs(seed + 1, count)), pairs(seed + 2, count)
    b[corrupt_at] = corrupt_pair(seed, 1500)
    short_then_bad = G.framed(c[:-1]) + M.chunk(0x01, b"abc") + G.framed(c[-1:], bad_crc=(0,))[len(ID):]
    return [G.framed(a, bad_crc=bad_crc), G.framed(b), short_then_bad], [a, b, c]


@functools.lru_cache(maxsize=None)
def foreign_batch():
    """-> (eight streams, capacities, the oracle's (status, bytes or None) per stream): five clean, then faulty_streams."""
    clean = [pairs(10 + b, PER_STREAM) for b in range(5)]
    faulty, faulty_pairs = faulty_streams(20, PER_STREAM, BAD_CRC, CORRUPT_AT)
    streams = [clean_stream(c) for c in clean] + faulty
    caps = [sum(len(raw) for _, raw in c) + b % 3 for b, c in enumerate(clean + faulty_pairs)]
    return streams, caps, [oracle_verdict(s) for s in streams]


@functools.lru_cache(maxsize=None)
def small_batch():
    """Five streams of 40 data chunks in all, the three faulty kinds among them."""
    faulty, faulty_pairs = faulty_streams(30, 7, (1, 6), 3)
    clean = [pairs(40, 12), pairs(41, 8)]
    streams = [clean_stream(clean[0]), faulty[0], faulty[1], clean_stream(clean[1]), faulty[2]]
    caps = [sum(len(raw) for _, raw in c) + 1 for c in (clean[0], faulty_pairs[0], faulty_pairs[1], clean[1], faulty_pairs[2])]
    return streams, caps, [oracle_verdict(s) for s in streams]


@functools.lru_cache(maxsize=None)
def single_bad_crc_batch(k: int):
    """foreign_batch with the stored CRC wrong in chunk k of the sixth stream and nowhere else: among BAD_CRC together a miss at one position of
    a group of four hides behind the others."""
    streams, caps, want = foreign_batch()
    s = G.framed(pairs(20, PER_STREAM), bad_crc=(k,))
    return streams[:5] + [s] + streams[6:], caps, want[:5] + [oracle_verdict(s)] + want[6:]


def oracle_verdict(s):
    try:
        return O.OK, O.frame_decode(s)
    except O.OracleError as e:
        return e.status, None


# ---- buffers for the encoding launch --------------------------------------------------------------------------------------------------------------
CHUNK = 1000


@functools.lru_cache(maxsize=None)
def ragged_buffers():
    """64 buffers whose 1 000-byte chunks number exactly THREE_TABLE_MIN + 3: the CRC launch of the encode ends three ranges into a wavefront's four."""
    rng = np.random.default_rng(1513)
    lens = [0, 1, CHUNK - 1, CHUNK, CHUNK + 1] + [int(x) for x in rng.integers(60_000, 400_000, 58)]
    left = THREE_TABLE_MIN + 3 - sum(K.nchunks(n, CHUNK) for n in lens)
    assert left > 1
    lens.append(left * CHUNK - 137)
    blobs = [SC.content(n, CHUNK, 40 + b) for b, n in enumerate(lens)]
    return blobs, K.encode(blobs, CHUNK, O.HASH_CRC32C)

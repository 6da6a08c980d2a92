"""Deterministic batches for the tier tests of the seekable-stream calls (test_gpu_seekable_tiers.py; checked for what they claim, without a
GPU, by test_seekable_cases.py): corpus bytes spliced with random and constant runs, so that every batch holds compressed AND raw chunks; the
request lists of each call; the launch thresholds as capi_internal.h sets them; and the arithmetic that stands in for the models where those
are too slow (frame_update_model.write_plan takes minutes from ten thousand slots on)."""
import functools

import numpy as np

import frame_chunked_model as K
import frame_range_model as R
import frame_update_model as U
from conftest import read_testdata

# The defaults of csrc/capi_internal.h.  The GPU tests never use these numbers: they read each threshold from the context (get_option) and
# assert once that the defaults still are these; the CPU test uses them to place the batches' slot counts.
WIN_DUAL_MIN, WIN_GLOBAL_MIN, WIN_MAX, SMALL_MIN_BATCH, SLICE = 1536, 4096, 32768, 4096, 262144
# The lane compressor's launch shape changes at these fragment counts.  No option states them: they are the policy of
# csrc/compress_lanes.hip as the comment over layouts.COMPRESS_TIERS records it (below 8 192, 8 192 .. 32 767, 32 768 .. 131 071, from 131 072).
LANE_TIERS = (8192, 32768, 131072)
COUNT_PAIRS = [(64, WIN_MAX + 1000), (256, 10000), (1000, 3000), (4096, 1600)]      # (chunk_bytes, real slots at least)
# The hint sequences (count_batch of each): chunked encodes on the lane compressor whose longest fragments walk its hint through every
# transition, and indexed reads of hint_rows() interior rows whose mean row size walks the decoder's.
COMPRESS_SEQUENCE = [(64, 3000), (300, 3000), (700, 3000), (4096, 3000), (96, 3000), (65536, 64), (256, 3000)]
DECODE_SEQUENCE = [32, 100, 400, 65536]


def hint_rows(small_min_batch: int) -> int:
    """Interior rows of a decoder hint batch: just past the batch size from which the decoder takes the small-block pre-pass."""
    return small_min_batch + 4


@functools.lru_cache(maxsize=None)
def _pools():
    corpus = read_testdata("html") + read_testdata("alice29.txt")[:150000] + read_testdata("geo.protodata")
    rnd = np.random.default_rng(77).integers(0, 256, 1 << 20, dtype=np.uint8).tobytes()
    return corpus, rnd


@functools.lru_cache(maxsize=None)
def content(n: int, cb: int, seed: int) -> bytes:
    """n bytes: runs of corpus bytes, of random bytes (2 .. 4 chunks long, so that whole chunks of them stay raw) and of one constant byte."""
    corpus, rnd = _pools()
    rng = np.random.default_rng(seed * 1000003 + cb)
    out, have, kind = [], 0, int(rng.integers(0, 3))
    while have < n:
        if kind == 1:
            ln = int(rng.integers(2 * cb, 4 * cb + 2))
            o = int(rng.integers(0, len(rnd) - ln))
            run = rnd[o:o + ln]
        else:
            ln = int(rng.integers(cb // 2 + 1, 2 * cb + 2))
            o = int(rng.integers(0, len(corpus) - ln))
            run = corpus[o:o + ln] if kind == 0 else bytes([int(rng.integers(0, 256))]) * ln
        out.append(run)
        have += ln
        kind = (kind + 1) % 3
    return b"".join(out)[:n]


# Chunk sizes at which the emit kernels of the rewrite calls (update, append, splice, rechunk, compose) run teams of 64, 128 and 256 threads
# (frame_chunked_device.h: fc_team(fc_group(cb))).
TEAM_CHUNK_SIZES = [1000, 32768, 65536]


@functools.lru_cache(maxsize=None)
def team_blobs(cb: int):
    """Three buffers of at most four chunks for the rewrite calls' team-size cases: random bytes (every chunk stays raw, tail of 7 bytes), a
    repeated 64-byte pattern (every chunk compresses, no short tail) and corpus bytes (a short tail)."""
    corpus, rnd = _pools()
    pattern = bytes(range(64, 128))
    return [rnd[11:11 + 3 * cb + 7], (pattern * (4 * cb // 64 + 1))[:4 * cb], corpus[:2 * cb + cb // 3]]


def chunk_types(stream: bytes):
    """The types of the non-empty data chunks of a framed stream: 0 compressed, 1 raw."""
    return {r[0] for r in R.walk(stream)[0] if r[5] > 0}


def windows(n: int, cb: int):
    """(offset, length): on a chunk boundary, one byte either side of it, inside one chunk, across three chunks, at the tail -- and past it."""
    return [(cb, cb), (cb - 1, 2), (1, max(cb - 2, 1)), (cb // 2, 2 * cb + (cb == 1)), (max(n - cb - 1, 0), cb + 5), (n, 3), (0, 1 << 62)]


class Batch:
    """blobs: what is encoded.  reads: (stream, off, len) for the indexed read; ranges: one (off, len) per stream of decode_streams() for the
    range decode; writes: (stream, off, len), sorted and disjoint, for the indexed write (write_srcs(): their bytes)."""

    def __init__(self, cb, blobs, reads, ranges, writes):
        self.cb, self.blobs, self.reads, self.ranges, self.writes = cb, blobs, reads, ranges, writes

    def slots(self) -> int:
        return sum(K.nchunks(len(x), self.cb) for x in self.blobs)

    @functools.lru_cache(maxsize=None)
    def streams(self, variant: int):
        return [K.stream_of(x, self.cb, variant) for x in self.blobs]

    def write_srcs(self, seed: int = 0):
        rng = np.random.default_rng(seed)
        return [U.fresh(rng, ln) for _, _, ln in self.writes]


CORRUPT_CHUNK = 2          # of small_batch's last stream, in the copy decode_streams() appends


@functools.lru_cache(maxsize=None)
def small_batch(cb: int) -> Batch:
    """Six streams of 0, 1, cb - 1, cb + 1, 3 cb + 7 and 40 cb + 3 bytes.  The decode calls get a seventh (decode_streams): the last one with
    chunk CORRUPT_CHUNK corrupted, so that requests which meet that chunk fail and every other one is served."""
    lens = [0, 1, cb - 1, cb + 1, 3 * cb + 7, 40 * cb + 3]
    blobs = [content(n, cb, 10 + b) for b, n in enumerate(lens)]
    n7 = lens + [lens[-1]]
    reads = [(b, ro, rl) for b, n in enumerate(n7) for ro, rl in windows(n, cb)]
    reads += [(4, cb, 0), (6, CORRUPT_CHUNK * cb + 1, 2), (6, CORRUPT_CHUNK * cb - 1, cb + 2), (6, (CORRUPT_CHUNK + 1) * cb, cb)]
    ranges = [windows(n, cb)[b % 7] for b, n in enumerate(lens)] + [(CORRUPT_CHUNK * cb - 1, 3)]
    shape = [8, 9, 0, 2, 5, 2]
    writes = [(b, off, ln) for b, n in enumerate(lens) for off, ln in U.request_shapes(n, cb)[shape[b]] if n or not ln]
    writes += [(5, 30 * cb + 1, 0), (6, 3, 2), (6, CORRUPT_CHUNK * cb + 1, 2)]   # a zero-length request; an edge in the corrupt chunk
    return Batch(cb, blobs, reads, ranges, writes)


def decode_streams(batch: Batch, variant: int):
    """The batch's streams plus the corrupt copy of the last one."""
    s = batch.streams(variant)
    rows = R.walk(s[-1])[0]
    return s + [R.corrupt_chunk(s[-1], rows[CORRUPT_CHUNK])]


@functools.lru_cache(maxsize=None)
def count_batch(cb: int, slots: int) -> Batch:
    """One long stream of `slots` chunks (the last one short) and a ragged tail of short ones.  reads: one window (k cb - 1, 3) across every
    chunk boundary of the long stream, one whole-chunk window per chunk and four requests on the corrupt copy of the last stream
    (decode_streams); ranges: one window per stream, the corrupt copy's across its corrupt chunk; writes: the whole long stream."""
    tail = [0, 1, cb - 1, cb, cb + 1, 2 * cb + 3, 7, 0, 5 * cb - 1]
    n = slots * cb - 5
    blobs = [content(n, cb, 1)] + [content(t, cb, 20 + i) for i, t in enumerate(tail)]
    bad = len(blobs)                                                    # the corrupt copy decode_streams() appends
    reads = [(0, k * cb - 1, 3) for k in range(1, slots)] + [(0, k * cb, cb) for k in range(slots)]
    reads += [(bad, CORRUPT_CHUNK * cb - 1, 3), (bad, CORRUPT_CHUNK * cb + 5, 2), (bad, 0, cb), (bad, cb, 0)]
    ranges = [(0, 1 << 62)] + [windows(t, cb)[i % 7] for i, t in enumerate(tail)] + [(CORRUPT_CHUNK * cb - 1, 3)]
    return Batch(cb, blobs, reads, ranges, [(0, 0, n)])


def boundary_writes(batch: Batch, corrupt: bool = False):
    """One 3-byte request across every second chunk boundary of the longest stream: every dirty chunk is an edge.  corrupt: and one across the
    corrupt chunk of the stream decode_streams() appends, which fails that stream alone."""
    cb = batch.cb
    b = max(range(len(batch.blobs)), key=lambda i: len(batch.blobs[i]))
    reqs = [(b, k * cb - 1, 3) for k in range(1, K.nchunks(len(batch.blobs[b]), cb), 2)]
    return reqs + [(len(batch.blobs), CORRUPT_CHUNK * cb - 1, 3)] if corrupt else reqs


# ---- arithmetic in place of the models, for streams of whole chunks that are all sound -----------------------------------------------------------
def read_needs(lens, cb: int, reads):
    """What frame_index_model.read_plan gives as d_result for requests that are all served, over streams K.stream_of made:
    -> [interior slots, bytes delivered, edge scratch bytes, requests]."""
    slots = edge = total = 0
    for b, ro, rl in reads:
        n = lens[b]
        lo, hi = R.clip(n, ro, rl)
        total += hi - lo
        if hi <= lo:
            continue
        r0, r1 = lo // cb, (hi + cb - 1) // cb
        head = r0 * cb < lo
        last = min(r1 * cb, n) > hi and not (head and r1 - 1 == r0)
        slots += r1 - r0 - head - last
        edge += (min(cb, n - r0 * cb) if head else 0) + (min(cb, n - (r1 - 1) * cb) if last else 0)
    return [slots, total, edge, len(reads)]


def write_needs(lens, cb: int, writes):
    """d_result[0] and [2] of the indexed write for sorted, disjoint, non-empty requests that are all served: -> (dirty slots, staging bytes)."""
    dirty = {}
    for b, off, ln in writes:
        if ln:
            dirty.setdefault(b, set()).update(range(off // cb, (off + ln - 1) // cb + 1))
    return sum(len(v) for v in dirty.values()), sum(min(cb, lens[b] - k * cb) for b, v in dirty.items() for k in v)

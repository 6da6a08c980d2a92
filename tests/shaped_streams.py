"""Well-formed Snappy streams shaped to drive the tag index of a large block (csrc/tag_index_device.h) to a known decision -- shared by the CPU
model test (tests/test_tag_index_model.py) and the device tests of the batched call (tests/test_gpu_buffers_stress.py).  Every stream is below
8 MiB of input, so the single-block path indexes it in one piece.

  S1  low-entropy, 3 MiB                                   candidates suffice: no fix pass, no look-back
  S2  corpus_bytes(1 000 000)                              one incompressible region (the jpeg): one fix pass resolves it
  S3  random, 4 MiB                                        the stream is >= 85 % of its output: the look-back pass, set up front
  S4  low-entropy, 2 MiB, one 40 KiB random region         the literal jumps over more than one chunk: one fix pass resolves it
  S5  as S4, three regions 512 KiB apart                   fewer than 834 chunks allow one fix pass; the second region's landing is still
                                                           pending after it, so the scan gives up: the look-back pass (not the 85 % rule)
"""
from functools import lru_cache

import numpy as np

import datagen
import oracle as O
from conftest import CORPUS, read_testdata

SHAPES = ["S1", "S2", "S3", "S4", "S5"]
LOOK_BACK = {"S1": 0, "S2": 0, "S3": 1, "S4": 0, "S5": 1}       # the decision each shape is built for (read from the code)


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


def with_random_regions(n: int, starts, region: int, seed: int) -> bytes:
    """Low-entropy bytes with a random region of `region` bytes at each of `starts` (each inside one 64 KiB fragment of the compressor, so
    it becomes one literal longer than a 16 KiB chunk of the stream)."""
    a = bytearray(low_entropy_bytes(n, seed))
    for i, at in enumerate(starts):
        a[at:at + region] = random_bytes(region, seed + 100 + i)
    return bytes(a)


@lru_cache(maxsize=None)
def raw(name: str) -> bytes:
    if name == "S1":
        return low_entropy_bytes(3 << 20, 11)
    if name == "S2":
        return corpus_bytes(1_000_000)
    if name == "S3":
        return random_bytes(4 << 20, 3)
    if name == "S4":
        return with_random_regions(2 << 20, [(1 << 20) + 8192], 40 << 10, 21)
    if name == "S5":
        return with_random_regions(2 << 20, [(k << 19) + 8192 for k in (1, 2, 3)], 40 << 10, 21)
    raise ValueError(name)


@lru_cache(maxsize=None)
def stream(name: str) -> bytes:
    return O.compress(raw(name), O.HASH_CRC32C)


def preamble_bytes(s: bytes) -> int:
    hb = 1
    while s[hb - 1] & 0x80:
        hb += 1
    return hb


def look_back_only(s: bytes, declared: int) -> bool:
    """snp_tag_index_look_back_only: a stream of >= 85 % of its output goes to the look-back pass without a scan."""
    return len(s) * 100 >= declared * 85

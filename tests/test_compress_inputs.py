"""The compressor tests' inputs (tests/compress_inputs.py), checked on the CPU: the fuzz generator is pinned, the tracer is held to the oracle on
everything it is used on, the directed set shows every event class, and the window compressor's CPU model already reproduces the oracle on
it.  Also writes the census of the fuzz rounds and the directed set (profiles/r13a_compress_input_census.json): how often each class occurs
where -- a record of what the GPU tests compare, not a threshold."""
import functools
import hashlib
import json
import os

import numpy as np
import pytest

import oracle as O
from conftest import ROOT, read_testdata
import compress_inputs as CI
import window_model as WM

VARIANTS = [O.HASH_CRC32C, O.HASH_MUL]
WORKERS = max(1, min(os.cpu_count() or 1, 8))
FUZZ_BLOCKS = 768


def fuzz_seeds(variant):
    """The seeds of test_fuzz_compress_bytes_equal_oracle's two rounds with layout lanes (FUZZ_SEED unset)."""
    return [1000 * r + 17 * variant + 1 for r in range(2)]


def _text():
    return np.frombuffer(read_testdata("html") + read_testdata("alice29.txt"), dtype=np.uint8)


def test_make_block_sequences_are_pinned():
    """sha256 over (length, bytes) of the first 64 blocks of seeds 0 and 17, computed from test_gpu_fuzz.py's make_block before it moved to
    compress_inputs.py: the seeds in profiles/*fuzz_log* keep their meaning."""
    want = {0: "2a48cb53fb4d555a7ed10f57cee58d655e3406811906b7dcfdcf95ce25db774d",
            17: "7113721d4f169cb6447468af460581ae8db0d765ea3680cc3dca0e7c6bae60c9"}
    text = _text()
    for seed, digest in want.items():
        rng = np.random.default_rng(seed)
        h = hashlib.sha256()
        for _ in range(64):
            b = CI.make_block(rng, text)
            h.update(len(b).to_bytes(4, "little"))
            h.update(b.tobytes())
        assert h.hexdigest() == digest, seed
    assert CI.EDGE_LENGTHS == [0, 1, 3, 4, 14, 15, 16, 17, 18, 19, 31, 32, 60, 61, 64, 65, 255, 256, 257, 4095, 4096, 16383, 16384, 16385,
                               32768, 65520, 65521, 65535, 65536]


def test_what_the_parse_cannot_produce():
    """The two places where compress_inputs.py's classes differ from a list of round numbers, as arithmetic: a literal in front of a copy is as
    long as a probe offset of one scan, and 60, 64, 256 and 257 are none; a hit lies at n - 16 at the latest."""
    offsets = CI.scan_offsets(65536)
    assert offsets[:34] == list(range(1, 34)) + [35] and offsets[32 + 16] == 65 and offsets[32 + 17] == 68
    assert [v for v in CI.LITERAL_LENGTHS if v not in offsets] == [60, 64, 256, 257]
    assert CI.LITERALS_BEFORE_COPY == [1, 14, 15, 16, 17, 61, 65]
    for variant in VARIANTS:
        for name, f in CI.directed_named(variant):
            if name == "off_max":
                assert max(a for kind, a, _l in CI.trace(f, variant)[0] if kind == "copy") == 65519 == len(f) - 16 - 1


@pytest.mark.parametrize("variant", VARIANTS)
def test_directed_set_shows_every_class_and_the_tracer_equals_the_oracle_on_it(variant):
    named = CI.directed_named(variant)
    assert named == CI.directed_named.__wrapped__(variant, 0), "directed() is not deterministic"
    frags = CI.directed(variant)
    encoded, census = CI.trace_all(frags, variant, WORKERS)
    for f, enc in zip(frags, encoded):
        assert enc == O.compress(f, variant), (len(f), f[:64].hex())
    short = {k: v for k, v in census.items() if v < CI.PER_CLASS}
    assert not short and set(census) == set(CI.CLASSES), short
    for name, f in named:                                             # every fragment was kept for the class it is listed under
        if name in CI.CLASSES:
            assert CI.trace(f, variant)[1][name] > 0, name
    assert max(len(f) for f in frags) == 65536 and sum(len(f) for f in frags) < 4 << 20


@functools.lru_cache(maxsize=None)
def _fuzz_rounds(variant):
    text = _text()
    rounds = []
    for seed in fuzz_seeds(variant):
        rng = np.random.default_rng(seed)
        blocks = [CI.make_block(rng, text).tobytes() for _ in range(FUZZ_BLOCKS)]
        rounds.append((seed, blocks, *CI.trace_all(blocks, variant, WORKERS)))
    return rounds


@pytest.mark.parametrize("variant", VARIANTS)
def test_tracer_equals_the_oracle_on_fuzz_blocks(variant):
    """(Every block of both rounds, not only 200: the census below needs their traces anyway.)"""
    for seed, blocks, encoded, _census in _fuzz_rounds(variant):
        for b, (f, enc) in enumerate(zip(blocks, encoded)):
            assert enc == O.compress(f, variant), f"seed {seed} block {b} (len {len(f)})"


def test_census_of_the_fuzz_rounds_and_the_directed_set():
    record = {"what": "number of fragments in which each event class of tests/compress_inputs.py occurs: two fuzz rounds of 768 make_block blocks "
                      "(the seeds of test_fuzz_compress_bytes_equal_oracle, layout lanes) and the directed set, per hash",
              "classes": list(CI.CLASSES), "hash": {}}
    for variant in VARIANTS:
        frags = CI.directed(variant)
        directed = CI.trace_all(frags, variant, WORKERS)[1]
        assert min(directed.values()) >= CI.PER_CLASS
        record["hash"][str(variant)] = {
            "directed": {"fragments": len(frags), "bytes": sum(len(f) for f in frags), "census": directed},
            "fuzz": [{"seed": seed, "fragments": len(blocks), "census": census} for seed, blocks, _enc, census in _fuzz_rounds(variant)]}
    try:
        with open(os.path.join(ROOT, "profiles", "r13a_compress_input_census.json"), "w") as f:
            json.dump(record, f, indent=1, sort_keys=True)
            f.write("\n")
    except OSError:                                                   # a read-only checkout: the committed record stays as it is
        pass


@pytest.mark.parametrize("variant", VARIANTS)
def test_window_model_equals_the_oracle_on_the_directed_set(variant):
    for f in CI.directed(variant):
        ref = O.compress(f, variant)
        for np_, cap in ((1, 32), (2, 32), (4, 32), (1, 16), (2, 16), (4, 16)):
            assert WM.compress(f, variant, np_, cap) == ref, (len(f), np_, cap, f[:64].hex())

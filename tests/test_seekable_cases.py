"""The batches of seekable_cases.py hold what they claim (no GPU): both chunk types in every batch, real slot counts on the intended side of
each launch threshold, lengths 0 and 1 in every ragged tail, request lists the models accept with served, empty and failing requests among
them, and the arithmetic that stands in for the models at the large counts equal to the models at the small ones."""
import re

import pytest

import frame_chunked_model as K
import frame_index_model as X
import frame_range_model as R
import frame_update_model as U
import oracle as O
import seekable_cases as SC
from conftest import ROOT

VARIANTS = [O.HASH_CRC32C, O.HASH_MUL]
SMALL = [64, 1000]


def kinds(want):
    """(compressed, raw) chunk counts of an encode."""
    types = [s[p] for s, f0, f1 in zip(want["streams"], want["first"], want["first"][1:]) for p in want["pos"][f0:f1]]
    return types.count(0), types.count(1)


def both_kinds(batch, variant):
    want = K.encode(batch.blobs, batch.cb, variant)
    comp, raw = kinds(want)
    assert want["status"] == [O.OK] * len(batch.blobs) and comp + raw == batch.slots()
    assert 10 * comp >= comp + raw and 10 * raw >= comp + raw, (batch.cb, comp, raw)


def test_the_defaults_are_those_of_capi_internal_h():
    text = open(f"{ROOT}/snappier_amd/csrc/capi_internal.h").read()
    for name, value in (("win_dual_min", SC.WIN_DUAL_MIN), ("win_gtab_min", SC.WIN_GLOBAL_MIN), ("win_max", SC.WIN_MAX),
                        ("small_min_blocks", SC.SMALL_MIN_BATCH), ("slice_fragments", SC.SLICE)):
        assert re.search(rf"\bu32 {name} = {value};", text), name


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("cb", SMALL)
def test_small_batch(cb, variant):
    b = SC.small_batch(cb)
    assert [len(x) for x in b.blobs] == [0, 1, cb - 1, cb + 1, 3 * cb + 7, 40 * cb + 3] and b is SC.small_batch(cb)
    both_kinds(b, variant)
    assert b.slots() < SC.WIN_DUAL_MIN                                  # the exact bound is the LDS window tier; every other tier comes from the bound
    streams = SC.decode_streams(b, variant)
    lens = [len(x) for x in b.blobs] + [len(b.blobs[-1])]
    ix = X.build_index(streams)
    assert ix["tail"] == [O.OK] * 7 and ix["total"] == lens
    # the indexed read: served, empty and failing requests, and the arithmetic equal to the model on the sound streams
    caps = [R.clip(lens[s], ro, rl)[1] - R.clip(lens[s], ro, rl)[0] for s, ro, rl in b.reads]
    mc, ec = X.read_needs(streams, ix, b.reads, caps)
    st, ol, data, res = X.read_plan(streams, ix, b.reads, caps, mc, ec)
    failing = [r for r, s in enumerate(st) if s != O.OK]
    assert failing and all(b.reads[r][0] == 6 for r in failing) and 0 in ol and sum(1 for n in ol if n) >= 25
    assert any(s == O.OK and q[0] == 6 and n for s, n, q in zip(st, ol, b.reads))
    sound = [q for q in b.reads if q[0] < 6]
    assert SC.read_needs(lens, cb, sound) == X.read_plan(streams, ix, sound, [c for c, q in zip(caps, b.reads) if q[0] < 6], 1 << 40, 1 << 40)[3]
    # the range decode: one window per stream, the corrupt stream's across the corrupt chunk
    rcaps = [R.clip(n, *w)[1] - R.clip(n, *w)[0] for n, w in zip(lens, b.ranges)]
    rst = R.range_plan(streams, b.ranges, rcaps, *R.needs(streams, b.ranges, rcaps))[0]
    assert rst[:6] == [O.OK] * 6 and rst[6] != O.OK and 0 in rcaps
    # the indexed write: sorted and disjoint, a zero-length request, the corrupt stream refused alone
    assert b.writes == sorted(b.writes) and any(ln == 0 for _, _, ln in b.writes)
    srcs = b.write_srcs()
    plan = U.write_plan(streams, ix, b.writes, srcs, variant=variant)
    assert plan["status"][:6] == [O.OK] * 6 and plan["status"][6] not in (O.OK, O.ERR_BAD_ARG, O.ERR_OUTPUT_TOO_SMALL)
    assert plan["result"][3] == 6 and all(s in (O.OK, plan["status"][6]) for s in plan["req_status"])
    assert SC.write_needs(lens, cb, b.writes) == (plan["result"][0], plan["result"][2])
    for s in range(6):
        assert plan["streams"][s] == K.stream_of(U.patched(b.blobs[s], b.writes, srcs, s), cb, variant)


@pytest.mark.parametrize("cb,slots", SC.COUNT_PAIRS)
def test_count_batch(cb, slots):
    b = SC.count_batch(cb, slots)
    lens = [len(x) for x in b.blobs]
    assert {0, 1} <= set(lens[1:]) and max(lens[1:]) < 6 * cb and K.nchunks(lens[0], cb) == slots
    for variant in VARIANTS:
        both_kinds(b, variant)
    # on the intended side of each threshold: the real count, not the bound, picks the tier
    real = b.slots()
    side = {64: real > SC.WIN_MAX and real > SC.LANE_TIERS[1], 256: SC.LANE_TIERS[0] <= real < SC.WIN_MAX and real >= SC.WIN_GLOBAL_MIN,
            1000: SC.WIN_DUAL_MIN <= real < SC.WIN_GLOBAL_MIN, 4096: SC.WIN_DUAL_MIN <= real < SC.SMALL_MIN_BATCH}
    assert side[cb] and real < SC.SLICE
    assert all(q[0] == len(lens) for q in b.reads[-4:]) and len(b.ranges) == len(lens) + 1
    interior, _, edge, nreq = SC.read_needs(lens, cb, b.reads[:-4])
    assert interior == slots and nreq == 2 * slots - 1 and edge == 2 * cb * (slots - 2) + cb + (cb - 5)
    if slots >= 10000:
        assert interior >= SC.SMALL_MIN_BATCH and 2 * (slots - 1) >= SC.SMALL_MIN_BATCH      # interior rows and edge rows both reach the pre-pass
    assert SC.write_needs(lens, cb, b.writes) == (slots, lens[0])
    edges = SC.boundary_writes(b)
    assert SC.write_needs(lens, cb, edges)[0] == 2 * len(edges) and len(edges) == (slots - 1 + 1) // 2


HINT_BATCHES = SC.COMPRESS_SEQUENCE + [(cb, 64 if cb == 65536 else SC.hint_rows(SC.SMALL_MIN_BATCH)) for cb in SC.DECODE_SEQUENCE]


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("cb,slots", HINT_BATCHES)
def test_hint_batches_hold_both_chunk_types(cb, slots, variant):
    """Every batch of the two hint sequences, as the GPU tests build them."""
    b = SC.count_batch(cb, slots)
    assert K.nchunks(len(b.blobs[0]), cb) == slots and (slots == 64 or slots >= 3000)
    both_kinds(b, variant)

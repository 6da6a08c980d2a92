"""The generator of foreign Snappy streams (tests/stream_grammar.py) held to the references, without a GPU: what it builds is what both oracles
decode; the corpus the device tests use really contains every tag form, length and offset it is there for; every near-miss gets the status
written down here; and the CPU models of the sub-chain parse and of the tag index take the foreign dialect as they take ours.  What the device
does with the same streams is tests/test_gpu_stream_grammar.py."""
from collections import Counter

import pytest

import frame_buffers_model as FM
import oracle as O
import stream_grammar as G
import subchain_model as SM
from oracle import pymodel
from tag_index_model import DEVICE_CHUNK, DEVICE_PROBE, DEVICE_SUB, TagIndexModel, device_fix_passes, reference_entries

TOTALS = (0, 1, 2, 60, 61, 64, 65, 300, 512, 4096, 12000, 65535, 65536)
LARGE_TOTALS = (65537, 150000, 262145)


def built(profile, totals=TOTALS):
    return [(total,) + G.build(3, total, profile) for total in totals]


# ---- agreement -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("profile", G.PROFILES)
def test_built_streams_decode_to_what_the_generator_produced(profile):
    for total, stream, raw, tags in built(profile):
        assert len(raw) == total
        assert raw == O.decompress(stream) == pymodel.decompress(stream), (profile, total)
        assert (stream, raw, tags) == G.build(3, total, profile)                     # the same seed: the same bytes
        ip, op = G.preamble_bytes(stream), 0
        for t_ip, t_op, kind, form, n, off in tags:                                  # the tag list is the stream: no gaps, no overlap
            assert (t_ip, t_op) == (ip, op)
            ip += 1 + (form if kind == G.LIT else {1: 1, 2: 2, 4: 4}[form]) + (n if kind == G.LIT else 0)
            op += n
        assert (ip, op) == (len(stream), total)


@pytest.mark.parametrize("profile", G.PROFILES)
def test_large_and_constrained_streams_decode_to_what_the_generator_produced(profile):
    for total in TOTALS[7:] + LARGE_TOTALS:
        for bounded in (False, True):
            stream, raw, tags = G.build(5, total, profile, fragment_local=True, bounded=bounded)
            assert raw == O.decompress(stream), (profile, total, bounded)
            assert G.is_fragment_local(tags)
            assert not bounded or len(stream) <= 38 + total + total // 6
            assert total > G.B or (stream, raw, tags) == G.build(5, total, profile, fragment_local=True, bounded=bounded)
    if profile == "far":
        for total in LARGE_TOTALS:
            stream, raw, tags = G.build(5, total, "far")
            assert raw == O.decompress(stream)
            assert not G.is_fragment_local(tags)
            assert total == 65537 or sum(1 for t in tags if t[5] >= 65536) >= 20
            assert max(t[5] for t in tags) >= 65536


def test_profiles_are_what_their_names_say():
    for total in (4096, 65536):
        tags = G.build(3, total, "copy4")[2]
        assert 2 * sum(1 for t in tags if t[2] == G.COPY and t[3] == 4) >= len(tags)
        tags = G.build(3, total, "fat-literals")[2]
        assert all(t[3] > G.min_literal_form(t[4]) or t[3] == 4 for t in tags if t[2] == G.LIT)
        assert sum(1 for t in tags if t[2] == G.LIT and t[3] > G.min_literal_form(t[4])) > 10
        tags = G.build(3, total, "pattern")[2]
        assert all(t[5] < t[4] and t[5] <= 16 for t in tags if t[2] == G.COPY) and sum(1 for t in tags if t[2] == G.COPY) > 20
        stream, _raw, tags = G.build(3, total, "dense")
        assert 2 * len(stream) >= 5 * total and all(t[4] <= 3 and t[3] == 4 for t in tags)
        tags = G.build(3, total, "two-slot")[2]
        fat = [i for i, t in enumerate(tags) if t[2] == G.LIT and 65 <= t[4] <= 128]
        assert {tags[i][3] for i in fat} == {1, 2, 3, 4}
        assert max(b - a for a, b in zip(fat, fat[1:])) >= 64                        # runs of 64 and more short tags between them
        assert any(t[2] == G.COPY and t[3] == 4 for t in tags)


# ---- coverage of the corpus the device tests decode ----------------------------------------------------------------------------------------
def device_corpus_tags():
    """The tag lists of every stream the device tests decode as built (a near-miss keeps most of its tags, but none is counted here)."""
    cases = [c for c in G.batch_corpus() if c.mutation is None]
    cases += [G.large_local(p) for p in G.PROFILES] + [G.large_local(p, True) for p in G.PROFILES if p != "dense"]
    cases += [G.large_foreign(k) for k in range(len(G.LARGE_FOREIGN))]
    return [(c.profile, c.tags) for c in cases]


def test_the_device_corpus_covers_every_form_length_and_offset():
    lit, copy, offsets, patterns, last_slot = Counter(), Counter(), Counter(), Counter(), Counter()
    for profile, tags in device_corpus_tags():
        for i, (_ip, _op, kind, form, n, off) in enumerate(tags):
            if kind == G.LIT:
                lit[n if n in G.LITERAL_EDGES else "other", form] += 1
                if profile == "two-slot" and 65 <= n <= 128 and i % 64 == 63:
                    last_slot[form] += 1
            else:
                copy[form, n] += 1
                offsets[off] += 1
                if off < n:
                    patterns[off] += 1
    # every literal length class in every encoding the format permits (class "other": lengths outside the edge set, in all five)
    want = [(n, f) for n in G.LITERAL_EDGES for f in range(G.min_literal_form(n), 5)] + [("other", f) for f in range(5)]
    assert [w for w in want if not lit[w]] == []
    assert [(n, f) for (n, f) in lit if n != "other" and f < G.min_literal_form(n)] == []
    # every copy form at the lengths where the decoders change path (copy-1 holds 4..11 only)
    assert [(f, n) for f in (1, 2, 4) for n in (1, 4, 11, 12, 64) if (f != 1 or 4 <= n <= 11) and not copy[f, n]] == []
    assert [o for o in G.OFFSET_EDGES if not offsets[o]] == []
    assert [o for o in range(1, 17) if not patterns[o]] == []
    assert [f for f in (1, 2, 3, 4) if not last_slot[f]] == []
    # copy-4 for offsets a copy-1 could hold, copy-2 likewise, and offsets no other form holds
    assert any(f == 4 for (f, n) in copy) and max(offsets) > 65537


# ---- near-misses ---------------------------------------------------------------------------------------------------------------------------
# The oracle's status of every kind of near-miss (oracle/snappy_oracle.c orc_decompress, read and then confirmed here on every stream).
STATUS = {
    "offset-past": O.ERR_BAD_OFFSET, "offset-zero": O.ERR_BAD_OFFSET, "offset-ffffffff": O.ERR_BAD_OFFSET, "offset-80000000": O.ERR_BAD_OFFSET,
    "last-length+1": O.ERR_TOO_LONG, "declared+1": O.ERR_INCOMPLETE, "declared-1": O.ERR_TOO_LONG,
    "cut-trailer": O.ERR_INCOMPLETE, "cut-body": O.ERR_INCOMPLETE, "cut-after-tag": O.ERR_INCOMPLETE, "extra-tag": O.ERR_TOO_LONG,
}
# What the oracle really accepts: an offset equal to the bytes produced so far is the largest legal one.
ACCEPTED = {"offset-at-start": O.OK}
# A literal whose declared length is 2^31 and more swallows the rest of the stream as its body: TOO_LONG when those bytes are more than the
# output still to come, INCOMPLETE when they are fewer -- and a stream that decodes (to other bytes) when they are exactly as many.
SWALLOWS = ("literal-7fffffff", "literal-80000000", "literal-ffffffff")


def swallow_status(stream: bytes, tags, kind: str) -> int:
    ip, op = tags[G.target(tags, kind)][:2]
    rest, room = len(stream) - ip, tags[-1][1] + tags[-1][4] - op
    return O.ERR_TOO_LONG if rest > room else O.ERR_INCOMPLETE if rest < room else O.OK


def test_every_near_miss_gets_its_status_from_the_oracle():
    assert set(STATUS) | set(ACCEPTED) | set(SWALLOWS) == set(G.MUTATIONS)
    cases = [c for c in G.batch_corpus() if c.mutation is None][::4] + [G.large_local(p) for p in G.PROFILES] + [G.large_foreign(0)]
    applied, seen = Counter(), {k: set() for k in G.MUTATIONS}
    for c in cases:
        for kind in G.MUTATIONS:
            m = G.mutate(c.stream, c.tags, kind)
            if m is None:
                assert G.target(c.tags, kind) is None
                continue
            assert m != c.stream
            applied[kind] += 1
            st = O.decompress_status(m)
            seen[kind].add(st)
            if kind in SWALLOWS:
                assert st == swallow_status(c.stream, c.tags, kind), (c.profile, c.total, kind)
            else:
                assert st == {**STATUS, **ACCEPTED}[kind], (c.profile, c.total, kind, st)
    assert all(applied[k] >= 100 for k in G.MUTATIONS), applied
    assert all(len(seen[k]) == 1 for k in STATUS) and all(seen[k] >= {O.ERR_TOO_LONG, O.ERR_INCOMPLETE} for k in SWALLOWS)
    # the near-misses inside the device corpus: a third of it, every kind, and none of them decodes unless listed above
    mutated = [c for c in G.batch_corpus() if c.mutation is not None]
    assert 3 * len(mutated) >= len(G.batch_corpus()) - 30 and {c.mutation for c in mutated} == set(G.MUTATIONS)
    for c in mutated:
        st = O.decompress_status(c.stream)
        assert st == (swallow_status(c.built, c.tags, c.mutation) if c.mutation in SWALLOWS else {**STATUS, **ACCEPTED}[c.mutation])


def test_named_near_misses_of_a_hand_built_stream():
    """The distinctions the statuses rest on, on a stream short enough to read: literal "abcd", copy-4 of 4 from offset 4, copy-2 of 2 from 8."""
    good = bytes([10, 0x0C]) + b"abcd" + G.copy_tag(4, 4, 4) + G.copy_tag(2, 8, 2)
    assert O.decompress(good) == b"abcdabcdab"
    at = 6                                                                           # the copy-4: 4 bytes produced before it
    assert O.decompress_status(good[:at] + G.copy_tag(4, 5, 4) + good[at + 5:]) == O.ERR_BAD_OFFSET       # offset = produced + 1
    assert O.decompress_status(good[:at] + G.copy_tag(4, 0, 4) + good[at + 5:]) == O.ERR_BAD_OFFSET       # offset 0
    assert O.decompress(good[:at] + G.copy_tag(4, 4, 2) + good[at + 5:]) == b"abcdabcdab"                 # offset = produced, as a copy-2
    assert O.decompress_status(good[:-3] + G.copy_tag(3, 8, 2)) == O.ERR_TOO_LONG                         # the last copy one byte too long
    fat = bytes([4, 0xFC, 3, 0, 0, 0]) + b"abcd"                                                          # a 4-byte literal under a 4-byte length
    assert O.decompress(fat) == pymodel.decompress(fat) == b"abcd"


# ---- the CPU models on the foreign dialect -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("profile", G.PROFILES)
def test_sub_chain_windows_equal_the_sequential_walk(profile):
    windows = 0
    for total, stream, _raw, _tags in built(profile):
        for ip, pos, consumed in SM.stream_windows(stream):
            want_pos, want_end = SM.sequential(stream[ip:] + bytes(SM.W + 16), min(SM.W, len(stream) - ip) - 8)
            assert pos == want_pos and consumed == want_end, (profile, total, ip)
            windows += 1
    assert windows >= 10


@pytest.mark.parametrize("profile", G.PROFILES)
def test_tag_index_model_gives_the_serial_walks_entries_or_fails(profile):
    done = 0
    for total, stream, _raw, _tags in built(profile, TOTALS[3:]):
        hb = G.preamble_bytes(stream)
        m = TagIndexModel(stream, hb)
        r = m.run()
        want, final = reference_entries(stream, hb, m.chunk, m.sub)
        assert final == (len(stream), total)
        assert r[0] == "fail" or (r[0] == "done" and r[1] == want and r[2] == final), (profile, total, r[0])
        done += r[0] == "done"
    assert done >= len(TOTALS[3:]) - 2, done


@pytest.mark.parametrize("profile", G.PROFILES)
def test_large_fragment_local_streams_give_their_look_back_verdict_at_device_sizes(profile):
    c = G.large_local(profile)
    assert G.is_fragment_local(c.tags) and 150000 <= c.total <= 300000 and O.decompress(c.stream) == c.raw
    assert look_back(c) == G.LARGE_LOOK_BACK[profile]


def look_back(c) -> int:
    hb = G.preamble_bytes(c.stream)
    if len(c.stream) * 100 >= c.total * 85:
        return 1
    nchunks = (len(c.stream) - hb + DEVICE_CHUNK - 1) // DEVICE_CHUNK
    m = TagIndexModel(c.stream, hb, DEVICE_CHUNK, DEVICE_SUB, DEVICE_PROBE)
    r = m.run(max_passes=device_fix_passes(nchunks))
    want, final = reference_entries(c.stream, hb, DEVICE_CHUNK, DEVICE_SUB)
    assert r[0] == "fail" or (r[1] == want and r[2] == final == (len(c.stream), c.total))
    return 0 if r[0] == "done" else 1


def test_large_foreign_streams_are_what_the_fragment_decoder_cannot_take():
    for k, (profile, total) in enumerate(G.LARGE_FOREIGN):
        c = G.large_foreign(k)
        assert O.decompress(c.stream) == c.raw and len(c.stream) <= 38 + total + total // 6
        straddles = [t for t in c.tags if t[1] // G.B != (t[1] + t[4] - 1) // G.B]
        reaches = [t for t in c.tags if t[2] == G.COPY and t[5] > t[1] % G.B]
        assert straddles and reaches
        assert profile != "far" or max(t[5] for t in c.tags) >= 65536
    # decode_chains.hip packs a re-dealt batch's offsets beside the slot's length and body position: 64 consecutive tags that hold a 65..128-byte
    # literal written as 0xf0 + one length byte (what re-deals a batch) and a copy from 65536 bytes back or more (an offset wider than 16 bits)
    tags = G.large_foreign(0).tags
    dealt = [i for i, t in enumerate(tags) if t[2] == G.LIT and t[3] == 1 and 65 <= t[4] <= 128]
    assert sum(1 for i in dealt if any(t[2] == G.COPY and t[5] >= 65536 for t in tags[max(i - 63, 0):i + 64])) >= 5


# ---- framing -------------------------------------------------------------------------------------------------------------------------------
def test_framed_foreign_chunks_decode_to_the_concatenated_output():
    statuses = {}
    for name, stream, raws in G.frame_corpus():
        assert stream.startswith(FM.STREAM_ID) and all(len(r) <= G.B for r in raws)
        try:
            assert O.frame_decode(stream) == b"".join(raws), name
            statuses[name] = O.OK
        except O.OracleError as e:
            statuses[name] = e.status
    assert statuses == {"one": 0, "empty-then-full": 0, "with-uncompressed": 0, "five": 0, "four": 0, "mutated-chunk": O.ERR_BAD_OFFSET,
                        "wrong-crc": O.ERR_CRC_MISMATCH, "mixed": 0}
    sizes = [len(r) for _n, _s, raws in G.frame_corpus() for r in raws]
    assert 0 in sizes and G.B in sizes and 1 <= min(len(r) for _n, _s, r in G.frame_corpus()) and max(len(r) for _n, _s, r in G.frame_corpus()) == 5


def test_frame_models_read_every_window_of_the_foreign_chunks():
    """What the device tests of the range and indexed reads compare with (frame_range_model.range_plan, frame_index_model.read_plan), on the
    framed foreign streams, against plain slices of the chunks' output."""
    import frame_index_model as X
    import frame_range_model as R
    frames = G.frame_corpus()
    streams = [s for _n, s, _r in frames]
    pairs = [(b, w) for b, s in enumerate(streams) for w in R.windows(*R.walk(s)[:2])]
    per, ranges = [streams[b] for b, _w in pairs], [w for _b, w in pairs]
    caps = [R.clip(R.walk(s)[1], *w)[1] - R.clip(R.walk(s)[1], *w)[0] for s, w in zip(per, ranges)]
    st, _ol, data, _res = R.range_plan(per, ranges, caps, *R.needs(per, ranges, caps))
    ix = X.build_index(streams)
    reqs = [(b, w[0], w[1]) for b, w in pairs]
    st_x, _ol, data_x, _res = X.read_plan(streams, ix, reqs, caps, *X.read_needs(streams, ix, reqs, caps))
    assert st == st_x and data == data_x and set(st) == {O.OK, O.ERR_BAD_OFFSET, O.ERR_CRC_MISMATCH}
    for (b, w), s, d in zip(pairs, st, data):
        whole = b"".join(frames[b][2])
        lo, hi = R.clip(len(whole), *w)
        if frames[b][0] not in ("mutated-chunk", "wrong-crc"):
            assert s == O.OK and d == whole[lo:hi], (frames[b][0], w)
        elif s == O.OK:                                                              # a window that does not meet the bad chunk
            assert d == whole[lo:hi]

"""The ranges of crc_cases.py hold what they claim (no GPU): every length at every alignment, 1 .. 16 bytes between ranges, the prefix counts on
the intended side of the launch policy's threshold and at each position of a group of four and of sixteen, one CRC per distinct length over
the zero buffer, and the reference's known answers inside the sweep."""
import re

import numpy as np

import crc_cases as CC
import frame_buffers_model as M
import kats
import oracle as O
from conftest import ROOT


def test_the_threshold_is_that_of_crc32c_hip():
    text = open(f"{ROOT}/snappier_amd/csrc/crc32c.hip").read()
    assert "if (!(masked & 6) && nblocks < 16u * 256u * kWaves11) masked |= 4;" in text
    waves, per = (int(re.search(rf"#define {name} (\d+)", text).group(1)) for name in ("SNP_CRC_WAVES11", "SNP_CRC_PER11"))
    assert CC.THREE_TABLE_MIN == 16 * 256 * waves == 16384 and (CC.PER_WAVEFRONT, CC.PER_WORKGROUP) == (per, per * waves)


def test_every_length_meets_every_alignment():
    off, ln, size = CC.ranges()
    assert len(off) == len(ln) == CC.COUNT == 16 * len(CC.LENGTHS) and len(set(CC.LENGTHS)) == len(CC.LENGTHS)
    assert set(range(2101)) <= set(CC.LENGTHS) and {3071, 3072, 3073, 4095, 4096, 4097, 5119, 5120, 5121, 65535, 65536, 65537, 70000} <= set(CC.LENGTHS)
    assert (off % 16 == np.arange(CC.COUNT) % 16).all()                 # range k at alignment k % 16
    assert set(zip(ln.tolist(), (off % 16).tolist())) == {(n, a) for n in CC.LENGTHS for a in range(16)}
    end = off + ln
    gaps = np.concatenate([off[:1], off[1:] - end[:-1]]).astype(np.int64)
    assert gaps.min() >= 1 and gaps.max() <= 16 and int(end[-1]) + 16 == size and 39_000_000 < size < 42_000_000
    # every residue mod 1024 in ranges of one row (from 4 bytes on: shorter ones take the byte path) and of two rows, and ranges of three rows:
    # a two-row prefetch with nothing, one row and two rows to fetch behind it
    residues = {rows: {n % 1024 for n in CC.LENGTHS if n >= 4 and (n + 1023) // 1024 == rows} for rows in (1, 2, 3)}
    assert residues[1] == set(range(4, 1024)) | {0} and residues[2] == set(range(1024)) and set(range(1, 53)) | {1023, 0} <= residues[3]
    # the shortest prefix already meets every length, and every alignment with over a thousand of them
    head_len, head_al = ln[:CC.THREE_TABLE_MIN - 1], (off % 16)[:CC.THREE_TABLE_MIN - 1]
    assert set(head_len.tolist()) == set(CC.LENGTHS)
    assert all(len(set(head_len[head_al == a].tolist())) >= 1023 for a in range(16))
    assert len(set(ln[k] for k in range(16))) == 16                     # the lengths of one group differ: they cycle


def test_the_prefixes_are_the_ones_the_policy_and_the_groups_ask_for():
    t = CC.THREE_TABLE_MIN
    assert CC.PREFIXES == [t - 1, t, t + 1, t + 3, t + 4, t + 5, t + 15, CC.COUNT]
    assert {n % CC.PER_WAVEFRONT for n in CC.PREFIXES[1:7]} == {0, 1, 3} and {n % CC.PER_WAVEFRONT for n in CC.PREFIXES} == {0, 1, 3}
    assert [n % CC.PER_WORKGROUP for n in CC.PREFIXES[1:7]] == [0, 1, 3, 4, 5, 15] and (t + 3) % 4 == 3 and (t + 5) % 4 == 1
    assert all(n >= t for n in CC.PREFIXES[1:]) and CC.PREFIXES[0] < t and CC.COUNT % CC.PER_WORKGROUP == 0


def test_the_zero_buffer_gives_one_crc_per_length():
    """The issue states 2 113 values; the lengths it lists (0 .. 2100 and thirteen more) are 2 114, and what it asks for is one value per
    distinct length."""
    for masked in (False, True):
        want = CC.expected("zeros", masked)
        assert len(set(want.tolist())) == len(set(CC.LENGTHS)) == 2114
        _, ln, _ = CC.ranges()
        by_len = {}
        for n, c in zip(ln.tolist(), want.tolist()):
            assert by_len.setdefault(n, c) == c                         # the length alone decides
    assert int(CC.expected("zeros", False)[np.nonzero(CC.ranges()[1] == 0)[0][0]]) == 0


def test_the_known_answers_lie_inside_the_sweep():
    off, ln, _ = CC.ranges()
    data = CC.contents()["random"]
    cases = CC.kat_ranges()
    assert [(d, c) for _, d, c in cases] == kats.CRC32C[:3] and all(k < CC.THREE_TABLE_MIN - 1 for k, _, _ in cases)
    for k, kat, crc in cases:
        assert data[int(off[k]):int(off[k]) + int(ln[k])].tobytes() == kat
        assert int(CC.expected("random", False)[k]) == crc == O.crc32c(kat) and int(CC.expected("random", True)[k]) == O.crc32c_mask(crc)
    assert not CC.contents()["zeros"].any() and len(set(CC.expected("random", False).tolist())) > CC.COUNT - 16 * 4 - 8


def test_the_foreign_batches_are_what_they_claim():
    streams, _, want = CC.foreign_batch()
    status = [s for s, _ in want]
    assert len(streams) == 8 and status[:5] == [O.OK] * 5 and status[5] == O.ERR_CRC_MISMATCH
    assert status[6] not in (O.OK, O.ERR_CRC_MISMATCH) and status[7] not in (O.OK, O.ERR_CRC_MISMATCH, status[6])   # the decoder's own; the walk's own
    rows = [M.serial_walk(s, 1 << 40)[0] for s in streams]
    assert sum(len(r) for r in rows) >= CC.THREE_TABLE_MIN + 5 and {r[0] for rs in rows for r in rs} == {0, 1}
    sizes = {r[5] for rs in rows for r in rs}
    assert min(sizes) == 1 and max(sizes) == 2100 and len(sizes) > 2000
    first = sum(len(r) for r in rows[:5])
    assert {(first + k) % 4 for k in CC.BAD_CRC[:4]} == {0, 1, 2, 3}      # the bad CRCs sit at every position of a wavefront's group of four
    for k in CC.BAD_CRC:
        assert CC.single_bad_crc_batch(k)[2] == want and CC.single_bad_crc_batch(k)[0][5] != streams[5]
    small, _, small_want = CC.small_batch()
    assert sum(len(M.serial_walk(s, 1 << 40)[0]) for s in small) == 40 and sorted(s for s, _ in small_want) == sorted([O.OK, O.OK] + status[5:])


def test_the_ragged_buffers_need_three_slots_past_the_threshold():
    blobs, want = CC.ragged_buffers()
    lens = [len(x) for x in blobs]
    assert len(blobs) == 64 and lens[:5] == [0, 1, 999, 1000, 1001] and len(set(lens)) == 64 and lens[-1] % CC.CHUNK
    assert want["result"][0] == want["result"][2] == CC.THREE_TABLE_MIN + 3 and want["status"] == [O.OK] * 64
    types = [s[p] for s, f0, f1 in zip(want["streams"], want["first"], want["first"][1:]) for p in want["pos"][f0:f1]]
    assert min(types.count(0), types.count(1)) * 10 >= len(types)       # both chunk types, a tenth of the slots at least

"""Pure-Python statement of include/snappier_hip_frame_dedup.h (snp_frame_dedup_indexed_batch), written from the header's text on top of
oracle, frame_buffers_model.hop (one header), frame_index_model.row_end and frame_rechunk_model.begin / rows_of (the index and its clamps): the
verdict of every stream over an untrusted index, the key of a row, the leader rule and canon, the pack and its index, the recipes in the
compose call's CSR form, the in-order admission by max_entries / out_cap / max_segs and d_result.  Also the forged pair: two payloads of equal
length and equal CRC-32C, by a four-byte fix-up.  The CPU and the GPU tests share it."""
import struct

import frame_buffers_model as M
import frame_index_model as X
import frame_rechunk_model as RC
import oracle as O

U64 = (1 << 64) - 1
NONE = U64                      # SNP_DEDUP_NONE
MAX_ROWS = (1 << 31) - 1


# ---- the verdict ---------------------------------------------------------------------------------------------------------------------------------
def nentries_of(ix) -> int:
    return min(len(ix["start"]), len(ix["pos"]))


def stream_verdict(ix, b: int, s: bytes, before: int):
    """-> (status, rows): rows is the list of (row, pos, size, dec, crc) of a stream that passed, size = the chunk's 4 + size bytes."""
    st = RC.begin(ix, b)
    if st != O.OK:
        return st, []
    f0, n = RC.rows_of(ix, b)
    if f0 < before:
        return O.ERR_BAD_ARG, []
    f1, total, rows = f0 + n, ix["total"][b], []
    for i in range(f0, f1):
        a, e, pos = ix["start"][i], X.row_end(ix, f1, total, i), ix["pos"][i]
        if e < a or pos >= len(s):
            return O.ERR_BAD_ARG, []
        h = M.hop(s, pos)
        if h.kind != "data" or e - a != h.dec:
            return O.ERR_BAD_ARG, []
        if i + 1 < f1 and ix["pos"][i + 1] < h.next:
            return O.ERR_BAD_ARG, []
        rows.append((i, pos, h.next - pos, h.dec, h.crc))
    return O.OK, rows


def verdicts(streams, ix):
    """-> (status per stream, rows per stream).  A stream that begins below the idx_first of one in front of it runs backwards."""
    ne, before, status, rows = nentries_of(ix), 0, [], []
    for b, s in enumerate(streams):
        st, r = stream_verdict(ix, b, s, before)
        status.append(st)
        rows.append(r)
        before = max(before, min(ix["first"][b], ne))
    return status, rows


# ---- the whole call ------------------------------------------------------------------------------------------------------------------------------
def dedup_plan(streams, ix, nbase: int = 0, max_entries: int | None = None, max_segs: int | None = None, out_cap: int | None = None):
    """snp_frame_dedup_indexed_batch.  None: a bound that admits all.
    -> dict of status, canon, out_len, pack (bytes; None when out_cap < 10), index (the pack's: first, start, pos, total, tail), segs (first,
    stream, off, len: the recipes), result [8]."""
    ns, ne = len(streams), nentries_of(ix)
    assert 0 <= nbase <= ns and ne <= MAX_ROWS
    BIG = 1 << 62
    max_entries = BIG if max_entries is None else max_entries
    max_segs = BIG if max_segs is None else max_segs
    out_cap = BIG if out_cap is None else out_cap
    status, rows = verdicts(streams, ix)
    # the map
    canon, leader, chunk_of, info = [NONE] * ne, {}, {}, {}
    for b in range(ns):
        for i, pos, size, dec, crc in rows[b]:
            if dec == 0:
                continue
            chunk_of[i] = streams[b][pos:pos + size]
            info[i] = (b, dec, size)
            leader.setdefault((dec, crc), i)                             # (rows in ascending order: the first is the smallest)
    coll = merged = mbytes = 0
    for i in sorted(chunk_of):
        b, dec, size = info[i]
        crc = int.from_bytes(chunk_of[i][4:8], "little")
        lead = leader[(dec, crc)]
        canon[i] = lead if chunk_of[lead] == chunk_of[i] else i
        if b >= nbase:
            if canon[i] != i:
                merged, mbytes = merged + 1, mbytes + size
            elif lead != i:
                coll += 1
    # the new streams in order: what each adds, admission, the pack, the recipes
    uniq = nbytes = ndec = nsegs = live = 0
    packed = {}                                                          # canonical new row -> its decoded offset in the pack
    pack, index = [M.STREAM_ID], dict(first=[0, 0], start=[], pos=[], total=[0], tail=[O.OK])
    segs = dict(first=[0], stream=[], off=[], len=[])
    need = [0, 10, 0]
    open_ = True                                                         # no stream missed a bound so far
    for b in range(nbase, ns):
        if status[b] == O.OK:
            mine, adds, u, ub, ud = [], [], uniq, nbytes, ndec
            place = dict(packed)
            for i, pos, size, dec, crc in rows[b]:
                if dec == 0:
                    continue
                live += 1
                c = canon[i]
                if c == i:
                    place[i] = ud
                    adds.append((i, ud, 10 + ub))
                    u, ub, ud = u + 1, ub + size, ud + dec
                cb = info[c][0]
                src, off = (cb, ix["start"][c]) if cb < nbase else (nbase, place[c])
                if mine and mine[-1][0] == src and mine[-1][1] + mine[-1][2] == off:
                    mine[-1][2] += dec
                else:
                    mine.append([src, off, dec])
            need = [u, 10 + ub, nsegs + len(mine)]
            fits = u <= max_entries and 10 + ub <= out_cap and nsegs + len(mine) <= max_segs
            nsegs += len(mine)
            uniq, nbytes, ndec, packed = u, ub, ud, place
            if open_ and fits:
                for i, start, at in adds:
                    pack.append(chunk_of[i])
                    index["start"].append(start)
                    index["pos"].append(at)
                index["first"][1], index["total"][0] = uniq, ndec
                for src, off, ln in mine:
                    segs["stream"].append(src)
                    segs["off"].append(off)
                    segs["len"].append(ln)
            else:
                open_ = False
                status[b] = O.ERR_OUTPUT_TOO_SMALL
        segs["first"].append(len(segs["stream"]))
    room = out_cap >= 10
    pack = b"".join(pack) if room else None
    if not room:
        index["tail"] = [O.ERR_OUTPUT_TOO_SMALL]
    result = [need[0], need[1], need[2], sum(1 for s in status if s == O.OK), live, merged, coll, mbytes]
    assert result[4] == result[0] + result[5]
    return dict(status=status, canon=canon, out_len=len(pack) if room else 0, pack=pack, index=index, segs=segs, result=result)


def needs(streams, ix, nbase: int = 0):
    """-> (max_entries, max_segs, out_cap) that admit every stream: the sizing call."""
    res = dedup_plan(streams, ix, nbase, 0, 0, 0)["result"]
    return res[0], res[2], res[1]


def sources(streams, ix, nbase: int, pack: bytes, pack_index):
    """The batch a recipe is composed from: the base streams, then the pack as source nbase: -> (streams, index)."""
    ne = nentries_of(ix)
    f0 = [min(v, ne) for v in ix["first"][:nbase + 1]]
    out = dict(first=[0], start=[], pos=[], total=list(ix["total"][:nbase]) + [pack_index["total"][0]],
               tail=list(ix["tail"][:nbase]) + [pack_index["tail"][0]])
    for b in range(nbase):
        out["start"] += ix["start"][f0[b]:f0[b + 1]]
        out["pos"] += ix["pos"][f0[b]:f0[b + 1]]
        out["first"].append(len(out["start"]))
    out["start"] += pack_index["start"]
    out["pos"] += pack_index["pos"]
    out["first"].append(len(out["start"]))
    return list(streams[:nbase]) + [pack], out


# ---- forged collisions ---------------------------------------------------------------------------------------------------------------------------
def forge_collision(raw: bytes, at: int = 0, flip: int = 1) -> bytes:
    """Another payload of the same length and the same CRC-32C: byte `at` (below len - 4) xor flip, and the last four bytes fixed up.  CRC is
    linear: crc(a ^ d) = crc(a) ^ crc0(d) for a difference d of that length, crc0 the register run from zero with no final xor.  The
    register after the part of d in front of its last four bytes is a word w, and four more bytes equal to w (little-endian) run it to
    zero -- no search."""
    n = len(raw)
    assert n >= 5 and 0 <= at < n - 4 and 0 < flip < 256
    d = bytearray(n - 4)
    d[at] = flip
    w = O.crc32c(bytes(d)) ^ O.crc32c(bytes(n - 4))                      # crc0 of the difference's front part
    d += w.to_bytes(4, "little")
    return bytes(x ^ y for x, y in zip(raw, d))


# ---- the plan check program (tests/abi/frame_dedup_plan_check.hip) ---------------------------------------------------------------------------------
M64 = U64


def key_of(dec: int, crc: int) -> int:
    return (dec << 32) | crc


def slots_of(ne: int) -> int:
    t = 64
    while t < 2 * ne:
        t <<= 1
    return t


def slot_of(key: int, mask: int) -> int:
    """The finaliser of splitmix64, masked."""
    h = key
    h ^= h >> 30
    h = h * 0xBF58476D1CE4E5B9 & M64
    h ^= h >> 27
    h = h * 0x94D049BB133111EB & M64
    h ^= h >> 31
    return h & mask


def begins(first: int, psrc: int, poff: int, plen: int, src: int, off: int) -> bool:
    return bool(first) or psrc != src or (poff + plen) & U64 != off


def write_cases(path: str, keys, runs, streams, indexes):
    """keys: (dec, crc, nentries); runs: (first, canon stream, nbase, canon start, canon packed, prev src, prev off, prev len); then the
    streams and, per index (any lists at all), the verdict of every stream."""
    ns = len(streams)
    with open(path, "wb") as f:
        f.write(struct.pack("<4Q", len(keys), len(runs), ns, len(indexes)))
        for q in keys:
            f.write(struct.pack("<3Q", *q))
        for q in runs:
            f.write(struct.pack("<8Q", *[int(v) & U64 for v in q]))
        for s in streams:
            f.write(struct.pack("<Q", len(s)))
            f.write(s)
        for ix in indexes:
            ne = nentries_of(ix)
            f.write(struct.pack("<Q", ne))
            for key, n in (("first", ns + 1), ("total", ns), ("tail", ns), ("start", ne), ("pos", ne)):
                assert len(ix[key]) >= n
                f.write(struct.pack("<%dQ" % n, *[int(v) & U64 for v in ix[key][:n]]))


def check_lines(keys, runs, streams, indexes):
    """What the plan check program must print for write_cases' input (after its own lines: the compare and the table against brute force)."""
    lines = []
    for dec, crc, ne in keys:
        t = slots_of(ne)
        lines.append("K %d %d %d" % (key_of(dec, crc), t, slot_of(key_of(dec, crc), t - 1)))
    for first, cs, nbase, cstart, cpacked, psrc, poff, plen in runs:
        src, off = (cs, cstart) if cs < nbase else (nbase, cpacked)
        lines.append("B %d %d %d" % (src, off, int(begins(first, psrc, poff, plen, src, off))))
    for ix in indexes:
        status, rows = verdicts(streams, ix)
        lines.append("V" + "".join(" %d:%d:%d" % (st, len(r), sum(q[2] for q in r)) for st, r in zip(status, rows)))
    return lines


# ---- cases the CPU and the GPU tests share -----------------------------------------------------------------------------------------------------------
def stream_of_chunks(chunks) -> bytes:
    return M.STREAM_ID + b"".join(chunks)


def raw_chunk(raw: bytes) -> bytes:
    """A data chunk of type 0x01 (uncompressed)."""
    return M.data_chunk(raw, compressed=False)


def content_defined(blobs, window: int, max_bytes: int, variant: int = O.HASH_CRC32C):
    """frame_encode_content_defined on the CPU: -> the streams."""
    import frame_cuts_model as F
    first, cuts = [0], []
    for x in blobs:
        cuts += F.cuts_of(x, window, max_bytes)[0]
        first.append(len(cuts))
    got = F.encode_at_cuts(blobs, first, cuts, variant)
    assert got["status"] == [O.OK] * len(blobs)
    return got["streams"]


def run_cases(rng, variant: int = O.HASH_CRC32C):
    """name -> (streams, nbase): the run-merging shapes of the recipes."""
    def piece(n):
        return bytes(rng.integers(0, 256, n, dtype="uint8"))
    a, b, c, d, e = (M.data_chunk(piece(n) + bytes(40), True, variant) for n in (300, 500, 77, 1200, 64))
    return {
        "all_unique_is_one_segment": ([stream_of_chunks([a, b, c, d])], 0),
        "abab": ([stream_of_chunks([a, b, a, b])], 0),
        "run_continues_from_the_previous_stream": ([stream_of_chunks([a, b]), stream_of_chunks([c, d, a])], 0),
        "run_passes_from_base_into_pack": ([stream_of_chunks([a, b]), stream_of_chunks([a, b, c, d])], 1),
        "duplicate_of_the_middle_of_a_base_stream": ([stream_of_chunks([a, b, c, d]), stream_of_chunks([e, b, c, e, c])], 1),
        "base_only": ([stream_of_chunks([a, b, a]), stream_of_chunks([b, c])], 2),
    }


def foreign_streams(html: bytes):
    """Streams no encoder of this project writes: zero-length rows and skippable chunks between data chunks; the same content twice."""
    a, b, c = html[:1000], html[1000:1700], html[1700:3000]
    skip, pad, zero = M.chunk(0x80, b"note"), M.chunk(0xFE, bytes(21)), M.data_chunk(b"", compressed=False)
    ch = M.data_chunk
    return [M.STREAM_ID + skip + ch(a) + pad + ch(b) + skip + M.STREAM_ID + ch(c) + skip,
            M.STREAM_ID + zero + ch(a) + zero + zero + ch(b) + ch(c) + zero,
            M.STREAM_ID + ch(c) + zero + ch(a)]


def unsound_indexes(ix, streams, rng):
    """name -> an index that does not hold for the streams (copies; ix itself is sound)."""
    def copy():
        return {k: list(v) for k, v in ix.items() if k != "result"}
    ns, ne = len(streams), nentries_of(ix)
    out = {}
    k = copy(); k["tail"][0] = O.ERR_CRC_MISMATCH; out["a_tail_that_is_not_ok"] = k
    k = copy(); k["tail"][ns - 1] = 77; out["a_tail_that_is_no_status"] = k
    k = copy(); k["tail"][0] = -3; out["a_negative_tail"] = k
    k = copy(); k["first"][1] = k["first"][2] + 1 if ns > 1 else ne + 5; out["first_runs_backwards"] = k
    k = copy(); k["first"] = [0] + [ne] * ns; k["first"][1:ns] = [ne // 2] * (ns - 1); k["first"][2 if ns > 2 else 1] = 1; out["first_below_an_earlier_one"] = k
    k = copy(); k["first"] = [v + 10 ** 12 for v in k["first"]]; k["first"][0] = 0; out["first_past_nentries"] = k
    k = copy(); k["pos"][ne // 2] = len(streams[0]) + (1 << 40); out["a_position_outside_in_len"] = k
    k = copy(); k["pos"][0] = U64; out["a_position_of_all_ones"] = k
    k = copy(); k["pos"][ne - 1] = k["pos"][ne - 1] + 1; out["a_position_inside_a_chunk"] = k
    k = copy(); k["start"][1] = k["start"][1] + 1; out["a_start_off_by_one"] = k
    k = copy(); k["total"][ns - 1] = k["total"][ns - 1] + 1; out["a_total_off_by_one"] = k
    if ne > 2:
        k = copy(); k["pos"][1], k["pos"][2] = k["pos"][2], k["pos"][1]; out["positions_swapped"] = k
    k = copy()
    for key in ("first", "start", "pos", "total"):
        k[key] = [int(v) for v in rng.integers(0, 1 << 63, len(k[key]), dtype="uint64") * 2 + rng.integers(0, 2, len(k[key]), dtype="uint64")]
    k["tail"] = [int(v) - (1 << 31) for v in rng.integers(0, 1 << 32, ns, dtype="uint64")]
    out["random_words"] = k
    k = copy()
    for key in ("start", "pos"):
        k[key] = [int(v) for v in rng.integers(0, 4000, len(k[key]))]
    out["random_small_words"] = k
    return out

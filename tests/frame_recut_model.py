"""Pure-Python statement of include/snappier_hip_frame_recut.h (snp_frame_recut_indexed_batch): framed streams kept with their chunk index brought
to the pieces of a caller's cut list -- what the encoder at given cuts writes for their decoded bytes and that list.  The planning half is a
transliteration of csrc/frame_recut_device.h on top of frame_rechunk_model.py (the verdict of a stream, its rows), frame_index_model.py and
frame_buffers_model.hop: both the index and the list are untrusted input, so it is clamp for clamp and probe for probe, and it also says what the
header does with arrays filled with anything at all.  The rest states the contract from the header's text: clean and dirty rows, kept and
rebuilt pieces (the rebuilt pieces taken one after the other from the decoded dirty rows, with no map between the two), the streams that are
left alone, the in-order admission by max_slots / the one staging budget / max_entries, out_cap, the verdicts, the new index, out_bound and
d_result.  The CPU and the GPU tests share it."""
import struct

import frame_buffers_model as M
import frame_chunked_model as K
import frame_cuts_model as C
import frame_index_model as X
import frame_range_model as R
import frame_rechunk_model as RC
import oracle as O

U64 = R.U64
REWRITE_ALL = 1
MAX_DEC = 65536
MAX_COUNT = RC.MAX_COUNT
MAX_STAGE = RC.MAX_STAGE


# ---- the planning (csrc/frame_recut_device.h) ---------------------------------------------------------------------------------------------------
def clean(cuts, lo: int, hi: int, total: int, s: int, ln: int) -> bool:
    """rx_clean: one search in cuts[lo : hi] (any list at all)."""
    if ln == 0:
        return False
    j = X.first_where(lo, hi, lambda k: cuts[k] > s)
    if s != 0 and (j == lo or cuts[j - 1] != s):
        return False
    return (cuts[j] if j < hi else total) == s + ln


def first_piece_from(cuts, lo: int, hi: int, at: int) -> int:
    """ec_first_piece_from."""
    return 0 if at == 0 else X.first_where(lo, hi, lambda k: cuts[k] >= at) - lo + 1


def row(ix, f0: int, f1: int, total: int, n: int, cuts, lo: int, hi: int, rewrite: bool, i: int, hop_at):
    """rx_row: -> dict of clean, start, len, pos, hop, or None for a row that fails its check."""
    s, e, pos = ix["start"][i], X.row_end(ix, f1, total, i), ix["pos"][i]
    if (i == f0 and s != 0) or e < s or pos >= n:
        return None
    h = hop_at(pos)
    if h.kind != "data" or e - s != h.dec:
        return None
    if i + 1 < f1 and ix["pos"][i + 1] < h.next:
        return None
    cl = not rewrite and clean(cuts, lo, hi, total, s, e - s)
    if not cl and e - s > MAX_DEC:
        return None
    return dict(clean=cl, start=s, len=e - s, pos=pos, hop=h)


def plan(ix, b: int, n: int, cut_first, cuts, ncuts: int, rewrite: bool, has_ident: bool, hop_at):
    """rx_plan: -> dict of status, work, f0, rows, dirty, dbytes, pieces, rebuilt, copied, kept, cbytes, bound, lo, hi and the dirty rows as the
    chunk table takes them (drows)."""
    f0, rows = RC.rows_of(ix, b)
    lo, hi = cut_first[b], cut_first[b + 1]
    k = dict(status=RC.begin(ix, b), work=False, f0=f0, rows=rows, dirty=0, dbytes=0, pieces=0, rebuilt=0, copied=0, kept=0, cbytes=0, bound=0,
             lo=lo, hi=hi, drows=[])
    if k["status"] != O.OK:
        return k
    total = ix["total"][b]
    k["status"] = O.ERR_BAD_ARG
    if lo > hi or hi > ncuts:                                           # (neither the list nor a row is looked at)
        return k
    badlist, prev, pstride = False, 0, 0
    for i in range(lo, hi):
        prev, cut = (cuts[i - 1] if i > lo else 0), cuts[i]
        if not (prev < cut < total and cut - prev <= MAX_DEC):
            badlist = True
        else:
            pstride += K.stride(cut - prev)
    last = cuts[hi - 1] if hi > lo else 0
    if (total - last) & U64 > MAX_DEC:
        badlist = True
    elif total:
        pstride += K.stride(total - last)
    f1 = f0 + rows
    bad = loose = False
    dirty = dbytes = ncl = kept = cstride = 0
    drows = []
    for i in range(f0, f1):
        r = row(ix, f0, f1, total, n, cuts, lo, hi, rewrite, i, hop_at)
        if r is None:
            bad = True
            continue
        h = r["hop"]
        if r["clean"]:
            ncl += 1
            kept += h.next - r["pos"]
            cstride += K.stride(r["len"])
        else:
            dirty += 1
            dbytes += r["len"]
            loose = True
            drows.append((h.type, r["pos"] + 8, h.body_len, h.crc, r["start"], h.dec))
        if (i == f0 and r["pos"] != 10) or ((ix["pos"][i + 1] != h.next) if i + 1 < f1 else (h.next != n)):
            loose = True
    if badlist or bad or (rows == 0 and total != 0):
        return k
    k["status"] = O.OK
    if not rewrite and not loose and has_ident and (rows != 0 or n == 10):
        return k
    pieces = hi - lo + 1 if total else 0
    copied = min(ncl, pieces)
    k.update(work=True, dirty=dirty, dbytes=dbytes, pieces=pieces, copied=copied, rebuilt=pieces - copied, kept=kept,
             cbytes=max(pstride - cstride, 0), bound=(10 + kept + 8 * (pieces - copied) + dbytes) & U64, drows=drows)
    return k


def counts(k):
    """rx_count_dirty, _slots, _stage, _dec, _rows."""
    w = k["work"]
    stage = (k["dbytes"] + k["cbytes"] if k["dbytes"] < MAX_STAGE and k["cbytes"] < MAX_STAGE - k["dbytes"] else MAX_STAGE) if w else 0
    return (min(k["dirty"], MAX_COUNT) if w else 0, min(k["rebuilt"], MAX_COUNT) if w else 0, stage, min(k["dbytes"], MAX_STAGE) if w else 0,
            min(max(k["pieces"], k["rows"]) if w else k["rows"], MAX_COUNT))


def piece(ix, f0: int, f1: int, total: int, cuts, lo: int, hi: int, rewrite: bool, j: int):
    """rx_piece: -> (kept, row, at, len)."""
    at = cuts[lo + j - 1] if j else 0
    ln = ((cuts[lo + j] if lo + j < hi else total) - at) & 0xFFFFFFFF
    r = X.first_where(f0, f1, lambda i: X.row_end(ix, f1, total, i) > at)
    if r >= f1:
        return False, r, at, ln
    s, e = ix["start"][r], X.row_end(ix, f1, total, r)
    return (not rewrite and s == at and e == at + ln), r, at, ln


def stage_bound(dbytes: int, rebuilt: int) -> int:
    """The bound the header gives a caller for stage_cap."""
    return 2 * dbytes + dbytes // 6 + 69 * rebuilt


# ---- the whole call ----------------------------------------------------------------------------------------------------------------------------
def recut_plan(streams, ix, cut_first, cuts, flags: int = 0, caps=None, max_slots: int | None = None, stage_cap: int | None = None,
               max_entries: int | None = None, variant: int = O.HASH_CRC32C, ncuts: int | None = None):
    """snp_frame_recut_indexed_batch.  None: a bound that admits all.
    -> dict of status, out_len, streams (the new stream, None unless written), alone, index (the new one), out_bound, result [8], plans."""
    assert flags in (0, REWRITE_ALL)
    rewrite = flags == REWRITE_ALL
    ns = len(streams)
    ncuts = len(cuts) if ncuts is None else ncuts
    BIG = 1 << 62
    max_slots = BIG if max_slots is None else max_slots
    stage_cap = BIG if stage_cap is None else stage_cap
    max_entries = BIG if max_entries is None else max_entries
    caps = [BIG] * ns if caps is None else caps
    pl = [plan(ix, b, len(s), cut_first, cuts, ncuts, rewrite, RC.ident(s), lambda pos, s=s: M.hop(s, pos)) for b, s in enumerate(streams)]
    dirty = slots = stage = nrows = copied = rebuilt = 0
    status, out_len, new, bound, alone = [], [], [None] * ns, [], []
    new_start, new_pos = [[] for _ in range(ns)], [[] for _ in range(ns)]
    for b, k in enumerate(pl):
        s = streams[b]
        cd, cs, cg, _, cr = counts(k)
        dirty, slots, stage, nrows = dirty + cd, slots + cs, stage + cg, nrows + cr
        status.append(k["status"])
        out_len.append(0)
        bound.append(k["bound"] if k["work"] else 0)
        alone.append(k["status"] == O.OK and not k["work"])
        if not k["work"]:
            continue
        status[b] = O.ERR_OUTPUT_TOO_SMALL
        if dirty > max_slots or slots > max_slots or stage > stage_cap or nrows > max_entries:
            continue
        staged, failed = [], O.OK
        for r in k["drows"]:                                            # the first failing chunk's status
            failed, dec = R.chunk_result(s, r)
            if failed != O.OK:
                break
            staged.append(dec)
        if failed != O.OK:
            status[b], bound[b] = failed, 0
            continue
        staged = b"".join(staged)
        assert len(staged) == k["dbytes"]
        f0, f1, total = k["f0"], k["f0"] + k["rows"], ix["total"][b]
        out, at, used, m = [M.STREAM_ID], 10, 0, 0
        for j in range(k["pieces"]):
            keep, r, start, ln = piece(ix, f0, f1, total, cuts, k["lo"], k["hi"], rewrite, j)
            if keep:
                c = s[ix["pos"][r]:M.hop(s, ix["pos"][r]).next]
            else:
                c = K.chunks_of(staged[used:used + ln], ln, variant)[0]     # the rebuilt pieces lie one behind the other
                used += ln
                m += 1
            new_start[b].append(start)
            new_pos[b].append(at)
            out.append(c)
            at += len(c)
        assert m == k["rebuilt"] and used == k["dbytes"]
        assert k["dbytes"] + k["cbytes"] <= stage_bound(k["dbytes"], k["rebuilt"])
        if at > caps[b]:
            continue
        new[b] = b"".join(out)
        assert len(new[b]) == at <= k["bound"]
        status[b], out_len[b] = O.OK, at
        copied, rebuilt = copied + k["copied"], rebuilt + k["rebuilt"]
    first, start, pos, total, tail = [0], [], [], [], []
    for b, k in enumerate(pl):
        f0, f1 = k["f0"], k["f0"] + k["rows"]
        if new[b] is None:
            start += ix["start"][f0:f1]
            pos += ix["pos"][f0:f1]
        else:
            start += new_start[b]
            pos += new_pos[b]
        first.append(len(start))
        total.append(ix["total"][b])
        tail.append(O.OK if new[b] is not None else ix["tail"][b])
    index = dict(first=[min(f, max_entries) for f in first], start=start[:max_entries], pos=pos[:max_entries], total=total, tail=tail)
    return dict(status=status, out_len=out_len, streams=new, alone=alone, index=index, out_bound=bound, plans=pl,
                result=[max(dirty, slots) & U64, sum(out_len) & U64, stage & U64, sum(1 for x in new if x is not None), nrows & U64, sum(alone),
                        copied, rebuilt])


def needs(streams, ix, cut_first, cuts, flags: int = 0):
    """-> (max_slots, stage_cap, max_entries) that admit every stream: the sizing call."""
    res = recut_plan(streams, ix, cut_first, cuts, flags, caps=[0] * len(streams), max_slots=0, stage_cap=0, max_entries=0)["result"]
    return res[0], res[2], res[4]


after = RC.after
same_index = RC.same_index


def lists(per_stream):
    """The CSR form of one cut list per stream: -> (cut_first, cuts)."""
    first, cuts = [0], []
    for c in per_stream:
        cuts += list(c)
        first.append(len(cuts))
    return first, cuts


def content_lists(raws, w: int, mx: int):
    return lists([C.cuts_of(a, w, mx)[0] for a in raws])


def stream_at(raw: bytes, cuts, variant: int = O.HASH_CRC32C) -> bytes:
    """What the encoder at given cuts writes for one buffer."""
    return C.encode_at_cuts([raw], [0, len(cuts)], list(cuts), variant)["streams"][0]


# ---- cases the CPU and the GPU tests share ---------------------------------------------------------------------------------------------------------
def directed(html: bytes):
    """name -> (stream, decoded bytes, cuts): the directed lists of the header's rule, on streams of a few KiB."""
    def ch(piece: bytes) -> bytes:                                      # the chunk every encoder of this project writes for the piece
        return K.chunks_of(piece, len(piece))[0]

    a = html[:4000]
    zero, skip, pad = M.data_chunk(b"", compressed=False), M.chunk(0x80, b"note"), M.chunk(0xFE, bytes(21))
    parts = [a[0:700], a[700:1000], a[1000:1900], a[1900:2600], a[2600:4000]]
    plain = M.STREAM_ID + b"".join(ch(p) for p in parts)
    big = (html * 3)[:65536 + 1 + 300]
    return {
        "dirty_row_spans_pieces": (M.STREAM_ID + ch(a[:3000]) + ch(a[3000:]), a, [500, 1100, 2000, 3000]),
        "dirty_rows_make_one_piece": (plain, a, [1900, 2600]),
        "clean_between_dirty": (plain, a, [300, 1000, 1900, 3000]),
        "start_matches_end_does_not": (plain, a, [700, 900, 1900, 2600]),
        "end_matches_start_does_not": (plain, a, [800, 1000, 1900, 2600]),
        "one_byte_pieces": (plain, a, [1, 2, 700, 701, 1000, 1900, 2600, 3999]),
        "a_full_size_piece": (M.STREAM_ID + ch(big[:1]) + ch(big[1:40000]) + ch(big[40000:65537]) + ch(big[65537:]), big, [1, 65537]),
        "a_full_size_piece_kept": (M.STREAM_ID + ch(big[:1]) + ch(big[1:65537]) + ch(big[65537:65600]) + ch(big[65600:]), big, [1, 65537]),
        "short_last_piece_kept": (plain, a, [650, 2600]),
        "zero_length_rows": (M.STREAM_ID + zero + ch(parts[0]) + ch(parts[1]) + zero + zero + ch(parts[2]) + ch(parts[3]) + ch(parts[4]) + zero, a,
                             [700, 1000, 1500, 2600]),
        "skippable_and_padding_dropped": (M.STREAM_ID + skip + ch(parts[0]) + pad + ch(parts[1]) + M.STREAM_ID + ch(parts[2]) + ch(parts[3]) +
                                          ch(parts[4]) + skip, a, [700, 1000, 1900, 2600]),
        "one_piece": (plain, a, []),
        "empty_in_len_10": (M.STREAM_ID, b"", []),
        "empty_in_len_0": (b"", b"", []),
        "only_zero_length_rows": (M.STREAM_ID + zero + zero, b"", []),
        "canonical_already": (M.STREAM_ID + b"".join(ch(p) for p in parts), a, [700, 1000, 1900, 2600]),
    }


def bad_lists(total: int):
    """name -> (cut_first of a batch of one stream, cuts, ncuts): every rejection of the list, for a stream that decodes to total >= 3000 bytes."""
    return {
        "a_cut_of_zero": ([0, 2], [0, 1000], 2),
        "a_cut_at_total": ([0, 2], [1000, total], 2),
        "a_cut_past_total": ([0, 2], [1000, total + 5], 2),
        "repeated_cuts": ([0, 3], [1000, 1000, 2000], 3),
        "descending_cuts": ([0, 3], [2000, 1000, 2500], 3),
        "cut_first_decreasing": ([2, 1], [1000, 2000], 2),
        "cut_first_past_ncuts": ([0, 3], [1000, 2000, 2500], 2),
        "all_past_ncuts": ([5, 6], [1000, 2000], 2),
    }


def end_to_end(html: bytes, w: int = 32, mx: int = 256, variant: int = O.HASH_CRC32C):
    """name -> (the edited stream, its decoded bytes): content-defined streams of about 8 KiB after an insert mid-chunk, a delete across chunks,
    an append and a three-edit script, each through the model of the call that makes the edit."""
    import frame_append_model as A
    import frame_edit_model as E
    import frame_splice_model as S

    out = {}
    base = bytes((v * 7 + i * i // 3 + (i >> 5)) & 0xFF for i, v in enumerate(html[100:8300]))     # non-constant
    cuts = C.cuts_of(base, w, mx)[0]
    s0 = stream_at(base, cuts, variant)
    ix0 = X.build_index([s0])
    mid = (cuts[20] + cuts[21]) // 2
    for name, (off, dele, src) in {"insert_mid_chunk": (mid, 0, html[5000:5037]), "delete_across_chunks": (cuts[30] + 3, cuts[33] - cuts[30], b"")}.items():
        got = S.splice_plan([s0], ix0, [(off, dele)], [src], 256, variant=variant)
        assert got["status"] == [O.OK]
        out[name] = (got["streams"][0], S.edited(base, off, dele, src))
    src = html[6000:6700]
    got = A.append_plan([s0], ix0, [src], 256, variant=variant)
    assert got["status"] == [O.OK]
    out["append"] = (got["streams"][0], base + src)
    script = [(cuts[10] + 1, 0, 11), (cuts[40] + 2, 40, 5), (cuts[70], 300, 0)]
    srcs = [html[7000 + 50 * i:7000 + 50 * i + ins] for i, (_, _, ins) in enumerate(script)]
    got = E.edit_plan([s0], ix0, [0, len(script)], [(o, d) for o, d, _ in script], srcs, 256, variant=variant)
    assert got["status"] == [O.OK]
    out["three_edits"] = (got["streams"][0], E.applied(base, [(o, d, x) for (o, d, _), x in zip(script, srcs)]))
    return out


# ---- the cases of the planning check (tests/abi/frame_recut_plan_check.hip) ----------------------------------------------------------------------
def plan_line(k, ix, total: int, cuts, rewrite: bool) -> str:
    """What the planning header must give for one stream, as the check program prints it: the plan, what it asks of the bounds, the first and
    the last piece (kept, row, at, len), and the first and the last rebuilt piece: (piece, where it lies among the decoded dirty rows, len)."""
    p0 = p1 = (0, 0, 0, 0)
    s0 = s1 = (0, 0, 0)
    if k["work"] and k["pieces"]:
        f0, f1 = k["f0"], k["f0"] + k["rows"]
        ps = [piece(ix, f0, f1, total, cuts, k["lo"], k["hi"], rewrite, j) for j in range(k["pieces"])]
        p0, p1 = ps[0], ps[-1]
        place, slots = 0, []
        for j, p in enumerate(ps):
            if not p[0]:
                slots.append((j, place, p[3]))
                place += p[3]
        if slots:
            s0, s1 = slots[0], slots[-1]
    return "%d %d %d %d %d %d %d %d %d %d %d %d | %d %d %d %d %d | %d %d %d %d %d %d %d %d | %d %d %d %d %d %d" % (
        k["status"], k["work"], k["f0"], k["rows"], k["dirty"], k["dbytes"], k["pieces"], k["rebuilt"], k["copied"], k["kept"], k["cbytes"],
        k["bound"] & U64, *counts(k), *[int(v) for v in p0], *[int(v) for v in p1], *s0, *s1)


def plan_lines(ix, streams, cut_first, cuts, ncuts: int, flags: int):
    rewrite = flags == REWRITE_ALL
    return [plan_line(plan(ix, b, len(s), cut_first, cuts, ncuts, rewrite, RC.ident(s), lambda pos, s=s: M.hop(s, pos)), ix, ix["total"][b], cuts,
                      rewrite) for b, s in enumerate(streams)]


NUMERIC_KEYS = ("n", "flags", "total", "tail", "rows", "ident", "start0", "pos0", "kind0", "size0", "dec0", "start1", "pos1", "kind1", "size1", "dec1",
                "ncuts", "cut0", "cut1", "cut2")


def numeric_line(case) -> str:
    """case: dict of NUMERIC_KEYS -- a stream of n bytes that is too long to hold, given as up to two index rows, the headers they point at
    (kind: 0 data, 1 skippable) and up to three cuts."""
    c = case
    rows, nc = c["rows"], c["ncuts"]
    ix = dict(first=[0, rows], start=[c["start0"], c["start1"]][:rows], pos=[c["pos0"], c["pos1"]][:rows], total=[c["total"]], tail=[c["tail"]])
    cuts = [c["cut0"], c["cut1"], c["cut2"]][:nc]

    def hop_at(pos):
        j = 0 if pos == c["pos0"] else 1
        size = c["size%d" % j]
        return M.Hop("data" if c["kind%d" % j] == 0 else "skip", pos + 4 + size, type=1, body_len=size - 4, dec=c["dec%d" % j])

    rewrite = c["flags"] == REWRITE_ALL
    return plan_line(plan(ix, 0, c["n"], [0, nc], cuts, nc, rewrite, bool(c["ident"]), hop_at), ix, c["total"], cuts, rewrite)


def write_cases(path: str, streams, cases, numeric):
    """The input of the check program: the streams; every case -- an index and a cut list (any lists at all), ncuts as the call is told, and flags;
    then the numeric cases, twenty words each."""
    ns = len(streams)
    with open(path, "wb") as f:
        f.write(struct.pack("<Q", ns))
        for s in streams:
            f.write(struct.pack("<Q", len(s)))
            f.write(s)
        f.write(struct.pack("<Q", len(cases)))
        for ix, cut_first, cuts, ncuts, flags in cases:
            ne = min(len(ix["start"]), len(ix["pos"]))
            assert ncuts <= len(cuts)
            f.write(struct.pack("<3Q", ne, ncuts, flags))
            for arr, n in ((ix["first"], ns + 1), (ix["total"], ns), (ix["tail"], ns), (ix["start"], ne), (ix["pos"], ne), (cut_first, ns + 1),
                           (cuts, ncuts)):
                assert len(arr) >= n
                f.write(struct.pack("<%dQ" % n, *[int(v) & U64 for v in arr[:n]]))
        f.write(struct.pack("<Q", len(numeric)))
        for c in numeric:
            f.write(struct.pack("<%dQ" % len(NUMERIC_KEYS), *[int(c[key]) & U64 for key in NUMERIC_KEYS]))

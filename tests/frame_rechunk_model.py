"""Pure-Python statement of include/snappier_hip_frame_rechunk.h (snp_frame_rechunk_indexed_batch): framed streams kept with their chunk index
brought to canonical form -- what the chunked encoder writes for their decoded bytes with chunk_bytes.  The planning half is a transliteration
of csrc/frame_rechunk_device.h on top of frame_index_model.py and frame_buffers_model.hop (the index is untrusted input: clamp for clamp and
probe for probe, so that it also says what the header does with an index filled with anything at all); the rest states the contract: clean and
dirty rows, kept and rebuilt pieces (frame_chunked_model.chunks_of: slots of the chunked encode), the streams that are left alone, the in-order
admission by max_slots / stage_cap / max_entries, out_cap, the verdicts, the new index, out_bound and d_result.  The CPU and the GPU tests
share it."""
import struct

import frame_buffers_model as M
import frame_chunked_model as K
import frame_index_model as X
import frame_range_model as R
import oracle as O

U64 = R.U64
REWRITE_ALL = 1
MAX_DEC = 65536
MAX_COUNT = 1 << 32
MAX_STAGE = 1 << 48
CHUNK_SIZES = [1, 63, 64, 65, 4096, 65536]


# ---- the planning (csrc/frame_rechunk_device.h) ------------------------------------------------------------------------------------------------
def rows_of(ix, b: int):
    """fr_rows: -> (f0, rows), inside nentries whatever idx_first holds."""
    ne = min(len(ix["start"]), len(ix["pos"]))
    a, e = min(ix["first"][b], ne), min(ix["first"][b + 1], ne)
    return a, max(e - a, 0)


def begin(ix, b: int) -> int:
    """fr_begin."""
    walk = ix["tail"][b]
    if walk < O.OK or walk > O.ERR_TRUNCATED_STREAM:
        return O.ERR_BAD_ARG
    if walk != O.OK:
        return walk
    ne = min(len(ix["start"]), len(ix["pos"]))
    return O.ERR_BAD_ARG if min(ix["first"][b + 1], ne) < min(ix["first"][b], ne) else O.OK


def ident(s: bytes) -> bool:
    return s[:10] == M.STREAM_ID


def clean(start: int, ln: int, at_end: bool, cb: int) -> bool:
    return ln > 0 and start % cb == 0 and (ln == cb or (ln <= cb and at_end))


def row(ix, f0: int, f1: int, total: int, n: int, cb: int, rewrite: bool, i: int, hop_at):
    """fr_row: -> dict of clean, start, len, pos, hop, or None for a row that fails its check."""
    s, e, pos = ix["start"][i], X.row_end(ix, f1, total, i), ix["pos"][i]
    if (i == f0 and s != 0) or e < s or pos >= n:
        return None
    h = hop_at(pos)
    if h.kind != "data" or e - s != h.dec:
        return None
    if i + 1 < f1 and ix["pos"][i + 1] < h.next:
        return None
    cl = not rewrite and clean(s, e - s, e == total, cb)
    if not cl and e - s > MAX_DEC:
        return None
    return dict(clean=cl, start=s, len=e - s, pos=pos, hop=h)


def plan(ix, b: int, n: int, cb: int, rewrite: bool, has_ident: bool, hop_at):
    """fr_plan: -> dict of status, work, last, f0, rows, dirty, dbytes, pieces, rebuilt, kept, bound, and the dirty rows as the chunk table takes
    them (drows).  hop_at(pos) -> M.Hop of the header at pos < n."""
    f0, rows = rows_of(ix, b)
    k = dict(status=begin(ix, b), work=False, last=False, f0=f0, rows=rows, dirty=0, dbytes=0, pieces=0, rebuilt=0, kept=0, bound=0, drows=[])
    if k["status"] != O.OK:
        return k
    f1, total = f0 + rows, ix["total"][b]
    bad = loose = last = False
    dirty = dbytes = ncl = kept = 0
    drows = []
    for i in range(f0, f1):
        r = row(ix, f0, f1, total, n, cb, rewrite, i, hop_at)
        if r is None:
            bad = True
            continue
        h = r["hop"]
        if r["clean"]:
            ncl += 1
            kept += h.next - r["pos"]
        else:
            dirty += 1
            dbytes += r["len"]
            loose = True
            last = last or (r["len"] > 0 and r["start"] + r["len"] == total)
            drows.append((h.type, r["pos"] + 8, h.body_len, h.crc, r["start"], h.dec))
        if (i == f0 and r["pos"] != 10) or ((ix["pos"][i + 1] != h.next) if i + 1 < f1 else (h.next != n)):
            loose = True
    k["status"] = O.ERR_BAD_ARG
    if bad or (rows == 0 and total != 0):
        return k
    k["status"] = O.OK
    if not rewrite and not loose and has_ident and (rows != 0 or n == 10):
        return k
    pieces = K.nchunks(total, cb)
    k.update(work=True, last=last, dirty=dirty, dbytes=dbytes, pieces=pieces, rebuilt=pieces - ncl, kept=kept,
             bound=(10 + kept + 8 * (pieces - ncl) + dbytes) & U64, drows=drows)
    return k


def counts(k):
    """fr_count_dirty, _slots, _stage, _rows."""
    w = k["work"]
    return (min(k["dirty"], MAX_COUNT) if w else 0, min(k["rebuilt"], MAX_COUNT) if w else 0, min(k["dbytes"], MAX_STAGE) if w else 0,
            min(max(k["pieces"], k["rows"]) if w else k["rows"], MAX_COUNT))


def piece(ix, f0: int, f1: int, total: int, cb: int, rewrite: bool, j: int):
    """fr_piece: -> (kept, row, at, len)."""
    at = j * cb
    ln = min(total - at, cb)
    r = X.first_where(f0, f1, lambda i: X.row_end(ix, f1, total, i) > at)
    if r >= f1:
        return False, r, at, ln
    s, e = ix["start"][r], X.row_end(ix, f1, total, r)
    return (not rewrite and s == at and e >= s and clean(s, e - s, e == total, cb)), r, at, ln


def slot_len(k, total: int, cb: int, m: int) -> int:
    return total - (k["pieces"] - 1) * cb if k["last"] and m + 1 == k["rebuilt"] else cb


# ---- the whole call ----------------------------------------------------------------------------------------------------------------------------
def rechunk_plan(streams, ix, cb: int, flags: int = 0, caps=None, max_slots: int | None = None, stage_cap: int | None = None,
                 max_entries: int | None = None, variant: int = O.HASH_CRC32C):
    """snp_frame_rechunk_indexed_batch.  None: a bound that admits all.
    -> dict of status, out_len, streams (the new stream, None unless written), alone (left alone as canonical), index (the new one: first, start,
    pos, total, tail), out_bound, result [6]."""
    assert 1 <= cb <= MAX_DEC and flags in (0, REWRITE_ALL)
    rewrite = flags == REWRITE_ALL
    ns = len(streams)
    BIG = 1 << 62
    max_slots = BIG if max_slots is None else max_slots
    stage_cap = BIG if stage_cap is None else stage_cap
    max_entries = BIG if max_entries is None else max_entries
    caps = [BIG] * ns if caps is None else caps
    pl = [plan(ix, b, len(s), cb, rewrite, ident(s), lambda pos, s=s: M.hop(s, pos)) for b, s in enumerate(streams)]
    dirty = slots = stage = nrows = 0
    status, out_len, new, bound, alone = [], [], [None] * ns, [], []
    new_pos = [[] for _ in range(ns)]
    for b, k in enumerate(pl):
        s = streams[b]
        cd, cs, cg, cr = counts(k)
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
        out, at, m = [M.STREAM_ID], 10, 0
        for j in range(k["pieces"]):
            keep, r, _, ln = piece(ix, f0, f1, total, cb, rewrite, j)
            if keep:
                c = s[ix["pos"][r]:M.hop(s, ix["pos"][r]).next]
            else:
                assert ln == slot_len(k, total, cb, m)
                c = K.chunks_of(staged[m * cb:m * cb + ln], cb, variant)[0]
                m += 1
            new_pos[b].append(at)
            out.append(c)
            at += len(c)
        assert m == k["rebuilt"]
        if at > caps[b]:
            new_pos[b] = []
            continue
        new[b] = b"".join(out)
        assert len(new[b]) == at <= k["bound"]
        status[b], out_len[b] = O.OK, at
    first, start, pos, total, tail = [0], [], [], [], []
    for b, k in enumerate(pl):
        f0, f1 = k["f0"], k["f0"] + k["rows"]
        if new[b] is None:
            start += ix["start"][f0:f1]
            pos += ix["pos"][f0:f1]
        else:
            start += [j * cb for j in range(k["pieces"])]
            pos += new_pos[b]
        first.append(len(start))
        total.append(ix["total"][b])
        tail.append(O.OK if new[b] is not None else ix["tail"][b])
    index = dict(first=[min(f, max_entries) for f in first], start=start[:max_entries], pos=pos[:max_entries], total=total, tail=tail)
    return dict(status=status, out_len=out_len, streams=new, alone=alone, index=index, out_bound=bound,
                result=[max(dirty, slots) & U64, sum(out_len) & U64, stage & U64, sum(1 for x in new if x is not None), nrows & U64, sum(alone)])


def needs(streams, ix, cb: int, flags: int = 0):
    """-> (max_slots, stage_cap, max_entries) that admit every stream: the sizing call."""
    res = rechunk_plan(streams, ix, cb, flags, caps=[0] * len(streams), max_slots=0, stage_cap=0, max_entries=0)["result"]
    return res[0], res[2], res[4]


def after(streams, got):
    """The batch after a call: the new streams where one was written, else the old."""
    return [n if n is not None else s for s, n in zip(streams, got["streams"])]


def same_index(a, b) -> bool:
    return all(list(a[key]) == list(b[key]) for key in ("first", "start", "pos", "total", "tail"))


def data_chunk_lengths(s: bytes):
    """Decoded bytes of every data chunk of a stream, in order."""
    return [r[5] for r in R.walk(s)[0]]


# ---- cases the CPU and the GPU tests share ---------------------------------------------------------------------------------------------------------
def fragmenting_edits(cb: int, n: int):
    """name -> list of (off, del, ins) applied in a row through the splice model to a stream of n decoded bytes (n >= 5 cb): the edits that
    fragment a stream."""
    mid = cb + cb // 2
    return {
        "insert_mid_chunk": [(mid, 0, cb // 3 + 5)],
        "delete_across_chunks": [(cb // 2, 2 * cb, 0)],
        "drop_prefix_of_a_non_multiple": [(0, cb + cb // 3 + 1, 0)],
        "several_edits": [(mid, 0, 7), (3 * cb + 1, cb // 2 + 1, 3), (2, 1, 0)],
        "edit_near_the_end": [(4 * cb + cb // 2, 0, 5)],               # in the last whole chunk (an edit of the last chunk itself stays canonical)
        "append_at_total": [(n, 0, cb // 2 + 1)],
    }


def foreign_streams(html: bytes):
    """name -> (stream, decoded bytes): streams no encoder of this project writes -- skippable, padding and repeated-identifier chunks,
    zero-length data chunks, no identifier, chunks of sizes off every grid."""
    a, b, c, d = html[:1000], html[1000:1700], html[1700:3000], html[3000:3400]
    skip, pad, zero = M.chunk(0x80, b"note"), M.chunk(0xFE, bytes(21)), M.data_chunk(b"", compressed=False)
    ch = M.data_chunk
    raw = a + b + c + d
    even = [html[i:i + 500] for i in range(0, 2000, 500)]
    return {
        "non_data_between": (M.STREAM_ID + ch(a) + ch(b) + skip + pad + M.STREAM_ID + ch(c) + ch(d), raw),
        "non_data_at_both_ends": (M.STREAM_ID + skip + ch(a) + pad + ch(b) + ch(c) + M.STREAM_ID + ch(d) + skip, raw),
        "zero_length_chunks": (M.STREAM_ID + ch(a) + zero + ch(b) + zero + ch(c) + zero + ch(d) + zero, raw),
        "only_zero_length_chunks": (M.STREAM_ID + zero + zero, b""),
        "identifier_only": (M.STREAM_ID, b""),
        "identifier_twice": (M.STREAM_ID + M.STREAM_ID, b""),
        "no_identifier": (ch(a) + ch(b), a + b),
        "on_the_grid_with_a_skippable_chunk": (M.STREAM_ID + ch(even[0], False) + ch(even[1], False) + skip + ch(even[2], False) + ch(even[3], False),
                                               b"".join(even)),
        "on_the_grid_uncompressed": (M.STREAM_ID + b"".join(ch(x, compressed=False) for x in even), b"".join(even)),
    }


def unsound_indexes(ix, streams, rng):
    """frame_update_model.unsound_indexes: the thirteen."""
    import frame_update_model as U
    return U.unsound_indexes(ix, streams, rng)


# ---- the cases of the planning check (tests/abi/frame_rechunk_plan_check.hip) --------------------------------------------------------------------
def plan_line(k, ix, total: int, cb: int, rewrite: bool) -> str:
    """What the planning header must give for one stream, as the check program prints it: the plan, what it asks of the bounds, then the first
    and the last piece (kept, row, at, len) and the length of the last rebuilt slot."""
    p0 = p1 = (0, 0, 0, 0)
    last = 0
    if k["work"] and k["pieces"]:
        f0, f1 = k["f0"], k["f0"] + k["rows"]
        p0, p1 = piece(ix, f0, f1, total, cb, rewrite, 0), piece(ix, f0, f1, total, cb, rewrite, k["pieces"] - 1)
        last = slot_len(k, total, cb, k["rebuilt"] - 1) if k["rebuilt"] else 0
    return "%d %d %d %d %d %d %d %d %d %d %d | %d %d %d %d | %d %d %d %d %d %d %d %d %d" % (
        k["status"], k["work"], k["last"], k["f0"], k["rows"], k["dirty"], k["dbytes"], k["pieces"], k["rebuilt"], k["kept"], k["bound"] & U64,
        *counts(k), *[int(v) for v in p0], *[int(v) for v in p1], last)


def plan_lines(ix, streams, cb: int, flags: int):
    rewrite = flags == REWRITE_ALL
    return [plan_line(plan(ix, b, len(s), cb, rewrite, ident(s), lambda pos, s=s: M.hop(s, pos)), ix, ix["total"][b], cb, rewrite)
            for b, s in enumerate(streams)]


NUMERIC_KEYS = ("n", "cb", "flags", "total", "tail", "rows", "ident", "start0", "pos0", "kind0", "size0", "dec0", "start1", "pos1", "kind1", "size1",
                "dec1")


def numeric_line(case) -> str:
    """case: dict of NUMERIC_KEYS -- a stream of n bytes that is too long to hold, given as up to two index rows and the headers they point at
    (kind: 0 data, 1 skippable)."""
    c = case
    rows = c["rows"]
    ix = dict(first=[0, rows], start=[c["start0"], c["start1"]][:rows], pos=[c["pos0"], c["pos1"]][:rows], total=[c["total"]], tail=[c["tail"]])

    def hop_at(pos):
        j = 0 if pos == c["pos0"] else 1
        size = c["size%d" % j]
        return M.Hop("data" if c["kind%d" % j] == 0 else "skip", pos + 4 + size, type=1, body_len=size - 4, dec=c["dec%d" % j])

    rewrite = c["flags"] == REWRITE_ALL
    return plan_line(plan(ix, 0, c["n"], c["cb"], rewrite, bool(c["ident"]), hop_at), ix, c["total"], c["cb"], rewrite)


def write_cases(path: str, streams, cases, numeric):
    """The input of the check program: the streams; every case -- an index (any lists at all), chunk_bytes and flags; then the numeric cases,
    seventeen words each."""
    with open(path, "wb") as f:
        f.write(struct.pack("<Q", len(streams)))
        for s in streams:
            f.write(struct.pack("<Q", len(s)))
            f.write(s)
        f.write(struct.pack("<Q", len(cases)))
        for ix, cb, flags in cases:
            ne = min(len(ix["start"]), len(ix["pos"]))
            f.write(struct.pack("<3Q", ne, cb, flags))
            for key, n in (("first", len(streams) + 1), ("total", len(streams)), ("tail", len(streams)), ("start", ne), ("pos", ne)):
                assert len(ix[key]) >= n
                f.write(struct.pack("<%dQ" % n, *[int(v) & U64 for v in ix[key][:n]]))
        f.write(struct.pack("<Q", len(numeric)))
        for c in numeric:
            f.write(struct.pack("<%dQ" % len(NUMERIC_KEYS), *[int(c[key]) & U64 for key in NUMERIC_KEYS]))

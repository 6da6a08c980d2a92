"""Pure-Python statement of include/snappier_hip_frame_compose.h (snp_frame_compose_indexed_batch): new framed streams made of windows
("segments") of old ones that are kept with their chunk index.  Written from the header's text on top of oracle, frame_index_model (the index,
the window's rows: the read call's plan), frame_buffers_model.hop and frame_chunked_model.chunks_of (slots of the chunked encode): a segment
planned on its own -- its rows, its edges and their pieces, its kept chunks --, the outputs' segment lists (untrusted, like the index), the
in-order admission by max_slots / stage_cap / max_entries, out_cap, the verdicts, the new index, out_bound and d_result.  The CPU and the GPU
tests share it."""
import struct

import frame_buffers_model as M
import frame_chunked_model as K
import frame_index_model as X
import frame_range_model as R
import frame_rechunk_model as RC
import oracle as O

U64 = R.U64
MAX_DEC = 65536
MAX_COUNT = 1 << 32
MAX_STAGE = 1 << 48
CHUNK_SIZES = [1, 63, 64, 65, 4096, 65536]


def seg_lists(outputs):
    """outputs: per output a list of (stream, off, len) -> dict of first, stream, off, len: the segment list as the call takes it."""
    segs = dict(first=[0], stream=[], off=[], len=[])
    for segments in outputs:
        for s, o, n in segments:
            segs["stream"].append(s)
            segs["off"].append(o)
            segs["len"].append(n)
        segs["first"].append(len(segs["stream"]))
    return segs


def concat(raws, segments) -> bytes:
    """What an output decodes to."""
    return b"".join(raws[s][o:o + n] for s, o, n in segments)


# ---- one segment -------------------------------------------------------------------------------------------------------------------------------
def _failed(status: int):
    return dict(status=status, head=False, tail=False, r0=0, r1=0, hdec=0, tdec=0, hlen=0, tlen=0, hskip=0, hp=0, tp=0, kept=0, kbytes=0, bytes=0,
                edges=[], items=[])


def segment(ix, lens, hop_at, src: int, off: int, ln: int, cb: int):
    """One segment on its own: -> dict of status and, for SNP_OK, head / tail (edges), r0, r1, what the edges decode to (hdec, tdec), their bytes
    inside the segment (hlen, tlen), hskip, the pieces (hp, tp), kept rows and their chunks' bytes, bytes (its decoded length), edges (rows as the
    chunk table takes them, head first) and items, in the order of the new stream:
      ("piece", tail, slot, edge, from, len, at)  piece `slot` of the segment: bytes [from, from + len) of what edge `edge` decodes to
      ("kept", row, pos, size, at)                old row `row`: the chunk [pos, pos + size) of the source
    at: the item's first decoded byte, relative to the segment's.  hop_at(src, pos) -> M.Hop; lens: the sources' bytes."""
    ns = len(lens)
    if src >= ns:
        return _failed(O.ERR_BAD_ARG)
    k = _failed(O.OK)
    if ln == 0:
        return k
    st = RC.begin(ix, src)
    if st != O.OK:
        return _failed(st)
    total = ix["total"][src]
    if off + ln > U64 or off + ln > total:
        return _failed(O.ERR_BAD_ARG)
    p = X.plan(ix, ns, src, off, ln, U64)
    if p["status"] != O.OK:
        return _failed(O.ERR_BAD_ARG)
    lo, hi, r0, r1, f1, n = p["lo"], p["hi"], p["r0"], p["r1"], p["f1"], lens[src]
    k.update(head=p["head"], tail=p["last"], r0=r0, r1=r1, bytes=hi - lo)
    slot = 0
    for i in range(r0, r1):
        s, e, pos = ix["start"][i], X.row_end(ix, f1, total, i), ix["pos"][i]
        if e < s or pos >= n:
            return _failed(O.ERR_BAD_ARG)
        h = hop_at(src, pos)
        if h.kind != "data" or e - s != h.dec:
            return _failed(O.ERR_BAD_ARG)
        if i + 1 < r1 and ix["pos"][i + 1] < h.next:
            return _failed(O.ERR_BAD_ARG)
        head, tail = p["head"] and i == r0, p["last"] and i == r1 - 1
        if head or tail:
            border = lo if head else hi
            if h.dec > MAX_DEC or not s < border < e:
                return _failed(O.ERR_BAD_ARG)
            a, b = max(s, lo), min(e, hi)
            k["edges"].append((h.type, pos + 8, h.body_len, h.crc, s, h.dec))
            for o in range(a, b, cb):
                k["items"].append(("piece", tail, slot, len(k["edges"]) - 1, o - s, min(cb, b - o), o - lo))
                slot += 1
            if head:
                k.update(hdec=h.dec, hlen=b - a, hskip=lo - s, hp=K.nchunks(b - a, cb))
            else:
                k.update(tdec=h.dec, tlen=b - a, tp=K.nchunks(b - a, cb))
        else:
            if s < lo or e > hi:
                return _failed(O.ERR_BAD_ARG)
            k["items"].append(("kept", i, pos, h.next - pos, s - lo))
            k["kept"] += 1
            k["kbytes"] += h.next - pos
    return k


def seg_counts(k):
    """What a segment asks: edge rows, pieces, staging bytes, rows of the new index (clamped), decoded bytes, size bound of its part."""
    pieces = k["hp"] + k["tp"]
    return (len(k["edges"]), pieces, k["hdec"] + k["tdec"], min(pieces + k["kept"], MAX_COUNT), k["bytes"],
            k["kbytes"] + 8 * pieces + k["hlen"] + k["tlen"])


def out_segs(segs, nsegs: int, j: int):
    """The segments of output j, inside nsegs whatever seg_first holds: -> (ok, s0, s1)."""
    s0, s1 = min(segs["first"][j], nsegs), min(segs["first"][j + 1], nsegs)
    return s1 >= s0, s0, s1


# ---- the whole call ----------------------------------------------------------------------------------------------------------------------------
def compose_plan(streams, ix, segs, cb: int, caps=None, max_slots: int | None = None, stage_cap: int | None = None,
                 max_entries: int | None = None, variant: int = O.HASH_CRC32C):
    """snp_frame_compose_indexed_batch.  segs: dict of first (nout + 1), stream, off, len.  None: a bound that admits all.
    -> dict of status, out_len, streams (the new stream, None unless written), alone (never: the key rechunk_plan has), index (the new one:
    first, start, pos, total, tail), out_bound, result [6]."""
    assert 1 <= cb <= MAX_DEC
    nout = len(segs["first"]) - 1
    nsegs = min(len(segs["stream"]), len(segs["off"]), len(segs["len"]))
    BIG = 1 << 62
    max_slots = BIG if max_slots is None else max_slots
    stage_cap = BIG if stage_cap is None else stage_cap
    max_entries = BIG if max_entries is None else max_entries
    caps = [BIG] * nout if caps is None else caps
    lens = [len(s) for s in streams]
    plans = {}

    def seg(g):
        if g not in plans:
            plans[g] = segment(ix, lens, lambda b, pos: M.hop(streams[b], pos), segs["stream"][g], segs["off"][g], segs["len"][g], cb)
        return plans[g]

    edges = slots = stage = nrows = copied = 0
    status, out_len, new, bound = [], [], [None] * nout, []
    index = dict(first=[0], start=[], pos=[], total=[], tail=[])
    for j in range(nout):
        ok, s0, s1 = out_segs(segs, nsegs, j)
        st = O.OK if ok else O.ERR_BAD_ARG
        mine = []
        for g in range(s0, s1) if ok else []:
            k = seg(g)
            if k["status"] != O.OK:                                     # the first failing segment in segment order
                st = k["status"]
                break
            mine.append((g, k))
        status.append(st)
        out_len.append(0)
        bound.append(0)
        if st == O.OK:
            c = [seg_counts(k) for _, k in mine]
            ce, cs, cg, cr = (min(sum(v[0] for v in c), MAX_COUNT), min(sum(v[1] for v in c), MAX_COUNT), min(sum(v[2] for v in c), MAX_STAGE),
                              min(sum(v[3] for v in c), MAX_COUNT))
            edges, slots, stage, nrows = edges + ce, slots + cs, stage + cg, nrows + cr
            bound[j] = (10 + sum(v[5] for v in c)) & U64
            status[j] = O.ERR_OUTPUT_TOO_SMALL
            if edges <= max_slots and slots <= max_slots and stage <= stage_cap and nrows <= max_entries:
                failed = O.OK
                staged = []
                for g, k in mine:                                       # the first failing edge: segment order, the head edge first
                    s = streams[segs["stream"][g]] if k["edges"] else None
                    staged.append([])
                    for r in k["edges"]:
                        failed, dec = R.chunk_result(s, r)
                        if failed != O.OK:
                            break
                        staged[-1].append(dec)
                    if failed != O.OK:
                        break
                if failed != O.OK:
                    status[j], bound[j] = failed, 0
                else:
                    out, at, base, starts, poss, kept = [M.STREAM_ID], 10, 0, [], [], 0
                    for (g, k), dec in zip(mine, staged):
                        s = streams[segs["stream"][g]] if k["items"] else None
                        for it in k["items"]:
                            if it[0] == "piece":
                                chunk = K.chunks_of(dec[it[3]][it[4]:it[4] + it[5]], cb, variant)[0]
                            else:
                                chunk = s[it[2]:it[2] + it[3]]
                                kept += 1
                            starts.append((base + it[-1]) & U64)
                            poss.append(at)
                            out.append(chunk)
                            at += len(chunk)
                        base += k["bytes"]
                    if at <= caps[j]:
                        new[j] = b"".join(out)
                        assert len(new[j]) == at <= bound[j]
                        status[j], out_len[j] = O.OK, at
                        copied += kept
                        index["start"] += starts
                        index["pos"] += poss
        written = new[j] is not None
        index["first"].append(len(index["start"]))
        index["total"].append(sum(k["bytes"] for _, k in mine) & U64 if written else 0)
        index["tail"].append(status[j])
    return dict(status=status, out_len=out_len, streams=new, alone=[False] * nout, index=index, out_bound=bound,
                result=[max(edges, slots) & U64, sum(out_len) & U64, stage & U64, sum(1 for x in new if x is not None), nrows & U64, copied])


def needs(streams, ix, segs, cb: int):
    """-> (max_slots, stage_cap, max_entries) that admit every output: the sizing call."""
    nout = len(segs["first"]) - 1
    res = compose_plan(streams, ix, segs, cb, caps=[0] * nout, max_slots=0, stage_cap=0, max_entries=0)["result"]
    return res[0], res[2], res[4]


def same_index(a, b) -> bool:
    return all(list(a[key]) == list(b[key]) for key in ("first", "start", "pos", "total", "tail"))


# ---- cases the CPU and the GPU tests share ---------------------------------------------------------------------------------------------------------
def shapes(totals, cb: int):
    """name -> (segments of one output, claim) over sources 0 and 1 of totals[0], totals[1] decoded bytes (each at least 5 cb, totals[0] a
    multiple of cb): the shapes of the issue.  claim "a": the output is the chunked encoder's for the concatenation when the sources are; "c":
    it decodes to the concatenation."""
    t0, t1 = totals[0], totals[1]
    assert t0 % cb == 0 and t0 >= 5 * cb and t1 >= 5 * cb
    half = cb // 2
    got = {
        "concatenation": ([(0, 0, t0), (1, 0, t1)], "a"),
        "split_at_a_grid_point_left": ([(1, 0, 2 * cb)], "a"),
        "split_at_a_grid_point_right": ([(1, 2 * cb, t1 - 2 * cb)], "a"),
        "aligned_extract": ([(0, cb, 3 * cb)], "a"),
        "no_segment": ([], "a"),
        "only_empty_segments": ([(0, 0, 0), (1, t1, 0), (0, 7, 0)], "a"),
        "empty_segments_everywhere": ([(1, 3, 0), (0, 0, t0), (0, t0, 0), (1, 0, 0), (1, 0, t1), (1, t1, 0)], "a"),
        "interleaved_records": ([(b, k * cb, cb) for k in range(4) for b in (0, 1)], "a"),
        "same_source_twice_overlapping": ([(0, 0, 3 * cb), (0, cb, 3 * cb)], "a"),
    }
    if cb > 1:
        got.update({
            "split_mid_chunk_left": ([(1, 0, 2 * cb + half)], "c"),
            "split_mid_chunk_right": ([(1, 2 * cb + half, t1 - 2 * cb - half)], "c"),
            "window_inside_one_chunk": ([(0, cb + cb // 4, max(half, 1))], "c"),
            "starts_mid_row_ends_at_a_row_end": ([(0, half, 3 * cb - half)], "c"),
            "starts_at_a_row_start_ends_mid_row": ([(0, cb, 2 * cb + half)], "c"),
            "both_edges": ([(1, half, 3 * cb)], "c"),
            "overlapping_off_the_grid": ([(0, 1, 2 * cb), (0, half, 2 * cb + 1), (1, cb - 1, 2)], "c"),
            "interleaved_off_the_grid": ([(b, k * cb + 1, cb) for k in range(3) for b in (0, 1)], "c"),
        })
    return got


def foreign_sources(html: bytes):
    """-> (streams, raws): sources no encoder of this project writes -- skippable, padding and repeated-identifier chunks between data chunks,
    zero-length data chunks."""
    a, b, c, d = html[:1000], html[1000:1700], html[1700:3000], html[3000:3400]
    skip, pad, zero = M.chunk(0x80, b"note"), M.chunk(0xFE, bytes(21)), M.data_chunk(b"", compressed=False)
    ch = M.data_chunk
    return ([M.STREAM_ID + skip + ch(a) + pad + ch(b) + skip + M.STREAM_ID + ch(c) + ch(d) + skip,
             M.STREAM_ID + zero + ch(a) + zero + zero + ch(b) + ch(c) + zero + ch(d) + zero], [a + b + c + d] * 2)


def foreign_outputs():
    """Outputs over foreign_sources: everything that is no data chunk is dropped; zero-length rows at a border are not taken, inside they are."""
    return [[(0, 0, 3400)], [(0, 1000, 2000)], [(0, 500, 2700), (1, 0, 3400)], [(1, 1000, 700)], [(1, 0, 1700)], [(1, 1000, 2400)], [(1, 999, 702)],
            [(1, 0, 3400), (0, 1700, 1300)]]


def mixed_batch(html: bytes, cb: int, variant: int = O.HASH_CRC32C):
    """One batch with every shape: -> (streams, raws, index, outputs, claims).  Sources 0 and 1 are the chunked encoder's at cb, source 2 is
    source 0 after a splice in the middle of a chunk (fragmented), sources 3 and 4 are foreign_sources.  claims[j]: "a" or "c" (shapes)."""
    import frame_splice_model as S
    raws = [html[:6 * cb], html[100:100 + 5 * cb + cb // 3 + 1]]
    streams = [K.stream_of(r, cb, variant) for r in raws]
    ins = html[7:7 + cb // 3 + 5]
    cut = S.splice_plan(streams[:1], X.build_index(streams[:1]), [(cb + cb // 2, 0)], [ins], cb, variant=variant)
    assert cut["status"] == [O.OK]
    streams.append(cut["streams"][0])
    raws.append(S.edited(raws[0], cb + cb // 2, 0, ins))
    fs, fr = foreign_sources(html)
    streams, raws = streams + fs, raws + fr
    outputs, claims = [], []
    for segments, claim in shapes([len(raws[0]), len(raws[1])], cb).values():
        outputs.append(segments)
        claims.append(claim)
    n2 = len(raws[2])
    outputs += [[(2, 0, n2)], [(2, cb, 2 * cb + 1)], [(2, 1, n2 - 2), (0, 0, cb)]]
    outputs += [[(s + 3, o, n) for s, o, n in segments] for segments in foreign_outputs()]
    claims += ["c"] * (len(outputs) - len(claims))
    return streams, raws, X.build_index(streams), outputs, claims


# ---- the cases of the planning check (tests/abi/frame_compose_plan_check.hip) --------------------------------------------------------------------
def item_words(it):
    """An item as cc_row gives it: kept tail row slot from len at."""
    if it[0] == "kept":
        return (1, 0, it[1], 0, 0, 0, it[4])
    return (0, int(it[1]), 0, it[2], it[4], it[5], it[6])


def seg_line(k) -> str:
    """What the planning header must give for one segment, as the check program prints it: the plan, what it counts, its first and last row."""
    first = item_words(k["items"][0]) if k["items"] else (0,) * 7
    last = item_words(k["items"][-1]) if k["items"] else (0,) * 7
    return "%d %d %d %d %d %d %d %d %d %d %d %d %d %d | %d %d %d %d %d %d | %d %d %d %d %d %d %d | %d %d %d %d %d %d %d" % (
        k["status"], k["head"], k["tail"], k["r0"], k["r1"], k["hdec"], k["tdec"], k["hlen"], k["tlen"], k["hskip"], k["hp"], k["tp"], k["kept"],
        k["kbytes"], *[v & U64 for v in seg_counts(k)], *first, *last)


def plan_lines(ix, streams, segs, cb: int):
    """Per segment its line, then per output: ok s0 s1."""
    nsegs = min(len(segs["stream"]), len(segs["off"]), len(segs["len"]))
    lens = [len(s) for s in streams]
    out = [seg_line(segment(ix, lens, lambda b, pos: M.hop(streams[b], pos), segs["stream"][g], segs["off"][g], segs["len"][g], cb))
           for g in range(nsegs)]
    return out + ["%d %d %d" % out_segs(segs, nsegs, j) for j in range(len(segs["first"]) - 1)]


NUMERIC_KEYS = ("n", "cb", "off", "len", "total", "tail", "rows", "start0", "pos0", "kind0", "size0", "dec0", "start1", "pos1", "kind1", "size1", "dec1")


def numeric_line(case) -> str:
    """case: dict of NUMERIC_KEYS -- a source of n bytes that is too long to hold, given as up to two index rows and the headers they point at
    (kind: 0 data, 1 skippable), and one segment of it."""
    c = case
    rows = c["rows"]
    ix = dict(first=[0, rows], start=[c["start0"], c["start1"]][:rows], pos=[c["pos0"], c["pos1"]][:rows], total=[c["total"]], tail=[c["tail"]])

    def hop_at(_, pos):
        j = 0 if pos == c["pos0"] else 1
        size = c["size%d" % j]
        return M.Hop("data" if c["kind%d" % j] == 0 else "skip", pos + 4 + size, type=1, body_len=size - 4, dec=c["dec%d" % j])

    return seg_line(segment(ix, [c["n"]], hop_at, 0, c["off"], c["len"], c["cb"]))


def write_cases(path: str, streams, cases, numeric):
    """The input of the check program: the streams; every case -- an index and a segment list (any lists at all) and chunk_bytes; then the
    numeric cases, seventeen words each."""
    ns = len(streams)
    with open(path, "wb") as f:
        f.write(struct.pack("<Q", ns))
        for s in streams:
            f.write(struct.pack("<Q", len(s)))
            f.write(s)
        f.write(struct.pack("<Q", len(cases)))
        for ix, segs, cb in cases:
            ne = min(len(ix["start"]), len(ix["pos"]))
            nsegs = min(len(segs["stream"]), len(segs["off"]), len(segs["len"]))
            nout = len(segs["first"]) - 1
            f.write(struct.pack("<4Q", ne, cb, nout, nsegs))
            for src, key, n in ((ix, "first", ns + 1), (ix, "total", ns), (ix, "tail", ns), (ix, "start", ne), (ix, "pos", ne),
                                (segs, "first", nout + 1), (segs, "stream", nsegs), (segs, "off", nsegs), (segs, "len", nsegs)):
                assert len(src[key]) >= n
                f.write(struct.pack("<%dQ" % n, *[int(v) & U64 for v in src[key][:n]]))
        f.write(struct.pack("<Q", len(numeric)))
        for c in numeric:
            f.write(struct.pack("<%dQ" % len(NUMERIC_KEYS), *[int(c[key]) & U64 for key in NUMERIC_KEYS]))

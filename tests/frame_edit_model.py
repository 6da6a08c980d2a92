"""Pure-Python statement of include/snappier_hip_frame_edit.h (snp_frame_edit_indexed_batch): a sorted EDIT SCRIPT per framed stream kept with its
chunk index -- edit e replaces decoded bytes [off, off + del) of the OLD stream by ins source bytes.  Built on frame_splice_model.plan (fs_plan:
the rows an edit owns, its edges, its hole and the probes of the untrusted index are the splice's, edit by edit), the way the splice model sits
on the index model.  What is added here is what csrc/frame_edit_device.h adds: the CSR edit list, the order of the edits, the links between
edits that own the same row, the groups with ONE region and ONE hole each, the running length, the admission over groups, and the new index.
The CPU and the GPU tests share it."""
import struct

import frame_buffers_model as M
import frame_chunked_model as K
import frame_range_model as R
import frame_splice_model as S
import oracle as O

U64 = R.U64
MAX_PIECES = S.MAX_PIECES
MAX_STAGE = S.MAX_STAGE


# ---- the planning (csrc/frame_edit_device.h) -------------------------------------------------------------------------------------------------------
def csr(ed_first, nedits: int, ns: int):
    """fe_csr: -> per stream (e0, e1, ok).  The values are clamped to nedits; from the first stream whose list runs backwards on, every stream is
    refused (its neighbours' lists could share edits with it)."""
    out, bad = [], False
    for b in range(ns):
        a, e = min(ed_first[b], nedits), min(ed_first[b + 1], nedits)
        bad = bad or e < a
        out.append((a, e, not bad))
    return out


def linked(p, hi_p: int, k, lo_k: int) -> bool:
    """fe_linked: both passed, in order, both own rows, and the last owned row of p is the first owned row of k."""
    return (p["splice"] and k["splice"] and hi_p <= U64 and lo_k >= hi_p and p["r1"] > p["r0"] and k["r1"] > k["r0"] and p["r1"] - 1 == k["r0"])


def verdict(k, lo_k: int, p, lo_p: int, del_p: int, total: int, ins_sum: int, del_mod: int) -> int:
    """fe_verdict: the edit's own verdict.  p: the plan of the named edit before it in its stream (None: there is none).  ins_sum: the inserted
    bytes of the stream's edits up to and with this one, exactly; del_mod: their deleted bytes modulo 2^64."""
    if k["status"] != O.OK:
        return k["status"]
    if p is not None:
        hi_p = lo_p + del_p
        if hi_p <= U64 and lo_k < hi_p:
            return O.ERR_BAD_ARG                                        # out of order with, or overlapping, its predecessor
        if p["splice"] and not linked(p, hi_p, k, lo_k) and (p["p1"] > k["p0"] or p["r1"] > k["r0"]):
            return O.ERR_BAD_ARG                                        # the holes, and the owned rows, in order
    if del_mod <= total and total - del_mod + ins_sum > U64:
        return O.ERR_BAD_ARG                                            # the running length wraps
    return O.OK


def region_len(ins_sum: int, extra: int):
    """fe_region: -> (|R| modulo 2^64, it fits 64 bits)."""
    r = ins_sum + extra
    return r & U64, r <= U64


# ---- the whole call -------------------------------------------------------------------------------------------------------------------------------
def edit_plan(streams, ix, ed_first, edits, srcs, cb: int, caps=None, max_slots: int | None = None, stage_cap: int | None = None,
              variant: int = O.HASH_CRC32C):
    """snp_frame_edit_indexed_batch.  ed_first: CSR, nstreams + 1; edits: (off, del) per edit, srcs: the bytes each puts in their place.  None: a
    bound that admits all.  -> dict of status, ed_status, out_len, streams (the new stream, None unless written), hole ((P0 of the first group,
    P1 of the last) per stream), holes (every group's), index (the new one), out_bound, result [4]."""
    assert 1 <= cb <= S.MAX_DEC
    ns, nedits = len(streams), len(edits)
    BIG = 1 << 62
    max_slots = BIG if max_slots is None else max_slots
    stage_cap = BIG if stage_cap is None else stage_cap
    caps = [BIG] * ns if caps is None else caps
    ne = min(len(ix["start"]), len(ix["pos"]))
    cap_rows = ne + max_slots
    ed_status = [O.OK] * nedits
    status, out_len, new, bound, holes, plans = [], [], [None] * ns, [], [[] for _ in range(ns)], []
    slots = stage = 0
    written = []                                                        # per written stream: what the new index needs
    for b, (e0, e1, ok) in enumerate(csr(ed_first, nedits, ns)):
        s, n = streams[b], len(streams[b])
        status.append(O.OK)
        out_len.append(0)
        bound.append(0)
        written.append(None)
        f0, rows = S.rows_of(ix, b)
        plans.append((f0, rows))
        if not ok:
            status[b] = O.ERR_BAD_ARG
            continue
        named = [e for e in range(e0, e1) if edits[e][1] or len(srcs[e])]
        if not named:
            continue
        total = ix["total"][b]
        pl, prev, ins_sum, del_sum, link = {}, None, 0, 0, {}
        for e in named:
            off, dele = edits[e]
            k = S.plan(ix, b, n, off, dele, len(srcs[e]), cb, lambda pos, s=s: M.hop(s, pos))
            ins_sum += len(srcs[e])
            del_sum += dele
            p = pl[prev] if prev is not None else None
            ed_status[e] = verdict(k, off, p, edits[prev][0] if p else 0, edits[prev][1] if p else 0, total, ins_sum, del_sum & U64)
            link[e] = p is not None and linked(p, edits[prev][0] + edits[prev][1], k, off)
            pl[e], prev = k, e
        failed = [ed_status[e] for e in named if ed_status[e] != O.OK]
        if failed:
            status[b] = failed[0]
            continue
        # groups: maximal runs of linked edits
        groups = []
        for e in named:
            if link[e]:
                groups[-1].append(e)
            else:
                groups.append([e])
        # what each group asks: its edge rows (a shared row entered once, by the first edit that touches it), its region, its pieces
        gi, spieces, sstage, sbound = [], 0, 0, n + (10 if n == 0 else 0)
        for g in groups:
            edges, extra, ins = [], 0, 0
            for j, e in enumerate(g):
                k = pl[e]
                if k["hrow"] is not None and not link[e]:
                    edges.append((k["r0"], k["hrow"]))
                if k["trow"] is not None:
                    edges.append((k["r1"] - 1, k["trow"]))
                ins += len(srcs[e])
                extra += (0 if link[e] else k["hl"]) + (edits[g[j + 1]][0] - (edits[e][0] + edits[e][1]) if j + 1 < len(g) else k["tl"])
            rlen, fits = region_len(ins, extra)
            pieces = min(K.nchunks(rlen, cb), MAX_PIECES) if fits else MAX_PIECES
            st = min(sum(r[5] for _, r in edges) + rlen, MAX_STAGE) if fits else MAX_STAGE
            p0, p1 = pl[g[0]]["p0"], pl[g[-1]]["p1"]
            gi.append(dict(edits=g, edges=edges, region=rlen, pieces=pieces, p0=p0, p1=p1, r0=pl[g[0]]["r0"], r1=pl[g[-1]]["r1"]))
            spieces += pieces
            sstage += st
            sbound += 8 * pieces + rlen - (p1 - p0)
            holes[b].append((p0, p1))
        spieces, sstage = min(spieces, MAX_PIECES), min(sstage, MAX_STAGE)
        bound[b] = sbound & U64
        slots += spieces
        stage += sstage
        status[b] = O.ERR_OUTPUT_TOO_SMALL
        if slots > max_slots or stage > stage_cap:
            continue
        # the edges, each decoded once: the first failing one in table order
        failed, rows_dec = O.OK, {}
        for g in gi:
            for r, row in g["edges"]:
                if failed == O.OK:
                    failed, dec = R.chunk_result(s, row)
                    rows_dec[r] = dec
        if failed != O.OK:
            status[b], bound[b] = failed, 0
            continue
        out, at, old_at = [], 0, 0
        if n == 0:
            out.append(M.STREAM_ID)
            at = 10
        for g in gi:
            first, last = pl[g["edits"][0]], pl[g["edits"][-1]]
            parts = [rows_dec[first["r0"]][:first["hl"]] if first["hl"] else b""]
            for j, e in enumerate(g["edits"]):
                parts.append(srcs[e])
                if j + 1 < len(g["edits"]):
                    nxt = g["edits"][j + 1]
                    row, k = rows_dec[pl[e]["r1"] - 1], pl[e]
                    a = len(row) - k["tl"]
                    parts.append(row[a:a + edits[nxt][0] - (edits[e][0] + edits[e][1])])
            if last["tl"]:
                row = rows_dec[last["r1"] - 1]
                parts.append(row[len(row) - last["tl"]:])
            region = b"".join(parts)
            assert len(region) == g["region"]
            out.append(s[old_at:g["p0"]])
            at += g["p0"] - old_at
            g["new_pos"] = []
            for c in K.chunks_of(region, cb, variant):
                g["new_pos"].append(at)
                out.append(c)
                at += len(c)
            assert len(g["new_pos"]) == g["pieces"]
            old_at = g["p1"]
            g["moved"] = at - old_at                                    # what a position behind this hole moves by
        out.append(s[old_at:])
        at += n - old_at
        if at > caps[b]:
            continue
        new[b] = b"".join(out)
        assert len(new[b]) == at <= bound[b]
        status[b], out_len[b] = O.OK, at
        written[b] = (gi, pl, named)
    # the new index
    first, start, pos, total, tail = [0], [], [], [], []
    for b in range(ns):
        f0, rows = plans[b]
        f1 = f0 + rows
        if written[b] is None:
            start += ix["start"][f0:f1]
            pos += ix["pos"][f0:f1]
            total.append(ix["total"][b])
            tail.append(ix["tail"][b])
        else:
            gi, pl, named = written[b]
            at, delta, moved = f0, 0, 0
            for g in gi:
                start += [(v + delta) & U64 for v in ix["start"][at:g["r0"]]]
                pos += [(v + moved) & U64 for v in ix["pos"][at:g["r0"]]]
                e = g["edits"][0]
                start += [(edits[e][0] - pl[e]["hl"] + delta + j * cb) & U64 for j in range(g["pieces"])]
                pos += g["new_pos"]
                delta += sum(len(srcs[e]) - edits[e][1] for e in g["edits"])
                moved, at = g["moved"], g["r1"]
            start += [(v + delta) & U64 for v in ix["start"][at:f1]]
            pos += [(v + moved) & U64 for v in ix["pos"][at:f1]]
            total.append((ix["total"][b] + delta) & U64)
            tail.append(O.OK)
        first.append(len(start))
    index = dict(first=[min(f, cap_rows) for f in first], start=start[:cap_rows], pos=pos[:cap_rows], total=total, tail=tail)
    return dict(status=status, ed_status=ed_status, out_len=out_len, streams=new, hole=[(h[0][0], h[-1][1]) if h else (0, 0) for h in holes],
                holes=holes, index=index, out_bound=bound,
                result=[slots & U64, sum(out_len) & U64, stage & U64, sum(1 for x in new if x is not None)])


def needs(streams, ix, ed_first, edits, srcs, cb: int):
    """-> (max_slots, stage_cap) that admit every stream: the sizing call."""
    res = edit_plan(streams, ix, ed_first, edits, srcs, cb, caps=[0] * len(streams), max_slots=0, stage_cap=0)["result"]
    return res[0], res[2]


def applied(raw: bytes, script) -> bytes:
    """script: (off, del, src) ascending and disjoint, in the OLD buffer's coordinates: applied from the last to the first."""
    for off, dele, src in reversed(script):
        raw = raw[:off] + src + raw[off + dele:]
    return raw


def flat(scripts):
    """scripts: per stream a list of (off, del, src) -> (ed_first, edits, srcs)."""
    first, edits, srcs = [0], [], []
    for sc in scripts:
        edits += [(o, d) for o, d, _ in sc]
        srcs += [x for _, _, x in sc]
        first.append(len(edits))
    return first, edits, srcs


# ---- cases the CPU and the GPU tests share --------------------------------------------------------------------------------------------------------
def directed_scripts(cb: int, src: bytes):
    """name -> (decoded length of the stream, [(off, del, ins bytes)]) for streams of a few chunks of cb bytes (the last one short): the edit
    scripts the contract tells apart.  (cb = 1 has no mid-chunk offset: those scripts fall on boundaries there.)"""
    n = 4 * cb + (cb + 1) // 2
    q = cb // 4

    def s(k, at=0):
        return src[at:at + k]

    return {
        "two_edits_inside_one_chunk": (n, [(cb + q, q // 2 + 1, s(5)), (cb + 3 * q + 1, 0, s(cb + 2, 9))]),
        "chain_each_tail_row_is_the_next_head_row": (n, [(q, cb, s(3)), (cb + 2 * q, cb, s(0)), (2 * cb + 3 * q, cb, s(2 * cb + 1, 5))]),
        "separate_chunks_untouched_between": (n, [(q, 1, s(2)), (2 * cb + q, q, s(0)), (4 * cb, 1, s(7, 3))]),
        "hi_equals_next_lo_on_a_boundary": (n, [(q, cb - q, s(4)), (cb, q, s(1, 50))]),
        "hi_equals_next_lo_off_a_boundary": (n, [(cb + 1, q, s(4)), (cb + 1 + q, q, s(6, 20))]),
        "two_inserts_at_one_offset_mid_chunk": (n, [(cb + q, 0, s(3)), (cb + q, 0, s(5, 100))]),
        "two_inserts_at_one_boundary": (n, [(2 * cb, 0, s(3)), (2 * cb, 0, s(cb + 1, 100))]),
        "insert_on_a_boundary_then_delete_from_it": (n, [(2 * cb, 0, s(9)), (2 * cb, q, s(0))]),
        "edit_ending_at_total_and_insert_at_total": (n, [(n - 1, 1, s(2)), (n, 0, s(cb + 3, 11))]),
        "everything_deleted_by_two_edits": (n, [(0, 2 * cb + q, s(0)), (2 * cb + q, n - 2 * cb - q, s(0))]),
        "empty_stream": (0, [(0, 0, s(cb + 2)), (0, 0, s(1, 77))]),
        "skipped_edits_only": (n, [(3, 0, s(0)), (cb, 0, s(0))]),
        "skipped_edits_between_linked_ones": (n, [(cb + 1, 1, s(1)), (cb + 2, 0, s(0)), (cb + 2, 1, s(2, 8)), (1, 0, s(0))]),
        "no_edit": (n, []),
    }


def scripts_batch(html: bytes, cb: int, variant: int = O.HASH_CRC32C):
    """One stream per directed script: -> (names, raws, streams, scripts)."""
    cases = directed_scripts(cb, html[3001:])
    raws = [html[7 + i:7 + i + n] for i, (n, _) in enumerate(cases.values())]
    streams = [K.stream_of(a, cb, variant) if a else b"" for a in raws]
    return list(cases), raws, streams, [sc for _, sc in cases.values()]


# ---- the cases of the planning check (tests/abi/frame_edit_plan_check.hip) -----------------------------------------------------------------------
def check_lines(ix, streams, ed_first, edits3, cb: int, lens=None, hops=None):
    """What the planning header must give, as the check program prints it: per stream `S b e0 e1 ok`, then per named edit of a stream whose list
    is sound `E e verdict linked |H| |T|` (|H| 0 when linked: the edit before it holds those bytes).  edits3: (off, del, ins) per edit.  lens
    and hops: streams too long to hold, as their lengths and as functions pos -> M.Hop."""
    out = []
    ne = len(edits3)
    ns = len(streams) if lens is None else len(lens)
    for b, (e0, e1, ok) in enumerate(csr(ed_first, ne, ns)):
        out.append("S %d %d %d %d" % (b, e0, e1, ok))
        if not ok:
            continue
        n = len(streams[b]) if lens is None else lens[b]
        hop_at = (lambda pos, s=streams[b]: M.hop(s, pos)) if hops is None else hops[b]
        total = ix["total"][b]
        prev, p, ins_sum, del_sum = None, None, 0, 0
        for e in range(e0, e1):
            off, dele, ins = edits3[e]
            if dele == 0 and ins == 0:
                continue
            k = S.plan(ix, b, n, off, dele, ins, cb, hop_at)
            ins_sum += ins
            del_sum += dele
            v = verdict(k, off, p, edits3[prev][0] if p else 0, edits3[prev][1] if p else 0, total, ins_sum, del_sum & U64)
            ln = p is not None and linked(p, edits3[prev][0] + edits3[prev][1], k, off)
            out.append("E %d %d %d %d %d" % (e, v, ln, 0 if ln else k["hl"], k["tl"]))
            prev, p = e, k
    return out


NUMERIC_KEYS = ("n", "cb", "total", "tail", "rows", "start0", "pos0", "kind0", "size0", "dec0", "start1", "pos1", "kind1", "size1", "dec1", "nedits",
                "off0", "del0", "ins0", "off1", "del1", "ins1", "off2", "del2", "ins2")


def numeric_lines(c):
    """c: dict of NUMERIC_KEYS -- a stream of n bytes that is too long to hold, given as up to two index rows and the headers they point at (kind:
    0 data, 1 skippable), and up to three edits of it."""
    rows = c["rows"]
    ix = dict(first=[0, rows], start=[c["start0"], c["start1"]][:rows], pos=[c["pos0"], c["pos1"]][:rows], total=[c["total"]], tail=[c["tail"]])

    def hop_at(pos):
        j = 0 if pos == c["pos0"] else 1
        size = c["size%d" % j]
        return M.Hop("data" if c["kind%d" % j] == 0 else "skip", pos + 4 + size, type=1, body_len=size - 4, dec=c["dec%d" % j])

    edits3 = [(c["off%d" % j], c["del%d" % j], c["ins%d" % j]) for j in range(c["nedits"])]
    return check_lines(ix, None, [0, len(edits3)], edits3, c["cb"], lens=[c["n"]], hops=[hop_at])


def write_cases(path: str, streams, cases, numeric=()):
    """The input of the check program: the streams; every case -- an index (any lists at all), chunk_bytes, ed_first and (off, del, ins) per edit;
    then the numeric cases, twenty-five words each."""
    with open(path, "wb") as f:
        f.write(struct.pack("<Q", len(streams)))
        for s in streams:
            f.write(struct.pack("<Q", len(s)))
            f.write(s)
        f.write(struct.pack("<Q", len(cases)))
        for ix, cb, ed_first, edits3 in cases:
            ne = min(len(ix["start"]), len(ix["pos"]))
            f.write(struct.pack("<3Q", ne, cb, len(edits3)))
            for key, n in (("first", len(streams) + 1), ("total", len(streams)), ("tail", len(streams)), ("start", ne), ("pos", ne)):
                assert len(ix[key]) >= n
                f.write(struct.pack("<%dQ" % n, *[int(v) & U64 for v in ix[key][:n]]))
            f.write(struct.pack("<%dQ" % (len(streams) + 1), *[int(v) & U64 for v in ed_first]))
            for j in range(3):
                f.write(struct.pack("<%dQ" % len(edits3), *[int(r[j]) & U64 for r in edits3]))
        f.write(struct.pack("<Q", len(numeric)))
        for c in numeric:
            f.write(struct.pack("<%dQ" % len(NUMERIC_KEYS), *[int(c[key]) & U64 for key in NUMERIC_KEYS]))

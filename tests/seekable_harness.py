"""Shared by the GPU tests of the seekable-stream calls (test_gpu_frame_range.py, test_gpu_frame_index.py, test_gpu_frame_chunked.py,
test_gpu_frame_update.py, test_gpu_seekable_tiers.py): each of the five calls made directly through its library, with every output array
between guard elements, the workspace guarded and the arena canary-filled.  Every harness takes the context (a BlockCodec) from its caller, so
the same call can be made under any option set, and every bound (max_chunks, max_slots, stage_cap, max_spans, edge_cap) explicitly.
One canary byte (frame_buffers_helpers.CANARY) and one Guarded serve all five: the range and index files, which had 0x5A and a Guarded
whose ptr() was the view's address, take these too."""
import ctypes as C

import numpy as np
import torch

import frame_buffers_helpers as H
import frame_chunked_model as K
import frame_index_model as X
import frame_update_model as U
import oracle as O

if torch.cuda.is_available():
    from snappier_amd import batch as SB, _native as N

GUARD = 16                 # guard elements on each side of every guarded array
CANARY = H.CANARY
KEYS = ("first", "start", "pos", "total", "tail")
UNTOUCHED = int.from_bytes(bytes([CANARY]) * 8, "little", signed=True)


def s64(v: int) -> int:
    v &= U.U64
    return v - (1 << 64) if v >> 63 else v


def s32(v: int) -> int:
    v &= 0xFFFFFFFF
    return v - (1 << 32) if v >> 31 else v


def words(vals):
    return H.dev([s64(int(v)) for v in vals])


def dev_u64(a):
    """u64 values as the bits of an int64 tensor."""
    return torch.from_numpy(np.array([s64(int(x)) for x in a], dtype=np.int64)).cuda()


def dev_i32(a):
    return torch.from_numpy(np.array([int(x) for x in a], dtype=np.int32)).cuda()


class Guarded:
    """An array between guard elements: the call gets the middle, the test checks the rims."""

    def __init__(self, n: int, dtype):
        self.n = n
        self.t = torch.empty(n + 2 * GUARD, dtype=dtype, device="cuda")
        self.t.view(torch.uint8).fill_(CANARY)
        self.mid = self.t[GUARD:GUARD + n]

    def ptr(self):
        return C.c_void_p(self.t.data_ptr() + GUARD * self.t.element_size())   # (valid for n == 0 too, where an empty view has no address)

    def read(self):
        h = self.t.cpu().numpy()
        rim = np.concatenate([h[:GUARD], h[GUARD + self.n:]])
        assert (rim.view(np.uint8) == CANARY).all(), "a write outside an array"
        return h[GUARD:GUARD + self.n].astype(np.int64).tolist()


def _p(t):
    return C.c_void_p(t.data_ptr()) if t.numel() else C.c_void_p(None)


def index_tensors(ix, ns):
    """The five arrays of a model index (any lists at all) on the device, and nentries."""
    ne = min(len(ix["start"]), len(ix["pos"]))
    tail = torch.tensor([s32(v) for v in ix["tail"][:ns]], dtype=torch.int32, device="cuda")
    return [words(ix["first"][:ns + 1]), words(ix["start"][:ne] or [0]), words(ix["pos"][:ne] or [0]), words(ix["total"][:ns]), tail], ne


# ---- snp_frame_encode_chunked_batch --------------------------------------------------------------------------------------------------------------
class Encoded:
    """One call of snp_frame_encode_chunked_batch, made directly with every array guarded and the output arena canary-filled: .got is what the
    model's encode() returns; the device tensors stay for the calls that read the streams back."""

    def __init__(self, cd, blobs, cb, max_chunks=None, caps=None, with_index=True):
        nb = len(blobs)
        CL = N.frame_chunked_lib()
        cd._bind()
        self.data, in_off, lens = H.pack(blobs)
        caps = np.array([K.frame_cap(len(x), cb) for x in blobs] if caps is None else caps, dtype=np.int64)
        self.out_off, total = H.out_layout(caps)
        self.out = torch.full((total,), CANARY, dtype=torch.uint8, device="cuda")
        mc = sum(K.nchunks(len(x), cb) for x in blobs) if max_chunks is None else max_chunks
        self.mc = mc
        self.out_len, self.status, self.result = Guarded(nb, torch.int64), Guarded(nb, torch.int32), Guarded(4, torch.int64)
        self.ix = [Guarded(nb + 1, torch.int64), Guarded(mc, torch.int64), Guarded(mc, torch.int64), Guarded(nb, torch.int64), Guarded(nb, torch.int32)]
        work = Guarded(CL.snp_frame_encode_chunked_workspace(nb, mc, cb), torch.uint8)
        self.tabs = [H.dev(in_off), H.dev(lens), H.dev(self.out_off), H.dev(caps)]
        ixp = [g.ptr() for g in self.ix] if with_index else [None] * 5
        st = CL.snp_frame_encode_chunked_batch(cd.ctx.handle, _p(self.data), _p(self.tabs[0]), _p(self.tabs[1]), nb, cb, mc, _p(self.out),
                                               _p(self.tabs[2]), _p(self.tabs[3]), self.out_len.ptr(), self.status.ptr(), *ixp, work.ptr(),
                                               self.result.ptr())
        assert st == O.OK
        torch.cuda.synchronize()
        work.read()
        status, out_len = self.status.read(), self.out_len.read()
        self.h = self.out.cpu().numpy()
        # nothing outside [out_off, out_off + out_len) of an OK buffer; a buffer that is not OK (out_len 0) has its whole range left untouched
        assert (H.outside_ranges(self.h, self.out_off, out_len) == CANARY).all(), "a write outside the output ranges"
        streams = [self.h[o:o + n].tobytes() if s == O.OK else None for s, n, o in zip(status, out_len, self.out_off.tolist())]
        self.got = {"status": status, "out_len": out_len, "streams": streams, "result": self.result.read(), **{k: [] for k in KEYS}}
        index = [g.read() for g in self.ix]
        untouched = int.from_bytes(bytes([CANARY]) * 8, "little", signed=True)
        if with_index:
            used = index[0][nb]
            assert 0 <= used <= mc and all(v == untouched for v in index[1][used:] + index[2][used:]), "a row beyond the index"
            index[1], index[2] = index[1][:used], index[2][:used]
            self.got.update(zip(KEYS, index))
        else:
            assert all((g.t.view(torch.uint8) == CANARY).all() for g in self.ix), "an index array written without an index"

    def frame_index(self):
        """The encoder's index as the wrapper's calls take it (the arrays the call wrote, on the device)."""
        return SB.FrameIndex(*[g.mid for g in self.ix], None)


# ---- snp_frame_write_indexed_batch ---------------------------------------------------------------------------------------------------------------
class Updated:
    """One call of snp_frame_write_indexed_batch, made directly with every output array guarded and the arena canary-filled; .got has the keys of
    the model's write_plan.  caps None: the model's size bound (the stream's own length where that is 0).  Bounds None: what the model needs.
    model False (batches too large for write_plan: caps, max_slots and stage_cap are then the caller's): .want is None, and the caller checks
    .got by its consequences."""

    def __init__(self, cd, streams, ix, reqs, srcs, caps=None, max_slots=None, stage_cap=None, variant=O.HASH_CRC32C, model=True):
        ns, nreq = len(streams), len(reqs)
        UL = N.frame_update_lib()
        cd._bind()
        if model:
            free = U.write_plan(streams, ix, reqs, srcs, variant=variant)
            caps = [bd or len(s) for bd, s in zip(free["out_bound"], streams)] if caps is None else caps
            max_slots = free["result"][0] if max_slots is None else max_slots
            stage_cap = free["result"][2] if stage_cap is None else stage_cap
        self.caps, self.ms, self.sc = caps, max_slots, stage_cap
        ms, sc = max_slots, stage_cap
        self.want = U.write_plan(streams, ix, reqs, srcs, caps, ms, sc, variant) if model else None
        self.data, in_off, lens = H.pack(streams)
        self.src, src_off, _ = H.pack(srcs, lead=5, gap=2)
        self.out_off, total = H.out_layout(np.array(caps, dtype=np.int64))
        self.out = torch.full((total,), CANARY, dtype=torch.uint8, device="cuda")
        self.ix, ne = index_tensors(ix, ns)
        self.out_len, self.status, self.req_status = Guarded(ns, torch.int64), Guarded(ns, torch.int32), Guarded(nreq, torch.int32)
        self.new_pos, self.bound, self.result = Guarded(ne, torch.int64), Guarded(ns, torch.int64), Guarded(4, torch.int64)
        work = Guarded(UL.snp_frame_write_indexed_workspace(ns, nreq, ms, sc), torch.uint8)
        self.tabs = [H.dev(in_off), H.dev(lens), H.dev(self.out_off), H.dev(caps), H.dev(src_off),
                     torch.tensor([s32(q[0]) for q in reqs] or [0], dtype=torch.int32, device="cuda"), words([q[1] for q in reqs] or [0]),
                     words([q[2] for q in reqs] or [0])]
        st = UL.snp_frame_write_indexed_batch(cd.ctx.handle, _p(self.data), _p(self.tabs[0]), _p(self.tabs[1]), ns, *[_p(t) for t in self.ix], ne,
                                              _p(self.src), _p(self.tabs[5]), _p(self.tabs[6]), _p(self.tabs[7]), _p(self.tabs[4]), nreq, ms, sc,
                                              _p(self.out), _p(self.tabs[2]), _p(self.tabs[3]), self.out_len.ptr(), self.status.ptr(),
                                              self.req_status.ptr(), self.new_pos.ptr(), self.bound.ptr(), work.ptr(), self.result.ptr())
        assert st == O.OK
        torch.cuda.synchronize()
        work.read()
        status, out_len = self.status.read(), self.out_len.read()
        self.h = self.out.cpu().numpy()
        # nothing outside [out_off, out_off + out_len) of a written stream; any other stream (out_len 0) has its whole range left untouched
        assert (H.outside_ranges(self.h, self.out_off, out_len) == CANARY).all(), "a write outside the output ranges"
        new = [self.h[o:o + n].tobytes() if s == O.OK and n else None for s, n, o in zip(status, out_len, self.out_off.tolist())]
        self.got = dict(status=status, out_len=out_len, streams=new, req_status=self.req_status.read(), new_pos=self.new_pos.read(),
                        out_bound=self.bound.read(), result=self.result.read())

    def check(self):
        w = self.want
        for key in ("status", "out_len", "req_status", "result", "out_bound"):
            assert self.got[key] == w[key], key
        assert self.got["new_pos"] == [s64(v) for v in w["new_pos"]]
        for b, (g, x) in enumerate(zip(self.got["streams"], w["streams"])):
            assert g == (x or None), b                                  # (a written stream of no bytes reads as None here)
        return self

    def frame_index(self):
        """The index of the new streams as the wrapper's calls take it: the old arrays with the positions the call wrote."""
        return SB.FrameIndex(self.ix[0], self.ix[1][:self.new_pos.n], self.new_pos.mid, self.ix[3], self.ix[4])


# ---- snp_frame_decode_range_batch ----------------------------------------------------------------------------------------------------------------
def pack_table(streams):
    """Every distinct stream once (the call only reads `in`: input ranges may overlap): -> (device tensor, in_off, in_len) per entry."""
    uniq = list(dict.fromkeys(streams))
    framed, off, _ = H.pack(uniq)
    where = {s: int(o) for s, o in zip(uniq, off)}
    return framed, [where[s] for s in streams], [len(s) for s in streams]


def range_call(cd, streams, ranges, caps, mc, sp, ec):
    """snp_frame_decode_range_batch called directly, every output guarded, the arena canary-filled:
    -> (status, out_len, bytes per stream (None unless OK), d_result)."""
    ns = len(streams)
    RL = N.frame_range_lib()
    cd._bind()
    framed, in_off, in_len = pack_table(streams) if ns else (torch.zeros(16, dtype=torch.uint8, device="cuda"), [], [])
    out_off, total = H.out_layout(caps)
    out = torch.full((max(total, 1),), CANARY, dtype=torch.uint8, device="cuda")
    out_len, status, result = Guarded(ns, torch.int64), Guarded(ns, torch.int32), Guarded(6, torch.int64)
    work = Guarded(RL.snp_frame_decode_range_workspace(ns, mc, sp, ec), torch.uint8)
    tables = [dev_u64(x) for x in (in_off, in_len, [r[0] for r in ranges], [r[1] for r in ranges], out_off, caps)]   # (named: they outlive the call)
    st = RL.snp_frame_decode_range_batch(cd.ctx.handle, _p(framed), _p(tables[0]), _p(tables[1]), ns, _p(tables[2]), _p(tables[3]), mc, sp, ec,
                                         _p(out), _p(tables[4]), _p(tables[5]), out_len.ptr(), status.ptr(), work.ptr(), result.ptr())
    assert st == O.OK
    torch.cuda.synchronize()
    work.read()
    st, ol, res, h = status.read(), out_len.read(), result.read(), out.cpu().numpy()
    # nothing outside [out_off, out_off + out_len) of an OK stream, nor outside [out_off, out_off + out_cap) of any other
    assert (H.outside_ranges(h, out_off, [n if s == O.OK else c for s, n, c in zip(st, ol, caps)]) == CANARY).all(), "a write outside the output ranges"
    data = [h[o:o + n].tobytes() if s == O.OK else None for s, n, o in zip(st, ol, out_off.tolist())]
    return st, ol, data, res


# ---- snp_frame_index_batch / snp_frame_read_indexed_batch ----------------------------------------------------------------------------------------
def index_call(cd, streams, max_spans=None, max_entries=None, lead=1, gap=3):
    """snp_frame_index_batch called directly, every array guarded: -> the index as the model states it (dict of lists, with result)."""
    ns = len(streams)
    IL = N.frame_index_lib()
    cd._bind()
    if max_spans is None or max_entries is None:
        want = X.build_index(streams)
        max_spans = want["result"][2] if max_spans is None else max_spans
        max_entries = want["result"][0] if max_entries is None else max_entries
    framed, in_off, in_len = H.pack(streams, lead, gap) if ns else (torch.zeros(16, dtype=torch.uint8, device="cuda"), [], [])
    first, total, tail = Guarded(ns + 1, torch.int64), Guarded(ns, torch.int64), Guarded(ns, torch.int32)
    start, pos, result = Guarded(max_entries, torch.int64), Guarded(max_entries, torch.int64), Guarded(4, torch.int64)
    work = Guarded(IL.snp_frame_index_workspace(ns, max_spans), torch.uint8)
    tabs = [dev_u64(in_off), dev_u64(in_len)]
    st = IL.snp_frame_index_batch(cd.ctx.handle, _p(framed), _p(tabs[0]), _p(tabs[1]), ns, max_spans, max_entries, first.ptr(), start.ptr(), pos.ptr(),
                                  total.ptr(), tail.ptr(), work.ptr(), result.ptr())
    assert st == O.OK
    torch.cuda.synchronize()
    work.read()
    ix = {"first": first.read(), "start": start.read(), "pos": pos.read(), "total": total.read(), "tail": tail.read(), "result": result.read()}
    used = ix["first"][ns] if ns else 0
    assert 0 <= used <= max_entries
    assert all(v == UNTOUCHED for v in ix["start"][used:] + ix["pos"][used:]), "a row beyond the index"
    ix["start"], ix["pos"] = ix["start"][:used], ix["pos"][:used]
    return ix


def read_call(cd, streams, ix, requests, caps, mc, ec, lead=1, gap=3, nentries=None):
    """snp_frame_read_indexed_batch called directly, every output guarded, the arena canary-filled:
    -> (status, out_len, bytes per request (None unless OK), d_result)."""
    ns, nreq = len(streams), len(requests)
    IL = N.frame_index_lib()
    cd._bind()
    framed, in_off, in_len = H.pack(streams, lead, gap) if ns else (torch.zeros(16, dtype=torch.uint8, device="cuda"), [], [])
    out_off, total = H.out_layout(caps)
    out = torch.full((max(total, 1),), CANARY, dtype=torch.uint8, device="cuda")
    out_len, status, result = Guarded(nreq, torch.int64), Guarded(nreq, torch.int32), Guarded(4, torch.int64)
    work = Guarded(IL.snp_frame_read_indexed_workspace(nreq, mc, ec), torch.uint8)
    ne = min(len(ix["start"]), len(ix["pos"])) if nentries is None else nentries
    tabs = [dev_u64(x) for x in (in_off, in_len, ix["first"], ix["start"] or [0], ix["pos"] or [0], ix["total"])] + [dev_i32(ix["tail"])] + \
        [dev_i32([b - (1 << 32) if b >= 1 << 31 else b for b, _, _ in requests])] + \
        [dev_u64(x) for x in ([r[1] for r in requests], [r[2] for r in requests], out_off, caps)]   # (named: they outlive the call)
    st = IL.snp_frame_read_indexed_batch(cd.ctx.handle, _p(framed), _p(tabs[0]), _p(tabs[1]), ns, *[_p(t) for t in tabs[2:7]], ne,
                                         _p(tabs[7]), _p(tabs[8]), _p(tabs[9]), nreq, mc, ec, _p(out), _p(tabs[10]), _p(tabs[11]),
                                         out_len.ptr(), status.ptr(), work.ptr(), result.ptr())
    assert st == O.OK
    torch.cuda.synchronize()
    work.read()
    st, ol, res, h = status.read(), out_len.read(), result.read(), out.cpu().numpy()
    # nothing outside [out_off, out_off + out_len) of an OK request, nor outside [out_off, out_off + out_cap) of any other
    assert (H.outside_ranges(h, out_off, [n if s == O.OK else c for s, n, c in zip(st, ol, caps)]) == CANARY).all(), "a write outside the output ranges"
    data = [h[o:o + n].tobytes() if s == O.OK else None for s, n, o in zip(st, ol, out_off.tolist())]
    return st, ol, data, res

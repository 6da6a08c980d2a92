"""Shared by the GPU tests of snp_frame_compose_indexed_batch (test_gpu_frame_compose.py): the call made directly through its library, in the
manner of rechunk_harness.Rechunked -- every output array and the workspace between guard elements, every out region canary-filled.  After the
call `in`, the old index, the segment list and the tables are compared with copies made before it, nothing outside [out_off, out_off + out_len)
of a written output has changed, and there are no rows beyond new_first[nout]."""
import numpy as np
import torch

import frame_buffers_helpers as H
import frame_compose_model as CM
import oracle as O
from seekable_harness import CANARY, KEYS, UNTOUCHED, Guarded, _p, index_tensors, s64, words

if torch.cuda.is_available():
    from snappier_amd import batch as SB, _native as N


def seg_tensors(segs):
    """The four arrays of a segment list (any lists at all) on the device, and nsegs."""
    nsegs = min(len(segs["stream"]), len(segs["off"]), len(segs["len"]))
    stream = torch.tensor([int(v) & 0xFFFFFFFF for v in segs["stream"][:nsegs]], dtype=torch.int64, device="cuda").to(torch.int32)
    return [words(segs["first"]), stream, words(segs["off"][:nsegs]), words(segs["len"][:nsegs])], nsegs


class Composed:
    """One call of snp_frame_compose_indexed_batch; .got has the keys of the model's compose_plan (but `alone`).  caps None: the model's size
    bound.  Bounds None: what the model needs.  model False (batches the model is too slow for: caps and the three bounds are then the
    caller's): .want is None, and the caller checks .got by its consequences."""

    def __init__(self, cd, streams, ix, segs, cb, caps=None, max_slots=None, stage_cap=None, max_entries=None, variant=O.HASH_CRC32C, model=True):
        ns, nout = len(streams), len(segs["first"]) - 1
        CL = N.frame_compose_lib()
        cd._bind()
        if model:
            free = CM.compose_plan(streams, ix, segs, cb, variant=variant)
            caps = list(free["out_bound"]) if caps is None else caps
            max_slots = free["result"][0] if max_slots is None else max_slots
            stage_cap = free["result"][2] if stage_cap is None else stage_cap
            max_entries = free["result"][4] if max_entries is None else max_entries
        self.streams, self.cb, self.caps, self.ms, self.sc, self.me = streams, cb, caps, max_slots, stage_cap, max_entries
        ms, sc, me = max_slots, stage_cap, max_entries
        self.want = CM.compose_plan(streams, ix, segs, cb, caps, ms, sc, me, variant) if model else None
        self.data, in_off, lens = H.pack(streams)
        self.out_off, total = H.out_layout(np.array(caps, dtype=np.int64))
        self.out = torch.full((total,), CANARY, dtype=torch.uint8, device="cuda")
        self.ix, ne = index_tensors(ix, ns)
        self.segs, nsegs = seg_tensors(segs)
        self.out_len, self.status, self.bound, self.result = Guarded(nout, torch.int64), Guarded(nout, torch.int32), Guarded(nout, torch.int64), Guarded(6, torch.int64)
        self.new = [Guarded(nout + 1, torch.int64), Guarded(me, torch.int64), Guarded(me, torch.int64), Guarded(nout, torch.int64), Guarded(nout, torch.int32)]
        work = Guarded(CL.snp_frame_compose_indexed_workspace(ns, nout, nsegs, ms, sc, cb, me), torch.uint8)
        self.tabs = [H.dev(in_off), H.dev(lens), H.dev(self.out_off), words(caps)]
        read_only = [self.data] + self.ix + self.segs + self.tabs
        before = [t.clone() for t in read_only]
        st = CL.snp_frame_compose_indexed_batch(cd.ctx.handle, _p(self.data), _p(self.tabs[0]), _p(self.tabs[1]), ns, *[_p(t) for t in self.ix], ne,
                                                *[_p(t) for t in self.segs], nout, nsegs, cb, ms, sc, me, _p(self.out), _p(self.tabs[2]),
                                                _p(self.tabs[3]), self.out_len.ptr(), self.status.ptr(), *[g.ptr() for g in self.new],
                                                self.bound.ptr(), work.ptr(), self.result.ptr())
        assert st == O.OK
        torch.cuda.synchronize()
        work.read()
        assert all(torch.equal(a, b) for a, b in zip(read_only, before)), "an input of the call changed"
        status, out_len = self.status.read(), self.out_len.read()
        self.h = self.out.cpu().numpy()
        # nothing outside [out_off, out_off + out_len) of a written output; any other output (out_len 0) has its whole range left untouched
        assert (H.outside_ranges(self.h, self.out_off, out_len) == CANARY).all(), "a write outside the output ranges"
        new = [self.h[o:o + n].tobytes() if s == O.OK and n else None for s, n, o in zip(status, out_len, self.out_off.tolist())]
        index = [g.read() for g in self.new]
        used = index[0][nout] if nout else 0
        assert 0 <= used <= me and all(v == UNTOUCHED for v in index[1][used:] + index[2][used:]), "a row beyond the index"
        index[1], index[2] = index[1][:used], index[2][:used]
        self.got = dict(status=status, out_len=out_len, streams=new, index=dict(zip(KEYS, index)), out_bound=self.bound.read(), result=self.result.read())

    def check(self):
        w = self.want
        assert self.got["status"] == w["status"]
        assert self.got["out_len"] == w["out_len"]
        assert self.got["out_bound"] == [s64(v) for v in w["out_bound"]]
        assert self.got["result"] == [s64(v) for v in w["result"]]
        for j, (g, x) in enumerate(zip(self.got["streams"], w["streams"])):
            assert g == x, j
        for key in KEYS:
            assert self.got["index"][key] == [s64(v) for v in w["index"][key]], key
        return self

    def written(self):
        """The outputs that were written, as bytes (None for the others)."""
        return self.got["streams"]

    def frame_index(self):
        """The new index as the wrapper's calls take it (the arrays the call wrote, on the device)."""
        used = self.got["index"]["first"][-1]
        return SB.FrameIndex(self.new[0].mid, self.new[1].mid[:used], self.new[2].mid[:used], self.new[3].mid, self.new[4].mid, None)

    def table(self):
        """(framed, off, len) of the outputs where the call wrote them: what the sibling calls take together with frame_index()."""
        return self.out, self.tabs[2], self.out_len.mid

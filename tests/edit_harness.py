"""Shared by the GPU tests of snp_frame_edit_indexed_batch (test_gpu_frame_edit.py): the call made directly through its library, in the manner of
splice_harness.Spliced -- every output array and the workspace between guard elements, every out region canary-filled.  After the call `in`,
`src`, the edit arrays and the old index are compared with copies made before it, and nothing outside [out_off, out_off + out_len) of a written
stream has changed."""
import numpy as np
import torch

import frame_buffers_helpers as H
import frame_edit_model as E
import oracle as O
from seekable_harness import CANARY, KEYS, UNTOUCHED, Guarded, _p, index_tensors, s64, words

if torch.cuda.is_available():
    from snappier_amd import _native as N


class Edited:
    """One call of snp_frame_edit_indexed_batch; .got has the keys of the model's edit_plan.  scripts: per stream a list of (off, del, src
    bytes) -- or ed_first / edits / srcs given flat, for lists no script gives (a malformed ed_first).  caps None: the model's size bound.
    Bounds None: what the model needs."""

    def __init__(self, cd, streams, ix, scripts, cb, caps=None, max_slots=None, stage_cap=None, variant=O.HASH_CRC32C, flat=None):
        ns = len(streams)
        EL = N.frame_edit_lib()
        cd._bind()
        ed_first, edits, srcs = E.flat(scripts) if flat is None else flat
        nedits = len(edits)
        free = E.edit_plan(streams, ix, ed_first, edits, srcs, cb, variant=variant)
        caps = list(free["out_bound"]) if caps is None else caps
        ms = free["result"][0] if max_slots is None else max_slots
        sc = free["result"][2] if stage_cap is None else stage_cap
        self.streams, self.cb, self.caps, self.ms, self.sc, self.edits, self.srcs, self.ed_first = streams, cb, caps, ms, sc, edits, srcs, ed_first
        self.want = E.edit_plan(streams, ix, ed_first, edits, srcs, cb, caps, ms, sc, variant)
        self.data, in_off, lens = H.pack(streams)
        self.src, src_off, src_len = H.pack(srcs, lead=5, gap=2) if nedits else (torch.zeros(16, dtype=torch.uint8, device="cuda"), [], [])
        self.out_off, total = H.out_layout(np.array(caps, dtype=np.int64))
        self.out = torch.full((total,), CANARY, dtype=torch.uint8, device="cuda")
        self.ix, ne = index_tensors(ix, ns)
        rows = ne + ms
        self.out_len, self.status, self.bound, self.result = Guarded(ns, torch.int64), Guarded(ns, torch.int32), Guarded(ns, torch.int64), Guarded(4, torch.int64)
        self.ed_status = Guarded(nedits, torch.int32)
        self.new = [Guarded(ns + 1, torch.int64), Guarded(rows, torch.int64), Guarded(rows, torch.int64), Guarded(ns, torch.int64), Guarded(ns, torch.int32)]
        work = Guarded(EL.snp_frame_edit_indexed_workspace(ns, nedits, ms, sc, cb), torch.uint8)
        self.tabs = [H.dev(in_off), H.dev(lens), words(ed_first), words([r[0] for r in edits]), words([r[1] for r in edits]), H.dev(src_len),
                     H.dev(src_off), H.dev(self.out_off), words(caps)]
        read_only = [self.data, self.src] + self.ix + self.tabs
        before = [t.clone() for t in read_only]
        st = EL.snp_frame_edit_indexed_batch(cd.ctx.handle, _p(self.data), _p(self.tabs[0]), _p(self.tabs[1]), ns, *[_p(t) for t in self.ix], ne,
                                             _p(self.src), _p(self.tabs[2]), _p(self.tabs[3]), _p(self.tabs[4]), _p(self.tabs[5]), _p(self.tabs[6]),
                                             nedits, cb, ms, sc, _p(self.out), _p(self.tabs[7]), _p(self.tabs[8]), self.out_len.ptr(),
                                             self.status.ptr(), self.ed_status.ptr(), *[g.ptr() for g in self.new], self.bound.ptr(), work.ptr(),
                                             self.result.ptr())
        assert st == O.OK
        torch.cuda.synchronize()
        work.read()
        assert all(torch.equal(a, b) for a, b in zip(read_only, before)), "an input of the call changed"
        status, out_len = self.status.read(), self.out_len.read()
        self.h = self.out.cpu().numpy()
        assert (H.outside_ranges(self.h, self.out_off, out_len) == CANARY).all(), "a write outside the output ranges"
        new = [self.h[o:o + n].tobytes() if s == O.OK and n else None for s, n, o in zip(status, out_len, self.out_off.tolist())]
        index = [g.read() for g in self.new]
        used = index[0][ns] if ns else 0
        assert 0 <= used <= rows and all(v == UNTOUCHED for v in index[1][used:] + index[2][used:]), "a row beyond the index"
        index[1], index[2] = index[1][:used], index[2][:used]
        self.got = dict(status=status, ed_status=self.ed_status.read(), out_len=out_len, streams=new, index=dict(zip(KEYS, index)),
                        out_bound=self.bound.read(), result=self.result.read())

    def check(self):
        w = self.want
        assert self.got["ed_status"] == w["ed_status"]
        assert self.got["status"] == w["status"]
        assert self.got["out_len"] == w["out_len"]
        assert self.got["out_bound"] == [s64(v) for v in w["out_bound"]]
        assert self.got["result"] == [s64(v) for v in w["result"]]
        for b, (g, x) in enumerate(zip(self.got["streams"], w["streams"])):
            assert g == x, b
        for key in KEYS:
            assert self.got["index"][key] == [s64(v) for v in w["index"][key]], key
        return self

    def after(self):
        """The batch after the call, as bytes."""
        return [n if n is not None else s for s, n in zip(self.streams, self.got["streams"])]

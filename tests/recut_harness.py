"""Shared by the GPU tests of snp_frame_recut_indexed_batch (test_gpu_frame_recut.py): the call made directly through its library, in the manner of
rechunk_harness.Rechunked -- every output array and the workspace between guard elements, every out region canary-filled.  After the call `in`,
the old index, the cut list and the tables are compared with copies made before it, and nothing outside [out_off, out_off + out_len) of a
written stream has changed."""
import numpy as np
import torch

import frame_buffers_helpers as H
import frame_recut_model as RX
import oracle as O
from seekable_harness import CANARY, KEYS, UNTOUCHED, Guarded, _p, index_tensors, s64, words

if torch.cuda.is_available():
    from snappier_amd import batch as SB, _native as N


class Recut:
    """One call of snp_frame_recut_indexed_batch; .got has the keys of the model's recut_plan (but `alone` and `plans`).  caps None: the model's
    size bound.  Bounds None: what the model needs.  model False (batches the model is too slow for: caps and the three bounds are then the
    caller's): .want is None, and the caller checks .got by its consequences.  ncuts None: the list's length."""

    def __init__(self, cd, streams, ix, cut_first, cuts, flags=0, caps=None, max_slots=None, stage_cap=None, max_entries=None, variant=O.HASH_CRC32C,
                 model=True, ncuts=None):
        ns = len(streams)
        RL = N.frame_recut_lib()
        cd._bind()
        ncuts = len(cuts) if ncuts is None else ncuts
        if model:
            free = RX.recut_plan(streams, ix, cut_first, cuts, flags, variant=variant, ncuts=ncuts)
            caps = list(free["out_bound"]) if caps is None else caps
            max_slots = free["result"][0] if max_slots is None else max_slots
            stage_cap = free["result"][2] if stage_cap is None else stage_cap
            max_entries = free["result"][4] if max_entries is None else max_entries
        self.streams, self.caps, self.ms, self.sc, self.me = streams, caps, max_slots, stage_cap, max_entries
        ms, sc, me = max_slots, stage_cap, max_entries
        self.want = RX.recut_plan(streams, ix, cut_first, cuts, flags, caps, ms, sc, me, variant, ncuts) if model else None
        self.data, in_off, lens = H.pack(streams)
        self.out_off, total = H.out_layout(np.array(caps, dtype=np.int64))
        self.out = torch.full((total,), CANARY, dtype=torch.uint8, device="cuda")
        self.ix, ne = index_tensors(ix, ns)
        # the list as the call is told it is: exactly ncuts values between guards, so that a read at or above ncuts meets a guard's page or a
        # value no list holds
        self.cut_first, self.cuts = words(cut_first), words(list(cuts[:ncuts]) + [UNTOUCHED & 0x7FFFFFFFFFFFFFFF] * 4)
        self.out_len, self.status, self.bound, self.result = Guarded(ns, torch.int64), Guarded(ns, torch.int32), Guarded(ns, torch.int64), Guarded(8, torch.int64)
        self.new = [Guarded(ns + 1, torch.int64), Guarded(me, torch.int64), Guarded(me, torch.int64), Guarded(ns, torch.int64), Guarded(ns, torch.int32)]
        work = Guarded(RL.snp_frame_recut_indexed_workspace(ns, ms, sc, me), torch.uint8)
        self.tabs = [H.dev(in_off), H.dev(lens), H.dev(self.out_off), words(caps)]
        read_only = [self.data] + self.ix + self.tabs + [self.cut_first, self.cuts]
        before = [t.clone() for t in read_only]
        st = RL.snp_frame_recut_indexed_batch(cd.ctx.handle, _p(self.data), _p(self.tabs[0]), _p(self.tabs[1]), ns, *[_p(t) for t in self.ix], ne,
                                              _p(self.cut_first), _p(self.cuts), ncuts, flags, ms, sc, me, _p(self.out), _p(self.tabs[2]),
                                              _p(self.tabs[3]), self.out_len.ptr(), self.status.ptr(), *[g.ptr() for g in self.new], self.bound.ptr(),
                                              work.ptr(), self.result.ptr())
        assert st == O.OK
        torch.cuda.synchronize()
        work.read()
        assert all(torch.equal(a, b) for a, b in zip(read_only, before)), "an input of the call changed"
        status, out_len = self.status.read(), self.out_len.read()
        self.h = self.out.cpu().numpy()
        # nothing outside [out_off, out_off + out_len) of a written stream; any other stream (out_len 0) has its whole range left untouched
        assert (H.outside_ranges(self.h, self.out_off, out_len) == CANARY).all(), "a write outside the output ranges"
        new = [self.h[o:o + n].tobytes() if s == O.OK and n else None for s, n, o in zip(status, out_len, self.out_off.tolist())]
        index = [g.read() for g in self.new]
        used = index[0][ns] if ns else 0
        assert 0 <= used <= me and all(v == UNTOUCHED for v in index[1][used:] + index[2][used:]), "a row beyond the index"
        index[1], index[2] = index[1][:used], index[2][:used]
        self.got = dict(status=status, out_len=out_len, streams=new, index=dict(zip(KEYS, index)), out_bound=self.bound.read(), result=self.result.read())

    def check(self):
        w = self.want
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

    def frame_index(self):
        """The new index as the wrapper's calls take it (the arrays the call wrote, on the device)."""
        used = self.got["index"]["first"][-1]
        return SB.FrameIndex(self.new[0].mid, self.new[1].mid[:used], self.new[2].mid[:used], self.new[3].mid, self.new[4].mid, None)


def new_table(rc):
    """(framed, off, len) of the batch after a Recut call, packed anew: what the sibling calls take together with rc.frame_index()."""
    framed, off, lens = H.pack(rc.after())
    return framed, H.dev(off), H.dev(lens)

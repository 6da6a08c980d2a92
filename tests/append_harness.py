"""Shared by the GPU tests of snp_frame_append_indexed_batch (test_gpu_frame_append.py): the call made directly through its library, in the manner
of seekable_harness.Updated -- every output array between guard elements, the workspace guarded, every stream in a region of an arena that is
canary-filled behind it.  After the call every region is checked: the bytes before the cut are the old stream's, a stream that is not written
has not one byte changed, and nothing beyond the new length was touched."""
import numpy as np
import torch

import frame_append_model as A
import frame_buffers_helpers as H
import oracle as O
from seekable_harness import CANARY, KEYS, UNTOUCHED, Guarded, _p, index_tensors, s64, words

if torch.cuda.is_available():
    from snappier_amd import batch as SB, _native as N


def arena_of(streams, caps):
    """Stream b at the start of a region of caps[b] bytes, canary bytes behind it and between the regions: -> (device tensor, offsets)."""
    off, total = H.out_layout(np.array(caps, dtype=np.int64))
    h = np.full(max(total, 1), CANARY, dtype=np.uint8)
    for s, o in zip(streams, off):
        h[o:o + len(s)] = np.frombuffer(s, dtype=np.uint8)
    return torch.from_numpy(h).cuda(), off


class Appended:
    """One call of snp_frame_append_indexed_batch; .got has the keys of the model's append_plan.  caps None: the model's size bound.  Bounds None:
    what the model needs.  model False (batches the model is too slow for: caps, max_tails and max_slots are then the caller's): .want is None,
    and the caller checks .got by its consequences."""

    def __init__(self, cd, streams, ix, srcs, cb, caps=None, max_tails=None, max_slots=None, variant=O.HASH_CRC32C, model=True):
        ns = len(streams)
        AL = N.frame_append_lib()
        cd._bind()
        if model:
            free = A.append_plan(streams, ix, srcs, cb, variant=variant)
            caps = [max(bd, len(s)) for bd, s in zip(free["out_bound"], streams)] if caps is None else caps
            max_tails = free["result"][2] if max_tails is None else max_tails
            max_slots = free["result"][0] if max_slots is None else max_slots
        self.streams, self.srcs, self.cb, self.caps, self.mt, self.ms = streams, srcs, cb, caps, max_tails, max_slots
        mt, ms = max_tails, max_slots
        self.want = A.append_plan(streams, ix, srcs, cb, caps, mt, ms, variant) if model else None
        self.buf, self.off = arena_of(streams, caps)
        self.src, src_off, src_len = H.pack(srcs, lead=5, gap=2)
        self.ix, ne = index_tensors(ix, ns)
        rows = ne + ms
        self.new_len, self.status, self.bound, self.result = Guarded(ns, torch.int64), Guarded(ns, torch.int32), Guarded(ns, torch.int64), Guarded(4, torch.int64)
        self.new = [Guarded(ns + 1, torch.int64), Guarded(rows, torch.int64), Guarded(rows, torch.int64), Guarded(ns, torch.int64), Guarded(ns, torch.int32)]
        work = Guarded(AL.snp_frame_append_indexed_workspace(ns, mt, ms, cb), torch.uint8)
        self.tabs = [H.dev(self.off), H.dev([len(s) for s in streams]), words(caps), H.dev(src_off), H.dev(src_len)]
        st = AL.snp_frame_append_indexed_batch(cd.ctx.handle, _p(self.buf), _p(self.tabs[0]), _p(self.tabs[1]), _p(self.tabs[2]), ns,
                                               *[_p(t) for t in self.ix], ne, _p(self.src), _p(self.tabs[3]), _p(self.tabs[4]), cb, mt, ms,
                                               self.new_len.ptr(), self.status.ptr(), *[g.ptr() for g in self.new], self.bound.ptr(), work.ptr(),
                                               self.result.ptr())
        assert st == O.OK
        torch.cuda.synchronize()
        work.read()
        status, new_len = self.status.read(), self.new_len.read()
        self.h = h = self.buf.cpu().numpy()
        # every region: the old stream's bytes before the cut (all of them when it is not written), canary bytes beyond the new length
        keep = [max(n, len(s)) for n, s in zip(new_len, streams)]       # (a loosely stored tail may shrink: the bytes behind it stay)
        assert (H.outside_ranges(h, self.off, keep) == CANARY).all(), "a write outside the streams"
        new = []
        for b, (s, o) in enumerate(zip(streams, self.off.tolist())):
            written = status[b] == O.OK and len(srcs[b]) > 0
            if not written:
                assert new_len[b] == len(s) and h[o:o + len(s)].tobytes() == s, "a byte of a stream that is not written changed"
            new.append(h[o:o + new_len[b]].tobytes() if written else None)
        index = [g.read() for g in self.new]
        used = index[0][ns] if ns else 0
        assert 0 <= used <= rows and all(v == UNTOUCHED for v in index[1][used:] + index[2][used:]), "a row beyond the index"
        index[1], index[2] = index[1][:used], index[2][:used]
        self.got = dict(status=status, new_len=new_len, streams=new, index=dict(zip(KEYS, index)), out_bound=self.bound.read(), result=self.result.read())

    def check(self):
        w = self.want
        for key in ("status", "new_len", "out_bound"):
            assert self.got[key] == w[key], key
        assert self.got["result"] == [s64(v) for v in w["result"]]
        for b, (g, x) in enumerate(zip(self.got["streams"], w["streams"])):
            assert g == x, b
            if g is not None:                                           # nothing before the cut was written
                assert g[:w["cut"][b]] == self.streams[b][:w["cut"][b]], b
        for key in KEYS:
            assert self.got["index"][key] == [s64(v) for v in w["index"][key]], key
        return self

    def after(self):
        """The batch after the call, as bytes."""
        return [n if n is not None else s for s, n in zip(self.streams, self.got["streams"])]

    def frame_index(self):
        """The new index as the wrapper's calls take it (the arrays the call wrote, on the device)."""
        return SB.FrameIndex(*[g.mid for g in self.new], None)

    def table(self):
        """(buf, buf_off, new_len) as the wrapper's calls take the framed streams."""
        return self.buf, self.tabs[0], self.new_len.mid

"""Device-resident batch API: thousands of independent 64 KiB blocks per launch, torch tensors as HBM buffers.

torch is plumbing here (allocation, streams, torch.distributed); the work is done by the snp_*_batch entry points.
"""
from __future__ import annotations

import ctypes as C
import itertools

import torch

from . import _native as N
from .context import Context
from .errors import raise_for_status

DIFF_PREFIX, DIFF_SUFFIX, DIFF_EXACT = N.DIFF_PREFIX, N.DIFF_SUFFIX, N.DIFF_EXACT   # the flags of BlockCodec.frame_diff_indexed


def _p(t: torch.Tensor | None):
    return C.c_void_p(t.data_ptr()) if t is not None and t.numel() else C.c_void_p(None)


class BlockCodec:
    """Wraps one snp_ctx bound to torch's current stream on `device`."""

    def __init__(self, device: int | torch.device = 0, hash_variant: int = N.HASH_CRC32C):
        self.device = torch.device("cuda", device) if isinstance(device, int) else device
        torch.cuda.set_device(self.device)
        stream = torch.cuda.current_stream(self.device).cuda_stream
        self.ctx = Context(self.device.index or 0, hash_variant, stream=stream)
        self.comp_stride = (N.lib().snp_max_compressed_length(N.BLOCK_SIZE) + 15) // 16 * 16

    def _bind(self):
        """Follow torch's current stream, so our launches are ordered with the tensors' producers and consumers."""
        self.ctx.set_stream(torch.cuda.current_stream(self.device).cuda_stream)

    def _work(self, method: str, work: torch.Tensor | None, workspace, *args: int) -> torch.Tensor:
        """The d_work of an extension call: `workspace(*args)` bytes, allocated here when the caller passed none, checked when they did."""
        need = workspace(*args)
        if work is None:
            work = torch.empty(max(need, 1), dtype=torch.uint8, device=self.device)
        if work.numel() < need:
            raise ValueError(f"{method}: work holds {work.numel()} bytes, {workspace.__name__}({', '.join(map(str, args))}) = {need}")
        return work

    def _readable(self, t: torch.Tensor, n: int) -> torch.Tensor:
        """`t`, or for an empty tensor under a batch of n > 0 empty items a 16-byte stand-in: a valid pointer that nothing reads or writes."""
        return torch.empty(16, dtype=torch.uint8, device=self.device) if n and t.numel() == 0 else t

    # -- layout helpers --------------------------------------------------------------------------------------
    def uniform_layout(self, nblocks: int, block: int = N.BLOCK_SIZE, last_len: int | None = None):
        off = torch.arange(nblocks, dtype=torch.int64, device=self.device) * block
        ln = torch.full((nblocks,), block, dtype=torch.int32, device=self.device)
        if last_len is not None and nblocks:
            ln[-1] = last_len
        return off, ln

    # -- hot path --------------------------------------------------------------------------------------------
    def compress(self, data: torch.Tensor, in_off: torch.Tensor, in_len: torch.Tensor, out: torch.Tensor | None = None,
                 out_off: torch.Tensor | None = None):
        """-> (out, out_off, out_len, status).  Block b's output starts at out_off[b] (default stride comp_stride)."""
        self._bind()
        nb = in_len.numel()
        if out_off is None:
            out_off = torch.arange(nb, dtype=torch.int64, device=self.device) * self.comp_stride
        if out is None:
            out = torch.empty(nb * self.comp_stride, dtype=torch.uint8, device=self.device)
        out_len = torch.empty(nb, dtype=torch.int32, device=self.device)
        status = torch.empty(nb, dtype=torch.int32, device=self.device)
        st = self.ctx.lib.snp_compress_batch(self.ctx.handle, _p(data), _p(in_off), _p(in_len), nb, _p(out), _p(out_off),
                                        _p(out_len), _p(status))
        raise_for_status(st, self.ctx.handle)
        return out, out_off, out_len, status

    def compress_buffers(self, data: torch.Tensor, in_off: torch.Tensor, in_len: torch.Tensor, out: torch.Tensor | None = None,
                         out_off: torch.Tensor | None = None, out_cap: torch.Tensor | None = None, max_fragments: int | None = None,
                         work: torch.Tensor | None = None):
        """Buffers of ANY length, each one Snappy block (snp_compress_buffers_batch, libsnappier_hip_buffers.so): -> (out, out_off, out_len, status, result).

        in_len holds u32 lengths (an int32 tensor's bits; lengths >= 2^31 are fine).  Defaults: out_cap = 32 + n + n // 6 + 1 + 5 per buffer
        (snp_max_compressed_length, in int64 on the device), out_off = its exclusive cumsum, out sized to the sum, and max_fragments EXACT
        (sum of ceil(n / 65536)).  Any default among out, max_fragments and work costs ONE synchronising read-back (the sums are fetched together);
        a caller that passes all three -- and out_off / out_cap -- enqueues only.  out_len is int64, status int32, result the 2-element int64
        d_result: [0] = fragments the batch needs, [1] = sum of out_len over the OK buffers."""
        self._bind()
        nb = in_len.numel()
        n = in_len.to(torch.int64) & 0xFFFFFFFF
        if out_cap is None:
            out_cap = 32 + n + n // 6 + 1 + 5
        if out_off is None:
            out_off = torch.cumsum(out_cap, 0) - out_cap
        if out is None or max_fragments is None:
            sums = torch.stack([(out_off + out_cap).max() if nb else n.new_zeros(()), ((n + N.BLOCK_SIZE - 1) // N.BLOCK_SIZE).sum()]).tolist()
            if out is None:
                out = torch.empty(max(int(sums[0]), 1), dtype=torch.uint8, device=self.device)
            if max_fragments is None:
                max_fragments = int(sums[1])
        BL = N.buffers_lib()
        work = self._work("compress_buffers", work, BL.snp_compress_buffers_workspace, nb, max_fragments)
        data = self._readable(data, nb)
        out_len = torch.empty(nb, dtype=torch.int64, device=self.device)
        status = torch.empty(nb, dtype=torch.int32, device=self.device)
        result = torch.empty(2, dtype=torch.int64, device=self.device)
        st = BL.snp_compress_buffers_batch(self.ctx.handle, _p(data), _p(in_off), _p(in_len), nb, max_fragments, _p(out), _p(out_off),
                                           _p(out_cap), _p(out_len), _p(status), _p(work), _p(result))
        raise_for_status(st, self.ctx.handle)
        return out, out_off, out_len, status, result

    def decompress(self, comp: torch.Tensor, in_off: torch.Tensor, in_len: torch.Tensor, out: torch.Tensor,
                   out_off: torch.Tensor, out_cap: torch.Tensor):
        """-> (out_len, status)."""
        self._bind()
        nb = in_len.numel()
        out_len = torch.empty(nb, dtype=torch.int32, device=self.device)
        status = torch.empty(nb, dtype=torch.int32, device=self.device)
        st = self.ctx.lib.snp_decompress_batch(self.ctx.handle, _p(comp), _p(in_off), _p(in_len), nb, _p(out), _p(out_off),
                                          _p(out_cap), _p(out_len), _p(status))
        raise_for_status(st, self.ctx.handle)
        return out_len, status

    def decompress_buffers(self, comp: torch.Tensor, in_off: torch.Tensor, in_len: torch.Tensor, out: torch.Tensor, out_off: torch.Tensor,
                           out_cap: torch.Tensor, max_fragments: int | None = None, work: torch.Tensor | None = None):
        """decompress() for batches that hold LARGE blocks (snp_decompress_buffers_batch, libsnappier_hip_buffers_decompress.so): the same
        (out_len, status) -- plus result, the 4-element int64 d_result: [0] = fragments the blocks chosen for splitting need, [1] = blocks decoded
        by fragments, [2] = chosen blocks that fell back to one wavefront, [3] = split blocks whose tag index took the look-back pass.
        Default max_fragments: sum of ceil(out_cap / 65536) over the blocks, an upper bound on what any split block can need (declared <= out_cap);
        it costs ONE synchronising read-back.  A caller that passes max_fragments and work enqueues only."""
        self._bind()
        nb = in_len.numel()
        if max_fragments is None:
            cap = out_cap.to(torch.int64) & 0xFFFFFFFF
            max_fragments = min(int(((cap + N.BLOCK_SIZE - 1) // N.BLOCK_SIZE).sum().item()) if nb else 0, 0xFFFFFFFF)
        BL = N.buffers_decompress_lib()
        work = self._work("decompress_buffers", work, BL.snp_decompress_buffers_workspace, nb, max_fragments)
        out_len = torch.empty(nb, dtype=torch.int32, device=self.device)
        status = torch.empty(nb, dtype=torch.int32, device=self.device)
        result = torch.empty(4, dtype=torch.int64, device=self.device)
        st = BL.snp_decompress_buffers_batch(self.ctx.handle, _p(comp), _p(in_off), _p(in_len), nb, max_fragments, _p(out), _p(out_off),
                                             _p(out_cap), _p(out_len), _p(status), _p(work), _p(result))
        raise_for_status(st, self.ctx.handle)
        return out_len, status, result

    def decompress_layout(self, comp: torch.Tensor, in_off: torch.Tensor, in_len: torch.Tensor, align: int = 1, arena_cap: int = 1 << 63,
                          work: torch.Tensor | None = None):
        """The output layout of a block decode from the compressed bytes alone (snp_decompress_layout_batch, libsnappier_hip_layout.so):
        -> (out_off, out_cap, declared, status, result).

        out_off (int64) and out_cap (u32 in an int32 tensor) are what decompress / decompress_buffers take; declared / status are what
        Snappy.GetUncompressedLength gives per buffer (plus the expansion rule: include/snappier_hip_layout.h).  result is the 4-element int64
        d_result: [0] = arena bytes needed, [1] = first buffer not placed, [2] = a safe max_fragments for decompress_buffers, [3] = bytes
        placed.  Nothing is read back; with `work` given (snp_decompress_layout_workspace bytes) the call enqueues only."""
        self._bind()
        nb = in_len.numel()
        LL = N.layout_lib()
        work = self._work("decompress_layout", work, LL.snp_decompress_layout_workspace, nb)
        comp = self._readable(comp, nb)
        out_off = torch.empty(nb, dtype=torch.int64, device=self.device)
        out_cap = torch.empty(nb, dtype=torch.int32, device=self.device)
        declared = torch.empty(nb, dtype=torch.int32, device=self.device)
        status = torch.empty(nb, dtype=torch.int32, device=self.device)
        result = torch.empty(4, dtype=torch.int64, device=self.device)
        st = LL.snp_decompress_layout_batch(self.ctx.handle, _p(comp), _p(in_off), _p(in_len), nb, align, arena_cap, _p(out_off), _p(out_cap),
                                            _p(declared), _p(status), _p(work), _p(result))
        raise_for_status(st, self.ctx.handle)
        return out_off, out_cap, declared, status, result

    def decompress_to_memory(self, comp: torch.Tensor, in_off: torch.Tensor, in_len: torch.Tensor, align: int = 1, max_bytes: int | None = None):
        """Decode a batch of blocks given nothing but the compressed tensor and its table (Snappy.DecompressToMemory over a batch):
        -> (out, out_off, out_len, status).

        decompress_layout, ONE synchronising read of its result, an output tensor of result[0] bytes (ValueError if that is above max_bytes:
        the sizes come from the data), then decompress_buffers with max_fragments from the result.  Block b's bytes are
        out[out_off[b] .. +out_len[b]).  status is the decoder's, except that a buffer whose preamble the layout call rejected keeps that
        status (BAD_LENGTH, INCOMPLETE): it was given no room, so the decoder could only say OUTPUT_TOO_SMALL."""
        out_off, out_cap, _, lstatus, result = self.decompress_layout(comp, in_off, in_len, align)
        need, _, frags, _ = result.tolist()
        if max_bytes is not None and need > max_bytes:
            raise ValueError(f"decompress_to_memory: the batch declares {need} bytes, max_bytes = {max_bytes}")
        out = torch.empty(max(need, 1), dtype=torch.uint8, device=self.device)
        out_len, status, _ = self.decompress_buffers(comp, in_off, in_len, out, out_off, out_cap, max_fragments=min(frags, 0xFFFFFFFF))
        return out[:need], out_off, out_len, torch.where(lstatus != N.OK, lstatus, status)

    def compact(self, data: torch.Tensor, in_off: torch.Tensor, in_len: torch.Tensor):
        """Concatenate the blocks (snp_concat_batch): -> (stream tensor sized to the exact total, dst_off).  Needs the
        total on the host (one sync) to size the result."""
        self._bind()
        nb = in_len.numel()
        lens = in_len.to(torch.int64)
        dst_off = torch.cumsum(lens, 0) - lens
        total = int(lens.sum().item()) if nb else 0
        out = torch.empty(total, dtype=torch.uint8, device=self.device)
        st = self.ctx.lib.snp_concat_batch(self.ctx.handle, _p(data), _p(in_off), _p(in_len), nb, _p(out), _p(dst_off))
        raise_for_status(st, self.ctx.handle)
        return out, dst_off

    def crc32c(self, data: torch.Tensor, in_off: torch.Tensor, in_len: torch.Tensor, masked: bool = False):
        self._bind()
        nb = in_len.numel()
        crc = torch.empty(nb, dtype=torch.int32, device=self.device)
        st = self.ctx.lib.snp_crc32c_batch(self.ctx.handle, _p(data), _p(in_off), _p(in_len), nb, int(masked), _p(crc))
        raise_for_status(st, self.ctx.handle)
        return crc

    # -- framing, device resident (config 4) --------------------------------------------------------------------
    def frame_encode(self, raw: torch.Tensor, out: torch.Tensor | None = None, work: torch.Tensor | None = None):
        """-> (framed tensor (capacity-sized), written: 1-element int64 tensor on device).  `out` / `work` may be
        passed in to reuse buffers across calls (sizes: snp_frame_max_encoded_length / snp_frame_encode_workspace)."""
        self._bind()
        n = raw.numel()
        cap = N.lib().snp_frame_max_encoded_length(n)
        need = N.lib().snp_frame_encode_workspace(n)
        if out is None:
            out = torch.empty(cap, dtype=torch.uint8, device=self.device)
        if work is None:
            work = torch.empty(need, dtype=torch.uint8, device=self.device)
        if out.numel() < cap or work.numel() < need:
            raise ValueError("frame_encode: out/work buffers too small")
        written = torch.zeros(1, dtype=torch.int64, device=self.device)
        st = self.ctx.lib.snp_frame_encode_device(self.ctx.handle, _p(raw), n, _p(out), cap, _p(written), _p(work))
        raise_for_status(st, self.ctx.handle)
        return out, written

    def frame_encode_buffers(self, data: torch.Tensor, in_off: torch.Tensor, in_len: torch.Tensor, out: torch.Tensor | None = None,
                             out_off: torch.Tensor | None = None, out_cap: torch.Tensor | None = None, max_chunks: int | None = None,
                             work: torch.Tensor | None = None):
        """Many framed streams in one call (snp_frame_encode_buffers_batch, libsnappier_hip_frame_buffers.so): -> (out, out_off, out_len, status, result).

        Buffer b is data[in_off[b] .. +in_len[b]) (int64 offsets and lengths) and becomes what frame_encode gives for it alone.  Defaults:
        out_cap = snp_frame_max_encoded_length per buffer (10 + 8 * chunks + n, in int64 on the device), out_off = its exclusive cumsum, out
        sized to the sum, and max_chunks EXACT (sum of ceil(n / 65536)).  Any default among out, max_chunks and work costs ONE synchronising
        read-back (the sums are fetched together); a caller that passes all three -- and out_off / out_cap -- enqueues only.  out_len is
        int64, status int32, result the 2-element int64 d_result: [0] = chunk slots the batch needs, [1] = sum of out_len over the OK buffers."""
        self._bind()
        nb = in_len.numel()
        n = in_len.to(torch.int64)
        chunks = (n + N.BLOCK_SIZE - 1) // N.BLOCK_SIZE
        if out_cap is None:
            out_cap = 10 + 8 * chunks + n
        if out_off is None:
            out_off = torch.cumsum(out_cap, 0) - out_cap
        if out is None or max_chunks is None:
            sums = torch.stack([(out_off + out_cap).max() if nb else n.new_zeros(()), chunks.sum()]).tolist()
            if out is None:
                out = torch.empty(max(int(sums[0]), 1), dtype=torch.uint8, device=self.device)
            if max_chunks is None:
                max_chunks = int(sums[1])
        FL = N.frame_buffers_lib()
        work = self._work("frame_encode_buffers", work, FL.snp_frame_encode_buffers_workspace, nb, max_chunks)
        data = self._readable(data, nb)
        out_len = torch.empty(nb, dtype=torch.int64, device=self.device)
        status = torch.empty(nb, dtype=torch.int32, device=self.device)
        result = torch.empty(2, dtype=torch.int64, device=self.device)
        st = FL.snp_frame_encode_buffers_batch(self.ctx.handle, _p(data), _p(in_off), _p(in_len), nb, max_chunks, _p(out), _p(out_off),
                                               _p(out_cap), _p(out_len), _p(status), _p(work), _p(result))
        raise_for_status(st, self.ctx.handle)
        return out, out_off, out_len, status, result

    def frame_encode_seekable(self, data: torch.Tensor, in_off: torch.Tensor, in_len: torch.Tensor, chunk_bytes: int = N.BLOCK_SIZE,
                              with_index: bool = True, out: torch.Tensor | None = None, out_off: torch.Tensor | None = None,
                              out_cap: torch.Tensor | None = None, max_chunks: int | None = None, work: torch.Tensor | None = None):
        """Many framed streams in one call with a chosen chunk size, and their seek index (snp_frame_encode_chunked_batch,
        libsnappier_hip_frame_chunked.so): -> (out, out_off, out_len, status, result, FrameIndex | None).

        frame_encode_buffers with one chunk per chunk_bytes (1 .. 65536) input bytes instead of per 65536: the chunk is what a window read
        decodes whole, so a caller who reads small records picks a small chunk and pays for it in compressed size.  Defaults: out_cap =
        10 + 8 * ceil(n / chunk_bytes) + n per buffer, out_off = its exclusive cumsum, out sized to the sum, and max_chunks EXACT (sum of
        ceil(n / chunk_bytes)).  Any default among out, max_chunks and work costs ONE synchronising read-back; a caller that passes all three
        -- and out_off / out_cap -- enqueues only.  result is the 4-element int64 d_result: [0] = chunk slots the batch needs, [1] = sum of
        out_len over the OK buffers, [2] = index rows written, [3] = buffers that are OK.  With with_index the returned FrameIndex (its start /
        pos hold max_chunks rows) is what frame_index_buffers gives for the emitted streams, with no header walk, and goes straight into
        frame_read_indexed / frame_gather_to_memory with (out, out_off, out_len) as the framed streams."""
        if not 1 <= chunk_bytes <= N.BLOCK_SIZE:
            raise ValueError(f"frame_encode_seekable: chunk_bytes = {chunk_bytes}, must be 1 .. {N.BLOCK_SIZE}")
        self._bind()
        nb = in_len.numel()
        n = in_len.to(torch.int64)
        chunks = (n + chunk_bytes - 1) // chunk_bytes
        if out_cap is None:
            out_cap = 10 + 8 * chunks + n
        if out_off is None:
            out_off = torch.cumsum(out_cap, 0) - out_cap
        if out is None or max_chunks is None:
            sums = torch.stack([(out_off + out_cap).max() if nb else n.new_zeros(()), chunks.sum()]).tolist()
            if out is None:
                out = torch.empty(max(int(sums[0]), 1), dtype=torch.uint8, device=self.device)
            if max_chunks is None:
                max_chunks = int(sums[1])
        CL = N.frame_chunked_lib()
        work = self._work("frame_encode_seekable", work, CL.snp_frame_encode_chunked_workspace, nb, max_chunks, chunk_bytes)
        data = self._readable(data, nb)
        out_len = torch.empty(nb, dtype=torch.int64, device=self.device)
        status = torch.empty(nb, dtype=torch.int32, device=self.device)
        result = torch.empty(4, dtype=torch.int64, device=self.device)
        index, ix = None, [None] * 5
        if with_index:
            first = torch.zeros(nb + 1, dtype=torch.int64, device=self.device)
            start = torch.empty(max(max_chunks, 1), dtype=torch.int64, device=self.device)
            pos = torch.empty(max(max_chunks, 1), dtype=torch.int64, device=self.device)
            total = torch.empty(max(nb, 1), dtype=torch.int64, device=self.device)
            tail = torch.empty(max(nb, 1), dtype=torch.int32, device=self.device)
            ix = [first, start, pos, total, tail]
            index = FrameIndex(first, start[:max_chunks], pos[:max_chunks], total[:nb], tail[:nb], result)
        st = CL.snp_frame_encode_chunked_batch(self.ctx.handle, _p(data), _p(in_off), _p(in_len), nb, chunk_bytes, max_chunks, _p(out), _p(out_off),
                                               _p(out_cap), _p(out_len), _p(status), *[_p(t) for t in ix], _p(work), _p(result))
        raise_for_status(st, self.ctx.handle)
        return out, out_off, out_len, status, result, index

    # -- content-defined chunking (libsnappier_hip_frame_cuts.so) ------------------------------------------------------------------------------
    @staticmethod
    def _check_cut_params(method: str, window: int, max_bytes: int):
        if not (N.CUTS_MIN_WINDOW <= window <= N.CUTS_MAX_WINDOW and window < max_bytes <= N.BLOCK_SIZE):
            raise ValueError(f"{method}: window = {window}, max_bytes = {max_bytes}; window must be {N.CUTS_MIN_WINDOW} .. {N.CUTS_MAX_WINDOW} "
                             f"and window < max_bytes <= {N.BLOCK_SIZE}")

    def content_cuts(self, data: torch.Tensor, in_off: torch.Tensor, in_len: torch.Tensor, window: int = 2048, max_bytes: int = 16384,
                     max_cuts: int | None = None, work: torch.Tensor | None = None, span_bytes: int | None = None):
        """Where the bytes of every buffer put its cuts (snp_content_cuts_batch, libsnappier_hip_frame_cuts.so):
        -> (cut_first, cuts, status, result).

        Buffer b is data[in_off[b] .. +in_len[b]) (int64).  Offset c of a buffer is a content cut when the gear hash of the 32 bytes before
        it is larger than that of the `window` offsets before c and no smaller than that of the `window` offsets behind it; pieces longer
        than max_bytes are cut again every max_bytes (include/snappier_hip_frame_cuts.h has the rule).  The mean piece is about 2 * window
        bytes, and an insert or delete moves the cuts behind it along with the bytes.  cuts[cut_first[b] .. cut_first[b + 1]) (int64) are
        buffer b's cuts, ascending, relative to its first byte; result is the 4-element int64 d_result: [0] = cuts the batch needs,
        [1] = cuts written, [2] = bytes the batch holds, [3] = buffers that are OK.  Defaults: max_cuts = the sum over the buffers of
        in_len / (window + 1) + in_len / max_bytes, which no buffer exceeds, and span_bytes = the sum of in_len -- ONE synchronising
        read-back for the two sums; a caller that passes max_cuts, span_bytes and work enqueues only."""
        self._check_cut_params("content_cuts", window, max_bytes)
        self._bind()
        nb = in_len.numel()
        if max_cuts is None or span_bytes is None:
            n = in_len.to(torch.int64)
            sums = torch.stack([(n // (window + 1) + n // max_bytes).sum(), n.sum()]).tolist() if nb else [0, 0]
            max_cuts = int(sums[0]) if max_cuts is None else max_cuts
            span_bytes = int(sums[1]) if span_bytes is None else span_bytes
        CL = N.frame_cuts_lib()
        work = self._work("content_cuts", work, CL.snp_content_cuts_workspace, nb, span_bytes, window)
        data = self._readable(data, nb)
        cut_first = torch.zeros(nb + 1, dtype=torch.int64, device=self.device)
        cuts = torch.empty(max(max_cuts, 1), dtype=torch.int64, device=self.device)
        status = torch.empty(nb, dtype=torch.int32, device=self.device)
        result = torch.empty(4, dtype=torch.int64, device=self.device)
        st = CL.snp_content_cuts_batch(self.ctx.handle, _p(data), _p(in_off), _p(in_len), nb, window, max_bytes, span_bytes, max_cuts,
                                       _p(cut_first), _p(cuts), _p(status), _p(work), _p(result))
        raise_for_status(st, self.ctx.handle)
        return cut_first, cuts[:max_cuts], status, result

    def frame_encode_at_cuts(self, data: torch.Tensor, in_off: torch.Tensor, in_len: torch.Tensor, cut_first: torch.Tensor, cuts: torch.Tensor,
                             with_index: bool = True, out: torch.Tensor | None = None, out_off: torch.Tensor | None = None,
                             out_cap: torch.Tensor | None = None, max_chunks: int | None = None, stage_cap: int | None = None,
                             work: torch.Tensor | None = None):
        """frame_encode_seekable with the pieces given by the caller (snp_frame_encode_cuts_batch, libsnappier_hip_frame_cuts.so):
        -> (out, out_off, out_len, status, result, FrameIndex | None), as frame_encode_seekable returns them.

        Buffer b's chunks are the pieces between cuts[cut_first[b] .. cut_first[b + 1]) (int64, ascending, inside (0, in_len[b]), relative
        to the buffer's first byte; no piece longer than 65536) -- the cuts of content_cuts, the positions of a delimiter from the find, or
        k * chunk_bytes, where every output is frame_encode_seekable's.  A buffer with a bad list gets status BAD_ARG alone.  Defaults:
        max_chunks = cuts.numel() + the buffers, out_cap = 10 + 8 * (the buffer's cuts + 1) + n per buffer (from cut_first, on the
        device), stage_cap = bytes + bytes / 6 + 69 * max_chunks, the documented bound; a default out costs ONE synchronising read-back,
        and so does a default stage_cap.  A caller that passes out, out_off, out_cap, max_chunks, stage_cap and work enqueues only."""
        self._bind()
        nb = in_len.numel()
        n = in_len.to(torch.int64)
        ncuts = cuts.numel()
        if max_chunks is None:
            max_chunks = ncuts + nb
        if out_cap is None:
            out_cap = 10 + 8 * ((cut_first[1:] - cut_first[:-1]).clamp(0, ncuts) + 1) + n
        if out_off is None:
            out_off = torch.cumsum(out_cap, 0) - out_cap
        if out is None or stage_cap is None:
            sums = torch.stack([(out_off + out_cap).max(), n.sum()]).tolist() if nb else [0, 0]
            if out is None:
                out = torch.empty(max(int(sums[0]), 1), dtype=torch.uint8, device=self.device)
            if stage_cap is None:
                stage_cap = int(sums[1]) + int(sums[1]) // 6 + 69 * max_chunks
        CL = N.frame_cuts_lib()
        work = self._work("frame_encode_at_cuts", work, CL.snp_frame_encode_cuts_workspace, nb, max_chunks, stage_cap)
        data = self._readable(data, nb)
        out_len = torch.empty(nb, dtype=torch.int64, device=self.device)
        status = torch.empty(nb, dtype=torch.int32, device=self.device)
        result = torch.empty(4, dtype=torch.int64, device=self.device)
        index, ix = None, [None] * 5
        if with_index:
            first = torch.zeros(nb + 1, dtype=torch.int64, device=self.device)
            start = torch.empty(max(max_chunks, 1), dtype=torch.int64, device=self.device)
            pos = torch.empty(max(max_chunks, 1), dtype=torch.int64, device=self.device)
            total = torch.empty(max(nb, 1), dtype=torch.int64, device=self.device)
            tail = torch.empty(max(nb, 1), dtype=torch.int32, device=self.device)
            ix = [first, start, pos, total, tail]
            index = FrameIndex(first, start[:max_chunks], pos[:max_chunks], total[:nb], tail[:nb], result)
        st = CL.snp_frame_encode_cuts_batch(self.ctx.handle, _p(data), _p(in_off), _p(in_len), nb, _p(cut_first), _p(cuts), ncuts, max_chunks,
                                            stage_cap, _p(out), _p(out_off), _p(out_cap), _p(out_len), _p(status), *[_p(t) for t in ix], _p(work),
                                            _p(result))
        raise_for_status(st, self.ctx.handle)
        return out, out_off, out_len, status, result, index

    def frame_encode_content_defined(self, data: torch.Tensor, in_off: torch.Tensor, in_len: torch.Tensor, window: int = 2048,
                                     max_bytes: int = 16384, with_index: bool = True, out: torch.Tensor | None = None,
                                     out_off: torch.Tensor | None = None, out_cap: torch.Tensor | None = None):
        """Seekable framed streams whose chunks follow the content: content_cuts and frame_encode_at_cuts back to back on the stream, with no
        read-back between them -> (out, out_off, out_len, status, result, FrameIndex | None), as frame_encode_seekable returns them.

        Everything is sized by the documented bounds, from ONE synchronising read-back of the batch's sums in front: per buffer
        in_len / (window + 1) + in_len / max_bytes cuts, one chunk more than cuts, 10 + 8 * chunks + n bytes of output.  Two versions of
        a buffer that differ by an insert or a delete, each encoded here from scratch, hold the same chunks outside the neighbourhood of the
        edit, so frame_diff_streams skips them by header CRC in both directions."""
        self._check_cut_params("frame_encode_content_defined", window, max_bytes)
        nb = in_len.numel()
        n = in_len.to(torch.int64)
        bound = n // (window + 1) + n // max_bytes                      # cuts per buffer, at the most
        if out_cap is None:
            out_cap = 10 + 8 * (bound + 1) + n
        if out_off is None:
            out_off = torch.cumsum(out_cap, 0) - out_cap
        sums = torch.stack([bound.sum(), n.sum(), (out_off + out_cap).max()]).tolist() if nb else [0, 0, 0]
        max_cuts, nbytes = int(sums[0]), int(sums[1])
        if out is None:
            out = torch.empty(max(int(sums[2]), 1), dtype=torch.uint8, device=self.device)
        cut_first, cuts, _, _ = self.content_cuts(data, in_off, in_len, window, max_bytes, max_cuts=max_cuts, span_bytes=nbytes)
        max_chunks = max_cuts + nb
        return self.frame_encode_at_cuts(data, in_off, in_len, cut_first, cuts, with_index, out, out_off, out_cap, max_chunks,
                                         nbytes + nbytes // 6 + 69 * max_chunks)

    def frame_decode_buffers(self, framed: torch.Tensor, in_off: torch.Tensor, in_len: torch.Tensor, out: torch.Tensor, out_off: torch.Tensor,
                             out_cap: torch.Tensor, max_chunks: int | None = None, max_spans: int | None = None, work: torch.Tensor | None = None):
        """Many framed streams in one call (snp_frame_decode_buffers_batch, libsnappier_hip_frame_buffers.so): -> (out_len, status, result).

        Stream b is framed[in_off[b] .. +in_len[b]) and decodes into out[out_off[b] .. +out_cap[b]) (int64 offsets, lengths and capacities);
        status[b] / out_len[b] are what frame_decode gives for it alone.  result is the 4-element int64 d_result: [0] = chunk slots the walked
        streams need, [1] = sum of out_len over the OK streams, [2] = span slots needed, [3] = spans the resolver walked on the spot.
        Default max_spans: EXACT (sum of ceil(in_len / 2^20)), ONE synchronising read-back.  Default max_chunks: a first call with max_chunks = 0
        (it walks every stream and decodes nothing), then a synchronising read of its d_result[0].  A caller that passes max_chunks, max_spans
        and work enqueues only."""
        self._bind()
        ns = in_len.numel()
        FL = N.frame_buffers_lib()
        if max_spans is None:
            n = in_len.to(torch.int64)
            max_spans = int(((n + (1 << 20) - 1) >> 20).sum().item()) if ns else 0
        framed, out = self._readable(framed, ns), self._readable(out, ns)
        out_len = torch.empty(ns, dtype=torch.int64, device=self.device)
        status = torch.empty(ns, dtype=torch.int32, device=self.device)
        result = torch.empty(4, dtype=torch.int64, device=self.device)

        def call(mc: int, w: torch.Tensor | None):
            w = self._work("frame_decode_buffers", w, FL.snp_frame_decode_buffers_workspace, ns, mc, max_spans)
            st = FL.snp_frame_decode_buffers_batch(self.ctx.handle, _p(framed), _p(in_off), _p(in_len), ns, mc, max_spans, _p(out), _p(out_off),
                                                   _p(out_cap), _p(out_len), _p(status), _p(w), _p(result))
            raise_for_status(st, self.ctx.handle)

        if max_chunks is None:
            call(0, None)
            max_chunks = min(int(result[0].item()), 0xFFFFFFFF)
        call(max_chunks, work)
        return out_len, status, result

    def frame_decode_layout(self, framed: torch.Tensor, in_off: torch.Tensor, in_len: torch.Tensor, align: int = 1, arena_cap: int = 1 << 63,
                            max_spans: int | None = None, work: torch.Tensor | None = None):
        """The output layout of a framed batch decode from the framed bytes alone (snp_frame_decode_layout_batch, libsnappier_hip_layout.so):
        -> (out_off, out_cap, decoded_len, nchunks, status, result).

        out_off / out_cap (int64) are what frame_decode_buffers takes; decoded_len / status are what snp_frame_decoded_length gives per stream,
        nchunks the data chunks its walk lists.  result is the 5-element int64 d_result: [0] = arena bytes needed, [1] = first stream not
        placed, [2] = span slots needed, [3] = the max_chunks the decode call wants, [4] = spans the resolver walked on the spot.
        Default max_spans: EXACT (sum of ceil(in_len / 2^20)), ONE synchronising read-back.  A caller that passes max_spans and work
        (snp_frame_decode_layout_workspace bytes) enqueues only."""
        self._bind()
        ns = in_len.numel()
        LL = N.layout_lib()
        if max_spans is None:
            n = in_len.to(torch.int64)
            max_spans = int(((n + (1 << 20) - 1) >> 20).sum().item()) if ns else 0
        work = self._work("frame_decode_layout", work, LL.snp_frame_decode_layout_workspace, ns, max_spans)
        framed = self._readable(framed, ns)
        out_off = torch.empty(ns, dtype=torch.int64, device=self.device)
        out_cap = torch.empty(ns, dtype=torch.int64, device=self.device)
        decoded_len = torch.empty(ns, dtype=torch.int64, device=self.device)
        nchunks = torch.empty(ns, dtype=torch.int32, device=self.device)
        status = torch.empty(ns, dtype=torch.int32, device=self.device)
        result = torch.empty(5, dtype=torch.int64, device=self.device)
        st = LL.snp_frame_decode_layout_batch(self.ctx.handle, _p(framed), _p(in_off), _p(in_len), ns, max_spans, align, arena_cap, _p(out_off),
                                              _p(out_cap), _p(decoded_len), _p(nchunks), _p(status), _p(work), _p(result))
        raise_for_status(st, self.ctx.handle)
        return out_off, out_cap, decoded_len, nchunks, status, result

    def frame_decode_to_memory(self, framed: torch.Tensor, in_off: torch.Tensor, in_len: torch.Tensor, align: int = 1, max_bytes: int | None = None):
        """Decode a batch of framed streams given nothing but the framed tensor and its table: -> (out, out_off, out_len, status).

        frame_decode_layout, ONE synchronising read of its result, an output tensor of result[0] bytes (ValueError if that is above max_bytes),
        then frame_decode_buffers with max_chunks and max_spans from the result (so without the walking call frame_decode_buffers makes to find
        max_chunks).  The layout's max_spans is bounded without a read-back by nstreams + framed bytes / 2^20; only a table whose ranges overlap
        can need more, and then the layout is made again with result[2].  status / out_len are frame_decode's for each stream alone."""
        ns = in_len.numel()
        bound = min(ns + (framed.numel() >> 20), 0xFFFFFFFF)
        out_off, out_cap, _, _, _, result = self.frame_decode_layout(framed, in_off, in_len, align, max_spans=bound)
        need, _, spans, chunks, _ = result.tolist()
        if spans > bound:
            out_off, out_cap, _, _, _, result = self.frame_decode_layout(framed, in_off, in_len, align, max_spans=spans)
            need, _, spans, chunks, _ = result.tolist()
        if max_bytes is not None and need > max_bytes:
            raise ValueError(f"frame_decode_to_memory: the batch declares {need} bytes, max_bytes = {max_bytes}")
        out = torch.empty(max(need, 1), dtype=torch.uint8, device=self.device)
        out_len, status, _ = self.frame_decode_buffers(framed, in_off, in_len, out, out_off, out_cap, max_chunks=min(chunks, 0xFFFFFFFF), max_spans=spans)
        return out[:need], out_off, out_len, status

    def frame_decode_range_buffers(self, framed: torch.Tensor, in_off: torch.Tensor, in_len: torch.Tensor, range_off: torch.Tensor,
                                   range_len: torch.Tensor, out: torch.Tensor, out_off: torch.Tensor, out_cap: torch.Tensor,
                                   max_chunks: int | None = None, max_spans: int | None = None, edge_cap: int | None = None,
                                   work: torch.Tensor | None = None):
        """A window of decoded bytes out of every framed stream (snp_frame_decode_range_batch, libsnappier_hip_frame_range.so):
        -> (out_len, status, result).

        Stream b is framed[in_off[b] .. +in_len[b]); bytes [range_off[b], range_off[b] + range_len[b]) of what it decodes to, clipped to its
        length like a read, go to out[out_off[b] .. +out_cap[b]) (int64 tensors, read as unsigned).  Only the chunks that meet the window are
        decoded and CRC-verified; a stream whose header walk ends in an error is not OK wherever its window lies (include/snappier_hip_frame_range.h).
        result is the 6-element int64 d_result: [0] = interior chunk slots needed, [1] = sum of out_len over the OK streams, [2] = span slots
        needed, [3] = spans the resolver walked on the spot, [4] = edge scratch bytes needed, [5] = chunks selected.
        Default max_spans: EXACT (sum of ceil(in_len / 2^20)), ONE synchronising read-back.  Default max_chunks and edge_cap: a first call with
        both 0 (it walks every stream and decodes nothing), then a synchronising read of its d_result[0] and [4].  A caller that passes
        max_chunks, max_spans, edge_cap and work enqueues only."""
        self._bind()
        ns = in_len.numel()
        RL = N.frame_range_lib()
        if max_spans is None:
            n = in_len.to(torch.int64)
            max_spans = int(((n + (1 << 20) - 1) >> 20).sum().item()) if ns else 0
        framed, out = self._readable(framed, ns), self._readable(out, ns)
        out_len = torch.empty(ns, dtype=torch.int64, device=self.device)
        status = torch.empty(ns, dtype=torch.int32, device=self.device)
        result = torch.empty(6, dtype=torch.int64, device=self.device)

        def call(mc: int, ec: int, w: torch.Tensor | None):
            w = self._work("frame_decode_range_buffers", w, RL.snp_frame_decode_range_workspace, ns, mc, max_spans, ec)
            st = RL.snp_frame_decode_range_batch(self.ctx.handle, _p(framed), _p(in_off), _p(in_len), ns, _p(range_off), _p(range_len), mc,
                                                 max_spans, ec, _p(out), _p(out_off), _p(out_cap), _p(out_len), _p(status), _p(w), _p(result))
            raise_for_status(st, self.ctx.handle)

        if max_chunks is None or edge_cap is None:
            call(0, 0, None)
            need = result.tolist()
            max_chunks = min(need[0], 0xFFFFFFFF) if max_chunks is None else max_chunks
            edge_cap = need[4] if edge_cap is None else edge_cap
        call(max_chunks, edge_cap, work)
        return out_len, status, result

    def frame_read_to_memory(self, framed: torch.Tensor, in_off: torch.Tensor, in_len: torch.Tensor, range_off: torch.Tensor,
                             range_len: torch.Tensor, align: int = 1, max_bytes: int | None = None):
        """Read a window of every framed stream given nothing but the framed tensor, its table and the windows: -> (out, out_off, out_len, status).

        Windows are clipped to the stream, so range_len[b] bounds what stream b delivers; so does 22 x in_len[b] (no chunk decodes to more:
        frame_hop's expansion rule).  Stream b's slot is the smaller of the two rounded up to `align`, out_off[b] the sum of the slots before
        it.  ONE sizing call (max_chunks = edge_cap = 0: it walks and decodes nothing) with ONE synchronising read of its result and of the
        arena size (ValueError if that is above max_bytes), then one decode.  max_spans is bounded without a read-back by nstreams + framed
        bytes / 2^20; only a table whose ranges overlap can need more, and then the sizing call is made again with result[2]."""
        ns = in_len.numel()
        empty = torch.empty(0, dtype=torch.uint8, device=self.device)
        if ns == 0:
            z = torch.empty(0, dtype=torch.int64, device=self.device)
            return empty, z, z.clone(), torch.empty(0, dtype=torch.int32, device=self.device)
        rl = range_len.to(torch.int64)
        bound = in_len.to(torch.int64) * 22
        out_cap = torch.where((rl < 0) | (rl > bound), bound, rl)            # (a negative int64 is a length of 2^63 or more)
        slot = (out_cap + (align - 1)) // align * align
        ends = torch.cumsum(slot, 0)
        out_off = ends - slot
        spans = min(ns + (framed.numel() >> 20), 0xFFFFFFFF)
        _, _, result = self.frame_decode_range_buffers(framed, in_off, in_len, range_off, range_len, empty, out_off, out_cap, 0, spans, 0)
        need = torch.cat([result, ends[-1:]]).tolist()
        if need[2] > spans:
            spans = need[2]
            _, _, result = self.frame_decode_range_buffers(framed, in_off, in_len, range_off, range_len, empty, out_off, out_cap, 0, spans, 0)
            need = result.tolist() + need[-1:]
        if max_bytes is not None and need[-1] > max_bytes:
            raise ValueError(f"frame_read_to_memory: the windows take {need[-1]} bytes, max_bytes = {max_bytes}")
        out = torch.empty(max(need[-1], 1), dtype=torch.uint8, device=self.device)
        out_len, status, _ = self.frame_decode_range_buffers(framed, in_off, in_len, range_off, range_len, out, out_off, out_cap,
                                                             max_chunks=min(need[0], 0xFFFFFFFF), max_spans=spans, edge_cap=need[4])
        return out[:need[-1]], out_off, out_len, status

    def frame_index_buffers(self, framed: torch.Tensor, in_off: torch.Tensor, in_len: torch.Tensor, max_spans: int | None = None,
                            max_entries: int | None = None, work: torch.Tensor | None = None) -> "FrameIndex":
        """The chunk index of many framed streams, walked once (snp_frame_index_batch, libsnappier_hip_frame_index.so): -> FrameIndex.

        Stream b is framed[in_off[b] .. +in_len[b]).  The index holds one row per data chunk (the decoded bytes before it and where its header
        is, relative to the stream's first byte), each stream's decoded length and the status of its header walk; frame_read_indexed and
        frame_gather_to_memory read any number of windows through it with no header walk, and it stays valid when the framed bytes move.
        index.result is the 4-element int64 d_result: [0] = rows needed, [1] = decoded bytes of the indexed streams, [2] = span slots needed,
        [3] = spans the resolver walked on the spot.  Default max_spans: EXACT (sum of ceil(in_len / 2^20)), ONE synchronising read-back.
        Default max_entries: a first call with max_entries = 0 (it walks every stream and writes no row), then a synchronising read of its
        d_result[0].  A caller that passes max_spans, max_entries and work enqueues only."""
        self._bind()
        ns = in_len.numel()
        IL = N.frame_index_lib()
        if max_spans is None:
            n = in_len.to(torch.int64)
            max_spans = int(((n + (1 << 20) - 1) >> 20).sum().item()) if ns else 0
        framed = self._readable(framed, ns)
        first = torch.zeros(ns + 1, dtype=torch.int64, device=self.device)
        total = torch.empty(ns, dtype=torch.int64, device=self.device)
        tail = torch.empty(ns, dtype=torch.int32, device=self.device)
        result = torch.empty(4, dtype=torch.int64, device=self.device)

        def call(me: int, w: torch.Tensor | None):
            w = self._work("frame_index_buffers", w, IL.snp_frame_index_workspace, ns, max_spans)
            start = torch.empty(max(me, 1), dtype=torch.int64, device=self.device)
            pos = torch.empty(max(me, 1), dtype=torch.int64, device=self.device)
            st = IL.snp_frame_index_batch(self.ctx.handle, _p(framed), _p(in_off), _p(in_len), ns, max_spans, me, _p(first), _p(start), _p(pos),
                                          _p(total), _p(tail), _p(w), _p(result))
            raise_for_status(st, self.ctx.handle)
            return start[:me], pos[:me]

        if max_entries is None:
            call(0, work)
            max_entries = int(result[0].item())
        start, pos = call(max_entries, work)
        return FrameIndex(first, start, pos, total, tail, result)

    def frame_read_indexed(self, framed: torch.Tensor, in_off: torch.Tensor, in_len: torch.Tensor, index: "FrameIndex", req_stream: torch.Tensor,
                           req_off: torch.Tensor, req_len: torch.Tensor, out: torch.Tensor, out_off: torch.Tensor, out_cap: torch.Tensor,
                           max_chunks: int | None = None, edge_cap: int | None = None, work: torch.Tensor | None = None):
        """Any number of windows, each naming a stream, read through a chunk index with no header walk (snp_frame_read_indexed_batch,
        libsnappier_hip_frame_index.so): -> (out_len, status, result).

        Request r reads bytes [req_off[r], req_off[r] + req_len[r]) of what stream req_stream[r] (int32) decodes to into
        out[out_off[r] .. +out_cap[r]) (int64 tensors, read as unsigned); status / out_len are what frame_decode_range_buffers gives for that
        stream alone with that window.  Requests are independent; many may name one stream.  The index is checked against the framed bytes
        row by row: a stale or foreign one gives SNP_ERR_BAD_ARG per request (include/snappier_hip_frame_index.h).  result is the 4-element
        int64 d_result: [0] = interior chunk slots needed, [1] = sum of out_len over the OK requests, [2] = edge scratch bytes needed, [3] =
        requests that are OK.  Default max_chunks and edge_cap: a first call with both 0 (it plans and decodes nothing), then a synchronising
        read of its d_result.  A caller that passes max_chunks, edge_cap and work enqueues only."""
        self._bind()
        nreq, ns = req_stream.numel(), in_len.numel()
        if req_stream.dtype != torch.int32:
            raise ValueError("frame_read_indexed: req_stream must be an int32 tensor")
        IL = N.frame_index_lib()
        framed, out = self._readable(framed, nreq), self._readable(out, nreq)
        out_len = torch.empty(nreq, dtype=torch.int64, device=self.device)
        status = torch.empty(nreq, dtype=torch.int32, device=self.device)
        result = torch.empty(4, dtype=torch.int64, device=self.device)
        start, pos = self._readable(index.start, ns), self._readable(index.pos, ns)

        def call(mc: int, ec: int, w: torch.Tensor | None):
            w = self._work("frame_read_indexed", w, IL.snp_frame_read_indexed_workspace, nreq, mc, ec)
            st = IL.snp_frame_read_indexed_batch(self.ctx.handle, _p(framed), _p(in_off), _p(in_len), ns, _p(index.first), _p(start), _p(pos),
                                                 _p(index.total), _p(index.tail), index.nentries, _p(req_stream), _p(req_off), _p(req_len), nreq,
                                                 mc, ec, _p(out), _p(out_off), _p(out_cap), _p(out_len), _p(status), _p(w), _p(result))
            raise_for_status(st, self.ctx.handle)

        if max_chunks is None or edge_cap is None:
            call(0, 0, None)
            need = result.tolist()
            max_chunks = min(need[0], 0xFFFFFFFF) if max_chunks is None else max_chunks
            edge_cap = need[2] if edge_cap is None else edge_cap
        call(max_chunks, edge_cap, work)
        return out_len, status, result

    def frame_gather_to_memory(self, framed: torch.Tensor, in_off: torch.Tensor, in_len: torch.Tensor, index: "FrameIndex", req_stream: torch.Tensor,
                               req_off: torch.Tensor, req_len: torch.Tensor, align: int = 1, max_bytes: int | None = None):
        """Read any number of windows given the framed tensor, its table, its index and the requests: -> (out, out_off, out_len, status).

        The counterpart of frame_read_to_memory.  Windows are clipped to the stream, so req_len[r] bounds what request r delivers; so does
        22 x in_len of its stream (no chunk decodes to more).  Request r's slot is the smaller of the two rounded up to `align`, out_off[r] the
        sum of the slots before it.  ONE sizing call (max_chunks = edge_cap = 0) with ONE synchronising read of its result and of the arena
        size (ValueError if that is above max_bytes), then the read."""
        nreq, ns = req_stream.numel(), in_len.numel()
        empty = torch.empty(0, dtype=torch.uint8, device=self.device)
        if nreq == 0:
            z = torch.empty(0, dtype=torch.int64, device=self.device)
            return empty, z, z.clone(), torch.empty(0, dtype=torch.int32, device=self.device)
        rl = req_len.to(torch.int64)
        rs = req_stream.to(torch.int64)
        known = (rs >= 0) & (rs < ns)
        lens = in_len.to(torch.int64)[torch.where(known, rs, torch.zeros_like(rs))] if ns else torch.zeros_like(rs)
        bound = torch.where(known, lens * 22, torch.zeros_like(rs))       # (a request on no stream of the batch delivers nothing)
        out_cap = torch.where((rl < 0) | (rl > bound), bound, rl)            # (a negative int64 is a length of 2^63 or more)
        slot = (out_cap + (align - 1)) // align * align
        ends = torch.cumsum(slot, 0)
        out_off = ends - slot
        _, _, result = self.frame_read_indexed(framed, in_off, in_len, index, req_stream, req_off, req_len, empty, out_off, out_cap, 0, 0)
        need = torch.cat([result, ends[-1:]]).tolist()
        if max_bytes is not None and need[-1] > max_bytes:
            raise ValueError(f"frame_gather_to_memory: the windows take {need[-1]} bytes, max_bytes = {max_bytes}")
        out = torch.empty(max(need[-1], 1), dtype=torch.uint8, device=self.device)
        out_len, status, _ = self.frame_read_indexed(framed, in_off, in_len, index, req_stream, req_off, req_len, out, out_off, out_cap,
                                                     max_chunks=min(need[0], 0xFFFFFFFF), edge_cap=need[2])
        return out[:need[-1]], out_off, out_len, status

    def frame_write_indexed(self, framed: torch.Tensor, in_off: torch.Tensor, in_len: torch.Tensor, index: "FrameIndex", req_stream: torch.Tensor,
                            req_off: torch.Tensor, data: torch.Tensor, data_off: torch.Tensor, data_len: torch.Tensor, out: torch.Tensor,
                            out_off: torch.Tensor, out_cap: torch.Tensor, max_slots: int | None = None, stage_cap: int | None = None,
                            work: torch.Tensor | None = None, with_bound: bool = False):
        """Replace decoded bytes of framed streams through their chunk index (snp_frame_write_indexed_batch, libsnappier_hip_frame_update.so):
        -> (out_len, status, req_status, FrameIndex, result, out_bound | None).

        Request r replaces bytes [req_off[r], req_off[r] + data_len[r]) of what stream req_stream[r] (int32) decodes to by
        data[data_off[r] .. +data_len[r]); requests are sorted by (req_stream, req_off) and byte-disjoint.  The new stream of b goes to
        out[out_off[b] .. +out_cap[b]): only the chunks a request touches are compressed again, every other byte is a copy; a stream no request
        names has out_len 0, a stream with a failing request is not written (include/snappier_hip_frame_update.h).  The returned FrameIndex
        shares first, start, total and tail with `index` and carries the positions of the new streams (for a stream that was not written:
        the old ones).  result is the 4-element int64 d_result: [0] = dirty slots needed, [1] = sum of out_len over the written streams, [2] =
        staging bytes needed, [3] = streams written.  Default max_slots and stage_cap: a first call with both 0 (it plans and writes nothing
        but copies of streams named by empty requests only), then a synchronising read of its d_result.  A caller that passes max_slots,
        stage_cap and work enqueues only."""
        self._bind()
        nreq, ns = req_stream.numel(), in_len.numel()
        if req_stream.dtype != torch.int32:
            raise ValueError("frame_write_indexed: req_stream must be an int32 tensor")
        UL = N.frame_update_lib()
        busy = nreq and ns
        framed, out, data = self._readable(framed, busy), self._readable(out, busy), self._readable(data, busy)
        out_len = torch.zeros(ns, dtype=torch.int64, device=self.device)
        status = torch.zeros(ns, dtype=torch.int32, device=self.device)
        req_status = torch.full((nreq,), N.ERR_BAD_ARG, dtype=torch.int32, device=self.device)     # (no stream at all: no request names one)
        result = torch.empty(4, dtype=torch.int64, device=self.device)
        ne = index.nentries
        new_pos = index.pos[:ne].clone()
        bound = torch.zeros(ns, dtype=torch.int64, device=self.device) if with_bound else None
        start, pos = self._readable(index.start, busy), self._readable(index.pos, busy)

        def call(ms: int, sc: int, w: torch.Tensor | None):
            w = self._work("frame_write_indexed", w, UL.snp_frame_write_indexed_workspace, ns, nreq, ms, sc)
            st = UL.snp_frame_write_indexed_batch(self.ctx.handle, _p(framed), _p(in_off), _p(in_len), ns, _p(index.first), _p(start), _p(pos),
                                                  _p(index.total), _p(index.tail), ne, _p(data), _p(req_stream), _p(req_off), _p(data_len),
                                                  _p(data_off), nreq, ms, sc, _p(out), _p(out_off), _p(out_cap), _p(out_len), _p(status),
                                                  _p(req_status), _p(new_pos), _p(bound), _p(w), _p(result))
            raise_for_status(st, self.ctx.handle)

        if max_slots is None or stage_cap is None:
            call(0, 0, None)
            need = result.tolist()
            max_slots = min(need[0], 0xFFFFFFFF) if max_slots is None else max_slots
            stage_cap = need[2] if stage_cap is None else stage_cap
        call(max_slots, stage_cap, work)
        return out_len, status, req_status, FrameIndex(index.first, index.start, new_pos, index.total, index.tail, result), result, bound

    def frame_update_to_memory(self, framed: torch.Tensor, in_off: torch.Tensor, in_len: torch.Tensor, index: "FrameIndex", req_stream: torch.Tensor,
                               req_off: torch.Tensor, data: torch.Tensor, data_off: torch.Tensor, data_len: torch.Tensor, align: int = 1,
                               max_bytes: int | None = None):
        """Update framed streams given the framed tensor, its table, its index and the requests:
        -> (out, out_off, out_len, status, req_status, FrameIndex).

        ONE sizing call (max_slots = stage_cap = 0, every out_cap 0: nothing is written) that also asks for each named stream's size bound,
        ONE synchronising read of its result and of the arena size (ValueError if that is above max_bytes), an arena in which stream b's slot
        is its bound rounded up to `align` (0 for a stream that is left alone or refused), then the write.  Streams with out_len 0 are not in
        the arena: the caller keeps their old bytes, and the returned index holds their old positions."""
        ns = in_len.numel()
        zero = torch.zeros(ns, dtype=torch.int64, device=self.device)
        empty = torch.empty(0, dtype=torch.uint8, device=self.device)
        _, _, _, _, result, bound = self.frame_write_indexed(framed, in_off, in_len, index, req_stream, req_off, data, data_off, data_len, empty,
                                                             zero, zero, 0, 0, with_bound=True)
        slot = (bound + (align - 1)) // align * align
        ends = torch.cumsum(slot, 0)
        out_off = ends - slot
        need = torch.cat([result, ends[-1:] if ns else zero[:0].new_zeros(1)]).tolist()
        if max_bytes is not None and need[-1] > max_bytes:
            raise ValueError(f"frame_update_to_memory: the new streams take up to {need[-1]} bytes, max_bytes = {max_bytes}")
        out = torch.empty(max(need[-1], 1), dtype=torch.uint8, device=self.device)
        out_len, status, req_status, new_index, _, _ = self.frame_write_indexed(framed, in_off, in_len, index, req_stream, req_off, data, data_off,
                                                                                data_len, out, out_off, bound, max_slots=min(need[0], 0xFFFFFFFF),
                                                                                stage_cap=need[2])
        return out[:need[-1]], out_off, out_len, status, req_status, new_index

    def frame_append_indexed(self, buf: torch.Tensor, buf_off: torch.Tensor, buf_len: torch.Tensor, buf_cap: torch.Tensor, index: "FrameIndex",
                             data: torch.Tensor, data_off: torch.Tensor, data_len: torch.Tensor, chunk_bytes: int, max_tails: int, max_slots: int,
                             work: torch.Tensor | None = None, with_bound: bool = False):
        """Append bytes to framed streams in place, through their chunk index (snp_frame_append_indexed_batch, libsnappier_hip_frame_append.so):
        -> (new_len, status, FrameIndex, result, out_bound | None).  The direct call: it enqueues only (it allocates its outputs, and the
        workspace when `work` is None).

        Stream b is buf[buf_off[b] .. +buf_len[b]) inside a region of buf_cap[b] bytes that it may grow into (int64 tensors, read as unsigned;
        the regions disjoint); data[data_off[b] .. +data_len[b]) is appended to what it decodes to, in chunks of chunk_bytes.  A short tail
        chunk that is physically last is reopened and encoded again where it was, the rest follows in fresh chunks; nothing before that is
        written, and a stream is appended to whole or not at all (new_len[b] = buf_len[b] then: include/snappier_hip_frame_append.h).  The
        returned FrameIndex is the batch's index after the call (start / pos hold index.nentries + max_slots rows) and goes straight into
        frame_read_indexed, frame_write_indexed and the next append, with (buf, buf_off, new_len) as the framed streams.  result is the
        4-element int64 d_result: [0] = fresh chunk slots needed, [1] = bytes the written streams grew by, [2] = reopened tails needed, [3] =
        streams written; max_tails = max_slots = 0 is the sizing call."""
        if not 1 <= chunk_bytes <= N.BLOCK_SIZE:
            raise ValueError(f"frame_append_indexed: chunk_bytes = {chunk_bytes}, must be 1 .. {N.BLOCK_SIZE}")
        self._bind()
        ns = buf_len.numel()
        AL = N.frame_append_lib()
        buf, data = self._readable(buf, ns), self._readable(data, ns)
        ne = index.nentries
        start, pos = self._readable(index.start, ns), self._readable(index.pos, ns)
        new_len = torch.empty(ns, dtype=torch.int64, device=self.device)
        status = torch.empty(ns, dtype=torch.int32, device=self.device)
        first = torch.zeros(ns + 1, dtype=torch.int64, device=self.device)
        rows = ne + max_slots
        new_start = torch.empty(max(rows, 1), dtype=torch.int64, device=self.device)
        new_pos = torch.empty(max(rows, 1), dtype=torch.int64, device=self.device)
        total = torch.empty(ns, dtype=torch.int64, device=self.device)
        tail = torch.empty(ns, dtype=torch.int32, device=self.device)
        bound = torch.zeros(ns, dtype=torch.int64, device=self.device) if with_bound else None
        result = torch.empty(4, dtype=torch.int64, device=self.device)
        w = self._work("frame_append_indexed", work, AL.snp_frame_append_indexed_workspace, ns, max_tails, max_slots, chunk_bytes)
        st = AL.snp_frame_append_indexed_batch(self.ctx.handle, _p(buf), _p(buf_off), _p(buf_len), _p(buf_cap), ns, _p(index.first), _p(start), _p(pos),
                                               _p(index.total), _p(index.tail), ne, _p(data), _p(data_off), _p(data_len), chunk_bytes, max_tails,
                                               max_slots, _p(new_len), _p(status), _p(first), _p(new_start), _p(new_pos), _p(total), _p(tail),
                                               _p(bound), _p(w), _p(result))
        raise_for_status(st, self.ctx.handle)
        return new_len, status, FrameIndex(first, new_start[:rows], new_pos[:rows], total, tail, result), result, bound

    def frame_append_to_memory(self, buf: torch.Tensor, buf_off: torch.Tensor, buf_len: torch.Tensor, buf_cap: torch.Tensor, index: "FrameIndex",
                               data: torch.Tensor, data_off: torch.Tensor, data_len: torch.Tensor, chunk_bytes: int = N.BLOCK_SIZE):
        """Append to framed streams given the arena they are kept in, its table, its index and the bytes: -> (new_len, status, FrameIndex).

        ONE sizing call (max_tails = max_slots = 0: nothing is written) with ONE synchronising read of its result, then the workspace, the new
        index (index.nentries + fresh slots rows: those of a stream that is not written stay unused at the end) and the append.  A stream whose
        region cannot hold it has status SNP_ERR_OUTPUT_TOO_SMALL and is left as it was: the caller moves it to a larger region and appends
        again."""
        _, _, _, result, _ = self.frame_append_indexed(buf, buf_off, buf_len, buf_cap, index, data, data_off, data_len, chunk_bytes, 0, 0)
        need = result.tolist()
        if need[0] > 0xFFFFFFFF or need[2] > 0xFFFFFFFF:
            raise ValueError(f"frame_append_to_memory: {need[0]} chunk slots and {need[2]} tails, one call takes 2^32 - 1 of each")
        new_len, status, new_index, _, _ = self.frame_append_indexed(buf, buf_off, buf_len, buf_cap, index, data, data_off, data_len, chunk_bytes,
                                                                     need[2], need[0])
        return new_len, status, new_index

    def frame_splice_indexed(self, framed: torch.Tensor, in_off: torch.Tensor, in_len: torch.Tensor, index: "FrameIndex", sp_off: torch.Tensor,
                             sp_del: torch.Tensor, data: torch.Tensor, data_off: torch.Tensor, data_len: torch.Tensor, chunk_bytes: int,
                             out: torch.Tensor, out_off: torch.Tensor, out_cap: torch.Tensor, max_slots: int, stage_cap: int,
                             work: torch.Tensor | None = None, with_bound: bool = False):
        """ONE splice per framed stream through its chunk index (snp_frame_splice_indexed_batch, libsnappier_hip_frame_splice.so):
        -> (out_len, status, FrameIndex, result) and, with_bound, out_bound behind them.  The direct call: it enqueues only (it allocates its
        outputs, and the workspace when `work` is None).

        In what stream b decodes to, bytes [sp_off[b], sp_off[b] + sp_del[b]) are replaced by data[data_off[b] .. +data_len[b]) (int64 tensors,
        read as unsigned): insert is sp_del 0, delete is data_len 0, truncate is sp_del = total - sp_off, and a stream with both 0 is left
        alone.  The new stream of b goes to out[out_off[b] .. +out_cap[b]): the chunks around the hole are decoded and compressed again in
        pieces of chunk_bytes, every other kept byte is a copy, and a stream is spliced whole or not at all (out_len[b] = 0 then:
        include/snappier_hip_frame_splice.h).  The returned FrameIndex is the batch's index after the call (start / pos hold index.nentries +
        max_slots rows; the old rows for a stream that is not written) and goes straight into frame_read_indexed, frame_write_indexed,
        frame_append_indexed and the next splice.  result is the 4-element int64 d_result: [0] = chunk slots needed, [1] = sum of out_len over
        the written streams, [2] = staging bytes needed, [3] = streams written; max_slots = stage_cap = 0 is the sizing call."""
        if not 1 <= chunk_bytes <= N.BLOCK_SIZE:
            raise ValueError(f"frame_splice_indexed: chunk_bytes = {chunk_bytes}, must be 1 .. {N.BLOCK_SIZE}")
        self._bind()
        ns = in_len.numel()
        SL = N.frame_splice_lib()
        framed, out, data = self._readable(framed, ns), self._readable(out, ns), self._readable(data, ns)
        ne = index.nentries
        start, pos = self._readable(index.start, ns), self._readable(index.pos, ns)
        out_len = torch.zeros(ns, dtype=torch.int64, device=self.device)
        status = torch.zeros(ns, dtype=torch.int32, device=self.device)
        first = torch.zeros(ns + 1, dtype=torch.int64, device=self.device)
        rows = ne + max_slots
        new_start = torch.empty(max(rows, 1), dtype=torch.int64, device=self.device)
        new_pos = torch.empty(max(rows, 1), dtype=torch.int64, device=self.device)
        total = torch.empty(ns, dtype=torch.int64, device=self.device)
        tail = torch.empty(ns, dtype=torch.int32, device=self.device)
        bound = torch.zeros(ns, dtype=torch.int64, device=self.device) if with_bound else None
        result = torch.empty(4, dtype=torch.int64, device=self.device)
        w = self._work("frame_splice_indexed", work, SL.snp_frame_splice_indexed_workspace, ns, max_slots, stage_cap, chunk_bytes)
        st = SL.snp_frame_splice_indexed_batch(self.ctx.handle, _p(framed), _p(in_off), _p(in_len), ns, _p(index.first), _p(start), _p(pos),
                                               _p(index.total), _p(index.tail), ne, _p(data), _p(sp_off), _p(sp_del), _p(data_len), _p(data_off),
                                               chunk_bytes, max_slots, stage_cap, _p(out), _p(out_off), _p(out_cap), _p(out_len), _p(status),
                                               _p(first), _p(new_start), _p(new_pos), _p(total), _p(tail), _p(bound), _p(w), _p(result))
        raise_for_status(st, self.ctx.handle)
        got = (out_len, status, FrameIndex(first, new_start[:rows], new_pos[:rows], total, tail, result), result)
        return got + (bound,) if with_bound else got

    def frame_splice_to_memory(self, framed: torch.Tensor, in_off: torch.Tensor, in_len: torch.Tensor, index: "FrameIndex", sp_off: torch.Tensor,
                               sp_del: torch.Tensor, data: torch.Tensor, data_off: torch.Tensor, data_len: torch.Tensor,
                               chunk_bytes: int = N.BLOCK_SIZE, align: int = 1, max_bytes: int | None = None):
        """Splice framed streams given the framed tensor, its table, its index and one splice per stream:
        -> (out, out_off, out_len, status, FrameIndex).

        ONE sizing call (max_slots = stage_cap = 0, every out_cap 0) that also asks for each named stream's size bound, ONE synchronising read
        of its result and of the arena size (ValueError if that is above max_bytes), an arena in which stream b's slot is its bound rounded up
        to `align` (0 for a stream that is left alone or refused), then the splice.  Streams with out_len 0 are not in the arena: the caller
        keeps their old bytes, and the returned index holds their old rows."""
        ns = in_len.numel()
        zero = torch.zeros(ns, dtype=torch.int64, device=self.device)
        empty = torch.empty(0, dtype=torch.uint8, device=self.device)
        _, _, _, result, bound = self.frame_splice_indexed(framed, in_off, in_len, index, sp_off, sp_del, data, data_off, data_len, chunk_bytes,
                                                           empty, zero, zero, 0, 0, with_bound=True)
        slot = (bound + (align - 1)) // align * align
        ends = torch.cumsum(slot, 0)
        out_off = ends - slot
        need = torch.cat([result, ends[-1:] if ns else zero[:0].new_zeros(1)]).tolist()
        if need[0] > 0xFFFFFFFF:
            raise ValueError(f"frame_splice_to_memory: {need[0]} chunk slots, one call takes 2^32 - 1")
        if max_bytes is not None and need[-1] > max_bytes:
            raise ValueError(f"frame_splice_to_memory: the new streams take up to {need[-1]} bytes, max_bytes = {max_bytes}")
        out = torch.empty(max(need[-1], 1), dtype=torch.uint8, device=self.device)
        out_len, status, new_index, _ = self.frame_splice_indexed(framed, in_off, in_len, index, sp_off, sp_del, data, data_off, data_len,
                                                                  chunk_bytes, out, out_off, bound, need[0], need[2])
        return out[:need[-1]], out_off, out_len, status, new_index

    def frame_rechunk_indexed(self, framed: torch.Tensor, in_off: torch.Tensor, in_len: torch.Tensor, index: "FrameIndex", chunk_bytes: int,
                              out: torch.Tensor, out_off: torch.Tensor, out_cap: torch.Tensor, max_slots: int, stage_cap: int, max_entries: int,
                              rewrite_all: bool = False, work: torch.Tensor | None = None, with_bound: bool = False):
        """Framed streams brought to canonical form through their chunk index (snp_frame_rechunk_indexed_batch,
        libsnappier_hip_frame_rechunk.so): -> (out_len, status, FrameIndex, result) and, with_bound, out_bound behind them.  The direct call: it
        enqueues only (it allocates its outputs, and the workspace when `work` is None).

        The new stream of b goes to out[out_off[b] .. +out_cap[b]) and is what frame_encode_seekable writes for the stream's decoded bytes with
        chunk_bytes: an old chunk that already is a piece of it is copied, the other pieces are decoded and compressed again; skippable, padding
        and repeated-identifier chunks are dropped.  rewrite_all decodes, verifies and compresses every chunk.  A stream that is canonical already
        is left alone (SNP_OK, out_len[b] = 0, its old rows), and a stream is rechunked whole or not at all (out_len[b] = 0 then:
        include/snappier_hip_frame_rechunk.h).  The returned FrameIndex is the batch's index after the call (start / pos hold max_entries rows)
        and goes straight into the read, update, append and splice calls and the next rechunk.  result is the 6-element int64 d_result:
        [0] = decode rows / chunk slots needed, [1] = sum of out_len, [2] = staging bytes needed, [3] = streams written, [4] = rows of the new
        index needed, [5] = streams left alone; max_slots = stage_cap = 0 is the sizing call."""
        if not 1 <= chunk_bytes <= N.BLOCK_SIZE:
            raise ValueError(f"frame_rechunk_indexed: chunk_bytes = {chunk_bytes}, must be 1 .. {N.BLOCK_SIZE}")
        self._bind()
        ns = in_len.numel()
        RL = N.frame_rechunk_lib()
        framed, out = self._readable(framed, ns), self._readable(out, ns)
        ne = index.nentries
        start, pos = self._readable(index.start, ns), self._readable(index.pos, ns)
        out_len = torch.zeros(ns, dtype=torch.int64, device=self.device)
        status = torch.zeros(ns, dtype=torch.int32, device=self.device)
        first = torch.zeros(ns + 1, dtype=torch.int64, device=self.device)
        new_start = torch.empty(max(max_entries, 1), dtype=torch.int64, device=self.device)
        new_pos = torch.empty(max(max_entries, 1), dtype=torch.int64, device=self.device)
        total = torch.empty(ns, dtype=torch.int64, device=self.device)
        tail = torch.empty(ns, dtype=torch.int32, device=self.device)
        bound = torch.zeros(ns, dtype=torch.int64, device=self.device) if with_bound else None
        result = torch.empty(6, dtype=torch.int64, device=self.device)
        w = self._work("frame_rechunk_indexed", work, RL.snp_frame_rechunk_indexed_workspace, ns, max_slots, stage_cap, chunk_bytes, max_entries)
        st = RL.snp_frame_rechunk_indexed_batch(self.ctx.handle, _p(framed), _p(in_off), _p(in_len), ns, _p(index.first), _p(start), _p(pos),
                                                _p(index.total), _p(index.tail), ne, chunk_bytes, N.RECHUNK_REWRITE_ALL if rewrite_all else 0,
                                                max_slots, stage_cap, max_entries, _p(out), _p(out_off), _p(out_cap), _p(out_len), _p(status),
                                                _p(first), _p(new_start), _p(new_pos), _p(total), _p(tail), _p(bound), _p(w), _p(result))
        raise_for_status(st, self.ctx.handle)
        got = (out_len, status, FrameIndex(first, new_start[:max_entries], new_pos[:max_entries], total, tail, result), result)
        return got + (bound,) if with_bound else got

    def frame_rechunk_to_memory(self, framed: torch.Tensor, in_off: torch.Tensor, in_len: torch.Tensor, index: "FrameIndex", chunk_bytes: int,
                                rewrite_all: bool = False, align: int = 1, max_bytes: int | None = None):
        """Rechunk framed streams given the framed tensor, its table and its index: -> (out, out_off, out_len, status, FrameIndex).

        ONE sizing call (max_slots = stage_cap = max_entries = 0, every out_cap 0) that also asks for each stream's size bound, ONE synchronising
        read of its result and of the arena size (ValueError if that is above max_bytes), an arena in which stream b's slot is its bound rounded
        up to `align` (0 for a stream that is left alone or refused), then the rechunk.  Streams with out_len 0 -- those that were canonical
        already among them -- are not in the arena: the caller keeps their old bytes, and the returned index holds their old rows."""
        ns = in_len.numel()
        zero = torch.zeros(ns, dtype=torch.int64, device=self.device)
        empty = torch.empty(0, dtype=torch.uint8, device=self.device)
        _, _, _, result, bound = self.frame_rechunk_indexed(framed, in_off, in_len, index, chunk_bytes, empty, zero, zero, 0, 0, 0, rewrite_all,
                                                            with_bound=True)
        slot = (bound + (align - 1)) // align * align
        ends = torch.cumsum(slot, 0)
        out_off = ends - slot
        need = torch.cat([result, ends[-1:] if ns else zero[:0].new_zeros(1)]).tolist()
        if need[0] > 0xFFFFFFFF or need[4] > 0xFFFFFFFF:
            raise ValueError(f"frame_rechunk_to_memory: {need[0]} chunk slots and {need[4]} index rows, one call takes 2^32 - 1 of each")
        if max_bytes is not None and need[-1] > max_bytes:
            raise ValueError(f"frame_rechunk_to_memory: the new streams take up to {need[-1]} bytes, max_bytes = {max_bytes}")
        out = torch.empty(max(need[-1], 1), dtype=torch.uint8, device=self.device)
        out_len, status, new_index, _ = self.frame_rechunk_indexed(framed, in_off, in_len, index, chunk_bytes, out, out_off, bound, need[0], need[2],
                                                                   need[4], rewrite_all)
        return out[:need[-1]], out_off, out_len, status, new_index

    # -- recut: rechunk to a caller's cut list (libsnappier_hip_frame_recut.so) ------------------------------------------------------------------
    def frame_recut_indexed(self, framed: torch.Tensor, in_off: torch.Tensor, in_len: torch.Tensor, index: "FrameIndex", cut_first: torch.Tensor,
                            cuts: torch.Tensor, out: torch.Tensor, out_off: torch.Tensor, out_cap: torch.Tensor, max_slots: int, stage_cap: int,
                            max_entries: int, rewrite_all: bool = False, work: torch.Tensor | None = None, with_bound: bool = False):
        """Framed streams brought to the pieces of a cut list through their chunk index (snp_frame_recut_indexed_batch,
        libsnappier_hip_frame_recut.so): -> (out_len, status, FrameIndex, result) and, with_bound, out_bound behind them, as
        frame_rechunk_indexed returns them.  The direct call: it enqueues only (it allocates its outputs, and the workspace when `work` is None).

        Stream b's pieces lie between cuts[cut_first[b] .. cut_first[b + 1]) (int64, ascending, inside (0, index.total[b]), relative to the
        stream's first decoded byte; no piece longer than 65536) -- what content_cuts gives for the decoded bytes, record boundaries, or a grid.
        The new stream of b goes to out[out_off[b] .. +out_cap[b]) and is what frame_encode_at_cuts writes for the stream's decoded bytes and
        that list: an old chunk that already is a piece of it is copied, the other pieces are decoded and compressed again; skippable, padding
        and repeated-identifier chunks are dropped.  rewrite_all decodes, verifies and compresses every chunk.  A stream whose chunks are the
        list's pieces already is left alone (SNP_OK, out_len[b] = 0, its old rows), a stream with a bad list gets BAD_ARG alone, and a stream
        is recut whole or not at all (include/snappier_hip_frame_recut.h).  stage_cap is ONE budget for the decoded and the compressed staging;
        2 * dbytes + dbytes / 6 + 69 * rebuilt always holds it.  result is the 8-element int64 d_result: [0] = decode rows / chunk slots needed,
        [1] = sum of out_len, [2] = staging bytes needed, [3] = streams written, [4] = rows of the new index needed, [5] = streams left alone,
        [6] = chunks copied, [7] = pieces rebuilt; max_slots = stage_cap = 0 is the sizing call."""
        self._bind()
        ns = in_len.numel()
        RL = N.frame_recut_lib()
        framed, out = self._readable(framed, ns), self._readable(out, ns)
        ne, ncuts = index.nentries, cuts.numel()
        start, pos, cuts = self._readable(index.start, ns), self._readable(index.pos, ns), self._readable(cuts, ns)
        out_len = torch.zeros(ns, dtype=torch.int64, device=self.device)
        status = torch.zeros(ns, dtype=torch.int32, device=self.device)
        first = torch.zeros(ns + 1, dtype=torch.int64, device=self.device)
        new_start = torch.empty(max(max_entries, 1), dtype=torch.int64, device=self.device)
        new_pos = torch.empty(max(max_entries, 1), dtype=torch.int64, device=self.device)
        total = torch.empty(ns, dtype=torch.int64, device=self.device)
        tail = torch.empty(ns, dtype=torch.int32, device=self.device)
        bound = torch.zeros(ns, dtype=torch.int64, device=self.device) if with_bound else None
        result = torch.empty(8, dtype=torch.int64, device=self.device)
        w = self._work("frame_recut_indexed", work, RL.snp_frame_recut_indexed_workspace, ns, max_slots, stage_cap, max_entries)
        st = RL.snp_frame_recut_indexed_batch(self.ctx.handle, _p(framed), _p(in_off), _p(in_len), ns, _p(index.first), _p(start), _p(pos),
                                              _p(index.total), _p(index.tail), ne, _p(cut_first), _p(cuts), ncuts,
                                              N.RECUT_REWRITE_ALL if rewrite_all else 0, max_slots, stage_cap, max_entries, _p(out), _p(out_off),
                                              _p(out_cap), _p(out_len), _p(status), _p(first), _p(new_start), _p(new_pos), _p(total), _p(tail),
                                              _p(bound), _p(w), _p(result))
        raise_for_status(st, self.ctx.handle)
        got = (out_len, status, FrameIndex(first, new_start[:max_entries], new_pos[:max_entries], total, tail, result), result)
        return got + (bound,) if with_bound else got

    def frame_recut_to_memory(self, framed: torch.Tensor, in_off: torch.Tensor, in_len: torch.Tensor, index: "FrameIndex", cut_first: torch.Tensor,
                              cuts: torch.Tensor, rewrite_all: bool = False, align: int = 1, max_bytes: int | None = None):
        """Recut framed streams given the framed tensor, its table, its index and the cut list: -> (out, out_off, out_len, status, FrameIndex).

        ONE sizing call (max_slots = stage_cap = max_entries = 0, every out_cap 0) that also asks for each stream's size bound, ONE synchronising
        read of its result and of the arena size (ValueError if that is above max_bytes), an arena in which stream b's slot is its bound rounded
        up to `align` (0 for a stream that is left alone or refused), then the recut with exactly what the sizing call asked for.  Streams with
        out_len 0 -- those whose chunks were the list's pieces already among them -- are not in the arena: the caller keeps their old bytes, and
        the returned index holds their old rows."""
        ns = in_len.numel()
        zero = torch.zeros(ns, dtype=torch.int64, device=self.device)
        empty = torch.empty(0, dtype=torch.uint8, device=self.device)
        _, _, _, result, bound = self.frame_recut_indexed(framed, in_off, in_len, index, cut_first, cuts, empty, zero, zero, 0, 0, 0, rewrite_all,
                                                          with_bound=True)
        slot = (bound + (align - 1)) // align * align
        ends = torch.cumsum(slot, 0)
        out_off = ends - slot
        need = torch.cat([result, ends[-1:] if ns else zero[:0].new_zeros(1)]).tolist()
        if need[0] > 0xFFFFFFFF or need[4] > 0xFFFFFFFF:
            raise ValueError(f"frame_recut_to_memory: {need[0]} chunk slots and {need[4]} index rows, one call takes 2^32 - 1 of each")
        if max_bytes is not None and need[-1] > max_bytes:
            raise ValueError(f"frame_recut_to_memory: the new streams take up to {need[-1]} bytes, max_bytes = {max_bytes}")
        out = torch.empty(max(need[-1], 1), dtype=torch.uint8, device=self.device)
        out_len, status, new_index, _ = self.frame_recut_indexed(framed, in_off, in_len, index, cut_first, cuts, out, out_off, bound, need[0],
                                                                 need[2], need[4], rewrite_all)
        return out[:need[-1]], out_off, out_len, status, new_index

    def frame_recut_content_defined(self, framed: torch.Tensor, in_off: torch.Tensor, in_len: torch.Tensor, index: "FrameIndex", window: int = 2048,
                                    max_bytes: int = 16384, rewrite_all: bool = False, align: int = 1, max_out_bytes: int | None = None):
        """Stored streams brought to the chunks frame_encode_content_defined would write for what they decode to:
        -> (out, out_off, out_len, status, FrameIndex), as frame_recut_to_memory returns them.

        Every stream is read whole with the indexed read into a TRANSIENT device tensor, content_cuts runs on it, and the recut takes the
        finder's cut_first / cuts as they lie on the device.  After an append, a splice or an edit script of a content-defined stream the cuts
        are in step again window + 32 bytes behind each edit, so almost every chunk is copied; a grid store is converted with every piece
        rebuilt.  THE TRANSIENT IS THE BATCH'S DECODED SIZE (the sum of index.total): a caller short of memory goes in parts, a slice of the
        streams at a time.  It is freed before the recut allocates its arena.  A stream that the read refuses (a corrupt chunk, an index
        that does not hold) gets the read's status, is not written and keeps its old rows.  Synchronising reads: one for the sizes of the
        transient and of the cut list, the read's sizing, the recut's sizing."""
        self._check_cut_params("frame_recut_content_defined", window, max_bytes)
        ns = in_len.numel()
        total = index.total.to(torch.int64).clamp(min=0)
        ends = torch.cumsum(total, 0)
        d_off = ends - total
        sums = torch.stack([ends[-1], (total // (window + 1) + total // max_bytes).sum()]).tolist() if ns else [0, 0]
        decoded = torch.empty(max(int(sums[0]), 1), dtype=torch.uint8, device=self.device)
        req_stream = torch.arange(ns, dtype=torch.int32, device=self.device)
        d_len, d_status, _ = self.frame_read_indexed(framed, in_off, in_len, index, req_stream, torch.zeros_like(total), total, decoded, d_off, total)
        cut_first, cuts, _, _ = self.content_cuts(decoded, d_off, d_len, window, max_bytes, max_cuts=int(sums[1]), span_bytes=int(sums[0]))
        del decoded
        # a stream the read refused goes in with the read's status as its tail: the recut hands that status back and leaves the stream alone
        failed = d_status != 0
        masked = FrameIndex(index.first, index.start, index.pos, index.total, torch.where(failed, d_status, index.tail), index.result)
        out, out_off, out_len, status, new_index = self.frame_recut_to_memory(framed, in_off, in_len, masked, cut_first, cuts, rewrite_all, align,
                                                                              max_out_bytes)
        new_index.tail = torch.where(failed, index.tail, new_index.tail)
        return out, out_off, out_len, torch.where(failed, d_status, status), new_index

    def frame_compose_indexed(self, framed: torch.Tensor, in_off: torch.Tensor, in_len: torch.Tensor, index: "FrameIndex", chunk_bytes: int,
                              out: torch.Tensor, out_off: torch.Tensor, out_cap: torch.Tensor, max_slots: int, stage_cap: int, max_entries: int,
                              seg_first: torch.Tensor, seg_stream: torch.Tensor, seg_off: torch.Tensor, seg_len: torch.Tensor,
                              work: torch.Tensor | None = None, with_bound: bool = False):
        """New framed streams made of windows of old ones through the old streams' chunk index (snp_frame_compose_indexed_batch,
        libsnappier_hip_frame_compose.so): -> (out_len, status, FrameIndex, result) and, with_bound, out_bound behind them.  The direct call: it
        enqueues only (it allocates its outputs, and the workspace when `work` is None).

        Output j is the segments [seg_first[j], seg_first[j + 1]) one behind the other (seg_first: int64, nout + 1 values); segment g is the
        decoded bytes [seg_off[g], seg_off[g] + seg_len[g]) of stream seg_stream[g] (int32).  It goes to out[out_off[j] .. +out_cap[j]): the
        chunks that lie inside a segment are copied, the chunk a segment cuts at its head or tail is decoded and the part inside compressed
        again in pieces of chunk_bytes; skippable, padding and repeated-identifier chunks are dropped.  An output is composed whole or not at
        all (out_len[j] = 0 then: include/snappier_hip_frame_compose.h).  The returned FrameIndex is the index of the OUTPUTS (start / pos hold
        max_entries rows) and goes straight into the read, update, append, splice and rechunk calls and the next compose.  result is the
        6-element int64 d_result: [0] = decode rows / chunk slots needed, [1] = sum of out_len, [2] = staging bytes needed, [3] = outputs
        written, [4] = rows of the new index needed, [5] = kept chunks copied; max_slots = stage_cap = 0 is the sizing call."""
        if not 1 <= chunk_bytes <= N.BLOCK_SIZE:
            raise ValueError(f"frame_compose_indexed: chunk_bytes = {chunk_bytes}, must be 1 .. {N.BLOCK_SIZE}")
        self._bind()
        ns, nout, nsegs = in_len.numel(), seg_first.numel() - 1, seg_stream.numel()
        if nout < 0 or seg_off.numel() != nsegs or seg_len.numel() != nsegs:
            raise ValueError("frame_compose_indexed: seg_first holds nout + 1 values; seg_stream, seg_off and seg_len one per segment")
        CL = N.frame_compose_lib()
        framed, out = self._readable(framed, ns), self._readable(out, nout)
        ne = index.nentries
        start, pos = self._readable(index.start, ns), self._readable(index.pos, ns)
        out_len = torch.zeros(nout, dtype=torch.int64, device=self.device)
        status = torch.zeros(nout, dtype=torch.int32, device=self.device)
        first = torch.zeros(nout + 1, dtype=torch.int64, device=self.device)
        new_start = torch.empty(max(max_entries, 1), dtype=torch.int64, device=self.device)
        new_pos = torch.empty(max(max_entries, 1), dtype=torch.int64, device=self.device)
        total = torch.zeros(nout, dtype=torch.int64, device=self.device)
        tail = torch.zeros(nout, dtype=torch.int32, device=self.device)
        bound = torch.zeros(nout, dtype=torch.int64, device=self.device) if with_bound else None
        result = torch.empty(6, dtype=torch.int64, device=self.device)
        w = self._work("frame_compose_indexed", work, CL.snp_frame_compose_indexed_workspace, ns, nout, nsegs, max_slots, stage_cap, chunk_bytes,
                       max_entries)
        st = CL.snp_frame_compose_indexed_batch(self.ctx.handle, _p(framed), _p(in_off), _p(in_len), ns, _p(index.first), _p(start), _p(pos),
                                                _p(index.total), _p(index.tail), ne, _p(seg_first), _p(seg_stream), _p(seg_off), _p(seg_len), nout,
                                                nsegs, chunk_bytes, max_slots, stage_cap, max_entries, _p(out), _p(out_off), _p(out_cap),
                                                _p(out_len), _p(status), _p(first), _p(new_start), _p(new_pos), _p(total), _p(tail), _p(bound),
                                                _p(w), _p(result))
        raise_for_status(st, self.ctx.handle)
        got = (out_len, status, FrameIndex(first, new_start[:max_entries], new_pos[:max_entries], total, tail, result), result)
        return got + (bound,) if with_bound else got

    def frame_compose_to_memory(self, framed: torch.Tensor, in_off: torch.Tensor, in_len: torch.Tensor, index: "FrameIndex",
                                seg_first: torch.Tensor, seg_stream: torch.Tensor, seg_off: torch.Tensor, seg_len: torch.Tensor,
                                chunk_bytes: int = N.BLOCK_SIZE, align: int = 1, max_bytes: int | None = None):
        """Compose new framed streams given the framed tensor, its table, its index and the segment list:
        -> (out, out_off, out_len, status, FrameIndex).

        ONE sizing call (max_slots = stage_cap = max_entries = 0, every out_cap 0) that also asks for each output's size bound, ONE
        synchronising read of its result and of the arena size (ValueError if that is above max_bytes), an arena in which output j's slot is its
        bound rounded up to `align` (0 for an output that is refused), then the compose.  The returned index is the outputs'."""
        nout = seg_first.numel() - 1
        zero = torch.zeros(max(nout, 0), dtype=torch.int64, device=self.device)
        empty = torch.empty(0, dtype=torch.uint8, device=self.device)
        _, _, _, result, bound = self.frame_compose_indexed(framed, in_off, in_len, index, chunk_bytes, empty, zero, zero, 0, 0, 0, seg_first,
                                                            seg_stream, seg_off, seg_len, with_bound=True)
        slot = (bound + (align - 1)) // align * align
        ends = torch.cumsum(slot, 0)
        out_off = ends - slot
        need = torch.cat([result, ends[-1:] if nout else zero[:0].new_zeros(1)]).tolist()
        if need[0] > 0xFFFFFFFF or need[4] > 0xFFFFFFFF:
            raise ValueError(f"frame_compose_to_memory: {need[0]} chunk slots and {need[4]} index rows, one call takes 2^32 - 1 of each")
        if max_bytes is not None and need[-1] > max_bytes:
            raise ValueError(f"frame_compose_to_memory: the new streams take up to {need[-1]} bytes, max_bytes = {max_bytes}")
        out = torch.empty(max(need[-1], 1), dtype=torch.uint8, device=self.device)
        out_len, status, new_index, _ = self.frame_compose_indexed(framed, in_off, in_len, index, chunk_bytes, out, out_off, bound, need[0], need[2],
                                                                   need[4], seg_first, seg_stream, seg_off, seg_len)
        return out[:need[-1]], out_off, out_len, status, new_index

    # -- dedup by chunk (libsnappier_hip_frame_dedup.so) -----------------------------------------------------------------------------------------
    def frame_dedup_indexed(self, framed: torch.Tensor, in_off: torch.Tensor, in_len: torch.Tensor, index: "FrameIndex", nbase: int,
                            max_entries: int, max_segs: int, out: torch.Tensor | None, work: torch.Tensor | None = None):
        """The duplicate chunks of a batch of seekable framed streams, the unique ones of the new streams once (snp_frame_dedup_indexed_batch,
        libsnappier_hip_frame_dedup.so): -> (out_len, status, canon, FrameIndex of the pack, recipe, result).  The direct call: it enqueues
        only (it allocates its outputs, and the workspace when `work` is None).

        The first nbase streams are the base (stored already, earlier packs for example), the others are new.  canon (int64, one per index
        row) maps every row to the lowest row whose chunk is byte-identical, to itself when there is none, and to DEDUP_NONE (-1 as int64)
        for a row of length 0 or of a stream that failed.  The pack goes to `out` (its capacity is out.numel(); None: 0): the identifier and
        the unique chunks of the admitted new streams, verbatim, with out_len (int64, 1 value) and its own FrameIndex (start / pos hold
        max_entries rows).  recipe = (seg_first, seg_stream, seg_off, seg_len) is the segment list frame_compose_indexed takes, over the
        sources base stream s -> s, the pack -> nbase (frame_restore_to_memory).  status (int32) is per stream.  result is the 8-element
        int64 d_result: [0] = unique rows, [1] = pack bytes, [2] = segments needed, [3] = streams OK, [4] = rows that take part, [5] = rows
        merged, [6] = rows with a leader's key but other bytes, [7] = chunk bytes saved; max_entries = max_segs = 0 with no `out` is the
        sizing call (include/snappier_hip_frame_dedup.h)."""
        self._bind()
        ns, ne = in_len.numel(), index.nentries
        if not 0 <= nbase <= ns:
            raise ValueError(f"frame_dedup_indexed: nbase = {nbase}, the batch holds {ns} streams")
        DL = N.frame_dedup_lib()
        framed = self._readable(framed, ns)
        start, pos = self._readable(index.start, ns), self._readable(index.pos, ns)
        out_cap = out.numel() if out is not None else 0
        dev = self.device
        out_len = torch.zeros(1, dtype=torch.int64, device=dev)
        status = torch.zeros(ns, dtype=torch.int32, device=dev)
        canon = torch.empty(max(ne, 1), dtype=torch.int64, device=dev)
        pk = [torch.zeros(2, dtype=torch.int64, device=dev), torch.empty(max(max_entries, 1), dtype=torch.int64, device=dev),
              torch.empty(max(max_entries, 1), dtype=torch.int64, device=dev), torch.zeros(1, dtype=torch.int64, device=dev),
              torch.zeros(1, dtype=torch.int32, device=dev)]
        seg_first = torch.zeros(ns - nbase + 1, dtype=torch.int64, device=dev)
        seg_stream = torch.zeros(max(max_segs, 1), dtype=torch.int32, device=dev)
        seg_off = torch.zeros(max(max_segs, 1), dtype=torch.int64, device=dev)
        seg_len = torch.zeros(max(max_segs, 1), dtype=torch.int64, device=dev)
        result = torch.empty(8, dtype=torch.int64, device=dev)
        w = self._work("frame_dedup_indexed", work, DL.snp_frame_dedup_indexed_workspace, ns, ne)
        st = DL.snp_frame_dedup_indexed_batch(self.ctx.handle, _p(framed), _p(in_off), _p(in_len), ns, _p(index.first), _p(start), _p(pos),
                                              _p(index.total), _p(index.tail), ne, nbase, max_entries, max_segs, out_cap, _p(out), _p(out_len),
                                              _p(status), _p(canon), *[_p(t) for t in pk], _p(seg_first), _p(seg_stream), _p(seg_off), _p(seg_len),
                                              _p(w), _p(result))
        raise_for_status(st, self.ctx.handle)
        pack_index = FrameIndex(pk[0], pk[1][:max_entries], pk[2][:max_entries], pk[3], pk[4], result)
        return out_len, status, canon[:ne], pack_index, (seg_first, seg_stream[:max_segs], seg_off[:max_segs], seg_len[:max_segs]), result

    def frame_dedup_to_memory(self, framed: torch.Tensor, in_off: torch.Tensor, in_len: torch.Tensor, index: "FrameIndex", nbase: int = 0):
        """Dedup a batch of seekable framed streams by chunk: -> (pack, FrameIndex of the pack, recipe, canon, status, result).

        ONE sizing call, ONE synchronising read of its result, the pack, its index and the recipe arrays allocated to exactly what the
        batch needs, then the call.  The pack is a framed stream: it goes into every seekable call with its index, and into the next
        frame_dedup_to_memory as a base stream; frame_restore_to_memory rebuilds the new streams from the base streams, the pack and the
        recipe."""
        *_, result = self.frame_dedup_indexed(framed, in_off, in_len, index, nbase, 0, 0, None)
        need = result.tolist()
        if need[0] > 0xFFFFFFFF or need[2] > 0xFFFFFFFF:
            raise ValueError(f"frame_dedup_to_memory: {need[0]} unique rows and {need[2]} segments, one call takes 2^32 - 1 of each")
        out = torch.empty(max(need[1], 10), dtype=torch.uint8, device=self.device)
        _, status, canon, pack_index, recipe, result = self.frame_dedup_indexed(framed, in_off, in_len, index, nbase, need[0], need[2], out)
        return out[:need[1]], pack_index, recipe, canon, status, result

    def frame_restore_to_memory(self, framed: torch.Tensor, in_off: torch.Tensor, in_len: torch.Tensor, index: "FrameIndex", nbase: int,
                                pack: torch.Tensor, pack_index: "FrameIndex", recipe, chunk_bytes: int = N.BLOCK_SIZE, align: int = 1,
                                max_bytes: int | None = None):
        """The new streams of a dedup again (frame_compose_to_memory on a recipe): -> (out, out_off, out_len, status, FrameIndex).

        The sources are the first nbase streams of (framed, in_off, in_len, index) and the pack with its index, as source nbase.  With base
        streams the pack is copied once behind `framed` (one torch.cat: the compose call takes one tensor); with nbase = 0 the pack alone is
        the source.  Every chunk is copied as it is, so a stream that was the identifier plus non-empty data chunks comes back byte for
        byte.  ONE synchronising read for the base streams' row count when nbase > 0, besides those of frame_compose_to_memory."""
        dev = self.device
        rows = min(int(index.first[nbase]), index.nentries) if nbase else 0
        src = torch.cat([framed, pack]) if nbase else pack
        pack_off = torch.tensor([framed.numel() if nbase else 0], dtype=torch.int64, device=dev)
        pack_len = torch.tensor([pack.numel()], dtype=torch.int64, device=dev)
        first = torch.cat([index.first[:nbase], index.first.new_full((1,), rows), pack_index.first[1:2] + rows])
        sources = FrameIndex(first, torch.cat([index.start[:rows], pack_index.start]), torch.cat([index.pos[:rows], pack_index.pos]),
                             torch.cat([index.total[:nbase], pack_index.total]), torch.cat([index.tail[:nbase], pack_index.tail]))
        return self.frame_compose_to_memory(src, torch.cat([in_off[:nbase].to(torch.int64), pack_off]),
                                            torch.cat([in_len[:nbase].to(torch.int64), pack_len]), sources, *recipe, chunk_bytes=chunk_bytes,
                                            align=align, max_bytes=max_bytes)

    # -- verify and repair (libsnappier_hip_frame_verify.so) ----------------------------------------------------------------------------------------
    def frame_verify_indexed(self, framed: torch.Tensor, in_off: torch.Tensor, in_len: torch.Tensor, index: "FrameIndex",
                             slot_bytes: int | None = None, scratch_cap: int = 256 << 20, work: torch.Tensor | None = None):
        """Which chunks of a batch of seekable framed streams are rotten (snp_frame_verify_indexed_batch, libsnappier_hip_frame_verify.so):
        -> (row_status, status, nbad, first_bad, bad_bytes, flags, result).  Nothing is written but verdicts.

        row_status (int32, one per index row) is what the framed decode gives that one chunk -- the decoder's status or ERR_CRC_MISMATCH --,
        ERR_BAD_ARG for a row the index does not describe, ERR_OUTPUT_TOO_SMALL for a row longer than slot_bytes (not verified) and
        VERIFY_SKIPPED for a row of a stream that was not looked at.  Per stream: status (int32: the stream's verdict, else its first bad
        row's status), nbad, first_bad (a global row number; VERIFY_NONE, -1 as int64, when there is none), bad_bytes (int64) and flags
        (int32; bit 0: the stream does not begin with the identifier).  Every data chunk is decoded and CRC-verified into scratch_cap bytes
        inside the workspace, in rounds of scratch_cap // (slot_bytes rounded up to 16) rows; the results do not depend on scratch_cap.
        result is the 8-element int64 d_result: [0] = rows looked at, [1] = rows not OK, [2] = decoded bytes verified, [3] = streams OK,
        [4] = the longest checked row, [5] = rows left unverified, [6] = rounds, [7] = the sum of bad_bytes
        (include/snappier_hip_frame_verify.h).  Default slot_bytes: a sizing call (scratch_cap = 0), then ONE synchronising read of its
        d_result[4].  A caller that passes slot_bytes enqueues only (the outputs, and the workspace when `work` is None, are allocated)."""
        self._bind()
        ns, ne = in_len.numel(), index.nentries
        VL = N.frame_verify_lib()
        framed = self._readable(framed, ns)
        start, pos = self._readable(index.start, ns), self._readable(index.pos, ns)
        dev = self.device
        row_status = torch.empty(max(ne, 1), dtype=torch.int32, device=dev)
        status = torch.zeros(ns, dtype=torch.int32, device=dev)
        nbad, first_bad, bad_bytes = (torch.zeros(ns, dtype=torch.int64, device=dev) for _ in range(3))
        flags = torch.zeros(ns, dtype=torch.int32, device=dev)
        result = torch.empty(8, dtype=torch.int64, device=dev)

        def call(sb: int, cap: int, w: torch.Tensor | None):
            w = self._work("frame_verify_indexed", w, VL.snp_frame_verify_indexed_workspace, ns, ne, sb, cap)
            st = VL.snp_frame_verify_indexed_batch(self.ctx.handle, _p(framed), _p(in_off), _p(in_len), ns, _p(index.first), _p(start), _p(pos),
                                                   _p(index.total), _p(index.tail), ne, sb, cap, _p(row_status), _p(status), _p(nbad),
                                                   _p(first_bad), _p(bad_bytes), _p(flags), _p(w), _p(result))
            raise_for_status(st, self.ctx.handle)

        if slot_bytes is None:
            call(N.BLOCK_SIZE, 0, None)
            slot_bytes = min(max(result.tolist()[4], 1), N.BLOCK_SIZE)
        if not 1 <= slot_bytes <= N.BLOCK_SIZE:
            raise ValueError(f"frame_verify_indexed: slot_bytes = {slot_bytes}, must be 1 .. {N.BLOCK_SIZE}")
        call(slot_bytes, scratch_cap, work)
        return row_status[:ne], status, nbad, first_bad, bad_bytes, flags, result

    def frame_repair_plan(self, index: "FrameIndex", row_status: torch.Tensor, rep_index: "FrameIndex", rp_stream: torch.Tensor,
                          rp_replica: torch.Tensor, max_segs: int, work: torch.Tensor | None = None):
        """The verdicts of frame_verify_indexed as compose recipes over a replica (snp_frame_repair_plan_batch): -> (plan_status, recipe,
        result).  The direct call: it enqueues only.

        Pair j names stream rp_stream[j] of `index` and replica rp_replica[j] of `rep_index` (int32 tensors).  Its output is the whole
        stream: every run of rows whose row_status is OK one segment of the stream itself, every run of other rows one segment of the replica
        over the same decoded range.  recipe = (seg_first, seg_stream, seg_off, seg_len) is the segment list frame_compose_indexed takes over
        the sources stream s -> s, replica t -> nstreams + t.  plan_status (int32) is per pair: ERR_BAD_ARG for a pair out of range, a stream
        or a replica whose index is not OK and totals that differ; ERR_OUTPUT_TOO_SMALL from the first pair whose segments pass max_segs.
        result is the 4-element int64 d_result: [0] = segments needed, [1] = pairs planned, [2] = bytes taken from replicas, [3] = bytes
        kept; max_segs = 0 is the sizing call."""
        self._bind()
        ns, ne, nrep, nout = index.total.numel(), min(index.start.numel(), row_status.numel()), rep_index.total.numel(), rp_stream.numel()
        if rp_stream.dtype != torch.int32 or rp_replica.dtype != torch.int32 or rp_replica.numel() != nout:
            raise ValueError("frame_repair_plan: rp_stream and rp_replica must be int32 tensors of one length")
        VL = N.frame_verify_lib()
        dev = self.device
        start = self._readable(index.start, ns)
        rows = self._readable(row_status, ns)
        plan_status = torch.zeros(nout, dtype=torch.int32, device=dev)
        seg_first = torch.zeros(nout + 1, dtype=torch.int64, device=dev)
        seg_stream = torch.zeros(max(max_segs, 1), dtype=torch.int32, device=dev)
        seg_off = torch.zeros(max(max_segs, 1), dtype=torch.int64, device=dev)
        seg_len = torch.zeros(max(max_segs, 1), dtype=torch.int64, device=dev)
        result = torch.empty(4, dtype=torch.int64, device=dev)
        w = self._work("frame_repair_plan", work, VL.snp_frame_repair_plan_workspace, nout)
        st = VL.snp_frame_repair_plan_batch(self.ctx.handle, _p(index.first), _p(start), _p(index.total), _p(index.tail), ne, ns, _p(rows),
                                            _p(rep_index.total), _p(rep_index.tail), nrep, _p(rp_stream), _p(rp_replica), nout, max_segs,
                                            _p(seg_first), _p(seg_stream), _p(seg_off), _p(seg_len), _p(plan_status), _p(w), _p(result))
        raise_for_status(st, self.ctx.handle)
        return plan_status, (seg_first, seg_stream[:max_segs], seg_off[:max_segs], seg_len[:max_segs]), result

    def frame_repair_streams(self, framed: torch.Tensor, in_off: torch.Tensor, in_len: torch.Tensor, index: "FrameIndex", rep_framed: torch.Tensor,
                             rep_off: torch.Tensor, rep_len: torch.Tensor, rep_index: "FrameIndex", chunk_bytes: int = N.BLOCK_SIZE):
        """The damaged streams of a batch built again from their good chunks and replica t = s for the bad ones:
        -> (damaged stream numbers, out, out_off, out_len, status, FrameIndex); output j is stream damaged[j].

        frame_verify_indexed; ONE synchronising read of the streams that are not OK, their bad rows (a stream with b bad rows has at most
        2 b + 1 segments, so the plan needs no sizing call) and the streams' row count; frame_repair_plan; the replicas copied once behind the streams (one torch.cat:
        the compose call takes one tensor) with the two indexes joined as frame_restore_to_memory joins them; frame_compose_to_memory; and a
        SECOND VERIFY, of the outputs: the replica chunks the compose copied were never checked.  status (int32) is the compose's where
        that failed, else the second verify's, so damage on both sides in the same range shows as a stream that is still bad.  A stream
        that was the identifier plus contiguous non-empty data chunks comes back byte for byte from an undamaged copy."""
        dev = self.device
        ns = in_len.numel()
        row_status, status, nbad, *_ = self.frame_verify_indexed(framed, in_off, in_len, index)
        seen = torch.cat([status.to(torch.int64), nbad, index.first[ns:ns + 1]]).tolist()
        damaged = [s for s in range(ns) if seen[s] != N.OK]
        if not damaged:
            none = torch.zeros(0, dtype=torch.int64, device=dev)
            empty = FrameIndex(torch.zeros(1, dtype=torch.int64, device=dev), none, none, none, torch.zeros(0, dtype=torch.int32, device=dev))
            return damaged, torch.empty(0, dtype=torch.uint8, device=dev), none, none, torch.zeros(0, dtype=torch.int32, device=dev), empty
        pairs = torch.tensor(damaged, dtype=torch.int32, device=dev)
        max_segs = sum(2 * seen[ns + s] + 1 for s in damaged)
        plan_status, recipe, _ = self.frame_repair_plan(index, row_status, rep_index, pairs, pairs, max_segs)
        rows = min(seen[2 * ns], index.nentries)
        sources = FrameIndex(torch.cat([index.first[:ns], rep_index.first + rows]), torch.cat([index.start[:rows], rep_index.start]),
                             torch.cat([index.pos[:rows], rep_index.pos]), torch.cat([index.total, rep_index.total]),
                             torch.cat([index.tail, rep_index.tail]))
        out, out_off, out_len, cst, new_index = self.frame_compose_to_memory(
            torch.cat([framed, rep_framed]), torch.cat([in_off.to(torch.int64), rep_off.to(torch.int64) + framed.numel()]),
            torch.cat([in_len.to(torch.int64), rep_len.to(torch.int64)]), sources, *recipe, chunk_bytes=chunk_bytes)
        again = self.frame_verify_indexed(out, out_off, out_len, new_index)[1]
        final = torch.where(plan_status != N.OK, plan_status, torch.where(cst != N.OK, cst, again))
        return damaged, out, out_off, out_len, final, new_index

    def frame_digest_indexed(self, framed: torch.Tensor, in_off: torch.Tensor, in_len: torch.Tensor, index: "FrameIndex", req_stream: torch.Tensor,
                             req_off: torch.Tensor, req_len: torch.Tensor, edge_cap: int | None = None, work: torch.Tensor | None = None):
        """The CRC-32C of any number of windows of what framed streams decode to, from the CRCs their chunk headers carry, with no decode of
        the chunks inside a window (snp_frame_digest_indexed_batch, libsnappier_hip_frame_digest.so): -> (digest, dig_len, status, result).

        Request r names stream req_stream[r] (int32) and the window [req_off[r], req_off[r] + req_len[r]) of what it decodes to (int64
        tensors, read as unsigned; req_off 0 and req_len -1 is the whole stream).  digest (int32, the bits of the unsigned plain CRC-32C) and
        dig_len (int64) are those of the clipped window; status is what frame_read_indexed gives for the same request.  The digest does not
        depend on how the stream is chunked.  A corrupt BODY of a chunk inside a window is not noticed: only the chunks a window cuts are decoded
        (include/snappier_hip_frame_digest.h).  result is the 4-element int64 d_result: [0] = interior rows combined, [1] = sum of dig_len over
        the OK requests, [2] = edge scratch bytes needed, [3] = requests that are OK.  Default edge_cap: a first call with 0, then a
        synchronising read of its d_result, and no second call if nothing more is needed.  A caller that passes edge_cap and work enqueues only."""
        self._bind()
        nreq, ns = req_stream.numel(), in_len.numel()
        if req_stream.dtype != torch.int32:
            raise ValueError("frame_digest_indexed: req_stream must be an int32 tensor")
        DL = N.frame_digest_lib()
        framed = self._readable(framed, nreq)
        digest = torch.empty(nreq, dtype=torch.int32, device=self.device)
        dig_len = torch.empty(nreq, dtype=torch.int64, device=self.device)
        status = torch.empty(nreq, dtype=torch.int32, device=self.device)
        result = torch.empty(4, dtype=torch.int64, device=self.device)
        start, pos = self._readable(index.start, ns), self._readable(index.pos, ns)

        def call(ec: int, w: torch.Tensor | None):
            w = self._work("frame_digest_indexed", w, DL.snp_frame_digest_indexed_workspace, nreq, ec)
            st = DL.snp_frame_digest_indexed_batch(self.ctx.handle, _p(framed), _p(in_off), _p(in_len), ns, _p(index.first), _p(start), _p(pos),
                                                   _p(index.total), _p(index.tail), index.nentries, _p(req_stream), _p(req_off), _p(req_len), nreq,
                                                   ec, _p(digest), _p(dig_len), _p(status), _p(w), _p(result))
            raise_for_status(st, self.ctx.handle)

        if edge_cap is None:
            call(0, None)
            edge_cap = result.tolist()[2]
            if edge_cap == 0:
                return digest, dig_len, status, result
        call(edge_cap, work)
        return digest, dig_len, status, result

    def frame_digest_streams(self, framed: torch.Tensor, in_off: torch.Tensor, in_len: torch.Tensor, index: "FrameIndex"):
        """The CRC-32C of everything each stream decodes to: -> (digest, dig_len, status), one per stream.  A whole stream cuts no chunk, so
        nothing is decoded (edge_cap = 0) and nothing synchronises: one header read and one multiplication per chunk."""
        ns = in_len.numel()
        req_stream = torch.arange(ns, dtype=torch.int32, device=self.device)
        req_off = torch.zeros(ns, dtype=torch.int64, device=self.device)
        req_len = torch.full((ns,), -1, dtype=torch.int64, device=self.device)
        return self.frame_digest_indexed(framed, in_off, in_len, index, req_stream, req_off, req_len, edge_cap=0)[:3]

    def frame_diff_indexed(self, a, b, req_stream_a: torch.Tensor, req_off_a: torch.Tensor, req_len_a: torch.Tensor, req_stream_b: torch.Tensor,
                           req_off_b: torch.Tensor, req_len_b: torch.Tensor, flags: int = DIFF_PREFIX | DIFF_SUFFIX, max_rows: int | None = None,
                           scratch_cap: int | None = None, work: torch.Tensor | None = None):
        """The longest common prefix and suffix of pairs of windows of what framed streams decode to (snp_frame_diff_indexed_batch,
        libsnappier_hip_frame_diff.so): -> (prefix, suffix, len_a, len_b, status, result).

        a and b are the two sides, each (framed, in_off, in_len, FrameIndex); the same tuple may be passed twice.  Request r compares the
        window [req_off_a[r], +req_len_a[r]) of stream req_stream_a[r] (int32) of side a with its counterpart on side b (int64 tensors, read as
        unsigned; offset 0 and length -1 is the whole stream).  len_a, len_b are the clipped lengths, prefix and suffix (int64) the common
        bytes at the windows' starts and ends; with both flags they never overlap, and (off = prefix, del = len_a - prefix - suffix,
        ins = b[prefix, len_b - suffix)) is a splice that turns window a into window b.  Spans between chunk boundaries both streams share are
        compared by the CRCs in their chunk headers and are not decoded: a corrupt BODY there is not noticed, and two different spans whose
        CRCs collide (2^-32 per span) are taken as equal, unless flags has DIFF_EXACT (include/snappier_hip_frame_diff.h).  result is the
        4-element int64 d_result: [0] = rows needed, [1] = sum of min(len_a, len_b) over the OK requests, [2] = scratch bytes needed,
        [3] = requests that are OK.  Default bounds: the two sizing rounds (max_rows = 0, then scratch_cap = 0), each with a synchronising read
        of d_result, then the real call unless a sizing round already was one.  A caller that passes both bounds and work enqueues only."""
        self._bind()
        nreq = req_stream_a.numel()
        if req_stream_a.dtype != torch.int32 or req_stream_b.dtype != torch.int32:
            raise ValueError("frame_diff_indexed: req_stream_a and req_stream_b must be int32 tensors")
        DL = N.frame_diff_lib()
        sides = []
        for framed, in_off, in_len, index in (a, b):
            ns = in_len.numel()
            framed = self._readable(framed, nreq)
            start, pos = self._readable(index.start, ns), self._readable(index.pos, ns)
            sides.append((framed, in_off, in_len, start, pos, index))
        prefix, suffix, len_a, len_b = (torch.empty(nreq, dtype=torch.int64, device=self.device) for _ in range(4))
        status = torch.empty(nreq, dtype=torch.int32, device=self.device)
        result = torch.empty(4, dtype=torch.int64, device=self.device)

        def call(mr: int, sc: int, w: torch.Tensor | None):
            w = self._work("frame_diff_indexed", w, DL.snp_frame_diff_indexed_workspace, nreq, mr, sc)
            args = []
            for framed, in_off, in_len, start, pos, index in sides:
                args += [_p(framed), _p(in_off), _p(in_len), in_len.numel(), _p(index.first), _p(start), _p(pos), _p(index.total), _p(index.tail),
                         index.nentries]
            st = DL.snp_frame_diff_indexed_batch(self.ctx.handle, *args, _p(req_stream_a), _p(req_off_a), _p(req_len_a), _p(req_stream_b),
                                                 _p(req_off_b), _p(req_len_b), nreq, flags, mr, sc, _p(len_a), _p(len_b), _p(prefix), _p(suffix),
                                                 _p(status), _p(w), _p(result))
            raise_for_status(st, self.ctx.handle)

        sized = False
        if max_rows is None:
            call(0, 0 if scratch_cap is None else scratch_cap, None)
            max_rows = result.tolist()[0]
            sized = max_rows == 0
        if scratch_cap is None:
            if not sized:
                call(max_rows, 0, None)
            scratch_cap = result.tolist()[2]
            sized = scratch_cap == 0
        if not sized:
            call(max_rows, scratch_cap, work)
        return prefix, suffix, len_a, len_b, status, result

    def frame_diff_streams(self, a, b, exact: bool = False):
        """Stream i of side a against stream i of side b, whole: -> (prefix, suffix, len_a, len_b, status), one per stream (the sides hold the
        same number of streams).  Stream i of a equals stream i of b iff prefix == len_a == len_b."""
        ns = a[2].numel()
        if b[2].numel() != ns:
            raise ValueError("frame_diff_streams: the two sides must hold the same number of streams")
        req_stream = torch.arange(ns, dtype=torch.int32, device=self.device)
        req_off = torch.zeros(ns, dtype=torch.int64, device=self.device)
        req_len = torch.full((ns,), -1, dtype=torch.int64, device=self.device)
        flags = DIFF_PREFIX | DIFF_SUFFIX | (DIFF_EXACT if exact else 0)
        return self.frame_diff_indexed(a, b, req_stream, req_off, req_len, req_stream, req_off, req_len, flags)[:5]

    def frame_delta_streams(self, a, b):
        """The one splice per stream that turns stream i of side a into stream i of side b: -> (off, del, ins_off, ins_len, status), int64
        tensors (status int32) -- replace bytes [off, off + del) of what a decodes to by bytes [ins_off, ins_off + ins_len) of what b decodes
        to.  Equal streams give del = ins_len = 0.  A stream whose status is not OK gives zeros.  The repair of a from b in three calls:

            off, dele, ins_off, ins_len, status = cd.frame_delta_streams(a, b)
            data_off = torch.cumsum(ins_len, 0) - ins_len
            data = torch.empty(int(ins_len.sum()), dtype=torch.uint8, device="cuda")
            cd.frame_read_indexed(*b, req_stream, ins_off, ins_len, data, data_off, ins_len)          # req_stream = arange(nstreams)
            cd.frame_splice_indexed(*a, off, dele, data, data_off, ins_len, chunk_bytes, out, out_off, out_cap, max_slots, stage_cap)
        """
        prefix, suffix, len_a, len_b, status = self.frame_diff_streams(a, b)
        return prefix, len_a - prefix - suffix, prefix.clone(), len_b - prefix - suffix, status

    def _needle_tensors(self, needles, nreq: int):
        """One needle for all requests (bytes), one per request (a list of bytes), or the three device tensors themselves
        (bytes uint8, needle_off int64, needle_len int32): -> those three tensors."""
        if isinstance(needles, tuple):
            return needles
        if isinstance(needles, (bytes, bytearray)):
            data, off, ln = bytes(needles), [0] * nreq, [len(needles)] * nreq
        else:
            if len(needles) != nreq:
                raise ValueError("frame_find_indexed: one needle per request")
            ln = [len(x) for x in needles]
            off = [0, *itertools.accumulate(ln[:-1])][:nreq]
            data = b"".join(needles)
        host = torch.frombuffer(bytearray(data or b"\0"), dtype=torch.uint8)
        return (host.to(self.device), torch.tensor(off, dtype=torch.int64).to(self.device), torch.tensor(ln, dtype=torch.int32).to(self.device))

    def frame_find_indexed(self, framed: torch.Tensor, in_off: torch.Tensor, in_len: torch.Tensor, index: "FrameIndex", req_stream: torch.Tensor,
                           req_off: torch.Tensor, req_len: torch.Tensor, needles, hit_cap, max_rows: int | None = None,
                           scratch_cap: int | None = None, work: torch.Tensor | None = None):
        """Where a byte string occurs in windows of what framed streams decode to: -> (status, win_len, count, nhits, hits, hit_off), the
        positions in hits AS OFFSETS INTO WHAT THE STREAM DECODES TO, not into the window.  frame_find_indexed_result, which says the rest,
        without the d_result."""
        return self.frame_find_indexed_result(framed, in_off, in_len, index, req_stream, req_off, req_len, needles, hit_cap, max_rows, scratch_cap,
                                              work)[:6]

    def frame_find_indexed_result(self, framed: torch.Tensor, in_off: torch.Tensor, in_len: torch.Tensor, index: "FrameIndex",
                                  req_stream: torch.Tensor, req_off: torch.Tensor, req_len: torch.Tensor, needles, hit_cap,
                                  max_rows: int | None = None, scratch_cap: int | None = None, work: torch.Tensor | None = None):
        """Where a byte string occurs in windows of what framed streams decode to (snp_frame_find_indexed_batch,
        libsnappier_hip_frame_find.so): -> (status, win_len, count, nhits, hits, hit_off, result); frame_find_indexed gives the first six.

        Request r searches the window [req_off[r], +req_len[r]) of what stream req_stream[r] (int32) decodes to (int64 tensors, read as
        unsigned; offset 0 and length -1 is the whole stream) for its needle: `needles` is one bytes for all requests, a list with one per
        request (1 to FIND_MAX_NEEDLE bytes each), or the three device tensors (bytes, needle_off int64, needle_len int32) themselves.
        hit_cap is one int for all requests or an int64 tensor; hit_off is its exclusive prefix sum.  count[r] is the number of all
        occurrences in the window, overlapping ones included; hits[hit_off[r] .. +nhits[r]) holds the first nhits[r] = min(count[r],
        hit_cap[r]) of them in ascending order.  THE POSITIONS ARE OFFSETS INTO WHAT THE STREAM DECODES TO, not into the window, so they go
        straight into req_off of frame_read_indexed and sp_off of the splice.  win_len is the clipped window's length; status is what
        frame_read_indexed gives for the same window.  A request that is not OK has win_len = count = nhits = 0.  Every chunk the window
        meets is decoded whole, into scratch inside the workspace, and verified (include/snappier_hip_frame_find.h).  result is the
        4-element int64 d_result: [0] = rows needed, [1] = sum of count over the OK requests, [2] = scratch bytes needed, [3] = requests that
        are OK.  Record boundaries, then the records:

            st, wl, count, nhits, hits, hit_off = cd.frame_find_indexed(framed, in_off, in_len, index, req_stream, req_off, req_len, b"\\n", cap)
            ends = hits[: int(nhits[0])]                       # request 0: the offset of every delimiter in its window
            starts = torch.cat([req_off[:1], ends[:-1] + 1])   # a record lies between two delimiters
            cd.frame_read_indexed(framed, in_off, in_len, index, req_stream[:1].expand(len(ends)).contiguous(), starts, ends - starts, out, ...)

        Default bounds: one sizing call (max_rows = scratch_cap = 0) and a synchronising read of its d_result, then the real call unless the
        sizing call already was one.  A caller that passes both bounds, work, an int hit_cap and needle tensors enqueues only."""
        self._bind()
        nreq, ns = req_stream.numel(), in_len.numel()
        if req_stream.dtype != torch.int32:
            raise ValueError("frame_find_indexed: req_stream must be an int32 tensor")
        FL = N.frame_find_lib()
        nd, nd_off, nd_len = self._needle_tensors(needles, nreq)
        if isinstance(hit_cap, int):
            total = nreq * hit_cap
            hit_off = torch.arange(nreq, dtype=torch.int64, device=self.device) * hit_cap
            hit_cap = torch.full((nreq,), hit_cap, dtype=torch.int64, device=self.device)
        else:
            hit_off = torch.cumsum(hit_cap, 0) - hit_cap
            total = int(hit_cap.sum().item()) if nreq else 0
        hits = torch.empty(max(total, 1), dtype=torch.int64, device=self.device)
        framed = self._readable(framed, nreq)
        start, pos = self._readable(index.start, ns), self._readable(index.pos, ns)
        win_len, count, nhits = (torch.empty(nreq, dtype=torch.int64, device=self.device) for _ in range(3))
        status = torch.empty(nreq, dtype=torch.int32, device=self.device)
        result = torch.empty(4, dtype=torch.int64, device=self.device)

        def call(mr: int, sc: int, w: torch.Tensor | None):
            w = self._work("frame_find_indexed", w, FL.snp_frame_find_indexed_workspace, nreq, mr, sc)
            st = FL.snp_frame_find_indexed_batch(self.ctx.handle, _p(framed), _p(in_off), _p(in_len), ns, _p(index.first), _p(start), _p(pos),
                                                 _p(index.total), _p(index.tail), index.nentries, _p(req_stream), _p(req_off), _p(req_len), nreq,
                                                 _p(nd), _p(nd_off), _p(nd_len), mr, sc, _p(hits), _p(hit_off), _p(hit_cap), _p(win_len), _p(count),
                                                 _p(nhits), _p(status), _p(w), _p(result))
            raise_for_status(st, self.ctx.handle)

        sized = False
        if max_rows is None or scratch_cap is None:
            call(0 if max_rows is None else max_rows, 0 if scratch_cap is None else scratch_cap, None)
            need = [v & 0xFFFFFFFFFFFFFFFF for v in result.tolist()]
            sized = need[0] == 0 and need[2] == 0
            max_rows = min(need[0], (1 << 31) - 1) if max_rows is None else max_rows
            scratch_cap = need[2] if scratch_cap is None else scratch_cap
        if not sized:
            call(max_rows, scratch_cap, work)
        return status, win_len, count, nhits, hits, hit_off, result

    def frame_find_streams(self, framed: torch.Tensor, in_off: torch.Tensor, in_len: torch.Tensor, index: "FrameIndex", needle: bytes,
                           max_hits: int | None = None, scratch_bytes: int = 256 << 20):
        """Every occurrence of `needle` in every stream, or the first max_hits per stream: -> (count, hits, status) -- count an int64 tensor
        with each stream's number of occurrences (all of them, whatever max_hits), hits a list with one int64 tensor of ascending positions
        per stream, status an int32 tensor with the first status that is not OK among a stream's windows (a stream that is not OK has count
        0 and no hits).  THE POSITIONS ARE OFFSETS INTO WHAT THE STREAM DECODES TO.

        The streams are cut into windows [k T, k T + T + m - 1), m = len(needle): an occurrence starts in [k T, k T + T) exactly when it lies
        inside that window, so the windows' hits, one after the other, are the stream's.  Windows are batched so that a call's scratch stays
        under scratch_bytes (a single window that needs more gets what it needs).  T is a multiple of 65536, so a window's first chunk is
        decoded twice only where the stream's chunks do not end on multiples of 65536 (a foreign stream, or one after a splice); its last
        chunk -- the one that holds the m - 1 bytes past k T + T -- is decoded again by the next window whenever m > 1.
        It reads idx_total and d_result back, so it is not capturable."""
        m, ns = len(needle), in_len.numel()
        if not 1 <= m <= N.FIND_MAX_NEEDLE:
            raise ValueError("frame_find_streams: the needle must have 1 to %d bytes" % N.FIND_MAX_NEEDLE)
        totals = index.total.tolist()
        T = max(65536, scratch_bytes // 2 // 65536 * 65536)
        wins = [(b, k * T, min(T + m - 1, totals[b] - k * T)) for b in range(ns) for k in range(max((max(totals[b] - m, -1) + T) // T, 1))]
        count = [0] * ns
        status = [0] * ns
        parts = [[] for _ in range(ns)]
        have = [0] * ns
        limit = (1 << 62) if max_hits is None else max_hits
        at = 0
        while at < len(wins):
            n, used = 0, 0
            while at + n < len(wins) and (n == 0 or used + wins[at + n][2] <= scratch_bytes):
                used += wins[at + n][2]
                n += 1
            while True:
                batch = wins[at:at + n]
                rs = torch.tensor([w[0] for w in batch], dtype=torch.int32).to(self.device)
                ro = torch.tensor([w[1] for w in batch], dtype=torch.int64).to(self.device)
                rl = torch.tensor([w[2] for w in batch], dtype=torch.int64).to(self.device)
                caps = [min(max(limit - have[w[0]], 0), max(1024, w[2] // 64)) for w in batch]
                cap_t = torch.tensor(caps, dtype=torch.int64).to(self.device)
                sizing = self.frame_find_indexed_result(framed, in_off, in_len, index, rs, ro, rl, needle, cap_t, 0, 0)
                need = [v & 0xFFFFFFFFFFFFFFFF for v in sizing[6].tolist()]
                if need[2] <= scratch_bytes or n == 1:
                    break
                n = max(1, min(n - 1, n * scratch_bytes // need[2]))
            st, _, cnt, nh, hits, hit_off = self.frame_find_indexed(framed, in_off, in_len, index, rs, ro, rl, needle, cap_t,
                                                                    min(need[0], (1 << 31) - 1), need[2])
            st, cnt, nh, off = st.tolist(), cnt.tolist(), nh.tolist(), hit_off.tolist()
            again = [i for i in range(n) if st[i] == 0 and nh[i] < min(cnt[i], max(limit - have[batch[i][0]], 0))]
            found = {i: hits[off[i]:off[i] + nh[i]] for i in range(n) if i not in again}
            if again:                                                   # more hits than the guess: those windows once more, with room for all
                pick = torch.tensor(again, dtype=torch.int64).to(self.device)
                cap2 = torch.tensor([min(cnt[i], max(limit - have[batch[i][0]], 0)) for i in again], dtype=torch.int64).to(self.device)
                _, _, _, nh2, hits2, off2 = self.frame_find_indexed(framed, in_off, in_len, index, rs[pick], ro[pick], rl[pick], needle, cap2)
                nh2, off2 = nh2.tolist(), off2.tolist()
                found.update({i: hits2[off2[j]:off2[j] + nh2[j]] for j, i in enumerate(again)})
            for i, (b, _, _) in enumerate(batch):
                if st[i] != 0:
                    status[b] = status[b] or st[i]
                    continue
                count[b] += cnt[i]
                take = found[i][:max(limit - have[b], 0)]
                if take.numel():
                    parts[b].append(take.clone())
                    have[b] += take.numel()
            at += n
        empty = torch.empty(0, dtype=torch.int64, device=self.device)
        hits = [empty if status[b] or not parts[b] else torch.cat(parts[b]) for b in range(ns)]
        count = [0 if status[b] else count[b] for b in range(ns)]
        return (torch.tensor(count, dtype=torch.int64).to(self.device), hits, torch.tensor(status, dtype=torch.int32).to(self.device))

    def frame_edit_indexed(self, framed: torch.Tensor, in_off: torch.Tensor, in_len: torch.Tensor, index: "FrameIndex", ed_first: torch.Tensor,
                           ed_off: torch.Tensor, ed_del: torch.Tensor, data: torch.Tensor, data_off: torch.Tensor, data_len: torch.Tensor,
                           chunk_bytes: int, out: torch.Tensor, out_off: torch.Tensor, out_cap: torch.Tensor, max_slots: int, stage_cap: int,
                           work: torch.Tensor | None = None, with_bound: bool = False):
        """A sorted EDIT SCRIPT per framed stream through its chunk index (snp_frame_edit_indexed_batch, libsnappier_hip_frame_edit.so):
        -> (out_len, status, ed_status, FrameIndex, result) and, with_bound, out_bound behind them.  The direct call: it enqueues only (it
        allocates its outputs, and the workspace when `work` is None).

        Stream b has the edits [ed_first[b], ed_first[b + 1]) (int64, nstreams + 1 values: the form hit_off has coming out of
        frame_find_indexed).  Edit e replaces bytes [ed_off[e], ed_off[e] + ed_del[e]) of what the OLD stream decodes to by
        data[data_off[e] .. +data_len[e]) (int64 tensors, read as unsigned); the edits of a stream are ascending and disjoint, all in the old
        stream's coordinates, and one with ed_del = data_len = 0 is skipped.  Each touched chunk is decoded once, each rewritten region
        compressed once in pieces of chunk_bytes, every other kept byte copied once, and a stream is edited whole or not at all
        (out_len[b] = 0 then: include/snappier_hip_frame_edit.h).  ed_status is each edit's own verdict (int32).  The outputs, the returned
        FrameIndex (start / pos hold index.nentries + max_slots rows), result and the sizing call (max_slots = stage_cap = 0) are those of
        frame_splice_indexed."""
        if not 1 <= chunk_bytes <= N.BLOCK_SIZE:
            raise ValueError(f"frame_edit_indexed: chunk_bytes = {chunk_bytes}, must be 1 .. {N.BLOCK_SIZE}")
        self._bind()
        ns, nedits = in_len.numel(), ed_off.numel()
        if ed_first.numel() != ns + 1:
            raise ValueError(f"frame_edit_indexed: ed_first holds {ed_first.numel()} values, {ns} streams need {ns + 1}")
        EL = N.frame_edit_lib()
        framed, out, data = self._readable(framed, ns), self._readable(out, ns), self._readable(data, ns)
        ne = index.nentries
        start, pos = self._readable(index.start, ns), self._readable(index.pos, ns)
        out_len = torch.zeros(ns, dtype=torch.int64, device=self.device)
        status = torch.zeros(ns, dtype=torch.int32, device=self.device)
        ed_status = torch.zeros(nedits, dtype=torch.int32, device=self.device)
        first = torch.zeros(ns + 1, dtype=torch.int64, device=self.device)
        rows = ne + max_slots
        new_start = torch.empty(max(rows, 1), dtype=torch.int64, device=self.device)
        new_pos = torch.empty(max(rows, 1), dtype=torch.int64, device=self.device)
        total = torch.empty(ns, dtype=torch.int64, device=self.device)
        tail = torch.empty(ns, dtype=torch.int32, device=self.device)
        bound = torch.zeros(ns, dtype=torch.int64, device=self.device) if with_bound else None
        result = torch.empty(4, dtype=torch.int64, device=self.device)
        w = self._work("frame_edit_indexed", work, EL.snp_frame_edit_indexed_workspace, ns, nedits, max_slots, stage_cap, chunk_bytes)
        st = EL.snp_frame_edit_indexed_batch(self.ctx.handle, _p(framed), _p(in_off), _p(in_len), ns, _p(index.first), _p(start), _p(pos),
                                             _p(index.total), _p(index.tail), ne, _p(data), _p(ed_first), _p(ed_off), _p(ed_del), _p(data_len),
                                             _p(data_off), nedits, chunk_bytes, max_slots, stage_cap, _p(out), _p(out_off), _p(out_cap),
                                             _p(out_len), _p(status), _p(ed_status), _p(first), _p(new_start), _p(new_pos), _p(total), _p(tail),
                                             _p(bound), _p(w), _p(result))
        raise_for_status(st, self.ctx.handle)
        got = (out_len, status, ed_status, FrameIndex(first, new_start[:rows], new_pos[:rows], total, tail, result), result)
        return got + (bound,) if with_bound else got

    def frame_edit_to_memory(self, framed: torch.Tensor, in_off: torch.Tensor, in_len: torch.Tensor, index: "FrameIndex", ed_first: torch.Tensor,
                             ed_off: torch.Tensor, ed_del: torch.Tensor, data: torch.Tensor, data_off: torch.Tensor, data_len: torch.Tensor,
                             chunk_bytes: int = N.BLOCK_SIZE, align: int = 1, max_bytes: int | None = None):
        """Edit framed streams given the framed tensor, its table, its index and an edit script per stream:
        -> (out, out_off, out_len, status, ed_status, FrameIndex).

        ONE sizing call (max_slots = stage_cap = 0, every out_cap 0) that also asks for each named stream's size bound, ONE synchronising read
        of its result and of the arena size (ValueError if that is above max_bytes), an arena in which stream b's slot is its bound rounded up
        to `align` (0 for a stream that is left alone or refused), then the edit.  Streams with out_len 0 are not in the arena: the caller
        keeps their old bytes, and the returned index holds their old rows."""
        ns = in_len.numel()
        zero = torch.zeros(ns, dtype=torch.int64, device=self.device)
        empty = torch.empty(0, dtype=torch.uint8, device=self.device)
        _, _, _, _, result, bound = self.frame_edit_indexed(framed, in_off, in_len, index, ed_first, ed_off, ed_del, data, data_off, data_len,
                                                            chunk_bytes, empty, zero, zero, 0, 0, with_bound=True)
        slot = (bound + (align - 1)) // align * align
        ends = torch.cumsum(slot, 0)
        out_off = ends - slot
        need = torch.cat([result, ends[-1:] if ns else zero[:0].new_zeros(1)]).tolist()
        if need[0] > 0xFFFFFFFF:
            raise ValueError(f"frame_edit_to_memory: {need[0]} chunk slots, one call takes 2^32 - 1")
        if max_bytes is not None and need[-1] > max_bytes:
            raise ValueError(f"frame_edit_to_memory: the new streams take up to {need[-1]} bytes, max_bytes = {max_bytes}")
        out = torch.empty(max(need[-1], 1), dtype=torch.uint8, device=self.device)
        out_len, status, ed_status, new_index, _ = self.frame_edit_indexed(framed, in_off, in_len, index, ed_first, ed_off, ed_del, data, data_off,
                                                                           data_len, chunk_bytes, out, out_off, bound, need[0], need[2])
        return out[:need[-1]], out_off, out_len, status, ed_status, new_index

    def frame_replace_streams(self, framed: torch.Tensor, in_off: torch.Tensor, in_len: torch.Tensor, index: "FrameIndex", needle: bytes,
                              replacement: bytes, chunk_bytes: int = N.BLOCK_SIZE):
        """Every occurrence of `needle` in every stream replaced by `replacement`: -> (out, out_off, out_len, status, FrameIndex, count); a
        written stream decodes to bytes.replace(needle, replacement) of what it decoded to, and count is each stream's number of
        replacements.  frame_find_streams, then ONE frame_edit_to_memory with one edit per kept hit.

        The find reports overlapping occurrences; bytes.replace takes the leftmost one and goes on behind it.  A needle without a proper
        border (no prefix that is also a suffix) cannot overlap itself, and every hit is kept.  Otherwise the kept hits are those reached
        from a stream's first hit by `the first hit at or behind this one's end`, found by pointer doubling over torch.searchsorted on the
        device, not by a host loop over the hits.  A stream without a hit, and one whose find is not OK (its status is returned), is left
        alone: out_len 0, its old rows in the index.  It reads results back between its steps, so it is not capturable."""
        m, ns = len(needle), in_len.numel()
        count, hits, fstatus = self.frame_find_streams(framed, in_off, in_len, index, needle)
        counts = torch.tensor([h.numel() for h in hits], dtype=torch.int64).to(self.device)
        ed_off = torch.cat(hits) if ns else counts.new_zeros(0)
        if any(needle[:k] == needle[m - k:] for k in range(1, m)):
            ed_off, counts = self._leftmost_disjoint(ed_off, counts, index.total, m)
        ed_first = torch.cat([counts.new_zeros(1), torch.cumsum(counts, 0)])
        nedits = ed_off.numel()
        ed_del = torch.full((nedits,), m, dtype=torch.int64, device=self.device)
        data = torch.frombuffer(bytearray(replacement), dtype=torch.uint8).to(self.device) if replacement else torch.empty(0, dtype=torch.uint8, device=self.device)
        data_off = torch.zeros(nedits, dtype=torch.int64, device=self.device)
        data_len = torch.full((nedits,), len(replacement), dtype=torch.int64, device=self.device)
        out, out_off, out_len, status, _, new_index = self.frame_edit_to_memory(framed, in_off, in_len, index, ed_first, ed_off, ed_del, data,
                                                                                 data_off, data_len, chunk_bytes)
        return out, out_off, out_len, torch.where(fstatus != 0, fstatus, status), new_index, counts

    @staticmethod
    def _leftmost_disjoint(hits: torch.Tensor, counts: torch.Tensor, total: torch.Tensor, m: int):
        """Of the ascending positions of all occurrences of an m-byte needle -- `hits`, the streams' one behind the other, counts[b] of stream b,
        which decodes to total[b] bytes -- the ones bytes.replace takes: a stream's first, then always the first at or behind the end of the
        one before.  -> (the kept hits, their count per stream).  ONE pointer doubling for the whole batch: every hit points at the first hit of
        its stream at or behind its end (one searchsorted over keys that set the streams apart), the end of a stream at a sentinel that points
        at itself; log2(the most hits a stream has) rounds of `mark what the marked ones point at; point twice as far`."""
        n = hits.numel()
        if n < 2:
            return hits, counts
        span = total + (m + 1)                                          # stream b's keys lie in [base[b], base[b] + total[b]]: apart by more than m
        keys = hits + torch.repeat_interleave(torch.cumsum(span, 0) - span, counts)
        last = torch.cumsum(counts, 0)
        ends = torch.repeat_interleave(last, counts)                    # where the hits of a hit's own stream end
        jump = torch.searchsorted(keys, keys + m)
        jump = torch.cat([torch.where(jump >= ends, jump.new_full((1,), n), jump), jump.new_full((1,), n)])
        kept = torch.zeros(n + 1, dtype=torch.bool, device=hits.device)
        kept[(last - counts)[counts > 0]] = True                        # every stream's first hit
        for _ in range(int(counts.max().item()).bit_length()):
            kept[jump[kept]] = True
            jump = jump[jump]
        kept = kept[:n]
        before = torch.cat([last.new_zeros(1), torch.cumsum(kept, 0)])
        return hits[kept], before[last] - before[last - counts]

    def frame_decode_chunks(self, framed: torch.Tensor, chunk_type, body_off, body_len, chunk_crc, out, out_off, out_cap):
        self._bind()
        nc = body_len.numel()
        out_len = torch.empty(nc, dtype=torch.int32, device=self.device)
        status = torch.empty(nc, dtype=torch.int32, device=self.device)
        st = self.ctx.lib.snp_frame_decode_chunks_device(self.ctx.handle, _p(framed), _p(chunk_type), _p(body_off),
                                                    _p(body_len), _p(chunk_crc), nc, _p(out), _p(out_off), _p(out_cap),
                                                    _p(out_len), _p(status))
        raise_for_status(st, self.ctx.handle)
        return out_len, status

    def frame_decode(self, framed: torch.Tensor, nbytes: int, out: torch.Tensor, max_chunks: int, work: torch.Tensor | None = None):
        """Framed stream without a chunk table, all on the device (snp_frame_decode_device): -> 2-element int64 tensor
        (bytes written, status).  The chunk headers are walked by a device kernel (serial, ~1 us per chunk)."""
        self._bind()
        need = N.lib().snp_frame_decode_workspace(max_chunks)
        if work is None:
            work = torch.empty(need, dtype=torch.uint8, device=self.device)
        if work.numel() < need:
            raise ValueError("frame_decode: work buffer too small")
        result = torch.zeros(2, dtype=torch.int64, device=self.device)
        st = self.ctx.lib.snp_frame_decode_device(self.ctx.handle, _p(framed), nbytes, _p(out), out.numel(), max_chunks, _p(work), _p(result))
        raise_for_status(st, self.ctx.handle)
        return result


class FrameIndex:
    """The chunk index of a batch of framed streams (BlockCodec.frame_index_buffers; include/snappier_hip_frame_index.h): five device tensors --
    first (int64, nstreams + 1), start and pos (int64, one per row), total (int64) and tail (int32) per stream -- and the d_result of the call
    that built it.  It names no address: it is valid for the same streams wherever they lie, and may be stored and loaded again."""

    def __init__(self, first: torch.Tensor, start: torch.Tensor, pos: torch.Tensor, total: torch.Tensor, tail: torch.Tensor,
                 result: torch.Tensor | None = None):
        self.first, self.start, self.pos, self.total, self.tail, self.result = first, start, pos, total, tail, result

    @property
    def nentries(self) -> int:
        """Rows the start / pos tensors hold."""
        return min(self.start.numel(), self.pos.numel())


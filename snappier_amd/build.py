"""Builds the gfx950 native libraries in-tree with hipcc (cross-compiles without a GPU).

    python snappier_amd/build.py            # libsnappier_hip.so, libsnappier_hip_buffers.so, libsnappier_hip_buffers_decompress.so,
                                            # libsnappier_hip_frame_buffers.so, libsnappier_hip_layout.so, libsnappier_hip_frame_range.so,
                                            # libsnappier_hip_frame_index.so, libsnappier_hip_frame_chunked.so, libsnappier_hip_frame_update.so,
                                            # libsnappier_hip_frame_append.so, libsnappier_hip_frame_splice.so, libsnappier_hip_frame_rechunk.so,
                                            # libsnappier_hip_frame_compose.so, libsnappier_hip_frame_digest.so,
                                            # libsnappier_hip_frame_diff.so, libsnappier_hip_frame_find.so,
                                            # libsnappier_hip_frame_edit.so, libsnappier_hip_frame_cuts.so,
                                            # libsnappier_hip_frame_dedup.so, libsnappier_hip_frame_recut.so,
                                            # libsnappier_hip_frame_verify.so
                                            # (+ libsnappier_datagen.so, bench/test helper)
"""
from __future__ import annotations

import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared", "-fconstexpr-steps=100000000", "-Wall", "-Wno-sometimes-uninitialized",
         "-Wno-unused-function", "-Wl,-rpath,/opt/rocm/lib"]

LIBS = {
    "libsnappier_hip.so": ["decode_chains.hip", "decompress.hip", "decompress_small.hip", "tag_index.hip", "compress_lanes.hip", "compress_win.hip", "crc32c.hip", "framing.hip", "frame_scan.hip",
                           "capi_ctx.hip", "capi_pool.hip", "capi_batch.hip", "capi_host.hip", "capi_frame.hip"],
    # include/snappier_hip_buffers.h: buffers of any length, one block each -- an extension linked against the product library (its contexts)
    "libsnappier_hip_buffers.so": ["buffers.hip"],
    # include/snappier_hip_buffers_decompress.h: device batch decompress that splits large blocks across wavefronts -- the same kind of extension
    "libsnappier_hip_buffers_decompress.so": ["buffers_decode.hip"],
    # include/snappier_hip_frame_buffers.h: device batch encode / decode of many framed streams -- the same kind of extension
    "libsnappier_hip_frame_buffers.so": ["frame_buffers.hip"],
    # include/snappier_hip_layout.h: device batch decoded-length query and output layout for the decode calls -- the same kind of extension
    "libsnappier_hip_layout.so": ["layout.hip"],
    # include/snappier_hip_frame_range.h: device batch range decode of framed streams (a window of every stream) -- the same kind of extension
    "libsnappier_hip_frame_range.so": ["frame_range.hip"],
    # include/snappier_hip_frame_index.h: device seek index for framed streams and indexed window reads -- the same kind of extension
    "libsnappier_hip_frame_index.so": ["frame_index.hip"],
    # include/snappier_hip_frame_chunked.h: device batch frame encode with a chosen chunk size and its seek index -- the same kind of extension
    "libsnappier_hip_frame_chunked.so": ["frame_chunked.hip"],
    # include/snappier_hip_frame_update.h: device batch update of seekable framed streams through their index -- the same kind of extension
    "libsnappier_hip_frame_update.so": ["frame_update.hip"],
    # include/snappier_hip_frame_append.h: device batch append to seekable framed streams, in place, with the new index -- the same kind of extension
    "libsnappier_hip_frame_append.so": ["frame_append.hip"],
    # include/snappier_hip_frame_splice.h: device batch splice (insert, delete, truncate) of seekable framed streams, with the new index -- the same kind of extension
    "libsnappier_hip_frame_splice.so": ["frame_splice.hip"],
    # include/snappier_hip_frame_rechunk.h: device batch rechunk of seekable framed streams to canonical form, with the new index -- the same kind of extension
    "libsnappier_hip_frame_rechunk.so": ["frame_rechunk.hip"],
    # include/snappier_hip_frame_compose.h: device batch compose of new seekable framed streams from windows of old ones, with the new index -- the same kind of extension
    "libsnappier_hip_frame_compose.so": ["frame_compose.hip"],
    # include/snappier_hip_frame_digest.h: device batch digest (CRC-32C of decoded windows) of seekable framed streams from their chunk headers, no decode -- the same kind of extension
    "libsnappier_hip_frame_digest.so": ["frame_digest.hip"],
    # include/snappier_hip_frame_diff.h: device batch diff (common prefix and suffix of decoded windows) of seekable framed streams, header CRCs between common chunk boundaries -- the same kind of extension
    "libsnappier_hip_frame_diff.so": ["frame_diff.hip"],
    # include/snappier_hip_frame_find.h: device batch find (where a byte string occurs in decoded windows) of seekable framed streams, the windows' chunks decoded into scratch -- the same kind of extension
    "libsnappier_hip_frame_find.so": ["frame_find.hip"],
    # include/snappier_hip_frame_edit.h: device batch edit (a sorted edit script per stream: many splices in one call) of seekable framed streams, with the new index -- the same kind of extension
    "libsnappier_hip_frame_edit.so": ["frame_edit.hip"],
    # include/snappier_hip_frame_cuts.h: device content-defined chunking -- the cuts the bytes of every buffer define, and the chunked frame encode with the pieces given by the caller -- the same kind of extension
    "libsnappier_hip_frame_cuts.so": ["frame_cuts.hip"],
    # include/snappier_hip_frame_dedup.h: device batch dedup of seekable framed streams by chunk -- the unique chunks of the new streams once, as a pack with its index, and the compose recipes that rebuild every stream -- the same kind of extension
    "libsnappier_hip_frame_dedup.so": ["frame_dedup.hip"],
    # include/snappier_hip_frame_recut.h: device batch recut of seekable framed streams to a caller's cut list -- the chunks that already are pieces copied, the others decoded and compressed again, with the new index -- the same kind of extension
    "libsnappier_hip_frame_recut.so": ["frame_recut.hip"],
    # include/snappier_hip_frame_verify.h: device batch verify of seekable framed streams chunk by chunk in bounded scratch -- a verdict per index row, nothing written but verdicts -- and the planner that turns the verdicts into compose recipes over a replica -- the same kind of extension
    "libsnappier_hip_frame_verify.so": ["frame_verify.hip"],
    "libsnappier_datagen.so": ["datagen.hip"],
}
# every library but the product and the data generator is an extension, linked against the product (LIBS keeps its order: the product is built first)
LINK = {lib: ["-L" + HERE, "-lsnappier_hip", "-Wl,-rpath,$ORIGIN"] for lib in LIBS if lib not in ("libsnappier_hip.so", "libsnappier_datagen.so")}


def _stale(target: str, sources: list[str]) -> bool:
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    inc = os.path.join(HERE, "..", "include")
    deps = sources + [os.path.join(d, f) for d in (CSRC, inc) for f in os.listdir(d) if f.endswith(".h")]   # every header either directory holds
    return any(os.path.getmtime(s) > t for s in deps)


def build_native(force: bool = False, verbose: bool = False) -> list[str]:
    """Compile every HIP library for gfx950; returns the paths of the built .so files."""
    built = []
    for lib, srcs in LIBS.items():
        target = os.path.join(HERE, lib)
        sources = [os.path.join(CSRC, s) for s in srcs]
        if force or _stale(target, sources):
            cmd = [HIPCC] + FLAGS + sources + ["-o", target] + LINK.get(lib, [])
            if verbose:
                print(" ".join(cmd), file=sys.stderr)
            subprocess.run(cmd, check=True)
        built.append(target)
    return built


if __name__ == "__main__":
    for p in build_native(force="--force" in sys.argv, verbose=True):
        print(p)

"""ctypes binding of libsnappier_hip.so -- the C-ABI declared in include/snappier_hip.h.

The library is the product: if it is missing or a symbol is absent this module raises, there is no fallback.
torch is imported first on purpose: torch bundles its own libamdhip64.so.7; loading it before our library makes
the dynamic loader resolve our DT_NEEDED libamdhip64.so.7 to that same object, so torch tensors and our kernels
share one HIP runtime (one context, one set of streams).
"""
from __future__ import annotations

import ctypes as C
import os
import re

import torch  # noqa: F401  (must precede CDLL -- see module docstring)

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("SNAPPIER_HIP_LIB") or os.path.join(HERE, "libsnappier_hip.so")   # override: kernel-variant A/B runs (scripts/build_variant.sh)
HEADER_PATH = os.path.join(HERE, "..", "include", "snappier_hip.h")

(OK, ERR_OUTPUT_TOO_SMALL, ERR_BAD_OFFSET, ERR_TOO_LONG, ERR_INCOMPLETE, ERR_BAD_LENGTH, ERR_CRC_MISMATCH,
 ERR_CHUNK_TYPE, ERR_OVERLAP, ERR_BAD_ARG, ERR_DEVICE, ERR_TRUNCATED_STREAM) = range(12)
HASH_CRC32C, HASH_MUL = 0, 1
BLOCK_SIZE = 65536
MAX_BLOCK_COMPRESSED = 76491
RECHUNK_REWRITE_ALL = 1                  # SNP_RECHUNK_REWRITE_ALL (include/snappier_hip_frame_rechunk.h)
DIFF_PREFIX, DIFF_SUFFIX, DIFF_EXACT = 1, 2, 4   # SNP_DIFF_PREFIX, SNP_DIFF_SUFFIX, SNP_DIFF_EXACT (include/snappier_hip_frame_diff.h)
FIND_MAX_NEEDLE = 256    # SNP_FIND_MAX_NEEDLE (include/snappier_hip_frame_find.h)
FIND_TILE = 16384        # kFindTile (csrc/frame_find_device.h): the start positions one workgroup step of the find takes
CUTS_MIN_WINDOW, CUTS_MAX_WINDOW = 32, 32767   # SNP_CUTS_MIN_WINDOW, SNP_CUTS_MAX_WINDOW (include/snappier_hip_frame_cuts.h)
CUTS_TILE = 4096         # kCutsTile (csrc/frame_cuts_device.h): the positions one workgroup of the cut finder takes at a time -- its seam
CUTS_BLOCK = 64          # kCutsBlock: the positions one stored hash maximum covers
CUTS_RUN = 17            # kCutsRun: the positions one lane hashes in a row
RECUT_REWRITE_ALL = 1                    # SNP_RECUT_REWRITE_ALL (include/snappier_hip_frame_recut.h)
VERIFY_NONE = (1 << 64) - 1  # SNP_VERIFY_NONE (include/snappier_hip_frame_verify.h): first_bad of a stream with no bad row (-1 in an int64 tensor)
VERIFY_SKIPPED = -1          # SNP_VERIFY_SKIPPED: row_status of a row that was not looked at
DEDUP_NONE = (1 << 64) - 1   # SNP_DEDUP_NONE (include/snappier_hip_frame_dedup.h): canon of a row that takes no part (-1 in an int64 tensor)
# snp_option (include/snappier_hip.h)
(OPT_DECODE_LAYOUT, OPT_SMALL_BLOCK_MAX, OPT_SMALL_BLOCK_MIN_BATCH, OPT_COMPRESS_LAYOUT, OPT_COMPRESS_WINDOW_MAX_BATCH,
 OPT_TABLE_PROBE_TRIES, OPT_TABLE_PROBE_MAX_BYTES, OPT_PARALLEL_DECODE_MIN, OPT_FENCED, OPT_DECODE_LEFTOVERS, OPT_CRC_KERNEL,
 OPT_COMPRESS_WINDOW_POSITIONS, OPT_COMPRESS_WINDOW_GLOBAL_MIN_BATCH, OPT_COMPRESS_LANE_STORES, OPT_COMPRESS_LANE_PROBES,
 OPT_COMPRESS_LANES_PER_WAVEFRONT, OPT_COMPRESS_SLICE, OPT_COMPRESS_SMALL_INPUT_LDS, OPT_COMPRESS_SMALL_INPUT_LANES, OPT_FRAME_SCAN,
 OPT_DECODE_LDS_THROTTLE, OPT_COMPRESS_WINDOW_GLOBAL_SLOTS, OPT_COMPRESS_WINDOW_DUAL_MIN_BATCH) = range(1, 24)
OPT_CRC_TABLE_FREE = OPT_CRC_KERNEL     # deprecated name (rounds 1-4), same number
# SNP_OPT_DECODE_LAYOUT / SNP_OPT_COMPRESS_LAYOUT values
DECODE_AUTO, DECODE_WAVE_ONLY, DECODE_SMALL_LANES, DECODE_SMALL_TEAM4, DECODE_SMALL_TEAM8, DECODE_SMALL_TEAM16, DECODE_SERIAL = range(7)
COMPRESS_AUTO, COMPRESS_LANES, COMPRESS_WINDOW_LDS, COMPRESS_WINDOW_GLOBAL, COMPRESS_WINDOW_DUAL = 0, 2, 3, 4, 5


def declared_symbols(header: str = HEADER_PATH) -> list[str]:
    """Every function name declared in a C header (default: include/snappier_hip.h)."""
    with open(header) as f:
        text = f.read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(snp_[a-z0-9_]+)\s*\(", text)))


_lib = None
_lab = None
LAB_PATH = os.path.join(HERE, "variants", "libsnappier_hip_lab.so")


def lab_requested() -> bool:
    """SNAPPIER_HIP_LAB=1: the explicit opt-in of the A/B scripts (scripts/) to the LAB library -- the product sources built with
    -DSNAPPIER_HIP_DEBUG_ENV plus the round-4 decoder front ends of scripts/lab/, the only build in which the SNAPPIER_HIP_* knobs act."""
    return os.environ.get("SNAPPIER_HIP_LAB", "") == "1"


def lab_path() -> str:
    """snappier_amd/variants/libsnappier_hip_lab.so -- built by `LAB=1 bash scripts/build_variant.sh lab`, never implicitly (no compiler runs at import)."""
    if not os.path.exists(LAB_PATH):
        raise ImportError(f"{LAB_PATH} is missing: SNAPPIER_HIP_LAB=1 asks for the lab library; build it with `LAB=1 bash scripts/build_variant.sh lab`")
    return LAB_PATH


def lib() -> C.CDLL:
    """The product library (libsnappier_hip.so, or the file SNAPPIER_HIP_LIB names).  It reads no environment: kernels and layouts are chosen per
    context through snp_ctx_set_option (Context.set_option).  Only with SNAPPIER_HIP_LAB=1 -- the A/B scripts -- is the LAB library loaded
    instead; a stray SNAPPIER_HIP_* variable without it is ignored, with a warning.  A Context remembers the library it was created from."""
    global _lib, _lab
    if not os.environ.get("SNAPPIER_HIP_LIB") and lab_requested():
        if _lab is None:
            _lab = _load(lab_path())
        return _lab
    if _lib is None:
        stray = sorted(k for k in os.environ if k.startswith("SNAPPIER_HIP_") and k not in ("SNAPPIER_HIP_LIB", "SNAPPIER_HIP_LAB"))
        if stray and not os.environ.get("SNAPPIER_HIP_LIB"):
            import warnings
            warnings.warn(f"{', '.join(stray)} ignored: libsnappier_hip.so reads no environment (use Context.set_option, or SNAPPIER_HIP_LAB=1 for the lab build)")
        _lib = _load(LIB_PATH)
    return _lib


def _load(path: str) -> C.CDLL:
    LIB_PATH = path
    if not os.path.exists(LIB_PATH):
        raise ImportError(f"{LIB_PATH} is missing: build it with `python snappier_amd/build.py` "
                          "(there is no CPU fallback for the codec)")
    L = C.CDLL(LIB_PATH)
    # every symbol the header declares must be exported; an installed copy without the repo's include/ directory
    # falls back to the signatures bound below (a missing one still raises AttributeError there)
    missing = [s for s in declared_symbols() if not hasattr(L, s)] if os.path.exists(HEADER_PATH) else []
    if missing:
        raise ImportError(f"libsnappier_hip.so does not export: {missing}")
    vp, sz, u32, u64, i32, i64 = C.c_void_p, C.c_size_t, C.c_uint32, C.c_uint64, C.c_int, C.c_int64
    szp = C.POINTER(sz)
    sig = {
        "snp_ctx_create": (i32, [i32, i32, vp, C.POINTER(vp)]),
        "snp_ctx_destroy": (None, [vp]),
        "snp_ctx_set_stream": (i32, [vp, vp]),
        "snp_ctx_last_error": (C.c_char_p, [vp]),
        "snp_ctx_synchronize": (i32, [vp]),
        "snp_ctx_counter": (u64, [vp, i32]),
        "snp_ctx_set_option": (i32, [vp, i32, i64]),
        "snp_ctx_get_option": (i32, [vp, i32, C.POINTER(i64)]),
        "snp_ctx_reserve_compress": (i32, [vp, u32]),
        "snp_status_string": (C.c_char_p, [i32]),
        "snp_version": (C.c_char_p, []),
        "snp_max_compressed_length": (i64, [i64]),
        "snp_max_fragment_compressed_length": (i64, [i64]),
        "snp_get_uncompressed_length": (i32, [vp, sz, C.POINTER(u32), C.POINTER(u32)]),
        "snp_try_compress": (i32, [vp, vp, sz, vp, sz, szp]),
        "snp_try_decompress": (i32, [vp, vp, sz, vp, sz, szp]),
        "snp_try_compress_segments": (i32, [vp, C.POINTER(vp), szp, u32, vp, sz, szp]),
        "snp_try_decompress_segments": (i32, [vp, C.POINTER(vp), szp, u32, vp, sz, szp]),
        "snp_crc32c": (i32, [vp, vp, sz, i32, C.POINTER(u32)]),
        "snp_frame_max_encoded_length": (i64, [i64]),
        "snp_frame_encode": (i32, [vp, vp, sz, vp, sz, szp]),
        "snp_frame_decoded_length": (i32, [vp, sz, C.POINTER(u64)]),
        "snp_frame_decode": (i32, [vp, vp, sz, vp, sz, szp]),
        "snp_compress_batch": (i32, [vp, vp, vp, vp, u32, vp, vp, vp, vp]),
        "snp_decompress_batch": (i32, [vp, vp, vp, vp, u32, vp, vp, vp, vp, vp]),
        "snp_crc32c_batch": (i32, [vp, vp, vp, vp, u32, i32, vp]),
        "snp_concat_batch": (i32, [vp, vp, vp, vp, u32, vp, vp]),
        "snp_frame_encode_workspace": (u64, [u64]),
        "snp_frame_encode_device": (i32, [vp, vp, u64, vp, u64, vp, vp]),
        "snp_frame_decode_chunks_device": (i32, [vp, vp, vp, vp, vp, vp, u32, vp, vp, vp, vp, vp]),
        "snp_frame_decode_workspace": (u64, [u32]),
        "snp_frame_decode_device": (i32, [vp, vp, u64, vp, u64, u32, vp, vp]),
    }
    for name, (res, args) in sig.items():
        fn = getattr(L, name)
        fn.restype = res
        fn.argtypes = args
    return L


PRODUCT_PATH = os.path.join(HERE, "libsnappier_hip.so")
_vp, _u32, _u64, _i32 = C.c_void_p, C.c_uint32, C.c_uint64, C.c_int
# The batch extension libraries: name -> (library file, header under include/, {function: (restype, argtypes)}).  Each is linked against the
# PRODUCT library and takes its contexts, so it is available only when lib() is the product library (not a variant under SNAPPIER_HIP_LIB, nor
# the lab build).
_EXTENSIONS = {
    # buffers of any length, one block each
    "buffers": ("libsnappier_hip_buffers.so", "snappier_hip_buffers.h", {
        "snp_compress_buffers_workspace": (_u64, [_u32, _u32]),
        "snp_compress_buffers_batch": (_i32, [_vp, _vp, _vp, _vp, _u32, _u32, _vp, _vp, _vp, _vp, _vp, _vp, _vp])}),
    # device batch decompress that splits large blocks across wavefronts
    "buffers_decompress": ("libsnappier_hip_buffers_decompress.so", "snappier_hip_buffers_decompress.h", {
        "snp_decompress_buffers_workspace": (_u64, [_u32, _u32]),
        "snp_decompress_buffers_batch": (_i32, [_vp, _vp, _vp, _vp, _u32, _u32, _vp, _vp, _vp, _vp, _vp, _vp, _vp])}),
    # device batch encode and decode of many framed streams
    "frame_buffers": ("libsnappier_hip_frame_buffers.so", "snappier_hip_frame_buffers.h", {
        "snp_frame_encode_buffers_workspace": (_u64, [_u32, _u32]),
        "snp_frame_encode_buffers_batch": (_i32, [_vp, _vp, _vp, _vp, _u32, _u32, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
        "snp_frame_decode_buffers_workspace": (_u64, [_u32, _u32, _u32]),
        "snp_frame_decode_buffers_batch": (_i32, [_vp, _vp, _vp, _vp, _u32, _u32, _u32, _vp, _vp, _vp, _vp, _vp, _vp, _vp])}),
    # device batch decoded-length query and output layout for the decode calls
    "layout": ("libsnappier_hip_layout.so", "snappier_hip_layout.h", {
        "snp_decompress_layout_workspace": (_u64, [_u32]),
        "snp_decompress_layout_batch": (_i32, [_vp, _vp, _vp, _vp, _u32, _u32, _u64, _vp, _vp, _vp, _vp, _vp, _vp]),
        "snp_frame_decode_layout_workspace": (_u64, [_u32, _u32]),
        "snp_frame_decode_layout_batch": (_i32, [_vp, _vp, _vp, _vp, _u32, _u32, _u32, _u64, _vp, _vp, _vp, _vp, _vp, _vp, _vp])}),
    # device batch range decode of framed streams: a window of every stream
    "frame_range": ("libsnappier_hip_frame_range.so", "snappier_hip_frame_range.h", {
        "snp_frame_decode_range_workspace": (_u64, [_u32, _u32, _u32, _u64]),
        "snp_frame_decode_range_batch": (_i32, [_vp, _vp, _vp, _vp, _u32, _vp, _vp, _u32, _u32, _u64, _vp, _vp, _vp, _vp, _vp, _vp, _vp])}),
    # device seek index for framed streams and indexed window reads: any number of windows, each naming a stream, with no header walk
    "frame_index": ("libsnappier_hip_frame_index.so", "snappier_hip_frame_index.h", {
        "snp_frame_index_workspace": (_u64, [_u32, _u32]),
        "snp_frame_index_batch": (_i32, [_vp, _vp, _vp, _vp, _u32, _u32, _u64, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
        "snp_frame_read_indexed_workspace": (_u64, [_u32, _u32, _u64]),
        "snp_frame_read_indexed_batch": (_i32, [_vp, _vp, _vp, _vp, _u32, _vp, _vp, _vp, _vp, _vp, _u64, _vp, _vp, _vp, _u32, _u32, _u64,
                                                _vp, _vp, _vp, _vp, _vp, _vp, _vp])}),
    # device batch frame encode with a chosen chunk size, and the seek index of what it wrote
    "frame_chunked": ("libsnappier_hip_frame_chunked.so", "snappier_hip_frame_chunked.h", {
        "snp_frame_encode_chunked_workspace": (_u64, [_u32, _u32, _u32]),
        "snp_frame_encode_chunked_batch": (_i32, [_vp, _vp, _vp, _vp, _u32, _u32, _u32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp])}),
    # device batch update of seekable framed streams through their index: only the chunks the requests touch are compressed again
    "frame_update": ("libsnappier_hip_frame_update.so", "snappier_hip_frame_update.h", {
        "snp_frame_write_indexed_workspace": (_u64, [_u32, _u32, _u32, _u64]),
        "snp_frame_write_indexed_batch": (_i32, [_vp, _vp, _vp, _vp, _u32, _vp, _vp, _vp, _vp, _vp, _u64, _vp, _vp, _vp, _vp, _vp, _u32, _u32, _u64,
                                                 _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp])}),
    # device batch append to seekable framed streams, in place: the tail chunk reopened, fresh chunks behind it, the new index
    "frame_append": ("libsnappier_hip_frame_append.so", "snappier_hip_frame_append.h", {
        "snp_frame_append_indexed_workspace": (_u64, [_u32, _u32, _u32, _u32]),
        "snp_frame_append_indexed_batch": (_i32, [_vp, _vp, _vp, _vp, _vp, _u32, _vp, _vp, _vp, _vp, _vp, _u64, _vp, _vp, _vp, _u32, _u32, _u32,
                                                  _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp])}),
    # device batch splice of seekable framed streams: one insert / delete / truncate per stream, the chunks around the hole compressed again, the new index
    "frame_splice": ("libsnappier_hip_frame_splice.so", "snappier_hip_frame_splice.h", {
        "snp_frame_splice_indexed_workspace": (_u64, [_u32, _u32, _u64, _u32]),
        "snp_frame_splice_indexed_batch": (_i32, [_vp, _vp, _vp, _vp, _u32, _vp, _vp, _vp, _vp, _vp, _u64, _vp, _vp, _vp, _vp, _vp, _u32, _u32, _u64,
                                                  _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp])}),
    # device batch rechunk of seekable framed streams to canonical form: clean chunks copied, the other pieces decoded and compressed again, the new index
    "frame_rechunk": ("libsnappier_hip_frame_rechunk.so", "snappier_hip_frame_rechunk.h", {
        "snp_frame_rechunk_indexed_workspace": (_u64, [_u32, _u32, _u64, _u32, _u32]),
        "snp_frame_rechunk_indexed_batch": (_i32, [_vp, _vp, _vp, _vp, _u32, _vp, _vp, _vp, _vp, _vp, _u64, _u32, _u32, _u32, _u64, _u32,
                                                   _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp])}),
    # device batch compose: new seekable framed streams from windows of old ones -- chunks inside a window copied, the cut chunks decoded and compressed again, the new index
    "frame_compose": ("libsnappier_hip_frame_compose.so", "snappier_hip_frame_compose.h", {
        "snp_frame_compose_indexed_workspace": (_u64, [_u32, _u32, _u32, _u32, _u64, _u32, _u32]),
        "snp_frame_compose_indexed_batch": (_i32, [_vp, _vp, _vp, _vp, _u32, _vp, _vp, _vp, _vp, _vp, _u64, _vp, _vp, _vp, _vp, _u32, _u32, _u32, _u32,
                                                   _u64, _u32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp])}),
    # device batch digest: CRC-32C of windows of what seekable framed streams decode to, combined from the chunk headers' CRCs -- only the cut chunks are decoded
    "frame_digest": ("libsnappier_hip_frame_digest.so", "snappier_hip_frame_digest.h", {
        "snp_frame_digest_indexed_workspace": (_u64, [_u32, _u64]),
        "snp_frame_digest_indexed_batch": (_i32, [_vp, _vp, _vp, _vp, _u32, _vp, _vp, _vp, _vp, _vp, _u64, _vp, _vp, _vp, _u32, _u64,
                                                  _vp, _vp, _vp, _vp, _vp]),
        "snp_crc32c_combine": (_u32, [_u32, _u32, _u64])}),
    # device batch diff: longest common prefix and suffix of pairs of windows of what seekable framed streams decode to -- spans between common chunk boundaries compared by header CRC
    "frame_diff": ("libsnappier_hip_frame_diff.so", "snappier_hip_frame_diff.h", {
        "snp_frame_diff_indexed_workspace": (_u64, [_u32, _u64, _u64]),
        "snp_frame_diff_indexed_batch": (_i32, [_vp, _vp, _vp, _vp, _u32, _vp, _vp, _vp, _vp, _vp, _u64, _vp, _vp, _vp, _u32, _vp, _vp, _vp, _vp, _vp, _u64,
                                                _vp, _vp, _vp, _vp, _vp, _vp, _u32, _u32, _u64, _u64, _vp, _vp, _vp, _vp, _vp, _vp, _vp])}),
    # device batch find: where a byte string occurs in windows of what seekable framed streams decode to -- the windows' chunks decoded into scratch and searched there
    "frame_find": ("libsnappier_hip_frame_find.so", "snappier_hip_frame_find.h", {
        "snp_frame_find_indexed_workspace": (_u64, [_u32, _u64, _u64]),
        "snp_frame_find_indexed_batch": (_i32, [_vp, _vp, _vp, _vp, _u32, _vp, _vp, _vp, _vp, _vp, _u64, _vp, _vp, _vp, _u32, _vp, _vp, _vp, _u64, _u64,
                                                _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp])}),
    # device batch edit: a sorted edit script per seekable framed stream -- each touched chunk decoded once, each rewritten region compressed once, the new index
    "frame_edit": ("libsnappier_hip_frame_edit.so", "snappier_hip_frame_edit.h", {
        "snp_frame_edit_indexed_workspace": (_u64, [_u32, _u32, _u32, _u64, _u32]),
        "snp_frame_edit_indexed_batch": (_i32, [_vp, _vp, _vp, _vp, _u32, _vp, _vp, _vp, _vp, _vp, _u64, _vp, _vp, _vp, _vp, _vp, _vp, _u32, _u32, _u32,
                                                _u64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp])}),
    # device content-defined chunking: the cuts the bytes of every buffer define, and the chunked frame encode with the pieces given by the caller
    "frame_cuts": ("libsnappier_hip_frame_cuts.so", "snappier_hip_frame_cuts.h", {
        "snp_content_cuts_workspace": (_u64, [_u32, _u64, _u32]),
        "snp_content_cuts_batch": (_i32, [_vp, _vp, _vp, _vp, _u32, _u32, _u32, _u64, _u64, _vp, _vp, _vp, _vp, _vp]),
        "snp_frame_encode_cuts_workspace": (_u64, [_u32, _u32, _u64]),
        "snp_frame_encode_cuts_batch": (_i32, [_vp, _vp, _vp, _vp, _u32, _vp, _vp, _u64, _u32, _u64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp,
                                               _vp, _vp])}),
    # device batch dedup of seekable framed streams by chunk: the pack, its index and the compose recipes
    "frame_dedup": ("libsnappier_hip_frame_dedup.so", "snappier_hip_frame_dedup.h", {
        "snp_frame_dedup_indexed_workspace": (_u64, [_u32, _u64]),
        "snp_frame_dedup_indexed_batch": (_i32, [_vp, _vp, _vp, _vp, _u32, _vp, _vp, _vp, _vp, _vp, _u64, _u32, _u32, _u32, _u64, _vp, _vp, _vp, _vp,
                                                  _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp])}),
    # device batch recut of seekable framed streams to a caller's cut list: clean chunks copied, the other pieces decoded and compressed again, the new index
    "frame_recut": ("libsnappier_hip_frame_recut.so", "snappier_hip_frame_recut.h", {
        "snp_frame_recut_indexed_workspace": (_u64, [_u32, _u32, _u64, _u32]),
        "snp_frame_recut_indexed_batch": (_i32, [_vp, _vp, _vp, _vp, _u32, _vp, _vp, _vp, _vp, _vp, _u64, _vp, _vp, _u64, _u32, _u32, _u64, _u32,
                                                  _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp])}),
    # device batch verify of seekable framed streams chunk by chunk in bounded scratch, and the repair planner: row verdicts to compose recipes over a replica
    "frame_verify": ("libsnappier_hip_frame_verify.so", "snappier_hip_frame_verify.h", {
        "snp_frame_verify_indexed_workspace": (_u64, [_u32, _u64, _u32, _u64]),
        "snp_frame_verify_indexed_batch": (_i32, [_vp, _vp, _vp, _vp, _u32, _vp, _vp, _vp, _vp, _vp, _u64, _u32, _u64, _vp, _vp, _vp, _vp, _vp, _vp,
                                                   _vp, _vp]),
        "snp_frame_repair_plan_workspace": (_u64, [_u32]),
        "snp_frame_repair_plan_batch": (_i32, [_vp, _vp, _vp, _vp, _vp, _u64, _u32, _vp, _vp, _vp, _u32, _vp, _vp, _u32, _u32, _vp, _vp, _vp, _vp,
                                                _vp, _vp, _vp])}),
}
_loaded: dict[str, C.CDLL] = {}


def _extension_path(name: str) -> str:
    return os.path.join(HERE, _EXTENSIONS[name][0])


def _extension_header(name: str) -> str:
    return os.path.join(HERE, "..", "include", _EXTENSIONS[name][1])


def _extension(name: str) -> C.CDLL:
    """The extension library `name`, loaded once: the product library must be the one in use, every symbol its header declares must be exported
    (an installed copy without include/ falls back to the signature table, as _load does), and the signatures are bound."""
    if name not in _loaded:
        file, _, signatures = _EXTENSIONS[name]
        path, header = _extension_path(name), _extension_header(name)
        base = lib()
        if os.path.realpath(base._name) != os.path.realpath(PRODUCT_PATH):
            raise ImportError(f"{file} is linked against {PRODUCT_PATH}; the loaded library is {base._name}")
        if not os.path.exists(path):
            raise ImportError(f"{path} is missing: build it with `python snappier_amd/build.py`")
        L = C.CDLL(path)
        missing = [s for s in declared_symbols(header) if not hasattr(L, s)] if os.path.exists(header) else []
        if missing:
            raise ImportError(f"{file} does not export: {missing}")
        for fn, (res, args) in signatures.items():
            getattr(L, fn).restype = res
            getattr(L, fn).argtypes = args
        _loaded[name] = L
    return _loaded[name]


BUFFERS_PATH = _extension_path("buffers")
BUFFERS_DECOMPRESS_PATH = _extension_path("buffers_decompress")
FRAME_BUFFERS_PATH = _extension_path("frame_buffers")
LAYOUT_PATH = _extension_path("layout")
FRAME_RANGE_PATH = _extension_path("frame_range")
FRAME_INDEX_PATH = _extension_path("frame_index")
FRAME_CHUNKED_PATH = _extension_path("frame_chunked")
FRAME_UPDATE_PATH = _extension_path("frame_update")
FRAME_APPEND_PATH = _extension_path("frame_append")
FRAME_SPLICE_PATH = _extension_path("frame_splice")
FRAME_RECHUNK_PATH = _extension_path("frame_rechunk")
FRAME_COMPOSE_PATH = _extension_path("frame_compose")
FRAME_DIGEST_PATH = _extension_path("frame_digest")
FRAME_DIFF_PATH = _extension_path("frame_diff")
FRAME_FIND_PATH = _extension_path("frame_find")
FRAME_EDIT_PATH = _extension_path("frame_edit")
FRAME_CUTS_PATH = _extension_path("frame_cuts")
FRAME_DEDUP_PATH = _extension_path("frame_dedup")
FRAME_RECUT_PATH = _extension_path("frame_recut")
FRAME_VERIFY_PATH = _extension_path("frame_verify")


def buffers_lib() -> C.CDLL:
    """libsnappier_hip_buffers.so (include/snappier_hip_buffers.h)."""
    return _extension("buffers")


def buffers_decompress_lib() -> C.CDLL:
    """libsnappier_hip_buffers_decompress.so (include/snappier_hip_buffers_decompress.h)."""
    return _extension("buffers_decompress")


def frame_buffers_lib() -> C.CDLL:
    """libsnappier_hip_frame_buffers.so (include/snappier_hip_frame_buffers.h)."""
    return _extension("frame_buffers")


def layout_lib() -> C.CDLL:
    """libsnappier_hip_layout.so (include/snappier_hip_layout.h)."""
    return _extension("layout")


def frame_range_lib() -> C.CDLL:
    """libsnappier_hip_frame_range.so (include/snappier_hip_frame_range.h)."""
    return _extension("frame_range")


def frame_index_lib() -> C.CDLL:
    """libsnappier_hip_frame_index.so (include/snappier_hip_frame_index.h)."""
    return _extension("frame_index")


def frame_chunked_lib() -> C.CDLL:
    """libsnappier_hip_frame_chunked.so (include/snappier_hip_frame_chunked.h)."""
    return _extension("frame_chunked")


def frame_update_lib() -> C.CDLL:
    """libsnappier_hip_frame_update.so (include/snappier_hip_frame_update.h)."""
    return _extension("frame_update")


def frame_append_lib() -> C.CDLL:
    """libsnappier_hip_frame_append.so (include/snappier_hip_frame_append.h)."""
    return _extension("frame_append")


def frame_splice_lib() -> C.CDLL:
    """libsnappier_hip_frame_splice.so (include/snappier_hip_frame_splice.h)."""
    return _extension("frame_splice")


def frame_rechunk_lib() -> C.CDLL:
    """libsnappier_hip_frame_rechunk.so (include/snappier_hip_frame_rechunk.h)."""
    return _extension("frame_rechunk")


def frame_compose_lib() -> C.CDLL:
    """libsnappier_hip_frame_compose.so (include/snappier_hip_frame_compose.h)."""
    return _extension("frame_compose")


def frame_digest_lib() -> C.CDLL:
    """libsnappier_hip_frame_digest.so (include/snappier_hip_frame_digest.h)."""
    return _extension("frame_digest")


def frame_diff_lib() -> C.CDLL:
    """libsnappier_hip_frame_diff.so (include/snappier_hip_frame_diff.h)."""
    return _extension("frame_diff")


def frame_find_lib() -> C.CDLL:
    """libsnappier_hip_frame_find.so (include/snappier_hip_frame_find.h)."""
    return _extension("frame_find")


def frame_edit_lib() -> C.CDLL:
    """libsnappier_hip_frame_edit.so (include/snappier_hip_frame_edit.h)."""
    return _extension("frame_edit")


def frame_cuts_lib() -> C.CDLL:
    """libsnappier_hip_frame_cuts.so (include/snappier_hip_frame_cuts.h)."""
    return _extension("frame_cuts")


def frame_dedup_lib() -> C.CDLL:
    """libsnappier_hip_frame_dedup.so (include/snappier_hip_frame_dedup.h)."""
    return _extension("frame_dedup")


def frame_recut_lib() -> C.CDLL:
    """libsnappier_hip_frame_recut.so (include/snappier_hip_frame_recut.h)."""
    return _extension("frame_recut")


def frame_verify_lib() -> C.CDLL:
    """libsnappier_hip_frame_verify.so (include/snappier_hip_frame_verify.h)."""
    return _extension("frame_verify")


def buffers_declared_symbols() -> list[str]:
    return declared_symbols(_extension_header("buffers"))


def buffers_decompress_declared_symbols() -> list[str]:
    return declared_symbols(_extension_header("buffers_decompress"))


def frame_buffers_declared_symbols() -> list[str]:
    return declared_symbols(_extension_header("frame_buffers"))


def layout_declared_symbols() -> list[str]:
    return declared_symbols(_extension_header("layout"))


def frame_range_declared_symbols() -> list[str]:
    return declared_symbols(_extension_header("frame_range"))


def frame_index_declared_symbols() -> list[str]:
    return declared_symbols(_extension_header("frame_index"))


def frame_chunked_declared_symbols() -> list[str]:
    return declared_symbols(_extension_header("frame_chunked"))


def frame_update_declared_symbols() -> list[str]:
    return declared_symbols(_extension_header("frame_update"))


def frame_append_declared_symbols() -> list[str]:
    return declared_symbols(_extension_header("frame_append"))


def frame_splice_declared_symbols() -> list[str]:
    return declared_symbols(_extension_header("frame_splice"))


def frame_rechunk_declared_symbols() -> list[str]:
    return declared_symbols(_extension_header("frame_rechunk"))


def frame_compose_declared_symbols() -> list[str]:
    return declared_symbols(_extension_header("frame_compose"))


def frame_digest_declared_symbols() -> list[str]:
    return declared_symbols(_extension_header("frame_digest"))


def frame_diff_declared_symbols() -> list[str]:
    return declared_symbols(_extension_header("frame_diff"))


def frame_find_declared_symbols() -> list[str]:
    return declared_symbols(_extension_header("frame_find"))


def frame_edit_declared_symbols() -> list[str]:
    return declared_symbols(_extension_header("frame_edit"))


def frame_cuts_declared_symbols() -> list[str]:
    return declared_symbols(_extension_header("frame_cuts"))


def frame_dedup_declared_symbols() -> list[str]:
    return declared_symbols(_extension_header("frame_dedup"))


def frame_recut_declared_symbols() -> list[str]:
    return declared_symbols(_extension_header("frame_recut"))


def frame_verify_declared_symbols() -> list[str]:
    return declared_symbols(_extension_header("frame_verify"))


def status_string(st: int) -> str:
    return lib().snp_status_string(st).decode()

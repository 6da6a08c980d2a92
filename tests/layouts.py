"""Kernel layouts of the PRODUCT library (libsnappier_hip.so), selected per context through snp_ctx_set_option -- what the parity and fuzz tests
parametrise over.  No test sets a SNAPPIER_HIP_* variable: the product reads no environment, and every path it contains has an option.
Also exported(): the snp_ names a built library exports, for the tests that hold each library to its header."""
import re
import subprocess

from snappier_amd import _native as N

COMPRESS_LAYOUTS = ["win", "win-np2", "wing", "wind", "lanes", "lanes-exact", "lanes-opts7", "lanes-opts31", "lanes-opts87-slots1", "lanes-opts215-slots1",
                    "lanes-opts151-slots2", "lanes-per16", "lanes-slots4"]
# The four launch forms snp_launch_compress_lanes picks from the batch size (stores | probes per trip | fragments per wavefront), selectable here on
# a batch of any size, and the one remaining wavefront filling: below 8 192 fragments, 8 192 .. 32 767, 32 768 .. 131 071, from 131 072.
# KEPT IN STEP BY HAND with the policy at snappier_amd/csrc/compress_lanes.hip:725-747 (per / opts / slots): when a threshold or a default there
# changes, change these names with it -- nothing derives them from the kernel.
COMPRESS_TIERS = ["lanes-opts71-slots2-per16", "lanes-opts71-slots2-per32", "lanes-opts87-slots2-per32", "lanes-opts215-slots1-per64"]
COMPRESS_LAYOUTS += COMPRESS_TIERS + ["lanes-per8"]
# chains = the default (decode_chains.hip after the small-block policy); wave-only = no pre-pass; serial = decompress.hip's tag-by-tag kernel;
# small* = every block through the small-block pre-pass first (decompress_small.hip), leftovers to the list kernel -- except small-grid, which
# runs NO pre-pass: SNP_OPT_DECODE_LEFTOVERS = 1 without a pinned pre-pass layout makes launch_decompress (capi_batch.hip: prepass = redo_list ||
# !chains || pinned || (!redo_grid && !hint_mostly_large)) skip it, so every block goes one per wavefront (k_decode_chains) and the capacities
# are sampled for the next batch's hint; the pre-pass with one workgroup per leftover needs !chains, which no option of the product sets
DECODE_LAYOUTS = ["chains", "wave-only", "serial", "small", "small-grid", "small-lanes", "small-team4", "small-team8", "small-team16"]


def set_compress_layout(ctx, layout: str):
    """win = one fragment per wavefront, table in LDS (-np2: two window positions per lane); wing = the same with the table in a global slot;
    wind = both forms side by side (two streams, one ticket counter);
    lanes = one fragment per lane, tables in the HBM workspace (-exact: exact-length stores only; -optsN: SNP_OPT_COMPRESS_LANE_STORES = N;
    -slotsN: N probes per trip; -perN: N fragments per wavefront)."""
    base = layout.split("-")[0]
    ctx.set_option(N.OPT_COMPRESS_LAYOUT, {"auto": N.COMPRESS_AUTO, "win": N.COMPRESS_WINDOW_LDS, "win2": N.COMPRESS_WINDOW_LDS,
                                           "wing": N.COMPRESS_WINDOW_GLOBAL, "wind": N.COMPRESS_WINDOW_DUAL, "lanes": N.COMPRESS_LANES}[base])
    ctx.set_option(N.OPT_COMPRESS_WINDOW_POSITIONS, 2 if (base == "win2" or "-np2" in layout) else 1)
    if layout.endswith("-exact"):
        ctx.set_option(N.OPT_COMPRESS_LANE_STORES, 0)
    for part in layout.split("-")[1:]:
        if part.startswith("opts"):
            ctx.set_option(N.OPT_COMPRESS_LANE_STORES, int(part[4:]))
        elif part.startswith("slots"):
            ctx.set_option(N.OPT_COMPRESS_LANE_PROBES, int(part[5:]))
        elif part.startswith("per"):
            ctx.set_option(N.OPT_COMPRESS_LANES_PER_WAVEFRONT, int(part[3:]))
    return ctx


def set_decode_layout(ctx, decode: str, fenced=None, small_max: int = 65536):
    if fenced is not None:
        ctx.set_option(N.OPT_FENCED, int(fenced))
    if decode == "chains":
        ctx.set_option(N.OPT_DECODE_LAYOUT, N.DECODE_AUTO)
    elif decode == "wave-only":
        ctx.set_option(N.OPT_DECODE_LAYOUT, N.DECODE_WAVE_ONLY)
    elif decode == "serial":
        ctx.set_option(N.OPT_DECODE_LAYOUT, N.DECODE_SERIAL)
    elif decode.startswith("small"):
        kind = decode.split("-")[1] if "-" in decode else ""
        ctx.set_option(N.OPT_DECODE_LAYOUT, {"": N.DECODE_AUTO, "grid": N.DECODE_AUTO, "lanes": N.DECODE_SMALL_LANES, "team4": N.DECODE_SMALL_TEAM4,
                                             "team8": N.DECODE_SMALL_TEAM8, "team16": N.DECODE_SMALL_TEAM16}[kind])
        ctx.set_option(N.OPT_SMALL_BLOCK_MIN_BATCH, 1)
        ctx.set_option(N.OPT_SMALL_BLOCK_MAX, small_max)
        ctx.set_option(N.OPT_DECODE_LEFTOVERS, 1 if kind == "grid" else 2)   # 2: always the pre-pass, whatever the previous batch was like (1: never, see above)
    else:
        raise ValueError(decode)
    return ctx


def exported(path: str) -> set[str]:
    """The snp_ functions the shared library at `path` exports (nm -D --defined-only)."""
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return {m.group(1) for m in re.finditer(r" T (snp_[a-z0-9_]+)$", out, flags=re.M)}

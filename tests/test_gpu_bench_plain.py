"""bench.py as a plain run (no --full) with --dump-outputs: the headline fields, nothing of what --full adds, and outputs that are what the codec
computes -- the sampled decompressed blocks are the inputs, the sampled compressed blocks are the oracle's bytes."""
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, read_testdata

pytestmark = pytest.mark.gpu


@pytest.mark.timeout(400)
def test_plain_bench_run_dumps_the_last_step(tmp_path):
    import torch
    import oracle as O
    from snappier_amd import datagen as SD
    spec = importlib.util.spec_from_file_location("bench_for_test", os.path.join(ROOT, "bench.py"))
    B = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(B)
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    nb, steps = 4096, 3
    out = tmp_path / "outputs"
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", "1", "--blocks", str(nb),
           "--dump-outputs", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, env=env, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr[-3000:]
    line = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert line["metric"] == "uncompressed GB/s block compress+decompress, 64 KiB blocks" and line["unit"] == "GB/s"
    assert line["higher_is_better"] is True and line["dtype"] == "u8" and line["steps"] == steps
    assert line["value"] > 0 and line["ms_per_step"] > 0
    assert abs(line["value"] - nb * 65536 / (line["ms_per_step"] * 1e-3) / 1e9) <= 0.01 * line["value"]
    for k in ("cpu_baseline", "other_configs", "config5_lines"):
        assert k not in line, k
    assert line["per_rank"] is None and line["value_plain_workspace"] is None and line["value_default_search"] is None

    got = {f[:-4]: np.load(out / f) for f in os.listdir(out)}
    assert set(got) == {"compressed_lengths", "compress_status", "compressed_bytes_sample", "decompressed_lengths", "decompress_status",
                        "decompressed_bytes_sample"}
    assert all(v.dtype == np.float32 for v in got.values()) and sum(v.nbytes for v in got.values()) <= 64 * 10**6
    assert got["compressed_lengths"].shape == (nb,) and not got["compress_status"].any() and not got["decompress_status"].any()
    assert (got["decompressed_lengths"] == 65536).all()
    raw = SD.html_like_blocks(read_testdata("html"), 0, nb, "cuda:0").cpu().numpy().reshape(nb, 65536)
    torch.cuda.synchronize()
    idx = np.sort(np.random.default_rng(B.DUMP_SEED).choice(nb, size=B.DUMP_SAMPLE_BLOCKS, replace=False))    # the documented sample
    assert np.array_equal(got["decompressed_bytes_sample"].astype(np.uint8), raw[idx])
    for b, cbytes in zip(idx, got["compressed_bytes_sample"]):
        want = O.compress(raw[b].tobytes(), O.HASH_CRC32C)
        assert int(got["compressed_lengths"][b]) == len(want)
        assert cbytes[: len(want)].astype(np.uint8).tobytes() == want and not cbytes[len(want):].any()

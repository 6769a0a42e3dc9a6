"""GPU: a plain `bench.py --gpus 1 --steps K --warmup W` run — the headline
only (nothing that `--full` adds), K timed steps, and with `--dump-outputs`
the last timed step's checksums, which are the reference's for config 0."""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, golden


@pytest.mark.gpu
def test_plain_run_times_the_headline_and_dumps_its_outputs(tmp_path):
    dump = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--settle-ms", "10", "--dump-outputs", str(dump)],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-3000:]
    out = [l for l in r.stdout.splitlines() if l.strip()]
    assert len(out) == 1, r.stdout
    d = json.loads(out[0])
    assert d["full"] is False and d["steps"] == 3 and d["warmup"] == 1 and d["n_gpus"] == 1
    assert d["unit"] == "GiB/s" and d["higher_is_better"] is True and d["dtype"] == "u8"
    assert d["value"] > 0 and d["ms_per_step"] > 0
    # value and ms_per_step describe the same timed region
    n_bytes = d["config"]["segments_total"] * d["config"]["segment_bytes"]
    assert d["value"] == pytest.approx(n_bytes / (d["ms_per_step"] / 1e3) / 2**30, rel=1e-2)
    # everything else the benchmark can measure waits for --full
    assert d["config5"] is None and d["cpu_baseline"] is None and d["host_inclusive"] is None
    assert d["bit_exact"] is None and d["roofline"]["traffic"] is None
    assert d["roofline"]["kernel_ms"] > 0 and d["per_rank"][0]["kernel_ms"] > 0
    # the dump: one float32 per segment, exactly the reference's config-0 outputs
    assert sorted(os.listdir(dump)) == ["checksums.npy"]
    a = np.load(dump / "checksums.npy")
    assert a.dtype == np.float32 and a.shape == (1 << 20,)
    u16 = a.astype(np.uint16)
    assert (u16.astype(np.float32) == a).all()
    assert hashlib.sha256(u16.tobytes()).hexdigest() == golden("configs.json")["0"]["out_sha256"]

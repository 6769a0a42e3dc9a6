"""CPU: bench.py's own rank launcher (`--gpus N` with no outer torchrun) and
its world-size check — the wiring the driver's 1/2/4/8-GPU scaling runs use.
`--launch-check` makes every rank join a gloo group and report what it saw,
without touching a GPU."""
import json
import os
import subprocess
import sys

import pytest

from conftest import ROOT

BENCH = os.path.join(ROOT, "bench.py")


def _env(**kw):
    env = {k: v for k, v in os.environ.items()
           if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env.update(kw)
    return env


@pytest.mark.parametrize("n", [2, 3, 8])
def test_gpus_n_starts_n_ranks(n):
    r = subprocess.run([sys.executable, BENCH, "--gpus", str(n), "--launch-check"], env=_env(),
                       capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-2000:]
    out = [l for l in r.stdout.splitlines() if l.strip()]
    assert len(out) == 1, r.stdout  # rank 0's line only (gloo's connection lines go to stderr)
    lines = [json.loads(out[0])]
    seen = lines[0]["launch_check"]
    assert sorted(s["rank"] for s in seen) == list(range(n))
    assert sorted(s["local_rank"] for s in seen) == list(range(n))
    assert {s["world_size"] for s in seen} == {n}
    assert {s["master_addr"] for s in seen} == {"127.0.0.1"}
    assert len({s["pid"] for s in seen}) == n  # one process per rank


def test_driver_style_outer_launcher():
    """The driver's own form: torch.distributed.run starts the ranks and each
    runs `bench.py --gpus N`; bench.py must not launch again."""
    import socket

    n = 4
    with socket.socket() as so:
        so.bind(("127.0.0.1", 0))
        port = so.getsockname()[1]
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}",
                        "--master-addr", "127.0.0.1", "--master-port", str(port), BENCH, "--gpus", str(n),
                        "--launch-check"], env=_env(), capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-2000:]
    out = [l for l in r.stdout.splitlines() if l.strip()]
    assert len(out) == 1, r.stdout  # the driver reads exactly one line
    seen = json.loads(out[0])["launch_check"]
    assert sorted(s["rank"] for s in seen) == list(range(n)) and {s["world_size"] for s in seen} == {n}
    assert len({s["pid"] for s in seen}) == n


def test_world_size_must_match_gpus():
    r = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--launch-check"],
                       env=_env(WORLD_SIZE="2", RANK="0", LOCAL_RANK="0"),
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 2
    assert "WORLD_SIZE=2 but --gpus 1" in r.stderr


def test_dump_outputs_writes_exact_float32(tmp_path):
    """--dump-outputs: the int16 output tensor's 16-bit patterns as float32
    values 0..65535, one file per rank of an N > 1 run"""
    import numpy as np
    import torch

    sys.path.insert(0, ROOT)
    import bench

    u16 = np.array([0, 1, 0x7FFF, 0x8000, 0xFFFF, 0x5A5A], dtype=np.uint16)
    out = torch.from_numpy(u16.view(np.int16).copy())
    bench.dump_outputs(str(tmp_path / "one"), out, 0, 1)
    got = np.load(tmp_path / "one" / "checksums.npy")
    assert got.dtype == np.float32 and (got == u16.astype(np.float32)).all()
    bench.dump_outputs(str(tmp_path / "two"), out, 1, 2)
    assert sorted(os.listdir(tmp_path / "two")) == ["checksums_rank1.npy"]


def test_full_is_off_by_default(monkeypatch):
    sys.path.insert(0, ROOT)
    import bench

    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "2"])
    a = bench.parse()
    assert a.full is False and a.dump_outputs is None and a.steps == 7 and a.warmup == 2
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "d"])
    a = bench.parse()
    assert a.full is True and a.dump_outputs == "d"
    monkeypatch.setattr(sys, "argv", ["bench.py", "--steps", "0"])
    with pytest.raises(SystemExit):
        bench.parse()


def test_cpu_share_reports_usable_cpus():
    sys.path.insert(0, ROOT)
    import bench

    n, how = bench.cpu_share()
    assert 1 <= n <= (os.cpu_count() or 1)
    assert "host CPUs" in how

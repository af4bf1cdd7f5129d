"""bench.py driver contract on the CPU: one JSON line, for N=1, for N=2 self-launched
(no torchrun: bench.py starts its own worker processes) and for N=2 under torchrun."""

from __future__ import annotations

import json
import os
import socket
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = {"metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
        "vs_baseline", "dtype", "data", "config"}


def _free_port() -> int:
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _env():
    return dict(os.environ, PYTHONPATH=ROOT, CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES="", OMP_NUM_THREADS="2",
                P2PFL_LOCKCHECK="0")


def _json_lines(out: str):
    return [json.loads(ln) for ln in out.splitlines() if ln.startswith("{")]


@pytest.mark.timeout(600)
@pytest.mark.parametrize("world,launcher", [(1, "self"), (2, "self"), (2, "torchrun")])
def test_bench_json_line(world, launcher):
    args = ["bench.py", "--gpus", str(world), "--steps", "1", "--warmup", "1", "--impl", "torch", "--number-sub", "200",
            "--watchdog", "300"]
    if launcher == "self":
        cmd = [sys.executable] + args
    else:
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={world}",
               "--master-addr=127.0.0.1", f"--master-port={_free_port()}"] + args
    r = subprocess.run(cmd, cwd=ROOT, env=_env(), capture_output=True, text=True, timeout=560)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    lines = _json_lines(r.stdout)
    assert len(lines) == 1, r.stdout  # rank 0 only
    rec = lines[0]
    assert KEYS <= set(rec)
    assert rec["n_gpus"] == world and rec["steps"] == 1 and rec["scaling"] == "weak"
    assert rec["config"]["parallelism"] == "gossip-p2p"  # full Node stack, gossip over the xGMI transport
    assert rec["value"] > 0 and rec["ms_per_step"] > 0
    # whole-job aggregate: value = per-peer throughput x peers
    assert abs(rec["value"] - rec["samples_per_sec_per_peer"] * world) <= 1e-3 * rec["value"] + 0.2


@pytest.mark.timeout(600)
def test_bench_dump_outputs_and_full(tmp_path):
    """``--dump-outputs`` writes the last timed round's model as float32 .npy files, the same
    from run to run (seeded inputs); ``--full`` adds the reports a plain run leaves out."""
    import numpy as np

    base = [sys.executable, "bench.py", "--gpus", "1", "--steps", "2", "--warmup", "1", "--impl", "torch",
            "--number-sub", "200", "--watchdog", "300"]
    runs = {}
    for tag, extra in (("plain", []), ("full", ["--full"])):
        out = tmp_path / tag
        r = subprocess.run(base + extra + ["--dump-outputs", str(out)], cwd=ROOT, env=_env(), capture_output=True,
                           text=True, timeout=280)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
        rec = _json_lines(r.stdout)[0]
        assert rec["steps"] == 2 and rec["ms_per_step"] > 0
        assert ("all spans, ms per round" in r.stderr) == (tag == "full")
        assert (f"round {1 + 2}: wall" in r.stderr) == (tag == "full")
        runs[tag] = {p.name: np.load(p) for p in sorted(out.iterdir())}
    from p2pfl_amd.models import CNN

    want = {k: tuple(v.shape) for k, v in CNN(seed=1234).state_dict().items()}
    for tag, arrs in runs.items():
        assert {k: a.shape for k, a in arrs.items()} == {k + ".npy": s for k, s in want.items()}, tag
        assert all(a.dtype == np.float32 and np.isfinite(a).all() for a in arrs.values())
        assert sum(a.nbytes for a in arrs.values()) <= 64 << 20
    init = CNN(seed=1234).state_dict()
    for name, a in runs["plain"].items():
        # same seeded inputs, same fp32 CPU arithmetic: only summation order may differ
        np.testing.assert_allclose(a, runs["full"][name], rtol=1e-4, atol=1e-6)
        # ... and it is the trained model, not the initial one
        if name.endswith("weight.npy"):
            assert np.abs(a - init[name[:-4]].numpy()).max() > 0


def test_bench_dump_samples_large_models(tmp_path):
    """A model above the size budget is written as the same seeded sample every time."""
    import numpy as np

    sys.path.insert(0, ROOT)
    import bench

    rng = np.random.default_rng(0)
    outs = {"a.weight": rng.standard_normal((300, 41), dtype=np.float32),
            "b.bias": rng.standard_normal(7, dtype=np.float32),
            "c.weight": rng.standard_normal((25, 409)).astype(np.float64)}
    budget = 40_000  # the three hold 90,108 bytes as float32
    for d in ("x", "y"):
        bench.dump_outputs(str(tmp_path / d), outs, budget=budget)
    total = 0
    for name, src in outs.items():
        x, y = np.load(tmp_path / "x" / (name + ".npy")), np.load(tmp_path / "y" / (name + ".npy"))
        assert x.dtype == np.float32 and x.ndim == 1 and 1 <= x.size < src.size
        assert np.array_equal(x, y)
        assert np.isin(x, src.astype(np.float32)).all()
        total += x.nbytes
    assert 0.9 * budget <= total <= budget
    # below the budget everything is written, in its own shape
    bench.dump_outputs(str(tmp_path / "z"), outs)
    for name, src in outs.items():
        assert np.array_equal(np.load(tmp_path / "z" / (name + ".npy")), src.astype(np.float32))
    assert bench.DUMP_BUDGET_BYTES <= 64 << 20


@pytest.mark.timeout(600)
def test_reference_baseline_script_runs():
    """The reference-equivalent baseline (scripts/reference_baseline.py) still runs."""
    cmd = [sys.executable, "scripts/reference_baseline.py", "--steps", "1", "--warmup", "0", "--number-sub", "200"]
    r = subprocess.run(cmd, cwd=ROOT, env=_env(), capture_output=True, text=True, timeout=560)
    assert r.returncode == 0, r.stderr[-3000:]
    rec = _json_lines(r.stdout)[0]
    assert rec["ms_per_round"] > 0 and rec["dtype"] == "fp32"

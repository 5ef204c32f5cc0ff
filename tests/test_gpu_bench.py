"""GPU: bench.py's multi-rank path as the driver starts it (`bench.py --gpus N`, no launcher).

Two ranks share the one GPU of a test box over gloo (RCCL refuses two ranks on one device); the
8-GPU scaling run uses the same code path with RCCL."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def _bench_line(argv):
    env = dict(os.environ)
    env.pop("WORLD_SIZE", None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + argv, capture_output=True, text=True,
                       timeout=300, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [x for x in r.stdout.splitlines() if x.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


def test_plain_run_times_the_steps_and_dumps_the_last_frame(gpu_available, tmp_path):
    """A plain run (64k entities) times exactly --steps frames and prints the headline only: no
    per-kernel pass, no leg beside it.  --dump-outputs writes the last timed frame as float64 arrays
    whose lengths are the line's event counts, the same from one run to the next."""
    import numpy as np
    argv = ["--gpus", "1", "--entities", "65536", "--groups", "256", "--steps", "4", "--warmup", "2"]
    out = _bench_line(argv + ["--dump-outputs", str(tmp_path / "a")])
    assert out["steps"] == 4 and out["warmup"] == 2 and out["unit"] == "entity-ticks/s" and out["higher_is_better"]
    assert out["ms_per_step"] > 0 and abs(out["value"] - 65536 / (out["ms_per_step"] * 1e-3)) <= 1e-6 * out["value"]
    for moved in ("kernels", "roofline", "cpu_baseline", "host_calls", "plugin_frame", "configs", "adapter_frame"):
        assert moved not in out
    a = {p.name[:-4]: np.load(p) for p in (tmp_path / "a").iterdir()}
    assert all(x.dtype == np.float64 for x in a.values())
    pf = out["per_frame"]
    assert len(a["ev_obj"]) == len(a["ev_new"]) == pf["prop_events"] > 0
    assert len(a["fi_obj"]) == pf["fired"] > 0 and len(a["mr_obj"]) == pf["msgs"] > 0
    assert len(a["prop_00"]) == 65536
    _bench_line(argv + ["--dump-outputs", str(tmp_path / "b")])
    for name, x in a.items():
        assert np.array_equal(x, np.load(tmp_path / "b" / (name + ".npy")), equal_nan=True), name


def test_bench_gpus_2_starts_two_ranks_and_migrates(gpu_available):
    """BASELINE config[2]'s shape at 64k entities per rank: bench.py starts both ranks itself,
    rank 0 prints one line with n_gpus = 2, and entities crossed shards (SwitchScene, KM:901-951)."""
    env = dict(os.environ)
    env.pop("WORLD_SIZE", None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--backend", "gloo",
                        "--entities", "65536", "--groups", "256", "--steps", "3", "--warmup", "2",
                        "--cpu-baseline", "off"], capture_output=True, text=True, timeout=300, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [x for x in r.stdout.splitlines() if x.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    out = json.loads(lines[0])
    assert out["n_gpus"] == 2 and out["steps"] == 3
    assert out["migrations"]["out"] > 0 and out["migrations"]["out"] == out["migrations"]["in"]
    assert out["value"] > 0 and out["config"]["entities_per_gpu"] == 65536

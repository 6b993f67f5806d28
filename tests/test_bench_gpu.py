"""bench.py on the GPU: a plain run times the training steps only
(``inference`` null, default atomic-accumulation step); ``--full`` adds the
graphed inference measurement; a run that dumps its outputs takes its steps
in deterministic mode and lists what it wrote.  Smoke-sized shapes."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARGS = ["--gpus", "1", "--steps", "2", "--warmup", "1", "--batch", "2", "--size", "128", "160", "--iters", "3",
        "--infer-size", "128", "160", "--infer-reps", "2"]


def _run(extra):
    env = dict(os.environ)
    env.pop("WORLD_SIZE", None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + ARGS + extra, env=env,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


def test_plain_run_times_training_only(cuda):
    out = _run([])
    assert out["inference"] is None and out["dumped"] is None
    assert out["steps"] == 2 and out["ms_per_step"] > 0 and out["dtype"] == "bf16"
    assert out["config"]["ops"] == "hip-kernels" and out["config"]["deterministic"] is False


def test_full_run_measures_inference_and_dumps(cuda, tmp_path):
    out = _run(["--full", "--dump-outputs", str(tmp_path)])
    inf = out["inference"]
    assert inf["mode"] == "hipgraph" and inf["fps"] > 0 and inf["size"] == [128, 160] and inf["iters"] == 3
    assert out["config"]["deterministic"] is True  # --deterministic auto: on in a run that dumps
    assert out["dumped"] == ["flow_final", "loss", "params"]
    flow, loss, params = (np.load(tmp_path / (n + ".npy")) for n in out["dumped"])
    assert flow.dtype == loss.dtype == params.dtype == np.float32
    assert flow.shape == (2, 2, 128, 160) and params.shape == (5257536,)
    assert np.isfinite(flow).all() and np.isfinite(params).all()
    assert abs(float(loss[0]) - out["final_loss"]) < 1e-3

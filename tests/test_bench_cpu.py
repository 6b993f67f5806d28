"""bench.py driver contract on the CPU (gloo ranks): ``--gpus N`` started
without a launcher must spawn N ranks itself (torch.distributed.run as a child
process), time the step on every rank and print ONE JSON line from rank 0
with the whole-job value and ``n_gpus``/``parallelism`` = N."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARGS = ["--device", "cpu", "--steps", "2", "--warmup", "1", "--batch", "1", "--size", "128", "128",
        "--iters", "2"]


def _run(extra):
    env = dict(os.environ)
    env.pop("WORLD_SIZE", None)
    env["OMP_NUM_THREADS"] = "2"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + ARGS + extra, env=env,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout  # exactly one JSON line (rank 0)
    return json.loads(lines[0])


def test_bench_spawns_ranks_for_gpus_n():
    out = _run(["--gpus", "2"])
    assert out["n_gpus"] == 2
    assert out["config"]["parallelism"] == "dp2"
    assert out["config"]["global_batch"] == 2
    assert out["steps"] == 2 and out["warmup"] == 1
    assert out["value"] > 0 and out["final_loss"] == out["final_loss"]  # finite
    # whole-job value: global pairs / the slowest rank's time
    assert abs(out["value"] - 2 * 2 / (out["ms_per_step"] * 2 / 1000.0)) / out["value"] < 0.01


def test_bench_single_rank_default():
    out = _run([])
    assert out["n_gpus"] == 1 and out["config"]["parallelism"] == "dp1"


def test_bench_dump_outputs(tmp_path):
    """``--dump-outputs DIR`` writes what the LAST timed step computed (loss,
    updated parameters, final flow prediction) as float32 .npy files and lists
    them in the result line.  The inputs are seeded: 1 warm-up + 2 timed steps
    and 0 + 3 take the same three steps and must dump the same values, while
    0 + 2 stops one step earlier and must not."""
    import numpy as np
    a = _run(["--dump-outputs", str(tmp_path / "a")])
    b = _run(["--steps", "3", "--warmup", "0", "--full", "--dump-outputs", str(tmp_path / "b")])
    c = _run(["--steps", "2", "--warmup", "0", "--dump-outputs", str(tmp_path / "c")])
    names = ["flow_final.npy", "loss.npy", "params.npy"]
    assert a["steps"] == 2 and b["steps"] == 3 and a["ms_per_step"] > 0
    assert a["inference"] is None and b["inference"] is None  # --full measures inference on the GPU only
    assert a["dumped"] == [n[:-4] for n in names] and _run([])["dumped"] is None
    assert sorted(os.listdir(tmp_path / "a")) == names
    got = {r: {n: np.load(tmp_path / r / n) for n in names} for r in "abc"}
    assert all(v.dtype == np.float32 and np.isfinite(v).all() for v in got["a"].values())
    assert got["a"]["flow_final.npy"].shape == (1, 2, 128, 128) and got["a"]["params.npy"].shape == (5257536,)
    assert abs(float(got["a"]["loss.npy"][0]) - a["final_loss"]) < 1e-3
    for n in names:  # same three steps: fp32 CPU ops, same thread count -> round-off at most
        np.testing.assert_allclose(got["b"][n], got["a"][n], rtol=1e-4, atol=1e-5)
    # one AdamW step moves every weight by about the learning rate (OneCycle start: 4e-4 / 25)
    assert np.abs(got["c"]["params.npy"] - got["a"]["params.npy"]).max() > 1e-6
    assert np.abs(got["c"]["flow_final.npy"] - got["a"]["flow_final.npy"]).max() > 1e-4
    assert abs(c["final_loss"] - a["final_loss"]) > 1e-3


def test_dump_outputs_samples_above_the_size_limit(tmp_path, monkeypatch):
    """Above the 64 MB limit the flow is written as a fixed, seeded sample of
    its elements: the same elements every time, in order, within the limit."""
    import importlib.util
    import numpy as np
    import torch
    spec = importlib.util.spec_from_file_location("bench_under_test", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    model = torch.nn.Linear(10, 10)  # 110 parameters
    flow = torch.arange(2 * 2 * 5 * 10, dtype=torch.float32).reshape(2, 2, 5, 10)
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 4 * 110 + 4 + 4 * 50)
    for d in ("x", "y"):
        assert bench.dump_outputs(str(tmp_path / d), torch.tensor(1.5), model, flow) == ["flow_final", "loss", "params"]
    x, y = np.load(tmp_path / "x" / "flow_final.npy"), np.load(tmp_path / "y" / "flow_final.npy")
    assert x.shape == (50,) and np.array_equal(x, y)
    assert np.all(np.diff(x) > 0) and set(x.tolist()) <= set(range(200))  # distinct elements of the flow, in order
    payload = sum(np.load(tmp_path / "x" / n).nbytes for n in os.listdir(tmp_path / "x"))
    assert payload <= 4 * 110 + 4 + 4 * 50
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 64 * 10**6)
    bench.dump_outputs(str(tmp_path / "z"), torch.tensor(1.5), model, flow)
    assert np.array_equal(np.load(tmp_path / "z" / "flow_final.npy"), flow.numpy())  # within the limit: all of it

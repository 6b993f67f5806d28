"""Warm-started sequence tracking on the CPU: the ATen oracle of forward
interpolation against fp64, the reference's recorded outputs and hand-made
edge inputs; SequenceTracker against the hand-written loop; the track.py CLI."""
import glob
import importlib.util
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from raft_stir_amd import ops
from raft_stir_amd.config import make_args
from raft_stir_amd.export.pointtrack import RaftPointTrack, SequenceTracker, sample_points
from raft_stir_amd.models import RAFT
from raft_stir_amd.ops import reference

from conftest import REFERENCE
from warm_start_cases import check_against_fp64, check_edge_outputs, edge_cases, smooth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "ref_forward_interpolate.npz")


# ------------------------------------------------------------------- the oracle
@pytest.mark.parametrize("amp,noise", [(1, 0.1), (6, 0.5), (40, 2)])
@pytest.mark.parametrize("seed", [0, 1, 2])
@pytest.mark.parametrize("shape", [(5, 7), (16, 20), (46, 62)])
def test_oracle_against_fp64(shape, seed, amp, noise):
    flow = smooth(*shape, seed, amp, noise)
    out = reference.forward_interpolate(flow[None])[0]
    assert out.dtype == torch.float32 and out.shape == flow.shape
    check_against_fp64(flow, out)


def test_tiny_field_without_valid_sample_gives_zeros():
    # amp 40 on 5x7 throws every sample off the grid for some seed: find one, do not assume it
    hit = 0
    for seed in range(40):
        flow = smooth(5, 7, seed, 40, 2)
        if check_against_fp64(flow, reference.forward_interpolate(flow[None])[0]) == 0:
            hit += 1
    assert hit > 0


def test_oracle_reproduces_reference_outputs():
    """tests/golden/ref_forward_interpolate.npz: flows from smooth() and what the
    reference's own forward_interpolate (scipy griddata 'nearest') returned."""
    z = np.load(GOLDEN)
    keys = sorted(k[5:] for k in z.files if k.startswith("flow_"))
    assert len(keys) == 12
    for k in keys:
        H, W = (int(v) for v in k.split("_")[0].split("x"))
        seed, amp = int(k.split("_s")[1].split("_")[0]), int(k.split("_a")[1])
        flow = torch.from_numpy(z["flow_" + k])
        assert torch.equal(flow, smooth(H, W, seed, amp, {1: 0.1, 6: 0.5}[amp])), k
        got = reference.forward_interpolate(flow[None])[0]
        want = torch.from_numpy(z["out_" + k])
        assert (got != want).float().mean().item() == 0, k


def test_golden_case_recomputed_from_reference():
    path = os.path.join(REFERENCE, "core", "utils", "utils.py")
    if not os.path.isfile(path):
        pytest.skip("reference not mounted")
    pytest.importorskip("scipy")
    spec = importlib.util.spec_from_file_location("_ref_core_utils", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    z = np.load(GOLDEN)
    flow = torch.from_numpy(z["flow_46x62_s1_a6"])
    want = mod.forward_interpolate(flow)
    assert torch.equal(want, torch.from_numpy(z["out_46x62_s1_a6"]))
    assert torch.equal(reference.forward_interpolate(flow[None])[0], want)


def test_edge_inputs():
    check_edge_outputs({name: reference.forward_interpolate(flow) for name, flow, _ in edge_cases()})


def test_wrapper_shapes_and_dtypes():
    flow = smooth(16, 20, 1, 6, 0.5)
    a = ops.forward_interpolate(flow)
    b = ops.forward_interpolate(flow[None])
    assert a.shape == (2, 16, 20) and b.shape == (1, 2, 16, 20) and a.dtype == torch.float32
    assert torch.equal(a, b[0])
    assert torch.equal(a, reference.forward_interpolate(flow[None])[0])
    two = torch.stack([flow, smooth(16, 20, 2, 1, 0.1)])
    out = ops.forward_interpolate(two)
    assert torch.equal(out[0], a) and torch.equal(out[1], ops.forward_interpolate(two[1]))
    h = ops.forward_interpolate(flow.to(torch.bfloat16))
    assert h.dtype == torch.float32
    assert torch.equal(h, ops.forward_interpolate(flow.to(torch.bfloat16).float()))
    with pytest.raises(ValueError):
        ops.forward_interpolate(torch.zeros(3, 4, 5))


# -------------------------------------------------------------- SequenceTracker
@pytest.fixture(scope="module")
def small_model():
    torch.manual_seed(0)
    return RAFT(make_args(small=True)).eval()


@pytest.fixture(scope="module")
def sequence():
    """4 frames of 128x160, the smallest the model handles: below 128 rows the
    top level of the 4-level correlation pyramid is one cell wide, the bilinear
    lookup divides by W - 1 = 0 and the flow is NaN everywhere (at 64x80 every
    comparison of this file would compare NaN with NaN)."""
    g = torch.Generator().manual_seed(5)
    frames = torch.rand(4, 1, 3, 128, 160, generator=g) * 255
    points = torch.rand(1, 8, 2, generator=g) * torch.tensor([159.0, 127.0])
    return frames, points


@pytest.fixture(scope="module")
def hand_loop(small_model, sequence):
    """The loop of SequenceTracker written out, with warm start."""
    frames, points = sequence
    traj, inits = [points[0]], []
    pts, init = points, torch.zeros(1, 2, 16, 20)
    with torch.no_grad():
        for t in range(1, len(frames)):
            inits.append(init)
            lo, up = small_model(frames[t - 1], frames[t], iters=2, flow_init=init, test_mode=True)
            pts = pts + sample_points(up, pts)
            init = ops.forward_interpolate(lo)
            traj.append(pts[0])
    return torch.stack(traj), inits


def test_tracker_matches_hand_written_loop(small_model, sequence, hand_loop):
    frames, points = sequence
    want, inits = hand_loop
    trk = SequenceTracker(small_model, iters=2, warm_start=True)
    traj = trk.track(frames, points)
    assert traj.shape == (4, 8, 2)
    assert torch.equal(traj[0], points[0])
    assert torch.equal(traj, want)
    assert any(i.abs().max() > 0 for i in inits[1:])  # the warm start did start warm
    # a list of frames, stepped by hand, with the per-step state readable
    trk.reset()
    assert torch.equal(trk.step(frames[0], points), points)
    for t in range(1, 4):
        pts = trk.step(frames[t])
        assert torch.equal(pts[0], want[t])
        assert torch.equal(trk.flow_init, inits[t - 1])
        assert torch.equal(trk.next_init, ops.forward_interpolate(trk.flow_low))
        assert trk.flow_up.shape == (1, 2, 128, 160) and trk.flow_low.shape == (1, 2, 16, 20)
    assert torch.equal(trk.track(list(frames), points), want)


def test_tracker_reset_and_shape_checks(small_model, sequence):
    frames, points = sequence
    trk = SequenceTracker(small_model, iters=2)
    trk.step(frames[0], points)
    first = trk.step(frames[1]).clone()
    with pytest.raises(ValueError):
        trk.step(torch.zeros(1, 3, 128, 168))  # another shape within the sequence
    trk.reset()
    assert trk.flow_init is None and trk.next_init is None and trk.points is None
    with pytest.raises(ValueError):
        trk.step(frames[1])  # a fresh sequence needs points
    trk.step(frames[0], points)
    assert torch.equal(trk.step(frames[1]), first)  # nothing of the old sequence is left
    trk.reset()
    assert torch.equal(trk.step(torch.zeros(1, 3, 128, 168), points), points)  # new shape after reset
    for bad in (torch.zeros(1, 3, 124, 160), torch.zeros(1, 3, 128, 161)):
        with pytest.raises(ValueError, match="multiples of 8"):
            SequenceTracker(small_model, iters=2).step(bad, points)


def test_tracker_without_warm_start_is_chained_pairs(small_model, sequence):
    frames, points = sequence
    pair = RaftPointTrack(small_model, iters=2)
    pts, want = points, [points[0]]
    with torch.no_grad():
        for t in range(1, 4):
            pts = pair(pts, frames[t - 1], frames[t])
            want.append(pts[0])
    trk = SequenceTracker(small_model, iters=2, warm_start=False)
    assert torch.equal(trk.track(frames, points), torch.stack(want))
    assert trk.next_init.abs().max() == 0


# --------------------------------------------------------------------- track.py
def test_track_cli_writes_csv(tmp_path):
    frames = sorted(glob.glob(os.path.join(ROOT, "demo-frames", "*.png")))
    assert len(frames) >= 2
    (tmp_path / "points.txt").write_text("100 50\n400.5 300\n900 20.25\n512 218\n")
    out = tmp_path / "tracks.csv"
    res = subprocess.run([sys.executable, os.path.join(ROOT, "track.py"), "--small", "--iters", "2",
                          "--path", os.path.join(ROOT, "demo-frames"), "--points", str(tmp_path / "points.txt"),
                          "--out", str(out), "--model", str(tmp_path / "missing.pth"), "--random_init"],
                         env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-2000:]
    rows = out.read_text().strip().splitlines()
    assert rows[0] == "frame,point,x,y"
    body = np.array([[float(v) for v in r.split(",")] for r in rows[1:]])
    assert body.shape == (len(frames) * 4, 4) and np.isfinite(body).all()
    assert body[:4, 2:].tolist() == [[100, 50], [400.5, 300], [900, 20.25], [512, 218]]
    assert sorted(set(body[:, 0])) == list(range(len(frames))) and sorted(set(body[:, 1])) == [0, 1, 2, 3]

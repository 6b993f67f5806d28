"""Multi-delta tracking on the CPU: the ATen oracle of
ops.multi_flow_track_points on hand-worked cases, the eager MultiFlowTracker
on an occlusion scenario with a stub model and against SequenceTracker, its
argument checks, and track.py --deltas."""
import glob
import os
import subprocess
import sys

import pytest
import torch

from raft_stir_amd import ops
from raft_stir_amd.export.multiflow import MultiFlowTracker
from raft_stir_amd.export.pointtrack import SequenceTracker
from raft_stir_amd.ops import reference

import multi_flow_cases as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------- the oracle
def test_hand_worked_selection_cases():
    M.check_selection_cases(ops.multi_flow_track_points)
    assert len(M.selection_cases()) >= 12


def test_one_slot_is_fb_track_points():
    fw, bw, starts, score, vis = M.kernel_inputs(1, 70)
    got = ops.multi_flow_track_points(fw, bw, starts, score, vis, torch.ones(1, dtype=torch.bool), *M.FB.ALPHA)
    new, err, ok = reference.fb_track_points(fw, bw, starts, *M.FB.ALPHA)
    s = score + err
    assert M.same(got[0], new) and M.same(got[4], err) and M.same(got[5], err) and M.same(got[1], s)
    assert torch.equal(got[2], vis & ok & (s < M.INF)) and (got[3] == 0).all()
    assert got[2].any() and not got[2].all()


@pytest.mark.parametrize("K", [3, 16])
def test_kernel_inputs_show_every_outcome(K):
    """The inputs of the GPU kernel test, on the oracle alone: among 300 points
    some are chosen by score, some by a tie, some fall back, and without an
    active slot none is chosen."""
    fw, bw, starts, score, vis = M.kernel_inputs(K, 300)
    ok = torch.cat([reference.fb_track_points(fw[k:k + 1], bw[k:k + 1], starts[k:k + 1], *M.FB.ALPHA)[2]
                    for k in range(K)])
    assert ok.any() and not ok.all()
    masks = dict(M.active_masks(K))
    outs = ops.multi_flow_track_points(fw, bw, starts, score, vis, masks["mixed"], *M.FB.ALPHA)
    n = M.outcome_counts(outs, score, vis, masks["mixed"], ok)
    print(K, n)
    assert n["score"] >= 5 and n["tie"] >= 5 and n["fallback"] >= 5 and n["none"] == 0, n
    outs = ops.multi_flow_track_points(fw, bw, starts, score, vis, masks["none"], *M.FB.ALPHA)
    n = M.outcome_counts(outs, score, vis, masks["none"], ok)
    assert n == {"score": 0, "tie": 0, "fallback": 0, "none": 300}, n
    assert M.same(outs[0][0], starts[0]) and M.same(outs[1][0], score[0]) and (outs[4] == M.INF).all()


def test_wrapper_converts_and_checks():
    fw, bw, starts, score, vis = M.kernel_inputs(3, 16)
    act = torch.tensor([True, False, True])
    want = ops.multi_flow_track_points(fw, bw, starts, score, vis, act)
    got = ops.multi_flow_track_points(fw.double(), bw.permute(0, 1, 3, 2).contiguous().permute(0, 1, 3, 2),
                                      starts.double(), score.double(), vis, act)
    assert all(M.same(a, b) for a, b in zip(got, want))
    with pytest.raises(ValueError, match="same shape"):
        ops.multi_flow_track_points(fw, bw[..., :-1], starts, score, vis, act)
    with pytest.raises(ValueError, match=r"\(K,2,H,W\)"):
        ops.multi_flow_track_points(fw[0], bw[0], starts, score, vis, act)
    with pytest.raises(ValueError, match="slots"):
        ops.multi_flow_track_points(*(t.repeat(6, *[1] * (t.dim() - 1)) for t in (fw, bw, starts, score, vis, act)))
    with pytest.raises(ValueError, match=r"\(K,N,2\)"):
        ops.multi_flow_track_points(fw, bw, starts[:2], score, vis, act)
    with pytest.raises(ValueError, match="start_score"):
        ops.multi_flow_track_points(fw, bw, starts, score[:, :-1], vis, act)
    with pytest.raises(ValueError, match="start_visible"):
        ops.multi_flow_track_points(fw, bw, starts, score, vis[:2], act)
    with pytest.raises(ValueError, match="active"):
        ops.multi_flow_track_points(fw, bw, starts, score, vis, act[:2])
    for a in ((-0.1, 0.5), (0.01, float("inf")), (float("nan"), 0.5)):
        with pytest.raises(ValueError, match="alpha"):
            ops.multi_flow_track_points(fw, bw, starts, score, vis, act, *a)


# ------------------------------------------------------------------ the tracker
def test_occlusion_recovery_with_stub_model():
    frames, points = M.scenario()
    stub = M.StubSpanFlow()
    single = MultiFlowTracker(stub, iters=2, deltas=(1,)).track(frames, points)
    assert stub.calls == M.SC_T - 1
    multi_trk = MultiFlowTracker(stub, iters=2, deltas=(1, 2, None))
    multi = multi_trk.track(frames, points)
    M.check_scenario(single, multi, points)
    # the attributes of the last step
    h, w = M.SC_H // 8, M.SC_W // 8
    assert multi_trk.flow_up.shape == (3, 2, M.SC_H, M.SC_W) and multi_trk.flow_bw_up.shape == (3, 2, M.SC_H, M.SC_W)
    assert multi_trk.flow_low.shape == (3, 2, h, w) and multi_trk.flow_bw_low.shape == (3, 2, h, w)
    assert multi_trk.flow_init.shape == (6, 2, h, w) and multi_trk.next_init.shape == (6, 2, h, w)
    assert multi_trk.cand_err.shape == (3, 4) and multi_trk.fb_err.shape == (1, 4)
    assert torch.equal(multi_trk.fb_err[0], multi_trk.cand_err[0])  # every point chose slot 0 (span 1) at the end


def test_warm_start_rule_and_first_active_step():
    """next_init of every slot by the rule of the docstring; a slot's first
    active step starts from zeros; without warm_start every step does."""
    frames, points = M.scenario()
    trk = MultiFlowTracker(M.StubSpanFlow(), iters=2, deltas=(1, 2, 4, None))
    K, deltas = 4, (1, 2, 4, None)
    trk.step(frames[0], points)
    assert (trk.next_init == 0).all() and trk.next_init.shape == (8, 2, 6, 8)
    carried = trk.next_init.clone()
    for t in range(1, 7):
        trk.step(frames[t])
        assert torch.equal(trk.flow_init, carried), t
        lo = torch.cat([trk.flow_low, trk.flow_bw_low])
        for k, d in enumerate(deltas):
            active = t >= (d or 1)
            for g, j in ((1.0, k), (-1.0, K + k)):
                if t == (d or 1):
                    assert (trk.flow_init[j] == 0).all(), (t, k)  # the first active step
                if not active:
                    want = torch.zeros_like(lo[j:j + 1])
                elif d is None:
                    want = lo[j:j + 1]
                else:
                    want = (g * d) * ops.forward_interpolate(lo[j:j + 1] / (g * d))
                assert torch.equal(trk.next_init[j:j + 1], want), (t, k, g)
        carried = trk.next_init.clone()
    assert carried.abs().max() > 0
    cold = MultiFlowTracker(M.StubSpanFlow(), iters=2, deltas=(1, None), warm_start=False)
    cold.track(frames[:4], points)
    assert (cold.flow_init == 0).all() and (cold.next_init == 0).all()


def test_single_delta_is_the_sequence_tracker():
    """deltas=(1,): positions and fb_err of SequenceTracker(fb_check=True) at
    every frame, and its visibility as a running AND."""
    frames, points = M.scenario()
    seq = SequenceTracker(M.StubSpanFlow(), iters=2, fb_check=True)
    want, want_vis, want_err = seq.track(frames, points, return_visibility=True)
    trk = MultiFlowTracker(M.StubSpanFlow(), iters=2, deltas=(1,))
    running = torch.ones(4, dtype=torch.bool)
    for t in range(M.SC_T):
        got = trk.step(frames[t], points if t == 0 else None)
        running = running & want_vis[t]
        assert torch.equal(got[0], want[t]) and M.same(trk.fb_err[0], want_err[t]), t
        assert torch.equal(trk.visible[0], running), t
    assert not running.all() and running.any()
    assert torch.equal(trk.next_init, torch.cat([seq.next_init, seq.next_bw_init]))  # the warm start, bit for bit


def test_argument_checks_and_reset():
    stub = M.StubSpanFlow()
    for bad in ((), (0,), (2, 1), (1, 1), (None, 1), (1, None, None), (1.5,), (True,), tuple(range(1, 18)), 3, ("1",)):
        with pytest.raises(ValueError, match="deltas"):
            MultiFlowTracker(stub, deltas=bad)
    with pytest.raises(ValueError, match="fb_alpha"):
        MultiFlowTracker(stub, fb_alpha=(-1.0, 0.5))
    assert MultiFlowTracker(stub, deltas=[None]).deltas == (None,)
    assert MultiFlowTracker(stub, deltas=tuple(range(1, 16)) + (None,)).K == 16
    frames, points = M.scenario()
    trk = MultiFlowTracker(stub, iters=2, deltas=(1, 2, None))
    with pytest.raises(ValueError, match="needs points"):
        trk.step(frames[0])
    with pytest.raises(ValueError, match=r"\(1,N,2\)"):
        trk.step(frames[0], points[0])
    with pytest.raises(ValueError, match=r"\(1,3,H,W\)"):
        trk.step(frames[0][0], points)
    with pytest.raises(ValueError, match="multiples of 8"):
        trk.step(frames[0][..., :60], points)
    trk.step(frames[0], points)
    with pytest.raises(ValueError, match="shape changed"):
        trk.step(frames[1][..., :56])
    with pytest.raises(ValueError, match="first frame"):
        trk.step(frames[1], points)
    traj, vis, score, delta = trk.track(frames[:3], points)
    assert traj.shape == (3, 4, 2) and vis.shape == (3, 4) and score.shape == (3, 4) and delta.shape == (3, 4)
    traj, vis, score, delta = trk.track(list(frames[:2]), points[:, :1])
    assert traj.shape == (2, 1, 2) and delta.shape == (2, 1)
    with pytest.raises(ValueError, match="at least one frame"):
        trk.track([], points)
    trk.reset()
    assert trk.points is None and trk.visible is None and trk.score is None and trk.delta is None
    assert trk.flow_up is None and trk.next_init is None and trk.t == 0
    with pytest.raises(ValueError, match="needs points"):
        trk.step(frames[0])
    # a second sequence on the same tracker is the first one again
    a = trk.track(frames, points)
    b = trk.track(frames, points)
    assert all(M.same(x, y) for x, y in zip(a, b))


# --------------------------------------------------------------------- track.py
def _run_track(tmp_path, extra):
    (tmp_path / "points.txt").write_text("100 50\n400.5 300\n900 20.25\n")
    out = tmp_path / "tracks.csv"
    res = subprocess.run([sys.executable, os.path.join(ROOT, "track.py"), "--small", "--iters", "2",
                          "--path", os.path.join(ROOT, "demo-frames"), "--points", str(tmp_path / "points.txt"),
                          "--out", str(out), "--model", str(tmp_path / "missing.pth"), "--random_init"] + extra,
                         env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True, timeout=900)
    assert res.returncode == 0, res.stderr[-2000:]
    return out.read_text().strip().splitlines()


def test_track_cli_deltas_columns(tmp_path):
    frames = sorted(glob.glob(os.path.join(ROOT, "demo-frames", "*.png")))
    rows = _run_track(tmp_path, ["--deltas", "1", "2", "inf", "--fb_alpha", "0.02", "1.0"])
    assert rows[0] == "frame,point,x,y,fb_err,visible,score,delta"
    assert len(rows) == 1 + 3 * len(frames)
    assert rows[1] == "0,0,100.0000,50.0000,0.0000,1,0.0000,0"
    spans = set()
    for r in rows[4:]:
        cells = r.split(",")
        assert len(cells) == 8 and cells[5] in ("0", "1") and float(cells[4]) >= 0
        assert (cells[5] == "1") == (float(cells[6]) < M.INF)
        spans.add(int(cells[7]))
    assert spans <= {0, 1, 2}


def test_track_cli_without_deltas_is_unchanged(tmp_path):
    frames = sorted(glob.glob(os.path.join(ROOT, "demo-frames", "*.png")))
    rows = _run_track(tmp_path, [])
    assert rows[0] == "frame,point,x,y" and len(rows) == 1 + 3 * len(frames)
    assert all(len(r.split(",")) == 4 for r in rows)

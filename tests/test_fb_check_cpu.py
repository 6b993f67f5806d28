"""Forward-backward check on the CPU: the fp32 ATen oracles of fb_consistency
and fb_track_points against their fp64 form and hand-worked cases, the
bidirectional RAFT pass on the module path, SequenceTracker(fb_check=True)
with a stub model, and track.py --fb_check."""
import glob
import os
import subprocess
import sys

import pytest
import torch

from raft_stir_amd import ops
from raft_stir_amd.config import make_args
from raft_stir_amd.export.pointtrack import SequenceTracker
from raft_stir_amd.models import RAFT

import fb_check_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------ oracle fp32 / fp64
@pytest.mark.parametrize("shape", C.DENSE_SHAPES)
def test_dense_oracle_against_fp64(shape):
    """Measured maximum of |err - err64|: 2.30 * 2^-24 * M (bound 32), at most
    0.21 % of the pixels in the threshold band (bound 1 %)."""
    B, H, W = shape
    fw, bw = C.flow_pair(B, H, W)
    err, ok = ops.fb_consistency(fw, bw)
    C.check_dense(f"dense{shape}", fw, bw, err, ok)
    again = ops.fb_consistency(fw, bw)
    assert C.same(again[0], err) and torch.equal(again[1], ok)
    if B == 2:  # batch images are independent
        one = ops.fb_consistency(fw[:1], bw[:1])
        assert torch.equal(one[0], err[:1]) and torch.equal(one[1], ok[:1])


@pytest.mark.parametrize("N", C.POINT_COUNTS)
def test_points_oracle_against_fp64(N):
    """Measured maximum error of new_points and err: 5.77 * 2^-24 * M (bound
    32), 2 of 2000 points in the threshold band; against points + sample_points
    at most 4.8e-6 (tolerance 1.07e-4)."""
    B, H, W = C.POINT_SHAPE
    fw, bw = C.flow_pair(B, H, W)
    pts = C.points_for(N)
    new, err, ok = ops.fb_track_points(fw, bw, pts)
    C.check_points(f"points{N}", fw, bw, pts, new, err, ok)
    again = ops.fb_track_points(fw, bw, pts)
    assert all(C.same(a, b) for a, b in zip(again, (new, err, ok)))
    one = ops.fb_track_points(fw[:1], bw[:1], pts[:1])
    assert all(C.same(a, b[:1]) for a, b in zip(one, (new, err, ok)))
    _, count = C.check_against_sample_points(f"points{N}", fw, pts, new)
    assert N < 16 or count >= N  # most of the 2N points start inside the image


def test_hand_worked_edge_cases():
    C.check_edge_cases(ops.fb_consistency, ops.fb_track_points)


def test_wrappers_convert_and_check():
    fw, bw = C.flow_pair(1, 16, 20)
    pts = C.points_for(16)[:1] * 0.25
    want = ops.fb_track_points(fw, bw, pts)
    got = ops.fb_track_points(fw.permute(0, 1, 3, 2).contiguous().permute(0, 1, 3, 2), bw.double(), pts.double())
    assert all(C.same(a, b) for a, b in zip(got, want))
    h = ops.fb_consistency(fw.bfloat16(), bw.bfloat16())
    w = ops.fb_consistency(fw.bfloat16().float(), bw.bfloat16().float())
    assert h[0].dtype == torch.float32 and C.same(h[0], w[0]) and torch.equal(h[1], w[1])
    with pytest.raises(ValueError, match="same shape"):
        ops.fb_consistency(fw, bw[..., :-1])
    with pytest.raises(ValueError, match=r"\(B,2,H,W\)"):
        ops.fb_consistency(fw[0], bw[0])
    with pytest.raises(ValueError, match="H, W >= 2"):
        ops.fb_consistency(fw[:, :, :1], bw[:, :, :1])
    with pytest.raises(ValueError, match="alpha"):
        ops.fb_consistency(fw, bw, -0.1, 0.5)
    with pytest.raises(ValueError, match=r"\(B,N,2\)"):
        ops.fb_track_points(fw, bw, pts[0])
    with pytest.raises(ValueError, match=r"\(B,N,2\)"):
        ops.fb_track_points(fw, bw, torch.cat([pts, pts]))


# ------------------------------------------------------------ bidirectional pass
@pytest.fixture(scope="module")
def pair():
    g = torch.Generator().manual_seed(7)
    return torch.rand(1, 3, 128, 160, generator=g) * 255, torch.rand(1, 3, 128, 160, generator=g) * 255


@pytest.mark.parametrize("alternate_corr", [False, True])
def test_bidirectional_matches_batched_pairs(pair, alternate_corr):
    """Module path.  Both sides run the same ATen ops on every sample (instance
    norm and eval-mode batch norm are per sample); only the batch the
    convolutions see differs (the feature encoder gets 2 images here and 4 in
    the batched call), and the CPU convolution may block its sums differently
    with the batch.  The outputs are therefore compared at 1e-4 (absolute and
    relative, flows of a few pixels), a hundred fp32 roundings of the largest
    flow, far below the 2e-3 the GPU comparison of two kernel sets uses.
    Measured: bit-equal (maximum difference 0.0) with the ATen build this was
    written against."""
    a, b = pair
    torch.manual_seed(0)
    model = RAFT(make_args(small=True, alternate_corr=alternate_corr)).eval()
    g = torch.Generator().manual_seed(1)
    init = torch.randn(2, 2, 16, 20, generator=g)
    with torch.no_grad():
        for fi in (None, init):
            lo, up = model(a, b, iters=2, flow_init=fi, test_mode=True, bidirectional=True)
            wlo, wup = model(torch.cat([a, b]), torch.cat([b, a]), iters=2, flow_init=fi, test_mode=True)
            assert lo.shape == (2, 2, 16, 20) and up.shape == (2, 2, 128, 160)
            torch.testing.assert_close(lo, wlo, atol=1e-4, rtol=1e-4)
            torch.testing.assert_close(up, wup, atol=1e-4, rtol=1e-4)
            # [:B] is today's forward call
            flo, fup = model(a, b, iters=2, flow_init=None if fi is None else fi[:1], test_mode=True)
            torch.testing.assert_close(up[:1], fup, atol=1e-4, rtol=1e-4)
            torch.testing.assert_close(lo[:1], flo, atol=1e-4, rtol=1e-4)
        assert (up[0] - up[1]).abs().max() > 1e-3  # two directions, not one twice


def test_bidirectional_argument_checks(pair):
    a, b = pair
    torch.manual_seed(0)
    model = RAFT(make_args(small=True)).eval()
    with torch.no_grad():
        with pytest.raises(ValueError, match="test_mode"):
            model(a, b, iters=1, bidirectional=True)
        with pytest.raises(ValueError, match="shape"):
            model(a, b[..., :152], iters=1, test_mode=True, bidirectional=True)
    with pytest.raises(ValueError, match="no_grad"):
        model(a, b, iters=1, test_mode=True, bidirectional=True)


# ---------------------------------------------------------- tracker, stub model
def test_tracker_with_stub_model():
    frames, points = C.stub_sequence()
    model = C.StubFlow()
    trk = SequenceTracker(model, iters=2, warm_start=True, fb_check=True)
    traj, vis, err = trk.track(frames, points, return_visibility=True)
    C.check_stub_tracking(traj, vis, err, points)
    assert model.calls == 3
    # stepping by hand: the per-step attributes
    trk.reset()
    assert torch.equal(trk.step(frames[0], points), points)
    assert trk.visible.shape == (1, 5) and trk.visible.all() and (trk.fb_err == 0).all()
    assert trk.fb_err.shape == (1, 5) and (trk.next_init == 0).all() and (trk.next_bw_init == 0).all()
    d = torch.tensor(C.STUB_D).view(1, 2, 1, 1)
    for t in range(1, 4):
        trk.step(frames[t])
        assert torch.equal(trk.visible[0], vis[t]) and C.same(trk.fb_err[0], err[t])
        assert trk.flow_up.shape == (1, 2, 64, 128) and trk.flow_bw_up.shape == (1, 2, 64, 128)
        assert trk.flow_low.shape == (1, 2, 8, 16) and trk.flow_bw_low.shape == (1, 2, 8, 16)
        assert trk.flow_init.shape == (1, 2, 8, 16) and trk.flow_bw_init.shape == (1, 2, 8, 16)
        assert torch.equal(trk.flow_up, d.expand(1, 2, 64, 128))
        assert torch.equal(trk.next_init, ops.forward_interpolate(trk.flow_low))
        assert torch.equal(trk.next_bw_init, -ops.forward_interpolate(-trk.flow_bw_low))
    err_map, ok_map = trk.fb_map()
    want = ops.fb_consistency(trk.flow_up, trk.flow_bw_up)
    assert C.same(err_map, want[0]) and torch.equal(ok_map, want[1])
    y0, y1, x0, x1 = C.STUB_RECT
    assert not ok_map[0, 0, y0 + 2:y1, x0:x1 - 3].any() and ok_map[0, 0, 2:y0 + 2, :x0 - 3].all()


def test_tracker_visibility_needs_fb_check():
    frames, points = C.stub_sequence()
    trk = SequenceTracker(C.StubFlow(), iters=2)
    assert trk.fb_check is False
    with pytest.raises(ValueError, match="fb_check"):
        trk.track(frames, points, return_visibility=True)
    with pytest.raises(ValueError, match="fb_check"):
        trk.fb_map()
    with pytest.raises(ValueError, match="fb_alpha"):
        SequenceTracker(C.StubFlow(), fb_check=True, fb_alpha=(-1.0, 0.5))


def test_tracker_real_model_matches_hand_written_loop():
    """SequenceTracker(fb_check=True) on the CPU is the loop of its docstring."""
    g = torch.Generator().manual_seed(5)
    frames = torch.rand(3, 1, 3, 128, 160, generator=g) * 255
    points = torch.rand(1, 8, 2, generator=g) * torch.tensor([159.0, 127.0])
    torch.manual_seed(0)
    model = RAFT(make_args(small=True)).eval()
    trk = SequenceTracker(model, iters=2, fb_check=True, fb_alpha=(0.02, 1.0))
    traj, vis, err = trk.track(frames, points, return_visibility=True)
    pts, init = points, torch.zeros(2, 2, 16, 20)
    sgn = torch.tensor([1.0, -1.0]).view(2, 1, 1, 1)
    with torch.no_grad():
        for t in range(1, 3):
            lo, up = model(frames[t - 1], frames[t], iters=2, flow_init=init, test_mode=True, bidirectional=True)
            pts, e, k = ops.fb_track_points(up[:1], up[1:], pts, 0.02, 1.0)
            init = sgn * ops.forward_interpolate(sgn * lo)
            assert torch.equal(traj[t], pts[0]) and C.same(err[t], e[0]) and torch.equal(vis[t], k[0])
    assert torch.equal(trk.next_init, init[:1]) and torch.equal(trk.next_bw_init, init[1:])
    assert init.abs().max() > 0


# --------------------------------------------------------------------- track.py
@pytest.mark.parametrize("fb_check", [False, True])
def test_track_cli_fb_check_columns(tmp_path, fb_check):
    frames = sorted(glob.glob(os.path.join(ROOT, "demo-frames", "*.png")))
    (tmp_path / "points.txt").write_text("100 50\n400.5 300\n900 20.25\n")
    out = tmp_path / "tracks.csv"
    res = subprocess.run([sys.executable, os.path.join(ROOT, "track.py"), "--small", "--iters", "2",
                          "--path", os.path.join(ROOT, "demo-frames"), "--points", str(tmp_path / "points.txt"),
                          "--out", str(out), "--model", str(tmp_path / "missing.pth"), "--random_init"]
                         + (["--fb_check", "--fb_alpha", "0.02", "1.0"] if fb_check else []),
                         env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-2000:]
    rows = out.read_text().strip().splitlines()
    assert len(rows) == 1 + 3 * len(frames)
    if not fb_check:
        assert rows[0] == "frame,point,x,y"
        assert all(len(r.split(",")) == 4 for r in rows)
        return
    assert rows[0] == "frame,point,x,y,fb_err,visible"
    assert rows[1] == "0,0,100.0000,50.0000,0.0000,1"
    assert all(r.endswith(",0.0000,1") for r in rows[1:4])
    for r in rows[4:]:
        cells = r.split(",")
        assert len(cells) == 6 and cells[5] in ("0", "1") and float(cells[4]) >= 0

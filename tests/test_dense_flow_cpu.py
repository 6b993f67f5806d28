"""Dense every-pixel tracking on the CPU: the ATen oracle of
ops.dense_multi_flow_step against the point form at every pixel, the eager
DenseMultiFlowTracker against MultiFlowTracker on all pixel centres and on the
occlusion scenario, query(), the argument checks and track.py --dense."""
import glob
import os
import sys

import numpy as np
import pytest
import torch

from raft_stir_amd import ops
from raft_stir_amd.data.frame_utils import readFlow
from raft_stir_amd.export.denseflow import DenseMultiFlowTracker
from raft_stir_amd.export.multiflow import MultiFlowTracker
from raft_stir_amd.ops import reference

import dense_flow_cases as D
import multi_flow_cases as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = D.INF


# ------------------------------------------------------------------- the oracle
def test_oracle_is_the_point_form_at_every_pixel():
    """24x40, K = 3: bit equality with reference.multi_flow_track_points on
    the rows picked by hand, the ring row written, every other row untouched,
    and every outcome class present (the counts are asserted)."""
    H, W = D.CPU_HW
    K = 3
    fw, bw, ring_pos, ring_score, idx = D.step_inputs(K, H, W)
    start = ring_pos.index_select(0, idx[:K].long())
    assert (~torch.isfinite(start)).any() and ((start[:, 0] < 0) | (start[:, 0] > W - 1)).any()  # NaN, outside
    assert (ring_score == INF).any() and torch.isnan(ring_score).any()
    for name, act in M.active_masks(K) + D.single_masks(K):
        rp, rs = ring_pos.clone(), ring_score.clone()
        got = ops.dense_multi_flow_step(fw, bw, rp, rs, idx, act, *D.FB.ALPHA, cand_err=True)
        want, (wp, ws), sscore = D.point_form(fw, bw, ring_pos, ring_score, idx, act)
        assert got[0].shape == (1, 2, H, W) and got[5].shape == (K, H, W)
        assert got[2].dtype == torch.bool and got[3].dtype == torch.int32
        for key, g, w in zip(D.NAMES, got, want):
            assert D.same(g, w), f"{name}: {key} differs at {int((g != w).sum())} places"
        assert D.same(rp, wp) and D.same(rs, ws), name
        dst = int(idx[K])
        assert D.same(rp[dst], got[0][0]) and D.same(rs[dst], got[1][0, 0]), name
        others = [r for r in range(K + 2) if r != dst]
        assert D.same(rp[others], ring_pos[others]) and D.same(rs[others], ring_score[others]), name
        assert torch.equal(got[2], got[1] < INF), name  # a stored score is finite iff visible
        assert ops.dense_multi_flow_step(fw, bw, rp.clone(), rs.clone(), idx, act, *D.FB.ALPHA)[5] is None
        n = D.outcome_counts(got, sscore, act, fw, bw, ring_pos, idx)
        print(name, n)
        if name == "mixed":
            assert not act.all() and act.any()
            assert n["score"] >= 5 and n["tie"] >= 5 and n["fallback"] >= 5 and n["none"] == 0, n
        if name == "none":
            assert n == {"score": 0, "tie": 0, "fallback": 0, "none": H * W}, n
            src0 = int(idx[0])
            assert D.same(got[0][0], ring_pos[src0]) and (got[1] == INF).all() and (got[4] == INF).all()


def test_oracle_clamps_and_ignores_a_source_that_is_written():
    H, W = 7, 9
    K, R = 3, 5
    fw, bw, ring_pos, ring_score, idx = D.step_inputs(K, H, W)
    act = torch.ones(K, dtype=torch.bool)

    def run(i, a=act):
        rp, rs = ring_pos.clone(), ring_score.clone()
        return ops.dense_multi_flow_step(fw, bw, rp, rs, torch.tensor(i, dtype=torch.int32), a, cand_err=True), rp, rs

    wild, wp, ws = run([-5, 1, R + 7, 2])
    clamped, cp, cs = run([0, 1, R - 1, 2])
    assert all(D.same(a, b) for a, b in zip(wild, clamped)) and D.same(wp, cp) and D.same(ws, cs)
    wild, wp, ws = run([0, 1, 2, R + 7])
    assert D.same(wp[:R - 1], ring_pos[:R - 1]) and D.same(wp[R - 1], wild[0][0])
    same_row, _, _ = run([0, 3, 2, 3])
    off, _, _ = run([0, 3, 2, 3], torch.tensor([True, False, True]))
    assert all(D.same(a, b) for a, b in zip(same_row[:5], off[:5]))
    assert (same_row[3] != 1).all()


def test_wrapper_converts_and_checks():
    K, (H, W) = 3, (7, 9)
    fw, bw, ring_pos, ring_score, idx = D.step_inputs(K, H, W)
    act = torch.tensor([True, False, True])

    def call(fw=fw, bw=bw, rp=ring_pos, rs=ring_score, idx=idx, act=act, alpha=(0.01, 0.5)):
        return ops.dense_multi_flow_step(fw, bw, rp.clone(), rs.clone(), idx, act, *alpha)

    want = call()
    got = call(fw=fw.double(), bw=bw.permute(0, 1, 3, 2).contiguous().permute(0, 1, 3, 2))
    assert all(D.same(a, b) for a, b in zip(got[:5], want[:5]))
    with pytest.raises(ValueError, match="same shape"):
        call(bw=bw[..., :-1])
    with pytest.raises(ValueError, match=r"\(K,2,H,W\)"):
        call(fw=fw[0], bw=bw[0])
    with pytest.raises(ValueError, match="slots"):
        call(fw=fw.repeat(6, 1, 1, 1), bw=bw.repeat(6, 1, 1, 1))
    with pytest.raises(ValueError, match="H, W >= 2"):
        call(fw=fw[:, :, :1], bw=bw[:, :, :1])
    with pytest.raises(ValueError, match="ring_pos"):
        call(rp=ring_pos[:, :, :-1])
    with pytest.raises(ValueError, match="R >= 2"):
        call(rp=ring_pos[:1], rs=ring_score[:1])
    with pytest.raises(ValueError, match="ring_score"):
        call(rs=ring_score[:-1])
    with pytest.raises(ValueError, match="contiguous fp32"):
        call(rp=ring_pos.double())
    with pytest.raises(ValueError, match="idx"):
        call(idx=idx[:-1])
    with pytest.raises(ValueError, match="idx"):
        call(idx=idx.long())
    with pytest.raises(ValueError, match="active"):
        call(act=act[:2])
    for a in ((-0.1, 0.5), (0.01, float("inf")), (float("nan"), 0.5)):
        with pytest.raises(ValueError, match="alpha"):
            call(alpha=a)


# ------------------------------------------------------------------ the tracker
@pytest.mark.parametrize("cache_features", [False, True])
@pytest.mark.parametrize("deltas", [(1,), (2, 4), (1, 3, None)])
def test_tracker_is_the_point_tracker_at_every_pixel(deltas, cache_features):
    """2L + 3 frames: the steps before every slot is active and the ring's
    wrap-around are among them."""
    L = max(d for d in deltas if d is not None)
    frames = D.frames(2 * L + 3)
    points = D.pixel_centres(M.SC_H, M.SC_W)
    dense = DenseMultiFlowTracker(D.StubWobble(), iters=2, deltas=deltas, cache_features=cache_features)
    sparse = MultiFlowTracker(D.StubWobble(), iters=2, deltas=deltas, cache_features=cache_features)
    seen_lost = seen_found = False
    spans = set()
    for t in range(len(frames)):
        pos = dense.step(frames[t])
        want = sparse.step(frames[t], points if t == 0 else None)
        assert pos.shape == (1, 2, M.SC_H, M.SC_W) and pos is dense.pos
        assert D.same(D.as_points(dense)[0], want), t
        for name, a, b in zip(("pos", "visible", "score", "fb_err", "delta"), D.as_points(dense), D.of_points(sparse)):
            assert D.same(a, b), (t, name)
        assert D.same(dense.flow, dense.pos - reference.coords_grid(1, M.SC_H, M.SC_W))
        assert D.same(dense.next_init, sparse.next_init) and (t == 0 or D.same(dense.flow_up, sparse.flow_up))
        seen_lost |= bool((~dense.visible).any())
        seen_found |= bool(dense.visible.any()) and t > 0
        spans |= set(dense.delta.unique().tolist())
    assert seen_lost and seen_found
    if deltas == (1, 3, None):
        assert spans == {0, 1, 3}, spans  # every slot is chosen somewhere
    assert dense.points is None and dense.cand_err is None
    assert list(dense.graphs) == [((1, 3, M.SC_H, M.SC_W), deltas) + (("cache_features",) if cache_features else ())]


def test_first_step_and_track():
    frames = D.frames(4)
    trk = DenseMultiFlowTracker(D.StubWobble(), iters=2, deltas=(1, None), cand_err=True)
    grid = reference.coords_grid(1, M.SC_H, M.SC_W)
    pos = trk.step(frames[0])
    assert D.same(pos, grid) and (trk.flow == 0).all() and trk.visible.all() and (trk.score == 0).all()
    assert (trk.fb_err == 0).all() and (trk.delta == 0).all() and trk.delta.dtype == torch.int32
    assert trk.visible.shape == trk.score.shape == trk.fb_err.shape == trk.delta.shape == (1, 1, M.SC_H, M.SC_W)
    trk.step(frames[1])
    assert trk.cand_err.shape == (2, M.SC_H, M.SC_W)
    flows, vis = trk.track(frames)
    assert flows.shape == (4, 2, M.SC_H, M.SC_W) and vis.shape == (4, 1, M.SC_H, M.SC_W) and vis.dtype == torch.bool
    assert (flows[0] == 0).all() and vis[0].all() and flows[1:].abs().max() > 1
    again = trk.track(list(frames))
    assert D.same(again[0], flows) and torch.equal(again[1], vis)
    with pytest.raises(ValueError, match="at least one frame"):
        trk.track([])


def test_query():
    frames = D.frames(6)
    trk = DenseMultiFlowTracker(D.StubWobble(), iters=2, deltas=(1, 2, None))
    with pytest.raises(ValueError, match="needs a step"):
        trk.query(torch.zeros(1, 1, 2))
    for t in range(6):
        trk.step(frames[t])
    H, W = M.SC_H, M.SC_W
    vis = trk.visible[0, 0]
    assert vis.any() and not vis.all()
    # integer points: the stored pixel, bit for bit
    pts, v, s = trk.query(D.pixel_centres(H, W))
    assert D.same(pts, D.as_points(trk)[0]) and torch.equal(v, trk.visible.view(1, -1))
    assert D.same(s, trk.score.view(1, -1))
    # half-way between a visible pixel and a lost one to its right: not visible, the worse score
    edge = (vis[:, :-1] & ~vis[:, 1:]).nonzero()
    assert len(edge) >= 1
    y, x = (int(c) for c in edge[0])
    half = torch.tensor([[[x + 0.5, float(y)], [x + 0.25, float(y)], [float(x), float(y)]]])
    pts, v, s = trk.query(half)
    assert v.tolist() == [[False, False, True]] and s[0, 0] == INF and s[0, 2] == trk.score[0, 0, y, x]
    a, b = trk.pos[0, :, y, x], trk.pos[0, :, y, x + 1]
    assert D.same(pts[0, 0], 0.5 * a + 0.5 * b)
    # between two visible pixels, one above the other: visible, the larger score, the weighted position
    both = (vis[:-1] & vis[1:]).nonzero()
    y, x = (int(c) for c in both[len(both) // 2])
    pts, v, s = trk.query(torch.tensor([[[float(x), y + 0.25]]]))
    assert bool(v[0, 0]) and s[0, 0] == max(trk.score[0, 0, y, x], trk.score[0, 0, y + 1, x])
    assert D.same(pts[0, 0], 0.75 * trk.pos[0, :, y, x] + 0.25 * trk.pos[0, :, y + 1, x])
    # the last row and column are inside; outside and non-finite points come back as they are
    far = torch.tensor([[[W - 1.0, H - 1.0], [W - 0.5, 3.0], [-0.25, 3.0], [5.0, float(H)], [D.NAN, 2.0], [INF, 2.0],
                         [3.0, -INF]]])
    pts, v, s = trk.query(far)
    assert D.same(pts[0, 0], trk.pos[0, :, H - 1, W - 1]) and bool(v[0, 0]) == bool(vis[H - 1, W - 1])
    assert D.same(pts[0, 1:], far[0, 1:]) and not v[0, 1:].any() and (s[0, 1:] == INF).all()
    with pytest.raises(ValueError, match=r"\(1,N,2\)"):
        trk.query(torch.zeros(4, 2))


def test_recovery_after_an_occlusion():
    """The occlusion scenario of the multi-delta tests, every pixel: pixels
    that stay under the occluder's rectangle are lost while it is there; with
    a longer span and the anchor they are found again where they truly are,
    with deltas=(1,) they are not.  Pixels that never meet it stay exact."""
    frames, points = M.scenario()
    d, drift = torch.tensor(M.SC_D).view(2, 1, 1), torch.tensor(M.SC_DRIFT).view(2, 1, 1)
    under = (slice(9, 19), slice(9, 25))    # y, x: inside SC_RECT for all 8 frames, drifted or not
    clear = (slice(34, 39), slice(2, 41))   # below it, inside the image for all 8 frames
    grid = reference.coords_grid(1, M.SC_H, M.SC_W)[0]
    single = DenseMultiFlowTracker(M.StubSpanFlow(), iters=2, deltas=(1,))
    multi = DenseMultiFlowTracker(M.StubSpanFlow(), iters=2, deltas=(1, 2, None))
    sparse = MultiFlowTracker(M.StubSpanFlow(), iters=2, deltas=(1, 2, None)).track(frames, points)
    first_clear = M.SC_OCCLUDED[1] + 1
    for t in range(M.SC_T):
        for name, trk in (("single", single), ("multi", multi)):
            pos = trk.step(frames[t])[0]
            vis, score, delta = trk.visible[0, 0], trk.score[0, 0], trk.delta[0, 0]
            assert torch.equal(pos[(slice(None),) + clear], (grid + t * d)[(slice(None),) + clear]), (name, t)
            assert vis[clear].all() and (score[clear] == 0).all(), (name, t)
            if t in M.SC_OCCLUDED:
                assert not vis[under].any() and (score[under] == INF).all(), (name, t)
            elif t < M.SC_OCCLUDED[0]:
                assert vis[under].all(), (name, t)
            elif name == "multi":
                assert vis[under].all() and (score[under] == 0).all(), t
                assert torch.equal(pos[(slice(None),) + under], (grid + t * d)[(slice(None),) + under]), t
                assert (delta[under] == (0 if t == first_clear else 1)).all(), t
            else:
                assert not vis[under].any() and (delta[under] == 1).all(), t
                assert torch.equal(pos[(slice(None),) + under], (grid + t * d + 2 * drift)[(slice(None),) + under]), t
        # the scenario's own points, asked after the fact: MultiFlowTracker's answers
        pts, v, s = multi.query(points)
        assert torch.equal(pts[0], sparse[0][t]) and torch.equal(v[0], sparse[1][t]) and D.same(s[0], sparse[2][t]), t


def test_argument_checks():
    frames = D.frames(3)
    trk = DenseMultiFlowTracker(D.StubWobble(), iters=2, deltas=(1, None))
    with pytest.raises(ValueError, match="takes no points"):
        trk.step(frames[0], D.pixel_centres(M.SC_H, M.SC_W))
    assert trk.t == 0
    with pytest.raises(ValueError, match=r"\(1,3,H,W\)"):
        trk.step(frames[0][0])
    with pytest.raises(ValueError, match="multiples of 8"):
        trk.step(frames[0][..., :60])
    trk.step(frames[0])
    with pytest.raises(ValueError, match="takes no points"):
        trk.step(frames[1], torch.zeros(1, 1, 2))
    with pytest.raises(ValueError, match="shape changed"):
        trk.step(frames[1][..., :56])
    trk.step(frames[1])
    trk.reset()
    assert trk.pos is None and trk.flow is None and trk.visible is None and trk.t == 0
    with pytest.raises(ValueError, match="deltas"):
        DenseMultiFlowTracker(D.StubWobble(), deltas=(2, 1))
    with pytest.raises(ValueError, match="encode"):
        DenseMultiFlowTracker(M.StubSpanFlow(), cache_features=True)


# --------------------------------------------------------------------- track.py
@pytest.fixture(scope="module")
def cli():
    sys.path.insert(0, ROOT)
    try:
        import track
    finally:
        sys.path.remove(ROOT)
    return track


def test_track_cli_dense_arguments(cli, tmp_path):
    a = cli.parse_args(["--dense", "--deltas", "1", "2", "inf", "--out", str(tmp_path)])
    assert a.dense and a.points is None and cli._deltas(a.deltas) == (1, 2, None) and a.out == str(tmp_path)
    a = cli.parse_args(["--dense", "--deltas", "1", "--points", "p.txt"])
    assert a.dense and a.points == "p.txt"
    a = cli.parse_args(["--points", "p.txt"])
    assert not a.dense and a.deltas is None and a.out == "tracks.csv"
    for bad in (["--dense"], ["--dense", "--points", "p.txt"], [], ["--deltas", "1"]):
        with pytest.raises(SystemExit):
            cli.parse_args(bad)


def test_track_cli_dense_files(cli, tmp_path):
    """The three demo frames (436x1024, padded to 440x1024) through a stub
    model: per frame a .flo and a visibility image of the unpadded size, the
    flow between unpadded coordinates, and with --points the CSV from query()."""
    from PIL import Image
    images = sorted(glob.glob(os.path.join(ROOT, "demo-frames", "*.png")))
    assert len(images) == 3
    W, H = Image.open(images[0]).size
    assert H % 8 != 0  # the frames are padded
    (tmp_path / "points.txt").write_text("100 50\n400.5 300\n")
    out = tmp_path / "dense"
    args = cli.parse_args(["--dense", "--deltas", "1", "--points", str(tmp_path / "points.txt"),
                           "--out", str(out), "--iters", "2"])
    pts = np.loadtxt(args.points, dtype=np.float32, ndmin=2)
    traj = cli.track_dense(args, D.StubAny(), images, pts, torch.device("cpu"))
    dx, dy = D.FB.STUB_D
    for t in range(3):
        flow = readFlow(str(out / f"flow_{t:04d}.flo"))
        vis = np.asarray(Image.open(out / f"visible_{t:04d}.png"))
        assert flow.shape == (H, W, 2) and vis.shape == (H, W) and vis.dtype == np.uint8
        assert set(np.unique(vis)) <= {0, 255}
        seen = vis == 255
        assert seen[50, 100] and (flow[seen] == np.float32([dx * t, dy * t])).all()
        assert np.allclose(traj[t], pts + np.float32([dx * t, dy * t]))
    rows = (out / "tracks.csv").read_text().strip().splitlines()
    assert rows[0] == "frame,point,x,y,fb_err,visible,score,delta" and len(rows) == 1 + 3 * 2
    assert rows[1] == "0,0,100.0000,50.0000,0.0000,1,0.0000,0"
    assert rows[3].startswith(f"1,0,{100 + dx:.4f},{50 + dy:.4f},0.0000,1,0.0000,")
    # without --points: the fields alone
    out2 = tmp_path / "dense2"
    args = cli.parse_args(["--dense", "--deltas", "1", "inf", "--out", str(out2), "--iters", "2"])
    assert cli.track_dense(args, D.StubAny(), images, None, torch.device("cpu")) is None
    assert sorted(os.listdir(out2)) == [f"{n}_{t:04d}.{e}" for n, e in (("flow", "flo"), ("visible", "png"))
                                        for t in range(3)]

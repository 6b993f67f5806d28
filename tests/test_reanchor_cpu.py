"""DenseMultiFlowTracker.reanchor on the CPU, on stubs whose answer is known:
a re-anchored tracker against one that never re-anchors, bit for bit on an
integer translation and within the composition's rounding on a fractional one;
labels carried through re-anchors; the two policies; reset(); a tracker
without re-anchoring never calls the op; and track.py --dense --reanchor_every."""
import os
import sys

import numpy as np
import pytest
import torch

import dense_flow_cases as D
import forward_splat_cases as S

from raft_stir_amd import ops
from raft_stir_amd.export.denseflow import DenseMultiFlowTracker

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W, T = 24, 40, 9
SHIFT = (2.0, -1.0)
DELTAS = (1, 3, None)


def tracker(d=SHIFT, **kw):
    return DenseMultiFlowTracker(S.StubShift(d), iters=2, deltas=DELTAS, **kw)


def published(trk):
    return tuple(t.clone() for t in (trk.pos, trk.visible, trk.score, trk.delta, trk.fb_err))


def plain_run(d=SHIFT, frames=None):
    frames = D.frames(T, H, W) if frames is None else frames
    trk = tracker(d)
    out = []
    for t in range(len(frames)):
        trk.step(frames[t])
        out.append(published(trk))
    return out


def inside_after(k, d=SHIFT):
    """The pixels of a frame whose translation by k steps is still in the image."""
    ys, xs = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    x, y = xs + k * d[0], ys + k * d[1]
    return ((x >= 0) & (x <= W - 1) & (y >= 0) & (y <= H - 1)).view(1, 1, H, W)


def assert_same_track(got, want, based, t):
    pos, vis, score, delta, err = got
    wpos, wvis, wscore, wdelta, _ = want
    assert torch.equal(vis, wvis), t
    assert S.same(score, wscore), t
    v2 = vis.expand(1, 2, H, W)
    assert S.same(pos[v2], wpos[v2]), t
    assert torch.equal(delta[vis], wdelta[vis]), t
    assert torch.equal((delta >= 0)[vis], (wdelta >= 0)[vis]) and bool((delta[vis] >= 0).all()), t
    if based:
        # the rule of the composition: no span where the pixel is not visible
        assert bool((delta[~vis] == -1).all()) and bool((err[~vis] == float("inf")).all()), t
    else:
        assert torch.equal(delta >= 0, wdelta >= 0), t


@pytest.mark.parametrize("at", [(3,), (2, 5)], ids=lambda a: "at" + "_".join(map(str, a)))
def test_reanchored_tracker_is_the_plain_one_on_an_integer_translation(at):
    frames = D.frames(T, H, W)
    want = plain_run()
    trk = tracker()
    trk.reanchor()  # before any step: nothing
    assert trk.pos is None and trk.anchor_frame == 0
    anchor = 0
    for t in range(T):
        trk.step(frames[t])
        if t == 0:
            trk.reanchor()  # before the first advance: nothing
            assert trk.t == 1 and trk.anchor_frame == 0 and not trk._based
        assert_same_track(published(trk), want[t], anchor > 0, t)
        # pixels are lost exactly when they leave the image
        assert torch.equal(trk.visible, inside_after(t)), t
        assert trk.anchor_frame == anchor
        assert torch.equal(trk.anchor_visible, inside_after(t - anchor)), t
        grid = trk._st["grid"]
        av = trk.anchor_visible.expand(1, 2, H, W)
        moved = grid + (t - anchor) * torch.tensor(SHIFT).view(1, 2, 1, 1)
        assert torch.equal(trk.anchor_pos[av], moved[av]), t
        if t in at:
            before = published(trk)
            trk.reanchor()
            anchor = t
            assert trk.anchor_frame == t and trk.t == 1
            # what is published for the re-anchor frame stays, bit for bit
            assert all(S.same(a, b) for a, b in zip(published(trk), before))
            assert torch.equal(trk.anchor_pos, grid) and bool(trk.anchor_visible.all())
            assert bool((trk.anchor_score == 0).all())
            trk.reanchor()  # right after a re-anchor: nothing
            assert trk.anchor_frame == t
    assert not bool(trk.visible.all()) and bool(trk.visible.any())


def test_reanchor_every_is_the_plain_tracker_and_counts_from_the_anchor():
    frames = D.frames(T, H, W)
    want = plain_run()
    trk = tracker(reanchor_every=2)
    for t in range(T):
        out = trk.step(frames[t])
        assert out is trk.pos
        assert_same_track(published(trk), want[t], t > 2, t)
        assert trk.anchor_frame == t - t % 2, t  # re-anchored after publishing frames 2, 4, 6, ...
    for bad in (0, -1, 1.5, True):
        with pytest.raises(ValueError, match="reanchor_every"):
            tracker(reanchor_every=bad)
    for bad in (0.0, 1.0, -0.5, 2):
        with pytest.raises(ValueError, match="reanchor_below"):
            tracker(reanchor_below=bad)


def test_fractional_translation_agrees_within_the_roundings_of_the_composition():
    d = (1.5, -0.75)
    frames = D.frames(T, H, W)
    want = plain_run(d)
    trk = tracker(d)
    # four products and three sums, each rounded once, of coordinates no larger than the frame plus the way gone
    largest = max(H, W) + T * max(abs(v) for v in d)
    bound = 4 * float(np.spacing(np.float32(largest)))
    seen = 0
    for t in range(T):
        trk.step(frames[t])
        if t in (2, 5):
            trk.reanchor()
        both = (trk.visible & want[t][1]).expand(1, 2, H, W)
        seen += int(both.sum())
        assert float((trk.pos[both] - want[t][0][both]).abs().max()) <= bound, t
        # a pixel the composition sees is one the plain tracker sees
        assert not bool((trk.visible & ~want[t][1]).any()), t
    assert seen > T * H * W  # more than half of all coordinates were compared


def test_labels_are_carried_through_reanchors():
    frames = D.frames(T, H, W)
    lab = torch.randint(0, 7, (H, W), generator=torch.Generator().manual_seed(1), dtype=torch.uint8)
    flows, vis, warped, cov = tracker().track(frames, lab, footprint=1, fill=9)
    trk = tracker(reanchor_every=2)
    f2, v2, w2, c2 = trk.track(frames, lab, footprint=1, fill=9)
    assert torch.equal(v2, vis) and torch.equal(w2, warped) and torch.equal(c2, cov)
    seen = vis.expand(T, 2, H, W)
    assert torch.equal(f2[seen], flows[seen])
    assert trk.anchor_frame == T - 1 - (T - 1) % 2 > 0
    # and step by step, with in-painting
    plain = tracker()
    trk = tracker()
    for t in range(T):
        plain.step(frames[t])
        trk.step(frames[t])
        if t in (3, 4):
            trk.reanchor()
        for kw in (dict(footprint=2), dict(footprint=1, inpaint=2)):
            a, b = trk.warp_labels(lab, fill=9, **kw), plain.warp_labels(lab, fill=9, **kw)
            assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), (t, kw)


def test_reanchor_below_fires_on_the_frame_the_geometry_predicts():
    f = 0.8
    frames = D.frames(T, H, W)
    # k frames past an anchor, (W - k|dx|) * (H - k|dy|) of its pixels are still in the image
    k = next(k for k in range(1, T) if (W - k * abs(SHIFT[0])) * (H - k * abs(SHIFT[1])) < f * H * W)
    assert 1 < k and 2 * k < T  # it fires, not at once, and twice in the sequence
    want = plain_run()
    trk = tracker(reanchor_below=f)
    for t in range(T):
        trk.step(frames[t])
        assert trk.anchor_frame == t - t % k, t
        assert_same_track(published(trk), want[t], t > k, t)


def test_reset_forgets_the_base(monkeypatch):
    frames = D.frames(T, H, W)
    want = plain_run()
    trk = tracker()
    for t in range(4):
        trk.step(frames[t])
    trk.reanchor()
    trk.step(frames[4])
    assert trk._based and trk.anchor_frame == 3
    trk.reset()
    assert not trk._based and trk.anchor_frame == 0 and trk.anchor_pos is None and trk.pos is None

    def boom(*a, **k):
        raise AssertionError("dense_compose was called")
    monkeypatch.setattr(ops, "dense_compose", boom)
    for t in range(T):
        trk.step(frames[t])
        assert all(S.same(a, b) for a, b in zip(published(trk), want[t])), t
        assert trk.anchor_pos is trk.pos and trk.anchor_visible is trk.visible and trk.anchor_score is trk.score


def test_a_tracker_that_never_reanchors_never_calls_the_op(monkeypatch):
    calls = []
    real = ops.dense_compose

    def counted(*a, **k):
        calls.append(1)
        return real(*a, **k)
    monkeypatch.setattr(ops, "dense_compose", counted)
    frames = D.frames(T, H, W)
    trk = tracker()
    for t in range(T):
        trk.step(frames[t])
    assert calls == []
    trk.track(frames)
    assert calls == []
    trk.reanchor()
    assert calls == []  # the re-anchor frame itself is not recomposed
    trk.step(frames[0])
    assert calls == [1]


# --------------------------------------------------------------------- track.py
@pytest.fixture(scope="module")
def cli():
    sys.path.insert(0, ROOT)
    try:
        import track
    finally:
        sys.path.remove(ROOT)
    return track


def _write_frames(folder, n, h, w):
    from PIL import Image
    folder.mkdir()
    g = np.random.default_rng(5)
    paths = []
    for t in range(n):
        p = folder / f"frame_{t:04d}.png"
        Image.fromarray(g.integers(0, 255, (h, w, 3)).astype(np.uint8)).save(p)
        paths.append(str(p))
    return paths


def test_track_cli_reanchor_every(cli, tmp_path, monkeypatch):
    from PIL import Image
    from raft_stir_amd.data.frame_utils import readFlow, writeFlow
    h, w, n = 32, 48, 6
    images = _write_frames(tmp_path / "frames", n, h, w)
    pts = np.array([[10.0, 20.0], [3.5, 30.25], [47.0, 0.0]], dtype=np.float32)
    out = tmp_path / "re"
    args = cli.parse_args(["--dense", "--deltas", "1", "--reanchor_every", "2", "--out", str(out), "--iters", "2"])
    assert args.reanchor_every == 2 and args.reanchor_below is None
    calls = []
    real = ops.dense_compose
    monkeypatch.setattr(ops, "dense_compose", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    traj = cli.track_dense(args, D.StubAny(), images, pts, torch.device("cpu"))
    assert len(calls) == n - 3  # frames 3, 4, 5 are composed; the anchors are frames 0, 2 and 4
    dx, dy = S.STUB_D
    ys, xs = np.mgrid[0:h, 0:w]
    assert sorted(os.listdir(out)) == sorted([f"{k}_{t:04d}.{e}" for k, e in (("flow", "flo"), ("visible", "png"))
                                              for t in range(n)] + ["tracks.csv"])
    for t in range(n):
        vis = np.asarray(Image.open(out / f"visible_{t:04d}.png"))
        x, y = xs + t * dx, ys + t * dy
        want = (x >= 0) & (x <= w - 1) & (y >= 0) & (y <= h - 1)
        assert np.array_equal(vis, want.astype(np.uint8) * 255), t
        flow = readFlow(str(out / f"flow_{t:04d}.flo"))
        assert np.array_equal(flow[want], np.broadcast_to(np.float32([t * dx, t * dy]), flow.shape)[want]), t
    for t in range(n):
        for j, (px, py) in enumerate(pts):
            x, y = px + t * dx, py + t * dy
            if 0 <= x <= w - 1 and 0 <= y <= h - 1:
                assert np.allclose(traj[t, j], (x, y)), (t, j)

    # without the flags: the files of the loop track.py ran before the options existed, byte for byte, and no op
    def boom(*a, **k):
        raise AssertionError("dense_compose was called")
    monkeypatch.setattr(ops, "dense_compose", boom)
    out2 = tmp_path / "plain"
    args = cli.parse_args(["--dense", "--deltas", "1", "--out", str(out2), "--iters", "2"])
    assert args.reanchor_every is None and args.reanchor_below is None
    cli.track_dense(args, D.StubAny(), images, pts, torch.device("cpu"))
    out3 = tmp_path / "before"
    out3.mkdir()
    trk = DenseMultiFlowTracker(D.StubAny(), iters=2, deltas=(1,), fb_alpha=(0.01, 0.5), warm_start=True,
                                cache_features=False)
    for t, f in enumerate(images):
        trk.step(cli.load_image(f, torch.device("cpu")))
        writeFlow(str(out3 / f"flow_{t:04d}.flo"), trk.flow[0].permute(1, 2, 0).numpy())
        Image.fromarray(trk.visible[0, 0].numpy().astype(np.uint8) * 255).save(out3 / f"visible_{t:04d}.png")
    for name in sorted(os.listdir(out3)):
        assert (out2 / name).read_bytes() == (out3 / name).read_bytes(), name
    with pytest.raises(SystemExit):
        cli.parse_args(["--points", "p.txt", "--reanchor_every", "2"])
    with pytest.raises(SystemExit):
        cli.parse_args(["--dense", "--deltas", "1", "--reanchor_below", "1.5"])
    with pytest.raises(SystemExit):
        cli.parse_args(["--dense", "--deltas", "1", "--reanchor_every", "0"])

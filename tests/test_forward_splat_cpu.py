"""Dense forward splatting on the CPU: the ATen oracle (ops/reference.py:
forward_splat) against a brute-force loop over sources and cells, the named
fields' closed forms, the wrapper's checks, DenseMultiFlowTracker.splat /
warp_labels / track(labels=) on a translating stub, and track.py --labels."""
import glob
import os
import sys

import numpy as np
import pytest
import torch

from raft_stir_amd import ops
from raft_stir_amd.export.denseflow import DenseMultiFlowTracker
from raft_stir_amd.ops import reference

import dense_flow_cases as D
import forward_splat_cases as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF, NAN = S.INF, S.NAN
f32 = np.float32


# ------------------------------------------------------------- brute force
def brute_force(pos, score, values, footprint, fill):
    """Per source, per offered cell, keep the smallest (class, score, n):
    plain Python over numpy fp32 scalars."""
    _, _, H, W = pos.shape
    px, py, sc = pos[0, 0].numpy().reshape(-1), pos[0, 1].numpy().reshape(-1), score.numpy().reshape(-1)
    best = {}
    for n in range(H * W):
        x, y, s = px[n], py[n], sc[n] + f32(0.0)
        if not (s >= 0 and s < INF and x > -1 and x < W and y > -1 and y < H):
            continue
        nx, ny = int(np.rint(x)), int(np.rint(y))
        if footprint == 1:
            cells = [(nx, ny, 0)]
        else:
            xf, yf = np.floor(x), np.floor(y)
            wx, wy = f32(x - xf), f32(y - yf)
            ux, uy = f32(f32(1) - wx), f32(f32(1) - wy)
            cells = []
            for dx, dy, w in ((0, 0, f32(ux * uy)), (1, 0, f32(wx * uy)), (0, 1, f32(ux * wy)), (1, 1, f32(wx * wy))):
                xi, yi = int(xf) + dx, int(yf) + dy
                if w != 0:
                    cells.append((xi, yi, 0 if (xi, yi) == (nx, ny) else 1))
        for xi, yi, cls in cells:
            if 0 <= xi < W and 0 <= yi < H:
                offer = (cls, float(s), n)
                c = yi * W + xi
                if c not in best or offer < best[c]:
                    best[c] = offer
    src = np.full(H * W, -1, np.int32)
    inv = np.full((2, H * W), np.nan, f32)
    C = 0 if values is None else values.shape[1]
    out = np.full((C, H * W), fill, f32)
    for c, (_, _, n) in best.items():
        src[c] = n
        inv[0, c] = f32(n % W) + f32(f32(c % W) - px[n])
        inv[1, c] = f32(n // W) + f32(f32(c // W) - py[n])
        if C:
            out[:, c] = values[0].numpy().reshape(C, -1)[:, n]
    return (torch.from_numpy(src).view(1, 1, H, W), torch.from_numpy(src >= 0).view(1, 1, H, W),
            torch.from_numpy(inv).view(1, 2, H, W), torch.from_numpy(out).view(1, C, H, W) if C else None)


def _all_same(got, want, what):
    for name, g, w in zip(S.NAMES, got, want):
        if w is None:
            assert g is None, (what, name)
        else:
            assert g.dtype == w.dtype and g.shape == w.shape and S.same(g, w), (what, name, int((g != w).sum()))


@pytest.mark.parametrize("footprint", S.FOOTPRINTS)
@pytest.mark.parametrize("name", S.FIELDS)
@pytest.mark.parametrize("hw", S.SHAPES, ids=lambda hw: f"{hw[0]}x{hw[1]}")
def test_oracle_against_brute_force(hw, name, footprint):
    H, W = hw
    pos, score = S.field(name, H, W)
    for C, fill in ((0, 0.0), (3, -7.5)):
        vals = S.values(C, H, W)
        got = S.expected(name, H, W, footprint, C, fill)
        assert got[0].dtype == torch.int32 and got[1].dtype == torch.bool and got[2].dtype == torch.float32
        _all_same(got, brute_force(pos, score, vals, footprint, fill), (hw, name, footprint, C))
    # through the public wrapper, which takes other dtypes and layouts (fp32 -> fp64 -> fp32 is exact)
    wrapped = ops.forward_splat(pos.double(), score.double().transpose(2, 3).contiguous().transpose(2, 3),
                                S.values(3, H, W), footprint=footprint, fill=-7.5)
    _all_same(wrapped, got, (hw, name, footprint, "wrapper"))


def test_mixed_field_exercises_every_outcome():
    """At (24,70), footprint 2: cells won in class 0 and in class 1, holes, and
    class-0 cells decided by nothing, by the score and by the index tie."""
    H, W = 24, 70
    pos, score = S.field("mixed", H, W)
    n = S.outcome_counts(pos, score, 2)
    print(n)
    assert n["class0"] + n["class1"] + n["holes"] == H * W
    assert n["uncontested"] + n["score"] + n["tie"] == n["class0"]
    for key in ("class0", "class1", "holes", "uncontested", "score", "tie"):
        assert n[key] >= 5, n
    # the fixed places: what each of them must do, footprint 1
    src = S.expected("mixed", H, W, 1)[0].flatten().tolist()
    spots = {(x, y): (j * 37 + 5) % (H * W) for j, (x, y) in enumerate(S.specials(H, W))}
    offered = set(src)
    for x, y in ((NAN, 1.0), (INF, 0.0), (-INF, 0.0), (1e30, 1.0), (-1.0, 0.0), (float(W), 0.0)):
        assert spots[(x, y)] not in offered, (x, y)  # no source
    assert spots[(-0.75, 1.0)] not in offered and spots[(W - 0.5, 1.0)] not in offered  # cells -1 and W (70: even)
    assert spots[(0.0, H - 0.25)] not in offered  # cell (0, H)
    # -0.5 rounds to -0, cell 0; its score is 0, so it takes the cell unless a lower index does
    assert src[0] >= 0 and src[0] <= spots[(-0.5, 0.0)]
    assert src[(H - 1) * W + W - 1] >= 0


@pytest.mark.parametrize("hw", S.SHAPES, ids=lambda hw: f"{hw[0]}x{hw[1]}")
def test_named_fields(hw):
    H, W = hw
    N = H * W
    grid = reference.coords_grid(1, H, W)
    for fp in S.FOOTPRINTS:
        src, cov, inv, out = S.expected("identity", H, W, fp, 3, -7.5)
        assert torch.equal(src.flatten(), torch.arange(N, dtype=torch.int32)) and cov.all()
        assert torch.equal(inv, grid) and torch.equal(out, S.values(3, H, W))
        src, cov, inv, out = S.expected("none", H, W, fp, 3, -7.5)
        assert (src == -1).all() and not cov.any() and torch.isnan(inv).all() and (out == -7.5).all()
        assert torch.isnan(reference.forward_splat(*S.field("none", H, W), S.values(1, H, W), fp, NAN)[3]).all()
        # every pixel at (3.25, 2.5): one winner, the pixel with the lower score
        src, cov, inv, out = S.expected("one_cell", H, W, fp, 1, -7.5)
        cells = [(3, 2)] if fp == 1 else [(3, 2), (4, 2), (3, 3), (4, 3)]
        cells = [(x, y) for x, y in cells if x < W and y < H]
        want = torch.full((H, W), -1, dtype=torch.int32)
        for x, y in cells:
            want[y, x] = S.one_cell_winner(H, W)
        assert torch.equal(src[0, 0], want) and int(cov.sum()) == len(cells)
        w = S.one_cell_winner(H, W)
        for x, y in cells:
            assert inv[0, :, y, x].tolist() == [w % W + (x - 3.25), w // W + (y - 2.5)]
            assert out[0, 0, y, x] == S.values(1, H, W).flatten()[w]


def test_score_order_and_zero_signs():
    """Two sources on one cell: the smaller score wins whatever the indices;
    -0 and +0 tie (the lower index wins); a denormal loses to 0 and beats 1e-38."""
    H, W = 4, 4
    grid = reference.coords_grid(1, H, W)

    def winner(s_a, s_b):
        pos, score = grid.clone(), torch.full((1, 1, H, W), INF)
        pos[0, :, 1, 1] = torch.tensor([2.0, 2.0])  # a = 5
        pos[0, :, 3, 0] = torch.tensor([2.25, 1.75])  # b = 12
        score[0, 0, 1, 1], score[0, 0, 3, 0] = s_a, s_b
        return [int(reference.forward_splat(pos, score, None, fp, 0.0)[0][0, 0, 2, 2]) for fp in (1, 2)]

    assert winner(0.5, 0.25) == [12, 12] and winner(0.25, 0.5) == [5, 5]
    assert winner(0.0, -0.0) == [5, 5] and winner(-0.0, 0.0) == [5, 5]
    assert winner(1e-40, 0.0) == [12, 12] and winner(1e-38, 1e-40) == [12, 12]
    assert winner(INF, 3.0) == [12, 12] and winner(NAN, -1.0) == [-1, -1]
    # a source that only touches a cell loses to one that lands on it, whatever the scores
    pos, score = grid.clone(), torch.full((1, 1, H, W), INF)
    pos[0, :, 0, 0] = torch.tensor([1.5, 1.0])  # n = 0: nearest (2,1) (half to even), touches (1,1)
    pos[0, :, 0, 1] = torch.tensor([1.0, 1.0])  # n = 1: lands on (1,1)
    score[0, 0, 0, 0], score[0, 0, 0, 1] = 0.0, 2.0
    src = reference.forward_splat(pos, score, None, 2, 0.0)[0][0, 0]
    assert int(src[1, 1]) == 1 and int(src[1, 2]) == 0 and int((src >= 0).sum()) == 2
    assert int(reference.forward_splat(pos, score, None, 1, 0.0)[0][0, 0, 1, 2]) == 0


def test_wrapper_checks():
    pos, score = S.field("mixed", 7, 9)
    with pytest.raises(ValueError, match=r"pos must be \(1,2,H,W\)"):
        ops.forward_splat(pos[0], score)
    with pytest.raises(ValueError, match=r"pos must be \(1,2,H,W\)"):
        ops.forward_splat(pos.repeat(2, 1, 1, 1), score)
    with pytest.raises(ValueError, match="H, W >= 2"):
        ops.forward_splat(pos[..., :1], score[..., :1])
    with pytest.raises(ValueError, match="score must be"):
        ops.forward_splat(pos, score[0])
    with pytest.raises(ValueError, match="values must be"):
        ops.forward_splat(pos, score, torch.zeros(1, 2, 7, 8))
    for fp in (0, 3):
        with pytest.raises(ValueError, match="footprint must be 1 or 2"):
            ops.forward_splat(pos, score, footprint=fp)
    assert "forward_splat" in ops.__all__
    # no kernel, no quiet run on another device
    with pytest.raises(NotImplementedError, match="no HIP kernel yet"):
        ops.forward_splat(pos.to("meta"), score.to("meta"))


# ------------------------------------------------------------------ the tracker
def _shifted(L, shift, fill):
    """L (C,H,W) moved by the integer (dx, dy): out[c] = L[c - shift] inside, fill elsewhere."""
    C, H, W = L.shape
    dx, dy = shift
    out = torch.full_like(L, fill)
    inside = torch.zeros(H, W, dtype=torch.bool)
    ys, xs = slice(max(dy, 0), H + min(dy, 0)), slice(max(dx, 0), W + min(dx, 0))
    yo, xo = slice(max(-dy, 0), H + min(-dy, 0)), slice(max(-dx, 0), W + min(-dx, 0))
    out[:, ys, xs] = L[:, yo, xo]
    inside[ys, xs] = True
    return out, inside


@pytest.mark.parametrize("deltas", [(1,), (1, 3, None)])
def test_tracker_warps_labels_by_the_translation(deltas):
    H, W, T = 24, 40, 6
    dx, dy = 3, -2
    frames = D.frames(T, H, W)
    trk = DenseMultiFlowTracker(S.StubShift((float(dx), float(dy))), iters=2, deltas=deltas)
    g = torch.Generator().manual_seed(3)
    labels = {"uint8": torch.randint(1, 255, (H, W), generator=g, dtype=torch.uint8),
              "int64": torch.randint(-2 ** 40, 2 ** 40, (1, 1, H, W), generator=g),
              "bool": torch.rand(1, 2, H, W, generator=g) < 0.5,
              "fp32": torch.randn(1, 3, H, W, generator=g)}
    fills = {"uint8": 255, "int64": -1, "bool": True, "fp32": -0.5}
    for what in ("splat", "warp_labels"):
        with pytest.raises(ValueError, match="needs a step first"):
            getattr(trk, what)(labels["fp32"])
    grid = reference.coords_grid(1, H, W)
    for t in range(T):
        trk.step(frames[t])
        shift = (t * dx, t * dy)
        index, inside = _shifted(torch.arange(H * W).view(1, H, W), shift, -1)
        for fp in S.FOOTPRINTS:
            src, cov, inv, out = trk.splat(labels["fp32"], footprint=fp, fill=-0.5)
            assert torch.equal(src[0], index.int()) and torch.equal(cov[0, 0], inside), (t, fp)
            assert torch.equal(out[0], _shifted(labels["fp32"][0], shift, -0.5)[0]), (t, fp)
            back = grid - torch.tensor([float(shift[0]), float(shift[1])]).view(1, 2, 1, 1)
            assert torch.equal(inv[cov.expand(1, 2, H, W)], back[cov.expand(1, 2, H, W)])
            assert torch.isnan(inv[~cov.expand(1, 2, H, W)]).all()
            # what is covered is what is visible, moved
            assert torch.equal(cov[0], _shifted(trk.visible[0], shift, False)[0]), (t, fp)
            for name, lab in labels.items():
                warped, c = trk.warp_labels(lab, footprint=fp, fill=fills[name])
                assert warped.dtype == lab.dtype and warped.shape == lab.shape and torch.equal(c, cov), (t, name)
                want = _shifted(lab.reshape(-1, H, W), shift, fills[name])[0].reshape(lab.shape)
                assert torch.equal(warped, want), (t, fp, name)
        if t == 0:
            assert cov.all() and torch.equal(src.flatten(), torch.arange(H * W, dtype=torch.int32))
    assert not cov.all() and cov.any()
    assert trk.splat()[3] is None
    for bad in (torch.zeros(H, W + 1), torch.zeros(1, H, W), torch.zeros(2, 1, H, W)):
        with pytest.raises(ValueError, match="labels must be"):
            trk.warp_labels(bad)
    with pytest.raises(ValueError, match="footprint must be 1 or 2"):
        trk.splat(footprint=4)


def test_track_with_and_without_labels():
    H, W, T = 24, 40, 5
    frames = D.frames(T, H, W)
    lab = torch.randint(0, 7, (H, W), generator=torch.Generator().manual_seed(1), dtype=torch.uint8)
    trk = DenseMultiFlowTracker(S.StubShift((3.0, -2.0)), iters=2, deltas=(1, None))
    plain = trk.track(frames)
    assert len(plain) == 2
    # what track() gave before labels existed: the flow and the visibility of every step
    trk.reset()
    for t in range(T):
        trk.step(frames[t])
        assert torch.equal(plain[0][t], trk.flow[0]) and torch.equal(plain[1][t], trk.visible[0])
    flows, vis, warped, cov = trk.track(frames, lab, footprint=1, fill=9)
    assert torch.equal(flows, plain[0]) and torch.equal(vis, plain[1])
    assert warped.shape == (T, H, W) and warped.dtype == torch.uint8 and cov.shape == (T, 1, H, W)
    assert torch.equal(warped[0], lab) and cov[0].all()
    for t in range(T):
        want, inside = _shifted(lab[None], (3 * t, -2 * t), 9)
        assert torch.equal(warped[t], want[0]) and torch.equal(cov[t, 0], inside)


# --------------------------------------------------------------------- track.py
@pytest.fixture(scope="module")
def cli():
    sys.path.insert(0, ROOT)
    try:
        import track
    finally:
        sys.path.remove(ROOT)
    return track


@pytest.mark.parametrize("bits", [8, 16])
def test_track_cli_labels(cli, tmp_path, bits):
    """The three demo frames (436x1024, padded to 440x1024) through StubAny: the
    mask of the first frame moves by the stub's translation per frame."""
    from PIL import Image
    images = sorted(glob.glob(os.path.join(ROOT, "demo-frames", "*.png")))
    W, H = Image.open(images[0]).size
    assert H % 8 != 0  # the frames are padded
    g = np.random.default_rng(2)
    mask = g.integers(1, 250 if bits == 8 else 60000, (H, W)).astype(np.uint8 if bits == 8 else np.uint16)
    Image.fromarray(mask).save(tmp_path / "mask.png")
    out = tmp_path / "dense"
    # one span: StubAny answers every pair with the same translation, whatever its span
    args = cli.parse_args(["--dense", "--deltas", "1", "--labels", str(tmp_path / "mask.png"),
                           "--splat_footprint", "1", "--out", str(out), "--iters", "2"])
    assert args.splat_footprint == 1 and cli.parse_args(["--dense", "--deltas", "1"]).splat_footprint == 2
    cli.track_dense(args, D.StubAny(), images, None, torch.device("cpu"))
    dx, dy = (int(v) for v in S.STUB_D)
    for t in range(3):
        lab = np.asarray(Image.open(out / f"labels_{t:04d}.png"))
        cov = np.asarray(Image.open(out / f"covered_{t:04d}.png"))
        assert lab.shape == (H, W) and lab.dtype == mask.dtype and cov.dtype == np.uint8
        want, inside = _shifted(torch.from_numpy(mask.astype(np.int64))[None], (dx * t, dy * t), 0)
        # pixels that started in the padding carry label 0 and may cover cells next to the border
        assert np.array_equal(lab[inside.numpy()], want[0].numpy()[inside.numpy()])
        assert (cov[inside.numpy()] == 255).all() and (lab[cov == 0] == 0).all()
        assert set(np.unique(cov)) <= {0, 255}
    assert (np.asarray(Image.open(out / "covered_0000.png")) == 255).all()
    assert np.array_equal(np.asarray(Image.open(out / "labels_0000.png")), mask)
    # without --labels nothing changes
    out2 = tmp_path / "dense2"
    args = cli.parse_args(["--dense", "--deltas", "1", "--out", str(out2), "--iters", "2"])
    assert args.labels is None
    cli.track_dense(args, D.StubAny(), images, None, torch.device("cpu"))
    assert sorted(os.listdir(out2)) == [f"{n}_{t:04d}.{e}" for n, e in (("flow", "flo"), ("visible", "png"))
                                        for t in range(3)]
    with pytest.raises(SystemExit):
        cli.parse_args(["--points", "p.txt", "--labels", "m.png"])
    bad = tmp_path / "bad.png"
    Image.fromarray(mask[:-1]).save(bad)
    args = cli.parse_args(["--dense", "--deltas", "1", "--labels", str(bad), "--out", str(out2)])
    with pytest.raises(ValueError, match="first frame's size"):
        cli.track_dense(args, D.StubAny(), images, None, torch.device("cpu"))

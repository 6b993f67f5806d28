"""Hole in-painting after a forward splat, on the CPU: the ATen oracle
(ops/reference.py: splat_inpaint) against a brute force over all (cell, covered
cell) pairs, conditions on the inputs, the rule's closed forms on the hand-made
maps, the wrapper's checks, ``inpaint=`` of DenseMultiFlowTracker.splat /
warp_labels / track on a translating stub, and track.py --inpaint."""
import glob
import math
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
import splat_inpaint_cases as I

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN = I.NAN
f32 = np.float32
HW_IDS = dict(ids=lambda hw: f"{hw[0]}x{hw[1]}")


# ------------------------------------------------------------- brute force
def pair_keys(src, H, W):
    """(keys (N, M) int64 of every cell against every covered cell, the clamped entries s (N,))."""
    N = H * W
    s = np.clip(src.numpy().reshape(N).astype(np.int64), -1, N - 1)
    cells = np.nonzero(s >= 0)[0]
    c = np.arange(N)
    d2 = (c[:, None] % W - cells[None, :] % W) ** 2 + (c[:, None] // W - cells[None, :] // W) ** 2
    return (d2 << 31) | cells[None, :], s


def brute_force(src, pos, inv, values, R, fill, keys=None):
    """The rule as it is stated: per cell the smallest (d2 << 31 | c') over
    all covered cells c', kept if d2 <= R*R; numpy on every pair."""
    _, _, H, W = src.shape
    N = H * W
    keys, s = pair_keys(src, H, W) if keys is None else keys
    best = keys.min(axis=1) if keys.shape[1] else np.full(N, -1, np.int64)
    has = (best >= 0) & ((best >> 31) <= R * R)
    donor = np.where(has, best & (2 ** 31 - 1), -1)
    dist2 = np.where(has, best >> 31, -1)
    win = np.where(has, s[np.maximum(donor, 0)], -1)
    px, py = pos[0, 0].numpy().reshape(N), pos[0, 1].numpy().reshape(N)
    out_inv = np.full((2, N), np.nan, f32)
    given = inv.numpy().reshape(2, N)
    C = 0 if values is None else values.shape[1]
    out = np.full((C, N), fill, f32)
    vals = None if values is None else values[0].numpy().reshape(C, N)
    for c in np.nonzero(has)[0]:
        w = win[c]
        if donor[c] == c:
            out_inv[:, c] = given[:, c]
        else:
            out_inv[0, c] = f32(w % W) + f32(f32(c % W) - px[w])
            out_inv[1, c] = f32(w // W) + f32(f32(c // W) - py[w])
        if C:
            out[:, c] = vals[:, w]
    t = lambda a, ch, dt: torch.from_numpy(a.astype(dt)).view(1, ch, H, W)  # noqa: E731
    return (t(win, 1, np.int32), t(donor, 1, np.int32), t(dist2, 1, np.int32), t(out_inv, 2, f32),
            t(out, C, f32) if C else None)


@pytest.mark.parametrize("name", I.MAPS)
@pytest.mark.parametrize("hw", I.SHAPES, **HW_IDS)
def test_oracle_against_brute_force(hw, name):
    H, W = hw
    src, pos, inv = I.case(name, H, W)
    keys = pair_keys(src, H, W)
    with np.errstate(invalid="ignore", over="ignore"):
        for R in I.RADII:
            for C, fill in ((0, 0.0), (3, -7.5)):
                got = I.expected(name, H, W, R, C, fill)
                assert [g.dtype for g in got[:4]] == [torch.int32] * 3 + [torch.float32]
                want = brute_force(src, pos, inv, I.values(C, H, W), I.radius(R, H, W), fill, keys)
                I.all_same(got, want, (hw, name, R, C))
            # through the public wrapper, which takes other dtypes and layouts (fp32 -> fp64 -> fp32 is exact)
            wrapped = ops.splat_inpaint(src.long(), pos.double(), inv.transpose(2, 3).contiguous().transpose(2, 3),
                                        I.values(3, H, W), max_dist=math.inf if R is None else R, fill=-7.5)
            I.all_same(wrapped, I.expected(name, H, W, R, 3, -7.5), (hw, name, R, "wrapper"))


@pytest.mark.parametrize("fp", S.FOOTPRINTS)
def test_mixed_map_exercises_the_rule(fp):
    """A condition on the inputs, from the brute force alone: on mixed 24x70,
    at each radius, cells are filled, holes are left, and filled cells have
    their smallest d2 shared by several covered cells (the index decides)."""
    H, W = 24, 70
    src, pos, inv = I.case(f"mixed_fp{fp}", H, W)
    keys, s = pair_keys(src, H, W)
    d2 = keys >> 31
    best = d2.min(axis=1)
    shared = (d2 == best[:, None]).sum(axis=1) > 1
    hole = s < 0
    if fp == 2:
        assert int(hole.sum()) == 776
    for R in (1, 2, 3, 5):
        filled = hole & (best <= R * R)
        n = dict(filled=int(filled.sum()), left=int((hole & ~filled).sum()), shared=int((filled & shared).sum()))
        print(fp, R, n)
        assert n["filled"] > 0 and n["left"] > 0 and n["shared"] > 0, (R, n)
        got = I.expected(f"mixed_fp{fp}", H, W, R)
        assert int(((got[0] >= 0).flatten().numpy() & hole).sum()) == n["filled"]


# ------------------------------------------------------------ closed forms
@pytest.mark.parametrize("hw", I.SHAPES, **HW_IDS)
def test_radius_zero_returns_the_input(hw):
    H, W = hw
    N = H * W
    for name in I.MAPS:
        src, pos, inv = I.case(name, H, W)
        got = I.expected(name, H, W, 0, 3, -7.5)
        s = src.long().clamp(-1, N - 1)
        assert torch.equal(got[0].long(), s) and I.same(got[3], torch.where(s >= 0, inv, torch.tensor(NAN)))
        own = torch.arange(N).view(1, 1, H, W)
        assert torch.equal(got[1].long(), torch.where(s >= 0, own, -1)) and torch.equal(got[2], (got[1] >= 0).int() - 1)
        vals = I.values(3, H, W).view(3, N)
        want = torch.where(s.view(1, N) >= 0, vals[:, s.view(N).clamp(min=0)], torch.tensor(-7.5)).view(1, 3, H, W)
        assert torch.equal(got[4], want)
        if name not in ("bad_entries",):
            assert torch.equal(got[0], src) and I.same(got[3], inv)


def test_ties_go_to_the_lowest_cell_index():
    H, W = 7, 9
    cy, cx = I.centre(H, W)
    c = cy * W + cx
    for name in ("tie_row", "tie_col", "tie_diag", "tie_anti"):
        (y0, x0), (y1, x1) = I.tie_cells(name, H, W)
        lower = min(y0 * W + x0, y1 * W + x1)
        d2 = (y0 - cy) ** 2 + (x0 - cx) ** 2
        assert d2 == (y1 - cy) ** 2 + (x1 - cx) ** 2 and d2 in (1, 2)
        src = I.case(name, H, W)[0]
        for R in I.RADII:
            out_src, donor, dist2, _, _ = I.expected(name, H, W, R)
            if I.radius(R, H, W) ** 2 >= d2:
                assert int(donor.view(-1)[c]) == lower and int(dist2.view(-1)[c]) == d2, (name, R)
                assert int(out_src.view(-1)[c]) == int(src.view(-1)[lower])
            else:
                assert int(donor.view(-1)[c]) == -1 and int(out_src.view(-1)[c]) == -1, (name, R)
    # anti-diagonal: the lower index is the cell to the right, so the index decides and not x
    assert I.tie_cells("tie_anti", H, W)[0] == (cy - 1, cx + 1)
    # checkerboard: a hole takes the cell above it, in the first row the cell to its left
    for R in (1, 2, None):
        donor = I.expected("checker", 24, 70, R)[1][0, 0]
        hole = I.case("checker", 24, 70)[0][0, 0] < 0
        own = torch.arange(24 * 70).view(24, 70)
        want = torch.where(hole, own - 70, own)
        want[0] = torch.where(hole[0], own[0] - 1, own[0])
        assert torch.equal(donor.long(), want), R
        assert torch.equal(I.expected("checker", 24, 70, R)[2][0, 0], hole.int())


def test_frame_and_corners():
    H, W = 24, 70
    cy, cx = I.centre(H, W)
    for R in (0, 1, 2, 3, 5):
        src, donor, dist2, inv, _ = I.expected("frame", H, W, R)
        depth = torch.minimum(torch.minimum(torch.arange(H).view(H, 1), H - 1 - torch.arange(H).view(H, 1)),
                              torch.minimum(torch.arange(W).view(1, W), W - 1 - torch.arange(W).view(1, W)))
        assert torch.equal(src[0, 0] >= 0, depth <= R), R  # filled R cells deep, and the centre stays a hole
        assert int(src[0, 0, cy, cx]) == -1 and int(donor[0, 0, cy, cx]) == -1 and int(dist2[0, 0, cy, cx]) == -1
        assert torch.isnan(inv[0, :, cy, cx]).all()
        assert torch.equal(dist2[0, 0], torch.where(depth <= R, depth * depth, -1).int())
    assert (I.expected("frame", H, W, None)[0] >= 0).all()
    # unlimited from four corners: every cell is filled from the nearest corner
    src, donor, dist2, _, _ = I.expected("corners", H, W, None)
    assert set(donor.flatten().tolist()) == {0, W - 1, (H - 1) * W, H * W - 1}
    ys, xs = torch.arange(H).view(H, 1), torch.arange(W).view(1, W)
    want = torch.minimum(ys, H - 1 - ys) ** 2 + torch.minimum(xs, W - 1 - xs) ** 2
    assert torch.equal(dist2[0, 0].long(), want)
    # R = 5: a quarter disc at every corner
    assert torch.equal(I.expected("corners", H, W, 5)[2][0, 0].long(), torch.where(want <= 25, want, -1))


def test_entries_out_of_range_are_clamped():
    H, W = 7, 9
    N = H * W
    src = I.case("bad_entries", H, W)[0]
    for R in I.RADII:
        out_src, donor, _, _, out = I.expected("bad_entries", H, W, R, 1, -7.5)
        assert int(out_src.min()) >= -1 and int(out_src.max()) <= N - 1
        for c, v in I.bad_entries(H, W).items():
            if v >= 0:  # covered by the last anchor pixel
                assert int(out_src.view(-1)[c]) == N - 1 and int(donor.view(-1)[c]) == c
                assert float(out.view(-1)[c]) == float(I.values(1, H, W).view(-1)[N - 1])
            elif R == 0:
                assert int(out_src.view(-1)[c]) == -1 and int(donor.view(-1)[c]) == -1
        # the same map with the entries clamped by hand
        clamped = reference.splat_inpaint(src.clamp(-1, N - 1), *I.case("bad_entries", H, W)[1:], I.values(1, H, W),
                                          I.radius(R, H, W), -7.5)
        I.all_same(I.expected("bad_entries", H, W, R, 1, -7.5), clamped, R)


# ---------------------------------------------------------------------- wrapper
def test_wrapper_checks():
    src, pos, inv = I.case("mixed_fp2", 7, 9)
    with pytest.raises(ValueError, match=r"src_index must be \(1,1,H,W\)"):
        ops.splat_inpaint(src[0], pos, inv)
    with pytest.raises(ValueError, match="integer dtype"):
        ops.splat_inpaint(src.float(), pos, inv)
    with pytest.raises(ValueError, match="H, W in"):
        ops.splat_inpaint(src[..., :1], pos[..., :1], inv[..., :1])
    with pytest.raises(ValueError, match="pos must be"):
        ops.splat_inpaint(src, pos[:, :1], inv)
    with pytest.raises(ValueError, match="inv_pos must be"):
        ops.splat_inpaint(src, pos, inv[0])
    with pytest.raises(ValueError, match="values must be"):
        ops.splat_inpaint(src, pos, inv, torch.zeros(1, 2, 7, 8))
    for bad in (-1, 32768):
        with pytest.raises(ValueError, match="max_dist must be in"):
            ops.splat_inpaint(src, pos, inv, max_dist=bad)
    for bad in (2.5, "3", True, -math.inf):
        with pytest.raises(ValueError, match="max_dist must be an integer"):
            ops.splat_inpaint(src, pos, inv, max_dist=bad)
    with pytest.raises(ValueError, match="max_dist"):
        reference.splat_inpaint(src, pos, inv, None, -1)
    assert "splat_inpaint" in ops.__all__
    # None and inf are max(H, W); the default is 8
    for R in (None, math.inf):
        I.all_same(ops.splat_inpaint(src, pos, inv, max_dist=R), I.expected("mixed_fp2", 7, 9, 9), R)
    I.all_same(ops.splat_inpaint(src, pos, inv), I.expected("mixed_fp2", 7, 9, 8), "default")
    # no kernel, no quiet run on another device
    with pytest.raises(NotImplementedError, match="no HIP kernel yet"):
        ops.splat_inpaint(src.to("meta"), pos.to("meta"), inv.to("meta"))


# ------------------------------------------------------------------ the tracker
def _labels(H, W):
    g = torch.Generator().manual_seed(3)
    labels = {"uint8": torch.randint(1, 255, (H, W), generator=g, dtype=torch.uint8),
              "int64": torch.randint(-2 ** 40, 2 ** 40, (1, 1, H, W), generator=g),
              "bool": torch.rand(1, 2, H, W, generator=g) < 0.5,
              "fp32": torch.randn(1, 3, H, W, generator=g)}
    return labels, {"uint8": 255, "int64": -1, "bool": True, "fp32": -0.5}


def test_inpaint_zero_is_todays_result(monkeypatch):
    """inpaint=0, given or left out, returns what the methods returned before
    the keyword existed, and the new op is not called."""
    H, W, T = 24, 40, 4
    frames = D.frames(T, H, W)
    labels, fills = _labels(H, W)

    def refuse(*a, **k):
        raise AssertionError("splat_inpaint called with inpaint=0")

    monkeypatch.setattr(ops, "splat_inpaint", refuse)
    trk = DenseMultiFlowTracker(S.StubShift((3.0, -2.0)), iters=2, deltas=(1, None))
    for t in range(T):
        trk.step(frames[t])
        for fp in S.FOOTPRINTS:
            want = ops.forward_splat(trk.pos, trk.score, labels["fp32"], footprint=fp, fill=-0.5)
            for got in (trk.splat(labels["fp32"], fp, -0.5), trk.splat(labels["fp32"], fp, -0.5, inpaint=0)):
                assert len(got) == 4 and all(S.same(g, w) for g, w in zip(got, want))
            for name, lab in labels.items():
                a, b = trk.warp_labels(lab, fp, fills[name]), trk.warp_labels(lab, fp, fills[name], inpaint=0)
                assert a[0].dtype == lab.dtype and S.same(a[0], b[0]) and torch.equal(a[1], b[1])
                if name == "fp32":
                    assert S.same(a[0], want[3]) and torch.equal(a[1], want[1])
                else:
                    g = lab.reshape(-1, H * W)[:, want[0].reshape(-1).long().clamp(min=0)].reshape(1, -1, H, W)
                    g = torch.where(want[1], g, torch.tensor(fills[name], dtype=lab.dtype))
                    assert torch.equal(a[0], g.reshape(lab.shape)) and torch.equal(a[1], want[1])
    a, b = trk.track(frames, labels["uint8"], 1, 9), trk.track(frames, labels["uint8"], 1, 9, inpaint=0)
    assert len(a) == 4 and all(torch.equal(x, y) for x, y in zip(a, b))
    assert len(trk.track(frames, inpaint=0)) == 2


@pytest.mark.parametrize("R", [1, 2, 5, None])
def test_inpaint_fills_the_uncovered_strip_to_its_radius(R):
    """The stub moves everything by (3, -2) per frame, which uncovers a strip
    at the left and at the bottom.  A cell of the strip is filled iff the
    covered rectangle is within R of it, with the label of the rectangle's
    nearest cell; integer labels stay exact."""
    H, W, T = 24, 40, 4
    dx, dy = 3, -2
    frames = D.frames(T, H, W)
    labels, fills = _labels(H, W)
    trk = DenseMultiFlowTracker(S.StubShift((float(dx), float(dy))), iters=2, deltas=(1, None))
    Rn = I.radius(R, H, W)
    ys, xs = torch.arange(H).view(H, 1).expand(H, W), torch.arange(W).view(1, W).expand(H, W)
    kept = []
    for t in range(T):
        trk.step(frames[t])
        x_lo, y_hi = dx * t, H - 1 + dy * t  # the covered rectangle: x >= x_lo, y <= y_hi
        inside = (xs >= x_lo) & (ys <= y_hi)
        nx, ny = xs.clamp(min=x_lo), ys.clamp(max=y_hi)
        d2 = (xs - nx) ** 2 + (ys - ny) ** 2
        filled = d2 <= Rn * Rn
        anchor = torch.where(filled, (ny - dy * t) * W + (nx - dx * t), -1)
        for fp in S.FOOTPRINTS:
            src, cov, inv, out = trk.splat(labels["fp32"], fp, -0.5, inpaint=R)
            assert torch.equal(cov[0, 0], inside) and torch.equal(src[0, 0].long(), anchor), (t, fp)
            assert torch.equal((src >= 0) & ~cov, (filled & ~inside).view(1, 1, H, W))
            want = torch.where(filled, labels["fp32"].view(3, -1)[:, anchor.clamp(min=0).view(-1)].view(3, H, W),
                               torch.tensor(-0.5))
            assert torch.equal(out[0], want)
            # the anchor pixel extended rigidly: the cell moved back by the translation
            back = torch.stack([xs - dx * t, ys - dy * t]).float()
            assert torch.equal(inv[0][:, filled], back[:, filled]) and torch.isnan(inv[0][:, ~filled]).all()
            plain = trk.splat(labels["fp32"], fp, -0.5)
            assert torch.equal(plain[1], cov) and all(S.same(a[cov.expand_as(a)], b[cov.expand_as(b)])
                                                      for a, b in zip((src, inv, out), (plain[0], plain[2], plain[3])))
            for name, lab in labels.items():
                warped, c = trk.warp_labels(lab, fp, fills[name], inpaint=R)
                ch = lab.numel() // (H * W)
                g = lab.reshape(ch, -1)[:, anchor.clamp(min=0).view(-1)].view(ch, H, W)
                want = torch.where(filled, g, torch.tensor(fills[name], dtype=lab.dtype)).reshape(lab.shape)
                assert warped.dtype == lab.dtype and torch.equal(warped, want) and torch.equal(c, cov), (t, fp, name)
        kept.append((trk.warp_labels(labels["int64"], 2, -1, inpaint=R)[0], inside.clone()))
        if t and R in (1, 2):
            assert (filled & ~inside).any() and (~filled).any()
    flows, vis, warped, cov = trk.track(frames, labels["int64"], 2, -1, inpaint=R)
    plain = trk.track(frames)
    assert torch.equal(flows, plain[0]) and torch.equal(vis, plain[1])
    for t in range(T):
        assert torch.equal(warped[t], kept[t][0]) and torch.equal(cov[t, 0], kept[t][1])


# --------------------------------------------------------------------- track.py
@pytest.fixture(scope="module")
def cli():
    sys.path.insert(0, ROOT)
    try:
        import track
    finally:
        sys.path.remove(ROOT)
    return track


def test_track_cli_inpaint(cli, tmp_path):
    """The three demo frames through StubAny with --inpaint 2: the strip the
    translation uncovers is in-painted two cells deep (128 in covered_TTTT.png)
    from the labels next to it; without the flag the files are what they were."""
    from PIL import Image
    images = sorted(glob.glob(os.path.join(ROOT, "demo-frames", "*.png")))
    W, H = Image.open(images[0]).size
    mask = np.random.default_rng(2).integers(1, 60000, (H, W)).astype(np.uint16)
    Image.fromarray(mask).save(tmp_path / "mask.png")
    base = ["--dense", "--deltas", "1", "--labels", str(tmp_path / "mask.png"), "--iters", "2"]
    outs = {}
    for flag in ((), ("--inpaint", "0"), ("--inpaint", "2"), ("--inpaint", "inf")):
        out = outs[flag[-1] if flag else None] = tmp_path / ("dense_" + "_".join(flag).strip("-"))
        args = cli.parse_args(base + ["--out", str(out), *flag])
        assert args.inpaint == {(): 0, ("--inpaint", "0"): 0, ("--inpaint", "2"): 2, ("--inpaint", "inf"): None}[flag]
        cli.track_dense(args, D.StubAny(), images, None, torch.device("cpu"))
    read = lambda d, n, t: np.asarray(Image.open(d / f"{n}_{t:04d}.png"))  # noqa: E731
    dx, dy = (int(v) for v in S.STUB_D)  # (3, -2)
    for t in range(3):
        for name in ("labels", "covered"):
            a, b = (open(outs[k] / f"{name}_{t:04d}.png", "rb").read() for k in (None, "0"))
            assert a == b
        lab0, cov0 = read(outs[None], "labels", t), read(outs[None], "covered", t)
        lab, cov = read(outs["2"], "labels", t), read(outs["2"], "covered", t)
        assert lab.dtype == mask.dtype and cov.dtype == np.uint8 and set(np.unique(cov0)) <= {0, 255}
        assert np.array_equal(cov == 255, cov0 == 255) and np.array_equal(lab[cov == 255], lab0[cov == 255])
        assert (lab[cov == 0] == 0).all()
        everywhere = read(outs["inf"], "covered", t)
        assert set(np.unique(everywhere)) <= {128, 255} and np.array_equal(everywhere == 255, cov0 == 255)
        if t == 0:
            assert (cov == 255).all()
            continue
        assert set(np.unique(cov)) == {0, 128, 255}
        # the left strip, away from the bottom rows: columns [dx*t - 2, dx*t) take the label of column dx*t
        rows = slice(0, H - 8)
        edge = dx * t
        assert (cov[rows, edge:] == 255).all() and (cov[rows, edge - 2:edge] == 128).all()
        assert (cov[rows, :edge - 2] == 0).all()
        for x in (edge - 2, edge - 1):
            assert np.array_equal(lab[rows, x], lab[rows, edge])
    with pytest.raises(SystemExit):
        cli.parse_args(["--dense", "--deltas", "1", "--inpaint", "2"])
    with pytest.raises(SystemExit):
        cli.parse_args(base + ["--inpaint", "2.5"])
    with pytest.raises(SystemExit):
        cli.parse_args(base + ["--inpaint", "-1"])

"""Inputs shared by tests/test_fb_check_cpu.py and tests/test_fb_check_gpu.py
(not a test module): the smooth forward / backward flow pairs, the comparison
of an op's output with the fp64 oracle, the hand-worked edge cases with their
expected values, and the stub model of the tracker tests."""
import math

import torch
import torch.nn as nn

from raft_stir_amd.export.pointtrack import sample_points
from raft_stir_amd.ops import reference

from warm_start_cases import smooth

ALPHA = (0.01, 0.5)
EPS = 2.0 ** -24
INF = float("inf")
NAN = float("nan")

# (B, H, W) -> amplitude of the forward flow.  The amplitude grows with the
# field so that at every size a part of the targets leaves the image and the
# rest splits between the two classes of the check.  On 2x2 any vector longer
# than one pixel leaves the image from every pixel, and every pixel is a corner
# that half of all directions leave: amplitude 0.5, and of the seeds 0-3 the one
# (2) whose field keeps a target inside (one pixel ok, three not).
DENSE_SHAPES = [(1, 2, 2), (1, 5, 7), (1, 16, 20), (2, 33, 70), (1, 128, 160)]
AMP = {(2, 2): 0.5, (5, 7): 2, (16, 20): 3, (33, 70): 4, (128, 160): 6}
SEED = {(2, 2): 2}  # 0 elsewhere
POINT_COUNTS = [1, 16, 70, 1000]
POINT_SHAPE = (2, 33, 70)


def flow_pair(B, H, W):
    """fw, bw (B,2,H,W): bw is the negated forward field plus a smooth
    disturbance, so that the check passes at some pixels and fails at others."""
    seed = SEED.get((H, W), 0)
    fw = torch.stack([smooth(H, W, seed + b, AMP[(H, W)], 0.2) for b in range(B)])
    bw = torch.stack([-fw[b] + smooth(H, W, seed + b + 100, 0.4, 0.05) for b in range(B)])
    return fw, bw


def points_for(N, seed=None):
    """(2,N,2) xy points uniform in [-2, W+1] x [-2, H+1] of the POINT_SHAPE
    fields, so that some start outside the image."""
    B, H, W = POINT_SHAPE
    g = torch.Generator().manual_seed(1000 + N if seed is None else seed)
    r = torch.rand(B, N, 2, generator=g)
    return r * torch.tensor([W + 3.0, H + 3.0]) - 2.0


def _grid(B, H, W):
    ys, xs = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    return xs.reshape(1, -1).float().expand(B, -1), ys.reshape(1, -1).float().expand(B, -1)


def _check_mask(name, ok, ok64, start_ok, inside, e2, m2, M, alpha, min_class):
    """ok against the oracle's outside the rounding band of the threshold.
    Returns (pixels left out, fraction ok, fraction not ok)."""
    thr = alpha[0] * m2 + alpha[1]
    band = start_ok & inside & ((e2 - thr).abs() <= 64 * EPS * (2 * M) ** 2)
    n = ok.numel()
    assert band.sum().item() <= 0.01 * n, f"{name}: {band.sum().item()} of {n} in the threshold band"
    assert torch.equal(ok[~band], ok64[~band]), f"{name}: {(ok != ok64)[~band].sum().item()} mask mismatches"
    f_ok, f_no = ok64.float().mean().item(), 1 - ok64.float().mean().item()
    if min_class:
        assert f_ok >= min_class and f_no >= min_class, f"{name}: classes {f_ok:.3f} / {f_no:.3f}"
    return int(band.sum()), f_ok, f_no


def check_dense(name, fw, bw, err, ok, alpha=ALPHA, min_class=0.05):
    """err (B,1,H,W) fp32 and ok (B,1,H,W) bool (on the CPU) of fb_consistency
    against the fp64 oracle.  Returns the largest |err - err64| / M."""
    B, _, H, W = fw.shape
    assert err.shape == (B, 1, H, W) and err.dtype == torch.float32, name
    assert ok.shape == (B, 1, H, W) and ok.dtype == torch.bool, name
    err64, ok64 = reference.fb_consistency(fw, bw, *alpha, dtype=torch.float64)
    M = max(fw.abs().max().item(), bw.abs().max().item())
    fin = torch.isfinite(err64)
    assert torch.equal(err == INF, err64 == INF), f"{name}: +inf pattern"
    worst = (err[fin].double() - err64[fin]).abs().max().item() if fin.any() else 0.0
    print(f"{name}: max |err - err64| = {worst / (EPS * M):.2f} * 2^-24 * M")
    assert worst <= 32 * EPS * M, f"{name}: err off by {worst / (EPS * M):.1f} * 2^-24 * M"
    px, py = _grid(B, H, W)
    f = fw.double().reshape(B, 2, H * W)
    inside, e2, m2 = reference.fb_terms(bw, px, py, f[:, 0], f[:, 1], torch.float64)
    left, f_ok, f_no = _check_mask(name, ok.reshape(B, -1), ok64.reshape(B, -1), torch.ones_like(inside), inside,
                                   e2, m2, M, alpha, min_class)
    print(f"{name}: {left} pixels in the band, ok {f_ok:.3f}, not ok {f_no:.3f}")
    return worst / M


def check_points(name, fw, bw, pts, new, err, ok, alpha=ALPHA, min_class=0.05):
    """new (B,N,2), err (B,N) fp32 and ok (B,N) bool (on the CPU) of
    fb_track_points against the fp64 oracle.  Returns the largest error / M."""
    B, _, H, W = fw.shape
    N = pts.shape[1]
    assert new.shape == (B, N, 2) and new.dtype == torch.float32, name
    assert err.shape == (B, N) and err.dtype == torch.float32 and ok.shape == (B, N) and ok.dtype == torch.bool, name
    new64, err64, ok64 = reference.fb_track_points(fw, bw, pts, *alpha, dtype=torch.float64)
    M = max(fw.abs().max().item(), bw.abs().max().item())
    fin = torch.isfinite(err64)
    assert torch.equal(err == INF, err64 == INF), f"{name}: +inf pattern"
    worst = (new.double() - new64).abs().max().item()
    if fin.any():
        worst = max(worst, (err[fin].double() - err64[fin]).abs().max().item())
    print(f"{name}: max error of new_points and err = {worst / (EPS * M):.2f} * 2^-24 * M")
    assert worst <= 32 * EPS * M, f"{name}: off by {worst / (EPS * M):.1f} * 2^-24 * M"
    px, py = pts[..., 0], pts[..., 1]
    start_ok = (px >= 0) & (px <= W - 1) & (py >= 0) & (py <= H - 1)
    uv = new64 - pts.double()
    inside, e2, m2 = reference.fb_terms(bw, px, py, uv[..., 0], uv[..., 1], torch.float64)
    left, f_ok, f_no = _check_mask(name, ok, ok64, start_ok, inside, e2, m2, M, alpha, min_class)
    print(f"{name}: {left} points in the band, ok {f_ok:.3f}, not ok {f_no:.3f}")
    return worst / M


def check_against_sample_points(name, fw, pts, new):
    """new_points of in-image points against today's path, points +
    sample_points(fw, points), image by image (sample_points takes batch 1)."""
    B, _, H, W = fw.shape
    M = fw.abs().max().item()
    G = max((fw[..., :, 1:] - fw[..., :, :-1]).abs().max().item(),
            (fw[..., 1:, :] - fw[..., :-1, :]).abs().max().item())
    tol = 32 * EPS * M + 2.0 ** -21 * max(H, W) * G  # grid_sample's coordinate round trip through [-1, 1]
    worst, count = 0.0, 0
    for b in range(B):
        p = pts[b:b + 1]
        inim = (p[..., 0] >= 0) & (p[..., 0] <= W - 1) & (p[..., 1] >= 0) & (p[..., 1] <= H - 1)
        want = p + sample_points(fw[b:b + 1], p)
        if inim.any():
            worst = max(worst, (new[b:b + 1] - want)[inim].abs().max().item())
            count += int(inim.sum())
    print(f"{name}: {count} in-image points, max |new - today's| = {worst:.3e}, tolerance {tol:.3e}")
    assert worst <= tol, f"{name}: {worst:.3e} > {tol:.3e}"
    return worst, count


# ------------------------------------------------------------ hand-worked cases
def _const(H, W, dx, dy):
    return torch.stack([torch.full((H, W), float(dx)), torch.full((H, W), float(dy))])[None]


def constant_case():
    """fw = (3,-2), bw = (-3,2) on 6x9 (H = 6, W = 9): the target of (x, y) is
    (x+3, y-2), inside iff x <= 5 and y >= 2 (x = 5 lands exactly on x = W-1,
    y = 2 exactly on y = 0); there the point comes home exactly."""
    H, W = 6, 9
    ok = torch.zeros(1, 1, H, W, dtype=torch.bool)
    ok[..., 2:, :6] = True
    err = torch.full((1, 1, H, W), INF)
    err[ok] = 0.0
    return _const(H, W, 3, -2), _const(H, W, -3, 2), err, ok


def constant_case_bottom_right():
    """fw = (2,1), bw = (-2,-1) on 6x9: targets exactly on x = W-1 (x = 6) and
    on y = H-1 (y = 4) are inside."""
    H, W = 6, 9
    ok = torch.zeros(1, 1, H, W, dtype=torch.bool)
    ok[..., :5, :7] = True
    err = torch.full((1, 1, H, W), INF)
    err[ok] = 0.0
    return _const(H, W, 2, 1), _const(H, W, -2, -1), err, ok


def inclusive_case():
    """fw = (1,0), bw = 0 on 4x5: e2 = 1 wherever the target is inside
    (x <= 3), m2 = 1.  alpha = (0, 1.0): 1 <= 1 holds; (0, 0.999): it does not."""
    H, W = 4, 5
    inside = torch.zeros(1, 1, H, W, dtype=torch.bool)
    inside[..., :4] = True
    err = torch.full((1, 1, H, W), INF)
    err[inside] = 1.0
    return _const(H, W, 1, 0), torch.zeros(1, 2, H, W), err, inside, torch.zeros_like(inside)


BAD_FW_CELLS = [(0, 3, 4, NAN), (1, 5, 6, NAN), (0, 7, 1, INF), (1, 9, 12, INF), (0, 11, 19, -INF),
                (1, 2, 2, -INF), (0, 13, 10, 1e30), (1, 14, 3, 1e30)]  # (channel, y, x, value)


def bad_fw_case():
    """The 16x20 pair and the same with NaN / +Inf / -Inf / 1e30 in single
    cells of fw.  Those pixels are not ok with err = +inf; the dense form reads
    fw at the pixel itself only, so every other pixel is unchanged."""
    fw, bw = flow_pair(1, 16, 20)
    bad = fw.clone()
    hit = torch.zeros(1, 1, 16, 20, dtype=torch.bool)
    for c, y, x, v in BAD_FW_CELLS:
        bad[0, c, y, x] = v
        hit[0, 0, y, x] = True
    return fw, bad, bw, hit


def bad_bw_case():
    """The 16x20 pair and the same with one NaN cell (channel 1, y = 7, x = 9)
    in bw.  A pixel reads that cell with a non-zero weight iff its fp32 target
    q = p + fw is inside the image and within less than one pixel of the cell
    in both axes (the weight of a tap at distance d along an axis is 1 - d)."""
    fw, bw = flow_pair(1, 16, 20)
    bad = bw.clone()
    yc, xc = 7, 9
    bad[0, 1, yc, xc] = NAN
    px, py = _grid(1, 16, 20)
    qx, qy = px + fw[:, 0].reshape(1, -1), py + fw[:, 1].reshape(1, -1)
    inside = (qx >= 0) & (qx <= 19) & (qy >= 0) & (qy <= 15)
    hit = inside & ((qx - xc).abs() < 1) & ((qy - yc).abs() < 1)
    assert hit.sum() >= 2
    return fw, bw, bad, hit.reshape(1, 1, 16, 20)


def point_edge_case():
    """6x9 fields (H = 6, W = 9): fw = (1 - 0.25 x, -0.25 y), linear, so its
    bilinear sample inside the image is the function itself; bw = (1, 1.25)
    constant.  All values are exact in fp32.
      (-0.5, 3)   start outside.  Taps x = -1 (outside, zero) and x = 0 with weight 0.5 each:
                  S = 0.5 * (1, -0.75) = (0.5, -0.375), new = (0, 2.625); ok = 0, err = +inf.
      (8, 5)      = (W-1, H-1), inside.  (u, v) = (-1, -1.25), new = q = (7, 3.75), inside;
                  bw there is (1, 1.25): e2 = 0, err = 0, ok = 1.
      (8.5, 2)    start outside.  Tap x = 8 with weight 0.5: S = 0.5 * (-1, -0.5), new = (8, 1.75).
      (nan, 2)    S = 0 by the rule, new = (nan, 2); ok = 0, err = +inf.
      (1e30, 1)   S = 0, new = (1e30, 1); ok = 0, err = +inf.
      (4, 2)      inside.  (u, v) = (0, -0.5), q = (4, 1.5); (u+bu, v+bv) = (1, 0.75):
                  e2 = 1.5625, err = 1.25; m2 = 0.25 + 1 + 1.5625 = 2.8125 and
                  0.01 * 2.8125 + 0.5 < 1.5625: ok = 0.
      (4.5, 2.5)  inside.  (u, v) = (-0.125, -0.625), q = (4.375, 1.875); sum = (0.875, 0.625):
                  e2 = 1.15625; with alpha = (0, 2): ok = 1 (checked with ALPHA: ok = 0).
    """
    H, W = 6, 9
    ys, xs = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    fw = torch.stack([1 - 0.25 * xs.float(), -0.25 * ys.float()])[None]
    bw = _const(H, W, 1, 1.25)
    pts = torch.tensor([[[-0.5, 3], [8, 5], [8.5, 2], [NAN, 2], [1e30, 1], [4, 2], [4.5, 2.5]]])
    new = torch.tensor([[[0, 2.625], [7, 3.75], [8, 1.75], [NAN, 2], [1e30, 1], [4, 1.5], [4.375, 1.875]]])
    err = torch.tensor([[INF, 0.0, INF, INF, INF, 1.25, math.sqrt(1.15625)]])
    ok = torch.tensor([[False, True, False, False, False, False, False]])
    ok_loose = torch.tensor([[False, True, False, False, False, True, True]])  # alpha = (0, 2)
    return fw, bw, pts, new, err, ok, ok_loose


def check_edge_cases(dense, points):
    """dense(fw, bw, a1, a2) -> (err, ok) and points(fw, bw, pts, a1, a2) ->
    (new, err, ok), CPU tensors in and out: the implementation under test."""
    for case in (constant_case, constant_case_bottom_right):
        fw, bw, want_err, want_ok = case()
        err, ok = dense(fw, bw, *ALPHA)
        assert torch.equal(err, want_err) and torch.equal(ok, want_ok), case.__name__
    fw, bw, want_err, ok_incl, ok_excl = inclusive_case()
    err, ok = dense(fw, bw, 0.0, 1.0)
    assert torch.equal(err, want_err) and torch.equal(ok, ok_incl), "inclusive test"
    err, ok = dense(fw, bw, 0.0, 0.999)
    assert torch.equal(err, want_err) and torch.equal(ok, ok_excl), "just below the threshold"
    # non-finite and huge cells of fw
    fw, bad, bw, hit = bad_fw_case()
    clean_err, clean_ok = dense(fw, bw, *ALPHA)
    err, ok = dense(bad, bw, *ALPHA)
    assert (err[hit] == INF).all() and not ok[hit].any()
    assert torch.equal(err[~hit], clean_err[~hit]) and torch.equal(ok[~hit], clean_ok[~hit])
    # a NaN cell of bw
    fw, bw, bad, hit = bad_bw_case()
    clean_err, clean_ok = dense(fw, bw, *ALPHA)
    err, ok = dense(fw, bad, *ALPHA)
    assert not ok[hit].any()
    assert torch.equal(err[~hit], clean_err[~hit]) and torch.equal(ok[~hit], clean_ok[~hit])
    assert torch.isfinite(clean_err[hit]).all() and clean_ok[hit].any()  # the NaN, not the field, fails them
    # points on and off the border, NaN and huge
    fw, bw, pts, want_new, want_err, want_ok, ok_loose = point_edge_case()
    new, err, ok = points(fw, bw, pts, *ALPHA)
    assert same(new, want_new), new
    assert torch.equal(err, want_err), err
    assert torch.equal(ok, want_ok), ok
    new, err, ok = points(fw, bw, pts, 0.0, 2.0)
    assert same(new, want_new) and torch.equal(err, want_err) and torch.equal(ok, ok_loose), ok


def same(a, b):
    """Bit-equal, NaN equal to NaN."""
    return a.shape == b.shape and a.dtype == b.dtype and bool(((a == b) | ((a != a) & (b != b))).all())


# ----------------------------------------------------------------- tracker stub
STUB_D = (3.0, -2.0)
STUB_RECT = (40, 72, 64, 104)  # y0, y1, x0, x1 of the rectangle where the backward flow is off by (5, 5)
# 64x128 frames.  A point p moves to p + d every step; it is visible iff its target is inside the
# image and outside the rectangle (there the backward vector is -d + (5,5): it misses home by sqrt(50)).
STUB_POINTS = [[10.0, 20.0],     # far from the rectangle: visible on every step
               [70.0, 50.0],     # targets (73,48), (76,46), (79,44): inside the rectangle, never visible
               [59.5, 60.5],     # targets (62.5,58.5) outside; (65.5,56.5), (68.5,54.5) well inside
               [120.5, 30.0],    # targets (123.5,28), (126.5,26) in the image; (129.5,24) has left it (W-1 = 127)
               [100.0, 43.0]]    # targets (103,41) inside; (106,39), (109,37) outside (above / right of it)
STUB_VISIBLE = [[True, True, True, True, True],       # the first frame
                [True, False, True, True, False],
                [True, False, False, True, True],
                [True, False, False, False, True]]
STUB_ERR_MISS = math.sqrt(50.0)


class StubFlow(nn.Module):
    """A 'model' whose bidirectional pass returns +d for the forward half and
    -d for the backward half of the batch at both resolutions (the backward
    full-resolution field offset by (5,5) inside STUB_RECT), from plain torch
    ops on its inputs, so that it can be captured.  The weight is ignored."""

    def __init__(self, H=64, W=128):
        super().__init__()
        self.weight = nn.Parameter(torch.zeros(1))
        self.register_buffer("d", torch.tensor(STUB_D).view(1, 2, 1, 1))
        off = torch.zeros(1, 2, H, W)
        y0, y1, x0, x1 = STUB_RECT
        off[..., y0:y1, x0:x1] = 5.0
        self.register_buffer("off", off)
        self.calls = 0

    def forward(self, image1, image2, iters=12, flow_init=None, test_mode=False, bidirectional=False):
        assert test_mode and bidirectional and flow_init.shape[0] == 2 * image1.shape[0]
        self.calls += 1
        zero = image1[:, :2] * 0 + image2[:, :2] * 0  # (B,2,H,W)
        up = torch.cat([zero + self.d, zero - self.d + self.off])
        lo = torch.cat([zero[..., ::8, ::8] + self.d / 8, zero[..., ::8, ::8] - self.d / 8]) + 0 * flow_init
        return lo, up


def stub_sequence():
    g = torch.Generator().manual_seed(3)
    return torch.rand(4, 1, 3, 64, 128, generator=g) * 255, torch.tensor([STUB_POINTS])


def check_stub_tracking(traj, vis, err, points):
    """traj (4,N,2), vis (4,N) bool, err (4,N) on the CPU."""
    d = torch.tensor(STUB_D)
    assert traj.shape == (4, 5, 2) and vis.shape == (4, 5) and err.shape == (4, 5)
    assert vis.dtype == torch.bool and err.dtype == torch.float32
    assert torch.equal(traj[0], points[0])
    for t in range(4):
        assert torch.equal(traj[t], points[0] + t * d), t  # positions advance by d regardless
    want = torch.tensor(STUB_VISIBLE)
    assert torch.equal(vis, want), vis
    assert (err[0] == 0).all()
    left = torch.zeros(4, 5, dtype=torch.bool)
    left[3, 3] = True  # the point that left the image
    assert (err[left] == INF).all()
    assert (err[want] == 0).all()
    miss = ~want & ~left
    torch.testing.assert_close(err[miss], torch.full((int(miss.sum()),), STUB_ERR_MISS), rtol=4 * EPS, atol=0)

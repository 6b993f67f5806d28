"""Inputs shared by tests/test_warm_start_cpu.py and tests/test_warm_start_gpu.py
(not a test module): the smooth flow generator, the edge inputs of forward
interpolation with their expected outputs, and the fp64 property check."""
import numpy as np
import torch
import torch.nn.functional as F

FAR = 1000.0  # a flow that moves every sample of these small fields off the grid


def smooth(H, W, seed, amp, noise):
    g = torch.Generator().manual_seed(seed)
    lo = torch.randn(1, 2, max(2, H // 8), max(2, W // 8), generator=g) * amp
    f = F.interpolate(lo, size=(H, W), mode="bilinear", align_corners=True)[0]
    return f + noise * torch.randn(2, H, W, generator=g)


def brute_force(flow):
    """The rule in numpy fp64 with an explicit lowest-index tie break, for one
    (2,H,W) flow whose positions and distances are exact in fp64 and fp32
    alike (integer or half-integer flows)."""
    f = flow.numpy().astype(np.float64)
    _, H, W = f.shape
    ys, xs = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    x1, y1 = (xs + f[0]).reshape(-1), (ys + f[1]).reshape(-1)
    ok = (x1 > 0) & (x1 < W) & (y1 > 0) & (y1 < H)
    out = np.zeros_like(f)
    if not ok.any():
        return torch.from_numpy(out).float()
    for qy in range(H):
        for qx in range(W):
            d2 = np.where(ok, (qx - x1) ** 2 + (qy - y1) ** 2, np.inf)
            s = int(np.flatnonzero(d2 == d2.min())[0])
            out[:, qy, qx] = f[:, s // W, s % W]
    return torch.from_numpy(out).float()


def _fill(H, W, cells):
    """(2,H,W) flow, FAR everywhere (invalid) except cells {(x, y): (dx, dy)}."""
    f = torch.full((2, H, W), FAR)
    for (x, y), (dx, dy) in cells.items():
        f[0, y, x], f[1, y, x] = dx, dy
    return f


def _const(H, W, dx, dy):
    return torch.stack([torch.full((H, W), float(dx)), torch.full((H, W), float(dy))])


def edge_cases():
    """[(name, flow (B,2,H,W), expected (B,2,H,W))]; every expected output is
    worked out by hand or by brute_force, never by the code under test."""
    cases = []
    cases.append(("all_invalid", _fill(6, 9, {})[None], torch.zeros(1, 2, 6, 9)))
    cases.append(("one_valid", _fill(6, 9, {(3, 2): (0.5, 0.25)})[None], _const(6, 9, 0.5, 0.25)[None]))
    # samples landing exactly on x = 0, x = W, y = H and y = 0 of a 4x5 field
    on_edge = {(2, 1): (-2.0, 0.0), (1, 2): (4.0, 0.0), (3, 0): (0.0, 4.0), (1, 3): (0.0, -3.0)}
    cases.append(("on_boundary_invalid", _fill(4, 5, on_edge)[None], torch.zeros(1, 2, 4, 5)))
    inside = dict(on_edge)
    inside[(2, 2)] = (0.5, -0.5)
    cases.append(("on_boundary_plus_one_inside", _fill(4, 5, inside)[None], _const(4, 5, 0.5, -0.5)[None]))
    # 3x4 by hand.  A = cell (1,1), index 5, moves to (1.5, 1); B = cell (3,1), index 7, moves to
    # (2.5, 1).  Columns 0-1 are nearer to A, column 3 to B, column 2 is at 0.5 from both: A (lower index).
    f = _fill(3, 4, {(1, 1): (0.5, 0.0), (3, 1): (-0.5, 0.0)})
    want = torch.zeros(2, 3, 4)
    want[0] = torch.tensor([0.5, 0.5, 0.5, -0.5]).expand(3, 4)
    cases.append(("tie_3x4_lower_index_left", f[None], want[None]))
    # the same with the samples crossing: A moves to (2.5, 1), B to (1.5, 1).  Columns 0-1 take B,
    # column 3 takes A, the tie in column 2 again goes to A, now the sample on the right.
    f = _fill(3, 4, {(1, 1): (1.5, 0.0), (3, 1): (-1.5, 0.0)})
    want = torch.zeros(2, 3, 4)
    want[0] = torch.tensor([-1.5, -1.5, 1.5, 1.5]).expand(3, 4)
    cases.append(("tie_3x4_lower_index_right", f[None], want[None]))
    # integer flow: rows >= 8 move by (3, -2) onto cells that rows < 8 (flow 0) already hold
    f = torch.zeros(2, 16, 20)
    f[0, 8:], f[1, 8:] = 3.0, -2.0
    cases.append(("tie_integer_16x20", f[None], brute_force(f)[None]))
    # NaN / +Inf / -Inf cells are invalid: the result is that of the same field with those
    # samples moved far off the grid, and it is finite
    f = smooth(16, 20, 0, 1, 0.1)
    bad, far = f.clone(), f.clone()
    for c, y, x, v in [(0, 3, 4, float("nan")), (1, 5, 6, float("nan")), (0, 7, 1, float("inf")),
                       (1, 9, 12, float("inf")), (0, 11, 19, float("-inf")), (1, 2, 2, float("-inf")),
                       (0, 15, 10, float("nan"))]:
        bad[c, y, x] = v
        far[:, y, x] = FAR
    cases.append(("nonfinite_cells", bad[None], None))  # expected: see nonfinite_twin
    cases.append(("nonfinite_twin", far[None], None))
    # two images in one batch are independent: image 1 all invalid, image 0 the one-valid field
    two = torch.stack([_fill(6, 9, {(3, 2): (0.5, 0.25)}), _fill(6, 9, {})])
    cases.append(("batch_independent", two, torch.stack([_const(6, 9, 0.5, 0.25), torch.zeros(2, 6, 9)])))
    return cases


def check_edge_outputs(outs):
    """outs: {name: output (B,2,H,W) on the CPU} for every case of edge_cases()."""
    for name, _, want in edge_cases():
        if want is not None:
            assert torch.equal(outs[name], want), name
    bad, twin = outs["nonfinite_cells"], outs["nonfinite_twin"]
    assert torch.isfinite(bad).all()
    assert torch.equal(bad, twin)


def check_against_fp64(flow, out):
    """One (2,H,W) flow and its output: every returned vector is bit-equal to
    the flow of a valid sample whose fp64 distance (from the fp32 positions) is
    within 2**-21 * max(H, W) of the smallest one; zeros without a valid sample."""
    _, H, W = flow.shape
    N = H * W
    ys, xs = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    gx, gy = xs.reshape(-1).float(), ys.reshape(-1).float()
    f = flow.reshape(2, N)
    x1, y1 = gx + f[0], gy + f[1]  # fp32 positions
    ok = (x1 > 0) & (x1 < W) & (y1 > 0) & (y1 < H)
    o = out.reshape(2, N)
    if not ok.any():
        assert (o == 0).all()
        return 0
    d = ((gx.double()[:, None] - x1.double()[None]) ** 2 + (gy.double()[:, None] - y1.double()[None]) ** 2).sqrt()
    inf = torch.tensor(float("inf"), dtype=torch.float64)
    d = torch.where(ok[None], d, inf)
    dmin = d.min(dim=1).values
    same = (f[0][None] == o[0][:, None]) & (f[1][None] == o[1][:, None]) & ok[None]
    assert same.any(dim=1).all(), "an output vector is not the flow of a valid sample"
    got = torch.where(same, d, inf).min(dim=1).values
    assert (got <= dmin + 2.0 ** -21 * max(H, W)).all(), float((got - dmin).max())
    return int(ok.sum())

"""Correlation kernels at edge inputs vs ops/reference.py in fp64 on the CPU.

csrc/corr_lookup.hip (generic and wave-per-pixel lookups, forward and
backward, every radius 0..4 and 1..4 levels, fp32 / bf16 pyramids and outputs,
compact and pitched rows, padded output / gradient rows) and
csrc/corr_onthefly.hip (tiled MFMA forward, MFMA and VALU tiled backward) with
coordinates on integers and on the map's borders, far outside it (+-1e6,
+-3e9, 1e20: zero padding, exactly) and non-finite (that pixel NaN, nothing
else).  The oracle takes the same input values, rounded to their storage
dtype, as fp64; what it says about the extreme coordinates is pinned in
tests/test_edge_oracles_cpu.py.

Shapes: B = 2, 17 x 23 queries (P = 782: the last 4-pixel wave block is
partial), levels 17x23, 8x11, 4x5, 2x2.

Bounds.  Lookup, fp32 output: atol = rtol = 1e-5 (the figure of
test_kernels_gpu.py for this op; the reference's own fp32-vs-fp64 gap is 5e-6
at these shapes), bf16 output: + 2^-8 |want| (one bf16 rounding).  Lookup
backward: atol = rtol = 1e-5.  On-the-fly: those of test_onthefly_tiled_*.
Measured on an MI355X (largest |err| and largest |err| / bound over all
cases; every test prints its own figures as it runs):
  lookup forward, fp32 output    4.3e-6   0.32
  lookup forward, bf16 output    7.8e-3   0.99  (a bf16 rounding is up to 2^-8 |want|: the bound is tight)
  lookup backward                6.6e-7   0.03
  on-the-fly forward, fp32 out   7.3e-7   < 0.001
  on-the-fly forward, bf16 out   7.8e-3   0.13
  on-the-fly backward, df1       7.9e-6   0.07
  on-the-fly backward, df2       1.6e-5   0.12
"""
import functools
import math

import pytest
import torch
import torch.nn.functional as F

from raft_stir_amd.ops import reference as ref

pytestmark = pytest.mark.gpu

B, H1, W1 = 2, 17, 23
N1 = H1 * W1
HUGE = [(0, 5, 3, 0, 1e6), (1, 6, 4, 1, -1e6), (0, 7, 20, 0, 3e9), (1, 8, 10, 1, -3e9), (1, 16, 22, 0, 1e20)]
NONFINITE = [(0, 4, 4, 0, math.inf), (1, 9, 9, 1, -math.inf), (1, 16, 21, 0, math.nan)]
F32, BF16 = torch.float32, torch.bfloat16


def _round_up(a, b):
    return (a + b - 1) // b * b


def _bound(want, out_dtype, tol=1e-5):
    b = tol + tol * want.abs()
    return b + 2.0 ** -8 * want.abs() if out_dtype == BF16 else b


def _check(name, got, want, bound):
    err = (got.double() - want).abs()
    finite = torch.isfinite(want)
    assert bool(torch.isfinite(got.double()[finite]).all()), name
    ratio = (err[finite] / bound[finite]).max().item()
    print(f"{name}: max|err| {err[finite].max().item():.3e}  err/bound {ratio:.3f}")
    assert ratio <= 1.0, f"{name}: err/bound {ratio:.3f}"


# ------------------------------------------------------------------ inputs
@functools.lru_cache(None)
def _coords(seed=1):
    """(plain, huge, nonfinite) fp32 coordinates: grid + 6 randn with exact
    integers (rows 0-2) and the map's borders planted; `huge` / `nonfinite`
    differ from `plain` only at the pixels of HUGE / NONFINITE."""
    g = torch.Generator().manual_seed(seed)
    c = ref.coords_grid(B, H1, W1) + 6.0 * torch.randn(B, 2, H1, W1, generator=g)
    c[:, :, 0:3] = c[:, :, 0:3].round()
    for i, v in enumerate([-1.0, -0.5, W1 - 1.0, W1 - 0.5, 0.0]):
        c[i % B, 0, 10, 2 + 3 * i] = v
    for i, v in enumerate([-1.0, -0.5, H1 - 1.0, H1 - 0.5, 0.0]):
        c[(i + 1) % B, 1, 11, 2 + 3 * i] = v
    c[0, :, 12, 5] = torch.tensor([W1 - 1.0, H1 - 1.0])  # the last cell, exactly
    huge, bad = c.clone(), c.clone()
    for b, y, x, ch, v in HUGE:
        huge[b, ch, y, x] = v
    for b, y, x, ch, v in NONFINITE:
        bad[b, ch, y, x] = v
    return c, huge, bad


@functools.lru_cache(None)
def _pyr_cpu(dtype, seed=0):
    """Random pyramid levels (B, N1, H_l, W_l), rounded to `dtype`, as fp32."""
    g = torch.Generator().manual_seed(seed)
    return tuple(torch.randn(B, N1, H1 >> l, W1 >> l, generator=g).to(dtype).float() for l in range(4))


@functools.lru_cache(None)
def _want_lookup(radius, levels, dtype, which):
    pyr = [p.double().reshape(B * N1, 1, p.shape[2], p.shape[3]) for p in _pyr_cpu(dtype)[:levels]]
    c = _coords()[which].double()
    return ref.corr_lookup(pyr, c, radius).permute(0, 2, 3, 1).contiguous()  # (B, H1, W1, CH)


def _pitched(t, dev, dtype, fill):
    """`t` (B, N, h, w) as a view with row pitch S % 64 == 0, S > h*w, over a
    buffer prefilled with `fill`; returns (view, buffer as (B*N, S))."""
    Bn, N, h, w = t.shape
    S = _round_up(h * w + 1, 64)
    store = torch.full((Bn * N * S,), fill, device=dev, dtype=dtype)
    view = store.as_strided((Bn, N, h, w), (N * S, S, w, 1))
    view.copy_(t.to(dev))
    return view, store.view(Bn * N, S)


def _gpu_pyr(levels, dtype, dev, pitched):
    if pitched:
        return [_pitched(p, dev, dtype, math.nan)[0] for p in _pyr_cpu(dtype)[:levels]]
    return [p.to(dev, dtype).contiguous() for p in _pyr_cpu(dtype)[:levels]]


def _mask(pixels):
    m = torch.zeros(B, H1, W1, dtype=torch.bool)
    for b, y, x, _, _ in pixels:
        m[b, y, x] = True
    return m


# ------------------------------------------------------------------ lookup forward
def _lookup_case(cuda, radius, levels, pdt, odt, pitched):
    R = torch.ops.raft_stir
    pyr = _gpu_pyr(levels, pdt, cuda, pitched)
    plain, huge, _ = _coords()
    CH = levels * (2 * radius + 1) ** 2
    tag = f"lookup r={radius} L={levels} pyr={pdt} out={odt} pitched={pitched}"
    got = R.corr_lookup(pyr, plain.to(cuda), radius, odt == BF16).cpu()
    assert got.shape == (B, H1, W1, CH) and got.dtype == odt
    want = _want_lookup(radius, levels, pdt, 0)
    _check(tag, got, want, _bound(want, odt))
    # far outside the map: that pixel exactly 0, every other pixel as before, bit for bit
    goth = R.corr_lookup(pyr, huge.to(cuda), radius, odt == BF16).cpu()
    m = _mask(HUGE)
    assert bool((goth[m] == 0).all()), tag
    assert torch.equal(goth[~m], got[~m]), tag
    wanth = _want_lookup(radius, levels, pdt, 1)
    assert bool((wanth[m] == 0).all())
    # corr_lookup_into: 64-aligned rows wider than CH, prefilled with NaN
    OW = _round_up(CH + 1, 64)
    out = torch.full((B, H1, W1, OW), math.nan, device=cuda, dtype=odt)
    R.corr_lookup_into(pyr, huge.to(cuda), radius, out)
    out = out.cpu()
    assert bool((out[..., CH:] == 0).all()), tag + " pad"
    assert torch.equal(out[..., :CH], goth), tag + " payload"


@pytest.mark.parametrize("levels", [1, 2, 3, 4])
@pytest.mark.parametrize("radius", [0, 1, 2, 3, 4])
def test_lookup_forward_fp32_grid(cuda, radius, levels):
    _lookup_case(cuda, radius, levels, F32, F32, False)


@pytest.mark.parametrize("pdt,odt,pitched", [(F32, F32, True), (F32, BF16, False), (BF16, F32, False),
                                             (BF16, BF16, False), (BF16, F32, True), (BF16, BF16, True),
                                             (F32, BF16, True)])
@pytest.mark.parametrize("radius,levels", [(2, 4), (4, 4), (2, 3), (4, 2)])
def test_lookup_forward_dtypes_and_pitch(cuda, radius, levels, pdt, odt, pitched):
    _lookup_case(cuda, radius, levels, pdt, odt, pitched)


@pytest.mark.parametrize("pdt,odt", [(F32, F32), (BF16, BF16)])
@pytest.mark.parametrize("radius,levels", [(0, 1), (2, 4), (3, 3), (4, 4)])
def test_lookup_forward_nonfinite_coordinates(cuda, radius, levels, pdt, odt):
    """+inf, -inf, NaN: that pixel all NaN (as the reference's sampler), every
    other pixel bit-identical to the run with an ordinary coordinate there."""
    R = torch.ops.raft_stir
    pyr = _gpu_pyr(levels, pdt, cuda, True)
    plain, _, bad = _coords()
    CH = levels * (2 * radius + 1) ** 2
    got = R.corr_lookup(pyr, plain.to(cuda), radius, odt == BF16).cpu()
    gotb = R.corr_lookup(pyr, bad.to(cuda), radius, odt == BF16).cpu()
    m = _mask(NONFINITE)
    assert bool(torch.isnan(gotb[m]).all())
    assert torch.equal(gotb[~m], got[~m])
    want = _want_lookup(radius, levels, pdt, 2)
    assert bool(torch.isnan(want[m]).all()) and bool(torch.isfinite(want[~m]).all())
    out = torch.full((B, H1, W1, _round_up(CH + 1, 64)), math.nan, device=cuda, dtype=odt)
    R.corr_lookup_into(pyr, bad.to(cuda), radius, out)
    out = out.cpu()
    assert bool((out[..., CH:] == 0).all())
    assert bool(torch.isnan(out[..., :CH][m]).all()) and torch.equal(out[..., :CH][~m], got[~m])


# ------------------------------------------------------------------ lookup backward
@functools.lru_cache(None)
def _dout_cpu(radius, levels, dtype, seed):
    g = torch.Generator().manual_seed(100 + seed)
    CH = levels * (2 * radius + 1) ** 2
    return torch.randn(B, H1, W1, CH, generator=g).to(dtype).float()


@functools.lru_cache(None)
def _g0_cpu(levels):
    g = torch.Generator().manual_seed(55)
    return tuple(torch.randn(B, N1, H1 >> l, W1 >> l, generator=g) for l in range(levels))


@functools.lru_cache(None)
def _want_lookup_bwd(radius, levels, gdt):
    """G0 + d/d pyr of sum_k <lookup(pyr, coords_k), dout_k>, fp64 autograd, k = two calls."""
    leaves = [torch.zeros(B * N1, 1, H1 >> l, W1 >> l, dtype=torch.float64, requires_grad=True) for l in range(levels)]
    loss = 0.0
    for k, seed in enumerate((1, 2)):
        c = _coords(seed)[1].double()
        out = ref.corr_lookup(leaves, c, radius).permute(0, 2, 3, 1)
        loss = loss + (out * _dout_cpu(radius, levels, gdt, k).double()).sum()
    grads = torch.autograd.grad(loss, leaves)
    return [g0.double() + g.reshape(g0.shape) for g0, g in zip(_g0_cpu(levels), grads)]


def _lookup_bwd_case(cuda, radius, levels, gdt):
    R = torch.ops.raft_stir
    CH = levels * (2 * radius + 1) ** 2
    DW = _round_up(CH + 1, 64)
    tag = f"lookup_bwd r={radius} L={levels} dout={gdt}"
    gp = [_pitched(g0, cuda, F32, 7.0) for g0 in _g0_cpu(levels)]
    for k, seed in enumerate((1, 2)):
        dout = torch.full((B, H1, W1, DW), math.nan, device=cuda, dtype=gdt)
        dout[..., :CH] = _dout_cpu(radius, levels, gdt, k).to(cuda, gdt)
        R.corr_lookup_backward([v for v, _ in gp], _coords(seed)[1].to(cuda), radius, dout)
    want = _want_lookup_bwd(radius, levels, gdt)
    m = _mask(HUGE).reshape(B, N1)
    for l, (view, store) in enumerate(gp):
        hw = (H1 >> l) * (W1 >> l)
        assert bool((store[:, hw:] == 7.0).all()), tag + " pad columns"
        got = view.cpu()
        _check(f"{tag} level {l}", got, want[l], _bound(want[l], F32))
        assert torch.equal(got[m], _g0_cpu(levels)[l][m]), tag + " rows of far pixels"


@pytest.mark.parametrize("levels", [1, 2, 3, 4])
@pytest.mark.parametrize("radius", [0, 1, 2, 3, 4])
def test_lookup_backward_fp32_grid(cuda, radius, levels):
    _lookup_bwd_case(cuda, radius, levels, F32)


@pytest.mark.parametrize("radius,levels", [(2, 4), (4, 4), (2, 3), (3, 2)])
def test_lookup_backward_bf16_dout(cuda, radius, levels):
    _lookup_bwd_case(cuda, radius, levels, BF16)


@pytest.mark.parametrize("radius", [2, 4])
def test_lookup_backward_nonfinite_coordinates_touch_nothing(cuda, radius):
    R = torch.ops.raft_stir
    levels = 4
    plain, _, bad = _coords()
    dout = _dout_cpu(radius, levels, F32, 0).to(cuda)
    res = []
    for c in (plain, bad):
        gp = [_pitched(g0, cuda, F32, 7.0) for g0 in _g0_cpu(levels)]
        R.corr_lookup_backward([v for v, _ in gp], c.to(cuda), radius, dout)
        res.append([v.cpu() for v, _ in gp])
    m = _mask(NONFINITE).reshape(B, N1)
    for l in range(levels):
        assert torch.equal(res[1][l][m], _g0_cpu(levels)[l][m])
        assert torch.equal(res[1][l][~m], res[0][l][~m])


def test_lookup_backward_rejects_radius_5(cuda):
    gp = [torch.zeros(B, N1, H1, W1, device=cuda)]
    dout = torch.zeros(B, H1, W1, 128, device=cuda)
    with pytest.raises(RuntimeError, match="radius"):
        torch.ops.raft_stir.corr_lookup_backward(gp, _coords()[0].to(cuda), 5, dout)
    with pytest.raises(RuntimeError, match="radius"):
        torch.ops.raft_stir.corr_lookup(gp, _coords()[0].to(cuda), 5, False)


# ------------------------------------------------------------------ on-the-fly
OB, OH, OW_ = 2, 23, 38
DISPLACED = (0, 9, 13)   # tile (ty = 2, tx = 3): + 50 000 cells in x and y
FAR = (1, 14, 22)        # x = 3e9
OTF_BAD = [(0, 5, 6, 0, math.inf), (1, 17, 30, 1, math.nan)]


@functools.lru_cache(None)
def _otf_inputs(C):
    g = torch.Generator().manual_seed(21 + C)
    f1 = torch.randn(OB, C, OH, OW_, generator=g).bfloat16().float()
    f2 = torch.randn(OB, C, OH, OW_, generator=g).bfloat16().float()
    f2l = [f2]
    for _ in range(3):
        f2l.append(F.avg_pool2d(f2l[-1], 2, stride=2))
    f2l = [t.bfloat16().float() for t in f2l]  # pooled in fp32, stored in bf16 (as OnTheFlyCorr does)
    base = ref.coords_grid(OB, OH, OW_)
    ys, xs = base[:, 1:2], base[:, 0:1]
    flow = torch.cat([3.0 + 0.08 * xs - 0.05 * ys, -2.0 + 0.04 * ys], 1) + 0.3 * torch.randn(OB, 2, OH, OW_, generator=g)
    smooth = base + flow
    edited = smooth.clone()
    b, y, x = DISPLACED
    edited[b, :, y, x] += 50000.0
    b, y, x = FAR
    edited[b, 0, y, x] = 3e9
    bad = smooth.clone()
    for b, y, x, ch, v in OTF_BAD:
        bad[b, ch, y, x] = v
    return f1, f2l, edited, bad


def _otf_oracle(C, r, coords, f1, f2l):
    """(B, H, W, L*K2) in fp64 from the stored (bf16-rounded) feature levels."""
    delta = ref._window_delta(r, coords.device, torch.float64).reshape(-1, 2)
    pos0 = coords.double().permute(0, 2, 3, 1)
    outs = []
    for lvl, t in enumerate(f2l):
        outs += [(ref.bilinear_sampler(t, pos0 / 2 ** lvl + delta[k]) * f1).sum(1) for k in range(delta.shape[0])]
    return torch.stack(outs, -1) / math.sqrt(C)


def _otf_gpu(C, cuda):
    f1, f2l, *_ = _otf_inputs(C)
    b1 = f1.to(cuda, BF16).permute(0, 2, 3, 1).contiguous()
    b2 = [t.to(cuda, BF16).permute(0, 2, 3, 1).contiguous() for t in f2l]
    return b1, b2


@pytest.mark.parametrize("out_bf16", [False, True])
@pytest.mark.parametrize("C", [128, 96])
def test_onthefly_forward_displaced_queries(cuda, C, out_bf16):
    """One query of a coherent 4 x 4 tile 50 000 cells away in x and y (the
    tile's bounding box has 2.5e9 cells: more than an int holds) and one at
    3e9: exact zeros there, the 15 tile neighbours and everything else within
    the tolerance of test_onthefly_tiled_forward."""
    r = 4
    f1, f2l, edited, bad = _otf_inputs(C)
    b1, b2 = _otf_gpu(C, cuda)
    ftol = 2e-2 if out_bf16 else 1e-2
    want = _otf_oracle(C, r, edited, f1.double(), [t.double() for t in f2l])
    got = torch.ops.raft_stir.corr_otf(b1, b2, edited.to(cuda), r, 1.0 / math.sqrt(C), out_bf16).cpu()
    for b, y, x in (DISPLACED, FAR):
        assert bool((want[b, y, x] == 0).all()) and bool((got[b, y, x] == 0).all())
    _check(f"otf fwd C={C} bf16={out_bf16}", got, want, ftol + ftol * want.abs())
    b, y, x = DISPLACED
    tile = (slice(y // 4 * 4, y // 4 * 4 + 4), slice(x // 4 * 4, x // 4 * 4 + 4))
    _check("  the displaced query's tile", got[b][tile], want[b][tile], ftol + ftol * want[b][tile].abs())
    # non-finite queries: NaN for that query only
    wantb = _otf_oracle(C, r, bad, f1.double(), [t.double() for t in f2l])
    gotb = torch.ops.raft_stir.corr_otf(b1, b2, bad.to(cuda), r, 1.0 / math.sqrt(C), out_bf16).cpu()
    m = torch.zeros(OB, OH, OW_, dtype=torch.bool)
    for b, y, x, _, _ in OTF_BAD:
        m[b, y, x] = True
    assert bool(torch.isnan(gotb[m]).all()) and bool(torch.isnan(wantb[m]).all())
    _check(f"otf fwd non-finite C={C}", gotb[~m], wantb[~m], ftol + ftol * wantb[~m].abs())


@pytest.mark.parametrize("det", [False, True])
@pytest.mark.parametrize("C", [128, 96])
def test_onthefly_backward_displaced_queries(cuda, C, det):
    """C = 128: otf_tile_bwd_mma_kernel, C = 96: otf_tile_bwd_kernel.  The
    displaced queries add nothing to df1 or df2; bounds of test_onthefly_tiled_backward."""
    r = 4
    f1, f2l, edited, _ = _otf_inputs(C)
    a1 = f1.double().requires_grad_()
    a2 = [t.double().requires_grad_() for t in f2l]
    want = _otf_oracle(C, r, edited, a1, a2)
    g = torch.Generator().manual_seed(6)
    dout = torch.randn(want.shape, generator=g)
    (want * dout.double()).sum().backward()
    b1, b2 = _otf_gpu(C, cuda)
    torch.ops.raft_stir.set_deterministic(det)
    try:
        got = torch.ops.raft_stir.corr_otf_backward(b1, b2, edited.to(cuda), r, 1.0 / math.sqrt(C), dout.to(cuda))
    finally:
        torch.ops.raft_stir.set_deterministic(False)
    got = [t.cpu() for t in got]
    w1 = a1.grad.permute(0, 2, 3, 1)
    for b, y, x in (DISPLACED, FAR):
        assert bool((w1[b, y, x] == 0).all()) and bool((got[0][b, y, x] == 0).all())
    _check(f"otf bwd df1 C={C} det={det}", got[0], w1, 1e-4 + 1e-4 * w1.abs())
    for lvl in range(4):
        w2 = a2[lvl].grad.permute(0, 2, 3, 1)
        _check(f"otf bwd df2[{lvl}] C={C} det={det}", got[1 + lvl], w2, 1e-4 + 1e-4 * w2.abs())

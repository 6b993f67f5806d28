"""The all-pairs correlation volume, its gradient fold and its backward, per element vs fp64 oracles.

corr_volume on its three routes (csrc/corr_volume.hip: pool_f2_kernel + corr_flat_kernel<OB>
for bf16 maps, split3_kernel + the flat GEMM over K = 3C, corr_volume_f32_kernel),
pyr_grad_fold / pyr_grad_fold_bf16 on each of the four fold kernels of csrc/corr_lookup.hip, and
corr_volume_backward (csrc/corr_bwd.hip, NP = 1 and 3), at the smallest shapes that reach each
path: 1x1 and one-row grids, odd sizes at every level, one target over a 128-tile or a 4-wide
store, one query row over / under a 64- and 128-row tile, one K step, rows that are no multiple
of a block's 4, more rows than gridDim.y holds, the Gt tile that reads across a row end of G.
Which kernel a case reaches is asserted through the mirrors of tests/corr_volume_cases.py, whose
oracles, bounds and derivations tests/test_corr_volume_oracles_cpu.py holds to autograd, to a
plain emulation of every route and to 13 mutants.

Every check prints max|err| and err / bound and asserts dtype, shape, finiteness and
ratio <= 1 for EVERY element (0 / 0 counts as 0).  Gradient levels are views of NaN-filled
stores: the padding must still be NaN, bit for bit, after a fold.  Planted: channel magnitudes
over 2^-20 .. 2^20, an all-zero row and pixel with signed zeros, windows whose level 1 cancels
to 2^-7 of its magnitude, a map whose rounding errors all have one sign, NaN in the f1 row that
out-of-range lanes clamp to, +Inf in the pixel without a parent, NaN in single gradient cells.

Not run: the exact fp32 kernel at C = 128 / 256, which needs RS_CORR_F32_SPLIT=0 in a fresh
process (deliberately: it has no channel-specific path beyond its K-step count, which
C = 32 / 96 / 160 cover); with that variable set this file skips.

Measured on an MI355X (largest err / bound over the cases of each check group; in brackets the
plain CPU emulation of tests/test_corr_volume_oracles_cpu.py where the GPU is above 0.9):
  volume, level            0              1              2       3
    exact fp32             0.116          0.055          0.028   0.011
    bf16 maps, fp32 out    0.085          0.986 [0.987]  0.280   0.128
    bf16 maps, bf16 out    0.993 [0.993]  0.813          0.546   0.181
    fp32 split             0.395          0.290          0.146   0.040
    finite part beside a planted NaN / Inf: 0.037 exact, 0.109 / 0.966 bf16 (fp32 / bf16 out), 0.035 split
  fold, bf16 out   wave4 0.995  wave8 0.996  wave12 0.994  rows 0.995 (vec0 = 0: 0.995)
                   fold4 element-wise 0.996  flat 0.992   [0.996]
  fold, in place   fold4 0.330  flat 0.320
  backward         bf16 df1 0.848 df2 0.848   fp32 split df1 0.405 df2 0.468
                   quad fold (bf16, N2 = 6288) df1 0.051 df2 0.479
  chain            lookups 0.098 bf16 / 0.032 fp32   df1 0.465 / 0.028   df2 0.430 / 0.043
No kernel missed its bound; 656 checks, 209 tests, under 4 s for the file (the slowest test 0.3 s).
The ratios near 1 are single bf16 roundings, which the emulation reproduces: the store of a
bf16 output (half an ulp is up to 2^-8 |want|), and at level 1 of the "coherent" map the one
rounding of the pooled f2, whose 2x2 means are ties of bf16 (2^-8 of the value, all of one sign
over the channels).  The fp32 routes use at most 0.4 of their bounds.
"""
import math
import os

import pytest
import torch

import corr_volume_cases as V
from corr_volume_cases import BF16, F32

pytestmark = pytest.mark.gpu

NAN = math.nan
B = 2
WORST = {}
COUNT = [0]


@pytest.fixture(autouse=True)
def _default_routes():
    if os.environ.get("RS_CORR_F32_SPLIT") is not None:
        pytest.skip("RS_CORR_F32_SPLIT is set: volume_route mirrors the default routing only")


def _check(name, got, want, bound, dtype, key):
    """max|err| and err / bound over every element (0 / 0 counts as 0)."""
    assert got.dtype == dtype, (name, got.dtype)
    got = got.detach().cpu()
    assert tuple(got.shape) == tuple(want.shape), (name, got.shape, want.shape)
    assert bool(torch.isfinite(got).all()), name + ": not finite"
    r = V.ratio(got, want, bound)
    err = (got.double() - want).abs().max().item() if want.numel() else 0.0
    WORST[key] = max(WORST.get(key, 0.0), r)
    COUNT[0] += 1
    print(f"{name}: max|err| {err:.3e}  err/bound {r:.3f}  (worst {key}: {WORST[key]:.3f}, check {COUNT[0]})")
    assert r <= 1.0, f"{name}: err/bound {r:.3f}"
    return r


def _bits(t):
    return t.view(torch.int32 if t.dtype == F32 else torch.int16)


# ------------------------------------------------------------------ forward
MODES = [("flat_bf16", False), ("flat_bf16", True), ("flat_split", False), ("exact", False)]
_ids = lambda m: f"{m[0]}{'-bf16out' if m[1] else ''}"  # noqa: E731


def _volume(cuda, f1, f2, L, C, route, out_bf16, tag):
    """Run the op, check the returned views, return (levels on the GPU, oracle)."""
    dt = V.ROUTE_DTYPE[route]
    assert f1.dtype == dt and V.volume_route(dt, C) == route and V.volume_accepts(dt, C), tag
    N1, (H, W) = f1.shape[1], f2.shape[1:3]
    pyr = torch.ops.raft_stir.corr_volume(f1.to(cuda), f2.to(cuda), L, C ** -0.5, out_bf16)
    assert len(pyr) == L
    for l, (h, w) in enumerate(V.level_sizes(H, W, L)):
        S = V.volume_pitch(h, w)
        assert pyr[l].shape == (B, N1, h, w) and pyr[l].stride() == (N1 * S, S, w, 1), (tag, l, pyr[l].stride())
        assert pyr[l].stride(2) == w and pyr[l].dtype == (BF16 if out_bf16 else F32)
    return pyr, V.pyramid(f1, f2, L, C ** -0.5)


def _volume_case(cuda, kind, N1, H, W, L, C, route, out_bf16):
    tag = f"volume {route} out_bf16={int(out_bf16)} {kind} N1={N1} {H}x{W} L{L} C={C}"
    f1, f2 = V.features(B, N1, H, W, C, V.ROUTE_DTYPE[route], kind)
    pyr, want = _volume(cuda, f1, f2, L, C, route, out_bf16, tag)
    for l, (w_, A) in enumerate(want):
        _check(f"{tag} level {l}", pyr[l], w_, V.vol_bound(route, l, C, A, w_, out_bf16),
               BF16 if out_bf16 else F32, f"{_ids((route, out_bf16))} L{l}")


@pytest.mark.parametrize("pair", range(len(V.fwd_pairs())))
@pytest.mark.parametrize("mode", MODES, ids=_ids)
def test_volume_shapes(cuda, mode, pair):
    N1, H, W, L, k = V.fwd_pairs()[pair]
    _volume_case(cuda, "randn", N1, H, W, L, V.CHANNELS[mode[0]][k], *mode)


@pytest.mark.parametrize("case", range(len(V.VALUE_CASES)))
@pytest.mark.parametrize("mode", MODES, ids=_ids)
def test_volume_values(cuda, mode, case):
    kind, N1, H, W, L = V.VALUE_CASES[case]
    for C in V.CHANNELS[mode[0]][case % 2::2]:
        _volume_case(cuda, kind, N1, H, W, L, C, *mode)


@pytest.mark.parametrize("mode", MODES, ids=_ids)
def test_volume_nonfinite_containment(cuda, mode):
    """NaN in f1 row N1-1 (the row out-of-range lanes clamp to): that volume row, every level,
    nothing else.  +Inf in f2 pixel (H2-1, W2-1) of an odd grid: level 0 only (it has no parent)."""
    route, out_bf16 = mode
    N1, H, W, L, C = 65, 9, 15, 4, V.CHANNELS[route][1]
    f1, f2 = V.features(B, N1, H, W, C, V.ROUTE_DTYPE[route])
    clean = V.pyramid(f1, f2, L, C ** -0.5)
    for what in ("nan_row", "inf_pixel"):
        g1, g2 = f1.clone(), f2.clone()
        if what == "nan_row":
            g1[1, N1 - 1, C // 2] = NAN
        else:
            g2[0, H - 1, W - 1, 3] = math.inf
        pyr, want = _volume(cuda, g1, g2, L, C, route, out_bf16, what)
        for l in range(L):
            got = pyr[l].cpu()
            bad = ~torch.isfinite(want[l][0])
            if what == "nan_row":
                exp = torch.zeros_like(bad)
                exp[1, N1 - 1] = True
            else:
                exp = torch.zeros_like(bad)
                if l == 0:
                    exp[0, :, H - 1, W - 1] = True
            assert torch.equal(bad, exp), (what, l)  # what the oracle says
            assert torch.equal(~torch.isfinite(got), bad), f"{what} level {l}: non-finite cells differ from the oracle's"
            w_, A = clean[l]
            ok = ~bad
            _check(f"{route} {what} level {l} (finite part)", torch.where(ok, got, torch.zeros_like(got)),
                   torch.where(ok, w_, torch.zeros_like(w_)), V.vol_bound(route, l, C, A, w_, out_bf16),
                   BF16 if out_bf16 else F32, f"{_ids(mode)} nonfinite")


def test_volume_host_checks(cuda):
    R = torch.ops.raft_stir

    def mk(N1=8, H=8, W=8, C=64, dt=BF16):
        return torch.randn(B, N1, C).to(dt).to(cuda), torch.randn(B, H, W, C).to(dt).to(cuda)
    f1, f2 = mk()
    with pytest.raises(RuntimeError, match="is empty"):
        R.corr_volume(*mk(H=4), 4, 0.125, False)
    with pytest.raises(RuntimeError, match="dtype mismatch"):
        R.corr_volume(f1, f2.float(), 2, 0.125, False)
    with pytest.raises(RuntimeError, match="multiple of 64"):
        R.corr_volume(*mk(C=48), 2, 0.125, False)
    with pytest.raises(RuntimeError, match="multiple of 64"):
        R.corr_volume(*mk(C=48, dt=F32), 2, 0.125, False)
    with pytest.raises(RuntimeError, match="bf16 pyramid needs bf16"):
        R.corr_volume(f1.float(), f2.float(), 2, 0.125, True)
    for L in (0, 5):
        with pytest.raises(RuntimeError, match=r"levels must be in \[1,4\]"):
            R.corr_volume(f1, f2, L, 0.125, False)
    wide = torch.randn(B, 8, 128).to(BF16).to(cuda)
    with pytest.raises(RuntimeError, match="contiguous"):
        R.corr_volume(wide[:, :, ::2], f2, 2, 0.125, False)


# ------------------------------------------------------------------ fold
def _stores(gp, store, dev):
    """Every level as a view of a NaN-filled store on ``dev``: [(view, store)]."""
    out = []
    for l, t in enumerate(gp):
        Bn, N1, h, w = t.shape
        S = V.fold_pitch(h * w, store if l == 0 or store in ("pitched", "compact") else "pitched")
        if store != "compact":
            S = max(S, 64)  # an empty level keeps a real pointer
        host = torch.full((max(Bn * N1 * S, 1),), NAN, dtype=F32)
        host.as_strided((Bn, N1, h, w), (N1 * S, S, w, 1)).copy_(t)
        st = host.to(dev)
        out.append((st.as_strided((Bn, N1, h, w), (N1 * S, S, w, 1)), st))
    return out


def _fold_case(cuda, case, mags):
    name, Bn, N1, H, W, L, store, k_inplace, k_bf16 = case
    E, coarse = H * W, V.coarse_cells(H, W, L)
    R = torch.ops.raft_stir
    for mag in mags:
        gp = V.grad_pyramid(Bn, N1, H, W, L, mag)
        want, Wf = V.fold(gp, 0.125)
        lv = _stores(gp, store, cuda)
        views = [v for v, _ in lv]
        before = [s.clone() for _, s in lv]
        S0, aligned = views[0].stride(1), views[0].data_ptr() % 16 == 0
        assert S0 == V.fold_pitch(E, store) or E == 0
        # bf16 form: gpyr untouched, bit for bit
        assert V.fold_route(E, S0, aligned, coarse, 0, True) == k_bf16, name
        out = torch.full((Bn, N1, H, W), NAN, dtype=BF16, device=cuda)
        R.pyr_grad_fold_bf16(views, 0.125, out)
        _check(f"fold {name} mag={mag:g} bf16 [{k_bf16}]", out, want, V.fold_bound(Wf, want, True), BF16, f"fold {k_bf16}")
        for (_, s), b0 in zip(lv, before):
            assert torch.equal(_bits(s), _bits(b0)), f"{name}: pyr_grad_fold_bf16 changed gpyr"
        # in place: level 0 cells only; the padding still NaN, the other levels unchanged
        assert V.fold_route(E, S0, aligned, coarse, 0, False) == k_inplace, name
        R.pyr_grad_fold(views, 0.125)
        _check(f"fold {name} mag={mag:g} in place [{k_inplace}]", views[0], want, V.fold_bound(Wf), F32, f"fold {k_inplace} in place")
        cells = torch.zeros(lv[0][1].shape, dtype=torch.bool, device=cuda)
        cells.as_strided(views[0].shape, views[0].stride()).fill_(True)
        assert torch.equal(_bits(lv[0][1])[~cells], _bits(before[0])[~cells]), f"{name}: padding of level 0 written"
        for (_, s), b0 in list(zip(lv, before))[1:]:
            assert torch.equal(_bits(s), _bits(b0)), f"{name}: a coarse level changed"
        # the all-zero row stays exactly zero
        if N1 > 2:
            assert not bool(views[0][:, N1 // 2].any()) and not bool(out[:, N1 // 2].float().any())


@pytest.mark.parametrize("case", V.FOLD_CASES, ids=[c[0] for c in V.FOLD_CASES])
def test_fold(cuda, case):
    _fold_case(cuda, case, V.GRAD_SCALES)


@pytest.mark.parametrize("case", V.FOLD_BIG, ids=[c[0] for c in V.FOLD_BIG])
def test_fold_more_rows_than_grid_y(cuda, case):
    """70001 rows > the 65535 of gridDim.y: pyr_fold4_kernel's row-stride loop."""
    assert case[1] * case[2] > V.FOLD4_GRID_Y
    _fold_case(cuda, case, (1.0,))


# ------------------------------------------------------------------ backward
def _bwd_inputs(cuda, N1, H, W, C, dt, store):
    L = V.max_levels(H, W)
    gp = V.grad_pyramid(B, N1, H, W, L)
    f1, f2 = V.features(B, N1, H, W, C, dt)
    lv = _stores(gp, store, cuda)
    return L, gp, f1, f2, lv


def _bwd_check(tag, got, gp, f1, f2, C, dt, key):
    N1, (H, W) = f1.shape[1], f2.shape[1:3]
    G0, _ = V.fold(gp, C ** -0.5)
    w1, w2, T1, T2 = V.backward(G0, f1, f2)
    _check(f"{tag} df1", got[0], w1, V.bwd_bound(dt == F32, H * W, T1, w1), dt, f"df1 {key}")
    _check(f"{tag} df2", got[1], w2, V.bwd_bound(dt == F32, N1, T2, w2), dt, f"df2 {key}")


@pytest.mark.parametrize("store", ["pitched", "compact"])
@pytest.mark.parametrize("dt", [BF16, F32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("C", [128, 256])
@pytest.mark.parametrize("shape", V.BWD_SHAPES, ids=[f"{n}-{h}x{w}" for n, h, w in V.BWD_SHAPES])
def test_backward(cuda, shape, C, dt, store):
    N1, H, W = shape
    L, gp, f1, f2, lv = _bwd_inputs(cuda, N1, H, W, C, dt, store)
    views = [v for v, _ in lv]
    route = V.bwd_route(B, N1, H, W, C, dt, V.coarse_cells(H, W, L), views[0].stride(1), views[0].data_ptr() % 16 == 0)
    assert route["ok"] and route["rowfold"] and route["Ep"] == V.round_up(H * W, 64)
    assert route["fold"].startswith("rows" if dt == F32 or views[0].stride(1) % 4 else "wave"), route
    before = [s.clone() for _, s in lv]
    d1, d2 = f1.to(cuda), f2.to(cuda)
    got = torch.ops.raft_stir.corr_volume_backward(views, d1, d2, C ** -0.5)
    tag = f"backward N1={N1} {H}x{W} L{L} C={C} {dt} {store} [{route['fold']}]"
    assert got[0].shape == f1.shape and got[1].shape == f2.shape
    _bwd_check(tag, got, gp, f1, f2, C, dt, "bf16" if dt == BF16 else "fp32 split")
    again = torch.ops.raft_stir.corr_volume_backward(views, d1, d2, C ** -0.5)
    assert torch.equal(_bits(got[0]), _bits(again[0])) and torch.equal(_bits(got[1]), _bits(again[1])), tag + ": two calls differ"
    for (_, s), b0 in zip(lv, before):
        assert torch.equal(_bits(s), _bits(b0)), tag + ": gpyr changed"
    if f1.numel() == f2.numel():  # the encoder hands the pair back as one batch's gradient
        assert got[1].data_ptr() == got[0].data_ptr() + f1.numel() * f1.element_size(), tag + ": df1 | df2 not adjacent"


@pytest.mark.parametrize("dt", [BF16, F32], ids=["bf16", "fp32"])
def test_backward_deterministic_modes_agree(cuda, dt):
    N1, H, W, C = 129, 11, 12, 128
    L, gp, f1, f2, lv = _bwd_inputs(cuda, N1, H, W, C, dt, "pitched")
    views, outs = [v for v, _ in lv], []
    try:
        for det in (True, False):
            torch.ops.raft_stir.set_deterministic(det)
            outs.append(torch.ops.raft_stir.corr_volume_backward(views, f1.to(cuda), f2.to(cuda), C ** -0.5))
    finally:
        torch.ops.raft_stir.set_deterministic(False)
    assert torch.equal(_bits(outs[0][0]), _bits(outs[1][0])) and torch.equal(_bits(outs[0][1]), _bits(outs[1][1]))


def test_backward_quad_fold(cuda):
    """N2 = 6288 > 6144: pyr_fold4_kernel<true> writes the padded G; fp32 features are refused."""
    N1, H, W = V.BWD_QUAD
    C = 128
    L, gp, f1, f2, lv = _bwd_inputs(cuda, N1, H, W, C, BF16, "pitched")
    views = [v for v, _ in lv]
    route = V.bwd_route(B, N1, H, W, C, BF16, V.coarse_cells(H, W, L), views[0].stride(1), views[0].data_ptr() % 16 == 0)
    assert L == 4 and route["ok"] and not route["rowfold"] and route["fold"] == "fold4(vec_out=1)", route
    got = torch.ops.raft_stir.corr_volume_backward(views, f1.to(cuda), f2.to(cuda), C ** -0.5)
    _bwd_check(f"backward quad fold N1={N1} {H}x{W}", got, gp, f1, f2, C, BF16, "bf16 quad fold")
    with pytest.raises(RuntimeError, match="grids over 6144 cells"):
        torch.ops.raft_stir.corr_volume_backward(views, f1.float().to(cuda), f2.float().to(cuda), C ** -0.5)


@pytest.mark.parametrize("dt", [BF16, F32], ids=["bf16", "fp32"])
def test_backward_nonfinite_containment(cuda, dt):
    N1, H, W, C, L = 65, 9, 15, 128, 4
    gp = V.grad_pyramid(B, N1, H, W, L)
    f1, f2 = V.features(B, N1, H, W, C, dt)
    d1, d2 = f1.to(cuda), f2.to(cuda)

    def run(gpyr, a=d1):
        lv = _stores(gpyr, "pitched", cuda)
        return [t.cpu() for t in torch.ops.raft_stir.corr_volume_backward([v for v, _ in lv], a, d2, C ** -0.5)]
    # one level-0 cell (b, i, y, x): df1[b, i, :] and df2[b, y, x, :]
    g = [t.clone() for t in gp]
    g[0][1, 7, 8, 14] = NAN
    e1, e2 = torch.zeros(B, N1, C, dtype=torch.bool), torch.zeros(B, H, W, C, dtype=torch.bool)
    e1[1, 7], e2[1, 8, 14] = True, True
    o1, o2 = run(g)
    assert torch.equal(~torch.isfinite(o1), e1) and torch.equal(~torch.isfinite(o2), e2), "level-0 NaN cell"
    # one level-2 cell: exactly its 16 children
    g = [t.clone() for t in gp]
    g[2][0, 64, 1, 2] = NAN
    e1, e2 = torch.zeros_like(e1), torch.zeros_like(e2)
    e1[0, 64], e2[0, 4:8, 8:12] = True, True
    o1, o2 = run(g)
    assert torch.equal(~torch.isfinite(o1), e1) and torch.equal(~torch.isfinite(o2), e2), "level-2 NaN cell"
    # NaN in f1 row N1-1 (the last K row of the Gt GEMM): df2 as the oracle's, df1 untouched
    a = f1.clone()
    a[1, N1 - 1, 5] = NAN
    G0, _ = V.fold(gp, C ** -0.5)
    w1, w2, _, _ = V.backward(G0, a, f2)
    o1, o2 = run(gp, a.to(cuda))
    assert bool(torch.isfinite(w1).all()) and torch.equal(~torch.isfinite(o1), ~torch.isfinite(w1))
    assert torch.equal(~torch.isfinite(o2), ~torch.isfinite(w2)) and not bool(torch.isfinite(o2[1, :, :, 5]).any())
    assert bool(torch.isfinite(o2[0]).all())


def test_backward_host_checks(cuda):
    R = torch.ops.raft_stir
    N1, H, W = 16, 4, 4
    gp = [torch.zeros(B, N1, H, W, device=cuda), torch.zeros(B, N1, 2, 2, device=cuda)]

    def mk(C=128, dt=BF16, h=H, w=W):
        return torch.randn(B, N1, C).to(dt).to(cuda), torch.randn(B, h, w, C).to(dt).to(cuda)
    with pytest.raises(RuntimeError, match="multiple of 128"):
        R.corr_volume_backward(gp, *mk(C=64), 0.1)
    with pytest.raises(RuntimeError, match="level 0 must be f2's grid"):
        R.corr_volume_backward(gp, *mk(h=2, w=8), 0.1)
    f1, f2 = mk()
    with pytest.raises(RuntimeError, match="dtypes differ"):
        R.corr_volume_backward(gp, f1, f2.float(), 0.1)
    wide = torch.randn(B, H, W, 256).to(BF16).to(cuda)
    with pytest.raises(RuntimeError, match="contiguous"):
        R.corr_volume_backward(gp, f1, wide[..., ::2], 0.1)
    buf = torch.randn(B * N1 * 128 + 1, device=cuda)
    off = buf[1:].view(B, N1, 128)
    assert off.is_contiguous() and off.data_ptr() % 16 == 4
    with pytest.raises(RuntimeError, match="16-B aligned"):
        R.corr_volume_backward(gp, off, f2.float(), 0.1)


# ------------------------------------------------------------------ the chain
@pytest.mark.parametrize("dt", [BF16, F32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("case", V.CHAIN_CASES, ids=[f"C{c[0]}-{c[1]}x{c[2]}-r{c[3]}" for c in V.CHAIN_CASES])
def test_chain(cuda, case, dt):
    """AllPairsCorr forward, two lookups, backward vs float64 autograd of the oracles.  Bounds
    composed per element: a lookup is a convex combination of cells, so its error is the
    lookup of the volume bounds + the lookup's own 1e-5 (1 + |want|); each lookup backward
    leaves 1e-5 (1 + |its cells|) in the gradient pyramid, which the (linear, non-negative)
    fold carries into G and sum |.| |f| into df1 / df2, on top of the backward's own bound."""
    from raft_stir_amd.ops.corr import AllPairsCorr
    C, H, W, r = case
    N, L, scale = H * W, 4, C ** -0.5
    route = V.volume_route(dt, C)
    f1, f2 = V.features(B, N, H, W, C, dt)
    coords = [V.chain_coords(H, W, k) for k in (0, 1)]
    CH = L * (2 * r + 1) ** 2
    wts = [torch.randn(B, H, W, CH, generator=V.gen(H, W, r, k)) for k in (0, 1)]
    # float64 oracle
    a, b = f1.double().requires_grad_(), f2.double().requires_grad_()
    pyr = V.pyramid(a, b, L, scale)
    looks = [V.lookup([v for v, _ in pyr], c, r) for c in coords]
    want1, want2 = torch.autograd.grad(sum((lk * w.double()).sum() for lk, w in zip(looks, wts)), (a, b))
    # the raw gradient pyramid of each lookup (what corr_lookup_backward accumulates)
    leaves = [v.detach().requires_grad_() for v, _ in pyr]
    gps = [torch.autograd.grad((V.lookup(leaves, c, r) * w.double()).sum(), leaves) for c, w in zip(coords, wts)]
    gp = [g0 + g1 for g0, g1 in zip(*gps)]
    G0, _ = V.fold(gp, 1.0)  # the pyramid oracle already carries scale: fold(., 1) is d loss / d vol0
    delta = [V.LOOKUP_TOL * (2 + g0.abs() + g1.abs()) for g0, g1 in zip(*gps)]
    dG, _ = V.fold(delta, 1.0)
    # the device
    m1 = f1.reshape(B, H, W, C).permute(0, 3, 1, 2).to(cuda).requires_grad_()
    m2 = f2.permute(0, 3, 1, 2).to(cuda).requires_grad_()
    corr = AllPairsCorr(m1, m2, num_levels=L, radius=r)
    assert corr.hip
    loss = 0
    for k, c in enumerate(coords):
        out = corr(c.to(cuda))
        assert out.shape == (B, CH, H, W)
        w_ = looks[k].detach()
        bnd = V.lookup([V.vol_bound(route, l, C, A.detach()) for l, (_, A) in enumerate(pyr)], c, r) + V.LOOKUP_TOL * (1 + w_.abs())
        _check(f"chain {case} {dt} lookup {k}", out.permute(0, 2, 3, 1), w_, bnd, F32, f"chain lookup {dt}")
        loss = loss + (out * wts[k].permute(0, 3, 1, 2).to(cuda)).sum()
    loss.backward()
    s = V.f32(scale)
    _, _, T1, T2 = V.backward(G0 * s, f1, f2)
    e1, e2, _, _ = V.backward(dG * s, f1.abs(), f2.abs())
    # G0 above is d loss / d vol0; the op folds the raw gradient pyramid and applies scale itself
    g1 = m1.grad.permute(0, 2, 3, 1).reshape(B, N, C)
    g2 = m2.grad.permute(0, 2, 3, 1)
    _check(f"chain {case} {dt} df1", g1, want1.detach(), V.bwd_bound(dt == F32, N, T1, want1) + e1, dt, f"chain df1 {dt}")
    _check(f"chain {case} {dt} df2", g2, want2.detach(), V.bwd_bound(dt == F32, N, T2, want2) + e2, dt, f"chain df2 {dt}")


def test_zz_report(cuda):
    """The largest err / bound of every check group (the figures of the docstring)."""
    for k in sorted(WORST):
        print(f"{k:40s} {WORST[k]:.3f}")
    print(f"{COUNT[0]} checks")

"""What the fp64 oracles of the edge-input GPU tests themselves say (CPU only).

tests/test_corr_edges_gpu.py and tests/test_gates_gpu.py hold the HIP kernels
to ``ops/reference.py`` evaluated in fp64.  The expectations they state about
extreme inputs are pinned here to the reference, not to the kernels:

* a coordinate far outside the map (+-1e6, +-3e9, 1e20) is zero padding: the
  pixel's whole window is exactly 0 and no other pixel changes;
* a non-finite coordinate (+-inf, NaN) turns exactly that pixel into NaN;
* the per-kernel gate formulas (``ref.gru_*``) chained as ops/gru.py chains
  them reproduce fp64 autograd through ``_gru_step_reference``.

The second half does the same for tests/test_flow_path_gpu.py, whose oracles
live in tests/flow_path_cases.py: they equal ``ref.convex_upsample``, fp64
autograd and the composite loss of train/loss.py; the flow encoder's bound
rejects a kernel without the bf16 hi + lo split; the planted loss magnitudes
are exact in fp32 and no unplanted pixel sits on a 1 / 3 / 5 px threshold.
"""
import math

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from raft_stir_amd.ops import reference as ref

HUGE = [1e6, -1e6, 3e9, -3e9, 1e20]
NONFINITE = [math.inf, -math.inf, math.nan]


def _pyramid(B, H, W, levels, seed=0):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(B * H * W, 1, H >> l, W >> l, generator=g, dtype=torch.float64) for l in range(levels)]


def _coords(B, H, W, seed=1):
    g = torch.Generator().manual_seed(seed)
    return ref.coords_grid(B, H, W, dtype=torch.float64) + 6.0 * torch.randn(B, 2, H, W, generator=g, dtype=torch.float64)


def _plant(coords, values):
    """One pixel per value: alternately in x and in y; returns the (b, y, x) list."""
    c = coords.clone()
    where = []
    for i, v in enumerate(values):
        b, y, x = i % c.shape[0], 2 + i, 3 + 2 * i
        c[b, i % 2, y, x] = v
        where.append((b, y, x))
    return c, where


def _others_equal(got, base, where):
    keep = torch.ones(got.shape[0], got.shape[2], got.shape[3], dtype=torch.bool)
    for b, y, x in where:
        keep[b, y, x] = False
    k = keep[:, None].expand_as(got)
    return torch.equal(got[k], base[k])


@pytest.mark.parametrize("radius", [2, 4])
def test_reference_lookup_far_coordinates_are_zero_padding(radius):
    B, H, W = 2, 17, 23
    pyr, coords = _pyramid(B, H, W, 4), _coords(B, H, W)
    base = ref.corr_lookup(pyr, coords, radius)
    far, where = _plant(coords, HUGE)
    got = ref.corr_lookup(pyr, far, radius)
    for b, y, x in where:
        assert bool((got[b, :, y, x] == 0).all())
    assert torch.isfinite(got).all() and _others_equal(got, base, where)


@pytest.mark.parametrize("radius", [2, 4])
def test_reference_lookup_nonfinite_coordinates_poison_one_pixel(radius):
    B, H, W = 2, 17, 23
    pyr, coords = _pyramid(B, H, W, 4), _coords(B, H, W)
    base = ref.corr_lookup(pyr, coords, radius)
    bad, where = _plant(coords, NONFINITE)
    got = ref.corr_lookup(pyr, bad, radius)
    for b, y, x in where:
        assert bool(torch.isnan(got[b, :, y, x]).all())
    assert int(torch.isnan(got).any(1).sum()) == len(where) and _others_equal(got, base, where)


def test_reference_onthefly_far_and_nonfinite_coordinates():
    B, C, H, W, r = 2, 8, 16, 24, 2
    g = torch.Generator().manual_seed(3)
    f1 = torch.randn(B, C, H, W, generator=g, dtype=torch.float64)
    f2 = torch.randn(B, C, H, W, generator=g, dtype=torch.float64)
    coords = _coords(B, H, W)
    # ref.corr_onthefly casts its feature maps to fp32: the same per-level form in fp64
    # (what the GPU tests use as their oracle), tied to the fp32 entry point below
    def otf(c):
        outs = []
        lv = f2
        delta = ref._window_delta(r, c.device, c.dtype).reshape(-1, 2)
        pos = c.permute(0, 2, 3, 1)
        for lvl in range(4):
            if lvl:
                lv = F.avg_pool2d(lv, 2, stride=2)
            outs += [(ref.bilinear_sampler(lv, pos / 2 ** lvl + delta[k]) * f1).sum(1) for k in range(delta.shape[0])]
        return torch.stack(outs, 1) / math.sqrt(C)
    base = otf(coords)
    # the fp32 entry point agrees with the per-level form the GPU tests differentiate through
    torch.testing.assert_close(ref.corr_onthefly(f1, f2, coords.float(), r).double(), otf(coords.float().double()),
                               atol=1e-4, rtol=1e-4)
    far, where = _plant(coords, HUGE)
    got = otf(far)
    for b, y, x in where:
        assert bool((got[b, :, y, x] == 0).all())
    assert torch.isfinite(got).all() and _others_equal(got, base, where)
    got32 = ref.corr_onthefly(f1, f2, far.float(), r)
    for b, y, x in where:
        assert bool((got32[b, :, y, x] == 0).all())
    bad, where = _plant(coords, NONFINITE)
    got = otf(bad)
    for b, y, x in where:
        assert bool(torch.isnan(got[b, :, y, x]).all())
    assert int(torch.isnan(got).any(1).sum()) == len(where) and _others_equal(got, base, where)


def _nhwc(t):
    return t.permute(0, 2, 3, 1)


def _nchw(t):
    return t.permute(0, 3, 1, 2)


@pytest.mark.parametrize("hd,cin,k", [(8, 12, 1), (6, 10, 3)])
def test_gate_formulas_equal_autograd_through_the_reference_step(hd, cin, k):
    from raft_stir_amd.models.update import _gru_step_reference
    torch.manual_seed(0)
    B, H, W = 2, 5, 7
    convz, convr, convq = (nn.Conv2d(hd + cin, hd, k, padding=k // 2).double() for _ in range(3))
    h = torch.tanh(torch.randn(B, hd, H, W, dtype=torch.float64)).requires_grad_()
    x = (2 * torch.randn(B, cin, H, W, dtype=torch.float64)).requires_grad_()
    want = _gru_step_reference(convz, convr, convq, h, x)
    gout = torch.randn_like(want)
    want_dh, want_dx = torch.autograd.grad(want, (h, x), gout)

    # the chain of ops/gru.py with the gate stages from ops/reference.py (convolutions through autograd)
    hx = torch.cat([h, x], 1).detach().requires_grad_()
    zr = torch.cat([convz(hx), convr(hx)], 1)
    z, r, rhx = ref.gru_gate_zr(_nhwc(zr).detach(), _nhwc(h).detach(), _nhwc(x).detach())
    rhx_in = _nchw(rhx).detach().requires_grad_()
    q = convq(rhx_in)
    hn, qt = ref.gru_gate_q(_nhwc(q).detach(), z, _nhwc(h).detach())
    torch.testing.assert_close(_nchw(hn), want.detach(), atol=1e-13, rtol=1e-13)

    dq, dz, dhd = ref.gru_bwd_q(_nhwc(gout), z, _nhwc(h).detach(), qt)
    drhx = _nhwc(torch.autograd.grad(q, rhx_in, _nchw(dq))[0])
    dr = ref.gru_bwd_r(drhx, _nhwc(h).detach(), r)
    dhx = _nhwc(torch.autograd.grad(zr, hx, _nchw(torch.cat([dz, dr], -1)))[0])
    dh, dx = ref.gru_bwd_fin(dhd, drhx, r, dhx)
    torch.testing.assert_close(_nchw(dh), want_dh, atol=1e-12, rtol=1e-12)
    torch.testing.assert_close(_nchw(dx), want_dx, atol=1e-12, rtol=1e-12)


def test_context_act_formulas_equal_autograd():
    torch.manual_seed(1)
    hd, cd = 6, 10
    cn = (3 * torch.randn(2, 5, 7, hd + cd, dtype=torch.float64)).requires_grad_()
    net, inp = ref.context_act(cn, hd)
    G = torch.randn(2, 5, 7, hd + cd + 3, dtype=torch.float64)
    want, = torch.autograd.grad(torch.cat([net, inp], -1), cn, G[..., :hd + cd])
    got = ref.context_act_backward(G, net.detach(), inp.detach(), hd)
    torch.testing.assert_close(got, want, atol=1e-14, rtol=1e-14)


# ------------------------------------------------------------------ the flow path
# What the oracles of tests/test_flow_path_gpu.py (tests/flow_path_cases.py) say, and
# that its bounds discriminate.
import flow_path_cases as fc  # noqa: E402


@pytest.mark.parametrize("N,H,W", [(1, 1, 1), (2, 3, 5)])
def test_convex_upsample_oracle_equals_reference_and_autograd(N, H, W):
    g = torch.Generator().manual_seed(0)
    flow = (30 * torch.randn(N, 2, H, W, generator=g, dtype=torch.float64)).requires_grad_()
    mask = (3 * torch.randn(N, H, W, 576, generator=g, dtype=torch.float64)).requires_grad_()
    want = ref.convex_upsample(flow, mask.permute(0, 3, 1, 2).contiguous().view(N, 576, H, W))
    got, bound = fc.cu_fwd_oracle(flow.detach(), mask.detach())
    torch.testing.assert_close(got, want.detach(), atol=1e-12, rtol=1e-13)
    assert bool((bound > 0).all())
    gup = torch.randn(N, 2, 8 * H, 8 * W, generator=g, dtype=torch.float64)
    wdf, wdm = torch.autograd.grad(want, (flow, mask), gup)
    df, bdf, dm, bdm = fc.cu_bwd_oracle(flow.detach(), mask.detach(), gup)
    torch.testing.assert_close(df, wdf, atol=1e-11, rtol=1e-12)
    torch.testing.assert_close(dm, wdm, atol=1e-11, rtol=1e-12)
    assert bool((bdf >= 0).all()) and bool((bdm > 0).all())


def test_convex_upsample_planted_logits_stay_finite_in_the_oracle():
    for dt in (torch.float32, torch.bfloat16):
        flow, mask = fc.cu_inputs(2, 2, 40, dt, seed=1)
        assert bool(torch.isinf(mask).any()) and float(mask[torch.isfinite(mask)].max()) >= 9984.0
        want, bound = fc.cu_fwd_oracle(flow, mask)
        gup = torch.randn(2, 2, 16, 320, generator=torch.Generator().manual_seed(2))
        parts = fc.cu_bwd_oracle(flow, mask, gup)
        assert all(bool(torch.isfinite(t).all()) for t in (want, bound, *parts))
        # a tap at -inf takes no weight and no gradient
        dm = parts[2]
        assert bool((dm[torch.isinf(mask)] == 0).all())


def test_flow_head_and_flow_wgrad_oracles_equal_autograd():
    g = torch.Generator().manual_seed(1)
    B, H, W, C = 2, 3, 5, 8
    x = torch.randn(B, H, W, C, generator=g, dtype=torch.float64)
    w = torch.randn(2, 3, 3, C, generator=g, dtype=torch.float64)
    bias, src = torch.randn(2, generator=g, dtype=torch.float64), torch.randn(B, 2, H, W, generator=g, dtype=torch.float64)
    xr = x.permute(0, 3, 1, 2).clone().requires_grad_()
    y = src + F.conv2d(xr, w.permute(0, 3, 1, 2), bias, padding=1)
    torch.testing.assert_close(fc.fh_fwd_oracle(x, w, bias, src)[0], y.detach(), atol=1e-13, rtol=1e-13)
    dflow = torch.randn(B, 2, H, W, generator=g, dtype=torch.float64)
    dx, = torch.autograd.grad(y, xr, dflow)
    want = dx.permute(0, 2, 3, 1) * (x > 0)
    torch.testing.assert_close(fc.fh_dgrad_oracle(dflow, w, x)[0], want, atol=1e-13, rtol=1e-13)
    # flow_wgrad: dW of conv7x7 in the [49][2][C] layout, accumulated into dw0 / db0
    flow = 100 * torch.randn(B, 2, H, W, generator=g, dtype=torch.float64)
    df = torch.randn(B, H, W, C + 3, generator=g, dtype=torch.float64)
    w7 = torch.zeros(49, 2, C, dtype=torch.float64, requires_grad=True)
    b7 = torch.zeros(C, dtype=torch.float64, requires_grad=True)
    out = F.conv2d(flow, fc.fe_conv_weight(w7), b7, padding=3)
    gw, gb = torch.autograd.grad(out, (w7, b7), df[..., :C].permute(0, 3, 1, 2))
    dw0, db0 = torch.randn(49, 2, C, generator=g, dtype=torch.float64), torch.randn(C, generator=g, dtype=torch.float64)
    dw, Sw, db, Sb = fc.fw_oracle(flow, df, dw0, db0)
    torch.testing.assert_close(dw, dw0 + gw, atol=1e-10, rtol=1e-12)
    torch.testing.assert_close(db, db0 + gb, atol=1e-10, rtol=1e-12)
    assert bool((Sw >= (dw - dw0).abs() - 1e-9).all()) and bool((Sb >= (db - db0).abs() - 1e-9).all())


@pytest.mark.parametrize("scale", [4.0, 100.0, 400.0])
def test_flow_encoder_bound_discriminates(scale):
    """The kernel's three split-bf16 products, in exact arithmetic, stay under the
    test's bound; the hi * hi product alone (plain bf16 operands) exceeds it > 50x
    at flow scale 100: dropping the split cannot pass."""
    coords, flow, w, bias = fc.fe_inputs(2, 13, 21, 128, seed=5, scale=scale)
    flow[:, :, 6, 10] = 4 * scale  # a spike at 4x the scale
    pre, A = fc.fe_oracle(flow, w, bias)
    exact = pre - bias.double()
    three = (fc.fe_emulate(flow, w, {"hh", "hl", "lh"}) - exact).abs()
    hi = (fc.fe_emulate(flow, w, {"hh"}) - exact).abs()
    drop = 3 * 2.0 ** -18 * A  # what the derivation allots to the dropped / rounded terms
    assert bool((three <= drop).all()), (three / drop).max()
    r3, rh = (three / (2.0 ** -16 * A)).max().item(), (hi / (2.0 ** -16 * A)).max().item()
    print(f"scale {scale}: three products {r3:.3f} of the bound, hi only {rh:.1f}x")
    assert r3 <= 0.75
    if scale == 100.0:
        assert rh >= 50.0, rh


def test_upflow8_helpers_mirror_the_kernel_file():
    assert fc.up8_band(1) == 8 and fc.up8_band(62) == 25 and fc.up8_cols_lds(62) == (25 * 62 + 4 * 8 * 62) * 4
    W = fc.up8_largest_w()
    assert fc.up8_cols_lds(W) <= 65536 < fc.up8_cols_lds(W + 1) and W >= 256
    from raft_stir_amd.models.fused_train import _interp_matrix
    for n in (1, 2, 62, 129):
        assert torch.equal(fc.interp_matrix(n, 8 * n), _interp_matrix(n, 8 * n, "cpu"))
    # the oracle is the adjoint of 8 * bilinear upsampling (align_corners)
    f = torch.zeros(1, 2, 3, 5, dtype=torch.float64, requires_grad=True)
    g = torch.randn(1, 2, 24, 40, generator=torch.Generator().manual_seed(0), dtype=torch.float64)
    (8 * F.interpolate(f, size=(24, 40), mode="bilinear", align_corners=True)).backward(g)
    want, _ = fc.up8_oracle(g, fc.interp_matrix(3, 24), fc.interp_matrix(5, 40))
    torch.testing.assert_close(want, f.grad, atol=1e-5, rtol=1e-5)  # fp32 matrices


LOSS_CASES = [(1, 1, 1, 1, 3), (12, 2, 3, 5, 20), (3, 1, 16, 17, 36), (2, 1, 725, 724, 725), (2, 1, 724, 724, 724)]


@pytest.mark.parametrize("N,B,H,W,seed", LOSS_CASES)
def test_loss_oracle_equals_the_composite_and_precondition_holds(N, B, H, W, seed):
    from raft_stir_amd.train.loss import sequence_loss
    preds, gt, valid, n = fc.loss_inputs(N, B, H, W, seed=seed)
    assert n == (12 if H * W >= 12 else 0)
    for gamma in (0.8, 1.0, 0.0):
        wl, wm, ok, epe = fc.loss_oracle(preds, gt, valid, gamma)
        assert fc.loss_precondition(epe, ok, n)
        loss, m = sequence_loss(list(preds.double().unbind(0)), gt.double(), valid.double(), gamma)
        assert abs(float(loss) - float(wl)) <= 1e-12 * max(1.0, abs(float(wl)))
        cnt = max(wm["cnt"], 1)
        assert abs(m["epe"] - wm["epe"]) <= 1e-12 * max(1.0, wm["epe"])
        assert [m["1px"], m["3px"], m["5px"]] == [wm["1px"] / cnt, wm["3px"] / cnt, wm["5px"] / cnt]
    if H * W >= 12:  # every plant is in: what fp64 says about them
        okp, e = ok.view(B, -1)[0, :n], epe.view(B, -1)[0, :n]
        assert okp.tolist() == [False, True, True, False, False] + [True] * 7
        assert [bool(e[5 + i] < k) for i, k in enumerate((1, 1, 3, 3, 5, 5, 1))] == [False, True, False, True, False, True, True]
    # pred - gt is exact in fp32 wherever the pixel counts
    d32, d64 = (preds - gt).double(), preds.double() - gt.double()
    assert torch.equal(d32[:, ok[:, None].expand_as(gt)], d64[:, ok[:, None].expand_as(gt)])


def test_loss_planted_magnitudes_are_exact_in_fp32():
    f = lambda *v: torch.tensor(v, dtype=torch.float32)
    mag = lambda u, v: torch.sqrt(f(u) * f(u) + f(v) * f(v))
    fused = lambda u, v: torch.sqrt((f(u).double() * f(u).double() + f(v).double() * f(v).double()).float())  # fma
    for m in (mag, fused):
        assert float(m(240.0, 320.0)) == 400.0 and float(m(240.0, fc.BELOW(320.0))) < 400.0
        for (du, dv), k, inside in zip(fc.EPE_PLANT, (1, 1, 3, 3, 5, 5, 1), (False, True, False, True, False, True, True)):
            assert (float(m(du, dv)) < k) == inside, (du, dv)
            assert (math.hypot(du, dv) < k) == inside
        # one fp32 step inside (3, 4) is invisible to any fp32 evaluation: hence four steps
        assert float(m(3.0, fc.BELOW(4.0))) == 5.0 and float(m(fc.BELOW(3.0), 4.0)) == 5.0
    assert fc.BELOW(0.5) < 0.5 and not (math.nan >= 0.5)

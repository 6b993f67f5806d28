"""What the fp64 oracles of the edge-input GPU tests themselves say (CPU only).

tests/test_corr_edges_gpu.py and tests/test_gates_gpu.py hold the HIP kernels
to ``ops/reference.py`` evaluated in fp64.  The expectations they state about
extreme inputs are pinned here to the reference, not to the kernels:

* a coordinate far outside the map (+-1e6, +-3e9, 1e20) is zero padding: the
  pixel's whole window is exactly 0 and no other pixel changes;
* a non-finite coordinate (+-inf, NaN) turns exactly that pixel into NaN;
* the per-kernel gate formulas (``ref.gru_*``) chained as ops/gru.py chains
  them reproduce fp64 autograd through ``_gru_step_reference``.
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

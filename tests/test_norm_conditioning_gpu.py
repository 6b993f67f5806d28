"""csrc/norm.hip statistics at large mean / std ratios vs fp64 on the CPU.

``norm_act`` (instance norm, and batch norm in training mode) on x = randn + k,
k in {0.25, 4, 16, 64}: mean / std up to 64, where sum(x^2)/n - mean^2 from
fp32 partial sums loses its digits to cancellation.  The statistics pass also
sums x - pivot and its square, and a channel with mean^2 > 12 (var + eps)
takes its statistics from those: k = 4, 16 and 64 do, k = 0.25 keeps the
one-pass sums.  Channel 5
is exactly constant (= k, so every sum is exact: variance exactly 0, y exactly
0 with gamma = 1, beta = 0) and channel 9 is 1 + 1e-3 randn (mean / std =
1000, variance 1e-6 below eps).  C = 64, B x H x W = 3 x 13 x 21 and
1 x 46 x 62, fp32 and bf16 (inputs rounded to bf16 first).

Oracle: F.instance_norm / F.batch_norm in fp64 on the CPU, dx through
autograd.  Criterion (fp32): the kernel's largest error is at most 8 x the
largest error of PyTorch's own fp32 CPU op against the same oracle, or
1e-6 max|want| where that is larger -- taken separately over the ordinary channels, the
constant channel and the low-variance channel, so that the (inherently
larger) rounding of the low-variance channel cannot hide a cancellation in
the others.  The factor covers the x * sc + sh form of the apply pass and a
different summation order, not cancellation.  bf16: + 2^-8 |want| per element.

Measured on an MI355X, fp32, largest |err| of y over the ordinary channels
(both shapes, instance and batch), kernel / PyTorch fp32 on the CPU:
  k = 0.25   4.9e-7 / 5.3e-7      k = 16   2.1e-6 / 2.4e-6
  k = 4      1.2e-6 / 8.8e-7      k = 64   9.0e-6 / 8.6e-6
and at most 0.28 of the bound in every group, y and dx (the low-variance
channel's 1.6e-5 to 2.2e-5 equals PyTorch's: both round the same mean to
fp32).  With the one-pass sums alone the kernel gave 7.8e-6 at k = 4 (over
8 x PyTorch's 8.8e-7), 1.3e-4 at k = 16 and 1.7e-3 at k = 64, 5e-3 to 8e-3 on
the low-variance channel at every k, and a dx of the constant channel wrong
by up to 5.6e2 (its zero variance came out as rounding noise above eps).
"""
import functools

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from raft_stir_amd.ops.norm import norm_act

pytestmark = pytest.mark.gpu

C, CONST, LOWVAR = 64, 5, 9
EPS = 1e-5
GROUPS = {"ordinary": [c for c in range(C) if c not in (CONST, LOWVAR)], "constant": [CONST], "low-variance": [LOWVAR]}


@functools.lru_cache(None)
def _case(shape, k, kind, dtype):
    """Inputs (rounded to `dtype`, as fp32), the fp64 oracle and PyTorch's fp32 CPU results."""
    B, H, W = shape
    g = torch.Generator().manual_seed(int(k * 4) + H)
    x = torch.randn(B, C, H, W, generator=g) + k
    x[:, CONST] = k
    x[:, LOWVAR] = 1.0 + 1e-3 * torch.randn(B, H, W, generator=g)
    dy = torch.randn(B, C, H, W, generator=g)
    x, dy = x.to(dtype).float(), dy.to(dtype).float()
    w = torch.rand(C, generator=g) + 0.5
    b = torch.rand(C, generator=g) * 0.6 - 0.3
    w[CONST], b[CONST] = 1.0, 0.0

    def run(t):
        xi = x.to(t, copy=True).requires_grad_()
        if kind == "instance":
            y = F.instance_norm(xi, eps=EPS)
        else:
            y = F.batch_norm(xi, None, None, w.to(t), b.to(t), training=True, eps=EPS)
        dx, = torch.autograd.grad(y, xi, dy.to(t))
        return y.detach(), dx
    return x, dy, w, b, run(torch.float64), run(torch.float32)


def _judge(name, got, want, torch32, dtype):
    ok = True
    for gname, ch in GROUPS.items():
        gk, wk, tk = got[:, ch].double(), want[:, ch], torch32[:, ch].double()
        ek, et = (gk - wk).abs(), (tk - wk).abs().max().item()
        bound = max(8.0 * et, 1e-6 * wk.abs().max().item())
        slack = 2.0 ** -8 * wk.abs() if dtype == torch.bfloat16 else torch.zeros_like(wk)
        worst = (ek - slack).max().item()
        print(f"{name} {gname}: kernel {ek.max().item():.3e}  torch fp32 {et:.3e}  bound {bound:.3e}"
              f"  max|want| {wk.abs().max().item():.3e}")
        ok = ok and bool(torch.isfinite(gk).all()) and worst <= bound
    return ok


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("kind", ["instance", "batch"])
@pytest.mark.parametrize("shape", [(3, 13, 21), (1, 46, 62)])
@pytest.mark.parametrize("k", [0.25, 4.0, 16.0, 64.0])
def test_norm_act_large_mean(cuda, k, shape, kind, dtype):
    x, dy, w, b, (y64, dx64), (y32, dx32) = _case(shape, k, kind, dtype)
    if kind == "instance":
        norm = nn.InstanceNorm2d(C, eps=EPS)
    else:
        norm = nn.BatchNorm2d(C, eps=EPS)
        with torch.no_grad():
            norm.weight.copy_(w)
            norm.bias.copy_(b)
        norm.train()
    norm = norm.to(cuda)
    xg = x.to(cuda, dtype).contiguous(memory_format=torch.channels_last).requires_grad_()
    y = norm_act(norm, xg, relu=False)
    assert y.dtype == dtype
    y.backward(dy.to(cuda, dtype).contiguous(memory_format=torch.channels_last))
    tag = f"k={k} {shape} {kind} {dtype}"
    ok_y = _judge(f"y  {tag}", y.detach().cpu(), y64, y32, dtype)
    ok_dx = _judge(f"dx {tag}", xg.grad.cpu(), dx64, dx32, dtype)
    assert ok_y and ok_dx, tag

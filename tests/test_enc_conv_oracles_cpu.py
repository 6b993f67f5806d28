"""The oracles, launch mirrors and bounds of tests/test_enc_conv_edges_gpu.py, on the CPU.

1. The float64 oracles of tests/enc_conv_cases.py equal float64 autograd of
   nn.Conv2d at every geometry of the GPU file, and the phase decomposition of the
   strided input gradient (ops/enc_conv.py _phase_taps) reproduces conv2d_input,
   writing every input pixel exactly once.
2. The launch mirrors reproduce the numbers written in the kernel files.
3. A plain fp32 evaluation of the same rounded operands, rounded to the storage
   dtype, stays under each bound at the case shapes (ratio printed).
4. Seven mutants exceed the bound on the elements they touch (largest and median
   ratio printed), at every case shape where they touch any:
   (a) a tap dropped at the last output column, (b) a stale halo in the second tile
   of a block, (c) a stride-2 phase with its taps in descending order, (d) the
   one-past-the-grid tap of the last odd row unmasked, (e) the last pixel of the
   last image dropped from a weight gradient, (f) bf16-rounded weights in sconv,
   (g) a hi-only product in the fp32 stem.
   Under bf16 storage the weights' rounding is smaller than a typical output's own
   half ulp and shows only where an output lies close to zero, so every sconv case
   has one output planted to cancel (enc_conv_cases.sconv_case): (f) is asserted
   at every shape, the one-pixel ones included, in bf16 as in fp32.
"""
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import enc_conv_cases as C
from enc_conv_cases import BF16, F32, F64

GEOMS = [(3, 1, 1), (3, 2, 1), (1, 2, 0), (1, 1, 0), (7, 2, 3)]


# ------------------------------------------------------------------ 1. oracles
@pytest.mark.parametrize("k,s,p", GEOMS)
@pytest.mark.parametrize("H,W", C.GEO_HW + [(9, 33)])
def test_oracles_equal_float64_autograd(k, s, p, H, W):
    g = C.gen(k, s, H, W)
    cin, cout = (3, 8) if k == 7 else (8, 16)
    conv = nn.Conv2d(cin, cout, k, stride=s, padding=p).double()
    x = torch.randn(2, H, W, cin, generator=g, dtype=F64)
    xin = x.permute(0, 3, 1, 2).clone().requires_grad_(True)
    y = conv(xin)
    dy = torch.randn(y.shape, generator=g, dtype=F64)
    y.backward(dy)
    w, b = conv.weight.detach(), conv.bias.detach()
    dyn = dy.permute(0, 2, 3, 1)
    want, A = C.conv_fwd(x, w, b, s, p)
    torch.testing.assert_close(want, y.detach().permute(0, 2, 3, 1), atol=1e-12, rtol=1e-12)
    assert bool((A >= want.abs() - 1e-12).all())
    dx, T = C.conv_dgrad(dyn, w, (H, W), s, p)
    torch.testing.assert_close(dx, xin.grad.permute(0, 2, 3, 1), atol=1e-12, rtol=1e-12)
    assert bool((T >= dx.abs() - 1e-12).all())
    dw, S, db, Sb = C.conv_wgrad(x, dyn, k, s, p)
    torch.testing.assert_close(dw, conv.weight.grad, atol=1e-11, rtol=1e-12)
    torch.testing.assert_close(db, conv.bias.grad, atol=1e-11, rtol=1e-12)
    assert bool((S >= dw.abs() - 1e-11).all()) and bool((Sb >= db.abs() - 1e-11).all())


@pytest.mark.parametrize("k,s,p", C.GEO_KSP)
@pytest.mark.parametrize("H,W", C.GEO_HW)
def test_phase_decomposition_reproduces_conv2d_input(k, s, p, H, W):
    from raft_stir_amd.ops import enc_conv
    for r in range(s):
        assert C.phase_taps(k, s, p, r) == enc_conv._phase_taps(k, s, p, r)
    g = C.gen(k, s, H, W, 3)
    ho, wo = C.out_hw(H, W, k, s, p)
    dy = torch.randn(2, ho, wo, 16, generator=g, dtype=F64)
    w = torch.randn(16, 8, k, k, generator=g, dtype=F64)
    dx, _ = C.conv_dgrad(dy, w, (H, W), s, p)
    px, wrote = C.phase_dgrad(dy, w, (H, W), s, p)
    torch.testing.assert_close(px, dx, atol=1e-12, rtol=1e-12)
    if k == 1 and s == 2:  # only phase (0, 0) has a tap: the other three stay zero
        assert bool((wrote[:, ::2, ::2] == 1).all()) and int(wrote.sum()) == wrote[:, ::2, ::2].numel()
        z = dx.clone()
        z[:, ::2, ::2] = 0
        assert not bool(z.any())
    else:
        assert bool((wrote == 1).all())


def test_epilogue_oracle_is_the_composite():
    g = C.gen(77)
    acc = torch.randn(2, 3, 4, 8, generator=g, dtype=F64)
    sc, sh = torch.randn(8, generator=g), torch.randn(8, generator=g)
    res = torch.randn(2, 3, 4, 8, generator=g)
    want, bound = C.epilogue(acc, 0.0 * acc, sc, sh, True, res)
    torch.testing.assert_close(want, torch.relu(torch.relu(acc * sc.double() + sh.double()) + res.double()))
    assert bool((bound > 0).all())
    want, _ = C.epilogue(acc, 0.0 * acc, res=res, res_relu=False)
    torch.testing.assert_close(want, acc + res.double())


# ------------------------------------------------------------------ 2. launch mirrors
def test_launch_mirrors_reproduce_the_kernel_files():
    assert C.halo_tiles(3, 9, 65, 64, 64) == (18, 4) and C.halo_tiles(*C.HALO_LONG) == (343, 12)
    assert C.halo_tiles(1, 8 * 27, 32 * 19, 64, 128) == (513, 12) and C.halo_tiles(1, 8 * 27, 32 * 19, 64, 64) == (513, 4)
    assert C.halo_chain(64) == 2 * 36 and C.halo_chain(96) == 2 * 54  # NS = 9 * (CIN / 16)
    assert C.stem_wgrad_blocks(1, 1, 1) == (1, 1) and C.stem_wgrad_blocks(2, 129, 65) == (258, 2)
    assert C.stem_wgrad_blocks(16, 184, 248) == (512, 23)  # 11776 chunks over <= 512 blocks
    assert C.enc_wgrad_splits(1, 1, 1, 64, 64) == (1, 1) and C.enc_wgrad_splits(3, 9, 65, 96, 96) == (18, 1)
    assert C.enc_wgrad_splits(16, 184, 248, 64, 64) == (246, 12)  # 2944 tiles over ~256 blocks
    assert C.wgrad_plan(768, 1, 64, 64, False) == (2, 384) and C.wgrad_plan(9, 9, 128, 96, True) == (1, 64)
    assert C.wgrad_plan(100000, 9, 64, 64, False) == (112, 896) and C.wgrad_plan(100000, 9, 64, 64, True) == (32, 3136)
    assert C.sconv_wgrad_blocks(3, 70, 96 * 9 * 24) == (105, 2) and C.sconv_wgrad_blocks(1, 1, 64) == (1, 1)
    assert C.sconv_wgrad_lanes(16, 12, 3) == (54, 4, 4) and C.sconv_wgrad_lanes(24, 96, 3) == (324, 1, 8)
    assert C.sconv_chain(3, 96) == 435 and not C.sconv_fits(96, 32, 3) and C.sconv_fits(24, 96, 3)


# ------------------------------------------------------------------ 3. plain fp32 under the bounds
def _f32_conv(x, w, b, s, p):
    y = F.conv2d(x.float().permute(0, 3, 1, 2), w.float(), None if b is None else b.float(), s, p)
    return y.permute(0, 2, 3, 1)


def _f32_wgrad(x, dy, k, s, p):
    return torch.nn.grad.conv2d_weight(x.float().permute(0, 3, 1, 2), (dy.shape[3], x.shape[3], k, k),
                                       dy.float().permute(0, 3, 1, 2), s, p)


def _under(name, got, want, bound, dtype, worst):
    r = C.ratio(got.to(dtype), want, bound, dtype)
    worst[0] = max(worst[0], r)
    assert r <= 1.0, f"{name}: plain fp32 at {r:.3f} of the bound"


@pytest.mark.parametrize("cin,cout", C.HALO_CH)
def test_fp32_reference_under_the_halo_bound(cin, cout):
    worst = [0.0]
    for B, H, W in C.HALO_SHAPES + [C.HALO_LONG[:3]]:
        x, w, _, want, A = C.fwd_case(B, H, W, cin, cout, 3, 1, 1)
        _under(f"halo {B, H, W}", _f32_conv(x, w, None, 1, 1), want, C.acc_bound(C.halo_chain(cin), A), BF16, worst)
    print(f"conv3x3_halo {cin}->{cout}: plain fp32, bf16 output: {worst[0]:.3f} of the bound")
    assert worst[0] > 0.5  # the half ulp of bf16: tight, as it should be


@pytest.mark.parametrize("cin,cout", C.GEO_CH)
@pytest.mark.parametrize("k,s,p", C.GEO_KSP)
def test_fp32_reference_under_the_geometry_bounds(cin, cout, k, s, p):
    worst = [0.0]
    for H, W in C.GEO_HW:
        x, w, b, want, A = C.fwd_case(2, H, W, cin, cout, k, s, p, bias=(k == 1 and s == 1))
        _under("geo fwd", _f32_conv(x, w, b, s, p), want, C.geo_fwd_bound(A, k * k, cin, b is not None), BF16, worst)
        _, dy = C.bwd_case(2, H, W, cin, cout, k, s, p)
        dx, T = C.conv_dgrad(dy, w, (H, W), s, p)
        got = torch.nn.grad.conv2d_input((2, cin, H, W), w.float(), dy.float().permute(0, 3, 1, 2), s, p)
        _under("geo dgrad", got.permute(0, 2, 3, 1), dx, C.acc_bound(C.geo_dgrad_chain(k, cout), T), BF16,
               worst)
    print(f"conv_geo {k}x{k}/s{s} {cin}->{cout}: plain fp32, bf16 output: {worst[0]:.3f} of the bound")


@pytest.mark.parametrize("det", [False, True])
@pytest.mark.parametrize("cin", [64, 160])
@pytest.mark.parametrize("k,s,p", C.GEO_KSP)
def test_fp32_reference_under_the_strided_wgrad_bound(cin, k, s, p, det):
    worst = [0.0]
    ktot = cin if cin % 64 == 0 else cin + 32
    for i, (H, W) in enumerate(C.GEO_HW):
        cout = (96, 64)[i % 2]
        x, dy, dw, S, db, Sb = C.wgrad_case(2, H, W, cin, cout, k, s, p)
        P = dy.shape[0] * dy.shape[1] * dy.shape[2]
        _under("wgrad", _f32_wgrad(x, dy, k, s, p), dw, C.acc_bound(C.wgrad_chain(P, k * k, ktot, cout, det), S), F32, worst)
        _under("db", dy.float().sum((0, 1, 2)), db, C.acc_bound(C.wgrad_bias_chain(P, k * k, ktot, cout, det), Sb), F32,
               worst)
    print(f"conv_wgrad_strided {k}x{k}/s{s} cin {cin} det {det}: plain fp32 {worst[0]:.3f} of the bound")


@pytest.mark.parametrize("cin,cout", C.ENC_WGRAD_CH)
def test_fp32_reference_under_the_enc_wgrad_bound(cin, cout):
    worst = [0.0]
    for B, H, W in C.ENC_WGRAD_SHAPES:
        x, dy, dw, S, _, _ = C.wgrad_case(B, H, W, cin, cout, 3, 1, 1)
        _under(f"enc_wgrad {B, H, W}", _f32_wgrad(x, dy, 3, 1, 1), dw,
               C.acc_bound(C.enc_wgrad_chain(B, H, W, cin, cout), S), F32, worst)
    print(f"enc_wgrad {cin}->{cout}: plain fp32 {worst[0]:.3f} of the bound")


@pytest.mark.parametrize("dtype", [BF16, F32])
@pytest.mark.parametrize("cout", C.STEM_COUT)
def test_fp32_reference_under_the_stem_bounds(cout, dtype):
    worst = [0.0]
    for B in (1, 2):
        for H, W in C.STEM_HW:
            x, w = C.stem_case(B, H, W, cout, dtype)
            if dtype == F32:
                want, A = C.conv_fwd(x, w, None, 2, 3)
                bound = C.stem_bound(A, True, False)
                got = _f32_conv(x, w, None, 2, 3)
            else:
                want, A = C.conv_fwd(x, C.rb(w), None, 2, 3)
                bound = C.stem_bound(A, False, False)
                got = _f32_conv(x, C.rb(w), None, 2, 3)
            _under(f"stem {B, H, W}", got, want, bound, dtype, worst)
            ho, wo = C.out_hw(H, W, 7, 2, 3)
            dy = C.act((B, ho, wo, cout), BF16, C.gen(B, H, W, cout, 9))
            xr = C.rb(x.float())
            dw, S, _, _ = C.conv_wgrad(xr, dy, 7, 2, 3)
            _under(f"stem_wgrad {B, H, W}", _f32_wgrad(xr, dy, 7, 2, 3), dw,
                   C.acc_bound(C.stem_wgrad_chain(B, ho, wo), S), F32, worst)
    print(f"stem {dtype} C{cout}: plain fp32 {worst[0]:.3f} of the bound")


@pytest.mark.parametrize("dtype", [BF16, F32])
@pytest.mark.parametrize("s", [1, 2])
@pytest.mark.parametrize("k", [1, 3])
@pytest.mark.parametrize("cin,cout", C.SCONV_CH)
def test_fp32_reference_under_the_sconv_bounds(cin, cout, k, s, dtype):
    if not C.sconv_fits(cin, cout, k):
        return
    worst, p = [0.0], k // 2
    for B, H, W in C.SCONV_SHAPES[s]:
        x, w, b, want, A = C.sconv_case(B, H, W, cin, cout, k, s, dtype)
        assert float(want[0, 0, 0, 0].abs()) <= 2.0 ** -23 * float(A[0, 0, 0, 0])  # the planted cancelling output
        _under(f"sconv {B, H, W}", _f32_conv(x, w, b, s, p), want, C.acc_bound(C.sconv_chain(k, cin), A), dtype, worst)
        res = C.act(tuple(want.shape), dtype, C.gen(B, H, W, cin, cout, 11))
        wr, _ = C.epilogue(want, 0.0 * A, relu=True, res=res)
        got = torch.relu(torch.relu(_f32_conv(x, w, b, s, p)) + res.float())
        _under(f"sconv relu + res {B, H, W}", got, wr, C.acc_bound(C.sconv_chain(k, cin), A + res.double().abs()), dtype,
               worst)
    print(f"sconv {dtype} {k}x{k}/s{s} {cin}->{cout}: plain fp32 {worst[0]:.3f} of the bound")
    if s == 2 and C.sconv_fits(cout, cin, k):  # the zero-interleaved input gradient of _SConvTrain.backward
        for B, H, W in ((1, 9, 25), (1, 10, 26), (1, 2, 2), (1, 1, 1)):
            _, w, _, _, _ = C.fwd_case(B, H, W, cin, cout, k, 2, p, dtype, round_w=False)
            _, dy = C.bwd_case(B, H, W, cin, cout, k, 2, p, dtype)
            dx, T = C.conv_dgrad(dy, w, (H, W), 2, p)
            got = torch.nn.grad.conv2d_input((B, cin, H, W), w, dy.float().permute(0, 3, 1, 2), 2, p)
            _under(f"sconv s2 dgrad {B, H, W}", got.permute(0, 2, 3, 1), dx, C.acc_bound(C.sconv_chain(k, cout), T), dtype,
                   worst)


@pytest.mark.parametrize("dtype", [BF16, F32])
@pytest.mark.parametrize("s", [1, 2])
@pytest.mark.parametrize("cin,cout,k", C.SWG_CH)
def test_fp32_reference_under_the_sconv_wgrad_bound(cin, cout, k, s, dtype):
    worst, p = [0.0], k // 2
    for B, H, W in C.swg_shapes(s):
        x, dy, dw, S, _, _ = C.wgrad_case(B, H, W, cin, cout, k, s, p, dtype)
        ho, wo = dy.shape[1:3]
        _under(f"sconv_wgrad {B, H, W}", _f32_wgrad(x, dy, k, s, p), dw,
               C.acc_bound(C.sconv_wgrad_chain(B, ho, wo, cin, cout, k), S), F32, worst)
    print(f"sconv_wgrad {dtype} {k}x{k}/s{s} {cin}->{cout}: plain fp32 {worst[0]:.3f} of the bound")


def _f32_epilogue(acc, scale=None, shift=None, relu=False, res=None, res_relu=True):
    """The epilogue in plain fp32 on an fp32 accumulator."""
    v = acc
    if scale is not None:
        v = v * scale + shift
    if relu:
        v = torch.relu(v)
    if res is not None:
        v = v + res.float()
        v = torch.relu(v) if res_relu else v
    return v


@pytest.mark.parametrize("cin,cout", C.HALO_CH)
def test_fp32_reference_under_the_halo_epilogue_and_dgrad_bounds(cin, cout):
    worst = [0.0]
    B, H, W = 2, 9, 33
    x, w, _, acc, A = C.fwd_case(B, H, W, cin, cout, 3, 1, 1)
    scale, shift, res, y0 = C.epi_case(B, H, W, cout, cin)
    ab, a32 = C.acc_bound(C.halo_chain(cin), A), _f32_conv(x, w, None, 1, 1)
    for relu, r in ((False, None), (True, None), (True, res)):
        want, bound = C.epilogue(acc, ab, scale, shift, relu, r)
        _under(f"halo norm relu {relu} res {r is not None}", _f32_epilogue(a32, scale, shift, relu, r), want, bound, BF16,
               worst)
    want, bound = C.epilogue(acc, ab, res=y0, res_relu=False)
    _under("halo accumulate", _f32_epilogue(a32, res=y0, res_relu=False), want, bound, BF16, worst)
    if (cin, cout) in ((64, 64), (96, 96)):
        for B, H, W in ((1, 9, 33), (3, 9, 65)):
            _, w, _, _, _ = C.fwd_case(B, H, W, cin, cout, 3, 1, 1)
            _, dy = C.bwd_case(B, H, W, cin, cout, 3, 1, 1)
            dx, T = C.conv_dgrad(dy, w, (H, W), 1, 1)
            got = torch.nn.grad.conv2d_input((B, cin, H, W), w, dy.float().permute(0, 3, 1, 2), 1, 1)
            _under("halo dgrad", got.permute(0, 2, 3, 1), dx, C.acc_bound(C.halo_chain(cout), T), BF16, worst)
    print(f"conv3x3_halo epilogues / dgrad {cin}->{cout}: plain fp32 {worst[0]:.3f} of the bound")


@pytest.mark.parametrize("k,s,p", C.GEO_KSP)
def test_fp32_reference_under_the_geo_norm_and_pair_bounds(k, s, p):
    worst = [0.0]
    B, H, W, cin, cout = 2, 5, 6, 64, 96
    x, w, _, acc, A = C.fwd_case(B, H, W, cin, cout, k, s, p)
    ho, wo = C.out_hw(H, W, k, s, p)
    scale, shift, _, _ = C.epi_case(B, ho, wo, cout, k, s)
    want, bound = C.epilogue(acc, C.geo_fwd_bound(A, k * k, cin, False), scale, shift, relu=True)
    _under("geo norm", _f32_epilogue(_f32_conv(x, w, None, s, p), scale, shift, True), want, bound, BF16, worst)
    if k == 3:
        for cin, cout in ((64, 96), (96, 128)):
            for H, W in ((5, 6), (2, 2)):
                _, w1, _, _, _ = C.fwd_case(2, H, W, cin, cout, 3, 2, 1)
                _, wd, _, _, _ = C.fwd_case(2, H, W, cin, cout, 1, 2, 0)
                _, d1 = C.bwd_case(2, H, W, cin, cout, 3, 2, 1)
                _, dd = C.bwd_case(2, H, W, cin, cout, 1, 2, 0)
                a, Ta = C.conv_dgrad(d1, w1, (H, W), 2, 1)
                b, Tb = C.conv_dgrad(dd, wd, (H, W), 2, 0)
                ci = torch.nn.grad.conv2d_input
                got = ci((2, cin, H, W), w1, d1.float().permute(0, 3, 1, 2), 2, 1) + \
                    ci((2, cin, H, W), wd, dd.float().permute(0, 3, 1, 2), 2, 0)
                _under("pair dgrad", got.permute(0, 2, 3, 1), a + b, C.acc_bound(C.geo_dgrad_chain(3, cout), Ta + Tb), BF16,
                       worst)
    print(f"conv_geo norm / pair {k}x{k}/s{s}: plain fp32 {worst[0]:.3f} of the bound")


def test_fp32_reference_under_the_stem_norm_and_three_call_bounds():
    worst = [0.0]
    for dtype in (BF16, F32):
        for cout in C.STEM_COUT:
            for B, H, W in ((1, 1, 1), (2, 5, 129)):
                x, w = C.stem_case(B, H, W, cout, dtype)
                g = C.gen(B, H, W, cout, 8)
                bias = torch.randn(cout, generator=g)
                scale = (0.5 + torch.rand(cout, generator=g)) * torch.where(torch.arange(cout) % 3 == 0, -1.0, 1.0)
                wk = w if dtype == F32 else C.rb(w)
                acc, A = C.conv_fwd(x, wk, None, 2, 3)
                want, bound = C.epilogue(acc, C.stem_bound(A, dtype == F32, False), scale, bias, relu=True)
                _under("stem norm", _f32_epilogue(_f32_conv(x, wk, None, 2, 3), scale, bias, True), want, bound, dtype, worst)
                want, A = C.conv_fwd(x, wk, bias, 2, 3)
                _under("stem bias", _f32_conv(x, wk, bias, 2, 3), want, C.stem_bound(A, dtype == F32, True), dtype, worst)
    B, H, W, cout = 2, 14, 18, 64  # the fp32 three-call split weight gradient of enc_conv.stem
    x, _ = C.stem_case(B, H, W, cout, F32)
    ho, wo = C.out_hw(H, W, 7, 2, 3)
    dy = C.act((B, ho, wo, cout), F32, C.gen(B, H, W, cout, 10))
    dw, S, _, _ = C.conv_wgrad(x, dy, 7, 2, 3)
    (xh, xl), (dh, dl) = C.split_bf16(x), C.split_bf16(dy)
    Si = sum(C.conv_wgrad(a, b, 7, 2, 3)[1] for a, b in ((xh, dh), (xl, dh), (xh, dl)))
    bound = C.acc_bound(C.stem_wgrad_chain(B, ho, wo), Si) + C.split_bound(S) + 2 * C.U * S
    _under("stem three-call wgrad", _f32_wgrad(x, dy, 7, 2, 3), dw, bound, F32, worst)
    print(f"stem norm / bias / three-call wgrad: plain fp32 {worst[0]:.3f} of the bound")


@pytest.mark.parametrize("cin,cout", C.WRAPPER_CH)
def test_fp32_reference_under_the_wrapper_bounds(cin, cout):
    worst = [0.0]
    for B, H, W in C.WRAPPER_SHAPES:
        w = C.rb(C.weight(cout, cin, 3, C.gen(B, H, W, cin, cout, 12)))
        x, dy = C.bwd_case(B, H, W, cin, cout, 3, 1, 1)
        want, A = C.conv_fwd(x, w, None, 1, 1)
        _under("wrapper fwd", _f32_conv(x, w, None, 1, 1), want, C.acc_bound(C.wrapper_chain(cin), A), BF16, worst)
        dx, T = C.conv_dgrad(dy, w, (H, W), 1, 1)
        got = torch.nn.grad.conv2d_input((B, cin, H, W), w, dy.float().permute(0, 3, 1, 2), 1, 1)
        _under("wrapper dgrad", got.permute(0, 2, 3, 1), dx, C.acc_bound(C.wrapper_chain(cout), T), BF16, worst)
        dw, S, _, _ = C.conv_wgrad(x, dy, 3, 1, 1)
        _under("wrapper wgrad", _f32_wgrad(x, dy, 3, 1, 1), dw, C.acc_bound(C.enc_wgrad_chain(B, H, W, cin, cout), S), F32,
               worst)
    print(f"enc_conv.conv3x3 {cin}->{cout}: plain fp32 {worst[0]:.3f} of the bound")


# ------------------------------------------------------------------ 4. mutants
def _exceeds(name, mut, want, bound, dtype=None, must_touch=True):
    r = C.touched_ratio(mut, want, bound, dtype)
    if r is None:
        assert not must_touch, f"{name}: the mutant touches nothing"
        return None
    print(f"{name}: err/bound on the touched elements: max {r[0]:.1f}  median {r[1]:.2f}")
    assert r[0] > 1.0, f"{name}: the mutant stays under the bound ({r[0]:.3f})"
    return r


@pytest.mark.parametrize("cin,cout", C.HALO_CH)
def test_mutants_a_b_exceed_the_halo_bound(cin, cout):
    for B, H, W in C.HALO_SHAPES + [C.HALO_LONG[:3]]:
        x, w, _, want, A = C.fwd_case(B, H, W, cin, cout, 3, 1, 1)
        bound = C.acc_bound(C.halo_chain(cin), A)
        _exceeds(f"(a) dropped tap, halo {cin}->{cout} {B, H, W}", C.mutant_drop_border_tap(x, w, 1, 1), want, bound, BF16)
        mut = C.mutant_stale_halo(want, B, H, W)
        if mut is not None:  # shapes with a second tile
            _exceeds(f"(b) stale halo {cin}->{cout} {B, H, W}", mut, want, bound, BF16)


@pytest.mark.parametrize("k,s,p", C.GEO_KSP)
def test_mutant_a_exceeds_the_geometry_bound(k, s, p):
    cin, cout = 64, 96
    for H, W in C.GEO_HW:
        x, w, _, want, A = C.fwd_case(2, H, W, cin, cout, k, s, p)
        _exceeds(f"(a) dropped tap, geo {k}x{k}/s{s} {H}x{W}", C.mutant_drop_border_tap(x, w, s, p), want,
                 C.geo_fwd_bound(A, k * k, cin, False), BF16)


@pytest.mark.parametrize("cin,cout", [(64, 96), (64, 64)])
def test_mutants_c_d_exceed_the_phase_bound(cin, cout):
    """3x3/s2/p1: phase 1 has two taps ((0, k = 2), (1, k = 0)); with an even input the
    second tap of the last odd row points one past the dY grid."""
    k, s, p = 3, 2, 1
    for H, W in C.GEO_HW:
        _, w, _, _, _ = C.fwd_case(2, H, W, cin, cout, k, s, p)
        _, dy = C.bwd_case(2, H, W, cin, cout, k, s, p)
        want, T = C.conv_dgrad(dy, w, (H, W), s, p)
        bound = C.acc_bound(C.geo_dgrad_chain(3, cout), T)
        mc, _ = C.phase_dgrad(dy, w, (H, W), s, p, descending=True)
        # a phase with two taps exists in y from 2 input rows on, in x from 2 columns on
        _exceeds(f"(c) descending taps {H}x{W}", mc, want, bound, BF16, must_touch=(H >= 2 or W >= 2))
        md, _ = C.phase_dgrad(dy, w, (H, W), s, p, unmasked_tail=True)
        # touched: the last odd row of an even input, in every image but the last (zeros follow it)
        _exceeds(f"(d) unmasked tail {H}x{W}", md, want, bound, BF16, must_touch=(H % 2 == 0))


def test_mutant_e_keeps_the_weight_gradient_constants_honest():
    """One dropped pixel exceeds every weight-gradient bound at every case shape; with
    c = the pixel count in place of the real chain it would pass at a few thousand pixels."""
    for B, H, W in C.ENC_WGRAD_SHAPES:
        for cin, cout in C.ENC_WGRAD_CH[:2]:
            x, dy, dw, S, _, _ = C.wgrad_case(B, H, W, cin, cout, 3, 1, 1)
            _exceeds(f"(e) enc_wgrad {cin}->{cout} {B, H, W}", C.mutant_drop_last_pixel(x, dy, 3, 1, 1), dw,
                     C.acc_bound(C.enc_wgrad_chain(B, H, W, cin, cout), S))
    for k, s, p in C.GEO_KSP:
        for H, W in C.GEO_HW:
            x, dy, dw, S, _, _ = C.wgrad_case(2, H, W, 64, 96, k, s, p)
            P = dy.shape[0] * dy.shape[1] * dy.shape[2]
            for det in (False, True):
                _exceeds(f"(e) conv_wgrad_strided {k}x{k}/s{s} {H}x{W} det {det}", C.mutant_drop_last_pixel(x, dy, k, s, p),
                         dw, C.acc_bound(C.wgrad_chain(P, k * k, 64, 96, det), S))
    for dtype in (BF16, F32):
        for s in (1, 2):
            for cin, cout, k in C.SWG_CH:
                for B, H, W in C.swg_shapes(s):
                    x, dy, dw, S, _, _ = C.wgrad_case(B, H, W, cin, cout, k, s, k // 2, dtype)
                    ho, wo = dy.shape[1:3]
                    _exceeds(f"(e) sconv_wgrad {dtype} {k}x{k}/s{s} {cin}->{cout} {B, H, W}",
                             C.mutant_drop_last_pixel(x, dy, k, s, k // 2), dw,
                             C.acc_bound(C.sconv_wgrad_chain(B, ho, wo, cin, cout, k), S))
    for B, H, W in [(1, 1, 1), (2, 7, 7), (2, 6, 130), C.STEM_WGRAD_LONG]:
        x, _ = C.stem_case(B, H, W, 64, BF16)
        ho, wo = C.out_hw(H, W, 7, 2, 3)
        dy = C.act((B, ho, wo, 64), BF16, C.gen(B, H, W, 64, 9))
        dw, S, _, _ = C.conv_wgrad(x, dy, 7, 2, 3)
        _exceeds(f"(e) stem_wgrad {B, H, W}", C.mutant_drop_last_pixel(x, dy, 7, 2, 3), dw,
                 C.acc_bound(C.stem_wgrad_chain(B, ho, wo), S))
    # the constant matters: 11520 pixels (2 x 72 x 80), 64 -> 64
    B, H, W = 2, 72, 80
    x, dy, dw, S, _, _ = C.wgrad_case(B, H, W, 64, 64, 3, 1, 1)
    mut = C.mutant_drop_last_pixel(x, dy, 3, 1, 1)
    real = C.touched_ratio(mut, dw, C.acc_bound(C.enc_wgrad_chain(B, H, W, 64, 64), S))
    loose = C.touched_ratio(mut, dw, C.acc_bound(B * H * W, S))
    print(f"(e) 11520 pixels: real chain {C.enc_wgrad_chain(B, H, W, 64, 64)} U: max {real[0]:.1f} median {real[1]:.2f};"
          f" c = pixels: max {loose[0]:.2f} median {loose[1]:.2f}")
    assert real[1] > 1.0 and loose[1] < 1.0


@pytest.mark.parametrize("k", [1, 3])
@pytest.mark.parametrize("cin,cout", C.SCONV_CH)
def test_mutant_f_bf16_weights_exceed_the_sconv_bound(cin, cout, k):
    if not C.sconv_fits(cin, cout, k):
        return
    p = k // 2
    for s in (1, 2):
        for B, H, W in C.SCONV_SHAPES[s]:
            for dtype in (F32, BF16):
                x, w, b, want, A = C.sconv_case(B, H, W, cin, cout, k, s, dtype)
                mut, _ = C.conv_fwd(x, C.rb(w), b, s, p)
                _exceeds(f"(f) bf16 weights, {dtype} sconv {k}x{k}/s{s} {cin}->{cout} {B, H, W}", mut, want,
                         C.acc_bound(C.sconv_chain(k, cin), A), dtype)


@pytest.mark.parametrize("cout", C.STEM_COUT)
def test_mutant_g_hi_only_product_exceeds_the_fp32_stem_bound(cout):
    for B in (1, 2):
        for H, W in C.STEM_HW + [(14, 18)]:
            x, w = C.stem_case(B, H, W, cout, F32)
            want, A = C.conv_fwd(x, w, None, 2, 3)
            bound = C.stem_bound(A, True, False)
            three = C.stem_products(x, w, {"hh", "hl", "lh"})
            assert bool(((three - want).abs() <= C.split_bound(A)).all())  # what the derivation allots
            _exceeds(f"(g) hi-only stem C{cout} {B, H, W}", C.stem_products(x, w, {"hh"}), want, bound, F32)

"""The encoders' convolution kernels, each on its own, per element vs fp64 oracles.

csrc/stem.hip, csrc/enc_halo.hip, the GEO form of conv_lds_kernel (csrc/conv.hip),
the strided path of csrc/conv_wgrad.hip, csrc/enc_wgrad.hip, csrc/sconv.hip and
csrc/sconv_train.hip at the smallest shapes that reach every path of each launch:
H = 1, W = 1, less than one tile, one pixel below / at / above a block, stride 2
from inputs of 1, 2 and 3 pixels (empty phases), blocks of tiles that straddle
images.  The oracles (tests/enc_conv_cases.py: F.conv2d / conv2d_input /
conv2d_weight in float64 on the CPU; tests/test_enc_conv_oracles_cpu.py ties them
to autograd and shows that the bounds admit a plain fp32 evaluation and reject
seven mutants) take the values the kernels read, after rounding to the storage
dtype.  Every check prints max|err| and err / bound and asserts finiteness and
ratio <= 1 for EVERY element; outputs are pre-filled with NaN and everything
outside the written window must still be NaN.

Bounds.  U = 2^-24.  bf16 storage adds 2^-8 |want|.  An fp32 FMA / add counts
1 U of the magnitude term, an MFMA step 2 U (2^-23: its internal rounding is not
known to be to nearest).  A = conv(|x|, |w|) (+ |bias|), T = conv^T(|dy|, |w|),
S = wgrad(|x|, |dy|).  c is the longest chain of dependent roundings, read off
the kernel (the mirrors of the launch code are in enc_conv_cases.py):

conv3x3_halo   c = 2 * 9 * cin / 16 (one 32x32x16 MFMA per tap and 16 channels)
  epilogue     v = acc * scale + shift: |scale| bound + U (|acc scale| + |v|);
               ReLU 1-Lipschitz; + res / accumulate: + U |v + res|
stem_conv      bf16: c = 2 * 7 (one 16x16x32 MFMA per kernel row), + 1 for a bias add;
               fp32: 3 * 2^-18 A for the dropped lo * lo product and the operand
               remainders + c = 2 * 21 (+ 1); the norm form goes through `epilogue`
stem_wgrad     c = 2 * 4 * chunks_per_block + ceil(blocks / 16) + 16;
               three-call fp32 form: the three calls' c U S_i + 3 * 2^-18 S + 2 U S
conv_geo       forward c = 2 * taps * cin / 32 (16x16x32 MFMAs), + 1 for a bias add;
               input gradient c = 2 * 4 * cout / 32 for 3x3/s2 (the 2 x 2
               sub-kernel of phase (1, 1) is the longest; the pair's (0, 0) phase has
               1 tap x 2 cout), 2 * cout / 32 for 1x1
conv_wgrad_strided  c = 2 * 2 * kchunk / 64 + ksplit + 1; db: 2 or 4 rows per K step
               per thread + 32 or 16 threads per column + ksplit + 1
enc_wgrad      c = 2 * 8 * tiles_per_block + ceil(splits / 4) + 3
sconv          c = k k cin / 2 + 3: even / odd channels in two FMA chains, their sum,
               bias, residual; magnitude A + |res|.  FP32 weights (not bf16-rounded):
               every case has one output planted to cancel to ~2^-25 of its terms
               (enc_conv_cases.sconv_case), where bf16 storage hides nothing.
sconv_wgrad    c = rows_per_block * ceil(Wo / sublanes) + sublanes + ceil(blocks / 16) + 16
enc_conv.conv3x3 (autograd): forward / input gradient c = 2 * 9 * K / 16 with K = cin
               (128 for 96: two 64-channel windows) on the v3 tiles, which is also
               at least the implicit-GEMM and halo chains; weight gradient = enc_wgrad
Deterministic kernels (enc_wgrad, stem_wgrad, sconv_wgrad, conv_wgrad_strided in
deterministic mode) are called twice and must be bit-equal.

stem fp32 note: 3 * 2^-18 A is the allotment the flow encoder's test uses, not a
worst case (a value just above a power of two rounds to bf16 within 2^-8, not
2^-9); the stem images are seeded so that the exact three-product sum stays inside
it at the 1 x 1 and 2 x 2 images too (enc_conv_cases.stem_case; asserted on the CPU).
sconv 96 -> 32 3x3 is over the kernel's LDS limit (27648 > 16384 fp32 weights per
block): the host rejects it, which is what the test asserts; 96 -> 32 runs as 1x1.

Measured on an MI355X (largest err / bound over the cases of each check):
  conv3x3_halo        forward 0.989  epilogues 0.990  input gradient 0.987 (the half ulp of bf16)
  stem_conv           bf16 0.994, norm + relu 0.993;  fp32 0.337, norm + relu 0.693
  stem_wgrad          0.048;  fp32 three-call form through enc_conv.stem 0.225
  conv_geo            forward 0.995  norm + relu 0.991  input gradient 0.995  pair 0.990
  conv_wgrad_strided  dw 0.311  db 0.018 (atomic and deterministic alike)
  enc_wgrad           0.082
  sconv               bf16 0.994  fp32 0.301;  stride-2 input gradient bf16 0.987  fp32 0.250
  sconv_wgrad         bf16 0.063  fp32 0.096
  enc_conv.conv3x3    forward / input gradient 0.981  weight gradient 0.073
No kernel missed its bound; 2275 checks, 9 s for the file.
"""
import math

import pytest
import torch
import torch.nn as nn

import enc_conv_cases as C
from enc_conv_cases import BF16, F32, U

pytestmark = pytest.mark.gpu

NAN = math.nan
WORST = {}


def _check(name, got, want, bound, dtype=None, op=None):
    """max|err| and err / bound over every element (0 / 0 counts as 0)."""
    if dtype is not None:
        assert got.dtype == dtype, name
    got = got.detach().cpu()
    assert tuple(got.shape) == tuple(want.shape), (name, got.shape, want.shape)
    assert bool(torch.isfinite(got).all()), name
    r = C.ratio(got, want, bound, got.dtype)
    err = (got.double() - want).abs().max().item() if want.numel() else 0.0
    print(f"{name}: max|err| {err:.3e}  err/bound {r:.3f}")
    if op is not None:
        WORST[op] = max(WORST.get(op, 0.0), r)
        print(f"  worst so far {op}: {WORST[op]:.3f}")
    assert r <= 1.0, f"{name}: err/bound {r:.3f}"
    return r


def _wide(t, extra, dev, off=0):
    """``t`` (NHWC) inside a NaN buffer with ``extra`` more channels, at channel ``off``."""
    buf = torch.full((*t.shape[:3], t.shape[3] + extra), NAN, dtype=t.dtype)
    buf[..., off:off + t.shape[3]] = t
    return buf.to(dev)


def _untouched(buf, lo, hi, tag):
    keep = torch.ones(buf.shape[-1], dtype=torch.bool, device=buf.device)
    keep[lo:hi] = False
    assert bool(torch.isnan(buf[..., keep]).all()), tag + ": written outside the window"


def _param(w, dev):
    return nn.Parameter(w.to(dev))


# ------------------------------------------------------------------ conv3x3_halo
def _halo(x, wp, y, cin, cout, **kw):
    torch.ops.raft_stir.conv3x3_halo(x, wp, y, cin, cout, **kw)


@pytest.mark.parametrize("cin,cout", C.HALO_CH)
def test_conv3x3_halo(cuda, cin, cout):
    from raft_stir_amd.ops import enc_conv
    for B, H, W in C.HALO_SHAPES:
        x, w, _, want, A = C.fwd_case(B, H, W, cin, cout, 3, 1, 1)
        p = _param(w, cuda)
        wp = enc_conv._packed(p, False)
        bound = C.acc_bound(C.halo_chain(cin), A)
        for xe, ye in ((0, 0), (8, 4)):  # strides wider than cin / cout
            y = torch.full((B, H, W, cout + ye), NAN, device=cuda, dtype=BF16)
            _halo(_wide(x, xe, cuda), wp, y, cin, cout)
            tag = f"conv3x3_halo {cin}->{cout} {B, H, W} +{xe}/+{ye}"
            _check(tag, y[..., :cout], want, bound, BF16, "conv3x3_halo")
            _untouched(y, 0, cout, tag)


def test_conv3x3_halo_twelve_tiles_per_block(cuda):
    """343 one-pixel images x 3 channel blocks >= 1024 tile-blocks: 12 tiles per block,
    the last block has 7, every block walks across images."""
    from raft_stir_amd.ops import enc_conv
    B, H, W, cin, cout = C.HALO_LONG
    assert C.halo_tiles(B, H, W, cin, cout) == (343, 12)
    x, w, _, want, A = C.fwd_case(B, H, W, cin, cout, 3, 1, 1)
    y = torch.full((B, H, W, cout + 4), NAN, device=cuda, dtype=BF16)
    _halo(x.to(cuda), enc_conv._packed(_param(w, cuda), False), y, cin, cout)
    _check("conv3x3_halo 12-tile blocks", y[..., :cout], want, C.acc_bound(C.halo_chain(cin), A), BF16, "conv3x3_halo")
    _untouched(y, 0, cout, "12-tile")


@pytest.mark.parametrize("cin,cout", C.HALO_CH)
def test_conv3x3_halo_epilogues(cuda, cin, cout):
    from raft_stir_amd.ops import enc_conv
    B, H, W = 2, 9, 33
    x, w, _, acc, A = C.fwd_case(B, H, W, cin, cout, 3, 1, 1)
    scale, shift, res, y0 = C.epi_case(B, H, W, cout, cin)
    wp = enc_conv._packed(_param(w, cuda), False)
    ab = C.acc_bound(C.halo_chain(cin), A)
    xs = x.to(cuda)
    for relu, with_res in ((False, False), (True, False), (True, True)):
        want, bound = C.epilogue(acc, ab, scale, shift, relu, res if with_res else None)
        y = torch.full((B, H, W, cout + 4), NAN, device=cuda, dtype=BF16)
        _halo(xs, wp, y, cin, cout, nscale=scale.to(cuda), nshift=shift.to(cuda),
              res=_wide(res, 4, cuda) if with_res else None, relu=relu)  # the residual's own stride
        tag = f"conv3x3_halo {cin}->{cout} norm relu {relu} res {with_res}"
        _check(tag, y[..., :cout], want, bound, BF16, "conv3x3_halo epilogue")
        _untouched(y, 0, cout, tag)
    # accumulate: y += conv(x), y read as a plain residual
    want, bound = C.epilogue(acc, ab, res=y0, res_relu=False)
    y = _wide(y0, 4, cuda)
    _halo(xs, wp, y, cin, cout, accumulate=True)
    _check(f"conv3x3_halo {cin}->{cout} accumulate", y[..., :cout], want, bound, BF16, "conv3x3_halo epilogue")
    _untouched(y, 0, cout, "accumulate")


@pytest.mark.parametrize("cin,cout", [(64, 64), (96, 96)])
@pytest.mark.parametrize("B,H,W", [(1, 9, 33), (3, 9, 65)])
def test_conv3x3_halo_input_gradient(cuda, cin, cout, B, H, W):
    """dX = conv(dY, transposed flipped w): enc_conv._packed(weight, True)."""
    from raft_stir_amd.ops import enc_conv
    _, w, _, _, _ = C.fwd_case(B, H, W, cin, cout, 3, 1, 1)
    _, dy = C.bwd_case(B, H, W, cin, cout, 3, 1, 1)
    want, T = C.conv_dgrad(dy, w, (H, W), 1, 1)
    dx = torch.full((B, H, W, cin + 4), NAN, device=cuda, dtype=BF16)
    _halo(dy.to(cuda), enc_conv._packed(_param(w, cuda), True), dx, cout, cin)
    _check(f"conv3x3_halo dgrad {cin}<-{cout} {B, H, W}", dx[..., :cin], want, C.acc_bound(C.halo_chain(cout), T),
           BF16, "conv3x3_halo dgrad")
    _untouched(dx, 0, cin, "halo dgrad")


# ------------------------------------------------------------------ enc_wgrad
@pytest.mark.parametrize("cin,cout", C.ENC_WGRAD_CH)
def test_enc_wgrad(cuda, cin, cout):
    for B, H, W in C.ENC_WGRAD_SHAPES:
        x, dy, dw, S, _, _ = C.wgrad_case(B, H, W, cin, cout, 3, 1, 1)
        got = torch.ops.raft_stir.enc_wgrad(dy.to(cuda), x.to(cuda))
        bound = C.acc_bound(C.enc_wgrad_chain(B, H, W, cin, cout), S)
        _check(f"enc_wgrad {cin}->{cout} {B, H, W}", got, dw, bound, F32, "enc_wgrad")
        again = torch.ops.raft_stir.enc_wgrad(dy.to(cuda), x.to(cuda))
        assert torch.equal(got, again)


def test_enc_wgrad_channel_strided_views(cuda):
    B, H, W, cin, cout = 2, 9, 33, 96, 64
    x, dy, dw, S, _, _ = C.wgrad_case(B, H, W, cin, cout, 3, 1, 1)
    xv = _wide(x, 16, cuda, off=8)[..., 8:8 + cin]
    dv = _wide(dy, 24, cuda, off=16)[..., 16:16 + cout]
    got = torch.ops.raft_stir.enc_wgrad(dv, xv)
    _check("enc_wgrad strided views", got, dw, C.acc_bound(C.enc_wgrad_chain(B, H, W, cin, cout), S), F32, "enc_wgrad")


# ------------------------------------------------------------------ stem
def _stem_packed(w, f32, dev):
    from raft_stir_amd.ops import enc_conv
    from raft_stir_amd.ops.conv import split_weight
    t = enc_conv._stem_layout([w])  # [64][7][32] fp32
    return (split_weight(t) if f32 else t.to(BF16)).contiguous().to(dev)


def _stem_oracle(x, w, bias, f32):
    """(acc, bound of acc) of the stem conv: bf16 operands, or the split fp32 form."""
    if f32:
        acc, A = C.conv_fwd(x, w, bias, 2, 3)
        return acc, C.stem_bound(A, True, bias is not None)
    acc, A = C.conv_fwd(x, C.rb(w), bias, 2, 3)
    return acc, C.stem_bound(A, False, bias is not None)


@pytest.mark.parametrize("dtype", [BF16, F32])
@pytest.mark.parametrize("cout", C.STEM_COUT)
def test_stem_conv(cuda, cout, dtype):
    from raft_stir_amd.ops.conv import EPI_NORM
    f32 = dtype == F32
    for B in (1, 2):
        for H, W in C.STEM_HW:
            x, w = C.stem_case(B, H, W, cout, dtype)
            g = C.gen(B, H, W, cout, 8)
            bias = torch.randn(cout, generator=g)
            scale = (0.5 + torch.rand(cout, generator=g)) * torch.where(torch.arange(cout) % 3 == 0, -1.0, 1.0)
            wp = _stem_packed(w, f32, cuda)
            ho, wo = C.out_hw(H, W, 7, 2, 3)
            tag = f"stem_conv {dtype} C{cout} {B, H, W}"
            # epi 0: conv + bias
            want, bound = _stem_oracle(x, w, bias, f32)
            out = torch.full((B, ho, wo, cout + 4), NAN, device=cuda, dtype=dtype)
            torch.ops.raft_stir.stem_conv(x.to(cuda), wp, bias.to(cuda), out, cout, 0)
            _check(tag + " bias", out[..., :cout], want, bound, dtype, f"stem_conv {dtype}")
            _untouched(out, 0, cout, tag)
            # EPI_NORM: relu(conv * scale + shift)
            acc, ab = _stem_oracle(x, w, None, f32)
            want, bound = C.epilogue(acc, ab, scale, bias, relu=True)
            out = torch.full((B, ho, wo, cout + 4), NAN, device=cuda, dtype=dtype)
            torch.ops.raft_stir.stem_conv(x.to(cuda), wp, bias.to(cuda), out, cout, EPI_NORM, scale.to(cuda), True)
            _check(tag + " norm relu", out[..., :cout], want, bound, dtype, f"stem_conv {dtype} norm")
            _untouched(out, 0, cout, tag)


def test_stem_conv_fp32_image_bf16_output(cuda):
    """Autocast: the fp32 image is rounded to bf16 on the way in."""
    B, H, W, cout = 2, 5, 129, 64
    x, w = C.stem_case(B, H, W, cout, F32)
    want, bound = _stem_oracle(C.rb(x), w, None, False)
    ho, wo = C.out_hw(H, W, 7, 2, 3)
    out = torch.full((B, ho, wo, cout), NAN, device=cuda, dtype=BF16)
    torch.ops.raft_stir.stem_conv(x.to(cuda), _stem_packed(w, False, cuda), None, out, cout, 0)
    _check("stem_conv fp32 image -> bf16", out, want, bound, BF16, "stem_conv torch.bfloat16")


def _stem_wgrad_case(B, H, W, cout, dtype):
    x, _ = C.stem_case(B, H, W, cout, dtype)
    ho, wo = C.out_hw(H, W, 7, 2, 3)
    dy = C.act((B, ho, wo, cout), BF16, C.gen(B, H, W, cout, 9))
    dw, S, _, _ = C.conv_wgrad(C.rb(x.float()), dy, 7, 2, 3)  # an fp32 image is rounded to bf16 while staged
    return x, dy, dw, S, ho, wo


@pytest.mark.parametrize("dtype", [BF16, F32])
@pytest.mark.parametrize("cout", [32, 64])
def test_stem_wgrad(cuda, cout, dtype):
    shapes = [(B, H, W) for B in (1, 2) for H, W in C.STEM_HW] + [C.STEM_WGRAD_LONG]
    assert C.stem_wgrad_blocks(1, 1, 1) == (1, 1)  # a single partial chunk in total
    assert C.stem_wgrad_blocks(2, 129, 65) == (258, 2)  # blocks of two chunks crossing rows and images
    for B, H, W in shapes:
        x, dy, dw, S, ho, wo = _stem_wgrad_case(B, H, W, cout, dtype)
        dyw = _wide(dy, 8, cuda)  # dy stride wider than Cout
        got = torch.full((cout, 3, 7, 7), NAN, device=cuda)
        torch.ops.raft_stir.stem_wgrad(x.to(cuda), dyw, cout, got)
        _check(f"stem_wgrad {dtype} C{cout} {B, H, W}", got, dw, C.acc_bound(C.stem_wgrad_chain(B, ho, wo), S), F32,
               "stem_wgrad")
        again = torch.full_like(got, NAN)
        torch.ops.raft_stir.stem_wgrad(x.to(cuda), dyw, cout, again)
        assert torch.equal(got, again)


def test_stem_fp32_training_through_the_wrapper(cuda):
    """enc_conv.stem in fp32: split forward, three-product split weight gradient."""
    from raft_stir_amd.ops import enc_conv
    B, H, W, cout = 2, 14, 18, 64
    x, w = C.stem_case(B, H, W, cout, F32)
    ho, wo = C.out_hw(H, W, 7, 2, 3)
    dy = C.act((B, ho, wo, cout), F32, C.gen(B, H, W, cout, 10))
    conv = nn.Conv2d(3, cout, 7, stride=2, padding=3).to(cuda)
    with torch.no_grad():
        conv.weight.copy_(w)
    xin = x.permute(0, 3, 1, 2).to(cuda).contiguous(memory_format=torch.channels_last)
    assert enc_conv.stem_eligible(conv, xin)
    y = enc_conv.stem(conv, xin)
    want, bound = _stem_oracle(x, w, None, True)
    _check("enc_conv.stem fp32 forward", y.permute(0, 2, 3, 1), want, bound, F32, "stem_conv torch.float32")
    y.backward(dy.permute(0, 3, 1, 2).to(cuda))
    dw, S, _, _ = C.conv_wgrad(x, dy, 7, 2, 3)
    (xh, xl), (dh, dl) = C.split_bf16(x), C.split_bf16(dy)
    Si = sum(C.conv_wgrad(a, b, 7, 2, 3)[1] for a, b in ((xh, dh), (xl, dh), (xh, dl)))
    bound = C.acc_bound(C.stem_wgrad_chain(B, ho, wo), Si) + C.split_bound(S) + 2 * U * S
    _check("enc_conv.stem fp32 weight gradient", conv.weight.grad, dw, bound, F32, "stem_wgrad fp32 split")


# ------------------------------------------------------------------ strided / 1x1 geometry conv
def _nchw_cuda(x, dev):
    return x.permute(0, 3, 1, 2).to(dev).contiguous(memory_format=torch.channels_last)


@pytest.mark.parametrize("cin,cout", C.GEO_CH)
@pytest.mark.parametrize("k,s,p", C.GEO_KSP)
def test_conv_geo_forward(cuda, cin, cout, k, s, p):
    from raft_stir_amd.ops import enc_conv
    for H, W in C.GEO_HW:
        x, w, b, want, A = C.fwd_case(2, H, W, cin, cout, k, s, p, bias=(k == 1 and s == 1))
        got = enc_conv._conv_geo_fwd(_nchw_cuda(x, cuda), _param(w, cuda), None if b is None else b.to(cuda),
                                     (s, s), (p, p))
        _check(f"conv_geo {k}x{k}/s{s} {cin}->{cout} {H}x{W}", got, want, C.geo_fwd_bound(A, k * k, cin, b is not None),
               BF16, "conv_geo forward")


def test_conv_geo_forward_channel_window(cuda):
    """The op itself with ooff = 8 into a wider NaN buffer."""
    from raft_stir_amd.ops import enc_conv
    B, H, W, cin, cout = 2, 5, 6, 64, 96
    x, w, _, want, A = C.fwd_case(B, H, W, cin, cout, 3, 2, 1)
    ho, wo = C.out_hw(H, W, 3, 2, 1)
    out = torch.full((B, ho, wo, cout + 16), NAN, device=cuda, dtype=BF16)
    torch.ops.raft_stir.conv_geo([x.to(cuda)], [0], [cin], enc_conv._fwd_weight(_param(w, cuda)), None, 3, 3, 1, 1, 2, 2,
                                 ho, wo, cout, out, 8, 1, 1, 0, 0, enc_conv._geo_tile(cout, [cin]))
    _check("conv_geo ooff 8", out[..., 8:8 + cout], want, C.geo_fwd_bound(A, 9, cin, False), BF16,
           "conv_geo forward")
    _untouched(out, 8, 8 + cout, "conv_geo ooff")


@pytest.mark.parametrize("k,s,p", C.GEO_KSP)
def test_conv_geo_norm_epilogue(cuda, k, s, p):
    """enc_conv.conv_norm's strided form: relu(conv * scale + shift) in the epilogue."""
    from raft_stir_amd.ops import enc_conv
    B, H, W, cin, cout = 2, 5, 6, 64, 96
    x, w, _, acc, A = C.fwd_case(B, H, W, cin, cout, k, s, p)
    ho, wo = C.out_hw(H, W, k, s, p)
    scale, shift, _, _ = C.epi_case(B, ho, wo, cout, k, s)
    want, bound = C.epilogue(acc, C.geo_fwd_bound(A, k * k, cin, False), scale, shift, relu=True)
    out = torch.full((B, ho, wo, cout + 8), NAN, device=cuda, dtype=BF16)
    torch.ops.raft_stir.conv_geo([x.to(cuda)], [0], [cin], enc_conv._fwd_weight(_param(w, cuda)), shift.to(cuda), k, k,
                                 p, p, s, s, ho, wo, cout, out, 0, 1, 1, 0, 0, enc_conv._geo_tile(cout, [cin]),
                                 scale.to(cuda), True)
    _check(f"conv_geo {k}x{k}/s{s} norm relu", out[..., :cout], want, bound, BF16, "conv_geo norm")
    _untouched(out, 0, cout, "conv_geo norm")


@pytest.mark.parametrize("cin,cout", C.GEO_CH)
@pytest.mark.parametrize("k,s,p", C.GEO_KSP)
def test_conv_geo_input_gradient(cuda, cin, cout, k, s, p):
    """Every phase written once with the right taps; empty phases (extent 1); the
    one-past-the-grid tap of the last odd row of an even input masked; for 1x1/s2
    the three unused phases exactly zero."""
    from raft_stir_amd.ops import enc_conv
    chain = C.geo_dgrad_chain(k, cout)
    for H, W in C.GEO_HW:
        _, w, _, _, _ = C.fwd_case(2, H, W, cin, cout, k, s, p)
        _, dy = C.bwd_case(2, H, W, cin, cout, k, s, p)
        want, T = C.conv_dgrad(dy, w, (H, W), s, p)
        got = enc_conv._conv_geo_dgrad([dy.to(cuda)], [_param(w, cuda)], (2, cin, H, W), (s, s), (p, p))
        _check(f"conv_geo dgrad {k}x{k}/s{s} {cin}<-{cout} {H}x{W}", got, want, C.acc_bound(chain, T), BF16,
               "conv_geo dgrad")
        if k == 1 and s == 2:
            z = got.clone()
            z[:, ::2, ::2] = 0
            assert not bool(z.any()), "1x1/s2: the unused phases must be exactly zero"


@pytest.mark.parametrize("cin,cout", [(64, 96), (96, 128)])
@pytest.mark.parametrize("H,W", [(5, 6), (2, 2)])
def test_conv_geo_pair_input_gradient(cuda, cin, cout, H, W):
    """3x3/s2 + the 1x1/s2 shortcut fused into phase (0, 0) as a second K segment."""
    from raft_stir_amd.ops import enc_conv
    _, w1, _, _, _ = C.fwd_case(2, H, W, cin, cout, 3, 2, 1)
    _, wd, _, _, _ = C.fwd_case(2, H, W, cin, cout, 1, 2, 0)
    _, d1 = C.bwd_case(2, H, W, cin, cout, 3, 2, 1)
    _, dd = C.bwd_case(2, H, W, cin, cout, 1, 2, 0)
    a, Ta = C.conv_dgrad(d1, w1, (H, W), 2, 1)
    b, Tb = C.conv_dgrad(dd, wd, (H, W), 2, 0)
    got = enc_conv._pair_dgrad(d1.to(cuda), dd.to(cuda), _param(w1, cuda), _param(wd, cuda), (2, cin, H, W), (2, 2))
    _check(f"pair dgrad {cin}<-{cout} {H}x{W}", got, a + b, C.acc_bound(C.geo_dgrad_chain(3, cout), Ta + Tb), BF16,
           "conv_geo pair dgrad")


@pytest.mark.parametrize("det", [False, True])
@pytest.mark.parametrize("cin", C.GEO_WGRAD_CIN)
@pytest.mark.parametrize("k,s,p", C.GEO_KSP)
def test_conv_wgrad_strided(cuda, cin, k, s, p, det):
    from raft_stir_amd.ops import enc_conv
    from raft_stir_amd.runtime import determinism
    ktot = cin if cin % 64 == 0 else cin + 32  # overlapping 64-channel windows
    for i, (H, W) in enumerate(C.GEO_HW):
        cout = (96, 64)[i % 2]
        x, dy, dw, S, db, Sb = C.wgrad_case(2, H, W, cin, cout, k, s, p)
        P = dy.shape[0] * dy.shape[1] * dy.shape[2]
        wpar = _param(torch.zeros(cout, cin, k, k), cuda)
        with determinism.deterministic(det):
            for want_b in (False, True):
                gw, gb = enc_conv._conv_geo_wgrad(dy.to(cuda), _nchw_cuda(x, cuda), wpar, (s, s), want_b)
                tag = f"conv_wgrad_strided {k}x{k}/s{s} {cin}->{cout} {H}x{W} det {det} db {want_b}"
                _check(tag, gw, dw, C.acc_bound(C.wgrad_chain(P, k * k, ktot, cout, det), S), F32, "conv_wgrad_strided")
                if want_b:
                    _check(tag + " db", gb, db, C.acc_bound(C.wgrad_bias_chain(P, k * k, ktot, cout, det), Sb), F32,
                           "conv_wgrad_strided db")
                else:
                    assert gb is None
                if det:
                    gw2, gb2 = enc_conv._conv_geo_wgrad(dy.to(cuda), _nchw_cuda(x, cuda), wpar, (s, s), want_b)
                    assert torch.equal(gw, gw2) and (gb is None or torch.equal(gb, gb2))


# ------------------------------------------------------------------ sconv
def _sconv_w(w):
    """fp32 [Cout, KH, KW, Cin] as enc_conv._sconv_weight lays it out."""
    return w.permute(0, 2, 3, 1).contiguous()


@pytest.mark.parametrize("dtype", [BF16, F32])
@pytest.mark.parametrize("s", [1, 2])
@pytest.mark.parametrize("k", [1, 3])
@pytest.mark.parametrize("cin,cout", C.SCONV_CH)
def test_sconv(cuda, cin, cout, k, s, dtype):
    if not C.sconv_fits(cin, cout, k):  # 96 -> 32 3x3: 27648 weights per block, over the LDS limit (host-checked)
        with pytest.raises(RuntimeError, match="weight tile too large"):
            torch.ops.raft_stir.sconv(torch.zeros(1, 1, 1, cin, device=cuda, dtype=dtype),
                                      torch.zeros(cout, k, k, cin, device=cuda), None, s, k // 2, False,
                                      torch.zeros(1, 1, 1, cout, device=cuda, dtype=dtype), 0, None)
        return
    p = k // 2
    for B, H, W in C.SCONV_SHAPES[s]:
        x, w, b, _, _ = C.sconv_case(B, H, W, cin, cout, k, s, dtype)  # one output cancels to ~0: pins fp32 weights
        ho, wo = C.out_hw(H, W, k, s, p)
        res = C.act((B, ho, wo, cout), dtype, C.gen(B, H, W, cin, cout, 11))
        chain = C.sconv_chain(k, cin)
        wk = _sconv_w(w).to(cuda)
        # (bias, relu, residual, yoff, extra channels, x as a channel window of a wider buffer)
        for bias, relu, with_res, yoff, extra, xwin in ((True, False, False, 0, 0, False),
                                                        (False, True, False, 8, 16, True),
                                                        (True, True, True, 0, 0, False),
                                                        (True, True, True, 8, 8, True)):
            acc, A = C.conv_fwd(x, w, b if bias else None, s, p)
            mag = A + (res.double().abs() if with_res else 0.0)
            want, _ = C.epilogue(acc, 0.0 * A, relu=relu, res=res if with_res else None)
            xs = _wide(x, 16, cuda, off=8)[..., 8:8 + cin] if xwin else x.to(cuda)
            out = torch.full((B, ho, wo, cout + extra), NAN, device=cuda, dtype=dtype)
            torch.ops.raft_stir.sconv(xs, wk, b.to(cuda) if bias else None, s, p, relu, out, yoff,
                                      res.to(cuda) if with_res else None)
            tag = f"sconv {dtype} {k}x{k}/s{s} {cin}->{cout} {B, H, W} bias {bias} relu {relu} res {with_res} yoff {yoff}"
            _check(tag, out[..., yoff:yoff + cout], want, C.acc_bound(chain, mag), dtype, f"sconv {dtype}")
            _untouched(out, yoff, yoff + cout, tag)


@pytest.mark.parametrize("dtype", [BF16, F32])
@pytest.mark.parametrize("k", [1, 3])
@pytest.mark.parametrize("cin,cout", [(8, 8), (16, 24), (32, 40)])
def test_sconv_stride2_input_gradient(cuda, cin, cout, k, dtype):
    """_SConvTrain.backward: dY zero-interleaved onto the input grid, a stride-1 conv
    with the flipped, transposed fp32 weight; at an odd and an even input."""
    from raft_stir_amd.ops import enc_conv
    p = k // 2
    for B, H, W in ((1, 9, 25), (1, 10, 26), (1, 2, 2), (1, 1, 1)):
        _, w, _, _, _ = C.fwd_case(B, H, W, cin, cout, k, 2, p, dtype, round_w=False)
        _, dy = C.bwd_case(B, H, W, cin, cout, k, 2, p, dtype)
        want, T = C.conv_dgrad(dy, w, (H, W), 2, p)
        src = torch.zeros(B, H, W, cout, device=cuda, dtype=dtype)
        src[:, ::2, ::2] = dy.to(cuda)
        dx = torch.full((B, H, W, cin), NAN, device=cuda, dtype=dtype)
        torch.ops.raft_stir.sconv(src, enc_conv._sconv_dgrad_weight(w.to(cuda)), None, 1, p, False, dx, 0, None)
        _check(f"sconv s2 dgrad {dtype} {k}x{k} {cin}<-{cout} {B, H, W}", dx, want,
               C.acc_bound(C.sconv_chain(k, cout), T), dtype, f"sconv dgrad {dtype}")


# sconv's channels x k in {1, 3} (8 -> 8 1x1: one thread group with 256 pixel sub-lanes;
# 32 -> 40 3x3: 180 groups, just under 256; 24 -> 96 3x3: 324 and 96 -> 32 3x3: 432, two
# passes without sub-lanes) and 16 -> 12 for the CO = 4 thread tile (Cout % 8 != 0)

@pytest.mark.parametrize("dtype", [BF16, F32])
@pytest.mark.parametrize("s", [1, 2])
@pytest.mark.parametrize("cin,cout,k", C.SWG_CH)
def test_sconv_wgrad(cuda, cin, cout, k, s, dtype):
    assert C.sconv_wgrad_lanes(8, 8, 1) == (1, 256, 8) and C.sconv_wgrad_lanes(16, 12, 3) == (54, 4, 4)
    assert C.sconv_wgrad_lanes(32, 40, 3) == (180, 1, 8) and C.sconv_wgrad_lanes(24, 96, 3) == (324, 1, 8)
    assert C.sconv_wgrad_lanes(96, 32, 3) == (432, 1, 8)
    assert C.sconv_wgrad_blocks(3, 70, 96 * 9 * 24) == (105, 2)  # several rows per block
    p = k // 2
    for B, H, W in C.swg_shapes(s):
        x, dy, dw, S, _, _ = C.wgrad_case(B, H, W, cin, cout, k, s, p, dtype)
        ho, wo = dy.shape[1:3]
        got = torch.full((cout, k, k, cin), NAN, device=cuda)
        torch.ops.raft_stir.sconv_wgrad(dy.to(cuda), x.to(cuda), k, k, s, p, got)
        chain = C.sconv_wgrad_chain(B, ho, wo, cin, cout, k)
        _check(f"sconv_wgrad {dtype} {k}x{k}/s{s} {cin}->{cout} {B, H, W}", got.permute(0, 3, 1, 2), dw,
               C.acc_bound(chain, S), F32, f"sconv_wgrad {dtype}")
        again = torch.full_like(got, NAN)
        torch.ops.raft_stir.sconv_wgrad(dy.to(cuda), x.to(cuda), k, k, s, p, again)
        assert torch.equal(got, again)


# ------------------------------------------------------------------ wrapper
@pytest.mark.parametrize("v3", [True, False])
@pytest.mark.parametrize("cin,cout", C.WRAPPER_CH)
@pytest.mark.parametrize("B,H,W", C.WRAPPER_SHAPES)
def test_conv3x3_wrapper_autograd(cuda, B, H, W, cin, cout, v3, monkeypatch):
    """enc_conv.conv3x3 forward, input and weight gradient: the v3 tiles, and with
    them off the halo kernel (64 -> 64, 96 -> 96) and the implicit GEMM."""
    from raft_stir_amd.ops import enc_conv
    monkeypatch.setattr(enc_conv, "_V3", v3)
    g = C.gen(B, H, W, cin, cout, 12)
    w = C.weight(cout, cin, 3, g)  # fp32 parameter: the wrapper packs it to bf16
    x, dy = C.bwd_case(B, H, W, cin, cout, 3, 1, 1)
    conv = nn.Conv2d(cin, cout, 3, padding=1, bias=False).to(cuda)
    with torch.no_grad():
        conv.weight.copy_(w)
    xin = _nchw_cuda(x, cuda).requires_grad_(True)
    assert enc_conv.eligible(conv, xin)
    y = enc_conv.conv3x3(conv, xin)
    y.backward(_nchw_cuda(dy, cuda))
    kf = C.wrapper_chain
    want, A = C.conv_fwd(x, C.rb(w), None, 1, 1)
    tag = f"conv3x3 {cin}->{cout} {B, H, W} v3 {v3}"
    _check(tag + " forward", y.permute(0, 2, 3, 1), want, C.acc_bound(kf(cin), A), BF16, "conv3x3 wrapper")
    dx, T = C.conv_dgrad(dy, C.rb(w), (H, W), 1, 1)
    _check(tag + " dgrad", xin.grad.permute(0, 2, 3, 1), dx, C.acc_bound(kf(cout), T), BF16, "conv3x3 wrapper")
    dw, S, _, _ = C.conv_wgrad(x, dy, 3, 1, 1)
    _check(tag + " wgrad", conv.weight.grad, dw, C.acc_bound(C.enc_wgrad_chain(B, H, W, cin, cout), S), F32,
           "conv3x3 wrapper wgrad")


# ------------------------------------------------------------------ host checks
def test_conv_wgrad_strided_rejects_a_mismatched_grid(cuda):
    """dY's grid must be (Hi + 2 (K / 2) - K) / S + 1 of the input grid."""
    x = torch.zeros(1, 6, 6, 64, device=cuda, dtype=BF16)
    acc = torch.zeros(128, 9, 64, device=cuda)
    for ho, wo in ((2, 3), (3, 4), (6, 6)):
        dy = torch.zeros(1, ho, wo, 64, device=cuda, dtype=BF16)
        with pytest.raises(RuntimeError, match="does not match the conv geometry"):
            torch.ops.raft_stir.conv_wgrad_strided(dy, 64, [x], [0], [64], 3, 3, 2, 2, acc, None)
    acc1 = torch.zeros(128, 1, 64, device=cuda)
    with pytest.raises(RuntimeError, match="does not match the conv geometry"):
        torch.ops.raft_stir.conv_wgrad_strided(torch.zeros(1, 4, 3, 64, device=cuda, dtype=BF16), 64, [x], [0], [64],
                                               1, 1, 2, 2, acc1, None)
    torch.ops.raft_stir.conv_wgrad_strided(torch.zeros(1, 3, 3, 64, device=cuda, dtype=BF16), 64, [x], [0], [64],
                                           3, 3, 2, 2, acc, None)  # the matching grid is accepted
    assert not bool(acc.any())


def test_ops_reject_tensors_on_two_devices(cuda):
    """A tensor from another device (here the host) is rejected before any launch,
    by the one-device check, in every op that takes raw pointers from several tensors."""
    from raft_stir_amd.ops.conv import EPI_NORM
    ops = torch.ops.raft_stir
    bf = lambda *s: torch.zeros(*s, device=cuda, dtype=BF16)
    f = lambda *s: torch.zeros(*s, device=cuda)
    one = pytest.raises(RuntimeError, match="must be on one device")
    with one:
        ops.enc_wgrad(bf(1, 1, 1, 64).cpu(), bf(1, 1, 1, 64))
    with one:
        ops.stem_wgrad(bf(1, 1, 1, 3), bf(1, 1, 1, 64).cpu(), 64, f(64, 3, 7, 7))
    with one:
        ops.stem_wgrad(bf(1, 1, 1, 3), bf(1, 1, 1, 64), 64, f(64, 3, 7, 7).cpu())
    with one:
        ops.sconv(bf(1, 1, 1, 8), f(8, 1, 1, 8).cpu(), None, 1, 0, False, bf(1, 1, 1, 8), 0, None)
    with one:
        ops.sconv(bf(1, 1, 1, 8), f(8, 1, 1, 8), f(8).cpu(), 1, 0, False, bf(1, 1, 1, 8), 0, None)
    with one:
        ops.sconv(bf(1, 1, 1, 8), f(8, 1, 1, 8), None, 1, 0, False, bf(1, 1, 1, 8), 0, bf(1, 1, 1, 8).cpu())
    with one:
        ops.sconv_wgrad(bf(1, 1, 1, 8).cpu(), bf(1, 1, 1, 8), 1, 1, 1, 0, f(8, 1, 1, 8))
    with one:
        ops.sconv_wgrad(bf(1, 1, 1, 8), bf(1, 1, 1, 8), 1, 1, 1, 0, f(8, 1, 1, 8).cpu())
    with one:
        ops.stem_conv(bf(1, 1, 1, 3), bf(64, 7, 32).cpu(), None, bf(1, 1, 1, 64), 64, 0)
    with one:
        ops.stem_conv(bf(1, 1, 1, 3), bf(64, 7, 32), f(64).cpu(), bf(1, 1, 1, 64), 64, 0)
    with one:
        ops.stem_conv(bf(1, 1, 1, 3), bf(64, 7, 32), None, bf(1, 1, 1, 64).cpu(), 64, 0)
    with one:
        ops.stem_conv(bf(1, 1, 1, 3), bf(64, 7, 32), f(64), bf(1, 1, 1, 64), 64, EPI_NORM, f(64).cpu(), True)
    with one:
        ops.conv_wgrad_strided(bf(1, 1, 1, 64), 64, [bf(1, 1, 1, 64)], [0], [64], 1, 1, 1, 1, f(128, 1, 64).cpu(), None)
    with one:
        ops.conv_wgrad_strided(bf(1, 1, 1, 64), 64, [bf(1, 1, 1, 64)], [0], [64], 1, 1, 1, 1, f(128, 1, 64), f(64).cpu())
    with one:
        ops.conv_wgrad_strided(bf(1, 1, 1, 64), 64, [bf(1, 1, 1, 64).cpu()], [0], [64], 1, 1, 1, 1, f(128, 1, 64), None)
    with one:
        ops.conv_wgrad(bf(1, 1, 1, 64), 0, 64, [bf(1, 1, 1, 64)], [0], [64], [1], 1, 1, f(128, 1, 64).cpu(), None, 0)
    with one:
        ops.conv3x3_halo(bf(1, 1, 1, 64), bf(128, 9, 64).cpu(), bf(1, 1, 1, 64), 64, 64)
    with one:
        ops.conv3x3_halo(bf(1, 1, 1, 64), bf(128, 9, 64), bf(1, 1, 1, 64), 64, 64, f(64), f(64).cpu())
    with one:
        ops.conv3x3_halo(bf(1, 1, 1, 64), bf(128, 9, 64), bf(1, 1, 1, 64), 64, 64, f(64), f(64), bf(1, 1, 1, 64).cpu())

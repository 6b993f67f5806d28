"""fp64 oracles, bounds, launch mirrors and mutants of tests/test_enc_conv_edges_gpu.py (CPU only).

Everything here is plain PyTorch in float64 on the CPU (``F.conv2d``,
``torch.nn.grad.conv2d_input`` / ``conv2d_weight``): no fused code path.  The
oracles take the values the kernels read, i.e. after rounding to the storage
dtype (bf16 activations and bf16 packed weights for the MFMA kernels, bf16 or
fp32 activations with FP32 weights for sconv, the fp32 image for the fp32 stem),
in NHWC as the kernels see them, and return NHWC (weight gradients in the
parameter layout (Cout, Cin, KH, KW)) together with the magnitude term of the
bound: A = conv(|x|, |w|) (+ |bias|), conv^T(|dy|, |w|), S = wgrad(|x|, |dy|).

The chain counts are in units of 2^-24 (U): an fp32 FMA / add rounds to nearest
(1 U); an MFMA step is counted 2 U (2^-23), its internal rounding not being
known to be to nearest.  tests/test_enc_conv_oracles_cpu.py ties the oracles to
autograd, the launch mirrors to the numbers in the kernel files, and checks
that the bounds admit a plain fp32 evaluation and reject the mutants below.
"""
import functools
import math

import torch
import torch.nn.functional as F
from torch.nn.grad import conv2d_input, conv2d_weight

F32, BF16, F64 = torch.float32, torch.bfloat16, torch.float64
U = 2.0 ** -24
MFMA = 2  # U per MFMA step


def cdiv(a, b):
    return -(-a // b)


def gen(*key):
    seed = 0
    for k in key:
        seed = (seed * 1000003 + int(k) + 17) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(seed)


def act(shape, dtype, g, scale=1.0):
    """randn activations as stored (rounded to ``dtype``)."""
    return (scale * torch.randn(*shape, generator=g)).to(dtype)


def weight(cout, cin, k, g, kw=None):
    """fp32 conv weight (Cout, Cin, k, kw or k), unit output variance for unit inputs."""
    kw = k if kw is None else kw
    return torch.randn(cout, cin, k, kw, generator=g) * (cin * k * kw) ** -0.5


def rb(t):
    """The bf16 value a packed weight / a bf16 activation holds, as fp32."""
    return t.to(BF16).to(F32)


def split_bf16(x):
    hi = x.to(BF16).to(F32)
    lo = (x - hi).to(BF16).to(F32)
    return hi, lo


def nchw(t):
    return t.double().permute(0, 3, 1, 2)


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def out_hw(h, w, k, s, p):
    return (h + 2 * p - k) // s + 1, (w + 2 * p - k) // s + 1


# ------------------------------------------------------------------ oracles
def conv_fwd(x, w, bias=None, stride=1, pad=0):
    """(want, A) NHWC fp64: conv(x, w) + bias and conv(|x|, |w|) + |bias|."""
    xd, wd = nchw(x), w.double()
    b = None if bias is None else bias.double()
    want = F.conv2d(xd, wd, b, stride, pad)
    A = F.conv2d(xd.abs(), wd.abs(), None if b is None else b.abs(), stride, pad)
    return nhwc(want), nhwc(A)


def conv_dgrad(dy, w, in_hw, stride, pad):
    """(dx, T) NHWC fp64: the input gradient and conv^T(|dy|, |w|)."""
    size = (dy.shape[0], w.shape[1], in_hw[0], in_hw[1])
    gd, wd = nchw(dy), w.double()
    dx = conv2d_input(size, wd, gd, stride, pad)
    T = conv2d_input(size, wd.abs(), gd.abs(), stride, pad)
    return nhwc(dx), nhwc(T)


def conv_wgrad(x, dy, k, stride, pad):
    """(dw, S, db, Sb): dw (Cout, Cin, k, k) fp64 with S = wgrad(|x|, |dy|); db = sum_p dy."""
    xd, gd = nchw(x), nchw(dy)
    size = (dy.shape[3], x.shape[3], k, k)
    dw = conv2d_weight(xd, size, gd, stride, pad)
    S = conv2d_weight(xd.abs(), size, gd.abs(), stride, pad)
    return dw, S, gd.sum((0, 2, 3)), gd.abs().sum((0, 2, 3))


def epilogue(acc, acc_bound, scale=None, shift=None, relu=False, res=None, res_relu=True):
    """The MFMA kernels' epilogue on an accumulator ``acc`` known to ``acc_bound``:
    v = acc * scale + shift (two roundings unless fused), [relu], then
    [relu](v + res) (one rounding).  ReLU is 1-Lipschitz.  -> (want, bound)."""
    want, bound = acc, acc_bound
    if scale is not None:
        sc, sh = scale.double(), shift.double()
        v = want * sc + sh
        bound = sc.abs() * bound + U * ((want * sc).abs() + v.abs())
        want = v
    if relu:
        want = want.clamp_min(0.0)
    if res is not None:
        v = want + res.double()
        bound = bound + U * v.abs()
        want = v.clamp_min(0.0) if res_relu else v
    return want, bound


# ------------------------------------------------------------------ phase-split input gradient
def phase_taps(k, s, p, r):
    """ops/enc_conv.py _phase_taps: taps k' (ascending dY offset d) feeding input phase r."""
    return sorted(((r + p - kk) // s, kk) for kk in range(k) if (r + p - kk) % s == 0)


def phase_dgrad(dy, w, in_hw, stride, pad, descending=False, unmasked_tail=False):
    """What ops/enc_conv.py _conv_geo_dgrad assembles from conv_geo calls, in fp64:
    input phase (ry, rx) = a dense stride-1 conv of dY with the sub-kernel of
    _phase_taps, tap i reading dY at offset d_i (zero outside the dY grid),
    written to every stride-th input pixel; phases without taps stay zero.

    Mutants: ``descending`` pairs the offsets with the taps in descending order
    (a phase weight packed back to front); ``unmasked_tail`` reads the dY row one
    past the grid from the memory that follows it (the next image's first row,
    zeros after the last image) instead of masking it."""
    N, Ho, Wo, cout = dy.shape
    cin, kh, kw = w.shape[1], w.shape[2], w.shape[3]
    Hi, Wi = in_hw
    gd, wd = dy.double(), w.double()
    flat = torch.cat([gd.reshape(N * Ho, Wo, cout), torch.zeros(1, Wo, cout, dtype=F64)])
    dx = torch.zeros(N, Hi, Wi, cin, dtype=F64)
    wrote = torch.zeros(N, Hi, Wi, dtype=torch.long)
    for ry in range(stride):
        for rx in range(stride):
            ty, tx = phase_taps(kh, stride, pad, ry), phase_taps(kw, stride, pad, rx)
            mh, mw = cdiv(Hi - ry, stride), cdiv(Wi - rx, stride)
            if not ty or not tx or mh <= 0 or mw <= 0:
                continue
            ky_of = [k for _, k in ty][::-1] if descending else [k for _, k in ty]
            kx_of = [k for _, k in tx][::-1] if descending else [k for _, k in tx]
            out = torch.zeros(N, mh, mw, cin, dtype=F64)
            for i, (d_y, _) in enumerate(ty):
                for j, (d_x, _) in enumerate(tx):
                    wt = wd[:, :, ky_of[i], kx_of[j]]  # (cout, cin)
                    for y in range(mh):
                        yy = y + d_y
                        tail = unmasked_tail and yy == Ho
                        if not (0 <= yy < Ho or tail):
                            continue
                        x0, x1 = max(0, -d_x), min(mw, Wo - d_x)
                        if x1 <= x0:
                            continue
                        if tail:
                            rows = flat[torch.arange(N) * Ho + yy]
                        else:
                            rows = gd[:, yy]
                        out[:, y, x0:x1] += rows[:, x0 + d_x:x1 + d_x] @ wt
            dx[:, ry::stride, rx::stride] = out
            wrote[:, ry::stride, rx::stride] += 1
    return dx, wrote


# ------------------------------------------------------------------ launch mirrors (from the kernel files)
def halo_tiles(B, H, W, cin, cout):
    """csrc/enc_halo.hip enc_halo_launch: (tiles, tiles per block): 8 x 32 tiles, 4
    consecutive tiles per block, 12 from 1024 tile-blocks on."""
    ntiles = B * cdiv(H, 8) * cdiv(W, 32)
    gy = cdiv(cout, 64 if cin == 64 else 32)
    return ntiles, (12 if ntiles * gy >= 1024 else 4)


def halo_chain(cin):
    """9 taps x cin / 16 MFMA steps into one accumulator."""
    return MFMA * 9 * (cin // 16)


def geo_chain(taps, ktot):
    """csrc/conv.hip conv_lds_kernel: taps x K / 32 MFMA steps (a 64-deep step is two)."""
    return MFMA * taps * (ktot // 32)


def stem_chain(f32):
    """csrc/stem.hip stem_fwd_kernel: 7 kernel rows, one MFMA each (three for the split fp32 form)."""
    return MFMA * 7 * (3 if f32 else 1)


def stem_wgrad_blocks(B, Ho, Wo):
    """csrc/stem.hip stem_wgrad_blocks: (blocks, 64-pixel row chunks per block)."""
    nchunk = B * Ho * cdiv(Wo, 64)
    per = max(1, cdiv(nchunk, 512))
    return cdiv(nchunk, per), per


def stem_wgrad_chain(B, Ho, Wo):
    """4 MFMA steps per chunk, then lane j adds blocks j, j + 16, ..., then 16 lane sums."""
    nblk, per = stem_wgrad_blocks(B, Ho, Wo)
    return MFMA * 4 * per + cdiv(nblk, 16) + 16


def enc_wgrad_splits(B, H, W, cin, cout):
    """csrc/enc_wgrad.hip enc_wgrad_splits: (splits, tiles per block)."""
    ntiles = B * cdiv(H, 8) * cdiv(W, 32)
    want = max(1, 256 // (cdiv(cout, 64) * cdiv(cin, 64)))
    tpb = cdiv(ntiles, want)
    return cdiv(ntiles, tpb), tpb


def enc_wgrad_chain(B, H, W, cin, cout):
    """8 MFMA steps (tile rows) per tile, then four slices of ceil(splits / 4) adds and 3 adds."""
    nsplit, tpb = enc_wgrad_splits(B, H, W, cin, cout)
    return MFMA * 8 * tpb + cdiv(nsplit, 4) + 3


def wgrad_plan(P, taps, ktot, cout, det):
    """csrc/conv_wgrad.hip wgrad_plan, tile variant 0: (K splits, pixels per split)."""
    bm = 64 if cout <= 64 else 128
    ntiles, mtiles = taps * (ktot // 64), cdiv(cout, bm)
    ksplit = max(1, min(cdiv(1024, ntiles * mtiles), cdiv(P, 64 * 8)))
    if det:
        ksplit = min(ksplit, 32)
    kchunk = cdiv(cdiv(P, ksplit), 64) * 64
    return cdiv(P, kchunk), kchunk


def wgrad_chain(P, taps, ktot, cout, det):
    """Two MFMA steps per 64-pixel K step of a split, then one add per split (atomics
    or the ordered reduction) and the add onto dw."""
    ksplit, kchunk = wgrad_plan(P, taps, ktot, cout, det)
    return MFMA * 2 * (kchunk // 64) + ksplit + 1


def wgrad_bias_chain(P, taps, ktot, cout, det):
    """db: a thread adds 2 (64-row M tile) or 4 (128) staged rows per K step, 32 / 16
    threads share a column, then the splits."""
    ksplit, kchunk = wgrad_plan(P, taps, ktot, cout, det)
    per, share = (2, 32) if cout <= 64 else (4, 16)
    return per * (kchunk // 64) + share + ksplit + 1


def sconv_chain(k, cin):
    """csrc/sconv.hip: even / odd input channels in two FMA chains of K / 2, their sum,
    the bias and the residual add."""
    return k * k * cin // 2 + 3


def sconv_wgrad_blocks(B, Ho, OUT):
    """csrc/sconv_train.hip sconv_wgrad_blocks: (blocks, output rows per block)."""
    nrows = B * Ho
    nblk = max(1, min(nrows, 1024, (4 << 20) // max(1, OUT)))
    per = cdiv(nrows, nblk)
    return cdiv(nrows, per), per


def sconv_wgrad_lanes(cin, cout, k):
    """(thread groups, pixel sub-lanes, CO): CO = 8 when Cout % 8 == 0, else 4."""
    co = 8 if cout % 8 == 0 else 4
    ng = (cout // co) * k * k * (cin // 8)
    NG = min(ng, 256)
    return ng, 256 // NG, co


def sconv_wgrad_chain(B, Ho, Wo, cin, cout, k):
    """A sub-lane's FMAs over its pixels of the block's rows, the sub-lanes added in
    order, then the block reduction (lane j adds blocks j, j + 16, ...; 16 lane sums)."""
    nblk, per = sconv_wgrad_blocks(B, Ho, cout * k * k * cin)
    _, SL, _ = sconv_wgrad_lanes(cin, cout, k)
    return per * cdiv(Wo, SL) + SL + cdiv(nblk, 16) + 16


# ------------------------------------------------------------------ bounds
def acc_bound(chain, mag):
    return chain * U * mag


def split_bound(mag):
    """fp32 operands as bf16 hi + lo with the lo * lo product dropped: x = hi + lo + d
    with |lo| ~ 2^-9 |x| and |d| ~ 2^-18 |x| per operand -> 3 * 2^-18 of the magnitude,
    as flow_encode's bound (the worst case, a value just above a power of two, is 4x
    that: see stem_case)."""
    return 3.0 * 2.0 ** -18 * mag


def geo_fwd_bound(A, taps, cin, bias):
    """conv_geo forward: the MFMA chain, and one more rounding for the bias add."""
    return acc_bound(geo_chain(taps, cin) + (1 if bias else 0), A)


def geo_dgrad_chain(k, cout):
    """Phase-split input gradient: the 2 x 2 sub-kernel of phase (1, 1) of a 3x3/s2 conv
    is the longest chain (the pair's (0, 0) phase: 1 tap x 2 cout); one tap for 1x1."""
    return geo_chain(4 if k == 3 else 1, cout)


def stem_bound(A, f32, bias):
    """stem_conv's accumulator (+ bias): the split allotment in fp32, the MFMA chain,
    one rounding for the bias add."""
    b = acc_bound(stem_chain(f32) + (1 if bias else 0), A)
    return b + split_bound(A) if f32 else b


def ratio(got, want, bound, dtype=None):
    """max over ALL elements of err / bound (0 / 0 counts as 0), with the bf16 storage term."""
    if dtype == BF16:
        bound = bound + 2.0 ** -8 * want.abs()
    err = (got.double() - want).abs()
    r = torch.where(err == 0, torch.zeros_like(err), err / bound)
    return r.max().item() if r.numel() else 0.0


def touched_ratio(mut, want, bound, dtype=None):
    """(max, median) of err / bound over the elements a mutant changes; None if it changes none."""
    if dtype == BF16:
        bound = bound + 2.0 ** -8 * want.abs()
    err = (mut - want).abs()
    m = err > 0
    if not bool(m.any()):
        return None
    r = err[m] / bound[m]
    return r.max().item(), r.median().item()


# ------------------------------------------------------------------ mutants
def mutant_drop_border_tap(x, w, stride, pad):
    """(a) one tap of the centre kernel row dropped at the last output column: the
    border tap kx = 0 where its input column lies inside the image, else (a single
    output column of a padded conv) the centre tap, which always does."""
    want, _ = conv_fwd(x, w, None, stride, pad)
    ix = (want.shape[2] - 1) * stride - pad  # input column of tap kx = 0 at the last output column
    kx = 0 if 0 <= ix < x.shape[2] else pad
    one = torch.zeros_like(w)
    one[:, :, pad, kx] = w[:, :, pad, kx]
    tap, _ = conv_fwd(x, one, None, stride, pad)
    mut = want.clone()
    mut[:, :, -1] -= tap[:, :, -1]
    return mut


def mutant_stale_halo(want, B, H, W):
    """(b) the second 8 x 32 tile of the first block computed from the first tile's
    halo: its outputs are those of the first tile (zeros where that tile has none)."""
    th, tw = cdiv(H, 8), cdiv(W, 32)
    if B * th * tw < 2:
        return None
    tiles = [(b, y, x) for b in range(B) for y in range(th) for x in range(tw)]
    (b0, y0, x0), (b1, y1, x1) = tiles[0], tiles[1]
    mut = want.clone()
    for r in range(8):
        for c in range(32):
            oy, ox = y1 * 8 + r, x1 * 32 + c
            if oy < H and ox < W:
                sy, sx = y0 * 8 + r, x0 * 32 + c
                mut[b1, oy, ox] = want[b0, sy, sx] if (sy < H and sx < W) else 0.0
    return mut


def mutant_drop_last_pixel(x, dy, k, stride, pad):
    """(e) the last pixel of the last image left out of a weight gradient."""
    g = dy.clone()
    g[-1, -1, -1] = 0
    return conv_wgrad(x, g, k, stride, pad)[0]


def stem_products(x, w, products):
    """The fp32 stem's split products in exact arithmetic: x and w as bf16 hi + lo,
    ``products`` of {"hh", "hl", "lh"} (weight part, image part) summed.  NHWC fp64."""
    xh, xl = split_bf16(x.float())
    wh, wl = split_bf16(w.float())
    out = 0.0
    for name, (a, b) in {"hh": (wh, xh), "hl": (wh, xl), "lh": (wl, xh)}.items():
        if name in products:
            out = out + F.conv2d(nchw(b), a.double(), None, 2, 3)
    return nhwc(out)


# ------------------------------------------------------------------ cases
# (cin, cout) x (B, H, W) of conv3x3_halo; the last shape runs 12 tiles per block
# (343 one-pixel images x 3 channel blocks = 1029 tile-blocks; 343 = 28 * 12 + 7)
HALO_CH = [(64, 64), (64, 128), (96, 96), (96, 32)]
HALO_SHAPES = [(1, 1, 1), (1, 1, 33), (2, 9, 1), (1, 8, 32), (1, 9, 33), (3, 9, 65)]
HALO_LONG = (343, 1, 1, 96, 96)

ENC_WGRAD_SHAPES = [(1, 1, 1), (1, 8, 32), (1, 9, 33), (2, 1, 70), (2, 17, 1), (3, 9, 65)]
ENC_WGRAD_CH = [(64, 64), (96, 96), (64, 160), (128, 96)]

STEM_HW = [(1, 1), (2, 2), (7, 7), (8, 8), (5, 127), (5, 129), (6, 130)]
STEM_COUT = [8, 32, 64]
# 2 x 129 x 2 = 516 row chunks > 512: two chunks per block, blocks crossing rows and images
STEM_WGRAD_LONG = (2, 257, 129)

GEO_KSP = [(3, 2, 1), (1, 2, 0), (1, 1, 0)]  # (k, stride, pad)
GEO_CH = [(64, 96), (96, 128), (128, 256), (64, 64)]
GEO_HW = [(1, 1), (2, 2), (3, 3), (1, 7), (8, 1), (5, 6), (6, 5), (16, 24)]
GEO_WGRAD_CIN = [64, 96, 128, 160]

SCONV_CH = [(8, 8), (16, 24), (32, 40), (96, 32), (24, 96)]
# B * Ho * Wo = 1, 63, 64, 65 with H = 1 and W = 1 among them; stride 2 from odd and even inputs
SCONV_SHAPES = {1: [(1, 1, 1), (3, 21, 1), (2, 1, 32), (1, 5, 13)],
                2: [(1, 1, 1), (1, 2, 2), (1, 1, 125), (3, 42, 1), (2, 1, 64), (1, 9, 25), (1, 10, 26)]}


# sconv_wgrad: the same channels and kernels (no LDS limit there: 96 -> 32 3x3 has 432
# thread groups), and 16 -> 12 for the CO = 4 thread tile (Cout % 8 != 0)
SWG_CH = [(ci, co, k) for ci, co in SCONV_CH for k in (1, 3)] + [(16, 12, 3)]


def swg_shapes(s):
    """sconv's shapes and one with several output rows per block (sconv_wgrad_blocks)."""
    return SCONV_SHAPES[s] + ([(3, 70, 3)] if s == 1 else [(3, 140, 5)])


def wrapper_chain(c):
    """enc_conv.conv3x3 forward / input gradient: 9 taps x K / 16 MFMA steps with K = c
    (128 for 96: two 64-channel windows) on the v3 tiles; the halo kernel's and the
    implicit GEMM's chains are no longer."""
    return MFMA * 9 * ((c if c % 64 == 0 else 128) // 16)


WRAPPER_CH = [(64, 64), (96, 96), (128, 128), (64, 96)]
WRAPPER_SHAPES = [(1, 1, 1), (1, 9, 33)]


def sconv_fits(cin, cout, k):
    """The host's LDS limit: min(4, Cout / 8) * 8 * k * k * Cin fp32 weights <= 16384."""
    return min(4, cout // 8) * 8 * k * k * cin <= 16384


def sconv_pixels(B, H, W, k, s):
    ho, wo = out_hw(H, W, k, s, k // 2)
    return B * ho * wo


assert sorted({sconv_pixels(*sh, 3, 1) for sh in SCONV_SHAPES[1]}) == [1, 63, 64, 65]
assert sorted({sconv_pixels(*sh, k, 2) for sh in SCONV_SHAPES[2] for k in (1, 3)}) == [1, 63, 64, 65]
assert math.isclose(U, 5.9604644775390625e-08)


# ------------------------------------------------------------------ seeded case builders (shared, never modified)

@functools.lru_cache(maxsize=None)
def fwd_case(B, H, W, cin, cout, k, s, p, dtype=BF16, round_w=True, bias=False):
    """x (NHWC, ``dtype``), w (fp32; the bf16 values a packed weight holds when
    ``round_w``), bias (fp32 or None), want, A."""
    g = gen(B, H, W, cin, cout, k, s, 1)
    x = act((B, H, W, cin), dtype, g)
    w = weight(cout, cin, k, g)
    w = rb(w) if round_w else w
    b = torch.randn(cout, generator=g) if bias else None
    want, A = conv_fwd(x, w, b, s, p)
    return x, w, b, want, A


@functools.lru_cache(maxsize=None)
def bwd_case(B, H, W, cin, cout, k, s, p, dtype=BF16):
    """x and dy (NHWC, ``dtype``) of a conv's backward; dy on the output grid."""
    g = gen(B, H, W, cin, cout, k, s, 2)
    ho, wo = out_hw(H, W, k, s, p)
    x = act((B, H, W, cin), dtype, g)
    dy = act((B, ho, wo, cout), dtype, g)
    return x, dy


@functools.lru_cache(maxsize=None)
def wgrad_case(B, H, W, cin, cout, k, s, p, dtype=BF16):
    x, dy = bwd_case(B, H, W, cin, cout, k, s, p, dtype)
    return (x, dy) + conv_wgrad(x, dy, k, s, p)


@functools.lru_cache(maxsize=None)
def stem_case(B, H, W, cout, dtype):
    """image (NHWC, 3 channels, ``dtype``) and the fp32 7x7 weight.

    The seed is chosen: split_bound's 3 * 2^-18 is no worst case (bf16 rounds to
    within 2^-8 of a value just above a power of two, not 2^-9, so the dropped and
    rounded terms can reach 3 * 2^-16), and at a 1 x 1 image (3 to 27 products, no
    averaging) the exact three-product sum of about every second random draw
    exceeds it.  tests/test_enc_conv_oracles_cpu.py asserts that these inputs
    stay inside the allotment (0.86 of it at the worst case)."""
    g = gen(B, H, W, cout, 70)
    return act((B, H, W, 3), dtype, g), weight(cout, 3, 7, g)


@functools.lru_cache(maxsize=None)
def sconv_case(B, H, W, cin, cout, k, s, dtype):
    """x (``dtype``), the fp32 weight as it is (not rounded), bias, want, A of an
    sconv case, with one cancelling output planted: bias[0] is minus the fp32 value
    of channel 0's sum at the first pixel, so that output is ~2^-25 of its terms.
    There the bf16 storage term vanishes and only the accumulation bound is left:
    at every shape, one-pixel ones included, the output tells fp32 weights from
    bf16-rounded ones (mutant (f)), in bf16 as in fp32."""
    p = k // 2
    x, w, b, _, _ = fwd_case(B, H, W, cin, cout, k, s, p, dtype, round_w=False, bias=True)
    acc, _ = conv_fwd(x, w, None, s, p)
    b = b.clone()
    b[0] = -acc[0, 0, 0, 0].float()
    want, A = conv_fwd(x, w, b, s, p)
    return x, w, b, want, A


@functools.lru_cache(maxsize=None)
def epi_case(B, H, W, cout, *key):
    """Per-channel scale (both signs) and shift, a bf16 residual and a bf16 y0 to accumulate onto."""
    g = gen(B, H, W, cout, 5, *key)
    scale = (0.5 + torch.rand(cout, generator=g)) * torch.where(torch.arange(cout) % 3 == 0, -1.0, 1.0)
    shift = torch.randn(cout, generator=g)
    return scale, shift, act((B, H, W, cout), BF16, g), act((B, H, W, cout), BF16, g)

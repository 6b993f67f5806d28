"""fp64 oracles, bounds, launch mirrors and mutants of tests/test_f32_conv_edges_gpu.py (CPU only).

The fp32 convolution family: every fp32 conv runs on the bf16 MFMAs by operand splitting,
x = xh + xl, w = wh + wl (hi = rne_bf16(v), lo = rne_bf16(v - hi): split8 of conv_common.h,
ops/conv.py split_weight, the in-place LDS split of conv_v3f.hip, csrc/split.hip), and
x.w ~= xh.wh + xl.wh + xh.wl.  Covered: the F32 instantiation of conv_lds_kernel
(csrc/conv.hip, tiles 6 / 7 / 8 and the intra-block split-K tiles 38 / 39 / 40), its GEO
form behind conv_geo, the weight-streaming tiles 81-85 of csrc/conv_v3f.hip, the fp32
epilogues of conv_common.h, and the three-call weight gradients dYh.Xh + dYl.Xh + dYh.Xl
of models/fused_train.py _conv_wgrad and ops/enc_conv.py _f32_wgrad.

Two oracles per convolution, both float64 on the CPU:

product oracle   the exact sum of the three products on the split values.  What is left for
                 the kernel is the fp32 accumulation alone: bound c U A3 with U = 2^-24, A3 the
                 sum of the three products' absolute values (+ |bias|), c the longest chain of
                 dependent roundings read off the kernel (an MFMA step counts 2 U as in
                 enc_conv_cases.py).  This is the bound a wrong product cannot meet.
value oracle     the plain fp64 convolution of the fp32 values; bound = product bound + split
                 bound.  The split bound, derived (SPLIT below): bf16 keeps 8 significand bits, so
                 rounding to nearest moves a value by at most half an ulp, 2^-8 |v| (reached just
                 above a power of two).  With xh = rne(x): |x - xh| <= 2^-8 |x|; x - xh is exact in
                 fp32 (it needs at most 16 of x's 24 bits), xl = rne(x - xh) and the remainder
                 dx = x - xh - xl has |dx| <= 2^-8 |x - xh| <= 2^-16 |x|, |xl| <= 2^-8 |x| (rounding
                 cannot pass the power of two 2^-8 2^e).  The same holds for w.  Writing
                 X = xh + xl, Y = wh + wl:  x w = X Y + dx Y + X dw + dx dw  and
                 X Y = xh wh + xl wh + xh wl + xl wl, so what the three products leave out is
                 xl wl + dx Y + X dw + dx dw, in magnitude at most
                 (2^-16 + 2^-16 (1 + 2^-16) + 2^-16 (1 + 2^-16) + 2^-32) |x| |w|
                 = (3 2^-16 + 3 2^-32) |x| |w|.  Summed over the taps and channels:
                 SPLIT A with A = conv(|x|, |w|) (the bias is not split).

tests/test_f32_conv_oracles_cpu.py ties the oracles to autograd, the launch mirrors to the
kernel files and ops/conv.py, and checks that both bounds admit a plain fp32 evaluation of
the three products and that the product bound rejects every mutant below.
"""
import functools
import json
import os

import torch
import torch.nn.functional as F
from torch.nn.grad import conv2d_weight

import enc_conv_cases as E
import update_conv_cases as C
from enc_conv_cases import (BF16, F32, F64, MFMA, U, acc_bound, cdiv, gen, nchw, nhwc, ratio, split_bf16,  # noqa: F401
                            touched_ratio, weight)
from update_conv_cases import (BORDER, COUT_MAX, COUT_PAD, E20, EPI_ACC_F32, EPI_BIAS, EPI_FLOW,  # noqa: F401
                               EPI_GRU_Q, EPI_GRU_QBWD, EPI_GRU_ZR, EPI_RELU, EPI_RELU_BWD, EPI_SCALE, FLAT_SHAPES,
                               FWD_COUTS, K3, KERNELS, PATCH_SHAPES, PLANT, conv_taps, droppable_tap, plant_pixel)

EPI_NORM = 9
SPLIT = 3.0 * 2.0 ** -16 + 3.0 * 2.0 ** -32  # see the module docstring
# just below the bf16 tie 1 + 2^-8: hi = 1, lo = rne(2^-8 - 2^-20) = +2^-8, the largest lo of one sign
XLO = 1.0 + 2.0 ** -8 - 2.0 ** -20
LO_PIXEL = (0, 0, 0)  # its channels all hold XLO
ROW_POS, ROW_LO = 1, 2  # output channels: all-positive weights / weights all XLO 2^-5

# ------------------------------------------------------------------ launch mirrors: tile -> geometry
# csrc/conv.hip conv_launch RS_F32(BM, BN, KG): conv_lds_kernel<BM, BN, 2, 2, 64, false, true, KG>
REG_TILES = {6: (64, 64, 1), 7: (128, 64, 1), 8: (128, 128, 1), 38: (64, 64, 4), 39: (128, 64, 2), 40: (64, 64, 2)}
# csrc/conv_v3f.hip v3f_launch: conv_v3f_kernel<KH, KW, NWM, THW, RA, NWP, SB>: (NWM, THW, NWP, SB)
V3F_TILES = {81: (4, 3, 1, 0), 82: (4, 1, 1, 0), 83: (4, 2, 1, 0), 84: (2, 2, 2, 0), 85: (2, 2, 2, 1)}


def tile_geom(tile):
    """family, bm (output channels per block), px (flat pixel tile) or patch (TH, TW), kstep
    (input channels per staged K step), mk (K depth of one MFMA), kg (intra-block K groups).
    A tile without a mirror raises: a retune that selects a new fp32 tile must extend this."""
    if tile in REG_TILES:
        bm, px, kg = REG_TILES[tile]
        return dict(tile=tile, family="reg", bm=bm, px=px, patch=None, kstep=32, mk=32, kg=kg, ktot=None)
    if tile in V3F_TILES:
        nwm, thw, nwp, sb = V3F_TILES[tile]
        return dict(tile=tile, family="v3f", bm=32 * nwm, px=None, patch=(thw * nwp, 32), kstep=64, mk=16, kg=1,
                    ktot=64 if sb else None)
    raise ValueError(f"no fp32 conv_fused tile {tile}: add its geometry to tests/f32_conv_cases.py")


def tile_accepts(tile, kh, kw, chans, cout):
    """The host checks of ops_conv.cpp conv_impl that bear on an fp32 (tile, kernel, segments) choice."""
    g = tile_geom(tile)
    if any(c % g["kstep"] for c in chans):
        return False
    if g["family"] == "v3f" and (kh, kw) not in K3:
        return False
    if g["ktot"] is not None and sum(chans) != g["ktot"]:
        return False
    return True


def fwd_chain(tile, taps, ktot, bias):
    """Longest chain of dependent roundings of one output, in U.
    Register tiles (conv_lds_kernel<..., F32, KG>): a K step is 32 input channels and three
    16x16x32 MFMAs ((wh, xh), (wh, xl), (wl, xh)) into ONE accumulator; group g of KG runs
    steps g, g + KG, ...: ceil(steps / KG) of them (steps past the end stage zeros: exact);
    group 0 then adds the KG - 1 parked partial tiles in order.
    Tiles 81-85 (conv_v3f_kernel): one accumulator per output over all nchunks * NSL = taps *
    Ktot / 16 slices, three 32x32x16 MFMAs per slice (V3F_GROUP x 3), no split-K.
    + 1 for the bias add of epi_loop_f32 / epi32_f32 (acc * 1 is exact)."""
    g = tile_geom(tile)
    steps = taps * (ktot // g["mk"])
    return 3 * MFMA * cdiv(steps, g["kg"]) + (g["kg"] - 1) + (1 if bias else 0)


def tuned_table_f32():
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "raft_stir_amd",
                        "conv_tuning.json")
    with open(path) as f:
        return {k: int(v) for k, v in json.load(f).get("tiles_f32", {}).items()}


def choose_tile_f32_range():
    """Every id ops/conv.py choose_tile_f32 can return, over a grid that crosses each of its
    thresholds: P 16384, 64-tile counts 256 / 768, Cout 64 / 256, taps 5 / 9, Ktot 64, with
    the weight-streaming tiles and the strided geometry on and off."""
    from raft_stir_amd.ops.conv import choose_tile_f32
    out = set()
    for P in (1, 64, 4096, 16383, 16384, 16385, 49152, 49153, 100000):
        for cout in (32, 64, 65, 128, 255, 256, 257, 512):
            for geo in (False, True):
                for v3f in (False, True):
                    for taps in (1, 5, 9):
                        for ktot in (64, 192):
                            out.add(choose_tile_f32(P, cout, geo=geo, v3f=v3f, taps=taps, ktot=ktot))
    return out


def tiles_under_test():
    """F32_TILES + the split-K tiles + V3F_TILES + the tuned table + choose_tile_f32's range;
    every id must have a geometry mirror (tile_geom raises otherwise)."""
    from raft_stir_amd.ops import conv as oc
    tiles = set(oc.F32_TILES) | {38, 39, 40} | set(oc.V3F_TILES) | set(tuned_table_f32().values()) \
        | choose_tile_f32_range()
    for t in tiles:
        tile_geom(t)
    return sorted(tiles)


# ------------------------------------------------------------------ segment layouts
# (buffer width, window offset, channels read); a window inside a wider buffer is surrounded by NaN
LAYOUTS = dict(C.LAYOUTS)
LAYOUTS.update({"32x1": [(48, 8, 32)], "32+64": [(48, 8, 32), (64, 0, 64)], "64x1": [(80, 8, 64)]})


def layout_ktot(layout):
    return sum(c for _, _, c in LAYOUTS[layout])


def seg_buffers(x, layout):
    """update_conv_cases.seg_buffers over this module's layouts (fp32 buffers for fp32 x)."""
    out, c0 = [], 0
    for width, off, c in LAYOUTS[layout]:
        buf = torch.full((*x.shape[:3], width), float("nan"), dtype=x.dtype)
        buf[..., off:off + c] = x[..., c0:c0 + c]
        out.append((buf, off, c))
        c0 += c
    assert c0 == x.shape[3]
    return out


def pack_spec(layout):
    spec, w0 = [], 0
    for _, _, c in LAYOUTS[layout]:
        spec.append((c, [(w0, c, 0)]))
        w0 += c
    return spec


def shapes_for(tile):
    return PATCH_SHAPES if tile_geom(tile)["patch"] else FLAT_SHAPES + [(1, 1, 1), (2, 9, 1)]


def layout_for(tile, i):
    g = tile_geom(tile)
    if g["ktot"] == 64:
        return "64x1"
    if g["kstep"] == 32:
        return "32x3" if i % 2 == 0 else "64x2"
    return "64x3" if i % 2 == 0 else "64x2"


def couts_for(tile):
    return FWD_COUTS + ([64] if tile in (84, 85) else [])


# the split-K tiles' extra 1x1 cases: Ktot 32 is one step (KG - 1 idle groups), Ktot 96 three
# (uneven over 2 groups, one group of 4 empty)
SPLITK_EXTRA = [("32x1", (1, 3, 43)), ("32+64", (1, 3, 43)), ("32+64", (1, 1, 1))]


# ------------------------------------------------------------------ the three products
TERMS = {"hh": (0, 0), "lh": (1, 0), "hl": (0, 1), "ll": (1, 1)}  # (x part, w part): 0 = hi, 1 = lo
THREE = ("hh", "lh", "hl")


def product3(x, w, bias, kh, kw, stride=1, pad=None, terms=THREE, xl_roll=0):
    """(want, A3) NHWC fp64: the exact sum of the split products ``terms`` (+ bias) and the sum
    of their absolute values (+ |bias|).  ``xl_roll``: the mutant that takes the lo part of the
    activations from the 32-channel chunk ``xl_roll`` chunks further on."""
    xs = list(split_bf16(x.float()))
    ws = split_bf16(w.float())
    if xl_roll:
        xs[1] = xs[1].roll(-32 * xl_roll, -1)
    pad = (kh // 2, kw // 2) if pad is None else pad
    want = A = 0.0
    for t in terms:
        a, b = xs[TERMS[t][0]], ws[TERMS[t][1]].double()
        want = want + F.conv2d(nchw(a), b, None, stride, pad)
        A = A + F.conv2d(nchw(a).abs(), b.abs(), None, stride, pad)
    if bias is not None:
        want = want + bias.double().view(1, -1, 1, 1)
        A = A + bias.double().abs().view(1, -1, 1, 1)
    return nhwc(want), nhwc(A)


def taps3(x, w, kh, kw, **mut):
    """The three products walked tap by tap (update_conv_cases.conv_taps and its wrap / drop mutants)."""
    xh, xl = split_bf16(x.float())
    wh, wl = split_bf16(w.float())
    return conv_taps(xh, wh, kh, kw, **mut) + conv_taps(xl, wh, kh, kw, **mut) + conv_taps(xh, wl, kh, kw, **mut)


def product_bound(chain, A3):
    return acc_bound(chain, A3)


def value_bound(chain, A3, A):
    """Against the fp64 conv of the fp32 values: accumulation + what the split leaves out."""
    return acc_bound(chain, A3) + SPLIT * A


def step_slices(taps, chans):
    """conv.hip RS_GLOAD: K step -> (tap, first channel): segments in order, per segment the
    taps, per tap the 32-channel chunks."""
    out, k0 = [], 0
    for c in chans:
        out += [(tap, k0 + 32 * ch) for tap in range(taps) for ch in range(c // 32)]
        k0 += c
    return out


def stale_steps(nsteps, kg):
    """The steps a split-K group would run twice if, past the end, it re-staged its previous
    step instead of zeros: slot (nst - 1) kg + g >= nsteps of a group that has a step before it."""
    last = (cdiv(nsteps, kg) - 1) * kg
    return [last + g - kg for g in range(kg) if last + g >= nsteps and last + g - kg >= 0]


def mutant_stale_step(x, w, kh, kw, chans, kg):
    """What the stale steps add to the result (None if the step count divides evenly)."""
    sl = step_slices(kh * kw, chans)
    extra = None
    for s in stale_steps(len(sl), kg):
        tap, k0 = sl[s]
        w1 = torch.zeros_like(w)
        w1[:, k0:k0 + 32, tap // kw, tap % kw] = w[:, k0:k0 + 32, tap // kw, tap % kw]
        e = product3(x, w1, None, kh, kw)[0]
        extra = e if extra is None else extra + e
    return extra


def border_scaled(x, scale=BORDER):
    x = x.clone()
    m = torch.zeros(x.shape[1], x.shape[2], dtype=torch.bool)
    m[0, :] = m[-1, :] = True
    m[:, 0] = m[:, -1] = True
    x[:, m] *= scale
    return x


def plant_lo(x, w):
    """Maximal lo parts of one sign: every channel of LO_PIXEL holds XLO (xh = 1, xl = +2^-8)
    next to the all-positive weight row ROW_POS, and row ROW_LO's weights all hold XLO 2^-5."""
    x[LO_PIXEL] = XLO
    w[ROW_POS] = w[ROW_POS].abs()
    w[ROW_LO] = XLO * 2.0 ** -5


@functools.lru_cache(maxsize=None)
def fwd_case(B, H, W, kh, kw, ktot=192):
    """fp32 x (NHWC, border x 64), w (200, ktot, kh, kw), bias; both oracles.  Planted: the lo
    pixel and rows of plant_lo, and bias[0] so that channel 0 at plant_pixel cancels to 2^-20
    of its magnitude term."""
    g = gen(B, H, W, kh, kw, ktot, 71)
    x = border_scaled(torch.randn(B, H, W, ktot, generator=g))
    w = weight(COUT_MAX, ktot, kh, g, kw)
    plant_lo(x, w)
    bias = torch.randn(COUT_MAX, generator=g)
    acc, A0 = product3(x, w, None, kh, kw)
    p = plant_pixel(B, H, W)
    bias[0] = (-acc[p][0] + E20 * A0[p][0]).float()
    want3, A3 = product3(x, w, bias, kh, kw)
    want, Ab = C.conv_fwd(x, w, bias, kh, kw)
    return dict(x=x, w=w, bias=bias, want3=want3, A3=A3, want=want, A=Ab - bias.double().abs())


# ------------------------------------------------------------------ epilogues
EPI_SHAPES = C.EPI_SHAPES
EPI_HD = C.EPI_HD
EPI_COUT = C.EPI_COUT
EPI_TILES = (7, 38, 81, 84)
NORM_KINDS = [(False, False), (True, False), (True, True)]  # (relu, residual)


@functools.lru_cache(maxsize=None)
def epi_case(B, H, W, kh, kw):
    """update_conv_cases.epi_case in fp32: x, w (128 rows: z | r), bias and fp32 aux tensors.
    Channels 0..10 and 64..74 have zero weight rows and the PLANT values as bias; z / r hold
    exact 0 and 1; the ReLU output holds 0.0, -0.0, the smallest normal fp32 of both signs and
    -1; o0 prefills the accumulating outputs; nscale (both signs) / nshift / res feed EPI_NORM.
    pre / A3 (with bias) and pre0 / A30 (without) are the product oracle of the conv."""
    g = gen(B, H, W, kh, kw, 73)
    x = torch.randn(B, H, W, C.KTOT, generator=g)
    w = weight(EPI_COUT, C.KTOT, kh, g, kw)
    bias = 0.1 * torch.randn(EPI_COUT, generator=g)
    for base in (0, EPI_HD):
        for i, v in enumerate(PLANT):
            w[base + i] = 0
            bias[base + i] = v
    pre, A3 = product3(x, w, bias, kh, kw)
    pre0, A30 = product3(x, w, None, kh, kw)
    shp = (B, H, W, EPI_COUT)
    h = torch.tanh(torch.randn(*shp, generator=g))
    z = torch.sigmoid(3.0 * torch.randn(*shp, generator=g))
    z[..., 3], z[..., 4] = 0.0, 1.0
    actv = torch.randn(*shp, generator=g)
    tiny = torch.finfo(F32).tiny
    for i, v in enumerate((0.0, -0.0, tiny, -tiny, -1.0)):
        actv[..., i::16] = v
    o0 = torch.randn(*shp, generator=g)
    nscale = (0.5 + torch.rand(EPI_COUT, generator=g)) * torch.where(torch.arange(EPI_COUT) % 3 == 0, -1.0, 1.0)
    nshift = torch.randn(EPI_COUT, generator=g)
    res = torch.randn(*shp, generator=g)
    return dict(x=x, w=w, bias=bias, pre=pre, A3=A3, pre0=pre0, A30=A30, h=h, z=z, actv=actv, o0=o0,
                nscale=nscale, nshift=nshift, res=res)


def epi_norm(pre0, pb0, scale, shift, relu, res):
    """EPI_NORM: [relu](acc * nscale + shift), then relu(. + res): enc_conv_cases.epilogue."""
    return E.epilogue(pre0, pb0, scale, shift, relu, res)


# ------------------------------------------------------------------ conv_geo (fp32) and the input gradients
GEO_KSP = E.GEO_KSP
GEO_HW = E.GEO_HW
GEO_CH = [(64, 96), (96, 128)]
GEO_B = 2
DGRAD_S1_SHAPES = [(1, 1, 1), (2, 9, 1), (1, 9, 33), (3, 5, 13)]
DGRAD_S1_CH = [(64, 64), (64, 96), (96, 128), (128, 64)]


def geo_chain(taps, ktot, bias):
    """conv_lds_kernel<..., GEO, F32> (tiles 6 / 7 / 8, one K group): three MFMAs per 32-channel step."""
    return 3 * MFMA * taps * (ktot // 32) + (1 if bias else 0)


def geo_dgrad_chain(k, cout):
    """The phase with the most taps of the phase-split input gradient: 2 x 2 for 3x3 / s2, one for 1x1."""
    return geo_chain(4 if k == 3 else 1, cout, False)


@functools.lru_cache(maxsize=None)
def geo_case(B, H, W, cin, cout, k, s, p):
    """fp32 x, w, bias of a strided / 1x1 conv with the lo plants; both oracles."""
    g = gen(B, H, W, cin, cout, k, s, 79)
    x = torch.randn(B, H, W, cin, generator=g)
    w = weight(cout, cin, k, g)
    plant_lo(x, w)
    bias = torch.randn(cout, generator=g)
    want3, A3 = product3(x, w, bias, k, k, s, p)
    want, Ab = E.conv_fwd(x, w, bias, s, p)
    return dict(x=x, w=w, bias=bias, want3=want3, A3=A3, want=want, A=Ab - bias.double().abs())


def dgrad3(dy, w, in_hw, stride, pad, terms=THREE):
    """(dx, T3): the three split products of the input gradient (dy takes the activation's part)."""
    dys, ws = split_bf16(dy.float()), split_bf16(w.float())
    dx = T = 0.0
    for t in terms:
        a, b = E.conv_dgrad(dys[TERMS[t][0]], ws[TERMS[t][1]], in_hw, stride, pad)
        dx, T = dx + a, T + b
    return dx, T


@functools.lru_cache(maxsize=None)
def dgrad_case(B, H, W, cin, cout, k, s, p):
    """fp32 dy (one row of maximal lo) and w (rows of plant_lo) of an input gradient; both oracles."""
    g = gen(B, H, W, cin, cout, k, s, 83)
    ho, wo = E.out_hw(H, W, k, s, p)
    dy = torch.randn(B, ho, wo, cout, generator=g)
    w = weight(cout, cin, k, g)
    plant_lo(dy, w)
    dx3, T3 = dgrad3(dy, w, (H, W), s, p)
    dx, T = E.conv_dgrad(dy, w, (H, W), s, p)
    return dict(dy=dy, w=w, dx3=dx3, T3=T3, dx=dx, T=T)


# ------------------------------------------------------------------ split_bf16
SPLIT_SIZES = [1, 3, 7, 8, 9, 4097]


def split_values(n):
    """n fp32 values: +-0, the largest and smallest normal bf16, fp32 subnormals, exact ties
    between two bf16 (to even: down at 1 + 2^-8, up at 1 + 3 2^-8), values one fp32 ulp off a
    tie, XLO, then randn over 40 binades.  No inf / NaN (split_specials)."""
    fi = torch.finfo(BF16)
    t = torch.tensor([0.0, -0.0, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, fi.max, -fi.tiny, 2.0 ** -149, -fi.max,
                      fi.tiny, -2.0 ** -140, 2.0 ** -127, -(1.0 + 2.0 ** -8), -(1.0 + 3 * 2.0 ** -8),
                      1.0 + 2.0 ** -8 + 2.0 ** -23, 1.0 + 2.0 ** -8 - 2.0 ** -23, XLO, -XLO,
                      3.0e38, 2.0 ** -126 * 1.5], dtype=F32)
    g = gen(n, 89)
    r = torch.randn(n, generator=g) * 2.0 ** torch.randint(-20, 20, (n,), generator=g).float()
    m = min(n, t.numel())
    r[:m] = t[:m]
    if n % 4 and n > 8:  # a tie in the scalar tail of the kernel (n % 4 elements) as well
        r[-1] = 1.0 + 3 * 2.0 ** -8
    return r


def split_oracle(t):
    """(hi, lo) bf16: rne(t) and rne(t - hi), as torch rounds (to nearest even)."""
    hi = t.to(BF16)
    return hi, (t - hi.float()).to(BF16)


def split_specials():
    """+-inf and NaN, and fp32 values that round up to inf in bf16.  By the formula hi = rne(t)
    keeps inf / NaN and lo = rne(t - hi) is NaN for inf (inf - inf) and NaN; a finite value
    above the largest bf16's rounding range gives hi = inf, lo = -inf."""
    big = torch.finfo(F32).max
    return torch.tensor([float("inf"), -float("inf"), float("nan"), big, -big, 1.0, -2.5], dtype=F32)


# ------------------------------------------------------------------ three-product weight gradients
# update block (models/fused_train.py _conv_wgrad): (iterations, B, H, W): 63 / 64 / 65 / 195 pixels
WG_STACKS = [(1, 1, 7, 9), (2, 2, 4, 4), (1, 1, 5, 13), (3, 1, 5, 13)]
assert [i * b * h * w for i, b, h, w in WG_STACKS] == [63, 64, 65, 195]
# (kh, kw, Cout): wgrad_v3 for Cout > 64 with 5 / 9 taps, conv_wgrad for Cout 64 and 1x1
WG_KC = [(3, 3, 200), (1, 5, 70), (5, 1, 126), (3, 3, 64), (1, 1, 200), (1, 1, 64)]
WG_SEG, WG_KTOT, WG_YOFF = C.WG_SEG, C.WG_KTOT, C.WG_YOFF
WG_TERMS = ("hh", "lh", "hl")  # (dy part, x part): dYh.Xh + dYl.Xh + dYh.Xl


def wgrad_route(kh, kw, cout):
    """models/fused_train.py _wgrad_fn: ('v3', bm) or ('wgrad', 0)."""
    if kh * kw in (5, 9) and cout > 64:
        return "v3", (128 if cout >= 512 else 64)
    return "wgrad", 0


def wgrad3(x, dy, kh, kw, stride=1, terms=WG_TERMS, db_terms=("h", "l")):
    """(dw, S3, db, Sb) of the three-call weight gradient in fp64: term 'ab' is wgrad(dy part a,
    x part b); db is the column sum of the dy parts the calls with a bias pointer see."""
    xs, gs = split_bf16(x.float()), split_bf16(dy.float())
    size = (dy.shape[3], x.shape[3], kh, kw)
    pad = (kh // 2, kw // 2)
    dw = S = 0.0
    for t in terms:
        a, b = nchw(gs[TERMS[t][0]]), nchw(xs[TERMS[t][1]])
        dw = dw + conv2d_weight(b, size, a, stride, pad)
        S = S + conv2d_weight(b.abs(), size, a.abs(), stride, pad)
    db = Sb = 0.0
    for t in db_terms:
        a = nchw(gs[0 if t == "h" else 1])
        db, Sb = db + a.sum((0, 2, 3)), Sb + a.abs().sum((0, 2, 3))
    return dw, S, db, Sb


def wgrad_value(x, dy, kh, kw, stride=1):
    """(dw, S, db, Sb): conv2d_weight of the fp32 values in fp64."""
    xd, gd = nchw(x), nchw(dy)
    size = (dy.shape[3], x.shape[3], kh, kw)
    pad = (kh // 2, kw // 2)
    return (conv2d_weight(xd, size, gd, stride, pad), conv2d_weight(xd.abs(), size, gd.abs(), stride, pad),
            gd.sum((0, 2, 3)), gd.abs().sum((0, 2, 3)))


@functools.lru_cache(maxsize=None)
def wgrad_case(iters, B, H, W, kh, kw):
    """fp32 segments x0, xb (broadcast over the iterations; image b holds b + 1 in channel 0),
    x2 and dy (200 channels) of update_conv_cases.wgrad_case, with maximal-lo plants: dy's
    row LO_PIXEL and x0's channel 1 all hold XLO.  Both oracles for Cout = 200."""
    g = gen(iters, B, H, W, kh, kw, 97)
    N = iters * B
    x0 = torch.randn(N, H, W, WG_SEG, generator=g)
    xb = torch.randn(B, H, W, WG_SEG, generator=g)
    for b in range(B):
        xb[b, :, :, 0] = b + 1.0
    x2 = torch.randn(N, H, W, WG_SEG, generator=g)
    dy = torch.randn(N, H, W, COUT_MAX, generator=g)
    dy[LO_PIXEL] = XLO
    x0[..., 1] = XLO
    x = C.stack_x(x0, xb, x2, iters)
    dw3, S3, db3, Sb3 = wgrad3(x, dy, kh, kw)
    dw, S, db, Sb = wgrad_value(x, dy, kh, kw)
    return dict(x0=x0, xb=xb, x2=x2, dy=dy, x=x, dw3=dw3, S3=S3, db3=db3, Sb3=Sb3, dw=dw, S=S, db=db, Sb=Sb)


def wgrad_chains(route, bm, stack, kh, kw, cout, det):
    """(dw chain, db chain) of the THREE calls: each call's own chain (which ends in its add onto
    dw / db: update_conv_cases.wgrad_chain / wgrad3_chain and their bias forms) three times
    for dw, twice for db (the third call has no bias pointer)."""
    it, B, H, W = stack
    P = it * B * H * W
    if route == "v3":
        c, cb = C.wgrad3_chain(it * B, H, W, cout, WG_KTOT, bm), C.wgrad3_bias_chain(it * B, H, W, cout, WG_KTOT, bm)
    else:
        c, cb = (C.wgrad_chain(P, kh * kw, WG_KTOT, cout, det, 0),
                 C.wgrad_bias_chain(P, kh * kw, WG_KTOT, cout, det, 0))
    return 3 * c, 2 * cb


# encoder (ops/enc_conv.py _f32_wgrad): (k, stride, pad) -> route
ENC_WG_KSP = [(3, 1, 1), (3, 2, 1), (1, 1, 0), (1, 2, 0)]
ENC_WG_CH = [(64, 64), (96, 96), (64, 160), (128, 96)]
ENC_WG_SHAPES = {1: E.ENC_WGRAD_SHAPES, 2: [(GEO_B, h, w) for h, w in GEO_HW]}


def enc_wgrad_chain(B, H, W, cin, cout, k, s, p):
    """Three calls, each into its own zeroed accumulator, then dw = f1 + f2 + f3 (two adds).
    3x3 / s1: enc_wgrad (enc_conv_cases.enc_wgrad_chain); the rest: conv_wgrad_strided over
    the dY grid (enc_conv_cases.wgrad_chain, K tile 64; the longer of the atomic and the
    deterministic plan's chains, whichever mode the process is in)."""
    if (k, s) == (3, 1):
        c = E.enc_wgrad_chain(B, H, W, cin, cout)
    else:
        ho, wo = E.out_hw(H, W, k, s, p)
        ktot = cin if cin % 64 == 0 else cin + 32  # two overlapping 64-wide segments for 96
        c = max(E.wgrad_chain(B * ho * wo, k * k, ktot, cout, d) for d in (False, True))
    return 3 * c + 2


@functools.lru_cache(maxsize=None)
def enc_wgrad_case(B, H, W, cin, cout, k, s, p):
    g = gen(B, H, W, cin, cout, k, s, 101)
    ho, wo = E.out_hw(H, W, k, s, p)
    x = torch.randn(B, H, W, cin, generator=g)
    dy = torch.randn(B, ho, wo, cout, generator=g)
    dy[LO_PIXEL] = XLO
    x[..., 1] = XLO
    size = (cout, cin, k, k)
    xs, gs = split_bf16(x), split_bf16(dy)
    dw3 = S3 = 0.0
    for t in WG_TERMS:
        a, b = nchw(gs[TERMS[t][0]]), nchw(xs[TERMS[t][1]])
        dw3 = dw3 + conv2d_weight(b, size, a, s, p)
        S3 = S3 + conv2d_weight(b.abs(), size, a.abs(), s, p)
    dw = conv2d_weight(nchw(x), size, nchw(dy), s, p)
    S = conv2d_weight(nchw(x).abs(), size, nchw(dy).abs(), s, p)
    return dict(x=x, dy=dy, dw3=dw3, S3=S3, dw=dw, S=S, db=nchw(dy).sum((0, 2, 3)), Sb=nchw(dy).abs().sum((0, 2, 3)))

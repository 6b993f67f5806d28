"""fp64 oracles, bounds, launch mirrors and mutants of tests/test_update_conv_edges_gpu.py (CPU only).

The bf16 update-block convolution family behind ``conv_fused`` (csrc/conv.hip,
conv_v2.hip, conv_v3.h, conv_gemm1.hip with the epilogues of conv_common.h), its
weight gradients (csrc/conv_wgrad.hip stride 1, csrc/wgrad_v3.hip) and the
element-wise backward ops gru_gate_bwd / relu_take.  Everything here is plain
PyTorch in float64 on the CPU: ``F.conv2d`` over the concatenated segment
windows, closed forms of every epilogue, ``conv2d_weight`` and a column sum, the
three formulas above gru_gate_bwd_kernel, ``G * (act > 0)``.  The oracles take
the values the kernels read (bf16 activations, the bf16 values of the packed
weight, fp32 bias) and return the magnitude term of the bound with the result.

Units as in enc_conv_cases.py: U = 2^-24 per fp32 FMA / add, 2 U per MFMA step,
2^-8 |want| for a bf16 store.  tests/test_update_conv_oracles_cpu.py ties the
oracles to autograd, the launch mirrors to the kernel files and ops/conv.py, and
checks that the bounds admit a plain fp32 evaluation and reject the mutants.
"""
import functools
import json
import os

import torch
import torch.nn.functional as F
from torch.nn.grad import conv2d_weight

from enc_conv_cases import (BF16, F32, F64, MFMA, U, acc_bound, act, cdiv, gen, nchw, nhwc, ratio, rb,  # noqa: F401
                            touched_ratio, weight)

E20 = 2.0 ** -20
(EPI_BIAS, EPI_RELU, EPI_SCALE, EPI_GRU_ZR, EPI_GRU_Q, EPI_FLOW,
 EPI_RELU_BWD, EPI_ACC_F32, EPI_GRU_QBWD) = range(9)
# tests/test_gates_gpu.py PLANT (asserted equal on the CPU)
PLANT = [0.0, 1e-3, -1e-3, 20.0, -20.0, 88.0, -88.0, 100.0, -100.0, 1e4, -1e4]

KERNELS = [(1, 1), (3, 3), (1, 5), (5, 1)]
K3 = KERNELS[1:]  # conv_v2 / conv_v3 / wgrad_v3


# ------------------------------------------------------------------ launch mirrors: tile -> geometry
def tile_geom(tile):
    """csrc/conv.hip conv_launch, conv_v2.hip conv_v2_launch, conv_v3.h v3_geom, conv_gemm1.hip:
    family, bm (output channels per block), px (flat pixel tile) or patch (TH, TW),
    bk (input channels per staged K step), kg (intra-block K groups), mk (K depth of one MFMA)."""
    g = dict(tile=tile, kg=1, px=None, patch=None, mk=32)
    if tile in (0, 1):  # conv_kernel<WM, 2, 1, 4>: 16 WM channels x 128 pixels, fragments from global
        g.update(family="plain", bm=32 if tile == 0 else 64, px=128, bk=32)
    elif tile == 5:  # conv_smalln_kernel: 16 x 16, the K steps dealt to the 4 waves
        g.update(family="smalln", bm=16, px=16, bk=32, kg=4)
    elif tile in (2, 3, 4, 6, 7, 8, 41):
        bm, px, bk = {2: (64, 128, 32), 3: (64, 64, 32), 4: (128, 64, 32), 6: (64, 64, 64), 7: (128, 64, 64),
                      8: (128, 128, 64), 41: (64, 64, 32)}[tile]
        g.update(family="lds", bm=bm, px=px, bk=bk, kg=4 if tile == 41 else 1)
    elif 9 <= tile <= 15:
        bm, bk = {9: (64, 64), 10: (128, 64), 11: (128, 64), 12: (128, 32), 13: (128, 32), 14: (64, 32),
                  15: (64, 64)}[tile]
        g.update(family="glds", bm=bm, px=64, bk=bk)
    elif 16 <= tile <= 23 or 27 <= tile <= 37:
        bm, px, kg = {16: (128, 64, 1), 17: (64, 64, 1), 18: (128, 64, 1), 19: (64, 64, 1), 20: (128, 128, 1),
                      21: (64, 128, 1), 22: (128, 128, 1), 23: (64, 64, 1), 27: (256, 96, 1), 28: (128, 96, 1),
                      29: (192, 96, 1), 30: (256, 96, 1), 31: (128, 96, 1), 32: (256, 192, 1), 33: (128, 192, 1),
                      34: (64, 64, 2), 35: (64, 64, 2), 36: (128, 64, 2), 37: (64, 64, 4)}[tile]
        g.update(family="buf", bm=bm, px=px, bk=64, kg=kg)
    elif 24 <= tile <= 26:
        g.update(family="halo", bm=64 if tile == 25 else 128, patch=(4 if tile == 26 else 8, 16), bk=64,
                 hcap=128 if tile == 26 else 192)
    elif 42 <= tile <= 54:  # V2<KH, KW, NWM, NWN, S, MW>: BM = 32 NWM MW, patch 2 NWN x 32
        mw = 2 if (48 <= tile <= 52 or tile == 54) else 1
        nwm = 1 if tile == 43 else 3 if tile == 54 else 4 if (tile == 44 or tile >= 50) else 2
        nwn = 4 if tile == 43 else 1 if tile in (44, 50) else 2
        g.update(family="v2", bm=32 * nwm * mw, patch=(2 * nwn, 32), bk=64, mk=16)
    elif tile in (56, 57, 61, 65, 66, 68):  # v3_geom: BM = 32 NWM, patch THW NWP x 32
        nwm, thw, nwp = {56: (4, 1, 1), 57: (4, 2, 1), 61: (4, 3, 1), 65: (2, 3, 1), 66: (4, 3, 2),
                         68: (2, 3, 4)}[tile]
        g.update(family="v3", bm=32 * nwm, patch=(thw * nwp, 32), bk=64, mk=16)
    elif tile == 70:
        g.update(family="gemm1", bm=128, px=128, bk=64, mk=16)
    else:
        raise ValueError(f"no bf16 conv_fused tile {tile}")
    return g


FAMILIES = ("plain", "smalln", "lds", "glds", "buf", "halo", "v2", "v3", "gemm1")
# the first tile of each kernel template (one per family is added when no table entry reaches it)
FAMILY_FIRST = {"plain": 0, "smalln": 5, "lds": 3, "glds": 9, "buf": 17, "halo": 25, "v2": 45, "v3": 56, "gemm1": 70}


def tile_accepts(tile, kh, kw, chans, cout):
    """The host checks of ops_conv.cpp conv_impl that bear on a (tile, kernel, segments, Cout) choice."""
    g = tile_geom(tile)
    if any(c % g["bk"] for c in chans):
        return False
    if g["family"] in ("v2", "v3") and (kh, kw) not in K3:
        return False
    if g["family"] == "gemm1" and (kh, kw) != (1, 1):
        return False
    if tile == 5 and cout > 16:
        return False
    if g["family"] == "halo" and (g["patch"][0] + kh - 1) * (16 + kw - 1) > g["hcap"]:
        return False
    return True


def fwd_chain(tile, taps, ktot, bias):
    """Longest chain of dependent roundings of one output, in U: every kernel keeps ONE
    accumulator per output over the whole K walk, ``taps * ktot / mk`` MFMA steps of depth
    mk (16x16x32 MFMAs: 32, the 32x32x16 of conv_v2 / conv_v3 / conv_gemm1: 16; a 64-deep
    staged step is 2 resp. 4 of them).  With kg K groups (tile 41, 34-37, 5) a group runs
    ceil(steps / kg) staged steps and group 0 adds the kg - 1 partial tiles in order
    (tile 5: the three adds of red[0] + red[1] + red[2] + red[3]).  + 1 for the bias add."""
    g = tile_geom(tile)
    staged = taps * (ktot // g["bk"])
    per_stage = g["bk"] // g["mk"]
    return MFMA * cdiv(staged, g["kg"]) * per_stage + (g["kg"] - 1) + (1 if bias else 0)


def tuned_table():
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "raft_stir_amd",
                        "conv_tuning.json")
    with open(path) as f:
        return {k: int(v) for k, v in json.load(f).get("tiles", {}).items()}


def choose_tile_range():
    """Every id ops/conv.py choose_tile can return, found by running it over a grid that
    crosses each of its thresholds (P 16384, Cout 16 / 64 / 126 / 128 / 192, K 384 / 1024,
    64-blocks 256)."""
    from raft_stir_amd.ops.conv import choose_tile
    out = set()
    for P in (1, 64, 4096, 7480, 16383, 16384, 22816, 100000):
        for cout in (2, 16, 17, 64, 65, 96, 126, 128, 129, 192, 193, 256, 576):
            for chans in ((32,), (96, 160), (64,), (128, 256), (128, 128, 128), (512,)):
                for taps in (1, 5, 9, 49):
                    out.add(choose_tile(P, cout, chans, taps))
    return out


def tiles_under_test():
    """Tuned table + choose_tile's range + one tile of every kernel template not reached by them."""
    tiles = set(tuned_table().values()) | choose_tile_range()
    have = {tile_geom(t)["family"] for t in tiles}
    for fam in FAMILIES:
        if fam not in have:
            tiles.add(FAMILY_FIRST[fam])
    return sorted(tiles)


# ------------------------------------------------------------------ forward cases
PATCH_SHAPES = [(1, 1, 1), (1, 1, 33), (2, 9, 1), (1, 8, 32), (1, 9, 33), (3, 9, 65)]
FLAT_SHAPES = [(1, 1, 63), (1, 1, 64), (1, 1, 65), (2, 8, 8), (1, 3, 43), (3, 5, 13)]
assert [b * h * w for b, h, w in FLAT_SHAPES] == [63, 64, 65, 128, 129, 195]
FWD_COUTS = [70, 96, 200]
SMALLN_COUTS = [2, 12]  # tile 5: Cout <= 16
KTOT = 192
COUT_MAX = 200
COUT_PAD = 384  # >= round_up(200, every block height 16 .. 256), a multiple of 32 (fragment-major rows)
BORDER = 64.0

# (buffer width, window offset, channels read): the same 192 channels in every layout; a
# window inside a wider buffer is surrounded by NaN, so one channel read outside it poisons
# the result
LAYOUTS = {
    "64x2": [(80, 8, 64), (128, 0, 128)],
    "64x3": [(80, 8, 64), (64, 0, 64), (72, 8, 64)],
    "32x3": [(48, 8, 32), (64, 0, 64), (96, 0, 96)],
}


def shapes_for(tile):
    """Patch tiles: the patch shapes; flat-pixel tiles: pixel counts around 64 / 128 (and
    192 = 195 - 3) plus the one-pixel and one-column grids."""
    return PATCH_SHAPES if tile_geom(tile)["patch"] else FLAT_SHAPES + [(1, 1, 1), (2, 9, 1)]


def layout_for(tile, i):
    if tile_geom(tile)["bk"] == 32:
        return "32x3" if i % 2 == 0 else "64x2"
    return "64x3" if i % 2 == 0 else "64x2"


def seg_buffers(x, layout):
    """[(NaN-padded NHWC buffer, offset, channels)] holding x's channels in order."""
    out, c0 = [], 0
    for width, off, c in LAYOUTS[layout]:
        buf = torch.full((*x.shape[:3], width), float("nan"), dtype=x.dtype)
        buf[..., off:off + c] = x[..., c0:c0 + c]
        out.append((buf, off, c))
        c0 += c
    assert c0 == x.shape[3]
    return out


def pack_spec(layout):
    """ops/conv.py pack_weight's segment spec of a layout."""
    spec, w0 = [], 0
    for _, _, c in LAYOUTS[layout]:
        spec.append((c, [(w0, c, 0)]))
        w0 += c
    return spec


def border_scaled(x, scale=BORDER):
    """Border pixels x ``scale`` (exact in bf16) next to the unit-scale interior."""
    x = x.float().clone()
    m = torch.zeros(x.shape[1], x.shape[2], dtype=torch.bool)
    m[0, :] = m[-1, :] = True
    m[:, 0] = m[:, -1] = True
    x[:, m] *= scale
    return x.to(BF16)


def conv_fwd(x, w, bias, kh, kw):
    """(want, A) NHWC fp64 of the stride-1 'same' conv: F.conv2d and conv(|x|, |w|) + |bias|."""
    xd, wd = nchw(x), w.double()
    b = None if bias is None else bias.double()
    pad = (kh // 2, kw // 2)
    want = F.conv2d(xd, wd, b, 1, pad)
    A = F.conv2d(xd.abs(), wd.abs(), None if b is None else b.abs(), 1, pad)
    return nhwc(want), nhwc(A)


def plant_pixel(B, H, W):
    return B - 1, H // 2, W // 2


@functools.lru_cache(maxsize=None)
def fwd_case(B, H, W, kh, kw):
    """x (NHWC bf16, 192 channels, border x 64), w (200, 192, kh, kw) fp32 holding bf16
    values, bias (fp32), want, A.  bias[0] is planted so that channel 0 at plant_pixel
    cancels to 2^-20 of its magnitude term: there the bf16 storage term vanishes and the
    accumulation bound alone is left."""
    g = gen(B, H, W, kh, kw, 31)
    x = border_scaled(act((B, H, W, KTOT), BF16, g))
    w = rb(weight(COUT_MAX, KTOT, kh, g, kw))
    bias = torch.randn(COUT_MAX, generator=g)
    acc, A0 = conv_fwd(x, w, None, kh, kw)
    p = plant_pixel(B, H, W)
    bias[0] = (-acc[p][0] + E20 * A0[p][0]).float()
    want, A = conv_fwd(x, w, bias, kh, kw)
    return x, w, bias, want, A


def conv_taps(x, w, kh, kw, wrap=None, drop=None):
    """The same conv written as the kernels walk it, one GEMM per tap over flat pixels, in
    fp64.  Mutants: ``wrap="row"`` masks a tap only by its flat index inside the image (a
    tap past the row end reads the next row), ``wrap="image"`` only by the flat index
    inside the whole stack (a tap past the image reads the next image); ``drop=(ky, kx)``
    leaves that tap out at the output pixels of the last column (kx != centre) or last row."""
    B, H, W, C = x.shape
    xf = x.double().reshape(B * H * W, C)
    wd = w.double()
    P = B * H * W
    p = torch.arange(P)
    b, q = p // (H * W), p % (H * W)
    y, xx = q // W, q % W
    out = torch.zeros(P, w.shape[0], dtype=F64)
    for ky in range(kh):
        for kx in range(kw):
            dy, dx = ky - kh // 2, kx - kw // 2
            if wrap == "row":
                ok = (q + dy * W + dx >= 0) & (q + dy * W + dx < H * W)
            elif wrap == "image":
                ok = (p + dy * W + dx >= 0) & (p + dy * W + dx < P)
            else:
                ok = (y + dy >= 0) & (y + dy < H) & (xx + dx >= 0) & (xx + dx < W)
            if drop == (ky, kx):
                ok = ok & ~((xx == W - 1) if dx != 0 else (y == H - 1))
            src = (p + dy * W + dx).clamp(0, P - 1)
            out += (xf[src] * ok[:, None]) @ wd[:, :, ky, kx].T
    return out.reshape(B, H, W, -1)


def droppable_tap(H, W, kh, kw):
    """A border tap whose input lies inside the image at the last column / row, if any."""
    if kw > 1 and W > 1:
        return kh // 2, kw // 2 - 1
    if kh > 1 and H > 1:
        return kh // 2 - 1, kw // 2
    return None


# ------------------------------------------------------------------ epilogue closed forms (conv_common.h)
def gate_bound(pre, pb, lip):
    """tests/test_gates_gpu.py: 2^-20 (1 + |pre|) for the fp32 sigmoid / tanh, plus the
    conv's accumulation bound through the gate's Lipschitz constant (1/4, 1)."""
    return E20 * (1.0 + pre.abs()) + lip * pb


def epi_plain(pre, pb, kind, scale=1.0):
    """EPI_BIAS / EPI_RELU (exact, 1-Lipschitz) / EPI_SCALE (one more rounding)."""
    if kind == EPI_RELU:
        return pre.clamp_min(0.0), pb
    if kind == EPI_SCALE:
        want = pre * scale
        return want, abs(scale) * pb + U * want.abs()
    return pre, pb


def epi_gru_zr(pre, pb, h, hd):
    """z = sigmoid(pre[:hd]); r = sigmoid(pre[hd:]); r h (one more rounding).  -> z, rh, r."""
    z, r = torch.sigmoid(pre[..., :hd]), torch.sigmoid(pre[..., hd:])
    bz, br = gate_bound(pre[..., :hd], pb[..., :hd], 0.25), gate_bound(pre[..., hd:], pb[..., hd:], 0.25)
    hh = h.double()
    rh = r * hh
    return (z, bz), (rh, hh.abs() * br + U * rh.abs()), (r, br)


def epi_gru_q(pre, pb, h, z):
    """q~ = tanh(pre); h' = (1 - z) h + z q~: 1 - z, two products and the sum round once each."""
    q, bq = torch.tanh(pre), gate_bound(pre, pb, 1.0)
    hh, zz = h.double(), z.double()
    a, b = (1.0 - zz) * hh, zz * q
    hn = a + b
    return (hn, zz.abs() * bq + U * (2.0 * a.abs() + b.abs() + hn.abs())), (q, bq)


def epi_relu_bwd(pre, pb, aux, ge=False):
    """out = v * (aux1 > 0): the mask is taken from the stored value, so 0.0 and -0.0 give
    exactly 0 (bound 0 there).  ``ge``: the mutant mask >= 0."""
    m = (aux.double() >= 0) if ge else (aux.double() > 0)
    return pre * m, pb * m


def epi_acc_f32(pre, pb, o0, overwrite=False):
    """out (fp32) += v: one rounding at the sum.  ``overwrite``: the mutant store."""
    want = pre if overwrite else o0.double() + pre
    return want, pb + U * want.abs()


def epi_gru_qbwd(pre, pb, h, r, o0, hd, r_only=False, store=False):
    """co < hd: dr_pre = v h r (1 - r) (1 - r and three products: 4 roundings) -> out2 (bf16),
    out[co] += v r (product, sum); co >= hd: out[co] += v.  Mutants: ``r_only`` uses r in
    place of r (1 - r); ``store`` writes v r instead of accumulating it."""
    v, vb = pre[..., :hd], pb[..., :hd]
    hh, rr, oo = h.double(), r.double(), o0.double()
    dr = v * hh * rr * (rr if r_only else (1.0 - rr))
    bdr = (hh * rr * (1.0 - rr)).abs() * vb + 4.0 * U * dr.abs()
    g = v * rr
    lo = g if store else oo[..., :hd] + g
    blo = rr.abs() * vb + U * g.abs() + U * lo.abs()
    hi = oo[..., hd:] + pre[..., hd:]
    bhi = pb[..., hd:] + U * hi.abs()
    return (torch.cat([lo, hi], -1), torch.cat([blo, bhi], -1)), (dr, bdr)


def epi_flow(pre, pb, src):
    """coords (fp32 NCHW) = src + v for the two flow channels."""
    want = src.double() + pre[..., :2].permute(0, 3, 1, 2)
    return want, pb[..., :2].permute(0, 3, 1, 2) + U * want.abs()


EPI_SHAPES = [(1, 1, 1), (1, 9, 33), (2, 5, 7)]
EPI_HD = 64
EPI_COUT = 128  # packed rows of an epilogue case's weight: z | r


@functools.lru_cache(maxsize=None)
def epi_case(B, H, W, kh, kw):
    """An epilogue case: x (bf16, 192 channels), w (128 rows), bias, pre = conv + bias, A, and
    the aux / prefill tensors.  Channels 0..10 and 64..74 have zero weight rows and the PLANT
    values as bias, so those pre-activations are exactly 0, +-1e-3, +-20, +-88, +-100, +-1e4
    in both halves of the z | r conv.  h in (-1, 1); z / r in [0, 1] with exact 0 and 1
    planted; the ReLU output ``actv`` holds 0.0, -0.0, the smallest positive normal and
    subnormal bf16 and negative values; o0 is the fp32 prefill of the accumulating outputs."""
    g = gen(B, H, W, kh, kw, 47)
    x = act((B, H, W, KTOT), BF16, g)
    w = rb(weight(EPI_COUT, KTOT, kh, g, kw))
    bias = 0.1 * torch.randn(EPI_COUT, generator=g)
    for base in (0, EPI_HD):
        for i, v in enumerate(PLANT):
            w[base + i] = 0
            bias[base + i] = v
    pre, A = conv_fwd(x, w, bias, kh, kw)
    pre0, A0 = conv_fwd(x, w, None, kh, kw)
    shp = (B, H, W, EPI_COUT)
    h = torch.tanh(torch.randn(*shp, generator=g)).to(BF16)
    z = torch.sigmoid(3.0 * torch.randn(*shp, generator=g))
    z[..., 3], z[..., 4] = 0.0, 1.0
    z = z.to(BF16)
    actv = torch.randn(*shp, generator=g)
    fi = torch.finfo(BF16)
    for i, v in enumerate((0.0, -0.0, fi.tiny, 2.0 ** -133, -fi.tiny, -1.0)):  # 2^-133: the smallest subnormal
        actv[..., i::16] = v  # every 4-channel epilogue group sees some of them
    actv = actv.to(BF16)
    o0 = torch.randn(*shp, generator=g)
    src = 10.0 * torch.randn(B, 2, H, W, generator=g)
    return dict(x=x, w=w, bias=bias, pre=pre, A=A, pre0=pre0, A0=A0, h=h, z=z, actv=actv, o0=o0, src=src)


# ------------------------------------------------------------------ weight gradients
WG_STACKS = [(1, 1, 1, 1), (1, 1, 1, 33), (2, 1, 9, 1), (3, 2, 1, 5), (1, 1, 8, 32), (2, 2, 9, 33), (3, 1, 5, 13)]
WG_COUTS = [64, 70, 126, 200]
WG_SEG = 128  # three segments of 128 channels: every tile variant keeps its 128-wide N tile
WG_KTOT = 3 * WG_SEG
WG_YOFF = 8
SENTINEL = 1.0e4


def wgrad_oracle(x, dy, kh, kw):
    """(dw, S, db, Sb): dw (Cout, Cin, kh, kw) fp64 and S = wgrad(|x|, |dy|); db = sum_p dy."""
    xd, gd = nchw(x), nchw(dy)
    size = (dy.shape[3], x.shape[3], kh, kw)
    pad = (kh // 2, kw // 2)
    dw = conv2d_weight(xd, size, gd, 1, pad)
    S = conv2d_weight(xd.abs(), size, gd.abs(), 1, pad)
    return dw, S, gd.sum((0, 2, 3)), gd.abs().sum((0, 2, 3))


def stack_x(x0, xb, x2, iters, mutant=False):
    """The conv input of a stack: segment 1 (``xb``, B images) repeats over the iterations.
    ``mutant``: it is read at the stack index instead (images past its own read as zeros,
    as a range-checked load returns them)."""
    if mutant:
        mid = torch.cat([xb, torch.zeros((x0.shape[0] - xb.shape[0], *xb.shape[1:]), dtype=xb.dtype)])
    else:
        mid = xb.repeat(iters, 1, 1, 1)
    return torch.cat([x0, mid, x2], -1)


@functools.lru_cache(maxsize=None)
def wgrad_case(iters, B, H, W, kh, kw):
    """Segments x0, xb (broadcast over the iterations; image b holds the constant b + 1 in
    channel 0, so a wrong image index moves dW by whole units), x2; dy (200 channels); and
    the oracle for Cout = 200 (a smaller Cout is its leading rows)."""
    g = gen(iters, B, H, W, kh, kw, 53)
    N = iters * B
    x0 = act((N, H, W, WG_SEG), BF16, g)
    xb = act((B, H, W, WG_SEG), BF16, g)
    for b in range(B):
        xb[b, :, :, 0] = b + 1.0
    x2 = act((N, H, W, WG_SEG), BF16, g)
    dy = act((N, H, W, COUT_MAX), BF16, g)
    dw, S, db, Sb = wgrad_oracle(stack_x(x0, xb, x2, iters), dy, kh, kw)
    return dict(x0=x0, xb=xb, x2=x2, dy=dy, dw=dw, S=S, db=db, Sb=Sb)


def dy_buffer(dy, cout):
    """dY's ``cout`` channels at WG_YOFF of a wider buffer: NaN before the window and after
    the last channel any M tile reads (round_up(cout, 256)); the channels between, which the
    DMA kernels read into discarded accumulator rows, hold a large finite sentinel."""
    wide = WG_YOFF + cdiv(cout, 256) * 256 + 8
    buf = torch.full((*dy.shape[:3], wide), float("nan"), dtype=dy.dtype)
    buf[..., WG_YOFF:WG_YOFF + cdiv(cout, 256) * 256] = SENTINEL
    buf[..., WG_YOFF:WG_YOFF + cout] = dy[..., :cout]
    return buf


def kernel_layout(dw):
    """(Cout, Cin, kh, kw) -> the kernels' [Cout][taps][Ktot]."""
    return dw.permute(0, 2, 3, 1).reshape(dw.shape[0], -1, dw.shape[1])


def wgrad_variant(var, cout, seg128=True):
    """csrc/conv_wgrad.hip wgrad_plan: (variant run, bm, bn, threads)."""
    if var in (1, 2, 3, 5) and not seg128:
        var = 0
    if var == 1 and cout <= 64:
        var = 0
    bm = 256 if var in (3, 4) else 64 if var == 5 else (64 if (var == 0 and cout <= 64) else 128)
    bn = 64 if var in (0, 4) else 128
    return var, bm, bn, (512 if 2 <= var <= 4 else 256)


def wgrad_plan(P, taps, ktot, cout, det, var, seg128=True):
    """(K splits, pixels per split) of variant ``var``."""
    _, bm, bn, _ = wgrad_variant(var, cout, seg128)
    ntiles, mtiles = taps * (ktot // bn), cdiv(cout, bm)
    ksplit = max(1, min(cdiv(1024, ntiles * mtiles), cdiv(P, 64 * 8)))
    if det:
        ksplit = min(ksplit, 32)
    kchunk = cdiv(cdiv(P, ksplit), 64) * 64
    return cdiv(P, kchunk), kchunk


def wgrad_chain(P, taps, ktot, cout, det, var):
    """Two 16x16x32 MFMA steps per 64-pixel K step of a split, one add per split (atomics,
    or det_reduce's ordered sum) and the add onto dw."""
    ksplit, kchunk = wgrad_plan(P, taps, ktot, cout, det, var)
    return MFMA * 2 * (kchunk // 64) + ksplit + 1


def wgrad_bias_chain(P, taps, ktot, cout, det, var):
    """db: a thread adds 64 (BM / 8) / threads staged rows per K step, threads / (BM / 8)
    threads share a column, then the splits and the add onto db."""
    _, bm, _, nthr = wgrad_variant(var, cout)
    ksplit, kchunk = wgrad_plan(P, taps, ktot, cout, det, var)
    ca = bm // 8
    return (64 * ca // nthr) * (kchunk // 64) + nthr // ca + ksplit + 1


def wgrad3_splits(NI, H, W, cout, ktot, bm):
    """csrc/wgrad_v3.hip wgrad3_splits / wgrad3_launch: (splits, patches per block); 4 x 32 patches."""
    npatch = NI * cdiv(H, 4) * cdiv(W, 32)
    tiles = cdiv(cout, bm) * (ktot // 64)
    ns = min(max(1, 512 // max(1, tiles)), npatch)
    return ns, cdiv(npatch, ns)


def wgrad3_chain(NI, H, W, cout, ktot, bm):
    """8 K steps (4 patch rows x 2 halves of 16 pixels), one 32x32x16 MFMA each per tap
    accumulator, per patch of the block; wg3_reduce adds the splits in order, then onto dw."""
    ns, ppb = wgrad3_splits(NI, H, W, cout, ktot, bm)
    return MFMA * 8 * ppb + ns


def wgrad3_bias_chain(NI, H, W, cout, ktot, bm):
    """A lane adds the 8 pixels of its A fragment per K step, the two half-waves are
    added, then the splits in order and the add onto db."""
    ns, ppb = wgrad3_splits(NI, H, W, cout, ktot, bm)
    return 8 * 8 * ppb + 1 + ns + 1


def colsum_blocks(P):
    return cdiv(P, 256)


def colsum_chain(P):
    """A thread adds its block's <= 256 pixels, then one add per block and onto db."""
    return min(P, 256) + colsum_blocks(P) + 1


def mutant_drop_last_pixel(case, iters, kh, kw):
    """(7) the last pixel of the stack left out of dW and db."""
    g = case["dy"].clone()
    g[-1, -1, -1] = 0
    dw, _, db, _ = wgrad_oracle(stack_x(case["x0"], case["xb"], case["x2"], iters), g, kh, kw)
    return dw, db


# ------------------------------------------------------------------ element-wise backward ops
def gru_gate_bwd_oracle(dh, z, q, h):
    """csrc/conv.hip gru_gate_bwd_kernel: dq_pre = dh' z (1 - q~^2), dz_pre = dh' (q~ - h) z (1 - z),
    dh = dh' (1 - z).  Bounds: q~ q~ rounds at U q~^2, which 1 - q~^2 does not shrink (exact
    +-1 cancel to 0), then 1 - ., and three products; (q~ - h), (1 - z) and three products;
    (1 - z) and one product: every factor's rounding is relative to the result."""
    g, zz, qq, hh = dh.double(), z.double(), q.double(), h.double()
    dq = g * zz * (1.0 - qq * qq)
    dz = g * (qq - hh) * zz * (1.0 - zz)
    dhn = g * (1.0 - zz)
    bq = U * ((g * zz).abs() * qq * qq + 4.0 * dq.abs())
    return (dq, bq), (dz, 5.0 * U * dz.abs()), (dhn, 2.0 * U * dhn.abs())


GATE_BWD_HD = [96, 128]
GATE_BWD_P = [(2, 5, 7), (1, 1, 1)]


@functools.lru_cache(maxsize=None)
def gate_bwd_case(shape, hd, dtype):
    g = gen(*shape, hd, 59, 1 if dtype == BF16 else 2)
    s = (*shape, hd)
    dh = torch.randn(*s, generator=g)
    z = torch.sigmoid(3.0 * torch.randn(*s, generator=g))
    q = torch.tanh(2.0 * torch.randn(*s, generator=g))
    h = torch.tanh(torch.randn(*s, generator=g))
    z[..., 0], z[..., 1] = 0.0, 1.0
    q[..., 0], q[..., 1], q[..., 2], q[..., 3] = 1.0, -1.0, 0.0, 1.0
    z[..., 3] = 1.0
    return dh, z.to(dtype), q.to(dtype), h.to(dtype)


# relu_take's two in-tree call shapes (models/fused_train.py): (G width, n, out width)
RELU_TAKE_SHAPES = [(256, 126, 128), (160, 80, 96)]
RELU_TAKE_P = (2, 5, 7)


def relu_take_oracle(G, goff, n, nz, actv, aoff, width):
    """out = G[:, goff:goff+n] * (act[:, aoff:aoff+n] > 0), zero-filled to ``width``;
    G[:, goff:goff+nz] = 0 afterwards.  Exact: a select, no arithmetic."""
    out = torch.zeros((*G.shape[:-1], width), dtype=F64)
    out[..., :n] = G[..., goff:goff + n].double() * (actv[..., aoff:aoff + n].double() > 0)
    Gn = G.clone()
    Gn[..., goff:goff + nz] = 0
    return out, Gn


@functools.lru_cache(maxsize=None)
def relu_take_case(gw, n, dtype):
    g = gen(gw, n, 61, 1 if dtype == BF16 else 2)
    G = torch.randn(*RELU_TAKE_P, gw, generator=g)
    actv = torch.randn(*RELU_TAKE_P, n + 16, generator=g)
    actv[..., 8::5] = 0.0
    actv[..., 9::5] = -0.0
    return G, actv.to(dtype)

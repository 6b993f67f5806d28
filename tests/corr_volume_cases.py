"""fp64 oracles, bounds, launch mirrors and mutants of tests/test_corr_volume_edges_gpu.py (CPU only).

The all-pairs correlation volume behind ``AllPairsCorr``: ``corr_volume`` (csrc/corr_volume.hip:
pool_f2_kernel + corr_flat_kernel for bf16 maps, split3_kernel + the same flat GEMM over K = 3C
or corr_volume_f32_kernel for fp32 maps), the pyramid-gradient fold (csrc/corr_lookup.hip
pyr_grad_fold_launch: pyr_fold_wave_kernel<4|8|12>, pyr_fold_rows_kernel, pyr_fold4_kernel,
pyr_fold_kernel) and ``corr_volume_backward`` (csrc/corr_bwd.hip: one launch, gemm_tile<false>
df1 = G f2 and gemm_tile<true> df2 = G^T f1).  Everything here is plain PyTorch in float64 on
the CPU, evaluated on the values the kernels read: the features rounded to their storage dtype
and the scale rounded to fp32 (the launchers take it as a float).

Oracles.
  pyramid   vol0[b,i,n] = scale sum_c f1[b,i,c] f2[b,n,c]; level l = avg_pool2d(., 2, 2) applied
            l times in float64 (floor sizes).  ops/reference.py corr_pyramid forces fp32: not used.
  fold      G0 = scale (g0 + sum_{l>=1} 4^-l g_l[y>>l, x>>l]), the term present only where
            y>>l < H_l and x>>l < W_l (the last odd row / column has no parent).
  backward  df1[b] = G0[b] f2[b], df2[b] = G0[b]^T f1[b] with G0 the unrounded fp64 fold.

Bounds, per element.  u = 2^-24 is one fp32 rounding of the magnitude term (a first-order
bound: n roundings cost n u, the (1 + u)^n - 1 - n u remainder is below 1e-5 of the bound for
every n here); an MFMA step counts 2 u; "bf16 out" adds 2^-8 |want|, one bf16 rounding.  The
magnitude terms are the same sums with absolute values:
  A0 = scale sum_c |f1| |f2|, A_l = avgpool^l(A0);
  Wf = scale (|g0| + sum 4^-l |g_l[parent]|);
  T1 = sum_n |G0| |f2| (K = N2), T2 = sum_i |G0| |f1| (K = N1).

  volume, exact fp32, level l     (C + 2 + 3 l) u A_l
      mfma_f32_16x16x4f32 is an fmaf chain: C roundings of one accumulator; the product with
      scale is one more, the fp32 rounding of scale itself is taken out by the oracle (+ 1 of
      slack); every level adds v += shfl, v += shfl (two adds; the 0.25 is exact): 2 <= 3 per level.
  volume, bf16 maps, level 0      (C + 2) u A_0
      bf16 x bf16 products are exact in fp32; C / 32 steps of mfma_f32_16x16x32_bf16 at 2 u are
      C / 16 <= C roundings, + the product with scale, + 1 of slack.
  volume, bf16 maps, level l >= 1 (2^-8 + (4^l + 1) u + (C + 2) u) A_l
      by linearity level l = corr(f1, avgpool^l f2).  pool_f2_kernel sums the 4^l bf16 values in
      fp32 (4^l - 1 adds, the 1 / 4^l exact) and rounds ONCE to bf16: 2^-8 of |pooled f2| <=
      avgpool |f2|, which under sum_c |f1| . is 2^-8 A_l; then the level-0 chain.
  volume, fp32 split, level l     (3 2^-16 + (3 C + 3 + 4^l) u) A_l
      split3_kernel pools in fp32 (4^l - 1 adds), then x = hi + lo + d with hi = bf16(x),
      lo = bf16(x - hi): |x - hi| <= 2^-8 |x|, |d| <= 2^-8 |x - hi| <= 2^-16 |x|.  The GEMM over
      K = 3C adds hi hi + hi lo + lo hi: what is missing is d1 f2, f1 d2 and lo lo, each at most
      2^-16 of |f1| |f2|; 3C / 32 MFMA steps at 2 u <= 3C u, + scale, + slack.
  fold, fp32 in place             8 u Wf
      three v += w g_l (a product and an add each when not contracted: 6), the product with
      scale (1), 1 of slack; every partial sum is below Wf / scale.
  fold, bf16 out                  8 u Wf + 2^-8 |want|
  df1 / df2, bf16 features        (2^-8 + 8 u + (K + 2) u) T + 2^-8 |want|
      G = bf16(fold): 2^-8 |G0| per element under sum |.| |f| is 2^-8 T, the fold's own 8 u
      (taken against |G0|: the level terms of no case here cancel to 2^-13 of Wf, where that
      would matter); K / 16 steps of mfma_f32_32x32x16_bf16 at 2 u <= K u; the bf16 store.
  df1 / df2, fp32 split           (3 2^-16 + (3 K + 10) u) T
      G and the features as hi + lo pairs, three K passes (hi hi + hi lo + lo hi) into one
      accumulator: the three 2^-16 residuals as above, 3 K / 16 MFMA steps at 2 u, the fold's 8 u.

tests/test_corr_volume_oracles_cpu.py ties the oracles to float64 autograd and the mirrors to
the sources, and shows that a plain emulation of every route stays inside every bound and that
every mutant below leaves it.
"""
import functools

import numpy as np
import torch
import torch.nn.functional as F

from enc_conv_cases import BF16, F32, F64, U, cdiv, gen, ratio, rb, split_bf16, touched_ratio  # noqa: F401

E8, E16 = 2.0 ** -8, 2.0 ** -16


def round_up(a, b):
    return (a + b - 1) // b * b


def f32(x):
    """The value a ``float`` kernel argument holds."""
    return float(np.float32(x))


def level_sizes(H, W, levels):
    return [(H >> l, W >> l) for l in range(levels)]


def max_levels(H, W):
    return max(1, min(4, min(H, W).bit_length()))


# ------------------------------------------------------------------ mirrors of the launch code
FB = 128               # corr_volume.hip: targets and queries per flat tile
VOL_PITCH = 64         # ops.cpp corr_volume: S_l = round_up(H_l W_l, 64)
EXACT_BLOCK = (64, 8, 32)  # corr_volume.hip BM, TH, TW of the exact kernel
FW_LDS = 1024          # corr_lookup.hip: coarse cells a wave of pyr_fold_wave_kernel stages
FOLD_LDS = 4096        # ... a block of pyr_fold_rows_kernel stages
WAVE_PITCH_MAX = 64 * 4 * 12
ROWS_PITCH_MAX = 6144
QW_STEPS = (4, 8)      # qw <= 4 -> <4>, <= 8 -> <8>, else <12>
FOLD4_GRID_Y = 65535
BWD_BM, BWD_BN, BWD_BK = 128, 128, 64  # corr_bwd.hip cgemm
BWD_ROWFOLD = (6144, 4096)             # ops.cpp / ops/corr.py: Ep and coarse limits of the row fold


def volume_route(dtype, C):
    """ops.cpp corr_volume, RS_CORR_F32_SPLIT unset: which kernels a (dtype, C) reaches."""
    if dtype == BF16:
        return "flat_bf16"
    return "flat_split" if (3 * C) % 64 == 0 else "exact"


def volume_accepts(dtype, C):
    return C % (64 if dtype == BF16 else 32) == 0


def volume_pitch(h, w):
    return round_up(h * w, VOL_PITCH)


def fold_route(E, S0, aligned, coarse, opitch, bf16_out, lo=False):
    """pyr_grad_fold_launch's selection ladder.  ``aligned``: the level-0 pointer is a multiple
    of 16 bytes; ``opitch`` <= 0: E (pyr_grad_fold_bf16)."""
    if opitch <= 0:
        opitch = E
    aligned0 = S0 % 4 == 0 and aligned
    if bf16_out and not lo and aligned0 and opitch % 4 == 0 and opitch <= WAVE_PITCH_MAX and coarse <= FW_LDS:
        qw = (opitch + 255) // 256
        return "wave4" if qw <= QW_STEPS[0] else "wave8" if qw <= QW_STEPS[1] else "wave12"
    if bf16_out and opitch % 4 == 0 and opitch <= ROWS_PITCH_MAX and coarse <= FOLD_LDS:
        return f"rows(vec0={int(aligned0)})"
    if aligned0 and E < 2 ** 30:
        return f"fold4(vec_out={int(opitch % 4 == 0)})" if bf16_out else "fold4"
    return "flat"


def corr_bwd_pitch(N2):
    return round_up(N2, BWD_BK)


def coarse_cells(H, W, levels):
    return sum(h * w for h, w in level_sizes(H, W, levels)[1:])


def bwd_route(B, N1, H2, W2, C, dtype, coarse, S0, aligned):
    """ops.cpp corr_volume_backward: (accepted, rowfold, Ep, fold kernel).  The TORCH_CHECKs on
    shapes that ops/corr.py::_fused_bwd_ok repeats."""
    split = dtype == F32
    N2 = H2 * W2
    Ep = corr_bwd_pitch(N2)
    rowfold = Ep <= BWD_ROWFOLD[0] and coarse <= BWD_ROWFOLD[1]
    ok = (C % 128 == 0 and dtype in (BF16, F32)
          and (rowfold or (not split and S0 % 4 == 0 and aligned))
          and B * N1 * Ep * 2 < 2 ** 31 and B * max(N1, N2) * C * 2 < 2 ** 31)
    return dict(ok=ok, rowfold=rowfold, Ep=Ep,
                fold=fold_route(N2, S0, aligned, coarse, Ep, True, lo=split) if ok else None)


def quad_row(e, W0):
    """The row of level-0 cell ``e`` as the wave and rows fold kernels compute it:
    (int)(((float)e + 0.5f) * (1.f / W0)) in float32."""
    e = np.asarray(e)
    inv = np.float32(1.0) / np.asarray(W0, dtype=np.float32)
    return ((e.astype(np.float32) + np.float32(0.5)) * inv).astype(np.int32)


# ------------------------------------------------------------------ inputs
KINDS = ("randn", "spread", "zeros", "cancel", "coherent")
# pixel values 1 + k 2^-7 of the "coherent" map, tiled: the 2x2 means are 1.5, 3.5, 3.5, 3.5
# (ties of bf16), the 4x4 mean is 3 exactly
COHERENT = ((1, 1, 3, 3), (2, 2, 4, 4), (3, 3, 3, 3), (4, 4, 4, 4))


@functools.lru_cache(None)
def features(B, N1, H2, W2, C, dtype, kind="randn"):
    """(f1 (B, N1, C), f2 (B, H2, W2, C)) as stored.
    spread:   channel c of f1 / f2 times 2^e, e over -20 .. 20 (products stay normal);
    zeros:    one f1 row and one f2 pixel all zero, every other channel -0.0;
    cancel:   inside every 2x2 window f2(0,1) = -f2(0,0) and f2(1,1) = -f2(1,0) (1 + 2^-5):
              level 1 is about 2^-7 of A_1;
    coherent: f1 = 1, f2 = 1 + k 2^-7 constant over the channels (COHERENT): every rounding
              error has one sign."""
    g = gen(B, N1, H2, W2, C, KINDS.index(kind), dtype == BF16)
    f1 = torch.randn(B, N1, C, generator=g)
    f2 = torch.randn(B, H2, W2, C, generator=g)
    if kind == "spread":
        e1 = torch.linspace(-20, 20, C).round()[torch.randperm(C, generator=g)]
        e2 = torch.linspace(-20, 20, C).round()[torch.randperm(C, generator=g)]
        f1, f2 = f1 * 2.0 ** e1, f2 * 2.0 ** e2
    elif kind == "zeros":
        z = torch.zeros(C)
        z[1::2] = -0.0
        f1[:, N1 // 2] = z
        f2[:, H2 // 2, W2 // 2] = z
    elif kind == "cancel":
        f2 = f2.to(dtype).float()
        he, we = H2 // 2 * 2, W2 // 2 * 2
        f2[:, 0:he:2, 1:we:2] = -f2[:, 0:he:2, 0:we:2]
        f2[:, 1:he:2, 1:we:2] = -f2[:, 1:he:2, 0:we:2] * (1 + 2.0 ** -5)
    elif kind == "coherent":
        k = torch.tensor(COHERENT, dtype=F32)[torch.arange(H2)[:, None] % 4, torch.arange(W2)[None, :] % 4]
        f1 = torch.ones(B, N1, C)
        f2 = (1 + k * 2.0 ** -7)[None, :, :, None].expand(B, H2, W2, C).contiguous()
    return f1.to(dtype), f2.to(dtype)


GRAD_SCALES = (1e-7, 1.0, 1e3)


@functools.lru_cache(None)
def grad_pyramid(B, N1, H, W, levels, mag=1.0, key=0):
    """fp32 gradient levels (B, N1, H_l, W_l); row N1 // 2 of every batch image all zero (N1 > 2)."""
    g = gen(B, N1, H, W, levels, key)
    out = []
    for h, w in level_sizes(H, W, levels):
        t = (mag * torch.randn(B, N1, h, w, generator=g)).to(F32)
        if N1 > 2:
            t[:, N1 // 2] = 0
        out.append(t)
    return tuple(out)


# ------------------------------------------------------------------ oracles
def _vol0(f1, f2, scale):
    B, N1, C = f1.shape
    _, H2, W2, _ = f2.shape
    v = torch.einsum("bic,bnc->bin", f1.double(), f2.double().reshape(B, H2 * W2, C))
    return f32(scale) * v.reshape(B, N1, H2, W2)


def pyramid(f1, f2, levels, scale):
    """[(vol_l, A_l)], float64."""
    v, A = _vol0(f1, f2, scale), _vol0(f1.abs(), f2.abs(), scale)
    out = [(v, A)]
    for _ in range(1, levels):
        v, A = F.avg_pool2d(v, 2, 2), F.avg_pool2d(A, 2, 2)
        out.append((v, A))
    return out


def vol_bound(route, l, C, A, want=None, out_bf16=False):
    if route == "exact":
        b = (C + 2 + 3 * l) * U * A
    elif route == "flat_bf16":
        b = (C + 2) * U * A if l == 0 else (E8 + (4 ** l + 1) * U + (C + 2) * U) * A
    elif route == "flat_split":
        b = (3 * E16 + (3 * C + 3 + 4 ** l) * U) * A
    else:
        raise ValueError(route)
    return b + E8 * want.abs() if out_bf16 else b


def fold(gpyr, scale, mutant=None):
    """(G0, Wf) (B, N1, H0, W0) float64.  mutant: 'clamp_parent' (a cell without a parent takes
    the last one), 'weight_pow2' (2^-l), 'row_index' (the last row's cells find their row by
    e // (W0 + 1))."""
    g0 = gpyr[0].double()
    B, N1, H0, W0 = g0.shape
    e = torch.arange(H0 * W0)
    y = e // W0
    if mutant == "row_index":
        y = torch.where(y == H0 - 1, e // (W0 + 1), y)
    x = e - y * W0
    G, Wf = g0.reshape(B, N1, -1).clone(), g0.abs().reshape(B, N1, -1)
    for l in range(1, len(gpyr)):
        h, w = gpyr[l].shape[2:]
        if h == 0 or w == 0:
            continue
        yl, xl = y >> l, x >> l
        ok = (yl < h) & (xl < w)
        if mutant == "clamp_parent":
            ok = torch.ones_like(ok)
        idx = yl.clamp(max=h - 1) * w + xl.clamp(max=w - 1)
        up = gpyr[l].double().reshape(B, N1, h * w)[:, :, idx]
        wt = (0.5 if mutant == "weight_pow2" else 0.25) ** l
        zero = torch.zeros((), dtype=F64)
        G = G + torch.where(ok, wt * up, zero)
        Wf = Wf + torch.where(ok, wt * up.abs(), zero)
    s = f32(scale)
    return (s * G).reshape(B, N1, H0, W0), (s * Wf).reshape(B, N1, H0, W0)


def fold_bound(Wf, want=None, out_bf16=False):
    b = 8 * U * Wf
    return b + E8 * want.abs() if out_bf16 else b


def backward(G0, f1, f2):
    """(df1, df2, T1, T2) float64 from the unrounded fold."""
    B, N1, C = f1.shape
    G = G0.reshape(B, N1, -1)
    a, b = f1.double(), f2.double().reshape(B, -1, C)
    return (G @ b, (G.transpose(1, 2) @ a).reshape(f2.shape),
            G.abs() @ b.abs(), (G.abs().transpose(1, 2) @ a.abs()).reshape(f2.shape))


def bwd_bound(split, K, T, want):
    if split:
        return (3 * E16 + (3 * K + 10) * U) * T
    return (E8 + 8 * U + (K + 2) * U) * T + E8 * want.abs()


# ------------------------------------------------------------------ plain emulations of each route
def _pool_direct(x, l):
    """(B, H, W, C) fp32 -> level l by one fp32 mean over 2^l x 2^l blocks (floor sizes)."""
    if l == 0:
        return x
    return F.avg_pool2d(x.permute(0, 3, 1, 2), 2 ** l, 2 ** l).permute(0, 2, 3, 1).contiguous()


def emulate_volume(f1, f2, levels, scale, route, out_bf16=False):
    """The route's arithmetic in fp32 on the CPU; list of (B, N1, H_l, W_l)."""
    B, N1, C = f1.shape
    s = torch.tensor(scale, dtype=F32)
    a, x = f1.float(), f2.float()
    out = []
    if route == "exact":
        v = (a @ x.reshape(B, -1, C).transpose(1, 2)).reshape(B, N1, *x.shape[1:3]) * s
        for l in range(levels):
            if l:
                v = F.avg_pool2d(v, 2, 2)
            out.append(v)
        return out
    ah, al = split_bf16(a)
    for l in range(levels):
        p = _pool_direct(x, l)
        hw = p.shape[1:3]
        if route == "flat_bf16":
            v = a @ rb(p).reshape(B, -1, C).transpose(1, 2)
        else:
            ph, pl = (t.reshape(B, -1, C).transpose(1, 2) for t in split_bf16(p))
            v = ah @ ph + ah @ pl + al @ ph
        v = (v * s).reshape(B, N1, *hw)
        out.append(rb(v) if out_bf16 else v)
    return out


def emulate_fold(gpyr, scale, out_bf16=False):
    g0 = gpyr[0]
    B, N1, H0, W0 = g0.shape
    y, x = torch.arange(H0)[:, None], torch.arange(W0)[None, :]
    v = g0.clone()
    for l in range(1, len(gpyr)):
        h, w = gpyr[l].shape[2:]
        if h == 0 or w == 0:
            continue
        ok = ((y >> l) < h) & ((x >> l) < w)
        up = gpyr[l][:, :, (y >> l).clamp(max=h - 1), (x >> l).clamp(max=w - 1)]
        v = v + torch.where(ok, torch.tensor(0.25 ** l, dtype=F32) * up, torch.zeros((), dtype=F32))
    v = v * torch.tensor(scale, dtype=F32)
    return rb(v) if out_bf16 else v


def emulate_backward(gpyr, f1, f2, scale):
    """bf16 features: G = bf16(fold), fp32 accumulation, bf16 store; fp32: the three split products."""
    B, N1, C = f1.shape
    G = emulate_fold(gpyr, scale).reshape(B, N1, -1)
    if f1.dtype == BF16:
        Gh, a, b = rb(G), f1.float(), f2.float().reshape(B, -1, C)
        return rb(Gh @ b), rb(Gh.transpose(1, 2) @ a).reshape(f2.shape)
    (Gh, Gl), (ah, al), (bh, bl) = split_bf16(G), split_bf16(f1), split_bf16(f2.reshape(B, -1, C))
    df1 = Gh @ bh + Gh @ bl + Gl @ bh
    GhT, GlT = Gh.transpose(1, 2), Gl.transpose(1, 2)
    return df1, (GhT @ ah + GhT @ al + GlT @ ah).reshape(f2.shape)


# ------------------------------------------------------------------ mutants (float64, one defect each)
def _pool_ceil_parent(v):
    """avg_pool2d(2, 2), but at an odd width the last pooled column takes columns W-2, W-1."""
    out = F.avg_pool2d(v, 2, 2)
    W = v.shape[-1]
    if W % 2 == 1 and W >= 3:
        out[..., -1] = F.avg_pool2d(v[..., W - 2:W], 2, 2)[..., 0]
    return out


def mutant_volume(name, f1, f2, levels, scale):
    """The pyramid oracle with one defect; list of (B, N1, H_l, W_l) float64."""
    B, N1, C = f1.shape
    if name == "batch":
        f2 = f2.clone()
        f2[1] = f2[0]
    if name in ("hi_only", "double_round"):
        a = f1.double() if name == "double_round" else rb(f1.float()).double()
        p, out = f2.float(), []
        for l in range(levels):
            if l:
                p = _pool_direct(p, 1)
                if name == "double_round":
                    p = rb(p)  # rounded at every level, not once
            q = p if name == "double_round" else rb(_pool_direct(f2.float(), l))
            v = torch.einsum("bic,bnc->bin", a, q.double().reshape(B, -1, C))
            out.append((f32(scale) * v).reshape(B, N1, *q.shape[1:3]))
        return out
    v = _vol0(f1, f2, scale)
    out = [v]
    for _ in range(1, levels):
        if name == "ceil_parent":
            v = _pool_ceil_parent(v)
        elif name == "no_quarter":
            v = 4 * F.avg_pool2d(v, 2, 2)
        else:
            v = F.avg_pool2d(v, 2, 2)
        out.append(v)
    if name == "row_copy":
        out = [t.clone() for t in out]
        for t in out:
            t[:, N1 - 1] = t[:, N1 - 2]
    return out


FWD_MUTANTS = ("ceil_parent", "no_quarter", "row_copy", "batch", "hi_only", "double_round")
FOLD_MUTANTS = ("clamp_parent", "weight_pow2", "row_index")
BWD_MUTANTS = ("untransposed", "k_tail", "hi_only", "batch_row")


def mutant_backward(name, G0, f1, f2):
    """(df1, df2) float64 with one defect."""
    B, N1, C = f1.shape
    G = G0.reshape(B, N1, -1).clone()
    a, b = f1.double(), f2.double().reshape(B, -1, C)
    N2 = G.shape[2]
    G1 = G
    if name == "batch_row":
        G[1, 0] = G[0, 0]
    elif name == "hi_only":
        G, a, b = rb(G.float()).double(), rb(f1.float()).double(), rb(f2.float()).double().reshape(B, -1, C)
        G1 = G
    elif name == "k_tail":
        G1 = G.clone()
        G1[:, :, N2 - N2 % BWD_BK:] = 0
    Gt = G if (name == "untransposed" and N1 == N2) else G.transpose(1, 2)
    return G1 @ b, (Gt @ a).reshape(f2.shape)


# ------------------------------------------------------------------ case tables
# (H2, W2, levels): the smallest target grids that reach each path of the volume kernels
GRIDS = ((1, 1, 1), (1, 5, 1), (2, 2, 2), (3, 3, 2), (8, 8, 4), (9, 15, 4), (8, 33, 4), (9, 32, 4), (15, 17, 4),
         (11, 12, 3), (10, 13, 3), (16, 16, 4))
N1S = (1, 63, 64, 65, 127, 128, 129)
CHANNELS = {"flat_bf16": (64, 128, 256), "flat_split": (64, 128, 256), "exact": (32, 96, 160)}
ROUTE_DTYPE = {"flat_bf16": BF16, "flat_split": F32, "exact": F32}


def fwd_pairs():
    """(N1, H2, W2, levels, k): every grid at two N1, every N1 at three grids or more;
    k picks the channel count of each route."""
    out = []
    for i, (H, W, L) in enumerate(GRIDS):
        out.append((N1S[i % 7], H, W, L, i % 3))
        out.append((N1S[(i + 3) % 7], H, W, L, (i + 1) % 3))
    return out


# value cases: (kind, N1, H2, W2, levels)
VALUE_CASES = (("spread", 65, 9, 15, 4), ("zeros", 65, 9, 15, 4), ("cancel", 65, 9, 15, 4), ("coherent", 64, 8, 8, 4))

# fold: (name, B, N1, H, W, levels, store, in-place kernel, bf16 kernel).  store: 'pitched'
# (S = round_up(E, 64)), 'compact' (S = E) or an int added to E.
FOLD_CASES = (
    ("wave4", 2, 6, 16, 16, 4, "pitched", "fold4", "wave4"),
    ("wave8", 2, 6, 23, 64, 4, "pitched", "fold4", "wave8"),
    ("wave12", 2, 4, 48, 64, 4, "pitched", "fold4", "wave12"),
    ("rows", 2, 4, 40, 77, 4, "pitched", "fold4", "rows(vec0=1)"),
    ("rows_unaligned", 2, 6, 16, 16, 4, 2, "flat", "rows(vec0=0)"),
    ("fold4_7x9", 2, 6, 7, 9, 3, "pitched", "fold4", "fold4(vec_out=0)"),
    ("fold4_12x20", 2, 6, 12, 20, 4, "pitched", "fold4", "wave4"),
    ("fold4_12x20_compact", 2, 6, 12, 20, 4, "compact", "fold4", "wave4"),
    ("flat_7x9", 2, 6, 7, 9, 3, "compact", "flat", "flat"),
    ("wave_5_rows", 1, 5, 16, 16, 4, "pitched", "fold4", "wave4"),
    ("no_parent_9x15", 2, 6, 9, 15, 4, "pitched", "fold4", "fold4(vec_out=0)"),
    ("no_parent_9x15_L2", 2, 6, 9, 15, 2, "compact", "flat", "flat"),
    ("levels1", 2, 6, 16, 16, 1, "pitched", "fold4", "wave4"),
    ("levels2", 2, 6, 23, 64, 2, "pitched", "fold4", "wave8"),
    ("levels3", 2, 4, 40, 77, 3, "pitched", "fold4", "rows(vec0=1)"),
)
FOLD_BIG = (("rows_70001_L1", 1, 70001, 1, 5, 1, "pitched", "fold4", "fold4(vec_out=0)"),
            ("rows_70001_L2", 1, 70001, 1, 5, 2, "pitched", "fold4", "fold4(vec_out=0)"))


def fold_pitch(E, store):
    return round_up(E, 64) if store == "pitched" else E if store == "compact" else E + store


# backward: (N1, H2, W2)
BWD_SHAPES = ((1, 1, 1), (63, 7, 9), (64, 8, 8), (65, 5, 13), (127, 10, 13), (129, 11, 12), (200, 8, 33), (130, 16, 16))
BWD_QUAD = (70, 48, 131)  # N2 = 6288 > 6144: the quad fold (bf16 only)


# ------------------------------------------------------------------ the chain: window lookup, float64
def lookup(pyr, coords, r):
    """Bilinear window lookup with zero padding, linear in the pyramid (ops/reference.py
    corr_lookup without its division by W_l - 1, which a 1x1 level does not survive).
    pyr: levels (B, H*W, h_l, w_l); coords (B, 2, H, W) as [x, y]; -> (B, H, W, L (2r+1)^2),
    channel (dx + r) (2r + 1) + (dy + r) within a level."""
    B, _, H, W = coords.shape
    N1, D = H * W, 2 * r + 1
    cx, cy = coords[:, 0].reshape(B, N1, 1).double(), coords[:, 1].reshape(B, N1, 1).double()
    d = torch.arange(-r, r + 1, dtype=F64)
    dx, dy = d.repeat_interleave(D), d.repeat(D)
    outs = []
    for l, v in enumerate(pyr):
        h, w = v.shape[2:]
        px, py = cx / 2 ** l + dx, cy / 2 ** l + dy
        x0, y0 = px.floor(), py.floor()
        fx, fy = px - x0, py - y0
        flat, acc = v.reshape(B, N1, h * w), 0
        for ox, oy, wt in ((0, 0, (1 - fx) * (1 - fy)), (1, 0, fx * (1 - fy)), (0, 1, (1 - fx) * fy), (1, 1, fx * fy)):
            xi, yi = x0 + ox, y0 + oy
            ok = (xi >= 0) & (xi < w) & (yi >= 0) & (yi < h)
            idx = (yi.clamp(0, h - 1) * w + xi.clamp(0, w - 1)).long()
            acc = acc + torch.where(ok, wt * flat.gather(2, idx), torch.zeros((), dtype=F64))
        outs.append(acc)
    return torch.cat(outs, -1).reshape(B, H, W, -1)


LOOKUP_TOL = 1e-5  # tests/test_corr_edges_gpu.py: atol = rtol of the lookup and of its backward
CHAIN_CASES = ((128, 9, 15, 3), (256, 10, 13, 4))  # (C, H, W, radius), 4 levels


@functools.lru_cache(None)
def chain_coords(H, W, key):
    g = gen(H, W, key, 77)
    xs = torch.arange(W, dtype=F32).view(1, W).expand(H, W)
    ys = torch.arange(H, dtype=F32).view(H, 1).expand(H, W)
    c = torch.stack([xs, ys])[None].repeat(2, 1, 1, 1) + 2.5 * torch.randn(2, 2, H, W, generator=g)
    c[:, :, 0] = c[:, :, 0].round()  # exact integers: the upper taps weigh 0
    return c

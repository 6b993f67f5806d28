"""fp64 oracles and planted inputs of tests/test_flow_path_gpu.py (CPU only).

Everything here is plain PyTorch in float64 on the CPU (``F.conv2d``,
``F.unfold`` + softmax, closed forms): no fused code path.  The oracles are
evaluated on the values the kernels read, i.e. after rounding to the storage
dtype.  tests/test_edge_oracles_cpu.py ties them to ``ops/reference.py``, to
autograd and to the composite loss, and checks that the bounds discriminate.
"""
import math

import torch
import torch.nn.functional as F

F32, BF16 = torch.float32, torch.bfloat16


def grid(B, H, W, dtype=F32):
    ys = torch.arange(H, dtype=dtype).view(H, 1).expand(H, W)
    xs = torch.arange(W, dtype=dtype).view(1, W).expand(H, W)
    return torch.stack([xs, ys], 0).unsqueeze(0).repeat(B, 1, 1, 1)


# ------------------------------------------------------------------ flow encoder
FE_PLANT = [0.0, 1e-3, -1e-3, 255.5, -255.5, 400.0, -400.0, 1000.0, -1000.0]


def fe_spots(H, W):
    """The four corners and the two sides of the interior tile seam x = 7 | 8."""
    s = [(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1)]
    if W > 8:
        s += [(H // 2, 7), (H // 2, 8)]
    return s


def fe_inputs(B, H, W, Cout, seed, scale=100.0):
    """coords (fp32), the fp32 flow the kernel forms from them (coords - grid,
    one fp32 subtraction), w [49][2][Cout] and bias."""
    g = torch.Generator().manual_seed(seed)
    flow = scale * torch.randn(B, 2, H, W, generator=g)
    i = 0
    for b in range(B):
        for (y, x) in fe_spots(H, W):
            flow[b, 0, y, x] = FE_PLANT[i % 9]
            flow[b, 1, y, x] = FE_PLANT[(i + 4) % 9]
            i += 1
    coords = grid(B, H, W) + flow
    flow = coords - grid(B, H, W)  # what the kernel sees: exact fp32 arithmetic on both sides
    w = 0.1 * torch.randn(49, 2, Cout, generator=g)
    w[24, 0, 0], w[24, 1, 1], w[0, 0, 2], w[48, 1, 3] = 1.0, 2.0 ** -10, 0.0, 1.0
    w[3, :, Cout - 1] = 0.0
    bias = torch.randn(Cout, generator=g)
    return coords, flow, w, bias


def fe_conv_weight(w):
    """[49][2][Cout] (tap = 7 ky + kx) -> conv2d's (Cout, 2, 7, 7)."""
    return w.reshape(7, 7, 2, -1).permute(3, 2, 0, 1)


def fe_oracle(flow, w, bias):
    """(pre-activation, A): conv7x7(flow, w) + bias and conv7x7(|flow|, |w|), fp64 NHWC."""
    cw = fe_conv_weight(w.double())
    pre = F.conv2d(flow.double(), cw, bias.double(), padding=3)
    A = F.conv2d(flow.double().abs(), cw.abs(), None, padding=3)
    return pre.permute(0, 2, 3, 1), A.permute(0, 2, 3, 1)


def fe_bound(pre, A):
    """2^-16 A for the split products and the fp32 accumulation, plus the one
    fp32 rounding of ``acc + bias`` the kernel does before the ReLU."""
    return 2.0 ** -16 * A + 2.0 ** -24 * pre.abs()


def split_bf16(x):
    hi = x.to(BF16).to(x.dtype)
    lo = (x - hi).to(BF16).to(x.dtype)
    return hi, lo


def fe_emulate(flow, w, products):
    """The kernel's products in exact arithmetic (fp64): both operands split
    into bf16 hi + lo, ``products`` of {"hh", "hl", "lh"} summed."""
    fh, fl = split_bf16(flow.float())
    wh, wl = split_bf16(w.float())
    out = 0.0
    for name, (a, b) in {"hh": (wh, fh), "hl": (wh, fl), "lh": (wl, fh)}.items():
        if name in products:
            out = out + F.conv2d(b.double(), fe_conv_weight(a.double()), None, padding=3)
    return out.permute(0, 2, 3, 1)


def fe_fout_bf16(flow):
    hi, lo = split_bf16(flow.float())
    return (hi + lo).to(BF16)


# ------------------------------------------------------------------ flow head
def fh_conv_weight(w):
    """[2][3][3][Cin] -> conv2d's (2, Cin, 3, 3)."""
    return w.permute(0, 3, 1, 2)


def fh_fwd_oracle(x, w, bias, src):
    """x NHWC (stored values), w [2][3][3][Cin] -> (want, bound), (B,2,H,W) fp64."""
    xd, cw = x.double().permute(0, 3, 1, 2), fh_conv_weight(w.double())
    want = src.double() + F.conv2d(xd, cw, bias.double(), padding=1)
    S = F.conv2d(xd.abs(), cw.abs(), None, padding=1)
    bound = 2.0 ** -18 * S + 2.0 ** -22 * (src.double().abs() + bias.double().abs().view(1, 2, 1, 1) + want.abs())
    return want, bound


def fh_dgrad_oracle(dflow, w, act):
    """(want, bound) NHWC fp64: (act > 0) * conv^T(dflow, w)."""
    cw = fh_conv_weight(w.double())
    m = (act.double() > 0).double()
    full = F.conv_transpose2d(dflow.double(), cw, None, padding=1).permute(0, 2, 3, 1)
    S = F.conv_transpose2d(dflow.double().abs(), cw.abs(), None, padding=1).permute(0, 2, 3, 1)
    return full * m, 2.0 ** -19 * S


def fh_act(B, H, W, C, dtype, g):
    """relu(randn) with +0.0, -0.0, the smallest positive normal and 1e4 planted."""
    a = torch.relu(torch.randn(B, H, W, C, generator=g))
    tiny = torch.finfo(dtype).tiny
    for i, v in enumerate([0.0, -0.0, tiny, 1e4]):
        a[..., i::16][..., ::2] = v  # channels i, i + 32, ...: every lane group meets each value
    a = a.to(dtype)
    assert float(a[0, 0, 0, 2]) == tiny and math.copysign(1.0, float(a[0, 0, 0, 1])) == -1.0
    return a


# ------------------------------------------------------------------ flow_wgrad
def fw_oracle(flow, df, dw0, db0):
    """dw [49][2][C] and db with their bounds' sums S (the op accumulates into
    dw0 / db0, whose magnitude every block's add rounds at)."""
    Bp, _, H, W = flow.shape
    C = dw0.shape[-1]
    d = df.double()[..., :C].reshape(Bp, H * W, C)
    cols = F.unfold(flow.double(), 7, padding=3)  # (Bp, 2 * 49, HW), row = ci * 49 + tap
    dw = torch.einsum("bkp,bpc->kc", cols, d).reshape(2, 49, C).permute(1, 0, 2)
    Sw = torch.einsum("bkp,bpc->kc", cols.abs(), d.abs()).reshape(2, 49, C).permute(1, 0, 2)
    return (dw0.double() + dw, dw0.double().abs() + Sw,
            db0.double() + d.sum((0, 1)), db0.double().abs() + d.abs().sum((0, 1)))


def fw_eps(Bp, H, W):
    nblocks = Bp * ((H + 7) // 8)
    return (8 * W + nblocks + 4) * 2.0 ** -24


# ------------------------------------------------------------------ convex upsample
def cu_inputs(N, H, W, mdtype, seed):
    """flow (30 randn, +-400 on the border) and NHWC logits (3 randn) with the
    planted columns, one coarse pixel each where the image has room: all nine
    equal; one tap +1e4; one tap -1e4; one tap -inf; eight taps -inf; taps
    2^-7 apart around 1 (ties once rounded to bf16)."""
    g = torch.Generator().manual_seed(seed)
    flow = 30.0 * torch.randn(N, 2, H, W, generator=g)
    flow[:, 0, 0, 0], flow[:, 1, H - 1, W - 1] = 400.0, -400.0
    flow[:, 1, 0, W - 1], flow[:, 0, H - 1, 0] = -400.0, 400.0
    m = (3.0 * torch.randn(N, H, W, 9, 64, generator=g))
    P = N * H * W
    flat = m.view(P, 9, 64)
    for i in range(6):
        # a single coarse pixel takes all six plants, in different sub-pixel columns
        p, cols = ((i * 5) % P, slice(None)) if P > 1 else (0, slice(8 * i, 8 * i + 8))
        if i == 0:
            flat[p, :, cols] = 0.75
        elif i == 1:
            flat[p, 4, cols] = 1e4
        elif i == 2:
            flat[p, 2, cols] = -1e4
        elif i == 3:
            flat[p, 7, cols] = -math.inf
        elif i == 4:
            flat[p, :, cols] = -math.inf
            flat[p, 5, cols] = 0.3
        else:
            flat[p, :, cols] = (1.0 + 2.0 ** -7 * torch.arange(9.0)).view(9, 1)
    return flow, m.view(N, H, W, 576).to(mdtype)


def cu_terms(flow, mask):
    N, _, H, W = flow.shape
    p = torch.softmax(mask.double().view(N, H, W, 9, 8, 8), dim=3)
    nb = F.unfold(8.0 * flow.double(), 3, padding=1).view(N, 2, 9, H, W)
    return p, nb


def cu_fwd_oracle(flow, mask):
    """(want, bound) (N,2,8H,8W) fp64; mask NHWC (N,H,W,576), channel 64 k + 8 a + b."""
    N, _, H, W = flow.shape
    p, nb = cu_terms(flow, mask)
    want = torch.einsum("nhwkab,nckhw->nchawb", p, nb).reshape(N, 2, 8 * H, 8 * W)
    S = nb.abs().sum(2)  # (N,2,H,W)
    bound = 2.0 ** -19 * (1.0 + S.repeat_interleave(8, 2).repeat_interleave(8, 3))
    return want, bound


def cu_bwd_oracle(flow, mask, g):
    """Closed form: dm_k = p_k (dp_k - sum_j p_j dp_j), dp_k = sum_c g_c nbr_kc;
    d nbr_kc = sum_ab p_k g_c, folded back (the adjoint of unfold) and x 8.
    Returns (dflow, dflow bound, dmask NHWC, dmask bound)."""
    N, _, H, W = flow.shape
    p, nb = cu_terms(flow, mask)
    gv = g.double().view(N, 2, H, 8, W, 8)
    dp = torch.einsum("nchawb,nckhw->nhwkab", gv, nb)
    dm = p * (dp - (p * dp).sum(3, keepdim=True))
    dm_bound = (2.0 ** -18 * (1.0 + dp.abs().sum(3, keepdim=True))).expand_as(dm)
    dnb = torch.einsum("nhwkab,nchawb->nckhw", p, gv)
    dnb_abs = torch.einsum("nhwkab,nchawb->nckhw", p, gv.abs())
    fold = lambda t: 8.0 * F.fold(t.reshape(N, 18, H * W), (H, W), 3, padding=1)
    return (fold(dnb), 2.0 ** -18 * fold(dnb_abs), dm.reshape(N, H, W, 576), dm_bound.reshape(N, H, W, 576))


# ------------------------------------------------------------------ upflow8 adjoint
def up8_band(W):
    """upflow8_band of csrc/convex_upsample.hip (fp32 ratio, as there)."""
    if W <= 1:
        return 8
    rw = torch.tensor(float(8 * W - 1), dtype=F32) / torch.tensor(float(W - 1), dtype=F32)
    return min(8 * W, int(math.ceil(float(torch.tensor(2.0, dtype=F32) * rw))) + 8)


def up8_cols_lds(W):
    RG = 1 if W >= 256 else 256 // W
    return (up8_band(W) * W + RG * 8 * W) * 4


def up8_largest_w(limit=65536):
    W = 1
    while up8_cols_lds(W + 1) <= limit:
        W += 1
    assert all(up8_cols_lds(w) > limit for w in range(W + 1, W + 64))
    return W


def interp_matrix(n_in, n_out):
    """[n_out, n_in] fp32 weights of 1-D linear interpolation, align_corners=True,
    in upsample_bilinear2d's fp32 source-index arithmetic."""
    scale = torch.tensor(float(n_in - 1), dtype=F32) / (n_out - 1) if n_out > 1 else torch.tensor(0.0)
    src = scale * torch.arange(n_out, dtype=F32)
    i0 = src.long()
    lam = src - i0.float()
    i1 = torch.where(i0 < n_in - 1, i0 + 1, i0)
    m = torch.zeros(n_out, n_in, dtype=F32)
    rows = torch.arange(n_out)
    m[rows, i0] += 1 - lam
    m[rows, i1] += lam
    return m


def up8_oracle(g, ah, aw):
    want = 8.0 * torch.einsum("Ii,ncIJ,Jj->ncij", ah.double(), g.double(), aw.double())
    S = 8.0 * torch.einsum("Ii,ncIJ,Jj->ncij", ah.double().abs(), g.double().abs(), aw.double().abs())
    return want, (up8_band(aw.shape[1]) + 4) * 2.0 ** -23 * S


# ------------------------------------------------------------------ sequence loss
MAX_FLOW = 400.0
BELOW = lambda v: float(torch.nextafter(torch.tensor(v, dtype=F32), torch.tensor(0.0)))
# (du, dv) of the last prediction at the planted EPE pixels and whether fp64 counts
# them under 1 / 3 / 5 px.  One fp32 step in one component of (3, 4) moves the EPE by
# 0.8 * 2^-22, under half an ulp of 5 (2^-22): no fp32 evaluation can see it, so that
# neighbour sits four steps inside (EPE = 5 - 1.6 * 2^-21, which rounds below 5).
EPE_PLANT = [(1.0, 0.0), (BELOW(1.0), 0.0), (0.0, 3.0), (0.0, BELOW(3.0)), (3.0, 4.0), (3.0, 4.0 - 2.0 ** -20),
             (0.0, 0.0)]


def loss_inputs(N, B, H, W, seed, all_invalid=False):
    """preds (N,B,2,H,W), gt, valid: multiples of 2^-10 (pred - gt is exact in
    fp32).  The last prediction differs from gt by odd multiples of 1/8 in both
    components: 64 EPE^2 = 2 (mod 8) while 64, 576 and 1600 = 0 (mod 8), so no
    unplanted pixel comes near a 1 / 3 / 5 px threshold.  Planted pixels follow
    in raster order from pixel 0 as far as the image has room; returns their
    count as well."""
    g = torch.Generator().manual_seed(seed)
    q = lambda t, s=1024.0: torch.round(t * s) / s
    gt = q(20.0 * torch.randn(B, 2, H, W, generator=g))
    preds = q(gt + 20.0 * torch.randn(N, B, 2, H, W, generator=g))
    odd = (2.0 * torch.round(12.0 * torch.randn(B, 2, H, W, generator=g)) + 1.0) / 8.0
    preds[-1] = gt + odd
    valid = (torch.rand(B, H, W, generator=g) > 0.3).float()
    gf, vf, pf = gt.view(B, 2, H * W), valid.view(B, H * W), preds.view(N, B, 2, H * W)
    plants = []
    # |gt| == max_flow exactly (masked), its fp32 neighbour below (kept)
    plants += [("gt", (240.0, 320.0), 1.0), ("gt", (240.0, BELOW(320.0)), 1.0)]
    plants += [("valid", None, 0.5), ("valid", None, BELOW(0.5)), ("valid", None, math.nan)]
    plants += [("epe", d, 1.0) for d in EPE_PLANT]
    n = 0
    if H * W < len(plants):  # no room (the 1 x 1 image): one plain valid pixel per image
        plants, valid[:] = [], 1.0
    for kind, val, v in plants:
        vf[0, n] = v
        if kind == "gt":
            gf[0, 0, n], gf[0, 1, n] = val
            pf[:, 0, :, n] = gf[0, :, n] + 0.125
        elif kind == "epe":
            gf[0, :, n] = 0.0
            pf[-1, 0, 0, n], pf[-1, 0, 1, n] = val
        n += 1
    if all_invalid:
        valid[:] = 0.0
    return preds, gt, valid, n


def loss_oracle(preds, gt, valid, gamma, max_flow=MAX_FLOW):
    """fp64 from the fp32 inputs: (loss, {epe, counts <1/<3/<5, cnt}, ok mask, last-prediction EPE)."""
    p, g = preds.double(), gt.double()
    N, B = p.shape[:2]
    ok = (valid >= 0.5) & (g.pow(2).sum(1).sqrt() < max_flow)  # NaN >= 0.5 is False
    okf = ok[:, None].expand(B, 2, *ok.shape[1:])
    M = g.numel()
    loss = 0.0
    for i in range(N):
        loss = loss + gamma ** (N - 1 - i) * (p[i] - g).abs()[okf].sum() / M
    epe = (p[-1] - g).pow(2).sum(1).sqrt()
    e = epe[ok]
    cnt = int(ok.sum())
    m = {"epe": float(e.sum()) / max(cnt, 1), "cnt": cnt}
    for k in (1, 3, 5):
        m[f"{k}px"] = int((e < k).sum())
    return loss, m, ok, epe


def loss_precondition(epe, ok, nplant):
    """On the oracle alone: off the planted pixels (the first ``nplant`` of image 0)
    no valid pixel's EPE is within 2^-18 (relative) of 1, 3 or 5."""
    rest = torch.ones_like(epe, dtype=torch.bool)
    rest.view(epe.shape[0], -1)[0, :nplant] = False
    e = epe[rest & ok]
    return all(bool(((e - k).abs() > 2.0 ** -18 * k).all()) for k in (1.0, 3.0, 5.0))


def loss_grad_mirror(preds, gt, ok, gamma, gout):
    """The kernel's gradient, bit for bit: go = gout * (1 / M) and the weights
    w_{N-1} = go, w_{i-1} = w_i * gamma, all in fp32; grad = w_i sign(pred - gt) valid."""
    N, B = preds.shape[:2]
    inv_m = torch.tensor(1.0, dtype=F32) / torch.tensor(float(gt.numel()), dtype=F32)
    w = torch.tensor(gout, dtype=F32) * inv_m
    gam = torch.tensor(gamma, dtype=F32)
    out = torch.zeros_like(preds)
    okf = ok[:, None].float()
    for i in range(N - 1, -1, -1):
        out[i] = w * torch.sign(preds[i] - gt) * okf
        w = w * gam
    return out

"""Pure-ATen reference implementations (numerics oracles + export path).

Each function is written from the math of the reference,
not from its code, and is what runs on CPU tensors, under TorchScript tracing
and under ONNX export (only standard ops appear in the traced graph).
The HIP kernels in ``csrc/`` are tested against these.

Conventions (reference core/corr.py:29-60, core/utils/utils.py:57-77):
  * coords are pixel coordinates, channel 0 = x, channel 1 = y;
  * bilinear sampling with align_corners=True semantics and zero padding;
  * the lookup window channel k of a level is (i, j) = divmod(k, 2r+1) with
    dx = i - r, dy = j - r  (x-offset-major);
  * pyramid level l is avg_pool2d(2, 2)^l of the level-0 volume over the
    target dims, i.e. floor-sized (55 -> 27 -> 13 -> 6).
"""
from __future__ import annotations

import math
from typing import List

import torch
import torch.nn.functional as F


def coords_grid(batch: int, ht: int, wd: int, device=None, dtype=torch.float32):
    ys = torch.arange(ht, device=device, dtype=dtype).view(ht, 1).expand(ht, wd)
    xs = torch.arange(wd, device=device, dtype=dtype).view(1, wd).expand(ht, wd)
    grid = torch.stack([xs, ys], dim=0)
    return grid.unsqueeze(0).repeat(batch, 1, 1, 1)


def bilinear_sampler(img, coords, mask: bool = False):
    """Sample ``img`` (N,C,H,W) at pixel coords (N,h,w,2) [x, y]."""
    H, W = img.shape[-2:]
    x, y = coords.split([1, 1], dim=-1)
    gx = 2 * x / (W - 1) - 1
    gy = 2 * y / (H - 1) - 1
    out = F.grid_sample(img, torch.cat([gx, gy], dim=-1), align_corners=True)
    if mask:
        m = (gx > -1) & (gy > -1) & (gx < 1) & (gy < 1)
        return out, m.float()
    return out


def corr_volume(fmap1, fmap2):
    """All-pairs correlation (B, H1*W1, H2, W2) = <f1, f2> / sqrt(C)."""
    B, C, H, W = fmap1.shape
    a = fmap1.reshape(B, C, H * W)
    b = fmap2.reshape(B, C, -1)
    corr = torch.matmul(a.transpose(1, 2), b)
    return corr.reshape(B, H * W, fmap2.shape[2], fmap2.shape[3]) / math.sqrt(C)


def corr_pyramid(fmap1, fmap2, num_levels: int = 4) -> List[torch.Tensor]:
    """Level list, each (B*H1*W1, 1, H2_l, W2_l) like reference core/corr.py:13-27."""
    B, C, H, W = fmap1.shape
    vol = corr_volume(fmap1.float(), fmap2.float())
    lvl = vol.reshape(B * H * W, 1, fmap2.shape[2], fmap2.shape[3])
    pyr = [lvl]
    for _ in range(num_levels - 1):
        lvl = F.avg_pool2d(lvl, 2, stride=2)
        pyr.append(lvl)
    return pyr


def _window_delta(r: int, device, dtype):
    d = torch.arange(-r, r + 1, device=device, dtype=dtype)
    # channel k = (dx + r) * (2r+1) + (dy + r): x-offset-major.
    dx = d.view(-1, 1).expand(2 * r + 1, 2 * r + 1)
    dy = d.view(1, -1).expand(2 * r + 1, 2 * r + 1)
    return torch.stack([dx, dy], dim=-1)  # (2r+1, 2r+1, 2) as [x, y]


def corr_lookup(pyramid: List[torch.Tensor], coords, radius: int):
    """Window lookup -> (B, L*(2r+1)^2, H1, W1) fp32."""
    B, _, H, W = coords.shape
    c = coords.permute(0, 2, 3, 1).reshape(B * H * W, 1, 1, 2)
    delta = _window_delta(radius, coords.device, coords.dtype).reshape(
        1, 2 * radius + 1, 2 * radius + 1, 2)
    outs = []
    for lvl, vol in enumerate(pyramid):
        sampled = bilinear_sampler(vol, c / (2 ** lvl) + delta)
        # sampled: (BHW, 1, 2r+1 [rows of grid = dx], 2r+1 [cols = dy])
        outs.append(sampled.reshape(B, H, W, -1))
    out = torch.cat(outs, dim=-1)
    return out.permute(0, 3, 1, 2).contiguous()


def corr_onthefly(fmap1, fmap2, coords, radius: int, num_levels: int = 4):
    """Memory-efficient correlation oracle: pool fmap2, correlate lazily.

    Uses pyramid[l] == corr(f1, avgpool^l(f2)) (linearity), so no
    HW x HW volume is materialised: for each level and each window tap the
    feature of fmap2 is bilinearly sampled and dotted with fmap1.
    """
    B, C, H, W = fmap1.shape
    delta = _window_delta(radius, coords.device, coords.dtype).reshape(-1, 2)
    outs = []
    f2 = fmap2.float()
    f1 = fmap1.float()
    base = coords.permute(0, 2, 3, 1)  # (B,H,W,2)
    for lvl in range(num_levels):
        if lvl > 0:
            f2 = F.avg_pool2d(f2, 2, stride=2)
        taps = []
        for t in range(delta.shape[0]):
            pos = base / (2 ** lvl) + delta[t]
            g = bilinear_sampler(f2, pos)  # (B,C,H,W)
            taps.append((g * f1).sum(dim=1))
        outs.append(torch.stack(taps, dim=1))
    return torch.cat(outs, dim=1) / math.sqrt(C)


def convex_upsample(flow, mask, factor: int = 8):
    """Convex upsampling (reference core/raft.py:72-83).

    flow (N,2,H,W), mask (N,9*f*f,H,W) -> (N,2,f*H,f*W); softmax over the 9
    taps, 3x3 neighbourhood of ``f * flow`` with zero padding.
    """
    N, _, H, W = flow.shape
    m = torch.softmax(mask.view(N, 1, 9, factor, factor, H, W), dim=2)
    nb = F.unfold(factor * flow, [3, 3], padding=1).view(N, 2, 9, 1, 1, H, W)
    up = torch.sum(m * nb, dim=2)  # (N,2,f,f,H,W)
    return up.permute(0, 1, 4, 2, 5, 3).reshape(N, 2, factor * H, factor * W)


# ConvGRU gate stages (reference core/update.py:16-60; the chain of ops/gru.py),
# channels-last rows (..., C) in the dtype of the inputs: the oracles of
# csrc/gru.hip, one function per kernel.
def gru_gate_zr(zr, h, x):
    """zr = [z_pre | r_pre] -> z, r, rhx = [r * h | x]."""
    hd = h.shape[-1]
    z, r = torch.sigmoid(zr[..., :hd]), torch.sigmoid(zr[..., hd:])
    return z, r, torch.cat([r * h, x], dim=-1)


def gru_gate_q(q, z, h):
    """q_pre -> h' = (1 - z) h + z q~, q~ = tanh(q_pre)."""
    qt = torch.tanh(q)
    return (1 - z) * h + z * qt, qt


def gru_bwd_q(dhn, z, h, qt):
    """d h' -> dq_pre, dz_pre, the direct part of dh."""
    return dhn * z * (1 - qt * qt), dhn * (qt - h) * z * (1 - z), dhn * (1 - z)


def gru_bwd_r(drhx, h, r):
    """d rhx (the q convolution's input gradient) -> dr_pre."""
    return drhx[..., :h.shape[-1]] * h * r * (1 - r)


def gru_bwd_fin(dhd, drhx, r, dhx):
    """dh = dh_direct + d(r h) r + dhx[h part]; dx = drhx[x part] + dhx[x part]."""
    hd = r.shape[-1]
    return dhd + drhx[..., :hd] * r + dhx[..., :hd], drhx[..., hd:] + dhx[..., hd:]


def context_act(cn, hd: int):
    """cnet output -> (tanh(net), relu(inp)) (reference core/raft.py:108-110)."""
    return torch.tanh(cn[..., :hd]), torch.relu(cn[..., hd:])


def context_act_backward(G, hx, inp, hd: int):
    """Gradient rows G = [d h | d inp | ...] -> d cnet, from the saved activations."""
    cd = inp.shape[-1]
    return torch.cat([G[..., :hd] * (1 - hx[..., :hd] ** 2), G[..., hd:hd + cd] * (inp > 0)], dim=-1)


def upflow8(flow, mode: str = "bilinear"):
    size = (8 * flow.shape[2], 8 * flow.shape[3])
    return 8 * F.interpolate(flow, size=size, mode=mode, align_corners=True)


def sequence_loss_terms(preds, gt, valid, gamma: float, max_flow: float = 400.0):
    """Weighted L1 over the sequence (reference train.py:47-60)."""
    mag = torch.sum(gt ** 2, dim=1).sqrt()
    v = (valid >= 0.5) & (mag < max_flow)
    n = len(preds)
    loss = 0.0
    for i, p in enumerate(preds):
        w = gamma ** (n - i - 1)
        loss = loss + w * (v[:, None] * (p - gt).abs()).mean()
    return loss, v


def forward_interpolate(flow, query_chunk: int = 1024):
    """Forward interpolation of a (B,2,H,W) fp32 flow for the video warm start
    (reference core/utils/utils.py:26-54), by the exact rule of
    csrc/forward_interp.hip: sample s of cell (x, y) moves to the fp32 position
    (x + dx[s], y + dy[s]); it is valid iff 0 < x1 < W and 0 < y1 < H; every
    cell takes the flow of the valid sample with the smallest fp32
    d2 = fl(fl(ex*ex) + fl(ey*ey)), the lowest row-major index among equals
    (``argmin`` returns the first minimum); an image without a valid sample
    gives zeros.  Queries go in chunks, so the N x N table never exists."""
    B, _, H, W = flow.shape
    N = H * W
    flow = flow.float()
    ys, xs = torch.meshgrid(torch.arange(H, device=flow.device), torch.arange(W, device=flow.device), indexing="ij")
    gx, gy = xs.reshape(-1).float(), ys.reshape(-1).float()
    inf = torch.tensor(float("inf"), device=flow.device)
    out = torch.zeros_like(flow)
    for b in range(B):
        f = flow[b].reshape(2, N)
        x1, y1 = gx + f[0], gy + f[1]
        ok = (x1 > 0) & (x1 < W) & (y1 > 0) & (y1 < H)
        x1, y1 = torch.where(ok, x1, inf), torch.where(ok, y1, inf)
        idx = []
        for q0 in range(0, N, query_chunk):
            ex = gx[q0:q0 + query_chunk, None] - x1[None]
            ey = gy[q0:q0 + query_chunk, None] - y1[None]
            idx.append(torch.argmin(ex * ex + ey * ey, dim=1))
        got = f[:, torch.cat(idx)].reshape(2, H, W)
        # without a valid sample every distance is +inf and argmin is meaningless
        out[b] = torch.where(ok.any(), got, torch.zeros_like(got))
    return out


def _fb_sample(f, x, y, dtype):
    """S(f, x, y) of csrc/fb_check.hip: f (B,2,H,W), x and y (B,K) fp32 ->
    (u, v), each (B,K) in ``dtype``.  The cell indices and the four weights are
    fp32, as in the kernel; products and sums with the flow are in ``dtype``."""
    B, _, H, W = f.shape
    live = (x > -1) & (x < W) & (y > -1) & (y < H)  # NaN / Inf / huge fail: S = 0
    zero = torch.zeros_like(x)
    xs, ys = torch.where(live, x, zero), torch.where(live, y, zero)
    x0, y0 = torch.floor(xs), torch.floor(ys)
    wx, wy = xs - x0, ys - y0
    ux, uy = 1 - wx, 1 - wy
    xi0, yi0 = x0.long(), y0.long()
    fd = f.to(dtype).reshape(B, 2, H * W)
    acc = torch.zeros(B, 2, x.shape[1], dtype=dtype, device=f.device)
    for dx, dy, w in ((0, 0, ux * uy), (1, 0, wx * uy), (0, 1, ux * wy), (1, 1, wx * wy)):
        xi, yi = xi0 + dx, yi0 + dy
        use = live & (w != 0) & (xi >= 0) & (xi < W) & (yi >= 0) & (yi < H)
        idx = yi.clamp(0, H - 1) * W + xi.clamp(0, W - 1)
        val = fd.gather(2, idx[:, None].expand(B, 2, -1))
        # a tap that is not used is not read: 0 * NaN must not leak in
        acc = acc + torch.where(use[:, None], w.to(dtype)[:, None] * val, torch.zeros_like(val))
    return acc[:, 0], acc[:, 1]


def fb_terms(bw, px, py, u, v, dtype=torch.float32):
    """The terms of the check rule of csrc/fb_check.hip for starts (px, py)
    (B,K) fp32 with forward vectors (u, v) in ``dtype``: (target inside (B,K)
    bool, e2, m2 (B,K) ``dtype``; e2 and m2 mean nothing where not inside)."""
    _, _, H, W = bw.shape
    qx, qy = px + u.float(), py + v.float()  # fp32 sums
    inside = (qx >= 0) & (qx <= W - 1) & (qy >= 0) & (qy <= H - 1)
    bu, bv = _fb_sample(bw, qx, qy, dtype)
    e2 = (u + bu) ** 2 + (v + bv) ** 2
    m2 = u * u + v * v + bu * bu + bv * bv
    return inside, e2, m2


def _fb_check(bw, px, py, u, v, start_ok, alpha1, alpha2, dtype):
    """err (B,K) ``dtype`` and ok (B,K) bool from fb_terms."""
    inside, e2, m2 = fb_terms(bw, px, py, u, v, dtype)
    inside = inside & start_ok
    inf = torch.full_like(e2, float("inf"))
    err = torch.where(inside, e2.sqrt(), inf)
    ok = inside & (e2 <= alpha1 * m2 + alpha2)
    return err, ok


def fb_consistency(flow_fw, flow_bw, alpha1: float = 0.01, alpha2: float = 0.5, dtype=torch.float32):
    """Dense forward-backward check of two (B,2,H,W) fp32 flows by the rule of
    csrc/fb_check.hip: every pixel centre follows its forward vector, reads the
    backward flow where it lands and is ok iff
    |fw + bw(landing)|^2 <= alpha1 * (|fw|^2 + |bw(landing)|^2) + alpha2.
    -> err (B,1,H,W) ``dtype`` (+inf for a target outside the image), ok (B,1,H,W) bool."""
    B, _, H, W = flow_fw.shape
    fw, bw = flow_fw.float(), flow_bw.float()
    ys, xs = torch.meshgrid(torch.arange(H, device=fw.device), torch.arange(W, device=fw.device), indexing="ij")
    px = xs.reshape(1, -1).float().expand(B, -1)
    py = ys.reshape(1, -1).float().expand(B, -1)
    f = fw.to(dtype).reshape(B, 2, H * W)
    err, ok = _fb_check(bw, px, py, f[:, 0], f[:, 1], torch.ones_like(px, dtype=torch.bool), alpha1, alpha2, dtype)
    return err.reshape(B, 1, H, W), ok.reshape(B, 1, H, W)


def fb_track_points(flow_fw, flow_bw, points, alpha1: float = 0.01, alpha2: float = 0.5, dtype=torch.float32):
    """Point form: points (B,N,2) xy fp32 -> (points + S(fw, points) (B,N,2)
    ``dtype``, err (B,N) ``dtype``, ok (B,N) bool).  A start outside
    [0,W-1]x[0,H-1] or non-finite gives ok = 0 and err = +inf; its new position
    is still the zero-padded sample."""
    _, _, H, W = flow_fw.shape
    fw, bw, p = flow_fw.float(), flow_bw.float(), points.float()
    px, py = p[..., 0], p[..., 1]
    u, v = _fb_sample(fw, px, py, dtype)
    start_ok = (px >= 0) & (px <= W - 1) & (py >= 0) & (py <= H - 1)
    err, ok = _fb_check(bw, px, py, u, v, start_ok, alpha1, alpha2, dtype)
    return p.to(dtype) + torch.stack([u, v], dim=-1), err, ok


def multi_flow_track_points(flow_fw, flow_bw, starts, start_score, start_visible, active,
                            alpha1: float = 0.01, alpha2: float = 0.5, track=None):
    """Multi-delta selection by the rule of csrc/multi_flow.hip.  flows
    (K,2,H,W), slot k spanning t-D_k -> t and back; starts (K,N,2), start_score
    (K,N), start_visible (K,N) bool: the tracked state in each slot's start
    frame; active (K,) bool.  Per slot the candidate is
    ``track(flow_fw[k:k+1], flow_bw[k:k+1], starts[k:k+1], alpha1, alpha2)``
    (:func:`fb_track_points` unless given: a GPU caller can pass the HIP op),
    ``s = start_score + err`` and a slot is eligible iff active, start-visible,
    ok and ``s < +inf``.  A point takes the eligible slot of smallest ``s`` (the
    lowest among equals), visible; without one the lowest active slot, not
    visible; without an active slot ``starts[0]`` and ``start_score[0]`` with
    err = +inf.  -> (points (1,N,2), score (1,N), visible (1,N) bool, choice
    (1,N) int32 (-1: none), err (1,N), cand_err (K,N))."""
    track = fb_track_points if track is None else track
    K, N = starts.shape[:2]
    cand, err = [], []
    ok = []
    for k in range(K):
        c, e, o = track(flow_fw[k:k + 1], flow_bw[k:k + 1], starts[k:k + 1], alpha1, alpha2)
        cand.append(c[0])
        err.append(e[0])
        ok.append(o[0])
    cand, err, ok = torch.stack(cand), torch.stack(err), torch.stack(ok)  # (K,N,2), (K,N), (K,N)
    score = start_score + err
    act = active.view(K, 1).expand(K, N)
    inf = torch.full_like(score, float("inf"))
    elig = act & start_visible & ok & (score < inf)
    # argmin returns the first minimum: the lowest slot among equals
    best = torch.argmin(torch.where(elig, score, inf), dim=0)
    first = torch.argmax(act.to(torch.uint8), dim=0)  # the lowest active slot
    any_elig, any_act = elig.any(dim=0), act.any(dim=0)
    pick = torch.where(any_elig, best, first)  # 0 without an active slot
    g = pick.view(1, N)
    none = ~any_act
    points = torch.where(none.view(N, 1), starts[0], cand.gather(0, g.view(1, N, 1).expand(1, N, 2))[0])
    out_score = torch.where(none, start_score[0], score.gather(0, g)[0])
    out_err = torch.where(none, inf[0], err.gather(0, g)[0])
    choice = torch.where(none, torch.full_like(pick, -1), pick).to(torch.int32)
    return points[None], out_score[None], any_elig[None], choice[None], out_err[None], err


def feature_ring_step(ring_f, ring_c, f_new, c_new, idx, x, ctx):
    """The put-then-gather of csrc/feat_ring.hip, in place, from ATen index
    ops.  ring_f (R,h,w,C), ring_c (R,h,w,Cc), f_new (1,h,w,C), c_new
    (1,h,w,Cc); idx (K+1,) int32 on the tensors' device: K source rows, then
    the row to write, each clamped to [0, R-1]; x (3K,h,w,C), ctx (2K,h,w,Cc):
      ring_f[dst] = f_new, ring_c[dst] = c_new
      x[k] = ring_f[src[k]], x[K+k] = f_new, x[2K+k] = x[k]
      ctx[k] = ring_c[src[k]], ctx[K+k] = c_new
    A source equal to dst sees the new features.  No host synchronisation."""
    R, K = ring_f.shape[0], idx.shape[0] - 1
    i = idx.long().clamp(0, R - 1)
    src, dst = i[:K], i[K:]
    ring_f.index_copy_(0, dst, f_new)
    ring_c.index_copy_(0, dst, c_new)
    x[:K] = ring_f.index_select(0, src)
    x[K:2 * K] = f_new
    x[2 * K:] = x[:K]
    ctx[:K] = ring_c.index_select(0, src)
    ctx[K:] = c_new


def dense_multi_flow_step(flow_fw, flow_bw, ring_pos, ring_score, idx, active, alpha1: float = 0.01,
                          alpha2: float = 0.5, track=None):
    """The dense step of csrc/dense_flow.hip as the point form at every pixel.
    flows (K,2,H,W); ring_pos (R,2,H,W), ring_score (R,H,W): the planar state
    ring, changed in place; idx (K+1,) int32 on the tensors' device: K source
    rows, then the row to write, each clamped to [0, R-1]; active (K,) bool.
    The state of row ``src[k]`` is gathered into the (K,N,2) / (K,N) inputs of
    :func:`multi_flow_track_points`, N = H*W, with ``start_visible =
    start_score < +inf`` (a stored score is finite iff the pixel was visible);
    a slot whose source is the row written counts as inactive; the score of a
    pixel that is not visible becomes +inf; the positions and scores go to row
    ``dst``.  -> (pos (1,2,H,W), score (1,1,H,W), visible (1,1,H,W) bool,
    choice (1,1,H,W) int32, fb_err (1,1,H,W), cand_err (K,H,W)).  No host
    synchronisation."""
    K, _, H, W = flow_fw.shape
    R, N = ring_pos.shape[0], H * W
    i = idx.long().clamp(0, R - 1)
    src, dst = i[:K], i[K:]
    starts = ring_pos.index_select(0, src).reshape(K, 2, N).transpose(1, 2).contiguous()
    start_score = ring_score.index_select(0, src).reshape(K, N)
    inf = torch.full_like(start_score[:1], float("inf"))
    pts, score, vis, choice, err, cand = multi_flow_track_points(
        flow_fw, flow_bw, starts, start_score, start_score < inf, active & (src != dst), alpha1, alpha2, track=track)
    score = torch.where(vis, score, inf)
    pos = pts.transpose(1, 2).reshape(1, 2, H, W)
    score = score.reshape(1, 1, H, W)
    ring_pos.index_copy_(0, dst, pos)
    ring_score.index_copy_(0, dst, score[0])
    return (pos, score, vis.reshape(1, 1, H, W), choice.reshape(1, 1, H, W), err.reshape(1, 1, H, W),
            cand.reshape(K, H, W))


def dense_query(pos, score, points):
    """Read a dense track field at points of the anchor frame.  pos (1,2,H,W),
    score (1,1,H,W) (+inf: not visible), points (1,N,2) xy -> (positions
    (1,N,2), visible (1,N) bool, score (1,N)).  For a point inside
    [0,W-1]x[0,H-1] the position is the bilinear sample of the two planes by
    the sampling rule S of csrc/fb_device.h (at an integer point: that pixel's
    stored position, bit for bit), visible the AND and score the max over the
    taps of non-zero weight.  A point outside the image or non-finite comes
    back unchanged, not visible, with score +inf."""
    _, _, H, W = pos.shape
    p = points.float()
    x, y = p[..., 0], p[..., 1]
    inside = (x >= 0) & (x <= W - 1) & (y >= 0) & (y <= H - 1)  # NaN fails
    zero = torch.zeros_like(x)
    xs, ys = torch.where(inside, x, zero), torch.where(inside, y, zero)
    u, v = _fb_sample(pos.float(), xs, ys, torch.float32)
    out = torch.where(inside[..., None], torch.stack([u, v], dim=-1), p)
    x0, y0 = torch.floor(xs), torch.floor(ys)
    wx, wy = xs - x0, ys - y0
    ux, uy = 1 - wx, 1 - wy
    xi0, yi0 = x0.long(), y0.long()
    flat = score.float().reshape(1, H * W)
    worst = torch.full_like(x, float("-inf"))
    for dx, dy, w in ((0, 0, ux * uy), (1, 0, wx * uy), (0, 1, ux * wy), (1, 1, wx * wy)):
        xi, yi = xi0 + dx, yi0 + dy
        use = (w != 0) & (xi < W) & (yi < H)
        val = flat.gather(1, yi.clamp(0, H - 1) * W + xi.clamp(0, W - 1))
        worst = torch.where(use, torch.maximum(worst, val), worst)
    inf = torch.full_like(x, float("inf"))
    worst = torch.where(inside, worst, inf)
    return out, worst < inf, worst


def dense_compose(base_pos, base_score, pos, score, delta, fb_err):
    """Compose two dense track fields: ``base`` maps anchor a -> frame r, the
    inner field (``pos``, ``score``, ``delta``, ``fb_err``, as
    DenseMultiFlowTracker publishes them) maps r -> t; the result maps a -> t,
    indexed by the pixels of a.  This docstring is the rule.  base_pos, pos
    (1,2,H,W); base_score, score, fb_err (1,1,H,W); delta (1,1,H,W) int32.

    With ``p, q_vis, q_score = dense_query(pos, score, base_pos as points)``:
    ``pos_c = p`` (a base position outside the inner frame or non-finite comes
    back unchanged); ``s = base_score + q_score`` (scores add as the tracker's
    do: start score + fb_err); ``visible_c = q_vis & (s < +inf)`` (NaN fails,
    -inf + inf fails); ``score_c = s`` where visible, else +inf, so that a
    stored score is finite iff the pixel is visible; ``delta_c`` and
    ``fb_err_c`` are the inner ``delta`` and ``fb_err`` at the pixel
    ``(round x, round y)`` of the base position, halves to even (the splat's
    class-0 cell), where visible, else -1 and +inf.
    -> (pos_c (1,2,H,W), score_c (1,1,H,W), visible_c (1,1,H,W) bool, delta_c
    (1,1,H,W) int32, fb_err_c (1,1,H,W)).  No host synchronisation."""
    _, _, H, W = pos.shape
    N = H * W
    bp = base_pos.float().reshape(1, 2, N).transpose(1, 2)
    p, q_vis, q_score = dense_query(pos, score, bp)
    s = base_score.float().reshape(1, N) + q_score
    inf = torch.full_like(s, float("inf"))
    vis = q_vis & (s < inf)
    score_c = torch.where(vis, s, inf)
    x, y = bp[..., 0], bp[..., 1]
    zero = torch.zeros_like(x)
    # visible: the base position is inside the frame, so the rounded one is a pixel; before any int conversion
    cell = torch.round(torch.where(vis, y, zero)).long() * W + torch.round(torch.where(vis, x, zero)).long()
    delta_c = torch.where(vis, delta.reshape(1, N).gather(1, cell), torch.full_like(delta.reshape(1, N), -1))
    err_c = torch.where(vis, fb_err.float().reshape(1, N).gather(1, cell), inf)
    return (p.transpose(1, 2).reshape(1, 2, H, W), score_c.reshape(1, 1, H, W), vis.reshape(1, 1, H, W),
            delta_c.reshape(1, 1, H, W), err_c.reshape(1, 1, H, W))


def backward_warp(image, coords, valid=None, fill=0):
    """Backward warp of an image through a field of positions: every cell of
    the output reads the image bilinearly at its position.  This docstring is
    the rule.  image (1,C,Hs,Ws) fp32 or uint8, of any layout; coords
    (1,2,H,W), xy positions in the image ((H,W) need not be (Hs,Ws)); valid
    (1,1,H,W) bool or None; fill a float (fp32) or an integer in [0,255]
    (uint8) -> (warped (1,C,H,W) of the image's dtype, ok (1,1,H,W) bool).

    ok      ``valid`` (if given) AND inside(x, y): 0 <= x <= Ws-1 and
            0 <= y <= Hs-1, decided on the floats (NaN, infinities, 1e30 fail).
    taps    (floor x + {0,1}, floor y + {0,1}) in the order (0,0), (1,0),
            (0,1), (1,1); a weight is one fp32 product of (1 - wx | wx) and
            (1 - wy | wy).  A tap of weight 0, or at column Ws or row Hs, is
            never read: a NaN or an infinity of the image cannot pass through
            a weight of 0.
    sample  per channel u = 0; u = u + w * f[i] per tap read, every product
            and every sum rounded once (no FMA); a uint8 value is converted to
            fp32 first, exactly.  At an integer point this is the stored value
            (a stored -0.0 reads as +0.0: 0 + -0 is +0).
    store   fp32: u.  uint8: clamp(rint(u), 0, 255), halves to even.  A cell
            that is not ok holds ``fill`` in every channel.

    The sampling rule is dense_query's (csrc/query_device.h).  No host
    synchronisation."""
    _, C, Hs, Ws = image.shape
    _, _, H, W = coords.shape
    N = H * W
    p = coords.float().reshape(2, N)
    x, y = p[0], p[1]
    inside = (x >= 0) & (x <= Ws - 1) & (y >= 0) & (y <= Hs - 1)  # NaN fails
    ok = inside if valid is None else inside & valid.reshape(N)
    zero = torch.zeros_like(x)
    xs, ys = torch.where(inside, x, zero), torch.where(inside, y, zero)  # before any int conversion
    x0, y0 = torch.floor(xs), torch.floor(ys)
    wx, wy = xs - x0, ys - y0
    ux, uy = 1 - wx, 1 - wy
    xi0, yi0 = x0.long(), y0.long()
    flat = image.reshape(C, Hs * Ws)
    u = torch.zeros(C, N, dtype=torch.float32, device=image.device)
    for dx, dy, w in ((0, 0, ux * uy), (1, 0, wx * uy), (0, 1, ux * wy), (1, 1, wx * wy)):
        xi, yi = xi0 + dx, yi0 + dy
        use = (w != 0) & (xi < Ws) & (yi < Hs)
        val = flat.index_select(1, yi.clamp(0, Hs - 1) * Ws + xi.clamp(0, Ws - 1)).float()
        u = torch.where(use, u + w * val, u)
    if image.dtype == torch.uint8:
        u = torch.round(u).clamp(0, 255).to(torch.uint8)
    warped = torch.where(ok, u, torch.full_like(u, fill))
    return warped.reshape(1, C, H, W), ok.reshape(1, 1, H, W)


_SPLAT_HOLE = torch.iinfo(torch.int64).max


def forward_splat(pos, score, values=None, footprint: int = 2, fill: float = 0.0):
    """Forward splatting of the anchor frame into the frame a dense track
    field points to: for every cell of the target frame, which anchor pixel
    sits there.  This docstring is the rule.  pos (1,2,H,W), channel 0
    = x; score (1,1,H,W), finite iff visible (as DenseMultiFlowTracker stores
    it); values (1,C,H,W) or None.

    Anchor pixel n = y*W + x is a source iff ``0 <= score < +inf`` and
    ``-1 < x' < W and -1 < y' < H`` (NaN fails both).  Its nearest cell is
    ``(round(x'), round(y'))``, halves to even.  With ``footprint=1`` it offers
    itself to that cell; with ``footprint=2`` to the up-to-four cells
    ``(floor x' + {0,1}, floor y' + {0,1})`` whose bilinear weight (the fp32
    products of S in csrc/fb_device.h) is not 0: the nearest cell in class 0,
    the others in class 1.  Offers to cells outside the image are dropped.  A
    cell takes the offer of smallest ``(class, score + 0.0, n)``; a cell
    without an offer is a hole.  The minimum is taken over one packed integer
    per offer, (class, the score's bits, n) from the top, so it does not depend
    on any order.

    -> (src_index (1,1,H,W) int32, -1 at holes; covered (1,1,H,W) bool;
    inv_pos (1,2,H,W): ``grid(n) + (cell - pos[n])``, the cell's position in
    the anchor frame, NaN at holes; out (1,C,H,W): ``values[:, n]``, ``fill``
    at holes, None without values).  No host synchronisation."""
    if footprint not in (1, 2):
        raise ValueError(f"forward_splat: footprint must be 1 or 2, got {footprint}")
    _, _, H, W = pos.shape
    N, dev = H * W, pos.device
    x, y = pos[0, 0].reshape(N).float(), pos[0, 1].reshape(N).float()
    s = score.reshape(N).float() + 0.0  # -0 -> +0
    inf = torch.full_like(s, float("inf"))
    src = (s >= 0) & (s < inf) & (x > -1) & (x < W) & (y > -1) & (y < H)  # before any int conversion
    zero = torch.zeros_like(x)
    xs, ys = torch.where(src, x, zero), torch.where(src, y, zero)
    nx, ny = torch.round(xs).long(), torch.round(ys).long()
    n = torch.arange(N, device=dev)
    # score >= 0: its bit pattern is ordered like the float and bit 31 is free
    base = (torch.where(src, s, zero).view(torch.int32).long() << 31) | n
    if footprint == 1:
        offers = [(nx, ny, src, base)]
    else:
        x0, y0 = torch.floor(xs), torch.floor(ys)
        wx, wy = xs - x0, ys - y0
        ux, uy = 1 - wx, 1 - wy
        xi0, yi0 = x0.long(), y0.long()
        offers = []
        for dx, dy, w in ((0, 0, ux * uy), (1, 0, wx * uy), (0, 1, ux * wy), (1, 1, wx * wy)):
            xi, yi = xi0 + dx, yi0 + dy
            far = ((xi != nx) | (yi != ny)).long()
            offers.append((xi, yi, src & (w != 0), base | (far << 62)))
    keys = torch.full((N,), _SPLAT_HOLE, dtype=torch.int64, device=dev)
    hole = torch.full_like(base, _SPLAT_HOLE)
    for xi, yi, use, key in offers:
        use = use & (xi >= 0) & (xi < W) & (yi >= 0) & (yi < H)
        cell = yi.clamp(0, H - 1) * W + xi.clamp(0, W - 1)
        keys.scatter_reduce_(0, cell, torch.where(use, key, hole), "amin")  # an offer not made: the hole key
    covered = keys != _SPLAT_HOLE
    win = torch.where(covered, keys & (2 ** 31 - 1), torch.zeros_like(keys))
    src_index = torch.where(covered, win, torch.full_like(win, -1)).to(torch.int32)
    cy = torch.div(n, W, rounding_mode="floor")
    gx, gy = (n - cy * W).float(), cy.float()
    nan = torch.full_like(x, float("nan"))
    inv = torch.stack([torch.where(covered, gx[win] + (gx - x[win]), nan),
                       torch.where(covered, gy[win] + (gy - y[win]), nan)])
    out = None
    if values is not None:
        v = values.float().reshape(-1, N)
        out = torch.where(covered, v[:, win], torch.full_like(v[:, :1], fill)).reshape(1, -1, H, W)
    return src_index.reshape(1, 1, H, W), covered.reshape(1, 1, H, W), inv.reshape(1, 2, H, W), out


_INPAINT_NONE = torch.iinfo(torch.int64).max
INPAINT_MAX_SIDE = 32767


def _shift(t, d, axis, pad):
    """s with s[i] = t[i - d] along ``axis`` of a 2-d tensor, ``pad`` where i - d is outside."""
    out = torch.full_like(t, pad)
    n = t.shape[axis]
    if abs(d) >= n:
        return out
    src = slice(0, n - d) if d >= 0 else slice(-d, n)
    dst = slice(d, n) if d >= 0 else slice(0, n + d)
    if axis == 0:
        out[dst] = t[src]
    else:
        out[:, dst] = t[:, src]
    return out


def splat_inpaint(src_index, pos, inv_pos, values=None, max_dist: int = 8, fill: float = 0.0):
    """In-paint the holes of a forward splat from the nearest covered cell.
    This docstring is the rule.  src_index (1,1,H,W) int32 and inv_pos
    (1,2,H,W) as :func:`forward_splat` returns them; pos (1,2,H,W), the field
    that was splatted; values (1,C,H,W) or None; max_dist R, an integer in
    [0, 32767]; H, W in [2, 32767], so that every d2 and H*W stay below 2^31.

    An entry s of src_index is read as ``clamp(s, -1, N-1)``, N = H*W: below 0
    a hole, N and above the last anchor pixel.  A cell c = y*W + x is covered
    iff ``s[c] >= 0``.  Every cell takes as donor the covered cell c' of
    smallest key ``(d2 << 31) | c'`` with ``d2 = (x-x')^2 + (y-y')^2``: the
    nearest covered cell in exact integer Euclidean distance, among equals the
    lowest cell index.  The donor counts only if ``d2 <= R*R``.  A covered cell
    is its own donor (d2 = 0); a hole without a covered cell within R stays a
    hole.  With R = 0 the input comes back unchanged.

    -> (src_index (1,1,H,W) int32: ``s[donor]``, -1 where there is none; donor
    (1,1,H,W) int32: the donor's cell index, or -1; dist2 (1,1,H,W) int32: its
    d2, or -1; inv_pos (1,2,H,W) fp32: at covered cells the input's value bit
    for bit, at filled cells ``grid(win) + (cell - pos[win])`` per axis with
    ``win = s[donor]`` (the donor's anchor pixel extended rigidly to this cell,
    the two fp32 operations of splat::inverse in csrc/splat_device.h), NaN where
    there is none; out (1,C,H,W) fp32: ``values[:, win]``, ``fill`` where there
    is none, None without values).

    The search is separable and exact.  Column pass: per cell the nearest
    covered row y' of its own column with |y - y'| <= R, y - d before y + d
    (the lower cell index), -1 if none.  Row pass: the donor of (x, y) is the
    smallest key over x' in [x-R, x+R] of column x''s row at y, with d2 <= R*R.
    A column's nearest row minimises d2 for every x and its tie went to the
    lower index, so the minimum over the columns' keys is the minimum over all
    covered cells.  Everything is integers but inverse's two fp32 operations,
    and nothing depends on a visiting order.  O(R) whole-tensor shifts on int64
    keys; no host synchronisation."""
    _, _, H, W = src_index.shape
    R = int(max_dist)
    if not (2 <= H <= INPAINT_MAX_SIDE and 2 <= W <= INPAINT_MAX_SIDE):
        raise ValueError(f"splat_inpaint: H, W in [2, {INPAINT_MAX_SIDE}] expected, got {(H, W)}")
    if not 0 <= R <= INPAINT_MAX_SIDE:
        raise ValueError(f"splat_inpaint: max_dist must be in [0, {INPAINT_MAX_SIDE}], got {max_dist}")
    N, dev = H * W, src_index.device
    s = src_index.reshape(H, W).long().clamp(-1, N - 1)
    cov = s >= 0
    ys = torch.arange(H, device=dev).view(H, 1).expand(H, W)
    xs = torch.arange(W, device=dev).view(1, W).expand(H, W)
    # column pass: the first hit in the order y, y-1, y+1, y-2, ...
    col = torch.where(cov, ys, torch.full_like(ys, -1))
    for d in range(1, min(R, H - 1) + 1):
        for sign in (1, -1):  # sign = 1: the row y - d
            hit = _shift(cov, sign * d, 0, False) & (col < 0)
            col = torch.where(hit, ys - sign * d, col)
    # row pass
    none = torch.full((H, W), _INPAINT_NONE, dtype=torch.int64, device=dev)
    best = none.clone()
    for dx in range(0, min(R, W - 1) + 1):
        for sign in ((1, -1) if dx else (1,)):  # sign = 1: the column x - dx
            yc = _shift(col, sign * dx, 1, -1)
            dy = ys - yc
            d2 = dx * dx + dy * dy
            key = (d2 << 31) | (yc * W + (xs - sign * dx))
            best = torch.minimum(best, torch.where((yc >= 0) & (d2 <= R * R), key, none))
    has = best != _INPAINT_NONE
    zero = torch.zeros_like(best)
    donor = torch.where(has, best & (2 ** 31 - 1), zero).reshape(N)
    dist2 = torch.where(has, best >> 31, zero - 1).reshape(N)
    has = has.reshape(N)
    win = s.reshape(N)[donor]  # >= 0 where has: a donor is covered
    win = torch.where(has, win, zero.reshape(N))
    src_out = torch.where(has, win, torch.full_like(win, -1)).to(torch.int32)
    n = torch.arange(N, device=dev)
    cy = torch.div(n, W, rounding_mode="floor")
    gx, gy = (n - cy * W).float(), cy.float()
    wy = torch.div(win, W, rounding_mode="floor")
    wx = win - wy * W
    x, y = pos[0, 0].reshape(N).float(), pos[0, 1].reshape(N).float()
    nan = torch.full_like(x, float("nan"))
    own = cov.reshape(N)
    given = inv_pos.reshape(2, N).float()
    inv = torch.stack([torch.where(own, given[0], torch.where(has, wx.float() + (gx - x[win]), nan)),
                       torch.where(own, given[1], torch.where(has, wy.float() + (gy - y[win]), nan))])
    out = None
    if values is not None:
        v = values.float().reshape(-1, N)
        out = torch.where(has, v[:, win], torch.full_like(v[:, :1], fill)).reshape(1, -1, H, W)
    donor = torch.where(has, donor, torch.full_like(donor, -1)).to(torch.int32)
    return (src_out.reshape(1, 1, H, W), donor.reshape(1, 1, H, W), dist2.to(torch.int32).reshape(1, 1, H, W),
            inv.reshape(1, 2, H, W), out)

"""Inputs shared by the dense_compose / dense_query tests (not a test module):
inner fields taken from forward_splat_cases and dense_flow_cases with their lost
pixels, base fields that put a query on every kind of place, the oracle's
answers computed once, and a scalar brute force of the rule in fp32."""
import functools

import numpy as np
import torch

import dense_flow_cases as D
import forward_splat_cases as S
from fb_check_cases import INF, NAN, same  # noqa: F401

from raft_stir_amd.ops import reference

NAMES = ("pos", "score", "visible", "delta", "fb_err")
QUERY_NAMES = ("positions", "visible", "score")

# 2x2, an odd one, and one whose plane (1680) is no multiple of the block size (256)
SHAPES = [(2, 2), (7, 9), (24, 70)]
INNER = ("mixed", "ring", "identity")
BASES = ("integers", "smooth", "edge")
# (inner, base) on which a good part of the pixels stays visible: the comparison is not mostly about holes
ORDINARY = [("mixed", "smooth"), ("ring", "smooth"), ("identity", "smooth"), ("identity", "integers")]
BIG = 3e38       # finite; BIG + BIG overflows
DENORMAL = 1e-40
F32 = np.float32


@functools.lru_cache(maxsize=None)
def inner(name, H, W):
    """(pos (1,2,H,W), score (1,1,H,W), delta (1,1,H,W) int32, fb_err
    (1,1,H,W)) on the CPU; shared, so never changed in place.  The scores keep
    the source's +inf, NaN and denormal entries; every 13th pixel of the
    non-trivial fields gets BIG, for the sums that overflow."""
    n = H * W
    g = torch.Generator().manual_seed(5200 + n)
    if name == "mixed":
        pos, score = S.field("mixed", H, W)
    elif name == "ring":
        D.FB.AMP.setdefault((H, W), 4)  # the flows' amplitude, which this field does not use
        _, _, ring_pos, ring_score, _ = D.step_inputs(2, H, W)
        pos, score = ring_pos[:1], ring_score[:1, None]
    elif name == "identity":
        pos, score = S.field("identity", H, W)
    else:
        raise KeyError(name)
    pos, score = pos.clone().contiguous(), score.clone().contiguous()
    if name != "identity":
        score.view(n)[5::13] = BIG
    spans = torch.tensor([-1, 0, 1, 2, 4, 8], dtype=torch.int32)
    delta = spans[torch.randint(0, len(spans), (1, 1, H, W), generator=g)]
    err = torch.rand(1, 1, H, W, generator=g) * 3
    err = torch.where(score < INF, err, torch.full_like(err, INF))
    err.view(n)[3::17] = NAN
    return pos, score, delta.contiguous(), err.contiguous()


def edge_points(H, W):
    """Base positions set in fixed places of the edge field: the borders
    exactly, where the tap at column W / row H has weight 0 and is not read;
    the floats next to them outside; -0.0 and everything non-finite or huge."""
    lo = float(np.nextafter(F32(0), F32(-1)))            # the largest float below 0 (a denormal)
    hx = float(np.nextafter(F32(W - 1), F32(np.inf)))
    hy = float(np.nextafter(F32(H - 1), F32(np.inf)))
    return [(0.0, 0.0), (W - 1.0, 0.0), (0.0, H - 1.0), (W - 1.0, H - 1.0), (W - 1.0, 0.5), (0.5, H - 1.0),
            (0.25, 0.0), (0.0, 0.75), (lo, 0.0), (0.0, lo), (hx, 0.0), (0.0, hy), (hx, hy), (-0.0, -0.0),
            (-0.0, H - 1.0), (NAN, 0.0), (1.0, NAN), (INF, 0.0), (0.0, -INF), (-INF, INF), (1e30, 1.0), (1.0, -1e30),
            (-1.0, 0.0), (float(W), 0.0), (0.5, 0.5),
            (5.0, 0.0),  # entry 25 gets base score BIG and pixel 5 holds BIG in inner(): a sum that overflows
            (W - 1.5, H - 1.5)]


@functools.lru_cache(maxsize=None)
def base(name, H, W):
    """(base_pos (1,2,H,W), base_score (1,1,H,W)) on the CPU; shared."""
    n = H * W
    g = torch.Generator().manual_seed(6100 + n)
    grid = reference.coords_grid(1, H, W).contiguous()
    if name == "integers":
        # every integer point once, in another order than the grid's
        perm = torch.randperm(n, generator=g)
        return grid.reshape(1, 2, n)[:, :, perm].reshape(1, 2, H, W).contiguous(), torch.zeros(1, 1, H, W)
    mild = torch.tensor([0.0, 0.0, 0.0, 0.0, 0.0, 0.5, 1.0, 2.0, DENORMAL, INF])
    if name == "smooth":
        pos = grid + (torch.rand(1, 2, H, W, generator=g) * 2 - 1)
        snap = torch.rand(1, 2, H, W, generator=g) < 0.4  # integers and exact halves
        pos = torch.where(snap, torch.round(pos * 2) / 2, pos)
        pos[:, 0].clamp_(0, W - 1)
        pos[:, 1].clamp_(0, H - 1)
        score = mild[torch.randint(0, len(mild), (1, 1, H, W), generator=g)]
        return pos.contiguous(), score.contiguous()
    if name == "edge":
        pos = grid + (torch.rand(1, 2, H, W, generator=g) * 4 - 2)  # a part leaves the frame
        snap = torch.rand(1, 2, H, W, generator=g) < 0.3
        pos = torch.where(snap, torch.round(pos * 2) / 2, pos)
        harsh = torch.tensor([0.0, 0.0, 0.5, 2.0, DENORMAL, BIG, BIG, -1.0, INF, -INF, NAN])
        score = harsh[torch.randint(0, len(harsh), (1, 1, H, W), generator=g)]
        fx, fy, fs = pos[0, 0].view(n), pos[0, 1].view(n), score.view(n)
        pts = edge_points(H, W)
        for j, (x, y) in enumerate(pts):
            k = (j * 37 + 5) % n if n > len(pts) else j % n
            fx[k], fy[k] = x, y
            fs[k] = (0.0, BIG, DENORMAL)[j % 3]
        return pos.contiguous(), score.contiguous()
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def expected(inner_name, base_name, H, W):
    """The oracle's answer on the CPU, computed once."""
    return reference.dense_compose(*base(base_name, H, W), *inner(inner_name, H, W))


def points_of(base_name, H, W, N):
    """(1,N,2): the base field's positions as interleaved points, repeated or cut to N."""
    p = base(base_name, H, W)[0].reshape(2, H * W).t()
    reps = -(-max(N, 1) // p.shape[0])
    return p.repeat(reps, 1)[:N][None].contiguous()


@functools.lru_cache(maxsize=None)
def expected_query(inner_name, base_name, H, W, N):
    pos, score, _, _ = inner(inner_name, H, W)
    return reference.dense_query(pos, score, points_of(base_name, H, W, N))


# ------------------------------------------------------------- the brute force
def _worse(m, s):
    if np.isnan(m) or np.isnan(s):
        return F32(np.nan)
    return s if s > m else m


def brute_query(px, py, sc, H, W, x, y):
    """One point by the rule, every operation on numpy fp32 scalars (one
    rounding each) -> (ox, oy, visible, score)."""
    x, y = F32(x), F32(y)
    if not (x >= 0 and x <= F32(W - 1) and y >= 0 and y <= F32(H - 1)):
        return x, y, False, F32(np.inf)
    xf, yf = np.floor(x), np.floor(y)
    wx, wy = F32(x - xf), F32(y - yf)
    ux, uy = F32(F32(1) - wx), F32(F32(1) - wy)
    x0, y0 = int(xf), int(yf)
    u, v, m = F32(0), F32(0), F32(-np.inf)
    for dx, dy, w in ((0, 0, F32(ux * uy)), (1, 0, F32(wx * uy)), (0, 1, F32(ux * wy)), (1, 1, F32(wx * wy))):
        xi, yi = x0 + dx, y0 + dy
        if w != 0 and xi < W and yi < H:
            u = F32(u + F32(w * px[yi, xi]))
            v = F32(v + F32(w * py[yi, xi]))
            m = _worse(m, sc[yi, xi])
    return u, v, bool(m < np.inf), m


def brute_compose(base_pos, base_score, pos, score, delta, fb_err):
    """reference.dense_compose by one loop per pixel and four taps."""
    _, _, H, W = pos.shape
    bx, by, bs = base_pos[0, 0].numpy(), base_pos[0, 1].numpy(), base_score[0, 0].numpy()
    px, py, sc = pos[0, 0].numpy(), pos[0, 1].numpy(), score[0, 0].numpy()
    dl, er = delta[0, 0].numpy(), fb_err[0, 0].numpy()
    out_p = np.empty((1, 2, H, W), F32)
    out_s = np.full((1, 1, H, W), np.inf, F32)
    out_v = np.zeros((1, 1, H, W), bool)
    out_d = np.full((1, 1, H, W), -1, np.int32)
    out_e = np.full((1, 1, H, W), np.inf, F32)
    with np.errstate(all="ignore"):
        for r in range(H):
            for c in range(W):
                ox, oy, seen, q = brute_query(px, py, sc, H, W, bx[r, c], by[r, c])
                out_p[0, 0, r, c], out_p[0, 1, r, c] = ox, oy
                s = F32(bs[r, c] + q)
                if seen and s < np.inf:
                    nx, ny = int(np.rint(bx[r, c])), int(np.rint(by[r, c]))
                    out_v[0, 0, r, c] = True
                    out_s[0, 0, r, c] = s
                    out_d[0, 0, r, c] = dl[ny, nx]
                    out_e[0, 0, r, c] = er[ny, nx]
    return tuple(torch.from_numpy(a) for a in (out_p, out_s, out_v, out_d, out_e))


def tap_classes(inner_name, base_name, H, W):
    """What the queries of a case meet, counted from the rule: a NaN and a
    +inf score at a tap that is read and at one of weight 0; base positions
    inside and outside; finite sums that overflow."""
    pos, score, _, _ = inner(inner_name, H, W)
    bp, bs = base(base_name, H, W)
    sc = score[0, 0].numpy()
    out = dict(inside=0, outside=0, nan_read=0, inf_read=0, nan_skipped=0, inf_skipped=0, overflow=0, integer=0)
    with np.errstate(all="ignore"):
        for x, y, b in zip(bp[0, 0].flatten().tolist(), bp[0, 1].flatten().tolist(), bs.flatten().tolist()):
            x, y = F32(x), F32(y)
            if not (x >= 0 and x <= F32(W - 1) and y >= 0 and y <= F32(H - 1)):
                out["outside"] += 1
                continue
            out["inside"] += 1
            x0, y0 = int(np.floor(x)), int(np.floor(y))
            wx, wy = F32(x - np.floor(x)), F32(y - np.floor(y))
            out["integer"] += int(wx == 0 and wy == 0)
            worst = F32(-np.inf)
            for dx, dy, w in ((0, 0, (1 - wx) * (1 - wy)), (1, 0, wx * (1 - wy)), (0, 1, (1 - wx) * wy),
                              (1, 1, wx * wy)):
                xi, yi = x0 + dx, y0 + dy
                if xi >= W or yi >= H:
                    continue
                s = sc[yi, xi]
                kind = "nan" if np.isnan(s) else "inf" if s == np.inf else None
                if kind:
                    out[f"{kind}_{'read' if w != 0 else 'skipped'}"] += 1
                if w != 0:
                    worst = _worse(worst, s)
            if np.isfinite(worst) and np.isfinite(F32(b)) and not np.isfinite(F32(F32(b) + worst)):
                out["overflow"] += 1
    return out

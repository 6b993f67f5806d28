"""Inputs shared by the backward_warp tests (not a test module): named images
of both dtypes, named coordinate fields that put a read on every kind of place,
the oracle's answers computed once, a scalar brute force of the rule in fp32,
and, checked when the module is imported, that the fields meet every class of
the rule (a condition on the inputs, decided with the oracle alone)."""
import functools

import numpy as np
import torch

from fb_check_cases import INF, NAN  # noqa: F401

from raft_stir_amd.ops import reference

F32 = np.float32
DENORMAL = 1e-40
# (output (H, W), source (Hs, Ws)): 2x2 the minimum, 7x9 odd, 24x70 = 1680 cells, no multiple of the block (256);
# sources of the output's size and of another, taller or wider, so that swapped sizes cannot pass
SIZES = [((2, 2), (2, 2)), ((7, 9), (7, 9)), ((7, 9), (5, 11)), ((24, 70), (24, 70)), ((24, 70), (31, 19))]
# for the kernel only (the brute force would take long): 4290 cells, 16 blocks and a partial one
BIG_SIZE = ((33, 130), (33, 130))
SIZES_WITH_BIG = SIZES + [BIG_SIZE]
SIZE_IDS = [f"{h}x{w}from{hs}x{ws}" for (h, w), (hs, ws) in SIZES_WITH_BIG]
IMAGES = {"fp32": ("ramp", "random", "special"), "uint8": ("ramp", "random", "odd")}
FIELDS = ("integers", "smooth", "edge", "identity")
CHANNELS = (1, 3, 4)
FILL = {"fp32": -7.5, "uint8": 200}
DTYPES = {"fp32": torch.float32, "uint8": torch.uint8}
# flat pixels of channel c of the special image (index modulo Hs*Ws), after SPECIAL_AT + c
SPECIAL_AT = 1
SPECIALS = (NAN, INF, -INF, DENORMAL, -0.0, -DENORMAL)


def same(a, b):
    """Bit-equal, the sign of a zero included; NaN equal to NaN."""
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if not a.is_floating_point():
        return bool((a == b).all())
    bits = a.contiguous().view(torch.int32) == b.contiguous().view(torch.int32)
    return bool((bits | ((a != a) & (b != b))).all())


@functools.lru_cache(maxsize=None)
def image(name, dtype, C, Hs, Ws):
    """(1,C,Hs,Ws) on the CPU, contiguous; shared, so never changed in place.
    The image of C channels is the first C channels of the one of 16."""
    if C != 16:
        return image(name, dtype, 16, Hs, Ws)[:, :C].contiguous()
    g = torch.Generator().manual_seed(7300 + Hs * 100 + Ws)
    y, x = torch.meshgrid(torch.arange(Hs), torch.arange(Ws), indexing="ij")
    c = torch.arange(16).view(16, 1, 1)
    if dtype == "uint8":
        if name == "ramp":
            img = (3 * x + 5 * y + 7 * c) % 256
        elif name == "random":
            img = torch.randint(0, 256, (16, Hs, Ws), generator=g)
        elif name == "odd":
            # neighbours differ by 1 along x and by 3 along y: a sample half-way between two is a half
            img = (x + 3 * y + 5 * c) % 256
        else:
            raise KeyError(name)
        return img.to(torch.uint8)[None].contiguous()
    if name == "ramp":
        img = (1000.0 * c + y * Ws + x).float() + 0.25
    elif name == "random":
        img = torch.randn(16, Hs, Ws, generator=g) * 100
    elif name == "special":
        img = torch.randn(16, Hs, Ws, generator=g)
        flat = img.view(16, Hs * Ws)
        for ch in range(16):
            for j, v in enumerate(SPECIALS):
                flat[ch, (SPECIAL_AT + ch + j) % (Hs * Ws)] = v
    else:
        raise KeyError(name)
    return img[None].contiguous()


def edge_points(Hs, Ws):
    """Positions set in fixed places of the edge field: the borders exactly,
    where the tap at column Ws / row Hs has weight 0 and is not read; the
    floats next to them outside; -0.0, halves, denormals and everything
    non-finite or huge."""
    lo = float(np.nextafter(F32(0), F32(-1)))            # the largest float below 0 (a denormal)
    hx = float(np.nextafter(F32(Ws - 1), F32(np.inf)))
    hy = float(np.nextafter(F32(Hs - 1), F32(np.inf)))
    return [(0.0, 0.0), (Ws - 1.0, 0.0), (0.0, Hs - 1.0), (Ws - 1.0, Hs - 1.0), (Ws - 1.0, 0.5), (0.5, Hs - 1.0),
            (0.25, 0.0), (0.0, 0.75), (lo, 0.0), (0.0, lo), (hx, 0.0), (0.0, hy), (hx, hy), (-0.0, -0.0),
            (-0.0, Hs - 1.0), (NAN, 0.0), (1.0, NAN), (INF, 0.0), (0.0, -INF), (-INF, INF), (1e30, 1.0), (1.0, -1e30),
            (-1.0, 0.0), (float(Ws), 0.0), (0.0, float(Hs)), (0.5, 0.5), (DENORMAL, 0.0), (0.0, DENORMAL),
            (DENORMAL, DENORMAL), (Ws - 1.5, Hs - 1.5), (1.0, 0.0), (0.5, 0.0), (0.0, 0.5), (1.0, 1.0)]


@functools.lru_cache(maxsize=None)
def field(name, H, W, Hs, Ws):
    """coords (1,2,H,W) on the CPU, positions in an image of Hs x Ws; shared."""
    n = H * W
    g = torch.Generator().manual_seed(8100 + n + Hs)
    grid = reference.coords_grid(1, H, W).contiguous()
    if name == "identity":
        return grid
    if name == "integers":
        x = torch.randint(0, Ws, (1, 1, H, W), generator=g)
        y = torch.randint(0, Hs, (1, 1, H, W), generator=g)
        return torch.cat([x, y], 1).float().contiguous()
    # the output's grid stretched over the source
    scaled = grid * torch.tensor([(Ws - 1) / (W - 1), (Hs - 1) / (H - 1)]).view(1, 2, 1, 1)
    if name == "smooth":
        pos = scaled + (torch.rand(1, 2, H, W, generator=g) * 2 - 1)
        snap = torch.rand(1, 2, H, W, generator=g) < 0.5  # integers and exact halves
        pos = torch.where(snap, torch.round(pos * 2) / 2, pos)
        pos[:, 0].clamp_(0, Ws - 1)
        pos[:, 1].clamp_(0, Hs - 1)
        return pos.contiguous()
    if name == "edge":
        pos = scaled + (torch.rand(1, 2, H, W, generator=g) * 4 - 2)  # a part leaves the image
        snap = torch.rand(1, 2, H, W, generator=g) < 0.3
        pos = torch.where(snap, torch.round(pos * 2) / 2, pos).contiguous()
        fx, fy = pos[0, 0].view(n), pos[0, 1].view(n)
        pts = edge_points(Hs, Ws)
        for j, (x, y) in enumerate(pts):
            k = (j * 37 + 5) % n if n > 37 * len(pts) else j % n
            fx[k], fy[k] = x, y
        return pos
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def valid(H, W):
    """(1,1,H,W) bool on the CPU: about one cell in five is not valid."""
    g = torch.Generator().manual_seed(9100 + H * W)
    v = torch.rand(1, 1, H, W, generator=g) < 0.8
    v.view(-1)[0] = False   # (0, 0) is inside in every field's source: a cell that is inside and not valid
    v.view(-1)[-1] = True
    return v


@functools.lru_cache(maxsize=None)
def expected(name, dtype, C, size, fname, with_valid, fill=None):
    """The oracle's answer on the CPU, computed once.  size: an index into SIZES_WITH_BIG."""
    (H, W), (Hs, Ws) = SIZES_WITH_BIG[size]
    return reference.backward_warp(image(name, dtype, C, Hs, Ws), field(fname, H, W, Hs, Ws),
                                   valid(H, W) if with_valid else None, FILL[dtype] if fill is None else fill)


def all_cases(big=False):
    """(dtype, image name, size index, field name) of every case; big: with BIG_SIZE."""
    sizes = range(len(SIZES) + bool(big))
    return [(dt, im, s, f) for dt in IMAGES for im in IMAGES[dt] for s in sizes for f in FIELDS]


def case_id(case):
    dt, im, s, f = case
    return f"{dt}-{im}-{SIZE_IDS[s]}-{f}"


# ------------------------------------------------------------- the brute force
def brute_force(img, coords, vmask, fill):
    """reference.backward_warp by one loop per cell, four taps and C channels,
    every operation on numpy fp32 scalars (one rounding each)."""
    _, C, Hs, Ws = img.shape
    _, _, H, W = coords.shape
    a = img[0].numpy()
    is_u8 = a.dtype == np.uint8
    cx, cy = coords[0, 0].numpy(), coords[0, 1].numpy()
    out = np.empty((1, C, H, W), a.dtype)
    ok = np.zeros((1, 1, H, W), bool)
    with np.errstate(all="ignore"):
        for r in range(H):
            for q in range(W):
                x, y = F32(cx[r, q]), F32(cy[r, q])
                good = bool(x >= 0 and x <= F32(Ws - 1) and y >= 0 and y <= F32(Hs - 1))
                if vmask is not None:
                    good = good and bool(vmask[0, 0, r, q])
                ok[0, 0, r, q] = good
                if not good:
                    out[0, :, r, q] = fill
                    continue
                xf, yf = np.floor(x), np.floor(y)
                wx, wy = F32(x - xf), F32(y - yf)
                ux, uy = F32(F32(1) - wx), F32(F32(1) - wy)
                x0, y0 = int(xf), int(yf)
                for c in range(C):
                    u = F32(0)
                    for dx, dy, w in ((0, 0, F32(ux * uy)), (1, 0, F32(wx * uy)), (0, 1, F32(ux * wy)),
                                      (1, 1, F32(wx * wy))):
                        xi, yi = x0 + dx, y0 + dy
                        if w != 0 and xi < Ws and yi < Hs:
                            u = F32(u + F32(w * F32(a[c, yi, xi])))
                    if is_u8:
                        u = min(max(np.rint(u), F32(0)), F32(255))  # halves to even
                    out[0, c, r, q] = u
    return torch.from_numpy(out), torch.from_numpy(ok)


# ------------------------------------------------- what the fields have to meet
def classes(size, fname, special=None):
    """Counted from the rule, in fp32 as the rule is: cells by the number of
    taps read; cells whose tap at column Ws / row Hs is
    dropped; zero-weight taps that lie over a NaN pixel of ``special`` (an
    image (1,C,Hs,Ws)); outside, non-finite and not-valid cells."""
    (H, W), (Hs, Ws) = SIZES[size]
    p = field(fname, H, W, Hs, Ws)
    x, y = p[0, 0].flatten(), p[0, 1].flatten()
    finite = torch.isfinite(x) & torch.isfinite(y)
    inside = (x >= 0) & (x <= Ws - 1) & (y >= 0) & (y <= Hs - 1)
    v = valid(H, W).flatten()
    out = dict(taps1=0, taps2=0, taps3=0, taps4=0, col_dropped=0, row_dropped=0, nan_skipped=0,
               outside=int((finite & ~inside).sum()), non_finite=int((~finite).sum()),
               not_valid=int((inside & ~v).sum()))
    xs, ys = x[inside], y[inside]
    x0, y0 = torch.floor(xs), torch.floor(ys)
    wx, wy = xs - x0, ys - y0
    reads = torch.zeros_like(xs, dtype=torch.long)
    nan_px = None if special is None else torch.isnan(special[0]).any(0)
    for dx, dy, w in ((0, 0, (1 - wx) * (1 - wy)), (1, 0, wx * (1 - wy)), (0, 1, (1 - wx) * wy), (1, 1, wx * wy)):
        xi, yi = x0.long() + dx, y0.long() + dy
        here = (xi < Ws) & (yi < Hs)
        reads += ((w != 0) & here).long()
        if nan_px is not None:
            over = nan_px[yi.clamp(max=Hs - 1), xi.clamp(max=Ws - 1)]
            out["nan_skipped"] += int(((w == 0) & here & over).sum())
    assert bool((reads >= 1).all())
    for k in (1, 2, 3, 4):  # three: both fractions denormal, their product underflows to 0
        out[f"taps{k}"] = int((reads == k).sum())
    out["col_dropped"] = int((x0.long() + 1 >= Ws).sum())
    out["row_dropped"] = int((y0.long() + 1 >= Hs).sum())
    return out


def halves(size, fname):
    """(down, up): the cells and channels of the 'odd' uint8 image (C = 4)
    whose exact sample is k + 1/2 with k even (rounds down) and k odd (rounds
    up), among the cells that are ok, each checked against the oracle's byte."""
    (H, W), (Hs, Ws) = SIZES[size]
    img = image("odd", "uint8", 4, Hs, Ws)
    p = field(fname, H, W, Hs, Ws).double()
    x, y = p[0, 0].flatten(), p[0, 1].flatten()
    inside = (x >= 0) & (x <= Ws - 1) & (y >= 0) & (y <= Hs - 1)
    xs, ys = torch.where(inside, x, torch.zeros_like(x)), torch.where(inside, y, torch.zeros_like(y))
    x0, y0 = torch.floor(xs), torch.floor(ys)
    wx, wy = xs - x0, ys - y0
    flat = img[0].double().reshape(4, Hs * Ws)
    u = torch.zeros(4, H * W, dtype=torch.float64)
    for dx, dy, w in ((0, 0, (1 - wx) * (1 - wy)), (1, 0, wx * (1 - wy)), (0, 1, (1 - wx) * wy), (1, 1, wx * wy)):
        xi, yi = (x0.long() + dx).clamp(max=Ws - 1), (y0.long() + dy).clamp(max=Hs - 1)
        u += w * flat[:, yi * Ws + xi]  # a tap that is not there has weight 0 in exact arithmetic
    k = torch.floor(u)
    # positions on the half-pixel lattice: weights of 0, 1/4, 1/2, 1, so that the fp32 sums are exact too
    lattice = (xs * 2 == torch.floor(xs * 2)) & (ys * 2 == torch.floor(ys * 2))
    half = ((u - k) == 0.5) & inside & lattice
    got = expected("odd", "uint8", 4, size, fname, False)[0][0].reshape(4, H * W).double()
    down, up = half & (k % 2 == 0), half & (k % 2 == 1)
    assert bool((got[down] == k[down]).all()) and bool((got[up] == k[up] + 1).all())
    return int(down.sum()), int(up.sum())


def _check_coverage():
    """Every class of the rule is met, on the larger sizes by one field alone."""
    for size, ((H, W), (Hs, Ws)) in enumerate(SIZES):
        if H * W < 63:
            continue
        special = image("special", "fp32", 4, Hs, Ws)
        c = classes(size, "edge", special)
        assert min(c.values()) > 0, (SIZE_IDS[size], c)
        c = classes(size, "identity", special)
        assert c["taps1"] == min(H, Hs) * min(W, Ws) and c["nan_skipped"] > 0 and c["taps2"] == c["taps4"] == 0, c
        c = classes(size, "smooth")
        assert c["taps1"] and c["taps2"] and c["taps4"] and c["outside"] == c["non_finite"] == 0, c
        down, up = halves(size, "smooth")
        assert down > 0 and up > 0, (SIZE_IDS[size], down, up)
    # the smallest output: the last four of the edge points, integers and halves on the border
    c = classes(0, "edge")
    assert c["taps1"] and c["taps2"] and c["col_dropped"] and c["row_dropped"], c


_check_coverage()

"""Inputs of the splat_inpaint tests (not a test module): coverage maps from the
splat of forward_splat_cases' fields and hand-made ones, built once and never
changed, the radii, and the oracle's answers."""
import functools

import torch

import forward_splat_cases as S
from forward_splat_cases import NAN, same  # noqa: F401

from raft_stir_amd.ops import reference

NAMES = ("src_index", "donor", "dist2", "inv_pos", "out")
SHAPES = S.SHAPES  # 2x2, 7x9, 24x70
RADII = (0, 1, 2, 3, 5, None)
SPLAT_MAPS = tuple(f"{name}_fp{fp}" for name in S.FIELDS for fp in S.FOOTPRINTS)
# checker: every hole ties four ways; corners: one covered cell in each corner; tie_*: two covered cells equidistant
# from the centre cell along a row, a column and both diagonals; frame: a covered border around an empty block;
# bad_entries: the mixed map with entries outside [-1, N-1]
HAND_MAPS = ("checker", "corners", "tie_row", "tie_col", "tie_diag", "tie_anti", "frame", "bad_entries")
MAPS = SPLAT_MAPS + HAND_MAPS
INT_MIN, INT_MAX = -2 ** 31, 2 ** 31 - 1


def radius(R, H, W):
    """The integer the oracle takes: None is unlimited."""
    return max(H, W) if R is None else R


def centre(H, W):
    return H // 2, W // 2


def tie_cells(name, H, W):
    """The two covered cells (y, x) of a tie map, clipped into the image."""
    cy, cx = centre(H, W)
    off = {"tie_row": ((0, -1), (0, 1)), "tie_col": ((-1, 0), (1, 0)), "tie_diag": ((-1, -1), (1, 1)),
           "tie_anti": ((-1, 1), (1, -1))}[name]
    return [(min(max(cy + dy, 0), H - 1), min(max(cx + dx, 0), W - 1)) for dy, dx in off]


def bad_entries(H, W):
    """cell -> entry, for the map bad_entries: holes (below -1) and covered cells (N and above)."""
    N = H * W
    vals = (N, -5, N + 7, INT_MIN, INT_MAX, -2)
    return {(j * 29 + 3) % N: v for j, v in enumerate(vals)}


def _coverage(name, H, W):
    cov = torch.zeros(H, W, dtype=torch.bool)
    ys, xs = torch.arange(H).view(H, 1), torch.arange(W).view(1, W)
    if name == "checker":
        cov = ((ys + xs) % 2 == 0).expand(H, W).clone()
    elif name == "corners":
        cov[0, 0] = cov[0, W - 1] = cov[H - 1, 0] = cov[H - 1, W - 1] = True
    elif name.startswith("tie_"):
        for y, x in tie_cells(name, H, W):
            cov[y, x] = True
    elif name == "frame":
        cov[0], cov[H - 1], cov[:, 0], cov[:, W - 1] = True, True, True, True
    else:
        raise KeyError(name)
    return cov


@functools.lru_cache(maxsize=None)
def case(name, H, W):
    """(src_index (1,1,H,W) int32, pos (1,2,H,W), inv_pos (1,2,H,W)) on the CPU; shared, so never changed in place."""
    N = H * W
    if name in SPLAT_MAPS:
        field, fp = name.rsplit("_fp", 1)
        src, _, inv, _ = S.expected(field, H, W, int(fp))
        return src, S.field(field, H, W)[0], inv
    pos = S.field("mixed", H, W)[0]  # NaN, infinities and 1e30 among the positions
    if name == "bad_entries":
        src, _, inv, _ = S.expected("mixed", H, W, 2)
        src, inv = src.clone(), inv.clone()
        for c, v in bad_entries(H, W).items():
            src.view(-1)[c] = v
            inv.view(2, -1)[:, c] = torch.tensor([c + 0.25, -0.0]) if v >= 0 else NAN
        return src, pos, inv
    cov = _coverage(name, H, W).view(-1)
    g = torch.Generator().manual_seed(900 + N + len(name))
    src = torch.where(cov, (torch.arange(N) * 7 + 3) % N, torch.tensor(-1)).to(torch.int32)
    inv = torch.randn(2, N, generator=g) * 50
    inv[0, ::5] = -0.0  # a bit pattern arithmetic would not keep
    inv = torch.where(cov, inv, torch.tensor(NAN))
    return src.view(1, 1, H, W), pos, inv.view(1, 2, H, W).contiguous()


def values(C, H, W):
    return S.values(C, H, W)


@functools.lru_cache(maxsize=None)
def expected(name, H, W, R, C=0, fill=0.0):
    """The oracle's answer on the CPU, computed once."""
    src, pos, inv = case(name, H, W)
    return reference.splat_inpaint(src, pos, inv, values(C, H, W), radius(R, H, W), fill)


def all_same(got, want, what, device="cpu"):
    for name, g, w in zip(NAMES, got, want):
        if w is None:
            assert g is None, (what, name)
        else:
            assert g.device.type == device, (what, name)
            g = g.cpu()
            assert g.dtype == w.dtype and g.shape == w.shape and same(g, w), (what, name, int((g != w).sum()))
            if w.dtype == torch.float32:  # same() takes -0 for +0: the bits, wherever the value is no NaN
                ok = w == w
                assert torch.equal(g.view(torch.int32)[ok], w.view(torch.int32)[ok]), (what, name, "bits")

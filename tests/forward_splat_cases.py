"""Inputs of tests/test_forward_splat_cpu.py (not a test module; a kernel test
will share them): the position and score fields of the splatting tests, built
once and never changed, the outcome classes the oracle finds in them, and the
stub of the tracker tests."""
import functools

import torch

import fb_check_cases as FB
from fb_check_cases import INF, NAN, same  # noqa: F401

from raft_stir_amd.ops import reference

NAMES = ("src_index", "covered", "inv_pos", "out")

# 2x2, an odd one, and one whose plane (1680) is no multiple of the block size (256)
SHAPES = [(2, 2), (7, 9), (24, 70)]
FIELDS = ("mixed", "identity", "one_cell", "none")
FOOTPRINTS = (1, 2)
ONE_CELL = (3.25, 2.5)  # nearest cell (3, 2): halves round to even
SCORES = (0.0, 0.0, -0.0, 0.5, 0.5, 1.0, 2.0, INF, NAN, -1.0, 1e-40)


def specials(H, W):
    """Positions set in fixed places of the mixed field."""
    return [(NAN, 1.0), (INF, 0.0), (-INF, 0.0), (1e30, 1.0), (-0.5, 0.0), (-0.75, 1.0), (W - 0.5, 1.0),
            (W - 1.0, H - 1.0), (-1.0, 0.0), (float(W), 0.0), (0.0, H - 0.25)]


def _mixed(H, W):
    g = torch.Generator().manual_seed(4100 + H * W)
    grid = reference.coords_grid(1, H, W)
    centre = torch.tensor([(W - 1) / 2, (H - 1) / 2]).view(1, 2, 1, 1)
    left = (torch.arange(W) < W // 2).view(1, 1, 1, W)
    # the left half contracted about the centre (collisions), the right half expanded (holes)
    pos = centre + (grid - centre) * torch.where(left, torch.tensor(0.5), torch.tensor(1.6))
    pos = pos + (torch.rand(1, 2, H, W, generator=g) * 0.5 - 0.25)
    snap = torch.rand(1, 2, H, W, generator=g) < 0.3  # integers and exact halves
    pos = torch.where(snap, torch.round(pos * 2) / 2, pos)
    values = torch.tensor(SCORES)
    score = values[torch.randint(0, len(values), (1, 1, H, W), generator=g)]
    n = H * W
    fx, fy, fs = pos[0, 0].view(n), pos[0, 1].view(n), score.view(n)
    for j, (x, y) in enumerate(specials(H, W)):
        k = (j * 37 + 5) % n
        fx[k], fy[k] = x, y
        if x in (-0.5, W - 0.5, W - 1.0) or y == H - 0.25:
            fs[k] = 0.0  # a source: the edge rule is exercised, not the score test
    return pos.contiguous(), score.contiguous()


@functools.lru_cache(maxsize=None)
def field(name, H, W):
    """(pos (1,2,H,W), score (1,1,H,W)) on the CPU; shared, so never changed in place."""
    grid = reference.coords_grid(1, H, W).contiguous()
    if name == "mixed":
        return _mixed(H, W)
    if name == "identity":
        return grid, torch.zeros(1, 1, H, W)
    if name == "one_cell":
        pos = torch.empty(1, 2, H, W)
        pos[:, 0], pos[:, 1] = ONE_CELL
        score = torch.full((1, 1, H, W), 0.5)
        score.view(-1)[one_cell_winner(H, W)] = 0.25
        return pos, score
    if name == "none":
        g = torch.Generator().manual_seed(7)
        return grid + torch.rand(1, 2, H, W, generator=g), torch.full((1, 1, H, W), INF)
    raise KeyError(name)


def one_cell_winner(H, W):
    return (H * W * 2) // 3


@functools.lru_cache(maxsize=None)
def values(C, H, W):
    """(1,C,H,W) fp32 with distinct entries; None for C = 0."""
    if C == 0:
        return None
    g = torch.Generator().manual_seed(C * 1000 + H * W)
    return torch.randn(1, C, H, W, generator=g) + torch.arange(H * W).view(1, 1, H, W) * 8.0


@functools.lru_cache(maxsize=None)
def expected(name, H, W, footprint, C=0, fill=0.0):
    """The oracle's answer on the CPU, computed once."""
    pos, score = field(name, H, W)
    return reference.forward_splat(pos, score, values(C, H, W), footprint, fill)


def outcome_counts(pos, score, footprint=2):
    """How the cells of a field were decided, from the oracle's own rule: cells
    won in class 0 and in class 1, holes, and of the class-0 cells those with
    one offer in that class (uncontested), with several and a unique smallest
    score (score), and with the smallest score shared (tie)."""
    _, _, H, W = pos.shape
    src, cov, _, _ = reference.forward_splat(pos, score, None, footprint, 0.0)
    x, y, s = pos[0, 0].reshape(-1), pos[0, 1].reshape(-1), score.reshape(-1) + 0.0
    ok = (s >= 0) & (s < INF) & (x > -1) & (x < W) & (y > -1) & (y < H)
    near = {}
    for n in ok.nonzero().flatten().tolist():
        cx, cy = int(torch.round(x[n])), int(torch.round(y[n]))
        if 0 <= cx < W and 0 <= cy < H:
            near.setdefault(cy * W + cx, []).append(float(s[n]))
    out = dict(class0=0, class1=0, holes=int((~cov).sum()), uncontested=0, score=0, tie=0)
    for c in cov.flatten().nonzero().flatten().tolist():
        if c not in near:
            out["class1"] += 1
            continue
        out["class0"] += 1
        offers = sorted(near[c])
        if len(offers) == 1:
            out["uncontested"] += 1
        elif offers[0] < offers[1]:
            out["score"] += 1
        else:
            out["tie"] += 1
    return out


class StubShift(torch.nn.Module):
    """A constant integer translation per frame of span, +d forward and -d
    backward, for frames that carry their index in pixel [0,0,0] (as
    dense_flow_cases.frames): the flow between frames a and b is (b - a) * d
    everywhere, so every forward-backward error is 0 and a pixel is lost
    exactly when it leaves the image."""

    def __init__(self, d=(2.0, -1.0)):
        super().__init__()
        self.weight = torch.nn.Parameter(torch.zeros(1))
        self.register_buffer("d", torch.tensor(d).view(1, 2, 1, 1))

    def forward(self, image1, image2, iters=12, flow_init=None, test_mode=False, bidirectional=False):
        assert test_mode and bidirectional
        span = (image2[:, :1, :1, :1] - image1[:, :1, :1, :1])
        zero = image1[:, :2] * 0 + image2[:, :2] * 0
        up = zero + span * self.d
        lo = torch.cat([up[..., ::8, ::8] / 8, -up[..., ::8, ::8] / 8]) + 0 * flow_init
        return lo, torch.cat([up, -up])


STUB_D = FB.STUB_D

"""Inputs shared by tests/test_dense_flow_cpu.py and tests/test_dense_flow_gpu.py
(not a test module): the random ring state and flows of the kernel test with
the outcome classes the oracle finds in them, the dense step rebuilt from the
point form with Python indices, and the stub models and frames of the tracker
tests."""
import torch

import fb_check_cases as FB
import feature_cache_cases as F
import multi_flow_cases as M
from fb_check_cases import INF, NAN, same  # noqa: F401
from warm_start_cases import smooth

from raft_stir_amd.ops import reference

NAMES = ("pos", "score", "visible", "choice", "fb_err", "cand_err")

# the CPU test's field, and the kernel test's: 2x2, an odd one with a tail in any vector access, one whose
# plane (1680) is no multiple of the block size (256).  Amplitudes as fb_check_cases chooses them: a part
# of the targets leaves the image, the rest splits between the two verdicts of the check
CPU_HW = (24, 40)
KERNEL_HW = [(2, 2), (7, 9), (24, 70)]
for _hw, _amp in (((24, 40), 3), ((7, 9), 2), ((24, 70), 4)):
    FB.AMP.setdefault(_hw, _amp)


def default_idx(K):
    """[src_0 .. src_{K-1}, dst] for a ring of R = K + 2 rows: slot 0 reads the
    last row (the anchor's place), slot k row k - 1; row K - 1 is written and
    row K is neither read nor written."""
    return torch.tensor([K + 1] + list(range(K - 1)) + [K - 1], dtype=torch.int32)


def step_inputs(K, H, W, seed=0):
    """(fw, bw (K,2,H,W), ring_pos (R,2,H,W), ring_score (R,H,W), idx (K+1,)
    int32) with R = K + 2.  The flows are fb_check_cases.flow_pair's (a few
    pixels, both verdicts occur).  Every row of ring_pos is the pixel grid
    moved by up to three pixels, so that some starts lie outside the image,
    with a few pixels on the border, NaN and +inf in every row; the scores
    come from a few values (ties), +inf and NaN.  For K >= 2 slot 1 repeats slot 0's flows
    and the row it reads repeats slot 0's positions and, for a third of the
    pixels, its scores, so that exact ties between two eligible slots occur."""
    R = K + 2
    fw, bw = FB.flow_pair(K, H, W)
    g = torch.Generator().manual_seed(9000 + 100 * K + H * W + seed)
    grid = reference.coords_grid(1, H, W)
    ring_pos = grid + (torch.rand(R, 2, H, W, generator=g) * 6.0 - 3.0)
    n = H * W
    flat = ring_pos.view(R, 2, n)
    special = [(0.0, 0.0), (W - 1.0, H - 1.0), (W - 1.0, 0.5), (0.25, 0.0), (NAN, 1.0), (W - 0.5, 1.0), (-0.5, H - 1.0),
               (INF, 0.0)]
    for j, (x, y) in enumerate(special):  # in every row: whatever idx says, some slot starts there
        flat[:, 0, (j * 37) % n], flat[:, 1, (j * 37) % n] = x, y
    values = torch.tensor([0.0, 0.0, 0.0, 0.5, 1.0, 2.0, INF, NAN])
    ring_score = values[torch.randint(0, len(values), (R, H, W), generator=g)]
    idx = default_idx(K)
    if K >= 2:
        fw[1], bw[1] = fw[0], bw[0]
        s0, s1 = int(idx[0]), int(idx[1])
        ring_pos[s1] = ring_pos[s0]
        twin = (torch.arange(n) % 3 == 0).view(H, W)
        ring_score[s1][twin] = ring_score[s0][twin]
    return fw, bw, ring_pos, ring_score, idx


def point_form(fw, bw, ring_pos, ring_score, idx, active, alpha=FB.ALPHA, op=None):
    """The dense step from the point form, the rows picked with Python
    indices: (the six outputs in the dense shapes, the ring after the step,
    the (K,N) start scores).  ``op``: the point form's implementation,
    reference.multi_flow_track_points unless given."""
    K, _, H, W = fw.shape
    R, N = ring_pos.shape[0], H * W
    i = [min(max(int(v), 0), R - 1) for v in idx.tolist()]
    src, dst = i[:K], i[K]
    starts = torch.stack([ring_pos[s].reshape(2, N).t() for s in src]).contiguous()
    sscore = torch.stack([ring_score[s].reshape(N) for s in src])
    act = active.clone()
    for k, s in enumerate(src):
        if s == dst:
            act[k] = False
    op = reference.multi_flow_track_points if op is None else op
    pts, score, vis, choice, err, cand = op(fw, bw, starts, sscore, sscore < INF, act, *alpha)
    score = torch.where(vis, score, torch.full_like(score, INF))
    outs = (pts[0].t().reshape(1, 2, H, W), score.reshape(1, 1, H, W), vis.reshape(1, 1, H, W),
            choice.reshape(1, 1, H, W), err.reshape(1, 1, H, W), cand.reshape(K, H, W))
    rp, rs = ring_pos.clone(), ring_score.clone()
    rp[dst], rs[dst] = outs[0][0], outs[1][0, 0]
    return outs, (rp, rs), sscore


def outcome_counts(outs, sscore, active, fw, bw, ring_pos, idx, alpha=FB.ALPHA):
    """multi_flow_cases.outcome_counts of a dense step: how many pixels were
    chosen by score, by a tie, fell back or had no active slot."""
    K, _, H, W = fw.shape
    N = H * W
    src = idx.tolist()[:K]
    ok = torch.cat([reference.fb_track_points(fw[k:k + 1], bw[k:k + 1], ring_pos[s].reshape(2, N).t()[None], *alpha)[2]
                    for k, s in enumerate(src)])
    flat = (None, outs[1].reshape(1, N), outs[2].reshape(1, N), outs[3].reshape(1, N), None, outs[5].reshape(K, N))
    return M.outcome_counts(flat, sscore, sscore < INF, active, ok)


def single_masks(K):
    return [(f"only{j}", torch.arange(K) == j) for j in sorted({0, K // 2, K - 1})]


# ------------------------------------------------------------------- trackers
def frames(T, H=M.SC_H, W=M.SC_W, seed=11):
    """(T,1,3,H,W) frames with the index in pixel [0,0,0], as multi_flow_cases.scenario()."""
    g = torch.Generator().manual_seed(seed)
    out = torch.rand(T, 1, 3, H, W, generator=g) * 255
    for t in range(T):
        out[t, 0, 0, 0, 0] = float(t)
    return out


def pixel_centres(H, W, device=None):
    """(1,H*W,2): every pixel centre as a point, in the order of the planes."""
    return reference.coords_grid(1, H, W, device=device).reshape(1, 2, H * W).transpose(1, 2).contiguous()


def as_points(trk):
    """A DenseMultiFlowTracker's attributes in MultiFlowTracker's shapes."""
    n = trk.pos.shape[-2] * trk.pos.shape[-1]
    return (trk.pos.reshape(1, 2, n).transpose(1, 2), trk.visible.reshape(1, n), trk.score.reshape(1, n),
            trk.fb_err.reshape(1, n), trk.delta.reshape(1, n))


def of_points(trk):
    return trk.points, trk.visible, trk.score, trk.fb_err, trk.delta


class StubWobble(F.StubSpanCached):
    """StubSpanCached (the occlusion scenario's translation per frame, with an
    encode / refine pair) plus a smooth field of under a pixel per frame of
    span, forward and, negated, backward: a deterministic function of the
    frame indices whose positions are not integers and whose forward-backward
    errors differ from pixel to pixel and from span to span, so that every
    slot's score takes part in the choice.  On frames of any size H x W that
    holds the scenario's rectangle.  ``amp = 0``: no such field; all positions
    are integers then and the CPU and the GPU give the same bits."""

    def __init__(self, H=M.SC_H, W=M.SC_W, amp=0.75):
        super().__init__()
        mask = torch.zeros(1, 1, H, W)
        y0, y1, x0, x1 = M.SC_RECT
        mask[..., y0:y1, x0:x1] = 1.0
        self.drift = mask * torch.tensor(M.SC_DRIFT).view(1, 2, 1, 1)
        self.off = mask * torch.tensor(M.SC_OFF).view(1, 2, 1, 1)
        self.register_buffer("wob", smooth(H, W, 5, amp, 0.02 if amp else 0.0)[None])

    def _refine(self, fmap1, fmap2, ctx, flow_init):
        _, up = super()._refine(fmap1, fmap2, ctx, flow_init)
        t1, t2 = fmap1[:, :1, :1, :1], fmap2[:, :1, :1, :1]
        up = up + (t2 - t1) * self.wob
        return up[..., ::8, ::8] / 8 + 0 * flow_init, up


class StubAny(torch.nn.Module):
    """Constant flows (+d forward, -d backward) on frames of any size, for the
    command-line run."""

    def __init__(self):
        super().__init__()
        self.weight = torch.nn.Parameter(torch.zeros(1))
        self.register_buffer("d", torch.tensor(FB.STUB_D).view(1, 2, 1, 1))

    def forward(self, image1, image2, iters=12, flow_init=None, test_mode=False, bidirectional=False):
        assert test_mode and bidirectional
        zero = image1[:, :2] * 0 + image2[:, :2] * 0
        lo = torch.cat([zero[..., ::8, ::8] + self.d / 8, zero[..., ::8, ::8] - self.d / 8]) + 0 * flow_init
        return lo, torch.cat([zero + self.d, zero - self.d])

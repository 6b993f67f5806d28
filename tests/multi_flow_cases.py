"""Inputs shared by tests/test_multi_flow_cpu.py and tests/test_multi_flow_gpu.py
(not a test module): the hand-worked selection cases of
ops.multi_flow_track_points, the random inputs of the kernel test with the
outcome classes the oracle finds in them, and the occlusion scenario with its
stub model."""
import torch
import torch.nn as nn

import fb_check_cases as FB
from fb_check_cases import INF, NAN, same  # noqa: F401

# the kernel test's field; the amplitude as for fb_check_cases' 33x70 (flow_pair reads it from this table)
KERNEL_HW = (40, 64)
FB.AMP.setdefault(KERNEL_HW, 4)

NAMES = ("points", "score", "visible", "choice", "err", "cand_err")


# ------------------------------------------------------------ hand-worked cases
H0, W0 = 16, 20
LOOSE = (0.0, 20.0)  # the check passes iff err^2 <= 20: err 0, 3 and 4 pass, 5 does not


def const_slots(vecs, miss):
    """K constant slots on 16x20: fw[k] = vecs[k], bw[k] = -vecs[k] + (miss[k], 0).
    A start whose target stays in the image comes back off by miss[k] pixels:
    err = |miss[k]| exactly, and with LOOSE the check passes iff |miss[k]| <= 4."""
    fw = torch.stack([FB._const(H0, W0, dx, dy)[0] for dx, dy in vecs])
    bw = torch.stack([FB._const(H0, W0, -dx + m, -dy)[0] for (dx, dy), m in zip(vecs, miss)])
    return fw, bw


def selection_cases():
    """[(name, inputs, expected)]: inputs = (fw, bw, starts (3,N,2), start_score
    (3,N), start_visible (3,N), active (3,), alpha); expected = dict of the
    outputs that the case pins, every value worked out by hand.  All slots
    start at (5, 6) unless said otherwise; slot k moves by VECS[k]."""
    vecs = [(1, 0), (2, 1), (-3, 2)]
    p = [5.0, 6.0]
    cand = [[6.0, 6.0], [7.0, 7.0], [2.0, 8.0]]

    def inp(miss, score, vis=(True, True, True), act=(True, True, True), starts=None, alpha=LOOSE):
        fw, bw = const_slots(vecs, miss)
        st = torch.tensor([[p]] * 3 if starts is None else starts)
        return (fw, bw, st, torch.tensor(score).view(3, 1), torch.tensor(vis).view(3, 1), torch.tensor(act), alpha)

    def exp(points, score, visible, choice, err, cand_err=None):
        out = {"points": torch.tensor([[points]]), "score": torch.tensor([[score]]),
               "visible": torch.tensor([[visible]]), "choice": torch.tensor([[choice]], dtype=torch.int32),
               "err": torch.tensor([[err]])}
        if cand_err is not None:
            out["cand_err"] = torch.tensor(cand_err).view(3, 1)
        return out

    cases = [
        # s = (2+0, 1+3, 0.5+4) = (2, 4, 4.5)
        ("smallest_score_slot0", inp([0, 3, 4], [2.0, 1.0, 0.5]), exp(cand[0], 2.0, True, 0, 0.0, [0.0, 3.0, 4.0])),
        # s = (5, 4, 3.5): the largest error, the smallest score
        ("smallest_score_slot2", inp([0, 3, 4], [5.0, 1.0, -0.5]), exp(cand[2], 3.5, True, 2, 4.0, [0.0, 3.0, 4.0])),
        # s = (4, 3, 3): equal scores go to the lowest slot
        ("tie_lowest_slot", inp([4, 3, 0], [0.0, 0.0, 3.0]), exp(cand[1], 3.0, True, 1, 3.0, [4.0, 3.0, 0.0])),
        ("tie_all_three", inp([0, 0, 0], [1.0, 1.0, 1.0]), exp(cand[0], 1.0, True, 0, 0.0)),
        # slot 0 is perfect (err 0, score 0) but may not be taken
        ("perfect_but_inactive", inp([0, 3, 4], [0.0, 1.0, 1.0], act=(False, True, True)),
         exp(cand[1], 4.0, True, 1, 3.0, [0.0, 3.0, 4.0])),
        ("perfect_but_not_start_visible", inp([0, 3, 4], [0.0, 1.0, 1.0], vis=(False, True, True)),
         exp(cand[1], 4.0, True, 1, 3.0)),
        ("perfect_but_inf_start_score", inp([0, 3, 4], [INF, 1.0, 1.0]), exp(cand[1], 4.0, True, 1, 3.0)),
        ("perfect_but_nan_start_score", inp([0, 3, 4], [NAN, 1.0, 1.0]), exp(cand[1], 4.0, True, 1, 3.0)),
        # every slot misses by 5: 25 > 20.  The lowest active slot's candidate and score come back
        ("all_fail_fallback", inp([5, 5, 5], [7.0, 1.0, 2.0]), exp(cand[0], 12.0, False, 0, 5.0, [5.0, 5.0, 5.0])),
        ("all_fail_fallback_lowest_active", inp([5, 5, 5], [7.0, 1.0, 2.0], act=(False, False, True)),
         exp(cand[2], 7.0, False, 2, 5.0)),
        # the only passing slot is not start-visible: fallback to slot 0 although slot 1 is 'better'
        ("fallback_ignores_scores", inp([5, 0, 5], [7.0, 0.0, 2.0], vis=(True, False, True)),
         exp(cand[0], 12.0, False, 0, 5.0)),
        # slot 2 starts at (2, 6): its target (-1, 8) has left the image; cand_err, score +inf, not eligible
        ("target_leaves_image", inp([3, 4, 0], [1.0, 1.0, 0.0], starts=[[p], [p], [[2.0, 6.0]]]),
         exp(cand[0], 4.0, True, 0, 3.0, [3.0, 4.0, INF])),
        # ... and when it is the only active slot it comes back all the same, with score +inf
        ("target_leaves_image_only_slot", inp([3, 4, 0], [1.0, 1.0, 0.0], act=(False, False, True),
                                              starts=[[p], [p], [[2.0, 6.0]]]),
         exp([-1.0, 8.0], INF, False, 2, INF, [3.0, 4.0, INF])),
        # no active slot: starts[0] and start_score[0]
        ("no_active_slot", inp([0, 0, 0], [2.5, 1.0, 0.0], act=(False, False, False),
                               starts=[[[4.0, 3.0]], [p], [p]]),
         exp([4.0, 3.0], 2.5, False, -1, INF, [0.0, 0.0, 0.0])),
    ]
    return cases


def check_selection_cases(op):
    """op(fw, bw, starts, start_score, start_visible, active, a1, a2) -> the six
    outputs, CPU tensors in and out: the implementation under test."""
    for name, (fw, bw, st, sc, vis, act, alpha), want in selection_cases():
        got = dict(zip(NAMES, op(fw, bw, st, sc, vis, act, *alpha)))
        assert got["points"].shape == (1, 1, 2) and got["cand_err"].shape == (3, 1), name
        assert got["choice"].dtype == torch.int32 and got["visible"].dtype == torch.bool, name
        for key, w in want.items():
            assert same(got[key], w), f"{name}: {key} = {got[key].tolist()}, expected {w.tolist()}"


# ------------------------------------------------------- kernel test's inputs
def kernel_inputs(K, N, seed=0):
    """flows (K,2,40,64) from fb_check_cases.flow_pair (both verdicts occur);
    starts uniform in [-2, W+1] x [-2, H+1] with points on the border, at the
    corners and NaN among them; random start_visible; start_score from a few
    values (ties), +inf and NaN.  For K >= 2 slot 1 repeats slot 0's flows and
    starts, and for a third of the points its start score and visibility, so
    that exact ties between two eligible slots occur."""
    H, W = KERNEL_HW
    fw, bw = FB.flow_pair(K, H, W)
    g = torch.Generator().manual_seed(7000 + 100 * K + N + seed)
    starts = torch.rand(K, N, 2, generator=g) * torch.tensor([W + 3.0, H + 3.0]) - 2.0
    special = torch.tensor([[0.0, 0.0], [W - 1.0, H - 1.0], [W - 1.0, 3.5], [7.25, 0.0], [NAN, 5.0], [W + 0.5, 2.0],
                            [-0.5, H - 1.0]])
    for j in range(min(N, len(special))):
        starts[(j * 5) % K, (j * 37) % N] = special[j]
    values = torch.tensor([0.0, 0.0, 0.0, 0.5, 1.0, 2.0, INF, NAN])
    score = values[torch.randint(0, len(values), (K, N), generator=g)]
    vis = torch.rand(K, N, generator=g) < 0.8
    if K >= 2:
        fw[1], bw[1], starts[1] = fw[0], bw[0], starts[0]
        twin = torch.arange(N) % 3 == 0
        score[1, twin] = score[0, twin]
        vis[1, twin] = vis[0, twin]
    return fw, bw, starts, score, vis


def active_masks(K):
    """The masks each shape is run with: a mixed one (slot 0 on, so that the
    twin slots can tie; about a third off), all on, and none."""
    g = torch.Generator().manual_seed(K)
    mixed = torch.rand(K, generator=g) < 0.7
    mixed[0] = True
    if K >= 2:
        mixed[1] = True
    if K >= 3:
        mixed[2] = False
    return [("mixed", mixed), ("all", torch.ones(K, dtype=torch.bool)), ("none", torch.zeros(K, dtype=torch.bool))]


def outcome_counts(outs, start_score, start_visible, active, ok):
    """How many points were chosen by score (one best among several eligible
    slots), by tie (two eligible slots share the best score), fell back, or had
    no active slot.  ok (K,N): the per-slot verdicts."""
    _, score, visible, choice, _, cand_err = outs
    s = start_score + cand_err
    elig = active.view(-1, 1) & start_visible & ok & (s < INF)
    best = torch.where(elig, s, torch.full_like(s, INF)).min(dim=0).values
    at_best = (elig & (s == best)).sum(dim=0)
    vis = visible[0]
    return {"score": int((vis & (elig.sum(dim=0) >= 2) & (at_best == 1)).sum()),
            "tie": int((vis & (at_best >= 2)).sum()),
            "fallback": int((~vis & (choice[0] >= 0)).sum()),
            "none": int((choice[0] < 0).sum())}


# ---------------------------------------------------------- occlusion scenario
SC_H, SC_W, SC_T = 48, 64, 8
SC_D = (2.0, 1.0)                # every point moves by d per frame
SC_RECT = (8, 32, 8, 48)         # y0, y1, x0, x1: where the occluder passes
SC_OCCLUDED = (3, 4)             # the frames in which it is there
SC_DRIFT = (3.0, 2.0)            # what it adds to the forward flow of a pair ending in such a frame
SC_OFF = (4.0, -3.0)             # and to the backward flow: the way back misses home by drift + off = (7, -1)
SC_INSIDE = [[12.0, 10.0], [15.5, 12.25]]   # stay in the rectangle for all 8 frames, drifted or not
SC_OUTSIDE = [[20.5, 33.25], [49.0, 10.0]]  # all four taps stay outside it; the second ends on x = W-1
SC_POINTS = SC_INSIDE + SC_OUTSIDE


class StubSpanFlow(nn.Module):
    """A 'model' for frames that carry their index in pixel [0,0,0]: the
    bidirectional pass returns the translation (index2 - index1) * d forward
    and its negative backward, at both resolutions, from plain torch ops on
    its inputs, so that it can be captured.  For a pair whose second frame is
    occluded the forward field has SC_DRIFT and the backward field SC_OFF
    added inside SC_RECT.  The weight is ignored."""

    def __init__(self):
        super().__init__()
        self.weight = nn.Parameter(torch.zeros(1))
        self.register_buffer("d", torch.tensor(SC_D).view(1, 2, 1, 1))
        mask = torch.zeros(1, 1, SC_H, SC_W)
        y0, y1, x0, x1 = SC_RECT
        mask[..., y0:y1, x0:x1] = 1.0
        self.register_buffer("drift", mask * torch.tensor(SC_DRIFT).view(1, 2, 1, 1))
        self.register_buffer("off", mask * torch.tensor(SC_OFF).view(1, 2, 1, 1))
        self.calls = 0

    def forward(self, image1, image2, iters=12, flow_init=None, test_mode=False, bidirectional=False):
        assert test_mode and bidirectional and flow_init.shape[0] == 2 * image1.shape[0]
        self.calls += 1
        t1, t2 = image1[:, :1, :1, :1], image2[:, :1, :1, :1]  # (B,1,1,1)
        occ = ((t2 == SC_OCCLUDED[0]) | (t2 == SC_OCCLUDED[1])).to(image1.dtype)
        zero = image1[:, :2] * 0 + image2[:, :2] * 0  # (B,2,H,W)
        fw = zero + (t2 - t1) * self.d + occ * self.drift
        bw = zero - (t2 - t1) * self.d + occ * self.off
        lo = torch.cat([fw[..., ::8, ::8], bw[..., ::8, ::8]]) / 8 + 0 * flow_init
        return lo, torch.cat([fw, bw])


def scenario():
    """frames (8,1,3,48,64) with the index in pixel [0,0,0], points (1,4,2)."""
    g = torch.Generator().manual_seed(11)
    frames = torch.rand(SC_T, 1, 3, SC_H, SC_W, generator=g) * 255
    for t in range(SC_T):
        frames[t, 0, 0, 0, 0] = float(t)
    return frames, torch.tensor([SC_POINTS])


def check_scenario(single, multi, points):
    """single, multi: (traj (8,4,2), visible, score, delta (8,4)) on the CPU of
    the deltas=(1,) and the deltas=(1,2,None) run."""
    d, drift = torch.tensor(SC_D), torch.tensor(SC_DRIFT)
    p0 = points[0]
    ins, outs = [0, 1], [2, 3]
    first_clear = SC_OCCLUDED[1] + 1
    for name, (traj, vis, score, delta) in (("single", single), ("multi", multi)):
        assert traj.shape == (SC_T, 4, 2) and vis.shape == (SC_T, 4) and score.shape == (SC_T, 4), name
        assert delta.shape == (SC_T, 4) and vis.dtype == torch.bool and delta.dtype == torch.int32, name
        assert torch.equal(traj[0], p0) and vis[0].all() and (score[0] == 0).all() and (delta[0] == 0).all(), name
        for t in range(1, SC_T):
            # outside the rectangle: exact, visible, score 0, the shortest span (ties go to the lowest slot)
            assert torch.equal(traj[t, outs], p0[outs] + t * d), (name, t)
            assert vis[t, outs].all() and (score[t, outs] == 0).all() and (delta[t, outs] == 1).all(), (name, t)
        for t in range(1, SC_OCCLUDED[0]):
            assert torch.equal(traj[t, ins], p0[ins] + t * d) and vis[t, ins].all(), (name, t)
            assert (score[t, ins] == 0).all() and (delta[t, ins] == 1).all(), (name, t)
        for i, t in enumerate(SC_OCCLUDED):
            # every span fails: the frame-to-frame chain goes on, carried away by the drift
            assert torch.equal(traj[t, ins], p0[ins] + t * d + (i + 1) * drift), (name, t)
            assert not vis[t, ins].any() and (delta[t, ins] == 1).all(), (name, t)
    traj, vis, score, delta = multi
    for t in range(first_clear, SC_T):
        assert torch.equal(traj[t, ins], p0[ins] + t * d), t
        assert vis[t, ins].all() and (score[t, ins] == 0).all(), t
        # at the first clear frame only the anchor's start is a visible one; after it the chain's is again
        assert (delta[t, ins] == (0 if t == first_clear else 1)).all(), (t, delta[t])
    traj, vis, score, delta = single
    for t in range(first_clear, SC_T):
        assert torch.equal(traj[t, ins], p0[ins] + t * d + 2 * drift), t
        assert not vis[t, ins].any() and (score[t, ins] == INF).all() and (delta[t, ins] == 1).all(), t

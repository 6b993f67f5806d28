"""Shared by tests/test_tracker_forms_cpu.py and tests/test_tracker_forms_gpu.py
(not a test module): a 13-frame stub sequence, long enough for the periodic
part of the ring's index table (t > 2L) at L = 3 and 4, the forms of the
multi-delta tracker that must agree on it bit for bit, and an oracle that
keeps its history in a Python list and cannot drift with the implementation."""
import torch

import dense_flow_cases as D
import feature_cache_cases as F
import multi_flow_cases as M

from raft_stir_amd.export.denseflow import DenseMultiFlowTracker
from raft_stir_amd.export.multiflow import MultiFlowTracker
from raft_stir_amd.ops import reference

T = 13
DELTAS = [(2, 4), (1, 3, None), (3,)]
DENSE_DELTAS = (1, 3, None)
ALPHA = (0.01, 0.5)
# of the 4 x 13 returned positions of M.SC_POINTS, the fraction that is visible (worked out on the oracle)
VISIBLE = {(2, 4): 0.44, (1, 3, None): 0.83, (3,): 0.19}
NAMES = ("positions", "visible", "score", "delta")


def oracle(frames, points, deltas):
    """The tracker's rule with Python indices, on the CPU: the start of slot k
    is what was returned for frame t - D_k (the anchor: frame 0; an inactive
    slot: frame 0, ignored), looked up in the list of all past results; the
    choice is ops/reference.py's.  -> (positions (T,N,2), visible, score, delta (T,N))."""
    model = M.StubSpanFlow()
    K, N = len(deltas), points.shape[1]
    h, w = frames.shape[-2] // 8, frames.shape[-1] // 8
    span = torch.tensor([d or 0 for d in deltas], dtype=torch.int32)
    past = [(points[0].clone(), torch.ones(N, dtype=torch.bool), torch.zeros(N), torch.zeros(N, dtype=torch.int32))]
    for t in range(1, len(frames)):
        active = [t >= 1 if d is None else t >= d for d in deltas]
        src = [t - d if d is not None and a else 0 for d, a in zip(deltas, active)]
        _, up = model(torch.cat([frames[s] for s in src]), frames[t].expand(K, -1, -1, -1), iters=2,
                      flow_init=torch.zeros(2 * K, 2, h, w), test_mode=True, bidirectional=True)
        pts, score, vis, choice, _, _ = reference.multi_flow_track_points(
            up[:K], up[K:], torch.stack([past[s][0] for s in src]), torch.stack([past[s][2] for s in src]),
            torch.stack([past[s][1] for s in src]), torch.tensor(active), *ALPHA)
        score = torch.where(vis, score, torch.full_like(score, M.INF))
        delta = torch.where(choice >= 0, span[choice.clamp(min=0).long()], torch.full_like(choice, -1))
        past.append((pts[0], vis[0], score[0], delta[0]))
    return tuple(torch.stack([p[i] for p in past]) for i in range(4))


def sequence():
    return D.frames(T), torch.tensor([M.SC_POINTS])


def run_points(trk, frames, points):
    """(positions, visible, score, delta) of every step, stepping by hand."""
    trk.reset()
    out = []
    for t in range(len(frames)):
        trk.step(frames[t], points if t == 0 else None)
        out.append((trk.points[0].clone(), trk.visible[0].clone(), trk.score[0].clone(), trk.delta[0].clone()))
    return tuple(torch.stack([o[i] for o in out]) for i in range(4))


def run_dense(trk, frames):
    trk.reset()
    out = []
    for t in range(len(frames)):
        trk.step(frames[t])
        pos, vis, score, _, delta = D.as_points(trk)
        out.append((pos[0].clone(), vis[0].clone(), score[0].clone(), delta[0].clone()))
    return tuple(torch.stack([o[i] for o in out]) for i in range(4))


def forms(deltas, device):
    """[(name, (positions, visible, score, delta) on the CPU)] of every form of
    the tracker on ``device``, each run twice with a reset() between; for
    DENSE_DELTAS also the dense tracker and the point tracker at every pixel
    centre, under names that start with 'pixels'."""
    frames, points = sequence()
    frames, points = frames.to(device), points.to(device)
    out = []
    plain = MultiFlowTracker(M.StubSpanFlow().to(device), iters=2, deltas=deltas, fb_alpha=ALPHA)
    cached = MultiFlowTracker(F.StubSpanCached().to(device), iters=2, deltas=deltas, fb_alpha=ALPHA,
                              cache_features=True)
    for name, trk in (("plain", plain), ("cached", cached)):
        out.append((name, run_points(trk, frames, points)))
        out.append((name + "_again", run_points(trk, frames, points)))
    if deltas == DENSE_DELTAS:
        centres = D.pixel_centres(M.SC_H, M.SC_W, device=device)
        out.append(("pixels_plain", run_points(plain, frames, centres)))
        for cache in (False, True):
            dense = DenseMultiFlowTracker(F.StubSpanCached().to(device), iters=2, deltas=deltas, fb_alpha=ALPHA,
                                          cache_features=cache)
            name = "pixels_dense_cached" if cache else "pixels_dense"
            out.append((name, run_dense(dense, frames)))
            out.append((name + "_again", run_dense(dense, frames)))
    return [(n, tuple(t.cpu() for t in r)) for n, r in out]


def check_forms(deltas, device):
    frames, points = sequence()
    want = oracle(frames, points, deltas)
    check_variety(deltas, want)
    want_pixels = oracle(frames, D.pixel_centres(M.SC_H, M.SC_W), deltas) if deltas == DENSE_DELTAS else None
    for name, got in forms(deltas, device):
        ref = want_pixels if name.startswith("pixels") else want
        for key, g, w in zip(NAMES, got, ref):
            assert g.shape == w.shape and g.dtype == w.dtype, (name, key)
            assert M.same(g, w), f"{deltas} {name}: {key} differs from the oracle first at frame " \
                                 f"{int((g != w).reshape(T, -1).any(dim=1).nonzero()[0])}"


def check_variety(deltas, result):
    """The sequence is not degenerate: the stated part of the positions is
    visible, every finite span and, where the first frames have no active
    slot, -1 are chosen, and points are still inside the image halfway and
    outside it at the end."""
    pos, vis, score, delta = result
    assert round(vis.float().mean().item(), 2) == VISIBLE[deltas], vis.float().mean().item()
    # 0 is the first frame's; the four points never need the anchor, the next longer span finds them first
    expected = {0} | {d for d in deltas if d} | (set() if deltas[-1] is None or deltas[0] == 1 else {-1})
    assert set(delta.unique().tolist()) == expected, (deltas, delta.unique().tolist())
    inside = (pos[..., 0] >= 0) & (pos[..., 0] <= M.SC_W - 1) & (pos[..., 1] >= 0) & (pos[..., 1] <= M.SC_H - 1)
    assert inside[:T // 2 + 1].all() and not inside[-1].all() and inside[-1].any()
    assert ((score == M.INF) == ~vis).all() and (score[vis] >= 0).all()

"""Multi-delta point tracking: the most reliable of K flow pairs per point
(csrc/multi_flow.hip on GPU, ATen on CPU and while tracing / exporting)."""
from __future__ import annotations

import math

import torch

from . import _ext
from . import reference as ref

MAX_SLOTS = 16


def multi_flow_track_points(flow_fw: torch.Tensor, flow_bw: torch.Tensor, starts: torch.Tensor,
                            start_score: torch.Tensor, start_visible: torch.Tensor, active: torch.Tensor,
                            alpha1: float = 0.01, alpha2: float = 0.5):
    """flows (K,2,H,W), any float dtype or layout, slot k spanning t-D_k -> t
    and back; starts (K,N,2) xy pixels, start_score (K,N), start_visible (K,N)
    and active (K,), the last a tensor on the flows' device (it is never read
    on the host) -> (points (1,N,2) fp32, score (1,N) fp32, visible (1,N)
    bool, choice (1,N) int32, err (1,N) fp32, cand_err (K,N) fp32) in one
    launch (the rule: ops/reference.py)."""
    name = "multi_flow_track_points"
    if flow_fw.dim() != 4 or flow_fw.shape[1] != 2:
        raise ValueError(f"{name}: flow_fw must be (K,2,H,W), got {tuple(flow_fw.shape)}")
    if flow_bw.shape != flow_fw.shape:
        raise ValueError(f"{name}: flow_fw and flow_bw must have the same shape, got {tuple(flow_fw.shape)} "
                         f"and {tuple(flow_bw.shape)}")
    K, _, H, W = flow_fw.shape
    if not 1 <= K <= MAX_SLOTS:
        raise ValueError(f"{name}: 1 to {MAX_SLOTS} slots expected, got K = {K}")
    if H < 2 or W < 2:
        raise ValueError(f"{name}: H, W >= 2 expected, got {(H, W)}")
    if not (alpha1 >= 0 and alpha2 >= 0 and math.isfinite(alpha1) and math.isfinite(alpha2)):
        raise ValueError(f"{name}: alpha1 and alpha2 must be finite and >= 0, got {alpha1} and {alpha2}")
    if starts.dim() != 3 or starts.shape[0] != K or starts.shape[1] < 1 or starts.shape[2] != 2:
        raise ValueError(f"{name}: starts must be (K,N,2) with K = {K} and N >= 1, got {tuple(starts.shape)}")
    N = starts.shape[1]
    for what, t, shape in (("start_score", start_score, (K, N)), ("start_visible", start_visible, (K, N)),
                           ("active", active, (K,))):
        if tuple(t.shape) != shape:
            raise ValueError(f"{name}: {what} must be {shape}, got {tuple(t.shape)}")
    fw, bw = flow_fw.float().contiguous(), flow_bw.float().contiguous()
    p, sc = starts.float().contiguous(), start_score.float().contiguous()
    vis, act = start_visible.bool().contiguous(), active.bool().contiguous()
    if _ext.use_hip(fw):
        return tuple(torch.ops.raft_stir.multi_flow_track_points(fw, bw, p, sc, vis, act, float(alpha1),
                                                                 float(alpha2)))
    return ref.multi_flow_track_points(fw, bw, p, sc, vis, act, float(alpha1), float(alpha2))

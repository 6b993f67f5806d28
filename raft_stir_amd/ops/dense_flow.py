"""Dense multi-delta tracking: the most reliable of K flow pairs at every pixel
of the anchor frame, on a planar state ring (csrc/dense_flow.hip on GPU, ATen
on CPU and while tracing / exporting)."""
from __future__ import annotations

import math

import torch

from . import _ext
from . import reference as ref
from .multi_flow import MAX_SLOTS


def dense_multi_flow_step(flow_fw: torch.Tensor, flow_bw: torch.Tensor, ring_pos: torch.Tensor,
                          ring_score: torch.Tensor, idx: torch.Tensor, active: torch.Tensor,
                          alpha1: float = 0.01, alpha2: float = 0.5, cand_err: bool = False):
    """flows (K,2,H,W), any float dtype or layout, slot k spanning the frame
    of ring row ``idx[k]`` -> t and back; ring_pos (R,2,H,W) and ring_score
    (R,H,W), contiguous fp32: for every pixel of the anchor frame its position
    in the frame of each row and its score there, +inf where it was not
    visible; idx (K+1,) int32 and active (K,) bool on the flows' device, never
    read on the host: the K source rows, then the row to write, each clamped
    to [0, R-1] (a source equal to the row written counts as inactive).
    -> (pos (1,2,H,W) fp32, score (1,1,H,W) fp32, +inf where not visible,
    visible (1,1,H,W) bool, choice (1,1,H,W) int32, fb_err (1,1,H,W) fp32,
    cand_err (K,H,W) fp32 or None unless asked for) in one launch; pos and
    score are also written to ring row ``idx[K]``, in place (the rule:
    ops/reference.py)."""
    name = "dense_multi_flow_step"
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
    if ring_pos.dim() != 4 or tuple(ring_pos.shape[1:]) != (2, H, W) or ring_pos.shape[0] < 2:
        raise ValueError(f"{name}: ring_pos must be (R,2,H,W) = (R,2,{H},{W}) with R >= 2, got "
                         f"{tuple(ring_pos.shape)}")
    R = ring_pos.shape[0]
    if tuple(ring_score.shape) != (R, H, W):
        raise ValueError(f"{name}: ring_score must be {(R, H, W)}, got {tuple(ring_score.shape)}")
    for what, t in (("ring_pos", ring_pos), ("ring_score", ring_score)):
        if t.dtype != torch.float32 or not t.is_contiguous():  # changed in place: no converted copy
            raise ValueError(f"{name}: {what} must be contiguous fp32, got {t.dtype}")
    if idx.dtype != torch.int32 or tuple(idx.shape) != (K + 1,):
        raise ValueError(f"{name}: idx must be int32 {(K + 1,)}, got {idx.dtype} {tuple(idx.shape)}")
    if tuple(active.shape) != (K,):
        raise ValueError(f"{name}: active must be {(K,)}, got {tuple(active.shape)}")
    fw, bw = flow_fw.float().contiguous(), flow_bw.float().contiguous()
    idx, act = idx.contiguous(), active.bool().contiguous()
    if not _ext.use_hip(fw):
        out = ref.dense_multi_flow_step(fw, bw, ring_pos, ring_score, idx, act, float(alpha1), float(alpha2))
        return out if cand_err else out[:5] + (None,)
    pos = torch.empty(1, 2, H, W, device=fw.device)
    score, err = torch.empty(1, 1, H, W, device=fw.device), torch.empty(1, 1, H, W, device=fw.device)
    visible = torch.empty(1, 1, H, W, dtype=torch.bool, device=fw.device)
    choice = torch.empty(1, 1, H, W, dtype=torch.int32, device=fw.device)
    cand = torch.empty(K, H, W, device=fw.device) if cand_err else None
    torch.ops.raft_stir.dense_multi_flow_step(fw, bw, ring_pos, ring_score, idx, act, float(alpha1), float(alpha2),
                                              pos, score, visible, choice, err, cand)
    return pos, score, visible, choice, err, cand

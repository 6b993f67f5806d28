"""Forward-backward consistency of two flow fields, dense and at points
(csrc/fb_check.hip on GPU, ATen on CPU and while tracing / exporting)."""
from __future__ import annotations

import torch

from . import _ext
from . import reference as ref


def _flows(name, flow_fw, flow_bw, alpha1, alpha2):
    if flow_fw.dim() != 4 or flow_fw.shape[1] != 2:
        raise ValueError(f"{name}: flow_fw must be (B,2,H,W), got {tuple(flow_fw.shape)}")
    if flow_bw.shape != flow_fw.shape:
        raise ValueError(f"{name}: flow_fw and flow_bw must have the same shape, got {tuple(flow_fw.shape)} "
                         f"and {tuple(flow_bw.shape)}")
    if flow_fw.shape[2] < 2 or flow_fw.shape[3] < 2:
        raise ValueError(f"{name}: H, W >= 2 expected, got {tuple(flow_fw.shape[2:])}")
    if not (alpha1 >= 0 and alpha2 >= 0):
        raise ValueError(f"{name}: alpha1 and alpha2 must be >= 0, got {alpha1} and {alpha2}")
    return flow_fw.float().contiguous(), flow_bw.float().contiguous()


def fb_consistency(flow_fw: torch.Tensor, flow_bw: torch.Tensor, alpha1: float = 0.01, alpha2: float = 0.5):
    """flows (B,2,H,W), any float dtype or layout -> (err (B,1,H,W) fp32,
    ok (B,1,H,W) bool): every pixel follows ``flow_fw``, reads ``flow_bw``
    where it lands and is ok iff it comes home (the rule: ops/reference.py)."""
    fw, bw = _flows("fb_consistency", flow_fw, flow_bw, alpha1, alpha2)
    if _ext.use_hip(fw):
        return torch.ops.raft_stir.fb_consistency(fw, bw, float(alpha1), float(alpha2))
    return ref.fb_consistency(fw, bw, float(alpha1), float(alpha2))


def fb_track_points(flow_fw: torch.Tensor, flow_bw: torch.Tensor, points: torch.Tensor,
                    alpha1: float = 0.01, alpha2: float = 0.5):
    """flows (B,2,H,W), points (B,N,2) xy pixels -> (points + flow_fw at the
    points (B,N,2) fp32, err (B,N) fp32, ok (B,N) bool) in one launch."""
    fw, bw = _flows("fb_track_points", flow_fw, flow_bw, alpha1, alpha2)
    if points.dim() != 3 or points.shape[2] != 2 or points.shape[0] != fw.shape[0] or points.shape[1] < 1:
        raise ValueError(f"fb_track_points: points must be (B,N,2) with B = {fw.shape[0]} and N >= 1, "
                         f"got {tuple(points.shape)}")
    p = points.float().contiguous()
    if _ext.use_hip(fw):
        return tuple(torch.ops.raft_stir.fb_track_points(fw, bw, p, float(alpha1), float(alpha2)))
    return ref.fb_track_points(fw, bw, p, float(alpha1), float(alpha2))

"""Forward interpolation of a flow field for the video warm start
(csrc/forward_interp.hip on GPU, ATen on CPU)."""
from __future__ import annotations

import torch

from . import _ext
from . import reference as ref


def forward_interpolate(flow: torch.Tensor) -> torch.Tensor:
    """flow (2,H,W) or (B,2,H,W), any float dtype -> fp32 of the same shape
    on the same device: every cell takes the flow of the nearest sample after
    each sample has moved by its own flow (the rule: ops/reference.py)."""
    if flow.dim() not in (3, 4) or flow.shape[-3] != 2:
        raise ValueError(f"forward_interpolate: (2,H,W) or (B,2,H,W) expected, got {tuple(flow.shape)}")
    f = flow[None] if flow.dim() == 3 else flow
    f = f.float().contiguous()
    if _ext.use_hip(f):
        out = torch.ops.raft_stir.forward_interpolate(f)
    else:
        out = ref.forward_interpolate(f)
    return out[0] if flow.dim() == 3 else out

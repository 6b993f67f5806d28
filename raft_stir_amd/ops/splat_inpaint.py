"""In-painting of the holes a forward splat leaves: every cell takes the nearest
covered cell within ``max_dist`` as its donor.  The rule and its ATen
implementation are ops/reference.py: splat_inpaint, which runs tensors on the
CPU; tensors on the GPU go to csrc/splat_inpaint.hip (a column pass, a row pass
over packed integer keys and an apply pass), never through eager ATen."""
from __future__ import annotations

import math

import torch

from . import _ext
from . import reference as ref

MAX_SIDE = ref.INPAINT_MAX_SIDE


def radius(max_dist, H: int, W: int) -> int:
    """``max_dist`` as the integer the op takes: None and math.inf mean
    unlimited, which is max(H, W)."""
    if max_dist is None or (isinstance(max_dist, float) and max_dist == math.inf):
        return max(H, W)
    if isinstance(max_dist, bool) or not isinstance(max_dist, int):
        raise ValueError(f"splat_inpaint: max_dist must be an integer, None or math.inf, got {max_dist!r}")
    if not 0 <= max_dist <= MAX_SIDE:
        raise ValueError(f"splat_inpaint: max_dist must be in [0, {MAX_SIDE}], got {max_dist}")
    return max_dist


def splat_inpaint(src_index: torch.Tensor, pos: torch.Tensor, inv_pos: torch.Tensor,
                  values: torch.Tensor | None = None, max_dist: int | float | None = 8, fill: float = 0.0):
    """src_index (1,1,H,W), any integer dtype, and inv_pos (1,2,H,W) as
    ops.forward_splat returns them; pos (1,2,H,W), the field that was
    splatted; values (1,C,H,W) or None; floats of any dtype or layout, on the
    CPU or the GPU; H, W in [2, 32767].  Every cell takes as donor the nearest
    covered cell (``src_index >= 0``) in exact integer Euclidean distance,
    among equals the lowest cell index, if it is within ``max_dist`` cells
    (an integer in [0, 32767]; None or math.inf: unlimited); a covered cell is
    its own donor (the rule: ops/reference.py).
    -> (src_index (1,1,H,W) int32, the donor's anchor pixel, -1 where there is
    none; donor (1,1,H,W) int32, the donor's cell, or -1; dist2 (1,1,H,W)
    int32, the squared distance to it, or -1; inv_pos (1,2,H,W) fp32, unchanged
    at covered cells, at filled cells the donor's anchor pixel extended rigidly
    to the cell, NaN where there is none; out (1,C,H,W) fp32, ``values`` of the
    anchor pixel and ``fill`` where there is none, None without values).  The
    result does not depend on any visiting order, so the kernel's answer is the
    oracle's bit for bit.  On the GPU the call allocates its workspace and
    outputs with torch, launches on the current stream without a host
    synchronisation, and can be captured in a graph."""
    name = "splat_inpaint"
    if src_index.dim() != 4 or src_index.shape[0] != 1 or src_index.shape[1] != 1:
        raise ValueError(f"{name}: src_index must be (1,1,H,W), got {tuple(src_index.shape)}")
    if src_index.is_floating_point() or src_index.is_complex() or src_index.dtype == torch.bool:
        raise ValueError(f"{name}: src_index must be of an integer dtype, got {src_index.dtype}")
    H, W = src_index.shape[2:]
    if not (2 <= H <= MAX_SIDE and 2 <= W <= MAX_SIDE):
        raise ValueError(f"{name}: H, W in [2, {MAX_SIDE}] expected, got {(H, W)}")
    for what, t in (("pos", pos), ("inv_pos", inv_pos)):
        if tuple(t.shape) != (1, 2, H, W):
            raise ValueError(f"{name}: {what} must be {(1, 2, H, W)}, got {tuple(t.shape)}")
    if values is not None and (values.dim() != 4 or values.shape[0] != 1 or values.shape[1] < 1
                               or tuple(values.shape[2:]) != (H, W)):
        raise ValueError(f"{name}: values must be (1,C,H,W) = (1,C,{H},{W}) with C >= 1, got {tuple(values.shape)}")
    R = radius(max_dist, H, W)
    for what, t in (("pos", pos), ("inv_pos", inv_pos), ("values", values)):
        if t is not None and t.device != src_index.device:
            raise ValueError(f"{name}: src_index and {what} must be on the same device, got {src_index.device} and "
                             f"{t.device}")
    if src_index.device.type not in ("cpu", "cuda"):
        raise NotImplementedError(f"{name}: no HIP kernel yet for {src_index.device}; tensors on the CPU or the GPU "
                                  "expected")
    if src_index.device.type == "cpu":
        return ref.splat_inpaint(src_index, pos.float(), inv_pos.float(), None if values is None else values.float(),
                                 R, float(fill))
    # a missing extension is an error, never a quiet run through eager ATen on the device
    _ext.load(raise_on_error=True)
    dev = src_index.device
    # an entry outside int32 is outside [-1, N-1] too: clamped as the rule reads it, before the conversion
    s = src_index if src_index.dtype == torch.int32 else src_index.clamp(-1, H * W - 1).to(torch.int32)
    s, p, i = s.contiguous(), pos.float().contiguous(), inv_pos.float().contiguous()
    v = None if values is None else values.float().contiguous()
    col = torch.empty(H * W, dtype=torch.int32, device=dev)
    donor, dist2, src_out = (torch.empty(1, 1, H, W, dtype=torch.int32, device=dev) for _ in range(3))
    inv_out = torch.empty(1, 2, H, W, device=dev)
    out = None if v is None else torch.empty_like(v)
    torch.ops.raft_stir.splat_inpaint(s, p, i, v, R, float(fill), col, donor, dist2, src_out, inv_out, out)
    return src_out, donor, dist2, inv_out, out

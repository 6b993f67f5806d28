"""Dense forward splatting: for every cell of the frame a dense track field
points to, the anchor pixel that sits there.  The rule and its ATen
implementation are ops/reference.py: forward_splat, which runs tensors on the
CPU; tensors on the GPU go to csrc/forward_splat.hip (a scatter of packed keys
with 64-bit atomicMin and a resolve pass), never through eager ATen."""
from __future__ import annotations

import torch

from . import _ext
from . import reference as ref


def forward_splat(pos: torch.Tensor, score: torch.Tensor, values: torch.Tensor | None = None, footprint: int = 2,
                  fill: float = 0.0):
    """pos (1,2,H,W), channel 0 = x: where every pixel of the anchor frame is
    in the target frame; score (1,1,H,W), finite iff the pixel is visible there
    (DenseMultiFlowTracker's ``pos`` and ``score``); values (1,C,H,W) or None;
    any float dtype or layout, on the CPU or the GPU.  Every visible anchor pixel whose
    position is within a pixel of the image offers itself to its nearest cell
    (``footprint=1``) or to the up-to-four cells its bilinear footprint touches
    (``footprint=2``), and every cell takes the offer of the pixel that lands on
    it before one that only touches it, among those the one of lowest score,
    among equals the lowest anchor index (the rule: ops/reference.py).
    -> (src_index (1,1,H,W) int32, the anchor pixel y*W + x, -1 at holes;
    covered (1,1,H,W) bool; inv_pos (1,2,H,W) fp32, the cell's position in the
    anchor frame, NaN at holes; out (1,C,H,W) fp32, ``values`` of the anchor
    pixel and ``fill`` at holes, None without values).  The result does not
    depend on the order in which the pixels are visited, so the kernel's
    answer is the oracle's bit for bit.  On the GPU the call allocates its
    workspace and outputs with torch, launches on the current stream without
    a host synchronisation, and can be captured in a graph."""
    name = "forward_splat"
    if pos.dim() != 4 or pos.shape[0] != 1 or pos.shape[1] != 2:
        raise ValueError(f"{name}: pos must be (1,2,H,W), got {tuple(pos.shape)}")
    H, W = pos.shape[2:]
    if H < 2 or W < 2:
        raise ValueError(f"{name}: H, W >= 2 expected, got {(H, W)}")
    if tuple(score.shape) != (1, 1, H, W):
        raise ValueError(f"{name}: score must be {(1, 1, H, W)}, got {tuple(score.shape)}")
    if values is not None and (values.dim() != 4 or values.shape[0] != 1 or values.shape[1] < 1
                               or tuple(values.shape[2:]) != (H, W)):
        raise ValueError(f"{name}: values must be (1,C,H,W) = (1,C,{H},{W}) with C >= 1, got {tuple(values.shape)}")
    if footprint not in (1, 2):
        raise ValueError(f"{name}: footprint must be 1 or 2, got {footprint}")
    for what, t in (("score", score), ("values", values)):
        if t is not None and t.device != pos.device:
            raise ValueError(f"{name}: pos and {what} must be on the same device, got {pos.device} and {t.device}")
    if pos.device.type not in ("cpu", "cuda"):
        raise NotImplementedError(f"{name}: no HIP kernel yet for {pos.device}; tensors on the CPU or the GPU expected")
    p, s = pos.float().contiguous(), score.float().contiguous()
    v = None if values is None else values.float().contiguous()
    if pos.device.type == "cpu":
        return ref.forward_splat(p, s, v, int(footprint), float(fill))
    # a missing extension is an error, never a quiet run through eager ATen on the device
    _ext.load(raise_on_error=True)
    dev = p.device
    keys = torch.empty(H * W, dtype=torch.int64, device=dev)
    src_index = torch.empty(1, 1, H, W, dtype=torch.int32, device=dev)
    covered = torch.empty(1, 1, H, W, dtype=torch.bool, device=dev)
    inv_pos = torch.empty(1, 2, H, W, device=dev)
    out = None if v is None else torch.empty_like(v)
    torch.ops.raft_stir.forward_splat(p, s, v, int(footprint), float(fill), keys, src_index, covered, inv_pos, out)
    return src_index, covered, inv_pos, out

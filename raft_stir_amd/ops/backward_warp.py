"""Backward warp of an image through a field of positions.  The rule and its
ATen implementation are ops/reference.py: backward_warp, which runs tensors on
the CPU; tensors on the GPU go to csrc/backward_warp.hip (one launch, one
thread per output cell), never through eager ATen."""
from __future__ import annotations

import numbers

import torch

from . import _ext
from . import reference as ref

_MAX_CELLS = 2 ** 31  # exclusive: a cell index is a 32-bit int in the kernel
_MAX_CHANNELS = 16


def backward_warp(image: torch.Tensor, coords: torch.Tensor, valid: torch.Tensor | None = None, fill=0, out=None):
    """image (1,C,Hs,Ws), fp32 or uint8, 1 <= C <= 16; coords (1,2,H,W), for
    every cell of the output its xy position in the image, of any float dtype
    ((H,W) need not be (Hs,Ws)); valid (1,1,H,W) bool or None -> (warped
    (1,C,H,W) of the image's dtype, ok (1,1,H,W) bool): the bilinear sample of
    the image at every position by ops.dense_query's sampling rule (a tap of
    weight 0 is never read; at an integer position the stored value), rounded
    to the nearest integer, halves to even, for uint8.  ``ok`` is ``valid``
    and the position inside [0,Ws-1]x[0,Hs-1] (NaN, infinities fail); where it
    is false every channel holds ``fill``: a float for fp32, an integer in
    [0,255] for uint8.  The rule: ops/reference.py: backward_warp.  On the CPU
    or the GPU.

    A contiguous image and a channels-last one are read in place; any other
    layout is made contiguous first.  ``out``: (warped, ok) to write into,
    contiguous, of the outputs' dtypes and shapes, on the inputs' device and
    neither an input; they are returned.  On the GPU the call is one launch on
    the current stream without a host synchronisation; with ``out``, fp32
    contiguous coords and a conforming image it allocates nothing and can be
    captured in a graph."""
    name = "backward_warp"
    if image.dim() != 4 or image.shape[0] != 1:
        raise ValueError(f"{name}: image must be (1,C,Hs,Ws), got {tuple(image.shape)}")
    C, Hs, Ws = image.shape[1:]
    if not 1 <= C <= _MAX_CHANNELS:
        raise ValueError(f"{name}: 1 <= C <= {_MAX_CHANNELS} expected, got C = {C}")
    if image.dtype not in (torch.float32, torch.uint8):
        raise ValueError(f"{name}: image must be float32 or uint8, got {image.dtype}")
    if coords.dim() != 4 or coords.shape[0] != 1 or coords.shape[1] != 2:
        raise ValueError(f"{name}: coords must be (1,2,H,W), got {tuple(coords.shape)}")
    H, W = coords.shape[2:]
    for what, h, w in (("Hs, Ws", Hs, Ws), ("H, W", H, W)):
        if h < 2 or w < 2:
            raise ValueError(f"{name}: {what} >= 2 expected, got {(h, w)}")
        if h * w >= _MAX_CELLS:
            raise ValueError(f"{name}: {what}: {h}*{w} = {h * w} must be below 2^31")
    if not coords.is_floating_point():
        raise ValueError(f"{name}: coords must be a float tensor, got {coords.dtype}")
    if valid is not None and (valid.dtype != torch.bool or tuple(valid.shape) != (1, 1, H, W)):
        raise ValueError(f"{name}: valid must be a bool tensor of shape {(1, 1, H, W)}, got {valid.dtype} "
                         f"{tuple(valid.shape)}")
    if image.device.type not in ("cpu", "cuda"):
        raise NotImplementedError(f"{name}: no HIP kernel yet for {image.device}; tensors on the CPU or the GPU "
                                  f"expected")
    for what, t in (("coords", coords), ("valid", valid)):
        if t is not None and t.device != image.device:
            raise ValueError(f"{name}: image and {what} must be on the same device, got {image.device} and "
                             f"{t.device}")
    if image.dtype == torch.uint8:
        if isinstance(fill, bool) or not isinstance(fill, numbers.Integral) or not 0 <= fill <= 255:
            raise ValueError(f"{name}: fill must be an integer in [0, 255] for a uint8 image, got {fill!r}")
        fill = int(fill)
    else:
        fill = float(fill)
    if out is not None:
        out = tuple(out)
        spec = (("warped", image.dtype, (1, C, H, W)), ("ok", torch.bool, (1, 1, H, W)))
        if len(out) != len(spec):
            raise ValueError(f"{name}: out must be (warped, ok), got {len(out)} tensors")
        for t, (what, dt, shape) in zip(out, spec):
            if t.dtype != dt or tuple(t.shape) != shape or not t.is_contiguous() or t.device != image.device:
                raise ValueError(f"{name}: out {what} must be a contiguous {dt} tensor of shape {shape} on "
                                 f"{image.device}, got {t.dtype} {tuple(t.shape)} on {t.device}")
    if not (image.is_contiguous() or image.is_contiguous(memory_format=torch.channels_last)):
        image = image.contiguous()
    coords = coords.float().contiguous()
    if valid is not None:
        valid = valid.contiguous()
    if image.device.type == "cpu":
        res = ref.backward_warp(image, coords, valid, fill)
        if out is None:
            return res
        for o, r in zip(out, res):
            o.copy_(r)
        return out
    # a missing extension is an error, never a quiet run through eager ATen on the device
    _ext.load(raise_on_error=True)
    if out is None:
        out = (torch.empty(1, C, H, W, dtype=image.dtype, device=image.device),
               torch.empty(1, 1, H, W, dtype=torch.bool, device=image.device))
    torch.ops.raft_stir.backward_warp(image, coords, valid, fill, out[0], out[1])
    return out

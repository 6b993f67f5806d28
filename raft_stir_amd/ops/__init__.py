"""Kernel-backed ops. GPU tensors run the in-tree HIP kernels (``_C.so``),
CPU tensors / tracing / export run the ATen references in ``reference.py``."""
from . import _ext, reference
from .corr import AllPairsCorr, OnTheFlyCorr, CorrState, to_nhwc, from_nhwc
from .upsample import convex_upsample, upflow8
from .warm import forward_interpolate
from .fb import fb_consistency, fb_track_points
from .multi_flow import multi_flow_track_points
from .ring import feature_ring_step
from .dense_flow import dense_multi_flow_step
from .forward_splat import forward_splat
from .splat_inpaint import splat_inpaint
from .dense_compose import dense_compose, dense_query
from .backward_warp import backward_warp
from . import gru

__all__ = ["_ext", "reference", "AllPairsCorr", "OnTheFlyCorr", "CorrState", "to_nhwc",
           "from_nhwc", "convex_upsample", "upflow8", "forward_interpolate", "fb_consistency",
           "fb_track_points", "multi_flow_track_points", "feature_ring_step", "dense_multi_flow_step",
           "forward_splat", "splat_inpaint", "dense_compose", "dense_query", "backward_warp",
           "gru"]

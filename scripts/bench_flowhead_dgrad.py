#!/usr/bin/env python
"""The flow head's input gradient (csrc/flowhead.hip flowhead_dgrad_kernel)
alone at the training shape, graph-timed: one call over the 12 x 8 stacked
images (96 x 46 x 62, cin 256, bf16, 512-channel rows) against 12 calls of
8 x 46 x 62, and against a device copy of the same two streams (read
head[..., 0:256], write d_head[..., 0:256]: 140 MB each, 512-channel row
stride), the bandwidth yardstick of profiles/head_batch/README.md.

    python scripts/bench_flowhead_dgrad.py [--blocks N ...]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from bench_small_ops import timeit  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, nargs="*", default=[], help="also time these grid sizes (RS_FH_BLOCKS)")
    a = ap.parse_args()
    from raft_stir_amd.ops import _ext
    _ext.load(raise_on_error=True)
    R = torch.ops.raft_stir
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    B, H, W, IT = 8, 46, 62, 12
    n = B * IT
    head = torch.relu(torch.randn(n, H, W, 512, device=dev)).to(torch.bfloat16)
    dh = torch.zeros(n, H, W, 512, device=dev, dtype=torch.bfloat16)
    w = (torch.randn(2, 256, 3, 3, device=dev) * 0.05).permute(0, 2, 3, 1).contiguous()
    dfl = torch.randn(n, 2, H, W, device=dev)
    mb = 2 * n * H * W * 256 * 2 / 1e6

    def stacked():
        R.flow_head_dgrad(dfl, w, 256, head, 0, dh, 0)

    def per_iteration():
        for i in range(IT):
            s = slice(i * B, (i + 1) * B)
            R.flow_head_dgrad(dfl[s], w, 256, head[s], 0, dh[s], 0)

    per_iteration()
    ref = dh.clone()
    dh.zero_()
    stacked()
    print(f"stacked == per-iteration: {torch.equal(dh, ref)}", flush=True)
    timeit(stacked)  # discarded: the first graph of a process measures ~15 % slow (68 against 59 us)
    us1 = timeit(stacked)
    us12 = timeit(per_iteration, reps=4)
    print(f"flow_head_dgrad 96x46x62 one call   {us1:7.1f} us  {mb / us1:.2f} TB/s", flush=True)
    print(f"flow_head_dgrad 12 x 8x46x62        {us12:7.1f} us  ({us12 / IT:.1f} us per call)", flush=True)
    best = None
    for name, dt in (("8-byte", torch.float64), ("16-byte", torch.complex128)):
        src, dst = head.view(dt), dh.view(dt)
        k = src.shape[-1] // 2
        us = timeit(lambda: dst[..., :k].copy_(src[..., :k]))
        print(f"strided copy, {name:7s} elements      {us:7.1f} us  {mb / us:.2f} TB/s", flush=True)
        best = us if best is None else min(best, us)
    print(f"kernel / copy = {us1 / best:.2f} (target <= 1.25)", flush=True)
    if a.blocks and hasattr(R, "flow_head_set_dgrad_blocks"):
        for nb in a.blocks:
            R.flow_head_set_dgrad_blocks(nb)
            print(f"  grid {nb:5d} blocks: {timeit(stacked):7.1f} us", flush=True)
        R.flow_head_set_dgrad_blocks(0)
        cus = torch.cuda.get_device_properties(0).multi_processor_count
        print(f"  default grid again ({cus} CUs): {timeit(stacked):7.1f} us", flush=True)


if __name__ == "__main__":
    main()

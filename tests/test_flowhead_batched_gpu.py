"""flow_head_dgrad over a stack of images vs the same op one image at a time.

The kernel of csrc/flowhead.hip is persistent: its grid comes from the CU count
(or RS_FH_BLOCKS / flow_head_set_dgrad_blocks), each wave walks the 8-pixel row
segments seg, seg + waves, ... and fetches the next segment while it computes
the current one.  The training engine calls it once over all iters * B images
(models/fused_train.py _HEAD_BATCH), where it used to call it per iteration, so
a stack must give, bit for bit, what the slices give: torch.equal, for cin 128
and 256 (CPL 2 and 4), bf16 and fp32.

Shapes (N, H, W): (3, 5, 11) an odd image count, a full and a partial segment
per row; (2, 4, 7) W shorter than one segment; (1, 1, 8) a single row.  act and
out are channel windows of 512-wide buffers (ooff != 0) filled with a sentinel;
channels outside the window must stay untouched.  With the grid forced to one
block (4 waves) every wave takes several trips and the last trip is partial
((3, 5, 11): 30 segments, waves 0 and 1 take 8, waves 2 and 3 take 7).  One
case holds the stack to the fp64 conv_transpose2d x ReLU-mask oracle of
tests/flow_path_cases.py at the bound of tests/test_flow_path_gpu.py:
2^-19 conv^T(|dflow|, |w|), plus 2^-8 |want| for bf16 storage.
"""
import functools

import pytest
import torch

import flow_path_cases as fc
from flow_path_cases import BF16, F32

pytestmark = pytest.mark.gpu

SHAPES = [(3, 5, 11), (2, 4, 7), (1, 1, 8)]
PITCH = 512
SENTINEL = -77.0  # exact in bf16


@functools.lru_cache(maxsize=None)
def _case(N, H, W, cin, dtype):
    g = torch.Generator().manual_seed(N * 1000 + H * 100 + W * 10 + cin)
    aoff, ooff = PITCH - cin - 8, 8
    act = torch.full((N, H, W, PITCH), SENTINEL, dtype=dtype)
    act[..., aoff:aoff + cin] = fc.fh_act(N, H, W, cin, dtype, g)
    w = 0.05 * torch.randn(2, 3, 3, cin, generator=g)
    dflow = torch.randn(N, 2, H, W, generator=g)
    return act, w, dflow, aoff, ooff


def _run(cuda, case, cin, dtype, per_image):
    act, w, dflow, aoff, ooff = case
    N, H, W = act.shape[:3]
    a, wd, d = act.to(cuda), w.to(cuda), dflow.to(cuda)
    out = torch.full((N, H, W, PITCH), SENTINEL, device=cuda, dtype=dtype)
    if per_image:
        for i in range(N):
            torch.ops.raft_stir.flow_head_dgrad(d[i:i + 1], wd, cin, a[i:i + 1], aoff, out[i:i + 1], ooff)
    else:
        torch.ops.raft_stir.flow_head_dgrad(d, wd, cin, a, aoff, out, ooff)
    return out


def _outside_untouched(out, cin, ooff):
    return bool((out[..., :ooff] == SENTINEL).all()) and bool((out[..., ooff + cin:] == SENTINEL).all())


@pytest.mark.parametrize("dtype", [BF16, F32])
@pytest.mark.parametrize("cin", [128, 256])
@pytest.mark.parametrize("N,H,W", SHAPES)
def test_stack_equals_slices(cuda, N, H, W, cin, dtype):
    case = _case(N, H, W, cin, dtype)
    ref = _run(cuda, case, cin, dtype, per_image=True)
    got = _run(cuda, case, cin, dtype, per_image=False)
    ooff = case[4]
    assert _outside_untouched(ref, cin, ooff) and _outside_untouched(got, cin, ooff)
    assert torch.equal(got, ref)
    assert bool(torch.isfinite(got.float()).all())


@pytest.mark.parametrize("dtype", [BF16, F32])
@pytest.mark.parametrize("cin", [128, 256])
def test_one_block_many_trips(cuda, cin, dtype):
    """RS_FH_BLOCKS = 1: 4 waves walk the 30 segments of (3, 5, 11), the last trip partial.
    Only here does a wave loop and prefetch (at the default grid these shapes get a wave
    per segment), so the result is held to the per-image calls and to the fp64 oracle."""
    N, H, W = SHAPES[0]
    act, w, dflow, aoff, ooff = case = _case(N, H, W, cin, dtype)
    # one image = 10 segments in a grid of 3 blocks (12 waves): a single trip per wave,
    # so the reference does not depend on the loop under test
    ref = _run(cuda, case, cin, dtype, per_image=True)
    torch.ops.raft_stir.flow_head_set_dgrad_blocks(1)
    try:
        got = _run(cuda, case, cin, dtype, per_image=False)
        torch.cuda.synchronize()
    finally:
        torch.ops.raft_stir.flow_head_set_dgrad_blocks(0)
    assert _outside_untouched(got, cin, ooff)
    assert torch.equal(got, ref)
    want, bound = fc.fh_dgrad_oracle(dflow, w, act[..., aoff:aoff + cin])
    if dtype == BF16:
        bound = bound + 2.0 ** -8 * want.abs()
    err = (got[..., ooff:ooff + cin].cpu().double() - want).abs()
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bound).max().item()
    print(f"flow_head_dgrad one block {N, H, W} cin {cin} {dtype}: max|err| {err.max().item():.3e} err/bound {ratio:.3f}")
    assert ratio <= 1.0


@pytest.mark.parametrize("dtype", [BF16, F32])
@pytest.mark.parametrize("cin", [128, 256])
def test_stack_vs_fp64_oracle(cuda, cin, dtype):
    N, H, W = SHAPES[0]
    act, w, dflow, aoff, ooff = case = _case(N, H, W, cin, dtype)
    want, bound = fc.fh_dgrad_oracle(dflow, w, act[..., aoff:aoff + cin])
    if dtype == BF16:
        bound = bound + 2.0 ** -8 * want.abs()
    got = _run(cuda, case, cin, dtype, per_image=False)[..., ooff:ooff + cin].cpu().double()
    err = (got - want).abs()
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bound).max().item()
    print(f"flow_head_dgrad stack {N, H, W} cin {cin} {dtype}: max|err| {err.max().item():.3e} err/bound {ratio:.3f}")
    assert ratio <= 1.0
    masked = ~(act[..., aoff:aoff + cin].double() > 0)
    assert bool((got[masked] == 0).all())


def test_rs_fh_blocks_env_sets_the_grid():
    """RS_FH_BLOCKS in the environment reaches the kernel's grid override when the
    extension loads (ops/_ext.py); the variable is read once, so in a fresh process."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = ("from raft_stir_amd.ops import _ext; import torch; _ext.load(raise_on_error=True); "
            "print('blocks', torch.ops.raft_stir.flow_head_dgrad_blocks())")
    env = dict(os.environ, RS_FH_BLOCKS="7")
    out = subprocess.run([sys.executable, "-c", code], cwd=root, env=env, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    assert "blocks 7" in out.stdout.splitlines(), out.stdout

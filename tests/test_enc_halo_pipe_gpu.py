"""The pipelined tile loop of csrc/enc_halo.hip gives the bits of the plain one.

The pipelined loop (the default; RS_HALO_PIPE=0 or conv3x3_halo_set_pipe(0)
selects the plain one) stages each output row in LDS, stores whole pixels,
prefetches the residual and moves a barrier; the MFMA chain and the fp32
epilogue expressions are the same, so every output element must be bitwise
equal.  The fp64 oracles of test_enc_conv_edges_gpu.py / test_enc_conv_gpu.py
hold either loop to the right answer; this file holds the two to each other at
the shapes where a tile pipeline can go wrong:

  B   H    W   tiles  blocks
  1   8   32      1   1                  no prefetch at all
  1   9   33      4   1 (of 4 tiles)     partial last row and column
  3   9   65     18   5, the last of 2   blocks that cross an image boundary
  3 150  600   1083   91 at 12 tiles per block, the last of 3 (the >= 1024 route)

each for 64 -> 64 and 96 -> 96 channels, with the forward and the transposed,
flipped (input gradient) weight, and with three epilogues: plain; scale /
shift / ReLU / residual / ReLU; accumulate into a pre-filled y.
"""
import pytest
import torch
import torch.nn as nn

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
SHAPES = [(1, 8, 32), (1, 9, 33), (3, 9, 65), (3, 150, 600)]


def _tiles(B, H, W, c):
    """(tiles, tiles per block) as enc_halo_launch picks them."""
    n = B * ((H + 7) // 8) * ((W + 31) // 32)
    gy = c // (64 if c == 64 else 32)
    return n, (12 if n * gy >= 1024 else 4)


def test_shapes_are_the_ones_described():
    assert [_tiles(*s, 64) for s in SHAPES] == [(1, 4), (4, 4), (18, 4), (1083, 12)]
    assert _tiles(3, 150, 600, 96) == (1083, 12)
    assert -(-18 // 4) == 5 and 18 % 4 == 2 and -(-1083 // 12) == 91 and 1083 % 12 == 3


@pytest.fixture
def pipe_switch(cuda):
    yield torch.ops.raft_stir.conv3x3_halo_set_pipe
    torch.ops.raft_stir.conv3x3_halo_set_pipe(-1)  # back to what the environment chose


def _runs(x, wp, c, scale, shift, res, y0):
    """The three epilogues -> three outputs."""
    halo = torch.ops.raft_stir.conv3x3_halo
    plain = torch.empty_like(y0)
    halo(x, wp, plain, c, c)
    full = torch.empty_like(y0)
    halo(x, wp, full, c, c, nscale=scale, nshift=shift, res=res, relu=True)
    accu = y0.clone()
    halo(x, wp, accu, c, c, accumulate=True)
    return plain, full, accu


@pytest.mark.parametrize("c", [64, 96])
@pytest.mark.parametrize("B,H,W", SHAPES)
def test_pipelined_loop_is_bitwise_the_plain_loop(cuda, pipe_switch, B, H, W, c):
    from raft_stir_amd.ops import enc_conv
    g = torch.Generator(device=cuda).manual_seed(1000 * c + H * W + B)
    rnd = lambda *s: torch.randn(*s, device=cuda, generator=g)
    x = (rnd(B, H, W, c) * 0.5).to(BF16)
    res = rnd(B, H, W, c).to(BF16)
    y0 = rnd(B, H, W, c).to(BF16)
    scale, shift = rnd(c) * 0.5 + 1.0, rnd(c) * 0.3
    p = nn.Parameter(rnd(c, c, 3, 3) * 0.05)
    for dgrad in (False, True):
        wp = enc_conv._packed(p, dgrad)
        pipe_switch(0)
        want = _runs(x, wp, c, scale, shift, res, y0)
        pipe_switch(1)
        got = _runs(x, wp, c, scale, shift, res, y0)
        for name, a, b in zip(("plain", "scale/shift/relu/res", "accumulate"), got, want):
            assert bool(torch.isfinite(b.float()).all()) and float(b.float().abs().max()) > 0, name
            assert torch.equal(a, b), (
                f"{c}->{c} {B, H, W} dgrad={dgrad} {name}: {int((a != b).sum())} of {a.numel()} elements differ")

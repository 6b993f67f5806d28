"""The fused training step with the off-chain head kernels issued once per step
(models/fused_train.py _HEAD_BATCH: the mask head's 1x1 conv after the loop,
its input gradient and the flow head's before the backward loop, each over all
iters * B images) against the per-iteration order, from the same weights in
deterministic mode: every prediction and every parameter gradient torch.equal.

RAFT and RAFT-small (no mask head: only flow_head_dgrad moves), bf16 and fp32,
batch 2, 64 x 96 images (an 8 x 12 grid), 3 iterations.  The stacked and the
per-iteration 1x1 convs take the same tile (conv_fused tune_batch), so every
element keeps its K order.
"""
import pytest
import torch

from raft_stir_amd.config import make_args
from raft_stir_amd.models import RAFT
from raft_stir_amd.models import fused_train as ft
from raft_stir_amd.runtime.determinism import deterministic

pytestmark = pytest.mark.gpu

ITERS = 3


def _step(model, batch):
    from raft_stir_amd.train.loss import sequence_loss
    i1, i2, flow, valid = batch
    model.zero_grad(set_to_none=True)
    preds = model(i1, i2, iters=ITERS)
    loss, _ = sequence_loss(preds, flow, valid, 0.8, sync_metrics=False)
    loss.backward()
    torch.cuda.synchronize()
    grads = {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None}
    return [p.detach().clone() for p in preds], grads


@pytest.mark.parametrize("bf16", [True, False], ids=["bf16", "fp32"])
@pytest.mark.parametrize("small", [False, True], ids=["raft", "raft_small"])
def test_head_batch_equals_per_iteration(cuda, monkeypatch, small, bf16):
    from raft_stir_amd.data.synthetic import make_batch
    torch.manual_seed(0)
    m = RAFT(make_args(mixed_precision=bf16, small=small)).to(cuda).to(memory_format=torch.channels_last).train()
    batch = make_batch(2, 64, 96, seed=7, device=cuda)
    calls = {}
    real = ft.conv_fused

    def counted(*a, **k):
        calls[flag] = calls.get(flag, 0) + 1
        return real(*a, **k)

    monkeypatch.setattr(ft, "conv_fused", counted)
    res = {}
    with deterministic():
        for flag in (False, True):
            monkeypatch.setattr(ft, "_HEAD_BATCH", flag)
            res[flag] = _step(m, batch)
    # the fused engine ran, and the switch changed what it issued: RAFT's 2 x ITERS
    # per-iteration mask-head calls became 2
    assert calls[False] > 0
    assert calls[False] - calls[True] == (0 if small else 2 * ITERS - 2)
    (p0, g0), (p1, g1) = res[False], res[True]
    assert len(p0) == len(p1) == ITERS
    for a, b in zip(p0, p1):
        assert bool(torch.isfinite(a).all()) and torch.equal(a, b)
    assert g0.keys() == g1.keys() and len(g0) > 0
    bad = [k for k in g0 if not torch.equal(g0[k], g1[k])]
    assert not bad, bad[:8]
    assert any(float(g.abs().max()) > 0 for k, g in g0.items() if k.startswith("update_block"))

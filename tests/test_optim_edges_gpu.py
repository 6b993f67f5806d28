"""csrc/optim.hip (op clip_adamw_, class FusedClipAdamW) vs the float64 oracle of tests/optim_cases.py.

The op is called directly, so exp_avg, exp_avg_sq, state and moff are the test's
own.  After every call p, m, v and the norm are compared with ONE oracle step
applied to the values that were on the device before that call (no drift, the
bounds are those of a single step); the bounds are derived in the docstring of
tests/optim_cases.py from the kernels' operation order, and
tests/test_optim_oracles_cpu.py shows on the CPU that a numpy fp32 mirror of the
kernels meets them and that ten mutants of it miss them at least tenfold.  Every
check prints max|err| and err / bound and asserts ratio <= 1 and finiteness.
Bit for bit: the gradients after every call; p, m, v after a skipped call; the
moments outside the passed ranges and parameters not passed; the (steps, pending)
state after every call; p == fl(p decay) where g == m == v == 0; two calls on
cloned state.

Cases (optim_cases.CASES; CH = 8192 elements per block, 256 threads, 96 tensors
per group): block and tensor edges in both orders, 200 tiny tensors (one block
over 96 tensors, three groups), 96 / 97 / 192 / 193 tensors with the only large
gradients in the last one, 258 block partials, gradient magnitudes 1e-8 / 1e-20 /
1e4 / 0 beside |p| from 0 to 1e3, max_norm far above / far below / equal to the
fp32 norm / 0, 0..1999 completed steps, lr as a float and a device tensor, lr = 0,
wd = 0, eps 1e-8 and 1e-3, betas (0.5, 0.9), a NaN / +inf / -inf / 1e20 gradient
(first call, between finite calls, twice in a row), a subset of the parameters
(moff with gaps), zero-element tensors and an all-empty list.

Measured on an MI355X (largest err / bound over the calls of each case):
  case               norm   m      v      p        case               norm   m      v      p
  edges_fwd          0.003  0.059  0.065  0.427    steps_99           0.007  0.496  0.597  0.765
  edges_rev          0.021  0.626  0.638  0.865    steps_1999         0.042  0.595  0.594  0.808
  many_tensors       0.003  0.571  0.589  0.782    hyper_lr_tensor    0.018  0.456  0.568  0.755
  groups_96          0.004  0.056  0.051  0.641    hyper_lr_zero      0.015  0.491  0.532  0 (exact)
  groups_97          0.014  0.058  0.054  0.729    hyper_wd_zero      0.022  0.501  0.600  0.366
  groups_192         0.020  0.058  0.053  0.394    hyper_eps_1e-8     0.004  0.592  0.541  0.760
  groups_193         0.008  0.059  0.056  0.438    hyper_eps_1e-3     0.022  0.464  0.633  0.749
  many_partials      0.037  0.100  0.110  0.537    hyper_betas_half   0.012  0.278  0.515  0.684
  magnitudes         0.003  0.500  0.557  0.746    skip_nan           0.043  0.273  0.453  0.575
  clip_above         0.008  0.452  0.571  0.791    skip_pinf          0.004  0.238  0.539  0.639
  clip_below         0.020  0.620  0.311  0.658    skip_ninf          0.015  0.234  0.374  0.508
  clip_at_norm       0.003  0.344  0.556  0.832    skip_sq_overflow   0.077  0.196  0.448  0.599
  clip_none          0.026  0.518  0.569  0.811    subset             0.039  0.527  0.507  0.726
  steps_0            0.002  0.080  0.079  0.214    zero_elems         0.014  0.167  0.246  0.467
  steps_1            0.022  0.563  0.571  0.726    steps_9            0.016  0.491  0.553  0.813
  FusedClipAdamW (channels_last views, three finite steps): norm 0.017  exp_avg 0.388  exp_avg_sq 0.528  p 0.757
  captured step, three replays: norm 0.040  exp_avg 0.482  exp_avg_sq 0.590  p 0.846 (0 at lr = 0: p == fl(p decay))
The kernels agree with the numpy mirror of tests/test_optim_oracles_cpu.py to the printed
digits on nearly every case: the p bound is tight (about 3.5 roundings of |p| are
allowed and 2.5 to 3 happen), not loose.  No bound was missed; every exact requirement held.

Found by this file: FusedClipAdamW.state_dict() put its clones into the LIVE per-parameter
state (torch's Optimizer.state_dict hands out the live dicts), so after the first
state_dict() the exp_avg / exp_avg_sq entries were no longer views of the flat buffers
and every later state_dict() saved the moments of the first one.  Fixed in train/optim.py;
test_fused_clip_adamw_channels_last_views_skip_and_resume calls state_dict() before every step.
"""
import functools
import math

import numpy as np
import pytest
import torch

import optim_cases as oc

pytestmark = pytest.mark.gpu


def _check(name, got, want, bound):
    """max|err| and err / bound (0 / 0 counts as 0: an exact result under a zero bound)."""
    assert got.shape == want.shape, (name, got.shape, want.shape)
    assert bool(np.isfinite(got).all()), name
    err, ratio = oc.ratio(got, want, bound)
    print(f"{name}: max|err| {err:.3e}  err/bound {ratio:.3f}")
    assert ratio <= 1.0, f"{name}: err/bound {ratio:.3f}"
    return ratio


class DeviceBackend:
    """torch.ops.raft_stir.clip_adamw_ behind the interface optim_cases.run_case drives."""

    def __init__(self, dev):
        self.dev = dev

    def load(self, case):
        self.case = case
        dev = self.dev
        self.p = [torch.from_numpy(x.copy()).to(dev) for x in case.p]
        self.m = torch.from_numpy(case.m.copy()).to(dev)
        self.v = torch.from_numpy(case.v.copy()).to(dev)
        self.state = torch.tensor([float(case.steps), 0.0], device=dev)
        self.nparts = oc.nparts_of([case.sizes[i] for i in case.passed])
        self.lr_t = torch.tensor(case.hyper["lr"], device=dev, dtype=torch.float32) if case.lr_tensor else None

    def read(self):
        st = self.state.cpu().tolist()
        return [x.cpu().numpy() for x in self.p], self.m.cpu().numpy(), self.v.cpu().numpy(), (st[0], st[1])

    def call(self, grads):
        c, h = self.case, self.case.hyper
        g = [torch.from_numpy(x).to(self.dev) for x in grads]
        # NaN scratch: a partial that is read without having been written skips the step
        partial = torch.full((self.nparts + 1,), math.nan, device=self.dev)
        norm = torch.ops.raft_stir.clip_adamw_(
            [self.p[i] for i in c.passed], g, self.m, self.v, partial, [c.moff[i] for i in c.passed], self.lr_t,
            0.0 if c.lr_tensor else h["lr"], h["b1"], h["b2"], h["eps"], h["wd"], c.max_norm, self.state)
        assert norm.dtype == torch.float32 and norm.dim() == 0
        for a, b in zip(g, grads):  # the gradients are left unclipped, bit for bit
            assert np.array_equal(a.cpu().numpy().view(np.uint32), b.view(np.uint32)), "gradient changed"
        return float(norm.item())


@functools.lru_cache(maxsize=None)
def _case(name):
    return oc.CASES[name]()


def _hold(records):
    worst = {}
    for rec in records:
        if rec[0] == "exact":
            assert rec[2], rec[1]
            continue
        _, name, got, want, bound = rec
        key = name.split()[-1]
        worst[key] = max(worst.get(key, 0.0), _check(name, got, want, bound))
    return worst


@pytest.mark.parametrize("name", list(oc.CASES))
def test_clip_adamw_case(cuda, name):
    case = _case(name)
    worst = _hold(oc.run_case(case, DeviceBackend(cuda)))
    print(f"worst {name}: " + "  ".join(f"{k} {x:.3f}" for k, x in worst.items()))


@pytest.mark.parametrize("name", ["edges_fwd", "groups_193", "many_partials"])
def test_clip_adamw_is_deterministic(cuda, name):
    case = _case(name)
    outs = []
    for _ in range(2):
        be = DeviceBackend(cuda)
        be.load(case)
        norm = be.call([g.copy() for g in case.calls[0]])
        p, m, v, st = be.read()
        outs.append((np.float32(norm), p, m, v, st))
    a, b = outs
    assert a[0].view(np.uint32) == b[0].view(np.uint32) and a[4] == b[4]
    assert all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(a[1], b[1]))
    assert np.array_equal(a[2].view(np.uint32), b[2].view(np.uint32))
    assert np.array_equal(a[3].view(np.uint32), b[3].view(np.uint32))


@pytest.mark.parametrize("sizes", [[0, 0], []])
def test_clip_adamw_without_elements_launches_nothing(cuda, sizes):
    """Only zero-element tensors (or none): a zero norm, and neither the moments
    nor the state move (the pending flag of the previous call is not folded:
    no kernel ran)."""
    ps = [torch.zeros(n, device=cuda) for n in sizes]
    m = torch.full((7,), 2.0, device=cuda)
    v = torch.full((7,), 3.0, device=cuda)
    state = torch.tensor([4.0, 1.0], device=cuda)
    partial = torch.full((1,), math.nan, device=cuda)
    norm = torch.ops.raft_stir.clip_adamw_(ps, [torch.zeros_like(p) for p in ps], m, v, partial, [7] * len(sizes), None,
                                           1e-3, 0.9, 0.999, 1e-8, 1e-2, 1.0, state)
    assert norm.dtype == torch.float32 and norm.dim() == 0 and norm.item() == 0.0
    assert state.tolist() == [4.0, 1.0] and bool((m == 2).all()) and bool((v == 3).all())
    assert bool(torch.isnan(partial).all())


# ------------------------------------------------------------------ through FusedClipAdamW
def _cl_params(dev, seed):
    g = torch.Generator().manual_seed(seed)
    a = torch.randn(24, 17, 3, 3, generator=g).to(dev).contiguous(memory_format=torch.channels_last)
    b = torch.randn(8, 5, 1, 7, generator=g).to(dev).contiguous(memory_format=torch.channels_last)
    c = torch.randn(37, generator=g).to(dev)
    return [t.requires_grad_() for t in (a, b, c)]


def _np(ts):
    return [t.detach().cpu().contiguous().numpy().reshape(-1) for t in ts]  # logical (row-major) order


def _opt_arrays(opt, ps):
    return (_np(ps), _np([opt.state[p]["exp_avg"] for p in ps]), _np([opt.state[p]["exp_avg_sq"] for p in ps]))


def _hold_step(tag, opt, ps, before, grads, steps_done, hyper, max_norm, norm):
    want = oc.adamw_oracle(before[0], grads, before[1], before[2], steps_done, hyper, max_norm)
    p, m, v = _opt_arrays(opt, ps)
    cat = lambda xs: np.concatenate([np.asarray(x, np.float64) for x in xs])
    _check(f"{tag} norm", np.array([float(norm)]), np.array([want.norm]), np.array([want.e_norm]))
    _check(f"{tag} exp_avg", cat(m), cat(want.m), cat(want.e_m))
    _check(f"{tag} exp_avg_sq", cat(v), cat(want.v), cat(want.e_v))
    _check(f"{tag} p", cat(p), cat(want.p), cat(want.e_p))


def test_fused_clip_adamw_channels_last_views_skip_and_resume(cuda):
    from raft_stir_amd.train.optim import FusedClipAdamW
    hyper = dict(lr=2e-3, b1=0.9, b2=0.999, eps=1e-8, wd=5e-2)
    ps = _cl_params(cuda, 1)
    opt = FusedClipAdamW(ps, lr=hyper["lr"], weight_decay=hyper["wd"], eps=hyper["eps"])
    gen = torch.Generator().manual_seed(2)
    steps = 0
    for k, bad in enumerate([False, False, True, False]):
        # gradients in the OTHER memory format than their parameter: the copy path of _run
        gs = [torch.randn(p.shape, generator=gen).to(cuda) for p in ps]
        if bad:
            gs[1][3, 2, 0, 5] = math.nan
        assert gs[0].stride() != ps[0].stride() and gs[1].stride() != ps[1].stride()
        for p, g in zip(ps, gs):
            p.grad = g
        before = _opt_arrays(opt, ps)
        step_before = float(opt.state_dict()["state"][0]["step"])
        assert step_before == steps
        norm = opt.clip_and_step(1.0)
        for p, g in zip(ps, gs):
            assert p.grad is g  # left in place, unclipped
        # state_dict() above must have left the live entries views of the flat moment buffers
        assert all(opt.state[p]["exp_avg"].data_ptr() == opt._m.data_ptr() + 4 * o
                   and opt.state[p]["exp_avg_sq"].data_ptr() == opt._v.data_ptr() + 4 * o
                   for p, o in zip(ps, opt._moff))
        if bad:
            assert math.isnan(norm.item())
            after = _opt_arrays(opt, ps)
            assert all(np.array_equal(x.view(np.uint32), y.view(np.uint32))
                       for a, b in zip(before, after) for x, y in zip(a, b))
            sd = opt.state_dict()
            assert all(float(sd["state"][i]["step"]) == steps for i in range(len(ps)))
            continue
        _hold_step(f"FusedClipAdamW step {k}", opt, ps, before, _np(gs), steps, hyper, 1.0, norm.item())
        steps += 1
    sd = opt.state_dict()
    assert float(sd["state"][0]["step"]) == 3.0
    qs = [p.detach().clone(memory_format=torch.preserve_format).requires_grad_() for p in ps]
    assert qs[0].stride() == ps[0].stride()
    opt2 = FusedClipAdamW(qs, lr=hyper["lr"], weight_decay=hyper["wd"], eps=hyper["eps"])
    opt2.load_state_dict(sd)
    gs = [torch.randn(p.shape, generator=gen).to(cuda) for p in ps]
    for p, q, g in zip(ps, qs, gs):
        p.grad, q.grad = g.clone(), g.clone()
    n1, n2 = opt.clip_and_step(1.0), opt2.clip_and_step(1.0)
    assert torch.equal(n1, n2)
    for a, b in zip(_opt_arrays(opt, ps), _opt_arrays(opt2, qs)):
        assert all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(a, b))


def test_fused_clip_adamw_captured_step_replays_with_new_lr_and_gradients(cuda):
    from raft_stir_amd.train.optim import FusedClipAdamW
    hyper = dict(lr=1e-3, b1=0.9, b2=0.999, eps=1e-8, wd=1e-2)
    ps = _cl_params(cuda, 5)
    lr = torch.tensor(hyper["lr"], device=cuda)
    opt = FusedClipAdamW(ps, lr=lr, weight_decay=hyper["wd"], eps=hyper["eps"], capturable=True)
    gen = torch.Generator().manual_seed(6)
    for p in ps:  # static gradient buffers with the parameters' strides
        p.grad = torch.empty_like(p).copy_(torch.randn(p.shape, generator=gen))
    s = torch.cuda.Stream(cuda)
    s.wait_stream(torch.cuda.current_stream(cuda))
    with torch.cuda.stream(s):
        opt.clip_and_step(1.0)  # warm-up (uncaptured): one completed step
    torch.cuda.current_stream(cuda).wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        norm = opt.clip_and_step(1.0)
    steps = 1
    for k, new_lr in enumerate([4e-3, 0.0, 7e-4]):
        h = dict(hyper, lr=new_lr)
        lr.fill_(new_lr)
        gs = [torch.randn(p.shape, generator=gen) * (0.1 + k) for p in ps]
        for p, g in zip(ps, gs):
            p.grad.copy_(g)
        before = _opt_arrays(opt, ps)
        graph.replay()
        torch.cuda.synchronize()
        _hold_step(f"graph replay {k} lr {new_lr}", opt, ps, before, _np([p.grad for p in ps]), steps, h, 1.0,
                   norm.item())
        steps += 1
    assert float(opt.state_dict()["state"][0]["step"]) == 4.0

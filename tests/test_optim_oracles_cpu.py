"""The float64 AdamW oracle, its bounds and the fp32 mirror of csrc/optim.hip, on the CPU.

tests/optim_cases.py holds what tests/test_optim_edges_gpu.py checks the kernels
with.  Here, before anything runs on a GPU:

* the oracle equals clip_grad_norm_ + torch.optim.AdamW(foreach=False) on float64
  copies over six steps (rtol 1e-12);
* rounding the hyper-parameters to fp32 moves p by less than a tenth of the GPU
  bound, element by element (measured over four steps: max |dp| 2.5e-10 against
  bounds of about 1.4e-7, ratio at most 0.020; the (1 - b2) rounding cancels
  between v and the bias correction, what is left is the rounding of lr);
* numpy's float32 power is within 1 ulp of float64 (measured 0.97), from which
  optim_cases.K_POW = 4 follows;
* the numpy fp32 mirror of the kernels' operation order stays within every bound
  on every case (largest err / bound: norm 0.08, m 0.63, v 0.64, p 0.87), so the
  bounds are attainable;
* every mutant of the mirror exceeds a bound at least 10 times on a case the GPU
  test runs:

  mutant                       case              check   measured err / bound
  eps_in_sqrt                  magnitudes        p       1.4e6
  eps_before_bc2               hyper_eps_1e-3    p       6.1e4
  l2_decay                     magnitudes        p       2.3e9
  decay_after                  hyper_betas_half  p       1.1e4
  unclipped_moments            clip_below        m       2.2e8
  t_minus_1                    steps_9           p       677
  skip_counted                 skip_nan          p       4.3e3
  coef_no_eps                  clip_at_norm      m       2.7e3
  last_partial_dropped         groups_97         norm    6.1e5
  partials_past_256_dropped    many_partials     norm    1.2e3
"""
import functools
import math

import numpy as np
import pytest
import torch

import optim_cases as oc

MUTANT_CASE = {
    "eps_in_sqrt": ("magnitudes", "p"),
    "eps_before_bc2": ("hyper_eps_1e-3", "p"),
    "l2_decay": ("magnitudes", "p"),
    "decay_after": ("hyper_betas_half", "p"),
    "unclipped_moments": ("clip_below", "m"),
    "t_minus_1": ("steps_9", "p"),
    "skip_counted": ("skip_nan", "p"),
    "coef_no_eps": ("clip_at_norm", "m"),
    "last_partial_dropped": ("groups_97", "norm"),
    "partials_past_256_dropped": ("many_partials", "norm"),
}


@functools.lru_cache(maxsize=None)
def _case(name):
    return oc.CASES[name]()


def _ratios(case, mutant=None):
    """{check (norm / m / v / p): largest err / bound}, and the failed exact requirements."""
    worst, failed = {}, []
    for rec in oc.run_case(case, oc.MirrorBackend(mutant)):
        if rec[0] == "exact":
            if not rec[2]:
                failed.append(rec[1])
            continue
        _, name, got, want, bound = rec
        key = name.split()[-1]
        worst[key] = max(worst.get(key, 0.0), oc.ratio(got, want, bound)[1])
    return worst, failed


def test_oracle_equals_torch_adamw_float64():
    r = np.random.default_rng(0)
    sizes = [37, 129 * 7, 3, 1]
    hyper = dict(lr=3e-3, b1=0.9, b2=0.999, eps=1e-8, wd=1e-2)
    for max_norm in (1.0, 1e6, 0.0):
        p = [r.standard_normal(n) for n in sizes]
        m = [np.zeros(n) for n in sizes]
        v = [np.zeros(n) for n in sizes]
        tp = [torch.tensor(x, dtype=torch.float64, requires_grad=True) for x in p]
        opt = torch.optim.AdamW(tp, lr=hyper["lr"], betas=(hyper["b1"], hyper["b2"]), eps=hyper["eps"],
                                weight_decay=hyper["wd"], foreach=False)
        steps = 0
        for step in range(6):
            g = [r.standard_normal(n) * (0.3 + step) for n in sizes]
            for t, x in zip(tp, g):
                t.grad = torch.tensor(x)
            if max_norm > 0:
                tn = torch.nn.utils.clip_grad_norm_(tp, max_norm, foreach=False)
            opt.step()
            s = oc.adamw_oracle(p, g, m, v, steps, hyper, max_norm, round32=False, bounds=False)
            p, m, v, steps = s.p, s.m, s.v, s.steps_done
            if max_norm > 0:
                assert abs(s.norm - tn.item()) <= 1e-12 * s.norm
            for i, t in enumerate(tp):
                torch.testing.assert_close(torch.tensor(p[i]), t.detach(), rtol=1e-12, atol=0)
                torch.testing.assert_close(torch.tensor(m[i]), opt.state[t]["exp_avg"], rtol=1e-12, atol=1e-16)
                torch.testing.assert_close(torch.tensor(v[i]), opt.state[t]["exp_avg_sq"], rtol=1e-12, atol=0)
        assert steps == 6


def test_oracle_skips_a_nonfinite_norm():
    for bad in oc.NONFINITE.values():
        p, g, m, v = [np.ones(4, oc.F)], [np.array([1, bad, 2, 3], oc.F)], [np.ones(4, oc.F)], [np.ones(4, oc.F)]
        s = oc.adamw_oracle(p, g, m, v, 7, oc.BASE, 1.0)
        assert s.skipped and s.steps_done == 7 and not math.isfinite(s.norm)
        assert np.array_equal(s.p[0], p[0]) and np.array_equal(s.m[0], m[0]) and np.array_equal(s.v[0], v[0])


@pytest.mark.parametrize("scale", [0.3, 1e-8])
def test_fp32_rounding_of_the_hyper_parameters_is_a_tenth_of_the_bound(scale):
    """Four steps from zero moments, each oracle on its own state (the moments must
    come from the same betas for the (1 - b2) rounding to cancel against the bias
    correction).  Measured after the fourth step: max |dp| 2.5e-10 (scale 0.3) and
    1.3e-10 (1e-8) against a median bound of 1.4e-7 / 1.1e-7; the largest
    |dp| / bound of any element is 0.020."""
    r = np.random.default_rng(0)
    n = 4000
    p = [r.standard_normal(n).astype(oc.F)]
    A = B = (p, [np.zeros(n)], [np.zeros(n)])
    for t in range(4):
        g = [(r.standard_normal(n) * scale).astype(oc.F)]
        a = oc.adamw_oracle(A[0], g, A[1], A[2], t, oc.BASE, 0.0)
        b = oc.adamw_oracle(B[0], g, B[1], B[2], t, oc.BASE, 0.0, round32=False, bounds=False)
        A, B = (a.p, a.m, a.v), (b.p, b.m, b.v)
        d = np.abs(a.p[0] - b.p[0])
        print(f"scale {scale} step {t + 1}: max|dp| {d.max():.2e}  largest |dp| / bound {(d / a.e_p[0]).max():.4f}  "
              f"median bound {np.median(a.e_p[0]):.2e}")
        assert float((d / a.e_p[0]).max()) < 0.1


def test_numpy_float32_power_is_within_one_ulp():
    worst = 0.0
    for b in (0.9, 0.999):
        t = np.arange(1, 4097)
        got = np.power(oc.F(b), t.astype(oc.F), dtype=oc.F)
        want = np.power(np.float64(oc.F(b)), t.astype(np.float64))
        ok = want >= 2.0 ** -126
        ulp = np.abs(got.astype(np.float64) - want)[ok] / np.spacing(want[ok].astype(oc.F)).astype(np.float64)
        worst = max(worst, float(ulp.max()))
        assert float(np.abs(got.astype(np.float64) - want)[~ok].max(initial=0.0)) <= 2.0 ** -126
    print(f"float32 power: {worst:.3f} ulp")
    assert worst <= 1.0
    assert oc.K_POW == 4 * math.ceil(worst)


@pytest.mark.parametrize("name", list(oc.CASES))
def test_fp32_mirror_within_every_bound(name):
    worst, failed = _ratios(_case(name))
    print(name, {k: round(x, 3) for k, x in worst.items()})
    assert not failed, failed
    assert all(x <= 1.0 for x in worst.values()), worst


@pytest.mark.parametrize("mutant", oc.MUTANTS)
def test_mutant_exceeds_a_bound_tenfold(mutant):
    name, check = MUTANT_CASE[mutant]
    worst, _ = _ratios(_case(name), mutant)
    print(mutant, name, {k: f"{x:.3g}" for k, x in worst.items()})
    assert math.isfinite(worst[check]) and worst[check] >= 10.0, worst


def test_every_mutant_has_a_case():
    assert set(MUTANT_CASE) == set(oc.MUTANTS)
    assert all(n in oc.CASES for n, _ in MUTANT_CASE.values())

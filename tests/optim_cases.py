"""Cases, float64 oracle, bounds and an fp32 mirror for the fused clip + AdamW
kernels (csrc/optim.hip, op clip_adamw_).  Shared by tests/test_optim_oracles_cpu.py
(oracle vs torch, mirror and mutants vs the bounds) and tests/test_optim_edges_gpu.py
(the kernels vs the same oracle under the same bounds).

Everything here is numpy on the CPU.  A case holds the fp32 values the kernel
reads; :func:`adamw_oracle` works on them in float64 with the hyper-parameters
rounded to fp32 as csrc/ops_optim.cpp passes them.  :func:`run_case` drives a
backend (the mirror here, the device op in the GPU test) call by call and
compares every call with ONE oracle step from the values the backend held before
that call, so no drift accumulates and the bounds are those of a single step.

Bounds (U = 2^-24, the unit roundoff of fp32; TINY = 2^-126 per result that can
underflow, which holds whether denormals are kept or flushed).  They are
derived from the operation order of sumsq_kernel / adamw_kernel; contraction of
a multiply-add into an fma only removes roundings.

norm   sq = sum g^2: every term is non-negative, so the error is relative:
       gamma_L sq, L = 32 (per thread: 32 squares of a CH = 8192 block over 256
       threads, one rounding for the first square and one per addition after it)
       + 6 (butterfly) + 4 (waves) + ceil(nparts / 256) (partials per thread)
       + 6 + 4 (the second block_sum).  norm = sqrtf(sq): half of that plus one
       rounding, evaluated at the ends of the interval of sq.
coef   min(max_norm / (norm + 1e-6), 1): the norm's relative error + 2 roundings
       (min with 1 is 1-Lipschitz).  g' = coef g: one more, r_g in all.
m      3 U (|b1 m| + |(1 - b1) g'|) + (r_g + U) |(1 - b1) g'| + TINY
       (two products and a sum; fl(1 - b1) is exact for b1 >= 0.5, U otherwise).
v      3 U (|b2 v| + |(1 - b2) g'^2|) + (2 r_g + 2 U) |(1 - b2) g'^2| + 2 TINY.
p      pv = p decay, decay = fl(1 - fl(lr wd)): |p| (U lr wd + U/2 + U);
       bc1 = 1 - powf(b1, t): K_POW U b1^t / (1 - b1^t) + U, step_size = lr / bc1
       one more; bc2_sqrt the same with b2, halved under the root, + U;
       sqrtf(v) at the ends of v's interval + U; the quotient, the + eps, m / denom
       and step_size * (.) one rounding each with m's error carried through;
       the final subtraction U (|pv| + |u|).
K_POW  4: numpy's float32 power is within 1 ulp of float64 for b in {0.9, 0.999},
       t = 1..4096 (measured 0.97, tests/test_optim_oracles_cpu.py); device math
       libraries document a few ulp for powf, so 4 times that.
All first-order terms are multiplied by 1 + 2^-10 for the second-order ones.
"""
import math
from dataclasses import dataclass, field
from typing import List, Optional

import numpy as np

F = np.float32
CH, THREADS, MAXT = 8192, 256, 96
U = 2.0 ** -24
TINY = 2.0 ** -126
K_POW = 4.0
SLACK = 1.0 + 2.0 ** -10
CLIP_EPS = 1e-6

BASE = dict(lr=3e-3, b1=0.9, b2=0.999, eps=1e-8, wd=1e-2)


def f32(x):
    return float(F(x))


def hyper32(h):
    """The hyper-parameters as the kernel sees them: (float) casts in ops_optim.cpp."""
    return {k: f32(v) for k, v in h.items()}


# ----------------------------------------------------------------- launch structure
def groups_of(sizes):
    """Indices of the non-empty tensors, MAXT per launch group (ops_optim.cpp)."""
    idx = [i for i, n in enumerate(sizes) if n > 0]
    return [idx[k:k + MAXT] for k in range(0, len(idx), MAXT)]


def nparts_of(sizes):
    return sum(-(-sum(sizes[i] for i in g) // CH) for g in groups_of(sizes))


def norm_chain(sizes):
    return 32 + 6 + 4 + -(-nparts_of(sizes) // THREADS) + 6 + 4


# ----------------------------------------------------------------- oracle + bounds
@dataclass
class Step:
    p: list
    m: list
    v: list
    norm: float
    steps_done: int
    skipped: bool
    coef: float = 1.0
    # bounds (None after a skipped step: everything is bit-unchanged)
    e_norm: float = 0.0
    e_p: Optional[list] = None
    e_m: Optional[list] = None
    e_v: Optional[list] = None


def adamw_oracle(params, grads, m, v, steps_done, hyper, max_norm, round32=True, bounds=True):
    """One clip + AdamW step in float64.  params / grads / m / v: lists of arrays
    (the fp32 values the kernel reads).  Returns a :class:`Step`; a non-finite
    norm leaves everything unchanged and steps_done does not advance."""
    h = hyper32(hyper) if round32 else dict(hyper)
    mx = f32(max_norm) if round32 else float(max_norm)
    ce = f32(CLIP_EPS) if round32 else CLIP_EPS
    P = [np.asarray(x, np.float64) for x in params]
    G = [np.asarray(x, np.float64) for x in grads]
    M = [np.asarray(x, np.float64) for x in m]
    V = [np.asarray(x, np.float64) for x in v]
    with np.errstate(all="ignore"):
        # the kernel's squares are fp32: |g| > sqrt(FLT_MAX) is an infinite square there
        sq64 = sum(float(np.sum(g * g)) for g in G)
        over = any(bool(np.any(np.abs(g) > math.sqrt(float(np.finfo(F).max)))) for g in G)
    norm = math.sqrt(sq64) if sq64 >= 0 and not math.isnan(sq64) else math.nan
    if over and not math.isnan(norm):
        norm = math.inf
    if not math.isfinite(norm):
        return Step(P, M, V, norm, steps_done, True)
    clip = mx > 0
    x = mx / (norm + ce) if clip else 1.0
    coef = min(x, 1.0)
    lr, b1, b2, eps, wd = h["lr"], h["b1"], h["b2"], h["eps"], h["wd"]
    t = steps_done + 1
    bc1, bc2 = 1.0 - b1 ** t, 1.0 - b2 ** t
    ss, bc2s = lr / bc1, math.sqrt(bc2)
    out = Step([], [], [], norm, t, False, coef)
    if bounds:
        sizes = [g.size for g in G]
        L = norm_chain(sizes)
        e_sq = L * U / (1 - L * U) * sq64 + sum(sizes) * TINY
        hi, lo = math.sqrt(sq64 + e_sq), math.sqrt(max(sq64 - e_sq, 0.0))
        out.e_norm = SLACK * (max(hi - norm, norm - lo) + U * hi)
        r_x = out.e_norm / norm + 2 * U if clip and norm > 0 else 0.0
        # x (1 - r_x) >= 1: the kernel's quotient is clamped to exactly 1 as well
        r_coef = 0.0 if not clip or x * (1 - r_x) >= 1 else r_x * x / coef
        r_g = r_coef + U
        r_bc1 = K_POW * U * b1 ** t / bc1 + U
        r_ss = r_bc1 + U
        r_bc2s = 0.5 * (K_POW * U * b2 ** t / bc2 + U) + U
        u_b1 = 0.0 if b1 >= 0.5 else U
        u_b2 = 0.0 if b2 >= 0.5 else U
        out.e_p, out.e_m, out.e_v = [], [], []
    for p, g, mm, vv in zip(P, G, M, V):
        gp = coef * g
        pv = p * (1.0 - lr * wd)
        mn = b1 * mm + (1.0 - b1) * gp
        vn = b2 * vv + (1.0 - b2) * gp * gp
        den = np.sqrt(vn) / bc2s + eps
        u = ss * mn / den
        out.p.append(pv - u)
        out.m.append(mn)
        out.v.append(vn)
        if bounds:
            am, ag = np.abs(b1 * mm), np.abs((1.0 - b1) * gp)
            e_m = 3 * U * (am + ag) + (r_g + U + u_b1) * ag + TINY
            av, ag2 = np.abs(b2 * vv), (1.0 - b2) * gp * gp
            e_v = 3 * U * (av + ag2) + (2 * r_g + 2 * U + u_b2) * ag2 + 2 * TINY
            sv = np.sqrt(vn)
            shi, slo = np.sqrt(vn + e_v), np.sqrt(np.maximum(vn - e_v, 0.0))
            e_sv = np.maximum(shi - sv, sv - slo) + U * shi
            q = sv / bc2s
            e_q = e_sv / bc2s + q * (r_bc2s + U)
            e_den = e_q + U * den
            den_lo = den - e_den
            assert bool(np.all(den_lo > 0))
            r = np.abs(mn) / den
            e_r = (e_m + np.abs(mn) * e_den / den) / den_lo + U * r
            e_u = np.abs(u) * (r_ss + U) + ss * e_r
            e_pv = np.abs(p) * (U * lr * wd + 0.5 * U + U)
            e_p = e_pv + e_u + U * (np.abs(pv) + np.abs(u)) + TINY
            out.e_p.append(SLACK * e_p)
            out.e_m.append(SLACK * e_m)
            out.e_v.append(SLACK * e_v)
    return out


# ----------------------------------------------------------------- fp32 mirror
MUTANTS = ("eps_in_sqrt", "eps_before_bc2", "l2_decay", "decay_after", "unclipped_moments", "t_minus_1",
           "skip_counted", "coef_no_eps", "last_partial_dropped", "partials_past_256_dropped")


def _wave_sum(a):
    """block_sum of optim.hip on a [256] fp32 vector: xor butterfly per wave, then the 4 waves in order."""
    a = a.reshape(THREADS // 64, 64)
    lane = np.arange(64)
    o = 32
    while o:
        a = a + a[:, lane ^ o]
        o >>= 1
    t = F(0)
    for w in range(THREADS // 64):
        t = F(t + a[w, 0])
    return t


def mirror_partials(sizes, grads):
    """sumsq_kernel: one fp32 partial per block of every group, in the kernel's order."""
    parts = []
    for grp in groups_of(sizes):
        off = np.cumsum([0] + [sizes[i] for i in grp])
        for e0 in range(0, int(off[-1]), CH):
            e1 = min(e0 + CH, int(off[-1]))
            acc = np.zeros(THREADS, F)
            for k, i in enumerate(grp):
                s, te = max(e0, int(off[k])), min(e1, int(off[k + 1]))
                if s >= te:
                    continue
                seg = grads[i].reshape(-1)[s - off[k]:te - off[k]]
                sq = np.zeros(-(-seg.size // THREADS) * THREADS, F)
                with np.errstate(over="ignore", invalid="ignore"):
                    sq[:seg.size] = seg * seg
                    for row in sq.reshape(-1, THREADS):
                        acc = acc + row
            with np.errstate(over="ignore", invalid="ignore"):
                parts.append(_wave_sum(acc))
    return np.array(parts, F)


def _final_sum(parts):
    """adamw_kernel's sum of all partials: thread i takes i, i + 256, ..., then block_sum."""
    acc = np.zeros(THREADS, F)
    pad = np.zeros(-(-parts.size // THREADS) * THREADS, F)
    pad[:parts.size] = parts
    for row in pad.reshape(-1, THREADS):
        acc = acc + row
    return _wave_sum(acc)


def mirror_step(sizes, p, g, m, v, state, hyper, max_norm, mutant=None):
    """The two kernels in numpy fp32, operation by operation (no fma).  p, g, m, v:
    lists of fp32 arrays; state: (steps, pending).  Returns (p, m, v, state, norm)."""
    h = {k: F(x) for k, x in hyper.items()}
    one = F(1)
    steps = F(state[0] + state[1])  # sumsq_kernel folds the pending flag
    parts = mirror_partials(sizes, g)
    if mutant == "last_partial_dropped":
        parts = parts[:-1]
    if mutant == "partials_past_256_dropped":
        parts = parts[:THREADS]
    with np.errstate(over="ignore", invalid="ignore"):
        norm = np.sqrt(_final_sum(parts))
    if not np.isfinite(norm):
        return p, m, v, (float(steps), 1.0 if mutant == "skip_counted" else 0.0), float(norm)
    t = steps if mutant == "t_minus_1" else F(steps + one)
    with np.errstate(all="ignore"):
        bc1 = one - np.power(h["b1"], t, dtype=F)
        bc2s = np.sqrt(one - np.power(h["b2"], t, dtype=F))
        mx = F(max_norm)
        coef = one
        if max_norm > 0:
            coef = np.minimum(mx / (norm if mutant == "coef_no_eps" else norm + F(CLIP_EPS)), one)
        lr, wd, eps = h["lr"], h["wd"], h["eps"]
        decay = one - lr * wd
        ss = lr / bc1
        ob1, ob2 = one - h["b1"], one - h["b2"]
        P, M, V = [], [], []
        for pp, gg, mm, vv in zip(p, g, m, v):
            gv = gg * coef
            gm = gg if mutant == "unclipped_moments" else gv
            if mutant == "l2_decay":
                gm = gm + wd * pp
            pv = pp if mutant in ("l2_decay", "decay_after") else pp * decay
            mv = h["b1"] * mm + ob1 * gm
            vn = h["b2"] * vv + ob2 * gm * gm
            if mutant == "eps_in_sqrt":
                den = np.sqrt(vn + eps * eps) / bc2s
            elif mutant == "eps_before_bc2":
                den = (np.sqrt(vn) + eps) / bc2s
            else:
                den = np.sqrt(vn) / bc2s + eps
            pv = pv - ss * (mv / den)
            if mutant == "decay_after":
                pv = pv * decay
            P.append(pv.astype(F))
            M.append(mv.astype(F))
            V.append(vn.astype(F))
    return P, M, V, (float(steps), 1.0), float(norm)


# ----------------------------------------------------------------- cases
@dataclass
class Case:
    name: str
    sizes: List[int]               # every parameter the moment buffers hold
    p: list
    m: np.ndarray                  # flat moment buffers (fp32)
    v: np.ndarray
    calls: list                    # per call: list of gradient arrays (one per PASSED parameter)
    passed: List[int]              # indices of the parameters handed to the op
    moff: List[int]                # flat moment offset of every parameter in `sizes`
    steps: int = 0
    hyper: dict = field(default_factory=lambda: dict(BASE))
    max_norm: float = 1.0
    lr_tensor: bool = False
    zero_state: List[int] = field(default_factory=list)  # passed params with g == m == v == 0 (exact result)


def _rng(name):
    return np.random.default_rng(sum(ord(c) * (i + 1) for i, c in enumerate(name)))


def _mk(name, sizes, gscale=1.0, steps=0, max_norm=1.0, hyper=None, passed=None, ncalls=1, pscale=1.0,
        lr_tensor=False, gap=0):
    """Random case: p ~ N(0, pscale), g ~ N(0, gscale[i]); with steps > 0 the moments are those of a
    stationary gradient of the same scale (m ~ g, v ~ g^2 >= 0), else zero."""
    r = _rng(name)
    gs = gscale if isinstance(gscale, (list, tuple)) else [gscale] * len(sizes)
    passed = list(range(len(sizes))) if passed is None else passed
    moff, o = [], gap
    for n in sizes:
        moff.append(o)
        o += n + gap
    p = [(r.standard_normal(n) * pscale).astype(F) for n in sizes]
    m, v = np.zeros(o, F), np.zeros(o, F)
    if steps > 0 or gap:
        for n, s, mo in zip(sizes, gs, moff):
            m[mo:mo + n] = (r.standard_normal(n) * s * 0.5).astype(F)
            v[mo:mo + n] = ((r.standard_normal(n) * s) ** 2).astype(F)
        if gap:  # recognisable values in the gaps, which no call may touch
            mask = np.ones(o, bool)
            for n, mo in zip(sizes, moff):
                mask[mo:mo + n] = False
            m[mask], v[mask] = F(-7.25), F(3.5)
    calls = [[(r.standard_normal(sizes[i]) * gs[i]).astype(F) for i in passed] for _ in range(ncalls)]
    return Case(name, list(sizes), p, m, v, calls, passed, moff, steps, dict(hyper or BASE), max_norm, lr_tensor)


EDGE_SIZES = [8192, 1, 8191, 8193, 3, 16384, 5]


def _group_case(nt):
    # the only large gradients are in the last tensor: the norm decides whether
    # every group's partials were summed, and coef (clipping active) shows in m
    c = _mk(f"groups_{nt}", [5] * nt, gscale=[1e-3] * (nt - 1) + [1e3], max_norm=1.0)
    return c


def _magnitudes():
    n = 257
    c = _mk("magnitudes", [n, n, n, n], gscale=[1e-8, 1e-20, 1e4, 0.0], steps=9, max_norm=0.0)
    r = _rng("magnitudes_p")
    for i in range(4):  # p == 0, tiny and up to 1e3 beside every gradient magnitude
        mag = 10.0 ** r.uniform(-6, 3, n)
        mag[::7] = 0.0
        mag[1] = 1e3
        c.p[i] = (mag * r.choice([-1.0, 1.0], n)).astype(F)
    o = c.moff[3]
    c.m[o:o + n] = 0
    c.v[o:o + n] = 0
    c.zero_state = [3]
    return c


def _clip_case(which):
    c = _mk(f"clip_{which}", [300, 7], gscale=1e-5, steps=3)
    if which == "above":
        c.max_norm = 1e3
    elif which == "below":
        c.max_norm = 1e-9
    elif which == "none":
        c.max_norm = 0.0
    else:  # max_norm = the fp32 norm the kernel's order of operations gives: coef just under 1
        c.max_norm = float(np.sqrt(_final_sum(mirror_partials(c.sizes, c.calls[0]))))
    return c


def _hyper_case(tag):
    h = dict(BASE)
    kw = {}
    if tag == "lr_tensor":
        kw["lr_tensor"] = True
    elif tag == "lr_zero":
        h["lr"] = 0.0
    elif tag == "wd_zero":
        h["wd"] = 0.0
    elif tag == "eps_1e-3":
        h["eps"] = 1e-3
    elif tag == "betas_half":  # with a decay large enough to tell decay-before from decay-after the update
        h.update(b1=0.5, b2=0.9, lr=0.05, wd=0.2)
    c = _mk(f"hyper_{tag}", [700, 3], gscale=[0.3, 1e-6], steps=9, hyper=h, **kw)
    c.p[0][::5] = 0
    return c


NONFINITE = {"nan": math.nan, "pinf": math.inf, "ninf": -math.inf, "sq_overflow": 1e20}


def _skip_case(kind):
    """97 tensors (the bad element in the one tensor of the last group); calls: bad (the very first
    step), finite, bad, bad (twice in a row), finite."""
    c = _mk(f"skip_{kind}", [5] * 97, ncalls=5)
    for k in (0, 2, 3):
        c.calls[k][96][3] = F(NONFINITE[kind])
    return c


def _zero_elems():
    c = _mk("zero_elems", [5, 0, 9, 0], steps=2)
    return c


CASES = {
    "edges_fwd": lambda: _mk("edges_fwd", EDGE_SIZES),
    "edges_rev": lambda: _mk("edges_rev", EDGE_SIZES[::-1], steps=1),
    "many_tensors": lambda: _mk("many_tensors", [(1, 3, 37, 2)[i % 4] for i in range(200)], steps=4),
    **{f"groups_{n}": (lambda n=n: _group_case(n)) for n in (96, 97, 192, 193)},
    "many_partials": lambda: _mk("many_partials", [257 * CH, 3], max_norm=50.0),
    "magnitudes": _magnitudes,
    **{f"clip_{w}": (lambda w=w: _clip_case(w)) for w in ("above", "below", "at_norm", "none")},
    **{f"steps_{s}": (lambda s=s: _mk(f"steps_{s}", [700, 3], steps=s)) for s in (0, 1, 9, 99, 1999)},
    **{f"hyper_{t}": (lambda t=t: _hyper_case(t)) for t in ("lr_tensor", "lr_zero", "wd_zero", "eps_1e-8", "eps_1e-3",
                                                           "betas_half")},
    **{f"skip_{k}": (lambda k=k: _skip_case(k)) for k in NONFINITE},
    "subset": lambda: _mk("subset", [10, 8192, 7, 300, 4], passed=[0, 2, 3], steps=5, gap=3),
    "zero_elems": _zero_elems,
}


# ----------------------------------------------------------------- driver
class MirrorBackend:
    """The fp32 mirror behind the interface run_case drives (the GPU test has the device op behind it)."""

    def __init__(self, mutant=None):
        self.mutant = mutant

    def load(self, case):
        self.case = case
        self.p = [x.copy() for x in case.p]
        self.m, self.v = case.m.copy(), case.v.copy()
        self.state = (float(case.steps), 0.0)

    def read(self):
        return [x.copy() for x in self.p], self.m.copy(), self.v.copy(), self.state

    def call(self, grads):
        c = self.case
        sz = [c.sizes[i] for i in c.passed]
        sl = [slice(c.moff[i], c.moff[i] + c.sizes[i]) for i in c.passed]
        P, M, V, self.state, norm = mirror_step(sz, [self.p[i] for i in c.passed], grads, [self.m[s] for s in sl],
                                                [self.v[s] for s in sl], self.state, c.hyper, c.max_norm, self.mutant)
        for k, i in enumerate(c.passed):
            self.p[i], self.m[sl[k]], self.v[sl[k]] = P[k], M[k], V[k]
        return norm


def _bits(a, b):
    a, b = np.ascontiguousarray(a, F), np.ascontiguousarray(b, F)
    return a.shape == b.shape and bool(np.array_equal(a.view(np.uint32), b.view(np.uint32)))


def run_case(case, backend):
    """Drive `backend` through the case's calls.  Returns records:
    ("bound", name, got, want, bound) -- float64 arrays, to be held to |got - want| <= bound, got finite;
    ("exact", name, ok)               -- a bit-for-bit requirement."""
    rec = []
    backend.load(case)
    c = case
    sl = [slice(c.moff[i], c.moff[i] + c.sizes[i]) for i in c.passed]
    steps_done = c.steps  # counted here, not read back: a finite call advances it, a skipped one does not
    for k, grads in enumerate(c.calls):
        p0, m0, v0, st0 = backend.read()
        want = adamw_oracle([p0[i] for i in c.passed], grads, [m0[s] for s in sl], [v0[s] for s in sl],
                            steps_done, c.hyper, c.max_norm)
        norm = backend.call([g.copy() for g in grads])
        p1, m1, v1, st1 = backend.read()
        tag = f"{c.name} call {k}"
        untouched = np.ones(m0.size, bool)
        for s in sl:
            untouched[s] = False
        rec.append(("exact", f"{tag} moments outside the passed ranges",
                    _bits(m0[untouched], m1[untouched]) and _bits(v0[untouched], v1[untouched])))
        rec.append(("exact", f"{tag} parameters not passed",
                    all(_bits(p0[i], p1[i]) for i in range(len(p0)) if i not in c.passed)))
        rec.append(("exact", f"{tag} state", tuple(st1) == (float(steps_done), 0.0 if want.skipped else 1.0)))
        steps_done = want.steps_done
        if want.skipped:
            same = math.isnan(norm) if math.isnan(want.norm) else norm == want.norm
            rec.append(("exact", f"{tag} norm {want.norm}", same))
            rec.append(("exact", f"{tag} skipped: p, m, v bit-unchanged",
                        all(_bits(a, b) for a, b in zip(p0, p1)) and _bits(m0, m1) and _bits(v0, v1)))
            continue
        rec.append(("bound", f"{tag} norm", np.array([norm], np.float64), np.array([want.norm]),
                    np.array([want.e_norm])))
        cat = lambda xs: np.concatenate([np.asarray(x, np.float64).reshape(-1) for x in xs]) if xs else np.zeros(0)
        rec.append(("bound", f"{tag} m", cat([m1[s] for s in sl]), cat(want.m), cat(want.e_m)))
        rec.append(("bound", f"{tag} v", cat([v1[s] for s in sl]), cat(want.v), cat(want.e_v)))
        rec.append(("bound", f"{tag} p", cat([p1[i] for i in c.passed]), cat(want.p), cat(want.e_p)))
        for j in c.zero_state:  # g == m == v == 0: p is exactly fl(p decay)
            i = c.passed[j]
            lr, wd = F(c.hyper["lr"]), F(c.hyper["wd"])
            d2 = F(1) - lr * wd                                   # two roundings
            d1 = F(1.0 - float(lr) * float(wd))                   # contracted into one fma
            ok = _bits(p1[i], p0[i] * d2) or _bits(p1[i], p0[i] * d1)
            rec.append(("exact", f"{tag} p == fl(p decay) where g == m == v == 0", ok))
    return rec


def ratio(got, want, bound):
    """max err / bound (0 / 0 = 0), inf for a non-finite result."""
    if got.size == 0:
        return 0.0, 0.0
    if not np.all(np.isfinite(got)):
        return math.inf, math.inf
    err = np.abs(got - want)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, 0.0, err / bound)
    return float(err.max()), float(r.max())

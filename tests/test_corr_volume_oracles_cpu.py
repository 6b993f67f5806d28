"""tests/corr_volume_cases.py on its own: the fp64 oracles against float64 autograd, a plain
emulation of every route inside every bound at every case of the table, every mutant outside
it on at least one case, and the launch mirrors tied to the kernel sources (no GPU)."""
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import corr_volume_cases as V
from corr_volume_cases import BF16, F32, F64

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "raft_stir_amd", "csrc")
B = 2


def _src(name):
    path = os.path.join(CSRC, name) if not name.endswith(".py") else os.path.join(os.path.dirname(CSRC), "ops", name)
    with open(path) as f:
        return f.read()


def _fwd_cases(route):
    """(kind, N1, H2, W2, levels, C) of the case table for one route."""
    ch = V.CHANNELS[route]
    for N1, H, W, L, k in V.fwd_pairs():
        yield "randn", N1, H, W, L, ch[k]
    for i, (kind, N1, H, W, L) in enumerate(V.VALUE_CASES):
        yield kind, N1, H, W, L, ch[i % 3]


def _bwd_cases():
    for N1, H, W in V.BWD_SHAPES:
        for C in (128, 256):
            for dt in (BF16, F32):
                yield N1, H, W, V.max_levels(H, W), C, dt


# ------------------------------------------------------------------ oracles vs float64 autograd
@pytest.mark.parametrize("H,W,L", [(9, 15, 4), (8, 8, 4), (5, 13, 3), (1, 5, 1)])
def test_oracles_match_autograd(H, W, L):
    N1, C, scale = 7, 8, 0.25
    g = V.gen(H, W, L)
    f1 = torch.randn(B, N1, C, generator=g, dtype=F64, requires_grad=True)
    f2 = torch.randn(B, H, W, C, generator=g, dtype=F64, requires_grad=True)
    gp = [torch.randn(B, N1, h, w, generator=g, dtype=F64) for h, w in V.level_sizes(H, W, L)]
    pyr = V.pyramid(f1, f2, L, scale)
    loss = sum((gl * v).sum() for gl, (v, _) in zip(gp, pyr))
    d1, d2 = torch.autograd.grad(loss, (f1, f2))
    G0, Wf = V.fold(gp, scale)
    o1, o2, T1, T2 = V.backward(G0, f1.detach(), f2.detach())
    torch.testing.assert_close(o1, d1, rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(o2, d2, rtol=1e-12, atol=1e-12)
    assert bool((Wf >= G0.abs() - 1e-15).all()) and bool((T1 >= o1.abs() - 1e-12).all()) and bool((T2 >= o2.abs() - 1e-12).all())
    # the fold is the gradient with respect to the unscaled level-0 product
    m = torch.randn(B, N1, H, W, generator=g, dtype=F64, requires_grad=True)
    v, loss = V.f32(scale) * m, 0
    for l in range(L):
        if l:
            v = F.avg_pool2d(v, 2, 2)
        loss = loss + (gp[l] * v).sum()
    torch.testing.assert_close(G0, torch.autograd.grad(loss, m)[0], rtol=1e-12, atol=1e-12)
    # A_l bounds |vol_l| and the pooled sizes are floor sizes
    for (v, A), (h, w) in zip(pyr, V.level_sizes(H, W, L)):
        assert v.shape == (B, N1, h, w) and bool((A >= v.detach().abs() - 1e-12).all())


# ------------------------------------------------------------------ emulations inside the bounds
@pytest.mark.parametrize("route,out_bf16", [("exact", False), ("flat_bf16", False), ("flat_bf16", True), ("flat_split", False)])
def test_volume_emulation_inside_bounds(route, out_bf16):
    dt, worst, n = V.ROUTE_DTYPE[route], {}, 0
    for kind, N1, H, W, L, C in _fwd_cases(route):
        assert V.volume_route(dt, C) == route and V.volume_accepts(dt, C)
        f1, f2 = V.features(B, N1, H, W, C, dt, kind)
        scale = C ** -0.5
        got = V.emulate_volume(f1, f2, L, scale, route, out_bf16)
        for l, (want, A) in enumerate(V.pyramid(f1, f2, L, scale)):
            r = V.ratio(got[l], want, V.vol_bound(route, l, C, A, want, out_bf16))
            worst[l] = max(worst.get(l, 0.0), r)
            n += 1
            assert r <= 1.0, (route, kind, N1, H, W, C, l, r)
    print(f"{route} out_bf16={out_bf16}: {n} checks, largest err/bound per level " +
          " ".join(f"L{l} {r:.3f}" for l, r in sorted(worst.items())))


def test_fold_emulation_inside_bounds():
    worst = {False: 0.0, True: 0.0}
    for name, b, N1, H, W, L, *_ in V.FOLD_CASES + V.FOLD_BIG[1:]:
        for mag in V.GRAD_SCALES if N1 < 100 else (1.0,):
            gp = V.grad_pyramid(b, N1, H, W, L, mag)
            want, Wf = V.fold(gp, 0.125)
            for ob in (False, True):
                r = V.ratio(V.emulate_fold(gp, 0.125, ob), want, V.fold_bound(Wf, want, ob))
                worst[ob] = max(worst[ob], r)
                assert r <= 1.0, (name, mag, ob, r)
    print(f"fold: largest err/bound in place {worst[False]:.3f}, bf16 out {worst[True]:.3f}")


def test_backward_emulation_inside_bounds():
    worst = {}
    for N1, H, W, L, C, dt in _bwd_cases():
        f1, f2 = V.features(B, N1, H, W, C, dt)
        gp = V.grad_pyramid(B, N1, H, W, L)
        scale = C ** -0.5
        G0, _ = V.fold(gp, scale)
        w1, w2, T1, T2 = V.backward(G0, f1, f2)
        g1, g2 = V.emulate_backward(gp, f1, f2, scale)
        split = dt == F32
        r1 = V.ratio(g1, w1, V.bwd_bound(split, H * W, T1, w1))
        r2 = V.ratio(g2, w2, V.bwd_bound(split, N1, T2, w2))
        worst[dt] = (max(worst.get(dt, (0, 0))[0], r1), max(worst.get(dt, (0, 0))[1], r2))
        assert r1 <= 1.0 and r2 <= 1.0, (N1, H, W, C, dt, r1, r2)
    for dt, (r1, r2) in worst.items():
        print(f"backward {dt}: largest err/bound df1 {r1:.3f} df2 {r2:.3f}")


# ------------------------------------------------------------------ mutants
_FWD_JUDGES = {"ceil_parent": ("exact", "flat_bf16", "flat_split"), "no_quarter": ("exact", "flat_bf16", "flat_split"),
               "row_copy": ("exact", "flat_bf16", "flat_split"), "batch": ("exact", "flat_bf16", "flat_split"),
               "hi_only": ("flat_split",), "double_round": ("flat_bf16",)}


@pytest.mark.parametrize("name", V.FWD_MUTANTS)
def test_forward_mutant_leaves_its_bound(name):
    for route in _FWD_JUDGES[name]:
        dt, best = V.ROUTE_DTYPE[route], (0.0, None)
        for kind, N1, H, W, L, C in _fwd_cases(route):
            if N1 < 2:
                continue
            f1, f2 = V.features(B, N1, H, W, C, dt, kind)
            scale = C ** -0.5
            mut = V.mutant_volume(name, f1, f2, L, scale)
            for l, (want, A) in enumerate(V.pyramid(f1, f2, L, scale)):
                r = V.ratio(mut[l], want, V.vol_bound(route, l, C, A))
                if r > best[0]:
                    best = (r, (kind, N1, H, W, L, C, l))
            if best[0] > 1.0:
                break
        print(f"forward mutant {name} on {route}: err/bound {best[0]:.3g} at {best[1]}")
        assert best[0] > 1.0, (name, route, best)


@pytest.mark.parametrize("name", V.FOLD_MUTANTS)
@pytest.mark.parametrize("out_bf16", [False, True])
def test_fold_mutant_leaves_its_bound(name, out_bf16):
    best = (0.0, None)
    for case, b, N1, H, W, L, *_ in V.FOLD_CASES:
        gp = V.grad_pyramid(b, N1, H, W, L)
        want, Wf = V.fold(gp, 0.125)
        r = V.ratio(V.fold(gp, 0.125, name)[0], want, V.fold_bound(Wf, want, out_bf16))
        if r > best[0]:
            best = (r, case)
    print(f"fold mutant {name} bf16={out_bf16}: err/bound {best[0]:.3g} at {best[1]}")
    assert best[0] > 1.0, (name, best)


@pytest.mark.parametrize("name", V.BWD_MUTANTS)
def test_backward_mutant_leaves_its_bound(name):
    for dt in (F32,) if name == "hi_only" else (BF16, F32):
        best = (0.0, None)
        for N1, H, W, L, C, d in _bwd_cases():
            if d != dt or N1 < 2:
                continue
            f1, f2 = V.features(B, N1, H, W, C, dt)
            G0, _ = V.fold(V.grad_pyramid(B, N1, H, W, L), C ** -0.5)
            w1, w2, T1, T2 = V.backward(G0, f1, f2)
            m1, m2 = V.mutant_backward(name, G0, f1, f2)
            r = max(V.ratio(m1, w1, V.bwd_bound(dt == F32, H * W, T1, w1)),
                    V.ratio(m2, w2, V.bwd_bound(dt == F32, N1, T2, w2)))
            if r > best[0]:
                best = (r, (N1, H, W, C))
        print(f"backward mutant {name} {dt}: err/bound {best[0]:.3g} at {best[1]}")
        assert best[0] > 1.0, (name, dt, best)


# ------------------------------------------------------------------ mirrors tied to the sources
def _one(pattern, text):
    m = re.findall(pattern, text)
    assert len(m) >= 1, pattern
    assert len(set(m)) == 1, (pattern, m)
    return m[0]


def test_mirror_constants_equal_the_sources():
    lk, vol, bwd, ops, py = (_src(n) for n in ("corr_lookup.hip", "corr_volume.hip", "corr_bwd.hip", "ops.cpp", "corr.py"))
    assert int(_one(r"constexpr int FW_LDS = (\d+);", lk)) == V.FW_LDS
    assert int(_one(r"constexpr int FOLD_LDS = (\d+);", lk)) == V.FOLD_LDS
    assert "__shared__ float cl[4][FW_LDS];" in lk and "__shared__ float cl[FOLD_LDS];" in lk
    assert _one(r"opitch <= (64 \* 4 \* 12) &&", lk) == "64 * 4 * 12" and V.WAVE_PITCH_MAX == 3072
    assert int(_one(r"opitch % 4 == 0 && opitch <= (\d+) && coarse <= lookup::FOLD_LDS", lk)) == V.ROWS_PITCH_MAX
    assert "coarse <= lookup::FW_LDS" in lk
    assert (int(_one(r"if \(qw <= (\d+)\) RS_FW\(4\);", lk)), int(_one(r"else if \(qw <= (\d+)\) RS_FW\(8\);", lk))) == V.QW_STEPS
    assert "else RS_FW(12);" in lk and "const int qw = (opitch + 255) / 256;" in lk
    assert int(_one(r"std::min<long>\(rows, (\d+)\)", lk)) == V.FOLD4_GRID_Y
    assert "constexpr int QPT = 6;" in lk  # 6 quads x 256 threads x 4 = 6144
    assert int(_one(r"constexpr int FB = (\d+);", vol)) == V.FB
    assert tuple(int(_one(rf"constexpr int {n} = (\d+);", vol)) for n in ("BM", "TH", "TW")) == V.EXACT_BLOCK
    assert tuple(int(x) for x in _one(r"constexpr int BM = (\d+), BN = (\d+), BK = (\d+);", bwd)) == (V.BWD_BM, V.BWD_BN, V.BWD_BK)
    assert "int corr_bwd_pitch(int N2) { return round_up(N2, cgemm::BK); }" in bwd
    a, b_ = _one(r"Ss\[l\] = \(Hs\[l\] \* Ws\[l\] \+ (\d+)\) / (\d+) \* \d+;", ops)
    assert int(a) + 1 == int(b_) == V.VOL_PITCH
    assert tuple(int(x) for x in _one(r"const bool rowfold = Ep <= (\d+) && coarse <= (\d+);", ops)) == V.BWD_ROWFOLD
    assert tuple(int(x) for x in _one(r"row_fold = Ep <= (\d+) and coarse <= (\d+)", py)) == V.BWD_ROWFOLD
    assert int(_one(r"Ep = -\(-\(H2 \* W2\) // (\d+)\) \* \d+", py)) == V.BWD_BK
    assert "split_f32_volume() && (3 * C) % 64 == 0" in ops
    assert 'TORCH_CHECK(C % (is_bf16(f1) ? 64 : 32) == 0' in ops
    assert 'TORCH_CHECK(C % 128 == 0, "corr_volume_backward' in ops
    assert V.ROWS_PITCH_MAX == V.BWD_ROWFOLD[0] and V.FOLD_LDS == V.BWD_ROWFOLD[1]
    # the shape checks bwd_route repeats
    assert "TORCH_CHECK(rowfold || (!split && Ss[0] % 4 == 0 && (uintptr_t)gpyr[0].data_ptr() % 16 == 0)," in ops
    assert ("TORCH_CHECK((int64_t)B * N1 * Ep * 2 < (int64_t(1) << 31) && "
            "(int64_t)B * std::max(N1, N2) * C * 2 < (int64_t(1) << 31),") in ops


def test_case_tables_reach_every_route():
    for route, chans in V.CHANNELS.items():
        assert {V.volume_route(V.ROUTE_DTYPE[route], C) for C in chans} == {route}
    grids, n1s = {}, {}
    for N1, H, W, L, _ in V.fwd_pairs():
        grids[(H, W)] = grids.get((H, W), 0) + 1
        n1s[N1] = n1s.get(N1, 0) + 1
        assert all(h > 0 and w > 0 for h, w in V.level_sizes(H, W, L))
    assert set(grids) == {g[:2] for g in V.GRIDS} and min(grids.values()) >= 2
    assert set(n1s) == set(V.N1S) and min(n1s.values()) >= 2
    seen = set()
    for name, b, N1, H, W, L, store, inplace, bf in V.FOLD_CASES + V.FOLD_BIG:
        E = H * W
        S, coarse = V.fold_pitch(E, store), V.coarse_cells(H, W, L)
        assert V.fold_route(E, S, True, coarse, 0, False) == inplace, name
        assert V.fold_route(E, S, True, coarse, 0, True) == bf, name
        seen |= {inplace, bf}
    assert seen >= {"wave4", "wave8", "wave12", "rows(vec0=1)", "rows(vec0=0)", "fold4", "fold4(vec_out=0)", "flat"}
    assert V.coarse_cells(48, 64, 4) == 1008 and V.coarse_cells(48, 66, 4) > V.FW_LDS
    # backward: bf16 takes the wave fold into the padded G, fp32 the row fold with a lo half
    for N1, H, W in V.BWD_SHAPES:
        L = V.max_levels(H, W)
        for dt, want in ((BF16, "wave"), (F32, "rows")):
            for S in (V.round_up(H * W, 64), H * W):
                r = V.bwd_route(B, N1, H, W, 128, dt, V.coarse_cells(H, W, L), S, True)
                assert r["ok"] and r["rowfold"] and r["Ep"] == V.round_up(H * W, 64)
                assert r["fold"].startswith(want if S % 4 == 0 else "rows"), (N1, H, W, dt, S, r)
    N1, H, W = V.BWD_QUAD
    S = V.round_up(H * W, 64)
    q = V.bwd_route(B, N1, H, W, 128, BF16, V.coarse_cells(H, W, 4), S, True)
    assert q["ok"] and not q["rowfold"] and q["fold"] == "fold4(vec_out=1)" and q["Ep"] == 6336
    assert not V.bwd_route(B, N1, H, W, 128, F32, V.coarse_cells(H, W, 4), S, True)["ok"]
    assert V.bwd_route(B, 127, 10, 13, 128, BF16, 0, 192, True)["Ep"] == 192


def test_quad_row_is_the_integer_division():
    """The float row index of the wave and rows kernels, every W0 they can see and every quad."""
    e = np.arange(0, 6144, 4, dtype=np.int64)
    for w0 in range(1, 6145, 512):
        W0 = np.arange(w0, min(w0 + 512, 6145), dtype=np.int64)[:, None]
        assert np.array_equal(V.quad_row(e[None, :], W0), (e[None, :] // W0).astype(np.int32)), w0
    assert e[-1] == 6140


class _FakeLevel:
    def __init__(self, N1, h, w, S, ptr):
        self.shape, self._S, self._ptr = (B, N1, h, w), S, ptr

    def stride(self, i):
        assert i == 1
        return self._S

    def data_ptr(self):
        return self._ptr


def test_fused_bwd_ok_agrees_with_the_op_checks():
    from raft_stir_amd.ops.corr import _fused_bwd_ok
    n = 0
    for Bn in (1, 2, 48):
        for N1 in (1, 130, 6288, 22816):
            for H, W in ((1, 1), (10, 13), (48, 128), (48, 131), (96, 128), (184, 124)):
                for C in (64, 128, 192, 256):
                    for dt in (BF16, F32, torch.float16):
                        for S_extra, ptr in ((0, 4096), (2, 4096), (0, 4100)):
                            L = V.max_levels(H, W)
                            S = H * W + S_extra
                            gp = [_FakeLevel(N1, h, w, S if l == 0 else h * w, ptr)
                                  for l, (h, w) in enumerate(V.level_sizes(H, W, L))]
                            got = _fused_bwd_ok(gp, Bn, N1, H, W, C, dt == BF16, dt == F32)
                            want = V.bwd_route(Bn, N1, H, W, C, dt, V.coarse_cells(H, W, L), S, ptr % 16 == 0)["ok"]
                            assert bool(got) == want, (Bn, N1, H, W, C, dt, S, ptr)
                            n += 1
    assert n > 1000


# ------------------------------------------------------------------ the chain's lookup oracle
@pytest.mark.parametrize("r", [3, 4])
def test_lookup_oracle_matches_reference_and_chain(r):
    """V.lookup equals ops/reference.py corr_lookup where every level is wider than one cell, and
    the raw gradient pyramid of the lookups, folded, gives the chain's feature gradients."""
    from raft_stir_amd.ops import reference as ref
    H, W, L, C, scale = 9, 15, 3, 8, 0.25
    g = V.gen(H, W, r)
    f1 = torch.randn(B, H * W, C, generator=g, dtype=F64, requires_grad=True)
    f2 = torch.randn(B, H, W, C, generator=g, dtype=F64, requires_grad=True)
    c = V.chain_coords(H, W, 0)
    w = torch.randn(B, H, W, L * (2 * r + 1) ** 2, generator=g, dtype=F64)
    pyr = [v for v, _ in V.pyramid(f1, f2, L, scale)]
    got = V.lookup(pyr, c, r)
    want = ref.corr_lookup([v.reshape(B * H * W, 1, *v.shape[2:]) for v in pyr], c.double(), r).permute(0, 2, 3, 1)
    torch.testing.assert_close(got, want, rtol=1e-11, atol=1e-11)
    d1, d2 = torch.autograd.grad((got * w).sum(), (f1, f2))
    leaves = [v.detach().requires_grad_() for v in pyr]
    gp = torch.autograd.grad((V.lookup(leaves, c, r) * w).sum(), leaves)
    o1, o2, _, _ = V.backward(V.fold(gp, scale)[0], f1.detach(), f2.detach())
    torch.testing.assert_close(o1, d1, rtol=1e-11, atol=1e-11)
    torch.testing.assert_close(o2, d2, rtol=1e-11, atol=1e-11)

"""The oracles, bounds, launch mirrors and mutants of tests/update_conv_cases.py (no GPU).

1. every oracle equals float64 autograd of the plain composite (conv -> gate -> state
   update for the GRU epilogues, F.conv2d(...).backward for the gradients);
2. the launch mirrors agree with the kernel files and ops/conv.py;
3. a plain fp32 evaluation of each operation stays inside its bound at every case of
   tests/test_update_conv_edges_gpu.py, so no bound is too tight for a correct kernel;
4. eight mutants of the oracles exceed the bound at every shape of the GPU file at which
   the mutation changes the result at all, and the shape lists hold, for each mutant, shapes
   at which it does (a one-pixel image has no border tap to drop and no row to wrap into).
"""
import os
import re

import pytest
import torch
import torch.nn.functional as F

import update_conv_cases as C
from update_conv_cases import BF16, F32, F64

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TILES = C.tiles_under_test()
ALL_FWD_SHAPES = sorted(set(C.PATCH_SHAPES + C.FLAT_SHAPES + [(1, 1, 1), (2, 9, 1)]))


def _src(name):
    with open(os.path.join(ROOT, "raft_stir_amd", "csrc", name)) as f:
        return f.read()


# ------------------------------------------------------------------ 1. oracles = autograd
@pytest.mark.parametrize("kh,kw", C.KERNELS)
def test_conv_taps_is_the_conv2d_oracle(kh, kw):
    for shape in [(1, 1, 1), (2, 9, 1), (3, 5, 13), (1, 9, 33)]:
        x, w, bias, want, A = C.fwd_case(*shape, kh, kw)
        got = C.conv_taps(x, w, kh, kw) + bias.double()
        assert C.ratio(got, want, 16 * 2.0 ** -53 * A) <= 1.0
        # the planted output cancels to 2^-20 of its magnitude
        p = C.plant_pixel(*shape)
        assert 0.5 * C.E20 < (want[p][0] / A[p][0]).item() < 2.0 * C.E20


def test_plant_is_the_gate_tests_plant():
    text = open(os.path.join(ROOT, "tests", "test_gates_gpu.py")).read()
    m = re.search(r"^PLANT = (\[.*\])$", text, re.M)
    assert m and eval(m.group(1)) == C.PLANT


def test_gru_forward_epilogues_are_the_composite():
    e = C.epi_case(2, 5, 7, 3, 3)
    hd = C.EPI_HD
    pre = e["pre"]
    zero = torch.zeros_like(pre)
    (z, _), (rh, _), (r, _) = C.epi_gru_zr(pre, zero, e["h"][..., :hd], hd)
    torch.testing.assert_close(z, torch.sigmoid(pre[..., :hd]))
    torch.testing.assert_close(rh, torch.sigmoid(pre[..., hd:]) * e["h"][..., :hd].double())
    (hn, _), (q, _) = C.epi_gru_q(pre[..., :hd], zero[..., :hd], e["h"][..., :hd], e["z"][..., :hd])
    zz = e["z"][..., :hd].double()
    torch.testing.assert_close(hn, (1 - zz) * e["h"][..., :hd].double() + zz * torch.tanh(pre[..., :hd]))
    assert bool((q.abs() <= 1).all())
    # exact saturation at the planted +-1e4 / +-100
    assert z[..., 9].min() == 1.0 and z[..., 10].max() == 0.0


def test_backward_epilogues_equal_autograd():
    """EPI_GRU_QBWD: v = dL/d(r h) and dL/dx of the q conv's input cat[r h, x]: dr_pre and
    the accumulation into dh are autograd's through r = sigmoid(r_pre), rh = r h.
    EPI_RELU_BWD: autograd through relu, the mask read from the ReLU's output."""
    g = C.gen(5)
    hd, n = 8, 12
    v = torch.randn(3, n, generator=g, dtype=F64)
    h = torch.randn(3, hd, generator=g, dtype=F64, requires_grad=True)
    rp = torch.randn(3, hd, generator=g, dtype=F64, requires_grad=True)
    o0 = torch.randn(3, n, generator=g, dtype=F64)
    r = torch.sigmoid(rp)
    ((r * h) * v[:, :hd]).sum().backward()
    (out, _), (dr, _) = C.epi_gru_qbwd(v, torch.zeros_like(v), h.detach(), r.detach(), o0, hd)
    torch.testing.assert_close(dr, rp.grad)
    torch.testing.assert_close(out[:, :hd], o0[:, :hd] + h.grad)
    torch.testing.assert_close(out[:, hd:], o0[:, hd:] + v[:, hd:])
    a = torch.randn(3, n, generator=g, dtype=F64, requires_grad=True)
    y = torch.relu(a)
    (y * v).sum().backward()
    want, _ = C.epi_relu_bwd(v, torch.zeros_like(v), y.detach())
    torch.testing.assert_close(want, a.grad)
    want, _ = C.epi_acc_f32(v, torch.zeros_like(v), o0)
    torch.testing.assert_close(want, o0 + v)


def test_gru_gate_bwd_oracle_equals_autograd():
    g = C.gen(6)
    s = (2, 3, 8)
    zp, qp, h = (torch.randn(*s, generator=g, dtype=F64, requires_grad=True) for _ in range(3))
    dh = torch.randn(*s, generator=g, dtype=F64)
    z, q = torch.sigmoid(zp), torch.tanh(qp)
    (((1 - z) * h + z * q) * dh).sum().backward()
    (dq, _), (dz, _), (dhn, _) = C.gru_gate_bwd_oracle(dh, z.detach(), q.detach(), h.detach())
    torch.testing.assert_close(dq, qp.grad)
    torch.testing.assert_close(dz, zp.grad)
    torch.testing.assert_close(dhn, h.grad)


@pytest.mark.parametrize("kh,kw", C.KERNELS)
def test_wgrad_oracle_equals_autograd(kh, kw):
    for stack in [(3, 2, 1, 5), (2, 1, 9, 1), (3, 1, 5, 13)]:
        c = C.wgrad_case(*stack, kh, kw)
        x = C.nchw(C.stack_x(c["x0"], c["xb"], c["x2"], stack[0]))
        w = torch.zeros(C.COUT_MAX, C.WG_KTOT, kh, kw, dtype=F64, requires_grad=True)
        b = torch.zeros(C.COUT_MAX, dtype=F64, requires_grad=True)
        F.conv2d(x, w, b, 1, (kh // 2, kw // 2)).backward(C.nchw(c["dy"]))
        torch.testing.assert_close(c["dw"], w.grad)
        torch.testing.assert_close(c["db"], b.grad)
        assert C.kernel_layout(c["dw"]).shape == (C.COUT_MAX, kh * kw, C.WG_KTOT)
        # the broadcast segment repeats image b = stack index mod B
        assert bool((C.stack_x(c["x0"], c["xb"], c["x2"], stack[0])[:, 0, 0, C.WG_SEG].float()
                     == (torch.arange(stack[0] * stack[1]) % stack[1] + 1)).all())


def test_relu_take_oracle():
    G, actv = C.relu_take_case(160, 80, BF16)
    out, Gn = C.relu_take_oracle(G, 32, 80, 96, actv, 8, 96)
    a = actv[..., 8:88].double()
    torch.testing.assert_close(out[..., :80], torch.where(a > 0, G[..., 32:112].double(), torch.zeros_like(a)))
    assert bool((out[..., 80:] == 0).all()) and bool((Gn[..., 32:128] == 0).all())
    assert torch.equal(Gn[..., :32], G[..., :32]) and torch.equal(Gn[..., 128:], G[..., 128:])
    assert bool((out[..., :80][a == 0] == 0).all())  # 0.0 and -0.0 are not positive


# ------------------------------------------------------------------ 2. launch mirrors
def test_tile_list_comes_from_the_table_and_the_heuristic():
    from raft_stir_amd.ops import conv as oc
    tuned = set(C.tuned_table().values())
    assert tuned and tuned <= set(TILES) and C.choose_tile_range() <= set(TILES)
    assert C.choose_tile_range() == {5, 17, 29, 16, 41, 4, 3}  # every return choose_tile reaches (31: behind _WIDE bits 1, 2)
    fams = {C.tile_geom(t)["family"] for t in TILES}
    assert fams == set(C.FAMILIES)
    assert any(9 <= t <= 15 for t in TILES)  # conv_glds_kernel
    assert {t for t in TILES if C.tile_geom(t)["family"] == "v3"} <= set(oc.V3_TILES)
    assert oc.GEMM1_TILE == 70
    assert (C.EPI_BIAS, C.EPI_GRU_QBWD, C.EPI_FLOW) == (oc.EPI_BIAS, oc.EPI_GRU_QBWD, oc.EPI_FLOW)


def test_launch_mirrors_reproduce_the_kernel_files():
    conv, v3 = _src("conv.hip"), _src("conv_v3.h")
    # conv_launch's template arguments: <BM, BN, ...> of the tiles the mirror lists
    for tile, bm, bn in re.findall(r"case (\d+): RS_BUF8?K?\((\d+), (\d+),", conv):
        g = C.tile_geom(int(tile))
        assert (g["family"], g["bm"], g["px"]) == ("buf", int(bm), int(bn)), tile
    for tile, bm, bn, bk in re.findall(r"case (\d+): RS_GLDS\((\d+), (\d+), (\d+),", conv):
        g = C.tile_geom(int(tile))
        assert (g["family"], g["bm"], g["px"], g["bk"]) == ("glds", int(bm), int(bn), int(bk)), tile
    assert "default: RS_BUFK(64, 64, 2, 4); break;  // 37" in conv and C.tile_geom(37)["kg"] == 4
    assert "conv_lds_kernel<64, 64, 2, 2, 32, false, false, 4>" in conv and C.tile_geom(41)["kg"] == 4
    assert "conv_halo_kernel<64, 8, 192>" in conv and C.tile_geom(25)["patch"] == (8, 16)
    assert "conv_halo_kernel<128, 4, 128>" in conv and C.tile_geom(26)["hcap"] == 128
    for tile, nwm, thw, nwp in re.findall(r"case (\d+): \*nwm = (\d); \*thw = (\d);(?: \*nwp = (\d);)?", v3):
        g = C.tile_geom(int(tile))
        assert (g["bm"], g["patch"]) == (32 * int(nwm), (int(thw) * int(nwp or 1), 32)), tile
    assert "constexpr int BM = 128, BN = 128;" in _src("conv_gemm1.hip")
    assert C.tile_geom(54)["bm"] == 192 and C.tile_geom(43)["patch"] == (8, 32) and C.tile_geom(52)["bm"] == 256
    # K depth: 3x3 over 192 channels
    assert C.fwd_chain(3, 9, 192, True) == 2 * 54 + 1       # 16x16x32, 32-deep steps
    assert C.fwd_chain(17, 9, 192, False) == 2 * 54         # 64-deep staged step = two MFMAs
    assert C.fwd_chain(41, 9, 192, False) == 2 * 14 + 3     # 54 steps over 4 groups, 3 adds
    assert C.fwd_chain(34, 9, 192, False) == 2 * 2 * 14 + 1 and C.fwd_chain(37, 5, 192, False) == 2 * 2 * 4 + 3
    assert C.fwd_chain(5, 9, 192, True) == 2 * 14 + 3 + 1
    assert C.fwd_chain(61, 9, 192, False) == 2 * 108 == C.fwd_chain(45, 9, 192, False)  # 32x32x16
    assert C.fwd_chain(70, 1, 192, False) == 2 * 12
    # host constraints
    assert not C.tile_accepts(70, 3, 3, (64, 128), 96) and C.tile_accepts(70, 1, 1, (64, 128), 96)
    assert not C.tile_accepts(61, 1, 1, (64, 128), 96) and not C.tile_accepts(61, 3, 3, (32, 64, 96), 96)
    assert not C.tile_accepts(5, 3, 3, (64, 128), 32) and C.tile_accepts(5, 3, 3, (32, 64, 96), 16)
    assert not C.tile_accepts(17, 3, 3, (32, 64, 96), 96) and C.tile_accepts(41, 3, 3, (32, 64, 96), 96)
    assert C.tile_accepts(26, 5, 1, (64, 128), 96) and C.tile_accepts(24, 5, 1, (64, 128), 96)
    # weight gradients: wgrad_plan, wgrad3_splits, colsum_blocks
    assert C.wgrad_variant(1, 64) == (0, 64, 64, 256) and C.wgrad_variant(3, 70) == (3, 256, 128, 512)
    assert C.wgrad_variant(5, 200) == (5, 64, 128, 256) and C.wgrad_variant(2, 200, False) == (0, 128, 64, 256)
    assert C.wgrad_plan(1188, 9, 384, 200, False, 0) == (3, 448) and C.wgrad_plan(1188, 9, 384, 200, True, 3) == (3, 448)
    assert C.wgrad_plan(1, 1, 384, 64, False, 0) == (1, 64)
    assert C.wgrad_plan(274000, 5, 384, 256, False, 0) == (18, 15232) and C.wgrad_plan(274000, 1, 384, 64, True, 0) == (32, 8576)
    assert C.wgrad_chain(1188, 9, 384, 200, False, 0) == 2 * 2 * 7 + 3 + 1
    assert C.wgrad_bias_chain(1188, 9, 384, 200, False, 2) == 2 * 7 + 32 + 3 + 1
    assert C.wgrad3_splits(4, 9, 33, 200, 384, 64) == (21, 2) and C.wgrad3_splits(96, 46, 62, 256, 384, 64) == (21, 110)
    assert C.wgrad3_splits(1, 1, 1, 64, 384, 128) == (1, 1) and C.wgrad3_chain(96, 46, 62, 256, 384, 64) == 2 * 8 * 110 + 21
    assert "static int wg3_th(int) { return 4; }" in _src("wgrad_v3.hip")
    assert C.colsum_blocks(1) == 1 and C.colsum_blocks(257) == 2 and "return cdiv(P, 256); }" in _src("conv_wgrad.hip")
    assert C.colsum_chain(1188) == 256 + 5 + 1


def test_relu_take_rejects_a_zero_window_wider_than_out():
    assert re.search(r"nz <= out\.size\(-1\)", _src("ops_conv.cpp"))


# ------------------------------------------------------------------ 3. plain fp32 under the bounds
def _chains(kh, kw, cout):
    """The distinct forward chains among the tiles that run this (kernel, Cout)."""
    out = set()
    for t in TILES:
        chans = (32, 64, 96) if C.tile_geom(t)["bk"] == 32 else (64, 128)
        if C.tile_accepts(t, kh, kw, chans, cout):
            out.add(C.fwd_chain(t, kh * kw, C.KTOT, True))
    return sorted(out)


def _f32_conv(x, w, b, kh, kw):
    y = F.conv2d(x.float().permute(0, 3, 1, 2), w.float(), None if b is None else b.float(), 1, (kh // 2, kw // 2))
    return y.permute(0, 2, 3, 1)


@pytest.mark.parametrize("kh,kw", C.KERNELS)
def test_fp32_reference_under_the_forward_bounds(kh, kw):
    worst = 0.0
    for shape in ALL_FWD_SHAPES:
        x, w, bias, want, A = C.fwd_case(*shape, kh, kw)
        got = _f32_conv(x, w, bias, kh, kw).to(BF16)
        for cout in C.FWD_COUTS + C.SMALLN_COUTS:
            for c in _chains(kh, kw, cout):
                r = C.ratio(got[..., :cout], want[..., :cout], C.acc_bound(c, A[..., :cout]), BF16)
                worst = max(worst, r)
                assert r <= 1.0, (shape, cout, c, r)
    print(f"forward {kh}x{kw}: plain fp32, bf16 output: {worst:.3f} of the bound")
    assert worst > 0.5  # the half ulp of bf16


def _epi_f32(e, kind, hd, lo, pre32):
    """fp32 evaluation of an epilogue on the fp32 conv result."""
    h, z, a, o0 = (e[k][..., lo:] for k in ("h", "z", "actv", "o0"))
    if kind == C.EPI_GRU_ZR:
        zz, r = torch.sigmoid(pre32[..., :hd]), torch.sigmoid(pre32[..., hd:])
        return zz.to(BF16), (r * h[..., :hd].float()).to(BF16), r.to(BF16)
    if kind == C.EPI_GRU_Q:
        q = torch.tanh(pre32)
        zz = z[..., :pre32.shape[-1]].float()
        return ((1 - zz) * h[..., :pre32.shape[-1]].float() + zz * q).to(BF16), q.to(BF16)
    raise AssertionError(kind)


@pytest.mark.parametrize("kh,kw", [(3, 3), (1, 1)])
def test_fp32_reference_under_the_epilogue_bounds(kh, kw):
    hd = C.EPI_HD
    chain = min(C.fwd_chain(t, kh * kw, C.KTOT, True) for t in TILES if C.tile_accepts(t, kh, kw, (64, 128), 96))
    for shape in C.EPI_SHAPES:
        e = C.epi_case(*shape, kh, kw)
        pre, pb = e["pre"], C.acc_bound(chain, e["A"])
        pre0, pb0 = e["pre0"], C.acc_bound(chain - 1, e["A0"])
        p32, p032 = _f32_conv(e["x"], e["w"], e["bias"], kh, kw), _f32_conv(e["x"], e["w"], None, kh, kw)
        for kind in (C.EPI_BIAS, C.EPI_RELU, C.EPI_SCALE):
            want, b = C.epi_plain(pre, pb, kind, 0.25)
            got = p32.clamp_min(0) if kind == C.EPI_RELU else p32 * 0.25 if kind == C.EPI_SCALE else p32
            assert C.ratio(got.to(BF16), want, b, BF16) <= 1.0, kind
        outs = C.epi_gru_zr(pre, pb, e["h"][..., :hd], hd)
        for (want, b), got in zip(outs, _epi_f32(e, C.EPI_GRU_ZR, hd, 0, p32)):
            assert C.ratio(got, want, b, BF16) <= 1.0, "zr"
        outs = C.epi_gru_q(pre[..., :hd], pb[..., :hd], e["h"][..., :hd], e["z"][..., :hd])
        for (want, b), got in zip(outs, _epi_f32(e, C.EPI_GRU_Q, hd, 0, p32[..., :hd])):
            assert C.ratio(got, want, b, BF16) <= 1.0, "q"
        want, b = C.epi_relu_bwd(pre0, pb0, e["actv"])
        assert C.ratio((p032 * (e["actv"].float() > 0)).to(BF16), want, b, BF16) <= 1.0
        want, b = C.epi_acc_f32(pre0, pb0, e["o0"])
        assert C.ratio(e["o0"] + p032, want, b, F32) <= 1.0
        n = 96
        (out, bo), (dr, bd) = C.epi_gru_qbwd(pre0[..., :n], pb0[..., :n], e["h"][..., :hd], e["z"][..., :hd],
                                             e["o0"][..., :n], hd)
        v, hh, rr = p032[..., :hd], e["h"][..., :hd].float(), e["z"][..., :hd].float()
        assert C.ratio((v * hh * rr * (1 - rr)).to(BF16), dr, bd, BF16) <= 1.0
        got = torch.cat([e["o0"][..., :hd] + v * rr, e["o0"][..., hd:n] + p032[..., hd:n]], -1)
        assert C.ratio(got, out, bo, F32) <= 1.0
        want, b = C.epi_flow(pre, pb, e["src"])
        assert C.ratio(e["src"] + p32[..., :2].permute(0, 3, 1, 2), want, b, F32) <= 1.0


@pytest.mark.parametrize("kh,kw", C.KERNELS)
def test_fp32_reference_under_the_weight_gradient_bounds(kh, kw):
    worst = 0.0
    for stack in C.WG_STACKS:
        it, B, H, W = stack
        c = C.wgrad_case(*stack, kh, kw)
        x = C.stack_x(c["x0"], c["xb"], c["x2"], it)
        P = it * B * H * W
        got = torch.nn.grad.conv2d_weight(x.float().permute(0, 3, 1, 2), (C.COUT_MAX, C.WG_KTOT, kh, kw),
                                          c["dy"].float().permute(0, 3, 1, 2), 1, (kh // 2, kw // 2))
        gdb = c["dy"].float().sum((0, 1, 2))
        for cout in C.WG_COUTS:
            chains = {C.wgrad_chain(P, kh * kw, C.WG_KTOT, cout, det, var) for det in (0, 1) for var in range(6)}
            bchains = {C.wgrad_bias_chain(P, kh * kw, C.WG_KTOT, cout, det, var) for det in (0, 1) for var in range(6)}
            if (kh, kw) != (1, 1):
                for bm in (64, 128):
                    chains.add(C.wgrad3_chain(it * B, H, W, cout, C.WG_KTOT, bm))
                    bchains.add(C.wgrad3_bias_chain(it * B, H, W, cout, C.WG_KTOT, bm))
            bchains.add(C.colsum_chain(P))
            r = C.ratio(got[:cout], c["dw"][:cout], C.acc_bound(min(chains), c["S"][:cout]), F32)
            rb_ = C.ratio(gdb[:cout], c["db"][:cout], C.acc_bound(min(bchains), c["Sb"][:cout]), F32)
            worst = max(worst, r, rb_)
            assert r <= 1.0 and rb_ <= 1.0, (stack, cout, r, rb_)
    print(f"weight gradient {kh}x{kw}: plain fp32 {worst:.3f} of the bound")


@pytest.mark.parametrize("dtype", [F32, BF16])
def test_fp32_reference_under_the_elementwise_bounds(dtype):
    for shape in C.GATE_BWD_P:
        for hd in C.GATE_BWD_HD:
            dh, z, q, h = C.gate_bwd_case(shape, hd, dtype)
            zf, qf, hf = z.float(), q.float(), h.float()
            gots = (dh * zf * (1 - qf * qf), dh * (qf - hf) * zf * (1 - zf), dh * (1 - zf))
            outs = C.gru_gate_bwd_oracle(dh, z, q, h)
            for i, ((want, b), got) in enumerate(zip(outs, gots)):
                od = F32 if i == 2 else dtype
                assert C.ratio(got.to(od), want, b, od) <= 1.0, (shape, hd, i)
            # exact z = 1 stops dh, exact q~ = +-1 stops dq
            assert bool((outs[2][0][..., 1] == 0).all()) and bool((outs[0][0][..., 0] == 0).all())


# ------------------------------------------------------------------ 4. mutants
def _exceeds(name, mut, want, bound, dtype, must_touch):
    r = C.touched_ratio(mut, want, bound, dtype)
    if r is None:
        assert not must_touch, f"{name}: the mutant changes nothing at a shape that should catch it"
        return False
    assert r[0] > 1.0, f"{name}: the mutant stays inside the bound ({r[0]:.3f})"
    return True


@pytest.mark.parametrize("kh,kw", C.KERNELS)
def test_forward_mutants_exceed_the_bound(kh, kw):
    """(1) a border tap dropped; (2) a tap that wraps over the row end / into the next image.
    The bound is the LARGEST chain any tile under test has (the loosest the GPU file uses)."""
    chain = max(C.fwd_chain(t, kh * kw, C.KTOT, True) for t in TILES)
    caught = {"drop": 0, "row": 0, "image": 0}
    for shape in ALL_FWD_SHAPES:
        B, H, W = shape
        x, w, bias, want, A = C.fwd_case(*shape, kh, kw)
        bound = C.acc_bound(chain, A)
        tap = C.droppable_tap(H, W, kh, kw)
        if tap is not None:
            mut = C.conv_taps(x, w, kh, kw, drop=tap) + bias.double()
            caught["drop"] += _exceeds(f"drop {shape}", mut, want, bound, BF16, True)
        if (kh, kw) != (1, 1):
            # a row to wrap into: a horizontal tap with another row below / above
            mut = C.conv_taps(x, w, kh, kw, wrap="row") + bias.double()
            caught["row"] += _exceeds(f"wrap row {shape}", mut, want, bound, BF16, kw > 1 and H > 1 and W > 1)
            mut = C.conv_taps(x, w, kh, kw, wrap="image") + bias.double()
            caught["image"] += _exceeds(f"wrap image {shape}", mut, want, bound, BF16, B > 1)
    if (kh, kw) != (1, 1):
        assert caught["drop"] >= 7 and caught["image"] >= 4, caught
        assert caught["row"] >= (6 if kw > 1 else 0), caught


@pytest.mark.parametrize("kh,kw", [(3, 3), (1, 1)])
def test_epilogue_mutants_exceed_the_bound(kh, kw):
    """(4) aux read at offset 0 instead of its window (here: the neighbouring 64 channels,
    finite, where the GPU file has NaN); (5) EPI_GRU_QBWD with r for r (1 - r) and with the
    accumulate turned into a store; (6) EPI_ACC_F32 overwriting; (8) the ReLU mask as >= 0."""
    hd = C.EPI_HD
    chain = max(C.fwd_chain(t, kh * kw, C.KTOT, True) for t in TILES)
    for shape in C.EPI_SHAPES:
        e = C.epi_case(*shape, kh, kw)
        pre, pb = e["pre"], C.acc_bound(chain, e["A"])
        pre0, pb0 = e["pre0"], C.acc_bound(chain, e["A0"])
        h, z, wrong_h, wrong_z = e["h"][..., hd:], e["z"][..., hd:], e["h"][..., :hd], e["z"][..., :hd]
        (_, (rh, brh), _) = C.epi_gru_zr(pre, pb, h, hd)
        (_, (mrh, _), _) = C.epi_gru_zr(pre, pb, wrong_h, hd)
        _exceeds("a1off zr", mrh, rh, brh, BF16, True)
        ((hn, bhn), _) = C.epi_gru_q(pre[..., :hd], pb[..., :hd], h, z)
        _exceeds("a1off q", C.epi_gru_q(pre[..., :hd], pb[..., :hd], wrong_h, z)[0][0], hn, bhn, BF16, True)
        _exceeds("a2off q", C.epi_gru_q(pre[..., :hd], pb[..., :hd], h, wrong_z)[0][0], hn, bhn, BF16, True)
        n = 96
        args = (pre0[..., :n], pb0[..., :n], h, z, e["o0"][..., :n], hd)
        (out, bo), (dr, bd) = C.epi_gru_qbwd(*args)
        _exceeds("qbwd r", C.epi_gru_qbwd(*args, r_only=True)[1][0], dr, bd, BF16, True)
        _exceeds("qbwd store", C.epi_gru_qbwd(*args, store=True)[0][0], out, bo, None, True)
        _exceeds("qbwd a2off", C.epi_gru_qbwd(args[0], args[1], h, wrong_z, args[4], hd)[1][0], dr, bd, BF16, True)
        want, b = C.epi_acc_f32(pre0, pb0, e["o0"])
        _exceeds("acc overwrite", C.epi_acc_f32(pre0, pb0, e["o0"], overwrite=True)[0], want, b, None, True)
        want, b = C.epi_relu_bwd(pre0, pb0, e["actv"])
        _exceeds("mask >= 0", C.epi_relu_bwd(pre0, pb0, e["actv"], ge=True)[0], want, b, BF16, True)
        _exceeds("a1off relu_bwd", C.epi_relu_bwd(pre0, pb0, e["actv"].roll(5, -1))[0], want, b, BF16, True)


@pytest.mark.parametrize("kh,kw", C.KERNELS)
def test_weight_gradient_mutants_exceed_the_bound(kh, kw):
    """(3) the broadcast segment read at the stack index; (7) the last pixel of the stack
    dropped from dW and db.  The loosest chain of any kernel under test."""
    for stack in C.WG_STACKS:
        it, B, H, W = stack
        P = it * B * H * W
        c = C.wgrad_case(*stack, kh, kw)
        chain = max([C.wgrad_chain(P, kh * kw, C.WG_KTOT, co, d, v) for co in C.WG_COUTS for d in (0, 1) for v in range(6)]
                    + [C.wgrad3_chain(it * B, H, W, co, C.WG_KTOT, bm) for co in C.WG_COUTS for bm in (64, 128)])
        bchain = max([C.wgrad_bias_chain(P, kh * kw, C.WG_KTOT, co, d, v) for co in C.WG_COUTS for d in (0, 1)
                      for v in range(6)] + [C.wgrad3_bias_chain(it * B, H, W, 200, C.WG_KTOT, 64), C.colsum_chain(P)])
        bound = C.acc_bound(chain, c["S"])
        mdw, mdb = C.mutant_drop_last_pixel(c, it, kh, kw)
        _exceeds(f"last pixel dw {stack}", mdw, c["dw"], bound, None, True)
        _exceeds(f"last pixel db {stack}", mdb, c["db"], C.acc_bound(bchain, c["Sb"]), None, True)
        mdw = C.wgrad_oracle(C.stack_x(c["x0"], c["xb"], c["x2"], it, mutant=True), c["dy"], kh, kw)[0]
        _exceeds(f"broadcast index {stack}", mdw, c["dw"], bound, None, it > 1)

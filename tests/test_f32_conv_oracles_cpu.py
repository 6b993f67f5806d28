"""The oracles, bounds, launch mirrors and mutants of tests/f32_conv_cases.py (no GPU).

1. the split is what the derivation of the value bound assumes (|lo| <= 2^-8 |v|, remainder
   <= 2^-16 |v|, XLO splits to (1, 2^-8)), the product oracle is the fp64 conv of hi + lo
   less the lo.lo term, the input- and weight-gradient oracles equal float64 autograd, and
   product and value oracle never differ by more than SPLIT A (while they do differ by more
   than the 3 * 2^-18 allotment of enc_conv_cases.split_bound);
2. the launch mirrors and chain constants agree with the kernel files, ops/conv.py and the
   host checks; every split rounds to nearest even;
3. a plain fp32 evaluation of the three products stays inside BOTH bounds at every case of
   tests/test_f32_conv_edges_gpu.py;
4. every mutant (a dropped lo product, lo.lo for hi.lo, lo from the wrong 32-channel chunk,
   a wrapped tap, a dropped border tap, a split-K group repeating its last step; for the
   weight gradients a dropped product and db counted three times) exceeds the PRODUCT bound on
   an element it touches, at the loosest chain any tile under test has.
"""
import os
import re

import pytest
import torch
import torch.nn.functional as F

import enc_conv_cases as E
import f32_conv_cases as C
import update_conv_cases as UC
from f32_conv_cases import F32, F64

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TILES = C.tiles_under_test()
ALL_FWD_SHAPES = sorted(set(C.PATCH_SHAPES + C.FLAT_SHAPES + [(1, 1, 1), (2, 9, 1)]))


def _src(name):
    with open(os.path.join(ROOT, "raft_stir_amd", "csrc", name)) as f:
        return f.read()


def _fwd_variants():
    """(shape, kh, kw, ktot, chans) of every forward case of the GPU file."""
    out = []
    for shape in ALL_FWD_SHAPES:
        for kh, kw in C.KERNELS:
            out.append((shape, kh, kw, 192, (64, 128)))
            out.append((shape, kh, kw, 192, (32, 64, 96)))
            if (kh, kw) != (1, 1) and shape in C.PATCH_SHAPES:
                out.append((shape, kh, kw, 64, (64,)))
    for layout, shape in C.SPLITK_EXTRA:
        out.append((shape, 1, 1, C.layout_ktot(layout), tuple(c for _, _, c in C.LAYOUTS[layout])))
    return sorted(set(out))


def _chains(kh, kw, chans, cout=96):
    return sorted({C.fwd_chain(t, kh * kw, sum(chans), True) for t in TILES if C.tile_accepts(t, kh, kw, chans, cout)})


# ------------------------------------------------------------------ 1. the split and the oracles
def test_split_is_what_the_value_bound_assumes():
    g = C.gen(1)
    x = torch.cat([torch.randn(20000, generator=g) * 2.0 ** torch.randint(-30, 30, (20000,), generator=g).float(),
                   C.split_values(64), torch.tensor([C.XLO, -C.XLO, 1.0 + 2.0 ** -7 - 2.0 ** -23])])
    hi, lo = C.split_bf16(x)
    xd = x.double()
    big = xd.abs() > 2.0 ** -100  # (near the subnormals of bf16 the half ulp is absolute, not relative)
    assert int(big.sum()) > 20000
    assert bool(((xd - hi.double()).abs()[big] <= 2.0 ** -8 * xd.abs()[big]).all())
    assert bool((lo.double().abs()[big] <= 2.0 ** -8 * xd.abs()[big]).all())
    assert bool(((xd - hi.double() - lo.double()).abs()[big] <= 2.0 ** -16 * xd.abs()[big]).all())
    assert bool(((x - hi).double() == xd - hi.double()).all())  # x - hi is exact in fp32
    hi, lo = C.split_bf16(torch.tensor([C.XLO]))
    assert hi.item() == 1.0 and lo.item() == 2.0 ** -8
    # the worst cases are real: a value just below a tie has |x - hi| ~ 2^-8 |x|
    assert (C.XLO - 1.0) / C.XLO > 0.99 * 2.0 ** -8
    assert C.SPLIT == 3 * 2.0 ** -16 + 3 * 2.0 ** -32


@pytest.mark.parametrize("kh,kw", C.KERNELS)
def test_product_oracle_is_the_conv_of_the_split_values(kh, kw):
    for shape in [(1, 1, 1), (2, 9, 1), (3, 5, 13), (1, 9, 33)]:
        c = C.fwd_case(*shape, kh, kw)
        x, w, bias = c["x"], c["w"], c["bias"]
        (xh, xl), (wh, wl) = C.split_bf16(x), C.split_bf16(w)
        full, _ = UC.conv_fwd(xh.double() + xl.double(), wh.double() + wl.double(), bias, kh, kw)
        ll, _ = C.product3(x, w, None, kh, kw, terms=("ll",))
        assert C.ratio(c["want3"], full - ll, 64 * 2.0 ** -53 * c["A3"]) <= 1.0
        assert C.ratio(C.taps3(x, w, kh, kw) + bias.double(), c["want3"], 64 * 2.0 ** -53 * c["A3"]) <= 1.0
        p = C.plant_pixel(*shape)  # the planted output cancels to 2^-20 of its magnitude
        assert 0.5 * C.E20 < (c["want3"][p][0] / c["A3"][p][0]).item() < 2.0 * C.E20
        # the plants: the lo pixel, the positive row, the lo row
        assert bool((x[C.LO_PIXEL] == C.XLO).all()) and bool((w[C.ROW_POS] > 0).all())
        assert bool((wl[C.ROW_LO] == 2.0 ** -13).all()) and bool((xl[C.LO_PIXEL] == 2.0 ** -8).all())


def test_product_and_value_oracle_differ_by_the_split_bound_at_most():
    worst = 0.0
    for shape, kh, kw, ktot, _ in _fwd_variants():
        c = C.fwd_case(*shape, kh, kw, ktot)
        r = C.ratio(c["want3"], c["want"], C.SPLIT * c["A"])
        worst = max(worst, r)
        assert r <= 1.0, (shape, kh, kw, ktot, r)
    print(f"|product - value| <= {worst:.3f} SPLIT A")
    # ... and the 3 * 2^-18 allotment of enc_conv_cases.split_bound would not hold here
    assert worst * C.SPLIT > 3 * 2.0 ** -18


def test_gradient_oracles_equal_autograd():
    B, H, W, cin, cout = 2, 5, 6, 64, 96
    for k, s, p in C.GEO_KSP + [(3, 1, 1)]:
        c = C.dgrad_case(B, H, W, cin, cout, k, s, p)
        (dyh, dyl), (wh, wl) = C.split_bf16(c["dy"]), C.split_bf16(c["w"])
        x = torch.zeros(B, cin, H, W, dtype=F64, requires_grad=True)
        F.conv2d(x, wh.double() + wl.double(), None, s, p).backward(C.nchw(dyh.double() + dyl.double()))
        dx4, _ = C.dgrad3(c["dy"], c["w"], (H, W), s, p, terms=("hh", "lh", "hl", "ll"))
        torch.testing.assert_close(dx4, C.nhwc(x.grad))
        x = torch.zeros(B, cin, H, W, dtype=F64, requires_grad=True)
        F.conv2d(x, c["w"].double(), None, s, p).backward(C.nchw(c["dy"]))
        torch.testing.assert_close(c["dx"], C.nhwc(x.grad))
        # the phase-split assembly is the same gradient
        ph, _ = E.phase_dgrad(c["dy"], c["w"], (H, W), s, p)
        torch.testing.assert_close(ph, c["dx"])
    for kh, kw in C.KERNELS:
        c = C.wgrad_case(3, 1, 5, 13, kh, kw)
        (xh, xl), (gh, gl) = C.split_bf16(c["x"]), C.split_bf16(c["dy"])
        w = torch.zeros(C.COUT_MAX, C.WG_KTOT, kh, kw, dtype=F64, requires_grad=True)
        b = torch.zeros(C.COUT_MAX, dtype=F64, requires_grad=True)
        y = F.conv2d(C.nchw(xh.double() + xl.double()), w, b, 1, (kh // 2, kw // 2))
        y.backward(C.nchw(gh.double() + gl.double()))
        dw4, _, db, _ = C.wgrad3(c["x"], c["dy"], kh, kw, terms=("hh", "lh", "hl", "ll"))
        torch.testing.assert_close(dw4, w.grad)
        torch.testing.assert_close(db, b.grad)
        torch.testing.assert_close(c["db3"], b.grad)
        w = torch.zeros(C.COUT_MAX, C.WG_KTOT, kh, kw, dtype=F64, requires_grad=True)
        F.conv2d(C.nchw(c["x"]), w, None, 1, (kh // 2, kw // 2)).backward(C.nchw(c["dy"]))
        torch.testing.assert_close(c["dw"], w.grad)
        assert C.ratio(c["dw3"], c["dw"], C.SPLIT * c["S"]) <= 1.0
        assert C.ratio(c["db3"], c["db"], 2.0 ** -16 * c["Sb"]) <= 1.0  # db: only dy's remainder is lost


def test_epilogue_case_plants():
    e = C.epi_case(2, 5, 7, 3, 3)
    for base in (0, C.EPI_HD):
        for i, v in enumerate(C.PLANT):
            assert bool((e["pre"][..., base + i] == torch.tensor(v, dtype=F32).double()).all())
            assert bool((e["A3"][..., base + i] == abs(torch.tensor(v, dtype=F32).double())).all())
    assert bool((e["z"][..., 3] == 0).all()) and bool((e["z"][..., 4] == 1).all())
    a = e["actv"][0, 0, 0, :5]
    assert a[0] == 0 and a[1] == 0 and torch.signbit(a[1]) and not torch.signbit(a[0]) and a[2] > 0 > a[3]
    assert bool((e["nscale"] < 0).any()) and bool((e["nscale"] > 0).any())
    text = open(os.path.join(ROOT, "tests", "test_gates_gpu.py")).read()
    m = re.search(r"^PLANT = (\[.*\])$", text, re.M)
    assert m and eval(m.group(1)) == C.PLANT


# ------------------------------------------------------------------ 2. launch mirrors
def test_tile_list_comes_from_the_table_and_the_heuristic():
    from raft_stir_amd.ops import conv as oc
    tuned = set(C.tuned_table_f32().values())
    assert tuned and tuned <= set(TILES)
    assert C.choose_tile_f32_range() == {6, 7, 8, 38, 40, 81, 82, 83, 84, 85}  # (39: by the tuned table only)
    assert set(TILES) == set(C.REG_TILES) | set(C.V3F_TILES)
    assert set(oc.F32_TILES) <= set(C.REG_TILES) and set(oc.V3F_TILES) == set(C.V3F_TILES)
    assert (C.EPI_BIAS, C.EPI_GRU_QBWD, C.EPI_FLOW) == (oc.EPI_BIAS, oc.EPI_GRU_QBWD, oc.EPI_FLOW)
    assert C.EPI_NORM == oc.EPI_NORM
    with pytest.raises(ValueError, match="no fp32 conv_fused tile 41"):
        C.tile_geom(41)


def test_launch_mirrors_reproduce_the_kernel_files():
    conv, v3f, ops = _src("conv.hip"), _src("conv_v3f.hip"), _src("ops_conv.cpp")
    # conv_launch: RS_F32(BM, BN, KG) per tile, tile 7 as the fall-through
    assert "conv_lds_kernel<BM_, BN_, 2, 2, 64, false, true, KG_>" in conv
    seen = {int(t): (int(a), int(b), int(k)) for t, a, b, k in
            re.findall(r"if \(L\.tile == (\d+)\) RS_F32\((\d+), (\d+), (\d)\);", conv)}
    m = re.search(r"else RS_F32\((\d+), (\d+), (\d)\);", conv)
    seen[7] = tuple(int(v) for v in m.groups())
    assert seen == C.REG_TILES
    # the F32 K step: 32 input channels, three MFMAs (wh, xh), (wh, xl), (wl, xh) into one accumulator
    assert "constexpr int KSTEP = F32 ? 32 : BK;" in conv and "constexpr int NPASS = F32 ? 3 : BK / 32;" in conv
    assert "const int ka = F32 ? (ps == 2 ? 1 : 0) : ps, kb = F32 ? (ps == 1 ? 1 : 0) : ps;" in conv
    assert "const int nst = (nsteps + KG - 1) / KG;" in conv and "for (int g = 0; g < KG - 1; ++g)" in conv
    assert "__builtin_amdgcn_mfma_f32_16x16x32_bf16" in conv
    # v3f_launch: <KH, KW, NWM, THW, RA, NWP, SB>
    seen = {}
    pat = r"case (\d+): hipLaunchKernelGGL\(\(conv_v3f_kernel<KH, KW, (\d), (\d), RA((?:, \d)*)>\)"
    for t, nwm, thw, rest in re.findall(pat, v3f):
        extra = [int(v) for v in re.findall(r"\d", rest)] + [1, 0][len(re.findall(r"\d", rest)):]
        seen[int(t)] = (int(nwm), int(thw), extra[0], extra[1])
    assert seen == C.V3F_TILES
    assert "static constexpr int T = KH * KW, NSL = 4 * T" in v3f
    assert v3f.count("V3F_GROUP(Ah[") + v3f.count("V3F_GROUP(Al[") == 3
    assert "V3F_GROUP(Ah[sc_], V3F_BH, fb_);" in v3f and "V3F_GROUP(Al[sc_], V3F_BH, fb_);" in v3f
    assert "V3F_GROUP(Ah[sc_], V3F_BL, fb_);" in v3f and "__builtin_amdgcn_mfma_f32_32x32x16_bf16" in v3f
    assert "static constexpr int TH = THW * NWP, TW = 32, BM = 32 * NWM;" in v3f
    # chains: 3x3 over 192 channels
    assert C.fwd_chain(7, 9, 192, True) == 2 * 3 * 54 + 1 == C.fwd_chain(6, 9, 192, True)
    assert C.fwd_chain(38, 9, 192, True) == 2 * 3 * 14 + 3 + 1 and C.fwd_chain(40, 9, 192, False) == 2 * 3 * 27 + 1
    assert C.fwd_chain(39, 1, 96, False) == 2 * 3 * 2 + 1 and C.fwd_chain(38, 1, 32, True) == 2 * 3 * 1 + 3 + 1
    assert C.fwd_chain(81, 9, 192, True) == 2 * 3 * 108 + 1 == C.fwd_chain(84, 9, 192, True)
    assert C.fwd_chain(85, 5, 64, False) == 2 * 3 * 20
    assert C.geo_chain(9, 64, True) == 2 * 3 * 18 + 1 and C.geo_dgrad_chain(3, 96) == 2 * 3 * 12
    # the split-K step walk and its uneven ends
    assert C.step_slices(2, (32, 64)) == [(0, 0), (1, 0), (0, 32), (0, 64), (1, 32), (1, 64)]
    assert C.stale_steps(3, 2) == [1] and C.stale_steps(3, 4) == [] and C.stale_steps(54, 4) == [50, 51]
    assert C.stale_steps(54, 2) == [] and C.stale_steps(6, 4) == [2, 3] and C.stale_steps(1, 4) == []
    # host checks
    assert "tile == 6 || tile == 7 || tile == 8 || (tile >= 38 && tile <= 40) || v3f" in ops
    assert 'TORCH_CHECK(epi != EPI_FLOW, "conv_fused: fp32 activations: no flow epilogue' in ops
    assert "tile != 85 || Ktot == 64" in ops and "tiles 81-85 need segment channels % 64 == 0" in ops
    assert C.tile_accepts(7, 1, 1, (32, 64, 96), 96) and not C.tile_accepts(81, 1, 1, (64, 128), 96)
    assert not C.tile_accepts(81, 3, 3, (32, 64, 96), 96) and not C.tile_accepts(85, 3, 3, (64, 128), 96)
    assert C.tile_accepts(85, 5, 1, (64,), 64)
    # weight-gradient routes (models/fused_train.py _wgrad_fn)
    ft = open(os.path.join(ROOT, "raft_stir_amd", "models", "fused_train.py")).read()
    assert "pc.kh * pc.kw in (5, 9) and pc.cout > 64" in ft and "bm = 128 if pc.cout >= 512 else 64" in ft
    assert C.wgrad_route(3, 3, 200) == ("v3", 64)
    assert C.wgrad_route(3, 3, 64) == ("wgrad", 0) == C.wgrad_route(1, 1, 200)
    assert {C.wgrad_route(kh, kw, co)[0] for kh, kw, co in C.WG_KC} == {"v3", "wgrad"}
    assert "wg(dyh, yoff, pc.cout, [x[1] for x in xs], offs, chans, per, pc.kh, pc.kw, pc.dw, None)" in ft
    ec = open(os.path.join(ROOT, "raft_stir_amd", "ops", "enc_conv.py")).read()
    assert "dw = f(dyh, xh) + f(dyl, xh) + f(dyh, xl)" in ec and "db = dyn.sum((0, 1, 2))" in ec


def test_every_split_rounds_to_nearest_even():
    """split8 (conv_common.h), V3F_CONVERT (conv_v3f.hip) and split4 (split.hip) convert with
    __builtin_convertvector to __bf16 (v_cvt_pk_bf16_f32: RNE) and subtract the widened hi in
    fp32; split.hip's tail and common.h f2bf cast to __bf16 (RNE); ops/conv.py split_weight
    uses torch's .to(bfloat16) (RNE): all are split_bf16 of enc_conv_cases.py."""
    cc, v3f, sp, cm = _src("conv_common.h"), _src("conv_v3f.hip"), _src("split.hip"), _src("common.h")
    assert "__builtin_convertvector(v, bf16x2v_t)" in cc and "__builtin_convertvector(v - hf, bf16x2v_t)" in cc
    assert "__builtin_convertvector(p0_, bf16x2_t)" in v3f and "__builtin_convertvector(r0_, bf16x2_t)" in v3f
    assert "const f32x2_t r0_ = p0_ - f32x2_t{" in v3f
    assert "__builtin_convertvector(p0, b2_t)" in sp and "lo[i] = f2bf(x[i] - bf2f(h0));" in sp
    assert "static_cast<__bf16>(f)" in cm
    py = open(os.path.join(ROOT, "raft_stir_amd", "ops", "conv.py")).read()
    assert "hi = w.to(torch.bfloat16)" in py and "lo = (w - hi.float()).to(torch.bfloat16)" in py
    from raft_stir_amd.ops.conv import split_weight
    w = C.split_values(64).view(1, 1, 64)
    hi, lo = C.split_oracle(w)
    got = split_weight(w).view(1, 1, 2, 2, 32)
    assert torch.equal(got[:, :, :, 0].reshape(1, 1, 64), hi) and torch.equal(got[:, :, :, 1].reshape(1, 1, 64), lo)
    t = torch.tensor([1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8])  # ties go to the even neighbour
    assert C.split_oracle(t)[0].tolist() == [1.0, 1.0 + 2.0 ** -6]


# ------------------------------------------------------------------ 3. plain fp32 under both bounds
def _f32_three(x, w, b, kh, kw, stride=1, pad=None):
    """The three products and their sum in plain fp32."""
    (xh, xl), (wh, wl) = C.split_bf16(x), C.split_bf16(w)
    pad = (kh // 2, kw // 2) if pad is None else pad
    n = lambda t: t.permute(0, 3, 1, 2)
    y = F.conv2d(n(xh), wh, None, stride, pad) + F.conv2d(n(xl), wh, None, stride, pad)
    y = y + F.conv2d(n(xh), wl, None, stride, pad)
    if b is not None:
        y = y + b.view(1, -1, 1, 1)
    assert y.dtype == F32
    return y.permute(0, 2, 3, 1)


def test_fp32_reference_under_the_forward_bounds():
    worst = [0.0, 0.0]
    for shape, kh, kw, ktot, chans in _fwd_variants():
        c = C.fwd_case(*shape, kh, kw, ktot)
        got = _f32_three(c["x"], c["w"], c["bias"], kh, kw)
        chains = _chains(kh, kw, chans)
        assert chains, (kh, kw, chans)
        for ch in chains:
            r3 = C.ratio(got, c["want3"], C.product_bound(ch, c["A3"]), F32)
            rv = C.ratio(got, c["want"], C.value_bound(ch, c["A3"], c["A"]), F32)
            worst = [max(worst[0], r3), max(worst[1], rv)]
            assert r3 <= 1.0 and rv <= 1.0, (shape, kh, kw, ktot, ch, r3, rv)
    print(f"forward: plain fp32 at {worst[0]:.3f} of the product bound, {worst[1]:.3f} of the value bound")


def test_fp32_reference_under_the_epilogue_bounds():
    hd, kh, kw = C.EPI_HD, 3, 3
    chain = min(C.fwd_chain(t, 9, UC.KTOT, True) for t in C.EPI_TILES)
    worst = {}
    for shape in C.EPI_SHAPES:
        e = C.epi_case(*shape, kh, kw)
        pre, pb = e["pre"], C.product_bound(chain, e["A3"])
        pre0, pb0 = e["pre0"], C.product_bound(chain - 1, e["A30"])
        p32, p032 = _f32_three(e["x"], e["w"], e["bias"], kh, kw), _f32_three(e["x"], e["w"], None, kh, kw)
        h, z = e["h"][..., :hd], e["z"][..., :hd]

        def chk(name, got, wb):
            r = C.ratio(got, wb[0], wb[1], F32)
            worst[name] = max(worst.get(name, 0.0), r)
            assert r <= 1.0, (name, shape, r)

        for kind in (C.EPI_BIAS, C.EPI_RELU, C.EPI_SCALE):
            got = p32.clamp_min(0) if kind == C.EPI_RELU else p32 * 0.25 if kind == C.EPI_SCALE else p32
            chk("plain", got, UC.epi_plain(pre, pb, kind, 0.25))
        zz, r = torch.sigmoid(p32[..., :hd]), torch.sigmoid(p32[..., hd:])
        for got, wb in zip((zz, r * h, r), UC.epi_gru_zr(pre, pb, h, hd)):
            chk("gru_zr", got, wb)
        q = torch.tanh(p32[..., :hd])
        for got, wb in zip(((1 - z) * h + z * q, q), UC.epi_gru_q(pre[..., :hd], pb[..., :hd], h, z)):
            chk("gru_q", got, wb)
        chk("relu_bwd", p032 * (e["actv"] > 0), UC.epi_relu_bwd(pre0, pb0, e["actv"]))
        chk("acc", e["o0"] + p032, UC.epi_acc_f32(pre0, pb0, e["o0"]))
        n = 96
        out, dr = UC.epi_gru_qbwd(pre0[..., :n], pb0[..., :n], h, z, e["o0"][..., :n], hd)
        v = p032[..., :hd]
        chk("qbwd dr", v * h * z * (1 - z), dr)
        chk("qbwd out", torch.cat([e["o0"][..., :hd] + v * z, e["o0"][..., hd:n] + p032[..., hd:n]], -1), out)
        for relu, use_res in C.NORM_KINDS:
            got = p032 * e["nscale"] + e["nshift"]
            got = got.clamp_min(0) if relu else got
            got = (got + e["res"]).clamp_min(0) if use_res else got
            chk("norm", got, C.epi_norm(pre0, pb0, e["nscale"], e["nshift"], relu, e["res"] if use_res else None))
    print("epilogues, plain fp32: " + "  ".join(f"{k} {v:.3f}" for k, v in sorted(worst.items())))


def test_fp32_reference_under_the_geo_and_dgrad_bounds():
    worst = [0.0, 0.0]
    for k, s, p in C.GEO_KSP:
        for H, W in C.GEO_HW:
            for cin, cout in C.GEO_CH:
                c = C.geo_case(C.GEO_B, H, W, cin, cout, k, s, p)
                got = _f32_three(c["x"], c["w"], c["bias"], k, k, s, p)
                ch = C.geo_chain(k * k, cin, True)
                r3 = C.ratio(got, c["want3"], C.product_bound(ch, c["A3"]), F32)
                rv = C.ratio(got, c["want"], C.value_bound(ch, c["A3"], c["A"]), F32)
                assert r3 <= 1.0 and rv <= 1.0, (k, s, H, W, cin, cout, r3, rv)
                d = C.dgrad_case(C.GEO_B, H, W, cin, cout, k, s, p)
                worst = [max(worst[0], r3, _dgrad_f32(d, (H, W), s, p, C.geo_dgrad_chain(k, cout))), max(worst[1], rv)]
    for shape in C.DGRAD_S1_SHAPES:
        for cin, cout in C.DGRAD_S1_CH:
            d = C.dgrad_case(*shape, cin, cout, 3, 1, 1)
            chain = min(C.fwd_chain(t, 9, cout, False) for t in TILES if C.tile_accepts(t, 3, 3, (cout,), cin))
            worst[0] = max(worst[0], _dgrad_f32(d, shape[1:], 1, 1, chain))
    print(f"conv_geo / dgrads: plain fp32 at {worst[0]:.3f} of the product bound, {worst[1]:.3f} of the value bound")


def _dgrad_f32(d, in_hw, s, p, chain):
    (gh, gl), (wh, wl) = C.split_bf16(d["dy"]), C.split_bf16(d["w"])
    size = (d["dy"].shape[0], d["w"].shape[1], *in_hw)
    n = lambda t: t.permute(0, 3, 1, 2)
    ci = torch.nn.grad.conv2d_input
    got = ci(size, wh, n(gh), s, p) + ci(size, wh, n(gl), s, p) + ci(size, wl, n(gh), s, p)
    got = got.permute(0, 2, 3, 1)
    r3 = C.ratio(got, d["dx3"], C.product_bound(chain, d["T3"]), F32)
    rv = C.ratio(got, d["dx"], C.value_bound(chain, d["T3"], d["T"]), F32)
    assert r3 <= 1.0 and rv <= 1.0, (in_hw, s, chain, r3, rv)
    return r3


def _wgrad_f32(x, dy, size, s, p):
    (xh, xl), (gh, gl) = C.split_bf16(x), C.split_bf16(dy)
    n = lambda t: t.permute(0, 3, 1, 2)
    cw = torch.nn.grad.conv2d_weight
    return cw(n(xh), size, n(gh), s, p) + cw(n(xh), size, n(gl), s, p) + cw(n(xl), size, n(gh), s, p), gh, gl


def test_fp32_reference_under_the_weight_gradient_bounds():
    worst = 0.0
    for stack in C.WG_STACKS:
        for kh, kw, cout in C.WG_KC:
            c = C.wgrad_case(*stack, kh, kw)
            got, gh, gl = _wgrad_f32(c["x"], c["dy"], (C.COUT_MAX, C.WG_KTOT, kh, kw), 1, (kh // 2, kw // 2))
            gdb = gh.sum((0, 1, 2)) + gl.sum((0, 1, 2))
            route, bm = C.wgrad_route(kh, kw, cout)
            cd, cb = (min(v) for v in zip(*(C.wgrad_chains(route, bm, stack, kh, kw, cout, d) for d in (False, True))))
            r3 = C.ratio(got[:cout], c["dw3"][:cout], C.acc_bound(cd, c["S3"][:cout]), F32)
            rv = C.ratio(got[:cout], c["dw"][:cout], C.acc_bound(cd, c["S3"][:cout]) + C.SPLIT * c["S"][:cout], F32)
            rb = C.ratio(gdb[:cout], c["db3"][:cout], C.acc_bound(cb, c["Sb3"][:cout]), F32)
            worst = max(worst, r3, rv, rb)
            assert r3 <= 1.0 and rv <= 1.0 and rb <= 1.0, (stack, kh, kw, cout, r3, rv, rb)
    for k, s, p in C.ENC_WG_KSP:
        for shape in C.ENC_WG_SHAPES[s]:
            for cin, cout in C.ENC_WG_CH:
                c = C.enc_wgrad_case(*shape, cin, cout, k, s, p)
                got, _, _ = _wgrad_f32(c["x"], c["dy"], (cout, cin, k, k), s, p)
                ch = C.enc_wgrad_chain(*shape, cin, cout, k, s, p)
                r3 = C.ratio(got, c["dw3"], C.acc_bound(ch, c["S3"]), F32)
                rv = C.ratio(got, c["dw"], C.acc_bound(ch, c["S3"]) + C.SPLIT * c["S"], F32)
                worst = max(worst, r3, rv)
                assert r3 <= 1.0 and rv <= 1.0, (k, s, shape, cin, cout, r3, rv)
    print(f"weight gradients: plain fp32 at {worst:.3f} of the bounds")


# ------------------------------------------------------------------ 4. mutants
def _exceeds(name, mut, want, bound, must_touch, log):
    r = C.touched_ratio(mut, want, bound, F32)
    if r is None:
        assert not must_touch, f"{name}: the mutant changes nothing at a shape that should catch it"
        return False
    log.append(f"{name}: {r[0]:.1f}")
    assert r[0] > 1.0, f"{name}: the mutant stays inside the product bound ({r[0]:.3f})"
    return True


def test_forward_mutants_exceed_the_product_bound():
    log = []
    caught = {k: 0 for k in ("drop lh", "drop hl", "ll for hl", "lo chunk", "drop tap", "row", "image", "stale")}
    for shape, kh, kw, ktot, chans in _fwd_variants():
        B, H, W = shape
        c = C.fwd_case(*shape, kh, kw, ktot)
        x, w, bias, want = c["x"], c["w"], c["bias"], c["want3"]
        chain = max(C.fwd_chain(t, kh * kw, ktot, True) for t in TILES if C.tile_accepts(t, kh, kw, chans, 96))
        bound = C.product_bound(chain, c["A3"])
        tag = f"{shape} {kh}x{kw} K{ktot}"
        for name, kw_ in (("drop lh", dict(terms=("hh", "hl"))), ("drop hl", dict(terms=("hh", "lh"))),
                          ("ll for hl", dict(terms=("hh", "lh", "ll")))):
            mut = C.product3(x, w, bias, kh, kw, **kw_)[0]
            caught[name] += _exceeds(f"{name} {tag}", mut, want, bound, True, log)
            # ... and on the planted elements alone (the lo pixel under the positive row, the lo row)
            # where no x 64 neighbour shares the output: there the loss is 2^-8 of the magnitude
            if (kh, kw) == (1, 1):
                el = (*C.LO_PIXEL, C.ROW_POS) if name == "drop lh" else (*C.LO_PIXEL, C.ROW_LO)
                assert abs(mut[el] - want[el]) > 0.9 * 2.0 ** -8 * (c["A3"][el] - abs(bias[el[-1]])), (name, tag)
                assert abs(mut[el] - want[el]) > 100 * bound[el], (name, tag)
        if ktot > 32:
            mut = C.product3(x, w, bias, kh, kw, xl_roll=1)[0]
            # (a one-pixel image holds XLO in every channel)
            caught["lo chunk"] += _exceeds(f"lo chunk {tag}", mut, want, bound, B * H * W > 1, log)
        tap = C.droppable_tap(H, W, kh, kw)
        if tap is not None:
            mut = C.taps3(x, w, kh, kw, drop=tap) + bias.double()
            caught["drop tap"] += _exceeds(f"drop tap {tag}", mut, want, bound, True, log)
        if (kh, kw) != (1, 1):
            mut = C.taps3(x, w, kh, kw, wrap="row") + bias.double()
            caught["row"] += _exceeds(f"wrap row {tag}", mut, want, bound, kw > 1 and H > 1 and W > 1, log)
            mut = C.taps3(x, w, kh, kw, wrap="image") + bias.double()
            caught["image"] += _exceeds(f"wrap image {tag}", mut, want, bound, B > 1, log)
        for kg in (2, 4):
            extra = C.mutant_stale_step(x, w, kh, kw, chans, kg)
            if extra is not None:
                # (a repeated border tap of a one-pixel or one-column image reads nothing)
                caught["stale"] += _exceeds(f"stale step KG {kg} {tag} {chans}", want + extra, want, bound,
                                            (kh, kw) == (1, 1), log)
    print("\n".join(log))
    print(caught)
    assert all(v >= 6 for v in caught.values()), caught
    # the uneven split-K ends of the GPU file's extra cases: 3 steps over 2 groups
    assert C.mutant_stale_step(*[C.fwd_case(1, 3, 43, 1, 1, 96)[k] for k in "xw"], 1, 1, (32, 64), 2) is not None


def test_weight_gradient_mutants_exceed_the_product_bound():
    log = []
    for stack in C.WG_STACKS:
        for kh, kw, cout in C.WG_KC:
            c = C.wgrad_case(*stack, kh, kw)
            route, bm = C.wgrad_route(kh, kw, cout)
            cd, cb = (max(v) for v in zip(*(C.wgrad_chains(route, bm, stack, kh, kw, cout, d) for d in (False, True))))
            bound, bbound = C.acc_bound(cd, c["S3"][:cout]), C.acc_bound(cb, c["Sb3"][:cout])
            tag = f"{stack} {kh}x{kw} cout {cout}"
            for name, terms in (("drop dYl.Xh", ("hh", "hl")), ("drop dYh.Xl", ("hh", "lh"))):
                mut = C.wgrad3(c["x"], c["dy"], kh, kw, terms=terms)[0]
                _exceeds(f"{name} {tag}", mut[:cout], c["dw3"][:cout], bound, True, log)
            mdb = C.wgrad3(c["x"], c["dy"], kh, kw, terms=(), db_terms=("h", "l", "h"))[2]
            _exceeds(f"db three times {tag}", mdb[:cout], c["db3"][:cout], bbound, True, log)
    for k, s, p in C.ENC_WG_KSP:
        for shape in C.ENC_WG_SHAPES[s]:
            cin, cout = C.ENC_WG_CH[0]
            c = C.enc_wgrad_case(*shape, cin, cout, k, s, p)
            bound = C.acc_bound(C.enc_wgrad_chain(*shape, cin, cout, k, s, p), c["S3"])
            (xh, xl), (gh, gl) = C.split_bf16(c["x"]), C.split_bf16(c["dy"])
            cw = torch.nn.grad.conv2d_weight
            for name, (a, b) in (("drop dYl.Xh", (gl, xh)), ("drop dYh.Xl", (gh, xl))):
                mut = c["dw3"] - cw(C.nchw(b), (cout, cin, k, k), C.nchw(a), s, p)
                _exceeds(f"enc {name} {k} s{s} {shape}", mut, c["dw3"], bound, True, log)
    print("\n".join(log))

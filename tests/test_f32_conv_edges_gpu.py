"""The fp32 (split-bf16) convolution family, each kernel on its own, per element vs fp64 oracles.

conv_fused on fp32 segments: the F32 instantiation of conv_lds_kernel (csrc/conv.hip; tiles
6 / 7 / 8 and the intra-block split-K tiles 38 / 39 / 40), the weight-streaming tiles 81-85 of
csrc/conv_v3f.hip, every fp32 epilogue of conv_common.h (epilogue_pix_f32 / epi_frag_f32 /
epi32_f32); conv_geo in fp32 and the two fp32 input gradients (the phase-split
_conv_geo_dgrad and the stride-1 3x3 dgrad of _ConvF32.backward); split_bf16 (csrc/split.hip)
bit for bit; the three-call weight gradients dYh.Xh + dYl.Xh + dYh.Xl of
models/fused_train.py _conv_wgrad and ops/enc_conv.py _f32_wgrad.  The tile list is read at
collection time (f32_conv_cases.tiles_under_test: F32_TILES, 38-40, V3F_TILES, the tuned
tiles_f32 table and choose_tile_f32's range); an id without a geometry mirror fails collection.

Oracles and bounds (tests/f32_conv_cases.py; tests/test_f32_conv_oracles_cpu.py ties them to
autograd and to the sources, shows that a plain fp32 evaluation of the three products stays
inside every bound and that every mutant leaves the product bound).  U = 2^-24, an MFMA step
counts 2 U.  Every check prints max|err| and err / bound and asserts dtype, finiteness and
ratio <= 1 for EVERY element.
  product oracle  conv(xh, wh) + conv(xl, wh) + conv(xh, wl) in fp64 on the split values
                  (hi = rne_bf16(v), lo = rne_bf16(v - hi)); bound c U A3, A3 the three products'
                  absolute sum (+ |bias|).
  value oracle    fp64 F.conv2d of the fp32 values; bound c U A3 + SPLIT A with
                  SPLIT = 3 2^-16 + 3 2^-32 derived from bf16's half ulp <= 2^-8 |v| (module
                  docstring of f32_conv_cases.py), A = conv(|x|, |w|).
c, the longest chain of dependent roundings, read off each kernel:
  tiles 6-8, 38-40   conv_lds_kernel<.., F32, KG>: a K step is 32 input channels = three 16x16x32
                     MFMAs (NPASS = 3: (wh, xh), (wh, xl), (wl, xh)) into one accumulator; group g
                     of KG runs ceil(taps Ktot / 32 / KG) steps (RS_GLOAD stages zeros past the
                     end), group 0 adds the KG - 1 parked tiles in order:
                     c = 2 * 3 * ceil(steps / KG) + (KG - 1), + 1 for the bias add.
  tiles 81-85        conv_v3f_kernel: one accumulator per output over nchunks * NSL = taps Ktot / 16
                     slices, three 32x32x16 MFMAs per slice (V3F_GROUP x 3), no split-K:
                     c = 2 * 3 * taps * Ktot / 16, + 1 for the bias add.
  conv_geo           tiles 6 / 7 / 8 with KG = 1: c = 2 * 3 * taps * Cin / 32 (+ 1); the phase-split
                     dgrad: the 2 x 2 sub-kernel of a 3x3 / s2 conv (1 tap for 1x1) over Cout.
  epilogues          the formulas and bounds of update_conv_cases.py (epi_plain, epi_gru_zr, epi_gru_q,
                     epi_relu_bwd, epi_acc_f32, epi_gru_qbwd) and enc_conv_cases.epilogue (EPI_NORM)
                     on the product oracle, fp32 storage (no 2^-8 |want| term).
  weight gradients   three calls, each with its own chain ending in the add onto dw
                     (update_conv_cases.wgrad_chain / wgrad3_chain): dw 3 x, db 2 x (colsum of
                     dYh + dYl; the third call has no bias pointer); encoder: three calls into
                     zeroed accumulators (enc_wgrad_chain / wgrad_chain) and two adds, db = the
                     fp32 column sum of dY (torch.sum: bounded by P U Sb).
Inputs are windows of wider NaN-filled buffers, outputs live in NaN-filled buffers and must
still be NaN outside the written window; accumulating outputs start from a known random
prefill that must be bit-unchanged outside the window.  Planted: border pixels x 64, one output
cancelling to 2^-20 of its magnitude term through bias[0], one pixel whose channels all hold
1 + 2^-8 - 2^-20 (xh = 1, xl = +2^-8) under an all-positive weight row, one weight row of
the same values, the PLANT pre-activations, gates exactly 0 and 1, a ReLU output holding 0.0
and -0.0.  Deterministic routes are called twice and must be bit-equal.

split_bf16 at +-inf / NaN / fp32 values beyond the bf16 range: hi = rne(t) (inf, NaN, +-inf),
lo = rne(t - hi) = NaN, NaN, -+inf by the formula; asserted as such.

Measured on an MI355X (largest err / bound over the cases of each check group):
                                   product   value
  forward tiles 6-8, 38-40           0.466     0.286   (0.466: tile 39, 1x1 over 32 channels: one K step, c = 8)
  forward tiles 81-85                0.072     0.237
  conv_geo forward (6 / 7 / 8)       0.220     0.284
  phase-split dgrad                  0.177     0.082   stride-1 3x3 dgrad  0.021  0.056
  update-block wgrad (wgrad_v3)   dw 0.049     0.167   db 0.004  0.065
  update-block wgrad (conv_wgrad) dw 0.145     0.146   db 0.011  0.080  (atomic and deterministic)
  encoder wgrad                   dw 0.144     0.451   db 0.495 (torch.sum against P U Sb)
  epilogues (register tiles / tiles 81, 84), against the product oracle:
    bias / relu / scale 0.010 / 0.004   gru_zr 0.048 / 0.047   gru_q 0.549 / 0.545   relu_bwd 0.010 / 0.004
    acc_f32 0.013 / 0.004   gru_qbwd out 0.709 / 0.522, dr_pre 0.010 / 0.004   norm 0.770 / 0.770
  split_bf16: bit-equal at every size, fp32 subnormals and ties included.
No kernel missed a bound and no product ratio comes near 1; 3152 checks, 39 tests, 5.5 s for the
file (the slowest test 0.8 s).  The largest ratios are single roundings against bounds of a few
roundings, not accumulated error: EPI_NORM with the residual (0.770) and h' of EPI_GRU_Q (0.549)
are reproduced digit for digit by the plain fp32 evaluation on the CPU
(test_fp32_reference_under_the_epilogue_bounds prints norm 0.770, gru_q 0.549), and the
EPI_GRU_QBWD accumulate (0.709; 0.810 on the CPU) is the one rounding of out += v r where r is small.
"""
import math
from types import SimpleNamespace

import pytest
import torch

import enc_conv_cases as E
import f32_conv_cases as C
import update_conv_cases as UC
from f32_conv_cases import BF16, F32

pytestmark = pytest.mark.gpu

NAN = math.nan
WORST = {}
COUNT = [0]
TILES = C.tiles_under_test()
_DEV = {}


def _check(name, got, want, bound, dtype, op):
    """max|err| and err / bound over every element (0 / 0 counts as 0)."""
    assert got.dtype == dtype, name
    got = got.detach().cpu()
    assert tuple(got.shape) == tuple(want.shape), (name, got.shape, want.shape)
    assert bool(torch.isfinite(got).all()), name + ": not finite"
    r = C.ratio(got, want, bound, dtype)
    err = (got.double() - want).abs().max().item() if want.numel() else 0.0
    WORST[op] = max(WORST.get(op, 0.0), r)
    COUNT[0] += 1
    print(f"{name}: max|err| {err:.3e}  err/bound {r:.3f}  (worst {op}: {WORST[op]:.3f})")
    assert r <= 1.0, f"{name}: err/bound {r:.3f}"
    return r


def _nan_outside(buf, lo, hi, tag):
    keep = torch.ones(buf.shape[-1], dtype=torch.bool, device=buf.device)
    keep[lo:hi] = False
    assert bool(torch.isnan(buf[..., keep]).all()), tag + ": written outside the window"


def _same_outside(buf, buf0, lo, hi, tag):
    keep = torch.ones(buf.shape[-1], dtype=torch.bool, device=buf.device)
    keep[lo:hi] = False
    assert torch.equal(buf[..., keep], buf0[..., keep]), tag + ": changed outside the window"


def _window(t, off, width, dev, fill=NAN):
    buf = torch.full((*t.shape[:-1], width), fill, dtype=t.dtype)
    buf[..., off:off + t.shape[-1]] = t
    return buf.to(dev)


def _prefill(shape, width, dev, key):
    return torch.randn(*shape, width, generator=C.gen(*shape, width, key)).to(dev)


def _packed(key, w, layout, dev):
    """The split [wh | wl] packed weight with COUT_PAD rows, tagged with its fragment-major
    copy when every segment is a multiple of 64 channels (tiles 81-85)."""
    from raft_stir_amd.ops.conv import frag_weight_split, pack_weight_split
    k = ("w", key, layout)
    if k not in _DEV:
        ws = pack_weight_split(w.to(dev), C.pack_spec(layout), C.COUT_PAD)
        if all(c % 64 == 0 for _, _, c in C.LAYOUTS[layout]):
            ws._rs_frag32 = frag_weight_split(ws)
        _DEV[k] = ws
    return _DEV[k]


def _segs(key, x, layout, dev):
    k = ("x", key, layout)
    if k not in _DEV:
        _DEV[k] = [(b.to(dev), off, c) for b, off, c in C.seg_buffers(x, layout)]
    return _DEV[k]


def _conv(segs, ws, bias, kh, kw, cout, epi, out, ooff, tile, **kw_):
    from raft_stir_amd.ops.conv import conv_fused
    conv_fused(segs, ws, bias, kh, kw, cout, epi, out, ooff, tile=tile, **kw_)


# ------------------------------------------------------------------ forward, every tile
@pytest.mark.parametrize("tile", TILES)
def test_forward_every_tile(cuda, tile):
    g = C.tile_geom(tile)
    cases = [(shape, C.layout_for(tile, i), k) for i, shape in enumerate(C.shapes_for(tile)) for k in C.KERNELS]
    if g["kg"] > 1:  # one step with idle groups; three steps: uneven over 2 groups, one of 4 empty
        cases += [(shape, layout, (1, 1)) for layout, shape in C.SPLITK_EXTRA]
    ran = 0
    for shape, layout, (kh, kw) in cases:
        chans = [c for _, _, c in C.LAYOUTS[layout]]
        ktot = sum(chans)
        if not C.tile_accepts(tile, kh, kw, chans, C.FWD_COUTS[0]):
            continue
        c = C.fwd_case(*shape, kh, kw, ktot)
        key = (shape, kh, kw, ktot)
        segs, ws = _segs(key, c["x"], layout, cuda), _packed(key, c["w"], layout, cuda)
        bdev = c["bias"].to(cuda)
        chain = C.fwd_chain(tile, kh * kw, ktot, True)
        b3, bv = C.product_bound(chain, c["A3"]), C.value_bound(chain, c["A3"], c["A"])
        for cout in C.couts_for(tile):
            out = torch.full((*shape, cout + 8), NAN, device=cuda, dtype=F32)
            _conv(segs, ws, bdev, kh, kw, cout, C.EPI_BIAS, out, 4, tile)
            tag = f"tile {tile} {kh}x{kw} {shape} {layout} cout {cout}"
            got = out[..., 4:4 + cout]
            _check(tag + " product", got, c["want3"][..., :cout], b3[..., :cout], F32, f"forward {g['family']} product")
            _check(tag + " value", got, c["want"][..., :cout], bv[..., :cout], F32, f"forward {g['family']} value")
            _nan_outside(out, 4, 4 + cout, tag)
            ran += 1
    assert ran >= 6, f"tile {tile}: only {ran} cases ran"


# ------------------------------------------------------------------ epilogues against formulas
def _pad4(n):
    return (n + 3) // 4 * 4


@pytest.mark.parametrize("form", ["vector", "elementwise"])
@pytest.mark.parametrize("tile", C.EPI_TILES)
def test_epilogues_against_formulas(cuda, tile, form):
    """A plain register tile, a split-K tile and the two wave layouts of conv_v3f.hip; the vector
    form (every offset and stride % 4) and the element-wise form (odd offsets and strides,
    Cout % 4 != 0 where the epilogue allows it)."""
    vec = form == "vector"
    kh, kw = 3, 3
    hd = C.EPI_HD
    fam = C.tile_geom(tile)["family"]
    ooff, a1off, a2off, o2off, o3off = (4, 8, 4, 8, 4) if vec else (2, 6, 2, 2, 6)

    def wd(n):  # buffer width around an n-channel window
        return _pad4(n + 12) if vec else n + 7 + (1 if (n + 7) % 4 == 0 else 0)

    for shape in C.EPI_SHAPES:
        e = C.epi_case(*shape, kh, kw)
        key = ("epi", shape, kh, kw)
        segs, ws = _segs(key, e["x"], "64x2", cuda), _packed(key, e["w"], "64x2", cuda)
        bias = e["bias"].to(cuda)
        pb = C.product_bound(C.fwd_chain(tile, kh * kw, UC.KTOT, True), e["A3"])
        pb0 = C.product_bound(C.fwd_chain(tile, kh * kw, UC.KTOT, False), e["A30"])
        pre, pre0 = e["pre"], e["pre0"]
        tag0 = f"tile {tile} {form} {shape}"

        def run(cout, epi, out, **kw_):
            _conv(segs, ws, kw_.pop("bias", None), kh, kw, cout, epi, out, ooff, tile, **kw_)

        def nanbuf(n):
            return torch.full((*shape, wd(n)), NAN, device=cuda, dtype=F32)

        # --- bias / relu / scale
        n = 96 if vec else 70
        for epi, name in ((C.EPI_BIAS, "bias"), (C.EPI_RELU, "relu"), (C.EPI_SCALE, "scale")):
            want, b = UC.epi_plain(pre[..., :n], pb[..., :n], epi, 0.25)
            out = nanbuf(n)
            run(n, epi, out, bias=bias, scale=0.25)
            _check(f"{tag0} {name}", out[..., ooff:ooff + n], want, b, F32, f"bias/relu/scale {fam}")
            _nan_outside(out, ooff, ooff + n, tag0 + name)
        # --- EPI_GRU_ZR (z | r conv, Cout = 2 hd), with and without out3
        h = e["h"][..., :hd]
        hbuf = _window(h, a1off, wd(hd), cuda)
        (z, bz), (rh, brh), (r, br) = UC.epi_gru_zr(pre, pb, h, hd)
        for with3 in (True, False):
            out, out2, out3 = nanbuf(hd), nanbuf(hd), nanbuf(hd)
            run(2 * hd, C.EPI_GRU_ZR, out, bias=bias, hd=hd, out2=out2, o2off=o2off, out3=out3 if with3 else None,
                o3off=o3off, aux1=hbuf, a1off=a1off)
            _check(f"{tag0} gru_zr z", out[..., ooff:ooff + hd], z, bz, F32, f"gru_zr {fam}")
            _check(f"{tag0} gru_zr rh", out2[..., o2off:o2off + hd], rh, brh, F32, f"gru_zr {fam}")
            _nan_outside(out, ooff, ooff + hd, tag0 + " z")
            _nan_outside(out2, o2off, o2off + hd, tag0 + " rh")
            if with3:
                _check(f"{tag0} gru_zr r", out3[..., o3off:o3off + hd], r, br, F32, f"gru_zr {fam}")
                _nan_outside(out3, o3off, o3off + hd, tag0 + " r")
            else:
                assert bool(torch.isnan(out3).all())
        # --- EPI_GRU_Q (Cout = hd), with and without out2
        zg = e["z"][..., :hd]
        zbuf = _window(zg, a2off, wd(hd), cuda)
        (hn, bhn), (q, bq) = UC.epi_gru_q(pre[..., :hd], pb[..., :hd], h, zg)
        for with2 in (True, False):
            out, out2 = nanbuf(hd), nanbuf(hd)
            run(hd, C.EPI_GRU_Q, out, bias=bias, out2=out2 if with2 else None, o2off=o2off, aux1=hbuf, a1off=a1off,
                aux2=zbuf, a2off=a2off)
            _check(f"{tag0} gru_q h'", out[..., ooff:ooff + hd], hn, bhn, F32, f"gru_q {fam}")
            _nan_outside(out, ooff, ooff + hd, tag0 + " h'")
            if with2:
                _check(f"{tag0} gru_q q~", out2[..., o2off:o2off + hd], q, bq, F32, f"gru_q {fam}")
                _nan_outside(out2, o2off, o2off + hd, tag0 + " q~")
            else:
                assert bool(torch.isnan(out2).all())
        # --- EPI_RELU_BWD (no bias)
        av = e["actv"][..., :n]
        want, b = UC.epi_relu_bwd(pre0[..., :n], pb0[..., :n], av)
        out = nanbuf(n)
        run(n, C.EPI_RELU_BWD, out, aux1=_window(av, a1off, wd(n), cuda), a1off=a1off)
        _check(f"{tag0} relu_bwd", out[..., ooff:ooff + n], want, b, F32, f"relu_bwd {fam}")
        _nan_outside(out, ooff, ooff + n, tag0 + " relu_bwd")
        masked = (av.double() <= 0)
        assert bool((out[..., ooff:ooff + n].cpu()[masked] == 0).all()), tag0 + ": masked outputs must be exactly 0"
        # --- EPI_ACC_F32: known random prefill, exact outside the window
        o0 = _prefill(shape, wd(n), cuda, 1)
        out = o0.clone()
        run(n, C.EPI_ACC_F32, out)
        want, b = UC.epi_acc_f32(pre0[..., :n], pb0[..., :n], o0[..., ooff:ooff + n].cpu())
        _check(f"{tag0} acc_f32", out[..., ooff:ooff + n], want, b, F32, f"acc_f32 {fam}")
        _same_outside(out, o0, ooff, ooff + n, tag0 + " acc_f32")
        # --- EPI_GRU_QBWD (hd <= Cout; channels >= hd accumulate v)
        nq = 96 if vec else 94
        oq0 = _prefill(shape, wd(nq), cuda, 2)
        out = oq0.clone()
        out2 = nanbuf(hd)
        run(nq, C.EPI_GRU_QBWD, out, hd=hd, out2=out2, o2off=o2off, aux1=hbuf, a1off=a1off, aux2=zbuf, a2off=a2off)
        (wo, bo), (dr, bd) = UC.epi_gru_qbwd(pre0[..., :nq], pb0[..., :nq], h, zg, oq0[..., ooff:ooff + nq].cpu(), hd)
        _check(f"{tag0} gru_qbwd out", out[..., ooff:ooff + nq], wo, bo, F32, f"gru_qbwd out {fam}")
        _check(f"{tag0} gru_qbwd dr_pre", out2[..., o2off:o2off + hd], dr, bd, F32, f"gru_qbwd dr_pre {fam}")
        _same_outside(out, oq0, ooff, ooff + nq, tag0 + " gru_qbwd")
        _nan_outside(out2, o2off, o2off + hd, tag0 + " dr_pre")
        # --- EPI_NORM: scale + shift; + ReLU; + residual
        sc, sh = e["nscale"][:_pad4(n)].contiguous().to(cuda), e["nshift"][:_pad4(n)].contiguous().to(cuda)
        resw = _window(e["res"][..., :n], a1off, wd(n), cuda)
        for relu, use_res in C.NORM_KINDS:
            want, b = C.epi_norm(pre0[..., :n], pb0[..., :n], e["nscale"][:n], e["nshift"][:n], relu,
                                 e["res"][..., :n] if use_res else None)
            out = nanbuf(n)
            run(n, C.EPI_NORM, out, bias=sh, hd=int(relu), aux1=resw if use_res else None, a1off=a1off, nscale=sc)
            _check(f"{tag0} norm relu {relu} res {use_res}", out[..., ooff:ooff + n], want, b, F32, f"norm {fam}")
            _nan_outside(out, ooff, ooff + n, tag0 + " norm")


# ------------------------------------------------------------------ conv_geo (fp32) and the input gradients
def _geo_weight(w, cout, dev):
    from raft_stir_amd.ops.conv import pack_weight_split, pad_to
    cin = w.shape[1]
    return pack_weight_split(w.to(dev), [(cin, [(0, cin, 0)])], pad_to(cout, 128))


@pytest.mark.parametrize("tile", [6, 7, 8])
def test_conv_geo_f32_forward(cuda, tile):
    for k, s, p in C.GEO_KSP:
        for H, W in C.GEO_HW:
            for cin, cout in C.GEO_CH:
                c = C.geo_case(C.GEO_B, H, W, cin, cout, k, s, p)
                Ho, Wo = E.out_hw(H, W, k, s, p)
                key = ("geo", H, W, cin, cout, k, s)
                if key not in _DEV:
                    _DEV[key] = (_window(c["x"], 8, cin + 16, cuda), _geo_weight(c["w"], cout, cuda),
                                 c["bias"].to(cuda))
                xb, wp, bias = _DEV[key]
                out = torch.full((C.GEO_B, Ho, Wo, cout + 8), NAN, device=cuda, dtype=F32)
                torch.ops.raft_stir.conv_geo([xb], [8], [cin], wp, bias, k, k, p, p, s, s, Ho, Wo, cout, out, 4,
                                             1, 1, 0, 0, tile)
                chain = C.geo_chain(k * k, cin, True)
                tag = f"conv_geo tile {tile} {k}x{k}/s{s} {H}x{W} {cin}->{cout}"
                got = out[..., 4:4 + cout]
                _check(tag + " product", got, c["want3"], C.product_bound(chain, c["A3"]), F32, "conv_geo product")
                _check(tag + " value", got, c["want"], C.value_bound(chain, c["A3"], c["A"]), F32, "conv_geo value")
                _nan_outside(out, 4, 4 + cout, tag)


def test_conv_geo_f32_dgrad(cuda):
    from raft_stir_amd.ops.enc_conv import _conv_geo_dgrad
    for k, s, p in C.GEO_KSP:
        for H, W in C.GEO_HW:
            for cin, cout in C.GEO_CH:
                d = C.dgrad_case(C.GEO_B, H, W, cin, cout, k, s, p)
                key = ("geo_dgrad", H, W, cin, cout, k, s)
                if key not in _DEV:  # (the packed phase weights are keyed on the weight tensor: keep it alive)
                    _DEV[key] = (d["dy"].to(cuda), d["w"].to(cuda))
                dy, w = _DEV[key]
                dx = _conv_geo_dgrad([dy], [w], (C.GEO_B, cin, H, W), (s, s), (p, p), f32=True)
                chain = C.geo_dgrad_chain(k, cout)
                tag = f"geo dgrad {k}x{k}/s{s} {H}x{W} {cin}<-{cout}"
                _check(tag + " product", dx, d["dx3"], C.product_bound(chain, d["T3"]), F32, "geo dgrad product")
                _check(tag + " value", dx, d["dx"], C.value_bound(chain, d["T3"], d["T"]), F32, "geo dgrad value")
                if s == 2 and k == 1:  # phases without taps are exactly zero
                    assert bool((dx[:, 1::2] == 0).all()) and bool((dx[:, :, 1::2] == 0).all())


def _auto_tile(B, H, W, cout, chans, kh, kw, epi, has32):
    """ops/conv.py conv_fused's fp32 tile choice for tile=None."""
    from raft_stir_amd.ops import conv as oc
    tile = oc.tuned_tiles_f32().get(oc.tune_key(B, H, W, cout, chans, kh, kw, epi))
    if tile is None or (tile in oc.V3F_TILES and not (has32 and oc._V3F)):
        tile = oc.choose_tile_f32(B * H * W, cout, v3f=has32, taps=kh * kw, ktot=sum(chans))
    return tile


def test_conv_f32_stride1_dgrad(cuda):
    """The input gradient of _ConvF32.backward for a stride-1 3x3 conv: conv_fused of dY with the
    flipped, transposed split weight, on the tile conv_fused picks."""
    from raft_stir_amd.ops import enc_conv as EC
    for shape in C.DGRAD_S1_SHAPES:
        B, H, W = shape
        for cin, cout in C.DGRAD_S1_CH:
            d = C.dgrad_case(B, H, W, cin, cout, 3, 1, 1)
            conv = torch.nn.Conv2d(cin, cout, 3, padding=1, bias=False).to(cuda)
            _DEV[("conv", shape, cin, cout)] = conv  # (packed layouts are keyed on the parameter: keep it alive)
            with torch.no_grad():
                conv.weight.copy_(d["w"].to(cuda))
            conv.weight.requires_grad_(False)
            x = torch.zeros(B, H, W, cin, device=cuda).permute(0, 3, 1, 2).requires_grad_(True)
            assert EC.eligible_f32_train(conv, x)
            out = EC.conv_f32_train(conv, x, bias=False)
            out.backward(d["dy"].to(cuda).permute(0, 3, 1, 2))
            dx = x.grad.permute(0, 2, 3, 1).contiguous()
            has32 = cin % 64 == 0 and cout % 64 == 0
            tile = _auto_tile(B, H, W, cin, [cout], 3, 3, C.EPI_BIAS, has32)
            chain = C.fwd_chain(tile, 9, cout, False)
            tag = f"s1 dgrad {shape} {cin}<-{cout} tile {tile}"
            _check(tag + " product", dx, d["dx3"], C.product_bound(chain, d["T3"]), F32, "s1 dgrad product")
            _check(tag + " value", dx, d["dx"], C.value_bound(chain, d["T3"], d["T"]), F32, "s1 dgrad value")


# ------------------------------------------------------------------ split_bf16, bit for bit
@pytest.mark.parametrize("n", C.SPLIT_SIZES)
def test_split_bf16_exact(cuda, n):
    t = C.split_values(n)
    hi, lo = torch.ops.raft_stir.split_bf16(t.to(cuda))
    whi, wlo = C.split_oracle(t)
    assert hi.dtype == BF16 and lo.dtype == BF16 and hi.shape == t.shape and lo.shape == t.shape
    bits = lambda v: v.cpu().view(torch.int16)
    bad = (bits(hi) != bits(whi)) | (bits(lo) != bits(wlo))
    print(f"split_bf16 n {n}: {int(bad.sum())} of {n} differ", t[bad][:8].tolist(), hi.cpu()[bad][:8].tolist(),
          lo.cpu()[bad][:8].tolist())
    COUNT[0] += 1
    assert not bool(bad.any())


def test_split_bf16_specials(cuda):
    """inf / NaN / beyond the bf16 range, in the vector body (first 4) and the scalar tail."""
    t = C.split_specials()
    assert t.numel() == 7
    hi, lo = (v.cpu().float() for v in torch.ops.raft_stir.split_bf16(t.to(cuda)))
    print("split_bf16 specials:", t.tolist(), hi.tolist(), lo.tolist())
    inf = math.inf
    assert hi[0] == inf and hi[1] == -inf and math.isnan(hi[2]) and hi[3] == inf and hi[4] == -inf
    assert math.isnan(lo[0]) and math.isnan(lo[1]) and math.isnan(lo[2]) and lo[3] == -inf and lo[4] == inf
    whi, wlo = C.split_oracle(t)
    assert torch.equal(hi[5:], whi[5:].float()) and torch.equal(lo[5:], wlo[5:].float())
    # the same values in the tail positions of a 7-vector rolled by 4
    t2 = t.roll(3)
    hi2, lo2 = (v.cpu().float() for v in torch.ops.raft_stir.split_bf16(t2.to(cuda)))
    assert torch.equal(hi2.roll(-3).nan_to_num(7.0), hi.nan_to_num(7.0))
    assert torch.equal(lo2.roll(-3).nan_to_num(7.0), lo.nan_to_num(7.0))


# ------------------------------------------------------------------ three-product weight gradients
@pytest.mark.parametrize("det", [False, True], ids=["atomic", "deterministic"])
def test_update_block_wgrad_three_products(cuda, det):
    from raft_stir_amd.models import fused_train as FT
    R = torch.ops.raft_stir
    was = R.is_deterministic()
    R.set_deterministic(det)
    try:
        for stack in C.WG_STACKS:
            it, B, H, W = stack
            for kh, kw, cout in C.WG_KC:
                route, bm = C.wgrad_route(kh, kw, cout)
                if route == "v3" and det:
                    continue  # wgrad_v3 has one (deterministic) mode: run with the atomic pass
                c = C.wgrad_case(*stack, kh, kw)
                key = ("wg", stack, kh, kw)
                if key not in _DEV:
                    _DEV[key] = [(_window(c["x0"], 8, C.WG_SEG + 16, cuda), 8, C.WG_SEG),
                                 (c["xb"].to(cuda), 0, C.WG_SEG), (c["x2"].to(cuda), 0, C.WG_SEG)]
                segs = _DEV[key]
                dyb = UC.dy_buffer(c["dy"], cout).to(cuda)
                taps = kh * kw
                dw0 = torch.randn(cout + 3, taps, C.WG_KTOT, device=cuda)
                db0 = torch.randn(cout + 3, device=cuda)

                def call():
                    pc = SimpleNamespace(cout=cout, kh=kh, kw=kw, dw=dw0.clone(), db=db0.clone())
                    FT._conv_wgrad(SimpleNamespace(f32=True), pc, dyb, C.WG_YOFF, segs, H, W)
                    return pc.dw, pc.db

                dw, db = call()
                cd, cb = C.wgrad_chains(route, bm, stack, kh, kw, cout, det)
                d0, b0 = dw0[:cout].cpu().double(), db0[:cout].cpu().double()
                S3 = d0.abs() + UC.kernel_layout(c["S3"][:cout])
                tag = f"update wgrad {route} det {det} {kh}x{kw} {stack} cout {cout}"
                _check(tag + " dw product", dw[:cout], d0 + UC.kernel_layout(c["dw3"][:cout]), C.acc_bound(cd, S3), F32,
                       f"update wgrad {route} dw product")
                _check(tag + " dw value", dw[:cout], d0 + UC.kernel_layout(c["dw"][:cout]),
                       C.acc_bound(cd, S3) + C.SPLIT * UC.kernel_layout(c["S"][:cout]), F32,
                       f"update wgrad {route} dw value")
                Sb3 = b0.abs() + c["Sb3"][:cout]
                _check(tag + " db product", db[:cout], b0 + c["db3"][:cout], C.acc_bound(cb, Sb3), F32,
                       f"update wgrad {route} db product")
                _check(tag + " db value", db[:cout], b0 + c["db"][:cout],
                       C.acc_bound(cb, Sb3) + 2.0 ** -16 * c["Sb"][:cout], F32, f"update wgrad {route} db value")
                assert torch.equal(dw[cout:], dw0[cout:]) and torch.equal(db[cout:], db0[cout:]), tag + ": rows >= Cout"
                if route == "v3" or det:  # deterministic: bit-equal from the same start
                    dw2, db2 = call()
                    assert torch.equal(dw2, dw) and torch.equal(db2, db), tag + ": two calls differ"
    finally:
        R.set_deterministic(was)


@pytest.mark.parametrize("k,s,p", C.ENC_WG_KSP)
def test_encoder_wgrad_three_products(cuda, k, s, p):
    from raft_stir_amd.ops.enc_conv import _f32_wgrad
    for shape in C.ENC_WG_SHAPES[s]:
        B, H, W = shape
        for cin, cout in C.ENC_WG_CH:
            c = C.enc_wgrad_case(B, H, W, cin, cout, k, s, p)
            conv = torch.nn.Conv2d(cin, cout, k, stride=s, padding=p).to(cuda)
            x = c["x"].to(cuda).permute(0, 3, 1, 2)
            dyn = c["dy"].to(cuda)
            dw, db = _f32_wgrad(conv, dyn, x, True, True)
            chain = C.enc_wgrad_chain(B, H, W, cin, cout, k, s, p)
            tag = f"encoder wgrad {k}x{k}/s{s} {shape} {cin}->{cout}"
            assert tuple(dw.shape) == (cout, cin, k, k)
            _check(tag + " dw product", dw, c["dw3"], C.acc_bound(chain, c["S3"]), F32, "encoder wgrad dw product")
            _check(tag + " dw value", dw, c["dw"], C.acc_bound(chain, c["S3"]) + C.SPLIT * c["S"], F32,
                   "encoder wgrad dw value")
            P = dyn.shape[0] * dyn.shape[1] * dyn.shape[2]
            _check(tag + " db", db, c["db"], C.acc_bound(P, c["Sb"]), F32, "encoder wgrad db")
            if (k, s) == (3, 1):  # enc_wgrad reduces its splits in a fixed order
                dw2, _ = _f32_wgrad(conv, dyn, x, True, False)
                assert torch.equal(dw2, dw), tag + ": two calls differ"


# ------------------------------------------------------------------ host rejections (no launch)
def test_host_rejections(cuda):
    from raft_stir_amd.ops.conv import conv_fused
    shape = (1, 5, 7)
    e = C.epi_case(*shape, 3, 3)
    key = ("epi", shape, 3, 3)
    segs, ws = _segs(key, e["x"], "64x2", cuda), _packed(key, e["w"], "64x2", cuda)
    out = torch.full((*shape, 104), NAN, device=cuda, dtype=F32)
    crd = torch.full((1, 2, 5, 7), NAN, device=cuda, dtype=F32)
    with pytest.raises(RuntimeError, match="no flow epilogue"):
        conv_fused(segs, ws, None, 3, 3, 2, C.EPI_FLOW, crd, 0, tile=7)
    for tile in (70, 3, 17, 41, 5, 61, 45):  # the bf16 1x1 GEMM and bf16 tiles of every family
        with pytest.raises((RuntimeError, ValueError), match="fp32 activations run on tiles|fragment-major"):
            conv_fused(segs, ws, None, 3, 3, 96, C.EPI_BIAS, out, 0, tile=tile)
    with pytest.raises(RuntimeError, match="fp32 activations run on tiles"):  # tile 70 with its own 1x1 shape
        conv_fused(segs, ws, None, 1, 1, 96, C.EPI_BIAS, out, 0, tile=70)
    segs32 = _segs(key, e["x"], "32x3", cuda)
    ws32 = _packed(key, e["w"], "32x3", cuda).view(ws.shape)  # (a fresh tensor object for the tag)
    ws32._rs_frag32 = ws._rs_frag32  # shape-compatible: the host must refuse on the segment widths
    with pytest.raises(RuntimeError, match="% 64"):
        conv_fused(segs32, ws32, None, 3, 3, 96, C.EPI_BIAS, out, 0, tile=81)
    with pytest.raises(RuntimeError, match="tile 85"):  # Ktot 192 on the single-buffer tile
        conv_fused(segs, ws, None, 3, 3, 64, C.EPI_BIAS, out, 0, tile=85)
    with pytest.raises(RuntimeError, match="3x3, 1x5 and 5x1"):
        conv_fused(segs, ws, None, 1, 1, 96, C.EPI_BIAS, out, 0, tile=81)
    assert bool(torch.isnan(out).all()) and bool(torch.isnan(crd).all())


def test_zz_report(cuda):
    """Prints the largest err / bound per check group of this run (run the file with -s)."""
    print(f"{COUNT[0]} checks")
    for op in sorted(WORST):
        print(f"  worst {op}: {WORST[op]:.3f}")

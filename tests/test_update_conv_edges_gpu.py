"""The bf16 update-block convolution family, each kernel on its own, per element vs fp64 oracles.

conv_fused on every kernel template of csrc/conv.hip (conv_kernel, conv_lds_kernel,
conv_glds_kernel, conv_buf_kernel, conv_halo_kernel, conv_smalln_kernel), conv_v2.hip,
conv_v3.h and conv_gemm1.hip with every epilogue of conv_common.h; the stride-1 weight
gradients of conv_wgrad.hip (tile variants 0-5, atomic and deterministic, colsum) and
wgrad_v3.hip; gru_gate_bwd and relu_take.  Shapes are the smallest that reach every path:
H = 1, W = 1, one pixel, less than one patch, pixel counts one below / at / above a
64- / 128- / 192-pixel tile with images straddling a tile, stacks shorter than one
64-pixel K step.  The tile list is read at collection time: conv_tuning.json's tiles,
everything choose_tile returns, and one tile of each kernel template those do not reach
(update_conv_cases.tiles_under_test), so a retune extends the test.

The oracles (tests/update_conv_cases.py; tests/test_update_conv_oracles_cpu.py ties them
to autograd, shows that a plain fp32 evaluation stays inside every bound and that eight
mutants leave it) are float64 on the CPU, evaluated on the values the kernels read.  Every
check prints max|err| and err / bound and asserts dtype, finiteness and ratio <= 1 for
EVERY element.  Inputs are windows of wider NaN-filled buffers (a read outside the window
poisons the result), outputs live in NaN-filled buffers and everything outside the written
window must still be NaN; the accumulating fp32 outputs start from a known random prefill
that must be unchanged, bit for bit, outside the window.  Planted: border pixels x 64 next
to a unit-scale interior (a wrapped or dropped tap is many bounds off), one output per
forward case that cancels to 2^-20 of its magnitude term (there the bf16 storage term
vanishes), pre-activations exactly 0, +-1e-3, +-20, +-88, +-100, +-1e4 (zero weight rows,
the value as bias), a ReLU output holding 0.0, -0.0, the smallest positive normal and
subnormal bf16, gates exactly 0 and 1, the broadcast segment's image b constant b + 1.

Bounds.  U = 2^-24; an fp32 FMA / add counts 1 U of the magnitude term, an MFMA step 2 U;
a bf16 store adds 2^-8 |want|.  A = conv(|x|, |w|) + |bias|, S = wgrad(|x|, |dy|) + |dw0|.
c is the longest chain of dependent roundings, read off each kernel:

forward        every kernel keeps ONE accumulator per output over the whole K walk:
               c = 2 * taps * Ktot / 32 on the 16x16x32 MFMAs (conv_kernel, conv_lds, conv_glds,
               conv_buf, conv_halo: a 64-deep staged step is two of them), 2 * taps * Ktot / 16
               on the 32x32x16 MFMAs of conv_v2 / conv_v3 / conv_gemm1; + 1 for the bias add.
               Intra-block split-K (tile 41: 4 groups of 32-deep steps; 34-36: 2, 37: 4 groups
               of 64-deep steps): c = 2 * ceil(steps / KG) * MFMAs per step + (KG - 1) adds in
               group order; tile 5: ceil(steps / 4) per wave + the 3 adds of the four partials.
epilogues      ReLU and the ReLU-backward mask are exact (the mask is read from the stored aux1:
               0.0 and -0.0 give exactly 0, bound 0); scale: |scale| bound + U |want|; fp32
               accumulate: bound + U |want|; sigmoid / tanh: 2^-20 (1 + |pre|) (test_gates_gpu.py)
               + the accumulation bound through Lipschitz 1/4 / 1; r h: |h| bound_r + U |r h|;
               h' = (1 - z) h + z q~: |z| bound_q + U (2 |(1-z) h| + |z q~| + |h'|);
               EPI_GRU_QBWD: dr_pre = v h r (1 - r): |h r (1-r)| bound + 4 U |dr_pre|,
               out += v r: |r| bound + U |v r| + U |out|; EPI_FLOW: bound + U |coords|.
conv_wgrad     c = 2 * 2 * kchunk / 64 + ksplit + 1 (two MFMAs per 64-pixel K step, one add per
               split -- atomic or det_reduce's ordered sum -- and the add onto dw);
               db: 64 (BM / 8) / threads rows per thread per K step + threads / (BM / 8)
               threads per column + ksplit + 1.
wgrad_v3       c = 2 * 8 * patches_per_block + splits (8 K steps of 16 pixels per 4 x 32 patch;
               wg3_reduce adds the splits in order, then onto dw); db: 8 * 8 * patches + 1 + splits + 1.
colsum         c = min(P, 256) + blocks + 1.
gru_gate_bwd   dq: U (|dh z| q~^2 + 4 |dq|) (q~ q~ rounds before 1 - . cancels), dz: 5 U |dz|,
               dh: 2 U |dh|; relu_take: exact.
Deterministic kernels (conv_wgrad and colsum in deterministic mode, wgrad_v3) are called
twice and must be bit-equal.

relu_take used to leave G[:, goff+out_width : goff+nz] un-zeroed when nz exceeded the
output's width (its loop runs over the output's channels); the host now rejects such a
call, which test_relu_take asserts.

Measured on an MI355X (largest err / bound over the cases of each check group):
  forward (25 tiles, every template)   0.995 (the half ulp of bf16)
  bias / relu / scale 0.993   gru_zr 0.987   gru_q 0.992   relu_bwd 0.986   gru_qbwd dr_pre 0.993 (bf16)
  acc_f32 0.067   flow 0.035   gru_qbwd out 0.865 (fp32, see below)
  conv_wgrad   dw 0.435  db 0.045 (atomic and deterministic)   colsum 0.332
  wgrad_v3     dw 0.130  db 0.015
  gru_gate_bwd bf16 0.989 (dh 0.500); fp32 dq / dz 0.730, dh 0.941 (see below)   relu_take 0.993 (bf16; fp32 exact)
No kernel missed its bound; 5940 checks, 66 tests, 7 s for the file (the slowest test 0.6 s).
The fp32 ratios near 1 are single roundings, not accumulated error: where r is small
(r = 2^-12 at the worst element) the EPI_GRU_QBWD bound |r| bound + U |v r| + U |out| is the
one rounding of the final add, U |out|, which a round-to-nearest add reaches when the sum
sits just above a power of two; a plain fp32 evaluation on the CPU gives the same 0.865 at
the same element.  gru_gate_bwd's dh = dh' (1 - z) is two roundings against a bound of two.
"""
import math

import pytest
import torch

import update_conv_cases as C
from update_conv_cases import BF16, F32

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
    """``t`` at channel ``off`` of a ``width``-channel buffer filled with ``fill``."""
    buf = torch.full((*t.shape[:-1], width), fill, dtype=t.dtype)
    buf[..., off:off + t.shape[-1]] = t
    return buf.to(dev)


def _prefill(shape, width, dev, key):
    """A known random fp32 prefill of an accumulating output."""
    return torch.randn(*shape, width, generator=C.gen(*shape, width, key)).to(dev)


def _packed(key, w, layout, dev):
    """(packed weight with COUT_PAD rows, its fragment-major copy), cached on the device."""
    from raft_stir_amd.ops.conv import frag_weight, pack_weight
    k = ("w", key, layout)
    if k not in _DEV:
        wp = pack_weight(w.to(dev), C.pack_spec(layout), C.COUT_PAD)
        _DEV[k] = (wp, frag_weight(wp))
    return _DEV[k]


def _segs(key, x, layout, dev):
    k = ("x", key, layout)
    if k not in _DEV:
        _DEV[k] = [(b.to(dev), off, c) for b, off, c in C.seg_buffers(x, layout)]
    return _DEV[k]


def _conv(segs, wpf, bias, kh, kw, cout, epi, out, ooff, tile, **kw_):
    from raft_stir_amd.ops.conv import conv_fused
    conv_fused(segs, wpf[0], bias, kh, kw, cout, epi, out, ooff, tile=tile, wf=wpf[1], **kw_)


# ------------------------------------------------------------------ forward, every kernel template
@pytest.mark.parametrize("tile", TILES)
def test_forward_every_tile(cuda, tile):
    fam = C.tile_geom(tile)["family"]
    ran = 0
    for i, shape in enumerate(C.shapes_for(tile)):
        layout = C.layout_for(tile, i)
        chans = [c for _, _, c in C.LAYOUTS[layout]]
        for kh, kw in C.KERNELS:
            couts = C.SMALLN_COUTS if tile == 5 else C.FWD_COUTS
            if not C.tile_accepts(tile, kh, kw, chans, couts[0]):
                continue
            x, w, bias, want, A = C.fwd_case(*shape, kh, kw)
            key = (shape, kh, kw)
            segs, wpf = _segs(key, x, layout, cuda), _packed(key, w, layout, cuda)
            bdev = bias.to(cuda)
            bound = C.acc_bound(C.fwd_chain(tile, kh * kw, C.KTOT, True), A)
            for cout in couts:
                out = torch.full((*shape, cout + 8), NAN, device=cuda, dtype=BF16)
                _conv(segs, wpf, bdev, kh, kw, cout, C.EPI_BIAS, out, 4, tile)
                tag = f"tile {tile} ({fam}) {kh}x{kw} {shape} {layout} cout {cout}"
                _check(tag, out[..., 4:4 + cout], want[..., :cout], bound[..., :cout], BF16, "forward")
                _nan_outside(out, 4, 4 + cout, tag)
                ran += 1
    assert ran >= 6, f"tile {tile}: only {ran} cases ran"


# ------------------------------------------------------------------ epilogues against formulas
def _family_tiles():
    out = {}
    for t in TILES:
        fam = C.tile_geom(t)["family"]
        if fam in ("lds", "buf", "halo", "v2", "v3", "gemm1"):
            out.setdefault(fam, t)
    return sorted(out.values())


def _pad4(n):
    return (n + 3) // 4 * 4


@pytest.mark.parametrize("form", ["vector", "elementwise"])
@pytest.mark.parametrize("tile", _family_tiles())
def test_epilogues_against_formulas(cuda, tile, form):
    """One tile of each kernel family; the vector form (every offset and stride % 4) and the
    element-wise form (odd offsets and strides, Cout % 4 != 0 where the epilogue allows it)."""
    vec = form == "vector"
    kh, kw = (1, 1) if C.tile_geom(tile)["family"] == "gemm1" else (3, 3)
    hd = C.EPI_HD
    ooff, a1off, a2off, o2off, o3off = (4, 8, 4, 8, 4) if vec else (2, 6, 2, 2, 6)

    def wd(n):  # buffer width around an n-channel window
        return _pad4(n + 12) if vec else n + 7 + (1 if (n + 7) % 4 == 0 else 0)

    for shape in C.EPI_SHAPES:
        e = C.epi_case(*shape, kh, kw)
        key = ("epi", shape, kh, kw)
        segs, wpf = _segs(key, e["x"], "64x2", cuda), _packed(key, e["w"], "64x2", cuda)
        bias = e["bias"].to(cuda)
        pb = C.acc_bound(C.fwd_chain(tile, kh * kw, C.KTOT, True), e["A"])
        pb0 = C.acc_bound(C.fwd_chain(tile, kh * kw, C.KTOT, False), e["A0"])
        pre, pre0 = e["pre"], e["pre0"]
        tag0 = f"tile {tile} {form} {shape}"

        def run(cout, epi, out, **kw_):
            _conv(segs, wpf, kw_.pop("bias", None), kh, kw, cout, epi, out, ooff, tile, **kw_)

        def nanbuf(n, dtype=BF16):
            return torch.full((*shape, wd(n)), NAN, device=cuda, dtype=dtype)

        # --- bias / relu / scale
        n = 96 if vec else 70
        for epi, name in ((C.EPI_BIAS, "bias"), (C.EPI_RELU, "relu"), (C.EPI_SCALE, "scale")):
            want, b = C.epi_plain(pre[..., :n], pb[..., :n], epi, 0.25)
            out = nanbuf(n)
            run(n, epi, out, bias=bias, scale=0.25)
            _check(f"{tag0} {name}", out[..., ooff:ooff + n], want, b, BF16, "bias/relu/scale")
            _nan_outside(out, ooff, ooff + n, tag0 + name)
        # --- EPI_GRU_ZR (z | r conv, Cout = 2 hd), with and without out3
        h = e["h"][..., :hd]
        hbuf = _window(h, a1off, wd(hd), cuda)
        (z, bz), (rh, brh), (r, br) = C.epi_gru_zr(pre, pb, h, hd)
        for with3 in (True, False):
            out, out2, out3 = nanbuf(hd), nanbuf(hd), nanbuf(hd)
            run(2 * hd, C.EPI_GRU_ZR, out, bias=bias, hd=hd, out2=out2, o2off=o2off, out3=out3 if with3 else None,
                o3off=o3off, aux1=hbuf, a1off=a1off)
            _check(f"{tag0} gru_zr z", out[..., ooff:ooff + hd], z, bz, BF16, "gru_zr")
            _check(f"{tag0} gru_zr rh", out2[..., o2off:o2off + hd], rh, brh, BF16, "gru_zr")
            _nan_outside(out, ooff, ooff + hd, tag0 + " z")
            _nan_outside(out2, o2off, o2off + hd, tag0 + " rh")
            if with3:
                _check(f"{tag0} gru_zr r", out3[..., o3off:o3off + hd], r, br, BF16, "gru_zr")
                _nan_outside(out3, o3off, o3off + hd, tag0 + " r")
            else:
                assert bool(torch.isnan(out3).all())
        # --- EPI_GRU_Q (Cout = hd), with and without out2
        zg = e["z"][..., :hd]
        zbuf = _window(zg, a2off, wd(hd), cuda)
        (hn, bhn), (q, bq) = C.epi_gru_q(pre[..., :hd], pb[..., :hd], h, zg)
        for with2 in (True, False):
            out, out2 = nanbuf(hd), nanbuf(hd)
            run(hd, C.EPI_GRU_Q, out, bias=bias, out2=out2 if with2 else None, o2off=o2off, aux1=hbuf, a1off=a1off,
                aux2=zbuf, a2off=a2off)
            _check(f"{tag0} gru_q h'", out[..., ooff:ooff + hd], hn, bhn, BF16, "gru_q")
            _nan_outside(out, ooff, ooff + hd, tag0 + " h'")
            if with2:
                _check(f"{tag0} gru_q q~", out2[..., o2off:o2off + hd], q, bq, BF16, "gru_q")
                _nan_outside(out2, o2off, o2off + hd, tag0 + " q~")
            else:
                assert bool(torch.isnan(out2).all())
        # --- EPI_RELU_BWD (no bias)
        av = e["actv"][..., :n]
        want, b = C.epi_relu_bwd(pre0[..., :n], pb0[..., :n], av)
        out = nanbuf(n)
        run(n, C.EPI_RELU_BWD, out, aux1=_window(av, a1off, wd(n), cuda), a1off=a1off)
        _check(f"{tag0} relu_bwd", out[..., ooff:ooff + n], want, b, BF16, "relu_bwd")
        _nan_outside(out, ooff, ooff + n, tag0 + " relu_bwd")
        masked = (av.double() <= 0)
        assert bool((out[..., ooff:ooff + n].cpu()[masked] == 0).all()), tag0 + ": masked outputs must be exactly 0"
        # --- EPI_ACC_F32: known random prefill, exact outside the window
        o0 = _prefill(shape, wd(n), cuda, 1)
        out = o0.clone()
        run(n, C.EPI_ACC_F32, out)
        want, b = C.epi_acc_f32(pre0[..., :n], pb0[..., :n], o0[..., ooff:ooff + n].cpu())
        _check(f"{tag0} acc_f32", out[..., ooff:ooff + n], want, b, F32, "acc_f32")
        _same_outside(out, o0, ooff, ooff + n, tag0 + " acc_f32")
        # --- EPI_GRU_QBWD (hd <= Cout; channels >= hd accumulate v)
        nq = 96 if vec else 94
        oq0 = _prefill(shape, wd(nq), cuda, 2)
        out = oq0.clone()
        out2 = nanbuf(hd)
        run(nq, C.EPI_GRU_QBWD, out, hd=hd, out2=out2, o2off=o2off, aux1=hbuf, a1off=a1off, aux2=zbuf, a2off=a2off)
        (wo, bo), (dr, bd) = C.epi_gru_qbwd(pre0[..., :nq], pb0[..., :nq], h, zg, oq0[..., ooff:ooff + nq].cpu(), hd)
        _check(f"{tag0} gru_qbwd out", out[..., ooff:ooff + nq], wo, bo, F32, "gru_qbwd out")
        _check(f"{tag0} gru_qbwd dr_pre", out2[..., o2off:o2off + hd], dr, bd, BF16, "gru_qbwd dr_pre")
        _same_outside(out, oq0, ooff, ooff + nq, tag0 + " gru_qbwd")
        _nan_outside(out2, o2off, o2off + hd, tag0 + " dr_pre")


@pytest.mark.parametrize("tile", [None, 5, 3])
def test_flow_epilogue(cuda, tile):
    """EPI_FLOW (coords fp32 NCHW += the two flow channels) on its default tile (the small-N
    kernel, by choose_tile), on tile 5 by name and on a register-staged tile, with out2 as
    the source and in place."""
    kh, kw = 3, 3
    for shape in C.EPI_SHAPES:
        e = C.epi_case(*shape, kh, kw)
        key = ("flow", shape)
        w2, b2 = e["w"][16:18], e["bias"][16:18].to(cuda)  # two rows with real weights
        segs, wpf = _segs(key, e["x"], "64x2", cuda), _packed(key, w2, "64x2", cuda)
        t = 5 if tile is None else tile
        pb = C.acc_bound(C.fwd_chain(t, 9, C.KTOT, True), e["A"][..., 16:18])
        want, b = C.epi_flow(e["pre"][..., 16:18], pb, e["src"])
        src = e["src"].to(cuda)
        crd = torch.full_like(src, NAN)
        _conv(segs, wpf, b2, kh, kw, 2, C.EPI_FLOW, crd, 0, tile, out2=src)
        _check(f"flow tile {tile} {shape} out2", crd, want, b, F32, "flow")
        assert torch.equal(src.cpu(), e["src"])
        crd = src.clone()
        _conv(segs, wpf, b2, kh, kw, 2, C.EPI_FLOW, crd, 0, tile)
        _check(f"flow tile {tile} {shape} in place", crd, want, b, F32, "flow")


# ------------------------------------------------------------------ weight gradients
def _wg_dev(stack, kh, kw, dev):
    k = ("wg", stack, kh, kw)
    if k not in _DEV:
        c = C.wgrad_case(*stack, kh, kw)
        x0 = _window(c["x0"], 8, C.WG_SEG + 16, dev)
        segs = [x0, c["xb"].to(dev), c["x2"].to(dev)]
        dys = {co: C.dy_buffer(c["dy"], co).to(dev) for co in C.WG_COUTS}
        _DEV[k] = (segs, dys)
    return _DEV[k]


def _wg_args(stack, segs):
    it, B, H, W = stack
    return segs, [8, 0, 0], [C.WG_SEG] * 3, [it * B * H * W, B * H * W, it * B * H * W]


def _wg_check(tag, op, call, c, cout, taps, chain, bchain, with_db, cuda, twice):
    dw0 = torch.randn(cout + 3, taps, C.WG_KTOT, device=cuda)
    db0 = torch.randn(cout + 3, device=cuda)
    dw, db = dw0.clone(), db0.clone()
    call(dw, db if with_db else None)
    want = dw0[:cout].cpu().double() + C.kernel_layout(c["dw"][:cout])
    S = dw0[:cout].cpu().double().abs() + C.kernel_layout(c["S"][:cout])
    _check(f"{tag} dw", dw[:cout], want, C.acc_bound(chain, S), F32, op + " dw")
    assert torch.equal(dw[cout:], dw0[cout:]), tag + ": dw rows >= Cout changed"
    if with_db:
        wb = db0[:cout].cpu().double() + c["db"][:cout]
        Sb = db0[:cout].cpu().double().abs() + c["Sb"][:cout]
        _check(f"{tag} db", db[:cout], wb, C.acc_bound(bchain, Sb), F32, op + " db")
        assert torch.equal(db[cout:], db0[cout:]), tag + ": db past Cout changed"
    else:
        assert torch.equal(db, db0)
    if twice:  # deterministic: bit-equal from the same start
        dw2, db2 = dw0.clone(), db0.clone()
        call(dw2, db2 if with_db else None)
        assert torch.equal(dw2, dw) and torch.equal(db2, db), tag + ": two calls differ"


@pytest.mark.parametrize("det", [False, True], ids=["atomic", "deterministic"])
@pytest.mark.parametrize("var", range(6))
def test_conv_wgrad(cuda, var, det):
    R = torch.ops.raft_stir
    was = R.is_deterministic()
    R.set_deterministic(det)
    try:
        for stack in C.WG_STACKS:
            it, B, H, W = stack
            P = it * B * H * W
            for ki, (kh, kw) in enumerate(C.KERNELS):
                c = C.wgrad_case(*stack, kh, kw)
                segs, dys = _wg_dev(stack, kh, kw, cuda)
                sg, offs, chans, per = _wg_args(stack, segs)
                for ci, cout in enumerate(C.WG_COUTS):
                    chain = C.wgrad_chain(P, kh * kw, C.WG_KTOT, cout, det, var)
                    bchain = C.wgrad_bias_chain(P, kh * kw, C.WG_KTOT, cout, det, var)

                    def call(dw, db, cout=cout):
                        R.conv_wgrad(dys[cout], C.WG_YOFF, cout, sg, offs, chans, per, kh, kw, dw, db, var)

                    for with_db in ((True, False) if ci == ki else (True,)):
                        tag = f"conv_wgrad var {var} det {det} {kh}x{kw} {stack} cout {cout} db {with_db}"
                        _wg_check(tag, "conv_wgrad", call, c, cout, kh * kw, chain, bchain, with_db, cuda, det)
    finally:
        R.set_deterministic(was)


@pytest.mark.parametrize("bm", [64, 128])
def test_wgrad_v3(cuda, bm):
    R = torch.ops.raft_stir
    for stack in C.WG_STACKS:
        it, B, H, W = stack
        for ki, (kh, kw) in enumerate(C.K3):
            c = C.wgrad_case(*stack, kh, kw)
            segs, dys = _wg_dev(stack, kh, kw, cuda)
            sg, offs, chans, per = _wg_args(stack, segs)
            for ci, cout in enumerate(C.WG_COUTS):
                chain = C.wgrad3_chain(it * B, H, W, cout, C.WG_KTOT, bm)
                bchain = C.wgrad3_bias_chain(it * B, H, W, cout, C.WG_KTOT, bm)

                def call(dw, db, cout=cout):
                    R.wgrad_v3(dys[cout], C.WG_YOFF, cout, sg, offs, chans, per, kh, kw, dw, db, bm)

                for with_db in ((True, False) if ci == ki else (True,)):
                    tag = f"wgrad_v3 bm {bm} {kh}x{kw} {stack} cout {cout} db {with_db}"
                    _wg_check(tag, "wgrad_v3", call, c, cout, kh * kw, chain, bchain, with_db, cuda, True)


@pytest.mark.parametrize("det", [False, True], ids=["atomic", "deterministic"])
def test_colsum(cuda, det):
    R = torch.ops.raft_stir
    was = R.is_deterministic()
    R.set_deterministic(det)
    try:
        for stack in C.WG_STACKS:
            it, B, H, W = stack
            c = C.wgrad_case(*stack, 1, 1)
            _, dys = _wg_dev(stack, 1, 1, cuda)
            for cout in C.WG_COUTS:
                db0 = torch.randn(cout + 3, device=cuda)
                db = db0.clone()
                R.colsum(dys[cout], C.WG_YOFF, cout, db)
                want = db0[:cout].cpu().double() + c["db"][:cout]
                Sb = db0[:cout].cpu().double().abs() + c["Sb"][:cout]
                tag = f"colsum det {det} {stack} C {cout}"
                _check(tag, db[:cout], want, C.acc_bound(C.colsum_chain(it * B * H * W), Sb), F32, "colsum")
                assert torch.equal(db[cout:], db0[cout:]), tag
                if det:
                    db2 = db0.clone()
                    R.colsum(dys[cout], C.WG_YOFF, cout, db2)
                    assert torch.equal(db2, db), tag + ": two calls differ"
    finally:
        R.set_deterministic(was)


# ------------------------------------------------------------------ element-wise backward ops
@pytest.mark.parametrize("dtype", [BF16, F32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("hd", C.GATE_BWD_HD)
def test_gru_gate_bwd(cuda, hd, dtype):
    hoff = 16
    for shape in C.GATE_BWD_P:
        dh, z, q, h = C.gate_bwd_case(shape, hd, dtype)
        (dq, bq), (dz, bz), (dhn, bh) = C.gru_gate_bwd_oracle(dh, z, q, h)
        dhb0 = _window(dh, 0, hd + 12, cuda, fill=0.0)
        dhb0[..., hd:] = torch.randn(*shape, 12, device=cuda)
        dhb = dhb0.clone()
        qb = _window(q, 0, hd + 8, cuda)
        hb = _window(h, hoff, hoff + hd + 8, cuda)
        dqb = torch.full((*shape, hd + 4), NAN, device=cuda, dtype=dtype)
        dzr = torch.full((*shape, 2 * hd), NAN, device=cuda, dtype=dtype)
        torch.ops.raft_stir.gru_gate_bwd(dhb, z.to(cuda), qb, hb, hoff, dqb, dzr)
        tag = f"gru_gate_bwd {shape} hd {hd} {dtype}"
        op = "gru_gate_bwd " + ("bf16" if dtype == BF16 else "fp32")
        _check(tag + " dq", dqb[..., :hd], dq, bq, dtype, op)
        _check(tag + " dz", dzr[..., :hd], dz, bz, dtype, op)
        _check(tag + " dh", dhb[..., :hd], dhn, bh, F32, op + " dh")
        _nan_outside(dqb, 0, hd, tag + " dq")
        _nan_outside(dzr, 0, hd, tag + " dzr")
        _same_outside(dhb, dhb0, 0, hd, tag + " dh")
        # z = 1 stops dh exactly, q~ = +-1 stops dq exactly
        assert bool((dhb[..., 1] == 0).all()) and bool((dqb[..., 0].float() == 0).all())


@pytest.mark.parametrize("dtype", [BF16, F32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("gw,n,ow", C.RELU_TAKE_SHAPES)
def test_relu_take(cuda, gw, n, ow, dtype):
    goff, aoff = 32, 8
    G, actv = C.relu_take_case(gw, n, dtype)
    adev = actv.to(cuda)
    for nz in (0, n, ow):
        want, Gn = C.relu_take_oracle(G, goff, n, nz, actv, aoff, ow)
        Gd = G.to(cuda)
        out = torch.full((*C.RELU_TAKE_P, ow), NAN, device=cuda, dtype=dtype)
        torch.ops.raft_stir.relu_take(Gd, goff, n, nz, adev, aoff, out)
        tag = f"relu_take {gw, n, ow} nz {nz} {dtype}"
        _check(tag, out, want, torch.zeros_like(want), dtype, "relu_take")
        assert bool((out[..., n:] == 0).all()), tag + ": channels >= n must be exactly 0"
        assert torch.equal(Gd.cpu(), Gn), tag + ": G"  # zero inside [goff, goff + nz), untouched outside
        zero = (actv[..., aoff:aoff + n].double() == 0)
        assert bool((out[..., :n].cpu()[zero] == 0).all()), tag + ": -0.0 / 0.0 are not positive"
    # the kernel walks out's channels: it cannot zero more of G than out is wide
    Gd = G.to(cuda)
    out = torch.full((*C.RELU_TAKE_P, ow), NAN, device=cuda, dtype=dtype)
    assert goff + ow + 8 <= gw
    with pytest.raises(RuntimeError, match="nz"):
        torch.ops.raft_stir.relu_take(Gd, goff, n, ow + 8, adev, aoff, out)
    assert torch.equal(Gd.cpu(), G) and bool(torch.isnan(out).all())


# ------------------------------------------------------------------ host rejections (no launch)
def test_host_rejections(cuda):
    from raft_stir_amd.ops.conv import conv_fused, frag_weight, pack_weight
    shape = (1, 5, 7)
    x = torch.randn(*shape, C.KTOT).to(BF16)
    out = torch.full((*shape, 104), NAN, device=cuda, dtype=BF16)

    def setup(kh, kw, layout):
        w = torch.randn(96, C.KTOT, kh, kw, device=cuda)
        wp = pack_weight(w, C.pack_spec(layout), C.COUT_PAD)
        return [(b.to(cuda), o, c) for b, o, c in C.seg_buffers(x, layout)], wp

    segs, wp = setup(3, 3, "64x2")
    with pytest.raises(RuntimeError, match="tile 70"):  # the 1x1 GEMM with a 3x3
        conv_fused(segs, wp, None, 3, 3, 96, C.EPI_BIAS, out, 0, tile=70)
    with pytest.raises(RuntimeError, match="Cout <= 16"):  # the small-N tile with Cout 32
        conv_fused(segs, wp, None, 3, 3, 32, C.EPI_BIAS, out, 0, tile=5)
    segs32, wp32 = setup(3, 3, "32x3")
    with pytest.raises(RuntimeError, match="% 64"):  # a weight-streaming tile without % 64 segments
        conv_fused(segs32, wp32, None, 3, 3, 96, C.EPI_BIAS, out, 0, tile=61, wf=frag_weight(wp32))
    assert bool(torch.isnan(out).all())
    R = torch.ops.raft_stir
    dy = torch.randn(3, 5, 7, 72, device=cuda).to(BF16)
    seg = torch.randn(3, 5, 7, 64, device=cuda).to(BF16)
    dw = torch.zeros(64, 1, 64, device=cuda)
    with pytest.raises(RuntimeError, match="3x3, 1x5 and 5x1"):  # wgrad_v3 has no 1x1
        R.wgrad_v3(dy, 8, 64, [seg], [0], [64], [3 * 35], 1, 1, dw, None, 64)
    with pytest.raises(RuntimeError, match="divide"):  # 2 segment images under 3 dY images
        R.conv_wgrad(dy, 8, 64, [seg[:2].contiguous()], [0], [64], [2 * 35], 1, 1, dw, None, 0)
    assert bool((dw == 0).all())


def test_zz_report(cuda):
    """Prints the largest err / bound per check group of this run (run the file with -s)."""
    print(f"{COUNT[0]} checks")
    for op in sorted(WORST):
        print(f"  worst {op}: {WORST[op]:.3f}")

"""csrc/gru.hip, every kernel on its own, vs the fp64 formulas of ops/reference.py.

gru_gate_zr, gru_gate_q, gru_bwd_q, gru_bwd_r, gru_bwd_fin, context_act and
context_act_backward; fp32 and bf16 states (and the fp32 state with a bf16
upstream gradient of gru_bwd_q); P = 2 * 5 * 7 pixels, (hd, cin) = (128, 256)
and (96, 146).  Pre-activations are 3 randn with columns planted at 0, +-1e-3,
+-20, +-88, +-100 and +-1e4 (exp overflow / underflow, saturation), h in
(-1, 1).  The oracle (tests/test_edge_oracles_cpu.py ties it to autograd) is
evaluated in fp64 on the same values after rounding to the storage dtype.

Bounds.  Forward, fp32: |err| <= 2^-20 (1 + |pre|) for z, r, q~, r h and h'.
sigmoid is v_rcp(1 + v_exp(-pre * log2 e)): v_exp and v_rcp are good to one
ulp (2^-23 relative each) and the rounded product pre * log2 e moves the
exponential by 2^-24 |pre| relative; sigmoid' <= 1/4 and |tanh'| <= 1 turn
that into at most (2 + |pre|) 2^-23 absolute, plus half an ulp of the result:
about a quarter of the bound.  Backward, fp32 (products of unit-scale
inputs): atol = rtol = 2^-20.  bf16 storage: + 2^-8 |want|.

Measured on an MI355X (largest |err| / bound; every test prints its own):
  fp32 forward   z 0.06  r 0.06  r h 0.06  q~ 0.12  h' 0.14  tanh(net) 0.13
                 (largest |err| 2.2e-7: under a quarter of the bound, as derived)
  fp32 backward  dq_pre 0.09  dz_pre 0.07  dh_direct 0.06  dr_pre 0.04  dh 0.11  dx 0.05  dcnet 0.06
  bf16           0.95 - 1.00 everywhere: a bf16 rounding is up to 2^-8 |want|, the bound is tight
"""
import math

import pytest
import torch

from raft_stir_amd.ops import reference as ref

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16
SHAPE = (2, 5, 7)
DIMS = [(128, 256), (96, 146)]
PLANT = [0.0, 1e-3, -1e-3, 20.0, -20.0, 88.0, -88.0, 100.0, -100.0, 1e4, -1e4]
E20 = 2.0 ** -20


def _pre(C, dtype, g):
    """3 randn with the PLANT values in channels 0..10 (rounded to `dtype`)."""
    t = 3.0 * torch.randn(*SHAPE, C, generator=g)
    for i, v in enumerate(PLANT):
        t[..., i] = v
    return t.to(dtype)


def _unit(C, dtype, g, kind="randn"):
    t = torch.randn(*SHAPE, C, generator=g)
    if kind == "tanh":
        t = torch.tanh(t)
    elif kind == "sigmoid":
        t = torch.sigmoid(3.0 * t)
    return t.to(dtype)


def _check(name, got, want, bound, dtype):
    assert got.dtype == dtype, name
    if dtype == BF16:
        bound = bound + 2.0 ** -8 * want.abs()
    err = (got.cpu().double() - want).abs()
    assert bool(torch.isfinite(got).all()), name
    ratio = (err / bound).max().item()
    print(f"{name} [{dtype}]: max|err| {err.max().item():.3e}  err/bound {ratio:.3f}")
    assert ratio <= 1.0, f"{name}: err/bound {ratio:.3f}"


def _fwd_bound(pre):
    return E20 * (1.0 + pre.double().abs())


def _bwd_bound(want):
    return E20 + E20 * want.abs()


def _d(*ts):
    return [t.double() for t in ts]


@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("hd,cin", DIMS)
def test_gate_zr(cuda, hd, cin, dtype):
    g = torch.Generator().manual_seed(0)
    zr = torch.cat([_pre(hd, dtype, g), _pre(hd, dtype, g)], -1)
    h, x = _unit(hd, dtype, g, "tanh"), _unit(cin, dtype, g)
    z, r, rhx = torch.ops.raft_stir.gru_gate_zr(zr.to(cuda), h.to(cuda), x.to(cuda))
    wz, wr, wrhx = ref.gru_gate_zr(*_d(zr, h, x))
    _check("z", z, wz, _fwd_bound(zr[..., :hd]), dtype)
    _check("r", r, wr, _fwd_bound(zr[..., hd:]), dtype)
    _check("r*h", rhx[..., :hd], wrhx[..., :hd], _fwd_bound(zr[..., hd:]), dtype)
    assert rhx.shape == (*SHAPE, hd + cin)
    assert torch.equal(rhx[..., hd:].cpu(), x)  # the pass-through half: a copy, bit for bit


@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("hd,cin", DIMS)
def test_gate_q(cuda, hd, cin, dtype):
    g = torch.Generator().manual_seed(1)
    q, z, h = _pre(hd, dtype, g), _unit(hd, dtype, g, "sigmoid"), _unit(hd, dtype, g, "tanh")
    z[..., :3] = torch.tensor([0.0, 1.0, 0.5], dtype=dtype)  # closed / open / half-open gate
    hn, qt = torch.ops.raft_stir.gru_gate_q(q.to(cuda), z.to(cuda), h.to(cuda))
    whn, wqt = ref.gru_gate_q(*_d(q, z, h))
    _check("q~", qt, wqt, _fwd_bound(q), dtype)
    _check("h'", hn, whn, _fwd_bound(q), dtype)


@pytest.mark.parametrize("dtype,gdtype", [(F32, F32), (BF16, BF16), (F32, BF16), (BF16, F32)])
@pytest.mark.parametrize("hd,cin", DIMS)
def test_bwd_q(cuda, hd, cin, dtype, gdtype):
    g = torch.Generator().manual_seed(2)
    dhn = _unit(hd, gdtype, g)
    z, h, qt = _unit(hd, dtype, g, "sigmoid"), _unit(hd, dtype, g, "tanh"), _unit(hd, dtype, g, "tanh")
    dq, dzr, dh = torch.ops.raft_stir.gru_bwd_q(dhn.to(cuda), z.to(cuda), h.to(cuda), qt.to(cuda))
    wdq, wdz, wdh = ref.gru_bwd_q(*_d(dhn, z, h, qt))
    assert dzr.shape == (*SHAPE, 2 * hd)
    _check("dq_pre", dq, wdq, _bwd_bound(wdq), dtype)
    _check("dz_pre", dzr[..., :hd], wdz, _bwd_bound(wdz), dtype)
    _check("dh_direct", dh, wdh, _bwd_bound(wdh), F32)  # fp32 whatever the state's dtype


@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("hd,cin", DIMS)
def test_bwd_r(cuda, hd, cin, dtype):
    g = torch.Generator().manual_seed(3)
    drhx, h, r = _unit(hd + cin, dtype, g), _unit(hd, dtype, g, "tanh"), _unit(hd, dtype, g, "sigmoid")
    dzr0 = _unit(2 * hd, dtype, g)
    dzr = dzr0.to(cuda)
    torch.ops.raft_stir.gru_bwd_r(drhx.to(cuda), h.to(cuda), r.to(cuda), dzr)
    want = ref.gru_bwd_r(*_d(drhx, h, r))
    _check("dr_pre", dzr[..., hd:], want, _bwd_bound(want), dtype)
    assert torch.equal(dzr[..., :hd].cpu(), dzr0[..., :hd])  # the dz_pre half belongs to gru_bwd_q


@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("hd,cin", DIMS)
def test_bwd_fin(cuda, hd, cin, dtype):
    g = torch.Generator().manual_seed(4)
    dhd = _unit(hd, F32, g)
    drhx, r, dhx = _unit(hd + cin, dtype, g), _unit(hd, dtype, g, "sigmoid"), _unit(hd + cin, dtype, g)
    dh, dx = torch.ops.raft_stir.gru_bwd_fin(dhd.to(cuda), drhx.to(cuda), r.to(cuda), dhx.to(cuda))
    wdh, wdx = ref.gru_bwd_fin(*_d(dhd, drhx, r, dhx))
    assert dx.shape == (*SHAPE, cin)
    _check("dh", dh, wdh, _bwd_bound(wdh), dtype)
    _check("dx", dx, wdx, _bwd_bound(wdx), dtype)


@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("hd,cd", [(128, 128), (96, 64)])
def test_context_act_pitched_windows(cuda, hd, cd, dtype):
    """tanh | relu written into the first hd channels of a wider hx buffer and
    into a channel window of a wider inp buffer: nothing else may change."""
    g = torch.Generator().manual_seed(5)
    cn = _pre(hd + cd, dtype, g)
    for i, v in enumerate(PLANT):  # the relu half sees the planted values too
        cn[..., hd + i] = v
    hxw, off, ipw = hd + cd + 40, 8, cd + 24
    hx = torch.full((*SHAPE, hxw), math.nan, device=cuda, dtype=dtype)
    ibuf = torch.full((*SHAPE, ipw), math.nan, device=cuda, dtype=dtype)
    torch.ops.raft_stir.context_act(cn.to(cuda), hx, ibuf[..., off:off + cd], hd)
    wnet, winp = ref.context_act(cn.double(), hd)
    _check("tanh(net)", hx[..., :hd], wnet, _fwd_bound(cn[..., :hd]), dtype)
    assert bool((ibuf[..., off:off + cd].cpu().double() == winp).all())  # relu: exact
    assert bool(torch.isnan(hx[..., hd:]).all())
    assert bool(torch.isnan(ibuf[..., :off]).all()) and bool(torch.isnan(ibuf[..., off + cd:]).all())


@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("hd,cd", [(128, 128), (96, 64)])
def test_context_act_backward_pitched_gradient(cuda, hd, cd, dtype):
    g = torch.Generator().manual_seed(6)
    G = torch.randn(*SHAPE, hd + cd + 24, generator=g)
    G[..., hd + cd:] = math.nan  # columns past hd + cd are not this op's
    hx = _unit(hd + 16, dtype, g, "tanh")
    inp = torch.relu(_unit(cd, dtype, g))
    dcn = torch.ops.raft_stir.context_act_backward(G.to(cuda), hx.to(cuda), inp.to(cuda), hd)
    want = ref.context_act_backward(*_d(G, hx, inp), hd)
    assert dcn.shape == (*SHAPE, hd + cd)
    _check("dcnet", dcn, want, _bwd_bound(want), dtype)


# ------------------------------------------------------------------ host checks
def _op_args(name, dtype, dev):
    hd, cin = 32, 48
    g = torch.Generator().manual_seed(7)
    t = lambda C, dt=dtype: _unit(C, dt, g).to(dev)
    R = torch.ops.raft_stir
    return {
        "gru_gate_zr": (R.gru_gate_zr, [t(2 * hd), t(hd), t(cin)], ()),
        "gru_gate_q": (R.gru_gate_q, [t(hd), t(hd), t(hd)], ()),
        "gru_bwd_q": (R.gru_bwd_q, [t(hd), t(hd), t(hd), t(hd)], ()),
        "gru_bwd_r": (R.gru_bwd_r, [t(hd + cin), t(hd), t(hd), t(2 * hd)], ()),
        "gru_bwd_fin": (R.gru_bwd_fin, [t(hd, F32), t(hd + cin), t(hd), t(hd + cin)], ()),
        "context_act_backward": (R.context_act_backward, [t(hd + cin + 8, F32), t(hd + 8), t(cin)], (hd,)),
    }[name]


OPS = ["gru_gate_zr", "gru_gate_q", "gru_bwd_q", "gru_bwd_r", "gru_bwd_fin", "context_act_backward"]


@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("name", OPS)
def test_host_checks_reject_views_and_float64(cuda, name, dtype):
    """Every tensor argument in turn as a sliced (non-contiguous) view of the
    same shape and values, and as float64: the kernels index dense rows of the
    state's dtype, so both must raise instead of reading other memory."""
    op, args, extra = _op_args(name, dtype, cuda)
    op(*args, *extra)  # the well-formed call passes
    for i, a in enumerate(args):
        wide = torch.zeros(*a.shape[:-1], a.shape[-1] + 8, device=cuda, dtype=a.dtype)
        wide[..., :a.shape[-1]] = a
        view = wide[..., :a.shape[-1]]
        assert not view.is_contiguous() and torch.equal(view, a)
        with pytest.raises(RuntimeError, match="contiguous"):
            op(*args[:i], view, *args[i + 1:], *extra)
        with pytest.raises(RuntimeError, match="dtype"):
            op(*args[:i], a.double(), *args[i + 1:], *extra)


@pytest.mark.parametrize("name", OPS)
def test_host_checks_reject_mixed_state_dtypes(cuda, name):
    """One state operand in the other storage dtype (the upstream gradient of
    gru_bwd_q may differ from the state; dhd and G are fp32 by contract)."""
    op, args, extra = _op_args(name, F32, cuda)
    free = {"gru_bwd_q": [0], "gru_bwd_fin": [0], "context_act_backward": [0]}.get(name, [])
    for i, a in enumerate(args):
        if i in free:
            continue
        with pytest.raises(RuntimeError, match="dtype"):
            op(*args[:i], a.bfloat16(), *args[i + 1:], *extra)
    if name == "gru_bwd_q":
        op(args[0].bfloat16(), *args[1:])  # fp32 state, bf16 upstream gradient: allowed
    else:
        for i in free:
            with pytest.raises(RuntimeError, match="dtype"):
                op(*args[:i], args[i].bfloat16(), *args[i + 1:], *extra)

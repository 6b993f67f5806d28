"""The kernels that produce and consume the flow, each on its own, vs fp64 oracles.

csrc/flow_enc.hip, csrc/flowhead.hip, flow_wgrad_kernel of csrc/conv_wgrad.hip,
csrc/convex_upsample.hip (convex upsampler and the upflow8 adjoint) and
csrc/loss.hip, at the smallest shapes that reach every path of each kernel and
with edge values planted.  The oracles (tests/flow_path_cases.py: F.conv2d /
F.unfold + softmax / closed forms in float64 on the CPU;
tests/test_edge_oracles_cpu.py ties them to ops/reference.py, to autograd and to
the composite loss) are evaluated on the values the kernels read, after rounding
to the storage dtype.  Every check prints max|err| and err / bound and asserts
ratio <= 1 and finiteness.  bf16 storage adds 2^-8 |want| to a bound.

Bounds.

flow_encode, fp32 output: |err| <= 2^-16 A + 2^-24 |pre|, A = conv7x7(|flow|, |w|),
  pre = conv + bias before the ReLU (which is 1-Lipschitz).  With x = hi + lo + d,
  |lo| <= 2^-9 |x|, |d| <= 2^-18 |x| per operand, the kernel's
  Whi Fhi + Whi Flo + Wlo Fhi misses Wlo Flo and the d terms: at most 3 * 2^-18 A;
  the other 2^-18 A covers the fp32 accumulation over 98 terms.  The 2^-24 |pre|
  term is not in the issue's bound: the kernel rounds acc + bias once more in
  fp32, which shows where A is tiny next to the bias (a flow of 0.001 px).
  tests/test_edge_oracles_cpu.py shows that a hi-only product exceeds this bound
  > 50x.  fout: fp32 form bit-equal to coords - grid in fp32, bf16 form equal to
  bf16(bf16hi + bf16lo).
flow_head: |err| <= 2^-18 conv3x3(|x|, |w|) + 2^-22 (|src| + |bias| + |want|): the
  longest chain is 9 taps x CPL fmas + a 6-step butterfly, under 64 roundings of
  2^-24; inputs are exact in fp32, so bf16 and fp32 x share the bound.
flow_head_dgrad: |err| <= 2^-19 conv^T(|dflow|, |w|) (18 fmas), masked channels
  (act <= 0, -0.0 included) exactly 0.
flow_wgrad: |err| <= (8 W + nblocks + 4) 2^-24 S, S = |dw0| + sum_p |dF| |flow|
  (|db0| + sum_p |dF| for db): an 8-row in-thread sum, then one add per block.
  |dw0| is added to the issue's S: the op accumulates, and every block's add
  rounds at the magnitude of what is already there.  Deterministic mode: same
  bound, two calls bit-equal.
convex_upsample: |err| <= 2^-19 (1 + sum_k 8 |flow_nbr_k|): a softmax weight is off
  by at most (2 + |arg|) 2^-23 p_k, p_k |arg| <= 1/e, so under 2^-21 per tap.
convex_upsample_backward, from dm_k = p_k (dp_k - sum_j p_j dp_j):
  dmask 2^-18 (1 + sum_k |dp_k|), dflow 2^-18 * 8 sum |p g|.
upflow8_backward: |err| <= (band + 4) 2^-23 (8 |ah|^T |g| |aw|), band = upflow8_band(W).
seq_loss: loss and EPE rtol 2^-20 vs the fp64 composite of the fp32 inputs (all
  terms non-negative); the 1 / 3 / 5 px rates equal the fp64 counts exactly; the
  gradient is bit-equal to w_i sign(pred - gt) valid / M with w_i and 1 / M formed
  in fp32 in the kernel's order.

Measured on an MI355X (largest err / bound over the cases of each check):
  flow_encode        fp32 0.36 (the exact three-product sum alone reaches 0.38 of the bound on
                     the CPU: the dropped lo * lo term, not the fp32 accumulation)  bf16 0.98
  flow_head          fp32 x 0.06  bf16 x 0.05
  flow_head_dgrad    fp32 0.11  bf16 0.99 (the 2^-8 |want| rounding: tight, as in test_gates_gpu.py)
  flow_wgrad         dw 0.14  db 0.08 (atomic and deterministic alike; 0.0002 at W = 579)
  convex_upsample    forward 0.10  dflow 0.02  dmask fp32 0.06, bf16 mask 0.98
  upflow8_backward   0.02 (0.013 at W = 496, the widest row the LDS check admits)
  seq_loss           loss 0.08  EPE 0.09 of rtol 2^-20; rates exact; gradient bit-equal
No kernel missed its bound: W = 1, the -inf logits and the half-empty Cout = 96 block included.
"""
import functools
import math

import pytest
import torch

import flow_path_cases as fc
from flow_path_cases import BF16, F32

pytestmark = pytest.mark.gpu

NAN = math.nan


def _check(name, got, want, bound, dtype=None):
    """max|err| and err / bound (0 / 0 counts as 0: an exact result under a zero bound)."""
    if dtype is not None:
        assert got.dtype == dtype, name
    if got.dtype == BF16:
        bound = bound + 2.0 ** -8 * want.abs()
    got = got.detach().cpu().double()
    assert got.shape == want.shape, (name, got.shape, want.shape)
    assert bool(torch.isfinite(got).all()), name
    err = (got - want).abs()
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bound).max().item() if err.numel() else 0.0
    print(f"{name}: max|err| {err.max().item():.3e}  err/bound {ratio:.3f}")
    assert ratio <= 1.0, f"{name}: err/bound {ratio:.3f}"
    return ratio


# ------------------------------------------------------------------ flow encoder
@functools.lru_cache(maxsize=None)
def _fe_case(B, H, W, Cout):
    coords, flow, w, bias = fc.fe_inputs(B, H, W, Cout, seed=B * 1000 + H * 31 + W + Cout)
    pre, A = fc.fe_oracle(flow, w, bias)
    return coords, flow, w, bias, pre, A


FE_SHAPES = [(1, 1, 1), (2, 8, 8), (1, 9, 17), (2, 13, 21)]


@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("B,H,W,Cout", [(*s, c) for s in FE_SHAPES for c in (64, 128)] + [(1, 9, 17, 96)])
def test_flow_encode(cuda, B, H, W, Cout, dtype):
    coords, flow, w, bias, pre, A = _fe_case(B, H, W, Cout)
    want, bound = pre.clamp_min(0.0), fc.fe_bound(pre, A)
    args = (coords.to(cuda), w.to(cuda), bias.to(cuda))
    for ooff in (0, 8):
        for with_fout in (True, False):
            Cw = ooff + Cout + 16
            foff = ooff + Cout + 5  # odd, as 254 / 240 in models/fused_train.py
            buf = torch.full((B, H, W, Cw), NAN, device=cuda, dtype=dtype)
            torch.ops.raft_stir.flow_encode(*args, buf, ooff, buf if with_fout else None, foff)
            tag = f"flow_encode {B, H, W} C{Cout} {dtype} ooff {ooff} fout {with_fout}"
            _check(tag, buf[..., ooff:ooff + Cout], want, bound, dtype)
            keep = torch.ones(Cw, dtype=torch.bool)
            keep[ooff:ooff + Cout] = False
            if with_fout:
                keep[foff:foff + 2] = False
                got = buf[..., foff:foff + 2].cpu()
                exp = flow.permute(0, 2, 3, 1) if dtype == F32 else fc.fe_fout_bf16(flow).permute(0, 2, 3, 1)
                assert torch.equal(got, exp), tag  # bit for bit
            assert bool(torch.isnan(buf[..., keep.to(cuda)]).all()), tag  # nothing else written


# ------------------------------------------------------------------ flow head
FH_SHAPES = [(1, 1, 1), (1, 1, 8), (1, 2, 9), (3, 1, 7), (2, 13, 21)]


@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("cin", [128, 256])
@pytest.mark.parametrize("B,H,W", FH_SHAPES)
def test_flow_head(cuda, B, H, W, cin, dtype):
    g = torch.Generator().manual_seed(B * 100 + H * 10 + W + cin)
    vn = 4 if cin == 256 else 2  # the host's alignment rule for xoff and the pitch
    xoff, pitch = vn, cin + 3 * vn
    x = torch.full((B, H, W, pitch), NAN)
    x[..., xoff:xoff + cin] = torch.relu(torch.randn(B, H, W, cin, generator=g))
    x = x.to(dtype)
    w = 0.05 * torch.randn(2, 3, 3, cin, generator=g)
    bias = torch.randn(2, generator=g)
    src = 10.0 * torch.randn(B, 2, H, W, generator=g)
    want, bound = fc.fh_fwd_oracle(x[..., xoff:xoff + cin], w, bias, src)
    crd = torch.full_like(src, NAN).to(cuda)
    torch.ops.raft_stir.flow_head(x.to(cuda), xoff, cin, w.to(cuda), bias.to(cuda), crd, src.to(cuda))
    _check(f"flow_head {B, H, W} cin {cin} {dtype}", crd, want, bound, F32)
    crd2 = src.to(cuda)  # src = None: in place
    torch.ops.raft_stir.flow_head(x.to(cuda), xoff, cin, w.to(cuda), bias.to(cuda), crd2, None)
    assert torch.equal(crd2, crd)


@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("cin", [128, 256])
@pytest.mark.parametrize("B,H,W", FH_SHAPES)
def test_flow_head_dgrad(cuda, B, H, W, cin, dtype):
    g = torch.Generator().manual_seed(B * 100 + H * 10 + W + cin + 1)
    vn = 4 if cin == 256 else 2
    aoff, apitch, ooff, opitch = vn, cin + 2 * vn, 2 * vn, cin + 3 * vn
    act = torch.full((B, H, W, apitch), NAN, dtype=dtype)
    act[..., aoff:aoff + cin] = fc.fh_act(B, H, W, cin, dtype, g)
    w = 0.05 * torch.randn(2, 3, 3, cin, generator=g)
    dflow = torch.randn(B, 2, H, W, generator=g)
    want, bound = fc.fh_dgrad_oracle(dflow, w, act[..., aoff:aoff + cin])
    out = torch.full((B, H, W, opitch), NAN, device=cuda, dtype=dtype)
    torch.ops.raft_stir.flow_head_dgrad(dflow.to(cuda), w.to(cuda), cin, act.to(cuda), aoff, out, ooff)
    got = out[..., ooff:ooff + cin]
    _check(f"flow_head_dgrad {B, H, W} cin {cin} {dtype}", got, want, bound, dtype)
    masked = ~(act[..., aoff:aoff + cin].double() > 0)
    assert bool(masked[..., :2].all()) and not bool(masked[..., 2:4].any())  # +-0.0 closed, tiny and 1e4 open
    assert bool((got.cpu()[masked] == 0).all())
    assert bool(torch.isnan(out[..., :ooff]).all()) and bool(torch.isnan(out[..., ooff + cin:]).all())


# ------------------------------------------------------------------ flow_wgrad
def _flow_wgrad_case(cuda, Bp, H, W, Cout, pad, dtype, det, seed):
    g = torch.Generator().manual_seed(seed)
    flow = 100.0 * torch.randn(Bp, 2, H, W, generator=g)
    coords = fc.grid(Bp, H, W) + flow
    flow = coords - fc.grid(Bp, H, W)
    df = torch.randn(Bp, H, W, Cout + pad, generator=g)
    df[..., Cout:] = NAN  # the pitch's pad is not this op's
    df = df.to(dtype)
    dw0, db0 = torch.randn(49, 2, Cout, generator=g), torch.randn(Cout, generator=g)
    wdw, Sw, wdb, Sb = fc.fw_oracle(flow, df, dw0, db0)
    eps = fc.fw_eps(Bp, H, W)
    res = []
    torch.ops.raft_stir.set_deterministic(det)
    try:
        for _ in range(2 if det else 1):
            dw, db = dw0.to(cuda), db0.to(cuda)
            torch.ops.raft_stir.flow_wgrad(coords.to(cuda), df.to(cuda), dw, db)
            res.append((dw, db))
    finally:
        torch.ops.raft_stir.set_deterministic(False)
    tag = f"{Bp, H, W} C{Cout}+{pad} {dtype} det {det}"
    _check(f"flow_wgrad dw {tag}", res[0][0], wdw, eps * Sw, F32)
    _check(f"flow_wgrad db {tag}", res[0][1], wdb, eps * Sb, F32)
    if det:
        assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])


@pytest.mark.parametrize("det", [False, True], ids=["atomic", "det"])
@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("Bp,H,W", [(1, 1, 1), (1, 3, 5), (2, 8, 7), (1, 9, 14), (3, 10, 13)])
def test_flow_wgrad(cuda, Bp, H, W, dtype, det):
    for Cout in (64, 96, 128):
        for pad in (0, 32):
            _flow_wgrad_case(cuda, Bp, H, W, Cout, pad, dtype, det, seed=Bp * 100 + H * 10 + W + Cout + pad)


def _fw_lds(W):  # flow_wgrad_lds of csrc/conv_wgrad.hip: [2][8 + 6][W + 6] fp32
    return 4 * 2 * 14 * (W + 6)


def test_flow_wgrad_lds_limit(cuda):
    """The widest row whose staging fits 64 KiB of LDS runs within the bound; one
    column more is rejected by the host check (nothing is launched)."""
    W = max(w for w in range(1, 1025) if _fw_lds(w) <= 65536)
    assert _fw_lds(W + 1) > 65536
    _flow_wgrad_case(cuda, 1, 1, W, 64, 0, BF16, False, seed=W)
    coords = fc.grid(1, 1, W + 1).to(cuda)
    df = torch.zeros(1, 1, W + 1, 64, device=cuda, dtype=BF16)
    dw, db = torch.zeros(49, 2, 64, device=cuda), torch.zeros(64, device=cuda)
    with pytest.raises(RuntimeError, match="LDS"):
        torch.ops.raft_stir.flow_wgrad(coords, df, dw, db)
    assert not bool(dw.any()) and not bool(db.any())


# ------------------------------------------------------------------ convex upsample
CU_SHAPES = [(1, 1, 1), (2, 1, 33), (1, 3, 32), (2, 2, 40), (1, 5, 9)]


@functools.lru_cache(maxsize=None)
def _cu_case(N, H, W, mdtype):
    flow, mask = fc.cu_inputs(N, H, W, mdtype, seed=N * 100 + H * 10 + W)
    return flow, mask, fc.cu_fwd_oracle(flow, mask)


@pytest.mark.parametrize("mdtype", [F32, BF16])
@pytest.mark.parametrize("N,H,W", CU_SHAPES)
def test_convex_upsample_forward(cuda, N, H, W, mdtype):
    flow, mask, (want, bound) = _cu_case(N, H, W, mdtype)
    up = torch.ops.raft_stir.convex_upsample(flow.to(cuda), mask.to(cuda))
    _check(f"convex_upsample {N, H, W} mask {mdtype}", up, want, bound, F32)


@pytest.mark.parametrize("gdtype", [F32, BF16])
@pytest.mark.parametrize("mdtype", [F32, BF16])
@pytest.mark.parametrize("N,H,W", CU_SHAPES)
def test_convex_upsample_backward(cuda, N, H, W, mdtype, gdtype):
    flow, mask, _ = _cu_case(N, H, W, mdtype)
    g = torch.Generator().manual_seed(N + H + W)
    gup = torch.randn(N, 2, 8 * H, 8 * W, generator=g).to(gdtype)
    wdf, bdf, wdm, bdm = fc.cu_bwd_oracle(flow, mask, gup)
    tag = f"{N, H, W} mask {mdtype} grad {gdtype}"
    dflow, dmask = torch.ops.raft_stir.convex_upsample_backward(flow.to(cuda), mask.to(cuda), gup.to(cuda))
    _check(f"convex_upsample dflow {tag}", dflow, wdf, bdf, F32)
    _check(f"convex_upsample dmask {tag}", dmask, wdm, bdm, mdtype)
    for pitch in (576, 640):
        buf = torch.full((N, H, W, pitch), NAN, device=cuda, dtype=mdtype)
        df2, dm2 = torch.ops.raft_stir.convex_upsample_backward(flow.to(cuda), mask.to(cuda), gup.to(cuda), buf)
        assert dm2.data_ptr() == buf.data_ptr() and torch.equal(df2, dflow)
        assert torch.equal(buf[..., :576], dmask) and bool(torch.isnan(buf[..., 576:]).all())


def test_convex_upsample_autograd_wrapper(cuda):
    """ops.upsample.convex_upsample (NCHW mask, fp32 upstream gradient) is the same two ops."""
    from raft_stir_amd.ops.upsample import convex_upsample
    N, H, W = 2, 2, 40
    flow, mask, (want, bound) = _cu_case(N, H, W, F32)
    f = flow.to(cuda).requires_grad_()
    m = mask.to(cuda).permute(0, 3, 1, 2).requires_grad_()  # (N,576,H,W), channels-last memory
    up = convex_upsample(f, m)
    _check("convex_upsample (wrapper)", up, want, bound, F32)
    gup = torch.randn(N, 2, 8 * H, 8 * W, generator=torch.Generator().manual_seed(3))
    up.backward(gup.to(cuda))
    wdf, bdf, wdm, bdm = fc.cu_bwd_oracle(flow, mask, gup)
    _check("convex_upsample dflow (wrapper)", f.grad, wdf, bdf, F32)
    _check("convex_upsample dmask (wrapper)", m.grad.permute(0, 2, 3, 1), wdm, bdm, F32)


def test_convex_upsample_backward_host_checks(cuda):
    """float64 / float16 masks, a float64 flow, a transposed flow view, a flow that is
    not (N,2,H,W) and a dmask_out that is not on the GPU raise; nothing is launched."""
    N, H, W = 1, 2, 3
    flow = torch.randn(N, 2, H, W, device=cuda)
    mask = torch.randn(N, H, W, 576, device=cuda)
    gup = torch.randn(N, 2, 8 * H, 8 * W, device=cuda)
    op = torch.ops.raft_stir.convex_upsample_backward
    op(flow, mask, gup)  # the well-formed call passes
    for bad in (mask.double(), mask.half()):
        with pytest.raises(RuntimeError, match="mask has unsupported dtype"):
            op(flow, bad, gup)
    with pytest.raises(RuntimeError, match="flow has unsupported dtype"):
        op(flow.double(), mask, gup)
    view = torch.randn(N, 2, W, H, device=cuda).transpose(2, 3)
    assert view.shape == flow.shape and not view.is_contiguous()
    with pytest.raises(RuntimeError, match="contiguous"):
        op(view, mask, gup)
    with pytest.raises(RuntimeError, match=r"flow must be \(N,2,H,W\)"):
        op(torch.randn(N, 3, H, W, device=cuda), mask, gup)
    with pytest.raises(RuntimeError, match=r"flow must be \(N,2,H,W\)"):
        op(torch.randn(2, H, W, device=cuda), mask, gup)
    with pytest.raises(RuntimeError, match="dmask_out"):
        op(flow, mask, gup, torch.zeros(N, H, W, 576))
    with pytest.raises(RuntimeError, match="dmask_out"):
        op(flow, mask, gup, torch.zeros(N, H, W, 576, device=cuda, dtype=BF16))


# ------------------------------------------------------------------ upflow8 adjoint
UP8_WMAX = fc.up8_largest_w()
UP8_SHAPES = [(1, 2, 3, 62), (3, 2, 3, 62), (1, 2, 2, 128), (1, 2, 1, 129), (1, 1, 1, 256), (1, 1, 1, UP8_WMAX)]


@pytest.mark.parametrize("N,C,H,W", UP8_SHAPES)
def test_upflow8_backward(cuda, N, C, H, W):
    g = torch.randn(N, C, 8 * H, 8 * W, generator=torch.Generator().manual_seed(W))
    ah, aw = fc.interp_matrix(H, 8 * H), fc.interp_matrix(W, 8 * W)
    want, bound = fc.up8_oracle(g, ah, aw)
    got = torch.ops.raft_stir.upflow8_backward(g.to(cuda), ah.to(cuda), aw.to(cuda))
    _check(f"upflow8_backward {N, C, H, W} band {fc.up8_band(W)}", got, want, bound, F32)


def test_upflow8_backward_lds_limit(cuda):
    W = (UP8_WMAX // 4 + 1) * 4  # the next multiple of 4 above the widest accepted row
    assert fc.up8_cols_lds(UP8_WMAX) <= 65536 < fc.up8_cols_lds(W)
    g = torch.zeros(1, 1, 8, 8 * W, device=cuda)
    with pytest.raises(RuntimeError, match="LDS"):
        torch.ops.raft_stir.upflow8_backward(g, fc.interp_matrix(1, 8).to(cuda), fc.interp_matrix(W, 8 * W).to(cuda))


# ------------------------------------------------------------------ sequence loss
def _run_loss(cuda, preds, gt, valid, gamma, gout=3.0):
    from raft_stir_amd.train.loss import _stacked, sequence_loss
    base = preds.to(cuda).requires_grad_()
    views = list(base.unbind(0))
    assert _stacked(views) is not None  # the fused path, not the composite
    loss, m = sequence_loss(views, gt.to(cuda), valid.to(cuda), gamma, sync_metrics=False)
    (loss * gout).backward()
    return loss.detach().cpu().double(), {k: v.cpu() for k, v in m.items()}, base.grad.cpu()


def _check_loss(tag, cuda, preds, gt, valid, gamma, nplant):
    wl, wm, ok, epe = fc.loss_oracle(preds, gt, valid, gamma)
    # precondition on the input, from the oracle alone: off the planted pixels no EPE is
    # within 2^-18 (relative) of a threshold.  Nothing is left out of any comparison.
    assert fc.loss_precondition(epe, ok, nplant), tag
    loss, m, grad = _run_loss(cuda, preds, gt, valid, gamma)
    rt = 2.0 ** -20
    for name, got, want in (("loss", float(loss), float(wl)), ("epe", float(m["epe"]), wm["epe"])):
        err = abs(got - want)
        ratio = err / (rt * abs(want)) if err else 0.0
        print(f"seq_loss {name} {tag}: {got:.9g} vs {want:.9g}  err/bound {ratio:.3f}")
        assert math.isfinite(got) and ratio <= 1.0, (tag, name, got, want)
    for k in (1, 3, 5):
        want = torch.tensor(wm[f"{k}px"] / max(wm["cnt"], 1), dtype=torch.float64).float()
        print(f"seq_loss {k}px {tag}: count {wm[f'{k}px']} of {wm['cnt']}")
        assert float(m[f"{k}px"]) == float(want), (tag, k, float(m[f"{k}px"]), float(want))
    want_grad = fc.loss_grad_mirror(preds, gt, ok, gamma, 3.0)
    assert torch.equal(grad, want_grad), (tag, (grad - want_grad).abs().max())
    print(f"seq_loss grad {tag}: bit-equal")


@pytest.mark.parametrize("gamma", [0.8, 1.0, 0.0])
@pytest.mark.parametrize("N,B,H,W", [(1, 1, 1, 1), (12, 2, 3, 5), (3, 1, 16, 17)])
def test_seq_loss_small(cuda, N, B, H, W, gamma):
    preds, gt, valid, n = fc.loss_inputs(N, B, H, W, seed=N + H + W)
    _check_loss(f"{N, B, H, W} gamma {gamma}", cuda, preds, gt, valid, gamma, n)


@pytest.mark.parametrize("H,W", [(725, 724), (724, 724)], ids=["grid-stride", "control"])
def test_seq_loss_grid_stride(cuda, H, W):
    """Just above 2048 * 256 pixels both grid-stride loops run (and sum_kernel's
    multi-pass loop over the 2048 partials); just below, the control."""
    assert (H * W > 2048 * 256) == (H == 725) and H * W > 2047 * 256
    preds, gt, valid, n = fc.loss_inputs(2, 1, H, W, seed=H)
    _check_loss(f"{2, 1, H, W}", cuda, preds, gt, valid, 0.8, n)


def test_seq_loss_all_invalid(cuda):
    preds, gt, valid, _ = fc.loss_inputs(3, 2, 3, 5, seed=9, all_invalid=True)
    loss, m, grad = _run_loss(cuda, preds, gt, valid, 0.8)
    assert float(loss) == 0.0 and all(float(v) == 0.0 for v in m.values()) and not bool(grad.any())


def test_seq_loss_nan_predictions(cuda):
    """A NaN prediction at a valid pixel makes the loss NaN.  At a masked pixel the fused
    loss never reads it: the loss stays finite and the gradient there is 0, where the
    composite's 0 * NaN gives NaN (train/loss.py says so)."""
    preds, gt, valid, _ = fc.loss_inputs(3, 2, 3, 5, seed=4)
    valid[:] = 1.0
    valid[1, 2, 4] = 0.0
    gt[1, :, 0, 0] = torch.tensor([400.0, 300.0])  # |gt| = 500: masked as well
    masked = preds.clone()
    masked[1, 1, 0, 2, 4] = NAN
    masked[2, 1, :, 0, 0] = NAN
    wl, wm, ok, _ = fc.loss_oracle(torch.nan_to_num(masked), gt, valid, 0.8)
    loss, m, grad = _run_loss(cuda, masked, gt, valid, 0.8)
    assert abs(float(loss) - float(wl)) <= 2.0 ** -20 * float(wl) and abs(float(m["epe"]) - wm["epe"]) <= 2.0 ** -20 * wm["epe"]
    assert bool(torch.isfinite(grad).all()) and not bool(grad[:, 1, :, 2, 4].any()) and not bool(grad[:, 1, :, 0, 0].any())
    assert torch.equal(grad, fc.loss_grad_mirror(torch.nan_to_num(masked), gt, ok, 0.8, 3.0))
    poisoned = preds.clone()
    poisoned[0, 0, 1, 1, 1] = NAN  # valid pixel, first prediction
    loss, _, _ = _run_loss(cuda, poisoned, gt, valid, 0.8)
    assert math.isnan(float(loss))

"""Dense every-pixel tracking on the GPU: the kernel of csrc/dense_flow.hip
against the selection rule composed from ops.fb_track_points and against
ops.multi_flow_track_points at N = H*W, bit for bit; its index safety, host
checks and hipGraph capture; and the graphed DenseMultiFlowTracker against
MultiFlowTracker on all pixel centres, with stubs and with the real model."""
import pytest
import torch

from raft_stir_amd import ops
from raft_stir_amd.config import make_args
from raft_stir_amd.export.denseflow import DenseMultiFlowTracker
from raft_stir_amd.export.multiflow import MultiFlowTracker
from raft_stir_amd.models import RAFT
from raft_stir_amd.ops import reference

import dense_flow_cases as D
import multi_flow_cases as M

pytestmark = pytest.mark.gpu

ALPHA = (0.02, 2.0)
INF = D.INF


def _step(ins, act, alpha=D.FB.ALPHA, cand_err=True):
    """One step on copies of the rings: (the six outputs, ring_pos, ring_score after it)."""
    fw, bw, ring_pos, ring_score, idx = ins
    rp, rs = ring_pos.clone(), ring_score.clone()
    return ops.dense_multi_flow_step(fw, bw, rp, rs, idx, act, *alpha, cand_err=cand_err), rp, rs


# ------------------------------------------------------ kernel vs composed rule
@pytest.mark.parametrize("hw", D.KERNEL_HW, ids=lambda hw: f"{hw[0]}x{hw[1]}")
@pytest.mark.parametrize("K", [1, 3, 16])
def test_kernel_against_composed_rule(cuda, K, hw):
    """Bit equality of every output and of the ring: this kernel, the point
    kernel and fb_points_kernel inline the device functions of
    csrc/fb_device.h under the same flags."""
    H, W = hw
    ins = tuple(t.to(cuda) for t in D.step_inputs(K, H, W))
    fw, bw, ring_pos, ring_score, idx = ins
    dst = int(idx[K])
    for name, act in M.active_masks(K) + D.single_masks(K):
        act = act.to(cuda)
        got, rp, rs = _step(ins, act)
        assert all(t.device.type == "cuda" for t in got)
        assert got[0].shape == (1, 2, H, W) and got[3].dtype == torch.int32 and got[5].shape == (K, H, W)
        # the oracle on the device, its candidates from the existing HIP kernel
        op, os_ = ring_pos.clone(), ring_score.clone()
        want = reference.dense_multi_flow_step(fw, bw, op, os_, idx, act, *D.FB.ALPHA, track=ops.fb_track_points)
        for key, g, w in zip(D.NAMES, got, want):
            assert D.same(g, w), f"K={K} {hw} {name}: {key} differs from the oracle at {int((g != w).sum())} places"
        assert D.same(rp, op) and D.same(rs, os_), name
        # the point kernel at N = H*W, the rows picked by hand
        want, (wp, ws), sscore = D.point_form(fw, bw, ring_pos, ring_score, idx, act, op=ops.multi_flow_track_points)
        for key, g, w in zip(D.NAMES, got, want):
            assert D.same(g, w), f"K={K} {hw} {name}: {key} differs from the point op at {int((g != w).sum())} places"
        assert D.same(rp, wp) and D.same(rs, ws), name
        others = [r for r in range(K + 2) if r != dst]
        assert D.same(rp[others], ring_pos[others]) and D.same(rs[others], ring_score[others]), name
        # again, and without cand_err
        again, rp2, rs2 = _step(ins, act)
        assert all(D.same(a, b) for a, b in zip(again, got)) and D.same(rp2, rp) and D.same(rs2, rs), name
        lean, rp2, rs2 = _step(ins, act, cand_err=False)
        assert lean[5] is None and all(D.same(a, b) for a, b in zip(lean[:5], got[:5])), name
        assert D.same(rp2, rp) and D.same(rs2, rs), name
        if hw == (24, 70) and K > 1 and name in ("mixed", "none"):
            n = D.outcome_counts([t.cpu() for t in got], sscore.cpu(), act.cpu(), fw.cpu(), bw.cpu(), ring_pos.cpu(),
                                 idx.cpu())
            if name == "mixed":
                assert n["score"] >= 5 and n["tie"] >= 5 and n["fallback"] >= 5, n
            else:
                assert n["none"] == H * W, n


# ---------------------------------------------------------------- index safety
def test_indices_are_clamped_and_a_written_source_is_inactive(cuda):
    H, W = 7, 9
    K, R = 3, 5
    fw, bw, ring_pos, ring_score, _ = (t.to(cuda) for t in D.step_inputs(K, H, W))
    act = torch.ones(K, dtype=torch.bool, device=cuda)

    def run(i, a=act, cand_err=True):
        idx = torch.tensor(i, dtype=torch.int32, device=cuda)
        return _step((fw, bw, ring_pos, ring_score, idx), a, cand_err=cand_err)

    for wild, clamped in (([-5, 1, R + 7, 2], [0, 1, R - 1, 2]), ([0, 1, 2, R + 7], [0, 1, 2, R - 1]),
                          ([3, R + 7, -5, -5], [3, R - 1, 0, 0])):
        for cand_err in (True, False):
            got, rp, rs = run(wild, cand_err=cand_err)
            want, wp, ws = run(clamped, cand_err=cand_err)
            assert all(D.same(a, b) for a, b in zip(got[:5], want[:5])) and D.same(rp, wp) and D.same(rs, ws)
            dst = clamped[K]
            others = [r for r in range(R) if r != dst]
            assert D.same(rp[others], ring_pos[others]) and D.same(rs[others], ring_score[others])
            assert D.same(rp[dst], got[0][0]) and D.same(rs[dst], got[1][0, 0])
    # slot 1 reads the row that is written: as if it were inactive
    off = torch.tensor([True, False, True], device=cuda)
    for cand_err in (True, False):
        got, rp, rs = run([0, 3, 2, 3], cand_err=cand_err)
        want, wp, ws = run([0, 3, 2, 3], off, cand_err=cand_err)
        assert all(D.same(a, b) for a, b in zip(got[:5], want[:5])) and D.same(rp, wp) and D.same(rs, ws)
        assert (got[3] != 1).all()
    # every slot does: no slot is active
    got, rp, rs = run([3, 3, 3, 3])
    assert (got[3] == -1).all() and D.same(got[0][0], ring_pos[3]) and (got[1] == INF).all() and not got[2].any()
    assert D.same(rp[3], ring_pos[3]) and (rs[3] == INF).all()


# ---------------------------------------------------------------- host checks
def test_host_checks(cuda):
    op = torch.ops.raft_stir.dense_multi_flow_step
    K, (H, W) = 3, (7, 9)
    fw, bw, ring_pos, ring_score, idx = (t.to(cuda) for t in D.step_inputs(K, H, W))
    act = torch.tensor([True, False, True], device=cuda)
    outs = dict(pos=torch.empty(1, 2, H, W, device=cuda), score=torch.empty(1, 1, H, W, device=cuda),
                vis=torch.empty(1, 1, H, W, dtype=torch.bool, device=cuda),
                choice=torch.empty(1, 1, H, W, dtype=torch.int32, device=cuda),
                err=torch.empty(1, 1, H, W, device=cuda))

    def call(fw=fw, bw=bw, rp=ring_pos, rs=ring_score, idx=idx, act=act, a1=0.01, a2=0.5, cand=None, **kw):
        o = dict(outs, **kw)
        return op(fw, bw, rp.clone() if rp.is_cuda else rp, rs.clone() if rs.is_cuda else rs, idx, act, a1, a2,
                  o["pos"], o["score"], o["vis"], o["choice"], o["err"], cand)

    call()
    call(cand=torch.empty(K, H, W, device=cuda))
    with pytest.raises(RuntimeError, match="fp32 flows"):
        call(fw=fw.to(torch.bfloat16), bw=bw.to(torch.bfloat16))
    with pytest.raises(RuntimeError, match="contiguous flows"):
        call(fw=fw.transpose(2, 3), bw=bw.transpose(2, 3))
    with pytest.raises(RuntimeError, match="same shape"):
        call(bw=bw[..., :-1].contiguous())
    with pytest.raises(RuntimeError, match=r"\(K,2,H,W\)"):
        call(fw=fw[0], bw=bw[0])
    with pytest.raises(RuntimeError, match="H, W >= 2"):
        call(fw=fw[:, :, :1].contiguous(), bw=bw[:, :, :1].contiguous())
    with pytest.raises(RuntimeError, match="at most 16 slots, got K = 17"):
        call(fw=fw.repeat(6, 1, 1, 1)[:17].contiguous(), bw=bw.repeat(6, 1, 1, 1)[:17].contiguous())
    with pytest.raises(RuntimeError, match="no slots"):
        call(fw=fw[:0], bw=bw[:0])
    with pytest.raises(RuntimeError, match="fp32 rings"):
        call(rp=ring_pos.double())
    with pytest.raises(RuntimeError, match="fp32 rings"):
        call(rs=ring_score.double())
    for bad in (ring_pos[:, :, :-1].contiguous(), ring_pos[:, :1].contiguous(), ring_pos[0], ring_pos[..., :-1].contiguous()):
        with pytest.raises(RuntimeError, match=r"ring_pos must be \(R,2,H,W\)"):
            call(rp=bad)
    with pytest.raises(RuntimeError, match="R >= 2 rows expected, got R = 1"):
        call(rp=ring_pos[:1].contiguous(), rs=ring_score[:1].contiguous())
    for bad in (ring_score[:-1].contiguous(), ring_score[:, :-1].contiguous(), ring_score[None]):
        with pytest.raises(RuntimeError, match=r"ring_score must be \(R,H,W\)"):
            call(rs=bad)
    with pytest.raises(RuntimeError, match="contiguous rings"):
        call(rp=ring_pos.flip(1).transpose(2, 3).contiguous().transpose(2, 3))
    with pytest.raises(RuntimeError, match="int32 idx"):
        call(idx=idx.long())
    for bad in (idx[:-1].contiguous(), torch.cat([idx, idx[:1]]), idx[None]):
        with pytest.raises(RuntimeError, match=r"idx must be a contiguous \(K\+1,\)"):
            call(idx=bad)
    with pytest.raises(RuntimeError, match="bool active"):
        call(act=act.float())
    with pytest.raises(RuntimeError, match=r"active must be a contiguous \(K,\)"):
        call(act=act[:2].contiguous())
    for name, t in (("bw", bw), ("rp", ring_pos), ("rs", ring_score), ("idx", idx), ("act", act),
                    ("pos", outs["pos"]), ("choice", outs["choice"])):
        with pytest.raises(RuntimeError, match="same device"):
            call(**{name: t.cpu()})
    with pytest.raises(RuntimeError, match="same device"):
        call(cand=torch.empty(K, H, W))
    for a1, a2 in ((-0.01, 0.5), (0.01, -0.5), (float("nan"), 0.5), (0.01, float("inf"))):
        with pytest.raises(RuntimeError, match="alpha"):
            call(a1=a1, a2=a2)
    for name, bad in (("pos", outs["pos"][:, :1].contiguous()), ("score", outs["score"][0]), ("vis", outs["score"]),
                      ("choice", outs["choice"].long()), ("err", outs["err"][..., :-1].contiguous())):
        with pytest.raises(RuntimeError, match={"vis": "visible", "err": "fb_err"}.get(name, name) + " must be"):
            call(**{name: bad})
    with pytest.raises(RuntimeError, match="cand_err must be"):
        call(cand=torch.empty(K - 1, H, W, device=cuda))
    # K*H*W must stay an int: 16 slots of 16384 x 8192 pixels, one element expanded (the size is checked first)
    huge = torch.zeros(1, device=cuda).expand(16, 2, 16384, 8192)
    with pytest.raises(RuntimeError, match=r"below 2\^31"):
        call(fw=huge, bw=huge)
    # the wrapper converts bf16 flows
    h16, hb = fw.to(torch.bfloat16), bw.to(torch.bfloat16)
    got = ops.dense_multi_flow_step(h16, hb, ring_pos.clone(), ring_score.clone(), idx, act)
    want = ops.dense_multi_flow_step(h16.float(), hb.float(), ring_pos.clone(), ring_score.clone(), idx, act)
    assert got[0].dtype == torch.float32 and all(D.same(a, b) for a, b in zip(got[:5], want[:5]))


# -------------------------------------------------------------------- capture
def test_op_is_graph_capturable(cuda):
    K, (H, W) = 3, (24, 70)
    first = D.step_inputs(K, H, W) + (torch.tensor([True, True, False]),)
    second = D.step_inputs(K, H, W, seed=1) + (torch.tensor([False, True, True]),)
    second = (first[1].flip(0), first[0].flip(0), second[2], second[3], torch.tensor([2, 4, 0, 1], dtype=torch.int32),
              second[5])
    third = first[:5] + (torch.tensor([False, False, False]),)
    fourth = first[:4] + (torch.tensor([-3, 1, 9, 4], dtype=torch.int32), torch.tensor([True, True, True]))
    static = [t.to(cuda).clone() for t in first]
    s = torch.cuda.Stream(device=cuda)
    s.wait_stream(torch.cuda.current_stream(cuda))
    with torch.cuda.stream(s):
        ops.dense_multi_flow_step(*static, *D.FB.ALPHA)
    torch.cuda.current_stream(cuda).wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        outs = ops.dense_multi_flow_step(*static, *D.FB.ALPHA)
    seen = []
    for ins in (second, third, fourth, first):
        for dst, src in zip(static, ins):
            dst.copy_(src)
        g.replay()
        dev = [t.to(cuda) for t in ins]
        eager = ops.dense_multi_flow_step(*dev, *D.FB.ALPHA)
        assert all(D.same(a, e) for a, e in zip(outs[:5], eager[:5]))
        assert D.same(static[2], dev[2]) and D.same(static[3], dev[3])  # the rings after the step
        seen.append(outs[3].clone())
    assert (seen[1] == -1).all() and (seen[0] >= 0).all() and not torch.equal(seen[0], seen[3])


# ---------------------------------------------------------- tracker, stub model
STUB_HW = (64, 96)


def _strict(fn):
    """fn() with host synchronisation forbidden, where this torch can."""
    if not hasattr(torch.cuda, "set_sync_debug_mode"):
        return fn()
    torch.cuda.synchronize()
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        return fn()
    finally:
        torch.cuda.set_sync_debug_mode(mode)


@pytest.mark.parametrize("cache_features", [False, True])
@pytest.mark.parametrize("deltas", [(1,), (2, 4), (1, 3, None)])
def test_tracker_with_stub_model(cuda, deltas, cache_features):
    """The CPU test's comparison at 64x96, graphed: against MultiFlowTracker on
    all pixel centres with the wobbling stub, and, with the stub whose
    positions are integers, against the eager CPU run as well, bit for bit."""
    H, W = STUB_HW
    L = max(d for d in deltas if d is not None)
    frames = D.frames(2 * L + 3, H, W)
    f, points = frames.to(cuda), D.pixel_centres(H, W, cuda)
    kw = dict(iters=2, deltas=deltas, cache_features=cache_features)
    for amp in (0.75, 0.0):
        stub = D.StubWobble(H, W, amp).to(cuda)
        dense, sparse = DenseMultiFlowTracker(stub, **kw), MultiFlowTracker(stub, **kw)
        cpu = DenseMultiFlowTracker(D.StubWobble(H, W, amp), **kw) if amp == 0 else None
        lost = found = False
        for t in range(len(frames)):
            pos = dense.step(f[t])
            sparse.step(f[t], points if t == 0 else None)
            assert pos.device.type == "cuda" and pos.shape == (1, 2, H, W)
            for name, a, b in zip(("pos", "visible", "score", "fb_err", "delta"), D.as_points(dense),
                                  D.of_points(sparse)):
                assert D.same(a, b), (amp, t, name)
            if cpu is not None:
                cpu.step(frames[t])
                for name, a, b in zip(("pos", "visible", "score", "fb_err", "delta"), D.as_points(dense),
                                      D.as_points(cpu)):
                    assert D.same(a.cpu(), b), (t, name)
            lost |= bool((~dense.visible).any())
            found |= t > 0 and bool(dense.visible.any())
        assert lost and found
        key = ((1, 3, H, W), deltas) + (("cache_features",) if cache_features else ())
        assert list(dense.graphs) == [key]
    # a second sequence replays the graph without a host synchronisation and gives the first one again
    flows, vis = dense.track(f)
    calls = stub.calls
    again = _strict(lambda: dense.track(f[:L + 2]))
    assert D.same(again[0], flows[:L + 2]) and torch.equal(again[1], vis[:L + 2])
    assert stub.calls == calls and len(dense.graphs) == 1
    pts, v, s = dense.query(points)
    assert D.same(pts, D.as_points(dense)[0]) and torch.equal(v, dense.visible.view(1, -1))


# ----------------------------------------------------------- tracker, real model
@pytest.fixture(scope="module", params=["fp32", "bf16"])
def model(request, cuda):
    torch.manual_seed(0)
    m = RAFT(make_args(small=True, mixed_precision=request.param == "bf16"))
    return m.to(cuda).to(memory_format=torch.channels_last).eval()


def test_tracker_with_real_model(cuda, model):
    """RAFT-small, random weights, 64x96, deltas=(1, 2, None): both trackers
    run the same pass on the same inputs, so everything is equal bit for bit,
    the flows first."""
    H, W = STUB_HW
    g = torch.Generator().manual_seed(5)
    frames = (torch.rand(6, 1, 3, H, W, generator=g) * 255).to(cuda)
    points = D.pixel_centres(H, W, cuda)
    kw = dict(iters=4, deltas=(1, 2, None), fb_alpha=ALPHA)
    dense, sparse = DenseMultiFlowTracker(model, **kw), MultiFlowTracker(model, **kw)
    found = False
    for t in range(6):
        dense.step(frames[t])
        sparse.step(frames[t], points if t == 0 else None)
        if t > 0:
            assert D.same(dense.flow_up, sparse.flow_up) and D.same(dense.flow_bw_up, sparse.flow_bw_up), t
            assert D.same(dense.next_init, sparse.next_init), t
        for name, a, b in zip(("pos", "visible", "score", "fb_err", "delta"), D.as_points(dense), D.of_points(sparse)):
            assert D.same(a, b), (t, name, int((a != b).sum()))
        found |= t > 0 and bool(dense.visible.any())
    print(f"visible at the end: {float(dense.visible.float().mean()):.3f}")
    assert found and torch.isfinite(dense.pos).all()
    # a second sequence of another length reuses the captured graph
    flows, vis = dense.track(frames[:4])
    assert flows.shape == (4, 2, H, W) and vis.shape == (4, 1, H, W) and (flows[0] == 0).all() and vis[0].all()
    assert len(dense.graphs) == 1 and list(dense.graphs) == [((1, 3, H, W), (1, 2, None))]

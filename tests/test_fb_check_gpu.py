"""Forward-backward check on the GPU: the kernels of csrc/fb_check.hip against
the fp64 oracle and hand-worked cases, their host checks and hipGraph capture,
the bidirectional RAFT pass through the fused inference engine, and the
graphed SequenceTracker(fb_check=True) with a stub and with the real model."""
import pytest
import torch

from raft_stir_amd import ops
from raft_stir_amd.config import make_args
from raft_stir_amd.export.pointtrack import SequenceTracker
from raft_stir_amd.models import RAFT
from raft_stir_amd.ops import reference

import fb_check_cases as C

pytestmark = pytest.mark.gpu

TOL = dict(atol=2e-3, rtol=2e-3)  # the same mathematics on different kernels, as tests/test_warm_start_gpu.py


def _cpu(ts):
    return tuple(t.cpu() for t in ts)


# ------------------------------------------------------------ kernel vs oracle
@pytest.mark.parametrize("shape", C.DENSE_SHAPES)
def test_dense_kernel_against_fp64(cuda, shape):
    """Measured maximum of |err - err64| over the shapes: 2.13 * 2^-24 * M
    (bound 32 * 2^-24 * M); pixels in the threshold band at most 0.21 %
    (43 of 20480; bound 1 %), no mask mismatch outside it."""
    B, H, W = shape
    fw, bw = C.flow_pair(B, H, W)
    err, ok = ops.fb_consistency(fw.to(cuda), bw.to(cuda))
    assert err.device.type == "cuda" and ok.device.type == "cuda"
    C.check_dense(f"dense{shape}", fw, bw, err.cpu(), ok.cpu())
    again = ops.fb_consistency(fw.to(cuda), bw.to(cuda))
    assert C.same(again[0], err) and torch.equal(again[1], ok)
    if B == 2:  # batch images are independent
        one = ops.fb_consistency(fw[:1].to(cuda), bw[:1].to(cuda))
        assert torch.equal(one[0], err[:1]) and torch.equal(one[1], ok[:1])


@pytest.mark.parametrize("N", C.POINT_COUNTS)
def test_points_kernel_against_fp64(cuda, N):
    """Measured maximum error of new_points and err: 4.86 * 2^-24 * M (bound
    32 * 2^-24 * M), 2 of 2000 points in the threshold band; new_points against
    points + sample_points: at most 4.8e-6 (tolerance 1.07e-4)."""
    B, H, W = C.POINT_SHAPE
    fw, bw = C.flow_pair(B, H, W)
    pts = C.points_for(N)
    out = ops.fb_track_points(fw.to(cuda), bw.to(cuda), pts.to(cuda))
    assert all(t.device.type == "cuda" for t in out)
    new, err, ok = _cpu(out)
    C.check_points(f"points{N}", fw, bw, pts, new, err, ok)
    again = ops.fb_track_points(fw.to(cuda), bw.to(cuda), pts.to(cuda))
    assert all(C.same(a, b) for a, b in zip(again, out))
    one = ops.fb_track_points(fw[:1].to(cuda), bw[:1].to(cuda), pts[:1].to(cuda))
    assert all(C.same(a, b[:1]) for a, b in zip(one, out))
    C.check_against_sample_points(f"points{N}", fw, pts, new)


def test_hand_worked_edge_cases(cuda):
    def dense(fw, bw, a1, a2):
        return _cpu(ops.fb_consistency(fw.to(cuda), bw.to(cuda), a1, a2))

    def points(fw, bw, pts, a1, a2):
        return _cpu(ops.fb_track_points(fw.to(cuda), bw.to(cuda), pts.to(cuda), a1, a2))

    C.check_edge_cases(dense, points)


# ---------------------------------------------------------------- host checks
def test_host_checks(cuda):
    dense, track = torch.ops.raft_stir.fb_consistency, torch.ops.raft_stir.fb_track_points
    fw, bw = (t.to(cuda) for t in C.flow_pair(1, 16, 20))
    pts = (C.points_for(16)[:1] * 0.25).to(cuda)
    for call in (lambda f, b: dense(f, b, 0.01, 0.5), lambda f, b: track(f, b, pts, 0.01, 0.5)):
        with pytest.raises(RuntimeError, match="fp32"):
            call(fw.to(torch.bfloat16), bw.to(torch.bfloat16))
        with pytest.raises(RuntimeError, match="contiguous"):
            call(fw.transpose(2, 3), bw.transpose(2, 3))
        with pytest.raises(RuntimeError, match="same shape"):
            call(fw, bw[..., :-1].contiguous())
        with pytest.raises(RuntimeError, match="H, W >= 2"):
            call(fw[:, :, :1].contiguous(), bw[:, :, :1].contiguous())
        with pytest.raises(RuntimeError, match="same device"):
            call(fw, bw.cpu())
    for a1, a2 in ((-0.01, 0.5), (0.01, -0.5), (float("nan"), 0.5)):
        with pytest.raises(RuntimeError, match="alpha"):
            dense(fw, bw, a1, a2)
        with pytest.raises(RuntimeError, match="alpha"):
            track(fw, bw, pts, a1, a2)
    with pytest.raises(RuntimeError, match=r"\(B,N,2\)"):
        track(fw, bw, pts[0], 0.01, 0.5)
    with pytest.raises(RuntimeError, match=r"\(B,N,2\)"):
        track(fw, bw, pts[..., :1].contiguous(), 0.01, 0.5)
    with pytest.raises(RuntimeError, match=r"\(B,N,2\)"):
        track(fw, bw, torch.cat([pts, pts]), 0.01, 0.5)  # another batch
    with pytest.raises(RuntimeError, match="fp32 points"):
        track(fw, bw, pts.double(), 0.01, 0.5)
    with pytest.raises(RuntimeError, match="contiguous points"):
        track(fw, bw, pts.flip(2).transpose(1, 2).contiguous().transpose(1, 2), 0.01, 0.5)
    with pytest.raises(RuntimeError, match="same device"):
        track(fw, bw, pts.cpu(), 0.01, 0.5)
    # the wrappers convert bf16 and non-contiguous inputs
    h16, hb = fw.to(torch.bfloat16), bw.to(torch.bfloat16)
    got = ops.fb_track_points(h16, hb, pts.double())
    want = reference.fb_track_points(h16.float().cpu(), hb.float().cpu(), pts.cpu())
    assert got[0].dtype == torch.float32 and got[1].dtype == torch.float32 and got[2].dtype == torch.bool
    C.check_points("bf16 inputs", h16.float().cpu(), hb.float().cpu(), pts.cpu(), *_cpu(got), min_class=0)
    assert torch.equal(got[1].cpu() == C.INF, want[1] == C.INF)
    t_fw, t_bw = fw.transpose(2, 3), bw.transpose(2, 3)  # (1,2,20,16), not contiguous
    err, ok = ops.fb_consistency(t_fw, t_bw)
    C.check_dense("transposed", t_fw.cpu().contiguous(), t_bw.cpu().contiguous(), err.cpu(), ok.cpu(), min_class=0)


# -------------------------------------------------------------------- capture
def test_ops_are_graph_capturable(cuda):
    B, H, W = C.POINT_SHAPE
    fw, bw = C.flow_pair(B, H, W)
    pts = C.points_for(70)
    second = (bw.flip(0), fw.flip(0), C.points_for(70, seed=9))
    s_fw, s_bw, s_p = fw.to(cuda), bw.to(cuda), pts.to(cuda)

    def both():
        return ops.fb_consistency(s_fw, s_bw) + ops.fb_track_points(s_fw, s_bw, s_p)

    s = torch.cuda.Stream(device=cuda)
    s.wait_stream(torch.cuda.current_stream(cuda))
    with torch.cuda.stream(s):
        both()
    torch.cuda.current_stream(cuda).wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        outs = both()
    for f, b, p in (second, (fw, bw, pts)):
        s_fw.copy_(f)
        s_bw.copy_(b)
        s_p.copy_(p)
        g.replay()
        eager = ops.fb_consistency(f.to(cuda), b.to(cuda)) + ops.fb_track_points(f.to(cuda), b.to(cuda), p.to(cuda))
        assert all(C.same(a, e) for a, e in zip(outs, eager))
    assert outs[1].any() and not outs[1].all() and outs[4].any() and not outs[4].all()


# --------------------------------------------------------- bidirectional pass
@pytest.fixture(scope="module")
def pair(cuda):
    g = torch.Generator().manual_seed(7)
    a, b = torch.rand(1, 3, 128, 160, generator=g) * 255, torch.rand(1, 3, 128, 160, generator=g) * 255
    init = torch.randn(2, 2, 16, 20, generator=g)
    return a.to(cuda), b.to(cuda), init.to(cuda)


def _bidirectional_against_batched(model, pair, inits):
    a, b, init = pair
    with torch.no_grad():
        for fi in inits:
            fi = init if fi else None
            lo, up = model(a, b, iters=4, flow_init=fi, test_mode=True, bidirectional=True)
            wlo, wup = model(torch.cat([a, b]), torch.cat([b, a]), iters=4, flow_init=fi, test_mode=True)
            assert lo.shape == (2, 2, 16, 20) and up.shape == (2, 2, 128, 160)
            torch.testing.assert_close(lo, wlo, **TOL)
            torch.testing.assert_close(up, wup, **TOL)
            assert (up[0] - up[1]).abs().max() > 1e-3  # two directions, not one twice


@pytest.fixture(scope="module")
def model(cuda):
    torch.manual_seed(0)
    return RAFT(make_args(small=True)).to(cuda).to(memory_format=torch.channels_last).eval()


def test_bidirectional_small_matches_batched_pairs(cuda, model, pair):
    _bidirectional_against_batched(model, pair, (False, True))
    assert model.__dict__.get("_fused") is not None  # the fused inference engine ran


def test_bidirectional_full_matches_batched_pairs(cuda, pair):
    torch.manual_seed(0)
    full = RAFT(make_args()).to(cuda).to(memory_format=torch.channels_last).eval()
    _bidirectional_against_batched(full, pair, (True,))


def test_bidirectional_alternate_corr_matches_batched_pairs(cuda, pair):
    torch.manual_seed(0)
    alt = RAFT(make_args(small=True, alternate_corr=True)).to(cuda).to(memory_format=torch.channels_last).eval()
    _bidirectional_against_batched(alt, pair, (True,))


def test_bidirectional_argument_checks(cuda, model, pair):
    a, b, _ = pair
    with torch.no_grad():
        with pytest.raises(ValueError, match="test_mode"):
            model(a, b, iters=1, bidirectional=True)
        with pytest.raises(ValueError, match="shape"):
            model(a, b[..., :152], iters=1, test_mode=True, bidirectional=True)


def test_bidirectional_is_graph_capturable(cuda, model, pair):
    a, b, init = pair
    sa, sb, si = a.clone(), b.clone(), torch.zeros_like(init)
    with torch.no_grad():
        s = torch.cuda.Stream(device=cuda)
        s.wait_stream(torch.cuda.current_stream(cuda))
        with torch.cuda.stream(s):
            for _ in range(2):
                model(sa, sb, iters=4, flow_init=si, test_mode=True, bidirectional=True)
        torch.cuda.current_stream(cuda).wait_stream(s)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            lo, up = model(sa, sb, iters=4, flow_init=si, test_mode=True, bidirectional=True)
        sa.copy_(b)
        sb.copy_(a)
        si.copy_(init)
        g.replay()
        wlo, wup = model(b, a, iters=4, flow_init=init, test_mode=True, bidirectional=True)
    torch.testing.assert_close(lo, wlo, **TOL)
    torch.testing.assert_close(up, wup, **TOL)


# ----------------------------------------------------------- tracker, stub model
def test_tracker_with_stub_model(cuda):
    frames, points = C.stub_sequence()
    stub = C.StubFlow().to(cuda)
    trk = SequenceTracker(stub, iters=2, warm_start=True, fb_check=True)
    traj, vis, err = trk.track(frames.to(cuda), points.to(cuda), return_visibility=True)
    assert traj.device.type == "cuda" and vis.device.type == "cuda" and err.device.type == "cuda"
    C.check_stub_tracking(traj.cpu(), vis.cpu(), err.cpu(), points)
    assert len(trk.graphs) == 1
    calls = stub.calls  # warm-up and capture only: the steps replay the graph
    trk.reset()
    assert torch.equal(trk.step(frames[0].to(cuda), points.to(cuda)).cpu(), points)
    assert trk.visible.shape == (1, 5) and trk.visible.all() and (trk.fb_err == 0).all()
    for t in range(1, 4):
        trk.step(frames[t].to(cuda))
        assert torch.equal(trk.visible[0], vis[t]) and C.same(trk.fb_err[0], err[t])
    assert stub.calls == calls and len(trk.graphs) == 1


# ----------------------------------------------------------- tracker, real model
@pytest.fixture(scope="module")
def sequence(cuda):
    g = torch.Generator().manual_seed(5)
    frames = torch.rand(4, 1, 3, 128, 160, generator=g) * 255
    points = torch.rand(1, 16, 2, generator=g) * torch.tensor([159.0, 127.0])
    return frames.to(cuda), points.to(cuda)


ALPHA = (0.02, 2.0)


def test_tracker_teacher_forced_against_eager(cuda, model, sequence):
    frames, points = sequence
    trk = SequenceTracker(model, iters=4, warm_start=True, fb_check=True, fb_alpha=ALPHA)
    assert torch.equal(trk.step(frames[0], points), points)
    assert trk.visible.all() and (trk.fb_err == 0).all()
    prev_pts, carried = points, None
    compared = 0
    for t in range(1, 4):
        pts = trk.step(frames[t]).clone()
        init = torch.cat([trk.flow_init, trk.flow_bw_init]).clone()
        if carried is None:
            assert (init == 0).all()  # the first pair starts cold in both directions
        else:
            assert torch.equal(init, carried)  # the inits used now are the last step's next inits
        assert torch.equal(trk.next_init, ops.forward_interpolate(trk.flow_low))
        assert torch.equal(trk.next_bw_init, -ops.forward_interpolate(-trk.flow_bw_low))
        assert trk.fb_err.shape == (1, 16) and trk.visible.shape == (1, 16) and trk.visible.dtype == torch.bool
        with torch.no_grad():
            lo, up = model(frames[t - 1], frames[t], iters=4, flow_init=init, test_mode=True, bidirectional=True)
        want, err, ok = ops.fb_track_points(up[0:1], up[1:2], prev_pts, *ALPHA)
        torch.testing.assert_close(trk.flow_up, up[0:1], **TOL)
        torch.testing.assert_close(trk.flow_bw_up, up[1:2], **TOL)
        torch.testing.assert_close(trk.flow_low, lo[0:1], **TOL)
        torch.testing.assert_close(trk.flow_bw_low, lo[1:2], **TOL)
        torch.testing.assert_close(pts, want, **TOL)
        assert torch.equal(torch.isinf(trk.fb_err), torch.isinf(err))
        fin = torch.isfinite(err)
        torch.testing.assert_close(trk.fb_err[fin], err[fin], **TOL)
        # visible only where the eager e2 is further from the threshold than TOL allows: the four
        # vectors of e2 and m2 may each be off by tol, so e2 by 2*|s|*2*tol and the threshold less
        uv = (want - prev_pts).double()
        _, e2, m2 = reference.fb_terms(up[1:2].cpu(), prev_pts[..., 0].cpu(), prev_pts[..., 1].cpu(),
                                       uv[..., 0].cpu(), uv[..., 1].cpu(), torch.float64)
        tol = TOL["atol"] + TOL["rtol"] * up.abs().max().item()
        margin = 4 * e2.sqrt() * tol + 4 * tol * tol + ALPHA[0] * 4 * m2.sqrt() * tol
        clear = (fin.cpu() & ((e2 - (ALPHA[0] * m2 + ALPHA[1])).abs() > margin)) | ~fin.cpu()
        assert torch.equal(trk.visible.cpu()[clear], ok.cpu()[clear])
        compared += int(clear.sum())
        # fb_map: the dense op on the stored fields
        err_map, ok_map = trk.fb_map()
        dense = ops.fb_consistency(trk.flow_up, trk.flow_bw_up, *ALPHA)
        assert C.same(err_map, dense[0]) and torch.equal(ok_map, dense[1]) and err_map.shape == (1, 1, 128, 160)
        prev_pts, carried = pts, torch.cat([trk.next_init, trk.next_bw_init]).clone()
    assert carried.abs().max() > 0 and compared >= 24
    assert len(trk.graphs) == 1
    traj, vis, err = trk.track(frames, points, return_visibility=True)
    assert traj.shape == (4, 16, 2) and vis.shape == (4, 16) and err.shape == (4, 16)
    assert torch.equal(traj[0], points[0]) and vis[0].all() and (err[0] == 0).all()
    assert len(trk.graphs) == 1


def test_tracker_steps_do_not_synchronise(cuda, model, sequence):
    if not hasattr(torch.cuda, "set_sync_debug_mode"):
        pytest.skip("this torch build has no torch.cuda.set_sync_debug_mode")
    frames, points = sequence
    trk = SequenceTracker(model, iters=4, warm_start=True, fb_check=True, fb_alpha=ALPHA)
    want = trk.track(frames, points, return_visibility=True)  # captures the graph
    torch.cuda.synchronize()
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        traj, vis, err = trk.track(frames, points, return_visibility=True)
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    # the cold first pair only: a nearest-sample choice may turn a last-bit difference
    # between two replays into another init for the later pairs
    torch.testing.assert_close(traj[1], want[0][1], **TOL)
    assert torch.isfinite(traj).all() and vis.dtype == torch.bool and err.shape == (4, 16)


def test_plain_tracker_unchanged_by_fb_tracker(cuda, model, sequence):
    """A tracker without fb_check gives bit-equal results before and after an
    fb_check tracker ran on the same model (the packed-weight caches and the
    fused engine's buffers are shared), with its graph keys as before."""
    frames, points = sequence
    plain = SequenceTracker(model, iters=4)
    before = plain.track(frames, points).clone()
    assert list(plain.graphs) == [((1, 3, 128, 160), 16)]
    SequenceTracker(model, iters=4, fb_check=True).track(frames, points)
    after = plain.track(frames, points)
    assert torch.equal(before, after)
    fresh = SequenceTracker(model, iters=4).track(frames, points)
    assert torch.equal(before, fresh)
    assert plain.visible is None and plain.fb_err is None and plain.flow_bw_up is None

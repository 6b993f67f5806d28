"""Warm-started sequence tracking on the GPU: the forward-interpolation kernel
bit for bit against the ATen oracle, its host checks, hipGraph capture, the
graphed SequenceTracker (teacher-forced against eager) and the Sintel
submission with the warm start kept on the device."""
import glob

import numpy as np
import pytest
import torch

from raft_stir_amd import ops
from raft_stir_amd.config import make_args
from raft_stir_amd.export.pointtrack import PointTrackServer, SequenceTracker, sample_points
from raft_stir_amd.models import RAFT
from raft_stir_amd.ops import reference

from warm_start_cases import FAR, check_against_fp64, check_edge_outputs, edge_cases, smooth

pytestmark = pytest.mark.gpu


def _batch(B, H, W):
    return torch.stack([smooth(H, W, seed, 6, 0.5) for seed in range(B)])


# ------------------------------------------------------------ kernel vs oracle
@pytest.mark.parametrize("shape", [(1, 5, 7),      # less than one wave
                                   (1, 16, 20),    # a partial block
                                   (2, 46, 62),    # several sample tiles and chunks; image 1 all invalid
                                   (1, 64, 80)])   # STIR's 1/8 field
def test_kernel_matches_oracle(cuda, shape):
    B, H, W = shape
    flow = _batch(B, H, W)
    if B == 2:
        flow[1] += FAR
    want = reference.forward_interpolate(flow)
    got = ops.forward_interpolate(flow.to(cuda))
    assert got.dtype == torch.float32 and got.device.type == "cuda" and got.shape == flow.shape
    assert torch.equal(got.cpu(), want)
    assert torch.equal(ops.forward_interpolate(flow.to(cuda)), got)  # the same call twice: bit-equal
    if H * W <= 46 * 62:  # the fp64 table of the check is N x N
        check_against_fp64(flow[0], got[0].cpu())
    if B == 2:
        assert (got[1] == 0).all()
        assert torch.equal(got[0], ops.forward_interpolate(flow[0].to(cuda)))  # image 0 unaffected


def test_kernel_edge_inputs(cuda):
    outs = {}
    for name, flow, _ in edge_cases():
        outs[name] = ops.forward_interpolate(flow.to(cuda)).cpu()
        assert torch.equal(outs[name], reference.forward_interpolate(flow)), name
    check_edge_outputs(outs)


def test_kernel_3d_input_and_out_argument(cuda):
    flow = smooth(16, 20, 1, 6, 0.5).to(cuda)
    a = ops.forward_interpolate(flow)
    assert a.shape == (2, 16, 20) and torch.equal(a, ops.forward_interpolate(flow[None])[0])
    buf = torch.full((1, 2, 16, 20), 7.0, device=cuda)
    ret = torch.ops.raft_stir.forward_interpolate(flow[None], out=buf)
    assert ret.data_ptr() == buf.data_ptr() and torch.equal(buf[0], a)


# ---------------------------------------------------------------- host checks
def test_host_checks(cuda):
    raw = torch.ops.raft_stir.forward_interpolate
    with pytest.raises(RuntimeError, match="65536"):
        raw(torch.zeros(1, 2, 257, 256, device=cuda))
    flow = smooth(16, 20, 0, 6, 0.5)[None].to(cuda)
    with pytest.raises(RuntimeError, match="fp32"):
        raw(flow.to(torch.bfloat16))
    swapped = flow.transpose(2, 3)  # (1,2,20,16), not contiguous
    with pytest.raises(RuntimeError, match="contiguous"):
        raw(swapped)
    with pytest.raises(RuntimeError, match=r"\(B,2,H,W\)"):
        raw(flow[0])
    with pytest.raises(RuntimeError, match="alias"):
        raw(flow, out=flow)
    # the wrapper converts such inputs
    got = ops.forward_interpolate(flow.to(torch.bfloat16))
    assert got.dtype == torch.float32
    assert torch.equal(got.cpu(), reference.forward_interpolate(flow.to(torch.bfloat16).float().cpu()))
    assert torch.equal(ops.forward_interpolate(swapped).cpu(), reference.forward_interpolate(swapped.cpu()))


# -------------------------------------------------------------------- capture
def test_op_is_graph_capturable(cuda):
    first, second = smooth(46, 62, 0, 6, 0.5)[None], smooth(46, 62, 1, 1, 0.1)[None]
    static = first.to(cuda)
    s = torch.cuda.Stream(device=cuda)
    s.wait_stream(torch.cuda.current_stream(cuda))
    with torch.cuda.stream(s):
        ops.forward_interpolate(static)
    torch.cuda.current_stream(cuda).wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = ops.forward_interpolate(static)
    for flow in (second, first):
        static.copy_(flow)
        g.replay()
        assert torch.equal(out, ops.forward_interpolate(flow.to(cuda)))
        assert torch.equal(out.cpu(), reference.forward_interpolate(flow))


# ------------------------------------------------------------ SequenceTracker
@pytest.fixture(scope="module")
def model(cuda):
    torch.manual_seed(0)
    return RAFT(make_args(small=True)).to(cuda).to(memory_format=torch.channels_last).eval()


@pytest.fixture(scope="module")
def sequence(cuda):
    g = torch.Generator().manual_seed(5)
    frames = torch.rand(4, 1, 3, 128, 160, generator=g) * 255
    points = torch.rand(1, 16, 2, generator=g) * torch.tensor([159.0, 127.0])
    return frames.to(cuda), points.to(cuda)


TOL = dict(atol=2e-3, rtol=2e-3)  # graph against eager, as test_graphed_inference_matches_eager


def test_tracker_teacher_forced_against_eager(cuda, model, sequence):
    frames, points = sequence
    trk = SequenceTracker(model, iters=4, warm_start=True)
    assert torch.equal(trk.step(frames[0], points), points)
    prev_pts, carried, first = points, None, None
    for t in range(1, 4):
        pts = trk.step(frames[t]).clone()
        init = trk.flow_init.clone()
        if carried is None:
            assert (init == 0).all()  # the first pair starts cold
        else:
            assert torch.equal(init, carried)  # the init used now is the last step's next_init
        assert torch.equal(trk.next_init, ops.forward_interpolate(trk.flow_low))
        with torch.no_grad():
            lo, up = model(frames[t - 1], frames[t], iters=4, flow_init=init, test_mode=True)
        torch.testing.assert_close(trk.flow_up, up, **TOL)
        torch.testing.assert_close(trk.flow_low, lo, **TOL)
        torch.testing.assert_close(pts, prev_pts + sample_points(up, prev_pts), **TOL)
        prev_pts, carried = pts, trk.next_init.clone()
        first = pts if first is None else first
    assert carried.abs().max() > 0
    assert len(trk.graphs) == 1
    # a second sequence through the same graph: reset, then track() on the (T,1,3,H,W) tensor
    traj = trk.track(frames, points)
    assert traj.shape == (4, 16, 2) and torch.equal(traj[0], points[0])
    # (only the cold first pair is compared: a nearest-sample choice may turn a last-bit
    # difference between two replays into another init for the later pairs)
    torch.testing.assert_close(traj[1:2], first, **TOL)
    assert torch.isfinite(traj).all()
    assert len(trk.graphs) == 1


def test_tracker_without_warm_start_matches_point_track_server(cuda, model, sequence):
    frames, points = sequence
    trk = SequenceTracker(model, iters=4, warm_start=False)
    server = PointTrackServer(model, iters=4)
    prev_pts = trk.step(frames[0], points).clone()
    for t in range(1, 4):
        pts = trk.step(frames[t]).clone()
        assert (trk.flow_init == 0).all() and (trk.next_init == 0).all()
        torch.testing.assert_close(pts, server(prev_pts, frames[t - 1], frames[t]), **TOL)
        prev_pts = pts


def test_tracker_steps_do_not_synchronise(cuda, model, sequence):
    if not hasattr(torch.cuda, "set_sync_debug_mode"):
        pytest.skip("this torch build has no torch.cuda.set_sync_debug_mode")
    frames, points = sequence
    trk = SequenceTracker(model, iters=4, warm_start=True)
    want = trk.track(frames, points)  # captures the graph
    torch.cuda.synchronize()
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        trk.reset()
        trk.step(frames[0], points)
        got = [trk.step(frames[t]) for t in range(1, 4)]
        traj = trk.track(frames, points)
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    got = torch.cat(got)
    assert got.shape == (3, 16, 2) and torch.isfinite(got).all() and torch.isfinite(traj).all()
    assert torch.equal(traj[0], points[0])
    # the cold first pair only (see test_tracker_teacher_forced_against_eager)
    torch.testing.assert_close(got[0], want[1], **TOL)
    torch.testing.assert_close(traj[1], want[1], **TOL)


# ---------------------------------------------------------- Sintel submission
@pytest.mark.parametrize("device_warm_start", [None, False])
def test_sintel_submission_warm_start(cuda, model, fake_root, tmp_path, device_warm_start):
    from raft_stir_amd.data import frame_utils as fu
    from raft_stir_amd.eval import evaluate as ev
    ev.create_sintel_submission(model, iters=2, warm_start=True, root=f"{fake_root}/Sintel",
                                output_path=str(tmp_path / "sintel"), device_warm_start=device_warm_start)
    flos = sorted(glob.glob(str(tmp_path / "sintel" / "*" / "*" / "*.flo")))
    assert len(flos) == 8  # 2 passes x 2 scenes x 2 pairs
    for f in flos:
        flow = fu.readFlow(f)
        assert flow.shape == (128, 160, 2) and np.isfinite(flow).all()

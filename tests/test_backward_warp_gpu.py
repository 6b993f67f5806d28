"""The kernel of csrc/backward_warp.hip against the ATen oracle on the CPU, bit
for bit: every case of backward_warp_cases and one of several blocks plus a
partial one, both dtypes, 1, 3, 4 and 16 channels, planar and channels-last
images, with and without ``valid``, into buffers filled with garbage; the
wrapper's conversions and the op's host checks; the op under graph capture;
DenseMultiFlowTracker.stabilize / warp_image with RAFT-small against the oracle
on the tracker's own published tensors; and track.py --dense --stabilize
--overlay on the GPU against the same run on the CPU."""
import glob
import os
import sys

import pytest
import torch

from raft_stir_amd import ops
from raft_stir_amd.config import make_args
from raft_stir_amd.export.denseflow import DenseMultiFlowTracker
from raft_stir_amd.models import RAFT
from raft_stir_amd.ops import reference

import backward_warp_cases as C
import dense_flow_cases as D

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHANNELS = C.CHANNELS + (16,)
HW = (64, 96)  # the frame size of test_reanchor_gpu.py
ALPHA = (0.02, 2.0)


def _garbage(cuda, dt, ch, H, W):
    fill = 123 if dt == "uint8" else C.NAN
    return (torch.full((1, ch, H, W), fill, dtype=C.DTYPES[dt], device=cuda),
            torch.full((1, 1, H, W), 255, dtype=torch.uint8, device=cuda).view(torch.bool))


def _all_same(got, want, what):
    for name, g, w in zip(("warped", "ok"), got, want):
        assert g.device.type == "cuda", (what, name)
        g = g.cpu()
        assert g.dtype == w.dtype and g.shape == w.shape and C.same(g, w), (what, name, int((g != w).sum()))


def _last(img):
    return img.contiguous(memory_format=torch.channels_last)


@pytest.mark.parametrize("case", C.all_cases(big=True), ids=C.case_id)
def test_kernel_against_oracle(cuda, case):
    dt, im, size, fname = case
    (H, W), (Hs, Ws) = C.SIZES_WITH_BIG[size]
    coords = C.field(fname, H, W, Hs, Ws).to(cuda)
    valid = C.valid(H, W).to(cuda)
    for ch in CHANNELS:
        planar = C.image(im, dt, ch, Hs, Ws).to(cuda)
        for what, img in (("planar", planar), ("channels-last", _last(planar))):
            for with_valid in (False, True):
                want = C.expected(im, dt, ch, size, fname, with_valid)
                out = _garbage(cuda, dt, ch, H, W)
                back = ops.backward_warp(img, coords, valid if with_valid else None, C.FILL[dt], out=out)
                assert back[0] is out[0] and back[1] is out[1]
                _all_same(out, want, (ch, what, with_valid))
                # ok is a bool of 0 or 1, whatever the buffer held
                assert int(out[1].view(torch.uint8).max()) <= 1
    _all_same(ops.backward_warp(planar, coords, valid, C.FILL[dt]), want, "allocated")


@pytest.mark.parametrize("dt", ["fp32", "uint8"])
def test_wrapper_converts_dtypes_and_layouts(cuda, dt):
    size = 4
    (H, W), (Hs, Ws) = C.SIZES[size]
    im = C.IMAGES[dt][2]
    coords, valid = C.field("edge", H, W, Hs, Ws).to(cuda), C.valid(H, W).to(cuda)
    for ch in (3, 4):
        want = C.expected(im, dt, ch, size, "edge", True)
        img = C.image(im, dt, ch, Hs, Ws).to(cuda)
        # float64 coords in another layout; a slice of a wider image (no layout the kernel reads: made contiguous)
        sliced = torch.cat([img, img], 3)[..., :Ws]
        assert not sliced.is_contiguous() and not sliced.is_contiguous(memory_format=torch.channels_last)
        got = ops.backward_warp(sliced, coords.double().transpose(2, 3).contiguous().transpose(2, 3), valid,
                                C.FILL[dt])
        _all_same(got, want, (ch, "converted"))
        assert all(g.is_contiguous() for g in got)
        # a channels-last image that starts one element into its storage: no packed load is aligned there
        buf = torch.zeros(ch * Hs * Ws + 1, dtype=img.dtype, device=cuda)
        odd = buf[1:].view(1, Hs, Ws, ch).permute(0, 3, 1, 2)
        odd.copy_(img)
        assert odd.is_contiguous(memory_format=torch.channels_last) and odd.data_ptr() % (4 * img.element_size())
        _all_same(ops.backward_warp(odd, coords, valid, C.FILL[dt]), want, (ch, "odd start"))
    # fill 0 by default
    got = ops.backward_warp(img, coords)
    want = C.expected(im, dt, 4, size, "edge", False, 0)
    _all_same(got, want, "fill 0")


def test_host_checks(cuda):
    (H, W), (Hs, Ws) = C.SIZES[2]
    img, u8 = C.image("ramp", "fp32", 3, Hs, Ws).to(cuda), C.image("ramp", "uint8", 3, Hs, Ws).to(cuda)
    coords, valid = C.field("smooth", H, W, Hs, Ws).to(cuda), C.valid(H, W).to(cuda)
    out, out8 = _garbage(cuda, "fp32", 3, H, W), _garbage(cuda, "uint8", 3, H, W)
    # the wrapper
    for bad in (torch.zeros(1, 0, Hs, Ws, device=cuda), torch.zeros(1, 17, Hs, Ws, device=cuda)):
        with pytest.raises(ValueError, match="1 <= C <= 16"):
            ops.backward_warp(bad, coords)
    for bad in (img[0], img[0, 0], img[None]):
        with pytest.raises(ValueError, match=r"image must be \(1,C,Hs,Ws\)"):
            ops.backward_warp(bad, coords)
    for bad in (coords[0], coords[None], coords[:, :1]):
        with pytest.raises(ValueError, match=r"coords must be \(1,2,H,W\)"):
            ops.backward_warp(img, bad)
    with pytest.raises(ValueError, match="same device"):
        ops.backward_warp(img, coords.cpu())
    with pytest.raises(ValueError, match="same device"):
        ops.backward_warp(img.cpu(), coords)
    with pytest.raises(ValueError, match="same device"):
        ops.backward_warp(img, coords, valid.cpu())
    for bad in (1.0, 0.5, 256, -1):
        with pytest.raises(ValueError, match=r"fill must be an integer in \[0, 255\]"):
            ops.backward_warp(u8, coords, fill=bad)
    for bad, match in (((out8[0], out[1]), "out warped"), ((out[0], out[1].view(torch.uint8)), "out ok"),
                       ((out[0].cpu(), out[1]), "out warped"), ((out[0].double(), out[1]), "out warped")):
        with pytest.raises(ValueError, match=match):
            ops.backward_warp(img, coords, out=bad)
    # the op itself
    op = torch.ops.raft_stir.backward_warp
    op(img, coords, valid, 1.5, *out)
    op(u8, coords, None, 7.0, *out8)
    for bad in (torch.zeros(1, 0, Hs, Ws, device=cuda), torch.zeros(1, 17, Hs, Ws, device=cuda)):
        with pytest.raises(RuntimeError, match="1 <= C <= 16"):
            op(bad, coords, valid, 0.0, *out)
    with pytest.raises(RuntimeError, match=r"image must be \(1,C,Hs,Ws\)"):
        op(img[0], coords, valid, 0.0, *out)
    with pytest.raises(RuntimeError, match="float32 or uint8"):
        op(img.double(), coords, valid, 0.0, *out)
    with pytest.raises(RuntimeError, match="contiguous or channels-last"):
        op(torch.cat([img, img], 3)[..., :Ws], coords, valid, 0.0, *out)
    with pytest.raises(RuntimeError, match="Hs, Ws >= 2"):
        op(img[..., :1].contiguous(), coords, valid, 0.0, *out)
    with pytest.raises(RuntimeError, match=r"below 2\^31"):
        op(torch.zeros(1, device=cuda).expand(1, 1, 32768, 65536), coords, valid, 0.0, *out)
    with pytest.raises(RuntimeError, match=r"coords must be \(1,2,H,W\)"):
        op(img, coords[0], valid, 0.0, *out)
    with pytest.raises(RuntimeError, match="coords must be a contiguous"):
        op(img, coords.double(), valid, 0.0, *out)
    with pytest.raises(RuntimeError, match="coords must be a contiguous"):
        op(img, coords.transpose(2, 3).contiguous().transpose(2, 3), valid, 0.0, *out)
    with pytest.raises(RuntimeError, match="valid must be a contiguous"):
        op(img, coords, valid.to(torch.uint8), 0.0, *out)
    with pytest.raises(RuntimeError, match="valid must be a contiguous"):
        op(img, coords, valid[..., :-1].contiguous(), 0.0, *out)
    with pytest.raises(RuntimeError, match="out warped must be"):
        op(img, coords, valid, 0.0, out8[0], out[1])
    with pytest.raises(RuntimeError, match="out warped must be"):
        op(img, coords, valid, 0.0, out[0][:, :2].contiguous(), out[1])
    with pytest.raises(RuntimeError, match="out ok must be"):
        op(img, coords, valid, 0.0, out[0], out[1].view(torch.uint8))
    for t in (1, 2):
        args = [img, coords, valid, 0.0, *out]
        args[t] = args[t].cpu()
        with pytest.raises(RuntimeError, match="same device"):
            op(*args)
    for bad in (0.5, 256.0, -1.0, float("nan")):
        with pytest.raises(RuntimeError, match=r"fill must be an integer in \[0, 255\]"):
            op(u8, coords, valid, bad, *out8)
    # an output that is an input
    with pytest.raises(RuntimeError, match="shares its storage"):
        op(img, coords, valid, 0.0, out[0], valid)
    both = torch.zeros(1, 3, H, W, device=cuda)  # an image of the output's size, given as the output too
    with pytest.raises(RuntimeError, match="shares its storage"):
        op(both, coords, valid, 0.0, both, out[1])


@pytest.mark.parametrize("dt", ["fp32", "uint8"])
def test_op_is_graph_capturable(cuda, dt):
    size = 3
    (H, W), (Hs, Ws) = C.SIZES[size]
    names = C.IMAGES[dt]
    first, others = (names[0], "identity"), [(names[2], "edge"), (names[1], "smooth"), (names[2], "edge")]
    img = _last(C.image(first[0], dt, 4, Hs, Ws).to(cuda).clone())
    coords = C.field(first[1], H, W, Hs, Ws).to(cuda).clone()
    valid = C.valid(H, W).to(cuda)
    out = _garbage(cuda, dt, 4, H, W)

    def run():
        ops.backward_warp(img, coords, valid, C.FILL[dt], out=out)
    s = torch.cuda.Stream(device=cuda)
    s.wait_stream(torch.cuda.current_stream(cuda))
    with torch.cuda.stream(s):
        run()
    torch.cuda.current_stream(cuda).wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        run()
    seen = []
    for im, fname in others:
        img.copy_(C.image(im, dt, 4, Hs, Ws))
        coords.copy_(C.field(fname, H, W, Hs, Ws))
        assert img.is_contiguous(memory_format=torch.channels_last)
        g.replay()
        _all_same(out, C.expected(im, dt, 4, size, fname, True), (im, fname))
        seen.append(out[0].clone())
    assert C.same(seen[0], seen[2]) and not C.same(seen[0], seen[1])
    assert img.is_cuda and g is not None  # the static inputs and the graph live to the end


# ------------------------------------------------------------------ the tracker
@pytest.fixture(scope="module", params=["fp32", "bf16"])
def model(request, cuda):
    torch.manual_seed(0)
    m = RAFT(make_args(small=True, mixed_precision=request.param == "bf16"))
    return m.to(cuda).to(memory_format=torch.channels_last).eval()


@pytest.mark.parametrize("cache_features", [False, True])
def test_tracker_methods_are_the_oracle_on_the_published_field(cuda, model, cache_features):
    H, W = HW
    g = torch.Generator().manual_seed(6)
    frames = (torch.rand(5, 1, 3, H, W, generator=g) * 255).floor()
    second = torch.randint(0, 256, (5, 1, 1, H, W), generator=g, dtype=torch.uint8)  # another modality
    overlay = {"fp32": torch.randn(1, 4, H, W, generator=g),
               "uint8": torch.randint(0, 256, (1, 3, H, W), generator=g, dtype=torch.uint8)}
    trk = DenseMultiFlowTracker(model, iters=4, deltas=(1, 2, None), fb_alpha=ALPHA, cache_features=cache_features)
    seen = holes = False
    for t in range(len(frames)):
        trk.step(frames[t].to(cuda))
        if t == 3:
            trk.reanchor()
        pos, vis = trk.pos.clone().cpu(), trk.visible.clone().cpu()
        keys = set(trk.graphs)
        # the static frame buffer, channels-last, read in place
        held = trk._st["frame"]
        assert held.is_contiguous(memory_format=torch.channels_last) and torch.equal(held.cpu(), frames[t])
        got = trk.stabilize()
        _all_same(got, reference.backward_warp(frames[t], pos, vis, 0), (t, "held"))
        _all_same(trk.stabilize(frames[t].to(cuda)), [x.cpu() for x in got], (t, "given"))
        assert got[0].data_ptr() != held.data_ptr()
        for img, fill in ((frames[t].to(torch.uint8), 9), (second[t], 0), (overlay["fp32"], -1.5)):
            got = trk.stabilize(img.to(cuda), fill=fill)
            _all_same(got, reference.backward_warp(img, pos, vis, fill), (t, img.dtype, "stabilize"))
        if t == 0:
            assert bool(got[1].all()) and torch.equal(trk.stabilize()[0].cpu(), frames[0])
        for inpaint in (0, 4):
            inv = trk.splat(None, footprint=2, inpaint=inpaint)[2].cpu()
            for name, img in overlay.items():
                fill = 5 if name == "uint8" else -2.0
                got = trk.warp_image(img.to(cuda), footprint=2, inpaint=inpaint, fill=fill)
                _all_same(got, reference.backward_warp(img, inv, None, fill), (t, name, inpaint))
            holes |= bool(torch.isnan(inv).any())
        seen |= t > 0 and bool(vis.any())
        # eager calls after the replay: no new graph, and what is published is untouched
        assert set(trk.graphs) == keys and len(keys) == 1
        assert C.same(trk.pos.cpu(), pos) and torch.equal(trk.visible.cpu(), vis)
    print(f"visible at the end: {float(vis.float().mean()):.3f}")
    assert seen and holes


@pytest.fixture(scope="module")
def cli():
    sys.path.insert(0, ROOT)
    try:
        import track
    finally:
        sys.path.remove(ROOT)
    return track


def test_track_cli_on_the_gpu_writes_the_cpu_files(cuda, cli, tmp_path):
    import numpy as np
    from PIL import Image
    images = sorted(glob.glob(os.path.join(ROOT, "demo-frames", "*.png")))
    W, H = Image.open(images[0]).size
    over = np.random.default_rng(4).integers(0, 256, (H, W, 4)).astype(np.uint8)
    Image.fromarray(over).save(tmp_path / "over.png")
    outs = {}
    for name, dev in (("cpu", torch.device("cpu")), ("gpu", cuda)):
        outs[name] = tmp_path / name
        args = cli.parse_args(["--dense", "--deltas", "1", "--iters", "2", "--stabilize", "--overlay",
                               str(tmp_path / "over.png"), "--inpaint", "3", "--out", str(outs[name])])
        cli.track_dense(args, D.StubAny().to(dev), images, None, dev)
    names = sorted(os.listdir(outs["cpu"]))
    assert names == sorted(os.listdir(outs["gpu"]))
    assert [n for n in names if n.startswith("stab_")] == [f"stab_{t:04d}.png" for t in range(3)]
    assert [n for n in names if n.startswith("overlay_")] == [f"overlay_{t:04d}.png" for t in range(3)]
    for n in names:
        assert open(outs["cpu"] / n, "rb").read() == open(outs["gpu"] / n, "rb").read(), n

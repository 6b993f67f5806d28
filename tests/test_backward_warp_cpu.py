"""ops.backward_warp on the CPU: the ATen oracle (ops/reference.py:
backward_warp) against a scalar fp32 brute force on every case of
backward_warp_cases, bit for bit; its invariance to the image's layout; the
wrapper's host checks; DenseMultiFlowTracker.stabilize / warp_image on a
translating stub; and track.py --dense --stabilize --overlay."""
import glob
import os
import sys

import numpy as np
import pytest
import torch

from raft_stir_amd import ops
from raft_stir_amd.export.denseflow import DenseMultiFlowTracker
from raft_stir_amd.ops import reference

import backward_warp_cases as C
import dense_flow_cases as D
import forward_splat_cases as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _same(got, want, what):
    for name, g, w in zip(("warped", "ok"), got, want):
        assert g.dtype == w.dtype and g.shape == w.shape and C.same(g, w), (what, name, int((g != w).sum()))


@pytest.mark.parametrize("case", C.all_cases(), ids=C.case_id)
def test_oracle_against_brute_force(case):
    dt, im, size, fname = case
    (H, W), (Hs, Ws) = C.SIZES[size]
    coords = C.field(fname, H, W, Hs, Ws)
    for with_valid in (False, True):
        v = C.valid(H, W) if with_valid else None
        want = C.brute_force(C.image(im, dt, 4, Hs, Ws), coords, v, C.FILL[dt])
        for ch in C.CHANNELS:
            got = C.expected(im, dt, ch, size, fname, with_valid)
            assert got[0].shape == (1, ch, H, W) and got[0].dtype == C.DTYPES[dt] and got[1].dtype == torch.bool
            _same(got, (want[0][:, :ch], want[1]), (ch, with_valid))
    # fill 0, the default
    got = reference.backward_warp(C.image(im, dt, 3, Hs, Ws), coords)
    want = C.expected(im, dt, 3, size, fname, False)
    assert torch.equal(got[1], want[1])
    zero = torch.zeros((), dtype=got[0].dtype)
    assert C.same(got[0], torch.where(want[1], want[0], zero))


def test_integer_positions_give_the_stored_values():
    (H, W), (Hs, Ws) = C.SIZES[4]
    coords = C.field("integers", H, W, Hs, Ws)
    idx = (coords[0, 1].long() * Ws + coords[0, 0].long()).flatten()
    for dt, im in (("fp32", "special"), ("fp32", "random"), ("uint8", "random")):
        img = C.image(im, dt, 3, Hs, Ws)
        got, ok = C.expected(im, dt, 3, 4, "integers", False)
        assert bool(ok.all())
        want = img.reshape(3, Hs * Ws)[:, idx].reshape(1, 3, H, W)
        if dt == "fp32":
            want = want + 0.0  # the rule's sum: a stored -0.0 reads as +0.0
        assert C.same(got, want)
    # no NaN or infinity of the image passes through a tap of weight 0
    got, _ = C.expected("special", "fp32", 1, 4, "integers", False)
    src = C.image("special", "fp32", 1, Hs, Ws).flatten()[idx]
    assert torch.equal(torch.isfinite(got).flatten(), torch.isfinite(src))


@pytest.mark.parametrize("dt", ["fp32", "uint8"])
def test_oracle_and_wrapper_do_not_depend_on_the_layout(dt):
    (H, W), (Hs, Ws) = C.SIZES[4]
    im = "special" if dt == "fp32" else "odd"
    coords, v = C.field("edge", H, W, Hs, Ws), C.valid(H, W)
    for ch in C.CHANNELS:
        img = C.image(im, dt, ch, Hs, Ws)
        want = C.expected(im, dt, ch, 4, "edge", True)
        last = img.contiguous(memory_format=torch.channels_last)
        other = torch.cat([img, img], 3)[..., :Ws]  # a row stride of 2 Ws
        assert not other.is_contiguous() and C.same(other, img) and C.same(last, img)
        for what, layout in (("channels-last", last), ("wide rows", other)):
            _same(reference.backward_warp(layout, coords, v, C.FILL[dt]), want, (ch, what))
            _same(ops.backward_warp(layout, coords, v, C.FILL[dt]), want, (ch, what, "wrapper"))
    # coords of another float dtype and layout; out=
    img = C.image(im, dt, 3, Hs, Ws)
    want = C.expected(im, dt, 3, 4, "edge", True)
    got = ops.backward_warp(img, coords.double().transpose(2, 3).contiguous().transpose(2, 3), v, C.FILL[dt])
    _same(got, want, "fp64 coords")
    out = (torch.full((1, 3, H, W), 9, dtype=C.DTYPES[dt]), torch.ones(1, 1, H, W, dtype=torch.bool))
    back = ops.backward_warp(img, coords, v, C.FILL[dt], out=out)
    assert back[0] is out[0] and back[1] is out[1]
    _same(out, want, "out=")


def test_wrapper_checks():
    (H, W), (Hs, Ws) = C.SIZES[2]
    img, u8 = C.image("ramp", "fp32", 3, Hs, Ws), C.image("ramp", "uint8", 3, Hs, Ws)
    coords, v = C.field("smooth", H, W, Hs, Ws), C.valid(H, W)
    assert "backward_warp" in ops.__all__
    for bad in (img[0], img.expand(2, -1, -1, -1), torch.zeros(1, 0, Hs, Ws), torch.zeros(1, 17, Hs, Ws)):
        with pytest.raises(ValueError, match=r"image must be \(1,C,Hs,Ws\)|1 <= C <= 16"):
            ops.backward_warp(bad, coords)
    for bad in (img.double(), img.half(), img.long()):
        with pytest.raises(ValueError, match="float32 or uint8"):
            ops.backward_warp(bad, coords)
    for bad in (coords[0], coords[:, :1], torch.zeros(1, 3, H, W), torch.zeros(2, 2, H, W)):
        with pytest.raises(ValueError, match=r"coords must be \(1,2,H,W\)"):
            ops.backward_warp(img, bad)
    with pytest.raises(ValueError, match="coords must be a float tensor"):
        ops.backward_warp(img, coords.long())
    with pytest.raises(ValueError, match=">= 2 expected"):
        ops.backward_warp(img[..., :1], coords)
    with pytest.raises(ValueError, match=">= 2 expected"):
        ops.backward_warp(img, coords[..., :1, :])
    for bad in (v.to(torch.uint8), v[..., :-1], v[0]):
        with pytest.raises(ValueError, match="valid must be a bool tensor"):
            ops.backward_warp(img, coords, bad)
    for bad in (1.0, 2.5, -1, 256, True, "0"):
        with pytest.raises(ValueError, match=r"fill must be an integer in \[0, 255\]"):
            ops.backward_warp(u8, coords, fill=bad)
    assert int(ops.backward_warp(u8, coords * 0 - 1, fill=np.uint8(255))[0].min()) == 255
    assert torch.isnan(ops.backward_warp(img, coords * 0 - 1, fill=float("nan"))[0]).all()
    good = (torch.empty(1, 3, H, W), torch.empty(1, 1, H, W, dtype=torch.bool))
    for out, match in (((good[0],), "out must be"), ((good[0].to(torch.uint8), good[1]), "out warped"),
                       ((good[0][:, :2], good[1]), "out warped"), ((good[0], good[1].to(torch.uint8)), "out ok"),
                       ((good[0].transpose(2, 3).contiguous().transpose(2, 3), good[1]), "out warped")):
        with pytest.raises(ValueError, match=match):
            ops.backward_warp(img, coords, out=out)
    # no kernel, no quiet run on another device
    with pytest.raises(NotImplementedError, match="no HIP kernel yet"):
        ops.backward_warp(img.to("meta"), coords.to("meta"))
    with pytest.raises(ValueError, match="same device"):
        ops.backward_warp(img, coords.to("meta"))


# ------------------------------------------------------------------ the tracker
def _shifted(L, shift, fill):
    """L (C,H,W) moved by the integer (dx, dy): out[c] = L[c - shift] inside, fill elsewhere."""
    _, H, W = L.shape
    dx, dy = shift
    out = torch.full_like(L, fill)
    inside = torch.zeros(H, W, dtype=torch.bool)
    ys, xs = slice(max(dy, 0), H + min(dy, 0)), slice(max(dx, 0), W + min(dx, 0))
    yo, xo = slice(max(-dy, 0), H + min(-dy, 0)), slice(max(-dx, 0), W + min(-dx, 0))
    out[:, ys, xs] = L[:, yo, xo]
    inside[ys, xs] = True
    return out, inside


@pytest.mark.parametrize("deltas", [(1,), (1, 3, None)])
def test_tracker_stabilizes_and_warps_by_the_translation(deltas):
    H, W, T = 24, 40, 6
    dx, dy = 3, -2
    frames = D.frames(T, H, W)
    trk = DenseMultiFlowTracker(S.StubShift((float(dx), float(dy))), iters=2, deltas=deltas)
    g = torch.Generator().manual_seed(4)
    overlay = {"fp32": torch.randn(1, 4, H, W, generator=g),
               "uint8": torch.randint(0, 256, (1, 3, H, W), generator=g, dtype=torch.uint8)}
    fills = {"fp32": -0.5, "uint8": 7}
    for call in (lambda: trk.stabilize(), lambda: trk.stabilize(frames[0]), lambda: trk.warp_image(overlay["fp32"])):
        with pytest.raises(ValueError, match="needs a step first"):
            call()
    for t in range(T):
        trk.step(frames[t])
        if t == 3:
            trk.reanchor()  # pos stays indexed by frame 0: nothing changes for the two methods
        shift = (t * dx, t * dy)
        # frame t seen from frame 0: the frame moved back by the translation
        for image in (None, frames[t], frames[t].to(torch.uint8), overlay["fp32"]):
            src = frames[t] if image is None else image
            fill = 7 if src.dtype == torch.uint8 else -0.5
            stab, ok = trk.stabilize(image, fill=fill)
            want, inside = _shifted(src[0], (-shift[0], -shift[1]), fill)
            assert stab.dtype == src.dtype and stab.shape == src.shape and ok.shape == (1, 1, H, W)
            assert torch.equal(ok[0, 0], inside) and torch.equal(ok, trk.visible), t
            assert torch.equal(stab[0], want), t
            assert stab.data_ptr() != src.data_ptr()
        # an image of frame 0 carried into frame t: moved by the translation
        for name, img in overlay.items():
            for fp in S.FOOTPRINTS:
                moved, ok = trk.warp_image(img, footprint=fp, fill=fills[name])
                want, inside = _shifted(img[0], shift, fills[name])
                assert moved.dtype == img.dtype and torch.equal(ok[0, 0], inside), (t, name, fp)
                assert torch.equal(moved[0], want), (t, name, fp)
                assert torch.equal(ok, trk.splat(None, footprint=fp)[1])
            # the rigid extension of an in-painted cell reads the image where it is inside
            moved, ok = trk.warp_image(img, inpaint=None, fill=fills[name])
            inv = trk.splat(None, inpaint=None)[2]
            _same((moved, ok), reference.backward_warp(img, inv, None, fills[name]), (t, name, "inpaint"))
            assert bool(ok[0, 0][inside].all())
        if t == 0:
            assert bool(ok.all())
            stab, ok = trk.stabilize()
            assert torch.equal(stab, frames[0]) and bool(ok.all())
    assert trk.anchor_frame == 3 and not bool(trk.visible.all()) and bool(trk.visible.any())
    for bad in (torch.zeros(H, W), torch.zeros(1, 3, H, W + 1), torch.zeros(2, 1, H, W), torch.zeros(1, 0, H, W)):
        for call in (trk.stabilize, trk.warp_image):
            with pytest.raises(ValueError, match=r"image must be \(1,C,H,W\)"):
                call(bad)
    with pytest.raises(ValueError, match="float32 or uint8"):
        trk.stabilize(torch.zeros(1, 1, H, W, dtype=torch.int32))
    # track() is what it was
    flows, vis = DenseMultiFlowTracker(trk.model, iters=2, deltas=deltas).track(frames)
    assert flows.shape == (T, 2, H, W) and vis.shape == (T, 1, H, W)


# --------------------------------------------------------------------- track.py
@pytest.fixture(scope="module")
def cli():
    sys.path.insert(0, ROOT)
    try:
        import track
    finally:
        sys.path.remove(ROOT)
    return track


def _files(d):
    return {f: open(os.path.join(d, f), "rb").read() for f in sorted(os.listdir(d))}


@pytest.mark.parametrize("channels", [1, 3, 4])
def test_track_cli_stabilize_and_overlay(cli, tmp_path, channels):
    """The three demo frames (436x1024, padded to 440x1024) through StubAny:
    frame t comes back by the stub's translation, the overlay moves with it."""
    from PIL import Image
    images = sorted(glob.glob(os.path.join(ROOT, "demo-frames", "*.png")))
    W, H = Image.open(images[0]).size
    assert H % 8 != 0  # the frames are padded
    g = np.random.default_rng(3)
    over = g.integers(0, 256, (H, W) if channels == 1 else (H, W, channels)).astype(np.uint8)
    Image.fromarray(over).save(tmp_path / "over.png")
    out = tmp_path / "dense"
    # one span: StubAny answers every pair with the same translation, whatever its span
    base = ["--dense", "--deltas", "1", "--iters", "2"]
    args = cli.parse_args(base + ["--stabilize", "--overlay", str(tmp_path / "over.png"), "--out", str(out)])
    cli.track_dense(args, D.StubAny(), images, None, torch.device("cpu"))
    dx, dy = (int(v) for v in S.STUB_D)
    chw = torch.from_numpy(over.reshape(H, W, channels)).permute(2, 0, 1)
    for t in range(3):
        stab = np.asarray(Image.open(out / f"stab_{t:04d}.png"))
        moved = np.asarray(Image.open(out / f"overlay_{t:04d}.png"))
        assert stab.shape == (H, W, 3) and stab.dtype == np.uint8
        assert moved.shape == over.shape and moved.dtype == np.uint8
        frame = torch.from_numpy(np.asarray(Image.open(images[t]))[..., :3].copy()).permute(2, 0, 1)
        want, inside = _shifted(frame, (-dx * t, -dy * t), 0)
        # a pixel next to the border may be followed into the padding, which repeats the border
        assert np.array_equal(stab[inside.numpy()], want.permute(1, 2, 0).numpy()[inside.numpy()])
        want, inside = _shifted(chw, (dx * t, dy * t), 0)
        got = torch.from_numpy(moved.reshape(H, W, channels).copy()).permute(2, 0, 1)
        assert torch.equal(got[:, inside], want[:, inside])
    assert np.array_equal(np.asarray(Image.open(out / "overlay_0000.png")), over)
    assert np.array_equal(np.asarray(Image.open(out / "stab_0000.png")), np.asarray(Image.open(images[0]))[..., :3])
    if channels != 3:
        return
    # without the two options: the other files, byte for byte, and nothing else
    out2 = tmp_path / "dense2"
    cli.track_dense(cli.parse_args(base + ["--out", str(out2)]), D.StubAny(), images, None, torch.device("cpu"))
    plain, full = _files(out2), _files(out)
    assert sorted(plain) == [f"{n}_{t:04d}.{e}" for n, e in (("flow", "flo"), ("visible", "png")) for t in range(3)]
    assert {k: v for k, v in full.items() if k in plain} == plain
    assert sorted(set(full) - set(plain)) == sorted(f"{n}_{t:04d}.png" for n in ("stab", "overlay") for t in range(3))
    for bad in (["--points", "p.txt", "--stabilize"], ["--points", "p.txt", "--overlay", "o.png"],
                base + ["--inpaint", "2"]):
        with pytest.raises(SystemExit):
            cli.parse_args(bad)
    assert cli.parse_args(base + ["--inpaint", "2", "--overlay", "o.png"]).inpaint == 2
    Image.fromarray(over[:-1]).save(tmp_path / "bad.png")
    args = cli.parse_args(base + ["--overlay", str(tmp_path / "bad.png"), "--out", str(out2)])
    with pytest.raises(ValueError, match="first frame's size"):
        cli.track_dense(args, D.StubAny(), images, None, torch.device("cpu"))

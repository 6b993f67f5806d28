"""Dense forward splatting on the GPU (csrc/forward_splat.hip): the scatter and
resolve kernels against the ATen oracle on the CPU, bit for bit, on the fields
of forward_splat_cases; repeatability; the op's host checks; the wrapper; graph
capture; DenseMultiFlowTracker.splat / warp_labels / track(labels=) on a GPU
tracker against a CPU tracker; and track.py --dense --labels on the GPU."""
import glob
import os
import sys

import numpy as np
import pytest
import torch

from raft_stir_amd import ops
from raft_stir_amd.export.denseflow import DenseMultiFlowTracker

import dense_flow_cases as D
import forward_splat_cases as S

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN = S.NAN
# S.SHAPES (2x2 the minimum, 7x9 odd, 24x70 = 1680 cells, no multiple of the block) and one whose rows are no
# multiple of the wave, in 17 blocks
SHAPES = S.SHAPES + [(33, 130)]
CASES = ((0, 0.0), (1, 0.0), (1, -7.5), (1, NAN), (3, 0.0), (3, -7.5), (3, NAN))  # (C, fill)


def _all_same(got, want, what):
    for name, g, w in zip(S.NAMES, got, want):
        if w is None:
            assert g is None, (what, name)
        else:
            assert g.device.type == "cuda", (what, name)
            g = g.cpu()
            assert g.dtype == w.dtype and g.shape == w.shape and S.same(g, w), (what, name, int((g != w).sum()))


def _splat(cuda, name, H, W, footprint, C=0, fill=0.0):
    pos, score = S.field(name, H, W)
    vals = S.values(C, H, W)
    return ops.forward_splat(pos.to(cuda), score.to(cuda), None if vals is None else vals.to(cuda),
                             footprint=footprint, fill=fill)


# ------------------------------------------------------------------ the kernels
@pytest.mark.parametrize("footprint", S.FOOTPRINTS)
@pytest.mark.parametrize("name", S.FIELDS)
@pytest.mark.parametrize("hw", SHAPES, ids=lambda hw: f"{hw[0]}x{hw[1]}")
def test_kernel_against_oracle(cuda, hw, name, footprint):
    H, W = hw
    for C, fill in CASES:
        got = _splat(cuda, name, H, W, footprint, C, fill)
        _all_same(got, S.expected(name, H, W, footprint, C, fill), (hw, name, footprint, C, fill))


@pytest.mark.parametrize("hw", [(24, 70), (33, 130)], ids=lambda hw: f"{hw[0]}x{hw[1]}")
def test_mixed_field_decides_cells_every_way(hw):
    """A condition on the inputs of test_kernel_against_oracle, from the oracle
    alone: the mixed field has cells decided by the score, by the index tie
    and by the class, and holes."""
    H, W = hw
    pos, score = S.field("mixed", H, W)
    for fp in S.FOOTPRINTS:
        n = S.outcome_counts(pos, score, fp)
        print(hw, fp, n)
        assert n["score"] >= 50 and n["tie"] >= 50 and n["holes"] >= 500, (fp, n)
        if fp == 2:
            assert n["class1"] >= 200, n


@pytest.mark.parametrize("hw", SHAPES, ids=lambda hw: f"{hw[0]}x{hw[1]}")
def test_named_fields(cuda, hw):
    H, W = hw
    N = H * W
    for fp in S.FOOTPRINTS:
        # all N sources contend for one cell
        src, cov, inv, out = _splat(cuda, "one_cell", H, W, fp, 1, -7.5)
        want = S.expected("one_cell", H, W, fp, 1, -7.5)
        cells = [(3, 2)] if fp == 1 else [(3, 2), (4, 2), (3, 3), (4, 3)]
        cells = [(x, y) for x, y in cells if x < W and y < H]
        exp = torch.full((H, W), -1, dtype=torch.int32)
        for x, y in cells:
            exp[y, x] = S.one_cell_winner(H, W)
        assert torch.equal(src[0, 0].cpu(), exp) and torch.equal(want[0][0, 0], exp)
        assert int(cov.sum()) == len(cells) and torch.equal(cov.cpu(), exp[None, None] >= 0)
        assert S.same(inv.cpu(), want[2]) and S.same(out.cpu(), want[3])
        # no source at all
        for fill in (-7.5, NAN):
            src, cov, inv, out = _splat(cuda, "none", H, W, fp, 3, fill)
            assert (src == -1).all() and not cov.any() and torch.isnan(inv).all()
            assert torch.isnan(out).all() if fill != fill else (out == fill).all()
        src, cov, inv, out = _splat(cuda, "identity", H, W, fp, 3, -7.5)
        assert torch.equal(src.flatten().cpu(), torch.arange(N, dtype=torch.int32)) and cov.all()
        assert torch.equal(inv.cpu(), S.field("identity", H, W)[0]) and torch.equal(out.cpu(), S.values(3, H, W))


# ----------------------------------------------- order independence, repeatability
def _raw(cuda, pos, score, vals, fp, fill, keys=None):
    """The op itself, on outputs filled with what no result holds and a
    workspace of the caller's."""
    _, _, H, W = pos.shape
    keys = torch.empty(H * W, dtype=torch.int64, device=cuda) if keys is None else keys
    src = torch.full((1, 1, H, W), -7, dtype=torch.int32, device=cuda)
    cov = torch.ones(1, 1, H, W, dtype=torch.bool, device=cuda)
    inv = torch.full((1, 2, H, W), 123.0, device=cuda)
    out = None if vals is None else torch.full_like(vals, 123.0)
    torch.ops.raft_stir.forward_splat(pos, score, vals, fp, fill, keys, src, cov, inv, out)
    return src, cov, inv, out


@pytest.mark.parametrize("footprint", S.FOOTPRINTS)
def test_repeatable_and_independent_of_what_ran_before(cuda, footprint):
    H, W = 33, 130
    pos, score = (t.to(cuda) for t in S.field("mixed", H, W))
    vals = S.values(3, H, W).to(cuda)
    want = S.expected("mixed", H, W, footprint, 3, -7.5)
    first = _raw(cuda, pos, score, vals, footprint, -7.5)
    second = _raw(cuda, pos, score, vals, footprint, -7.5)
    _all_same(first, want, "first")
    assert all(torch.equal(a.view(torch.uint8) if a.dtype == torch.bool else a.view(torch.int32),
                           b.view(torch.uint8) if b.dtype == torch.bool else b.view(torch.int32))
               for a, b in zip(first, second))
    # after another warm-up: other fields through the same workspace, which each leaves in another state,
    # and a workspace that starts as all zeros (below every key) or as small keys of class 0
    keys = torch.zeros(H * W, dtype=torch.int64, device=cuda)
    for warm in ("one_cell", "none", "identity"):
        p, s = (t.to(cuda) for t in S.field(warm, H, W))
        _raw(cuda, p, s, None, 3 - footprint, 0.0, keys)
        _all_same(_raw(cuda, pos, score, vals, footprint, -7.5, keys), want, warm)
    keys.copy_(torch.arange(H * W, device=cuda))
    _all_same(_raw(cuda, pos, score, vals, footprint, -7.5, keys), want, "arange")
    # the same scores and positions with the other planes of the call changed: the map does not move
    again = _raw(cuda, pos.clone(), score.clone(), (vals * 2).contiguous(), footprint, 0.0)
    assert all(S.same(a.cpu(), b) for a, b in zip(again[:3], want[:3]))


# ------------------------------------------------------------------- host checks
def test_host_checks(cuda):
    op = torch.ops.raft_stir.forward_splat
    H, W = 7, 9
    pos, score = (t.to(cuda) for t in S.field("mixed", H, W))
    vals = S.values(3, H, W).to(cuda)
    good = dict(pos=pos, score=score, values=vals, footprint=2, fill=0.0,
                keys=torch.empty(H * W, dtype=torch.int64, device=cuda),
                src_index=torch.empty(1, 1, H, W, dtype=torch.int32, device=cuda),
                covered=torch.empty(1, 1, H, W, dtype=torch.bool, device=cuda),
                inv_pos=torch.empty(1, 2, H, W, device=cuda), out=torch.empty(1, 3, H, W, device=cuda))
    order = ("pos", "score", "values", "footprint", "fill", "keys", "src_index", "covered", "inv_pos", "out")

    def call(**kw):
        a = dict(good, **kw)
        return op(*(a[k] for k in order))

    call()
    call(values=None, out=None)
    call(keys=torch.empty(1, 1, H, W, dtype=torch.int64, device=cuda))  # any shape of H*W elements
    # every output: a wrong dtype, a wrong shape
    bad = {"src_index": (good["src_index"].long(), good["src_index"][0]),
           "covered": (good["covered"].to(torch.uint8), good["covered"][..., :-1].contiguous()),
           "inv_pos": (good["inv_pos"].double(), good["inv_pos"][:, :1].contiguous()),
           "out": (good["out"].half(), good["out"][:, :2].contiguous())}
    for name, tensors in bad.items():
        for t in tensors:
            with pytest.raises(RuntimeError, match=name + " must be"):
                call(**{name: t})
    with pytest.raises(RuntimeError, match="inv_pos must be"):
        call(inv_pos=torch.empty(1, 2, W, H, device=cuda).transpose(2, 3))
    with pytest.raises(RuntimeError, match="pos must be a contiguous fp32"):
        call(pos=pos.transpose(2, 3).contiguous().transpose(2, 3))
    with pytest.raises(RuntimeError, match="pos must be a contiguous fp32"):
        call(pos=pos.double())
    with pytest.raises(RuntimeError, match=r"pos must be \(1,2,H,W\)"):
        call(pos=pos[0])
    with pytest.raises(RuntimeError, match="score must be"):
        call(score=score[0])
    with pytest.raises(RuntimeError, match="score must be"):
        call(score=score.half())
    with pytest.raises(RuntimeError, match="values must be"):
        call(values=vals[..., :-1].contiguous())
    with pytest.raises(RuntimeError, match="H, W >= 2"):
        call(pos=pos[..., :1].contiguous(), score=score[..., :1].contiguous())
    for keys in (torch.empty(H * W - 1, dtype=torch.int64, device=cuda),
                 torch.empty(H * W, dtype=torch.int32, device=cuda),
                 torch.empty(2 * H * W, dtype=torch.int64, device=cuda)[::2]):
        with pytest.raises(RuntimeError, match="keys must be"):
            call(keys=keys)
    for fp in (0, 3):
        with pytest.raises(RuntimeError, match="footprint must be 1 or 2"):
            call(footprint=fp)
    with pytest.raises(RuntimeError, match="out without values"):
        call(values=None)
    with pytest.raises(RuntimeError, match="values without out"):
        call(out=None)
    # an anchor index takes 31 bits of a key: one element expanded (the size is checked first)
    with pytest.raises(RuntimeError, match=r"below 2\^31"):
        call(pos=torch.zeros(1, device=cuda).expand(1, 2, 32768, 65536))
    # tensors on two devices
    for name in ("score", "values", "keys", "src_index", "covered", "inv_pos", "out"):
        with pytest.raises(RuntimeError, match="same device"):
            call(**{name: good[name].cpu()})
    # CPU tensors: the op has no CPU kernel, and a CPU pos is refused by name
    with pytest.raises(RuntimeError):
        call(**{k: v.cpu() for k, v in good.items() if isinstance(v, torch.Tensor)})
    with pytest.raises(RuntimeError, match="GPU tensors expected"):
        call(pos=pos.cpu())


# ---------------------------------------------------------------------- wrapper
def test_wrapper_converts_dtypes_and_layouts(cuda):
    H, W = 24, 70
    pos, score = (t.to(cuda) for t in S.field("mixed", H, W))
    vals = S.values(3, H, W).to(cuda)
    for fp in S.FOOTPRINTS:
        want = ops.forward_splat(pos, score, vals, footprint=fp, fill=-7.5)
        _all_same(want, S.expected("mixed", H, W, fp, 3, -7.5), fp)
        # fp32 -> fp64 -> fp32 is exact
        got = ops.forward_splat(pos.double(), score.double().transpose(2, 3).contiguous().transpose(2, 3),
                                vals.double().flip(1).contiguous().flip(1), footprint=fp, fill=-7.5)
        assert all(g.dtype == w.dtype and g.is_contiguous() and S.same(g.cpu(), w.cpu()) for g, w in zip(got, want))
        assert ops.forward_splat(pos, score, footprint=fp)[3] is None
    with pytest.raises(ValueError, match="same device"):
        ops.forward_splat(pos, score, vals.cpu())
    with pytest.raises(ValueError, match="same device"):
        ops.forward_splat(pos, score.cpu())
    with pytest.raises(ValueError, match="footprint must be 1 or 2"):
        ops.forward_splat(pos, score, footprint=3)


# ---------------------------------------------------------------------- capture
@pytest.mark.parametrize("footprint", S.FOOTPRINTS)
def test_op_is_graph_capturable(cuda, footprint):
    H, W = 24, 70
    vals = S.values(3, H, W).to(cuda)
    static = [t.to(cuda).clone() for t in S.field("identity", H, W)]
    s = torch.cuda.Stream(device=cuda)
    s.wait_stream(torch.cuda.current_stream(cuda))
    with torch.cuda.stream(s):
        ops.forward_splat(*static, vals, footprint=footprint, fill=-7.5)
    torch.cuda.current_stream(cuda).wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        outs = ops.forward_splat(*static, vals, footprint=footprint, fill=-7.5)
    seen = []
    for name in ("mixed", "none", "one_cell", "mixed"):
        ins = S.field(name, H, W)
        for dst, src in zip(static, ins):
            dst.copy_(src)
        g.replay()
        eager = ops.forward_splat(*(t.to(cuda) for t in ins), vals, footprint=footprint, fill=-7.5)
        assert all(S.same(a, e) for a, e in zip(outs, eager)), name
        _all_same(outs, S.expected(name, H, W, footprint, 3, -7.5), name)
        seen.append(outs[0].clone())
    assert (seen[1] == -1).all() and torch.equal(seen[0], seen[3]) and not torch.equal(seen[0], seen[2])
    assert static[0].is_cuda and g is not None  # the static inputs and the graph live to the end


# ---------------------------------------------------------------------- tracker
class StubShiftCached(S.StubShift):
    """S.StubShift with the two halves of the pass, for ``cache_features``:
    ``encode`` keeps the frame's index, ``refine`` forms the same translation
    from the indices of the two feature maps of every row."""

    def encode(self, image):
        f = (image[:, :1, ::8, ::8] * 0 + image[:, :1, :1, :1]).expand(-1, 8, -1, -1).contiguous()
        return f, f * 0 + 1

    def refine(self, fmap1, fmap2, ctx, iters=12, flow_init=None):
        span = fmap2[:, :1, :1, :1] - fmap1[:, :1, :1, :1]
        zero = (fmap1[:, :2] * 0 + 0 * (ctx[:, :2] - 1)).repeat_interleave(8, 2).repeat_interleave(8, 3)
        up = zero + span * self.d
        return up[..., ::8, ::8] / 8 + 0 * flow_init, up


STUB_HW = (64, 96)


def _labels(H, W):
    g = torch.Generator().manual_seed(3)
    labels = {"uint8": torch.randint(1, 255, (H, W), generator=g, dtype=torch.uint8),
              "int64": torch.randint(-2 ** 40, 2 ** 40, (1, 1, H, W), generator=g),
              "bool": torch.rand(1, 2, H, W, generator=g) < 0.5,
              "fp32": torch.randn(1, 3, H, W, generator=g)}
    return labels, {"uint8": 255, "int64": -1, "bool": True, "fp32": -0.5}


@pytest.mark.parametrize("cache_features", [False, True])
def test_tracker_splats_on_the_gpu(cuda, cache_features):
    """At every frame a GPU tracker's splat(), warp_labels() and
    track(frames, labels) equal a CPU tracker's, bit for bit; what they return
    is the caller's own, and the step graph stays the only graph."""
    H, W = STUB_HW
    frames = D.frames(9, H, W)
    f = frames.to(cuda)
    kw = dict(iters=2, deltas=(1, 3, None), cache_features=cache_features)
    make = StubShiftCached if cache_features else S.StubShift
    gpu, cpu = DenseMultiFlowTracker(make().to(cuda), **kw), DenseMultiFlowTracker(make(), **kw)
    labels, fills = _labels(H, W)
    on_gpu = {k: v.to(cuda) for k, v in labels.items()}
    static = lambda: {t.data_ptr() for t in (gpu.pos, gpu.score, gpu.visible)}  # noqa: E731
    kept, holes = [], False
    for t in range(len(frames)):
        gpu.step(f[t])
        cpu.step(frames[t])
        assert S.same(gpu.pos.cpu(), cpu.pos) and S.same(gpu.score.cpu(), cpu.score), t
        assert len(gpu.graphs) == 1
        # the results of frame t - 1: the step did not change them
        for got, snap, want in kept:
            assert all(S.same(a, b) and S.same(a.cpu(), c) for a, b, c in zip(got, snap, want)), t
        kept = []
        for fp in S.FOOTPRINTS:
            got = gpu.splat(on_gpu["fp32"], footprint=fp, fill=-0.5)
            want = cpu.splat(labels["fp32"], footprint=fp, fill=-0.5)
            _all_same(got, want, (t, fp))
            assert not {g.data_ptr() for g in got} & static()
            kept.append((got, [g.clone() for g in got], want))
            holes |= not bool(want[1].all())
            for name, lab in labels.items():
                w_cpu, c_cpu = cpu.warp_labels(lab, footprint=fp, fill=fills[name])
                # labels on the GPU and labels that the tracker moves there
                for given in (on_gpu[name], lab):
                    warped, cov = gpu.warp_labels(given, footprint=fp, fill=fills[name])
                    assert warped.is_cuda and cov.is_cuda and warped.dtype == lab.dtype and warped.shape == lab.shape
                    assert torch.equal(warped.cpu(), w_cpu) and torch.equal(cov.cpu(), c_cpu), (t, fp, name)
        assert gpu.splat()[3] is None and len(gpu.graphs) == 1
    assert holes
    for name in ("uint8", "fp32"):
        got = gpu.track(f, on_gpu[name], footprint=1, fill=fills[name])
        want = cpu.track(frames, labels[name], footprint=1, fill=fills[name])
        assert len(got) == 4 and all(g.is_cuda and g.dtype == w.dtype and S.same(g.cpu(), w) for g, w in zip(got, want))
        assert len(gpu.graphs) == 1
    plain = gpu.track(f)
    assert len(plain) == 2 and S.same(plain[0], got[0]) and torch.equal(plain[1], got[1])


# --------------------------------------------------------------------- track.py
def test_track_cli_labels_on_the_gpu(cuda, tmp_path):
    """track.py --dense --labels with the stub on the GPU writes the images
    that the oracle gives on the host from the tracker's pos and score."""
    from PIL import Image
    from raft_stir_amd.cli_common import load_image
    from raft_stir_amd.ops import reference
    from raft_stir_amd.utils.padder import InputPadder
    sys.path.insert(0, ROOT)
    try:
        import track
    finally:
        sys.path.remove(ROOT)
    images = sorted(glob.glob(os.path.join(ROOT, "demo-frames", "*.png")))
    Wi, Hi = Image.open(images[0]).size
    mask = np.random.default_rng(2).integers(1, 60000, (Hi, Wi)).astype(np.uint16)
    Image.fromarray(mask).save(tmp_path / "mask.png")
    out = tmp_path / "dense"
    args = track.parse_args(["--dense", "--deltas", "1", "--labels", str(tmp_path / "mask.png"), "--out", str(out),
                             "--iters", "2"])
    stub = D.StubAny().to(cuda)
    track.track_dense(args, stub, images, None, cuda)
    # the same tracker again, and what track.py did before: two copies to the host and the oracle there
    trk = DenseMultiFlowTracker(stub, iters=2, deltas=(1,))
    padder = InputPadder(load_image(images[0], cuda).shape)
    labels = torch.nn.functional.pad(torch.from_numpy(mask.astype(np.int32)), padder._pad, value=0)
    for t, name in enumerate(images):
        trk.step(padder.pad(load_image(name, cuda))[0])
        src, covered, _, _ = reference.forward_splat(trk.pos.cpu(), trk.score.cpu(), None, 2, 0.0)
        warped = labels.reshape(-1)[src[0, 0].long().clamp(min=0)]
        warped = torch.where(covered[0, 0], warped, torch.zeros_like(warped))
        warped = padder.unpad(warped).numpy().astype(mask.dtype)
        lab = np.asarray(Image.open(out / f"labels_{t:04d}.png"))
        cov = np.asarray(Image.open(out / f"covered_{t:04d}.png"))
        assert lab.dtype == mask.dtype and np.array_equal(lab, warped), t
        assert cov.dtype == np.uint8 and np.array_equal(cov, padder.unpad(covered)[0, 0].numpy().astype(np.uint8) * 255)
        assert t == 0 or (cov == 0).any()
    assert np.array_equal(np.asarray(Image.open(out / "labels_0000.png")), mask)

"""Hole in-painting on the GPU (csrc/splat_inpaint.hip): the column, row and
apply kernels against the ATen oracle on the CPU, bit for bit, on the maps of
splat_inpaint_cases; the row pass's segment boundary and its two ways to read
col; repeatability on a workspace of garbage; the op's host checks; the
wrapper; graph capture; ``inpaint=`` of a GPU tracker against a CPU tracker;
and track.py --inpaint on the GPU."""
import glob
import math
import os
import sys

import numpy as np
import pytest
import torch

from raft_stir_amd import ops
from raft_stir_amd.export.denseflow import DenseMultiFlowTracker
from raft_stir_amd.ops import reference

import dense_flow_cases as D
import forward_splat_cases as S
import splat_inpaint_cases as I

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN = I.NAN
SEG, STAGE = 256, 2048  # csrc/splat_inpaint.hip: cells of a row per block, cells of col a block stages in LDS
# I.SHAPES (2x2 the minimum, 7x9 odd, 24x70 = 1680 cells, no multiple of the block); 33x130, rows that are no multiple
# of the wave; 3 rows with R = 5, so that the column walk is bounded by H; 4 rows of a segment plus 5 cells
SHAPES = I.SHAPES + [(33, 130), (3, 9), (4, SEG + 5)]
CASES = ((0, 0.0), (1, NAN), (3, -7.5))  # (C, fill)


def _run(cuda, src, pos, inv, vals, R, fill):
    return ops.splat_inpaint(src.to(cuda), pos.to(cuda), inv.to(cuda), None if vals is None else vals.to(cuda),
                             max_dist=R, fill=fill)


# ------------------------------------------------------------------ the kernels
@pytest.mark.parametrize("name", I.MAPS)
@pytest.mark.parametrize("hw", SHAPES, ids=lambda hw: f"{hw[0]}x{hw[1]}")
def test_kernel_against_oracle(cuda, hw, name):
    H, W = hw
    src, pos, inv = (t.to(cuda) for t in I.case(name, H, W))
    for R in I.RADII:
        for C, fill in CASES:
            vals = I.values(C, H, W)
            got = ops.splat_inpaint(src, pos, inv, None if vals is None else vals.to(cuda), max_dist=R, fill=fill)
            I.all_same(got, I.expected(name, H, W, R, C, fill), (hw, name, R, C, fill), "cuda")


def _column_map(H, W, x_cov):
    """Only column x_cov is covered."""
    N = H * W
    src = torch.full((1, 1, H, W), -1, dtype=torch.int32)
    src[..., x_cov] = ((torch.arange(H) * W + x_cov) * 5 + 1).int() % N
    g = torch.Generator().manual_seed(x_cov)
    pos = reference.coords_grid(1, H, W) + torch.rand(1, 2, H, W, generator=g)
    inv = torch.where(src >= 0, torch.randn(1, 2, H, W, generator=g), torch.tensor(NAN))
    return src, pos, inv


@pytest.mark.parametrize("x_cov", [SEG - 2, SEG + 1], ids=["left_of", "right_of"])
def test_donors_across_the_segment_boundary(cuda, x_cov):
    """4 x (SEG + 5) with one covered column next to the boundary between the
    row pass's two blocks: the cells of the other block within R take it as
    donor, read from the part of the span beyond their own segment."""
    H, W = 4, SEG + 5
    src, pos, inv = _column_map(H, W, x_cov)
    xs = torch.arange(W)
    for R in (1, 2, 3, 5, None):
        Rn = I.radius(R, H, W)
        want = reference.splat_inpaint(src, pos, inv, I.values(3, H, W), Rn, -7.5)
        got = _run(cuda, src, pos, inv, I.values(3, H, W), R, -7.5)
        I.all_same(got, want, (x_cov, R), "cuda")
        donor = got[1].cpu()[0, 0]
        near = (xs - x_cov).abs() <= Rn
        assert torch.equal(donor >= 0, near.expand(H, W))
        assert torch.equal(donor[:, near], (torch.arange(H).view(H, 1) * W + x_cov).expand(H, int(near.sum())).int())
        other = (xs >= SEG) if x_cov < SEG else (xs < SEG)
        assert R == 1 or (near & other).any()


@pytest.mark.parametrize("name", ["mixed_fp2", "corners", "tie_row", "none_fp1", "bad_entries"])
def test_wide_rows_read_col_in_place(cuda, name):
    """2 x (STAGE + 52): with R = 5 a block's span of col fits the LDS tile; with
    R = 1000 and without a limit it is the whole row, wider than the tile, and
    the row pass reads col in place."""
    H, W = 2, STAGE + 52
    assert min(W, SEG + 2 * 5) <= STAGE < min(W, SEG + 2 * 1000)
    src, pos, inv = I.case(name, H, W)
    for R in (5, 1000, None):
        got = _run(cuda, src, pos, inv, I.values(1, H, W), R, -7.5)
        I.all_same(got, I.expected(name, H, W, R, 1, -7.5), (name, R), "cuda")


# ----------------------------------------------- repeatability, workspace of garbage
def _raw(cuda, src, pos, inv, vals, R, fill, col=None, junk=-7):
    """The op itself, on outputs filled with what no result holds and a workspace of the caller's."""
    _, _, H, W = src.shape
    col = torch.empty(H * W, dtype=torch.int32, device=cuda) if col is None else col
    donor, dist2, out_src = (torch.full((1, 1, H, W), junk, dtype=torch.int32, device=cuda) for _ in range(3))
    out_inv = torch.full((1, 2, H, W), 123.0, device=cuda)
    out = None if vals is None else torch.full_like(vals, 123.0)
    torch.ops.raft_stir.splat_inpaint(src, pos, inv, vals, R, fill, col, donor, dist2, out_src, out_inv, out)
    return out_src, donor, dist2, out_inv, out


@pytest.mark.parametrize("R", [2, 5, 130])
def test_repeatable_and_independent_of_what_ran_before(cuda, R):
    H, W = 33, 130
    name = "mixed_fp2"
    src, pos, inv = (t.to(cuda) for t in I.case(name, H, W))
    vals = I.values(3, H, W).to(cuda)
    want = I.expected(name, H, W, R, 3, -7.5)
    first = _raw(cuda, src, pos, inv, vals, R, -7.5)
    second = _raw(cuda, src, pos, inv, vals, R, -7.5)
    I.all_same(first, want, "first", "cuda")
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(first, second))
    # a workspace of garbage: rows far outside the image, negative ones, and what another map left there
    for junk in (2 ** 31 - 1, -2 ** 31, H, 0):
        col = torch.full((H * W,), junk, dtype=torch.int32, device=cuda)
        I.all_same(_raw(cuda, src, pos, inv, vals, R, -7.5, col, junk), want, junk, "cuda")
    col = torch.empty(H * W, dtype=torch.int32, device=cuda)
    for warm in ("none_fp1", "identity_fp1", "checker"):
        _raw(cuda, *(t.to(cuda) for t in I.case(warm, H, W)), None, 7 - min(R, 6), 0.0, col)
        I.all_same(_raw(cuda, src, pos, inv, vals, R, -7.5, col), want, warm, "cuda")


# ------------------------------------------------------------------- host checks
def test_host_checks(cuda):
    op = torch.ops.raft_stir.splat_inpaint
    H, W = 7, 9
    src, pos, inv = (t.to(cuda) for t in I.case("mixed_fp2", H, W))
    vals = I.values(3, H, W).to(cuda)
    ints = lambda: torch.empty(1, 1, H, W, dtype=torch.int32, device=cuda)  # noqa: E731
    good = dict(src_index=src, pos=pos, inv_pos_in=inv, values=vals, max_dist=2, fill=0.0,
                col=torch.empty(H * W, dtype=torch.int32, device=cuda), donor=ints(), dist2=ints(), src_out=ints(),
                inv_pos=torch.empty(1, 2, H, W, device=cuda), out=torch.empty(1, 3, H, W, device=cuda))
    order = ("src_index", "pos", "inv_pos_in", "values", "max_dist", "fill", "col", "donor", "dist2", "src_out",
             "inv_pos", "out")

    def call(**kw):
        a = dict(good, **kw)
        return op(*(a[k] for k in order))

    call()
    call(values=None, out=None)
    call(col=torch.empty(1, 1, H, W, dtype=torch.int32, device=cuda))  # any shape of H*W elements
    call(max_dist=0)
    call(max_dist=32767)
    bad = {"src_index": (src.long(), src[0]), "pos": (pos.double(), pos[:, :1].contiguous()),
           "inv_pos_in": (inv.half(), inv[..., :-1].contiguous()),
           "donor": (good["donor"].long(), good["donor"][0]), "dist2": (good["dist2"].short(), good["dist2"][0]),
           "src_out": (good["src_out"].long(), good["src_out"][..., :-1].contiguous()),
           "inv_pos": (good["inv_pos"].double(), good["inv_pos"][:, :1].contiguous()),
           "out": (good["out"].half(), good["out"][:, :2].contiguous())}
    for name, tensors in bad.items():
        for t in tensors:
            with pytest.raises(RuntimeError, match="splat_inpaint: " + name + " must be"):
                call(**{name: t})
    with pytest.raises(RuntimeError, match="pos must be a contiguous"):
        call(pos=pos.transpose(2, 3).contiguous().transpose(2, 3))
    with pytest.raises(RuntimeError, match="values must be"):
        call(values=vals[..., :-1].contiguous())
    with pytest.raises(RuntimeError, match="H, W in"):
        call(src_index=src[..., :1].contiguous())
    # an element expanded (the size is checked first)
    with pytest.raises(RuntimeError, match="H, W in"):
        call(src_index=torch.zeros(1, dtype=torch.int32, device=cuda).expand(1, 1, 2, 32768))
    for col in (torch.empty(H * W - 1, dtype=torch.int32, device=cuda),
                torch.empty(H * W, dtype=torch.int64, device=cuda),
                torch.empty(2 * H * W, dtype=torch.int32, device=cuda)[::2]):
        with pytest.raises(RuntimeError, match="col must be"):
            call(col=col)
    for R in (-1, 32768, 2 ** 40):
        with pytest.raises(RuntimeError, match="max_dist must be in"):
            call(max_dist=R)
    with pytest.raises(RuntimeError, match="out without values"):
        call(values=None)
    with pytest.raises(RuntimeError, match="values without out"):
        call(out=None)
    # outputs that share memory with what the passes still read
    for name in ("col", "donor", "dist2", "src_out"):
        with pytest.raises(RuntimeError, match="must not share memory with src_index"):
            call(**{name: src.view(-1) if name == "col" else src})
    with pytest.raises(RuntimeError, match="must not share memory with each other"):
        call(donor=good["dist2"])
    for other in (inv, pos):
        with pytest.raises(RuntimeError, match="inv_pos must not share memory"):
            call(inv_pos=other)
    with pytest.raises(RuntimeError, match="out must not share memory"):
        call(out=vals)
    for name in ("pos", "inv_pos_in", "values", "col", "donor", "dist2", "src_out", "inv_pos", "out"):
        with pytest.raises(RuntimeError, match="same device"):
            call(**{name: good[name].cpu()})
    with pytest.raises(RuntimeError):
        call(**{k: v.cpu() for k, v in good.items() if isinstance(v, torch.Tensor)})
    with pytest.raises(RuntimeError, match="GPU tensors expected"):
        call(src_index=src.cpu())


# ---------------------------------------------------------------------- wrapper
def test_wrapper_converts_dtypes_and_layouts(cuda):
    H, W = 24, 70
    src, pos, inv = (t.to(cuda) for t in I.case("bad_entries", H, W))
    vals = I.values(3, H, W).to(cuda)
    for R in (3, None):
        want = ops.splat_inpaint(src, pos, inv, vals, max_dist=R, fill=-7.5)
        I.all_same(want, I.expected("bad_entries", H, W, R, 3, -7.5), R, "cuda")
        # fp32 -> fp64 -> fp32 is exact; int64 entries beyond int32 are clamped as the rule reads them
        wide = src.long()
        assert int(wide[0, 0, 0, 3]) == H * W  # I.bad_entries
        wide[0, 0, 0, 3] = 2 ** 40
        got = ops.splat_inpaint(wide, pos.double(), inv.double().transpose(2, 3).contiguous().transpose(2, 3),
                                vals.double().flip(1).contiguous().flip(1),
                                max_dist=math.inf if R is None else R, fill=-7.5)
        assert all(g.dtype == w.dtype and g.is_contiguous() and I.same(g.cpu(), w.cpu()) for g, w in zip(got, want))
        assert ops.splat_inpaint(src, pos, inv, max_dist=R)[4] is None
    with pytest.raises(ValueError, match="same device"):
        ops.splat_inpaint(src, pos, inv, vals.cpu())
    with pytest.raises(ValueError, match="same device"):
        ops.splat_inpaint(src, pos.cpu(), inv)
    with pytest.raises(ValueError, match="max_dist must be in"):
        ops.splat_inpaint(src, pos, inv, max_dist=-1)


# ---------------------------------------------------------------------- capture
def test_op_is_graph_capturable(cuda):
    H, W = 24, 70
    R = 3
    vals = I.values(3, H, W).to(cuda)
    static = [t.to(cuda).clone() for t in I.case("identity_fp1", H, W)]
    s = torch.cuda.Stream(device=cuda)
    s.wait_stream(torch.cuda.current_stream(cuda))
    with torch.cuda.stream(s):
        ops.splat_inpaint(*static, vals, max_dist=R, fill=-7.5)
    torch.cuda.current_stream(cuda).wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        outs = ops.splat_inpaint(*static, vals, max_dist=R, fill=-7.5)
    seen = []
    for name in ("mixed_fp2", "none_fp1", "frame", "mixed_fp2"):
        ins = I.case(name, H, W)
        for dst, src in zip(static, ins):
            dst.copy_(src)
        g.replay()
        eager = ops.splat_inpaint(*(t.to(cuda) for t in ins), vals, max_dist=R, fill=-7.5)
        assert all(I.same(a, e) for a, e in zip(outs, eager)), name
        I.all_same(outs, I.expected(name, H, W, R, 3, -7.5), name, "cuda")
        seen.append(outs[0].clone())
    assert (seen[1] == -1).all() and torch.equal(seen[0], seen[3]) and not torch.equal(seen[0], seen[2])
    assert static[0].is_cuda and g is not None  # the static inputs and the graph live to the end


# ---------------------------------------------------------------------- tracker
def test_tracker_inpaints_on_the_gpu(cuda):
    """At every frame a GPU tracker's splat(), warp_labels() and track() with
    ``inpaint`` equal a CPU tracker's, bit for bit, and the step graph stays
    the only graph."""
    H, W = 64, 96
    frames = D.frames(6, H, W)
    f = frames.to(cuda)
    kw = dict(iters=2, deltas=(1, 3, None))
    gpu, cpu = DenseMultiFlowTracker(S.StubShift().to(cuda), **kw), DenseMultiFlowTracker(S.StubShift(), **kw)
    g = torch.Generator().manual_seed(3)
    labels = {"uint8": torch.randint(1, 255, (H, W), generator=g, dtype=torch.uint8),
              "int64": torch.randint(-2 ** 40, 2 ** 40, (1, 1, H, W), generator=g),
              "fp32": torch.randn(1, 3, H, W, generator=g)}
    fills = {"uint8": 255, "int64": -1, "fp32": -0.5}
    filled = False
    for t in range(len(frames)):
        gpu.step(f[t])
        cpu.step(frames[t])
        for fp, R in ((1, 2), (2, 3), (2, None)):
            got = gpu.splat(labels["fp32"], footprint=fp, fill=-0.5, inpaint=R)
            want = cpu.splat(labels["fp32"], footprint=fp, fill=-0.5, inpaint=R)
            assert len(got) == 4 and all(a.is_cuda and S.same(a.cpu(), b) for a, b in zip(got, want)), (t, fp, R)
            filled |= bool(((want[0] >= 0) & ~want[1]).any())
            for name, lab in labels.items():
                w_cpu, c_cpu = cpu.warp_labels(lab, footprint=fp, fill=fills[name], inpaint=R)
                warped, cov = gpu.warp_labels(lab, footprint=fp, fill=fills[name], inpaint=R)
                assert warped.is_cuda and warped.dtype == lab.dtype and warped.shape == lab.shape
                assert torch.equal(warped.cpu(), w_cpu) and torch.equal(cov.cpu(), c_cpu), (t, fp, R, name)
        assert len(gpu.graphs) == 1
    assert filled
    got = gpu.track(f, labels["uint8"].to(cuda), footprint=2, fill=255, inpaint=4)
    want = cpu.track(frames, labels["uint8"], footprint=2, fill=255, inpaint=4)
    assert len(got) == 4 and all(a.is_cuda and a.dtype == b.dtype and S.same(a.cpu(), b) for a, b in zip(got, want))
    plain = gpu.track(f, labels["uint8"].to(cuda), footprint=2, fill=255)
    assert not torch.equal(plain[2], got[2]) and torch.equal(plain[3], got[3]) and len(gpu.graphs) == 1


# --------------------------------------------------------------------- track.py
def test_track_cli_inpaint_on_the_gpu(cuda, tmp_path):
    """track.py --dense --labels --inpaint 2 with the stub on the GPU writes
    the files it writes on the CPU."""
    from PIL import Image
    sys.path.insert(0, ROOT)
    try:
        import track
    finally:
        sys.path.remove(ROOT)
    images = sorted(glob.glob(os.path.join(ROOT, "demo-frames", "*.png")))
    Wi, Hi = Image.open(images[0]).size
    mask = np.random.default_rng(2).integers(1, 60000, (Hi, Wi)).astype(np.uint16)
    Image.fromarray(mask).save(tmp_path / "mask.png")
    outs = {}
    for dev in ("cuda", "cpu"):
        outs[dev] = tmp_path / dev
        args = track.parse_args(["--dense", "--deltas", "1", "--labels", str(tmp_path / "mask.png"), "--out",
                                 str(outs[dev]), "--iters", "2", "--inpaint", "2"])
        device = cuda if dev == "cuda" else torch.device("cpu")
        track.track_dense(args, D.StubAny().to(device), images, None, device)
    for t in range(len(images)):
        for name in ("labels", "covered"):
            a, b = (np.asarray(Image.open(outs[dev] / f"{name}_{t:04d}.png")) for dev in ("cuda", "cpu"))
            assert a.dtype == b.dtype and np.array_equal(a, b), (t, name)
        assert t == 0 or set(np.unique(b)) == {0, 128, 255}

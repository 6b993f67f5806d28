"""The kernels of csrc/dense_compose.hip against the ATen oracle on the CPU,
bit for bit: the dense form on the fields of dense_compose_cases and on one of
several blocks plus a partial one, into buffers filled with garbage; the point
form at counts around the block size and at N = 0; the op's host checks; and
both forms under graph capture, replayed on changed inputs."""
import pytest
import torch

from raft_stir_amd import ops

import dense_compose_cases as C

pytestmark = pytest.mark.gpu

# C.SHAPES (2x2 the minimum, 7x9 odd, 24x70 = 1680 cells, no multiple of the block) and one of 16 blocks and a part
SHAPES = C.SHAPES + [(33, 130)]
COUNTS = (0, 1, 63, 64, 65, 300)
IDS = dict(ids=lambda hw: f"{hw[0]}x{hw[1]}")


def _garbage(cuda, H, W):
    return (torch.full((1, 2, H, W), 123.0, device=cuda), torch.full((1, 1, H, W), C.NAN, device=cuda),
            torch.ones(1, 1, H, W, dtype=torch.bool, device=cuda),
            torch.full((1, 1, H, W), -7, dtype=torch.int32, device=cuda), torch.full((1, 1, H, W), -3.0, device=cuda))


def _all_same(got, want, names, what):
    for name, g, w in zip(names, got, want):
        assert g.device.type == "cuda", (what, name)
        g = g.cpu()
        assert g.dtype == w.dtype and g.shape == w.shape and C.same(g, w), (what, name, int((g != w).sum()))


@pytest.mark.parametrize("base", C.BASES)
@pytest.mark.parametrize("inner", C.INNER)
@pytest.mark.parametrize("hw", SHAPES, **IDS)
def test_dense_kernel_against_oracle(cuda, hw, inner, base):
    H, W = hw
    args = [t.to(cuda) for t in C.base(base, H, W) + C.inner(inner, H, W)]
    want = C.expected(inner, base, H, W)
    _all_same(ops.dense_compose(*args), want, C.NAMES, "allocated")
    out = _garbage(cuda, H, W)
    back = ops.dense_compose(*args, out=out)
    assert all(b is o for b, o in zip(back, out))
    _all_same(out, want, C.NAMES, "out=")
    # visible is a bool of 0 or 1, whatever the buffer held
    assert int(out[2].view(torch.uint8).max()) <= 1


@pytest.mark.parametrize("N", COUNTS)
@pytest.mark.parametrize("hw", [(2, 2), (24, 70)], **IDS)
def test_point_kernel_against_oracle(cuda, hw, N):
    H, W = hw
    for inner in ("mixed", "ring"):
        pos, score, _, _ = (t.to(cuda) for t in C.inner(inner, H, W))
        got = ops.dense_query(pos, score, C.points_of("edge", H, W, N).to(cuda))
        assert got[0].shape == (1, N, 2) and got[1].shape == (1, N) and got[2].shape == (1, N)
        _all_same(got, C.expected_query(inner, "edge", H, W, N), C.QUERY_NAMES, (inner, N))
    # points that start at an odd float of their storage, and another float dtype
    if N:
        pts = C.points_of("smooth", H, W, N)
        odd = torch.cat([torch.zeros(1), pts.flatten()]).to(cuda)[1:].view(1, N, 2)
        _all_same(ops.dense_query(pos, score, odd), C.expected_query("ring", "smooth", H, W, N), C.QUERY_NAMES, "odd")
        _all_same(ops.dense_query(pos.double(), score, pts.double().to(cuda)),
                  C.expected_query("ring", "smooth", H, W, N), C.QUERY_NAMES, "fp64")


def test_wrapper_converts_dtypes_and_layouts(cuda):
    H, W = 24, 70
    b, i = [t.to(cuda) for t in C.base("edge", H, W)], [t.to(cuda) for t in C.inner("mixed", H, W)]
    want = C.expected("mixed", "edge", H, W)
    got = ops.dense_compose(b[0].double(), b[1].transpose(2, 3).contiguous().transpose(2, 3), i[0].double(), i[1],
                            i[2].transpose(2, 3).contiguous().transpose(2, 3), i[3].double())
    _all_same(got, want, C.NAMES, "converted")
    assert all(g.is_contiguous() for g in got)
    with pytest.raises(ValueError, match="same device"):
        ops.dense_compose(b[0].cpu(), *b[1:], *i)
    with pytest.raises(ValueError, match="same device"):
        ops.dense_query(i[0], i[1], torch.zeros(1, 3, 2))
    with pytest.raises(ValueError, match="out pos"):
        ops.dense_compose(*b, *i, out=tuple(t.cpu() for t in _garbage(cuda, H, W)))


def test_host_checks(cuda):
    H, W = 7, 9
    b, i = [t.to(cuda) for t in C.base("edge", H, W)], [t.to(cuda) for t in C.inner("mixed", H, W)]
    outs = list(_garbage(cuda, H, W))
    good = b + i + outs
    names = ("base_pos", "base_score", "pos", "score", "delta", "fb_err", "out pos", "out score", "out visible",
             "out delta", "out fb_err")
    op = torch.ops.raft_stir.dense_compose
    op(*good)
    for k, name in enumerate(names):
        t = good[k]
        wrong = [t.double() if t.dtype != torch.float64 and t.is_floating_point() else t.to(torch.int64),
                 t[..., :-1].contiguous(), t.transpose(2, 3).contiguous().transpose(2, 3)]
        if name == "pos":
            del wrong[1]  # the shape is read from pos: another tensor would be named
        for bad in wrong:
            with pytest.raises(RuntimeError, match=r"pos must be \(1,2,H,W\)|" + name + " must be"):
                op(*good[:k], bad, *good[k + 1:])
        if name != "pos":
            with pytest.raises(RuntimeError, match="same device"):
                op(*good[:k], t.cpu(), *good[k + 1:])
    with pytest.raises(RuntimeError, match="GPU tensors expected"):
        op(*good[:2], good[2].cpu(), *good[3:])
    with pytest.raises(RuntimeError, match="H, W >= 2"):
        op(*(t[..., :1].contiguous() for t in good))
    with pytest.raises(RuntimeError, match=r"below 2\^31"):
        op(*good[:2], torch.zeros(1, device=cuda).expand(1, 2, 32768, 65536), *good[3:])
    # an output that is an input
    with pytest.raises(RuntimeError, match="shares its storage"):
        op(*good[:6], good[2], *good[7:])
    with pytest.raises(RuntimeError, match="shares its storage"):
        op(*good[:9], good[4], good[10])
    q = torch.ops.raft_stir.dense_query
    pts = C.points_of("edge", H, W, 5).to(cuda)
    qo = [torch.empty(1, 5, 2, device=cuda), torch.empty(1, 5, dtype=torch.bool, device=cuda),
          torch.empty(1, 5, device=cuda)]
    q(i[0], i[1], pts, *qo)
    with pytest.raises(RuntimeError, match=r"points must be \(1,N,2\)"):
        q(i[0], i[1], pts[0], *qo)
    with pytest.raises(RuntimeError, match="points must be a contiguous"):
        q(i[0], i[1], pts.double(), *qo)
    with pytest.raises(RuntimeError, match="out positions must be"):
        q(i[0], i[1], pts, qo[0][:, :4].contiguous(), *qo[1:])
    with pytest.raises(RuntimeError, match="out visible must be"):
        q(i[0], i[1], pts, qo[0], qo[1].to(torch.uint8), qo[2])
    with pytest.raises(RuntimeError, match="out score must be"):
        q(i[0], i[1], pts, qo[0], qo[1], qo[2][:, :4].contiguous())
    with pytest.raises(RuntimeError, match="score must be"):
        q(i[0], i[1][0], pts, *qo)
    with pytest.raises(RuntimeError, match="same device"):
        q(i[0], i[1], pts.cpu(), *qo)


def test_ops_are_graph_capturable(cuda):
    H, W, N = 24, 70, 65
    first, others = ("identity", "integers"), [("mixed", "edge"), ("ring", "smooth"), ("mixed", "edge")]
    static = [t.to(cuda).clone() for t in C.base(first[1], H, W) + C.inner(first[0], H, W)]
    points = C.points_of(first[1], H, W, N).to(cuda).clone()
    out = _garbage(cuda, H, W)

    def run():
        ops.dense_compose(*static, out=out)
        return ops.dense_query(static[2], static[3], points)
    s = torch.cuda.Stream(device=cuda)
    s.wait_stream(torch.cuda.current_stream(cuda))
    with torch.cuda.stream(s):
        run()
    torch.cuda.current_stream(cuda).wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        queried = run()
    seen = []
    for inner, base in others:
        for dst, src in zip(static, C.base(base, H, W) + C.inner(inner, H, W)):
            dst.copy_(src)
        points.copy_(C.points_of(base, H, W, N))
        g.replay()
        _all_same(out, C.expected(inner, base, H, W), C.NAMES, (inner, base))
        _all_same(queried, C.expected_query(inner, base, H, W, N), C.QUERY_NAMES, (inner, base))
        seen.append(out[0].clone())
    assert C.same(seen[0], seen[2]) and not C.same(seen[0], seen[1])
    assert static[0].is_cuda and g is not None  # the static inputs and the graph live to the end

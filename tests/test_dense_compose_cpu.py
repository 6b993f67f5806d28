"""ops.reference.dense_compose (the rule of composing two dense track fields)
against a scalar brute force in fp32, bit for bit, on fields with lost pixels
and base positions on every kind of place; what the cases cover, asserted from
the rule; and the checks of ops.dense_compose / ops.dense_query on the CPU."""
import pytest
import torch

import dense_compose_cases as C

from raft_stir_amd import ops
from raft_stir_amd.ops import reference

IDS = dict(ids=lambda hw: f"{hw[0]}x{hw[1]}")


@pytest.mark.parametrize("base", C.BASES)
@pytest.mark.parametrize("inner", C.INNER)
@pytest.mark.parametrize("hw", C.SHAPES, **IDS)
def test_oracle_is_the_brute_force(hw, inner, base):
    H, W = hw
    got = C.expected(inner, base, H, W)
    want = C.brute_compose(*C.base(base, H, W), *C.inner(inner, H, W))
    for what, g, w in zip(C.NAMES, got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, what
        assert C.same(g, w), (what, int((~((g == w) | ((g != g) & (w != w)))).sum()))
    pos_c, score_c, vis_c, delta_c, err_c = got
    # the tracker's convention: a stored score is below +inf iff the pixel is visible
    assert torch.equal(score_c < C.INF, vis_c)
    assert torch.equal(delta_c[~vis_c], torch.full_like(delta_c[~vis_c], -1))
    assert bool((err_c[~vis_c] == C.INF).all())


@pytest.mark.parametrize("inner", C.INNER)
@pytest.mark.parametrize("hw", C.SHAPES, **IDS)
def test_an_integer_point_returns_the_stored_pixel(hw, inner):
    H, W = hw
    pos, score, delta, err = C.inner(inner, H, W)
    bp, _ = C.base("integers", H, W)
    pos_c, score_c, vis_c, delta_c, err_c = C.expected(inner, "integers", H, W)
    cell = (bp[0, 1].long() * W + bp[0, 0].long()).reshape(-1)
    for ch in range(2):
        stored = pos[0, ch].reshape(-1)[cell]
        got = pos_c[0, ch].reshape(-1)
        assert bool(((got == stored) | ((got != got) & (stored != stored))).all())  # 0 + -0 = +0: equal all the same
        nz = stored != 0
        assert C.same(got[nz], stored[nz])  # bit for bit
    s = score[0, 0].reshape(-1)[cell]
    assert torch.equal(vis_c.reshape(-1), s < C.INF)  # the base score is 0
    v = vis_c.reshape(-1)
    assert C.same(score_c.reshape(-1)[v], (s + 0.0)[v])
    assert torch.equal(delta_c.reshape(-1)[v], delta.reshape(-1)[cell][v])
    assert C.same(err_c.reshape(-1)[v], err.reshape(-1)[cell][v])


@pytest.mark.parametrize("case", C.ORDINARY, ids=lambda c: "-".join(c))
@pytest.mark.parametrize("hw", C.SHAPES, **IDS)
def test_ordinary_fields_are_not_mostly_holes(hw, case):
    H, W = hw
    vis = C.expected(*case, H, W)[2]
    assert int(vis.sum()) * 4 >= H * W, (int(vis.sum()), H * W)


@pytest.mark.parametrize("hw", C.SHAPES[1:], **IDS)
def test_the_cases_cover_what_they_claim(hw):
    """A NaN and a +inf score at a tap that is read and at a tap of weight 0,
    positions inside and outside, sums of two finite scores that overflow."""
    H, W = hw
    for inner in ("mixed", "ring"):
        got = C.tap_classes(inner, "edge", H, W)
        for key in ("inside", "outside", "nan_read", "inf_read", "nan_skipped", "inf_skipped", "overflow", "integer"):
            assert got[key] > 0, (inner, key, got)
    bp, bs = C.base("edge", H, W)
    n = H * W
    for j, (x, y) in enumerate(C.edge_points(H, W)):
        k = (j * 37 + 5) % n
        want = torch.tensor([x, y])
        assert C.same(torch.stack([bp[0, 0].view(n)[k], bp[0, 1].view(n)[k]]), want), (j, x, y)
    assert bool(torch.isnan(bs).any()) and bool((bs == C.INF).any()) and bool((bs == C.DENORMAL).any())


@pytest.mark.parametrize("hw", C.SHAPES, **IDS)
def test_outside_and_nonfinite_base_positions_come_back_unchanged(hw):
    H, W = hw
    bp, _ = C.base("edge", H, W)
    pos_c, score_c, vis_c, delta_c, err_c = C.expected("mixed", "edge", H, W)
    x, y = bp[0, 0], bp[0, 1]
    inside = (x >= 0) & (x <= W - 1) & (y >= 0) & (y <= H - 1)
    out = ~inside
    assert bool(out.any())
    assert C.same(pos_c[0, 0][out], x[out]) and C.same(pos_c[0, 1][out], y[out])
    assert not bool(vis_c[0, 0][out].any()) and bool((score_c[0, 0][out] == C.INF).all())


def test_a_nan_score_at_a_read_tap_is_not_dropped():
    """fmaxf would return the other operand: the rule keeps the NaN, and the pixel is not visible."""
    pos = reference.coords_grid(1, 2, 2).contiguous()
    score = torch.tensor([0.0, C.NAN, 0.0, 0.0]).view(1, 1, 2, 2)
    delta = torch.zeros(1, 1, 2, 2, dtype=torch.int32)
    err = torch.zeros(1, 1, 2, 2)
    bp = torch.tensor([[0.5, 0.0], [0.0, 0.5], [0.0, 1.0], [0.5, 0.5]]).t().reshape(1, 2, 2, 2).contiguous()
    bs = torch.zeros(1, 1, 2, 2)
    _, score_c, vis_c, delta_c, _ = reference.dense_compose(bp, bs, pos, score, delta, err)
    # (0.5, 0) reads pixels 0 and 1; (0, 0.5) pixels 0 and 2; (0, 1) pixel 2 only; (0.5, 0.5) all four
    assert vis_c.flatten().tolist() == [False, True, True, False]
    assert delta_c.flatten().tolist() == [-1, 0, 0, -1]
    assert bool((score_c.flatten()[[0, 3]] == C.INF).all())
    _, q_vis, q_score = reference.dense_query(pos, score, bp.reshape(1, 2, 4).transpose(1, 2))
    assert bool(torch.isnan(q_score[0, [0, 3]]).all()) and q_vis[0].tolist() == [False, True, True, False]


def test_the_wrappers_on_the_cpu_are_the_oracle_and_check_their_arguments():
    H, W = 7, 9
    b, i = C.base("edge", H, W), C.inner("mixed", H, W)
    want = C.expected("mixed", "edge", H, W)
    got = ops.dense_compose(*b, *i)
    outs = (torch.full((1, 2, H, W), 7.0), torch.full((1, 1, H, W), 7.0), torch.ones(1, 1, H, W, dtype=torch.bool),
            torch.full((1, 1, H, W), 7, dtype=torch.int32), torch.full((1, 1, H, W), 7.0))
    back = ops.dense_compose(*b, *i, out=outs)
    for what, g, o, r, w in zip(C.NAMES, got, outs, back, want):
        assert C.same(g, w) and C.same(o, w) and r is o, what
    # any float dtype or layout
    got = ops.dense_compose(b[0].double(), b[1], i[0].permute(0, 1, 3, 2).contiguous().permute(0, 1, 3, 2), *i[1:])
    assert all(C.same(g, w) for g, w in zip(got, want))
    for N in (0, 1, 65):
        pts = C.points_of("edge", H, W, N)
        got = ops.dense_query(i[0], i[1], pts)
        assert got[0].shape == (1, N, 2) and got[1].shape == (1, N) and got[2].shape == (1, N)
        assert all(C.same(g, w) for g, w in zip(got, C.expected_query("mixed", "edge", H, W, N)))
    with pytest.raises(ValueError, match="H, W >= 2"):
        ops.dense_compose(*(t[..., :1] for t in b), *(t[..., :1] for t in i))
    with pytest.raises(ValueError, match="H, W >= 2"):
        ops.dense_query(i[0][..., :1, :], i[1][..., :1, :], C.points_of("edge", H, W, 3))
    with pytest.raises(ValueError, match="base_pos and base_score"):
        ops.dense_compose(b[0][..., :-1], b[1], *i)
    with pytest.raises(ValueError, match="delta must be int32"):
        ops.dense_compose(*b, i[0], i[1], i[2].long(), i[3])
    with pytest.raises(ValueError, match=r"pos must be \(1,2,H,W\)"):
        ops.dense_compose(*b, i[0][0], *i[1:])
    with pytest.raises(ValueError, match="out visible"):
        ops.dense_compose(*b, *i, out=outs[:2] + (outs[1],) + outs[3:])
    with pytest.raises(ValueError, match="out must be"):
        ops.dense_compose(*b, *i, out=outs[:4])
    with pytest.raises(ValueError, match=r"points must be \(1,N,2\)"):
        ops.dense_query(i[0], i[1], torch.zeros(4, 2))
    assert "dense_compose" in ops.__all__ and "dense_query" in ops.__all__
    # no kernel, no quiet run on another device
    with pytest.raises(NotImplementedError, match="no HIP kernel yet"):
        ops.dense_compose(*(t.to("meta") for t in b + i))
    with pytest.raises(NotImplementedError, match="no HIP kernel yet"):
        ops.dense_query(i[0].to("meta"), i[1].to("meta"), torch.zeros(1, 3, 2, device="meta"))
    with pytest.raises(ValueError, match="below 2\\^31"):
        ops.dense_query(torch.zeros(1).expand(1, 2, 2 ** 16, 2 ** 15), torch.zeros(1).expand(1, 1, 2 ** 16, 2 ** 15),
                        torch.zeros(1, 1, 2))

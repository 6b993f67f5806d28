"""csrc/wpack.hip (op wpack_gather) vs the CPU oracle of tests/wpack_cases.py, bit for bit.

The kernel reads every source in place with its own strides, optionally takes
the low half v - bf16(v) of a split weight, multiplies by the scales of the output
ranges that contain the element and casts: each step is one fp32 operation or
exact, so every comparison here is equality of bits (NaN by isnan).

Direct calls: 1-D to 4-D sources, contiguous and channels_last, a bf16 source, a
dead table row, 63 sources (row 62); codes that cover every element of every
source, -1 entries, first and last elements, the lo flag on fp32 and bf16
sources; planted +-0, denormals, FLT_MAX, 0x3F7FFFFF, bf16 ties in both
directions, NaN, +-inf; no / one / four / overlapping / empty ranges with scales
0.25, -1, 0; bf16 and fp32 outputs; n = 0, 1, 255, 256, 257, every code once, and
8192 * 256 + 77 (the grid-stride loop runs a second pass).  The host refuses a
65-row table, five ranges and an output of another length before any launch.

Through the callers: ops/wpack.py (packed and packed_split views of
channels_last parameters, before and after a FusedClipAdamW step) and
models/fused_train.py pack (RAFT and RAFT-small, bf16 and fp32 engine) against
the reference branch of pack computed from the engine's own maps.
"""
import functools

import pytest
import torch

import wpack_cases as wc
from wpack_cases import BF16, F32

pytestmark = pytest.mark.gpu

BIG = 8192 * 256 + 77
SIZES = [0, 1, 255, 256, 257, None, BIG]  # None: every code of the base list once


@functools.lru_cache(maxsize=None)
def _sources(nrows):
    return wc.build_sources(nrows)


@functools.lru_cache(maxsize=None)
def _code(nrows, n):
    return wc.build_code(_sources(nrows)[1], n, seed=(n or 7) % 1000)


def _on(dev, nrows):
    src, _ = _sources(nrows)
    dsrc = [None if s is None else s.to(dev) for s in src]  # .to keeps the strides
    for s, d in zip(src, dsrc):
        assert s is None or s.stride() == d.stride()
    return dsrc, wc.table(dsrc).to(dev)


def _gather(dev, code, tab, ranges, dtype):
    """Into the middle of a NaN-filled buffer: returns the output and whether the margins are untouched."""
    n = code.numel()
    buf = torch.full((n + 16,), float("nan"), device=dev, dtype=dtype)
    out = buf[8:8 + n]
    torch.ops.raft_stir.wpack_gather(code.to(dev), tab, out, [a for a, _, _ in ranges], [b for _, b, _ in ranges],
                                     [s for _, _, s in ranges])
    return out.cpu(), bool(torch.isnan(buf[:8]).all() and torch.isnan(buf[8 + n:]).all())


@pytest.mark.parametrize("dtype", [BF16, F32], ids=["bf16", "f32"])
@pytest.mark.parametrize("n", SIZES, ids=lambda n: "all" if n is None else str(n))
def test_wpack_gather_bits(cuda, n, dtype):
    src, _ = _sources(10)
    dsrc, tab = _on(cuda, 10)
    code = _code(10, n)
    names = ("none", "four") if n == BIG else ("none", "one", "four", "overlap")
    for name in names:
        ranges = wc.ranges_for(code.numel())[name]
        got, clean = _gather(cuda, code, tab, ranges, dtype)
        want = wc.gather_oracle(code, src, ranges, dtype)
        assert clean, (name, "wrote outside the output")
        assert wc.same_bits(got, want), (name, int((got.float() != want.float()).sum()))


@pytest.mark.parametrize("dtype", [BF16, F32], ids=["bf16", "f32"])
def test_wpack_gather_63_sources(cuda, dtype):
    src, numel = _sources(63)
    assert len(src) == 63
    dsrc, tab = _on(cuda, 63)
    code = _code(63, None)
    assert int(((code[code >= 0].long() >> 24) & 63).max()) == 62
    ranges = wc.ranges_for(code.numel())["overlap"]
    got, clean = _gather(cuda, code, tab, ranges, dtype)
    assert clean and wc.same_bits(got, wc.gather_oracle(code, src, ranges, dtype))


def test_wpack_gather_planted_values_reach_the_output(cuda):
    """The oracle itself on the planted values: what the bit comparison above rests on."""
    src, _ = _sources(10)
    k = len(wc.PLANTED)
    code = torch.cat([(1 << 24) | torch.arange(k), (1 << 24) | torch.arange(k) | wc.LO,
                      (8 << 24) | torch.arange(k) | wc.LO, (9 << 24) | torch.arange(3)]).to(torch.int32)
    want = wc.gather_oracle(code, src, [], BF16)
    pl = torch.tensor(wc.PLANTED)
    assert wc.same_bits(want[:k], pl.to(BF16))
    assert torch.isinf(want[6]) and want[8].item() == 1.0  # FLT_MAX -> inf, 0x3F7FFFFF -> 1.0
    assert want[9].view(torch.int16).item() == 0x3F80 and want[10].view(torch.int16).item() == 0x3F82  # ties to even
    lo = want[k:2 * k]
    assert lo[6].item() == float("-inf") and bool(torch.isnan(lo[15:18]).all())  # FLT_MAX - inf, inf - inf
    fin = torch.isfinite(src[8].reshape(-1)[:k].float())
    assert bool((want[2 * k:3 * k][fin] == 0).all())  # lo of a bf16 source: 0 (inf - inf where FLT_MAX became inf)
    assert bool((want[3 * k:] == 0).all())            # dead row
    dsrc, tab = _on(cuda, 10)
    got, clean = _gather(cuda, code, tab, [], BF16)
    assert clean and wc.same_bits(got, want)


def test_wpack_gather_host_checks(cuda):
    dsrc, tab = _on(cuda, 10)
    code = _code(10, 257).to(cuda)
    out = torch.empty(257, device=cuda, dtype=BF16)
    G = torch.ops.raft_stir.wpack_gather
    G(code, tab, out, [], [], [])
    tab64 = torch.zeros(64, 10, dtype=torch.int64, device=cuda)
    tab64[:10] = tab
    G(code, tab64, out, [], [], [])  # 64 rows: what (code >> 24) & 63 can name
    with pytest.raises(RuntimeError, match="tab"):
        G(code, torch.zeros(65, 10, dtype=torch.int64, device=cuda), out, [], [], [])
    with pytest.raises(RuntimeError, match="ranges"):
        G(code, tab, out, [0] * 5, [1] * 5, [1.0] * 5)
    with pytest.raises(RuntimeError, match="ranges"):
        G(code, tab, out, [0], [1, 2], [1.0])
    with pytest.raises(RuntimeError, match="size"):
        G(code, tab, torch.empty(256, device=cuda, dtype=BF16), [], [], [])
    torch.cuda.synchronize()


# ------------------------------------------------------------------ through the callers
def test_wpack_views_follow_a_fused_adamw_step(cuda):
    from raft_stir_amd.ops import wpack
    from raft_stir_amd.ops.conv import pack_weight, pad_to, split_weight
    from raft_stir_amd.train.optim import FusedClipAdamW
    torch.manual_seed(0)
    cl = torch.channels_last
    w1 = torch.nn.Parameter(torch.randn(96, 64, 3, 3, device=cuda).contiguous(memory_format=cl))
    w2 = torch.nn.Parameter(torch.randn(96, 64, 1, 1, device=cuda).contiguous(memory_format=cl))
    lay1 = lambda ws: pack_weight(ws[0], [(64, [(0, 64, 0)])], pad_to(96, 128), torch.float32)  # noqa: E731
    lay2 = lambda ws: pack_weight(torch.cat([ws[0][:, :, 1:2, 1:2], ws[1]], 0).transpose(0, 1),  # noqa: E731
                                  [(192, [(0, 192, 0)])], 128, torch.float32)
    opt = FusedClipAdamW([w1, w2], lr=0.5, weight_decay=0.0)
    old = None
    for step in range(2):
        a = wpack.packed(("gpu_t1", id(w1), id(w2)), [w1, w2], lay2)
        b = wpack.packed_split(("gpu_t2", id(w1)), [w1], lay1)
        want_a = lay2([w1.detach().float(), w2.detach().float()]).to(BF16)
        want_b = split_weight(lay1([w1.detach().float()]))
        assert a.dtype == BF16 and b.dtype == BF16
        assert wc.same_bits(a.cpu(), want_a.cpu()) and wc.same_bits(b.cpu(), want_b.cpu())
        if old is not None:  # the step moved the weights, and the views with them
            assert not torch.equal(a, old[0]) and not torch.equal(b, old[1])
        old = (a.clone(), b.clone())
        w1.grad = torch.randn(w1.shape, device=cuda).contiguous(memory_format=cl)
        w2.grad = torch.randn(w2.shape, device=cuda).contiguous(memory_format=cl)
        opt.clip_and_step(1.0)


@pytest.mark.parametrize("mixed", [True, False], ids=["bf16", "fp32"])
@pytest.mark.parametrize("small", [False, True], ids=["raft", "raft_small"])
def test_fused_train_pack_equals_its_reference_branch(cuda, small, mixed):
    from raft_stir_amd.config import make_args
    from raft_stir_amd.models import RAFT
    from raft_stir_amd.models.fused_train import FusedTrainEngine
    torch.manual_seed(3)
    model = RAFT(make_args(mixed_precision=mixed, small=small)).to(cuda).to(memory_format=torch.channels_last)
    eng = FusedTrainEngine(model)
    eng.pack(cuda)
    M = eng._maps
    nbf = M["nbf"]
    src = torch.cat([p.detach().reshape(-1).float() for p in eng.params] + [M["zero"]])
    v = src.index_select(0, M["gather"])
    for a, b, s in M["scaled"]:
        v[a:b].mul_(s)
    want_bf = v[:nbf] if eng.f32 else v[:nbf].to(BF16)
    assert any(p.dim() == 4 and not p.is_contiguous() for p in eng.params)  # channels_last sources are read in place
    assert M["out_bf"].dtype == (F32 if eng.f32 else BF16) and M["out_f32"].dtype == F32
    assert wc.same_bits(M["out_bf"].cpu(), want_bf.cpu())
    assert wc.same_bits(M["out_f32"].cpu(), v[nbf:].cpu())
    assert bool((want_bf != 0).any()) and (small or len(M["scaled"]) > 0)

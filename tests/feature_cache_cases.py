"""Inputs shared by tests/test_feature_cache_cpu.py and
tests/test_feature_cache_gpu.py (not a test module): the feature ring's inputs
and index rows, the stub model with an encode / refine pair, the tolerance of
the cached trackers against the uncached ones and the sequence they run on."""
import torch

import multi_flow_cases as M

TOL = 2e-3  # the project's tolerance for the same mathematics on different kernels (tests/test_fb_check_gpu.py)

# ------------------------------------------------------------- feature ring op
RING_HW = [(1, 1), (3, 5), (16, 20)]  # one vector per image, a block tail, the trackers' test shape
RING_C = [(128, 160), (256, 256)]     # RAFT-small and RAFT: fnet, hidden + context
RING_K = [1, 3, 16]
RING_R = [2, 18]
NAMES = ("ring_f", "ring_c", "x", "ctx")


def ring_inputs(R, K, h, w, C, Cc, dtype, seed=0):
    """(ring_f, ring_c, f_new, c_new, x, ctx): random values that are exact in
    bf16 (multiples of 1/8 below 16), so that one set serves both dtypes; x and
    ctx start from a value the op never writes."""
    g = torch.Generator().manual_seed(1000 * R + 10 * K + h + seed)

    def rnd(*shape):
        return (torch.randint(-127, 128, shape, generator=g).float() / 8).to(dtype)

    return (rnd(R, h, w, C), rnd(R, h, w, Cc), rnd(1, h, w, C), rnd(1, h, w, Cc),
            torch.full((3 * K, h, w, C), 99.0, dtype=dtype), torch.full((2 * K, h, w, Cc), 99.0, dtype=dtype))


def ring_index_rows(R, K):
    """[(name, [src_0 .. src_{K-1}, dst])]: every source the same row; the
    sources walking down from the anchor row R-1; every source the row written
    (the new features must come out); an index of -1 and one of R (they clamp
    to 0 and R-1), the second as dst too."""
    rows = [("repeated", [0] * K + [R - 1]),
            ("anchor", [(R - 1 - k) % R for k in range(K)] + [0]),
            ("src_is_dst", [R - 1] * K + [R - 1]),
            ("below_range", [-1] + [k % R for k in range(1, K)] + [R - 1]),
            ("above_range", [R] + [k % R for k in range(1, K)] + [0]),
            ("dst_above_range", [k % R for k in range(K)] + [R + 5])]
    return [(n, torch.tensor(r, dtype=torch.int32)) for n, r in rows]


def ring_expected(ring_f, ring_c, f_new, c_new, idx, K):
    """The rule written out with Python indices, clamped: what the oracle and
    the kernel must both give."""
    R = ring_f.shape[0]
    i = [min(max(int(v), 0), R - 1) for v in idx]
    src, dst = i[:K], i[K]
    rf, rc = ring_f.clone(), ring_c.clone()
    rf[dst], rc[dst] = f_new[0], c_new[0]
    x = torch.stack([rf[s] for s in src] + [f_new[0]] * K + [rf[s] for s in src])
    ctx = torch.stack([rc[s] for s in src] + [c_new[0]] * K)
    return rf, rc, x, ctx


# ------------------------------------------------------------------ stub model
STUB_C = 8  # 32 bytes of fp32 per pixel: whole 16-byte vectors


class StubSpanCached(M.StubSpanFlow):
    """StubSpanFlow with the two halves of the pass.  ``encode`` returns
    (B,8,h,w) features that hold the frame's index and a constant context;
    ``refine`` forms StubSpanFlow's fields from the indices of the two feature
    maps of every row: a row whose second frame is the later one is a forward
    field, the others are backward fields.  ``forward`` is built from the same
    two halves, so that it serves a SequenceTracker without fb_check too.
    ``calls`` counts all three."""

    def encode(self, image):
        self.calls += 1
        return self._encode(image)

    def _encode(self, image):
        t = image[:, :1, :1, :1]
        f = (image[:, :1, ::8, ::8] * 0 + t).expand(-1, STUB_C, -1, -1).contiguous()
        return f, f * 0 + 1

    def refine(self, fmap1, fmap2, ctx, iters=12, flow_init=None):
        self.calls += 1
        return self._refine(fmap1, fmap2, ctx, flow_init)

    def _refine(self, fmap1, fmap2, ctx, flow_init):
        assert fmap1.shape == fmap2.shape and ctx.shape[0] == fmap1.shape[0] == flow_init.shape[0]
        t1, t2 = fmap1[:, :1, :1, :1], fmap2[:, :1, :1, :1]  # (B',1,1,1)

        def occluded(t):
            return ((t == M.SC_OCCLUDED[0]) | (t == M.SC_OCCLUDED[1])).to(fmap1.dtype)

        fwd = (t2 > t1).to(fmap1.dtype)
        up = self.drift * 0 + (t2 - t1) * self.d + fwd * occluded(t2) * self.drift + (1 - fwd) * occluded(t1) * self.off
        up = up + 0 * (ctx[:, :1, :1, :1] - 1)
        return up[..., ::8, ::8] / 8 + 0 * flow_init, up

    def forward(self, image1, image2, iters=12, flow_init=None, test_mode=False, bidirectional=False):
        assert test_mode
        self.calls += 1
        (f1, c1), (f2, c2) = self._encode(image1), self._encode(image2)
        if bidirectional:
            f1, f2, c1 = torch.cat([f1, f2]), torch.cat([f2, f1]), torch.cat([c1, c2])
        return self._refine(f1, f2, c1, flow_init)


# ------------------------------------------------------ real model: tolerance
def batch_sensitivity(model, a, b, others):
    """d0: how far the existing forward's flow_up of the pair (a, b) moves when
    the encoders run it as row 0 of a batch of 3 instead of alone, both
    directions, zero init.  ``others``: two more (1,3,H,W) images."""
    with torch.no_grad():
        _, one = model(a, b, iters=4, test_mode=True, bidirectional=True)
        i1 = torch.cat([a, others[0], others[1]])
        i2 = torch.cat([b, others[1], others[0]])
        _, three = model(i1, i2, iters=4, test_mode=True, bidirectional=True)
    return max((one[0] - three[0]).abs().max().item(), (one[1] - three[3]).abs().max().item())


def tolerance(d0):
    """rtol, atol for flows whose encoders ran at another batch size: the
    project's TOL, or twice the sensitivity measured on one small sample."""
    return dict(rtol=TOL, atol=max(TOL, 2 * d0))


def images(n, seed=7, H=128, W=160):
    g = torch.Generator().manual_seed(seed)
    return [torch.rand(1, 3, H, W, generator=g) * 255 for _ in range(n)]


def sequence(T=6, N=16, seed=5, H=128, W=160):
    g = torch.Generator().manual_seed(seed)
    frames = torch.rand(T, 1, 3, H, W, generator=g) * 255
    points = torch.rand(1, N, 2, generator=g) * torch.tensor([W - 1.0, H - 1.0])
    return frames, points

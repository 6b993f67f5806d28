"""Sources, codes and the CPU oracle for the packed-weight gather (csrc/wpack.hip,
op wpack_gather); used by tests/test_wpack_gather_gpu.py.

code[i] = (lo << 30) | (row << 24) | li, li a logical row-major index into the
source of table row `row`; code < 0 and a dead row (null pointer) give 0.  The
value is read as fp32, `lo` takes v - bf16(v), every output range that contains
i multiplies by its scale in fp32, in order, and the result is cast to the output
dtype with round-to-nearest-even.  Each step is one fp32 operation or exact, so
the oracle (torch indexing on the CPU) is to be met bit for bit.
"""
import struct

import torch

LO = 1 << 30
F32, BF16 = torch.float32, torch.bfloat16


def _f(bits):
    return struct.unpack("<f", struct.pack("<I", bits))[0]


# +-0, fp32 denormals, FLT_MAX (rounds to inf in bf16), 0x3F7FFFFF (the carry runs into the
# exponent), exact bf16 halves for both directions of ties-to-even (and their negatives), NaN, +-inf
PLANTED = [0.0, -0.0, _f(0x00000001), _f(0x80000001), _f(0x00012345), _f(0x007FFFFF), _f(0x7F7FFFFF), _f(0xFF7FFFFF),
           _f(0x3F7FFFFF), _f(0x3F808000), _f(0x3F818000), _f(0xBF808000), _f(0xBF818000), _f(0x3F808001),
           _f(0x3F807FFF), float("nan"), float("inf"), float("-inf")]


def build_sources(nrows=10, seed=0):
    """CPU sources in table-row order (None: a dead row and its element count).
    Rows 0..9 are the shapes of the issue; further rows are 3-element vectors up
    to `nrows` (63: row 62 is used)."""
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g)
    cl = torch.channels_last
    src = [rn(37), rn(129, 70), rn(4, 5, 6), rn(24, 17, 3, 3), rn(24, 17, 3, 3).contiguous(memory_format=cl),
           rn(8, 5, 1, 7).contiguous(memory_format=cl), rn(1, 1, 1, 4099).contiguous(memory_format=cl),
           rn(4099, 1, 1, 1).contiguous(memory_format=cl), rn(16, 9).to(BF16), None]
    numel = [s.numel() if s is not None else 11 for s in src]
    pl = torch.tensor(PLANTED)
    for r in (0, 1, 4, 5):  # planted at the start of a 1-D, a 2-D and two channels_last sources
        flat = src[r].contiguous().reshape(-1).clone()  # logical order
        flat[:pl.numel()] = pl
        t = flat.view(src[r].shape)
        src[r] = t.contiguous(memory_format=cl) if r in (4, 5) else t
    b = src[8].reshape(-1).clone()
    b[:pl.numel()] = pl.to(BF16)
    src[8] = b.view(16, 9)
    while len(src) < nrows:
        src.append(rn(3))
        numel.append(3)
    return src, numel


def table(dev_sources):
    """int64 [rows][10] = (data_ptr, is_bf16, size[4] padded with leading 1, stride[4] padded with 0)."""
    rows = []
    for w in dev_sources:
        if w is None:
            rows.append([0] * 10)
            continue
        pad = 4 - w.dim()
        rows.append([w.data_ptr(), int(w.dtype == BF16)] + [1] * pad + list(w.shape) + [0] * pad + list(w.stride()))
    return torch.tensor(rows, dtype=torch.int64)


def build_code(numel, n, seed=0):
    """n valid codes.  The base list holds a random permutation of every element of
    every source, the first and last element of every source plain and with the
    lo flag, the planted values with the lo flag, and -1 entries; a random third
    of it carries the lo flag.  n below its length takes a shuffled part of it,
    n above repeats it."""
    g = torch.Generator().manual_seed(seed)
    every = torch.cat([(r << 24) | torch.arange(k) for r, k in enumerate(numel)])
    ends = torch.tensor([(r << 24) | i for r, k in enumerate(numel) for i in (0, k - 1)])
    planted = torch.cat([(r << 24) | torch.arange(len(PLANTED)) for r in (0, 1, 4, 5, 8)])
    perm = every[torch.randperm(every.numel(), generator=g)]
    perm = torch.where(torch.rand(perm.numel(), generator=g) < 1 / 3, perm | LO, perm)
    base = torch.cat([perm, ends, ends | LO, planted, planted | LO, torch.full((7,), -1)])
    if n is None:
        n = base.numel()
    if n < base.numel():
        base = base[torch.randperm(base.numel(), generator=g)]
    reps = -(-n // base.numel()) if n else 1
    code = base.repeat(reps)[:n]
    if n > 2:
        code[n // 2] = -1
    return code.to(torch.int32)


def ranges_for(n):
    """name -> [(lo, hi, scale)]: none, one, four (an empty one, one ending at n, scales 0.25 / -1 / 0), two that overlap."""
    return {
        "none": [],
        "one": [(n // 3, 2 * n // 3, 0.25)],
        "four": [(0, n // 4, 0.25), (n // 4, n // 2, -1.0), (n // 2, n // 2, 7.0), (3 * n // 4, n, 0.0)],
        "overlap": [(0, 2 * n // 3, 0.25), (n // 3, n, -1.0)],
    }


def gather_oracle(code, sources, ranges, out_dtype):
    code = code.long()
    ok = code >= 0
    row, li = (code >> 24) & 63, code & 0xFFFFFF
    lo = ok & ((code >> 30) & 1).bool()
    v = torch.zeros(code.numel(), dtype=F32)
    for r, s in enumerate(sources):
        if s is None:
            continue
        sel = ok & (row == r)
        v[sel] = s.contiguous().reshape(-1)[li[sel]].float()  # logical row-major order
    v = torch.where(lo, v - v.to(BF16).float(), v)
    for a, b, sc in ranges:
        v[a:b] = v[a:b] * torch.tensor(sc, dtype=F32)
    return v.to(out_dtype)


def same_bits(got, want):
    """Equal bit for bit, NaN compared by isnan."""
    if got.dtype != want.dtype or got.shape != want.shape:
        return False
    nan = torch.isnan(want)
    if not torch.equal(torch.isnan(got), nan):
        return False
    it = torch.int16 if got.dtype == BF16 else torch.int32
    return torch.equal(got.contiguous().view(it)[~nan], want.contiguous().view(it)[~nan])

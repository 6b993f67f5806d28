"""The rule of csrc/query_device.h on the host, under AddressSanitizer and
UBSan: tests/host/dense_compose_host.cpp runs the dense and the point pass of
csrc/dense_compose.hip as plain loops over the fields of dense_compose_cases
(NaN, +-inf, 1e30, border and denormal inputs among them), as a child process
of its own with nothing preloaded.  Every output must equal the oracle's bit
for bit and the sanitizers must stay silent: the index arithmetic the kernels
inline is in bounds and defined before a GPU runs it."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest
import torch

import dense_compose_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "dense_compose_host.cpp")
CSRC = os.path.join(ROOT, "raft_stir_amd", "csrc")
# the runtimes linked statically: the program needs no libasan.so to be found, or to come first, when it starts
FLAGS = ["-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
         "-static-libasan", "-static-libubsan"]
POINTS = 65


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no g++")
    d = tmp_path_factory.mktemp("compose_host")
    probe = d / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    res = subprocess.run([cxx] + FLAGS + [str(probe), "-o", str(d / "probe")], capture_output=True, text=True)
    if res.returncode != 0:
        pytest.skip("g++ lacks the sanitizer runtimes: " + res.stderr.strip()[-300:])
    exe = d / "dense_compose_host"
    res = subprocess.run([cxx] + FLAGS + [f"-I{CSRC}", SRC, "-o", str(exe)], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    return str(exe)


def run(exe, tmp_path, base, inner, points):
    _, _, H, W = inner[0].shape
    HW, N = H * W, points.shape[1]
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(src, "wb") as f:
        f.write(struct.pack("<3i", H, W, N))
        for t, dt in ((base[0], "<f4"), (base[1], "<f4"), (inner[0], "<f4"), (inner[1], "<f4"), (inner[2], "<i4"),
                      (inner[3], "<f4"), (points, "<f4")):
            f.write(t.contiguous().numpy().astype(dt).tobytes())
    env = {k: v for k, v in os.environ.items() if k not in ("ASAN_OPTIONS", "UBSAN_OPTIONS")}
    res = subprocess.run([exe, str(src), str(dst)], capture_output=True, text=True, env=env, timeout=60)
    assert res.returncode == 0 and res.stderr == "", (res.returncode, res.stderr[-2000:])
    raw = open(dst, "rb").read()
    assert len(raw) == HW * (8 + 4 + 1 + 4 + 4) + N * (8 + 1 + 4)

    def take(dt, n, at):
        return torch.from_numpy(np.frombuffer(raw, dt, n, at).copy())

    vis = take(np.uint8, HW, 12 * HW)
    at = 21 * HW
    qvis = take(np.uint8, N, at + 8 * N)
    assert int(vis.max()) <= 1 and (N == 0 or int(qvis.max()) <= 1)
    dense = (take("<f4", 2 * HW, 0).view(1, 2, H, W), take("<f4", HW, 8 * HW).view(1, 1, H, W),
             vis.bool().view(1, 1, H, W), take("<i4", HW, 13 * HW).view(1, 1, H, W),
             take("<f4", HW, 17 * HW).view(1, 1, H, W))
    point = (take("<f4", 2 * N, at).view(1, N, 2), qvis.bool().view(1, N), take("<f4", N, at + 9 * N).view(1, N))
    return dense, point


@pytest.mark.parametrize("base", C.BASES)
@pytest.mark.parametrize("inner", C.INNER)
@pytest.mark.parametrize("hw", C.SHAPES, ids=lambda hw: f"{hw[0]}x{hw[1]}")
def test_host_rule_is_the_oracle_and_sanitizer_clean(program, tmp_path, hw, inner, base):
    H, W = hw
    dense, point = run(program, tmp_path, C.base(base, H, W), C.inner(inner, H, W), C.points_of(base, H, W, POINTS))
    for what, g, w in zip(C.NAMES, dense, C.expected(inner, base, H, W)):
        assert g.dtype == w.dtype and g.shape == w.shape and C.same(g, w), (what, int((g != w).sum()))
    for what, g, w in zip(C.QUERY_NAMES, point, C.expected_query(inner, base, H, W, POINTS)):
        assert g.dtype == w.dtype and g.shape == w.shape and C.same(g, w), (what, int((g != w).sum()))


def test_host_rule_without_points(program, tmp_path):
    H, W = 7, 9
    dense, point = run(program, tmp_path, C.base("edge", H, W), C.inner("mixed", H, W), C.points_of("edge", H, W, 0))
    assert all(C.same(g, w) for g, w in zip(dense, C.expected("mixed", "edge", H, W)))
    assert point[0].shape == (1, 0, 2)

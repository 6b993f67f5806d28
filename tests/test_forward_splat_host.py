"""The forward-splatting rule of csrc/splat_device.h on the host, under
AddressSanitizer and UBSan: tests/host/forward_splat_host.cpp runs the scatter
and the resolve pass of csrc/forward_splat.hip as plain loops over the fields
of forward_splat_cases (NaN, +-inf, 1e30, border and denormal inputs among
them), as a child process of its own with nothing preloaded.  Every output
must equal the oracle's bit for bit and the sanitizers must stay silent: the
index arithmetic the kernels inline is in bounds and defined before a GPU
runs it."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest
import torch

import forward_splat_cases as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "forward_splat_host.cpp")
CSRC = os.path.join(ROOT, "raft_stir_amd", "csrc")
# the runtimes linked statically: the program needs no libasan.so to be found, or to come first, when it starts
FLAGS = ["-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
         "-static-libasan", "-static-libubsan"]


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no g++")
    d = tmp_path_factory.mktemp("splat_host")
    probe = d / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    res = subprocess.run([cxx] + FLAGS + [str(probe), "-o", str(d / "probe")], capture_output=True, text=True)
    if res.returncode != 0:
        pytest.skip("g++ lacks the sanitizer runtimes: " + res.stderr.strip()[-300:])
    exe = d / "forward_splat_host"
    res = subprocess.run([cxx] + FLAGS + [f"-I{CSRC}", SRC, "-o", str(exe)], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    return str(exe)


def run(exe, tmp_path, pos, score, values, footprint, fill):
    _, _, H, W = pos.shape
    N = H * W
    C = 0 if values is None else values.shape[1]
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(src, "wb") as f:
        f.write(struct.pack("<4if", H, W, footprint, C, fill))
        for t in (pos, score) + (() if values is None else (values,)):
            f.write(t.contiguous().numpy().astype("<f4").tobytes())
    env = {k: v for k, v in os.environ.items() if k not in ("ASAN_OPTIONS", "UBSAN_OPTIONS")}
    res = subprocess.run([exe, str(src), str(dst)], capture_output=True, text=True, env=env, timeout=60)
    assert res.returncode == 0 and res.stderr == "", (res.returncode, res.stderr[-2000:])
    raw = open(dst, "rb").read()
    assert len(raw) == N * (4 + 1 + 8 + 4 * C)
    src_index = torch.from_numpy(np.frombuffer(raw, "<i4", N, 0).copy()).view(1, 1, H, W)
    covered = torch.from_numpy(np.frombuffer(raw, np.uint8, N, 4 * N).copy())
    assert int(covered.max()) <= 1
    inv = torch.from_numpy(np.frombuffer(raw, "<f4", 2 * N, 5 * N).copy()).view(1, 2, H, W)
    out = torch.from_numpy(np.frombuffer(raw, "<f4", C * N, 13 * N).copy()).view(1, C, H, W) if C else None
    return src_index, covered.bool().view(1, 1, H, W), inv, out


@pytest.mark.parametrize("C", (0, 3))
@pytest.mark.parametrize("footprint", S.FOOTPRINTS)
@pytest.mark.parametrize("name", S.FIELDS)
@pytest.mark.parametrize("hw", S.SHAPES, ids=lambda hw: f"{hw[0]}x{hw[1]}")
def test_host_rule_is_the_oracle_and_sanitizer_clean(program, tmp_path, hw, name, footprint, C):
    H, W = hw
    fill = -7.5
    pos, score = S.field(name, H, W)
    got = run(program, tmp_path, pos, score, S.values(C, H, W), footprint, fill)
    want = S.expected(name, H, W, footprint, C, fill)
    for what, g, w in zip(S.NAMES, got, want):
        if w is None:
            assert g is None, what
        else:
            assert g.dtype == w.dtype and g.shape == w.shape and S.same(g, w), (what, int((g != w).sum()))

"""The in-painting rule of csrc/inpaint_device.h on the host, under
AddressSanitizer and UBSan: tests/host/splat_inpaint_host.cpp runs the column,
row and apply pass of csrc/splat_inpaint.hip as plain loops over the maps of
splat_inpaint_cases (entries outside [-1, N-1] among them), as a child process
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

import splat_inpaint_cases as I

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "splat_inpaint_host.cpp")
CSRC = os.path.join(ROOT, "raft_stir_amd", "csrc")
# the runtimes linked statically: the program needs no libasan.so to be found, or to come first, when it starts
FLAGS = ["-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
         "-static-libasan", "-static-libubsan"]
# the maps' shapes, and one wider than the row pass's segment of 256 cells with a span that is clipped on both sides
SHAPES = I.SHAPES + [(3, 300)]


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no g++")
    d = tmp_path_factory.mktemp("inpaint_host")
    probe = d / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    res = subprocess.run([cxx] + FLAGS + [str(probe), "-o", str(d / "probe")], capture_output=True, text=True)
    if res.returncode != 0:
        pytest.skip("g++ lacks the sanitizer runtimes: " + res.stderr.strip()[-300:])
    exe = d / "splat_inpaint_host"
    res = subprocess.run([cxx] + FLAGS + [f"-I{CSRC}", SRC, "-o", str(exe)], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    return str(exe)


def run(exe, tmp_path, src, pos, inv, values, R, fill):
    _, _, H, W = src.shape
    N = H * W
    C = 0 if values is None else values.shape[1]
    fin, fout = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(fin, "wb") as f:
        f.write(struct.pack("<4if", H, W, R, C, fill))
        f.write(src.contiguous().numpy().astype("<i4").tobytes())
        for t in (pos, inv) + (() if values is None else (values,)):
            f.write(t.contiguous().numpy().astype("<f4").tobytes())
    env = {k: v for k, v in os.environ.items() if k not in ("ASAN_OPTIONS", "UBSAN_OPTIONS")}
    res = subprocess.run([exe, str(fin), str(fout)], capture_output=True, text=True, env=env, timeout=60)
    assert res.returncode == 0 and res.stderr == "", (res.returncode, res.stderr[-2000:])
    raw = open(fout, "rb").read()
    assert len(raw) == N * 4 * (3 + 2 + C)
    ints = [torch.from_numpy(np.frombuffer(raw, "<i4", N, 4 * N * k).copy()).view(1, 1, H, W) for k in range(3)]
    inv_out = torch.from_numpy(np.frombuffer(raw, "<f4", 2 * N, 12 * N).copy()).view(1, 2, H, W)
    out = torch.from_numpy(np.frombuffer(raw, "<f4", C * N, 20 * N).copy()).view(1, C, H, W) if C else None
    return (*ints, inv_out, out)


@pytest.mark.parametrize("name", I.MAPS)
@pytest.mark.parametrize("hw", SHAPES, ids=lambda hw: f"{hw[0]}x{hw[1]}")
def test_host_rule_is_the_oracle_and_sanitizer_clean(program, tmp_path, hw, name):
    H, W = hw
    src, pos, inv = I.case(name, H, W)
    for R in I.RADII:
        for C, fill in ((0, 0.0), (3, -7.5)):
            got = run(program, tmp_path, src, pos, inv, I.values(C, H, W), I.radius(R, H, W), fill)
            I.all_same(got, I.expected(name, H, W, R, C, fill), (hw, name, R, C))

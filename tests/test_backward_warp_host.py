"""The rule of csrc/warp_device.h on the host, under AddressSanitizer and
UBSan: tests/host/backward_warp_host.cpp runs the pass of
csrc/backward_warp.hip as a plain loop over the cases of backward_warp_cases
(NaN, +-inf, 1e30, border and denormal positions among them), for both dtypes,
planar and channels-last images and the packed forms of three and four channels, as a
child process of its own with nothing preloaded.  Every output must equal the
oracle's bit for bit and the sanitizers must stay silent: the index arithmetic
the kernel inlines is in bounds and defined before a GPU runs it."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest
import torch

import backward_warp_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "backward_warp_host.cpp")
CSRC = os.path.join(ROOT, "raft_stir_amd", "csrc")
# the runtimes linked statically: the program needs no libasan.so to be found, or to come first, when it starts
FLAGS = ["-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
         "-static-libasan", "-static-libubsan"]
PACKED = 10  # the program's exit status when it took the packed form


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no g++")
    d = tmp_path_factory.mktemp("warp_host")
    probe = d / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    res = subprocess.run([cxx] + FLAGS + [str(probe), "-o", str(d / "probe")], capture_output=True, text=True)
    if res.returncode != 0:
        pytest.skip("g++ lacks the sanitizer runtimes: " + res.stderr.strip()[-300:])
    exe = d / "backward_warp_host"
    res = subprocess.run([cxx] + FLAGS + [f"-I{CSRC}", SRC, "-o", str(exe)], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    return str(exe)


def run(exe, tmp_path, image, coords, valid, fill, channels_last):
    _, ch, Hs, Ws = image.shape
    _, _, H, W = coords.shape
    u8 = image.dtype == torch.uint8
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    mem = image.permute(0, 2, 3, 1) if channels_last else image  # the layout's memory order
    with open(src, "wb") as f:
        f.write(struct.pack("<9if", int(u8), int(channels_last), ch, Hs, Ws, H, W, int(valid is not None),
                            int(fill) if u8 else 0, 0.0 if u8 else float(fill)))
        f.write(mem.contiguous().numpy().tobytes())
        f.write(coords.contiguous().numpy().astype("<f4").tobytes())
        if valid is not None:
            f.write(valid.contiguous().numpy().astype(np.uint8).tobytes())
    env = {k: v for k, v in os.environ.items() if k not in ("ASAN_OPTIONS", "UBSAN_OPTIONS")}
    res = subprocess.run([exe, str(src), str(dst)], capture_output=True, text=True, env=env, timeout=60)
    assert res.returncode in (0, PACKED) and res.stderr == "", (res.returncode, res.stderr[-2000:])
    raw = open(dst, "rb").read()
    size = 1 if u8 else 4
    assert len(raw) == H * W * (ch * size + 1)
    warped = torch.from_numpy(np.frombuffer(raw, np.uint8 if u8 else "<f4", ch * H * W, 0).copy())
    ok = torch.from_numpy(np.frombuffer(raw, np.uint8, H * W, ch * H * W * size).copy())
    assert int(ok.max()) <= 1
    return (warped.view(1, ch, H, W), ok.bool().view(1, 1, H, W)), res.returncode == PACKED


@pytest.mark.parametrize("case", C.all_cases(), ids=C.case_id)
def test_host_rule_is_the_oracle_and_sanitizer_clean(program, tmp_path, case):
    dt, im, size, fname = case
    (H, W), (Hs, Ws) = C.SIZES[size]
    coords = C.field(fname, H, W, Hs, Ws)
    for ch in C.CHANNELS:
        for channels_last in (False, True):
            with_valid = bool((ch + channels_last) % 2)
            got, packed = run(program, tmp_path, C.image(im, dt, ch, Hs, Ws), coords,
                              C.valid(H, W) if with_valid else None, C.FILL[dt], channels_last)
            assert packed == (ch in (3, 4) and channels_last)
            for what, g, w in zip(("warped", "ok"), got, C.expected(im, dt, ch, size, fname, with_valid)):
                assert g.dtype == w.dtype and g.shape == w.shape and C.same(g, w), (ch, channels_last, what,
                                                                                    int((g != w).sum()))


@pytest.mark.parametrize("dt", ["fp32", "uint8"])
def test_host_rule_with_sixteen_channels(program, tmp_path, dt):
    (H, W), (Hs, Ws) = C.SIZES[2]
    im = C.IMAGES[dt][2]
    for channels_last in (False, True):
        got, packed = run(program, tmp_path, C.image(im, dt, 16, Hs, Ws), C.field("edge", H, W, Hs, Ws),
                          C.valid(H, W), C.FILL[dt], channels_last)
        assert not packed
        assert all(C.same(g, w) for g, w in zip(got, C.expected(im, dt, 16, 2, "edge", True)))

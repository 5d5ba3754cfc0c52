"""csrc/noise_walk.hpp -- which slabs of the split lazy covariance's noise term cov_noise_beam_kernel walks (the full ones) and how cov_noise_tail_kernel packs the half
slabs two to a slab (cov.hip) -- checked on the host: tests/noise_walk_host.cpp (plain C++, its own main, no HIP and no library) enumerates, for every K in 8 .. 4096, the
(slab, sample slot) -> (row, Philox slot, half) map of both kernels and requires every row k < K exactly once and no row >= K, and that the step counts the beam-sum's
schedule (beam_stream.hpp) is handed are the main kernel's.  Built once plainly and once with the address + undefined-behaviour sanitizers; both are run directly."""
from __future__ import annotations

import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = "5g_based_system_level_integrated_sensing_and_communication_simulator_amd"


@pytest.mark.parametrize("flags", [(), ("-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g")], ids=["plain", "asan_ubsan"])
def test_noise_walk_header_on_the_host(tmp_path, flags):
    gxx = shutil.which("g++")
    assert gxx, "no host C++ compiler"
    exe = str(tmp_path / "noise_walk_host")
    cmd = [gxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", *flags, "-I", os.path.join(ROOT, PKG, "csrc"),
           os.path.join(ROOT, "tests", "noise_walk_host.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    print(r.stdout.strip())
    assert "noise_walk:" in r.stdout and "checks OK" in r.stdout
    assert "K 3276 L 224 A 64: 192 full + 26 half slabs per column (13 packed); main 512 workgroups x 84 steps, 3584 of 3584 units beside the slabs" in r.stdout   # the bench shape

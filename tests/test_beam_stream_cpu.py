"""csrc/beam_stream.hpp -- how cov_noise_beam_kernel (cov.hip) spreads the beam-sum's antenna loads over its slab steps -- checked on the host: tests/beam_stream_host.cpp
(plain C++, its own main, no HIP and no library) walks every workgroup of the shapes of tests/test_gpu_lazy_split.py and of the bench shape (K = 3276, L = 224) at 49 / 56 / 64
antennas the way the kernel does and requires that every (unit, sample, antenna) is loaded exactly once, that a unit started beside the slabs is also stored there, and that no
load is issued in a workgroup's last step.  Built once plainly and once with the address + undefined-behaviour sanitizers; both are run directly."""
from __future__ import annotations

import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = "5g_based_system_level_integrated_sensing_and_communication_simulator_amd"


@pytest.mark.parametrize("flags", [(), ("-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g")], ids=["plain", "asan_ubsan"])
def test_beam_stream_header_on_the_host(tmp_path, flags):
    gxx = shutil.which("g++")
    assert gxx, "no host C++ compiler"
    exe = str(tmp_path / "beam_stream_host")
    cmd = [gxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", *flags, "-I", os.path.join(ROOT, PKG, "csrc"),
           os.path.join(ROOT, "tests", "beam_stream_host.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    print(r.stdout.strip())
    assert "beam_stream:" in r.stdout and "checks OK" in r.stdout
    assert "K 3276 L 224 A 64: 3584 units" in r.stdout                       # the bench shape: 16 units per symbol

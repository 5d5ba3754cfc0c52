"""ISA-level checks of the split lazy covariance's kernels (no GPU: the gfx950 code objects of the freshly built objects, as tests/test_isa_cpu.py reads them).

cov_noise_beam_kernel<1|2> must keep what cov_lazy_kernel has -- two workgroups per CU (<= 256 registers, no scratch at one target, <= 32 B at two), the 2 x 30 MFMAs of its two slab steps per tile group with
no branch between them, the four Box-Muller transforms of a step between the MFMAs -- and load nothing of D: the only vector-memory loads of a step are the beam-sum's six.
echo_range_xc_kernel<1> must stay at four waves per SIMD (<= 128 registers) without scratch; it exists for one LoS target only: the two-target range kernel sits at exactly
128 registers and the cross term did not fit (csrc/echo.hip) -- cov_cross_kernel<2> forms it instead."""
from __future__ import annotations

import pytest

from test_isa_cpu import LLVM, CodeObject

import os

pytestmark = pytest.mark.skipif(not os.path.exists(os.path.join(LLVM, "llvm-objdump")), reason="ROCm LLVM tools not installed")


@pytest.fixture(scope="module")
def cov_co(tmp_path_factory):
    return CodeObject(str(tmp_path_factory.mktemp("isa_split_cov")), "cov")


@pytest.fixture(scope="module")
def echo_co(tmp_path_factory):
    return CodeObject(str(tmp_path_factory.mktemp("isa_split_echo")), "echo")


@pytest.mark.parametrize("q", [1, 2])
def test_noise_beam_kernel_shape(cov_co, q):
    name, meta, asm = cov_co.find("cov_noise_beam_kernel", f"ILi{q}E")
    assert meta["vgpr_count"] <= 256 and meta["agpr_count"] == 0, meta
    assert meta["private_segment_fixed_size"] <= (0 if q == 1 else 32), meta
    mf = [i for i, ln in enumerate(asm) if ln.startswith("v_mfma_f64_16x16x4")]
    assert len(mf) == 2 * 2 * 30, len(mf)                                  # two tile groups x two unrolled steps x 30
    for g in range(2):
        loop = asm[mf[60 * g]:mf[60 * g + 59] + 1]
        assert not any(ln.startswith(("s_cbranch", "s_branch")) for ln in loop), "a branch inside the MFMA stream"
    body = asm[mf[0]:mf[29] + 1]                                             # one slab step of one tile group
    assert sum(1 for ln in body if ln.startswith(("v_log_f32", "v_sin_f32", "v_cos_f32", "v_sqrt_f32"))) == 16, "four Box-Muller transforms (4 transcendentals each) per step"
    assert sum(1 for ln in body if ln.startswith("buffer_load_dwordx4")) == 6, "the six antenna loads of the beam-sum and no D load"
    assert not any(ln.startswith(("global_load", "flat_load")) for ln in body)
    assert sum(1 for ln in body if ln.startswith("buffer_store_dwordx4")) == q                 # the unit's beam-sums (dropped by the bounds check until the unit is complete)
    assert sum(1 for ln in body if ln.startswith("ds_write_b128") or ln.startswith("ds_write2_b64")) >= 4


@pytest.mark.parametrize("q", [1, 2])
def test_small_kernels_of_the_split_route_exist_without_scratch(cov_co, echo_co, q):
    for co, kern in ((cov_co, "cov_dgram_kernel"), (cov_co, "cov_assemble_kernel"), (echo_co, "coef_window_kernel")):
        name, meta, asm = co.find(kern, f"ILi{q}E")
        assert meta["private_segment_fixed_size"] == 0, (name, meta)
    name, meta, asm = cov_co.find("cov_cross_kernel", "ILi2E")                 # two targets only: one target's cross term is the range kernel's
    assert meta["private_segment_fixed_size"] == 0 and sum(1 for ln in asm if ln.startswith(("v_log_f32", "v_sin_f32", "v_cos_f32", "v_sqrt_f32"))) >= 8, meta


def test_cross_term_range_kernel_budget(echo_co):
    name, meta, asm = echo_co.find("echo_range_xc_kernel", "ILi1E")
    assert meta["vgpr_count"] <= 128 and meta["agpr_count"] == 0 and meta["private_segment_fixed_size"] == 0, meta
    assert not any(ln.startswith("buffer_store_dwordx4") for ln in asm), "the lazy form must not store the echo grid"
    assert sum(1 for ln in asm if ln.startswith("global_load_dwordx4")) >= 8 * 2               # txGrid + D loads of the eight elements

"""ISA-level checks of the noise generator's instruction diet in the two widest kernels of the lazy CPI (no GPU needed: the gfx950 code objects are
taken out of the freshly built objects, as in test_isa_cpu.py).

Both kernels are bound by vector-ALU issue, so their time follows the VALU instruction count and nothing numerical would notice if
an edit or a compiler update put the instructions back:
  * Philox's three-way xor is ONE v_bitop3_b32 (echo_dev.hpp xor3), not two v_xor_b32;
  * the straight-line fused kernel zero-pads the range-IFFT input through the padded window table, not through a select per element;
  * the beam-sum that also writes the coefficient vectors keeps the beam-sum's occupancy.
The counts are taken on the objects of the project's own build (-ffp-contract=on), where the parent commit has 1207 / 2431 vector-ALU instructions in the two kernels; the
totals asserted below (1105, 2120) were set from a compile with the default contraction (1184 / 2367 there) and are met on the real build all the same: 1089 and 2117.
"""
from __future__ import annotations

import pytest

from test_isa_cpu import CodeObject, pytestmark  # noqa: F401  (the same skip condition, the same code-object reader)


@pytest.fixture(scope="module")
def echo_co(tmp_path_factory):
    return CodeObject(str(tmp_path_factory.mktemp("isa_gen_echo")), "echo")


@pytest.fixture(scope="module")
def cov_co(tmp_path_factory):
    return CodeObject(str(tmp_path_factory.mktemp("isa_gen_cov")), "cov")


def count(asm, prefix):
    return sum(1 for ln in asm if ln.startswith(prefix))


def valu_count(asm):
    """Vector-ALU instructions: everything that is neither scalar (s_*), nor memory (global_/buffer_/ds_/scratch_/flat_), nor an MFMA."""
    return sum(1 for ln in asm if ln.startswith("v_") and not ln.startswith("v_mfma"))


@pytest.mark.parametrize("store", [0, 1])
def test_fused_kernel_generator_diet(echo_co, store):
    name, meta, asm = echo_co.find("echo_range_sl_kernel", f"ILi1ELi1ELb{store}ELi4E")
    x2, x3, sel = count(asm, "v_xor_b32"), count(asm, "v_bitop3_b32"), count(asm, "v_cndmask_b32")
    print(f"{name}: v_xor_b32 {x2}, v_bitop3_b32 {x3}, v_cndmask_b32 {sel}, VALU {valu_count(asm)}, VGPRs {meta['vgpr_count']}")
    assert x2 <= 8, x2                    # 140 with the two-instruction xor
    assert x3 >= 70, x3                   # 4 calls x 10 rounds x 2
    assert sel <= 8, sel                  # 32 with the per-element `k < K` select


def test_lazy_fused_kernel_valu_total(echo_co):
    name, meta, asm = echo_co.find("echo_range_sl_kernel", "ILi1ELi1ELb0ELi4E")
    n = valu_count(asm)
    print(f"{name}: VALU {n}")
    assert n <= 1105, n                   # 1207 on the parent's object


def test_lazy_covariance_kernel_generator_diet(cov_co):
    name, meta, asm = cov_co.find("cov_lazy_kernel", "ILi1E")
    x2, n = count(asm, "v_xor_b32"), valu_count(asm)
    print(f"{name}: v_xor_b32 {x2}, v_bitop3_b32 {count(asm, 'v_bitop3_b32')}, VALU {n}, VGPRs {meta['vgpr_count']}")
    assert x2 <= 16, x2                   # 592 before
    assert n <= 2120, n                   # 2431 on the parent's object


@pytest.mark.parametrize("q", [1, 2])
def test_beamsum_coef_kernel_keeps_the_beamsum_occupancy(echo_co, q):
    name, meta, asm = echo_co.find("beamsum_coef_kernel", f"ILi{q}ELi32E")
    _, ref, _ = echo_co.find("beamsum_kernel", f"ILi{q}ELi32E")
    print(f"{name}: VGPRs {meta['vgpr_count']} (beamsum_kernel<{q},32>: {ref['vgpr_count']})")
    assert meta["private_segment_fixed_size"] == 0 and meta["agpr_count"] == 0, meta
    assert meta["vgpr_count"] <= 128 and ref["vgpr_count"] <= 128, (meta, ref)      # the same occupancy step: four 256-thread workgroups per CU and more

"""ISA-level check of echo_range_xc_kernel<1>'s dead-column test (csrc/echo.hip; no GPU: the gfx950 code object of the freshly built object, as tests/test_isa_cpu.py
reads it).  The test has to stand IN FRONT of the generator, or a dead column still pays for its draws:
  * the kernel has an exit (s_endpgm) before its first transcendental instruction, i.e. before the first Box-Muller transform;
  * in front of that exit lie the peek -- the column's eight tx samples per thread, eight global_load_dwordx4 and sixteen compares against zero (v_cmp_neq_f64: an
    unordered-or-unequal compare, so NaN counts as non-zero) -- one workgroup-wide OR (s_barrier), and no transcendental and no load of D (the D half is one scalar load
    of the flag demod_kernel wrote);
  * behind it the kernel is the text it was: 32 transcendentals (eight Box-Muller transforms), <= 128 VGPRs, no AGPRs, no scratch.
The VALU and transcendental totals are printed for the next reader (the parent's text: 1233 vector instructions in the code object, 32 of them transcendental)."""
from __future__ import annotations

import os

import pytest

from test_isa_cpu import LLVM, CodeObject

pytestmark = pytest.mark.skipif(not os.path.exists(os.path.join(LLVM, "llvm-objdump")), reason="ROCm LLVM tools not installed")

TRANS = ("v_log_f32", "v_sin_f32", "v_cos_f32", "v_sqrt_f32", "v_rcp_f32", "v_rsq_f32", "v_exp_f32")


@pytest.fixture(scope="module")
def echo_co(tmp_path_factory):
    return CodeObject(str(tmp_path_factory.mktemp("isa_range_dead")), "echo")


def test_dead_column_test_stands_in_front_of_the_generator(echo_co):
    name, meta, asm = echo_co.find("echo_range_xc_kernel", "ILi1E")
    assert meta["vgpr_count"] <= 128 and meta["agpr_count"] == 0 and meta["private_segment_fixed_size"] == 0, meta
    box_muller = [i for i, ln in enumerate(asm) if ln.startswith(("v_log_f32", "v_sin_f32", "v_cos_f32", "v_sqrt_f32"))]
    exits = [i for i, ln in enumerate(asm) if ln.startswith("s_endpgm")]
    assert len(box_muller) == 32, len(box_muller)
    assert exits and exits[0] < box_muller[0], "no exit in front of the first Box-Muller transform"
    head = asm[:exits[0]]
    assert sum(1 for ln in head if ln.startswith("global_load_dwordx4")) == 8, "the peek: eight tx samples per thread and nothing of D"
    assert sum(1 for ln in head if ln.startswith("v_cmp_neq_f64")) == 16, "both parts of the eight samples, NaN counted as non-zero"
    assert any(ln.startswith("s_barrier") for ln in head), "the workgroup-wide OR"
    assert sum(1 for ln in head if ln.startswith("s_load_dword ")) >= 1, "the scalar load of the symbol's D flag"
    valu = sum(1 for ln in asm if ln.startswith("v_"))
    trans = sum(1 for ln in asm if ln.startswith(TRANS))
    print(f"{name}: {valu} vector instructions in the code object, {trans} transcendental, {len(head)} instructions in front of the dead column's exit; {meta}")

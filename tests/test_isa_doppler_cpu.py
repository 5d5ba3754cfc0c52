"""ISA-level check of doppler_fft256_kernel (csrc/rdm.hip; no GPU: the gfx950 code object of the freshly built object, as tests/test_isa_cpu.py reads it).  Both
instantiations -- the one that forms only the outputs k2 = 0 and 15 of the second radix-16 pass (K2MASK 0x8001 = 32769) and the full one (0xFFFF = 65535) -- must
  * stay at four workgroups per compute unit: <= 128 VGPRs, no AGPRs, no scratch (the full one gets there only by parking four outputs in its own LDS slots: a
    toolchain that schedules differently must not spill silently);
  * have their loads in flight together: the twiddle and the sixteen slow-time samples, seventeen global_load_dwordx4, all issued in front of the first wait on the
    vector-memory counter;
  * exchange through four barriers (twiddles, real plane written, real plane read, imaginary plane written);
and the pruned one must have dropped the dead outputs: two global stores where the full one has sixteen.  The totals are printed for the next reader."""
from __future__ import annotations

import os

import pytest

from test_isa_cpu import LLVM, CodeObject

pytestmark = pytest.mark.skipif(not os.path.exists(os.path.join(LLVM, "llvm-objdump")), reason="ROCm LLVM tools not installed")


@pytest.fixture(scope="module")
def rdm_co(tmp_path_factory):
    return CodeObject(str(tmp_path_factory.mktemp("isa_doppler")), "rdm")


@pytest.mark.parametrize("mask,stores", [(0x8001, 2), (0xFFFF, 16)], ids=["pruned", "full"])
def test_doppler_fft256_registers_and_loads_in_flight(rdm_co, mask, stores):
    name, meta, asm = rdm_co.find("doppler_fft256_kernel", f"ILj{mask}E")
    assert meta["vgpr_count"] <= 128 and meta["agpr_count"] == 0 and meta["private_segment_fixed_size"] == 0, meta
    loads = [i for i, ln in enumerate(asm) if ln.startswith("global_load_dwordx4")]
    waits = [i for i, ln in enumerate(asm) if ln.startswith("s_waitcnt") and "vmcnt" in ln]
    assert len(loads) == 17, len(loads)
    assert waits and loads[-1] < waits[0], "a wait on the vector-memory counter stands between the loads"
    assert sum(1 for ln in asm if ln.startswith("s_barrier")) == 4
    assert sum(1 for ln in asm if ln.startswith("global_store_dwordx2")) == stores
    print(f"{name}: {len(asm)} instructions, {sum(1 for ln in asm if ln.startswith('v_'))} vector; {meta}")

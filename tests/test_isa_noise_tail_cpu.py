"""ISA-level checks of the noise term's two kernels (no GPU: the gfx950 code object of the freshly built cov.o, as tests/test_isa_split_cpu.py reads it).

cov_noise_tail_kernel -- the half slabs of the lazy grid, packed two to a slab (csrc/noise_walk.hpp) -- must run two workgroups per CU like the kernel it relieves
(<= 256 registers, no scratch), hold the 2 x 30 MFMAs of its two unrolled slab steps per tile group with no branch between them, draw four Box-Muller transforms per step
(16 transcendentals) and load nothing: it carries no beam-sum and no D.

cov_noise_beam_kernel<1> addresses the waveform through one buffer descriptor, the antenna in the load's scalar offset.  The double-step loop of tile group 0 -- from the
target of the backward branch behind the group's 60th MFMA to that branch -- held 843 instructions in the parent of this change, 303 of them scalar (60 MFMA, 430 other
vector-ALU, 36 LDS, 14 buffer), counted on the code object built with _build.py's flags by exactly this function; each of its 12 loads rebuilt a descriptor of its own (a
64-bit antenna x T x 16 product, base add, clamp, compare: about 15 scalar instructions).  With one descriptor the loop holds 680 instructions, 164 scalar.  Required: at
least 120 scalar instructions fewer than the parent's 303; otherwise the addressing has not changed."""
from __future__ import annotations

import importlib
import os
import re
import shutil
import subprocess

import pytest

from test_isa_cpu import LLVM, PKG, CodeObject

pytestmark = pytest.mark.skipif(not os.path.exists(os.path.join(LLVM, "llvm-objdump")), reason="ROCm LLVM tools not installed")

PARENT_LOOP_SCALAR = 303          # the parent commit's count (module docstring)
TRANSCENDENTALS = ("v_log_f32", "v_sin_f32", "v_cos_f32", "v_sqrt_f32")


@pytest.fixture(scope="module")
def cov_co(tmp_path_factory):
    return CodeObject(str(tmp_path_factory.mktemp("isa_noise_tail")), "cov")


def test_tail_kernel_shape(cov_co):
    name, meta, asm = cov_co.find("cov_noise_tail_kernel")
    assert meta["vgpr_count"] <= 256 and meta["agpr_count"] == 0 and meta["private_segment_fixed_size"] == 0, meta
    mf = [i for i, ln in enumerate(asm) if ln.startswith("v_mfma_f64_16x16x4")]
    assert len(mf) == 2 * 2 * 30, len(mf)                                  # two tile groups x two unrolled steps x 30
    for g in range(2):
        loop = asm[mf[60 * g]:mf[60 * g + 59] + 1]
        assert not any(ln.startswith(("s_cbranch", "s_branch")) for ln in loop), "a branch inside the MFMA stream"
        assert not any(ln.startswith(("buffer_load", "global_load", "flat_load")) for ln in loop), "the tail kernel loads nothing in its steps"
    body = asm[mf[0]:mf[29] + 1]                                             # one slab step of one tile group
    assert sum(1 for ln in body if ln.startswith(TRANSCENDENTALS)) == 16, "four Box-Muller transforms (4 transcendentals each) per step"
    assert sum(1 for ln in body if ln.startswith("ds_write_b128") or ln.startswith("ds_write2_b64")) >= 4


def _group0_loop(lines):
    """The double-step loop of tile group 0 out of [(instruction, address)]: from the target of the backward branch behind the 60th MFMA to that branch."""
    mf = [i for i, (ln, _) in enumerate(lines) if ln.startswith("v_mfma_f64_16x16x4")]
    e = mf[59]
    while not lines[e][0].startswith("s_cbranch"):
        e += 1
    off = int(lines[e][0].split()[1])
    off -= 65536 if off >= 32768 else 0                                      # simm16, in dwords from the next instruction
    assert off < 0, "the branch behind the MFMAs closes the loop"
    b = [a for _, a in lines].index(lines[e][1] + 4 + 4 * off)
    assert b <= mf[0]
    return [ln for ln, _ in lines[b:e + 1]]


def test_beam_loads_share_one_descriptor(cov_co, tmp_path):
    name, meta, asm = cov_co.find("cov_noise_beam_kernel", "ILi1E")
    # the same disassembly with addresses (CodeObject drops them): the loop is delimited by its closing branch's target
    b = importlib.import_module(PKG + "._build")
    obj = str(tmp_path / "cov.o")
    shutil.copy(os.path.join(b.OBJ, "cov.o"), obj)
    subprocess.run([os.path.join(LLVM, "llvm-objdump"), "--offloading", obj], check=True, capture_output=True)
    co = [os.path.join(str(tmp_path), f) for f in os.listdir(str(tmp_path)) if "gfx950" in f][0]
    dis = subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-d", co], check=True, capture_output=True, text=True).stdout
    lines, cur = [], None
    for ln in dis.splitlines():
        m = re.match(r"^[0-9a-f]+ <(\S+)>:", ln)
        if m:
            cur = m.group(1)
        elif cur == name and ln.startswith("\t") and "//" in ln:
            lines.append((ln.strip().split("//")[0].strip(), int(ln.split("//")[1].split(":")[0], 16)))
    loop = _group0_loop(lines)
    n = {k: sum(1 for ln in loop if ln.startswith(p)) for k, p in (("mfma", "v_mfma"), ("vector", "v_"), ("scalar", "s_"), ("lds", "ds_"), ("buffer", "buffer_"))}
    print(f"double-step loop of tile group 0: {len(loop)} instructions, {n}")
    assert n["mfma"] == 60 and sum(1 for ln in loop if ln.startswith("buffer_load_dwordx4")) == 12
    assert n["scalar"] <= PARENT_LOOP_SCALAR - 120, n

"""ISA-level regression checks of the hot kernels (no GPU needed: the gfx950 code objects are taken out of the freshly built objects).

The measured gains of round 3 came from properties of the generated code that nothing in the numerical tests would notice if a compiler
update or an innocent edit lost them again (DESIGN_HISTORY.md section 3c):
  * no vector-memory instruction of the fused echo + range kernel sits behind an `s_waitcnt vmcnt(0)` while its eight stores are issued
    (a branch around a load / store makes the wait-count pass give up: every wait becomes vmcnt(0));
  * the covariance block kernel keeps its loads in flight, its accumulators in place and its diagonal form compile-time (no selects);
  * the register budgets that set the occupancy (128 VGPRs = four waves per SIMD for the fused kernel, <= 256 for the covariance kernels)
    are met without scratch memory.
"""
from __future__ import annotations

import importlib
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = "5g_based_system_level_integrated_sensing_and_communication_simulator_amd"
LLVM = "/opt/rocm/lib/llvm/bin"
TARGET_SUFFIX = "hipv4-amdgcn-amd-amdhsa--gfx950"

pytestmark = pytest.mark.skipif(not os.path.exists(os.path.join(LLVM, "llvm-objdump")), reason="ROCm LLVM tools not installed")


class CodeObject:
    """Kernel metadata (.vgpr_count, .agpr_count, .private_segment_fixed_size) and per-kernel disassembly of one translation unit."""

    def __init__(self, tmp, unit):
        b = importlib.import_module(PKG + "._build")
        b.build()
        src = os.path.join(b.OBJ, unit + ".o")
        obj = os.path.join(tmp, unit + ".o")
        shutil.copy(src, obj)                       # llvm-objdump --offloading writes the bundles next to its input
        subprocess.run([os.path.join(LLVM, "llvm-objdump"), "--offloading", obj], check=True, capture_output=True)
        co = f"{obj}.0.{TARGET_SUFFIX}"
        assert os.path.exists(co), "no gfx950 code object in " + src
        notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", co], check=True, capture_output=True, text=True).stdout
        self.meta = {}
        cur = {}
        for ln in notes.splitlines():
            m = re.match(r"\s*(?:- )?\.(\w+):\s+(\S+)", ln)
            if not m:
                continue
            k, v = m.group(1), m.group(2)
            if k == "agpr_count":                   # first key of a kernel's block
                cur = {"agpr_count": int(v)}
            elif k in ("vgpr_count", "private_segment_fixed_size", "sgpr_count", "group_segment_fixed_size"):
                cur[k] = int(v)
            elif k == "name" and v.startswith("_Z"):
                cur["name"] = v
            elif k == "symbol" and "name" in cur:
                self.meta[cur["name"]] = cur
        dis = subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-d", co], check=True, capture_output=True, text=True).stdout
        self.asm = {}
        name = None
        for ln in dis.splitlines():
            m = re.match(r"^[0-9a-f]+ <(\S+)>:", ln)
            if m:
                name = m.group(1)
                self.asm[name] = []
            elif name and ln.startswith("\t"):
                self.asm[name].append(ln.strip().split("//")[0].strip())

    def find(self, *parts):
        hits = [n for n in self.meta if all(p in n for p in parts)]
        assert len(hits) == 1, (parts, hits)
        return hits[0], self.meta[hits[0]], self.asm[hits[0]]


@pytest.fixture(scope="module")
def echo_co(tmp_path_factory):
    return CodeObject(str(tmp_path_factory.mktemp("isa_echo")), "echo")


@pytest.fixture(scope="module")
def eigh_co(tmp_path_factory):
    return CodeObject(str(tmp_path_factory.mktemp("isa_eigh")), "eigh")


@pytest.fixture(scope="module")
def music_co(tmp_path_factory):
    return CodeObject(str(tmp_path_factory.mktemp("isa_music")), "music")


@pytest.fixture(scope="module")
def cov_co(tmp_path_factory):
    return CodeObject(str(tmp_path_factory.mktemp("isa_cov")), "cov")


def vm_waits(asm):
    return [int(m.group(1)) for ln in asm for m in [re.search(r"s_waitcnt.*vmcnt\((\d+)\)", ln)] if m]


@pytest.mark.parametrize("q,group", [(1, 4), (2, 2)])
def test_fused_kernel_keeps_exact_wait_counts(echo_co, q, group):
    name, meta, asm = echo_co.find("echo_range_sl_kernel", f"ILi{q}ELi1ELb1ELi{group}E")
    assert meta["vgpr_count"] <= 128 and meta["agpr_count"] == 0, meta      # four waves per SIMD, two 512-thread workgroups per CU
    assert meta["private_segment_fixed_size"] == 0, meta                     # no spills
    stores = [i for i, ln in enumerate(asm) if ln.startswith("buffer_store_dwordx4")]
    assert len(stores) == 8, f"{name}: expected the eight unconditional echoGrid stores, found {len(stores)}"
    assert all(" nt" in asm[i] for i in stores)
    between = vm_waits(asm[stores[0]:stores[-1]])
    assert between and min(between) > 0, f"{name}: a vmcnt(0) wait between the echoGrid stores: {between}"
    # the second load group is issued before the first group's stores
    loads = [i for i, ln in enumerate(asm) if ln.startswith("global_load_dwordx4")]
    assert sum(1 for i in loads if i < stores[0]) >= 2 * 2 * group, "the next group's loads must be in flight when the stores start"


@pytest.mark.parametrize("q,group", [(1, 4), (2, 2)])
def test_lazy_fused_kernel_has_no_echo_grid_store(echo_co, q, group):
    """echo_range_sl_kernel<Q, 1, STORE = false> (lazy echo grid, round 6): the same kernel without the eight echoGrid stores -- nothing else of a column goes to memory
    but its CUT rows."""
    name, meta, asm = echo_co.find("echo_range_sl_kernel", f"ILi{q}ELi1ELb0ELi{group}E")
    assert meta["vgpr_count"] <= 128 and meta["agpr_count"] == 0 and meta["private_segment_fixed_size"] == 0, meta
    assert not any(ln.startswith("buffer_store_dwordx4") for ln in asm), "the lazy form must not store the echo grid"
    assert sum(1 for ln in asm if ln.startswith("global_load_dwordx4")) >= 8 * (1 + q)       # txGrid + D loads of the eight elements are still there


@pytest.mark.parametrize("q", [1, 2])
def test_lazy_covariance_kernel_shape(cov_co, q):
    """cov_lazy_kernel<Q>: two workgroups per CU (<= 256 registers, at most a handful of spilled registers at two targets), the 2 x 30 MFMAs of its two slab steps, no
    global load of the grid (only the D values: 2 Q per thread and slab), the generator's transcendentals between the MFMAs, no waterfall loop (uniform descriptors)."""
    name, meta, asm = cov_co.find("cov_lazy_kernel", f"ILi{q}E")
    assert meta["vgpr_count"] <= 256 and meta["agpr_count"] == 0, meta
    assert meta["private_segment_fixed_size"] <= (0 if q == 1 else 32), meta
    mf = [i for i, ln in enumerate(asm) if ln.startswith("v_mfma_f64_16x16x4")]
    assert len(mf) == 2 * 2 * 30, len(mf)                                  # two tile groups x two unrolled steps x 30
    for g in range(2):                                                       # inside the slab loops: no waterfall loop (a buffer descriptor that is not provably uniform), no branch at all
        loop = asm[mf[60 * g]:mf[60 * g + 59] + 1]
        assert not any(ln.startswith(("s_cbranch", "s_branch")) for ln in loop), "a branch inside the MFMA stream"
    body = asm[mf[0]:mf[29] + 1]                                             # one slab step of one tile group
    assert sum(1 for ln in body if ln.startswith(("v_log_f32", "v_sin_f32", "v_cos_f32", "v_sqrt_f32"))) == 16, "four Box-Muller transforms (4 transcendentals each) per step"
    assert sum(1 for ln in body if ln.startswith("buffer_load_dwordx4")) == 2 * q
    assert sum(1 for ln in body if ln.startswith("ds_write_b128") or ln.startswith("ds_write2_b64")) >= 4


def test_fused_kernel_fallback_forms_exist(echo_co):
    for q in (0, 3, 4):
        echo_co.find("echo_range_kernelILi%dELi1E" % q)


def test_covariance_block_kernel_shape(cov_co):
    name, meta, asm = cov_co.find("cov_mfma_block_kernel")
    assert meta["private_segment_fixed_size"] == 0 and meta["agpr_count"] == 0 and meta["vgpr_count"] <= 256, meta
    w = vm_waits(asm)
    assert sum(1 for x in w if x == 0) <= 4 and sum(1 for x in w if x > 0) >= 24, w   # staging loads stay in flight under the MFMAs
    assert sum(1 for ln in asm if ln.startswith("v_cndmask")) <= 24                    # no operand selects beside v_mfma_f64
    assert not any("s_cbranch_execnz" in ln for ln in asm), "a waterfall loop: some buffer descriptor is not provably uniform"
    # the off-diagonal main loop: 48 MFMAs per slab with (next to) nothing but their operand reads in between -- no accumulator moves
    mf = [i for i, ln in enumerate(asm) if ln.startswith("v_mfma_f64_16x16x4")]
    assert len(mf) >= 96 + 60
    a = min(range(len(mf) - 47), key=lambda k: mf[k + 47] - mf[k])       # the tightest run of 48 MFMAs
    body = asm[mf[a]:mf[a + 47] + 1]
    assert len(body) <= 48 + 60, len(body)
    assert sum(1 for ln in body if ln.startswith("v_mov_b64")) <= 2 and not any(ln.startswith(("v_accvgpr", "scratch_")) for ln in body), \
        "accumulator moves inside the MFMA stream"
    assert sum(1 for ln in asm if ln.startswith("v_mov_b64")) <= 220


def test_covariance_small_kernel_budget(cov_co):
    name, meta, asm = cov_co.find("cov_mfma_small_kernelILi4E")
    assert meta["private_segment_fixed_size"] == 0 and meta["agpr_count"] == 0 and meta["vgpr_count"] <= 240, meta   # two workgroups per CU
    w = vm_waits(asm)
    assert sum(1 for x in w if x == 0) <= 6 and len(w) >= 60, (len(w), sum(1 for x in w if x == 0))


def test_covariance_staged_kernel_is_pipelined_inside_the_wave(cov_co):
    """A = 33..64: on gfx950 every instruction of either wave of a SIMD waits while a v_mfma_f64 is pending (tools/cobench.hip), so the staged
    covariance kernel hides its LDS reads / staging writes / staging loads one by one behind its own MFMAs.  A scheduler change that regroups
    them into a burst in front of the MFMA run costs ~10 us per launch and no numerical test would notice."""
    name, meta, asm = cov_co.find("cov_mfma_lds_kernelILi4E")
    assert meta["private_segment_fixed_size"] == 0 and meta["agpr_count"] == 0 and meta["vgpr_count"] <= 248, meta   # two workgroups per CU
    mf = [i for i, ln in enumerate(asm) if ln.startswith("v_mfma_f64_16x16x4")]
    assert len(mf) == 120                                          # 2 tile groups x 2 unrolled slab steps x 30
    gaps = sorted(mf[i + 1] - mf[i] - 1 for i in range(len(mf) - 1))
    assert gaps[-1] > 100 and gaps[-2] <= 20, gaps[-8:]            # (the one long gap: group 0's epilogue + group 1's prologue)
    assert sum(1 for g in gaps if g > 6) <= 6, gaps[-12:]          # barrier + loop bookkeeping once per slab step, nothing else bunches up
    mem = [i for i, ln in enumerate(asm) if ln.startswith(("ds_read_b128", "ds_write_b128", "buffer_load_dwordx4"))]
    in_loop = [i for i in mem if any(a < i < b for a, b in zip(mf, mf[1:]) if b - a <= 21)]
    assert len(in_loop) >= 2 * (16 + 14)                           # group 0: 8 reads + 4 writes + 4 loads per step; group 1: 6 + 4 + 4
    for i in in_loop:                                              # each of them directly between two MFMAs (with at most its wait / address op)
        assert any(asm[j].startswith("v_mfma") for j in range(i - 3, i)) and any(asm[j].startswith("v_mfma") for j in range(i + 1, i + 4)), asm[i - 3:i + 4]


def test_covariance_block_kernel_is_pipelined_inside_the_wave(cov_co):
    """cov_mfma_block_pl_kernel (A > 64): no scratch, <= 256 registers (two workgroups per CU), and the operand reads / staging writes / staging loads of a unit
    sit in the gaps of its MFMA stream -- at most a handful of instructions between two MFMAs except at the unit / diagonal-vs-off-diagonal seams."""
    name, meta, asm = cov_co.find("cov_mfma_block_pl_kernel")
    assert meta["private_segment_fixed_size"] == 0 and meta["vgpr_count"] <= 256, meta
    mf = [i for i, ln in enumerate(asm) if ln.startswith("v_mfma_f64_16x16x4")]
    assert len(mf) >= 200
    gaps = [b - a - 1 for a, b in zip(mf, mf[1:])]
    assert sum(1 for g in gaps if g <= 4) >= 0.9 * len(gaps), sorted(gaps)[-12:]
    assert sum(1 for g in gaps if g > 16) <= 2, sorted(gaps)[-6:]       # (the two code paths: diagonal and off-diagonal block pairs)


def test_one_pass_householder_kernel_budget(eigh_co):
    """1024-thread workgroup: 128 VGPRs is all a wave gets; the fused pass keeps four matrix loads in flight per thread (eight spilled)."""
    name, meta, asm = eigh_co.find("eigh_tridiag_fused_kernel")
    assert meta["private_segment_fixed_size"] == 0 and meta["vgpr_count"] <= 128, meta
    loads = sum(1 for ln in asm if ln.startswith("global_load_dwordx4"))
    stores = sum(1 for ln in asm if ln.startswith("global_store_dwordx4"))
    assert loads >= 4 and stores >= 4


def test_distributed_householder_kernel_exchange_code(eigh_co):
    """eigh_tridiag_dist_kernel: the matrix stays in registers (no scratch, one wave per SIMD), the exchange is tagged 16-byte granules -- write-through (sc1)
    and L2-resident stores both present, every polling load sc1 (never served by the CU's L1) -- with no release / acquire fence anywhere (no L2 write-back or
    L1 invalidate per reflector) and ONE workgroup barrier per reflector besides the two of the prologue."""
    name, meta, asm = eigh_co.find("eigh_tridiag_dist_kernel")
    assert meta["private_segment_fixed_size"] == 0 and meta["vgpr_count"] <= 256, meta
    assert not any(ln.startswith(("buffer_wbl2", "buffer_inv")) for ln in asm)
    st = [ln for ln in asm if ln.startswith("buffer_store_dwordx4")]
    ld = [ln for ln in asm if ln.startswith("buffer_load_dwordx4")]
    assert sum(" sc1" in ln for ln in st) >= 4 and sum(" sc1" not in ln for ln in st) >= 4, st
    assert len(ld) >= 6 and all(" sc1" in ln for ln in ld), ld
    assert sum(1 for ln in asm if ln.startswith("s_barrier")) <= 4


def test_scratch_users_are_the_known_ones(echo_co, eigh_co, music_co, cov_co):
    known = ("echo_range_kernelILi4E", "eigh_replay_kernel",       # spill a few registers by design
             "cov_lazy_kernelILi2E")                               # two targets, spread generator placement: 3 registers (16 B) beyond the 256 of two waves per SIMD
    for co in (echo_co, eigh_co, music_co, cov_co):
        for n, m in co.meta.items():
            if m.get("private_segment_fixed_size", 0) > 0:
                assert any(k in n for k in known), f"{n} uses {m['private_segment_fixed_size']} B of scratch"


@pytest.fixture(scope="module")
def cdl_co(tmp_path_factory):
    return CodeObject(str(tmp_path_factory.mktemp("cdl_co")), "cdl")


def test_fused_cdl_kernels_code_generation(cdl_co):
    """cdl_fused_kernel / cdl_fused_ul_kernel (DESIGN_HISTORY.md section 3g): two waves per SIMD (<= 256 registers), no scratch inside the tile loop (the compiler once turned
    the gather's slot array into a dynamically indexed scratch array and its lane selects into exec-masked branches: 2.6 k -> 7.9 k cycles per column tile), and the
    contraction as one straight-line run of MFMAs per tile / chunk."""
    # downlink, CDL-A shape: 3 column tiles, 4 delay slots
    name, meta, asm = cdl_co.find("cdl_fused_kernel", "ILi3ELi4E")
    assert meta["vgpr_count"] <= 256 and meta["agpr_count"] == 0
    assert meta["private_segment_fixed_size"] <= 64, "more than a handful of prologue spills"        # (a few registers of the per-range prologue)
    mf = [i for i, ln in enumerate(asm) if ln.startswith("v_mfma_f64_16x16x4")]
    assert len(mf) == 16 * 3 * 3, len(mf)                                  # 16 k-steps x 3 column tiles x 3 forms, unrolled once
    body = asm[mf[0]:mf[-1] + 1]
    assert not any(ln.startswith("scratch_") for ln in body), "scratch traffic inside the contraction"
    after = asm[mf[-1]:]
    assert sum(ln.startswith("scratch_") for ln in after) == 0, "scratch traffic in the filter / gather phases"
    assert sum(ln.startswith("s_barrier") for ln in after) <= 2 * 3 + 2, "more than two barriers per column tile"
    # the gather is branch-free: no exec-mask manipulation behind the MFMAs except loop control
    assert sum(ln.startswith("s_and_saveexec") or ln.startswith("s_or_saveexec") for ln in after) <= 6
    # uplink, 64 receive elements: 4 column tiles
    name, meta, asm = cdl_co.find("cdl_fused_ul_kernel", "ILi4E")
    assert meta["vgpr_count"] <= 256 and meta["private_segment_fixed_size"] == 0
    assert sum(ln.startswith("v_mfma_f64_16x16x4") for ln in asm) == 4 * 4 * 3       # one chunk: 4 k-steps x 4 column tiles x 3 forms
    assert not any(ln.startswith("scratch_") for ln in asm)

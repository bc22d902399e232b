"""Static budget of the C3 fast pass's Newton step (tools/valu_count.py on the device
assembly of the compile-time-(n, m) units, compiled with the product flags; no GPU needed).

The number of VALU instructions the one-wave SCHUR fast pass issues per Newton step is held
here, together with what keeps five waves on a SIMD: at most 96 VGPRs and no scratch access
inside the loop.  Every other compile-time SCHUR instantiation (affine, shared-matrix, fused
pullback; fast pass and pass 2) is held to the VGPRs it had before the round-7 trim.

Counts of tools/valu_count.py (every instruction of the loop's blocks once, line search and
alpha-trace blocks included):

    before the round-7 trim   1,177   (DESIGN.md §4's per-phase table, counted by hand, sums to 1,183)
    round 7                   1,120
"""

from __future__ import annotations

import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from mcp_amd import build as B  # noqa: E402

C3_FAST = "ipm_solve_kernelILi32ELi0ELi32ELi16ELi2ELi1ELi0ELb0E"   # <32, QP, 32, 16, SCHUR, PASS 1>
VALU_PARENT = 1177
VALU_BUDGET = 1120

pytestmark = pytest.mark.skipif(not (os.path.exists(B.HIPCC) or shutil.which(B.HIPCC)), reason="no hipcc")

_ASM: dict = {}


def unit_asm(unit: str, tmp_path_factory) -> str:
    """Device .s of csrc/<unit>.hip: the one the library build kept, else compiled here."""
    if unit not in _ASM:
        src = os.path.join(B.CSRC, unit + ".hip")
        cdir = os.path.join(B.OBJ_CACHE, unit + ".hip." + B._tu_key(src, B.FLAGS))
        found = None
        if os.path.exists(os.path.join(cdir, "ok")):
            found = next((os.path.join(cdir, f) for f in os.listdir(cdir) if f.endswith("gfx950.s")), None)
        if found is None:
            found = str(tmp_path_factory.mktemp("valu") / (unit + ".s"))
            subprocess.run([B.HIPCC, *B.FLAGS, "--cuda-device-only", "-S", src, "-o", found], check=True,
                           capture_output=True, timeout=900)
        _ASM[unit] = found
    return _ASM[unit]


def test_c3_fast_pass_newton_step_budget(tmp_path_factory):
    import valu_count

    r = valu_count.count(unit_asm("ipm_inst_spec", tmp_path_factory), C3_FAST)
    print(r)
    assert r["mfma"] == 16  # the loop found is the Newton step (16 Schur MFMAs)
    assert r["valu"] <= VALU_BUDGET < VALU_PARENT, r
    assert r["vgprs"] <= 96 and r["agprs"] == 0, r
    assert r["scratch_in_loop"] == 0, r


def kernel(nmax, fam, n, m, pas, fuse, shared):
    return f"ipm_solve_kernelILi{nmax}ELi{fam}ELi{n}ELi{m}ELi2ELi{pas}ELi{fuse}ELb{int(shared)}E"


# (unit, kernel, VGPRs before the round-7 trim); the C3 fast pass of the QP family itself is
# held to the 96 of five waves above
VGPRS_BEFORE = [
    ("ipm_inst_spec", kernel(32, 1, 32, 16, 1, 0, 0), 98), ("ipm_inst_spec", kernel(32, 1, 32, 16, 2, 0, 0), 118),
    ("ipm_inst_spec", kernel(2, 0, 2, 2, 1, 0, 0), 46), ("ipm_inst_spec", kernel(2, 0, 2, 2, 2, 0, 0), 56),
    ("ipm_inst_spec", kernel(16, 0, 16, 8, 1, 0, 0), 62), ("ipm_inst_spec", kernel(16, 0, 16, 8, 2, 0, 0), 100),
    ("ipm_inst_spec", kernel(32, 0, 32, 16, 2, 0, 0), 108),
    ("ipm_inst_shared_spec", kernel(2, 0, 2, 2, 1, 0, 1), 46), ("ipm_inst_shared_spec", kernel(2, 0, 2, 2, 2, 0, 1), 56),
    ("ipm_inst_shared_spec", kernel(16, 0, 16, 8, 1, 0, 1), 62), ("ipm_inst_shared_spec", kernel(16, 0, 16, 8, 2, 0, 1), 100),
    ("ipm_inst_shared_spec", kernel(32, 0, 32, 16, 1, 0, 1), 89), ("ipm_inst_shared_spec", kernel(32, 0, 32, 16, 2, 0, 1), 108),
    ("ipm_inst_fused", kernel(2, 0, 2, 2, 1, 8, 0), 46), ("ipm_inst_fused", kernel(2, 0, 2, 2, 2, 8, 0), 56),
    ("ipm_inst_fused", kernel(16, 0, 16, 8, 1, 24, 0), 63), ("ipm_inst_fused", kernel(16, 0, 16, 8, 2, 24, 0), 100),
    ("ipm_inst_fused", kernel(32, 0, 32, 16, 1, 48, 0), 95), ("ipm_inst_fused", kernel(32, 0, 32, 16, 2, 48, 0), 128),
    ("ipm_inst_shared_fused", kernel(2, 0, 2, 2, 1, 8, 1), 46), ("ipm_inst_shared_fused", kernel(2, 0, 2, 2, 2, 8, 1), 56),
    ("ipm_inst_shared_fused", kernel(16, 0, 16, 8, 1, 24, 1), 63), ("ipm_inst_shared_fused", kernel(16, 0, 16, 8, 2, 24, 1), 100),
    ("ipm_inst_shared_fused", kernel(32, 0, 32, 16, 1, 48, 1), 95), ("ipm_inst_shared_fused", kernel(32, 0, 32, 16, 2, 48, 1), 128),
]


@pytest.mark.parametrize("unit", ["ipm_inst_spec", "ipm_inst_shared_spec", "ipm_inst_fused", "ipm_inst_shared_fused"])
def test_compile_time_schur_kernels_keep_their_registers(unit, tmp_path_factory):
    import valu_count

    asm = unit_asm(unit, tmp_path_factory)
    for u, name, before in VGPRS_BEFORE:
        if u != unit:
            continue
        _, _, meta = valu_count.kernel_body(asm, name)
        print(name, meta)
        assert meta["NumVgprs"] <= before and meta["ScratchSize"] == 0, (name, meta, before)


def test_counter_classifies_by_prefix():
    import valu_count

    got = [valu_count.classify(op) for op in
           ("v_fmac_f64_dpp", "v_mfma_f64_16x16x4_f64", "ds_read2_b64", "global_load_dwordx2", "flat_load_dwordx2",
            "scratch_load_dword", "s_mov_b64", "s_waitcnt", "s_nop", "s_cbranch_execz")]
    assert got == ["valu", "mfma", "lds", "vmem", "vmem", "vmem", "salu", "wait", "wait", "branch"]

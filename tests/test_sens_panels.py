"""Panel width of a generated module's sensitivity kernels (CPU part).

The blocked LU of mcpx_nl_vjp_wg / mcpx_nl_jvp_wg keeps a panel of 16, 8 or 4 columns of all
remaining rows in LDS; the widest that fits is chosen twice — by the C macros of
csrc/ipm_nl_kernel.hpp (MCPX_NL_SENS_NB_VJP / _JVP: which kernels the code object holds and the
MCPX_MODULE_VJP / _JVP mask bits) and by NLSystem.sens_panels() (what the front end reports).
This file evaluates the macros with gcc against the Python rule at the lane-change sizes around
every width change, with and without the `sens_panel_max` cap, and checks that the code objects
of horizons past the 16-column fit really hold both kernels.  The GPU part is
tests/test_sens_panels_gpu.py."""

from __future__ import annotations

import os
import subprocess

import pytest

from mcp_amd import codegen
from mcp_amd.lane_change import LaneChangeGame

HDR = os.path.join(os.path.dirname(codegen.__file__), "csrc", "ipm_nl_kernel.hpp")
MACROS = ("MCPX_NL_SENS_NB_VJP", "MCPX_NL_SENS_NB_JVP", "MCPX_NL_CAN_WG_REDUCED", "MCPX_NL_CAN_WG_DENSE",
          "MCPX_NL_CAN_WG_SCHUR")
LIMIT = 160 * 1024 - 2048

# lane change (n, m) = (20T, 25T) at T = 2, 14, 15, 20, 21, 30; then the sizes where the 4-column
# panel stops fitting: LDS(NS, 4) = 24·NV + 39·NS + 512 ≤ 161,792.  m = 0: 63·n ≤ 161,280 ⇔
# n ≤ 2,560 (exactly the limit at 2,560).  (1000, 1000): the pullback's 2,000 rows fit 4 columns
# (150,512 B), the tangents' 3,000 do not (189,512 B).  (2000, 1000): neither (213,512 B for the
# pullback).
SIZES = [(40, 50), (280, 350), (300, 375), (400, 500), (420, 525), (600, 750),
         (2560, 0), (2561, 0), (1000, 1000), (2000, 1000)]
# the widths of the default module (ISSUE table: T = 15 → 16 / 8, T = 21 → 8 / 8, T = 30 → 8 / 4)
DEFAULT_WIDTHS = {(40, 50): (16, 16), (280, 350): (16, 16), (300, 375): (16, 8), (400, 500): (16, 8),
                  (420, 525): (8, 8), (600, 750): (8, 4), (2560, 0): (4, 4), (2561, 0): (0, 0),
                  (1000, 1000): (4, 0), (2000, 1000): (0, 0)}


def _section() -> str:
    """The preprocessor lines of the header from MCPX_NL_NV to MCPX_NL_SENS_NB_JVP: the workgroup
    kernels' LDS macros and the sensitivity kernels' width selection, `#ifndef` default included."""
    text = open(HDR).read().replace("\\\n", " ")
    lines = text.splitlines()
    lo = next(i for i, l in enumerate(lines) if l.startswith("#define MCPX_NL_NV "))
    hi = next(i for i, l in enumerate(lines) if l.startswith("#define MCPX_NL_SENS_NB_JVP "))
    return "\n".join(l for l in lines[lo:hi + 1] if l.startswith("#"))


def _system(n, m, cap=None):
    nl = object.__new__(codegen.NLSystem)
    nl.n, nl.m, nl.has_s = n, m, False
    if cap is not None:
        nl.sens_panel_max = cap
    return nl


def _macros(tmp_path, cap):
    """{(n, m): the MACROS' values} with MCPX_NL_SENS_NB_MAX = cap (None: the header's default)."""
    src = ["#include <stdio.h>", "#define MCPX_NL_HAS_S 0", _section(), "int main(void) {"]
    for n, m in SIZES:
        src += ["#undef MCPX_NL_N", "#undef MCPX_NL_M", f"#define MCPX_NL_N {n}", f"#define MCPX_NL_M {m}",
                '  printf("' + " ".join(["%d"] * len(MACROS)) + '\\n", ' + ", ".join(f"(int)({x})" for x in MACROS) + ");"]
    src += ["  return 0;", "}"]
    tag = "default" if cap is None else str(cap)
    c = tmp_path / f"panels_{tag}.c"
    c.write_text("\n".join(src) + "\n")
    exe = tmp_path / f"panels_{tag}"
    subprocess.run(["gcc", "-O0", *([] if cap is None else [f"-DMCPX_NL_SENS_NB_MAX={cap}"]), "-o", str(exe), str(c)],
                   check=True)
    rows = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split("\n")
    return {nm: tuple(int(v) for v in row.split()) for nm, row in zip(SIZES, rows)}


def test_sens_panel_macros_equal_sens_panels(tmp_path):
    default = _macros(tmp_path, None)
    for cap in (16, 8, 4):
        got = _macros(tmp_path, cap)
        for n, m in SIZES:
            nl = _system(n, m, cap)
            sp, ws = nl.sens_panels(), nl.wg_solvers()
            assert got[(n, m)][:2] == (sp["vjp"], sp["jvp"]), (n, m, cap, got[(n, m)], sp)
            # the cap is a cap: min(default width, cap), and nothing appears that did not fit
            assert got[(n, m)][:2] == tuple(min(w, cap) for w in DEFAULT_WIDTHS[(n, m)]), (n, m, cap)
            # the solve kernels do not follow the width: MCPX_NL_CAN_WG_* and wg_solvers() as before
            lds16 = lambda ns: 8 * 3 * (n + 2 * m) + ns * (8 * 16 + 7) + 512
            want = (int(lds16(n + m) <= LIMIT), int(lds16(n + 2 * m) <= LIMIT), int(lds16(n) <= LIMIT))
            assert got[(n, m)][2:] == want == (int(ws["reduced"]), int(ws["dense"]), int(ws["schur"])), (n, m, cap)
        if cap == 16:
            assert got == default  # the header's own default is 16
    for n, m in SIZES:  # an NLSystem nobody set a cap on
        sp = _system(n, m).sens_panels()
        assert default[(n, m)][:2] == DEFAULT_WIDTHS[(n, m)] == (sp["vjp"], sp["jvp"]), (n, m)


def test_lds_formula_values_of_the_width_table():
    """The byte counts DESIGN.md §4 quotes for the lane change (24·NV + NS·(8·NB + 7) + 512)."""
    lds = lambda T, ns, nb: 24 * 70 * T + ns * T * (8 * nb + 7) + 512
    assert lds(14, 70, 16) == 156332 and lds(15, 70, 16) == 167462 and lds(15, 70, 8) == 100262
    assert lds(15, 45, 16) == 116837 and lds(20, 45, 16) == 155612 and lds(21, 45, 16) == 163367
    assert lds(21, 45, 8) == 102887 and lds(30, 45, 8) == 146762 and lds(30, 70, 8) == 200012
    assert lds(30, 70, 4) == 132812


def test_sens_panel_max_rejects_other_widths():
    with pytest.raises(ValueError):
        LaneChangeGame(2, backend_options={"sens_panel_max": 12})


def test_code_objects_hold_the_sensitivity_kernels_past_the_16_column_fit():
    """T = 15 (tangents on 8 columns) and T = 21 (pullback and tangents on 8): both kernels are
    in the code object.  The capped T = 2 modules are code objects of their own, built from the
    same generated text (the oracle's C is shared)."""
    for T, widths in ((15, {"vjp": 16, "jvp": 8}), (21, {"vjp": 8, "jvp": 8})):
        nl = LaneChangeGame(T).mcp.nl
        assert nl.sens_panels() == widths
        blob = open(nl.build_module(), "rb").read()
        assert b"mcpx_nl_vjp_wg" in blob and b"mcpx_nl_jvp_wg" in blob, T
    base = LaneChangeGame(2).mcp.nl
    paths = {16: base.build_module()}
    for cap in (8, 4):
        nl = LaneChangeGame(2, backend_options={"sens_panel_max": cap}).mcp.nl
        assert nl.sens_panels() == {"vjp": cap, "jvp": cap}
        assert nl.key == base.key and nl.body == base.body
        assert f"#define MCPX_NL_SENS_NB_MAX {cap}" in nl.hip_source()
        paths[cap] = nl.build_module()
        blob = open(paths[cap], "rb").read()
        assert b"mcpx_nl_vjp_wg" in blob and b"mcpx_nl_jvp_wg" in blob, cap
    assert "MCPX_NL_SENS_NB_MAX" not in base.hip_source()
    assert len({os.path.realpath(p) for p in paths.values()}) == 3

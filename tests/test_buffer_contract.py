"""The case table of the buffer-contract tests (tests/helpers/contract_cases.py), checked on the
CPU before any GPU is involved.

* The table reaches every kernel family the full-θ entry points can launch, by the host layer's
  selection rule restated in the helper: a future family fails here until a case is added.
* Its inputs are what the GPU tests rely on, asserted on the oracle's output: every one-wave and
  module solve case has an instance with a NaN in θ (whose record is NaN), an instance stopped at
  max_outer_iters (MCPX_FAIL_MAX_OUTER) and at least three solved instances; every workgroup case
  and every sensitivity point solves throughout.
* The θ of the fast-pass stride test really defeats the SCHUR kernels' symmetry check.
* The helpers that build padded and tight θ buffers and the expected α trace do what they say."""

from __future__ import annotations

import numpy as np
import pytest

from mcp_amd import _abi
from tests.helpers import contract_cases as cc
from tests.helpers.wg_cases import QP, kernel_constants

SOLVERS = ("reduced", "dense", "schur")


def _ids(cases):
    return [pytest.param(c, id=c.id) for c in cases]


def test_table_reaches_every_kernel_family():
    k = kernel_constants()
    want = set()
    # one wave, compile-time sizes (ipm_inst_spec.hip), and the affine SCHUR kernel at C3's shape
    want |= {("wave", "spec", "qp", ls, n, m) for n, m in cc.SPEC_QP for ls in ("reduced", "schur")}
    want |= {("wave", "spec", "affine", "schur", 32, 16)}
    # one wave, runtime sizes: even and odd p
    want |= {("wave", "generic", "qp", ls, n, m) for n, m in ((5, 3), (4, 3)) for ls in SOLVERS}
    want |= {("wave", "generic", "affine", ls, 6, 4) for ls in SOLVERS}
    want |= {("wave", "generic-forced", "qp", "schur", 32, 16)}
    want |= {("wave", "two-pass", "qp", 16, 8)}
    # one workgroup per instance
    want |= {("wg", f, ls, 128, "vr") for f in ("qp", "affine") for ls in ("reduced", "dense")}
    want |= {("wg", "qp", "reduced", 256, "vr"), ("wg", "qp", "dense", 256, "workspace")}
    want |= {("wg", "schur", 256, "A in LDS", 2), ("wg", "schur", 512, "A from theta", 2)}
    # the fused solve + pullback
    want |= {("fused", "epilogue", "schur", 32, 16), ("fused", "composed", "reduced", 5, 3)}
    # sensitivities
    want |= {("sens-wave", f, kind) for f in ("qp", "affine") for kind in ("vjp", "jvp")}
    want |= {("sens-wg", f, kind) for f in ("qp", "affine") for kind in ("vjp", "jvp", "cond")}
    # generated modules
    want |= {("module", "cubic", "reduced", "wave")}
    want |= {("module", "lane", "schur", kern) for kern in ("wave", "multiwave", "band", "workgroup")}
    want |= {("module-sens", "lane", kind) for kind in ("vjp", "jvp")}

    got = {cc.solve_family(c, k) for c in cc.SOLVE_CASES + cc.FUSED}
    for c in cc.SENS_CASES:
        got |= cc.sens_families(c)
    assert got == want, f"not reached: {sorted(map(str, want - got))}; unknown: {sorted(map(str, got - want))}"

    # the families of the host layer that exist at all: every family / solver pair of the one-wave
    # and workgroup launchers appears, so a new launcher has no row to hide behind
    one_wave = {(f[2], f[3]) for f in got if f[0] == "wave" and f[1] in ("spec", "generic")}
    assert one_wave == {(f, ls) for f in ("qp", "affine") for ls in SOLVERS}
    assert {f[1:3] for f in got if f[0] == "wg" and f[1] != "schur"} == {(f, ls) for f in ("qp", "affine")
                                                                         for ls in ("reduced", "dense")}
    ids = [c.id for c in cc.SOLVE_CASES + cc.FUSED + cc.SENS_CASES]
    assert len(ids) == len(set(ids))


def test_table_shapes_follow_the_issue():
    solve = cc.SOLVE_CASES + cc.FUSED
    for c in solve:
        assert (c.B == 2) if c.N > 256 else (c.B in (5, 7)), c.id  # odd on purpose; 2 in the 512 bucket
        assert c.pad in (1, 3)
    for c in cc.SENS_CASES:
        assert c.B in (5, 7) and c.pad in (1, 3) and c.K == 9
    # both paddings meet an even and an odd p, so the parity of a row's first double flips both ways
    parity = {(cc.theta_p(c) % 2, c.pad) for c in solve if c.one_wave}
    assert parity == {(0, 1), (0, 3), (1, 1), (1, 3)}
    assert _abi.theta_dim(QP, 5, 3) == 48 and _abi.theta_dim(QP, 4, 3) == 35
    warm = [c.warm for c in cc.SOLVE_CASES if not c.module]
    assert abs(sum(warm) - len(warm) / 2) <= 1  # warm starts on half of the cases
    assert any(c.m > 64 for c in cc.SOLVE_CASES)  # W = 2 active-mask words


@pytest.mark.parametrize("case", _ids([c for c in cc.SOLVE_CASES + cc.FUSED if c.one_wave or c.module]))
def test_one_wave_and_module_inputs_on_the_oracle(oracle_lib, case):
    """A NaN instance, an instance at the outer limit, at least three solved ones — so that NaN
    results and failed records are told apart from an unwritten (poisoned) output."""
    th, _ = case.inputs()
    r = cc.oracle_solve(oracle_lib, case)
    nan_rows = np.isnan(th).any(axis=1)
    assert nan_rows.sum() >= 1 and np.isnan(r["x"][nan_rows]).all() and np.isnan(r["kkt_error"][nan_rows]).all()
    limit = (r["outer_iters"] == cc.OUTER_LIMIT) & ((r["fail_reason"] & _abi.FAIL_MAX_OUTER) != 0) & ~nan_rows
    assert limit.sum() >= 1 and (r["status"][limit] == _abi.STATUS_FAILED).all()
    assert (r["newton_iters"][limit] > cc.TRACE).all()  # their trace fills all TRACE steps
    solved = (r["status"] == 0) & ~nan_rows & np.isfinite(r["x"]).all(axis=1) & (r["fail_reason"] == 0)
    assert solved.sum() >= 3, r["status"]
    assert (r["newton_iters"][solved] < cc.TRACE).all()  # … and theirs leaves a tail untouched
    if case.asym:  # rows the fast pass defers, and rows it finishes
        asym = th[:, 1] != th[:, case.n]
        assert (asym & solved).sum() >= 1 and (~asym & solved).sum() >= 1


@pytest.mark.parametrize("case", _ids([c for c in cc.SOLVE_CASES if not (c.one_wave or c.module)]))
def test_workgroup_inputs_all_solve(oracle_lib, case):
    r = cc.oracle_solve(oracle_lib, case)
    assert (r["status"] == 0).all() and np.isfinite(r["x"]).all()
    if case.m > 64:  # both mask words carry bits somewhere in the batch
        assert r["active_mask"].shape == (case.B, 2) and (r["active_mask"] != 0).any(axis=0).all()


@pytest.mark.parametrize("case", _ids(cc.FUSED))
def test_fused_reference_is_solve_then_pullback(oracle_lib, case):
    r, dth, st = cc.oracle_fused(oracle_lib, case)
    assert dth.shape == (case.B, cc.theta_p(case)) and st.shape == (case.B,)
    ok = (r["status"] == 0) & np.isfinite(r["x"]).all(axis=1)
    assert ok.sum() >= 3 and (st[ok] == 0).all() and np.isfinite(dth[ok]).all()


@pytest.mark.parametrize("case", _ids(cc.SENS_CASES))
def test_sensitivity_points_solve(oracle_lib, case):
    r = cc.oracle_point(oracle_lib, case)
    assert (r["status"] == 0).all()
    for kind in case.kinds:
        res, st = cc.oracle_sens(oracle_lib, case, kind)
        assert (st == 0).all() and np.isfinite(res).all(), kind


@pytest.mark.parametrize("n,m,pad", [(16, 8, 1), (32, 16, 3), (32, 16, 1), (2, 2, 3), (5, 3, 1), (4, 3, 3)])
def test_shift_blind_theta_defeats_the_symmetry_check(oracle_lib, n, m, pad):
    """The window a fast pass would read for instance 1 with p in place of theta_ld — the doubles
    from 1·p of the padded buffer — has a symmetric M block, is a QP the oracle takes Newton steps
    on, and gives another x than instance 1: the GPU test on this θ can fail."""
    th, wide = cc.shift_blind_qp(n, m, 5, pad)
    p = th.shape[1]
    assert wide.shape == (5, p + pad) and np.array_equal(wide[:, :p], th) and np.isfinite(wide).all()
    kw = dict(tol=1e-6, linear_solver="schur", max_outer_iters=cc.OUTER_LIMIT)
    r = oracle_lib.solve_batch(QP, n, m, th, **kw)
    assert (r["status"] == 0).all()
    window = wide.reshape(-1)[p:2 * p]
    M = window[:n * n].reshape(n, n)
    assert np.array_equal(M, M.T) and not np.array_equal(window, th[1])
    w = oracle_lib.solve_batch(QP, n, m, window[None, :], **kw)
    assert w["newton_iters"][0] > 0 and not np.array_equal(w["x"][0], r["x"][1])


def test_padding_helpers():
    from tests.helpers.contract_calls import tight

    a = np.arange(12.0).reshape(3, 4)
    w = cc.padded(a, 3)
    assert w.shape == (3, 7) and w.flags.c_contiguous
    assert np.array_equal(w[:, :4], a) and np.isnan(w[:, 4:]).all()
    t = tight(a, 7)
    assert t.size == 2 * 7 + 4 and np.array_equal(t[14:], a[2]) and np.isnan(t[4:7]).all()
    assert np.array_equal(t[:14].reshape(2, 7)[:, :4], a[:2])


def test_expected_trace_and_mismatch_report(oracle_lib):
    case = cc.SOLVE_CASES[0]
    r = cc.oracle_solve(oracle_lib, case)
    tr = cc.expected_trace(r, cc.FILL)
    for b in range(case.B):
        k = min(int(r["newton_iters"][b]), cc.TRACE)
        assert np.array_equal(tr[b, :k], r["alpha_trace"][b, :k]) and (tr[b, k:] == cc.FILL).all()
        assert (r["alpha_trace"][b, :k] <= _abi.MAX_LS_TRIALS).all()
    assert cc.solve_mismatches(r, r) == []
    moved = {k: v.copy() for k, v in r.items()}
    moved["x"][0, 0] = np.nextafter(moved["x"][0, 0], np.inf)  # one ulp is a mismatch
    moved["fail_reason"][2] ^= 1
    assert cc.solve_mismatches(moved, r) == ["x", "fail_reason"]
    assert cc.solve_mismatches({k: v for k, v in moved.items() if k != "fail_reason"}, r, absent=("fail_reason",)) == ["x"]

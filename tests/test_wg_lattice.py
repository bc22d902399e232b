"""Every workgroup-per-instance kernel of the QP and affine families, and the oracle beyond
one wave.

The workgroup path compiles 40 kernels for the two families (ipm_inst_wg.hip,
ipm_inst_wg_vr.hip, ipm_inst_wg_gj.hip, sens_inst_wg.hip): REDUCED / DENSE solves at
{128 and 256 in registers, 256 / 512 / 768 through the slot's workspace}, the QP SCHUR
Gauss-Jordan at four buckets, VJP and JVP at four buckets.  One table
(tests/helpers/wg_cases.py) holds the smallest shapes that reach each of them or sit on
an edge of its range (bucket edges, MCPX_VR_MAX, Gauss-Jordan panels of width < 16, 16, 17,
the MFMA's K padding, the LDS copy of A against A read from θ).

CPU: the table reaches all 40 kernels by the host layer's selection rule; and on the
same inputs the C oracle (whose SCHUR branch follows the kernels: K padding,
gj_spd_solve) agrees with the independent LAPACK restatement oracle/ipm_ref.py, which
always factors the full ∇F + tol·I — counts equal, iterates within the project's 1e-8
 — and the oracle's sensitivities with a dense LAPACK solve.
GPU: every case bit-identical to the oracle."""

from __future__ import annotations

import numpy as np
import pytest
import scipy.linalg

from oracle import ipm_ref
from tests.helpers.wg_cases import (AFFINE, FAMILY_NAME, JVP_RHS, QP, SENS_CASES, SOLVE_CASES, SensCase,
                                    feasible_qp_theta, gj_a_cap, gj_lda, kernel_constants)
from tests.test_sensitivity import _same
from tests.test_wg import TRACE, assert_bit_exact

BAR = 1e-8  # oracle against the LAPACK restatement, relative to max(1, max|ref|)


def _params(cases):
    return [pytest.param(c, id=c.id, marks=[pytest.mark.slow] if c.slow else []) for c in cases]


_ORACLE = {}


def _oracle_solve(oracle_lib, case):
    """The oracle's solve of a table case (all case.B instances), computed once for the CPU and
    the GPU test of the case; nobody writes into it."""
    if case not in _ORACLE:
        th, start = case.inputs()
        _ORACLE[case] = oracle_lib.solve_batch(case.family, case.n, case.m, th, tol=1e-6, linear_solver=case.solver,
                                               trace_len=TRACE, nthreads=8, **start)
    return _ORACLE[case]


def _oracle_point(oracle_lib, case):
    """The solutions (default solver) a sensitivity case is differentiated at."""
    if case not in _ORACLE:
        th = case.inputs()[0]
        _ORACLE[case] = oracle_lib.solve_batch(case.family, case.n, case.m, th, tol=1e-6, nthreads=8)
    return _ORACLE[case]


def _rel(a, ref):
    return float(np.max(np.abs(a - ref)) / max(1.0, np.max(np.abs(ref))))


# ---------------------------------------------------------------- CPU: the table reaches every kernel


def test_table_reaches_every_workgroup_kernel():
    """The kernel each case launches, by the host layer's rule with the constants read from
    the headers: the table's set is the full product of the compiled kernels, and its
    cases sit on both sides of every switch (MCPX_VR_MAX, bucket edges, the SCHUR
    kernels' LDS capacity for A).  A new bucket or a moved MCPX_VR_MAX fails here until
    the table follows."""
    c = kernel_constants()
    buckets, vr_max = c["buckets"], c["vr_max"]
    fams, solvers = tuple(FAMILY_NAME.values()), ("reduced", "dense")
    want = {(f, ls, nv, "vr") for f in fams for ls in solvers for nv in buckets if nv <= 256}
    want |= {(f, ls, nv, "workspace") for f in fams for ls in solvers for nv in buckets if nv >= 256}
    want |= {("schur", nv) for nv in buckets}
    want |= {(f, k, nv) for f in fams for k in ("vjp", "jvp") for nv in buckets}
    assert len(want) == 20 + 4 + 16

    got = {case.kernel(c) for case in SOLVE_CASES}
    for case in SENS_CASES:
        if case.gpu:
            got |= case.kernels(c)
    assert got == want, f"not reached: {sorted(map(str, want - got))}; unknown: {sorted(map(str, got - want))}"

    for fam in FAMILY_NAME:
        for ls in solvers:
            mine = [s for s in SOLVE_CASES if s.family == fam and s.solver == ls and not s.warm]
            rows_256 = {s.ns for s in mine if 128 < s.N <= 256}
            assert {vr_max, vr_max + 1} <= rows_256, (fam, ls, "both sides of MCPX_VR_MAX")
            dims = {s.N for s in mine}
            edges = {e for b in buckets[:-1] for e in (b, b + 1)} | {buckets[0] + 1, buckets[-1]}
            assert edges <= dims, (fam, ls, sorted(edges - dims))
        assert any(s.m > 64 for s in SOLVE_CASES if s.family == fam)  # multi-word active masks

    schur = [s for s in SOLVE_CASES if s.solver == "schur"]
    for nv in buckets:
        cap = gj_a_cap(nv, c["gj_max"])
        fits = {s.n * gj_lda(s.m) <= cap for s in schur if s.kernel(c) == ("schur", nv)}
        if nv >= 512:
            assert cap == 8320
            assert fits == {True, False}, f"bucket {nv}: A in LDS and A read from θ"
        else:  # the largest A of the bucket fits by construction
            assert fits == {True}
    assert {s.n for s in schur} >= {1, 16, 17} and any(s.n < 16 for s in schur) and any(s.n % 16 for s in schur)
    assert any(s.m % 4 == 3 for s in schur)  # one padded K lane of the MFMA
    assert any(s.K > JVP_RHS for s in SENS_CASES if s.gpu)  # a second, narrower JVP factorisation


def test_feasible_qp_theta_is_strictly_feasible():
    n, m, B = 5, 70, 3
    th = feasible_qp_theta(np.random.default_rng(0), n, m, B)
    ref = np.random.default_rng(0)
    from mcp_amd.qp_benchmark import generate_random_parameter, unpack_parameters

    plain = generate_random_parameter(ref, n, m, 0.0, batch=B)
    xs = ref.standard_normal((B, n))
    keep = np.ones(th.shape[1], bool)
    keep[n * n + m * n:n * n + m * n + m] = False
    np.testing.assert_array_equal(th[:, keep], plain[:, keep])  # only b is replaced
    for b in range(B):
        u = unpack_parameters(th[b], n, m)
        slack = u["A"] @ xs[b] - u["b"]
        assert slack.min() >= 0.1 - 1e-12 and slack.max() <= 1.0 + 1e-12


# ---------------------------------------------------------------- CPU: oracle against the LAPACK restatement


@pytest.mark.parametrize("case", _params(SOLVE_CASES))
def test_oracle_matches_lapack_restatement_beyond_one_wave(oracle_lib, case):
    """Every instance solves, with the restatement's status and counts, and its iterates
    within 1e-8 of the restatement's (LAPACK getrf of the full system whatever the
    oracle's linear solver: SCHUR's K padding and Gauss-Jordan, REDUCED's slack
    elimination and the warm start are checked against it).  Observed: ≤ 5e-14."""
    th, start = case.inputs()
    r = _oracle_solve(oracle_lib, case)
    worst = 0.0
    for b in range(case.B):
        ref = ipm_ref.solve(case.family, th[b], case.n, case.m, tol=1e-6, **{k: v[b] for k, v in start.items()})
        assert ref.status == "solved" and r["status"][b] == 0, b
        assert (r["outer_iters"][b], r["newton_iters"][b]) == (ref.outer_iters, ref.newton_iters), b
        z = np.concatenate([r["x"][b], r["y"][b], r["s"][b]])
        d = _rel(z, np.concatenate([ref.x, ref.y, ref.s]))
        worst = max(worst, d)
        assert d <= BAR, (b, d)
    print(f"{case.id}: worst relative difference {worst:.2e}")


def _lapack_vjp(family, theta, n, m, x, y, s, gx, gy, gs):
    """(∂z/∂θ)ᵀ g with ∂z/∂θ = (−∇F_z)⁻¹ ∇F_θ (src/AutoDiff.jl:18-40), in closed form: one LAPACK
    solve λ = (−∇F_z)⁻ᵀ g, then ∇F_θᵀ λ by outer products — F is affine in θ, its G rows
    P x + Q y + g and its H rows R x + S y + h (the QP: M x − Aᵀ y − ϕ and A x − b)."""
    J = ipm_ref.F_and_jacobian(ipm_ref.unpack(family, theta, n, m), x, y, s, 0.0)[1]
    lam = scipy.linalg.solve(-J.T, np.concatenate([gx, gy, gs]))
    lg, lh = lam[:n], lam[n:n + m]
    vec = lambda a: a.flatten("F")
    if family == QP:
        return np.concatenate([vec(np.outer(lg, x)), vec(np.outer(lh, x) - np.outer(y, lg)), -lh, -lg])
    return np.concatenate([vec(np.outer(lg, x)), vec(np.outer(lg, y)), vec(np.outer(lh, x)), vec(np.outer(lh, y)),
                           lg, lh])


def _lapack_jvp(family, theta, n, m, x, y, s, theta_dot):
    """(−∇F_z)⁻¹ ∇F_θ θ̇ per partial: ∇F_θ θ̇ is the G and H rows of the family at the blocks of θ̇."""
    J = ipm_ref.F_and_jacobian(ipm_ref.unpack(family, theta, n, m), x, y, s, 0.0)[1]
    rhs = np.zeros((n + 2 * m, len(theta_dot)))
    for k, td in enumerate(theta_dot):
        P, Q, R, S, g, h = ipm_ref.unpack(family, td, n, m)
        rhs[:n, k] = P @ x + Q @ y + g
        rhs[n:n + m, k] = R @ x + S @ y + h
    return scipy.linalg.solve(-J, rhs).T


@pytest.mark.parametrize("family", [QP, AFFINE], ids=["qp", "affine"])
def test_closed_form_sensitivities_equal_pivoted_qr_restatement(oracle_lib, family):
    """The closed form above against ipm_ref.vjp / jvp (∇F_θ column by column, pivoted QR as
    the reference) at n = 6, m = 4: 1e-12 relative."""
    case = SensCase(family, 6, 4, K=3, B=4)
    th, (gx, gy, gs), td = case.inputs()
    r = oracle_lib.solve_batch(family, 6, 4, th, tol=1e-6)
    assert np.all(r["status"] == 0)
    for b in range(case.B):
        at = (family, th[b], 6, 4, r["x"][b], r["y"][b], r["s"][b])
        assert _rel(_lapack_vjp(*at, gx[b], gy[b], gs[b]), ipm_ref.vjp(*at, gx[b], gy[b], gs[b])) <= 1e-12
        assert _rel(_lapack_jvp(*at, td[b]), ipm_ref.jvp(*at, td[b])) <= 1e-12


@pytest.mark.parametrize("case", _params([c for c in SENS_CASES if c.cpu]))
def test_oracle_sensitivities_match_lapack_beyond_one_wave(oracle_lib, case):
    """oracle vjp_batch / jvp_batch against the dense LAPACK closed form, every instance,
    within 1e-8.  Observed: ≤ 1e-13."""
    fam, n, m = case.family, case.n, case.m
    th, (gx, gy, gs), td = case.inputs()
    r = _oracle_point(oracle_lib, case)
    assert np.all(r["status"] == 0)
    dth, st = oracle_lib.vjp_batch(fam, n, m, th, r["x"], r["y"], r["s"], gx, gy, gs, nthreads=8)
    zd, stj = oracle_lib.jvp_batch(fam, n, m, th, r["x"], r["y"], r["s"], td, nthreads=8)
    assert np.all(st == 0) and np.all(stj == 0)
    worst = 0.0
    for b in range(case.B):
        at = (fam, th[b], n, m, r["x"][b], r["y"][b], r["s"][b])
        dv = _rel(dth[b], _lapack_vjp(*at, gx[b], gy[b], gs[b]))
        dj = _rel(zd[b], _lapack_jvp(*at, td[b]))
        worst = max(worst, dv, dj)
        assert dv <= BAR and dj <= BAR, (b, dv, dj)
    print(f"{case.id}: worst relative difference {worst:.2e}")


# ---------------------------------------------------------------- GPU: every kernel against the oracle


def _first(r, B):
    return {k: (v[:B] if isinstance(v, np.ndarray) else v) for k, v in r.items()}


@pytest.mark.gpu
@pytest.mark.parametrize("case", [pytest.param(c, id=c.id) for c in SOLVE_CASES])
def test_workgroup_solve_kernels_vs_oracle(gpu, oracle_lib, case):
    """Each solve case of the table through the default (AUTO) selector: every instance
    solved, every output bit-identical to the oracle."""
    from mcp_amd.batch import solve_batch

    B = case.gpu_B(kernel_constants()["buckets"])
    th, start = case.inputs()
    ref = _first(_oracle_solve(oracle_lib, case), B)
    got = solve_batch(case.family, case.n, case.m, th[:B], tol=1e-6, linear_solver=case.solver, trace_len=TRACE,
                      **{k: v[:B] for k, v in start.items()})
    assert np.all(got["status"] == 0)
    assert_bit_exact(got, ref)


@pytest.mark.gpu
def test_qp_schur_bucket_512_lu_fallback(gpu, oracle_lib):
    """n = 128, m = 66 (bucket 512, A read from θ) with M not symmetric: every Newton step takes
    the pivoting LU instead of the Gauss-Jordan."""
    from mcp_amd.batch import solve_batch

    n, m, B = 128, 66, 2
    th = feasible_qp_theta(np.random.default_rng(7), n, m, B)
    th[:, 1] += 1e-3  # M_21 ≠ M_12
    ref = oracle_lib.solve_batch(QP, n, m, th, tol=1e-6, linear_solver="schur", trace_len=TRACE, nthreads=8)
    got = solve_batch(QP, n, m, th, tol=1e-6, linear_solver="schur", trace_len=TRACE)
    assert_bit_exact(got, ref)


@pytest.mark.gpu
def test_qp_schur_workgroup_queue_longer_than_grid(gpu, oracle_lib):
    """1500 small instances forced onto the Gauss-Jordan workgroup kernel: more than the
    resident workgroups, so each takes several instances off the work queue.  The same
    bits as the oracle and as the one-wave kernel."""
    from mcp_amd.batch import solve_batch
    from mcp_amd.qp_benchmark import generate_random_parameter

    n, m, B = 6, 4, 1500
    th = generate_random_parameter(np.random.default_rng(7), n, m, 0.0, batch=B)
    ref = oracle_lib.solve_batch(QP, n, m, th, tol=1e-6, linear_solver="schur", trace_len=TRACE, nthreads=8)
    got = solve_batch(QP, n, m, th, tol=1e-6, linear_solver="schur", trace_len=TRACE, kernel="workgroup")
    assert_bit_exact(got, ref)
    wave = solve_batch(QP, n, m, th, tol=1e-6, linear_solver="schur", trace_len=TRACE, kernel="wave")
    assert_bit_exact(got, wave)


@pytest.mark.gpu
@pytest.mark.parametrize("case", [pytest.param(c, id=c.id) for c in SENS_CASES if c.gpu])
def test_workgroup_sensitivity_kernels_vs_oracle(gpu, oracle_lib, case):
    """The workgroup VJP (gx, gy, gs all given) and JVP (K = 9 partials: MCPX_JVP_RHS of them,
    then one more in a second factorisation; 3 at N = 768) of every bucket and family,
    bit-identical to the oracle; cond_batch at the case that asks for it."""
    from mcp_amd.batch import cond_batch, jvp_batch, vjp_batch

    fam, n, m = case.family, case.n, case.m
    th, (gx, gy, gs), td = case.inputs()
    r = _oracle_point(oracle_lib, case)
    assert np.all(r["status"] == 0)
    at = (fam, n, m, th, r["x"], r["y"], r["s"])
    dth, st = vjp_batch(*at, gx, gy, gs)
    rdth, rst = oracle_lib.vjp_batch(*at, gx, gy, gs, nthreads=8)
    np.testing.assert_array_equal(st, rst)
    assert np.all(st == 0) and _same(dth, rdth)
    zd, stj = jvp_batch(*at, td)
    rzd, rstj = oracle_lib.jvp_batch(*at, td, nthreads=8)
    np.testing.assert_array_equal(stj, rstj)
    assert np.all(stj == 0) and _same(zd, rzd)
    if case.cond:
        rc, cst = cond_batch(*at)
        rrc, rcst = oracle_lib.cond_batch(*at, nthreads=8)
        np.testing.assert_array_equal(cst, rcst)
        assert np.array_equal(rc.view(np.int64), rrc.view(np.int64)), np.abs(rc - rrc).max()

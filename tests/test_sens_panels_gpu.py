"""Sensitivity kernels of generated modules on the 8- and 4-column LU panels (GPU part).

A module whose 16-column panel does not fit the LDS runs its pullback / tangent / rcond kernels
on a panel of 8 or 4 columns (csrc/ipm_nl_kernel.hpp MCPX_NL_SENS_NB_*).  Every entry of the
elimination sees the same k-ascending fma chain at every width, so the results are the oracle's
bit for bit (oracle_{vjp,jvp,cond}_batch_nl), through the C ABI:

* the lane change at T = 2 with the panel capped at 8 and at 4 (backend_options
  "sens_panel_max") on the 1,024 games of the bench's θ stream, failed games included;
* T = 15 (tangents and rcond on 8 columns; the pullback still runs 16);
* T = 21 (pullback and tangents on 8 columns), and rrule(solve, game, θ) through it.
The CPU part is tests/test_sens_panels.py."""

from __future__ import annotations

import numpy as np
import pytest

from mcp_amd import _abi
from mcp_amd.lane_change import LaneChangeGame
from tests.test_sensitivity import _same
from tests.test_sensitivity_nl import _gpu_vs_oracle_nl


def _bench_theta(game, B):
    from mcp_amd.qp_benchmark import chunked_slice

    th = chunked_slice(lambda rng, k: game.generate_random_parameter(rng, k), 1, 0, B)
    return np.ascontiguousarray(game.mcp.theta_map(th))


def _solve(game, tp):
    from mcp_amd.batch import solve_batch

    nl = game.mcp.nl
    return solve_batch(_abi.FAMILY_NONLINEAR, nl.n, nl.m, tp, linear_solver="schur", tol=1e-6, module=game.mcp.module())


@pytest.fixture(scope="module")
def c4(gpu, oracle_lib):
    """The 1,024 bench games at T = 2 solved once (default module), cotangents / tangents drawn
    once, and the oracle's pullback, 10 tangents and rcond of every game: shared, never written."""
    game = LaneChangeGame(2)
    nl = game.mcp.nl
    tp = _bench_theta(game, 1024)
    r = _solve(game, tp)
    assert (r["status"] != 0).sum() >= 10  # failed games (NaN iterates, status 1) are in the batch
    rng = np.random.default_rng(21)
    g = [rng.standard_normal((1024, k)) for k in (nl.n, nl.m, nl.m)]
    td = rng.standard_normal((1024, 10, nl.p))
    z = (r["x"], r["y"], r["s"])
    ref = dict(vjp=oracle_lib.vjp_batch_nl(nl, tp, *z, *g, nthreads=8),
               jvp=oracle_lib.jvp_batch_nl(nl, tp, *z, td, nthreads=8),
               cond=oracle_lib.cond_batch(0, 0, 0, tp, *z, nthreads=8, nl=nl))
    return dict(tp=tp, z=z, g=g, td=td, ref=ref)


@pytest.mark.gpu
@pytest.mark.parametrize("cap", [8, 4])
def test_gpu_capped_panel_bit_exact_on_the_bench_games(gpu, c4, cap):
    from mcp_amd.batch import cond_batch, jvp_batch, vjp_batch

    mcp = LaneChangeGame(2, backend_options={"sens_panel_max": cap}).mcp
    assert mcp.nl.sens_panels() == {"vjp": cap, "jvp": cap}
    mod = mcp.module()
    assert mod.has_vjp and mod.has_jvp
    tp, z = c4["tp"], c4["z"]
    for name, got in (("vjp", vjp_batch(_abi.FAMILY_NONLINEAR, 40, 50, tp, *z, *c4["g"], module=mod)),
                      ("jvp", jvp_batch(_abi.FAMILY_NONLINEAR, 40, 50, tp, *z, c4["td"], module=mod)),
                      ("cond", cond_batch(_abi.FAMILY_NONLINEAR, 40, 50, tp, *z, module=mod))):
        ref = c4["ref"][name]
        np.testing.assert_array_equal(got[1], ref[1], err_msg=f"{name} status, panel {cap}")
        assert _same(got[0], ref[0]), (name, cap)


@pytest.mark.gpu
def test_gpu_cap4_null_cotangent(gpu, oracle_lib):
    game = LaneChangeGame(2, backend_options={"sens_panel_max": 4})
    th = game.generate_random_parameter(np.random.default_rng(8), 64)
    tp = np.ascontiguousarray(game.mcp.theta_map(th))
    r = _solve(game, tp)
    _gpu_vs_oracle_nl(oracle_lib, game.mcp, tp, r["x"], r["y"], r["s"], np.random.default_rng(9), K=1, null="gy")


@pytest.mark.gpu
def test_gpu_t15_tangents_and_rcond_on_8_columns(gpu, oracle_lib):
    """T = 15 (n = 300, m = 375): the 1,050-row tangent system does not fit 16 columns."""
    from mcp_amd.batch import cond_batch, jvp_batch

    game = LaneChangeGame(15)
    nl = game.mcp.nl
    assert nl.sens_panels() == {"vjp": 16, "jvp": 8} and not nl.wg_solvers()["dense"]
    tp = _bench_theta(game, 4)
    r = _solve(game, tp)
    z = (r["x"], r["y"], r["s"])
    td = np.random.default_rng(15).standard_normal((4, 3, nl.p))
    zd, st = jvp_batch(_abi.FAMILY_NONLINEAR, nl.n, nl.m, tp, *z, td, module=game.mcp.module())
    rzd, rst = oracle_lib.jvp_batch_nl(nl, tp, *z, td, nthreads=8)
    np.testing.assert_array_equal(st, rst)
    assert _same(zd, rzd)
    rc, cst = cond_batch(_abi.FAMILY_NONLINEAR, nl.n, nl.m, tp, *z, module=game.mcp.module())
    rrc, rcst = oracle_lib.cond_batch(0, 0, 0, tp, *z, nthreads=8, nl=nl)
    np.testing.assert_array_equal(cst, rcst)
    assert _same(rc, rrc)


@pytest.fixture(scope="module")
def t21():
    return LaneChangeGame(21)


@pytest.mark.gpu
def test_gpu_t21_pullback_and_tangent_on_8_columns(gpu, oracle_lib, t21):
    """T = 21 (n = 420, m = 525): neither the 945-row adjoint system nor the 1,470-row tangent
    system fits 16 columns."""
    nl = t21.mcp.nl
    assert nl.sens_panels() == {"vjp": 8, "jvp": 8} and not nl.wg_solvers()["reduced"]
    tp = _bench_theta(t21, 3)
    r = _solve(t21, tp)
    _gpu_vs_oracle_nl(oracle_lib, t21.mcp, tp, r["x"], r["y"], r["s"], np.random.default_rng(22), K=1)


@pytest.mark.gpu
def test_gpu_t21_rrule_through_the_game(gpu, oracle_lib, t21):
    """rrule(solve, game, θ) (the Zygote path of examples/utils.jl:233-269) past the horizon where
    the pullback kernel used to be missing: ∂θ is the oracle's."""
    from mcp_amd.api import solve
    from mcp_amd.autodiff import rrule

    th = t21.generate_random_parameter(np.random.default_rng(1), 4)[1]
    x0 = t21.initial_guess(th[None])[0]
    sol, back = rrule(solve, t21.game, th, x0=x0, tol=1e-8, linear_solve_algorithm="schur")
    w = np.random.default_rng(2).standard_normal(t21.primal_dim)
    _, _, dθ = back({"primals": [w, None]})
    nl = t21.mcp.nl
    gx = np.zeros((1, nl.n))
    gx[0, :t21.primal_dim] = w
    rdθ, _ = oracle_lib.vjp_batch_nl(nl, th[None], sol.variables["x"][None], sol.variables["y"][None],
                                     sol.variables["s"][None], gx)
    assert _same(dθ, rdθ[0])

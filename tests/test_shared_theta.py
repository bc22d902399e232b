"""Shared-matrix batches without a GPU: the split dimensions, the argument checks of
mcpx_solve_batch_shared[_device] through ctypes, and ThetaMap.split / PrimalDualMCP.shared_split
(the front end's decision between the split and the full-θ path)."""

from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

from mcp_amd import _abi
from mcp_amd._lib import lib
from mcp_amd.api import PrimalDualMCP

# test/runtests.jl:8-26 (integer data, as the reference's test and tests/test_api.py write it)
M2 = np.array([[2, 1], [1, 2]])
A2 = np.array([[1, 0], [0, 1]])
B2 = np.array([1, 1])


def readme_qp():
    """README.md:51-66 / test/runtests.jl:8-26: θ enters ϕ only."""
    return PrimalDualMCP(lambda x, y, θ: M2 @ x - θ - A2.T @ y, lambda x, y, θ: A2 @ x - B2,
                         unconstrained_dimension=2, constrained_dimension=2, parameter_dimension=2)


MQ = np.array([[3.0, 0.5, 0.0], [0.5, 2.0, -0.25], [0.0, -0.25, 1.5]])
AQ = np.array([[1.0, -1.0, 0.0], [0.5, 0.0, 2.0]])


def vector_qp():
    """n = 3, m = 2, θ ∈ R⁵ in b and ϕ only (scaled, shifted and summed entries)."""
    def G(x, y, θ):
        return MQ @ x - np.array([θ[2], 2 * θ[3] + 1.0, θ[4] - θ[2]]) - AQ.T @ y

    def H(x, y, θ):
        return AQ @ x - np.array([θ[0] + 0.5, -θ[1]])

    return PrimalDualMCP(G, H, unconstrained_dimension=3, constrained_dimension=2, parameter_dimension=5)


def matrix_mcp():
    """M[0, 0] = 2 + θ₁: the matrix block depends on θ, so there is no split."""
    def G(x, y, θ):
        return np.array([(2 + θ[0]) * x[0] + x[1], x[0] + 2 * x[1]]) - θ - y

    return PrimalDualMCP(G, lambda x, y, θ: x - B2, unconstrained_dimension=2, constrained_dimension=2,
                         parameter_dimension=2)


@pytest.mark.parametrize("fam,n,m", [(0, 2, 2), (0, 32, 16), (1, 4, 8)])
def test_split_dimensions_add_up(fam, n, m):
    L = lib()
    ds, dv = L.mcpx_theta_shared_dim(fam, n, m), L.mcpx_theta_var_dim(fam, n, m)
    assert ds + dv == L.mcpx_theta_dim(fam, n, m)
    assert dv == n + m
    assert (ds, dv) == (_abi.theta_shared_dim(fam, n, m), _abi.theta_var_dim(fam, n, m))


def test_split_dimensions_reject_bad_input():
    L = lib()
    for f in (L.mcpx_theta_shared_dim, L.mcpx_theta_var_dim):
        assert f(9, 2, 2) < 0 and f(_abi.FAMILY_NONLINEAR, 2, 2) < 0
        assert f(0, -1, 2) < 0 and f(1, 2, -1) < 0


def _call(desc, shared, var, params, device=False):
    """mcpx_solve_batch_shared (or _device with host pointers: only its checks run) → code."""
    B = max(desc.batch, 1)
    outs = [np.empty(B * 64) for _ in range(5)] + [np.empty(B, np.int32) for _ in range(2)]
    o = _abi.Out(*[a.ctypes.data for a in outs], None, None, None, 0, 0)
    ptr = lambda a: None if a is None else a.ctypes.data
    if device:
        return lib().mcpx_solve_batch_shared_device(C.byref(desc), ptr(shared), ptr(var), None, None, None,
                                                    C.byref(params), C.byref(o), None)
    return lib().mcpx_solve_batch_shared(C.byref(desc), ptr(shared), ptr(var), None, None, None, C.byref(params), 1,
                                         C.byref(o))


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_argument_errors(device):
    n, m = 2, 2
    sh, var, prm = np.zeros(_abi.theta_shared_dim(0, n, m)), np.zeros(n + m), _abi.make_params()
    ok = _abi.Desc(0, n, m, 0, 1, n + m)
    assert _call(ok, None, var, prm, device) == _abi.MCPX_EINVAL  # NULL shared
    assert lib().mcpx_last_error()
    assert _call(ok, sh, None, prm, device) == _abi.MCPX_EINVAL  # NULL var
    assert _call(_abi.Desc(_abi.FAMILY_NONLINEAR, n, m, 0, 1, n + m), sh, var, prm, device) == _abi.MCPX_EINVAL
    assert _call(_abi.Desc(0, n, m, 0, 1, n + m - 1), sh, var, prm, device) == _abi.MCPX_EINVAL  # theta_ld < n + m
    assert _call(_abi.Desc(0, 400, 200, 0, 1, 600), sh, var, prm, device) == _abi.MCPX_EUNSUPPORTED
    assert _call(ok, sh, var, _abi.make_params(linear_solver=9), device) == _abi.MCPX_EINVAL
    # an empty batch reads nothing (NULL blocks included) and needs no device
    assert _call(_abi.Desc(0, n, m, 0, 0, n + m), None, None, prm, device) == _abi.MCPX_OK


def test_theta_ld_counts_the_var_block_only():
    """theta_ld = n + m is valid here (it would be too short for mcpx_solve_batch's θ′): with no
    device the valid call gets as far as MCPX_ENODEV, with one it solves."""
    n, m = 2, 2
    sh = np.concatenate([M2.flatten("F"), A2.flatten("F")]).astype(np.float64)
    var = np.array([1.0, 1.0, -0.5, 0.5])
    want = _abi.MCPX_OK if lib().mcpx_device_count() > 0 else _abi.MCPX_ENODEV
    for device in (False,) if want == _abi.MCPX_OK else (False, True):
        assert _call(_abi.Desc(0, n, m, 0, 1, n + m), sh, var, _abi.make_params(), device) == want


@pytest.mark.parametrize("make", [readme_qp, vector_qp])
def test_theta_map_splits_constant_matrices(make):
    mcp = make()
    n, m = mcp.unconstrained_dimension, mcp.constrained_dimension
    assert mcp.family == _abi.FAMILY_QP
    split = mcp.shared_split()
    assert split is not None
    shared, var_map = split
    D = _abi.theta_shared_dim(mcp.family, n, m)
    assert shared.shape == (D,) and var_map.p_out == n + m and var_map.p_in == mcp.parameter_dimension
    th = np.random.default_rng(3).standard_normal((5, mcp.parameter_dimension))
    full = mcp.theta_map(th)
    var = var_map(th)
    assert var.shape == (5, n + m)
    # bit for bit: shared ‖ var_map(θ) is theta_map(θ)
    assert np.array_equal(np.concatenate([np.broadcast_to(shared, (5, D)), var], 1), full)
    assert np.array_equal(var, full[:, D:])
    assert np.array_equal(var_map(th[0]), full[:1, D:])  # a single θ


def test_split_of_the_readme_qp_is_its_matrices():
    shared, _ = readme_qp().shared_split()
    assert np.array_equal(shared, np.concatenate([M2.flatten("F"), A2.flatten("F")]))


def test_theta_dependent_matrix_has_no_split():
    """api.solve decides by this return value: None sends the MCP down the full-θ path."""
    mcp = matrix_mcp()
    assert mcp.family == _abi.FAMILY_QP
    assert mcp.theta_map.split(_abi.theta_shared_dim(0, 2, 2)) is None
    assert mcp.shared_split() is None


def test_lambdified_matrix_entry_has_no_split():
    """A non-polynomial θ term in the matrix block is θ-dependent too (the lambdified terms)."""
    def G(x, y, θ):
        import sympy

        return np.array([(2 + sympy.exp(θ[0])) * x[0], 2 * x[1]]) - θ - y

    mcp = PrimalDualMCP(G, lambda x, y, θ: x - B2, unconstrained_dimension=2, constrained_dimension=2,
                        parameter_dimension=2)
    assert mcp.family != _abi.FAMILY_NONLINEAR and mcp.shared_split() is None


def test_affine_family_splits_at_its_own_offset():
    """G = P x + Q y + g(θ), H = R x + S y + h(θ) with −Q ≠ Rᵀ: affine family, [g; h] per instance."""
    def G(x, y, θ):
        return np.array([2.0 * x[0] + x[1] - 0.5 * y[0] + θ[0], x[0] + 3.0 * x[1] + θ[1] * 2.0])

    mcp = PrimalDualMCP(G, lambda x, y, θ: np.array([x[0] + 0.25 * y[0] - θ[2]]), unconstrained_dimension=2,
                        constrained_dimension=1, parameter_dimension=3)
    assert mcp.family == _abi.FAMILY_AFFINE
    shared, var_map = mcp.shared_split()
    D = _abi.theta_shared_dim(1, 2, 1)
    th = np.random.default_rng(4).standard_normal((5, 3))
    assert shared.shape == (D,) and np.array_equal(var_map(th), mcp.theta_map(th)[:, D:])
    assert np.array_equal(np.broadcast_to(shared, (5, D)), mcp.theta_map(th)[:, :D])


def test_nonlinear_family_has_no_split():
    mcp = PrimalDualMCP(lambda x, y, θ: x ** 3 - θ, lambda x, y, θ: x - y, unconstrained_dimension=1,
                        constrained_dimension=1, parameter_dimension=1)
    assert mcp.family == _abi.FAMILY_NONLINEAR and mcp.shared_split() is None


def test_python_entry_rejects_a_wrong_shared_block():
    from mcp_amd.batch import solve_batch_shared

    with pytest.raises(ValueError):
        solve_batch_shared(0, 2, 2, np.zeros(7), np.zeros((1, 4)))

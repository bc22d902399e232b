"""Sensitivities of shared-matrix batches without a GPU: the five split entry points exist
(header, export list, library), their argument checks through ctypes, and the front end's
chain rule through ThetaMap.split — var_map.vjp / var_map.jvp are the full map's, bit for bit,
on the per-instance block, and the full map's tangent of the matrix block is zero."""

from __future__ import annotations

import ctypes as C
import os
import re

import numpy as np
import pytest

from mcp_amd import _abi
from mcp_amd._lib import EXPORTS, lib
from mcp_amd.api import PrimalDualMCP
from tests.test_shared_theta import readme_qp, vector_qp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("mcpx_vjp_batch_shared", "mcpx_vjp_batch_shared_device", "mcpx_jvp_batch_shared",
         "mcpx_jvp_batch_shared_device", "mcpx_solve_vjp_batch_shared_device")
EINVAL, EUNSUPPORTED, ENODEV, OK = _abi.MCPX_EINVAL, _abi.MCPX_EUNSUPPORTED, _abi.MCPX_ENODEV, _abi.MCPX_OK


def affine_mcp():
    """The affine MCP of tests/test_shared_theta.py (−Q ≠ Rᵀ): [g; h] per instance."""
    def G(x, y, θ):
        return np.array([2.0 * x[0] + x[1] - 0.5 * y[0] + θ[0], x[0] + 3.0 * x[1] + θ[1] * 2.0])

    return PrimalDualMCP(G, lambda x, y, θ: np.array([x[0] + 0.25 * y[0] - θ[2]]), unconstrained_dimension=2,
                         constrained_dimension=1, parameter_dimension=3)


def test_entry_points_are_declared_exported_and_defined():
    header = open(os.path.join(ROOT, "include", "mcpx.h")).read()
    L = lib()
    for name in NAMES:
        assert re.search(r"\bint\s+%s\s*\(" % name, header), f"{name} is not declared in include/mcpx.h"
        assert name in EXPORTS
        assert getattr(L, name) is not None  # ctypes raises AttributeError for an undefined symbol
    assert L.mcpx_version() == 20200  # added without a version step


# ---- argument checks -----------------------------------------------------------

class Call:
    """One of the four pure sensitivity entries on host arrays (the device entries see host
    pointers: only their checks run).  kw overrides an argument by name; None is NULL."""

    def __init__(self, jvp: bool, device: bool):
        self.jvp, self.device = jvp, device

    def __call__(self, desc, K=2, **kw):
        n, m, B = max(desc.n, 1), max(desc.m, 1), max(int(desc.batch), 1)
        a = dict(shared=np.zeros(16), x=np.zeros(B * n), y=np.ones(B * m), s=np.ones(B * m),
                 out=np.zeros(B * max(K, 1) * (n + 2 * m)), status=np.zeros(B, np.int32),
                 var_dot=np.zeros(B * max(K, 1) * (n + m)))
        a.update(kw)
        p = lambda k: None if a[k] is None else a[k].ctypes.data
        L, d = lib(), C.byref(desc)
        if self.jvp:
            head = (d, p("shared"), p("x"), p("y"), p("s"), int(K), p("var_dot"))
            if self.device:
                return L.mcpx_jvp_batch_shared_device(*head, p("out"), p("status"), None)
            return L.mcpx_jvp_batch_shared(*head, 1, p("out"), p("status"))
        head = (d, p("shared"), p("x"), p("y"), p("s"), None, None, None)
        if self.device:
            return L.mcpx_vjp_batch_shared_device(*head, p("out"), p("status"), None)
        return L.mcpx_vjp_batch_shared(*head, 1, p("out"), p("status"))


def fused_call(desc, shared=True, var=True, out=True, dvar=True, ct=True, prm=None):
    """mcpx_solve_vjp_batch_shared_device on host pointers (its checks only) → code."""
    buf = np.zeros(256)
    ptr = buf.ctypes.data
    o = _abi.Out(*([ptr] * 8), None, None, 0, 0) if out else _abi.Out(None, *([ptr] * 7), None, None, 0, 0)
    cot = _abi.Cotangent(2.0, 2.0, 0.0, None, None, None)
    prm = prm or _abi.make_params(linear_solver="schur")
    return lib().mcpx_solve_vjp_batch_shared_device(
        C.byref(desc), ptr if shared else None, ptr if var else None, None, None, None, C.byref(prm), C.byref(o),
        C.byref(cot) if ct else None, ptr if dvar else None, None, None)


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("jvp", [False, True], ids=["vjp", "jvp"])
def test_argument_errors(jvp, device):
    call = Call(jvp, device)
    n, m = 2, 2
    ok = _abi.Desc(0, n, m, 0, 1, n + m)
    assert call(ok, shared=None) == EINVAL
    assert lib().mcpx_last_error()
    assert call(ok, out=None) == EINVAL
    for k in ("x", "y", "s"):
        assert call(ok, **{k: None}) == EINVAL, k
    assert call(_abi.Desc(_abi.FAMILY_NONLINEAR, n, m, 0, 1, n + m)) == EINVAL
    assert call(_abi.Desc(0, n, m, 0, 1, n + m - 1)) == EINVAL  # theta_ld < var_dim
    assert call(_abi.Desc(1, n, m, 0, 1, n + m - 1)) == EINVAL
    assert call(_abi.Desc(0, 400, 200, 0, 1, 600)) == EUNSUPPORTED  # n + 2m = 800 > 768
    if jvp:
        assert call(ok, K=-1) == EINVAL
        assert call(ok, K=2, var_dot=None) == EINVAL
    # an empty batch reads nothing (NULL blocks included) and needs no device
    assert call(_abi.Desc(0, n, m, 0, 0, n + m), shared=None, x=None, y=None, s=None, out=None) == OK
    assert call(_abi.Desc(1, n, m, 0, 0, n + m), shared=None, out=None) == OK


def test_fused_argument_errors():
    n, m = 2, 2
    ok = _abi.Desc(0, n, m, 0, 1, n + m)
    assert fused_call(ok, shared=False) == EINVAL
    assert fused_call(ok, var=False) == EINVAL
    assert fused_call(ok, dvar=False) == EINVAL
    assert fused_call(ok, out=False) == EINVAL
    assert fused_call(ok, ct=False) == EINVAL
    assert fused_call(_abi.Desc(_abi.FAMILY_NONLINEAR, n, m, 0, 1, n + m)) == EINVAL
    assert fused_call(_abi.Desc(0, n, m, 0, 1, n + m - 1)) == EINVAL
    assert fused_call(_abi.Desc(0, 400, 200, 0, 1, 600), prm=_abi.make_params()) == EUNSUPPORTED
    assert fused_call(ok, prm=_abi.make_params(linear_solver=9)) == EINVAL
    assert fused_call(_abi.Desc(0, n, m, 0, 0, n + m), shared=False, var=False, dvar=False) == OK


def test_valid_calls_need_a_device():
    """No CPU fallback: with no device a valid call ends in MCPX_ENODEV (theta_ld = n + m, too short
    for a full θ′, is valid here); with one, the host entries run (the device entries would be
    handed host pointers: the GPU suite runs those)."""
    ok = _abi.Desc(0, 2, 2, 0, 1, 4)
    if lib().mcpx_device_count() > 0:
        assert Call(False, False)(ok) == OK and Call(True, False)(ok) == OK
        return
    for jvp in (False, True):
        for device in (False, True):
            assert Call(jvp, device)(ok) == ENODEV
    assert fused_call(ok) == ENODEV


# ---- the chain rule through the split map ------------------------------------------

@pytest.mark.parametrize("make", [readme_qp, vector_qp, affine_mcp])
def test_var_map_is_the_full_map_on_the_per_instance_block(make):
    mcp = make()
    n, m = mcp.unconstrained_dimension, mcp.constrained_dimension
    D = _abi.theta_shared_dim(mcp.family, n, m)
    shared, var_map = mcp.shared_split()
    rng = np.random.default_rng(11)
    B, K, p = 5, 3, mcp.parameter_dimension
    th = rng.standard_normal((B, p))
    d = rng.standard_normal((B, n + m))
    padded = np.concatenate([np.zeros((B, D)), d], 1)
    assert np.array_equal(var_map.vjp(th, d), mcp.theta_map.vjp(th, padded))
    tdot = rng.standard_normal((B, K, p))
    full = mcp.theta_map.jvp(th, tdot)
    assert np.array_equal(var_map.jvp(th, tdot), full[..., D:])
    assert not full[..., :D].any()  # the matrix block's tangent: all zero


def test_python_entries_reject_a_wrong_shared_block():
    from mcp_amd import batch

    x, y = np.zeros((1, 2)), np.ones((1, 2))
    with pytest.raises(ValueError):
        batch.vjp_batch_shared(0, 2, 2, np.zeros(7), x, y, y)
    with pytest.raises(ValueError):
        batch.jvp_batch_shared(0, 2, 2, np.zeros(9), x, y, y, np.zeros((1, 1, 4)))
    for name in ("vjp_batch_shared_device", "jvp_batch_shared_device", "solve_vjp_batch_shared_device"):
        assert callable(getattr(batch, name))

"""Tangents of the shared block and the condition estimate of shared-matrix batches, without a
GPU: the four entry points exist (header, export list, library), their argument checks through
ctypes — each before any device work — and the shape checks of the Python wrappers."""

from __future__ import annotations

import ctypes as C
import os
import re

import numpy as np
import pytest

from mcp_amd import _abi
from mcp_amd._lib import EXPORTS, lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("mcpx_jvp_batch_shared_dot", "mcpx_jvp_batch_shared_dot_device", "mcpx_cond_batch_shared",
         "mcpx_cond_batch_shared_device")
EINVAL, EUNSUPPORTED, ENODEV, OK = _abi.MCPX_EINVAL, _abi.MCPX_EUNSUPPORTED, _abi.MCPX_ENODEV, _abi.MCPX_OK


def test_entry_points_are_declared_exported_and_defined():
    header = open(os.path.join(ROOT, "include", "mcpx.h")).read()
    L = lib()
    for name in NAMES:
        assert re.search(r"\bint\s+%s\s*\(" % name, header), f"{name} is not declared in include/mcpx.h"
        assert name in EXPORTS
        assert getattr(L, name) is not None  # ctypes raises AttributeError for an undefined symbol
    assert L.mcpx_version() == 20200  # added without a version step
    assert "No mcpx_cond_batch on a split" not in header


class Call:
    """One of the four entries on host arrays (the device entries see host pointers: only their
    checks run).  kw overrides an argument by name; None is NULL."""

    def __init__(self, jvp: bool, device: bool):
        self.jvp, self.device = jvp, device

    def __call__(self, desc, K=2, **kw):
        n, m, B = max(desc.n, 1), max(desc.m, 1), max(int(desc.batch), 1)
        a = dict(shared=np.zeros(16), x=np.zeros(B * n), y=np.ones(B * m), s=np.ones(B * m),
                 out=np.zeros(B * max(K, 1) * (n + 2 * m)), status=np.zeros(B, np.int32),
                 shared_dot=np.zeros(max(K, 1) * 16), var_dot=np.zeros(B * max(K, 1) * (n + m)))
        a.update(kw)
        p = lambda k: None if a[k] is None else a[k].ctypes.data
        L, d = lib(), C.byref(desc)
        if self.jvp:
            head = (d, p("shared"), p("x"), p("y"), p("s"), int(K), p("shared_dot"), p("var_dot"))
            if self.device:
                return L.mcpx_jvp_batch_shared_dot_device(*head, p("out"), p("status"), None)
            return L.mcpx_jvp_batch_shared_dot(*head, 1, p("out"), p("status"))
        head = (d, p("shared"), p("x"), p("y"), p("s"))
        if self.device:
            return L.mcpx_cond_batch_shared_device(*head, p("out"), p("status"), None)
        return L.mcpx_cond_batch_shared(*head, 1, p("out"), p("status"))


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("jvp", [False, True], ids=["cond", "jvp"])
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
        assert call(ok, K=2, shared_dot=None) == EINVAL
        assert b"shared_dot" in lib().mcpx_last_error()
        assert call(ok, K=2, shared_dot=None, var_dot=None) == EINVAL
        assert call(ok, K=-1) == EINVAL  # as mcpx_jvp_batch_shared
    # an empty batch reads nothing (NULL blocks included) and needs no device
    assert call(_abi.Desc(0, n, m, 0, 0, n + m), shared=None, x=None, y=None, s=None, out=None, shared_dot=None,
                var_dot=None) == OK
    assert call(_abi.Desc(1, n, m, 0, 0, n + m), shared=None, out=None) == OK


def test_valid_calls_need_a_device():
    """No CPU fallback: with no device a valid call ends in MCPX_ENODEV — a NULL var_dot is valid;
    with one, the host entries run (the GPU suite runs the device entries)."""
    ok = _abi.Desc(0, 2, 2, 0, 1, 4)
    if lib().mcpx_device_count() > 0:
        assert Call(False, False)(ok) == OK and Call(True, False)(ok) == OK and Call(True, False)(ok, var_dot=None) == OK
        return
    for jvp in (False, True):
        for device in (False, True):
            assert Call(jvp, device)(ok) == ENODEV
    assert Call(True, False)(ok, var_dot=None) == ENODEV
    assert Call(True, True)(ok, var_dot=None) == ENODEV


def test_python_wrappers_check_shapes():
    from mcp_amd import autodiff, batch

    n, m = 2, 2
    D = _abi.theta_shared_dim(0, n, m)
    sh, x, y = np.zeros(D), np.zeros((3, n)), np.ones((3, m))
    with pytest.raises(ValueError):  # a wrong shared block
        batch.jvp_batch_shared(0, n, m, np.zeros(D + 1), x, y, y, None, shared_dot=np.zeros((2, D)))
    with pytest.raises(ValueError):  # shared_dot is not K rows of shared_dim
        batch.jvp_batch_shared(0, n, m, sh, x, y, y, None, shared_dot=np.zeros(D + 1))
    with pytest.raises(ValueError):  # K of shared_dot and of var_dot differ
        batch.jvp_batch_shared(0, n, m, sh, x, y, y, np.zeros((3, 3, n + m)), shared_dot=np.zeros((2, D)))
    with pytest.raises(ValueError):  # neither tangent
        batch.jvp_batch_shared(0, n, m, sh, x, y, y, None)
    with pytest.raises(ValueError):
        batch.cond_batch_shared(0, n, m, np.zeros(D - 1), x, y, y)
    for name in ("jvp_batch_shared_device", "cond_batch_shared_device"):
        assert callable(getattr(batch, name))
    var = np.zeros((3, n + m))
    with pytest.raises(ValueError):  # at least one of the two
        autodiff.solve_shared_dual(0, n, m, sh, var)
    with pytest.raises(ValueError):  # (shared_dim, K), not (K, shared_dim)
        autodiff.solve_shared_dual(0, n, m, sh, var, shared_partials=np.zeros((3, D)))
    with pytest.raises(ValueError):  # (B, var_dim, K)
        autodiff.solve_shared_dual(0, n, m, sh, var, var_partials=np.zeros((3, 2, n + m)))
    with pytest.raises(ValueError):  # K differs
        autodiff.solve_shared_dual(0, n, m, sh, var, shared_partials=np.zeros((D, 2)),
                                   var_partials=np.zeros((3, n + m, 3)))

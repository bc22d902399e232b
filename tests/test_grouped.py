"""Grouped shared-matrix batches without a GPU (mcpx_{solve,vjp}_batch_grouped[_device],
mcpx_vjp_batch_grouped_reduce[_device]): the six entry points exist (header, export list, library,
Python bindings), their argument checks through ctypes, MCPX_ENODEV without a device, the empty
batch of the host reduce call, and the Python wrappers' own checks."""

from __future__ import annotations

import ctypes as C
import os
import re

import numpy as np
import pytest

from mcp_amd import _abi
from mcp_amd._lib import EXPORTS, lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"mcpx_solve_batch_grouped": 12, "mcpx_solve_batch_grouped_device": 12, "mcpx_vjp_batch_grouped": 14,
         "mcpx_vjp_batch_grouped_device": 14, "mcpx_vjp_batch_grouped_reduce": 18,
         "mcpx_vjp_batch_grouped_reduce_device": 18}
EINVAL, EUNSUPPORTED, ENODEV, OK = _abi.MCPX_EINVAL, _abi.MCPX_EUNSUPPORTED, _abi.MCPX_ENODEV, _abi.MCPX_OK


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def test_entry_points_are_declared_exported_and_bound():
    from mcp_amd import autodiff, batch

    header = open(os.path.join(ROOT, "include", "mcpx.h")).read()
    L = lib()
    for name, nargs in NAMES.items():
        assert re.search(r"\bint\s+%s\s*\(" % name, header), f"{name} is not declared in include/mcpx.h"
        assert name in EXPORTS
        assert getattr(L, name).restype is C.c_int
        assert len(getattr(L, name).argtypes) == nargs, name
    for name in ("solve_batch_grouped", "vjp_batch_grouped", "vjp_batch_grouped_reduce"):
        assert callable(getattr(batch, name)) and callable(getattr(batch, name + "_device"))
    assert callable(autodiff.solve_grouped_torch)
    assert L.mcpx_version() == 20200  # added without a version step


class Call:
    """One of the six entries on host arrays (a device entry sees host pointers: only its checks
    run).  kw overrides an argument by name; None is NULL."""

    def __init__(self, kind: str, device: bool):
        self.kind, self.device = kind, device

    def __call__(self, desc, **kw):
        n, m, B = max(desc.n, 1), max(desc.m, 1), max(int(desc.batch), 1)
        G = kw.pop("G", 2)
        # shared_ld = 16: the QP (2, 2) block has 8 doubles, the affine one 16
        a = dict(shared=np.zeros(3 * 16), shared_ld=16, off=np.array([0, int(desc.batch), int(desc.batch)], np.int64),
                 var=np.zeros(B * (n + m)), x=np.zeros(B * n), y=np.ones(B * m), s=np.ones(B * m), skip=None,
                 dshared=np.full(3 * 16, np.nan), dshared_ld=16, used=np.full(3, -1, np.int64),
                 dvar=np.zeros(B * (n + m)), status=np.zeros(B, np.int32), prm=_abi.make_params(), out=True)
        a.update(kw)
        self.last = a
        p = lambda k: None if a[k] is None else a[k].ctypes.data
        L, d = lib(), C.byref(desc)
        groups = (p("shared"), int(a["shared_ld"]), int(G), p("off"))
        if self.kind == "solve":
            outs = [np.empty(B * 64) for _ in range(5)] + [np.empty(B, np.int32) for _ in range(2)]
            self.keep = outs
            o = _abi.Out(*[t.ctypes.data for t in outs], None, None, None, 0, 0)
            if a["out"] is None:
                o.x = None
            prm = None if a["prm"] is None else C.byref(a["prm"])
            head = (d, *groups, p("var"), None, None, None, prm)
            if self.device:
                return L.mcpx_solve_batch_grouped_device(*head, C.byref(o), None)
            return L.mcpx_solve_batch_grouped(*head, 1, C.byref(o))
        head = (d, *groups, p("x"), p("y"), p("s"), None, None, None)
        if self.kind == "vjp":
            if self.device:
                return L.mcpx_vjp_batch_grouped_device(*head, p("dvar"), p("status"), None)
            return L.mcpx_vjp_batch_grouped(*head, 1, p("dvar"), p("status"))
        tail = (p("dshared"), int(a["dshared_ld"]), p("used"), p("dvar"), p("status"))
        if self.device:
            return L.mcpx_vjp_batch_grouped_reduce_device(*head, p("skip"), *tail, None)
        return L.mcpx_vjp_batch_grouped_reduce(*head, p("skip"), 1, *tail)


KINDS = [(k, dev) for k in ("solve", "vjp", "reduce") for dev in (False, True)]
IDS = [f"{k}-{'device' if dev else 'host'}" for k, dev in KINDS]


@pytest.mark.parametrize("kind,device", KINDS, ids=IDS)
def test_argument_errors(kind, device):
    call = Call(kind, device)
    n, m = 2, 2
    ok = _abi.Desc(0, n, m, 0, 1, n + m)
    i64 = lambda *v: np.array(v, np.int64)
    assert call(_abi.Desc(_abi.FAMILY_NONLINEAR, n, m, 0, 1, n + m)) == EINVAL
    assert lib().mcpx_last_error()
    assert call(ok, shared=None) == EINVAL
    assert call(ok, off=None) == EINVAL
    assert call(ok, G=-1) == EINVAL
    assert call(ok, G=0, off=i64(0)) == EINVAL  # no group for a non-empty batch
    assert call(_abi.Desc(0, n, m, 0, 0, n + m), G=-1) == EINVAL  # also for an empty batch
    assert call(ok, off=i64(0, 2, 1)) == EINVAL  # decreasing (and past the batch)
    assert call(_abi.Desc(0, n, m, 0, 3, n + m), off=i64(0, 3, 2, 3), G=3) == EINVAL  # decreasing inside
    assert call(ok, off=i64(1, 1, 1)) == EINVAL  # does not start at 0
    assert call(ok, off=i64(0, 0, 0)) == EINVAL  # does not end at the batch
    assert call(ok, off=i64(0, 1, 2)) == EINVAL
    assert call(ok, shared_ld=7) == EINVAL  # below shared_dim = 8
    assert call(_abi.Desc(1, n, m, 0, 1, n + m), shared_ld=15) == EINVAL  # affine: shared_dim = 16
    assert call(_abi.Desc(0, n, m, 0, 1, n + m - 1)) == EINVAL  # theta_ld < var_dim
    assert call(_abi.Desc(0, n, m, 0, -1, n + m)) == EINVAL
    if kind == "solve":
        assert call(ok, var=None) == EINVAL
        assert call(ok, out=None) == EINVAL
        assert call(ok, prm=None) == EINVAL
        assert call(ok, prm=_abi.make_params(tol=0.0)) == EINVAL
        assert call(_abi.Desc(0, 400, 200, 0, 1, 600), shared_ld=400 * 400 + 200 * 400) == EUNSUPPORTED
        return
    for k in ("x", "y", "s"):
        assert call(ok, **{k: None}) == EINVAL, k
    assert call(_abi.Desc(0, 400, 200, 0, 1, 600), shared_ld=400 * 400 + 200 * 400) == EUNSUPPORTED  # n + 2m > 768
    if kind == "vjp":
        assert call(ok, dvar=None) == EINVAL
        return
    assert call(ok, dshared=None) == EINVAL
    assert call(ok, used=None) == EINVAL
    assert call(ok, dshared_ld=7) == EINVAL
    assert call(_abi.Desc(0, n, m, 0, 0, n + m), dshared=None) == EINVAL  # also for an empty batch
    assert call(_abi.Desc(0, n, m, 0, 0, n + m), used=None) == EINVAL


@pytest.mark.parametrize("kind,device", KINDS, ids=IDS)
def test_valid_calls_need_a_device(kind, device):
    """No CPU fallback: with no device every valid non-empty call ends in MCPX_ENODEV; with one, the
    host entries run (a device entry would be handed host pointers: the GPU suite runs those)."""
    call = Call(kind, device)
    ok = _abi.Desc(0, 2, 2, 0, 1, 4)
    if lib().mcpx_device_count() > 0:
        if not device:
            assert call(ok) == OK
        return
    assert call(ok) == ENODEV
    assert call(_abi.Desc(1, 2, 2, 0, 300, 4)) == ENODEV
    if kind == "reduce":
        assert call(ok, dvar=None, status=None) == ENODEV
        assert call(ok, skip=np.zeros(1, np.uint8)) == ENODEV
        if device:  # the device entry writes device memory, even for an empty batch
            assert call(_abi.Desc(0, 2, 2, 0, 0, 4)) == ENODEV


@pytest.mark.parametrize("fam", [0, 1])
def test_empty_batch_of_the_host_reduce_is_all_zero_and_needs_no_device(fam):
    call = Call("reduce", False)
    rc = call(_abi.Desc(fam, 2, 2, 0, 0, 4), G=3, off=np.zeros(4, np.int64), shared=None, x=None, y=None, s=None,
              dvar=None, status=None)
    assert rc == OK
    D = _abi.theta_shared_dim(fam, 2, 2)
    rows = call.last["dshared"].reshape(3, 16)
    assert bits_equal(rows[:, :D], np.zeros((3, D)))  # +0.0, every group
    assert np.isnan(rows[:, D:]).all()  # the padding of dshared is not written
    assert (call.last["used"] == 0).all()
    for kind in ("solve", "vjp"):  # the other host entries: an empty batch is a no-op
        assert Call(kind, False)(_abi.Desc(fam, 2, 2, 0, 0, 4), G=3, off=np.zeros(4, np.int64)) == OK


def test_python_wrappers_reject_bad_groups_and_blocks():
    from mcp_amd import batch

    n, m, B = 2, 2, 3
    D = _abi.theta_shared_dim(0, n, m)
    x, y = np.zeros((B, n)), np.ones((B, m))
    var, sh = np.zeros((B, n + m)), np.zeros((2, D))
    with pytest.raises(ValueError, match="sum"):
        batch.solve_batch_grouped(0, n, m, sh, var, [1, 1])
    with pytest.raises(ValueError, match="sum"):
        batch.vjp_batch_grouped(0, n, m, sh, x, y, y, [2, 2])
    with pytest.raises(ValueError, match="sum"):
        batch.vjp_batch_grouped_reduce(0, n, m, sh, x, y, y, [3, 1])
    with pytest.raises(ValueError, match="non-negative"):
        batch.solve_batch_grouped(0, n, m, sh, var, [4, -1])
    for bad in (np.zeros((2, D - 1)), np.zeros((3, D)), np.zeros(2 * D)):
        with pytest.raises(ValueError, match="theta_shared"):
            batch.solve_batch_grouped(0, n, m, bad, var, [1, 2])
        with pytest.raises(ValueError, match="theta_shared"):
            batch.vjp_batch_grouped(0, n, m, bad, x, y, y, [1, 2])
        with pytest.raises(ValueError, match="theta_shared"):
            batch.vjp_batch_grouped_reduce(0, n, m, bad, x, y, y, [1, 2])

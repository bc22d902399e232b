"""The reduced gradient of a shared-matrix batch's matrix block without a GPU
(mcpx_vjp_batch_shared_reduce[_device]): the entry points exist (header, export list, library,
Python bindings), their argument checks through ctypes, the empty batch, and the test-side
restatement of the contract's fma chain (tests/helpers/shared_reduce_chain.py), which the GPU
suite compares the kernels against, checked against itself."""

from __future__ import annotations

import ctypes as C
import os
import re

import numpy as np
import pytest

from mcp_amd import _abi
from mcp_amd._lib import EXPORTS, lib
from tests.helpers import shared_reduce_chain as chain

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("mcpx_vjp_batch_shared_reduce", "mcpx_vjp_batch_shared_reduce_device")
EINVAL, EUNSUPPORTED, ENODEV, OK = _abi.MCPX_EINVAL, _abi.MCPX_EUNSUPPORTED, _abi.MCPX_ENODEV, _abi.MCPX_OK


def test_entry_points_are_declared_exported_and_bound():
    from mcp_amd import autodiff, batch

    header = open(os.path.join(ROOT, "include", "mcpx.h")).read()
    L = lib()
    for name in NAMES:
        assert re.search(r"\bint\s+%s\s*\(" % name, header), f"{name} is not declared in include/mcpx.h"
        assert name in EXPORTS
        assert getattr(L, name).restype is C.c_int
    assert len(L.mcpx_vjp_batch_shared_reduce.argtypes) == 14 == len(_abi.VJP_SHARED_REDUCE_ARGTYPES)
    assert len(L.mcpx_vjp_batch_shared_reduce_device.argtypes) == 14 == len(_abi.VJP_SHARED_REDUCE_DEVICE_ARGTYPES)
    value = int(re.search(r"#define\s+MCPX_REDUCE_CHUNK\s+(\d+)\b", header).group(1))
    assert value == _abi.REDUCE_CHUNK == chain.CHUNK
    assert value >= 64 and value & (value - 1) == 0  # a power of two, at least one wave of instances
    for name in ("vjp_batch_shared_reduce", "vjp_batch_shared_reduce_device"):
        assert callable(getattr(batch, name))
    assert callable(autodiff.solve_shared_torch)
    assert L.mcpx_version() == 20200  # added without a version step


class Call:
    """One of the two entries on host arrays (the device entry sees host pointers: only its
    checks run).  kw overrides an argument by name; None is NULL."""

    def __init__(self, device: bool):
        self.device = device

    def __call__(self, desc, **kw):
        n, m, B = max(desc.n, 1), max(desc.m, 1), max(int(desc.batch), 1)
        a = dict(shared=np.zeros(16), x=np.zeros(B * n), y=np.ones(B * m), s=np.ones(B * m), skip=None,
                 dshared=np.full(16, np.nan), used=np.full(1, -1, np.int64), dvar=np.zeros(B * (n + m)),
                 status=np.zeros(B, np.int32))
        a.update(kw)
        self.last = a
        p = lambda k: None if a[k] is None else a[k].ctypes.data
        L, d = lib(), C.byref(desc)
        head = (d, p("shared"), p("x"), p("y"), p("s"), None, None, None, p("skip"))
        tail = (p("dshared"), p("used"), p("dvar"), p("status"))
        if self.device:
            return L.mcpx_vjp_batch_shared_reduce_device(*head, *tail, None)
        return L.mcpx_vjp_batch_shared_reduce(*head, 1, *tail)


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_argument_errors(device):
    call = Call(device)
    n, m = 2, 2
    ok = _abi.Desc(0, n, m, 0, 1, n + m)
    assert call(_abi.Desc(_abi.FAMILY_NONLINEAR, n, m, 0, 1, n + m)) == EINVAL
    assert lib().mcpx_last_error()
    assert call(ok, dshared=None) == EINVAL
    assert call(ok, used=None) == EINVAL
    assert call(_abi.Desc(0, n, m, 0, 0, n + m), dshared=None) == EINVAL  # also for an empty batch
    assert call(_abi.Desc(0, n, m, 0, 0, n + m), used=None) == EINVAL
    assert call(ok, shared=None) == EINVAL
    for k in ("x", "y", "s"):
        assert call(ok, **{k: None}) == EINVAL, k
    assert call(_abi.Desc(0, n, m, 0, 1, n + m - 1)) == EINVAL  # theta_ld < var_dim
    assert call(_abi.Desc(0, n, m, 0, -1, n + m)) == EINVAL
    assert call(_abi.Desc(0, 400, 200, 0, 1, 600)) == EUNSUPPORTED  # n + 2m = 800 > 768


def test_valid_calls_need_a_device():
    """No CPU fallback: with no device every valid call ends in MCPX_ENODEV, dvar / status / skip
    given or NULL; with one, the host entry runs (the device entry would be handed host pointers:
    the GPU suite runs it)."""
    ok = _abi.Desc(0, 2, 2, 0, 1, 4)
    if lib().mcpx_device_count() > 0:
        assert Call(False)(ok) == OK
        return
    for device in (False, True):
        call = Call(device)
        assert call(ok) == ENODEV
        assert call(ok, dvar=None, status=None) == ENODEV
        assert call(ok, skip=np.zeros(1, np.uint8)) == ENODEV
        assert call(_abi.Desc(1, 2, 2, 0, 300, 4)) == ENODEV
    assert Call(True)(_abi.Desc(0, 2, 2, 0, 0, 4)) == ENODEV  # the device entry writes device memory


@pytest.mark.parametrize("fam", [0, 1])
def test_empty_batch_on_host_is_all_zero_and_needs_no_device(fam):
    call = Call(False)
    assert call(_abi.Desc(fam, 2, 2, 0, 0, 4), shared=None, x=None, y=None, s=None, dvar=None, status=None) == OK
    D = _abi.theta_shared_dim(fam, 2, 2)
    head = call.last["dshared"][:D]
    assert chain.bits_equal(head, np.zeros(D)) and np.isnan(call.last["dshared"][D:]).all()
    assert call.last["used"][0] == 0


def test_python_entries_reject_a_wrong_shared_block():
    from mcp_amd import batch

    x, y = np.zeros((1, 2)), np.ones((1, 2))
    with pytest.raises(ValueError):
        batch.vjp_batch_shared_reduce(0, 2, 2, np.zeros(7), x, y, y)


# ---- the restated chain ------------------------------------------------------------------

def random_case(rng, fam, n, m, B):
    return rng.standard_normal((B, n)), rng.standard_normal((B, m)), rng.standard_normal((B, n + m))


@pytest.fixture(scope="module")
def chain_c(tmp_path_factory):
    return chain.chain_c(tmp_path_factory.mktemp("reduce_chain"))


@pytest.mark.parametrize("fam", [0, 1])
def test_c_and_fraction_forms_agree_bit_for_bit(chain_c, fam):
    if chain_c is None:
        pytest.skip("no gcc: the Fraction form is the only restatement")
    n, m, B = 3, 2, 7
    x, y, dv = random_case(np.random.default_rng(7), fam, n, m, B)
    inc = np.array([1, 1, 0, 1, 1, 1, 0], bool)
    for mask in (None, inc):
        a, b = chain_c(fam, n, m, x, y, dv, mask), chain.chain_fraction(fam, n, m, x, y, dv, mask)
        assert a.shape == (_abi.theta_shared_dim(fam, n, m),) and np.isfinite(a).all() and a.any()
        assert chain.bits_equal(a, b)
    # an excluded instance's values never reach the sum
    bad = dv.copy()
    bad[2], bad[6] = np.nan, np.inf
    assert chain.bits_equal(chain_c(fam, n, m, x, y, bad, inc), chain_c(fam, n, m, x, y, dv, inc))


def test_chunks_are_folded_in_ascending_order(chain_c):
    """Two full chunks and one of 3 instances — the result is ((0 + P₀) + P₁) + P₂ of the three
    chunks' own chains."""
    form = chain_c or chain.chain_fraction
    K = chain.CHUNK
    n, m, B = 2, 1, 2 * K + 3
    x, y, dv = random_case(np.random.default_rng(8), 0, n, m, B)
    parts = [form(0, n, m, x[a:b], y[a:b], dv[a:b]) for a, b in ((0, K), (K, 2 * K), (2 * K, B))]
    assert chain.bits_equal(form(0, n, m, x, y, dv), ((0.0 + parts[0]) + parts[1]) + parts[2])
    assert not chain.bits_equal(form(0, n, m, x, y, dv), form(0, n, m, x[::-1], y[::-1], dv[::-1]))  # order matters


def test_one_instance_is_the_full_records_entry(chain_c):
    """B = 1: ∂M_ij = −(λx_i·x_j) and ∂A_kj = fma(λx_j, y_k, −(λy_k·x_j)), the formulas of the full
    pullback record, as values; affine: the four blocks of [∂g; ∂h][x; y]ᵀ."""
    n, m = 3, 2
    rng = np.random.default_rng(9)
    x, y, dv = random_case(rng, 0, n, m, 1)
    ly, lx = dv[0, :m], dv[0, m:]
    M = np.array([[-(lx[i] * x[0, j]) for j in range(n)] for i in range(n)])
    A = np.array([[chain.fma(lx[j], y[0, k], -(ly[k] * x[0, j])) for j in range(n)] for k in range(m)])
    want = np.concatenate([M.T.reshape(-1), A.T.reshape(-1)])  # column-major
    forms = [chain.chain_fraction] + ([chain_c] if chain_c else [])
    for form in forms:
        assert np.array_equal(form(0, n, m, x, y, dv), want)
    g, h = dv[0, :n], dv[0, n:]
    z = np.concatenate([x[0], y[0]])
    full = np.outer(np.concatenate([g, h]), z)  # rows [∂g; ∂h], columns [x; y]
    want = np.concatenate([full[:n, :n].T.reshape(-1), full[:n, n:].T.reshape(-1), full[n:, :n].T.reshape(-1),
                           full[n:, n:].T.reshape(-1)])
    for form in forms:
        assert np.array_equal(form(1, n, m, x, y, dv), want)

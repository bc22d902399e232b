"""Shared-matrix batches on the GPU (mcpx_solve_batch_shared[_device]): every output field is
bit-identical to the full-θ call on the materialised θ′ = [shared ‖ var_b] — the in-kernel
shared read of the one-wave QP SCHUR kernels, the θ′ expansion in front of every other
kernel, the host pipeline, and the front end's split path.  Inputs: one random shared block
plus per-instance vectors; the reference θ′ is their host concatenation."""

from __future__ import annotations

import os
import subprocess
import sys

import numpy as np
import pytest

from mcp_amd import _abi
from mcp_amd.qp_benchmark import generate_random_parameter

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TRACE = 32
FIELDS = ("x", "y", "s", "kkt_error", "eps", "outer_iters", "status", "newton_iters", "active_mask", "alpha_trace",
          "fail_reason")


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and bool(np.all((a == b) | (np.isnan(a) & np.isnan(b))))


def assert_all_fields_equal(got: dict, ref: dict):
    for k in FIELDS:
        g, r = np.asarray(got[k]), np.asarray(ref[k])
        if k == "active_mask":  # torch holds the uint64 words as int64
            g, r = g.view(np.uint64), r.view(np.uint64)
        if g.dtype.kind == "f":
            assert _same(g, r), f"{k} differs in {int(np.sum(~((g == r) | (np.isnan(g) & np.isnan(r)))))} entries"
        else:
            assert g.shape == r.shape and np.array_equal(g, r), f"{k} differs"


def shared_qp(rng, n, m, B):
    """(shared [vec(M); vec(A)] of one random benchmark QP, var (B, m + n) = [b; ϕ])."""
    D = _abi.theta_shared_dim(0, n, m)
    return generate_random_parameter(rng, n, m, 0.0, batch=1)[0, :D].copy(), rng.standard_normal((B, m + n))


def shared_affine(rng, n, m, B, zero_s=False):
    """(shared [vec P; vec Q; vec R; vec S] of one monotone affine MCP, var (B, n + m) = [g; h])."""
    from tests.test_sensitivity import random_affine_theta

    D = _abi.theta_shared_dim(1, n, m)
    sh = random_affine_theta(rng, n, m, 1)[0, :D].copy()
    if zero_s:
        sh[D - m * m:] = 0.0
    return sh, rng.standard_normal((B, n + m))


def materialise(shared, var, dv):
    return np.ascontiguousarray(np.concatenate([np.broadcast_to(shared, (var.shape[0], shared.size)), var[:, :dv]], 1))


def _to_host(out: dict) -> dict:
    return {k: (None if v is None else v.cpu().numpy()) for k, v in out.items()}


def device_pair(fam, n, m, shared, var, warm=None, **kw):
    """(split call, full-θ call on the materialised θ′) through the device API, as host dicts."""
    import torch

    from mcp_amd.batch import solve_batch_device, solve_batch_shared_device

    dev = torch.device("cuda", 0)
    up = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    full = materialise(shared, var, n + m)
    w = {k: up(v) for k, v in (warm or {}).items()}
    got = solve_batch_shared_device(fam, n, m, up(shared), up(var), trace_len=TRACE, **w, **kw)
    ref = solve_batch_device(fam, n, m, up(full), trace_len=TRACE, **w, **kw)
    torch.cuda.synchronize()
    return _to_host(got), _to_host(ref), full


@pytest.fixture(scope="module")
def c3_case(gpu):
    """The (32, 16) SCHUR case, solved once: shared by the in-kernel and the oracle test."""
    shared, var = shared_qp(np.random.default_rng(3216), 32, 16, 257)
    return device_pair(0, 32, 16, shared, var, tol=1e-6, linear_solver="schur")


@pytest.fixture(scope="module")
def affine_case(gpu):
    """The (6, 4) affine SCHUR case with S = 0 (expansion path), solved once."""
    shared, var = shared_affine(np.random.default_rng(64), 6, 4, 67, zero_s=True)
    return device_pair(1, 6, 4, shared, var, tol=1e-6, linear_solver="schur")


# ---- in-kernel path: compile-time sizes --------------------------------------

@pytest.mark.parametrize("n,m,B", [(2, 2, 3), (16, 8, 130)])
def test_in_kernel_compile_time_sizes(gpu, n, m, B):
    shared, var = shared_qp(np.random.default_rng(100 * n + m), n, m, B)
    got, ref, _ = device_pair(0, n, m, shared, var, tol=1e-6, linear_solver="schur")
    assert_all_fields_equal(got, ref)
    assert (ref["status"] == 0).any()  # the case solves: the comparison is not of two failures


def test_in_kernel_c3(c3_case):
    got, ref, _ = c3_case
    assert_all_fields_equal(got, ref)
    assert (ref["status"] == 0).any()


# ---- in-kernel path: runtime-(n, m) kernels ----------------------------------

@pytest.mark.parametrize("n,m,B", [(8, 4, 65), (40, 16, 33)])
def test_in_kernel_generic_sizes(gpu, n, m, B):
    shared, var = shared_qp(np.random.default_rng(100 * n + m), n, m, B)
    got, ref, _ = device_pair(0, n, m, shared, var, tol=1e-6, linear_solver="schur")
    assert_all_fields_equal(got, ref)


def test_in_kernel_generic_c3_in_a_child_process(gpu):
    """(32, 16) through the runtime-(n, m) kernels: MCPX_GENERIC_KERNELS=1 in a fresh process."""
    env = dict(os.environ, MCPX_GENERIC_KERNELS="1")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "helpers", "shared_generic_probe.py")], env=env,
                       cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "shared-generic: OK" in r.stdout


# ---- expansion path ------------------------------------------------------------

@pytest.mark.parametrize("fam,n,m,ls,B", [
    (0, 16, 8, "reduced", 67), (0, 12, 6, "dense", 67), (1, 6, 4, "reduced", 67),
    (0, 70, 20, "schur", 8), (0, 40, 30, "reduced", 8),  # one workgroup per instance
])
def test_expansion_path(gpu, fam, n, m, ls, B):
    rng = np.random.default_rng(1000 * fam + 10 * n + m)
    shared, var = shared_qp(rng, n, m, B) if fam == 0 else shared_affine(rng, n, m, B)
    got, ref, _ = device_pair(fam, n, m, shared, var, tol=1e-6, linear_solver=ls)
    assert_all_fields_equal(got, ref)


def test_expansion_affine_schur(affine_case):
    got, ref, _ = affine_case
    assert_all_fields_equal(got, ref)
    assert (ref["fail_reason"] & _abi.FAIL_INPUT == 0).all() and (ref["status"] == 0).any()


def test_expansion_in_slices(gpu, monkeypatch):
    """A 1 MiB expansion block holds 321 instances of the (16, 8) θ′: 700 instances run in three
    slices through the one block."""
    monkeypatch.setenv("MCPX_EXPAND_MB", "1")
    shared, var = shared_qp(np.random.default_rng(7), 16, 8, 700)
    got, ref, _ = device_pair(0, 16, 8, shared, var, tol=1e-6, linear_solver="reduced")
    assert_all_fields_equal(got, ref)


# ---- edge cases ----------------------------------------------------------------

def test_var_stride_with_nan_padding(gpu):
    n, m, B = 16, 8, 130
    shared, var = shared_qp(np.random.default_rng(21), n, m, B)
    padded = np.full((B, n + m + 3), np.nan)
    padded[:, :n + m] = var
    got, ref, _ = device_pair(0, n, m, shared, padded, tol=1e-6, linear_solver="schur")
    assert_all_fields_equal(got, ref)
    assert not np.isnan(got["x"]).any()  # the padding was not read
    got, ref, _ = device_pair(0, n, m, shared, padded, tol=1e-6, linear_solver="reduced")  # expansion path
    assert_all_fields_equal(got, ref)
    assert not np.isnan(got["x"]).any()


def test_warm_starts(gpu):
    n, m, B = 16, 8, 130
    rng = np.random.default_rng(22)
    shared, var = shared_qp(rng, n, m, B)
    warm = dict(x0=rng.standard_normal((B, n)), y0=rng.uniform(0.5, 2.0, (B, m)), s0=rng.uniform(0.5, 2.0, (B, m)))
    got, ref, _ = device_pair(0, n, m, shared, var, warm=warm, tol=1e-6, linear_solver="schur")
    assert_all_fields_equal(got, ref)
    cold, _, _ = device_pair(0, n, m, shared, var, tol=1e-6, linear_solver="schur")
    assert not _same(cold["newton_iters"], got["newton_iters"])  # the warm starts were read


def test_asymmetric_shared_matrix_defers_every_instance(gpu):
    """M[1, 0] += 1e-3 in the shared block: the fast pass defers the whole batch to pass 2."""
    n, m, B = 16, 8, 130
    shared, var = shared_qp(np.random.default_rng(23), n, m, B)
    shared[1] += 1e-3
    got, ref, _ = device_pair(0, n, m, shared, var, tol=1e-6, linear_solver="schur")
    assert_all_fields_equal(got, ref)
    assert set(np.unique(got["status"])) <= {0, 1}  # no instance is left marked deferred


def test_affine_schur_with_a_nonzero_s_entry(gpu):
    n, m, B = 6, 4, 33
    shared, var = shared_affine(np.random.default_rng(24), n, m, B, zero_s=True)
    shared[_abi.theta_shared_dim(1, n, m) - 3] = 0.25
    got, ref, _ = device_pair(1, n, m, shared, var, tol=1e-6, linear_solver="schur")
    assert_all_fields_equal(got, ref)
    assert (got["fail_reason"] == _abi.FAIL_INPUT).all() and (got["status"] == 1).all()


# ---- host API ------------------------------------------------------------------

@pytest.mark.parametrize("shards", [None, 2])
def test_host_api_in_chunks(gpu, monkeypatch, shards):
    """B = 2,500 with MCPX_HOST_CHUNK = 1024: three chunks of the var block behind one upload of
    the shared block; with MCPX_HOST_SHARDS = 2 two such pipelines side by side."""
    from mcp_amd.batch import solve_batch, solve_batch_shared

    monkeypatch.setenv("MCPX_HOST_CHUNK", "1024")
    if shards:
        monkeypatch.setenv("MCPX_HOST_SHARDS", str(shards))
    n, m, B = 16, 8, 2500
    rng = np.random.default_rng(25)
    shared, var = shared_qp(rng, n, m, B)
    kw = dict(tol=1e-6, linear_solver="schur", trace_len=TRACE, x0=rng.standard_normal((B, n)))
    got = solve_batch_shared(0, n, m, shared, var, **kw)
    ref = solve_batch(0, n, m, materialise(shared, var, n + m), **kw)
    assert_all_fields_equal(got, ref)
    got = solve_batch_shared(0, n, m, shared, var, **dict(kw, linear_solver="reduced"))  # expansion per chunk
    ref = solve_batch(0, n, m, materialise(shared, var, n + m), **dict(kw, linear_solver="reduced"))
    assert_all_fields_equal(got, ref)


# ---- oracle ----------------------------------------------------------------------

def test_c3_equals_the_oracle(c3_case, oracle_lib):
    got, _, full = c3_case
    assert_all_fields_equal(got, oracle_lib.solve_batch(0, 32, 16, full, trace_len=TRACE, tol=1e-6,
                                                        linear_solver="schur"))


def test_affine_equals_the_oracle(affine_case, oracle_lib):
    got, _, full = affine_case
    assert_all_fields_equal(got, oracle_lib.solve_batch(1, 6, 4, full, trace_len=TRACE, tol=1e-6,
                                                        linear_solver="schur"))


# ---- front end -------------------------------------------------------------------

@pytest.mark.parametrize("which", ["readme", "vector"])
@pytest.mark.parametrize("kind", ["numpy", "torch"])
def test_front_end_takes_the_split_path(gpu, which, kind):
    """solve(InteriorPoint(), mcp, θ) of an MCP with constant matrices equals solve_batch on
    mcp.theta_map(θ), field for field, for host and for device θ."""
    import torch

    from mcp_amd.api import InteriorPoint, solve
    from mcp_amd.batch import solve_batch
    from tests.test_shared_theta import readme_qp, vector_qp

    mcp = readme_qp() if which == "readme" else vector_qp()
    assert mcp.shared_split() is not None
    n, m = mcp.unconstrained_dimension, mcp.constrained_dimension
    th = np.random.default_rng(26).standard_normal((64, mcp.parameter_dimension))
    ref = solve_batch(mcp.family, n, m, mcp.theta_map(th), linear_solver="schur", trace_len=TRACE)
    sol = solve(InteriorPoint(), mcp, th if kind == "numpy" else torch.from_numpy(th).to("cuda:0"), trace_len=TRACE)
    host = (lambda v: v) if kind == "numpy" else (lambda v: v.cpu().numpy())
    for k in FIELDS:
        if k == "fail_reason":  # not a field of MCPSolution
            continue
        g = np.asarray(host(getattr(sol, k)))
        if k == "status" and kind == "numpy":
            g = (g == "failed").astype(np.int32)
        if k == "active_mask":
            g = g.view(np.uint64)
        assert _same(g, ref[k]) if g.dtype.kind == "f" else np.array_equal(g, ref[k]), k

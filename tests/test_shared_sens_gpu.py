"""Sensitivities of shared-matrix batches on the GPU (mcpx_vjp_batch_shared*,
mcpx_jvp_batch_shared*, mcpx_solve_vjp_batch_shared_device): the gradient [∂b; ∂ϕ] / [∂g; ∂h]
and the tangents of the per-instance block are the bits of the full-θ calls on the materialised
θ′ = [shared ‖ var_b] (sliced / with a zero-padded θ̇) and of the oracle; the fused call is the
shared solve plus that pullback; the front end takes the split entries.

Inputs: one random shared block, random per-instance vectors, the oracle's iterate (tol 1e-6)
on θ′, random cotangents, K = 13 tangents (two chunks of MCPX_JVP_RHS)."""

from __future__ import annotations

import os
import subprocess
import sys

import numpy as np
import pytest

from mcp_amd import _abi
from mcp_amd.qp_benchmark import generate_random_parameter
from tests.test_shared_theta_gpu import (FIELDS, TRACE, _same, _to_host, assert_all_fields_equal, materialise,
                                         shared_affine, shared_qp)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = 13
_CASES: dict = {}


def make_case(oracle, fam, n, m, B, asym=False):
    """Inputs of one shape and the oracle's results on θ′ (computed once per shape, read-only):
    shared, var, full θ′, the iterate x / y / s, cotangents gx / gy / gs, tangents vdot (B, K, n + m)
    and its zero-padded full θ̇, the oracle's dθ′ / zdot and statuses."""
    key = (fam, n, m, B, asym)
    if key in _CASES:
        return _CASES[key]
    rng = np.random.default_rng(100 * n + m)
    shared, var = shared_qp(rng, n, m, B) if fam == 0 else shared_affine(rng, n, m, B)
    if asym:
        shared[1] += 0.125  # M[1, 0] != M[0, 1]
    D = shared.size
    full = materialise(shared, var, n + m)
    r = oracle.solve_batch(fam, n, m, full, tol=1e-6)
    c = dict(shared=shared, var=var, full=full, D=D, x=r["x"], y=r["y"], s=r["s"],
             gx=rng.standard_normal((B, n)), gy=rng.standard_normal((B, m)), gs=rng.standard_normal((B, m)),
             vdot=rng.standard_normal((B, K, n + m)))
    c["tdot"] = np.concatenate([np.zeros((B, K, D)), c["vdot"]], 2)
    c["o_dth"], c["o_vst"] = oracle.vjp_batch(fam, n, m, full, c["x"], c["y"], c["s"], c["gx"], c["gy"], c["gs"])
    c["o_zd"], c["o_jst"] = oracle.jvp_batch(fam, n, m, full, c["x"], c["y"], c["s"], c["tdot"])
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    _CASES[key] = c
    return c


def check_split_host(c, fam, n, m):
    """The split host calls against the full-θ GPU calls' slices and the oracle."""
    from mcp_amd.batch import jvp_batch, jvp_batch_shared, vjp_batch, vjp_batch_shared

    D = c["D"]
    dv, st = vjp_batch_shared(fam, n, m, c["shared"], c["x"], c["y"], c["s"], c["gx"], c["gy"], c["gs"])
    fdth, fst = vjp_batch(fam, n, m, c["full"], c["x"], c["y"], c["s"], c["gx"], c["gy"], c["gs"])
    assert dv.shape == (c["x"].shape[0], n + m)
    assert 2 * int((st == 0).sum()) >= st.size  # not a comparison between failures
    assert _same(dv, fdth[:, D:]) and _same(st, fst)
    assert _same(dv, c["o_dth"][:, D:]) and _same(st, c["o_vst"])
    zd, jst = jvp_batch_shared(fam, n, m, c["shared"], c["x"], c["y"], c["s"], c["vdot"])
    fzd, fjst = jvp_batch(fam, n, m, c["full"], c["x"], c["y"], c["s"], c["tdot"])
    assert zd.shape == (c["x"].shape[0], K, n + 2 * m)
    assert 2 * int((jst == 0).sum()) >= jst.size
    assert _same(zd, fzd) and _same(jst, fjst)
    assert _same(zd, c["o_zd"]) and _same(jst, c["o_jst"])


# ---- split VJP and JVP, host API -----------------------------------------------------

@pytest.mark.parametrize("fam,n,m,B", [
    (0, 2, 2, 3), (0, 16, 8, 130), (0, 32, 16, 65), (0, 8, 4, 65), (0, 5, 0, 17), (0, 1, 1, 5),
    (1, 6, 4, 67), (1, 20, 22, 33),  # affine; n + 2m = 64: the widest one-wave system
])
def test_split_equals_full_slice_and_oracle(gpu, oracle_lib, fam, n, m, B):
    check_split_host(make_case(oracle_lib, fam, n, m, B), fam, n, m)


@pytest.mark.parametrize("fam,n,m,B", [(0, 30, 20, 9), (1, 20, 24, 9)])  # n + 2m = 70, 68
def test_workgroup_kernels(gpu, oracle_lib, fam, n, m, B):
    check_split_host(make_case(oracle_lib, fam, n, m, B), fam, n, m)


def test_device_api_equals_host_api(gpu, oracle_lib):
    import torch

    from mcp_amd.batch import jvp_batch_shared, jvp_batch_shared_device, vjp_batch_shared, vjp_batch_shared_device

    n, m, B = 16, 8, 130
    c = make_case(oracle_lib, 0, n, m, B)
    dev = torch.device("cuda", 0)
    T = lambda a: torch.from_numpy(np.array(a)).to(dev)  # (a copy: the case's arrays are read-only)
    sh, x, y, s = T(c["shared"]), T(c["x"]), T(c["y"]), T(c["s"])
    hdv, hst = vjp_batch_shared(0, n, m, c["shared"], c["x"], c["y"], c["s"], c["gx"], c["gy"], c["gs"])
    hzd, hjst = jvp_batch_shared(0, n, m, c["shared"], c["x"], c["y"], c["s"], c["vdot"])
    # fresh allocations
    dv, st = vjp_batch_shared_device(0, n, m, sh, x, y, s, T(c["gx"]), T(c["gy"]), T(c["gs"]))
    zd, jst = jvp_batch_shared_device(0, n, m, sh, x, y, s, T(c["vdot"]))
    # caller-provided outputs (poisoned: every entry must be written)
    dv2 = torch.full((B, n + m), float("nan"), dtype=torch.float64, device=dev)
    zd2 = torch.full((B, K, n + 2 * m), float("nan"), dtype=torch.float64, device=dev)
    st2 = torch.full((B,), 7, dtype=torch.int32, device=dev)
    jst2 = torch.full((B,), 7, dtype=torch.int32, device=dev)
    r = vjp_batch_shared_device(0, n, m, sh, x, y, s, T(c["gx"]), T(c["gy"]), T(c["gs"]), dvar=dv2, status=st2)
    assert r[0] is dv2 and r[1] is st2
    jvp_batch_shared_device(0, n, m, sh, x, y, s, T(c["vdot"]), zdot=zd2, status=jst2)
    torch.cuda.synchronize()
    for a, b in ((dv, hdv), (dv2, hdv), (st, hst), (st2, hst), (zd, hzd), (zd2, hzd), (jst, hjst), (jst2, hjst)):
        assert _same(a.cpu().numpy(), b)


@pytest.mark.parametrize("null", ["gx", "gy", "gs"])
def test_null_cotangent_blocks(gpu, oracle_lib, null):
    from mcp_amd.batch import vjp_batch, vjp_batch_shared

    n, m = 16, 8
    c = make_case(oracle_lib, 0, n, m, 130)
    g = {k: (None if k == null else c[k]) for k in ("gx", "gy", "gs")}
    dv, st = vjp_batch_shared(0, n, m, c["shared"], c["x"], c["y"], c["s"], g["gx"], g["gy"], g["gs"])
    fdth, fst = vjp_batch(0, n, m, c["full"], c["x"], c["y"], c["s"], g["gx"], g["gy"], g["gs"])
    assert _same(dv, fdth[:, c["D"]:]) and _same(st, fst) and (st == 0).all()


def test_asymmetric_shared_m_takes_the_reduced_lu(gpu, oracle_lib):
    """shared[1] += 0.125: M is not symmetric, so the pullback's Schur path does not apply and
    every instance is solved by the LU of the reduced system."""
    n, m = 16, 8
    c = make_case(oracle_lib, 0, n, m, 33, asym=True)
    check_split_host(c, 0, n, m)
    sym = make_case(oracle_lib, 0, n, m, 130)
    assert c["shared"][1] != c["shared"][n] and sym["shared"][1] == sym["shared"][n]


def test_singular_jacobian(gpu):
    """The inputs of tests/test_sensitivity.py::test_gpu_singular_jacobian with instance 0's M, A
    shared: instance 0 (y₀ = s₀ = 0) is singular — status 1 and a NaN row, as in the full call."""
    from mcp_amd.batch import jvp_batch, jvp_batch_shared, vjp_batch, vjp_batch_shared

    n, m = 4, 2
    th = generate_random_parameter(np.random.default_rng(5), n, m, 0.0, batch=2)
    D = _abi.theta_shared_dim(0, n, m)
    shared, var = th[0, :D].copy(), th[:, D:].copy()
    full = materialise(shared, var, n + m)
    x, y, s = np.ones((2, 4)), np.array([[0.0, 1.0], [1.0, 2.0]]), np.array([[0.0, 1.0], [0.5, 0.25]])
    dv, st = vjp_batch_shared(0, n, m, shared, x, y, s, np.ones((2, 4)))
    assert st.tolist() == [1, 0] and np.isnan(dv[0]).all() and np.isfinite(dv[1]).all()
    fdth, fst = vjp_batch(0, n, m, full, x, y, s, np.ones((2, 4)))
    assert _same(dv, fdth[:, D:]) and _same(st, fst)
    vdot = np.ones((2, 3, n + m))
    zd, jst = jvp_batch_shared(0, n, m, shared, x, y, s, vdot)
    fzd, fjst = jvp_batch(0, n, m, full, x, y, s, np.concatenate([np.zeros((2, 3, D)), vdot], 2))
    assert jst.tolist() == [1, 0] and np.isnan(zd[0]).all()
    assert _same(zd, fzd) and _same(jst, fjst)


# ---- fused solve + pullback ------------------------------------------------------------

def cotangent(kind, rng, B, n, m, T):
    if kind == "loss":  # f = Σx² + Σy² (test/runtests.jl:72-75)
        return (2.0, 2.0, 0.0), (None, None, None)
    if kind == "affine":
        return (0.5, -1.5, 3.0), (T(rng.standard_normal((B, n))), T(rng.standard_normal((B, m))),
                                  T(rng.standard_normal((B, m))))
    return (0.0, 0.0, 0.0), (T(rng.standard_normal((B, n))), None, T(rng.standard_normal((B, m))))  # plain arrays


def check_fused(fam, n, m, B, ls, kind, asym=False):
    """solve_vjp_batch_shared_device: all output fields equal solve_batch_shared_device; dvar and
    vjp_status equal solve_vjp_batch_device on θ′, sliced."""
    import torch

    from mcp_amd.batch import (alloc_device_outputs, solve_batch_shared_device, solve_vjp_batch_device,
                               solve_vjp_batch_shared_device)

    rng = np.random.default_rng(100 * n + m)
    shared, var = shared_qp(rng, n, m, B) if fam == 0 else shared_affine(rng, n, m, B, zero_s=ls == "schur")
    if asym:
        shared[1] += 0.125
    D = shared.size
    dev = torch.device("cuda", 0)
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    ct, b = cotangent(kind, rng, B, n, m, T)
    kw = dict(tol=1e-6, linear_solver=ls)
    out = alloc_device_outputs(B, n, m, dev, TRACE)
    out, dv, st = solve_vjp_batch_shared_device(fam, n, m, T(shared), T(var), out, ct=ct, bx=b[0], by=b[1], bs=b[2],
                                                **kw)
    ref = solve_batch_shared_device(fam, n, m, T(shared), T(var), trace_len=TRACE, **kw)
    _, fdth, fst = solve_vjp_batch_device(fam, n, m, T(materialise(shared, var, n + m)), ct=ct, bx=b[0], by=b[1],
                                          bs=b[2], **kw)
    torch.cuda.synchronize()
    got, ref = _to_host(out), _to_host(ref)
    assert_all_fields_equal(got, ref)
    assert set(np.unique(got["status"])) <= {0, 1}  # no instance is left marked deferred
    st = st.cpu().numpy()
    assert 2 * int((st == 0).sum()) >= st.size
    assert _same(dv.cpu().numpy(), fdth.cpu().numpy()[:, D:]) and _same(st, fst.cpu().numpy())


@pytest.mark.parametrize("n,m,B", [(2, 2, 3), (16, 8, 130), (32, 16, 65)])
@pytest.mark.parametrize("kind", ["loss", "affine", "plain"])
def test_fused_in_kernel(gpu, n, m, B, kind):
    check_fused(0, n, m, B, "schur", kind)


@pytest.mark.parametrize("fam,n,m,B,ls", [(0, 16, 8, 130, "reduced"), (1, 6, 4, 67, "reduced")])
def test_fused_composed(gpu, fam, n, m, B, ls):
    check_fused(fam, n, m, B, ls, "affine")


def test_fused_asymmetric_m_goes_through_pass_two(gpu):
    check_fused(0, 16, 8, 33, "schur", "loss", asym=True)


def test_fused_warm_start_in_place_with_asymmetric_m(gpu):
    """x0 = out.x, y0 = out.y, s0 = out.s with an asymmetric shared M: the fast pass defers every
    instance and must have written nothing — pass 2 starts from the warm start, as the composed
    calls on separate warm-start buffers do (tests/test_fused_vjp.py, warm start in place)."""
    import torch

    from mcp_amd.batch import alloc_device_outputs, solve_batch_device, solve_vjp_batch_shared_device, vjp_batch_device

    n, m, B = 16, 8, 33
    rng = np.random.default_rng(100 * n + m)
    shared, var = shared_qp(rng, n, m, B)
    shared[1] += 0.125
    D = shared.size
    dev = torch.device("cuda", 0)
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    x0, y0, s0 = T(rng.standard_normal((B, n))), T(rng.uniform(0.5, 2.0, (B, m))), T(rng.uniform(0.5, 2.0, (B, m)))
    kw = dict(tol=1e-6, linear_solver="schur")
    th = T(materialise(shared, var, n + m))
    ref = solve_batch_device(0, n, m, th, alloc_device_outputs(B, n, m, dev), x0=x0, y0=y0, s0=s0, **kw)
    cold = solve_batch_device(0, n, m, th, alloc_device_outputs(B, n, m, dev), **kw)
    rdth, rst = vjp_batch_device(0, n, m, th, ref["x"], ref["y"], ref["s"], 2.0 * ref["x"], 2.0 * ref["y"])
    out = alloc_device_outputs(B, n, m, dev)
    out["x"].copy_(x0)
    out["y"].copy_(y0)
    out["s"].copy_(s0)
    dvar = torch.full((B, n + m), float("nan"), dtype=torch.float64, device=dev)
    out, dv, st = solve_vjp_batch_shared_device(0, n, m, T(shared), T(var), out, ct=(2.0, 2.0, 0.0), dvar=dvar,
                                                x0=out["x"], y0=out["y"], s0=out["s"], **kw)
    torch.cuda.synchronize()
    # the warm start was read (it changes the iteration counts) and every solve moved x
    assert not _same(cold["newton_iters"].cpu().numpy(), ref["newton_iters"].cpu().numpy())
    assert not np.array_equal(ref["x"].cpu().numpy(), x0.cpu().numpy())
    for f in ("x", "y", "s", "kkt_error", "eps", "outer_iters", "status", "newton_iters"):
        assert _same(out[f].cpu().numpy(), ref[f].cpu().numpy()), f
    assert _same(dv.cpu().numpy(), rdth.cpu().numpy()[:, D:]) and _same(st.cpu().numpy(), rst.cpu().numpy())
    assert (st.cpu().numpy() == 0).all()


# ---- host sharding -----------------------------------------------------------------------

def test_host_shards_in_a_child_process(gpu):
    """MCPX_HOST_SHARDS=3 over B = 67 (shards of 23, 22, 22) equals one shard, bit for bit."""
    env = dict(os.environ, MCPX_HOST_SHARDS="3")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "helpers", "shared_sens_shards_probe.py")],
                       env=env, cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "shared-sens-shards: OK" in r.stdout


# ---- front end -----------------------------------------------------------------------------

class Spy:
    """Counts the calls of a function of mcp_amd.batch and passes them on."""

    def __init__(self, monkeypatch, name):
        from mcp_amd import batch

        self.calls, self.fn = 0, getattr(batch, name)
        monkeypatch.setattr(batch, name, self)

    def __call__(self, *a, **kw):
        self.calls += 1
        return self.fn(*a, **kw)


def _mcp(which):
    from tests.test_shared_theta import readme_qp, vector_qp

    mcp = readme_qp() if which == "readme" else vector_qp()
    mcp.compute_sensitivities = True
    return mcp


@pytest.mark.parametrize("which", ["readme", "vector"])
@pytest.mark.parametrize("kind", ["numpy", "torch"])
def test_front_end_pullback_takes_the_split_entry(gpu, monkeypatch, which, kind):
    """solve_pullback equals the result computed explicitly through the full map: vjp_batch on
    mcp.theta_map(θ), then theta_map.vjp."""
    import torch

    from mcp_amd.api import InteriorPoint, solve
    from mcp_amd.autodiff import solve_pullback
    from mcp_amd.batch import vjp_batch, vjp_batch_device

    mcp = _mcp(which)
    n, m, p = mcp.unconstrained_dimension, mcp.constrained_dimension, mcp.parameter_dimension
    rng = np.random.default_rng(31)
    B = 64
    th = rng.standard_normal((B, p))
    dx, dy, ds = rng.standard_normal((B, n)), rng.standard_normal((B, m)), rng.standard_normal((B, m))
    spy = Spy(monkeypatch, "vjp_batch_shared" if kind == "numpy" else "vjp_batch_shared_device")
    if kind == "numpy":
        sol = solve(InteriorPoint(), mcp, th)
        dθ, st = solve_pullback(sol, dx, dy, ds, return_status=True)
        dtp, rst = vjp_batch(mcp.family, n, m, mcp.theta_map(th), sol.x, sol.y, sol.s, dx, dy, ds)
        ref = mcp.theta_map.vjp(th, dtp)
    else:
        T = lambda a: torch.from_numpy(a).to("cuda:0")
        tht = T(th)
        sol = solve(InteriorPoint(), mcp, tht)
        dθ, st = solve_pullback(sol, T(dx), T(dy), T(ds), return_status=True)
        dtp, rst = vjp_batch_device(mcp.family, n, m, mcp.theta_map(tht).contiguous(), sol.x, sol.y, sol.s, T(dx),
                                    T(dy), T(ds))
        ref = mcp.theta_map.vjp(tht, dtp)
        dθ, st, ref, rst = (t.cpu().numpy() for t in (dθ, st, ref, rst))
    assert spy.calls == 1
    assert dθ.shape == (B, p) and (st == 0).all()
    assert _same(dθ, ref) and _same(st, rst)


@pytest.mark.parametrize("which", ["readme", "vector"])
def test_front_end_dual_takes_the_split_entry(gpu, monkeypatch, which):
    """solve_dual (host θ: it has no device form) equals jvp_batch on mcp.theta_map(θ) with the
    full map's tangents, in the partial layout."""
    from mcp_amd.api import InteriorPoint, solve
    from mcp_amd.autodiff import solve_dual
    from mcp_amd.batch import jvp_batch

    mcp = _mcp(which)
    n, m, p = mcp.unconstrained_dimension, mcp.constrained_dimension, mcp.parameter_dimension
    rng = np.random.default_rng(32)
    B, Kp = 64, 3
    th, tpar = rng.standard_normal((B, p)), rng.standard_normal((B, p, Kp))
    spy = Spy(monkeypatch, "jvp_batch_shared")
    d = solve_dual(InteriorPoint(), mcp, th, tpar)
    assert spy.calls == 1
    sol = solve(InteriorPoint(), mcp, th)
    tdot = mcp.theta_map.jvp(th, np.ascontiguousarray(np.swapaxes(tpar, 1, 2)))
    zd, st = jvp_batch(mcp.family, n, m, mcp.theta_map(th), sol.x, sol.y, sol.s, tdot)
    zp = np.swapaxes(zd, 1, 2)
    assert (st == 0).all() and _same(d.sensitivity_status, st)
    assert _same(d.x_partials, zp[:, :n]) and _same(d.y_partials, zp[:, n:n + m]) and _same(d.s_partials, zp[:, n + m:])


def test_solve_torch_backward_gives_that_gradient(gpu, monkeypatch):
    import torch

    from mcp_amd.autodiff import solve_torch
    from mcp_amd.batch import vjp_batch_device

    mcp = _mcp("vector")
    n, m, p = mcp.unconstrained_dimension, mcp.constrained_dimension, mcp.parameter_dimension
    th = torch.from_numpy(np.random.default_rng(33).standard_normal((64, p))).to("cuda:0").requires_grad_(True)
    spy = Spy(monkeypatch, "vjp_batch_shared_device")
    x, y, s, _ = solve_torch(mcp, th)
    ((x ** 2).sum() + (y ** 2).sum()).backward()
    assert spy.calls == 1
    thd = th.detach()
    dtp, st = vjp_batch_device(mcp.family, n, m, mcp.theta_map(thd).contiguous(), x.detach(), y.detach(), s.detach(),
                               2.0 * x.detach(), 2.0 * y.detach(), torch.zeros_like(s))
    ref = mcp.theta_map.vjp(thd, dtp)
    assert (st.cpu().numpy() == 0).all()
    assert _same(th.grad.cpu().numpy(), ref.cpu().numpy())


def test_theta_dependent_matrix_still_takes_the_full_path(gpu, monkeypatch):
    from mcp_amd.api import InteriorPoint, solve
    from mcp_amd.autodiff import solve_pullback
    from tests.test_shared_theta import matrix_mcp

    mcp = matrix_mcp()
    mcp.compute_sensitivities = True
    assert mcp.shared_split() is None
    split, full = Spy(monkeypatch, "vjp_batch_shared"), Spy(monkeypatch, "vjp_batch")
    th = np.random.default_rng(34).uniform(0.1, 1.0, (8, 2))
    sol = solve(InteriorPoint(), mcp, th)
    dθ = solve_pullback(sol, np.ones((8, 2)))
    assert split.calls == 0 and full.calls == 1
    assert dθ.shape == (8, 2) and np.isfinite(dθ).all()

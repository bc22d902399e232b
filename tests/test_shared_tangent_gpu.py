"""Tangents along the shared block and the condition estimate of shared-matrix batches on the GPU
(mcpx_jvp_batch_shared_dot*, mcpx_cond_batch_shared*): zdot / rcond and status are the bits of the
existing full-θ calls on θ′ = [shared ‖ var_b] and θ̇_{b,c} = [shared_dot_c ‖ var_dot_{b,c}]
materialised here — for every instance, NaN rows of a singular ∇F_z and non-finite iterates
included.

Inputs: one random shared block, random per-instance vectors, the iterate of solve_batch_shared
at tol 1e-6, seeded normal shared_dot (K, shared_dim) and var_dot (B, K, n + m)."""

from __future__ import annotations

import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from mcp_amd import _abi
from mcp_amd.qp_benchmark import generate_random_parameter
from tests.test_shared_theta_gpu import _same, materialise, shared_affine, shared_qp

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_CASES: dict = {}


def make_case(fam, n, m, B, K):
    """Inputs of one shape (computed once per shape, read-only): shared, var, the full θ′, the
    iterate x / y / s of the shared solve, sdot (K, D), vdot (B, K, n + m) and the full θ̇."""
    key = (fam, n, m, B, K)
    if key in _CASES:
        return _CASES[key]
    from mcp_amd.batch import solve_batch_shared

    rng = np.random.default_rng(1000 * n + 10 * m + K)
    shared, var = shared_qp(rng, n, m, B) if fam == 0 else shared_affine(rng, n, m, B)
    r = solve_batch_shared(fam, n, m, shared, var, tol=1e-6)
    assert 2 * int((r["status"] == 0).sum()) >= B  # the case solves
    c = dict(shared=shared, var=var, full=materialise(shared, var, n + m), D=shared.size, x=r["x"], y=r["y"], s=r["s"],
             sdot=rng.standard_normal((K, shared.size)), vdot=rng.standard_normal((B, K, n + m)))
    c["tdot"] = full_tdot(c["sdot"], c["vdot"], B)
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    _CASES[key] = c
    return c


def full_tdot(sdot, vdot, B):
    """θ̇ (B, K, p) of the full call: every instance's partial c is [sdot_c ‖ vdot_{b,c}]."""
    K, D = sdot.shape
    v = np.zeros((B, K, 0)) if vdot is None else vdot
    return np.ascontiguousarray(np.concatenate([np.broadcast_to(sdot, (B, K, D)), v], 2))


def T(a):
    import torch

    return None if a is None else torch.from_numpy(np.array(a)).to("cuda:0")  # (a copy: cases are read-only)


def dot_device(fam, n, m, c, x=None, y=None, s=None, sdot=None, vdot="case"):
    """jvp_batch_shared_device with shared_dot → host (zdot, status)."""
    import torch

    from mcp_amd.batch import jvp_batch_shared_device

    pick = lambda a, k: c[k] if a is None else a
    vd = c["vdot"] if isinstance(vdot, str) else vdot
    zd, st = jvp_batch_shared_device(fam, n, m, T(c["shared"]), T(pick(x, "x")), T(pick(y, "y")), T(pick(s, "s")), T(vd),
                                     shared_dot=T(pick(sdot, "sdot")))
    torch.cuda.synchronize()
    return zd.cpu().numpy(), st.cpu().numpy()


def full_device(fam, n, m, c, tdot, x=None, y=None, s=None):
    """The reference: jvp_batch_device on the materialised θ′ and θ̇ → host (zdot, status)."""
    import torch

    from mcp_amd.batch import jvp_batch_device

    pick = lambda a, k: c[k] if a is None else a
    zd, st = jvp_batch_device(fam, n, m, T(c["full"]), T(pick(x, "x")), T(pick(y, "y")), T(pick(s, "s")), T(tdot))
    torch.cuda.synchronize()
    return zd.cpu().numpy(), st.cpu().numpy()


def check_equals_full(fam, n, m, B, K):
    c = make_case(fam, n, m, B, K)
    zd, st = dot_device(fam, n, m, c)
    fzd, fst = full_device(fam, n, m, c, c["tdot"])
    assert zd.shape == (B, K, n + 2 * m)
    assert 2 * int((fst == 0).sum()) >= B  # not a comparison between failures
    assert np.array_equal(zd, fzd, equal_nan=True) and np.array_equal(st, fst)
    return c, zd, st


# ---- the bits of the full call ---------------------------------------------------------

@pytest.mark.parametrize("fam,n,m,K,B", [
    (0, 2, 2, 1, 3), (0, 16, 8, 3, 67),
    (0, 32, 16, 9, 65),  # two rounds of MCPX_JVP_RHS, the second with one live column
    (0, 20, 12, 8, 33),  # no compiled (n, m): the runtime bucket
    (0, 5, 0, 2, 5), (1, 8, 4, 3, 67),
])
def test_one_wave_equals_the_full_call(gpu, oracle_lib, fam, n, m, K, B):
    c, zd, st = check_equals_full(fam, n, m, B, K)
    if (n, m) == (16, 8):  # and the oracle, on the first 8 instances
        ozd, ost = oracle_lib.jvp_batch(fam, n, m, c["full"][:8], c["x"][:8], c["y"][:8], c["s"][:8], c["tdot"][:8])
        assert np.array_equal(zd[:8], ozd, equal_nan=True) and np.array_equal(st[:8], ost)


@pytest.mark.parametrize("fam,n,m,K,B", [(0, 30, 20, 3, 9), (1, 20, 24, 9, 9)])  # n + 2m = 70, 68
def test_workgroup_equals_the_full_call(gpu, fam, n, m, K, B):
    check_equals_full(fam, n, m, B, K)


@pytest.mark.parametrize("fam,n,m,K,B", [(0, 16, 8, 3, 67), (1, 8, 4, 3, 67), (0, 30, 20, 3, 9), (1, 20, 24, 9, 9)])
def test_null_var_dot_is_a_zero_var_dot(gpu, fam, n, m, K, B):
    c = make_case(fam, n, m, B, K)
    zeros = np.zeros((B, K, n + m))
    zd, st = dot_device(fam, n, m, c, vdot=None)
    zd0, st0 = dot_device(fam, n, m, c, vdot=zeros)
    fzd, fst = full_device(fam, n, m, c, full_tdot(c["sdot"], zeros, B))
    assert np.array_equal(zd, zd0, equal_nan=True) and np.array_equal(st, st0)
    assert np.array_equal(zd, fzd, equal_nan=True) and np.array_equal(st, fst)
    assert np.isfinite(zd[st == 0]).all() and zd[st == 0].any()


@pytest.mark.parametrize("fam,n,m,K,B", [(0, 16, 8, 3, 67), (1, 8, 4, 3, 67), (0, 30, 20, 3, 9)])
def test_zero_shared_dot_is_the_split_call(gpu, fam, n, m, K, B):
    """shared_dot = 0 with a var_dot: the existing split call's bits on finite iterates."""
    import torch

    from mcp_amd.batch import jvp_batch_shared_device

    c = make_case(fam, n, m, B, K)
    assert np.isfinite(c["x"]).all() and np.isfinite(c["y"]).all() and np.isfinite(c["s"]).all()
    zd, st = dot_device(fam, n, m, c, sdot=np.zeros((K, c["D"])))
    szd, sst = jvp_batch_shared_device(fam, n, m, T(c["shared"]), T(c["x"]), T(c["y"]), T(c["s"]), T(c["vdot"]))
    torch.cuda.synchronize()
    assert np.array_equal(zd, szd.cpu().numpy(), equal_nan=True) and np.array_equal(st, sst.cpu().numpy())


@pytest.mark.parametrize("fam,n,m,K,B", [(0, 16, 8, 3, 67), (1, 8, 4, 3, 67), (0, 30, 20, 3, 9)])
def test_non_finite_iterate(gpu, fam, n, m, K, B):
    """x of instance 1 holds a NaN, y of instance 2 an Inf (overwritten after the solve): the
    matrix-tangent chains run, so these rows equal the full call's too."""
    c = make_case(fam, n, m, B, K)
    x, y = c["x"].copy(), c["y"].copy()
    x[1, 0] = np.nan
    y[2, m - 1] = np.inf
    zd, st = dot_device(fam, n, m, c, x=x, y=y)
    fzd, fst = full_device(fam, n, m, c, c["tdot"], x=x, y=y)
    assert np.array_equal(zd, fzd, equal_nan=True) and np.array_equal(st, fst)
    assert not np.isfinite(zd[1]).all() and not np.isfinite(zd[2]).all() and np.isfinite(zd[0]).all()


def test_singular_jacobian(gpu):
    """The inputs of tests/test_shared_sens_gpu.py::test_singular_jacobian: instance 0 (y₀ = s₀ = 0)
    is singular — status 1 and NaN rows, as in the full call."""
    from mcp_amd.batch import cond_batch, cond_batch_shared, jvp_batch, jvp_batch_shared

    n, m, K = 4, 2, 3
    rng = np.random.default_rng(5)
    th = generate_random_parameter(rng, n, m, 0.0, batch=2)
    D = _abi.theta_shared_dim(0, n, m)
    shared, var = th[0, :D].copy(), th[:, D:].copy()
    full = materialise(shared, var, n + m)
    x, y, s = np.ones((2, 4)), np.array([[0.0, 1.0], [1.0, 2.0]]), np.array([[0.0, 1.0], [0.5, 0.25]])
    sdot, vdot = rng.standard_normal((K, D)), rng.standard_normal((2, K, n + m))
    zd, st = jvp_batch_shared(0, n, m, shared, x, y, s, vdot, shared_dot=sdot)
    fzd, fst = jvp_batch(0, n, m, full, x, y, s, full_tdot(sdot, vdot, 2))
    assert st.tolist() == [1, 0] and np.isnan(zd[0]).all() and np.isfinite(zd[1]).all()
    assert np.array_equal(zd, fzd, equal_nan=True) and np.array_equal(st, fst)
    rc, cst = cond_batch_shared(0, n, m, shared, x, y, s)
    frc, fcst = cond_batch(0, n, m, full, x, y, s)
    assert cst.tolist() == [1, 0] and rc[0] == 0.0 and rc[1] > 0.0
    assert np.array_equal(rc, frc) and np.array_equal(cst, fcst)


# ---- host API ----------------------------------------------------------------------------

def test_device_api_equals_host_api(gpu):
    import torch

    from mcp_amd.batch import jvp_batch_shared, jvp_batch_shared_device

    fam, n, m, K, B = 0, 16, 8, 3, 67
    c = make_case(fam, n, m, B, K)
    zd, st = dot_device(fam, n, m, c)
    hzd, hst = jvp_batch_shared(fam, n, m, c["shared"], c["x"], c["y"], c["s"], c["vdot"], shared_dot=c["sdot"])
    hzd0, hst0 = jvp_batch_shared(fam, n, m, c["shared"], c["x"], c["y"], c["s"], None, shared_dot=c["sdot"])
    zd0, st0 = dot_device(fam, n, m, c, vdot=None)
    # caller-provided outputs (poisoned: every entry must be written)
    zd2 = torch.full((B, K, n + 2 * m), float("nan"), dtype=torch.float64, device="cuda:0")
    st2 = torch.full((B,), 7, dtype=torch.int32, device="cuda:0")
    r = jvp_batch_shared_device(fam, n, m, T(c["shared"]), T(c["x"]), T(c["y"]), T(c["s"]), T(c["vdot"]), zdot=zd2,
                                status=st2, shared_dot=T(c["sdot"]))
    torch.cuda.synchronize()
    assert r[0] is zd2 and r[1] is st2
    assert (hst == 0).all()
    for a, b in ((hzd, zd), (hst, st), (zd2.cpu().numpy(), zd), (st2.cpu().numpy(), st), (hzd0, zd0), (hst0, st0)):
        assert np.array_equal(a, b, equal_nan=True)


def test_host_shards_in_a_child_process(gpu):
    """MCPX_HOST_SHARDS=3 with MCPX_HOST_CHUNK=1024 over B = 67 (shards of 23, 22, 22): the bits
    of one shard."""
    env = dict(os.environ, MCPX_HOST_SHARDS="3", MCPX_HOST_CHUNK="1024")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "helpers", "shared_tangent_shards_probe.py")],
                       env=env, cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "shared-tangent-shards: OK" in r.stdout


# ---- condition estimate --------------------------------------------------------------------

@pytest.mark.parametrize("fam,n,m,B", [(0, 16, 8, 33), (1, 8, 4, 17), (0, 30, 20, 9)])
def test_cond_equals_the_full_call(gpu, fam, n, m, B):
    import torch

    from mcp_amd._lib import check, lib
    from mcp_amd.batch import cond_batch, cond_batch_shared, cond_batch_shared_device

    c = make_case(fam, n, m, B, 3)
    y, s = c["y"].copy(), c["s"].copy()
    y[0], s[0] = 0.0, 0.0  # instance 0: zero complementarity rows, ∇F_z exactly singular
    rc, st = cond_batch_shared(fam, n, m, c["shared"], c["x"], y, s)
    frc, fst = cond_batch(fam, n, m, c["full"], c["x"], y, s)
    assert rc.shape == (B,) and st[0] == 1 and rc[0] == 0.0 and (st[1:] == 0).all() and (rc[1:] > 0.0).all()
    assert np.array_equal(rc, frc) and np.array_equal(st, fst)
    drc, dst = cond_batch_shared_device(fam, n, m, T(c["shared"]), T(c["x"]), T(y), T(s))
    # the full-θ device entry, which has no wrapper of its own
    full, x, yt, s_t = T(c["full"]), T(c["x"]), T(y), T(s)
    frc_d = torch.full((B,), float("nan"), dtype=torch.float64, device="cuda:0")
    fst_d = torch.full((B,), 7, dtype=torch.int32, device="cuda:0")
    desc = _abi.Desc(fam, n, m, 0, B, full.shape[1])
    check(lib().mcpx_cond_batch_device(C.byref(desc), full.data_ptr(), x.data_ptr(), yt.data_ptr(), s_t.data_ptr(),
                                       frc_d.data_ptr(), fst_d.data_ptr(),
                                       C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    assert np.array_equal(drc.cpu().numpy(), rc) and np.array_equal(dst.cpu().numpy(), st)
    assert np.array_equal(frc_d.cpu().numpy(), rc) and np.array_equal(fst_d.cpu().numpy(), st)


# ---- solve_shared_dual -----------------------------------------------------------------------

DUAL = dict(fam=0, n=16, m=8, B=16, K=2, seed=1608)
# forward/reverse consistency: bound on the relative gap, 10 × the larger gap of the first GPU run
# (2.915e-10; see test_forward_and_reverse_mode_agree)
DUAL_GAP_BOUND = 2.915e-9
DUAL_RCOND_MIN = 1e-8


def dual_inputs():
    rng = np.random.default_rng(DUAL["seed"])
    n, m, B, K = DUAL["n"], DUAL["m"], DUAL["B"], DUAL["K"]
    shared, var = shared_qp(rng, n, m, B)
    return dict(shared=shared, var=var, sp=rng.standard_normal((shared.size, K)),
                vp=rng.standard_normal((B, n + m, K)), gx=rng.standard_normal((B, n)),
                gy=rng.standard_normal((B, m)), gs=rng.standard_normal((B, m)))


def test_solve_shared_dual_partials(gpu):
    """The partials are solve_dual-style slices of the full call's zdot at the same iterate."""
    from mcp_amd.autodiff import solve_shared_dual
    from mcp_amd.batch import jvp_batch, solve_batch_shared

    fam, n, m, B, K = (DUAL[k] for k in ("fam", "n", "m", "B", "K"))
    d = dual_inputs()
    sol = solve_shared_dual(fam, n, m, d["shared"], d["var"], d["sp"], d["vp"], tol=1e-6)
    r = solve_batch_shared(fam, n, m, d["shared"], d["var"], tol=1e-6)
    assert (r["status"] == 0).all()
    for k in ("x", "y", "status", "kkt_error"):
        assert _same(getattr(sol, k), r[k])
    assert _same(sol.s, r["y"]) and _same(sol.s_value_true, r["s"])  # solve_dual's `s` quirk
    tdot = full_tdot(np.ascontiguousarray(d["sp"].T), np.ascontiguousarray(np.swapaxes(d["vp"], 1, 2)), B)
    zd, st = jvp_batch(fam, n, m, materialise(d["shared"], d["var"], n + m), r["x"], r["y"], r["s"], tdot)
    zp = np.swapaxes(zd, 1, 2)
    assert sol.x_partials.shape == (B, n, K) and (st == 0).all() and _same(sol.sensitivity_status, st)
    assert _same(sol.x_partials, zp[:, :n]) and _same(sol.y_partials, zp[:, n:n + m])
    assert _same(sol.s_partials, zp[:, n + m:])
    # one block alone: the other is zero
    only_s = solve_shared_dual(fam, n, m, d["shared"], d["var"], shared_partials=d["sp"], tol=1e-6)
    zd0, _ = jvp_batch(fam, n, m, materialise(d["shared"], d["var"], n + m), r["x"], r["y"], r["s"],
                       full_tdot(np.ascontiguousarray(d["sp"].T), np.zeros((B, K, n + m)), B))
    assert _same(only_s.x_partials, np.swapaxes(zd0, 1, 2)[:, :n])


def test_forward_and_reverse_mode_agree(gpu):
    """Σ_b ⟨g_b, ż_b⟩ of the tangent call along (Ṡ, V̇) against ⟨dshared, Ṡ⟩ + Σ_b ⟨dvar_b, V̇_b⟩ of
    vjp_batch_shared_reduce with the same cotangents g, over the instances with rcond ≥ 1e-8
    (cond_batch_shared; at least 90 % of the batch).  The gap is rounding amplified by cond(∇F_z).
    First GPU run (MI355X): 16 of 16 instances kept (smallest rcond 6.7e-5), relative gaps
    |fwd − rev| / max(|fwd|, |rev|) = 2.915e-10 and 1.612e-10 for the K = 2 directions; the bound is
    10 × the larger one, DUAL_GAP_BOUND = 2.915e-9."""
    from mcp_amd.autodiff import solve_shared_dual
    from mcp_amd.batch import cond_batch_shared, vjp_batch_shared_reduce

    fam, n, m, B, K = (DUAL[k] for k in ("fam", "n", "m", "B", "K"))
    d = dual_inputs()
    sol = solve_shared_dual(fam, n, m, d["shared"], d["var"], d["sp"], d["vp"], tol=1e-6)
    x, y, s = sol.x, sol.y, sol.s_value_true
    rc, cst = cond_batch_shared(fam, n, m, d["shared"], x, y, s)
    keep = (rc >= DUAL_RCOND_MIN) & (cst == 0) & (sol.sensitivity_status == 0)
    assert keep.sum() >= 0.9 * B
    dshared, used, dvar, vst = vjp_batch_shared_reduce(fam, n, m, d["shared"], x, y, s, d["gx"], d["gy"], d["gs"],
                                                       skip=~keep)
    assert used == int(keep.sum()) and (vst[keep] == 0).all()
    g = np.concatenate([d["gx"], d["gy"], d["gs"]], 1)  # (B, n + 2m), z = [x; y; s]
    zp = np.concatenate([sol.x_partials, sol.y_partials, sol.s_partials], 1)  # (B, n + 2m, K)
    for c in range(K):
        fwd = float(np.sum(g[keep] * zp[keep, :, c]))
        rev = float(dshared @ d["sp"][:, c] + np.sum(dvar[keep] * d["vp"][keep, :, c]))
        gap = abs(fwd - rev) / max(abs(fwd), abs(rev))
        print(f"forward/reverse direction {c}: fwd {fwd!r} rev {rev!r} relative gap {gap:.3e} "
              f"(kept {int(keep.sum())}/{B}, min rcond {rc[keep].min():.3e})")
        assert gap <= DUAL_GAP_BOUND

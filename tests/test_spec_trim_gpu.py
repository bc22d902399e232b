"""The compile-time-(n, m) SCHUR kernels after the round-7 VALU trim (formation preload by
base + immediate, `tol` under a constant EXEC mask, the residual stream's pointer and stride
formed once per instance) against the C
oracle, every output field bit for bit, at (32, 16), (16, 8) and (2, 2), 128 instances each,
through the four entry points that instantiate them: the QP family, the affine embedding of
the same QPs, the shared-matrix call and the fused solve + pullback.

One batch per size holds, in this order (KINDS):
  plain   random dense QPs of the benchmark's generator (the fast pass; the oracle alone solves
          ≥ 90 % of them, checked below on the CPU, so the comparison is of full solves);
  negz    the same kind with −0.0 entries in M, off the diagonal (a symmetric pair) and on it;
  nan     one instance with a NaN in M;
  asym    one off-diagonal entry of M perturbed: not symmetric, solved by pass 2;
  shift   M − 3·I: a non-positive pivot in mid-solve, deferred to pass 2.
It is solved at tol = 1e-6 and again at tol = 1e-2, where the diagonal add moves the iterates
visibly.  tests/helpers/spec_trim_probe.py runs the same comparisons in a child process with
MCPX_GENERIC_KERNELS=1 (the runtime-(n, m) kernels, which keep the clamped code path).
"""

from __future__ import annotations

import os
import subprocess
import sys

import numpy as np
import pytest

from mcp_amd import _abi
from mcp_amd.qp_benchmark import affine_embedding, generate_random_parameter

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TRACE = 32
SIZES = [(32, 16), (16, 8), (2, 2)]
TOLS = [1e-6, 1e-2]
KINDS = (("plain", 80), ("negz", 16), ("nan", 1), ("asym", 15), ("shift", 16))  # 128 instances
FIELDS = ("x", "y", "s", "kkt_error", "eps", "outer_iters", "status", "newton_iters", "active_mask", "alpha_trace",
          "fail_reason")


def kind_slices():
    out, at = {}, 0
    for k, c in KINDS:
        out[k] = slice(at, at + c)
        at += c
    return out


def make_batch(n: int, m: int) -> np.ndarray:
    """(128, p) θ = [vec M; vec A; b; ϕ] of KINDS, seeded by the size."""
    rng = np.random.default_rng(7000 + 100 * n + m)
    B = sum(c for _, c in KINDS)
    th = generate_random_parameter(rng, n, m, 0.0, batch=B)
    sl = kind_slices()
    M = th[:, :n * n].reshape(B, n, n)  # [b, j, i] = M_ij (column-major); a view of th
    for b in range(sl["negz"].start, sl["negz"].stop):
        i, j = (0, 1) if n == 2 else rng.choice(n, 2, replace=False)
        M[b, i, j] = M[b, j, i] = -0.0  # a symmetric pair: the fast pass takes the instance
        d = int(rng.integers(n))
        M[b, d, d] = -0.0
    b = sl["nan"].start
    M[b, n - 1, 0] = M[b, 0, n - 1] = np.nan
    for b in range(sl["asym"].start, sl["asym"].stop):
        i, j = (0, 1) if n == 2 else rng.choice(n, 2, replace=False)
        M[b, j, i] += 1e-3  # M_ij alone
    for b in range(sl["shift"].start, sl["shift"].stop):
        M[b] -= 3.0 * np.eye(n)
    return np.ascontiguousarray(th)


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and bool(np.all((a == b) | (np.isnan(a) & np.isnan(b))))


def assert_fields_equal(got: dict, ref: dict, fields=FIELDS, what=""):
    for k in fields:
        if got.get(k) is None:
            continue
        g, r = np.asarray(got[k]), np.asarray(ref[k])
        if k == "active_mask":  # torch holds the uint64 words as int64
            g, r = g.view(np.uint64), r.view(np.uint64)
        if g.dtype.kind == "f":
            assert _same(g, r), f"{what}{k} differs in {int(np.sum(~((g == r) | (np.isnan(g) & np.isnan(r)))))} entries"
        else:
            assert g.shape == r.shape and np.array_equal(g, r), f"{what}{k} differs"


def _host(out: dict) -> dict:
    return {k: (None if v is None else v.cpu().numpy()) for k, v in out.items()}


# ---- the oracle's answers, once per (size, tol) -----------------------------------------

_REF: dict = {}


def reference(oracle, n, m, tol):
    """dict(th, qp, aff, dth, dst) of the oracle for the batch of (n, m) at `tol`."""
    key = (n, m, tol)
    if key not in _REF:
        th = make_batch(n, m)
        kw = dict(trace_len=TRACE, tol=tol, linear_solver="schur")
        qp = oracle.solve_batch(0, n, m, th, **kw)
        aff = oracle.solve_batch(1, n, m, affine_embedding(th, n, m), **kw)
        dth, dst = oracle.vjp_batch(0, n, m, th, qp["x"], qp["y"], qp["s"], 2.0 * qp["x"], 2.0 * qp["y"], None)
        _REF[key] = dict(th=th, qp=qp, aff=aff, dth=dth, dst=dst)
    return _REF[key]


def shared_reference(oracle, n, m, tol, src):
    """Oracle solve of the batch whose every instance takes [M; A] of instance `src`."""
    key = (n, m, tol, "shared", src)
    if key not in _REF:
        th = make_batch(n, m)
        D = _abi.theta_shared_dim(0, n, m)
        full = np.ascontiguousarray(np.concatenate([np.broadcast_to(th[src, :D], (th.shape[0], D)), th[:, D:]], 1))
        qp = oracle.solve_batch(0, n, m, full, trace_len=TRACE, tol=tol, linear_solver="schur")
        _REF[key] = dict(shared=th[src, :D].copy(), var=np.ascontiguousarray(th[:, D:]), qp=qp, full=full)
    return _REF[key]


def shared_sources():
    """One instance of each kind lends its [M; A] to a shared-matrix batch."""
    sl = kind_slices()
    return [sl[k].start for k, _ in KINDS]


# ---- CPU: the inputs are what the docstring says -----------------------------------------

@pytest.mark.parametrize("n,m", SIZES)
def test_inputs_cover_the_cases(oracle_lib, n, m):
    r = reference(oracle_lib, n, m, 1e-6)
    th, st = r["th"], r["qp"]["status"]
    sl = kind_slices()
    assert th.shape[0] == 128
    assert (st[sl["plain"]] == 0).mean() >= 0.9           # full solves, not early exits
    M = th[:, :n * n].reshape(-1, n, n)
    sym = np.array([np.array_equal(a, a.T) for a in M])
    assert sym[sl["plain"]].all() and sym[sl["negz"]].all() and sym[sl["shift"]].all()
    assert not sym[sl["asym"]].any()
    neg0 = (M == 0.0) & np.signbit(M)
    eye = np.eye(n, dtype=bool)
    assert all((z & eye).any() and (z & ~eye).any() for z in neg0[sl["negz"]])
    assert np.isnan(M[sl["nan"]]).any() and not np.isnan(np.delete(th, sl["nan"].start, 0)).any()
    # asym: the fast pass defers whatever is not exactly symmetric (asserted above).  shift: the
    # first Newton step's S = M + tol·I + Aᵀ D⁻¹ A (x = 0, y = s = 1: D = tol + 1/(1 + tol)) is not
    # positive definite, so its pivot-free Gauss-Jordan meets a pivot ≤ 0 and the fast pass
    # defers the instance (no output field records the pass; the inputs force it)
    A = th[:, n * n:n * n + n * m].reshape(-1, n, m).transpose(0, 2, 1)  # [b, k, i] = A_ki
    tol = 1e-6
    S0 = M + tol * np.eye(n) + np.einsum("bki,bkj->bij", A, A) / (tol + 1.0 / (1.0 + tol))
    neg = np.array([np.linalg.eigvalsh(0.5 * (a + a.T)).min() < 0.0 for a in S0[sl["shift"]]])
    assert neg.mean() >= 0.5 if n > m else neg.any(), neg  # (the others may lose definiteness at a later step)
    assert not any(np.linalg.eigvalsh(a).min() < 0.0 for a in S0[sl["plain"]])
    # tol = 1e-2 changes the iterates of the plain instances
    r2 = reference(oracle_lib, n, m, 1e-2)
    assert not _same(r["qp"]["x"][sl["plain"]], r2["qp"]["x"][sl["plain"]])


# ---- GPU ------------------------------------------------------------------------------------

def gpu_compare(oracle, n, m, tol):
    """Every entry point against the oracle for one (size, tol); prints one line per call."""
    import torch

    from mcp_amd.batch import (solve_batch_device, solve_batch_shared_device, solve_vjp_batch_device,
                               solve_vjp_batch_shared_device)

    dev = torch.device("cuda", 0)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    r = reference(oracle, n, m, tol)
    kw = dict(tol=tol, linear_solver="schur")
    tag = f"({n}, {m}) tol={tol:g} "
    sl = kind_slices()

    got = _host(solve_batch_device(0, n, m, up(r["th"]), trace_len=TRACE, **kw))
    assert_fields_equal(got, r["qp"], what=tag + "qp: ")
    assert (got["status"][sl["plain"]] == 0).mean() >= 0.9
    assert set(np.unique(got["status"])) <= {0, 1}  # nothing left marked deferred

    got = _host(solve_batch_device(1, n, m, up(affine_embedding(r["th"], n, m)), trace_len=TRACE, **kw))
    assert_fields_equal(got, r["aff"], what=tag + "affine: ")

    out, dth, st = solve_vjp_batch_device(0, n, m, up(r["th"]), ct=(2.0, 2.0, 0.0), **kw)
    assert_fields_equal(_host(out), r["qp"], what=tag + "fused: ")
    assert _same(dth.cpu().numpy(), r["dth"]), tag + "fused: dθ differs"
    assert _same(st.cpu().numpy(), r["dst"]), tag + "fused: pullback status differs"

    for src in shared_sources():
        s = shared_reference(oracle, n, m, tol, src)
        got = _host(solve_batch_shared_device(0, n, m, up(s["shared"]), up(s["var"]), trace_len=TRACE, **kw))
        assert_fields_equal(got, s["qp"], what=tag + f"shared[{src}]: ")
    # the fused shared call on the plain shared block: the solve fields, and ∂[b; ϕ] = the
    # per-instance tail of the oracle's ∂θ′
    s = shared_reference(oracle, n, m, tol, 0)
    out, dvar, st = solve_vjp_batch_shared_device(0, n, m, up(s["shared"]), up(s["var"]), ct=(2.0, 2.0, 0.0), **kw)
    assert_fields_equal(_host(out), s["qp"], what=tag + "shared fused: ")
    q = s["qp"]
    odth, ost = oracle.vjp_batch(0, n, m, s["full"], q["x"], q["y"], q["s"], 2.0 * q["x"], 2.0 * q["y"], None)
    D = _abi.theta_shared_dim(0, n, m)
    assert _same(dvar.cpu().numpy(), odth[:, D:]), tag + "shared fused: ∂var differs"
    assert _same(st.cpu().numpy(), ost), tag + "shared fused: pullback status differs"


@pytest.mark.gpu
@pytest.mark.parametrize("tol", TOLS)
@pytest.mark.parametrize("n,m", SIZES)
def test_compile_time_kernels_equal_the_oracle(gpu, oracle_lib, n, m, tol):
    gpu_compare(oracle_lib, n, m, tol)


@pytest.mark.gpu
def test_generic_kernels_equal_the_oracle_in_a_child_process(gpu, oracle_lib):
    """The same inputs through the runtime-(n, m) kernels: MCPX_GENERIC_KERNELS=1 in a fresh process."""
    env = dict(os.environ, MCPX_GENERIC_KERNELS="1")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "helpers", "spec_trim_probe.py")], env=env,
                       cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "spec-trim-generic: OK" in r.stdout

"""The reduced gradient of a shared-matrix batch's matrix block on the GPU
(mcpx_vjp_batch_shared_reduce[_device]): dshared has the bits of the contract's fma chain
(include/mcpx.h) restated on the host (tests/helpers/shared_reduce_chain.py) from the x, y, dvar
and status of the plain split call; with one instance it is the full record's head; its value
agrees with the summed full-θ pullback within the rounding bound of two differently ordered
sums; excluded instances never reach it; and the bits do not move with the API, the host
shards, a NULL dvar, or a repeated call.

Inputs as in tests/test_shared_sens_gpu.py: instance 0's matrices shared, the iterate of the GPU
solve, the cotangents of f = Σx² + Σy²."""

from __future__ import annotations

import os
import subprocess
import sys

import numpy as np
import pytest

from mcp_amd import _abi
from mcp_amd.qp_benchmark import generate_random_parameter
from tests.helpers import shared_reduce_chain as chain
from tests.test_shared_theta_gpu import _same, materialise, shared_affine, shared_qp

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_CASES: dict = {}


@pytest.fixture(scope="module")
def restated(tmp_path_factory):
    """The contract's chain: the C form, or exact rationals where there is no gcc."""
    return chain.chain_c(tmp_path_factory.mktemp("reduce_chain")) or chain.chain_fraction


def make_case(fam, n, m, B):
    """One shape, computed once and read-only: the shared block, the iterate of the GPU solve,
    the cotangents of f = Σx² + Σy², and the plain split call's dvar / status."""
    from mcp_amd.batch import solve_batch_shared, vjp_batch_shared

    key = (fam, n, m, B)
    if key in _CASES:
        return _CASES[key]
    rng = np.random.default_rng(100 * n + m)
    shared, var = shared_qp(rng, n, m, B) if fam == 0 else shared_affine(rng, n, m, B)
    ls = "schur" if fam == 0 and m > 0 and n + m <= 64 else "reduced"
    r = solve_batch_shared(fam, n, m, shared, var, tol=1e-6, linear_solver=ls)
    c = dict(shared=shared, var=var, x=r["x"], y=r["y"], s=r["s"], solve_status=r["status"], gx=2.0 * r["x"],
             gy=2.0 * r["y"])
    c["dvar"], c["status"] = vjp_batch_shared(fam, n, m, shared, c["x"], c["y"], c["s"], c["gx"], c["gy"])
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    _CASES[key] = c
    return c


def reduce_host(fam, n, m, c, **kw):
    from mcp_amd.batch import vjp_batch_shared_reduce

    return vjp_batch_shared_reduce(fam, n, m, c["shared"], c["x"], c["y"], c["s"], c["gx"], c["gy"], **kw)


# ---- bits against the restated chain ---------------------------------------------------

@pytest.mark.parametrize("fam,n,m,B", [
    (0, 2, 2, 5),      # K tails of both tile kinds
    (0, 5, 3, 130),    # rows and columns that are no multiple of 16
    (0, 16, 8, 515),   # several full chunks and one of 3 instances: the fold
    (0, 32, 16, 300),
    (0, 7, 0, 9),      # no ∂A
    (0, 70, 40, 9),    # the workgroup pullback, several tiles
    (1, 6, 4, 259),    # affine
])
def test_bits_of_the_restated_chain(gpu, restated, fam, n, m, B):
    c = make_case(fam, n, m, B)
    assert 2 * int((c["status"] == 0).sum()) >= B  # not a sum over failures
    dsh, used, dvar, st = reduce_host(fam, n, m, c)
    assert _same(dvar, c["dvar"]) and _same(st, c["status"])
    want = restated(fam, n, m, c["x"], c["y"], c["dvar"], c["status"] == 0)
    assert dsh.shape == (_abi.theta_shared_dim(fam, n, m),)
    assert used == int((c["status"] == 0).sum())
    assert np.isfinite(dsh).all() and (dsh.any() or dsh.size == 0)
    assert chain.bits_equal(dsh, want), f"{int((dsh != want).sum())} of {dsh.size} entries differ"


@pytest.mark.parametrize("fam,n,m", [(0, 16, 8), (1, 6, 4)])
def test_one_instance_is_the_head_of_the_full_record(gpu, fam, n, m):
    from mcp_amd.batch import vjp_batch

    src = make_case(fam, n, m, 515 if fam == 0 else 259)
    c = {k: (v[:1] if k != "shared" else v) for k, v in src.items()}
    D = src["shared"].size
    dsh, used, _, st = reduce_host(fam, n, m, c)
    full, fst = vjp_batch(fam, n, m, materialise(c["shared"], c["var"], n + m), c["x"], c["y"], c["s"], c["gx"],
                          c["gy"])
    assert used == 1 and st[0] == 0 and fst[0] == 0
    assert np.array_equal(dsh, full[0, :D])  # as values: only the sign of a zero may differ


def test_value_agrees_with_the_summed_full_pullback(gpu):
    """(16, 8), B = 515 against Σ_b dtheta_full[b, :shared_dim] summed in numpy (the oracle-pinned
    full-θ path).  Both are sums of the same 2B products in different orders, so entry by entry
    they agree within 2·(B + 2)·2⁻⁵³·Σ_b(|term₁| + |term₂|): the standard bound, not a measured one."""
    from mcp_amd.batch import vjp_batch

    n, m, B = 16, 8, 515
    c = make_case(0, n, m, B)
    D = c["shared"].size
    full, fst = vjp_batch(0, n, m, materialise(c["shared"], c["var"], n + m), c["x"], c["y"], c["s"], c["gx"], c["gy"])
    assert (fst == 0).all() and (c["status"] == 0).all()
    dsh, used, _, _ = reduce_host(0, n, m, c)
    assert used == B
    ly, lx, x, y = np.abs(c["dvar"][:, :m]), np.abs(c["dvar"][:, m:]), np.abs(c["x"]), np.abs(c["y"])
    mag_m = np.einsum("bi,bj->ij", lx, x)                                       # |λx_i x_j|
    mag_a = np.einsum("bk,bj->kj", ly, x) + np.einsum("bj,bk->kj", lx, y)       # |λy_k x_j| + |λx_j y_k|
    mag = np.concatenate([mag_m.T.reshape(-1), mag_a.T.reshape(-1)])            # column-major blocks
    bound = 2.0 * (B + 2) * 2.0 ** -53 * mag
    err = np.abs(dsh - full[:, :D].sum(0))
    print(f"max err / bound = {float(np.max(err / bound)):.3e}")
    assert (err <= bound).all()


# ---- exclusion ---------------------------------------------------------------------------

def test_excluded_instances_never_reach_the_sum(gpu, restated):
    """The singular-∇F_z inputs of tests/test_shared_sens_gpu.py::test_singular_jacobian (instance 0:
    y₀ = s₀ = 0 → status 1, a NaN row) in a batch of 6, and a skip mask over two more."""
    from mcp_amd.batch import vjp_batch_shared, vjp_batch_shared_reduce

    n, m, B = 4, 2, 6
    rng = np.random.default_rng(5)
    th = generate_random_parameter(rng, n, m, 0.0, batch=B)
    shared = th[0, :_abi.theta_shared_dim(0, n, m)].copy()
    x, y, s = np.ones((B, n)), rng.uniform(0.5, 2.0, (B, m)), rng.uniform(0.25, 1.0, (B, m))
    y[0, 0] = s[0, 0] = 0.0
    gx = np.ones((B, n))
    skip = np.array([0, 0, 1, 0, 1, 0], np.uint8)
    dv0, st0 = vjp_batch_shared(0, n, m, shared, x, y, s, gx)
    assert st0.tolist() == [1, 0, 0, 0, 0, 0] and np.isnan(dv0[0]).all()
    dsh, used, dvar, st = vjp_batch_shared_reduce(0, n, m, shared, x, y, s, gx, skip=skip)
    assert used == B - 3
    assert np.isfinite(dsh).all() and dsh.any()
    assert chain.bits_equal(dsh, restated(0, n, m, x, y, dv0, (st0 == 0) & (skip == 0)))
    assert _same(dvar, dv0) and _same(st, st0) and np.isnan(dvar[0]).all()  # dvar still carries the NaN row
    # the same sum over the three included instances alone, had they been the whole batch
    keep = np.array([1, 3, 5])
    alone, used3, _, _ = vjp_batch_shared_reduce(0, n, m, shared, x[keep], y[keep], s[keep], gx[keep])
    assert used3 == 3 and chain.bits_equal(dsh, alone)


# ---- invariance --------------------------------------------------------------------------

def test_device_api_null_dvar_and_a_second_call_give_the_same_bits(gpu):
    import torch

    from mcp_amd.batch import vjp_batch_shared_reduce_device

    n, m, B = 16, 8, 515
    c = make_case(0, n, m, B)
    dev = torch.device("cuda", 0)
    T = lambda a: torch.from_numpy(np.array(a)).to(dev)  # (a copy: the case's arrays are read-only)
    sh, x, y, s, gx, gy = (T(c[k]) for k in ("shared", "x", "y", "s", "gx", "gy"))
    host = reduce_host(0, n, m, c)
    host_null = reduce_host(0, n, m, c, want_dvar=False)
    assert host_null[2] is None
    first = vjp_batch_shared_reduce_device(0, n, m, sh, x, y, s, gx, gy)
    second = vjp_batch_shared_reduce_device(0, n, m, sh, x, y, s, gx, gy)
    # caller-provided outputs (poisoned: every entry must be written), dvar NULL
    dsh = torch.full((sh.numel(),), float("nan"), dtype=torch.float64, device=dev)
    used = torch.full((1,), -7, dtype=torch.int64, device=dev)
    null = vjp_batch_shared_reduce_device(0, n, m, sh, x, y, s, gx, gy, dshared=dsh, used=used, want_dvar=False)
    assert null[0] is dsh and null[1] is used and null[2] is None
    skip0 = vjp_batch_shared_reduce_device(0, n, m, sh, x, y, s, gx, gy,
                                           skip=torch.zeros(B, dtype=torch.bool, device=dev))
    torch.cuda.synchronize()
    for r in (host_null, first, second, null, skip0):
        got = r[0] if isinstance(r[0], np.ndarray) else r[0].cpu().numpy()
        assert chain.bits_equal(got, host[0])
        assert int(r[1]) == host[1] == B
    for r in (first, second, skip0):
        assert _same(r[2].cpu().numpy(), c["dvar"]) and _same(r[3].cpu().numpy(), c["status"])


def test_capped_partials_block_gives_the_same_bits(gpu, monkeypatch):
    """MCPX_REDUCE_CAP_KB=8 (read at every call): the partials block holds two chunks of the
    (16, 8) shape, so B = 515 goes through it in groups — the device fold continues from dshared,
    the host copy lands at each group's offset — and the bits are those of one group."""
    import torch

    from mcp_amd.batch import vjp_batch_shared_reduce_device

    n, m, B = 16, 8, 515
    c = make_case(0, n, m, B)
    assert c["shared"].size * 8 * 3 > 8 * 1024 and -(-B // _abi.REDUCE_CHUNK) >= 3  # more than one group
    dev = torch.device("cuda", 0)
    T = lambda a: torch.from_numpy(np.array(a)).to(dev)
    args = [T(c[k]) for k in ("shared", "x", "y", "s", "gx", "gy")]
    skip = np.zeros(B, np.uint8)
    skip[[5, 300, 514]] = 1
    whole = reduce_host(0, n, m, c, skip=skip)
    monkeypatch.setenv("MCPX_REDUCE_CAP_KB", "8")
    host = reduce_host(0, n, m, c, skip=skip)
    d = vjp_batch_shared_reduce_device(0, n, m, *args, skip=T(skip))
    torch.cuda.synchronize()
    monkeypatch.delenv("MCPX_REDUCE_CAP_KB")
    assert whole[1] == B - 3 and whole[0].any()
    assert chain.bits_equal(host[0], whole[0]) and host[1] == whole[1]
    assert chain.bits_equal(d[0].cpu().numpy(), whole[0]) and int(d[1]) == whole[1]


def test_device_api_empty_batch(gpu):
    import torch

    from mcp_amd.batch import vjp_batch_shared_reduce_device

    n, m = 3, 2
    dev = torch.device("cuda", 0)
    z = lambda *shape: torch.zeros(*shape, dtype=torch.float64, device=dev)
    dsh = torch.full((n * n + m * n,), float("nan"), dtype=torch.float64, device=dev)
    used = torch.full((1,), -7, dtype=torch.int64, device=dev)
    vjp_batch_shared_reduce_device(0, n, m, z(n * n + m * n), z(0, n), z(0, m), z(0, m), dshared=dsh, used=used)
    torch.cuda.synchronize()
    assert chain.bits_equal(dsh.cpu().numpy(), np.zeros(n * n + m * n)) and int(used) == 0


def test_host_shards_in_a_child_process(gpu):
    """MCPX_HOST_SHARDS=3 over B = 515 (shards cut at multiples of MCPX_REDUCE_CHUNK, the last one
    ragged) equals one shard, bit for bit."""
    env = dict(os.environ, MCPX_HOST_SHARDS="3")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "helpers", "shared_reduce_shards_probe.py")],
                       env=env, cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "shared-reduce-shards: OK" in r.stdout


# ---- torch autograd ------------------------------------------------------------------------

def test_solve_shared_torch_backward(gpu):
    import torch

    from mcp_amd.autodiff import solve_shared_torch
    from mcp_amd.batch import vjp_batch_shared_device, vjp_batch_shared_reduce_device

    n, m, B = 16, 8, 515
    c = make_case(0, n, m, B)
    dev = torch.device("cuda", 0)
    sh = torch.from_numpy(np.array(c["shared"])).to(dev).requires_grad_(True)
    var = torch.from_numpy(np.array(c["var"])).to(dev).requires_grad_(True)
    sol = solve_shared_torch(0, n, m, sh, var, tol=1e-6, linear_solver="schur")
    assert sol.used is None
    ((sol.x ** 2).sum() + (sol.y ** 2).sum()).backward()
    x, y, s = sol.x.detach(), sol.y.detach(), sol.s.detach()
    assert _same(x.cpu().numpy(), c["x"]) and (sol.status.cpu().numpy() == 0).all()
    g = (2.0 * x, 2.0 * y, torch.zeros_like(s))
    ref = vjp_batch_shared_reduce_device(0, n, m, sh.detach(), x, y, s, *g, skip=(sol.status != 0).to(torch.uint8))
    dv, st = vjp_batch_shared_device(0, n, m, sh.detach(), x, y, s, *g)
    torch.cuda.synchronize()
    assert sh.grad.shape == sh.shape and var.grad.shape == var.shape
    assert chain.bits_equal(sh.grad.cpu().numpy(), ref[0].cpu().numpy()) and sh.grad.abs().sum() > 0
    assert chain.bits_equal(var.grad.cpu().numpy(), dv.cpu().numpy())
    assert int(sol.used) == int(ref[1]) == B and (st.cpu().numpy() == 0).all()

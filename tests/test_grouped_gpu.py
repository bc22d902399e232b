"""Grouped shared-matrix batches on the GPU (mcpx_{solve,vjp}_batch_grouped[_device],
mcpx_vjp_batch_grouped_reduce[_device]): G matrix blocks, each shared by a run of instances.  Every
comparison is bitwise.  The solve's eleven output fields equal the full-θ call on the materialised
θ′ and the shared call on each group alone; dvar / status equal the shared pullback per group;
dshared[g] / used[g] equal the shared reduce call on group g alone and the contract's chain restated
on the host (tests/helpers/shared_reduce_chain.py).

Group shape [70, 0, 1, 65, 130] (B = 266): a short second chunk, an empty group, a lone instance,
64 + 1 and 2·64 + 2.  Inputs: qp_benchmark.generate_random_parameter and the helpers of
tests/test_shared_theta_gpu.py, one set of matrices per group."""

from __future__ import annotations

import os
import subprocess
import sys

import numpy as np
import pytest

from mcp_amd import _abi
from mcp_amd.qp_benchmark import generate_random_parameter
from tests.helpers import shared_reduce_chain as chain
from tests.test_shared_theta_gpu import (TRACE, _same, _to_host, assert_all_fields_equal, shared_affine)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = (70, 0, 1, 65, 130)
PROBE = os.path.join(ROOT, "tests", "helpers", "grouped_probe.py")
_CASES: dict = {}


def spans(sizes):
    off = np.concatenate([[0], np.cumsum(sizes)])
    return [(int(off[g]), int(off[g + 1])) for g in range(len(sizes))]


def grouped_inputs(rng, fam, n, m, sizes, zero_s=False):
    """(blocks (G, shared_dim): one random problem's matrices per group, var (B, n + m))."""
    G, B, D = len(sizes), int(sum(sizes)), _abi.theta_shared_dim(fam, n, m)
    if fam == 0:
        blocks = generate_random_parameter(rng, n, m, 0.0, batch=G)[:, :D].copy()
    else:
        blocks = np.stack([shared_affine(rng, n, m, 1, zero_s=zero_s)[0] for _ in range(G)])
    return blocks, rng.standard_normal((B, n + m))


def materialise(blocks, var, sizes, dv):
    rows = np.repeat(np.arange(len(sizes)), sizes)
    return np.ascontiguousarray(np.concatenate([blocks[rows], var[:, :dv]], 1))


def padded(a, extra):
    """`a` as a view into a wider array whose extra columns are NaN."""
    wide = np.full((a.shape[0], a.shape[1] + extra), np.nan)
    wide[:, :a.shape[1]] = a
    return wide[:, :a.shape[1]], wide


def rows_of(out, a, b):
    return {k: (None if v is None else v[a:b]) for k, v in out.items()}


def device_solves(fam, n, m, blocks, var, sizes, warm=None, pad=0, per_group=True, **kw):
    """(grouped call, full-θ call on the materialised θ′, the shared call per non-empty group) through
    the device API, as host dicts.  pad: NaN columns behind every block and every var row."""
    import torch

    from mcp_amd.batch import solve_batch_device, solve_batch_grouped_device, solve_batch_shared_device

    dev = torch.device("cuda", 0)
    up = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    w = {k: up(v) for k, v in (warm or {}).items()}
    tb, tv = up(blocks), up(var)
    if pad:
        tb = up(padded(blocks, pad)[1])[:, :blocks.shape[1]]  # a padded 2-D view
        tv = up(padded(var, pad)[1])  # theta_ld = n + m + pad
    got = solve_batch_grouped_device(fam, n, m, tb, tv, sizes, trace_len=TRACE, **w, **kw)
    ref = solve_batch_device(fam, n, m, up(materialise(blocks, var, sizes, n + m)), trace_len=TRACE, **w, **kw)
    alone = []
    for g, (a, b) in enumerate(spans(sizes)):
        if per_group and b > a:
            wg = {k: v[a:b].contiguous() for k, v in w.items()}
            alone.append((a, b, solve_batch_shared_device(fam, n, m, up(blocks[g]), up(var[a:b]), trace_len=TRACE,
                                                          **wg, **kw)))
    torch.cuda.synchronize()
    return _to_host(got), _to_host(ref), [(a, b, _to_host(o)) for a, b, o in alone]


def check_solves(got, ref, alone):
    assert_all_fields_equal(got, ref)
    for a, b, o in alone:
        assert_all_fields_equal(rows_of(got, a, b), o)
    assert (ref["status"] == 0).any()  # not a comparison of failures


# ---- solve: the in-kernel path (QP, SCHUR, one wave) ------------------------------------------

@pytest.mark.parametrize("n,m", [(16, 8), (32, 16), (2, 2), (5, 3)])
def test_solve_in_kernel(gpu, n, m):
    blocks, var = grouped_inputs(np.random.default_rng(100 * n + m), 0, n, m, SIZES)
    check_solves(*device_solves(0, n, m, blocks, var, SIZES, tol=1e-6, linear_solver="schur"))


def test_solve_in_kernel_generic_in_a_child_process(gpu):
    """(16, 8) through the runtime-(n, m) kernels: MCPX_GENERIC_KERNELS=1 in a fresh process."""
    r = subprocess.run([sys.executable, PROBE, "generic"], env=dict(os.environ, MCPX_GENERIC_KERNELS="1"), cwd=ROOT,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "grouped-generic: OK" in r.stdout


@pytest.mark.parametrize("ls", ["schur", "reduced"])
def test_solve_padded_strides_with_nan_padding(gpu, ls):
    n, m = 16, 8
    blocks, var = grouped_inputs(np.random.default_rng(21), 0, n, m, SIZES)
    got, ref, alone = device_solves(0, n, m, blocks, var, SIZES, pad=3, tol=1e-6, linear_solver=ls)
    check_solves(got, ref, alone)
    assert not np.isnan(got["x"]).any()  # the padding was not read


def test_solve_warm_starts(gpu):
    n, m, B = 16, 8, sum(SIZES)
    rng = np.random.default_rng(22)
    blocks, var = grouped_inputs(rng, 0, n, m, SIZES)
    warm = dict(x0=rng.standard_normal((B, n)), y0=rng.uniform(0.5, 2.0, (B, m)), s0=rng.uniform(0.5, 2.0, (B, m)))
    got, ref, alone = device_solves(0, n, m, blocks, var, SIZES, warm=warm, tol=1e-6, linear_solver="schur")
    check_solves(got, ref, alone)
    cold, _, _ = device_solves(0, n, m, blocks, var, SIZES, per_group=False, tol=1e-6, linear_solver="schur")
    assert not _same(cold["newton_iters"], got["newton_iters"])  # the warm starts were read


def test_one_group_with_an_asymmetric_m(gpu):
    """M[1, 0] += 1e-3 in group 3's block only: its 65 instances are deferred to pass 2 (the bits of
    the full-θ call, which defers them too); the other groups' bits are those of the batch in
    which every M is symmetric."""
    n, m = 16, 8
    blocks, var = grouped_inputs(np.random.default_rng(23), 0, n, m, SIZES)
    sym, _, _ = device_solves(0, n, m, blocks, var, SIZES, per_group=False, tol=1e-6, linear_solver="schur")
    skew = blocks.copy()
    skew[3, 1] += 1e-3
    got, ref, alone = device_solves(0, n, m, skew, var, SIZES, tol=1e-6, linear_solver="schur")
    check_solves(got, ref, alone)
    assert set(np.unique(got["status"])) <= {0, 1}  # no instance is left marked deferred
    a, b = spans(SIZES)[3]
    assert_all_fields_equal(rows_of(got, 0, a), rows_of(sym, 0, a))
    assert_all_fields_equal(rows_of(got, b, None), rows_of(sym, b, None))
    assert not _same(got["x"][a:b], sym["x"][a:b])


# ---- solve: the expansion path -------------------------------------------------------------------

@pytest.mark.parametrize("fam,n,m,ls", [
    (0, 16, 8, "reduced"), (0, 16, 8, "dense"), (1, 6, 4, "reduced"),
    (0, 40, 20, "reduced"),  # one workgroup per instance
])
def test_solve_expansion_path(gpu, fam, n, m, ls):
    blocks, var = grouped_inputs(np.random.default_rng(1000 * fam + 10 * n + m), fam, n, m, SIZES)
    check_solves(*device_solves(fam, n, m, blocks, var, SIZES, tol=1e-6, linear_solver=ls))


@pytest.mark.parametrize("n,m,scale", [(16, 8, 3), (40, 20, 1)])
def test_solve_expansion_slices_straddle_groups(gpu, monkeypatch, n, m, scale):
    """A 1 MiB expansion block holds 321 instances of the (16, 8) θ′ and 53 of the (40, 20) one: the
    slice boundaries (321 and 642 of 798 instances; every 53 of 266) fall inside groups."""
    monkeypatch.setenv("MCPX_EXPAND_MB", "1")
    sizes = tuple(scale * k for k in SIZES)
    per = (1 << 20) // (8 * ((_abi.theta_dim(0, n, m) + 1) & ~1))
    inner = [b for b in range(per, sum(sizes), per) if all(b not in (lo, hi) for lo, hi in spans(sizes))]
    assert inner  # a slice boundary inside a group
    blocks, var = grouped_inputs(np.random.default_rng(7 + n), 0, n, m, sizes)
    check_solves(*device_solves(0, n, m, blocks, var, sizes, per_group=False, tol=1e-6, linear_solver="reduced"))


# ---- solve: the APIs --------------------------------------------------------------------------------

@pytest.mark.parametrize("ls", ["schur", "reduced"])
def test_solve_host_api_equals_device_api(gpu, ls):
    from mcp_amd.batch import solve_batch_grouped

    n, m, B = 16, 8, sum(SIZES)
    rng = np.random.default_rng(25)
    blocks, var = grouped_inputs(rng, 0, n, m, SIZES)
    warm = dict(x0=rng.standard_normal((B, n)))
    got, ref, _ = device_solves(0, n, m, blocks, var, SIZES, warm=warm, per_group=False, tol=1e-6, linear_solver=ls)
    host = solve_batch_grouped(0, n, m, padded(blocks, 5)[0], var, SIZES, trace_len=TRACE, tol=1e-6, linear_solver=ls,
                               **warm)
    assert_all_fields_equal(host, got)
    assert_all_fields_equal(host, ref)


@pytest.mark.parametrize("mode,env", [
    ("shards", dict(MCPX_HOST_SHARDS="3", MCPX_HOST_CHUNK="1024")),
    ("reduce-shards", dict(MCPX_HOST_SHARDS="3")),
])
def test_host_shards_in_a_child_process(gpu, mode, env):
    """shards: the solve and the pullback on B = 3,000 in 5 uneven groups, three shards of chunks of
    1,024.  reduce-shards: the reduce call's shards, cut at chunk boundaries of the grouped table."""
    r = subprocess.run([sys.executable, PROBE, mode], env=dict(os.environ, **env), cwd=ROOT, capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert f"grouped-{mode}: OK" in r.stdout


# ---- the pullback and the reduced gradient ----------------------------------------------------------

@pytest.fixture(scope="module")
def restated(tmp_path_factory):
    """The contract's chain: the C form, or exact rationals where there is no gcc."""
    return chain.chain_c(tmp_path_factory.mktemp("grouped_chain")) or chain.chain_fraction


def make_case(fam, n, m, sizes):
    """One shape, computed once and read-only: the blocks, the iterate of the grouped GPU solve, the
    cotangents of f = Σx² + Σy², and per group the shared calls' dvar / status / dshared / used."""
    from mcp_amd.batch import solve_batch_grouped, vjp_batch_shared_reduce

    key = (fam, n, m, tuple(sizes))
    if key in _CASES:
        return _CASES[key]
    blocks, var = grouped_inputs(np.random.default_rng(100 * n + m + 7), fam, n, m, sizes)
    ls = "schur" if fam == 0 and n + m <= 64 else "reduced"
    r = solve_batch_grouped(fam, n, m, blocks, var, sizes, tol=1e-6, linear_solver=ls)
    B, D = int(sum(sizes)), blocks.shape[1]
    c = dict(blocks=blocks, x=r["x"], y=r["y"], s=r["s"], gx=2.0 * r["x"], gy=2.0 * r["y"], sizes=tuple(sizes),
             skip=(np.random.default_rng(5).uniform(size=B) < 0.1).astype(np.uint8))
    c["dvar"], c["status"] = np.empty((B, n + m)), np.empty(B, np.int32)
    c["dshared"], c["used"] = np.empty((len(sizes), D)), np.empty(len(sizes), np.int64)
    c["dshared_skip"], c["used_skip"] = c["dshared"].copy(), c["used"].copy()
    for g, (a, b) in enumerate(spans(sizes)):  # the shared calls on each group alone (host API)
        if b == a:
            c["dshared"][g] = c["dshared_skip"][g] = 0.0
            c["used"][g] = c["used_skip"][g] = 0
            continue
        args = (fam, n, m, blocks[g], c["x"][a:b], c["y"][a:b], c["s"][a:b], c["gx"][a:b], c["gy"][a:b])
        c["dshared"][g], c["used"][g], c["dvar"][a:b], c["status"][a:b] = vjp_batch_shared_reduce(*args)
        c["dshared_skip"][g], c["used_skip"][g], _, _ = vjp_batch_shared_reduce(*args, skip=c["skip"][a:b])
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    _CASES[key] = c
    return c


SHAPES = [(0, 16, 8, SIZES), (0, 5, 3, SIZES), (1, 6, 4, SIZES), (0, 70, 40, (4, 0, 5))]


def on_device(c, *keys):
    import torch

    return [torch.from_numpy(np.array(c[k])).to("cuda:0") for k in keys]  # (a copy: the arrays are read-only)


@pytest.mark.parametrize("fam,n,m,sizes", SHAPES)
def test_vjp_equals_the_shared_call_per_group(gpu, fam, n, m, sizes):
    import torch

    from mcp_amd.batch import vjp_batch_grouped, vjp_batch_grouped_device, vjp_batch_shared

    c = make_case(fam, n, m, sizes)
    assert 2 * int((c["status"] == 0).sum()) >= sum(sizes)  # not a comparison of failures
    a, b = spans(sizes)[-1]  # (the case's per-group reference is the reduce call's dvar: pin it to the plain call)
    dv, st = vjp_batch_shared(fam, n, m, c["blocks"][-1], c["x"][a:b], c["y"][a:b], c["s"][a:b], c["gx"][a:b],
                              c["gy"][a:b])
    assert _same(dv, c["dvar"][a:b]) and _same(st, c["status"][a:b])
    dvar, status = vjp_batch_grouped(fam, n, m, padded(c["blocks"], 2)[0], c["x"], c["y"], c["s"], sizes, c["gx"], c["gy"])
    assert _same(dvar, c["dvar"]) and _same(status, c["status"])
    ddv, dst = vjp_batch_grouped_device(fam, n, m, *on_device(c, "blocks", "x", "y", "s"), sizes,
                                        *on_device(c, "gx", "gy"))
    torch.cuda.synchronize()
    assert _same(ddv.cpu().numpy(), c["dvar"]) and _same(dst.cpu().numpy(), c["status"])


def test_vjp_singular_jacobian_in_one_group(gpu):
    """The singular-∇F_z inputs of tests/test_shared_sens_gpu.py (y₀ = s₀ = 0) at the first instance of
    group 2: a NaN row and status 1, as the shared call on that group gives; the rest untouched."""
    from mcp_amd.batch import vjp_batch_grouped, vjp_batch_grouped_reduce, vjp_batch_shared

    n, m, sizes = 4, 2, (2, 0, 3, 1)
    B = sum(sizes)
    rng = np.random.default_rng(5)
    blocks, _ = grouped_inputs(rng, 0, n, m, sizes)
    x, y, s = np.ones((B, n)), rng.uniform(0.5, 2.0, (B, m)), rng.uniform(0.25, 1.0, (B, m))
    y[2, 0] = s[2, 0] = 0.0
    gx = np.ones((B, n))
    dvar, st = vjp_batch_grouped(0, n, m, blocks, x, y, s, sizes, gx)
    assert st.tolist() == [0, 0, 1, 0, 0, 0] and np.isnan(dvar[2]).all() and np.isfinite(np.delete(dvar, 2, 0)).all()
    for g, (a, b) in enumerate(spans(sizes)):
        if b > a:
            dv, s1 = vjp_batch_shared(0, n, m, blocks[g], x[a:b], y[a:b], s[a:b], gx[a:b])
            assert _same(dvar[a:b], dv) and _same(st[a:b], s1)
    dsh, used, dv2, st2 = vjp_batch_grouped_reduce(0, n, m, blocks, x, y, s, sizes, gx)
    assert used.tolist() == [2, 0, 2, 1] and np.isfinite(dsh).all()  # the NaN row never reaches the sum
    assert _same(dv2, dvar) and _same(st2, st)


@pytest.mark.parametrize("fam,n,m,sizes", SHAPES)
def test_reduce_equals_the_shared_call_per_group_and_the_restated_chain(gpu, restated, fam, n, m, sizes):
    import torch

    from mcp_amd.batch import vjp_batch_grouped_reduce, vjp_batch_grouped_reduce_device

    c = make_case(fam, n, m, sizes)
    G, D = len(sizes), c["blocks"].shape[1]
    args = (c["x"], c["y"], c["s"], sizes, c["gx"], c["gy"])
    dsh, used, dvar, st = vjp_batch_grouped_reduce(fam, n, m, padded(c["blocks"], 3)[0], *args)
    assert dsh.shape == (G, D) and used.shape == (G,)
    assert chain.bits_equal(dsh, c["dshared"]) and np.array_equal(used, c["used"])
    assert _same(dvar, c["dvar"]) and _same(st, c["status"])
    assert np.isfinite(dsh).all() and all(dsh[g].any() == (k > 0) for g, k in enumerate(sizes))
    for g, (a, b) in enumerate(spans(sizes)):
        want = restated(fam, n, m, c["x"][a:b], c["y"][a:b], c["dvar"][a:b], c["status"][a:b] == 0)
        assert chain.bits_equal(dsh[g], want), f"group {g}: {int((dsh[g] != want).sum())} of {D} entries differ"
        assert used[g] == int((c["status"][a:b] == 0).sum())
    # skip, and a NULL dvar
    sk = vjp_batch_grouped_reduce(fam, n, m, c["blocks"], *args, skip=c["skip"], want_dvar=False)
    assert chain.bits_equal(sk[0], c["dshared_skip"]) and np.array_equal(sk[1], c["used_skip"]) and sk[2] is None
    assert _same(sk[3], c["status"])
    # the device API: caller-provided outputs in a padded view, poisoned — every entry must be written
    wide = torch.full((G, D + 3), float("nan"), dtype=torch.float64, device="cuda:0")
    du = torch.full((G,), -7, dtype=torch.int64, device="cuda:0")
    targs = (*on_device(c, "blocks", "x", "y", "s"), sizes, *on_device(c, "gx", "gy"))
    d1 = vjp_batch_grouped_reduce_device(fam, n, m, *targs, dshared=wide[:, :D], used=du, want_dvar=False)
    d2 = vjp_batch_grouped_reduce_device(fam, n, m, *targs, skip=on_device(c, "skip")[0])
    torch.cuda.synchronize()
    assert d1[2] is None and torch.isnan(wide[:, D:]).all()  # the padding of dshared is not written
    assert chain.bits_equal(wide[:, :D].cpu().numpy(), c["dshared"]) and np.array_equal(du.cpu().numpy(), c["used"])
    assert chain.bits_equal(d2[0].cpu().numpy(), c["dshared_skip"])
    assert np.array_equal(d2[1].cpu().numpy(), c["used_skip"])
    assert _same(d2[2].cpu().numpy(), c["dvar"]) and _same(d2[3].cpu().numpy(), c["status"])


def test_reduce_portion_boundary_inside_a_group(gpu, monkeypatch):
    """MCPX_REDUCE_CAP_KB=9: three (16, 8) partials (3 KB each) per portion.  The table's 8 chunks —
    groups 0: 2, 2: 1, 3: 2, 4: 3 — go through in portions [0, 3), [3, 6), [6, 8): the last boundary
    falls inside the 130-instance group, whose chain the next fold continues from dshared[4]."""
    import torch

    from mcp_amd.batch import vjp_batch_grouped_reduce, vjp_batch_grouped_reduce_device

    n, m = 16, 8
    c = make_case(0, n, m, SIZES)
    assert c["blocks"].shape[1] * 8 * 3 <= 9 * 1024 < c["blocks"].shape[1] * 8 * 4
    monkeypatch.setenv("MCPX_REDUCE_CAP_KB", "9")
    host = vjp_batch_grouped_reduce(0, n, m, c["blocks"], c["x"], c["y"], c["s"], SIZES, c["gx"], c["gy"],
                                    skip=c["skip"])
    d = vjp_batch_grouped_reduce_device(0, n, m, *on_device(c, "blocks", "x", "y", "s"), SIZES,
                                        *on_device(c, "gx", "gy"), skip=on_device(c, "skip")[0])
    torch.cuda.synchronize()
    monkeypatch.delenv("MCPX_REDUCE_CAP_KB")
    assert chain.bits_equal(host[0], c["dshared_skip"]) and np.array_equal(host[1], c["used_skip"])
    assert chain.bits_equal(d[0].cpu().numpy(), c["dshared_skip"]) and np.array_equal(d[1].cpu().numpy(), c["used_skip"])


def test_device_api_empty_batch_and_empty_groups(gpu):
    import torch

    from mcp_amd.batch import vjp_batch_grouped_reduce_device

    n, m, G = 3, 2, 3
    D = n * n + m * n
    z = lambda *shape: torch.zeros(*shape, dtype=torch.float64, device="cuda:0")
    dsh = torch.full((G, D), float("nan"), dtype=torch.float64, device="cuda:0")
    used = torch.full((G,), -7, dtype=torch.int64, device="cuda:0")
    vjp_batch_grouped_reduce_device(0, n, m, z(G, D), z(0, n), z(0, m), z(0, m), (0, 0, 0), dshared=dsh, used=used)
    torch.cuda.synchronize()
    assert chain.bits_equal(dsh.cpu().numpy(), np.zeros((G, D))) and (used.cpu().numpy() == 0).all()


# ---- no cap on the number of groups --------------------------------------------------------------------

def test_66000_groups_of_one_instance(gpu):
    """QP (2, 2), G = B = 66,000 (past the 65,535 rows of a grid dimension): the solve equals the
    full-θ call; dshared[g] is the head of instance g's full-θ pullback record as values (only the
    sign of a zero may differ, as in test_one_instance_is_the_head_of_the_full_record); used is ones."""
    import torch

    from mcp_amd.batch import (solve_batch_device, solve_batch_grouped_device, vjp_batch_device,
                               vjp_batch_grouped_reduce_device)

    n, m, G = 2, 2, 66000
    D = _abi.theta_shared_dim(0, n, m)
    full = torch.from_numpy(generate_random_parameter(np.random.default_rng(66), n, m, 0.0, batch=G)).to("cuda:0")
    blocks, var, sizes = full[:, :D], full[:, D:].contiguous(), np.ones(G, np.int64)  # blocks: a padded view
    got = solve_batch_grouped_device(0, n, m, blocks, var, sizes, trace_len=TRACE, tol=1e-6, linear_solver="schur")
    ref = solve_batch_device(0, n, m, full, trace_len=TRACE, tol=1e-6, linear_solver="schur")
    x, y, s = got["x"], got["y"], got["s"]
    dsh, used, dvar, st = vjp_batch_grouped_reduce_device(0, n, m, blocks, x, y, s, sizes, 2.0 * x, 2.0 * y)
    rec, rst = vjp_batch_device(0, n, m, full, x, y, s, 2.0 * x, 2.0 * y)
    torch.cuda.synchronize()
    assert_all_fields_equal(_to_host(got), _to_host(ref))
    ok = (st == 0).cpu().numpy()
    assert ok.mean() > 0.9 and np.array_equal(ok, (rst == 0).cpu().numpy())
    assert np.array_equal(used.cpu().numpy(), ok.astype(np.int64))
    assert np.array_equal(dsh.cpu().numpy()[ok], rec[:, :D].cpu().numpy()[ok])  # as values
    assert _same(dvar.cpu().numpy(), rec[:, D:].cpu().numpy())
    assert (dsh.cpu().numpy()[~ok] == 0).all()  # a singular instance is left out of its group's sum


# ---- torch autograd ------------------------------------------------------------------------------------

def test_solve_grouped_torch_backward(gpu):
    """(16, 8), groups [70, 65]: the gradients equal solve_shared_torch on each group alone bit for
    bit, and — the check tests/test_shared_reduce_gpu.py applies to solve_shared_torch — the direct
    reduce and pullback calls at the returned iterate."""
    import torch

    from mcp_amd.autodiff import solve_grouped_torch, solve_shared_torch
    from mcp_amd.batch import vjp_batch_grouped_device, vjp_batch_grouped_reduce_device

    n, m, sizes = 16, 8, (70, 65)
    blocks, var = grouped_inputs(np.random.default_rng(31), 0, n, m, sizes)
    dev = torch.device("cuda", 0)
    sh = torch.from_numpy(blocks).to(dev).requires_grad_(True)
    tv = torch.from_numpy(var).to(dev).requires_grad_(True)
    sol = solve_grouped_torch(0, n, m, sh, tv, sizes, tol=1e-6, linear_solver="schur")
    assert sol.used is None
    ((sol.x ** 2).sum() + (sol.y ** 2).sum()).backward()
    x, y, s = sol.x.detach(), sol.y.detach(), sol.s.detach()
    assert (sol.status.cpu().numpy() == 0).all()
    g = (2.0 * x, 2.0 * y, torch.zeros_like(s))
    ref = vjp_batch_grouped_reduce_device(0, n, m, sh.detach(), x, y, s, sizes, *g,
                                          skip=(sol.status != 0).to(torch.uint8))
    dv, st = vjp_batch_grouped_device(0, n, m, sh.detach(), x, y, s, sizes, *g)
    torch.cuda.synchronize()
    assert sh.grad.shape == sh.shape and tv.grad.shape == tv.shape
    assert chain.bits_equal(sh.grad.cpu().numpy(), ref[0].cpu().numpy()) and sh.grad.abs().sum() > 0
    assert chain.bits_equal(tv.grad.cpu().numpy(), dv.cpu().numpy())
    assert sol.used.shape == (2,) and sol.used.tolist() == ref[1].tolist() == list(sizes)
    assert (st.cpu().numpy() == 0).all()
    for k, (a, b) in enumerate(spans(sizes)):
        s1 = torch.from_numpy(blocks[k]).to(dev).requires_grad_(True)
        v1 = torch.from_numpy(var[a:b]).to(dev).requires_grad_(True)
        one = solve_shared_torch(0, n, m, s1, v1, tol=1e-6, linear_solver="schur")
        ((one.x ** 2).sum() + (one.y ** 2).sum()).backward()
        assert chain.bits_equal(sh.grad[k].cpu().numpy(), s1.grad.cpu().numpy())
        assert chain.bits_equal(tv.grad[a:b].cpu().numpy(), v1.grad.cpu().numpy())
        assert int(one.used) == int(sol.used[k])

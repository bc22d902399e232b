"""Child process of tests/test_grouped_gpu.py, for the switches that are read from the
environment (set by the parent).  One mode per run; prints "grouped-<mode>: OK" and exits 0.

  generic        MCPX_GENERIC_KERNELS=1: the grouped (16, 8) SCHUR solve through the runtime-(n, m)
                 kernels against the full-θ call on the materialised θ′ and the shared call per group.
  shards         MCPX_HOST_SHARDS=3, MCPX_HOST_CHUNK=1024: B = 3,000 in 5 uneven groups — the host
                 solve (in-kernel and expansion path) and the host pullback against the full-θ host
                 solve and the same calls as one shard.
  reduce-shards  MCPX_HOST_SHARDS=3: the host reduce call on the groups [70, 0, 1, 65, 130], its
                 shards cut at chunk boundaries of the grouped table, against one shard."""

from __future__ import annotations

import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402


def generic() -> str | None:
    from tests.test_grouped_gpu import SIZES, check_solves, device_solves, grouped_inputs

    if os.environ.get("MCPX_GENERIC_KERNELS") != "1":
        return "MCPX_GENERIC_KERNELS=1 is not set"
    blocks, var = grouped_inputs(np.random.default_rng(1608), 0, 16, 8, SIZES)
    check_solves(*device_solves(0, 16, 8, blocks, var, SIZES, tol=1e-6, linear_solver="schur"))
    return None


def shards() -> str | None:
    from mcp_amd.batch import solve_batch, solve_batch_grouped, vjp_batch_grouped
    from tests.test_grouped_gpu import grouped_inputs, materialise
    from tests.test_shared_theta_gpu import TRACE, _same, assert_all_fields_equal

    if os.environ.get("MCPX_HOST_SHARDS") != "3" or os.environ.get("MCPX_HOST_CHUNK") != "1024":
        return "MCPX_HOST_SHARDS=3 / MCPX_HOST_CHUNK=1024 are not set"
    n, m, sizes = 16, 8, (900, 1, 1300, 0, 799)  # shard cuts at 1,000 and 2,000, chunk cuts inside groups
    rng = np.random.default_rng(3000)
    blocks, var = grouped_inputs(rng, 0, n, m, sizes)
    x0 = rng.standard_normal((sum(sizes), n))

    def run(ls):
        r = solve_batch_grouped(0, n, m, blocks, var, sizes, tol=1e-6, linear_solver=ls, trace_len=TRACE, x0=x0)
        return r, vjp_batch_grouped(0, n, m, blocks, r["x"], r["y"], r["s"], sizes, 2.0 * r["x"], 2.0 * r["y"])

    sharded = {ls: run(ls) for ls in ("schur", "reduced")}
    del os.environ["MCPX_HOST_SHARDS"]  # read at every call: the same calls as one shard
    for ls, (r, (dv, st)) in sharded.items():
        r1, (dv1, st1) = run(ls)
        assert_all_fields_equal(r, r1)
        assert_all_fields_equal(r, solve_batch(0, n, m, materialise(blocks, var, sizes, n + m), tol=1e-6,
                                               linear_solver=ls, trace_len=TRACE, x0=x0))
        if not (_same(dv, dv1) and _same(st, st1) and (st == 0).any()):
            return "the sharded pullback differs from one shard"
    return None


def reduce_shards() -> str | None:
    from mcp_amd.batch import solve_batch_grouped, vjp_batch_grouped_reduce
    from tests.helpers.shared_reduce_chain import bits_equal
    from tests.test_grouped_gpu import SIZES, grouped_inputs
    from tests.test_shared_theta_gpu import _same

    if os.environ.get("MCPX_HOST_SHARDS") != "3":
        return "MCPX_HOST_SHARDS=3 is not set"
    n, m = 16, 8
    rng = np.random.default_rng(1609)
    blocks, var = grouped_inputs(rng, 0, n, m, SIZES)
    skip = (rng.uniform(size=sum(SIZES)) < 0.1).astype(np.uint8)

    def run():
        r = solve_batch_grouped(0, n, m, blocks, var, SIZES, tol=1e-6, linear_solver="schur")
        return vjp_batch_grouped_reduce(0, n, m, blocks, r["x"], r["y"], r["s"], SIZES, 2.0 * r["x"], 2.0 * r["y"],
                                        skip=skip)

    sharded = run()  # 8 chunks: shards [0, 3), [3, 6), [6, 8) — cut at instances 71 and 200, the second inside a group
    del os.environ["MCPX_HOST_SHARDS"]
    single = run()
    if not (single[3] == 0).all() or int(single[1].sum()) != sum(SIZES) - int(skip.sum()) or not single[0].any():
        return "singular instances, or an empty sum"
    if not (bits_equal(sharded[0], single[0]) and np.array_equal(sharded[1], single[1])
            and _same(sharded[2], single[2]) and _same(sharded[3], single[3])):
        return "the sharded call differs from one shard"
    return None


def main() -> int:
    mode = sys.argv[1] if len(sys.argv) > 1 else ""
    fn = {"generic": generic, "shards": shards, "reduce-shards": reduce_shards}.get(mode)
    if fn is None:
        print(f"grouped-probe: unknown mode {mode!r}")
        return 2
    err = fn()
    if err:
        print(f"grouped-{mode}: {err}")
        return 1
    print(f"grouped-{mode}: OK")
    return 0


if __name__ == "__main__":
    sys.exit(main())

"""Child process of tests/test_shared_sens_gpu.py: the split host sensitivity calls with
MCPX_HOST_SHARDS=3 (set by the parent) over a ragged batch of 67 against the same calls as one
shard, bit for bit.  Prints "shared-sens-shards: OK" and exits 0 when they agree."""

from __future__ import annotations

import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402


def main() -> int:
    from mcp_amd.batch import jvp_batch_shared, solve_batch_shared, vjp_batch_shared
    from tests.test_shared_theta_gpu import _same, shared_qp

    if os.environ.get("MCPX_HOST_SHARDS") != "3":
        print("shared-sens-shards: MCPX_HOST_SHARDS=3 is not set")
        return 2
    n, m, B, K = 16, 8, 67, 13
    rng = np.random.default_rng(100 * n + m)
    shared, var = shared_qp(rng, n, m, B)
    gx, gy, gs = rng.standard_normal((B, n)), rng.standard_normal((B, m)), rng.standard_normal((B, m))
    vdot = rng.standard_normal((B, K, n + m))

    def run():
        r = solve_batch_shared(0, n, m, shared, var, tol=1e-6, linear_solver="schur")
        dv, st = vjp_batch_shared(0, n, m, shared, r["x"], r["y"], r["s"], gx, gy, gs)
        zd, jst = jvp_batch_shared(0, n, m, shared, r["x"], r["y"], r["s"], vdot)
        return r["x"], dv, st, zd, jst

    sharded = run()
    del os.environ["MCPX_HOST_SHARDS"]  # read at every call: the same calls as one shard
    single = run()
    if not (sharded[2] == 0).all():
        print("shared-sens-shards: singular instances")
        return 1
    for a, b in zip(sharded, single):
        if not _same(a, b):
            print("shared-sens-shards: the sharded call differs from one shard")
            return 1
    print("shared-sens-shards: OK")
    return 0


if __name__ == "__main__":
    sys.exit(main())

"""Child process of tests/test_shared_reduce_gpu.py: mcpx_vjp_batch_shared_reduce with
MCPX_HOST_SHARDS=3 (set by the parent) over B = 515 — at least three chunks of MCPX_REDUCE_CHUNK, the
shards cut at its multiples and the last one ragged — against the same call as one shard, bit for bit.  Prints
"shared-reduce-shards: OK" and exits 0 when they agree."""

from __future__ import annotations

import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402


def main() -> int:
    from mcp_amd.batch import solve_batch_shared, vjp_batch_shared_reduce
    from tests.helpers.shared_reduce_chain import bits_equal
    from tests.test_shared_theta_gpu import _same, shared_qp

    if os.environ.get("MCPX_HOST_SHARDS") != "3":
        print("shared-reduce-shards: MCPX_HOST_SHARDS=3 is not set")
        return 2
    n, m, B = 16, 8, 515
    rng = np.random.default_rng(100 * n + m)
    shared, var = shared_qp(rng, n, m, B)
    skip = (rng.uniform(size=B) < 0.1).astype(np.uint8)

    def run():
        r = solve_batch_shared(0, n, m, shared, var, tol=1e-6, linear_solver="schur")
        return vjp_batch_shared_reduce(0, n, m, shared, r["x"], r["y"], r["s"], 2.0 * r["x"], 2.0 * r["y"], skip=skip)

    sharded = run()
    del os.environ["MCPX_HOST_SHARDS"]  # read at every call: the same call as one shard
    single = run()
    if not (single[3] == 0).all() or single[1] != B - int(skip.sum()) or not single[0].any():
        print("shared-reduce-shards: singular instances, or an empty sum")
        return 1
    if not (bits_equal(sharded[0], single[0]) and sharded[1] == single[1] and _same(sharded[2], single[2])
            and _same(sharded[3], single[3])):
        print("shared-reduce-shards: the sharded call differs from one shard")
        return 1
    print("shared-reduce-shards: OK")
    return 0


if __name__ == "__main__":
    sys.exit(main())

"""Child process of tests/test_shared_tangent_gpu.py: the host calls mcpx_jvp_batch_shared_dot (with
and without a var_dot) and mcpx_cond_batch_shared with MCPX_HOST_SHARDS=3 and MCPX_HOST_CHUNK=1024
(set by the parent) over a ragged batch of 67 against the same calls as one shard and against the
device entry, bit for bit.  Prints "shared-tangent-shards: OK" and exits 0 when they agree."""

from __future__ import annotations

import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402


def main() -> int:
    import torch

    from mcp_amd.batch import cond_batch_shared, jvp_batch_shared, jvp_batch_shared_device, solve_batch_shared
    from tests.test_shared_theta_gpu import _same, shared_qp

    if os.environ.get("MCPX_HOST_SHARDS") != "3" or os.environ.get("MCPX_HOST_CHUNK") != "1024":
        print("shared-tangent-shards: MCPX_HOST_SHARDS=3 / MCPX_HOST_CHUNK=1024 are not set")
        return 2
    n, m, B, K = 16, 8, 67, 9
    rng = np.random.default_rng(100 * n + m)
    shared, var = shared_qp(rng, n, m, B)
    sdot, vdot = rng.standard_normal((K, shared.size)), rng.standard_normal((B, K, n + m))

    def run():
        r = solve_batch_shared(0, n, m, shared, var, tol=1e-6, linear_solver="schur")
        zd, st = jvp_batch_shared(0, n, m, shared, r["x"], r["y"], r["s"], vdot, shared_dot=sdot)
        zd0, st0 = jvp_batch_shared(0, n, m, shared, r["x"], r["y"], r["s"], None, shared_dot=sdot)
        rc, cst = cond_batch_shared(0, n, m, shared, r["x"], r["y"], r["s"])
        return r["x"], r["y"], r["s"], zd, st, zd0, st0, rc, cst

    sharded = run()
    del os.environ["MCPX_HOST_SHARDS"]  # read at every call: the same calls as one shard
    single = run()
    if not (sharded[4] == 0).all():
        print("shared-tangent-shards: singular instances")
        return 1
    for a, b in zip(sharded, single):
        if not _same(a, b):
            print("shared-tangent-shards: the sharded call differs from one shard")
            return 1
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")
    dzd, dst = jvp_batch_shared_device(0, n, m, T(shared), T(sharded[0]), T(sharded[1]), T(sharded[2]), T(vdot),
                                       shared_dot=T(sdot))
    torch.cuda.synchronize()
    if not (_same(dzd.cpu().numpy(), sharded[3]) and _same(dst.cpu().numpy(), sharded[4])):
        print("shared-tangent-shards: the sharded host call differs from the device call")
        return 1
    print("shared-tangent-shards: OK")
    return 0


if __name__ == "__main__":
    sys.exit(main())

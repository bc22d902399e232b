"""Child process of tests/test_shared_theta_gpu.py: the (32, 16) shared-matrix SCHUR solve with
the environment of its parent (MCPX_GENERIC_KERNELS=1: the runtime-(n, m) kernels) against the
full-θ call on the materialised θ′, every output field bit for bit.  Prints
"shared-generic: OK" and exits 0 when they agree."""

from __future__ import annotations

import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402


def main() -> int:
    from tests.test_shared_theta_gpu import assert_all_fields_equal, device_pair, shared_qp

    if os.environ.get("MCPX_GENERIC_KERNELS") != "1":
        print("shared-generic: MCPX_GENERIC_KERNELS=1 is not set")
        return 2
    shared, var = shared_qp(np.random.default_rng(3217), 32, 16, 257)
    got, ref, _ = device_pair(0, 32, 16, shared, var, tol=1e-6, linear_solver="schur")
    assert_all_fields_equal(got, ref)
    print("shared-generic: OK")
    return 0


if __name__ == "__main__":
    sys.exit(main())

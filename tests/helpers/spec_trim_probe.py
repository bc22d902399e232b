"""Child process of tests/test_spec_trim_gpu.py: its comparisons against the oracle with the
environment of its parent (MCPX_GENERIC_KERNELS=1: the runtime-(n, m) kernels), every size and
tol.  Prints "spec-trim-generic: OK" and exits 0 when every field agrees."""

from __future__ import annotations

import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main() -> int:
    from oracle import coracle
    from tests.test_spec_trim_gpu import SIZES, TOLS, gpu_compare

    if os.environ.get("MCPX_GENERIC_KERNELS") != "1":
        print("spec-trim-generic: MCPX_GENERIC_KERNELS=1 is not set")
        return 2
    coracle.build()
    for n, m in SIZES:
        for tol in TOLS:
            gpu_compare(coracle, n, m, tol)
            print(f"spec-trim-generic: ({n}, {m}) tol={tol:g} agrees", flush=True)
    print("spec-trim-generic: OK")
    return 0


if __name__ == "__main__":
    sys.exit(main())

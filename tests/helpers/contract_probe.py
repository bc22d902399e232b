"""Child process of tests/test_buffer_contract_gpu.py::test_library_blocks_under_padding, run
with MCPX_POISON=1 (set by the parent; read when the library's block cache starts): every block
the library allocates for itself is NaN-filled up to its requested size with a canary behind it.

Runs the host-entry calls of the stride check (θ at stride p + pad, NaN padding) and prints one
JSON line per call: {"call", "differ": output fields that differ from the oracle on the packed
θ, "canary": mcpx_debug_canary_violations() after the call}."""

from __future__ import annotations

import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main() -> int:
    if os.environ.get("MCPX_POISON") != "1":
        print("contract-probe: MCPX_POISON=1 is not set")
        return 2
    from mcp_amd._lib import lib
    from oracle import coracle
    from tests.helpers.contract_calls import host_stride_calls

    coracle.build()
    L = lib()
    for label, differ in host_stride_calls(coracle):
        print(json.dumps({"call": label, "differ": differ, "canary": int(L.mcpx_debug_canary_violations())}),
              flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())

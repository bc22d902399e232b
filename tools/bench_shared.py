"""Shared-matrix batches at the C3 shape (n = 32, m = 16, SCHUR), B = 65,536 on one GPU: the
split call (mcpx_solve_batch_shared*: one [vec(M); vec(A)] block, [b; ϕ] per instance) against
the full-θ call on the materialised copy of the same inputs.

    python tools/bench_shared.py [--batch B] [--steps K] [--full-only]

Inputs: M and A of instance 0 of qp_benchmark.generate_random_parameter (seed 1), b and ϕ of
every instance.  Prints ONE JSON line: for each call the device-resident rate (device tensors,
hipEvent time around the launch) and the host end-to-end rate (host arrays in and out through
mcpx_solve_batch*, page-locked inputs, reused result buffers, wall clock), the bytes each sends
over the host link per call, the cost of the θ′ expansion path (`expand`: the REDUCED solver's
split call — expansion plus the full-θ kernels slice by slice — against its full-θ call), and
the parity of the two calls on every output field.  The expansion kernel's own time, and so its
bandwidth over `expand.bytes`, is read from a kernel trace of this script (theta_expand_kernel:
the slices of one call add up to one pass over `bytes`).  1 warm-up, then the
median of `--steps` (≥ 5) timed steps.  `--full-only` measures the full-θ
call alone and needs nothing of the split entry points: it runs on a build without them.
"""

from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from mcp_amd import batch as mb  # noqa: E402
from mcp_amd.qp_benchmark import generate_random_parameter  # noqa: E402

N, M = 32, 16
KW = dict(tol=1e-6, linear_solver="schur")
FIELDS = ("x", "y", "s", "kkt_error", "eps", "outer_iters", "status", "newton_iters", "active_mask", "alpha_trace",
          "fail_reason")
TRACE = 32


def same(a, b) -> bool:
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype.kind == "f":
        return a.shape == b.shape and bool(np.all((a == b) | (np.isnan(a) & np.isnan(b))))
    return a.shape == b.shape and bool(np.array_equal(a, b))


def median_ms(fn, steps: int) -> float:
    fn()  # warm-up
    t = [fn() for _ in range(steps)]
    return float(np.median(t))


def device_ms(launch, steps: int) -> float:
    import torch

    def once():
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        launch()
        b.record()
        b.synchronize()
        return a.elapsed_time(b)

    return median_ms(once, steps)


def host_ms(call, steps: int) -> float:
    def once():
        t = time.perf_counter()
        call()
        return (time.perf_counter() - t) * 1e3

    return median_ms(once, steps)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--full-only", action="store_true")
    a = ap.parse_args()
    if a.steps < 5:
        ap.error("--steps must be at least 5 (BASELINE.md §Timing)")
    import torch

    B = a.batch
    D = N * N + M * N
    theta = generate_random_parameter(np.random.default_rng(1), N, M, 0.0, batch=B)
    shared = theta[0, :D].copy()
    var = np.ascontiguousarray(theta[:, D:])
    theta[:, :D] = shared  # the materialised copy of the same inputs
    dev = torch.device("cuda", 0)
    rate = lambda ms: B / (ms * 1e-3)
    rec = {"bench": "shared_theta", "n": N, "m": M, "batch": B, "steps": a.steps, "solver": "schur",
           "device": torch.cuda.get_device_name(0)}
    out_bytes = B * (8 * (N + 2 * M + 2) + 4 * 3 + 8 + 1)  # results back over the link, both calls alike

    # ---- full θ -----------------------------------------------------------------
    th_d = torch.from_numpy(theta).to(dev)
    out_d = mb.alloc_device_outputs(B, N, M, dev, TRACE)
    full_dev = device_ms(lambda: mb.solve_batch_device(0, N, M, th_d, out_d, **KW), a.steps)
    ref_d = {k: v.cpu().numpy() for k, v in out_d.items()}
    out_h = mb.alloc_host_outputs(B, N, M, TRACE)
    with mb.pinned(theta):
        full_host = host_ms(lambda: mb.solve_batch(0, N, M, theta, num_devices=1, trace_len=TRACE, out=out_h, **KW),
                            a.steps)
    ref_h = {k: np.array(v) for k, v in out_h.items()}
    rec["full"] = {"device_solves_per_s": rate(full_dev), "device_ms": full_dev, "host_solves_per_s": rate(full_host),
                   "host_ms": full_host, "h2d_bytes": int(theta.nbytes), "d2h_bytes": int(out_bytes)}
    rec["full_device_equals_host"] = all(same(ref_d[k].view(ref_h[k].dtype) if k == "active_mask" else ref_d[k],
                                              ref_h[k]) for k in FIELDS)
    if a.full_only:
        print(json.dumps(rec), flush=True)
        return 0

    # ---- split -------------------------------------------------------------------
    del th_d
    sh_d, var_d = torch.from_numpy(shared).to(dev), torch.from_numpy(var).to(dev)
    out_s = mb.alloc_device_outputs(B, N, M, dev, TRACE)
    split_dev = device_ms(lambda: mb.solve_batch_shared_device(0, N, M, sh_d, var_d, out_s, **KW), a.steps)
    got_d = {k: v.cpu().numpy() for k, v in out_s.items()}
    out_hs = mb.alloc_host_outputs(B, N, M, TRACE)
    with mb.pinned(var):
        split_host = host_ms(lambda: mb.solve_batch_shared(0, N, M, shared, var, num_devices=1, trace_len=TRACE,
                                                           out=out_hs, **KW), a.steps)
    rec["split"] = {"device_solves_per_s": rate(split_dev), "device_ms": split_dev,
                    "host_solves_per_s": rate(split_host), "host_ms": split_host,
                    "h2d_bytes": int(shared.nbytes + var.nbytes), "d2h_bytes": int(out_bytes)}
    rec["h2d_ratio"] = theta.nbytes / (shared.nbytes + var.nbytes)
    rec["device_split_over_full"] = full_dev / split_dev
    rec["host_split_over_full"] = full_host / split_host
    parity = {k: same(got_d[k], ref_d[k]) and same(out_hs[k], ref_h[k]) for k in FIELDS}
    rec["parity"] = all(parity.values())
    if not rec["parity"]:
        rec["parity_failed"] = sorted(k for k, v in parity.items() if not v)

    # ---- the expansion kernel ----------------------------------------------------
    # REDUCED has no in-kernel shared read: its split call is the expansion of every slice plus
    # the full-θ kernels on that slice.  The difference of the two device times is what the path
    # costs: the expansion kernels and the solve running as one launch per slice instead of one
    # over the batch.  `bytes`: the θ′ the expansion writes plus the var block it reads (the
    # shared block is read from L2).
    kr = dict(tol=1e-6, linear_solver="reduced")
    th_d = torch.from_numpy(theta).to(dev)
    red_full = device_ms(lambda: mb.solve_batch_device(0, N, M, th_d, out_d, **kr), a.steps)
    ref_r = {k: v.cpu().numpy() for k, v in out_d.items()}
    red_split = device_ms(lambda: mb.solve_batch_shared_device(0, N, M, sh_d, var_d, out_s, **kr), a.steps)
    got_r = {k: v.cpu().numpy() for k, v in out_s.items()}
    moved = theta.nbytes + var.nbytes
    rec["expand"] = {"reduced_full_ms": red_full, "reduced_split_ms": red_split, "bytes": int(moved),
                     "parity": all(same(got_r[k], ref_r[k]) for k in FIELDS)}
    rec["expand"]["split_minus_full_ms"] = red_split - red_full
    print(json.dumps(rec), flush=True)
    return 0 if rec["parity"] and rec["expand"]["parity"] else 1


if __name__ == "__main__":
    sys.exit(main())

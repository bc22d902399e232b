"""Tangents of shared-matrix batches along a direction of the shared block at the C3 shape
(n = 32, m = 16), K = 8 partials, on one GPU: mcpx_jvp_batch_shared_dot* (one [K × shared_dim]
block of matrix tangents, [B × K × (n + m)] per instance) against the route a caller had before it,
mcpx_jvp_batch* on the materialised θ′ [B × p] and θ̇ [B × K × p] of the same inputs.

    python tools/bench_shared_tangent.py [--batch B] [--host-batch B] [--steps K] [--full-only]

Inputs: M and A of instance 0 of qp_benchmark.generate_random_parameter (seed 1), b and ϕ of every
instance, the iterate of the GPU solve (tol 1e-6), seeded normal tangents.
Prints ONE JSON line:
  device  the tangent call alone on device tensors (hipEvent time around the launch), the bytes
          of tangents the caller allocates;
  host    the call on host arrays (page-locked inputs, reused result buffers, wall clock) and the
          bytes over the host link both ways, by count;
  parity  zdot and status of the new calls equal to the full-θ calls' on these inputs.
1 warm-up, then the median of `--steps` (default 7) timed steps.  `--full-only` measures the
full-θ route alone and needs none of the new entry points: it runs on a build without them.
"""

from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from mcp_amd import _abi  # noqa: E402
from mcp_amd import batch as mb  # noqa: E402
from mcp_amd._lib import check, lib  # noqa: E402
from mcp_amd.qp_benchmark import generate_random_parameter  # noqa: E402

N, M, K = 32, 16, 8
D, DV, P, NZ = N * N + M * N, N + M, N * N + M * N + M + N, N + 2 * M
KW = dict(tol=1e-6, linear_solver="schur")


def same(a, b) -> bool:
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype.kind == "f":
        return a.shape == b.shape and bool(np.all((a == b) | (np.isnan(a) & np.isnan(b))))
    return a.shape == b.shape and bool(np.array_equal(a, b))


def median_ms(fn, steps: int) -> float:
    fn()  # warm-up
    return float(np.median([fn() for _ in range(steps)]))


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


def inputs(B: int):
    """(θ′ materialised (B, P), shared (D,), sdot (K, D), vdot (B, K, DV))."""
    theta = generate_random_parameter(np.random.default_rng(1), N, M, 0.0, batch=B)
    shared = theta[0, :D].copy()
    theta[:, :D] = shared
    rng = np.random.default_rng(2)
    return theta, shared, rng.standard_normal((K, D)), rng.standard_normal((B, K, DV))


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16384)
    ap.add_argument("--host-batch", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--full-only", action="store_true")
    a = ap.parse_args()
    import torch

    dev = torch.device("cuda", 0)
    T = lambda v: torch.from_numpy(v).to(dev)
    split = not a.full_only
    rate = lambda n, ms: n / (ms * 1e-3)
    rec = {"bench": "shared_tangent", "n": N, "m": M, "partials": K, "batch": a.batch, "host_batch": a.host_batch,
           "steps": a.steps, "gpu": torch.cuda.get_device_name(0), "full_only": a.full_only}
    parity = {}

    # ---- 1. the tangent call alone, device-resident --------------------------------------
    B = a.batch
    theta, shared, sdot, vdot = inputs(B)
    th_d, sd_d, vd_d = T(theta), T(sdot), T(vdot)
    sol = mb.solve_batch_device(0, N, M, th_d, **KW)
    x, y, s = sol["x"], sol["y"], sol["s"]
    td_d = torch.cat([sd_d.expand(B, K, D), vd_d], 2).contiguous()  # θ̇ (B, K, P): what the full route needs
    zd = torch.empty(B, K, NZ, dtype=torch.float64, device=dev)
    st = torch.empty(B, dtype=torch.int32, device=dev)
    ms = device_ms(lambda: mb.jvp_batch_device(0, N, M, th_d, x, y, s, td_d, zdot=zd, status=st), a.steps)
    rec["device"] = {"full": {"ms": ms, "jvps_per_s": rate(B, ms),
                              "tangent_bytes": int(td_d.numel() * 8), "theta_bytes": int(theta.nbytes)}}
    if split:
        sh_d = T(shared)
        zs = torch.empty(B, K, NZ, dtype=torch.float64, device=dev)
        ss = torch.empty(B, dtype=torch.int32, device=dev)
        ms_s = device_ms(lambda: mb.jvp_batch_shared_device(0, N, M, sh_d, x, y, s, vd_d, zdot=zs, status=ss,
                                                            shared_dot=sd_d), a.steps)
        rec["device"]["split"] = {"ms": ms_s, "jvps_per_s": rate(B, ms_s),
                                  "tangent_bytes": int((sdot.size + vdot.size) * 8), "theta_bytes": int(shared.nbytes)}
        rec["device"]["split_over_full"] = ms / ms_s
        parity["device.zdot"] = same(zs.cpu().numpy(), zd.cpu().numpy())
        parity["device.status"] = same(ss.cpu().numpy(), st.cpu().numpy())
        rec["device"]["status_ok"] = int((ss == 0).sum())
    del th_d, td_d, vd_d, zd

    # ---- 2. end to end from host arrays ------------------------------------------------------
    B = a.host_batch
    theta, shared, sdot, vdot = inputs(B)
    sol = mb.solve_batch_device(0, N, M, T(theta), **KW)
    xh, yh, sh_ = (np.ascontiguousarray(sol[k].cpu().numpy()) for k in ("x", "y", "s"))
    tdot = np.ascontiguousarray(np.concatenate([np.broadcast_to(sdot, (B, K, D)), vdot], 2))
    zd_h, st_h = np.zeros((B, K, NZ)), np.zeros(B, np.int32)  # reused, first-touched here
    ptr = lambda v: v.ctypes.data
    L = lib()
    desc = _abi.Desc(0, N, M, 0, B, P)
    pins = [mb.pinned(v) for v in (theta, xh, yh, sh_, tdot, vdot)]
    for p_ in pins:
        p_.__enter__()
    ms = host_ms(lambda: check(L.mcpx_jvp_batch(C.byref(desc), ptr(theta), ptr(xh), ptr(yh), ptr(sh_), K, ptr(tdot), 1,
                                                ptr(zd_h), ptr(st_h))), a.steps)
    it = sum(v.nbytes for v in (xh, yh, sh_))
    rec["host"] = {"full": {"ms": ms, "jvps_per_s": rate(B, ms), "h2d_bytes": int(theta.nbytes + tdot.nbytes + it),
                            "d2h_bytes": int(zd_h.nbytes + st_h.nbytes)}}
    if split:
        zs_h, ss_h = np.zeros((B, K, NZ)), np.zeros(B, np.int32)
        dsc = _abi.Desc(0, N, M, 0, B, DV)
        ms_s = host_ms(lambda: check(L.mcpx_jvp_batch_shared_dot(C.byref(dsc), ptr(shared), ptr(xh), ptr(yh), ptr(sh_),
                                                                 K, ptr(sdot), ptr(vdot), 1, ptr(zs_h), ptr(ss_h))),
                       a.steps)
        rec["host"]["split"] = {"ms": ms_s, "jvps_per_s": rate(B, ms_s),
                                "h2d_bytes": int(shared.nbytes + sdot.nbytes + vdot.nbytes + it),
                                "d2h_bytes": int(zs_h.nbytes + ss_h.nbytes)}
        rec["host"]["split_over_full"] = ms / ms_s
        parity["host.zdot"] = same(zs_h, zd_h)
        parity["host.status"] = same(ss_h, st_h)
    for p_ in pins[::-1]:
        p_.__exit__(None, None, None)

    if split:
        rec["parity"] = all(parity.values())
        rec["parity_fields"] = len(parity)
        if not rec["parity"]:
            rec["parity_failed"] = sorted(k for k, v in parity.items() if not v)
    print(json.dumps(rec), flush=True)
    return 0 if (not split or rec["parity"]) else 1


if __name__ == "__main__":
    sys.exit(main())

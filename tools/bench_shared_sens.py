"""Sensitivities of shared-matrix batches at the C3 / C5 shape (n = 32, m = 16, SCHUR) on one
GPU: the split calls (mcpx_vjp_batch_shared*, mcpx_solve_vjp_batch_shared_device: one
[vec(M); vec(A)] block, [∂b; ∂ϕ] per instance) against the full-θ calls on the materialised copy
of the same inputs.

    python tools/bench_shared_sens.py [--batch B] [--fused-batches 4096,65536] [--steps K] [--full-only]

Inputs: M and A of instance 0 of qp_benchmark.generate_random_parameter (seed 1), b and ϕ of
every instance, the iterate of the GPU solve (tol 1e-6), the cotangent of f = Σx² + Σy².
Prints ONE JSON line:
  vjp    the pullback alone on device tensors (hipEvent time around the launch) and its bytes;
  fused  solve + pullback in one call (BASELINE C5) on device tensors, per batch size;
  host   the pullback on host arrays through mcpx_vjp_batch*, page-locked inputs, reused result
         buffers, wall clock, and the bytes over the host link both ways;
  parity every compared field of the split calls equal to the full-θ calls' (sliced).
1 warm-up, then the median of `--steps` (≥ 5) timed steps.  `--full-only`
measures the full-θ calls alone and needs nothing of the split entry points: it runs on a build
without them.
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

N, M = 32, 16
D, DV, P = N * N + M * N, N + M, N * N + M * N + M + N
KW = dict(tol=1e-6, linear_solver="schur")
CT = (2.0, 2.0, 0.0)  # f = Σx² + Σy² (test/runtests.jl:72-75)
SOLVE_FIELDS = ("x", "y", "s", "kkt_error", "eps", "outer_iters", "status", "newton_iters", "active_mask",
                "fail_reason")


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
    theta = generate_random_parameter(np.random.default_rng(1), N, M, 0.0, batch=B)
    shared = theta[0, :D].copy()
    var = np.ascontiguousarray(theta[:, D:])
    theta[:, :D] = shared  # the materialised copy of the same inputs
    return theta, shared, var


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--fused-batches", default="4096,65536")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--full-only", action="store_true")
    a = ap.parse_args()
    if a.steps < 5:
        ap.error("--steps must be at least 5 (BASELINE.md §Timing)")
    import torch

    dev = torch.device("cuda", 0)
    T = lambda v: torch.from_numpy(v).to(dev)
    B, split = a.batch, not a.full_only
    rate = lambda n, ms: n / (ms * 1e-3)
    rec = {"bench": "shared_sens", "n": N, "m": M, "batch": B, "steps": a.steps, "solver": "schur",
           "device": torch.cuda.get_device_name(0), "full_only": a.full_only}
    parity = {}

    # ---- 1. the pullback alone, device-resident -------------------------------------
    theta, shared, var = inputs(B)
    th_d = T(theta)
    sol = mb.solve_batch_device(0, N, M, th_d, **KW)
    x, y, s = sol["x"], sol["y"], sol["s"]
    gx, gy = 2.0 * x, 2.0 * y
    dth = torch.empty(B, P, dtype=torch.float64, device=dev)
    st = torch.empty(B, dtype=torch.int32, device=dev)
    ms = device_ms(lambda: mb.vjp_batch_device(0, N, M, th_d, x, y, s, gx, gy, None, dtheta=dth, status=st), a.steps)
    rec["vjp"] = {"full": {"ms": ms, "vjps_per_s": rate(B, ms), "read_bytes": int(theta.nbytes),
                           "write_bytes": int(B * P * 8)}}
    if split:
        sh_d = T(shared)
        dv = torch.empty(B, DV, dtype=torch.float64, device=dev)
        sv = torch.empty(B, dtype=torch.int32, device=dev)
        ms_s = device_ms(lambda: mb.vjp_batch_shared_device(0, N, M, sh_d, x, y, s, gx, gy, None, dvar=dv, status=sv),
                         a.steps)
        rec["vjp"]["split"] = {"ms": ms_s, "vjps_per_s": rate(B, ms_s), "read_bytes": int(shared.nbytes),
                               "write_bytes": int(B * DV * 8)}
        rec["vjp"]["split_over_full"] = ms / ms_s
        parity["vjp.dvar"] = same(dv.cpu().numpy(), dth[:, D:].cpu().numpy())
        parity["vjp.status"] = same(sv.cpu().numpy(), st.cpu().numpy())
        rec["vjp"]["status_ok"] = int((sv == 0).sum())

    # ---- 3. the pullback end to end from host arrays ----------------------------------
    xh, yh, sh_ = (np.ascontiguousarray(t.cpu().numpy()) for t in (x, y, s))
    gxh, gyh = 2.0 * xh, 2.0 * yh
    dth_h, st_h = np.zeros((B, P)), np.zeros(B, np.int32)  # reused, first-touched here
    ptr = lambda v: v.ctypes.data
    L = lib()
    desc = _abi.Desc(0, N, M, 0, B, P)
    pins = [mb.pinned(v) for v in (theta, xh, yh, sh_, gxh, gyh)]
    for p_ in pins:
        p_.__enter__()
    ms = host_ms(lambda: check(L.mcpx_vjp_batch(C.byref(desc), ptr(theta), ptr(xh), ptr(yh), ptr(sh_), ptr(gxh),
                                                ptr(gyh), None, 1, ptr(dth_h), ptr(st_h))), a.steps)
    sens_in = sum(v.nbytes for v in (xh, yh, sh_, gxh, gyh))
    rec["host"] = {"full": {"ms": ms, "vjps_per_s": rate(B, ms), "h2d_bytes": int(theta.nbytes + sens_in),
                            "d2h_bytes": int(dth_h.nbytes + st_h.nbytes)}}
    if split:
        dv_h, sv_h = np.zeros((B, DV)), np.zeros(B, np.int32)
        dsc = _abi.Desc(0, N, M, 0, B, DV)
        ms_s = host_ms(lambda: check(L.mcpx_vjp_batch_shared(C.byref(dsc), ptr(shared), ptr(xh), ptr(yh), ptr(sh_),
                                                             ptr(gxh), ptr(gyh), None, 1, ptr(dv_h), ptr(sv_h))),
                       a.steps)
        rec["host"]["split"] = {"ms": ms_s, "vjps_per_s": rate(B, ms_s), "h2d_bytes": int(shared.nbytes + sens_in),
                                "d2h_bytes": int(dv_h.nbytes + sv_h.nbytes)}
        rec["host"]["split_over_full"] = ms / ms_s
        parity["host.dvar"] = same(dv_h, dth_h[:, D:])
        parity["host.status"] = same(sv_h, st_h)
    for p_ in pins[::-1]:
        p_.__exit__(None, None, None)
    del th_d, dth

    # ---- 2. solve + pullback in one call (C5), device-resident -------------------------
    rec["fused"] = {}
    for Bf in (int(v) for v in a.fused_batches.split(",") if v):
        theta, shared, var = inputs(Bf)
        th_d = T(theta)
        out = mb.alloc_device_outputs(Bf, N, M, dev)
        dth = torch.empty(Bf, P, dtype=torch.float64, device=dev)
        st = torch.empty(Bf, dtype=torch.int32, device=dev)
        ms = device_ms(lambda: mb.solve_vjp_batch_device(0, N, M, th_d, out, ct=CT, dtheta=dth, status=st, **KW),
                       a.steps)
        r = {"full": {"ms": ms, "solve_vjps_per_s": rate(Bf, ms)}}
        if split:
            sh_d, var_d = T(shared), T(var)
            out_s = mb.alloc_device_outputs(Bf, N, M, dev)
            dv = torch.empty(Bf, DV, dtype=torch.float64, device=dev)
            sv = torch.empty(Bf, dtype=torch.int32, device=dev)
            ms_s = device_ms(lambda: mb.solve_vjp_batch_shared_device(0, N, M, sh_d, var_d, out_s, ct=CT, dvar=dv,
                                                                      status=sv, **KW), a.steps)
            r["split"] = {"ms": ms_s, "solve_vjps_per_s": rate(Bf, ms_s)}
            r["split_over_full"] = ms / ms_s
            for k in SOLVE_FIELDS:
                parity[f"fused{Bf}.{k}"] = same(out_s[k].cpu().numpy(), out[k].cpu().numpy())
            parity[f"fused{Bf}.dvar"] = same(dv.cpu().numpy(), dth[:, D:].cpu().numpy())
            parity[f"fused{Bf}.vjp_status"] = same(sv.cpu().numpy(), st.cpu().numpy())
        rec["fused"][str(Bf)] = r
        del th_d, dth

    if split:
        rec["parity"] = all(parity.values())
        rec["parity_fields"] = len(parity)
        if not rec["parity"]:
            rec["parity_failed"] = sorted(k for k, v in parity.items() if not v)
    print(json.dumps(rec), flush=True)
    return 0 if (not split or rec["parity"]) else 1


if __name__ == "__main__":
    sys.exit(main())

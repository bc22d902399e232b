"""The gradient of the shared matrix block of a shared-matrix batch at the C3 shape (n = 32,
m = 16) on one GPU: mcpx_vjp_batch_shared_reduce[_device] against the only route there is without
it — the full-θ pullback on the materialised θ′, then the sum of the head of every record.

    python tools/bench_shared_reduce.py [--batch B] [--steps K] [--full-only]

Inputs and method of tools/bench_shared_sens.py: M and A of instance 0 of
qp_benchmark.generate_random_parameter (seed 1), b and ϕ of every instance, the iterate of the
GPU solve (tol 1e-6), the cotangent of f = Σx² + Σy²; 1 warm-up, then the median of `--steps`
(≥ 5) timed steps.  Prints ONE JSON line:
  device  full: vjp_batch_device into a (B, p) buffer, then dtheta[:, :shared_dim].sum(0) in torch;
          reduce: vjp_batch_shared_reduce_device (dvar kept / dvar NULL); hipEvent time, and the
          bytes each route moves through HBM;
  host    the same two routes from host arrays (mcpx_vjp_batch + numpy sum against
          mcpx_vjp_batch_shared_reduce), page-locked inputs, wall clock;
  check   the reduce call's dshared against the summed full records (largest error in units of
          the rounding bound 2·(B + 2)·2⁻⁵³·Σ|terms|), device against host bits, `used`.
`--full-only` measures the full-θ route alone and needs nothing of the reduce entry points: it
runs on a build without them.
"""

from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_shared_sens import D, DV, KW, M, N, P, device_ms, host_ms, inputs  # noqa: E402
from mcp_amd import _abi  # noqa: E402
from mcp_amd import batch as mb  # noqa: E402
from mcp_amd._lib import check, lib  # noqa: E402


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--full-only", action="store_true")
    a = ap.parse_args()
    if a.steps < 5:
        ap.error("--steps must be at least 5 (BASELINE.md §Timing)")
    import torch

    dev = torch.device("cuda", 0)
    T = lambda v: torch.from_numpy(v).to(dev)
    B, new = a.batch, not a.full_only
    rate = lambda ms: B / (ms * 1e-3)
    rec = {"bench": "shared_reduce", "n": N, "m": M, "batch": B, "steps": a.steps, "solver": "schur",
           "gpu": torch.cuda.get_device_name(0), "full_only": a.full_only}

    theta, shared, var = inputs(B)
    th_d = T(theta)
    sol = mb.solve_batch_device(0, N, M, th_d, **KW)
    x, y, s = sol["x"], sol["y"], sol["s"]
    gx, gy = 2.0 * x, 2.0 * y
    state_bytes = int(sum(t.numel() for t in (x, y, s, gx, gy)) * 8)

    # ---- device-resident ------------------------------------------------------------------
    dth = torch.empty(B, P, dtype=torch.float64, device=dev)
    st = torch.empty(B, dtype=torch.int32, device=dev)
    full_sum = [None]

    def full_route():
        mb.vjp_batch_device(0, N, M, th_d, x, y, s, gx, gy, None, dtheta=dth, status=st)
        full_sum[0] = dth[:, :D].sum(0)

    ms = device_ms(full_route, a.steps)
    rec["device"] = {"full": {"ms": ms, "grads_per_s": rate(ms),
                              "hbm_bytes": int(theta.nbytes + state_bytes + B * P * 8 + B * D * 8)}}
    if new:
        sh_d = T(shared)
        dsh = torch.empty(D, dtype=torch.float64, device=dev)
        used = torch.empty(1, dtype=torch.int64, device=dev)
        dv = torch.empty(B, DV, dtype=torch.float64, device=dev)
        sv = torch.empty(B, dtype=torch.int32, device=dev)
        ms_r = device_ms(lambda: mb.vjp_batch_shared_reduce_device(0, N, M, sh_d, x, y, s, gx, gy, None, dshared=dsh,
                                                                   used=used, dvar=dv, status=sv), a.steps)
        dsh_n = torch.empty(D, dtype=torch.float64, device=dev)
        ms_n = device_ms(lambda: mb.vjp_batch_shared_reduce_device(0, N, M, sh_d, x, y, s, gx, gy, None, dshared=dsh_n,
                                                                   used=used, status=sv, want_dvar=False), a.steps)
        ms_v = device_ms(lambda: mb.vjp_batch_shared_device(0, N, M, sh_d, x, y, s, gx, gy, None, dvar=dv, status=sv),
                         a.steps)
        nch = (B + _abi.REDUCE_CHUNK - 1) // _abi.REDUCE_CHUNK
        rec["device"]["reduce"] = {"ms": ms_r, "grads_per_s": rate(ms_r), "ms_dvar_null": ms_n,
                                   "split_vjp_alone_ms": ms_v, "reduce_share_of_split_vjp": (ms_r - ms_v) / ms_v,
                                   "hbm_bytes": int(shared.nbytes + state_bytes + 2 * B * DV * 8 + B * (N + M) * 8
                                                    + 2 * nch * D * 8 + D * 8)}
        rec["device"]["reduce_over_full"] = ms / ms_r
        torch.cuda.synchronize()
        lam, xa, ya = dv.abs(), x.abs(), y.abs()
        mag = torch.cat([(lam[:, M:].T @ xa).T.reshape(-1),                       # |λx_i x_j|, column-major
                         ((lam[:, :M].T @ xa) + (lam[:, M:].T @ ya).T).T.reshape(-1)])  # |λy_k x_j| + |λx_j y_k|
        ok = (sv == 0)
        bound = 2.0 * (B + 2) * 2.0 ** -53 * mag
        err = (dsh - full_sum[0]).abs()
        rec["check"] = {"used": int(used), "status_ok": int(ok.sum()), "all_included": bool(ok.all()),
                        "max_err_over_bound": float((err / bound).max()),
                        "dvar_null_same_bits": bool(torch.equal(dsh.view(torch.int64), dsh_n.view(torch.int64)))}

    # ---- end to end from host arrays ------------------------------------------------------
    xh, yh, sh_ = (np.ascontiguousarray(t.cpu().numpy()) for t in (x, y, s))
    gxh, gyh = 2.0 * xh, 2.0 * yh
    dth_h, st_h = np.zeros((B, P)), np.zeros(B, np.int32)  # reused, first-touched here
    ptr = lambda v: v.ctypes.data
    L = lib()
    desc = _abi.Desc(0, N, M, 0, B, P)
    pins = [mb.pinned(v) for v in (theta, xh, yh, sh_, gxh, gyh)]
    for p_ in pins:
        p_.__enter__()
    host_sum = [None]

    def full_host():
        check(L.mcpx_vjp_batch(C.byref(desc), ptr(theta), ptr(xh), ptr(yh), ptr(sh_), ptr(gxh), ptr(gyh), None, 1,
                               ptr(dth_h), ptr(st_h)))
        host_sum[0] = dth_h[:, :D].sum(0)

    ms = host_ms(full_host, a.steps)
    sens_in = sum(v.nbytes for v in (xh, yh, sh_, gxh, gyh))
    rec["host"] = {"full": {"ms": ms, "grads_per_s": rate(ms), "h2d_bytes": int(theta.nbytes + sens_in),
                            "d2h_bytes": int(dth_h.nbytes + st_h.nbytes)}}
    if new:
        dsh_h, used_h = np.zeros(D), np.zeros(1, np.int64)
        dv_h, sv_h = np.zeros((B, DV)), np.zeros(B, np.int32)
        dsc = _abi.Desc(0, N, M, 0, B, DV)
        ms_r = host_ms(lambda: check(L.mcpx_vjp_batch_shared_reduce(
            C.byref(dsc), ptr(shared), ptr(xh), ptr(yh), ptr(sh_), ptr(gxh), ptr(gyh), None, None, 1, ptr(dsh_h),
            ptr(used_h), ptr(dv_h), ptr(sv_h))), a.steps)
        ms_n = host_ms(lambda: check(L.mcpx_vjp_batch_shared_reduce(
            C.byref(dsc), ptr(shared), ptr(xh), ptr(yh), ptr(sh_), ptr(gxh), ptr(gyh), None, None, 1, ptr(dsh_h),
            ptr(used_h), None, None)), a.steps)
        rec["host"]["reduce"] = {"ms": ms_r, "grads_per_s": rate(ms_r), "ms_dvar_null": ms_n,
                                 "h2d_bytes": int(shared.nbytes + sens_in),
                                 "d2h_bytes": int(dv_h.nbytes + sv_h.nbytes + nch * (D + 1) * 8)}
        rec["host"]["reduce_over_full"] = ms / ms_r
        rec["check"]["host_same_bits_as_device"] = bool(np.array_equal(dsh_h.view(np.uint64),
                                                                       dsh.cpu().numpy().view(np.uint64)))
        rec["check"]["host_used"] = int(used_h[0])
    for p_ in pins[::-1]:
        p_.__exit__(None, None, None)
    print(json.dumps(rec), flush=True)
    if not new:
        return 0
    c = rec["check"]
    good = (c["max_err_over_bound"] <= 1.0 and c["dvar_null_same_bits"] and c["host_same_bits_as_device"]
            and c["used"] == c["status_ok"] == c["host_used"])
    return 0 if good else 1


if __name__ == "__main__":
    sys.exit(main())

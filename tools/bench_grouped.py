"""Grouped shared-matrix batches at the C3 shape (n = 32, m = 16, SCHUR, tol 1e-6) on one GPU:
mcpx_solve_batch_grouped[_device] and mcpx_vjp_batch_grouped_reduce[_device] against the route there
is without them — G back-to-back shared calls, one per group, on one stream.

    python tools/bench_grouped.py [--batch B] [--groups G] [--steps K] [--loop-only]

Inputs: qp_benchmark.generate_random_parameter (seed 1); group g's M and A are those of instance
off[g] of the stream, b and ϕ are every instance's own; G equal groups of B / G.  The gradient runs
at the iterate of the GPU solve with the cotangent of f = Σx² + Σy².  1 warm-up, then the median of
`--steps` (≥ 5) timed steps.  Prints ONE JSON line:
  device  solve / reduce: `loop` (G solve_batch_shared_device / vjp_batch_shared_reduce_device calls
          on slices), `grouped` (one call), `single_block` (the shared call on the whole batch with
          group 0's block: a ceiling, another problem); hipEvent time, instances per second;
  host    the same routes from page-locked host arrays, wall clock;
  bytes   what the caller allocates for θ: grouped against the materialised full θ′;
  parity  the grouped outputs against the loop route's, bit for bit (solve fields, dvar, status,
          dshared, used), device and host.
`--loop-only` measures the loop route (and the ceiling) alone and needs none of the grouped entry
points: it runs on a build without them.
"""

from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_shared_sens import D, DV, KW, M, N, P, SOLVE_FIELDS, device_ms, host_ms, same  # noqa: E402
from mcp_amd import batch as mb  # noqa: E402
from mcp_amd.qp_benchmark import generate_random_parameter  # noqa: E402


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--groups", type=int, default=64)
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--loop-only", action="store_true")
    a = ap.parse_args()
    if a.steps < 5:
        ap.error("--steps must be at least 5 (BASELINE.md §Timing)")
    if a.batch % a.groups:
        ap.error("--batch must be a multiple of --groups")
    import torch

    dev = torch.device("cuda", 0)
    T = lambda v: torch.from_numpy(v).to(dev)
    B, G, new = a.batch, a.groups, not a.loop_only
    S = B // G
    sizes = [S] * G
    rate = lambda ms: B / (ms * 1e-3)
    rec = {"bench": "grouped", "n": N, "m": M, "batch": B, "groups": G, "steps": a.steps, "solver": "schur",
           "gpu": torch.cuda.get_device_name(0), "loop_only": a.loop_only,
           "bytes": {"grouped_theta": G * D * 8 + B * DV * 8, "full_theta": B * P * 8}}

    theta = generate_random_parameter(np.random.default_rng(1), N, M, 0.0, batch=B)
    blocks = np.ascontiguousarray(theta[::S, :D])  # instance off[g]'s M and A
    var = np.ascontiguousarray(theta[:, D:])
    del theta
    bl_d, var_d = T(blocks), T(var)
    spans = [(g * S, (g + 1) * S) for g in range(G)]

    # ---- device-resident solve ---------------------------------------------------------------
    out_l = mb.alloc_device_outputs(B, N, M, dev)
    views = [{k: (None if v is None else v[lo:hi]) for k, v in out_l.items()} for lo, hi in spans]
    var_v = [var_d[lo:hi] for lo, hi in spans]

    def solve_loop():
        for g in range(G):
            mb.solve_batch_shared_device(0, N, M, bl_d[g], var_v[g], views[g], **KW)

    ms_l = device_ms(solve_loop, a.steps)
    out_c = mb.alloc_device_outputs(B, N, M, dev)
    ms_c = device_ms(lambda: mb.solve_batch_shared_device(0, N, M, bl_d[0], var_d, out_c, **KW), a.steps)
    rec["device"] = {"solve": {"loop": {"ms": ms_l, "solves_per_s": rate(ms_l)},
                               "single_block": {"ms": ms_c, "solves_per_s": rate(ms_c)}}}
    parity = {}
    if new:
        out_g = mb.alloc_device_outputs(B, N, M, dev)
        ms_g = device_ms(lambda: mb.solve_batch_grouped_device(0, N, M, bl_d, var_d, sizes, out_g, **KW), a.steps)
        rec["device"]["solve"]["grouped"] = {"ms": ms_g, "solves_per_s": rate(ms_g)}
        rec["device"]["solve"]["grouped_over_loop"] = ms_l / ms_g
        torch.cuda.synchronize()
        parity["device_solve"] = all(same(out_g[k].cpu().numpy(), out_l[k].cpu().numpy()) for k in SOLVE_FIELDS)

    # ---- device-resident gradient of the blocks --------------------------------------------------
    x, y, s = out_l["x"], out_l["y"], out_l["s"]
    gx, gy = 2.0 * x, 2.0 * y
    dsh_l = torch.empty(G, D, dtype=torch.float64, device=dev)
    used_l = torch.empty(G, dtype=torch.int64, device=dev)
    dv_l = torch.empty(B, DV, dtype=torch.float64, device=dev)
    st_l = torch.empty(B, dtype=torch.int32, device=dev)
    sl = lambda t: [t[lo:hi] for lo, hi in spans]
    xs, ys, ss, gxs, gys, dvs, sts = (sl(t) for t in (x, y, s, gx, gy, dv_l, st_l))
    useds = [used_l[g:g + 1] for g in range(G)]

    def reduce_loop():
        for g in range(G):
            mb.vjp_batch_shared_reduce_device(0, N, M, bl_d[g], xs[g], ys[g], ss[g], gxs[g], gys[g], None,
                                              dshared=dsh_l[g], used=useds[g], dvar=dvs[g], status=sts[g])

    ms_l = device_ms(reduce_loop, a.steps)
    dsh_c = torch.empty(D, dtype=torch.float64, device=dev)
    used_c = torch.empty(1, dtype=torch.int64, device=dev)
    dv_c, st_c = torch.empty_like(dv_l), torch.empty_like(st_l)
    ms_c = device_ms(lambda: mb.vjp_batch_shared_reduce_device(0, N, M, bl_d[0], x, y, s, gx, gy, None, dshared=dsh_c,
                                                               used=used_c, dvar=dv_c, status=st_c), a.steps)
    rec["device"]["reduce"] = {"loop": {"ms": ms_l, "grads_per_s": rate(ms_l)},
                               "single_block": {"ms": ms_c, "grads_per_s": rate(ms_c)}}
    if new:
        dsh_g, used_g = torch.empty_like(dsh_l), torch.empty_like(used_l)
        dv_g, st_g = torch.empty_like(dv_l), torch.empty_like(st_l)
        ms_g = device_ms(lambda: mb.vjp_batch_grouped_reduce_device(0, N, M, bl_d, x, y, s, sizes, gx, gy, None,
                                                                    dshared=dsh_g, used=used_g, dvar=dv_g,
                                                                    status=st_g), a.steps)
        rec["device"]["reduce"]["grouped"] = {"ms": ms_g, "grads_per_s": rate(ms_g)}
        rec["device"]["reduce"]["grouped_over_loop"] = ms_l / ms_g
        torch.cuda.synchronize()
        bits = lambda t: t.view(torch.int64)
        parity["device_reduce"] = bool(torch.equal(bits(dsh_g), bits(dsh_l)) and torch.equal(used_g, used_l)
                                       and same(dv_g.cpu().numpy(), dv_l.cpu().numpy()) and torch.equal(st_g, st_l))
        parity["used"] = int(used_g.sum())

    # ---- end to end from host arrays -------------------------------------------------------------
    xh, yh, sh = (np.ascontiguousarray(t.cpu().numpy()) for t in (x, y, s))
    gxh, gyh = 2.0 * xh, 2.0 * yh
    pins = [mb.pinned(v) for v in (var, xh, yh, sh, gxh, gyh)]
    for p_ in pins:
        p_.__enter__()
    ho_l = mb.alloc_host_outputs(B, N, M)
    hviews = [{k: (None if v is None else v[lo:hi]) for k, v in ho_l.items()} for lo, hi in spans]

    def host_solve_loop():
        for g, (lo, hi) in enumerate(spans):
            mb.solve_batch_shared(0, N, M, blocks[g], var[lo:hi], out=hviews[g], **KW)

    res_l = [None] * G

    def host_reduce_loop():
        for g, (lo, hi) in enumerate(spans):
            res_l[g] = mb.vjp_batch_shared_reduce(0, N, M, blocks[g], xh[lo:hi], yh[lo:hi], sh[lo:hi], gxh[lo:hi],
                                                  gyh[lo:hi])

    ms_sl, ms_rl = host_ms(host_solve_loop, a.steps), host_ms(host_reduce_loop, a.steps)
    rec["host"] = {"solve": {"loop": {"ms": ms_sl, "solves_per_s": rate(ms_sl)}},
                   "reduce": {"loop": {"ms": ms_rl, "grads_per_s": rate(ms_rl)}}}
    if new:
        ho_g = mb.alloc_host_outputs(B, N, M)
        res_g = [None]

        def host_reduce_grouped():
            res_g[0] = mb.vjp_batch_grouped_reduce(0, N, M, blocks, xh, yh, sh, sizes, gxh, gyh)

        ms_sg = host_ms(lambda: mb.solve_batch_grouped(0, N, M, blocks, var, sizes, out=ho_g, **KW), a.steps)
        ms_rg = host_ms(host_reduce_grouped, a.steps)
        rec["host"]["solve"]["grouped"] = {"ms": ms_sg, "solves_per_s": rate(ms_sg)}
        rec["host"]["solve"]["grouped_over_loop"] = ms_sl / ms_sg
        rec["host"]["reduce"]["grouped"] = {"ms": ms_rg, "grads_per_s": rate(ms_rg)}
        rec["host"]["reduce"]["grouped_over_loop"] = ms_rl / ms_rg
        parity["host_solve"] = all(same(ho_g[k], ho_l[k]) for k in SOLVE_FIELDS)
        u64 = lambda v: np.ascontiguousarray(v).view(np.uint64)
        parity["host_reduce"] = bool(
            all(np.array_equal(u64(res_g[0][0][g]), u64(res_l[g][0])) and int(res_g[0][1][g]) == res_l[g][1]
                for g in range(G))
            and same(res_g[0][2], np.concatenate([r[2] for r in res_l]))
            and same(res_g[0][3], np.concatenate([r[3] for r in res_l])))
        parity["host_same_bits_as_device"] = bool(np.array_equal(u64(res_g[0][0]), u64(dsh_g.cpu().numpy())))
        rec["parity"] = parity
    for p_ in pins[::-1]:
        p_.__exit__(None, None, None)
    print(json.dumps(rec), flush=True)
    if not new:
        return 0
    return 0 if all(v for k, v in parity.items() if k != "used") and parity["used"] > 0 else 1


if __name__ == "__main__":
    sys.exit(main())

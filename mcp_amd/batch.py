"""Batched solves through the C ABI (include/mcpx.h).

Two entry points, both running the HIP kernel (never a CPU fallback):

* :func:`solve_batch` — numpy host arrays in, numpy arrays out
  (``mcpx_solve_batch``: H→D copy, solve, D→H copy; shards over GPUs).
* :func:`solve_batch_device` — torch device tensors in and out, enqueued on
  the current HIP stream (``mcpx_solve_batch_device``); the benchmark's hot path.

Both return the per-instance fields of the reference's result NamedTuple
(src/solver.jl:121: status, x, y, s, kkt_error, ϵ, outer_iters) plus
``newton_iters``, ``active_mask`` and an optional ``alpha_trace``.
"""

from __future__ import annotations

import ctypes as C
import os

import numpy as np

from . import _abi
from ._lib import check, lib


def _ptr(a):
    return None if a is None else a.ctypes.data


def _params(params=None, **kw) -> _abi.Params:
    return params if params is not None else _abi.make_params(**kw)


class Module:
    """A generated nonlinear-MCP code object (mcp_amd/codegen.py) loaded through
    the C ABI (mcpx_module_load, include/mcpx.h MCPX_FAMILY_NONLINEAR).  Kept for
    the process lifetime unless close() is called."""

    def __init__(self, path: str):
        h = C.c_void_p()
        check(lib().mcpx_module_load(os.fsencode(path), C.byref(h)))
        self.handle = h
        v = [C.c_int32() for _ in range(4)]
        check(lib().mcpx_module_dims(h, *(C.byref(x) for x in v)))
        self.n, self.m, self.p, self.solvers = (x.value for x in v)
        self.path = path

    @property
    def has_vjp(self) -> bool:
        return bool((self.solvers >> _abi.MODULE_VJP) & 1)

    @property
    def has_jvp(self) -> bool:
        return bool((self.solvers >> _abi.MODULE_JVP) & 1)

    @property
    def has_schur_mw(self) -> bool:
        return bool((self.solvers >> _abi.MODULE_SCHUR_MW) & 1)

    def close(self) -> None:
        if self.handle:
            lib().mcpx_module_unload(self.handle)
            self.handle = None


def alloc_host_outputs(B: int, n: int, m: int, trace_len: int = 0) -> dict:
    """Host result buffers of solve_batch(out=...), first-touched here: reused across
    calls they spare the D→H copy the page faults of fresh numpy pages."""
    words = max(1, (m + 63) // 64)
    r = dict(
        x=np.zeros((B, n)), y=np.zeros((B, m)), s=np.zeros((B, m)), kkt_error=np.zeros(B),
        eps=np.zeros(B), outer_iters=np.zeros(B, np.int32), status=np.zeros(B, np.int32),
        newton_iters=np.zeros(B, np.int32),
        active_mask=np.zeros((B, words), np.uint64),
        alpha_trace=np.full((B, max(trace_len, 0), 2), 254, np.uint8),
        fail_reason=np.zeros(B, np.uint8),
    )
    return r


def _host_out(B: int, n: int, m: int, trace_len: int, out: dict | None):
    """The result arrays of a host-buffer solve (`out` when given, else fresh) and their mcpx_out."""
    words = max(1, (m + 63) // 64)
    if out is not None:
        r = out
        if r["x"].shape != (B, n) or r["y"].shape != (B, m) or r["status"].shape != (B,) or (
                trace_len > 0 and r["alpha_trace"].shape[1] < trace_len):
            raise ValueError("out buffers do not match the batch (alloc_host_outputs(B, n, m, trace_len))")
    else:
        r = dict(
            x=np.empty((B, n)), y=np.empty((B, m)), s=np.empty((B, m)), kkt_error=np.empty(B),
            eps=np.empty(B), outer_iters=np.empty(B, np.int32), status=np.empty(B, np.int32),
            newton_iters=np.empty(B, np.int32),
            active_mask=np.empty((B, words), np.uint64),
            alpha_trace=np.full((B, max(trace_len, 0), 2), 254, np.uint8),
            fail_reason=np.empty(B, np.uint8),
        )
    fr = r.get("fail_reason")
    return r, _abi.Out(_ptr(r["x"]), _ptr(r["y"]), _ptr(r["s"]), _ptr(r["kkt_error"]), _ptr(r["eps"]),
                      _ptr(r["outer_iters"]), _ptr(r["status"]), _ptr(r["newton_iters"]),
                      _ptr(r["active_mask"]), _ptr(r["alpha_trace"]) if trace_len > 0 else None,
                      int(trace_len), 0, _ptr(fr) if fr is not None else None)


def solve_batch(family: int, n: int, m: int, theta, *, x0=None, y0=None, s0=None, params=None,
                num_devices: int = 0, trace_len: int = 0, module: Module | None = None, out: dict | None = None,
                **kw) -> dict:
    """Solve B instances on the GPU(s).  theta: (B, ≥p) float64 host array.  `out`: result
    buffers from alloc_host_outputs (filled in place and returned), else fresh arrays."""
    theta = np.ascontiguousarray(theta, dtype=np.float64)
    if theta.ndim == 1:
        theta = theta[None, :]
    B, ld = theta.shape
    prm = _params(params, **kw)
    conv = lambda a, k: None if a is None else np.ascontiguousarray(np.broadcast_to(a, (B, k)), dtype=np.float64)
    x0, y0, s0 = conv(x0, n), conv(y0, m), conv(s0, m)
    r, out = _host_out(B, n, m, trace_len, out)
    desc = _abi.Desc(int(family), int(n), int(m), 0, int(B), int(ld))
    if module is not None:  # MCPX_FAMILY_NONLINEAR: the problem's generated code object
        check(lib().mcpx_solve_batch_module(module.handle, C.byref(desc), _ptr(theta), _ptr(x0), _ptr(y0),
                                            _ptr(s0), C.byref(prm), int(num_devices), C.byref(out)))
    else:
        check(lib().mcpx_solve_batch(C.byref(desc), _ptr(theta), _ptr(x0), _ptr(y0), _ptr(s0),
                                     C.byref(prm), int(num_devices), C.byref(out)))
    return r


def solve_batch_shared(family: int, n: int, m: int, theta_shared, theta_var, *, x0=None, y0=None, s0=None,
                       params=None, num_devices: int = 0, trace_len: int = 0, out: dict | None = None, **kw) -> dict:
    """solve_batch for a batch that shares its matrices (mcpx_solve_batch_shared; QP and affine
    families).  theta_shared: the _abi.theta_shared_dim doubles every instance has in common,
    once; theta_var: (B, ≥ _abi.theta_var_dim) — [b; ϕ] (QP) or [g; h] (affine) per instance.
    Every field equals solve_batch on the materialised [theta_shared ‖ theta_var] bit for bit;
    only theta_var crosses the host link per instance."""
    theta_shared = np.ascontiguousarray(theta_shared, dtype=np.float64).reshape(-1)
    if theta_shared.size != _abi.theta_shared_dim(family, n, m):
        raise ValueError(f"theta_shared has {theta_shared.size} entries, the family's shared block has "
                         f"{_abi.theta_shared_dim(family, n, m)}")
    theta_var = np.ascontiguousarray(theta_var, dtype=np.float64)
    if theta_var.ndim == 1:
        theta_var = theta_var[None, :]
    B, ld = theta_var.shape
    prm = _params(params, **kw)
    conv = lambda a, k: None if a is None else np.ascontiguousarray(np.broadcast_to(a, (B, k)), dtype=np.float64)
    x0, y0, s0 = conv(x0, n), conv(y0, m), conv(s0, m)
    r, o = _host_out(B, n, m, trace_len, out)
    desc = _abi.Desc(int(family), int(n), int(m), 0, int(B), int(ld))
    check(lib().mcpx_solve_batch_shared(C.byref(desc), _ptr(theta_shared), _ptr(theta_var), _ptr(x0), _ptr(y0),
                                        _ptr(s0), C.byref(prm), int(num_devices), C.byref(o)))
    return r


class pinned:
    """Context manager that page-locks a host numpy array for the host-buffer calls
    (mcpx_host_register / mcpx_host_unregister): θ is then read by asynchronous DMA
    straight from it while earlier chunks solve.  For long-lived input batches."""

    def __init__(self, array: np.ndarray):
        if not (isinstance(array, np.ndarray) and array.flags.c_contiguous):
            raise ValueError("pinned() needs a C-contiguous numpy array")
        self.array = array

    def __enter__(self):
        check(lib().mcpx_host_register(self.array.ctypes.data, self.array.nbytes))
        return self.array

    def __exit__(self, *exc):
        check(lib().mcpx_host_unregister(self.array.ctypes.data))
        return False


def alloc_device_outputs(B: int, n: int, m: int, device, trace_len: int = 0, newton: bool = True,
                         active: bool = True) -> dict:
    import torch

    f64 = dict(dtype=torch.float64, device=device)
    i32 = dict(dtype=torch.int32, device=device)
    return dict(
        x=torch.empty(B, n, **f64), y=torch.empty(B, m, **f64), s=torch.empty(B, m, **f64),
        kkt_error=torch.empty(B, **f64), eps=torch.empty(B, **f64),
        outer_iters=torch.empty(B, **i32), status=torch.empty(B, **i32),
        newton_iters=torch.empty(B, **i32) if newton else None,
        # (B, W) uint64 words, W = max(1, ⌈m/64⌉) — the host path's and distributed.py's shape
        active_mask=torch.empty(B, max(1, (m + 63) // 64), dtype=torch.int64, device=device) if active else None,
        alpha_trace=torch.full((B, trace_len, 2), 254, dtype=torch.uint8, device=device) if trace_len > 0 else None,
        fail_reason=torch.empty(B, dtype=torch.uint8, device=device),
    )


def solve_batch_device(family: int, n: int, m: int, theta, out: dict | None = None, *, x0=None, y0=None,
                       s0=None, params=None, trace_len: int = 0, stream=None, module: Module | None = None,
                       **kw) -> dict:
    """Enqueue a batched solve on torch device tensors (no synchronisation).

    theta: (B, ≥p) contiguous float64 CUDA(HIP) tensor.  `out` (from
    :func:`alloc_device_outputs`) is reused when given — nothing is allocated
    on the hot path then.
    """
    import torch

    if not (theta.is_cuda and theta.dtype == torch.float64 and theta.dim() == 2 and theta.is_contiguous()):
        raise ValueError("theta must be a contiguous (B, p) float64 device tensor")
    B, ld = theta.shape
    if out is None:
        out = alloc_device_outputs(B, n, m, theta.device, trace_len)
    for t in (x0, y0, s0):
        if t is not None and not (t.is_cuda and t.dtype == torch.float64 and t.is_contiguous()):
            raise ValueError("warm starts must be contiguous float64 device tensors")
    dp = lambda t: None if t is None else t.data_ptr()
    tl = 0 if out.get("alpha_trace") is None else out["alpha_trace"].shape[1]
    o = _abi.Out(dp(out["x"]), dp(out["y"]), dp(out["s"]), dp(out["kkt_error"]), dp(out["eps"]),
                 dp(out["outer_iters"]), dp(out["status"]), dp(out.get("newton_iters")),
                 dp(out.get("active_mask")), dp(out.get("alpha_trace")), int(tl), 0, dp(out.get("fail_reason")))
    prm = _params(params, **kw)
    desc = _abi.Desc(int(family), int(n), int(m), 0, int(B), int(ld))
    st = stream if stream is not None else torch.cuda.current_stream(theta.device)
    if module is not None:
        check(lib().mcpx_solve_batch_module_device(module.handle, C.byref(desc), dp(theta), dp(x0), dp(y0), dp(s0),
                                                   C.byref(prm), C.byref(o), C.c_void_p(st.cuda_stream)))
    else:
        check(lib().mcpx_solve_batch_device(C.byref(desc), dp(theta), dp(x0), dp(y0), dp(s0), C.byref(prm),
                                            C.byref(o), C.c_void_p(st.cuda_stream)))
    return out


def solve_batch_shared_device(family: int, n: int, m: int, theta_shared, theta_var, out: dict | None = None, *,
                              x0=None, y0=None, s0=None, params=None, trace_len: int = 0, stream=None, **kw) -> dict:
    """solve_batch_device for a batch that shares its matrices (mcpx_solve_batch_shared_device):
    theta_shared a contiguous float64 device tensor of _abi.theta_shared_dim entries, theta_var
    a contiguous (B, ≥ _abi.theta_var_dim) one.  Enqueued on the current stream, no
    synchronisation; the bits of solve_batch_device on the materialised θ′."""
    import torch

    ok = lambda t: t.is_cuda and t.dtype == torch.float64 and t.is_contiguous()
    if not (ok(theta_var) and theta_var.dim() == 2):
        raise ValueError("theta_var must be a contiguous (B, n + m) float64 device tensor")
    if not (ok(theta_shared) and theta_shared.numel() == _abi.theta_shared_dim(family, n, m)):
        raise ValueError("theta_shared must be a contiguous float64 device tensor of theta_shared_dim entries")
    B, ld = theta_var.shape
    if out is None:
        out = alloc_device_outputs(B, n, m, theta_var.device, trace_len)
    for t in (x0, y0, s0):
        if t is not None and not ok(t):
            raise ValueError("warm starts must be contiguous float64 device tensors")
    dp = lambda t: None if t is None else t.data_ptr()
    tl = 0 if out.get("alpha_trace") is None else out["alpha_trace"].shape[1]
    o = _abi.Out(dp(out["x"]), dp(out["y"]), dp(out["s"]), dp(out["kkt_error"]), dp(out["eps"]),
                 dp(out["outer_iters"]), dp(out["status"]), dp(out.get("newton_iters")),
                 dp(out.get("active_mask")), dp(out.get("alpha_trace")), int(tl), 0, dp(out.get("fail_reason")))
    prm = _params(params, **kw)
    desc = _abi.Desc(int(family), int(n), int(m), 0, int(B), int(ld))
    st = stream if stream is not None else torch.cuda.current_stream(theta_var.device)
    check(lib().mcpx_solve_batch_shared_device(C.byref(desc), dp(theta_shared), dp(theta_var), dp(x0), dp(y0), dp(s0),
                                               C.byref(prm), C.byref(o), C.c_void_p(st.cuda_stream)))
    return out


# ---------------------------------------------------------------------------
# sensitivities (reference src/AutoDiff.jl; include/mcpx.h mcpx_vjp_* / mcpx_jvp_*)


def _host_f64(a, shape):
    return None if a is None else np.ascontiguousarray(np.broadcast_to(a, shape), dtype=np.float64)


def _pdim(family: int, n: int, m: int, module: Module | None) -> int:
    return module.p if module is not None else _abi.theta_dim(family, n, m)


def vjp_batch(family: int, n: int, m: int, theta, x, y, s, gx=None, gy=None, gs=None,
              num_devices: int = 0, module: Module | None = None) -> tuple:
    """rrule pullback on the GPU(s) for host arrays: ∂θ = (∂z/∂θ)ᵀ [gx; gy; gs]
    (src/AutoDiff.jl:59-76).  None cotangents are zero.  Returns
    (dtheta (B, p) in the family's θ layout, status (B,) int32: 1 = ∇F_z singular).
    `module`: the generated module of a nonlinear-family MCP (mcpx_vjp_batch_module)."""
    theta = np.ascontiguousarray(np.atleast_2d(theta), dtype=np.float64)
    B, ld = theta.shape
    p = _pdim(family, n, m, module)
    x, y, s = _host_f64(x, (B, n)), _host_f64(y, (B, m)), _host_f64(s, (B, m))
    gx, gy, gs = _host_f64(gx, (B, n)), _host_f64(gy, (B, m)), _host_f64(gs, (B, m))
    dth = np.empty((B, p))
    st = np.empty(B, np.int32)
    desc = _abi.Desc(int(family), int(n), int(m), 0, int(B), int(ld))
    if module is not None:
        check(lib().mcpx_vjp_batch_module(module.handle, C.byref(desc), _ptr(theta), _ptr(x), _ptr(y), _ptr(s),
                                          _ptr(gx), _ptr(gy), _ptr(gs), int(num_devices), _ptr(dth), _ptr(st)))
    else:
        check(lib().mcpx_vjp_batch(C.byref(desc), _ptr(theta), _ptr(x), _ptr(y), _ptr(s), _ptr(gx), _ptr(gy),
                                   _ptr(gs), int(num_devices), _ptr(dth), _ptr(st)))
    return dth, st


def jvp_batch(family: int, n: int, m: int, theta, x, y, s, theta_dot, num_devices: int = 0,
              module: Module | None = None) -> tuple:
    """ForwardDiff-Dual tangents on the GPU(s): ż = (∂z/∂θ) θ̇ (src/AutoDiff.jl:94-100).
    theta_dot (B, K, p) → (zdot (B, K, n+2m), status (B,))."""
    theta = np.ascontiguousarray(np.atleast_2d(theta), dtype=np.float64)
    B, ld = theta.shape
    p = _pdim(family, n, m, module)
    td = np.ascontiguousarray(theta_dot, dtype=np.float64).reshape(B, -1, p)
    K = td.shape[1]
    x, y, s = _host_f64(x, (B, n)), _host_f64(y, (B, m)), _host_f64(s, (B, m))
    zd = np.empty((B, K, n + 2 * m))
    st = np.empty(B, np.int32)
    desc = _abi.Desc(int(family), int(n), int(m), 0, int(B), int(ld))
    if module is not None:
        check(lib().mcpx_jvp_batch_module(module.handle, C.byref(desc), _ptr(theta), _ptr(x), _ptr(y), _ptr(s),
                                          int(K), _ptr(td), int(num_devices), _ptr(zd), _ptr(st)))
    else:
        check(lib().mcpx_jvp_batch(C.byref(desc), _ptr(theta), _ptr(x), _ptr(y), _ptr(s), int(K), _ptr(td),
                                   int(num_devices), _ptr(zd), _ptr(st)))
    return zd, st


# rcond below which an instance's sensitivities count as ill-conditioned (include/mcpx.h
# mcpx_cond_batch): cond₁(∇F_z) > 1e12 leaves fewer than ~4 significant digits in ∂z/∂θ
ILL_CONDITIONED = 1e-12


def cond_batch(family: int, n: int, m: int, theta, x, y, s, num_devices: int = 0,
               module: Module | None = None) -> tuple:
    """Reciprocal 1-norm condition estimate of ∇F_z at the solutions (the matrix of the rrule's
    solve, src/AutoDiff.jl:39) on the GPU(s) → (rcond (B,), status (B,): 1 = exactly singular).
    `rcond < ILL_CONDITIONED` is the per-instance ill-conditioning flag."""
    theta = np.ascontiguousarray(np.atleast_2d(theta), dtype=np.float64)
    B, ld = theta.shape
    x, y, s = _host_f64(x, (B, n)), _host_f64(y, (B, m)), _host_f64(s, (B, m))
    rc = np.empty(B)
    st = np.empty(B, np.int32)
    desc = _abi.Desc(int(family), int(n), int(m), 0, int(B), int(ld))
    if module is not None:
        check(lib().mcpx_cond_batch_module(module.handle, C.byref(desc), _ptr(theta), _ptr(x), _ptr(y), _ptr(s),
                                           int(num_devices), _ptr(rc), _ptr(st)))
    else:
        check(lib().mcpx_cond_batch(C.byref(desc), _ptr(theta), _ptr(x), _ptr(y), _ptr(s), int(num_devices),
                                    _ptr(rc), _ptr(st)))
    return rc, st


def _dev_f64(t, what):
    import torch

    if t is None:
        return None
    if not (t.is_cuda and t.dtype == torch.float64 and t.is_contiguous()):
        raise ValueError(f"{what} must be a contiguous float64 device tensor")
    return t.data_ptr()


def vjp_batch_device(family: int, n: int, m: int, theta, x, y, s, gx=None, gy=None, gs=None, dtheta=None,
                     status=None, stream=None, module: Module | None = None):
    """Device-tensor pullback enqueued on the current stream (no sync).
    Returns (dtheta (B, p), status (B,) int32) tensors."""
    import torch

    if not (theta.is_cuda and theta.dtype == torch.float64 and theta.dim() == 2 and theta.is_contiguous()):
        raise ValueError("theta must be a contiguous (B, p) float64 device tensor")
    B, ld = theta.shape
    p = _pdim(family, n, m, module)
    dev = theta.device
    if dtheta is None:
        dtheta = torch.empty(B, p, dtype=torch.float64, device=dev)
    if status is None:
        status = torch.empty(B, dtype=torch.int32, device=dev)
    ptrs = [_dev_f64(t, k) for t, k in ((x, "x"), (y, "y"), (s, "s"), (gx, "gx"), (gy, "gy"), (gs, "gs"))]
    desc = _abi.Desc(int(family), int(n), int(m), 0, int(B), int(ld))
    st = stream if stream is not None else torch.cuda.current_stream(dev)
    if module is not None:
        check(lib().mcpx_vjp_batch_module_device(module.handle, C.byref(desc), theta.data_ptr(), *ptrs,
                                                 _dev_f64(dtheta, "dtheta"), status.data_ptr(),
                                                 C.c_void_p(st.cuda_stream)))
    else:
        check(lib().mcpx_vjp_batch_device(C.byref(desc), theta.data_ptr(), *ptrs, _dev_f64(dtheta, "dtheta"),
                                          status.data_ptr(), C.c_void_p(st.cuda_stream)))
    return dtheta, status


def solve_vjp_batch_device(family: int, n: int, m: int, theta, out: dict | None = None, *, ct=(0.0, 0.0, 0.0),
                           bx=None, by=None, bs=None, dtheta=None, status=None, x0=None, y0=None, s0=None,
                           params=None, stream=None, **kw):
    """Solve and pull back in one call (mcpx_solve_vjp_batch_device): the solve into
    `out` (as :func:`solve_batch_device`), then ∂θ of the loss whose cotangent is
    ∂l/∂x = ct[0]·x + bx, ∂l/∂y = ct[1]·y + by, ∂l/∂s = ct[2]·s + bs (b tensors or
    None = 0).  The README / C5 loss f = Σx² + Σy² is ct = (2, 2, 0).  SCHUR QPs at the
    benchmark sizes run the pullback inside the solve kernel.  Returns
    (out, dtheta (B, p), status (B,))."""
    import torch

    if not (theta.is_cuda and theta.dtype == torch.float64 and theta.dim() == 2 and theta.is_contiguous()):
        raise ValueError("theta must be a contiguous (B, p) float64 device tensor")
    B, ld = theta.shape
    dev = theta.device
    if out is None:
        out = alloc_device_outputs(B, n, m, dev)
    if dtheta is None:
        dtheta = torch.empty(B, _abi.theta_dim(family, n, m), dtype=torch.float64, device=dev)
    if status is None:
        status = torch.empty(B, dtype=torch.int32, device=dev)
    for t in (x0, y0, s0):
        if t is not None and not (t.is_cuda and t.dtype == torch.float64 and t.is_contiguous()):
            raise ValueError("warm starts must be contiguous float64 device tensors")
    dp = lambda t: None if t is None else t.data_ptr()
    tl = 0 if out.get("alpha_trace") is None else out["alpha_trace"].shape[1]
    o = _abi.Out(dp(out["x"]), dp(out["y"]), dp(out["s"]), dp(out["kkt_error"]), dp(out["eps"]),
                 dp(out["outer_iters"]), dp(out["status"]), dp(out.get("newton_iters")),
                 dp(out.get("active_mask")), dp(out.get("alpha_trace")), int(tl), 0, dp(out.get("fail_reason")))
    cot = _abi.Cotangent(float(ct[0]), float(ct[1]), float(ct[2]), _dev_f64(bx, "bx"), _dev_f64(by, "by"),
                         _dev_f64(bs, "bs"))
    prm = _params(params, **kw)
    desc = _abi.Desc(int(family), int(n), int(m), 0, int(B), int(ld))
    st = stream if stream is not None else torch.cuda.current_stream(dev)
    check(lib().mcpx_solve_vjp_batch_device(C.byref(desc), dp(theta), dp(x0), dp(y0), dp(s0), C.byref(prm),
                                            C.byref(o), C.byref(cot), _dev_f64(dtheta, "dtheta"), dp(status),
                                            C.c_void_p(st.cuda_stream)))
    return out, dtheta, status


def jvp_batch_device(family: int, n: int, m: int, theta, x, y, s, theta_dot, zdot=None, status=None,
                     stream=None, module: Module | None = None):
    """Device-tensor tangents: theta_dot (B, K, p) → (zdot (B, K, n+2m), status (B,))."""
    import torch

    if not (theta.is_cuda and theta.dtype == torch.float64 and theta.dim() == 2 and theta.is_contiguous()):
        raise ValueError("theta must be a contiguous (B, p) float64 device tensor")
    B, ld = theta.shape
    p = _pdim(family, n, m, module)
    td = theta_dot.reshape(B, -1, p)
    K = td.shape[1]
    dev = theta.device
    if zdot is None:
        zdot = torch.empty(B, K, n + 2 * m, dtype=torch.float64, device=dev)
    if status is None:
        status = torch.empty(B, dtype=torch.int32, device=dev)
    desc = _abi.Desc(int(family), int(n), int(m), 0, int(B), int(ld))
    st = stream if stream is not None else torch.cuda.current_stream(dev)
    fn = lib().mcpx_jvp_batch_device if module is None else (
        lambda *a: lib().mcpx_jvp_batch_module_device(module.handle, *a))
    check(fn(C.byref(desc), theta.data_ptr(), _dev_f64(x, "x"), _dev_f64(y, "y"), _dev_f64(s, "s"), int(K),
             _dev_f64(td.contiguous(), "theta_dot"), _dev_f64(zdot, "zdot"), status.data_ptr(),
             C.c_void_p(st.cuda_stream)))
    return zdot, status


# ---------------------------------------------------------------------------
# sensitivities of a shared-matrix batch (include/mcpx.h mcpx_vjp_batch_shared* /
# mcpx_jvp_batch_shared* / mcpx_solve_vjp_batch_shared_device): one matrix block for the
# batch, gradients and tangents of the per-instance block [b; ϕ] (QP) / [g; h] (affine) only


def _host_shared(family: int, n: int, m: int, theta_shared) -> np.ndarray:
    theta_shared = np.ascontiguousarray(theta_shared, dtype=np.float64).reshape(-1)
    if theta_shared.size != _abi.theta_shared_dim(family, n, m):
        raise ValueError(f"theta_shared has {theta_shared.size} entries, the family's shared block has "
                         f"{_abi.theta_shared_dim(family, n, m)}")
    return theta_shared


def _dev_shared(family: int, n: int, m: int, theta_shared) -> int:
    import torch

    if not (theta_shared.is_cuda and theta_shared.dtype == torch.float64 and theta_shared.is_contiguous()
            and theta_shared.numel() == _abi.theta_shared_dim(family, n, m)):
        raise ValueError("theta_shared must be a contiguous float64 device tensor of theta_shared_dim entries")
    return theta_shared.data_ptr()


def _batch_of(x, y, n: int, m: int) -> int:
    """Instances of a split sensitivity call: the rows of x (of y when n = 0)."""
    a = x if n > 0 else y
    return int(a.shape[0]) if a.ndim == 2 else 1


def vjp_batch_shared(family: int, n: int, m: int, theta_shared, x, y, s, gx=None, gy=None, gs=None,
                     num_devices: int = 0) -> tuple:
    """vjp_batch for a shared-matrix batch (mcpx_vjp_batch_shared): theta_shared as in
    solve_batch_shared, no per-instance θ (∇F_z does not contain it).  Returns (dvar (B, n + m) —
    [∂b; ∂ϕ] (QP) or [∂g; ∂h] (affine), the bits of vjp_batch(θ′)[0][:, shared_dim:] — and
    status (B,))."""
    theta_shared = _host_shared(family, n, m, theta_shared)
    B = _batch_of(np.atleast_2d(np.asarray(x)), np.atleast_2d(np.asarray(y)), n, m)
    dv = _abi.theta_var_dim(family, n, m)
    x, y, s = _host_f64(x, (B, n)), _host_f64(y, (B, m)), _host_f64(s, (B, m))
    gx, gy, gs = _host_f64(gx, (B, n)), _host_f64(gy, (B, m)), _host_f64(gs, (B, m))
    dvar = np.empty((B, dv))
    st = np.empty(B, np.int32)
    desc = _abi.Desc(int(family), int(n), int(m), 0, int(B), int(dv))
    check(lib().mcpx_vjp_batch_shared(C.byref(desc), _ptr(theta_shared), _ptr(x), _ptr(y), _ptr(s), _ptr(gx),
                                      _ptr(gy), _ptr(gs), int(num_devices), _ptr(dvar), _ptr(st)))
    return dvar, st


def _need_a_tangent(var_dot, shared_dot) -> None:
    if var_dot is None and shared_dot is None:
        raise ValueError("var_dot is None: give var_dot, shared_dot or both")


def _shared_dot_partials(shared_dot_size: int, ds: int, vd_partials: int | None) -> int:
    """K of a tangent call from shared_dot (K, shared_dim) and, when given, var_dot's K."""
    if ds == 0 or shared_dot_size % ds:
        raise ValueError(f"shared_dot must be (K, {ds}): K tangents of the shared block")
    K = shared_dot_size // ds
    if vd_partials is not None and vd_partials != K:
        raise ValueError(f"shared_dot has {K} partials, var_dot {vd_partials}")
    return K


def jvp_batch_shared(family: int, n: int, m: int, theta_shared, x, y, s, var_dot, num_devices: int = 0,
                     shared_dot=None) -> tuple:
    """jvp_batch for a shared-matrix batch (mcpx_jvp_batch_shared): var_dot (B, K, n + m), the
    tangents of the per-instance block (the matrix block's are zero) → (zdot (B, K, n+2m),
    status (B,)), the bits of jvp_batch on θ̇ = [0 ‖ var_dot] for finite iterates.
    `shared_dot` (K, shared_dim): the tangents of the shared block too, given once for the batch
    (mcpx_jvp_batch_shared_dot) — the bits of jvp_batch on θ̇_{b,c} = [shared_dot_c ‖ var_dot_{b,c}],
    whatever the iterate; var_dot may then be None (zero)."""
    theta_shared = _host_shared(family, n, m, theta_shared)
    B = _batch_of(np.atleast_2d(np.asarray(x)), np.atleast_2d(np.asarray(y)), n, m)
    dv = _abi.theta_var_dim(family, n, m)
    _need_a_tangent(var_dot, shared_dot)
    vd = None if var_dot is None else np.ascontiguousarray(var_dot, dtype=np.float64).reshape(B, -1, dv)
    if shared_dot is None:
        K = vd.shape[1]
    else:
        sd = np.ascontiguousarray(shared_dot, dtype=np.float64)
        K = _shared_dot_partials(sd.size, theta_shared.size, None if vd is None else vd.shape[1])
    x, y, s = _host_f64(x, (B, n)), _host_f64(y, (B, m)), _host_f64(s, (B, m))
    zd = np.empty((B, K, n + 2 * m))
    st = np.empty(B, np.int32)
    desc = _abi.Desc(int(family), int(n), int(m), 0, int(B), int(dv))
    if shared_dot is None:
        check(lib().mcpx_jvp_batch_shared(C.byref(desc), _ptr(theta_shared), _ptr(x), _ptr(y), _ptr(s), int(K),
                                          _ptr(vd), int(num_devices), _ptr(zd), _ptr(st)))
    else:
        check(lib().mcpx_jvp_batch_shared_dot(C.byref(desc), _ptr(theta_shared), _ptr(x), _ptr(y), _ptr(s), int(K),
                                              _ptr(sd), _ptr(vd), int(num_devices), _ptr(zd), _ptr(st)))
    return zd, st


def cond_batch_shared(family: int, n: int, m: int, theta_shared, x, y, s, num_devices: int = 0) -> tuple:
    """cond_batch for a shared-matrix batch (mcpx_cond_batch_shared): theta_shared as in
    solve_batch_shared, no per-instance θ (∇F_z does not contain it) → (rcond (B,), status (B,)),
    the bits of cond_batch on the materialised θ′."""
    theta_shared = _host_shared(family, n, m, theta_shared)
    B = _batch_of(np.atleast_2d(np.asarray(x)), np.atleast_2d(np.asarray(y)), n, m)
    x, y, s = _host_f64(x, (B, n)), _host_f64(y, (B, m)), _host_f64(s, (B, m))
    rc = np.empty(B)
    st = np.empty(B, np.int32)
    desc = _abi.Desc(int(family), int(n), int(m), 0, int(B), int(_abi.theta_var_dim(family, n, m)))
    check(lib().mcpx_cond_batch_shared(C.byref(desc), _ptr(theta_shared), _ptr(x), _ptr(y), _ptr(s),
                                       int(num_devices), _ptr(rc), _ptr(st)))
    return rc, st


def vjp_batch_shared_device(family: int, n: int, m: int, theta_shared, x, y, s, gx=None, gy=None, gs=None,
                            dvar=None, status=None, stream=None):
    """Device-tensor pullback of a shared-matrix batch, enqueued on the current stream (no sync):
    (dvar (B, n + m), status (B,) int32) tensors."""
    import torch

    sh = _dev_shared(family, n, m, theta_shared)
    B = _batch_of(x, y, n, m)
    dv = _abi.theta_var_dim(family, n, m)
    dev = theta_shared.device
    if dvar is None:
        dvar = torch.empty(B, dv, dtype=torch.float64, device=dev)
    if status is None:
        status = torch.empty(B, dtype=torch.int32, device=dev)
    ptrs = [_dev_f64(t, k) for t, k in ((x, "x"), (y, "y"), (s, "s"), (gx, "gx"), (gy, "gy"), (gs, "gs"))]
    desc = _abi.Desc(int(family), int(n), int(m), 0, int(B), int(dv))
    st = stream if stream is not None else torch.cuda.current_stream(dev)
    check(lib().mcpx_vjp_batch_shared_device(C.byref(desc), sh, *ptrs, _dev_f64(dvar, "dvar"), status.data_ptr(),
                                             C.c_void_p(st.cuda_stream)))
    return dvar, status


def jvp_batch_shared_device(family: int, n: int, m: int, theta_shared, x, y, s, var_dot, zdot=None, status=None,
                            stream=None, shared_dot=None):
    """Device-tensor tangents of a shared-matrix batch: var_dot (B, K, n + m) →
    (zdot (B, K, n+2m), status (B,)).  `shared_dot` (K, shared_dim), a device tensor: the tangents
    of the shared block too (mcpx_jvp_batch_shared_dot_device); var_dot may then be None."""
    import torch

    sh = _dev_shared(family, n, m, theta_shared)
    B = _batch_of(x, y, n, m)
    dv = _abi.theta_var_dim(family, n, m)
    _need_a_tangent(var_dot, shared_dot)
    vd = None if var_dot is None else var_dot.reshape(B, -1, dv).contiguous()
    K = vd.shape[1] if shared_dot is None else _shared_dot_partials(
        shared_dot.numel(), theta_shared.numel(), None if vd is None else vd.shape[1])
    dev = theta_shared.device
    if zdot is None:
        zdot = torch.empty(B, K, n + 2 * m, dtype=torch.float64, device=dev)
    if status is None:
        status = torch.empty(B, dtype=torch.int32, device=dev)
    desc = _abi.Desc(int(family), int(n), int(m), 0, int(B), int(dv))
    st = stream if stream is not None else torch.cuda.current_stream(dev)
    if shared_dot is None:
        check(lib().mcpx_jvp_batch_shared_device(C.byref(desc), sh, _dev_f64(x, "x"), _dev_f64(y, "y"),
                                                 _dev_f64(s, "s"), int(K), _dev_f64(vd, "var_dot"),
                                                 _dev_f64(zdot, "zdot"), status.data_ptr(),
                                                 C.c_void_p(st.cuda_stream)))
    else:
        check(lib().mcpx_jvp_batch_shared_dot_device(C.byref(desc), sh, _dev_f64(x, "x"), _dev_f64(y, "y"),
                                                     _dev_f64(s, "s"), int(K), _dev_f64(shared_dot, "shared_dot"),
                                                     _dev_f64(vd, "var_dot"), _dev_f64(zdot, "zdot"),
                                                     status.data_ptr(), C.c_void_p(st.cuda_stream)))
    return zdot, status


def cond_batch_shared_device(family: int, n: int, m: int, theta_shared, x, y, s, rcond=None, status=None,
                             stream=None):
    """Device-tensor condition estimate of a shared-matrix batch (mcpx_cond_batch_shared_device),
    enqueued on the current stream (no sync): (rcond (B,), status (B,) int32) tensors."""
    import torch

    sh = _dev_shared(family, n, m, theta_shared)
    B = _batch_of(x, y, n, m)
    dev = theta_shared.device
    if rcond is None:
        rcond = torch.empty(B, dtype=torch.float64, device=dev)
    if status is None:
        status = torch.empty(B, dtype=torch.int32, device=dev)
    desc = _abi.Desc(int(family), int(n), int(m), 0, int(B), int(_abi.theta_var_dim(family, n, m)))
    st = stream if stream is not None else torch.cuda.current_stream(dev)
    check(lib().mcpx_cond_batch_shared_device(C.byref(desc), sh, _dev_f64(x, "x"), _dev_f64(y, "y"), _dev_f64(s, "s"),
                                              _dev_f64(rcond, "rcond"), status.data_ptr(),
                                              C.c_void_p(st.cuda_stream)))
    return rcond, status


def solve_vjp_batch_shared_device(family: int, n: int, m: int, theta_shared, theta_var, out: dict | None = None, *,
                                  ct=(0.0, 0.0, 0.0), bx=None, by=None, bs=None, dvar=None, status=None, x0=None,
                                  y0=None, s0=None, params=None, stream=None, **kw):
    """solve_vjp_batch_device for a shared-matrix batch (mcpx_solve_vjp_batch_shared_device): the
    solve of solve_batch_shared_device into `out`, then the gradient of the per-instance block
    for the cotangent ct[k]·z + b (as there).  Returns (out, dvar (B, n + m), status (B,))."""
    import torch

    ok = lambda t: t.is_cuda and t.dtype == torch.float64 and t.is_contiguous()
    if not (ok(theta_var) and theta_var.dim() == 2):
        raise ValueError("theta_var must be a contiguous (B, n + m) float64 device tensor")
    sh = _dev_shared(family, n, m, theta_shared)
    B, ld = theta_var.shape
    dev = theta_var.device
    if out is None:
        out = alloc_device_outputs(B, n, m, dev)
    if dvar is None:
        dvar = torch.empty(B, _abi.theta_var_dim(family, n, m), dtype=torch.float64, device=dev)
    if status is None:
        status = torch.empty(B, dtype=torch.int32, device=dev)
    for t in (x0, y0, s0):
        if t is not None and not ok(t):
            raise ValueError("warm starts must be contiguous float64 device tensors")
    dp = lambda t: None if t is None else t.data_ptr()
    tl = 0 if out.get("alpha_trace") is None else out["alpha_trace"].shape[1]
    o = _abi.Out(dp(out["x"]), dp(out["y"]), dp(out["s"]), dp(out["kkt_error"]), dp(out["eps"]),
                 dp(out["outer_iters"]), dp(out["status"]), dp(out.get("newton_iters")),
                 dp(out.get("active_mask")), dp(out.get("alpha_trace")), int(tl), 0, dp(out.get("fail_reason")))
    cot = _abi.Cotangent(float(ct[0]), float(ct[1]), float(ct[2]), _dev_f64(bx, "bx"), _dev_f64(by, "by"),
                         _dev_f64(bs, "bs"))
    prm = _params(params, **kw)
    desc = _abi.Desc(int(family), int(n), int(m), 0, int(B), int(ld))
    st = stream if stream is not None else torch.cuda.current_stream(dev)
    check(lib().mcpx_solve_vjp_batch_shared_device(C.byref(desc), sh, dp(theta_var), dp(x0), dp(y0), dp(s0),
                                                   C.byref(prm), C.byref(o), C.byref(cot), _dev_f64(dvar, "dvar"),
                                                   dp(status), C.c_void_p(st.cuda_stream)))
    return out, dvar, status


# ---------------------------------------------------------------------------
# the reduced gradient of the matrix block of a shared-matrix batch (include/mcpx.h
# mcpx_vjp_batch_shared_reduce*): Σ_b ∂shared for matrices that are weights shared by the batch


def vjp_batch_shared_reduce(family: int, n: int, m: int, theta_shared, x, y, s, gx=None, gy=None, gs=None,
                            skip=None, num_devices: int = 0, want_dvar: bool = True) -> tuple:
    """vjp_batch_shared plus the gradient of the shared block summed over the batch
    (mcpx_vjp_batch_shared_reduce).  `skip` (B,): instances with a nonzero entry are left out of the
    sum, as are those whose pullback status is 1.  Returns (dshared (shared_dim,) in the layout of
    theta_shared, used: the number of instances summed, dvar (B, n + m) or None, status (B,)); dvar
    and status are vjp_batch_shared's.  dshared has one defined bit pattern (chunks of
    _abi.REDUCE_CHUNK instances, include/mcpx.h), whatever the devices and shards."""
    theta_shared = _host_shared(family, n, m, theta_shared)
    B = _batch_of(np.atleast_2d(np.asarray(x)), np.atleast_2d(np.asarray(y)), n, m)
    dv = _abi.theta_var_dim(family, n, m)
    x, y, s = _host_f64(x, (B, n)), _host_f64(y, (B, m)), _host_f64(s, (B, m))
    gx, gy, gs = _host_f64(gx, (B, n)), _host_f64(gy, (B, m)), _host_f64(gs, (B, m))
    if skip is not None:
        skip = np.ascontiguousarray(np.broadcast_to(np.asarray(skip) != 0, (B,)), dtype=np.uint8)
    dshared = np.empty(theta_shared.size)
    used = np.zeros(1, np.int64)
    dvar = np.empty((B, dv)) if want_dvar else None
    st = np.empty(B, np.int32)
    desc = _abi.Desc(int(family), int(n), int(m), 0, int(B), int(dv))
    check(lib().mcpx_vjp_batch_shared_reduce(C.byref(desc), _ptr(theta_shared), _ptr(x), _ptr(y), _ptr(s), _ptr(gx),
                                             _ptr(gy), _ptr(gs), _ptr(skip), int(num_devices), _ptr(dshared),
                                             _ptr(used), _ptr(dvar), _ptr(st)))
    return dshared, int(used[0]), dvar, st


def vjp_batch_shared_reduce_device(family: int, n: int, m: int, theta_shared, x, y, s, gx=None, gy=None, gs=None,
                                   skip=None, dshared=None, used=None, dvar=None, status=None,
                                   want_dvar: bool = True, stream=None):
    """Device-tensor form, enqueued on the current stream (no sync): `skip` a (B,) uint8 / bool
    device tensor or None.  Returns (dshared (shared_dim,), used (1,) int64, dvar (B, n + m) or
    None, status (B,) int32) tensors.  want_dvar=False with dvar=None: the pullback's λ stays in a
    block of the library's own and None is returned for it."""
    import torch

    sh = _dev_shared(family, n, m, theta_shared)
    B = _batch_of(x, y, n, m)
    dv = _abi.theta_var_dim(family, n, m)
    dev = theta_shared.device
    if dshared is None:
        dshared = torch.empty(theta_shared.numel(), dtype=torch.float64, device=dev)
    if used is None:
        used = torch.empty(1, dtype=torch.int64, device=dev)
    if dvar is None and want_dvar:
        dvar = torch.empty(B, dv, dtype=torch.float64, device=dev)
    if status is None:
        status = torch.empty(B, dtype=torch.int32, device=dev)
    if skip is not None:
        if skip.dtype == torch.bool:
            skip = skip.view(torch.uint8)
        if not (skip.is_cuda and skip.dtype == torch.uint8 and skip.is_contiguous() and skip.numel() == B):
            raise ValueError("skip must be a contiguous (B,) uint8 or bool device tensor")
    if not (used.is_cuda and used.dtype == torch.int64 and used.numel() == 1):
        raise ValueError("used must be a one-element int64 device tensor")
    ptrs = [_dev_f64(t, k) for t, k in ((x, "x"), (y, "y"), (s, "s"), (gx, "gx"), (gy, "gy"), (gs, "gs"))]
    desc = _abi.Desc(int(family), int(n), int(m), 0, int(B), int(dv))
    st = stream if stream is not None else torch.cuda.current_stream(dev)
    check(lib().mcpx_vjp_batch_shared_reduce_device(
        C.byref(desc), sh, *ptrs, None if skip is None else skip.data_ptr(), _dev_f64(dshared, "dshared"),
        used.data_ptr(), _dev_f64(dvar, "dvar"), status.data_ptr(), C.c_void_p(st.cuda_stream)))
    return dshared, used, dvar, status


# ---------------------------------------------------------------------------
# grouped shared-matrix batches (include/mcpx.h mcpx_*_batch_grouped*): G matrix blocks, each shared
# by a run of instances — between one block per instance (solve_batch) and one per batch (*_shared)


def _group_offsets(group_sizes, B: int) -> np.ndarray:
    """The G + 1 host offsets of `group_sizes` (G non-negative ints that sum to B)."""
    sizes = np.asarray(list(group_sizes), dtype=np.int64).reshape(-1)
    if sizes.size and sizes.min() < 0:
        raise ValueError("group_sizes must be non-negative")
    if int(sizes.sum()) != int(B):
        raise ValueError(f"group_sizes sum to {int(sizes.sum())}, the batch has {int(B)} instances")
    return np.concatenate([np.zeros(1, np.int64), np.cumsum(sizes, dtype=np.int64)])


def _host_groups(family: int, n: int, m: int, theta_shared, G: int):
    """(array, shared_ld) of a host (G, shared_dim) block array, or a 2-D view of a padded one."""
    ds = _abi.theta_shared_dim(family, n, m)
    a = np.asarray(theta_shared, dtype=np.float64)
    if a.ndim != 2 or a.shape != (G, ds):
        raise ValueError(f"theta_shared must be (G, shared_dim) = ({G}, {ds}), got {a.shape}")
    if G > 1 and ds > 0 and a.strides[1] == 8 and a.strides[0] >= 8 * ds and a.strides[0] % 8 == 0:
        return a, a.strides[0] // 8  # rows in place, padding and all
    return np.ascontiguousarray(a), ds


def _dev_groups(family: int, n: int, m: int, theta_shared, G: int):
    """(pointer, shared_ld) of a device (G, shared_dim) float64 tensor or a padded 2-D view."""
    import torch

    ds = _abi.theta_shared_dim(family, n, m)
    t = theta_shared
    if not (t.is_cuda and t.dtype == torch.float64 and t.dim() == 2 and tuple(t.shape) == (G, ds)):
        raise ValueError(f"theta_shared must be a (G, shared_dim) = ({G}, {ds}) float64 device tensor")
    if G > 1 and ds > 0:
        if not (t.stride(1) == 1 and t.stride(0) >= ds):
            raise ValueError("theta_shared rows must be contiguous (a padded 2-D view is fine)")
        return t.data_ptr(), t.stride(0)
    if not t.is_contiguous():
        raise ValueError("theta_shared must be contiguous")
    return t.data_ptr(), ds


def solve_batch_grouped(family: int, n: int, m: int, theta_shared, theta_var, group_sizes, *, x0=None, y0=None,
                        s0=None, params=None, num_devices: int = 0, trace_len: int = 0, out: dict | None = None,
                        **kw) -> dict:
    """solve_batch for a batch of G runs of instances, each run sharing its matrices
    (mcpx_solve_batch_grouped).  theta_shared: (G, shared_dim) or a padded 2-D view; theta_var:
    (B, ≥ var_dim); group_sizes: G ints summing to B, run g takes the next group_sizes[g] instances
    (0 allowed).  Every field equals solve_batch on the materialised θ′ bit for bit."""
    theta_var = np.ascontiguousarray(theta_var, dtype=np.float64)
    if theta_var.ndim == 1:
        theta_var = theta_var[None, :]
    B, ld = theta_var.shape
    off = _group_offsets(group_sizes, B)
    G = off.size - 1
    sh, sld = _host_groups(family, n, m, theta_shared, G)
    prm = _params(params, **kw)
    conv = lambda a, k: None if a is None else np.ascontiguousarray(np.broadcast_to(a, (B, k)), dtype=np.float64)
    x0, y0, s0 = conv(x0, n), conv(y0, m), conv(s0, m)
    r, o = _host_out(B, n, m, trace_len, out)
    desc = _abi.Desc(int(family), int(n), int(m), 0, int(B), int(ld))
    check(lib().mcpx_solve_batch_grouped(C.byref(desc), _ptr(sh), int(sld), int(G), _ptr(off), _ptr(theta_var),
                                         _ptr(x0), _ptr(y0), _ptr(s0), C.byref(prm), int(num_devices), C.byref(o)))
    return r


def solve_batch_grouped_device(family: int, n: int, m: int, theta_shared, theta_var, group_sizes,
                               out: dict | None = None, *, x0=None, y0=None, s0=None, params=None,
                               trace_len: int = 0, stream=None, **kw) -> dict:
    """Device-tensor form (mcpx_solve_batch_grouped_device), enqueued on the current stream, no
    synchronisation; group_sizes stays a host sequence."""
    import torch

    ok = lambda t: t.is_cuda and t.dtype == torch.float64 and t.is_contiguous()
    if not (ok(theta_var) and theta_var.dim() == 2):
        raise ValueError("theta_var must be a contiguous (B, n + m) float64 device tensor")
    B, ld = theta_var.shape
    off = _group_offsets(group_sizes, B)
    G = off.size - 1
    sh, sld = _dev_groups(family, n, m, theta_shared, G)
    if out is None:
        out = alloc_device_outputs(B, n, m, theta_var.device, trace_len)
    for t in (x0, y0, s0):
        if t is not None and not ok(t):
            raise ValueError("warm starts must be contiguous float64 device tensors")
    dp = lambda t: None if t is None else t.data_ptr()
    tl = 0 if out.get("alpha_trace") is None else out["alpha_trace"].shape[1]
    o = _abi.Out(dp(out["x"]), dp(out["y"]), dp(out["s"]), dp(out["kkt_error"]), dp(out["eps"]),
                 dp(out["outer_iters"]), dp(out["status"]), dp(out.get("newton_iters")),
                 dp(out.get("active_mask")), dp(out.get("alpha_trace")), int(tl), 0, dp(out.get("fail_reason")))
    prm = _params(params, **kw)
    desc = _abi.Desc(int(family), int(n), int(m), 0, int(B), int(ld))
    st = stream if stream is not None else torch.cuda.current_stream(theta_var.device)
    check(lib().mcpx_solve_batch_grouped_device(C.byref(desc), sh, int(sld), int(G), _ptr(off), dp(theta_var), dp(x0),
                                                dp(y0), dp(s0), C.byref(prm), C.byref(o),
                                                C.c_void_p(st.cuda_stream)))
    return out


def vjp_batch_grouped(family: int, n: int, m: int, theta_shared, x, y, s, group_sizes, gx=None, gy=None, gs=None,
                      num_devices: int = 0) -> tuple:
    """vjp_batch_shared for a grouped batch (mcpx_vjp_batch_grouped): (dvar (B, n + m), status (B,)),
    the bits of vjp_batch_shared on each group alone."""
    B = _batch_of(np.atleast_2d(np.asarray(x)), np.atleast_2d(np.asarray(y)), n, m)
    off = _group_offsets(group_sizes, B)
    G = off.size - 1
    sh, sld = _host_groups(family, n, m, theta_shared, G)
    dv = _abi.theta_var_dim(family, n, m)
    x, y, s = _host_f64(x, (B, n)), _host_f64(y, (B, m)), _host_f64(s, (B, m))
    gx, gy, gs = _host_f64(gx, (B, n)), _host_f64(gy, (B, m)), _host_f64(gs, (B, m))
    dvar = np.empty((B, dv))
    st = np.empty(B, np.int32)
    desc = _abi.Desc(int(family), int(n), int(m), 0, int(B), int(dv))
    check(lib().mcpx_vjp_batch_grouped(C.byref(desc), _ptr(sh), int(sld), int(G), _ptr(off), _ptr(x), _ptr(y), _ptr(s),
                                       _ptr(gx), _ptr(gy), _ptr(gs), int(num_devices), _ptr(dvar), _ptr(st)))
    return dvar, st


def vjp_batch_grouped_device(family: int, n: int, m: int, theta_shared, x, y, s, group_sizes, gx=None, gy=None,
                             gs=None, dvar=None, status=None, stream=None):
    """Device-tensor pullback of a grouped batch, enqueued on the current stream (no sync)."""
    import torch

    B = _batch_of(x, y, n, m)
    off = _group_offsets(group_sizes, B)
    G = off.size - 1
    sh, sld = _dev_groups(family, n, m, theta_shared, G)
    dv = _abi.theta_var_dim(family, n, m)
    dev = theta_shared.device
    if dvar is None:
        dvar = torch.empty(B, dv, dtype=torch.float64, device=dev)
    if status is None:
        status = torch.empty(B, dtype=torch.int32, device=dev)
    ptrs = [_dev_f64(t, k) for t, k in ((x, "x"), (y, "y"), (s, "s"), (gx, "gx"), (gy, "gy"), (gs, "gs"))]
    desc = _abi.Desc(int(family), int(n), int(m), 0, int(B), int(dv))
    st = stream if stream is not None else torch.cuda.current_stream(dev)
    check(lib().mcpx_vjp_batch_grouped_device(C.byref(desc), sh, int(sld), int(G), _ptr(off), *ptrs,
                                              _dev_f64(dvar, "dvar"), status.data_ptr(), C.c_void_p(st.cuda_stream)))
    return dvar, status


def vjp_batch_grouped_reduce(family: int, n: int, m: int, theta_shared, x, y, s, group_sizes, gx=None, gy=None,
                             gs=None, skip=None, num_devices: int = 0, want_dvar: bool = True) -> tuple:
    """vjp_batch_grouped plus every group's gradient of its matrix block summed over the group
    (mcpx_vjp_batch_grouped_reduce).  Returns (dshared (G, shared_dim), used (G,) int64, dvar
    (B, n + m) or None, status (B,)); dshared[g] and used[g] are the bits of vjp_batch_shared_reduce
    on group g alone (an empty group: +0.0 and 0)."""
    B = _batch_of(np.atleast_2d(np.asarray(x)), np.atleast_2d(np.asarray(y)), n, m)
    off = _group_offsets(group_sizes, B)
    G = off.size - 1
    sh, sld = _host_groups(family, n, m, theta_shared, G)
    ds, dv = _abi.theta_shared_dim(family, n, m), _abi.theta_var_dim(family, n, m)
    x, y, s = _host_f64(x, (B, n)), _host_f64(y, (B, m)), _host_f64(s, (B, m))
    gx, gy, gs = _host_f64(gx, (B, n)), _host_f64(gy, (B, m)), _host_f64(gs, (B, m))
    if skip is not None:
        skip = np.ascontiguousarray(np.broadcast_to(np.asarray(skip) != 0, (B,)), dtype=np.uint8)
    dshared = np.empty((G, ds))
    used = np.zeros(max(G, 1), np.int64)
    dvar = np.empty((B, dv)) if want_dvar else None
    st = np.empty(B, np.int32)
    desc = _abi.Desc(int(family), int(n), int(m), 0, int(B), int(dv))
    check(lib().mcpx_vjp_batch_grouped_reduce(C.byref(desc), _ptr(sh), int(sld), int(G), _ptr(off), _ptr(x), _ptr(y),
                                              _ptr(s), _ptr(gx), _ptr(gy), _ptr(gs), _ptr(skip), int(num_devices),
                                              dshared.ctypes.data, int(ds), _ptr(used), _ptr(dvar), _ptr(st)))
    return dshared, used[:G], dvar, st


def vjp_batch_grouped_reduce_device(family: int, n: int, m: int, theta_shared, x, y, s, group_sizes, gx=None,
                                    gy=None, gs=None, skip=None, dshared=None, used=None, dvar=None, status=None,
                                    want_dvar: bool = True, stream=None):
    """Device-tensor form, enqueued on the current stream (no sync).  Returns (dshared
    (G, shared_dim), used (G,) int64, dvar (B, n + m) or None, status (B,) int32) tensors."""
    import torch

    B = _batch_of(x, y, n, m)
    off = _group_offsets(group_sizes, B)
    G = off.size - 1
    sh, sld = _dev_groups(family, n, m, theta_shared, G)
    ds, dv = _abi.theta_shared_dim(family, n, m), _abi.theta_var_dim(family, n, m)
    dev = theta_shared.device
    if dshared is None:
        dshared = torch.empty(G, ds, dtype=torch.float64, device=dev)
    if used is None:
        used = torch.empty(G, dtype=torch.int64, device=dev)
    if dvar is None and want_dvar:
        dvar = torch.empty(B, dv, dtype=torch.float64, device=dev)
    if status is None:
        status = torch.empty(B, dtype=torch.int32, device=dev)
    if skip is not None:
        if skip.dtype == torch.bool:
            skip = skip.view(torch.uint8)
        if not (skip.is_cuda and skip.dtype == torch.uint8 and skip.is_contiguous() and skip.numel() == B):
            raise ValueError("skip must be a contiguous (B,) uint8 or bool device tensor")
    if not (dshared.is_cuda and dshared.dtype == torch.float64 and tuple(dshared.shape) == (G, ds)
            and (G <= 1 or ds == 0 or (dshared.stride(1) == 1 and dshared.stride(0) >= ds))):
        raise ValueError("dshared must be a (G, shared_dim) float64 device tensor with contiguous rows")
    if not (used.is_cuda and used.dtype == torch.int64 and used.is_contiguous() and used.numel() == G):
        raise ValueError("used must be a contiguous (G,) int64 device tensor")
    dld = dshared.stride(0) if G > 1 and ds > 0 else ds
    ptrs = [_dev_f64(t, k) for t, k in ((x, "x"), (y, "y"), (s, "s"), (gx, "gx"), (gy, "gy"), (gs, "gs"))]
    desc = _abi.Desc(int(family), int(n), int(m), 0, int(B), int(dv))
    st = stream if stream is not None else torch.cuda.current_stream(dev)
    check(lib().mcpx_vjp_batch_grouped_reduce_device(
        C.byref(desc), sh, int(sld), int(G), _ptr(off), *ptrs, None if skip is None else skip.data_ptr(),
        dshared.data_ptr(), int(dld), used.data_ptr(), _dev_f64(dvar, "dvar"), status.data_ptr(),
        C.c_void_p(st.cuda_stream)))
    return dshared, used, dvar, status

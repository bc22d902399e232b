"""The full-θ entry points of include/mcpx.h called through ctypes with raw addresses, for
tests/test_buffer_contract_gpu.py and tests/helpers/contract_probe.py: θ at any stride, any
output NULL, outputs anywhere in a larger allocation, any stream.  mcp_amd/batch.py always
passes every output and the stride of a 2-D array, so it cannot say these things.

An address is an int (numpy: a.ctypes.data, torch: t.data_ptr()) or None for NULL."""

from __future__ import annotations

import ctypes as C

import numpy as np

from mcp_amd import _abi
from mcp_amd._lib import check, lib
from tests.helpers.contract_cases import FIELDS, FUSED_CT, module_of
from tests.test_sensitivity import _same

DTYPES = dict(x=np.float64, y=np.float64, s=np.float64, kkt_error=np.float64, eps=np.float64, outer_iters=np.int32,
              status=np.int32, newton_iters=np.int32, active_mask=np.uint64, alpha_trace=np.uint8, fail_reason=np.uint8)


def out_shapes(c, trace_len):
    """Shape of every mcpx_out array of a solve case (include/mcpx.h)."""
    B, n, m = c.B, c.n, c.m
    return dict(x=(B, n), y=(B, m), s=(B, m), kkt_error=(B,), eps=(B,), outer_iters=(B,), status=(B,),
                newton_iters=(B,), active_mask=(B, max(1, (m + 63) // 64)), alpha_trace=(B, trace_len, 2),
                fail_reason=(B,))


def sens_shape(c, kind):
    p = module_of(c).nl.p if c.module else _abi.theta_dim(c.family, c.n, c.m)
    return {"vjp": (c.B, p), "jvp": (c.B, c.K, c.N), "cond": (c.B,)}[kind]


def _handle(c):
    return module_of(c).module().handle if c.module else None


def solve(c, theta, ld, start, out, trace_len, *, device, stream=None, B=None, fused=None):
    """mcpx_solve_batch[_module][_device], or (fused = (dtheta, vjp_status) addresses)
    mcpx_solve_vjp_batch_device.  theta: address of instance 0, ld: its stride in doubles; start:
    {} or the addresses x0 / y0 / s0; out: field → address or None (alpha_trace None: no trace)."""
    L = lib()
    B = c.B if B is None else B
    desc = _abi.Desc(int(c.family), c.n, c.m, 0, int(B), int(ld))
    prm = _abi.make_params(**c.params)
    tl = trace_len if out.get("alpha_trace") else 0
    o = _abi.Out(*(out.get(k) for k in FIELDS[:9]), out.get("alpha_trace"), int(tl), 0, out.get("fail_reason"))
    w = [start.get(k) for k in ("x0", "y0", "s0")]
    h = _handle(c)
    if fused is not None:
        ct = _abi.Cotangent(*FUSED_CT, None, None, None)
        check(L.mcpx_solve_vjp_batch_device(C.byref(desc), theta, *w, C.byref(prm), C.byref(o), C.byref(ct), fused[0],
                                            fused[1], C.c_void_p(stream)))
    elif device:
        args = (C.byref(desc), theta, *w, C.byref(prm), C.byref(o), C.c_void_p(stream))
        check(L.mcpx_solve_batch_module_device(h, *args) if h else L.mcpx_solve_batch_device(*args))
    else:
        args = (C.byref(desc), theta, *w, C.byref(prm), 0, C.byref(o))
        check(L.mcpx_solve_batch_module(h, *args) if h else L.mcpx_solve_batch(*args))


def sens(c, kind, theta, ld, point, g, td, result, status, *, device, stream=None):
    """mcpx_{vjp,jvp,cond}_batch[_module][_device].  point: addresses (x, y, s); g: (gx, gy, gs)
    of the VJP; td: θ̇ of the JVP (c.K partials); result: dtheta / zdot / rcond; status or None."""
    L = lib()
    desc = _abi.Desc(int(c.family), c.n, c.m, 0, int(c.B), int(ld))
    h = _handle(c)
    head = (C.byref(desc), theta, *point)
    tail = (result, status, C.c_void_p(stream)) if device else (0, result, status)
    mid = {"vjp": tuple(g), "jvp": (int(c.K), td), "cond": ()}[kind]
    name = f"mcpx_{kind}_batch" + ("_module" if h else "") + ("_device" if device else "")
    fn = getattr(L, name)
    check(fn(h, *head, *mid, *tail) if h else fn(*head, *mid, *tail))


# ---------------------------------------------------------------- host buffers


def host_outputs(c, trace_len, absent=(), fill=None):
    """Fresh numpy arrays for every field not in `absent` (filled with the byte `fill`, if given)
    and their address dict."""
    arrays = {}
    for k, shp in out_shapes(c, trace_len).items():
        if k in absent or (k == "alpha_trace" and trace_len == 0):
            continue
        a = np.empty(shp, DTYPES[k])
        if fill is not None:
            a.view(np.uint8).fill(fill)
        arrays[k] = a
    return arrays, {k: a.ctypes.data for k, a in arrays.items()}


def host_solve(c, theta2d, start, trace_len, absent=(), fill=None):
    """mcpx_solve_batch[_module] on a (B, ld) host array; → the output arrays."""
    th = np.ascontiguousarray(theta2d)
    st = {k: np.ascontiguousarray(v) for k, v in start.items()}
    arrays, ptrs = host_outputs(c, trace_len, absent, fill)
    solve(c, th.ctypes.data, th.shape[1], {k: v.ctypes.data for k, v in st.items()}, ptrs, trace_len, device=False,
          B=th.shape[0])
    return arrays


def host_sens(c, kind, theta2d, point, g, td, want_status=True):
    """mcpx_{vjp,jvp,cond}_batch[_module] on a (B, ld) host array; → (result, status or None)."""
    th = np.ascontiguousarray(theta2d)
    keep = [None if a is None else np.ascontiguousarray(a) for a in (*point, *g, td)]
    at = [None if a is None else a.ctypes.data for a in keep]
    res = np.empty(sens_shape(c, kind))
    st = np.empty(c.B, np.int32) if want_status else None
    sens(c, kind, th.ctypes.data, th.shape[1], at[:3], at[3:6], at[6], res.ctypes.data,
         None if st is None else st.ctypes.data, device=False)
    return res, st


def host_stride_calls(oracle_lib):
    """Every host-entry call of the stride check, θ at stride p + pad with NaN padding: yields
    (label, number of output fields that differ from the oracle on the packed θ).  The case that
    needs MCPX_GENERIC_KERNELS is left to its own test (the variable is the caller's to set)."""
    from tests.helpers import contract_cases as cc

    for c in cc.SOLVE_CASES:
        if c.generic:
            continue
        th, start = c.inputs()
        got = host_solve(c, cc.padded(th, c.pad), start, cc.TRACE)
        yield c.id, len(cc.solve_mismatches(got, cc.oracle_solve(oracle_lib, c)))
    for c in cc.SENS_CASES:
        th, g, td = c.inputs()
        r = cc.oracle_point(oracle_lib, c)
        for kind in c.kinds:
            res, st = host_sens(c, kind, cc.padded(th, c.pad), (r["x"], r["y"], r["s"]), g, td)
            ref, rst = cc.oracle_sens(oracle_lib, c, kind)
            yield f"{c.id}-{kind}", int(not _same(res, ref)) + int(not _same(st, rst))


def tight(theta_packed, ld):
    """θ in a flat host buffer of exactly (B − 1)·ld + p doubles, NaN between the instances: the
    allocation ends with the last instance (include/mcpx.h, Conventions)."""
    B, p = theta_packed.shape
    flat = np.full((B - 1) * ld + p, np.nan)
    for b in range(B):
        flat[b * ld:b * ld + p] = theta_packed[b]
    return flat

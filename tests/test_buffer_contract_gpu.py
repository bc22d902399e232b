"""The buffer contract of include/mcpx.h on the full-θ entry points: mcpx_solve_batch[_device],
mcpx_solve_vjp_batch_device, mcpx_{vjp,jvp,cond}_batch[_device] and their _module forms, at the
smallest shape that reaches each kernel family (tests/helpers/contract_cases.py; the table and
its inputs are checked on the CPU in tests/test_buffer_contract.py).

The reference throughout is the oracle on the PACKED θ, compared bit for bit on every field of
every instance (assert_parity and the field-by-field report for solves, _same for sensitivities).

  (a) stride    θ at stride p + pad (pad 1 or 3, so a row's 16-byte parity flips for even and odd
                p) with NaN padding, through the device and the host entry; the host pipeline's
                chunk and shard offsets and the sensitivities' shards under padding; θ in a buffer
                that ends with its last instance; and the QP SCHUR fast pass on a θ whose
                misplaced window passes the kernel's symmetry check (NaN padding alone lets the
                two-pass protocol repair a wrong instance pointer: the instance is deferred).
  (b) extent    every output a contiguous interior slice of a larger device tensor, one element of
                its own type in front (natural alignment only), everything filled with 0xA5: the
                guards survive, every entry of a non-trace array is written, the α trace is written
                where the oracle recorded a step and nowhere else.
  (c) optional  each of newton_iters / active_mask / alpha_trace / fail_reason NULL alone, all four
                NULL; status NULL on the sensitivities; device and host entry.
  (d) stream    inputs produced on a side stream, the call on that stream, outputs read after
                synchronising that stream only; two calls back to back on two side streams.
  (e) blocks    the host-entry calls of (a) in a child process under MCPX_POISON=1: the library's
                own blocks NaN-filled with canaries behind them."""

from __future__ import annotations

import json
import os
import subprocess
import sys
from dataclasses import replace

import numpy as np
import pytest

from tests.helpers import contract_calls as calls
from tests.helpers import contract_cases as cc
from tests.test_gpu_parity import assert_parity
from tests.test_sensitivity import _same

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROBE = os.path.join(ROOT, "tests", "helpers", "contract_probe.py")
FILL = cc.FILL


def _ids(cases):
    return [pytest.param(c, id=c.id) for c in cases]


def _by(**kw):
    return next(c for c in cc.SOLVE_CASES + cc.FUSED if all(getattr(c, k) == v for k, v in kw.items()))


def _sens_by(**kw):
    return next(c for c in cc.SENS_CASES if all(getattr(c, k) == v for k, v in kw.items()))


def _env(case, monkeypatch):
    if getattr(case, "generic", False):
        monkeypatch.setenv("MCPX_GENERIC_KERNELS", "1")  # read at every call


# ---------------------------------------------------------------- device buffers


def _dev():
    import torch

    return torch.device("cuda", 0)


def up(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).to(_dev())


class Guarded:
    """An output array as a contiguous interior slice of a larger device tensor: `front` elements
    of its own type before it (1: the array keeps its natural alignment and no more), `back`
    behind, every byte FILL."""

    def __init__(self, shape, dtype, front=1, back=3):
        import torch

        self.shape, self.dtype = tuple(shape), np.dtype(dtype)
        item = self.dtype.itemsize
        count = int(np.prod(self.shape))
        self.lo, self.hi = front * item, (front + count) * item
        self.raw = torch.full(((front + count + back) * item,), FILL, dtype=torch.uint8, device=_dev())
        self.ptr = self.raw.data_ptr() + self.lo
        assert self.raw.data_ptr() % 64 == 0 and self.ptr % item == 0

    def read(self):
        """(the array on the host, True when every guard byte still holds FILL)."""
        b = self.raw.cpu().numpy()
        intact = bool((b[:self.lo] == FILL).all() and (b[self.hi:] == FILL).all())
        return b[self.lo:self.hi].copy().view(self.dtype).reshape(self.shape), intact


def unwritten(a):
    """Entries of `a` that still hold the fill pattern in every byte."""
    item = a.dtype.itemsize
    return int((np.ascontiguousarray(a).view(np.uint8).reshape(-1, item) == FILL).all(axis=1).sum())


def device_outputs(c, trace_len, absent=()):
    return {k: Guarded(shp, calls.DTYPES[k]) for k, shp in calls.out_shapes(c, trace_len).items()
            if k not in absent and not (k == "alpha_trace" and trace_len == 0)}


def read_outputs(bufs):
    """(field → host array, names of the fields whose guards were overwritten)."""
    got, broken = {}, []
    for k, g in bufs.items():
        got[k], intact = g.read()
        if not intact:
            broken.append(k)
    return got, broken


def device_solve(c, theta2d, start, bufs, trace_len=cc.TRACE, stream=None, fused=None):
    """The device solve entry of the case on θ (B, ld) (a host array, uploaded here) into the
    Guarded outputs `bufs`; returns the device inputs, which must outlive the call."""
    th = up(theta2d)
    st = {k: up(v) for k, v in start.items()}
    calls.solve(c, th.data_ptr(), th.shape[1], {k: v.data_ptr() for k, v in st.items()},
                {k: g.ptr for k, g in bufs.items()}, trace_len, device=True, stream=stream,
                fused=None if fused is None else (fused[0].ptr, None if fused[1] is None else fused[1].ptr))
    return th, st


def fused_outputs(c, want_status=True):
    return (Guarded((c.B, cc.theta_p(c)), np.float64), Guarded((c.B,), np.int32) if want_status else None)


def check_solve(got, ref, untouched, absent=()):
    bad = cc.solve_mismatches(got, ref, untouched=untouched, absent=absent)
    assert not bad, f"fields that differ from the oracle on the packed θ: {bad}"
    if not absent:  # the suite's own comparison as well
        assert_parity(got, dict(ref, alpha_trace=cc.expected_trace(ref, untouched)))
    for k in ("x", "y", "s", "kkt_error", "eps"):  # no NaN where the oracle has none: the padding was not read
        assert not (np.isnan(got[k]) & ~np.isnan(ref[k])).any(), k


def check_fused(oracle_lib, c, fb):
    _, rdth, rst = cc.oracle_fused(oracle_lib, c)
    dth, ok = fb[0].read()
    assert ok and unwritten(dth) == 0 and _same(dth, rdth)
    if fb[1] is not None:
        st, ok = fb[1].read()
        assert ok and unwritten(st) == 0 and _same(st, rst)


def device_sens(c, kind, theta2d, point, g, td, want_status=True, stream=None):
    """The device sensitivity entry on θ (B, ld) into Guarded outputs → (result, status or None,
    guards intact)."""
    import torch

    th = up(theta2d)
    keep = [up(a) for a in (*point, *g, td)]
    res = Guarded(calls.sens_shape(c, kind), np.float64)
    st = Guarded((c.B,), np.int32) if want_status else None
    at = [t.data_ptr() for t in keep]
    calls.sens(c, kind, th.data_ptr(), th.shape[1], at[:3], at[3:6], at[6], res.ptr, None if st is None else st.ptr,
               device=True, stream=stream)
    torch.cuda.synchronize()
    r, ok = res.read()
    s, ok2 = st.read() if st is not None else (None, True)
    return r, s, ok and ok2


def sens_inputs(oracle_lib, c):
    th, g, td = c.inputs()
    r = cc.oracle_point(oracle_lib, c)
    return th, (r["x"], r["y"], r["s"]), g, td


# ---------------------------------------------------------------- (a) stride, (b) extent: solves


@pytest.mark.parametrize("case", _ids(cc.SOLVE_CASES))
def test_stride_and_extent_device_solve(gpu, oracle_lib, case, monkeypatch):
    """(a) and (b) through mcpx_solve_batch[_module]_device: θ at stride p + pad with NaN padding,
    every output a guarded interior slice filled with 0xA5."""
    import torch

    _env(case, monkeypatch)
    th, start = case.inputs()
    ref = cc.oracle_solve(oracle_lib, case)
    bufs = device_outputs(case, cc.TRACE)
    keep = device_solve(case, cc.padded(th, case.pad), start, bufs)
    torch.cuda.synchronize()
    got, broken = read_outputs(bufs)
    assert not broken, f"written outside the array: {broken}"
    for k in cc.FIELDS:
        if k != "alpha_trace":
            assert unwritten(got[k]) == 0, f"{k}: entries never written"
    check_solve(got, ref, untouched=FILL)  # the trace: the oracle's steps, the fill everywhere else
    del keep


@pytest.mark.parametrize("case", _ids(cc.SOLVE_CASES))
def test_stride_host_solve(gpu, oracle_lib, case, monkeypatch):
    """(a) through mcpx_solve_batch[_module]: the same padded θ from host memory."""
    _env(case, monkeypatch)
    th, start = case.inputs()
    got = calls.host_solve(case, cc.padded(th, case.pad), start, cc.TRACE, fill=FILL)
    for k in cc.FIELDS:
        if k != "alpha_trace":
            assert unwritten(got[k]) == 0, f"{k}: entries never written"
    check_solve(got, cc.oracle_solve(oracle_lib, case), untouched=254)


@pytest.mark.parametrize("case", _ids(cc.FUSED))
def test_stride_and_extent_fused(gpu, oracle_lib, case):
    """(a) and (b) through mcpx_solve_vjp_batch_device (the epilogue kernel at (32, 16) SCHUR,
    solve then pullback at (5, 3) REDUCED): the solve record, dtheta and vjp_status."""
    import torch

    th, start = case.inputs()
    bufs, fb = device_outputs(case, cc.TRACE), fused_outputs(case)
    keep = device_solve(case, cc.padded(th, case.pad), start, bufs, fused=fb)
    torch.cuda.synchronize()
    got, broken = read_outputs(bufs)
    assert not broken, f"written outside the array: {broken}"
    for k in cc.FIELDS:
        if k != "alpha_trace":
            assert unwritten(got[k]) == 0, f"{k}: entries never written"
    check_solve(got, cc.oracle_solve(oracle_lib, case), untouched=FILL)
    check_fused(oracle_lib, case, fb)
    del keep


@pytest.mark.parametrize("n,m,pad", [(16, 8, 1), (32, 16, 3), (32, 16, 1), (2, 2, 3), (5, 3, 1), (4, 3, 3)])
def test_fast_pass_stride_where_pass_two_cannot_heal(gpu, oracle_lib, n, m, pad):
    """The QP SCHUR fast pass on a θ whose misplaced window is symmetric too (M = c·𝟙𝟙ᵀ, padding
    c; contract_cases.shift_blind_qp).  With NaN padding an instance pointer formed with p instead
    of theta_ld makes the fast pass see a non-symmetric M and defer the instance to pass 2, which
    reads the right address: the outputs are right and only the time is lost.  Here the fast pass
    keeps such an instance and its numbers show.  Device and host entry, every instance solved."""
    import torch

    case = replace(_by(family=cc.QP, solver="schur", n=n, m=m, generic=False, fused=False, asym=False), B=5, warm=False)
    th, wide = cc.shift_blind_qp(n, m, case.B, pad)
    ref = oracle_lib.solve_batch(cc.QP, n, m, th, trace_len=cc.TRACE, **case.params)
    assert (ref["status"] == 0).all()
    bufs = device_outputs(case, cc.TRACE)
    keep = device_solve(case, wide, {}, bufs)
    torch.cuda.synchronize()
    got, broken = read_outputs(bufs)
    assert not broken
    check_solve(got, ref, untouched=FILL)
    check_solve(calls.host_solve(case, wide, {}, cc.TRACE, fill=FILL), ref, untouched=254)
    # the fused call's fast pass (its own instantiation, pullback in the epilogue)
    fcase = replace(case, fused=True)
    ax, ay, _ = cc.FUSED_CT
    rdth, rst = oracle_lib.vjp_batch(cc.QP, n, m, th, ref["x"], ref["y"], ref["s"], ax * ref["x"], ay * ref["y"], None)
    bufs, fb = device_outputs(fcase, cc.TRACE), fused_outputs(fcase)
    keep2 = device_solve(fcase, wide, {}, bufs, fused=fb)
    torch.cuda.synchronize()
    got, broken = read_outputs(bufs)
    assert not broken
    check_solve(got, ref, untouched=FILL)
    (dth, ok), (st, ok2) = fb[0].read(), fb[1].read()
    assert ok and ok2 and _same(st, rst) and _same(dth, rdth)
    del keep, keep2


# ---------------------------------------------------------------- (a), (b): sensitivities


@pytest.mark.parametrize("case", _ids(cc.SENS_CASES))
def test_stride_and_extent_sensitivities(gpu, oracle_lib, case):
    """vjp, jvp (K = 9) and cond on θ at stride p + pad with NaN padding: the device entry into
    guarded outputs, then the host entry."""
    th, point, g, td = sens_inputs(oracle_lib, case)
    wide = cc.padded(th, case.pad)
    for kind in case.kinds:
        ref, rst = cc.oracle_sens(oracle_lib, case, kind)
        res, st, intact = device_sens(case, kind, wide, point, g, td)
        assert intact, f"{kind}: written outside the array"
        assert unwritten(res) == 0 and unwritten(st) == 0, kind
        assert _same(st, rst) and _same(res, ref), f"device {kind}"
        assert not np.isnan(res).any(), kind
        res, st = calls.host_sens(case, kind, wide, point, g, td)
        assert _same(st, rst) and _same(res, ref), f"host {kind}"


def test_sensitivities_host_shards_under_padding(gpu, oracle_lib, monkeypatch):
    """The host VJP, JVP and cond at (16, 8) as three shards (offsets b0·theta_ld into padded θ)."""
    monkeypatch.setenv("MCPX_HOST_SHARDS", "3")  # read at every call
    case = _sens_by(family=cc.QP, n=16, m=8)
    th, point, g, td = sens_inputs(oracle_lib, case)
    for kind in case.kinds:
        ref, rst = cc.oracle_sens(oracle_lib, case, kind)
        res, st = calls.host_sens(case, kind, cc.padded(th, 3), point, g, td)
        assert _same(st, rst) and _same(res, ref), kind


@pytest.mark.parametrize("knob", ["chunks", "shards"])
def test_host_pipeline_under_padding(gpu, oracle_lib, knob, monkeypatch):
    """(6, 4) SCHUR, B = 2·1024 + 5 at stride p + 3: three chunks of the pipeline under
    MCPX_HOST_CHUNK=1024, then three shards as well — every chunk and shard offset is a multiple
    of theta_ld, not of p."""
    monkeypatch.setenv("MCPX_HOST_CHUNK", "1024")
    if knob == "shards":
        monkeypatch.setenv("MCPX_HOST_SHARDS", "3")
    case = replace(_by(family=cc.AFFINE, solver="schur", n=6, m=4), B=2 * 1024 + 5)
    th, start = case.inputs()
    got = calls.host_solve(case, cc.padded(th, 3), start, cc.TRACE, fill=FILL)
    check_solve(got, cc.oracle_solve(oracle_lib, case), untouched=254)


def test_tight_buffers(gpu, oracle_lib):
    """θ in a flat host buffer of exactly (B − 1)·ld + p doubles, through ctypes: one solve, one
    VJP, one JVP, one cond.  (That the library reads nothing behind the last instance is fixed in
    the host layer from its code — strided_span — and cannot be shown without a fault; this checks
    the results of such a call.)"""
    case = _by(family=cc.QP, solver="reduced", n=4, m=3)  # p = 35
    th, start = case.inputs()
    ld = th.shape[1] + 3
    flat = calls.tight(th, ld)
    assert flat.size == (case.B - 1) * ld + th.shape[1]
    st = {k: np.ascontiguousarray(v) for k, v in start.items()}
    arrays, ptrs = calls.host_outputs(case, cc.TRACE, fill=FILL)
    calls.solve(case, flat.ctypes.data, ld, {k: v.ctypes.data for k, v in st.items()}, ptrs, cc.TRACE, device=False)
    check_solve(arrays, cc.oracle_solve(oracle_lib, case), untouched=254)

    sc = _sens_by(family=cc.QP, n=16, m=8)
    th, point, g, td = sens_inputs(oracle_lib, sc)
    ld = th.shape[1] + 1
    flat = calls.tight(th, ld)
    keep = [np.ascontiguousarray(a) for a in (*point, *g, td)]
    at = [a.ctypes.data for a in keep]
    for kind in sc.kinds:
        res, stt = np.empty(calls.sens_shape(sc, kind)), np.empty(sc.B, np.int32)
        calls.sens(sc, kind, flat.ctypes.data, ld, at[:3], at[3:6], at[6], res.ctypes.data, stt.ctypes.data,
                   device=False)
        ref, rst = cc.oracle_sens(oracle_lib, sc, kind)
        assert _same(stt, rst) and _same(res, ref), kind


# ---------------------------------------------------------------- (c) optional outputs

OPTIONAL_CASES = (_by(family=cc.QP, solver="schur", n=32, m=16, generic=False, fused=False),
                  _by(family=cc.QP, solver="dense", n=5, m=3),
                  _by(family=cc.QP, solver="reduced", n=40, m=30),
                  _by(module="lane", kernel="band"),
                  _by(fused=True, n=32, m=16))
ABSENT = tuple((k,) for k in cc.OPTIONAL) + (cc.OPTIONAL,)


@pytest.mark.parametrize("absent", [pytest.param(a, id="all" if len(a) > 1 else a[0]) for a in ABSENT])
@pytest.mark.parametrize("case", _ids(OPTIONAL_CASES))
def test_optional_outputs_null(gpu, oracle_lib, case, absent):
    """The NULL paths of the kernels (device entry) and of the host pipeline (host entry): the
    remaining fields are the oracle's bits."""
    import torch

    th, start = case.inputs()
    ref = cc.oracle_solve(oracle_lib, case)
    tl = 0 if "alpha_trace" in absent else cc.TRACE
    bufs = device_outputs(case, tl, absent)
    fb = fused_outputs(case) if case.fused else None
    keep = device_solve(case, th, start, bufs, trace_len=tl, fused=fb)
    torch.cuda.synchronize()
    got, broken = read_outputs(bufs)
    assert not broken and set(got) == set(cc.FIELDS) - set(absent)
    check_solve(got, ref, untouched=FILL, absent=absent)
    if case.fused:
        check_fused(oracle_lib, case, fb)
        return  # the fused call has no host entry
    got = calls.host_solve(case, th, start, tl, absent=absent, fill=FILL)
    assert set(got) == set(cc.FIELDS) - set(absent)
    check_solve(got, ref, untouched=254, absent=absent)
    del keep


@pytest.mark.parametrize("case", _ids(cc.SENS_CASES))
def test_sensitivity_status_null(gpu, oracle_lib, case):
    th, point, g, td = sens_inputs(oracle_lib, case)
    for kind in case.kinds:
        ref, _ = cc.oracle_sens(oracle_lib, case, kind)
        res, st, intact = device_sens(case, kind, th, point, g, td, want_status=False)
        assert st is None and intact and _same(res, ref), f"device {kind}"
        res, st = calls.host_sens(case, kind, th, point, g, td, want_status=False)
        assert st is None and _same(res, ref), f"host {kind}"


def test_fused_vjp_status_null(gpu, oracle_lib):
    import torch

    case = _by(fused=True, n=32, m=16)
    th, start = case.inputs()
    bufs, fb = device_outputs(case, cc.TRACE), fused_outputs(case, want_status=False)
    keep = device_solve(case, th, start, bufs, fused=fb)
    torch.cuda.synchronize()
    got, broken = read_outputs(bufs)
    assert not broken
    check_solve(got, cc.oracle_solve(oracle_lib, case), untouched=FILL)
    check_fused(oracle_lib, case, fb)
    del keep


# ---------------------------------------------------------------- (d) stream

STREAM_CASES = (replace(_by(family=cc.QP, solver="schur", n=32, m=16, generic=False, fused=False), asym=True),
                _by(family=cc.QP, solver="reduced", n=40, m=30),
                _by(fused=True, n=32, m=16))


def _stage(arrays):
    """(staged, dest) device tensors on the default stream: the data, and where a copy enqueued on
    a side stream will produce it.  Nothing here is ordered against a side stream: synchronise
    the device before _produce."""
    import torch

    staged = [up(a) for a in arrays]
    return staged, [torch.empty_like(t) for t in staged]


def _produce(stream, staged, dest):
    """Enqueue the device-to-device copies that produce the inputs ON `stream`; no synchronisation."""
    import torch

    with torch.cuda.stream(stream):
        for t, d in zip(staged, dest):
            d.copy_(t, non_blocking=True)
    return dest


def _prepare(case):
    """Everything a call of the case needs before it is enqueued: the inputs staged, every Guarded
    output allocated and filled (default stream).  The caller synchronises the device once."""
    th, start = case.inputs()
    names = list(start)
    staged, dest = _stage([cc.padded(th, case.pad)] + [start[k] for k in names])
    return dict(case=case, names=names, staged=staged, dest=dest, bufs=device_outputs(case, cc.TRACE),
                fb=fused_outputs(case) if case.fused else None)


def _enqueue(stream, job):
    """The inputs produced on `stream`, then the library call on it; returns without any
    device or stream synchronisation."""
    case, fb = job["case"], job["fb"]
    dev_in = _produce(stream, job["staged"], job["dest"])
    calls.solve(case, dev_in[0].data_ptr(), dev_in[0].shape[1],
                {k: t.data_ptr() for k, t in zip(job["names"], dev_in[1:])}, {k: g.ptr for k, g in job["bufs"].items()},
                cc.TRACE, device=True, stream=stream.cuda_stream, fused=None if fb is None else (fb[0].ptr, fb[1].ptr))


def _check_stream_result(oracle_lib, case, bufs, fb):
    got, broken = read_outputs(bufs)
    assert not broken
    check_solve(got, cc.oracle_solve(oracle_lib, case), untouched=FILL)
    if fb is not None:
        check_fused(oracle_lib, case, fb)


@pytest.mark.parametrize("case", _ids(STREAM_CASES))
def test_solve_on_a_side_stream(gpu, oracle_lib, case):
    """Both passes of the (32, 16) SCHUR protocol, the workgroup kernels' work queue and the fused
    call: every copy, memset and launch of the library must be ordered on the caller's stream."""
    import torch

    cc.oracle_solve(oracle_lib, case)  # before anything is enqueued
    s = torch.cuda.Stream(_dev())
    job = _prepare(case)
    torch.cuda.synchronize()
    _enqueue(s, job)
    s.synchronize()  # that stream only
    _check_stream_result(oracle_lib, case, job["bufs"], job["fb"])


def test_vjp_on_a_side_stream(gpu, oracle_lib):
    import torch

    case = _sens_by(family=cc.QP, n=16, m=8)
    th, point, g, td = sens_inputs(oracle_lib, case)
    ref, rst = cc.oracle_sens(oracle_lib, case, "vjp")
    s = torch.cuda.Stream(_dev())
    res, st = Guarded(calls.sens_shape(case, "vjp"), np.float64), Guarded((case.B,), np.int32)
    staged, dest = _stage([cc.padded(th, case.pad), *point, *g])
    torch.cuda.synchronize()
    dev_in = _produce(s, staged, dest)
    at = [t.data_ptr() for t in dev_in]
    calls.sens(case, "vjp", at[0], dev_in[0].shape[1], at[1:4], at[4:7], None, res.ptr, st.ptr, device=True,
               stream=s.cuda_stream)
    s.synchronize()
    (r, ok), (sv, ok2) = res.read(), st.read()
    assert ok and ok2 and _same(sv, rst) and _same(r, ref)


def test_two_calls_on_two_side_streams(gpu, oracle_lib):
    """Four calls in flight on two side streams, separate outputs: the two-pass SCHUR solve and
    the workgroup solve on s1 / s2, then swapped.  Every input is staged and every output filled
    first and the device synchronised once; the copies that produce the inputs and the four
    library calls are then enqueued with no device or stream synchronisation between them, and
    s1 and s2 are synchronised at the end.  What two calls share — the library's block cache
    (a block released on one stream and taken on the other), the work queue's counter, the
    deferred-instance marks in status — must be per call or ordered by the library itself."""
    import torch

    a, b = STREAM_CASES[0], STREAM_CASES[1]
    for c in (a, b):
        cc.oracle_solve(oracle_lib, c)
    s1, s2 = torch.cuda.Stream(_dev()), torch.cuda.Stream(_dev())
    plan = [(s1, _prepare(a)), (s2, _prepare(b)), (s1, _prepare(b)), (s2, _prepare(a))]
    torch.cuda.synchronize()  # the only device-wide synchronisation, before the first enqueue
    for s, job in plan:
        _enqueue(s, job)
    s1.synchronize()
    s2.synchronize()
    for _, job in plan:
        _check_stream_result(oracle_lib, job["case"], job["bufs"], job["fb"])


def test_optional_outputs_through_the_python_hooks(gpu, oracle_lib):
    """The device entry as mcp_amd.batch offers the NULL outputs: alloc_device_outputs(newton=False,
    active=False), out["fail_reason"] = None and trace_len = 0 — all four optional pointers NULL
    through solve_batch_device; the required fields are the oracle's bits."""
    import torch

    from mcp_amd.batch import alloc_device_outputs, solve_batch_device

    case = _by(family=cc.QP, solver="schur", n=32, m=16, generic=False, fused=False)
    th, start = case.inputs()
    out = alloc_device_outputs(case.B, case.n, case.m, _dev(), trace_len=0, newton=False, active=False)
    out["fail_reason"] = None
    assert all(out[k] is None for k in cc.OPTIONAL)
    for k in cc.FIELDS:
        if k not in cc.OPTIONAL:
            out[k].view(torch.uint8).fill_(FILL)
    solve_batch_device(case.family, case.n, case.m, up(cc.padded(th, case.pad)), out,
                       **{k: up(v) for k, v in start.items()}, **case.params)
    torch.cuda.synchronize()
    got = {k: v.cpu().numpy() for k, v in out.items() if v is not None}
    assert set(got) == set(cc.FIELDS) - set(cc.OPTIONAL)
    check_solve(got, cc.oracle_solve(oracle_lib, case), untouched=FILL, absent=cc.OPTIONAL)


# ---------------------------------------------------------------- (e) library blocks under padding


def test_library_blocks_under_padding(gpu):
    """The host-entry calls of (a) in a child process with MCPX_POISON=1 and nothing else set:
    the library's θ buffers are NaN beyond what it uploads — the padding of every row and the
    stride's remainder behind a chunk's last instance — and carry a canary.  Every call is the
    oracle's bits and no canary is touched."""
    env = {k: v for k, v in os.environ.items() if k != "PYTHONPATH"}
    env["MCPX_POISON"] = "1"
    p = subprocess.run([sys.executable, "-u", PROBE], capture_output=True, text=True, timeout=300, env=env, cwd=ROOT)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    assert "MCPX_POISON canary" not in p.stderr, p.stderr[-2000:]
    rows = [json.loads(line) for line in p.stdout.splitlines() if line.startswith("{")]
    want = sum(1 for c in cc.SOLVE_CASES if not c.generic) + sum(len(c.kinds) for c in cc.SENS_CASES)
    assert len(rows) == want
    assert all(r["differ"] == 0 and r["canary"] == 0 for r in rows), [r for r in rows if r["differ"] or r["canary"]]

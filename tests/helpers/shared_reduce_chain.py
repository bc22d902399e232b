"""Test-side restatement of the contract of mcpx_vjp_batch_shared_reduce (include/mcpx.h): per
chunk of MCPX_REDUCE_CHUNK instances and entry an fma chain from +0.0 over the instances in ascending order
(an excluded instance's operands replaced by +0.0), then the chunk partials added in ascending
order from +0.0.  The chunk length is the header's MCPX_REDUCE_CHUNK (mcp_amd._abi.REDUCE_CHUNK).  Two independent forms:

* `chain_c(tmp_dir)`: a few lines of C compiled with `gcc -O2 -ffp-contract=off` (fma from libm);
* `chain_fraction`: exact rational arithmetic, fma(a, b, c) = float(a·b + c) — float() of a
  Fraction is correctly rounded.  Slow: small cases only.

Both: chain(family, n, m, x (B, n), y (B, m), dvar (B, n + m), include (B,) bool) → (shared_dim,)."""

from __future__ import annotations

import ctypes as C
import os
import shutil
import subprocess
from fractions import Fraction

import numpy as np

from mcp_amd import _abi

CHUNK = _abi.REDUCE_CHUNK  # MCPX_REDUCE_CHUNK

SOURCE = r"""
#include <math.h>
#include <stdlib.h>
/* operands of an excluded instance: +0.0 (also the negated ones) */
int chain(int family, int n, int m, long B, const double* x, const double* y, const double* dv,
          const unsigned char* inc, long CHUNK, double* out) {
  const long nn = (long)n * n, nm = (long)n * m, vd = n + m;
  const long ds = family == 0 ? nn + nm : nn + 2 * nm + (long)m * m;
  double* P = (double*)malloc(sizeof(double) * (ds > 0 ? ds : 1));
  if (!P) return 1;
  for (long e = 0; e < ds; ++e) out[e] = 0.0;
  for (long c0 = 0; c0 < B; c0 += CHUNK) {
    const long c1 = c0 + CHUNK < B ? c0 + CHUNK : B;
    for (long e = 0; e < ds; ++e) P[e] = 0.0;
    for (long b = c0; b < c1; ++b) {
      const int on = inc[b] != 0;
      const double *xb = x + b * n, *yb = y + b * m, *d = dv + b * vd;
#define X(j) (on ? xb[j] : 0.0)
#define Y(k) (on ? yb[k] : 0.0)
      if (family == 0) { /* d = [ly (m); lx (n)] */
#define LX(i) (on ? d[m + (i)] : 0.0)
#define NLX(i) (on ? -d[m + (i)] : 0.0)
#define NLY(k) (on ? -d[k] : 0.0)
        for (int j = 0; j < n; ++j)
          for (int i = 0; i < n; ++i) P[i + (long)n * j] = fma(NLX(i), X(j), P[i + (long)n * j]);
        for (int j = 0; j < n; ++j)
          for (int k = 0; k < m; ++k) {
            double acc = P[nn + k + (long)m * j];
            acc = fma(NLY(k), X(j), acc);
            acc = fma(LX(j), Y(k), acc);
            P[nn + k + (long)m * j] = acc;
          }
      } else { /* d = [dg (n); dh (m)] */
#define DG(i) (on ? d[i] : 0.0)
#define DH(k) (on ? d[n + (k)] : 0.0)
        for (int j = 0; j < n; ++j)
          for (int i = 0; i < n; ++i) P[i + (long)n * j] = fma(DG(i), X(j), P[i + (long)n * j]);
        for (int k = 0; k < m; ++k)
          for (int i = 0; i < n; ++i) P[nn + i + (long)n * k] = fma(DG(i), Y(k), P[nn + i + (long)n * k]);
        for (int j = 0; j < n; ++j)
          for (int k = 0; k < m; ++k) P[nn + nm + k + (long)m * j] = fma(DH(k), X(j), P[nn + nm + k + (long)m * j]);
        for (int q = 0; q < m; ++q)
          for (int k = 0; k < m; ++k)
            P[nn + 2 * nm + k + (long)m * q] = fma(DH(k), Y(q), P[nn + 2 * nm + k + (long)m * q]);
      }
    }
    for (long e = 0; e < ds; ++e) out[e] = out[e] + P[e];
  }
  free(P);
  return 0;
}
"""


def shared_dim(family: int, n: int, m: int) -> int:
    return n * n + m * n if family == 0 else n * n + 2 * n * m + m * m


def _args(family, n, m, x, y, dvar, include):
    x = np.ascontiguousarray(x, np.float64).reshape(-1, n)
    B = x.shape[0] if n > 0 else np.asarray(y).reshape(-1, m).shape[0]
    y = np.ascontiguousarray(y, np.float64).reshape(B, m)
    dvar = np.ascontiguousarray(dvar, np.float64).reshape(B, n + m)
    inc = np.ones(B, bool) if include is None else np.asarray(include, bool).reshape(B)
    return B, x.reshape(B, n), y, dvar, inc


def chain_c(tmp_dir):
    """The C form, compiled into tmp_dir; None when there is no gcc."""
    gcc = shutil.which("gcc")
    if gcc is None:
        return None
    src, lib = os.path.join(str(tmp_dir), "reduce_chain.c"), os.path.join(str(tmp_dir), "reduce_chain.so")
    with open(src, "w") as f:
        f.write(SOURCE)
    subprocess.run([gcc, "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-o", lib, src, "-lm"], check=True)
    fn = C.CDLL(lib).chain
    fn.restype = C.c_int
    P = C.c_void_p
    fn.argtypes = [C.c_int, C.c_int, C.c_int, C.c_long, P, P, P, P, C.c_long, P]

    def chain(family, n, m, x, y, dvar, include=None):
        B, x, y, dvar, inc = _args(family, n, m, x, y, dvar, include)
        inc8 = np.ascontiguousarray(inc, np.uint8)
        out = np.full(shared_dim(family, n, m), np.nan)
        rc = fn(family, n, m, B, x.ctypes.data, y.ctypes.data, dvar.ctypes.data, inc8.ctypes.data, CHUNK,
                out.ctypes.data)
        assert rc == 0
        return out

    return chain


def fma(a: float, b: float, c: float) -> float:
    """Correctly rounded a·b + c of finite doubles (an exact zero comes out as +0.0)."""
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def chain_fraction(family, n, m, x, y, dvar, include=None):
    B, x, y, dvar, inc = _args(family, n, m, x, y, dvar, include)
    nn, nm = n * n, n * m
    out = np.zeros(shared_dim(family, n, m))
    for c0 in range(0, B, CHUNK):
        P = np.zeros_like(out)
        for b in range(c0, min(B, c0 + CHUNK)):
            z = (lambda v: float(v)) if inc[b] else (lambda v: 0.0)
            X, Y = [z(v) for v in x[b]], [z(v) for v in y[b]]
            if family == 0:
                lx = [z(v) for v in dvar[b, m:]]  # dvar = [λy (m); λx (n)]
                nlx, nly = [z(-v) for v in dvar[b, m:]], [z(-v) for v in dvar[b, :m]]
                for j in range(n):
                    for i in range(n):
                        P[i + n * j] = fma(nlx[i], X[j], P[i + n * j])
                    for k in range(m):
                        e = nn + k + m * j
                        P[e] = fma(lx[j], Y[k], fma(nly[k], X[j], P[e]))
            else:
                dg, dh = [z(v) for v in dvar[b, :n]], [z(v) for v in dvar[b, n:]]
                for j in range(n):
                    for i in range(n):
                        P[i + n * j] = fma(dg[i], X[j], P[i + n * j])
                    for k in range(m):
                        P[nn + nm + k + m * j] = fma(dh[k], X[j], P[nn + nm + k + m * j])
                for k in range(m):
                    for i in range(n):
                        P[nn + i + n * k] = fma(dg[i], Y[k], P[nn + i + n * k])
                    for q in range(m):
                        P[nn + 2 * nm + q + m * k] = fma(dh[q], Y[k], P[nn + 2 * nm + q + m * k])
        out = out + P
    return out


def bits_equal(a, b) -> bool:
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return a.shape == b.shape and bool(np.array_equal(a.view(np.uint64), b.view(np.uint64)))

"""The case table of tests/test_wg_lattice.py: one list of solve cases and one of sensitivity
cases, read by the CPU tests (oracle against the LAPACK restatement) and by the GPU tests
(kernels against the oracle), with their input generators and the kernel-selection rule of
the C ABI host layer restated (csrc/mcpx_api.cpp prepare / prepare_sens,
csrc/ipm_inst_wg.hip pick), so that a test can say which compiled kernel a case launches."""

from __future__ import annotations

import os
import re
from dataclasses import dataclass

import numpy as np

from mcp_amd.qp_benchmark import generate_random_parameter
from tests.test_sensitivity import random_affine_theta

QP, AFFINE = 0, 1
FAMILY_NAME = {QP: "qp", AFFINE: "affine"}
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))), "mcp_amd", "csrc")
WAVE_ROWS = 64  # MCPX_MAX_KKT_DIM: the one-wave kernels' rows (include/mcpx.h)
JVP_RHS = 8  # MCPX_JVP_RHS: partials per factorisation of the JVP kernels (include/mcpx.h)


# ---------------------------------------------------------------- inputs


def feasible_qp_theta(rng, n, m, B):
    """generate_random_parameter's QP with b ← A x* − u, x* ~ N(0, I), u ~ U(0.1, 1): A x ≥ b has
    the strictly feasible point x*, whatever m is.  (A random b with m > n constraints is
    infeasible: every instance then runs to the iteration limits and fails.)"""
    th = generate_random_parameter(rng, n, m, 0.0, batch=B)
    A = th[:, n * n:n * n + m * n].reshape(B, n, m).transpose(0, 2, 1)  # vec(A) is column-major
    xs = rng.standard_normal((B, n))
    u = rng.uniform(0.1, 1.0, (B, m))
    th[:, n * n + m * n:n * n + m * n + m] = np.einsum("bkj,bj->bk", A, xs) - u
    return th


def _rng(family):
    return np.random.default_rng(7 if family == QP else 3)


# ---------------------------------------------------------------- kernel selection


def kernel_constants():
    """kDimBuckets and kGjMax of csrc/ipm_wg.h, MCPX_VR_MAX of csrc/ipm_wg_impl.hpp."""
    with open(os.path.join(CSRC, "ipm_wg.h")) as f:
        h = f.read()
    with open(os.path.join(CSRC, "ipm_wg_impl.hpp")) as f:
        impl = f.read()
    buckets = re.search(r"kDimBuckets\[\d+\]\s*=\s*\{([^}]*)\}", h).group(1)
    return dict(buckets=tuple(int(v) for v in buckets.split(",")),
                gj_max=int(re.search(r"kGjMax\s*=\s*(\d+)", h).group(1)),
                vr_max=int(re.search(r"#define\s+MCPX_VR_MAX\s+(\d+)", impl).group(1)))


def bucket_of(N, buckets):
    """pick_wg_bucket: the smallest vector-dimension bucket ≥ N."""
    return next(b for b in buckets if N <= b)


def gj_lda(m):
    """wg::kGjLda: the LDS row stride of the SCHUR kernels' copy of A."""
    return m | 1


def gj_a_cap(nv, gj_max):
    """wg::kGjACapOf: doubles of A the SCHUR kernel of bucket nv keeps in LDS."""
    best = max([1] + [n * gj_lda((nv - n) // 2) for n in range(1, gj_max + 1) if n < nv])
    return min(best, 128 * 65)


# ---------------------------------------------------------------- solve cases


@dataclass(frozen=True)
class SolveCase:
    family: int
    solver: str  # "reduced", "dense" or "schur"
    n: int
    m: int
    B: int = 4  # instances on the CPU; the GPU tests take the first gpu_B(...) of them
    slow: bool = False
    warm: bool = False  # x0, y0, s0 given

    @property
    def N(self):
        return self.n + 2 * self.m

    @property
    def ns(self):
        """wg::system_rows: rows of the system one Newton step factors."""
        return {"schur": self.n, "reduced": self.n + self.m, "dense": self.N}[self.solver]

    @property
    def id(self):
        return f"{FAMILY_NAME[self.family]}-{self.solver}-{self.n}x{self.m}" + ("-warm" if self.warm else "")

    def gpu_B(self, buckets):
        """4 instances; 2 from bucket 512 upwards."""
        return min(self.B, 4 if bucket_of(self.N, buckets) < 512 else 2)

    def inputs(self):
        """(θ (B, p), dict of the start: empty, or x0 / y0 / s0)."""
        rng = _rng(self.family)
        if self.family == AFFINE:
            th = random_affine_theta(rng, self.n, self.m, self.B)
        elif self.solver == "schur":
            th = feasible_qp_theta(rng, self.n, self.m, self.B)
        else:
            th = generate_random_parameter(rng, self.n, self.m, 0.0, batch=self.B)
        start = {}
        if self.warm:
            start = dict(x0=0.1 * rng.standard_normal((self.B, self.n)), y0=rng.uniform(0.5, 2.0, (self.B, self.m)),
                         s0=rng.uniform(0.5, 2.0, (self.B, self.m)))
        return th, start

    def kernel(self, c):
        """The compiled kernel the default (AUTO) selector launches for this case, as
        prepare picks the path and ipm_wg_kernel / pick the kernel; c: kernel_constants()."""
        lanes = self.N if self.solver == "dense" else self.n + self.m
        assert not (self.ns <= WAVE_ROWS and lanes <= WAVE_ROWS), f"{self.id}: a one-wave kernel takes it"
        nv = bucket_of(self.N, c["buckets"])
        if self.solver == "schur":
            assert self.family == QP and self.n <= c["gj_max"], f"{self.id}: no workgroup SCHUR kernel"
            return ("schur", nv)
        vr = nv == 128 or (nv == 256 and self.ns <= c["vr_max"])
        return (FAMILY_NAME[self.family], self.solver, nv, "vr" if vr else "workspace")


_BOTH = ((40, 30), (64, 32),  # 128-VR: N = 100, top edge N = 128
         (65, 32), (100, 50), (150, 50),  # 256-VR: bottom edge N = 129; ns = 200 (DENSE / REDUCED)
         (101, 50), (151, 50), (180, 38),  # 256-workspace: ns = 201 (DENSE / REDUCED); N = 256, ns = 218
         (129, 64), (200, 156),  # 512: N = 257, N = 512
         (201, 156))  # 768: N = 513
SCHUR_SHAPES = ((1, 64), (5, 70), (16, 60), (17, 120), (70, 11), (128, 66), (40, 200), (26, 319), (128, 320))

SOLVE_CASES = tuple(
    [SolveCase(fam, ls, n, m) for fam in (QP, AFFINE) for ls in ("reduced", "dense") for n, m in _BOTH]
    # N = 768 with ns = 576 and 768
    + [SolveCase(fam, "reduced", 384, 192, B=2, slow=True) for fam in (QP, AFFINE)]
    + [SolveCase(fam, "dense", 256, 256, B=2, slow=True) for fam in (QP, AFFINE)]
    + [SolveCase(QP, "schur", n, m) for n, m in SCHUR_SHAPES]
    + [SolveCase(QP, "reduced", 100, 78, warm=True), SolveCase(AFFINE, "dense", 60, 40, warm=True)])


# ---------------------------------------------------------------- sensitivity cases


@dataclass(frozen=True)
class SensCase:
    family: int
    n: int
    m: int
    K: int = JVP_RHS + 1  # JVP partials: a second factorisation with a 1-wide right-hand side
    B: int = 2
    cpu: bool = False  # compared with the dense LAPACK restatement on the CPU
    gpu: bool = True
    cond: bool = False  # the GPU test also runs cond_batch (the JVP kernel's estimate mode)
    slow: bool = False

    @property
    def N(self):
        return self.n + 2 * self.m

    @property
    def id(self):
        return f"{FAMILY_NAME[self.family]}-{self.n}x{self.m}"

    def inputs(self):
        """θ (B, p), cotangents gx, gy, gs and partials θ̇ (B, K, p)."""
        rng = _rng(self.family)
        n, m, B = self.n, self.m, self.B
        th = (generate_random_parameter(rng, n, m, 0.0, batch=B) if self.family == QP
              else random_affine_theta(rng, n, m, B))
        g = rng.standard_normal((B, n)), rng.standard_normal((B, m)), rng.standard_normal((B, m))
        return th, g, rng.standard_normal((B, self.K, th.shape[1]))

    def kernels(self, c):
        """prepare_sens: beyond one wave's rows, the VJP and the JVP kernel of the bucket."""
        assert self.N > WAVE_ROWS, f"{self.id}: the one-wave kernels take it"
        nv = bucket_of(self.N, c["buckets"])
        return {(FAMILY_NAME[self.family], "vjp", nv), (FAMILY_NAME[self.family], "jvp", nv)}


SENS_CASES = (
    SensCase(QP, 40, 30), SensCase(AFFINE, 40, 30),  # bucket 128
    SensCase(QP, 65, 32), SensCase(AFFINE, 60, 40),  # bucket 256
    SensCase(QP, 129, 64), SensCase(AFFINE, 129, 64),  # bucket 512: N = 257 …
    SensCase(QP, 200, 156, cpu=True, cond=True), SensCase(AFFINE, 200, 156),  # … and N = 512
    SensCase(AFFINE, 150, 100, K=3, cpu=True, gpu=False),
    SensCase(QP, 201, 156), SensCase(AFFINE, 201, 156),  # bucket 768: N = 513 …
    SensCase(QP, 256, 256, K=3, cpu=True, slow=True),  # … and N = 768 (K = 3 bounds the slot)
)

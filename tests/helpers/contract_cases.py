"""The case table of tests/test_buffer_contract*.py: the smallest shape that reaches each kernel
family through each full-θ entry point (mcpx_solve_batch[_device], mcpx_solve_vjp_batch_device,
mcpx_{vjp,jvp,cond}_batch[_device] and their _module forms), with the inputs, the oracle's
reference on the PACKED θ, and the host layer's selection rule restated (csrc/mcpx_api.cpp
prepare / prepare_sens / launch, csrc/ipm_inst_spec.hip, csrc/ipm_inst_fused.hip), so that a
CPU test can say which kernel family a case launches.

Inputs.  One-wave and module solve cases hold, on the oracle: an instance with a NaN in θ (row 1),
an instance that stops at max_outer_iters (row 2: an infeasible QP, A₁ = −A₀ with b₀ = b₁ = 1;
the modules: games and cubics that do not converge) and at least three solved instances.  The
outer limit is 16 for the whole call: every solvable instance here needs at most 13 outer
iterations at tol = 1e-6, so 16 keeps them solved and bounds the unsolvable one at 285 Newton steps (a limit
of 2 would leave no solved instance in a cold-started batch).  Workgroup cases use
feasible_qp_theta / random_affine_theta and all solve, as in tests/helpers/wg_cases.py.
Batches are 5 or 7 instances (odd), 2 in the 512 bucket."""

from __future__ import annotations

from dataclasses import dataclass, replace

import numpy as np

from mcp_amd import _abi
from mcp_amd.qp_benchmark import affine_embedding, generate_random_parameter
from tests.helpers.wg_cases import (AFFINE, FAMILY_NAME, JVP_RHS, QP, WAVE_ROWS, bucket_of, feasible_qp_theta, gj_a_cap,
                                    gj_lda, kernel_constants)
from tests.test_sensitivity import _same, random_affine_theta

NL = _abi.FAMILY_NONLINEAR
TRACE = 64  # steps of the α trace every solve case records (the unsolvable rows take more)
OUTER_LIMIT = 16
SPEC_QP = ((2, 2), (16, 8), (32, 16))  # compile-time (n, m) of ipm_inst_spec.hip / ipm_inst_fused.hip
FIELDS = ("x", "y", "s", "kkt_error", "eps", "outer_iters", "status", "newton_iters", "active_mask", "alpha_trace",
          "fail_reason")
OPTIONAL = ("newton_iters", "active_mask", "alpha_trace", "fail_reason")
FILL = 0xA5  # the byte every caller-provided output is filled with before a call


def theta_p(case) -> int:
    return module_of(case).nl.p if case.module else _abi.theta_dim(case.family, case.n, case.m)


# ---------------------------------------------------------------- modules (built by other tests' makers)

_MODULES: dict = {}


def module_of(case):
    """The PrimalDualMCP of a module case: the cubic of tests/test_nonlinear.py or the T = 2
    lane-change game (the modules build() prebuilds; nothing new is generated)."""
    if case.module not in _MODULES:
        if case.module == "cubic":
            from tests.test_nonlinear import cubic_mcp

            _MODULES["cubic"] = cubic_mcp()
        else:
            from mcp_amd.lane_change import LaneChangeGame

            _MODULES["game"] = LaneChangeGame(2)
            _MODULES["lane"] = _MODULES["game"].mcp
    return _MODULES[case.module]


# ---------------------------------------------------------------- solve cases


@dataclass(frozen=True)
class SolveCase:
    family: int
    solver: str
    n: int
    m: int
    B: int = 5
    pad: int = 1  # NaN doubles behind every instance's θ in the stride tests: 1 or 3
    warm: bool = False  # x0, y0, s0 given
    generic: bool = False  # MCPX_GENERIC_KERNELS=1: the runtime-(n, m) kernel at a compile-time size
    asym: bool = False  # M[1,0] += 1e-3 in rows 0, 3, …: the fast pass defers them to pass 2
    kernel: str = "auto"
    module: str = ""  # "cubic" or "lane"
    fused: bool = False  # through mcpx_solve_vjp_batch_device

    @property
    def N(self):
        return self.n + 2 * self.m

    @property
    def id(self):
        name = self.module or FAMILY_NAME[self.family]
        tags = [t for t, on in (("generic", self.generic), ("asym", self.asym), ("fused", self.fused),
                                (self.kernel, self.kernel != "auto"), ("warm", self.warm)) if on]
        return "-".join([name, self.solver, f"{self.n}x{self.m}", *tags])

    @property
    def one_wave(self):
        return self.family != NL and wave_ok(self)

    @property
    def params(self):
        """Solver keywords of every call of the case (and of its oracle run)."""
        kw = dict(tol=1e-6, linear_solver=self.solver)
        if self.module:
            kw["kernel"] = self.kernel
        if self.one_wave or self.module:
            kw["max_outer_iters"] = OUTER_LIMIT
        return kw

    def inputs(self):
        """(packed θ (B, p), start: {} or x0 / y0 / s0)."""
        n, m, B = self.n, self.m, self.B
        if self.module == "cubic":
            from tests.test_nonlinear import _cubic_theta

            th = _cubic_theta(B)  # rows 2 and 3 stop at the outer limit
            th[B - 1, 0] = np.nan
            return th, {}
        if self.module == "lane":
            from mcp_amd.qp_benchmark import chunked_slice

            mcp = module_of(self)
            game = _MODULES["game"]
            raw = chunked_slice(lambda rng, k: game.generate_random_parameter(rng, k), 1, 0, 19 + B)[19:]
            th = np.ascontiguousarray(mcp.theta_map(raw))  # game 23 of the stream (row 4) does not converge
            th[1, 0] = np.nan
            return th, {}
        rng = np.random.default_rng(100 * n + m + (17 if self.family == AFFINE else 0))
        if not self.one_wave:  # workgroup: every instance solves
            th = random_affine_theta(rng, n, m, B) if self.family == AFFINE else feasible_qp_theta(rng, n, m, B)
        else:
            qp = generate_random_parameter(rng, n, m, 0.0, batch=B)
            a0 = n * n  # vec(A) column-major: A[k, j] at a0 + j·m + k
            A = qp[2, a0:a0 + m * n].reshape(n, m)
            A[:, 1] = -A[:, 0]  # A₁ x ≥ 1 and −A₁ x ≥ 1: infeasible, the solve runs to the outer limit
            qp[2, a0 + m * n:a0 + m * n + 2] = 1.0
            if self.asym:
                qp[0::3, 1] += 1e-3  # M[1,0] ≠ M[0,1] in rows 0, 3, …
            if self.family == QP:
                th = qp
            elif self.solver == "schur":
                th = affine_embedding(qp, n, m)  # S ≡ 0
            else:
                th = random_affine_theta(rng, n, m, B)
                th[2] = affine_embedding(qp[2:3], n, m)[0]
            th[1, 0] = np.nan
        start = {}
        if self.warm:
            start = dict(x0=0.1 * rng.standard_normal((B, n)), y0=rng.uniform(0.5, 2.0, (B, m)),
                         s0=rng.uniform(0.5, 2.0, (B, m)))
        return np.ascontiguousarray(th), start


def wave_ok(c) -> bool:
    """prepare: a one-wave kernel takes the case (QP / affine families)."""
    rows = {"schur": c.n, "reduced": c.n + c.m, "dense": c.N}[c.solver]
    lanes = c.N if c.solver == "dense" else c.n + c.m
    return rows <= WAVE_ROWS and lanes <= WAVE_ROWS


def solve_family(c, k=None):
    """The kernel family a solve case launches, by the host layer's rule; k: kernel_constants()."""
    k = k or kernel_constants()
    if c.module:
        mcp = module_of(c)
        nl = mcp.nl
        if c.module == "cubic":
            assert nl.solvers()[c.solver] and c.kernel == "auto"
            return ("module", "cubic", c.solver, "wave")
        assert c.solver == "schur" and nl.solvers()["schur"] and nl.band_can and not nl.band_auto
        assert nl.wg_solvers()["schur"]
        return ("module", "lane", "schur", {"auto": "wave"}.get(c.kernel, c.kernel))
    fam = FAMILY_NAME[c.family]
    if wave_ok(c):
        spec = ((c.family == QP and c.solver in ("reduced", "schur") and (c.n, c.m) in SPEC_QP)
                or (c.family == AFFINE and c.solver == "schur" and (c.n, c.m) == (32, 16)))
        if c.fused:
            epilogue = c.family == QP and c.solver == "schur" and (c.n, c.m) in SPEC_QP
            return ("fused", "epilogue" if epilogue else "composed", c.solver, c.n, c.m)
        if spec and not c.generic:
            if c.asym:
                assert c.solver == "schur"
                return ("wave", "two-pass", fam, c.n, c.m)
            return ("wave", "spec", fam, c.solver, c.n, c.m)
        assert not c.asym
        return ("wave", "generic-forced" if c.generic else "generic", fam, c.solver, c.n, c.m)
    assert not (c.fused or c.generic or c.asym)
    nv = bucket_of(c.N, k["buckets"])
    ns = {"schur": c.n, "reduced": c.n + c.m, "dense": c.N}[c.solver]
    if c.solver == "schur":
        assert c.family == QP and c.n <= k["gj_max"]
        lds = c.n * gj_lda(c.m) <= gj_a_cap(nv, k["gj_max"])
        return ("wg", "schur", nv, "A in LDS" if lds else "A from theta", max(1, (c.m + 63) // 64))
    vr = nv == 128 or (nv == 256 and ns <= k["vr_max"])
    return ("wg", fam, c.solver, nv, "vr" if vr else "workspace")


def _one_wave_cases():
    out = []
    for n, m in SPEC_QP:
        out += [SolveCase(QP, "reduced", n, m), SolveCase(QP, "schur", n, m)]
    out.append(SolveCase(AFFINE, "schur", 32, 16))
    for n, m, B in ((5, 3, 5), (4, 3, 7)):  # p = 48 (even) and p = 35 (odd)
        out += [SolveCase(QP, ls, n, m, B=B) for ls in ("reduced", "dense", "schur")]
    out += [SolveCase(AFFINE, ls, 6, 4, B=7) for ls in ("reduced", "dense", "schur")]
    out.append(SolveCase(QP, "schur", 32, 16, generic=True))
    out.append(SolveCase(QP, "schur", 16, 8, asym=True, B=7))
    return out


def _numbered(cases):
    """pad alternates 1 / 3 down the table and every other case is warm-started (the modules
    start cold)."""
    return tuple(replace(c, pad=(1, 3)[i % 2], warm=(i % 2 == 1) and not c.module) for i, c in enumerate(cases))


WG_CASES = ([SolveCase(f, ls, 40, 30) for f in (QP, AFFINE) for ls in ("reduced", "dense")]
            # bucket 256: REDUCED factors 151 rows in registers, DENSE 201 (> MCPX_VR_MAX) through the workspace
            + [SolveCase(QP, "reduced", 101, 50), SolveCase(QP, "dense", 101, 50)]
            + [SolveCase(QP, "schur", 5, 70), SolveCase(QP, "schur", 128, 66, B=2)])
MODULE_CASES = [SolveCase(NL, "reduced", 1, 1, B=7, module="cubic")] + [
    SolveCase(NL, "schur", 40, 50, B=7, module="lane", kernel=k) for k in ("auto", "multiwave", "band", "workgroup")]
FUSED_CASES = [SolveCase(QP, "schur", 32, 16, fused=True), SolveCase(QP, "reduced", 5, 3, fused=True)]

SOLVE_CASES = _numbered(_one_wave_cases() + WG_CASES + MODULE_CASES)
FUSED = _numbered(FUSED_CASES)
FUSED_CT = (2.0, 2.0, 0.0)  # the cotangent of f = Σx² + Σy²: ax, ay, as (b arrays NULL)


def case_by_id(cid):
    return next(c for c in SOLVE_CASES + FUSED + SENS_CASES if c.id == cid)


# ---------------------------------------------------------------- sensitivity cases


@dataclass(frozen=True)
class SensCase:
    family: int
    n: int
    m: int
    B: int = 5
    K: int = JVP_RHS + 1  # a second factorisation with a 1-wide right-hand side
    pad: int = 1
    module: str = ""

    @property
    def N(self):
        return self.n + 2 * self.m

    @property
    def id(self):
        return f"sens-{self.module or FAMILY_NAME[self.family]}-{self.n}x{self.m}"

    @property
    def kinds(self):
        return ("vjp", "jvp") if self.module else ("vjp", "jvp", "cond")

    def inputs(self):
        """(packed θ (B, p), (gx, gy, gs), θ̇ (B, K, p)); every instance solves."""
        n, m, B = self.n, self.m, self.B
        rng = np.random.default_rng(1000 + 100 * n + m + self.family)
        if self.module:
            from mcp_amd.qp_benchmark import chunked_slice

            mcp = module_of(self)
            game = _MODULES["game"]
            th = np.ascontiguousarray(mcp.theta_map(chunked_slice(
                lambda r, k: game.generate_random_parameter(r, k), 1, 0, B)))
        elif self.family == QP:
            th = generate_random_parameter(rng, n, m, 0.0, batch=B)
        else:
            th = random_affine_theta(rng, n, m, B)
        g = rng.standard_normal((B, n)), rng.standard_normal((B, m)), rng.standard_normal((B, m))
        return th, g, rng.standard_normal((B, self.K, th.shape[1]))


def sens_families(c):
    """prepare_sens: the kernel family of each sensitivity call of the case."""
    if c.module:
        return {("module-sens", c.module, kind) for kind in c.kinds}
    fam = FAMILY_NAME[c.family]
    out = set()
    for kind in c.kinds:
        if c.N <= WAVE_ROWS and kind != "cond":
            out.add(("sens-wave", fam, kind))
        else:  # the condition estimate runs the workgroup layout at every size
            out.add(("sens-wg", fam, kind))
    return out


SENS_CASES = (SensCase(QP, 16, 8, B=5, pad=1), SensCase(AFFINE, 6, 4, B=7, pad=3),
              SensCase(QP, 40, 30, B=5, pad=3), SensCase(AFFINE, 40, 30, B=7, pad=1),
              SensCase(NL, 40, 50, B=5, pad=1, module="lane"))


# ---------------------------------------------------------------- the oracle's references (packed θ)

_REF: dict = {}


def oracle_solve(oracle_lib, c, trace_len=TRACE):
    """The oracle's solve of a case on the packed θ, computed once; nobody writes into it."""
    key = (c, trace_len)
    if key not in _REF:
        th, start = c.inputs()
        if c.module:
            _REF[key] = oracle_lib.solve_batch_nl(module_of(c).nl, th, trace_len=trace_len, nthreads=8, **start,
                                                  **c.params)
        else:
            _REF[key] = oracle_lib.solve_batch(c.family, c.n, c.m, th, trace_len=trace_len, nthreads=8, **start,
                                               **c.params)
    return _REF[key]


def oracle_fused(oracle_lib, c):
    """(solve record, dtheta, status) of a fused case: the oracle's solve, then its pullback at
    that iterate with g = a·z (two roundings, as the header's rule; the b arrays are NULL)."""
    key = (c, "fused")
    if key not in _REF:
        r = oracle_solve(oracle_lib, c)
        th = c.inputs()[0]
        ax, ay, as_ = FUSED_CT
        g = [None if a == 0.0 else a * r[k] for a, k in ((ax, "x"), (ay, "y"), (as_, "s"))]
        _REF[key] = (r, *oracle_lib.vjp_batch(c.family, c.n, c.m, th, r["x"], r["y"], r["s"], *g, nthreads=8))
    return _REF[key]


def oracle_point(oracle_lib, c):
    """The solutions a sensitivity case is differentiated at: the oracle's own solve."""
    key = (c, "point")
    if key not in _REF:
        th = c.inputs()[0]
        if c.module:
            _REF[key] = oracle_lib.solve_batch_nl(module_of(c).nl, th, tol=1e-6, linear_solver="schur", nthreads=8)
        else:
            _REF[key] = oracle_lib.solve_batch(c.family, c.n, c.m, th, tol=1e-6, nthreads=8)
    return _REF[key]


def oracle_sens(oracle_lib, c, kind):
    """(result, status) of the oracle's vjp / jvp / cond at oracle_point, on the packed θ."""
    key = (c, kind)
    if key not in _REF:
        th, g, td = c.inputs()
        r = oracle_point(oracle_lib, c)
        at = (r["x"], r["y"], r["s"])
        if c.module:
            nl = module_of(c).nl
            _REF[key] = (oracle_lib.vjp_batch_nl(nl, th, *at, *g, nthreads=8) if kind == "vjp"
                         else oracle_lib.jvp_batch_nl(nl, th, *at, td, nthreads=8))
        elif kind == "vjp":
            _REF[key] = oracle_lib.vjp_batch(c.family, c.n, c.m, th, *at, *g, nthreads=8)
        elif kind == "jvp":
            _REF[key] = oracle_lib.jvp_batch(c.family, c.n, c.m, th, *at, td, nthreads=8)
        else:
            _REF[key] = oracle_lib.cond_batch(c.family, c.n, c.m, th, *at, nthreads=8)
    return _REF[key]


# ---------------------------------------------------------------- padding and comparison


def padded(a, pad):
    """(B, w) → a fresh contiguous (B, w + pad) array, the extra columns NaN."""
    wide = np.full((a.shape[0], a.shape[1] + pad), np.nan)
    wide[:, :a.shape[1]] = a
    return wide


def expected_trace(ref, untouched):
    """The α trace a call must leave: the oracle's entries for the steps it recorded (the first
    min(newton_iters, trace_len) of an instance), `untouched` everywhere else — the caller's fill
    through a device entry, 254 through a host entry (whose whole array is written)."""
    tr = ref["alpha_trace"]
    steps = np.arange(tr.shape[1])[None, :] < np.minimum(ref["newton_iters"], tr.shape[1])[:, None]
    assert np.array_equal(tr[~steps], np.full_like(tr[~steps], 254))  # the oracle's own rule
    return np.where(steps[:, :, None], tr, np.uint8(untouched))


def solve_mismatches(got, ref, untouched=254, absent=()):
    """Names of the fields of `got` whose bits differ from the oracle's record `ref`; fields in
    `absent` (passed as NULL) are not in `got`.  NaN equals NaN whatever its payload."""
    bad = []
    for k in FIELDS:
        if k in absent:
            continue
        g = np.asarray(got[k])
        r = expected_trace(ref, untouched) if k == "alpha_trace" else np.asarray(ref[k])
        if k == "active_mask":
            g, r = g.view(np.uint64).reshape(r.shape), r.view(np.uint64)
        if not _same(g, r):
            bad.append(k)
    return bad


# ---------------------------------------------------------------- a θ the two-pass protocol cannot heal


def shift_blind_qp(n, m, B=5, pad=1, c=0.5):
    """(packed θ (B, p), the same at stride p + pad) for the QP family's SCHUR kernels, built so
    that a fast pass which forms instance 1's pointer with p instead of theta_ld still passes its
    own symmetry check.  Under NaN padding that mistake heals itself: the misplaced M block is not
    symmetric, the fast pass defers the instance, and pass 2 solves it from the right address.
    Here M = c·𝟙𝟙ᵀ (every entry c, positive semidefinite) and the padding doubles are c too, so the
    window that starts at 1·p — row 0's padding, then row 1 shifted by `pad` — has a symmetric
    M block as well, and the fast pass goes on to solve it with a shifted A, b and ϕ.
    b = A x* − u keeps every instance strictly feasible; ϕ = φ·𝟙 lies in M's range, so the
    objective is bounded below."""
    rng = np.random.default_rng(4000 + 100 * n + m + pad)
    th = feasible_qp_theta(rng, n, m, B)
    th[:, :n * n] = c
    th[:, n * n + m * n + m:] = rng.uniform(0.2, 1.0, (B, 1))
    wide = np.full((B, th.shape[1] + pad), c)
    wide[:, :th.shape[1]] = th
    return th, wide

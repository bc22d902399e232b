/*
 * mcpx.h — C ABI of the MI355X-native batched interior-point MCP solver.
 *
 * This is the drop-in boundary for the Newton-step hot path of
 * MixedComplementarityProblems.jl (TianyuQ/MCP).  One call replaces, for a
 * whole batch of parameter vectors θ, the host loop of
 *
 *     solve(::InteriorPoint, mcp::PrimalDualMCP, θ; x₀, y₀, s₀, tol,
 *           max_inner_iters, max_outer_iters, tightening_rate,
 *           loosening_rate, min_stepsize, verbose, linear_solve_algorithm)
 *                                                  reference src/solver.jl:35-51
 *
 * i.e. the per-instance block src/solver.jl:53-121 (residual F! and Jacobian
 * ∇F_z! callbacks of src/mcp.jl:82-120, the regularised Newton solve
 * src/solver.jl:81-90, the fraction-to-the-boundary line search
 * src/solver.jl:93-100,127-138, the update src/solver.jl:103-108 and the
 * ϵ-continuation src/solver.jl:71-121).  The reference binds nothing over an
 * FFI today (it is pure Julia); the `ccall` a maintainer would add is shown in
 * INTEGRATION.md.
 *
 * Problem families (how F and ∇F are evaluated on device per instance):
 *
 *   MCPX_FAMILY_QP      the convex-QP family of
 *                       benchmark/quadratic_program_benchmark.jl:7-90:
 *                         G(x,y;θ) = M x − ϕ − Aᵀ y,  H(x,y;θ) = A x − b,
 *                       θ = [vec(M); vec(A); b; ϕ] column-major
 *                       (unpack_parameters, :77-90), p = n² + m n + m + n.
 *   MCPX_FAMILY_AFFINE  general affine MCP (any G/H affine in (x,y)):
 *                         G = P x + Q y + g,  H = R x + S y + h,
 *                       θ = [vec(P); vec(Q); vec(R); vec(S); g; h]
 *                       column-major, p = n² + 2 n m + m² + n + m.
 *                       (The Python front-end traces user G/H callables —
 *                       src/mcp.jl:27-52, :155-210 — into this layout.)
 *   MCPX_FAMILY_NONLINEAR  general G(x,y;θ), H(x,y;θ) (e.g. the trajectory games of
 *                       src/game.jl): device code generated per problem and run
 *                       through an mcpx_module (end of this header); θ is the
 *                       problem's own parameter vector.
 *
 * Conventions: all arrays are instance-major (instance b's data is contiguous,
 * stride `theta_ld` for θ); all buffers are caller-owned; the library keeps no
 * pointer after returning.  The theta_ld − p doubles after each instance's θ are
 * never read or written by any call, the last instance's included: a θ buffer may
 * end with its last instance, at (B − 1)·theta_ld + p doubles.  Return value
 * 0 = OK, < 0 = API misuse / HIP error
 * (message via mcpx_last_error(), thread-local).  Numerical failure is never
 * an error: it is status[b] = MCPX_STATUS_FAILED, as in src/solver.jl:84-100,
 * 117-119, which never throws.
 */
#ifndef MCPX_H
#define MCPX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 2.0.0: mcpx_out gained the trailing fail_reason pointer (1.6), which changes the
 * struct's size and layout: a caller built against a 1.x header passes a shorter
 * struct, so the major version moved.  Callers check mcpx_version() / 10000 against
 * MCPX_VERSION / 10000 before the first call (mcp_amd/_lib.py does). */
#define MCPX_VERSION 20200 /* 2.1.0: mcpx_cond_batch*; 2.2.0: MCPX_FAIL_INPUT */
/* The shared-matrix entries (mcpx_theta_shared_dim, mcpx_theta_var_dim, mcpx_solve_batch_shared,
 * mcpx_solve_batch_shared_device) were added under 2.2.0 without a version step: no struct and no
 * existing function changed, so every 2.x caller keeps working; a caller that needs them looks
 * the symbols up.  The same holds for their sensitivities (mcpx_vjp_batch_shared[_device],
 * mcpx_jvp_batch_shared[_device], mcpx_solve_vjp_batch_shared_device), the reduced gradient
 * (mcpx_vjp_batch_shared_reduce[_device]), the tangents along the shared block
 * (mcpx_jvp_batch_shared_dot[_device]) and the condition estimate (mcpx_cond_batch_shared[_device]). */

/* error codes */
#define MCPX_OK 0
#define MCPX_EINVAL (-1)      /* argument check failed (reference: ArgumentError / @assert) */
#define MCPX_EHIP (-2)        /* HIP runtime error */
#define MCPX_ENODEV (-3)      /* no usable gfx950 device */
#define MCPX_EUNSUPPORTED (-4) /* size outside what the compiled kernels cover */

/* per-instance status (reference: :solved / :failed, src/solver.jl:69,86,98,118) */
#define MCPX_STATUS_SOLVED 0
#define MCPX_STATUS_FAILED 1
/* mcpx_out.fail_reason bits: the events behind the reference's `verbose` warnings
 * (src/solver.jl), each set when it happened at least once during the solve */
#define MCPX_FAIL_LINSOLVE 1u   /* a Newton system was singular, a zero pivot (:84-88) */
#define MCPX_FAIL_LINESEARCH 2u /* the fraction-to-the-boundary line search gave NaN (:93-99) */
#define MCPX_FAIL_MAX_OUTER 4u  /* outer_iters reached max_outer_iters (:117-119) */
/* the instance is outside what the chosen elimination is exact for, so it was not solved:
 * MCPX_LINSOLVE_SCHUR on an affine θ whose S block (∂H/∂y) is not exactly zero.  The record
 * is status FAILED, kkt_error NaN, the initial point, outer_iters 1, newton_iters 0. */
#define MCPX_FAIL_INPUT 8u

#define MCPX_FAMILY_QP 0
#define MCPX_FAMILY_AFFINE 1
#define MCPX_FAMILY_NONLINEAR 2

/* largest linear-system dimension of the register-resident one-wave kernels
 * (n + m for MCPX_LINSOLVE_REDUCED, n + 2m for MCPX_LINSOLVE_DENSE) */
#define MCPX_MAX_KKT_DIM 64
/* largest KKT dimension n + 2m of the workgroup-per-instance kernels of the QP
 * and affine families (blocked LU with MFMA trailing updates, REDUCED / DENSE);
 * a generated nonlinear module sizes its own (mcpx_module_dims) */
#define MCPX_MAX_WG_KKT_DIM 768

/* Which kernel family runs a solve (mcpx_params.kernel):
 *  MCPX_KERNEL_AUTO       one wave per instance when the system fits its 64 rows,
 *                         else one workgroup per instance;
 *  MCPX_KERNEL_WAVE       only the one-wave kernels (MCPX_EUNSUPPORTED beyond);
 *  MCPX_KERNEL_WORKGROUP  the workgroup-per-instance kernels at any size they
 *                         support (REDUCED / DENSE, and SCHUR for generated
 *                         modules) — bit-identical results to the one-wave path;
 *  MCPX_KERNEL_MULTIWAVE  generated modules, SCHUR: one 4-wave workgroup per
 *                         instance, S in LDS, the LU's columns split over the waves
 *                         (module kernel-mask bit MCPX_MODULE_SCHUR_MW); same bits,
 *                         opt-in (slower than one wave on the lane-change game);
 *  MCPX_KERNEL_BAND       generated modules, SCHUR: one wave per instance, the band LU
 *                         of the symmetrically reordered Schur complement (module bit
 *                         MCPX_MODULE_BAND; the oracle's lu_band_solve).  AUTO takes it
 *                         when the module prefers it (bit MCPX_MODULE_BAND_AUTO) or has
 *                         no one-wave SCHUR kernel. */
#define MCPX_KERNEL_AUTO 0
#define MCPX_KERNEL_WAVE 1
#define MCPX_KERNEL_WORKGROUP 2
#define MCPX_KERNEL_MULTIWAVE 3
#define MCPX_KERNEL_BAND 4
/* largest max_inner_iters (ϵ-schedule table length) */
#define MCPX_MAX_INNER_ITERS 128
/* largest number of line-search trials (α = decayᵉ, e = 0..E) */
#define MCPX_MAX_LS_TRIALS 64

/* Newton linear solve (∇F + tol·I) δz = −F, src/solver.jl:81-83:
 *  MCPX_LINSOLVE_REDUCED  exact block elimination of the slack block first —
 *                         ∂(s⊙y − ϵ)/∂s = Y + tol·I is diagonal for every MCP of
 *                         the form F = [G; H − s; s⊙y − ϵ] (src/mcp.jl:76-80) —
 *                         then dense LU with partial pivoting of the (n+m)-dim
 *                         Schur complement (default; N ≤ 64 means n + m ≤ 64);
 *  MCPX_LINSOLVE_DENSE    dense LU with partial pivoting of the full
 *                         (n+2m)-dim system (n + 2m ≤ 64);
 *  MCPX_LINSOLVE_SCHUR    ∂H/∂y = 0 (QP family; affine family, whose S block must
 *                         then be exactly 0 — an instance with any nonzero (or NaN)
 *                         S entry is not solved and reports MCPX_FAIL_INPUT; generated modules
 *                         without an ∂H/∂y block): after the slack block, the
 *                         now-diagonal y block is eliminated as well, leaving the
 *                         n×n Schur complement S = (M + tol·I) + Aᵀ D⁻¹ A (affine:
 *                         (P + tol·I) − Q D⁻¹ R; both formed on the matrix cores,
 *                         fp64 MFMA).  M (affine: P) exactly symmetric (affine:
 *                         and −Q = Rᵀ exactly): S is solved by pivot-free
 *                         Gauss-Jordan while every pivot is > 0 (S SPD), and by
 *                         dense LU with partial pivoting otherwise — the oracle
 *                         takes the same branch (gj_spd_solve / lu_solve); a QP
 *                         passed as affine (P = M, Q = −Aᵀ, R = A, g = −ϕ, h = −b)
 *                         gives the QP solve's bits.  Modules: dense LU with
 *                         partial pivoting.  One wave: n + m ≤ 64; the QP family
 *                         also on one workgroup per instance up to n = 128 (S formed
 *                         on MFMA, blocked Gauss-Jordan with MFMA trailing updates,
 *                         the same bits). */
#define MCPX_LINSOLVE_REDUCED 0
#define MCPX_LINSOLVE_DENSE 1
#define MCPX_LINSOLVE_SCHUR 2

/* Solver keyword arguments, same names and defaults as src/solver.jl:42-50;
 * tau and decay are the hard-coded defaults of
 * fraction_to_the_boundary_linesearch (src/solver.jl:127). */
typedef struct mcpx_params {
  double tol;               /* 1e-4 */
  double tightening_rate;   /* 0.1  */
  double loosening_rate;    /* 0.5  */
  double min_stepsize;      /* 1e-4 (the docstring's 1e-2 is stale, src/solver.jl:31 vs :48) */
  double tau;               /* 0.995 */
  double decay;             /* 0.5  */
  int32_t max_inner_iters;  /* 20 */
  int32_t max_outer_iters;  /* 50 */
  int32_t linear_solver;    /* MCPX_LINSOLVE_* — the reference's linear_solve_algorithm kwarg (src/solver.jl:50) */
  int32_t kernel;           /* MCPX_KERNEL_* (0 = auto) */
} mcpx_params;

/* Batch descriptor. */
typedef struct mcpx_desc {
  int32_t family;   /* MCPX_FAMILY_* */
  int32_t n;        /* unconstrained_dimension (src/mcp.jl:22) */
  int32_t m;        /* constrained_dimension   (src/mcp.jl:23) */
  int32_t pad_;
  int64_t batch;    /* number of instances B */
  int64_t theta_ld; /* doubles between consecutive instances' θ (>= mcpx_theta_dim) */
} mcpx_desc;

/* Outputs, one record per instance.  Required: x, y, s, kkt_error, eps,
 * outer_iters, status (the NamedTuple of src/solver.jl:121).  Optional
 * (NULL = not wanted): newton_iters (total Newton steps taken),
 * active_mask (bit k of word b*W + k/64 set iff y_k > s_k at return, W = max(1, ⌈m/64⌉)),
 * alpha_trace (per accepted Newton step two bytes (e_s, e_y): α = decay^e;
 * at most trace_len steps recorded per instance), fail_reason (MCPX_FAIL_* bits of the
 * failure events seen; status is FAILED iff MCPX_FAIL_MAX_OUTER is set or the last
 * outer iteration ended in one of the other two). */
typedef struct mcpx_out {
  double* x;            /* [B*n] */
  double* y;            /* [B*m] */
  double* s;            /* [B*m] */
  double* kkt_error;    /* [B] */
  double* eps;          /* [B] */
  int32_t* outer_iters; /* [B] */
  int32_t* status;      /* [B] */
  int32_t* newton_iters;  /* [B] or NULL */
  uint64_t* active_mask;  /* [B*W] or NULL */
  uint8_t* alpha_trace;   /* [B*trace_len*2] or NULL */
  int32_t trace_len;
  int32_t pad_;
  uint8_t* fail_reason;   /* [B] or NULL */
} mcpx_out;

int mcpx_version(void);
const char* mcpx_last_error(void);
void mcpx_default_params(mcpx_params* prm);
/* θ dimension p of a family at (n, m); < 0 on bad input. */
int64_t mcpx_theta_dim(int32_t family, int32_t n, int32_t m);
/* The split of θ′ for shared-matrix batches (QP and affine families; < 0 on bad input, and
 * for MCPX_FAMILY_NONLINEAR, whose θ is the module's own).  θ′ is cut at one offset:
 *   QP      shared [vec(M); vec(A)]                   n² + m·n          per instance [b; ϕ]  m + n
 *   affine  shared [vec(P); vec(Q); vec(R); vec(S)]   n² + 2nm + m²     per instance [g; h]  n + m
 * so shared ‖ var_b is instance b's θ′, and shared_dim + var_dim = mcpx_theta_dim. */
int64_t mcpx_theta_shared_dim(int32_t family, int32_t n, int32_t m);
int64_t mcpx_theta_var_dim(int32_t family, int32_t n, int32_t m);
/* number of visible HIP devices (0 when none) */
int mcpx_device_count(void);
/* Debug: with MCPX_POISON=1 in the environment every device block the library allocates for
 * itself is filled with NaN bytes up to its requested size and a canary after it, checked when
 * the block is released; this returns the number of blocks found overwritten past their size
 * (each also reported on stderr).  0 without MCPX_POISON. */
int64_t mcpx_debug_canary_violations(void);

/* Host-buffer batched solve (what the Julia ccall / Python API drive).
 * Copies θ (and optional warm starts x0/y0/s0, each [B*n] / [B*m], NULL ⇒
 * the defaults x₀=0, y₀=1, s₀=1 of src/solver.jl:39-41) to `num_devices`
 * GPUs (0 ⇒ all visible), shards the batch contiguously, solves and copies
 * the outputs back.  Blocking.  Per device the shard is pipelined in chunks on
 * two streams (the upload of chunk c+1 overlaps the solve of chunk c); θ in a
 * range registered with mcpx_host_register is read by DMA straight from the
 * caller's pages, any other θ is staged by the HIP runtime.  The environment
 * variable MCPX_HOST_SHARDS = k (tests) splits the batch into k shards over the
 * visible devices round-robin, one host thread each, as k devices would. */
int mcpx_solve_batch(const mcpx_desc* desc, const double* theta,
                     const double* x0, const double* y0, const double* s0,
                     const mcpx_params* prm, int num_devices, mcpx_out* out);

/* Shared-matrix batches: every instance has the same matrix block and its own vectors.
 * `theta_shared` holds mcpx_theta_shared_dim doubles ONCE; `theta_var` holds instance b's
 * mcpx_theta_var_dim doubles at theta_var + b·desc->theta_ld — in these two calls
 * desc->theta_ld is the stride of theta_var (>= mcpx_theta_var_dim; padding is never read).
 * Contract: every output field is bit-identical to mcpx_solve_batch[_device] on the
 * materialised θ′ (shared ‖ var_b per instance).  Everything else is as in those calls: warm
 * starts, params, outputs, size limits, kernel selection, MCPX_ENODEV, the pipeline knobs and
 * num_devices.  MCPX_EINVAL: MCPX_FAMILY_NONLINEAR; NULL theta_shared or theta_var with
 * batch > 0.  The shared block must not alias an output array.
 * The host call uploads the shared block once per device and sends only theta_var (and warm
 * starts) through the chunk pipeline.  QP family with MCPX_LINSOLVE_SCHUR on one wave: the
 * kernels read the two blocks in place.  Every other combination: θ′ is materialised on the
 * device, a slice of at most MCPX_EXPAND_MB MiB (environment, default 256) at a time, and
 * the kernels of the full-θ call run on each slice. */
int mcpx_solve_batch_shared(const mcpx_desc* desc, const double* theta_shared, const double* theta_var,
                            const double* x0, const double* y0, const double* s0,
                            const mcpx_params* prm, int num_devices, mcpx_out* out);
/* The same on device buffers of the current device, enqueued on `stream`. */
int mcpx_solve_batch_shared_device(const mcpx_desc* desc, const double* theta_shared, const double* theta_var,
                                   const double* x0, const double* y0, const double* s0,
                                   const mcpx_params* prm, const mcpx_out* out, void* stream);

/* Page-lock a caller-owned host range (hipHostRegister, all devices) so that the
 * host-buffer calls read it by asynchronous DMA; optional, for long-lived θ
 * batches.  The range must stay allocated until mcpx_host_unregister(ptr).
 * MCPX_OK, MCPX_EINVAL (NULL / empty), MCPX_EHIP. */
int mcpx_host_register(void* ptr, size_t bytes);
int mcpx_host_unregister(void* ptr);

/* Device-buffer batched solve on the current device: every pointer in the
 * call (theta, x0/y0/s0 and every mcpx_out array) is device memory.
 * Enqueued on `stream` (a hipStream_t; NULL = default stream); returns
 * without synchronising.  This is the hot path the benchmark times. */
int mcpx_solve_batch_device(const mcpx_desc* desc, const double* theta,
                            const double* x0, const double* y0, const double* s0,
                            const mcpx_params* prm, const mcpx_out* out,
                            void* stream);


/* ---------------------------------------------------------------------------
 * Sensitivities of a solution w.r.t. θ (reference src/AutoDiff.jl).
 *
 * The reference differentiates F(z; θ) = 0 at the returned iterate:
 *     ∂z/∂θ = −(∇F_z)⁻¹ ∇F_θ      (src/AutoDiff.jl:18-40; `qr(−∇F_z, ColumnNorm()) \ ∇F_θ`)
 * with ∇F_z WITHOUT the tol·I regularisation, at the final (x, y, s)
 * (SURVEY.md Appendix A.10).  For both families ∇F_z and ∇F_θ do not depend on ϵ.
 * The kernels solve the same square system by dense LU with partial pivoting:
 * the JVP factors the full (n+2m)-dim ∇F_z, the VJP the (n+m)-dim system left
 * after eliminating λ_s of ∇F_zᵀ exactly through its −1 entries (no division);
 * for a nonsingular ∇F_z that equals the reference's pivoted-QR solve up to
 * rounding (amplified by cond(∇F_z), which is large at degenerate solutions).  An exactly zero
 * pivot (∇F_z singular, where the reference's QR would return a basic
 * least-squares solution) is reported per instance: status[b] = 1 and the
 * instance's outputs are NaN.
 *
 * Reverse mode — the ChainRulesCore.rrule pullback (src/AutoDiff.jl:42-82):
 *     ∂θ = (∂z/∂θ)ᵀ [∂l/∂x; ∂l/∂y; ∂l/∂s] = −∇F_θᵀ λ,  ∇F_zᵀ λ = [∂l/∂x; ∂l/∂y; ∂l/∂s].
 * Inputs (instance-major): θ (stride theta_ld), x [B*n], y [B*m], s [B*m],
 * gx [B*n], gy [B*m], gs [B*m] (any of gx/gy/gs may be NULL = zero cotangent,
 * ChainRulesCore's ZeroTangent).  Output: dtheta [B*p] (p = mcpx_theta_dim,
 * dense stride p, the family's θ layout), status [B] or NULL.
 * n + 2m <= MCPX_MAX_KKT_DIM runs one wave per instance (the system in registers),
 * larger systems up to MCPX_MAX_WG_KKT_DIM one workgroup per instance: blocked LU
 * with partial pivoting and MFMA trailing updates, on a per-slot HBM workspace
 * holding [K | rhs] (the register-resident LU of the solve kernels, lu_vr.hpp, is
 * not used by the sensitivity kernels); both give the same bits. */
int mcpx_vjp_batch(const mcpx_desc* desc, const double* theta, const double* x, const double* y,
                   const double* s, const double* gx, const double* gy, const double* gs,
                   int num_devices, double* dtheta, int32_t* status);
/* Same on device buffers of the current device, enqueued on `stream`. */
int mcpx_vjp_batch_device(const mcpx_desc* desc, const double* theta, const double* x,
                          const double* y, const double* s, const double* gx, const double* gy,
                          const double* gs, double* dtheta, int32_t* status, void* stream);

/* Solve and pullback in one call — the rrule of solve (src/AutoDiff.jl:42-82) applied
 * at the returned iterate, for a loss whose cotangent is given per block as
 *     ∂l/∂x = ax·x + bx,  ∂l/∂y = ay·y + by,  ∂l/∂s = as·s + bs
 * (b arrays [B*n] / [B*m] on the device, NULL = 0; a = 0 with b = NULL is
 * ChainRulesCore's ZeroTangent; a·z + b is rounded twice, no fma).  The AD test's
 * f = Σx² + Σy² (test/runtests.jl:72-75) is {ax = 2, ay = 2, as = 0, NULLs}. */
typedef struct mcpx_cotangent {
  double ax, ay, as;
  const double* bx; /* [B*n] or NULL */
  const double* by; /* [B*m] or NULL */
  const double* bs; /* [B*m] or NULL */
} mcpx_cotangent;

/* mcpx_solve_batch_device into `out`, then the pullback of `ct` at the solution into
 * dtheta [B*p] / vjp_status [B] (or NULL), device buffers of the current device,
 * enqueued on `stream`.  For the QP family with linear_solver = SCHUR at the
 * compiled (n, m) of the benchmarks ((2,2), (16,8), (32,16)) the pullback runs in
 * the epilogue of the solve kernel (one launch, the iterate never leaves the wave);
 * every other configuration runs the solve and mcpx_vjp_batch_device on `stream`.
 * Both give the bits of mcpx_solve_batch_device followed by mcpx_vjp_batch_device
 * with gx = ax·x + bx, gy = ay·y + by, gs = as·s + bs. */
int mcpx_solve_vjp_batch_device(const mcpx_desc* desc, const double* theta,
                                const double* x0, const double* y0, const double* s0,
                                const mcpx_params* prm, const mcpx_out* out,
                                const mcpx_cotangent* ct, double* dtheta,
                                int32_t* vjp_status, void* stream);

/* Conditioning of the pullback's matrix.  The reference's rrule solves with a column-pivoted QR
 * of −∇F_z (src/AutoDiff.jl:39); at degenerate solutions ∇F_z is nearly singular and QR and LU
 * sensitivities can differ at O(1).  rcond[b] = 1 / (‖∇F_z‖₁ · est‖∇F_z⁻¹‖₁) at (x, y, s), ∇F_z
 * without tol·I: the Hager–Higham estimate (≤ 5 rounds of solves with the LU factors and
 * their transpose, plus the alternating-sign lower bound), which never exceeds the true
 * ‖∇F_z⁻¹‖₁, so rcond[b] ≥ 1 / cond₁(∇F_z).  status[b] = 1 and rcond[b] = 0: ∇F_z exactly
 * singular.  A caller flags an instance as ill-conditioned when rcond[b] < its threshold
 * (mcp_amd.batch.ILL_CONDITIONED = 1e-12: fewer than ~4 significant digits in the
 * sensitivities).  Every size runs one workgroup per instance (n + 2m <= MCPX_MAX_WG_KKT_DIM). */
int mcpx_cond_batch(const mcpx_desc* desc, const double* theta, const double* x, const double* y,
                    const double* s, int num_devices, double* rcond, int32_t* status);
int mcpx_cond_batch_device(const mcpx_desc* desc, const double* theta, const double* x, const double* y,
                           const double* s, double* rcond, int32_t* status, void* stream);

/* Forward mode — the ForwardDiff.Dual method of solve (src/AutoDiff.jl:84-117):
 *     ż_c = (∂z/∂θ) θ̇_c = −(∇F_z)⁻¹ (∇F_θ θ̇_c),   c = 0 .. n_partials−1.
 * theta_dot [B*n_partials*p] (instance-major, then partial-major, stride p);
 * zdot [B*n_partials*(n+2m)], z = [x; y; s] ordering (src/mcp.jl:74);
 * status [B] or NULL.  One factorisation of ∇F_z serves up to
 * MCPX_JVP_RHS partials at a time. */
#define MCPX_JVP_RHS 8
int mcpx_jvp_batch(const mcpx_desc* desc, const double* theta, const double* x, const double* y,
                   const double* s, int32_t n_partials, const double* theta_dot, int num_devices,
                   double* zdot, int32_t* status);
int mcpx_jvp_batch_device(const mcpx_desc* desc, const double* theta, const double* x,
                          const double* y, const double* s, int32_t n_partials,
                          const double* theta_dot, double* zdot, int32_t* status, void* stream);

/* Sensitivities of a shared-matrix batch (mcpx_solve_batch_shared*; QP and affine families)
 * with respect to the per-instance block only.  `theta_shared` is the one matrix block; the
 * calls take no theta_var: for these families ∇F_z holds M, A (affine: P, Q, R, S) and the
 * iterate, none of b, ϕ (g, h), so nothing per instance is read from θ′.  The gradient of the
 * per-instance block is λ itself (QP: ∂b = λ_y, ∂ϕ = λ_x; affine: ∂g = −λ_x, ∂h = −λ_y), and the
 * rank-1 matrix blocks of the full record are neither formed nor stored.
 *   dvar    [B × var_dim], dense stride var_dim = mcpx_theta_var_dim, in the layout of the tail
 *           of the family's θ′: QP [∂b; ∂ϕ], affine [∂g; ∂h];
 *   var_dot [B × n_partials × var_dim], the tangents of the per-instance block.
 * desc->theta_ld is checked as in the shared solve (>= var_dim); only the fused call reads it,
 * as the stride of theta_var.
 * Contracts:
 *   VJP    dvar[b] and status[b] equal dtheta[b][shared_dim:] and status[b] of
 *          mcpx_vjp_batch[_device] on the materialised θ′, entry for entry, the NaN row of a
 *          singular instance included.
 *   JVP    zdot and status equal those of mcpx_jvp_batch[_device] with θ̇ = [0 … 0 ‖ var_dot],
 *          for every instance whose x, y, s are finite.  The full call multiplies the zero
 *          matrix tangent by the iterate (fma(0, z, acc)), which turns a non-finite entry of
 *          x or y into NaN right-hand sides; the split call does not run those chains, so
 *          there its right-hand sides are −(∇F_θ θ̇) of the per-instance block alone and a
 *          non-finite iterate reaches the result only through the rows of ∇F_z that hold it.
 *          That case is outside the contract.
 *   fused  every mcpx_out field equals mcpx_solve_batch_shared_device; dvar and vjp_status
 *          equal mcpx_vjp_batch_shared_device at that iterate with g = a ⊙ z + b (the rule of
 *          mcpx_solve_vjp_batch_device).  QP family, SCHUR, at (2,2), (16,8), (32,16): one
 *          launch with the pullback in the solve kernel's epilogue; every other configuration:
 *          the shared solve, then the split pullback on out->x / y / s.
 * The host calls upload the shared block once per device and no per-instance θ, and bring back
 * var_dim doubles per instance; num_devices and MCPX_HOST_SHARDS are those of mcpx_vjp_batch.
 * Errors, the empty batch, the size limit (MCPX_MAX_WG_KKT_DIM) and MCPX_ENODEV are as in the
 * full-θ sensitivity calls; MCPX_FAMILY_NONLINEAR: MCPX_EINVAL.  (The tangents of the shared
 * block and the condition estimate on a split θ: mcpx_jvp_batch_shared_dot and
 * mcpx_cond_batch_shared below.)  Added under 2.2.0 without a version step, as the shared solve
 * entries. */
int mcpx_vjp_batch_shared(const mcpx_desc* desc, const double* theta_shared, const double* x, const double* y,
                          const double* s, const double* gx, const double* gy, const double* gs,
                          int num_devices, double* dvar, int32_t* status);
int mcpx_vjp_batch_shared_device(const mcpx_desc* desc, const double* theta_shared, const double* x,
                                 const double* y, const double* s, const double* gx, const double* gy,
                                 const double* gs, double* dvar, int32_t* status, void* stream);
int mcpx_jvp_batch_shared(const mcpx_desc* desc, const double* theta_shared, const double* x, const double* y,
                          const double* s, int32_t n_partials, const double* var_dot, int num_devices,
                          double* zdot, int32_t* status);
int mcpx_jvp_batch_shared_device(const mcpx_desc* desc, const double* theta_shared, const double* x,
                                 const double* y, const double* s, int32_t n_partials,
                                 const double* var_dot, double* zdot, int32_t* status, void* stream);
int mcpx_solve_vjp_batch_shared_device(const mcpx_desc* desc, const double* theta_shared,
                                       const double* theta_var, const double* x0, const double* y0,
                                       const double* s0, const mcpx_params* prm, const mcpx_out* out,
                                       const mcpx_cotangent* ct, double* dvar, int32_t* vjp_status,
                                       void* stream);

/* Forward mode along a direction of the SHARED block as well — the forward-mode twin of the
 * reduced gradient below, for a caller who moves the shared weights (a line search over a weight
 * update, a Gauss-Newton product, a forward-mode check of mcpx_vjp_batch_shared_reduce):
 *     θ̇_{b,c} = [shared_dot_c ‖ var_dot_{b,c}],   c = 0 .. n_partials−1.
 *   shared_dot [n_partials × mcpx_theta_shared_dim], dense, given ONCE for the batch: partial c
 *              of every instance has the same matrix tangent.  Required (NULL with batch > 0 and
 *              n_partials > 0: MCPX_EINVAL);
 *   var_dot    [B × n_partials × var_dim] as in mcpx_jvp_batch_shared, or NULL = +0.0 tangents
 *              of the per-instance block;
 *   zdot, status as in mcpx_jvp_batch_shared.
 * Contract: zdot and status are bit-identical to mcpx_jvp_batch[_device] on the materialised θ′
 * and θ̇, for EVERY instance: the NaN rows and status 1 of a singular ∇F_z, and non-finite
 * iterates too — the matrix-tangent chains of the right-hand side really run here
 * (fma(±Ṁ_ij, x_j, acc) …: the x-block chain, the y-block chain, then the vector term), so the
 * "outside the contract" clause of mcpx_jvp_batch_shared does not apply.  With var_dot NULL the
 * last step still runs on +0.0 (QP: acc − (+0.0); affine: acc + (+0.0), which is not the
 * identity on acc = −0.0).
 * The caller allocates K·shared_dim + B·K·var_dim doubles of tangents in place of B·K·p.  The
 * host call uploads the shared block and shared_dot once per device, sends the iterate (and
 * var_dot, if given) per shard and brings back zdot; num_devices and MCPX_HOST_SHARDS are those
 * of mcpx_jvp_batch.  Errors, the empty batch, MCPX_ENODEV, the size limit, the theta_ld ≥
 * var_dim check, MCPX_FAMILY_NONLINEAR → MCPX_EINVAL and n_partials ≤ 0 (negative: MCPX_EINVAL;
 * 0: status only, shared_dot not read) as in mcpx_jvp_batch_shared.  Added under 2.2.0 without a
 * version step, as the other shared entries. */
int mcpx_jvp_batch_shared_dot(const mcpx_desc* desc, const double* theta_shared, const double* x, const double* y,
                              const double* s, int32_t n_partials, const double* shared_dot,
                              const double* var_dot, int num_devices, double* zdot, int32_t* status);
int mcpx_jvp_batch_shared_dot_device(const mcpx_desc* desc, const double* theta_shared, const double* x,
                                     const double* y, const double* s, int32_t n_partials,
                                     const double* shared_dot, const double* var_dot, double* zdot,
                                     int32_t* status, void* stream);

/* mcpx_cond_batch of a shared-matrix batch: ∇F_z reads nothing per instance from θ′, so the
 * call takes the one matrix block.  rcond and status are bit-identical to
 * mcpx_cond_batch[_device] on the materialised θ′ (the same workgroup kernels, reading every
 * instance's rows of ∇F_z from theta_shared).  The host call uploads the shared block once per
 * device and brings back one double per instance.  Errors as the other shared sensitivity
 * entries.  Added under 2.2.0 without a version step. */
int mcpx_cond_batch_shared(const mcpx_desc* desc, const double* theta_shared, const double* x, const double* y,
                           const double* s, int num_devices, double* rcond, int32_t* status);
int mcpx_cond_batch_shared_device(const mcpx_desc* desc, const double* theta_shared, const double* x,
                                  const double* y, const double* s, double* rcond, int32_t* status,
                                  void* stream);

/* The reduced gradient of the SHARED block of a shared-matrix batch: Σ_b of the matrix blocks of
 * the full pullback record, for a caller whose matrices are weights shared by every instance of
 * the batch (an optimisation layer: ∂weights = Σ_b ∂θ′_b over the shared block).  The call runs
 * mcpx_vjp_batch_shared[_device] and contracts its λ (= dvar) with the iterate over the batch
 * axis on the matrix cores; no per-instance record of the matrix block is formed or stored.
 *   skip     [B] or NULL: instance b is left out of the sum when skip[b] != 0 (e.g. the solve's
 *            status, to leave out failed solves);
 *   dshared  [mcpx_theta_shared_dim], the layout of the shared block;
 *   used     the number of instances summed;
 *   dvar     [B × var_dim] or NULL, status [B] or NULL: exactly what mcpx_vjp_batch_shared[_device]
 *            returns for the same inputs (skip does not touch them).
 * Contract — one defined bit pattern:
 *   chunks     instance b of the whole call belongs to chunk c = b / MCPX_REDUCE_CHUNK; the last
 *              chunk may be short.
 *   inclusion  b is included when (skip == NULL or skip[b] == 0) and its pullback status is 0.
 *              For an excluded instance every multiplication operand taken from it (x, y, λ) is
 *              replaced by +0.0; the chain still runs.  A NaN row of a singular ∇F_z, or the
 *              non-finite iterate of a failed solve, therefore never reaches the sum.  Such a
 *              step, fma(+0.0, +0.0, acc), returns acc except that it turns an accumulator of
 *              −0.0 into +0.0; an implementation may run further steps of this kind (the kernels
 *              pad a short chunk with them).  Neither can show in dshared: the fold starts from
 *              +0.0, and +0.0 + (−0.0) = +0.0 + (+0.0).
 *   entries    per chunk and entry: acc = +0.0, instances ascending, every step an fma.
 *              QP, λy = dvar[b][:m] (∂b), λx = dvar[b][m:] (∂ϕ):
 *                ∂M_ij  acc = fma(−λx_i, x_j, acc)
 *                ∂A_kj  acc = fma(−λy_k, x_j, acc), then acc = fma(λx_j, y_k, acc)
 *              (with B = 1 the full record's entries).  Affine, ∂g = dvar[b][:n], ∂h = dvar[b][n:]:
 *                ∂P_ij  fma(∂g_i, x_j, acc)     ∂Q_ik  fma(∂g_i, y_k, acc)
 *                ∂R_kj  fma(∂h_k, x_j, acc)     ∂S_kq  fma(∂h_k, y_q, acc)
 *   fold       dshared = ((+0.0 + P₀) + P₁) + P₂ …, the chunk partials in ascending chunk order,
 *              plain additions.
 * The bits do not depend on num_devices, MCPX_HOST_SHARDS, MCPX_HOST_CHUNK, the launch geometry,
 * or which kernel produced λ.  The host call cuts its shards at multiples of MCPX_REDUCE_CHUNK
 * (for this entry only), uploads the shared block once per device, and folds the shards' chunk
 * partials in global chunk order.  Sizes: every (n, m) of the split pullback, m = 0 included.
 * Errors and MCPX_ENODEV as mcpx_vjp_batch_shared*; NULL dshared or used: MCPX_EINVAL; an empty
 * batch gives dshared = +0.0 throughout and used = 0 (the host call then needs no device).
 * Added under 2.2.0 without a version step, as the other shared entries. */
#define MCPX_REDUCE_CHUNK 64
int mcpx_vjp_batch_shared_reduce(const mcpx_desc* desc, const double* theta_shared, const double* x,
                                 const double* y, const double* s, const double* gx, const double* gy,
                                 const double* gs, const uint8_t* skip, int num_devices, double* dshared,
                                 int64_t* used, double* dvar, int32_t* status);
/* The same on device buffers of the current device (dshared and used included), enqueued on
 * `stream`; with dvar (status) NULL the pullback writes into a block of the library's own. */
int mcpx_vjp_batch_shared_reduce_device(const mcpx_desc* desc, const double* theta_shared, const double* x,
                                        const double* y, const double* s, const double* gx, const double* gy,
                                        const double* gs, const uint8_t* skip, double* dshared, int64_t* used,
                                        double* dvar, int32_t* status, void* stream);

/* ---------------------------------------------------------------------------
 * Grouped shared-matrix batches: G matrix blocks, each shared by a run of instances (several
 * heads of a QP layer in one minibatch, G hypotheses with S sampled right-hand sides each, G plants
 * under one MPC formulation).  Between the full-θ calls (one block per instance) and the shared
 * calls (one block per batch), in ONE call at the batch's full occupancy.
 *   theta_shared   G blocks: block g is mcpx_theta_shared_dim doubles at theta_shared + g·shared_ld,
 *                  shared_ld >= shared_dim; the padding is never read;
 *   group_offsets  G + 1 offsets in HOST memory (in the _device forms too: metadata, like desc):
 *                  group g owns the instances [off[g], off[g+1]); off[0] = 0, off[G] = batch,
 *                  non-decreasing (empty groups are allowed).  Read before the call returns; the
 *                  library builds its device-side lookup (one int32 per instance) from it in a block
 *                  of its own, in stream order;
 *   theta_var      [b; ϕ] / [g; h] per instance, stride desc->theta_ld, as in the shared calls.
 * Families: QP and affine (MCPX_FAMILY_NONLINEAR: MCPX_EINVAL).  MCPX_EINVAL also for NULL
 * theta_shared or group_offsets with batch > 0, num_groups < 0 (or 0 with batch > 0), offsets that
 * decrease or do not run from 0 to batch, shared_ld / dshared_ld < shared_dim, and the NULL outputs
 * the shared twins reject.  num_groups is bounded by the batch and int32 only.  Warm starts, params,
 * outputs, size limits, kernel selection, MCPX_ENODEV, MCPX_HOST_CHUNK / _BUFFERS / _SHARDS and
 * num_devices are those of the shared twins; the host calls upload all G blocks once per device, and
 * theta_var, the warm starts and the lookup go through the chunk pipeline.
 * Contracts (bitwise):
 *   solve   every mcpx_out field of instance b of group g is that of mcpx_solve_batch[_device] on
 *           θ′_b = [block g ‖ var_b], which is also mcpx_solve_batch_shared* on group g alone;
 *   vjp     dvar[b], status[b] are those of mcpx_vjp_batch_shared* on group g alone;
 *   reduce  dshared + g·dshared_ld [shared_dim] and used[g] are those of mcpx_vjp_batch_shared_reduce*
 *           on group g alone: chunks of MCPX_REDUCE_CHUNK instances counted from off[g], the same
 *           inclusion rule, entries and fold; an empty group gives +0.0 throughout and used[g] = 0;
 *           the padding of dshared is not written.  dvar / status: those of the grouped vjp.  The
 *           bits do not depend on devices, shards (cut at chunk boundaries), host chunks, launch
 *           geometry or MCPX_REDUCE_CAP_KB.  An empty batch needs no device in the host call.
 * No grouped JVP, shared_dot, cond or fused solve+VJP entry: a grouped solve followed by a grouped
 * vjp is the composed route.  Added under 2.2.0 without a version step, as the shared entries. */
int mcpx_solve_batch_grouped(const mcpx_desc* desc, const double* theta_shared, int64_t shared_ld,
                             int32_t num_groups, const int64_t* group_offsets, const double* theta_var,
                             const double* x0, const double* y0, const double* s0, const mcpx_params* prm,
                             int num_devices, mcpx_out* out);
int mcpx_solve_batch_grouped_device(const mcpx_desc* desc, const double* theta_shared, int64_t shared_ld,
                                    int32_t num_groups, const int64_t* group_offsets, const double* theta_var,
                                    const double* x0, const double* y0, const double* s0, const mcpx_params* prm,
                                    const mcpx_out* out, void* stream);
int mcpx_vjp_batch_grouped(const mcpx_desc* desc, const double* theta_shared, int64_t shared_ld, int32_t num_groups,
                           const int64_t* group_offsets, const double* x, const double* y, const double* s,
                           const double* gx, const double* gy, const double* gs, int num_devices, double* dvar,
                           int32_t* status);
int mcpx_vjp_batch_grouped_device(const mcpx_desc* desc, const double* theta_shared, int64_t shared_ld,
                                  int32_t num_groups, const int64_t* group_offsets, const double* x,
                                  const double* y, const double* s, const double* gx, const double* gy,
                                  const double* gs, double* dvar, int32_t* status, void* stream);
int mcpx_vjp_batch_grouped_reduce(const mcpx_desc* desc, const double* theta_shared, int64_t shared_ld,
                                  int32_t num_groups, const int64_t* group_offsets, const double* x,
                                  const double* y, const double* s, const double* gx, const double* gy,
                                  const double* gs, const uint8_t* skip, int num_devices, double* dshared,
                                  int64_t dshared_ld, int64_t* used, double* dvar, int32_t* status);
int mcpx_vjp_batch_grouped_reduce_device(const mcpx_desc* desc, const double* theta_shared, int64_t shared_ld,
                                         int32_t num_groups, const int64_t* group_offsets, const double* x,
                                         const double* y, const double* s, const double* gx, const double* gy,
                                         const double* gs, const uint8_t* skip, double* dshared,
                                         int64_t dshared_ld, int64_t* used, double* dvar, int32_t* status,
                                         void* stream);

/* ---------------------------------------------------------------------------
 * Nonlinear G/H — MCPX_FAMILY_NONLINEAR (BASELINE C4: games, src/game.jl).
 *
 * The reference compiles F!/∇F_z! from Symbolics expressions once per problem
 * (build_function, src/mcp.jl:82-120).  The front-end does the same for the
 * GPU (mcp_amd/codegen.py): straight-line device code for G, H and their
 * Jacobian blocks, compiled with the solver template
 * (mcp_amd/csrc/ipm_nl_kernel.hpp) into one gfx950 code object per problem.
 * These calls load and run it.  A module holds the kernels its size admits:
 * one-wave MCPX_LINSOLVE_SCHUR (∂H/∂y ≡ 0, n ≤ 64, m ≤ 128), _REDUCED
 * (n + m ≤ 64), _DENSE (n + 2m ≤ 64), and workgroup-per-instance kernels of
 * each of them (SCHUR: ∂H/∂y ≡ 0) whose LDS footprint fits
 * (e.g. the lane change at T = 10: n = 200, m = 250, KKT dimension 700), and
 * the one-wave band SCHUR kernel when the reordered Schur complement has a
 * narrow band (MCPX_KERNEL_BAND); another linear_solver is MCPX_EUNSUPPORTED.
 * The sensitivity kernels reach further than the workgroup solve kernels: their
 * blocked LU keeps a panel of 16, 8 or 4 columns in LDS, the widest that fits
 * (the lane change at T = 30, n = 600, m = 750: 8 columns for the pullback's
 * 1350 rows, 4 for the tangents' 2100).  The width changes no bit of a result.
 */
typedef struct mcpx_module mcpx_module;
/* Sensitivity kernels of a module (bits of the mcpx_module_dims kernel mask): set when a
 * panel of at least 4 columns of the factored system (VJP: n + m rows; JVP and the condition
 * estimate: n + 2m rows) fits the LDS, 24·(n+2m) + rows·(8·width + 7) + 512 <= 161792 bytes */
#define MCPX_MODULE_VJP 6
#define MCPX_MODULE_JVP 7
#define MCPX_MODULE_SCHUR_MW 8  /* the 4-wave SCHUR solve kernel (MCPX_KERNEL_MULTIWAVE) */
#define MCPX_MODULE_BAND 9       /* the band SCHUR solve kernel (MCPX_KERNEL_BAND) */
#define MCPX_MODULE_BAND_AUTO 10 /* MCPX_KERNEL_AUTO prefers the band kernel */
/* Loads the code object at `path` on the current device (other devices load
 * it on first use).  No usable GPU: MCPX_ENODEV. */
int mcpx_module_load(const char* path, mcpx_module** mod);
/* The module's n, m, θ dimension p and kernel mask: bit MCPX_LINSOLVE_* for the
 * one-wave kernels, bit 3 + MCPX_LINSOLVE_* for the workgroup kernels, bits
 * MCPX_MODULE_VJP / MCPX_MODULE_JVP for the sensitivity kernels; NULL pointers
 * are skipped. */
int mcpx_module_dims(const mcpx_module* mod, int32_t* n, int32_t* m, int32_t* p, int32_t* solvers);
void mcpx_module_unload(mcpx_module* mod);
/* mcpx_solve_batch / mcpx_solve_batch_device for the module's problem:
 * desc->family = MCPX_FAMILY_NONLINEAR, desc->n / m = the module's, theta_ld >= p. */
int mcpx_solve_batch_module(mcpx_module* mod, const mcpx_desc* desc, const double* theta,
                            const double* x0, const double* y0, const double* s0,
                            const mcpx_params* prm, int num_devices, mcpx_out* out);
int mcpx_solve_batch_module_device(mcpx_module* mod, const mcpx_desc* desc, const double* theta,
                                   const double* x0, const double* y0, const double* s0,
                                   const mcpx_params* prm, const mcpx_out* out, void* stream);

/* Sensitivities of the module's problem — the rrule pullback and the Dual method of
 * src/AutoDiff.jl for any PrimalDualMCP built with compute_sensitivities = true
 * (src/mcp.jl:122-147: ∇F_θ from the generated mcpx_nl_eval_theta), e.g. the
 * trajectory games of src/game.jl.  Same argument meaning as mcpx_vjp_batch /
 * mcpx_jvp_batch with p = the module's θ dimension; one workgroup per instance
 * (VJP: the (n+m)-dim reduced ∇F_zᵀ system, JVP: the (n+2m)-dim ∇F_z, blocked LU
 * with partial pivoting, panel of 16 / 8 / 4 columns by what fits the LDS).  A call takes
 * at most 4 GiB of workspace: systems whose slot is tens of MB run on fewer workgroups.
 * MCPX_EUNSUPPORTED when the module has no such kernel (mask bits MCPX_MODULE_VJP /
 * MCPX_MODULE_JVP: not even 4 columns fit). */
int mcpx_vjp_batch_module(mcpx_module* mod, const mcpx_desc* desc, const double* theta, const double* x,
                          const double* y, const double* s, const double* gx, const double* gy,
                          const double* gs, int num_devices, double* dtheta, int32_t* status);
int mcpx_vjp_batch_module_device(mcpx_module* mod, const mcpx_desc* desc, const double* theta,
                                 const double* x, const double* y, const double* s, const double* gx,
                                 const double* gy, const double* gs, double* dtheta, int32_t* status,
                                 void* stream);
int mcpx_jvp_batch_module(mcpx_module* mod, const mcpx_desc* desc, const double* theta, const double* x,
                          const double* y, const double* s, int32_t n_partials, const double* theta_dot,
                          int num_devices, double* zdot, int32_t* status);
int mcpx_jvp_batch_module_device(mcpx_module* mod, const mcpx_desc* desc, const double* theta,
                                 const double* x, const double* y, const double* s, int32_t n_partials,
                                 const double* theta_dot, double* zdot, int32_t* status, void* stream);
int mcpx_cond_batch_module(mcpx_module* mod, const mcpx_desc* desc, const double* theta, const double* x,
                           const double* y, const double* s, int num_devices, double* rcond, int32_t* status);
int mcpx_cond_batch_module_device(mcpx_module* mod, const mcpx_desc* desc, const double* theta,
                                  const double* x, const double* y, const double* s, double* rcond,
                                  int32_t* status, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* MCPX_H */

// sens_kernel.h — argument block and launchers of the sensitivity kernels
// (reference src/AutoDiff.jl): the reverse-mode pullback (rrule, :42-82) and the
// forward-mode Dual path (:84-117).  Shared by mcpx_api.cpp and sens_inst_*.hip.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/mcpx.h"

namespace mcpx {

struct SensArgs {
  const double* theta;
  int64_t theta_ld;
  const double* x;  // [B*n] solution (src/AutoDiff.jl:25 `(; x, y, s, ϵ) = solution`)
  const double* y;  // [B*m]
  const double* s;  // [B*m]
  const double* gx;  // VJP cotangents ∂l/∂x [B*n] (NULL = 0)
  const double* gy;  // ∂l/∂y [B*m]
  const double* gs;  // ∂l/∂s [B*m]
  const double* theta_dot;  // JVP tangents [B*K*p]
  double* out;              // VJP: dtheta [B*p]; JVP: zdot [B*K*(n+2m)]
  int32_t* status;          // [B] or NULL: 0 ok, 1 ∇F_z singular (outputs NaN)
  int64_t p;                // θ dimension of the family (dense stride of dtheta / theta_dot)
  int32_t n, m;
  int32_t n_partials;       // K (JVP)
  int32_t family;
  int32_t mode;             // workgroup JVP kernels: 1 = condition estimate (out = rcond [B], mcpx_cond_batch)
  int32_t pad_;
  // VJP cotangent g = a ⊙ z + b per block (b = gx / gy / gs above, NULL = 0): a = 0 is the
  // plain cotangent arrays; a ≠ 0 the gradient of a separable quadratic loss
  // l = Σ ½ a z² + b·z (e.g. a = 2, b = 0: f = Σx² + Σy², test/runtests.jl:72-75),
  // computed in the kernel as a·z + b (two roundings, no fma)
  double ga_x, ga_y, ga_s;
  // mcpx_jvp_batch_shared_dot*: the tangents of the shared matrix block, [K × shared_dim], the
  // same for every instance (theta_dot is then the per-instance block's, or NULL = +0.0).
  // Last, so that the kernels of generated modules built against this header are unaffected.
  const double* shared_dot;
  // mcpx_vjp_batch_grouped* (the SPLIT pullback kernels; NULL otherwise): instance b's matrix block
  // is theta + group_map[b]·shared_ld.
  const int32_t* group_map;
  int64_t shared_ld;
};

// Where a kernel's θ (and a JVP's θ̇) comes from.  kThetaFull: instance b's θ′ at
// theta + b·theta_ld, θ̇ [B × K × p].  kThetaSplit (a shared-matrix batch): theta is the ONE
// matrix block; the JVP takes the per-instance block's tangents only (the matrix block's are
// zero).  kThetaSplitDot (mcpx_jvp_batch_shared_dot*): as kThetaSplit, with the matrix block's
// tangents in shared_dot.
constexpr int kThetaFull = 0, kThetaSplit = 1, kThetaSplitDot = 2;

// One cotangent entry g = a·z + b (a = 0 → b, 0 when b is absent; b absent → a·z).
__device__ __forceinline__ double affine_ct(double a, double z, const double* b) {
  if (a == 0.0) return b ? *b : 0.0;
  return b ? a * z + *b : a * z;
}

// (∇F_θ θ̇)_i of a shared-matrix batch (mcpx_jvp_batch_shared*): the tangent of the matrix
// block is zero, so of dtheta_row() only its last step is left, on the +0.0 that the fma
// chains over a zero tangent and a finite iterate end in.  d: this partial's [ḃ; ϕ̇]
// (QP) or [ġ; ḣ] (affine), n + m doubles.
template <int FAMILY>
__device__ __forceinline__ double dvar_row(const double* __restrict__ d, int i, int n, int m) {
  const double acc = 0.0;
  if (i < n) return FAMILY == MCPX_FAMILY_QP ? acc - d[m + i] : acc + d[i];
  if (i < n + m) return FAMILY == MCPX_FAMILY_QP ? acc - d[i - n] : acc + d[n + (i - n)];
  return 0.0;
}

// One 64-lane wave per instance; nmax ∈ {8,16,24,32,48,64} ≥ n + 2m.
// hipErrorInvalidValue when no kernel matches.
hipError_t launch_vjp(int nmax, const SensArgs& a, int64_t batch, hipStream_t st);
hipError_t launch_jvp(int nmax, const SensArgs& a, int64_t batch, hipStream_t st);
// The same on a shared-matrix batch (mcpx_vjp_batch_shared*, mcpx_jvp_batch_shared*): a.theta is
// the ONE matrix block of every instance (a.theta_ld is not read), a.out the [B × (n+m)]
// gradient of the per-instance block / a.theta_dot its [B × K × (n+m)] tangents.
hipError_t launch_vjp_shared(int nmax, const SensArgs& a, int64_t batch, hipStream_t st);
hipError_t launch_jvp_shared(int nmax, const SensArgs& a, int64_t batch, hipStream_t st);
// The tangents of a shared-matrix batch along a direction of the shared block too
// (mcpx_jvp_batch_shared_dot*): a.shared_dot [K × shared_dim], a.theta_dot [B × K × (n+m)] or NULL.
hipError_t launch_jvp_shared_dot(int nmax, const SensArgs& a, int64_t batch, hipStream_t st);

// The reduced gradient of the shared block (mcpx_vjp_batch_shared_reduce*, shared_reduce.hip).
struct ReduceArgs {
  const double* x;        // [B*n]
  const double* y;        // [B*m]
  const double* dvar;     // [B*(n+m)]: the split pullback's output (λ)
  const int32_t* status;  // [B]: the split pullback's status
  const uint8_t* skip;    // [B] or NULL
  double* part;           // [chunks of the launch × ds]: the chunk partials
  int64_t* count;         // [chunks of the launch]: included instances per chunk
  int64_t batch;          // B: the arrays' instances; the last chunk may be short
  int64_t chunk0;         // the launch's first chunk (of MCPX_REDUCE_CHUNK instances)
  int64_t ds;             // mcpx_theta_shared_dim
  int32_t n, m;
  int32_t family;
  int32_t pad_;
};
// Partials of chunks [a.chunk0, a.chunk0 + nchunks) into a.part / a.count.
hipError_t launch_shared_reduce_partial(const ReduceArgs& a, int64_t nchunks, hipStream_t st);
// dshared / used ← (first ? 0 : their value) + the partials / counts, chunks ascending.
hipError_t launch_shared_reduce_fold(const double* part, const int64_t* count, int64_t nchunks, int64_t ds,
                                     bool first, double* dshared, int64_t* used, hipStream_t st);

// The reduced gradient per group of a grouped batch (mcpx_vjp_batch_grouped_reduce*, grouped_reduce.hip).
// A row of the chunk table: at most MCPX_REDUCE_CHUNK instances of one group, counted from the
// group's first instance; the chunks ascend with the instances, empty groups own none.
struct GroupChunk {
  int64_t first;  // the chunk's first instance (index into the whole batch)
  int32_t len;
  int32_t group;
};
struct GroupReduceArgs {
  ReduceArgs r;              // as above; the arrays' element 0 is instance inst0, r.chunk0 indexes `chunks`
  const GroupChunk* chunks;  // the rows of the table (device) that the call covers: the batch's, or a shard's
  int64_t inst0;
};
// dshared + g·dshared_ld [ds] ← +0.0 and used[g] ← 0 for g < G (the padding of dshared is not written).
hipError_t launch_grouped_reduce_zero(double* dshared, int64_t dshared_ld, int64_t ds, int64_t G, int64_t* used,
                                      hipStream_t st);
// Partials of chunks [a.r.chunk0, a.r.chunk0 + nchunks) into a.r.part / a.r.count.
hipError_t launch_grouped_reduce_partial(const GroupReduceArgs& a, int64_t nchunks, hipStream_t st);
// The partials / counts of chunks [c0, c0 + nchunks) added, ascending, to dshared + g·dshared_ld and
// used[g] of their groups g ∈ [g_lo, g_hi); cbase [G + 1] (device): group g owns the chunks
// [cbase[g], cbase[g + 1]).  Continues each group's chain from what dshared[g] / used[g] hold.
hipError_t launch_grouped_reduce_fold(const double* part, const int64_t* count, int64_t c0, int64_t nchunks,
                                      const int64_t* cbase, int64_t g_lo, int64_t g_hi, int64_t ds, double* dshared,
                                      int64_t dshared_ld, int64_t* used, hipStream_t st);

}  // namespace mcpx

// θ′ expansion for shared-matrix batches (mcpx_solve_batch_shared*): writes
// [shared ‖ var_i] for a slice of instances, so that every kernel without an in-kernel
// shared read (QP REDUCED / DENSE, the affine family, the workgroup kernels) runs on the
// slice unchanged.  Pure data movement: one 16-byte store per thread, consecutive threads on
// consecutive pairs of one instance's θ′ (coalesced along θ′); the shared block's reads hit L2
// after the first instance, so the kernel runs at the store bandwidth.
#include "ipm_kernel.h"

namespace mcpx {

namespace {

constexpr int kExpandThreads = 256;
constexpr int kExpandRows = 2048;  // most rows of blocks (grid.y) of one launch

// out_ld is even and `out` 16-byte aligned, so every pair (2q, 2q + 1) of a row is one aligned
// double2.  A row's last pair may reach one element past ds + dv (odd θ′ dimension): that
// element is padding inside out_ld and is written as 0.
__global__ __launch_bounds__(kExpandThreads) void theta_expand_kernel(const double* __restrict__ shared,
                                                                       const double* __restrict__ var,
                                                                       int64_t var_ld, double* __restrict__ out,
                                                                       int64_t out_ld, int64_t ds, int64_t dv,
                                                                       int64_t nb) {
  const int64_t q = (int64_t)blockIdx.x * kExpandThreads + threadIdx.x;  // pair index in the row
  const int64_t j = 2 * q;
  if (j >= out_ld) return;
  const int64_t pd = ds + dv;
  const bool s0 = j < ds, s1 = j + 1 < ds;
  const double c0 = s0 ? shared[j] : 0.0, c1 = s1 ? shared[j + 1] : 0.0;  // the same for every instance
  for (int64_t i = blockIdx.y; i < nb; i += gridDim.y) {
    const double* v = var + i * var_ld;  // read at [0, dv) only
    double2 w;
    w.x = s0 ? c0 : (j < pd ? v[j - ds] : 0.0);
    w.y = s1 ? c1 : (j + 1 < pd ? v[j + 1 - ds] : 0.0);
    *reinterpret_cast<double2*>(out + i * out_ld + j) = w;
  }
}

// A grouped batch (mcpx_solve_batch_grouped*): instance i's head is the block of its group,
// shared + map[i]·shared_ld.  The pair of the block is read per instance (a run of instances of one
// group reads it from L2); the slice may straddle group boundaries.
__global__ __launch_bounds__(kExpandThreads) void theta_expand_grouped_kernel(
    const double* __restrict__ shared, int64_t shared_ld, const int32_t* __restrict__ map,
    const double* __restrict__ var, int64_t var_ld, double* __restrict__ out, int64_t out_ld, int64_t ds, int64_t dv,
    int64_t nb) {
  const int64_t q = (int64_t)blockIdx.x * kExpandThreads + threadIdx.x;  // pair index in the row
  const int64_t j = 2 * q;
  if (j >= out_ld) return;
  const int64_t pd = ds + dv;
  const bool s0 = j < ds, s1 = j + 1 < ds;
  for (int64_t i = blockIdx.y; i < nb; i += gridDim.y) {
    const double* sh = shared + (int64_t)map[i] * shared_ld;  // read at [0, ds) only
    const double* v = var + i * var_ld;                       // read at [0, dv) only
    double2 w;
    w.x = s0 ? sh[j] : (j < pd ? v[j - ds] : 0.0);
    w.y = s1 ? sh[j + 1] : (j + 1 < pd ? v[j + 1 - ds] : 0.0);
    *reinterpret_cast<double2*>(out + i * out_ld + j) = w;
  }
}

}  // namespace

hipError_t launch_theta_expand_grouped(const double* shared, int64_t shared_ld, const int32_t* map, const double* var,
                                       int64_t var_ld, double* out, int64_t out_ld, int64_t ds, int64_t dv,
                                       int64_t nb, hipStream_t st) {
  if (nb <= 0) return hipSuccess;
  if (out_ld < ds + dv || (out_ld & 1) || ((uintptr_t)out & 15) || shared_ld < ds || !map) return hipErrorInvalidValue;
  const int64_t gx = (out_ld / 2 + kExpandThreads - 1) / kExpandThreads;
  if (gx > 0x7fffffff) return hipErrorInvalidValue;
  const int64_t gy = nb < kExpandRows ? nb : kExpandRows;
  hipLaunchKernelGGL(theta_expand_grouped_kernel, dim3((unsigned)gx, (unsigned)gy), dim3(kExpandThreads), 0, st, shared,
                     shared_ld, map, var, var_ld, out, out_ld, ds, dv, nb);
  return hipGetLastError();
}

hipError_t launch_theta_expand(const double* shared, const double* var, int64_t var_ld, double* out, int64_t out_ld,
                               int64_t ds, int64_t dv, int64_t nb, hipStream_t st) {
  if (nb <= 0) return hipSuccess;
  if (out_ld < ds + dv || (out_ld & 1) || ((uintptr_t)out & 15)) return hipErrorInvalidValue;
  const int64_t pairs = out_ld / 2;
  const int64_t gx = (pairs + kExpandThreads - 1) / kExpandThreads;
  if (gx > 0x7fffffff) return hipErrorInvalidValue;
  // instances over grid.y: at most kExpandRows rows of blocks, each striding over the rest with
  // its pair of the shared block held in registers (a row of blocks per instance made the launch
  // 262,144 blocks of one 4 KB row each at C3: dispatch-bound at 0.5 TB/s)
  const int64_t gy = nb < kExpandRows ? nb : kExpandRows;
  hipLaunchKernelGGL(theta_expand_kernel, dim3((unsigned)gx, (unsigned)gy), dim3(kExpandThreads), 0, st, shared, var,
                     var_ld, out, out_ld, ds, dv, nb);
  return hipGetLastError();
}

}  // namespace mcpx

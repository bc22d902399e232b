// Shared-matrix batches with the rrule pullback fused into the solve's epilogue
// (mcpx_solve_vjp_batch_shared_device): the SCHUR QP kernels of ipm_inst_fused.hip with the
// SHARED flag — one [vec(M); vec(A)] block for the whole batch, [b; ϕ] per instance read,
// [∂b; ∂ϕ] per instance written.  README QP (2, 2), C2 (16, 8), C3/C5 (32, 16).
#include "sens_kernel_impl.hpp"

namespace mcpx {

hipError_t launch_ipm_shared_fused_vjp(int n, int m, const KernelArgs& a, int64_t batch, hipStream_t st) {
  if (n == 2 && m == 2) return launch_one<2, 0, 2, 2, MCPX_LINSOLVE_SCHUR, 8, true>(a, batch, st);
  if (n == 16 && m == 8) return launch_one<16, 0, 16, 8, MCPX_LINSOLVE_SCHUR, 24, true>(a, batch, st);
  if (n == 32 && m == 16) return launch_one<32, 0, 32, 16, MCPX_LINSOLVE_SCHUR, 48, true>(a, batch, st);
  return hipErrorNotFound;
}

}  // namespace mcpx

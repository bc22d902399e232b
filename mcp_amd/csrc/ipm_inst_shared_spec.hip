// Shared-matrix batches, compile-time (n, m): the QP family's SCHUR solve of ipm_inst_spec.hip
// with the SHARED flag — one [vec(M); vec(A)] block for the whole batch, [b; ϕ] per instance
// (mcpx_solve_batch_shared*).  README QP (2, 2), C2 (16, 8), C3 (32, 16).
#include "ipm_kernel_impl.hpp"

namespace mcpx {

hipError_t launch_ipm_shared_spec(int n, int m, const KernelArgs& a, int64_t batch, hipStream_t st) {
  if (n == 2 && m == 2) return launch_one<2, 0, 2, 2, MCPX_LINSOLVE_SCHUR, 0, true>(a, batch, st);
  if (n == 16 && m == 8) return launch_one<16, 0, 16, 8, MCPX_LINSOLVE_SCHUR, 0, true>(a, batch, st);
  if (n == 32 && m == 16) return launch_one<32, 0, 32, 16, MCPX_LINSOLVE_SCHUR, 0, true>(a, batch, st);
  return hipErrorNotFound;
}

}  // namespace mcpx

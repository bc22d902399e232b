// Shared-matrix batches, runtime (n, m): the QP family's SCHUR solve of ipm_inst_schur_qp.hip
// with the SHARED flag — one [vec(M); vec(A)] block for the whole batch, [b; ϕ] per instance
// (mcpx_solve_batch_shared*; nmax = register-row width ≥ n).
#include "ipm_kernel_impl.hpp"

namespace mcpx {

hipError_t launch_ipm_shared_schur(int nmax, const KernelArgs& a, int64_t batch, hipStream_t st) {
  switch (nmax) {
    case 8: return launch_one<8, 0, 0, 0, MCPX_LINSOLVE_SCHUR, 0, true>(a, batch, st);
    case 16: return launch_one<16, 0, 0, 0, MCPX_LINSOLVE_SCHUR, 0, true>(a, batch, st);
    case 24: return launch_one<24, 0, 0, 0, MCPX_LINSOLVE_SCHUR, 0, true>(a, batch, st);
    case 32: return launch_one<32, 0, 0, 0, MCPX_LINSOLVE_SCHUR, 0, true>(a, batch, st);
    case 48: return launch_one<48, 0, 0, 0, MCPX_LINSOLVE_SCHUR, 0, true>(a, batch, st);
    case 64: return launch_one<64, 0, 0, 0, MCPX_LINSOLVE_SCHUR, 0, true>(a, batch, st);
    default: return hipErrorInvalidValue;
  }
}

}  // namespace mcpx

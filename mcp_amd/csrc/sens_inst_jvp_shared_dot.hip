// jvp_kernel instantiations with SPLIT = kThetaSplitDot (sens_kernel_impl.hpp) for
// NMAX ∈ {8,16,24,32,48,64} ≥ n + 2m, QP and affine families: the tangents of a
// shared-matrix batch along a direction of the shared block too (mcpx_jvp_batch_shared_dot*) —
// rows of ∇F_z from the one matrix block, right-hand sides from the one [K × shared_dim] block
// of matrix tangents (dtheta_row's fma chains) and the per-instance block's tangents or +0.0.
#include "sens_kernel_impl.hpp"

namespace mcpx {

namespace {
template <int NMAX>
hipError_t go_jvp_shared_dot(const SensArgs& a, int64_t batch, hipStream_t st) {
  if (a.family == MCPX_FAMILY_QP)
    hipLaunchKernelGGL((jvp_kernel<NMAX, 0, kThetaSplitDot>), dim3((unsigned)batch), dim3(64), 0, st, a);
  else
    hipLaunchKernelGGL((jvp_kernel<NMAX, 1, kThetaSplitDot>), dim3((unsigned)batch), dim3(64), 0, st, a);
  return hipGetLastError();
}
}  // namespace

hipError_t launch_jvp_shared_dot(int nmax, const SensArgs& a, int64_t batch, hipStream_t st) {
  switch (nmax) {
    case 8: return go_jvp_shared_dot<8>(a, batch, st);
    case 16: return go_jvp_shared_dot<16>(a, batch, st);
    case 24: return go_jvp_shared_dot<24>(a, batch, st);
    case 32: return go_jvp_shared_dot<32>(a, batch, st);
    case 48: return go_jvp_shared_dot<48>(a, batch, st);
    case 64: return go_jvp_shared_dot<64>(a, batch, st);
    default: return hipErrorInvalidValue;
  }
}

}  // namespace mcpx

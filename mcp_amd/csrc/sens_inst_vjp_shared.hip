// vjp_kernel instantiations with the SPLIT flag (sens_kernel_impl.hpp) for
// NMAX ∈ {8,16,24,32,48,64} ≥ n + m, QP and affine families: the pullback of a shared-matrix
// batch (mcpx_vjp_batch_shared*) — one matrix block read by every instance, [∂b; ∂ϕ] /
// [∂g; ∂h] written.
#include "sens_kernel_impl.hpp"

namespace mcpx {

namespace {
template <int NMAX>
hipError_t go_vjp_shared(const SensArgs& a, int64_t batch, hipStream_t st) {
  if (a.family == MCPX_FAMILY_QP)
    hipLaunchKernelGGL((vjp_kernel<NMAX, 0, true>), dim3((unsigned)batch), dim3(64), 0, st, a);
  else
    hipLaunchKernelGGL((vjp_kernel<NMAX, 1, true>), dim3((unsigned)batch), dim3(64), 0, st, a);
  return hipGetLastError();
}
}  // namespace

hipError_t launch_vjp_shared(int nmax, const SensArgs& a, int64_t batch, hipStream_t st) {
  switch (nmax) {
    case 8: return go_vjp_shared<8>(a, batch, st);
    case 16: return go_vjp_shared<16>(a, batch, st);
    case 24: return go_vjp_shared<24>(a, batch, st);
    case 32: return go_vjp_shared<32>(a, batch, st);
    case 48: return go_vjp_shared<48>(a, batch, st);
    case 64: return go_vjp_shared<64>(a, batch, st);
    default: return hipErrorInvalidValue;
  }
}

}  // namespace mcpx

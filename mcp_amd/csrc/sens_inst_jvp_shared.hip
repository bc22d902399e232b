// jvp_kernel instantiations with SPLIT = kThetaSplit (sens_kernel_impl.hpp) for
// NMAX ∈ {8,16,24,32,48,64} ≥ n + 2m, QP and affine families: the tangents of a
// shared-matrix batch (mcpx_jvp_batch_shared*) — rows of ∇F_z from the one matrix block,
// right-hand sides from the per-instance block's tangents.
#include "sens_kernel_impl.hpp"

namespace mcpx {

namespace {
template <int NMAX>
hipError_t go_jvp_shared(const SensArgs& a, int64_t batch, hipStream_t st) {
  if (a.family == MCPX_FAMILY_QP)
    hipLaunchKernelGGL((jvp_kernel<NMAX, 0, kThetaSplit>), dim3((unsigned)batch), dim3(64), 0, st, a);
  else
    hipLaunchKernelGGL((jvp_kernel<NMAX, 1, kThetaSplit>), dim3((unsigned)batch), dim3(64), 0, st, a);
  return hipGetLastError();
}
}  // namespace

hipError_t launch_jvp_shared(int nmax, const SensArgs& a, int64_t batch, hipStream_t st) {
  switch (nmax) {
    case 8: return go_jvp_shared<8>(a, batch, st);
    case 16: return go_jvp_shared<16>(a, batch, st);
    case 24: return go_jvp_shared<24>(a, batch, st);
    case 32: return go_jvp_shared<32>(a, batch, st);
    case 48: return go_jvp_shared<48>(a, batch, st);
    case 64: return go_jvp_shared<64>(a, batch, st);
    default: return hipErrorInvalidValue;
  }
}

}  // namespace mcpx

// Workgroup-per-instance JVP kernels of mcpx_jvp_batch_shared_dot*: the kernels of
// sens_inst_wg_shared.hip with SPLIT = kThetaSplitDot (sens_wg_impl.hpp) — one matrix block and
// one [K × shared_dim] block of its tangents for the whole batch, the per-instance block's
// tangents or +0.0.  QP and affine families, buckets 128 … 768.
#include "sens_wg_impl.hpp"

namespace mcpx {

template <int FAMILY, int NV>
__global__ __launch_bounds__(wg::kThreads) void sens_wg_shared_dot_kernel_t(const wg::WgSensArgs args) {
  wg::sens_instances<FAMILY, true, NV, NV, wg::NoGen, wg::kNB, kThetaSplitDot>(args);
}

namespace {
template <int FAMILY>
const void* pick(int nv) {
  switch (nv) {
    case 128: return (const void*)&sens_wg_shared_dot_kernel_t<FAMILY, 128>;
    case 256: return (const void*)&sens_wg_shared_dot_kernel_t<FAMILY, 256>;
    case 512: return (const void*)&sens_wg_shared_dot_kernel_t<FAMILY, 512>;
    case 768: return (const void*)&sens_wg_shared_dot_kernel_t<FAMILY, 768>;
    default: return nullptr;
  }
}
}  // namespace

const void* sens_wg_shared_dot_kernel(int family, int nv) {
  if (family == MCPX_FAMILY_QP) return pick<MCPX_FAMILY_QP>(nv);
  if (family == MCPX_FAMILY_AFFINE) return pick<MCPX_FAMILY_AFFINE>(nv);
  return nullptr;
}

hipError_t launch_sens_wg_shared_dot(int family, int nv, const wg::WgSensArgs& a, int grid, hipStream_t st) {
  const void* k = sens_wg_shared_dot_kernel(family, nv);
  if (!k) return hipErrorInvalidValue;
  void* params[] = {(void*)&a};
  return hipLaunchKernel(k, dim3((unsigned)grid), dim3(wg::kThreads), params, 0, st);
}

}  // namespace mcpx

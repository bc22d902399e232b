// wg_layout.h — the per-slot workspace layout and the grid size of the persistent
// workgroup kernels (ipm_wg_impl.hpp, sens_wg_impl.hpp, the generated modules' _wg
// kernels), written down once for mcpx_api.cpp and the tools that launch these kernels
// themselves.  Host only, pure functions: no HIP call.
#pragma once

#include <stdint.h>
#include <algorithm>

#include "ipm_wg.h"

namespace mcpx {
namespace wg {

// Most instances of one launch: a batch runs in chunks of this many.
constexpr int64_t kChunk = (int64_t)1 << 30;
// The sensitivity kernels' workspace cap (bytes): a long-horizon module's slot is tens of MB
// (T = 30 tangents: 35 MB of [K | rhs] alone), so the persistent grid takes at most 4 GiB of
// workspace, fewer workgroups on the same queue.
constexpr int64_t kSensWorkCap = (int64_t)4 << 30;

// Every part of a slot starts on a 256-B boundary (32 doubles).
inline int64_t align(int64_t doubles) { return (doubles + 31) / 32 * 32; }

// Rows of the system the solve kernels factor.
inline int system_rows(int solver, int n, int m) {
  return solver == MCPX_LINSOLVE_SCHUR ? n : (solver == MCPX_LINSOLVE_REDUCED ? n + m : n + 2 * m);
}

// Slot of a solve kernel: [K | rhs] row-major, a generated module's Jacobian blocks
// (`block` doubles, 0 for the QP / affine families), SCHUR's 4 × m auxiliaries.
inline WgArgs solve_layout(int solver, int n, int m, int64_t block) {
  const int ns = system_rows(solver, n, m);
  WgArgs w{};
  w.ld = ns + 1;
  w.off_blk = align((int64_t)ns * w.ld);
  w.off_aux = align(w.off_blk + block);
  w.off_rd = w.off_aux;  // (R·D⁻¹ no longer kept: the SCHUR entries read R and D⁻¹ directly)
  w.slot_stride = align(w.off_aux + (solver == MCPX_LINSOLVE_SCHUR ? 4 * (int64_t)m : 0));
  return w;
}

constexpr int64_t kNoModule = -1;  // sens_layout's `block` for the QP / affine families

// Slot of a sensitivity kernel: [K | rhs] of the (n+m)-row VJP system or the (n+2m)-row JVP
// system, then for a generated module (`block` ≥ 0 doubles of Jacobian blocks) the blocks
// and ∇F_θ ((n+m) × p), then the JVP's solutions.  mode 1 (the condition estimate): two
// vectors of scratch in the right-hand-side area.
inline WgSensArgs sens_layout(bool jvp, int mode, int n, int m, int64_t p, int n_partials, int64_t block) {
  const int nr = n + m, ns = jvp ? n + 2 * m : nr;
  const bool mod = block != kNoModule;
  WgSensArgs w{};
  w.nrhs = mode == 1 ? 2 : (jvp ? std::max(1, std::min(n_partials, MCPX_JVP_RHS)) : 1);
  w.ld = ns + w.nrhs;
  w.off_blk = align((int64_t)ns * w.ld);
  w.off_dth = align(w.off_blk + (mod ? block : 0));
  w.off_sol = align(w.off_dth + (mod ? (int64_t)nr * p : 0));
  w.slot_stride = align(w.off_sol + (jvp ? (int64_t)w.nrhs * ns : 0));
  return w;
}

// Workgroups of the persistent grid: the resident slots, at most one per instance of a
// chunk, and no more than fit `cap_bytes` of workspace (0: no cap), but at least one.
inline int64_t grid_size(int64_t slots, int64_t batch, int64_t slot_stride, int64_t cap_bytes) {
  int64_t grid = std::min(slots, std::min(kChunk, batch));
  const int64_t cap = cap_bytes / (int64_t)sizeof(double);
  if (cap_bytes && grid * slot_stride > cap) grid = std::max<int64_t>(1, cap / slot_stride);
  return grid;
}

}  // namespace wg
}  // namespace mcpx

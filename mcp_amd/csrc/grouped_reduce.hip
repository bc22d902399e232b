// The reduced gradient of every group's matrix block of a grouped shared-matrix batch
// (mcpx_vjp_batch_grouped_reduce*, include/mcpx.h): per group the sum mcpx_vjp_batch_shared_reduce
// forms for a whole batch, with the same chunking (chunks of MCPX_REDUCE_CHUNK instances counted
// from the group's first instance) and the same two routines (shared_reduce_impl.hpp), so group
// g's bits are those of the shared call on group g alone.
//
//   grouped_reduce_partial  reduce_chunk_tile on row r.chunk0 + blockIdx.x of the chunk table.
//   grouped_reduce_zero     +0.0 / 0 into every group's row and count, ahead of the folds.
//   grouped_reduce_fold     per group of the launch (grid.y, folded past 65,535 groups) fold_chunks
//                           over the part of its chunk range that lies in the launch's portion,
//                           continuing the chain dshared[g] holds (zeroed before the first portion).
#include <algorithm>

#include "shared_reduce_impl.hpp"

namespace mcpx {

namespace {

constexpr int64_t kFoldGroupRows = 65535;  // grid.y

__global__ __launch_bounds__(64 * kReduceWaves) void grouped_reduce_partial(const GroupReduceArgs A) {
  const GroupChunk c = A.chunks[A.r.chunk0 + blockIdx.x];
  reduce_chunk_tile(A.r, c.first - A.inst0, c.len, A.r.part + (int64_t)blockIdx.x * A.r.ds, A.r.count + blockIdx.x);
}

__global__ __launch_bounds__(kFoldThreads) void grouped_reduce_fold(const double* __restrict__ part,
                                                                    const int64_t* __restrict__ count, int64_t c0,
                                                                    int64_t nchunks, const int64_t* __restrict__ cbase,
                                                                    int64_t g_lo, int64_t g_hi, int64_t ds,
                                                                    double* __restrict__ dshared, int64_t dshared_ld,
                                                                    int64_t* __restrict__ used) {
  for (int64_t g = g_lo + blockIdx.y; g < g_hi; g += gridDim.y) {  // g is the same for the whole block
    const int64_t lo = cbase[g] > c0 ? cbase[g] : c0;
    const int64_t hi = cbase[g + 1] < c0 + nchunks ? cbase[g + 1] : c0 + nchunks;
    if (hi <= lo) continue;
    fold_chunks(part + (lo - c0) * ds, count + (lo - c0), hi - lo, ds, 0, dshared + g * dshared_ld, used + g,
                blockIdx.x, blockIdx.x == 0);
    __syncthreads();  // the next group's rounds reuse the stage
  }
}

__global__ __launch_bounds__(256) void grouped_reduce_zero(double* __restrict__ dshared, int64_t dshared_ld,
                                                            int64_t ds, int64_t G, int64_t* __restrict__ used) {
  const int64_t stride = (int64_t)gridDim.x * 256;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < G * ds; i += stride)
    dshared[(i / ds) * dshared_ld + i % ds] = 0.0;
  for (int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x; g < G; g += stride) used[g] = 0;
}

}  // namespace

hipError_t launch_grouped_reduce_zero(double* dshared, int64_t dshared_ld, int64_t ds, int64_t G, int64_t* used,
                                      hipStream_t st) {
  if (G <= 0) return hipSuccess;
  const int64_t blocks = std::min<int64_t>(4096, (G * std::max<int64_t>(ds, 1) + 255) / 256);
  hipLaunchKernelGGL(grouped_reduce_zero, dim3((unsigned)blocks), dim3(256), 0, st, dshared, dshared_ld, ds, G, used);
  return hipGetLastError();
}

hipError_t launch_grouped_reduce_partial(const GroupReduceArgs& a, int64_t nchunks, hipStream_t st) {
  if (nchunks <= 0) return hipSuccess;
  if (nchunks > 0x7fffffff || a.r.n < 0 || a.r.m < 0 || !a.chunks) return hipErrorInvalidValue;
  const int64_t tn = (a.r.n + 15) >> 4, tm = (a.r.m + 15) >> 4;
  const int64_t tiles = a.r.family == MCPX_FAMILY_QP ? tn * tn + tm * tn : (tn + tm) * (tn + tm);
  const int64_t gy = std::max<int64_t>(1, (tiles + kReduceWaves - 1) / kReduceWaves);
  if (gy > 65535) return hipErrorInvalidValue;
  hipLaunchKernelGGL(grouped_reduce_partial, dim3((unsigned)nchunks, (unsigned)gy), dim3(64 * kReduceWaves), 0, st, a);
  return hipGetLastError();
}

hipError_t launch_grouped_reduce_fold(const double* part, const int64_t* count, int64_t c0, int64_t nchunks,
                                      const int64_t* cbase, int64_t g_lo, int64_t g_hi, int64_t ds, double* dshared,
                                      int64_t dshared_ld, int64_t* used, hipStream_t st) {
  if (nchunks <= 0 || g_hi <= g_lo) return hipSuccess;
  const int64_t gx = std::max<int64_t>(1, (ds + kFoldEntries - 1) / kFoldEntries);
  if (gx > 0x7fffffff) return hipErrorInvalidValue;
  const int64_t gy = std::min(g_hi - g_lo, kFoldGroupRows);
  hipLaunchKernelGGL(grouped_reduce_fold, dim3((unsigned)gx, (unsigned)gy), dim3(kFoldThreads), 0, st, part, count, c0,
                     nchunks, cbase, g_lo, g_hi, ds, dshared, dshared_ld, used);
  return hipGetLastError();
}

}  // namespace mcpx

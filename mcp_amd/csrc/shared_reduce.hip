// The reduced gradient of the matrix block of a shared-matrix batch
// (mcpx_vjp_batch_shared_reduce*, include/mcpx.h): Σ_b of the rank-1 matrix blocks of the full
// pullback record, formed from x, y and the split pullback's dvar (λ) without ever storing a
// per-instance record.
//
//   shared_reduce_partial  reduce_chunk_tile (shared_reduce_impl.hpp) on chunk chunk0 + blockIdx.x of
//                          MCPX_REDUCE_CHUNK instances counted from instance 0.
//   shared_reduce_fold     fold_chunks over the launch's chunks.
#include <algorithm>

#include "shared_reduce_impl.hpp"

namespace mcpx {

namespace {

__global__ __launch_bounds__(64 * kReduceWaves) void shared_reduce_partial(const ReduceArgs A) {
  const int64_t b0 = (A.chunk0 + blockIdx.x) * MCPX_REDUCE_CHUNK;  // the chunk's first instance
  const int len = (int)(A.batch - b0 < MCPX_REDUCE_CHUNK ? A.batch - b0 : MCPX_REDUCE_CHUNK);
  reduce_chunk_tile(A, b0, len, A.part + (int64_t)blockIdx.x * A.ds, A.count + blockIdx.x);
}

__global__ __launch_bounds__(kFoldThreads) void shared_reduce_fold(const double* __restrict__ part,
                                                                   const int64_t* __restrict__ count, int64_t nchunks,
                                                                   int64_t ds, int first, double* __restrict__ dshared,
                                                                   int64_t* __restrict__ used) {
  fold_chunks(part, count, nchunks, ds, first, dshared, used, blockIdx.x, blockIdx.x == 0);
}

}  // namespace

hipError_t launch_shared_reduce_partial(const ReduceArgs& a, int64_t nchunks, hipStream_t st) {
  if (nchunks <= 0) return hipSuccess;
  if (nchunks > 0x7fffffff || a.n < 0 || a.m < 0 ||
      (a.chunk0 + nchunks - 1) * MCPX_REDUCE_CHUNK >= a.batch)  // every chunk holds an instance
    return hipErrorInvalidValue;
  const int64_t tn = (a.n + 15) >> 4, tm = (a.m + 15) >> 4;
  const int64_t tiles = a.family == MCPX_FAMILY_QP ? tn * tn + tm * tn : (tn + tm) * (tn + tm);
  const int64_t gy = std::max<int64_t>(1, (tiles + kReduceWaves - 1) / kReduceWaves);
  if (gy > 65535) return hipErrorInvalidValue;
  hipLaunchKernelGGL(shared_reduce_partial, dim3((unsigned)nchunks, (unsigned)gy), dim3(64 * kReduceWaves), 0, st, a);
  return hipGetLastError();
}

hipError_t launch_shared_reduce_fold(const double* part, const int64_t* count, int64_t nchunks, int64_t ds,
                                     bool first, double* dshared, int64_t* used, hipStream_t st) {
  const int64_t gx = std::max<int64_t>(1, (ds + kFoldEntries - 1) / kFoldEntries);
  if (gx > 0x7fffffff) return hipErrorInvalidValue;
  hipLaunchKernelGGL(shared_reduce_fold, dim3((unsigned)gx), dim3(kFoldThreads), 0, st, part, count, nchunks, ds,
                     first ? 1 : 0, dshared, used);
  return hipGetLastError();
}

}  // namespace mcpx

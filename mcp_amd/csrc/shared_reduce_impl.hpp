// shared_reduce_impl.hpp — the two device routines behind the reduced gradient of a shared matrix
// block, used by shared_reduce.hip (one block for the batch) and grouped_reduce.hip (one block per
// group of instances):
//
//   reduce_chunk_tile  one wave per (chunk of at most MCPX_REDUCE_CHUNK instances, 16×16 tile of
//                      the shared block): the chunk's ordered fma chain of every entry of the tile
//                      on v_mfma_f64_16x16x4_f64, K = instance.  The instruction equals a
//                      k-ascending chain of fma, so the tile holds the
//                      contract's bits whatever the grid.  Operands come straight from global
//                      memory (16 consecutive doubles of 4 — or 2 — instances per load; the tiles
//                      of a chunk share a workgroup, so they hit in L2).
//   fold_chunks        one thread per entry: the chunk partials added in ascending order.
//
// The output column index of a tile runs over the A-fragment (MFMA row i) and the output row
// over the B-fragment (MFMA column j = lane & 15): the block is column-major, so the 16 lanes
// of a DPP row then store 16 consecutive doubles.  a·b commutes bit for bit, so which operand
// sits in which fragment does not touch the result.
#pragma once

#include "sens_kernel.h"

namespace mcpx {

namespace {

typedef double d4 __attribute__((ext_vector_type(4)));

constexpr int kReduceWaves = 4;  // tiles (waves) per workgroup
constexpr int kReduceDepth = 8;  // MFMAs whose operand loads are in flight together
constexpr int kFoldThreads = 256;
constexpr int kFoldEntries = 16;  // consecutive entries per fold block: one 128-byte line per chunk
constexpr int kFoldDepth = 8;     // loads in flight per fold thread
constexpr int kFoldRound = kFoldThreads / kFoldEntries * kFoldDepth;  // chunks staged per round

// Instance b enters the sum: not skipped by the caller and its pullback succeeded.
__device__ __forceinline__ bool included(const ReduceArgs& A, int64_t b) {
  return A.status[b] == 0 && (!A.skip || A.skip[b] == 0);
}

// The chunk of `len` instances from b0 on (indices into A's arrays): tile blockIdx.y·kReduceWaves +
// wave of its partial into P [A.ds], and (tile 0's wave) its number of included instances into *count.
__device__ __forceinline__ void reduce_chunk_tile(const ReduceArgs& A, const int64_t b0, const int len,
                                                  double* const P0, int64_t* const count) {
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int n = A.n, m = A.m, vd = n + m;
  const int tn = (n + 15) >> 4, tm = (m + 15) >> 4;
  const bool qp = A.family == MCPX_FAMILY_QP;
  const int tiles = qp ? tn * tn + tm * tn : (tn + tm) * (tn + tm);
  const int t = (int)blockIdx.y * kReduceWaves + wave;

  if (blockIdx.y == 0 && wave == 0) {  // the chunk's number of included instances
    int cnt = 0;
    for (int q0 = 0; q0 < len; q0 += 64) {
      const bool inc = q0 + lane < len && included(A, b0 + q0 + lane);
      cnt += __popcll(__ballot(inc));
    }
    if (lane == 0) *count = cnt;
  }
  if (t >= tiles) return;

  // The tile: rows [16 I, 16 I + 16) of a block with R rows, columns [16 J, …) of its C, the
  // block at `base` of the shared layout (column-major, leading dimension R).  Row operand:
  // element e of instance b at rp[b·vd + e] (a slice of dvar); column operand at cp[b·cld + e].
  const int64_t nn = (int64_t)n * n, nm = (int64_t)n * m;
  const double* rp;
  const double* cp;
  int64_t cld, base;
  int I, J, R, C;
  bool neg = false, pair = false;
  if (qp) {
    cp = A.x;
    cld = n;
    C = n;
    if (t < tn * tn) {  // ∂M_ij: fma(−λx_i, x_j, acc)
      I = t % tn;
      J = t / tn;
      rp = A.dvar + m;
      R = n;
      base = 0;
      neg = true;
    } else {  // ∂A_kj: fma(−λy_k, x_j, acc), then fma(λx_j, y_k, acc)
      const int u = t - tn * tn;
      I = u % tm;
      J = u / tm;
      rp = A.dvar;
      R = m;
      base = nn;
      pair = true;
    }
  } else {  // the four blocks of [∂g; ∂h][x; y]ᵀ
    const int tt = tn + tm;
    I = t % tt;
    J = t / tt;
    const bool grow = I < tn, xcol = J < tn;
    if (!grow) I -= tn;
    if (!xcol) J -= tn;
    rp = grow ? A.dvar : A.dvar + n;
    R = grow ? n : m;
    cp = xcol ? A.x : A.y;
    cld = xcol ? n : m;
    C = xcol ? n : m;
    base = grow ? (xcol ? 0 : nn) : (xcol ? nn + nm : nn + 2 * nm);
  }

  const int li = lane & 15, k = lane >> 4;
  const int row = 16 * I + li, col = 16 * J + li;  // this lane's operand elements
  const bool rin = row < R, cin = col < C;
  d4 acc = {0.0, 0.0, 0.0, 0.0};
  // This lane's K slot of an MFMA: instance offset `kq` of `per` instances per MFMA, and where
  // its two operands live.  Outer-product tiles: four instances per MFMA.  ∂A tiles: two, the
  // K-pair [x_j, λx_j] (columns) · [−λy_k, y_k] (rows) per instance.
  const bool second = pair && (k & 1);
  const int per = pair ? 2 : 4, kq = pair ? k >> 1 : k;
  if (pair) {
    cp = second ? A.dvar + m : A.x;  // λx_j : x_j
    cld = second ? vd : n;
    rp = second ? A.y : A.dvar;  // y_k : λy_k
    neg = !second;
  }
  const int64_t rld = pair && second ? m : vd;
  // kReduceDepth MFMAs' operands are loaded before the first of them issues; steps wholly past
  // the chunk's end run on +0.0 operands, which leave the accumulator as it is
  for (int c = 0; c < len; c += per * kReduceDepth) {
    double rv[kReduceDepth], cv[kReduceDepth];
    bool on[kReduceDepth];
#pragma unroll
    for (int u = 0; u < kReduceDepth; ++u) {
      const int q = c + per * u + kq;
      const bool live = q < len;
      const int64_t b = b0 + (live ? q : 0);
      on[u] = live && included(A, b);
      rv[u] = live && rin ? rp[b * rld + row] : 0.0;
      cv[u] = live && cin ? cp[b * cld + col] : 0.0;
    }
#pragma unroll
    for (int u = 0; u < kReduceDepth; ++u)  // excluded instance, K tail, rows / columns beyond the block: +0.0
      acc = __builtin_amdgcn_mfma_f64_16x16x4f64(on[u] && cin ? cv[u] : 0.0,
                                                 on[u] && rin ? (neg ? -rv[u] : rv[u]) : 0.0, acc, 0, 0, 0);
  }
  double* P = P0 + base;
#pragma unroll
  for (int r = 0; r < 4; ++r) {  // C/D layout: MFMA row (lane >> 4) + 4r = output column, lane & 15 = output row
    const int oc = 16 * J + k + 4 * r;
    if (rin && oc < C) P[row + (int64_t)R * oc] = acc[r];
  }
}

// dshared[e] ← (first ? +0.0 : dshared[e]) + P_0[e] + P_1[e] + …, chunks ascending, for the
// kFoldEntries entries from eblock·kFoldEntries on; `used` likewise over the chunk counts
// (integers: any order; the block with do_used set).  Called by every thread of a block of
// kFoldThreads.  The additions of an entry are one thread's serial chain, as the contract orders
// them; what the other threads of the block do is keep that thread fed: per round the 256
// threads bring kFoldRound chunks' values of the block's entries through LDS (kFoldDepth loads in
// flight per thread), so the chain waits for one memory latency per kFoldRound chunks, not one
// per few.
__device__ __forceinline__ void fold_chunks(const double* __restrict__ part, const int64_t* __restrict__ count,
                                            int64_t nchunks, int64_t ds, int first, double* __restrict__ dshared,
                                            int64_t* __restrict__ used, int64_t eblock, bool do_used) {
  __shared__ double stage[kFoldRound][kFoldEntries];
  __shared__ unsigned long long total;
  const int le = threadIdx.x % kFoldEntries, slot = threadIdx.x / kFoldEntries;
  const int64_t e = eblock * kFoldEntries + le;
  const bool ein = e < ds;
  double acc = 0.0;
  if (slot == 0 && ein && !first) acc = dshared[e];
  for (int64_t c0 = 0; c0 < nchunks; c0 += kFoldRound) {
    double v[kFoldDepth];
#pragma unroll
    for (int u = 0; u < kFoldDepth; ++u) {
      const int64_t c = c0 + slot * kFoldDepth + u;
      v[u] = ein && c < nchunks ? part[c * ds + e] : 0.0;
    }
    __syncthreads();  // the previous round's chain has read its stage
#pragma unroll
    for (int u = 0; u < kFoldDepth; ++u) stage[slot * kFoldDepth + u][le] = v[u];
    __syncthreads();
    if (slot == 0) {
      const int lim = (int)(nchunks - c0 < kFoldRound ? nchunks - c0 : kFoldRound);  // no step past the last chunk
      for (int k = 0; k < lim; ++k) acc = acc + stage[k][le];
    }
  }
  if (slot == 0 && ein) dshared[e] = acc;
  if (do_used) {
    if (threadIdx.x == 0) total = 0;
    __syncthreads();
    unsigned long long mine = 0;
    for (int64_t c = threadIdx.x; c < nchunks; c += kFoldThreads) mine += (unsigned long long)count[c];
    if (mine) atomicAdd(&total, mine);
    __syncthreads();
    if (threadIdx.x == 0) *used = (first ? 0 : *used) + (int64_t)total;
  }
}

}  // namespace

}  // namespace mcpx

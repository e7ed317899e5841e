// The fixed reduction tree of the diagnostics contract (include/sphmi.h, reduce(a)): terms padded with +0.0 to whole chunks of
// 1024; in a chunk, a[i] += a[i + stride] for stride = 512 ... 1; the chunks' results are the terms of the next level. What the
// kernels that reduce in that shape share (sph_diag.hip, sph_elastic_measure.hip); one 256-thread block owns one chunk.
#pragma once
#include "sph_common.h"

#define DIAG_CHUNK 1024

__device__ __forceinline__ double diag_wave_sum(double x) {  // strides 32 ... 1 of the tree; lane 0 holds the result
#pragma unroll
  for (int s = 32; s >= 1; s >>= 1) x = x + __shfl_down(x, s, 64);
  return x;
}

enum { DIAG_OP_SUM = 0, DIAG_OP_MIN = 1, DIAG_OP_MAX = 2 };

template <int OP>
__device__ __forceinline__ double diag_combine(double a, double b) {
  if (OP == DIAG_OP_SUM) return a + b;
  if (OP == DIAG_OP_MIN) return b < a ? b : a;
  return b > a ? b : a;
}

// chunk `chunk` of the nIn partials at `in` (padded with `pad`), by a whole block; sh: SPH_BLOCK doubles of LDS
template <int OP>
__device__ double diag_block_reduce(const double* __restrict__ in, int nIn, int chunk, double pad, double* sh) {
  const int t = threadIdx.x;
  double e[4];
#pragma unroll
  for (int k = 0; k < 4; k++) {
    const int i = chunk * DIAG_CHUNK + k * SPH_BLOCK + t;
    e[k] = i < nIn ? in[i] : pad;
  }
  sh[t] = diag_combine<OP>(diag_combine<OP>(e[0], e[2]), diag_combine<OP>(e[1], e[3]));
  __syncthreads();
  for (int s = 128; s >= 1; s >>= 1) {
    if (t < s) sh[t] = diag_combine<OP>(sh[t], sh[t + s]);
    __syncthreads();
  }
  const double x = sh[0];
  __syncthreads();
  return x;
}

// The leaf of the diagnostics tree (sph_diag.hip), for every kernel that produces diagnostics records: one
// 256-thread block owns one chunk of 1024 sorted particles, thread t holds elements t, t+256, t+512, t+768 in registers
// (diag_leaf_load), and diag_leaf_reduce reduces the chunk for ONE selection of those elements. Who is selected is the caller's
// business: a region or a component label (k_diag_leaf), a lattice bin (k_bin_leaf, sph_bins.hip).
#pragma once
#include "sph_common.h"
#include "sph_tree.h"

#define DIAG_SUMS 14   // record words 0..13
#define DIAG_TERMS 13  // x y z, vx vy vz, Lx Ly Lz, v2, rho, e2, p: record words 1..13

// the 10 plain extremes of a record, in this order: words 16, 18, 23, 24, 25 (minima), then 17, 19, 26, 27, 28 (maxima)
__device__ static const int kDiagMinWord[5] = {16, 18, 23, 24, 25};
__device__ static const int kDiagMaxWord[5] = {17, 19, 26, 27, 28};

struct DiagLeafLds {
  double sh[DIAG_SUMS][SPH_BLOCK];
  float shx[4][10];
  float shv[4];
  int shi[4];
};

// the 13 terms of sorted particle j (position record p), every operation a rounded float one
__device__ __forceinline__ void diag_leaf_load(const SphDev& d, float rho0, int j, const float4& p, float (&f)[DIAG_TERMS]) {
  const float4 v = d.sortedVel[j];
  const float rho = d.rho[j];
  const float pr = d.rp[j].y;
  f[0] = p.x; f[1] = p.y; f[2] = p.z;
  f[3] = v.x; f[4] = v.y; f[5] = v.z;
  f[6] = p.y * v.z - p.z * v.y;
  f[7] = p.z * v.x - p.x * v.z;
  f[8] = p.x * v.y - p.y * v.x;
  f[9] = v.x * v.x + v.y * v.y + v.z * v.z;
  f[10] = rho;
  const float er = rho - rho0;
  f[11] = er * er;
  f[12] = pr;
}

// The partials of chunk `chunk` for the selection sel[e] of this thread's four elements (f[e]: zeros where there is no
// particle), by the whole block: strides 512 and 256 in registers, tree_group_sums below, the extremes and the pair (max v2,
// lowest index) through the shuffle loop. store(word, x) receives the 14 sums, the 10 extremes (kDiagMinWord, kDiagMaxWord)
// and words 20, 21, each from one thread. Ends with a barrier: L may be written again at once.
template <class Store>
__device__ __forceinline__ void diag_leaf_reduce(DiagLeafLds& L, const float (&f)[4][DIAG_TERMS], const bool (&sel)[4], int chunk,
                                                 Store store) {
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  // sums: strides 512 and 256 in registers, one word at a time (the 14 doubles are never live together)
#pragma unroll
  for (int w = 0; w < DIAG_SUMS; w++) {
    double q[4];
#pragma unroll
    for (int e = 0; e < 4; e++) {
      float x = w == 0 ? 1.0f : f[e][w == 0 ? 0 : w - 1];
      asm volatile("" : "+v"(x));  // widen here, per selection: hoisted out of the caller's loop, the 52 doubles cost 104 VGPRs
      q[e] = sel[e] ? (double)x : 0.0;
    }
    L.sh[w][t] = (q[0] + q[2]) + (q[1] + q[3]);
  }
  // extremes of this thread's four elements, then of its wave
  float mn[5], mx[5], bestV = -INFINITY;
  int bestI = 0x7fffffff;
#pragma unroll
  for (int k = 0; k < 5; k++) { mn[k] = INFINITY; mx[k] = -INFINITY; }
#pragma unroll
  for (int e = 0; e < 4; e++) {
    if (!sel[e]) continue;
    const float q[5] = {f[e][10], f[e][12], f[e][0], f[e][1], f[e][2]};
#pragma unroll
    for (int k = 0; k < 5; k++) { mn[k] = q[k] < mn[k] ? q[k] : mn[k]; mx[k] = q[k] > mx[k] ? q[k] : mx[k]; }
    if (f[e][9] > bestV) { bestV = f[e][9]; bestI = chunk * DIAG_CHUNK + e * SPH_BLOCK + t; }  // ascending index: the first wins
  }
#pragma unroll
  for (int s = 32; s >= 1; s >>= 1) {
#pragma unroll
    for (int k = 0; k < 5; k++) {
      const float om = __shfl_down(mn[k], s, 64), ox = __shfl_down(mx[k], s, 64);
      mn[k] = om < mn[k] ? om : mn[k];
      mx[k] = ox > mx[k] ? ox : mx[k];
    }
    const float ov = __shfl_down(bestV, s, 64);
    const int oi = __shfl_down(bestI, s, 64);
    if (ov > bestV || (ov == bestV && oi < bestI)) { bestV = ov; bestI = oi; }
  }
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < 5; k++) { L.shx[wave][k] = mn[k]; L.shx[wave][5 + k] = mx[k]; }
    L.shv[wave] = bestV; L.shi[wave] = bestI;
  }
  __syncthreads();
  // strides 128, 64 and the in-wave strides: the 14 words are shared out among the four waves
  tree_group_sums<DIAG_SUMS>(L.sh, DIAG_SUMS, store);
  if (t < 10) {
    float x = L.shx[0][t];
    for (int q = 1; q < 4; q++) { const float o = L.shx[q][t]; x = t < 5 ? (o < x ? o : x) : (o > x ? o : x); }
    store(t < 5 ? kDiagMinWord[t] : kDiagMaxWord[t - 5], (double)x);
  } else if (t == 10) {
    float bv = L.shv[0]; int bi = L.shi[0];
    for (int q = 1; q < 4; q++) if (L.shv[q] > bv || (L.shv[q] == bv && L.shi[q] < bi)) { bv = L.shv[q]; bi = L.shi[q]; }
    store(20, (double)bv);
    store(21, (double)bi);
  }
  __syncthreads();  // L is reused by the next selection
}

// Word w of a record from the top of its tree: canonical extremes (+ 0.0f), the empty-selection rule, the original id of the
// fastest particle. top(word): the tree's result for that word (read only for the words the rule needs).
template <class Top>
__device__ __forceinline__ double diag_record_word(const SphDev& d, int w, Top top) {
  const double n = top(0);
  double x = 0.0;
  if (w < DIAG_SUMS) x = top(w);
  else if (w == 21 || w == 22) {
    x = -1.0;
    if (n > 0.0) {
      const int idx = (int)top(21);
      if (idx < d.N) x = w == 21 ? (double)idx : (double)d.vals[idx];  // (no index when every selected v2 is NaN)
    }
  } else if ((w >= 16 && w <= 20) || (w >= 23 && w <= 28)) {
    if (n > 0.0) x = (double)((float)top(w) + 0.0f);
  }
  return x;
}

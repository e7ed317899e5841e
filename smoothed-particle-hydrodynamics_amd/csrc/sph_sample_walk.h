// Shared by the sampling kernels (sph_sample.hip) and the gradient kernels (sph_gradient.hip): the launch arguments, the
// cell walk of one query point (axis ranges, masked keys, runs of the cell table), the sampling record and the wave-wide
// reductions of the brick walk. See sph_sample.hip for the contract these serve.
#pragma once
#include "sph_common.h"

#define SPH_SAMPLE_WAVE 64
#define SPH_SAMPLE_BOX_MAX 64  // cells a brick box may hold for the wave-uniform walk (3x3x3 = 27 while spacing <= 2h/3)

struct SampleArgs {
  uint32_t typeMask;  // bits 1..3
  float hh;           // h*h, rounded to float once: the selection test r2 < hh
  float ss2;          // simScale*simScale
  float mwp;          // (float)massWpoly6
  // grid: point (i, j, k) = origin + (float)i * spacing per axis; k counts from kBase (the chunk's first z plane)
  float ox, oy, oz, sx, sy, sz;
  int nx, ny, nz, kBase;
};

// Cell range of one axis that holds every particle a query coordinate c can select. The hash truncates x * cellSizeInv and
// is monotone, so [(int)((c-h)*inv), (int)((c+h)*inv)] holds them up to rounding; the range is widened by a margin far
// above the rounding of those two products and of the float distance test (visiting an extra cell costs time, never
// correctness: its particles fail the distance test). The margin grows with |u| so that it stays above one ulp of u.
__device__ __forceinline__ void sample_axis_range(float c, const SphDev& d, int& lo, int& hi) {
  float ul = (c - d.h) * d.cellSizeInv, uh = (c + d.h) * d.cellSizeInv;
  ul -= fminf(fabsf(ul) * 0x1p-21f + 0x1p-10f, 0.5f);
  uh += fminf(fabsf(uh) * 0x1p-21f + 0x1p-10f, 0.5f);
  ul = fminf(fmaxf(ul, -0x1p30f), 0x1p30f);  // (a float -> int conversion out of range is undefined)
  uh = fminf(fmaxf(uh, -0x1p30f), 0x1p30f);
  lo = (int)ul; hi = (int)uh;
  if (hi - lo > 3) hi = lo + 3;  // only for |u| beyond ~2^20 cells, where float coordinates no longer resolve h
}

// masked key of cell (cx, cy, cz) exactly as k_hash computes it (the int products wrap like these unsigned ones)
__device__ __forceinline__ uint32_t sample_key(const SphDev& d, int cx, int cy, int cz) {
  return ((uint32_t)cx + (uint32_t)cy * (uint32_t)d.gx + (uint32_t)cz * (uint32_t)d.gx * (uint32_t)d.gy) & d.cellMask;
}

// Sorted-index run [start, end) of key k < G. cellStart[G] is N, so the run of key G-1 would also hold particles whose keys are
// >= G (outside the declared grid, not in the cell table): it ends at the first of those instead.
__device__ __forceinline__ void sample_run(const SphDev& d, uint32_t k, uint32_t& start, uint32_t& end) {
  start = d.cellStart[k];
  end = d.cellStart[k + 1];
  if (k + 1 == (uint32_t)d.G) {
    uint32_t lo = start, hi = end;
    while (lo < hi) {
      const uint32_t mid = (lo + hi) >> 1;
      if (d.keys[mid] < (uint32_t)d.G) lo = mid + 1; else hi = mid;
    }
    end = lo;
  }
}

struct SampleAcc {
  float W, S, Ux, Uy, Uz, P;
  int n;
};

__device__ __forceinline__ bool sample_type_ok(const SampleArgs& a, float w) {
  const int t = (int)w;
  return t >= 1 && t <= 3 && ((1u << t) & a.typeMask);
}

__device__ __forceinline__ void sample_store(const SampleArgs& a, const SampleAcc& acc, float* out) {
  float4 r0 = make_float4(a.mwp * acc.W, a.mwp * acc.S, 0.f, 0.f), r1 = make_float4(0.f, 0.f, (float)acc.n, 0.f);
  if (acc.S != 0.f) { r0.z = acc.Ux / acc.S; r0.w = acc.Uy / acc.S; r1.x = acc.Uz / acc.S; r1.y = acc.P / acc.S; }
  reinterpret_cast<float4*>(out)[0] = r0;
  reinterpret_cast<float4*>(out)[1] = r1;
}

__device__ __forceinline__ bool sample_finite(float x, float y, float z) {
  return fabsf(x) <= 3.402823466e38f && fabsf(y) <= 3.402823466e38f && fabsf(z) <= 3.402823466e38f;
}

// Consecutive bricks share most of their cells: keep runs of them on one XCD (one L2) — the remap of sph_pcisph.hip's xcd_block.
__device__ __forceinline__ int sample_xcd_block(int nblocks) {
  const int b = blockIdx.x;
  const int per = nblocks >> 3;
  const int even = per << 3;
  if (b >= even) return b;
  return (b & 7) * per + (b >> 3);
}

__device__ __forceinline__ int wave_min_i(int v) {
  for (int o = 32; o >= 1; o >>= 1) v = min(v, __shfl_xor(v, o, SPH_SAMPLE_WAVE));
  return v;
}
__device__ __forceinline__ int wave_max_i(int v) {
  for (int o = 32; o >= 1; o >>= 1) v = max(v, __shfl_xor(v, o, SPH_SAMPLE_WAVE));
  return v;
}
__device__ __forceinline__ uint32_t wave_min_u(uint32_t v) {
  for (int o = 32; o >= 1; o >>= 1) v = min(v, (uint32_t)__shfl_xor((int)v, o, SPH_SAMPLE_WAVE));
  return v;
}


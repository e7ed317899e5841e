// The first stage of the search bands (sph_bands.hip): one flag byte per sorted particle and, per wave of 64 sorted
// particles and band, the ballot and its count. The gather kernel of the fused step (sph_sort.hip) computes them from the record
// and the key it holds in registers when it stores them; sphk_build_bands scans and scatters what it left. One producer.
#pragma once
#include "sph_common.h"

// Bit s of the result: the particle is in band s. A particle whose key is not the id of the in-grid cell its coordinates
// truncate to (negative or non-finite coordinates, a cell outside the grid, ids that the mask aliases) is in every band.
__device__ __forceinline__ uint32_t band_flags(const SphBandGeom& g, const float4 q, const uint32_t key) {
  if (!(q.x >= 0.f && q.y >= 0.f && q.z >= 0.f && q.x < 1.0e9f && q.y < 1.0e9f && q.z < 1.0e9f) || g.aliased) return 0xffu;
  const int cx = (int)(q.x * g.cellSizeInv), cy = (int)(q.y * g.cellSizeInv), cz = (int)(q.z * g.cellSizeInv);  // as k_hash
  if (cx >= g.gx || cy >= g.gy || cz >= g.gz || key != (uint32_t)(cx + cy * g.gx + cz * g.gx * g.gy)) return 0xffu;
  const bool loY = q.y - (float)cy * g.cellSize <= g.Rb, hiY = (float)(cy + 1) * g.cellSize - q.y <= g.Rb;
  const bool loZ = q.z - (float)cz * g.cellSize <= g.Rb, hiZ = (float)(cz + 1) * g.cellSize - q.z <= g.Rb;
  return (hiY && hiZ ? 1u : 0u) | (hiZ ? 2u : 0u) | (loY && hiZ ? 4u : 0u) | (hiY ? 8u : 0u) | (loY ? 16u : 0u) |
         (hiY && loZ ? 32u : 0u) | (loZ ? 64u : 0u) | (loY && loZ ? 128u : 0u);
}

// Sorted particle i of a launch of SPH_BLOCK threads per block, one lane per particle: f = band_flags of (sortedPos[i], keys[i]),
// 0 in the lanes past N. EVERY lane of the wave calls this (the ballots are wave-level): no early return in front of it.
__device__ __forceinline__ void band_flags_store(const SphBandGeom& g, const SphBands& b, int i, uint32_t f) {
  const int lane = threadIdx.x & 63;
  if (i < g.N) b.flags[i] = (uint8_t)f;
  unsigned long long mine = 0ull;
#pragma unroll
  for (int s = 0; s < 8; s++) {
    const unsigned long long m = __ballot((f >> s) & 1u);
    if (lane == s) mine = m;
  }
  const int w = i >> 6;  // (whole waves: the block starts at a multiple of 64)
  if (lane < 8 && w < g.waves) {  // one 64-byte and one 32-byte store per wave
    b.mask[(size_t)w * 8 + lane] = mine;
    b.waveOff[(size_t)w * 8 + lane] = (uint32_t)__popcll(mine);
  }
}

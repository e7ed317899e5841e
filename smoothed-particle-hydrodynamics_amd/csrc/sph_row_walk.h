// The slot loop over one sorted particle's neighbour row, shared by the analysis kernels that read the rows after a step
// (sph_select.hip, sph_components.hip; through sph_selector.h the neighbour count of sph_diag.hip and sph_render.hip).
#pragma once
#include "sph_common.h"

// fn(j) for the 32 slots of sorted particle i's row IN SLOT ORDER (0 .. 31): j is what sph_read_neighbor_rows returns for the
// slot, -1 for an empty one. A wave reads 4 slots of its 64 particles as one contiguous transaction (layout: sph_common.h);
// the rows are streamed once, so the loads are non-temporal. The 32-bit row is read only where the 16-bit one could not be
// written (entry 0 == SPH_N16_WIDE).
template <typename F>
__device__ __forceinline__ void sph_row_for_each_slot(const SphDev& d, int i, F fn) {
  const size_t base = ((size_t)(i >> 6) * 8) * 64 + (size_t)(i & 63);
  typedef unsigned int nt2 __attribute__((ext_vector_type(2)));
  typedef int nt4 __attribute__((ext_vector_type(4)));
  const nt2* v16 = reinterpret_cast<const nt2*>(d.nbr16) + base;
  const nt4* v32 = reinterpret_cast<const nt4*>(d.nbrId) + base;
  const nt2 first = __builtin_nontemporal_load(v16);
  const bool wide = (first.x & 0xffffu) == SPH_N16_WIDE;
  const int zBase = wide ? 0 : d.nbrBase[i];
#pragma unroll 2
  for (int g = 0; g < 8; g++) {
    int nb[4];
    if (wide) {
      const nt4 q = __builtin_nontemporal_load(v32 + (size_t)g * 64);
      nb[0] = q.x; nb[1] = q.y; nb[2] = q.z; nb[3] = q.w;
    } else {
      const nt2 q = g == 0 ? first : __builtin_nontemporal_load(v16 + (size_t)g * 64);
      const uint32_t e[4] = {q.x & 0xffffu, q.x >> 16, q.y & 0xffffu, q.y >> 16};
#pragma unroll
      for (int k = 0; k < 4; k++) nb[k] = e[k] == SPH_N16_EMPTY ? -1 : ((e[k] & 0x8000u) ? zBase : i) + (int)(e[k] & 0x7fffu) - SPH_N16_BIAS;
    }
#pragma unroll
    for (int k = 0; k < 4; k++) fn(nb[k]);
  }
}

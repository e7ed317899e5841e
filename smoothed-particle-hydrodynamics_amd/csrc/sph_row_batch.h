// One sorted particle's neighbour row read in groups of four slots, for the kernels that hold a batch of a row in registers and
// gather a record per neighbour (sph_forces.hip, sph_fields.hip). The slot loop of sph_row_walk.h visits one neighbour at a time;
// these kernels want the ids and the stored distances of several slots side by side, so that all gathers of a batch are in
// flight together.
#pragma once
#include "sph_common.h"

// the row of particle `id` in the tiled maps (sph_common.h): group g = slots 4g .. 4g+3
struct FmRow {
  const int32_t* ids;
  const float4* dist;
  const uint2* v16;
  int self, zOff;
  __device__ __forceinline__ FmRow(const SphDev& d, int id) {
    const size_t base = ((size_t)(id >> 6) * 8) * 64 + (size_t)(id & 63);
    ids = reinterpret_cast<const int32_t*>(reinterpret_cast<const int4*>(d.nbrId) + base);
    dist = reinterpret_cast<const float4*>(d.nbrDist) + base;
    v16 = reinterpret_cast<const uint2*>(d.nbr16) + base;
    self = id;
    zOff = d.nbrBase[id] - id;
  }
  // the rows are streamed once: non-temporal, as the step's kernels read them
  __device__ __forceinline__ float4 dist4(int g) const {
    typedef float nt4 __attribute__((ext_vector_type(4)));
    const nt4 q = __builtin_nontemporal_load(reinterpret_cast<const nt4*>(&dist[(size_t)g * 64]));
    return make_float4(q.x, q.y, q.z, q.w);
  }
  __device__ __forceinline__ uint2 vec16(int g) const {
    typedef unsigned int nt2 __attribute__((ext_vector_type(2)));
    const nt2 q = __builtin_nontemporal_load(reinterpret_cast<const nt2*>(&v16[(size_t)g * 64]));
    return make_uint2(q.x, q.y);
  }
  __device__ __forceinline__ int id_wide(int slot) const { return ids[((size_t)(slot >> 2) * 64) * 4 + (size_t)(slot & 3)]; }
  __device__ __forceinline__ int decode(const uint2& v, int k) const {
    const uint32_t w = (k >> 1) == 0 ? v.x : v.y;
    const uint32_t e = (k & 1) ? (w >> 16) : (w & 0xffffu);
    const int j = self - SPH_N16_BIAS + (int)(e & 0x7fffu) + ((e & 0x8000u) ? zOff : 0);
    return e == SPH_N16_EMPTY ? -1 : j;
  }
};

// "Which particles does this call act on", written once (include/sphmi.h states the rule per call): a particle is
// selected when its type (int)position.w is 1..3 with its bit set in typeMask, its cell key is valid (keys[j] < G: it lies in
// the declared grid) and its position lies in the half-open box x0 <= x < x1, likewise y and z. The box bounds may be ±inf;
// every comparison is written so that a NaN coordinate (or bound) fails it. The pieces are separate because not every caller
// has all three: the region kernels test type and key once per particle and the box once per region; sph_remove_region reads
// posOrig, which has no keys; sampling and the components have no box. SphSelector itself (box[6], typeMask) is in sph_common.h
// with the argument structs that carry it.
// Also here: the per-particle quantity a field number names (sph_histogram, sph_select_particles' streamed terms, sph_render_view).
#pragma once
#include "sph_common.h"
#include "sph_row_walk.h"

// (int) truncates, so 1.0 <= w < 4.0 selects; the range guard comes before the shift (a shift by a wild count is undefined).
// sph_type_key_selected below holds a second copy of this test: a change to one is a change to both.
__device__ __forceinline__ bool sph_type_selected(float w, uint32_t typeMask) {
  const int type = (int)w;
  return type >= 1 && type <= 3 && ((1u << type) & typeMask);
}

__device__ __forceinline__ bool sph_box_holds(float x0, float y0, float z0, float x1, float y1, float z1, float x, float y, float z) {
  return x0 <= x && x < x1 && y0 <= y && y < y1 && z0 <= z && z < z1;
}
// b = x0, y0, z0, x1, y1, z1
__device__ __forceinline__ bool sph_box_holds(const float (&b)[6], float x, float y, float z) {
  return sph_box_holds(b[0], b[1], b[2], b[3], b[4], b[5], x, y, z);
}

// Type and key of sorted particle j, whose position record is p. The type test is written out a second time here on purpose:
// through sph_type_selected the same test compiles to other code in the callers (k_cc_init among them).
__device__ __forceinline__ bool sph_type_key_selected(const SphDev& d, uint32_t typeMask, int j, const float4& p) {
  const int type = (int)p.w;
  return type >= 1 && type <= 3 && ((1u << type) & typeMask) && d.keys[j] < (uint32_t)d.G;
}

// the whole rule for sorted particle j
__device__ __forceinline__ bool sph_selected(const SphDev& d, const SphSelector& s, int j, const float4& p) {
  return sph_type_key_selected(d, s.typeMask, j, p) && sph_box_holds(s.box, p.x, p.y, p.z);
}

// entries >= 0 of sorted particle j's neighbour row, as the float the quantities use
__device__ __forceinline__ float sph_neighbor_count(const SphDev& d, int j) {
  int n = 0;
  sph_row_for_each_slot(d, j, [&](int nb) { n += nb >= 0; });
  return (float)n;
}

// quantity `field` of sorted particle j (position record p): 0 density, 1 speed, 2 pressure, 3 neighbour count, 4..6 x, y, z
__device__ __forceinline__ float sph_particle_quantity(const SphDev& d, int field, int j, const float4& p) {
  switch (field) {
    case 0: return d.rho[j];
    case 1: { const float4 v = d.sortedVel[j]; return sqrtf(v.x * v.x + v.y * v.y + v.z * v.z); }
    case 2: return d.rp[j].y;
    case 3: return sph_neighbor_count(d, j);
    case 4: return p.x;
    case 5: return p.y;
    default: return p.z;
  }
}

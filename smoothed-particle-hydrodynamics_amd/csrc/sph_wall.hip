// Per-body wall loads: what a set of boundary particles (a kinematic body, every wall, or the walls that belong to no body) did to
// each non-boundary particle in the last completed step -- the position shift and velocity reflection of integrate
// (integrate_particle in sph_pcisph.hip, the reference's computeInteractionWithBoundaryParticles), attributed to the set by its
// share w / wsum of the contact weights, and the set's K7 / K12 terms of the force decomposition (sph_forces.hip). Per particle and
// as deterministic region totals (include/sphmi.h: sph_wall_measure / sph_wall_diagnostics). Read-only on every
// solver array; the step's kernels are not touched.
//
// One lane per particle. The part of integrate in front of the contact is a stream over sortedPos, sortedVel, acc, accP, bndMask
// and, for the two scales, rho and rp; the slot walk runs only in waves where some lane has a boundary neighbour
// (__any(bndMask != 0), as integrate does it) and visits only the set bits of the lane's mask: the row through the 16-bit ids (the
// 32-bit row where that could not be written), per slot the neighbour's position, wall normal, density and (rho*, p).
// Membership of a slot's neighbour in the set is one bit test in a mask over SORTED indices, which k_wall_mask builds per call
// from the members' original ids through backIndex (integer atomicOr: the result does not depend on the order). The arithmetic is the contract's: plain `/` and sqrtf in the order integrate_particle,
// k_forces and pf_batch<false> write it (no contraction: the Makefile's flags).
//
// The records leave through LDS by the code k_force_records uses (a block's 256 records of 32 floats are one contiguous 32-KB piece
// of the output); the totals go word-major to the leaf kernel the force totals use and on through the fixed tree of sph_tree.h
// (sph_terms.h). No floating-point atomics.
#include "sph_common.h"
#include "sph_terms.h"  // the records' way out through LDS; leaf, tree and final of the region totals
#include "sph_wall_record.h"  // WallSet, wl_record: the per-particle record

#define WL_SUMS (WL_TERMS + 1)  // word 0 counts the particles, words 1..26 are the terms
#define WL_GROUP 9              // record words reduced together by the leaf: 27 = 3 x 9

enum { WL_RECORDS = 0, WL_TERMS_OUT = 1 };

// mask bit of backIndex[ids[r]] for the `count` members of a body (original ids; an id or an index outside 0..N-1 is never followed)
__global__ __launch_bounds__(SPH_BLOCK) void k_wall_mask(SphDev d, const uint32_t* __restrict__ ids, int count, uint32_t* __restrict__ mask) {
  const int r = blockIdx.x * SPH_BLOCK + threadIdx.x;
  if (r >= count) return;
  const uint32_t o = ids[r];
  if (o >= (uint32_t)d.N) return;
  const uint32_t j = d.backIndex[o];
  if (j >= (uint32_t)d.N) return;
  atomicOr(&mask[j >> 5], 1u << (j & 31));
}

size_t sphk_wall_mask_bytes(int N) { return sizeof(uint32_t) * (size_t)((std::max(N, 1) + 31) / 32); }

int sphk_wall_mask_clear(sph_solver* s, uint32_t* mask) {
  SPH_HIP(hipMemsetAsync(mask, 0, sphk_wall_mask_bytes(s->d.N), s->stream));
  return SPH_OK;
}

int sphk_wall_mask_add(sph_solver* s, const uint32_t* ids, int count, uint32_t* mask) {
  if (count <= 0) return SPH_OK;
  hipLaunchKernelGGL(k_wall_mask, dim3(sph_blocks(count)), dim3(SPH_BLOCK), 0, s->stream, s->d, ids, count, mask);
  SPH_HIP(hipGetLastError());
  return SPH_OK;
}

// (the record itself, wl_record, and the region terms, wl_terms, are in sph_wall_record.h: the fused body load evaluates them too)
// Particles first .. first + n (LIST: list[0..n), the selection's sorted indices) -> OUT == WL_RECORDS: n records of 32 floats at
// out, 16-byte aligned; OUT == WL_TERMS_OUT: the 26 terms of a region record at out[word * stride + r].
template <int OUT, bool LIST>
__global__ __launch_bounds__(SPH_BLOCK) void k_wall_records(SphDev d, WallSet ws, int first, int n, const int32_t* __restrict__ list,
                                                            float* __restrict__ out, size_t stride) {
  __shared__ float sm[OUT == WL_RECORDS ? SPH_BLOCK * (SPH_WALL_WORDS + 1) : 1];
  const int r = blockIdx.x * SPH_BLOCK + threadIdx.x;
  int id = -1;
  if (r < n) id = LIST ? list[r] : first + r;
  const bool active = id >= 0 && id < d.N;  // (a list entry outside 0..N-1 would be a defect of the selection: never followed)
  float rec[SPH_WALL_WORDS];
  float4 xi;
  wl_record(d, ws, active ? id : 0, active, rec, xi);
  if (OUT == WL_RECORDS) records_through_lds(rec, sm, n, out);
  else {
    if (r >= n) return;
    float* o = out + (size_t)r;
    float term[WL_TERMS];
    wl_terms(rec, xi, term);
#pragma unroll
    for (int w = 0; w < WL_TERMS; w++) o[(size_t)w * stride] = term[w];
  }
}

int sphk_wall_records(sph_solver* s, const uint32_t* mask, bool inverted, int first, int n, const int32_t* list, float* out) {
  if (n <= 0) return SPH_OK;
  const WallSet ws = {mask, inverted ? 1 : 0};
  if (list) hipLaunchKernelGGL((k_wall_records<WL_RECORDS, true>), dim3(sph_blocks(n)), dim3(SPH_BLOCK), 0, s->stream, s->d, ws, first, n, list, out, (size_t)0);
  else hipLaunchKernelGGL((k_wall_records<WL_RECORDS, false>), dim3(sph_blocks(n)), dim3(SPH_BLOCK), 0, s->stream, s->d, ws, first, n, list, out, (size_t)0);
  SPH_HIP(hipGetLastError());
  return SPH_OK;
}

// ---- region totals: 27 sums in three groups of nine (sph_terms.h) -----------------------------------------------------------------
int sphk_wall_diagnostics(sph_solver* s, const uint32_t* mask, bool inverted, const DiagArgs& a, float* terms, int pieceChunks,
                          double* scratch, double** records) {
  const WallSet ws = {mask, inverted ? 1 : 0};
  return sphk_terms_diagnostics<SPH_WALL_DIAG_WORDS, WL_SUMS, WL_GROUP>(
      s, a, terms, pieceChunks, scratch, records, [&](int first, int n, float* out, size_t stride) {
        hipLaunchKernelGGL((k_wall_records<WL_TERMS_OUT, false>), dim3(sph_blocks(n)), dim3(SPH_BLOCK), 0, s->stream, s->d, ws, first, n,
                           (const int32_t*)nullptr, out, stride);
      });
}

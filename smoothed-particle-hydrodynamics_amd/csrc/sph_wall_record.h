// The per-particle wall record (include/sphmi.h: sph_wall_measure) as one device function, for the kernels that
// evaluate it: k_wall_records (sph_wall.hip) and the fused body-load kernel (sph_body_dynamics.hip). Set: the wall set of the
// launch, anything wl_member() is overloaded for.
#pragma once
#include "sph_common.h"
#include "sph_row_batch.h"  // FmRow: a row in groups of four slots

// the wall set of a launch: every boundary particle, the sorted indices whose bit is set in mask, or those whose bit is clear
struct WallSet {
  const uint32_t* mask;  // 1 bit per SORTED particle, ceil(N / 32) words (null: SPH_WALL_ALL)
  int inverted;          // SPH_WALL_NO_BODY: mask is the union of all bodies
};

__device__ __forceinline__ bool wl_member(const WallSet& ws, int j) {
  if (!ws.mask) return true;
  const bool bit = (ws.mask[j >> 5] >> (j & 31)) & 1u;
  return ws.inverted ? !bit : bit;
}

// the wall set "the members of dynamic body `body`": bodyOf holds one byte per SORTED particle, the slot of the dynamic body the
// particle is a member of, or 0xff (k_bdyn_map, sph_body_dynamics.hip)
struct WallBodySet {
  const uint8_t* bodyOf;
  int body;
};

__device__ __forceinline__ bool wl_member(const WallBodySet& ws, int j) { return (int)ws.bodyOf[j] == ws.body; }

// The 32-word record of sorted particle `id` (include/sphmi.h) into rec[]; a boundary particle's, and an inactive lane's, is all
// zero. Called by every lane of a wave, so that the wave decides together whether anybody walks a row. xi: the particle's position.
template <class Set>
__device__ __forceinline__ void wl_record(const SphDev& d, const Set& ws, int id, bool active, float (&rec)[SPH_WALL_WORDS], float4& xi) {
#pragma unroll
  for (int w = 0; w < SPH_WALL_WORDS; w++) rec[w] = 0.f;
  const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
  float4 x = zero, v = zero, a0 = zero, a1 = zero;
  uint32_t bnd = 0u;
  bool moving = false;
  float2 rpi = make_float2(0.f, 0.f);
  if (active) {
    x = d.sortedPos[id];
    moving = (int)x.w != SPH_BOUNDARY_PARTICLE;
  }
  xi = x;
  if (moving) {
    v = d.sortedVel[id]; a0 = d.acc[id]; a1 = d.accP[id];
    bnd = d.bndMask[id];  // boundary neighbours, found by the forces kernel of the step
    rpi = d.rp[id];       // (rho*, p)
  }
  // before the contact, the expressions of integrate_particle
  const float ax = a0.x + a1.x, ay = a0.y + a1.y, az = a0.z + a1.z;
  float nvx = v.x + d.dt * ax, nvy = v.y + d.dt * ay, nvz = v.z + d.dt * az, nvw = v.w + d.dt * 0.f;
  float nx = x.x + d.posTimeStep * nvx, ny = x.y + d.posTimeStep * nvy, nz = x.z + d.posTimeStep * nvz;
  if (nx < d.xmin) nx = d.xmin;
  if (ny < d.ymin) ny = d.ymin;
  if (nz < d.zmin) nz = d.zmin;
  if (nx > d.xmax - 0.000001f) nx = d.xmax - 0.000001f;
  if (ny > d.ymax - 0.000001f) ny = d.ymax - 0.000001f;
  if (nz > d.zmax - 0.000001f) nz = d.zmax - 0.000001f;
  nvx = (v.x + nvx) * 0.5f; nvy = (v.y + nvy) * 0.5f; nvz = (v.z + nvz) * 0.5f; nvw = (v.w + nvw) * 0.5f;

  float ncx = 0.f, ncy = 0.f, ncz = 0.f, ncw = 0.f, wsum = 0.f, wsum2 = 0.f;
  float wS = 0.f, mS = 0.f, cS = 0.f;
  float S[9];  // the set's unscaled sums: V (viscous), T (tension), P (pressure), xyz each
#pragma unroll
  for (int q = 0; q < 9; q++) S[q] = 0.f;
  if (__any(bnd != 0u) && bnd != 0u) {  // waves in the bulk of the liquid skip the walk entirely
    const float pi_ = rpi.y;
    const float hq = d.hs * 0.25f;
    const FmRow t(d, id);
    const bool wideRow = (t.vec16(0).x & 0xffffu) == SPH_N16_WIDE;
    const int last = d.N - 1;
#pragma unroll 1
    for (int g = 0; g < 8; g++) {
      if (!((bnd >> (g * 4)) & 0xfu)) continue;
      const uint2 v16 = t.vec16(g);
      const float4 rq = t.dist4(g);
      const float rr[4] = {rq.x, rq.y, rq.z, rq.w};
#pragma unroll
      for (int k = 0; k < 4; k++) {
        if (!((bnd >> (g * 4 + k)) & 1u)) continue;
        int j = wideRow ? t.id_wide(g * 4 + k) : t.decode(v16, k);
        j = min(max(j, 0), last);  // (a set bit names a used slot; an index outside 0..N-1 would be a defect: never followed)
        const float4 pb = d.sortedPos[j];
        const float4 nb = d.sortedVel[j];  // wall normal, stored in the velocity slot
        // the contact weights, the expressions of integrate_particle
        float dist = (nx - pb.x) * (nx - pb.x);
        dist += (ny - pb.y) * (ny - pb.y);
        dist += (nz - pb.z) * (nz - pb.z);
        dist = sqrtf(dist);
        const float w = fmaxf(0.f, (d.r0 - dist) / d.r0);
        ncx += nb.x * w; ncy += nb.y * w; ncz += nb.z * w; ncw += nb.w * w;
        wsum += w;
        wsum2 += w * (d.r0 - dist);
        if (!wl_member(ws, j)) continue;
        wS += w;
        mS += 1.f;
        if (w > 0.f) cS += 1.f;
        // K7, the expressions of k_forces
        const float rhoj = d.rho[j];
        const float2 rpj = d.rp[j];
        const bool useF = rr[k] < d.hs;
        const float wv = d.hs - rr[k];
        float term[9];
        term[0] = (nb.x - v.x) * wv / rhoj;
        term[1] = (nb.y - v.y) * wv / rhoj;
        term[2] = (nb.z - v.z) * wv / rhoj;
        term[3] = d.surfTens * (x.x - pb.x);
        term[4] = d.surfTens * (x.y - pb.y);
        term[5] = d.surfTens * (x.z - pb.z);
        // K12, the expressions of pf_batch<false>
        const float ex = x.x - pb.x, ey = x.y - pb.y, ez = x.z - pb.z;
        const float d2 = ex * ex + ey * ey + ez * ez;
        const float r = sqrtf(d2) * d.simScale;
        float num = -(d.hs - r) * (d.hs - r) * 0.5f * (pi_ + rpj.y);
        num = (r < d.closeRf) ? -(hq - r) * (hq - r) * 0.5f * d.rho0delta : num;
        const float value = num / rpj.x;
        const float vx = ex * d.simScale, vy = ey * d.simScale, vz = ez * d.simScale;
        const float px = value * vx, py = value * vy, pz = value * vz;
        term[6] = px / r; term[7] = py / r; term[8] = pz / r;
        const bool useP = r < d.hs;
#pragma unroll
        for (int q = 0; q < 6; q++) S[q] = useF ? S[q] + term[q] : S[q];
#pragma unroll
        for (int q = 6; q < 9; q++) S[q] = useP ? S[q] + term[q] : S[q];
      }
    }
  }
  if (!moving) return;
  // the contact, the expressions of integrate_particle
  const float len2 = ((ncx * ncx + ncy * ncy) + ncz * ncz) + ncw * ncw;  // dot(float4, float4) incl. the .w lane
  const bool contact = len2 != 0.f;
  bool reflected = false;
  float shx = 0.f, shy = 0.f, shz = 0.f, share = 0.f;
  float ux = nvx, uy = nvy, uz = nvz, uw = nvw;
  if (contact) {
    const float len = sqrtf(len2);
    shx = ((ncx / len) * wsum2) / wsum;
    shy = ((ncy / len) * wsum2) / wsum;
    shz = ((ncz / len) * wsum2) / wsum;
    nx += shx; ny += shy; nz += shz;
    const float vn = ncx * nvx + ncy * nvy + ncz * nvz;
    if (vn < 0.f) {
      reflected = true;
      ux -= ncx * vn; uy -= ncy * vn; uz -= ncz * vn;
      ux *= 0.99f; uy *= 0.99f; uz *= 0.99f; uw *= 0.99f;
    }
    share = wS / wsum;
  }
  if (!d.hasElastic) { nx += 0.f; ny += 0.f; nz += 0.f; }  // integrate's fold of the membrane kernels' `position += 0`
  rec[0] = shx * share; rec[1] = shy * share; rec[2] = shz * share;
  rec[3] = (ux - nvx) * share; rec[4] = (uy - nvy) * share; rec[5] = (uz - nvz) * share;
  rec[6] = share; rec[7] = wS; rec[8] = cS; rec[9] = mS;
  // scaled whatever the sums hold: sP is negative, so a particle without a slot of the set has -0 in its pressure words, as in
  // sph_force_measure
  const float sF = d.massMu * (float)(d.del2W / (double)d.rho[id]);
  const float sP = (float)(d.massGradW / (double)rpi.x);
  rec[10] = S[0] * sF; rec[11] = S[1] * sF; rec[12] = S[2] * sF;
  rec[13] = S[3]; rec[14] = S[4]; rec[15] = S[5];
  rec[16] = S[6] * sP; rec[17] = S[7] * sP; rec[18] = S[8] * sP;
  rec[19] = nx; rec[20] = ny; rec[21] = nz;
  rec[22] = ux; rec[23] = uy; rec[24] = uz; rec[25] = uw;
  rec[26] = contact ? 1.f : 0.f;
  rec[27] = reflected ? 1.f : 0.f;
}

// the 26 per-particle terms of a region record (include/sphmi.h: sph_wall_diagnostics, words 1..26) from the particle's record
// (WL_TERMS: sph_common.h, beside sphk_wall_diagnostics, because the entry point sizes the terms' scratch with it)
__device__ __forceinline__ void wl_terms(const float (&rec)[SPH_WALL_WORDS], const float4& xi, float (&term)[WL_TERMS]) {
  const float* q = rec + 10;
  // h_S = (visc + pres) + tens; the cross products written like Lx, Ly, Lz of the diagnostics
  const float hx = (q[0] + q[6]) + q[3], hy = (q[1] + q[7]) + q[4], hz = (q[2] + q[8]) + q[5];
  term[0] = rec[26];
  term[1] = rec[6] > 0.f ? 1.f : 0.f;
  term[2] = (rec[27] != 0.f && rec[6] > 0.f) ? 1.f : 0.f;
#pragma unroll
  for (int w = 0; w < 6; w++) term[3 + w] = rec[w];
#pragma unroll
  for (int w = 0; w < 9; w++) term[9 + w] = rec[10 + w];
  term[18] = xi.y * rec[5] - xi.z * rec[4];
  term[19] = xi.z * rec[3] - xi.x * rec[5];
  term[20] = xi.x * rec[4] - xi.y * rec[3];
  term[21] = xi.y * hz - xi.z * hy;
  term[22] = xi.z * hx - xi.x * hz;
  term[23] = xi.x * hy - xi.y * hx;
  term[24] = rec[6];
  term[25] = rec[7];
}

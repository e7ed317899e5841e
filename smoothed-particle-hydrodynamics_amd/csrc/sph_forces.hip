// Force decomposition: the viscous, surface-tension and pressure accelerations of K7 (k_forces) and K12 (k_pressure_force),
// recomputed once from the sorted state of the last completed step and kept apart by the class of the neighbour that exerted
// them (1 liquid, 2 elastic, 3 boundary), per particle and as deterministic region totals (include/sphmi.h: sph_force_measure /
// sph_force_diagnostics). Read-only on every solver array; the step's kernels (sph_pcisph.hip) are not touched.
//
// One lane per particle, the gathers of K7 and K12 together: the row through the 16-bit ids (the 32-bit row where that could
// not be written), the stored distances for K7, r recomputed for K12, a neighbour's (x, y, z, type) and (v.xyz, rho) from ONE
// line of gatherRec and its (rho*, p) from rp, in batches of FM_BATCH neighbours with all gathers of a batch in flight
// together. Accumulation is masked and branch-free into the all-class sums (the step's own) and the three class sums; a skipped
// term leaves a sum untouched, exactly as in the step. The contract is the IEEE result, so the arithmetic is plain `/` and
// sqrtf in the order k_forces and pf_batch<false> write it (no contraction: the Makefile's flags).
//
// The records leave through LDS: a block's 256 records of 40 floats are one contiguous 40-KB piece of the output, written as
// 16-byte stores of consecutive lanes (a 160-byte stride per lane is the 4x write amplification of DESIGN.md §7 item 3).
// The totals never see the records: the same kernel writes the 48 per-particle terms of a region record word-major
// ([word][particle of the piece], coalesced as they stand) and a leaf kernel in the shape of k_diag_leaf feeds them to the fixed
// tree of sph_tree.h. No floating-point atomics.
#include "sph_common.h"
#include "sph_row_batch.h"  // FmRow: a row in groups of four slots
#include "sph_terms.h"  // the records' way out through LDS; leaf, tree and final of the region totals

#define FM_BATCH 8
#define FM_SUMS (FM_TERMS + 1)  // word 0 counts the particles, words 1..48 are the terms
#define FM_GROUP 7              // record words reduced together by the leaf: 49 = 7 x 7

enum { FM_RECORDS = 0, FM_TERMS_OUT = 1 };

__device__ __forceinline__ size_t fm_rec_index(int j, int part) {  // SphDev::gatherRec (k_pack_gather_records)
  return ((size_t)(j >> 2) << 3) + (size_t)(part << 2) + (size_t)(j & 3);
}

// The 40-word record of sorted particle `id` (include/sphmi.h) into rec[]; a boundary particle's is all zero. xi, vi: the
// particle's own position and velocity, for the caller's derived words.
__device__ __forceinline__ void fm_record(const SphDev& d, int id, float (&rec)[SPH_FORCE_WORDS], float4& xi, float4& vi) {
#pragma unroll
  for (int w = 0; w < SPH_FORCE_WORDS; w++) rec[w] = 0.f;
  xi = d.sortedPos[id];
  vi = d.sortedVel[id];
  if ((int)xi.w == SPH_BOUNDARY_PARTICLE) return;
  const float2 rpi = d.rp[id];  // (rho*, p)
  const float pi_ = rpi.y;
  const float hq = d.hs * 0.25f;
  const FmRow t(d, id);
  // [0] the step's own sums over all used slots, [c] those of class c: V (viscous), T (tension), P (pressure), xyz each
  float S[4][9];
  float cnt[3] = {0.f, 0.f, 0.f};
#pragma unroll
  for (int c = 0; c < 4; c++)
#pragma unroll
    for (int w = 0; w < 9; w++) S[c][w] = 0.f;
  bool wideRow = false;
#pragma unroll 1  // a real loop, as in k_forces: unrolled, the loads of all four batches are hoisted and the registers run out
  for (int b = 0; b < 32 / FM_BATCH; b++) {
    int jj[FM_BATCH];
    float rr[FM_BATCH];
#pragma unroll
    for (int q = 0; q < FM_BATCH / 4; q++) {
      const float4 rq = t.dist4(b * (FM_BATCH / 4) + q);
      rr[4 * q] = rq.x; rr[4 * q + 1] = rq.y; rr[4 * q + 2] = rq.z; rr[4 * q + 3] = rq.w;
    }
#pragma unroll
    for (int q = 0; q < FM_BATCH / 4; q++) {
      const uint2 v = t.vec16(b * (FM_BATCH / 4) + q);
      if (b == 0 && q == 0) wideRow = (v.x & 0xffffu) == SPH_N16_WIDE;
#pragma unroll
      for (int k = 0; k < 4; k++) jj[4 * q + k] = t.decode(v, k);
    }
    if (wideRow) {  // rare
#pragma unroll
      for (int k = 0; k < FM_BATCH; k++) jj[k] = t.id_wide(b * FM_BATCH + k);
    }
    float4 xj[FM_BATCH], vr[FM_BATCH];
    float2 rpj[FM_BATCH];
#pragma unroll
    for (int k = 0; k < FM_BATCH; k++) {
      const int jc = max(jj[k], 0);  // an empty slot reads record 0 and is masked out of every sum
      xj[k] = d.gatherRec[fm_rec_index(jc, 0)];
      vr[k] = d.gatherRec[fm_rec_index(jc, 1)];  // (v.xyz, rho); a boundary neighbour's v is its wall normal (sphFluid.cl:653)
      rpj[k] = d.rp[jc];
    }
#pragma unroll
    for (int k = 0; k < FM_BATCH; k++) {
      const bool valid = jj[k] != -1;
      const int cls = (int)xj[k].w;
      // K7, the expressions of k_forces
      const bool useF = valid && rr[k] < d.hs;
      const float w = d.hs - rr[k];
      float term[9];
      term[0] = (vr[k].x - vi.x) * w / vr[k].w;
      term[1] = (vr[k].y - vi.y) * w / vr[k].w;
      term[2] = (vr[k].z - vi.z) * w / vr[k].w;
      term[3] = d.surfTens * (xi.x - xj[k].x);
      term[4] = d.surfTens * (xi.y - xj[k].y);
      term[5] = d.surfTens * (xi.z - xj[k].z);
      // K12, the expressions of pf_batch<false>
      const float ex = xi.x - xj[k].x, ey = xi.y - xj[k].y, ez = xi.z - xj[k].z;
      const float d2 = ex * ex + ey * ey + ez * ez;
      const float r = sqrtf(d2) * d.simScale;
      float num = -(d.hs - r) * (d.hs - r) * 0.5f * (pi_ + rpj[k].y);
      num = (r < d.closeRf) ? -(hq - r) * (hq - r) * 0.5f * d.rho0delta : num;
      const float value = num / rpj[k].x;
      const float vx = ex * d.simScale, vy = ey * d.simScale, vz = ez * d.simScale;
      const float ax = value * vx, ay = value * vy, az = value * vz;
      term[6] = ax / r; term[7] = ay / r; term[8] = az / r;
      const bool useP = valid && r < d.hs;
#pragma unroll
      for (int c = 0; c < 4; c++) {
        const bool mine = c == 0 || cls == c;
        const bool mf = useF && mine, mp = useP && mine;
#pragma unroll
        for (int q = 0; q < 6; q++) S[c][q] = mf ? S[c][q] + term[q] : S[c][q];
#pragma unroll
        for (int q = 6; q < 9; q++) S[c][q] = mp ? S[c][q] + term[q] : S[c][q];
        if (c > 0) cnt[c - 1] = mf ? cnt[c - 1] + 1.f : cnt[c - 1];
      }
    }
  }
  const float sF = d.massMu * (float)(d.del2W / (double)d.rho[id]);
  const float sP = (float)(d.massGradW / (double)rpi.x);
#pragma unroll
  for (int c = 1; c < 4; c++) {
    float* o = rec + 9 * (c - 1);
    o[0] = S[c][0] * sF; o[1] = S[c][1] * sF; o[2] = S[c][2] * sF;
    o[3] = S[c][3]; o[4] = S[c][4]; o[5] = S[c][5];
    o[6] = S[c][6] * sP; o[7] = S[c][7] * sP; o[8] = S[c][8] * sP;
  }
  rec[27] = cnt[0]; rec[28] = cnt[1]; rec[29] = cnt[2];
  rec[30] = S[0][0] * sF + d.gravx + S[0][3];  // as k_forces writes the acceleration
  rec[31] = S[0][1] * sF + d.gravy + S[0][4];
  rec[32] = S[0][2] * sF + d.gravz + S[0][5];
  rec[33] = S[0][6] * sP; rec[34] = S[0][7] * sP; rec[35] = S[0][8] * sP;
}

// Particles first .. first + n (LIST: list[0..n), the selection's sorted indices) -> OUT == FM_RECORDS: n records of 40 floats
// at out, 16-byte aligned; OUT == FM_TERMS_OUT: the 48 terms of a region record at out[word * stride + r].
template <int OUT, bool LIST>
__global__ __launch_bounds__(SPH_BLOCK) void k_force_records(SphDev d, int first, int n, const int32_t* __restrict__ list,
                                                             float* __restrict__ out, size_t stride) {
  __shared__ float sm[OUT == FM_RECORDS ? SPH_BLOCK * (SPH_FORCE_WORDS + 1) : 1];
  const int r = blockIdx.x * SPH_BLOCK + threadIdx.x;
  int id = -1;
  if (r < n) id = LIST ? list[r] : first + r;
  const bool active = id >= 0 && id < d.N;  // (a list entry outside 0..N-1 would be a defect of the selection: never followed)
  float rec[SPH_FORCE_WORDS];
  float4 xi = make_float4(0.f, 0.f, 0.f, 0.f), vi = xi;
  if (active) fm_record(d, id, rec, xi, vi);
  else {
#pragma unroll
    for (int w = 0; w < SPH_FORCE_WORDS; w++) rec[w] = 0.f;
  }
  if (OUT == FM_RECORDS) records_through_lds(rec, sm, n, out);
  else {
    if (r >= n) return;
    float* o = out + (size_t)r;
#pragma unroll
    for (int w = 0; w < 27; w++) o[(size_t)w * stride] = rec[w];
#pragma unroll
    for (int w = 0; w < 6; w++) o[(size_t)(27 + w) * stride] = rec[30 + w];
#pragma unroll
    for (int c = 0; c < 3; c++) {
      const float* q = rec + 9 * c;
      // h_c = (visc_c + pres_c) + tens_c; tau_c = x_i x h_c written like Lx, Ly, Lz of the diagnostics; w_c = h_c . v_i
      const float hx = (q[0] + q[6]) + q[3], hy = (q[1] + q[7]) + q[4], hz = (q[2] + q[8]) + q[5];
      o[(size_t)(33 + 3 * c) * stride] = xi.y * hz - xi.z * hy;
      o[(size_t)(34 + 3 * c) * stride] = xi.z * hx - xi.x * hz;
      o[(size_t)(35 + 3 * c) * stride] = xi.x * hy - xi.y * hx;
      o[(size_t)(42 + c) * stride] = (hx * vi.x + hy * vi.y) + hz * vi.z;
      o[(size_t)(45 + c) * stride] = rec[27 + c];
    }
  }
}

int sphk_force_records(sph_solver* s, int first, int n, const int32_t* list, float* out) {
  if (n <= 0) return SPH_OK;
  if (list) hipLaunchKernelGGL((k_force_records<FM_RECORDS, true>), dim3(sph_blocks(n)), dim3(SPH_BLOCK), 0, s->stream, s->d, first, n, list, out, (size_t)0);
  else hipLaunchKernelGGL((k_force_records<FM_RECORDS, false>), dim3(sph_blocks(n)), dim3(SPH_BLOCK), 0, s->stream, s->d, first, n, list, out, (size_t)0);
  SPH_HIP(hipGetLastError());
  return SPH_OK;
}

// ---- region totals: 49 sums in seven groups of seven (sph_terms.h) ---------------------------------------------------------------
int sphk_force_diagnostics(sph_solver* s, const DiagArgs& a, float* terms, int pieceChunks, double* scratch, double** records) {
  return sphk_terms_diagnostics<SPH_FORCE_DIAG_WORDS, FM_SUMS, FM_GROUP>(
      s, a, terms, pieceChunks, scratch, records, [&](int first, int n, float* out, size_t stride) {
        hipLaunchKernelGGL((k_force_records<FM_TERMS_OUT, false>), dim3(sph_blocks(n)), dim3(SPH_BLOCK), 0, s->stream, s->d, first, n,
                           (const int32_t*)nullptr, out, stride);
      });
}

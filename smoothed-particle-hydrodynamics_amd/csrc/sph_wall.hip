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
// The records leave through LDS as in k_force_records (a block's 256 records of 32 floats are one contiguous 32-KB piece of the
// output); the totals go word-major to a leaf kernel in the shape of k_force_leaf and on through the fixed tree of sph_tree.h. No
// floating-point atomics.
#include "sph_common.h"
#include "sph_row_batch.h"  // FmRow: a row in groups of four slots
#include "sph_selector.h"  // the selection rule of the region totals
#include "sph_tree.h"

#include <algorithm>

#define WL_LDS_STRIDE (SPH_WALL_WORDS + 1)  // 33 words: lane-strided ds_write_b32 without bank conflicts
#define WL_TERMS 26                         // words 1..26 of a region record (word 0 counts the particles)
#define WL_SUMS (WL_TERMS + 1)
#define WL_GROUP 9                          // record words reduced together by the leaf: 27 = 3 x 9

enum { WL_RECORDS = 0, WL_TERMS_OUT = 1 };

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

// The 32-word record of sorted particle `id` (include/sphmi.h) into rec[]; a boundary particle's, and an inactive lane's, is all
// zero. Called by every lane of a wave, so that the wave decides together whether anybody walks a row. xi: the particle's position.
__device__ __forceinline__ void wl_record(const SphDev& d, const WallSet& ws, int id, bool active, float (&rec)[SPH_WALL_WORDS], float4& xi) {
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

// Particles first .. first + n (LIST: list[0..n), the selection's sorted indices) -> OUT == WL_RECORDS: n records of 32 floats at
// out, 16-byte aligned; OUT == WL_TERMS_OUT: the 26 terms of a region record at out[word * stride + r].
template <int OUT, bool LIST>
__global__ __launch_bounds__(SPH_BLOCK) void k_wall_records(SphDev d, WallSet ws, int first, int n, const int32_t* __restrict__ list,
                                                            float* __restrict__ out, size_t stride) {
  __shared__ float sm[OUT == WL_RECORDS ? SPH_BLOCK * WL_LDS_STRIDE : 1];
  const int t = threadIdx.x;
  const int r = blockIdx.x * SPH_BLOCK + t;
  int id = -1;
  if (r < n) id = LIST ? list[r] : first + r;
  const bool active = id >= 0 && id < d.N;  // (a list entry outside 0..N-1 would be a defect of the selection: never followed)
  float rec[SPH_WALL_WORDS];
  float4 xi;
  wl_record(d, ws, active ? id : 0, active, rec, xi);
  if (OUT == WL_RECORDS) {
#pragma unroll
    for (int w = 0; w < SPH_WALL_WORDS; w++) sm[t * WL_LDS_STRIDE + w] = rec[w];
    __syncthreads();
    const int rows = min(SPH_BLOCK, n - blockIdx.x * SPH_BLOCK);  // records of this block
    float4* dst = reinterpret_cast<float4*>(out + (size_t)blockIdx.x * SPH_BLOCK * SPH_WALL_WORDS);
    const int quads = rows * (SPH_WALL_WORDS / 4);
    for (int q = t; q < quads; q += SPH_BLOCK) {
      const float* src = sm + (q / (SPH_WALL_WORDS / 4)) * WL_LDS_STRIDE + 4 * (q % (SPH_WALL_WORDS / 4));
      dst[q] = make_float4(src[0], src[1], src[2], src[3]);
    }
  } else {
    if (r >= n) return;
    float* o = out + (size_t)r;
    const float* q = rec + 10;
    // h_S = (visc + pres) + tens; the cross products written like Lx, Ly, Lz of the diagnostics
    const float hx = (q[0] + q[6]) + q[3], hy = (q[1] + q[7]) + q[4], hz = (q[2] + q[8]) + q[5];
    o[(size_t)0 * stride] = rec[26];
    o[(size_t)1 * stride] = rec[6] > 0.f ? 1.f : 0.f;
    o[(size_t)2 * stride] = (rec[27] != 0.f && rec[6] > 0.f) ? 1.f : 0.f;
#pragma unroll
    for (int w = 0; w < 6; w++) o[(size_t)(3 + w) * stride] = rec[w];
#pragma unroll
    for (int w = 0; w < 9; w++) o[(size_t)(9 + w) * stride] = rec[10 + w];
    o[(size_t)18 * stride] = xi.y * rec[5] - xi.z * rec[4];
    o[(size_t)19 * stride] = xi.z * rec[3] - xi.x * rec[5];
    o[(size_t)20 * stride] = xi.x * rec[4] - xi.y * rec[3];
    o[(size_t)21 * stride] = xi.y * hz - xi.z * hy;
    o[(size_t)22 * stride] = xi.z * hx - xi.x * hz;
    o[(size_t)23 * stride] = xi.x * hy - xi.y * hx;
    o[(size_t)24 * stride] = rec[6];
    o[(size_t)25 * stride] = rec[7];
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

// ---- region totals: the shape of sph_forces.hip's, 27 sums in three groups of nine -------------------------------------------------
// Partials of a level: part[(region * SPH_WALL_DIAG_WORDS + word) * chunks + chunk], read coalesced by the next level.
__device__ __forceinline__ size_t wl_at(int region, int word, int chunks, int chunk) {
  return ((size_t)(region * SPH_WALL_DIAG_WORDS + word)) * (size_t)chunks + (size_t)chunk;
}

// Level 0 for the chunks [firstChunk, firstChunk + gridDim.x) whose terms lie at `terms` (word-major, `stride` particles per
// word, particle firstChunk * 1024 first). One block per chunk of 1024 particles in k_diag_leaf's layout: thread t holds
// elements t, t + 256, t + 512, t + 768 (strides 512 and 256 in registers), 128 and 64 through LDS, 32 ... 1 inside a wave.
__global__ __launch_bounds__(SPH_BLOCK) void k_wall_leaf(SphDev d, DiagArgs a, const float* __restrict__ terms, size_t stride,
                                                         int firstChunk, double* __restrict__ part, int chunks) {
  __shared__ double sh[WL_GROUP][SPH_BLOCK];
  const int t = threadIdx.x, chunk = firstChunk + blockIdx.x, lane = t & 63, wave = t >> 6;
  float px[4], py[4], pz[4];
  bool ok[4];
#pragma unroll
  for (int e = 0; e < 4; e++) {
    const int j = chunk * DIAG_CHUNK + e * SPH_BLOCK + t;
    ok[e] = false;
    px[e] = py[e] = pz[e] = 0.f;
    if (j < d.N) {
      const float4 p = d.sortedPos[j];
      ok[e] = sph_type_key_selected(d, a.typeMask, j, p);
      px[e] = p.x; py[e] = p.y; pz[e] = p.z;
    }
  }
  for (int g = 0; g < WL_SUMS / WL_GROUP; g++) {
    float f[4][WL_GROUP];
#pragma unroll
    for (int e = 0; e < 4; e++) {
      const int j = chunk * DIAG_CHUNK + e * SPH_BLOCK + t;
      const size_t at = (size_t)(blockIdx.x * DIAG_CHUNK + e * SPH_BLOCK + t);
#pragma unroll
      for (int k = 0; k < WL_GROUP; k++) {
        const int w = g * WL_GROUP + k;  // record word; word 0 counts
        f[e][k] = w == 0 ? 1.0f : (j < d.N ? terms[(size_t)(w - 1) * stride + at] : 0.f);
      }
    }
    for (int r = 0; r < a.count; r++) {
      const float x0 = a.box[r][0], y0 = a.box[r][1], z0 = a.box[r][2], x1 = a.box[r][3], y1 = a.box[r][4], z1 = a.box[r][5];
      bool sel[4];
#pragma unroll
      for (int e = 0; e < 4; e++) sel[e] = ok[e] && sph_box_holds(x0, y0, z0, x1, y1, z1, px[e], py[e], pz[e]);
      // no particle of this chunk in the region: every sum of +0.0 terms is +0.0, which is what the tree below would produce
      if (!__syncthreads_or(sel[0] || sel[1] || sel[2] || sel[3])) {
        if (t < WL_GROUP) part[wl_at(r, g * WL_GROUP + t, chunks, chunk)] = 0.0;
        continue;
      }
#pragma unroll
      for (int k = 0; k < WL_GROUP; k++) {
        double q[4];
#pragma unroll
        for (int e = 0; e < 4; e++) q[e] = sel[e] ? (double)f[e][k] : 0.0;
        sh[k][t] = (q[0] + q[2]) + (q[1] + q[3]);
      }
      __syncthreads();
      if (t < 128) {
#pragma unroll
        for (int k = 0; k < WL_GROUP; k++) sh[k][t] = sh[k][t] + sh[k][t + 128];
      }
      __syncthreads();
      for (int k = wave; k < WL_GROUP; k += 4) {
        const double x = diag_wave_sum(sh[k][lane] + sh[k][lane + 64]);
        if (lane == 0) part[wl_at(r, g * WL_GROUP + k, chunks, chunk)] = x;
      }
      __syncthreads();  // sh is reused by the next region
    }
  }
}

// Upper levels: `nIn` partials per word and region -> ceil(nIn / 1024), the same tree. One block per output chunk, region and word.
__global__ __launch_bounds__(SPH_BLOCK) void k_wall_upper(const double* __restrict__ in, int nIn, double* __restrict__ out, int nOut) {
  __shared__ double sh[SPH_BLOCK];
  const int chunk = blockIdx.x, r = blockIdx.y, w = blockIdx.z;
  const double x = diag_block_reduce<DIAG_OP_SUM>(in + wl_at(r, w, nIn, 0), nIn, chunk, 0.0, sh);
  if (threadIdx.x == 0) out[wl_at(r, w, nOut, chunk)] = x;
}

__global__ void k_wall_final(const double* __restrict__ top /* one chunk per word */, double* __restrict__ out) {
  const int r = blockIdx.x, w = threadIdx.x;  // SPH_WALL_DIAG_WORDS threads
  out[r * SPH_WALL_DIAG_WORDS + w] = w < WL_SUMS ? top[wl_at(r, w, 1, 0)] : 0.0;
}

static int wl_chunks(int n) { return n > 0 ? (n + DIAG_CHUNK - 1) / DIAG_CHUNK : 1; }

size_t sphk_wall_diag_scratch_doubles(int N, int regions) {
  size_t total = 0;
  for (int c = wl_chunks(N);; c = wl_chunks(c)) {
    total += (size_t)c;
    if (c == 1) break;
  }
  return (total + 1) * (size_t)regions * SPH_WALL_DIAG_WORDS;  // the levels' partials, then the records
}

size_t sphk_wall_terms_bytes(int chunks) { return sizeof(float) * WL_TERMS * DIAG_CHUNK * (size_t)chunks; }

int sphk_wall_diagnostics(sph_solver* s, const uint32_t* mask, bool inverted, const DiagArgs& a, float* terms, int pieceChunks,
                          double* scratch, double** records) {
  const int R = a.count, N = s->d.N;
  const WallSet ws = {mask, inverted ? 1 : 0};
  int chunks = wl_chunks(N);
  double* cur = scratch;
  const size_t stride = (size_t)pieceChunks * DIAG_CHUNK;
  for (int c0 = 0; c0 < chunks; c0 += pieceChunks) {
    const int nC = std::min(pieceChunks, chunks - c0);
    const int first = c0 * DIAG_CHUNK, n = std::min(nC * DIAG_CHUNK, N - first);
    if (n > 0) hipLaunchKernelGGL((k_wall_records<WL_TERMS_OUT, false>), dim3(sph_blocks(n)), dim3(SPH_BLOCK), 0, s->stream, s->d, ws, first, n,
                                  (const int32_t*)nullptr, terms, stride);
    hipLaunchKernelGGL(k_wall_leaf, dim3(nC), dim3(SPH_BLOCK), 0, s->stream, s->d, a, (const float*)terms, stride, c0, cur, chunks);
    SPH_HIP(hipGetLastError());
  }
  while (chunks > 1) {
    const int nOut = wl_chunks(chunks);
    double* next = cur + (size_t)R * SPH_WALL_DIAG_WORDS * (size_t)chunks;
    hipLaunchKernelGGL(k_wall_upper, dim3(nOut, R, WL_SUMS), dim3(SPH_BLOCK), 0, s->stream, (const double*)cur, chunks, next, nOut);
    SPH_HIP(hipGetLastError());
    cur = next; chunks = nOut;
  }
  double* out = cur + (size_t)R * SPH_WALL_DIAG_WORDS;
  hipLaunchKernelGGL(k_wall_final, dim3(R), dim3(SPH_WALL_DIAG_WORDS), 0, s->stream, (const double*)cur, out);
  SPH_HIP(hipGetLastError());
  return *records = out, SPH_OK;
}

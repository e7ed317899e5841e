// Elastic-matter diagnostics: per-particle spring strain and spring / contraction accelerations, per-muscle-group reductions and
// membrane triangle areas, read from the sorted state of the last completed step and the tables given to sph_create
// (include/sphmi.h: sph_elastic_measure / sph_muscle_diagnostics / sph_membrane_measure). Read-only on every
// solver array; the step's kernels (sph_elastic.hip) are not touched.
//
// The connection table is 32 float4 slots per elastic particle, so everything here gives a row HALF A WAVE, lane = slot (as
// k_membranes does): the table is read as one contiguous 512-byte transaction per row and the 32 backIndex -> sortedPos gathers
// of a row are in flight together, where k_elastic walks them one after the other in one lane. The problem is small (the worm:
// 10 k rows, 325 k slots), so the kernels are bound by latency and launches, not by bandwidth.
//
// The group sums are doubles added in the fixed tree of the diagnostics contract (sph_tree.h) over the numOfElasticP * 32 slot
// terms in table order: one block per chunk of 1024 slots (32 rows) runs the tree only for the groups that occur in its chunk
// -- an absent group's partial is +0.0 and is put there by the fill kernel -- and the upper levels reduce the dense
// [group][word][chunk] table. No floating-point atomics.
#include "sph_common.h"
#include "sph_tree.h"

#define EM_ROWS (SPH_BLOCK / 32)  // rows of the connection table per block
#define EM_SUMS 12

// record words that are tree sums, in the order of the leaf's LDS rows; words 7 and 8 are the extremes, 1 and 15 are constants
__device__ static const int kEmSumWord[EM_SUMS] = {0, 2, 3, 4, 5, 6, 9, 10, 11, 12, 13, 14};

// (the rows of the tree are the groups, SPH_MUSCLE_WORDS words each)

// One slot of the connection table as the contract defines it. v = (x_i - x_j) * simScale; r, dr, e in float, in k_elastic's
// order; m = 0 for "no muscle group".
struct EmSlot {
  bool live;
  int m;
  float L0, r, dr, e, sig;
  float vx, vy, vz;
  float xi, yi, zi;
};

// Slot `slot` of row `row`; the 32 lanes of a half-wave call this together with slot = their lane (both halves of a wave, and
// all rows of a block, run it in step: the row's end comes from a ballot). An id outside 0..N-1 is reported in *bad and not
// followed; the slot then counts as dead.
__device__ __forceinline__ EmSlot em_slot(const SphDev& d, int row, int slot, uint32_t* __restrict__ bad) {
  EmSlot o = {};
  const bool rowOk = row < d.numElastic;
  float4 conn = make_float4(-1.f, 0.f, 0.f, 0.f);
  if (rowOk) conn = d.elastic[(size_t)row * SPH_MAXN + slot];  // (j + 0.1, r0_ij, muscle id . colour, 0)
  const int jo = (int)conn.x;
  const unsigned long long ends = __ballot(jo == -1);  // the first NO_PARTICLE_ID ends the row (sphFluid.cl:802-803)
  const uint32_t mine = (uint32_t)(ends >> (threadIdx.x & 32));
  const int first = mine ? __ffs(mine) - 1 : SPH_MAXN;
  if (!rowOk || slot >= first) return o;
  const int io = row + d.elasticOffset;
  if (jo < 0 || jo >= d.N || io < 0 || io >= d.N) { atomicOr(bad, 1u); return o; }
  const uint32_t i = d.backIndex[io], j = d.backIndex[jo];
  if (i >= (uint32_t)d.N || j >= (uint32_t)d.N) { atomicOr(bad, 2u); return o; }
  const float4 xi = d.sortedPos[i], xj = d.sortedPos[j];
  o.live = true;
  o.xi = xi.x; o.yi = xi.y; o.zi = xi.z;
  o.vx = (xi.x - xj.x) * d.simScale; o.vy = (xi.y - xj.y) * d.simScale; o.vz = (xi.z - xj.z) * d.simScale;
  o.r = sqrtf(((o.vx * o.vx + o.vy * o.vy) + o.vz * o.vz) + 0.f * 0.f);  // dot(float4, float4) with .w = 0, as k_elastic
  o.L0 = conn.y;
  o.dr = o.r - o.L0;
  o.e = o.L0 > 0.f ? o.dr / o.L0 : 0.f;
  const int m = (int)conn.z;
  if (m >= 1 && m <= d.muscleCount) { o.m = m; o.sig = d.muscle[m - 1]; }
  return o;
}

// ---- per-particle records ---------------------------------------------------------------------------------------------------
// The per-slot terms are parked in LDS and lane 0 of the half-wave adds them in slot order: the float sums are order-defined
// (they are the step's accelerations, as sums of their own). Any output pointer may be null.
__global__ __launch_bounds__(SPH_BLOCK) void k_elastic_terms(SphDev d, int32_t* __restrict__ sortedIndex, uint32_t* __restrict__ origId,
                                                             float4* __restrict__ records, float2* __restrict__ connections,
                                                             uint32_t* __restrict__ bad) {
  __shared__ float sm[EM_ROWS][32][9];  // e, dr*dr, s.xyz, c.xyz, flags (1 live, 2 muscle, 4 spring term, 8 contraction term)
  const int lane = threadIdx.x & 31, group = threadIdx.x >> 5;
  const int row = blockIdx.x * EM_ROWS + group;
  const EmSlot o = em_slot(d, row, lane, bad);
  float sx = 0.f, sy = 0.f, sz = 0.f, cx = 0.f, cy = 0.f, cz = 0.f;
  int flags = 0;
  if (o.live) {
    flags = 1 | (o.m > 0 ? 2 : 0);
    if (o.r != 0.f) {  // exactly the terms k_elastic adds to the acceleration
      const float kSpring = 600000000.f;
      flags |= 4;
      sx = -(o.vx / o.r) * o.dr * kSpring;
      sy = -(o.vy / o.r) * o.dr * kSpring;
      sz = -(o.vz / o.r) * o.dr * kSpring;
      if (o.m > 0 && o.sig > 0.f) {
        flags |= 8;
        cx = -(o.vx / o.r) * o.sig * 800.f;
        cy = -(o.vy / o.r) * o.sig * 800.f;
        cz = -(o.vz / o.r) * o.sig * 800.f;
      }
    }
  }
  float* mine = sm[group][lane];
  mine[0] = o.e; mine[1] = o.dr * o.dr;
  mine[2] = sx; mine[3] = sy; mine[4] = sz; mine[5] = cx; mine[6] = cy; mine[7] = cz;
  mine[8] = __int_as_float(flags);
  if (connections && row < d.numElastic) connections[(size_t)row * SPH_MAXN + lane] = o.live ? make_float2(o.r, o.dr) : make_float2(-1.f, 0.f);
  __syncthreads();
  if (lane != 0 || row >= d.numElastic) return;
  int n = 0, nMuscle = 0;
  float eMin = INFINITY, eMax = -INFINITY, eSum = 0.f, d2Sum = 0.f;
  float ax = 0.f, ay = 0.f, az = 0.f, bx = 0.f, by = 0.f, bz = 0.f;
  for (int nc = 0; nc < SPH_MAXN; nc++) {
    const float* q = sm[group][nc];
    const int f = __float_as_int(q[8]);
    if (!(f & 1)) continue;
    n++;
    nMuscle += (f >> 1) & 1;
    eMin = q[0] < eMin ? q[0] : eMin;
    eMax = q[0] > eMax ? q[0] : eMax;
    eSum += q[0];
    d2Sum += q[1];
    if (f & 4) { ax += q[2]; ay += q[3]; az += q[4]; }
    if (f & 8) { bx += q[5]; by += q[6]; bz += q[7]; }
  }
  if (n == 0) eMin = eMax = 0.f;
  const int io = row + d.elasticOffset;
  if (sortedIndex) sortedIndex[row] = (io >= 0 && io < d.N) ? (int32_t)d.backIndex[io] : -1;
  if (origId) origId[row] = (uint32_t)io;
  if (records) {
    records[3 * (size_t)row + 0] = make_float4((float)n, (float)nMuscle, eMin + 0.0f, eMax + 0.0f);
    records[3 * (size_t)row + 1] = make_float4(eSum, d2Sum, ax, ay);
    records[3 * (size_t)row + 2] = make_float4(az, bx, by, bz);
  }
}

int sphk_elastic_measure(sph_solver* s, int32_t* sortedIndex, uint32_t* origId, float* records, float* connections, uint32_t* bad) {
  SPH_HIP(hipMemsetAsync(bad, 0, sizeof(uint32_t), s->stream));
  hipLaunchKernelGGL(k_elastic_terms, dim3(sph_blocks(s->d.numElastic, EM_ROWS)), dim3(SPH_BLOCK), 0, s->stream, s->d, sortedIndex, origId,
                     (float4*)records, (float2*)connections, bad);
  SPH_HIP(hipGetLastError());
  return SPH_OK;
}

// ---- per-group reductions ----------------------------------------------------------------------------------------------------
// Level 0's table before the leaf: +0.0 everywhere (an absent group's sums), the extremes' identities in words 7 and 8.
__global__ __launch_bounds__(SPH_BLOCK) void k_muscle_fill(double* __restrict__ part, int chunks, size_t total) {
  const size_t i = (size_t)blockIdx.x * SPH_BLOCK + threadIdx.x;
  if (i >= total) return;
  const int w = (int)((i / (size_t)chunks) % SPH_MUSCLE_WORDS);
  part[i] = w == 7 ? (double)INFINITY : w == 8 ? -(double)INFINITY : 0.0;
}

// One block per chunk of 1024 slots = 32 rows; thread t holds slots t, t + 256, t + 512, t + 768 of the chunk, i.e. slot t % 32
// of four rows, so every half-wave still owns whole rows and all four gathers of a thread are issued together. The groups that
// occur in the chunk are collected in an LDS bit set; the tree runs once per such group, in k_diag_leaf's stride layout:
// 512 and 256 in registers, 128 and 64 through LDS, 32 ... 1 inside a wave.
__global__ __launch_bounds__(SPH_BLOCK) void k_muscle_leaf(SphDev d, double* __restrict__ part, int chunks, uint32_t* __restrict__ bad) {
  __shared__ double sh[EM_SUMS][SPH_BLOCK];
  __shared__ float shx[4][2];
  __shared__ uint32_t present[4096 / 32 + 1];  // sph_create admits muscleCount <= 4096
  const int t = threadIdx.x, chunk = blockIdx.x, lane = t & 63, wave = t >> 6;
  const int words = d.muscleCount / 32 + 1;
  for (int w = t; w < words; w += SPH_BLOCK) present[w] = 0u;
  __syncthreads();
  float f[4][EM_SUMS - 1];  // L0, r, dr, dr*dr, e, dr * kSpring, sig * 800, x, y, z, (r == 0): sum words after n
  int grp[4];
#pragma unroll
  for (int e = 0; e < 4; e++) {
    const EmSlot o = em_slot(d, chunk * (DIAG_CHUNK / 32) + e * EM_ROWS + (t >> 5), t & 31, bad);
    grp[e] = o.live ? o.m : -1;
    f[e][0] = o.L0; f[e][1] = o.r; f[e][2] = o.dr; f[e][3] = o.dr * o.dr; f[e][4] = o.e;
    f[e][5] = o.dr * 600000000.f;
    f[e][6] = (o.r != 0.f && o.sig > 0.f) ? o.sig * 800.f : 0.f;
    f[e][7] = o.xi; f[e][8] = o.yi; f[e][9] = o.zi;
    f[e][10] = o.r == 0.f ? 1.0f : 0.0f;
    if (o.live) atomicOr(&present[o.m >> 5], 1u << (o.m & 31));
  }
  __syncthreads();
  for (int pw = 0; pw < words; pw++) {
    uint32_t bits = present[pw];  // the same value in every thread
    while (bits) {
      const int g = pw * 32 + __ffs(bits) - 1;
      bits &= bits - 1u;
      bool sel[4];
#pragma unroll
      for (int e = 0; e < 4; e++) sel[e] = grp[e] == g;
#pragma unroll
      for (int w = 0; w < EM_SUMS; w++) {
        double q[4];
#pragma unroll
        for (int e = 0; e < 4; e++) {
          const float x = w == 0 ? 1.0f : f[e][w == 0 ? 0 : w - 1];
          q[e] = sel[e] ? (double)x : 0.0;
        }
        sh[w][t] = (q[0] + q[2]) + (q[1] + q[3]);
      }
      float mn = INFINITY, mx = -INFINITY;
#pragma unroll
      for (int e = 0; e < 4; e++)
        if (sel[e]) { mn = f[e][4] < mn ? f[e][4] : mn; mx = f[e][4] > mx ? f[e][4] : mx; }
#pragma unroll
      for (int s = 32; s >= 1; s >>= 1) {
        const float om = __shfl_down(mn, s, 64), ox = __shfl_down(mx, s, 64);
        mn = om < mn ? om : mn;
        mx = ox > mx ? ox : mx;
      }
      if (lane == 0) { shx[wave][0] = mn; shx[wave][1] = mx; }
      __syncthreads();
      tree_group_sums<EM_SUMS>(sh, EM_SUMS, [&](int w, double x) { part[tree_at(SPH_MUSCLE_WORDS, g, kEmSumWord[w], chunks, chunk)] = x; });
      if (t < 2) {
        float x = shx[0][t];
        for (int q = 1; q < 4; q++) { const float o = shx[q][t]; x = t == 0 ? (o < x ? o : x) : (o > x ? o : x); }
        part[tree_at(SPH_MUSCLE_WORDS, g, 7 + t, chunks, chunk)] = (double)x;
      }
      __syncthreads();  // sh / shx are reused by the next group
    }
  }
}

// The records: the signal, canonical extremes (+ 0.0f), the empty-group rule; the error flags ride behind the last record.
__global__ void k_muscle_final(SphDev d, const double* __restrict__ top /* one chunk per word */, const uint32_t* __restrict__ bad,
                               double* __restrict__ out) {
  const int g = blockIdx.x, w = threadIdx.x;  // SPH_MUSCLE_WORDS threads
  const double n = top[tree_at(SPH_MUSCLE_WORDS, g, 0, 1, 0)];
  double x = 0.0;
  if (w == 1) x = g > 0 ? (double)d.muscle[g - 1] : 0.0;
  else if (w == 7 || w == 8) { if (n > 0.0) x = (double)((float)top[tree_at(SPH_MUSCLE_WORDS, g, w, 1, 0)] + 0.0f); }
  else if (w != 15) x = top[tree_at(SPH_MUSCLE_WORDS, g, w, 1, 0)];
  out[(size_t)g * SPH_MUSCLE_WORDS + w] = x;
  if (g == 0 && w == 0) out[(size_t)gridDim.x * SPH_MUSCLE_WORDS] = (double)*bad;
}

// doubles of the scratch of a call: the levels, the records with the copy of the error flags behind them, the flags' own cell
size_t sphk_group_tree_doubles(long long terms, int groups) { return tree_scratch_doubles(terms, groups, SPH_MUSCLE_WORDS) + 2; }

// levels above `cur` (chunks partials per group and word) until one chunk is left: the sums of kEmSumWord, the minimum in word 7
// and the maximum in word 8; *top: where that level lies, *end: behind it
static int em_upper_levels(sph_solver* s, int groups, double* cur, int chunks, double** top, double** end) {
  TreeShape S = tree_shape(SPH_MUSCLE_WORDS, 0);
  for (int w = 0; w < 15; w++)
    if (w != 1) tree_shape_add(S, w, w == 7 ? DIAG_OP_MIN : w == 8 ? DIAG_OP_MAX : DIAG_OP_SUM);
  return sphk_tree_upper(s, S, groups, cur, chunks, top, end);
}

int sphk_muscle_diagnostics(sph_solver* s, double* scratch, double** records) {
  const int groups = s->d.muscleCount + 1;
  const long long terms = (long long)s->d.numElastic * SPH_MAXN;
  const int chunks = tree_chunks(terms);
  uint32_t* bad = (uint32_t*)(scratch + sphk_group_tree_doubles(terms, groups) - 1);
  SPH_HIP(hipMemsetAsync(bad, 0, sizeof(double), s->stream));
  const size_t total = (size_t)groups * SPH_MUSCLE_WORDS * (size_t)chunks;
  hipLaunchKernelGGL(k_muscle_fill, dim3((unsigned)((total + SPH_BLOCK - 1) / SPH_BLOCK)), dim3(SPH_BLOCK), 0, s->stream, scratch, chunks, total);
  hipLaunchKernelGGL(k_muscle_leaf, dim3(chunks), dim3(SPH_BLOCK), 0, s->stream, s->d, scratch, chunks, bad);
  SPH_HIP(hipGetLastError());
  double *top = nullptr, *out = nullptr;
  const int rc = em_upper_levels(s, groups, scratch, chunks, &top, &out);
  if (rc != SPH_OK) return rc;
  hipLaunchKernelGGL(k_muscle_final, dim3(groups), dim3(SPH_MUSCLE_WORDS), 0, s->stream, s->d, (const double*)top, (const uint32_t*)bad, out);
  SPH_HIP(hipGetLastError());
  *records = out;  // groups x SPH_MUSCLE_WORDS doubles, then the error flags as one double
  return SPH_OK;
}

// ---- membranes ----------------------------------------------------------------------------------------------------------------
// One lane per triangle, one block per chunk of 1024 triangles: the records, and the chunk's partial of the area tree as
// "group 0" of the table above (word 0 the count, 2 the area sum, 7 and 8 the extremes), so that the upper levels are shared.
__global__ __launch_bounds__(SPH_BLOCK) void k_membrane_measure(SphDev d, float4* __restrict__ out, double* __restrict__ part, int chunks,
                                                                uint32_t* __restrict__ bad) {
  __shared__ double sh[2][SPH_BLOCK];
  __shared__ float shx[4][2];
  const int t = threadIdx.x, chunk = blockIdx.x, lane = t & 63, wave = t >> 6;
  double q[4], c[4];
  float mn = INFINITY, mx = -INFINITY;
#pragma unroll
  for (int e = 0; e < 4; e++) {
    const int tri = chunk * DIAG_CHUNK + e * SPH_BLOCK + t;
    q[e] = 0.0; c[e] = 0.0;
    if (tri >= d.numMembranes) continue;
    const int ia = d.membraneData[3 * (size_t)tri + 0], ib = d.membraneData[3 * (size_t)tri + 1], ic = d.membraneData[3 * (size_t)tri + 2];
    float4 r0 = make_float4(0.f, 0.f, 0.f, 0.f), r1 = r0;
    bool ok = ia >= 0 && ia < d.N && ib >= 0 && ib < d.N && ic >= 0 && ic < d.N;
    uint32_t ja = 0, jb = 0, jc = 0;
    if (ok) {
      ja = d.backIndex[ia]; jb = d.backIndex[ib]; jc = d.backIndex[ic];
      ok = ja < (uint32_t)d.N && jb < (uint32_t)d.N && jc < (uint32_t)d.N;
    }
    if (!ok) atomicOr(bad, 1u);
    else {
      const float4 a = d.sortedPos[ja], b = d.sortedPos[jb], cc = d.sortedPos[jc];
      const float e1x = b.x - a.x, e1y = b.y - a.y, e1z = b.z - a.z;
      const float e2x = cc.x - a.x, e2y = cc.y - a.y, e2z = cc.z - a.z;
      const float nx = e1y * e2z - e1z * e2y, ny = e1z * e2x - e1x * e2z, nz = e1x * e2y - e1y * e2x;
      const float len = sqrtf((nx * nx + ny * ny) + nz * nz);
      const float area = 0.5f * len;
      const bool flat = len == 0.f;
      r0 = make_float4(area, flat ? 0.f : nx / len, flat ? 0.f : ny / len, flat ? 0.f : nz / len);
      r1 = make_float4(((a.x + b.x) + cc.x) / 3.0f, ((a.y + b.y) + cc.y) / 3.0f, ((a.z + b.z) + cc.z) / 3.0f, 0.f);
      q[e] = (double)area; c[e] = 1.0;
      mn = area < mn ? area : mn;
      mx = area > mx ? area : mx;
    }
    if (out) { out[2 * (size_t)tri] = r0; out[2 * (size_t)tri + 1] = r1; }
  }
  sh[0][t] = (c[0] + c[2]) + (c[1] + c[3]);
  sh[1][t] = (q[0] + q[2]) + (q[1] + q[3]);
#pragma unroll
  for (int s = 32; s >= 1; s >>= 1) {
    const float om = __shfl_down(mn, s, 64), ox = __shfl_down(mx, s, 64);
    mn = om < mn ? om : mn;
    mx = ox > mx ? ox : mx;
  }
  if (lane == 0) { shx[wave][0] = mn; shx[wave][1] = mx; }
  __syncthreads();
  tree_group_sums<2>(sh, 2, [&](int k, double x) { part[tree_at(SPH_MUSCLE_WORDS, 0, k == 0 ? 0 : 2, chunks, chunk)] = x; });  // waves 0, 1
  if (wave == 2 && lane < 2) {
    float x = shx[0][lane];
    for (int k = 1; k < 4; k++) { const float o = shx[k][lane]; x = lane == 0 ? (o < x ? o : x) : (o > x ? o : x); }
    part[tree_at(SPH_MUSCLE_WORDS, 0, 7 + lane, chunks, chunk)] = (double)x;
  } else if (wave == 3 && lane < SPH_MUSCLE_WORDS && lane != 0 && lane != 2 && lane != 7 && lane != 8) {
    part[tree_at(SPH_MUSCLE_WORDS, 0, lane, chunks, chunk)] = 0.0;  // the sum words the shared upper level reads and this table does not use
  }
}

// *top: 16 doubles (word 0 count, 2 area sum, 7 min, 8 max), directly followed by one 8-byte cell whose low word holds the error
// flags, so that one copy brings both to the host
int sphk_membrane_measure(sph_solver* s, float* out, double* scratch, double** top) {
  const int chunks = tree_chunks(s->d.numMembranes);
  uint32_t* bad = (uint32_t*)(scratch + tree_level_chunks(s->d.numMembranes) * SPH_MUSCLE_WORDS);  // behind the levels of one group
  SPH_HIP(hipMemsetAsync(bad, 0, sizeof(double), s->stream));
  hipLaunchKernelGGL(k_membrane_measure, dim3(chunks), dim3(SPH_BLOCK), 0, s->stream, s->d, (float4*)out, scratch, chunks, bad);
  SPH_HIP(hipGetLastError());
  double* end = nullptr;
  return em_upper_levels(s, 1, scratch, chunks, top, &end);  // (end == the flags' cell)
}

// Flow gauges (include/sphmi.h: sph_gauge_define / sph_gauges_accumulate / sph_gauge_crossings): after a completed
// step, which particles went through an oriented parallelogram or plane, and the sums of what they carried. A crossing is a sign
// change of s(p) between sortedPos[i], where sorted particle i was when the step began, and posOrig[vals[i]], where the step left
// it. Read-only on every solver array; the step's kernels are not touched.
//   k_gauge_leaf    one block per chunk of 1024 sorted particles in the element layout of the diagnostics leaf (thread t holds
//                   elements t, t + 256, t + 512, t + 768). Per element it streams sortedPos and vals and gathers posOrig[id]; the
//                   gauges come by value, so their doubles are scalar loads. The side tests of all defined gauges give a 32-bit
//                   word per element, 2 bits per gauge (positive, negative); a lane that crosses a parallelogram's plane computes
//                   (alpha, beta) at once and drops the bits of a crossing outside it. The block or-s a presence mask through one
//                   LDS word and reduces, in the fixed tree of sph_tree.h from registers through LDS, only the (gauge, direction)
//                   pairs present: velocity and field are gathered, and t, alpha, beta computed again, only by the lanes that
//                   contribute to the pair. An absent pair gets +0.0 partials, which is what the tree makes of +0.0 terms.
//   (sph_tree.hip)  the upper levels of the tree, the rows of the defined gauges only
//   k_gauge_final   one thread per (gauge, word): the record, total = total + record, the call words 16..19, the history row
//   k_gauge_clear   the totals of the slots in a mask
//   k_gauge_mark    the crossing list of one gauge: the ballot of each wave and the count of each block, in the layout of the
//                   selection's scan (sphk_select_scan / sphk_select_scatter then list the sorted indices in ascending order)
//   k_gauge_list    original id, direction and (t, alpha, beta) of the listed particles
// All arithmetic on positions in double, one operation at a time in the contract's order (no contraction: the Makefile's flags).
// Integer atomics only where the result cannot depend on the order (or). No floating-point atomics.
#include "sph_common.h"
#include "sph_tree.h"

#include <algorithm>

#define GA_WORDS SPH_GAUGE_WORDS
#define GA_HALF (SPH_GAUGE_WORDS / 2)  // the terms of one direction: reduced together through LDS
#define GA_WAVES (SPH_BLOCK / 64)

// (the rows of the tree are the gauges, GA_WORDS words each)

__device__ __forceinline__ double ga_side(const GaugeOne& G, double px, double py, double pz) {
  return (G.n[0] * (px - G.o[0]) + G.n[1] * (py - G.o[1])) + G.n[2] * (pz - G.o[2]);
}

// 0: the particle is not considered or stays on its side (a NaN crosses nothing); 1: a positive crossing; 2: a negative one
__device__ __forceinline__ uint32_t ga_cross(const GaugeOne& G, const float4& a, const float4& b) {
  const int type = (int)a.w;
  if (!(type >= 1 && type <= 2 && ((G.typeMask >> type) & 1u))) return 0u;
  const double sa = ga_side(G, (double)a.x, (double)a.y, (double)a.z);
  const double sb = ga_side(G, (double)b.x, (double)b.y, (double)b.z);
  if (sa < 0.0 && sb >= 0.0) return 1u;
  if (sa >= 0.0 && sb < 0.0) return 2u;
  return 0u;
}

// for a crossing: where it meets the plane; true if it is counted
__device__ __forceinline__ bool ga_hit(const GaugeOne& G, const float4& a, const float4& b, double& t, double& alpha, double& beta) {
  const double ax = (double)a.x, ay = (double)a.y, az = (double)a.z;
  const double bx = (double)b.x, by = (double)b.y, bz = (double)b.z;
  const double sa = ga_side(G, ax, ay, az), sb = ga_side(G, bx, by, bz);
  t = sa / (sa - sb);
  const double xx = ax + t * (bx - ax), xy = ay + t * (by - ay), xz = az + t * (bz - az);
  alpha = (G.A[0] * (xx - G.o[0]) + G.A[1] * (xy - G.o[1])) + G.A[2] * (xz - G.o[2]);
  beta = (G.B[0] * (xx - G.o[0]) + G.B[1] * (xy - G.o[1])) + G.B[2] * (xz - G.o[2]);
  return G.plane != 0u || (0.0 <= alpha && alpha < 1.0 && 0.0 <= beta && beta < 1.0);
}

__global__ __launch_bounds__(SPH_BLOCK) void k_gauge_leaf(SphDev d, GaugeSet set, double* __restrict__ part, int chunks) {
  __shared__ double sh[GA_HALF][SPH_BLOCK];
  __shared__ uint32_t shPres;
  const int t = threadIdx.x, chunk = blockIdx.x;
  float4 a[4], b[4];
  uint32_t id[4], word[4];
#pragma unroll
  for (int e = 0; e < 4; e++) {
    const int j = chunk * DIAG_CHUNK + e * SPH_BLOCK + t;
    a[e] = make_float4(0.f, 0.f, 0.f, 0.f); b[e] = a[e];  // type 0: considered by no gauge
    id[e] = 0u; word[e] = 0u;
    if (j < d.N) {
      const uint32_t o = d.vals[j];
      if (o < (uint32_t)d.N) {  // (always: vals is a permutation; an id outside 0..N-1 is never followed)
        a[e] = d.sortedPos[j];
        b[e] = d.posOrig[o];
        id[e] = o;
      }
    }
  }
  // the side tests: wave-uniform over the gauges, whose doubles are scalar operands
#pragma unroll 1
  for (int g = 0; g < SPH_MAX_GAUGES; g++) {
    if (!((set.defMask >> g) & 1u)) continue;
    const GaugeOne& G = set.g[g];
#pragma unroll
    for (int e = 0; e < 4; e++) {
      uint32_t c = ga_cross(G, a[e], b[e]);
      if (c && !G.plane) {
        double tt, al, be;
        if (!ga_hit(G, a[e], b[e], tt, al, be)) c = 0u;
      }
      word[e] |= c << (2 * g);
    }
  }
  const uint32_t mine = (word[0] | word[1]) | (word[2] | word[3]);
  if (t == 0) shPres = 0u;
  __syncthreads();
  if (mine) atomicOr(&shPres, mine);
  __syncthreads();
  const uint32_t blockPres = shPres;
#pragma unroll 1
  for (int g = 0; g < SPH_MAX_GAUGES; g++) {
    if (!((set.defMask >> g) & 1u)) continue;
    const GaugeOne& G = set.g[g];
#pragma unroll 1
    for (int dir = 0; dir < 2; dir++) {
      const int bit = 2 * g + dir;
      if (!((blockPres >> bit) & 1u)) {  // every term of this chunk is +0.0: so is every sum of the tree
        if (t < GA_HALF) part[tree_at(GA_WORDS, g, dir * GA_HALF + t, chunks, chunk)] = 0.0;
        continue;
      }
      double acc[GA_HALF], prev[GA_HALF];
#pragma unroll
      for (int k = 0; k < GA_HALF; k++) { acc[k] = 0.0; prev[k] = 0.0; }
      // elements in the order 0, 2, 1, 3: the tree's (q0 + q2) + (q1 + q3)
#pragma unroll
      for (int i = 0; i < 4; i++) {
        const int e = (i & 1) * 2 + (i >> 1);
        double q[GA_HALF];
#pragma unroll
        for (int k = 0; k < GA_HALF; k++) q[k] = 0.0;
        if ((word[e] >> bit) & 1u) {
          const float4 w = d.velOrig[id[e]];
          const double wx = (double)w.x, wy = (double)w.y, wz = (double)w.z;
          double tt, al, be;
          ga_hit(G, a[e], b[e], tt, al, be);
          q[0] = 1.0; q[1] = wx; q[2] = wy; q[3] = wz;
          q[4] = (wx * wx + wy * wy) + wz * wz;
          q[5] = G.field ? (double)G.field[id[e]] : 0.0;
          q[6] = al; q[7] = be;
        }
        if (i & 1) {
#pragma unroll
          for (int k = 0; k < GA_HALF; k++) {
            const double pair = prev[k] + q[k];
            acc[k] = i == 1 ? pair : acc[k] + pair;
          }
        } else {
#pragma unroll
          for (int k = 0; k < GA_HALF; k++) prev[k] = q[k];
        }
      }
#pragma unroll
      for (int k = 0; k < GA_HALF; k++) sh[k][t] = acc[k];
      __syncthreads();
      tree_group_sums<GA_HALF>(sh, GA_HALF, [&](int k, double x) { part[tree_at(GA_WORDS, g, dir * GA_HALF + k, chunks, chunk)] = x; });
      __syncthreads();  // sh is reused by the next pair
    }
  }
}

// top: the tree's last level, one partial per gauge and word. One thread per (gauge, word).
__global__ __launch_bounds__(SPH_MAX_GAUGES * GA_WORDS) void k_gauge_final(const double* __restrict__ top, uint32_t defMask,
                                                                           GaugeDev* __restrict__ D, double* __restrict__ hist,
                                                                           int rows, long long call) {
  const int g = threadIdx.x / GA_WORDS, w = threadIdx.x % GA_WORDS;
  const bool defined = ((defMask >> g) & 1u) != 0u;
  const double rec = defined ? top[tree_at(GA_WORDS, g, w, 1, 0)] : 0.0;
  D->record[g][w] = rec;
  if (hist) hist[(size_t)(call % rows) * (SPH_MAX_GAUGES * GA_WORDS) + threadIdx.x] = rec;
  if (!defined) return;
  double* T = D->totals[g];
  T[w] = T[w] + rec;
  if (w == 0) {  // (this thread alone touches words 16..19 of the gauge)
    const double plus = rec, minus = top[tree_at(GA_WORDS, g, GA_HALF, 1, 0)];
    T[16] = T[16] + 1.0;
    if (plus > 0.0 && T[17] < 0.0) T[17] = (double)call;
    if (minus > 0.0 && T[18] < 0.0) T[18] = (double)call;
    if (plus > 0.0 || minus > 0.0) T[19] = (double)call;
  }
}

__global__ __launch_bounds__(SPH_MAX_GAUGES * 32) void k_gauge_clear(GaugeDev* __restrict__ D, uint32_t slots) {
  const int g = threadIdx.x / 32, w = threadIdx.x % 32;
  if (w >= SPH_GAUGE_TOTAL_WORDS || !((slots >> g) & 1u)) return;
  D->totals[g][w] = w <= 16 ? 0.0 : -1.0;
}

// ---- the crossing list of one gauge --------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t ga_counted(const SphDev& d, const GaugeOne& G, int j, uint32_t& o, double& t, double& alpha,
                                               double& beta) {
  o = d.vals[j];
  if (o >= (uint32_t)d.N) return 0u;
  const float4 a = d.sortedPos[j], b = d.posOrig[o];
  const uint32_t c = ga_cross(G, a, b);
  if (!c) return 0u;
  return ga_hit(G, a, b, t, alpha, beta) ? c : 0u;
}

__global__ __launch_bounds__(SPH_BLOCK) void k_gauge_mark(SphDev d, GaugeOne G, unsigned long long* __restrict__ mask,
                                                          uint32_t* __restrict__ blockCnt) {
  __shared__ uint32_t cnt[GA_WAVES];
  const int t = threadIdx.x, j = blockIdx.x * SPH_BLOCK + t, lane = t & 63, wave = t >> 6;
  bool hit = false;
  if (j < d.N) {
    uint32_t o;
    double tt, al, be;
    hit = ga_counted(d, G, j, o, tt, al, be) != 0u;
  }
  const unsigned long long ballot = __ballot(hit);
  if (lane == 0) {
    mask[(size_t)blockIdx.x * GA_WAVES + wave] = ballot;
    cnt[wave] = (uint32_t)__popcll(ballot);
  }
  __syncthreads();
  if (t == 0) blockCnt[blockIdx.x] = (cnt[0] + cnt[1]) + (cnt[2] + cnt[3]);
}

__global__ __launch_bounds__(SPH_BLOCK) void k_gauge_list(SphDev d, GaugeOne G, const int32_t* __restrict__ list, int n,
                                                          uint32_t* __restrict__ origId, int32_t* __restrict__ direction,
                                                          float* __restrict__ tab3) {
  const int r = blockIdx.x * SPH_BLOCK + threadIdx.x;
  if (r >= n) return;
  const int j = list[r];
  uint32_t o = 0u, c = 0u;
  double tt = 0.0, al = 0.0, be = 0.0;
  if (j >= 0 && j < d.N) c = ga_counted(d, G, j, o, tt, al, be);  // (always counted: the list is the mark's)
  origId[r] = o;
  direction[r] = c == 1u ? 1 : c == 2u ? -1 : 0;
  tab3[3 * (size_t)r] = (float)tt; tab3[3 * (size_t)r + 1] = (float)al; tab3[3 * (size_t)r + 2] = (float)be;
}

// ---- launchers ---------------------------------------------------------------------------------------------------------------
static_assert(GA_WAVES == 4, "k_gauge_mark writes the four ballots per block that k_select_scatter reads");

size_t sphk_gauge_tree_bytes(int N) { return sizeof(double) * tree_level_chunks(N) * SPH_MAX_GAUGES * GA_WORDS; }

int sphk_gauge_clear(sph_solver* s, GaugeDev* D, uint32_t slots) {
  hipLaunchKernelGGL(k_gauge_clear, dim3(1), dim3(SPH_MAX_GAUGES * 32), 0, s->stream, D, slots);
  SPH_HIP(hipGetLastError());
  return SPH_OK;
}

int sphk_gauges_accumulate(sph_solver* s, const GaugeSet& set, double* tree, GaugeDev* D, double* hist, int rows, int64_t call) {
  const int chunks = tree_chunks(s->d.N);
  hipLaunchKernelGGL(k_gauge_leaf, dim3(chunks), dim3(SPH_BLOCK), 0, s->stream, s->d, set, tree, chunks);
  SPH_HIP(hipGetLastError());
  double *top = nullptr, *end = nullptr;  // the rows of undefined gauges are unwritten at every level: masked out, never read
  const int rc = sphk_tree_upper(s, tree_shape(GA_WORDS, GA_WORDS, set.defMask), SPH_MAX_GAUGES, tree, chunks, &top, &end);
  if (rc != SPH_OK) return rc;
  hipLaunchKernelGGL(k_gauge_final, dim3(1), dim3(SPH_MAX_GAUGES * GA_WORDS), 0, s->stream, (const double*)top, set.defMask, D, hist,
                     rows > 0 ? rows : 1, (long long)call);
  SPH_HIP(hipGetLastError());
  return SPH_OK;
}

int sphk_gauge_mark(sph_solver* s, const GaugeOne& g, void* scratch, uint32_t** totals) {
  const SelLayout L = sphk_select_layout(s->d.N);
  char* base = (char*)scratch;
  hipLaunchKernelGGL(k_gauge_mark, dim3(L.nb), dim3(SPH_BLOCK), 0, s->stream, s->d, g, (unsigned long long*)(base + L.mask),
                     (uint32_t*)(base + L.blockCnt));
  SPH_HIP(hipGetLastError());
  *totals = (uint32_t*)(base + L.totals);
  return sphk_select_scan(s, scratch, s->d.N);
}

int sphk_gauge_list(sph_solver* s, const GaugeOne& g, const int32_t* list, int n, uint32_t* origId, int32_t* direction, float* tab3) {
  if (n <= 0) return SPH_OK;
  hipLaunchKernelGGL(k_gauge_list, dim3(sph_blocks(n)), dim3(SPH_BLOCK), 0, s->stream, s->d, g, list, n, origId, direction, tab3);
  SPH_HIP(hipGetLastError());
  return SPH_OK;
}

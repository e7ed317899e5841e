// Flow diagnostics: reductions over the selected particles of up to 16 axis-aligned regions, and histograms of one per-particle
// quantity, read from the sorted state of the last completed step (include/sphmi.h: sph_diagnostics / sph_histogram, DESIGN.md
// §15). Read-only on every solver array. Which particles a region or a histogram selects: sph_selector.h.
//
// The sums are doubles reduced in the FIXED TREE of the contract: the terms in ascending sorted index, padded with +0.0 to whole
// chunks of 1024; in a chunk, a[i] += a[i + stride] for stride = 512 ... 1; the chunks' results are the terms of the next
// level, until one chunk is left. One 256-thread block owns one chunk, so the shape depends on nothing but N:
//   stride 512, 256   thread t holds elements t, t+256, t+512, t+768:  (e0 + e2) + (e1 + e3) in registers
//   stride 128, 64    across the four waves, through LDS (every thread parks its 14 values there: 28 KB per block)
//   stride 32 ... 1   inside one wave, __shfl_down
// No floating-point atomics anywhere. Extremes are order-independent (float compares; the max-v2 particle by the pair
// (larger v2, then lower index)) and travel through the levels as exactly widened doubles.
#include "sph_common.h"
#include "sph_selector.h"  // the selection rule and the histogram's quantity
#include "sph_tree.h"  // the tree's layout (rows: the regions), the leaf's tail and the upper levels
#include "sph_diag_leaf.h"  // the reduction of one chunk for one selection, and a record's words from the top of its tree

#include <algorithm>

// ---- level 0: particles -> one partial per chunk, word and region ---------------------------------------------------------
// Every array is read once, whatever the number of regions: the per-particle terms stay in registers and the region loop only
// selects among them; the reduction of one selection is diag_leaf_reduce (sph_diag_leaf.h).
// COMP: the selection of record r is labels[j] == comp[r] (sph_component_diagnostics) instead of type, key and box; everything
// after the selection is the same code.
template <bool COMP>
__global__ __launch_bounds__(SPH_BLOCK) void k_diag_leaf(SphDev d, DiagArgs a, double* __restrict__ part, int chunks) {
  __shared__ DiagLeafLds L;
  const int t = threadIdx.x, chunk = blockIdx.x;
  float f[4][DIAG_TERMS];
  bool ok[4];
  int lab[4];
#pragma unroll
  for (int e = 0; e < 4; e++) {
    const int j = chunk * DIAG_CHUNK + e * SPH_BLOCK + t;
    ok[e] = false;
    lab[e] = -1;
#pragma unroll
    for (int w = 0; w < DIAG_TERMS; w++) f[e][w] = 0.f;
    if (j < d.N) {
      const float4 p = d.sortedPos[j];
      diag_leaf_load(d, a.rho0, j, p, f[e]);
      if (COMP) { lab[e] = a.labels[j]; ok[e] = lab[e] >= 0; }
      else ok[e] = sph_type_key_selected(d, a.typeMask, j, p);
    }
  }
  for (int r = 0; r < a.count; r++) {
    const float x0 = a.box[r][0], y0 = a.box[r][1], z0 = a.box[r][2], x1 = a.box[r][3], y1 = a.box[r][4], z1 = a.box[r][5];
    bool sel[4];
#pragma unroll
    for (int e = 0; e < 4; e++)
      sel[e] = COMP ? (ok[e] && lab[e] == a.comp[r]) : ok[e] && sph_box_holds(x0, y0, z0, x1, y1, z1, f[e][0], f[e][1], f[e][2]);
    // No particle of this chunk in the region (the sorted order is spatial, so that is the common case for a small region): every
    // sum of +0.0 terms is +0.0 and every extreme keeps its identity, which is what the tree below would produce.
    if (!__syncthreads_or(sel[0] || sel[1] || sel[2] || sel[3])) {
      if (t < SPH_DIAG_WORDS) {
        double x = 0.0;
        bool used = t < DIAG_SUMS || t == 20 || t == 21;
        if (t == 20) x = -(double)INFINITY;
        if (t == 21) x = 2147483647.0;
#pragma unroll
        for (int k = 0; k < 5; k++) {
          if (t == kDiagMinWord[k]) { x = (double)INFINITY; used = true; }
          if (t == kDiagMaxWord[k]) { x = -(double)INFINITY; used = true; }
        }
        if (used) part[tree_at(SPH_DIAG_WORDS, r, t, chunks, chunk)] = x;
      }
      continue;
    }
    diag_leaf_reduce(L, f, sel, chunk, [&](int w, double x) { part[tree_at(SPH_DIAG_WORDS, r, w, chunks, chunk)] = x; });
  }
}

// ---- the records: canonical extremes (+ 0.0f), the empty-selection rule, the original id of the fastest particle ------------
__global__ void k_diag_final(SphDev d, const double* __restrict__ top /* one chunk per word */, double* __restrict__ out) {
  const int r = blockIdx.x, w = threadIdx.x;  // SPH_DIAG_WORDS threads
  out[r * SPH_DIAG_WORDS + w] = diag_record_word(d, w, [&](int word) { return top[tree_at(SPH_DIAG_WORDS, r, word, 1, 0)]; });
}

int sphk_diagnostics(sph_solver* s, const DiagArgs& a, double* scratch, double** records) {
  const int R = a.count, chunks = tree_chunks(s->d.N);
  if (a.labels) hipLaunchKernelGGL(k_diag_leaf<true>, dim3(chunks), dim3(SPH_BLOCK), 0, s->stream, s->d, a, scratch, chunks);
  else hipLaunchKernelGGL(k_diag_leaf<false>, dim3(chunks), dim3(SPH_BLOCK), 0, s->stream, s->d, a, scratch, chunks);
  SPH_HIP(hipGetLastError());
  // upper levels: the sums, the minima and the maxima (kDiagMinWord, kDiagMaxWord), the pair (max v2, lowest index) in words 20, 21
  TreeShape S = tree_shape(SPH_DIAG_WORDS, DIAG_SUMS);
  for (int w : {16, 18, 23, 24, 25}) tree_shape_add(S, w, DIAG_OP_MIN);
  for (int w : {17, 19, 26, 27, 28}) tree_shape_add(S, w, DIAG_OP_MAX);
  tree_shape_add(S, 20, DIAG_OP_PAIR);
  double *top = nullptr, *out = nullptr;
  const int rc = sphk_tree_upper(s, S, R, scratch, chunks, &top, &out);
  if (rc != SPH_OK) return rc;
  hipLaunchKernelGGL(k_diag_final, dim3(R), dim3(SPH_DIAG_WORDS), 0, s->stream, s->d, (const double*)top, out);
  SPH_HIP(hipGetLastError());
  *records = out;
  return SPH_OK;
}

// ---- histogram ---------------------------------------------------------------------------------------------------------------
// Counts are integers, so any order gives the same result: a histogram per block in LDS (integer atomics), then one integer
// atomicAdd per non-empty bin and block.
// The neighbour count of field 3 keeps its own decoder of the row (plain loads), not sph_neighbor_count over the shared row walk
// (non-temporal loads): the two have not been timed against each other on an MI355X.
__device__ __forceinline__ float hist_neighbor_count(const SphDev& d, int id) {
  int n = 0;
  const bool wide = d.nbr16[nbr_index(id, 0)] == SPH_N16_WIDE;
  if (wide) {
#pragma unroll
    for (int g = 0; g < 8; g++) {
      const int4 q = *(const int4*)(d.nbrId + nbr_index(id, 4 * g));
      n += (q.x >= 0) + (q.y >= 0) + (q.z >= 0) + (q.w >= 0);
    }
  } else {
    const int base = d.nbrBase[id];
#pragma unroll
    for (int g = 0; g < 8; g++) {
      const uint2 q = *(const uint2*)(d.nbr16 + nbr_index(id, 4 * g));
      const uint32_t e[4] = {q.x & 0xffffu, q.x >> 16, q.y & 0xffffu, q.y >> 16};
#pragma unroll
      for (int k = 0; k < 4; k++)
        if (e[k] != SPH_N16_EMPTY) n += (((e[k] & 0x8000u) ? base : id) + (int)(e[k] & 0x7fffu) - SPH_N16_BIAS) >= 0;
    }
  }
  return (float)n;
}

__global__ __launch_bounds__(SPH_BLOCK) void k_histogram(SphDev d, HistArgs a, uint32_t* __restrict__ out) {
  __shared__ uint32_t hist[SPH_HIST_MAX_BINS + 2];
  const int slots = a.bins + 2;
  for (int b = threadIdx.x; b < slots; b += SPH_BLOCK) hist[b] = 0u;
  __syncthreads();
  for (int j = blockIdx.x * SPH_BLOCK + threadIdx.x; j < d.N; j += gridDim.x * SPH_BLOCK) {
    const float4 p = d.sortedPos[j];
    if (!sph_selected(d, a.sel, j, p)) continue;
    const float q = a.field == 3 ? hist_neighbor_count(d, j) : sph_particle_quantity(d, a.field, j, p);
    int slot;
    if (q < a.lo) slot = 0;
    else if (q >= a.hi) slot = a.bins + 1;
    else {
      const int b = (int)((q - a.lo) * a.scale);
      slot = 1 + (b < a.bins - 1 ? b : a.bins - 1);
      if (slot < 1) slot = 1;  // (a NaN value; the state has blown up)
    }
    atomicAdd(&hist[slot], 1u);
  }
  __syncthreads();
  for (int b = threadIdx.x; b < slots; b += SPH_BLOCK)
    if (hist[b]) atomicAdd(&out[b], hist[b]);
}

int sphk_histogram(sph_solver* s, const HistArgs& a, uint32_t* out) {
  SPH_HIP(hipMemsetAsync(out, 0, sizeof(uint32_t) * (size_t)(a.bins + 2), s->stream));
  if (s->d.N <= 0) return SPH_OK;
  const int blocks = std::min(sph_blocks(s->d.N), 4096);
  hipLaunchKernelGGL(k_histogram, dim3(blocks), dim3(SPH_BLOCK), 0, s->stream, s->d, a, out);
  SPH_HIP(hipGetLastError());
  return SPH_OK;
}

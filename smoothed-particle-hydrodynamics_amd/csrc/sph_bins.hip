// Binned diagnostics: the diagnostics record of every bin of a lattice (include/sphmi.h: sph_bin_diagnostics / sph_bin_index,
// DESIGN.md §50). Read-only on every solver array. The record of bin b is, word for word, what sph_diagnostics returns for the
// bin's box, so the arithmetic is sph_diag.hip's: the leaf is diag_leaf_reduce (sph_diag_leaf.h) with the selection
// "binId[j] == b", and the upper levels are the positional ones of sph_tree.h, done here per bin.
//   k_bin_index   one lane per sorted particle: its bin (-1: in none) by float compares with the lattice's edges; per chunk of
//                 1024 the distinct bins it holds, counted into the bins (integer atomics: a count has no order)
//   k_bin_scan    counts -> where each bin's entries start in the pool; the total sizes the pool
//   k_bin_leaf    one block per chunk, every array read once: for each distinct bin of the chunk, ascending, the leaf writes an
//                 entry (chunk, 26 partials) into the bin's part of the pool
//   k_bin_upper   one block per bin: partial of chunk c is term c of level 1 (group c / 1024, slot c % 1024), every other slot
//                 +0.0, exactly what k_diag_leaf leaves for a chunk without a member; a[i] += a[i + stride] over the 1024 slots
//                 in LDS, a level 2 over the groups for more than 1024 chunks; then the record (diag_record_word)
// The order in which a bin's entries land in the pool is not fixed (an integer atomic hands out the places); nothing depends on
// it, because an entry carries its chunk and the sums are placed by it, and extremes do not depend on order.
// No floating-point atomics anywhere.
#include "sph_common.h"
#include "sph_selector.h"
#include "sph_tree.h"
#include "sph_diag_leaf.h"

#define BIN_POOL_WORDS 26  // per entry: the 14 sums, the 10 extremes, the pair
#define BIN_NONE 0x7fffffff

// record word -> row of the pool: 0..13 | 16..21 -> 14..19 | 23..28 -> 20..25
__device__ __forceinline__ int bin_pool_row(int w) { return w < DIAG_SUMS ? w : (w <= 21 ? w - 2 : w - 3); }

// edge i of an axis: one float multiply, one float add, no contraction (the expression of sph_sample_grid)
__device__ __forceinline__ float bin_edge(float o, float s, int i) { return __fadd_rn(o, __fmul_rn((float)i, s)); }

// The i with e(i) <= x < e(i + 1), i < n, or -1: the largest i in 0..n with e(i) <= x, by bisection on the float edges
// themselves (they never decrease with i), so the result is what sph_box_holds says about the bin's box whatever a division
// would round to; runs of coinciding edges are empty bins. n == 1 with s == 0: the whole axis, -inf <= x < +inf.
__device__ __forceinline__ int bin_axis(float o, float s, int n, float x) {
  if (n == 1 && s == 0.f) return (-INFINITY <= x && x < INFINITY) ? 0 : -1;
  if (!(bin_edge(o, s, 0) <= x)) return -1;  // (a NaN fails here)
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (bin_edge(o, s, mid) <= x) lo = mid; else hi = mid - 1;
  }
  return lo < n ? lo : -1;
}

// f(b) for every distinct b >= 0 among the block's ids (four per thread), ascending; b and the trip count are block-uniform, so
// f may hold barriers. shm: 4 ints of LDS.
template <class F>
__device__ __forceinline__ void bin_for_each_distinct(const int (&id)[4], int* shm, F f) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int last = -1;
  for (;;) {
    int m = BIN_NONE;
#pragma unroll
    for (int e = 0; e < 4; e++) if (id[e] > last && id[e] < m) m = id[e];
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) { const int o = __shfl_xor(m, s, 64); m = o < m ? o : m; }
    if (lane == 0) shm[wave] = m;
    __syncthreads();
    m = min(min(shm[0], shm[1]), min(shm[2], shm[3]));
    __syncthreads();
    if (m == BIN_NONE) return;
    f(m);
    last = m;
  }
}

// binCount == nullptr: the ids only (sph_bin_index)
__global__ __launch_bounds__(SPH_BLOCK) void k_bin_index(SphDev d, BinArgs a, int32_t* __restrict__ binId, uint32_t* __restrict__ binCount) {
  __shared__ int shm[4];
  const int t = threadIdx.x, chunk = blockIdx.x;
  int id[4];
#pragma unroll
  for (int e = 0; e < 4; e++) {
    const int j = chunk * DIAG_CHUNK + e * SPH_BLOCK + t;
    id[e] = -1;
    if (j < d.N) {
      const float4 p = d.sortedPos[j];
      if (sph_type_key_selected(d, a.typeMask, j, p)) {
        const int i = bin_axis(a.o[0], a.s[0], a.n[0], p.x);
        const int jy = bin_axis(a.o[1], a.s[1], a.n[1], p.y);
        const int k = bin_axis(a.o[2], a.s[2], a.n[2], p.z);
        if (i >= 0 && jy >= 0 && k >= 0) id[e] = (k * a.n[1] + jy) * a.n[0] + i;
      }
      binId[j] = id[e];
    }
  }
  if (!binCount) return;
  bin_for_each_distinct(id, shm, [&](int b) { if (t == 0) atomicAdd(&binCount[b], 1u); });
}

// cnt[0 .. B) -> its exclusive prefix sums, cnt[B] = the total; one block, 1024 words per trip
__global__ __launch_bounds__(SPH_BLOCK) void k_bin_scan(uint32_t* __restrict__ cnt, int B) {
  __shared__ uint32_t ws[4];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  uint32_t carry = 0;
  for (int base = 0; base < B; base += 4 * SPH_BLOCK) {
    const int i0 = base + 4 * t;
    uint32_t v[4], sum = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) { v[k] = i0 + k < B ? cnt[i0 + k] : 0u; sum += v[k]; }
    uint32_t x = sum;
#pragma unroll
    for (int s = 1; s < 64; s <<= 1) { const uint32_t y = __shfl_up(x, s, 64); if (lane >= s) x += y; }
    if (lane == 63) ws[wave] = x;
    __syncthreads();
    uint32_t before = carry + x - sum, total = 0;
#pragma unroll
    for (int q = 0; q < 4; q++) { if (q < wave) before += ws[q]; total += ws[q]; }
#pragma unroll
    for (int k = 0; k < 4; k++) { if (i0 + k < B) cnt[i0 + k] = before; before += v[k]; }
    carry += total;
    __syncthreads();
  }
  if (t == 0) cnt[B] = carry;
}

__global__ __launch_bounds__(SPH_BLOCK) void k_bin_leaf(SphDev d, float rho0, const int32_t* __restrict__ binId,
                                                        const uint32_t* __restrict__ binStart, uint32_t* __restrict__ binFill,
                                                        int32_t* __restrict__ entChunk, double* __restrict__ pool, uint32_t total) {
  __shared__ DiagLeafLds L;
  __shared__ int shm[4];
  __shared__ uint32_t place;
  const int t = threadIdx.x, chunk = blockIdx.x;
  float f[4][DIAG_TERMS];
  int id[4];
#pragma unroll
  for (int e = 0; e < 4; e++) {
    const int j = chunk * DIAG_CHUNK + e * SPH_BLOCK + t;
    id[e] = -1;
#pragma unroll
    for (int w = 0; w < DIAG_TERMS; w++) f[e][w] = 0.f;
    if (j < d.N) {
      diag_leaf_load(d, rho0, j, d.sortedPos[j], f[e]);
      id[e] = binId[j];
    }
  }
  bin_for_each_distinct(id, shm, [&](int b) {
    if (t == 0) place = binStart[b] + atomicAdd(&binFill[b], 1u);  // (k_bin_index counted this entry: place < binStart[b + 1])
    __syncthreads();
    const uint32_t q = place;
    if (q >= total) return;  // (block-uniform; cannot happen while the counts are those of this state)
    if (t == 0) entChunk[q] = chunk;
    const bool sel[4] = {id[0] == b, id[1] == b, id[2] == b, id[3] == b};
    diag_leaf_reduce(L, f, sel, chunk, [&](int w, double x) { pool[(size_t)bin_pool_row(w) * total + q] = x; });
  });
}

// sh[0 .. 1024) -> its tree sum in every thread, in the order of diag_block_reduce; sh is left dirty
__device__ __forceinline__ double bin_slots_sum(double* sh) {
  const int t = threadIdx.x;
  const double e0 = sh[t], e1 = sh[SPH_BLOCK + t], e2 = sh[2 * SPH_BLOCK + t], e3 = sh[3 * SPH_BLOCK + t];
  sh[t] = (e0 + e2) + (e1 + e3);  // (thread t alone reads and writes these four slots)
  __syncthreads();
  for (int s = 128; s >= 1; s >>= 1) {
    if (t < s) sh[t] = sh[t] + sh[t + s];
    __syncthreads();
  }
  const double x = sh[0];
  __syncthreads();
  return x;
}

// The levels above the leaf for one bin, as sphk_tree_upper runs them for a region: none for one chunk, one for up to 1024
// chunks, two beyond (SPH_MAX_PARTICLES: at most 128 groups). The number of levels follows `chunks`, never the bin's population.
__global__ __launch_bounds__(SPH_BLOCK) void k_bin_upper(SphDev d, int chunks, const uint32_t* __restrict__ binStart,
                                                         const int32_t* __restrict__ entChunk, const double* __restrict__ pool,
                                                         uint32_t total, double* __restrict__ out) {
  __shared__ double slots[DIAG_CHUNK];
  __shared__ double level2[DIAG_CHUNK];
  __shared__ double top[SPH_DIAG_WORDS];
  __shared__ double wx[4][12];
  __shared__ uint8_t present[DIAG_CHUNK];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, b = blockIdx.x;
  const uint32_t q0 = binStart[b], q1 = binStart[b + 1];
  if (q0 == q1) {  // (block-uniform) no entry: every sum is a tree of +0.0 terms, which is +0.0, and n = 0 makes the rest the empty record
    if (t < SPH_DIAG_WORDS) out[(size_t)b * SPH_DIAG_WORDS + t] = (t == 21 || t == 22) ? -1.0 : 0.0;
    return;
  }
  const int groups = (chunks + DIAG_CHUNK - 1) / DIAG_CHUNK;  // tree_chunks(chunks)
  if (t < SPH_DIAG_WORDS) top[t] = 0.0;
  if (groups > 1) {
    for (int g = t; g < DIAG_CHUNK; g += SPH_BLOCK) present[g] = 0;
    __syncthreads();
    for (uint32_t q = q0 + t; q < q1; q += SPH_BLOCK) present[entChunk[q] >> 10] = 1;
  }
  __syncthreads();
  // group g of level 1 for word w: the bin's partials at their chunks' slots, +0.0 everywhere else
  auto group_sum = [&](int w, int g) {
    for (int i = t; i < DIAG_CHUNK; i += SPH_BLOCK) slots[i] = 0.0;
    __syncthreads();
    for (uint32_t q = q0 + t; q < q1; q += SPH_BLOCK) {
      const int c = entChunk[q];
      if ((c >> 10) == g) slots[c & (DIAG_CHUNK - 1)] = pool[(size_t)w * total + q];
    }
    __syncthreads();
    return bin_slots_sum(slots);
  };
  for (int w = 0; w < DIAG_SUMS; w++) {
    double x;
    if (chunks == 1) x = q1 > q0 ? pool[(size_t)w * total + q0] : 0.0;  // no upper level: the leaf's partial is the result
    else if (groups == 1) x = group_sum(w, 0);
    else {
      for (int i = t; i < DIAG_CHUNK; i += SPH_BLOCK) level2[i] = 0.0;
      __syncthreads();
      for (int g = 0; g < groups; g++) {
        if (!present[g]) continue;  // (block-uniform) a group of +0.0 terms sums to +0.0
        const double y = group_sum(w, g);
        if (t == 0) level2[g] = y;
      }
      __syncthreads();
      x = bin_slots_sum(level2);
    }
    if (t == 0) top[w] = x;
  }
  // extremes and the pair: order-independent, so straight over the entries
  double mn[5], mx[5], bv = -(double)INFINITY, bi = 2147483647.0;
#pragma unroll
  for (int k = 0; k < 5; k++) { mn[k] = (double)INFINITY; mx[k] = -(double)INFINITY; }
  for (uint32_t q = q0 + t; q < q1; q += SPH_BLOCK) {
#pragma unroll
    for (int k = 0; k < 5; k++) {
      const double a = pool[(size_t)bin_pool_row(kDiagMinWord[k]) * total + q], c = pool[(size_t)bin_pool_row(kDiagMaxWord[k]) * total + q];
      mn[k] = a < mn[k] ? a : mn[k];
      mx[k] = c > mx[k] ? c : mx[k];
    }
    const double ov = pool[(size_t)bin_pool_row(20) * total + q], oi = pool[(size_t)bin_pool_row(21) * total + q];
    if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
  }
#pragma unroll
  for (int s = 32; s >= 1; s >>= 1) {
#pragma unroll
    for (int k = 0; k < 5; k++) {
      const double a = __shfl_down(mn[k], s, 64), c = __shfl_down(mx[k], s, 64);
      mn[k] = a < mn[k] ? a : mn[k];
      mx[k] = c > mx[k] ? c : mx[k];
    }
    const double ov = __shfl_down(bv, s, 64), oi = __shfl_down(bi, s, 64);
    if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
  }
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < 5; k++) { wx[wave][k] = mn[k]; wx[wave][5 + k] = mx[k]; }
    wx[wave][10] = bv; wx[wave][11] = bi;
  }
  __syncthreads();
  if (t < 10) {
    double x = wx[0][t];
    for (int q = 1; q < 4; q++) { const double o = wx[q][t]; x = t < 5 ? (o < x ? o : x) : (o > x ? o : x); }
    top[t < 5 ? kDiagMinWord[t] : kDiagMaxWord[t - 5]] = x;
  } else if (t == 10) {
    double v = wx[0][10], i = wx[0][11];
    for (int q = 1; q < 4; q++) if (wx[q][10] > v || (wx[q][10] == v && wx[q][11] < i)) { v = wx[q][10]; i = wx[q][11]; }
    top[20] = v; top[21] = i;
  }
  __syncthreads();
  if (t < SPH_DIAG_WORDS) out[(size_t)b * SPH_DIAG_WORDS + t] = diag_record_word(d, t, [&](int w) { return top[w]; });
}

// ---- the scratch: [records: 32 B doubles][binStart: B + 1 words][binFill: B words][binId: N words] ---------------------------
size_t sphk_bin_scratch_bytes(int N, int B) {
  return sizeof(double) * SPH_DIAG_WORDS * (size_t)B + sizeof(uint32_t) * (2 * (size_t)B + 1) + sizeof(int32_t) * (size_t)N;
}
size_t sphk_bin_pool_bytes(uint32_t entries) { return (sizeof(double) * BIN_POOL_WORDS + sizeof(int32_t)) * (size_t)entries; }
static uint32_t* bin_start(void* scratch, int B) { return (uint32_t*)((double*)scratch + (size_t)SPH_DIAG_WORDS * B); }
int32_t* sphk_bin_ids(void* scratch, int B) { return (int32_t*)(bin_start(scratch, B) + 2 * (size_t)B + 1); }

int sphk_bin_index(sph_solver* s, const BinArgs& a, int B, void* scratch, bool count, uint32_t** total) {
  uint32_t* start = bin_start(scratch, B);
  if (count) SPH_HIP(hipMemsetAsync(start, 0, sizeof(uint32_t) * (2 * (size_t)B + 1), s->stream));
  hipLaunchKernelGGL(k_bin_index, dim3(tree_chunks(s->d.N)), dim3(SPH_BLOCK), 0, s->stream, s->d, a, sphk_bin_ids(scratch, B),
                     count ? start : nullptr);
  SPH_HIP(hipGetLastError());
  if (!count) return SPH_OK;
  hipLaunchKernelGGL(k_bin_scan, dim3(1), dim3(SPH_BLOCK), 0, s->stream, start, B);
  SPH_HIP(hipGetLastError());
  *total = start + B;
  return SPH_OK;
}

int sphk_bin_records(sph_solver* s, const BinArgs& a, int B, void* scratch, void* pool, uint32_t entries, double** records) {
  const int chunks = tree_chunks(s->d.N);
  uint32_t* start = bin_start(scratch, B);
  double* part = (double*)pool;
  int32_t* entChunk = (int32_t*)(part + (size_t)BIN_POOL_WORDS * entries);
  if (entries) {
    hipLaunchKernelGGL(k_bin_leaf, dim3(chunks), dim3(SPH_BLOCK), 0, s->stream, s->d, a.rho0, (const int32_t*)sphk_bin_ids(scratch, B),
                       (const uint32_t*)start, start + B + 1, entChunk, part, entries);
    SPH_HIP(hipGetLastError());
  }
  hipLaunchKernelGGL(k_bin_upper, dim3(B), dim3(SPH_BLOCK), 0, s->stream, s->d, chunks, (const uint32_t*)start, (const int32_t*)entChunk,
                     (const double*)part, entries, (double*)scratch);
  SPH_HIP(hipGetLastError());
  *records = (double*)scratch;
  return SPH_OK;
}

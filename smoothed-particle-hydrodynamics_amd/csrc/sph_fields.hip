// Carried particle fields: a user's scalar per particle that travels with the particles (include/sphmi.h: sph_field_*, DESIGN.md
// §25). A slot's values lie in ORIGINAL-id order, so no kernel of the step knows them; the kernels here paint them, diffuse them
// along the neighbour rows of the last completed step and reduce them. Read-only on every solver array.
//   k_field_pack      sorted particle j -> the record (c, rho) as one float2: c gathered through vals, the stores coalesced. Whether
//                     j PARTICIPATES (type bit in typeMask, valid cell key) is decided here once and kept in the record's SIGN BIT
//                     of rho: set = does not participate. The step's density is max(sum, hs^6) times a positive constant, so a
//                     participant's own sign bit is clear and nothing is lost. A slot whose neighbour does not participate is
//                     masked out of the sums like an empty one: the sums are left untouched, as the contract says.
//   k_field_diffuse   one lane per sorted particle, the shape of k_forces' viscous term: the row through FmRow (16-bit ids, the
//                     32-bit row where that could not be written, the stored distances; non-temporal), ONE 8-byte gather per
//                     neighbour in batches of FD_BATCH with every gather of a batch in flight, masked branch-free accumulation
//                     in slot order. Jacobi: a substep reads the records of one buffer and writes those of the other; the last
//                     one scatters through vals into the slot instead. The first pass also reduces the stability number.
//   k_field_paint_*   the marking rule of sph_remove_region / the entries of the live selection
//   k_field_compact   out[map[o]] = in[o] with the old-to-new map a removal leaves; k_field_fill for the ids an adding call creates
//   k_field_leaf      level 0 of the fixed tree of sph_tree.h for the region records; the upper levels are diag_block_reduce
// The stability number is a maximum of non-negative floats, whose order is the order of their bit patterns: one integer
// atomicMax per wave. No floating-point atomics anywhere. The contract is the IEEE result in the written order (no contraction:
// the Makefile's flags).
#include "sph_common.h"
#include "sph_row_batch.h"
#include "sph_selector.h"
#include "sph_tree.h"

#define FD_BATCH 8
#define FIELD_SUMS 6  // record words 0..5: n, sum c, sum c*c, min, max, tagged

enum { FD_MEASURE = 0, FD_RECORDS = 1, FD_SCATTER = 2 };

__global__ __launch_bounds__(SPH_BLOCK) void k_field_pack(SphDev d, uint32_t typeMask, const float* __restrict__ field,
                                                          float2* __restrict__ rec) {
  const int j = blockIdx.x * SPH_BLOCK + threadIdx.x;
  if (j >= d.N) return;
  const uint32_t o = d.vals[j];
  const float c = o < (uint32_t)d.N ? field[o] : 0.f;  // (vals is a permutation of 0..N-1: the guard keeps a corrupted one inside the slot)
  const float4 p = d.sortedPos[j];
  const uint32_t bits = __float_as_uint(d.rho[j]);
  rec[j] = make_float2(c, __uint_as_float(sph_type_key_selected(d, typeMask, j, p) ? bits : (bits | 0x80000000u)));
}

// OUT == FD_MEASURE: nothing is written but *sigma; FD_RECORDS: out[i] = (c', rho) for every i; FD_SCATTER: field[vals[i]] = c' for
// the participants (the others keep their value where it lies). SIGMA: this pass reduces the stability number too.
template <int OUT, bool SIGMA>
__global__ __launch_bounds__(SPH_BLOCK) void k_field_diffuse(SphDev d, float coefficient, const float2* __restrict__ in,
                                                             float2* __restrict__ out, float* __restrict__ field,
                                                             uint32_t* __restrict__ sigma) {
  const int i = blockIdx.x * SPH_BLOCK + threadIdx.x;
  float stab = 0.f;
  if (i < d.N) {
    const float2 me = in[i];
    const bool mine = !(__float_as_uint(me.y) >> 31);
    if (mine) {
      const float ci = me.x;
      const FmRow t(d, i);
      float S = 0.f, W = 0.f;
      bool wideRow = false;
#pragma unroll 1  // a real loop, as in k_forces: unrolled, the loads of all four batches are hoisted
      for (int b = 0; b < 32 / FD_BATCH; b++) {
        int jj[FD_BATCH];
        float rr[FD_BATCH];
#pragma unroll
        for (int q = 0; q < FD_BATCH / 4; q++) {
          const float4 rq = t.dist4(b * (FD_BATCH / 4) + q);
          rr[4 * q] = rq.x; rr[4 * q + 1] = rq.y; rr[4 * q + 2] = rq.z; rr[4 * q + 3] = rq.w;
        }
#pragma unroll
        for (int q = 0; q < FD_BATCH / 4; q++) {
          const uint2 v = t.vec16(b * (FD_BATCH / 4) + q);
          if (b == 0 && q == 0) wideRow = (v.x & 0xffffu) == SPH_N16_WIDE;
#pragma unroll
          for (int k = 0; k < 4; k++) jj[4 * q + k] = t.decode(v, k);
        }
        if (wideRow) {  // rare
#pragma unroll
          for (int k = 0; k < FD_BATCH; k++) jj[k] = t.id_wide(b * FD_BATCH + k);
        }
        float2 nb[FD_BATCH];
#pragma unroll
        for (int k = 0; k < FD_BATCH; k++) nb[k] = in[min(max(jj[k], 0), d.N - 1)];  // always a valid index; an empty slot is masked out below
#pragma unroll
        for (int k = 0; k < FD_BATCH; k++) {
          const bool used = jj[k] != -1 && rr[k] < d.hs && !(__float_as_uint(nb[k].y) >> 31);
          const float w = d.hs - rr[k];
          const float ts = ((nb[k].x - ci) * w) / nb[k].y;
          const float tw = w / nb[k].y;
          S = used ? S + ts : S;
          W = used ? W + tw : W;
        }
      }
      const float sD = d.mass * (float)(d.del2W / (double)me.y);
      const float a = coefficient * sD;
      if (SIGMA) stab = a * W;
      const float cn = ci + a * S;
      if (OUT == FD_RECORDS) out[i] = make_float2(cn, me.y);
      if (OUT == FD_SCATTER) {
        const uint32_t o = d.vals[i];
        if (o < (uint32_t)d.N) field[o] = cn;
      }
    } else if (OUT == FD_RECORDS) {
      out[i] = me;
    }
  }
  if (SIGMA) {
    // max with float compares from +0: a value counts only when it is > 0 (a NaN never does), and among those the float order is
    // the order of the bit patterns
    uint32_t m = stab > 0.f ? __float_as_uint(stab) : 0u;
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) m = max(m, (uint32_t)__shfl_down(m, s, 64));
    if ((threadIdx.x & 63) == 0 && m) atomicMax(sigma, m);
  }
}

size_t sphk_field_scratch_bytes(int N) { return 2 * sizeof(float2) * (size_t)(N > 0 ? N : 1) + 256; }

template <int OUT, bool SIGMA>
static void fd_launch(sph_solver* s, float coefficient, const float2* in, float2* out, float* field, uint32_t* sigma) {
  hipLaunchKernelGGL((k_field_diffuse<OUT, SIGMA>), dim3(sph_blocks(s->d.N)), dim3(SPH_BLOCK), 0, s->stream, s->d, coefficient, in, out,
                     field, sigma);
}

int sphk_field_diffuse(sph_solver* s, float* field, float coefficient, int substeps, uint32_t typeMask, void* scratch, uint32_t** sigma) {
  const int N = s->d.N;
  float2* rec[2] = {(float2*)scratch, (float2*)scratch + (size_t)(N > 0 ? N : 1)};
  uint32_t* sg = (uint32_t*)(rec[1] + (size_t)(N > 0 ? N : 1));
  *sigma = sg;
  SPH_HIP(hipMemsetAsync(sg, 0, sizeof(uint32_t), s->stream));
  if (N <= 0) return SPH_OK;
  hipLaunchKernelGGL(k_field_pack, dim3(sph_blocks(N)), dim3(SPH_BLOCK), 0, s->stream, s->d, typeMask, (const float*)field, rec[0]);
  SPH_HIP(hipGetLastError());
  if (substeps == 0) fd_launch<FD_MEASURE, true>(s, coefficient, rec[0], rec[1], field, sg);
  for (int k = 0; k < substeps; k++) {  // no host wait in between: the caller waits once, for the stability word
    const float2* in = rec[k & 1];
    float2* out = rec[(k + 1) & 1];
    const bool last = k == substeps - 1;
    if (k == 0) {
      if (last) fd_launch<FD_SCATTER, true>(s, coefficient, in, out, field, sg);
      else fd_launch<FD_RECORDS, true>(s, coefficient, in, out, field, sg);
    } else {
      if (last) fd_launch<FD_SCATTER, false>(s, coefficient, in, out, field, sg);
      else fd_launch<FD_RECORDS, false>(s, coefficient, in, out, field, sg);
    }
  }
  SPH_HIP(hipGetLastError());
  return SPH_OK;
}

// ---- painting -------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(SPH_BLOCK) void k_field_paint_region(const float4* __restrict__ pos, int N, SphSelector a,
                                                                  float* __restrict__ field, float value, uint32_t* __restrict__ count) {
  const int o = blockIdx.x * SPH_BLOCK + threadIdx.x;
  bool hit = false;
  if (o < N) {
    const float4 p = pos[o];
    hit = sph_type_selected(p.w, a.typeMask) && sph_box_holds(a.box, p.x, p.y, p.z);  // k_edit_mark_region's test: no key condition
    if (hit) field[o] = value;
  }
  const unsigned long long word = __ballot(hit);
  if ((threadIdx.x & 63) == 0 && word) atomicAdd(count, (uint32_t)__popcll(word));
}

__global__ __launch_bounds__(SPH_BLOCK) void k_field_paint_list(const int32_t* __restrict__ list, const uint32_t* __restrict__ vals,
                                                                int n, int N, float* __restrict__ field, float value) {
  const int r = blockIdx.x * SPH_BLOCK + threadIdx.x;
  if (r >= n) return;
  const int j = list[r];
  if (j < 0 || j >= N) return;  // (an entry outside 0..N-1 would be a defect of the selection: never followed)
  const uint32_t o = vals[j];
  if (o < (uint32_t)N) field[o] = value;
}

int sphk_field_paint_region(sph_solver* s, float* field, const SphSelector& a, float value, uint32_t* count) {
  if (s->d.N <= 0) return SPH_OK;
  hipLaunchKernelGGL(k_field_paint_region, dim3(sph_blocks(s->d.N)), dim3(SPH_BLOCK), 0, s->stream, (const float4*)s->d.posOrig, s->d.N, a,
                     field, value, count);
  SPH_HIP(hipGetLastError());
  return SPH_OK;
}

int sphk_field_paint_list(sph_solver* s, float* field, const int32_t* list, int n, float value) {
  if (n <= 0) return SPH_OK;
  hipLaunchKernelGGL(k_field_paint_list, dim3(sph_blocks(n)), dim3(SPH_BLOCK), 0, s->stream, list, (const uint32_t*)s->d.vals, n, s->d.N,
                     field, value);
  SPH_HIP(hipGetLastError());
  return SPH_OK;
}

// ---- following the edits --------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(SPH_BLOCK) void k_field_compact(const float* __restrict__ in, const int32_t* __restrict__ map, int nOld,
                                                             float* __restrict__ out) {
  const int o = blockIdx.x * SPH_BLOCK + threadIdx.x;
  if (o >= nOld) return;
  const int at = map[o];
  if (at >= 0 && at <= o) out[at] = in[o];  // (a survivor never moves up: the guard keeps a corrupted map inside the buffer)
}

__global__ __launch_bounds__(SPH_BLOCK) void k_field_fill(float* __restrict__ field, int n, float value) {
  const int k = blockIdx.x * SPH_BLOCK + threadIdx.x;
  if (k < n) field[k] = value;
}

int sphk_field_compact(sph_solver* s, const float* in, const int32_t* map, int nOld, float* out) {
  if (nOld <= 0) return SPH_OK;
  hipLaunchKernelGGL(k_field_compact, dim3(sph_blocks(nOld)), dim3(SPH_BLOCK), 0, s->stream, in, map, nOld, out);
  SPH_HIP(hipGetLastError());
  return SPH_OK;
}

int sphk_field_fill(sph_solver* s, float* field, int first, int n, float value) {
  if (n <= 0) return SPH_OK;
  hipLaunchKernelGGL(k_field_fill, dim3(sph_blocks(n)), dim3(SPH_BLOCK), 0, s->stream, field + first, n, value);
  SPH_HIP(hipGetLastError());
  return SPH_OK;
}

// ---- region records -------------------------------------------------------------------------------------------------------------
// The rows of the tree (sph_tree.h) are the regions, SPH_FIELD_DIAG_WORDS words each.
// Level 0, one block per chunk of 1024 particles in k_diag_leaf's layout: thread t holds elements t, t + 256, t + 512, t + 768
// (strides 512 and 256 in registers), 128 and 64 through LDS, 32 ... 1 inside a wave. Words: 0 n, 1 sum c, 2 sum c*c (the product
// in double), 3 min, 4 max (float compares, travelling as exactly widened doubles), 5 the selected particles with c != 0.
__global__ __launch_bounds__(SPH_BLOCK) void k_field_leaf(SphDev d, DiagArgs a, const float* __restrict__ field, double* __restrict__ part,
                                                          int chunks) {
  __shared__ double sh[4][SPH_BLOCK];
  __shared__ float shx[4][2];
  const int t = threadIdx.x, chunk = blockIdx.x, lane = t & 63, wave = t >> 6;
  float px[4], py[4], pz[4], c[4];
  bool ok[4];
#pragma unroll
  for (int e = 0; e < 4; e++) {
    const int j = chunk * DIAG_CHUNK + e * SPH_BLOCK + t;
    ok[e] = false;
    px[e] = py[e] = pz[e] = c[e] = 0.f;
    if (j < d.N) {
      const float4 p = d.sortedPos[j];
      const uint32_t o = d.vals[j];
      ok[e] = sph_type_key_selected(d, a.typeMask, j, p) && o < (uint32_t)d.N;
      px[e] = p.x; py[e] = p.y; pz[e] = p.z;
      if (o < (uint32_t)d.N) c[e] = field[o];
    }
  }
  for (int r = 0; r < a.count; r++) {
    const float x0 = a.box[r][0], y0 = a.box[r][1], z0 = a.box[r][2], x1 = a.box[r][3], y1 = a.box[r][4], z1 = a.box[r][5];
    bool sel[4];
#pragma unroll
    for (int e = 0; e < 4; e++) sel[e] = ok[e] && sph_box_holds(x0, y0, z0, x1, y1, z1, px[e], py[e], pz[e]);
    // no particle of this chunk in the region: every sum of +0.0 terms is +0.0 and every extreme keeps its identity
    if (!__syncthreads_or(sel[0] || sel[1] || sel[2] || sel[3])) {
      if (t < FIELD_SUMS) part[tree_at(SPH_FIELD_DIAG_WORDS, r, t, chunks, chunk)] = t == 3 ? (double)INFINITY : t == 4 ? -(double)INFINITY : 0.0;
      continue;
    }
    double q[4][4];
    float mn = INFINITY, mx = -INFINITY;
#pragma unroll
    for (int e = 0; e < 4; e++) {
      const double cd = (double)c[e];
      q[0][e] = sel[e] ? 1.0 : 0.0;
      q[1][e] = sel[e] ? cd : 0.0;
      q[2][e] = sel[e] ? cd * cd : 0.0;
      q[3][e] = sel[e] && c[e] != 0.f ? 1.0 : 0.0;
      if (sel[e]) { mn = c[e] < mn ? c[e] : mn; mx = c[e] > mx ? c[e] : mx; }
    }
#pragma unroll
    for (int k = 0; k < 4; k++) sh[k][t] = (q[k][0] + q[k][2]) + (q[k][1] + q[k][3]);
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) {
      const float om = __shfl_down(mn, s, 64), ox = __shfl_down(mx, s, 64);
      mn = om < mn ? om : mn;
      mx = ox > mx ? ox : mx;
    }
    if (lane == 0) { shx[wave][0] = mn; shx[wave][1] = mx; }
    __syncthreads();
    // strides 128, 64 and the in-wave strides: one word per wave
    tree_group_sums<4>(sh, 4, [&](int k, double x) { part[tree_at(SPH_FIELD_DIAG_WORDS, r, k < 3 ? k : 5, chunks, chunk)] = x; });
    if (t < 2) {
      float x = shx[0][t];
      for (int w = 1; w < 4; w++) { const float o = shx[w][t]; x = t == 0 ? (o < x ? o : x) : (o > x ? o : x); }
      part[tree_at(SPH_FIELD_DIAG_WORDS, r, 3 + t, chunks, chunk)] = (double)x;
    }
    __syncthreads();  // sh / shx are reused by the next region
  }
}

// the records: canonical extremes (+ 0.0f) and the empty-selection rule
__global__ void k_field_final(const double* __restrict__ top /* one chunk per word */, double* __restrict__ out) {
  const int r = blockIdx.x, w = threadIdx.x;  // SPH_FIELD_DIAG_WORDS threads
  const double n = top[tree_at(SPH_FIELD_DIAG_WORDS, r, 0, 1, 0)];
  double x = 0.0;
  if (w < 3 || w == 5) x = top[tree_at(SPH_FIELD_DIAG_WORDS, r, w, 1, 0)];
  else if (w < 5 && n > 0.0) x = (double)((float)top[tree_at(SPH_FIELD_DIAG_WORDS, r, w, 1, 0)] + 0.0f);
  out[r * SPH_FIELD_DIAG_WORDS + w] = x;
}

int sphk_field_diagnostics(sph_solver* s, const float* field, const DiagArgs& a, double* scratch, double** records) {
  const int R = a.count, chunks = tree_chunks(s->d.N);
  hipLaunchKernelGGL(k_field_leaf, dim3(chunks), dim3(SPH_BLOCK), 0, s->stream, s->d, a, field, scratch, chunks);
  SPH_HIP(hipGetLastError());
  TreeShape S = tree_shape(SPH_FIELD_DIAG_WORDS, 3);  // words 0..2 sums, then 3 min, 4 max, 5 a sum
  tree_shape_add(S, 3, DIAG_OP_MIN);
  tree_shape_add(S, 4, DIAG_OP_MAX);
  tree_shape_add(S, 5, DIAG_OP_SUM);
  double *top = nullptr, *out = nullptr;
  const int rc = sphk_tree_upper(s, S, R, scratch, chunks, &top, &out);
  if (rc != SPH_OK) return rc;
  hipLaunchKernelGGL(k_field_final, dim3(R), dim3(SPH_FIELD_DIAG_WORDS), 0, s->stream, (const double*)top, out);
  SPH_HIP(hipGetLastError());
  *records = out;
  return SPH_OK;
}

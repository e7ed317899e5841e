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
#include "sph_selector.h"  // the selection rule of the region totals
#include "sph_wall_record.h"  // WallSet, wl_record: the per-particle record
#include "sph_tree.h"

#include <algorithm>

#define WL_LDS_STRIDE (SPH_WALL_WORDS + 1)  // 33 words: lane-strided ds_write_b32 without bank conflicts
#define WL_SUMS (WL_TERMS + 1)
#define WL_GROUP 9                          // record words reduced together by the leaf: 27 = 3 x 9

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

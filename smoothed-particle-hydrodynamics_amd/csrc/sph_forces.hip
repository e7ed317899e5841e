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
#include "sph_selector.h"  // the selection rule of the region totals
#include "sph_tree.h"

#include <algorithm>

#define FM_BATCH 8
#define FM_LDS_STRIDE (SPH_FORCE_WORDS + 1)  // 41 words: lane-strided ds_write_b32 without bank conflicts
#define FM_TERMS 48                          // words 1..48 of a region record (word 0 counts the particles)
#define FM_SUMS (FM_TERMS + 1)
#define FM_GROUP 7                           // record words reduced together by the leaf: 49 = 7 x 7

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
  __shared__ float sm[OUT == FM_RECORDS ? SPH_BLOCK * FM_LDS_STRIDE : 1];
  const int t = threadIdx.x;
  const int r = blockIdx.x * SPH_BLOCK + t;
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
  if (OUT == FM_RECORDS) {
#pragma unroll
    for (int w = 0; w < SPH_FORCE_WORDS; w++) sm[t * FM_LDS_STRIDE + w] = rec[w];
    __syncthreads();
    const int rows = min(SPH_BLOCK, n - blockIdx.x * SPH_BLOCK);  // records of this block
    float4* dst = reinterpret_cast<float4*>(out + (size_t)blockIdx.x * SPH_BLOCK * SPH_FORCE_WORDS);
    const int quads = rows * (SPH_FORCE_WORDS / 4);
    for (int q = t; q < quads; q += SPH_BLOCK) {
      const float* src = sm + (q / (SPH_FORCE_WORDS / 4)) * FM_LDS_STRIDE + 4 * (q % (SPH_FORCE_WORDS / 4));
      dst[q] = make_float4(src[0], src[1], src[2], src[3]);
    }
  } else {
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

// ---- region totals ----------------------------------------------------------------------------------------------------------
// Partials of a level: part[(region * SPH_FORCE_DIAG_WORDS + word) * chunks + chunk], read coalesced by the next level.
__device__ __forceinline__ size_t fm_at(int region, int word, int chunks, int chunk) {
  return ((size_t)(region * SPH_FORCE_DIAG_WORDS + word)) * (size_t)chunks + (size_t)chunk;
}

// Level 0 for the chunks [firstChunk, firstChunk + gridDim.x) whose terms lie at `terms` (word-major, `stride` particles per
// word, particle firstChunk * 1024 first). One block per chunk of 1024 particles in k_diag_leaf's layout: thread t holds
// elements t, t + 256, t + 512, t + 768 (strides 512 and 256 in registers), 128 and 64 through LDS, 32 ... 1 inside a wave.
// The words go through in groups of FM_GROUP, so that a term is read once whatever the number of regions.
__global__ __launch_bounds__(SPH_BLOCK) void k_force_leaf(SphDev d, DiagArgs a, const float* __restrict__ terms, size_t stride,
                                                          int firstChunk, double* __restrict__ part, int chunks) {
  __shared__ double sh[FM_GROUP][SPH_BLOCK];
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
  for (int g = 0; g < FM_SUMS / FM_GROUP; g++) {
    float f[4][FM_GROUP];
#pragma unroll
    for (int e = 0; e < 4; e++) {
      const int j = chunk * DIAG_CHUNK + e * SPH_BLOCK + t;
      const size_t at = (size_t)(blockIdx.x * DIAG_CHUNK + e * SPH_BLOCK + t);
#pragma unroll
      for (int k = 0; k < FM_GROUP; k++) {
        const int w = g * FM_GROUP + k;  // record word; word 0 counts
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
        if (t < FM_GROUP) part[fm_at(r, g * FM_GROUP + t, chunks, chunk)] = 0.0;
        continue;
      }
#pragma unroll
      for (int k = 0; k < FM_GROUP; k++) {
        double q[4];
#pragma unroll
        for (int e = 0; e < 4; e++) q[e] = sel[e] ? (double)f[e][k] : 0.0;
        sh[k][t] = (q[0] + q[2]) + (q[1] + q[3]);
      }
      __syncthreads();
      if (t < 128) {
#pragma unroll
        for (int k = 0; k < FM_GROUP; k++) sh[k][t] = sh[k][t] + sh[k][t + 128];
      }
      __syncthreads();
      for (int k = wave; k < FM_GROUP; k += 4) {
        const double x = diag_wave_sum(sh[k][lane] + sh[k][lane + 64]);
        if (lane == 0) part[fm_at(r, g * FM_GROUP + k, chunks, chunk)] = x;
      }
      __syncthreads();  // sh is reused by the next region
    }
  }
}

// Upper levels: `nIn` partials per word and region -> ceil(nIn / 1024), the same tree. One block per output chunk, region and word.
__global__ __launch_bounds__(SPH_BLOCK) void k_force_upper(const double* __restrict__ in, int nIn, double* __restrict__ out, int nOut) {
  __shared__ double sh[SPH_BLOCK];
  const int chunk = blockIdx.x, r = blockIdx.y, w = blockIdx.z;
  const double x = diag_block_reduce<DIAG_OP_SUM>(in + fm_at(r, w, nIn, 0), nIn, chunk, 0.0, sh);
  if (threadIdx.x == 0) out[fm_at(r, w, nOut, chunk)] = x;
}

__global__ void k_force_final(const double* __restrict__ top /* one chunk per word */, double* __restrict__ out) {
  const int r = blockIdx.x, w = threadIdx.x;  // SPH_FORCE_DIAG_WORDS threads
  out[r * SPH_FORCE_DIAG_WORDS + w] = w < FM_SUMS ? top[fm_at(r, w, 1, 0)] : 0.0;
}

static int fm_chunks(int n) { return n > 0 ? (n + DIAG_CHUNK - 1) / DIAG_CHUNK : 1; }

size_t sphk_force_diag_scratch_doubles(int N, int regions) {
  size_t total = 0;
  for (int c = fm_chunks(N);; c = fm_chunks(c)) {
    total += (size_t)c;
    if (c == 1) break;
  }
  return (total + 1) * (size_t)regions * SPH_FORCE_DIAG_WORDS;  // the levels' partials, then the records
}

size_t sphk_force_terms_bytes(int chunks) { return sizeof(float) * FM_TERMS * DIAG_CHUNK * (size_t)chunks; }

int sphk_force_diagnostics(sph_solver* s, const DiagArgs& a, float* terms, int pieceChunks, double* scratch, double** records) {
  const int R = a.count, N = s->d.N;
  int chunks = fm_chunks(N);
  double* cur = scratch;
  const size_t stride = (size_t)pieceChunks * DIAG_CHUNK;
  for (int c0 = 0; c0 < chunks; c0 += pieceChunks) {
    const int nC = std::min(pieceChunks, chunks - c0);
    const int first = c0 * DIAG_CHUNK, n = std::min(nC * DIAG_CHUNK, N - first);
    if (n > 0) hipLaunchKernelGGL((k_force_records<FM_TERMS_OUT, false>), dim3(sph_blocks(n)), dim3(SPH_BLOCK), 0, s->stream, s->d, first, n,
                                  (const int32_t*)nullptr, terms, stride);
    hipLaunchKernelGGL(k_force_leaf, dim3(nC), dim3(SPH_BLOCK), 0, s->stream, s->d, a, (const float*)terms, stride, c0, cur, chunks);
    SPH_HIP(hipGetLastError());
  }
  while (chunks > 1) {
    const int nOut = fm_chunks(chunks);
    double* next = cur + (size_t)R * SPH_FORCE_DIAG_WORDS * (size_t)chunks;
    hipLaunchKernelGGL(k_force_upper, dim3(nOut, R, FM_SUMS), dim3(SPH_BLOCK), 0, s->stream, (const double*)cur, chunks, next, nOut);
    SPH_HIP(hipGetLastError());
    cur = next; chunks = nOut;
  }
  double* out = cur + (size_t)R * SPH_FORCE_DIAG_WORDS;
  hipLaunchKernelGGL(k_force_final, dim3(R), dim3(SPH_FORCE_DIAG_WORDS), 0, s->stream, (const double*)cur, out);
  SPH_HIP(hipGetLastError());
  *records = out;
  return SPH_OK;
}

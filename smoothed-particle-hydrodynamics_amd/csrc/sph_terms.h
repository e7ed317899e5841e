// What the force decomposition (sph_forces.hip) and the wall loads (sph_wall.hip) do alike around their own per-particle record:
// the records' way out through LDS, and the region totals over terms staged word-major -- leaf, upper levels (sph_tree.h), final,
// and the host loop over pieces of whole chunks. Templates: each of the two files instantiates the kernels with its constants.
#pragma once
#include "sph_common.h"
#include "sph_selector.h"  // the selection rule of the region totals
#include "sph_tree.h"

#include <algorithm>

// A block's records of WORDS floats, one per thread in rec[], out as one contiguous piece: through sm (SPH_BLOCK * (WORDS + 1)
// floats: lane-strided ds_write_b32 without bank conflicts), then 16-byte stores of consecutive lanes (a WORDS * 4-byte stride per
// lane is the 4x write amplification of DESIGN.md §7 item 3). n: records of the launch; out: 16-byte aligned.
template <int WORDS>
__device__ __forceinline__ void records_through_lds(const float (&rec)[WORDS], float* sm, int n, float* __restrict__ out) {
  const int t = threadIdx.x;
#pragma unroll
  for (int w = 0; w < WORDS; w++) sm[t * (WORDS + 1) + w] = rec[w];
  __syncthreads();
  const int rows = min(SPH_BLOCK, n - blockIdx.x * SPH_BLOCK);  // records of this block
  float4* dst = reinterpret_cast<float4*>(out + (size_t)blockIdx.x * SPH_BLOCK * WORDS);
  const int quads = rows * (WORDS / 4);
  for (int q = t; q < quads; q += SPH_BLOCK) {
    const float* src = sm + (q / (WORDS / 4)) * (WORDS + 1) + 4 * (q % (WORDS / 4));
    dst[q] = make_float4(src[0], src[1], src[2], src[3]);
  }
}

// Level 0 for the chunks [firstChunk, firstChunk + gridDim.x) whose terms lie at `terms` (word-major, `stride` particles per
// word, particle firstChunk * 1024 first). One block per chunk of 1024 particles in k_diag_leaf's layout: thread t holds
// elements t, t + 256, t + 512, t + 768 (strides 512 and 256 in registers), 128 and 64 through LDS, 32 ... 1 inside a wave.
// The SUMS words of a region record (word 0 counts, word w is term w - 1) go through in groups of GROUP, so that a term is read
// once whatever the number of regions. Rows of the tree: the regions, ROW_WORDS words each.
template <int ROW_WORDS, int SUMS, int GROUP>
__global__ __launch_bounds__(SPH_BLOCK) void k_terms_leaf(SphDev d, DiagArgs a, const float* __restrict__ terms, size_t stride,
                                                          int firstChunk, double* __restrict__ part, int chunks) {
  static_assert(SUMS % GROUP == 0, "the words go through in whole groups");
  __shared__ double sh[GROUP][SPH_BLOCK];
  const int t = threadIdx.x, chunk = firstChunk + blockIdx.x;
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
  for (int g = 0; g < SUMS / GROUP; g++) {
    float f[4][GROUP];
#pragma unroll
    for (int e = 0; e < 4; e++) {
      const int j = chunk * DIAG_CHUNK + e * SPH_BLOCK + t;
      const size_t at = (size_t)(blockIdx.x * DIAG_CHUNK + e * SPH_BLOCK + t);
#pragma unroll
      for (int k = 0; k < GROUP; k++) {
        const int w = g * GROUP + k;  // record word; word 0 counts
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
        if (t < GROUP) part[tree_at(ROW_WORDS, r, g * GROUP + t, chunks, chunk)] = 0.0;
        continue;
      }
#pragma unroll
      for (int k = 0; k < GROUP; k++) {
        double q[4];
#pragma unroll
        for (int e = 0; e < 4; e++) q[e] = sel[e] ? (double)f[e][k] : 0.0;
        sh[k][t] = (q[0] + q[2]) + (q[1] + q[3]);
      }
      __syncthreads();
      tree_group_sums<GROUP>(sh, GROUP, [&](int k, double x) { part[tree_at(ROW_WORDS, r, g * GROUP + k, chunks, chunk)] = x; });
      __syncthreads();  // sh is reused by the next region
    }
  }
}

template <int ROW_WORDS, int SUMS>
__global__ void k_terms_final(const double* __restrict__ top /* one chunk per word */, double* __restrict__ out) {
  const int r = blockIdx.x, w = threadIdx.x;  // ROW_WORDS threads
  out[r * ROW_WORDS + w] = w < SUMS ? top[tree_at(ROW_WORDS, r, w, 1, 0)] : 0.0;
}

// The region totals of a.count regions: the particles go through `terms` (terms_bytes(SUMS - 1, pieceChunks)) in pieces of
// pieceChunks chunks, records(first, n, terms, stride) launching the kernel that writes the SUMS - 1 terms of particles
// first .. first + n at terms[word * stride + r]; *records: where the a.count x ROW_WORDS doubles land (in scratch).
template <int ROW_WORDS, int SUMS, int GROUP, class Records>
int sphk_terms_diagnostics(sph_solver* s, const DiagArgs& a, float* terms, int pieceChunks, double* scratch, double** records,
                           Records launchRecords) {
  const int R = a.count, N = s->d.N, chunks = tree_chunks(N);
  const size_t stride = (size_t)pieceChunks * DIAG_CHUNK;
  for (int c0 = 0; c0 < chunks; c0 += pieceChunks) {
    const int nC = std::min(pieceChunks, chunks - c0);
    const int first = c0 * DIAG_CHUNK, n = std::min(nC * DIAG_CHUNK, N - first);
    if (n > 0) launchRecords(first, n, terms, stride);
    hipLaunchKernelGGL((k_terms_leaf<ROW_WORDS, SUMS, GROUP>), dim3(nC), dim3(SPH_BLOCK), 0, s->stream, s->d, a, (const float*)terms, stride,
                       c0, scratch, chunks);
    SPH_HIP(hipGetLastError());
  }
  double *top = nullptr, *out = nullptr;
  const int rc = sphk_tree_upper(s, tree_shape(ROW_WORDS, SUMS), R, scratch, chunks, &top, &out);
  if (rc != SPH_OK) return rc;
  hipLaunchKernelGGL((k_terms_final<ROW_WORDS, SUMS>), dim3(R), dim3(ROW_WORDS), 0, s->stream, (const double*)top, out);
  SPH_HIP(hipGetLastError());
  *records = out;
  return SPH_OK;
}

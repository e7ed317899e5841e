// The upper levels of the fixed reduction tree (sph_tree.h), for every tree of the library: `nIn` partials per row and word ->
// ceil(nIn / 1024), one block per output chunk, row and job of the shape. Tiny launches.
#include "sph_tree.h"

__global__ __launch_bounds__(SPH_BLOCK) void k_tree_upper(TreeShape S, const double* __restrict__ in, int nIn, double* __restrict__ out,
                                                          int nOut) {
  __shared__ double sh[SPH_BLOCK];
  __shared__ double shI[SPH_BLOCK];
  const int t = threadIdx.x, chunk = blockIdx.x, r = blockIdx.y, job = blockIdx.z;
  if (r < 32 && !((S.rowMask >> r) & 1u)) return;  // (block-uniform, as every branch below)
  int w = job, op = DIAG_OP_SUM;
  if (job >= S.sums) { w = S.word[job - S.sums]; op = S.op[job - S.sums]; }
  if (r == S.shortRow && w >= S.shortWords) return;
  const double* src = in + tree_at(S.rowWords, r, w, nIn, 0);
  double* dst = out + tree_at(S.rowWords, r, w, nOut, chunk);
  if (op == DIAG_OP_PAIR) {  // (max value, lowest index that attains it): words w and w + 1
    const double* srcI = in + tree_at(S.rowWords, r, w + 1, nIn, 0);
    double bv = -(double)INFINITY, bi = 2147483647.0;
    for (int k = 0; k < 4; k++) {
      const int i = chunk * DIAG_CHUNK + k * SPH_BLOCK + t;
      if (i >= nIn) continue;
      const double ov = src[i], oi = srcI[i];
      if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
    }
    sh[t] = bv; shI[t] = bi;
    __syncthreads();
    for (int s = 128; s >= 1; s >>= 1) {
      if (t < s && (sh[t + s] > sh[t] || (sh[t + s] == sh[t] && shI[t + s] < shI[t]))) { sh[t] = sh[t + s]; shI[t] = shI[t + s]; }
      __syncthreads();
    }
    if (t == 0) { dst[0] = sh[0]; out[tree_at(S.rowWords, r, w + 1, nOut, chunk)] = shI[0]; }
    return;
  }
  double x;
  if (op == DIAG_OP_MIN) x = diag_block_reduce<DIAG_OP_MIN>(src, nIn, chunk, (double)INFINITY, sh);
  else if (op == DIAG_OP_MAX) x = diag_block_reduce<DIAG_OP_MAX>(src, nIn, chunk, -(double)INFINITY, sh);
  else x = diag_block_reduce<DIAG_OP_SUM>(src, nIn, chunk, 0.0, sh);
  if (t == 0) dst[0] = x;
}

int sphk_tree_upper(sph_solver* s, const TreeShape& S, int rows, double* cur, int chunks, double** top, double** end) {
  if (S.listed > TREE_MAX_LISTED || (S.rowMask != 0xffffffffu && rows > 32)) {
    sph_set_error("sphk_tree_upper: a shape of %d listed jobs, or a row mask over %d rows", S.listed, rows);
    return SPH_ERR_INVALID;
  }
  const size_t rowDoubles = (size_t)rows * (size_t)S.rowWords;
  while (chunks > 1) {
    const int nOut = tree_chunks(chunks);
    double* next = cur + rowDoubles * (size_t)chunks;
    hipLaunchKernelGGL(k_tree_upper, dim3(nOut, rows, S.sums + S.listed), dim3(SPH_BLOCK), 0, s->stream, S, (const double*)cur, chunks, next, nOut);
    SPH_HIP(hipGetLastError());
    cur = next; chunks = nOut;
  }
  *top = cur;
  *end = cur + rowDoubles;
  return SPH_OK;
}

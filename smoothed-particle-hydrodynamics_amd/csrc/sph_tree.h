// The fixed reduction tree of the diagnostics contract (include/sphmi.h, reduce(a)): terms padded with +0.0 to whole chunks of
// 1024; in a chunk, a[i] += a[i + stride] for stride = 512 ... 1; the chunks' results are the terms of the next level, until one
// chunk is left. The summation order is the API, so everything that fixes it is here, once, for the seven trees of the library
// (sph_diag, sph_forces, sph_wall, sph_fields, sph_elastic_measure, sph_gauge, sph_body_dynamics):
//   layout     a level is part[(row * rowWords + word) * chunks + chunk] (tree_at), the levels lie one behind the other
//              (tree_chunks, tree_level_chunks size them), so that the next level reads its terms coalesced
//   level 0    one 256-thread block owns one chunk. Each leaf kernel loads and selects its own terms and adds strides 512 and 256
//              in registers, (e0 + e2) + (e1 + e3); tree_group_sums takes GROUP such words on from LDS: stride 128, then per wave
//              stride 64 and diag_wave_sum (32 ... 1)
//   upper      sphk_tree_upper (sph_tree.hip) launches one kernel per level, diag_block_reduce per (chunk, row, job) of a TreeShape
// Not here: what a leaf reads, whom it selects, its float extremes, and the kernel that turns the top level into records.
#pragma once
#include "sph_common.h"

#define DIAG_CHUNK 1024

__host__ __device__ __forceinline__ size_t tree_at(int rowWords, int row, int word, int chunks, int chunk) {
  return ((size_t)(row * rowWords + word)) * (size_t)chunks + (size_t)chunk;
}

// chunks of a level of n terms (a tree over nothing still has its one chunk of padding)
inline int tree_chunks(long long n) { return n > 0 ? (int)((n + DIAG_CHUNK - 1) / DIAG_CHUNK) : 1; }

// ... and of all levels of a tree over n terms: partials per row and word
inline size_t tree_level_chunks(long long n) {
  size_t total = 0;
  for (int c = tree_chunks(n);; c = tree_chunks(c)) {
    total += (size_t)c;
    if (c == 1) return total;
  }
}

// doubles of a scratch that holds every level of `rows` rows over n terms and, behind them, a record of rowWords doubles per row
inline size_t tree_scratch_doubles(long long n, int rows, int rowWords) {
  return (tree_level_chunks(n) + 1) * (size_t)rows * (size_t)rowWords;
}

// bytes of `terms` per-particle floats staged word-major for `chunks` chunks of particles (sph_terms.h)
inline size_t terms_bytes(int terms, int chunks) { return sizeof(float) * (size_t)terms * DIAG_CHUNK * (size_t)chunks; }

__device__ __forceinline__ double diag_wave_sum(double x) {  // strides 32 ... 1 of the tree; lane 0 holds the result
#pragma unroll
  for (int s = 32; s >= 1; s >>= 1) x = x + __shfl_down(x, s, 64);
  return x;
}

// The tail of a leaf: sh[k][t], k < GROUP, holds thread t's (e0 + e2) + (e1 + e3) of word k, and a barrier lies behind the
// writes. Stride 128 for all GROUP words, then waves k = wave, wave + 4, ... < count add stride 64 and the in-wave strides; lane 0
// hands word k's sum of the chunk to store(k, x). The caller puts a barrier behind this before it writes sh again.
template <int GROUP, class Store>
__device__ __forceinline__ void tree_group_sums(double (*sh)[SPH_BLOCK], int count, Store store) {
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  if (t < 128) {
#pragma unroll
    for (int k = 0; k < GROUP; k++) sh[k][t] = sh[k][t] + sh[k][t + 128];
  }
  __syncthreads();
  for (int k = wave; k < count; k += 4) {
    const double x = diag_wave_sum(sh[k][lane] + sh[k][lane + 64]);
    if (lane == 0) store(k, x);
  }
}

enum { DIAG_OP_SUM = 0, DIAG_OP_MIN = 1, DIAG_OP_MAX = 2, DIAG_OP_PAIR = 3 };

template <int OP>
__device__ __forceinline__ double diag_combine(double a, double b) {
  if (OP == DIAG_OP_SUM) return a + b;
  if (OP == DIAG_OP_MIN) return b < a ? b : a;
  return b > a ? b : a;
}

// chunk `chunk` of the nIn partials at `in` (padded with `pad`), by a whole block; sh: SPH_BLOCK doubles of LDS
template <int OP>
__device__ double diag_block_reduce(const double* __restrict__ in, int nIn, int chunk, double pad, double* sh) {
  const int t = threadIdx.x;
  double e[4];
#pragma unroll
  for (int k = 0; k < 4; k++) {
    const int i = chunk * DIAG_CHUNK + k * SPH_BLOCK + t;
    e[k] = i < nIn ? in[i] : pad;
  }
  sh[t] = diag_combine<OP>(diag_combine<OP>(e[0], e[2]), diag_combine<OP>(e[1], e[3]));
  __syncthreads();
  for (int s = 128; s >= 1; s >>= 1) {
    if (t < s) sh[t] = diag_combine<OP>(sh[t], sh[t + s]);
    __syncthreads();
  }
  const double x = sh[0];
  __syncthreads();
  return x;
}

// What the upper levels of a tree reduce, by value to the kernel. Jobs 0 .. sums-1 are the sums of words 0 .. sums-1 (a force
// record has 49 of them); the jobs behind them are listed as (word, op), op one of DIAG_OP_*. DIAG_OP_PAIR is the diagnostics'
// (max value, lowest index that attains it) over the words (word, word + 1).
#define TREE_MAX_LISTED 16
struct TreeShape {
  int rowWords;
  int sums;
  int listed;
  // rows 0..31 whose bit is clear are not reduced (level 0 left them unwritten); all ones: every row. A row >= 32 is always
  // reduced, so a tree with a mask that is not all ones has at most 32 rows (sphk_tree_upper refuses any other).
  uint32_t rowMask;
  int shortRow, shortWords;  // row shortRow holds only words 0 .. shortWords-1 (shortRow = -1: no such row)
  uint8_t word[TREE_MAX_LISTED], op[TREE_MAX_LISTED];
};
inline TreeShape tree_shape(int rowWords, int sums, uint32_t rowMask = 0xffffffffu) {
  TreeShape S = {};
  S.rowWords = rowWords; S.sums = sums; S.rowMask = rowMask; S.shortRow = -1;
  return S;
}
// (an entry beyond TREE_MAX_LISTED is counted and not stored: sphk_tree_upper refuses the shape)
inline void tree_shape_add(TreeShape& S, int word, int op) {
  if (S.listed < TREE_MAX_LISTED) { S.word[S.listed] = (uint8_t)word; S.op[S.listed] = (uint8_t)op; }
  S.listed++;
}

// Levels above `cur` (chunks partials per row and word, `rows` rows) until one chunk is left, each level directly behind the one
// it reduces. *top: where the last level lies, *end: the address behind it. SPH_ERR_INVALID for a shape with more than
// TREE_MAX_LISTED listed jobs or with a row mask over more than 32 rows; nothing is launched then.
int sphk_tree_upper(sph_solver* s, const TreeShape& S, int rows, double* cur, int chunks, double** top, double** end);

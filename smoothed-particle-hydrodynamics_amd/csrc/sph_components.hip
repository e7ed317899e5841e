// Connected components of the particles (include/sphmi.h: sph_label_components / sph_read_components). The graph:
// nodes = the selected sorted particles (type and key: sph_selector.h), edges = the entries of the last step's neighbour rows
// between two selected particles (either end's row; optionally only pairs closer than a link radius). Read-only on every solver
// array.
//   k_cc_init      parent[j] = selected ? j : -1
//   k_cc_prelink   parent[i] = the smallest particle below i that i's own row links it to: a forest without a single atomic
//   k_cc_compress  pointer jumping on that forest, so that the hooks start from short trees
//   k_cc_hook      one lane per particle walks its row: lock-free union-find, the LARGER root is hooked under the smaller by a
//                  compare-and-swap on parent[larger root], path halving in find
//   k_cc_flatten   parent[j] = root of j (a launch of its own: it sees every hook)
//   k_cc_flags     per-block counts of roots and of selected particles
//   k_cc_scan      one workgroup: exclusive offsets of the block counts, the totals (C, selected) for the host
//   k_cc_rank      roots: labels[r] = rank of r among the roots in sorted order; opens the root's table row
//   k_cc_label     labels[j] = labels[parent[j]]
//   k_cc_table     members and bounding box per component: integer atomics, aggregated per wave over runs of equal labels and
//                  per block at the end
//   k_cc_table_fin the bounding boxes back from their integer images to floats (+ 0.0f)
// Every result is an integer or a float minimum / maximum, and none depends on the order of execution: parent[x] <= x always,
// and parent[x] is a member of x's set, so every tree's root is the minimum of its set whatever the interleaving.
// Every access to `parent` while hooks are running is an agent-scope atomic (the XCDs' L2s are not coherent for plain accesses);
// a stale value read on the way is still a smaller member of the same set, and a hook is a compare-and-swap that expects
// parent[r] == r, so it fails, and is retried from the value it returns, if r has stopped being a root.
// Every pointer walk and every retry loop is bounded by N + 1 steps; an overrun sets err[0] instead of spinning.
#include "sph_common.h"
#include "sph_row_walk.h"
#include "sph_selector.h"  // the type and key pieces of the selection rule
#include "sph_union_find.h"  // cc_load, cc_find, cc_union, cc_block_exclusive, cc_ordered: shared with sph_shells.hip

#include <algorithm>

#define CC_SCAN_THREADS 1024
#define CC_TABLE_WORDS 8  // root, n, then min x, y, z, max x, y, z

__global__ __launch_bounds__(SPH_BLOCK) void k_cc_init(SphDev d, uint32_t typeMask, int32_t* __restrict__ parent) {
  const int j = blockIdx.x * SPH_BLOCK + threadIdx.x;
  if (j >= d.N) return;
  parent[j] = sph_type_key_selected(d, typeMask, j, d.sortedPos[j]) ? j : -1;
}

// fn(j) for every entry j of selected particle i's row that is an edge of the contract (j selected, j != i, r2 < link2 if FINITE)
template <bool FINITE, typename F>
__device__ __forceinline__ void cc_for_each_edge(const SphDev& d, float link2, const int32_t* parent, int i, F fn) {
  float4 pi = make_float4(0.f, 0.f, 0.f, 0.f);
  if (FINITE) pi = d.sortedPos[i];
  sph_row_for_each_slot(d, i, [&](int j) {
    if (j < 0 || j >= d.N || j == i) return;
    if (cc_load(parent + j) < 0) return;  // not selected (-1 never changes)
    if (FINITE) {
      const float4 pj = d.sortedPos[j];
      const float dx = pi.x - pj.x, dy = pi.y - pj.y, dz = pi.z - pj.z;
      const float r2 = dx * dx + dy * dy + dz * dz;
      if (!(r2 < link2)) return;
    }
    fn(j);
  });
}

// (The kernels that walk `parent` take their blocks in XCD order — xcd_block, sph_common.h — so that the parent lines their finds
// walk stay in one XCD's L2.)
// Before any hook: parent[i] = the smallest particle below i that i's own row links it to (or i). A forest already (parent[i] <= i,
// same set), written without atomics: only lane i writes entry i here, and other lanes only test the sign of what they read.
template <bool FINITE>
__global__ __launch_bounds__(SPH_BLOCK) void k_cc_prelink(SphDev d, float link2, int32_t* parent) {
  const int i = xcd_block(gridDim.x) * SPH_BLOCK + threadIdx.x;
  if (i >= d.N) return;
  if (cc_load(parent + i) < 0) return;
  int m = i;
  cc_for_each_edge<FINITE>(d, link2, parent, i, [&](int j) { m = j < m ? j : m; });
  if (m != i) __hip_atomic_store(parent + i, m, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Pointer jumping on the forest k_cc_prelink left (no hooks run meanwhile): parent[i] moves to its grandparent until its parent is
// a root. Only lane i writes entry i; whatever another lane reads there is an ancestor of i. With every lane jumping at once a
// chain of length L is gone after about log2(L) rounds (the sorted order follows the cells, so the chains of a long box run
// hundreds of cell layers deep).
__global__ __launch_bounds__(SPH_BLOCK) void k_cc_compress(int N, int32_t* parent, uint32_t* err) {
  const int i = xcd_block(gridDim.x) * SPH_BLOCK + threadIdx.x;
  if (i >= N) return;
  int p = cc_load(parent + i);
  if (p < 0) return;
  for (int steps = 0;; steps++) {
    const int g = cc_load(parent + p);
    if (g == p) break;
    __hip_atomic_store(parent + i, g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    p = g;
    if (steps > N) { atomicOr(err, 8u); break; }
  }
}

template <bool FINITE>
__global__ __launch_bounds__(SPH_BLOCK) void k_cc_hook(SphDev d, float link2, int32_t* parent, uint32_t* err) {
  const int i = xcd_block(gridDim.x) * SPH_BLOCK + threadIdx.x;
  if (i >= d.N) return;
  if (cc_load(parent + i) < 0) return;
  int mine = i;  // a member of i's set, as close to its root as this lane has seen: where the next find for i starts
  cc_for_each_edge<FINITE>(d, link2, parent, i, [&](int j) { mine = cc_union(parent, mine, j, d.N, err); });
}

// Read-only walk to the root, then one store to the particle's own entry. Another lane that passes through this entry meanwhile
// reads either the old value or the root: both are members of the set that are not larger than the entry's index.
__global__ __launch_bounds__(SPH_BLOCK) void k_cc_flatten(int N, int32_t* parent, uint32_t* err) {
  const int j = xcd_block(gridDim.x) * SPH_BLOCK + threadIdx.x;
  if (j >= N) return;
  int x = cc_load(parent + j);
  if (x < 0) return;
  int steps = 0;
  for (int p = cc_load(parent + x); p != x; p = cc_load(parent + x)) {
    x = p;
    if (++steps > N) { atomicOr(err, 4u); return; }
  }
  __hip_atomic_store(parent + j, x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ __launch_bounds__(SPH_BLOCK) void k_cc_flags(int N, const int32_t* __restrict__ parent, uint2* __restrict__ blockTot) {
  const int j = blockIdx.x * SPH_BLOCK + threadIdx.x;
  const int p = j < N ? parent[j] : -1;
  uint32_t roots, sel;
  cc_block_exclusive(p == j ? 1u : 0u, roots);
  cc_block_exclusive(p >= 0 ? 1u : 0u, sel);
  if (threadIdx.x == 0) blockTot[blockIdx.x] = make_uint2(roots, sel);
}

// off[b] = roots in blocks < b; totals = {selected, roots, err[0]}. One workgroup: each thread sums a contiguous run of blocks,
// the run sums are scanned in LDS, then each thread writes its run's offsets (the pattern of k_surface_scan).
__global__ __launch_bounds__(CC_SCAN_THREADS) void k_cc_scan(const uint2* __restrict__ blockTot, int nb, uint32_t* __restrict__ off,
                                                             const uint32_t* __restrict__ err, uint32_t* __restrict__ totals) {
  __shared__ uint32_t sR[CC_SCAN_THREADS], sS[CC_SCAN_THREADS];
  const int tid = threadIdx.x;
  const int per = (nb + CC_SCAN_THREADS - 1) / CC_SCAN_THREADS;
  const int b0 = min(tid * per, nb), b1 = min(b0 + per, nb);
  uint32_t r = 0, q = 0;
  for (int b = b0; b < b1; b++) { const uint2 x = blockTot[b]; r += x.x; q += x.y; }
  sR[tid] = r; sS[tid] = q;
  __syncthreads();
  for (int o = 1; o < CC_SCAN_THREADS; o <<= 1) {  // inclusive Hillis-Steele scan
    uint32_t ar = 0, as = 0;
    if (tid >= o) { ar = sR[tid - o]; as = sS[tid - o]; }
    __syncthreads();
    sR[tid] += ar; sS[tid] += as;
    __syncthreads();
  }
  uint32_t o = sR[tid] - r;
  for (int b = b0; b < b1; b++) { off[b] = o; o += blockTot[b].x; }
  if (tid == CC_SCAN_THREADS - 1) { totals[0] = sS[tid]; totals[1] = sR[tid]; totals[2] = err[0]; }
}

__global__ __launch_bounds__(SPH_BLOCK) void k_cc_rank(int N, const int32_t* __restrict__ parent, const uint32_t* __restrict__ off,
                                                       int32_t* __restrict__ labels, int32_t* __restrict__ table) {
  const int j = blockIdx.x * SPH_BLOCK + threadIdx.x;
  const bool root = j < N && parent[j] == j;
  uint32_t total;
  const uint32_t rank = off[blockIdx.x] + cc_block_exclusive(root ? 1u : 0u, total);
  if (!root) return;
  labels[j] = (int32_t)rank;
  int32_t* row = table + (size_t)rank * CC_TABLE_WORDS;
  row[0] = j; row[1] = 0;
  row[2] = row[3] = row[4] = 0x7fffffff;
  row[5] = row[6] = row[7] = (int32_t)0x80000000;
}

__global__ __launch_bounds__(SPH_BLOCK) void k_cc_label(int N, const int32_t* __restrict__ parent, int32_t* labels) {
  const int j = blockIdx.x * SPH_BLOCK + threadIdx.x;
  if (j >= N) return;
  const int p = parent[j];
  if (p == j) return;  // a root: k_cc_rank has written its label, and only roots' labels are read here
  labels[j] = p < 0 ? -1 : labels[p];
}

struct CcAcc {  // per lane: members and box of the lane's particles in the current run
  int n, mn[3], mx[3];
  __device__ __forceinline__ void clear() { n = 0; mn[0] = mn[1] = mn[2] = 0x7fffffff; mx[0] = mx[1] = mx[2] = (int)0x80000000; }
  __device__ __forceinline__ void add(const int q[3]) {
    n++;
#pragma unroll
    for (int k = 0; k < 3; k++) { mn[k] = min(mn[k], q[k]); mx[k] = max(mx[k], q[k]); }
  }
};

__device__ __forceinline__ void cc_row_add(int32_t* table, int label, const CcAcc& a) {
  int32_t* row = table + (size_t)label * CC_TABLE_WORDS;
  atomicAdd(row + 1, a.n);
#pragma unroll
  for (int k = 0; k < 3; k++) { atomicMin(row + 2 + k, a.mn[k]); atomicMax(row + 5 + k, a.mx[k]); }
}

// the sum / minimum / maximum of the wave's accumulators, in lane 0
__device__ __forceinline__ CcAcc cc_wave_reduce(CcAcc a) {
#pragma unroll
  for (int s = 32; s >= 1; s >>= 1) {
    a.n += __shfl_down(a.n, s, CC_WAVE);
#pragma unroll
    for (int k = 0; k < 3; k++) { a.mn[k] = min(a.mn[k], __shfl_down(a.mn[k], s, CC_WAVE)); a.mx[k] = max(a.mx[k], __shfl_down(a.mx[k], s, CC_WAVE)); }
  }
  return a;
}

// the whole wave's accumulators (all for `label`) -> one set of atomics by lane 0
__device__ __forceinline__ void cc_flush(int32_t* table, int label, const CcAcc& acc) {
  const CcAcc a = cc_wave_reduce(acc);
  if ((threadIdx.x & (CC_WAVE - 1)) == 0 && a.n > 0) cc_row_add(table, label, a);
}

// Each wave owns a contiguous run of `perWave` particles (a multiple of 64). Consecutive sorted particles nearly always share a
// label (in bulk liquid millions do), or alternate between two (liquid and the wall it touches), so a wave keeps the runs of its
// two most recent labels in registers, lane by lane, and touches memory once per run: one set of 7 integer atomics per wave and
// label instead of one per particle. A step takes up to four labels through these accumulators and the rest lane by lane. What
// the four waves of a block still hold at the end is merged through LDS first: atomics on one table row run one after the other
// (about 90 per microsecond), and in bulk liquid every wave ends with the same label.
__global__ __launch_bounds__(SPH_BLOCK) void k_cc_table(SphDev d, const int32_t* __restrict__ labels, int32_t* table, int perWave) {
  const int lane = threadIdx.x & (CC_WAVE - 1);
  const long long wave = (long long)blockIdx.x * CC_WAVES + threadIdx.x / CC_WAVE;
  __shared__ int shLab[2 * CC_WAVES];
  __shared__ CcAcc shAcc[2 * CC_WAVES];
  const long long begin = min(wave * perWave, (long long)d.N);  // (a wave past the end has no work, but joins the block's merge)
  const int end = (int)min((long long)d.N, begin + perWave);
  CcAcc acc0, acc1;  // slot 0: the most recent label
  acc0.clear();
  acc1.clear();
  int cur0 = -1, cur1 = -1;  // wave-uniform: the labels the accumulators belong to
  for (int j0 = (int)begin; j0 < end; j0 += CC_WAVE) {
    const int j = j0 + lane;
    const int lab = j < end ? labels[j] : -1;
    int q[3] = {0, 0, 0};
    if (lab >= 0) {
      const float4 p = d.sortedPos[j];
      q[0] = cc_ordered(p.x); q[1] = cc_ordered(p.y); q[2] = cc_ordered(p.z);
    }
    bool mine = lab >= 0;
    for (int round = 0; round < 4; round++) {
      const unsigned long long live = __ballot(mine);
      if (!live) break;
      const int l = __shfl(lab, __ffsll((long long)live) - 1, CC_WAVE);
      if (l != cur0) {
        if (l == cur1) {
          const CcAcc t = acc0; acc0 = acc1; acc1 = t;
          cur1 = cur0;
        } else {
          if (cur1 >= 0) cc_flush(table, cur1, acc1);
          acc1 = acc0; cur1 = cur0;
          acc0.clear();
        }
        cur0 = l;
      }
      if (mine && lab == l) { acc0.add(q); mine = false; }
    }
    if (mine) { CcAcc one; one.clear(); one.add(q); cc_row_add(table, lab, one); }
  }
  acc0 = cc_wave_reduce(acc0);
  acc1 = cc_wave_reduce(acc1);
  if (lane == 0) {
    const int w = threadIdx.x / CC_WAVE;
    shLab[2 * w] = acc0.n > 0 ? cur0 : -1; shAcc[2 * w] = acc0;
    shLab[2 * w + 1] = acc1.n > 0 ? cur1 : -1; shAcc[2 * w + 1] = acc1;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int e = 0; e < 2 * CC_WAVES; e++) {
      const int l = shLab[e];
      if (l < 0) continue;
      CcAcc a = shAcc[e];
      for (int f = e + 1; f < 2 * CC_WAVES; f++) {
        if (shLab[f] != l) continue;
        shLab[f] = -1;
        const CcAcc b = shAcc[f];
        a.n += b.n;
        for (int k = 0; k < 3; k++) { a.mn[k] = min(a.mn[k], b.mn[k]); a.mx[k] = max(a.mx[k], b.mx[k]); }
      }
      cc_row_add(table, l, a);
    }
  }
}

__global__ __launch_bounds__(SPH_BLOCK) void k_cc_table_fin(int C, int32_t* table) {
  const int c = blockIdx.x * SPH_BLOCK + threadIdx.x;
  if (c >= C) return;
  int32_t* row = table + (size_t)c * CC_TABLE_WORDS;
#pragma unroll
  for (int k = 2; k < CC_TABLE_WORDS; k++) row[k] = __float_as_int(cc_unordered(row[k]) + 0.0f);
}

// ---- launchers ---------------------------------------------------------------------------------------------------------------
// The steps that do not depend on what the nodes and edges are, for sph_shells.hip too (N nodes, N >= 0; parent[x] < 0: no node).
int sphk_uf_compress(sph_solver* s, int N, int32_t* parent, uint32_t* err) {
  if (N <= 0) return SPH_OK;
  hipLaunchKernelGGL(k_cc_compress, dim3(sph_blocks(N)), dim3(SPH_BLOCK), 0, s->stream, N, parent, err);
  SPH_HIP(hipGetLastError());
  return SPH_OK;
}

int sphk_uf_flatten_count(sph_solver* s, int N, int32_t* parent, void* blockTot, uint32_t* off, uint32_t* err, uint32_t* totals) {
  const int nb = N > 0 ? sph_blocks(N) : 1;
  if (N > 0) {
    hipLaunchKernelGGL(k_cc_flatten, dim3(nb), dim3(SPH_BLOCK), 0, s->stream, N, parent, err);
    SPH_HIP(hipGetLastError());
  }
  hipLaunchKernelGGL(k_cc_flags, dim3(nb), dim3(SPH_BLOCK), 0, s->stream, N, (const int32_t*)parent, (uint2*)blockTot);
  SPH_HIP(hipGetLastError());
  hipLaunchKernelGGL(k_cc_scan, dim3(1), dim3(CC_SCAN_THREADS), 0, s->stream, (const uint2*)blockTot, nb, off, (const uint32_t*)err, totals);
  SPH_HIP(hipGetLastError());
  return SPH_OK;
}

int sphk_uf_label(sph_solver* s, int N, const int32_t* parent, int32_t* labels) {
  if (N <= 0) return SPH_OK;
  hipLaunchKernelGGL(k_cc_label, dim3(sph_blocks(N)), dim3(SPH_BLOCK), 0, s->stream, N, parent, labels);
  SPH_HIP(hipGetLastError());
  return SPH_OK;
}

static size_t cc_align(size_t b) { return (b + 255) & ~(size_t)255; }

// scratch layout: parent[N] | labels[N] | blockTot[nb] (uint2) | off[nb] | {err, pad} | totals[4]
struct CcLayout {
  size_t parent, labels, blockTot, off, err, totals, bytes;
  int nb;
};
static CcLayout cc_layout(int N) {
  CcLayout L;
  L.nb = N > 0 ? sph_blocks(N) : 1;
  size_t at = 0;
  L.parent = at; at += cc_align(sizeof(int32_t) * (size_t)std::max(N, 1));
  L.labels = at; at += cc_align(sizeof(int32_t) * (size_t)std::max(N, 1));
  L.blockTot = at; at += cc_align(sizeof(uint2) * (size_t)L.nb);
  L.off = at; at += cc_align(sizeof(uint32_t) * (size_t)L.nb);
  L.err = at; at += 256;
  L.totals = at; at += 256;
  L.bytes = at;
  return L;
}

size_t sphk_components_scratch_bytes(int N) { return cc_layout(N).bytes; }
int32_t* sphk_components_labels(void* scratch, int N) { return (int32_t*)((char*)scratch + cc_layout(N).labels); }

int sphk_components_link(sph_solver* s, uint32_t typeMask, bool finite, float link2, void* scratch, uint32_t** totals) {
  const int N = s->d.N;
  const CcLayout L = cc_layout(N);
  char* base = (char*)scratch;
  int32_t* parent = (int32_t*)(base + L.parent);
  uint32_t* err = (uint32_t*)(base + L.err);
  SPH_HIP(hipMemsetAsync(err, 0, 256, s->stream));
  const int nb = L.nb;
  if (N > 0) {
    hipLaunchKernelGGL(k_cc_init, dim3(nb), dim3(SPH_BLOCK), 0, s->stream, s->d, typeMask, parent);
    SPH_HIP(hipGetLastError());
    if (finite) hipLaunchKernelGGL(k_cc_prelink<true>, dim3(nb), dim3(SPH_BLOCK), 0, s->stream, s->d, link2, parent);
    else hipLaunchKernelGGL(k_cc_prelink<false>, dim3(nb), dim3(SPH_BLOCK), 0, s->stream, s->d, link2, parent);
    SPH_HIP(hipGetLastError());
    const int rc = sphk_uf_compress(s, N, parent, err);
    if (rc != SPH_OK) return rc;
    if (finite) hipLaunchKernelGGL(k_cc_hook<true>, dim3(nb), dim3(SPH_BLOCK), 0, s->stream, s->d, link2, parent, err);
    else hipLaunchKernelGGL(k_cc_hook<false>, dim3(nb), dim3(SPH_BLOCK), 0, s->stream, s->d, link2, parent, err);
    SPH_HIP(hipGetLastError());
  }
  *totals = (uint32_t*)(base + L.totals);
  return sphk_uf_flatten_count(s, N, parent, base + L.blockTot, (uint32_t*)(base + L.off), err, *totals);
}

int sphk_components_number(sph_solver* s, void* scratch, int C, int32_t* table) {
  const int N = s->d.N;
  if (N <= 0) return SPH_OK;
  const CcLayout L = cc_layout(N);
  char* base = (char*)scratch;
  const int32_t* parent = (const int32_t*)(base + L.parent);
  int32_t* labels = (int32_t*)(base + L.labels);
  hipLaunchKernelGGL(k_cc_rank, dim3(L.nb), dim3(SPH_BLOCK), 0, s->stream, N, parent, (const uint32_t*)(base + L.off), labels, table);
  SPH_HIP(hipGetLastError());
  const int rc = sphk_uf_label(s, N, parent, labels);
  if (rc != SPH_OK) return rc;
  if (C <= 0) return SPH_OK;
  // 4096 particles per wave where there are enough of them to fill the device, never less than one wave step
  int perWave = 4096;
  while (perWave > CC_WAVE && (long long)N / perWave < 4096) perWave >>= 1;
  const long long waves = ((long long)N + perWave - 1) / perWave;
  const int blocks = (int)((waves + CC_WAVES - 1) / CC_WAVES);
  hipLaunchKernelGGL(k_cc_table, dim3(blocks), dim3(SPH_BLOCK), 0, s->stream, s->d, (const int32_t*)labels, table, perWave);
  SPH_HIP(hipGetLastError());
  hipLaunchKernelGGL(k_cc_table_fin, dim3(sph_blocks(C)), dim3(SPH_BLOCK), 0, s->stream, C, table);
  SPH_HIP(hipGetLastError());
  return SPH_OK;
}

// Measures of the extracted surface (include/sphmi.h: sph_measure_surface / sph_read_shells): the shells the mesh
// consists of, their open sides, and per shell the exact integer sums of area, signed volume and area moment. Read-only on the
// mesh and on every solver array. Nodes = the V vertex ids, edges = the three sides of every triangle.
//   k_sh_init       parent[v] = v, side[v] = 0
//   k_sh_prelink    one lane per triangle: an atomic minimum of each side's lower end into the higher end's parent (a forest
//                   already: parent[x] <= x, same set), and side[corner] += next - prev for the three corners
//   (compress)      pointer jumping on that forest (sphk_uf_compress, sph_components.hip)
//   k_sh_hook       one lane per triangle hooks (a, b) and (a, c): the lock-free union-find of sph_union_find.h. Every side is
//                   processed here, so the labelling does not rest on the prelink
//   (flatten, flags, scan)  sphk_uf_flatten_count: parent[v] = root, the roots per block, their offsets, the totals for the host
//   k_sh_rank       roots: labels[r] = rank of r among the roots; opens the shell's row and box
//   (label)         sphk_uf_label
//   k_sh_vertices   vertices, open sides and box per shell
//   k_sh_triangles  triangles, bad triangles and the five quantised sums per shell
//   k_sh_fin        the boxes back from their integer images to floats (+ 0.0f); closed shells, open sides, bad triangles in total
// Open sides: around an interior vertex of an oriented manifold the triangles' (next - prev) telescope to 0; a border vertex has
// one unmatched outgoing side, and its sum is the difference of two different vertex ids. So side[v] != 0 marks the start of an
// open side (tests/shell_ref.py holds the definition it is compared against).
// Both table kernels combine before they touch memory: a wave reduces, label by label, the lanes that share the label of its
// first live lane (integers: any order is exact), adds the result to one of SH_SLOTS rows in LDS, and the block ends with one set
// of atomics per used row. Triangles and vertices follow the cells, so a block of 4096 sees few shells; labels beyond the slots
// go to memory per wave and label. No floating-point atomics.
#include "sph_common.h"
#include "sph_union_find.h"

#include <algorithm>

#define SH_SLOTS 8
#define SH_TRI_SUMS 7  // row words 2 (triangles), 4 (bad), 5..9 (a2, d6, mx, my, mz)
#define SH_BOX_WORDS 6

typedef unsigned long long sh_u64;

__global__ __launch_bounds__(SPH_BLOCK) void k_sh_init(int V, int32_t* __restrict__ parent, long long* __restrict__ side) {
  const int v = blockIdx.x * SPH_BLOCK + threadIdx.x;
  if (v >= V) return;
  parent[v] = v;
  side[v] = 0;
}

// the three corners of triangle t, or false (and an error flag) if one is not a vertex id
__device__ __forceinline__ bool sh_corners(const int32_t* __restrict__ tris, int t, int V, int& a, int& b, int& c, uint32_t* err) {
  const int32_t* q = tris + 3 * (size_t)t;
  a = q[0]; b = q[1]; c = q[2];
  if ((unsigned)a >= (unsigned)V || (unsigned)b >= (unsigned)V || (unsigned)c >= (unsigned)V) { atomicOr(err, 16u); return false; }
  return true;
}

__device__ __forceinline__ void sh_min_link(int32_t* parent, int x, int y) {
  const int hi = x > y ? x : y, lo = x > y ? y : x;
  if (hi != lo) __hip_atomic_fetch_min(parent + hi, lo, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ __launch_bounds__(SPH_BLOCK) void k_sh_prelink(int T, int V, const int32_t* __restrict__ tris, int32_t* parent, long long* side,
                                                          uint32_t* err) {
  const int t = xcd_block(gridDim.x) * SPH_BLOCK + threadIdx.x;
  if (t >= T) return;
  int a, b, c;
  if (!sh_corners(tris, t, V, a, b, c, err)) return;
  sh_min_link(parent, a, b);
  sh_min_link(parent, b, c);
  sh_min_link(parent, c, a);
  atomicAdd((sh_u64*)side + a, (sh_u64)((long long)b - (long long)c));
  atomicAdd((sh_u64*)side + b, (sh_u64)((long long)c - (long long)a));
  atomicAdd((sh_u64*)side + c, (sh_u64)((long long)a - (long long)b));
}

__global__ __launch_bounds__(SPH_BLOCK) void k_sh_hook(int T, int V, const int32_t* __restrict__ tris, int32_t* parent, uint32_t* err) {
  const int t = xcd_block(gridDim.x) * SPH_BLOCK + threadIdx.x;
  if (t >= T) return;
  int a, b, c;
  if (!sh_corners(tris, t, V, a, b, c, err)) return;
  const int mine = cc_union(parent, a, b, V, err);
  cc_union(parent, mine, c, V, err);
}

__global__ __launch_bounds__(SPH_BLOCK) void k_sh_rank(int V, const int32_t* __restrict__ parent, const uint32_t* __restrict__ off,
                                                       int32_t* __restrict__ labels, long long* __restrict__ table, int32_t* __restrict__ box) {
  const int j = blockIdx.x * SPH_BLOCK + threadIdx.x;
  const bool root = j < V && parent[j] == j;
  uint32_t total;
  const uint32_t rank = off[blockIdx.x] + cc_block_exclusive(root ? 1u : 0u, total);
  if (!root) return;
  labels[j] = (int32_t)rank;
  long long* row = table + (size_t)rank * SPH_SHELL_WORDS;
  row[0] = j;
#pragma unroll
  for (int w = 1; w < SPH_SHELL_WORDS; w++) row[w] = 0;
  int32_t* bx = box + (size_t)rank * SH_BOX_WORDS;
  bx[0] = bx[1] = bx[2] = 0x7fffffff;
  bx[3] = bx[4] = bx[5] = (int32_t)0x80000000;
}

// ---- the block's rows in LDS
// the slot of label l (claimed on first use), or -1 when SH_SLOTS other labels hold them all
__device__ __forceinline__ int sh_slot(int* slotLab, int l) {
  for (int k = 0; k < SH_SLOTS; k++) {
    const int seen = atomicCAS(slotLab + k, -1, l);
    if (seen == -1 || seen == l) return k;
  }
  return -1;
}

__device__ __forceinline__ long long sh_wave_sum(long long v) {
#pragma unroll
  for (int s = 32; s >= 1; s >>= 1) v += __shfl_xor(v, s, CC_WAVE);
  return v;
}
__device__ __forceinline__ int sh_wave_min(int v) {
#pragma unroll
  for (int s = 32; s >= 1; s >>= 1) v = min(v, __shfl_xor(v, s, CC_WAVE));
  return v;
}
__device__ __forceinline__ int sh_wave_max(int v) {
#pragma unroll
  for (int s = 32; s >= 1; s >>= 1) v = max(v, __shfl_xor(v, s, CC_WAVE));
  return v;
}

// Each block owns `perBlock` consecutive vertices (a multiple of SPH_BLOCK); its waves take them 64 at a time.
__global__ __launch_bounds__(SPH_BLOCK) void k_sh_vertices(int V, const float* __restrict__ verts, const int32_t* __restrict__ labels,
                                                           const long long* __restrict__ side, long long* table, int32_t* box, int perBlock) {
  __shared__ int slotLab[SH_SLOTS];
  __shared__ sh_u64 slotSum[SH_SLOTS][2];
  __shared__ int slotBox[SH_SLOTS][SH_BOX_WORDS];
  if (threadIdx.x < SH_SLOTS) {
    const int k = threadIdx.x;
    slotLab[k] = -1;
    slotSum[k][0] = slotSum[k][1] = 0;
    slotBox[k][0] = slotBox[k][1] = slotBox[k][2] = 0x7fffffff;
    slotBox[k][3] = slotBox[k][4] = slotBox[k][5] = (int)0x80000000;
  }
  __syncthreads();
  const int lane = threadIdx.x & (CC_WAVE - 1);
  const long long first = (long long)blockIdx.x * perBlock;
  const int end = (int)min((long long)V, first + perBlock);
  for (long long v0 = first + (threadIdx.x - lane); v0 < end; v0 += SPH_BLOCK) {
    const int v = (int)v0 + lane;
    bool live = v < end;
    int lab = -1, open = 0, q[3] = {0, 0, 0};
    if (live) {
      lab = labels[v];
      open = side[v] != 0 ? 1 : 0;
      const float* p = verts + 3 * (size_t)v;
      q[0] = cc_ordered(p[0]); q[1] = cc_ordered(p[1]); q[2] = cc_ordered(p[2]);
    }
    for (;;) {
      const sh_u64 m = __ballot(live);
      if (!m) break;
      const int l = __shfl(lab, __ffsll((long long)m) - 1, CC_WAVE);
      const bool in = live && lab == l;
      const long long n = sh_wave_sum(in ? 1 : 0), o = sh_wave_sum(in ? open : 0);
      int mn[3], mx[3];
#pragma unroll
      for (int k = 0; k < 3; k++) { mn[k] = sh_wave_min(in ? q[k] : 0x7fffffff); mx[k] = sh_wave_max(in ? q[k] : (int)0x80000000); }
      if (lane == 0) {
        const int k = sh_slot(slotLab, l);
        sh_u64* sums = k >= 0 ? slotSum[k] : (sh_u64*)(table + (size_t)l * SPH_SHELL_WORDS);
        int* bx = k >= 0 ? slotBox[k] : box + (size_t)l * SH_BOX_WORDS;
        atomicAdd(sums + (k >= 0 ? 0 : 1), (sh_u64)n);
        if (o) atomicAdd(sums + (k >= 0 ? 1 : 3), (sh_u64)o);
#pragma unroll
        for (int c = 0; c < 3; c++) { atomicMin(bx + c, mn[c]); atomicMax(bx + 3 + c, mx[c]); }
      }
      live = live && !in;
    }
  }
  __syncthreads();
  if (threadIdx.x < SH_SLOTS && slotLab[threadIdx.x] >= 0) {
    const int k = threadIdx.x, l = slotLab[k];
    sh_u64* row = (sh_u64*)(table + (size_t)l * SPH_SHELL_WORDS);
    atomicAdd(row + 1, slotSum[k][0]);
    if (slotSum[k][1]) atomicAdd(row + 3, slotSum[k][1]);
#pragma unroll
    for (int c = 0; c < 3; c++) { atomicMin(box + (size_t)l * SH_BOX_WORDS + c, slotBox[k][c]); atomicMax(box + (size_t)l * SH_BOX_WORDS + 3 + c, slotBox[k][3 + c]); }
  }
}

// row word of triangle sum w
__device__ __forceinline__ int sh_tri_word(int w) { return w == 0 ? 2 : w == 1 ? 4 : 3 + w; }

// x * 2^k, whether it is below the limit in magnitude (a NaN is not), and its nearest integer (ties to even)
__device__ __forceinline__ bool sh_quantise(double x, int k, double limit, long long& q) {
  const double s = ldexp(x, k);
  const bool ok = fabs(s) < limit;
  q = ok ? llrint(s) : 0;
  return ok;
}

__global__ __launch_bounds__(SPH_BLOCK) void k_sh_triangles(ShellArgs a, const int32_t* __restrict__ labels, long long* table, int perBlock) {
  __shared__ int slotLab[SH_SLOTS];
  __shared__ sh_u64 slotSum[SH_SLOTS][SH_TRI_SUMS];
  if (threadIdx.x < SH_SLOTS) {
    slotLab[threadIdx.x] = -1;
#pragma unroll
    for (int w = 0; w < SH_TRI_SUMS; w++) slotSum[threadIdx.x][w] = 0;
  }
  __syncthreads();
  const int lane = threadIdx.x & (CC_WAVE - 1);
  const long long first = (long long)blockIdx.x * perBlock;
  const int end = (int)min((long long)a.T, first + perBlock);
  for (long long t0 = first + (threadIdx.x - lane); t0 < end; t0 += SPH_BLOCK) {
    const int t = (int)t0 + lane;
    bool live = t < end;
    int lab = -1;
    long long term[SH_TRI_SUMS] = {0, 0, 0, 0, 0, 0, 0};
    if (live) {
      const int32_t* c = a.tris + 3 * (size_t)t;
      const int i0 = c[0], i1 = c[1], i2 = c[2];
      lab = labels[i0];
      double p0[3], p1[3], p2[3];
#pragma unroll
      for (int k = 0; k < 3; k++) {
        p0[k] = (double)a.verts[3 * (size_t)i0 + k] - a.origin[k];
        p1[k] = (double)a.verts[3 * (size_t)i1 + k] - a.origin[k];
        p2[k] = (double)a.verts[3 * (size_t)i2 + k] - a.origin[k];
      }
      const double e1x = p1[0] - p0[0], e1y = p1[1] - p0[1], e1z = p1[2] - p0[2];
      const double e2x = p2[0] - p0[0], e2y = p2[1] - p0[1], e2z = p2[2] - p0[2];
      const double nx = e1y * e2z - e1z * e2y, ny = e1z * e2x - e1x * e2z, nz = e1x * e2y - e1y * e2x;
      const double a2 = sqrt((nx * nx + ny * ny) + nz * nz);
      const double d6 = (p0[0] * nx + p0[1] * ny) + p0[2] * nz;
      long long q[5];
      bool ok = sh_quantise(a2, a.kA, a.limit, q[0]);
      ok = sh_quantise(d6, a.kV, a.limit, q[1]) && ok;
#pragma unroll
      for (int k = 0; k < 3; k++) ok = sh_quantise(a2 * ((p0[k] + p1[k]) + p2[k]), a.kM, a.limit, q[2 + k]) && ok;
      term[0] = 1;
      term[1] = ok ? 0 : 1;
#pragma unroll
      for (int k = 0; k < 5; k++) term[2 + k] = ok ? q[k] : 0;
    }
    for (;;) {
      const sh_u64 m = __ballot(live);
      if (!m) break;
      const int l = __shfl(lab, __ffsll((long long)m) - 1, CC_WAVE);
      const bool in = live && lab == l;
      long long sum[SH_TRI_SUMS];
#pragma unroll
      for (int w = 0; w < SH_TRI_SUMS; w++) sum[w] = sh_wave_sum(in ? term[w] : 0);
      if (lane == 0) {
        const int k = sh_slot(slotLab, l);
        sh_u64* row = (sh_u64*)(table + (size_t)l * SPH_SHELL_WORDS);
#pragma unroll
        for (int w = 0; w < SH_TRI_SUMS; w++) {
          if (!sum[w]) continue;
          if (k >= 0) atomicAdd(&slotSum[k][w], (sh_u64)sum[w]);
          else atomicAdd(row + sh_tri_word(w), (sh_u64)sum[w]);
        }
      }
      live = live && !in;
    }
  }
  __syncthreads();
  if (threadIdx.x < SH_SLOTS && slotLab[threadIdx.x] >= 0) {
    sh_u64* row = (sh_u64*)(table + (size_t)slotLab[threadIdx.x] * SPH_SHELL_WORDS);
#pragma unroll
    for (int w = 0; w < SH_TRI_SUMS; w++)
      if (slotSum[threadIdx.x][w]) atomicAdd(row + sh_tri_word(w), slotSum[threadIdx.x][w]);
  }
}

__global__ __launch_bounds__(SPH_BLOCK) void k_sh_fin(int S, const long long* __restrict__ table, int32_t* __restrict__ box, sh_u64* totals) {
  const int c = blockIdx.x * SPH_BLOCK + threadIdx.x;
  long long closed = 0, open = 0, bad = 0;
  if (c < S) {
    int32_t* bx = box + (size_t)c * SH_BOX_WORDS;
#pragma unroll
    for (int k = 0; k < SH_BOX_WORDS; k++) bx[k] = __float_as_int(cc_unordered(bx[k]) + 0.0f);
    const long long* row = table + (size_t)c * SPH_SHELL_WORDS;
    open = row[3];
    bad = row[4];
    closed = open == 0 ? 1 : 0;
  }
  closed = sh_wave_sum(closed); open = sh_wave_sum(open); bad = sh_wave_sum(bad);
  if ((threadIdx.x & (CC_WAVE - 1)) == 0) {
    if (closed) atomicAdd(totals + 0, (sh_u64)closed);
    if (open) atomicAdd(totals + 1, (sh_u64)open);
    if (bad) atomicAdd(totals + 2, (sh_u64)bad);
  }
}

// ---- launchers ---------------------------------------------------------------------------------------------------------------
static size_t sh_align(size_t b) { return (b + 255) & ~(size_t)255; }

// scratch layout: parent[V] | labels[V] | side[V] (int64) | blockTot[nb] (uint2) | off[nb] | {err, pad} | totals[4]
struct ShLayout {
  size_t parent, labels, side, blockTot, off, err, totals, bytes;
  int nb;
};
static ShLayout sh_layout(int V) {
  ShLayout L;
  L.nb = V > 0 ? sph_blocks(V) : 1;
  const size_t n = (size_t)std::max(V, 1);
  size_t at = 0;
  L.parent = at; at += sh_align(sizeof(int32_t) * n);
  L.labels = at; at += sh_align(sizeof(int32_t) * n);
  L.side = at; at += sh_align(sizeof(long long) * n);
  L.blockTot = at; at += sh_align(sizeof(uint2) * (size_t)L.nb);
  L.off = at; at += sh_align(sizeof(uint32_t) * (size_t)L.nb);
  L.err = at; at += 256;
  L.totals = at; at += 256;
  L.bytes = at;
  return L;
}

// table layout: rows[S][SPH_SHELL_WORDS] (int64) | box[S][6] | totals[3] (int64)
static size_t sh_box_at(int S) { return sh_align(sizeof(long long) * SPH_SHELL_WORDS * (size_t)std::max(S, 1)); }
static size_t sh_totals_at(int S) { return sh_box_at(S) + sh_align(sizeof(int32_t) * SH_BOX_WORDS * (size_t)std::max(S, 1)); }

size_t sphk_shells_scratch_bytes(int V) { return sh_layout(V).bytes; }
int32_t* sphk_shells_labels(void* scratch, int V) { return (int32_t*)((char*)scratch + sh_layout(V).labels); }
size_t sphk_shells_table_bytes(int S) { return sh_totals_at(S) + 256; }
float* sphk_shells_bbox(void* table, int S) { return (float*)((char*)table + sh_box_at(S)); }
int64_t* sphk_shells_totals(void* table, int S) { return (int64_t*)((char*)table + sh_totals_at(S)); }

int sphk_shells_link(sph_solver* s, const ShellArgs& a, void* scratch, uint32_t** totals) {
  const ShLayout L = sh_layout(a.V);
  char* base = (char*)scratch;
  int32_t* parent = (int32_t*)(base + L.parent);
  uint32_t* err = (uint32_t*)(base + L.err);
  SPH_HIP(hipMemsetAsync(err, 0, 256, s->stream));
  if (a.V > 0) {
    hipLaunchKernelGGL(k_sh_init, dim3(L.nb), dim3(SPH_BLOCK), 0, s->stream, a.V, parent, (long long*)(base + L.side));
    SPH_HIP(hipGetLastError());
  }
  if (a.V > 0 && a.T > 0) {
    const int tb = sph_blocks(a.T);
    hipLaunchKernelGGL(k_sh_prelink, dim3(tb), dim3(SPH_BLOCK), 0, s->stream, a.T, a.V, a.tris, parent, (long long*)(base + L.side), err);
    SPH_HIP(hipGetLastError());
    const int rc = sphk_uf_compress(s, a.V, parent, err);
    if (rc != SPH_OK) return rc;
    hipLaunchKernelGGL(k_sh_hook, dim3(tb), dim3(SPH_BLOCK), 0, s->stream, a.T, a.V, a.tris, parent, err);
    SPH_HIP(hipGetLastError());
  }
  *totals = (uint32_t*)(base + L.totals);
  return sphk_uf_flatten_count(s, a.V, parent, base + L.blockTot, (uint32_t*)(base + L.off), err, *totals);
}

// items per block of the table kernels: 4096 where that still fills the device, never less than one block step
static int sh_per_block(int n) {
  int per = 4096;
  while (per > SPH_BLOCK && n / per < 512) per >>= 1;
  return per;
}

int sphk_shells_number(sph_solver* s, const ShellArgs& a, void* scratch, int S, void* table) {
  sh_u64* totals = (sh_u64*)sphk_shells_totals(table, S);
  SPH_HIP(hipMemsetAsync(totals, 0, 256, s->stream));
  if (a.V <= 0 || S <= 0) return SPH_OK;
  const ShLayout L = sh_layout(a.V);
  char* base = (char*)scratch;
  const int32_t* parent = (const int32_t*)(base + L.parent);
  int32_t* labels = (int32_t*)(base + L.labels);
  long long* rows = (long long*)table;
  int32_t* box = (int32_t*)sphk_shells_bbox(table, S);
  hipLaunchKernelGGL(k_sh_rank, dim3(L.nb), dim3(SPH_BLOCK), 0, s->stream, a.V, parent, (const uint32_t*)(base + L.off), labels, rows, box);
  SPH_HIP(hipGetLastError());
  const int rc = sphk_uf_label(s, a.V, parent, labels);
  if (rc != SPH_OK) return rc;
  const int perV = sh_per_block(a.V);
  hipLaunchKernelGGL(k_sh_vertices, dim3(sph_blocks(a.V, perV)), dim3(SPH_BLOCK), 0, s->stream, a.V, a.verts, (const int32_t*)labels,
                     (const long long*)(base + L.side), rows, box, perV);
  SPH_HIP(hipGetLastError());
  if (a.T > 0) {
    const int perT = sh_per_block(a.T);
    hipLaunchKernelGGL(k_sh_triangles, dim3(sph_blocks(a.T, perT)), dim3(SPH_BLOCK), 0, s->stream, a, (const int32_t*)labels, rows, perT);
    SPH_HIP(hipGetLastError());
  }
  hipLaunchKernelGGL(k_sh_fin, dim3(sph_blocks(S)), dim3(SPH_BLOCK), 0, s->stream, S, (const long long*)rows, box, totals);
  SPH_HIP(hipGetLastError());
  return SPH_OK;
}

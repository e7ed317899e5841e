// Isosurface extraction: marching cubes over a sampled scalar lattice (include/sphmi.h: sph_extract_surface).
// Read-only on every solver array. The host side (sph_api.hip) fills the lattice through sphk_sample_grid in z-chunks, then:
//   k_surface_field      word `field` of a chunk's records -> the scalar lattice (4 B per point)
//   k_surface_classify   one lane per lattice point: its crossed-edge mask (+x, +y, +z) and the case of the cell it is the lower
//                        corner of, packed into 2 B; per-block vertex and triangle totals
//   k_surface_scan       one workgroup: exclusive 64-bit offsets of the block totals and the grand totals (no atomics: the
//                        output order is the contract's)
//   k_surface_vertices   each point's first vertex id (4 B per point) and its vertices' positions
//   k_surface_triangles  each cell's triangles from the case table; a cube edge's vertex id is its owning point's first id plus
//                        the crossed edges of that point along lower axes
// Vertex and triangle numbering follow the x-fastest point order because every block's offset is the exclusive sum of the
// blocks before it and lanes number their own items by an in-block exclusive scan.
#include "sph_common.h"

#define SPH_MC_TABLE_QUALIFIER static __constant__ const
#include "sph_mc_table.h"

#define SURF_WAVE 64
#define SURF_WAVES (SPH_BLOCK / SURF_WAVE)
#define SURF_SCAN_THREADS 1024

// Exclusive prefix of v over the block's lanes (lane order = point order) and the block total. Wave64 shuffles, then LDS
// across the block's waves.
__device__ __forceinline__ uint32_t block_exclusive(uint32_t v, uint32_t& total) {
  __shared__ uint32_t waveSum[SURF_WAVES];
  const int lane = threadIdx.x & (SURF_WAVE - 1), wave = threadIdx.x / SURF_WAVE;
  uint32_t inc = v;
  for (int o = 1; o < SURF_WAVE; o <<= 1) {
    const uint32_t u = (uint32_t)__shfl_up((int)inc, o, SURF_WAVE);
    if (lane >= o) inc += u;
  }
  if (lane == SURF_WAVE - 1) waveSum[wave] = inc;
  __syncthreads();
  uint32_t before = 0, all = 0;
#pragma unroll
  for (int w = 0; w < SURF_WAVES; w++) {
    const uint32_t s = waveSum[w];
    if (w < wave) before += s;
    all += s;
  }
  total = all;
  __syncthreads();  // waveSum may be reused by a second call
  return before + inc - v;
}

__global__ __launch_bounds__(SPH_BLOCK) void k_surface_field(const float* __restrict__ records, int word, int n,
                                                             float* __restrict__ field) {
  const int i = blockIdx.x * SPH_BLOCK + threadIdx.x;
  if (i < n) field[i] = records[(size_t)i * SPH_SAMPLE_WORDS + word];
}

struct SurfLattice {
  int nx, ny, nz, P;  // P = nx * ny * nz <= 2^31 - 1
  float iso;
};

// inside = f >= iso (a NaN is outside)
__device__ __forceinline__ uint32_t surf_in(const float* f, int p, float iso) { return f[p] >= iso ? 1u : 0u; }

// code = crossed-edge mask (bit a: the edge from this point along axis a) | case of the cell whose lower corner this is << 3
__global__ __launch_bounds__(SPH_BLOCK) void k_surface_classify(const float* __restrict__ f, SurfLattice L,
                                                                uint16_t* __restrict__ code, uint2* __restrict__ blockTot) {
  const int p = blockIdx.x * SPH_BLOCK + threadIdx.x;
  uint32_t nv = 0, nt = 0;
  if (p < L.P) {
    const int plane = L.nx * L.ny;
    const int k = p / plane, rem = p - k * plane, j = rem / L.nx, i = rem - j * L.nx;
    const bool ex = i + 1 < L.nx, ey = j + 1 < L.ny, ez = k + 1 < L.nz;
    const uint32_t c0 = surf_in(f, p, L.iso);
    const uint32_t cx = ex ? surf_in(f, p + 1, L.iso) : c0;
    const uint32_t cy = ey ? surf_in(f, p + L.nx, L.iso) : c0;
    const uint32_t cz = ez ? surf_in(f, p + plane, L.iso) : c0;
    const uint32_t mask = (c0 ^ cx) | ((c0 ^ cy) << 1) | ((c0 ^ cz) << 2);
    uint32_t cse = 0;
    if (ex && ey && ez) {
      cse = c0 | (cx << 1) | (cy << 2) | (surf_in(f, p + L.nx + 1, L.iso) << 3) | (cz << 4) | (surf_in(f, p + plane + 1, L.iso) << 5) |
            (surf_in(f, p + plane + L.nx, L.iso) << 6) | (surf_in(f, p + plane + L.nx + 1, L.iso) << 7);
    }
    code[p] = (uint16_t)(mask | (cse << 3));
    nv = __popc(mask);
    nt = kMcTriCount[cse];
  }
  uint32_t totV, totT;
  block_exclusive(nv, totV);
  block_exclusive(nt, totT);
  if (threadIdx.x == 0) blockTot[blockIdx.x] = make_uint2(totV, totT);
}

// offsets[b] = sum of the totals of blocks < b (x: vertices, y: triangles), totals = grand totals. One workgroup: each thread
// sums a contiguous run of blocks, the run sums are scanned in LDS, then each thread writes its run's offsets.
__global__ __launch_bounds__(SURF_SCAN_THREADS) void k_surface_scan(const uint2* __restrict__ blockTot, int nb,
                                                                   unsigned long long* __restrict__ offV,
                                                                   unsigned long long* __restrict__ offT,
                                                                   unsigned long long* __restrict__ totals) {
  __shared__ unsigned long long sV[SURF_SCAN_THREADS], sT[SURF_SCAN_THREADS];
  const int tid = threadIdx.x;
  const int per = (nb + SURF_SCAN_THREADS - 1) / SURF_SCAN_THREADS;
  const int b0 = min(tid * per, nb), b1 = min(b0 + per, nb);
  unsigned long long v = 0, t = 0;
  for (int b = b0; b < b1; b++) { const uint2 x = blockTot[b]; v += x.x; t += x.y; }
  sV[tid] = v; sT[tid] = t;
  __syncthreads();
  for (int off = 1; off < SURF_SCAN_THREADS; off <<= 1) {  // inclusive Hillis-Steele scan
    unsigned long long av = 0, at = 0;
    if (tid >= off) { av = sV[tid - off]; at = sT[tid - off]; }
    __syncthreads();
    sV[tid] += av; sT[tid] += at;
    __syncthreads();
  }
  unsigned long long ov = sV[tid] - v, ot = sT[tid] - t;
  for (int b = b0; b < b1; b++) {
    const uint2 x = blockTot[b];
    offV[b] = ov; offT[b] = ot;
    ov += x.x; ot += x.y;
  }
  if (tid == SURF_SCAN_THREADS - 1) { totals[0] = sV[tid]; totals[1] = sT[tid]; }
}

struct SurfGeom {
  float o[3], s[3];
};

// Vertex of the edge from point (i, j, k) along `axis`: the lower point's coordinates with that axis' one replaced by
// x0 + t*(x1 - x0), t = (iso - f0)/(f1 - f0); x0, x1 = origin + (float)index * spacing. Float, no contraction (Makefile flags).
__global__ __launch_bounds__(SPH_BLOCK) void k_surface_vertices(const float* __restrict__ f, SurfLattice L, SurfGeom g,
                                                                const uint16_t* __restrict__ code,
                                                                const unsigned long long* __restrict__ offV,
                                                                uint32_t* __restrict__ vbase, float* __restrict__ verts) {
  const int p = blockIdx.x * SPH_BLOCK + threadIdx.x;
  const uint32_t mask = p < L.P ? (code[p] & 7u) : 0u;
  uint32_t tot;
  const uint32_t first = (uint32_t)offV[blockIdx.x] + block_exclusive(__popc(mask), tot);
  if (p >= L.P) return;
  vbase[p] = first;
  if (!mask) return;
  const int plane = L.nx * L.ny;
  const int k = p / plane, rem = p - k * plane, j = rem / L.nx, i = rem - j * L.nx;
  const int idx[3] = {i, j, k};
  const int step[3] = {1, L.nx, plane};
  float base[3];
#pragma unroll
  for (int a = 0; a < 3; a++) base[a] = g.o[a] + (float)idx[a] * g.s[a];
  const float f0 = f[p];
  uint32_t v = first;
#pragma unroll
  for (int a = 0; a < 3; a++) {
    if (!((mask >> a) & 1u)) continue;
    const float f1 = f[p + step[a]];
    const float t = (L.iso - f0) / (f1 - f0);
    const float x0 = base[a], x1 = g.o[a] + (float)(idx[a] + 1) * g.s[a];
    float q[3] = {base[0], base[1], base[2]};
    q[a] = x0 + t * (x1 - x0);
    float* out = verts + (size_t)v * 3;
    out[0] = q[0]; out[1] = q[1]; out[2] = q[2];
    v++;
  }
}

// Cube edge e (axis e/4, q = e%4) starts at the corner whose two other coordinates, in axis order, are (q&1, q>>1).
__device__ __forceinline__ int surf_edge_owner(int e, int p, int nx, int plane) {
  const int axis = e >> 2, q = e & 3, lo = q & 1, hi = q >> 1;
  if (axis == 0) return p + lo * nx + hi * plane;
  if (axis == 1) return p + lo + hi * plane;
  return p + lo + hi * nx;
}

__global__ __launch_bounds__(SPH_BLOCK) void k_surface_triangles(SurfLattice L, const uint16_t* __restrict__ code,
                                                                 const uint32_t* __restrict__ vbase,
                                                                 const unsigned long long* __restrict__ offT,
                                                                 int32_t* __restrict__ tris) {
  const int p = blockIdx.x * SPH_BLOCK + threadIdx.x;
  const uint32_t cse = p < L.P ? (uint32_t)(code[p] >> 3) : 0u;
  const uint32_t nt = kMcTriCount[cse];
  uint32_t tot;
  const unsigned long long first = offT[blockIdx.x] + block_exclusive(nt, tot);
  if (!nt) return;
  const int plane = L.nx * L.ny;
  int32_t* out = tris + (size_t)first * 3;
  for (uint32_t r = 0; r < 3 * nt; r++) {
    const int e = kMcTriEdges[cse][r];
    const int owner = surf_edge_owner(e, p, L.nx, plane);
    const uint32_t lower = code[owner] & ((1u << (e >> 2)) - 1u);
    out[r] = (int32_t)(vbase[owner] + __popc(lower));
  }
}

static size_t surf_align(size_t b) { return (b + 255) & ~(size_t)255; }

size_t sphk_surface_scratch_bytes(long long P) {
  const size_t nb = (size_t)((P + SPH_BLOCK - 1) / SPH_BLOCK);
  return surf_align(sizeof(float) * P) + surf_align(sizeof(uint16_t) * P) + surf_align(sizeof(uint32_t) * P) +
         surf_align(sizeof(uint2) * nb) + 2 * surf_align(sizeof(unsigned long long) * nb) + surf_align(2 * sizeof(unsigned long long));
}

// Carves the scratch (sphk_surface_scratch_bytes) into its arrays.
struct SurfScratch {
  float* field; uint16_t* code; uint32_t* vbase; uint2* blockTot; unsigned long long *offV, *offT, *totals;
};
static SurfScratch surf_carve(void* buf, long long P) {
  const size_t nb = (size_t)((P + SPH_BLOCK - 1) / SPH_BLOCK);
  char* c = (char*)buf;
  SurfScratch r;
  r.field = (float*)c; c += surf_align(sizeof(float) * P);
  r.code = (uint16_t*)c; c += surf_align(sizeof(uint16_t) * P);
  r.vbase = (uint32_t*)c; c += surf_align(sizeof(uint32_t) * P);
  r.blockTot = (uint2*)c; c += surf_align(sizeof(uint2) * nb);
  r.offV = (unsigned long long*)c; c += surf_align(sizeof(unsigned long long) * nb);
  r.offT = (unsigned long long*)c; c += surf_align(sizeof(unsigned long long) * nb);
  r.totals = (unsigned long long*)c;
  return r;
}

int sphk_surface_field(sph_solver* s, const float* records, int word, int n, float* field) {
  if (n <= 0) return SPH_OK;
  hipLaunchKernelGGL(k_surface_field, dim3(sph_blocks(n)), dim3(SPH_BLOCK), 0, s->stream, records, word, n, field);
  SPH_HIP(hipGetLastError());
  return SPH_OK;
}

int sphk_surface_count(sph_solver* s, void* scratch, const int dims[3], float iso, unsigned long long* totalsHost) {
  const long long P = (long long)dims[0] * dims[1] * dims[2];
  const SurfScratch r = surf_carve(scratch, P);
  const SurfLattice L = {dims[0], dims[1], dims[2], (int)P, iso};
  const int nb = (int)((P + SPH_BLOCK - 1) / SPH_BLOCK);
  hipLaunchKernelGGL(k_surface_classify, dim3(nb), dim3(SPH_BLOCK), 0, s->stream, r.field, L, r.code, r.blockTot);
  hipLaunchKernelGGL(k_surface_scan, dim3(1), dim3(SURF_SCAN_THREADS), 0, s->stream, r.blockTot, nb, r.offV, r.offT, r.totals);
  SPH_HIP(hipGetLastError());
  SPH_HIP(hipMemcpyAsync(totalsHost, r.totals, 2 * sizeof(unsigned long long), hipMemcpyDeviceToHost, s->stream));
  SPH_HIP(hipStreamSynchronize(s->stream));
  return SPH_OK;
}

int sphk_surface_emit(sph_solver* s, void* scratch, const int dims[3], float iso, const float origin[3], const float spacing[3],
                      float* verts, int32_t* tris) {
  const long long P = (long long)dims[0] * dims[1] * dims[2];
  const SurfScratch r = surf_carve(scratch, P);
  const SurfLattice L = {dims[0], dims[1], dims[2], (int)P, iso};
  SurfGeom g;
  for (int a = 0; a < 3; a++) { g.o[a] = origin[a]; g.s[a] = spacing[a]; }
  const int nb = (int)((P + SPH_BLOCK - 1) / SPH_BLOCK);
  hipLaunchKernelGGL(k_surface_vertices, dim3(nb), dim3(SPH_BLOCK), 0, s->stream, r.field, L, g, r.code, r.offV, r.vbase, verts);
  hipLaunchKernelGGL(k_surface_triangles, dim3(nb), dim3(SPH_BLOCK), 0, s->stream, L, r.code, r.vbase, r.offT, tris);
  SPH_HIP(hipGetLastError());
  return SPH_OK;
}

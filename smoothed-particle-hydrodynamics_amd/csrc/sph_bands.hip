// Search bands: per step and for the whole domain, the sorted particles that lie within Rb of a y or z face of
// their cell, compacted in sorted order into eight arrays — one per neighbour row of the search kernel's 3 x 3 rows of cells
// other than its own x-row — with a start table per band that is read exactly like cellStart. k_find_neighbors stages its eight
// non-own rows from these arrays: a candidate of a y / z / yz neighbour cell that is not in the band of the shared face(s) is
// farther than the filter radius from every particle of the visiting cell, so it fails the distance test anyway.
//
//   slot s of row r = (sy + 1) + 3 (sz + 1), r != 4:  s = r - (r > 4)
//     s   0        1     2        3     4     5        6     7
//     row (-,-)    (0,-) (+,-)    (-,0) (+,0) (-,+)    (0,+) (+,+)          (sy, sz): the step from the visiting particle's cell
//     Q   hiY&hiZ  hiZ   loY&hiZ  hiY   loY   hiY&loZ  loZ   loY&loZ        the face(s) of its OWN cell the candidate is near
//
// The step's gather kernel (sph_sort.hip, with sph_band_flags.h) leaves one flag byte per sorted particle (bit s: member of band s)
// and, per wave and band, the ballot and its count: it holds the record and the key in registers. Four launches on the solver's
// stream behind k_cell_start do the rest:
//   k_band_super    the counts summed per 1024 waves and band
//   k_band_offsets  exclusive scan of the wave counts per band (the sums of the blocks in front, then a scan inside the block)
//   k_band_scatter  records (x, y, z, sorted index) to band[s][offset of the wave + rank inside the ballot]: stable
//   k_band_start    bandStart[s][c] = band-s entries in front of cellStart[c], c = 0 .. G
// No atomics: every word has one writer.
// The scan and k_band_start read counts, ballots and cellStart, never the records, so the scatter may come later for the particles
// whose records the first search launches do not read: the overlapped step scatters a prefix here and the rest beside the first
// search chunks (sphk_band_scatter by a device table; sph_api.hip).
#include "sph_common.h"

#define BAND_SUPER 1024  // wave entries per block of the scan

// block x: superCnt[s][x] = entries of band s in the waves [1024 x, 1024 x + 1024)
__global__ __launch_bounds__(SPH_BLOCK) void k_band_super(SphBandGeom g, SphBands b) {
  __shared__ uint32_t part[8][SPH_BLOCK];
  const int t = threadIdx.x, e0 = blockIdx.x * BAND_SUPER + 4 * t;
  uint32_t sum[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
  for (int k = 0; k < 4; k++) {
    if (e0 + k < g.waves) {
      const uint4 lo = *reinterpret_cast<const uint4*>(b.waveOff + (size_t)(e0 + k) * 8), hi = *reinterpret_cast<const uint4*>(b.waveOff + (size_t)(e0 + k) * 8 + 4);
      sum[0] += lo.x; sum[1] += lo.y; sum[2] += lo.z; sum[3] += lo.w; sum[4] += hi.x; sum[5] += hi.y; sum[6] += hi.z; sum[7] += hi.w;
    }
  }
#pragma unroll
  for (int s = 0; s < 8; s++) part[s][t] = sum[s];
  __syncthreads();
  for (int off = SPH_BLOCK / 2; off > 0; off >>= 1) {
    if (t < off) {
#pragma unroll
      for (int s = 0; s < 8; s++) part[s][t] += part[s][t + off];
    }
    __syncthreads();
  }
  if (t < 8) b.superCnt[t * b.superStride + blockIdx.x] = part[t][0];
}

// grid (supers, 8): block (x, s) turns the counts of the waves [1024 x, 1024 x + 1024) of band s into exclusive offsets in place
__global__ __launch_bounds__(SPH_BLOCK) void k_band_offsets(SphBandGeom g, SphBands b) {
  __shared__ uint32_t part[SPH_BLOCK];
  const int s = blockIdx.y, t = threadIdx.x;
  uint32_t before = 0;  // entries of the band in front of this block's waves
  for (int j = t; j < (int)blockIdx.x; j += SPH_BLOCK) before += b.superCnt[s * b.superStride + j];
  part[t] = before;
  __syncthreads();
  for (int off = SPH_BLOCK / 2; off > 0; off >>= 1) {
    if (t < off) part[t] += part[t + off];
    __syncthreads();
  }
  before = part[0];
  __syncthreads();
  uint32_t* row = b.waveOff + s;  // entry e of the band: row[8 e]
  const int e0 = blockIdx.x * BAND_SUPER + 4 * t;
  uint32_t v[4], sum = 0;
#pragma unroll
  for (int k = 0; k < 4; k++) { v[k] = (e0 + k < g.waves) ? row[(size_t)(e0 + k) * 8] : 0u; sum += v[k]; }
  part[t] = sum;
  __syncthreads();
  for (int off = 1; off < SPH_BLOCK; off <<= 1) {  // Hillis-Steele inclusive scan of the per-thread sums
    const uint32_t u = (t >= off) ? part[t - off] : 0u;
    __syncthreads();
    part[t] += u;
    __syncthreads();
  }
  uint32_t run = before + part[t] - sum;
#pragma unroll
  for (int k = 0; k < 4; k++) {
    if (e0 + k <= g.waves) row[(size_t)(e0 + k) * 8] = run;  // (entry `waves`: the band's total)
    run += v[k];
  }
}

// The sorted particles [begin, end) of a scatter launch: entries a and b of a small device table (the pipeline table or one of the
// serial tables that k_halo_check leaves every step, sph_api.hip), or a and b themselves where there is no table. begin is a
// multiple of SPH_BLOCK (a chunk edge, sphmi_chunks.h), so a wave of the launch is a wave of the gather's ballots.
struct BandRange { const uint32_t* table; int a, b; };
__device__ __forceinline__ void band_range(const BandRange& r, int N, int& begin, int& end) {
  begin = r.table ? (int)r.table[r.a] : r.a;
  end = min(r.table ? (int)r.table[r.b] : r.b, N);
}

// block `blk` of 256 of the range's particles; whole waves (the ballots), the lanes from `end` on contribute nothing
__device__ __forceinline__ void band_scatter_block(const SphBandGeom& g, const SphBands& b, const float4* __restrict__ sortedPos, int begin,
                                                   int end, int blk) {
  const int i = begin + blk * SPH_BLOCK + threadIdx.x, lane = threadIdx.x & 63, w = i >> 6;
  const uint32_t f = i < end ? b.flags[i] : 0u;
  float4 rec = make_float4(0.f, 0.f, 0.f, 0.f);
  if (f) { rec = sortedPos[i]; rec.w = __int_as_float(i); }
  const unsigned long long lt = (lane == 0) ? 0ull : (~0ull >> (64 - lane));
#pragma unroll
  for (int s = 0; s < 8; s++) {
    const unsigned long long m = __ballot((f >> s) & 1u);
    if ((f >> s) & 1u) {  // (only lanes with i < N; the rank is below the band's total, which is at most N <= cap)
      const uint32_t dst = b.waveOff[(size_t)w * 8 + s] + (uint32_t)__popcll(m & lt);
      if (dst < (uint32_t)b.cap) b.pos[(size_t)s * b.cap + dst] = rec;
    }
  }
}

// One block per 256 particles of the range the host sized the grid for; the blocks past the range's end leave.
__global__ __launch_bounds__(SPH_BLOCK) void k_band_scatter(SphBandGeom g, SphBands b, const float4* __restrict__ sortedPos, BandRange r) {
  int begin, end;
  band_range(r, g.N, begin, end);
  if (begin + (int)blockIdx.x * SPH_BLOCK >= end) return;  // uniform
  band_scatter_block(g, b, sortedPos, begin, end, blockIdx.x);
}
// The same over a fixed grid (SPH_SERIAL_GRID): for the launch that is empty on every step whose halo check passed.
__global__ __launch_bounds__(SPH_BLOCK) void k_band_scatter_strided(SphBandGeom g, SphBands b, const float4* __restrict__ sortedPos, BandRange r) {
  int begin, end;
  band_range(r, g.N, begin, end);
  const int active = end > begin ? (end - begin + SPH_BLOCK - 1) / SPH_BLOCK : 0;
  for (int blk = blockIdx.x; blk < active; blk += gridDim.x) band_scatter_block(g, b, sortedPos, begin, end, blk);
}

__global__ __launch_bounds__(SPH_BLOCK) void k_band_start(SphBandGeom g, SphBands b, const uint32_t* __restrict__ cellStart) {
  const int c = blockIdx.x * SPH_BLOCK + threadIdx.x;
  if (c > g.G) return;
  const int i = min((int)cellStart[c], g.N);
  const int w = i >> 6, l = i & 63;  // (w <= waves)
  const unsigned long long lt = (l == 0) ? 0ull : (~0ull >> (64 - l));
#pragma unroll
  for (int s = 0; s < 8; s++) {
    uint32_t v = b.waveOff[(size_t)w * 8 + s];
    if (l) v += (uint32_t)__popcll(b.mask[(size_t)w * 8 + s] & lt);
    b.start[(size_t)s * ((size_t)g.G + 1) + c] = v;
  }
}

// The margin on top of the filter radius Rf = sqrt(binU[63]): with kappa = |cellSizeInv * cellSize - 1| and L the
// largest face coordinate of the y and z axes, a candidate within the filter of a particle of the neighbouring cell lies within
//   Rf (1 + 2^-23) + L (kappa + 2^-22)
// of the shared face as band_flags evaluates that distance. Rounded up to the next float.
float sph_band_radius(const SphDev& d, float filterR2) {
  const double Rf = sqrt((double)filterR2);
  const double kappa = fabs((double)d.cellSizeInv * (double)d.cellSize - 1.0);
  const double L = (double)d.cellSize * (double)(max(d.gy, d.gz) + 1);
  const double rb = Rf * (1.0 + 0x1p-23) + L * (kappa + 0x1p-22);
  float f = (float)rb;
  if ((double)f < rb) f = nextafterf(f, INFINITY);
  return f;
}

size_t sphk_bands_bytes(const sph_solver* s, SphBands* out) {
  SphBands b = {};
  b.cap = s->capacity;
  b.waveStride = s->capTiles + 1;
  b.superStride = (b.waveStride + BAND_SUPER - 1) / BAND_SUPER;
  const size_t G1 = (size_t)s->d.G + 1;
  size_t at = 0;
  auto take = [&at](size_t bytes) { const size_t p = at; at += (bytes + 255) & ~(size_t)255; return p; };
  const size_t oPos = take(sizeof(float4) * 8 * (size_t)b.cap), oMask = take(sizeof(unsigned long long) * 8 * b.waveStride);
  const size_t oStart = take(sizeof(uint32_t) * 8 * G1), oOff = take(sizeof(uint32_t) * 8 * b.waveStride);
  const size_t oSuper = take(sizeof(uint32_t) * 8 * b.superStride), oFlags = take((size_t)b.cap);
  if (out) {
    char* base = (char*)s->bandBuf.p;
    b.pos = (float4*)(base + oPos); b.mask = (unsigned long long*)(base + oMask); b.start = (uint32_t*)(base + oStart);
    b.waveOff = (uint32_t*)(base + oOff); b.superCnt = (uint32_t*)(base + oSuper); b.flags = (uint8_t*)(base + oFlags);
    *out = b;
  }
  return at;
}

SphBandGeom sph_band_geom(const sph_solver* s) {
  const SphDev& d = s->d;
  SphBandGeom g;
  g.N = d.N; g.G = d.G; g.gx = d.gx; g.gy = d.gy; g.gz = d.gz; g.waves = (d.N + 63) >> 6;
  g.aliased = (unsigned long long)d.G > (unsigned long long)d.cellMask + 1ull ? 1 : 0;
  g.cellSize = d.cellSize; g.cellSizeInv = d.cellSizeInv;
  g.Rb = s->bandRadius;
  return g;
}

int sphk_band_scatter(sph_solver* s, const uint32_t* table, int a, int b, int count, bool strided, hipStream_t stream) {
  if (count <= 0) return SPH_OK;
  SphBands bands;
  sphk_bands_bytes(s, &bands);
  const SphBandGeom g = sph_band_geom(s);
  const BandRange r{table, a, b};
  const int nb = sph_blocks(count);
  if (strided) hipLaunchKernelGGL(k_band_scatter_strided, dim3(min(nb, SPH_SERIAL_GRID)), dim3(SPH_BLOCK), 0, stream, g, bands, (const float4*)s->d.sortedPos, r);
  else hipLaunchKernelGGL(k_band_scatter, dim3(nb), dim3(SPH_BLOCK), 0, stream, g, bands, (const float4*)s->d.sortedPos, r);
  SPH_HIP(hipGetLastError());
  return SPH_OK;
}

int sphk_build_bands(sph_solver* s, int scatterEnd) {
  SphBands b;
  sphk_bands_bytes(s, &b);
  const SphBandGeom g = sph_band_geom(s);
  const int supers = (g.waves + 1 + BAND_SUPER - 1) / BAND_SUPER;  // (<= superStride: waves + 1 <= waveStride)
  hipLaunchKernelGGL(k_band_super, dim3(supers), dim3(SPH_BLOCK), 0, s->stream, g, b);
  hipLaunchKernelGGL(k_band_offsets, dim3(supers, 8), dim3(SPH_BLOCK), 0, s->stream, g, b);
  const int end = min(max(scatterEnd, 0), g.N);
  const int rc = sphk_band_scatter(s, nullptr, 0, end, end, false, s->stream);
  if (rc != SPH_OK) return rc;
  hipLaunchKernelGGL(k_band_start, dim3(sph_blocks(g.G + 1)), dim3(SPH_BLOCK), 0, s->stream, g, b, (const uint32_t*)s->d.cellStart);
  SPH_HIP(hipGetLastError());
  return SPH_OK;
}

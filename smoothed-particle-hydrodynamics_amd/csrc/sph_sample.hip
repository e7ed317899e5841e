// Field sampling: SPH (poly6) interpolation of density, Shepard sum, velocity and pressure at arbitrary points and on regular
// grids, read from the sorted state of the last completed step (include/sphmi.h: sph_sample_points / sph_sample_grid, DESIGN.md
// §12). Read-only on every solver array.
//
// The arithmetic is fixed by the contract: for each selected particle j in ASCENDING SORTED INDEX,
//   a = hs2 - r2*ss2, w = a*a*a, v = w*(1/rho_j);  W += w, S += v, U += v*vel_j, P += v*p_j   (sequential float sums)
// so both kernels below (and a numpy float32 restatement) produce the same bits whatever order they enumerate cells in:
// the runs of distinct cell keys are disjoint and ascending in the sorted array, and every kernel walks the distinct keys of
// its cell box in ascending order.
#include "sph_sample_walk.h"

__device__ __forceinline__ void sample_hit(const SphDev& d, const SampleArgs& a, SampleAcc& acc, float px, float py, float pz,
                                           float4 xj, float4 vj /* vel.xyz, pressure */, float invRho) {
  const float dx = px - xj.x, dy = py - xj.y, dz = pz - xj.z;
  const float r2 = dx * dx + dy * dy + dz * dz;
  if (r2 < a.hh) {
    const float t = d.hs2 - r2 * a.ss2;
    const float w = t * t * t;
    const float v = w * invRho;
    acc.W += w; acc.S += v;
    acc.Ux += v * vj.x; acc.Uy += v * vj.y; acc.Uz += v * vj.z;
    acc.P += v * vj.w;
    acc.n++;
  }
}

// One point, one lane, direct loads: the distinct keys of the point's cell box in ascending order (each step finds the
// smallest key above the last one, so equal masked keys — aliased cells in reference mode — are visited once).
__device__ void sample_one(const SphDev& d, const SampleArgs& a, float px, float py, float pz, float* out) {
  SampleAcc acc = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0};
  if (sample_finite(px, py, pz)) {
    int x0, x1, y0, y1, z0, z1;
    sample_axis_range(px, d, x0, x1); sample_axis_range(py, d, y0, y1); sample_axis_range(pz, d, z0, z1);
    uint64_t last = 0;  // 0 = none yet; otherwise key + 1
    for (;;) {
      uint32_t best = 0xffffffffu;
      for (int cz = z0; cz <= z1; cz++)
        for (int cy = y0; cy <= y1; cy++)
          for (int cx = x0; cx <= x1; cx++) {
            const uint32_t k = sample_key(d, cx, cy, cz);
            if (k < (uint32_t)d.G && (uint64_t)k + 1 > last && k < best) best = k;
          }
      if (best == 0xffffffffu) break;
      last = (uint64_t)best + 1;
      uint32_t start, end;
      sample_run(d, best, start, end);
      for (uint32_t j = start; j < end; j++) {
        const float4 xj = d.sortedPos[j];
        if (!sample_type_ok(a, xj.w)) continue;
        const float4 v = d.sortedVel[j];
        sample_hit(d, a, acc, px, py, pz, xj, make_float4(v.x, v.y, v.z, d.rp[j].y), 1.0f / d.rho[j]);
      }
    }
  }
  sample_store(a, acc, out);
}

__global__ __launch_bounds__(SPH_BLOCK) void k_sample_points(SphDev d, SampleArgs a, const float4* __restrict__ pts, int count,
                                                             float* __restrict__ out) {
  const int i = blockIdx.x * SPH_BLOCK + threadIdx.x;
  if (i >= count) return;
  const float4 p = pts[i];
  sample_one(d, a, p.x, p.y, p.z, out + (size_t)i * SPH_SAMPLE_WORDS);
}

// Grid points whose bricks would span too many cells for the wave-uniform walk (spacing > 2h/3): one lane per point.
__global__ __launch_bounds__(SPH_BLOCK) void k_sample_grid_points(SphDev d, SampleArgs a, float* __restrict__ out) {
  const long long i = (long long)blockIdx.x * SPH_BLOCK + threadIdx.x;
  const long long plane = (long long)a.nx * a.ny;
  if (i >= plane * a.nz) return;
  const int k = (int)(i / plane), rem = (int)(i - (long long)k * plane), j = rem / a.nx, ii = rem - j * a.nx;
  const float px = a.ox + (float)ii * a.sx, py = a.oy + (float)j * a.sy, pz = a.oz + (float)(a.kBase + k) * a.sz;
  sample_one(d, a, px, py, pz, out + (size_t)i * SPH_SAMPLE_WORDS);
}

// The hot path: one wave (one block) per 4x4x4 brick of grid points, lane = x + 4y + 16z. The brick's cell box is the union of
// its points' boxes; its distinct keys are taken in ascending order (wave-wide minimum above the last one, made scalar), and
// each run is streamed through LDS in chunks of 64 candidates: one coalesced load per candidate (position, velocity, pressure,
// 1/rho once per candidate; particles of unselected types get a NaN x so that every lane's distance test rejects them), then
// every lane loops over the chunk with broadcast LDS reads. A candidate from a cell outside a lane's own box fails that lane's
// distance test (monotone hash), so each lane's sums come out in ascending sorted index with no per-lane cell logic.
// (Broadcasting each candidate with v_readlane instead of LDS was measured 2x slower: DESIGN.md §12.)
__global__ __launch_bounds__(SPH_SAMPLE_WAVE) void k_sample_grid(SphDev d, SampleArgs a, int nbx, int nby, int nblocks,
                                                                 float* __restrict__ out) {
  __shared__ float4 sPos[SPH_SAMPLE_WAVE];
  __shared__ float4 sVel[SPH_SAMPLE_WAVE];
  __shared__ float sInv[SPH_SAMPLE_WAVE];
  const int b = sample_xcd_block(nblocks);
  const int lane = threadIdx.x;
  const int bx = b % nbx, by = (b / nbx) % nby, bz = b / (nbx * nby);
  const int i = bx * 4 + (lane & 3), j = by * 4 + ((lane >> 2) & 3), k = bz * 4 + (lane >> 4);
  const bool valid = i < a.nx && j < a.ny && k < a.nz;
  float px = a.ox + (float)i * a.sx, py = a.oy + (float)j * a.sy, pz = a.oz + (float)(a.kBase + k) * a.sz;
  const bool active = valid && sample_finite(px, py, pz);
  float* o = out + (((size_t)k * a.ny + j) * a.nx + i) * SPH_SAMPLE_WORDS;
  int x0 = 0x7fffffff, x1 = -0x7fffffff - 1, y0 = x0, y1 = x1, z0 = x0, z1 = x1;
  if (active) { sample_axis_range(px, d, x0, x1); sample_axis_range(py, d, y0, y1); sample_axis_range(pz, d, z0, z1); }
  else px = py = pz = __builtin_nanf("");  // never selects anything
  const int bx0 = wave_min_i(x0), bx1 = wave_max_i(x1), by0 = wave_min_i(y0), by1 = wave_max_i(y1);
  const int bz0 = wave_min_i(z0), bz1 = wave_max_i(z1);
  if (bx0 > bx1) {  // no active lane: non-finite points only
    if (valid) sample_store(a, SampleAcc{0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0}, o);
    return;
  }
  const long long nbox = (long long)(bx1 - bx0 + 1) * (by1 - by0 + 1) * (bz1 - bz0 + 1);
  if (nbox > SPH_SAMPLE_BOX_MAX) {  // points far apart (huge coordinates): per-lane walk
    if (valid) sample_one(d, a, px, py, pz, o);
    return;
  }
  // lane l holds the key of box cell l (0xffffffff: none, or outside the table)
  const int wx = bx1 - bx0 + 1, wy = by1 - by0 + 1;
  uint32_t myKey = 0xffffffffu;
  if (lane < (int)nbox) {
    const int cx = bx0 + lane % wx, cy = by0 + (lane / wx) % wy, cz = bz0 + lane / (wx * wy);
    const uint32_t key = sample_key(d, cx, cy, cz);
    if (key < (uint32_t)d.G) myKey = key;
  }
  SampleAcc acc = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0};
  for (;;) {
    const uint32_t key = __builtin_amdgcn_readfirstlane(wave_min_u(myKey));
    if (key == 0xffffffffu) break;
    if (myKey == key) myKey = 0xffffffffu;  // dedupe: every lane holding this key drops it
    uint32_t start, end;
    sample_run(d, key, start, end);
    for (uint32_t base = start; base < end; base += SPH_SAMPLE_WAVE) {
      const uint32_t c = base + (uint32_t)lane;
      if (c < end) {
        float4 xj = d.sortedPos[c];
        const float4 v = d.sortedVel[c];
        if (!sample_type_ok(a, xj.w)) xj.x = __builtin_nanf("");
        sPos[lane] = xj;
        sVel[lane] = make_float4(v.x, v.y, v.z, d.rp[c].y);
        sInv[lane] = 1.0f / d.rho[c];
      }
      __syncthreads();
      const int cnt = (int)min(end - base, (uint32_t)SPH_SAMPLE_WAVE);
      for (int q = 0; q < cnt; q++) sample_hit(d, a, acc, px, py, pz, sPos[q], sVel[q], sInv[q]);
      __syncthreads();
    }
  }
  if (valid) sample_store(a, acc, o);
}

int sphk_sample_points(sph_solver* s, const SampleParams& p, const float* pts4, int count, float* out) {
  if (count <= 0) return SPH_OK;
  SampleArgs a = {};
  a.typeMask = p.typeMask; a.hh = p.hh; a.ss2 = p.ss2; a.mwp = p.mwp;
  hipLaunchKernelGGL(k_sample_points, dim3(sph_blocks(count)), dim3(SPH_BLOCK), 0, s->stream, s->d, a, (const float4*)pts4, count, out);
  SPH_HIP(hipGetLastError());
  return SPH_OK;
}

int sphk_sample_grid(sph_solver* s, const SampleParams& p, const float origin[3], const float spacing[3], int nx, int ny,
                     int kBase, int nz, float* out) {
  SampleArgs a = {};
  a.typeMask = p.typeMask; a.hh = p.hh; a.ss2 = p.ss2; a.mwp = p.mwp;
  a.ox = origin[0]; a.oy = origin[1]; a.oz = origin[2];
  a.sx = spacing[0]; a.sy = spacing[1]; a.sz = spacing[2];
  a.nx = nx; a.ny = ny; a.nz = nz; a.kBase = kBase;
  // A 4-point brick spans 3 spacings; with spacing <= 2h/3 its box is at most 3 cells (of 2h) per axis: the wave-uniform walk.
  const float lim = 2.0f * s->d.h / 3.0f;
  const bool bricks = fabsf(a.sx) <= lim && fabsf(a.sy) <= lim && fabsf(a.sz) <= lim;
  if (bricks) {
    const int nbx = (nx + 3) / 4, nby = (ny + 3) / 4, nbz = (nz + 3) / 4;
    const long long nb = (long long)nbx * nby * nbz;
    if (nb > 0x7fffffffLL) { sph_set_error("sph_sample_grid: chunk too large"); return SPH_ERR_INVALID; }
    hipLaunchKernelGGL(k_sample_grid, dim3((unsigned)nb), dim3(SPH_SAMPLE_WAVE), 0, s->stream, s->d, a, nbx, nby, (int)nb, out);
  } else {
    const long long n = (long long)nx * ny * nz;
    hipLaunchKernelGGL(k_sample_grid_points, dim3((unsigned)((n + SPH_BLOCK - 1) / SPH_BLOCK)), dim3(SPH_BLOCK), 0, s->stream, s->d, a, out);
  }
  SPH_HIP(hipGetLastError());
  return SPH_OK;
}

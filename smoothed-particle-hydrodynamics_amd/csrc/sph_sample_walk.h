// Shared by the sampling kernels (sph_sample.hip) and the gradient kernels (sph_gradient.hip): the two cell walks (one query
// point per lane; one 4x4x4 brick of grid points per wave) as templates over what is done per selected particle, the pieces
// they are made of (axis ranges, masked keys, runs of the cell table), the sampling record and the split of a grid launch
// between the two walks. See sph_sample.hip for the contract these serve.
#pragma once
#include "sph_common.h"

#define SPH_SAMPLE_WAVE 64
#define SPH_SAMPLE_BOX_MAX 64  // cells a brick box may hold for the wave-uniform walk (3x3x3 = 27 while spacing <= 2h/3)

// Cell range of one axis that holds every particle a query coordinate c can select. The hash truncates x * cellSizeInv and
// is monotone, so [(int)((c-h)*inv), (int)((c+h)*inv)] holds them up to rounding; the range is widened by a margin far
// above the rounding of those two products and of the float distance test (visiting an extra cell costs time, never
// correctness: its particles fail the distance test). The margin grows with |u| so that it stays above one ulp of u.
__device__ __forceinline__ void sample_axis_range(float c, const SphDev& d, int& lo, int& hi) {
  float ul = (c - d.h) * d.cellSizeInv, uh = (c + d.h) * d.cellSizeInv;
  ul -= fminf(fabsf(ul) * 0x1p-21f + 0x1p-10f, 0.5f);
  uh += fminf(fabsf(uh) * 0x1p-21f + 0x1p-10f, 0.5f);
  ul = fminf(fmaxf(ul, -0x1p30f), 0x1p30f);  // (a float -> int conversion out of range is undefined)
  uh = fminf(fmaxf(uh, -0x1p30f), 0x1p30f);
  lo = (int)ul; hi = (int)uh;
  if (hi - lo > 3) hi = lo + 3;  // only for |u| beyond ~2^20 cells, where float coordinates no longer resolve h
}

// masked key of cell (cx, cy, cz) exactly as k_hash computes it (the int products wrap like these unsigned ones)
__device__ __forceinline__ uint32_t sample_key(const SphDev& d, int cx, int cy, int cz) {
  return ((uint32_t)cx + (uint32_t)cy * (uint32_t)d.gx + (uint32_t)cz * (uint32_t)d.gx * (uint32_t)d.gy) & d.cellMask;
}

// Sorted-index run [start, end) of key k < G. cellStart[G] is N, so the run of key G-1 would also hold particles whose keys are
// >= G (outside the declared grid, not in the cell table): it ends at the first of those instead.
__device__ __forceinline__ void sample_run(const SphDev& d, uint32_t k, uint32_t& start, uint32_t& end) {
  start = d.cellStart[k];
  end = d.cellStart[k + 1];
  if (k + 1 == (uint32_t)d.G) {
    uint32_t lo = start, hi = end;
    while (lo < hi) {
      const uint32_t mid = (lo + hi) >> 1;
      if (d.keys[mid] < (uint32_t)d.G) lo = mid + 1; else hi = mid;
    }
    end = lo;
  }
}

struct SampleAcc {
  float W, S, Ux, Uy, Uz, P;
  int n;
};

// One selected candidate into the sums: the arithmetic of the sampling contract (sph_sample.hip), in its order.
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

__device__ __forceinline__ bool sample_type_ok(const SampleArgs& a, float w) {
  const int t = (int)w;
  return t >= 1 && t <= 3 && ((1u << t) & a.typeMask);
}

__device__ __forceinline__ void sample_store(const SampleArgs& a, const SampleAcc& acc, float* out) {
  float4 r0 = make_float4(a.mwp * acc.W, a.mwp * acc.S, 0.f, 0.f), r1 = make_float4(0.f, 0.f, (float)acc.n, 0.f);
  if (acc.S != 0.f) { r0.z = acc.Ux / acc.S; r0.w = acc.Uy / acc.S; r1.x = acc.Uz / acc.S; r1.y = acc.P / acc.S; }
  reinterpret_cast<float4*>(out)[0] = r0;
  reinterpret_cast<float4*>(out)[1] = r1;
}

__device__ __forceinline__ bool sample_finite(float x, float y, float z) {
  return fabsf(x) <= 3.402823466e38f && fabsf(y) <= 3.402823466e38f && fabsf(z) <= 3.402823466e38f;
}

// Consecutive bricks share most of their cells: keep runs of them on one XCD (one L2) — the remap of sph_pcisph.hip's xcd_block.
__device__ __forceinline__ int sample_xcd_block(int nblocks) {
  const int b = blockIdx.x;
  const int per = nblocks >> 3;
  const int even = per << 3;
  if (b >= even) return b;
  return (b & 7) * per + (b >> 3);
}

__device__ __forceinline__ int wave_min_i(int v) {
  for (int o = 32; o >= 1; o >>= 1) v = min(v, __shfl_xor(v, o, SPH_SAMPLE_WAVE));
  return v;
}
__device__ __forceinline__ int wave_max_i(int v) {
  for (int o = 32; o >= 1; o >>= 1) v = max(v, __shfl_xor(v, o, SPH_SAMPLE_WAVE));
  return v;
}
__device__ __forceinline__ uint32_t wave_min_u(uint32_t v) {
  for (int o = 32; o >= 1; o >>= 1) v = min(v, (uint32_t)__shfl_xor((int)v, o, SPH_SAMPLE_WAVE));
  return v;
}

// The point walk. One point, one lane, direct loads: the distinct keys of the point's cell box in ascending order (each step
// finds the smallest key above the last one, so equal masked keys — aliased cells in reference mode — are visited once), and
// hit(px, py, pz, xj, (vel.xyz, pressure), 1/rho_j) for every particle of a selected type in those runs, in ascending
// sorted index. Returns whether the point is finite (a non-finite point selects nothing).
template <typename Hit>
__device__ __forceinline__ bool sample_point_walk(const SphDev& d, const SampleArgs& a, float px, float py, float pz, Hit hit) {
  if (!sample_finite(px, py, pz)) return false;
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
      hit(px, py, pz, xj, make_float4(v.x, v.y, v.z, d.rp[j].y), 1.0f / d.rho[j]);
    }
  }
  return true;
}

// Point i of a grid chunk in the order of its records (x fastest); false past the chunk's end.
__device__ __forceinline__ bool sample_grid_point(const SampleArgs& a, long long i, float& px, float& py, float& pz) {
  const long long plane = (long long)a.nx * a.ny;
  if (i >= plane * a.nz) return false;
  const int k = (int)(i / plane), rem = (int)(i - (long long)k * plane), j = rem / a.nx, ii = rem - j * a.nx;
  px = a.ox + (float)ii * a.sx; py = a.oy + (float)j * a.sy; pz = a.oz + (float)(a.kBase + k) * a.sz;
  return true;
}

struct SampleBrickLane {
  bool valid;    // the lane's point lies inside the chunk: it has a record
  bool finite;   // ... and its coordinates are finite
  size_t index;  // of that record in the chunk
};

// The brick walk, the hot path: one wave (one block) per 4x4x4 brick of grid points, lane = x + 4y + 16z. The brick's cell box
// is the union of its points' boxes; its distinct keys are taken in ascending order (wave-wide minimum above the last one, made
// scalar), and each run is streamed through LDS in chunks of 64 candidates: one coalesced load per candidate (position,
// velocity, pressure, 1/rho once per candidate; particles of unselected types get a NaN x so that every lane's distance test
// rejects them), then every lane loops over the chunk with broadcast LDS reads and calls hit as the point walk does. A candidate
// from a cell outside a lane's own box fails that lane's distance test (monotone hash), so each lane's hits come in ascending
// sorted index with no per-lane cell logic; hit has to make that distance test, with r2 < a.hh false for a NaN.
// (Broadcasting each candidate with v_readlane instead of LDS was measured 2x slower: DESIGN.md §12.)
// Bricks whose box would exceed SPH_SAMPLE_BOX_MAX cells (points far apart: huge coordinates) walk each lane's own box in turn
// (at most 4x4x4 cells, sample_axis_range) with the other lanes' query points made NaN: the same ascending walk as the point
// walk's, without inlining a second walk, which would cost the kernels registers.
template <typename Hit>
__device__ __forceinline__ SampleBrickLane sample_brick_walk(const SphDev& d, const SampleArgs& a, int nbx, int nby, int nblocks,
                                                             Hit hit) {
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
  int x0 = 0x7fffffff, x1 = -0x7fffffff - 1, y0 = x0, y1 = x1, z0 = x0, z1 = x1;
  if (active) { sample_axis_range(px, d, x0, x1); sample_axis_range(py, d, y0, y1); sample_axis_range(pz, d, z0, z1); }
  else px = py = pz = __builtin_nanf("");  // never selects anything
  int bx0 = wave_min_i(x0), bx1 = wave_max_i(x1), by0 = wave_min_i(y0), by1 = wave_max_i(y1);
  int bz0 = wave_min_i(z0), bz1 = wave_max_i(z1);
  const bool perLane = bx0 <= bx1 && (long long)(bx1 - bx0 + 1) * (by1 - by0 + 1) * (bz1 - bz0 + 1) > SPH_SAMPLE_BOX_MAX;
  // walks: 1 over the brick's box (none if no lane is active), or one per lane's box
  for (int w = 0; w < (perLane ? SPH_SAMPLE_WAVE : 1); w++) {
    float qx = px, qy = py, qz = pz;
    if (perLane) {
      bx0 = __shfl(x0, w, SPH_SAMPLE_WAVE); bx1 = __shfl(x1, w, SPH_SAMPLE_WAVE);
      by0 = __shfl(y0, w, SPH_SAMPLE_WAVE); by1 = __shfl(y1, w, SPH_SAMPLE_WAVE);
      bz0 = __shfl(z0, w, SPH_SAMPLE_WAVE); bz1 = __shfl(z1, w, SPH_SAMPLE_WAVE);
      if (lane != w) qx = qy = qz = __builtin_nanf("");
    }
    if (bx0 > bx1) continue;  // no active lane (in this walk)
    const int nbox = (bx1 - bx0 + 1) * (by1 - by0 + 1) * (bz1 - bz0 + 1);
    // lane l holds the key of box cell l (0xffffffff: none, or outside the table)
    const int wx = bx1 - bx0 + 1, wy = by1 - by0 + 1;
    uint32_t myKey = 0xffffffffu;
    if (lane < nbox) {
      const int cx = bx0 + lane % wx, cy = by0 + (lane / wx) % wy, cz = bz0 + lane / (wx * wy);
      const uint32_t key = sample_key(d, cx, cy, cz);
      if (key < (uint32_t)d.G) myKey = key;
    }
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
        for (int q = 0; q < cnt; q++) hit(qx, qy, qz, sPos[q], sVel[q], sInv[q]);
        __syncthreads();
      }
    }
  }
  return SampleBrickLane{valid, active, ((size_t)k * a.ny + j) * a.nx + i};
}

// One chunk of a grid (z-planes [kBase, kBase + nz)): fills the lattice part of the arguments and launches the brick walk,
// bricks(args, nbx, nby, blocks), or one lane per point, points(args, blocks). `what` names the entry point in the error.
template <typename Bricks, typename Points>
static int sample_launch_grid(const sph_solver* s, SampleArgs a, const float origin[3], const float spacing[3], int nx, int ny,
                              int kBase, int nz, const char* what, Bricks bricks, Points points) {
  a.ox = origin[0]; a.oy = origin[1]; a.oz = origin[2];
  a.sx = spacing[0]; a.sy = spacing[1]; a.sz = spacing[2];
  a.nx = nx; a.ny = ny; a.nz = nz; a.kBase = kBase;
  // A 4-point brick spans 3 spacings; with spacing <= 2h/3 its box is at most 3 cells (of 2h) per axis: the wave-uniform walk.
  const float lim = 2.0f * s->d.h / 3.0f;
  if (fabsf(a.sx) <= lim && fabsf(a.sy) <= lim && fabsf(a.sz) <= lim) {
    const int nbx = (nx + 3) / 4, nby = (ny + 3) / 4, nbz = (nz + 3) / 4;
    const long long nb = (long long)nbx * nby * nbz;
    if (nb > 0x7fffffffLL) { sph_set_error("%s: chunk too large", what); return SPH_ERR_INVALID; }
    bricks(a, nbx, nby, (int)nb);
  } else {
    const long long n = (long long)nx * ny * nz;
    points(a, (unsigned)((n + SPH_BLOCK - 1) / SPH_BLOCK));
  }
  SPH_HIP(hipGetLastError());
  return SPH_OK;
}

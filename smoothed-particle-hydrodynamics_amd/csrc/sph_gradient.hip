// Gradient sampling: the SPH (poly6) gradients of density, Shepard sum, velocity and pressure, with vorticity, divergence and
// the Q-criterion, at arbitrary points and on regular grids, plus vertex normals of the last extracted surface
// (include/sphmi.h: sph_sample_gradient_points / sph_sample_gradient_grid / sph_surface_normals).
// Read-only on every solver array.
//
// The walk is sampling's (sph_sample.hip, sph_sample_walk.h): every selected particle j in ASCENDING SORTED INDEX, so the
// sums below come out the same in every kernel and in the numpy restatement. Per hit, on top of sampling's sums:
//   g = t*t, q = g*(1/rho_j);  B += g*d, C += q*d, E_A += (q*A)*d for A in (vx, vy, vz, p)   (sequential float sums)
// and the record's words 8..30 are formed from them once (grad_record).
#include "sph_sample_walk.h"

struct GradAcc {
  SampleAcc s;       // sampling's sums: words 0..7 come out of sample_store's arithmetic
  float B[3], C[3];  // sum g*d, sum q*d
  float E[4][3];     // sum (q*A)*d for A = vx, vy, vz, p
};

__device__ __forceinline__ void grad_zero(GradAcc& g) {
  g.s = SampleAcc{0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0};
#pragma unroll
  for (int c = 0; c < 3; c++) {
    g.B[c] = 0.f; g.C[c] = 0.f;
#pragma unroll
    for (int i = 0; i < 4; i++) g.E[i][c] = 0.f;
  }
}

__device__ __forceinline__ void grad_hit(const SphDev& d, const SampleArgs& a, GradAcc& g, float px, float py, float pz,
                                         float4 xj, float4 vj /* vel.xyz, pressure */, float invRho) {
  const float dx = px - xj.x, dy = py - xj.y, dz = pz - xj.z;
  const float r2 = dx * dx + dy * dy + dz * dz;
  if (r2 < a.hh) {
    const float t = d.hs2 - r2 * a.ss2;
    const float tt = t * t;
    const float w = tt * t;  // t*t*t of sample_hit, bit for bit
    const float v = w * invRho;
    g.s.W += w; g.s.S += v;
    g.s.Ux += v * vj.x; g.s.Uy += v * vj.y; g.s.Uz += v * vj.z;
    g.s.P += v * vj.w;
    g.s.n++;
    const float q = tt * invRho;
    g.B[0] += tt * dx; g.B[1] += tt * dy; g.B[2] += tt * dz;
    g.C[0] += q * dx; g.C[1] += q * dy; g.C[2] += q * dz;
    const float A[4] = {vj.x, vj.y, vj.z, vj.w};
#pragma unroll
    for (int i = 0; i < 4; i++) {
      const float av = q * A[i];
      g.E[i][0] += av * dx; g.E[i][1] += av * dy; g.E[i][2] += av * dz;
    }
  }
}

// The 32-word record (include/sphmi.h). K = (float)(-6 * massWpoly6 * simScale).
__device__ __forceinline__ void grad_record(const SampleArgs& a, float K, const GradAcc& g, float r[SPH_GRADIENT_WORDS]) {
  const SampleAcc& s = g.s;
  r[0] = a.mwp * s.W; r[1] = a.mwp * s.S;
  r[2] = r[3] = r[4] = r[5] = 0.f;
  if (s.S != 0.f) { r[2] = s.Ux / s.S; r[3] = s.Uy / s.S; r[4] = s.Uz / s.S; r[5] = s.P / s.S; }
  r[6] = (float)s.n; r[7] = 0.f;
#pragma unroll
  for (int c = 0; c < 3; c++) { r[8 + c] = K * g.B[c]; r[11 + c] = K * g.C[c]; }
#pragma unroll
  for (int w = 14; w < SPH_GRADIENT_WORDS; w++) r[w] = 0.f;
  if (s.S != 0.f) {
    float G[3][3];
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
      for (int c = 0; c < 3; c++) { G[i][c] = K * (g.E[i][c] - r[2 + i] * g.C[c]); r[14 + 3 * i + c] = G[i][c]; }
#pragma unroll
    for (int c = 0; c < 3; c++) r[23 + c] = K * (g.E[3][c] - r[5] * g.C[c]);
    r[26] = G[2][1] - G[1][2]; r[27] = G[0][2] - G[2][0]; r[28] = G[1][0] - G[0][1];
    r[29] = (G[0][0] + G[1][1]) + G[2][2];
    float qq = 0.f;
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
      for (int j = 0; j < 3; j++) qq += G[i][j] * G[j][i];
    r[30] = -0.5f * qq;
  }
}

// finite = false: a non-finite query point, whose record is all +0 (K*0 would be -0 in words 8..13)
__device__ __forceinline__ void grad_store(const SampleArgs& a, float K, const GradAcc& g, bool finite, float* out) {
  float r[SPH_GRADIENT_WORDS];
  grad_record(a, K, g, r);
  if (!finite) {
#pragma unroll
    for (int w = 0; w < SPH_GRADIENT_WORDS; w++) r[w] = 0.f;
  }
  float4* o = reinterpret_cast<float4*>(out);
#pragma unroll
  for (int k = 0; k < SPH_GRADIENT_WORDS / 4; k++) o[k] = make_float4(r[4 * k], r[4 * k + 1], r[4 * k + 2], r[4 * k + 3]);
}

// One point, one lane, direct loads: sample_one's walk with the gradient sums. Returns whether the point is finite.
__device__ bool grad_one(const SphDev& d, const SampleArgs& a, float px, float py, float pz, GradAcc& g) {
  grad_zero(g);
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
      grad_hit(d, a, g, px, py, pz, xj, make_float4(v.x, v.y, v.z, d.rp[j].y), 1.0f / d.rho[j]);
    }
  }
  return true;
}

__global__ __launch_bounds__(SPH_BLOCK) void k_gradient_points(SphDev d, SampleArgs a, float K, const float4* __restrict__ pts,
                                                               int count, float* __restrict__ out) {
  const int i = blockIdx.x * SPH_BLOCK + threadIdx.x;
  if (i >= count) return;
  const float4 p = pts[i];
  GradAcc g;
  const bool finite = grad_one(d, a, p.x, p.y, p.z, g);
  grad_store(a, K, g, finite, out + (size_t)i * SPH_GRADIENT_WORDS);
}

// Grid points whose bricks would span too many cells for the wave-uniform walk (spacing > 2h/3): one lane per point.
__global__ __launch_bounds__(SPH_BLOCK) void k_gradient_grid_points(SphDev d, SampleArgs a, float K, float* __restrict__ out) {
  const long long i = (long long)blockIdx.x * SPH_BLOCK + threadIdx.x;
  const long long plane = (long long)a.nx * a.ny;
  if (i >= plane * a.nz) return;
  const int k = (int)(i / plane), rem = (int)(i - (long long)k * plane), j = rem / a.nx, ii = rem - j * a.nx;
  const float px = a.ox + (float)ii * a.sx, py = a.oy + (float)j * a.sy, pz = a.oz + (float)(a.kBase + k) * a.sz;
  GradAcc g;
  const bool finite = grad_one(d, a, px, py, pz, g);
  grad_store(a, K, g, finite, out + (size_t)i * SPH_GRADIENT_WORDS);
}

// The hot path: k_sample_grid's brick walk (one wave per 4x4x4 brick, the brick box's distinct keys ascending and made scalar,
// runs staged through LDS 64 candidates at a time with the type folded into a NaN x) with the gradient sums per hit. The LDS
// bytes per candidate are sampling's; only the work per hit and the accumulators grow.
// Bricks whose box would exceed SPH_SAMPLE_BOX_MAX cells (points far apart: huge coordinates) walk each lane's own box in turn
// (at most 4x4x4 cells, sample_axis_range) with the other lanes' query points made NaN: the same ascending walk as grad_one,
// without inlining a second walk, which would double the kernel's registers.
__global__ __launch_bounds__(SPH_SAMPLE_WAVE) void k_gradient_grid(SphDev d, SampleArgs a, float K, int nbx, int nby, int nblocks,
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
  float* o = out + (((size_t)k * a.ny + j) * a.nx + i) * SPH_GRADIENT_WORDS;
  int x0 = 0x7fffffff, x1 = -0x7fffffff - 1, y0 = x0, y1 = x1, z0 = x0, z1 = x1;
  if (active) { sample_axis_range(px, d, x0, x1); sample_axis_range(py, d, y0, y1); sample_axis_range(pz, d, z0, z1); }
  else px = py = pz = __builtin_nanf("");  // never selects anything
  int bx0 = wave_min_i(x0), bx1 = wave_max_i(x1), by0 = wave_min_i(y0), by1 = wave_max_i(y1);
  int bz0 = wave_min_i(z0), bz1 = wave_max_i(z1);
  GradAcc g;
  grad_zero(g);
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
        for (int q = 0; q < cnt; q++) grad_hit(d, a, g, qx, qy, qz, sPos[q], sVel[q], sInv[q]);
        __syncthreads();
      }
    }
  }
  if (valid) grad_store(a, K, g, active, o);
}

// One normal per mesh vertex: the gradient record at the vertex's coordinates (the points path, bit for bit), then
// n = -grad/|grad| with |grad| = sqrtf((gx*gx + gy*gy) + gz*gz); (0, 0, 0) where that length is 0 or not finite.
__global__ __launch_bounds__(SPH_BLOCK) void k_surface_normals(SphDev d, SampleArgs a, float K, int field,
                                                               const float* __restrict__ verts, int count, float* __restrict__ normals) {
  const int i = blockIdx.x * SPH_BLOCK + threadIdx.x;
  if (i >= count) return;
  GradAcc g;
  grad_one(d, a, verts[3 * (size_t)i], verts[3 * (size_t)i + 1], verts[3 * (size_t)i + 2], g);
  float r[SPH_GRADIENT_WORDS];
  grad_record(a, K, g, r);
  float gx, gy, gz;  // (a switch, so that the record stays in registers)
  switch (field) {
    case 0: gx = r[8]; gy = r[9]; gz = r[10]; break;
    case 1: gx = r[11]; gy = r[12]; gz = r[13]; break;
    case 2: gx = r[14]; gy = r[15]; gz = r[16]; break;
    case 3: gx = r[17]; gy = r[18]; gz = r[19]; break;
    case 4: gx = r[20]; gy = r[21]; gz = r[22]; break;
    default: gx = r[23]; gy = r[24]; gz = r[25]; break;
  }
  const float len = sqrtf(gx * gx + gy * gy + gz * gz);
  float nx = 0.f, ny = 0.f, nz = 0.f;
  if (len != 0.f && len <= 3.402823466e38f) { nx = -(gx / len); ny = -(gy / len); nz = -(gz / len); }
  normals[3 * (size_t)i] = nx;
  normals[3 * (size_t)i + 1] = ny;
  normals[3 * (size_t)i + 2] = nz;
}

static SampleArgs grad_args(const SampleParams& p) {
  SampleArgs a = {};
  a.typeMask = p.typeMask; a.hh = p.hh; a.ss2 = p.ss2; a.mwp = p.mwp;
  return a;
}

int sphk_gradient_points(sph_solver* s, const SampleParams& p, float K, const float* pts4, int count, float* out) {
  if (count <= 0) return SPH_OK;
  hipLaunchKernelGGL(k_gradient_points, dim3(sph_blocks(count)), dim3(SPH_BLOCK), 0, s->stream, s->d, grad_args(p), K,
                     (const float4*)pts4, count, out);
  SPH_HIP(hipGetLastError());
  return SPH_OK;
}

int sphk_gradient_grid(sph_solver* s, const SampleParams& p, float K, const float origin[3], const float spacing[3], int nx, int ny,
                       int kBase, int nz, float* out) {
  SampleArgs a = grad_args(p);
  a.ox = origin[0]; a.oy = origin[1]; a.oz = origin[2];
  a.sx = spacing[0]; a.sy = spacing[1]; a.sz = spacing[2];
  a.nx = nx; a.ny = ny; a.nz = nz; a.kBase = kBase;
  // the brick / per-lane split of sphk_sample_grid
  const float lim = 2.0f * s->d.h / 3.0f;
  const bool bricks = fabsf(a.sx) <= lim && fabsf(a.sy) <= lim && fabsf(a.sz) <= lim;
  if (bricks) {
    const int nbx = (nx + 3) / 4, nby = (ny + 3) / 4, nbz = (nz + 3) / 4;
    const long long nb = (long long)nbx * nby * nbz;
    if (nb > 0x7fffffffLL) { sph_set_error("sph_sample_gradient_grid: chunk too large"); return SPH_ERR_INVALID; }
    hipLaunchKernelGGL(k_gradient_grid, dim3((unsigned)nb), dim3(SPH_SAMPLE_WAVE), 0, s->stream, s->d, a, K, nbx, nby, (int)nb, out);
  } else {
    const long long n = (long long)nx * ny * nz;
    hipLaunchKernelGGL(k_gradient_grid_points, dim3((unsigned)((n + SPH_BLOCK - 1) / SPH_BLOCK)), dim3(SPH_BLOCK), 0, s->stream,
                       s->d, a, K, out);
  }
  SPH_HIP(hipGetLastError());
  return SPH_OK;
}

int sphk_surface_normals(sph_solver* s, const SampleParams& p, float K, int field, const float* verts, int count, float* normals) {
  if (count <= 0) return SPH_OK;
  hipLaunchKernelGGL(k_surface_normals, dim3(sph_blocks(count)), dim3(SPH_BLOCK), 0, s->stream, s->d, grad_args(p), K, field, verts,
                     count, normals);
  SPH_HIP(hipGetLastError());
  return SPH_OK;
}

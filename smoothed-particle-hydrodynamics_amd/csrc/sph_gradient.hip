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

// One point through the point walk (sph_sample_walk.h) with the gradient sums. Returns whether the point is finite.
__device__ bool grad_one(const SphDev& d, const SampleArgs& a, float px, float py, float pz, GradAcc& g) {
  grad_zero(g);
  return sample_point_walk(d, a, px, py, pz, [&](float x, float y, float z, float4 xj, float4 vj, float invRho) {
    grad_hit(d, a, g, x, y, z, xj, vj, invRho);
  });
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
  float px, py, pz;
  if (!sample_grid_point(a, i, px, py, pz)) return;
  GradAcc g;
  const bool finite = grad_one(d, a, px, py, pz, g);
  grad_store(a, K, g, finite, out + (size_t)i * SPH_GRADIENT_WORDS);
}

// The hot path: the brick walk (sph_sample_walk.h) with the gradient sums per hit. The LDS bytes per candidate are sampling's;
// only the work per hit and the accumulators grow.
__global__ __launch_bounds__(SPH_SAMPLE_WAVE) void k_gradient_grid(SphDev d, SampleArgs a, float K, int nbx, int nby, int nblocks,
                                                                   float* __restrict__ out) {
  GradAcc g;
  grad_zero(g);
  const SampleBrickLane l = sample_brick_walk(d, a, nbx, nby, nblocks, [&](float x, float y, float z, float4 xj, float4 vj, float invRho) {
    grad_hit(d, a, g, x, y, z, xj, vj, invRho);
  });
  if (l.valid) grad_store(a, K, g, l.finite, out + l.index * SPH_GRADIENT_WORDS);
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

int sphk_gradient_points(sph_solver* s, const SampleArgs& a, float K, const float* pts4, int count, float* out) {
  if (count <= 0) return SPH_OK;
  hipLaunchKernelGGL(k_gradient_points, dim3(sph_blocks(count)), dim3(SPH_BLOCK), 0, s->stream, s->d, a, K, (const float4*)pts4, count,
                     out);
  SPH_HIP(hipGetLastError());
  return SPH_OK;
}

int sphk_gradient_grid(sph_solver* s, const SampleArgs& a, float K, const float origin[3], const float spacing[3], int nx, int ny,
                       int kBase, int nz, float* out) {
  return sample_launch_grid(
      s, a, origin, spacing, nx, ny, kBase, nz, "sph_sample_gradient_grid",
      [&](const SampleArgs& g, int nbx, int nby, int nb) {
        hipLaunchKernelGGL(k_gradient_grid, dim3((unsigned)nb), dim3(SPH_SAMPLE_WAVE), 0, s->stream, s->d, g, K, nbx, nby, nb, out);
      },
      [&](const SampleArgs& g, unsigned blocks) {
        hipLaunchKernelGGL(k_gradient_grid_points, dim3(blocks), dim3(SPH_BLOCK), 0, s->stream, s->d, g, K, out);
      });
}

int sphk_surface_normals(sph_solver* s, const SampleArgs& a, float K, int field, const float* verts, int count, float* normals) {
  if (count <= 0) return SPH_OK;
  hipLaunchKernelGGL(k_surface_normals, dim3(sph_blocks(count)), dim3(SPH_BLOCK), 0, s->stream, s->d, a, K, field, verts, count,
                     normals);
  SPH_HIP(hipGetLastError());
  return SPH_OK;
}

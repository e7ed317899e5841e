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

// One point through the point walk (sph_sample_walk.h): zero sums, a hit per selected particle, the record.
__device__ void sample_one(const SphDev& d, const SampleArgs& a, float px, float py, float pz, float* out) {
  SampleAcc acc = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0};
  sample_point_walk(d, a, px, py, pz, [&](float x, float y, float z, float4 xj, float4 vj, float invRho) {
    sample_hit(d, a, acc, x, y, z, xj, vj, invRho);
  });
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
  float px, py, pz;
  if (!sample_grid_point(a, i, px, py, pz)) return;
  sample_one(d, a, px, py, pz, out + (size_t)i * SPH_SAMPLE_WORDS);
}

// The hot path: one wave per 4x4x4 brick of grid points through the brick walk (sph_sample_walk.h).
__global__ __launch_bounds__(SPH_SAMPLE_WAVE) void k_sample_grid(SphDev d, SampleArgs a, int nbx, int nby, int nblocks,
                                                                 float* __restrict__ out) {
  SampleAcc acc = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0};
  const SampleBrickLane l = sample_brick_walk(d, a, nbx, nby, nblocks, [&](float x, float y, float z, float4 xj, float4 vj, float invRho) {
    sample_hit(d, a, acc, x, y, z, xj, vj, invRho);
  });
  if (l.valid) sample_store(a, acc, out + l.index * SPH_SAMPLE_WORDS);
}

int sphk_sample_points(sph_solver* s, const SampleArgs& a, const float* pts4, int count, float* out) {
  if (count <= 0) return SPH_OK;
  hipLaunchKernelGGL(k_sample_points, dim3(sph_blocks(count)), dim3(SPH_BLOCK), 0, s->stream, s->d, a, (const float4*)pts4, count, out);
  SPH_HIP(hipGetLastError());
  return SPH_OK;
}

int sphk_sample_grid(sph_solver* s, const SampleArgs& a, const float origin[3], const float spacing[3], int nx, int ny,
                     int kBase, int nz, float* out) {
  return sample_launch_grid(
      s, a, origin, spacing, nx, ny, kBase, nz, "sph_sample_grid",
      [&](const SampleArgs& g, int nbx, int nby, int nb) {
        hipLaunchKernelGGL(k_sample_grid, dim3((unsigned)nb), dim3(SPH_SAMPLE_WAVE), 0, s->stream, s->d, g, nbx, nby, nb, out);
      },
      [&](const SampleArgs& g, unsigned blocks) {
        hipLaunchKernelGGL(k_sample_grid_points, dim3(blocks), dim3(SPH_BLOCK), 0, s->stream, s->d, g, out);
      });
}

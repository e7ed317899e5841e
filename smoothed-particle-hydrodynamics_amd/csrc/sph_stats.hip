// Time statistics on a lattice: the sample record of every lattice point folded, call by call, into 24 double accumulators per node
// that stay on the device (include/sphmi.h: sph_stats_*). Read-only on every solver array. The record is the
// sampling contract's: the walks of sph_sample_walk.h with the hit of sph_sample.hip, so the folded words are those of
// sph_sample_grid bit for bit; no record is written anywhere.
//   k_stats_grid         one wave per 4x4x4 brick of the whole lattice (the brick walk); after the walk a wet lane (n > 0) reads its
//                        node's 192 bytes as twelve 16-byte words, folds and writes them back. A dry lane touches no memory.
//   k_stats_grid_points  the same fold behind the point walk, one lane per node: lattices with a spacing above 2h/3
//   k_stats_init         the empty values (+0, -1, -inf, +inf: no byte pattern a memset could write)
//   k_stats_moments      the 16 float moment words of a window of nodes, in double, one rounded operation at a time
// Every node belongs to exactly one lane of one launch, and launches on the solver's stream run in order: no atomics.
#include "sph_sample_walk.h"

// The record of sample_store in registers: rho, vx, vy, vz, p as doubles (every float is exact in double), n as counted.
struct StatsRecord {
  double rho, vx, vy, vz, p;
};

__device__ __forceinline__ StatsRecord stats_record(const SampleArgs& a, const SampleAcc& acc) {
  alignas(16) float rec[SPH_SAMPLE_WORDS];
  sample_store(a, acc, rec);
  return StatsRecord{(double)rec[0], (double)rec[2], (double)rec[3], (double)rec[4], (double)rec[5]};
}

// One wet record into the node's 24 words at call index c (the table of include/sphmi.h). Every product is of two floats widened
// to double: exact, so the sums see the same addends with or without contraction.
__device__ __forceinline__ void stats_fold(double* __restrict__ node, const StatsRecord& r, double c) {
  double2* w = reinterpret_cast<double2*>(node);
  double2 a0 = w[0], a1 = w[1], a2 = w[2], a3 = w[3], a4 = w[4], a5 = w[5];
  double2 a6 = w[6], a7 = w[7], a8 = w[8], a9 = w[9], a10 = w[10], a11 = w[11];
  a0.x += 1.0;                                  // 0: wet calls
  if (a0.y < 0.0) a0.y = c;                     // 1: first wet call
  a1.x = c;                                     // 2: last wet call
  a1.y += r.rho;                                // 3
  a2.x += r.rho * r.rho;                        // 4
  a2.y += r.vx; a3.x += r.vy; a3.y += r.vz;     // 5..7
  a4.x += r.vx * r.vx; a4.y += r.vy * r.vy; a5.x += r.vz * r.vz;  // 8..10: xx, yy, zz
  a5.y += r.vx * r.vy; a6.x += r.vx * r.vz; a6.y += r.vy * r.vz;  // 11..13: xy, xz, yz
  a7.x += r.p;                                  // 14
  a7.y += r.p * r.p;                            // 15
  if (r.rho > a8.x) { a8.x = r.rho; a8.y = c; }  // 16, 17
  const double q = (r.vx * r.vx + r.vy * r.vy) + r.vz * r.vz;
  if (q > a9.x) { a9.x = q; a9.y = c; }          // 18, 19
  if (r.p > a10.x) { a10.x = r.p; a10.y = c; }   // 20, 21
  if (r.p < a11.x) { a11.x = r.p; a11.y = c; }   // 22, 23
  w[0] = a0; w[1] = a1; w[2] = a2; w[3] = a3; w[4] = a4; w[5] = a5;
  w[6] = a6; w[7] = a7; w[8] = a8; w[9] = a9; w[10] = a10; w[11] = a11;
}

__global__ __launch_bounds__(SPH_SAMPLE_WAVE) void k_stats_grid(SphDev d, SampleArgs a, int nbx, int nby, int nblocks, double call,
                                                                double* __restrict__ acc24) {
  SampleAcc acc = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0};
  const SampleBrickLane l = sample_brick_walk(d, a, nbx, nby, nblocks, [&](float x, float y, float z, float4 xj, float4 vj, float invRho) {
    sample_hit(d, a, acc, x, y, z, xj, vj, invRho);
  });
  if (l.valid && acc.n > 0) stats_fold(acc24 + l.index * SPH_STATS_WORDS, stats_record(a, acc), call);
}

__global__ __launch_bounds__(SPH_BLOCK) void k_stats_grid_points(SphDev d, SampleArgs a, double call, double* __restrict__ acc24) {
  const long long i = (long long)blockIdx.x * SPH_BLOCK + threadIdx.x;
  float px, py, pz;
  if (!sample_grid_point(a, i, px, py, pz)) return;
  SampleAcc acc = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0};
  sample_point_walk(d, a, px, py, pz, [&](float x, float y, float z, float4 xj, float4 vj, float invRho) {
    sample_hit(d, a, acc, x, y, z, xj, vj, invRho);
  });
  if (acc.n > 0) stats_fold(acc24 + (size_t)i * SPH_STATS_WORDS, stats_record(a, acc), call);
}

// One thread per 16-byte pair of words: pair p of a node holds words 2p and 2p + 1.
__global__ __launch_bounds__(SPH_BLOCK) void k_stats_init(double2* __restrict__ acc, long long pairs) {
  const long long i = (long long)blockIdx.x * SPH_BLOCK + threadIdx.x;
  if (i >= pairs) return;
  const int p = (int)(i % (SPH_STATS_WORDS / 2));
  const double inf = __builtin_inf();
  double2 v = make_double2(0.0, 0.0);
  if (p == 0) v.y = -1.0;                              // 1
  else if (p == 1) v.x = -1.0;                         // 2
  else if (p >= 8 && p <= 10) v = make_double2(-inf, -1.0);  // 16..21
  else if (p == 11) v = make_double2(inf, -1.0);       // 22, 23
  acc[i] = v;
}

// node: the window's first node in the accumulators; out: count x SPH_STATS_MOMENT_WORDS floats
__global__ __launch_bounds__(SPH_BLOCK) void k_stats_moments(const double* __restrict__ node, long long count, double calls,
                                                             float* __restrict__ out) {
  const long long i = (long long)blockIdx.x * SPH_BLOCK + threadIdx.x;
  if (i >= count) return;
  const double2* w = reinterpret_cast<const double2*>(node + (size_t)i * SPH_STATS_WORDS);
  const double2 a0 = w[0], a1 = w[1], a2 = w[2], a3 = w[3], a4 = w[4], a5 = w[5], a6 = w[6], a7 = w[7], a10 = w[10];
  const double n = a0.x, C = calls;
  const double mr = a1.y / C;
  float4 o0 = make_float4((float)(n / C), (float)mr, (float)(a2.x / C - mr * mr), 0.f);
  float4 o1 = make_float4(0.f, 0.f, 0.f, 0.f), o2 = o1, o3 = make_float4(0.f, 0.f, -1.f, 0.f);
  if (n > 0.0) {
    const double mx = a2.y / n, my = a3.x / n, mz = a3.y / n, mp = a7.x / n;
    o0.w = (float)mx; o1.x = (float)my; o1.y = (float)mz;
    o1.z = (float)(a4.x / n - mx * mx); o1.w = (float)(a4.y / n - my * my); o2.x = (float)(a5.x / n - mz * mz);
    o2.y = (float)(a5.y / n - mx * my); o2.z = (float)(a6.x / n - mx * mz); o2.w = (float)(a6.y / n - my * mz);
    o3.x = (float)mp; o3.y = (float)(a7.y / n - mp * mp);
    o3.z = (float)a0.y; o3.w = (float)a10.x;
  }
  float4* o = reinterpret_cast<float4*>(out + (size_t)i * SPH_STATS_MOMENT_WORDS);
  o[0] = o0; o[1] = o1; o[2] = o2; o[3] = o3;
}

int sphk_stats_accumulate(sph_solver* s, const SampleArgs& a, const sph_stats_lattice& g, int64_t call, double* acc) {
  const double c = (double)call;
  return sample_launch_grid(
      s, a, g.origin, g.spacing, g.dims[0], g.dims[1], 0, g.dims[2], "sph_stats_accumulate",
      [&](const SampleArgs& q, int nbx, int nby, int nb) {
        hipLaunchKernelGGL(k_stats_grid, dim3((unsigned)nb), dim3(SPH_SAMPLE_WAVE), 0, s->stream, s->d, q, nbx, nby, nb, c, acc);
      },
      [&](const SampleArgs& q, unsigned blocks) {
        hipLaunchKernelGGL(k_stats_grid_points, dim3(blocks), dim3(SPH_BLOCK), 0, s->stream, s->d, q, c, acc);
      });
}

int sphk_stats_init(sph_solver* s, double* acc, int64_t nodes) {
  const long long pairs = (long long)nodes * (SPH_STATS_WORDS / 2);
  hipLaunchKernelGGL(k_stats_init, dim3((unsigned)((pairs + SPH_BLOCK - 1) / SPH_BLOCK)), dim3(SPH_BLOCK), 0, s->stream,
                     reinterpret_cast<double2*>(acc), pairs);
  SPH_HIP(hipGetLastError());
  return SPH_OK;
}

int sphk_stats_moments(sph_solver* s, const double* node, int64_t count, int64_t calls, float* out) {
  if (count <= 0) return SPH_OK;
  hipLaunchKernelGGL(k_stats_moments, dim3((unsigned)((count + SPH_BLOCK - 1) / SPH_BLOCK)), dim3(SPH_BLOCK), 0, s->stream, node,
                     (long long)count, (double)calls, out);
  SPH_HIP(hipGetLastError());
  return SPH_OK;
}

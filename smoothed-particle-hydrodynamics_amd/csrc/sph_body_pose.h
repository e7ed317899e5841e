// One member of a body under a pose (include/sphmi.h: sph_body_set_pose) as one device function, for the two
// kernels that place bodies: k_body_pose (sph_body.hip, the pose comes with the launch) and k_bdyn_pose (sph_body_dynamics.hip, the
// pose comes from device memory). Validation and commit share the expressions, so they cannot drift apart.
#pragma once
#include "sph_common.h"

#define BODY_WAVE 64
#define BODY_WAVES (SPH_BLOCK / BODY_WAVE)

// the contract's expressions, one float operation each in the written order (the build has -ffp-contract=off)
__device__ __forceinline__ float body_row(const float* m, float x, float y, float z) { return (m[0] * x + m[1] * y) + m[2] * z; }

// Member k = blockIdx.x * SPH_BLOCK + threadIdx.x, called by every lane of the block.
// COMMIT false: counters[0] += failing members, counters[1] = min(failing member), counters[2] = max(bits of d2), one atomic per
// wave and counter; COMMIT true: the stores
template <bool COMMIT>
__device__ __forceinline__ void body_pose_member(const BodyPose& a, const uint32_t* __restrict__ ids, const float4* __restrict__ ref,
                                                 int count, int N, float4* __restrict__ pos, float4* __restrict__ vel,
                                                 uint32_t* __restrict__ counters) {
  const int k = blockIdx.x * SPH_BLOCK + threadIdx.x;
  const bool live = k < count;
  uint32_t o = 0;
  float4 p = make_float4(0.f, 0.f, 0.f, 0.f);
  if (live) {
    o = ids[k];
    p = ref[2 * (size_t)k];
  }
  const float x = body_row(a.m, p.x, p.y, p.z) + a.m[3];
  const float y = body_row(a.m + 4, p.x, p.y, p.z) + a.m[7];
  const float z = body_row(a.m + 8, p.x, p.y, p.z) + a.m[11];
  const bool inRange = live && o < (uint32_t)N;  // (o < N always: the edits carry the bodies; the test keeps the accesses inside)
  if (COMMIT) {
    if (!inRange) return;
    const float4 n = ref[2 * (size_t)k + 1];
    pos[o] = make_float4(x, y, z, p.w);
    vel[o] = make_float4(body_row(a.m, n.x, n.y, n.z), body_row(a.m + 4, n.x, n.y, n.z), body_row(a.m + 8, n.x, n.y, n.z), n.w);
    return;
  }
  const bool finite = isfinite(x) && isfinite(y) && isfinite(z);
  const bool inside = x >= a.xmin && x <= a.xmax && y >= a.ymin && y <= a.ymax && z >= a.zmin && z <= a.zmax;
  const bool bad = live && (!inRange || !finite || (a.wide && !inside));
  uint32_t d2bits = 0u;
  if (inRange && !bad) {
    const float4 c = pos[o];
    const float dx = x - c.x, dy = y - c.y, dz = z - c.z;
    d2bits = __float_as_uint((dx * dx + dy * dy) + dz * dz);  // >= +0 or NaN: as integers the patterns order like the floats
  }
  const unsigned long long badWord = __ballot(bad);
#pragma unroll
  for (int s = BODY_WAVE / 2; s > 0; s >>= 1) d2bits = max(d2bits, (uint32_t)__shfl_xor((int)d2bits, s, BODY_WAVE));
  if ((threadIdx.x & (BODY_WAVE - 1)) != 0) return;
  if (badWord) {
    atomicAdd(&counters[0], (uint32_t)__popcll(badWord));
    atomicMin(&counters[1], (uint32_t)(k + __ffsll((long long)badWord) - 1));  // k: the wave's first member
  }
  if (d2bits) atomicMax(&counters[2], d2bits);
}

// Integral curves of the sampled velocity field: streamlines of the frozen field from seed points, and tracers that are advanced
// one step per call (include/sphmi.h: sph_trace_streamlines / sph_tracers_*). Read-only on every solver array.
//
// Both kernels run one device function, trace_run: the step of the contract (items 1-7 of sphmi.h) as a loop over STAGES, each of
// which samples the velocity at one point through the point walk of sph_sample_walk.h. A midpoint step is two stages, so the walk
// is inlined once and lanes of a wave that are in different stages of their curves still share its instructions. The arithmetic
// is the sampling contract's (S, Ux, Uy, Uz of sample_hit in ascending sorted index; W, P and the count do not influence them and
// are not formed), so a vertex equals what a host loop over sph_sample_points computes, bit for bit.
#include "sph_sample_walk.h"

#ifndef SPH_TRACE_BLOCK     // (a variant build may set it, to measure: make variant EXTRA=-DSPH_TRACE_BLOCK=256)
#define SPH_TRACE_BLOCK 64  // one wave per block: a few thousand curves reach every CU
#endif

// velocity(p): whether S != 0, and then u = U / S
__device__ __forceinline__ bool trace_velocity(const SphDev& d, const SampleArgs& a, float px, float py, float pz, float& ux,
                                               float& uy, float& uz) {
  float S = 0.f, Ux = 0.f, Uy = 0.f, Uz = 0.f;
  sample_point_walk(d, a, px, py, pz, [&](float x, float y, float z, float4 xj, float4 vj, float invRho) {
    const float dx = x - xj.x, dy = y - xj.y, dz = z - xj.z;
    const float r2 = dx * dx + dy * dy + dz * dz;
    if (r2 < a.hh) {
      const float t = d.hs2 - r2 * a.ss2;
      const float w = t * t * t;
      const float v = w * invRho;
      S += v;
      Ux += v * vj.x; Uy += v * vj.y; Uz += v * vj.z;
    }
  });
  if (S == 0.f) return false;
  ux = Ux / S; uy = Uy / S; uz = Uz / S;
  return true;
}

__device__ __forceinline__ bool trace_in_region(const TraceArgs& t, float x, float y, float z) {
  return t.box[0] <= x && x <= t.box[3] && t.box[1] <= y && y <= t.box[4] && t.box[2] <= z && z <= t.box[5];
}

// The curve from (px, py, pz), its vertex 0: vertex(k, x, y, z, s) for every vertex k = 0, 1, ... as it is reached, until the
// curve stops (the code is returned, the position is that of the last vertex) or, with limit < 0, until it has advanced once
// (SPH_TRACE_MOVING, the position is p_1). limit >= 0: the maxSteps of item 6.
template <typename Vertex>
__device__ __forceinline__ int trace_run(const SphDev& d, const SampleArgs& a, const TraceArgs& t, float& px, float& py, float& pz,
                                         int limit, Vertex vertex) {
  int k = 0;
  bool mid = false;                  // the stage samples the midpoint q of a step, not the vertex p_k
  float qx = px, qy = py, qz = pz;   // where the stage samples
  for (;;) {
    if (!sample_finite(qx, qy, qz)) {
      if (!mid) vertex(k, px, py, pz, 0.f);
      return SPH_TRACE_NONFINITE;
    }
    float ux = 0.f, uy = 0.f, uz = 0.f;
    const bool hit = trace_velocity(d, a, qx, qy, qz, ux, uy, uz);
    const float s = hit ? sqrtf(ux * ux + uy * uy + uz * uz) : 0.f;
    if (!mid) {
      vertex(k, px, py, pz, s);
      if (!hit) return SPH_TRACE_LEFT_MATTER;
      if (t.hasRegion && !trace_in_region(t, px, py, pz)) return SPH_TRACE_LEFT_REGION;
      if (!(s > t.minSpeed)) return SPH_TRACE_STAGNANT;
      if (k == limit) return SPH_TRACE_MAX_STEPS;
      const float c = t.mode == SPH_TRACE_ARC ? t.step / s : t.step;
      if (t.integrator == SPH_TRACE_MIDPOINT) {
        const float hc = 0.5f * c;
        qx = px + hc * ux; qy = py + hc * uy; qz = pz + hc * uz;
        mid = true;
        continue;
      }
      px = px + c * ux; py = py + c * uy; pz = pz + c * uz;
    } else {
      if (!hit) return SPH_TRACE_LEFT_MATTER;
      if (!(s > t.minSpeed)) return SPH_TRACE_STAGNANT;
      const float c = t.mode == SPH_TRACE_ARC ? t.step / s : t.step;
      px = px + c * ux; py = py + c * uy; pz = pz + c * uz;
      mid = false;
    }
    if (limit < 0) return SPH_TRACE_MOVING;
    k++;
    qx = px; qy = py; qz = pz;
  }
}

// One lane per curve, the whole curve inside the launch. Curve-major vertices: lane i writes 16 bytes per vertex at a stride of
// (maxSteps + 1) * 16 bytes between lanes, which is the host layout, so the piece is copied out as it lies.
__global__ __launch_bounds__(SPH_TRACE_BLOCK) void k_trace_streamlines(SphDev d, SampleArgs a, TraceArgs t,
                                                                       const float4* __restrict__ seeds, int count,
                                                                       float4* __restrict__ verts, int32_t* __restrict__ lengths,
                                                                       int32_t* __restrict__ status) {
  const int i = blockIdx.x * SPH_TRACE_BLOCK + threadIdx.x;
  if (i >= count) return;
  const float4 p = seeds[i];
  float px = p.x, py = p.y, pz = p.z;
  float4* curve = verts + (size_t)i * (size_t)(t.maxSteps + 1);
  int n = 0;
  const int code = trace_run(d, a, t, px, py, pz, t.maxSteps, [&](int k, float x, float y, float z, float s) {
    curve[k] = make_float4(x, y, z, s);  // k <= maxSteps: trace_run stops at k == limit before it advances
    n = k + 1;
  });
  lengths[i] = n;
  status[i] = code;
}

// The same step, once per tracer that is still moving.
__global__ __launch_bounds__(SPH_TRACE_BLOCK) void k_tracers_advect(SphDev d, SampleArgs a, TraceArgs t, float4* __restrict__ pos,
                                                                    int32_t* __restrict__ status, int32_t* __restrict__ steps,
                                                                    int count, uint32_t* __restrict__ moving) {
  const int i = blockIdx.x * SPH_TRACE_BLOCK + threadIdx.x;
  if (i >= count || status[i] != SPH_TRACE_MOVING) return;
  const float4 p = pos[i];
  float px = p.x, py = p.y, pz = p.z, speed = 0.f;
  const int code = trace_run(d, a, t, px, py, pz, -1, [&](int, float, float, float, float s) { speed = s; });
  pos[i] = make_float4(px, py, pz, speed);
  status[i] = code;
  steps[i] = steps[i] + 1;
  if (code == SPH_TRACE_MOVING) atomicAdd(moving, 1u);
}

int sphk_trace_streamlines(sph_solver* s, const SampleArgs& a, const TraceArgs& t, const float* seeds4, int count, float* verts,
                           int32_t* lengths, int32_t* status) {
  if (count <= 0) return SPH_OK;
  hipLaunchKernelGGL(k_trace_streamlines, dim3(sph_blocks(count, SPH_TRACE_BLOCK)), dim3(SPH_TRACE_BLOCK), 0, s->stream, s->d, a, t,
                     (const float4*)seeds4, count, (float4*)verts, lengths, status);
  SPH_HIP(hipGetLastError());
  return SPH_OK;
}

int sphk_tracers_advect(sph_solver* s, const SampleArgs& a, const TraceArgs& t, float* pos4, int32_t* status, int32_t* steps,
                        int count, uint32_t* moving) {
  if (count <= 0) return SPH_OK;
  hipLaunchKernelGGL(k_tracers_advect, dim3(sph_blocks(count, SPH_TRACE_BLOCK)), dim3(SPH_TRACE_BLOCK), 0, s->stream, s->d, a, t,
                     (float4*)pos4, status, steps, count, moving);
  SPH_HIP(hipGetLastError());
  return SPH_OK;
}

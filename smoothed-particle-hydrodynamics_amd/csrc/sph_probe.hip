// Probes: point samples and water levels on lines, recorded once per call into a current-record buffer and a history ring
// (include/sphmi.h: sph_probes_*). Read-only on every solver array. Every record is the sampling contract's: the
// points go through the point walk of sph_sample_walk.h with the hit of sph_sample.hip, so the sums are those of
// sph_sample_points bit for bit.
//   k_probe_points   one lane per point: its 8-word record
//   k_probe_levels   one wave per line, four lines per block: the line's points in chunks of 64 from the far end, lane l of chunk
//                    c at k = count - 1 - 64c - l, so neighbouring lanes walk the same cells. The far end decides SUBMERGED; below
//                    it every point above the first inside one is outside, so that point is K and its upper neighbour's f comes
//                    from the lane in front of it, or from the chunk before (the seam value carried in a register; no point is
//                    sampled twice). The wave stops at the first chunk that holds an inside point: the ballot is wave-uniform, and
//                    no barrier stands in the loop, because the waves of a block stop at different chunks.
// Both write the record twice: into the current-record buffer the blocking copy reads, and into the ring's row if there is one.
#include "sph_sample_walk.h"

#define PROBE_LINES_PER_BLOCK (SPH_BLOCK / SPH_SAMPLE_WAVE)

// the sample record at (px, py, pz) into registers, through the stores of sample_store
__device__ __forceinline__ void probe_sample(const SphDev& d, const SampleArgs& a, float px, float py, float pz, float4& r0, float4& r1) {
  SampleAcc acc = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0};
  sample_point_walk(d, a, px, py, pz, [&](float x, float y, float z, float4 xj, float4 vj, float invRho) {
    sample_hit(d, a, acc, x, y, z, xj, vj, invRho);
  });
  alignas(16) float rec[SPH_SAMPLE_WORDS];
  sample_store(a, acc, rec);
  r0 = make_float4(rec[0], rec[1], rec[2], rec[3]);
  r1 = make_float4(rec[4], rec[5], rec[6], rec[7]);
}

__device__ __forceinline__ void probe_write(float* __restrict__ cur, float* __restrict__ row, size_t record, float4 r0, float4 r1) {
  float4* c = reinterpret_cast<float4*>(cur + record * SPH_PROBE_LEVEL_WORDS);
  c[0] = r0; c[1] = r1;
  if (row) {
    float4* h = reinterpret_cast<float4*>(row + record * SPH_PROBE_LEVEL_WORDS);
    h[0] = r0; h[1] = r1;
  }
}

__global__ __launch_bounds__(SPH_BLOCK) void k_probe_points(SphDev d, SampleArgs a, const float4* __restrict__ pts, int count,
                                                            float* __restrict__ cur, float* __restrict__ row) {
  const int i = blockIdx.x * SPH_BLOCK + threadIdx.x;
  if (i >= count) return;
  const float4 p = pts[i];
  float4 r0, r1;
  probe_sample(d, a, p.x, p.y, p.z, r0, r1);
  probe_write(cur, row, (size_t)i, r0, r1);
}

__device__ __forceinline__ float probe_word(float4 r0, float4 r1, int field) {
  switch (field) {
    case 0: return r0.x;
    case 1: return r0.y;
    case 2: return r0.z;
    case 3: return r0.w;
    case 4: return r1.x;
    default: return r1.y;
  }
}

// records: the line records of the current buffer / the ring's row (behind the point records)
__global__ __launch_bounds__(SPH_BLOCK) void k_probe_levels(SphDev d, SampleArgs a, const sph_probe_line* __restrict__ lines, int count,
                                                            float* __restrict__ cur, float* __restrict__ row) {
  const int lane = threadIdx.x & (SPH_SAMPLE_WAVE - 1);
  const int line = __builtin_amdgcn_readfirstlane(blockIdx.x * PROBE_LINES_PER_BLOCK + (int)(threadIdx.x / SPH_SAMPLE_WAVE));
  if (line >= count) return;
  const sph_probe_line L = lines[line];  // wave-uniform
  a.typeMask = L.typeMask;
  const int n = L.count, field = L.field;
  const float iso = L.iso;
  const float ox = L.origin[0], oy = L.origin[1], oz = L.origin[2], sx = L.step[0], sy = L.step[1], sz = L.step[2];
  float seam = 0.f;  // f of the lowest point of the chunk before: the upper neighbour of this chunk's lane 0
  float4 r0, r1;
  for (int top = n - 1;; top -= SPH_SAMPLE_WAVE) {  // top: the chunk's highest k; wave-uniform
    if (top < 0) {                                  // every point was outside
      r0 = make_float4(ox + 0.0f * sx, oy + 0.0f * sy, oz + 0.0f * sz, 0.f);
      r1 = make_float4((float)SPH_PROBE_DRY, -1.f, 0.f, 0.f);
      break;
    }
    const int k = top - lane;
    float f = 0.f;
    bool inside = false;
    if (k >= 0) {
      float4 s0, s1;
      probe_sample(d, a, ox + (float)k * sx, oy + (float)k * sy, oz + (float)k * sz, s0, s1);
      f = probe_word(s0, s1, field);
      inside = f >= iso;  // (a NaN is outside)
    }
    const unsigned long long in = __ballot(inside);
    if (in) {
      const int hit = __ffsll((long long)in) - 1;  // the inside point nearest the far end
      const float fK = __shfl(f, hit, SPH_SAMPLE_WAVE);
      const float fUp = __shfl(f, max(hit - 1, 0), SPH_SAMPLE_WAVE);
      const int K = top - hit;
      if (K == n - 1) {
        const float e = (float)K;
        r0 = make_float4(ox + e * sx, oy + e * sy, oz + e * sz, e);
        r1 = make_float4((float)SPH_PROBE_SUBMERGED, e, fK, 0.f);
      } else {
        const float fK1 = hit ? fUp : seam;
        const float t = (iso - fK) / (fK1 - fK);
        const float e0 = (float)K, e1 = (float)(K + 1);
        const float x0 = ox + e0 * sx, y0 = oy + e0 * sy, z0 = oz + e0 * sz;
        const float x1 = ox + e1 * sx, y1 = oy + e1 * sy, z1 = oz + e1 * sz;
        r0 = make_float4(x0 + t * (x1 - x0), y0 + t * (y1 - y0), z0 + t * (z1 - z0), e0 + t);
        r1 = make_float4((float)SPH_PROBE_FOUND, e0, fK, fK1);
      }
      break;
    }
    seam = __shfl(f, SPH_SAMPLE_WAVE - 1, SPH_SAMPLE_WAVE);  // (the last chunk alone may be short, and nothing follows it)
  }
  if (lane == 0) probe_write(cur, row, (size_t)line, r0, r1);
}

int sphk_probe_points(sph_solver* s, const SampleArgs& a, const float* pts4, int count, float* cur, float* row) {
  if (count <= 0) return SPH_OK;
  hipLaunchKernelGGL(k_probe_points, dim3(sph_blocks(count)), dim3(SPH_BLOCK), 0, s->stream, s->d, a, (const float4*)pts4, count, cur, row);
  SPH_HIP(hipGetLastError());
  return SPH_OK;
}

int sphk_probe_levels(sph_solver* s, const SampleArgs& a, const sph_probe_line* lines, int count, float* cur, float* row) {
  if (count <= 0) return SPH_OK;
  hipLaunchKernelGGL(k_probe_levels, dim3(sph_blocks(count, PROBE_LINES_PER_BLOCK)), dim3(SPH_BLOCK), 0, s->stream, s->d, a, lines, count,
                     cur, row);
  SPH_HIP(hipGetLastError());
  return SPH_OK;
}

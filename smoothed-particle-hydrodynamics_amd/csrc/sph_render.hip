// Particle rendering: depth, id, colour and thickness images of the sorted state of the last completed step (include/sphmi.h:
// sph_render_particles / sph_read_render). Read-only on every solver array. The selection is sph_selector.h's.
//   k_render_clear    one lane per pixel: key = all ones (uncovered), thickness sum = 0
//   k_render_splat    one lane per sorted particle: selection, projection, then either the lane rasterises its clipped footprint
//                     (at most 8 x 8 pixels) or the particle goes to the queue of large splats (one counter bump per wave)
//   k_render_drain    fixed grid, one wave per queued splat, the lanes striding its clipped box; the queue length is read on the
//                     device, so the host does not wait between the two kernels
//   k_render_resolve  one lane per pixel: unpacks the winning key, recomputes the winner's fragment, colours and shades it and
//                     writes depth, sorted index, original id, rgba and the saturated thickness coalesced
// A pixel's key is the minimum of ((uint64)bits(depth) << 32) | sorted index over its fragments and its thickness the sum of
// integers: 64-bit integer atomics, whose results do not depend on the order they arrive in. No floating-point atomics.
// Projection and fragment are one inline function each, used by the three kernels that need them, so their bits cannot differ.
#include "sph_common.h"
#include "sph_selector.h"  // the selection rule and the quantity of colour mode 2

#include <algorithm>

#define RN_WAVE 64
#define RN_SMALL 8           // a clipped footprint of at most RN_SMALL x RN_SMALL pixels is rasterised by the particle's lane
#define RN_DRAIN_BLOCKS 1024 // x SPH_BLOCK / RN_WAVE waves drain the queue of large splats
#define RN_EMPTY 0xFFFFFFFFFFFFFFFFull

struct RenderSplat {
  float u, v, R2, cz;
  int x0, x1, y0, y1;  // the search box clipped to the image (empty when x0 > x1 or y0 > y1)
};

__device__ static const float kRenderRamp[5][3] = SPH_RENDER_FIELD_RAMP;
__device__ static const float kRenderPalette[SPH_RENDER_LABEL_COLOURS][3] = SPH_RENDER_LABEL_PALETTE;

// PROJECTION of the contract; false: the particle is not drawn
__device__ __forceinline__ bool render_project(const sph_render_view& w, const float4& p, RenderSplat& s) {
  const float dx = p.x - w.eye[0], dy = p.y - w.eye[1], dz = p.z - w.eye[2];
  const float cx = (dx * w.right[0] + dy * w.right[1]) + dz * w.right[2];
  const float cy = (dx * w.up[0] + dy * w.up[1]) + dz * w.up[2];
  const float cz = (dx * w.forward[0] + dy * w.forward[1]) + dz * w.forward[2];
  const float k = w.projection ? w.scale / cz : w.scale;
  s.u = cx * k + w.centre[0];
  s.v = w.centre[1] - cy * k;
  const float R = w.radius * k;
  s.R2 = R * R;
  s.cz = cz;
  if (!(cz > w.nearPlane && R > 0.f && R <= w.maxRadiusPx && fabsf(s.u) < 1048576.f && fabsf(s.v) < 1048576.f)) return false;
  // |u|, |v| < 2^20 and R <= 4096: every bound below is an int
  s.x0 = max((int)floorf(s.u - R) - 1, 0);
  s.x1 = min((int)floorf(s.u + R) + 1, w.width - 1);
  s.y0 = max((int)floorf(s.v - R) - 1, 0);
  s.y1 = min((int)floorf(s.v + R) + 1, w.height - 1);
  return true;
}

// FRAGMENT of the contract at pixel (px, py); false: none
__device__ __forceinline__ bool render_fragment(const sph_render_view& w, const RenderSplat& s, int px, int py, float& nz, float& depth) {
  const float dx = ((float)px + 0.5f) - s.u, dy = ((float)py + 0.5f) - s.v;
  const float d2 = dx * dx + dy * dy;
  if (!(d2 <= s.R2)) return false;
  nz = sqrtf(1.0f - d2 / s.R2);
  depth = s.cz - w.radius * nz;
  return depth > w.nearPlane;
}

// The plain load may return a stale cached key; keys only decrease within a render, so a stale one is never below the true one
// and a fragment that does not beat it cannot beat the true one either.
template <bool THICK>
__device__ __forceinline__ void render_emit(unsigned long long* keys, unsigned long long* thick, size_t pixel, float depth, float nz, int j) {
  const unsigned long long key = ((unsigned long long)__float_as_uint(depth) << 32) | (unsigned long long)(uint32_t)j;
  if (key < keys[pixel]) __hip_atomic_fetch_min(&keys[pixel], key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (THICK) atomicAdd(&thick[pixel], (unsigned long long)(uint32_t)(int)(nz * 256.0f + 0.5f));
}

__global__ __launch_bounds__(SPH_BLOCK) void k_render_clear(int pixels, unsigned long long* __restrict__ keys,
                                                            unsigned long long* __restrict__ thick) {
  const int p = blockIdx.x * SPH_BLOCK + threadIdx.x;
  if (p >= pixels) return;
  keys[p] = RN_EMPTY;
  if (thick) thick[p] = 0ull;
}

// head: [0] particles drawn, [1] covered pixels (k_render_resolve), [2] length of the queue
template <bool THICK>
__global__ __launch_bounds__(SPH_BLOCK) void k_render_splat(SphDev d, RenderArgs a, unsigned long long* keys, unsigned long long* thick,
                                                            uint32_t* __restrict__ head, int32_t* __restrict__ queue) {
  const int j = blockIdx.x * SPH_BLOCK + threadIdx.x;
  const int lane = threadIdx.x & (RN_WAVE - 1);
  RenderSplat s;
  bool drawn = false;
  if (j < d.N) {
    const float4 p = d.sortedPos[j];
    drawn = sph_selected(d, a.sel, j, p) && render_project(a.view, p, s);
  }
  const unsigned long long drawnWave = __ballot(drawn);
  if (lane == 0 && drawnWave) atomicAdd(&head[0], (uint32_t)__popcll(drawnWave));
  const bool inside = drawn && s.x0 <= s.x1 && s.y0 <= s.y1;
  const bool large = inside && (s.x1 - s.x0 >= RN_SMALL || s.y1 - s.y0 >= RN_SMALL);
  const unsigned long long largeWave = __ballot(large);
  if (largeWave) {  // (wave-uniform)
    uint32_t base = 0;
    if (lane == 0) base = atomicAdd(&head[2], (uint32_t)__popcll(largeWave));
    base = __shfl(base, 0);
    const uint32_t at = base + (uint32_t)__popcll(largeWave & ((1ull << lane) - 1ull));
    if (large && at < (uint32_t)d.N) queue[at] = j;  // (always: every particle is queued at most once)
  }
  if (!inside || large) return;
  for (int py = s.y0; py <= s.y1; py++)
    for (int px = s.x0; px <= s.x1; px++) {
      float nz, depth;
      if (render_fragment(a.view, s, px, py, nz, depth)) render_emit<THICK>(keys, thick, (size_t)py * a.view.width + px, depth, nz, j);
    }
}

template <bool THICK>
__global__ __launch_bounds__(SPH_BLOCK) void k_render_drain(SphDev d, RenderArgs a, unsigned long long* keys, unsigned long long* thick,
                                                            const uint32_t* __restrict__ head, const int32_t* __restrict__ queue) {
  const int lane = threadIdx.x & (RN_WAVE - 1);
  const uint32_t wave = (uint32_t)(blockIdx.x * SPH_BLOCK + threadIdx.x) / RN_WAVE, waves = gridDim.x * (SPH_BLOCK / RN_WAVE);
  const uint32_t count = min(head[2], (uint32_t)d.N);
  for (uint32_t q = wave; q < count; q += waves) {
    const int j = queue[q];
    if (j < 0 || j >= d.N) continue;
    RenderSplat s;
    if (!render_project(a.view, d.sortedPos[j], s)) continue;  // (never: it was drawn when it was queued)
    const int bw = s.x1 - s.x0 + 1, n = bw * (s.y1 - s.y0 + 1);  // <= 2^24 pixels
    for (int t = lane; t < n; t += RN_WAVE) {
      const int py = s.y0 + t / bw, px = s.x0 + t % bw;
      float nz, depth;
      if (render_fragment(a.view, s, px, py, nz, depth)) render_emit<THICK>(keys, thick, (size_t)py * a.view.width + px, depth, nz, j);
    }
  }
}

__device__ __forceinline__ void render_colour(const SphDev& d, const RenderArgs& a, int j, const float4& p, float c[3]) {
  const sph_render_view& w = a.view;
  if (w.colourMode == 0) {
    const int t = min(max((int)p.w, 1), 3);
    for (int k = 0; k < 3; k++) c[k] = w.typeColour[t - 1][k];
  } else if (w.colourMode == 1) {  // owWorldSimulation.cpp:127-141 as frames.density_colour states it
    const float rho0 = d.rho0, top = 2.0f * rho0;
    float rho = d.rho[j];
    rho = rho < 0.f ? 0.f : (rho > top ? top : rho);
    c[0] = 0.f; c[1] = 0.f; c[2] = 1.f;
    float dc;
    dc = (100.0f * (rho - rho0 * 1.00f)) / rho0; if (dc > 0.f) { c[0] = 0.f; c[1] = dc; c[2] = 1.f; }
    dc = (100.0f * (rho - rho0 * 1.01f)) / rho0; if (dc > 0.f) { c[0] = 0.f; c[1] = 1.f; c[2] = 1.f - dc; }
    dc = (100.0f * (rho - rho0 * 1.02f)) / rho0; if (dc > 0.f) { c[0] = dc; c[1] = 1.f; c[2] = 0.f; }
    dc = (100.0f * (rho - rho0 * 1.03f)) / rho0; if (dc > 0.f) { c[0] = 1.f; c[1] = 1.f - dc; c[2] = 0.f; }
    dc = (100.0f * (rho - rho0 * 1.04f)) / rho0; if (dc > 0.f) { c[0] = 1.f; c[1] = 0.f; c[2] = 0.f; }
  } else if (w.colourMode == 2) {
    const float q = sph_particle_quantity(d, w.field, j, p);
    const float s = fminf(fmaxf((q - w.lo) * a.inv, 0.f), 1.f);
    const float t = s * 4.0f;
    const int i = min((int)t, 3);
    const float f = t - (float)i;
    for (int k = 0; k < 3; k++) c[k] = kRenderRamp[i][k] + f * (kRenderRamp[i + 1][k] - kRenderRamp[i][k]);
  } else {
    const int label = a.labels[j];
    for (int k = 0; k < 3; k++) c[k] = label < 0 ? 0.5f : kRenderPalette[label % SPH_RENDER_LABEL_COLOURS][k];
  }
}

__global__ __launch_bounds__(SPH_BLOCK) void k_render_resolve(SphDev d, RenderArgs a, int pixels, const unsigned long long* __restrict__ keys,
                                                              const unsigned long long* __restrict__ thick, uint32_t* __restrict__ head,
                                                              float* __restrict__ depthOut, int32_t* __restrict__ indexOut,
                                                              uint32_t* __restrict__ idOut, uint32_t* __restrict__ rgbaOut,
                                                              uint32_t* __restrict__ thickOut) {
  const int p = blockIdx.x * SPH_BLOCK + threadIdx.x;
  const int lane = threadIdx.x & (RN_WAVE - 1);
  const sph_render_view& w = a.view;
  bool covered = false;
  if (p < pixels) {
    const unsigned long long key = keys[p];
    const int j = (int)(uint32_t)key;
    covered = key != RN_EMPTY && j >= 0 && j < d.N;
    float depth = INFINITY;
    int32_t index = -1;
    uint32_t id = 0xFFFFFFFFu;
    uint32_t rgba = (uint32_t)w.background[0] | ((uint32_t)w.background[1] << 8) | ((uint32_t)w.background[2] << 16) |
                    ((uint32_t)w.background[3] << 24);
    if (covered) {
      const float4 pos = d.sortedPos[j];
      RenderSplat s;
      render_project(w, pos, s);
      float nz = 0.f, again;
      render_fragment(w, s, p % w.width, p / w.width, nz, again);
      depth = __uint_as_float((uint32_t)(key >> 32));
      index = j;
      id = d.vals[j];
      float c[3];
      render_colour(d, a, j, pos, c);
      const float shade = w.ambient + (1.0f - w.ambient) * nz;
      rgba = 0xFF000000u;
      for (int k = 0; k < 3; k++) rgba |= (uint32_t)(int)(fminf(fmaxf(c[k] * shade, 0.f), 1.f) * 255.0f + 0.5f) << (8 * k);
    }
    depthOut[p] = depth;
    indexOut[p] = index;
    idOut[p] = id;
    rgbaOut[p] = rgba;
    if (thickOut) {
      const unsigned long long t = thick[p];
      thickOut[p] = t > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)t;
    }
  }
  const unsigned long long coveredWave = __ballot(covered);
  if (lane == 0 && coveredWave) atomicAdd(&head[1], (uint32_t)__popcll(coveredWave));
}

// ---- launchers ---------------------------------------------------------------------------------------------------------------
static size_t rn_align(size_t b) { return (b + 255) & ~(size_t)255; }

RenderLayout sphk_render_layout(int width, int height, bool thickness, int N) {
  const size_t P = (size_t)width * (size_t)height;
  RenderLayout L = {};
  size_t at = 0;
  L.head = at; at += 256;
  L.keys = at; at += rn_align(8 * P);
  if (thickness) { L.thick = at; at += rn_align(8 * P); }
  L.depth = at; at += rn_align(4 * P);
  L.index = at; at += rn_align(4 * P);
  L.origId = at; at += rn_align(4 * P);
  L.rgba = at; at += rn_align(4 * P);
  if (thickness) { L.thickOut = at; at += rn_align(4 * P); }
  L.queue = at; at += rn_align(4 * (size_t)std::max(N, 1));
  L.bytes = at;
  return L;
}

template <bool THICK>
static int render_scatter(sph_solver* s, const RenderArgs& a, unsigned long long* keys, unsigned long long* thick, uint32_t* head, int32_t* queue) {
  hipLaunchKernelGGL(k_render_splat<THICK>, dim3(sph_blocks(s->d.N)), dim3(SPH_BLOCK), 0, s->stream, s->d, a, keys, thick, head, queue);
  SPH_HIP(hipGetLastError());
  hipLaunchKernelGGL(k_render_drain<THICK>, dim3(RN_DRAIN_BLOCKS), dim3(SPH_BLOCK), 0, s->stream, s->d, a, keys, thick,
                     (const uint32_t*)head, (const int32_t*)queue);
  SPH_HIP(hipGetLastError());
  return SPH_OK;
}

int sphk_render(sph_solver* s, const RenderArgs& a, bool thickness, void* buf) {
  const RenderLayout L = sphk_render_layout(a.view.width, a.view.height, thickness, s->d.N);
  const int pixels = a.view.width * a.view.height;
  char* base = (char*)buf;
  uint32_t* head = (uint32_t*)(base + L.head);
  unsigned long long* keys = (unsigned long long*)(base + L.keys);
  unsigned long long* thick = thickness ? (unsigned long long*)(base + L.thick) : nullptr;
  SPH_HIP(hipMemsetAsync(head, 0, 256, s->stream));
  hipLaunchKernelGGL(k_render_clear, dim3(sph_blocks(pixels)), dim3(SPH_BLOCK), 0, s->stream, pixels, keys, thick);
  SPH_HIP(hipGetLastError());
  if (s->d.N > 0) {
    const int rc = thickness ? render_scatter<true>(s, a, keys, thick, head, (int32_t*)(base + L.queue))
                             : render_scatter<false>(s, a, keys, thick, head, (int32_t*)(base + L.queue));
    if (rc != SPH_OK) return rc;
  }
  hipLaunchKernelGGL(k_render_resolve, dim3(sph_blocks(pixels)), dim3(SPH_BLOCK), 0, s->stream, s->d, a, pixels,
                     (const unsigned long long*)keys, (const unsigned long long*)thick, head, (float*)(base + L.depth),
                     (int32_t*)(base + L.index), (uint32_t*)(base + L.origId), (uint32_t*)(base + L.rgba),
                     thickness ? (uint32_t*)(base + L.thickOut) : nullptr);
  SPH_HIP(hipGetLastError());
  return SPH_OK;
}

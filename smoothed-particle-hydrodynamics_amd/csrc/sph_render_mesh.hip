// Triangle rendering: the mesh of the last extraction or the membrane triangles drawn into the images of sph_render.hip, fresh or
// composed over them by depth (include/sphmi.h: sph_render_mesh / sph_read_render_triangles). Read-only on every
// solver array.
//   k_rm_points           one lane per mesh vertex: (x, y, z) -> the float4 query point the sampling kernel reads (colour mode 1)
//   k_rm_vertex_mesh      one lane per mesh vertex: projection, snap to 1/256 pixel, 1/cz; the position and the scalar beside them
//   k_rm_vertex_membrane  the same per membrane corner (vertex 3 t + k is corner k of triangle t), through backIndex
//   k_rm_raster           one lane per triangle: orientation, clipped box, counts; the lane rasterises a box of at most 8 x 8
//                         pixels, a larger triangle goes to the queue (one counter bump per wave)
//   k_rm_drain            fixed grid, one wave per queued triangle, the lanes striding its clipped box; the queue length is read on
//                         the device
//   k_rm_resolve          one lane per pixel: unpacks the winning key, recomputes the winner's fragment, shades it, compares it with
//                         the depth the image holds (compose) and writes depth, index, id, rgba and triangle coalesced
// Coverage is decided in integers: 64-bit edge functions of the snapped corners and the pixel centre, with the top-left rule on a
// zero. A pixel's key is the minimum of ((uint64)bits(depth) << 32) | triangle over its fragments: an integer atomic, whose result
// does not depend on the order of arrival. Set-up and fragment are one inline function each, used by the three kernels that need
// them, so their bits cannot differ.
#include "sph_common.h"
#include "sph_selector.h"  // the quantity of colour mode 1 on membranes

#include <algorithm>

#define RM_WAVE 64
#define RM_SMALL 8           // a clipped box of at most RM_SMALL x RM_SMALL pixels is rasterised by the triangle's lane
#define RM_DRAIN_BLOCKS 1024 // x SPH_BLOCK / RM_WAVE waves drain the queue of large triangles
#define RM_EMPTY 0xFFFFFFFFFFFFFFFFull

__device__ static const float kMeshRamp[5][3] = SPH_RENDER_FIELD_RAMP;

struct RmTri {
  int a, b, c;           // vertex ids, b and c exchanged when the table order is clockwise on the screen
  bool swapped;
  int Xa, Ya, Xb, Yb, Xc, Yc;
  float za, zb, zc;
  float A;               // (float)E(a, b, c) > 0
  int x0, x1, y0, y1;    // the box of the snapped corners in pixels, clipped to the image (empty when x0 > x1 or y0 > y1)
};

__device__ __forceinline__ long long rm_edge(int Xp, int Yp, int Xq, int Yq, int Xr, int Yr) {
  return (long long)(Xq - Xp) * (long long)(Yr - Yp) - (long long)(Yq - Yp) * (long long)(Xr - Xp);
}

// edge p -> q owns the pixel centres on its line
__device__ __forceinline__ bool rm_owns(int Xp, int Yp, int Xq, int Yq) {
  const int dx = Xq - Xp, dy = Yq - Yp;
  return dy > 0 || (dy == 0 && dx < 0);
}

// VERTICES of the contract: projection as render_project's first lines, then the snap
__device__ __forceinline__ RmVertex rm_project(const sph_render_view& w, float x, float y, float z) {
  const float dx = x - w.eye[0], dy = y - w.eye[1], dz = z - w.eye[2];
  const float cx = (dx * w.right[0] + dy * w.right[1]) + dz * w.right[2];
  const float cy = (dx * w.up[0] + dy * w.up[1]) + dz * w.up[2];
  const float cz = (dx * w.forward[0] + dy * w.forward[1]) + dz * w.forward[2];
  const float k = w.projection ? w.scale / cz : w.scale;
  const float u = cx * k + w.centre[0];
  const float v = w.centre[1] - cy * k;
  RmVertex r = {0, 0, 0.f, 0};
  if (!(cz > w.nearPlane && fabsf(u) < 1048576.f && fabsf(v) < 1048576.f)) return r;
  r.X = (int)floorf(u * 256.0f + 0.5f);  // |u| < 2^20: below 2^28 + 1 in magnitude
  r.Y = (int)floorf(v * 256.0f + 0.5f);
  r.zi = w.projection ? 1.0f / cz : cz;
  r.usable = 1;
  return r;
}

// TRIANGLE of the contract; false: skipped. T.x0.. are set whenever it returns true.
__device__ __forceinline__ bool rm_setup(const sph_render_view& w, const RmVertex* __restrict__ vtx, const int32_t* __restrict__ tris, int V,
                                         int t, RmTri& T) {
  T.a = tris ? tris[3 * (size_t)t] : 3 * t;
  T.b = tris ? tris[3 * (size_t)t + 1] : 3 * t + 1;
  T.c = tris ? tris[3 * (size_t)t + 2] : 3 * t + 2;
  if (T.a < 0 || T.a >= V || T.b < 0 || T.b >= V || T.c < 0 || T.c >= V) return false;  // (never: the ids are the extraction's own)
  const RmVertex a = vtx[T.a];
  RmVertex b = vtx[T.b], c = vtx[T.c];
  if (!(a.usable && b.usable && c.usable)) return false;
  long long A = rm_edge(a.X, a.Y, b.X, b.Y, c.X, c.Y);
  if (A == 0) return false;
  T.swapped = A < 0;
  if (T.swapped) {
    const RmVertex h = b; b = c; c = h;
    const int i = T.b; T.b = T.c; T.c = i;
    A = -A;
  }
  T.Xa = a.X; T.Ya = a.Y; T.Xb = b.X; T.Yb = b.Y; T.Xc = c.X; T.Yc = c.Y;
  T.za = a.zi; T.zb = b.zi; T.zc = c.zi;
  T.A = (float)A;
  T.x0 = max(min(a.X, min(b.X, c.X)) >> 8, 0);
  T.x1 = min(max(a.X, max(b.X, c.X)) >> 8, w.width - 1);
  T.y0 = max(min(a.Y, min(b.Y, c.Y)) >> 8, 0);
  T.y1 = min(max(a.Y, max(b.Y, c.Y)) >> 8, w.height - 1);
  return true;
}

// COVERAGE and FRAGMENT of the contract at pixel (px, py); false: none
__device__ __forceinline__ bool rm_fragment(const sph_render_view& w, const RmTri& T, int px, int py, float& l1, float& l2, float& depth) {
  const int Px = 256 * px + 128, Py = 256 * py + 128;
  const long long w0 = rm_edge(T.Xb, T.Yb, T.Xc, T.Yc, Px, Py);
  const long long w1 = rm_edge(T.Xc, T.Yc, T.Xa, T.Ya, Px, Py);
  const long long w2 = rm_edge(T.Xa, T.Ya, T.Xb, T.Yb, Px, Py);
  if (w0 < 0 || w1 < 0 || w2 < 0) return false;
  if (w0 == 0 && !rm_owns(T.Xb, T.Yb, T.Xc, T.Yc)) return false;
  if (w1 == 0 && !rm_owns(T.Xc, T.Yc, T.Xa, T.Ya)) return false;
  if (w2 == 0 && !rm_owns(T.Xa, T.Ya, T.Xb, T.Yb)) return false;
  l1 = (float)w1 / T.A;
  l2 = (float)w2 / T.A;
  const float z = (T.za + l1 * (T.zb - T.za)) + l2 * (T.zc - T.za);
  depth = w.projection ? 1.0f / z : z;
  return depth > w.nearPlane && depth < INFINITY;
}

// The plain load may return a stale cached key; keys only decrease within a pass, so a stale one is never below the true one and
// a fragment that does not beat it cannot beat the true one either (render_emit's argument).
__device__ __forceinline__ void rm_emit(unsigned long long* keys, size_t pixel, float depth, int t) {
  const unsigned long long key = ((unsigned long long)__float_as_uint(depth) << 32) | (unsigned long long)(uint32_t)t;
  if (key < keys[pixel]) __hip_atomic_fetch_min(&keys[pixel], key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ __launch_bounds__(SPH_BLOCK) void k_rm_clear(int pixels, unsigned long long* __restrict__ keys) {
  const int p = blockIdx.x * SPH_BLOCK + threadIdx.x;
  if (p < pixels) keys[p] = RM_EMPTY;
}

__global__ __launch_bounds__(SPH_BLOCK) void k_rm_points(int V, const float* __restrict__ verts, float4* __restrict__ pts) {
  const int i = blockIdx.x * SPH_BLOCK + threadIdx.x;
  if (i < V) pts[i] = make_float4(verts[3 * (size_t)i], verts[3 * (size_t)i + 1], verts[3 * (size_t)i + 2], 0.f);
}

// records: the sample records of the vertices (field >= 0), field 0..5 that word, 6 the speed
__global__ __launch_bounds__(SPH_BLOCK) void k_rm_vertex_mesh(sph_render_view w, int V, const float* __restrict__ verts,
                                                              const float* __restrict__ records, int field, RmVertex* __restrict__ vtx,
                                                              float4* __restrict__ attr) {
  const int i = blockIdx.x * SPH_BLOCK + threadIdx.x;
  if (i >= V) return;
  const float x = verts[3 * (size_t)i], y = verts[3 * (size_t)i + 1], z = verts[3 * (size_t)i + 2];
  float q = 0.f;
  if (field >= 0) {
    const float* r = records + (size_t)SPH_SAMPLE_WORDS * i;
    q = field < 6 ? r[field] : sqrtf((r[2] * r[2] + r[3] * r[3]) + r[4] * r[4]);
  }
  vtx[i] = rm_project(w, x, y, z);
  attr[i] = make_float4(x, y, z, q);
}

// head[3]: error flags (a corner outside 0..N-1, not followed: its vertex is not usable)
__global__ __launch_bounds__(SPH_BLOCK) void k_rm_vertex_membrane(SphDev d, sph_render_view w, int V, int field, RmVertex* __restrict__ vtx,
                                                                  float4* __restrict__ attr, uint32_t* __restrict__ head) {
  const int i = blockIdx.x * SPH_BLOCK + threadIdx.x;
  if (i >= V) return;
  const int o = d.membraneData[i];
  uint32_t j = 0;
  bool ok = o >= 0 && o < d.N;
  if (ok) { j = d.backIndex[o]; ok = j < (uint32_t)d.N; }
  if (!ok) {
    atomicOr(&head[3], 1u);
    vtx[i] = RmVertex{0, 0, 0.f, 0};
    attr[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    return;
  }
  const float4 p = d.sortedPos[j];
  vtx[i] = rm_project(w, p.x, p.y, p.z);
  attr[i] = make_float4(p.x, p.y, p.z, field >= 0 ? sph_particle_quantity(d, field, (int)j, p) : 0.f);
}

// head: [0] triangles drawn, [1] triangles skipped, [2] length of the queue, [3] error flags, [4] pixels the mesh holds, [5] covered pixels
__global__ __launch_bounds__(SPH_BLOCK) void k_rm_raster(sph_render_view w, int T, int V, const RmVertex* __restrict__ vtx,
                                                         const int32_t* __restrict__ tris, unsigned long long* keys,
                                                         uint32_t* __restrict__ head, int32_t* __restrict__ queue) {
  const int t = blockIdx.x * SPH_BLOCK + threadIdx.x;
  const int lane = threadIdx.x & (RM_WAVE - 1);
  RmTri R;
  const bool drawn = t < T && rm_setup(w, vtx, tris, V, t, R);
  const unsigned long long drawnWave = __ballot(drawn), skippedWave = __ballot(t < T && !drawn);
  if (lane == 0 && drawnWave) atomicAdd(&head[0], (uint32_t)__popcll(drawnWave));
  if (lane == 0 && skippedWave) atomicAdd(&head[1], (uint32_t)__popcll(skippedWave));
  const bool inside = drawn && R.x0 <= R.x1 && R.y0 <= R.y1;
  const bool large = inside && (R.x1 - R.x0 >= RM_SMALL || R.y1 - R.y0 >= RM_SMALL);
  const unsigned long long largeWave = __ballot(large);
  if (largeWave) {  // (wave-uniform)
    uint32_t base = 0;
    if (lane == 0) base = atomicAdd(&head[2], (uint32_t)__popcll(largeWave));
    base = __shfl(base, 0);
    const uint32_t at = base + (uint32_t)__popcll(largeWave & ((1ull << lane) - 1ull));
    if (large && at < (uint32_t)T) queue[at] = t;  // (always: every triangle is queued at most once)
  }
  if (!inside || large) return;
  for (int py = R.y0; py <= R.y1; py++)
    for (int px = R.x0; px <= R.x1; px++) {
      float l1, l2, depth;
      if (rm_fragment(w, R, px, py, l1, l2, depth)) rm_emit(keys, (size_t)py * w.width + px, depth, t);
    }
}

__global__ __launch_bounds__(SPH_BLOCK) void k_rm_drain(sph_render_view w, int T, int V, const RmVertex* __restrict__ vtx,
                                                        const int32_t* __restrict__ tris, unsigned long long* keys,
                                                        const uint32_t* __restrict__ head, const int32_t* __restrict__ queue) {
  const int lane = threadIdx.x & (RM_WAVE - 1);
  const uint32_t wave = (uint32_t)(blockIdx.x * SPH_BLOCK + threadIdx.x) / RM_WAVE, waves = gridDim.x * (SPH_BLOCK / RM_WAVE);
  const uint32_t count = min(head[2], (uint32_t)T);
  for (uint32_t q = wave; q < count; q += waves) {
    const int t = queue[q];
    if (t < 0 || t >= T) continue;
    RmTri R;
    if (!rm_setup(w, vtx, tris, V, t, R)) continue;  // (never: it was drawn when it was queued)
    const int bw = R.x1 - R.x0 + 1, n = bw * (R.y1 - R.y0 + 1);  // <= 2^24 pixels
    for (int k = lane; k < n; k += RM_WAVE) {
      const int py = R.y0 + k / bw, px = R.x0 + k % bw;
      float l1, l2, depth;
      if (rm_fragment(w, R, px, py, l1, l2, depth)) rm_emit(keys, (size_t)py * w.width + px, depth, t);
    }
  }
}

__global__ __launch_bounds__(SPH_BLOCK) void k_rm_resolve(RenderMeshArgs a, int pixels, const unsigned long long* __restrict__ keys,
                                                          const RmVertex* __restrict__ vtx, const float4* __restrict__ attr,
                                                          const float* __restrict__ normals, const int32_t* __restrict__ tris,
                                                          uint32_t* __restrict__ head, float* __restrict__ depthOut,
                                                          int32_t* __restrict__ indexOut, uint32_t* __restrict__ idOut,
                                                          uint32_t* __restrict__ rgbaOut, int32_t* __restrict__ triOut) {
  const int p = blockIdx.x * SPH_BLOCK + threadIdx.x;
  const int lane = threadIdx.x & (RM_WAVE - 1);
  const sph_render_view& w = a.view;
  bool held = false, covered = false;
  if (p < pixels && head[3] == 0u) {  // after a bad corner nothing is written: the call fails and the images stay as they were
    const unsigned long long key = keys[p];
    const int t = (int)(uint32_t)key;
    RmTri R;
    float l1 = 0.f, l2 = 0.f, again;
    held = key != RM_EMPTY && t >= 0 && t < a.T && rm_setup(w, vtx, tris, a.V, t, R) &&
           rm_fragment(w, R, p % w.width, p / w.width, l1, l2, again);  // (the last two: always, the key came from them)
    const float depth = __uint_as_float((uint32_t)(key >> 32));
    if (a.compose) {
      const float old = depthOut[p];
      held = held && depth < old;
      covered = held || old < INFINITY;
    } else {
      covered = held;
    }
    if (held) {
      const int ib = R.swapped ? R.c : R.b, ic = R.swapped ? R.b : R.c;  // table order
      const float4 pa = attr[R.a], pb = attr[R.b], pc = attr[R.c];
      float nx, ny, nz;
      if (a.shading == 0) {  // sph_membrane_measure's normal
        const float4 tb = attr[ib], tc = attr[ic];
        const float e1x = tb.x - pa.x, e1y = tb.y - pa.y, e1z = tb.z - pa.z;
        const float e2x = tc.x - pa.x, e2y = tc.y - pa.y, e2z = tc.z - pa.z;
        nx = e1y * e2z - e1z * e2y; ny = e1z * e2x - e1x * e2z; nz = e1x * e2y - e1y * e2x;
        const float len = sqrtf((nx * nx + ny * ny) + nz * nz);
        const bool flat = len == 0.f;
        nx = flat ? 0.f : nx / len; ny = flat ? 0.f : ny / len; nz = flat ? 0.f : nz / len;
      } else {
        const float* na = normals + 3 * (size_t)R.a;
        const float* nb = normals + 3 * (size_t)R.b;
        const float* nc = normals + 3 * (size_t)R.c;
        nx = (na[0] + l1 * (nb[0] - na[0])) + l2 * (nc[0] - na[0]);
        ny = (na[1] + l1 * (nb[1] - na[1])) + l2 * (nc[1] - na[1]);
        nz = (na[2] + l1 * (nb[2] - na[2])) + l2 * (nc[2] - na[2]);
        const float len = sqrtf((nx * nx + ny * ny) + nz * nz);
        const bool none = !(len > 0.f && len < INFINITY);
        nx = none ? 0.f : nx / len; ny = none ? 0.f : ny / len; nz = none ? 0.f : nz / len;
      }
      const float facing = fabsf((nx * w.forward[0] + ny * w.forward[1]) + nz * w.forward[2]);
      const float shade = w.ambient + (1.0f - w.ambient) * facing;
      float c[3] = {a.colour[0], a.colour[1], a.colour[2]};
      if (a.colourMode == 1) {
        const float q = (pa.w + l1 * (pb.w - pa.w)) + l2 * (pc.w - pa.w);
        const float s = fminf(fmaxf((q - a.lo) * a.inv, 0.f), 1.f);
        const float u = s * 4.0f;
        const int i = min((int)u, 3);
        const float f = u - (float)i;
        for (int k = 0; k < 3; k++) c[k] = kMeshRamp[i][k] + f * (kMeshRamp[i + 1][k] - kMeshRamp[i][k]);
      }
      uint32_t rgba = 0xFF000000u;
      for (int k = 0; k < 3; k++) rgba |= (uint32_t)(int)(fminf(fmaxf(c[k] * shade, 0.f), 1.f) * 255.0f + 0.5f) << (8 * k);
      depthOut[p] = depth;
      indexOut[p] = -1;
      idOut[p] = 0xFFFFFFFFu;
      rgbaOut[p] = rgba;
      triOut[p] = t;
    } else {
      triOut[p] = -1;
      if (!a.compose) {
        depthOut[p] = INFINITY;
        indexOut[p] = -1;
        idOut[p] = 0xFFFFFFFFu;
        rgbaOut[p] = (uint32_t)w.background[0] | ((uint32_t)w.background[1] << 8) | ((uint32_t)w.background[2] << 16) |
                     ((uint32_t)w.background[3] << 24);
      }
    }
  }
  const unsigned long long heldWave = __ballot(held), coveredWave = __ballot(covered);
  if (lane == 0 && heldWave) atomicAdd(&head[4], (uint32_t)__popcll(heldWave));
  if (lane == 0 && coveredWave) atomicAdd(&head[5], (uint32_t)__popcll(coveredWave));
}

// ---- launchers ---------------------------------------------------------------------------------------------------------------
static size_t rm_align(size_t b) { return (b + 255) & ~(size_t)255; }

RenderMeshLayout sphk_render_mesh_layout(int64_t V, int64_t T, bool normals, bool samples) {
  RenderMeshLayout L = {};
  size_t at = 0;
  const size_t v = (size_t)std::max<int64_t>(V, 1);
  L.head = at; at += 256;
  L.vtx = at; at += rm_align(sizeof(RmVertex) * v);
  L.attr = at; at += rm_align(sizeof(float4) * v);
  if (normals) { L.normals = at; at += rm_align(sizeof(float) * 3 * v); }
  if (samples) {
    L.points = at; at += rm_align(sizeof(float4) * v);
    L.records = at; at += rm_align(sizeof(float) * SPH_SAMPLE_WORDS * v);
  }
  L.queue = at; at += rm_align(sizeof(int32_t) * (size_t)std::max<int64_t>(T, 1));
  L.bytes = at;
  return L;
}

int sphk_render_mesh_points(sph_solver* s, int V, const float* verts, float* pts4) {
  if (V <= 0) return SPH_OK;
  hipLaunchKernelGGL(k_rm_points, dim3(sph_blocks(V)), dim3(SPH_BLOCK), 0, s->stream, V, verts, (float4*)pts4);
  SPH_HIP(hipGetLastError());
  return SPH_OK;
}

int sphk_render_mesh(sph_solver* s, const RenderMeshArgs& a, const float* verts, const int32_t* tris, void* scratch,
                     const RenderMeshLayout& L, const RenderLayout& I, void* images, int32_t* triangleImage) {
  const int pixels = a.view.width * a.view.height;
  char* base = (char*)scratch;
  char* img = (char*)images;
  uint32_t* head = (uint32_t*)(base + L.head);
  RmVertex* vtx = (RmVertex*)(base + L.vtx);
  float4* attr = (float4*)(base + L.attr);
  unsigned long long* keys = (unsigned long long*)(img + I.keys);
  SPH_HIP(hipMemsetAsync(head, 0, 256, s->stream));
  hipLaunchKernelGGL(k_rm_clear, dim3(sph_blocks(pixels)), dim3(SPH_BLOCK), 0, s->stream, pixels, keys);
  SPH_HIP(hipGetLastError());
  if (a.V > 0) {
    const int field = a.colourMode == 1 ? a.field : -1;
    if (a.source == 0)
      hipLaunchKernelGGL(k_rm_vertex_mesh, dim3(sph_blocks(a.V)), dim3(SPH_BLOCK), 0, s->stream, a.view, a.V, verts,
                         (const float*)(base + L.records), field, vtx, attr);
    else
      hipLaunchKernelGGL(k_rm_vertex_membrane, dim3(sph_blocks(a.V)), dim3(SPH_BLOCK), 0, s->stream, s->d, a.view, a.V, field, vtx, attr, head);
    SPH_HIP(hipGetLastError());
  }
  if (a.T > 0) {
    hipLaunchKernelGGL(k_rm_raster, dim3(sph_blocks(a.T)), dim3(SPH_BLOCK), 0, s->stream, a.view, a.T, a.V, (const RmVertex*)vtx, tris, keys,
                       head, (int32_t*)(base + L.queue));
    SPH_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_rm_drain, dim3(RM_DRAIN_BLOCKS), dim3(SPH_BLOCK), 0, s->stream, a.view, a.T, a.V, (const RmVertex*)vtx, tris, keys,
                       (const uint32_t*)head, (const int32_t*)(base + L.queue));
    SPH_HIP(hipGetLastError());
  }
  hipLaunchKernelGGL(k_rm_resolve, dim3(sph_blocks(pixels)), dim3(SPH_BLOCK), 0, s->stream, a, pixels, (const unsigned long long*)keys,
                     (const RmVertex*)vtx, (const float4*)attr, (const float*)(base + L.normals), tris, head, (float*)(img + I.depth),
                     (int32_t*)(img + I.index), (uint32_t*)(img + I.origId), (uint32_t*)(img + I.rgba), triangleImage);
  SPH_HIP(hipGetLastError());
  return SPH_OK;
}

// Particle editing between steps (include/sphmi.h: sph_remove_* / sph_add_particles / sph_emit_lattice): a stable
// compaction of the original-order state (posOrig, velOrig) and a lattice emitter that appends to it.
//   k_edit_mark_region  one lane per particle: type and half-open box (sph_selector.h) on posOrig; one ballot word per wave, the
//                       mask layout of k_select_flags (mask[4 b + w], bit l = particle 256 b + 64 w + l is MARKED for removal)
//   k_edit_mark_ids     one lane per listed id (or per entry of the live selection, through vals): 64-bit atomicOr into a cleared mask
//   k_edit_counts       one lane per 256-block: the survivors of the block from its four mask words, and the lowest marked id
//                       below the protected (elastic) range, if any
//   (k_select_scan)     the selection's one-workgroup scan turns the survivor counts into block offsets and the total
//   k_edit_scatter      survivor j -> slot off[block] + rank in the block (popcounts of the mask words): both float4 streams move
//                       with 16-byte loads and stores, map[j] = new id or -1
//   k_edit_emit         lattice point k -> slot N + k, with the number of points that fail sph_create's validation
// The compaction writes into the sorted arrays (sortedPos, sortedVel, backIndex), which are dead once the state is invalidated; the
// entry point then swaps the pointers. Integer ballots, popcounts, sums, or and min only: every result is a function of the
// state and the arguments, whatever the order the blocks run in.
#include "sph_common.h"
#include "sph_selector.h"  // the type and box pieces of the selection rule

#define EDIT_WAVE 64
#define EDIT_WAVES (SPH_BLOCK / EDIT_WAVE)

__global__ __launch_bounds__(SPH_BLOCK) void k_edit_mark_region(const float4* __restrict__ pos, int N, SphSelector a,
                                                                unsigned long long* __restrict__ mask) {
  const int j = blockIdx.x * SPH_BLOCK + threadIdx.x;
  bool hit = false;
  if (j < N) {
    const float4 p = pos[j];
    hit = sph_type_selected(p.w, a.typeMask) && sph_box_holds(a.box, p.x, p.y, p.z);  // no key test: posOrig has no keys
  }
  const unsigned long long word = __ballot(hit);
  if ((threadIdx.x & (EDIT_WAVE - 1)) == 0) mask[(size_t)blockIdx.x * EDIT_WAVES + threadIdx.x / EDIT_WAVE] = word;
}

// ids[r] (list == nullptr) or vals[list[r]] (the original id of entry r of a selection); the mask was cleared before
__global__ __launch_bounds__(SPH_BLOCK) void k_edit_mark_ids(const uint32_t* __restrict__ ids, const int32_t* __restrict__ list,
                                                             const uint32_t* __restrict__ vals, int count, int N,
                                                             unsigned long long* __restrict__ mask) {
  const int r = blockIdx.x * SPH_BLOCK + threadIdx.x;
  if (r >= count) return;
  uint32_t o;
  if (list) {
    const int j = list[r];
    if (j < 0 || j >= N) return;
    o = vals[j];
  } else {
    o = ids[r];
  }
  if (o >= (uint32_t)N) return;  // (the entry point has refused such ids already: the guard keeps the store inside the mask)
  atomicOr(&mask[o >> 6], 1ull << (o & 63u));
}

// blockCnt[b] = unmarked particles of block b; *firstBad = min(*firstBad, lowest marked id < protectEnd)
__global__ __launch_bounds__(SPH_BLOCK) void k_edit_counts(const unsigned long long* __restrict__ mask, int nb, int N, int protectEnd,
                                                           uint32_t* __restrict__ blockCnt, uint32_t* __restrict__ firstBad) {
  const int b = blockIdx.x * SPH_BLOCK + threadIdx.x;
  if (b >= nb) return;
  uint32_t kept = 0;
#pragma unroll
  for (int w = 0; w < EDIT_WAVES; w++) {
    const int base = b * SPH_BLOCK + w * EDIT_WAVE;
    const int valid = min(max(N - base, 0), EDIT_WAVE);
    const unsigned long long in = valid == EDIT_WAVE ? ~0ull : ((1ull << valid) - 1ull);
    const unsigned long long marked = mask[(size_t)b * EDIT_WAVES + w] & in;
    kept += (uint32_t)__popcll(~marked & in);
    if (marked && base < protectEnd) {
      const int o = base + __ffsll((long long)marked) - 1;
      if (o < protectEnd) atomicMin(firstBad, (uint32_t)o);
    }
  }
  blockCnt[b] = kept;
}

__global__ __launch_bounds__(SPH_BLOCK) void k_edit_scatter(int N, const unsigned long long* __restrict__ mask,
                                                            const uint32_t* __restrict__ off, uint32_t total,
                                                            const float4* __restrict__ posIn, const float4* __restrict__ velIn,
                                                            float4* __restrict__ posOut, float4* __restrict__ velOut,
                                                            int32_t* __restrict__ map) {
  const int b = blockIdx.x;
  const int j = b * SPH_BLOCK + threadIdx.x;
  if (j >= N) return;
  const int lane = threadIdx.x & (EDIT_WAVE - 1), wave = threadIdx.x / EDIT_WAVE;
  const unsigned long long mine = mask[(size_t)b * EDIT_WAVES + wave];
  if ((mine >> lane) & 1ull) { map[j] = -1; return; }
  // (j < N: every lane below this one, and every wave before this one, holds particles, so ~word counts survivors only)
  uint32_t at = off[b];
#pragma unroll
  for (int w = 0; w < EDIT_WAVES; w++)
    if (w < wave) at += (uint32_t)__popcll(~mask[(size_t)b * EDIT_WAVES + w]);
  at += (uint32_t)__popcll(~mine & ((1ull << lane) - 1ull));
  if (at >= total) return;  // (never: the guard keeps a corrupted mask inside the arrays)
  posOut[at] = posIn[j];
  velOut[at] = velIn[j];
  map[j] = (int32_t)at;
}

// point k = (iz*ny + iy)*nx + ix at origin + (float)i * spacing per axis (one multiply, one add: built with -ffp-contract=off);
// counters[0] = points that are not finite or, if `wide`, outside the box; counters[1] = the lowest such k
__global__ __launch_bounds__(SPH_BLOCK) void k_edit_emit(EditLattice a, int count, float4* __restrict__ pos, float4* __restrict__ vel,
                                                         uint32_t* __restrict__ counters) {
  const int k = blockIdx.x * SPH_BLOCK + threadIdx.x;
  if (k >= count) return;
  const int ix = k % a.nx, iy = (k / a.nx) % a.ny, iz = k / (a.nx * a.ny);
  const float x = a.ox + (float)ix * a.sx, y = a.oy + (float)iy * a.sy, z = a.oz + (float)iz * a.sz;
  const bool finite = isfinite(x) && isfinite(y) && isfinite(z);
  const bool inside = x >= a.xmin && x <= a.xmax && y >= a.ymin && y <= a.ymax && z >= a.zmin && z <= a.zmax;
  if (!finite || (a.wide && !inside)) {
    atomicAdd(&counters[0], 1u);
    atomicMin(&counters[1], (uint32_t)k);
  }
  pos[k] = make_float4(x, y, z, a.typeValue);
  vel[k] = make_float4(a.vx, a.vy, a.vz, 0.f);
}

// ---- launchers ---------------------------------------------------------------------------------------------------------------
// scratch: the selection's layout (mask | block counts | offsets | totals); totals[0..1] the survivors (the scan's), totals[2] the
// lowest marked id below protectEnd or 0xffffffff, totals[4..5] the emitter's counters
size_t sphk_edit_scratch_bytes(int N) { return sphk_select_layout(N).bytes; }

int sphk_edit_mark_region(sph_solver* s, const SphSelector& a, void* scratch) {
  const SelLayout L = sphk_select_layout(s->d.N);
  hipLaunchKernelGGL(k_edit_mark_region, dim3(L.nb), dim3(SPH_BLOCK), 0, s->stream, (const float4*)s->d.posOrig, s->d.N, a,
                     (unsigned long long*)((char*)scratch + L.mask));
  SPH_HIP(hipGetLastError());
  return SPH_OK;
}

int sphk_edit_clear_marks(sph_solver* s, void* scratch) {
  const SelLayout L = sphk_select_layout(s->d.N);
  SPH_HIP(hipMemsetAsync((char*)scratch + L.mask, 0, sizeof(unsigned long long) * EDIT_WAVES * (size_t)L.nb, s->stream));
  return SPH_OK;
}

int sphk_edit_mark_ids(sph_solver* s, const uint32_t* ids, const int32_t* list, int count, void* scratch) {
  if (count <= 0) return SPH_OK;
  const SelLayout L = sphk_select_layout(s->d.N);
  hipLaunchKernelGGL(k_edit_mark_ids, dim3(sph_blocks(count)), dim3(SPH_BLOCK), 0, s->stream, ids, list, (const uint32_t*)s->d.vals,
                     count, s->d.N, (unsigned long long*)((char*)scratch + L.mask));
  SPH_HIP(hipGetLastError());
  return SPH_OK;
}

int sphk_edit_count(sph_solver* s, int protectEnd, void* scratch, uint32_t** totals) {
  const SelLayout L = sphk_select_layout(s->d.N);
  char* base = (char*)scratch;
  uint32_t* t = (uint32_t*)(base + L.totals);
  SPH_HIP(hipMemsetAsync(t + 2, 0xff, sizeof(uint32_t), s->stream));
  hipLaunchKernelGGL(k_edit_counts, dim3(sph_blocks(L.nb)), dim3(SPH_BLOCK), 0, s->stream, (const unsigned long long*)(base + L.mask),
                     L.nb, s->d.N, protectEnd, (uint32_t*)(base + L.blockCnt), t + 2);
  SPH_HIP(hipGetLastError());
  const int rc = sphk_select_scan(s, scratch, s->d.N);
  *totals = t;
  return rc;
}

int sphk_edit_scatter(sph_solver* s, void* scratch, uint32_t total, float4* posOut, float4* velOut, int32_t* map) {
  const SelLayout L = sphk_select_layout(s->d.N);
  char* base = (char*)scratch;
  hipLaunchKernelGGL(k_edit_scatter, dim3(L.nb), dim3(SPH_BLOCK), 0, s->stream, s->d.N, (const unsigned long long*)(base + L.mask),
                     (const uint32_t*)(base + L.off), total, (const float4*)s->d.posOrig, (const float4*)s->d.velOrig, posOut, velOut,
                     map);
  SPH_HIP(hipGetLastError());
  return SPH_OK;
}

int sphk_edit_emit(sph_solver* s, const EditLattice& a, int count, void* scratch, uint32_t** counters) {
  const SelLayout L = sphk_select_layout(s->d.N);
  uint32_t* c = (uint32_t*)((char*)scratch + L.totals) + 4;
  SPH_HIP(hipMemsetAsync(c, 0, sizeof(uint32_t), s->stream));
  SPH_HIP(hipMemsetAsync(c + 1, 0xff, sizeof(uint32_t), s->stream));
  hipLaunchKernelGGL(k_edit_emit, dim3(sph_blocks(count)), dim3(SPH_BLOCK), 0, s->stream, a, count, s->d.posOrig + s->d.N,
                     s->d.velOrig + s->d.N, c);
  SPH_HIP(hipGetLastError());
  *counters = c;
  return SPH_OK;
}

// PCISPH kernels K6, K7, K9-K13 (sphFluid.cl:472-708, 824-1212, 1684-1808) for gfx950.
//
// One lane per sorted particle (the reference's `id = particleIndexBack[get_global_id]` is a pure thread permutation and
// is dropped — SURVEY App. B #11). Every kernel streams its own 32 neighbour slots from the tiled maps — the ids as 16-bit
// offsets, eight coalesced 8-byte loads per lane (NbrTile; sph_common.h, SPH_N16_*), the distances where it needs them as eight
// 16-byte loads — and gathers neighbour state as single 12/16-byte transactions.
// Arithmetic keeps the reference's operand types and evaluation order: no FMA contraction, IEEE division/sqrt,
// f32 denormals kept, f64 where sphFluid.cl uses double.
#include "sph_common.h"
#include "sph_fastmath.h"

#define TYPE_OF(p4) ((int)(p4).w)
typedef float f32x3 __attribute__((ext_vector_type(3)));
// Predicted positions are packed (x, y, z), 12 bytes per particle: 10.7 records per 128-byte line instead of 8 — the gathers of
// predictDensity touch a quarter fewer lines (tools/micro/gather_lanes.hip: -25 % of the gather cost) and every stream of them is
// 12 bytes instead of 16. (The .w the reference keeps there is dead data.)
typedef f32x3 f32x3a __attribute__((aligned(4)));
__device__ __forceinline__ float4 load_pred(const SphDev& d, int id) {
  const f32x3a v = *reinterpret_cast<const f32x3a*>(d.predPos + 3 * (size_t)id);
  return make_float4(v.x, v.y, v.z, 0.f);
}
__device__ __forceinline__ void store_pred(const SphDev& d, int id, const float4 p) {
  const f32x3a v = {p.x, p.y, p.z};
  *reinterpret_cast<f32x3a*>(d.predPos + 3 * (size_t)id) = v;
}
// The always-valid gather index of the branch-free kernels: an empty slot (-1) reads record 0 and is masked out of the sum.
// (The 16-byte neighbour gathers — 64 different cache lines per wave instruction — cost about a fifth of the step: DESIGN.md 4.1.)
#define NBR_INDEX(j) (max((j), 0))

// neighbour gathers kept in flight per lane by the branch-free kernels: as many as the kernel's register budget leaves room for
#define FC_BATCH 8   // forces: two 16-B gathers per neighbour
#define PF_BATCH 8   // pressure force: 16 B + 4 B per neighbour
#define PD_BATCH 16  // predicted density: 16 B per neighbour

// index into SphDev::gatherRec: groups of four particles, [4 x part 0][4 x part 1] (one 128-byte line; see k_pack_gather_records)
__device__ __forceinline__ size_t rec_index(int j, int part) { return ((size_t)(j >> 2) << 3) + (size_t)(part << 2) + (size_t)(j & 3); }

// the 8 x (int4 ids, float4 dists) of particle `id`, and its ids again as 8 x (4 x 16-bit offsets) (sph_common.h, SPH_N16_*)
struct NbrTile {
  const int4* ids;
  const float4* dist;
  const uint2* v16;
  int self, zOff;  // the particle and (base of its flagged offsets) - (the particle)
  __device__ __forceinline__ NbrTile(const SphDev& d, int id) {
    const size_t base = ((size_t)(id >> 6) * 8) * 64 + (size_t)(id & 63);
    ids = reinterpret_cast<const int4*>(d.nbrId) + base;
    dist = reinterpret_cast<const float4*>(d.nbrDist) + base;
    v16 = reinterpret_cast<const uint2*>(d.nbr16) + base;
    self = id;
    zOff = d.nbrBase[id] - id;
  }
  __device__ __forceinline__ int4 id4(int g) const { return ids[(size_t)g * 64]; }
  // The rows are streamed once per kernel: non-temporal loads keep them from displacing the records the gathers live on
  // (A/B at 16.5 M, profiles/r03/gather_rows_nontemporal_ab.txt: predictDensity 0.498 -> 0.490 ms, forces 1.549 -> 1.529, pressure force unchanged)
  __device__ __forceinline__ float4 dist4(int g) const {
    typedef float nt4 __attribute__((ext_vector_type(4)));
    const nt4 q = __builtin_nontemporal_load(reinterpret_cast<const nt4*>(&dist[(size_t)g * 64]));
    return make_float4(q.x, q.y, q.z, q.w);
  }
  __device__ __forceinline__ uint2 vec16(int g) const {  // slots 4g .. 4g+3
    typedef unsigned int nt2 __attribute__((ext_vector_type(2)));
    const nt2 q = __builtin_nontemporal_load(reinterpret_cast<const nt2*>(&v16[(size_t)g * 64]));
    return make_uint2(q.x, q.y);
  }
  // the row has no 16-bit copy (an offset did not fit, or findNeighbors served the particle by its exact walk): use id_wide()
  __device__ __forceinline__ static bool wide(const uint2& group0) { return (group0.x & 0xffffu) == SPH_N16_WIDE; }
  __device__ __forceinline__ int id_wide(int slot) const {
    return reinterpret_cast<const int32_t*>(ids)[((size_t)(slot >> 2) * 64) * 4 + (size_t)(slot & 3)];
  }
  // entry k (0..3) of a group -> sorted index of the neighbour, -1 for an empty slot
  __device__ __forceinline__ int decode(const uint2& v, int k) const {
    const uint32_t w = (k >> 1) == 0 ? v.x : v.y;
    const uint32_t e = (k & 1) ? (w >> 16) : (w & 0xffffu);
    const int j = self - SPH_N16_BIAS + (int)(e & 0x7fffu) + ((e & 0x8000u) ? zOff : 0);
    return e == SPH_N16_EMPTY ? -1 : j;
  }
};

// XCD-aware block order (xcd_block, sph_common.h) in its range-aware form, for launches restricted to a cell range (slab mode): the remap must run over the blocks that HAVE work.
// Remapping over the whole grid would hand the first eighth of the logical blocks — for a short range, all of the work — to
// one XCD (a 5-layer launch then took as long as the full one: 120 us instead of 17).
// b: the launch's block (blockIdx.x in a launch of one block per 256 particles; a grid-stride launch passes each of its blocks)
__device__ __forceinline__ bool xcd_range_id(const SphDev& d, int b, int& id) {
  const int begin = (int)d.cellStart[d.rangeLo], end = (int)d.cellStart[d.rangeHi];
  const int active = (end - begin + SPH_BLOCK - 1) / SPH_BLOCK;
  if (b >= active) return false;
  const int per = active >> 3, even = per << 3;
  if (b < even) {
    const int x = b & 7;
    int k = b >> 3;  // k-th workgroup dealt to XCD x
    // (a CU-local sub-order inside the XCD — every CU a contiguous sub-range, hoping its resident workgroups share L1 lines — was
    // measured: 0-7 % slower on all three gather kernels)
    b = x * per + k;
  }
  id = begin + b * SPH_BLOCK + threadIdx.x;
  return id < end;
}
__device__ __forceinline__ bool xcd_range_id(const SphDev& d, int& id) { return xcd_range_id(d, (int)blockIdx.x, id); }
// blocks of 256 particles in the launch's range: what a grid-stride launch loops over
__device__ __forceinline__ int range_blocks(const SphDev& d) {
  return ((int)d.cellStart[d.rangeHi] - (int)d.cellStart[d.rangeLo] + SPH_BLOCK - 1) / SPH_BLOCK;
}

// ---- per-wave flags of the predict-correct loop (SphDev::pBlk ...). Where they are in use the launch's range starts
// at a multiple of SPH_BLOCK, so the lanes of a wave are the particles of one id >> 6.
// The lane that writes the wave's byte: the lowest one still active (boundary lanes of K12 and lanes past the range have left).
__device__ __forceinline__ bool wave_leader() { return (int)__lane_id() == __ffsll((unsigned long long)__ballot(1)) - 1; }
__device__ __forceinline__ bool wave_flag_store(uint8_t* flags, int id, bool set) {  // returns the byte
  const bool any = __any(set);
  if (wave_leader()) flags[id >> 6] = any ? 1 : 0;
  return any;
}
// The launch-level gate (SphDev::skipGate): the writers count their flagged waves over every 64th block and the consumer decides once,
// by a uniform load. It consults only where the sample found nothing flagged — liquid at rest or in free fall. Where some waves are
// flagged, the writers' marking of the neighbourhood bytes has to be paid for by the waves that skip, and of the states measured
// (profiles/r28) only the config #2 cube gained from always consulting; the worm, the dam break and the box at 0.85 r0 came out
// 1.4-4 % slower. SphDev::gatePolicy switches the counting off (sph_set_wave_skip mode 1).
__device__ __forceinline__ bool gate_open(const SphDev& d) { return d.skipGate[d.gateIn] == 0u; }
__device__ __forceinline__ void gate_count(const SphDev& d, int id, bool waveFlagged) {
  // (only "none" against "some" is read, so a wave that already sees a count leaves it: thousands of atomic adds on one word
  // cost a pressure-active launch more than everything else the flags add to it)
  if (d.gatePolicy && waveFlagged && ((id >> 8) & 63) == 0 && wave_leader() && *(volatile uint32_t*)&d.skipGate[d.gateOut] == 0u)
    atomicAdd(&d.skipGate[d.gateOut], 1u);
}
// The neighbourhood bytes (SphDev::nbhd). A writer wave whose flag is set stores a 1 for every wave that could hold a particle with
// a neighbour in it. "Could" is judged by cells: findNeighbors, on its fast path and in its exact walk, looks for the neighbours of a
// particle with key ki only in the cells wrap_cell(ki + dx + dy gx + dz gx gy, G), d in {-1, 0, 1}^3, so a particle with key kj can
// be a neighbour only of particles in the 27 cells ki = kj - delta, wrapped back into [0, G) (the inverse of that rule; one cell
// per offset because G exceeds every offset, which enqueue_step checks). Keys, not cells: 16-bit aliasing is the search's too.
// The wave walks the distinct keys of its active lanes (1-3 as a rule) and deals the 27 offsets of each to those lanes; a cell's
// sorted range [lo, hi) marks the waves lo >> 6 .. (hi - 1) >> 6 with plain stores of the same value. delta = 0 marks the wave
// itself and its cell-mates. A key outside [0, G) (a blown-up state) cannot name its readers and closes the stage's gate instead,
// as does a cell the search would refuse to walk. With gatePolicy the wave leaves the marking out once the gate reads closed: the
// word only grows within a step, so every consumer of that stage will read it closed too and consult nothing.
__device__ __forceinline__ void mark_readers(const SphDev& d, const int id) {
  if (d.gatePolicy && *(volatile uint32_t*)&d.skipGate[d.gateOut] != 0u) return;
  const uint32_t mine = d.keys[id];
  const unsigned long long act = __ballot(1);
  const int lane = (int)__lane_id();
  const int rank = __popcll(act & ((1ull << lane) - 1ull)), n = __popcll(act);
  const int layer = d.gx * d.gy;
  bool todo = true;
  for (;;) {
    const unsigned long long m = __ballot(todo);
    if (m == 0ull) break;
    const uint32_t kj = (uint32_t)__builtin_amdgcn_readlane((int)mine, __ffsll(m) - 1);
    todo = todo && mine != kj;
    bool refuse = kj >= (uint32_t)d.G;
    if (!refuse) {
      for (int o = rank; o < 27; o += n) {
        const int off = (o % 3 - 1) + ((o / 3) % 3 - 1) * d.gx + (o / 9 - 1) * layer;
        int ki = (int)kj - off;
        if (ki < 0) ki += d.G;
        if (ki >= d.G) ki -= d.G;
        if (ki < 0 || ki >= d.G) continue;
        const uint32_t lo = d.cellTable[ki], hi = min(d.cellTable[ki + 1], (uint32_t)d.N);
        if (hi <= lo) continue;  // an empty cell marks nothing
        if (hi - lo > (1u << 20)) { refuse = true; continue; }  // (fn_exact_walk does not walk such a cell)
        for (uint32_t w = lo >> 6; w <= (hi - 1u) >> 6; w++) d.nbOut[w] = 1;
      }
    }
    if (__any(refuse) && rank == 0) atomicAdd(&d.skipGate[d.gateOut], 1u);
  }
}
// A wave's byte of a per-wave array, as part of its aligned word: the address is wave-uniform, so the load is a scalar one and
// leaves with the first loads of the kernel. w: the wave's index in an SGPR (readfirstlane of id >> 6).
__device__ __forceinline__ uint32_t wave_byte(const uint8_t* a, int w) {
  return (reinterpret_cast<const uint32_t*>(a)[w >> 2] >> ((w & 3) * 8)) & 0xffu;
}

// ------------------------------------------------------------------ K6 pcisph_computeDensity (sphFluid.cl:472-518)
// The HBM-roofline-graded pass: reads 32 x 4 B of distances, writes 4 B. The empty-slot test uses the distance
// sentinel (-1), which is set iff the id is -1 (both are written together), so the id half of the map is not read.
// A/B on MI355X (bench.py roofline, 16.5 M particles): XCD-remapped blocks + plain loads 0.66 of 8 TB/s, plain block
// order 0.67-0.69, plain order + non-temporal loads 0.75 (6.0 TB/s = 96 % of this part's 6.29 TB/s copy rate). The pass has
// no reuse, so neither an XCD-local L2 nor keeping the stream in cache helps.
// Particles per thread, all of their 8 x 16-B loads in flight together. One: the pass runs at 91 % of the part's copy rate, eight
// loads per lane cover HBM. The loops over it stay: written out for one particle the same arithmetic compiles to a different load
// and wait order (profiles/r10/README.md), which would have to be timed on the graded kernel.
constexpr int DENSITY_ITEMS = 1;
__global__ __launch_bounds__(SPH_BLOCK) void k_density(SphDev d, int nblocks) {
  typedef float nt4 __attribute__((ext_vector_type(4)));
  const int begin = (int)d.cellStart[d.rangeLo], end = (int)d.cellStart[d.rangeHi];
  const int first = begin + blockIdx.x * (SPH_BLOCK * DENSITY_ITEMS) + threadIdx.x;
  float4 r[DENSITY_ITEMS][8];
#pragma unroll
  for (int it = 0; it < DENSITY_ITEMS; it++) {
    const int id = first + it * SPH_BLOCK;
    if (id < end) {
      const NbrTile t(d, id);
#pragma unroll
      for (int g = 0; g < 8; g++) {  // all loads in flight before the first use
        const nt4 q = __builtin_nontemporal_load(reinterpret_cast<const nt4*>(&t.dist[(size_t)g * 64]));
        r[it][g] = make_float4(q.x, q.y, q.z, q.w);
      }
    }
  }
#pragma unroll
  for (int it = 0; it < DENSITY_ITEMS; it++) {
    const int id = first + it * SPH_BLOCK;
    if (id >= end) continue;
    double density = 0.0;
#pragma unroll
    for (int g = 0; g < 8; g++) {
      const float rr[4] = {r[it][g].x, r[it][g].y, r[it][g].z, r[it][g].w};
#pragma unroll
      for (int k = 0; k < 4; k++) {
        if (rr[k] != -1.f) {
          const float r2 = rr[k] * rr[k];
          const float a = d.hs2 - r2;
          density += (double)(a * a * a);  // no r < hScaled test here
        }
      }
    }
    if (density < (double)d.hs6) density = (double)d.hs6;
    density *= d.massWpoly6;
    d.rho[id] = (float)density;
  }
}

int sphk_density(sph_solver* s, int ghostDepth) {
  const int nb = sph_blocks(s->d.N, SPH_BLOCK * DENSITY_ITEMS);
  hipLaunchKernelGGL(k_density, dim3(nb), dim3(SPH_BLOCK), 0, s->stream, sph_ranged(s, ghostDepth), nb);
  SPH_HIP(hipGetLastError());
  return SPH_OK;
}

// ------------------------------------------------------------------ K9 pcisph_predictPositions (sphFluid.cl:889-979)
__device__ __forceinline__ float4 predict_position(const SphDev& d, const float4 x, const float4 v, const float4 ap) {
  if (TYPE_OF(x) == SPH_BOUNDARY_PARTICLE) return x;
  // v* = v + dt*a_p (pressure acceleration only, :924); x* = x + (dt/simScale)*v*
  float4 o;
  o.x = x.x + d.posTimeStep * (v.x + d.dt * ap.x);
  o.y = x.y + d.posTimeStep * (v.y + d.dt * ap.y);
  o.z = x.z + d.posTimeStep * (v.z + d.dt * ap.z);
  o.w = x.w;  // dead in the reference (holds cell id + ...); we keep the type
  return o;
}

__global__ __launch_bounds__(SPH_BLOCK) void k_predict_positions(SphDev d) {
  const int id = blockIdx.x * SPH_BLOCK + threadIdx.x;
  if (id >= d.N) return;
  store_pred(d, id, predict_position(d, d.sortedPos[id], d.sortedVel[id], d.accP[id]));
}

int sphk_predict_positions(sph_solver* s) {
  hipLaunchKernelGGL(k_predict_positions, dim3(sph_blocks(s->d.N)), dim3(SPH_BLOCK), 0, s->stream, s->d);
  SPH_HIP(hipGetLastError());
  return SPH_OK;
}

// ------------------------------------------------------------------ K7 pcisph_computeForcesAndInitPressure (sphFluid.cl:589-708)
__device__ __forceinline__ float corrected_pressure(const SphDev& d, float p, float rhoPred);  // (K11, below)

// FUSE_DENSITY (fused step outside slab mode; needs FUSE_PREDICT): the kernel is also iteration 0 of K10 + K11. The pressure
// acceleration is still zero there, so a neighbour's predicted position follows from the (x_j, v_j) this kernel gathers anyway:
// it is formed again in registers by the same predict_position() call that wrote predPos, and the density sum runs over the
// same 32 slots in the same order with k_predict_density's expressions. That launch then neither streams the id rows a second
// time nor gathers 32 predicted positions per particle. Boundary particles have a predicted density too (the pressure force
// gathers their (rho*, p)), so they run the loop here and leave without the force half's stores.
// The kernel's body for sorted particle id. Two entry points share it: k_forces, one block per 256 particles, and k_forces_strided,
// a small grid looping over those blocks (the pipelined step's launch over all particles, which is empty on most steps).
// MARK: a wave that holds a pressure marks its readers' neighbourhood bytes (mark_readers); without it such a wave closes the gate
// of its stage instead, which is exact as well. The grid-stride entry point goes without: its launch over all particles is empty
// unless the halo check failed, and with the marking inlined it would need scratch memory.
template <bool FUSE_PREDICT, bool FUSE_DENSITY, bool MARK>
__device__ __forceinline__ void forces_particle(const SphDev& d, const int id) {
  static_assert(FUSE_PREDICT || !FUSE_DENSITY, "the density half reads what the predict half forms");
  const float4 xi = d.sortedPos[id];
  const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
  const bool boundary = TYPE_OF(xi) == SPH_BOUNDARY_PARTICLE;
  if (!FUSE_DENSITY && boundary) {
    d.acc[id] = zero;
    if (FUSE_PREDICT) store_pred(d, id, xi);
    else { d.accP[id] = zero; d.rp[id].y = 0.f; }  // (fused step: nobody reads either before the next kernel overwrites it)
    return;
  }
  const float4 vi = d.sortedVel[id];
  const NbrTile t(d, id);
  float4 xpi = xi;  // FUSE_DENSITY: the particle's own iteration-0 predicted position (a boundary particle's is its position)
  if (FUSE_DENSITY) xpi = predict_position(d, xi, vi, zero);
  double density = 0.0;
  float sx = 0.f, sy = 0.f, sz = 0.f, tx = 0.f, ty = 0.f, tz = 0.f;
  uint32_t bnd = 0u, ela = 0u;  // which neighbour slots hold boundary / elastic particles: saves integrate and the
                                // membrane kernel 32 type gathers per particle
  bool wideRow = false;
  bool closePair = false;  // FUSE_DENSITY: a valid neighbour at a stored distance < closeRf, the pairs K12 treats apart (cBlk)
  // Branch-free (see k_predict_density): per batch of FC_BATCH neighbours the map loads, then all gathers in flight together.
  // The map is read batch by batch (not all 32 entries up front) and the velocity gather takes 12 bytes: at 193 VGPRs the
  // kernel ran two waves per SIMD, too few to cover its gathers.
#pragma unroll 1  // (a real loop: unrolled, hipcc hoists the loads of all four batches to the top and needs ~190 VGPRs)
  for (int b = 0; b < 32 / FC_BATCH; b++) {
    int jj[FC_BATCH];
    float rr[FC_BATCH];
#pragma unroll
    for (int q = 0; q < FC_BATCH / 4; q++) {  // (recomputing r from the gathered positions, as K12 does, is not faster here: 1.505 vs 1.521 ms)
      const float4 rq = t.dist4(b * (FC_BATCH / 4) + q);
      rr[4 * q] = rq.x; rr[4 * q + 1] = rq.y; rr[4 * q + 2] = rq.z; rr[4 * q + 3] = rq.w;
    }
#pragma unroll
    for (int q = 0; q < FC_BATCH / 4; q++) {
      const uint2 v = t.vec16(b * (FC_BATCH / 4) + q);
      if (b == 0 && q == 0) wideRow = NbrTile::wide(v);
#pragma unroll
      for (int k = 0; k < 4; k++) jj[4 * q + k] = t.decode(v, k);
    }
    if (wideRow) {  // rare
#pragma unroll
      for (int k = 0; k < FC_BATCH; k++) jj[k] = t.id_wide(b * FC_BATCH + k);
    }
    float4 xj[FC_BATCH], vr[FC_BATCH];
#pragma unroll
    for (int k = 0; k < FC_BATCH; k++) {
      const int jc = NBR_INDEX(jj[k]);
      xj[k] = d.gatherRec[rec_index(jc, 0)];
      vr[k] = d.gatherRec[rec_index(jc, 1)];  // (v.xyz, rho); for a boundary neighbour v is its wall normal (sphFluid.cl:653)
    }
#pragma unroll
    for (int k = 0; k < FC_BATCH; k++) {
      const int slot = b * FC_BATCH + k;
      const bool valid = jj[k] != -1;
      if (valid && TYPE_OF(xj[k]) == SPH_BOUNDARY_PARTICLE) bnd |= 1u << slot;
      if (valid && TYPE_OF(xj[k]) == SPH_ELASTIC_PARTICLE) ela |= 1u << slot;
      const bool use = valid && rr[k] < d.hs;
      if (FUSE_DENSITY) closePair |= valid && rr[k] < d.closeRf;  // (an empty slot holds -1)
      const float rj = vr[k].w;
      const float w = d.hs - rr[k];
      sx = use ? sx + (vr[k].x - vi.x) * w / rj : sx;
      sy = use ? sy + (vr[k].y - vi.y) * w / rj : sy;
      sz = use ? sz + (vr[k].z - vi.z) * w / rj : sz;
      tx = use ? tx + d.surfTens * (xi.x - xj[k].x) : tx;
      ty = use ? ty + d.surfTens * (xi.y - xj[k].y) : ty;
      tz = use ? tz + d.surfTens * (xi.z - xj[k].z) : tz;
      if (FUSE_DENSITY) {  // k_predict_density's term, on the neighbour's predicted position formed here
        const float4 xpj = predict_position(d, xj[k], vr[k], zero);
        const float rx = xpi.x - xpj.x, ry = xpi.y - xpj.y, rz = xpi.z - xpj.z;
        const float r2 = (rx * rx + ry * ry + rz * rz) * d.simScale * d.simScale;
        const float a = d.hs2 - r2;
        const float term = (valid && r2 < d.hs2) ? a * a * a : 0.f;
        density += (double)term;
      }
    }
  }
  bool mark = false;  // FUSE_DENSITY: the wave holds a pressure and marks its readers' neighbourhood bytes, behind the last store
  if (FUSE_DENSITY) {
    if (density < (double)d.hs6) density = (double)d.hs6;
    density *= d.massWpoly6;
    const float rhoP = (float)density;
    const float p = corrected_pressure(d, 0.f, rhoP);
    d.rp[id] = make_float2(rhoP, p);
    store_pred(d, id, xpi);
    if (d.pBlk) {  // (every lane of the wave is still here; K12 never walks a boundary particle's row)
      mark = wave_flag_store(d.pBlk, id, p != 0.f);
      const bool anyC = wave_flag_store(d.cBlk, id, closePair && !boundary);
      gate_count(d, id, mark || anyC);
    }
  }
  if (FUSE_DENSITY && boundary) {
    d.acc[id] = zero;
  } else {
    d.bndMask[id] = bnd;
    if (d.hasElastic) d.elasticMask[id] = ela;
    const float scale = d.massMu * (float)(d.del2W / (double)d.rho[id]);
    float4 a;
    a.x = sx * scale + d.gravx + tx;
    a.y = sy * scale + d.gravy + ty;
    a.z = sz * scale + d.gravz + tz;
    a.w = 0.f;  // acceleration.w is never read (integrate zeroes it, sphFluid.cl:1721)
    d.acc[id] = a;
  }
  if (mark) {  // (every lane, the boundary ones too: K12 gathers a boundary neighbour's pressure)
    if (MARK) mark_readers(d, id);
    else if (wave_leader() && *(volatile uint32_t*)&d.skipGate[d.gateOut] == 0u) atomicAdd(&d.skipGate[d.gateOut], 1u);
  }
  if (FUSE_DENSITY) return;  // (predPos and rp are written above)
  // The staged API needs pressure = 0 and a zero pressure acceleration in memory; in the fused step the first predictDensity
  // starts from p = 0 by itself and the pressure acceleration is not read before the last pressure-force kernel writes it.
  if (FUSE_PREDICT) store_pred(d, id, predict_position(d, xi, vi, zero));
  else { d.accP[id] = zero; d.rp[id].y = 0.f; }
}

template <bool FUSE_PREDICT, bool FUSE_DENSITY>
__global__ __launch_bounds__(SPH_BLOCK, 4) void k_forces(SphDev d, int nblocks) {  // <= 128 VGPRs: four waves per SIMD
  int id;
  if (!xcd_range_id(d, id)) return;
  forces_particle<FUSE_PREDICT, FUSE_DENSITY, true>(d, id);
}
template <bool FUSE_PREDICT, bool FUSE_DENSITY>
__global__ __launch_bounds__(SPH_BLOCK, 4) void k_forces_strided(SphDev d) {
  const int active = range_blocks(d);
  for (int b = blockIdx.x; b < active; b += gridDim.x) {  // (the grid is a multiple of 8 blocks: b keeps its XCD)
    int id;
    if (xcd_range_id(d, b, id)) forces_particle<FUSE_PREDICT, FUSE_DENSITY, false>(d, id);
  }
}

// Gather records of the forces kernel: what it needs of a neighbour — (x, y, z, type) and (v.xyz, rho) — in ONE 128-byte line,
// groups of four particles: [4 x (x,y,z,type)][4 x (vx,vy,vz,rho)]. A/B on MI355X at 16.5 M particles (tools/time_stage.py):
// three gathers from three arrays (position, velocity, density) 2.06 ms; position and velocity in one line, density apart
// 1.54 ms; everything in one line 1.22 ms + this pack pass (68 B per particle, 0.2 ms). A wave's gather instruction costs by
// the number of different lines it touches. Kept out of k_density so that the roofline-graded pass moves exactly its 132 B.

// The launch packs the sorted particles [lo, hi); lo is a multiple of four, so record groups stay whole.
__global__ __launch_bounds__(SPH_BLOCK) void k_pack_gather_records(SphDev d, int lo, int hi) {
  const int id = lo + blockIdx.x * SPH_BLOCK + threadIdx.x;
  if (id >= hi) return;
  const float4 v = d.sortedVel[id];
  d.gatherRec[rec_index(id, 0)] = d.sortedPos[id];
  d.gatherRec[rec_index(id, 1)] = make_float4(v.x, v.y, v.z, d.rho[id]);
}

// Slab mode: forces are only needed on the owned layers, but every local particle needs what K7 does besides the
// acceleration — the iteration-0 predicted position (pressure = 0 is implied by the first fused predictDensity).
__global__ __launch_bounds__(SPH_BLOCK) void k_ghost_init(SphDev d) {
  const int id = blockIdx.x * SPH_BLOCK + threadIdx.x;
  if (id >= d.N) return;
  const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
  store_pred(d, id, predict_position(d, d.sortedPos[id], d.sortedVel[id], zero));
}

int sphk_ghost_init(sph_solver* s) {
  hipLaunchKernelGGL(k_ghost_init, dim3(sph_blocks(s->d.N)), dim3(SPH_BLOCK), 0, s->stream, s->d);
  SPH_HIP(hipGetLastError());
  return SPH_OK;
}

int sphk_pack_gather_records(sph_solver* s, int idxLo, int idxHi, hipStream_t stream) {
  if (idxLo < 0 || idxLo % 4 != 0) { sph_set_error("sphk_pack_gather_records: idxLo %d is not a multiple of 4", idxLo); return SPH_ERR_INVALID; }
  idxHi = min(idxHi, s->d.N);
  if (idxHi <= idxLo) return SPH_OK;
  hipLaunchKernelGGL(k_pack_gather_records, dim3(sph_blocks(idxHi - idxLo)), dim3(SPH_BLOCK), 0, stream, s->d, idxLo, idxHi);
  SPH_HIP(hipGetLastError());
  return SPH_OK;
}

// The density pass of chunk c = [idxLo, idxHi) of the partition that s->chunkEdges holds on the device. k_density takes its range
// as two entries of a table it calls the cell table; here that table is the chunk partition and the "cells" are c and c + 1, so
// the roofline-graded kernel runs unchanged (it reads nothing else of the cell table) and its grid covers the chunk alone.
// INVARIANT this rests on: k_density and the NbrTile constructor read of d.cellStart exactly cellStart[rangeLo] and
// cellStart[rangeHi]. A change that makes either read the cell table for anything else must give this launcher a kernel of its
// own (tests/test_step_overlap.py compares the chunked density with the oracle's and would fail). The trade: the source text
// that bench.py's density_sources_sha() hashes stays as it was, so a PMC traffic figure taken on k_density describes the
// kernel of both paths, at the price of a one-block launch per change of (N, chunk count) and 17 device words.
int sphk_density_chunk(sph_solver* s, int c, int idxLo, int idxHi, hipStream_t stream) {
  if (c < 0 || c >= SPH_STEP_CHUNKS_MAX || idxLo < 0 || idxHi > s->d.N) { sph_set_error("sphk_density_chunk: chunk %d [%d, %d) of %d particles", c, idxLo, idxHi, s->d.N); return SPH_ERR_INVALID; }
  if (idxHi <= idxLo) return SPH_OK;
  SphDev d = s->d;
  d.cellStart = s->chunkEdges; d.rangeLo = c; d.rangeHi = c + 1;
  const int nb = sph_blocks(idxHi - idxLo, SPH_BLOCK * DENSITY_ITEMS);
  hipLaunchKernelGGL(k_density, dim3(nb), dim3(SPH_BLOCK), 0, stream, d, nb);
  SPH_HIP(hipGetLastError());
  return SPH_OK;
}

// The launch's view of the per-wave flags: the fused kernels of a step that enqueue_step set waveSkip for see them, every other
// launch gets null pointers and runs the code without them. (The null pointer is also the A/B switch when measuring.)
// stage: the launch's place in the loop (1 the forces kernel, 2 i + 1 / 2 i + 2 predicted density / pressure force of iteration i):
// it counts into the gate word of its stage and marks the neighbourhood bytes of its stage, and reads those of the stage before.
// The built-in policy (sph_set_wave_skip mode 0): 1 the launch-level gate, 0 always mark and consult (mode 1).
#ifndef SPH_WAVE_SKIP_GATED
#define SPH_WAVE_SKIP_GATED 1
#endif
static SphDev wave_skip_view(const sph_solver* s, SphDev d, bool fused, int stage) {
  if (!(fused && s->waveSkip)) d.pBlk = d.cBlk = d.xBlk = d.k12Skip = d.k10Skip = nullptr;
  d.gateIn = (stage - 1) & (SPH_GATE_SLOTS - 1); d.gateOut = stage & (SPH_GATE_SLOTS - 1);
  d.nbIn = s->d.nbhd + (size_t)d.gateIn * s->d.nbStride; d.nbOut = s->d.nbhd + (size_t)d.gateOut * s->d.nbStride;
  d.cellTable = s->d.cellStart;  // (the real one: the launches of the pipelined step hand the kernels a table of their own as cellStart)
  d.gatePolicy = s->waveSkipMode == 1 ? 0 : SPH_WAVE_SKIP_GATED;
  return d;
}

// fuseDensity: the launch is also the first predictDensity + correctPressure of the fused step (every particle, so not in slab mode)
int sphk_forces(sph_solver* s, bool fusePredict, int ghostDepth, bool fuseDensity, bool packRecords) {
  if (fuseDensity && (!fusePredict || s->hasSlab)) { sph_set_error("sphk_forces: the density half needs the fused step outside slab mode"); return SPH_ERR_INVALID; }
  const int nb = sph_blocks(s->d.N);
  const SphDev d = wave_skip_view(s, sph_ranged(s, ghostDepth), fuseDensity, 1);
  if (packRecords) { const int rc = sphk_pack_gather_records(s, 0, s->d.N, s->stream); if (rc != SPH_OK) return rc; }
  if (fuseDensity) hipLaunchKernelGGL((k_forces<true, true>), dim3(nb), dim3(SPH_BLOCK), 0, s->stream, d, nb);
  else if (fusePredict) hipLaunchKernelGGL((k_forces<true, false>), dim3(nb), dim3(SPH_BLOCK), 0, s->stream, d, nb);
  else hipLaunchKernelGGL((k_forces<false, false>), dim3(nb), dim3(SPH_BLOCK), 0, s->stream, d, nb);
  SPH_HIP(hipGetLastError());
  return SPH_OK;
}

// ------------------------------------------------------------------ K10 pcisph_predictDensity (+ K11 correctPressure)
// (sphFluid.cl:982-1059, 1062-1098)
__device__ __forceinline__ float corrected_pressure(const SphDev& d, float p, float rhoPred) {
  const float rho_err = rhoPred - d.rho0;
  float p_corr = rho_err * d.delta;
  if (p_corr < 0.f) p_corr = 0.f;
  return p + p_corr;
}

// What k_predict_density leaves for the pressure-force kernel behind it besides rp: the wave's pBlk byte, its count into the gate
// (pBlk or cBlk: what K12 will be stopped by) and, if the wave holds a pressure, the neighbourhood bytes of its readers.
__device__ __forceinline__ void publish_pressure(const SphDev& d, const int id, const float p) {
  const bool anyP = wave_flag_store(d.pBlk, id, p != 0.f);
  gate_count(d, id, anyP || d.cBlk[id >> 6] != 0);
  if (anyP) mark_readers(d, id);
}

// FIRST (fused step, iteration 0): the pressure being corrected is the 0 that K7 sets, without reading it.
template <bool FUSE_CORRECT, bool FIRST>
__device__ __forceinline__ void predict_density_particle(const SphDev& d, const int id) {  // (two entry points, as for forces_particle)
  // Iterations >= 1 of the fused step: if no wave that could hold a neighbour of this wave's particles, itself included, changed a
  // bit of a predicted position in the pressure-force kernel before this launch (its neighbourhood byte, marked by the waves whose
  // xBlk byte that kernel set), the sum below would run over the inputs of the launch before, in the same order: rho* is the value
  // that launch left in rp. One wave-uniform branch, decided from the gate word and one byte, both scalar loads
  // that leave with the kernel's first loads; only a wave that runs its loop requests its id rows.
  if (FUSE_CORRECT && !FIRST && d.xBlk) {
    const int w = __builtin_amdgcn_readfirstlane(id) >> 6;
    const bool skip = gate_open(d) && wave_byte(d.nbIn, w) == 0u;
    const float2 old = d.rp[id];  // (requested in front of the decision: a skipping wave is a chain of round trips and little else)
    if (wave_leader()) d.k10Skip[id >> 6] = skip ? 1 : 0;
    if (skip) {
      const float p = corrected_pressure(d, old.y, old.x);
      d.rp[id] = make_float2(old.x, p);
      publish_pressure(d, id, p);
      return;
    }
  }
  const float4 xi = load_pred(d, id);
  const NbrTile t(d, id);
  // Branch-free: all 8 id loads first, then the gathers in batches of 8 with an always-valid index (empty slots read
  // record 0 and are masked out of the sum), so a wave keeps 8 gathers in flight instead of one per `if`.
  uint2 v16[8];  // the ids as 16-bit offsets: 64 bytes per particle instead of 128 (this kernel streams little else)
#pragma unroll
  for (int g = 0; g < 8; g++) v16[g] = t.vec16(g);
  const bool wideRow = NbrTile::wide(v16[0]);
  double density = 0.0;
#pragma unroll
  for (int b = 0; b < 32 / PD_BATCH; b++) {
    int jj[PD_BATCH];
#pragma unroll
    for (int k = 0; k < PD_BATCH; k++) {
      const int slot = b * PD_BATCH + k;
      jj[k] = t.decode(v16[slot >> 2], slot & 3);
    }
    if (wideRow) {  // rare
#pragma unroll
      for (int k = 0; k < PD_BATCH; k++) jj[k] = t.id_wide(b * PD_BATCH + k);
    }
    float4 xj[PD_BATCH];
#pragma unroll
    for (int k = 0; k < PD_BATCH; k++) xj[k] = load_pred(d, NBR_INDEX(jj[k]));
#pragma unroll
    for (int k = 0; k < PD_BATCH; k++) {
      const float rx = xi.x - xj[k].x, ry = xi.y - xj[k].y, rz = xi.z - xj[k].z;
      const float r2 = (rx * rx + ry * ry + rz * rz) * d.simScale * d.simScale;
      const float a = d.hs2 - r2;
      // a skipped term is added as +0.0: the sum is >= +0 (it starts there and only grows), so x + 0.0 == x bit for bit
      const float term = (jj[k] != -1 && r2 < d.hs2) ? a * a * a : 0.f;
      density += (double)term;
    }
  }
  if (density < (double)d.hs6) density = (double)d.hs6;
  density *= d.massWpoly6;
  const float rhoP = (float)density;
  if (FUSE_CORRECT) {  // (rho*, p) is one 8-byte record: what the pressure-force kernel gathers per neighbour besides the position
    const float pOld = FIRST ? 0.f : d.rp[id].y;
    const float p = corrected_pressure(d, pOld, rhoP);
    d.rp[id] = make_float2(rhoP, p);
    if (d.pBlk) publish_pressure(d, id, p);
  } else {
    d.rp[id].x = rhoP;
  }
}

template <bool FUSE_CORRECT, bool FIRST>
__global__ __launch_bounds__(SPH_BLOCK) void k_predict_density(SphDev d, int nblocks) {
  int id;
  if (!xcd_range_id(d, id)) return;
  predict_density_particle<FUSE_CORRECT, FIRST>(d, id);
}
template <bool FUSE_CORRECT, bool FIRST>
__global__ __launch_bounds__(SPH_BLOCK) void k_predict_density_strided(SphDev d) {
  const int active = range_blocks(d);
  for (int b = blockIdx.x; b < active; b += gridDim.x) {
    int id;
    if (xcd_range_id(d, b, id)) predict_density_particle<FUSE_CORRECT, FIRST>(d, id);
  }
}

int sphk_predict_density(sph_solver* s, bool fuseCorrect, int ghostDepth, bool first, int iteration) {
  const int nb = sph_blocks(s->d.N);
  const SphDev d = wave_skip_view(s, sph_ranged(s, ghostDepth), fuseCorrect, 2 * iteration + 1);
  if (fuseCorrect && first) hipLaunchKernelGGL((k_predict_density<true, true>), dim3(nb), dim3(SPH_BLOCK), 0, s->stream, d, nb);
  else if (fuseCorrect) hipLaunchKernelGGL((k_predict_density<true, false>), dim3(nb), dim3(SPH_BLOCK), 0, s->stream, d, nb);
  else hipLaunchKernelGGL((k_predict_density<false, false>), dim3(nb), dim3(SPH_BLOCK), 0, s->stream, d, nb);
  SPH_HIP(hipGetLastError());
  return SPH_OK;
}

__global__ __launch_bounds__(SPH_BLOCK) void k_correct_pressure(SphDev d) {
  const int id = blockIdx.x * SPH_BLOCK + threadIdx.x;
  if (id >= d.N) return;
  const float2 v = d.rp[id];
  d.rp[id].y = corrected_pressure(d, v.y, v.x);
}

int sphk_correct_pressure(sph_solver* s) {
  hipLaunchKernelGGL(k_correct_pressure, dim3(sph_blocks(s->d.N)), dim3(SPH_BLOCK), 0, s->stream, s->d);
  SPH_HIP(hipGetLastError());
  return SPH_OK;
}

// ------------------------------------------------------------------ K13 pcisph_integrate (sphFluid.cl:1684-1808)
// + computeInteractionWithBoundaryParticles (sphFluid.cl:824-887), tangVel = true.
// Boundary neighbours are read from the sorted arrays: boundary particles never move, so sortedPos/sortedVel hold the
// same bits as position[]/velocity[] of the reference and the particleIndex indirection is unnecessary.
__device__ __forceinline__ void integrate_particle(const SphDev& d, int id, const float4 x, const float4 v, const float4 a0,
                                                   const float4 a1) {
  const float ax = a0.x + a1.x, ay = a0.y + a1.y, az = a0.z + a1.z;  // acceleration_.w = 0
  float nvx = v.x + d.dt * ax, nvy = v.y + d.dt * ay, nvz = v.z + d.dt * az, nvw = v.w + d.dt * 0.f;
  float nx = x.x + d.posTimeStep * nvx, ny = x.y + d.posTimeStep * nvy, nz = x.z + d.posTimeStep * nvz;
  if (nx < d.xmin) nx = d.xmin;
  if (ny < d.ymin) ny = d.ymin;
  if (nz < d.zmin) nz = d.zmin;
  if (nx > d.xmax - 0.000001f) nx = d.xmax - 0.000001f;
  if (ny > d.ymax - 0.000001f) ny = d.ymax - 0.000001f;
  if (nz > d.zmax - 0.000001f) nz = d.zmax - 0.000001f;
  nvx = (v.x + nvx) * 0.5f; nvy = (v.y + nvy) * 0.5f; nvz = (v.z + nvz) * 0.5f; nvw = (v.w + nvw) * 0.5f;

  const NbrTile t(d, id);
  float ncx = 0.f, ncy = 0.f, ncz = 0.f, ncw = 0.f, wsum = 0.f, wsum2 = 0.f;
  const uint32_t bnd = d.bndMask[id];  // boundary neighbours, found by the forces kernel of this step
  if (__any(bnd != 0u)) {              // waves in the bulk of the liquid skip the loop (and its 32 id loads) entirely
    const bool wideRow = NbrTile::wide(t.vec16(0));
#pragma unroll 2
    for (int g = 0; g < 8; g++) {
      const uint2 v = t.vec16(g);
#pragma unroll
      for (int k = 0; k < 4; k++) {
        if (!((bnd >> (g * 4 + k)) & 1u)) continue;
        const int jb = wideRow ? t.id_wide(g * 4 + k) : t.decode(v, k);
        const float4 pb = d.sortedPos[jb];
        float dist = (nx - pb.x) * (nx - pb.x);
        dist += (ny - pb.y) * (ny - pb.y);
        dist += (nz - pb.z) * (nz - pb.z);
        dist = sqrtf(dist);
        const float w = fmaxf(0.f, (d.r0 - dist) / d.r0);  // Ihmsen 2010 (10)
        const float4 nb = d.sortedVel[jb];                  // wall normal, stored in the velocity slot
        ncx += nb.x * w; ncy += nb.y * w; ncz += nb.z * w; ncw += nb.w * w;
        wsum += w;
        wsum2 += w * (d.r0 - dist);
      }
    }
  }
  float len = ((ncx * ncx + ncy * ncy) + ncz * ncz) + ncw * ncw;  // dot(float4,float4) incl. the .w lane
  if (len != 0.f) {
    len = sqrtf(len);
    nx += ((ncx / len) * wsum2) / wsum;
    ny += ((ncy / len) * wsum2) / wsum;
    nz += ((ncz / len) * wsum2) / wsum;
    const float vn = ncx * nvx + ncy * nvy + ncz * nvz;  // un-normalised n_c_i (sphFluid.cl:878)
    if (vn < 0.f) {
      nvx -= ncx * vn; nvy -= ncy * vn; nvz -= ncz * vn;
      nvx *= 0.99f; nvy *= 0.99f; nvz *= 0.99f; nvw *= 0.99f;
    }
  }
  if (!d.hasElastic) {
    // no elastic matter: the three membrane kernels reduce to `position += 0` for non-boundary particles
    // (sphFluid.cl:1673 with an all-zero scratch half); fold that add in so the bits match (-0 + 0 = +0).
    nx += 0.f; ny += 0.f; nz += 0.f;
  }
  const uint32_t src = d.vals[id];
  d.velOrig[src] = make_float4(nvx, nvy, nvz, nvw);
  d.posOrig[src] = make_float4(nx, ny, nz, x.w);  // (x,y,z,type) in one store
}

__global__ __launch_bounds__(SPH_BLOCK) void k_integrate(SphDev d, int nblocks) {
  const int id = xcd_block(nblocks) * SPH_BLOCK + threadIdx.x;
  if (id >= d.N) return;
  const float4 x = d.sortedPos[id];
  if (TYPE_OF(x) == SPH_BOUNDARY_PARTICLE) return;
  integrate_particle(d, id, x, d.sortedVel[id], d.acc[id], d.accP[id]);
}

int sphk_integrate(sph_solver* s) {
  const int nb = sph_blocks(s->d.N);
  { const int g = sph_guard_position_write(s); if (g != SPH_OK) return g; }
  hipLaunchKernelGGL(k_integrate, dim3(nb), dim3(SPH_BLOCK), 0, s->stream, s->d, nb);
  SPH_HIP(hipGetLastError());
  return SPH_OK;
}

// ------------------------------------------------------------------ K12 pcisph_computePressureForceAcceleration
// (sphFluid.cl:1101-1212). FUSE: 0 = alone, 1 = + next iteration's predictPositions, 2 = + integrate (last iteration).
// One batch of PF_BATCH neighbours of the pressure-force sum. FAST: square root and the divisions by r through sph_fastmath.h;
// returns false (wave-uniform) if any lane had an operand outside the ranges those sequences are valid in.
template <bool FAST>
__device__ __forceinline__ bool pf_batch(const SphDev& d, const float4 xi, const float pi_, const float hq, const float4 (&xj)[PF_BATCH],
                                         const float2 (&rpj)[PF_BATCH], const int (&jj)[PF_BATCH], float& rx, float& ry, float& rz,
                                         const bool ownOk) {
  bool ok = ownOk;
  // FAST: value, the three numerators and the three quotients carry the factor 2^40 of sph_fastmath.h (the 0.5 of the numerator
  // becomes 2^39; the sums take the quotients through fma(q, 2^-40, sum) — the same single rounding as sum + q / 2^40)
  const float half = FAST ? SPH_FAST_HALF_SCALED : 0.5f;
#pragma unroll
  for (int k = 0; k < PF_BATCH; k++) {
    const float ex_ = xi.x - xj[k].x, ey_ = xi.y - xj[k].y, ez_ = xi.z - xj[k].z;
    const float d2_ = ex_ * ex_ + ey_ * ey_ + ez_ * ez_;
    float sq_;
    if (FAST) ok = sph_sqrt_fast(d2_, d.fastD2Min, d.fastD2Max, &sq_) && ok;  // (the bounds also keep r inside the division's range)
    else sq_ = sqrtf(d2_);
    const float r = sq_ * d.simScale;  // == the stored neighborMap distance (sphFluid.cl:131-136,172), which is therefore not read
    // value = -(hs-r)^2*0.5*(p_i+p_j)/rho*_j, or for very close pairs -(hs/4-r)^2*0.5*(rho0*delta)/rho*_j (:1166-1168):
    // the numerator is selected first, so only one IEEE division is spent
    float num = -(d.hs - r) * (d.hs - r) * half * (pi_ + rpj[k].y);
    if (__any(r < d.closeRf)) num = (r < d.closeRf) ? -(hq - r) * (hq - r) * half * d.rho0delta : num;  // (pairs closer than h/4: rare, so wave-uniformly skipped)
    const float value = FAST ? sph_div1_by(num, rpj[k].x) : num / rpj[k].x;  // (8 instructions against the 13-15 of the compiler's division)
    const float vx = (xi.x - xj[k].x) * d.simScale, vy = (xi.y - xj[k].y) * d.simScale, vz = (xi.z - xj[k].z) * d.simScale;
    const bool use = jj[k] != -1 && r < d.hs;
    const float ax_ = value * vx, ay_ = value * vy, az_ = value * vz;
    float q_[3];
    // (the division's guard only matters for terms that are used: beyond the support radius, where value is tiny, nothing is added.
    // Guarding every lane and dropping unused terms by scaling them with 0 — one select instead of three — was measured: no change)
    if (FAST) ok = (sph_div3_by<false>(ax_, ay_, az_, value, d.fastValueMin, r, q_) || !use) && ok;
    else { q_[0] = ax_ / r; q_[1] = ay_ / r; q_[2] = az_ / r; }
    if (FAST) {
      rx = use ? __builtin_fmaf(q_[0], SPH_FAST_UNSCALE, rx) : rx;
      ry = use ? __builtin_fmaf(q_[1], SPH_FAST_UNSCALE, ry) : ry;
      rz = use ? __builtin_fmaf(q_[2], SPH_FAST_UNSCALE, rz) : rz;
    } else {
      rx = use ? rx + q_[0] : rx;
      ry = use ? ry + q_[1] : ry;
      rz = use ? rz + q_[2] : rz;
    }
  }
  return !FAST || !__any(!ok);
}

template <int FUSE>
__device__ __forceinline__ void pressure_force_particle(const SphDev& d, const int id) {  // (two entry points, as for forces_particle)
  const float4 xi = d.sortedPos[id];
  const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
  // The wave has nothing to add if the pressure sum p_i + p_j is +0 for every pair it would walk and no pair is closer than hs / 4:
  // every term is then a +-0 added to a sum that starts at +0 and cannot become -0. p >= +0 always, so that is: no
  // wave that could hold a neighbour of this wave's particles, itself included, holds a pressure (its neighbourhood byte, marked by
  // the waves whose pBlk byte is set; a NaN counts as a pressure) and no close pair in the wave's own rows (cBlk). Such a wave takes
  // rx = ry = rz = 0 through the unchanged tail below. One wave-uniform branch, decided from the gate word and two bytes: scalar
  // loads that leave with the kernel's first loads, in front of the id rows, which only a wave that runs its loop requests.
  bool consult = false, skip = false;
  if (FUSE != 0 && d.pBlk) {
    const int w = __builtin_amdgcn_readfirstlane(id) >> 6;
    consult = gate_open(d);
    skip = consult && (wave_byte(d.nbIn, w) | wave_byte(d.cBlk, w)) == 0u;
  }
  const bool boundary = TYPE_OF(xi) == SPH_BOUNDARY_PARTICLE;
  if (FUSE != 0 && d.pBlk && !__any(!boundary) && wave_leader()) {  // a wave of boundary particles: nobody is left below to write its bytes
    d.k12Skip[id >> 6] = 1;
    if (FUSE == 1) d.xBlk[id >> 6] = 0;
  }
  if (boundary) {
    if (FUSE == 1) store_pred(d, id, xi);  // (the bits it has held since the forces kernel: "unchanged" for xBlk)
    else d.accP[id] = zero;  // (FUSE == 1, a middle iteration of the fused step: the next pressure-force kernel overwrites it unread)
    return;
  }
  const float2 rpi = d.rp[id];  // (rho*, p) of this particle
  float4 vi = zero;
  if (FUSE != 0) vi = d.sortedVel[id];  // (the tail's: requested in front of the loop, a skipping wave is a chain of round trips and little else)
  const float pi_ = rpi.y;
  float rx = 0.f, ry = 0.f, rz = 0.f;
  if (FUSE != 0 && d.pBlk && wave_leader()) d.k12Skip[id >> 6] = skip ? 1 : 0;
  if (!skip) {
    // precondition of the short division sequence (sph_fastmath.h): own coordinates not within 2^-4 of zero
    const bool ownOk = sph_exp_in(xi.x, SPH_FAST_COORD_EXP_LO, 100) && sph_exp_in(xi.y, SPH_FAST_COORD_EXP_LO, 100) &&
                       sph_exp_in(xi.z, SPH_FAST_COORD_EXP_LO, 100);
    const NbrTile t(d, id);
    const float hq = d.hs * 0.25f;
    // Branch-free, like k_predict_density: map loads first, gathers in batches of PF_BATCH with an always-valid index,
    // masked accumulation (a skipped term leaves the sum untouched, exactly as the reference's `if`).
    // The distances are NOT read: r_ij is recomputed from the two position records this kernel has anyway, with the expression
    // findNeighbors stored it with (sphFluid.cl:131-136,172; IEEE sqrt) — bit-identical, and 128 of the 272 bytes the kernel
    // streamed per particle are gone (1.24 -> 1.17 ms per launch at 16.5 M particles; re-measured in round 3 with the short
    // arithmetic in place: reading the rows instead of taking the square root is 1.26 vs 1.00 ms per launch).
    uint2 v16[8];
#pragma unroll
    for (int g = 0; g < 8; g++) v16[g] = t.vec16(g);
    const bool wideRow = NbrTile::wide(v16[0]);
#pragma unroll
    for (int b = 0; b < 32 / PF_BATCH; b++) {
      int jj[PF_BATCH];
#pragma unroll
      for (int k = 0; k < PF_BATCH; k++) {
        const int slot = b * PF_BATCH + k;
        jj[k] = t.decode(v16[slot >> 2], slot & 3);
      }
      if (wideRow) {  // rare
#pragma unroll
        for (int k = 0; k < PF_BATCH; k++) jj[k] = t.id_wide(b * PF_BATCH + k);
      }
      float4 xj[PF_BATCH];
      float2 rpj[PF_BATCH];
#pragma unroll
      for (int k = 0; k < PF_BATCH; k++) {
        const int jc = NBR_INDEX(jj[k]);
        xj[k] = d.sortedPos[jc];
        rpj[k] = d.rp[jc];
      }
      // The kernel is bound by its arithmetic: the IEEE square root and the three IEEE divisions by r take the short sequences of
      // sph_fastmath.h, bit-identical inside their operand ranges; a batch in which any lane of the wave leaves those ranges is
      // simply computed again with the compiler's sqrtf and `/` (same results for the lanes that were inside).
      const float bx = rx, by = ry, bz = rz;
      if (!pf_batch<true>(d, xi, pi_, hq, xj, rpj, jj, rx, ry, rz, ownOk)) {
        if ((threadIdx.x & 63) == 0) atomicAdd(&d.dbg[8], 1u);  // (wave, batch) pairs recomputed with sqrtf and `/`: rare (tests assert it)
        rx = bx; ry = by; rz = bz;
        pf_batch<false>(d, xi, pi_, hq, xj, rpj, jj, rx, ry, rz, true);
      }
    }
  }
  const float scale = (float)(d.massGradW / (double)rpi.x);
  const float4 ap = make_float4(rx * scale, ry * scale, rz * scale, 0.f);
  if (FUSE != 1) d.accP[id] = ap;
  if (FUSE == 1) {
    const float4 xp = predict_position(d, xi, vi, ap);
    bool moved = false;
    if (d.xBlk) {
      bool changed = true;  // (behind a closed gate nothing was skipped: "changed" without looking is the safe byte)
      if (consult) {  // compared on bits: a zero velocity's sign decides whether v + dt * (-0) equals the v + dt * (+0) before it
        const float4 was = load_pred(d, id);
        changed = __float_as_uint(was.x) != __float_as_uint(xp.x) || __float_as_uint(was.y) != __float_as_uint(xp.y) ||
                  __float_as_uint(was.z) != __float_as_uint(xp.z);
      }
      moved = wave_flag_store(d.xBlk, id, changed);
      gate_count(d, id, moved);
    }
    store_pred(d, id, xp);
    if (moved) mark_readers(d, id);  // (the keys of the lanes still here: a boundary particle's predicted position never changes)
  }
  if (FUSE == 2) integrate_particle(d, id, xi, vi, d.acc[id], ap);
}

template <int FUSE>
__global__ __launch_bounds__(SPH_BLOCK) void k_pressure_force(SphDev d, int nblocks) {
  int id;
  if (!xcd_range_id(d, id)) return;
  pressure_force_particle<FUSE>(d, id);
}
template <int FUSE>
__global__ __launch_bounds__(SPH_BLOCK) void k_pressure_force_strided(SphDev d) {
  const int active = range_blocks(d);
  for (int b = blockIdx.x; b < active; b += gridDim.x) {
    int id;
    if (xcd_range_id(d, b, id)) pressure_force_particle<FUSE>(d, id);
  }
}

static int launch_pressure_force(sph_solver* s, int fuse, const SphDev& ranged, int nb, hipStream_t stream, int stage) {
  const SphDev d = wave_skip_view(s, ranged, fuse != 0, stage);
  if (fuse == 2) { const int g = sph_guard_position_write(s, stream); if (g != SPH_OK) return g; }  // (+ integrate: writes posOrig)
  if (fuse == 0) hipLaunchKernelGGL((k_pressure_force<0>), dim3(nb), dim3(SPH_BLOCK), 0, stream, d, nb);
  else if (fuse == 1) hipLaunchKernelGGL((k_pressure_force<1>), dim3(nb), dim3(SPH_BLOCK), 0, stream, d, nb);
  else hipLaunchKernelGGL((k_pressure_force<2>), dim3(nb), dim3(SPH_BLOCK), 0, stream, d, nb);
  SPH_HIP(hipGetLastError());
  return SPH_OK;
}

int sphk_pressure_force(sph_solver* s, int fuse, int ghostDepth, int iteration) {
  return launch_pressure_force(s, fuse, sph_ranged(s, ghostDepth), sph_blocks(s->d.N), s->stream, 2 * iteration + 2);
}

int sphk_pressure_force_layers(sph_solver* s, int fuse, long long loLayer, long long hiLayer) {
  return launch_pressure_force(s, fuse, sph_ranged_layers(s, loLayer, hiLayer), sph_blocks(s->d.N), s->stream, 0);  // (slab mode: no flags)
}

// One stage of the pipelined step over one chunk, or over all particles behind the join. As in sphk_density_chunk the
// kernel is handed a small table in place of the cell table: the pipeline table with "cells" c and c + 1 and a grid that covers the
// chunk, or the serial table with "cells" 0 and 1 and the full grid. k_halo_check fills both every step, so that exactly one of the
// two launches of a stage finds particles and the blocks of the other leave in xcd_range_id (b >= active = 0).
// INVARIANT this rests on: k_forces, k_predict_density and k_pressure_force — with predict_position, integrate_particle, the NbrTile
// constructor and xcd_range_id — read of d.cellStart exactly cellStart[rangeLo] and cellStart[rangeHi] (integrate_particle finds a
// boundary neighbour through the neighbour row, not through the cell table). tests/test_step_pipeline.py compares every depth with
// the oracle and the serial step.
int sphk_pipeline_stage(sph_solver* s, int stage, int c, int idxLo, int idxHi, hipStream_t stream) {
  const int M = s->cfg.maxIteration;
  if (s->hasSlab || !s->pipeTable || stage < 1 || stage > 2 * M || c >= SPH_STEP_CHUNKS_MAX || idxLo < 0 || idxHi > s->d.N) {
    sph_set_error("sphk_pipeline_stage: stage %d of %d, chunk %d [%d, %d) of %d particles", stage, 2 * M, c, idxLo, idxHi, s->d.N);
    return SPH_ERR_INVALID;
  }
  if (idxHi <= idxLo) return SPH_OK;
  SphDev d = wave_skip_view(s, s->d, true, stage);
  d.cellStart = c >= 0 ? s->pipeTable : s->pipeTable + SPH_STEP_CHUNKS_MAX + 1;
  d.rangeLo = c >= 0 ? c : 0; d.rangeHi = d.rangeLo + 1;
  const int nb = sph_blocks(idxHi - idxLo);
  const bool last = stage == 2 * M;
  if (c < 0) {
    // Over all particles the grid-stride entry points: the launch is empty on every step whose halo check passed, and a grid of
    // one block per 256 particles would cost 17 us there at 16.5 M particles whereas this one costs what a launch costs
    // (profiles/r24/README.md). 8 blocks per CU of a 256-CU part.
    const int grid = min(nb, SPH_SERIAL_GRID);
    if (last) { const int g = sph_guard_position_write(s, stream); if (g != SPH_OK) return g; }
    if (stage == 1) hipLaunchKernelGGL((k_forces_strided<true, true>), dim3(grid), dim3(SPH_BLOCK), 0, stream, d);
    else if (stage & 1) hipLaunchKernelGGL((k_predict_density_strided<true, false>), dim3(grid), dim3(SPH_BLOCK), 0, stream, d);
    else if (last) hipLaunchKernelGGL((k_pressure_force_strided<2>), dim3(grid), dim3(SPH_BLOCK), 0, stream, d);
    else hipLaunchKernelGGL((k_pressure_force_strided<1>), dim3(grid), dim3(SPH_BLOCK), 0, stream, d);
  } else if (stage == 1) {
    hipLaunchKernelGGL((k_forces<true, true>), dim3(nb), dim3(SPH_BLOCK), 0, stream, d, nb);
  } else if (stage & 1) {  // predicted density (+ pressure correction) of iteration stage / 2 >= 1
    hipLaunchKernelGGL((k_predict_density<true, false>), dim3(nb), dim3(SPH_BLOCK), 0, stream, d, nb);
  } else {  // pressure force of iteration stage / 2 - 1: + the next iteration's predicted positions, or + integrate behind the last
    return launch_pressure_force(s, last ? 2 : 1, d, nb, stream, stage);
  }
  SPH_HIP(hipGetLastError());
  return SPH_OK;
}

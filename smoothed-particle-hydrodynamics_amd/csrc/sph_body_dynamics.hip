// Free bodies (include/sphmi.h: sph_body_set_dynamics / sph_bodies_advance): after a completed step, the load of that
// step on every dynamic body, one step of rigid-body dynamics and the new placement of the members, without a host wait.
//   k_bdyn_map        member k of dynamic body b: bodyOf[backIndex[id]] = b, one byte per SORTED particle (0xff: member of no
//                     dynamic body). Plain byte stores: two dynamic bodies never share a member (sph_body_set_dynamics).
//   k_bdyn_leaf       the fused load: one block per chunk of 1024 sorted particles in the element layout of the diagnostics leaf
//                     (thread t holds elements t, t + 256, t + 512, t + 768). The per-particle record is wl_record
//                     (sph_wall_record.h), the function sph_wall_measure evaluates, with the wall set "members of body b"; its
//                     terms are wl_terms, the function sph_wall_diagnostics sums. The block reduces the 19 words the integrator
//                     needs per body in the fixed tree of sph_tree.h, from registers through LDS; no per-particle term reaches
//                     memory. A wave evaluates records only for the bodies some lane of it has in its row (a 16-bit presence
//                     mask per element, found by walking the set bits of bndMask once); a block without a lane that touches
//                     body b writes +0.0 partials for it and does no tree. Slot 16 of the partials is no body: its word 0 counts
//                     the particles in contact with any wall (word 1 of the diagnostics record).
//   (sph_tree.hip)    the upper levels of the tree, the rows of the dynamic bodies and word 0 of the count row only
//   k_bdyn_integrate  one thread per slot: the contract's doubles; the new state goes to a staging record, the pose as floats
//   k_bdyn_pose<C>    validate (C = false) and commit (C = true) of all dynamic bodies in one launch each (blockIdx.y = slot),
//                     through body_pose_member (sph_body_pose.h), the function k_body_pose runs; the commit is predicated on the
//                     offender counter the validation left on the device
//   k_bdyn_finish     one thread per slot: the staged state becomes the live one unless the pose was refused; the record
//   k_bdyn_overlap_*  sph_body_set_dynamics: members of one body that are members of another dynamic body
// Integer atomics only where the result cannot depend on the order (or, add, min, max). No floating-point atomics.
#include "sph_body_pose.h"
#include "sph_common.h"
#include "sph_tree.h"
#include "sph_wall_record.h"

#include <algorithm>

#define BD_WORDS 19   // per body: n with share > 0 | C xyz | visc, tens, pres xyz | TC xyz | TH xyz
#define BD_GROUP 10   // words reduced together through LDS: 19 -> 10 + 9
#define BD_SLOTS (SPH_MAX_BODIES + 1)  // the bodies, then the contact count of all walls
#define BD_ALL SPH_MAX_BODIES

// (the rows of the tree are the BD_SLOTS slots, BD_WORDS words each; the last row holds word 0 only)

__global__ __launch_bounds__(SPH_BLOCK) void k_bdyn_map(SphDev d, BodyDynSet set, uint8_t* __restrict__ bodyOf) {
  const int b = blockIdx.y, r = blockIdx.x * SPH_BLOCK + threadIdx.x;
  if (!((set.dynMask >> b) & 1u) || r >= set.count[b]) return;
  const uint32_t o = set.ids[b][r];
  if (o >= (uint32_t)d.N) return;
  const uint32_t j = d.backIndex[o];
  if (j >= (uint32_t)d.N) return;
  bodyOf[j] = (uint8_t)b;
}

// the dynamic bodies among the boundary neighbours of sorted particle `id` (bnd: its boundary-slot mask, not 0), one bit per slot
__device__ __forceinline__ uint32_t bd_presence(const SphDev& d, const uint8_t* __restrict__ bodyOf, int id, uint32_t bnd) {
  const FmRow t(d, id);
  const bool wideRow = (t.vec16(0).x & 0xffffu) == SPH_N16_WIDE;
  const int last = d.N - 1;
  uint32_t pres = 0u;
#pragma unroll 1
  for (int g = 0; g < 8; g++) {
    if (!((bnd >> (g * 4)) & 0xfu)) continue;
    const uint2 v16 = t.vec16(g);
#pragma unroll
    for (int k = 0; k < 4; k++) {
      if (!((bnd >> (g * 4 + k)) & 1u)) continue;
      int j = wideRow ? t.id_wide(g * 4 + k) : t.decode(v16, k);
      j = min(max(j, 0), last);  // as wl_record: an index outside 0..N-1 is never followed
      const uint32_t b = bodyOf[j];
      if (b < SPH_MAX_BODIES) pres |= 1u << b;
    }
  }
  return pres;
}

__global__ __launch_bounds__(SPH_BLOCK) void k_bdyn_leaf(SphDev d, const uint8_t* __restrict__ bodyOf, uint32_t dynMask,
                                                         double* __restrict__ part, int chunks) {
  __shared__ double sh[BD_GROUP][SPH_BLOCK];
  __shared__ uint32_t shPres;
  const int t = threadIdx.x, chunk = blockIdx.x;
  // per element: the boundary-slot mask of a selected non-boundary particle (0 otherwise) and the bodies in its row
  uint32_t bnd[4], pres[4];
  uint32_t mine = 0u;
#pragma unroll
  for (int e = 0; e < 4; e++) {
    const int j = chunk * DIAG_CHUNK + e * SPH_BLOCK + t;
    bnd[e] = 0u; pres[e] = 0u;
    if (j < d.N) {
      uint32_t b = d.bndMask[j];
      if (b) {
        const float4 p = d.sortedPos[j];
        const int type = (int)p.w;
        // the diagnostics' selection with typeMask = types 1..3 (sph_type_key_selected), and not a boundary particle
        if (!(type >= 1 && type <= 3 && type != SPH_BOUNDARY_PARTICLE && d.keys[j] < (uint32_t)d.G)) b = 0u;
      }
      bnd[e] = b;
      if (b) {
        pres[e] = bd_presence(d, bodyOf, j, b);
        mine |= pres[e] | (1u << BD_ALL);
      }
    }
  }
  if (t == 0) shPres = 0u;
  __syncthreads();
  if (mine) atomicOr(&shPres, mine);
  __syncthreads();
  const uint32_t blockPres = shPres;
  const uint32_t wanted = dynMask | (1u << BD_ALL);
#pragma unroll 1
  for (int b = 0; b < BD_SLOTS; b++) {
    if (!((wanted >> b) & 1u)) continue;
    const int nW = b == BD_ALL ? 1 : BD_WORDS;
    if (!((blockPres >> b) & 1u)) {  // every term of this chunk is zero: +0.0, which is what the tree would produce from +0.0 terms
      if (t < nW) part[tree_at(BD_WORDS, b, t, chunks, chunk)] = 0.0;
      continue;
    }
    const WallBodySet ws = {bodyOf, b};
    double acc[BD_WORDS];
    float prev[BD_WORDS];
#pragma unroll
    for (int w = 0; w < BD_WORDS; w++) { acc[w] = 0.0; prev[w] = 0.f; }
    // elements in the order 0, 2, 1, 3: the tree's (q0 + q2) + (q1 + q3)
#pragma unroll 1
    for (int i = 0; i < 4; i++) {
      const int e = (i & 1) * 2 + (i >> 1);
      const uint32_t bndE = e == 0 ? bnd[0] : e == 1 ? bnd[1] : e == 2 ? bnd[2] : bnd[3];
      const uint32_t presE = e == 0 ? pres[0] : e == 1 ? pres[1] : e == 2 ? pres[2] : pres[3];
      const bool has = b == BD_ALL ? bndE != 0u : ((presE >> b) & 1u) != 0u;
      float q[BD_WORDS];
#pragma unroll
      for (int w = 0; w < BD_WORDS; w++) q[w] = 0.f;
      if (__any(has)) {  // wave-uniform: every lane calls wl_record, which decides with the wave who walks a row
        const int j = chunk * DIAG_CHUNK + e * SPH_BLOCK + t;
        const bool active = j < d.N;
        float rec[SPH_WALL_WORDS], term[WL_TERMS];
        float4 xi;
        wl_record(d, ws, active ? j : 0, active, rec, xi);
        wl_terms(rec, xi, term);
        // a lane without a selected particle in reach of a wall contributes +0.0, like an unselected particle of the diagnostics
        const bool sel = bndE != 0u;
        q[0] = sel ? (b == BD_ALL ? term[0] : term[1]) : 0.f;
#pragma unroll
        for (int w = 0; w < 3; w++) q[1 + w] = sel ? term[6 + w] : 0.f;    // record words 7..9
#pragma unroll
        for (int w = 0; w < 15; w++) q[4 + w] = sel ? term[9 + w] : 0.f;   // record words 10..24
      }
      if (i & 1) {
#pragma unroll
        for (int w = 0; w < BD_WORDS; w++) {
          const double pair = (double)prev[w] + (double)q[w];
          acc[w] = i == 1 ? pair : acc[w] + pair;
        }
      } else {
#pragma unroll
        for (int w = 0; w < BD_WORDS; w++) prev[w] = q[w];
      }
    }
#pragma unroll
    for (int g = 0; g < (BD_WORDS + BD_GROUP - 1) / BD_GROUP; g++) {
      if (g * BD_GROUP >= nW) break;
#pragma unroll
      for (int k = 0; k < BD_GROUP; k++)
        if (g * BD_GROUP + k < BD_WORDS) sh[k][t] = acc[g * BD_GROUP + k];
      __syncthreads();
      tree_group_sums<BD_GROUP>(sh, min(BD_GROUP, nW - g * BD_GROUP),
                                [&](int k, double x) { part[tree_at(BD_WORDS, b, g * BD_GROUP + k, chunks, chunk)] = x; });
      __syncthreads();  // sh is reused by the next group and the next body
    }
  }
}

// R(q), row-major, the contract's expressions
__device__ __forceinline__ void bd_rotation(const double* q, double* R) {
  const double w = q[0], x = q[1], y = q[2], z = q[3];
  R[0] = 1.0 - 2.0 * (y * y + z * z); R[1] = 2.0 * (x * y - w * z); R[2] = 2.0 * (x * z + w * y);
  R[3] = 2.0 * (x * y + w * z); R[4] = 1.0 - 2.0 * (x * x + z * z); R[5] = 2.0 * (y * z - w * x);
  R[6] = 2.0 * (x * z - w * y); R[7] = 2.0 * (y * z + w * x); R[8] = 1.0 - 2.0 * (x * x + y * y);
}
__device__ __forceinline__ double bd_row(double a, double b, double c, double d, double e, double f) { return (a * b + c * d) + e * f; }

// top: the tree's last level, one partial per body and word. One thread per slot.
__global__ void k_bdyn_integrate(BodyDynDev* __restrict__ D, const double* __restrict__ top, BodyDynSet set, BodyPose box, double dt,
                                 double hp, double mp) {
  const int b = threadIdx.x;
  if (b >= SPH_MAX_BODIES) return;
  double* rec = D->record[b];
  for (int w = 0; w < SPH_BODY_STATE_WORDS; w++) rec[w] = 0.0;
  D->counters[b][0] = 0u; D->counters[b][1] = 0xffffffffu; D->counters[b][2] = 0u; D->counters[b][3] = 0u;
  if (!((set.dynMask >> b) & 1u)) { rec[0] = -1.0; return; }
  const BodyDynSlot live = D->live[b];
  const sph_body_dynamics& p = live.p;
  const double* S = top + tree_at(BD_WORDS, b, 0, 1, 0);
  double Fl[3], T0[3], Tl[3], V[3], X[3], L[3], om[3], q[4];
  for (int c = 0; c < 3; c++) {
    const double C = S[1 + c], H = (S[4 + c] + S[10 + c]) + S[7 + c], TC = S[13 + c], TH = S[16 + c];
    Fl[c] = -(mp * (p.contactGain * (C / dt) + p.forceGain * H));
    T0[c] = -(mp * (p.contactGain * (TC / dt) + p.forceGain * TH));
  }
  const double* Xo = p.position;
  Tl[0] = T0[0] - (Xo[1] * Fl[2] - Xo[2] * Fl[1]);
  Tl[1] = T0[1] - (Xo[2] * Fl[0] - Xo[0] * Fl[2]);
  Tl[2] = T0[2] - (Xo[0] * Fl[1] - Xo[1] * Fl[0]);
  for (int c = 0; c < 3; c++) {
    const double F = (Fl[c] + p.mass * p.gravity[c]) + p.force[c];
    V[c] = ((p.locks >> c) & 1u) ? p.velocity[c] : p.velocity[c] + dt * (F / p.mass);
    X[c] = Xo[c] + hp * V[c];
  }
  double R[9];
  if (p.locks & 8u) {
    for (int c = 0; c < 3; c++) { L[c] = p.angularMomentum[c]; om[c] = p.spin[c]; }
  } else {
    for (int c = 0; c < 3; c++) L[c] = p.angularMomentum[c] + dt * (Tl[c] + p.torque[c]);
    bd_rotation(p.orientation, R);
    const double* J = p.inertiaInv;  // xx yy zz xy xz yz
    const double ux = bd_row(R[0], L[0], R[3], L[1], R[6], L[2]);
    const double uy = bd_row(R[1], L[0], R[4], L[1], R[7], L[2]);
    const double uz = bd_row(R[2], L[0], R[5], L[1], R[8], L[2]);
    const double wx = bd_row(J[0], ux, J[3], uy, J[4], uz);
    const double wy = bd_row(J[3], ux, J[1], uy, J[5], uz);
    const double wz = bd_row(J[4], ux, J[5], uy, J[2], uz);
    om[0] = bd_row(R[0], wx, R[1], wy, R[2], wz);
    om[1] = bd_row(R[3], wx, R[4], wy, R[5], wz);
    om[2] = bd_row(R[6], wx, R[7], wy, R[8], wz);
  }
  {
    const double w = p.orientation[0], x = p.orientation[1], y = p.orientation[2], z = p.orientation[3];
    const double dw = -((om[0] * x + om[1] * y) + om[2] * z);
    const double dx = (om[0] * w + om[1] * z) - om[2] * y;
    const double dy = (om[1] * w + om[2] * x) - om[0] * z;
    const double dz = (om[2] * w + om[0] * y) - om[1] * x;
    const double hh = 0.5 * hp;
    q[0] = w + hh * dw; q[1] = x + hh * dx; q[2] = y + hh * dy; q[3] = z + hh * dz;
    const double n = sqrt(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3]);
    for (int c = 0; c < 4; c++) q[c] = q[c] / n;
  }
  bd_rotation(q, R);
  BodyPose pose = box;
  bool finite = true;
  for (int r = 0; r < 3; r++) {
    const double tr = X[r] - bd_row(R[3 * r], p.com[0], R[3 * r + 1], p.com[1], R[3 * r + 2], p.com[2]);
    for (int c = 0; c < 3; c++) pose.m[4 * r + c] = (float)R[3 * r + c];
    pose.m[4 * r + 3] = (float)tr;
  }
  for (int k = 0; k < 12; k++) finite = finite && isfinite(pose.m[k]);
  for (int c = 0; c < 3; c++) finite = finite && isfinite(X[c]) && isfinite(V[c]) && isfinite(L[c]);
  for (int c = 0; c < 4; c++) finite = finite && isfinite(q[c]);
  BodyDynSlot next = live;
  for (int c = 0; c < 3; c++) { next.p.position[c] = X[c]; next.p.velocity[c] = V[c]; next.p.angularMomentum[c] = L[c]; }
  for (int c = 0; c < 4; c++) next.p.orientation[c] = q[c];
  next.advances = live.advances + 1u;
  D->staged[b] = next;
  D->pose[b] = pose;
  rec[0] = finite ? 0.0 : 2.0;
  rec[1] = (double)set.count[b];
  rec[2] = (double)live.advances;
  for (int c = 0; c < 3; c++) {
    rec[4 + c] = X[c]; rec[11 + c] = V[c]; rec[14 + c] = L[c]; rec[17 + c] = om[c]; rec[20 + c] = Fl[c]; rec[23 + c] = Tl[c];
  }
  for (int c = 0; c < 4; c++) rec[7 + c] = q[c];
  rec[26] = top[tree_at(BD_WORDS, BD_ALL, 0, 1, 0)];
  rec[27] = S[0];
}

// blockIdx.y = slot. Neither pass runs for a body whose integration was not finite; the commit needs a validation without offenders.
template <bool COMMIT>
__global__ __launch_bounds__(SPH_BLOCK) void k_bdyn_pose(BodyDynDev* __restrict__ D, BodyDynSet set, int N, float4* __restrict__ pos,
                                                         float4* __restrict__ vel) {
  const int b = blockIdx.y;
  if (!((set.dynMask >> b) & 1u) || (int)(blockIdx.x * SPH_BLOCK) >= set.count[b]) return;  // (block-uniform)
  if (D->record[b][0] != 0.0) return;
  if (COMMIT && D->counters[b][0] != 0u) return;
  const BodyPose a = D->pose[b];
  body_pose_member<COMMIT>(a, set.ids[b], set.ref[b], set.count[b], N, pos, vel, D->counters[b]);
}

__global__ void k_bdyn_finish(BodyDynDev* __restrict__ D, uint32_t dynMask, float r0) {
  const int b = threadIdx.x;
  if (b >= SPH_MAX_BODIES || !((dynMask >> b) & 1u)) return;
  double* rec = D->record[b];
  if (rec[0] != 0.0) return;
  const uint32_t offenders = D->counters[b][0];
  if (offenders) {
    rec[0] = 1.0;
    rec[28] = (double)offenders;
    rec[29] = (double)D->counters[b][1];
    return;
  }
  D->live[b] = D->staged[b];
  rec[2] = (double)D->staged[b].advances;
  rec[3] = (double)(sqrtf(__uint_as_float(D->counters[b][2])) / r0);  // sph_body_set_pose's tunnelling number
}

// ---- sph_body_set_dynamics: members shared with another dynamic body -----------------------------------------------------------
__global__ __launch_bounds__(SPH_BLOCK) void k_bdyn_overlap_mark(const uint32_t* __restrict__ ids, int count, int N,
                                                                 unsigned long long* __restrict__ seen) {
  const int r = blockIdx.x * SPH_BLOCK + threadIdx.x;
  if (r >= count) return;
  const uint32_t o = ids[r];
  if (o < (uint32_t)N) atomicOr(&seen[o >> 6], 1ull << (o & 63u));
}

// every member of `slot` that another body has marked counts once, however many bodies hold it
__global__ __launch_bounds__(SPH_BLOCK) void k_bdyn_overlap_count(const uint32_t* __restrict__ ids, int count, int N,
                                                                  const unsigned long long* __restrict__ seen,
                                                                  uint32_t* __restrict__ overlap) {
  const int r = blockIdx.x * SPH_BLOCK + threadIdx.x;
  if (r >= count) return;
  const uint32_t o = ids[r];
  if (o >= (uint32_t)N || !((seen[o >> 6] >> (o & 63u)) & 1ull)) return;
  atomicAdd(&overlap[0], 1u);
  atomicMin(&overlap[1], o);
}

// ---- launchers ---------------------------------------------------------------------------------------------------------------
static size_t bd_map_bytes(int N) { return ((size_t)std::max(N, 1) + 255) & ~(size_t)255; }

size_t sphk_bdyn_scratch_bytes(int N) { return bd_map_bytes(N) + sizeof(double) * tree_level_chunks(N) * BD_SLOTS * BD_WORDS; }

int sphk_bdyn_overlap(sph_solver* s, const BodyDynSet& set, int slot, unsigned long long* seen, BodyDynDev* D) {
  const int N = s->d.N;
  SPH_HIP(hipMemsetAsync(seen, 0, sizeof(unsigned long long) * (size_t)sph_blocks(std::max(N, 1), 64), s->stream));
  SPH_HIP(hipMemsetAsync(&D->overlap[0], 0, sizeof(uint32_t), s->stream));
  SPH_HIP(hipMemsetAsync(&D->overlap[1], 0xff, sizeof(uint32_t), s->stream));
  bool any = false;
  for (int b = 0; b < SPH_MAX_BODIES; b++) {
    if (b == slot || !((set.dynMask >> b) & 1u) || set.count[b] <= 0) continue;
    hipLaunchKernelGGL(k_bdyn_overlap_mark, dim3(sph_blocks(set.count[b])), dim3(SPH_BLOCK), 0, s->stream, set.ids[b], set.count[b], N, seen);
    SPH_HIP(hipGetLastError());
    any = true;
  }
  if (any && set.count[slot] > 0) {
    hipLaunchKernelGGL(k_bdyn_overlap_count, dim3(sph_blocks(set.count[slot])), dim3(SPH_BLOCK), 0, s->stream, set.ids[slot],
                       set.count[slot], N, (const unsigned long long*)seen, D->overlap);
    SPH_HIP(hipGetLastError());
  }
  return SPH_OK;
}

int sphk_bdyn_advance(sph_solver* s, const BodyDynSet& set, const BodyPose& box, void* scratch, BodyDynDev* D) {
  const int N = s->d.N;
  uint8_t* bodyOf = (uint8_t*)scratch;
  double* cur = (double*)((char*)scratch + bd_map_bytes(N));
  int most = 0;
  for (int b = 0; b < SPH_MAX_BODIES; b++)
    if ((set.dynMask >> b) & 1u) most = std::max(most, set.count[b]);
  if (most <= 0) return SPH_OK;
  const dim3 members(sph_blocks(most), SPH_MAX_BODIES);
  SPH_HIP(hipMemsetAsync(bodyOf, 0xff, bd_map_bytes(N), s->stream));
  hipLaunchKernelGGL(k_bdyn_map, members, dim3(SPH_BLOCK), 0, s->stream, s->d, set, bodyOf);
  SPH_HIP(hipGetLastError());
  const int chunks = tree_chunks(N);
  hipLaunchKernelGGL(k_bdyn_leaf, dim3(chunks), dim3(SPH_BLOCK), 0, s->stream, s->d, (const uint8_t*)bodyOf, set.dynMask, cur, chunks);
  SPH_HIP(hipGetLastError());
  // the rows of non-dynamic bodies and words 1..18 of the count row are unwritten at every level: not reduced, never read
  TreeShape S = tree_shape(BD_WORDS, BD_WORDS, set.dynMask | (1u << BD_ALL));
  S.shortRow = BD_ALL; S.shortWords = 1;
  double *top = nullptr, *end = nullptr;
  int rc = sphk_tree_upper(s, S, BD_SLOTS, cur, chunks, &top, &end);
  if (rc != SPH_OK) return rc;
  hipLaunchKernelGGL(k_bdyn_integrate, dim3(1), dim3(64), 0, s->stream, D, (const double*)top, set, box, (double)s->d.dt,
                     (double)s->d.posTimeStep, (double)s->cfg.mass);
  SPH_HIP(hipGetLastError());
  hipLaunchKernelGGL(k_bdyn_pose<false>, members, dim3(SPH_BLOCK), 0, s->stream, D, set, N, s->d.posOrig, s->d.velOrig);
  SPH_HIP(hipGetLastError());
  rc = sph_guard_position_write(s);  // an asynchronous read-back of posOrig finishes its device copy first
  if (rc != SPH_OK) return rc;
  hipLaunchKernelGGL(k_bdyn_pose<true>, members, dim3(SPH_BLOCK), 0, s->stream, D, set, N, s->d.posOrig, s->d.velOrig);
  SPH_HIP(hipGetLastError());
  hipLaunchKernelGGL(k_bdyn_finish, dim3(1), dim3(64), 0, s->stream, D, set.dynMask, s->d.r0);
  SPH_HIP(hipGetLastError());
  return SPH_OK;
}

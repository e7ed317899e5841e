// Kinematic bodies (include/sphmi.h: sph_body_*): ordered groups of boundary particles of the original-order state
// (posOrig, velOrig) that are placed at a rigid image of their reference placement between two steps.
//   k_body_seen_ids      one lane per list entry: 64-bit atomicOr into the cleared `seen` mask (1 bit per particle, the layout of
//                        k_edit_mark_ids); an id that was seen already is or-ed into the `twice` mask as well
//   k_body_judge_ids     one lane per list entry: an offender is an id >= N, a particle that is not a boundary particle, or an id in
//                        `twice` (every occurrence, so that neither the count nor the lowest index depends on which lane came first)
//   k_body_block_counts  one lane per 256-block: the MARKED particles of the block from the four ballot words k_edit_mark_region
//                        wrote (k_edit_counts counts the unmarked ones); (k_select_scan) and (k_select_scatter) do the rest
//   k_body_gather        member k: ref[2k] = posOrig[id], ref[2k + 1] = velOrig[id] (the wall normal lives in the velocity slot)
//   k_body_pose<false>   member k: the new position from the reference row, its validation, d2 against the current position; the
//                        offenders are counted, the lowest one found and the largest d2 kept by integer atomics, one per wave
//   k_body_pose<true>    the same expressions again, and the two 16-byte stores: runs only after the validation has passed
//   k_body_keep          member k survives a removal when map[id] >= 0: one ballot word per wave, the mask layout of k_select_flags;
//                        k_body_block_counts and (k_select_scan) turn the words into block offsets
//   k_body_compact       survivor k -> slot off[block] + rank in the block (popcounts of the mask words), its id through the map, its
//                        two reference rows with 16-byte loads and stores
// Integer ballots, popcounts, sums, or, min and max only: every result is a function of the state and the arguments, whatever the
// order the blocks run in. No floating-point atomics, no LDS.
#include "sph_common.h"
#include "sph_body_pose.h"  // BODY_WAVE, body_pose_member: one member under a pose

__global__ __launch_bounds__(SPH_BLOCK) void k_body_seen_ids(const uint32_t* __restrict__ ids, int count, int N,
                                                             unsigned long long* __restrict__ seen,
                                                             unsigned long long* __restrict__ twice) {
  const int r = blockIdx.x * SPH_BLOCK + threadIdx.x;
  if (r >= count) return;
  const uint32_t o = ids[r];
  if (o >= (uint32_t)N) return;  // (keeps the atomics inside the masks; k_body_judge_ids counts the entry)
  const unsigned long long bit = 1ull << (o & 63u);
  if (atomicOr(&seen[o >> 6], bit) & bit) atomicOr(&twice[o >> 6], bit);
}

__global__ __launch_bounds__(SPH_BLOCK) void k_body_judge_ids(const uint32_t* __restrict__ ids, int count, int N,
                                                              const float4* __restrict__ pos,
                                                              const unsigned long long* __restrict__ twice,
                                                              uint32_t* __restrict__ counters) {
  const int r = blockIdx.x * SPH_BLOCK + threadIdx.x;
  if (r >= count) return;
  const uint32_t o = ids[r];
  bool bad = o >= (uint32_t)N;
  if (!bad) bad = (int)pos[o].w != SPH_BOUNDARY_PARTICLE || ((twice[o >> 6] >> (o & 63u)) & 1ull);
  if (bad) {
    atomicAdd(&counters[0], 1u);
    atomicMin(&counters[1], (uint32_t)r);
  }
}

// blockCnt[b] = marked particles of block b (mask[4 b + w], bit l = particle 256 b + 64 w + l; the bits past N are clear)
__global__ __launch_bounds__(SPH_BLOCK) void k_body_block_counts(const unsigned long long* __restrict__ mask, int nb,
                                                                 uint32_t* __restrict__ blockCnt) {
  const int b = blockIdx.x * SPH_BLOCK + threadIdx.x;
  if (b >= nb) return;
  uint32_t n = 0;
#pragma unroll
  for (int w = 0; w < BODY_WAVES; w++) n += (uint32_t)__popcll(mask[(size_t)b * BODY_WAVES + w]);
  blockCnt[b] = n;
}

__global__ __launch_bounds__(SPH_BLOCK) void k_body_gather(const uint32_t* __restrict__ ids, int count, int N,
                                                           const float4* __restrict__ pos, const float4* __restrict__ vel,
                                                           float4* __restrict__ ref) {
  const int k = blockIdx.x * SPH_BLOCK + threadIdx.x;
  if (k >= count) return;
  const uint32_t o = ids[k];
  if (o >= (uint32_t)N) return;  // (never: the definition has been checked)
  ref[2 * (size_t)k] = pos[o];
  ref[2 * (size_t)k + 1] = vel[o];
}

// COMMIT false: the validation's three counters; COMMIT true: the stores (body_pose_member, sph_body_pose.h)
template <bool COMMIT>
__global__ __launch_bounds__(SPH_BLOCK) void k_body_pose(BodyPose a, const uint32_t* __restrict__ ids, const float4* __restrict__ ref,
                                                         int count, int N, float4* __restrict__ pos, float4* __restrict__ vel,
                                                         uint32_t* __restrict__ counters) {
  body_pose_member<COMMIT>(a, ids, ref, count, N, pos, vel, counters);
}

// mask[4 b + w]: the ballot of wave w of block b (bit l = member 256 b + 64 w + l survives); blockCnt[b] its total
__global__ __launch_bounds__(SPH_BLOCK) void k_body_keep(const uint32_t* __restrict__ ids, int count, const int32_t* __restrict__ map,
                                                         int oldN, unsigned long long* __restrict__ mask) {
  const int k = blockIdx.x * SPH_BLOCK + threadIdx.x;
  bool keep = false;
  if (k < count) {
    const uint32_t o = ids[k];
    keep = o < (uint32_t)oldN && map[o] >= 0;
  }
  const unsigned long long word = __ballot(keep);
  if ((threadIdx.x & (BODY_WAVE - 1)) == 0) mask[(size_t)blockIdx.x * BODY_WAVES + threadIdx.x / BODY_WAVE] = word;
}

__global__ __launch_bounds__(SPH_BLOCK) void k_body_compact(const uint32_t* __restrict__ ids, const float4* __restrict__ ref, int count,
                                                            const int32_t* __restrict__ map, const unsigned long long* __restrict__ mask,
                                                            const uint32_t* __restrict__ off, uint32_t* __restrict__ idsOut,
                                                            float4* __restrict__ refOut) {
  const int b = blockIdx.x;
  const int k = b * SPH_BLOCK + threadIdx.x;
  if (k >= count) return;
  const int lane = threadIdx.x & (BODY_WAVE - 1), wave = threadIdx.x / BODY_WAVE;
  const unsigned long long mine = mask[(size_t)b * BODY_WAVES + wave];
  if (!((mine >> lane) & 1ull)) return;
  uint32_t at = off[b];
#pragma unroll
  for (int w = 0; w < BODY_WAVES; w++)
    if (w < wave) at += (uint32_t)__popcll(mask[(size_t)b * BODY_WAVES + w]);
  at += (uint32_t)__popcll(mine & ((1ull << lane) - 1ull));
  if (at >= (uint32_t)count) return;  // (never: the guard keeps a corrupted mask inside the arrays)
  idsOut[at] = (uint32_t)map[ids[k]];  // (the bit is set: ids[k] < oldN and map[ids[k]] >= 0)
  refOut[2 * (size_t)at] = ref[2 * (size_t)k];
  refOut[2 * (size_t)at + 1] = ref[2 * (size_t)k + 1];
}

// ---- launchers ---------------------------------------------------------------------------------------------------------------
#define BODY_HEAD 256  // bytes in front of a scratch: the counters of the call

static size_t body_mask_bytes(int N) { return ((sizeof(unsigned long long) * (size_t)sph_blocks(N > 0 ? N : 1, BODY_WAVE)) + 255) & ~(size_t)255; }

// scratch: counters | seen mask | twice mask
size_t sphk_body_check_bytes(int N) { return BODY_HEAD + 2 * body_mask_bytes(N); }

int sphk_body_check_ids(sph_solver* s, const uint32_t* ids, int count, void* scratch, uint32_t** counters) {
  const int N = s->d.N;
  uint32_t* c = (uint32_t*)scratch;
  unsigned long long* seen = (unsigned long long*)((char*)scratch + BODY_HEAD);
  unsigned long long* twice = (unsigned long long*)((char*)scratch + BODY_HEAD + body_mask_bytes(N));
  SPH_HIP(hipMemsetAsync(c, 0, sizeof(uint32_t), s->stream));
  SPH_HIP(hipMemsetAsync(c + 1, 0xff, sizeof(uint32_t), s->stream));
  SPH_HIP(hipMemsetAsync(seen, 0, 2 * body_mask_bytes(N), s->stream));
  hipLaunchKernelGGL(k_body_seen_ids, dim3(sph_blocks(count)), dim3(SPH_BLOCK), 0, s->stream, ids, count, N, seen, twice);
  SPH_HIP(hipGetLastError());
  hipLaunchKernelGGL(k_body_judge_ids, dim3(sph_blocks(count)), dim3(SPH_BLOCK), 0, s->stream, ids, count, N, (const float4*)s->d.posOrig,
                     (const unsigned long long*)twice, c);
  SPH_HIP(hipGetLastError());
  *counters = c;
  return SPH_OK;
}

int sphk_body_count_marks(sph_solver* s, void* scratch, uint32_t** totals) {
  const SelLayout L = sphk_select_layout(s->d.N);
  char* base = (char*)scratch;
  hipLaunchKernelGGL(k_body_block_counts, dim3(sph_blocks(L.nb)), dim3(SPH_BLOCK), 0, s->stream,
                     (const unsigned long long*)(base + L.mask), L.nb, (uint32_t*)(base + L.blockCnt));
  SPH_HIP(hipGetLastError());
  *totals = (uint32_t*)(base + L.totals);
  return sphk_select_scan(s, scratch, s->d.N);
}

int sphk_body_gather(sph_solver* s, const uint32_t* ids, int count, float4* ref) {
  if (count <= 0) return SPH_OK;
  hipLaunchKernelGGL(k_body_gather, dim3(sph_blocks(count)), dim3(SPH_BLOCK), 0, s->stream, ids, count, s->d.N,
                     (const float4*)s->d.posOrig, (const float4*)s->d.velOrig, ref);
  SPH_HIP(hipGetLastError());
  return SPH_OK;
}

int sphk_body_pose_validate(sph_solver* s, const BodyPose& a, const uint32_t* ids, const float4* ref, int count, uint32_t* counters) {
  SPH_HIP(hipMemsetAsync(counters, 0, 3 * sizeof(uint32_t), s->stream));
  SPH_HIP(hipMemsetAsync(counters + 1, 0xff, sizeof(uint32_t), s->stream));
  hipLaunchKernelGGL(k_body_pose<false>, dim3(sph_blocks(count)), dim3(SPH_BLOCK), 0, s->stream, a, ids, ref, count, s->d.N,
                     s->d.posOrig, s->d.velOrig, counters);
  SPH_HIP(hipGetLastError());
  return SPH_OK;
}

int sphk_body_pose_commit(sph_solver* s, const BodyPose& a, const uint32_t* ids, const float4* ref, int count) {
  hipLaunchKernelGGL(k_body_pose<true>, dim3(sph_blocks(count)), dim3(SPH_BLOCK), 0, s->stream, a, ids, ref, count, s->d.N,
                     s->d.posOrig, s->d.velOrig, (uint32_t*)nullptr);
  SPH_HIP(hipGetLastError());
  return SPH_OK;
}

// scratch: counters (unused head) | the selection's layout for `count` entries
size_t sphk_body_compact_bytes(int count) { return BODY_HEAD + sphk_select_layout(count).bytes; }

int sphk_body_compact(sph_solver* s, const uint32_t* ids, const float4* ref, int count, const int32_t* map, int oldN, void* scratch,
                      uint32_t* idsOut, float4* refOut, uint32_t** totals) {
  const SelLayout L = sphk_select_layout(count);
  char* base = (char*)scratch + BODY_HEAD;
  unsigned long long* mask = (unsigned long long*)(base + L.mask);
  hipLaunchKernelGGL(k_body_keep, dim3(L.nb), dim3(SPH_BLOCK), 0, s->stream, ids, count, map, oldN, mask);
  SPH_HIP(hipGetLastError());
  hipLaunchKernelGGL(k_body_block_counts, dim3(sph_blocks(L.nb)), dim3(SPH_BLOCK), 0, s->stream, (const unsigned long long*)mask, L.nb,
                     (uint32_t*)(base + L.blockCnt));
  SPH_HIP(hipGetLastError());
  const int rc = sphk_select_scan(s, base, count);
  if (rc != SPH_OK) return rc;
  hipLaunchKernelGGL(k_body_compact, dim3(L.nb), dim3(SPH_BLOCK), 0, s->stream, ids, ref, count, map, (const unsigned long long*)mask,
                     (const uint32_t*)(base + L.off), idsOut, refOut);
  SPH_HIP(hipGetLastError());
  *totals = (uint32_t*)(base + L.totals);
  return SPH_OK;
}

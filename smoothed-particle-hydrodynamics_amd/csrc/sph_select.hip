// Particle selection, the free-surface measure and the compact read-back (include/sphmi.h: sph_particle_measure /
// sph_select_particles / sph_read_selection). Read-only on every solver array. Type, key and box are the rule of
// sph_selector.h, which also names the quantities of the streamed terms.
//   k_select_flags     one lane per sorted particle: type / key / box / component and the terms on streamed arrays first, the row
//                      walk (neighbour count, surface measure) only for lanes that are still alive; one ballot word per wave
//                      (the 1-bit-per-particle mask) and the survivors per block
//   k_select_scan      one workgroup: exclusive offsets of the block counts, the total for the host's one blocking read
//   k_select_scatter   list[block offset + rank in the block] = j, the rank from the mask words (popcounts): ascending sorted
//                      index without atomics, whatever the order the blocks run in
//   k_select_gather    one lane per selected particle: the 12-word record (one row walk for count and measure), the original id
//   k_particle_measure the measure of every sorted particle of a range
// Everything a result depends on is a per-particle function of the state and the arguments; the only cross-lane operations are
// integer ballots, popcounts and sums. No floating-point atomics.
#include "sph_common.h"
#include "sph_row_walk.h"
#include "sph_selector.h"  // the selection rule and the streamed terms' quantities

#include <algorithm>

#define SEL_WAVE 64
#define SEL_WAVES (SPH_BLOCK / SEL_WAVE)
#define SEL_SCAN_THREADS 1024

// XCD-aware block order (as cc_block): each XCD works on one contiguous eighth of the sorted range, so that the sortedPos lines
// its row walks gather stay in that XCD's L2. A permutation of the block ids: it changes which block computes what, never a result.
__device__ __forceinline__ int sel_block(int nblocks) {
  const int b = blockIdx.x;
  const int per = nblocks >> 3, even = per << 3;
  if (b >= even) return b;
  return (b & 7) * per + (b >> 3);
}

// The row of sorted particle i: count = its entries >= 0 as a float (sph_histogram's field 3), and, if MEASURE, the surface
// measure of the contract: slots in ascending order, float throughout, no contraction (-ffp-contract=off), IEEE / and sqrtf.
template <bool MEASURE>
__device__ __forceinline__ void select_row(const SphDev& d, float ss2, int i, float& count, float& m) {
  float4 pi = make_float4(0.f, 0.f, 0.f, 0.f);
  if (MEASURE) pi = d.sortedPos[i];
  int n = 0;
  float W = 0.f, Bx = 0.f, By = 0.f, Bz = 0.f;
  sph_row_for_each_slot(d, i, [&](int j) {
    if (j < 0) return;
    n++;
    if (!MEASURE || j == i || j >= d.N) return;
    const float4 pj = d.sortedPos[j];
    const float dx = pj.x - pi.x, dy = pj.y - pi.y, dz = pj.z - pi.z;
    const float r2 = dx * dx + dy * dy + dz * dz;
    const float t = d.hs2 - r2 * ss2;
    if (!(t > 0.f)) return;
    const float w = (t * t) * t;
    W += w;
    Bx += w * dx; By += w * dy; Bz += w * dz;
  });
  count = (float)n;
  m = 1.0f;
  if (MEASURE && W != 0.f) {
    const float cx = Bx / W, cy = By / W, cz = Bz / W;
    m = sqrtf((cx * cx + cy * cy) + cz * cz) / d.h;
  }
}

__device__ __forceinline__ bool select_test(const SphDev& d, const SelectArgs& a, int j) {
  const float4 p = d.sortedPos[j];
  if (!sph_selected(d, a.sel, j, p)) return false;
  if (a.component >= 0 && a.labels[j] != a.component) return false;
  for (int k = 0; k < a.termCount; k++) {  // the terms on streamed arrays
    if (a.field[k] == 3 || a.field[k] == 7) continue;  // they need the row: below, once for both, by the lanes still alive
    const float q = sph_particle_quantity(d, a.field[k], j, p);
    if (!(q >= a.lo[k] && q < a.hi[k])) return false;
  }
  if (!a.needRow) return true;
  float count, m;
  if (a.needMeasure) select_row<true>(d, a.ss2, j, count, m);
  else select_row<false>(d, a.ss2, j, count, m);
  for (int k = 0; k < a.termCount; k++) {
    if (a.field[k] != 3 && a.field[k] != 7) continue;
    const float q = a.field[k] == 3 ? count : m;
    if (!(q >= a.lo[k] && q < a.hi[k])) return false;
  }
  return true;
}

// mask[4 * b + w]: the ballot of wave w of logical block b (bit l = particle 256 b + 64 w + l is selected); blockCnt[b] its total.
__global__ __launch_bounds__(SPH_BLOCK) void k_select_flags(SphDev d, SelectArgs a, unsigned long long* __restrict__ mask,
                                                            uint32_t* __restrict__ blockCnt) {
  __shared__ uint32_t waveCnt[SEL_WAVES];
  const int b = sel_block(gridDim.x);
  const int j = b * SPH_BLOCK + threadIdx.x;
  const int lane = threadIdx.x & (SEL_WAVE - 1), wave = threadIdx.x / SEL_WAVE;
  const bool ok = j < d.N && select_test(d, a, j);
  const unsigned long long word = __ballot(ok);
  if (lane == 0) {
    mask[(size_t)b * SEL_WAVES + wave] = word;
    waveCnt[wave] = (uint32_t)__popcll(word);
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t n = 0;
#pragma unroll
    for (int w = 0; w < SEL_WAVES; w++) n += waveCnt[w];
    blockCnt[b] = n;
  }
}

// off[b] = selected particles in blocks < b; totals[0..1] = the 64-bit total. One workgroup: each thread sums a contiguous run
// of blocks, the run sums are scanned in LDS, then each thread writes its run's offsets (the pattern of k_cc_scan, with the
// loads of a run issued eight at a time).
__global__ __launch_bounds__(SEL_SCAN_THREADS) void k_select_scan(const uint32_t* __restrict__ blockCnt, int nb, uint32_t* __restrict__ off,
                                                                  uint32_t* __restrict__ totals) {
  __shared__ uint32_t sS[SEL_SCAN_THREADS];
  const int tid = threadIdx.x;
  const int per = (nb + SEL_SCAN_THREADS - 1) / SEL_SCAN_THREADS;
  const int b0 = min(tid * per, nb), b1 = min(b0 + per, nb);
  uint32_t q = 0;
  int b = b0;
  for (; b + 8 <= b1; b += 8) {  // eight independent loads in flight: a thread's run is contiguous, so the wave's loads do not coalesce
    uint32_t v[8];
#pragma unroll
    for (int k = 0; k < 8; k++) v[k] = blockCnt[b + k];
#pragma unroll
    for (int k = 0; k < 8; k++) q += v[k];
  }
  for (; b < b1; b++) q += blockCnt[b];
  sS[tid] = q;
  __syncthreads();
  for (int o = 1; o < SEL_SCAN_THREADS; o <<= 1) {  // inclusive Hillis-Steele scan
    uint32_t add = 0;
    if (tid >= o) add = sS[tid - o];
    __syncthreads();
    sS[tid] += add;
    __syncthreads();
  }
  uint32_t o = sS[tid] - q;
  for (b = b0; b + 8 <= b1; b += 8) {
    uint32_t v[8];
#pragma unroll
    for (int k = 0; k < 8; k++) v[k] = blockCnt[b + k];
#pragma unroll
    for (int k = 0; k < 8; k++) { off[b + k] = o; o += v[k]; }
  }
  for (; b < b1; b++) { off[b] = o; o += blockCnt[b]; }
  if (tid == SEL_SCAN_THREADS - 1) { totals[0] = sS[tid]; totals[1] = 0u; }  // (N <= SPH_MAX_PARTICLES < 2^31)
}

__global__ __launch_bounds__(SPH_BLOCK) void k_select_scatter(int N, const unsigned long long* __restrict__ mask,
                                                              const uint32_t* __restrict__ off, uint32_t total, int32_t* __restrict__ list) {
  const int b = blockIdx.x;
  const int j = b * SPH_BLOCK + threadIdx.x;
  const int lane = threadIdx.x & (SEL_WAVE - 1), wave = threadIdx.x / SEL_WAVE;
  const unsigned long long mine = mask[(size_t)b * SEL_WAVES + wave];
  if (!((mine >> lane) & 1ull) || j >= N) return;
  uint32_t at = off[b];
#pragma unroll
  for (int w = 0; w < SEL_WAVES; w++)
    if (w < wave) at += (uint32_t)__popcll(mask[(size_t)b * SEL_WAVES + w]);
  at += (uint32_t)__popcll(mine & ((1ull << lane) - 1ull));
  if (at < total) list[at] = j;  // (always: the guard keeps a corrupted mask inside the list)
}

__global__ __launch_bounds__(SPH_BLOCK) void k_select_gather(SphDev d, float ss2, const int32_t* __restrict__ list, int n,
                                                             float4* __restrict__ records, uint32_t* __restrict__ origId) {
  const int r = blockIdx.x * SPH_BLOCK + threadIdx.x;
  if (r >= n) return;
  const int j = list[r];
  if (j < 0 || j >= d.N) return;
  const float4 p = d.sortedPos[j];
  const float4 v = d.sortedVel[j];
  float count, m;
  select_row<true>(d, ss2, j, count, m);
  float4* rec = records + (size_t)r * (SPH_SELECT_WORDS / 4);
  rec[0] = p;  // x, y, z, type (the position.w bit pattern)
  rec[1] = make_float4(v.x, v.y, v.z, d.rho[j]);
  rec[2] = make_float4(d.rp[j].y, count, m, 0.f);
  origId[r] = d.vals[j];
}

__global__ __launch_bounds__(SPH_BLOCK) void k_particle_measure(SphDev d, float ss2, int first, int n, float* __restrict__ out) {
  const int r = sel_block(gridDim.x) * SPH_BLOCK + threadIdx.x;
  if (r >= n) return;
  float count, m;
  select_row<true>(d, ss2, first + r, count, m);
  out[r] = m;
}

// ---- launchers ---------------------------------------------------------------------------------------------------------------
static size_t sel_align(size_t b) { return (b + 255) & ~(size_t)255; }

// scratch layout: mask[4 nb] (64-bit ballots) | blockCnt[nb] | off[nb] | totals
SelLayout sphk_select_layout(int N) {
  SelLayout L;
  L.nb = N > 0 ? sph_blocks(N) : 1;
  size_t at = 0;
  L.mask = at; at += sel_align(sizeof(unsigned long long) * SEL_WAVES * (size_t)L.nb);
  L.blockCnt = at; at += sel_align(sizeof(uint32_t) * (size_t)L.nb);
  L.off = at; at += sel_align(sizeof(uint32_t) * (size_t)L.nb);
  L.totals = at; at += 256;
  L.bytes = at;
  return L;
}

size_t sphk_select_scratch_bytes(int N) { return sphk_select_layout(N).bytes; }

int sphk_select_count(sph_solver* s, const SelectArgs& a, void* scratch, uint32_t** totals) {
  const SelLayout L = sphk_select_layout(s->d.N);
  char* base = (char*)scratch;
  hipLaunchKernelGGL(k_select_flags, dim3(L.nb), dim3(SPH_BLOCK), 0, s->stream, s->d, a, (unsigned long long*)(base + L.mask),
                     (uint32_t*)(base + L.blockCnt));
  SPH_HIP(hipGetLastError());
  *totals = (uint32_t*)(base + L.totals);
  return sphk_select_scan(s, scratch, s->d.N);
}

int sphk_select_scan(sph_solver* s, void* scratch, int N) {
  const SelLayout L = sphk_select_layout(N);
  char* base = (char*)scratch;
  hipLaunchKernelGGL(k_select_scan, dim3(1), dim3(SEL_SCAN_THREADS), 0, s->stream, (const uint32_t*)(base + L.blockCnt), L.nb,
                     (uint32_t*)(base + L.off), (uint32_t*)(base + L.totals));
  SPH_HIP(hipGetLastError());
  return SPH_OK;
}

int sphk_select_scatter(sph_solver* s, void* scratch, uint32_t total, int32_t* list) {
  if (total == 0) return SPH_OK;
  const SelLayout L = sphk_select_layout(s->d.N);
  char* base = (char*)scratch;
  hipLaunchKernelGGL(k_select_scatter, dim3(L.nb), dim3(SPH_BLOCK), 0, s->stream, s->d.N, (const unsigned long long*)(base + L.mask),
                     (const uint32_t*)(base + L.off), total, list);
  SPH_HIP(hipGetLastError());
  return SPH_OK;
}

int sphk_select_gather(sph_solver* s, float ss2, const int32_t* list, int n, float* records, uint32_t* origId) {
  if (n <= 0) return SPH_OK;
  hipLaunchKernelGGL(k_select_gather, dim3(sph_blocks(n)), dim3(SPH_BLOCK), 0, s->stream, s->d, ss2, list, n, (float4*)records, origId);
  SPH_HIP(hipGetLastError());
  return SPH_OK;
}

int sphk_particle_measure(sph_solver* s, float ss2, int first, int n, float* out) {
  if (n <= 0) return SPH_OK;
  hipLaunchKernelGGL(k_particle_measure, dim3(sph_blocks(n)), dim3(SPH_BLOCK), 0, s->stream, s->d, ss2, first, n, out);
  SPH_HIP(hipGetLastError());
  return SPH_OK;
}

// The lock-free union-find that the particle components (sph_components.hip) and the surface shells (sph_shells.hip) share, and
// the small device helpers both number and tabulate their sets with. The invariants: parent[x] <= x always,
// and parent[x] is a member of x's set, so every tree's root is the minimum of its set whatever the interleaving. Every access
// to `parent` while hooks are running is an agent-scope atomic (the XCDs' L2s are not coherent for plain accesses); a stale value
// read on the way is still a smaller member of the same set, and a hook is a compare-and-swap that expects parent[r] == r, so it
// fails, and is retried from the value it returns, if r has stopped being a root. Every pointer walk and every retry loop is
// bounded by limit + 1 steps (limit = the number of nodes); an overrun sets err[0] instead of spinning.
#pragma once
#include "sph_common.h"

#define CC_WAVE 64
#define CC_WAVES (SPH_BLOCK / CC_WAVE)

__device__ __forceinline__ int cc_load(const int32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// Root of x's tree as far as this lane can see it (a value that was a root when it was read). Path halving: parent[x] moves to
// its grandparent by an atomic minimum, so that a slower lane's older value never moves it back up.
__device__ __forceinline__ int cc_find(int32_t* parent, int x, int limit, uint32_t* err) {
  int steps = 0;
  int p = cc_load(parent + x);
  while (p != x) {
    const int g = cc_load(parent + p);
    if (g != p) __hip_atomic_fetch_min(parent + x, g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    x = p;
    p = g;
    if (++steps > limit) { atomicOr(err, 1u); break; }
  }
  return x;
}

// Joins the sets of a and b; returns the root the pair ended under (a member of both sets, not larger than either root seen).
__device__ __forceinline__ int cc_union(int32_t* parent, int i, int j, int limit, uint32_t* err) {
  int a = cc_find(parent, i, limit, err), b = cc_find(parent, j, limit, err);
  int tries = 0;
  while (a != b) {
    const int hi = a > b ? a : b, lo = a > b ? b : a;
    int seen = hi;
    if (__hip_atomic_compare_exchange_strong(parent + hi, &seen, lo, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) return lo;
    // hi has been hooked by another lane meanwhile: go on from where it points now (a smaller member of its set)
    a = cc_find(parent, seen, limit, err);
    b = lo;
    if (++tries > limit) { atomicOr(err, 2u); return lo; }
  }
  return a;
}

// Exclusive prefix of v over the block's lanes (lane order = index order) and the block total.
__device__ __forceinline__ uint32_t cc_block_exclusive(uint32_t v, uint32_t& total) {
  __shared__ uint32_t waveSum[CC_WAVES];
  const int lane = threadIdx.x & (CC_WAVE - 1), wave = threadIdx.x / CC_WAVE;
  uint32_t inc = v;
  for (int o = 1; o < CC_WAVE; o <<= 1) {
    const uint32_t u = (uint32_t)__shfl_up((int)inc, o, CC_WAVE);
    if (lane >= o) inc += u;
  }
  if (lane == CC_WAVE - 1) waveSum[wave] = inc;
  __syncthreads();
  uint32_t before = 0, all = 0;
#pragma unroll
  for (int w = 0; w < CC_WAVES; w++) {
    const uint32_t s = waveSum[w];
    if (w < wave) before += s;
    all += s;
  }
  total = all;
  __syncthreads();  // waveSum is reused by a second call
  return before + inc - v;
}

// order-preserving integer image of a float (signed compare) and back
__device__ __forceinline__ int cc_ordered(float f) { const int i = __float_as_int(f); return i ^ ((i >> 31) & 0x7fffffff); }
__device__ __forceinline__ float cc_unordered(int i) { return __int_as_float(i ^ ((i >> 31) & 0x7fffffff)); }

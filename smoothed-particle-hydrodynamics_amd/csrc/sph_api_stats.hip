// C ABI of libsphmi.so (include/sphmi.h), the time statistics on a lattice: sph_stats_define / sph_stats_get / sph_stats_accumulate /
// sph_stats_reset / sph_stats_read / sph_stats_read_moments. Statistics are passive and belong to the solver, as
// probes do: no call here says sph_state_changes or touches `progress`, and every buffer is the feature's own. What the translation
// units of the ABI share is in sph_api_internal.h.
#include <algorithm>
#include <cmath>

#include "sph_api_internal.h"

static const size_t kStatsNode = sizeof(double) * SPH_STATS_WORDS;          // bytes of a node's accumulators
static const size_t kStatsMoment = sizeof(float) * SPH_STATS_MOMENT_WORDS;  // bytes of a node's moment words
static const int64_t kStatsMomentPiece = (int64_t)1 << 18;                  // nodes per piece of the moment scratch (16 MiB)

static bool stats_defined(const sph_solver* s, int slot) { return s->statsAcc[slot].p != nullptr; }
static int64_t stats_nodes(const sph_stats_lattice& g) { return (int64_t)g.dims[0] * g.dims[1] * g.dims[2]; }

// What every statistics call checks first: no slab solver (SPH_ERR_INVALID), and a slot in lo..SPH_MAX_STATS-1.
static int stats_check(sph_solver* s, int32_t slot, int lo, const char* what) {
  if (s->hasSlab) { sph_set_error("%s: a slab solver is not supported", what); return SPH_ERR_INVALID; }
  if (slot < lo || slot >= SPH_MAX_STATS) { sph_set_error("%s: slot %d is not in %d..%d", what, slot, lo, SPH_MAX_STATS - 1); return SPH_ERR_INVALID; }
  return SPH_OK;
}

static int stats_need_defined(const sph_solver* s, int32_t slot, const char* what) {
  if (stats_defined(s, slot)) return SPH_OK;
  sph_set_error("%s: slot %d is not defined (sph_stats_define)", what, slot);
  return SPH_ERR_ORDER;
}

static void stats_release(sph_solver* s, int slot) {
  SphScratch& b = s->statsAcc[slot];
  if (b.p) { hipStreamSynchronize(s->stream); hipFree(b.p); }
  b.p = nullptr; b.bytes = 0;
  s->statsLattice[slot] = sph_stats_lattice{};
  s->statsCalls[slot] = 0;
}

// the window firstNode .. firstNode + count - 1 of a defined slot, and the caller's pointer
static int stats_window(const sph_solver* s, int32_t slot, int64_t firstNode, int64_t count, const void* out, const char* what) {
  const int64_t nodes = stats_nodes(s->statsLattice[slot]);
  if (firstNode < 0 || count < 0 || firstNode > nodes || count > nodes - firstNode) {
    sph_set_error("%s: nodes %lld .. %lld are not all in the lattice of %lld nodes", what, (long long)firstNode,
                  (long long)(firstNode + count - 1), (long long)nodes);
    return SPH_ERR_INVALID;
  }
  if (count > 0 && !out) { sph_set_error("%s: null pointer", what); return SPH_ERR_INVALID; }
  return SPH_OK;
}

extern "C" int sph_stats_define(sph_solver* s, int32_t slot, const sph_stats_lattice* g) {
  ENTER(s);
  const char* what = "sph_stats_define";
  int rc = stats_check(s, slot, 0, what);
  if (rc != SPH_OK) return rc;
  if (!g) { stats_release(s, slot); return SPH_OK; }
  for (int c = 0; c < 3; c++) {
    if (!std::isfinite(g->origin[c]) || !std::isfinite(g->spacing[c])) { sph_set_error("%s: a word of origin or spacing is not finite", what); return SPH_ERR_INVALID; }
    if (g->dims[c] <= 0) { sph_set_error("%s: dims <= 0", what); return SPH_ERR_INVALID; }
  }
  if (g->typeMask == 0u || (g->typeMask & ~0xEu)) { sph_set_error("%s: typeMask must be a non-empty set of bits 1..3", what); return SPH_ERR_INVALID; }
  // (the products cannot wrap: each partial product is tested against the cap before the next factor comes in)
  const int64_t capNodes = SPH_STATS_BYTES_MAX / (int64_t)kStatsNode;
  const int64_t plane = (int64_t)g->dims[0] * g->dims[1];
  if (plane > capNodes || plane * g->dims[2] > capNodes) {
    sph_set_error("%s: the accumulators of %d x %d x %d nodes exceed %lld bytes", what, g->dims[0], g->dims[1], g->dims[2],
                  (long long)SPH_STATS_BYTES_MAX);
    return SPH_ERR_INVALID;
  }
  const int64_t nodes = plane * g->dims[2];
  // a buffer of exactly this lattice's size: the old one goes once the stream has finished with it
  void* fresh = nullptr;
  SPH_HIP(hipMalloc(&fresh, (size_t)nodes * kStatsNode));
  rc = sphk_stats_init(s, (double*)fresh, nodes);
  if (rc != SPH_OK) { hipFree(fresh); return rc; }
  stats_release(s, slot);
  s->statsAcc[slot].p = fresh;
  s->statsAcc[slot].bytes = (size_t)nodes * kStatsNode;
  s->statsLattice[slot] = *g;
  return SPH_OK;
}

extern "C" int sph_stats_get(sph_solver* s, int32_t slot, sph_stats_lattice* out, int32_t* defined, int64_t* calls) {
  ENTER(s);
  const int rc = stats_check(s, slot, 0, "sph_stats_get");
  if (rc != SPH_OK) return rc;
  const bool has = stats_defined(s, slot);
  if (defined) *defined = has ? 1 : 0;
  if (out && has) *out = s->statsLattice[slot];
  if (calls) *calls = s->statsCalls[slot];
  return SPH_OK;
}

extern "C" int sph_stats_accumulate(sph_solver* s, int32_t slot) {
  ENTER(s);
  const char* what = "sph_stats_accumulate";
  int rc = stats_check(s, slot, -1, what);
  if (rc != SPH_OK) return rc;
  const int first = slot < 0 ? 0 : slot, last = slot < 0 ? SPH_MAX_STATS - 1 : slot;
  // every slot of the call is checked before the first launch: a failed call changes no slot
  SampleArgs a[SPH_MAX_STATS];
  bool any = false;
  for (int q = first; q <= last; q++) {
    if (!stats_defined(s, q)) continue;
    any = true;
    rc = sph_sample_check(s, s->statsLattice[q].typeMask, what, &a[q]);
    if (rc != SPH_OK) return rc;
  }
  if (!any) {
    if (slot < 0) { sph_set_error("%s: no slot is defined (sph_stats_define)", what); return SPH_ERR_ORDER; }
    return stats_need_defined(s, slot, what);
  }
  for (int q = first; q <= last; q++) {
    if (!stats_defined(s, q)) continue;
    rc = sphk_stats_accumulate(s, a[q], s->statsLattice[q], s->statsCalls[q], (double*)s->statsAcc[q].p);
    if (rc != SPH_OK) return rc;
    s->statsCalls[q]++;
  }
  return SPH_OK;
}

extern "C" int sph_stats_reset(sph_solver* s, int32_t slot) {
  ENTER(s);
  const char* what = "sph_stats_reset";
  int rc = stats_check(s, slot, -1, what);
  if (rc != SPH_OK) return rc;
  if (slot >= 0) { rc = stats_need_defined(s, slot, what); if (rc != SPH_OK) return rc; }
  for (int q = slot < 0 ? 0 : slot; q <= (slot < 0 ? SPH_MAX_STATS - 1 : slot); q++) {
    if (!stats_defined(s, q)) continue;
    rc = sphk_stats_init(s, (double*)s->statsAcc[q].p, stats_nodes(s->statsLattice[q]));
    if (rc != SPH_OK) return rc;
    s->statsCalls[q] = 0;
  }
  return SPH_OK;
}

extern "C" int sph_stats_read(sph_solver* s, int32_t slot, int64_t firstNode, int64_t count, double* out, int64_t* calls) {
  ENTER(s);
  const char* what = "sph_stats_read";
  int rc = stats_check(s, slot, 0, what);
  if (rc != SPH_OK) return rc;
  rc = stats_need_defined(s, slot, what);
  if (rc != SPH_OK) return rc;
  if (calls) *calls = s->statsCalls[slot];
  rc = stats_window(s, slot, firstNode, count, out, what);
  if (rc != SPH_OK || count == 0) return rc;
  return sph_d2h(s, out, (const char*)s->statsAcc[slot].p + (size_t)firstNode * kStatsNode, (size_t)count * kStatsNode);
}

extern "C" int sph_stats_read_moments(sph_solver* s, int32_t slot, int64_t firstNode, int64_t count, float* out, int64_t* calls) {
  ENTER(s);
  const char* what = "sph_stats_read_moments";
  int rc = stats_check(s, slot, 0, what);
  if (rc != SPH_OK) return rc;
  rc = stats_need_defined(s, slot, what);
  if (rc != SPH_OK) return rc;
  if (calls) *calls = s->statsCalls[slot];
  rc = stats_window(s, slot, firstNode, count, out, what);
  if (rc != SPH_OK) return rc;
  if (s->statsCalls[slot] == 0) { sph_set_error("%s: slot %d has no call yet (sph_stats_accumulate)", what, slot); return SPH_ERR_ORDER; }
  if (count == 0) return SPH_OK;
  const int64_t piece = std::min(count, kStatsMomentPiece);
  rc = sph_grow_scratch(s, s->statsOut, (size_t)piece * kStatsMoment);
  if (rc != SPH_OK) return rc;
  const double* acc = (const double*)s->statsAcc[slot].p;
  for (int64_t done = 0; done < count; done += piece) {
    const int64_t n = std::min(piece, count - done);
    rc = sphk_stats_moments(s, acc + (size_t)(firstNode + done) * SPH_STATS_WORDS, n, s->statsCalls[slot], (float*)s->statsOut.p);
    if (rc != SPH_OK) return rc;
    rc = sph_d2h(s, out + (size_t)done * SPH_STATS_MOMENT_WORDS, s->statsOut.p, (size_t)n * kStatsMoment);
    if (rc != SPH_OK) return rc;
  }
  return SPH_OK;
}

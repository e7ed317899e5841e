// C ABI of libsphmi.so (include/sphmi.h), the flow gauges: sph_gauge_define / sph_gauge_get / sph_gauges_accumulate /
// sph_gauges_read / sph_gauges_reset / sph_gauges_history / sph_gauges_read_history / sph_gauge_crossings /
// sph_read_gauge_crossings. A gauge is passive: no call here says sph_state_changes or touches `progress`, and
// every buffer is the feature's own, so the analysis state and everything derived from it stay valid. What the translation units
// of the ABI share is in sph_api_internal.h.
#include <algorithm>
#include <cmath>
#include <vector>

#include "sph_api_internal.h"

// What every gauge call checks first: no slab solver (SPH_ERR_INVALID).
static int gauge_check(sph_solver* s, const char* what) {
  if (s->hasSlab) { sph_set_error("%s: a slab solver is not supported", what); return SPH_ERR_INVALID; }
  return SPH_OK;
}
static int gauge_slot_check(sph_solver* s, int32_t slot, const char* what) {
  const int rc = gauge_check(s, what);
  if (rc != SPH_OK) return rc;
  if (slot < 0 || slot >= SPH_MAX_GAUGES) { sph_set_error("%s: slot %d is not in 0..%d", what, slot, SPH_MAX_GAUGES - 1); return SPH_ERR_INVALID; }
  return SPH_OK;
}

// the order rules of the two calls that read a completed step
static int gauge_order(sph_solver* s, const char* what) {
  NEED(s, P_INTEGRATE, what);  // (an edit clears `progress`: removed and added particles are not crossings)
  if (s->stepOpen) {
    sph_set_error("%s: a stage-by-stage step is half done; positions are final after its integrate stage, with elastic matter after "
                  "its membranes-finalize stage", what);
    return SPH_ERR_ORDER;
  }
  return SPH_OK;
}

// the contract's derived doubles, one operation at a time (no contraction: the Makefile's flags); false: nn is 0 or not finite
static void gauge_cross(const double* a, const double* b, double* out) {
  out[0] = a[1] * b[2] - a[2] * b[1];
  out[1] = a[2] * b[0] - a[0] * b[2];
  out[2] = a[0] * b[1] - a[1] * b[0];
}
static bool gauge_derive(const sph_gauge& g, GaugeOne* out) {
  double u[3], v[3], vn[3], nu[3];
  for (int c = 0; c < 3; c++) { out->o[c] = (double)g.origin[c]; u[c] = (double)g.u[c]; v[c] = (double)g.v[c]; }
  double* n = out->n;
  gauge_cross(u, v, n);
  const double nn = (n[0] * n[0] + n[1] * n[1]) + n[2] * n[2];
  if (!(nn > 0.0) || !std::isfinite(nn)) return false;
  gauge_cross(v, n, vn);
  gauge_cross(n, u, nu);
  for (int c = 0; c < 3; c++) { out->A[c] = vn[c] / nn; out->B[c] = nu[c] / nn; }
  out->field = nullptr;
  out->typeMask = g.typeMask;
  out->plane = (g.flags & SPH_GAUGE_PLANE) ? 1u : 0u;
  return true;
}

// the gauge of a live slot as the kernels take it; SPH_ERR_ORDER if its carried field is gone
static int gauge_one(sph_solver* s, int32_t slot, const char* what, GaugeOne* out) {
  const sph_gauge& g = s->gaugeDef[slot];
  gauge_derive(g, out);  // (a live definition has passed it)
  if (g.fieldSlot >= 0) {
    if (!s->fieldLive[g.fieldSlot]) {
      sph_set_error("%s: carried field %d of gauge %d has been released (sph_gauge_define)", what, g.fieldSlot, slot);
      return SPH_ERR_ORDER;
    }
    out->field = (const float*)s->fieldSlot[g.fieldSlot].p;
  }
  return SPH_OK;
}

static int gauge_dev(sph_solver* s, GaugeDev** D) {
  const bool fresh = !s->gaugeBuf.p;
  int rc = sph_grow_scratch(s, s->gaugeBuf, sizeof(GaugeDev));
  if (rc != SPH_OK) return rc;
  *D = (GaugeDev*)s->gaugeBuf.p;
  if (fresh) {
    SPH_HIP(hipMemsetAsync(*D, 0, sizeof(GaugeDev), s->stream));
    rc = sphk_gauge_clear(s, *D, 0xffffu);
  }
  return rc;
}

extern "C" int sph_gauge_define(sph_solver* s, int32_t slot, const sph_gauge* g) {
  ENTER(s);
  const char* what = "sph_gauge_define";
  int rc = gauge_slot_check(s, slot, what);
  if (rc != SPH_OK) return rc;
  if (g) {
    for (int c = 0; c < 3; c++)
      if (!std::isfinite(g->origin[c]) || !std::isfinite(g->u[c]) || !std::isfinite(g->v[c])) {
        sph_set_error("%s: a word of origin, u or v is not finite", what);
        return SPH_ERR_INVALID;
      }
    GaugeOne one;
    if (!gauge_derive(*g, &one)) { sph_set_error("%s: u x v is zero or not finite: u and v span no plane", what); return SPH_ERR_INVALID; }
    if (g->typeMask == 0u || (g->typeMask & ~0x6u)) { sph_set_error("%s: typeMask 0x%x is empty or has a bit outside 1..2", what, g->typeMask); return SPH_ERR_INVALID; }
    if (g->fieldSlot != -1 && (g->fieldSlot < 0 || g->fieldSlot >= SPH_FIELD_SLOTS || !s->fieldLive[g->fieldSlot])) {
      sph_set_error("%s: fieldSlot %d is neither -1 nor an existing carried field", what, g->fieldSlot);
      return SPH_ERR_INVALID;
    }
    if (g->flags & ~SPH_GAUGE_PLANE) { sph_set_error("%s: flags 0x%x has unknown bits", what, g->flags); return SPH_ERR_INVALID; }
  } else if (!s->gaugeLive[slot]) {
    return SPH_OK;  // releasing a free slot: a no-op
  }
  GaugeDev* D = nullptr;
  rc = gauge_dev(s, &D);
  if (rc != SPH_OK) return rc;
  rc = sphk_gauge_clear(s, D, 1u << slot);  // on the solver's stream, behind every accumulate enqueued so far
  if (rc != SPH_OK) return rc;
  s->gaugeLive[slot] = g != nullptr;
  if (g) s->gaugeDef[slot] = *g;
  return SPH_OK;
}

extern "C" int sph_gauge_get(sph_solver* s, int32_t slot, sph_gauge* out, int32_t* defined) {
  ENTER(s);
  const int rc = gauge_slot_check(s, slot, "sph_gauge_get");
  if (rc != SPH_OK) return rc;
  if (!defined) { sph_set_error("sph_gauge_get: null pointer"); return SPH_ERR_INVALID; }
  *defined = s->gaugeLive[slot] ? 1 : 0;
  if (s->gaugeLive[slot] && out) *out = s->gaugeDef[slot];
  return SPH_OK;
}

extern "C" int sph_gauges_accumulate(sph_solver* s, double* out) {
  ENTER(s);
  const char* what = "sph_gauges_accumulate";
  int rc = gauge_check(s, what);
  if (rc != SPH_OK) return rc;
  rc = gauge_order(s, what);
  if (rc != SPH_OK) return rc;
  GaugeSet set = {};
  for (int32_t g = 0; g < SPH_MAX_GAUGES; g++) {
    if (!s->gaugeLive[g]) continue;
    rc = gauge_one(s, g, what, &set.g[g]);
    if (rc != SPH_OK) return rc;
    set.defMask |= 1u << g;
  }
  if (!set.defMask) { sph_set_error("%s: no gauge is defined (sph_gauge_define)", what); return SPH_ERR_ORDER; }
  GaugeDev* D = nullptr;
  rc = gauge_dev(s, &D);
  if (rc != SPH_OK) return rc;
  rc = sph_grow_scratch(s, s->gaugeTree, sphk_gauge_tree_bytes(s->d.N));
  if (rc != SPH_OK) return rc;
  rc = sphk_gauges_accumulate(s, set, (double*)s->gaugeTree.p, D, (double*)s->gaugeHist.p, s->gaugeHistRows, s->gaugeCalls);
  if (rc != SPH_OK) return rc;
  s->gaugeCalls++;
  if (!out) return SPH_OK;
  return sph_d2h(s, out, D->record, sizeof(double) * SPH_MAX_GAUGES * SPH_GAUGE_WORDS);
}

extern "C" int sph_gauges_read(sph_solver* s, double* totals, int64_t* calls) {
  ENTER(s);
  int rc = gauge_check(s, "sph_gauges_read");
  if (rc != SPH_OK) return rc;
  if (!totals) { sph_set_error("sph_gauges_read: null pointer"); return SPH_ERR_INVALID; }
  GaugeDev* D = nullptr;
  rc = gauge_dev(s, &D);
  if (rc != SPH_OK) return rc;
  rc = sph_d2h(s, totals, D->totals, sizeof(double) * SPH_MAX_GAUGES * SPH_GAUGE_TOTAL_WORDS);
  if (rc == SPH_OK && calls) *calls = s->gaugeCalls;
  return rc;
}

extern "C" int sph_gauges_reset(sph_solver* s, int32_t slot) {
  ENTER(s);
  int rc = slot == -1 ? gauge_check(s, "sph_gauges_reset") : gauge_slot_check(s, slot, "sph_gauges_reset");
  if (rc != SPH_OK) return rc;
  GaugeDev* D = nullptr;
  rc = gauge_dev(s, &D);
  if (rc != SPH_OK) return rc;
  return sphk_gauge_clear(s, D, slot == -1 ? 0xffffu : 1u << slot);
}

extern "C" int sph_gauges_history(sph_solver* s, int32_t rows) {
  ENTER(s);
  const int rc = gauge_check(s, "sph_gauges_history");
  if (rc != SPH_OK) return rc;
  if (rows < 0 || rows > SPH_GAUGE_HISTORY_MAX) { sph_set_error("sph_gauges_history: rows %d is not in 0..%d", rows, SPH_GAUGE_HISTORY_MAX); return SPH_ERR_INVALID; }
  SphScratch& b = s->gaugeHist;
  if (b.p) {
    SPH_HIP(hipStreamSynchronize(s->stream));
    hipFree(b.p);
    b.p = nullptr; b.bytes = 0;
  }
  s->gaugeHistRows = 0;
  s->gaugeHistFirst = s->gaugeCalls;
  if (rows == 0) return SPH_OK;
  const int rcGrow = sph_grow_scratch(s, b, sizeof(double) * SPH_MAX_GAUGES * SPH_GAUGE_WORDS * (size_t)rows);
  if (rcGrow != SPH_OK) return rcGrow;
  s->gaugeHistRows = rows;
  return SPH_OK;
}

extern "C" int sph_gauges_read_history(sph_solver* s, int64_t firstCall, int32_t count, double* out, int64_t* callsWritten) {
  ENTER(s);
  const char* what = "sph_gauges_read_history";
  int rc = gauge_check(s, what);
  if (rc != SPH_OK) return rc;
  if (callsWritten) *callsWritten = s->gaugeCalls;
  if (!s->gaugeHistRows) { sph_set_error("%s: there is no history (sph_gauges_history)", what); return SPH_ERR_ORDER; }
  if (count < 0 || (count > 0 && !out)) { sph_set_error("%s: bad count or null pointer", what); return SPH_ERR_INVALID; }
  if (count == 0) return SPH_OK;
  const int64_t rows = s->gaugeHistRows, end = s->gaugeCalls;
  const int64_t oldest = std::max(s->gaugeHistFirst, end - rows);
  if (firstCall < oldest || firstCall > end - count) {
    sph_set_error("%s: calls %lld .. %lld are not all in the ring, which holds %lld .. %lld", what, (long long)firstCall,
                  (long long)(firstCall + count - 1), (long long)oldest, (long long)(end - 1));
    return SPH_ERR_INVALID;
  }
  const size_t row = (size_t)SPH_MAX_GAUGES * SPH_GAUGE_WORDS;
  const double* ring = (const double*)s->gaugeHist.p;
  // at most two runs: up to the ring's end, then from its start
  const int64_t r0 = firstCall % rows;
  const int64_t n0 = std::min<int64_t>(count, rows - r0);
  rc = sph_d2h(s, out, ring + (size_t)r0 * row, sizeof(double) * row * (size_t)n0);
  if (rc != SPH_OK || n0 == count) return rc;
  return sph_d2h(s, out + (size_t)n0 * row, ring, sizeof(double) * row * (size_t)(count - n0));
}

// where the pieces of the crossing list lie in gaugeList (bytes from its start), for room for n crossings
struct GaugeListLayout { size_t index, origId, direction, tab, bytes; };
static GaugeListLayout gauge_list_layout(size_t n) {
  const size_t words = (n + 63) & ~(size_t)63;
  GaugeListLayout L;
  L.index = 0; L.origId = 4 * words; L.direction = 8 * words; L.tab = 12 * words; L.bytes = 24 * words;
  return L;
}

extern "C" int sph_gauge_crossings(sph_solver* s, int32_t slot, int64_t* count) {
  ENTER(s);
  const char* what = "sph_gauge_crossings";
  int rc = gauge_slot_check(s, slot, what);
  if (rc != SPH_OK) return rc;
  if (!count) { sph_set_error("%s: null pointer", what); return SPH_ERR_INVALID; }
  rc = gauge_order(s, what);
  if (rc != SPH_OK) return rc;
  if (!s->gaugeLive[slot]) { sph_set_error("%s: slot %d holds no gauge (sph_gauge_define)", what, slot); return SPH_ERR_ORDER; }
  GaugeOne one;
  rc = gauge_one(s, slot, what, &one);
  if (rc != SPH_OK) return rc;
  sph_derived_drop(s->gaugeCross);
  *count = 0;
  rc = sph_grow_scratch(s, s->gaugeScan, sphk_select_scratch_bytes(s->d.N));
  if (rc != SPH_OK) return rc;
  uint32_t* dTotals = nullptr;
  rc = sphk_gauge_mark(s, one, s->gaugeScan.p, &dTotals);
  if (rc != SPH_OK) return rc;
  uint32_t t[2] = {0, 0};
  rc = sph_d2h(s, t, dTotals, sizeof(t));  // the call's one wait
  if (rc != SPH_OK) return rc;
  if (t[0] > (uint32_t)std::max(s->d.N, 0)) { sph_set_error("%s: the crossing count %u exceeds N", what, t[0]); return SPH_ERR_HIP; }
  const GaugeListLayout L = gauge_list_layout(t[0]);
  if (t[0]) {
    rc = sph_grow_scratch(s, s->gaugeList, L.bytes);
    if (rc != SPH_OK) return rc;
    char* base = (char*)s->gaugeList.p;
    rc = sphk_select_scatter(s, s->gaugeScan.p, t[0], (int32_t*)(base + L.index));
    if (rc != SPH_OK) return rc;
    rc = sphk_gauge_list(s, one, (const int32_t*)(base + L.index), (int)t[0], (uint32_t*)(base + L.origId), (int32_t*)(base + L.direction),
                         (float*)(base + L.tab));
    if (rc != SPH_OK) return rc;
  }
  s->gaugeCrossCount = t[0];
  sph_derived_stamp(s, s->gaugeCross);
  *count = t[0];
  return SPH_OK;
}

extern "C" int sph_read_gauge_crossings(sph_solver* s, int32_t* sortedIndex, uint32_t* origId, int32_t* direction, float* tab3) {
  ENTER(s);
  const char* what = "sph_read_gauge_crossings";
  int rc = gauge_check(s, what);
  if (rc != SPH_OK) return rc;
  rc = sph_derived_check(s, s->gaugeCross, what, "there is no crossing list (sph_gauge_crossings)",
                         "the state has changed since sph_gauge_crossings");
  if (rc != SPH_OK) return rc;
  const size_t n = (size_t)s->gaugeCrossCount;
  if (!n) return SPH_OK;
  const GaugeListLayout L = gauge_list_layout(n);
  const char* base = (const char*)s->gaugeList.p;
  if (sortedIndex) { rc = sph_d2h(s, sortedIndex, base + L.index, sizeof(int32_t) * n); if (rc != SPH_OK) return rc; }
  if (origId) { rc = sph_d2h(s, origId, base + L.origId, sizeof(uint32_t) * n); if (rc != SPH_OK) return rc; }
  if (direction) { rc = sph_d2h(s, direction, base + L.direction, sizeof(int32_t) * n); if (rc != SPH_OK) return rc; }
  if (tab3) { rc = sph_d2h(s, tab3, base + L.tab, sizeof(float) * 3 * n); if (rc != SPH_OK) return rc; }
  return SPH_OK;
}

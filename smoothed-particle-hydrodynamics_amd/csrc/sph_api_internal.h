// What the translation units of the C ABI share (sph_api.hip: errors, timing, solver lifetime, stages, the fused step; sph_api_read.hip:
// read-back and reference-layout export; sph_api_slab.hip: the slab protocol; sph_api_analysis.hip: sampling, surfaces, gradients,
// diagnostics, components, selection, integral curves, rendering; sph_api_edit.hip: particle editing; sph_api_fields.hip: carried fields; sph_api_body.hip: kinematic bodies; sph_api_gauge.hip: flow gauges; sph_api_probe.hip: probes; sph_api_stats.hip: time statistics on a lattice): the order contract and the entry checks,
// the one rule for "the state has changed" and for results derived from it, and the per-particle input checks of sph_create
// and the adding calls.
#pragma once
#include <string.h>

#include <cmath>

#include "sph_common.h"

// stage progress bits for the order contract of simulationStep()
enum { P_HASH = 1, P_SORT = 2, P_SORTPOST = 4, P_INDEXX = 8, P_INDEXPOST = 16, P_FIND = 32, P_DENSITY = 64, P_FORCES = 128,
       P_PREDICTPOS = 256, P_PREDICTDENS = 512, P_PRESSUREFORCE = 1024,
       P_INTEGRATE = 2048 /* the step's integrate has run: acceleration and the boundary masks are what it read (sph_wall_*) */ };

#define NEED(s, bits, what)                                                              \
  do {                                                                                   \
    if (!(s)) { sph_set_error("null solver"); return SPH_ERR_INVALID; }                  \
    if (((s)->progress & (bits)) != (bits)) {                                            \
      sph_set_error("%s called before the stage(s) it depends on (simulationStep order, " \
                    "owPhysicsFluidSimulator.cpp:88-113)", what);                        \
      return SPH_ERR_ORDER;                                                              \
    }                                                                                    \
  } while (0)

// ---- the state and what is derived from it
// The sorted state or the particle set is about to change: every stage, step, slab call and edit says so here, and nowhere else.
static inline void sph_state_changes(sph_solver* s) { s->stateEpoch++; }
// r is current from now on / there is no r (a producer drops its result first, so a failed call leaves none behind)
static inline void sph_derived_stamp(const sph_solver* s, SphDerived& r) { r.valid = true; r.N = s->d.N; r.epoch = s->stateEpoch; }
static inline void sph_derived_drop(SphDerived& r) { r.valid = false; }
// SPH_ERR_ORDER with "<what>: <none>" unless r exists, and with "<what>: <stale>" unless it was made on the current state;
// stale == nullptr: r is self-contained by contract and only has to exist
static inline int sph_derived_check(const sph_solver* s, const SphDerived& r, const char* what, const char* none, const char* stale) {
  if (!r.valid) { sph_set_error("%s: %s", what, none); return SPH_ERR_ORDER; }
  if (stale && (r.epoch != s->stateEpoch || r.N != s->d.N)) { sph_set_error("%s: %s", what, stale); return SPH_ERR_ORDER; }
  return SPH_OK;
}

// ---- one particle of sph_create's or an adding call's input
// folded into the liquid signature (see sph_slab_liquid_signature): the common position.w bits of the non-boundary particles
// with velocity.w == +0; 0 = none seen yet, 0xffffffff = not uniform
static inline void sph_fold_liquid_signature(uint32_t& sig, const float* p4, const float* v4) {
  if ((int)p4[3] == SPH_BOUNDARY_PARTICLE || sig == 0xffffffffu) return;
  uint32_t tb, wb;
  memcpy(&tb, &p4[3], 4); memcpy(&wb, &v4[3], 4);
  if (wb != 0u || tb == 0u || tb == 0xffffffffu || (sig != 0u && sig != tb)) sig = 0xffffffffu;
  else sig = tb;
}
// nullptr if the position is finite and, with wide cell ids, inside the box; otherwise what is wrong with it, for the caller's message
static inline const char* sph_position_fault(const sph_config& c, const float* p4) {
  const float x = p4[0], y = p4[1], z = p4[2];
  if (!(std::isfinite(x) && std::isfinite(y) && std::isfinite(z))) return "not finite";
  const bool inside = x >= c.xmin && x <= c.xmax && y >= c.ymin && y <= c.ymax && z >= c.zmin && z <= c.zmax;
  return c.cellIdMask == 0xffffffffu && !inside ? "outside the box (wide cell ids need in-box input)" : nullptr;
}

// (bodies in sph_api.hip)
// The launches of one fused step on s->stream. tail (slab mode, the overlapped step of sph_slab_step_begin only): where the halo
// messages go, packed as soon as the owned layers next to the cuts are integrated.
struct StepTail {
  uint32_t *frameDown, *frameUp;
  int capRecords;
};
int enqueue_step(sph_solver* s, const StepTail* tail);
// (bodies in sph_api_read.hip)
int sph_d2h(sph_solver* s, void* dst, const void* src, size_t bytes);  // blocking copy to the host on s->stream
int sph_check_finite_state(sph_solver* s);                             // synchronises the stream; SPH_ERR_INVALID once the state has blown up
// (body in sph_api_slab.hip)
int sph_slab_finish(sph_solver* s, int32_t counts[4]);
// (bodies in sph_api_analysis.hip)
int sph_grow_scratch(sph_solver* s, SphScratch& b, size_t bytes);  // device buffer b grown to at least `bytes`
// The argument and order rules every analysis call shares (sph_sample_points' own); a != nullptr: the constants of the sampling
// contract too.
int sph_sample_check(sph_solver* s, uint32_t typeMask, const char* what, SampleArgs* a = nullptr);
// The selection arguments every call that takes them shares: typeMask must be a non-empty set of bits 1..3; region6 (x0, y0, z0,
// x1, y1, z1) may be null (everything: -inf .. +inf) and must not hold a NaN. SPH_ERR_INVALID with "<what>: ..." otherwise.
int sph_fill_selector(SphSelector* sel, const float* region6 /* may be null */, uint32_t typeMask, const char* what);
// SPH_ERR_ORDER unless a labelling / a selection exists and was made on the current state; *labels: the N labels (device)
int sph_labels_current(sph_solver* s, const char* what, const int32_t** labels);
int sph_selection_current(sph_solver* s, const char* what);

// (bodies in sph_api_fields.hip) What an edit does to the carried fields, enqueued on s->stream next to the edit's own work; with
// no slot in existence neither enqueues anything.
int sph_fields_follow_removal(sph_solver* s, int oldN, const int32_t* map);  // every slot through the removal's old-to-new map
int sph_fields_follow_add(sph_solver* s, int first, int count);              // ids first .. first + count get each slot's inflow
// (body in sph_api_body.hip) What a removal does to the kinematic bodies, next to the fields: member ids through the old-to-new map,
// removed members dropped with their reference rows, a body left empty released. Blocking per body in use (its new count).
int sph_bodies_follow_removal(sph_solver* s, int oldN, const int32_t* map);
// the dynamic bodies as the launches of sph_body_dynamics.hip take them (sph_api_body.hip: set_dynamics; sph_api_analysis.hip: advance)
static inline BodyDynSet sph_body_dyn_set(const sph_solver* s) {
  BodyDynSet set = {};
  for (int b = 0; b < SPH_MAX_BODIES; b++) {
    if (!s->bodyDynamic[b] || !s->bodyCount[b]) continue;
    set.dynMask |= 1u << b;
    set.count[b] = s->bodyCount[b];
    set.ids[b] = (const uint32_t*)s->bodyIds[b].p;
    set.ref[b] = (const float4*)s->bodyRef[b].p;
  }
  return set;
}
// the box a pose is validated against (sph_body_set_pose and the advance)
static inline BodyPose sph_body_pose_box(const sph_solver* s) {
  const sph_config& c = s->cfg;
  BodyPose a = {};
  a.wide = c.cellIdMask == 0xffffffffu;
  a.xmin = c.xmin; a.xmax = c.xmax; a.ymin = c.ymin; a.ymax = c.ymax; a.zmin = c.zmin; a.zmax = c.zmax;
  return a;
}

// (a rebuild whose particle count is still on its way to the host — sph_slab_rebuild_framed — is finished first)
#define ENTER_RAW(s) do { if (!(s)) { sph_set_error("null solver"); return SPH_ERR_INVALID; } SPH_HIP(hipSetDevice((s)->cfg.device)); } while (0)
#define ENTER(s) do { ENTER_RAW(s); if ((s)->slabRebuildPending) { const int rcf_ = sph_slab_finish((s), nullptr); if (rcf_ != SPH_OK) return rcf_; } } while (0)

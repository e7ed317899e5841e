// C ABI of libsphmi.so (include/sphmi.h), the kinematic bodies: sph_body_define_ids / sph_body_define_region / sph_body_release /
// sph_body_count / sph_body_read / sph_body_set_pose, the dynamic state of a free body (sph_body_set_dynamics / sph_body_get_dynamics,
// DESIGN.md §37), and what a removal does to the bodies (sph_bodies_follow_removal). A pose
// rewrites rows of posOrig / velOrig but not the particle set: no call here says sph_state_changes or touches `progress`, so the
// analysis state and everything derived from it stay valid. What the translation units of the ABI share is in
// sph_api_internal.h.
#include <cmath>
#include <utility>
#include <vector>

#include "sph_api_internal.h"

// ---------------------------------------------------------------------------------------------- kinematic bodies
// What every body call checks first: no slab solver, a slot number in range (SPH_ERR_INVALID), no stage-by-stage step half done
// (SPH_ERR_ORDER: posOrig / velOrig are the solver's state only between two steps).
static int body_check(sph_solver* s, int32_t slot, const char* what) {
  if (s->hasSlab) { sph_set_error("%s: a slab solver is not supported", what); return SPH_ERR_INVALID; }
  if (slot < 0 || slot >= SPH_MAX_BODIES) { sph_set_error("%s: slot %d is not in 0..%d", what, slot, SPH_MAX_BODIES - 1); return SPH_ERR_INVALID; }
  if (s->stepOpen) {
    sph_set_error("%s: a stage-by-stage step is half done; bodies are defined and moved between two steps", what);
    return SPH_ERR_ORDER;
  }
  return SPH_OK;
}

static int body_grow_stage(sph_solver* s, int count) {
  const int rc = sph_grow_scratch(s, s->bodyStageIds, sizeof(uint32_t) * (size_t)count);
  return rc != SPH_OK ? rc : sph_grow_scratch(s, s->bodyStageRef, 2 * sizeof(float4) * (size_t)count);
}

static void body_swap(SphScratch& a, SphScratch& b) { std::swap(a.p, b.p); std::swap(a.bytes, b.bytes); }

// the stage pair holds the new body of `count` members: it is the slot's from now on, and the slot's old buffers stage the next one
static void body_install(sph_solver* s, int32_t slot, int count) {
  body_swap(s->bodyIds[slot], s->bodyStageIds);
  body_swap(s->bodyRef[slot], s->bodyStageRef);
  s->bodyCount[slot] = count;
}

// (the stream has been drained by the caller)
static void body_drop(sph_solver* s, int32_t slot) {
  for (SphScratch* b : {&s->bodyIds[slot], &s->bodyRef[slot]}) {
    if (b->p) hipFree(b->p);
    b->p = nullptr; b->bytes = 0;
  }
  s->bodyCount[slot] = 0;
  s->bodyDynamic[slot] = false;  // a body that is gone has no dynamics
}

extern "C" int sph_body_define_ids(sph_solver* s, int32_t slot, const uint32_t* origIds, int64_t count) {
  ENTER(s);
  int rc = body_check(s, slot, "sph_body_define_ids");
  if (rc != SPH_OK) return rc;
  if (!origIds) { sph_set_error("sph_body_define_ids: null pointer"); return SPH_ERR_INVALID; }
  if (count <= 0) { sph_set_error("sph_body_define_ids: a body has at least one member (count %lld)", (long long)count); return SPH_ERR_INVALID; }
  if (count > s->d.N) {
    sph_set_error("sph_body_define_ids: %lld entries exceed the particle count %d, so some id is out of range or listed twice", (long long)count, s->d.N);
    return SPH_ERR_INVALID;
  }
  const int n = (int)count;
  rc = body_grow_stage(s, n);
  if (rc != SPH_OK) return rc;
  rc = sph_grow_scratch(s, s->bodyBuf, sphk_body_check_bytes(s->d.N));
  if (rc != SPH_OK) return rc;
  uint32_t* ids = (uint32_t*)s->bodyStageIds.p;
  SPH_HIP(hipMemcpyAsync(ids, origIds, sizeof(uint32_t) * (size_t)n, hipMemcpyHostToDevice, s->stream));
  uint32_t* dCounters = nullptr;
  rc = sphk_body_check_ids(s, ids, n, s->bodyBuf.p, &dCounters);
  if (rc != SPH_OK) return rc;
  uint32_t bad[2] = {0, 0};
  rc = sph_d2h(s, bad, dCounters, sizeof(bad));  // the call's one wait (the host array is pageable: its copy has landed too)
  if (rc != SPH_OK) return rc;
  if (bad[0]) {
    sph_set_error("sph_body_define_ids: %u of %d entries are not below the particle count %d, are not boundary particles or are listed "
                  "more than once; the lowest is entry %u", bad[0], n, s->d.N, bad[1]);
    return SPH_ERR_INVALID;
  }
  rc = sphk_body_gather(s, ids, n, (float4*)s->bodyStageRef.p);
  if (rc != SPH_OK) return rc;
  body_install(s, slot, n);
  s->bodyDynamic[slot] = false;  // a new definition is kinematic
  return SPH_OK;
}

extern "C" int sph_body_define_region(sph_solver* s, int32_t slot, const float* region6, int64_t* count) {
  ENTER(s);
  int rc = body_check(s, slot, "sph_body_define_region");
  if (rc != SPH_OK) return rc;
  if (!count) { sph_set_error("sph_body_define_region: null pointer"); return SPH_ERR_INVALID; }
  SphSelector a = {};
  rc = sph_fill_selector(&a, region6, 1u << SPH_BOUNDARY_PARTICLE, "sph_body_define_region");
  if (rc != SPH_OK) return rc;
  // sph_remove_region's marks in the edit scratch; the members are the MARKED particles, listed by the selection's scan and scatter
  rc = sph_grow_scratch(s, s->editBuf, sphk_edit_scratch_bytes(s->d.N));
  if (rc != SPH_OK) return rc;
  rc = sphk_edit_mark_region(s, a, s->editBuf.p);
  if (rc != SPH_OK) return rc;
  uint32_t* dTotals = nullptr;
  rc = sphk_body_count_marks(s, s->editBuf.p, &dTotals);
  if (rc != SPH_OK) return rc;
  uint32_t t[2] = {0, 0};
  rc = sph_d2h(s, t, dTotals, sizeof(t));  // the call's one wait
  if (rc != SPH_OK) return rc;
  if (t[0] > (uint32_t)s->d.N) { sph_set_error("sph_body_define_region: the member count %u exceeds N", t[0]); return SPH_ERR_HIP; }
  *count = 0;
  if (t[0] == 0) { sph_set_error("sph_body_define_region: the region holds no boundary particle"); return SPH_ERR_INVALID; }
  const int n = (int)t[0];
  rc = body_grow_stage(s, n);
  if (rc != SPH_OK) return rc;
  rc = sphk_select_scatter(s, s->editBuf.p, t[0], (int32_t*)s->bodyStageIds.p);  // ascending original id
  if (rc != SPH_OK) return rc;
  rc = sphk_body_gather(s, (const uint32_t*)s->bodyStageIds.p, n, (float4*)s->bodyStageRef.p);
  if (rc != SPH_OK) return rc;
  body_install(s, slot, n);
  s->bodyDynamic[slot] = false;  // a new definition is kinematic
  *count = n;
  return SPH_OK;
}

extern "C" int sph_body_release(sph_solver* s, int32_t slot) {
  ENTER(s);
  const int rc = body_check(s, slot, "sph_body_release");
  if (rc != SPH_OK) return rc;
  if (!s->bodyCount[slot]) return SPH_OK;
  SPH_HIP(hipStreamSynchronize(s->stream));
  body_drop(s, slot);
  return SPH_OK;
}

extern "C" int sph_body_count(sph_solver* s, int32_t slot, int64_t* count) {
  ENTER(s);
  const int rc = body_check(s, slot, "sph_body_count");
  if (rc != SPH_OK) return rc;
  if (!count) { sph_set_error("sph_body_count: null pointer"); return SPH_ERR_INVALID; }
  *count = s->bodyCount[slot];
  return SPH_OK;
}

extern "C" int sph_body_read(sph_solver* s, int32_t slot, uint32_t* origIds, float* refPosition4, float* refNormal4) {
  ENTER(s);
  int rc = body_check(s, slot, "sph_body_read");
  if (rc != SPH_OK) return rc;
  const size_t n = (size_t)s->bodyCount[slot];
  if (!n) return SPH_OK;
  if (origIds) {
    rc = sph_d2h(s, origIds, s->bodyIds[slot].p, sizeof(uint32_t) * n);
    if (rc != SPH_OK) return rc;
  }
  if (!refPosition4 && !refNormal4) return SPH_OK;
  std::vector<float> rows(8 * n);  // position, normal, position, ...
  rc = sph_d2h(s, rows.data(), s->bodyRef[slot].p, sizeof(float) * rows.size());
  if (rc != SPH_OK) return rc;
  for (size_t k = 0; k < n; k++)
    for (int c = 0; c < 4; c++) {
      if (refPosition4) refPosition4[4 * k + c] = rows[8 * k + c];
      if (refNormal4) refNormal4[4 * k + c] = rows[8 * k + 4 + c];
    }
  return SPH_OK;
}

extern "C" int sph_body_set_pose(sph_solver* s, int32_t slot, const float pose[12], int64_t* offenders, int64_t* lowestMember,
                                 float* maxMoveInR0) {
  ENTER(s);
  int rc = body_check(s, slot, "sph_body_set_pose");
  if (rc != SPH_OK) return rc;
  if (!pose) { sph_set_error("sph_body_set_pose: null pointer"); return SPH_ERR_INVALID; }
  BodyPose a = sph_body_pose_box(s);
  for (int k = 0; k < 12; k++) {
    if (!std::isfinite(pose[k])) { sph_set_error("sph_body_set_pose: pose word %d (%g) is not finite", k, pose[k]); return SPH_ERR_INVALID; }
    a.m[k] = pose[k];
  }
  const int n = s->bodyCount[slot];
  if (!n) { sph_set_error("sph_body_set_pose: slot %d holds no body (sph_body_define_ids / sph_body_define_region)", slot); return SPH_ERR_ORDER; }
  rc = sph_grow_scratch(s, s->bodyBuf, sphk_body_check_bytes(0));  // the counters
  if (rc != SPH_OK) return rc;
  const uint32_t* ids = (const uint32_t*)s->bodyIds[slot].p;
  const float4* ref = (const float4*)s->bodyRef[slot].p;
  uint32_t* dCounters = (uint32_t*)s->bodyBuf.p;
  rc = sphk_body_pose_validate(s, a, ids, ref, n, dCounters);
  if (rc != SPH_OK) return rc;
  uint32_t t[3] = {0, 0, 0};
  rc = sph_d2h(s, t, dCounters, sizeof(t));  // the call's one wait
  if (rc != SPH_OK) return rc;
  if (offenders) *offenders = t[0];
  if (lowestMember) *lowestMember = t[0] ? (int64_t)t[1] : -1;
  if (t[0]) {
    sph_set_error("sph_body_set_pose: %u of %d members would be placed at a position that is not finite%s; the lowest is member %u; "
                  "nothing was moved", t[0], n, a.wide ? " or lies outside the box (wide cell ids need in-box positions)" : "", t[1]);
    return SPH_ERR_INVALID;
  }
  rc = sph_guard_position_write(s);  // an asynchronous read-back of posOrig finishes its device copy first
  if (rc != SPH_OK) return rc;
  rc = sphk_body_pose_commit(s, a, ids, ref, n);  // on the solver's stream: everything that reads the state is ordered behind it
  if (rc != SPH_OK) return rc;
  if (maxMoveInR0) {
    float d2;
    memcpy(&d2, &t[2], sizeof(d2));
    *maxMoveInR0 = sqrtf(d2) / s->d.r0;
  }
  return SPH_OK;
}

// ---------------------------------------------------------------------------------------------- free bodies: the dynamic state
// (sph_bodies_advance is in sph_api_analysis.hip, next to the wall loads whose order rules it shares)
static bool dyn_finite(const double* v, int n) {
  for (int k = 0; k < n; k++)
    if (!std::isfinite(v[k])) return false;
  return true;
}

extern "C" int sph_body_set_dynamics(sph_solver* s, int32_t slot, const sph_body_dynamics* dyn) {
  ENTER(s);
  const char* what = "sph_body_set_dynamics";
  int rc = body_check(s, slot, what);
  if (rc != SPH_OK) return rc;
  if (!s->bodyCount[slot]) { sph_set_error("%s: slot %d holds no body (sph_body_define_ids / sph_body_define_region)", what, slot); return SPH_ERR_ORDER; }
  if (!dyn) { s->bodyDynamic[slot] = false; return SPH_OK; }
  sph_body_dynamics p = *dyn;
  const bool finite = std::isfinite(p.mass) && dyn_finite(p.com, 3) && dyn_finite(p.inertiaInv, 6) && dyn_finite(p.position, 3) &&
                      dyn_finite(p.orientation, 4) && dyn_finite(p.velocity, 3) && dyn_finite(p.angularMomentum, 3) &&
                      dyn_finite(p.spin, 3) && dyn_finite(p.gravity, 3) && dyn_finite(p.force, 3) && dyn_finite(p.torque, 3) &&
                      std::isfinite(p.contactGain) && std::isfinite(p.forceGain);
  if (!finite) { sph_set_error("%s: a parameter is not finite", what); return SPH_ERR_INVALID; }
  if (!(p.mass > 0.0)) { sph_set_error("%s: mass %g is not > 0", what, p.mass); return SPH_ERR_INVALID; }
  const double* J = p.inertiaInv;  // xx yy zz xy xz yz
  // positive semi-definite up to rounding (a pseudo-inverse of a singular inertia has minors that are zero but for it): no
  // diagonal word, 2 x 2 principal minor or determinant below -1e-9 of the size of its terms
  auto minor_bad = [](double a, double b, double c) { return a * b - c * c < -1e-9 * (a * b + c * c); };
  const double det = J[0] * (J[1] * J[2] - J[5] * J[5]) - J[3] * (J[3] * J[2] - J[5] * J[4]) + J[4] * (J[3] * J[5] - J[1] * J[4]);
  const double tr = J[0] + J[1] + J[2];
  if (J[0] < 0.0 || J[1] < 0.0 || J[2] < 0.0 || minor_bad(J[0], J[1], J[3]) || minor_bad(J[0], J[2], J[4]) || minor_bad(J[1], J[2], J[5]) ||
      det < -1e-9 * tr * tr * tr) {
    sph_set_error("%s: inertiaInv is not positive semi-definite", what);
    return SPH_ERR_INVALID;
  }
  if (p.locks & ~0xFu) { sph_set_error("%s: locks 0x%x has bits above 3", what, p.locks); return SPH_ERR_INVALID; }
  double* q = p.orientation;
  const double n = std::sqrt(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3]);
  if (!(n >= 0.5 && n <= 2.0)) { sph_set_error("%s: |orientation| = %g is not in [0.5, 2]", what, n); return SPH_ERR_INVALID; }
  for (int k = 0; k < 4; k++) q[k] = q[k] / n;
  rc = sph_grow_scratch(s, s->bodyDynBuf, sizeof(BodyDynDev));
  if (rc != SPH_OK) return rc;
  BodyDynDev* D = (BodyDynDev*)s->bodyDynBuf.p;
  // members shared with another dynamic body: counted on the device, the call's one wait
  BodyDynSet set = sph_body_dyn_set(s);
  set.dynMask &= ~(1u << slot);
  if (set.dynMask) {
    set.count[slot] = s->bodyCount[slot];
    set.ids[slot] = (const uint32_t*)s->bodyIds[slot].p;
    rc = sph_grow_scratch(s, s->bodyBuf, sphk_body_check_bytes(s->d.N));
    if (rc != SPH_OK) return rc;
    rc = sphk_bdyn_overlap(s, set, slot, (unsigned long long*)((char*)s->bodyBuf.p + 256), D);
    if (rc != SPH_OK) return rc;
    uint32_t shared[2] = {0, 0};
    rc = sph_d2h(s, shared, D->overlap, sizeof(shared));
    if (rc != SPH_OK) return rc;
    if (shared[0]) {
      sph_set_error("%s: %u of the %d members of slot %d are members of another dynamic body; the lowest shared id is %u", what,
                    shared[0], s->bodyCount[slot], slot, shared[1]);
      return SPH_ERR_INVALID;
    }
  }
  BodyDynSlot rec = {};
  rec.p = p;
  rc = hipMemcpyAsync(&D->live[slot], &rec, sizeof(rec), hipMemcpyHostToDevice, s->stream) == hipSuccess ? SPH_OK : SPH_ERR_HIP;
  if (rc == SPH_OK) rc = hipStreamSynchronize(s->stream) == hipSuccess ? SPH_OK : SPH_ERR_HIP;  // (rec is a local)
  if (rc != SPH_OK) { sph_set_error("%s: the copy of the state to the device failed", what); return rc; }
  s->bodyDynamic[slot] = true;
  return SPH_OK;
}

extern "C" int sph_body_get_dynamics(sph_solver* s, int32_t slot, sph_body_dynamics* out, int32_t* isDynamic) {
  ENTER(s);
  const int rc = body_check(s, slot, "sph_body_get_dynamics");
  if (rc != SPH_OK) return rc;
  if (!isDynamic) { sph_set_error("sph_body_get_dynamics: null pointer"); return SPH_ERR_INVALID; }
  *isDynamic = s->bodyDynamic[slot] ? 1 : 0;
  if (!s->bodyDynamic[slot] || !out) return SPH_OK;
  BodyDynSlot rec = {};
  const int rcCopy = sph_d2h(s, &rec, &((BodyDynDev*)s->bodyDynBuf.p)->live[slot], sizeof(rec));
  if (rcCopy != SPH_OK) return rcCopy;
  *out = rec.p;
  return SPH_OK;
}

// ---------------------------------------------------------------------------------------------- what a removal does to the bodies
int sph_bodies_follow_removal(sph_solver* s, int oldN, const int32_t* map) {
  for (int32_t slot = 0; slot < SPH_MAX_BODIES; slot++) {
    const int n = s->bodyCount[slot];
    if (!n) continue;
    int rc = body_grow_stage(s, n);
    if (rc != SPH_OK) return rc;
    rc = sph_grow_scratch(s, s->bodyBuf, sphk_body_compact_bytes(n));
    if (rc != SPH_OK) return rc;
    uint32_t* dTotals = nullptr;
    rc = sphk_body_compact(s, (const uint32_t*)s->bodyIds[slot].p, (const float4*)s->bodyRef[slot].p, n, map, oldN, s->bodyBuf.p,
                           (uint32_t*)s->bodyStageIds.p, (float4*)s->bodyStageRef.p, &dTotals);
    if (rc != SPH_OK) return rc;
    uint32_t kept = 0;
    rc = sph_d2h(s, &kept, dTotals, sizeof(kept));
    if (rc != SPH_OK) return rc;
    if (kept > (uint32_t)n) { sph_set_error("sph_bodies_follow_removal: body %d keeps %u of %d members", slot, kept, n); return SPH_ERR_HIP; }
    if (kept == 0) body_drop(s, slot);  // (the copy above has drained the stream)
    else body_install(s, slot, (int)kept);
  }
  return SPH_OK;
}

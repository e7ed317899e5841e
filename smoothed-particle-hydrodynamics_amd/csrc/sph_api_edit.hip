// C ABI of libsphmi.so (include/sphmi.h), the particle-editing calls: sph_remove_region / sph_remove_selection / sph_remove_ids /
// sph_add_particles / sph_emit_lattice / sph_read_edit_map. Unlike the analysis calls (sph_api_analysis.hip) they rewrite the
// solver's state; what the translation units of the ABI share is in sph_api_internal.h.
#include <string.h>

#include <algorithm>
#include <cmath>

#include "sph_api_internal.h"

// ---------------------------------------------------------------------------------------------- particle editing
// Adding and removing particles between steps (sph_edit.hip). The calls act on the current state in original-id
// order (posOrig, velOrig), not on the sorted state the analysis calls above read; one that changes the set invalidates that sorted
// state (progress = 0, sph_state_changes), which is what frees the sorted arrays to stage the compaction. Blocking, no stage timing.
static int edit_check(sph_solver* s, const char* what) {
  if (s->hasSlab) { sph_set_error("%s: a slab solver is not supported", what); return SPH_ERR_INVALID; }
  return SPH_OK;
}

// what every successful edit that changes the set does
static void edit_commit(sph_solver* s, int newN) {
  s->d.N = newN;
  sph_state_changes(s);
  s->progress = 0;
  s->stepOpen = false;  // (a stage-by-stage step the edit cut short is abandoned: the next stage has to be the hash)
}

// the id map of a removal of a set of N particles is current from now on (identity: nothing was marked, nothing moved)
static void edit_stamp_map(sph_solver* s, int N, bool identity) {
  sph_derived_stamp(s, s->map);
  s->mapIdentity = identity; s->mapLength = N;
}

// The marks are in editBuf: count them and, unless countOnly, compact the state. *removed receives the number of marked particles.
static int edit_remove_marked(sph_solver* s, const char* what, bool countOnly, int64_t* removed) {
  const SphDev& d = s->d;
  const int N = d.N;
  const int protectEnd = d.hasElastic ? d.elasticOffset + d.numElastic : 0;
  uint32_t* dTotals = nullptr;
  int rc = sphk_edit_count(s, protectEnd, s->editBuf.p, &dTotals);
  if (rc != SPH_OK) return rc;
  uint32_t t[3] = {0, 0, 0};
  rc = sph_d2h(s, t, dTotals, sizeof(t));  // the call's one wait for a result
  if (rc != SPH_OK) return rc;
  if (t[0] > (uint32_t)N) { sph_set_error("%s: the survivor count %u exceeds N", what, t[0]); return SPH_ERR_HIP; }
  const int kept = (int)t[0];
  if (countOnly) { *removed = N - kept; return SPH_OK; }
  if (kept == N) {  // nothing marked: the solver, its analysis state and its epoch stay as they are; the map is the identity
    *removed = 0;
    edit_stamp_map(s, N, true);
    return SPH_OK;
  }
  if (t[2] != 0xffffffffu) {
    sph_set_error("%s: particle %u lies below the end of the elastic range (%d): the connection, membrane and muscle tables address "
                  "original ids up to there, so those ids cannot shift", what, t[2], protectEnd);
    return SPH_ERR_INVALID;
  }
  if (kept == 0) { sph_set_error("%s: every particle is marked; a solver holds at least one particle", what); return SPH_ERR_INVALID; }
  rc = sph_guard_position_write(s);  // an asynchronous read-back of posOrig finishes its device copy first
  if (rc != SPH_OK) return rc;
  rc = sphk_edit_scatter(s, s->editBuf.p, (uint32_t)kept, s->d.sortedPos, s->d.sortedVel, (int32_t*)s->d.backIndex);
  if (rc != SPH_OK) return rc;
  // membDelta (orig-indexed): all zero again, as sph_create leaves it (the step clears it before it reads it anyway)
  if (s->d.membDelta) SPH_HIP(hipMemsetAsync(s->d.membDelta, 0, sizeof(float4) * (size_t)N, s->stream));
  rc = sph_fields_follow_removal(s, N, (const int32_t*)s->d.backIndex);  // the carried fields move with position and velocity
  if (rc != SPH_OK) return rc;
  rc = sph_bodies_follow_removal(s, N, (const int32_t*)s->d.backIndex);  // the kinematic bodies keep their surviving members
  if (rc != SPH_OK) return rc;
  SPH_HIP(hipStreamSynchronize(s->stream));
  std::swap(s->d.posOrig, s->d.sortedPos);
  std::swap(s->d.velOrig, s->d.sortedVel);
  edit_commit(s, kept);
  edit_stamp_map(s, N, false);
  *removed = N - kept;
  return SPH_OK;
}

extern "C" int sph_remove_region(sph_solver* s, const float* region6, uint32_t typeMask, int32_t countOnly, int64_t* removed) {
  ENTER(s);
  int rc = edit_check(s, "sph_remove_region");
  if (rc != SPH_OK) return rc;
  if (!removed) { sph_set_error("sph_remove_region: null pointer"); return SPH_ERR_INVALID; }
  SphSelector a = {};
  rc = sph_fill_selector(&a, region6, typeMask, "sph_remove_region");
  if (rc != SPH_OK) return rc;
  rc = sph_grow_scratch(s, s->editBuf, sphk_edit_scratch_bytes(s->d.N));
  if (rc != SPH_OK) return rc;
  rc = sphk_edit_mark_region(s, a, s->editBuf.p);
  if (rc != SPH_OK) return rc;
  return edit_remove_marked(s, "sph_remove_region", countOnly != 0, removed);
}

extern "C" int sph_remove_selection(sph_solver* s, int64_t* removed) {
  ENTER(s);
  int rc = edit_check(s, "sph_remove_selection");
  if (rc != SPH_OK) return rc;
  if (!removed) { sph_set_error("sph_remove_selection: null pointer"); return SPH_ERR_INVALID; }
  rc = sph_selection_current(s, "sph_remove_selection");
  if (rc != SPH_OK) return rc;
  rc = sph_grow_scratch(s, s->editBuf, sphk_edit_scratch_bytes(s->d.N));
  if (rc != SPH_OK) return rc;
  rc = sphk_edit_clear_marks(s, s->editBuf.p);
  if (rc != SPH_OK) return rc;
  rc = sphk_edit_mark_ids(s, nullptr, (const int32_t*)s->selList.p, (int)s->selCount, s->editBuf.p);
  if (rc != SPH_OK) return rc;
  return edit_remove_marked(s, "sph_remove_selection", false, removed);
}

extern "C" int sph_remove_ids(sph_solver* s, const uint32_t* origIds, int64_t count, int64_t* removed) {
  ENTER(s);
  int rc = edit_check(s, "sph_remove_ids");
  if (rc != SPH_OK) return rc;
  if (!removed || count < 0 || (count > 0 && !origIds)) { sph_set_error("sph_remove_ids: null pointer or negative count"); return SPH_ERR_INVALID; }
  for (int64_t r = 0; r < count; r++)
    if (origIds[r] >= (uint32_t)s->d.N) {
      sph_set_error("sph_remove_ids: id %u (entry %lld) is not below the particle count %d", origIds[r], (long long)r, s->d.N);
      return SPH_ERR_INVALID;
    }
  rc = sph_grow_scratch(s, s->editBuf, sphk_edit_scratch_bytes(s->d.N));
  if (rc != SPH_OK) return rc;
  rc = sphk_edit_clear_marks(s, s->editBuf.p);
  if (rc != SPH_OK) return rc;
  // the ids go through keysAlt (idle between a step's sort and the next one's) in pieces of at most `capacity` entries
  const int64_t piece = s->capacity;
  for (int64_t first = 0; first < count; first += piece) {
    const int n = (int)std::min<int64_t>(piece, count - first);
    SPH_HIP(hipMemcpyAsync(s->d.keysAlt, origIds + first, sizeof(uint32_t) * (size_t)n, hipMemcpyHostToDevice, s->stream));
    rc = sphk_edit_mark_ids(s, s->d.keysAlt, nullptr, n, s->editBuf.p);
    if (rc != SPH_OK) return rc;
    SPH_HIP(hipStreamSynchronize(s->stream));  // (the host array is pageable: the next piece must not overtake this copy)
  }
  return edit_remove_marked(s, "sph_remove_ids", false, removed);
}

extern "C" int sph_read_edit_map(sph_solver* s, int32_t* newIdOfOld) {
  ENTER(s);
  if (!newIdOfOld) { sph_set_error("sph_read_edit_map: null pointer"); return SPH_ERR_INVALID; }
  const int rc = sph_derived_check(s, s->map, "sph_read_edit_map", "no removal has been made", "a stage, step or edit has run since the removal");
  if (rc != SPH_OK) return rc;
  if (s->mapIdentity) {
    for (int o = 0; o < s->mapLength; o++) newIdOfOld[o] = o;
    return SPH_OK;
  }
  return sph_d2h(s, newIdOfOld, s->d.backIndex, sizeof(int32_t) * (size_t)s->mapLength);
}

// one particle to be added: sph_create's test of its position, and its type; k: its index in the call's list
static int edit_validate(const sph_solver* s, const char* what, int k, const float* p4) {
  const float w = p4[3];
  if (const char* fault = sph_position_fault(s->cfg, p4)) {
    sph_set_error("%s: particle %d at (%g, %g, %g) is %s", what, k, p4[0], p4[1], p4[2], fault);
    return SPH_ERR_INVALID;
  }
  if (!(w >= 1.f && w < 4.f) || ((int)w != SPH_LIQUID_PARTICLE && (int)w != SPH_BOUNDARY_PARTICLE)) {
    sph_set_error("%s: particle %d has type %g; only liquid (1) and boundary (3) particles can be added", what, k, w);
    return SPH_ERR_INVALID;
  }
  return SPH_OK;
}

extern "C" int sph_add_particles(sph_solver* s, const float* position4, const float* velocity4, int32_t count) {
  ENTER(s);
  int rc = edit_check(s, "sph_add_particles");
  if (rc != SPH_OK) return rc;
  if (count < 0 || (count > 0 && (!position4 || !velocity4))) { sph_set_error("sph_add_particles: null pointer or negative count"); return SPH_ERR_INVALID; }
  if (count == 0) return SPH_OK;
  const int N = s->d.N;
  if ((long long)N + count > s->capacity) {
    sph_set_error("sph_add_particles: %d + %d particles exceed the capacity %d", N, count, s->capacity);
    return SPH_ERR_SIZE;
  }
  uint32_t sig = s->liquidSig;
  for (int k = 0; k < count; k++) {
    rc = edit_validate(s, "sph_add_particles", k, position4 + 4 * (size_t)k);
    if (rc != SPH_OK) return rc;
    sph_fold_liquid_signature(sig, position4 + 4 * (size_t)k, velocity4 + 4 * (size_t)k);
  }
  rc = sph_guard_position_write(s);
  if (rc != SPH_OK) return rc;
  SPH_HIP(hipMemcpyAsync(s->d.posOrig + N, position4, sizeof(float4) * (size_t)count, hipMemcpyHostToDevice, s->stream));
  SPH_HIP(hipMemcpyAsync(s->d.velOrig + N, velocity4, sizeof(float4) * (size_t)count, hipMemcpyHostToDevice, s->stream));
  if (s->d.membDelta) SPH_HIP(hipMemsetAsync(s->d.membDelta + N, 0, sizeof(float4) * (size_t)count, s->stream));
  rc = sph_fields_follow_add(s, N, count);  // the new ids carry each field's inflow
  if (rc != SPH_OK) return rc;
  SPH_HIP(hipStreamSynchronize(s->stream));
  s->liquidSig = sig;
  edit_commit(s, N + count);
  return SPH_OK;
}

extern "C" int sph_emit_lattice(sph_solver* s, const float origin[3], const float spacing[3], const int32_t dims[3], const float velocity[3],
                                float typeValue, int64_t* added) {
  ENTER(s);
  int rc = edit_check(s, "sph_emit_lattice");
  if (rc != SPH_OK) return rc;
  if (!origin || !spacing || !dims || !velocity || !added) { sph_set_error("sph_emit_lattice: null pointer"); return SPH_ERR_INVALID; }
  if (dims[0] < 0 || dims[1] < 0 || dims[2] < 0) { sph_set_error("sph_emit_lattice: negative dims"); return SPH_ERR_INVALID; }
  if (!(typeValue >= 1.f && typeValue < 4.f) || ((int)typeValue != SPH_LIQUID_PARTICLE && (int)typeValue != SPH_BOUNDARY_PARTICLE)) {
    sph_set_error("sph_emit_lattice: type %g; only liquid (1) and boundary (3) particles can be added", typeValue);
    return SPH_ERR_INVALID;
  }
  *added = 0;
  if (dims[0] == 0 || dims[1] == 0 || dims[2] == 0) return SPH_OK;
  const int N = s->d.N;
  // (each factor is bounded before the next product is formed: nothing overflows 64 bits)
  if (dims[0] > s->capacity || dims[1] > s->capacity || dims[2] > s->capacity || (long long)dims[0] * dims[1] > s->capacity ||
      N + (long long)dims[0] * dims[1] * dims[2] > s->capacity) {
    sph_set_error("sph_emit_lattice: %d particles + a %d x %d x %d lattice exceed the capacity %d", N, dims[0], dims[1], dims[2], s->capacity);
    return SPH_ERR_SIZE;
  }
  const long long count = (long long)dims[0] * dims[1] * dims[2];
  const sph_config& c = s->cfg;
  EditLattice a = {};
  a.ox = origin[0]; a.oy = origin[1]; a.oz = origin[2]; a.sx = spacing[0]; a.sy = spacing[1]; a.sz = spacing[2];
  a.nx = dims[0]; a.ny = dims[1]; a.nz = dims[2];
  a.vx = velocity[0]; a.vy = velocity[1]; a.vz = velocity[2]; a.typeValue = typeValue;
  a.wide = c.cellIdMask == 0xffffffffu;
  a.xmin = c.xmin; a.xmax = c.xmax; a.ymin = c.ymin; a.ymax = c.ymax; a.zmin = c.zmin; a.zmax = c.zmax;
  rc = sph_grow_scratch(s, s->editBuf, sphk_edit_scratch_bytes(s->capacity));
  if (rc != SPH_OK) return rc;
  rc = sph_guard_position_write(s);
  if (rc != SPH_OK) return rc;
  uint32_t* dCounters = nullptr;
  rc = sphk_edit_emit(s, a, (int)count, s->editBuf.p, &dCounters);  // into the unused tail [N, N + count)
  if (rc != SPH_OK) return rc;
  if (s->d.membDelta) SPH_HIP(hipMemsetAsync(s->d.membDelta + N, 0, sizeof(float4) * (size_t)count, s->stream));
  rc = sph_fields_follow_add(s, N, (int)count);  // into the fields' unused tail too: it only counts once the count is raised
  if (rc != SPH_OK) return rc;
  uint32_t bad[2] = {0, 0};
  rc = sph_d2h(s, bad, dCounters, sizeof(bad));
  if (rc != SPH_OK) return rc;
  if (bad[0]) {  // the count is not raised: the tail stays unused
    const int k = (int)bad[1], ix = k % a.nx, iy = (k / a.nx) % a.ny, iz = k / (a.nx * a.ny);
    sph_set_error("sph_emit_lattice: %u of %lld points are not finite%s; the first is point %d = (%d, %d, %d)", bad[0], count,
                  a.wide ? " or lie outside the box (wide cell ids need in-box input)" : "", k, ix, iy, iz);
    return SPH_ERR_INVALID;
  }
  const float p4[4] = {0.f, 0.f, 0.f, typeValue}, v4[4] = {velocity[0], velocity[1], velocity[2], 0.f};
  sph_fold_liquid_signature(s->liquidSig, p4, v4);
  edit_commit(s, N + (int)count);
  *added = count;
  return SPH_OK;
}

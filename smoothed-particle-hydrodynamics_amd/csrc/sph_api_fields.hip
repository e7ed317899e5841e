// C ABI of libsphmi.so (include/sphmi.h), the carried particle fields: sph_field_create / sph_field_release / sph_field_write /
// sph_field_read / sph_field_set_region / sph_field_set_selection / sph_field_diffuse / sph_field_diagnostics, and what the edits of
// sph_api_edit.hip do to the fields (sph_fields_follow_removal / sph_fields_follow_add). A field is passive: no call here says
// sph_state_changes, and the step never reads or writes a slot. What the translation units of the ABI share is in sph_api_internal.h.
#include <algorithm>
#include <cmath>

#include "sph_api_internal.h"
#include "sph_tree.h"  // tree_scratch_doubles

// ---------------------------------------------------------------------------------------------- carried fields
// What every field call checks first: no slab solver, a slot number in range (SPH_ERR_INVALID). Whether the slot exists is
// asked after the other arguments have been checked (SPH_ERR_ORDER).
static int field_check(sph_solver* s, int32_t slot, const char* what) {
  if (s->hasSlab) { sph_set_error("%s: a slab solver is not supported", what); return SPH_ERR_INVALID; }
  if (slot < 0 || slot >= SPH_FIELD_SLOTS) { sph_set_error("%s: slot %d is not in 0..%d", what, slot, SPH_FIELD_SLOTS - 1); return SPH_ERR_INVALID; }
  return SPH_OK;
}
static int field_exists(sph_solver* s, int32_t slot, const char* what) {
  if (!s->fieldLive[slot]) { sph_set_error("%s: slot %d does not exist (sph_field_create)", what, slot); return SPH_ERR_ORDER; }
  return SPH_OK;
}
static int field_finite(const char* what, const char* name, float x) {
  if (!std::isfinite(x)) { sph_set_error("%s: %s must be finite", what, name); return SPH_ERR_INVALID; }
  return SPH_OK;
}
// the first entry of a host array that is not finite is named; nothing has been written by then
static int field_values_finite(const char* what, const float* values, int n) {
  for (int o = 0; o < n; o++)
    if (!std::isfinite(values[o])) { sph_set_error("%s: value %d (%g) is not finite", what, o, values[o]); return SPH_ERR_INVALID; }
  return SPH_OK;
}
static float* field_of(sph_solver* s, int32_t slot) { return (float*)s->fieldSlot[slot].p; }

static int field_upload(sph_solver* s, int32_t slot, const float* values) {
  SPH_HIP(hipMemcpyAsync(field_of(s, slot), values, sizeof(float) * (size_t)s->d.N, hipMemcpyHostToDevice, s->stream));
  SPH_HIP(hipStreamSynchronize(s->stream));  // (the host array is pageable, and the call is blocking)
  return SPH_OK;
}

extern "C" int sph_field_create(sph_solver* s, int32_t slot, const float* valuesN, float inflow) {
  ENTER(s);
  int rc = field_check(s, slot, "sph_field_create");
  if (rc != SPH_OK) return rc;
  rc = field_finite("sph_field_create", "inflow", inflow);
  if (rc != SPH_OK) return rc;
  if (s->fieldLive[slot]) { sph_set_error("sph_field_create: slot %d exists already", slot); return SPH_ERR_ORDER; }
  if (valuesN) {
    rc = field_values_finite("sph_field_create", valuesN, s->d.N);
    if (rc != SPH_OK) return rc;
  }
  const size_t bytes = sizeof(float) * (size_t)std::max(s->capacity, 1);
  rc = sph_grow_scratch(s, s->fieldSlot[slot], bytes);
  if (rc != SPH_OK) return rc;
  SPH_HIP(hipMemsetAsync(s->fieldSlot[slot].p, 0, bytes, s->stream));
  if (valuesN) rc = field_upload(s, slot, valuesN);
  else SPH_HIP(hipStreamSynchronize(s->stream));
  if (rc != SPH_OK) return rc;
  s->fieldLive[slot] = true;
  s->fieldInflow[slot] = inflow;
  return SPH_OK;
}

extern "C" int sph_field_release(sph_solver* s, int32_t slot) {
  ENTER(s);
  int rc = field_check(s, slot, "sph_field_release");
  if (rc != SPH_OK) return rc;
  rc = field_exists(s, slot, "sph_field_release");
  if (rc != SPH_OK) return rc;
  SPH_HIP(hipStreamSynchronize(s->stream));
  SphScratch& b = s->fieldSlot[slot];
  hipFree(b.p);
  b.p = nullptr; b.bytes = 0;
  s->fieldLive[slot] = false;
  return SPH_OK;
}

extern "C" int sph_field_write(sph_solver* s, int32_t slot, const float* valuesN) {
  ENTER(s);
  int rc = field_check(s, slot, "sph_field_write");
  if (rc != SPH_OK) return rc;
  if (!valuesN) { sph_set_error("sph_field_write: null pointer"); return SPH_ERR_INVALID; }
  rc = field_exists(s, slot, "sph_field_write");
  if (rc != SPH_OK) return rc;
  rc = field_values_finite("sph_field_write", valuesN, s->d.N);
  return rc != SPH_OK ? rc : field_upload(s, slot, valuesN);
}

extern "C" int sph_field_read(sph_solver* s, int32_t slot, float* outN) {
  ENTER(s);
  int rc = field_check(s, slot, "sph_field_read");
  if (rc != SPH_OK) return rc;
  if (!outN) { sph_set_error("sph_field_read: null pointer"); return SPH_ERR_INVALID; }
  rc = field_exists(s, slot, "sph_field_read");
  return rc != SPH_OK ? rc : sph_d2h(s, outN, field_of(s, slot), sizeof(float) * (size_t)s->d.N);
}

extern "C" int sph_field_set_region(sph_solver* s, int32_t slot, const float* region6, uint32_t typeMask, float value, int64_t* painted) {
  ENTER(s);
  int rc = field_check(s, slot, "sph_field_set_region");
  if (rc != SPH_OK) return rc;
  if (!painted) { sph_set_error("sph_field_set_region: null pointer"); return SPH_ERR_INVALID; }
  rc = field_finite("sph_field_set_region", "value", value);
  if (rc != SPH_OK) return rc;
  SphSelector a = {};
  rc = sph_fill_selector(&a, region6, typeMask, "sph_field_set_region");
  if (rc != SPH_OK) return rc;
  rc = field_exists(s, slot, "sph_field_set_region");
  if (rc != SPH_OK) return rc;
  rc = sph_grow_scratch(s, s->fieldBuf, sphk_field_scratch_bytes(0));  // one word for the count
  if (rc != SPH_OK) return rc;
  uint32_t* dCount = (uint32_t*)s->fieldBuf.p;
  SPH_HIP(hipMemsetAsync(dCount, 0, sizeof(uint32_t), s->stream));
  rc = sphk_field_paint_region(s, field_of(s, slot), a, value, dCount);
  if (rc != SPH_OK) return rc;
  uint32_t n = 0;
  rc = sph_d2h(s, &n, dCount, sizeof(n));
  if (rc != SPH_OK) return rc;
  *painted = n;
  return SPH_OK;
}

extern "C" int sph_field_set_selection(sph_solver* s, int32_t slot, float value, int64_t* painted) {
  ENTER(s);
  int rc = field_check(s, slot, "sph_field_set_selection");
  if (rc != SPH_OK) return rc;
  if (!painted) { sph_set_error("sph_field_set_selection: null pointer"); return SPH_ERR_INVALID; }
  rc = field_finite("sph_field_set_selection", "value", value);
  if (rc != SPH_OK) return rc;
  rc = field_exists(s, slot, "sph_field_set_selection");
  if (rc != SPH_OK) return rc;
  rc = sph_selection_current(s, "sph_field_set_selection");
  if (rc != SPH_OK) return rc;
  rc = sphk_field_paint_list(s, field_of(s, slot), (const int32_t*)s->selList.p, (int)s->selCount, value);
  if (rc != SPH_OK) return rc;
  SPH_HIP(hipStreamSynchronize(s->stream));
  *painted = s->selCount;
  return SPH_OK;
}

static int field_mask_ok(uint32_t typeMask, const char* what) {
  if (typeMask == 0u || (typeMask & ~0xEu)) { sph_set_error("%s: typeMask must be a non-empty set of bits 1..3", what); return SPH_ERR_INVALID; }
  return SPH_OK;
}

extern "C" int sph_field_diffuse(sph_solver* s, int32_t slot, float coefficient, int32_t substeps, uint32_t typeMask, float* stability) {
  ENTER(s);
  int rc = field_check(s, slot, "sph_field_diffuse");
  if (rc != SPH_OK) return rc;
  rc = field_finite("sph_field_diffuse", "coefficient", coefficient);
  if (rc != SPH_OK) return rc;
  if (coefficient < 0.f) { sph_set_error("sph_field_diffuse: coefficient %g is negative", coefficient); return SPH_ERR_INVALID; }
  if (substeps < 0) { sph_set_error("sph_field_diffuse: substeps %d is negative", substeps); return SPH_ERR_INVALID; }
  rc = field_mask_ok(typeMask, "sph_field_diffuse");
  if (rc != SPH_OK) return rc;
  rc = field_exists(s, slot, "sph_field_diffuse");
  if (rc != SPH_OK) return rc;
  NEED(s, P_FIND | P_DENSITY, "sph_field_diffuse");  // the rows with their distances, and rho
  rc = sph_grow_scratch(s, s->fieldBuf, sphk_field_scratch_bytes(s->d.N));
  if (rc != SPH_OK) return rc;
  uint32_t* dSigma = nullptr;
  rc = sphk_field_diffuse(s, field_of(s, slot), coefficient, substeps, typeMask, s->fieldBuf.p, &dSigma);
  if (rc != SPH_OK) return rc;
  float sigma = 0.f;
  rc = sph_d2h(s, &sigma, dSigma, sizeof(sigma));  // the call's one wait
  if (rc != SPH_OK) return rc;
  if (stability) *stability = sigma;
  return SPH_OK;
}

extern "C" int sph_field_diagnostics(sph_solver* s, int32_t slot, const float* regions6, int32_t count, uint32_t typeMask, double* out) {
  ENTER(s);
  int rc = field_check(s, slot, "sph_field_diagnostics");
  if (rc != SPH_OK) return rc;
  if (!regions6 || !out) { sph_set_error("sph_field_diagnostics: null pointer"); return SPH_ERR_INVALID; }
  if (count < 1 || count > SPH_DIAG_MAX_REGIONS) { sph_set_error("sph_field_diagnostics: count %d is not in 1..%d", count, SPH_DIAG_MAX_REGIONS); return SPH_ERR_INVALID; }
  rc = field_mask_ok(typeMask, "sph_field_diagnostics");
  if (rc != SPH_OK) return rc;
  rc = field_exists(s, slot, "sph_field_diagnostics");
  if (rc != SPH_OK) return rc;
  NEED(s, P_DENSITY | P_PRESSUREFORCE, "sph_field_diagnostics");  // what sph_diagnostics needs
  DiagArgs a = {};
  for (int r = 0; r < count; r++) {
    SphSelector one = {};
    rc = sph_fill_selector(&one, regions6 + 6 * r, typeMask, "sph_field_diagnostics");
    if (rc != SPH_OK) return rc;
    std::copy(one.box, one.box + 6, a.box[r]);
  }
  a.count = count; a.typeMask = typeMask; a.rho0 = s->d.rho0;
  rc = sph_grow_scratch(s, s->diagBuf, sizeof(double) * tree_scratch_doubles(s->d.N, count, SPH_FIELD_DIAG_WORDS));
  if (rc != SPH_OK) return rc;
  double* records = nullptr;
  rc = sphk_field_diagnostics(s, field_of(s, slot), a, (double*)s->diagBuf.p, &records);
  if (rc != SPH_OK) return rc;
  rc = sph_d2h(s, out, records, sizeof(double) * SPH_FIELD_DIAG_WORDS * (size_t)count);
  return rc != SPH_OK ? rc : sph_check_finite_state(s);
}

// ---------------------------------------------------------------------------------------------- what an edit does to the fields
int sph_fields_follow_removal(sph_solver* s, int oldN, const int32_t* map) {
  bool any = false;
  for (int k = 0; k < SPH_FIELD_SLOTS; k++) any = any || s->fieldLive[k];
  if (!any) return SPH_OK;
  int rc = sph_grow_scratch(s, s->fieldStage, sizeof(float) * (size_t)std::max(s->capacity, 1));
  if (rc != SPH_OK) return rc;
  for (int k = 0; k < SPH_FIELD_SLOTS; k++) {
    if (!s->fieldLive[k]) continue;
    rc = sphk_field_compact(s, field_of(s, k), map, oldN, (float*)s->fieldStage.p);
    if (rc != SPH_OK) return rc;
    // the compacted copy is the slot from now on, and the slot's old buffer stages the next one (same size, the same stream)
    std::swap(s->fieldSlot[k].p, s->fieldStage.p);
    std::swap(s->fieldSlot[k].bytes, s->fieldStage.bytes);
  }
  return SPH_OK;
}

int sph_fields_follow_add(sph_solver* s, int first, int count) {
  for (int k = 0; k < SPH_FIELD_SLOTS; k++) {
    if (!s->fieldLive[k]) continue;
    const int rc = sphk_field_fill(s, field_of(s, k), first, count, s->fieldInflow[k]);
    if (rc != SPH_OK) return rc;
  }
  return SPH_OK;
}

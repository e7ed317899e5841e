// C ABI of libsphmi.so (include/sphmi.h), the analysis calls: field and gradient sampling, isosurfaces and their normals, flow
// diagnostics and histograms, connected components, particle selection, elastic-matter diagnostics, force decomposition, integral
// curves, particle and triangle rendering. All of them read the sorted state of the last completed step and write nothing the step reads. The results that
// outlive their call (mesh, labelling, selection, image) are SphDerived records: dropped first, stamped on success, checked by
// their readers. What the translation units of the ABI share is in sph_api_internal.h.
#include <stddef.h>
#include <string.h>

#include <algorithm>
#include <cmath>
#include <vector>

#include "sph_api_internal.h"
#include "sph_tree.h"  // tree_chunks, tree_scratch_doubles, terms_bytes

// ---------------------------------------------------------------------------------------------- field sampling
// Reads the sorted state the last step's density and pressure loop ran on (sph_sample.hip); enqueued on s->stream and waited
// for, like the sph_read_* family. Large requests go through the device scratch in pieces (z-chunks of a grid, runs of points)
// so that the scratch stays bounded whatever the request.
static const size_t kSampleScratchBytes = (size_t)64 << 20;

// region6 (or, when null, everything) into box, a NaN refused: the region half of sph_fill_selector, and the region lists' rule
static int region_fill(float box[6], const float* region6, const char* what) {
  for (int k = 0; k < 6; k++) {
    box[k] = region6 ? region6[k] : (k < 3 ? -INFINITY : INFINITY);
    if (std::isnan(box[k])) { sph_set_error("%s: a region bound is NaN", what); return SPH_ERR_INVALID; }
  }
  return SPH_OK;
}

// The argument and order rules every analysis call shares (declared in sph_api_internal.h, where the probes find them too).
int sph_sample_check(sph_solver* s, uint32_t typeMask, const char* what, SampleArgs* a) {
  if (s->hasSlab) { sph_set_error("%s: sampling a slab solver is not supported", what); return SPH_ERR_INVALID; }
  if (typeMask == 0u || (typeMask & ~0xEu)) { sph_set_error("%s: typeMask must be a non-empty set of bits 1..3", what); return SPH_ERR_INVALID; }
  NEED(s, P_DENSITY | P_PRESSUREFORCE, what);
  if (!a) return SPH_OK;
  volatile float hh = s->cfg.h * s->cfg.h;
  volatile float ss2 = s->cfg.simulationScale * s->cfg.simulationScale;
  *a = SampleArgs{};
  a->typeMask = typeMask; a->hh = hh; a->ss2 = ss2; a->mwp = (float)s->d.massWpoly6;
  return SPH_OK;
}

int sph_fill_selector(SphSelector* sel, const float* region6, uint32_t typeMask, const char* what) {
  if (typeMask == 0u || (typeMask & ~0xEu)) { sph_set_error("%s: typeMask must be a non-empty set of bits 1..3", what); return SPH_ERR_INVALID; }
  sel->typeMask = typeMask;
  return region_fill(sel->box, region6, what);
}

int sph_labels_current(sph_solver* s, const char* what, const int32_t** labels) {
  const int rc = sph_derived_check(s, s->cc, what, "no labelling has been made (sph_label_components)",
                                   "the solver's state has changed since the labelling");
  if (rc == SPH_OK) *labels = sphk_components_labels(s->ccBuf.p, s->cc.N);
  return rc;
}

int sph_selection_current(sph_solver* s, const char* what) {
  return sph_derived_check(s, s->sel, what, "no selection has been made", "the solver's state has changed since the selection");
}

// device buffer b grown to at least `bytes` (the old one is freed once the stream has finished with it)
int sph_grow_scratch(sph_solver* s, SphScratch& b, size_t bytes) {
  if (b.bytes >= bytes) return SPH_OK;
  if (b.p) { SPH_HIP(hipStreamSynchronize(s->stream)); hipFree(b.p); }
  b.p = nullptr; b.bytes = 0;
  SPH_HIP(hipMalloc(&b.p, bytes));
  b.bytes = bytes;
  return SPH_OK;
}

// Runs of `count` host query points (x, y, z, unused) through the sampling scratch: a piece's points are uploaded behind the
// room for its records of `words` floats, launch(points, n, records) enqueues the kernel on them (device pointers), and the
// records are copied out.
template <typename Launch>
static int sample_point_runs(sph_solver* s, const float* points4, int count, int words, float* out, Launch launch) {
  const size_t rec = sizeof(float) * words, perPoint = sizeof(float4) + rec;
  const int piece = (int)std::min<size_t>((size_t)count, kSampleScratchBytes / perPoint);
  int rc = sph_grow_scratch(s, s->sampleBuf, (size_t)piece * perPoint);
  if (rc != SPH_OK) return rc;
  float* dOut = (float*)s->sampleBuf.p;
  float* dPts = (float*)((char*)s->sampleBuf.p + (size_t)piece * rec);
  for (int first = 0; first < count; first += piece) {
    const int n = std::min(piece, count - first);
    SPH_HIP(hipMemcpyAsync(dPts, points4 + (size_t)first * 4, sizeof(float4) * (size_t)n, hipMemcpyHostToDevice, s->stream));
    rc = launch(dPts, n, dOut);
    if (rc != SPH_OK) return rc;
    rc = sph_d2h(s, out + (size_t)first * words, dOut, rec * (size_t)n);
    if (rc != SPH_OK) return rc;
  }
  return SPH_OK;
}

// A lattice in z-chunks of whole bricks (4 planes) that fit the sampling scratch, at least one brick layer however large a
// plane is: launch(k0, nz, records) enqueues the kernel that fills the records (`words` floats each) of planes [k0, k0 + nz),
// consume(first, n, records) takes those n records, the lattice's records first .. first + n, from the scratch.
template <typename Launch, typename Consume>
static int sample_grid_chunks(sph_solver* s, const int32_t dims[3], int words, Launch launch, Consume consume) {
  const size_t plane = (size_t)dims[0] * (size_t)dims[1], planeBytes = sizeof(float) * words * plane;
  const int planes = (int)std::min<size_t>((size_t)dims[2], std::max<size_t>(kSampleScratchBytes / planeBytes / 4, 1) * 4);
  int rc = sph_grow_scratch(s, s->sampleBuf, planeBytes * (size_t)planes);
  if (rc != SPH_OK) return rc;
  float* records = (float*)s->sampleBuf.p;
  for (int k0 = 0; k0 < dims[2]; k0 += planes) {
    const int nz = std::min(planes, dims[2] - k0);
    rc = launch(k0, nz, records);
    if (rc != SPH_OK) return rc;
    rc = consume(plane * (size_t)k0, plane * (size_t)nz, records);
    if (rc != SPH_OK) return rc;
  }
  return SPH_OK;
}

extern "C" int sph_sample_points(sph_solver* s, const float* points4, int32_t count, uint32_t typeMask, float* out) {
  ENTER(s);
  if (count < 0 || (count > 0 && (!points4 || !out))) { sph_set_error("sph_sample_points: bad count or null pointer"); return SPH_ERR_INVALID; }
  SampleArgs a;
  const int rc = sph_sample_check(s, typeMask, "sph_sample_points", &a);
  if (rc != SPH_OK || count == 0) return rc;
  return sample_point_runs(s, points4, count, SPH_SAMPLE_WORDS, out,
                           [&](const float* pts, int n, float* records) { return sphk_sample_points(s, a, pts, n, records); });
}

extern "C" int sph_sample_grid(sph_solver* s, const float origin[3], const float spacing[3], const int32_t dims[3],
                               uint32_t typeMask, float* out) {
  ENTER(s);
  if (!origin || !spacing || !dims || !out || dims[0] <= 0 || dims[1] <= 0 || dims[2] <= 0) {
    sph_set_error("sph_sample_grid: null pointer or dims <= 0");
    return SPH_ERR_INVALID;
  }
  SampleArgs a;
  const int rc = sph_sample_check(s, typeMask, "sph_sample_grid", &a);
  if (rc != SPH_OK) return rc;
  return sample_grid_chunks(
      s, dims, SPH_SAMPLE_WORDS,
      [&](int k0, int nz, float* records) { return sphk_sample_grid(s, a, origin, spacing, dims[0], dims[1], k0, nz, records); },
      [&](size_t first, size_t n, const float* records) {
        return sph_d2h(s, out + first * SPH_SAMPLE_WORDS, records, sizeof(float) * SPH_SAMPLE_WORDS * n);
      });
}

// ---------------------------------------------------------------------------------------------- isosurface extraction
// The scalar lattice comes from the sampling kernels (z-chunks through the sampling scratch, one word kept per record), then
// marching cubes runs on it (sph_surface.hip). Blocks once, for the counts; the emitting kernels stay queued on s->stream.
static size_t surf_bytes_align(size_t b) { return (b + 255) & ~(size_t)255; }  // triangles start at a 256-B boundary

extern "C" int sph_extract_surface(sph_solver* s, const float origin[3], const float spacing[3], const int32_t dims[3],
                                   uint32_t typeMask, int32_t field, float iso, int64_t counts[2]) {
  ENTER(s);
  sph_derived_drop(s->mesh);
  sph_derived_drop(s->shells);  // a measure is of the mesh it was made on
  s->meshCounts[0] = s->meshCounts[1] = 0;
  if (counts) counts[0] = counts[1] = 0;
  if (!origin || !spacing || !dims || !counts) { sph_set_error("sph_extract_surface: null pointer"); return SPH_ERR_INVALID; }
  if (field < 0 || field >= SPH_SURFACE_FIELDS) { sph_set_error("sph_extract_surface: field %d is not in 0..5", field); return SPH_ERR_INVALID; }
  if (!std::isfinite(iso)) { sph_set_error("sph_extract_surface: iso is not finite"); return SPH_ERR_INVALID; }
  if (dims[0] < 2 || dims[1] < 2 || dims[2] < 2) { sph_set_error("sph_extract_surface: dims must all be >= 2"); return SPH_ERR_INVALID; }
  const long long P = (long long)dims[0] * (long long)dims[1] * (long long)dims[2];
  if (P > 0x7fffffffLL) { sph_set_error("sph_extract_surface: the lattice has more than 2^31-1 points"); return SPH_ERR_INVALID; }
  SampleArgs a;
  int rc = sph_sample_check(s, typeMask, "sph_extract_surface", &a);
  if (rc != SPH_OK) return rc;
  rc = sph_grow_scratch(s, s->surfBuf, sphk_surface_scratch_bytes(P));
  if (rc != SPH_OK) return rc;
  float* lattice = (float*)s->surfBuf.p;  // the scratch's first P floats
  rc = sample_grid_chunks(
      s, dims, SPH_SAMPLE_WORDS,
      [&](int k0, int nz, float* records) { return sphk_sample_grid(s, a, origin, spacing, dims[0], dims[1], k0, nz, records); },
      [&](size_t first, size_t n, const float* records) { return sphk_surface_field(s, records, field, (int)n, lattice + first); });
  if (rc != SPH_OK) return rc;
  unsigned long long totals[2] = {0, 0};
  rc = sphk_surface_count(s, s->surfBuf.p, dims, iso, totals);
  if (rc != SPH_OK) return rc;
  if (totals[0] > 0x7fffffffULL) {
    sph_set_error("sph_extract_surface: %llu vertices exceed the int32 vertex ids", totals[0]);
    return SPH_ERR_SIZE;
  }
  const size_t vBytes = surf_bytes_align(sizeof(float) * 3 * (size_t)totals[0]);
  rc = sph_grow_scratch(s, s->meshBuf, std::max<size_t>(vBytes + sizeof(int32_t) * 3 * (size_t)totals[1], 1));
  if (rc != SPH_OK) return rc;
  rc = sphk_surface_emit(s, s->surfBuf.p, dims, iso, origin, spacing, (float*)s->meshBuf.p, (int32_t*)((char*)s->meshBuf.p + vBytes));
  if (rc != SPH_OK) return rc;
  s->meshCounts[0] = (int64_t)totals[0];
  s->meshCounts[1] = (int64_t)totals[1];
  s->meshTypeMask = typeMask;
  s->meshField = field;
  for (int k = 0; k < 3; k++) { s->meshOrigin[k] = origin[k]; s->meshSpacing[k] = spacing[k]; s->meshDims[k] = dims[k]; }
  sph_derived_stamp(s, s->mesh);
  counts[0] = s->meshCounts[0];
  counts[1] = s->meshCounts[1];
  return SPH_OK;
}

extern "C" int sph_read_surface(sph_solver* s, float* vertices, int32_t* triangles) {
  ENTER(s);
  int rc = sph_derived_check(s, s->mesh, "sph_read_surface", "no surface has been extracted", nullptr);
  if (rc != SPH_OK) return rc;
  const size_t vBytes = sizeof(float) * 3 * (size_t)s->meshCounts[0];
  if (vertices && vBytes) rc = sph_d2h(s, vertices, s->meshBuf.p, vBytes);
  if (rc != SPH_OK) return rc;
  const size_t tBytes = sizeof(int32_t) * 3 * (size_t)s->meshCounts[1];
  if (triangles && tBytes) rc = sph_d2h(s, triangles, (char*)s->meshBuf.p + surf_bytes_align(vBytes), tBytes);
  return rc;
}

// ---------------------------------------------------------------------------------------------- surface measures
// Shells, open sides, area, volume and area moments of the mesh in meshBuf (sph_shells.hip). A function of the mesh alone: the
// measure stays valid across steps and is dropped by the next extraction. Blocks twice: for the shell count, and for the totals.
// frexp's exponent of x, 0 for a zero or non-finite x
static int shell_exponent(double x) {
  int e = 0;
  if (std::isfinite(x) && x != 0.0) frexp(x, &e);
  return e;
}

extern "C" int sph_measure_surface(sph_solver* s, int64_t counts[4], int32_t exps[3]) {
  ENTER(s);
  const char* what = "sph_measure_surface";
  sph_derived_drop(s->shells);
  for (int k = 0; k < 4; k++) { s->shellCounts[k] = 0; if (counts) counts[k] = 0; }
  if (!counts || !exps) { sph_set_error("%s: null pointer", what); return SPH_ERR_INVALID; }
  if (s->hasSlab) { sph_set_error("%s: measuring a slab solver is not supported", what); return SPH_ERR_INVALID; }
  int rc = sph_derived_check(s, s->mesh, what, "no surface has been extracted", nullptr);
  if (rc != SPH_OK) return rc;
  const int64_t V = s->meshCounts[0], T = s->meshCounts[1];
  if (V > 0x7fffffffLL - 4096 || T > 0x7fffffffLL - 4096) { sph_set_error("%s: %lld vertices or %lld triangles exceed the int32 indices", what, (long long)V, (long long)T); return SPH_ERR_SIZE; }
  // the exponents: a function of the lattice and of T (include/sphmi.h)
  double extent = 0.0, widest = 0.0;
  for (int k = 0; k < 3; k++) {
    const double sp = fabs((double)s->meshSpacing[k]);
    extent = std::max(extent, (double)(s->meshDims[k] - 1) * sp);
    widest = std::max(widest, sp);
  }
  int bT = 0;
  while (((int64_t)1 << bT) < T + 1) bT++;
  const int eL = 1 + shell_exponent(extent), eS = 1 + shell_exponent(widest);
  ShellArgs a = {};
  a.V = (int)V; a.T = (int)T;
  a.verts = (const float*)s->meshBuf.p;
  a.tris = (const int32_t*)((const char*)s->meshBuf.p + surf_bytes_align(sizeof(float) * 3 * (size_t)V));
  for (int k = 0; k < 3; k++) a.origin[k] = (double)s->meshOrigin[k];
  a.kA = 60 - bT - 2 * eS; a.kV = 59 - bT - eL - 2 * eS; a.kM = 58 - bT - eL - 2 * eS;
  a.limit = ldexp(1.0, 62 - bT);
  exps[0] = a.kA; exps[1] = a.kV; exps[2] = a.kM;
  int S = 0;
  if (V > 0) {
    rc = sph_grow_scratch(s, s->shellBuf, sphk_shells_scratch_bytes(a.V));
    if (rc != SPH_OK) return rc;
    uint32_t* dTotals = nullptr;
    rc = sphk_shells_link(s, a, s->shellBuf.p, &dTotals);
    if (rc != SPH_OK) return rc;
    uint32_t totals[3] = {0, 0, 0};
    rc = sph_d2h(s, totals, dTotals, sizeof(totals));  // the first wait: the table's size
    if (rc != SPH_OK) return rc;
    if (totals[2]) {
      sph_set_error("%s: a parent walk or hook retry ran past its bound of V steps, or a triangle names no vertex (flags 0x%x)", what, totals[2]);
      return SPH_ERR_HIP;
    }
    S = (int)totals[1];
    rc = sph_grow_scratch(s, s->shellTable, sphk_shells_table_bytes(S));
    if (rc != SPH_OK) return rc;
    rc = sphk_shells_number(s, a, s->shellBuf.p, S, s->shellTable.p);
    if (rc != SPH_OK) return rc;
    int64_t sums[3] = {0, 0, 0};
    rc = sph_d2h(s, sums, sphk_shells_totals(s->shellTable.p, S), sizeof(sums));  // the second: closed shells, open sides, bad triangles
    if (rc != SPH_OK) return rc;
    s->shellCounts[0] = S; s->shellCounts[1] = sums[0]; s->shellCounts[2] = sums[1]; s->shellCounts[3] = sums[2];
  }
  sph_derived_stamp(s, s->shells);
  for (int k = 0; k < 4; k++) counts[k] = s->shellCounts[k];
  return SPH_OK;
}

extern "C" int sph_read_shells(sph_solver* s, int32_t* vertexShell, int64_t* table, float* bbox) {
  ENTER(s);
  int rc = sph_derived_check(s, s->shells, "sph_read_shells", "no surface has been measured (sph_measure_surface)", nullptr);
  if (rc != SPH_OK) return rc;
  const size_t V = (size_t)s->meshCounts[0], S = (size_t)s->shellCounts[0];
  if (vertexShell && V) rc = sph_d2h(s, vertexShell, sphk_shells_labels(s->shellBuf.p, (int)V), sizeof(int32_t) * V);
  if (rc != SPH_OK) return rc;
  if (table && S) rc = sph_d2h(s, table, s->shellTable.p, sizeof(int64_t) * SPH_SHELL_WORDS * S);
  if (rc != SPH_OK) return rc;
  if (bbox && S) rc = sph_d2h(s, bbox, sphk_shells_bbox(s->shellTable.p, (int)S), sizeof(float) * 6 * S);
  return rc;
}

// ---------------------------------------------------------------------------------------------- gradient sampling
// The same state, selection, argument rules and scratch as field sampling, with 32-word records (sph_gradient.hip).
static float gradient_scale(const sph_solver* s) { return (float)(-6.0 * s->d.massWpoly6 * (double)s->cfg.simulationScale); }

extern "C" int sph_sample_gradient_points(sph_solver* s, const float* points4, int32_t count, uint32_t typeMask, float* out) {
  ENTER(s);
  if (count < 0 || (count > 0 && (!points4 || !out))) { sph_set_error("sph_sample_gradient_points: bad count or null pointer"); return SPH_ERR_INVALID; }
  SampleArgs a;
  const int rc = sph_sample_check(s, typeMask, "sph_sample_gradient_points", &a);
  if (rc != SPH_OK || count == 0) return rc;
  const float K = gradient_scale(s);
  return sample_point_runs(s, points4, count, SPH_GRADIENT_WORDS, out,
                           [&](const float* pts, int n, float* records) { return sphk_gradient_points(s, a, K, pts, n, records); });
}

extern "C" int sph_sample_gradient_grid(sph_solver* s, const float origin[3], const float spacing[3], const int32_t dims[3],
                                        uint32_t typeMask, float* out) {
  ENTER(s);
  if (!origin || !spacing || !dims || !out || dims[0] <= 0 || dims[1] <= 0 || dims[2] <= 0) {
    sph_set_error("sph_sample_gradient_grid: null pointer or dims <= 0");
    return SPH_ERR_INVALID;
  }
  SampleArgs a;
  const int rc = sph_sample_check(s, typeMask, "sph_sample_gradient_grid", &a);
  if (rc != SPH_OK) return rc;
  const float K = gradient_scale(s);
  return sample_grid_chunks(
      s, dims, SPH_GRADIENT_WORDS,
      [&](int k0, int nz, float* records) { return sphk_gradient_grid(s, a, K, origin, spacing, dims[0], dims[1], k0, nz, records); },
      [&](size_t first, size_t n, const float* records) {
        return sph_d2h(s, out + first * SPH_GRADIENT_WORDS, records, sizeof(float) * SPH_GRADIENT_WORDS * n);
      });
}

// Normals of the mesh in meshBuf, computed from its vertices where they lie; runs of vertices through the sampling scratch.
extern "C" int sph_surface_normals(sph_solver* s, float* normals) {
  ENTER(s);
  int rc = sph_derived_check(s, s->mesh, "sph_surface_normals", "no surface has been extracted",
                             "the solver's state has changed since the surface was extracted");
  if (rc != SPH_OK) return rc;
  const int64_t V = s->meshCounts[0];
  if (V > 0 && !normals) { sph_set_error("sph_surface_normals: null pointer"); return SPH_ERR_INVALID; }
  SampleArgs a;
  rc = sph_sample_check(s, s->meshTypeMask, "sph_surface_normals", &a);
  if (rc != SPH_OK || V == 0) return rc;
  const size_t rec = sizeof(float) * 3;
  const int piece = (int)std::min<size_t>((size_t)V, kSampleScratchBytes / rec);
  rc = sph_grow_scratch(s, s->sampleBuf, (size_t)piece * rec);
  if (rc != SPH_OK) return rc;
  const float K = gradient_scale(s);
  for (int64_t first = 0; first < V; first += piece) {
    const int n = (int)std::min<int64_t>(piece, V - first);
    rc = sphk_surface_normals(s, a, K, s->meshField, (const float*)s->meshBuf.p + 3 * (size_t)first, n, (float*)s->sampleBuf.p);
    if (rc != SPH_OK) return rc;
    rc = sph_d2h(s, normals + 3 * (size_t)first, s->sampleBuf.p, rec * (size_t)n);
    if (rc != SPH_OK) return rc;
  }
  return SPH_OK;
}

// ---------------------------------------------------------------------------------------------- flow diagnostics
// Reductions and histograms over the same state as sampling (sph_diag.hip); blocking, read-only, no stage timing.
// the `count` regions (6 floats each) and the types of a region-list call into its arguments (sph_sample_check has checked the mask)
static int diag_fill_regions(sph_solver* s, DiagArgs* a, const float* regions6, int count, uint32_t typeMask, const char* what) {
  for (int r = 0; r < count; r++) {
    const int rc = region_fill(a->box[r], regions6 + 6 * r, what);
    if (rc != SPH_OK) return rc;
  }
  a->count = count; a->typeMask = typeMask; a->rho0 = s->d.rho0;
  return SPH_OK;
}

// the records of a.count selections: through the diagnostics scratch to `out`, then the check every blocking call ends with
static int diag_records(sph_solver* s, const DiagArgs& a, double* out) {
  int rc = sph_grow_scratch(s, s->diagBuf, sizeof(double) * tree_scratch_doubles(s->d.N, a.count, SPH_DIAG_WORDS));
  if (rc != SPH_OK) return rc;
  double* records = nullptr;
  rc = sphk_diagnostics(s, a, (double*)s->diagBuf.p, &records);
  if (rc != SPH_OK) return rc;
  rc = sph_d2h(s, out, records, sizeof(double) * SPH_DIAG_WORDS * (size_t)a.count);
  return rc != SPH_OK ? rc : sph_check_finite_state(s);
}

extern "C" int sph_diagnostics(sph_solver* s, const float* regions6, int32_t count, uint32_t typeMask, double* out) {
  ENTER(s);
  if (!regions6 || !out) { sph_set_error("sph_diagnostics: null pointer"); return SPH_ERR_INVALID; }
  if (count < 1 || count > SPH_DIAG_MAX_REGIONS) { sph_set_error("sph_diagnostics: count %d is not in 1..%d", count, SPH_DIAG_MAX_REGIONS); return SPH_ERR_INVALID; }
  int rc = sph_sample_check(s, typeMask, "sph_diagnostics");
  if (rc != SPH_OK) return rc;
  DiagArgs a = {};
  rc = diag_fill_regions(s, &a, regions6, count, typeMask, "sph_diagnostics");
  return rc != SPH_OK ? rc : diag_records(s, a, out);
}

extern "C" int sph_histogram(sph_solver* s, int32_t field, float lo, float hi, int32_t bins, const float* region6, uint32_t typeMask,
                             uint32_t* out) {
  ENTER(s);
  if (!out) { sph_set_error("sph_histogram: null pointer"); return SPH_ERR_INVALID; }
  if (field < 0 || field > 6) { sph_set_error("sph_histogram: field %d is not in 0..6", field); return SPH_ERR_INVALID; }
  if (bins < 1 || bins > SPH_HIST_MAX_BINS) { sph_set_error("sph_histogram: bins %d is not in 1..%d", bins, SPH_HIST_MAX_BINS); return SPH_ERR_INVALID; }
  if (!std::isfinite(lo) || !std::isfinite(hi) || !(lo < hi)) { sph_set_error("sph_histogram: lo and hi must be finite with lo < hi"); return SPH_ERR_INVALID; }
  int rc = sph_sample_check(s, typeMask, "sph_histogram");
  if (rc != SPH_OK) return rc;
  HistArgs a = {};
  rc = sph_fill_selector(&a.sel, region6, typeMask, "sph_histogram");
  if (rc != SPH_OK) return rc;
  volatile float width = hi - lo;
  volatile float scale = (float)bins / width;
  a.field = field; a.bins = bins; a.lo = lo; a.hi = hi; a.scale = scale;
  rc = sph_grow_scratch(s, s->diagBuf, sizeof(uint32_t) * (size_t)(bins + 2));
  if (rc != SPH_OK) return rc;
  rc = sphk_histogram(s, a, (uint32_t*)s->diagBuf.p);
  if (rc != SPH_OK) return rc;
  rc = sph_d2h(s, out, s->diagBuf.p, sizeof(uint32_t) * (size_t)(bins + 2));
  return rc != SPH_OK ? rc : sph_check_finite_state(s);
}

// ---------------------------------------------------------------------------------------------- binned diagnostics
// The diagnostics record of every bin of a lattice (sph_bins.hip): same state, order and mask rules as sph_diagnostics, plus the
// lattice's own. Blocks once for the number of (chunk, bin) entries, which sizes the pool.
static int bin_check(sph_solver* s, const sph_bin_lattice* g, const void* out, const char* what, BinArgs* a, int* bins) {
  if (!g || !out) { sph_set_error("%s: null pointer", what); return SPH_ERR_INVALID; }
  const int rc = sph_sample_check(s, g->typeMask, what);
  if (rc != SPH_OK) return rc;
  long long B = 1;
  for (int k = 0; k < 3; k++) {
    if (!std::isfinite(g->origin[k]) || !std::isfinite(g->spacing[k])) { sph_set_error("%s: origin and spacing must be finite", what); return SPH_ERR_INVALID; }
    if (g->dims[k] <= 0) { sph_set_error("%s: dims must be > 0", what); return SPH_ERR_INVALID; }
    if (g->spacing[k] < 0.f || (g->spacing[k] == 0.f && g->dims[k] != 1)) {
      sph_set_error("%s: spacing must be > 0 (0 with dims 1: the whole axis)", what);
      return SPH_ERR_INVALID;
    }
    B *= g->dims[k];
    if (B > SPH_BIN_MAX_BINS) { sph_set_error("%s: more than %d bins", what, SPH_BIN_MAX_BINS); return SPH_ERR_INVALID; }
    a->o[k] = g->origin[k]; a->s[k] = g->spacing[k]; a->n[k] = g->dims[k];
  }
  a->typeMask = g->typeMask; a->rho0 = s->d.rho0;
  *bins = (int)B;
  return SPH_OK;
}

extern "C" int sph_bin_diagnostics(sph_solver* s, const sph_bin_lattice* g, double* out) {
  ENTER(s);
  BinArgs a = {};
  int B = 0;
  int rc = bin_check(s, g, out, "sph_bin_diagnostics", &a, &B);
  if (rc != SPH_OK) return rc;
  rc = sph_grow_scratch(s, s->binBuf, sphk_bin_scratch_bytes(s->d.N, B));
  if (rc != SPH_OK) return rc;
  uint32_t *dTotal = nullptr, entries = 0;
  rc = sphk_bin_index(s, a, B, s->binBuf.p, true, &dTotal);
  if (rc != SPH_OK) return rc;
  rc = sph_d2h(s, &entries, dTotal, sizeof(entries));
  if (rc != SPH_OK) return rc;
  rc = sph_grow_scratch(s, s->binPool, sphk_bin_pool_bytes(entries));
  if (rc != SPH_OK) return rc;
  double* records = nullptr;
  rc = sphk_bin_records(s, a, B, s->binBuf.p, s->binPool.p, entries, &records);
  if (rc != SPH_OK) return rc;
  rc = sph_d2h(s, out, records, sizeof(double) * SPH_DIAG_WORDS * (size_t)B);
  return rc != SPH_OK ? rc : sph_check_finite_state(s);
}

extern "C" int sph_bin_index(sph_solver* s, const sph_bin_lattice* g, int32_t* binOfSorted) {
  ENTER(s);
  BinArgs a = {};
  int B = 0;
  int rc = bin_check(s, g, binOfSorted, "sph_bin_index", &a, &B);
  if (rc != SPH_OK) return rc;
  rc = sph_grow_scratch(s, s->binBuf, sphk_bin_scratch_bytes(s->d.N, B));
  if (rc != SPH_OK) return rc;
  rc = sphk_bin_index(s, a, B, s->binBuf.p, false, nullptr);
  if (rc != SPH_OK) return rc;
  rc = sph_d2h(s, binOfSorted, sphk_bin_ids(s->binBuf.p, B), sizeof(int32_t) * (size_t)s->d.N);
  return rc != SPH_OK ? rc : sph_check_finite_state(s);
}

// ---------------------------------------------------------------------------------------------- connected components
// The pieces the matter is in: components of the graph of the last step's neighbour rows (sph_components.hip). The labelling
// lives in ccBuf / ccTable until the next one; the per-component records reuse the diagnostics tree with the labels as selection.
extern "C" int sph_label_components(sph_solver* s, float linkRadius, uint32_t typeMask, int64_t counts[2]) {
  ENTER(s);
  sph_derived_drop(s->cc);
  s->ccCounts[0] = s->ccCounts[1] = 0;
  if (counts) counts[0] = counts[1] = 0;
  if (!counts) { sph_set_error("sph_label_components: null pointer"); return SPH_ERR_INVALID; }
  if (std::isnan(linkRadius) || !(linkRadius > 0.f)) { sph_set_error("sph_label_components: linkRadius must be > 0"); return SPH_ERR_INVALID; }
  int rc = sph_sample_check(s, typeMask, "sph_label_components");
  if (rc != SPH_OK) return rc;
  NEED(s, P_FIND, "sph_label_components");
  const bool finite = !std::isinf(linkRadius);
  volatile float link2 = linkRadius * linkRadius;
  rc = sph_grow_scratch(s, s->ccBuf, sphk_components_scratch_bytes(s->d.N));
  if (rc != SPH_OK) return rc;
  uint32_t* dTotals = nullptr;
  rc = sphk_components_link(s, typeMask, finite, link2, s->ccBuf.p, &dTotals);
  if (rc != SPH_OK) return rc;
  uint32_t totals[3] = {0, 0, 0};
  rc = sph_d2h(s, totals, dTotals, sizeof(totals));  // the call's one wait for a result
  if (rc != SPH_OK) return rc;
  if (totals[2]) {
    sph_set_error("sph_label_components: a parent walk or hook retry ran past its bound of N steps (flags 0x%x)", totals[2]);
    return SPH_ERR_HIP;
  }
  const int C = (int)totals[1];
  rc = sph_grow_scratch(s, s->ccTable, sizeof(int32_t) * 8 * (size_t)std::max(C, 1));
  if (rc != SPH_OK) return rc;
  rc = sphk_components_number(s, s->ccBuf.p, C, (int32_t*)s->ccTable.p);
  if (rc != SPH_OK) return rc;
  rc = sph_check_finite_state(s);  // (synchronises the stream)
  if (rc != SPH_OK) return rc;
  s->ccCounts[0] = (int64_t)totals[0];
  s->ccCounts[1] = (int64_t)C;
  sph_derived_stamp(s, s->cc);
  counts[0] = s->ccCounts[0];
  counts[1] = s->ccCounts[1];
  return SPH_OK;
}

extern "C" int sph_read_components(sph_solver* s, int32_t* labels, int32_t* rootCount, float* bbox) {
  ENTER(s);
  int rc = sph_derived_check(s, s->cc, "sph_read_components", "no labelling has been made", nullptr);
  if (rc != SPH_OK) return rc;
  if (labels && s->cc.N > 0) rc = sph_d2h(s, labels, sphk_components_labels(s->ccBuf.p, s->cc.N), sizeof(int32_t) * (size_t)s->cc.N);
  if (rc != SPH_OK) return rc;
  const size_t C = (size_t)s->ccCounts[1];
  if ((rootCount || bbox) && C > 0) {
    std::vector<int32_t> rows(C * 8);
    rc = sph_d2h(s, rows.data(), s->ccTable.p, sizeof(int32_t) * 8 * C);
    if (rc != SPH_OK) return rc;
    for (size_t c = 0; c < C; c++) {
      if (rootCount) { rootCount[2 * c] = rows[8 * c]; rootCount[2 * c + 1] = rows[8 * c + 1]; }
      if (bbox) memcpy(bbox + 6 * c, &rows[8 * c + 2], sizeof(float) * 6);
    }
  }
  return SPH_OK;
}

extern "C" int sph_component_diagnostics(sph_solver* s, const int32_t* components, int32_t count, double* out) {
  ENTER(s);
  if (!components || !out) { sph_set_error("sph_component_diagnostics: null pointer"); return SPH_ERR_INVALID; }
  if (count < 1 || count > SPH_DIAG_MAX_REGIONS) { sph_set_error("sph_component_diagnostics: count %d is not in 1..%d", count, SPH_DIAG_MAX_REGIONS); return SPH_ERR_INVALID; }
  DiagArgs a = {};
  const int rc = sph_labels_current(s, "sph_component_diagnostics", &a.labels);
  if (rc != SPH_OK) return rc;
  for (int r = 0; r < count; r++) {
    if (components[r] < 0 || (int64_t)components[r] >= s->ccCounts[1]) {
      sph_set_error("sph_component_diagnostics: component %d is not in 0..%lld", components[r], (long long)s->ccCounts[1] - 1);
      return SPH_ERR_INVALID;
    }
    a.comp[r] = components[r];
  }
  a.count = count; a.typeMask = 0xEu; a.rho0 = s->d.rho0;
  return diag_records(s, a, out);
}


// ---------------------------------------------------------------------------------------------- particle selection
// Which particles, not what about them (sph_select.hip): a counting pass sizes the list, the list is written in ascending
// sorted index, and the records are gathered from the live state when they are asked for (an SphDerived record, like the mesh and the labelling).
static int select_check(sph_solver* s, uint32_t typeMask, const char* what, float* ss2) {
  SampleArgs a;
  const int rc = sph_sample_check(s, typeMask, what, &a);
  if (rc != SPH_OK) return rc;
  NEED(s, P_FIND, what);
  *ss2 = a.ss2;
  return SPH_OK;
}

extern "C" int sph_particle_measure(sph_solver* s, float* out) {
  ENTER(s);
  if (!out) { sph_set_error("sph_particle_measure: null pointer"); return SPH_ERR_INVALID; }
  float ss2 = 0.f;
  int rc = select_check(s, 0xEu, "sph_particle_measure", &ss2);
  if (rc != SPH_OK) return rc;
  const int N = s->d.N;
  if (N <= 0) return SPH_OK;
  const int piece = (int)std::min<size_t>(((size_t)N + SPH_BLOCK - 1) / SPH_BLOCK * SPH_BLOCK, kSampleScratchBytes / sizeof(float));
  rc = sph_grow_scratch(s, s->sampleBuf, sizeof(float) * (size_t)piece);
  if (rc != SPH_OK) return rc;
  for (int first = 0; first < N; first += piece) {
    const int n = std::min(piece, N - first);
    rc = sphk_particle_measure(s, ss2, first, n, (float*)s->sampleBuf.p);
    if (rc != SPH_OK) return rc;
    rc = sph_d2h(s, out + first, s->sampleBuf.p, sizeof(float) * (size_t)n);
    if (rc != SPH_OK) return rc;
  }
  return sph_check_finite_state(s);
}

extern "C" int sph_select_particles(sph_solver* s, const float* region6, uint32_t typeMask, const sph_select_term* terms,
                                    int32_t termCount, int32_t component, int64_t* count) {
  ENTER(s);
  sph_derived_drop(s->sel);
  s->selCount = 0;
  if (count) *count = 0;
  if (!count) { sph_set_error("sph_select_particles: null count"); return SPH_ERR_INVALID; }
  SelectArgs a = {};
  int rc = select_check(s, typeMask, "sph_select_particles", &a.ss2);
  if (rc != SPH_OK) return rc;
  rc = sph_fill_selector(&a.sel, region6, typeMask, "sph_select_particles");
  if (rc != SPH_OK) return rc;
  if (termCount < 0 || termCount > SPH_SELECT_MAX_TERMS) {
    sph_set_error("sph_select_particles: termCount %d is not in 0..%d", termCount, SPH_SELECT_MAX_TERMS);
    return SPH_ERR_INVALID;
  }
  if (termCount > 0 && !terms) { sph_set_error("sph_select_particles: null terms"); return SPH_ERR_INVALID; }
  a.termCount = termCount;
  for (int k = 0; k < termCount; k++) {
    const sph_select_term& t = terms[k];
    if (t.field < 0 || t.field > SPH_SELECT_FIELD_SURFACE) { sph_set_error("sph_select_particles: field %d is not in 0..7", t.field); return SPH_ERR_INVALID; }
    if (std::isnan(t.lo) || std::isnan(t.hi) || !(t.lo < t.hi)) { sph_set_error("sph_select_particles: a term needs lo < hi, neither NaN"); return SPH_ERR_INVALID; }
    a.field[k] = t.field; a.lo[k] = t.lo; a.hi[k] = t.hi;
    if (t.field == 3 || t.field == SPH_SELECT_FIELD_SURFACE) a.needRow = 1;
    if (t.field == SPH_SELECT_FIELD_SURFACE) a.needMeasure = 1;
  }
  a.component = -1;
  if (component < -1) { sph_set_error("sph_select_particles: component %d is below -1", component); return SPH_ERR_INVALID; }
  if (component >= 0) {
    rc = sph_labels_current(s, "sph_select_particles", &a.labels);
    if (rc != SPH_OK) return rc;
    if ((int64_t)component >= s->ccCounts[1]) {
      sph_set_error("sph_select_particles: component %d is not in 0..%lld", component, (long long)s->ccCounts[1] - 1);
      return SPH_ERR_INVALID;
    }
    a.component = component;
  }
  rc = sph_grow_scratch(s, s->selBuf, sphk_select_scratch_bytes(s->d.N));
  if (rc != SPH_OK) return rc;
  uint32_t* dTotals = nullptr;
  rc = sphk_select_count(s, a, s->selBuf.p, &dTotals);
  if (rc != SPH_OK) return rc;
  uint32_t totals[2] = {0, 0};
  rc = sph_d2h(s, totals, dTotals, sizeof(totals));  // the call's one wait for a result
  if (rc != SPH_OK) return rc;
  if (totals[0] > (uint32_t)std::max(s->d.N, 0)) { sph_set_error("sph_select_particles: the count %u exceeds N", totals[0]); return SPH_ERR_HIP; }
  rc = sph_grow_scratch(s, s->selList, sizeof(int32_t) * (size_t)std::max<uint32_t>(totals[0], 1u));
  if (rc != SPH_OK) return rc;
  rc = sphk_select_scatter(s, s->selBuf.p, totals[0], (int32_t*)s->selList.p);
  if (rc != SPH_OK) return rc;
  rc = sph_check_finite_state(s);  // (synchronises the stream)
  if (rc != SPH_OK) return rc;
  s->selCount = (int64_t)totals[0];
  sph_derived_stamp(s, s->sel);
  *count = s->selCount;
  return SPH_OK;
}

extern "C" int sph_read_selection(sph_solver* s, int32_t* sortedIndex, uint32_t* origId, float* records) {
  ENTER(s);
  int rc = sph_selection_current(s, "sph_read_selection");
  if (rc != SPH_OK) return rc;
  const size_t n = (size_t)s->selCount;
  if (n == 0) return SPH_OK;
  const int32_t* list = (const int32_t*)s->selList.p;
  if (sortedIndex) rc = sph_d2h(s, sortedIndex, list, sizeof(int32_t) * n);
  if (rc != SPH_OK || (!origId && !records)) return rc;
  float ss2 = 0.f;
  rc = select_check(s, 0xEu, "sph_read_selection", &ss2);
  if (rc != SPH_OK) return rc;
  const size_t rec = sizeof(float) * SPH_SELECT_WORDS, per = rec + sizeof(uint32_t);
  const size_t piece = std::min<size_t>(n, kSampleScratchBytes / per);
  rc = sph_grow_scratch(s, s->sampleBuf, piece * per);
  if (rc != SPH_OK) return rc;
  float* dRec = (float*)s->sampleBuf.p;
  uint32_t* dIds = (uint32_t*)((char*)s->sampleBuf.p + piece * rec);
  for (size_t first = 0; first < n; first += piece) {
    const size_t m = std::min(piece, n - first);
    rc = sphk_select_gather(s, ss2, list + first, (int)m, dRec, dIds);
    if (rc != SPH_OK) return rc;
    if (records) rc = sph_d2h(s, records + first * SPH_SELECT_WORDS, dRec, rec * m);
    if (rc == SPH_OK && origId) rc = sph_d2h(s, origId + first, dIds, sizeof(uint32_t) * m);
    if (rc != SPH_OK) return rc;
  }
  return SPH_OK;
}

// ---------------------------------------------------------------------------------------------- elastic-matter diagnostics
// Spring strain per elastic particle, reductions per muscle group and membrane triangle areas (sph_elastic_measure.hip): the
// tables given to sph_create, evaluated on the sorted state of the last completed step. Blocking, read-only, no stage timing.
static int elastic_check(sph_solver* s, const char* what) {
  if (s->hasSlab) { sph_set_error("%s: a slab solver is not supported", what); return SPH_ERR_INVALID; }
  if (s->d.numElastic <= 0 || !s->d.elastic) { sph_set_error("%s: the solver holds no elastic matter", what); return SPH_ERR_INVALID; }
  NEED(s, P_DENSITY | P_PRESSUREFORCE, what);
  return SPH_OK;
}

static int elastic_bad_ids(uint32_t flags, const char* what) {
  if (!flags) return SPH_OK;
  sph_set_error("%s: a connection or membrane id lies outside 0..N-1 (flags 0x%x); it was not followed", what, flags);
  return SPH_ERR_INVALID;
}

extern "C" int sph_elastic_measure(sph_solver* s, int32_t* sortedIndex, uint32_t* origId, float* records, float* connections) {
  ENTER(s);
  int rc = elastic_check(s, "sph_elastic_measure");
  if (rc != SPH_OK) return rc;
  // [flags, 256 bytes][records][connections][sorted indices][original ids]; an output that is not asked for is not written
  const size_t E = (size_t)s->d.numElastic, head = 256;
  const size_t recBytes = sizeof(float) * SPH_ELASTIC_WORDS * E, conBytes = sizeof(float) * 2 * SPH_MAX_NEIGHBOR_COUNT * E;
  rc = sph_grow_scratch(s, s->elasticBuf, head + recBytes + conBytes + 2 * sizeof(uint32_t) * E);
  if (rc != SPH_OK) return rc;
  char* base = (char*)s->elasticBuf.p;
  uint32_t* dBad = (uint32_t*)base;
  float* dRec = (float*)(base + head);
  float* dCon = (float*)(base + head + recBytes);
  int32_t* dIdx = (int32_t*)(base + head + recBytes + conBytes);
  uint32_t* dIds = (uint32_t*)(dIdx + E);
  rc = sphk_elastic_measure(s, sortedIndex ? dIdx : nullptr, origId ? dIds : nullptr, records ? dRec : nullptr,
                            connections ? dCon : nullptr, dBad);
  if (rc != SPH_OK) return rc;
  // enqueued together, waited for once
  if (records) SPH_HIP(hipMemcpyAsync(records, dRec, recBytes, hipMemcpyDeviceToHost, s->stream));
  if (connections) SPH_HIP(hipMemcpyAsync(connections, dCon, conBytes, hipMemcpyDeviceToHost, s->stream));
  if (sortedIndex) SPH_HIP(hipMemcpyAsync(sortedIndex, dIdx, sizeof(int32_t) * E, hipMemcpyDeviceToHost, s->stream));
  if (origId) SPH_HIP(hipMemcpyAsync(origId, dIds, sizeof(uint32_t) * E, hipMemcpyDeviceToHost, s->stream));
  uint32_t flags = 0;
  rc = sph_d2h(s, &flags, dBad, sizeof(flags));
  if (rc != SPH_OK) return rc;
  rc = elastic_bad_ids(flags, "sph_elastic_measure");
  return rc != SPH_OK ? rc : sph_check_finite_state(s);
}

extern "C" int sph_muscle_diagnostics(sph_solver* s, double* out) {
  ENTER(s);
  if (!out) { sph_set_error("sph_muscle_diagnostics: null pointer"); return SPH_ERR_INVALID; }
  int rc = elastic_check(s, "sph_muscle_diagnostics");
  if (rc != SPH_OK) return rc;
  const int groups = s->d.muscleCount + 1;
  rc = sph_grow_scratch(s, s->elasticBuf, sizeof(double) * sphk_group_tree_doubles((long long)s->d.numElastic * SPH_MAX_NEIGHBOR_COUNT, groups));
  if (rc != SPH_OK) return rc;
  double* records = nullptr;
  rc = sphk_muscle_diagnostics(s, (double*)s->elasticBuf.p, &records);
  if (rc != SPH_OK) return rc;
  const size_t words = (size_t)groups * SPH_MUSCLE_WORDS;
  SPH_HIP(hipMemcpyAsync(out, records, sizeof(double) * words, hipMemcpyDeviceToHost, s->stream));
  double flags = 0.0;
  rc = sph_d2h(s, &flags, records + words, sizeof(flags));
  if (rc != SPH_OK) return rc;
  rc = elastic_bad_ids((uint32_t)flags, "sph_muscle_diagnostics");
  return rc != SPH_OK ? rc : sph_check_finite_state(s);
}

extern "C" int sph_membrane_measure(sph_solver* s, float* out, double totals[4]) {
  ENTER(s);
  if (!totals) { sph_set_error("sph_membrane_measure: null totals"); return SPH_ERR_INVALID; }
  int rc = elastic_check(s, "sph_membrane_measure");
  if (rc != SPH_OK) return rc;
  const size_t M = (size_t)std::max(s->d.numMembranes, 0);
  if (M == 0 || !s->d.membraneData) { sph_set_error("sph_membrane_measure: the solver holds no membranes"); return SPH_ERR_INVALID; }
  // [records, 32 bytes per triangle][the tree's levels and flags]
  const size_t recBytes = sizeof(float) * SPH_MEMBRANE_WORDS * M;
  rc = sph_grow_scratch(s, s->elasticBuf, recBytes + sizeof(double) * sphk_group_tree_doubles((long long)M, 1));
  if (rc != SPH_OK) return rc;
  float* dRec = (float*)s->elasticBuf.p;
  double* top = nullptr;
  rc = sphk_membrane_measure(s, out ? dRec : nullptr, (double*)((char*)s->elasticBuf.p + recBytes), &top);
  if (rc != SPH_OK) return rc;
  if (out) SPH_HIP(hipMemcpyAsync(out, dRec, recBytes, hipMemcpyDeviceToHost, s->stream));
  double t[SPH_MUSCLE_WORDS + 1];
  rc = sph_d2h(s, t, top, sizeof(t));
  if (rc != SPH_OK) return rc;
  uint32_t flags = 0;
  memcpy(&flags, &t[SPH_MUSCLE_WORDS], sizeof(flags));
  rc = elastic_bad_ids(flags, "sph_membrane_measure");
  if (rc != SPH_OK) return rc;
  volatile float mn = (float)t[7] + 0.0f, mx = (float)t[8] + 0.0f;  // the extremes' canonical form, as the diagnostics'
  totals[0] = t[0]; totals[1] = t[2];
  totals[2] = t[0] > 0.0 ? (double)mn : 0.0;
  totals[3] = t[0] > 0.0 ? (double)mx : 0.0;
  return sph_check_finite_state(s);
}

// ---------------------------------------------------------------------------------------------- force decomposition
// The K7 and K12 accelerations by the class of the neighbour that exerted them (sph_forces.hip): per particle in pieces through
// the sampling scratch, and as region totals through the diagnostics scratch. Blocking, read-only, no stage timing.
static int force_check(sph_solver* s, uint32_t typeMask, const char* what) {
  const int rc = sph_sample_check(s, typeMask, what);
  if (rc != SPH_OK) return rc;
  NEED(s, P_FIND | P_FORCES, what);  // the rows, and the gather records K7 packs
  return SPH_OK;
}

// The two piece loops of the force decomposition and the wall loads.
// n particles, or the selection list, in pieces of whole blocks through the sampling scratch: records(first, m, list, dst)
// enqueues the records of `words` floats of a piece, which are then copied out
template <class Records>
static int measure_records(sph_solver* s, size_t n, const int32_t* list, size_t words, float* out, Records records) {
  const size_t rec = sizeof(float) * words;
  const size_t piece = std::min((n + SPH_BLOCK - 1) / SPH_BLOCK * SPH_BLOCK, kSampleScratchBytes / rec / SPH_BLOCK * SPH_BLOCK);
  int rc = sph_grow_scratch(s, s->sampleBuf, piece * rec);
  if (rc != SPH_OK) return rc;
  for (size_t first = 0; first < n; first += piece) {
    const size_t m = std::min(piece, n - first);
    rc = records((int)first, (int)m, list ? list + first : nullptr, (float*)s->sampleBuf.p);
    if (rc != SPH_OK) return rc;
    rc = sph_d2h(s, out + first * words, s->sampleBuf.p, rec * m);
    if (rc != SPH_OK) return rc;
  }
  return sph_check_finite_state(s);
}

// Region totals: the `terms` per-particle terms of a piece of whole chunks in the sampling scratch, the tree's partials in the
// diagnostics scratch; run(terms, pieceChunks, scratch, &records) enqueues the call, whose count x words doubles are copied out
template <class Run>
static int region_totals(sph_solver* s, int terms, int words, int32_t count, double* out, Run run) {
  const int pieceChunks = (int)std::min<size_t>((size_t)tree_chunks(s->d.N), kSampleScratchBytes / terms_bytes(terms, 1));
  int rc = sph_grow_scratch(s, s->sampleBuf, terms_bytes(terms, pieceChunks));
  if (rc != SPH_OK) return rc;
  rc = sph_grow_scratch(s, s->diagBuf, sizeof(double) * tree_scratch_doubles(s->d.N, count, words));
  if (rc != SPH_OK) return rc;
  double* records = nullptr;
  rc = run((float*)s->sampleBuf.p, pieceChunks, (double*)s->diagBuf.p, &records);
  if (rc != SPH_OK) return rc;
  rc = sph_d2h(s, out, records, sizeof(double) * (size_t)words * (size_t)count);
  return rc != SPH_OK ? rc : sph_check_finite_state(s);
}

extern "C" int sph_force_measure(sph_solver* s, int32_t fromSelection, float* out) {
  ENTER(s);
  if (fromSelection != 0 && fromSelection != 1) { sph_set_error("sph_force_measure: fromSelection %d is not 0 or 1", fromSelection); return SPH_ERR_INVALID; }
  size_t n = (size_t)std::max(s->d.N, 0);
  const int32_t* list = nullptr;
  if (fromSelection) {
    const int rcSel = sph_selection_current(s, "sph_force_measure");
    if (rcSel != SPH_OK) return rcSel;
    n = (size_t)s->selCount;
    list = (const int32_t*)s->selList.p;
  }
  int rc = force_check(s, 0xEu, "sph_force_measure");
  if (rc != SPH_OK) return rc;
  if (n == 0) return sph_check_finite_state(s);
  if (!out) { sph_set_error("sph_force_measure: null pointer"); return SPH_ERR_INVALID; }
  return measure_records(s, n, list, SPH_FORCE_WORDS, out,
                         [&](int first, int m, const int32_t* l, float* dst) { return sphk_force_records(s, first, m, l, dst); });
}

extern "C" int sph_force_diagnostics(sph_solver* s, const float* regions6, int32_t count, uint32_t typeMask, double* out) {
  ENTER(s);
  if (!regions6 || !out) { sph_set_error("sph_force_diagnostics: null pointer"); return SPH_ERR_INVALID; }
  if (count < 1 || count > SPH_DIAG_MAX_REGIONS) { sph_set_error("sph_force_diagnostics: count %d is not in 1..%d", count, SPH_DIAG_MAX_REGIONS); return SPH_ERR_INVALID; }
  int rc = force_check(s, typeMask, "sph_force_diagnostics");
  if (rc != SPH_OK) return rc;
  DiagArgs a = {};
  rc = diag_fill_regions(s, &a, regions6, count, typeMask, "sph_force_diagnostics");
  if (rc != SPH_OK) return rc;
  return region_totals(s, FM_TERMS, SPH_FORCE_DIAG_WORDS, count, out, [&](float* terms, int pieceChunks, double* scratch, double** records) {
    return sphk_force_diagnostics(s, a, terms, pieceChunks, scratch, records);
  });
}

// ---------------------------------------------------------------------------------------------- wall loads
// What a set of boundary particles did to each particle in integrate, K7 and K12 (sph_wall.hip): the rules and the two piece
// loops of the force decomposition, and in front of them the call's wall set as a bit mask over sorted indices.
static int wall_check(sph_solver* s, int32_t slot, uint32_t typeMask, const char* what) {
  const int rc = force_check(s, typeMask, what);
  if (rc != SPH_OK) return rc;
  if (slot != SPH_WALL_ALL && slot != SPH_WALL_NO_BODY && (slot < 0 || slot >= SPH_MAX_BODIES)) {
    sph_set_error("%s: slot %d is not in 0..%d, SPH_WALL_ALL or SPH_WALL_NO_BODY", what, slot, SPH_MAX_BODIES - 1);
    return SPH_ERR_INVALID;
  }
  NEED(s, P_INTEGRATE, what);  // acceleration and the boundary masks are what the step's integrate read
  if (slot >= 0 && !s->bodyCount[slot]) { sph_set_error("%s: slot %d holds no body (sph_body_define_ids / sph_body_define_region)", what, slot); return SPH_ERR_ORDER; }
  return SPH_OK;
}

// *mask: the set's bits (null: every boundary particle), *inverted: the set is the particles whose bit is clear
static int wall_set(sph_solver* s, int32_t slot, const uint32_t** mask, bool* inverted) {
  *mask = nullptr; *inverted = false;
  if (slot == SPH_WALL_ALL) return SPH_OK;
  int rc = sph_grow_scratch(s, s->wallBuf, sphk_wall_mask_bytes(s->d.N));
  if (rc != SPH_OK) return rc;
  uint32_t* m = (uint32_t*)s->wallBuf.p;
  rc = sphk_wall_mask_clear(s, m);
  for (int32_t b = 0; b < SPH_MAX_BODIES && rc == SPH_OK; b++)
    if (slot == SPH_WALL_NO_BODY || slot == b) rc = sphk_wall_mask_add(s, (const uint32_t*)s->bodyIds[b].p, s->bodyCount[b], m);
  *mask = m; *inverted = slot == SPH_WALL_NO_BODY;
  return rc;
}

extern "C" int sph_wall_measure(sph_solver* s, int32_t slot, int32_t fromSelection, float* out) {
  ENTER(s);
  if (fromSelection != 0 && fromSelection != 1) { sph_set_error("sph_wall_measure: fromSelection %d is not 0 or 1", fromSelection); return SPH_ERR_INVALID; }
  int rc = wall_check(s, slot, 0xEu, "sph_wall_measure");
  if (rc != SPH_OK) return rc;
  size_t n = (size_t)std::max(s->d.N, 0);
  const int32_t* list = nullptr;
  if (fromSelection) {
    rc = sph_selection_current(s, "sph_wall_measure");
    if (rc != SPH_OK) return rc;
    n = (size_t)s->selCount;
    list = (const int32_t*)s->selList.p;
  }
  if (n == 0) return sph_check_finite_state(s);
  if (!out) { sph_set_error("sph_wall_measure: null pointer"); return SPH_ERR_INVALID; }
  const uint32_t* mask = nullptr;
  bool inverted = false;
  rc = wall_set(s, slot, &mask, &inverted);
  if (rc != SPH_OK) return rc;
  return measure_records(s, n, list, SPH_WALL_WORDS, out, [&](int first, int m, const int32_t* l, float* dst) {
    return sphk_wall_records(s, mask, inverted, first, m, l, dst);
  });
}

extern "C" int sph_wall_diagnostics(sph_solver* s, int32_t slot, const float* regions6, int32_t count, uint32_t typeMask, double* out) {
  ENTER(s);
  if (!regions6 || !out) { sph_set_error("sph_wall_diagnostics: null pointer"); return SPH_ERR_INVALID; }
  if (count < 1 || count > SPH_DIAG_MAX_REGIONS) { sph_set_error("sph_wall_diagnostics: count %d is not in 1..%d", count, SPH_DIAG_MAX_REGIONS); return SPH_ERR_INVALID; }
  int rc = wall_check(s, slot, typeMask, "sph_wall_diagnostics");
  if (rc != SPH_OK) return rc;
  DiagArgs a = {};
  rc = diag_fill_regions(s, &a, regions6, count, typeMask, "sph_wall_diagnostics");
  if (rc != SPH_OK) return rc;
  const uint32_t* mask = nullptr;
  bool inverted = false;
  rc = wall_set(s, slot, &mask, &inverted);
  if (rc != SPH_OK) return rc;
  return region_totals(s, WL_TERMS, SPH_WALL_DIAG_WORDS, count, out, [&](float* terms, int pieceChunks, double* scratch, double** records) {
    return sphk_wall_diagnostics(s, mask, inverted, a, terms, pieceChunks, scratch, records);
  });
}

// ---------------------------------------------------------------------------------------------- free bodies
// One step of every dynamic body (sph_body_dynamics.hip) under the order rules of the wall loads, whose state it reads. With
// out == NULL nothing here waits for the device.
extern "C" int sph_bodies_advance(sph_solver* s, double* out) {
  ENTER(s);
  int rc = wall_check(s, SPH_WALL_ALL, 0xEu, "sph_bodies_advance");
  if (rc != SPH_OK) return rc;
  if (s->stepOpen) { sph_set_error("sph_bodies_advance: a stage-by-stage step is half done; bodies are moved between two steps"); return SPH_ERR_ORDER; }
  const BodyDynSet set = sph_body_dyn_set(s);
  if (!set.dynMask) {
    if (out)
      for (int k = 0; k < SPH_MAX_BODIES * SPH_BODY_STATE_WORDS; k++) out[k] = k % SPH_BODY_STATE_WORDS == 0 ? -1.0 : 0.0;
    return SPH_OK;
  }
  rc = sph_grow_scratch(s, s->bodyDynScratch, sphk_bdyn_scratch_bytes(s->d.N));
  if (rc != SPH_OK) return rc;
  BodyDynDev* D = (BodyDynDev*)s->bodyDynBuf.p;  // (exists: sph_body_set_dynamics made the bodies dynamic)
  rc = sphk_bdyn_advance(s, set, sph_body_pose_box(s), s->bodyDynScratch.p, D);
  if (rc != SPH_OK || !out) return rc;
  return sph_d2h(s, out, D->record, sizeof(double) * SPH_MAX_BODIES * SPH_BODY_STATE_WORDS);
}

// ---------------------------------------------------------------------------------------------- integral curves
// Streamlines and tracers (sph_trace.hip): the rules of sampling, the step's parameters checked here. Streamlines go through the
// sampling scratch in pieces of seeds, [vertices][seeds][lengths][status] each; the tracers live in a buffer of their own.
static int trace_check(sph_solver* s, uint32_t typeMask, const sph_trace_params* p, const float* region6, bool curves,
                       const char* what, SampleArgs* a, TraceArgs* t) {
  if (!p) { sph_set_error("%s: null params", what); return SPH_ERR_INVALID; }
  const int rc = sph_sample_check(s, typeMask, what, a);
  if (rc != SPH_OK) return rc;
  if (!std::isfinite(p->step) || p->step == 0.f) { sph_set_error("%s: step must be finite and not 0", what); return SPH_ERR_INVALID; }
  if (!(p->minSpeed >= 0.f)) { sph_set_error("%s: minSpeed must be >= 0", what); return SPH_ERR_INVALID; }
  if (curves && (p->maxSteps < 0 || p->maxSteps > SPH_TRACE_MAX_STEPS_LIMIT)) {
    sph_set_error("%s: maxSteps %d is not in 0..%d", what, p->maxSteps, SPH_TRACE_MAX_STEPS_LIMIT);
    return SPH_ERR_INVALID;
  }
  if (p->mode != SPH_TRACE_TIME && p->mode != SPH_TRACE_ARC) { sph_set_error("%s: mode %d is not 0 or 1", what, p->mode); return SPH_ERR_INVALID; }
  if (p->integrator != SPH_TRACE_EULER && p->integrator != SPH_TRACE_MIDPOINT) {
    sph_set_error("%s: integrator %d is not 0 or 1", what, p->integrator);
    return SPH_ERR_INVALID;
  }
  *t = TraceArgs{};
  t->step = p->step; t->minSpeed = p->minSpeed; t->maxSteps = curves ? p->maxSteps : 0; t->mode = p->mode; t->integrator = p->integrator;
  t->hasRegion = region6 != nullptr;
  return region_fill(t->box, region6, what);
}

extern "C" int sph_trace_streamlines(sph_solver* s, const float* seeds4, int32_t count, uint32_t typeMask, const sph_trace_params* params,
                                     const float* region6, float* vertices, int32_t* lengths, int32_t* status) {
  ENTER(s);
  const char* what = "sph_trace_streamlines";
  if (count < 0 || (count > 0 && (!seeds4 || !vertices || !lengths || !status))) { sph_set_error("%s: bad count or null pointer", what); return SPH_ERR_INVALID; }
  SampleArgs a;
  TraceArgs t;
  int rc = trace_check(s, typeMask, params, region6, true, what, &a, &t);
  if (rc != SPH_OK || count == 0) return rc;
  const size_t curve = sizeof(float4) * (size_t)(t.maxSteps + 1), perSeed = curve + sizeof(float4) + 2 * sizeof(int32_t);
  const int piece = (int)std::min<size_t>((size_t)count, kSampleScratchBytes / perSeed);  // >= 63: a curve is at most 1 MiB
  rc = sph_grow_scratch(s, s->sampleBuf, (size_t)piece * perSeed);
  if (rc != SPH_OK) return rc;
  char* base = (char*)s->sampleBuf.p;
  float* dVerts = (float*)base;
  float* dSeeds = (float*)(base + (size_t)piece * curve);
  int32_t* dLen = (int32_t*)(base + (size_t)piece * (curve + sizeof(float4)));
  int32_t* dStatus = dLen + piece;
  for (int first = 0; first < count; first += piece) {
    const int n = std::min(piece, count - first);
    SPH_HIP(hipMemcpyAsync(dSeeds, seeds4 + (size_t)first * 4, sizeof(float4) * (size_t)n, hipMemcpyHostToDevice, s->stream));
    SPH_HIP(hipMemsetAsync(dVerts, 0, curve * (size_t)n, s->stream));  // the slots behind a curve's last vertex
    rc = sphk_trace_streamlines(s, a, t, dSeeds, n, dVerts, dLen, dStatus);
    if (rc != SPH_OK) return rc;
    // enqueued together, waited for once
    SPH_HIP(hipMemcpyAsync(vertices + (size_t)first * 4 * (size_t)(t.maxSteps + 1), dVerts, curve * (size_t)n, hipMemcpyDeviceToHost, s->stream));
    SPH_HIP(hipMemcpyAsync(lengths + first, dLen, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost, s->stream));
    rc = sph_d2h(s, status + first, dStatus, sizeof(int32_t) * (size_t)n);
    if (rc != SPH_OK) return rc;
  }
  return SPH_OK;
}

static const size_t kTracerHead = 256;  // the advect's counter in front of the tracers
static float* tracer_pos(const sph_solver* s) { return (float*)((char*)s->tracerBuf.p + kTracerHead); }
static int32_t* tracer_status(const sph_solver* s) { return (int32_t*)((char*)s->tracerBuf.p + kTracerHead + sizeof(float4) * (size_t)s->tracerCount); }

extern "C" int sph_tracers_set(sph_solver* s, const float* points4, int32_t count) {
  ENTER(s);
  if (count < 0 || (count > 0 && !points4)) { sph_set_error("sph_tracers_set: bad count or null pointer"); return SPH_ERR_INVALID; }
  s->tracerCount = 0;
  if (count == 0) {
    if (s->tracerBuf.p) { SPH_HIP(hipStreamSynchronize(s->stream)); hipFree(s->tracerBuf.p); }
    s->tracerBuf.p = nullptr; s->tracerBuf.bytes = 0;
    return SPH_OK;
  }
  const size_t n = (size_t)count;
  int rc = sph_grow_scratch(s, s->tracerBuf, kTracerHead + n * (sizeof(float4) + 2 * sizeof(int32_t)));
  if (rc != SPH_OK) return rc;
  std::vector<float> p4(points4, points4 + 4 * n);
  for (size_t i = 0; i < n; i++) p4[4 * i + 3] = 0.f;  // no sample yet
  s->tracerCount = count;
  SPH_HIP(hipMemcpyAsync(tracer_pos(s), p4.data(), sizeof(float4) * n, hipMemcpyHostToDevice, s->stream));
  SPH_HIP(hipMemsetAsync(tracer_status(s), 0, 2 * sizeof(int32_t) * n, s->stream));  // SPH_TRACE_MOVING, 0 steps
  SPH_HIP(hipStreamSynchronize(s->stream));  // (p4 is read until then)
  return SPH_OK;
}

static int tracers_exist(const sph_solver* s, const char* what) {
  if (s->tracerCount > 0) return SPH_OK;
  sph_set_error("%s: no tracers have been set (sph_tracers_set)", what);
  return SPH_ERR_ORDER;
}

extern "C" int sph_tracers_advect(sph_solver* s, uint32_t typeMask, const sph_trace_params* params, const float* region6, int64_t counts[2]) {
  ENTER(s);
  const char* what = "sph_tracers_advect";
  if (counts) counts[0] = counts[1] = 0;
  if (!counts) { sph_set_error("%s: null counts", what); return SPH_ERR_INVALID; }
  SampleArgs a;
  TraceArgs t;
  int rc = trace_check(s, typeMask, params, region6, false, what, &a, &t);
  if (rc != SPH_OK) return rc;
  rc = tracers_exist(s, what);
  if (rc != SPH_OK) return rc;
  uint32_t* dMoving = (uint32_t*)s->tracerBuf.p;
  SPH_HIP(hipMemsetAsync(dMoving, 0, sizeof(uint32_t), s->stream));
  int32_t* st = tracer_status(s);
  rc = sphk_tracers_advect(s, a, t, tracer_pos(s), st, st + s->tracerCount, s->tracerCount, dMoving);
  if (rc != SPH_OK) return rc;
  uint32_t moving = 0;
  rc = sph_d2h(s, &moving, dMoving, sizeof(moving));
  if (rc != SPH_OK) return rc;
  counts[0] = (int64_t)moving;
  counts[1] = (int64_t)s->tracerCount - (int64_t)moving;
  return SPH_OK;
}

extern "C" int sph_tracers_read(sph_solver* s, float* pos4, int32_t* status, int32_t* steps) {
  ENTER(s);
  const int rc = tracers_exist(s, "sph_tracers_read");
  if (rc != SPH_OK) return rc;
  const size_t n = (size_t)s->tracerCount;
  const int32_t* st = tracer_status(s);
  // enqueued together, waited for once
  if (pos4) SPH_HIP(hipMemcpyAsync(pos4, tracer_pos(s), sizeof(float4) * n, hipMemcpyDeviceToHost, s->stream));
  if (status) SPH_HIP(hipMemcpyAsync(status, st, sizeof(int32_t) * n, hipMemcpyDeviceToHost, s->stream));
  if (steps) SPH_HIP(hipMemcpyAsync(steps, st + n, sizeof(int32_t) * n, hipMemcpyDeviceToHost, s->stream));
  SPH_HIP(hipStreamSynchronize(s->stream));
  return SPH_OK;
}

// ---------------------------------------------------------------------------------------------- particle rendering
// Images of the particles (sph_render.hip): clear, splat, drain and resolve are enqueued together and waited for once, for the
// two counts. The images stay in renderBuf and hold everything sph_read_render returns, so they outlive the state they show.
static bool render_view_ok(const sph_render_view& v) {
  const float* f[] = {v.eye, v.right, v.up, v.forward};
  for (const float* a : f)
    for (int k = 0; k < 3; k++)
      if (!std::isfinite(a[k])) { sph_set_error("sph_render_particles: eye, right, up and forward must be finite"); return false; }
  if (v.width < 1 || v.width > 8192 || v.height < 1 || v.height > 8192 || (int64_t)v.width * v.height > ((int64_t)1 << 24)) {
    sph_set_error("sph_render_particles: width and height must be in 1..8192 with width*height <= 1<<24"); return false;
  }
  if (v.projection != 0 && v.projection != 1) { sph_set_error("sph_render_particles: projection %d is not 0 or 1", v.projection); return false; }
  if (!std::isfinite(v.scale) || !(v.scale > 0.f)) { sph_set_error("sph_render_particles: scale must be finite and > 0"); return false; }
  if (!std::isfinite(v.centre[0]) || !std::isfinite(v.centre[1])) { sph_set_error("sph_render_particles: centre must be finite"); return false; }
  if (!std::isfinite(v.nearPlane) || !(v.nearPlane >= 0.f)) { sph_set_error("sph_render_particles: nearPlane must be finite and >= 0"); return false; }
  if (!std::isfinite(v.radius) || !(v.radius > 0.f)) { sph_set_error("sph_render_particles: radius must be finite and > 0"); return false; }
  if (!(v.maxRadiusPx > 0.f && v.maxRadiusPx <= 4096.f)) { sph_set_error("sph_render_particles: maxRadiusPx must be in (0, 4096]"); return false; }
  if (v.colourMode < 0 || v.colourMode > 3) { sph_set_error("sph_render_particles: colourMode %d is not in 0..3", v.colourMode); return false; }
  if (v.colourMode == 2) {
    if (v.field < 0 || v.field > 6) { sph_set_error("sph_render_particles: field %d is not in 0..6", v.field); return false; }
    if (!std::isfinite(v.lo) || !std::isfinite(v.hi) || !(v.lo < v.hi)) { sph_set_error("sph_render_particles: lo and hi must be finite with lo < hi"); return false; }
  }
  if (v.colourMode == 0)
    for (int t = 0; t < 3; t++)
      for (int k = 0; k < 3; k++)
        if (!std::isfinite(v.typeColour[t][k])) { sph_set_error("sph_render_particles: typeColour must be finite"); return false; }
  if (!(v.ambient >= 0.f && v.ambient <= 1.f)) { sph_set_error("sph_render_particles: ambient must be in 0..1"); return false; }
  return true;
}

extern "C" int sph_render_particles(sph_solver* s, const sph_render_view* view, const float* region6, uint32_t typeMask,
                                    int32_t wantThickness, int64_t counts[2]) {
  ENTER(s);
  sph_derived_drop(s->render);
  s->renderHasMesh = false;
  if (counts) counts[0] = counts[1] = 0;
  if (!view || !counts) { sph_set_error("sph_render_particles: null pointer"); return SPH_ERR_INVALID; }
  int rc = sph_sample_check(s, typeMask, "sph_render_particles");
  if (rc != SPH_OK) return rc;
  if (!render_view_ok(*view)) return SPH_ERR_INVALID;
  RenderArgs a = {};
  a.view = *view;
  rc = sph_fill_selector(&a.sel, region6, typeMask, "sph_render_particles");
  if (rc != SPH_OK) return rc;
  if (view->colourMode == 2) {
    if (view->field == 3) NEED(s, P_FIND, "sph_render_particles (field 3)");
    volatile float width = view->hi - view->lo;
    volatile float inv = 1.0f / width;
    a.inv = inv;
  }
  if (view->colourMode == 3) {
    rc = sph_labels_current(s, "sph_render_particles", &a.labels);
    if (rc != SPH_OK) return rc;
  }
  const bool thickness = wantThickness != 0;
  const RenderLayout L = sphk_render_layout(view->width, view->height, thickness, s->d.N);
  rc = sph_grow_scratch(s, s->renderBuf, L.bytes);
  if (rc != SPH_OK) return rc;
  rc = sphk_render(s, a, thickness, s->renderBuf.p);
  if (rc != SPH_OK) return rc;
  uint32_t head[2] = {0, 0};
  rc = sph_d2h(s, head, (char*)s->renderBuf.p + L.head, sizeof(head));  // the call's one wait for a result
  if (rc != SPH_OK) return rc;
  rc = sph_check_finite_state(s);
  if (rc != SPH_OK) return rc;
  s->renderW = view->width; s->renderH = view->height;
  s->renderThickness = thickness;
  s->renderView = *view;
  sph_derived_stamp(s, s->render);
  counts[0] = (int64_t)head[0];
  counts[1] = (int64_t)head[1];
  return SPH_OK;
}

extern "C" int sph_read_render(sph_solver* s, float* depth, int32_t* sortedIndex, uint32_t* origId, uint8_t* rgba, uint32_t* thickness) {
  ENTER(s);
  const int rc = sph_derived_check(s, s->render, "sph_read_render", "nothing has been rendered", nullptr);
  if (rc != SPH_OK) return rc;
  if (thickness && !s->renderThickness) { sph_set_error("sph_read_render: the last render accumulated no thickness"); return SPH_ERR_INVALID; }
  const RenderLayout L = sphk_render_layout(s->renderW, s->renderH, s->renderThickness, s->render.N);
  const size_t words = sizeof(uint32_t) * (size_t)s->renderW * (size_t)s->renderH;
  const char* base = (const char*)s->renderBuf.p;
  // enqueued together, waited for once
  if (depth) SPH_HIP(hipMemcpyAsync(depth, base + L.depth, words, hipMemcpyDeviceToHost, s->stream));
  if (sortedIndex) SPH_HIP(hipMemcpyAsync(sortedIndex, base + L.index, words, hipMemcpyDeviceToHost, s->stream));
  if (origId) SPH_HIP(hipMemcpyAsync(origId, base + L.origId, words, hipMemcpyDeviceToHost, s->stream));
  if (rgba) SPH_HIP(hipMemcpyAsync(rgba, base + L.rgba, words, hipMemcpyDeviceToHost, s->stream));
  if (thickness) SPH_HIP(hipMemcpyAsync(thickness, base + L.thickOut, words, hipMemcpyDeviceToHost, s->stream));
  SPH_HIP(hipStreamSynchronize(s->stream));
  return SPH_OK;
}

// ---------------------------------------------------------------------------------------------- triangle rendering
// The mesh of the last extraction or the membrane triangles into the same images (sph_render_mesh.hip), fresh or composed over the
// last render by depth. Normals and vertex scalars come from the gradient and sampling kernels on the device; everything is
// enqueued together and waited for once, for the counts.
extern "C" int sph_render_mesh(sph_solver* s, const sph_render_view* view, const sph_render_mesh_style* style, int64_t counts[4]) {
  ENTER(s);
  const char* what = "sph_render_mesh";
  if (counts) counts[0] = counts[1] = counts[2] = counts[3] = 0;
  if (!view || !style || !counts) { sph_set_error("%s: null pointer", what); return SPH_ERR_INVALID; }
  const sph_render_mesh_style& y = *style;
  if (y.compose != 0 && y.compose != 1) { sph_set_error("%s: compose %d is not 0 or 1", what, y.compose); return SPH_ERR_INVALID; }
  if (!y.compose) {  // a fresh image: a failed call leaves none behind
    sph_derived_drop(s->render);
    s->renderHasMesh = false;
  }
  int rc = sph_sample_check(s, 0xEu, what);
  if (rc != SPH_OK) return rc;
  if (!render_view_ok(*view)) return SPH_ERR_INVALID;
  if (y.source != 0 && y.source != 1) { sph_set_error("%s: source %d is not 0 or 1", what, y.source); return SPH_ERR_INVALID; }
  if (y.shading != 0 && y.shading != 1) { sph_set_error("%s: shading %d is not 0 or 1", what, y.shading); return SPH_ERR_INVALID; }
  if (y.colourMode != 0 && y.colourMode != 1) { sph_set_error("%s: colourMode %d is not 0 or 1", what, y.colourMode); return SPH_ERR_INVALID; }
  if (y.shading == 1 && y.source == 1) { sph_set_error("%s: smooth shading needs the surface mesh (source 0)", what); return SPH_ERR_INVALID; }
  RenderMeshArgs a = {};
  if (y.colourMode == 1) {
    if (y.field < 0 || y.field > 6) { sph_set_error("%s: field %d is not in 0..6", what, y.field); return SPH_ERR_INVALID; }
    if (!std::isfinite(y.lo) || !std::isfinite(y.hi) || !(y.lo < y.hi)) { sph_set_error("%s: lo and hi must be finite with lo < hi", what); return SPH_ERR_INVALID; }
    volatile float width = y.hi - y.lo;
    volatile float inv = 1.0f / width;
    a.inv = inv;
  } else {
    for (int k = 0; k < 3; k++)
      if (!std::isfinite(y.colour[k])) { sph_set_error("%s: colour must be finite", what); return SPH_ERR_INVALID; }
  }
  int64_t V = 0, T = 0;
  if (y.source == 1) {
    if (s->d.numMembranes <= 0 || !s->d.membraneData) { sph_set_error("%s: the solver holds no membranes", what); return SPH_ERR_INVALID; }
    T = s->d.numMembranes; V = 3 * T;
    if (y.colourMode == 1 && y.field == 3) NEED(s, P_FIND, "sph_render_mesh (field 3)");
  } else {
    const bool live = y.shading == 1 || y.colourMode == 1;  // these read the state at the vertices
    rc = sph_derived_check(s, s->mesh, what, "no surface has been extracted",
                           live ? "the solver's state has changed since the surface was extracted (flat shading with a constant colour draws a stale mesh)" : nullptr);
    if (rc != SPH_OK) return rc;
    V = s->meshCounts[0]; T = s->meshCounts[1];
  }
  if (V > 0x7fffffffLL || T > 0x7fffffffLL) { sph_set_error("%s: more than 2^31-1 vertices or triangles", what); return SPH_ERR_SIZE; }
  RenderLayout I;
  if (y.compose) {
    rc = sph_derived_check(s, s->render, what, "compose needs the images of a successful render", nullptr);
    if (rc != SPH_OK) return rc;
    if (memcmp(view, &s->renderView, offsetof(sph_render_view, radius)) != 0) {
      sph_set_error("%s: compose needs the last render's width .. nearPlane, byte for byte", what);
      return SPH_ERR_INVALID;
    }
    I = sphk_render_layout(s->renderW, s->renderH, s->renderThickness, s->render.N);
  } else {
    I = sphk_render_layout(view->width, view->height, false, s->d.N);
    rc = sph_grow_scratch(s, s->renderBuf, I.bytes);
    if (rc != SPH_OK) return rc;
  }
  a.view = *view;
  a.source = y.source; a.shading = y.shading; a.colourMode = y.colourMode; a.field = y.field; a.compose = y.compose;
  a.lo = y.lo;
  for (int k = 0; k < 3; k++) a.colour[k] = y.colour[k];
  a.V = (int)V; a.T = (int)T;
  const bool normals = y.shading == 1, samples = y.source == 0 && y.colourMode == 1;
  const RenderMeshLayout L = sphk_render_mesh_layout(V, T, normals, samples);
  rc = sph_grow_scratch(s, s->renderMeshBuf, L.bytes);
  if (rc != SPH_OK) return rc;
  rc = sph_grow_scratch(s, s->renderTriBuf, sizeof(int32_t) * (size_t)view->width * (size_t)view->height);
  if (rc != SPH_OK) return rc;
  char* base = (char*)s->renderMeshBuf.p;
  const float* verts = nullptr;
  const int32_t* tris = nullptr;
  if (y.source == 0) {
    verts = (const float*)s->meshBuf.p;
    tris = (const int32_t*)((const char*)s->meshBuf.p + surf_bytes_align(sizeof(float) * 3 * (size_t)V));
    if ((normals || samples) && V > 0) {
      SampleArgs sa;
      rc = sph_sample_check(s, s->meshTypeMask, what, &sa);
      if (rc != SPH_OK) return rc;
      if (normals) rc = sphk_surface_normals(s, sa, gradient_scale(s), s->meshField, verts, (int)V, (float*)(base + L.normals));
      if (rc != SPH_OK) return rc;
      if (samples) {
        rc = sphk_render_mesh_points(s, (int)V, verts, (float*)(base + L.points));
        if (rc != SPH_OK) return rc;
        rc = sphk_sample_points(s, sa, (const float*)(base + L.points), (int)V, (float*)(base + L.records));
        if (rc != SPH_OK) return rc;
      }
    }
  }
  rc = sphk_render_mesh(s, a, verts, tris, base, L, I, s->renderBuf.p, (int32_t*)s->renderTriBuf.p);
  if (rc != SPH_OK) return rc;
  uint32_t head[6] = {};
  rc = sph_d2h(s, head, base + L.head, sizeof(head));  // the call's one wait for a result
  if (rc != SPH_OK) return rc;
  if (head[3]) {
    sph_set_error("%s: a membrane id lies outside 0..N-1 (flags 0x%x); it was not followed and nothing was drawn", what, head[3]);
    return SPH_ERR_INVALID;
  }
  rc = sph_check_finite_state(s);
  if (rc != SPH_OK) return rc;
  if (!y.compose) {
    s->renderW = view->width; s->renderH = view->height;
    s->renderThickness = false;
    s->renderView = *view;
    sph_derived_stamp(s, s->render);
  }
  s->renderHasMesh = true;
  counts[0] = (int64_t)head[0];
  counts[1] = (int64_t)head[1];
  counts[2] = (int64_t)head[4];
  counts[3] = (int64_t)head[5];
  return SPH_OK;
}

extern "C" int sph_read_render_triangles(sph_solver* s, int32_t* triangle) {
  ENTER(s);
  const int rc = sph_derived_check(s, s->render, "sph_read_render_triangles", "nothing has been rendered", nullptr);
  if (rc != SPH_OK) return rc;
  if (!s->renderHasMesh) { sph_set_error("sph_read_render_triangles: the last render had no mesh pass"); return SPH_ERR_ORDER; }
  if (!triangle) { sph_set_error("sph_read_render_triangles: null pointer"); return SPH_ERR_INVALID; }
  return sph_d2h(s, triangle, s->renderTriBuf.p, sizeof(int32_t) * (size_t)s->renderW * (size_t)s->renderH);
}

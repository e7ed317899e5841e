// C ABI of libsphmi.so (include/sphmi.h), the probes: sph_probes_set_points / sph_probes_set_lines / sph_probes_count /
// sph_probes_record / sph_probes_history / sph_probes_read_history. Probes are passive and belong to the solver, as
// tracers do: no call here says sph_state_changes or touches `progress`, and every buffer is the feature's own. What the
// translation units of the ABI share is in sph_api_internal.h.
#include <algorithm>
#include <cmath>

#include "sph_api_internal.h"

static const size_t kProbeRecord = sizeof(float) * SPH_PROBE_LEVEL_WORDS;  // bytes of a point record and of a line record
static const size_t kProbeRingBytes = (size_t)1 << 28;

// What every probe call checks first: no slab solver (SPH_ERR_INVALID).
static int probe_check(sph_solver* s, const char* what) {
  if (s->hasSlab) { sph_set_error("%s: a slab solver is not supported", what); return SPH_ERR_INVALID; }
  return SPH_OK;
}

static bool probe_mask_ok(uint32_t typeMask) { return typeMask != 0u && !(typeMask & ~0xEu); }

static void probe_release(sph_solver* s, SphScratch& b) {
  if (!b.p) return;
  hipStreamSynchronize(s->stream);
  hipFree(b.p);
  b.p = nullptr; b.bytes = 0;
}

// A set of `points` points and `lines` lines is about to replace the current one: SPH_ERR_INVALID if the ring's rows would not fit
// the byte cap with it; otherwise the current-record buffer and the ring grown to it.
static int probe_fit(sph_solver* s, int points, int lines, const char* what) {
  const size_t row = kProbeRecord * ((size_t)points + (size_t)lines);
  if ((size_t)s->probeHistRows * row > kProbeRingBytes) {
    sph_set_error("%s: %d history rows of %zu bytes exceed %zu bytes (sph_probes_history)", what, s->probeHistRows, row, kProbeRingBytes);
    return SPH_ERR_INVALID;
  }
  if (!row) return SPH_OK;
  int rc = sph_grow_scratch(s, s->probeCur, row);
  if (rc != SPH_OK || !s->probeHistRows) return rc;
  return sph_grow_scratch(s, s->probeHist, (size_t)s->probeHistRows * row);
}

extern "C" int sph_probes_set_points(sph_solver* s, const float* points4, int32_t count, uint32_t typeMask) {
  ENTER(s);
  const char* what = "sph_probes_set_points";
  int rc = probe_check(s, what);
  if (rc != SPH_OK) return rc;
  if (count < 0 || count > SPH_PROBE_MAX_POINTS || (count > 0 && !points4)) {
    sph_set_error("%s: count %d is not in 0..%d, or null pointer", what, count, SPH_PROBE_MAX_POINTS);
    return SPH_ERR_INVALID;
  }
  if (count > 0 && !probe_mask_ok(typeMask)) { sph_set_error("%s: typeMask must be a non-empty set of bits 1..3", what); return SPH_ERR_INVALID; }
  rc = probe_fit(s, count, s->probeLineCount, what);
  if (rc != SPH_OK) return rc;
  if (count > 0) {
    rc = sph_grow_scratch(s, s->probePts, sizeof(float4) * (size_t)count);
    if (rc != SPH_OK) return rc;
    SPH_HIP(hipMemcpyAsync(s->probePts.p, points4, sizeof(float4) * (size_t)count, hipMemcpyHostToDevice, s->stream));
    SPH_HIP(hipStreamSynchronize(s->stream));  // the caller's array is free again
  } else {
    probe_release(s, s->probePts);
  }
  s->probePointCount = count;
  s->probeTypeMask = count > 0 ? typeMask : 0u;
  s->probeHistFirst = s->probeCalls;  // the ring restarts empty
  return SPH_OK;
}

extern "C" int sph_probes_set_lines(sph_solver* s, const sph_probe_line* lines, int32_t count) {
  ENTER(s);
  const char* what = "sph_probes_set_lines";
  int rc = probe_check(s, what);
  if (rc != SPH_OK) return rc;
  if (count < 0 || count > SPH_PROBE_MAX_LINES || (count > 0 && !lines)) {
    sph_set_error("%s: count %d is not in 0..%d, or null pointer", what, count, SPH_PROBE_MAX_LINES);
    return SPH_ERR_INVALID;
  }
  for (int32_t i = 0; i < count; i++) {
    const sph_probe_line& l = lines[i];
    for (int c = 0; c < 3; c++)
      if (!std::isfinite(l.origin[c]) || !std::isfinite(l.step[c])) {
        sph_set_error("%s: line %d: a word of origin or step is not finite", what, i);
        return SPH_ERR_INVALID;
      }
    if (!std::isfinite(l.iso)) { sph_set_error("%s: line %d: iso is not finite", what, i); return SPH_ERR_INVALID; }
    if (l.count < 2 || l.count > SPH_PROBE_LINE_MAX) { sph_set_error("%s: line %d: count %d is not in 2..%d", what, i, l.count, SPH_PROBE_LINE_MAX); return SPH_ERR_INVALID; }
    if (l.field < 0 || l.field >= SPH_SURFACE_FIELDS) { sph_set_error("%s: line %d: field %d is not in 0..5", what, i, l.field); return SPH_ERR_INVALID; }
    if (!probe_mask_ok(l.typeMask)) { sph_set_error("%s: line %d: typeMask must be a non-empty set of bits 1..3", what, i); return SPH_ERR_INVALID; }
  }
  rc = probe_fit(s, s->probePointCount, count, what);
  if (rc != SPH_OK) return rc;
  if (count > 0) {
    rc = sph_grow_scratch(s, s->probeLines, sizeof(sph_probe_line) * (size_t)count);
    if (rc != SPH_OK) return rc;
    SPH_HIP(hipMemcpyAsync(s->probeLines.p, lines, sizeof(sph_probe_line) * (size_t)count, hipMemcpyHostToDevice, s->stream));
    SPH_HIP(hipStreamSynchronize(s->stream));  // the caller's array is free again
  } else {
    probe_release(s, s->probeLines);
  }
  s->probeLineCount = count;
  s->probeHistFirst = s->probeCalls;  // the ring restarts empty
  return SPH_OK;
}

extern "C" int sph_probes_count(sph_solver* s, int32_t counts[2]) {
  ENTER(s);
  const int rc = probe_check(s, "sph_probes_count");
  if (rc != SPH_OK) return rc;
  if (!counts) { sph_set_error("sph_probes_count: null pointer"); return SPH_ERR_INVALID; }
  counts[0] = s->probePointCount;
  counts[1] = s->probeLineCount;
  return SPH_OK;
}

extern "C" int sph_probes_record(sph_solver* s, float* points, float* levels) {
  ENTER(s);
  const char* what = "sph_probes_record";
  int rc = probe_check(s, what);
  if (rc != SPH_OK) return rc;
  const int P = s->probePointCount, L = s->probeLineCount;
  if (!P && !L) { sph_set_error("%s: neither points nor lines are set (sph_probes_set_points, sph_probes_set_lines)", what); return SPH_ERR_ORDER; }
  SampleArgs a;
  rc = sph_sample_check(s, P ? s->probeTypeMask : 0xEu, what, &a);  // (the level kernel takes each line's own mask)
  if (rc != SPH_OK) return rc;
  const size_t rowWords = (size_t)SPH_PROBE_LEVEL_WORDS * ((size_t)P + (size_t)L), lineWords = (size_t)SPH_PROBE_LEVEL_WORDS * (size_t)P;
  float* cur = (float*)s->probeCur.p;
  float* row = s->probeHistRows ? (float*)s->probeHist.p + (size_t)(s->probeCalls % s->probeHistRows) * rowWords : nullptr;
  rc = sphk_probe_points(s, a, (const float*)s->probePts.p, P, cur, row);
  if (rc != SPH_OK) return rc;
  rc = sphk_probe_levels(s, a, (const sph_probe_line*)s->probeLines.p, L, cur + lineWords, row ? row + lineWords : nullptr);
  if (rc != SPH_OK) return rc;
  s->probeCalls++;
  if (!points && !levels) return SPH_OK;
  if (points && P) SPH_HIP(hipMemcpyAsync(points, cur, kProbeRecord * (size_t)P, hipMemcpyDeviceToHost, s->stream));
  if (levels && L) SPH_HIP(hipMemcpyAsync(levels, cur + lineWords, kProbeRecord * (size_t)L, hipMemcpyDeviceToHost, s->stream));
  SPH_HIP(hipStreamSynchronize(s->stream));  // the call's one wait
  return SPH_OK;
}

extern "C" int sph_probes_history(sph_solver* s, int32_t rows) {
  ENTER(s);
  const char* what = "sph_probes_history";
  const int rc = probe_check(s, what);
  if (rc != SPH_OK) return rc;
  if (rows < 0 || rows > SPH_PROBE_HISTORY_MAX) { sph_set_error("%s: rows %d is not in 0..%d", what, rows, SPH_PROBE_HISTORY_MAX); return SPH_ERR_INVALID; }
  const size_t row = kProbeRecord * ((size_t)s->probePointCount + (size_t)s->probeLineCount);
  if ((size_t)rows * row > kProbeRingBytes) {
    sph_set_error("%s: %d rows of %zu bytes exceed %zu bytes", what, rows, row, kProbeRingBytes);
    return SPH_ERR_INVALID;
  }
  probe_release(s, s->probeHist);
  s->probeHistRows = 0;
  s->probeHistFirst = s->probeCalls;
  if (rows == 0) return SPH_OK;
  if (row) {
    const int rcGrow = sph_grow_scratch(s, s->probeHist, (size_t)rows * row);
    if (rcGrow != SPH_OK) return rcGrow;
  }
  s->probeHistRows = rows;
  return SPH_OK;
}

// `n` consecutive ring rows from row r0: the `words` floats at `offset` of each, packed into out
static int probe_rows_d2h(sph_solver* s, float* out, int64_t r0, int64_t n, size_t rowWords, size_t offset, size_t words) {
  const float* src = (const float*)s->probeHist.p + (size_t)r0 * rowWords + offset;
  if (words == rowWords) {  // the rows hold nothing else: one run
    SPH_HIP(hipMemcpyAsync(out, src, sizeof(float) * words * (size_t)n, hipMemcpyDeviceToHost, s->stream));
    return SPH_OK;
  }
  SPH_HIP(hipMemcpy2DAsync(out, sizeof(float) * words, src, sizeof(float) * rowWords, sizeof(float) * words, (size_t)n,
                           hipMemcpyDeviceToHost, s->stream));
  return SPH_OK;
}

extern "C" int sph_probes_read_history(sph_solver* s, int64_t firstCall, int32_t count, float* points, float* levels,
                                       int64_t* callsWritten) {
  ENTER(s);
  const char* what = "sph_probes_read_history";
  int rc = probe_check(s, what);
  if (rc != SPH_OK) return rc;
  if (callsWritten) *callsWritten = s->probeCalls;
  if (!s->probeHistRows) { sph_set_error("%s: there is no history (sph_probes_history)", what); return SPH_ERR_ORDER; }
  if (count < 0) { sph_set_error("%s: bad count", what); return SPH_ERR_INVALID; }
  if (count == 0) return SPH_OK;
  const int64_t rows = s->probeHistRows, end = s->probeCalls;
  const int64_t oldest = std::max(s->probeHistFirst, end - rows);
  if (firstCall < oldest || firstCall > end - count) {
    sph_set_error("%s: calls %lld .. %lld are not all in the ring, which holds %lld .. %lld", what, (long long)firstCall,
                  (long long)(firstCall + count - 1), (long long)oldest, (long long)(end - 1));
    return SPH_ERR_INVALID;
  }
  const size_t pWords = (size_t)SPH_PROBE_LEVEL_WORDS * (size_t)s->probePointCount;
  const size_t lWords = (size_t)SPH_PROBE_LEVEL_WORDS * (size_t)s->probeLineCount;
  // at most two runs: up to the ring's end, then from its start
  const int64_t r0 = firstCall % rows;
  const int64_t n0 = std::min<int64_t>(count, rows - r0);
  for (int run = 0; run < 2; run++) {
    const int64_t first = run ? 0 : r0, n = run ? count - n0 : n0, done = run ? n0 : 0;
    if (n <= 0) continue;
    if (points && pWords) { rc = probe_rows_d2h(s, points + (size_t)done * pWords, first, n, pWords + lWords, 0, pWords); if (rc != SPH_OK) return rc; }
    if (levels && lWords) { rc = probe_rows_d2h(s, levels + (size_t)done * lWords, first, n, pWords + lWords, pWords, lWords); if (rc != SPH_OK) return rc; }
  }
  SPH_HIP(hipStreamSynchronize(s->stream));
  return SPH_OK;
}

// C ABI of libsphmi.so (include/sphmi.h), read-back: the position, velocity, density and index reads, the asynchronous position
// read-back, the export in the reference's buffer layouts (sph_read_buffer) and the neighbour rows. What the translation units of
// the ABI share is in sph_api_internal.h.
#include <string.h>

#include <vector>

#include "sph_api_internal.h"

// ---------------------------------------------------------------------------------------------- read-back
int sph_d2h(sph_solver* s, void* dst, const void* src, size_t bytes) {
  SPH_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, s->stream));
  SPH_HIP(hipStreamSynchronize(s->stream));
  return SPH_OK;
}

// dbg[6]: particles with a non-finite coordinate seen by the hash kernel (the state has blown up). Sticky: once seen, every
// blocking call keeps reporting it until the solver is destroyed — a caller that ignores one SPH_ERR_INVALID does not continue
// silently on NaN state.
static int report_blown_up(sph_solver* s) {
  sph_set_error("%llu particle coordinate(s) were not finite: the simulation state has blown up", (unsigned long long)s->blownUp);
  return SPH_ERR_INVALID;
}
int sph_check_finite_state(sph_solver* s) {
  uint32_t bad = 0;
  SPH_HIP(hipMemcpyAsync(&bad, s->d.dbg + 6, sizeof(bad), hipMemcpyDeviceToHost, s->stream));
  SPH_HIP(hipStreamSynchronize(s->stream));
  if (bad) {
    s->blownUp += bad;
    SPH_HIP(hipMemsetAsync(s->d.dbg + 6, 0, sizeof(uint32_t), s->stream));
  }
  return s->blownUp ? report_blown_up(s) : SPH_OK;
}

extern "C" int sph_read_position(sph_solver* s, float* out) {
  ENTER(s); if (!out) return SPH_ERR_INVALID;
  const int rc = sph_d2h(s, out, s->d.posOrig, sizeof(float4) * (size_t)s->d.N);
  return rc != SPH_OK ? rc : sph_check_finite_state(s);
}
// ---- asynchronous read_position_buffer. The reference's step always ends with a blocking 16N-byte read
// (owPhysicsFluidSimulator.cpp:115; 264 MB at 16.5 M particles: +45 % on the step when it is waited for). posOrig is written by
// exactly one kernel per step, the last one (integrate; + the membrane finalize pass), so the copy of step t can run on its own
// stream under the search and PCISPH stages of step t+1: copyStream waits for an event recorded on s->stream when the read is
// requested, and the next kernel that writes posOrig waits for the copy's event (sph_guard_position_write).
static int copy_setup(sph_solver* s) {
  if (s->copyStream) return SPH_OK;
  SPH_HIP(hipStreamCreateWithFlags(&s->copyStream, hipStreamNonBlocking));
  SPH_HIP(hipEventCreateWithFlags(&s->evReadReady, hipEventDisableTiming));
  SPH_HIP(hipEventCreateWithFlags(&s->evCopyDone, hipEventDisableTiming));
  SPH_HIP(hipHostMalloc((void**)&s->pinnedFlags, sizeof(uint32_t) * 4, hipHostMallocDefault));
  s->pinnedFlags[0] = 0u;
  return SPH_OK;
}

// true if the DMA engine can write [p, p + bytes) directly: pinned already, or page-locked in place now
static bool host_pinned(sph_solver* s, void* p, size_t bytes) {
  for (int i = 0; i < s->numHostRegs; i++)
    if ((char*)p >= (char*)s->hostRegs[i].p && (char*)p + bytes <= (char*)s->hostRegs[i].p + s->hostRegs[i].bytes) return true;
  unsigned int flags = 0;
  if (hipHostGetFlags(&flags, p) == hipSuccess) return true;  // hipHostMalloc'ed or registered by the caller
  (void)hipGetLastError();
  if (s->numHostRegs >= 8) return false;
  const hipError_t e = hipHostRegister(p, bytes, hipHostRegisterDefault);
  if (e != hipSuccess) { (void)hipGetLastError(); return false; }
  s->hostRegs[s->numHostRegs].p = p; s->hostRegs[s->numHostRegs].bytes = bytes; s->numHostRegs++;
  return true;
}

extern "C" int sph_read_position_wait(sph_solver* s) {
  ENTER(s);
  if (!s->copyPending) return s->blownUp ? report_blown_up(s) : SPH_OK;
  SPH_HIP(hipEventSynchronize(s->evCopyDone));
  s->copyPending = false;
  if (s->copyViaStage) memcpy(s->copyUserDst, s->copyStage, s->copyBytes);  // (the count at request time: an edit may have changed d.N)
  if (s->pinnedFlags[0]) {  // (the device counter keeps counting; it is cleared by the next blocking check)
    if (!s->blownUp) s->blownUp = s->pinnedFlags[0];
    return report_blown_up(s);
  }
  return s->blownUp ? report_blown_up(s) : SPH_OK;
}

extern "C" int sph_read_position_async(sph_solver* s, float* out) {
  ENTER(s); if (!out) return SPH_ERR_INVALID;
  int rc = copy_setup(s);
  if (rc != SPH_OK) return rc;
  if (s->copyPending) {  // the previous read must have landed before its staging area / flags are reused (long done in a step loop)
    rc = sph_read_position_wait(s);
    if (rc != SPH_OK) return rc;
  }
  const size_t bytes = sizeof(float4) * (size_t)s->d.N;
  void* dst = out;
  s->copyViaStage = false;
  if (!host_pinned(s, out, bytes)) {
    if (s->copyStageBytes < bytes) {
      if (s->copyStage) hipHostFree(s->copyStage);
      s->copyStage = nullptr; s->copyStageBytes = 0;
      SPH_HIP(hipHostMalloc(&s->copyStage, bytes, hipHostMallocDefault));
      s->copyStageBytes = bytes;
    }
    dst = s->copyStage;
    s->copyViaStage = true;
  }
  s->copyUserDst = out;
  s->copyBytes = bytes;
  SPH_HIP(hipEventRecord(s->evReadReady, s->stream));
  SPH_HIP(hipStreamWaitEvent(s->copyStream, s->evReadReady, 0));
  SPH_HIP(hipMemcpyAsync(dst, s->d.posOrig, bytes, hipMemcpyDeviceToHost, s->copyStream));
  SPH_HIP(hipMemcpyAsync(s->pinnedFlags, s->d.dbg + 6, sizeof(uint32_t), hipMemcpyDeviceToHost, s->copyStream));
  SPH_HIP(hipEventRecord(s->evCopyDone, s->copyStream));
  s->copyPending = true;
  return SPH_OK;
}

extern "C" int sph_host_unregister(sph_solver* s, void* p) {
  ENTER(s);
  if (s->copyPending) { const int rc = sph_read_position_wait(s); if (rc != SPH_OK && rc != SPH_ERR_INVALID) return rc; }
  for (int i = 0; i < s->numHostRegs; i++)
    if (s->hostRegs[i].p == p) {
      hipHostUnregister(p);
      s->hostRegs[i] = s->hostRegs[--s->numHostRegs];
      return SPH_OK;
    }
  return SPH_OK;  // not one of ours: nothing to do
}

int sph_guard_position_write(sph_solver* s, hipStream_t stream) {
  if (s->copyPending) SPH_HIP(hipStreamWaitEvent(stream ? stream : s->stream, s->evCopyDone, 0));
  return SPH_OK;
}

extern "C" int sph_read_velocity(sph_solver* s, float* out) {
  ENTER(s); if (!out) return SPH_ERR_INVALID;
  return sph_d2h(s, out, s->d.velOrig, sizeof(float4) * (size_t)s->d.N);
}
extern "C" int sph_read_density(sph_solver* s, float* out) {
  ENTER(s); if (!out) return SPH_ERR_INVALID;
  return sph_d2h(s, out, s->d.rho, sizeof(float) * (size_t)s->d.N);
}
extern "C" int sph_read_particle_index(sph_solver* s, uint32_t* out) {
  ENTER(s); if (!out) return SPH_ERR_INVALID;
  const size_t n = (size_t)s->d.N;
  std::vector<uint32_t> k(n), v(n);
  int rc = sph_d2h(s, k.data(), s->d.keys, sizeof(uint32_t) * n);
  if (rc == SPH_OK) rc = sph_d2h(s, v.data(), s->d.vals, sizeof(uint32_t) * n);
  if (rc != SPH_OK) return rc;
  for (size_t i = 0; i < n; i++) { out[2 * i] = k[i]; out[2 * i + 1] = v[i]; }
  return SPH_OK;
}

// Export in the reference's layouts (SURVEY table 2.2). Test/inspection path: converts on the host.
extern "C" int sph_read_buffer(sph_solver* s, const char* name, void* out, size_t bytes, size_t* needed) {
  ENTER(s);
  if (!name) return SPH_ERR_INVALID;
  const SphDev& d = s->d;
  const size_t n = (size_t)d.N, G1 = (size_t)d.G + 1;
  size_t need = 0;
  enum { B_POS, B_VEL, B_SPOS, B_SVEL, B_ACC, B_NMAP, B_NIDS, B_PI, B_PIB, B_GCI, B_GCIF, B_P, B_RHO, B_DBG, B_TRACE, B_K12SKIP, B_K10SKIP, B_NBP, B_NBX, B_PBLK, B_XBLK, B_BANDFLAGS, B_BANDS, B_BANDSTART } which;
  if (!strcmp(name, "position")) { which = B_POS; need = sizeof(float4) * 2 * n; }
  else if (!strcmp(name, "velocity")) { which = B_VEL; need = sizeof(float4) * 2 * n; }
  else if (!strcmp(name, "sortedPosition")) { which = B_SPOS; need = sizeof(float4) * 2 * n; }
  else if (!strcmp(name, "sortedVelocity")) { which = B_SVEL; need = sizeof(float4) * n; }
  else if (!strcmp(name, "acceleration")) { which = B_ACC; need = sizeof(float4) * 2 * n; }
  else if (!strcmp(name, "neighborMap")) { which = B_NMAP; need = sizeof(float) * 2 * 32 * n; }
  else if (!strcmp(name, "neighborIds")) { which = B_NIDS; need = sizeof(int32_t) * 32 * n; }
  else if (!strcmp(name, "particleIndex")) { which = B_PI; need = sizeof(uint32_t) * 2 * n; }
  else if (!strcmp(name, "particleIndexBack")) { which = B_PIB; need = sizeof(uint32_t) * n; }
  else if (!strcmp(name, "gridCellIndex")) { which = B_GCI; need = sizeof(uint32_t) * G1; }
  else if (!strcmp(name, "gridCellIndexFixedUp")) { which = B_GCIF; need = sizeof(uint32_t) * G1; }
  else if (!strcmp(name, "pressure")) { which = B_P; need = sizeof(float) * n; }
  else if (!strcmp(name, "rho")) { which = B_RHO; need = sizeof(float) * 2 * n; }
  else if (!strcmp(name, "diagnosticTrace")) { which = B_TRACE; need = sizeof(uint32_t) * n; }  // scratch words of diagnostic builds
  else if (!strcmp(name, "debugCounters")) { which = B_DBG; need = sizeof(uint32_t) * SPH_DBG_WORDS; }
  // one byte per 64 sorted particles: 1 = the wave skipped its neighbour loop in the last launch that consulted the per-wave flags
  else if (!strcmp(name, "pressureForceSkipped")) { which = B_K12SKIP; need = (n + SPH_TILE - 1) / SPH_TILE; }
  else if (!strcmp(name, "predictDensitySkipped")) { which = B_K10SKIP; need = (n + SPH_TILE - 1) / SPH_TILE; }
  // the neighbourhood bytes the last pressure-force launch (stage 2 M) / the last predicted-density launch behind a pressure-force
  // kernel (stage 2 M - 1) read, and the per-wave flags pBlk / xBlk as their last writers left them
  else if (!strcmp(name, "pressureNeighbourhood")) { which = B_NBP; need = (n + SPH_TILE - 1) / SPH_TILE; }
  else if (!strcmp(name, "movedNeighbourhood")) { which = B_NBX; need = (n + SPH_TILE - 1) / SPH_TILE; }
  else if (!strcmp(name, "pressureFlags")) { which = B_PBLK; need = (n + SPH_TILE - 1) / SPH_TILE; }
  else if (!strcmp(name, "movedFlags")) { which = B_XBLK; need = (n + SPH_TILE - 1) / SPH_TILE; }
  // the search bands of the last step: one flag byte per sorted particle (bit s: member of band s); the eight band
  // arrays, N records (x, y, z, sorted index as bits) each, zeros behind a band's entries; the eight start tables of G + 1 words
  else if (!strcmp(name, "searchBandFlags")) { which = B_BANDFLAGS; need = n; }
  else if (!strcmp(name, "searchBands")) { which = B_BANDS; need = sizeof(float4) * 8 * n; }
  else if (!strcmp(name, "searchBandStart")) { which = B_BANDSTART; need = sizeof(uint32_t) * 8 * G1; }
  else { sph_set_error("unknown buffer '%s'", name); return SPH_ERR_UNKNOWN_BUFFER; }
  if ((which == B_BANDFLAGS || which == B_BANDS || which == B_BANDSTART) && !s->bandsStep) {
    sph_set_error("buffer '%s': the last step built no search bands", name);
    return SPH_ERR_ORDER;
  }
  if (needed) *needed = need;
  if (!out) return SPH_OK;
  if (bytes != need) { sph_set_error("buffer '%s' is %zu bytes, caller gave %zu", name, need, bytes); return SPH_ERR_SIZE; }
  int rc = SPH_OK;
  char* o = (char*)out;
  switch (which) {
    case B_POS:
      rc = sph_d2h(s, o, d.posOrig, sizeof(float4) * n);
      if (rc == SPH_OK) { if (d.membDelta) rc = sph_d2h(s, o + sizeof(float4) * n, d.membDelta, sizeof(float4) * n); else memset(o + sizeof(float4) * n, 0, sizeof(float4) * n); }
      break;
    case B_VEL:
      rc = sph_d2h(s, o, d.velOrig, sizeof(float4) * n);
      memset(o + sizeof(float4) * n, 0, sizeof(float4) * n);  // the scratch half is only ever zeroed (App. B #16)
      break;
    case B_SPOS: {
      std::vector<uint32_t> k(n);
      std::vector<float4> sv(n);
      rc = sph_d2h(s, o, d.sortedPos, sizeof(float4) * n);
      if (rc == SPH_OK) {  // the predicted half: packed (x, y, z) on the device; .w is dead data in the reference
        std::vector<float> p3(3 * n);
        rc = sph_d2h(s, p3.data(), d.predPos, sizeof(float) * 3 * n);
        float4* half = (float4*)(o + sizeof(float4) * n);
        if (rc == SPH_OK) for (size_t i = 0; i < n; i++) half[i] = make_float4(p3[3 * i], p3[3 * i + 1], p3[3 * i + 2], 0.f);
      }
      if (rc == SPH_OK) rc = sph_d2h(s, k.data(), d.keys, sizeof(uint32_t) * n);
      if (rc == SPH_OK) rc = sph_d2h(s, sv.data(), d.sortedVel, sizeof(float4) * n);
      if (rc != SPH_OK) break;
      float4* a = (float4*)o;
      for (size_t i = 0; i < n; i++) {
        const int type = (int)a[i].w;
        const float cellf = (float)(int)k[i];  // POSITION_CELL_ID = (float)cellId (sphFluid.cl:461)
        a[i].w = cellf;
        // .w of the predicted half is dead data in the reference: cell id for boundary particles, cell id + posTimeStep *
        // (v.w + dt*a_p.w) otherwise, with a_p.w == 0
        a[n + i].w = (type == SPH_BOUNDARY_PARTICLE) ? cellf : cellf + d.posTimeStep * (sv[i].w + d.dt * 0.f);
      }
    } break;
    case B_SVEL: rc = sph_d2h(s, o, d.sortedVel, sizeof(float4) * n); break;
    case B_ACC:
      rc = sph_d2h(s, o, d.acc, sizeof(float4) * n);
      if (rc == SPH_OK) rc = sph_d2h(s, o + sizeof(float4) * n, d.accP, sizeof(float4) * n);
      break;
    case B_NIDS: rc = sph_read_neighbor_rows(s, 0, d.N, (int32_t*)o, nullptr); break;  // (already the reference's layout)
    case B_NMAP: {  // (id as float, distance) pairs
      std::vector<int32_t> ids(32 * n);
      std::vector<float> dist(32 * n);
      rc = sph_read_neighbor_rows(s, 0, d.N, ids.data(), dist.data());
      if (rc == SPH_OK) for (size_t e = 0; e < 32 * n; e++) { ((float*)o)[2 * e] = (float)ids[e]; ((float*)o)[2 * e + 1] = dist[e]; }
    } break;
    case B_PI: rc = sph_read_particle_index(s, (uint32_t*)o); break;
    case B_PIB: rc = sph_d2h(s, o, d.backIndex, sizeof(uint32_t) * n); break;
    case B_GCI: rc = sph_d2h(s, o, d.cellStartRaw, sizeof(uint32_t) * G1); break;
    case B_GCIF: rc = sph_d2h(s, o, d.cellStart, sizeof(uint32_t) * G1); break;
    case B_P: {
      std::vector<float2> rp(n);
      rc = sph_d2h(s, rp.data(), d.rp, sizeof(float2) * n);
      if (rc == SPH_OK) for (size_t i = 0; i < n; i++) ((float*)o)[i] = rp[i].y;
    } break;
    case B_TRACE: rc = sph_d2h(s, o, d.valsAlt, sizeof(uint32_t) * n); break;
    case B_DBG: rc = sph_d2h(s, o, d.dbg, sizeof(uint32_t) * SPH_DBG_WORDS); break;
    case B_K12SKIP: rc = sph_d2h(s, o, d.k12Skip, need); break;
    case B_K10SKIP: rc = sph_d2h(s, o, d.k10Skip, need); break;
    // (stage k reads the array of stage k - 1; with maxIteration < 2 no predicted-density launch consults: the array of stage 0, zeros)
    case B_NBP: rc = sph_d2h(s, o, d.nbhd + (size_t)((2 * s->cfg.maxIteration - 1) & (SPH_GATE_SLOTS - 1)) * d.nbStride, need); break;
    case B_NBX: rc = sph_d2h(s, o, d.nbhd + (size_t)((s->cfg.maxIteration >= 2 ? 2 * s->cfg.maxIteration - 2 : 0) & (SPH_GATE_SLOTS - 1)) * d.nbStride, need); break;
    case B_PBLK: rc = sph_d2h(s, o, d.pBlk, need); break;
    case B_XBLK: rc = sph_d2h(s, o, d.xBlk, need); break;
    case B_BANDFLAGS: { SphBands b; sphk_bands_bytes(s, &b); rc = sph_d2h(s, o, b.flags, need); } break;
    case B_BANDSTART: { SphBands b; sphk_bands_bytes(s, &b); rc = sph_d2h(s, o, b.start, need); } break;
    case B_BANDS: {
      SphBands b;
      sphk_bands_bytes(s, &b);
      memset(o, 0, need);
      for (int k = 0; k < 8 && rc == SPH_OK; k++) {
        uint32_t count = 0;  // the band's total: the last entry of its start table
        rc = sph_d2h(s, &count, b.start + (size_t)k * G1 + d.G, sizeof(uint32_t));
        if (rc == SPH_OK && count > n) { sph_set_error("buffer '%s': band %d holds %u entries of %zu particles", name, k, count, n); rc = SPH_ERR_INVALID; }
        if (rc == SPH_OK && count) rc = sph_d2h(s, o + sizeof(float4) * n * k, b.pos + (size_t)k * b.cap, sizeof(float4) * count);
      }
    } break;
    case B_RHO:
      rc = sph_d2h(s, o, d.rho, sizeof(float) * n);
      if (rc == SPH_OK) {
        std::vector<float2> rp(n);
        rc = sph_d2h(s, rp.data(), d.rp, sizeof(float2) * n);
        if (rc == SPH_OK) for (size_t i = 0; i < n; i++) ((float*)o)[n + i] = rp[i].x;
      }
      break;
  }
  return rc;
}

// Rows [first, first + count) of the tiled neighbour map as ids[32 * count] and / or dist[32 * count] (either may be null): the one
// place the host decodes the map (the neighborMap / neighborIds exports above come through here).
extern "C" int sph_read_neighbor_rows(sph_solver* s, int32_t first, int32_t count, int32_t* ids, float* dist) {
  ENTER(s);
  if (first < 0 || count < 0 || (long long)first + count > s->d.N) { sph_set_error("sph_read_neighbor_rows: range outside [0, N)"); return SPH_ERR_INVALID; }
  if (count == 0) return SPH_OK;
  const size_t t0 = (size_t)first / SPH_TILE, t1 = ((size_t)first + count + SPH_TILE - 1) / SPH_TILE;  // tiles [t0, t1)
  const size_t words = (t1 - t0) * 64 * 32, base = t0 * 64 * 32;
  std::vector<int32_t> ti;
  std::vector<float> td;
  int rc = SPH_OK;
  std::vector<uint16_t> t16;
  std::vector<int32_t> tb;
  if (ids) {
    ti.resize(words); t16.resize(words); tb.resize((t1 - t0) * 64);
    rc = sph_d2h(s, ti.data(), s->d.nbrId + base, sizeof(int32_t) * words);
    if (rc == SPH_OK) rc = sph_d2h(s, t16.data(), s->d.nbr16 + base, sizeof(uint16_t) * words);
    if (rc == SPH_OK) rc = sph_d2h(s, tb.data(), s->d.nbrBase + t0 * 64, sizeof(int32_t) * tb.size());
  }
  if (rc == SPH_OK && dist) { td.resize(words); rc = sph_d2h(s, td.data(), s->d.nbrDist + base, sizeof(float) * words); }
  if (rc != SPH_OK) return rc;
  const int shift = (int)(t0 * 64);  // the copies start at tile t0: decode with tile-relative particle numbers
  for (int32_t i = 0; i < count; i++)
    for (int k = 0; k < 32; k++) {
      const size_t src = nbr_index(first + i, k) - base;
      if (ids) {
        int j = nbr_decode(t16.data(), tb.data(), ti.data(), first + i - shift, k);
        // (offsets are relative to the particle's own sorted index: undo the tile-relative numbering for the unflagged ones)
        const uint32_t e = t16[src];
        if (t16[nbr_index(first + i - shift, 0)] != SPH_N16_WIDE && e != SPH_N16_EMPTY && !(e & 0x8000u)) j += shift;
        ids[(size_t)i * 32 + k] = j;
      }
      if (dist) dist[(size_t)i * 32 + k] = td[src];
    }
  return SPH_OK;
}

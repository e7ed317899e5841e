// C ABI of libsphmi.so (include/sphmi.h), the slab protocol: one solver per slab of cell layers, halo messages packed after a step
// and merged before the next one (sph_slab.hip), with or without a host round trip, and the overlapped step. What the
// translation units of the ABI share is in sph_api_internal.h.
#include "sph_api_internal.h"

extern "C" int sph_particle_count(sph_solver* s) {
  ENTER(s);
  return s->d.N;
}

extern "C" int sph_slab_init(sph_solver* s, const sph_slab* slab, const uint32_t* globalIds) {
  ENTER(s);
  sph_state_changes(s);
  if (!slab || !globalIds) { sph_set_error("sph_slab_init: null argument"); return SPH_ERR_INVALID; }
  if (s->cfg.cellIdMask != 0xffffffffu) { sph_set_error("slab decomposition needs wide cell ids (cellIdMask = 0xffffffff)"); return SPH_ERR_INVALID; }
  if (s->d.hasElastic) { sph_set_error("slab decomposition supports pure-liquid scenes only"); return SPH_ERR_INVALID; }
  if (slab->layerLo >= slab->layerHi || slab->ghostLayers < 1 || slab->globalIdBits < 1 || slab->globalIdBits > 32) { sph_set_error("bad sph_slab"); return SPH_ERR_INVALID; }
  if ((2 * s->cfg.maxIteration * 31 + 59) / 60 > slab->ghostLayers) {  // 2*maxIteration hops of 31h/30 must fit the ghost zone
    sph_set_error("ghostLayers = %d is too thin for maxIteration = %d", slab->ghostLayers, s->cfg.maxIteration);
    return SPH_ERR_INVALID;
  }
  s->slab = *slab; s->hasSlab = true; s->slabKept = -1; s->slabStepPending = false;
  if (!s->slabHost) SPH_HIP(hipHostMalloc((void**)&s->slabHost, sizeof(uint32_t) * SPH_SLAB_COUNT_WORDS, hipHostMallocDefault));
  if (!s->slabMsgEvent) SPH_HIP(hipEventCreateWithFlags(&s->slabMsgEvent, hipEventDisableTiming));
  if (!s->slabRebuildEvent) SPH_HIP(hipEventCreateWithFlags(&s->slabRebuildEvent, hipEventDisableTiming));
  SPH_HIP(hipMemcpyAsync(s->d.gid, globalIds, sizeof(uint32_t) * (size_t)s->d.N, hipMemcpyHostToDevice, s->stream));
  // ownership flags from the initial positions: reuse the rebuild path with nothing received
  SPH_HIP(hipMemcpyAsync(s->d.sortedPos, s->d.posOrig, sizeof(float4) * (size_t)s->d.N, hipMemcpyDeviceToDevice, s->stream));
  SPH_HIP(hipMemcpyAsync(s->d.sortedVel, s->d.velOrig, sizeof(float4) * (size_t)s->d.N, hipMemcpyDeviceToDevice, s->stream));
  SPH_HIP(hipMemcpyAsync(s->d.keys, s->d.gid, sizeof(uint32_t) * (size_t)s->d.N, hipMemcpyDeviceToDevice, s->stream));
  SPH_HIP(hipMemsetAsync(s->slabCounts, 0, sizeof(uint32_t) * SPH_SLAB_COUNT_WORDS, s->stream));
  int rc = sphk_slab_sort_rebuild(s, s->d.N);
  if (rc != SPH_OK) return rc;
  SPH_HIP(hipStreamSynchronize(s->stream));
  return SPH_OK;
}

// The two flags a pack or the end of an overlapped step brings back (host copies of slabCounts[3] and [7]); the one that is
// reported is cleared on the device. unsorted: raised by the last rebuild's merge kernels. moved: owned particles that moved more
// than one cell layer in a step, which breaks the assumption behind the halo depth (include/sphmi.h).
static int slab_check_flags(sph_solver* s, uint32_t unsorted, uint32_t moved) {
  if (unsorted) {
    SPH_HIP(hipMemsetAsync(s->slabCounts + 3, 0, sizeof(uint32_t), s->stream));
    sph_set_error("a halo message passed to the last sph_slab_rebuild was not sorted by global id");
    return SPH_ERR_INVALID;
  }
  if (moved) {
    hipMemsetAsync(s->slabCounts + 7, 0, sizeof(uint32_t), s->stream);
    sph_set_error("%u owned particle(s) moved more than one cell layer in one step: the %d-layer halo no longer guarantees "
                  "single-domain results (time step too large for these velocities?)", moved, s->slab.ghostLayers);
    return SPH_ERR_INVALID;
  }
  return SPH_OK;
}

static int slab_pack(sph_solver* s, uint32_t* msgDown, uint32_t* msgUp, int32_t capRecords, int32_t counts[3], uint32_t* headDown,
                     uint32_t* headUp) {
  int rc = sphk_slab_pack(s, msgDown, msgUp, capRecords, headDown, headUp);
  if (rc != SPH_OK) return rc;
  uint32_t h[8];
  SPH_HIP(hipMemcpyAsync(h, s->slabCounts, sizeof(h), hipMemcpyDeviceToHost, s->stream));
  SPH_HIP(hipStreamSynchronize(s->stream));
  counts[0] = (int32_t)h[0]; counts[1] = (int32_t)h[1]; counts[2] = (int32_t)h[2];
  rc = slab_check_flags(s, h[3], h[7]);
  if (rc != SPH_OK) return rc;
  s->slabKept = (int)h[0];
  if ((int)h[1] > capRecords || (int)h[2] > capRecords) { sph_set_error("halo message overflow: %u / %u records, room for %d", h[1], h[2], capRecords); return SPH_ERR_SIZE; }
  return SPH_OK;
}

extern "C" int sph_slab_pack(sph_solver* s, void* msgDown, void* msgUp, int32_t capRecords, int32_t counts[3]) {
  ENTER(s);
  if (!s->hasSlab || !counts || capRecords < 0 || ((s->slab.hasLower && !msgDown) || (s->slab.hasUpper && !msgUp))) {
    sph_set_error("sph_slab_pack: slab not initialised or null message buffer"); return SPH_ERR_INVALID; }
  return slab_pack(s, (uint32_t*)msgDown, (uint32_t*)msgUp, capRecords, counts, nullptr, nullptr);
}

extern "C" int sph_slab_pack_framed(sph_solver* s, void* frameDown, void* frameUp, int32_t capRecords, int32_t counts[3]) {
  ENTER(s);
  if (!s->hasSlab || !counts || capRecords < 0 || ((s->slab.hasLower && !frameDown) || (s->slab.hasUpper && !frameUp))) {
    sph_set_error("sph_slab_pack_framed: slab not initialised or null frame buffer"); return SPH_ERR_INVALID; }
  uint32_t* fd = (uint32_t*)frameDown;
  uint32_t* fu = (uint32_t*)frameUp;
  return slab_pack(s, fd ? fd + 1 : nullptr, fu ? fu + 1 : nullptr, capRecords, counts, fd, fu);
}

// ---- overlapped step: sph_slab_step_begin enqueues everything and returns; sph_slab_step_messages blocks only until the
// messages are packed (the rest of the step is still running); sph_slab_rebuild then waits for the step itself.
extern "C" int sph_slab_step_begin(sph_solver* s, int iterationCount, void* frameDown, void* frameUp, int32_t capRecords) {
  (void)iterationCount;
  ENTER(s);
  if (!s->hasSlab || capRecords < 0 || (s->slab.hasLower && !frameDown) || (s->slab.hasUpper && !frameUp)) {
    sph_set_error("sph_slab_step_begin: slab not initialised or null frame buffer"); return SPH_ERR_INVALID; }
  if (s->slabStepPending) { sph_set_error("sph_slab_step_begin: the previous overlapped step was not rebuilt"); return SPH_ERR_ORDER; }
  StepTail tail{(uint32_t*)frameDown, (uint32_t*)frameUp, (int)capRecords};
  const int rc = enqueue_step(s, &tail);
  if (rc != SPH_OK) return rc;
  s->slabStepPending = true;
  s->slabKept = -1;
  s->slabCapRecords = (int)capRecords;
  return SPH_OK;
}

extern "C" int sph_slab_step_messages(sph_solver* s, int32_t counts[2]) {
  ENTER(s);
  if (!s->hasSlab || !s->slabStepPending || !counts) { sph_set_error("sph_slab_step_messages without sph_slab_step_begin"); return SPH_ERR_ORDER; }
  SPH_HIP(hipEventSynchronize(s->slabMsgEvent));
  counts[0] = (int32_t)s->slabHost[5]; counts[1] = (int32_t)s->slabHost[6];
  if (counts[0] > s->slabCapRecords || counts[1] > s->slabCapRecords) {
    sph_set_error("halo message overflow: %d / %d records, room for %d", counts[0], counts[1], s->slabCapRecords);
    return SPH_ERR_SIZE;
  }
  return SPH_OK;
}

extern "C" int sph_slab_rebuild(sph_solver* s, const void* recvDown, int32_t nDown, const void* recvUp, int32_t nUp) {
  ENTER(s);
  sph_state_changes(s);
  if (!s->hasSlab || nDown < 0 || nUp < 0 || (nDown && !recvDown) || (nUp && !recvUp)) { sph_set_error("sph_slab_rebuild: bad arguments"); return SPH_ERR_INVALID; }
  if (s->slabStepPending) {  // overlapped step: the kept count arrives with the end of the step
    SPH_HIP(hipStreamSynchronize(s->stream));
    s->slabStepPending = false;
    const int rc = slab_check_flags(s, s->slabHost[3], s->slabHost[7]);
    if (rc != SPH_OK) return rc;
    s->slabKept = (int)s->slabHost[8];
  }
  if (s->slabKept < 0) { sph_set_error("sph_slab_rebuild without a preceding sph_slab_pack"); return SPH_ERR_ORDER; }
  const int kept = s->slabKept;
  s->slabKept = -1;
  const long long total = (long long)kept + nDown + nUp;
  if (total > s->capacity || total <= 0) { sph_set_error("slab holds %lld particles after the exchange, capacity %d", total, s->capacity); return SPH_ERR_SIZE; }
  return sphk_slab_rebuild(s, (const uint32_t*)recvDown, nDown, (const uint32_t*)recvUp, nUp, kept);
}

// ---- the rebuild without a host round trip. The frames are what RCCL delivered: [payload words | payload]; the kept count is
// where the pack left it on the device. Everything is enqueued at once; the totals come back through pinned memory and
// sph_slab_finish (called by sph_slab_rebuild_finish, or implicitly by the next entry point) sets the new particle count.
extern "C" int sph_slab_rebuild_framed(sph_solver* s, const void* frameDown, int32_t capDownRecords, const void* frameUp,
                                       int32_t capUpRecords) {
  ENTER(s);
  sph_state_changes(s);
  if (!s->hasSlab || capDownRecords < 0 || capUpRecords < 0 || (s->slab.hasLower && !frameDown) || (s->slab.hasUpper && !frameUp)) {
    sph_set_error("sph_slab_rebuild_framed: slab not initialised, negative capacity, or no frame from a neighbour that exists");
    return SPH_ERR_INVALID;
  }
  const uint32_t* keptPtr;
  if (s->slabStepPending) keptPtr = s->slabCounts + 8;       // overlapped step: the kept pass of sph_slab_step_begin
  else if (s->slabKept >= 0) keptPtr = s->slabCounts + 0;    // sph_slab_pack / sph_slab_pack_framed
  else { sph_set_error("sph_slab_rebuild_framed without a preceding pack"); return SPH_ERR_ORDER; }
  s->slabCapDown = frameDown ? capDownRecords : 0; s->slabCapUp = frameUp ? capUpRecords : 0;
  int rc = sphk_slab_rebuild_framed(s, (const uint32_t*)frameDown, s->slabCapDown, (const uint32_t*)frameUp, s->slabCapUp, keptPtr, s->slabCounts + 12);
  if (rc != SPH_OK) return rc;
  SPH_HIP(hipMemcpyAsync(s->slabHost + 12, s->slabCounts + 12, sizeof(uint32_t) * 4, hipMemcpyDeviceToHost, s->stream));
  SPH_HIP(hipEventRecord(s->slabRebuildEvent, s->stream));
  s->slabRebuildPending = true;
  return SPH_OK;
}

// counts: kept, records from below, records from above, and 1 if NOTHING was merged because a frame announced more records than
// its buffer had room for (the caller fetches the missing part and rebuilds with sph_slab_rebuild; the state is untouched).
int sph_slab_finish(sph_solver* s, int32_t counts[4]) {
  SPH_HIP(hipEventSynchronize(s->slabRebuildEvent));
  s->slabRebuildPending = false;
  if (s->slabStepPending) {  // the flags that came back with the end of the overlapped step
    s->slabStepPending = false;
    const int rc = slab_check_flags(s, s->slabHost[3], s->slabHost[7]);
    if (rc != SPH_OK) return rc;
  }
  const int kept = (int)s->slabHost[12], nDown = (int)s->slabHost[13], nUp = (int)s->slabHost[14];
  const bool nothing = s->slabHost[15] != 0u;
  if (counts) { counts[0] = kept; counts[1] = nDown; counts[2] = nUp; counts[3] = nothing ? 1 : 0; }
  if (nothing) {
    if (nDown <= s->slabCapDown && nUp <= s->slabCapUp) {
      sph_set_error("slab holds %lld particles after the exchange, capacity %d", (long long)kept + nDown + nUp, s->capacity);
      return SPH_ERR_SIZE;
    }
    s->slabKept = kept;  // the frames were too short: sph_slab_rebuild with the complete messages finishes the job
    if (!counts) { sph_set_error("a halo frame announced %d / %d records, room for %d / %d", nDown, nUp, s->slabCapDown, s->slabCapUp); return SPH_ERR_SIZE; }
    return SPH_OK;
  }
  s->slabKept = -1;
  s->d.N = kept + nDown + nUp;
  s->progress = 0;
  return SPH_OK;
}

extern "C" int sph_slab_rebuild_finish(sph_solver* s, int32_t counts[4]) {
  ENTER_RAW(s);
  if (!counts) { sph_set_error("sph_slab_rebuild_finish: null argument"); return SPH_ERR_INVALID; }
  if (!s->slabRebuildPending) { sph_set_error("sph_slab_rebuild_finish without sph_slab_rebuild_framed"); return SPH_ERR_ORDER; }
  return sph_slab_finish(s, counts);
}

extern "C" int sph_slab_liquid_signature(sph_solver* s, uint32_t* typeBits) {
  ENTER(s);
  if (!typeBits) return SPH_ERR_INVALID;
  *typeBits = s->liquidSig;
  return SPH_OK;
}

extern "C" int sph_slab_set_record_format(sph_solver* s, int32_t recordWords, uint32_t typeBits) {
  ENTER(s);
  if (recordWords != SPH_SLAB_RECORD_WORDS && recordWords != SPH_SLAB_COMPACT_WORDS) { sph_set_error("record words must be %d or %d", SPH_SLAB_RECORD_WORDS, SPH_SLAB_COMPACT_WORDS); return SPH_ERR_INVALID; }
  if (recordWords == SPH_SLAB_COMPACT_WORDS && (s->liquidSig == 0xffffffffu || (s->liquidSig != 0u && s->liquidSig != typeBits))) {
    sph_set_error("compact halo records need one common type word and velocity.w == 0 for every non-boundary particle");
    return SPH_ERR_INVALID;
  }
  s->slabRecWords = recordWords; s->slabTypeBits = typeBits;
  return SPH_OK;
}

extern "C" int sph_stream_wait_event(sph_solver* s, void* hipEvent) {
  ENTER(s);
  if (!hipEvent) return SPH_ERR_INVALID;
  SPH_HIP(hipStreamWaitEvent(s->stream, (hipEvent_t)hipEvent, 0));
  return SPH_OK;
}

extern "C" int sph_slab_read(sph_solver* s, float* position4, float* velocity4, uint32_t* globalIds, uint32_t* owned) {
  ENTER(s);
  if (!s->hasSlab) { sph_set_error("slab not initialised"); return SPH_ERR_INVALID; }
  const size_t n = (size_t)s->d.N;
  int rc = SPH_OK;
  if (position4) rc = sph_d2h(s, position4, s->d.posOrig, sizeof(float4) * n);
  if (rc == SPH_OK && velocity4) rc = sph_d2h(s, velocity4, s->d.velOrig, sizeof(float4) * n);
  if (rc == SPH_OK && globalIds) rc = sph_d2h(s, globalIds, s->d.gid, sizeof(uint32_t) * n);
  if (rc == SPH_OK && owned) rc = sph_d2h(s, owned, s->d.owned, sizeof(uint32_t) * n);
  return rc;
}

// C ABI of libsphmi.so (include/sphmi.h): errors and build info, stage timing, solver lifetime, the 18 stage entry points that mirror
// owOpenCLSolver::_run* (owOpenCLSolver.cpp:213-687) and the fused step. Read-back and the reference-layout export are in
// sph_api_read.hip, the slab protocol in sph_api_slab.hip, the analysis calls in sph_api_analysis.hip, particle editing in
// sph_api_edit.hip; what they share is in sph_api_internal.h.
// There is no CPU path in this library: every entry point needs a HIP device and fails with SPH_ERR_HIP otherwise.
#include <stdarg.h>
#include <string.h>

#include <cmath>
#include <memory>

#include "sph_api_internal.h"
#include "sph_fastmath.h"

#define SPH_STR_(x) #x
#define SPH_STR(x) SPH_STR_(x)
static thread_local char g_err[512] = "";
void sph_set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

extern "C" const char* sph_last_error(void) { return g_err; }
extern "C" int sph_abi_version(void) { return SPHMI_ABI_VERSION; }

// What this binary was built as: the product, or a variant of it (make variant NAME=... EXTRA=-D...); bench.py prints this string.
extern "C" const char* sph_build_info(void) {
  return "libsphmi gfx950 abi " SPH_STR(SPHMI_ABI_VERSION)
#ifdef FN_STAMPS
         " FN_STAMPS"
#endif
#ifdef SPH_VARIANT
         " variant:" SPH_STR(SPH_VARIANT)
#endif
      ;
}

// Every permanent device allocation: recorded in the solver, which frees the record (~sph_solver)
template <typename T>
static int dev_alloc(sph_solver* s, T** p, size_t count) {
  *p = nullptr;
  SPH_HIP(hipMalloc((void**)p, sizeof(T) * (count ? count : 1)));
  s->allocs.push_back(*p);
  return SPH_OK;
}

SphDev sph_ranged(const sph_solver* s, int ghostDepth) {
  SphDev d = s->d;
  d.rangeLo = 0; d.rangeHi = d.G;
  if (s->hasSlab && ghostDepth >= 0) {
    const long long layerCells = (long long)d.gx * d.gy;
    long long lo = (long long)s->slab.layerLo - ghostDepth, hi = (long long)s->slab.layerHi + ghostDepth;
    if (lo < 0) lo = 0;
    if (hi > d.gz) hi = d.gz;
    if (hi < lo) hi = lo;
    d.rangeLo = (int)(lo * layerCells); d.rangeHi = (int)(hi * layerCells);
  }
  return d;
}

SphDev sph_ranged_layers(const sph_solver* s, long long lo, long long hi) {
  SphDev d = s->d;
  const long long layerCells = (long long)d.gx * d.gy;
  if (lo < 0) lo = 0;
  if (hi > d.gz) hi = d.gz;
  if (hi < lo) hi = lo;
  d.rangeLo = (int)(lo * layerCells); d.rangeHi = (int)(hi * layerCells);
  return d;
}

static int bit_length(uint32_t v) { int b = 0; while (v) { b++; v >>= 1; } return b; }

// Radial-histogram bin of a squared distance exactly as findNeighbors computes it (sphFluid.cl:159-160):
// (int)(sqrt(d2) * radius_segments / h), float arithmetic, IEEE sqrt and divide (this file is built with -ffp-contract=off).
static int radial_bin(float d2, float h) {
  volatile float dist = sqrtf(d2);
  volatile float scaled = dist * (float)SPH_RSEG;
  volatile float q = scaled / h;
  return (int)q;
}
static float bits_to_float(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }
static uint32_t float_to_bits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }

// binU[j], j = 0..29: the smallest float U such that "d2 < U" <=> "d2 <= h*h and radial_bin(d2) <= j". radial_bin is
// monotone in d2 (sqrt, multiply and divide round monotonically), so T[b] = min{ d2 : radial_bin(d2) >= b } is found by
// bisection over the float bit patterns; U[j] = min(T[j+1], nextafter(h*h)).
static void compute_bin_thresholds(float h, float* U) {
  volatile float h2v = h * h;
  const float h2 = h2v;
  const uint32_t h2next = float_to_bits(h2) + 1u;
  const uint32_t top = float_to_bits(16.0f * h2);
  for (int j = 0; j < SPH_RSEG; j++) {
    uint32_t lo = 0u, hi = top;  // smallest bit pattern with radial_bin >= j+1
    while (lo < hi) {
      const uint32_t mid = lo + (hi - lo) / 2u;
      if (radial_bin(bits_to_float(mid), h) >= j + 1) hi = mid; else lo = mid + 1u;
    }
    U[j] = bits_to_float(lo < h2next ? lo : h2next);
  }
  U[SPH_RSEG] = U[SPH_RSEG + 1] = bits_to_float(h2next);
  // U[32 + jb], jb = 0..30: r_thr^2 of pass 1, r_thr = (float)(jb + 1) * h / (float)radius_segments evaluated in float like
  // sphFluid.cl:313-321 (jb = 30: "fewer than 32 candidates", r_thr = 31h/30)
  for (int jb = 0; jb <= SPH_RSEG; jb++) {
    volatile float a = (float)(jb + 1) * h;
    volatile float r = a / (float)SPH_RSEG;
    volatile float r2 = r * r;
    U[32 + jb] = r2;
  }
  // U[63]: radius^2 of the search kernel's filter, a superset of pass 0 (h) and of every pass-1 radius (<= 31h/30)
  {
    const float rmax2 = U[32 + SPH_RSEG] > h2 ? U[32 + SPH_RSEG] : h2;
    volatile float f = rmax2 * (1.f + 0x1p-20f);
    U[63] = f;
  }
}

// ---------------------------------------------------------------------------------------------- timing
struct StageTimer {
  sph_solver* s; int stage; hipEvent_t a, b; bool on;
  StageTimer(sph_solver* s_, int stage_) : s(s_), stage(stage_), a(nullptr), b(nullptr), on(s_->timing) {
    if (!on) return;
    if (hipEventCreate(&a) != hipSuccess) { on = false; return; }
    if (hipEventCreate(&b) != hipSuccess) { hipEventDestroy(a); on = false; return; }
    hipEventRecord(a, s->stream);
  }
  ~StageTimer() {
    if (!on) return;
    hipEventRecord(b, s->stream);
    s->pending.push_back({stage, a, b});
  }
};

// the recorded event pairs are read into the stage totals (read == true) and destroyed
static void release_pending(sph_solver* s, bool read) {
  for (const sph_solver::Pending& p : s->pending) {
    float ms = 0.f;
    if (read && hipEventElapsedTime(&ms, p.a, p.b) == hipSuccess) {
      s->stageMs[p.stage] += (double)ms;
      s->stageLaunches[p.stage] += 1;
    }
    hipEventDestroy(p.a);
    hipEventDestroy(p.b);
  }
  s->pending.clear();
}

static int resolve_pending(sph_solver* s) {
  if (s->pending.empty()) return SPH_OK;
  SPH_HIP(hipStreamSynchronize(s->stream));
  release_pending(s, true);
  return SPH_OK;
}

extern "C" int sph_set_stage_timing(sph_solver* s, int enable) {
  if (!s) return SPH_ERR_INVALID;
  s->timing = enable != 0;
  return SPH_OK;
}
extern "C" int sph_reset_stage_times(sph_solver* s) {
  if (!s) return SPH_ERR_INVALID;
  int rc = resolve_pending(s);
  // (every diagnostic counter except dbg[6], the non-finite-coordinate count that sph_check_finite_state reports)
  hipMemsetAsync(s->d.dbg, 0, sizeof(uint32_t) * 6, s->stream);
  hipMemsetAsync(s->d.dbg + 7, 0, sizeof(uint32_t) * (SPH_DBG_WORDS - 7), s->stream);
  memset(s->stageMs, 0, sizeof(s->stageMs));
  memset(s->stageLaunches, 0, sizeof(s->stageLaunches));
  return rc;
}
extern "C" int sph_get_stage_times(sph_solver* s, double* ms_total, int64_t* launches, int n) {
  if (!s || (n != SPH_ST_COUNT && n != SPH_ST_BANDS)) return SPH_ERR_INVALID;  // (SPH_ST_BANDS: a caller from before the band stage)
  int rc = resolve_pending(s);
  if (rc) return rc;
  for (int i = 0; i < n; i++) {
    if (ms_total) ms_total[i] = s->stageMs[i];
    if (launches) launches[i] = s->stageLaunches[i];
  }
  return SPH_OK;
}

// ---------------------------------------------------------------------------------------------- create / destroy
// Two different libamdhip64 files in one process (e.g. /opt/rocm's and the copy bundled with PyTorch) do not both see the
// GPU. Returns true and the two paths if /proc/self/maps shows that situation.
static bool two_hip_runtimes(char* out, size_t cap) {
  FILE* f = fopen("/proc/self/maps", "r");
  if (!f) return false;
  char line[1024], first[512] = "";
  bool two = false;
  while (!two && fgets(line, sizeof(line), f)) {
    if (!strstr(line, "libamdhip64")) continue;
    char* path = strchr(line, '/');
    if (!path) continue;
    path[strcspn(path, "\n")] = 0;
    if (!first[0]) snprintf(first, sizeof(first), "%s", path);
    else if (strcmp(first, path) != 0) { snprintf(out, cap, "%s and %s", first, path); two = true; }
  }
  fclose(f);
  return two;
}

sph_solver::~sph_solver() {
  for (void* p : allocs) hipFree(p);
  if (slabHost) hipHostFree(slabHost);
  for (int i = 0; i < numHostRegs; i++) hipHostUnregister(hostRegs[i].p);
  if (copyStage) hipHostFree(copyStage);
  if (pinnedFlags) hipHostFree(pinnedFlags);
  if (evReadReady) hipEventDestroy(evReadReady);
  if (evCopyDone) hipEventDestroy(evCopyDone);
  if (copyStream) hipStreamDestroy(copyStream);
  for (hipEvent_t e : evChunk) if (e) hipEventDestroy(e);
  if (evChunkJoin) hipEventDestroy(evChunkJoin);
  if (evDeferred) hipEventDestroy(evDeferred);
  if (chunkStream) hipStreamDestroy(chunkStream);
  if (evSearchFork) hipEventDestroy(evSearchFork);
  if (searchStream) hipStreamDestroy(searchStream);
  if (slabMsgEvent) hipEventDestroy(slabMsgEvent);
  if (slabRebuildEvent) hipEventDestroy(slabRebuildEvent);
  if (ownStream && stream) hipStreamDestroy(stream);
}

extern "C" int sph_destroy(sph_solver* s) {
  if (!s) return SPH_OK;
  hipSetDevice(s->cfg.device);
  if (s->stream) hipStreamSynchronize(s->stream);
  if (s->copyStream) hipStreamSynchronize(s->copyStream);
  if (s->searchStream) hipStreamSynchronize(s->searchStream);  // (both idle already: every step joins them into s->stream)
  if (s->chunkStream) hipStreamSynchronize(s->chunkStream);
  release_pending(s, false);
  delete s;
  return SPH_OK;
}

// The index arrays of the elastic matter, checked like the coordinates: every one of these words becomes a device address
// (k_elastic: backIndex[(int)conn.x]; k_membranes: posOrig[membraneData[..]], pml[orig id * 7 + ..] for ANY neighbour whose type
// truncates to 2), and the reference checks none of them. One pass over 39 E + 3 M + N words.
static int check_elastic_input(const sph_config& c, const float* position, const float* elastic, const int32_t* membraneData,
                               const int32_t* pml) {
  const int N = c.particleCount, E = c.numOfElasticP, M = c.numOfMembranes;
  if (M < 0) { sph_set_error("numOfMembranes %d is negative", M); return SPH_ERR_INVALID; }
  for (int i = 0; i < E; i++) {
    bool ended = false;
    for (int k = 0; k < SPH_MAXN; k++) {
      const float* w = elastic + 4 * ((size_t)i * SPH_MAXN + k);
      const float x = w[0];  // every kernel truncates it with (int): (-2, -1] is NO_PARTICLE_ID, (-1, 0] is particle 0
      if (!std::isfinite(x)) { sph_set_error("elastic connection %d of particle %d: partner %g is not finite", k, i, x); return SPH_ERR_INVALID; }
      if (ended) continue;   // past the first -1 only the (int) of this word is ever formed
      if (x <= -2.f || (double)x >= (double)N) {
        sph_set_error("elastic connection %d of particle %d: partner %g is neither -1 nor in [0, %d)", k, i, x, N);
        return SPH_ERR_INVALID;
      }
      if ((int)x == -1) { ended = true; continue; }
      if (!std::isfinite(w[1])) { sph_set_error("elastic connection %d of particle %d: rest length %g is not finite", k, i, w[1]); return SPH_ERR_INVALID; }
      if (!(w[2] >= -2147483648.f && w[2] < 2147483648.f)) {  // (int)conn.z must be defined (a NaN fails both comparisons)
        sph_set_error("elastic connection %d of particle %d: muscle word %g does not convert to int", k, i, w[2]);
        return SPH_ERR_INVALID;
      }
    }
  }
  if (!(membraneData && pml && M > 0)) return SPH_OK;  // (the condition under which sph_create uploads the lists and the stage runs)
  for (size_t k = 0; k < (size_t)3 * M; k++)
    if (membraneData[k] < 0 || membraneData[k] >= N) {
      sph_set_error("membraneData[%zu] (corner %zu of membrane %zu) = %d is not in [0, %d)", k, k % 3, k / 3, membraneData[k], N);
      return SPH_ERR_INVALID;
    }
  for (int i = 0; i < E; i++)
    for (int k = 0; k < SPH_MAX_MEMBRANES_INCLUDING_SAME_PARTICLE; k++) {
      const int32_t m = pml[(size_t)i * SPH_MAX_MEMBRANES_INCLUDING_SAME_PARTICLE + k];
      if (m < 0) break;  // any negative entry ends the list, as in the kernel
      if (m >= M) {
        sph_set_error("particleMembranesList[%d][%d] = %d is not below numOfMembranes %d", i, k, m, M);
        return SPH_ERR_INVALID;
      }
    }
  // the list has numOfElasticP rows and the kernel indexes it by the ORIGINAL id of whichever neighbour has elastic type
  if (c.elasticOffset != 0) { sph_set_error("membrane lists need elasticOffset 0 (got %d): they are indexed by original particle id", c.elasticOffset); return SPH_ERR_INVALID; }
  for (int i = E; i < N; i++)
    if (position[4 * (size_t)i + 3] >= 2.f && position[4 * (size_t)i + 3] < 3.f) {  // (int)type == SPH_ELASTIC_PARTICLE
      sph_set_error("particle %d has elastic type %g but lies outside the elastic block [0, %d) that the membrane lists cover", i,
                    position[4 * (size_t)i + 3], E);
      return SPH_ERR_INVALID;
    }
  return SPH_OK;
}

extern "C" int sph_create(const sph_config* cfg, const float* position, const float* velocity, const float* elastic,
                          const int32_t* membraneData, const int32_t* pml, sph_solver** out) {
  if (!cfg || !position || !velocity || !out) { sph_set_error("sph_create: null argument"); return SPH_ERR_INVALID; }
  *out = nullptr;
  if (cfg->abi_version != SPHMI_ABI_VERSION) { sph_set_error("sph_config.abi_version %d != %d", cfg->abi_version, SPHMI_ABI_VERSION); return SPH_ERR_INVALID; }
  const int N = cfg->particleCount;
  const int cap = cfg->capacity > 0 ? cfg->capacity : N;
  // (k_find_neighbors forms 32-bit element indices into the tiled neighbour map, 32 slots per particle: capacity * 32 < 2^32)
  static_assert((long long)SPH_MAX_PARTICLES * SPH_MAXN < 0x100000000LL, "uint32 mapBase in k_find_neighbors");
  if (N <= 0 || cap < N || cap > SPH_MAX_PARTICLES) {
    sph_set_error("particleCount %d / capacity %d out of range: one solver holds at most %d particles (2^27 - 1; 32-bit neighbour-map "
                  "indices)", N, cap, SPH_MAX_PARTICLES);
    return SPH_ERR_INVALID;
  }
  if (cfg->gridCellsX <= 0 || cfg->gridCellsY <= 0 || cfg->gridCellsZ <= 0 ||
      (long long)cfg->gridCellsX * cfg->gridCellsY * cfg->gridCellsZ != (long long)cfg->gridCellCount) {
    sph_set_error("gridCellCount does not equal gridCellsX*gridCellsY*gridCellsZ");
    return SPH_ERR_INVALID;
  }
  if (cfg->cellIdMask != 0xffffu && cfg->cellIdMask != 0xffffffffu) { sph_set_error("cellIdMask must be 0xffff (reference) or 0xffffffff (wide)"); return SPH_ERR_INVALID; }
  if (cfg->numOfElasticP < 0 || (cfg->numOfElasticP > 0 && cfg->elasticOffset < 0) || (long long)cfg->numOfElasticP + cfg->elasticOffset > N ||
      (cfg->numOfElasticP > 0 && !elastic)) {
    sph_set_error("elastic configuration inconsistent");
    return SPH_ERR_INVALID;
  }
  if (cfg->numOfElasticP > 0 && (cfg->muscleCount <= 0 || cfg->muscleCount > 4096)) { sph_set_error("muscleCount out of range"); return SPH_ERR_INVALID; }
  if (cfg->maxIteration < 1) { sph_set_error("maxIteration must be >= 1"); return SPH_ERR_INVALID; }
  if (!(cfg->h > 0.f) || !(cfg->hashGridCellSize > 0.f)) { sph_set_error("h / hashGridCellSize must be positive"); return SPH_ERR_INVALID; }

  uint32_t liquidSig = 0u;
  // Input sanity the reference does not have. Non-finite coordinates make every particle hash into one cell (a quadratic
  // search); in wide mode a coordinate outside the box gives a cell id outside [0, gridCellCount), and the radix sort only
  // orders the bits a valid id can have. (Reference mode keeps the reference's behaviour for out-of-box input: ids alias.)
  // Creation is the only way in for such coordinates: integrate clamps every new position into the box (sphFluid.cl:1750-1755,
  // integrate_particle), and a NaN — which no clamp catches — is counted by the hash kernel (dbg[6], sph_check_finite_state).
  for (int i = 0; i < N; i++) {
    const float* p4 = position + 4 * (size_t)i;
    sph_fold_liquid_signature(liquidSig, p4, velocity + 4 * (size_t)i);
    if (const char* fault = sph_position_fault(*cfg, p4)) {
      sph_set_error("particle %d at (%g, %g, %g) is %s", i, p4[0], p4[1], p4[2], fault);
      return SPH_ERR_INVALID;
    }
  }
  { const int rc = check_elastic_input(*cfg, position, elastic, membraneData, pml); if (rc != SPH_OK) return rc; }
  int ndev = 0;
  const hipError_t devErr = hipGetDeviceCount(&ndev);
  if (devErr != hipSuccess || ndev <= 0 || cfg->device < 0 || cfg->device >= ndev) {
    char two[300];
    if (two_hip_runtimes(two, sizeof(two)))  // the usual cause of "no ROCm-capable device" on a box that has one
      sph_set_error("no HIP device %d (found %d): two HIP runtimes are mapped into this process (%s); load the one the rest of the "
                    "process uses BEFORE libsphmi.so so that both bind to it", cfg->device, ndev, two);
    else
      sph_set_error("no HIP device %d (found %d%s%s): libsphmi has no CPU fallback", cfg->device, ndev,
                    devErr != hipSuccess ? ", " : "", devErr != hipSuccess ? hipGetErrorString(devErr) : "");
    return SPH_ERR_HIP;
  }
  SPH_HIP(hipSetDevice(cfg->device));

  // (a return before the release below destroys the solver and, with it, everything it owns by then)
  std::unique_ptr<sph_solver> owner(new sph_solver());
  sph_solver* const s = owner.get();
  s->cfg = *cfg;
  s->liquidSig = liquidSig;
  if (cfg->stream) { s->stream = (hipStream_t)cfg->stream; s->ownStream = false; }
  else {
    hipError_t e = hipStreamCreateWithFlags(&s->stream, hipStreamNonBlocking);
    if (e != hipSuccess) { sph_set_error("hipStreamCreate failed: %s", hipGetErrorString(e)); return SPH_ERR_HIP; }
    s->ownStream = true;
  }
  // the overlapped step's streams and events; like the copy stream, never the caller's
  SPH_HIP(hipStreamCreateWithFlags(&s->chunkStream, hipStreamNonBlocking));
  SPH_HIP(hipStreamCreateWithFlags(&s->searchStream, hipStreamNonBlocking));
  SPH_HIP(hipEventCreateWithFlags(&s->evSearchFork, hipEventDisableTiming));
  for (hipEvent_t& e : s->evChunk) SPH_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
  SPH_HIP(hipEventCreateWithFlags(&s->evChunkJoin, hipEventDisableTiming));
  SPH_HIP(hipEventCreateWithFlags(&s->evDeferred, hipEventDisableTiming));
  SphDev& d = s->d;
  d.N = N; d.G = cfg->gridCellCount; d.gx = cfg->gridCellsX; d.gy = cfg->gridCellsY; d.gz = cfg->gridCellsZ;
  d.cellMask = cfg->cellIdMask;
  d.h = cfg->h; d.cellSize = cfg->hashGridCellSize; d.cellSizeInv = cfg->hashGridCellSizeInv;
  d.simScale = cfg->simulationScale; d.simScaleInv = cfg->simulationScaleInv;
  d.xmin = cfg->xmin; d.xmax = cfg->xmax; d.ymin = cfg->ymin; d.ymax = cfg->ymax; d.zmin = cfg->zmin; d.zmax = cfg->zmax;
  d.r0 = cfg->r0; d.mass = cfg->mass; d.rho0 = cfg->rho0; d.dt = cfg->timeStep; d.delta = cfg->delta;
  d.gravx = cfg->gravity_x; d.gravy = cfg->gravity_y; d.gravz = cfg->gravity_z;
  d.surfTens = cfg->surfTensCoeff;
  // per-step constants in the reference's exact expression types (see sph_common.h for the source lines)
  {
    volatile float massMu = cfg->mass * cfg->viscosity;
    volatile float hs = cfg->h * cfg->simulationScale;
    volatile float hs2 = hs * hs;
    volatile float hs4 = hs2 * hs2;
    volatile float hs6 = hs4 * hs2;
    volatile float pts = cfg->timeStep * cfg->simulationScaleInv;
    volatile float r0d = cfg->rho0 * cfg->delta;
    volatile float halfHs = hs / 2;
    d.massMu = massMu; d.hs = hs; d.hs2 = hs2; d.hs6 = hs6; d.posTimeStep = pts; d.rho0delta = r0d;
    d.closeR = 0.5 * (double)halfHs;
    // (double)r < closeR  <=>  r < closeRf, with closeRf the smallest float whose double value is >= closeR
    float f = (float)d.closeR;
    while ((double)f < d.closeR) f = nextafterf(f, INFINITY);
    while ((double)nextafterf(f, -INFINITY) >= d.closeR) f = nextafterf(f, -INFINITY);
    d.closeRf = f;
  }
  d.massWpoly6 = ((double)cfg->mass) * cfg->Wpoly6Coefficient;
  // operand bounds of k_pressure_force's short division / square-root path; the smallest density a kernel can write is hs^6 * mass * Wpoly6
  sph_fast_bounds(cfg->simulationScale, d.hs, (float)((double)d.hs6 * d.massWpoly6), &d.fastD2Min, &d.fastD2Max, &d.fastValueMin);
  d.massGradW = ((double)cfg->mass) * cfg->gradWspikyCoefficient;
  d.del2W = cfg->del2WviscosityCoefficient;
  d.numElastic = cfg->numOfElasticP; d.elasticOffset = cfg->elasticOffset; d.muscleCount = cfg->muscleCount;
  d.numMembranes = cfg->numOfMembranes; d.hasElastic = cfg->numOfElasticP > 0;
  d.rangeLo = 0; d.rangeHi = d.G;

  s->capacity = cap;
  s->capTiles = (cap + SPH_TILE - 1) / SPH_TILE;
  s->sortBits = (cfg->cellIdMask == 0xffffu) ? 16 : bit_length((uint32_t)(d.G > 0 ? d.G - 1 : 0));
  if (s->sortBits < 1) s->sortBits = 1;
  s->maxSortBlocks = (cap + (SPH_BLOCK * 16) - 1) / (SPH_BLOCK * 16);

  int rc = SPH_OK;
  const size_t n = (size_t)cap, nUp = (size_t)N, G1 = (size_t)d.G + 1, mapN = (size_t)s->capTiles * 64 * 32;
#define A(ptr, count) if (rc == SPH_OK) rc = dev_alloc(s, &(ptr), (count))
  A(d.posOrig, n); A(d.velOrig, n); A(d.sortedPos, n); A(d.sortedVel, n); A(d.predPos, 3 * n); A(d.acc, n); A(d.accP, n); A(d.rp, n); A(d.bndMask, n); A(d.gatherRec, 2 * ((n + 3) / 4 * 4));
  A(d.keys, n); A(d.vals, n); A(d.keysAlt, n); A(d.valsAlt, n); A(d.backIndex, n);
  A(d.cellStart, G1); A(d.cellStartRaw, G1);
  A(d.nbrId, mapN); A(d.nbrDist, mapN); A(d.nbr16, mapN); A(d.nbrBase, (size_t)s->capTiles * 64);
  A(d.rho, n);
  const size_t waves = (size_t)s->capTiles;  // (SPH_TILE == 64: a tile of the neighbour map is a wave of the gather kernels)
  const size_t waves4 = (waves + 3) / 4 * 4;     // (the consumers load a wave's byte as part of its aligned word: a scalar load)
  A(d.pBlk, waves4); A(d.cBlk, waves4); A(d.xBlk, waves4); A(d.k12Skip, waves); A(d.k10Skip, waves); A(d.skipGate, SPH_GATE_SLOTS);
  A(d.nbhd, waves4 * SPH_GATE_SLOTS);
  d.nbStride = (int)waves4; d.nbOut = d.nbIn = d.nbhd; d.gatePolicy = 1; d.cellTable = d.cellStart;
  A(s->blockHist, (size_t)SPH_SORT_MAX_DIGITS * s->maxSortBlocks + SPH_SORT_MAX_DIGITS);  // block histograms + digit totals
  A(d.gid, n); A(d.owned, n); A(s->slabCounts, SPH_SLAB_COUNT_WORDS);
  A(d.dbg, SPH_DBG_WORDS); A(s->chunkEdges, SPH_STEP_CHUNKS_MAX + 1); A(s->pipeTable, SPH_PIPE_TABLE_WORDS);
  float* binU = nullptr;
  A(binU, 64);
  d.binU = binU;
  if (d.hasElastic) {
    A(d.elasticMask, n); A(d.membDelta, n); A(d.elastic, (size_t)32 * d.numElastic); A(d.muscle, (size_t)d.muscleCount);
    if (membraneData && pml && cfg->numOfMembranes > 0) { A(d.membraneData, (size_t)3 * cfg->numOfMembranes); A(d.pml, (size_t)7 * d.numElastic); }
  }
#undef A
  if (rc != SPH_OK) return rc;

#define UP(dst, src, bytes) do { hipError_t e_ = hipMemcpyAsync((dst), (src), (bytes), hipMemcpyHostToDevice, s->stream); \
    if (e_ != hipSuccess) { sph_set_error("upload failed: %s", hipGetErrorString(e_)); return SPH_ERR_HIP; } } while (0)
  UP(d.posOrig, position, sizeof(float4) * nUp);
  UP(d.velOrig, velocity, sizeof(float4) * nUp);
  if (d.hasElastic) {
    UP(d.elastic, elastic, sizeof(float4) * 32 * (size_t)d.numElastic);
    // quirk #18: the reference never uploads the signal before step 0 (zeros in practice)
    hipMemsetAsync(d.muscle, 0, sizeof(float) * (size_t)d.muscleCount, s->stream);
    hipMemsetAsync(d.membDelta, 0, sizeof(float4) * n, s->stream);
    if (d.membraneData) {
      UP(d.membraneData, membraneData, sizeof(int32_t) * 3 * (size_t)cfg->numOfMembranes);
      UP(d.pml, pml, sizeof(int32_t) * 7 * (size_t)d.numElastic);
    }
  }
  {
    float U[64];
    compute_bin_thresholds(cfg->h, U);
    UP(binU, U, sizeof(U));
    s->bandRadius = sph_band_radius(d, U[63]);
  }
#undef UP
  // buffers the reference leaves uninitialised but that an export may read before they are written
  hipMemsetAsync(d.predPos, 0, sizeof(float) * 3 * n, s->stream);
  hipMemsetAsync(d.acc, 0, sizeof(float4) * n, s->stream);
  hipMemsetAsync(d.accP, 0, sizeof(float4) * n, s->stream);
  hipMemsetAsync(d.rho, 0, sizeof(float) * n, s->stream);
  hipMemsetAsync(d.rp, 0, sizeof(float2) * n, s->stream);
  for (uint8_t* f : {d.pBlk, d.cBlk, d.xBlk, d.k12Skip, d.k10Skip}) hipMemsetAsync(f, 0, waves, s->stream);  // (for a read-back before the first step: the kernels never rely on it)
  hipMemsetAsync(d.nbhd, 0, waves4 * SPH_GATE_SLOTS, s->stream);
  hipMemsetAsync(d.nbrId, 0xff, sizeof(int32_t) * mapN, s->stream);
  hipMemsetAsync(d.nbrDist, 0, sizeof(float) * mapN, s->stream);
  hipMemsetAsync(d.nbr16, 0xff, sizeof(uint16_t) * mapN, s->stream);
  hipMemsetAsync(d.nbrBase, 0, sizeof(int32_t) * (size_t)s->capTiles * 64, s->stream);
  hipMemsetAsync(d.dbg, 0, sizeof(uint32_t) * SPH_DBG_WORDS, s->stream);
  hipMemsetAsync(d.skipGate, 0, sizeof(uint32_t) * SPH_GATE_SLOTS, s->stream);
  hipMemsetAsync(d.cellStartRaw, 0, sizeof(uint32_t) * G1, s->stream);
  hipMemsetAsync(d.cellStart, 0, sizeof(uint32_t) * G1, s->stream);
  hipMemsetAsync(d.sortedPos, 0, sizeof(float4) * n, s->stream);
  hipMemsetAsync(d.sortedVel, 0, sizeof(float4) * n, s->stream);
  hipMemsetAsync(d.keys, 0, sizeof(uint32_t) * n, s->stream);
  hipMemsetAsync(d.vals, 0, sizeof(uint32_t) * n, s->stream);
  hipMemsetAsync(d.backIndex, 0, sizeof(uint32_t) * n, s->stream);
  hipError_t e = hipStreamSynchronize(s->stream);  // host arrays may be freed by the caller after return
  if (e != hipSuccess) { sph_set_error("sph_create: %s", hipGetErrorString(e)); return SPH_ERR_HIP; }
  *out = owner.release();
  return SPH_OK;
}

// ---------------------------------------------------------------------------------------------- stages
// One row per stage entry point: the progress bits it needs, the timer slot it is booked on, its launcher and the bits it gains.
struct Stage {
  const char* name;
  int need, timer;
  int (*launch)(sph_solver*);
  int gain;
};
#define LAUNCH(call) [](sph_solver* s) { return call; }
static const Stage kClearBuffers = {"sph_run_clear_buffers", 0, SPH_ST_FIND_NEIGHBORS, LAUNCH(sphk_clear_neighbors(s)), 0};
static const Stage kHashParticles = {"sph_run_hash_particles", 0, SPH_ST_HASH, LAUNCH(sphk_hash(s)), P_HASH};
static const Stage kSort = {"sph_run_sort", P_HASH, SPH_ST_SORT, LAUNCH(sphk_sort(s)), P_SORT};
static const Stage kSortPostPass = {"sph_run_sort_post_pass", P_SORT, SPH_ST_SORT_POST, LAUNCH(sphk_sort_post(s)), P_SORTPOST};
static const Stage kIndexx = {"sph_run_indexx", P_SORT, SPH_ST_INDEX, LAUNCH(sphk_index_raw(s)), P_INDEXX};
static const Stage kIndexPostPass = {"sph_run_index_post_pass", P_INDEXX, SPH_ST_INDEX, LAUNCH(sphk_index_fixed(s)), P_INDEXPOST};
static const Stage kFindNeighbors = {"sph_run_find_neighbors", P_SORTPOST | P_INDEXPOST, SPH_ST_FIND_NEIGHBORS, LAUNCH(sphk_find_neighbors(s)), P_FIND};
static const Stage kComputeDensity = {"sph_run_pcisph_compute_density", P_FIND, SPH_ST_DENSITY, LAUNCH(sphk_density(s)), P_DENSITY};
static const Stage kComputeForces = {"sph_run_pcisph_compute_forces_and_init_pressure", P_DENSITY, SPH_ST_FORCES, LAUNCH(sphk_forces(s, false)), P_FORCES};
static const Stage kElasticForces = {"sph_run_pcisph_compute_elastic_forces", P_FORCES, SPH_ST_ELASTIC, LAUNCH(sphk_elastic(s)), 0};
static const Stage kPredictPositions = {"sph_run_pcisph_predict_positions", P_FORCES, SPH_ST_PRESSURE_FORCE, LAUNCH(sphk_predict_positions(s)), P_PREDICTPOS};
static const Stage kPredictDensity = {"sph_run_pcisph_predict_density", P_PREDICTPOS, SPH_ST_PREDICT_DENSITY, LAUNCH(sphk_predict_density(s, false)), P_PREDICTDENS};
static const Stage kCorrectPressure = {"sph_run_pcisph_correct_pressure", P_PREDICTDENS, SPH_ST_PREDICT_DENSITY, LAUNCH(sphk_correct_pressure(s)), 0};
static const Stage kPressureForce = {"sph_run_pcisph_compute_pressure_force_acceleration", P_PREDICTDENS, SPH_ST_PRESSURE_FORCE, LAUNCH(sphk_pressure_force(s, 0)), P_PRESSUREFORCE};
static const Stage kIntegrate = {"sph_run_pcisph_integrate", P_FORCES, SPH_ST_INTEGRATE, LAUNCH(sphk_integrate(s)), P_INTEGRATE};
static const Stage kClearMembraneBuffers = {"sph_run_clear_membrane_buffers", 0, SPH_ST_MEMBRANES, LAUNCH(sphk_clear_membranes(s)), 0};
static const Stage kMembranes = {"sph_run_compute_interaction_with_membranes", P_FIND, SPH_ST_MEMBRANES, LAUNCH(sphk_membranes(s)), 0};
static const Stage kMembranesFinalize = {"sph_run_compute_interaction_with_membranes_finalize", 0, SPH_ST_MEMBRANES, LAUNCH(sphk_membranes_finalize(s)), 0};
#undef LAUNCH

static int run_stage(sph_solver* s, const Stage& st) {
  ENTER(s); NEED(s, st.need, st.name);
  sph_state_changes(s);
  StageTimer t(s, st.timer);
  const int rc = st.launch(s);
  if (rc == SPH_OK) s->progress = st.gain == P_HASH ? P_HASH : s->progress | st.gain;  // (a new step starts at the hash)
  // posOrig / velOrig are the solver's state again once integrate has run, or with elastic matter the membranes' finalize pass,
  // which rewrites them; the membrane stages of a solver without elastic matter are no-ops behind integrate
  const bool membraneStage = st.timer == SPH_ST_MEMBRANES;
  if (&st == &kIntegrate) s->stepOpen = s->d.hasElastic != 0;
  else if (&st == &kMembranesFinalize) s->stepOpen = false;
  else if (!membraneStage) s->stepOpen = true;
  // a new step has begun (its first stage may be clearBuffers, which gains nothing): the last integrate is no longer "this step's"
  if (&st != &kIntegrate && !membraneStage) s->progress &= ~P_INTEGRATE;
  return rc;
}

extern "C" int sph_run_clear_buffers(sph_solver* s) { return run_stage(s, kClearBuffers); }
extern "C" int sph_run_hash_particles(sph_solver* s) { return run_stage(s, kHashParticles); }
extern "C" int sph_run_sort(sph_solver* s) { return run_stage(s, kSort); }
extern "C" int sph_run_sort_post_pass(sph_solver* s) { return run_stage(s, kSortPostPass); }
extern "C" int sph_run_indexx(sph_solver* s) { return run_stage(s, kIndexx); }
extern "C" int sph_run_index_post_pass(sph_solver* s) { return run_stage(s, kIndexPostPass); }
extern "C" int sph_run_find_neighbors(sph_solver* s) { return run_stage(s, kFindNeighbors); }
extern "C" int sph_run_pcisph_compute_density(sph_solver* s) { return run_stage(s, kComputeDensity); }
extern "C" int sph_run_pcisph_compute_forces_and_init_pressure(sph_solver* s) { return run_stage(s, kComputeForces); }
extern "C" int sph_run_pcisph_compute_elastic_forces(sph_solver* s) { return run_stage(s, kElasticForces); }
extern "C" int sph_run_pcisph_predict_positions(sph_solver* s) { return run_stage(s, kPredictPositions); }
extern "C" int sph_run_pcisph_predict_density(sph_solver* s) { return run_stage(s, kPredictDensity); }
extern "C" int sph_run_pcisph_correct_pressure(sph_solver* s) { return run_stage(s, kCorrectPressure); }
extern "C" int sph_run_pcisph_compute_pressure_force_acceleration(sph_solver* s) { return run_stage(s, kPressureForce); }
// (iterationCount is only used by commented-out debug prints in the reference, sphFluid.cl:1784-1805)
extern "C" int sph_run_pcisph_integrate(sph_solver* s, int /*iterationCount*/) { return run_stage(s, kIntegrate); }
extern "C" int sph_run_clear_membrane_buffers(sph_solver* s) { return run_stage(s, kClearMembraneBuffers); }
extern "C" int sph_run_compute_interaction_with_membranes(sph_solver* s) {
  ENTER(s); NEED(s, kMembranes.need, kMembranes.name);
  if (!s->d.pml) return SPH_OK;  // no membrane lists were supplied: nothing runs and nothing changes
  return run_stage(s, kMembranes);
}
extern "C" int sph_run_compute_interaction_with_membranes_finalize(sph_solver* s) { return run_stage(s, kMembranesFinalize); }

// ---- the overlapped search. findNeighbors is bound by vector ALU issue and leaves HBM nearly idle; the density
// pass and the record pack that follow it are pure HBM streams over the particle's own rows and records. So the sorted particles
// are cut into chunks. findNeighbors(c) runs on s->stream (even c) or searchStream (odd c): the chunks do not depend on each
// other, and with two streams the tail of one launch — workgroups of the last wave of tiles running on a half-empty GPU — is
// filled by the next. density(c) and pack(c) run on chunkStream behind the event of findNeighbors(c), under the launches of the
// later chunks. Results do not depend on the chunk count: every kernel computes a particle from the same inputs whichever launch
// serves it.
// The chunk count the fused step takes when sph_set_step_chunks left it automatic, and the particle count from which it does
// (both measured, profiles/r23/README.md).
#ifndef SPH_OVERLAP_CHUNKS
#define SPH_OVERLAP_CHUNKS 16
#endif
#ifndef SPH_OVERLAP_MIN_PARTICLES
#define SPH_OVERLAP_MIN_PARTICLES (4 << 20)
#endif
static_assert(SPH_OVERLAP_CHUNKS >= 1 && SPH_OVERLAP_CHUNKS <= SPH_STEP_CHUNKS_MAX, "chunk count");
// Fewest particles for which the automatic mode of sph_set_search_bands builds bands
#ifndef SPH_BANDS_MIN_PARTICLES
#define SPH_BANDS_MIN_PARTICLES 0
#endif
// ---- the pipelined step. Where the search runs in chunks, the first D of the kernels behind it (forces; then
// predicted density and pressure force of every iteration) can follow it on chunkStream chunk by chunk, stage k one chunk behind
// stage k - 1: a stage reads of other particles only what the stage before wrote for direct neighbours, so if the neighbours of
// chunk c lie in chunks c - 1 .. c + 1 the one in-order stream orders every read after its write and every overwrite after its
// last read, and no array needs a second copy. k_halo_check tests that premise on the device every step and either way leaves two
// tables by which each stage runs exactly once per particle: chunk by chunk, or over all particles behind the join.
// The depth the step takes when sph_set_step_pipeline left it automatic is 1: the forces kernel alone. Deeper pipelines were
// measured and are slower, the whole loop (6) slower than none (profiles/r24/README.md).

extern "C" int sph_set_step_chunks(sph_solver* s, int32_t chunks) {
  ENTER(s);
  if (chunks < 0 || chunks > SPH_STEP_CHUNKS_MAX) { sph_set_error("sph_set_step_chunks: %d is not in [0, %d]", chunks, SPH_STEP_CHUNKS_MAX); return SPH_ERR_INVALID; }
  s->stepChunks = chunks;
  return SPH_OK;
}

extern "C" int sph_set_step_pipeline(sph_solver* s, int32_t depth) {
  ENTER(s);
  if (depth < -1 || depth > SPH_PIPELINE_STAGES_MAX) { sph_set_error("sph_set_step_pipeline: %d is not in [-1, %d]", depth, SPH_PIPELINE_STAGES_MAX); return SPH_ERR_INVALID; }
  s->stepPipeline = depth;
  return SPH_OK;
}

// The per-wave flags of the predict-correct loop: 0 the built-in policy (the launch-level gate), 1 the writers
// always mark and the consumers always consult, 2 the flags are off. Results do not depend on it.
extern "C" int sph_set_wave_skip(sph_solver* s, int32_t mode) {
  ENTER(s);
  if (mode < 0 || mode > 2) { sph_set_error("sph_set_wave_skip: %d is not in [0, 2]", mode); return SPH_ERR_INVALID; }
  s->waveSkipMode = mode;
  return SPH_OK;
}

// The search bands: 0 automatic, 1 off. Results do not depend on it.
extern "C" int sph_set_search_bands(sph_solver* s, int32_t mode) {
  ENTER(s);
  if (mode < 0 || mode > 1) { sph_set_error("sph_set_search_bands: %d is not in [0, 1]", mode); return SPH_ERR_INVALID; }
  s->bandsMode = mode;
  return SPH_OK;
}

// Whether this step's search may read bands. The superset proof needs keys that are cell ids (an id mask that changes no id of the grid), at least
// three cells per axis (a cell reached by an offset that crosses the grid's edge along an axis is then farther away than the search
// radius) and the 27 cell offsets distinct, also modulo G (a key difference then names one step per axis).
static bool sph_bands_apply(const sph_solver* s) {
  const SphDev& d = s->d;
  if (s->hasSlab || s->bandsMode != 0 || (unsigned long long)d.G > (unsigned long long)d.cellMask + 1ull || d.N < SPH_BANDS_MIN_PARTICLES) return false;
  if (d.gx < 3 || d.gy < 3 || d.gz < 3 || (long long)d.gx * d.gy * d.gz != (long long)d.G) return false;
  long long off[27];
  for (int k = 0; k < 27; k++) off[k] = (k % 3 - 1) + (long long)(k / 3 % 3 - 1) * d.gx + (long long)(k / 9 - 1) * d.gx * d.gy;
  for (int a = 0; a < 27; a++)
    for (int b = a + 1; b < 27; b++)
      if ((off[a] - off[b]) % (long long)d.G == 0) return false;
  return true;
}

// 1: the serial search. Slab mode launches by ghost layers; with stage timing on, the step stays the sequence of stages that
// stages_ms and the density roofline describe.
static int step_chunks(const sph_solver* s) {
  if (s->hasSlab || s->timing) return 1;
  if (s->stepChunks > 0) return s->stepChunks;
  return s->d.N >= SPH_OVERLAP_MIN_PARTICLES ? SPH_OVERLAP_CHUNKS : 1;
}

struct ChunkEdges { uint32_t e[SPH_STEP_CHUNKS_MAX + 1]; };  // (a kernel argument: no host buffer has to outlive the call)
__global__ void k_chunk_edges(uint32_t* edges, ChunkEdges v) {
  if (threadIdx.x <= SPH_STEP_CHUNKS_MAX) edges[threadIdx.x] = v.e[threadIdx.x];
}

// Stages of the chunked step that follow the search chunk by chunk (0: none; only asked where the search runs in chunks)
static int step_pipeline(const sph_solver* s) {
  return sphPipelineDepth(s->stepPipeline >= 0 ? s->stepPipeline : 1, s->cfg.maxIteration, s->d.hasElastic ? 1 : 0);
}

// The halo check of the pipelined step, one lane per chunk (sphChunkHaloOk, sphmi_chunks.h: every table index is clamped there).
// table: the pipeline table (the edges, or zeros), then the serial table {0, passed ? 0 : N}, then the serial table of the deferred
// band scatter {passed ? 0 : edge[deferFirst], passed ? 0 : N} (deferFirst == chunks: nothing is deferred, both
// empty). dbg[9] counts the steps that took the serial tables, dbg[10] those that ran chunk by chunk.
__global__ void k_halo_check(const uint32_t* keys, const uint32_t* cellStart, int G, int gx, int gy, int N, int chunks, int deferFirst,
                             ChunkEdges v, uint32_t* table, uint32_t* dbg) {
  const int c = threadIdx.x;  // one wave
  int ok = 1;
  if (c < chunks) {
    const int64_t reach = (int64_t)gx * gy + gx + 1;
    ok = sphChunkHaloOk(keys, cellStart, G, reach, N, v.e[c], v.e[c + 1], v.e[max(c - 1, 0)], v.e[min(c + 2, chunks)]);
  }
  const bool passed = __all(ok);
  if (c <= SPH_STEP_CHUNKS_MAX) table[c] = passed ? v.e[c] : 0u;
  if (c == 0) {
    table[SPH_STEP_CHUNKS_MAX + 1] = 0u;
    table[SPH_STEP_CHUNKS_MAX + 2] = passed ? 0u : (uint32_t)N;
    table[SPH_STEP_CHUNKS_MAX + 3] = passed ? 0u : v.e[min(max(deferFirst, 0), SPH_STEP_CHUNKS_MAX)];
    table[SPH_STEP_CHUNKS_MAX + 4] = passed ? 0u : (uint32_t)N;
    atomicAdd(&dbg[passed ? 10 : 9], 1u);
  }
}

// ---- the prelude under the first search chunks. Two parts of the serial prelude produce nothing that the search
// launches starting at the fork read, and run beside them:
//  * The velocity half of the gather (k_sort_post_vel: sortedVel, backIndex), first thing on chunkStream, which is otherwise idle
//    until evChunk[0]. k_find_neighbors reads neither. Their readers in stream
//    order — the record pack and the forces kernel, the stages on the serial table, k_elastic, the membrane kernels, every later
//    call — are on chunkStream behind it or on s->stream behind evChunkJoin. Write after read: it reads vals and velOrig, which are
//    next written by k_pressure_force<2> (integrate; on chunkStream behind it or behind the join) and by the next step's hash and
//    sort (s->stream, behind the join); it overwrites sortedVel and backIndex, whose readers of the step before were all joined into
//    s->stream in front of evSearchFork.
//  * The band records of the chunks from deferFirst = sphBandDeferFirst(chunks) on. Under the premise of k_halo_check findNeighbors
//    of chunk c reads records only of chunks c - 1 .. c + 1 (its runs lie between bandStart of the cells keys[lo] - S and
//    keys[hi - 1] + S + 1, and bandStart counts the entries in front of cellStart of the same cell). The prelude scatters chunks
//    [0, deferFirst); the search of a chunk c with c + 1 < deferFirst starts at the fork; every later search launch is behind the
//    deferred scatter: on searchStream in stream order (the scatter is enqueued there in front of chunk 1), on s->stream by a wait
//    for evDeferred. The check's verdict is on the device only, so the rest is enqueued twice, as the stages of the pipelined step
//    are: on s->stream in front of the fork by the serial table (empty if the check passed), and behind the fork by the pipeline
//    table (empty if it failed). Every particle is scattered once either way; the scan and k_band_start read no records
//    (sph_bands.hip).
// With two chunks in the prelude chunk 1 starts late, behind the scatter, and the two streaming kernels run beside chunk 0 alone;
// that measured faster than three chunks in the prelude and the scatter on chunkStream beside chunks 0 and 1, which the streams
// slow down by more, and faster than either part alone (profiles/r39/README.md). Results do not depend on the placement.
struct PreludeSplit {
  bool vel;        // the gather left sortedVel and backIndex to k_sort_post_vel
  int deferFirst;  // the band records of the chunks from here on are not scattered yet (== chunks: all are)
};
static PreludeSplit prelude_split(const sph_solver* s, int chunks, bool bands) {
  PreludeSplit p;
  p.vel = chunks > 1;
  p.deferFirst = (chunks > 1 && bands) ? sphBandDeferFirst(chunks) : chunks;
  // (more chunks than blocks: the deferred chunks may all be empty)
  if (sphChunkEdge(s->d.N, chunks, p.deferFirst) >= s->d.N) p.deferFirst = chunks;
  return p;
}

// depth: stages 1 .. depth run here as well (clamped by the caller), by the schedule of sphPipelineSchedule.
static int enqueue_search_overlapped(sph_solver* s, int chunks, int depth, PreludeSplit split) {
  const int N = s->d.N;
  ChunkEdges v;
  for (int i = 0; i <= SPH_STEP_CHUNKS_MAX; i++) v.e[i] = (uint32_t)sphChunkEdge(N, chunks, i);
  if (s->chunkEdgesN != N || s->chunkEdgesC != chunks) {  // the partition on the device, for sphk_density_chunk
    hipLaunchKernelGGL(k_chunk_edges, dim3(1), dim3(64), 0, s->stream, s->chunkEdges, v);
    SPH_HIP(hipGetLastError());
    s->chunkEdgesN = N; s->chunkEdgesC = chunks;
  }
  const bool deferred = split.deferFirst < chunks;
  const int deferLo = (int)v.e[split.deferFirst], deferCount = N - deferLo;
  int rc = SPH_OK;
  if (depth > 0 || deferred) {  // behind the sort and the cell table, in front of everything that reads the tables
    hipLaunchKernelGGL(k_halo_check, dim3(1), dim3(64), 0, s->stream, s->d.keys, s->d.cellStart, s->d.G, s->d.gx, s->d.gy, N, chunks,
                       split.deferFirst, v, s->pipeTable, s->d.dbg);
    SPH_HIP(hipGetLastError());
  }
  // the deferred band records where the check failed: here, in front of every search launch
  if (deferred) rc = sphk_band_scatter(s, s->pipeTable, SPH_STEP_CHUNKS_MAX + 3, SPH_STEP_CHUNKS_MAX + 4, deferCount, true, s->stream);
  // searchStream starts where s->stream stands now: behind the sort and the cell table
  SPH_HIP(hipEventRecord(s->evSearchFork, s->stream));
  SPH_HIP(hipStreamWaitEvent(s->searchStream, s->evSearchFork, 0));
  bool waited[2] = {!deferred, !deferred};  // per search stream: it has waited for evDeferred
  if (split.vel || deferred) {  // chunkStream too: what the searches at the fork do not read
    SPH_HIP(hipStreamWaitEvent(s->chunkStream, s->evSearchFork, 0));
    if (split.vel && rc == SPH_OK) rc = sphk_sort_post_vel(s, s->chunkStream);
    if (deferred) {  // on searchStream in front of its first search launch, which then needs no wait
      if (rc == SPH_OK) rc = sphk_band_scatter(s, s->pipeTable, split.deferFirst, chunks, deferCount, false, s->searchStream);
      SPH_HIP(hipEventRecord(s->evDeferred, s->searchStream));
      waited[1] = true;
    }
  }
  auto launch = [s, N, chunks, split, &waited](int stage, int c) -> int {
    const int lo = (int)sphChunkEdge(N, chunks, c), hi = (int)sphChunkEdge(N, chunks, c + 1);
    if (hi <= lo) return SPH_OK;  // more chunks than blocks of 256 particles
    if (stage > 0) return sphk_pipeline_stage(s, stage, c, lo, hi, s->chunkStream);
    hipStream_t fnStream = (c & 1) ? s->searchStream : s->stream;
    if (c + 1 >= split.deferFirst && !waited[c & 1]) {  // the chunk may read deferred band records
      SPH_HIP(hipStreamWaitEvent(fnStream, s->evDeferred, 0));
      waited[c & 1] = true;
    }
    int rc = sphk_find_neighbors(s, -1, lo, hi, fnStream, s->bandsStep);
    if (rc != SPH_OK) return rc;
    SPH_HIP(hipEventRecord(s->evChunk[c], fnStream));
    SPH_HIP(hipStreamWaitEvent(s->chunkStream, s->evChunk[c], 0));
    rc = sphk_density_chunk(s, c, lo, hi, s->chunkStream);
    return rc != SPH_OK ? rc : sphk_pack_gather_records(s, lo, hi, s->chunkStream);
  };
  // The issue order is the schedule's (depth 0: stage 0 of every chunk, the overlapped search alone), never derived here.
  int32_t stage[SPH_PIPELINE_ITEMS_MAX(SPH_STEP_CHUNKS_MAX)], chunk[SPH_PIPELINE_ITEMS_MAX(SPH_STEP_CHUNKS_MAX)];
  const int items = sphPipelineSchedule(chunks, depth, s->cfg.maxIteration, s->d.hasElastic ? 1 : 0, stage, chunk);
  for (int i = 0; i < items && rc == SPH_OK; i++) rc = launch(stage[i], chunk[i]);
  // The join, on the device, also after a failed launch. Every findNeighbors launch, on either stream, has a density launch behind
  // it on chunkStream, so chunkStream's last event covers searchStream too.
  if (deferred) SPH_HIP(hipStreamWaitEvent(s->chunkStream, s->evDeferred, 0));  // (no odd chunk may have followed it)
  SPH_HIP(hipEventRecord(s->evChunkJoin, s->chunkStream));
  SPH_HIP(hipStreamWaitEvent(s->stream, s->evChunkJoin, 0));
  // The same stages again over all particles, by the serial table: empty launches unless the halo check failed.
  for (int k = 1; k <= depth && rc == SPH_OK; k++) rc = sphk_pipeline_stage(s, k, -1, 0, N, s->stream);
  return rc;
}

// The fused fast path. Stage sequence of simulationStep() (owPhysicsFluidSimulator.cpp:88-113) with:
//   clearBuffers folded into findNeighbors; sortPostPass + indexx + index fix-up in one kernel;
//   predictPositions folded into the kernel that produces the pressure acceleration it integrates
//   (forces for iteration 0, pressure force for the later ones); correctPressure folded into predictDensity;
//   integrate folded into the last pressure-force kernel; membrane kernels skipped when there is no elastic matter
//   (their only effect, `position += 0`, is applied in integrate).
// The launches of one fused step, in order, on s->stream. `tail` (slab mode, overlapped step only): the last stage —
// pressure force + integrate, the only one whose results the halo messages carry — is launched first on the owned layers
// next to the cuts, then the messages are packed (tail->packMessages), then the remaining owned layers follow.
int enqueue_step(sph_solver* s, const StepTail* tail) {
  int rc;
  sph_state_changes(s);
#define RUN(stage, call) do { StageTimer t_(s, stage); rc = (call); if (rc != SPH_OK) return rc; } while (0)
  // Host state only, so decided in front of the gather: where the search runs in chunks, the gather and the band scatter leave to
  // chunkStream what the first search launches do not read (prelude_split; everywhere else both do all of their work here).
  const int chunks = step_chunks(s);  // > 1: no stage timers (the path is not taken with timing on)
  PreludeSplit split = {false, chunks};
  if (s->hasSlab) {
    s->bandsStep = false;  // (sph_bands_apply: never in slab mode)
    RUN(SPH_ST_SORT, sphk_hash_sort_post_slab(s));
    RUN(SPH_ST_SORT_POST, sphk_index_fixed(s));
  } else {
    // The search bands are decided in front of the gather: it writes their flags, ballots and counts beside its own outputs.
    s->bandsStep = sph_bands_apply(s);
    if (s->bandsStep) {
      rc = sph_grow_scratch(s, s->bandBuf, sphk_bands_bytes(s, nullptr));  // (the first such step allocates)
      if (rc != SPH_OK) { s->bandsStep = false; return rc; }
    }
    split = prelude_split(s, chunks, s->bandsStep);
    int bits = s->sortBits;
    bool compact = false;  // wide cell ids: only ~1/8 of the declared index space is reachable, which can save a radix pass
    RUN(SPH_ST_HASH, sphk_hash_for_step(s, &bits, &compact));
    RUN(SPH_ST_SORT, sphk_sort_pairs(s, s->d.N, bits));
    if (compact) {
      StageTimer t_(s, SPH_ST_SORT_POST);
      rc = sphk_sort_post_rekey(s, s->bandsStep, !split.vel);
      if (rc == SPH_OK) rc = sphk_index_fixed(s);
      if (rc != SPH_OK) return rc;
    } else {
      RUN(SPH_ST_SORT_POST, sphk_sort_post_and_index(s, s->bandsStep, !split.vel));
    }
  }
  // Slab mode: a stage runs only on the ghost layers its results are needed on (owned layers + depth layers per side).
  // Information travels one neighbour hop (<= 31h/30, i.e. 31/60 of a 2h cell layer) per stage, backwards from the owned
  // layers: with `left` predict-correct iterations still to come, the pressure force is needed 2*left hops out and
  // predictDensity 2*left + 1; density 1 hop; the neighbour lists as far as the first predictDensity; forces on the owned
  // layers only; the iteration-0 predicted positions one hop further than anything else (k_ghost_init: everywhere).
  const bool slab = s->hasSlab;
  const int M = s->cfg.maxIteration;
  // The rest of the search bands (scan, scatter, start tables), behind the cell table and in front of everything that forks off this stream.
  // (the records of the chunks from split.deferFirst on: enqueue_search_overlapped)
  if (s->bandsStep) RUN(SPH_ST_BANDS, sphk_build_bands(s, split.deferFirst < chunks ? (int)sphChunkEdge(s->d.N, chunks, split.deferFirst) : INT32_MAX));
  auto layersFor = [&](int hops) { return slab ? min((hops * 31 + 59) / 60, s->slab.ghostLayers) : -1; };
  const int piped = chunks > 1 ? step_pipeline(s) : 0;  // stages 1 .. piped are enqueued with the search
  // The per-wave flags of the predict-correct loop need launch ranges that start at multiples of SPH_BLOCK, so that a
  // wave is one id >> 6, and every writer of a flag finished before its first reader starts: the serial step, the chunked search
  // and the forces kernel behind it chunk by chunk. Deeper pipelines and slab mode run without them.
  // The neighbourhood bytes invert the search's cell relation with one cell per offset, which needs a grid larger than an offset.
  s->waveSkip = !slab && piped <= 1 && s->waveSkipMode != 2 && (long long)s->d.G > (long long)s->d.gx * s->d.gy + s->d.gx + 1;
  if (chunks > 1) {
    rc = enqueue_search_overlapped(s, chunks, piped, split);
    if (rc != SPH_OK) return rc;
  } else {
    RUN(SPH_ST_FIND_NEIGHBORS, sphk_find_neighbors(s, layersFor(2 * (M - 1) + 1), 0, INT32_MAX, nullptr, s->bandsStep));
    RUN(SPH_ST_DENSITY, sphk_density(s, layersFor(1)));
  }
  if (slab) RUN(SPH_ST_FORCES, sphk_ghost_init(s));
  // Outside slab mode the forces kernel is also the first predictDensity: every neighbour's iteration-0 predicted position follows
  // from the (x, v) it gathers anyway. (In slab mode the forces run on fewer layers than that predictDensity.)
  const bool densityInForces = !slab && M >= 1;
  if (piped < 1) RUN(SPH_ST_FORCES, sphk_forces(s, true, layersFor(0), densityInForces, chunks <= 1));  // (the chunks packed their records)
  if (s->d.hasElastic) RUN(SPH_ST_ELASTIC, sphk_elastic(s));
  for (int iter = 0; iter < M; iter++) {
    const int left = M - 1 - iter;  // iterations after this one
    if (piped >= 2 * iter + 2) continue;  // both stages of the iteration ran with the search
    if (piped < 2 * iter + 1) {           // (else the predicted density did)
      if (iter > 0 || !densityInForces) RUN(SPH_ST_PREDICT_DENSITY, sphk_predict_density(s, true, layersFor(2 * left + 1), iter == 0, iter));
      else RUN(SPH_ST_PREDICT_DENSITY, SPH_OK);  // the stage ran inside the forces kernel: counted (M per step, as ever), an empty interval
    }
    if (left > 0 || !tail) { RUN(SPH_ST_PRESSURE_FORCE, sphk_pressure_force(s, left == 0 ? 2 : 1, layersFor(2 * left), iter)); continue; }
    // ---- overlapped tail. A particle that ends the step within W layers of a cut started it within W + 1 layers (particles
    // move less than one layer per step — the same assumption the ghost depth rests on), so integrating the W + 1 owned
    // layers next to each cut first makes every message particle final; the pack below only looks at those.
    const long long lo = max((long long)s->slab.layerLo, 0LL), hi = min((long long)s->slab.layerHi, (long long)s->d.gz);
    const long long W1 = (long long)s->slab.ghostLayers + 1;
    const long long dEnd = s->slab.hasLower ? min(lo + W1, hi) : lo;         // [lo, dEnd): next to the lower cut
    const long long uBeg = s->slab.hasUpper ? max(hi - W1, dEnd) : hi;       // [uBeg, hi): next to the upper cut
    if (dEnd > lo) RUN(SPH_ST_PRESSURE_FORCE, sphk_pressure_force_layers(s, 2, lo, dEnd));
    if (hi > uBeg) RUN(SPH_ST_PRESSURE_FORCE, sphk_pressure_force_layers(s, 2, uBeg, hi));
    const SphDev dA = sph_ranged_layers(s, lo, dEnd), dB = sph_ranged_layers(s, uBeg, hi);
    // (cell ranges: the pack kernel turns them into sorted-index ranges with the cell table, which lives on the device)
    SlabPart part{SLAB_PART_MESSAGES, dA.rangeLo, dA.rangeHi, dB.rangeLo, dB.rangeHi};
    rc = sphk_slab_pack(s, tail->frameDown ? tail->frameDown + 1 : nullptr, tail->frameUp ? tail->frameUp + 1 : nullptr, tail->capRecords,
                        tail->frameDown, tail->frameUp, part, s->slabCounts + 4);
    if (rc != SPH_OK) return rc;
    SPH_HIP(hipMemcpyAsync(s->slabHost + 4, s->slabCounts + 4, sizeof(uint32_t) * 3, hipMemcpyDeviceToHost, s->stream));
    SPH_HIP(hipEventRecord(s->slabMsgEvent, s->stream));
    if (uBeg > dEnd) RUN(SPH_ST_PRESSURE_FORCE, sphk_pressure_force_layers(s, 2, dEnd, uBeg));
    rc = sphk_slab_pack(s, nullptr, nullptr, 0, nullptr, nullptr, SlabPart{SLAB_PART_KEPT, 0, 0, 0, 0}, s->slabCounts + 8);
    if (rc != SPH_OK) return rc;
    SPH_HIP(hipMemcpyAsync(s->slabHost + 8, s->slabCounts + 8, sizeof(uint32_t) * 3, hipMemcpyDeviceToHost, s->stream));
    SPH_HIP(hipMemcpyAsync(s->slabHost + 3, s->slabCounts + 3, sizeof(uint32_t), hipMemcpyDeviceToHost, s->stream));
    SPH_HIP(hipMemcpyAsync(s->slabHost + 7, s->slabCounts + 7, sizeof(uint32_t), hipMemcpyDeviceToHost, s->stream));
  }
  if (s->d.hasElastic) {
    RUN(SPH_ST_MEMBRANES, sphk_clear_membranes(s));
    if (s->d.pml) RUN(SPH_ST_MEMBRANES, sphk_membranes(s));
    RUN(SPH_ST_MEMBRANES, sphk_membranes_finalize(s));
  }
#undef RUN
  s->progress = P_HASH | P_SORT | P_SORTPOST | P_INDEXPOST | P_FIND | P_DENSITY | P_FORCES | P_PREDICTPOS | P_PREDICTDENS |
                P_PRESSUREFORCE | P_INTEGRATE;
  s->stepOpen = false;
  return SPH_OK;
}

extern "C" int sph_step(sph_solver* s, int iterationCount) {
  (void)iterationCount;
  ENTER(s);
  return enqueue_step(s, nullptr);
}

extern "C" int sph_update_muscles(sph_solver* s, const float* signal, int n) {
  ENTER(s);
  if (!signal || n != s->cfg.muscleCount) { sph_set_error("sph_update_muscles: n must equal muscleCount"); return SPH_ERR_SIZE; }
  if (!s->d.muscle) return SPH_OK;  // no elastic matter: nothing reads the signal
  SPH_HIP(hipMemcpyAsync(s->d.muscle, signal, sizeof(float) * (size_t)n, hipMemcpyHostToDevice, s->stream));
  SPH_HIP(hipStreamSynchronize(s->stream));  // blocking, like the reference's enqueueWriteBuffer(CL_TRUE)
  return SPH_OK;
}

extern "C" int sph_step_sort_passes(sph_solver* s) {
  ENTER(s);
  bool compact;
  return sph_sort_passes(sphk_step_sort_bits(s, &compact));
}

extern "C" int sph_synchronize(sph_solver* s) {
  ENTER(s);
  return sph_check_finite_state(s);  // (synchronises the stream)
}

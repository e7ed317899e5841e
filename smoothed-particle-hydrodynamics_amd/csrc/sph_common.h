// Internal declarations of libsphmi.so (gfx950 only). Data layout in HBM — see DESIGN.md §3.
//
//   orig order (API state)      posOrig  float4[N] (x,y,z,type)        velOrig float4[N] (vx,vy,vz,w)
//   sorted order (per step)     sortedPos float4[N] (x,y,z,type)       sortedVel float4[N]     predPos float[3N] (x,y,z)
//                               keys u32[N] (cell)  vals u32[N] (orig id)  backIndex u32[N] (orig -> sorted)
//                               rho f32[N]   rp float2[N] (rhoPred, pressure)   acc / accP float4[N]
//   neighbour map, tiled        nbr16 u16 (ids as offsets), nbrDist f32, nbrId i32 (rows nbr16 cannot hold):
//                               [tile = id/64][group = slot/4][lane = id%64][slot%4]
//                               -> one wave reads 4 slots of its 64 particles as ONE contiguous 512-B / 1-KiB transaction
//   grid                        cellStart u32[G+1]  (== gridCellIndexFixedUp: #particles with cell < c)
//
// float4 is kept for everything that other particles gather (one 16-B transaction per neighbour instead of
// three 4-B ones); pure per-particle streams (map, rho, pressure) are SoA.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "sphmi.h"
#include "sphmi_chunks.h"

#define SPH_BLOCK 256
#define SPH_TILE 64
#define SPH_MAXN 32
#define SPH_RSEG 30  // radius_segments, sphFluid.cl:116
#define SPH_DBG_WORDS 32  // diagnostic counters (SphDev::dbg)
#define SPH_SLAB_COUNT_WORDS 24
#define SPH_SORT_MAX_DIGITS 512   // radix digits per pass: 256 (8 bits) or 512 (9 bits)
#define SPH_GATE_SLOTS 16         // words of SphDev::skipGate: one per stage of the predict-correct loop (stage & 15)
#define SPH_STEP_CHUNKS_MAX 16    // most chunks the overlapped step takes (sph_set_step_chunks)
#define SPH_SERIAL_GRID 2048      // blocks of the grid-stride entry points (sphk_pipeline_stage, sphk_band_scatter); a multiple of 8, the XCD count
// words of sph_solver::pipeTable: the pipeline table, the serial table of the stages and the serial table of the deferred band scatter
#define SPH_PIPE_TABLE_WORDS (SPH_STEP_CHUNKS_MAX + 5)
static_assert(SPH_CHUNK_ALIGN == SPH_BLOCK, "chunk edges are launch-block edges of the density and pack passes");

struct SphDev {  // what the kernels see; passed by value
  int N, G;
  int gx, gy, gz;
  uint32_t cellMask;
  float h, cellSize, cellSizeInv, simScale, simScaleInv;
  float xmin, xmax, ymin, ymax, zmin, zmax;
  float r0, mass, rho0, dt, delta;
  float gravx, gravy, gravz;
  float surfTens;      // sphFluid.cl:662
  float massMu;        // (float)(mass*mu), sphFluid.cl:688
  float hs, hs2, hs6;  // hScaled, hScaled^2, hScaled^6 (float products as in sphFluid.cl:495-497)
  float posTimeStep;   // timeStep * simulationScaleInv (sphFluid.cl:928)
  float rho0delta;     // rho0*delta (sphFluid.cl:1168)
  double massWpoly6;   // ((double)mass)*Wpoly6Coefficient (sphFluid.cl:516)
  double massGradW;    // ((double)mass)*gradWspikyCoefficient (sphFluid.cl:1194)
  double del2W;        // del2WviscosityCoefficient
  double closeR;       // 0.5*(hScaled/2) as the double the comparison at sphFluid.cl:1166 uses
  float fastValueMin, fastD2Min, fastD2Max;  // operand bounds of k_pressure_force's short division / square-root path (sph_fast_bounds)
  float closeRf;       // the same test on floats: (double)r < closeR <=> r < closeRf (smallest float >= closeR)
  int rangeLo, rangeHi;  // a launch serves the sorted particles of cells [rangeLo, rangeHi): all of them ([0, G)) except in
                         // slab mode, where ghost layers that a stage's results are not needed on are skipped (sph_api.hip)
  int numElastic, elasticOffset, muscleCount, numMembranes;
  int hasElastic;      // 0: membrane kernels are no-ops and are folded into integrate
  // buffers
  float4 *posOrig, *velOrig, *membDelta;
  float4 *sortedPos, *sortedVel, *acc, *accP;
  float* predPos;    // predicted positions, packed (x, y, z): 3 floats per sorted particle
  uint32_t* elasticMask;  // bit k set: neighbour slot k holds an elastic particle (forces kernel -> membrane kernel)
  uint32_t* bndMask;  // bit k set: neighbour slot k holds a boundary particle (written by the forces kernel, read by integrate)
  float4* gatherRec; // 2 x ceil4(N) float4, groups of four particles [4 x (x,y,z,type)][4 x (v.xyz, rho)]: the forces kernel's neighbour gathers
  float2* rp;        // (rhoPred, pressure) per sorted particle: one 8-byte record, gathered per neighbour by the pressure-force kernel
  // Per-wave flags of the predict-correct loop: one byte per 64 consecutive sorted particles (index id >> 6), each
  // written with a plain store by the wave that owns those particles, in the kernel and at the point where it writes the data the
  // byte summarises. Null in every launch that does not take part (staged entry points, slab mode, pipeline depths 2-6).
  uint8_t* pBlk;     // some particle of the wave has p != 0 in rp (forces kernel at iteration 0, k_predict_density<true, *>)
  uint8_t* cBlk;     // some non-boundary particle of the wave has a valid neighbour at a stored distance < closeRf (forces kernel)
  uint8_t* xBlk;     // some particle of the wave got a predicted position whose bits differ from the one before (k_pressure_force<1>)
  // The launch-level gate in front of them: a writer of flags counts its flagged waves, from a sample of blocks (every 64th), into
  // skipGate[gateOut]; the consumer of those flags reads skipGate[gateIn] at entry and, unless the sample found nothing flagged, runs
  // without consulting anything. A heuristic: results never depend on it. The words also carry the closures the exactness of the
  // neighbourhood bytes needs: a wave that cannot name its readers adds to its stage's word, and k_cell_start sets all of them
  // in a blown-up state. The hash kernel zeroes the words. One word per stage of
  // the loop, stage & (SPH_GATE_SLOTS - 1): with maxIteration > 7 stages share words and their counts add up, which can only close
  // a gate that would have been open.
  uint32_t* skipGate;
  int gateIn, gateOut;
  // Neighbourhood bytes: what a consumer wave asks in place of its neighbours' flags. A writer wave whose pBlk (forces kernel,
  // k_predict_density) or xBlk (k_pressure_force<1>) byte is set stores a 1 for every wave that could hold a particle with a
  // neighbour in it, judged by cells as findNeighbors looks them up (mark_readers, sph_pcisph.hip). SPH_GATE_SLOTS arrays of nbStride
  // bytes in one allocation, indexed like the gate words; nbOut / nbIn are the launch's two (wave_skip_view). The hash kernel
  // zeroes them. cellTable: the real cell table (in launches of the pipelined step cellStart is the pipeline table).
  uint8_t* nbhd;
  uint8_t *nbOut, *nbIn;
  int nbStride;
  int gatePolicy;  // 1: the writers count their flagged waves into the gate (and stop marking behind a closed one); 0: they always mark
  const uint32_t* cellTable;
  uint8_t *k12Skip, *k10Skip;  // the decision of the wave in the last launch of the pressure-force / predicted-density kernel that
                               // consulted the flags: 1 = it skipped its neighbour loop (read-back only: "pressureForceSkipped", "predictDensitySkipped")
  uint32_t *keys, *vals, *keysAlt, *valsAlt, *backIndex;
  uint32_t *cellStart, *cellStartRaw;
  uint32_t *gid, *owned;  // slab decomposition: global id and ownership flag per local particle (orig order)
  int32_t* nbrId;
  float* nbrDist;
  uint16_t* nbr16;    // the ids again as 16-bit offsets (see nbr16_index / SPH_N16_*): what the PCISPH gather kernels stream
  int32_t* nbrBase;   // per sorted particle: first sorted index of its z-neighbour cell, the base of the flagged offsets
  float* rho;
  float4* elastic;
  int32_t *membraneData, *pml;
  float* muscle;
  const float* binU;  // 64 floats: [0..31] d^2 < binU[j] <=> the candidate is counted in radial-histogram bins 0..j;
                      // [32..62] pass-1 radii r_thr(jb)^2; [63] the search kernel's filter radius^2 (sph_api.hip)
  uint32_t* dbg;  // SPH_DBG_WORDS diagnostic counters (neighbour-search fallbacks etc.), zeroed by sph_reset_stage_times
};

// Search bands (sph_bands.hip). Slot s = r - (r > 4) belongs to the search kernel's row r != 4 of cells.
struct SphBandGeom {  // what the band kernels need of the step's geometry
  int N, G, gx, gy, gz, waves;  // waves = ceil(N / 64)
  int aliased;  // the id mask can change a cell id of the grid (G > mask + 1): keys are not cell ids, every particle is in every band
  float cellSize, cellSizeInv, Rb;
};
struct SphBands {  // the arrays, all in sph_solver::bandBuf
  float4* pos;               // [8][cap] records (x, y, z, sorted index as bits), each band in sorted order
  uint32_t* start;           // [8][G + 1] band entries in front of cellStart[c]
  uint8_t* flags;            // [cap] bit s: the sorted particle is in band s
  unsigned long long* mask;  // [waveStride][8] the ballot of each wave of 64 sorted particles, per band
  uint32_t* waveOff;         // [waveStride][8] counts, then exclusive offsets, per wave and band; entry ceil(N / 64): the bands' totals
  uint32_t* superCnt;        // [8][superStride] entries per 1024 waves
  int cap, waveStride, superStride;
};

// A device buffer that only grows (sph_grow_scratch) and frees itself with the solver that holds it.
struct SphScratch {
  void* p = nullptr;
  size_t bytes = 0;
  SphScratch() = default;
  SphScratch(const SphScratch&) = delete;
  SphScratch& operator=(const SphScratch&) = delete;
  ~SphScratch() { if (p) hipFree(p); }
};

// A result derived from the solver's state that a later call reads (a mesh, a labelling, a selection, an id map, an image): whether
// one exists, and the particle count and stateEpoch it was made at. Stamped, dropped and checked by sph_derived_stamp /
// sph_derived_drop / sph_derived_check (sph_api_internal.h) only.
struct SphDerived {
  bool valid = false;
  int N = 0;
  uint64_t epoch = 0;
};

struct sph_solver {
  sph_config cfg = {};
  SphDev d = {};
  // every permanent device allocation (dev_alloc, sph_api.hip): the destructor frees these, whichever SphDev member points at
  // them by then (an edit swaps posOrig / sortedPos and velOrig / sortedVel)
  std::vector<void*> allocs;
  hipStream_t stream = nullptr;
  bool ownStream = false;
  int sortBits = 0;              // significant bits of the sort key
  int capacity = 0;              // particles the buffers are sized for (>= d.N)
  int capTiles = 0;              // ceil(capacity/64)
  sph_slab slab = {}; bool hasSlab = false;
  uint32_t* slabCounts = nullptr;  // device, SPH_SLAB_COUNT_WORDS words: [0..2] kept / down / up of sph_slab_pack, [3] unsorted-message flag,
                             // [4..6] and [8..10] the same triples of the overlapped step's message / kept passes, [7] owned
                             // particles that moved more than a layer, [12..15] totals of sph_slab_rebuild_framed (kept, from
                             // below, from above, 1 = nothing merged)
  uint32_t* slabHost = nullptr;        // pinned host mirror of slabCounts (overlapped step)
  hipEvent_t slabMsgEvent = nullptr;   // recorded when the messages of the overlapped step are packed
  bool slabStepPending = false;  // sph_slab_step_begin issued, rebuild not yet done
  int slabCapRecords = 0;        // frame capacity given to sph_slab_step_begin
  int slabKept = 0;              // host copy of the kept count of the last sph_slab_pack (-1: none pending)
  int slabRecWords = 0;          // words per message record: 9 (full) or 7 (compact); 0 = 9
  uint32_t slabTypeBits = 0;     // compact records: the type word every non-boundary particle carries
  uint32_t liquidSig = 0;        // from sph_create: common position.w bits of the non-boundary particles with velocity.w == +0,
                             // 0 = there are none, 0xffffffff = not uniform
  bool slabRebuildPending = false;  // sph_slab_rebuild_framed issued: the particle count is still on its way to the host
  hipEvent_t slabRebuildEvent = nullptr;
  int slabCapDown = 0, slabCapUp = 0;  // records the frames given to sph_slab_rebuild_framed had room for
  // radix-sort workspace
  uint32_t* blockHist = nullptr;  // [SPH_SORT_MAX_DIGITS][maxSortBlocks] block histograms + SPH_SORT_MAX_DIGITS digit totals
  int maxSortBlocks = 0;
  // stage progress for SPH_ERR_ORDER checks
  int progress = 0;
  // stage timing
  bool timing = false;
  struct Pending { int stage; hipEvent_t a, b; };
  std::vector<Pending> pending;  // event pairs recorded and not yet read (resolve_pending, sph_destroy)
  double stageMs[SPH_ST_COUNT] = {};
  int64_t stageLaunches[SPH_ST_COUNT] = {};
  // asynchronous position read-back (sph_read_position_async): a copy stream of its own, ordered against s->stream by events
  hipStream_t copyStream = nullptr;
  hipEvent_t evReadReady = nullptr, evCopyDone = nullptr;  // positions final on s->stream / copy landed on the host
  // overlapped step (sph_api.hip): the findNeighbors launches of the chunks of sorted particles alternate between
  // s->stream and searchStream (which starts behind evSearchFork, recorded on s->stream); density and the record pack of chunk c
  // run on chunkStream behind evChunk[c], and behind them the stages of the pipelined step; s->stream waits for
  // evChunkJoin before the rest of the step, so nothing is pending on either stream when enqueue_step returns. Created by sph_create, destroyed with the solver.
  hipStream_t chunkStream = nullptr, searchStream = nullptr;
  hipEvent_t evChunk[SPH_STEP_CHUNKS_MAX] = {}, evChunkJoin = nullptr, evSearchFork = nullptr;
  // recorded on searchStream behind the deferred band scatter; s->stream waits for it in front of its first search launch that may
  // read those records, chunkStream in front of the join
  hipEvent_t evDeferred = nullptr;
  int stepChunks = 0;                  // sph_set_step_chunks: 0 = automatic, 1 = serial, else that many chunks
  uint32_t* chunkEdges = nullptr;      // device, SPH_STEP_CHUNKS_MAX + 1 words: the partition chunkEdgesN / chunkEdgesC was made for
  int chunkEdgesN = -1, chunkEdgesC = -1;
  // pipelined step (sph_api.hip): up to stepPipeline stages behind the search run on chunkStream chunk by chunk.
  // pipeTable, device, written every step by k_halo_check: [0 .. SPH_STEP_CHUNKS_MAX] the pipeline table (the chunk edges if the
  // halo check passed, zeros if not), then the two words of the serial table {0, passed ? 0 : N}, then the two of the deferred band
  // scatter's serial table {passed ? 0 : edge[sphBandDeferFirst], passed ? 0 : N} (SPH_PIPE_TABLE_WORDS in all)
  int stepPipeline = -1;               // sph_set_step_pipeline: -1 = the built-in depth, else that many stages
  bool waveSkip = false;               // set by enqueue_step: the fused kernels of this step write and consult the per-wave flags
                                       // (SphDev::pBlk ...); the launchers of sph_pcisph.hip hand every other launch null pointers
  int waveSkipMode = 0;                // sph_set_wave_skip: 0 the built-in policy, 1 always mark and consult, 2 flags off
  uint32_t* pipeTable = nullptr;
  // search bands (sph_bands.hip): built by enqueue_step behind the cell table where sph_bands_apply allows it
  int bandsMode = 0;                   // sph_set_search_bands: 0 automatic, 1 off
  bool bandsStep = false;              // set by enqueue_step: this step's search reads the bands (and bandBuf holds them)
  float bandRadius = 0.f;              // Rb of the bands in bandBuf
  SphScratch bandBuf;                  // grown on the first step that builds bands
  bool copyPending = false;           // a copy was issued and sph_read_position_wait has not run since
  float* copyUserDst = nullptr;        // where the caller wants the data
  void* copyStage = nullptr; size_t copyStageBytes = 0;  // pinned staging, only for destinations that cannot be page-locked in place
  bool copyViaStage = false;
  size_t copyBytes = 0;                // bytes of the read-back in flight (the particle count may change before it is waited for)
  struct HostReg { void* p; size_t bytes; };
  HostReg hostRegs[8] = {}; int numHostRegs = 0;  // caller buffers page-locked in place by hipHostRegister (released with the solver)
  uint32_t* pinnedFlags = nullptr;     // pinned: [0] copy of dbg[6] taken with the last asynchronous read-back
  uint64_t blownUp = 0;                // sticky: non-finite coordinates seen so far (sph_check_finite_state)
  // bumped by sph_state_changes (sph_api_internal.h), which every call that rewrites the sorted state or the particle set makes
  // (stages, steps, slab calls, edits): a derived result is current while its epoch still equals this
  uint64_t stateEpoch = 0;
  // device scratch of the analysis calls (sph_api_analysis.hip), each grown on demand and kept: query points and records of
  // field / gradient sampling; the diagnostics tree's partials and the histogram bins; the isosurface lattice; the last mesh
  SphScratch sampleBuf, diagBuf, surfBuf, meshBuf;
  SphDerived mesh;                            // the last successful extraction (sph_surface_normals needs it current)
  int64_t meshCounts[2] = {};                 // ... its vertices, triangles
  uint32_t meshTypeMask = 0; int meshField = 0;  // ... and its arguments (sph_surface_normals)
  float meshOrigin[3] = {}, meshSpacing[3] = {}; int32_t meshDims[3] = {};  // ... and the lattice it was cut on (sph_measure_surface)
  // surface measures (sph_measure_surface / sph_read_shells): the union-find scratch with the vertices' shell numbers, and the
  // shells' table (S x SPH_SHELL_WORDS int64, then S x 6 box words, then the call's totals)
  SphScratch shellBuf, shellTable;
  SphDerived shells;                  // the last successful measure: of the mesh alone, so steps do not stale it; an extraction drops it
  int64_t shellCounts[4] = {};        // ... its shells, closed shells, open sides, bad triangles
  // connected components (sph_label_components / sph_read_components): the labelling's scratch and table, grown on demand
  SphScratch ccBuf, ccTable;
  SphDerived cc;                      // the last successful labelling (sph_component_diagnostics needs it current)
  int64_t ccCounts[2] = {};           // ... its selected particles, components
  // particle selection (sph_select_particles / sph_read_selection): the scan's scratch (mask, block counts) and the list of
  // selected sorted indices, grown on demand; the records go through sampleBuf in pieces
  SphScratch selBuf, selList;
  SphDerived sel;                     // the last successful selection (sph_read_selection gathers from the live state)
  int64_t selCount = 0;               // ... its length
  // elastic-matter diagnostics (sph_elastic_measure / sph_muscle_diagnostics / sph_membrane_measure): records on their way to
  // the host and the group tree's partials, grown on demand
  SphScratch elasticBuf;
  // particle rendering (sph_render_particles / sph_read_render): keys, thickness sums, the resolved images and the queue of large
  // splats in one buffer, grown on demand; the images are self-contained, so no reader asks whether they are current
  SphScratch renderBuf;
  SphDerived render;                  // the last successful render; N: the particle count its buffer was laid out for
  bool renderThickness = false;       // ... it accumulated thickness
  int renderW = 0, renderH = 0;       // ... its size
  // triangle rendering (sph_render_mesh / sph_read_render_triangles): vertex records, normals, sample records and the queue of
  // large triangles in renderMeshBuf, the triangle image in renderTriBuf, both grown on demand
  SphScratch renderMeshBuf, renderTriBuf;
  bool renderHasMesh = false;         // the last render had a mesh pass: the triangle image exists
  sph_render_view renderView = {};    // the view of the last successful render (compose needs the same width .. nearPlane)
  // particle editing (sph_remove_* / sph_add_particles / sph_emit_lattice): the compaction's scan scratch, grown on demand. The
  // id map of the last removal lies in backIndex (dead until the next step's sort), or is the identity (an empty removal).
  SphScratch editBuf;
  SphDerived map;                     // stamped right after that removal (sph_read_edit_map)
  bool mapIdentity = false;
  int mapLength = 0;                  // the particle count before that removal: the map's length
  // carried particle fields (sph_field_*, sph_fields.hip): one float per particle in ORIGINAL-id order, `capacity` floats per slot.
  // A slot exists while fieldLive says so; its buffer is dropped by sph_field_release. fieldBuf: the diffusion's two sorted
  // (c, rho) records per particle and its stability word; fieldStage: the buffer a removal compacts a slot into (then swapped
  // with the slot's own)
  SphScratch fieldSlot[SPH_FIELD_SLOTS], fieldBuf, fieldStage;
  bool fieldLive[SPH_FIELD_SLOTS] = {};
  float fieldInflow[SPH_FIELD_SLOTS] = {};  // what the ids an adding call creates receive
  // tracers (sph_tracers_*, sph_trace.hip): [the advect's counter, 256 bytes][float4 x, y, z, last speed][status][steps] for
  // tracerCount tracers; independent of the particle state, so no stage, step or edit touches it
  SphScratch tracerBuf;
  int tracerCount = 0;
  // kinematic bodies (sph_body_*, sph_body.hip): per slot the members' original ids (uint32[count]) and their
  // reference rows (float4[2 count]: position, normal, position, ...); a slot is in use while its count is > 0. A definition and a
  // removal's compaction build the new arrays in the stage pair, which is then swapped with the slot's own. bodyBuf: the counters
  // of a call (256 bytes), then the two 1-bit-per-particle masks of a definition by ids or the scan scratch of a compaction.
  SphScratch bodyIds[SPH_MAX_BODIES], bodyRef[SPH_MAX_BODIES], bodyStageIds, bodyStageRef, bodyBuf;
  int bodyCount[SPH_MAX_BODIES] = {};
  // wall loads (sph_wall_*, sph_wall.hip): the call's wall set, 1 bit per sorted particle, grown on demand
  SphScratch wallBuf;
  // free bodies (sph_body_set_dynamics / sph_bodies_advance, sph_body_dynamics.hip): which slots are dynamic;
  // bodyDynBuf: one BodyDynDev (live and staged states, poses, counters, records); bodyDynScratch: the body-of-particle map (one
  // byte per sorted particle), then the load tree's partials. Both grown on demand.
  bool bodyDynamic[SPH_MAX_BODIES] = {};
  SphScratch bodyDynBuf, bodyDynScratch;
  // flow gauges (sph_gauge_* / sph_gauges_*, sph_gauge.hip): the definitions live here, on the host, and travel to the
  // kernels by value; gaugeBuf: one GaugeDev (totals and the last records); gaugeTree: the partials of every tree level;
  // gaugeHist: the history ring of gaugeHistRows rows, written for the calls from gaugeHistFirst on; gaugeScan / gaugeList: the
  // crossing list's scan scratch and the list itself (sorted index, original id, direction, t alpha beta). All grown on demand.
  sph_gauge gaugeDef[SPH_MAX_GAUGES] = {};
  bool gaugeLive[SPH_MAX_GAUGES] = {};
  int64_t gaugeCalls = 0;             // successful sph_gauges_accumulate calls so far: the index of the next one
  int gaugeHistRows = 0;
  int64_t gaugeHistFirst = 0;
  SphScratch gaugeBuf, gaugeTree, gaugeHist, gaugeScan, gaugeList;
  SphDerived gaugeCross;              // the last successful sph_gauge_crossings
  int64_t gaugeCrossCount = 0;        // ... its length
  // probes (sph_probes_*, sph_probe.hip): the point set (float4 each) and the lines as given, on the device;
  // probeCur: the records of the last call, points first, then lines; probeHist: the ring of probeHistRows rows of that layout,
  // written for the calls from probeHistFirst on. Independent of the particle state, like the tracers.
  SphScratch probePts, probeLines, probeCur, probeHist;
  int probePointCount = 0, probeLineCount = 0;
  uint32_t probeTypeMask = 0;         // of the point set
  int64_t probeCalls = 0;             // successful sph_probes_record calls so far: the index of the next one
  int probeHistRows = 0;
  int64_t probeHistFirst = 0;
  // time statistics (sph_stats_*, sph_stats.hip): per slot the lattice as given, its accumulators on the device
  // (SPH_STATS_WORDS doubles per node; the buffer exists exactly while the slot is defined) and the index of the next call.
  // statsOut: the bounded scratch sph_stats_read_moments goes through. Independent of the particle state, like the probes.
  sph_stats_lattice statsLattice[SPH_MAX_STATS] = {};
  SphScratch statsAcc[SPH_MAX_STATS], statsOut;
  int64_t statsCalls[SPH_MAX_STATS] = {};
  // binned diagnostics (sph_bin_diagnostics / sph_bin_index, sph_bins.hip): binBuf: the records, the bin tables and
  // the bin of every particle; binPool: the leaf's (chunk, bin) entries. Both grown on demand.
  SphScratch binBuf, binPool;
  // a stage-by-stage step is half done: set by every stage entry point, cleared by the stage that leaves posOrig / velOrig final
  // (integrate, or membranes-finalize with elastic matter), by sph_step and by an edit that changes the set
  bool stepOpen = false;

  sph_solver() = default;
  // Frees everything the solver owns (sph_api.hip): the recorded device allocations, then pinned buffers, host registrations,
  // events and streams; the scratch buffers free themselves after that. The caller has set the device and drained the streams.
  ~sph_solver();
};

// Called by every launcher whose kernel WRITES posOrig (integrate, membranes finalize, slab rebuild): makes s->stream wait for
// an asynchronous position read-back that is still in flight. `stream`: the stream the kernel runs on, if not s->stream.
int sph_guard_position_write(sph_solver* s, hipStream_t stream = nullptr);

void sph_set_error(const char* fmt, ...);

#define SPH_HIP(call)                                                                   \
  do {                                                                                  \
    hipError_t _e = (call);                                                             \
    if (_e != hipSuccess) {                                                             \
      sph_set_error("%s failed: %s (%s:%d)", #call, hipGetErrorString(_e), __FILE__, __LINE__); \
      return SPH_ERR_HIP;                                                               \
    }                                                                                   \
  } while (0)

static inline int sph_blocks(int n, int per = SPH_BLOCK) { return (n + per - 1) / per; }

// SphDev for a launch restricted to the owned layers plus `ghostDepth` ghost layers per side (slab mode; otherwise and
// for ghostDepth < 0 the whole particle set).
SphDev sph_ranged(const sph_solver* s, int ghostDepth);

#ifdef __HIPCC__
// id of the linear-th particle of the launch's range; false past its end
__device__ __forceinline__ bool sph_range_id(const SphDev& d, int linear, int& id) {
  const int begin = (int)d.cellStart[d.rangeLo], end = (int)d.cellStart[d.rangeHi];
  id = begin + linear;
  return id < end;
}

// XCD-aware block order: the hardware deals consecutive workgroups round-robin over the 8 XCDs; remapped, each XCD works on
// one contiguous eighth of the blocks (of the sorted particle range), and its L2 holds only that slab's neighbourhood.
__device__ __forceinline__ int xcd_block(int nblocks) {
  const int b = blockIdx.x;
  const int per = nblocks >> 3;  // blocks per XCD in the evenly divisible part
  const int even = per << 3;
  if (b >= even) return b;       // tail blocks keep their index
  return (b & 7) * per + (b >> 3);
}
#endif


// index of (sorted particle id, slot) in the tiled neighbour map
__host__ __device__ static inline size_t nbr_index(int id, int slot) {
  return ((((size_t)(id >> 6) * 8 + (size_t)(slot >> 2)) * 64 + (size_t)(id & 63)) << 2) + (size_t)(slot & 3);
}

// The neighbour ids a second time, 2 bytes each, in the layout of the other two maps ([tile = id/64][group = slot/4][lane = id%64]
// [slot%4]: same element index, so findNeighbors computes one address per entry): a wave reads 4 slots of its 64 particles as
// one contiguous 512-byte transaction and a particle's 32 ids are 64 bytes instead of 128. The three PCISPH
// gather kernels are bound by the bytes they stream per particle, and the id rows were 40-85 % of those.
//   entry = 0xFFFF                       empty slot
//   entry = flag << 15 | (j - base + SPH_N16_BIAS)   with base = (flag ? nbrBase[id] : id); 0 <= low 15 bits <= SPH_N16_MAX
//   entry 0 of a row = SPH_N16_WIDE      the row could not be encoded (an offset out of range, or the particle took the exact
//                                        walk): readers take the 32-bit row of nbrId instead
// Neighbours lie in the particle's own x-row of cells, the adjacent y-row (both within (cells per row + 2) x occupancy of the
// particle itself) or the same two rows one z layer away (within that distance of the z-neighbour cell's first particle).
#define SPH_N16_BIAS 16384
#define SPH_N16_MAX 0x7FFD
#define SPH_N16_EMPTY 0xFFFFu
#define SPH_N16_WIDE 0xFFFEu
// The sorted index in slot `slot` of particle `id` (-1: empty) from the arrays (any mix of host copies or device pointers):
// findNeighbors writes the 32-bit row only where the 16-bit one could not be written.
__host__ __device__ static inline int nbr_decode(const uint16_t* n16, const int32_t* nbase, const int32_t* n32, int id, int slot) {
  const size_t row0 = nbr_index(id, 0), at = nbr_index(id, slot);
  if (n16[row0] == SPH_N16_WIDE) return n32[at];
  const uint32_t e = n16[at];
  if (e == SPH_N16_EMPTY) return -1;
  return ((e & 0x8000u) ? nbase[id] : id) + (int)(e & 0x7fffu) - SPH_N16_BIAS;
}

// ---- launchers (each enqueues on s->stream and returns SPH_OK / SPH_ERR_HIP) ----
// sph_sort.hip
int sphk_hash(sph_solver* s);
int sphk_sort(sph_solver* s);
int sphk_sort_pairs(sph_solver* s, int n, int bits);  // stable LSD sort of (keys, vals)[0..n) by the low `bits` of keys
int sph_sort_passes(int bits);                         // radix passes sphk_sort_pairs takes for `bits` key bits (8- or 9-bit digits)
int sphk_step_sort_bits(const sph_solver* s, bool* compact);         // key bits the fused step sorts (compacted keys or the real ones)
int sphk_hash_for_step(sph_solver* s, int* sortBits, bool* compact);  // fused step: hash with compacted keys where that saves a pass
// bandFlags (both gathers): also write the first stage of the step's search bands — flags, ballots, counts (sph_band_flags.h) — into
// bandBuf, which the caller has grown; sphk_build_bands does the rest
// vel (both gathers): false leaves out sortedVel and backIndex; the caller launches sphk_sort_post_vel for them
int sphk_sort_post_rekey(sph_solver* s, bool bandFlags = false, bool vel = true);  // the gather after a sort of compacted keys (puts the real cell ids back)
int sphk_sort_post(sph_solver* s, bool bandFlags = false, bool vel = true);        // gather + backIndex (K3)
int sphk_sort_post_vel(sph_solver* s, hipStream_t stream);  // sortedVel and backIndex of every particle, from vals and velOrig, on `stream`
int sphk_index_raw(sph_solver* s);        // K4 table with -1 for empty cells
int sphk_index_fixed(sph_solver* s);      // H2 table (cellStart)
int sphk_sort_post_and_index(sph_solver* s, bool bandFlags = false, bool vel = true);  // fused K3 + K4 + H2
int sphk_hash_sort_post_slab(sph_solver* s);  // slab mode: K2 + sort + K3 with compacted sort keys (2 radix passes)
// sph_neighbors.hip
int sphk_clear_neighbors(sph_solver* s);
// [idxLo, idxHi): the sorted particles of the launch, intersected with the cell range that ghostDepth gives; the grid covers
// min(idxHi, N) - idxLo particles. On `stream` (nullptr: s->stream).
// bands: stage the eight non-own rows from this step's search bands (the caller built them: sphk_build_bands)
int sphk_find_neighbors(sph_solver* s, int ghostDepth = -1, int idxLo = 0, int idxHi = INT32_MAX, hipStream_t stream = nullptr,
                        bool bands = false);
// sph_bands.hip
size_t sphk_bands_bytes(const sph_solver* s, SphBands* out);  // bytes of bandBuf for the solver's capacity and grid; *out: the arrays in it
SphBandGeom sph_band_geom(const sph_solver* s);
float sph_band_radius(const SphDev& d, float filterR2);       // Rb from the search filter's radius^2 (binU[63])
// scan, scatter, start tables from the flags the gather left (bandFlags); on s->stream behind the cell table. scatterEnd: the
// records of the sorted particles [0, scatterEnd) only (a chunk edge); the caller scatters the rest with sphk_band_scatter
int sphk_build_bands(sph_solver* s, int scatterEnd = INT32_MAX);
// The records of the sorted particles [table[a], table[b]) — table == nullptr: [a, b) — on `stream`, behind the scan. count: the
// most particles the range can hold (sizes the grid). strided: a grid-stride launch on SPH_SERIAL_GRID blocks, for a range that is
// empty on most steps.
int sphk_band_scatter(sph_solver* s, const uint32_t* table, int a, int b, int count, bool strided, hipStream_t stream);
// sph_pcisph.hip
int sphk_density(sph_solver* s, int ghostDepth = -1);
// density and the record pack of chunk c of the partition that enqueue_search_overlapped (sph_api.hip) keeps in s->chunkEdges
// (sphChunkEdge, sphmi_chunks.h), on `stream`
int sphk_density_chunk(sph_solver* s, int c, int idxLo, int idxHi, hipStream_t stream);
int sphk_pack_gather_records(sph_solver* s, int idxLo, int idxHi, hipStream_t stream);
// packRecords: launch the record pack over all particles first (false: the caller has packed them, sphk_pack_gather_records)
int sphk_forces(sph_solver* s, bool fusePredict, int ghostDepth = -1, bool fuseDensity = false, bool packRecords = true);  // fuseDensity: + the first predictDensity
int sphk_ghost_init(sph_solver* s);  // what K7 does besides the acceleration, for every particle (slab mode)
int sphk_predict_positions(sph_solver* s);
int sphk_predict_density(sph_solver* s, bool fuseCorrect, int ghostDepth = -1, bool first = false, int iteration = 0);  // first: fused step, iteration 0
int sphk_correct_pressure(sph_solver* s);
int sphk_pressure_force(sph_solver* s, int fuse, int ghostDepth = -1, int iteration = 0);  // 0 none, 1 + predictPositions, 2 + integrate
int sphk_integrate(sph_solver* s);
// Stage `stage` (1 .. 2 * maxIteration, numbered as in sphmi_chunks.h) of the fused step outside slab mode, on `stream`: for c >= 0
// over chunk c = [idxLo, idxHi) by the pipeline table, for c < 0 over all particles by the serial table (s->pipeTable: the
// launch's blocks leave at once where k_halo_check left the table empty).
int sphk_pipeline_stage(sph_solver* s, int stage, int c, int idxLo, int idxHi, hipStream_t stream);
// sph_slab.hip
// Which part of the pack a launch does. ALL: kept set + both messages (sph_slab_pack). The overlapped step packs the MESSAGES
// as soon as the particles near the cuts (CELL ranges [a0,a1) and [b0,b1) of the sorted order) are integrated, and the KEPT set
// at the end.
enum { SLAB_PART_ALL = 0, SLAB_PART_MESSAGES = 1, SLAB_PART_KEPT = 2 };
struct SlabPart { int mode, a0, a1, b0, b1; };
int sphk_slab_pack(sph_solver* s, uint32_t* msgDown, uint32_t* msgUp, int capRecords, uint32_t* headDown = nullptr,
                   uint32_t* headUp = nullptr,  // head*: where to store the payload word count of each message (framed mode)
                   SlabPart part = SlabPart{SLAB_PART_ALL, 0, 0, 0, 0}, uint32_t* counts = nullptr);  // counts: 3 device words (default slabCounts)
SphDev sph_ranged_layers(const sph_solver* s, long long loLayer, long long hiLayer);  // launch restricted to cell layers [lo, hi)
int sphk_pressure_force_layers(sph_solver* s, int fuse, long long loLayer, long long hiLayer);
int sphk_slab_rebuild(sph_solver* s, const uint32_t* recvDown, int nDown, const uint32_t* recvUp, int nUp, int kept);  // 3-way merge
int sphk_slab_rebuild_framed(sph_solver* s, const uint32_t* frameDown, int capDown, const uint32_t* frameUp, int capUp,
                             const uint32_t* keptPtr, uint32_t* totals);  // every length read on the device; d.N is left alone
int sphk_slab_sort_rebuild(sph_solver* s, int total);  // staging area in any order -> local set sorted by global id
// sph_sample.hip (read-only on every solver array). The kernels' arguments: the constants of the sampling contract
// (include/sphmi.h), which the entry points fill, and the lattice of a grid launch, which the grid launchers fill.
struct SampleArgs {
  uint32_t typeMask;  // bits 1..3: liquid, elastic, boundary
  float hh;           // h*h, rounded to float once: the selection test r2 < hh
  float ss2;          // simScale*simScale
  float mwp;          // (float)massWpoly6
  // grid: point (i, j, k) = origin + (float)i * spacing per axis; k counts from kBase (the chunk's first z plane)
  float ox, oy, oz, sx, sy, sz;
  int nx, ny, nz, kBase;
};
int sphk_sample_points(sph_solver* s, const SampleArgs& a, const float* pts4, int count, float* out);  // device pointers
// grid z-planes [kBase, kBase + nz) of the lattice origin + (float)i * spacing; out = nz x ny x nx records (device)
int sphk_sample_grid(sph_solver* s, const SampleArgs& a, const float origin[3], const float spacing[3], int nx, int ny,
                     int kBase, int nz, float* out);
// sph_gradient.hip (the gradient records of include/sphmi.h; K = (float)(-6 * massWpoly6 * simScale)); device pointers
int sphk_gradient_points(sph_solver* s, const SampleArgs& a, float K, const float* pts4, int count, float* out);
int sphk_gradient_grid(sph_solver* s, const SampleArgs& a, float K, const float origin[3], const float spacing[3], int nx, int ny,
                       int kBase, int nz, float* out);  // as sphk_sample_grid, 32-word records
// normals[3*i..] of the `count` packed (x, y, z) vertices at verts, from the gradient of record word `field` (0..5)
int sphk_surface_normals(sph_solver* s, const SampleArgs& a, float K, int field, const float* verts, int count, float* normals);
// sph_trace.hip (integral curves of the sampled velocity; read-only on every solver array). Device pointers.
struct TraceArgs {
  float step, minSpeed;
  int maxSteps, mode, integrator;
  int hasRegion;
  float box[6];  // x0, y0, z0, x1, y1, z1, both ends inside
};
// one curve per seed, curve-major: verts = count x (maxSteps + 1) float4, zeroed by the caller; lengths, status = count words
int sphk_trace_streamlines(sph_solver* s, const SampleArgs& a, const TraceArgs& t, const float* seeds4, int count, float* verts,
                           int32_t* lengths, int32_t* status);
// one step of every moving tracer; *moving (one device word, zeroed by the caller) += the tracers still moving afterwards
int sphk_tracers_advect(sph_solver* s, const SampleArgs& a, const TraceArgs& t, float* pos4, int32_t* status, int32_t* steps,
                        int count, uint32_t* moving);
// One selection of particles: the half-open box x0, y0, z0, x1, y1, z1 (±inf: unbounded) and the types, bits 1..3. The entry
// points fill it with sph_fill_selector (sph_api_internal.h); the kernels test it with the functions of sph_selector.h.
struct SphSelector {
  float box[6];
  uint32_t typeMask;
};
// sph_diag.hip (the records and histograms of include/sphmi.h; read-only on every solver array)
struct DiagArgs {
  float box[SPH_DIAG_MAX_REGIONS][6];  // x0, y0, z0, x1, y1, z1 per region
  int count;
  uint32_t typeMask;
  float rho0;
  // component mode (sph_component_diagnostics): record r selects the particles with labels[j] == comp[r] instead of the box test
  const int32_t* labels;  // nullptr: box mode
  int32_t comp[SPH_DIAG_MAX_REGIONS];
};
struct HistArgs {
  SphSelector sel;
  int field, bins;
  float lo, hi, scale;  // scale = (float)bins / (hi - lo)
};
// scratch: tree_scratch_doubles(N, a.count, SPH_DIAG_WORDS) (sph_tree.h); *records: where the records land (in scratch)
int sphk_diagnostics(sph_solver* s, const DiagArgs& a, double* scratch, double** records);
int sphk_histogram(sph_solver* s, const HistArgs& a, uint32_t* out);  // out: bins + 2 device words
// sph_bins.hip (the diagnostics record of every bin of a lattice; read-only on every solver array)
struct BinArgs {
  float o[3], s[3];  // edge i of axis a: o[a] + (float)i * s[a]
  int n[3];
  uint32_t typeMask;
  float rho0;
};
size_t sphk_bin_scratch_bytes(int N, int B);     // records, bin tables and the N bin ids of a call over B bins
size_t sphk_bin_pool_bytes(uint32_t entries);    // the (chunk, bin) entries of the leaf
int32_t* sphk_bin_ids(void* scratch, int B);     // where the N bin ids lie in that scratch
// the bin of every sorted particle; count: also the entries per bin and their prefix sums, *total = the device word that holds
// their number
int sphk_bin_index(sph_solver* s, const BinArgs& a, int B, void* scratch, bool count, uint32_t** total);
// after sphk_bin_index(count) on the same scratch, with a pool of sphk_bin_pool_bytes(entries): *records = B records (in scratch)
int sphk_bin_records(sph_solver* s, const BinArgs& a, int B, void* scratch, void* pool, uint32_t entries, double** records);
// sph_components.hip (connected components of the neighbour graph; read-only on every solver array)
size_t sphk_components_scratch_bytes(int N);             // parent and labels (4 B per particle each), the scan's block totals
int32_t* sphk_components_labels(void* scratch, int N);   // where the N labels lie in that scratch
// init, hook, flatten, count: *totals = 3 device words {selected particles, components, error flags of the bounded walks}
int sphk_components_link(sph_solver* s, uint32_t typeMask, bool finite, float link2, void* scratch, uint32_t** totals);
// after sphk_components_link on the same scratch: labels, and the table of C rows of 8 words (root, n, bbox as floats)
int sphk_components_number(sph_solver* s, void* scratch, int C, int32_t* table);
// The steps of that sequence that do not depend on what the nodes and edges are (sph_shells.hip runs them on the mesh's vertices).
// N nodes, parent[x] < 0: not a node. compress: pointer jumping on a forest no hook is running on. flatten_count: parent[x] = root
// of x, then totals = {nodes, roots, err[0]} and off[b] = roots in the 256-node blocks before b (blockTot: 8 B per block).
// label: labels[x] = labels[parent[x]] for the non-roots (the roots' labels are the caller's), -1 for a non-node.
int sphk_uf_compress(sph_solver* s, int N, int32_t* parent, uint32_t* err);
int sphk_uf_flatten_count(sph_solver* s, int N, int32_t* parent, void* blockTot, uint32_t* off, uint32_t* err, uint32_t* totals);
int sphk_uf_label(sph_solver* s, int N, const int32_t* parent, int32_t* labels);

// sph_shells.hip (shells, open sides, area, volume and area moments of the extracted mesh; read-only on the mesh)
struct ShellArgs {
  int V, T;
  const float* verts;    // V x 3
  const int32_t* tris;   // T x 3
  double origin[3];      // (double) of the lattice origin
  int kA, kV, kM;        // the quantisation exponents
  double limit;          // 2^(62 - bT): a triangle with a scaled term not below it in magnitude is bad
};
size_t sphk_shells_scratch_bytes(int V);                // parent, labels (4 B per vertex each), the side sums (8 B), the scan's block words
int32_t* sphk_shells_labels(void* scratch, int V);      // where the V shell numbers lie in that scratch
size_t sphk_shells_table_bytes(int S);                  // S x (SPH_SHELL_WORDS x 8 + 24) B and the totals
float* sphk_shells_bbox(void* table, int S);            // where the S x 6 box words lie in the table allocation
int64_t* sphk_shells_totals(void* table, int S);        // {closed shells, open sides, bad triangles} after sphk_shells_number
// parents of the vertices under the triangles' sides, flattened; *totals (device) = {V, shells, error flags}
int sphk_shells_link(sph_solver* s, const ShellArgs& a, void* scratch, uint32_t** totals);
// after sphk_shells_link on the same scratch: the shell numbers, the table's S rows and boxes, the totals
int sphk_shells_number(sph_solver* s, const ShellArgs& a, void* scratch, int S, void* table);
// sph_select.hip (particle selection, surface measure and compact read-back; read-only on every solver array)
struct SelectArgs {
  SphSelector sel;
  int termCount;
  int field[SPH_SELECT_MAX_TERMS];
  float lo[SPH_SELECT_MAX_TERMS], hi[SPH_SELECT_MAX_TERMS];
  int component;          // -1: any
  const int32_t* labels;  // the current labelling (component >= 0)
  float ss2;              // simScale*simScale, one float (the sampling contract's)
  int needRow, needMeasure;  // a term on field 3 or 7 / on field 7: the surviving lanes walk their row
};
size_t sphk_select_scratch_bytes(int N);  // the 1-bit mask (8 B per 64 particles), block counts and offsets (8 B per 256), totals
// flags + scan: *totals = 2 device words, the number of selected particles
int sphk_select_count(sph_solver* s, const SelectArgs& a, void* scratch, uint32_t** totals);
int sphk_select_scatter(sph_solver* s, void* scratch, uint32_t total, int32_t* list);  // after sphk_select_count, same scratch
// records (SPH_SELECT_WORDS floats each, 16-byte aligned) and original ids of list[0..n); device pointers
int sphk_select_gather(sph_solver* s, float ss2, const int32_t* list, int n, float* records, uint32_t* origId);
int sphk_particle_measure(sph_solver* s, float ss2, int first, int n, float* out);  // out[r] = m of sorted particle first + r
// where the pieces of the scan lie in its scratch (bytes from its start): mask[4 nb] (64-bit ballots) | blockCnt[nb] | off[nb] | totals (256 bytes)
struct SelLayout {
  size_t mask, blockCnt, off, totals, bytes;
  int nb;
};
SelLayout sphk_select_layout(int N);
int sphk_select_scan(sph_solver* s, void* scratch, int N);  // off = exclusive offsets of blockCnt, totals[0..1] = its sum
// sph_edit.hip (adding and removing particles between steps; acts on the original-order state posOrig / velOrig)
struct EditLattice {
  float ox, oy, oz, sx, sy, sz;
  int nx, ny, nz;
  float vx, vy, vz, typeValue;
  int wide;  // wide cell ids: a point outside the box fails
  float xmin, xmax, ymin, ymax, zmin, zmax;
};
size_t sphk_edit_scratch_bytes(int N);  // the selection scan's layout and size
int sphk_edit_mark_region(sph_solver* s, const SphSelector& a, void* scratch);  // type and box only (posOrig has no keys); writes every mask word
int sphk_edit_clear_marks(sph_solver* s, void* scratch);
// or-s the marks of ids[0..count) (list == nullptr) or of vals[list[0..count)] into the mask; device pointers
int sphk_edit_mark_ids(sph_solver* s, const uint32_t* ids, const int32_t* list, int count, void* scratch);
// survivors per block + scan: *totals = device words {survivors, 0, lowest marked id < protectEnd or 0xffffffff}
int sphk_edit_count(sph_solver* s, int protectEnd, void* scratch, uint32_t** totals);
// after sphk_edit_count, same scratch: the survivors of posOrig / velOrig in order into posOut / velOut, map[old id] = new id or -1
int sphk_edit_scatter(sph_solver* s, void* scratch, uint32_t total, float4* posOut, float4* velOut, int32_t* map);
// lattice points into posOrig / velOrig [N, N + count); *counters = device words {points that fail validation, the lowest such k}
int sphk_edit_emit(sph_solver* s, const EditLattice& a, int count, void* scratch, uint32_t** counters);
// sph_body.hip (kinematic bodies; acts on the original-order state posOrig / velOrig). Device pointers.
struct BodyPose {
  float m[12];  // row-major 3 x 4, (R | t)
  int wide;     // wide cell ids: a position outside the box fails
  float xmin, xmax, ymin, ymax, zmin, zmax;
};
size_t sphk_body_check_bytes(int N);  // the counters and the two masks of sphk_body_check_ids
// *counters = device words {offending entries of ids[0..count), the lowest offending index or 0xffffffff}
int sphk_body_check_ids(sph_solver* s, const uint32_t* ids, int count, void* scratch, uint32_t** counters);
// blockCnt of the selection layout from the mask sphk_edit_mark_region wrote (marked particles per block), then its scan:
// *totals = 2 device words, the number of marked particles; sphk_select_scatter then lists them in ascending id
int sphk_body_count_marks(sph_solver* s, void* scratch, uint32_t** totals);
int sphk_body_gather(sph_solver* s, const uint32_t* ids, int count, float4* ref);  // ref[2k], ref[2k+1] = posOrig, velOrig [ids[k]]
// *counters = device words {members whose new position fails, the lowest such member or 0xffffffff, the bits of max d2}
int sphk_body_pose_validate(sph_solver* s, const BodyPose& a, const uint32_t* ids, const float4* ref, int count, uint32_t* counters);
int sphk_body_pose_commit(sph_solver* s, const BodyPose& a, const uint32_t* ids, const float4* ref, int count);
size_t sphk_body_compact_bytes(int count);  // the counters and the scan scratch of sphk_body_compact for a body of `count` members
// members whose map[id] >= 0, in order, with their rows: idsOut / refOut (room for `count`); *totals = device word, their number
int sphk_body_compact(sph_solver* s, const uint32_t* ids, const float4* ref, int count, const int32_t* map, int oldN, void* scratch,
                      uint32_t* idsOut, float4* refOut, uint32_t** totals);
// sph_body_dynamics.hip (free bodies: the fused per-body load, the rigid-body step and the pose from device memory)
struct BodyDynSlot {
  sph_body_dynamics p;  // parameters and state, as the caller's struct (q normalised)
  uint32_t advances, pad;
};
struct BodyDynDev {  // everything of the feature that lives on the device, one allocation
  BodyDynSlot live[SPH_MAX_BODIES], staged[SPH_MAX_BODIES];
  BodyPose pose[SPH_MAX_BODIES];          // the pose of the advance in flight
  uint32_t counters[SPH_MAX_BODIES][4];   // its validation: offenders, lowest failing member, bits of max d2
  double record[SPH_MAX_BODIES][SPH_BODY_STATE_WORDS];
  uint32_t overlap[2];                    // sph_body_set_dynamics: shared members, the lowest shared id
};
struct BodyDynSet {  // the bodies of a launch, by value
  uint32_t dynMask;  // bit b: slot b is dynamic
  int count[SPH_MAX_BODIES];
  const uint32_t* ids[SPH_MAX_BODIES];
  const float4* ref[SPH_MAX_BODIES];
};
size_t sphk_bdyn_scratch_bytes(int N);  // the map and every tree level's partials
// D->overlap = {members of `slot` that are members of another body of set.dynMask, the lowest such original id or 0xffffffff};
// seen: N bits, cleared here
int sphk_bdyn_overlap(sph_solver* s, const BodyDynSet& set, int slot, unsigned long long* seen, BodyDynDev* D);
// one advance of every body of set.dynMask, enqueued on s->stream: map, fused load, tree, integrate, validate, commit, finish
int sphk_bdyn_advance(sph_solver* s, const BodyDynSet& set, const BodyPose& box, void* scratch, BodyDynDev* D);
// sph_gauge.hip (flow gauges: crossings of oriented gates between the sorted state and the current one; read-only on
// every solver array)
struct GaugeOne {  // what sph_gauge_define derived, in double (include/sphmi.h)
  double o[3], n[3], A[3], B[3];
  const float* field;  // the gauge's carried field in original-id order, or null
  uint32_t typeMask, plane;
};
struct GaugeSet {  // the gauges of a launch, by value: the kernels read them through scalar loads
  uint32_t defMask;  // bit g: slot g is defined
  GaugeOne g[SPH_MAX_GAUGES];
};
struct GaugeDev {  // everything of the feature that lives on the device besides tree, ring and list; one allocation
  double totals[SPH_MAX_GAUGES][SPH_GAUGE_TOTAL_WORDS];
  double record[SPH_MAX_GAUGES][SPH_GAUGE_WORDS];
};
size_t sphk_gauge_tree_bytes(int N);  // the partials of every tree level
int sphk_gauge_clear(sph_solver* s, GaugeDev* D, uint32_t slots);  // the totals of the slots in the mask: words 0..16 +0.0, 17..19 -1
// record, totals and history row of call `call`, enqueued on s->stream; hist: the ring of `rows` rows, or null
int sphk_gauges_accumulate(sph_solver* s, const GaugeSet& set, double* tree, GaugeDev* D, double* hist, int rows, int64_t call);
// the counted crossings of gauge g into the selection scan's layout at `scratch` (mask, block counts, scan): *totals = 2 device words
int sphk_gauge_mark(sph_solver* s, const GaugeOne& g, void* scratch, uint32_t** totals);
// after sphk_gauge_mark and sphk_select_scatter: original id, direction and (t, alpha, beta) of list[0..n)
int sphk_gauge_list(sph_solver* s, const GaugeOne& g, const int32_t* list, int n, uint32_t* origId, int32_t* direction, float* tab3);
// sph_probe.hip (probes: point samples and water levels on lines; read-only on every solver array). Device pointers;
// cur / row: where the launch's first record goes in the current-record buffer and in the ring's row (row may be null). `a` as for
// sphk_sample_points; the level kernel takes each line's own typeMask.
int sphk_probe_points(sph_solver* s, const SampleArgs& a, const float* pts4, int count, float* cur, float* row);
int sphk_probe_levels(sph_solver* s, const SampleArgs& a, const sph_probe_line* lines, int count, float* cur, float* row);
// sph_stats.hip (time statistics on a lattice; read-only on every solver array). Device pointers. acc: the slot's
// SPH_STATS_WORDS doubles per node; `a` as for sphk_sample_points with the lattice's typeMask; call: the slot's call index.
int sphk_stats_accumulate(sph_solver* s, const SampleArgs& a, const sph_stats_lattice& g, int64_t call, double* acc);
int sphk_stats_init(sph_solver* s, double* acc, int64_t nodes);  // the empty values
// the SPH_STATS_MOMENT_WORDS floats of `count` nodes from `node` on, after `calls` calls
int sphk_stats_moments(sph_solver* s, const double* node, int64_t count, int64_t calls, float* out);
// sph_fields.hip (carried particle fields: paint, diffuse along the neighbour rows, reduce). `field`: a slot's
// values in original-id order (device). Read-only on every solver array.
size_t sphk_field_scratch_bytes(int N);  // two float2 records per particle (ping-pong) and the stability word
// `substeps` Jacobi substeps of the diffusion contract on `field`; *sigma: one device word, the bits of the stability number
int sphk_field_diffuse(sph_solver* s, float* field, float coefficient, int substeps, uint32_t typeMask, void* scratch, uint32_t** sigma);
// field[o] = value for the particles sph_remove_region would mark; *count (one device word) += their number
int sphk_field_paint_region(sph_solver* s, float* field, const SphSelector& a, float value, uint32_t* count);
int sphk_field_paint_list(sph_solver* s, float* field, const int32_t* list, int n, float value);  // field[vals[list[r]]] = value
int sphk_field_compact(sph_solver* s, const float* in, const int32_t* map, int nOld, float* out);  // out[map[o]] = in[o], map[o] >= 0
int sphk_field_fill(sph_solver* s, float* field, int first, int n, float value);
// scratch: tree_scratch_doubles(N, a.count, SPH_FIELD_DIAG_WORDS) (sph_tree.h); *records: where the records land (in scratch)
int sphk_field_diagnostics(sph_solver* s, const float* field, const DiagArgs& a, double* scratch, double** records);
// sph_elastic_measure.hip (spring strain, muscle groups, membrane areas; read-only on every solver array)
// per elastic particle, device pointers, any of the four may be null; *bad: one device word of error flags (ids out of range)
int sphk_elastic_measure(sph_solver* s, int32_t* sortedIndex, uint32_t* origId, float* records, float* connections, uint32_t* bad);
size_t sphk_group_tree_doubles(long long terms, int groups);  // scratch of the two calls below for `terms` slots / triangles
// *records: (muscleCount + 1) x SPH_MUSCLE_WORDS doubles, directly followed by the error flags as one double
int sphk_muscle_diagnostics(sph_solver* s, double* scratch, double** records);
// out: numMembranes x 8 floats (device) or null; *top: 16 doubles (word 0 count, 2 area sum, 7 min, 8 max), directly followed by
// an 8-byte cell whose low word holds the error flags
int sphk_membrane_measure(sph_solver* s, float* out, double* scratch, double** top);
// sph_render.hip (depth, id, colour and thickness images of the particles; read-only on every solver array)
struct RenderArgs {
  sph_render_view view;
  SphSelector sel;
  float inv;              // 1.0f / (hi - lo), one float (colour mode 2)
  const int32_t* labels;  // the current labelling (colour mode 3)
};
// where the pieces of a render lie in its buffer (bytes from its start); thick / thickOut are 0 without thickness
struct RenderLayout { size_t head, keys, thick, depth, index, origId, rgba, thickOut, queue, bytes; };
RenderLayout sphk_render_layout(int width, int height, bool thickness, int N);
// clear, splat, drain the queue of large splats, resolve; head words afterwards: [0] particles drawn, [1] covered pixels
int sphk_render(sph_solver* s, const RenderArgs& a, bool thickness, void* buf);
// sph_render_mesh.hip (triangles into the same images, fresh or composed by depth; read-only on every solver array)
struct RmVertex { int32_t X, Y; float zi; int32_t usable; };  // snapped screen position (1/256 pixel), 1/cz (perspective) or cz
struct RenderMeshArgs {
  sph_render_view view;
  int source, shading, colourMode, field, compose;
  float lo, inv;      // inv = 1.0f / (hi - lo), one float (colour mode 1)
  float colour[3];
  int V, T;           // vertices (source 1: 3 per membrane triangle, in table order) and triangles
};
// where the pieces of a mesh pass lie in its scratch (bytes from its start); normals / points / records are 0 when not asked for
struct RenderMeshLayout { size_t head, vtx, attr, normals, points, records, queue, bytes; };
RenderMeshLayout sphk_render_mesh_layout(int64_t V, int64_t T, bool normals, bool samples);
int sphk_render_mesh_points(sph_solver* s, int V, const float* verts, float* pts4);  // packed (x, y, z) -> (x, y, z, 0) query points
// clear, vertex pass, raster, drain, resolve into the images laid out by I at `images` (keys reused) and the triangle image. verts /
// tris: the mesh (source 0; source 1 reads the solver's tables). Head words afterwards: [0] drawn, [1] skipped, [3] error flags,
// [4] pixels the mesh holds, [5] covered pixels
int sphk_render_mesh(sph_solver* s, const RenderMeshArgs& a, const float* verts, const int32_t* tris, void* scratch,
                     const RenderMeshLayout& L, const RenderLayout& I, void* images, int32_t* triangleImage);
// sph_forces.hip (the K7 / K12 accelerations by the class of the neighbour that exerted them; read-only on every
// solver array). Device pointers.
// records (SPH_FORCE_WORDS floats each, 16-byte aligned) of the sorted particles first .. first + n, or of list[0..n) if given
int sphk_force_records(sph_solver* s, int first, int n, const int32_t* list, float* out);
#define FM_TERMS 48  // words 1..48 of a region record (word 0 counts the particles)
// the particles go through `terms` (terms_bytes(FM_TERMS, pieceChunks), sph_tree.h) in pieces of pieceChunks chunks; scratch:
// tree_scratch_doubles(N, a.count, SPH_FORCE_DIAG_WORDS); *records: where the records land (in scratch)
int sphk_force_diagnostics(sph_solver* s, const DiagArgs& a, float* terms, int pieceChunks, double* scratch, double** records);
// sph_wall.hip (what a set of boundary particles did to each particle in integrate, K7 and K12; read-only on every
// solver array). Device pointers. mask: 1 bit per SORTED particle (sphk_wall_mask_bytes), null = every boundary particle;
// inverted: the set is the boundary particles whose bit is clear.
size_t sphk_wall_mask_bytes(int N);
int sphk_wall_mask_clear(sph_solver* s, uint32_t* mask);
int sphk_wall_mask_add(sph_solver* s, const uint32_t* origIds, int count, uint32_t* mask);  // or-s the bits of backIndex[origIds[..]]
// records (SPH_WALL_WORDS floats each, 16-byte aligned) of the sorted particles first .. first + n, or of list[0..n) if given
int sphk_wall_records(sph_solver* s, const uint32_t* mask, bool inverted, int first, int n, const int32_t* list, float* out);
#define WL_TERMS 26  // words 1..26 of a region record (word 0 counts the particles)
// as sphk_force_diagnostics, with WL_TERMS and SPH_WALL_DIAG_WORDS
int sphk_wall_diagnostics(sph_solver* s, const uint32_t* mask, bool inverted, const DiagArgs& a, float* terms, int pieceChunks,
                          double* scratch, double** records);
// sph_surface.hip (marching cubes over a scalar lattice of P = dims[0]*dims[1]*dims[2] <= 2^31-1 points)
size_t sphk_surface_scratch_bytes(long long P);  // the lattice scratch; its first P floats are the field
int sphk_surface_field(sph_solver* s, const float* records, int word, int n, float* field);  // word of n sample records
// classify + scan; blocks until totals (vertices, triangles) are on the host
int sphk_surface_count(sph_solver* s, void* scratch, const int dims[3], float iso, unsigned long long* totals);
int sphk_surface_emit(sph_solver* s, void* scratch, const int dims[3], float iso, const float origin[3], const float spacing[3],
                      float* verts, int32_t* tris);  // after sphk_surface_count, on the same scratch
// sph_elastic.hip
int sphk_elastic(sph_solver* s);
int sphk_clear_membranes(sph_solver* s);
int sphk_membranes(sph_solver* s);
int sphk_membranes_finalize(sph_solver* s);

// owHIPSolver.h — the reference's `owOpenCLSolver` (src/owOpenCLSolver.h:28-62) re-implemented over the C ABI of
// libsphmi.so. Same constructor, same method names, same return/exception behaviour, so owPhysicsFluidSimulator.cpp
// needs only `#include "owHIPSolver.h"` and `typedef owHIPSolver owOpenCLSolver;`.
//
// Differences that the C ABI makes explicit: the globals the reference reads (PARTICLE_COUNT, numOfElasticP, delta, box
// macros ...) arrive in a `sph_config`; `particleMembranesList_cpp` is NOT freed by the solver.
#pragma once
#include <stdexcept>
#include <string>
#include <vector>

#include "sphmi.h"
#include "sphmi_host.h"

class owHIPSolver {
 public:
  owHIPSolver(const sph_config& cfg, const float* position_cpp, const float* velocity_cpp,
              const float* elasticConnectionsData_cpp = nullptr, const int* membraneData_cpp = nullptr,
              const int* particleMembranesList_cpp = nullptr)
      : cfg_(cfg), s_(nullptr) {
    // owOpenCLSolver.cpp:88-91: setup failures surface as std::exception ("ERROR: ..." + exit(-1) in the caller)
    check(sph_create(&cfg_, position_cpp, velocity_cpp, elasticConnectionsData_cpp, membraneData_cpp,
                     particleMembranesList_cpp, &s_), "sph_create");
  }
  // The same from containers, whose lengths are checked against the counts in cfg first (the C ABI and the constructor above see
  // pointers only): 4 N floats of position and velocity, 4 * 32 * numOfElasticP, 3 * numOfMembranes, 7 * numOfElasticP. An empty
  // vector stands for "not given".
  owHIPSolver(const sph_config& cfg, const std::vector<float>& position, const std::vector<float>& velocity,
              const std::vector<float>& elasticConnections = {}, const std::vector<int>& membraneData = {},
              const std::vector<int>& particleMembranesList = {})
      : cfg_(cfg), s_(nullptr) {
    expect(position.size(), 4 * (long long)cfg.particleCount, "position", "4*particleCount");
    expect(velocity.size(), 4 * (long long)cfg.particleCount, "velocity", "4*particleCount");
    if (!elasticConnections.empty()) expect(elasticConnections.size(), 4LL * 32 * cfg.numOfElasticP, "elasticConnectionsData", "4*32*numOfElasticP");
    if (!membraneData.empty()) expect(membraneData.size(), 3LL * cfg.numOfMembranes, "membraneData", "3*numOfMembranes");
    if (!particleMembranesList.empty()) expect(particleMembranesList.size(), 7LL * cfg.numOfElasticP, "particleMembranesList", "7*numOfElasticP");
    check(sph_create(&cfg_, position.data(), velocity.data(), elasticConnections.empty() ? nullptr : elasticConnections.data(),
                     membraneData.empty() ? nullptr : membraneData.data(),
                     particleMembranesList.empty() ? nullptr : particleMembranesList.data(), &s_), "sph_create");
  }
  ~owHIPSolver() { sph_destroy(s_); }
  owHIPSolver(const owHIPSolver&) = delete;
  owHIPSolver& operator=(const owHIPSolver&) = delete;

  // PCISPH kernels for data structures support and management — owOpenCLSolver.h:37-43. The reference returns the
  // cl_int of the enqueue (0 = OK) and callers ignore it; here: the sph_status.
  unsigned int _runClearBuffers() { return (unsigned)sph_run_clear_buffers(s_); }
  unsigned int _runHashParticles() { return (unsigned)sph_run_hash_particles(s_); }
  unsigned int _runSort() { return (unsigned)sph_run_sort(s_); }
  unsigned int _runSortPostPass() { return (unsigned)sph_run_sort_post_pass(s_); }
  unsigned int _runIndexx() { return (unsigned)sph_run_indexx(s_); }
  unsigned int _runIndexPostPass() { return (unsigned)sph_run_index_post_pass(s_); }
  unsigned int _runFindNeighbors() { return (unsigned)sph_run_find_neighbors(s_); }
  // PCISPH kernels for physics-related calculations — owOpenCLSolver.h:45-52
  unsigned int _run_pcisph_computeDensity() { return (unsigned)sph_run_pcisph_compute_density(s_); }
  unsigned int _run_pcisph_computeForcesAndInitPressure() { return (unsigned)sph_run_pcisph_compute_forces_and_init_pressure(s_); }
  unsigned int _run_pcisph_computeElasticForces() { return (unsigned)sph_run_pcisph_compute_elastic_forces(s_); }
  unsigned int _run_pcisph_predictPositions() { return (unsigned)sph_run_pcisph_predict_positions(s_); }
  unsigned int _run_pcisph_predictDensity() { return (unsigned)sph_run_pcisph_predict_density(s_); }
  unsigned int _run_pcisph_correctPressure() { return (unsigned)sph_run_pcisph_correct_pressure(s_); }
  unsigned int _run_pcisph_computePressureForceAcceleration() { return (unsigned)sph_run_pcisph_compute_pressure_force_acceleration(s_); }
  unsigned int _run_pcisph_integrate(int iterationCount) { return (unsigned)sph_run_pcisph_integrate(s_, iterationCount); }
  // owOpenCLSolver.h:54-56
  unsigned int _run_clearMembraneBuffers() { return (unsigned)sph_run_clear_membrane_buffers(s_); }
  unsigned int _run_computeInteractionWithMembranes() { return (unsigned)sph_run_compute_interaction_with_membranes(s_); }
  unsigned int _run_computeInteractionWithMembranes_finalize() { return (unsigned)sph_run_compute_interaction_with_membranes_finalize(s_); }
  // owOpenCLSolver.h:58
  unsigned int updateMuscleActivityData(float* _muscle_activation_signal_cpp) {
    return (unsigned)sph_update_muscles(s_, _muscle_activation_signal_cpp, cfg_.muscleCount);
  }
  // owOpenCLSolver.h:60-62 — copy failures throw std::runtime_error there (owOpenCLSolver.cpp:727-736)
  void read_position_buffer(float* position_cpp) { check(sph_read_position(s_, position_cpp), "read_position_buffer"); }
  // The same read without the wait (sph_read_position_async): the 16N-byte copy runs on its own stream under the NEXT step's
  // kernels and position_cpp is complete after wait_position_buffer() — call that where the data is consumed (the reference:
  // owPhysicsFluidSimulator::getPosition_cpp(), which the viewer calls once per frame). position_cpp is page-locked in place on
  // first use. INTEGRATION.md §1 shows the two lines.
  void read_position_buffer_async(float* position_cpp) { check(sph_read_position_async(s_, position_cpp), "read_position_buffer_async"); }
  void wait_position_buffer() { check(sph_read_position_wait(s_), "wait_position_buffer"); }
  void read_density_buffer(float* density_cpp) { check(sph_read_density(s_, density_cpp), "read_density_buffer"); }
  void read_particleIndex_buffer(unsigned int* particleIndexBuffer) {
    check(sph_read_particle_index(s_, particleIndexBuffer), "read_particleIndex_buffer");
  }
  // beyond the reference: the search bands of the fused step (sph_set_search_bands): 0 automatic, 1 off; results do not depend on it
  void setSearchBands(int mode) { check(sph_set_search_bands(s_, mode), "setSearchBands"); }

  // beyond the reference: SPH interpolation over the sorted state of the last completed step (include/sphmi.h, sph_sample_*);
  // out holds count x SPH_SAMPLE_WORDS / dims[2] x dims[1] x dims[0] x SPH_SAMPLE_WORDS floats. typeMask bits: 1 liquid, 2 elastic, 3 boundary
  void samplePoints(const float* points4, int count, unsigned int typeMask, float* out) {
    check(sph_sample_points(s_, points4, count, typeMask, out), "samplePoints");
  }
  void sampleGrid(const float origin[3], const float spacing[3], const int dims[3], unsigned int typeMask, float* out) {
    check(sph_sample_grid(s_, origin, spacing, dims, typeMask, out), "sampleGrid");
  }
  // beyond the reference: marching-cubes isosurface of word `field` (0..5) of sampleGrid's records (include/sphmi.h,
  // sph_extract_surface); counts = {vertices, triangles}; readSurface copies the mesh (vertices x 3 floats, triangles x 3 ints)
  void extractSurface(const float origin[3], const float spacing[3], const int dims[3], unsigned int typeMask, int field, float iso,
                      int64_t counts[2]) {
    check(sph_extract_surface(s_, origin, spacing, dims, typeMask, field, iso, counts), "extractSurface");
  }
  void readSurface(float* vertices, int32_t* triangles) { check(sph_read_surface(s_, vertices, triangles), "readSurface"); }
  // beyond the reference: SPH gradients, vorticity, divergence and Q at points / on sampleGrid's lattice (include/sphmi.h,
  // sph_sample_gradient_*; SPH_GRADIENT_WORDS floats per record), and unit vertex normals of the last extractSurface mesh
  // (counts[0] x 3 floats; refused once the solver has stepped since the extraction)
  void sampleGradientPoints(const float* points4, int count, unsigned int typeMask, float* out) {
    check(sph_sample_gradient_points(s_, points4, count, typeMask, out), "sampleGradientPoints");
  }
  void sampleGradientGrid(const float origin[3], const float spacing[3], const int dims[3], unsigned int typeMask, float* out) {
    check(sph_sample_gradient_grid(s_, origin, spacing, dims, typeMask, out), "sampleGradientGrid");
  }
  void surfaceNormals(float* normals) { check(sph_surface_normals(s_, normals), "surfaceNormals"); }
  // beyond the reference: shells, open sides and exact sums of area, volume and area moment of the last extractSurface mesh
  // (include/sphmi.h, sph_measure_surface); counts = {shells, closed shells, open sides, bad triangles}, exps = {kA, kV, kM};
  // readShells copies the shell number per vertex, the table (shells x SPH_SHELL_WORDS) and the boxes (shells x 6); any may be null
  void measureSurface(int64_t counts[4], int32_t exps[3]) { check(sph_measure_surface(s_, counts, exps), "measureSurface"); }
  void readShells(int32_t* vertexShell, int64_t* table, float* bbox) { check(sph_read_shells(s_, vertexShell, table, bbox), "readShells"); }
  // beyond the reference: reductions over the particles inside `count` (1..16) regions (x0,y0,z0,x1,y1,z1), SPH_DIAG_WORDS doubles
  // each, and the distribution of one per-particle quantity in bins + 2 counters (include/sphmi.h, sph_diagnostics / sph_histogram)
  void diagnostics(const float* regions6, int count, unsigned int typeMask, double* out) {
    check(sph_diagnostics(s_, regions6, count, typeMask, out), "diagnostics");
  }
  void histogram(int field, float lo, float hi, int bins, const float* region6, unsigned int typeMask, uint32_t* out) {
    check(sph_histogram(s_, field, lo, hi, bins, region6, typeMask, out), "histogram");
  }
  // beyond the reference: the connected components of the particles of `typeMask` in the graph of the last step's neighbour rows
  // (pairs closer than linkRadius; INFINITY = every row entry): counts = {selected particles, components}; components() copies
  // the labels (particleCount ints in sorted order, -1 = not selected) and the table (C x (root, n), C x 6 bbox floats; any
  // pointer may be null); componentDiagnostics gives the diagnostics() record of each of `count` (1..16) component ids
  // (include/sphmi.h, sph_label_components / sph_read_components / sph_component_diagnostics)
  void labelComponents(float linkRadius, unsigned int typeMask, int64_t counts[2]) {
    check(sph_label_components(s_, linkRadius, typeMask, counts), "labelComponents");
  }
  void components(int32_t* labels, int32_t* rootCount, float* bbox) { check(sph_read_components(s_, labels, rootCount, bbox), "components"); }
  void componentDiagnostics(const int32_t* ids, int count, double* out) {
    check(sph_component_diagnostics(s_, ids, count, out), "componentDiagnostics");
  }
  // beyond the reference: the particles themselves. particleMeasure writes the surface measure of every sorted particle
  // (particleCount floats); selectParticles selects on the device by type, region (x0,y0,z0,x1,y1,z1 or null), up to
  // SPH_SELECT_MAX_TERMS range terms and a component of the last labelling (-1 = any) and returns the number selected;
  // readSelection copies the ascending sorted indices, the original ids and the SPH_SELECT_WORDS-float records (any pointer may
  // be null) (include/sphmi.h, sph_particle_measure / sph_select_particles / sph_read_selection)
  void particleMeasure(float* out) { check(sph_particle_measure(s_, out), "particleMeasure"); }
  int64_t selectParticles(const float* region6, unsigned int typeMask, const sph_select_term* terms, int termCount, int component = -1) {
    int64_t count = 0;
    check(sph_select_particles(s_, region6, typeMask, terms, termCount, component, &count), "selectParticles");
    return count;
  }
  void readSelection(int32_t* sortedIndex, uint32_t* origId, float* records) {
    check(sph_read_selection(s_, sortedIndex, origId, records), "readSelection");
  }

  // beyond the reference: the elastic matter. elasticMeasure writes one row per elastic particle in connection-table order (sorted
  // index, original id, SPH_ELASTIC_WORDS floats of strain and spring / contraction acceleration, and (r, r - L0) for each of the
  // 32 slots; any pointer may be null); muscleDiagnostics writes (muscleCount + 1) x SPH_MUSCLE_WORDS doubles, record 0 the
  // connections of no muscle group; membraneMeasure writes numOfMembranes x SPH_MEMBRANE_WORDS floats (or nothing for null) and
  // totals = {count, total area, min area, max area} (include/sphmi.h, sph_elastic_measure / sph_muscle_diagnostics /
  // sph_membrane_measure)
  void elasticMeasure(int32_t* sortedIndex, uint32_t* origId, float* records, float* connections) {
    check(sph_elastic_measure(s_, sortedIndex, origId, records, connections), "elasticMeasure");
  }
  void muscleDiagnostics(double* out) { check(sph_muscle_diagnostics(s_, out), "muscleDiagnostics"); }
  void membraneMeasure(float* out, double totals[4]) { check(sph_membrane_measure(s_, out, totals), "membraneMeasure"); }

  // beyond the reference: who pushes on whom. forceMeasure writes SPH_FORCE_WORDS floats per sorted particle (fromSelection =
  // false: particleCount records) or per particle of the current selection, in its order (fromSelection = true): the viscous,
  // tension and pressure accelerations of the last step by the class of the neighbour that exerted them; forceDiagnostics writes
  // their totals over `count` (1..16) regions, SPH_FORCE_DIAG_WORDS doubles each. Accelerations: times cfg.mass they are forces
  // (include/sphmi.h, sph_force_measure / sph_force_diagnostics)
  void forceMeasure(bool fromSelection, float* out) { check(sph_force_measure(s_, fromSelection ? 1 : 0, out), "forceMeasure"); }
  void forceDiagnostics(const float* regions6, int count, unsigned int typeMask, double* out) {
    check(sph_force_diagnostics(s_, regions6, count, typeMask, out), "forceDiagnostics");
  }

  // beyond the reference: a picture. renderParticles draws the particles of typeMask inside region6 (or null) as shaded spheres
  // through `view` into depth, sorted-index, original-id, rgba and (wantThickness) thickness images kept on the device and fills
  // counts = {particles drawn, covered pixels}; readRender copies the images out, width x height words each (any pointer may be
  // null) (include/sphmi.h, sph_render_particles / sph_read_render)
  void renderParticles(const sph_render_view& view, const float* region6, unsigned int typeMask, bool wantThickness, int64_t counts[2]) {
    check(sph_render_particles(s_, &view, region6, typeMask, wantThickness ? 1 : 0, counts), "renderParticles");
  }
  void readRender(float* depth, int32_t* sortedIndex, uint32_t* origId, uint8_t* rgba, uint32_t* thickness) {
    check(sph_read_render(s_, depth, sortedIndex, origId, rgba, thickness), "readRender");
  }
  // beyond the reference: triangles in the same picture. renderMesh draws the mesh of the last extractSurface (style.source 0) or
  // the membrane triangles (1) through `view`, as a fresh render (style.compose 0) or over the images of the last render by depth
  // (1: the same width .. nearPlane), and fills counts = {triangles drawn, triangles skipped, pixels the mesh holds, covered
  // pixels}; readRender keeps working; readRenderTriangles copies out the winning triangle per pixel, -1 where none
  // (include/sphmi.h, sph_render_mesh / sph_read_render_triangles)
  void renderMesh(const sph_render_view& view, const sph_render_mesh_style& style, int64_t counts[4]) {
    check(sph_render_mesh(s_, &view, &style, counts), "renderMesh");
  }
  void readRenderTriangles(int32_t* triangle) { check(sph_read_render_triangles(s_, triangle), "readRenderTriangles"); }

  // beyond the reference: the particle set changes between two steps (emitters, drains, gates). removeRegion removes the
  // particles of typeMask inside region6 (or null = everywhere) from the current state (read_position_buffer's order), or only
  // counts them (countOnly); removeSelection those of the current selection; removeIds the listed original ids. The survivors keep
  // their order, readEditMap tells where each went (new id or -1; as many ints as there were particles before the removal).
  // addParticles appends count particles (x, y, z, type 1 or 3 / vx, vy, vz, 0), emitLattice a lattice generated on the device,
  // within config().capacity. An edit that changes the set changes particleCount() (size read_*_buffer's arrays from it) and
  // invalidates the analysis calls until the next step (include/sphmi.h, sph_remove_* / sph_add_particles / sph_emit_lattice)
  int64_t removeRegion(const float* region6, unsigned int typeMask, bool countOnly = false) {
    int64_t removed = 0;
    check(sph_remove_region(s_, region6, typeMask, countOnly ? 1 : 0, &removed), "removeRegion");
    return removed;
  }
  int64_t removeSelection() {
    int64_t removed = 0;
    check(sph_remove_selection(s_, &removed), "removeSelection");
    return removed;
  }
  int64_t removeIds(const uint32_t* origIds, int64_t count) {
    int64_t removed = 0;
    check(sph_remove_ids(s_, origIds, count, &removed), "removeIds");
    return removed;
  }
  void addParticles(const float* position4, const float* velocity4, int count) {
    check(sph_add_particles(s_, position4, velocity4, count), "addParticles");
  }
  int64_t emitLattice(const float origin[3], const float spacing[3], const int dims[3], const float velocity[3], float typeValue = 1.0f) {
    int64_t added = 0;
    check(sph_emit_lattice(s_, origin, spacing, dims, velocity, typeValue, &added), "emitLattice");
    return added;
  }
  void readEditMap(int32_t* newIdOfOld) { check(sph_read_edit_map(s_, newIdOfOld), "readEditMap"); }
  int particleCount() {
    const int n = sph_particle_count(s_);
    if (n < 0) check(n, "particleCount");
    return n;
  }

  // beyond the reference: walls that move between two steps (a piston, a paddle, a blade, a sliding gate). Up to SPH_MAX_BODIES
  // bodies, each an ordered list of original ids of boundary particles with the position and normal they had when the body was
  // defined (its reference placement). bodyDefineIds takes a list, bodyDefineRegion every boundary particle inside region6 (or
  // null = everywhere) in ascending id, and returns the member count; bodyRead copies ids and reference rows (any pointer may be
  // null). bodySetPose places the members at pose (row-major 3 x 4, (R | t)) applied to the reference placement, all or nothing,
  // and returns the largest displacement against the current position in units of r0: from about 1 on the wall tunnels through
  // liquid. The analysis state stays valid; removals carry the bodies along (include/sphmi.h, sph_body_*)
  void bodyDefineIds(int slot, const uint32_t* origIds, int64_t count) { check(sph_body_define_ids(s_, slot, origIds, count), "bodyDefineIds"); }
  int64_t bodyDefineRegion(int slot, const float* region6) {
    int64_t count = 0;
    check(sph_body_define_region(s_, slot, region6, &count), "bodyDefineRegion");
    return count;
  }
  void bodyRelease(int slot) { check(sph_body_release(s_, slot), "bodyRelease"); }
  int64_t bodyCount(int slot) {
    int64_t count = 0;
    check(sph_body_count(s_, slot, &count), "bodyCount");
    return count;
  }
  void bodyRead(int slot, uint32_t* origIds, float* refPosition4, float* refNormal4) {
    check(sph_body_read(s_, slot, origIds, refPosition4, refNormal4), "bodyRead");
  }
  float bodySetPose(int slot, const float pose[12], int64_t* offenders = nullptr, int64_t* lowestMember = nullptr) {
    float maxMove = 0.f;
    check(sph_body_set_pose(s_, slot, pose, offenders, lowestMember, &maxMove), "bodySetPose");
    return maxMove;
  }

  // beyond the reference: free bodies. bodySetDynamics gives body `slot` a dynamic state (null: kinematic again), bodyGetDynamics
  // returns whether it has one and, if so, the live state; bodiesAdvance, after a completed step, computes the load of that step on
  // every dynamic body, advances its rigid-body state by one step and places its members, all on the GPU: with out == null nothing
  // waits for the device, otherwise SPH_MAX_BODIES x SPH_BODY_STATE_WORDS doubles are copied out (include/sphmi.h, sph_bodies_advance)
  void bodySetDynamics(int slot, const sph_body_dynamics* dyn) { check(sph_body_set_dynamics(s_, slot, dyn), "bodySetDynamics"); }
  bool bodyGetDynamics(int slot, sph_body_dynamics* out) {
    int32_t isDynamic = 0;
    check(sph_body_get_dynamics(s_, slot, out, &isDynamic), "bodyGetDynamics");
    return isDynamic != 0;
  }
  void bodiesAdvance(double* out = nullptr) { check(sph_bodies_advance(s_, out), "bodiesAdvance"); }

  // beyond the reference: the load on a wall. slot: a body slot, SPH_WALL_ALL (every boundary particle) or SPH_WALL_NO_BODY (the
  // boundary particles of no body). wallMeasure writes SPH_WALL_WORDS floats per sorted particle (fromSelection = true: per
  // particle of the current selection): the set's share of the position shift and velocity change of the contact inside the last
  // step's integrate, the set's K7 / K12 words of forceMeasure, the position and velocity integrate stored; wallDiagnostics writes
  // their totals over `count` (1..16) regions, SPH_WALL_DIAG_WORDS doubles each. Per unit mass, on the liquid: cfg.mass times the
  // summed velocity change over timeStep is the contact's force, and minus that, approximately, the load on the body
  // (include/sphmi.h, sph_wall_measure / sph_wall_diagnostics)
  void wallMeasure(int slot, bool fromSelection, float* out) { check(sph_wall_measure(s_, slot, fromSelection ? 1 : 0, out), "wallMeasure"); }
  void wallDiagnostics(int slot, const float* regions6, int count, unsigned int typeMask, double* out) {
    check(sph_wall_diagnostics(s_, slot, regions6, count, typeMask, out), "wallDiagnostics");
  }

  // beyond the reference: flow gauges. Up to SPH_MAX_GAUGES oriented parallelograms (or planes); after a completed step
  // gaugesAccumulate counts the particles that went through each and sums what they carried, adds the record to the totals on the
  // device and appends it to the history ring (out == null: no host wait; otherwise SPH_MAX_GAUGES x SPH_GAUGE_WORDS doubles).
  // gaugeDefine with null releases a slot; gaugesRead returns the totals (SPH_MAX_GAUGES x SPH_GAUGE_TOTAL_WORDS) and the number of
  // calls so far; gaugeCrossings lists the crossings of one gauge and returns their number, readGaugeCrossings copies the list (any
  // pointer may be null) (include/sphmi.h, sph_gauge_define / sph_gauges_accumulate)
  void gaugeDefine(int slot, const sph_gauge* g) { check(sph_gauge_define(s_, slot, g), "gaugeDefine"); }
  bool gaugeGet(int slot, sph_gauge* out) {
    int32_t defined = 0;
    check(sph_gauge_get(s_, slot, out, &defined), "gaugeGet");
    return defined != 0;
  }
  void gaugesAccumulate(double* out = nullptr) { check(sph_gauges_accumulate(s_, out), "gaugesAccumulate"); }
  int64_t gaugesRead(double* totals) {
    int64_t calls = 0;
    check(sph_gauges_read(s_, totals, &calls), "gaugesRead");
    return calls;
  }
  void gaugesReset(int slot = -1) { check(sph_gauges_reset(s_, slot), "gaugesReset"); }
  void gaugesHistory(int rows) { check(sph_gauges_history(s_, rows), "gaugesHistory"); }
  int64_t gaugesReadHistory(int64_t firstCall, int count, double* out) {
    int64_t calls = 0;
    check(sph_gauges_read_history(s_, firstCall, count, out, &calls), "gaugesReadHistory");
    return calls;
  }
  int64_t gaugeCrossings(int slot) {
    int64_t n = 0;
    check(sph_gauge_crossings(s_, slot, &n), "gaugeCrossings");
    return n;
  }
  void readGaugeCrossings(int32_t* sortedIndex, uint32_t* origId, int32_t* direction, float* tab3) {
    check(sph_read_gauge_crossings(s_, sortedIndex, origId, direction, tab3), "readGaugeCrossings");
  }

  // beyond the reference: probes. Point probes (the sph_sample_points record at fixed points) and level probes (the first crossing
  // of a field's iso value along a fixed line, searched from its far end) kept by the solver; after a completed step probesRecord
  // computes every record, writes it to the history ring on the device if there is one (probesHistory) and, with both pointers
  // null, returns without a host wait. probesSetPoints / probesSetLines with count 0 release a set; probesReadHistory copies the
  // records of calls firstCall .. firstCall + count - 1 (either pointer may be null) and returns the number of calls so far
  // (include/sphmi.h, sph_probes_*)
  void probesSetPoints(const float* points4, int count, uint32_t typeMask) { check(sph_probes_set_points(s_, points4, count, typeMask), "probesSetPoints"); }
  void probesSetLines(const sph_probe_line* lines, int count) { check(sph_probes_set_lines(s_, lines, count), "probesSetLines"); }
  void probesCount(int32_t counts[2]) { check(sph_probes_count(s_, counts), "probesCount"); }
  void probesRecord(float* points = nullptr, float* levels = nullptr) { check(sph_probes_record(s_, points, levels), "probesRecord"); }
  void probesHistory(int rows) { check(sph_probes_history(s_, rows), "probesHistory"); }
  int64_t probesReadHistory(int64_t firstCall, int count, float* points, float* levels) {
    int64_t calls = 0;
    check(sph_probes_read_history(s_, firstCall, count, points, levels, &calls), "probesReadHistory");
    return calls;
  }

  // beyond the reference: time statistics on a lattice. Up to SPH_MAX_STATS lattices kept by the solver; after a completed step
  // statsAccumulate folds the sample record at every node of a slot (-1: of every defined slot) into SPH_STATS_WORDS doubles per
  // node that stay on the device, without a host wait. statsRead copies the accumulators of nodes firstNode .. firstNode + count - 1
  // (node-major, x fastest), statsReadMoments the SPH_STATS_MOMENT_WORDS floats computed from them on the device; both return the
  // slot's calls. statsDefine with a null lattice (statsRelease) frees the slot (include/sphmi.h, sph_stats_*)
  void statsDefine(int slot, const sph_stats_lattice* g) { check(sph_stats_define(s_, slot, g), "statsDefine"); }
  void statsRelease(int slot) { check(sph_stats_define(s_, slot, nullptr), "statsRelease"); }
  bool statsGet(int slot, sph_stats_lattice* out, int64_t* calls = nullptr) {
    int32_t defined = 0;
    check(sph_stats_get(s_, slot, out, &defined, calls), "statsGet");
    return defined != 0;
  }
  void statsAccumulate(int slot = -1) { check(sph_stats_accumulate(s_, slot), "statsAccumulate"); }
  void statsReset(int slot = -1) { check(sph_stats_reset(s_, slot), "statsReset"); }
  int64_t statsRead(int slot, int64_t firstNode, int64_t count, double* out) {
    int64_t calls = 0;
    check(sph_stats_read(s_, slot, firstNode, count, out, &calls), "statsRead");
    return calls;
  }
  int64_t statsReadMoments(int slot, int64_t firstNode, int64_t count, float* out) {
    int64_t calls = 0;
    check(sph_stats_read_moments(s_, slot, firstNode, count, out, &calls), "statsReadMoments");
    return calls;
  }

  // beyond the reference: binned diagnostics. binDiagnostics writes the diagnostics() record of every bin of the lattice (edge i of
  // axis a: origin[a] + (float)i * spacing[a]; dims 1 with spacing 0: the whole axis), nx * ny * nz x SPH_DIAG_WORDS doubles, bin
  // (i, j, k) at (k * ny + j) * nx + i, each word for word what diagnostics() returns for the bin's box; binIndex the bin of every
  // sorted particle, -1 = in none (include/sphmi.h, sph_bin_diagnostics / sph_bin_index)
  void binDiagnostics(const sph_bin_lattice* g, double* out) { check(sph_bin_diagnostics(s_, g, out), "binDiagnostics"); }
  void binIndex(const sph_bin_lattice* g, int32_t* binOfSorted) { check(sph_bin_index(s_, g, binOfSorted), "binIndex"); }

  // beyond the reference: a scalar of the user's own that travels with the particles (a dye, a temperature). Up to
  // SPH_FIELD_SLOTS fields of one float per particle in original-id order (read_position_buffer's); a step never touches them,
  // the edits above carry them along (new particles get `inflow`). fieldSetRegion paints the particles removeRegion would
  // remove, fieldSetSelection those of the current selection; fieldDiffuse runs `substeps` Jacobi substeps of K7's viscous sum
  // with the scalar in place of a velocity component over the last step's neighbour rows and returns the stability number (<= 1:
  // the field keeps its bounds); fieldDiagnostics writes SPH_FIELD_DIAG_WORDS doubles per region (n, sum, sum of squares, min,
  // max, non-zero count) (include/sphmi.h, sph_field_*)
  void fieldCreate(int slot, const float* valuesN = nullptr, float inflow = 0.f) { check(sph_field_create(s_, slot, valuesN, inflow), "fieldCreate"); }
  void fieldRelease(int slot) { check(sph_field_release(s_, slot), "fieldRelease"); }
  void fieldWrite(int slot, const float* valuesN) { check(sph_field_write(s_, slot, valuesN), "fieldWrite"); }
  void fieldRead(int slot, float* outN) { check(sph_field_read(s_, slot, outN), "fieldRead"); }
  int64_t fieldSetRegion(int slot, float value, const float* region6, unsigned int typeMask) {
    int64_t painted = 0;
    check(sph_field_set_region(s_, slot, region6, typeMask, value, &painted), "fieldSetRegion");
    return painted;
  }
  int64_t fieldSetSelection(int slot, float value) {
    int64_t painted = 0;
    check(sph_field_set_selection(s_, slot, value, &painted), "fieldSetSelection");
    return painted;
  }
  float fieldDiffuse(int slot, float coefficient, int substeps, unsigned int typeMask) {
    float stability = 0.f;
    check(sph_field_diffuse(s_, slot, coefficient, substeps, typeMask, &stability), "fieldDiffuse");
    return stability;
  }
  void fieldDiagnostics(int slot, const float* regions6, int count, unsigned int typeMask, double* out) {
    check(sph_field_diagnostics(s_, slot, regions6, count, typeMask, out), "fieldDiagnostics");
  }
  // beyond the reference: curves that follow the sampled velocity field (include/sphmi.h, sph_trace_streamlines / sph_tracers_*).
  // traceStreamlines: one curve per seed of the field frozen at the last completed step; vertices holds count x (maxSteps + 1) x
  // 4 floats (x, y, z, speed; +0 behind a curve's end), lengths and status one int per seed. Tracers are points kept on the device
  // and moved by one step of the same rule per tracersAdvect call (returns the number still moving); steps and edits leave them
  // alone. region6 may be null.
  void traceStreamlines(const float* seeds4, int count, unsigned int typeMask, const sph_trace_params& params, const float* region6,
                        float* vertices, int32_t* lengths, int32_t* status) {
    check(sph_trace_streamlines(s_, seeds4, count, typeMask, &params, region6, vertices, lengths, status), "traceStreamlines");
  }
  void tracersSet(const float* points4, int count) { check(sph_tracers_set(s_, points4, count), "tracersSet"); }
  int64_t tracersAdvect(unsigned int typeMask, const sph_trace_params& params, const float* region6 = nullptr) {
    int64_t counts[2] = {0, 0};
    check(sph_tracers_advect(s_, typeMask, &params, region6, counts), "tracersAdvect");
    return counts[0];
  }
  void tracersRead(float* pos4, int32_t* status, int32_t* steps) { check(sph_tracers_read(s_, pos4, status, steps), "tracersRead"); }

  // beyond the reference: the whole stage sequence of simulationStep() as one call, and per-stage device timing
  unsigned int step(int iterationCount) { return (unsigned)sph_step(s_, iterationCount); }
  sph_solver* handle() { return s_; }
  const sph_config& config() const { return cfg_; }

 private:
  static void check(int rc, const char* what) {
    if (rc != SPH_OK) throw std::runtime_error(std::string(what) + ": " + sph_last_error());
  }
  static void expect(size_t have, long long want, const char* array, const char* rule) {
    if (want < 0 || have != (size_t)want)
      throw std::runtime_error(std::string(array) + " holds " + std::to_string(have) + " words, the configuration asks for " + rule +
                               " = " + std::to_string(want));
  }
  sph_config cfg_;
  sph_solver* s_;
};

/* sphmi.h — C ABI of libsphmi.so, the MI355X (gfx950) PCISPH / Electrofluid step solver.
 *
 * Drop-in boundary: this library replaces the reference's C++ class `owOpenCLSolver`
 * (/root/reference/src/owOpenCLSolver.h:28-62), which is the only seam between the step
 * orchestrator owPhysicsFluidSimulator::simulationStep() (src/owPhysicsFluidSimulator.cpp:79-149)
 * and the device kernels (src/sphFluid.cl). Each entry point names the reference member it replaces.
 * Plain pointers and sizes only; no C++/torch types cross this boundary. All functions return
 * 0 on success or a negative sph_status; nothing throws. sph_last_error() gives the text.
 *
 * The reference keeps its inputs in mutable globals (PARTICLE_COUNT, gridCells*, numOf*, delta, the
 * box macros — owOpenCLSolver.h:14-17, owOpenCLSolver.cpp:7-23, owPhysicsConstant.h); here they are
 * the explicit `sph_config`.
 *
 * After each sph_run_* the solver holds what the reference's buffers would hold after the same
 * _run* call; sph_read_buffer() exports any of them in the reference's own
 * layout and index space, so stage-by-stage parity can be checked. Internally the data is laid out
 * for CDNA4, not as the reference's AoS buffers.
 */
#ifndef SPHMI_H
#define SPHMI_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SPHMI_ABI_VERSION 2
#define SPH_MAX_PARTICLES ((1 << 27) - 1) /* capacity ceiling of one solver: the tiled neighbour map is addressed with 32-bit
                                             element indices (32 slots x 2^27 particles = 2^32); sph_create rejects more */
#define SPH_MAX_NEIGHBOR_COUNT 32 /* owOpenCLConstant.h:4 */
#define SPH_MAX_MEMBRANES_INCLUDING_SAME_PARTICLE 7 /* owOpenCLConstant.h:6 */
#define SPH_LIQUID_PARTICLE 1   /* owOpenCLConstant.h:8-10 */
#define SPH_ELASTIC_PARTICLE 2
#define SPH_BOUNDARY_PARTICLE 3

typedef enum sph_status {
  SPH_OK = 0,
  SPH_ERR_INVALID = -1,  /* bad argument / configuration the kernels cannot represent */
  SPH_ERR_HIP = -2,      /* a HIP runtime call failed (no GPU, out of memory, launch failure) */
  SPH_ERR_ORDER = -3,    /* stage called before the stage it depends on */
  SPH_ERR_UNKNOWN_BUFFER = -4,
  SPH_ERR_SIZE = -5
} sph_status;

/* Everything the reference passes as kernel arguments or globals. Field names follow the reference. */
typedef struct sph_config {
  int32_t abi_version;      /* SPHMI_ABI_VERSION */
  int32_t particleCount;    /* PARTICLE_COUNT */
  int32_t capacity;         /* buffers are sized for this many particles (slab decomposition: the count varies per step);
                               0 = particleCount. At most SPH_MAX_PARTICLES (2^27 - 1 = 134,217,727) */
  int32_t gridCellsX, gridCellsY, gridCellsZ, gridCellCount; /* owOpenCLSolver.cpp:14-17 */
  uint32_t cellIdMask;      /* 0xffff = reference behaviour (sphFluid.cl:229,377); 0xffffffff = wide */
  float h, hashGridCellSize, hashGridCellSizeInv, simulationScale, simulationScaleInv; /* owPhysicsConstant.h:19-24 */
  float xmin, xmax, ymin, ymax, zmin, zmax;                                           /* owOpenCLSolver.cpp:7-12 */
  float r0, mass, rho0, timeStep, viscosity, delta;                                   /* owPhysicsConstant.h:12-27,63,75 */
  float gravity_x, gravity_y, gravity_z;                                              /* owPhysicsConstant.h:72-74 */
  float surfTensCoeff;      /* sphFluid.cl:662, evaluated once on the host in the reference's types */
  double Wpoly6Coefficient, gradWspikyCoefficient, del2WviscosityCoefficient;         /* owPhysicsConstant.h:69-71 */
  int32_t numOfElasticP;    /* rows of elasticConnectionsData */
  int32_t elasticOffset;    /* numOfBoundaryP*(!generateInitialConfiguration), owOpenCLSolver.cpp:435 */
  int32_t muscleCount;      /* MUSCLE_COUNT (owWorldSimulation.cpp:31) */
  int32_t numOfMembranes;
  int32_t maxIteration;     /* owPhysicsConstant.h:76 */
  int32_t device;           /* HIP device ordinal */
  void* stream;             /* hipStream_t to launch on; NULL = the solver creates its own */
} sph_config;

typedef struct sph_solver sph_solver;

/* owOpenCLSolver::owOpenCLSolver(position_cpp, velocity_cpp, elasticConnectionsData_cpp, membraneData_cpp,
 * particleMembranesList_cpp) — owOpenCLSolver.cpp:27-92. Host arrays are copied; the caller keeps ownership
 * of all five (unlike the reference, particleMembranesList is NOT freed here). position/velocity: 4*N floats
 * (x,y,z,type) / (vx,vy,vz,w); elastic: 4*32*numOfElasticP floats; membranes: 3*numOfMembranes ints;
 * particleMembranesList: 7*numOfElasticP ints. */
int sph_create(const sph_config* cfg, const float* position, const float* velocity, const float* elasticConnections,
               const int32_t* membraneData, const int32_t* particleMembranesList, sph_solver** out);
/* owOpenCLSolver::~owOpenCLSolver — owOpenCLSolver.cpp:744-748 */
int sph_destroy(sph_solver* s);

/* One per owOpenCLSolver::_run* (owOpenCLSolver.h:37-56, owOpenCLSolver.cpp:213-687), same order contract as
 * simulationStep(). Asynchronous on the solver's stream. */
int sph_run_clear_buffers(sph_solver* s);                          /* _runClearBuffers            :213 */
int sph_run_hash_particles(sph_solver* s);                         /* _runHashParticles           :229 */
int sph_run_sort(sph_solver* s);                                   /* _runSort (host qsort there) :255 */
int sph_run_sort_post_pass(sph_solver* s);                         /* _runSortPostPass            :262 */
int sph_run_indexx(sph_solver* s);                                 /* _runIndexx                  :284 */
int sph_run_index_post_pass(sph_solver* s);                        /* _runIndexPostPass (host)    :305 */
int sph_run_find_neighbors(sph_solver* s);                         /* _runFindNeighbors           :320 */
int sph_run_pcisph_compute_density(sph_solver* s);                 /* _run_pcisph_computeDensity  :357 */
int sph_run_pcisph_compute_forces_and_init_pressure(sph_solver* s);/* ..._computeForcesAndInitPressure :386 */
int sph_run_pcisph_compute_elastic_forces(sph_solver* s);          /* ..._computeElasticForces    :420 */
int sph_run_pcisph_predict_positions(sph_solver* s);               /* ..._predictPositions        :454 */
int sph_run_pcisph_predict_density(sph_solver* s);                 /* ..._predictDensity          :490 */
int sph_run_pcisph_correct_pressure(sph_solver* s);                /* ..._correctPressure         :519 */
int sph_run_pcisph_compute_pressure_force_acceleration(sph_solver* s); /* ..._computePressureForceAcceleration :549 */
int sph_run_pcisph_integrate(sph_solver* s, int iterationCount);   /* _run_pcisph_integrate       :649 */
int sph_run_clear_membrane_buffers(sph_solver* s);                 /* _run_clearMembraneBuffers   :583 */
int sph_run_compute_interaction_with_membranes(sph_solver* s);     /* _run_computeInteractionWithMembranes :602 */
int sph_run_compute_interaction_with_membranes_finalize(sph_solver* s); /* ..._finalize           :628 */

/* The whole stage sequence of owPhysicsFluidSimulator::simulationStep() (owPhysicsFluidSimulator.cpp:88-113) as one
 * call on the solver's stream, with the fusions of DESIGN.md §4. Same results as calling the sph_run_* above in order. */
int sph_step(sph_solver* s, int iterationCount);

/* owOpenCLSolver::updateMuscleActivityData — owOpenCLSolver.cpp:738-742 (n must equal muscleCount) */
int sph_update_muscles(sph_solver* s, const float* signal, int n);

/* owOpenCLSolver::read_position_buffer / read_density_buffer / read_particleIndex_buffer — owOpenCLSolver.h:60-62.
 * Blocking. position: 4N floats, orig order. density: N floats, SORTED order (as the reference).
 * particleIndex: 2N uints (cell, origId), sorted. velocity has no reference getter; provided for checks. */
int sph_read_position(sph_solver* s, float* out4N);
int sph_read_velocity(sph_solver* s, float* out4N);
int sph_read_density(sph_solver* s, float* outN);
int sph_read_particle_index(sph_solver* s, uint32_t* out2N);

/* read_position_buffer without the wait. The reference ends every simulationStep() with a blocking 16N-byte read
 * (owPhysicsFluidSimulator.cpp:115, owOpenCLSolver.h:60); here the copy can run on a stream of its own under the NEXT step's
 * search and PCISPH stages: sph_read_position_async returns at once, the positions of the steps enqueued so far land in
 * out4N in the background, and the next kernel that writes positions (integrate, the last kernel of a step) waits for the
 * copy on the device. sph_read_position_wait blocks until the last requested copy has landed (and reports a blown-up state
 * like sph_read_position); a second sph_read_position_async waits for the previous one first. out4N must stay valid until
 * then. For the copy to overlap, out4N must be DMA-able: memory that is already pinned (hipHostMalloc / hipHostRegister) is
 * used as it is, any other buffer is page-locked in place with hipHostRegister on first use (kept until sph_destroy or
 * sph_host_unregister — call that before freeing the buffer); if that fails the copy goes through a pinned staging area and
 * sph_read_position_wait does the final memcpy. */
int sph_read_position_async(sph_solver* s, float* out4N);
int sph_read_position_wait(sph_solver* s);
int sph_host_unregister(sph_solver* s, void* buffer);

/* Test/inspection export in the reference's layout. Names: position[2N f4] velocity[2N f4]
 * sortedPosition[2N f4] sortedVelocity[N f4] acceleration[2N f4] neighborMap[32N f2] neighborIds[32N i32]
 * particleIndex[N u2] particleIndexBack[N u32] gridCellIndex[G+1 u32] gridCellIndexFixedUp[G+1 u32]
 * pressure[N f32] rho[2N f32]. `bytes` must equal the buffer's size (query with out == NULL: returns the size
 * through *needed). Blocking. */
int sph_read_buffer(sph_solver* s, const char* name, void* out, size_t bytes, size_t* needed);
/* The neighbour lists of the SORTED particles [first, first + count) only (a 64 M-particle map is 16 GB): ids[count][32]
 * (sorted index of the neighbour, -1 = empty slot: neighborMap[].x of the reference, sphFluid.cl:170) and dist[count][32]
 * (neighborMap[].y: distance * simulationScale, -1 = empty). Either pointer may be NULL. Blocking. */
int sph_read_neighbor_rows(sph_solver* s, int32_t first, int32_t count, int32_t* ids, float* dist);

/* ---- Field sampling (SPH interpolation; no reference counterpart) ---------------------------------------------------------
 * Reads the SORTED STATE OF THE LAST COMPLETED STEP: the arrays that step's neighbour search, density and pressure loop ran on
 * (sortedPos / sortedVel as gathered by the sort, before integration; rho from computeDensity; pressure after the last
 * predict-correct iteration; the cell table). This is the state sph_read_density describes, ONE INTEGRATION STEP BEHIND
 * sph_read_position. Read-only on every solver array; not a stage (no stage timing).
 *
 * For a query point p and a type mask m, particle j (sorted index) is selected when all of:
 *   (1 << (int)position.w) & m != 0        (bit 1 = liquid, 2 = elastic, 3 = boundary; the worm's elastic types are 2.x)
 *   dx*dx + dy*dy + dz*dz < h*h            (d = p - x_j in scene units, float, products and sums in that order, h*h one float)
 *   j's cell key is in the step's cell table (key < gridCellCount)
 * For the selected j in ASCENDING SORTED INDEX, in float throughout: a = hs2 - r2*ss2 (ss2 = simScale*simScale as a float,
 * hs2 = (h*simScale)^2 as the step computes it), w = a*a*a, v_j = w * (1.0f/rho_j); W += w, S += v_j, U += v_j*vel_j.xyz,
 * P += v_j*p_j as sequential float sums. Record (SPH_SAMPLE_WORDS floats):
 *   { rho = (float)massWpoly6 * W, shepard = (float)massWpoly6 * S, vx, vy, vz = U/S, p = P/S, n = count, 0 }
 * with zeros in place of the quotients when S == 0; a non-finite query point gives an all-zero record. The sums start at +0, and
 * f32 denormals are kept: in the last ulps of r2 below h*h the weight w underflows to +0 or -0 (a may be negative there), such
 * a particle counts in n and leaves +0 in every sum; farther in, W and S are subnormal numbers, and S may be 0 while W is not.
 * Allowed once the density and pressure-force stages of a step have run (sph_step or the sph_run_* path), SPH_ERR_ORDER before;
 * SPH_ERR_INVALID for a slab solver, a typeMask of 0 or with bits outside 1..3, dims <= 0, count < 0, or null pointers
 * (count == 0 is a no-op). Blocking, on the solver's stream; device scratch is grown on demand (bounded: large grids go in
 * z-chunks) and freed by sph_destroy. */
#define SPH_SAMPLE_WORDS 8
int sph_sample_points(sph_solver* s, const float* points4 /* host, count x (x,y,z,unused) */, int32_t count,
                      uint32_t typeMask, float* out /* host, count x 8 */);
/* Grid point (i, j, k) = origin + (float)i * spacing per axis (one float multiply, one float add). */
int sph_sample_grid(sph_solver* s, const float origin[3], const float spacing[3], const int32_t dims[3],
                    uint32_t typeMask, float* out /* host, dims[2] x dims[1] x dims[0] x 8, x fastest */);

/* ---- Isosurface extraction (marching cubes over a sampled field; no reference counterpart) --------------------------------
 * Field: f(i,j,k) is word `field` (0 density, 1 shepard, 2 vx, 3 vy, 4 vz, 5 pressure) of the record that
 * sph_sample_grid(s, origin, spacing, dims, typeMask, ...) would return at lattice point (i,j,k), bit for bit: the same state
 * (the last completed step, one integration step behind sph_read_position). Inside: f >= iso (float compare; NaN is outside).
 * Cells: cell (i,j,k), i < nx-1, j < ny-1, k < nz-1, has corner c (0..7) at lattice point (i + (c&1), j + ((c>>1)&1), k + (c>>2));
 * its case is sum of inside(c) << c.
 * Edges: cube edges 0..3 run along x between corners (0,1) (2,3) (4,5) (6,7); 4..7 along y between (0,2) (1,3) (4,6) (5,7);
 * 8..11 along z between (0,4) (1,5) (2,6) (3,7). Cube edge e is the lattice edge that starts at its first corner, axis e/4.
 * Vertices: one per lattice edge whose two ends differ in inside-ness, numbered by the edge's lower lattice point in x-fastest
 * order (k, then j, then i) and within a point in the order +x, +y, +z. Its position is the lower point's coordinates with the
 * edge's axis changed to x0 + t*(x1 - x0), t = (iso - f0)/(f1 - f0), where f0, f1 are the field at the lower and upper point and
 * x0, x1 their coordinates on that axis, each origin + (float)i*spacing; all float, in that order, no contraction, IEEE division.
 * t may be 0: coincident vertices and zero-area triangles are allowed.
 * Triangles: cells in x-fastest order; within a cell, the triangles of the case table, three vertex ids each, oriented so that
 * (v1-v0)x(v2-v0) points from inside toward outside (toward lower f). The table (csrc/sph_mc_table.h, tools/gen_mc_table.py):
 *   1. on each cube face, a face with 2 crossed edges gets one segment between them; a face with 4 has two inside corners on
 *      a diagonal, and each is cut off on its own by a segment joining the two crossed edges next to it;
 *   2. each segment is directed so that, seen from outside the cube, the face's inside corner(s) it cuts off lie to its right;
 *   3. the directed segments form disjoint cycles; each starts at its smallest edge number, cycles in ascending order of it;
 *   4. a cycle c0..c(L-1) becomes the fan (c0, cq, c(q+1)), q = 1..L-2, of its first rotation whose chords (c0, cq),
 *      q = 2..L-2, never join two edges that lie on a common cube face.
 * The mesh is closed wherever the lattice's border points are outside.
 * Lifetime: the mesh stays in device memory owned by the solver until the next sph_extract_surface or sph_destroy; steps do
 * not change it. counts = {vertices, triangles}. sph_read_surface copies it to the host, blocking; either pointer may be NULL;
 * SPH_ERR_ORDER before any successful extraction.
 * Errors: SPH_ERR_ORDER before a step's density and pressure-force stages have run; SPH_ERR_INVALID for a slab solver, a bad
 * typeMask (as sampling), field outside 0..5, a non-finite iso, any dims < 2, a lattice of more than 2^31-1 points, or null
 * pointers; SPH_ERR_SIZE if the vertex count exceeds 2^31-1 (vertex ids are int32). A failed call leaves no mesh behind.
 * Read-only on every solver array; on the solver's stream, blocking only to return the counts. Device memory beyond the
 * sampling scratch: about 10 bytes per lattice point plus 12 bytes per vertex and per triangle, grown on demand, freed by
 * sph_destroy. */
#define SPH_SURFACE_FIELDS 6 /* record words 0..5 of sph_sample_*: density, shepard, vx, vy, vz, pressure */
int sph_extract_surface(sph_solver* s, const float origin[3], const float spacing[3], const int32_t dims[3], uint32_t typeMask,
                        int32_t field, float iso, int64_t counts[2] /* out: vertices, triangles */);
int sph_read_surface(sph_solver* s, float* vertices /* host, counts[0] x 3 */, int32_t* triangles /* host, counts[1] x 3 */);

/* ---- Gradient sampling and surface normals (SPH gradients of the sampled fields; no reference counterpart) -----------------
 * State, selected set, order (ascending sorted index), lattice point formula, argument rules and errors are exactly those of
 * sph_sample_points / sph_sample_grid (SPH_ERR_ORDER before a step's density and pressure-force stages; SPH_ERR_INVALID for a
 * slab solver, a bad typeMask, dims <= 0, count < 0 or null pointers; count == 0 is a no-op). Read-only, blocking.
 * For each selected particle j in ascending sorted index, with dx, dy, dz, r2, t = hs2 - r2*ss2, w = t*t*t and
 * invRho = 1.0f/rho_j those of the sampling contract (d = p - x_j in scene units), all in float, in this order, no contraction:
 *   g = t*t (the value inside w);  q = g*invRho
 *   Bx += g*dx, By += g*dy, Bz += g*dz
 *   Cx += q*dx, Cy += q*dy, Cz += q*dz
 *   for A in (vx_j, vy_j, vz_j, p_j):  a = q*A;  E_A.x += a*dx, E_A.y += a*dy, E_A.z += a*dz
 * 18 sequential float sums starting at 0, beside sampling's W, S, U, P, n. K = (float)(-6.0 * massWpoly6 * (double)simScale),
 * computed in double and rounded once (massWpoly6 as in the sampling contract): gradients are taken with respect to
 * simulation-scaled (physical) coordinates, so vorticity is in 1/s. Record (SPH_GRADIENT_WORDS floats):
 *   0..7    the sph_sample_* record at the same point, bit for bit (U_x, U_y, U_z, P below are its words 2..5)
 *   8..10   grad rho      = K*Bx, K*By, K*Bz
 *   11..13  grad shepard  = K*Cx, K*Cy, K*Cz
 *   14..22  grad u, row-major G[i][c] = K*(E_ui.c - U_i*C.c) for i = x, y, z and c = x, y, z (u_i = vx, vy, vz)
 *   23..25  grad p        = K*(E_p.c - P*C.c)
 *   26..28  vorticity     = (G[2][1] - G[1][2], G[0][2] - G[2][0], G[1][0] - G[0][1])
 *   29      divergence    = (G[0][0] + G[1][1]) + G[2][2]
 *   30      Q-criterion   = -0.5f * s, s = 0, then s += G[i][j]*G[j][i] for (i, j) in row-major order (9 terms)
 *   31      0
 * When S == 0, words 14..30 are 0 (as sampling's quotients); a non-finite query point gives an all-zero record (+0 bits), while
 * a finite point that selects nothing has -0 in words 8..13 (K*0 with K < 0). */
#define SPH_GRADIENT_WORDS 32
int sph_sample_gradient_points(sph_solver* s, const float* points4 /* host, count x (x,y,z,unused) */, int32_t count,
                               uint32_t typeMask, float* out /* host, count x 32 */);
int sph_sample_gradient_grid(sph_solver* s, const float origin[3], const float spacing[3], const int32_t dims[3],
                             uint32_t typeMask, float* out /* host, dims[2] x dims[1] x dims[0] x 32, x fastest */);
/* One normal per vertex of the mesh of the last successful sph_extract_surface, computed on the device from the mesh's
 * vertices (no host round trip). The gradient used for a vertex is the record sph_sample_gradient_points would return at the
 * vertex's float coordinates with the extraction's typeMask; its words are chosen by the extraction's field: 0 -> 8..10,
 * 1 -> 11..13, 2, 3, 4 -> 14..16, 17..19, 20..22, 5 -> 23..25. len = sqrtf((gx*gx + gy*gy) + gz*gz) and
 * n = (-(gx/len), -(gy/len), -(gz/len)) (toward lower f: the side the triangles' winding faces), or (0, 0, 0) where len is 0
 * or not finite. Blocking. SPH_ERR_ORDER before any successful extraction, and once any stage, step or slab call has run since
 * that extraction (the sampled state has changed; sph_read_surface keeps working); SPH_ERR_INVALID for a null pointer with
 * counts[0] > 0. */
int sph_surface_normals(sph_solver* s, float* normals /* host, counts[0] x 3 */);

/* ---- Surface measures (shells, area and enclosed volume of the extracted mesh; no reference counterpart) -------
 * Input: the mesh of the last successful sph_extract_surface (V vertices as packed float3, T triangles as int32 x 3) and the
 * lattice (origin, spacing, dims) it was cut on. The result is a function of these alone.
 * Shells: a shell is a connected component of the graph whose nodes are the vertex ids and whose edges are the three sides of
 * every triangle. A shell's ROOT is its lowest vertex id; shells are numbered 0 .. S-1 in ascending order of their roots;
 * vertexShell[v] is the shell number of vertex v; a triangle belongs to the shell of its first vertex. Coincident vertices (t == 0)
 * have different ids and are not merged.
 * Open sides: a directed side (a, b) of a triangle is open when no triangle has the side (b, a); it is counted in the shell of
 * a. A shell is CLOSED when it has no open side. On these meshes open sides occur only where the lattice border cuts the surface.
 * Euler characteristic of a shell: chi = V_s - (3*T_s + open_s)/2 + T_s.
 * Per-triangle terms, ALL IN DOUBLE, in the written order, no contraction, IEEE sqrt; v0, v1, v2 the triangle's vertices:
 *   p_i = (double)v_i - (double)origin, per component;   e1 = p1 - p0, e2 = p2 - p0
 *   n = e1 x e2: nx = e1y*e2z - e1z*e2y, ny = e1z*e2x - e1x*e2z, nz = e1x*e2y - e1y*e2x
 *   a2 = sqrt((nx*nx + ny*ny) + nz*nz)             twice the area
 *   d6 = (p0x*nx + p0y*ny) + p0z*nz                six times the signed volume of the tetrahedron to the lattice origin: positive
 *                                                  for a drop, negative for a cavity (the normals point toward lower f)
 *   m_c = a2 * ((p0_c + p1_c) + p2_c), c = x, y, z six times the area moment
 * Sums are EXACT INTEGERS, so they do not depend on any order. Each term x is quantised once, q = llrint(ldexp(x, k)) (round to
 * nearest, ties to even), and added as int64. The exponents are a function of the lattice and of T, computed on the host in
 * double:
 *   bT = ceil(log2(T + 1))
 *   eL = 1 + E,  frexp(max_a (dims_a - 1) * |spacing_a|) = (., E);     eS = 1 + E',  frexp(max_a |spacing_a|) = (., E')
 *   (E = 0 for an argument that is 0 or not finite)
 *   kA = 60 - bT - 2*eS (for a2),   kV = 59 - bT - eL - 2*eS (for d6),   kM = 58 - bT - eL - 2*eS (for m_c)
 * No partial sum can overflow. With sigma = 2^eS and Lambda = 2^eL: a triangle's sides lie inside one cell, so
 * |e| <= sqrt(3) * max spacing < sqrt(3)*sigma/2, and |p| < Lambda; hence a2 < 4 sigma^2, |d6| < 8 Lambda sigma^2 and
 * |m_c| < 16 Lambda sigma^2, every scaled term is below 2^(62 - bT), and there are at most 2^bT triangles, so every sum stays
 * below 2^62. The bound is also enforced: a triangle with ANY scaled term ldexp(x, k) that is not below 2^(62 - bT) in magnitude
 * (a non-finite a2 or d6 among them) adds nothing to the five sums and counts as a BAD triangle.
 * A value is ldexp((double)sum, -k): area = value/2, volume = value/6, the centroid of the area = m / (3 * a2 sum), measured
 * from the lattice origin.
 * Table, one row of SPH_SHELL_WORDS int64 per shell: root, vertices, triangles, open sides, bad triangles, sum q(a2), sum q(d6),
 * sum q(mx), q(my), q(mz). Beside it a float bounding box of six words per shell, min x, y, z, max x, y, z of the shell's
 * vertices (float compares, canonicalised by + 0.0f as the components' boxes).
 * counts = {shells, closed shells, open sides, bad triangles}; exps = {kA, kV, kM}.
 * Rules: both calls are blocking, on the solver's stream, not stages (no stage timing), and do not count as a change of state.
 * Both are read-only on every solver array and on the mesh: normals, renders, labellings and selections stay valid. The measure
 * depends on the mesh only, so unlike sph_surface_normals it remains legal after further steps. It lives in device memory owned
 * by the solver until the next sph_extract_surface (successful or not) or sph_destroy.
 * Errors: SPH_ERR_ORDER before any successful extraction, and for sph_read_shells before a successful measure; SPH_ERR_INVALID
 * for a slab solver and for null counts / exps; SPH_ERR_SIZE for more than 2^31-4097 vertices or triangles. An empty mesh is
 * legal: all counts are 0 and exps is computed with T = 0. A pointer walk that exceeds its bound of V steps, or a triangle that
 * names no vertex (never, unless memory is corrupted), is reported as SPH_ERR_HIP rather than followed. A failed measure leaves
 * none behind.
 * Device memory: 16 bytes per vertex (the union-find parents, the shell numbers and the int64 side sums that find the open
 * sides), 104 bytes per shell, 12 bytes per 256 vertices for the scan; grown on demand and freed by sph_destroy. */
#define SPH_SHELL_WORDS 10
int sph_measure_surface(sph_solver* s, int64_t counts[4] /* out: shells, closed shells, open sides, bad triangles */,
                        int32_t exps[3] /* out: kA, kV, kM */);
/* Any pointer may be NULL. */
int sph_read_shells(sph_solver* s, int32_t* vertexShell /* host, V */, int64_t* table /* host, S x SPH_SHELL_WORDS */,
                    float* bbox /* host, S x 6 */);

/* ---- Flow diagnostics (reductions and histograms over the particles; no reference counterpart) ------------------------------
 * State: the sorted state of the last completed step, exactly the one sph_sample_* describes (one integration step behind
 * sph_read_position). Sorted particle j is SELECTED for the region (x0,y0,z0,x1,y1,z1) when its type t = (int)position.w is
 * 1..3 with (1 << t) & typeMask, its cell key is in the step's cell table (key < gridCellCount, as sampling), and
 * x0 <= x && x < x1, y0 <= y && y < y1, z0 <= z && z < z1 (float compares; a bound may be +-infinity, so (-inf, +inf) on every
 * axis is "everything"; a region with x0 >= x1 is empty).
 * Per-particle terms, IN FLOAT, in the written order, no contraction, then widened to double (exact):
 *   v2 = vx*vx + vy*vy + vz*vz;  Lx = y*vz - z*vy, Ly = z*vx - x*vz, Lz = x*vy - y*vx;  e = rho - rho0 (cfg.rho0), e2 = e*e.
 * An unselected particle contributes +0.0 to every sum. Record, SPH_DIAG_WORDS doubles per region:
 *   0        n, the number of selected particles
 *   1..3     sum x, y, z            4..6   sum vx, vy, vz          7..9   sum Lx, Ly, Lz (about the origin, per unit mass)
 *   10       sum v2                 11     sum rho                 12     sum e2
 *   13       sum p (pressure after the last predict-correct iteration)
 *   16, 17   min rho, max rho       18, 19 min p, max p
 *   20..22   max v2; the lowest sorted index that attains it; that particle's original id (its particleIndex value)
 *   23..25   min x, y, z            26..28 max x, y, z             14, 15, 29..31   0 (reserved)
 * Minima and maxima are float compares; the result is canonicalised by + 0.0f (-0 is reported as +0) and widened. With n = 0
 * words 16..20 and 23..28 are 0 and words 21, 22 are -1.
 * THE SUMS ARE DOUBLES ADDED IN A FIXED SHAPE, so that a result depends on nothing but the state and the region: not on the
 * launch geometry, the device, or the other regions of the call. With the terms t[0..N) in ascending sorted index:
 *   reduce(a): pad a with +0.0 to a whole number (at least one) of chunks of 1024
 *              in each chunk, for stride = 512, 256, ..., 1:  a[i] = a[i] + a[i + stride]  for every i < stride
 *              c = the chunks' a[0], in chunk order;  return c[0] if there is one chunk, else reduce(c)
 * (at most three levels for SPH_MAX_PARTICLES; trailing zero terms never change a result). No atomics on floating-point values.
 * A float widened to double has 29 spare mantissa bits, so unless the terms span more than ~2^29 in magnitude these sums equal
 * the exactly rounded sum of the terms.
 * Boundary particles (type 3) keep the wall normal in `velocity`: sums over them are legal but are not momenta.
 * Errors (both functions): SPH_ERR_ORDER before a step's density and pressure-force stages have run; SPH_ERR_INVALID for a slab
 * solver, a typeMask of 0 or with bits outside 1..3, null pointers (region6 of sph_histogram may be NULL = everything), count
 * outside 1..SPH_DIAG_MAX_REGIONS, a NaN region bound, bins outside 1..SPH_HIST_MAX_BINS, field outside 0..6, non-finite lo or
 * hi, lo >= hi; a blown-up state is reported as by every blocking call. Blocking, on the solver's stream, read-only on every
 * solver array (a mesh stays valid for sph_surface_normals), not a stage (no stage timing). Device scratch (256 bytes per region
 * and 1024 particles, or the bins) is grown on demand and freed by sph_destroy. */
#define SPH_DIAG_WORDS 32
#define SPH_DIAG_MAX_REGIONS 16
int sph_diagnostics(sph_solver* s, const float* regions6 /* host, count x (x0,y0,z0,x1,y1,z1) */, int32_t count,
                    uint32_t typeMask, double* out /* host, count x 32 */);
/* Distribution of one per-particle quantity q over the selected particles (same state and selection). field: 0 density,
 * 1 speed sqrtf(v2) (correctly rounded), 2 pressure, 3 the number of valid entries of the particle's neighbour row as a float
 * (the ids >= 0 of sph_read_neighbor_rows), 4, 5, 6 x, y, z. All in float: q < lo counts in out[0]; q >= hi in out[bins + 1];
 * otherwise in bin min((int)((q - lo) * scale), bins - 1), scale = (float)bins / (hi - lo) computed once on the host in float.
 * field 3, lo 0, hi 33, bins 33 is the exact neighbour-count distribution: bin 32 counts the particles at the cap. */
#define SPH_HIST_MAX_BINS 4096
int sph_histogram(sph_solver* s, int32_t field, float lo, float hi, int32_t bins, const float* region6 /* host or NULL */,
                  uint32_t typeMask, uint32_t* out /* host, bins + 2: below, bin 0 .. bins-1, at-or-above */);

/* ---- Connected components (the pieces the matter is in: droplets, fragments, bodies; no reference counterpart) ---------------
 * State: the sorted state of the last completed step, as sampling and diagnostics (one integration step behind
 * sph_read_position), and that step's neighbour rows: row(i) = the ids >= 0 that sph_read_neighbor_rows returns for sorted
 * particle i.
 * Nodes: sorted particle j is SELECTED exactly as for sph_diagnostics with the region "everything": type t = (int)position.w in
 * 1..3 with (1 << t) & typeMask, and its cell key < gridCellCount.
 * Edges: {i, j}, i != j, both selected, j in row(i) OR i in row(j) (a row holds at most 32 entries, chosen through a per-particle
 * threshold radius, so the rows are not symmetric; the graph is their symmetric closure), and r2 < link2, where d = x_i - x_j per
 * coordinate in float, r2 = dx*dx + dy*dy + dz*dz (float, that order, no contraction, scene units: the sampling contract's
 * expression) and link2 = linkRadius * linkRadius as one float. Float negation is exact, so r2 is the same from either end.
 * linkRadius = +infinity keeps every row entry ("the pairs that exchanged forces in this step") and reads no neighbour position.
 * Two particles within h that are absent from each other's capped rows are linked only through third particles.
 * Components: the connected components of that graph; an isolated selected particle is a component of one. A component's ROOT
 * is its lowest sorted index. Components are numbered 0 .. C-1 in ascending order of their roots. labels[j] is j's component
 * number, or -1 if j is not selected. The result is integers and float minima / maxima only and does not depend on the order of
 * execution: it is a function of the state and the arguments.
 * Table, one row per component: root, n (members), and the bounding box min x, y, z, max x, y, z of the members' sorted
 * positions (float compares, canonicalised by + 0.0f as the diagnostics' extremes).
 * sph_component_diagnostics: record r is the sph_diagnostics record, word for word (same per-particle float terms, same widening,
 * the same fixed tree over all N terms in ascending sorted index with non-members contributing +0.0, same rules for the extremes,
 * the same "lowest sorted index that attains max v2" and its original id), where "selected" means labels[j] == components[r].
 * Ids may repeat; a record does not depend on the other ids of the call. Hence word 0 equals the table's n, words 23..28 equal
 * the table's bounding box, and when a labelling has a single component its record equals sph_diagnostics(everything, typeMask)
 * bit for bit.
 * Lifetime: the labelling lives in device memory owned by the solver until the next sph_label_components or sph_destroy;
 * sph_read_components keeps working after further steps. sph_component_diagnostics reads the live state, so it returns
 * SPH_ERR_ORDER once any stage, step or slab call has run since the labelling. The three calls are read-only on every solver
 * array (a mesh stays valid for sph_surface_normals; a labelling stays valid across sph_diagnostics, sampling and extraction
 * calls), blocking, on the solver's stream, and not stages (no stage timing).
 * Errors: SPH_ERR_ORDER before a step's neighbour, density and pressure-force stages have run, and for the two readers before
 * any successful labelling; SPH_ERR_INVALID for a slab solver, a typeMask of 0 or with bits outside 1..3, a linkRadius that is NaN
 * or <= 0, null counts / components / out, count outside 1..SPH_DIAG_MAX_REGIONS, a component id outside 0..C-1. A failed
 * sph_label_components leaves no labelling behind. Zero selected particles is legal: counts = {0, 0}, all labels -1. A pointer
 * walk that exceeds its bound of N steps (never, unless memory is corrupted) is reported as SPH_ERR_HIP rather than followed.
 * Device memory: 8 bytes per particle (the union-find parents and the labels), 32 bytes per component for the table, 12 bytes
 * per 256 particles for the scan; grown on demand and freed by sph_destroy. */
int sph_label_components(sph_solver* s, float linkRadius, uint32_t typeMask, int64_t counts[2] /* selected particles, components */);
/* Any pointer may be NULL. */
int sph_read_components(sph_solver* s, int32_t* labels /* host, N, sorted order */, int32_t* rootCount /* host, C x (root, n) */,
                        float* bbox /* host, C x 6 */);
int sph_component_diagnostics(sph_solver* s, const int32_t* components /* host, count ids */, int32_t count,
                              double* out /* host, count x SPH_DIAG_WORDS */);

/* ---- Particle selection, free-surface measure and compact read-back (no reference counterpart) --------------------------------
 * State: the sorted state of the last completed step and that step's neighbour rows, exactly as sph_label_components describes
 * them (one integration step behind sph_read_position). row(i) = the 32 slots of sorted particle i as sph_read_neighbor_rows
 * returns them (-1 = empty).
 * SURFACE MEASURE m_i of sorted particle i, all float, in the written order, no contraction, IEEE division and square root:
 *   W = Bx = By = Bz = 0
 *   for slot k = 0 .. 31 in ascending order, j = row(i)[k], skipped when j < 0 or j == i:
 *     dx = x_j - x_i, dy = y_j - y_i, dz = z_j - z_i           (sorted positions, scene units)
 *     r2 = dx*dx + dy*dy + dz*dz                                (the sampling contract's expression and order)
 *     t  = hs2 - r2*ss2                                         (hs2, ss2 as in the sampling contract)
 *     skipped when !(t > 0)                                     (the rows hold entries at or beyond h: the search admits 31h/30)
 *     w  = (t*t)*t;  W += w;  Bx += w*dx;  By += w*dy;  Bz += w*dz
 *   if W == 0:  m = 1.0f
 *   else:       cx = Bx/W, cy = By/W, cz = Bz/W;  m = sqrtf((cx*cx + cy*cy) + cz*cz) / h
 * i.e. the distance from the particle to the kernel-weighted centroid of the neighbours the step used, in units of h: 0 in a
 * symmetric neighbourhood, 1 by definition for a particle without neighbours, never above 1 up to rounding. Neighbours of every
 * type count (liquid at a wall or at an elastic shell is not "surface"), selected or not. The quotients are taken BEFORE the
 * squares: w is about 1e-31 with the usual simulationScale, and Bx*Bx would underflow float to 0.
 * sph_particle_measure writes m for every sorted particle.
 * SELECTION: sorted particle j is selected when all of these hold:
 *   - sph_diagnostics selects it for region6 with typeMask (type, cell key < gridCellCount, half-open float box; region6 == NULL
 *     is "everything");
 *   - for each of the termCount (0 .. SPH_SELECT_MAX_TERMS) terms {field, lo, hi}: q >= lo && q < hi in float, where q for field
 *     0..6 is bit for bit the q of sph_histogram for that field (density, speed, pressure, neighbour count as a float, x, y, z)
 *     and field 7 (SPH_SELECT_FIELD_SURFACE) is m_j. lo may be -infinity and hi +infinity; a NaN q fails the term;
 *   - if component >= 0: labels[j] == component in the solver's current labelling (sph_label_components).
 * The selection is the list of the selected sorted indices IN ASCENDING ORDER; every entry is a function of the state and the
 * arguments, and nothing in it depends on launch geometry or execution order. *count receives its length. It lives in device
 * memory owned by the solver until the next sph_select_particles or sph_destroy.
 * READ-BACK: sph_read_selection(s, sortedIndex, origId, records); any pointer may be NULL. Entry r describes selected particle
 * j = sortedIndex[r]: origId[r] is its particleIndex value (the mapping of word 22 of the diagnostics record), records[r] is
 * SPH_SELECT_WORDS floats { x, y, z, type, vx, vy, vz, rho, p, neighbour count, m, 0 }, each word bit-identical to what the
 * existing exports give for particle j (sortedPosition xyz, sortedVelocity, rho, pressure, the histogram's field 3) and to
 * sph_particle_measure. type is the particle's position.w bit pattern (1, 2.x, 3: sph_read_position's .w of particle origId[r]),
 * not the .w of the exported sortedPosition, which carries the cell id in the reference's layout.
 * Rules: blocking, on the solver's stream, read-only on every solver array (a mesh stays valid for sph_surface_normals, a
 * labelling for sph_component_diagnostics), not stages (no stage timing). SPH_ERR_ORDER before a step's neighbour, density and
 * pressure-force stages have run; for sph_read_selection before any successful selection and, because it gathers from the live
 * state, once any stage, step or slab call has run since the selection; for component >= 0 without a labelling of the current
 * state. SPH_ERR_INVALID for a slab solver, a typeMask of 0 or with bits outside 1..3, a NaN region bound, termCount outside
 * 0..SPH_SELECT_MAX_TERMS or null terms with termCount > 0, a field outside 0..7, a NaN bound or lo >= hi, component < -1 or
 * >= the labelling's component count, a null count or out. Zero selected particles is legal. A failed selection leaves none
 * behind. Device memory: 4 bytes per SELECTED particle for the list (sized from a counting pass), 40 bytes per 256 particles for
 * the scan (a 1-bit-per-particle mask of the counting pass, block counts and offsets), and the sampling scratch (at most 64 MiB)
 * as staging for the records and the measure, which go to the host in pieces; grown on demand, freed by sph_destroy. */
#define SPH_SELECT_WORDS 12
#define SPH_SELECT_MAX_TERMS 4
#define SPH_SELECT_FIELD_SURFACE 7
typedef struct sph_select_term { int32_t field; float lo, hi; } sph_select_term;
int sph_particle_measure(sph_solver* s, float* out /* host, N floats, sorted order */);
int sph_select_particles(sph_solver* s, const float* region6 /* host or NULL */, uint32_t typeMask,
                         const sph_select_term* terms /* host, termCount */, int32_t termCount, int32_t component /* -1 = any */,
                         int64_t* count);
int sph_read_selection(sph_solver* s, int32_t* sortedIndex /* host, count */, uint32_t* origId /* host, count */,
                       float* records /* host, count x 12 */);

/* ---- Elastic-matter diagnostics (spring strain, muscle groups, membranes; no reference counterpart) ----------------------------
 * State: the sorted state of the last completed step, as sampling and diagnostics (one integration step behind
 * sph_read_position): positions are the sorted positions the step's stages ran on, the sorted index of original id o is
 * particleIndexBack[o], the tables are the connection table, the membrane table and elasticOffset given to sph_create, and the
 * muscle signal is the one sph_update_muscles stored last. Hence r and dr below are the values the step's elastic-force stage
 * used, provided the signal has not been changed since that step.
 * CONNECTION: row index in 0..numOfElasticP-1, slot nc in 0..31 of the connection table; conn = (x, y, z, w) of that slot. A
 * row ends at the first slot with (int)conn.x == -1, as in the elastic-force stage; the slots before it are LIVE, the others
 * dead. Connections are DIRECTED: a spring that is listed from both of its ends is two connections, one owned by each end, and
 * every count and sum below counts it twice. Per live connection, in float, in the written order, no contraction, IEEE division
 * and square root:
 *   i = particleIndexBack[index + elasticOffset] (the owning end), j = particleIndexBack[(int)conn.x]
 *   v = (x_i - x_j) * simulationScale per coordinate;  r = sqrtf(((vx*vx + vy*vy) + vz*vz) + 0.f*0.f)
 *   L0 = conn.y;  dr = r - L0;  e = dr / L0, or e = 0 when !(L0 > 0)
 *   group m = (int)conn.z if 1 <= m <= muscleCount, else 0 (no muscle);  sig = signal[m - 1] for m > 0
 *   only when r != 0:  spring term s = -(v / r) * dr * 600000000.f per coordinate, and, only when m > 0 && sig > 0,
 *                      contraction term c = -(v / r) * sig * 800.f per coordinate       (both exactly as the stage adds them)
 * sph_elastic_measure: one row per elastic particle in connection-table order; any pointer may be NULL. sortedIndex = i,
 * origId = index + elasticOffset (the particleIndex value of sorted particle i). records: SPH_ELASTIC_WORDS floats
 *   { n, nMuscle, eMin, eMax, eSum, sum dr*dr, sx, sy, sz, cx, cy, cz }
 * n = live slots, nMuscle = live slots with m > 0; eMin / eMax are float compares canonicalised by + 0.0f, 0 when n == 0; the
 * four scalar and vector sums start from +0.0f and are added in ascending slot order (s only for the slots with r != 0, c only
 * for those that have a contraction term), so s and c are the spring and contraction accelerations the step applied to the
 * particle, each as a sum of its own. connections: (r, dr) per slot, (-1, 0) for a dead slot.
 * sph_muscle_diagnostics: record 0 holds the live connections of no muscle group (m == 0), record m those of muscle m;
 * SPH_MUSCLE_WORDS doubles each:
 *   0 n                      1 signal (float widened; 0 for record 0)
 *   2 sum L0                 3 sum r                   4 sum dr             5 sum (dr*dr as float)
 *   6 sum e                  7 min e                   8 max e              9 sum (dr * 600000000.f as float)
 *   10 sum (sig * 800.f as float) over the connections with r != 0 && sig > 0
 *   11..13 sum x_i, y_i, z_i of the owning end (scene units)                14 connections with r == 0          15 0
 * Every spring of the reference's generator is listed from both ends, so words 11..13 divided by n are the centroid of the
 * group's spring midpoints. Each term is a float widened to double; the sums use the fixed tree reduce(a) of sph_diagnostics
 * above over the numOfElasticP * 32 slot terms in table order (row-major, slot fastest), where a slot that is dead or belongs
 * to another group contributes +0.0: a record depends on nothing but the state, the tables and the signal, and not on
 * muscleCount's other groups. Extremes as in sph_diagnostics: float compares, + 0.0f, widened, 0 when n == 0.
 * sph_membrane_measure: per triangle (a, b, c) of original ids, positions p = sortedPosition[particleIndexBack[.]], in float and
 * scene units: e1 = b - a, e2 = c - a, n = (e1y*e2z - e1z*e2y, e1z*e2x - e1x*e2z, e1x*e2y - e1y*e2x),
 * len = sqrtf((nx*nx + ny*ny) + nz*nz), area = 0.5f * len, unit normal n / len (0 when len == 0), centroid ((a + b) + c) / 3.0f;
 * record { area, nx, ny, nz, cx, cy, cz, 0 }. totals = { count, sum area (the same fixed tree over the triangles in table order,
 * areas widened), min area, max area (as the extremes above) }. out may be NULL. There is no signed volume: the reference
 * generator's worm mesh is closed but not consistently oriented, so a divergence-theorem volume would mean nothing.
 * Rules: blocking, on the solver's stream, read-only on every solver array (meshes, labellings and selections stay valid), not
 * stages (no stage timing). SPH_ERR_ORDER before a step's density and pressure-force stages have run. SPH_ERR_INVALID for a slab
 * solver, a solver without elastic matter (numOfElasticP == 0), sph_membrane_measure with numOfMembranes == 0, a null out of
 * sph_muscle_diagnostics or null totals, and a connection or membrane id outside 0..N-1 met on the device (reported, never
 * followed; the outputs are then unspecified). A blown-up state is reported as by every blocking call. Device scratch, grown on
 * demand and freed by sph_destroy: 312 bytes per elastic particle for sph_elastic_measure; (muscleCount + 1) x 128 bytes per
 * 1024 slots (32 elastic particles) for sph_muscle_diagnostics; 32 bytes per triangle for sph_membrane_measure. */
#define SPH_ELASTIC_WORDS 12
#define SPH_MUSCLE_WORDS 16
#define SPH_MEMBRANE_WORDS 8
int sph_elastic_measure(sph_solver* s, int32_t* sortedIndex /* host, numOfElasticP */, uint32_t* origId /* host, numOfElasticP */,
                        float* records /* host, numOfElasticP x 12 */, float* connections /* host, numOfElasticP x 32 x 2 */);
int sph_muscle_diagnostics(sph_solver* s, double* out /* host, (muscleCount + 1) x SPH_MUSCLE_WORDS */);
int sph_membrane_measure(sph_solver* s, float* out /* host, numOfMembranes x 8, or NULL */, double totals[4]);

/* ---- Force decomposition (which matter pushes on which; no reference counterpart) ------------------------------
 * The viscous, surface-tension and pressure accelerations of the step's kernels K7 (computeForcesAndInitPressure) and K12
 * (computePressureForceAcceleration), recomputed once and kept apart by the class of the neighbour that exerted them.
 * State: the sorted state of the last completed step and that step's neighbour rows, as sph_select_particles describes them:
 * x, v, rho, rhoStar (the predicted density, second half of buffer "rho") and p of the last predict-correct iteration;
 * row(i)[k] and dist(i)[k] are what sph_read_neighbor_rows returns for sorted particle i. hs = h * simulationScale,
 * simScale = simulationScale, and massMu, closeRf, rho0delta, del2W, massGradW are the step's own constants: (float)(mass *
 * viscosity); the smallest float >= 0.5 * (double)(float)(hs / 2); (float)(rho0 * delta); del2WviscosityCoefficient;
 * (double)mass * gradWspikyCoefficient.
 * CLASS of a neighbour j: c = (int)sortedPosition[j].w: 1 liquid, 2 elastic, 3 boundary.
 * For a sorted particle i that is not a boundary particle, the slots k = 0..31 in ascending order, j = row(i)[k]; all
 * arithmetic in float in the written order, no contraction, IEEE division and square root:
 *   K7 terms, used when j != -1 && dist(i)[k] < hs, with rk = dist(i)[k] the STORED distance:
 *     tv = ((v_j - v_i) * (hs - rk)) / rho_j  per component; v_j of a BOUNDARY neighbour is its wall normal, which the
 *          boundary keeps in its velocity slot: the reference adds it as if it were a velocity (sphFluid.cl:653), and so does
 *          this decomposition, because it reports what the step computed
 *     tt = surfTensCoeff * (x_i - x_j)        per component (scene units, as the reference)
 *   K12 terms, used when j != -1 && r < hs:
 *     e = x_i - x_j;  r = sqrtf(ex*ex + ey*ey + ez*ez) * simScale
 *     num = -(hs - r) * (hs - r) * 0.5f * (p_i + p_j);  when r < closeRf: num = -(hq - r) * (hq - r) * 0.5f * rho0delta,
 *     hq = hs * 0.25f;  value = num / rhoStar_j;  tq = (value * (e * simScale)) / r  per component
 * SUMS, sequential float sums that start at +0 and run in slot order (a slot that is not used leaves a sum untouched):
 *   V, T, P over all used slots (the step's own sums); V_c, T_c, P_c over the used slots of class c; n_c = K7-used slots of class c.
 * SCALES, the step's own: sF = massMu * (float)(del2W / (double)rho_i);  sP = (float)(massGradW / (double)rhoStar_i).
 * RECORD, SPH_FORCE_WORDS floats per particle:
 *   0..8     class 1 (what the liquid exerts): V_1*sF (xyz), T_1 (xyz), P_1*sP (xyz)
 *   9..17    class 2 (elastic matter), 18..26 class 3 (boundary): the same nine words
 *   27..29   n_1, n_2, n_3 as floats
 *   30..32   aF = V*sF + g + T per component, exactly as K7 writes the acceleration (sx*scale + gravity_x + tx)
 *   33..35   aP = P*sP, the pressure acceleration of the last K12          36..39   0
 * A boundary particle's record is all zero. Values are ACCELERATIONS of particle i; the force is cfg.mass times them.
 * Words 30..32 equal buffer "acceleration"[i] wherever the elastic-force stage added nothing (every liquid particle); words
 * 33..35 equal its second half for every non-boundary particle.
 * sph_force_measure: fromSelection = 0 writes one record for each of the N sorted particles, in sorted order; fromSelection = 1
 * writes the records of the particles of the current selection (sph_select_particles), in its order, sph_read_selection's
 * count of them, under sph_read_selection's SPH_ERR_ORDER rules (no selection, or the state has changed since). The records
 * travel to the host in pieces through the sampling scratch.
 * sph_force_diagnostics: selection, region rules, count limit and errors exactly as sph_diagnostics. Per-particle terms, floats
 * widened to double, an unselected particle contributing +0.0, summed by the fixed tree reduce(a) of sph_diagnostics over all N
 * terms in ascending sorted index. With visc_c, tens_c, pres_c the record's words of class c, per component and in float:
 *   h_c = (visc_c + pres_c) + tens_c;  tau_c = x_i x h_c = (y*hz - z*hy, z*hx - x*hz, x*hy - y*hx);
 *   w_c = (h_c.x*v_x + h_c.y*v_y) + h_c.z*v_z
 * Record, SPH_FORCE_DIAG_WORDS doubles per region:
 *   0        n, the number of selected particles       1..27    sum of record words 0..26
 *   28..30   sum aF          31..33   sum aP           34..42   sum tau_c for c = 1, 2, 3 (torque about the origin per unit mass)
 *   43..45   sum w_c (power per unit mass)             46..48   sum n_c             49..63   0
 * SCOPE. Only K7 and K12 are decomposed. The spring and muscle accelerations are sph_elastic_measure's. The boundary hand-off
 * inside integrate and the membrane interaction are position corrections, not forces, and are not reported here
 * (sph_wall_measure reports the former). The reference's
 * pressure term divides by rhoStar_j, so it is not antisymmetric: the reaction on class c is only approximately minus what
 * class c exerts, and no word here pretends otherwise.
 * Rules: blocking, on the solver's stream, read-only on every solver array (a mesh, a labelling, a selection and a render stay
 * valid), not stages (no stage timing). SPH_ERR_ORDER before a step's neighbour, density, force and pressure-force stages have
 * run. SPH_ERR_INVALID for a slab solver, null pointers, fromSelection outside 0..1, a typeMask of 0 or with bits outside 1..3,
 * count outside 1..SPH_DIAG_MAX_REGIONS, a NaN region bound. A blown-up state is reported as by every blocking call. Device
 * scratch, grown on demand and freed by sph_destroy: the sampling scratch (at most 64 MiB) and 512 bytes per region and 1024
 * particles for the totals. */
#define SPH_FORCE_WORDS 40
#define SPH_FORCE_DIAG_WORDS 64
int sph_force_measure(sph_solver* s, int32_t fromSelection, float* out /* host, N (or the selection's count) x 40 */);
int sph_force_diagnostics(sph_solver* s, const float* regions6 /* host, count x (x0,y0,z0,x1,y1,z1) */, int32_t count,
                          uint32_t typeMask, double* out /* host, count x 64 */);

/* ---- Particle rendering: depth, id, colour and thickness images (no reference counterpart in the solver: the
 * reference's viewer, owWorldSimulation.cpp, draws every particle each frame) ---------------------------------------------------
 * sph_render_particles draws the selected particles of the sorted state of the last completed step (the state sph_sample_*
 * describes: one integration step behind sph_read_position) as shaded spheres into images that stay on the device;
 * sph_read_render copies them out. Everything is a function of the state and the arguments alone: the only cross-lane operations
 * are 64-bit integer min and add atomics, ballots and popcounts; no floating-point atomics; no dependence on launch geometry.
 * SELECTION: sorted particle j is a candidate when sph_diagnostics would select it for region6 (NULL = everything) and typeMask
 * (type bit, cell key < number of cells, half-open box); the box doubles as a cut-away.
 * PROJECTION, all in float, in the written order, no contraction, IEEE division and square root:
 *   d = x_j - eye per coordinate;  cx = (d.x*right.x + d.y*right.y) + d.z*right.z;  cy likewise with up, cz with forward
 *   k = scale / cz (perspective) or k = scale (orthographic);  u = cx*k + centre[0];  v = centre[1] - cy*k  (row 0 is the top)
 *   R = radius*k;  R2 = R*R
 * The particle is DRAWN when cz > nearPlane, R > 0, R <= maxRadiusPx, fabsf(u) < 1048576.f and fabsf(v) < 1048576.f (NaN fails
 * every test). right / up / forward are used as given (the caller's orthonormal frame; frames.look_at makes one).
 * FRAGMENTS: pixel (px, py) has its centre at ((float)px + 0.5f, (float)py + 0.5f); dx = centre.x - u, dy = centre.y - v,
 * d2 = dx*dx + dy*dy; the pixel is covered when d2 <= R2; nz = sqrtf(1.0f - d2/R2); depth = cz - radius*nz; the fragment exists
 * when depth > nearPlane. The pixel set is that test over the whole image (the kernels search floor(u-R)-1 .. floor(u+R)+1 and
 * likewise in y, which contains it). Under perspective this is a sphere IMPOSTOR: a disc of the projected radius at the centre's
 * depth, shaded and offset in depth like a sphere seen along the view axis, not the true perspective outline of a sphere.
 * WINNER: key = ((uint64)bits(depth) << 32) | j; depth is positive, so its bit pattern orders as the float does. A pixel holds
 * the minimum key over its fragments: the nearest fragment, and on equal depth bits the lower sorted index. Images, row-major
 * [height][width]: depth (float; +inf where uncovered), sortedIndex (int32; -1), origId (uint32, the winner's particleIndex value;
 * 0xFFFFFFFF), rgba (4 bytes; background).
 * COLOUR of a covered pixel: the winner's u, v, R2 and nz are recomputed by the same expressions; base colour c per channel:
 *   mode 0  typeColour[t - 1], t = (int)position.w
 *   mode 1  the reference viewer's density ramp (owWorldSimulation.cpp:127-141, frames.density_colour) of rho_j against rho0, for
 *           every type: rho clipped to [0, 2.0f*rho0]; c = (0, 0, 1); then for f in 1.00f, 1.01f, 1.02f, 1.03f, 1.04f in this
 *           order dc = (100.0f*(rho - rho0*f))/rho0 and, when dc > 0, c = (0, dc, 1), (0, 1, 1 - dc), (dc, 1, 0), (1, 1 - dc, 0),
 *           (1, 0, 0) respectively (later ramps win)
 *   mode 2  q = sph_histogram's quantity for `field`; s = fminf(fmaxf((q - lo)*inv, 0.f), 1.f) with inv = 1.0f/(hi - lo) computed
 *           once on the host; a = s*4.0f; i = min((int)a, 3); f = a - (float)i; c = stop[i] + f*(stop[i+1] - stop[i]) over
 *           SPH_RENDER_FIELD_RAMP (a NaN q gives s = 0)
 *   mode 3  SPH_RENDER_LABEL_PALETTE[label % 12] of the current sph_label_components labelling; (0.5, 0.5, 0.5) for a label < 0
 * then shade = ambient + (1.0f - ambient)*nz, byte = (uint8)(int)(fminf(fmaxf(c*shade, 0.f), 1.f)*255.0f + 0.5f), A = 255.
 * THICKNESS (wantThickness != 0): every fragment, not only the winner, adds (uint32)(int)(nz*256.0f + 0.5f) to its pixel: the
 * chord 2*radius*nz in units of radius/128, an X-ray column of the selected matter. The sum is a 64-bit integer (integer adds
 * commute), returned saturated to uint32; 0 where uncovered.
 * counts = { particles drawn (candidates that pass the five tests above, whether or not a fragment lands in the image), covered
 * pixels }. The images live in device memory owned by the solver until the next render or sph_destroy; they are self-contained:
 * sph_read_render returns the same bytes after further steps. Any pointer of sph_read_render may be NULL.
 * Rules: blocking, on the solver's stream, read-only on every solver array (meshes, labellings and selections stay valid), not a
 * stage (no stage timing). SPH_ERR_ORDER before a step's density and pressure-force stages have run (mode 2 with field 3: the
 * neighbour stage too), for mode 3 without a labelling of the current state, and for sph_read_render before any successful render.
 * SPH_ERR_INVALID for a slab solver, a bad typeMask, a NaN region bound, a null view or counts, any field of the view outside the
 * ranges below or not finite, and thickness != NULL after a render made without it. A failed render leaves no image behind.
 * Device memory, grown on demand: 24 bytes per pixel (36 with thickness) and 4 bytes per particle. */
typedef struct sph_render_view {
  int32_t width, height;        /* 1..8192 each, width*height <= 1<<24 */
  int32_t projection;           /* 0 orthographic, 1 perspective */
  float eye[3], right[3], up[3], forward[3];   /* the caller's orthonormal frame; used as given, only checked finite */
  float scale;                  /* orthographic: pixels per scene unit; perspective: focal length in pixels; > 0 */
  float centre[2];              /* principal point in pixels */
  float nearPlane;              /* >= 0, finite */
  float radius;                 /* sphere radius in scene units, > 0 */
  float maxRadiusPx;            /* 0 < . <= 4096 */
  int32_t colourMode;           /* 0 type, 1 density (the viewer's ramp), 2 field, 3 component label */
  int32_t field; float lo, hi;  /* mode 2: sph_histogram's field 0..6, lo < hi, finite */
  float typeColour[3][3];       /* mode 0: rgb for liquid, elastic, boundary */
  float ambient;                /* 0..1 */
  uint8_t background[4];        /* RGBA of an uncovered pixel */
} sph_render_view;
/* the five stops of mode 2: blue, cyan, green, yellow, red */
#define SPH_RENDER_FIELD_RAMP { {0.f, 0.f, 1.f}, {0.f, 1.f, 1.f}, {0.f, 1.f, 0.f}, {1.f, 1.f, 0.f}, {1.f, 0.f, 0.f} }
/* the twelve colours of mode 3, label % 12 */
#define SPH_RENDER_LABEL_COLOURS 12
#define SPH_RENDER_LABEL_PALETTE { {0.90f, 0.10f, 0.10f}, {0.10f, 0.50f, 0.90f}, {0.20f, 0.70f, 0.20f}, {0.95f, 0.60f, 0.10f}, \
                                   {0.60f, 0.30f, 0.80f}, {0.10f, 0.75f, 0.75f}, {0.95f, 0.90f, 0.20f}, {0.85f, 0.35f, 0.65f}, \
                                   {0.55f, 0.35f, 0.15f}, {0.40f, 0.85f, 0.55f}, {0.30f, 0.30f, 0.65f}, {0.75f, 0.75f, 0.75f} }
int sph_render_particles(sph_solver* s, const sph_render_view* view, const float* region6 /* or NULL */, uint32_t typeMask,
                         int32_t wantThickness, int64_t counts[2] /* particles drawn, covered pixels */);
int sph_read_render(sph_solver* s, float* depth, int32_t* sortedIndex, uint32_t* origId, uint8_t* rgba /* 4 per pixel */,
                    uint32_t* thickness);  /* host, width x height each; any may be NULL */

/* ---- Triangle rendering: the extracted surface and the membranes in the same images (the reference's viewer draws
 * the membrane table, owWorldSimulation.cpp) -----------------------------------------------------------------------------------
 * sph_render_mesh draws a triangle table into the images of sph_render_particles, as a fresh render (compose 0) or over the
 * images of the last successful render, depth-correct (compose 1). Coverage is decided in integers, so every word is a function
 * of the inputs alone. `view` is checked exactly as by sph_render_particles; its radius, maxRadiusPx, colourMode, field, lo, hi and
 * typeColour are not used, ambient and background are.
 * VERTICES. source 0: vertex i of the mesh of the last sph_extract_surface, at its float coordinates. source 1: the membrane table
 * given to sph_create; corner o (an original id) is at sortedPosition[particleIndexBack[o]], the state of sph_membrane_measure.
 * Projection is sph_render_particles' PROJECTION up to v (d, cx, cy, cz, k, u, v in float, in that order, no contraction). A
 * vertex is USABLE when cz > nearPlane, fabsf(u) < 1048576.f and fabsf(v) < 1048576.f. Snap: X = (int)floorf(u*256.0f + 0.5f),
 * Y likewise from v (1/256-pixel fixed point); zi = 1.0f/cz under perspective, zi = cz under orthographic.
 * TRIANGLE t = (a, b, c) in table order is SKIPPED when any corner is not usable (there is NO NEAR-PLANE CLIPPING: a triangle that
 * crosses the near plane is not drawn) or when A = E(a, b, c) == 0, with
 *   E(p, q, r) = (int64)(Xq - Xp)*(Yr - Yp) - (int64)(Yq - Yp)*(Xr - Xp)     (operands below 2^29: exact)
 * When A < 0, b and c are exchanged for everything that follows and A is negated. It is DRAWN otherwise, whether or not a pixel is
 * hit.
 * COVERAGE. Pixel (px, py) has its centre at P = (256*px + 128, 256*py + 128); w0 = E(b, c, P), w1 = E(c, a, P), w2 = E(a, b, P).
 * Edge p -> q with dx = Xq - Xp, dy = Yq - Yp OWNS ITS LINE when dy > 0 || (dy == 0 && dx < 0). The pixel is covered when each
 * wi > 0, or wi == 0 and that edge (b -> c, c -> a, a -> b) owns its line. An edge and its reverse get opposite verdicts: two
 * triangles that share an edge never both cover a pixel centre on it, and a closed mesh covers every pixel an even number of times.
 * The pixel set is that test over the whole image (the kernels search the box floor(min) .. floor(max) of the snapped corners in
 * pixels, clipped to the image, which contains it).
 * FRAGMENT. l1 = (float)w1/(float)A, l2 = (float)w2/(float)A (int64 -> float round to nearest, IEEE division);
 * z = (zi_a + l1*(zi_b - zi_a)) + l2*(zi_c - zi_a); depth = 1.0f/z under perspective, z under orthographic. The fragment exists
 * when depth > nearPlane and depth is finite. key = ((uint64)bits(depth) << 32) | t; the pixel keeps the minimum key: the nearest
 * fragment, and on equal depth bits the lower triangle index.
 * RESOLVE, once per pixel, the winner recomputed by the same expressions. Flat normal (shading 0): sph_membrane_measure's, from
 * the three scene positions in table order: e1 = b - a, e2 = c - a, n = e1 x e2, len = sqrtf((nx*nx + ny*ny) + nz*nz), n/len or 0
 * when len == 0. Smooth normal (shading 1, source 0 only): n = (na + l1*(nb - na)) + l2*(nc - na) per component from the normals
 * sph_surface_normals defines (computed on the device), len as above, n/len, or 0 when len is 0 or not finite.
 * facing = fabsf((nx*forward.x + ny*forward.y) + nz*forward.z) (two-sided: the membranes are not consistently oriented);
 * shade = ambient + (1.0f - ambient)*facing. Base colour: `colour` (colourMode 0) or the ramp of sph_render_particles' mode 2 of
 * q = (qa + l1*(qb - qa)) + l2*(qc - qa), with inv = 1.0f/(hi - lo) computed once on the host (a NaN q gives s = 0). The vertex
 * scalar: source 0, field 0..5 = that word of the sph_sample_points record at the vertex with the extraction's typeMask, field 6
 * = sqrtf((vx*vx + vy*vy) + vz*vz) of its words 2..4; source 1, sph_histogram's quantity `field` of the corner's sorted particle.
 * Bytes as sph_render_particles, A = 255.
 * IMAGES. compose 0: depth, rgba and the triangle image (int32; the winning t, -1 where none) come from the mesh; sortedIndex = -1
 * and origId = 0xFFFFFFFF everywhere; no thickness. compose 1: the mesh takes a pixel when its depth < the depth image's value
 * there (a float compare; a tie stays with what is there); taken pixels get the mesh's depth and rgba, sortedIndex = -1,
 * origId = 0xFFFFFFFF and triangle = t; every other pixel keeps its bytes and gets triangle = -1; a thickness image stays as it is.
 * counts = { triangles drawn, triangles skipped, pixels the mesh holds, pixels covered by anything }. sph_read_render keeps working
 * on the result; sph_read_render_triangles copies the triangle image out; a later sph_render_particles drops it.
 * Rules: blocking, on the solver's stream, read-only on every solver array (the mesh, a labelling, a selection and the fields stay
 * valid), not a stage. SPH_ERR_ORDER before a step's density and pressure-force stages have run; for source 0 before any
 * extraction, and with shading 1 or colourMode 1 once the state has changed since the extraction (sph_surface_normals' rule; flat
 * shading with a constant colour draws a stale mesh); for source 1 with colourMode 1 and field 3 before the neighbour stage; for
 * compose 1 without a successful render; for sph_read_render_triangles when the last render had no mesh pass. SPH_ERR_INVALID for
 * a slab solver, null pointers, a view sph_render_particles would refuse, any style field out of range or not finite, shading 1
 * with source 1, source 1 without membranes, and compose 1 when width .. nearPlane of `view` differ in any byte from the last
 * render's. A membrane corner outside 0..N-1 is reported as by sph_membrane_measure and never followed. A failed call leaves the
 * previous images as they were under compose 1 and none under compose 0.
 * Device memory, grown on demand and freed by sph_destroy: the render buffer (its key plane is reused), 4 bytes per pixel for the
 * triangle image, 32 bytes per vertex (44 with smooth shading; 92 with colourMode 1 on source 0: query points and sample records)
 * and 4 bytes per triangle for the queue of large triangles. Source 1 has three vertices per membrane triangle. */
typedef struct sph_render_mesh_style {
  int32_t source;      /* 0: the mesh of the last sph_extract_surface; 1: the membrane triangles (sph_create's table) */
  int32_t shading;     /* 0 flat (face normal); 1 smooth (vertex normals; source 0 only) */
  int32_t colourMode;  /* 0 constant `colour`; 1 a per-vertex scalar through SPH_RENDER_FIELD_RAMP */
  int32_t field;       /* mode 1. source 0: 0..5 = that word of the sample record at the vertex, 6 = speed.
                          source 1: sph_histogram's field 0..6 of the corner's sorted particle */
  float lo, hi;        /* mode 1: lo < hi, finite */
  float colour[3];     /* mode 0: finite */
  int32_t compose;     /* 0: a fresh image; 1: over the images of the last successful render */
} sph_render_mesh_style;
int sph_render_mesh(sph_solver* s, const sph_render_view* view, const sph_render_mesh_style* style,
                    int64_t counts[4] /* triangles drawn, triangles skipped, pixels won by the mesh, covered pixels */);
int sph_read_render_triangles(sph_solver* s, int32_t* triangle /* host, width x height; -1 where no triangle won */);

/* ---- Particle editing: emitters, drains, gates (no reference counterpart: the reference fixes the particle set
 * when the solver is made) -----------------------------------------------------------------------------------------------------
 * Particles are removed from and appended to a live solver between two steps, within the capacity given to sph_create.
 * STATE: the edits act on the CURRENT state, the one sph_read_position and sph_read_velocity return in original-id order, not on
 * the sorted state one step behind it that the analysis calls read. Between two steps that pair of arrays IS the solver's state
 * (the step rewrites every other array before it reads it), so an edited solver continues bit for bit like a solver newly
 * created from the edited arrays.
 * MARKING. sph_remove_region marks particle o when (int)position[o].w is 1, 2 or 3 with that bit set in typeMask and its float
 * position lies in the half-open box x0 <= x < x1, y0 <= y < y1, z0 <= z < z1, compared as sph_diagnostics compares (bounds of
 * +-infinity allowed, region6 == NULL is "everywhere"). There is no cell-key condition: the keys are stale at this point. With
 * countOnly != 0 it only writes *removed, the number of marked particles: no solver array is touched, the analysis state and the
 * edit map stay as they were ("is the inlet clear?"). sph_remove_selection marks origId[r] of every entry of the live selection
 * of sph_select_particles, under the epoch rule of sph_read_selection. sph_remove_ids marks the listed original ids; duplicates
 * are allowed; an id >= N is SPH_ERR_INVALID and nothing changes.
 * REMOVAL is a stable compaction: the unmarked particles keep their relative order, survivor o gets the new id
 * o - #(marked ids below o), and position and velocity move together. *removed receives the number removed.
 * sph_read_edit_map returns newIdOfOld[o] for every o below the count BEFORE the last removal: the new id, or -1 for a removed
 * particle. The map stays readable until the next stage, step or edit that changes the set; after that it is SPH_ERR_ORDER.
 * Removing NOTHING succeeds and changes nothing: no array is touched, the analysis state, meshes, labellings and selections stay
 * valid, and the edit map becomes the identity of the current count. Removing EVERYTHING is SPH_ERR_INVALID with the state
 * untouched: a solver holds at least one particle.
 * ELASTIC MATTER: with numOfElasticP > 0 a removal that marks an id below elasticOffset + numOfElasticP is SPH_ERR_INVALID, the
 * error names the lowest such id, and nothing changes: the connection, membrane and muscle tables address original ids in that
 * range, so those ids never shift. Liquid stored behind the elastic block (generated scenes: elastic, liquid, boundary; file-mode
 * scenes: boundary, elastic, liquid) can be drained; walls stored in front of it cannot; elastic particles are never removed or
 * added.
 * ADDING. sph_add_particles appends count particles at ids N .. N+count-1 in the given order. Each gets the validation of
 * sph_create (finite coordinates; inside the box with wide cell ids) and (int)w must be 1 or 3; the first offender is named and
 * nothing is committed unless all pass. N + count > capacity is SPH_ERR_SIZE. The liquid signature of
 * sph_slab_liquid_signature is folded exactly as sph_create folds it. sph_emit_lattice does the same without a host array: it
 * appends dims[0]*dims[1]*dims[2] particles in ascending k = (iz*ny + iy)*nx + ix (x fastest) at origin + (float)i * spacing per
 * axis (one float multiply, one float add, no contraction: the lattice of sph_sample_grid), position.w = typeValue, velocity =
 * (vx, vy, vz, 0). The points are generated and validated on the device in the unused tail of the arrays; the count is raised,
 * and *added written, only if every point passed.
 * EVERY SUCCESSFUL EDIT THAT CHANGES THE SET updates the particle count (sph_particle_count), and invalidates the sorted state:
 * every analysis call returns SPH_ERR_ORDER until a step has run, exactly as on a new solver, and sph_read_selection,
 * sph_surface_normals and sph_component_diagnostics see a changed state. Until that step sph_read_density holds the previous
 * step's values in the previous sorted order, and the sorted exports of sph_read_buffer are undefined: a removal stages through
 * them (sortedPosition / sortedVelocity then hold the original-order arrays of before the removal, particleIndexBack the edit map). An outstanding sph_read_position_async finishes its device copy before an edit moves
 * anything; sph_read_position_wait then delivers the positions and the byte count of the time of the request.
 * Rules: blocking, on the solver's stream, not stages (no stage timing). SPH_ERR_INVALID for a slab solver, a typeMask of 0 or
 * with bits outside 1..3, a NaN region bound, null pointers, negative counts or dims. A count of 0 is a no-op. A failed call
 * leaves the solver exactly as it was. Device memory: 40 bytes per 256 particles for the scan (the layout of the selection's);
 * the compaction is staged through the sorted arrays, which the invalidation has just made dead. */
int sph_remove_region(sph_solver* s, const float* region6 /* host or NULL = everywhere */, uint32_t typeMask, int32_t countOnly,
                      int64_t* removed);
int sph_remove_selection(sph_solver* s, int64_t* removed); /* the current sph_select_particles list */
int sph_remove_ids(sph_solver* s, const uint32_t* origIds /* host */, int64_t count, int64_t* removed);
int sph_add_particles(sph_solver* s, const float* position4, const float* velocity4 /* host, count x 4 */, int32_t count);
int sph_emit_lattice(sph_solver* s, const float origin[3], const float spacing[3], const int32_t dims[3], const float velocity[3],
                     float typeValue /* position.w: 1.0f liquid */, int64_t* added);
int sph_read_edit_map(sph_solver* s, int32_t* newIdOfOld /* host, the count BEFORE the last removal */);

/* ---- Carried particle fields: paint, diffuse, measure a dye (no reference counterpart) -------------------------
 * Up to SPH_FIELD_SLOTS scalar float fields per solver, one value per particle, stored in ORIGINAL-id order (the order of
 * sph_read_position) and sized by the capacity given to sph_create. A step never reads or writes them; the edits carry them
 * along; the calls below paint them, diffuse them along the neighbour rows and reduce them.
 * STATE AND LIFETIME. A slot exists from sph_field_create to sph_field_release or sph_destroy. sph_field_create sets the N values
 * from valuesN (NULL: all +0) and remembers `inflow`, the value new particles receive. Creating a slot that exists, or using one
 * that does not, is SPH_ERR_ORDER; a slot outside 0..SPH_FIELD_SLOTS-1 is SPH_ERR_INVALID. Finite values only: a non-finite
 * value, inflow or coefficient is SPH_ERR_INVALID, and so is a non-finite entry of a host array, with the first offender named
 * and nothing written. No field call changes the solver's state: a mesh, a labelling, a selection, a render and an edit map stay
 * valid across all of them. sph_field_read, sph_field_write, sph_field_set_region and sph_field_set_selection act on the CURRENT
 * particle set, like the edits, and are legal at any time between steps, also right after an edit. sph_field_diffuse and
 * sph_field_diagnostics read the sorted state of the last completed step: SPH_ERR_ORDER before one, and after an edit until the
 * next step. sph_field_diffuse needs that step's neighbour and density stages, sph_field_diagnostics what sph_diagnostics needs.
 * PAINTING. sph_field_set_region marks particle o by the rule of sph_remove_region, word for word ((int)position[o].w is 1, 2 or
 * 3 with that bit set in typeMask; the float position in the half-open box; no cell-key condition; region6 == NULL is
 * "everywhere"), sets the marked particles to `value` and writes their number to *painted. sph_field_set_selection sets
 * origId[r] of every entry of the live selection of sph_select_particles, under the epoch rule of sph_read_selection, and
 * writes the selection's length.
 * EDITS CARRY THE FIELDS. A successful removal compacts every existing slot with the same old-to-new map as position and
 * velocity (sph_read_edit_map). A successful sph_add_particles or sph_emit_lattice gives the new ids the slot's inflow. A failed
 * or counting edit, and a removal of nothing, leave the fields untouched.
 * DIFFUSION is the viscous sum of the step's kernel K7 with the scalar in place of a velocity component. P(x) holds when the type
 * of sorted particle x is 1..3 with its bit in typeMask and its cell key is valid (as sph_diagnostics selects). row, dist, hs and
 * del2W as in the force decomposition above; c_x is the value of the particle whose original id is particleIndex[x]. For sorted
 * particle i with P(i), the slots k = 0..31 in ascending order, j = row(i)[k], rk = dist(i)[k]; a slot is USED when
 * j != -1 && rk < hs && P(j). All arithmetic in float in the written order, no contraction, IEEE division; the sums start at +0,
 * run in slot order, and a slot that is not used leaves them untouched:
 *     S_i = sum ((c_j - c_i) * (hs - rk)) / rho_j          W_i = sum (hs - rk) / rho_j
 *     sD_i = mass * (float)(del2W / (double)rho_i)         a_i = coefficient * sD_i
 *     c_i' = c_i + a_i * S_i                               sigma = max over P(i) of a_i * W_i, float compares from +0
 * A particle without P(i) keeps its value. `coefficient` is diffusivity x time in the units in which `viscosity` multiplies the
 * same sum; it is >= 0 (< 0: SPH_ERR_INVALID), and so is substeps. The update is JACOBI: every c' of a substep is computed from
 * the c of before that substep; it is repeated `substeps` times on the same rows and densities. *stability (may be NULL) receives
 * sigma, the same for every substep; substeps == 0 only measures sigma and changes nothing. Two properties: for sigma <= 1 each
 * new value is a convex combination of old ones (c_i' = (1 - a_i W_i) c_i + sum of non-negative weights times c_j), up to
 * rounding, so the field keeps its bounds; and the sum of c over the participants is conserved, up to rounding, exactly when the
 * used slots are symmetric (j used by i with the same distance whenever i is used by j; then the weight a_i (hs - rk) / rho_j is
 * mass * del2W * coefficient * (hs - rk) / (rho_i rho_j) both ways). That holds unless a row was truncated at 32 entries.
 * DIAGNOSTICS. sph_field_diagnostics: selection, region rules, count limit and errors exactly as sph_diagnostics. Per selected
 * particle c is widened to double. Record, SPH_FIELD_DIAG_WORDS doubles per region:
 *   0  n, the number of selected particles      1  sum c       2  sum c*c (the product in double)
 *   3  min c     4  max c (float compares, canonicalised by + 0.0f; 0 when n = 0)
 *   5  the number of selected particles with c != 0              6, 7  0
 * The sums are reduce(a) of sph_diagnostics over all N terms in ascending sorted index, an unselected particle contributing +0.0.
 * No floating-point atomics anywhere.
 * Rules: blocking, on the solver's stream, not stages (no stage timing). SPH_ERR_INVALID for a slab solver, null pointers (only
 * region6 and stability may be NULL), a typeMask of 0 or with bits outside 1..3, a NaN region bound, count outside
 * 1..SPH_DIAG_MAX_REGIONS. Device memory: 4 bytes per slot and particle of capacity, one more such buffer once a removal has
 * moved a field, and 16 bytes per particle for the diffusion's sorted records; grown on demand, freed by sph_field_release
 * (the slot) and sph_destroy. */
#define SPH_FIELD_SLOTS 4
#define SPH_FIELD_DIAG_WORDS 8
int sph_field_create(sph_solver* s, int32_t slot, const float* valuesN /* host, orig order, or NULL = all +0 */, float inflow);
int sph_field_release(sph_solver* s, int32_t slot);
int sph_field_write(sph_solver* s, int32_t slot, const float* valuesN /* host, N, orig order */);
int sph_field_read(sph_solver* s, int32_t slot, float* outN /* host, N, orig order */);
int sph_field_set_region(sph_solver* s, int32_t slot, const float* region6 /* or NULL */, uint32_t typeMask, float value,
                         int64_t* painted);
int sph_field_set_selection(sph_solver* s, int32_t slot, float value, int64_t* painted);
int sph_field_diffuse(sph_solver* s, int32_t slot, float coefficient, int32_t substeps, uint32_t typeMask, float* stability);
int sph_field_diagnostics(sph_solver* s, int32_t slot, const float* regions6 /* host, count x (x0,y0,z0,x1,y1,z1) */, int32_t count,
                          uint32_t typeMask, double* out /* host, count x 8 */);

/* ---- Kinematic bodies: groups of boundary particles moved between steps (no reference counterpart: the
 * reference's walls stay where the scene put them) -------------------------------------------------------------------------------
 * Up to SPH_MAX_BODIES bodies per solver. A body is an ORDERED list of original ids of boundary particles ((int)position.w == 3)
 * together with their REFERENCE PLACEMENT: the position float4 and the wall normal float4 (a boundary particle's velocity slot)
 * they had when the body was defined, kept on the device. sph_body_set_pose places the members at a rigid image of the reference
 * placement; the liquid answers through what the step already does with boundary neighbours (the density sum, and the position
 * and velocity correction of the integration). No step kernel knows about bodies.
 * STATE: like the particle edits above, the calls act on the CURRENT state (sph_read_position / sph_read_velocity, original-id
 * order). Between two steps that pair of arrays is the solver's state, so a solver whose walls were moved in place continues bit
 * for bit like a solver newly created from the moved arrays.
 * DEFINING. sph_body_define_ids keeps the members in the caller's order. An entry r is an OFFENDER when origIds[r] >= N, when
 * that particle is not a boundary particle, or when its id occurs more than once in the list (every occurrence counts). With any
 * offender the call is SPH_ERR_INVALID, the message names their number and the lowest offending list index, and the slot keeps
 * what it held. count == 0, count > N and a slot outside 0..SPH_MAX_BODIES-1 are SPH_ERR_INVALID too. sph_body_define_region
 * takes every boundary particle whose float position lies in the half-open box, by the compare of sph_remove_region with typeMask
 * fixed to type 3 (+-infinity allowed, NULL = everywhere, a NaN bound is SPH_ERR_INVALID); the members come in ascending original
 * id and *count receives their number. An empty result is SPH_ERR_INVALID (*count = 0) and leaves the slot as it was. Defining a
 * slot that is in use replaces its body once the new definition has succeeded. sph_body_release frees a slot (a free slot:
 * a no-op); sph_body_count gives the member count, 0 for a free slot; sph_body_read copies out the ids and the reference rows in
 * member order (any pointer may be NULL; a free slot writes nothing). Bodies may overlap: poses apply in call order and the last
 * one wins.
 * POSE. pose = 12 floats, row-major 3 x 4, (R | t): R00 R01 R02 tx, R10 R11 R12 ty, R20 R21 R22 tz. For member k with reference
 * position p and reference normal n, every operation one float operation in exactly this order, no contraction:
 *     x' = ((R00*p.x + R01*p.y) + R02*p.z) + tx        nx' = (R00*n.x + R01*n.y) + R02*n.z
 *     y' = ((R10*p.x + R11*p.y) + R12*p.z) + ty        ny' = (R10*n.x + R11*n.y) + R12*n.z
 *     z' = ((R20*p.x + R21*p.y) + R22*p.z) + tz        nz' = (R20*n.x + R21*n.y) + R22*n.z
 * and p.w and n.w copied bit for bit. position[id_k] = (x', y', z', p.w), velocity[id_k] = (nx', ny', nz', n.w). The linear part
 * is applied to the normal as given and the result is not renormalised: passing a rotation is the caller's business. The pose is
 * always applied to the REFERENCE placement, never to the current one: a body driven for 10^5 steps accumulates no rounding.
 * A pose word that is not finite is SPH_ERR_INVALID. Every new position gets the validation of sph_add_particles (finite; inside
 * the box with wide cell ids). The call is ALL OR NOTHING: if any member fails, nothing is written, *offenders receives their
 * number, *lowestMember the lowest failing member index k (not an id), and the call returns SPH_ERR_INVALID. On success
 * *offenders = 0, *lowestMember = -1 and *maxMoveInR0 = sqrtf(max_k d2_k) / r0 in float, with d = new - current position per
 * axis and d2 = (dx*dx + dy*dy) + dz*dz in float on the device, the maximum taken on the bit patterns of the non-negative floats
 * (order-independent). This is the caller's TUNNELLING NUMBER, the counterpart of sph_field_diffuse's stability number: a wall
 * that moves about r0 or more in one step passes through liquid instead of pushing it. No limit is enforced. The three outputs may
 * be NULL.
 * WHAT A POSE LEAVES ALONE. The particle set does not change, so the sorted state of the last completed step, which the analysis
 * calls read, stays valid (it is one step behind the current state anyway), and so do selections, meshes, labellings, renders, the
 * edit map, tracers and carried fields. The liquid signature of sph_slab_liquid_signature does not see boundary particles.
 * EDITS CARRY THE BODIES, like the fields. A successful removal maps every member id through the removal's old-to-new map
 * (sph_read_edit_map); removed members are dropped together with their reference rows, the others keep their order; a body left
 * without members is released. Additions, failed or counting edits, and a removal of nothing leave the bodies untouched.
 * Rules: on the solver's stream, not stages (no stage timing); each call waits for the results it returns. SPH_ERR_INVALID for a
 * slab solver and for null pointers where none is allowed. SPH_ERR_ORDER while a stage-by-stage step is half done (from the first
 * stage entry point of a step until its integrate stage, or with elastic matter its membranes-finalize stage, has run; sph_step is
 * never half done), and for sph_body_set_pose on a free slot. A failed call leaves the solver and the slot as they were. An
 * outstanding sph_read_position_async finishes its device copy before a pose moves anything. Device memory: 36 bytes per member,
 * once more for the largest body as staging, and 16 bytes per 64 particles while a definition is checked. */
#define SPH_MAX_BODIES 16
int sph_body_define_ids(sph_solver* s, int32_t slot, const uint32_t* origIds /* host */, int64_t count);
int sph_body_define_region(sph_solver* s, int32_t slot, const float* region6 /* host or NULL = everywhere */, int64_t* count);
int sph_body_release(sph_solver* s, int32_t slot);
int sph_body_count(sph_solver* s, int32_t slot, int64_t* count);
int sph_body_read(sph_solver* s, int32_t slot, uint32_t* origIds, float* refPosition4, float* refNormal4 /* host, count x 4 */);
int sph_body_set_pose(sph_solver* s, int32_t slot, const float pose[12], int64_t* offenders, int64_t* lowestMember,
                      float* maxMoveInR0);

/* ---- Wall loads: contact and force terms per kinematic body (no reference counterpart) --------------------------
 * What a set of boundary particles did to each non-boundary particle in the last completed step: the wall's main action, the
 * position shift and velocity reflection inside integrate (the reference's computeInteractionWithBoundaryParticles), and the K7 /
 * K12 terms of sph_force_measure, both attributed to the set.
 * STATE: the sorted state and neighbour rows of the last completed step, as sph_force_measure describes them, and that step's
 * buffer "acceleration", both halves (a0 = acceleration[i], a1 = acceleration[N + i]). The walls are where that step saw them:
 * a pose applied since does not change the answer. dt = timeStep, posTimeStep = timeStep * simulationScaleInv (float).
 * THE WALL SET S. slot 0..SPH_MAX_BODIES-1: the members of that body as it is defined now, by original id, mapped to sorted
 * indices through the step's particleIndex; SPH_WALL_ALL: every boundary particle; SPH_WALL_NO_BODY: the boundary particles that
 * are members of no body. The set of a free slot is SPH_ERR_ORDER.
 * CONTRACT, for a sorted particle i that is not a boundary particle; all arithmetic in float, one operation at a time in the
 * written order, no contraction, IEEE division and square root. x, v: sortedPosition[i], sortedVelocity[i].
 *   Before contact, exactly as integrate:
 *     a = a0 + a1 per component (xyz);  nv = v + dt*a (xyz), nv.w = v.w + dt*0.f;  x0 = x + posTimeStep*nv (xyz);
 *     x0 clamped to the box: x0.c < min_c -> min_c, then x0.c > max_c - 0.000001f -> max_c - 0.000001f;
 *     u0 = (v + nv) * 0.5f on all four lanes.
 *   Slot walk, k = 0..31 ascending, over the slots with j = row(i)[k] != -1 and (int)sortedPosition[j].w == 3; pb =
 *   sortedPosition[j], nb = sortedVelocity[j] (a boundary particle's velocity slot holds its wall normal); sums start at +0:
 *     dx = x0.x - pb.x, likewise dy, dz;  d = dx*dx; d += dy*dy; d += dz*dz; d = sqrtf(d);
 *     w = fmaxf(0, (r0 - d) / r0);  n += nb*w on four lanes;  wsum += w;  wsum2 += w * (r0 - d);
 *     when j is in S:  wS += w;  mS += 1;  cS += 1 when w > 0.
 *   Contact:
 *     len2 = ((n.x*n.x + n.y*n.y) + n.z*n.z) + n.w*n.w;  contact <=> len2 != 0;
 *     sh_c = ((n_c / sqrtf(len2)) * wsum2) / wsum for c = x, y, z (0 without contact);  x1 = x0 + sh;
 *     vn = (n.x*u0.x + n.y*u0.y) + n.z*u0.z;  reflected <=> contact && vn < 0;
 *     reflected: u1_c = (u0_c - n_c*vn) * 0.99f for xyz and u1.w = u0.w * 0.99f;  otherwise u1 = u0;
 *     DV = u1 - u0 per component;  share = contact ? wS / wsum : 0.
 *   Force-stage terms of S: the K7 and K12 terms of sph_force_measure's contract (tv, tt, tq with their use conditions), summed in
 *   slot order over the used slots whose neighbour is a boundary particle in S: V_S, T_S, P_S, scaled as there: V_S*sF, T_S,
 *   P_S*sP. The scales are applied whatever the sums hold: without a used slot in S the words are +0 * sF, +0 and +0 * sP (sP is
 *   negative: -0), as in sph_force_measure.
 * RECORD, SPH_WALL_WORDS floats per particle:
 *   0..2     sh * share                      3..5     DV * share (xyz)              6   share      7   wS      8   cS      9   mS
 *   10..18   V_S*sF (xyz), T_S (xyz), P_S*sP (xyz)
 *   19..21   the position exactly as integrate stores it: x1, and in a solver without elastic matter x1 + 0.f (integrate's fold
 *            of the membrane stages)
 *   22..25   u1, the velocity as integrate stores it
 *   26       contact (1 or 0)                27       reflected (1 or 0)             28..31   0
 * A boundary particle's record is all zero. Values are per unit mass: cfg.mass * DV / timeStep is the contact's force on the
 * particle, cfg.mass times words 10..18 the force-stage force.
 * TIES TO THE STEP. In a solver without elastic matter words 19..21 equal sph_read_position and words 22..25 sph_read_velocity
 * right after the step, at the particle's original id, for every non-boundary particle, bit for bit; with elastic matter they
 * equal the two at the integrate stage of a staged step, before the membrane stages rewrite positions. With slot = SPH_WALL_ALL
 * wS has the bits of wsum, so share is exactly 1 wherever there is contact, words 0..5 are sh and DV themselves, and words 10..18
 * equal words 18..26 of sph_force_measure.
 * sph_wall_measure: fromSelection as in sph_force_measure (0: all N sorted particles in sorted order; 1: the particles of the
 * current selection in its order, under sph_read_selection's SPH_ERR_ORDER rules).
 * sph_wall_diagnostics: selection, region rules, count limit and errors exactly as sph_force_diagnostics. Per-particle terms,
 * floats widened to double, an unselected particle contributing +0.0, summed by the fixed tree reduce(a) of sph_diagnostics over
 * all N terms in ascending sorted index. Record, SPH_WALL_DIAG_WORDS doubles per region:
 *   0        n selected         1   n with contact        2   n with share > 0        3   n reflected with share > 0
 *   4..6     sum words 0..2     7..9     sum words 3..5        10..18   sum words 10..18
 *   19..21   sum x_i x (words 3..5)          22..24   sum x_i x h_S,  h_S = (visc + pres) + tens of words 10..18 per component
 *   25       sum share          26       sum wS                27..31   0
 * Both cross products are a x b = (a.y*b.z - a.z*b.y, a.z*b.x - a.x*b.z, a.x*b.y - a.y*b.x) in float with x_i the SORTED position
 * (the state the step started from), as in sph_force_diagnostics.
 * SCOPE. The split of sh and DV by w / wsum is this library's attribution; the reference has none, because the direction of the
 * shift is shared by all walls in reach. The K12 term is not antisymmetric (see sph_force_measure). The load on the body is
 * approximately minus these sums, and no word claims more than that.
 * Rules: blocking, on the solver's stream, read-only on every solver array, not stages (no stage timing). SPH_ERR_ORDER until the
 * last step's integrate stage has run (in the staged path too; sph_step is never half done), after an edit, for a free slot, and
 * for fromSelection without a current selection. SPH_ERR_INVALID for a slab solver, a slot outside 0..SPH_MAX_BODIES-1 that is
 * neither SPH_WALL_ALL nor SPH_WALL_NO_BODY, null pointers, fromSelection outside 0..1, a typeMask of 0 or with bits outside 1..3,
 * count outside 1..SPH_DIAG_MAX_REGIONS, a NaN region bound. A blown-up state is reported as by every blocking call. Device
 * scratch, grown on demand and freed by sph_destroy: 1 bit per particle for the set, the sampling scratch (at most 64 MiB) and 256
 * bytes per region and 1024 particles for the totals. */
#define SPH_WALL_WORDS 32
#define SPH_WALL_DIAG_WORDS 32
#define SPH_WALL_ALL (-1)     /* the wall set = every boundary particle */
#define SPH_WALL_NO_BODY (-2) /* the wall set = boundary particles that are members of no body */
int sph_wall_measure(sph_solver* s, int32_t slot, int32_t fromSelection, float* out /* host, N (or the selection's count) x 32 */);
int sph_wall_diagnostics(sph_solver* s, int32_t slot, const float* regions6 /* host, count x (x0,y0,z0,x1,y1,z1) */, int32_t count,
                         uint32_t typeMask, double* out /* host, count x 32 */);

/* ---- Free bodies: rigid-body dynamics driven by the wall loads (no reference counterpart) ------------------------
 * A kinematic body gets a DYNAMIC STATE (sph_body_set_dynamics); after a completed step one call, sph_bodies_advance, computes
 * the load of that step on every dynamic body, advances its state by one step and places its members, all on the device. The step
 * kernels know nothing of it; every other call behaves as before.
 * UNITS. The state lives in the solver's own units: positions in position units, velocities as the particles' velocities. A
 * velocity moves a position by posTimeStep * V and an angular velocity turns by posTimeStep * omega (posTimeStep = the float
 * timeStep * simulationScaleInv of the step, widened); inertia is therefore in kg * (position unit)^2.
 * sph_body_set_dynamics checks the parameters (SPH_ERR_INVALID: mass not finite or <= 0; any non-finite word; inertiaInv with a
 * negative diagonal word, or a 2 x 2 principal minor or a determinant below zero by more than 1e-9 of the size of its terms; |q| outside [0.5, 2]; locks with bits above 3), normalises q
 * (n = sqrt(((w*w + x*x) + y*y) + z*z) in double, q / n) and stores the state on the device. The advance counter restarts at 0.
 * Two dynamic bodies must not share a member: the call counts, blocking, the members of the slot that are members of another
 * dynamic body, and refuses with SPH_ERR_INVALID naming their number and the lowest shared original id. dyn == NULL makes the
 * body kinematic again. sph_body_get_dynamics (blocking) returns the live state; *isDynamic = 0 and `out` untouched otherwise.
 * sph_bodies_advance. With out == NULL everything is enqueued on the solver's stream and the call returns without a host wait;
 * with `out` it waits once and copies SPH_MAX_BODIES records of SPH_BODY_STATE_WORDS doubles. For every dynamic body:
 *  1. LOAD. D[0..31] is the record sph_wall_diagnostics(slot, one region = everything, typeMask = types 1..3) returns on this
 *     state (the last completed step's, the walls where that step saw them). The words used below and words 1 and 2 are equal as
 *     IEEE values to that call's; the sign of a zero total is not part of the contract (chunks without a neighbour of the body
 *     contribute +0.0).
 *  2. INTEGRATE, all in double, one operation at a time in the written order, no contraction, IEEE / and sqrt. dt =
 *     (double)timeStep, hp = (double)posTimeStep, mp = (double)cfg.mass, c over x, y, z:
 *       C_c = D[7+c];  H_c = (D[10+c] + D[16+c]) + D[13+c];  TC_c = D[19+c];  TH_c = D[22+c]
 *       Fl_c = -(mp * (contactGain*(C_c/dt) + forceGain*H_c));  T0_c = -(mp * (contactGain*(TC_c/dt) + forceGain*TH_c))
 *       Tl = T0 - X x Fl, written T0.x - (X.y*Fl.z - X.z*Fl.y), T0.y - (X.z*Fl.x - X.x*Fl.z), T0.z - (X.x*Fl.y - X.y*Fl.x)
 *       F_c = (Fl_c + mass*gravity_c) + force_c;  V'_c = V_c on a locked axis, else V_c + dt*(F_c/mass);  X'_c = X_c + hp*V'_c
 *       rotation free:   L'_c = L_c + dt*(Tl_c + torque_c);  R = R(q);  u = R^T L';  w = Jinv u;  omega = R w, every matrix row
 *                        (a*b + c*d) + e*f  (u_x = (R00*L'x + R10*L'y) + R20*L'z; w_x = (Jxx*u_x + Jxy*u_y) + Jxz*u_z)
 *       rotation locked: L' = L, omega = spin
 *       dw = -((ox*x + oy*y) + oz*z);  dx = (ox*w + oy*z) - oz*y;  dy = (oy*w + oz*x) - ox*z;  dz = (oz*w + ox*y) - oy*x
 *       q* = q + (0.5*hp)*d;  n = sqrt(((w*w + x*x) + y*y) + z*z) of q*;  q' = q* / n
 *       R00 = 1 - 2*(y*y + z*z)   R01 = 2*(x*y - w*z)       R02 = 2*(x*z + w*y)
 *       R10 = 2*(x*y + w*z)       R11 = 1 - 2*(x*x + z*z)   R12 = 2*(y*z - w*x)
 *       R20 = 2*(x*z - w*y)       R21 = 2*(y*z + w*x)       R22 = 1 - 2*(x*x + y*y)
 *  3. PLACE. R' = R(q'), t_c = X'_c - ((R'c0*com.x + R'c1*com.y) + R'c2*com.z); the twelve numbers narrowed to float once are the
 *     pose, applied with the expressions, the validation, the all-or-nothing rule and the tunnelling number of sph_body_set_pose.
 *     If a member fails, nothing of that body is written, its dynamic state stays as it was and its status is 1; a non-finite
 *     word in X', q', V', L' or the pose gives status 2 with the same consequences. Other bodies are not affected and the call
 *     is SPH_OK.
 * RECORD per slot, doubles:  0 status (-1 not dynamic, 0 advanced, 1 pose refused, 2 non-finite)   1 member count
 *   2 advances since sph_body_set_dynamics (this one included when status is 0)   3 tunnelling number (status 0)
 *   4..6 X'   7..10 q'   11..13 V'   14..16 L'   17..19 omega   20..22 Fl   23..25 Tl   (the computed values, whatever the status)
 *   26 n with contact (D[1])   27 n with share > 0 (D[2])   28 offenders   29 lowest failing member (status 1)   30..47 0
 * RULES. SPH_OK with nothing to do when no body is dynamic. SPH_ERR_ORDER under exactly the conditions of sph_wall_diagnostics
 * (no completed step, a half-done staged step, after an edit); sph_body_set_dynamics on a free slot is SPH_ERR_ORDER too.
 * SPH_ERR_INVALID for a slab solver and a slot out of range. Defining or releasing a slot clears its dynamics; a removal carries
 * them along unchanged (the mass properties are the caller's) unless it empties the body. sph_body_set_pose on a dynamic body
 * stays legal and moves the particles only: the next advance places them from the dynamic state again. An advance leaves analysis
 * state valid, like a pose.
 * SCOPE. The coupling is explicit and one step behind. The load inherits the caveats of the wall loads above. A body much lighter
 * than the liquid it displaces will be unstable; no limit is enforced, the tunnelling number is what the caller watches. No
 * body-body contact, no no-slip walls. Device memory, grown on demand: one byte per particle and 2.6 KB per 1024 particles (152 bytes for each of the 16 slots and
 * for the contact count), plus 17 KB of states and records. */
typedef struct sph_body_dynamics {
  double mass;          /* kg, finite, > 0 */
  double com[3];        /* centre of mass in the REFERENCE placement, position units */
  double inertiaInv[6]; /* inverse inertia about com in reference axes: xx yy zz xy xz yz, 1/(kg * position unit^2);
                           finite, symmetric positive semi-definite (all zero: never turns) */
  double position[3];   /* X: current centre of mass, position units */
  double orientation[4];/* q = (w, x, y, z), maps reference axes to world; normalised by the call, |q| in [0.5, 2] else INVALID */
  double velocity[3];   /* V, the particles' velocity units */
  double angularMomentum[3]; /* L about the centre of mass, world axes, kg * position unit * velocity unit */
  double spin[3];       /* the angular velocity used while rotation is locked */
  double gravity[3];    /* acceleration on the body (the wrappers default it to cfg.gravity_*) */
  double force[3], torque[3]; /* constant external force and torque about the centre of mass */
  double contactGain, forceGain; /* weights of the two load terms; 1, 1 by default */
  uint32_t locks;       /* bits 0..2: V.x / V.y / V.z keep their value (a driven axis); bit 3: rotation locked (omega = spin) */
} sph_body_dynamics;
#define SPH_BODY_STATE_WORDS 48
int sph_body_set_dynamics(sph_solver* s, int32_t slot, const sph_body_dynamics* dyn /* NULL: the body is kinematic again */);
int sph_body_get_dynamics(sph_solver* s, int32_t slot, sph_body_dynamics* out, int32_t* isDynamic); /* blocking */
int sph_bodies_advance(sph_solver* s, double* out /* host, SPH_MAX_BODIES x SPH_BODY_STATE_WORDS, or NULL */);

/* ---- Flow gauges: particle crossings of oriented gates (no reference counterpart) -------------------------------
 * A gauge counts the particles that went through an oriented parallelogram (or plane) in the last completed step, and sums what
 * they carried. Up to SPH_MAX_GAUGES gauges per solver, all served by one pass over the particles. No step kernel knows of them;
 * every call below is read-only on every solver array and leaves mesh, labelling, selection, render, edit map, fields, tracers and
 * body state valid.
 * THE GAUGE is the set origin + alpha*u + beta*v with 0 <= alpha < 1 and 0 <= beta < 1: half-open, so gauges that tile a section
 * count a particle once. With SPH_GAUGE_PLANE in flags it is the whole plane through origin spanned by u and v. The positive
 * direction is n = u x v. sph_gauge_define derives, in double from the floats, one operation at a time, no contraction:
 *     n = u x v, written n.x = u.y*v.z - u.z*v.y, n.y = u.z*v.x - u.x*v.z, n.z = u.x*v.y - u.y*v.x
 *     nn = (n.x*n.x + n.y*n.y) + n.z*n.z        A = (v x n) / nn        B = (n x u) / nn      (the cross products written as n is)
 * so that A.u = 1, A.v = 0, B.v = 1, B.u = 0 up to rounding. It is SPH_ERR_INVALID for a word of origin, u or v that is not finite,
 * for nn == 0 or not finite, for a typeMask of 0 or with a bit outside 1..2, for a fieldSlot that is neither -1 nor an existing
 * slot of the carried fields, for flags other than 0 and SPH_GAUGE_PLANE, for a slot outside 0..SPH_MAX_GAUGES-1 and for a slab
 * solver; the slot then keeps what it held. g == NULL releases the slot. Boundary particles are never counted: a pose or
 * sph_bodies_advance rewrites their current position after the step. sph_gauge_get returns the definition (*defined = 0 and `out`
 * untouched for a free slot). Definitions live on the host; a definition, a redefinition and a release clear the slot's totals.
 * THE STATE is that of a completed step: a_i = sortedPosition[i], where sorted particle i was when the step began, and with
 * id = particleIndex[i] its original id, b_i = position[id] and w_i = velocity[id], where the step's integration (with elastic
 * matter, the membranes' finalize pass) left it, and c_i = field[id] of the gauge's carried field (+0.0 with fieldSlot -1), all
 * widened to double. Sorted particle i is CONSIDERED by a gauge when (int)a_i.w is 1 or 2 with that bit in typeMask.
 *     s(p) = (n.x*(p.x - o.x) + n.y*(p.y - o.y)) + n.z*(p.z - o.z)
 *     a positive crossing: s(a) < 0 && s(b) >= 0        a negative crossing: s(a) >= 0 && s(b) < 0       (a NaN crosses nothing)
 *     t = s(a) / (s(a) - s(b));   x = a + t*(b - a) per component;
 *     alpha = (A.x*(x.x - o.x) + A.y*(x.y - o.y)) + A.z*(x.z - o.z),  beta likewise with B
 * The crossing is COUNTED if the gauge is a plane or 0 <= alpha && alpha < 1 && 0 <= beta && beta < 1. All in double, one
 * operation at a time in the written order, no contraction, IEEE division. A particle on the plane counts as on its non-negative
 * side, so the net count of a plane over K steps equals, exactly, the change of the number of considered particles with s >= 0.
 * RECORD, SPH_GAUGE_WORDS doubles per gauge and call. A counted crossing contributes the terms
 *     1, w.x, w.y, w.z, (w.x*w.x + w.y*w.y) + w.z*w.z, c, alpha, beta
 * to words 0..7 if it is positive and to words 8..15 if it is negative; every other particle contributes +0.0. Each of the 16
 * words is reduce() of sph_diagnostics over all N terms in ascending sorted index. The sign of a zero total is not part of the
 * contract. The record of a free slot is all +0.0. No floating-point atomics anywhere.
 * sph_gauges_accumulate computes the record of every defined gauge, adds it to the gauge's totals on the device and appends it to
 * the history. With out == NULL everything is enqueued on the solver's stream and the call returns without a host wait; with
 * `out` it waits once and copies SPH_MAX_GAUGES records. Every successful call has an INDEX, counted from 0 per solver and never
 * reset. Calling it twice after one step counts that step twice; that is not detected.
 * TOTALS, SPH_GAUGE_TOTAL_WORDS doubles per gauge, on the device:  0..15 total = total + record, once per call
 *   16 calls accumulated since the slot's totals were cleared     17 index of the first call with a positive crossing, -1 if none
 *   18 index of the first call with a negative crossing, -1 if none      19 index of the last call with any crossing, -1 if none
 * Totals survive steps, edits and pose changes. sph_gauges_reset (slot, or -1: all), a definition and a release clear a slot's
 * totals (words 0..16 to +0.0, 17..19 to -1). sph_gauges_read (blocking) copies the totals; *calls (may be NULL) receives the
 * number of calls so far, which is the index of the next one.
 * HISTORY. sph_gauges_history(rows) gives the solver a device ring of `rows` rows of SPH_MAX_GAUGES records (rows == 0 releases
 * it; rows outside 0..SPH_GAUGE_HISTORY_MAX is SPH_ERR_INVALID; a new ring starts empty). Every accumulate writes its row, index %
 * rows, without a host wait. sph_gauges_read_history (blocking) copies the records of calls firstCall .. firstCall + count - 1,
 * count x SPH_MAX_GAUGES x SPH_GAUGE_WORDS doubles, and *callsWritten (may be NULL) the number of calls so far. It is
 * SPH_ERR_INVALID unless every asked call was made since the ring was set up and is among the last `rows`, and SPH_ERR_ORDER
 * without a ring.
 * CROSSING LIST. sph_gauge_crossings (blocking) finds the counted crossings of ONE gauge on the same state and writes their number
 * to *count; sph_read_gauge_crossings copies them out (any pointer may be NULL), in ascending sorted index: the sorted index, the
 * original id, the direction (+1, -1) and t, alpha, beta narrowed to float once. It touches neither totals nor history. The list
 * is a derived result: reading it is SPH_ERR_ORDER without one and after anything that changes the state (a stage, a step, an
 * edit). sph_remove_ids and sph_field_write can act on its ids.
 * ORDER. sph_gauges_accumulate and sph_gauge_crossings are SPH_ERR_ORDER unless the integrate stage of the last step has run,
 * while a stage-by-stage step is half done (with elastic matter the positions are final only after the membranes' finalize stage),
 * after an edit until the next step (removed and added particles are not crossings), with no gauge defined (the crossing list:
 * with `slot` free), and when a gauge's carried field has been released. SPH_ERR_INVALID for a slab solver, a slot out of range
 * and null pointers where none is allowed.
 * SCOPE. Flat gauges only. A particle that crosses and returns within one step is not seen. The path between a and b is taken as
 * straight. Device memory, grown on demand: 2 bytes per particle for the tree, 5 KB of totals and records, 2 KB per history row,
 * and for the crossing list the scan's scratch plus 24 bytes per crossing. */
#define SPH_MAX_GAUGES 16
#define SPH_GAUGE_WORDS 16
#define SPH_GAUGE_TOTAL_WORDS 20
#define SPH_GAUGE_HISTORY_MAX 16384
#define SPH_GAUGE_PLANE 1u
typedef struct sph_gauge {
  float origin[3], u[3], v[3];
  uint32_t typeMask; /* bits 1..2: liquid, elastic */
  int32_t fieldSlot; /* a carried field, or -1 */
  uint32_t flags;    /* 0 or SPH_GAUGE_PLANE */
} sph_gauge;
int sph_gauge_define(sph_solver* s, int32_t slot, const sph_gauge* g /* NULL releases the slot */);
int sph_gauge_get(sph_solver* s, int32_t slot, sph_gauge* out, int32_t* defined);
int sph_gauges_accumulate(sph_solver* s, double* out /* host, SPH_MAX_GAUGES x SPH_GAUGE_WORDS, or NULL: no host wait */);
int sph_gauges_read(sph_solver* s, double* totals /* host, SPH_MAX_GAUGES x SPH_GAUGE_TOTAL_WORDS */, int64_t* calls); /* blocking */
int sph_gauges_reset(sph_solver* s, int32_t slot /* -1: all */);
int sph_gauges_history(sph_solver* s, int32_t rows /* 0 releases; at most SPH_GAUGE_HISTORY_MAX */);
int sph_gauges_read_history(sph_solver* s, int64_t firstCall, int32_t count, double* out, int64_t* callsWritten); /* blocking */
int sph_gauge_crossings(sph_solver* s, int32_t slot, int64_t* count); /* blocking */
int sph_read_gauge_crossings(sph_solver* s, int32_t* sortedIndex, uint32_t* origId, int32_t* direction, float* tab3 /* t, alpha, beta */);

/* ---- Probes: point samples and water levels on lines, with history (no reference counterpart) --------------------
 * The instruments of a run: a field at a fixed point over time, and the level of a surface along a fixed line over time. The
 * definitions are kept by the solver, one call after a step enqueues every record, and a history ring lives on the device; nothing
 * waits for the host unless asked. State, selected set, order of the sums, denormals and the all-zero record of a non-finite point
 * are those of sph_sample_points: the sorted state of the last completed step. Every call is read-only on every solver array and
 * is not a stage. Probes belong to the solver, as tracers do: steps, stages and edits leave them alone. A slab solver is
 * SPH_ERR_INVALID for every call.
 * POINT PROBE. Its record is the SPH_SAMPLE_WORDS record sph_sample_points returns at that point with the set's typeMask, bit for
 * bit.
 * LEVEL PROBE, a line of `count` points: q_k = origin + (float)k * step per component (one float multiply, one float add: the
 * lattice expression of sph_sample_grid), k = 0 .. count-1. f_k is word `field` (0..5, as sph_extract_surface) of the sample record
 * at q_k with the line's typeMask. Point k is INSIDE when f_k >= iso (float compare; NaN is outside). The line is searched from its
 * far end, k = count-1. Record (SPH_PROBE_LEVEL_WORDS floats):
 *   SPH_PROBE_SUBMERGED  point count-1 is inside:           { q_{count-1}.xyz, (float)(count-1), 2, (float)(count-1), f_{count-1}, 0 }
 *   SPH_PROBE_FOUND      K = the largest k with k inside and k+1 outside:
 *                                                           { x, y, z, (float)K + t, 0, (float)K, f_K, f_{K+1} }
 *                        t = (iso - f_K)/(f_{K+1} - f_K), x = q_K.x + t*(q_{K+1}.x - q_K.x), likewise y and z
 *   SPH_PROBE_DRY        there is no such k:                { q_0.xyz, 0, 1, -1, 0, 0 }
 * all in float, in the written order, no contraction, IEEE division: the vertex expression of sph_extract_surface. t may be 0; a NaN
 * f_{K+1} gives NaN coordinates. To find a lower face or the bed, orient the line the other way. A line's record depends on the
 * state and the line alone: not on the other lines, their order or number, nor on how far the search went.
 * DEFINITIONS. sph_probes_set_points replaces the point set (at most SPH_PROBE_MAX_POINTS; points may be non-finite, as for
 * sampling), sph_probes_set_lines the lines (at most SPH_PROBE_MAX_LINES); count == 0 releases the set. Both validate all or
 * nothing: on SPH_ERR_INVALID the set keeps what it held. Invalid: a count above the maximum or below 0, a bad typeMask (as
 * sampling; per line for lines), a non-finite word of a line's origin or step, a non-finite iso, a line's count outside
 * 2..SPH_PROBE_LINE_MAX, a field outside 0..5, null pointers with count > 0, and a set whose row no longer fits the existing
 * ring's byte cap. Both set calls copy the caller's array before they return (blocking). sph_probes_count gives {points, lines}.
 * RECORDING. sph_probes_record computes every point and line record, writes them to row index % rows of the ring if there is one,
 * and increments the call INDEX, counted from 0 per solver and never reset. With both pointers NULL everything is enqueued on the
 * solver's stream and the call returns without a host wait; otherwise it waits once and copies what was asked for (points: P x 8
 * floats, levels: L x 8 floats). It is SPH_ERR_ORDER with neither points nor lines set; in every other state it returns exactly
 * what sph_sample_points returns there. A failed call consumes no index.
 * HISTORY. sph_probes_history(rows) gives the solver a device ring of `rows` rows of P + L records, points first (rows == 0
 * releases it; SPH_ERR_INVALID for rows outside 0..SPH_PROBE_HISTORY_MAX and for rows * row bytes > 1 << 28). A new ring and a new
 * set both restart the ring empty. sph_probes_read_history (blocking) copies the records of calls firstCall .. firstCall + count - 1
 * (points: count x P x 8, levels: count x L x 8; either may be NULL) and *callsWritten (may be NULL) the number of calls so far. It
 * is SPH_ERR_ORDER without a ring and SPH_ERR_INVALID unless every asked call was made since the ring (re)started and is among the
 * last `rows` calls.
 * SCOPE. Straight, fixed lines; the first crossing from the far end only (counting all crossings would forbid the early stop). */
#define SPH_PROBE_MAX_POINTS 65536
#define SPH_PROBE_MAX_LINES 65536
#define SPH_PROBE_LINE_MAX 1024      /* points of one line */
#define SPH_PROBE_LEVEL_WORDS 8
#define SPH_PROBE_HISTORY_MAX 16384  /* rows; and rows * row bytes <= 1 << 28 */
#define SPH_PROBE_FOUND 0
#define SPH_PROBE_DRY 1
#define SPH_PROBE_SUBMERGED 2
typedef struct sph_probe_line {      /* 40 bytes */
  float origin[3], step[3];
  int32_t count;      /* 2..SPH_PROBE_LINE_MAX */
  int32_t field;      /* 0..5, as sph_extract_surface */
  float iso;
  uint32_t typeMask;  /* as sampling, per line */
} sph_probe_line;
int sph_probes_set_points(sph_solver* s, const float* points4 /* host, count x (x,y,z,unused) */, int32_t count, uint32_t typeMask); /* 0 releases */
int sph_probes_set_lines(sph_solver* s, const sph_probe_line* lines /* host */, int32_t count); /* 0 releases */
int sph_probes_count(sph_solver* s, int32_t counts[2] /* out: points, lines */);
int sph_probes_record(sph_solver* s, float* points /* host, P x 8, or NULL */, float* levels /* host, L x 8, or NULL */);
int sph_probes_history(sph_solver* s, int32_t rows /* 0 releases; at most SPH_PROBE_HISTORY_MAX */);
int sph_probes_read_history(sph_solver* s, int64_t firstCall, int32_t count, float* points, float* levels, int64_t* callsWritten); /* blocking */

/* ---- Time statistics on a lattice: means, covariances, extremes (no reference counterpart) ------------------------
 * What a flow is reported by: at every node of a fixed lattice, the sums over time of the sampled field, the fraction of time the
 * node is wet, the call at which matter first arrived, the peak pressure and the call it occurred at. The solver keeps up to
 * SPH_MAX_STATS lattices (slots); one call after a step folds every node's record into accumulators that stay on the device; no
 * record is written and nothing waits for the host until the accumulators are read.
 * RECORD. Everything is a function of the SPH_SAMPLE_WORDS record r that sph_sample_grid(origin, spacing, dims, typeMask) would
 * return at the node, bit for bit. State, selected set, order of the sums, denormals and the all-zero record of a non-finite point
 * are those of sph_sample_points: the sorted state of the last completed step. A lattice point may overflow to a non-finite value:
 * it gives the all-zero record and is simply dry. Every call is read-only on every solver array and is not a stage. Statistics belong
 * to the solver, as probes do: steps, stages, edits and poses leave the numbers alone, and the lattice is fixed in space.
 * SLOTS. sph_stats_define gives slot 0..SPH_MAX_STATS-1 the lattice *g and SPH_STATS_WORDS doubles per node, node-major, x fastest
 * (node = (k * dims[1] + j) * dims[0] + i, as the records of sph_sample_grid), all empty, with calls = 0; g == NULL releases the
 * slot. SPH_ERR_INVALID, with the slot's old definition and numbers untouched: a slot outside the range, a non-finite word of
 * origin or spacing, any dims <= 0, a typeMask of 0 or with bits outside 1..3, accumulators above SPH_STATS_BYTES_MAX bytes
 * (nodes * SPH_STATS_WORDS * 8), a slab solver (every call). sph_stats_get reports a slot: *defined (0 or 1), *out (left alone when
 * not defined) and *calls; any out pointer may be NULL.
 * THE FOLD of record r at the slot's call index c (0-based, counted per slot). D(x) = (double)x; rho, vx, vy, vz, p, n are words
 * 0, 2, 3, 4, 5, 6 of r. If n > 0 (the node is WET in this call), with A the node's words:
 *   0       A0 += 1                                      wet calls
 *   1, 2    if (A1 < 0) A1 = c;  A2 = c                  first and last wet call
 *   3, 4    A3 += D(rho);  A4 += D(rho)*D(rho)
 *   5..7    += D(vx), D(vy), D(vz)
 *   8..13   += D(a)*D(b) for ab = xx, yy, zz, xy, xz, yz
 *   14, 15  A14 += D(p);  A15 += D(p)*D(p)
 *   16, 17  if (D(rho) > A16) { A16 = D(rho); A17 = c; }
 *   18, 19  q = (D(vx)*D(vx) + D(vy)*D(vy)) + D(vz)*D(vz);  if (q > A18) { A18 = q; A19 = c; }
 *   20, 21  if (D(p) > A20) { A20 = D(p); A21 = c; }     peak pressure and its call
 *   22, 23  if (D(p) < A22) { A22 = D(p); A23 = c; }
 * A dry call leaves the node's words untouched (n == 0 implies rho == 0, so A3 / calls is still the mean density over all calls).
 * EMPTY: the sums and word 0 are +0; words 1, 2, 17, 19, 21, 23 are -1; words 16, 18, 20 are -inf; word 22 is +inf. The strict
 * compares keep the first call of a tie and ignore a NaN; the sums propagate it. Every product above is of two floats widened to
 * double and therefore exact: contraction cannot change a bit. One node, one lane: no atomics, a fixed order.
 * ACCUMULATING. sph_stats_accumulate(slot) folds the slot's lattice and increments its call count; slot -1 means every defined
 * slot, in ascending order. Everything is enqueued on the solver's stream; the call never waits for the host. It is SPH_ERR_ORDER
 * with nothing defined (the slot, or with -1 any slot) and SPH_ERR_INVALID for a slot outside -1..SPH_MAX_STATS-1; in every other
 * state it returns exactly what sph_sample_points returns there. A failed call changes no slot and consumes no index.
 * sph_stats_reset(slot; -1: every defined slot) makes numbers and calls empty again and keeps the definition; SPH_ERR_ORDER for
 * a slot that is not defined (with -1: never).
 * READING. sph_stats_read (blocking) copies the SPH_STATS_WORDS doubles of nodes firstNode .. firstNode + count - 1 and *calls (may
 * be NULL). SPH_ERR_INVALID unless 0 <= firstNode, 0 <= count and firstNode + count <= nodes, and for a null `out` with count > 0;
 * SPH_ERR_ORDER for a slot that is not defined. sph_stats_read_moments (blocking, the same window rule) computes
 * SPH_STATS_MOMENT_WORDS floats per node on the device, in double, one rounded operation at a time in the written order, each value
 * then cast to float; C = calls, n = A0:
 *   0       n/C                                          wet fraction
 *   1       A3/C                                         mean density over all calls
 *   2       A4/C - (A3/C)*(A3/C)
 *   3..5    m_a = A(5+a)/n                               mean velocity over the wet calls
 *   6..11   A(8+i)/n - m_a*m_b for ab = xx, yy, zz, xy, xz, yz      velocity covariances (Reynolds stresses / density)
 *   12      mp = A14/n
 *   13      A15/n - mp*mp
 *   14      A1                                           arrival call
 *   15      A20                                          peak pressure
 * With n == 0, words 3..13 and 15 are +0 and word 14 is -1. It is SPH_ERR_ORDER while calls == 0.
 * SCOPE. Unweighted calls; no gradient quantities; no history of the accumulators; no lattice that moves with a body. */
#define SPH_MAX_STATS 4
#define SPH_STATS_WORDS 24
#define SPH_STATS_MOMENT_WORDS 16
#define SPH_STATS_BYTES_MAX ((int64_t)1 << 31) /* accumulators of one slot */
typedef struct sph_stats_lattice { /* 40 bytes */
  float origin[3], spacing[3];
  int32_t dims[3];    /* nx, ny, nz */
  uint32_t typeMask;  /* as sampling */
} sph_stats_lattice;
int sph_stats_define(sph_solver* s, int32_t slot, const sph_stats_lattice* g /* NULL releases the slot */);
int sph_stats_get(sph_solver* s, int32_t slot, sph_stats_lattice* out, int32_t* defined, int64_t* calls);
int sph_stats_accumulate(sph_solver* s, int32_t slot /* -1: every defined slot */); /* no host wait */
int sph_stats_reset(sph_solver* s, int32_t slot /* -1: all */);
int sph_stats_read(sph_solver* s, int32_t slot, int64_t firstNode, int64_t count, double* out /* host, count x 24 */, int64_t* calls); /* blocking */
int sph_stats_read_moments(sph_solver* s, int32_t slot, int64_t firstNode, int64_t count, float* out /* host, count x 16 */, int64_t* calls); /* blocking */

/* ---- Binned diagnostics: the sph_diagnostics record of every bin of a lattice (no reference counterpart) ---------
 * Maps and profiles of particle SUMS (water depth over a plan view, u(z) across a channel, mass and momentum per block): a bin's
 * record is a share of the particles, unlike a node value of sph_sample_grid, the probes or the time statistics.
 * EDGES. Edge i of axis a is e_a(i) = origin[a] + (float)i * spacing[a]: one float multiply, one float add, no contraction (the
 * expression of sph_sample_grid). Bin (i, j, k), i < nx, j < ny, k < nz, is the box [e_x(i), e_x(i+1)) x [e_y(j), e_y(j+1)) x
 * [e_z(k), e_z(k+1)); its record is record b = (k * ny + j) * nx + i. Neighbouring bins share the same float edge, so every
 * particle lies in at most one bin and a particle exactly on an edge belongs to the upper bin; where the origin is so large
 * against the spacing that consecutive edges coincide, the bins between them are empty and no particle is lost. An axis with
 * dims[a] == 1 and spacing[a] == 0 is the whole axis (-inf, +inf).
 * RECORD. out[b] is, word for word as 64-bit patterns, the record sph_diagnostics returns for that one box with the same typeMask
 * in the same state: the 14 sums in the positional fixed tree over all N terms, the extremes, the (max v2, lowest index, original
 * id) triple and the empty-record rule. Hence a record depends on the state and its own box only (not on the rest of the lattice),
 * and the counts over all bins add up exactly to the count of sph_diagnostics over the lattice's outer box.
 * sph_bin_index returns the bin b of every sorted particle under the same rule, -1 for a particle that is unselected by type or
 * key or lies in no bin: the tiling itself.
 * Errors: as sph_diagnostics (SPH_ERR_ORDER before a step's density and pressure-force stages have run; SPH_ERR_INVALID for a
 * slab solver, a typeMask of 0 or with bits outside 1..3, null pointers; a blown-up state is reported as by every blocking call),
 * and SPH_ERR_INVALID for a non-finite origin or spacing, a negative spacing, a spacing of 0 on an axis with dims != 1, dims <= 0,
 * nx * ny * nz > SPH_BIN_MAX_BINS. Blocking, on the solver's stream, read-only on every solver array, not a stage.
 * Device scratch, grown on demand and freed by sph_destroy, for B bins, N particles and E (chunk of 1024 particles, bin) pairs
 * with at least one member (E <= N; for a spatially sorted state about the chunks times the bins a chunk touches):
 *   264 * B + 4 * N + 4 bytes of tables, and 212 * E bytes of partials (sph_bin_index: the tables only). */
typedef struct sph_bin_lattice { /* 40 bytes, laid out like sph_stats_lattice */
  float origin[3], spacing[3];
  int32_t dims[3];    /* nx, ny, nz */
  uint32_t typeMask;  /* as sph_diagnostics */
} sph_bin_lattice;
#define SPH_BIN_MAX_BINS (1 << 18)
int sph_bin_diagnostics(sph_solver* s, const sph_bin_lattice* g, double* out /* host, bins x SPH_DIAG_WORDS */);
int sph_bin_index(sph_solver* s, const sph_bin_lattice* g, int32_t* binOfSorted /* host, N, sorted order; -1 = in no bin */);

/* ---- Integral curves: streamlines and tracers (no reference counterpart) ---------------------------------------
 * Curves that follow the sampled velocity field. State, selected set, order of the sums, argument rules and errors are those of
 * sph_sample_points: the sorted state of the last completed step (one integration step behind sph_read_position), SPH_ERR_ORDER
 * before a step's density and pressure-force stages have run, SPH_ERR_INVALID for a slab solver and for a typeMask of 0 or with
 * bits outside 1..3. Read-only on every solver array; blocking, on the solver's stream; not stages (no stage timing).
 * velocity(p): S, Ux, Uy, Uz of the sampling contract at p (the same operations in the same order); hit = (S != 0) and
 * u = (Ux/S, Uy/S, Uz/S): the bits of words 2..4 of the sph_sample_points record at p. speed(u) = sqrtf(ux*ux + uy*uy + uz*uz),
 * the products summed left to right. All arithmetic in float in the written order, no contraction, IEEE division and square root.
 * THE STEP at a curve's vertex p_k (k counts from 0), with step (may be negative: upstream), minSpeed >= 0, mode and integrator
 * of sph_trace_params and an optional region (x0, y0, z0, x1, y1, z1):
 *   1. p_k not finite: vertex (p_k, 0) is written and the curve stops with SPH_TRACE_NONFINITE.
 *   2. u = velocity(p_k); vertex (p_k.x, p_k.y, p_k.z, s) is written, s = speed(u), or 0 without a hit.
 *   3. no hit: stop with SPH_TRACE_LEFT_MATTER.
 *   4. a region is given and x0 <= x && x <= x1 is false for some axis of p_k: stop with SPH_TRACE_LEFT_REGION.
 *   5. !(s > minSpeed): stop with SPH_TRACE_STAGNANT (a NaN speed stops here too).
 *   6. k == maxSteps: stop with SPH_TRACE_MAX_STEPS.
 *   7. c = step (SPH_TRACE_TIME) or step / s (SPH_TRACE_ARC).
 *      SPH_TRACE_EULER:    p_{k+1} = p_k + c*u, per component one multiply, then one add.
 *      SPH_TRACE_MIDPOINT: q = p_k + (0.5f*c)*u; u2 = velocity(q); if q is not finite, there is no hit at q or
 *                          !(speed(u2) > minSpeed), the curve stops with SPH_TRACE_NONFINITE, SPH_TRACE_LEFT_MATTER or
 *                          SPH_TRACE_STAGNANT (tested in that order) and no further vertex is written; otherwise
 *                          c2 = step or step / speed(u2), and p_{k+1} = p_k + c2*u2.
 * In SPH_TRACE_TIME mode `step` is in scene units per unit of velocity: a time dt in seconds is dt / simulationScale, the factor
 * the step's integration applies. In SPH_TRACE_ARC mode it is the chord length in scene units.
 * sph_trace_streamlines runs the step from every seed until the curve stops, in one launch per piece of seeds. vertices holds
 * count x (maxSteps + 1) x 4 floats, curve by curve; lengths[i] >= 1 is the number of vertices written for seed i, the slots
 * behind them are +0, and status[i] is the code the curve stopped with (never SPH_TRACE_MOVING). The results do not depend on
 * the order or the number of the seeds. count == 0 is a no-op. Seeds go through the sampling scratch in pieces.
 * TRACERS are points carried along with a run: a device buffer of the solver's own (16 + 8 bytes per tracer, freed by
 * sph_tracers_set with count 0 and by sph_destroy), not derived from the particle state: steps, stages and edits leave them alone.
 * sph_tracers_set replaces them by `count` points with status SPH_TRACE_MOVING and 0 steps; it is legal at any time, on any
 * solver. sph_tracers_advect applies the step (items 1-5 and 7; there is no maxSteps test, params->maxSteps is not read) once to
 * every tracer whose status is SPH_TRACE_MOVING: the tracer moves to p_{k+1} or stops where it is with the step's code, and its
 * step count grows by 1. A stopped tracer keeps its position and code. Several calls without a step in between integrate the
 * frozen field. counts = {tracers still moving, tracers stopped} after the call. sph_tracers_read copies them out (any pointer
 * may be NULL): pos4 = x, y, z and the speed at the tracer's last sample (item 2; 0 before the first), status, steps.
 * sph_tracers_advect and sph_tracers_read are SPH_ERR_ORDER while there are no tracers.
 * Errors beside those above: SPH_ERR_INVALID for null pointers (region6 may be NULL), count < 0, a step that is 0 or not finite,
 * a minSpeed that is negative or NaN, maxSteps outside 0..65535 (streamlines), a mode or integrator outside 0..1, a NaN region
 * bound. */
#define SPH_TRACE_TIME 0
#define SPH_TRACE_ARC 1
#define SPH_TRACE_EULER 0
#define SPH_TRACE_MIDPOINT 1
#define SPH_TRACE_MOVING 0
#define SPH_TRACE_MAX_STEPS 1
#define SPH_TRACE_LEFT_MATTER 2
#define SPH_TRACE_LEFT_REGION 3
#define SPH_TRACE_STAGNANT 4
#define SPH_TRACE_NONFINITE 5
#define SPH_TRACE_MAX_STEPS_LIMIT 65535
typedef struct sph_trace_params {
  float step;
  float minSpeed;
  int32_t maxSteps;
  int32_t mode;        /* SPH_TRACE_TIME or SPH_TRACE_ARC */
  int32_t integrator;  /* SPH_TRACE_EULER or SPH_TRACE_MIDPOINT */
} sph_trace_params;
int sph_trace_streamlines(sph_solver* s, const float* seeds4 /* host, count x (x,y,z,unused) */, int32_t count, uint32_t typeMask,
                          const sph_trace_params* params, const float* region6 /* or NULL */,
                          float* vertices /* host, count x (maxSteps+1) x 4 */, int32_t* lengths /* host, count */,
                          int32_t* status /* host, count */);
int sph_tracers_set(sph_solver* s, const float* points4 /* host, count x (x,y,z,unused) */, int32_t count); /* 0 releases them */
int sph_tracers_advect(sph_solver* s, uint32_t typeMask, const sph_trace_params* params, const float* region6 /* or NULL */,
                       int64_t counts[2] /* out: still moving, stopped */);
int sph_tracers_read(sph_solver* s, float* pos4 /* host, count x (x,y,z,speed) */, int32_t* status, int32_t* steps);

int sph_synchronize(sph_solver* s);

/* Per-stage device timing with hipEvents on the solver's stream (the reference prints per-stage wall time,
 * owPhysicsFluidSimulator.cpp:88-115). Stage ids = sph_stage. Times accumulate until reset. */
typedef enum sph_stage {
  SPH_ST_HASH = 0, SPH_ST_SORT, SPH_ST_SORT_POST, SPH_ST_INDEX, SPH_ST_FIND_NEIGHBORS, SPH_ST_DENSITY,
  SPH_ST_FORCES, SPH_ST_ELASTIC, SPH_ST_PREDICT_DENSITY, SPH_ST_PRESSURE_FORCE, SPH_ST_INTEGRATE, SPH_ST_MEMBRANES,
  SPH_ST_BANDS, /* the search bands of sph_step() (sph_set_search_bands), built between the cell table and the search */
  SPH_ST_COUNT
} sph_stage;
int sph_set_stage_timing(sph_solver* s, int enable);
/* n = SPH_ST_COUNT, or SPH_ST_BANDS for a caller that knows the stages in front of it only */
int sph_get_stage_times(sph_solver* s, double* ms_total, int64_t* launches, int n);
int sph_reset_stage_times(sph_solver* s);
/* Radix passes (8- or 9-bit digits) the sort of sph_step() takes for this solver: 24 algorithmic bytes per particle each. */
int sph_step_sort_passes(sph_solver* s);
/* sph_step() outside slab mode and with stage timing off can run the density pass and the forces kernel's record pack of one
 * range of sorted particles while findNeighbors works on the next range. chunks = 0 (the default): the solver
 * decides by its particle count; 1: never; 2 .. 16: that many ranges, whatever the particle count. Results do not depend on it:
 * every particle is computed from the same inputs by the same code whichever launch serves it. */
int sph_set_step_chunks(sph_solver* s, int32_t chunks);
/* Where that step runs in chunks it can also run the kernels behind the search chunk by chunk on the chunk stream, each stage one
 * chunk behind the stage before it: the forces kernel, then predicted density and pressure force of every
 * predict-correct iteration. depth = -1 (the default): the solver's built-in depth; 0: none (every kernel behind the search runs
 * once over all particles); 1 .. 6: that many stages, clamped to the 2 * maxIteration the step has and to 1 with elastic matter.
 * A check on the device decides every step whether the chunks are wide enough for it; if not, the same stages run over all
 * particles behind the search. Results do not depend on it. */
int sph_set_step_pipeline(sph_solver* s, int32_t depth);

/* The per-wave skipping of the predict-correct loop in sph_step(): a wave of 64 sorted particles leaves out the neighbour loop of
 * the pressure-force or predicted-density kernel where its terms cannot change a bit of the result. 0: the built-in policy (a
 * launch consults the per-wave bytes only where the launch before found nothing flagged); 1: always mark and consult; 2: off.
 * Results do not depend on it. */
int sph_set_wave_skip(sph_solver* s, int32_t mode);

/* The search bands of sph_step(): once per step, the sorted particles within the search radius of a y or z face of their cell are
 * compacted into one array per neighbour row of cells, and findNeighbors tests only those of the cells it visits across a face
 * or an edge. 0 (the default): automatic — used outside slab mode on every grid for which the bands are provably a superset of
 * the neighbours (a cell id mask that changes no id of the grid, at least 3 cells per axis, the 27 cell offsets distinct); 1: off. Results do not depend on
 * it. The flags, the arrays and their start tables of the last step that used them: sph_read_buffer "searchBandFlags",
 * "searchBands", "searchBandStart" (SPH_ERR_ORDER if the last step did not build them). */
int sph_set_search_bands(sph_solver* s, int32_t mode);

/* ---- Spatial decomposition (no reference counterpart: the reference is single-device) -----------------
 * The global box is cut into z-slabs of whole cell layers, one solver (one GPU, one process) per slab. A solver holds the
 * particles of its own layers [layerLo, layerHi) plus `ghostLayers` layers on each side and advances ALL of them with the
 * ordinary sph_step(); only the particles it owned when the set was last rebuilt are authoritative afterwards. Once per
 * step the authoritative particles near a cut are sent to the neighbouring solver (sph_slab_pack -> the caller's
 * RCCL send/recv -> sph_slab_rebuild), which replaces its whole ghost zone with them. ghostLayers = 4 cell layers (8h)
 * cover the 6 neighbour hops (6 x 31h/30) that one PCISPH step propagates information, so owned particles get bit-identical
 * results to a single-solver run; the local arrays are kept sorted by global id so that the within-cell order (ascending
 * orig id) is the global one. Requires cellIdMask = 0xffffffff.
 * Message = n records of 9 words: position (x,y,z,type), velocity (vx,vy,vz,w), global id (or 7 words, see
 * sph_slab_set_record_format). All pointers below are DEVICE pointers on the solver's device. */
typedef struct sph_slab {
  int32_t layerLo, layerHi;   /* owned cell layers along z: cz = (int)(z * hashGridCellSizeInv) */
  int32_t ghostLayers;        /* W */
  int32_t hasLower, hasUpper; /* a neighbouring slab exists below / above */
  int32_t globalIdBits;       /* bit length of the largest global id */
} sph_slab;
#define SPH_SLAB_RECORD_WORDS 9
#define SPH_SLAB_COMPACT_WORDS 7 /* x, y, z, vx, vy, vz, global id: see sph_slab_set_record_format */
int sph_slab_init(sph_solver* s, const sph_slab* slab, const uint32_t* globalIds /* host, particleCount entries */);
/* counts[0] = authoritative particles kept, counts[1] / counts[2] = records written to msgDown / msgUp (each has room for
 * `capRecords`), every list in ascending global-id order (order-preserving compaction of the sorted local set).
 * Blocking (the counts come back to the host). */
int sph_slab_pack(sph_solver* s, void* msgDown, void* msgUp, int32_t capRecords, int32_t counts[3]);
/* The same, for callers that ship a message as ONE transfer `[count word | payload | padding]` (sphmi/slab.py): frame buffers
 * have room for 1 + 9*capRecords words; word 0 receives the number of payload words (9 x records), written on the device, and
 * the payload starts at word 1 — the frame can be handed to RCCL as it is. */
int sph_slab_pack_framed(sph_solver* s, void* frameDown, void* frameUp, int32_t capRecords, int32_t counts[3]);
/* New local set = kept + nDown records received from below + nUp from above, sorted by global id (three-way merge: the
 * received messages must be in ascending global-id order, as sph_slab_pack writes them; a message that is not makes the
 * next sph_slab_pack fail with SPH_ERR_INVALID). */
int sph_slab_rebuild(sph_solver* s, const void* recvDown, int32_t nDown, const void* recvUp, int32_t nUp);
/* Overlapped variant of "sph_step, then sph_slab_pack_framed": sph_slab_step_begin enqueues the whole step with its last stage
 * (pressure force + integrate) running first on the owned layers next to the cuts, packs the two frames as soon as those are
 * integrated, and returns without waiting; sph_slab_step_messages blocks only until the frames are ready and gives the
 * record counts (down, up) — the caller can hand the frames to RCCL while the rest of the step is still running; the following
 * sph_slab_rebuild waits for the step and takes the kept count from it. capRecords overflow is reported by sph_slab_step_messages. */
int sph_slab_step_begin(sph_solver* s, int iterationCount, void* frameDown, void* frameUp, int32_t capRecords);
int sph_slab_step_messages(sph_solver* s, int32_t counts[2]);
/* The same rebuild with NO host round trip: frameDown / frameUp are complete received frames `[payload words | payload]` with room
 * for capXRecords records (NULL where there is no neighbour), the kept count is taken where the preceding pack left it on the
 * device. Everything is enqueued and the call returns; the new particle count reaches the host with sph_slab_rebuild_finish
 * (blocking; also done implicitly by the next call that needs it): counts = kept, records from below, from above, and
 * counts[3] = 1 if NOTHING was merged because a frame announced more records than its buffer holds — fetch the rest and call
 * sph_slab_rebuild with the complete messages. A total beyond the solver's capacity is SPH_ERR_SIZE. */
int sph_slab_rebuild_framed(sph_solver* s, const void* frameDown, int32_t capDownRecords, const void* frameUp, int32_t capUpRecords);
int sph_slab_rebuild_finish(sph_solver* s, int32_t counts[4]);
/* Boundary particles never move: every solver keeps the boundary particles of its ghost layers from sph_slab_init on, and no
 * message ever carries one. The other particles' records can drop two more words: *typeBits = the position.w bit pattern common
 * to all non-boundary particles this solver was created with, provided their velocity.w is +0 (neither value ever changes);
 * 0 = it holds none, 0xffffffff = not uniform. When EVERY rank reports the same pattern (or 0), all of them may call
 * sph_slab_set_record_format(s, SPH_SLAB_COMPACT_WORDS, pattern) before the first pack: records are then 7 words
 * (x, y, z, vx, vy, vz, global id), 28 instead of 36 bytes. Default: SPH_SLAB_RECORD_WORDS. */
int sph_slab_liquid_signature(sph_solver* s, uint32_t* typeBits);
int sph_slab_set_record_format(sph_solver* s, int32_t recordWords, uint32_t typeBits);
/* Make the solver's stream wait for a hipEvent_t recorded on another stream (e.g. behind the RCCL receive on the caller's
 * communication stream) — stream-to-stream, the host does not wait. */
int sph_stream_wait_event(sph_solver* s, void* hipEvent);
int sph_particle_count(sph_solver* s);
/* Blocking read of the local set in its current order: positions, velocities (4 floats each), global ids and the
 * ownership flag (1 = in the owned layers when the set was last rebuilt); arrays sized sph_particle_count(). */
int sph_slab_read(sph_solver* s, float* position4, float* velocity4, uint32_t* globalIds, uint32_t* owned);

const char* sph_last_error(void);
int sph_abi_version(void);
/* What the loaded binary was built as: "libsphmi gfx950 abi 2" for the product build; diagnostic (timing-only, INVALID results)
 * variants add the names of their switches, each containing "DIAG". */
const char* sph_build_info(void);

#ifdef __cplusplus
}
#endif
#endif /* SPHMI_H */

// sphmi_run — headless driver shaped like owPhysicsFluidSimulator (src/owPhysicsFluidSimulator.cpp:27-149): loads
// configuration/position.txt + velocity.txt style files (or generates a synthetic box), constructs the solver through
// the owOpenCLSolver-compatible facade, and issues the reference's stage sequence with its per-stage timing printout.
//
//   sphmi_run --position P.txt --velocity V.txt [--steps N] [--staged] [--out positions.bin] [--quiet] [--blocking-readback]
//   sphmi_run --box 50 50 50 --lattice 100 100 100 [--wide] ...
//   sphmi_run --worm [--muscles] ...      the generated worm scene of the reference's default start-up (owHelper.cpp:709)
//   ... --sample-grid NX NY NZ --sample-every K --sample-out DIR
//        after every K-th step, sample the fields of all particle types on an NX x NY x NZ lattice spanning the scene's box
//        ([xmin, xmax] x [ymin, ymax] x [zmin, zmax], spacing (max - min) / (N - 1) in float) and write DIR/fields_<steps done>.bin:
//        raw float32 records in sph_sample_grid's layout (NZ x NY x NX x 8, x fastest; sphmi.frames.read_fields)
//   ... --surface-grid NX NY NZ --surface-every K --surface-out DIR [--surface-iso X]
//        after every K-th step, extract the isosurface shepard = X (default 0.5) of the liquid and elastic particles on the same
//        box-spanning lattice (sph_extract_surface) and write DIR/surface_<steps done>.ply (binary little-endian PLY;
//        sphmi.frames.read_ply)
//   ... --sample-gradients      with --sample-grid: also write DIR/gradients_<steps done>.bin, sph_sample_gradient_grid's
//        32-word records on the same lattice (NZ x NY x NX x 32; sphmi.frames.read_gradients)
//   ... --surface-normals       with --surface-grid: the PLY files carry unit vertex normals (sph_surface_normals) as nx ny nz
//   ... --surface-shells        with --surface-grid: measure each extracted mesh on the device (sph_measure_surface) and write
//        DIR/shells_<steps done>.csv beside the PLY file: one row per shell with its ten exact int64 words and its bounding box
//        (sphmi.frames.read_shells / shell_summary)
//   ... --diagnostics-every K --diagnostics-out FILE.csv [--diagnostics-region X0 Y0 Z0 X1 Y1 Z1]...
//        after every K-th step, sph_diagnostics of the liquid and elastic particles over the whole scene (region 0) and up to 15
//        further regions ("inf" / "-inf" are accepted as bounds): one CSV row per report and region (step, region, the 32 record
//        words as %.17g; sphmi.frames.read_diagnostics_csv) and, unless --quiet, one summary line per report
//   ... --components-every K --components-out FILE.csv [--components-link R] [--components-types T...] [--components-top M]
//        after every K-th step, label the connected components (sph_label_components) of the particles of the given types
//        (1 liquid, 2 elastic, 3 boundary; default 1 2) with link radius R (scene units; default inf = every neighbour-row entry)
//        and write one CSV row per report and component for the M largest components (default 16, at most 16), ordered by
//        descending n, then ascending root: step, component id, root, n, bounding box (%.9g) and the 32 words of its
//        sph_component_diagnostics record (%.17g; sphmi.frames.read_components_csv); unless --quiet, one summary line per report
//   ... --select-every K --select-out DIR [--select-surface T] [--select-region X0 Y0 Z0 X1 Y1 Z1] [--select-types T...]
//       [--select-term FIELD LO HI]...
//        after every K-th step, select particles on the device (sph_select_particles) and write DIR/selection_<steps done>.bin:
//        the count as int64, then the sorted indices (int32), the original ids (uint32) and the 12-float records
//        (sphmi.frames.read_selection). Types default to 1 (liquid); FIELD is density, speed, pressure, neighbors, x, y, z,
//        surface or 0..7, "inf" / "-inf" are accepted as bounds, up to 4 terms; --select-surface T is the term surface T inf
//   ... --elastic-every K --elastic-out DIR
//        after every K-th step of a scene with elastic matter (--worm), sph_muscle_diagnostics into DIR/muscles_<steps done>.csv:
//        one row per group (0 = the connections of no muscle): group, n, signal, mean length, mean rest length, mean strain, min
//        and max strain as %.17g (sphmi.frames.read_muscles_csv); unless --quiet, one line per report with the total membrane area
//        (sph_membrane_measure) and the global min, mean and max strain over all connections
//   ... --forces-every K
//        after every K-th step, sph_force_diagnostics over the whole scene: one line per call with the load in newtons (cfg.mass
//        times the summed accelerations; viscous + pressure + tension). On --worm the liquid's load on the elastic matter (type 2)
//        with its torque about the origin and its power; otherwise the boundary's and the liquid's load on the liquid (type 1)
//   ... --render-every K --render-out DIR [--render-size W H] [--render-eye X Y Z] [--render-target X Y Z] [--render-up X Y Z]
//       [--render-ortho S | --render-focal F] [--render-radius R] [--render-colour type|density|field:N:LO:HI|label]
//       [--render-thickness] [--render-surface] [--render-membranes] [--render-types T...]
//        after every K-th step, draw the liquid and elastic particles on the device (sph_render_particles) and write
//        DIR/frame_<steps done>.ppm (binary P6; sphmi.frames.read_ppm), DIR/frame_<steps done>.depth.f32 (raw float32, H x W, +inf
//        where nothing was drawn) and, with --render-thickness, DIR/frame_<steps done>.thickness.u32. The camera is at --render-eye
//        looking at --render-target (defaults: the centre of the scene's box, seen from two box diagonals away towards
//        (0.6, 0.5, 1)) with --render-up (default 0 1 0), the frame computed in double and narrowed once (sphmi.frames.look_at);
//        --render-ortho S: orthographic, S pixels per scene unit; --render-focal F: perspective, focal length F pixels (default:
//        perspective with F = W); the principal point is the image centre, the sphere radius defaults to r0 / 2, N is a field
//        number 0..6 of sph_histogram; label colours need no other option (the components of the drawn types are labelled first)
//        --render-surface: in each frame, extract the isosurface of --surface-grid NX NY NZ (--surface-iso; no PLY file unless
//        --surface-every / --surface-out are given too) and draw it smooth-shaded (sph_render_mesh); --render-membranes: draw the
//        membrane triangles flat-shaded (--worm). Without --render-types T... the frame shows the triangles alone; with it the
//        particles of those types are drawn first and the triangles are composed over them by depth. One "_render_mesh:" line
//        per frame.
//   ... --capacity N --emit-lattice OX OY OZ NX NY NZ [--emit-spacing S] [--emit-velocity VX VY VZ] [--emit-every K] [--emit-until STEP]
//       --drain-region X0 Y0 Z0 X1 Y1 Z1 [--drain-types T...] [--drain-every K] [--drain-at STEP]
//        particles appear and disappear between steps (sph_emit_lattice / sph_remove_region). Edits happen BEFORE
//        step S (S = steps done so far). Emitter: an NX x NY x NZ lattice of liquid at (OX, OY, OZ), spacing S (scene units;
//        default 0.93 r0) with velocity VX VY VZ (default 0), before every step S with S % K == 0 (K default 1) and S < STEP
//        (default: every step of the run); the solver needs room: --capacity N (at least the largest count reached). Drain: the
//        particles of the given types (default 1; "inf" / "-inf" are accepted as bounds, --drain-region may be left out =
//        everywhere) are removed before every step S > 0 with S % K == 0 (--drain-every) and before step STEP (--drain-at); a
//        gate that opens at step 200 is `--drain-types 3 --drain-region ... --drain-at 200`. The drain runs before the emitter.
//        Each step with an edit prints `_edit: step S removed R added A particles N`. With these options the position read-back
//        is the blocking one, and --out holds the final count of particles.
//   ... --body-region X0 Y0 Z0 X1 Y1 Z1 [--body-velocity VX VY VZ] [--body-spin AX AY AZ CX CY CZ RATE] [--body-from STEP] [--body-until STEP]
//        a wall that moves (sph_body_*): the boundary particles inside the region at the start ("inf" / "-inf" are
//        accepted as bounds) are body 0, and their placement then is its reference placement. Before every step S with
//        from <= S < until (defaults 0 and the end of the run), with k = S - from + 1, the body is placed at the reference
//        placement turned by k * RATE radians about the line through (CX, CY, CZ) along (AX, AY, AZ) and then shifted by
//        k * (VX, VY, VZ) (scene units per step); the pose is computed in double and narrowed once. Each moved step prints
//        `_body: step S members M max_move X` (X: the largest displacement in units of r0, %.9g; from about 1 on the wall
//        tunnels through liquid). With these options the position read-back is the blocking one.
//   ... --body-region ... --body-free [--body-mass M] [--body-locks xyzr] [--body-gains C F]
//        the body is free (sph_body_set_dynamics / sph_bodies_advance): the liquid moves it. Its members are equal
//        point masses, M in total (default: members x cfg.mass); the centre of mass is their mean, summed in member order in
//        double; the inverse inertia is the inverse of the point masses' inertia tensor, or all zero (the body never turns) where
//        that tensor is singular (det <= 1e-12 x trace^3: a single row of particles, a single particle). --body-locks: the letters
//        of the locked velocity axes and r for a locked rotation; --body-gains: contactGain and forceGain (default 1 1); gravity
//        is the scene's. --body-velocity gives the initial velocity (scene units per step, divided by posTimeStep in double);
//        --body-spin, --body-from and --body-until do not apply. After every step one line per advance is printed (%.9e):
//        `_free: step S body 0 status T advances A max_move M  X x y z  V x y z  F x y z` (S steps done; F the load in newtons).
//   ... --wall-load-every K
//        after every K-th step, sph_wall_diagnostics over the liquid of the whole scene, one line per defined body B
//        (with no body defined: one line for all walls, `body all`):
//        `_wall: step S body B (members M): contact n C shared H reflected R  contact force X Y Z N  stage force X Y Z N  load on
//        body X Y Z N  torque on body X Y Z` -- the numbers of frames.wall_summary (%.9e): cfg.mass / timeStep times the summed
//        velocity change of the contact inside integrate, cfg.mass times the body's K7 / K12 terms, and minus their sum.
//   ... --gauge "OX OY OZ UX UY UZ VX VY VZ" [--gauge-plane] [--gauge-field SLOT] ... --gauge-every K
//        flow gauges (sph_gauge_* / sph_gauges_*): every --gauge (one argument of nine numbers, scene units) defines
//        the next slot as the parallelogram origin + alpha U + beta V over the liquid, positive along U x V; --gauge-plane behind it
//        makes it the whole plane, --gauge-field SLOT sums carried field SLOT (0 with --dye-region) over its crossings. After every
//        step the crossings are accumulated on the device without a wait; after every K-th step one line per gauge G is printed from
//        the totals: `_gauge: step S gauge G plus P minus M net N calls C first F last L  mean velocity plus X Y Z minus X Y Z
//        field plus A minus B` (counts %.0f; F: the first call, counted from 0, with a crossing in either direction, -1: none yet;
//        mean velocities and field sums %.9e, the velocity sums over the counts, 0 without a crossing)
//   ... --probe X Y Z ... --level-line OX OY OZ SX SY SZ N ... --level-grid OX OY OZ SX SY SZ NX NY NZ --probe-every K --probe-out FILE
//        probes (sph_probes_*): every --probe adds a point probe (the sample record over liquid and elastic matter),
//        every --level-line a level probe of N points OX.. + k * SX.. (the Shepard sum of the liquid against 0.5, searched from the
//        far end), --level-grid one such line per (x, y) column of the lattice, along +z, x fastest. After every K-th step all
//        records go to a history ring on the device without a wait; the ring is read ONCE, at the end, and written to FILE: the text
//        line `sphmi probes calls C points P lines L every K`, then C x (P + L) x 8 raw float32 words, a call's point records in
//        front of its line records (frames.read_probes). One line is printed: `_probes: calls C points P lines L`. The ring's limits
//        (SPH_PROBE_HISTORY_MAX calls, 2^28 bytes) bound steps / K.
//   ... --stats-grid OX OY OZ SX SY SZ NX NY NZ [--stats-types "T ..."] [--stats-from S] [--stats-every K] --stats-out FILE
//        time statistics (sph_stats_*) on the lattice OX.. + i * SX.., i < NX NY NZ, over the particle types T
//        (1 liquid, 2 elastic, 3 boundary; default: liquid). After step S + 1 (default S = 0: the first step) and every K-th step
//        behind it (default 1) the lattice is folded into accumulators on the device without a wait; they are read ONCE, at the
//        end, and written to FILE: the text line `sphmi stats calls C from S every K nx NX ny NY nz NZ`, the 40 bytes of the
//        sph_stats_lattice, then NX x NY x NZ x 24 raw float64 words, x fastest (frames.read_stats). One line is printed:
//        `_stats: calls C nodes N`.
//   ... --bin-grid OX OY OZ SX SY SZ NX NY NZ [--bin-types "T ..."] [--bin-every K] --bin-out FILE
//        binned diagnostics (sph_bin_diagnostics): the diagnostics record of every bin of the lattice whose edges are
//        OX.. + i * SX.., i <= NX NY NZ (N 1 with S 0: the whole axis), over the particle types T (default: liquid and elastic).
//        After every K-th step (default 1) the records are appended to the CSV FILE, one row per bin: `step,bin,` and the 32 words
//        as %.17g (frames.read_bins). One line is printed per call: `_bins: step S bins B n N`.
//   ... --dye-region X0 Y0 Z0 X1 Y1 Z1 [--dye-inflow V] [--dye-diffusivity D] [--dye-every K]
//        a dye carried by the liquid (sph_field_*): carried field 0 starts at 1 on the liquid inside the region
//        ("inf" / "-inf" are accepted as bounds) and at 0 elsewhere; the emitter's liquid carries V (default 0; --dye-inflow alone
//        dyes only what the emitter adds). After every step the dye diffuses among the liquid by one substep of sph_field_diffuse
//        with coefficient = D * timeStep (default D = 0: it is only carried), and after every K-th step one line is printed:
//        `dye step=S n=N sum=... mean=... var=... min=... max=... stability=...` (S steps done; the liquid of the whole scene;
//        %.17g; stability is sph_field_diffuse's number for that step's substep, <= 1: the dye keeps its bounds)
//   ... --streamlines NU NV --stream-every K --stream-out DIR [--stream-step S] [--stream-max-steps M]
//        after every K-th step, streamlines of the liquid and elastic matter's velocity field (sph_trace_streamlines; DESIGN.md
//        §34; midpoint rule, chord length S in scene units, default h/2; at most M steps, default 256) from NU x NV seeds on the
//        plane across the box's mid-height (y = (ymin + ymax) / 2; seed (i, j) at x = xmin + (i + 0.5) (xmax - xmin) / NU,
//        z likewise with NV) into DIR/streamlines_<steps done>.vtk: legacy-VTK POLYDATA, one polyline per seed, the speed as point
//        data (sphmi.frames.read_polylines)
//   ... --tracers NU NV [--tracers-every K]
//        tracers carried with the run (sph_tracers_*): the same seed plane, set once; after every step they are advected through
//        that step's velocity field of the liquid by the scene's time step (midpoint rule), and after every K-th step (default 1)
//        one line is printed: `tracers step=S moving=M stopped=T`
//   --help   prints the usage line
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <string>
#include <vector>

#include "owHIPSolver.h"

typedef owHIPSolver owOpenCLSolver;  // the one line a reference maintainer changes

static double now_ms() {
  using namespace std::chrono;
  return duration<double, std::milli>(steady_clock::now().time_since_epoch()).count();
}

struct Watch {  // owHelper::refreshTime / watch_report (owHelper.cpp:44-57,1806-1841)
  double t0, t1; bool quiet;
  void refresh() { t0 = t1 = now_ms(); }
  void report(const char* fmt) { double t = now_ms(); if (!quiet) printf(fmt, t - t1); t1 = t; }
  double elapsed() const { return t1 - t0; }
};

// the table of sph_read_shells as text (sphmi.frames.write_shells_csv writes the same file)
static void write_shells_csv(const std::string& path, const std::vector<int64_t>& table, const std::vector<float>& boxes, const int32_t exps[3]) {
  FILE* f = fopen(path.c_str(), "w");
  if (!f) throw std::runtime_error("cannot write " + path);
  fprintf(f, "# exps %d %d %d\nshell,root,vertices,triangles,open,bad,a2,d6,mx,my,mz,min_x,min_y,min_z,max_x,max_y,max_z\n", exps[0], exps[1], exps[2]);
  for (size_t r = 0; r < table.size() / SPH_SHELL_WORDS; r++) {
    fprintf(f, "%zu", r);
    for (int w = 0; w < SPH_SHELL_WORDS; w++) fprintf(f, ",%lld", (long long)table[r * SPH_SHELL_WORDS + w]);
    for (int w = 0; w < 6; w++) fprintf(f, ",%.9g", (double)boxes[r * 6 + w]);
    fputc('\n', f);
  }
  if (fclose(f) != 0) throw std::runtime_error("cannot write " + path);
}

// binary little-endian PLY: float x y z (and nx ny nz when normals are given) per vertex, list uchar int vertex_indices per
// face (sphmi.frames.write_ply)
static void write_ply(const std::string& path, const std::vector<float>& verts, const std::vector<int32_t>& tris,
                      const std::vector<float>* normals = nullptr) {
  const size_t nv = verts.size() / 3, nt = tris.size() / 3;
  FILE* f = fopen(path.c_str(), "wb");
  if (!f) throw std::runtime_error("cannot write " + path);
  fprintf(f, "ply\nformat binary_little_endian 1.0\nelement vertex %zu\nproperty float x\nproperty float y\nproperty float z\n%s"
             "element face %zu\nproperty list uchar int vertex_indices\nend_header\n", nv,
          normals ? "property float nx\nproperty float ny\nproperty float nz\n" : "", nt);
  bool ok;
  if (normals) {
    std::vector<float> vn(nv * 6);
    for (size_t v = 0; v < nv; v++) {
      memcpy(&vn[v * 6], &verts[v * 3], 12);
      memcpy(&vn[v * 6 + 3], &(*normals)[v * 3], 12);
    }
    ok = fwrite(vn.data(), sizeof(float), vn.size(), f) == vn.size();
  } else {
    ok = fwrite(verts.data(), sizeof(float), verts.size(), f) == verts.size();
  }
  std::vector<unsigned char> faces(nt * 13);
  for (size_t t = 0; t < nt; t++) {
    faces[t * 13] = 3;
    memcpy(&faces[t * 13 + 1], &tris[t * 3], 12);  // little-endian host
  }
  ok = ok && fwrite(faces.data(), 1, faces.size(), f) == faces.size();
  if (fclose(f) != 0 || !ok) throw std::runtime_error("cannot write " + path);
}

// legacy-VTK POLYDATA, binary (big-endian): the vertices of every curve as POINTS, one LINES cell per curve, the vertices' fourth
// word as the point scalar "speed" (sphmi.frames.write_vtk_polylines)
static void write_vtk_polylines(const std::string& path, const std::vector<float>& vertices, const std::vector<int32_t>& lengths, int slots) {
  auto be = [](const void* word) { uint32_t v; memcpy(&v, word, 4); return __builtin_bswap32(v); };  // little-endian host
  size_t total = 0;
  for (int32_t n : lengths) total += (size_t)n;
  std::vector<uint32_t> points(3 * total), speed(total), cells(total + lengths.size());
  size_t at = 0, cell = 0;
  for (size_t c = 0; c < lengths.size(); c++) {
    const int32_t n = lengths[c];
    const uint32_t count = (uint32_t)n;
    cells[cell++] = be(&count);
    for (int32_t k = 0; k < n; k++, at++) {
      const float* v = &vertices[(c * (size_t)slots + (size_t)k) * 4];
      for (int a = 0; a < 3; a++) points[3 * at + a] = be(v + a);
      speed[at] = be(v + 3);
      const uint32_t id = (uint32_t)at;
      cells[cell++] = be(&id);
    }
  }
  FILE* f = fopen(path.c_str(), "wb");
  if (!f) throw std::runtime_error("cannot write " + path);
  fprintf(f, "# vtk DataFile Version 3.0\nsphmi streamlines\nBINARY\nDATASET POLYDATA\nPOINTS %zu float\n", total);
  bool ok = fwrite(points.data(), 4, points.size(), f) == points.size();
  fprintf(f, "\nLINES %zu %zu\n", lengths.size(), cells.size());
  ok = ok && fwrite(cells.data(), 4, cells.size(), f) == cells.size();
  fprintf(f, "\nPOINT_DATA %zu\nSCALARS speed float\nLOOKUP_TABLE default\n", total);
  ok = ok && fwrite(speed.data(), 4, speed.size(), f) == speed.size();
  fputc('\n', f);
  if (fclose(f) != 0 || !ok) throw std::runtime_error("cannot write " + path);
}

static int select_field(const char* name) {
  static const char* names[] = {"density", "speed", "pressure", "neighbors", "x", "y", "z", "surface"};
  for (int f = 0; f < 8; f++)
    if (!strcmp(name, names[f])) return f;
  if (name[0] >= '0' && name[0] <= '7' && !name[1]) return name[0] - '0';
  return -1;
}

// the camera frame of sphmi.frames.look_at: double arithmetic in this order, narrowed once; false when it is degenerate
static bool look_at(const double eye[3], const double target[3], const double up[3], sph_render_view* v) {
  double f[3] = {target[0] - eye[0], target[1] - eye[1], target[2] - eye[2]};
  double n = std::sqrt((f[0] * f[0] + f[1] * f[1]) + f[2] * f[2]);
  if (!(n > 0)) return false;
  for (int k = 0; k < 3; k++) f[k] /= n;
  double r[3] = {f[1] * up[2] - f[2] * up[1], f[2] * up[0] - f[0] * up[2], f[0] * up[1] - f[1] * up[0]};
  n = std::sqrt((r[0] * r[0] + r[1] * r[1]) + r[2] * r[2]);
  if (!(n > 1e-12)) return false;
  for (int k = 0; k < 3; k++) r[k] /= n;
  const double u[3] = {r[1] * f[2] - r[2] * f[1], r[2] * f[0] - r[0] * f[2], r[0] * f[1] - r[1] * f[0]};
  for (int k = 0; k < 3; k++) { v->eye[k] = (float)eye[k]; v->right[k] = (float)r[k]; v->up[k] = (float)u[k]; v->forward[k] = (float)f[k]; }
  return true;
}

static bool write_file(const std::string& path, const void* header, size_t headerBytes, const void* body, size_t bodyBytes) {
  FILE* f = fopen(path.c_str(), "wb");
  bool ok = f && fwrite(header, 1, headerBytes, f) == headerBytes && fwrite(body, 1, bodyBytes, f) == bodyBytes;
  if (f && fclose(f) != 0) ok = false;
  return ok;
}

// The pose (row-major 3 x 4, (R | t)) of the --body options after k moved steps: the reference placement turned by k * rate about
// the line through c along a (spin = ax ay az cx cy cz rate; Rodrigues' formula as sphmi.frames.pose_rotate writes it), then
// shifted by k * vel. Computed in double, narrowed once; without a spin the linear part is the exact identity.
static void body_pose(const double spin[7], const double vel[3], double k, float pose[12]) {
  double a[3] = {spin[0], spin[1], spin[2]};
  const double n = std::sqrt((a[0] * a[0] + a[1] * a[1]) + a[2] * a[2]);
  for (double& x : a) x /= n;
  const double angle = spin[6] * k, c = std::cos(angle), s = std::sin(angle);
  const double K[3][3] = {{0.0, -a[2], a[1]}, {a[2], 0.0, -a[0]}, {-a[1], a[0], 0.0}};
  for (int r = 0; r < 3; r++) {
    double row[3], t = spin[3 + r];
    for (int q = 0; q < 3; q++) {
      row[q] = (c * (r == q ? 1.0 : 0.0) + s * K[r][q]) + (1.0 - c) * (a[r] * a[q]);
      t -= row[q] * spin[3 + q];
    }
    for (int q = 0; q < 3; q++) pose[4 * r + q] = (float)row[q];
    pose[4 * r + 3] = (float)(t + vel[r] * k);
  }
}

// the 32 words of a diagnostics record as the CSV tables name them (frames.DIAG_FIELDS): --diagnostics-out and --bin-out
static const char kDiagCsvFields[] =
    "n,sum_x,sum_y,sum_z,sum_vx,sum_vy,sum_vz,sum_lx,sum_ly,sum_lz,sum_v2,sum_rho,sum_e2,sum_p,reserved14,reserved15,"
    "min_rho,max_rho,min_p,max_p,max_v2,max_v2_index,max_v2_id,min_x,min_y,min_z,max_x,max_y,max_z,reserved29,reserved30,"
    "reserved31\n";

int main(int argc, char** argv) {
  const char *posFile = nullptr, *velFile = nullptr, *outFile = nullptr;
  int steps = 10; bool staged = false, wide = false, quiet = false, muscles = false, worm = false, blockingRead = false;
  double box[3] = {0, 0, 0}; int lat[3] = {0, 0, 0};
  int sampleDims[3] = {0, 0, 0}, sampleEvery = 0; const char* sampleDir = nullptr;
  int surfDims[3] = {0, 0, 0}, surfEvery = 0; const char* surfDir = nullptr; float surfIso = 0.5f;
  bool sampleGradients = false, surfNormals = false, surfShells = false;
  int diagEvery = 0; bool diagEverySeen = false; const char* diagFile = nullptr;
  std::vector<float> diagRegions = {-INFINITY, -INFINITY, -INFINITY, INFINITY, INFINITY, INFINITY};  // region 0: everything
  int compEvery = 0, compTop = SPH_DIAG_MAX_REGIONS; bool compSeen = false, compTypesSeen = false; const char* compFile = nullptr;
  float compLink = INFINITY; unsigned compMask = 0;
  int selEvery = 0; bool selSeen = false, selTypesSeen = false, selRegionSeen = false; const char* selDir = nullptr;
  unsigned selMask = 0; float selRegion[6] = {-INFINITY, -INFINITY, -INFINITY, INFINITY, INFINITY, INFINITY};
  std::vector<sph_select_term> selTerms;
  int elaEvery = 0; bool elaSeen = false; const char* elaDir = nullptr;
  int forEvery = 0; bool forSeen = false;
  int wallEvery = 0; bool wallSeen = false;
  std::vector<sph_gauge> gaugeDefs; int gaugeEvery = 0; bool gaugeSeen = false, gaugeOk = true;
  std::vector<float> probePoints; std::vector<sph_probe_line> probeLines; int probeEvery = 0; bool probeSeen = false, probeOk = true;
  const char* probeFile = nullptr;
  sph_stats_lattice statsGrid = {}; int statsFrom = 0, statsEvery = 1, statsCalls = 0; bool statsSeen = false, statsGridSeen = false;
  const char* statsFile = nullptr;
  sph_bin_lattice binGrid = {}; int binEvery = 1; bool binSeen = false, binGridSeen = false; const char* binFile = nullptr;
  int renEvery = 0, renSize[2] = {640, 480}; bool renSeen = false, renEyeSeen = false, renTargetSeen = false, renThickness = false;
  const char* renDir = nullptr; const char* renColour = "density";
  double renEye[3] = {0, 0, 0}, renTarget[3] = {0, 0, 0}, renUp[3] = {0, 1, 0};
  float renOrtho = 0.f, renFocal = 0.f, renRadius = 0.f; bool renOrthoSeen = false, renFocalSeen = false, renRadiusSeen = false;
  bool renSurface = false, renMembranes = false, renTypesSeen = false; unsigned renTypes = 0;
  int capacity = 0; bool capSeen = false;
  bool emitSeen = false, emitLatSeen = false; float emitOrigin[3] = {0, 0, 0}, emitSpacing = 0.f, emitVel[3] = {0, 0, 0};
  int emitDims[3] = {0, 0, 0}, emitEvery = 1, emitUntil = -1;
  bool drainSeen = false, drainRegionSeen = false, drainTypesSeen = false; unsigned drainMask = 0; int drainEvery = 0, drainAt = -1;
  float drainRegion[6] = {-INFINITY, -INFINITY, -INFINITY, INFINITY, INFINITY, INFINITY};
  bool bodySeen = false, bodyRegionSeen = false, bodySpinSeen = false; float bodyRegion[6] = {0, 0, 0, 0, 0, 0};
  double bodyVel[3] = {0, 0, 0}, bodySpin[7] = {0, 0, 1, 0, 0, 0, 0}; int bodyFrom = 0, bodyUntil = -1;
  bool bodyFree = false; double bodyMass = 0, bodyGains[2] = {1, 1}; unsigned bodyLocks = 0; bool bodyLocksOk = true;
  bool dyeSeen = false, dyeRegionSeen = false, dyeEverySeen = false; float dyeRegion[6] = {0, 0, 0, 0, 0, 0}, dyeInflow = 0.f, dyeDiffusivity = 0.f; int dyeEvery = 0;
  int streamSeeds[2] = {0, 0}, streamEvery = 0, streamMaxSteps = 256; float streamStep = 0.f; bool streamSeen = false; const char* streamDir = nullptr;
  int tracerSeeds[2] = {0, 0}, tracersEvery = 1; bool tracersSeen = false;
  const char* usage = "usage: sphmi_run (--position P --velocity V | --box X Y Z --lattice A B C | --worm [--muscles]) [--steps N] [--staged] [--wide] [--out F]\n"
                      "       [--streamlines NU NV --stream-every K --stream-out DIR [--stream-step S] [--stream-max-steps M]] [--tracers NU NV [--tracers-every K]]\n"
                      "       (every option: the comment at the top of host/sphmi_run.cpp)\n";
  for (int i = 1; i < argc; i++) {
    if (!strcmp(argv[i], "--position") && i + 1 < argc) posFile = argv[++i];
    else if (!strcmp(argv[i], "--help")) { fputs(usage, stdout); return 0; }
    else if (!strcmp(argv[i], "--streamlines") && i + 2 < argc) { streamSeeds[0] = atoi(argv[++i]); streamSeeds[1] = atoi(argv[++i]); streamSeen = true; }
    else if (!strcmp(argv[i], "--stream-step") && i + 1 < argc) { streamStep = (float)atof(argv[++i]); streamSeen = true; }
    else if (!strcmp(argv[i], "--stream-max-steps") && i + 1 < argc) { streamMaxSteps = atoi(argv[++i]); streamSeen = true; }
    else if (!strcmp(argv[i], "--stream-every") && i + 1 < argc) { streamEvery = atoi(argv[++i]); streamSeen = true; }
    else if (!strcmp(argv[i], "--stream-out") && i + 1 < argc) { streamDir = argv[++i]; streamSeen = true; }
    else if (!strcmp(argv[i], "--tracers") && i + 2 < argc) { tracerSeeds[0] = atoi(argv[++i]); tracerSeeds[1] = atoi(argv[++i]); tracersSeen = true; }
    else if (!strcmp(argv[i], "--tracers-every") && i + 1 < argc) { tracersEvery = atoi(argv[++i]); tracersSeen = true; }
    else if (!strcmp(argv[i], "--capacity") && i + 1 < argc) { capacity = atoi(argv[++i]); capSeen = true; }
    else if (!strcmp(argv[i], "--emit-lattice") && i + 6 < argc) {
      for (int k = 0; k < 3; k++) emitOrigin[k] = (float)atof(argv[++i]);
      for (int k = 0; k < 3; k++) emitDims[k] = atoi(argv[++i]);
      emitSeen = emitLatSeen = true;
    }
    else if (!strcmp(argv[i], "--emit-spacing") && i + 1 < argc) { emitSpacing = (float)atof(argv[++i]); emitSeen = true; }
    else if (!strcmp(argv[i], "--emit-velocity") && i + 3 < argc) { for (int k = 0; k < 3; k++) emitVel[k] = (float)atof(argv[++i]); emitSeen = true; }
    else if (!strcmp(argv[i], "--emit-every") && i + 1 < argc) { emitEvery = atoi(argv[++i]); emitSeen = true; }
    else if (!strcmp(argv[i], "--emit-until") && i + 1 < argc) { emitUntil = atoi(argv[++i]); emitSeen = true; }
    else if (!strcmp(argv[i], "--drain-region") && i + 6 < argc) { for (int k = 0; k < 6; k++) drainRegion[k] = (float)atof(argv[++i]); drainSeen = drainRegionSeen = true; }
    else if (!strcmp(argv[i], "--body-region") && i + 6 < argc) { for (int k = 0; k < 6; k++) bodyRegion[k] = (float)atof(argv[++i]); bodySeen = bodyRegionSeen = true; }
    else if (!strcmp(argv[i], "--body-velocity") && i + 3 < argc) { for (int k = 0; k < 3; k++) bodyVel[k] = atof(argv[++i]); bodySeen = true; }
    else if (!strcmp(argv[i], "--body-spin") && i + 7 < argc) { for (int k = 0; k < 7; k++) bodySpin[k] = atof(argv[++i]); bodySeen = bodySpinSeen = true; }
    else if (!strcmp(argv[i], "--body-from") && i + 1 < argc) { bodyFrom = atoi(argv[++i]); bodySeen = true; }
    else if (!strcmp(argv[i], "--body-until") && i + 1 < argc) { bodyUntil = atoi(argv[++i]); bodySeen = true; }
    else if (!strcmp(argv[i], "--body-free")) { bodyFree = bodySeen = true; }
    else if (!strcmp(argv[i], "--body-mass") && i + 1 < argc) { bodyMass = atof(argv[++i]); bodySeen = true; if (!(bodyMass > 0) || !std::isfinite(bodyMass)) bodyLocksOk = false; }
    else if (!strcmp(argv[i], "--body-gains") && i + 2 < argc) { for (int k = 0; k < 2; k++) bodyGains[k] = atof(argv[++i]); bodySeen = true; }
    else if (!strcmp(argv[i], "--body-locks") && i + 1 < argc) {
      bodySeen = true;
      for (const char* c = argv[++i]; *c; c++) {
        const char* at = strchr("xyzr", *c);
        if (at) bodyLocks |= 1u << (at - "xyzr"); else bodyLocksOk = false;
      }
    }
    else if (!strcmp(argv[i], "--drain-every") && i + 1 < argc) { drainEvery = atoi(argv[++i]); drainSeen = true; }
    else if (!strcmp(argv[i], "--drain-at") && i + 1 < argc) { drainAt = atoi(argv[++i]); drainSeen = true; }
    else if (!strcmp(argv[i], "--drain-types")) {
      drainSeen = drainTypesSeen = true;
      while (i + 1 < argc && argv[i + 1][0] != '-') {
        const int t = atoi(argv[++i]);
        if (t < 1 || t > 3) { fprintf(stderr, "--drain-types: a type is 1 (liquid), 2 (elastic) or 3 (boundary)\n"); return 2; }
        drainMask |= 1u << t;
      }
    }
    else if (!strcmp(argv[i], "--dye-region") && i + 6 < argc) { for (int k = 0; k < 6; k++) dyeRegion[k] = (float)atof(argv[++i]); dyeSeen = dyeRegionSeen = true; }
    else if (!strcmp(argv[i], "--dye-inflow") && i + 1 < argc) { dyeInflow = (float)atof(argv[++i]); dyeSeen = true; }
    else if (!strcmp(argv[i], "--dye-diffusivity") && i + 1 < argc) { dyeDiffusivity = (float)atof(argv[++i]); dyeSeen = true; }
    else if (!strcmp(argv[i], "--dye-every") && i + 1 < argc) { dyeEvery = atoi(argv[++i]); dyeSeen = dyeEverySeen = true; }
    else if (!strcmp(argv[i], "--elastic-every") && i + 1 < argc) { elaEvery = atoi(argv[++i]); elaSeen = true; }
    else if (!strcmp(argv[i], "--elastic-out") && i + 1 < argc) { elaDir = argv[++i]; elaSeen = true; }
    else if (!strcmp(argv[i], "--forces-every") && i + 1 < argc) { forEvery = atoi(argv[++i]); forSeen = true; }
    else if (!strcmp(argv[i], "--wall-load-every") && i + 1 < argc) { wallEvery = atoi(argv[++i]); wallSeen = true; }
    else if (!strcmp(argv[i], "--gauge") && i + 1 < argc) {
      sph_gauge g = {};
      float w[9];
      int used = 0;
      gaugeOk = gaugeOk && sscanf(argv[++i], "%f %f %f %f %f %f %f %f %f %n", &w[0], &w[1], &w[2], &w[3], &w[4], &w[5], &w[6], &w[7], &w[8], &used) == 9 &&
                argv[i][used] == 0 && gaugeDefs.size() < SPH_MAX_GAUGES;
      for (int k = 0; k < 3; k++) { g.origin[k] = w[k]; g.u[k] = w[3 + k]; g.v[k] = w[6 + k]; }
      g.typeMask = 1u << SPH_LIQUID_PARTICLE; g.fieldSlot = -1;
      gaugeDefs.push_back(g); gaugeSeen = true;
    }
    else if (!strcmp(argv[i], "--gauge-plane")) { if (gaugeDefs.empty()) gaugeOk = false; else gaugeDefs.back().flags |= SPH_GAUGE_PLANE; gaugeSeen = true; }
    else if (!strcmp(argv[i], "--gauge-field") && i + 1 < argc) { if (gaugeDefs.empty()) { gaugeOk = false; ++i; } else gaugeDefs.back().fieldSlot = atoi(argv[++i]); gaugeSeen = true; }
    else if (!strcmp(argv[i], "--gauge-every") && i + 1 < argc) { gaugeEvery = atoi(argv[++i]); gaugeSeen = true; }
    else if (!strcmp(argv[i], "--probe") && i + 3 < argc) {
      for (int k = 0; k < 3; k++) probePoints.push_back((float)atof(argv[++i]));
      probePoints.push_back(0.f); probeSeen = true;
    }
    else if ((!strcmp(argv[i], "--level-line") && i + 7 < argc) || (!strcmp(argv[i], "--level-grid") && i + 9 < argc)) {
      const bool grid = !strcmp(argv[i], "--level-grid");
      float w[6];
      for (int k = 0; k < 6; k++) w[k] = (float)atof(argv[++i]);
      int n[3] = {1, 1, 0};
      if (grid) { n[0] = atoi(argv[++i]); n[1] = atoi(argv[++i]); }
      n[2] = atoi(argv[++i]);
      probeOk = probeOk && n[0] > 0 && n[1] > 0 && (long long)n[0] * n[1] + (long long)probeLines.size() <= SPH_PROBE_MAX_LINES;
      for (int j = 0; probeOk && j < n[1]; j++)
        for (int ii = 0; ii < n[0]; ii++) {
          sph_probe_line l = {};
          for (int k = 0; k < 3; k++) { l.origin[k] = w[k]; l.step[k] = grid ? 0.f : w[3 + k]; }
          if (grid) { l.origin[0] = w[0] + (float)ii * w[3]; l.origin[1] = w[1] + (float)j * w[4]; l.step[2] = w[5]; }
          l.count = n[2]; l.field = 1; l.iso = 0.5f; l.typeMask = 1u << SPH_LIQUID_PARTICLE;
          probeLines.push_back(l);
        }
      probeSeen = true;
    }
    else if (!strcmp(argv[i], "--probe-every") && i + 1 < argc) { probeEvery = atoi(argv[++i]); probeSeen = true; }
    else if (!strcmp(argv[i], "--probe-out") && i + 1 < argc) { probeFile = argv[++i]; probeSeen = true; }
    else if (!strcmp(argv[i], "--stats-grid") && i + 9 < argc) {
      for (int k = 0; k < 3; k++) statsGrid.origin[k] = (float)atof(argv[++i]);
      for (int k = 0; k < 3; k++) statsGrid.spacing[k] = (float)atof(argv[++i]);
      for (int k = 0; k < 3; k++) statsGrid.dims[k] = atoi(argv[++i]);
      if (!statsGrid.typeMask) statsGrid.typeMask = 1u << SPH_LIQUID_PARTICLE;
      statsSeen = statsGridSeen = true;
    }
    else if (!strcmp(argv[i], "--stats-types") && i + 1 < argc) {
      statsGrid.typeMask = 0u;
      for (const char* p = argv[++i]; *p; p++)
        if (*p >= '0' && *p <= '9') statsGrid.typeMask |= 1u << (*p - '0');
      statsSeen = true;
    }
    else if (!strcmp(argv[i], "--stats-from") && i + 1 < argc) { statsFrom = atoi(argv[++i]); statsSeen = true; }
    else if (!strcmp(argv[i], "--stats-every") && i + 1 < argc) { statsEvery = atoi(argv[++i]); statsSeen = true; }
    else if (!strcmp(argv[i], "--stats-out") && i + 1 < argc) { statsFile = argv[++i]; statsSeen = true; }
    else if (!strcmp(argv[i], "--bin-grid") && i + 9 < argc) {
      for (int k = 0; k < 3; k++) binGrid.origin[k] = (float)atof(argv[++i]);
      for (int k = 0; k < 3; k++) binGrid.spacing[k] = (float)atof(argv[++i]);
      for (int k = 0; k < 3; k++) binGrid.dims[k] = atoi(argv[++i]);
      if (!binGrid.typeMask) binGrid.typeMask = (1u << SPH_LIQUID_PARTICLE) | (1u << SPH_ELASTIC_PARTICLE);
      binSeen = binGridSeen = true;
    }
    else if (!strcmp(argv[i], "--bin-types") && i + 1 < argc) {
      binGrid.typeMask = 0u;
      for (const char* p = argv[++i]; *p; p++)
        if (*p >= '0' && *p <= '9') binGrid.typeMask |= 1u << (*p - '0');
      binSeen = true;
    }
    else if (!strcmp(argv[i], "--bin-every") && i + 1 < argc) { binEvery = atoi(argv[++i]); binSeen = true; }
    else if (!strcmp(argv[i], "--bin-out") && i + 1 < argc) { binFile = argv[++i]; binSeen = true; }
    else if (!strcmp(argv[i], "--render-every") && i + 1 < argc) { renEvery = atoi(argv[++i]); renSeen = true; }
    else if (!strcmp(argv[i], "--render-out") && i + 1 < argc) { renDir = argv[++i]; renSeen = true; }
    else if (!strcmp(argv[i], "--render-size") && i + 2 < argc) { renSize[0] = atoi(argv[++i]); renSize[1] = atoi(argv[++i]); renSeen = true; }
    else if (!strcmp(argv[i], "--render-eye") && i + 3 < argc) { for (int k = 0; k < 3; k++) renEye[k] = atof(argv[++i]); renSeen = renEyeSeen = true; }
    else if (!strcmp(argv[i], "--render-target") && i + 3 < argc) { for (int k = 0; k < 3; k++) renTarget[k] = atof(argv[++i]); renSeen = renTargetSeen = true; }
    else if (!strcmp(argv[i], "--render-up") && i + 3 < argc) { for (int k = 0; k < 3; k++) renUp[k] = atof(argv[++i]); renSeen = true; }
    else if (!strcmp(argv[i], "--render-ortho") && i + 1 < argc) { renOrtho = (float)atof(argv[++i]); renSeen = renOrthoSeen = true; }
    else if (!strcmp(argv[i], "--render-focal") && i + 1 < argc) { renFocal = (float)atof(argv[++i]); renSeen = renFocalSeen = true; }
    else if (!strcmp(argv[i], "--render-radius") && i + 1 < argc) { renRadius = (float)atof(argv[++i]); renSeen = renRadiusSeen = true; }
    else if (!strcmp(argv[i], "--render-colour") && i + 1 < argc) { renColour = argv[++i]; renSeen = true; }
    else if (!strcmp(argv[i], "--render-thickness")) { renThickness = renSeen = true; }
    else if (!strcmp(argv[i], "--render-surface")) { renSurface = renSeen = true; }
    else if (!strcmp(argv[i], "--render-membranes")) { renMembranes = renSeen = true; }
    else if (!strcmp(argv[i], "--render-types")) {
      renSeen = renTypesSeen = true;
      while (i + 1 < argc && argv[i + 1][0] != '-') {
        const int t = atoi(argv[++i]);
        if (t < 1 || t > 3) { fprintf(stderr, "--render-types: a type is 1 (liquid), 2 (elastic) or 3 (boundary)\n"); return 2; }
        renTypes |= 1u << t;
      }
    }
    else if (!strcmp(argv[i], "--select-every") && i + 1 < argc) { selEvery = atoi(argv[++i]); selSeen = true; }
    else if (!strcmp(argv[i], "--select-out") && i + 1 < argc) { selDir = argv[++i]; selSeen = true; }
    else if (!strcmp(argv[i], "--select-surface") && i + 1 < argc) { selTerms.push_back(sph_select_term{SPH_SELECT_FIELD_SURFACE, (float)atof(argv[++i]), INFINITY}); selSeen = true; }
    else if (!strcmp(argv[i], "--select-region") && i + 6 < argc) { for (int k = 0; k < 6; k++) selRegion[k] = (float)atof(argv[++i]); selSeen = selRegionSeen = true; }
    else if (!strcmp(argv[i], "--select-term") && i + 3 < argc) {
      const int f = select_field(argv[++i]);
      if (f < 0) { fprintf(stderr, "--select-term FIELD LO HI: FIELD is density, speed, pressure, neighbors, x, y, z, surface or 0..7\n"); return 2; }
      const float lo = (float)atof(argv[++i]), hi = (float)atof(argv[++i]);
      selTerms.push_back(sph_select_term{f, lo, hi});
      selSeen = true;
    }
    else if (!strcmp(argv[i], "--select-types")) {
      selSeen = selTypesSeen = true;
      while (i + 1 < argc && argv[i + 1][0] != '-') {
        const int t = atoi(argv[++i]);
        if (t < 1 || t > 3) { fprintf(stderr, "--select-types: a type is 1 (liquid), 2 (elastic) or 3 (boundary)\n"); return 2; }
        selMask |= 1u << t;
      }
    }
    else if (!strcmp(argv[i], "--components-every") && i + 1 < argc) { compEvery = atoi(argv[++i]); compSeen = true; }
    else if (!strcmp(argv[i], "--components-out") && i + 1 < argc) { compFile = argv[++i]; compSeen = true; }
    else if (!strcmp(argv[i], "--components-link") && i + 1 < argc) { compLink = (float)atof(argv[++i]); compSeen = true; }
    else if (!strcmp(argv[i], "--components-top") && i + 1 < argc) { compTop = atoi(argv[++i]); compSeen = true; }
    else if (!strcmp(argv[i], "--components-types")) {
      compSeen = compTypesSeen = true;
      while (i + 1 < argc && argv[i + 1][0] != '-') {
        const int t = atoi(argv[++i]);
        if (t < 1 || t > 3) { fprintf(stderr, "--components-types: a type is 1 (liquid), 2 (elastic) or 3 (boundary)\n"); return 2; }
        compMask |= 1u << t;
      }
    }
    else if (!strcmp(argv[i], "--velocity") && i + 1 < argc) velFile = argv[++i];
    else if (!strcmp(argv[i], "--out") && i + 1 < argc) outFile = argv[++i];
    else if (!strcmp(argv[i], "--steps") && i + 1 < argc) steps = atoi(argv[++i]);
    else if (!strcmp(argv[i], "--box") && i + 3 < argc) { for (int k = 0; k < 3; k++) box[k] = atof(argv[++i]); }
    else if (!strcmp(argv[i], "--lattice") && i + 3 < argc) { for (int k = 0; k < 3; k++) lat[k] = atoi(argv[++i]); }
    else if (!strcmp(argv[i], "--staged")) staged = true;
    else if (!strcmp(argv[i], "--wide")) wide = true;
    else if (!strcmp(argv[i], "--quiet")) quiet = true;
    else if (!strcmp(argv[i], "--muscles")) muscles = true;
    else if (!strcmp(argv[i], "--worm")) worm = true;
    else if (!strcmp(argv[i], "--blocking-readback")) blockingRead = true;  // the reference's blocking read_position_buffer
    else if (!strcmp(argv[i], "--sample-grid") && i + 3 < argc) { for (int k = 0; k < 3; k++) sampleDims[k] = atoi(argv[++i]); }
    else if (!strcmp(argv[i], "--sample-every") && i + 1 < argc) sampleEvery = atoi(argv[++i]);
    else if (!strcmp(argv[i], "--sample-out") && i + 1 < argc) sampleDir = argv[++i];
    else if (!strcmp(argv[i], "--surface-grid") && i + 3 < argc) { for (int k = 0; k < 3; k++) surfDims[k] = atoi(argv[++i]); }
    else if (!strcmp(argv[i], "--surface-every") && i + 1 < argc) surfEvery = atoi(argv[++i]);
    else if (!strcmp(argv[i], "--surface-out") && i + 1 < argc) surfDir = argv[++i];
    else if (!strcmp(argv[i], "--surface-iso") && i + 1 < argc) surfIso = (float)atof(argv[++i]);
    else if (!strcmp(argv[i], "--sample-gradients")) sampleGradients = true;
    else if (!strcmp(argv[i], "--diagnostics-every") && i + 1 < argc) { diagEvery = atoi(argv[++i]); diagEverySeen = true; }
    else if (!strcmp(argv[i], "--diagnostics-out") && i + 1 < argc) diagFile = argv[++i];
    else if (!strcmp(argv[i], "--diagnostics-region") && i + 6 < argc) { for (int k = 0; k < 6; k++) diagRegions.push_back((float)atof(argv[++i])); }
    else if (!strcmp(argv[i], "--surface-normals")) surfNormals = true;
    else if (!strcmp(argv[i], "--surface-shells")) surfShells = true;
    else { fprintf(stderr, "unknown argument %s\n", argv[i]); return 2; }
  }
  const bool sampling = sampleDims[0] > 0 || sampleEvery > 0 || sampleDir;
  if (sampling && (sampleDims[0] <= 0 || sampleDims[1] <= 0 || sampleDims[2] <= 0 || sampleEvery <= 0 || !sampleDir)) {
    fprintf(stderr, "--sample-grid NX NY NZ (all > 0), --sample-every K (> 0) and --sample-out DIR go together\n");
    return 2;
  }
  // --render-surface draws the --surface-grid mesh; the PLY files need --surface-every and --surface-out as before
  const bool surfacing = surfEvery > 0 || surfDir || (surfDims[0] > 0 && !renSurface);
  if (surfacing && (surfDims[0] < 2 || surfDims[1] < 2 || surfDims[2] < 2 || surfEvery <= 0 || !surfDir)) {
    fprintf(stderr, "--surface-grid NX NY NZ (all >= 2), --surface-every K (> 0) and --surface-out DIR go together\n");
    return 2;
  }
  const long long kSeedMax = 1 << 24;
  if (streamSeen && (streamSeeds[0] <= 0 || streamSeeds[1] <= 0 || (long long)streamSeeds[0] * streamSeeds[1] > kSeedMax || streamEvery <= 0 || !streamDir ||
                     streamMaxSteps < 0 || streamMaxSteps > SPH_TRACE_MAX_STEPS_LIMIT || !std::isfinite(streamStep))) {
    fprintf(stderr, "--streamlines NU NV (> 0), --stream-every K (> 0) and --stream-out DIR go together; --stream-step S: finite, not 0; --stream-max-steps M: 0..65535\n");
    return 2;
  }
  if (tracersSeen && (tracerSeeds[0] <= 0 || tracerSeeds[1] <= 0 || (long long)tracerSeeds[0] * tracerSeeds[1] > kSeedMax || tracersEvery <= 0)) {
    fprintf(stderr, "--tracers NU NV (> 0) [--tracers-every K (> 0)]\n");
    return 2;
  }
  if (sampleGradients && !sampling) { fprintf(stderr, "--sample-gradients needs --sample-grid\n"); return 2; }
  if (surfNormals && !surfacing) { fprintf(stderr, "--surface-normals needs --surface-grid\n"); return 2; }
  if (surfShells && !surfacing) { fprintf(stderr, "--surface-shells needs --surface-grid\n"); return 2; }
  const int diagCount = (int)(diagRegions.size() / 6);
  const bool diagnosing = diagEverySeen || diagFile || diagCount > 1;
  if (diagnosing && (diagEvery <= 0 || !diagFile)) {
    fprintf(stderr, "--diagnostics-every K (> 0) and --diagnostics-out FILE.csv go together (--diagnostics-region needs both)\n");
    return 2;
  }
  if (diagCount > SPH_DIAG_MAX_REGIONS) {
    fprintf(stderr, "at most %d --diagnostics-region (the whole scene is always region 0)\n", SPH_DIAG_MAX_REGIONS - 1);
    return 2;
  }
  for (float b : diagRegions)
    if (std::isnan(b)) { fprintf(stderr, "--diagnostics-region: a bound is not a number\n"); return 2; }
  if (compSeen && (compEvery <= 0 || !compFile)) {
    fprintf(stderr, "--components-every K (> 0) and --components-out FILE.csv go together (the other --components options need both)\n");
    return 2;
  }
  if (compTypesSeen && !compMask) { fprintf(stderr, "--components-types needs at least one type\n"); return 2; }
  if (!compMask) compMask = (1u << SPH_LIQUID_PARTICLE) | (1u << SPH_ELASTIC_PARTICLE);
  if (std::isnan(compLink) || !(compLink > 0.f)) { fprintf(stderr, "--components-link R: R must be > 0\n"); return 2; }
  if (compTop < 1 || compTop > SPH_DIAG_MAX_REGIONS) { fprintf(stderr, "--components-top M: M must be in 1..%d\n", SPH_DIAG_MAX_REGIONS); return 2; }
  const bool labelling = compSeen;
  if (selSeen && (selEvery <= 0 || !selDir)) {
    fprintf(stderr, "--select-every K (> 0) and --select-out DIR go together (the other --select options need both)\n");
    return 2;
  }
  if (selTypesSeen && !selMask) { fprintf(stderr, "--select-types needs at least one type\n"); return 2; }
  if (!selMask) selMask = 1u << SPH_LIQUID_PARTICLE;
  if (selTerms.size() > SPH_SELECT_MAX_TERMS) { fprintf(stderr, "at most %d terms (--select-term, --select-surface)\n", SPH_SELECT_MAX_TERMS); return 2; }
  for (const sph_select_term& t : selTerms)
    if (std::isnan(t.lo) || std::isnan(t.hi) || !(t.lo < t.hi)) { fprintf(stderr, "a selection term needs LO < HI, both numbers\n"); return 2; }
  for (float b : selRegion)
    if (std::isnan(b)) { fprintf(stderr, "--select-region: a bound is not a number\n"); return 2; }
  const bool selecting = selSeen;
  if (elaSeen && (elaEvery <= 0 || !elaDir)) { fprintf(stderr, "--elastic-every K (> 0) and --elastic-out DIR go together\n"); return 2; }
  const bool measuringElastic = elaSeen;
  if (forSeen && forEvery <= 0) { fprintf(stderr, "--forces-every K needs K > 0\n"); return 2; }
  const bool measuringForces = forSeen;
  if (wallSeen && wallEvery <= 0) { fprintf(stderr, "--wall-load-every K needs K > 0\n"); return 2; }
  if (gaugeSeen && (!gaugeOk || gaugeDefs.empty() || gaugeEvery <= 0)) {
    fprintf(stderr, "--gauge \"OX OY OZ UX UY UZ VX VY VZ\" (nine numbers in one argument, at most %d gauges) and --gauge-every K (> 0) go "
                    "together; --gauge-plane and --gauge-field SLOT follow the gauge they belong to\n", SPH_MAX_GAUGES);
    return 2;
  }
  if (probeSeen && (!probeOk || (probePoints.empty() && probeLines.empty()) || probeEvery <= 0 || !probeFile ||
                    probePoints.size() / 4 > SPH_PROBE_MAX_POINTS)) {
    fprintf(stderr, "--probe X Y Z, --level-line OX OY OZ SX SY SZ N and --level-grid OX OY OZ SX SY SZ NX NY NZ (at most %d points and %d "
                    "lines) go with --probe-every K (> 0) and --probe-out FILE\n", SPH_PROBE_MAX_POINTS, SPH_PROBE_MAX_LINES);
    return 2;
  }
  if (statsSeen && (!statsGridSeen || statsFrom < 0 || statsEvery <= 0 || !statsFile)) {
    fprintf(stderr, "--stats-grid OX OY OZ SX SY SZ NX NY NZ goes with --stats-out FILE; --stats-types \"T ...\", --stats-from S (>= 0) and "
                    "--stats-every K (> 0) need both\n");
    return 2;
  }
  if (binSeen && (!binGridSeen || binEvery <= 0 || !binFile || binGrid.dims[0] <= 0 || binGrid.dims[1] <= 0 || binGrid.dims[2] <= 0 ||
                  (long long)binGrid.dims[0] * binGrid.dims[1] * binGrid.dims[2] > SPH_BIN_MAX_BINS)) {
    fprintf(stderr, "--bin-grid OX OY OZ SX SY SZ NX NY NZ (NX, NY, NZ > 0, at most %d bins) goes with --bin-out FILE; --bin-types \"T ...\" and "
                    "--bin-every K (> 0) need both\n", SPH_BIN_MAX_BINS);
    return 2;
  }
  if (renSeen && (renEvery <= 0 || !renDir)) {
    fprintf(stderr, "--render-every K (> 0) and --render-out DIR go together (the other --render options need both)\n");
    return 2;
  }
  const bool rendering = renSeen;
  const bool renMeshes = renSurface || renMembranes;
  if (renSurface && (surfDims[0] < 2 || surfDims[1] < 2 || surfDims[2] < 2)) { fprintf(stderr, "--render-surface needs --surface-grid NX NY NZ (all >= 2)\n"); return 2; }
  if (renTypesSeen && (!renMeshes || !renTypes)) {
    fprintf(stderr, "--render-types T... (at least one type) chooses the particles --render-surface / --render-membranes are drawn over\n"); return 2;
  }
  if (renMeshes && !renTypesSeen && renThickness) { fprintf(stderr, "--render-thickness needs particles: give --render-types\n"); return 2; }
  if (capSeen && capacity <= 0) { fprintf(stderr, "--capacity N: N must be > 0\n"); return 2; }
  if (emitSeen && (!emitLatSeen || emitDims[0] <= 0 || emitDims[1] <= 0 || emitDims[2] <= 0 || emitEvery <= 0)) {
    fprintf(stderr, "--emit-lattice OX OY OZ NX NY NZ (NX, NY, NZ > 0) is needed by the other --emit options; --emit-every K needs K > 0\n");
    return 2;
  }
  if (emitSeen && !capSeen) { fprintf(stderr, "--emit-lattice needs --capacity N: the solver's buffers are sized when it is made\n"); return 2; }
  if (emitSeen && (std::isnan(emitSpacing) || emitSpacing < 0.f)) { fprintf(stderr, "--emit-spacing S: S must be > 0\n"); return 2; }
  if (drainSeen && drainEvery <= 0 && drainAt < 0) { fprintf(stderr, "a drain needs --drain-every K (> 0) or --drain-at STEP (>= 0)\n"); return 2; }
  if (drainTypesSeen && !drainMask) { fprintf(stderr, "--drain-types needs at least one type\n"); return 2; }
  if (!drainMask) drainMask = 1u << SPH_LIQUID_PARTICLE;
  for (float b : drainRegion)
    if (std::isnan(b)) { fprintf(stderr, "--drain-region: a bound is not a number\n"); return 2; }
  for (float b : dyeRegion)
    if (std::isnan(b)) { fprintf(stderr, "--dye-region: a bound is not a number\n"); return 2; }
  if (dyeSeen && (!std::isfinite(dyeInflow) || !std::isfinite(dyeDiffusivity) || dyeDiffusivity < 0.f || (dyeEverySeen && dyeEvery <= 0))) {
    fprintf(stderr, "--dye-inflow V: a finite number; --dye-diffusivity D: a finite number >= 0; --dye-every K: K > 0\n");
    return 2;
  }
  if (bodySeen) {
    bool ok = bodyRegionSeen && bodyFrom >= 0;
    for (float b : bodyRegion) ok = ok && !std::isnan(b);
    for (double v : bodyVel) ok = ok && std::isfinite(v);
    for (double v : bodySpin) ok = ok && std::isfinite(v);
    if (bodySpinSeen && !(bodySpin[0] * bodySpin[0] + bodySpin[1] * bodySpin[1] + bodySpin[2] * bodySpin[2] > 0)) ok = false;
    if (!bodyLocksOk || !std::isfinite(bodyGains[0]) || !std::isfinite(bodyGains[1])) ok = false;
    if (!ok && bodyFree) fprintf(stderr, "--body-free: --body-mass M > 0, --body-locks of the letters x y z r, --body-gains C F finite\n");
    if (!ok) {
      fprintf(stderr, "--body-region X0 Y0 Z0 X1 Y1 Z1 (no bound a NaN) is needed by the other --body options; --body-velocity and "
                      "--body-spin take finite numbers, the spin axis is not zero; --body-from STEP: STEP >= 0\n");
      return 2;
    }
  }
  const bool dyeing = dyeSeen;
  const bool emitting = emitSeen, draining = drainSeen, editing = emitSeen || drainSeen;
  const bool moving = bodySeen;
  // the host buffer of the asynchronous read-back is page-locked in place at its first size: with a changing count the driver
  // reads the positions the blocking way; so it does with a body, whose pose waits for a read-back in flight anyway
  if (editing || moving) blockingRead = true;
  sph_render_view renView;
  memset(&renView, 0, sizeof(renView));
  if (rendering) {
    if (renSize[0] < 1 || renSize[0] > 8192 || renSize[1] < 1 || renSize[1] > 8192 || (long long)renSize[0] * renSize[1] > (1LL << 24)) {
      fprintf(stderr, "--render-size W H: 1..8192 each and W*H <= 16777216\n"); return 2;
    }
    if (renOrthoSeen && renFocalSeen) { fprintf(stderr, "--render-ortho and --render-focal exclude each other\n"); return 2; }
    if ((renOrthoSeen && !(renOrtho > 0.f && std::isfinite(renOrtho))) || (renFocalSeen && !(renFocal > 0.f && std::isfinite(renFocal)))) {
      fprintf(stderr, "--render-ortho S / --render-focal F: a finite number > 0\n"); return 2;
    }
    if (renRadiusSeen && !(renRadius > 0.f && std::isfinite(renRadius))) { fprintf(stderr, "--render-radius R: a finite number > 0\n"); return 2; }
    if (!strcmp(renColour, "type")) renView.colourMode = 0;
    else if (!strcmp(renColour, "density")) renView.colourMode = 1;
    else if (!strcmp(renColour, "label")) renView.colourMode = 3;
    else {
      int n = 0;
      if (sscanf(renColour, "field:%d:%f:%f%n", &renView.field, &renView.lo, &renView.hi, &n) != 3 || renColour[n] || renView.field < 0 ||
          renView.field > 6 || !std::isfinite(renView.lo) || !std::isfinite(renView.hi) || !(renView.lo < renView.hi)) {
        fprintf(stderr, "--render-colour: type, density, label or field:N:LO:HI with N in 0..6 and LO < HI, both finite\n"); return 2;
      }
      renView.colourMode = 2;
    }
  }
  try {
    sph_config cfg;
    sphmi_default_config(&cfg);
    std::vector<float> position_cpp, velocity_cpp, elasticConnectionsData_cpp;
    std::vector<int> membraneData_cpp, particleMembranesList_cpp;
    int numOfLiquidP = 0, numOfElasticP = 0, numOfBoundaryP = 0;
    if (posFile && velFile) {  // owHelper::preLoadConfiguration + loadConfiguration
      int n = sphmi_count_particles(posFile);
      if (n <= 0) throw std::runtime_error(std::string("Could not open file ") + posFile);
      cfg.particleCount = n;
      position_cpp.resize(4 * (size_t)n); velocity_cpp.resize(4 * (size_t)n);
      if (sphmi_load_configuration(posFile, velFile, n, position_cpp.data(), velocity_cpp.data(), &numOfLiquidP, &numOfElasticP, &numOfBoundaryP))
        throw std::runtime_error("could not load configuration");
      if (numOfElasticP) throw std::runtime_error("elastic particles need elasticconnections.txt, which the reference repository does not ship");
    } else if (worm) {  // owHelper::generateConfiguration, shipped box (owPhysicsFluidSimulator.cpp:36-53)
      int numOfMembranes = 0;
      if (sphmi_worm_counts(&cfg, 30.0, 20.0, 250.0, &numOfElasticP, &numOfLiquidP, &numOfBoundaryP, &numOfMembranes)) throw std::runtime_error("worm scene: bad configuration");
      cfg.particleCount = numOfElasticP + numOfLiquidP + numOfBoundaryP;
      cfg.numOfElasticP = numOfElasticP; cfg.numOfMembranes = numOfMembranes; cfg.elasticOffset = 0;
      position_cpp.resize(4 * (size_t)cfg.particleCount); velocity_cpp.resize(4 * (size_t)cfg.particleCount);
      elasticConnectionsData_cpp.resize((size_t)4 * SPH_MAX_NEIGHBOR_COUNT * numOfElasticP);
      membraneData_cpp.resize(3 * (size_t)numOfMembranes);
      particleMembranesList_cpp.resize((size_t)SPH_MAX_MEMBRANES_INCLUDING_SAME_PARTICLE * numOfElasticP);
      if (sphmi_generate_worm(&cfg, 30.0, 20.0, 250.0, position_cpp.data(), velocity_cpp.data(), elasticConnectionsData_cpp.data(),
                              membraneData_cpp.data(), particleMembranesList_cpp.data()))
        throw std::runtime_error("worm scene generation failed");
    } else if (box[0] > 0 && lat[0] > 0) {  // synthetic pure-liquid box, SURVEY 8(d)
      if (sphmi_config_set_box(&cfg, box[0], box[1], box[2], wide ? 0xffffffffu : 0xffffu)) throw std::runtime_error("bad box");
      if (sphmi_box_counts(&cfg, box[0], box[1], box[2], lat[0], lat[1], lat[2], &numOfLiquidP, &numOfBoundaryP)) throw std::runtime_error("bad lattice");
      cfg.particleCount = numOfLiquidP + numOfBoundaryP;
      position_cpp.resize(4 * (size_t)cfg.particleCount); velocity_cpp.resize(4 * (size_t)cfg.particleCount);
      const float sp = 0.93f * cfg.r0, o = 3.0f * cfg.r0;
      if (sphmi_generate_box(&cfg, box[0], box[1], box[2], lat[0], lat[1], lat[2], sp, o, o, o, 0.f, 20261004ull, position_cpp.data(), velocity_cpp.data()))
        throw std::runtime_error("box generation failed");
    } else {
      fputs(usage, stderr);
      return 2;
    }
    if (capSeen) {
      if (capacity < cfg.particleCount) { fprintf(stderr, "--capacity %d is below the scene's %d particles\n", capacity, cfg.particleCount); return 2; }
      cfg.capacity = capacity;
    }
    if (emitting && emitSpacing == 0.f) emitSpacing = 0.93f * cfg.r0;
    if (emitUntil < 0) emitUntil = steps;
    int particleCount = cfg.particleCount;  // changes with every edit
    if (measuringElastic && numOfElasticP == 0) { fprintf(stderr, "--elastic-every needs a scene with elastic matter (--worm)\n"); return 2; }
    if (renMembranes && membraneData_cpp.empty()) { fprintf(stderr, "--render-membranes needs a scene with membranes (--worm)\n"); return 2; }
    printf("particles: %d (liquid %d, elastic %d, boundary %d), grid %d x %d x %d\n", cfg.particleCount, numOfLiquidP,
           numOfElasticP, numOfBoundaryP, cfg.gridCellsX, cfg.gridCellsY, cfg.gridCellsZ);
    owOpenCLSolver* ocl_solver = new owOpenCLSolver(cfg, position_cpp.data(), velocity_cpp.data(),
                                                    elasticConnectionsData_cpp.empty() ? nullptr : elasticConnectionsData_cpp.data(),
                                                    membraneData_cpp.empty() ? nullptr : membraneData_cpp.data(),
                                                    particleMembranesList_cpp.empty() ? nullptr : particleMembranesList_cpp.data());
    std::vector<float> muscle_activation_signal_cpp(cfg.muscleCount, 0.f);
    std::vector<double> muscleRecords(measuringElastic ? ((size_t)cfg.muscleCount + 1) * SPH_MUSCLE_WORDS : 0);
    float sampleOrigin[3] = {cfg.xmin, cfg.ymin, cfg.zmin}, sampleSpacing[3];
    const float boxMax[3] = {cfg.xmax, cfg.ymax, cfg.zmax};
    for (int k = 0; k < 3; k++) sampleSpacing[k] = sampleDims[k] > 1 ? (boxMax[k] - sampleOrigin[k]) / (float)(sampleDims[k] - 1) : 0.f;
    std::vector<float> fields(sampling ? (size_t)sampleDims[0] * sampleDims[1] * sampleDims[2] * SPH_SAMPLE_WORDS : 0);
    float surfSpacing[3];
    for (int k = 0; k < 3; k++) surfSpacing[k] = surfDims[k] > 1 ? (boxMax[k] - sampleOrigin[k]) / (float)(surfDims[k] - 1) : 0.f;
    std::vector<float> gradients(sampleGradients ? (size_t)sampleDims[0] * sampleDims[1] * sampleDims[2] * SPH_GRADIENT_WORDS : 0);
    std::vector<float> meshVerts, meshNormals;
    std::vector<int32_t> meshTris;
    std::vector<double> diagRecords((size_t)diagCount * SPH_DIAG_WORDS);
    FILE* diagCsv = nullptr;
    if (diagnosing) {
      diagCsv = fopen(diagFile, "w");
      if (!diagCsv) throw std::runtime_error(std::string("cannot write ") + diagFile);
      fputs("step,region,", diagCsv);
      fputs(kDiagCsvFields, diagCsv);
    }
    std::vector<double> binRecords(binSeen ? (size_t)binGrid.dims[0] * binGrid.dims[1] * binGrid.dims[2] * SPH_DIAG_WORDS : 0);
    FILE* binCsv = nullptr;
    if (binSeen) {
      binCsv = fopen(binFile, "w");
      if (!binCsv) throw std::runtime_error(std::string("cannot write ") + binFile);
      fputs("step,bin,", binCsv);
      fputs(kDiagCsvFields, binCsv);
    }
    FILE* compCsv = nullptr;
    std::vector<int32_t> compRootCount, compIds;
    std::vector<float> compBbox;
    std::vector<double> compRecords;
    std::vector<int32_t> selIndex; std::vector<uint32_t> selIds; std::vector<float> selRecords;
    std::vector<uint8_t> renRgba; std::vector<float> renDepth; std::vector<uint32_t> renThick;
    if (rendering) {  // the defaults of sphmi.frames.render_view
      const double lo[3] = {cfg.xmin, cfg.ymin, cfg.zmin}, hi[3] = {cfg.xmax, cfg.ymax, cfg.zmax};
      const double diag = std::sqrt(((hi[0] - lo[0]) * (hi[0] - lo[0]) + (hi[1] - lo[1]) * (hi[1] - lo[1])) + (hi[2] - lo[2]) * (hi[2] - lo[2]));
      const double dir[3] = {0.6, 0.5, 1.0}, dirLen = std::sqrt((0.6 * 0.6 + 0.5 * 0.5) + 1.0);
      for (int k = 0; k < 3; k++) {
        if (!renTargetSeen) renTarget[k] = 0.5 * (lo[k] + hi[k]);
        if (!renEyeSeen) renEye[k] = renTarget[k] + 2.0 * diag * dir[k] / dirLen;
      }
      if (!look_at(renEye, renTarget, renUp, &renView)) throw std::runtime_error("--render-eye / --render-target / --render-up: the eye is at the target, or up is parallel to the view direction");
      renView.width = renSize[0]; renView.height = renSize[1];
      renView.projection = renOrthoSeen ? 0 : 1;
      renView.scale = renOrthoSeen ? renOrtho : (renFocalSeen ? renFocal : (float)renSize[0]);
      renView.centre[0] = 0.5f * (float)renSize[0]; renView.centre[1] = 0.5f * (float)renSize[1];
      renView.nearPlane = 0.f;
      renView.radius = renRadiusSeen ? renRadius : 0.5f * cfg.r0;
      renView.maxRadiusPx = 256.f;
      const float typeColour[3][3] = {{0.2f, 0.45f, 0.9f}, {0.9f, 0.55f, 0.2f}, {0.6f, 0.6f, 0.6f}};
      memcpy(renView.typeColour, typeColour, sizeof(typeColour));
      renView.ambient = 0.25f;
      renView.background[0] = renView.background[1] = renView.background[2] = 0; renView.background[3] = 255;
    }
    if (labelling) {
      compCsv = fopen(compFile, "w");
      if (!compCsv) throw std::runtime_error(std::string("cannot write ") + compFile);
      fputs("step,component,root,n,min_x,min_y,min_z,max_x,max_y,max_z,"
            "n,sum_x,sum_y,sum_z,sum_vx,sum_vy,sum_vz,sum_lx,sum_ly,sum_lz,sum_v2,sum_rho,sum_e2,sum_p,reserved14,reserved15,"
            "min_rho,max_rho,min_p,max_p,max_v2,max_v2_index,max_v2_id,min_x,min_y,min_z,max_x,max_y,max_z,reserved29,reserved30,"
            "reserved31\n", compCsv);
    }
    // the seed plane of --streamlines / --tracers: across the box at mid-height, one multiply and one add per axis
    auto seed_plane = [&](const int n[2]) {
      std::vector<float> seeds(4 * (size_t)n[0] * (size_t)n[1], 0.f);
      const float dx = (cfg.xmax - cfg.xmin) / (float)n[0], dz = (cfg.zmax - cfg.zmin) / (float)n[1];
      const float x0 = cfg.xmin + 0.5f * dx, z0 = cfg.zmin + 0.5f * dz, y = 0.5f * (cfg.ymin + cfg.ymax);
      for (int j = 0; j < n[1]; j++)
        for (int i = 0; i < n[0]; i++) {
          float* p = &seeds[4 * ((size_t)j * n[0] + i)];
          p[0] = x0 + (float)i * dx; p[1] = y; p[2] = z0 + (float)j * dz;
        }
      return seeds;
    };
    std::vector<float> streamSeedPoints, streamVerts;
    std::vector<int32_t> streamLengths, streamStatus;
    const sph_trace_params streamParams = {streamStep != 0.f ? streamStep : 0.5f * cfg.h, 0.f, streamMaxSteps, SPH_TRACE_ARC, SPH_TRACE_MIDPOINT};
    if (streamSeen) {
      streamSeedPoints = seed_plane(streamSeeds);
      const size_t count = streamSeedPoints.size() / 4;
      streamVerts.resize(count * (size_t)(streamMaxSteps + 1) * 4); streamLengths.resize(count); streamStatus.resize(count);
    }
    const sph_trace_params tracerParams = {cfg.timeStep / cfg.simulationScale, 0.f, 0, SPH_TRACE_TIME, SPH_TRACE_MIDPOINT};
    if (tracersSeen) {
      const std::vector<float> points = seed_plane(tracerSeeds);
      ocl_solver->tracersSet(points.data(), (int)(points.size() / 4));
    }
    const unsigned dyeMask = 1u << SPH_LIQUID_PARTICLE;
    if (dyeing) {
      ocl_solver->fieldCreate(0, nullptr, dyeInflow);
      if (dyeRegionSeen) ocl_solver->fieldSetRegion(0, 1.0f, dyeRegion, dyeMask);
    }
    for (size_t g = 0; g < gaugeDefs.size(); g++) ocl_solver->gaugeDefine((int)g, &gaugeDefs[g]);  // (behind the dye: a gauge may sum field 0)
    if (probeSeen) {
      ocl_solver->probesSetPoints(probePoints.data(), (int)(probePoints.size() / 4), (1u << SPH_LIQUID_PARTICLE) | (1u << SPH_ELASTIC_PARTICLE));
      ocl_solver->probesSetLines(probeLines.data(), (int)probeLines.size());
      if (steps / probeEvery > 0) ocl_solver->probesHistory(steps / probeEvery);  // every call of the run stays in the ring
    }
    if (statsSeen) ocl_solver->statsDefine(0, &statsGrid);
    int64_t bodyMembers = 0;
    if (moving) {
      bodyMembers = ocl_solver->bodyDefineRegion(0, bodyRegion);
      if (bodyUntil < 0) bodyUntil = steps;
      if (bodyFree) {  // equal point masses at the reference placement, where the body stands now
        std::vector<float> ref(4 * (size_t)bodyMembers);
        ocl_solver->bodyRead(0, nullptr, ref.data(), nullptr);
        sph_body_dynamics dyn = {};
        dyn.mass = bodyMass > 0 ? bodyMass : (double)bodyMembers * (double)cfg.mass;
        double sum[3] = {0, 0, 0};
        for (int64_t k = 0; k < bodyMembers; k++)
          for (int c = 0; c < 3; c++) sum[c] = sum[c] + (double)ref[4 * k + c];
        for (int c = 0; c < 3; c++) dyn.com[c] = dyn.position[c] = sum[c] / (double)bodyMembers;
        double I[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}};
        const double mk = dyn.mass / (double)bodyMembers;
        for (int64_t k = 0; k < bodyMembers; k++) {
          const double r[3] = {(double)ref[4 * k] - dyn.com[0], (double)ref[4 * k + 1] - dyn.com[1], (double)ref[4 * k + 2] - dyn.com[2]};
          const double r2 = r[0] * r[0] + r[1] * r[1] + r[2] * r[2];
          for (int a = 0; a < 3; a++)
            for (int b = 0; b < 3; b++) I[a][b] += mk * ((a == b ? r2 : 0.0) - r[a] * r[b]);
        }
        const double c00 = I[1][1] * I[2][2] - I[1][2] * I[2][1], c01 = I[1][2] * I[2][0] - I[1][0] * I[2][2], c02 = I[1][0] * I[2][1] - I[1][1] * I[2][0];
        const double det = I[0][0] * c00 + I[0][1] * c01 + I[0][2] * c02, tr = I[0][0] + I[1][1] + I[2][2];
        if (det > 1e-12 * tr * tr * tr) {  // symmetric: the inverse is the adjugate over the determinant
          dyn.inertiaInv[0] = c00 / det;
          dyn.inertiaInv[1] = (I[0][0] * I[2][2] - I[0][2] * I[2][0]) / det;
          dyn.inertiaInv[2] = (I[0][0] * I[1][1] - I[0][1] * I[1][0]) / det;
          dyn.inertiaInv[3] = c01 / det;
          dyn.inertiaInv[4] = c02 / det;
          dyn.inertiaInv[5] = (I[0][2] * I[1][0] - I[0][0] * I[1][2]) / det;
        }
        dyn.orientation[0] = 1.0;
        const float posTimeStep = cfg.timeStep * cfg.simulationScaleInv;
        for (int c = 0; c < 3; c++) dyn.velocity[c] = bodyVel[c] / (double)posTimeStep;
        dyn.gravity[0] = cfg.gravity_x; dyn.gravity[1] = cfg.gravity_y; dyn.gravity[2] = cfg.gravity_z;
        dyn.contactGain = bodyGains[0]; dyn.forceGain = bodyGains[1];
        dyn.locks = bodyLocks;
        ocl_solver->bodySetDynamics(0, &dyn);
      }
    }
    Watch helper; helper.quiet = quiet;
    double total = 0;
    for (int iterationCount = 0; iterationCount < steps; iterationCount++) {
      helper.refresh();
      if (!quiet) printf("\n[[ Step %d ]]\n", iterationCount);
      if (moving && !bodyFree && ocl_solver->bodyCount(0) > 0 && iterationCount >= bodyFrom && iterationCount < bodyUntil) {  // (a drain may have taken the body)
        float pose[12];
        body_pose(bodySpin, bodyVel, (double)(iterationCount - bodyFrom + 1), pose);
        const float maxMove = ocl_solver->bodySetPose(0, pose);
        bodyMembers = ocl_solver->bodyCount(0);
        printf("_body: step %d members %lld max_move %.9g\n", iterationCount, (long long)bodyMembers, (double)maxMove);
        helper.report("_body: \t\t\t%9.3f ms\n");
      }
      if (editing) {  // between two steps: the drain first, then the emitter
        int64_t removed = 0, added = 0;
        bool edited = false;
        if (draining && ((drainEvery > 0 && iterationCount > 0 && iterationCount % drainEvery == 0) || iterationCount == drainAt)) {
          removed = ocl_solver->removeRegion(drainRegionSeen ? drainRegion : nullptr, drainMask);
          edited = true;
        }
        if (emitting && iterationCount % emitEvery == 0 && iterationCount < emitUntil) {
          const float sp[3] = {emitSpacing, emitSpacing, emitSpacing};
          added = ocl_solver->emitLattice(emitOrigin, sp, emitDims, emitVel, 1.0f);
          edited = true;
        }
        if (edited) {
          particleCount = ocl_solver->particleCount();
          position_cpp.resize(4 * (size_t)particleCount);
          printf("_edit: step %d removed %lld added %lld particles %d\n", iterationCount, (long long)removed, (long long)added, particleCount);
          helper.report("_edit: \t\t\t%9.3f ms\n");
        }
      }
      if (staged) {  // owPhysicsFluidSimulator.cpp:88-113, call for call
        ocl_solver->_runClearBuffers();       sph_synchronize(ocl_solver->handle()); helper.report("_runClearBuffers: \t%9.3f ms\n");
        ocl_solver->_runHashParticles();      sph_synchronize(ocl_solver->handle()); helper.report("_runHashParticles: \t%9.3f ms\n");
        ocl_solver->_runSort();               sph_synchronize(ocl_solver->handle()); helper.report("_runSort: \t\t%9.3f ms\n");
        ocl_solver->_runSortPostPass();       sph_synchronize(ocl_solver->handle()); helper.report("_runSortPostPass: \t%9.3f ms\n");
        ocl_solver->_runIndexx();             sph_synchronize(ocl_solver->handle()); helper.report("_runIndexx: \t\t%9.3f ms\n");
        ocl_solver->_runIndexPostPass();      sph_synchronize(ocl_solver->handle()); helper.report("_runIndexPostPass: \t%9.3f ms\n");
        ocl_solver->_runFindNeighbors();      sph_synchronize(ocl_solver->handle()); helper.report("_runFindNeighbors: \t%9.3f ms\n");
        ocl_solver->_run_pcisph_computeDensity();
        ocl_solver->_run_pcisph_computeForcesAndInitPressure();
        ocl_solver->_run_pcisph_computeElasticForces();
        int iter = 0;
        do {
          ocl_solver->_run_pcisph_predictPositions();
          ocl_solver->_run_pcisph_predictDensity();
          ocl_solver->_run_pcisph_correctPressure();
          ocl_solver->_run_pcisph_computePressureForceAcceleration();
          iter++;
        } while (iter < cfg.maxIteration);
        ocl_solver->_run_pcisph_integrate(iterationCount);
        sph_synchronize(ocl_solver->handle()); helper.report("_runPCISPH: \t\t%9.3f ms\t3 iteration(s)\n");
        ocl_solver->_run_clearMembraneBuffers();
        ocl_solver->_run_computeInteractionWithMembranes();
        ocl_solver->_run_computeInteractionWithMembranes_finalize();
      } else {
        ocl_solver->step(iterationCount);
        sph_synchronize(ocl_solver->handle()); helper.report("sph_step (fused): \t%9.3f ms\n");
      }
      // owPhysicsFluidSimulator.cpp:115. Default: the copy is only started here and overlaps the next step (the positions are
      // consumed after the loop); --blocking-readback waits for it like the reference does.
      if (blockingRead) ocl_solver->read_position_buffer(position_cpp.data());
      else ocl_solver->read_position_buffer_async(position_cpp.data());
      helper.report("_readBuffer: \t\t%9.3f ms\n");
      if (!quiet) printf("------------------------------------\n_Total_step_time:\t%9.3f ms\n------------------------------------\n", helper.elapsed());
      total += helper.elapsed();
      if (sampling && (iterationCount + 1) % sampleEvery == 0) {
        ocl_solver->sampleGrid(sampleOrigin, sampleSpacing, sampleDims, (1u << SPH_LIQUID_PARTICLE) | (1u << SPH_ELASTIC_PARTICLE) |
                               (1u << SPH_BOUNDARY_PARTICLE), fields.data());
        const std::string path = std::string(sampleDir) + "/fields_" + std::to_string(iterationCount + 1) + ".bin";
        FILE* f = fopen(path.c_str(), "wb");
        if (!f || fwrite(fields.data(), sizeof(float), fields.size(), f) != fields.size()) throw std::runtime_error("cannot write " + path);
        fclose(f);
        helper.report("_sampleGrid: \t\t%9.3f ms\n");
        if (sampleGradients) {
          ocl_solver->sampleGradientGrid(sampleOrigin, sampleSpacing, sampleDims, (1u << SPH_LIQUID_PARTICLE) |
                                         (1u << SPH_ELASTIC_PARTICLE) | (1u << SPH_BOUNDARY_PARTICLE), gradients.data());
          const std::string gpath = std::string(sampleDir) + "/gradients_" + std::to_string(iterationCount + 1) + ".bin";
          FILE* g = fopen(gpath.c_str(), "wb");
          if (!g || fwrite(gradients.data(), sizeof(float), gradients.size(), g) != gradients.size()) throw std::runtime_error("cannot write " + gpath);
          fclose(g);
          helper.report("_sampleGradientGrid: \t%9.3f ms\n");
        }
      }
      if (surfacing && (iterationCount + 1) % surfEvery == 0) {
        int64_t counts[2];
        ocl_solver->extractSurface(sampleOrigin, surfSpacing, surfDims, (1u << SPH_LIQUID_PARTICLE) | (1u << SPH_ELASTIC_PARTICLE),
                                   1 /* shepard */, surfIso, counts);
        meshVerts.resize((size_t)counts[0] * 3);
        meshTris.resize((size_t)counts[1] * 3);
        ocl_solver->readSurface(meshVerts.data(), meshTris.data());
        if (surfNormals) {
          meshNormals.resize(meshVerts.size());
          ocl_solver->surfaceNormals(meshNormals.data());
        }
        write_ply(std::string(surfDir) + "/surface_" + std::to_string(iterationCount + 1) + ".ply", meshVerts, meshTris,
                  surfNormals ? &meshNormals : nullptr);
        helper.report("_extractSurface: \t%9.3f ms\n");
        if (surfShells) {
          int64_t shellCounts[4];
          int32_t exps[3];
          ocl_solver->measureSurface(shellCounts, exps);
          std::vector<int64_t> table((size_t)shellCounts[0] * SPH_SHELL_WORDS);
          std::vector<float> boxes((size_t)shellCounts[0] * 6);
          ocl_solver->readShells(nullptr, table.data(), boxes.data());
          write_shells_csv(std::string(surfDir) + "/shells_" + std::to_string(iterationCount + 1) + ".csv", table, boxes, exps);
          helper.report("_measureSurface: \t%9.3f ms\n");
        }
      }
      if (binSeen && (iterationCount + 1) % binEvery == 0) {
        ocl_solver->binDiagnostics(&binGrid, binRecords.data());
        const size_t bins = binRecords.size() / SPH_DIAG_WORDS;
        double n = 0.0;
        for (size_t b = 0; b < bins; b++) {
          fprintf(binCsv, "%d,%zu", iterationCount + 1, b);
          for (int w = 0; w < SPH_DIAG_WORDS; w++) fprintf(binCsv, ",%.17g", binRecords[b * SPH_DIAG_WORDS + w]);
          fputc('\n', binCsv);
          n += binRecords[b * SPH_DIAG_WORDS];
        }
        if (fflush(binCsv) != 0) throw std::runtime_error(std::string("cannot write ") + binFile);
        if (!quiet) printf("_bins: step %d bins %zu n %.0f\n", iterationCount + 1, bins, n);
        helper.report("_binDiagnostics: \t%9.3f ms\n");
      }
      if (diagnosing && (iterationCount + 1) % diagEvery == 0) {
        ocl_solver->diagnostics(diagRegions.data(), diagCount, (1u << SPH_LIQUID_PARTICLE) | (1u << SPH_ELASTIC_PARTICLE), diagRecords.data());
        for (int r = 0; r < diagCount; r++) {
          fprintf(diagCsv, "%d,%d", iterationCount + 1, r);
          for (int w = 0; w < SPH_DIAG_WORDS; w++) fprintf(diagCsv, ",%.17g", diagRecords[(size_t)r * SPH_DIAG_WORDS + w]);
          fputc('\n', diagCsv);
        }
        if (fflush(diagCsv) != 0) throw std::runtime_error(std::string("cannot write ") + diagFile);
        if (!quiet) {
          const double* d = diagRecords.data();  // the whole scene
          const double n = d[0], inv = n > 0 ? 1.0 / n : 0.0;
          printf("_diagnostics: n %.0f  Ekin %.6e  max|v| %.6e  rho mean %.4f min %.4f max %.4f  rms(rho-rho0)/rho0 %.3e\n", n,
                 0.5 * (double)cfg.mass * d[10], std::sqrt(d[20]), d[11] * inv, d[16], d[17], std::sqrt(d[12] * inv) / (double)cfg.rho0);
        }
        helper.report("_diagnostics: \t\t%9.3f ms\n");
      }
      if (labelling && (iterationCount + 1) % compEvery == 0) {
        int64_t counts[2];
        ocl_solver->labelComponents(compLink, compMask, counts);
        const size_t C = (size_t)counts[1];
        compRootCount.resize(2 * C);
        compBbox.resize(6 * C);
        ocl_solver->components(nullptr, compRootCount.data(), compBbox.data());
        compIds.resize(C);
        for (size_t c = 0; c < C; c++) compIds[c] = (int32_t)c;
        const size_t top = std::min(C, (size_t)compTop);
        // descending n, then ascending root (= ascending id)
        std::partial_sort(compIds.begin(), compIds.begin() + top, compIds.end(), [&](int32_t a, int32_t b) {
          const int32_t na = compRootCount[2 * (size_t)a + 1], nb = compRootCount[2 * (size_t)b + 1];
          return na != nb ? na > nb : a < b;
        });
        compRecords.assign(top * SPH_DIAG_WORDS, 0.0);
        if (top) ocl_solver->componentDiagnostics(compIds.data(), (int)top, compRecords.data());
        for (size_t r = 0; r < top; r++) {
          const size_t c = (size_t)compIds[r];
          fprintf(compCsv, "%d,%d,%d,%d", iterationCount + 1, compIds[r], compRootCount[2 * c], compRootCount[2 * c + 1]);
          for (int k = 0; k < 6; k++) fprintf(compCsv, ",%.9g", compBbox[6 * c + k]);
          for (int w = 0; w < SPH_DIAG_WORDS; w++) fprintf(compCsv, ",%.17g", compRecords[r * SPH_DIAG_WORDS + w]);
          fputc('\n', compCsv);
        }
        if (fflush(compCsv) != 0) throw std::runtime_error(std::string("cannot write ") + compFile);
        if (!quiet) {
          const long long largest = top ? compRootCount[2 * (size_t)compIds[0] + 1] : 0;
          printf("_components: selected %lld  components %lld  largest %lld  outside it %lld\n", (long long)counts[0], (long long)counts[1],
                 largest, (long long)counts[0] - largest);
        }
        helper.report("_components: \t\t%9.3f ms\n");
      }
      if (rendering && (iterationCount + 1) % renEvery == 0) {
        const unsigned renMask = renTypesSeen ? renTypes : (1u << SPH_LIQUID_PARTICLE) | (1u << SPH_ELASTIC_PARTICLE);
        const bool particles = !renMeshes || renTypesSeen;
        int64_t counts[2] = {0, 0};
        if (particles) {
          if (renView.colourMode == 3) ocl_solver->labelComponents(INFINITY, renMask, counts);
          ocl_solver->renderParticles(renView, nullptr, renMask, renThickness, counts);
        }
        // the triangle passes: the surface of this frame's state, then the membranes, each over what is there already
        int64_t meshCounts[2][4] = {{0, 0, 0, 0}, {0, 0, 0, 0}};
        bool drawnOver = particles;
        if (renSurface) {
          int64_t mesh[2];
          ocl_solver->extractSurface(sampleOrigin, surfSpacing, surfDims, (1u << SPH_LIQUID_PARTICLE) | (1u << SPH_ELASTIC_PARTICLE),
                                     1 /* shepard */, surfIso, mesh);
          sph_render_mesh_style st = {0, 1, 0, 0, 0.f, 1.f, {0.35f, 0.6f, 0.95f}, drawnOver ? 1 : 0};  // smooth, one colour
          ocl_solver->renderMesh(renView, st, meshCounts[0]);
          drawnOver = true;
        }
        if (renMembranes) {
          sph_render_mesh_style st = {1, 0, 0, 0, 0.f, 1.f, {0.95f, 0.6f, 0.25f}, drawnOver ? 1 : 0};  // flat, one colour
          ocl_solver->renderMesh(renView, st, meshCounts[1]);
        }
        const size_t pixels = (size_t)renView.width * (size_t)renView.height;
        renRgba.resize(4 * pixels); renDepth.resize(pixels); renThick.resize(renThickness ? pixels : 0);
        ocl_solver->readRender(renDepth.data(), nullptr, nullptr, renRgba.data(), renThickness ? renThick.data() : nullptr);
        for (size_t p = 0; p < pixels; p++) memmove(&renRgba[3 * p], &renRgba[4 * p], 3);  // RGBA -> RGB in place
        const std::string base = std::string(renDir) + "/frame_" + std::to_string(iterationCount + 1);
        char header[64];
        const int hn = snprintf(header, sizeof(header), "P6\n%d %d\n255\n", renView.width, renView.height);
        if (!write_file(base + ".ppm", header, (size_t)hn, renRgba.data(), 3 * pixels)) throw std::runtime_error("cannot write " + base + ".ppm");
        if (!write_file(base + ".depth.f32", header, 0, renDepth.data(), sizeof(float) * pixels)) throw std::runtime_error("cannot write " + base + ".depth.f32");
        if (renThickness && !write_file(base + ".thickness.u32", header, 0, renThick.data(), sizeof(uint32_t) * pixels))
          throw std::runtime_error("cannot write " + base + ".thickness.u32");
        if (!quiet && particles) printf("_render: drew %lld particles, covered %lld of %zu pixels -> %s.ppm\n", (long long)counts[0], (long long)counts[1], pixels, base.c_str());
        if (!quiet && renMeshes) {
          const int64_t* last = meshCounts[renMembranes ? 1 : 0];
          printf("_render_mesh: surface drew %lld skipped %lld holds %lld, membranes drew %lld skipped %lld holds %lld, covered %lld of %zu pixels -> %s.ppm\n",
                 (long long)meshCounts[0][0], (long long)meshCounts[0][1], (long long)meshCounts[0][2], (long long)meshCounts[1][0],
                 (long long)meshCounts[1][1], (long long)meshCounts[1][2], (long long)last[3], pixels, base.c_str());
        }
        helper.report("_render: \t\t%9.3f ms\n");
      }
      if (selecting && (iterationCount + 1) % selEvery == 0) {
        const int64_t n = ocl_solver->selectParticles(selRegionSeen ? selRegion : nullptr, selMask, selTerms.data(), (int)selTerms.size());
        selIndex.resize((size_t)n); selIds.resize((size_t)n); selRecords.resize((size_t)n * SPH_SELECT_WORDS);
        ocl_solver->readSelection(selIndex.data(), selIds.data(), selRecords.data());
        const std::string path = std::string(selDir) + "/selection_" + std::to_string(iterationCount + 1) + ".bin";
        FILE* f = fopen(path.c_str(), "wb");  // little-endian host
        bool ok = f && fwrite(&n, sizeof(n), 1, f) == 1 && fwrite(selIndex.data(), sizeof(int32_t), selIndex.size(), f) == selIndex.size() &&
                  fwrite(selIds.data(), sizeof(uint32_t), selIds.size(), f) == selIds.size() &&
                  fwrite(selRecords.data(), sizeof(float), selRecords.size(), f) == selRecords.size();
        if (f && fclose(f) != 0) ok = false;
        if (!ok) throw std::runtime_error("cannot write " + path);
        if (!quiet) printf("_select: selected %lld of %d\n", (long long)n, particleCount);
        helper.report("_select: \t\t%9.3f ms\n");
      }
      if (measuringElastic && (iterationCount + 1) % elaEvery == 0) {
        ocl_solver->muscleDiagnostics(muscleRecords.data());
        const std::string path = std::string(elaDir) + "/muscles_" + std::to_string(iterationCount + 1) + ".csv";
        FILE* f = fopen(path.c_str(), "w");
        if (!f) throw std::runtime_error("cannot write " + path);
        fputs("group,n,signal,mean_length,mean_rest_length,mean_strain,min_strain,max_strain\n", f);
        double nAll = 0, eAll = 0, eMin = INFINITY, eMax = -INFINITY;
        for (int g = 0; g <= cfg.muscleCount; g++) {
          const double* r = &muscleRecords[(size_t)g * SPH_MUSCLE_WORDS];
          const double n = r[0];
          fprintf(f, "%d,%.0f,%.17g,%.17g,%.17g,%.17g,%.17g,%.17g\n", g, n, r[1], n > 0 ? r[3] / n : 0.0, n > 0 ? r[2] / n : 0.0,
                  n > 0 ? r[6] / n : 0.0, r[7], r[8]);
          if (n > 0) { nAll += n; eAll += r[6]; eMin = std::min(eMin, r[7]); eMax = std::max(eMax, r[8]); }
        }
        if (fclose(f) != 0) throw std::runtime_error("cannot write " + path);
        if (!quiet) {
          double totals[4] = {0, 0, 0, 0};
          if (cfg.numOfMembranes > 0) ocl_solver->membraneMeasure(nullptr, totals);
          printf("_elastic: connections %.0f  strain min %.6e mean %.6e max %.6e  membrane area %.9e over %.0f triangles\n", nAll,
                 nAll > 0 ? eMin : 0.0, nAll > 0 ? eAll / nAll : 0.0, nAll > 0 ? eMax : 0.0, totals[1], totals[0]);
        }
        helper.report("_elastic: \t\t%9.3f ms\n");
      }
      if (measuringForces && (iterationCount + 1) % forEvery == 0) {
        const float everything[6] = {-INFINITY, -INFINITY, -INFINITY, INFINITY, INFINITY, INFINITY};
        double r[SPH_FORCE_DIAG_WORDS];
        const bool worm = numOfElasticP > 0;
        ocl_solver->forceDiagnostics(everything, 1, worm ? (1u << SPH_ELASTIC_PARTICLE) : (1u << SPH_LIQUID_PARTICLE), r);
        const double m = (double)cfg.mass;
        // load of class c (1 liquid, 2 elastic, 3 boundary) on the selected particles: (viscous + pressure) + tension
        auto load = [&](int c, int axis) { const double* q = r + 1 + 9 * (c - 1); return (m * q[axis] + m * q[6 + axis]) + m * q[3 + axis]; };
        if (worm)
          printf("_forces: step %d  liquid on elastic (n %.0f): load %.9e %.9e %.9e N  torque %.9e %.9e %.9e  power %.9e W  "
                 "(pressure part %.9e %.9e %.9e N)\n", iterationCount + 1, r[0], load(1, 0), load(1, 1), load(1, 2), m * r[34], m * r[35],
                 m * r[36], m * r[43], m * r[7], m * r[8], m * r[9]);
        else
          printf("_forces: step %d  on liquid (n %.0f): boundary load %.9e %.9e %.9e N  liquid load %.9e %.9e %.9e N\n", iterationCount + 1,
                 r[0], load(3, 0), load(3, 1), load(3, 2), load(1, 0), load(1, 1), load(1, 2));
        helper.report("_forces: \t\t%9.3f ms\n");
      }
      if (wallSeen && (iterationCount + 1) % wallEvery == 0) {
        const float everything[6] = {-INFINITY, -INFINITY, -INFINITY, INFINITY, INFINITY, INFINITY};
        const double m = (double)cfg.mass, perDt = (double)cfg.mass / (double)cfg.timeStep;
        int defined = 0;
        for (int b = 0; b < SPH_MAX_BODIES; b++) defined += ocl_solver->bodyCount(b) > 0;
        for (int b = defined ? 0 : SPH_WALL_ALL; b < (defined ? SPH_MAX_BODIES : 0); b++) {
          const long long members = b >= 0 ? (long long)ocl_solver->bodyCount(b) : 0;
          if (b >= 0 && !members) continue;
          double r[SPH_WALL_DIAG_WORDS];
          ocl_solver->wallDiagnostics(b, everything, 1, 1u << SPH_LIQUID_PARTICLE, r);
          double contact[3], stage[3], load[3], torque[3];
          for (int a = 0; a < 3; a++) {
            contact[a] = perDt * r[7 + a];
            stage[a] = (m * r[10 + a] + m * r[16 + a]) + m * r[13 + a];
            load[a] = -(contact[a] + stage[a]);
            torque[a] = -(perDt * r[19 + a] + m * r[22 + a]);
          }
          char name[16];
          if (b >= 0) snprintf(name, sizeof(name), "%d", b); else snprintf(name, sizeof(name), "all");
          printf("_wall: step %d body %s (members %lld): contact n %.0f shared %.0f reflected %.0f  contact force %.9e %.9e %.9e N  "
                 "stage force %.9e %.9e %.9e N  load on body %.9e %.9e %.9e N  torque on body %.9e %.9e %.9e\n", iterationCount + 1, name,
                 members, r[1], r[2], r[3], contact[0], contact[1], contact[2], stage[0], stage[1], stage[2], load[0], load[1], load[2],
                 torque[0], torque[1], torque[2]);
        }
        helper.report("_wall: \t\t\t%9.3f ms\n");
      }
      if (gaugeSeen) {  // in front of the free body's advance, like every reader of the step just done
        ocl_solver->gaugesAccumulate(nullptr);
        if ((iterationCount + 1) % gaugeEvery == 0) {
          double tot[SPH_MAX_GAUGES * SPH_GAUGE_TOTAL_WORDS];
          ocl_solver->gaugesRead(tot);
          for (size_t g = 0; g < gaugeDefs.size(); g++) {
            const double* r = tot + g * SPH_GAUGE_TOTAL_WORDS;
            const double first = r[17] < 0 ? r[18] : r[18] < 0 ? r[17] : std::min(r[17], r[18]);
            double mp[3], mm[3];
            for (int a = 0; a < 3; a++) { mp[a] = r[0] > 0 ? r[1 + a] / r[0] : 0.0; mm[a] = r[8] > 0 ? r[9 + a] / r[8] : 0.0; }
            printf("_gauge: step %d gauge %d plus %.0f minus %.0f net %.0f calls %.0f first %.0f last %.0f  mean velocity plus %.9e %.9e %.9e "
                   "minus %.9e %.9e %.9e  field plus %.9e minus %.9e\n", iterationCount + 1, (int)g, r[0], r[8], r[0] - r[8], r[16], first, r[19],
                   mp[0], mp[1], mp[2], mm[0], mm[1], mm[2], r[5], r[13]);
          }
        }
        helper.report("_gauge: \t\t%9.3f ms\n");
      }
      if (probeSeen && (iterationCount + 1) % probeEvery == 0) {
        ocl_solver->probesRecord();  // no wait: the ring is read after the run
        helper.report("_probes: \t\t%9.3f ms\n");
      }
      if (statsSeen && iterationCount >= statsFrom && (iterationCount - statsFrom) % statsEvery == 0) {
        ocl_solver->statsAccumulate(0);  // no wait: the accumulators are read after the run
        statsCalls++;
        helper.report("_stats: \t\t%9.3f ms\n");
      }
      if (bodyFree && ocl_solver->bodyCount(0) > 0) {  // the load of the step just done moves the body (a drain may have taken it)
        std::vector<double> rec((size_t)SPH_MAX_BODIES * SPH_BODY_STATE_WORDS);
        ocl_solver->bodiesAdvance(rec.data());
        const double* r = rec.data();
        printf("_free: step %d body 0 status %.0f advances %.0f max_move %.9e  X %.9e %.9e %.9e  V %.9e %.9e %.9e  F %.9e %.9e %.9e\n",
               iterationCount + 1, r[0], r[2], r[3], r[4], r[5], r[6], r[11], r[12], r[13], r[20], r[21], r[22]);
        helper.report("_free: \t\t\t%9.3f ms\n");
      }
      if (dyeing) {
        const float stability = ocl_solver->fieldDiffuse(0, dyeDiffusivity * cfg.timeStep, dyeDiffusivity > 0.f ? 1 : 0, dyeMask);
        if (dyeEvery > 0 && (iterationCount + 1) % dyeEvery == 0) {
          const float everything[6] = {-INFINITY, -INFINITY, -INFINITY, INFINITY, INFINITY, INFINITY};
          double r[SPH_FIELD_DIAG_WORDS];
          ocl_solver->fieldDiagnostics(0, everything, 1, dyeMask, r);
          const double mean = r[0] > 0 ? r[1] / r[0] : 0.0, var = r[0] > 0 ? r[2] / r[0] - mean * mean : 0.0;
          printf("dye step=%d n=%.0f sum=%.17g mean=%.17g var=%.17g min=%.17g max=%.17g stability=%.9g\n", iterationCount + 1, r[0], r[1],
                 mean, var, r[3], r[4], (double)stability);
        }
        helper.report("_dye: \t\t\t%9.3f ms\n");
      }
      if (streamSeen && (iterationCount + 1) % streamEvery == 0) {
        ocl_solver->traceStreamlines(streamSeedPoints.data(), (int)streamLengths.size(), (1u << SPH_LIQUID_PARTICLE) | (1u << SPH_ELASTIC_PARTICLE),
                                     streamParams, nullptr, streamVerts.data(), streamLengths.data(), streamStatus.data());
        write_vtk_polylines(std::string(streamDir) + "/streamlines_" + std::to_string(iterationCount + 1) + ".vtk", streamVerts, streamLengths,
                            streamMaxSteps + 1);
        helper.report("_streamlines: \t\t%9.3f ms\n");
      }
      if (tracersSeen) {
        const int64_t moving = ocl_solver->tracersAdvect(1u << SPH_LIQUID_PARTICLE, tracerParams);
        if ((iterationCount + 1) % tracersEvery == 0)
          printf("tracers step=%d moving=%lld stopped=%lld\n", iterationCount + 1, (long long)moving,
                 (long long)tracerSeeds[0] * tracerSeeds[1] - (long long)moving);
        helper.report("_tracers: \t\t%9.3f ms\n");
      }
      if (muscles) {  // signals computed after step t drive step t+1 (owPhysicsFluidSimulator.cpp:134-141)
        sphmi_muscle_signal(iterationCount, muscle_activation_signal_cpp.data(), cfg.muscleCount);
        ocl_solver->updateMuscleActivityData(muscle_activation_signal_cpp.data());
      }
    }
    {
      helper.refresh();
      ocl_solver->wait_position_buffer();  // the last step's copy
      helper.report("");
      total += helper.elapsed();
    }
    printf("%d steps, %.3f ms/step incl. the 16N-byte position read-back, %.3e particle-steps/s\n", steps, total / steps,
           particleCount * 1000.0 / (total / steps));
    if (outFile) {
      FILE* f = fopen(outFile, "wb");
      if (!f || fwrite(position_cpp.data(), sizeof(float), position_cpp.size(), f) != position_cpp.size()) throw std::runtime_error("cannot write --out file");
      fclose(f);
    }
    if (probeSeen) {
      const size_t P = probePoints.size() / 4, L = probeLines.size(), words = SPH_PROBE_LEVEL_WORDS;
      const int calls = steps / probeEvery;
      std::vector<float> pts((size_t)calls * P * words), lev((size_t)calls * L * words);
      if (calls > 0) ocl_solver->probesReadHistory(0, calls, pts.data(), lev.data());
      FILE* f = fopen(probeFile, "wb");
      bool ok = f && fprintf(f, "sphmi probes calls %d points %zu lines %zu every %d\n", calls, P, L, probeEvery) > 0;
      for (int c = 0; ok && c < calls; c++)
        ok = fwrite(pts.data() + (size_t)c * P * words, sizeof(float), P * words, f) == P * words &&
             fwrite(lev.data() + (size_t)c * L * words, sizeof(float), L * words, f) == L * words;
      if (!ok || fclose(f) != 0) throw std::runtime_error(std::string("cannot write ") + probeFile);
      printf("_probes: calls %d points %zu lines %zu\n", calls, P, L);
    }
    if (statsSeen) {
      const size_t nodes = (size_t)statsGrid.dims[0] * statsGrid.dims[1] * statsGrid.dims[2], words = nodes * SPH_STATS_WORDS;
      std::vector<double> acc(words);
      const int64_t calls = ocl_solver->statsRead(0, 0, (int64_t)nodes, acc.data());
      if (calls != statsCalls) throw std::runtime_error("statistics: the slot's calls differ from the calls made");
      FILE* f = fopen(statsFile, "wb");
      const bool ok = f && fprintf(f, "sphmi stats calls %lld from %d every %d nx %d ny %d nz %d\n", (long long)calls, statsFrom, statsEvery,
                                   statsGrid.dims[0], statsGrid.dims[1], statsGrid.dims[2]) > 0 &&
                      fwrite(&statsGrid, sizeof(statsGrid), 1, f) == 1 && fwrite(acc.data(), sizeof(double), words, f) == words;
      if (!ok || fclose(f) != 0) throw std::runtime_error(std::string("cannot write ") + statsFile);
      printf("_stats: calls %lld nodes %zu\n", (long long)calls, nodes);
    }
    if (diagCsv && fclose(diagCsv) != 0) throw std::runtime_error(std::string("cannot write ") + diagFile);
    if (binCsv && fclose(binCsv) != 0) throw std::runtime_error(std::string("cannot write ") + binFile);
    if (compCsv && fclose(compCsv) != 0) throw std::runtime_error(std::string("cannot write ") + compFile);
    delete ocl_solver;
  } catch (std::exception& e) {  // owPhysicsFluidSimulator.cpp:73-76,144-148
    std::cout << "ERROR: " << e.what() << std::endl;
    exit(-1);
  }
  return 0;
}

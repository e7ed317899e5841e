"""Headless counterpart of the reference viewer's per-frame feed.

The GLUT viewer (owWorldSimulation.cpp:100-140, out of scope) pulls three things from the simulator every frame:
`getPosition_cpp()` (orig order), `getDensity_cpp()` (SORTED order) and `getParticleIndex_cpp()` ((cell, orig id) pairs in
sorted order), inverts the permutation itself (`p_indexb[2*p_indexb[2*i+1]] = i`) and colours particle i by
`density[p_indexb[2*i]]`. `frame()` does the same inversion and returns per-particle arrays in orig order; `density_colour()`
is the viewer's blue -> cyan -> green -> yellow -> red ramp over 0..5 % compression; `write_vtk` / `write_npz` replace the GL
window with files ParaView or numpy can open.

Field grids (owHIPSolver.sample_grid, float32[nz, ny, nx, 8] records: density, shepard, vx, vy, vz, pressure, count, 0):
`write_vtk_grid` writes one as a legacy-VTK volume beside the point cloud, `free_surface_height` turns one into a water-height
map (the dam-break gauge) and `read_fields` loads the raw files `sphmi_run --sample-grid` writes.

Surface meshes (owHIPSolver.extract_surface): `write_ply` / `read_ply` write and read binary little-endian PLY triangle meshes,
the format `sphmi_run --surface-out` writes, with vertex normals (owHIPSolver.surface_normals) when given.

Gradient grids (owHIPSolver.sample_gradient_grid, float32[nz, ny, nx, 32] records named by GRADIENT_FIELDS):
`write_vtk_gradients` writes vorticity, density gradient, divergence and Q as a legacy-VTK volume, and `read_gradients` loads
the raw files `sphmi_run --sample-gradients` writes.

Diagnostics (owHIPSolver.diagnostics, float64[R, 32] records named by DIAG_FIELDS): `diagnostics_summary` derives mass, centre
of mass, kinetic energy, density error and the like from one record, `write_diagnostics_csv` / `read_diagnostics_csv` write and
read the per-step table `sphmi_run --diagnostics-out` writes (every word as %.17g: a round trip keeps every bit).

Connected components (owHIPSolver.label_components / components / component_diagnostics): `component_summary` turns the table
into sizes and masses, `labels_in_original_order` maps the sorted-order labels to the particles' original order so that
`write_vtk` / `write_npz` can store a label beside each particle (`labels=`), and `write_components_csv` /
`read_components_csv` write and read the table `sphmi_run --components-out` writes.

Selections (owHIPSolver.select / selection, float32[n, 12] records named by SELECT_FIELDS): `write_vtk_selection` writes the
selected particles as a point cloud with everything a record holds as point data, `write_npz(selection=...)` stores one beside a
frame, and `write_selection` / `read_selection` write and read the files `sphmi_run --select-out` writes.

Elastic matter (owHIPSolver.elastic_measure / muscle_diagnostics / membrane_measure): `muscle_summary` turns the per-group records
(float64[G + 1, 16] named by MUSCLE_FIELDS) into mean length, rest length and strain per group, `write_muscles_csv` /
`read_muscles_csv` write and read the table `sphmi_run --elastic-out` writes, and `write_vtk_elastic` writes the elastic particles
as a point cloud with their strain record (ELASTIC_FIELDS) as point data.

Pictures (owHIPSolver.render / rendered): `look_at` makes the camera frame, `render_view` fills an SphRenderView that frames a
bounding box, `write_ppm` / `read_ppm` (binary P6) and `write_png` / `read_png` (8-bit RGBA, zlib from the standard library) store
the colour image, `thickness_in_scene_units` scales the thickness image; FIELD_RAMP and LABEL_PALETTE are the header's tables.

Integral curves (owHIPSolver.streamlines / tracers): `seed_rake` and `seed_plane` make seed points on a segment and on a plane,
`write_vtk_polylines` / `read_polylines` write and read the curves as legacy-VTK polylines with the speed as point data, the
format `sphmi_run --stream-out` writes.

Kinematic bodies (owHIPSolver.body_set_pose): `pose_identity`, `pose_translate`, `pose_rotate` and `pose_compose` build the
float32[3, 4] pose (R | t) in float64 and narrow it once; `piston` and `spin` return the pose of a wave-maker or a blade for a
step number, always relative to the body's reference placement.

Probes (owHIPSolver.probes_set_lines / probes_record / probe_history, level records named by LEVEL_FIELDS): `level_columns` makes one
level-probe line per column of a lattice, `level_heights` turns level records into the height map `free_surface_height` gives from
a whole grid, `probe_series` takes one word out of a history, `read_probes` loads the file `sphmi_run --probe-out` writes.

Time statistics (owHIPSolver.stats_define / stats_accumulate / stats, accumulators named by sphmi.STATS_FIELDS): `stats_moments`
restates the device's moment words in float64, `stats_summary` names what a flow is reported by (wet fraction, mean velocity,
stress tensor, TKE, pressure mean and rms, arrival call, peak pressure and its call), `write_vtk_stats` writes that as a VTK lattice,
`read_stats` loads the file `sphmi_run --stats-out` writes.

Binned diagnostics (owHIPSolver.bin_diagnostics / bin_index over a sphmi.bin_lattice, records named by DIAG_FIELDS): `bin_edges`
and `bin_boxes` restate the lattice's float32 edges and the bins' boxes (usable as diagnostics() regions), `bin_profile` gives
mass, mean velocity and mean density per bin, `bin_column_depth` the water depth of a plan-view map, `write_bins_csv` /
`read_bins` write and read the table `sphmi_run --bin-out` writes, `write_vtk_bins` writes the profile as VTK cell data.
"""
import math
import struct
import zlib

import numpy as np


def invert_particle_index(particle_index):
    """orig id -> sorted position, from the (cell, orig id) pairs the solver returns (owWorldSimulation.cpp:112-116)."""
    pi = np.asarray(particle_index, np.uint32).reshape(-1, 2)
    back = np.empty(pi.shape[0], np.uint32)
    back[pi[:, 1]] = np.arange(pi.shape[0], dtype=np.uint32)
    return back


def frame(simulator):
    """(position[N,4] in orig order, density[N] in orig order) of the simulator's current state."""
    pos = simulator.ocl_solver.read_position_buffer()
    rho_sorted = simulator.getDensity_cpp()
    back = invert_particle_index(simulator.getParticleIndex_cpp())
    return pos, rho_sorted[back]


def density_colour(rho, rho0):
    """RGB per particle exactly as display() picks it (owWorldSimulation.cpp:127-141): float arithmetic, later ramps win."""
    rho = np.clip(np.asarray(rho, np.float32), np.float32(0), np.float32(2) * np.float32(rho0))
    rho0 = np.float32(rho0)
    rgb = np.zeros((rho.shape[0], 3), np.float32)
    rgb[:, 2] = 1.0  # blue
    hundred = np.float32(100)
    ramps = ((1.00, lambda dc: (0 * dc, dc, 1 + 0 * dc)), (1.01, lambda dc: (0 * dc, 1 + 0 * dc, 1 - dc)),
             (1.02, lambda dc: (dc, 1 + 0 * dc, 0 * dc)), (1.03, lambda dc: (1 + 0 * dc, 1 - dc, 0 * dc)),
             (1.04, lambda dc: (1 + 0 * dc, 0 * dc, 0 * dc)))
    for factor, colour in ramps:
        dc = hundred * (rho - rho0 * np.float32(factor)) / rho0
        m = dc > 0
        r, g, b = colour(dc[m])
        rgb[m, 0], rgb[m, 1], rgb[m, 2] = r, g, b
    return rgb  # like glColor4f, components outside [0,1] are left to the consumer to clamp


def write_npz(path, position, density, step=None, labels=None, selection=None):
    """`labels`: optional component label per particle in orig order (labels_in_original_order), stored as int32 `component`.
    `selection`: optional (sorted_index, orig_id, records) of owHIPSolver.selection(), stored as `selection_index`,
    `selection_id` and `selection_records`."""
    extra = {} if labels is None else {"component": np.asarray(labels, np.int32)}
    if selection is not None:
        idx, ids, rec = selection
        extra.update(selection_index=np.asarray(idx, np.int32), selection_id=np.asarray(ids, np.uint32),
                     selection_records=np.asarray(rec, np.float32).reshape(-1, len(SELECT_FIELDS)))
    np.savez_compressed(path, position=np.asarray(position, np.float32), density=np.asarray(density, np.float32),
                        step=np.int64(-1 if step is None else step), **extra)


def write_vtk(path, position, density, include_boundary=False, labels=None):
    """Legacy-VTK polydata (binary, big-endian): points + `density` and `type` point scalars, and `component` (int) when
    `labels` (one per particle, orig order: labels_in_original_order) is given."""
    pos = np.asarray(position, np.float32).reshape(-1, 4)
    rho = np.asarray(density, np.float32)
    lab = None if labels is None else np.asarray(labels, np.int32).reshape(-1)
    if lab is not None and lab.shape[0] != pos.shape[0]:
        raise ValueError("labels must hold one entry per particle")
    if not include_boundary:
        keep = pos[:, 3].astype(np.int32) != 3  # BOUNDARY_PARTICLE (owOpenCLConstant.h:12)
        pos, rho = pos[keep], rho[keep]
        lab = None if lab is None else lab[keep]
    n = pos.shape[0]
    with open(path, "wb") as f:
        f.write(b"# vtk DataFile Version 3.0\nsphmi frame\nBINARY\nDATASET POLYDATA\n")
        f.write(("POINTS %d float\n" % n).encode())
        f.write(pos[:, :3].astype(">f4").tobytes())
        f.write(("\nVERTICES %d %d\n" % (n, 2 * n)).encode())
        cells = np.empty((n, 2), ">i4")
        cells[:, 0] = 1
        cells[:, 1] = np.arange(n)
        f.write(cells.tobytes())
        f.write(("\nPOINT_DATA %d\nSCALARS density float 1\nLOOKUP_TABLE default\n" % n).encode())
        f.write(rho.astype(">f4").tobytes())
        f.write(b"\nSCALARS type float 1\nLOOKUP_TABLE default\n")
        f.write(pos[:, 3].astype(">f4").tobytes())
        f.write(b"\n")
        if lab is not None:
            f.write(b"SCALARS component int 1\nLOOKUP_TABLE default\n")
            f.write(lab.astype(">i4").tobytes())
            f.write(b"\n")
    return n


GRID_FIELDS = ("density", "shepard", "vx", "vy", "vz", "pressure", "count")
# the 32 words of a sph_sample_gradient_* record (include/sphmi.h); gradients are per metre of simulation-scaled space
GRADIENT_FIELDS = GRID_FIELDS + ("unused7",) + \
    tuple("d%s_d%s" % (f, c) for f in ("rho", "shepard", "vx", "vy", "vz", "p") for c in "xyz") + \
    ("vorticity_x", "vorticity_y", "vorticity_z", "divergence", "q_criterion", "unused31")


def write_vtk_grid(path, origin, spacing, fields):
    """Legacy-VTK STRUCTURED_POINTS (binary, big-endian like write_vtk) of a sample_grid result `fields` [nz, ny, nx, 8]:
    point data `density`, `shepard`, `pressure` (scalars) and `velocity` (vectors)."""
    g = np.asarray(fields, np.float32)
    if g.ndim != 4 or g.shape[3] < 6:
        raise ValueError("fields must be [nz, ny, nx, 8] records")
    nz, ny, nx = g.shape[:3]
    n = nx * ny * nz
    o = [float(np.float32(v)) for v in origin]
    sp = [float(np.float32(v)) for v in spacing]
    with open(path, "wb") as f:
        f.write(b"# vtk DataFile Version 3.0\nsphmi fields\nBINARY\nDATASET STRUCTURED_POINTS\n")
        f.write(("DIMENSIONS %d %d %d\n" % (nx, ny, nz)).encode())
        f.write(("ORIGIN %.9g %.9g %.9g\n" % tuple(o)).encode())
        f.write(("SPACING %.9g %.9g %.9g\n" % tuple(sp)).encode())
        f.write(("POINT_DATA %d\n" % n).encode())
        for name, col in (("density", 0), ("shepard", 1), ("pressure", 5)):
            f.write(("SCALARS %s float 1\nLOOKUP_TABLE default\n" % name).encode())
            f.write(np.ascontiguousarray(g[..., col]).astype(">f4").tobytes())
            f.write(b"\n")
        f.write(b"VECTORS velocity float\n")
        f.write(np.ascontiguousarray(g[..., 2:5]).astype(">f4").tobytes())
        f.write(b"\n")
    return n


def free_surface_height(grid, origin, spacing, threshold=0.5):
    """Water height per (y, x) column of a sample_grid result [nz, ny, nx, 8]: the highest z at which `shepard` (the fraction of
    space the fluid fills, ~1 inside) falls from >= threshold to < threshold between two grid planes, interpolated linearly
    between them. A column whose top plane is still >= threshold gives the top plane's z; one that never reaches the
    threshold gives NaN. float64 [ny, nx]."""
    g = np.asarray(grid, np.float32)
    s = g[..., 1].astype(np.float64)  # [nz, ny, nx]
    nz = s.shape[0]
    z = float(np.float32(origin[2])) + np.arange(nz, dtype=np.float64) * float(np.float32(spacing[2]))
    thr = float(threshold)
    above = s >= thr
    out = np.full(s.shape[1:], np.nan)
    top = above[-1]
    out[top] = z[-1]
    if nz > 1:
        cross = above[:-1] & ~above[1:]  # plane k >= thr, plane k+1 below
        has = cross.any(axis=0) & ~top
        k = (nz - 2) - np.argmax(cross[::-1], axis=0)  # highest crossing per column
        yy, xx = np.nonzero(has)
        kk = k[yy, xx]
        s0, s1 = s[kk, yy, xx], s[kk + 1, yy, xx]
        out[yy, xx] = z[kk] + (s0 - thr) / (s0 - s1) * (z[kk + 1] - z[kk])
    return out


def read_fields(path, dims):
    """A `sphmi_run --sample-grid NX NY NZ` output file (raw float32 records in sph_sample_grid's layout) as [NZ, NY, NX, 8]."""
    nx, ny, nz = (int(v) for v in dims)
    return np.fromfile(path, np.float32).reshape(nz, ny, nx, 8)


def write_ply(path, vertices, triangles, normals=None):
    """Binary little-endian PLY of a triangle mesh (extract_surface): `float x y z` per vertex (then `float nx ny nz` when
    `normals` [V, 3] is given, e.g. surface_normals()), `list uchar int vertex_indices` per face. ParaView, Blender and
    MeshLab read it."""
    v = np.ascontiguousarray(vertices, "<f4").reshape(-1, 3)
    t = np.ascontiguousarray(triangles, "<i4").reshape(-1, 3)
    nprops = ""
    if normals is not None:
        n = np.asarray(normals, "<f4").reshape(-1, 3)
        if n.shape != v.shape:
            raise ValueError("normals must be [V, 3] like the vertices")
        v = np.ascontiguousarray(np.concatenate([v, n], axis=1))
        nprops = "property float nx\nproperty float ny\nproperty float nz\n"
    faces = np.empty(t.shape[0], dtype=[("n", "u1"), ("i", "<i4", (3,))])
    faces["n"] = 3
    faces["i"] = t
    with open(path, "wb") as f:
        f.write(("ply\nformat binary_little_endian 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\n%s"
                 "element face %d\nproperty list uchar int vertex_indices\nend_header\n" % (v.shape[0], nprops, t.shape[0])).encode())
        f.write(v.tobytes())
        f.write(faces.tobytes())
    return v.shape[0], t.shape[0]


def read_ply(path, with_normals=False):
    """(vertices float32[V, 3], triangles int32[T, 3]) of a binary little-endian triangle PLY as write_ply (and sphmi_run
    --surface-out) write it. with_normals=True adds a third item: the `nx ny nz` vertex properties as float32[V, 3], or
    None when the file has none."""
    with open(path, "rb") as f:
        data = f.read()
    end = data.index(b"end_header\n") + len(b"end_header\n")
    header = data[:end].decode("ascii").split("\n")
    if header[0] != "ply" or header[1] != "format binary_little_endian 1.0":
        raise ValueError("%s: not a binary little-endian PLY" % path)
    counts, vprops, face_prop = {}, [], None
    element = None
    for line in header[2:]:
        w = line.split()
        if not w or w[0] in ("comment", "obj_info", "end_header"):
            continue
        if w[0] == "element":
            element = w[1]
            counts[element] = int(w[2])
        elif w[0] == "property" and element == "vertex":
            if w[1] not in ("float", "float32"):
                raise ValueError("%s: vertex property %s is not float" % (path, w[2]))
            vprops.append(w[2])
        elif w[0] == "property" and element == "face":
            face_prop = w[1:]
    if vprops[:3] != ["x", "y", "z"] or face_prop is None or face_prop[:3] not in (["list", "uchar", "int"], ["list", "uint8", "int32"]):
        raise ValueError("%s: expected float x y z vertices and list uchar int faces" % path)
    nv, nf = counts.get("vertex", 0), counts.get("face", 0)
    vert = np.frombuffer(data, "<f4", nv * len(vprops), end).reshape(nv, len(vprops))[:, :3]
    faces = np.frombuffer(data, [("n", "u1"), ("i", "<i4", (3,))], nf, end + 4 * nv * len(vprops))
    if nf and (faces["n"] != 3).any():
        raise ValueError("%s: faces must be triangles" % path)
    v, t = np.array(vert, np.float32), np.array(faces["i"], np.int32).reshape(nf, 3)
    if not with_normals:
        return v, t
    normals = None
    if all(c in vprops for c in ("nx", "ny", "nz")):
        allv = np.frombuffer(data, "<f4", nv * len(vprops), end).reshape(nv, len(vprops))
        normals = np.array(allv[:, [vprops.index(c) for c in ("nx", "ny", "nz")]], np.float32)
    return v, t, normals


def write_vtk_gradients(path, origin, spacing, records):
    """Legacy-VTK STRUCTURED_POINTS (binary, big-endian like write_vtk_grid) of a sample_gradient_grid result `records`
    [nz, ny, nx, 32]: point data `vorticity` and `density_gradient` (vectors), `divergence` and `q_criterion` (scalars)."""
    g = np.asarray(records, np.float32)
    if g.ndim != 4 or g.shape[3] != len(GRADIENT_FIELDS):
        raise ValueError("records must be [nz, ny, nx, 32]")
    nz, ny, nx = g.shape[:3]
    n = nx * ny * nz
    o = [float(np.float32(v)) for v in origin]
    sp = [float(np.float32(v)) for v in spacing]
    w = GRADIENT_FIELDS.index
    with open(path, "wb") as f:
        f.write(b"# vtk DataFile Version 3.0\nsphmi gradients\nBINARY\nDATASET STRUCTURED_POINTS\n")
        f.write(("DIMENSIONS %d %d %d\n" % (nx, ny, nz)).encode())
        f.write(("ORIGIN %.9g %.9g %.9g\n" % tuple(o)).encode())
        f.write(("SPACING %.9g %.9g %.9g\n" % tuple(sp)).encode())
        f.write(("POINT_DATA %d\n" % n).encode())
        for name, first in (("vorticity", w("vorticity_x")), ("density_gradient", w("drho_dx"))):
            f.write(("VECTORS %s float\n" % name).encode())
            f.write(np.ascontiguousarray(g[..., first:first + 3]).astype(">f4").tobytes())
            f.write(b"\n")
        for name in ("divergence", "q_criterion"):
            f.write(("SCALARS %s float 1\nLOOKUP_TABLE default\n" % name).encode())
            f.write(np.ascontiguousarray(g[..., w(name)]).astype(">f4").tobytes())
            f.write(b"\n")
    return n


def read_gradients(path, dims):
    """A `sphmi_run --sample-gradients` output file (raw float32 records in sph_sample_gradient_grid's layout) as
    [NZ, NY, NX, 32]."""
    nx, ny, nz = (int(v) for v in dims)
    return np.fromfile(path, np.float32).reshape(nz, ny, nx, len(GRADIENT_FIELDS))


# ---- flow diagnostics (owHIPSolver.diagnostics; include/sphmi.h, sph_diagnostics) ----
DIAG_FIELDS = ("n", "sum_x", "sum_y", "sum_z", "sum_vx", "sum_vy", "sum_vz", "sum_lx", "sum_ly", "sum_lz", "sum_v2", "sum_rho",
               "sum_e2", "sum_p", "reserved14", "reserved15", "min_rho", "max_rho", "min_p", "max_p", "max_v2", "max_v2_index",
               "max_v2_id", "min_x", "min_y", "min_z", "max_x", "max_y", "max_z", "reserved29", "reserved30", "reserved31")


def diagnostics_summary(record, cfg):
    """Physical numbers (Python floats, computed in double) from one 32-word diagnostics record: mass = n * cfg.mass, centre of
    mass and mean velocity (scene units, as positions and velocities are stored), kinetic energy 0.5 * mass-per-particle * sum v2,
    linear and angular momentum, max speed, mean / min / max density, rms and max relative density error against cfg.rho0, mean
    pressure and the bounding box. With n = 0 the means are 0."""
    r = np.asarray(record, np.float64).reshape(-1)
    if r.size != len(DIAG_FIELDS):
        raise ValueError("diagnostics_summary: a record has %d words" % len(DIAG_FIELDS))
    n = float(r[0])
    m = float(cfg.mass)
    rho0 = float(cfg.rho0)
    def mean(x):
        return float(x) / n if n > 0 else 0.0
    return dict(
        n=int(n), mass=n * m,
        centre_of_mass=tuple(mean(x) for x in r[1:4]),
        mean_velocity=tuple(mean(x) for x in r[4:7]),
        momentum=tuple(m * float(x) for x in r[4:7]),
        angular_momentum=tuple(m * float(x) for x in r[7:10]),
        kinetic_energy=0.5 * m * float(r[10]),
        max_speed=float(np.sqrt(r[20])), max_speed_index=int(r[21]), max_speed_id=int(r[22]),
        mean_density=mean(r[11]), min_density=float(r[16]), max_density=float(r[17]),
        rms_density_error=float(np.sqrt(mean(r[12]))) / rho0,
        max_density_error=(max(abs(float(r[16]) - rho0), abs(float(r[17]) - rho0)) / rho0) if n > 0 else 0.0,
        mean_pressure=mean(r[13]), min_pressure=float(r[18]), max_pressure=float(r[19]),
        bbox_min=tuple(float(x) for x in r[23:26]), bbox_max=tuple(float(x) for x in r[26:29]))


def write_diagnostics_csv(path, steps, records):
    """One row per step and region: `step,region,` then the 32 record words as %.17g, under a header naming them. `steps`: S step
    numbers; `records`: float64[S, R, 32] (or [S, 32] for one region)."""
    rec = np.asarray(records, np.float64)
    if rec.ndim == 2:
        rec = rec[:, None, :]
    if rec.ndim != 3 or rec.shape[2] != len(DIAG_FIELDS) or rec.shape[0] != len(steps):
        raise ValueError("write_diagnostics_csv: records must be [len(steps), R, %d]" % len(DIAG_FIELDS))
    with open(path, "w") as f:
        f.write("step,region," + ",".join(DIAG_FIELDS) + "\n")
        for s, block in zip(steps, rec):
            for r, row in enumerate(block):
                f.write("%d,%d," % (int(s), r) + ",".join("%.17g" % float(x) for x in row) + "\n")


def read_diagnostics_csv(path):
    """(steps int64[S], records float64[S, R, 32]) of a file written by write_diagnostics_csv or `sphmi_run --diagnostics-out`."""
    with open(path) as f:
        header = f.readline().strip().split(",")
        if header != ["step", "region"] + list(DIAG_FIELDS):
            raise ValueError("%s: not a diagnostics table" % path)
        rows = [line.strip().split(",") for line in f if line.strip()]
    if not rows:
        return np.zeros(0, np.int64), np.zeros((0, 0, len(DIAG_FIELDS)), np.float64)
    steps, regions = [int(r[0]) for r in rows], [int(r[1]) for r in rows]
    R = max(regions) + 1
    if len(rows) % R or regions != list(range(R)) * (len(rows) // R):
        raise ValueError("%s: rows are not grouped as one block of regions per step" % path)
    rec = np.array([[float(x) for x in r[2:]] for r in rows], np.float64).reshape(-1, R, len(DIAG_FIELDS))
    return np.array(steps[::R], np.int64), rec


# ---- connected components (owHIPSolver.label_components / components / component_diagnostics; include/sphmi.h) ----
COMPONENT_FIELDS = ("root", "n", "min_x", "min_y", "min_z", "max_x", "max_y", "max_z")


def component_summary(root_count, bbox, mass):
    """Sizes of a labelling from its table: number of components, the largest one (lowest id among equals) and its size, the
    component ids by descending size (then ascending id), the sizes in that order, the particles outside the largest one and
    the mass per component id (n * mass, float64)."""
    rc = np.asarray(root_count, np.int64).reshape(-1, 2)
    bb = np.asarray(bbox, np.float32).reshape(-1, 6)
    if bb.shape[0] != rc.shape[0]:
        raise ValueError("component_summary: root_count and bbox must have one row per component")
    n = rc[:, 1]
    order = np.lexsort((np.arange(n.size), -n))
    largest = int(order[0]) if n.size else -1
    return dict(components=int(n.size), largest=largest, largest_n=int(n[largest]) if n.size else 0, order=order,
                sizes=n[order], outside_largest=int(n.sum() - (n[largest] if n.size else 0)), mass=n.astype(np.float64) * float(mass),
                largest_bbox=tuple(float(x) for x in bb[largest]) if n.size else None)


def labels_in_original_order(labels, particle_index):
    """Component label per particle in ORIG order from the sorted-order labels and the (cell, orig id) pairs of
    read_particleIndex_buffer taken in the same step: out[orig id] = labels[sorted position] (invert_particle_index)."""
    lab = np.asarray(labels, np.int32).reshape(-1)
    back = invert_particle_index(particle_index)
    if back.shape[0] != lab.shape[0]:
        raise ValueError("labels_in_original_order: one label per particle expected")
    return lab[back]


def write_components_csv(path, steps, ids, root_count, bbox, records):
    """One row per report and component: `step,component,root,n,` the bounding box as %.9g (float32 round trip) and the 32 words
    of the component's diagnostics record as %.17g. steps[k] goes with ids[k] (component ids), root_count[k] [R, 2], bbox[k]
    [R, 6] and records[k] [R, 32]; R may differ from report to report."""
    with open(path, "w") as f:
        f.write("step,component," + ",".join(COMPONENT_FIELDS) + "," + ",".join(DIAG_FIELDS) + "\n")
        for k, step in enumerate(steps):
            rc = np.asarray(root_count[k], np.int64).reshape(-1, 2)
            bb = np.asarray(bbox[k], np.float32).reshape(-1, 6)
            rec = np.asarray(records[k], np.float64).reshape(-1, len(DIAG_FIELDS))
            cid = np.asarray(ids[k], np.int64).reshape(-1)
            if not (rc.shape[0] == bb.shape[0] == rec.shape[0] == cid.shape[0]):
                raise ValueError("write_components_csv: report %d has rows of different lengths" % k)
            for r in range(cid.shape[0]):
                f.write("%d,%d,%d,%d," % (int(step), cid[r], rc[r, 0], rc[r, 1]) + ",".join("%.9g" % float(x) for x in bb[r]) + "," +
                        ",".join("%.17g" % float(x) for x in rec[r]) + "\n")


def read_components_csv(path):
    """The rows of a file written by write_components_csv or `sphmi_run --components-out`, in file order:
    (steps int64[K], ids int64[K], root_count int32[K, 2], bbox float32[K, 6], records float64[K, 32])."""
    with open(path) as f:
        header = f.readline().strip().split(",")
        if header != ["step", "component"] + list(COMPONENT_FIELDS) + list(DIAG_FIELDS):
            raise ValueError("%s: not a components table" % path)
        rows = [line.strip().split(",") for line in f if line.strip()]
    K = len(rows)
    steps = np.array([int(r[0]) for r in rows], np.int64)
    ids = np.array([int(r[1]) for r in rows], np.int64)
    rc = np.array([[int(r[2]), int(r[3])] for r in rows], np.int32).reshape(K, 2)
    bb = np.array([[float(x) for x in r[4:10]] for r in rows], np.float64).astype(np.float32).reshape(K, 6)
    rec = np.array([[float(x) for x in r[10:]] for r in rows], np.float64).reshape(K, len(DIAG_FIELDS))
    return steps, ids, rc, bb, rec


# ---- surface measures (owHIPSolver.measure_surface / surface_shells; include/sphmi.h, sph_measure_surface) ----
SHELL_FIELDS = ("root", "vertices", "triangles", "open", "bad", "a2", "d6", "mx", "my", "mz")
SHELL_BBOX_FIELDS = COMPONENT_FIELDS[2:]
SHELL_KINDS = ("drop", "cavity", "open")


def _shell_value(total, k):
    """ldexp((double)sum, -k) of an exact integer sum."""
    return float(np.ldexp(np.float64(int(total)), -int(k)))


def shell_summary(table, exps, origin):
    """Physical numbers from the table of surface_shells() and the exponents (kA, kV, kM) of measure_surface(); `origin` is the
    origin of the lattice the mesh was extracted on. Per shell (arrays of length S): area, volume (signed: negative for a
    cavity; meaningful for closed shells), centroid float64[S, 3] of the area in scene coordinates (NaN for a shell without
    area), chi (Euler characteristic), genus (closed shells, else -1), closed, kind (an index into SHELL_KINDS: drop, cavity,
    open) and radius (of the sphere with the shell's |volume|). "totals": the whole mesh from the exact integer column sums
    (shells, closed, vertices, triangles, open, bad, area, volume, centroid)."""
    t = np.asarray(table, np.int64).reshape(-1, len(SHELL_FIELDS))
    kA, kV, kM = (int(x) for x in np.asarray(exps).reshape(3))
    o = np.asarray(origin, np.float32).astype(np.float64).reshape(3)
    S = t.shape[0]
    a2 = np.ldexp(t[:, 5].astype(np.float64), -kA)
    d6 = np.ldexp(t[:, 6].astype(np.float64), -kV)
    m = np.ldexp(t[:, 7:10].astype(np.float64), -kM)
    with np.errstate(divide="ignore", invalid="ignore"):
        centroid = o[None, :] + m / (3.0 * a2[:, None])
    closed = t[:, 3] == 0
    twice_edges = 3 * t[:, 2] + t[:, 3]
    chi = t[:, 1] - twice_edges // 2 + t[:, 2]
    genus = np.where(closed & (chi % 2 == 0), (2 - chi) // 2, -1)
    volume = d6 / 6.0
    kind = np.where(~closed, 2, np.where(volume < 0, 1, 0)).astype(np.int32)
    cols = [sum(int(x) for x in t[:, c]) for c in range(len(SHELL_FIELDS))]  # exact, whatever the number of shells
    ta2 = _shell_value(cols[5], kA)
    tm = np.array([_shell_value(cols[7 + c], kM) for c in range(3)])
    with np.errstate(divide="ignore", invalid="ignore"):
        tc = o + tm / (3.0 * ta2)
    totals = dict(shells=S, closed=int(closed.sum()), vertices=cols[1], triangles=cols[2], open=cols[3], bad=cols[4],
                  area=ta2 / 2.0, volume=_shell_value(cols[6], kV) / 6.0, centroid=tc)
    return dict(area=a2 / 2.0, volume=volume, centroid=centroid, chi=chi, genus=genus, closed=closed, kind=kind,
                radius=np.cbrt(3.0 * np.abs(volume) / (4.0 * np.pi)), totals=totals)


def write_shells_csv(path, table, bbox, exps):
    """The table of surface_shells() as text, lossless: a line `# exps kA kV kM`, a header, then one row per shell: its number,
    the ten int64 words and the bounding box as %.9g (float32 round trip). `sphmi_run --surface-shells` writes the same file."""
    t = np.asarray(table, np.int64).reshape(-1, len(SHELL_FIELDS))
    bb = np.asarray(bbox, np.float32).reshape(-1, 6)
    if bb.shape[0] != t.shape[0]:
        raise ValueError("write_shells_csv: table and bbox must have one row per shell")
    with open(path, "w") as f:
        f.write("# exps %d %d %d\n" % tuple(int(x) for x in np.asarray(exps).reshape(3)))
        f.write("shell," + ",".join(SHELL_FIELDS) + "," + ",".join(SHELL_BBOX_FIELDS) + "\n")
        for r in range(t.shape[0]):
            f.write("%d," % r + ",".join("%d" % int(x) for x in t[r]) + "," + ",".join("%.9g" % float(x) for x in bb[r]) + "\n")


def read_shells(path):
    """(table int64[S, 10], bbox float32[S, 6], exps int32[3]) of a file written by write_shells_csv or `sphmi_run
    --surface-shells`."""
    with open(path) as f:
        first = f.readline().split()
        header = f.readline().strip().split(",")
        if first[:2] != ["#", "exps"] or len(first) != 5 or header != ["shell"] + list(SHELL_FIELDS) + list(SHELL_BBOX_FIELDS):
            raise ValueError("%s: not a shells table" % path)
        rows = [line.strip().split(",") for line in f if line.strip()]
    S = len(rows)
    if [int(r[0]) for r in rows] != list(range(S)):
        raise ValueError("%s: shells out of order" % path)
    table = np.array([[int(x) for x in r[1:11]] for r in rows], np.int64).reshape(S, len(SHELL_FIELDS))
    bb = np.array([[float(x) for x in r[11:17]] for r in rows], np.float64).astype(np.float32).reshape(S, 6)
    return table, bb, np.array([int(x) for x in first[2:]], np.int32)


# ---- particle selection (owHIPSolver.select / selection; include/sphmi.h, sph_select_particles) ----
SELECT_FIELDS = ("x", "y", "z", "type", "vx", "vy", "vz", "density", "pressure", "neighbors", "surface", "unused11")


def write_vtk_selection(path, records, orig_id):
    """Legacy-VTK polydata (binary, big-endian like write_vtk) of a selection: one point per record with `type`, `density`,
    `pressure`, `neighbors`, `surface` (float scalars), `id` (int, the original particle id) and `velocity` (vectors)."""
    rec = np.asarray(records, np.float32).reshape(-1, len(SELECT_FIELDS))
    ids = np.asarray(orig_id, np.uint32).reshape(-1)
    if ids.shape[0] != rec.shape[0]:
        raise ValueError("write_vtk_selection: one id per record expected")
    n = rec.shape[0]
    w = SELECT_FIELDS.index
    with open(path, "wb") as f:
        f.write(b"# vtk DataFile Version 3.0\nsphmi selection\nBINARY\nDATASET POLYDATA\n")
        f.write(("POINTS %d float\n" % n).encode())
        f.write(rec[:, :3].astype(">f4").tobytes())
        f.write(("\nVERTICES %d %d\n" % (n, 2 * n)).encode())
        cells = np.empty((n, 2), ">i4")
        cells[:, 0] = 1
        cells[:, 1] = np.arange(n)
        f.write(cells.tobytes())
        f.write(("\nPOINT_DATA %d\n" % n).encode())
        for name in ("type", "density", "pressure", "neighbors", "surface"):
            f.write(("SCALARS %s float 1\nLOOKUP_TABLE default\n" % name).encode())
            f.write(np.ascontiguousarray(rec[:, w(name)]).astype(">f4").tobytes())
            f.write(b"\n")
        f.write(b"SCALARS id int 1\nLOOKUP_TABLE default\n")
        f.write(ids.astype(">i4").tobytes())
        f.write(b"\nVECTORS velocity float\n")
        f.write(np.ascontiguousarray(rec[:, w("vx"):w("vz") + 1]).astype(">f4").tobytes())
        f.write(b"\n")
    return n


def write_selection(path, sorted_index, orig_id, records):
    """The file `sphmi_run --select-out` writes, little-endian: the count n as int64, then n int32 sorted indices, n uint32
    original ids and n x 12 float32 records."""
    idx = np.ascontiguousarray(sorted_index, "<i4").reshape(-1)
    ids = np.ascontiguousarray(orig_id, "<u4").reshape(-1)
    rec = np.ascontiguousarray(records, "<f4").reshape(-1, len(SELECT_FIELDS))
    if not (idx.shape[0] == ids.shape[0] == rec.shape[0]):
        raise ValueError("write_selection: the three arrays must have one entry per selected particle")
    with open(path, "wb") as f:
        f.write(np.array([idx.shape[0]], "<i8").tobytes())
        f.write(idx.tobytes())
        f.write(ids.tobytes())
        f.write(rec.tobytes())
    return idx.shape[0]


def read_selection(path):
    """(sorted_index int32[n], orig_id uint32[n], records float32[n, 12]) of a file written by write_selection or
    `sphmi_run --select-out`."""
    with open(path, "rb") as f:
        data = f.read()
    if len(data) < 8:
        raise ValueError("%s: not a selection file" % path)
    n = int(np.frombuffer(data, "<i8", 1, 0)[0])
    W = len(SELECT_FIELDS)
    if n < 0 or len(data) != 8 + n * (8 + 4 * W):
        raise ValueError("%s: %d bytes do not hold %d selected particles" % (path, len(data), n))
    idx = np.frombuffer(data, "<i4", n, 8).astype(np.int32)
    ids = np.frombuffer(data, "<u4", n, 8 + 4 * n).astype(np.uint32)
    rec = np.frombuffer(data, "<f4", n * W, 8 + 8 * n).astype(np.float32).reshape(n, W)
    return idx, ids, rec


# ---- elastic-matter diagnostics (owHIPSolver.elastic_measure / muscle_diagnostics / membrane_measure; include/sphmi.h) ----
ELASTIC_FIELDS = ("n", "n_muscle", "min_strain", "max_strain", "sum_strain", "sum_dr2", "spring_x", "spring_y", "spring_z",
                  "contraction_x", "contraction_y", "contraction_z")
MUSCLE_FIELDS = ("n", "signal", "sum_rest_length", "sum_length", "sum_dr", "sum_dr2", "sum_strain", "min_strain", "max_strain",
                 "sum_spring", "sum_contraction", "sum_x", "sum_y", "sum_z", "n_zero_length", "reserved15")
MEMBRANE_FIELDS = ("area", "normal_x", "normal_y", "normal_z", "centroid_x", "centroid_y", "centroid_z", "unused7")
MUSCLE_SUMMARY_FIELDS = ("group", "n", "signal", "mean_length", "mean_rest_length", "mean_strain", "min_strain", "max_strain")


def muscle_summary(records):
    """float64[G + 1, 8] from muscle_diagnostics() records, one row per group named by MUSCLE_SUMMARY_FIELDS: group (0 = the
    connections of no muscle), n, signal, mean length sum_length / n, mean rest length, mean strain, min and max strain. Lengths
    are simulation-scaled (the units of the connection table's rest lengths). The quotients are IEEE double divisions of the
    record's words; with n = 0 they are 0."""
    r = np.asarray(records, np.float64).reshape(-1, len(MUSCLE_FIELDS))
    out = np.zeros((r.shape[0], len(MUSCLE_SUMMARY_FIELDS)), np.float64)
    n = r[:, 0]
    has = n > 0
    out[:, 0] = np.arange(r.shape[0])
    out[:, 1], out[:, 2] = n, r[:, 1]
    for col, word in ((3, 3), (4, 2), (5, 6)):
        out[has, col] = r[has, word] / n[has]
    out[:, 6], out[:, 7] = r[:, 7], r[:, 8]
    return out


def write_muscles_csv(path, records):
    """The table `sphmi_run --elastic-out` writes: one row per group, muscle_summary's columns, every number as %.17g."""
    rows = muscle_summary(records)
    with open(path, "w") as f:
        f.write(",".join(MUSCLE_SUMMARY_FIELDS) + "\n")
        for row in rows:
            f.write("%d,%d," % (int(row[0]), int(row[1])) + ",".join("%.17g" % float(x) for x in row[2:]) + "\n")
    return rows.shape[0]


def read_muscles_csv(path):
    """float64[G + 1, 8] of a file written by write_muscles_csv or `sphmi_run --elastic-out`."""
    with open(path) as f:
        header = f.readline().strip().split(",")
        if header != list(MUSCLE_SUMMARY_FIELDS):
            raise ValueError("%s: not a muscle table" % path)
        rows = [[float(x) for x in line.strip().split(",")] for line in f if line.strip()]
    return np.array(rows, np.float64).reshape(-1, len(MUSCLE_SUMMARY_FIELDS))


def write_vtk_elastic(path, position, orig_id, records):
    """Legacy-VTK polydata (binary, big-endian like write_vtk) of the elastic particles: one point per row of
    owHIPSolver.elastic_measure() at position[orig_id] (`position`: [N, 4] in orig order, e.g. read_position_buffer()), with
    `connections`, `muscle_connections`, `min_strain`, `max_strain`, `mean_strain` (float scalars), `id` (int) and
    `spring_acceleration`, `contraction_acceleration` (vectors) as point data."""
    rec = np.asarray(records, np.float32).reshape(-1, len(ELASTIC_FIELDS))
    ids = np.asarray(orig_id, np.uint32).reshape(-1)
    if ids.shape[0] != rec.shape[0]:
        raise ValueError("write_vtk_elastic: one id per record expected")
    pos = np.asarray(position, np.float32).reshape(-1, 4)[ids.astype(np.int64), :3]
    n = rec.shape[0]
    w = ELASTIC_FIELDS.index
    live = np.maximum(rec[:, w("n")], np.float32(1))
    scalars = (("connections", rec[:, w("n")]), ("muscle_connections", rec[:, w("n_muscle")]), ("min_strain", rec[:, w("min_strain")]),
               ("max_strain", rec[:, w("max_strain")]), ("mean_strain", rec[:, w("sum_strain")] / live))
    with open(path, "wb") as f:
        f.write(b"# vtk DataFile Version 3.0\nsphmi elastic matter\nBINARY\nDATASET POLYDATA\n")
        f.write(("POINTS %d float\n" % n).encode())
        f.write(pos.astype(">f4").tobytes())
        f.write(("\nVERTICES %d %d\n" % (n, 2 * n)).encode())
        cells = np.empty((n, 2), ">i4")
        cells[:, 0] = 1
        cells[:, 1] = np.arange(n)
        f.write(cells.tobytes())
        f.write(("\nPOINT_DATA %d\n" % n).encode())
        for name, col in scalars:
            f.write(("SCALARS %s float 1\nLOOKUP_TABLE default\n" % name).encode())
            f.write(np.ascontiguousarray(col).astype(">f4").tobytes())
            f.write(b"\n")
        f.write(b"SCALARS id int 1\nLOOKUP_TABLE default\n")
        f.write(ids.astype(">i4").tobytes())
        for name, first in (("spring_acceleration", w("spring_x")), ("contraction_acceleration", w("contraction_x"))):
            f.write(("\nVECTORS %s float\n" % name).encode())
            f.write(np.ascontiguousarray(rec[:, first:first + 3]).astype(">f4").tobytes())
        f.write(b"\n")
    return n


# ---- force decomposition (owHIPSolver.force_measure / force_diagnostics; include/sphmi.h, sph_force_measure) ----
FORCE_CLASSES = ("liquid", "elastic", "boundary")  # class 1, 2, 3 of the neighbour that exerts the term
_FORCE_KINDS = ("viscous", "tension", "pressure")
FORCE_FIELDS = tuple("%s_%s_%s" % (c, k, a) for c in FORCE_CLASSES for k in _FORCE_KINDS for a in "xyz") + \
    tuple("n_" + c for c in FORCE_CLASSES) + ("step_x", "step_y", "step_z", "step_pressure_x", "step_pressure_y", "step_pressure_z") + \
    ("unused36", "unused37", "unused38", "unused39")
FORCE_DIAG_FIELDS = ("n",) + tuple("sum_" + f for f in FORCE_FIELDS[:27]) + tuple("sum_" + f for f in FORCE_FIELDS[30:36]) + \
    tuple("sum_torque_%s_%s" % (c, a) for c in FORCE_CLASSES for a in "xyz") + tuple("sum_power_" + c for c in FORCE_CLASSES) + \
    tuple("sum_n_" + c for c in FORCE_CLASSES) + tuple("reserved%d" % w for w in range(49, 64))


def force_summary(record, mass):
    """A force_diagnostics() record as physical numbers, a dict of float64 values: the record's sums are accelerations, `mass`
    (cfg.mass, kg per particle) times them are newtons. n; viscous, tension, pressure and load = (viscous + pressure) + tension
    per class as [3, 3] arrays (rows liquid, elastic, boundary: what that class exerts on the selected particles); hydrodynamic =
    the liquid's row of load (thrust and drag on a selected body); torque [3, 3] about the origin in newton x scene unit; power
    [3] in watts; neighbors [3], the summed neighbour counts; step = mass x (sum of the step's own viscous + gravity + tension
    acceleration + sum of its pressure acceleration)."""
    r = np.asarray(record, np.float64).reshape(len(FORCE_DIAG_FIELDS))
    m = float(mass)
    per = r[1:28].reshape(3, 3, 3)  # class, kind, axis
    out = {"n": r[0], "viscous": m * per[:, 0], "tension": m * per[:, 1], "pressure": m * per[:, 2]}
    out["load"] = (out["viscous"] + out["pressure"]) + out["tension"]
    out["hydrodynamic"] = out["load"][0].copy()
    out["torque"] = m * r[34:43].reshape(3, 3)
    out["power"] = m * r[43:46]
    out["neighbors"] = r[46:49].copy()
    out["step"] = m * (r[28:31] + r[31:34])
    return out


# ---- wall loads (owHIPSolver.wall_measure / wall_diagnostics; include/sphmi.h, sph_wall_measure) ----
WALL_FIELDS = ("shift_x", "shift_y", "shift_z", "dv_x", "dv_y", "dv_z", "share", "w_set", "n_touching", "n_slots") + \
    tuple("%s_%s" % (k, a) for k in _FORCE_KINDS for a in "xyz") + ("x", "y", "z", "vx", "vy", "vz", "vw", "contact", "reflected") + \
    ("unused28", "unused29", "unused30", "unused31")
WALL_DIAG_FIELDS = ("n", "n_contact", "n_shared", "n_reflected") + tuple("sum_" + f for f in WALL_FIELDS[:6]) + \
    tuple("sum_" + f for f in WALL_FIELDS[10:19]) + tuple("sum_torque_contact_" + a for a in "xyz") + \
    tuple("sum_torque_force_" + a for a in "xyz") + ("sum_share", "sum_w_set") + tuple("reserved%d" % w for w in range(27, 32))


def wall_summary(record, mass, time_step):
    """A wall_diagnostics() record as physical numbers, a dict of float64 values. The record's sums are per unit mass: `mass`
    (cfg.mass, kg per particle) times the summed velocity change over `time_step` (cfg.timeStep) is the contact's force in
    newtons, `mass` times the summed K7 / K12 accelerations the force-stage force. contact_force, viscous, tension, pressure and
    stage_force = (viscous + pressure) + tension: [3], on the selected liquid; contact_torque, stage_torque: [3] about the origin
    in newton x scene unit; shift: the summed position shift (scene units); body_contact_load, body_stage_load, body_load and
    body_torque: the negatives, approximately what the liquid does to the body (include/sphmi.h, SCOPE); n, n_contact, n_shared,
    n_reflected, share and w_set: the counts and the summed share and weight."""
    r = np.asarray(record, np.float64).reshape(len(WALL_DIAG_FIELDS))
    m, per_dt = float(mass), float(mass) / float(time_step)
    out = {"n": r[0], "n_contact": r[1], "n_shared": r[2], "n_reflected": r[3], "shift": r[4:7].copy(), "share": r[25], "w_set": r[26]}
    out["contact_force"] = per_dt * r[7:10]
    out["viscous"], out["tension"], out["pressure"] = m * r[10:13], m * r[13:16], m * r[16:19]
    out["stage_force"] = (out["viscous"] + out["pressure"]) + out["tension"]
    out["contact_torque"] = per_dt * r[19:22]
    out["stage_torque"] = m * r[22:25]
    out["body_contact_load"] = -out["contact_force"]
    out["body_stage_load"] = -out["stage_force"]
    out["body_load"] = -(out["contact_force"] + out["stage_force"])
    out["body_torque"] = -(out["contact_torque"] + out["stage_torque"])
    return out


def write_vtk_forces(path, position, orig_id, records, mass=1.0):
    """Legacy-VTK polydata (binary, big-endian like write_vtk) of the particles of force_measure(selection=True): one point per
    record at position[orig_id] (`position`: [N, 4] in orig order; orig_id from selection()), with `id` (int), the three
    neighbour counts (float scalars) and the vectors load_liquid, load_elastic, load_boundary = mass x ((viscous + pressure) +
    tension) of that class, pressure_liquid = mass x the liquid's pressure term, and step = mass x (words 30..32 + words 33..35)."""
    rec = np.asarray(records, np.float32).reshape(-1, len(FORCE_FIELDS))
    ids = np.asarray(orig_id, np.uint32).reshape(-1)
    if ids.shape[0] != rec.shape[0]:
        raise ValueError("write_vtk_forces: one id per record expected")
    pos = np.asarray(position, np.float32).reshape(-1, 4)[ids.astype(np.int64), :3]
    n = rec.shape[0]
    m = np.float32(mass)
    per = rec[:, :27].reshape(n, 3, 3, 3)
    load = m * ((per[:, :, 0] + per[:, :, 2]) + per[:, :, 1])
    vectors = [("load_" + c, load[:, k]) for k, c in enumerate(FORCE_CLASSES)]
    vectors += [("pressure_liquid", m * per[:, 0, 2]), ("step", m * (rec[:, 30:33] + rec[:, 33:36]))]
    with open(path, "wb") as f:
        f.write(b"# vtk DataFile Version 3.0\nsphmi force decomposition\nBINARY\nDATASET POLYDATA\n")
        f.write(("POINTS %d float\n" % n).encode())
        f.write(pos.astype(">f4").tobytes())
        f.write(("\nVERTICES %d %d\n" % (n, 2 * n)).encode())
        cells = np.empty((n, 2), ">i4")
        cells[:, 0] = 1
        cells[:, 1] = np.arange(n)
        f.write(cells.tobytes())
        f.write(("\nPOINT_DATA %d\n" % n).encode())
        f.write(b"SCALARS id int 1\nLOOKUP_TABLE default\n")
        f.write(ids.astype(">i4").tobytes())
        for k, c in enumerate(FORCE_CLASSES):
            f.write(("\nSCALARS neighbors_%s float 1\nLOOKUP_TABLE default\n" % c).encode())
            f.write(np.ascontiguousarray(rec[:, 27 + k]).astype(">f4").tobytes())
        for name, v in vectors:
            f.write(("\nVECTORS %s float\n" % name).encode())
            f.write(np.ascontiguousarray(v).astype(">f4").tobytes())
        f.write(b"\n")
    return n


# ---- particle rendering (owHIPSolver.render / rendered; include/sphmi.h, sph_render_particles) ----
# SPH_RENDER_FIELD_RAMP: the five stops of colour mode 2 (blue, cyan, green, yellow, red)
FIELD_RAMP = np.array([(0, 0, 1), (0, 1, 1), (0, 1, 0), (1, 1, 0), (1, 0, 0)], np.float32)
# SPH_RENDER_LABEL_PALETTE: the twelve colours of colour mode 3 (label % 12)
LABEL_PALETTE = np.array([(0.90, 0.10, 0.10), (0.10, 0.50, 0.90), (0.20, 0.70, 0.20), (0.95, 0.60, 0.10), (0.60, 0.30, 0.80),
                          (0.10, 0.75, 0.75), (0.95, 0.90, 0.20), (0.85, 0.35, 0.65), (0.55, 0.35, 0.15), (0.40, 0.85, 0.55),
                          (0.30, 0.30, 0.65), (0.75, 0.75, 0.75)], np.float32)
TYPE_COLOURS = ((0.2, 0.45, 0.9), (0.9, 0.55, 0.2), (0.6, 0.6, 0.6))  # render_view's default for liquid, elastic, boundary


def look_at(eye, target, up=(0.0, 1.0, 0.0)):
    """(eye, right, up, forward) as float32[3] each, the orthonormal frame of a camera at `eye` looking at `target`:
    forward = (target - eye) normalised, right = forward x up normalised, up = right x forward. Computed in float64 and narrowed
    once. Raises when eye == target or `up` is parallel to the view direction."""
    e = [float(x) for x in np.asarray(eye, np.float64).reshape(3)]
    t = [float(x) for x in np.asarray(target, np.float64).reshape(3)]
    up = [float(x) for x in np.asarray(up, np.float64).reshape(3)]
    # plain double arithmetic in a fixed order, so that the C++ driver's frame has the same bits
    f = [t[0] - e[0], t[1] - e[1], t[2] - e[2]]
    n = math.sqrt((f[0] * f[0] + f[1] * f[1]) + f[2] * f[2])
    if not n > 0:
        raise ValueError("look_at: eye and target coincide")
    f = [x / n for x in f]
    r = [f[1] * up[2] - f[2] * up[1], f[2] * up[0] - f[0] * up[2], f[0] * up[1] - f[1] * up[0]]
    n = math.sqrt((r[0] * r[0] + r[1] * r[1]) + r[2] * r[2])
    if not n > 1e-12:
        raise ValueError("look_at: up is parallel to the view direction")
    r = [x / n for x in r]
    u = [r[1] * f[2] - r[2] * f[1], r[2] * f[0] - r[0] * f[2], r[0] * f[1] - r[1] * f[0]]
    e, r, u, f = (np.array(x, np.float64) for x in (e, r, u, f))
    return e.astype(np.float32), r.astype(np.float32), u.astype(np.float32), f.astype(np.float32)


def render_view(bbox_min, bbox_max, width=640, height=480, eye=None, target=None, up=(0.0, 1.0, 0.0), perspective=True, scale=None,
                radius=None, colour="density", field="speed", lo=0.0, hi=1.0, type_colours=TYPE_COLOURS, ambient=0.25,
                background=(0, 0, 0, 255), near=0.0, max_radius_px=256.0, margin=0.95):
    """An SphRenderView whose camera frames the box [bbox_min, bbox_max]: `target` defaults to the box centre, `eye` to a point
    two box diagonals away from it towards (+x, +y, +z) weighted (0.6, 0.5, 1); the principal point is the image centre; `scale`
    (pixels per scene unit, or the focal length in pixels with perspective=True) defaults to the largest value at which the eight
    corners in front of the camera stay inside `margin` of the half image. `radius` (scene units) defaults to 1/60 of the box
    diagonal. colour: "type", "density", "field" (with `field` a name of HIST_FIELDS or 0..6 and lo < hi) or "label"."""
    import sphmi
    lo3, hi3 = np.asarray(bbox_min, np.float64).reshape(3), np.asarray(bbox_max, np.float64).reshape(3)
    centre, diag = 0.5 * (lo3 + hi3), float(np.linalg.norm(hi3 - lo3))
    target = centre if target is None else np.asarray(target, np.float64).reshape(3)
    if eye is None:
        d = np.array([0.6, 0.5, 1.0])
        eye = target + 2.0 * diag * d / np.linalg.norm(d)
    e, r, u, f = look_at(eye, target, up)
    if scale is None:
        corners = np.array([[x, y, z] for x in (lo3[0], hi3[0]) for y in (lo3[1], hi3[1]) for z in (lo3[2], hi3[2])]) - e.astype(np.float64)
        cx, cy, cz = corners @ r.astype(np.float64), corners @ u.astype(np.float64), corners @ f.astype(np.float64)
        if perspective:
            front = cz > 1e-9 * max(diag, 1.0)
            cx, cy = np.abs(cx[front]) / cz[front], np.abs(cy[front]) / cz[front]
        ex = max(float(np.max(np.abs(cx), initial=0.0)), 1e-30)
        ey = max(float(np.max(np.abs(cy), initial=0.0)), 1e-30)
        scale = margin * min(0.5 * width / ex, 0.5 * height / ey)
    v = sphmi.SphRenderView()
    v.width, v.height, v.projection = int(width), int(height), 1 if perspective else 0
    for k in range(3):
        v.eye[k], v.right[k], v.up[k], v.forward[k] = float(e[k]), float(r[k]), float(u[k]), float(f[k])
    v.scale = float(scale)
    v.centre[0], v.centre[1] = 0.5 * width, 0.5 * height
    v.nearPlane, v.radius, v.maxRadiusPx = float(near), float(diag / 60.0 if radius is None else radius), float(max_radius_px)
    if isinstance(colour, str):
        if colour not in sphmi.RENDER_COLOUR_MODES:
            raise ValueError("render_view: colour must be one of %s" % (sphmi.RENDER_COLOUR_MODES,))
        colour = sphmi.RENDER_COLOUR_MODES.index(colour)
    if isinstance(field, str):
        if field not in sphmi.HIST_FIELDS:
            raise ValueError("render_view: field must be one of %s" % (sphmi.HIST_FIELDS,))
        field = sphmi.HIST_FIELDS.index(field)
    v.colourMode, v.field, v.lo, v.hi = int(colour), int(field), float(lo), float(hi)
    for t in range(3):
        for k in range(3):
            v.typeColour[t][k] = float(type_colours[t][k])
    v.ambient = float(ambient)
    for k in range(4):
        v.background[k] = int(background[k])
    return v


def thickness_in_scene_units(thickness, radius):
    """float64 image of the summed chord lengths in scene units: a thickness word counts radius / 128 (a fragment through the
    middle of a sphere adds 256 = the diameter 2 * radius)."""
    return np.asarray(thickness, np.float64) * (float(np.float32(radius)) / 128.0)


def _rgb_image(image, channels):
    a = np.asarray(image)
    if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] not in (3, 4) or a.shape[0] < 1 or a.shape[1] < 1:
        raise ValueError("an image must be uint8[H, W, 3] or uint8[H, W, 4]")
    if a.shape[2] == channels:
        return np.ascontiguousarray(a)
    if channels == 3:
        return np.ascontiguousarray(a[:, :, :3])
    return np.ascontiguousarray(np.concatenate([a, np.full(a.shape[:2] + (1,), 255, np.uint8)], axis=2))


def write_ppm(path, image):
    """Binary PPM (P6, maxval 255) of uint8[H, W, 3] or the RGB of uint8[H, W, 4] (rendered()["rgba"]): the file
    `sphmi_run --render-out` writes."""
    a = _rgb_image(image, 3)
    with open(path, "wb") as f:
        f.write(b"P6\n%d %d\n255\n" % (a.shape[1], a.shape[0]))
        f.write(a.tobytes())
    return a.shape[0], a.shape[1]


def read_ppm(path):
    """uint8[H, W, 3] of a binary P6 file with maxval 255 (comments in the header are skipped)."""
    with open(path, "rb") as f:
        data = f.read()
    tokens, at = [], 0
    while len(tokens) < 4:
        while at < len(data) and data[at:at + 1].isspace():
            at += 1
        if data[at:at + 1] == b"#":
            while at < len(data) and data[at:at + 1] != b"\n":
                at += 1
            continue
        start = at
        while at < len(data) and not data[at:at + 1].isspace():
            at += 1
        if start == at:
            raise ValueError("%s: truncated PPM header" % path)
        tokens.append(data[start:at])
    at += 1  # the single whitespace byte after maxval
    if tokens[0] != b"P6" or int(tokens[3]) != 255:
        raise ValueError("%s: not a binary P6 file with maxval 255" % path)
    w, h = int(tokens[1]), int(tokens[2])
    if len(data) - at != 3 * w * h:
        raise ValueError("%s: %d bytes of pixels, %d expected" % (path, len(data) - at, 3 * w * h))
    return np.frombuffer(data, np.uint8, 3 * w * h, at).reshape(h, w, 3).copy()


_PNG_MAGIC = b"\x89PNG\r\n\x1a\n"


def write_png(path, image, level=6):
    """PNG of uint8[H, W, 4] (or [H, W, 3], made opaque): 8-bit RGBA, non-interlaced, every row with filter 0."""
    a = _rgb_image(image, 4)
    h, w = a.shape[:2]
    rows = np.zeros((h, 1 + 4 * w), np.uint8)  # the leading 0 of a row is its filter type
    rows[:, 1:] = a.reshape(h, 4 * w)

    def chunk(kind, body):
        return struct.pack(">I", len(body)) + kind + body + struct.pack(">I", zlib.crc32(kind + body) & 0xffffffff)
    with open(path, "wb") as f:
        f.write(_PNG_MAGIC)
        f.write(chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 6, 0, 0, 0)))
        f.write(chunk(b"IDAT", zlib.compress(rows.tobytes(), level)))
        f.write(chunk(b"IEND", b""))
    return h, w


def read_png(path):
    """uint8[H, W, 4] of a PNG as write_png writes it (8-bit RGBA, non-interlaced, filter 0 on every row); anything else is
    refused."""
    with open(path, "rb") as f:
        data = f.read()
    if data[:8] != _PNG_MAGIC:
        raise ValueError("%s: not a PNG" % path)
    at, header, body = 8, None, b""
    while at + 12 <= len(data):
        n, kind = struct.unpack(">I4s", data[at:at + 8])
        chunk = data[at + 8:at + 8 + n]
        crc, = struct.unpack(">I", data[at + 8 + n:at + 12 + n])
        if len(chunk) != n or (zlib.crc32(kind + chunk) & 0xffffffff) != crc:
            raise ValueError("%s: damaged %s chunk" % (path, kind.decode("latin-1")))
        if kind == b"IHDR":
            header = struct.unpack(">IIBBBBB", chunk)
        elif kind == b"IDAT":
            body += chunk
        elif kind == b"IEND":
            break
        at += 12 + n
    if header is None or header[2:] != (8, 6, 0, 0, 0):
        raise ValueError("%s: only 8-bit non-interlaced RGBA is read" % path)
    w, h = header[:2]
    raw = np.frombuffer(zlib.decompress(body), np.uint8)
    if raw.size != h * (1 + 4 * w):
        raise ValueError("%s: %d bytes of rows, %d expected" % (path, raw.size, h * (1 + 4 * w)))
    rows = raw.reshape(h, 1 + 4 * w)
    if rows[:, 0].any():
        raise ValueError("%s: a row uses a filter other than 0" % path)
    return rows[:, 1:].reshape(h, w, 4).copy()


# ----------------------------------------------------------------------------- particle identities across edits
def track_ids(ids, edit_map=None, added=0, next_id=None):
    """Persistent particle identities across an edit of the particle set (owHIPSolver.remove_* / add_particles / emit_lattice).
    `ids` (int64[N]) names the particle at every original id before the edit; identities of a new run are np.arange(N).
    `edit_map` is owHIPSolver.edit_map() of a removal (None: nothing was removed): survivors keep their identity at their new
    id. `added` particles were appended after that and get the fresh identities next_id, next_id + 1, ... (next_id None: one
    above the largest identity in `ids`, or 0 for an empty set; pass the value returned by the previous call so that an identity
    of a removed particle is never given out again). Returns (ids after the edit, the next unused identity). Joining two
    frames on these identities gives trajectories by particle whatever was drained or emitted in between."""
    ids = np.asarray(ids, np.int64).reshape(-1)
    if next_id is None:
        next_id = int(ids.max()) + 1 if ids.size else 0
    if edit_map is not None:
        m = np.asarray(edit_map, np.int64).reshape(-1)
        if m.size != ids.size:
            raise ValueError("track_ids: the edit map describes %d particles, ids %d" % (m.size, ids.size))
        keep = m >= 0
        out = np.empty(int(keep.sum()), np.int64)
        out[m[keep]] = ids[keep]
        ids = out
    added = int(added)
    if added < 0:
        raise ValueError("track_ids: added must be >= 0")
    fresh = np.arange(next_id, next_id + added, dtype=np.int64)
    return np.concatenate([ids, fresh]), int(next_id) + added


# ----------------------------------------------------------------------------- carried particle fields
FIELD_DIAG_FIELDS = ("n", "sum", "sum_sq", "min", "max", "tagged", "unused6", "unused7")  # owHIPSolver.field_diagnostics


def field_summary(record):
    """One record of owHIPSolver.field_diagnostics as numbers: count, mean, variance (sum_sq / n - mean * mean, in double: the
    spread that mixing removes), min, max, and tagged, the particles with a non-zero value. An empty selection gives zeros."""
    r = np.asarray(record, np.float64).reshape(-1)
    if r.size != len(FIELD_DIAG_FIELDS):
        raise ValueError("field_summary: a record holds %d doubles" % len(FIELD_DIAG_FIELDS))
    n = int(r[0])
    mean = r[1] / n if n else 0.0
    var = r[2] / n - mean * mean if n else 0.0
    return dict(count=n, mean=float(mean), variance=float(var), min=float(r[3]), max=float(r[4]), tagged=int(r[5]))


def field_sorted(values, particle_index):
    """A carried field (owHIPSolver.field_read: one float per particle in ORIG order) in SORTED order, from the (cell, orig id)
    pairs of read_particleIndex_buffer taken in the same step: out[sorted position] = values[orig id]. The sorted order is the
    one of force_measure, the selection's sorted indices and the rendered index image."""
    v = np.asarray(values, np.float32).reshape(-1)
    pi = np.asarray(particle_index).reshape(-1, 2)
    if pi.shape[0] != v.shape[0]:
        raise ValueError("field_sorted: one value per particle expected")
    return v[pi[:, 1].astype(np.int64)]


# ----------------------------------------------------------------------------- integral curves
def seed_rake(p0, p1, n):
    """n seeds on the segment p0 .. p1, both ends included (n == 1: p0), float32[n, 3]: p0 + (float)i * ((p1 - p0) / (n - 1)) per
    axis, one multiply and one add like sample_grid's lattice."""
    a, b = np.asarray(p0, np.float32).reshape(3), np.asarray(p1, np.float32).reshape(3)
    n = int(n)
    if n < 1:
        raise ValueError("seed_rake: n must be >= 1")
    d = (b - a) / np.float32(n - 1) if n > 1 else np.zeros(3, np.float32)
    return a[None, :] + np.arange(n, dtype=np.float32)[:, None] * d[None, :]


def seed_plane(origin, du, dv, nu, nv):
    """nu x nv seeds origin + (float)i * du + (float)j * dv (i fastest), float32[nv * nu, 3]: per axis one multiply and one add
    for each of the two directions, in that order."""
    o, du, dv = (np.asarray(v, np.float32).reshape(3) for v in (origin, du, dv))
    nu, nv = int(nu), int(nv)
    if nu < 1 or nv < 1:
        raise ValueError("seed_plane: nu and nv must be >= 1")
    i = np.arange(nu, dtype=np.float32)[None, :, None]
    j = np.arange(nv, dtype=np.float32)[:, None, None]
    return ((o[None, None, :] + i * du[None, None, :]) + j * dv[None, None, :]).reshape(-1, 3)


def write_vtk_polylines(path, vertices, lengths, scalars=None):
    """Legacy-VTK POLYDATA (binary, big-endian like write_vtk) of owHIPSolver.streamlines' result: the first lengths[c] vertices of
    every curve c of `vertices` [Q, M + 1, >= 3] as POINTS, one LINES cell per curve, and as point data the scalar `speed`: the
    vertices' fourth word, or `scalars` [Q, M + 1]. The format `sphmi_run --stream-out` writes. Returns the number of points."""
    v = np.asarray(vertices, np.float32)
    ln = np.asarray(lengths, np.int64).reshape(-1)
    if v.ndim != 3 or v.shape[2] < 3 or v.shape[0] != ln.shape[0] or (ln < 0).any() or (ln > v.shape[1]).any():
        raise ValueError("write_vtk_polylines: vertices [Q, M + 1, >= 3] and lengths [Q] within 0..M + 1 expected")
    if scalars is None:
        if v.shape[2] < 4:
            raise ValueError("write_vtk_polylines: no scalars and no fourth vertex word")
        sc = v[..., 3]
    else:
        sc = np.asarray(scalars, np.float32)
        if sc.shape != v.shape[:2]:
            raise ValueError("write_vtk_polylines: scalars must be [Q, M + 1]")
    keep = np.arange(v.shape[1])[None, :] < ln[:, None]
    total = int(ln.sum())
    cells = np.empty(total + ln.shape[0], np.int64)
    is_head = np.zeros(cells.shape[0], bool)
    is_head[np.cumsum(ln + 1) - (ln + 1)] = True  # each cell: its length, then its point ids
    cells[is_head] = ln
    cells[~is_head] = np.arange(total)
    with open(path, "wb") as f:
        f.write(b"# vtk DataFile Version 3.0\nsphmi streamlines\nBINARY\nDATASET POLYDATA\n")
        f.write(("POINTS %d float\n" % total).encode())
        f.write(np.ascontiguousarray(v[..., :3][keep]).astype(">f4").tobytes())
        f.write(("\nLINES %d %d\n" % (ln.shape[0], cells.shape[0])).encode())
        f.write(cells.astype(">i4").tobytes())
        f.write(("\nPOINT_DATA %d\nSCALARS speed float\nLOOKUP_TABLE default\n" % total).encode())
        f.write(np.ascontiguousarray(sc[keep]).astype(">f4").tobytes())
        f.write(b"\n")
    return total


def read_polylines(path):
    """A file of write_vtk_polylines / `sphmi_run --stream-out` as (points float32[P, 3], lengths int32[Q], speed float32[P]): the
    curves' vertices one curve after the other."""
    data = open(path, "rb").read()
    pos = 0

    def line():
        nonlocal pos
        end = data.index(b"\n", pos)
        out = data[pos:end].decode()
        pos = end + 1
        return out

    def block(count, dtype):
        nonlocal pos
        out = np.frombuffer(data, dtype, count, pos)
        pos += 4 * count
        if data[pos:pos + 1] != b"\n":
            raise ValueError("read_polylines: %s is not a polyline file of write_vtk_polylines" % path)
        pos += 1
        return out

    head = [line() for _ in range(4)]
    if head[0] != "# vtk DataFile Version 3.0" or head[2] != "BINARY" or head[3] != "DATASET POLYDATA":
        raise ValueError("read_polylines: %s is not a binary legacy-VTK POLYDATA file" % path)
    total = int(line().split()[1])
    points = block(3 * total, ">f4").astype(np.float32).reshape(total, 3)
    q, words = (int(w) for w in line().split()[1:3])
    cells = block(words, ">i4").astype(np.int64)
    lengths = np.empty(q, np.int32)
    at = 0
    for c in range(q):
        lengths[c] = cells[at]
        at += 1 + int(cells[at])
    if at != words or int(lengths.sum()) != total:
        raise ValueError("read_polylines: the LINES of %s do not cover its points once" % path)
    if int(line().split()[1]) != total or not line().startswith("SCALARS speed") or line() != "LOOKUP_TABLE default":
        raise ValueError("read_polylines: %s has no speed point data" % path)
    return points, lengths, block(total, ">f4").astype(np.float32)


# ---- kinematic bodies (owHIPSolver.body_set_pose; include/sphmi.h, sph_body_set_pose) ----
# A pose is float32[3, 4] = (R | t), always relative to the body's REFERENCE placement. Every helper computes in float64 and
# narrows once, at the end; pose_compose widens its arguments again, so a chain of compositions rounds once per link.
def _pose32(R, t):
    out = np.empty((3, 4), np.float64)
    out[:, :3] = R
    out[:, 3] = t
    return out.astype(np.float32)


def pose_identity():
    return _pose32(np.eye(3), np.zeros(3))


def pose_translate(v):
    """The pose that shifts the reference placement by v = (vx, vy, vz)."""
    return _pose32(np.eye(3), np.asarray(v, np.float64).reshape(3))


def pose_rotate(axis, angle, about=(0.0, 0.0, 0.0)):
    """The pose that turns the reference placement by `angle` (radians, right-handed) about the line through the point `about`
    along `axis` (normalised here): Rodrigues' R = cos I + sin [a]x + (1 - cos) a a^T and t = about - R about."""
    a = np.asarray(axis, np.float64).reshape(3)
    n = math.sqrt((a[0] * a[0] + a[1] * a[1]) + a[2] * a[2])
    if not n > 0:
        raise ValueError("pose_rotate: the axis is zero")
    a = a / n
    c, s = math.cos(float(angle)), math.sin(float(angle))
    K = np.array([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]])
    R = c * np.eye(3) + s * K + (1.0 - c) * np.outer(a, a)
    o = np.asarray(about, np.float64).reshape(3)
    return _pose32(R, o - R @ o)


def pose_compose(a, b):
    """The pose that applies b first and a second: (Ra Rb | Ra tb + ta)."""
    a, b = (np.asarray(p, np.float64).reshape(3, 4) for p in (a, b))
    return _pose32(a[:, :3] @ b[:, :3], a[:, :3] @ b[:, 3] + a[:, 3])


def piston(direction, amplitude, period, step):
    """The pose of a piston at step number `step`: the reference placement shifted along `direction` (normalised here) by
    amplitude * sin(2 pi step / period); the identity at step 0."""
    d = np.asarray(direction, np.float64).reshape(3)
    n = math.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
    if not n > 0 or not float(period) != 0.0:
        raise ValueError("piston: the direction and the period must not be zero")
    return pose_translate(d / n * (float(amplitude) * math.sin(2.0 * math.pi * float(step) / float(period))))


def spin(axis, about, rate, step):
    """The pose of a blade at step number `step`: the reference placement turned by rate * step radians about the line through
    `about` along `axis`; the identity at step 0."""
    return pose_rotate(axis, float(rate) * float(step), about)


# ---- free bodies (owHIPSolver.body_set_dynamics / bodies_advance; include/sphmi.h, sph_bodies_advance) ----
def body_mass_properties(ref_positions, mass):
    """Mass properties of a body whose members are equal point masses: ref_positions [M, 3 or 4] (body_read's reference
    positions), `mass` the body's total mass. Returns (com float64[3], inertia float64[3, 3] about com in reference axes, position
    units squared times kg, inertiaInv float64[6] = xx yy zz xy xz yz as sph_body_dynamics takes it). The inverse is the
    pseudo-inverse: a principal axis along which the members have no extent (a single row of particles about its own line, a
    single particle) has zero inertia and gets a zero row, so the body never turns about it."""
    p = np.asarray(ref_positions, np.float64)
    p = p.reshape(-1, p.shape[-1])[:, :3]
    if p.shape[0] < 1 or not float(mass) > 0:
        raise ValueError("body_mass_properties: at least one member and a mass > 0")
    com = p.mean(axis=0)
    r = p - com
    m = float(mass) / p.shape[0]
    inertia = m * (np.eye(3) * (r * r).sum() - r.T @ r)
    w, v = np.linalg.eigh(inertia)
    keep = w > 1e-12 * max(float(w.max()), 0.0)
    inv = (v[:, keep] / w[keep]) @ v[:, keep].T if keep.any() else np.zeros((3, 3))
    inv = 0.5 * (inv + inv.T)
    return com, inertia, np.array([inv[0, 0], inv[1, 1], inv[2, 2], inv[0, 1], inv[0, 2], inv[1, 2]], np.float64)


def body_state_summary(record, cfg):
    """One slot's bodies_advance() record as physical numbers, a dict: status, members, advances, max_move (in r0); position
    (metres: position units times simulationScale), velocity (the particles' velocity units, metres per second), orientation,
    angular_momentum, omega as they are; load_force in newtons; load_torque about the centre of mass in newton x position unit;
    n_contact, n_share, offenders, lowest_member."""
    r = np.asarray(record, np.float64).reshape(48)
    out = {"status": int(r[0]), "members": int(r[1]), "advances": int(r[2]), "max_move": r[3],
           "position": r[4:7] * float(cfg.simulationScale), "orientation": r[7:11].copy(), "velocity": r[11:14].copy(),
           "angular_momentum": r[14:17].copy(), "omega": r[17:20].copy(), "load_force": r[20:23].copy(),
           "load_torque": r[23:26].copy(), "n_contact": int(r[26]), "n_share": int(r[27]), "offenders": int(r[28]),
           "lowest_member": int(r[29]) if r[0] == 1 else -1}
    return out


# ---- flow gauges (owHIPSolver.gauge_define / gauges_accumulate; include/sphmi.h, sph_gauges_accumulate) ----
_GAUGE_TERMS = ("n", "sum_vx", "sum_vy", "sum_vz", "sum_v2", "sum_field", "sum_alpha", "sum_beta")
GAUGE_FIELDS = tuple("plus_" + t for t in _GAUGE_TERMS) + tuple("minus_" + t for t in _GAUGE_TERMS)
GAUGE_TOTAL_FIELDS = GAUGE_FIELDS + ("calls", "first_plus_call", "first_minus_call", "last_call")


def gauge_rect(centre, normal, width, height, up=(0.0, 1.0, 0.0)):
    """The definition of a rectangular gauge, a dict with origin, u, v (float32[3] each) for owHIPSolver.gauge_define: `width` along
    u and `height` along v about `centre`, u x v pointing along `normal`. v is `up` made orthogonal to the normal (an `up` along the
    normal is refused), u = v x normal."""
    n = np.asarray(normal, np.float64).reshape(3)
    ln = float(np.sqrt((n * n).sum()))
    if not (ln > 0 and np.isfinite(ln)) or not (float(width) > 0 and float(height) > 0):
        raise ValueError("gauge_rect: a normal that is not zero, and a width and a height > 0")
    n = n / ln
    v = np.asarray(up, np.float64).reshape(3)
    v = v - n * float((v * n).sum())
    lv = float(np.sqrt((v * v).sum()))
    if not lv > 1e-9:
        raise ValueError("gauge_rect: up is along the normal")
    v = v / lv
    u = np.cross(v, n)  # u x v = (v x n) x v = n
    u, v = u * float(width), v * float(height)
    origin = np.asarray(centre, np.float64).reshape(3) - 0.5 * u - 0.5 * v
    return dict(origin=origin.astype(np.float32), u=u.astype(np.float32), v=v.astype(np.float32))


def gauge_plane(point, normal):
    """The definition of a whole-plane gauge through `point` with positive direction `normal`: a dict with origin, u, v and
    plane=True for owHIPSolver.gauge_define. u and v are unit vectors, so alpha and beta are scene units along them."""
    n = np.asarray(normal, np.float64).reshape(3)
    ln = float(np.sqrt((n * n).sum()))
    if not (ln > 0 and np.isfinite(ln)):
        raise ValueError("gauge_plane: a normal that is not zero")
    n = n / ln
    k = int(np.argmin(np.abs(n)))  # the axis the normal has least of
    v = np.cross(n, np.eye(3)[k])
    v = v / np.sqrt((v * v).sum())
    u = np.cross(v, n)
    return dict(origin=np.asarray(point, np.float32).reshape(3), u=u.astype(np.float32), v=v.astype(np.float32), plane=True)


def gauge_summary(record_or_total, cfg, calls=1):
    """A gauge's record (16 words) or totals (20 words) as physical numbers, a dict of float64 values. plus, minus, net, gross: the
    particle counts; volume_rate: net count times the particle's volume cfg.mass / cfg.rho0 per `calls` steps of cfg.timeStep (cubic
    metres per second; with totals `calls` defaults to their word 16); mean_velocity_plus / _minus [3] and mean_v2_plus / _minus:
    what the crossing particles had on average (nan without a crossing); field_flux: the carried field's net sum, plus minus minus;
    centroid_plus / _minus: the mean (alpha, beta) of the crossings."""
    r = np.asarray(record_or_total, np.float64).reshape(-1)
    if r.size not in (len(GAUGE_FIELDS), len(GAUGE_TOTAL_FIELDS)):
        raise ValueError("gauge_summary: a record of %d or totals of %d words" % (len(GAUGE_FIELDS), len(GAUGE_TOTAL_FIELDS)))
    if r.size == len(GAUGE_TOTAL_FIELDS) and calls == 1:
        calls = r[16]
    p, m = r[0:8], r[8:16]
    out = {"plus": p[0], "minus": m[0], "net": p[0] - m[0], "gross": p[0] + m[0]}
    seconds = float(calls) * float(cfg.timeStep)
    out["volume_rate"] = (p[0] - m[0]) * (float(cfg.mass) / float(cfg.rho0)) / seconds if seconds > 0 else np.nan
    with np.errstate(invalid="ignore", divide="ignore"):
        for name, h in (("plus", p), ("minus", m)):
            out["mean_velocity_" + name] = h[1:4] / h[0]
            out["mean_v2_" + name] = h[4] / h[0]
            out["centroid_" + name] = h[6:8] / h[0]
    out["field_flux"] = p[5] - m[5]
    return out


# the 8 words of a level-probe record (include/sphmi.h, sph_probes_record): where the level is, the fractional point index,
# PROBE_FOUND / PROBE_DRY / PROBE_SUBMERGED, the index K of the inside point (-1: none) and the field at K and at K + 1
LEVEL_FIELDS = ("x", "y", "z", "index", "status", "k", "f_inside", "f_outside")


def level_columns(origin, spacing, dims, axis=2, field="shepard", iso=0.5, types=(1,)):
    """One level-probe line per column of the lattice origin + (float)i * spacing, i < dims, along `axis`, with the far end up: a
    line starts at the column's lowest lattice point, steps by spacing[axis] and has dims[axis] points, so its points are the
    lattice's own, bit for bit. The columns come in the lattice's order over the other two axes, the lower axis fastest (axis 2: a
    [ny, nx] map). An array of PROBE_LINE_DTYPE for owHIPSolver.probes_set_lines."""
    from . import PROBE_LINE_DTYPE, SURFACE_FIELDS, _field_index, type_mask
    o = np.asarray(origin, np.float32).reshape(3)
    sp = np.asarray(spacing, np.float32).reshape(3)
    dm = [int(v) for v in np.asarray(dims).reshape(3)]
    axis = int(axis)
    if axis not in (0, 1, 2):
        raise ValueError("level_columns: axis must be 0, 1 or 2")
    a, b = [c for c in range(3) if c != axis]  # a runs fastest
    lines = np.zeros(dm[a] * dm[b], PROBE_LINE_DTYPE)
    ia, ib = np.meshgrid(np.arange(dm[a]), np.arange(dm[b]))  # [nb, na]
    org = np.empty((dm[b], dm[a], 3), np.float32)
    org[..., a] = o[a] + ia.astype(np.float32) * sp[a]
    org[..., b] = o[b] + ib.astype(np.float32) * sp[b]
    org[..., axis] = o[axis]
    lines["origin"] = org.reshape(-1, 3)
    lines["step"][:, axis] = sp[axis]
    lines["count"] = dm[axis]
    lines["field"] = _field_index(field, GRID_FIELDS[:SURFACE_FIELDS], "level_columns")
    lines["iso"] = np.float32(iso)
    lines["typeMask"] = type_mask(types)
    return lines


def level_heights(records, axis=2):
    """The level along `axis` of level-probe records [..., 8]: the crossing's coordinate, the far end's where the line is
    submerged, NaN where it is dry — the convention of free_surface_height. float64 [...]."""
    r = np.asarray(records, np.float32)
    if r.shape[-1] != len(LEVEL_FIELDS):
        raise ValueError("level_heights: records of %d words" % len(LEVEL_FIELDS))
    out = r[..., int(axis)].astype(np.float64)
    out[r[..., 4] == 1.0] = np.nan
    return out


def probe_series(history, word):
    """One word of every record over a history's calls: history [calls, n, 8] (owHIPSolver.probe_history, either half) and a word
    number or name (GRID_FIELDS for point records, LEVEL_FIELDS for level records) -> float32 [calls, n]."""
    h = np.asarray(history, np.float32)
    if h.ndim != 3 or h.shape[-1] != len(LEVEL_FIELDS):
        raise ValueError("probe_series: a history is [calls, n, 8]")
    if isinstance(word, str):
        names = LEVEL_FIELDS if word in LEVEL_FIELDS else GRID_FIELDS
        if word not in names:
            raise ValueError("probe_series: word must be one of %s or %s" % (GRID_FIELDS, LEVEL_FIELDS))
        word = names.index(word)
    return np.ascontiguousarray(h[:, :, int(word)])


def stats_moments(acc, calls):
    """The 16 moment words of sph_stats_read_moments (sphmi.STATS_MOMENT_FIELDS) from accumulators [..., 24]
    (owHIPSolver.stats), in float64 before the narrowing to float: the same operations in the same order, so
    stats_moments(acc, calls).astype(float32) is what owHIPSolver.stats_moments returns, bit for bit. calls >= 1."""
    from . import STATS_MOMENT_WORDS, STATS_WORDS
    a = np.asarray(acc, np.float64)
    if a.shape[-1] != STATS_WORDS:
        raise ValueError("stats_moments: accumulators of %d words" % STATS_WORDS)
    if int(calls) < 1:
        raise ValueError("stats_moments: no call has been made")
    C = np.float64(int(calls))
    n = a[..., 0]
    wet = n > 0
    out = np.zeros(a.shape[:-1] + (STATS_MOMENT_WORDS,), np.float64)
    with np.errstate(all="ignore"):
        out[..., 0] = n / C
        mr = a[..., 3] / C
        out[..., 1] = mr
        out[..., 2] = a[..., 4] / C - mr * mr
        nn = np.where(wet, n, 1.0)
        m = [a[..., 5 + k] / nn for k in range(3)]
        for k in range(3):
            out[..., 3 + k] = m[k]
        for w, (i, j) in enumerate(((0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2))):
            out[..., 6 + w] = a[..., 8 + w] / nn - m[i] * m[j]
        mp = a[..., 14] / nn
        out[..., 12] = mp
        out[..., 13] = a[..., 15] / nn - mp * mp
    out[..., 14] = a[..., 1]
    out[..., 15] = a[..., 20]
    out[..., 3:14][~wet] = 0.0
    out[..., 15][~wet] = 0.0
    out[..., 14][~wet] = -1.0
    return out


def stats_summary(acc, calls):
    """What a flow is reported by, from accumulators [..., 24] (owHIPSolver.stats) after `calls` calls, float64: `wet_fraction`,
    `mean_velocity` [..., 3], `stress` [..., 3, 3] (the symmetric velocity covariance <u_a' u_b'>: times the density, the Reynolds
    stresses), `tke` = (xx + yy + zz) / 2, `mean_pressure`, `rms_pressure` (the root of the variance, which rounding may leave a
    little below 0: clamped there), `arrival_call` (-1: never wet), `peak_pressure` and `peak_pressure_call` (-1). The moments are
    stats_moments', so a node that was never wet has zeros."""
    a = np.asarray(acc, np.float64)
    m = stats_moments(a, calls)
    stress = np.empty(m.shape[:-1] + (3, 3), np.float64)
    for w, (i, j) in enumerate(((0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2))):
        stress[..., i, j] = m[..., 6 + w]
        stress[..., j, i] = m[..., 6 + w]
    return {"wet_fraction": m[..., 0], "mean_velocity": m[..., 3:6], "stress": stress,
            "tke": 0.5 * ((m[..., 6] + m[..., 7]) + m[..., 8]), "mean_pressure": m[..., 12],
            "rms_pressure": np.sqrt(np.maximum(m[..., 13], 0.0)), "arrival_call": m[..., 14], "peak_pressure": m[..., 15],
            "peak_pressure_call": a[..., 21]}


def write_vtk_stats(path, origin, spacing, acc, calls):
    """Legacy-VTK STRUCTURED_POINTS (binary, big-endian like write_vtk_grid) of the statistics `acc` [nz, ny, nx, 24] after `calls`
    calls: scalars `wet_fraction`, `tke`, `mean_pressure`, `rms_pressure`, `arrival_call`, `peak_pressure`, `peak_pressure_call`,
    vectors `mean_velocity` and the six `stress_ab` scalars. Returns the node count."""
    a = np.asarray(acc, np.float64)
    if a.ndim != 4:
        raise ValueError("write_vtk_stats: accumulators must be [nz, ny, nx, 24]")
    s = stats_summary(a, calls)
    nz, ny, nx = a.shape[:3]
    n = nx * ny * nz
    with open(path, "wb") as f:
        f.write(b"# vtk DataFile Version 3.0\nsphmi statistics\nBINARY\nDATASET STRUCTURED_POINTS\n")
        f.write(("DIMENSIONS %d %d %d\n" % (nx, ny, nz)).encode())
        f.write(("ORIGIN %.9g %.9g %.9g\n" % tuple(float(np.float32(v)) for v in origin)).encode())
        f.write(("SPACING %.9g %.9g %.9g\n" % tuple(float(np.float32(v)) for v in spacing)).encode())
        f.write(("POINT_DATA %d\n" % n).encode())
        scalars = [(k, s[k]) for k in ("wet_fraction", "tke", "mean_pressure", "rms_pressure", "arrival_call", "peak_pressure",
                                       "peak_pressure_call")]
        scalars += [("stress_%s%s" % ("xyz"[i], "xyz"[j]), s["stress"][..., i, j]) for i, j in
                    ((0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2))]
        for name, v in scalars:
            f.write(("SCALARS %s float 1\nLOOKUP_TABLE default\n" % name).encode())
            f.write(np.ascontiguousarray(v).astype(">f4").tobytes())
            f.write(b"\n")
        f.write(b"VECTORS mean_velocity float\n")
        f.write(np.ascontiguousarray(s["mean_velocity"]).astype(">f4").tobytes())
        f.write(b"\n")
    return n


def read_stats(path):
    """A `sphmi_run --stats-out` file: (lattice dict of origin, spacing, dims, typeMask; acc float64[nz, ny, nx, 24]; calls; first
    step; every), the accumulators as the run left them after one stats_accumulate behind every `every`-th step from `first` on."""
    with open(path, "rb") as f:
        head = f.readline().split()
        if head[:2] != [b"sphmi", b"stats"] or head[2::2] != [b"calls", b"from", b"every", b"nx", b"ny", b"nz"]:
            raise ValueError("read_stats: not a statistics file")
        calls, first, every, nx, ny, nz = (int(v) for v in head[3::2])
        g = np.frombuffer(f.read(40), np.dtype([("origin", np.float32, 3), ("spacing", np.float32, 3), ("dims", np.int32, 3),
                                                ("typeMask", np.uint32)]))
        data = np.frombuffer(f.read(), np.float64)
    if g.size != 1 or tuple(int(v) for v in g["dims"][0]) != (nx, ny, nz) or data.size != nx * ny * nz * 24:
        raise ValueError("read_stats: %d words for a lattice of %d x %d x %d nodes" % (data.size, nx, ny, nz))
    lattice = {"origin": g["origin"][0].copy(), "spacing": g["spacing"][0].copy(), "dims": (nx, ny, nz), "typeMask": int(g["typeMask"][0])}
    return lattice, data.reshape(nz, ny, nx, 24).copy(), calls, first, every


# ---- binned diagnostics (owHIPSolver.bin_diagnostics / bin_index; include/sphmi.h, sph_bin_diagnostics) ----
def _bin_lattice(lattice):
    g = np.asarray(lattice)
    if g.dtype.names is None or g.size != 1 or set(g.dtype.names) != {"origin", "spacing", "dims", "typeMask"}:
        raise ValueError("a bin lattice is what sphmi.bin_lattice() returns")
    g = g.reshape(1)
    return g["origin"][0].astype(np.float32), g["spacing"][0].astype(np.float32), tuple(int(v) for v in g["dims"][0])


def bin_edges(lattice):
    """(ex, ey, ez): the float32 edges of the lattice's bins per axis, dims[a] + 1 each, by the contract's expression origin[a] +
    (float32)i * spacing[a] (one rounded multiply, one rounded add); (-inf, +inf) for a whole axis (dims 1, spacing 0)."""
    o, sp, dims = _bin_lattice(lattice)
    out = []
    for a in range(3):
        if dims[a] == 1 and sp[a] == 0:
            out.append(np.array([-np.inf, np.inf], np.float32))
        else:
            i = np.arange(dims[a] + 1).astype(np.float32)
            out.append((o[a] + (i * sp[a]).astype(np.float32)).astype(np.float32))
    return tuple(out)


def bin_boxes(lattice):
    """float32[bins, 6]: the box (x0, y0, z0, x1, y1, z1) of every bin, bin (i, j, k) at row (k * ny + j) * nx + i, usable as
    diagnostics() regions (16 at a time): bin_diagnostics' record b is the diagnostics record of row b."""
    ex, ey, ez = bin_edges(lattice)
    nx, ny, nz = ex.size - 1, ey.size - 1, ez.size - 1
    k, j, i = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    i, j, k = i.reshape(-1), j.reshape(-1), k.reshape(-1)
    return np.stack([ex[i], ey[j], ez[k], ex[i + 1], ey[j + 1], ez[k + 1]], axis=1).astype(np.float32)


def bin_profile(records, cfg):
    """Per bin, from records [..., 32] (float64, computed in double): `n`, `mass` = n * cfg.mass, `mean_velocity` [..., 3],
    `mean_position` [..., 3], `mean_density`, `mean_pressure`. An empty bin has zeros everywhere (no NaN, no warning)."""
    r = np.asarray(records, np.float64)
    if r.shape[-1] != len(DIAG_FIELDS):
        raise ValueError("bin_profile: a record has %d words" % len(DIAG_FIELDS))
    n = r[..., 0]
    inv = np.zeros_like(n)
    np.divide(1.0, n, out=inv, where=n > 0)
    return {"n": n, "mass": n * float(cfg.mass), "mean_position": r[..., 1:4] * inv[..., None],
            "mean_velocity": r[..., 4:7] * inv[..., None], "mean_density": r[..., 11] * inv, "mean_pressure": r[..., 13] * inv}


def bin_column_depth(records, cfg, lattice):
    """The water depth of a plan-view map, scene units: a lattice with exactly one whole axis (dims 1, spacing 0), records
    [nz, ny, nx, 32] (or any shape of nx * ny * nz records). Each particle stands for the volume cfg.mass / cfg.rho0 (cubic
    metres; scene units are metres / cfg.simulationScale), so depth = n * volume / bin area. Returns float64 of the records'
    leading shape."""
    _, sp, dims = _bin_lattice(lattice)
    whole = [a for a in range(3) if dims[a] == 1 and sp[a] == 0]
    if len(whole) != 1:
        raise ValueError("bin_column_depth: the lattice must have exactly one whole axis (dims 1, spacing 0)")
    r = np.asarray(records, np.float64)
    if r.shape[-1] != len(DIAG_FIELDS) or r[..., 0].size != dims[0] * dims[1] * dims[2]:
        raise ValueError("bin_column_depth: records do not fit the lattice")
    area = float(np.prod([float(sp[a]) for a in range(3) if a != whole[0]]))
    volume = float(cfg.mass) / float(cfg.rho0) / float(cfg.simulationScale) ** 3
    return r[..., 0] * (volume / area)


def write_bins_csv(path, steps, records):
    """One row per step and bin: `step,bin,` then the 32 record words as %.17g (a round trip keeps every bit), under a header naming
    them. `steps`: S step numbers; `records`: float64[S, ..., 32], the bins of a step in flat order (k * ny + j) * nx + i."""
    rec = np.asarray(records, np.float64)
    if rec.ndim < 2 or rec.shape[-1] != len(DIAG_FIELDS) or rec.shape[0] != len(steps):
        raise ValueError("write_bins_csv: records must be [len(steps), ..., %d]" % len(DIAG_FIELDS))
    rec = rec.reshape(len(steps), -1, len(DIAG_FIELDS))
    with open(path, "w") as f:
        f.write("step,bin," + ",".join(DIAG_FIELDS) + "\n")
        for s, block in zip(steps, rec):
            for b, row in enumerate(block):
                f.write("%d,%d," % (int(s), b) + ",".join("%.17g" % float(x) for x in row) + "\n")


def read_bins(path):
    """(steps int64[S], records float64[S, bins, 32]) of a file written by write_bins_csv or `sphmi_run --bin-out`."""
    with open(path) as f:
        header = f.readline().strip().split(",")
        if header != ["step", "bin"] + list(DIAG_FIELDS):
            raise ValueError("%s: not a table of binned diagnostics" % path)
        rows = [line.strip().split(",") for line in f if line.strip()]
    if not rows:
        return np.zeros(0, np.int64), np.zeros((0, 0, len(DIAG_FIELDS)), np.float64)
    steps, bins = [int(r[0]) for r in rows], [int(r[1]) for r in rows]
    B = max(bins) + 1
    if len(rows) % B or bins != list(range(B)) * (len(rows) // B):
        raise ValueError("%s: rows are not grouped as one block of bins per step" % path)
    rec = np.array([[float(x) for x in r[2:]] for r in rows], np.float64).reshape(-1, B, len(DIAG_FIELDS))
    return np.array(steps[::B], np.int64), rec


def write_vtk_bins(path, lattice, records, cfg):
    """Legacy-VTK STRUCTURED_POINTS (binary, big-endian like write_vtk_stats) whose CELLS are the bins: cell scalars `n`, `mass`,
    `mean_density`, `mean_pressure` and cell vectors `mean_velocity` of bin_profile(records [nz, ny, nx, 32]). A whole axis is
    drawn as one cell from 0 to 1. Returns the bin count."""
    o, sp, dims = _bin_lattice(lattice)
    r = np.asarray(records, np.float64)
    nx, ny, nz = dims
    if r.shape != (nz, ny, nx, len(DIAG_FIELDS)):
        raise ValueError("write_vtk_bins: records must be [nz, ny, nx, %d]" % len(DIAG_FIELDS))
    prof = bin_profile(r, cfg)
    whole = [dims[a] == 1 and sp[a] == 0 for a in range(3)]
    with open(path, "wb") as f:
        f.write(b"# vtk DataFile Version 3.0\nsphmi binned diagnostics\nBINARY\nDATASET STRUCTURED_POINTS\n")
        f.write(("DIMENSIONS %d %d %d\n" % (nx + 1, ny + 1, nz + 1)).encode())
        f.write(("ORIGIN %.9g %.9g %.9g\n" % tuple(0.0 if whole[a] else float(o[a]) for a in range(3))).encode())
        f.write(("SPACING %.9g %.9g %.9g\n" % tuple(1.0 if whole[a] else float(sp[a]) for a in range(3))).encode())
        f.write(("CELL_DATA %d\n" % (nx * ny * nz)).encode())
        for name in ("n", "mass", "mean_density", "mean_pressure"):
            f.write(("SCALARS %s float 1\nLOOKUP_TABLE default\n" % name).encode())
            f.write(np.ascontiguousarray(prof[name]).astype(">f4").tobytes())
            f.write(b"\n")
        f.write(b"VECTORS mean_velocity float\n")
        f.write(np.ascontiguousarray(prof["mean_velocity"]).astype(">f4").tobytes())
        f.write(b"\n")
    return nx * ny * nz


def read_probes(path):
    """A `sphmi_run --probe-out` file: (points float32[calls, P, 8], levels float32[calls, L, 8], every), the history of the run's
    probes_record calls, one after every `every` steps."""
    with open(path, "rb") as f:
        head = f.readline().split()
        if head[:2] != [b"sphmi", b"probes"] or head[2::2] != [b"calls", b"points", b"lines", b"every"]:
            raise ValueError("read_probes: not a probe history")
        calls, P, L, every = (int(v) for v in head[3::2])
        data = np.frombuffer(f.read(), np.float32)
    if data.size != calls * (P + L) * 8:
        raise ValueError("read_probes: %d words for %d calls of %d points and %d lines" % (data.size, calls, P, L))
    rows = data.reshape(calls, P + L, 8)
    return np.ascontiguousarray(rows[:, :P]), np.ascontiguousarray(rows[:, P:]), every

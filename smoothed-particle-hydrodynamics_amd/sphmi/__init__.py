"""sphmi — ctypes binding of libsphmi.so / libsphmi_host.so (include/sphmi.h, include/sphmi_host.h).

`owHIPSolver` mirrors the reference's `owOpenCLSolver` (src/owOpenCLSolver.h:28-62) method for method, and
`owPhysicsFluidSimulator` mirrors the stage order of `simulationStep()` (src/owPhysicsFluidSimulator.cpp:79-149),
so tests read like calls into the reference. There is no CPU fallback: if libsphmi.so or a GPU is missing the
constructor raises.
"""
import ctypes as C
import os

import numpy as np

_PKG = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB_PATH = os.environ.get("SPHMI_LIB", os.path.join(_PKG, "libsphmi.so"))  # SPHMI_LIB: A/B builds of the same ABI
HOST_LIB_PATH = os.path.join(_PKG, "libsphmi_host.so")

ABI_VERSION = 2
MAX_BODIES = 16  # SPH_MAX_BODIES: kinematic-body slots per solver
SAMPLE_WORDS = 8  # sph_sample_* record: density, shepard, vx, vy, vz, pressure, count, 0
SURFACE_FIELDS = 6  # sph_extract_surface: record words 0..5
SHELL_WORDS = 10  # SPH_SHELL_WORDS: int64 words of one row of sph_read_shells' table
SHELL_FIELDS = ("root", "vertices", "triangles", "open", "bad", "a2", "d6", "mx", "my", "mz")  # ... and their names
DIAG_WORDS = 32  # sph_diagnostics record (frames.DIAG_FIELDS)
DIAG_MAX_REGIONS = 16
HIST_MAX_BINS = 4096
BIN_MAX_BINS = 1 << 18  # SPH_BIN_MAX_BINS: bins of one bin_diagnostics / bin_index lattice
HIST_FIELDS = ("density", "speed", "pressure", "neighbors", "x", "y", "z")  # sph_histogram field numbers 0..6
SELECT_WORDS = 12  # sph_read_selection record: x, y, z, type, vx, vy, vz, rho, p, neighbour count, surface measure, 0 (frames.SELECT_FIELDS)
SELECT_MAX_TERMS = 4
SELECT_FIELDS = HIST_FIELDS + ("surface",)  # sph_select_particles term fields 0..7
GRADIENT_WORDS = 32  # sph_sample_gradient_* record: the sample record, then gradients, vorticity, divergence, Q (frames.GRADIENT_FIELDS)
ELASTIC_WORDS = 12  # sph_elastic_measure record (frames.ELASTIC_FIELDS)
MUSCLE_WORDS = 16  # sph_muscle_diagnostics record (frames.MUSCLE_FIELDS)
MEMBRANE_WORDS = 8  # sph_membrane_measure record: area, unit normal, centroid, 0 (frames.MEMBRANE_FIELDS)
FORCE_WORDS = 40  # sph_force_measure record (frames.FORCE_FIELDS)
FORCE_DIAG_WORDS = 64  # sph_force_diagnostics record (frames.FORCE_DIAG_FIELDS)
WALL_WORDS = 32  # sph_wall_measure record (frames.WALL_FIELDS)
WALL_DIAG_WORDS = 32  # sph_wall_diagnostics record (frames.WALL_DIAG_FIELDS)
BODY_STATE_WORDS = 48  # sph_bodies_advance record per slot (BODY_STATE_FIELDS)
MAX_GAUGES = 16  # SPH_MAX_GAUGES: flow-gauge slots per solver
GAUGE_WORDS = 16  # sph_gauges_accumulate record per gauge (frames.GAUGE_FIELDS)
GAUGE_TOTAL_WORDS = 20  # sph_gauges_read totals per gauge (frames.GAUGE_TOTAL_FIELDS)
GAUGE_HISTORY_MAX = 16384
GAUGE_PLANE = 1  # sph_gauge.flags
PROBE_MAX_POINTS = 65536  # SPH_PROBE_MAX_POINTS
PROBE_MAX_LINES = 65536  # SPH_PROBE_MAX_LINES
PROBE_LINE_MAX = 1024  # points of one line
PROBE_LEVEL_WORDS = 8  # sph_probes_record record per line (frames.LEVEL_FIELDS); a point record is a sample record
PROBE_HISTORY_MAX = 16384
PROBE_HISTORY_BYTES = 1 << 28  # rows * row bytes of the ring
PROBE_FOUND, PROBE_DRY, PROBE_SUBMERGED = 0, 1, 2  # word 4 of a level record
MAX_STATS = 4  # SPH_MAX_STATS: time-statistics slots per solver
STATS_WORDS = 24  # float64 accumulators per lattice node (STATS_FIELDS)
STATS_MOMENT_WORDS = 16  # sph_stats_read_moments floats per node (STATS_MOMENT_FIELDS)
STATS_BYTES_MAX = 1 << 31  # accumulators of one slot
# the accumulators of a node (include/sphmi.h, sph_stats_*): sums over the wet calls, call indices, extremes
STATS_FIELDS = ("wet_calls", "first_wet_call", "last_wet_call", "sum_rho", "sum_rho2", "sum_vx", "sum_vy", "sum_vz", "sum_vxvx",
                "sum_vyvy", "sum_vzvz", "sum_vxvy", "sum_vxvz", "sum_vyvz", "sum_p", "sum_p2", "max_rho", "max_rho_call",
                "max_speed2", "max_speed2_call", "max_p", "max_p_call", "min_p", "min_p_call")
STATS_MOMENT_FIELDS = ("wet_fraction", "mean_rho", "var_rho", "mean_vx", "mean_vy", "mean_vz", "cov_xx", "cov_yy", "cov_zz", "cov_xy",
                       "cov_xz", "cov_yz", "mean_p", "var_p", "arrival_call", "peak_p")
# word ranges of that record (include/sphmi.h): name -> (first word, count)
BODY_STATE_FIELDS = {"status": (0, 1), "members": (1, 1), "advances": (2, 1), "max_move": (3, 1), "position": (4, 3),
                     "orientation": (7, 4), "velocity": (11, 3), "angular_momentum": (14, 3), "omega": (17, 3), "load_force": (20, 3),
                     "load_torque": (23, 3), "n_contact": (26, 1), "n_share": (27, 1), "offenders": (28, 1), "lowest_member": (29, 1)}
WALL_ALL, WALL_NO_BODY = -1, -2  # the wall set in place of a body slot: every boundary particle / those that belong to no body
FIELD_SLOTS = 4  # carried particle fields per solver (sph_field_*)
FIELD_DIAG_WORDS = 8  # sph_field_diagnostics record (frames.FIELD_DIAG_FIELDS)
TRACE_TIME, TRACE_ARC = 0, 1  # sph_trace_params.mode
TRACE_EULER, TRACE_MIDPOINT = 0, 1  # sph_trace_params.integrator
# why a curve stopped (sph_trace_streamlines status; a tracer that has not stopped is TRACE_MOVING)
TRACE_MOVING, TRACE_MAX_STEPS, TRACE_LEFT_MATTER, TRACE_LEFT_REGION, TRACE_STAGNANT, TRACE_NONFINITE = 0, 1, 2, 3, 4, 5
TRACE_MAX_STEPS_LIMIT = 65535
TRACE_MODES = ("time", "arc")
TRACE_INTEGRATORS = ("euler", "midpoint")
MAX_NEIGHBOR_COUNT = 32
LIQUID_PARTICLE, ELASTIC_PARTICLE, BOUNDARY_PARTICLE = 1, 2, 3

STAGE_NAMES = ["hash", "sort", "sort_post", "index", "find_neighbors", "density", "forces", "elastic",
               "predict_density", "pressure_force", "integrate", "membranes", "bands"]


class SphConfig(C.Structure):
    _fields_ = [("abi_version", C.c_int32), ("particleCount", C.c_int32), ("capacity", C.c_int32),
                ("gridCellsX", C.c_int32), ("gridCellsY", C.c_int32), ("gridCellsZ", C.c_int32),
                ("gridCellCount", C.c_int32), ("cellIdMask", C.c_uint32)] + \
               [(n, C.c_float) for n in
                ["h", "hashGridCellSize", "hashGridCellSizeInv", "simulationScale", "simulationScaleInv",
                 "xmin", "xmax", "ymin", "ymax", "zmin", "zmax", "r0", "mass", "rho0", "timeStep", "viscosity",
                 "delta", "gravity_x", "gravity_y", "gravity_z", "surfTensCoeff"]] + \
               [(n, C.c_double) for n in ["Wpoly6Coefficient", "gradWspikyCoefficient", "del2WviscosityCoefficient"]] + \
               [(n, C.c_int32) for n in ["numOfElasticP", "elasticOffset", "muscleCount", "numOfMembranes",
                                         "maxIteration", "device"]] + \
               [("stream", C.c_void_p)]


class SphSlab(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ["layerLo", "layerHi", "ghostLayers", "hasLower", "hasUpper", "globalIdBits"]]


SLAB_RECORD_WORDS = 9
SLAB_COMPACT_WORDS = 7  # x, y, z, vx, vy, vz, global id (sph_slab_set_record_format)


class SphSelectTerm(C.Structure):
    _fields_ = [("field", C.c_int32), ("lo", C.c_float), ("hi", C.c_float)]


class SphRenderView(C.Structure):
    """sph_render_view of include/sphmi.h (frames.render_view fills one)."""
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("projection", C.c_int32),
                ("eye", C.c_float * 3), ("right", C.c_float * 3), ("up", C.c_float * 3), ("forward", C.c_float * 3),
                ("scale", C.c_float), ("centre", C.c_float * 2), ("nearPlane", C.c_float), ("radius", C.c_float),
                ("maxRadiusPx", C.c_float), ("colourMode", C.c_int32), ("field", C.c_int32), ("lo", C.c_float), ("hi", C.c_float),
                ("typeColour", (C.c_float * 3) * 3), ("ambient", C.c_float), ("background", C.c_uint8 * 4)]


RENDER_COLOUR_MODES = ("type", "density", "field", "label")  # sph_render_view.colourMode 0..3


class SphRenderMeshStyle(C.Structure):
    """sph_render_mesh_style of include/sphmi.h (owHIPSolver.render_mesh fills one)."""
    _fields_ = [("source", C.c_int32), ("shading", C.c_int32), ("colourMode", C.c_int32), ("field", C.c_int32),
                ("lo", C.c_float), ("hi", C.c_float), ("colour", C.c_float * 3), ("compose", C.c_int32)]


RENDER_MESH_SOURCES = ("surface", "membranes")  # sph_render_mesh_style.source 0..1
RENDER_MESH_SHADINGS = ("flat", "smooth")  # sph_render_mesh_style.shading 0..1
RENDER_MESH_SURFACE_FIELDS = ("density", "shepard", "vx", "vy", "vz", "pressure", "speed")  # field 0..6 with source 0


class SphTraceParams(C.Structure):
    """sph_trace_params of include/sphmi.h (owHIPSolver.streamlines / tracers_advect fill one)."""
    _fields_ = [("step", C.c_float), ("minSpeed", C.c_float), ("maxSteps", C.c_int32), ("mode", C.c_int32), ("integrator", C.c_int32)]


class SphBodyDynamics(C.Structure):
    """sph_body_dynamics of include/sphmi.h (owHIPSolver.body_set_dynamics fills one, body_dynamics returns its fields)."""
    _fields_ = [("mass", C.c_double), ("com", C.c_double * 3), ("inertiaInv", C.c_double * 6), ("position", C.c_double * 3),
                ("orientation", C.c_double * 4), ("velocity", C.c_double * 3), ("angularMomentum", C.c_double * 3),
                ("spin", C.c_double * 3), ("gravity", C.c_double * 3), ("force", C.c_double * 3), ("torque", C.c_double * 3),
                ("contactGain", C.c_double), ("forceGain", C.c_double), ("locks", C.c_uint32)]


class SphGauge(C.Structure):
    _fields_ = [("origin", C.c_float * 3), ("u", C.c_float * 3), ("v", C.c_float * 3), ("typeMask", C.c_uint32),
                ("fieldSlot", C.c_int32), ("flags", C.c_uint32)]


class SphProbeLine(C.Structure):
    """sph_probe_line of include/sphmi.h (frames.level_columns builds arrays of PROBE_LINE_DTYPE, the same 40 bytes)."""
    _fields_ = [("origin", C.c_float * 3), ("step", C.c_float * 3), ("count", C.c_int32), ("field", C.c_int32), ("iso", C.c_float),
                ("typeMask", C.c_uint32)]


# the same record as a numpy dtype: what probes_set_lines reads and probe_lines returns
PROBE_LINE_DTYPE = np.dtype([("origin", np.float32, 3), ("step", np.float32, 3), ("count", np.int32), ("field", np.int32),
                             ("iso", np.float32), ("typeMask", np.uint32)])


class SphStatsLattice(C.Structure):
    """sph_stats_lattice of include/sphmi.h (STATS_LATTICE_DTYPE is the same 40 bytes)."""
    _fields_ = [("origin", C.c_float * 3), ("spacing", C.c_float * 3), ("dims", C.c_int32 * 3), ("typeMask", C.c_uint32)]


STATS_LATTICE_DTYPE = np.dtype([("origin", np.float32, 3), ("spacing", np.float32, 3), ("dims", np.int32, 3), ("typeMask", np.uint32)])


class SphError(RuntimeError):
    pass


_host = None
_dev = None


def host_lib():
    global _host
    if _host is None:
        if not os.path.exists(HOST_LIB_PATH):
            raise SphError("libsphmi_host.so not built (run `python -c 'import __graft_entry__ as g; g.build()'`)")
        L = C.CDLL(HOST_LIB_PATH)
        L.sphmi_default_config.argtypes = [C.POINTER(SphConfig)]
        L.sphmi_config_set_box.argtypes = [C.POINTER(SphConfig), C.c_double, C.c_double, C.c_double, C.c_uint32]
        L.sphmi_count_particles.argtypes = [C.c_char_p]
        L.sphmi_load_configuration.argtypes = [C.c_char_p, C.c_char_p, C.c_int, C.c_void_p, C.c_void_p,
                                               C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]
        L.sphmi_load_elastic_connections.argtypes = [C.c_char_p, C.c_int, C.c_void_p]
        L.sphmi_box_counts.argtypes = [C.POINTER(SphConfig), C.c_double, C.c_double, C.c_double, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int),
                                       C.POINTER(C.c_int)]
        L.sphmi_generate_box.argtypes = [C.POINTER(SphConfig), C.c_double, C.c_double, C.c_double, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float,
                                         C.c_float, C.c_float, C.c_float, C.c_uint64, C.c_void_p, C.c_void_p]
        _box = [C.POINTER(SphConfig), C.c_double, C.c_double, C.c_double, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float,
                C.c_float, C.c_float, C.c_float, C.c_uint64]
        L.sphmi_box_layer_histogram.argtypes = _box + [C.c_void_p, C.c_int]
        L.sphmi_generate_box_slice.argtypes = _box + [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_int)]
        L.sphmi_muscle_signal.argtypes = [C.c_int, C.c_void_p, C.c_int]
        L.sphmi_step_chunk_edges.argtypes = [C.c_int64, C.c_int32, C.c_void_p]
        L.sphmi_step_pipeline_schedule.argtypes = [C.c_int32] * 4 + [C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(C.c_int32)]
        L.sphmi_step_halo_check.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int32, C.c_int32, C.c_int32]
        L.sphmi_step_band_defer_first.argtypes = [C.c_int32]
        L.sphmi_trajectory_info.argtypes = [C.c_char_p] + [C.POINTER(C.c_int)] * 4
        L.sphmi_trajectory_frame.argtypes = [C.c_char_p, C.c_int, C.c_void_p]
        L.sphmi_trajectory_connections.argtypes = [C.c_char_p, C.c_int, C.c_void_p]
        L.sphmi_trajectory_membranes.argtypes = [C.c_char_p, C.c_int, C.c_void_p]
        L.sphmi_worm_counts.argtypes = [C.POINTER(SphConfig), C.c_double, C.c_double, C.c_double] + [C.POINTER(C.c_int)] * 4
        L.sphmi_generate_worm.argtypes = [C.POINTER(SphConfig), C.c_double, C.c_double, C.c_double] + [C.c_void_p] * 5
        L.sphmi_save_configuration.argtypes = [C.c_char_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                               C.c_int, C.c_int]
        _host = L
    return _host


_STAGE_FUNCS = ["sph_run_clear_buffers", "sph_run_hash_particles", "sph_run_sort", "sph_run_sort_post_pass",
                "sph_run_indexx", "sph_run_index_post_pass", "sph_run_find_neighbors",
                "sph_run_pcisph_compute_density", "sph_run_pcisph_compute_forces_and_init_pressure",
                "sph_run_pcisph_compute_elastic_forces", "sph_run_pcisph_predict_positions",
                "sph_run_pcisph_predict_density", "sph_run_pcisph_correct_pressure",
                "sph_run_pcisph_compute_pressure_force_acceleration", "sph_run_clear_membrane_buffers",
                "sph_run_compute_interaction_with_membranes", "sph_run_compute_interaction_with_membranes_finalize"]
EXPORTED_SYMBOLS = ["sph_create", "sph_destroy", "sph_run_pcisph_integrate", "sph_step", "sph_update_muscles",
                    "sph_read_position", "sph_read_velocity", "sph_read_density", "sph_read_particle_index",
                    "sph_read_position_async", "sph_read_position_wait", "sph_host_unregister", "sph_build_info",
                    "sph_read_buffer", "sph_read_neighbor_rows", "sph_synchronize", "sph_set_stage_timing", "sph_get_stage_times",
                    "sph_reset_stage_times", "sph_step_sort_passes", "sph_set_step_chunks", "sph_set_step_pipeline", "sph_set_wave_skip", "sph_set_search_bands", "sph_last_error", "sph_abi_version", "sph_slab_init", "sph_slab_pack", "sph_slab_pack_framed", "sph_slab_step_begin", "sph_slab_step_messages",
                    "sph_slab_rebuild", "sph_particle_count", "sph_slab_read", "sph_slab_rebuild_framed", "sph_slab_rebuild_finish",
                    "sph_slab_liquid_signature", "sph_slab_set_record_format", "sph_stream_wait_event", "sph_sample_points",
                    "sph_sample_grid", "sph_extract_surface", "sph_read_surface", "sph_sample_gradient_points",
                    "sph_sample_gradient_grid", "sph_surface_normals", "sph_measure_surface", "sph_read_shells", "sph_diagnostics", "sph_histogram", "sph_label_components",
                    "sph_read_components", "sph_component_diagnostics", "sph_particle_measure", "sph_select_particles",
                    "sph_read_selection", "sph_elastic_measure", "sph_muscle_diagnostics", "sph_membrane_measure",
                    "sph_render_particles", "sph_read_render", "sph_render_mesh", "sph_read_render_triangles", "sph_force_measure", "sph_force_diagnostics", "sph_remove_region",
                    "sph_remove_selection", "sph_remove_ids", "sph_add_particles", "sph_emit_lattice", "sph_read_edit_map", "sph_field_create",
                    "sph_field_release", "sph_field_write", "sph_field_read", "sph_field_set_region", "sph_field_set_selection",
                    "sph_field_diffuse", "sph_field_diagnostics", "sph_trace_streamlines", "sph_tracers_set", "sph_tracers_advect",
                    "sph_tracers_read", "sph_body_define_ids", "sph_body_define_region", "sph_body_release", "sph_body_count",
                    "sph_body_read", "sph_body_set_pose", "sph_wall_measure", "sph_wall_diagnostics", "sph_body_set_dynamics",
                    "sph_body_get_dynamics", "sph_bodies_advance", "sph_gauge_define", "sph_gauge_get", "sph_gauges_accumulate",
                    "sph_gauges_read", "sph_gauges_reset", "sph_gauges_history", "sph_gauges_read_history", "sph_gauge_crossings",
                    "sph_read_gauge_crossings", "sph_probes_set_points", "sph_probes_set_lines", "sph_probes_count", "sph_probes_record",
                    "sph_probes_history", "sph_probes_read_history", "sph_stats_define", "sph_stats_get", "sph_stats_accumulate",
                    "sph_stats_reset", "sph_stats_read", "sph_stats_read_moments", "sph_bin_diagnostics", "sph_bin_index"] + _STAGE_FUNCS
HOST_EXPORTED_SYMBOLS = ["sphmi_default_config", "sphmi_config_set_box", "sphmi_count_particles",
                         "sphmi_load_configuration", "sphmi_load_elastic_connections", "sphmi_box_counts",
                         "sphmi_generate_box", "sphmi_box_layer_histogram", "sphmi_generate_box_slice", "sphmi_muscle_signal", "sphmi_step_chunk_edges", "sphmi_step_pipeline_schedule", "sphmi_step_halo_check", "sphmi_step_band_defer_first", "sphmi_save_configuration", "sphmi_worm_counts",
                         "sphmi_generate_worm", "sphmi_trajectory_info", "sphmi_trajectory_frame", "sphmi_trajectory_connections",
                         "sphmi_trajectory_membranes"]


def hip_runtimes_loaded():
    """Paths of every libamdhip64 mapped into this process (two of them do not both see the GPU)."""
    paths = set()
    try:
        with open("/proc/self/maps") as f:
            for line in f:
                if "libamdhip64" in line:
                    paths.add(line.split()[-1])
    except OSError:
        pass
    return sorted(paths)


def _bind_one_hip_runtime():
    """PyTorch-ROCm ships its own libamdhip64 (same SONAME as /opt/rocm's). Whichever copy is mapped first serves every
    later user, so if none is loaded yet and torch is installed, map torch's copy now — by path, without importing torch —
    and libsphmi.so, a later `import torch` and RCCL all share it, whatever the import order."""
    if hip_runtimes_loaded():
        return
    import importlib.util
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    if spec and spec.submodule_search_locations:
        cand = os.path.join(list(spec.submodule_search_locations)[0], "lib", "libamdhip64.so")
        if os.path.exists(cand):
            C.CDLL(cand, mode=C.RTLD_GLOBAL)


def device_lib():
    """Load libsphmi.so (the HIP solver). Raises if it has not been built — there is no fallback."""
    global _dev
    if _dev is None:
        if not os.path.exists(LIB_PATH):
            raise SphError("libsphmi.so not built: the HIP extension is required (no CPU fallback exists)")
        _bind_one_hip_runtime()
        L = C.CDLL(LIB_PATH)
        L.sph_create.argtypes = [C.POINTER(SphConfig), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                 C.POINTER(C.c_void_p)]
        L.sph_destroy.argtypes = [C.c_void_p]
        for f in _STAGE_FUNCS + ["sph_synchronize", "sph_reset_stage_times", "sph_step_sort_passes"]:
            getattr(L, f).argtypes = [C.c_void_p]
        L.sph_run_pcisph_integrate.argtypes = [C.c_void_p, C.c_int]
        L.sph_step.argtypes = [C.c_void_p, C.c_int]
        L.sph_update_muscles.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
        for f in ["sph_read_position", "sph_read_velocity", "sph_read_density", "sph_read_particle_index", "sph_read_position_async",
                  "sph_host_unregister"]:
            getattr(L, f).argtypes = [C.c_void_p, C.c_void_p]
        L.sph_read_position_wait.argtypes = [C.c_void_p]
        L.sph_build_info.restype = C.c_char_p
        L.sph_read_buffer.argtypes = [C.c_void_p, C.c_char_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]
        L.sph_read_neighbor_rows.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]
        L.sph_set_stage_timing.argtypes = [C.c_void_p, C.c_int]
        L.sph_set_step_chunks.argtypes = [C.c_void_p, C.c_int32]
        if hasattr(L, "sph_set_step_pipeline"):  # (optional: an A/B library built from an older csrc/ has no pipelined step)
            L.sph_set_step_pipeline.argtypes = [C.c_void_p, C.c_int32]
        if hasattr(L, "sph_set_wave_skip"):  # (optional, likewise)
            L.sph_set_wave_skip.argtypes = [C.c_void_p, C.c_int32]
        if hasattr(L, "sph_set_search_bands"):  # (optional, likewise)
            L.sph_set_search_bands.argtypes = [C.c_void_p, C.c_int32]
        L.sph_get_stage_times.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_int64), C.c_int]
        L.sph_last_error.restype = C.c_char_p
        L.sph_slab_init.argtypes = [C.c_void_p, C.POINTER(SphSlab), C.c_void_p]
        L.sph_slab_pack.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(C.c_int32)]
        L.sph_slab_pack_framed.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(C.c_int32)]
        L.sph_slab_step_begin.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int32]
        L.sph_slab_step_messages.argtypes = [C.c_void_p, C.POINTER(C.c_int32)]
        L.sph_slab_rebuild.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32]
        L.sph_slab_rebuild_framed.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32]
        L.sph_slab_rebuild_finish.argtypes = [C.c_void_p, C.POINTER(C.c_int32)]
        L.sph_slab_liquid_signature.argtypes = [C.c_void_p, C.POINTER(C.c_uint32)]
        L.sph_slab_set_record_format.argtypes = [C.c_void_p, C.c_int32, C.c_uint32]
        L.sph_stream_wait_event.argtypes = [C.c_void_p, C.c_void_p]
        L.sph_particle_count.argtypes = [C.c_void_p]
        L.sph_slab_read.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.sph_sample_points.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_uint32, C.c_void_p]
        L.sph_sample_grid.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]
        L.sph_extract_surface.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_int32, C.c_float,
                                          C.c_void_p]
        L.sph_read_surface.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.sph_sample_gradient_points.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_uint32, C.c_void_p]
        L.sph_sample_gradient_grid.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]
        L.sph_surface_normals.argtypes = [C.c_void_p, C.c_void_p]
        L.sph_measure_surface.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.sph_read_shells.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.sph_diagnostics.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_uint32, C.c_void_p]
        L.sph_histogram.argtypes = [C.c_void_p, C.c_int32, C.c_float, C.c_float, C.c_int32, C.c_void_p, C.c_uint32, C.c_void_p]
        L.sph_label_components.argtypes = [C.c_void_p, C.c_float, C.c_uint32, C.c_void_p]
        L.sph_read_components.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.sph_component_diagnostics.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]
        L.sph_particle_measure.argtypes = [C.c_void_p, C.c_void_p]
        L.sph_select_particles.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]
        L.sph_read_selection.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.sph_elastic_measure.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.sph_muscle_diagnostics.argtypes = [C.c_void_p, C.c_void_p]
        L.sph_membrane_measure.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.sph_force_measure.argtypes = [C.c_void_p, C.c_int32, C.c_void_p]
        L.sph_force_diagnostics.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_uint32, C.c_void_p]
        L.sph_render_particles.argtypes = [C.c_void_p, C.POINTER(SphRenderView), C.c_void_p, C.c_uint32, C.c_int32, C.c_void_p]
        L.sph_read_render.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.sph_render_mesh.argtypes = [C.c_void_p, C.POINTER(SphRenderView), C.POINTER(SphRenderMeshStyle), C.c_void_p]
        L.sph_read_render_triangles.argtypes = [C.c_void_p, C.c_void_p]
        L.sph_remove_region.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_int32, C.c_void_p]
        L.sph_remove_selection.argtypes = [C.c_void_p, C.c_void_p]
        L.sph_remove_ids.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]
        L.sph_add_particles.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32]
        L.sph_emit_lattice.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_void_p]
        L.sph_read_edit_map.argtypes = [C.c_void_p, C.c_void_p]
        L.sph_field_create.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_float]
        L.sph_field_release.argtypes = [C.c_void_p, C.c_int32]
        L.sph_field_write.argtypes = [C.c_void_p, C.c_int32, C.c_void_p]
        L.sph_field_read.argtypes = [C.c_void_p, C.c_int32, C.c_void_p]
        L.sph_field_set_region.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_uint32, C.c_float, C.c_void_p]
        L.sph_field_set_selection.argtypes = [C.c_void_p, C.c_int32, C.c_float, C.c_void_p]
        L.sph_field_diffuse.argtypes = [C.c_void_p, C.c_int32, C.c_float, C.c_int32, C.c_uint32, C.c_void_p]
        L.sph_field_diagnostics.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_uint32, C.c_void_p]
        L.sph_trace_streamlines.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_uint32, C.POINTER(SphTraceParams), C.c_void_p,
                                            C.c_void_p, C.c_void_p, C.c_void_p]
        L.sph_tracers_set.argtypes = [C.c_void_p, C.c_void_p, C.c_int32]
        L.sph_tracers_advect.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(SphTraceParams), C.c_void_p, C.c_void_p]
        L.sph_tracers_read.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        if hasattr(L, "sph_body_set_pose"):  # (optional: an A/B library built from an older csrc/ has no kinematic bodies)
            L.sph_body_define_ids.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_int64]
            L.sph_body_define_region.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]
            L.sph_body_release.argtypes = [C.c_void_p, C.c_int32]
            L.sph_body_count.argtypes = [C.c_void_p, C.c_int32, C.c_void_p]
            L.sph_body_read.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
            L.sph_body_set_pose.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        if hasattr(L, "sph_bodies_advance"):  # (optional: an A/B library built from an older csrc/ has no free bodies)
            L.sph_body_set_dynamics.argtypes = [C.c_void_p, C.c_int32, C.c_void_p]
            L.sph_body_get_dynamics.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]
            L.sph_bodies_advance.argtypes = [C.c_void_p, C.c_void_p]
        if hasattr(L, "sph_wall_measure"):  # (optional: an A/B library built from an older csrc/ has no wall loads)
            L.sph_wall_measure.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]
            L.sph_wall_diagnostics.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_uint32, C.c_void_p]
        if hasattr(L, "sph_gauges_accumulate"):  # (optional: an A/B library built from an older csrc/ has no flow gauges)
            L.sph_gauge_define.argtypes = [C.c_void_p, C.c_int32, C.c_void_p]
            L.sph_gauge_get.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]
            L.sph_gauges_accumulate.argtypes = [C.c_void_p, C.c_void_p]
            L.sph_gauges_read.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
            L.sph_gauges_reset.argtypes = [C.c_void_p, C.c_int32]
            L.sph_gauges_history.argtypes = [C.c_void_p, C.c_int32]
            L.sph_gauges_read_history.argtypes = [C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p]
            L.sph_gauge_crossings.argtypes = [C.c_void_p, C.c_int32, C.c_void_p]
            L.sph_read_gauge_crossings.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        if hasattr(L, "sph_probes_record"):  # (optional: an A/B library built from an older csrc/ has no probes)
            L.sph_probes_set_points.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_uint32]
            L.sph_probes_set_lines.argtypes = [C.c_void_p, C.c_void_p, C.c_int32]
            L.sph_probes_count.argtypes = [C.c_void_p, C.c_void_p]
            L.sph_probes_record.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
            L.sph_probes_history.argtypes = [C.c_void_p, C.c_int32]
            L.sph_probes_read_history.argtypes = [C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
        if hasattr(L, "sph_stats_accumulate"):  # (optional: an A/B library built from an older csrc/ has no time statistics)
            L.sph_stats_define.argtypes = [C.c_void_p, C.c_int32, C.c_void_p]
            L.sph_stats_get.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
            L.sph_stats_accumulate.argtypes = [C.c_void_p, C.c_int32]
            L.sph_stats_reset.argtypes = [C.c_void_p, C.c_int32]
            L.sph_stats_read.argtypes = [C.c_void_p, C.c_int32, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p]
            L.sph_stats_read_moments.argtypes = [C.c_void_p, C.c_int32, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p]
        if hasattr(L, "sph_bin_diagnostics"):  # (optional: an A/B library built from an older csrc/ has no binned diagnostics)
            L.sph_bin_diagnostics.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
            L.sph_bin_index.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        _dev = L
    return _dev


# ----------------------------------------------------------------------------- host helpers
def default_config():
    cfg = SphConfig()
    rc = host_lib().sphmi_default_config(C.byref(cfg))
    if rc:
        raise SphError("sphmi_default_config failed: %d" % rc)
    cfg._box_in_h = (30.0, 20.0, 250.0)  # owPhysicsConstant.h:32-37
    return cfg


def set_box(cfg, xmax_in_h, ymax_in_h, zmax_in_h, cell_id_mask=0xffff):
    rc = host_lib().sphmi_config_set_box(C.byref(cfg), xmax_in_h, ymax_in_h, zmax_in_h, cell_id_mask)
    if rc:
        raise SphError("sphmi_config_set_box failed: %d" % rc)
    cfg._box_in_h = (float(xmax_in_h), float(ymax_in_h), float(zmax_in_h))
    return cfg


def config_dict(cfg):
    """sph_config as a dict with the oracle's key names (oracle/oraclebind.make_params)."""
    d = {n: getattr(cfg, n) for n, _ in SphConfig._fields_ if n not in ("stream",)}
    d["N"] = d["particleCount"]
    return d


def load_configuration(position_file, velocity_file):
    """owHelper::preLoadConfiguration + loadConfiguration (owHelper.cpp:1431-1545)."""
    n = host_lib().sphmi_count_particles(position_file.encode())
    if n <= 0:
        raise SphError("cannot read %s" % position_file)
    pos = np.empty((n, 4), np.float32)
    vel = np.empty((n, 4), np.float32)
    nl, ne, nb = C.c_int(), C.c_int(), C.c_int()
    rc = host_lib().sphmi_load_configuration(position_file.encode(), velocity_file.encode(), n, pos.ctypes.data,
                                             vel.ctypes.data, C.byref(nl), C.byref(ne), C.byref(nb))
    if rc:
        raise SphError("sphmi_load_configuration failed: %d" % rc)
    return pos, vel, dict(numOfLiquidP=nl.value, numOfElasticP=ne.value, numOfBoundaryP=nb.value)


def generate_box(cfg, lx, ly, lz, spacing=None, origin=None, jitter=0.0, seed=20261004):
    """Synthetic pure-liquid box of SURVEY §8(d): liquid lattice + reference boundary shell. Sets cfg.particleCount."""
    nl, nb = C.c_int(), C.c_int()
    bx = cfg._box_in_h
    rc = host_lib().sphmi_box_counts(C.byref(cfg), bx[0], bx[1], bx[2], lx, ly, lz, C.byref(nl), C.byref(nb))
    if rc:
        raise SphError("sphmi_box_counts failed: %d" % rc)
    n = nl.value + nb.value
    r0 = np.float32(cfg.r0)
    if spacing is None:
        spacing = np.float32(0.93) * r0
    if origin is None:
        origin = (np.float32(3) * r0,) * 3
    pos = np.empty((n, 4), np.float32)
    vel = np.empty((n, 4), np.float32)
    rc = host_lib().sphmi_generate_box(C.byref(cfg), bx[0], bx[1], bx[2], lx, ly, lz, spacing, origin[0], origin[1], origin[2], jitter,
                                       seed, pos.ctypes.data, vel.ctypes.data)
    if rc:
        raise SphError("sphmi_generate_box failed: %d" % rc)
    cfg.particleCount = n
    return pos, vel, dict(numOfLiquidP=nl.value, numOfElasticP=0, numOfBoundaryP=nb.value)


def _box_args(cfg, lx, ly, lz, spacing, origin, jitter, seed):
    bx = cfg._box_in_h
    r0 = np.float32(cfg.r0)
    if spacing is None:
        spacing = np.float32(0.93) * r0
    if origin is None:
        origin = (np.float32(3) * r0,) * 3
    return [C.byref(cfg), bx[0], bx[1], bx[2], lx, ly, lz, spacing, origin[0], origin[1], origin[2], jitter, seed]


def box_counts(cfg, lx, ly, lz):
    """(numOfLiquidP, numOfBoundaryP) of generate_box without generating anything."""
    nl, nb = C.c_int(), C.c_int()
    bx = cfg._box_in_h
    rc = host_lib().sphmi_box_counts(C.byref(cfg), bx[0], bx[1], bx[2], lx, ly, lz, C.byref(nl), C.byref(nb))
    if rc:
        raise SphError("sphmi_box_counts failed: %d" % rc)
    return nl.value, nb.value


def box_layer_histogram(cfg, lx, ly, lz, spacing=None, origin=None, jitter=0.0, seed=20261004):
    """Particles of generate_box's scene per z cell layer (int64[gridCellsZ]) — what balanced_cuts_hist needs — without
    materialising the scene."""
    hist = np.zeros(cfg.gridCellsZ, np.int64)
    rc = host_lib().sphmi_box_layer_histogram(*_box_args(cfg, lx, ly, lz, spacing, origin, jitter, seed), hist.ctypes.data, hist.size)
    if rc:
        raise SphError("sphmi_box_layer_histogram failed: %d" % rc)
    return hist


def generate_box_slice(cfg, lx, ly, lz, layer_lo, layer_hi, spacing=None, origin=None, jitter=0.0, seed=20261004):
    """The rows of generate_box's scene whose z cell layer lies in [layer_lo, layer_hi), with their global ids (ascending):
    (position, velocity, global_ids). Does not touch cfg.particleCount."""
    args = _box_args(cfg, lx, ly, lz, spacing, origin, jitter, seed) + [int(max(layer_lo, -(1 << 30))), int(min(layer_hi, 1 << 30))]
    n = C.c_int()
    rc = host_lib().sphmi_generate_box_slice(*args, None, None, None, 0, C.byref(n))
    if rc:
        raise SphError("sphmi_generate_box_slice failed: %d" % rc)
    pos, vel, gid = np.empty((n.value, 4), np.float32), np.empty((n.value, 4), np.float32), np.empty(n.value, np.uint32)
    rc = host_lib().sphmi_generate_box_slice(*args, pos.ctypes.data, vel.ctypes.data, gid.ctypes.data, n.value, C.byref(n))
    if rc:
        raise SphError("sphmi_generate_box_slice failed: %d" % rc)
    return pos, vel, gid


def generate_worm(cfg):
    """The reference's generated worm scene (owHelper::generateConfiguration) for cfg's box. Sets
    cfg.particleCount / numOfElasticP / numOfMembranes / elasticOffset and returns a scene dict."""
    bx = cfg._box_in_h
    ne, nl, nb, nm = C.c_int(), C.c_int(), C.c_int(), C.c_int()
    rc = host_lib().sphmi_worm_counts(C.byref(cfg), bx[0], bx[1], bx[2], C.byref(ne), C.byref(nl), C.byref(nb), C.byref(nm))
    if rc:
        raise SphError("sphmi_worm_counts failed: %d" % rc)
    n = ne.value + nl.value + nb.value
    pos = np.empty((n, 4), np.float32)
    vel = np.empty((n, 4), np.float32)
    elastic = np.empty((ne.value * 32, 4), np.float32)
    membranes = np.empty((nm.value, 3), np.int32)
    pml = np.empty((ne.value, 7), np.int32)
    rc = host_lib().sphmi_generate_worm(C.byref(cfg), bx[0], bx[1], bx[2], pos.ctypes.data, vel.ctypes.data, elastic.ctypes.data,
                                        membranes.ctypes.data, pml.ctypes.data)
    if rc:
        raise SphError("sphmi_generate_worm failed: %d" % rc)
    cfg.particleCount, cfg.numOfElasticP, cfg.numOfMembranes, cfg.elasticOffset = n, ne.value, nm.value, 0
    return dict(cfg=cfg, position=pos, velocity=vel, elastic=elastic, membranes=membranes, particle_membranes=pml,
                numOfLiquidP=nl.value, numOfElasticP=ne.value, numOfBoundaryP=nb.value)


def save_configuration(directory, position, num_elastic, num_liquid, connections=None, membranes=None, first=True):
    """owHelper::loadConfigurationToFile (owHelper.cpp:1640-1672): the `-l_to` trajectory dump."""
    pos = np.ascontiguousarray(position, np.float32)
    con = None if connections is None else np.ascontiguousarray(connections, np.float32)
    mem = None if membranes is None else np.ascontiguousarray(membranes, np.int32)
    rc = host_lib().sphmi_save_configuration(directory.encode(), pos.ctypes.data, pos.shape[0], num_elastic, num_liquid,
                                             None if con is None else con.ctypes.data,
                                             None if mem is None else mem.ctypes.data,
                                             0 if mem is None else mem.shape[0], int(first))
    if rc:
        raise SphError("sphmi_save_configuration failed: %d" % rc)


def load_trajectory(directory):
    """owHelper::loadConfigurationFromFile (owHelper.cpp:1674-1741): read back a `-l_to` dump. Returns a dict with
    numOfElasticP, numOfLiquidP, frames[F, P, 4] and, when present, connections[32*E, 4] and membranes[M, 4]."""
    L = host_lib()
    ne, nl, nf, nm = C.c_int(), C.c_int(), C.c_int(), C.c_int()
    d = directory.encode()
    if L.sphmi_trajectory_info(d, C.byref(ne), C.byref(nl), C.byref(nf), C.byref(nm)):
        raise SphError("no trajectory in %s" % directory)
    P = ne.value + nl.value
    frames = np.empty((nf.value, P, 4), np.float32)
    for f in range(nf.value):
        if L.sphmi_trajectory_frame(d, f, frames[f].ctypes.data):
            raise SphError("trajectory frame %d unreadable" % f)
    out = dict(numOfElasticP=ne.value, numOfLiquidP=nl.value, frames=frames, connections=None, membranes=None)
    if ne.value:
        con = np.empty((32 * ne.value, 4), np.float32)
        if L.sphmi_trajectory_connections(d, ne.value, con.ctypes.data) == 0:
            out["connections"] = con
    if nm.value:
        mem = np.empty((nm.value, 4), np.int32)
        if L.sphmi_trajectory_membranes(d, nm.value, mem.ctypes.data) == 0:
            out["membranes"] = mem
    return out


def muscle_signal(step, muscle_count=100):
    out = np.zeros(muscle_count, np.float32)
    rc = host_lib().sphmi_muscle_signal(step, out.ctypes.data, muscle_count)
    if rc:
        raise SphError("sphmi_muscle_signal failed: %d" % rc)
    return out


def step_chunk_edges(n, chunks):
    """The chunks + 1 edges of the ranges of sorted particles that the overlapped step launches by (host library, no GPU)."""
    if n < 0 or chunks < 1:
        raise SphError("step_chunk_edges: n >= 0 and chunks >= 1")
    out = np.zeros(chunks + 1, np.int64)
    rc = host_lib().sphmi_step_chunk_edges(n, chunks, out.ctypes.data)
    if rc:
        raise SphError("sphmi_step_chunk_edges failed: %d" % rc)
    return out


def step_pipeline_schedule(chunks, depth, max_iteration=3, has_elastic=False):
    """(clamped depth, [(stage, chunk), ...]): the launches of the pipelined step's chunk stream in issue order (host library, no
    GPU). Stage 0 is a chunk's density pass and record pack, 1 the forces kernel, 2j + 1 / 2j + 2 the predicted density / the
    pressure force of iteration j."""
    if chunks < 1 or not 0 <= depth <= 6 or max_iteration < 0:
        raise SphError("step_pipeline_schedule: chunks >= 1, 0 <= depth <= 6, max_iteration >= 0")
    cap = 7 * chunks
    stage, chunk = np.zeros(cap, np.int32), np.zeros(cap, np.int32)
    clamped = C.c_int32(-1)
    n = host_lib().sphmi_step_pipeline_schedule(chunks, depth, max_iteration, int(bool(has_elastic)), stage.ctypes.data,
                                                chunk.ctypes.data, cap, C.byref(clamped))
    if n < 0:
        raise SphError("sphmi_step_pipeline_schedule failed: %d" % n)
    return clamped.value, [(int(a), int(b)) for a, b in zip(stage[:n], chunk[:n])]


def step_band_defer_first(chunks):
    """The first chunk whose search-band records the overlapped step scatters beside the first search launches (host library, no
    GPU): the prelude scatters chunks [0, result), search chunks 0 .. result - 2 start at the fork, every later one behind the
    deferred scatter. `chunks` where nothing is deferred."""
    rc = host_lib().sphmi_step_band_defer_first(int(chunks))
    if rc < 0:
        raise SphError("sphmi_step_band_defer_first failed: %d" % rc)
    return rc


def step_halo_check(keys, cell_start, edges, gx, gy):
    """The pipelined step's halo check restated on the host: True if, judged from the sorted cell ids and the cell table
    (G + 1 entries) alone, every possible neighbour of a particle of chunk c of the partition `edges` lies in chunks c - 1 .. c + 1."""
    keys = np.ascontiguousarray(keys, np.uint32)
    cell_start = np.ascontiguousarray(cell_start, np.uint32)
    edges = np.ascontiguousarray(edges, np.int64)
    rc = host_lib().sphmi_step_halo_check(keys.ctypes.data, keys.size, cell_start.ctypes.data, cell_start.size - 1, edges.ctypes.data,
                                          edges.size - 1, int(gx), int(gy))
    if rc < 0:
        raise SphError("sphmi_step_halo_check failed: %d" % rc)
    return bool(rc)


# ----------------------------------------------------------------------------- device solver
_BUF_DTYPE = {"position": np.float32, "velocity": np.float32, "sortedPosition": np.float32,
              "sortedVelocity": np.float32, "acceleration": np.float32, "neighborMap": np.float32,
              "neighborIds": np.int32, "particleIndex": np.uint32, "particleIndexBack": np.uint32,
              "gridCellIndex": np.uint32, "gridCellIndexFixedUp": np.uint32, "pressure": np.float32,
              "rho": np.float32, "debugCounters": np.uint32, "diagnosticTrace": np.uint32,
              "pressureForceSkipped": np.uint8, "predictDensitySkipped": np.uint8,
              "pressureNeighbourhood": np.uint8, "movedNeighbourhood": np.uint8, "pressureFlags": np.uint8, "movedFlags": np.uint8,
              "searchBandFlags": np.uint8, "searchBands": np.float32, "searchBandStart": np.uint32}


def type_mask(types):
    """Particle types (1 liquid, 2 elastic, 3 boundary) -> the typeMask bit set of sph_sample_*; other values are passed on
    as bits for the library to reject."""
    m = 0
    for t in types:
        m |= 1 << int(t)
    return m & 0xffffffff


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _points4(points, what):
    """Query points ([Q, 3] or [Q, 4]) as the float32[Q, 4] array the sph_sample_*_points calls read."""
    pts = np.asarray(points, np.float32)
    pts = pts.reshape(-1, pts.shape[-1]) if pts.ndim else pts.reshape(-1, 1)
    if pts.shape[1] not in (3, 4):
        raise SphError("%s: points must be [Q, 3] or [Q, 4]" % what)
    p4 = np.zeros((pts.shape[0], 4), np.float32)
    p4[:, :3] = pts[:, :3]
    return p4


def _lattice(origin, spacing, dims):
    """A lattice's (origin, spacing, dims) as the three arrays the grid calls read."""
    return (np.ascontiguousarray(origin, np.float32).reshape(3), np.ascontiguousarray(spacing, np.float32).reshape(3),
            np.ascontiguousarray(dims, np.int32).reshape(3))


def _region(region, what):
    """One region (x0, y0, z0, x1, y1, z1; None = everywhere) as the float32[6] the calls read, or None."""
    if region is None:
        return None
    rg = np.ascontiguousarray(region, np.float32)
    if rg.size != 6:
        raise SphError("%s: region must be (x0, y0, z0, x1, y1, z1)" % what)
    return rg


def _regions(regions, what):
    """A list of regions (None = one region holding everything) as float32[R, 6]."""
    if regions is None:
        regions = [(-np.inf,) * 3 + (np.inf,) * 3]
    rg = np.ascontiguousarray(regions, np.float32)
    if rg.size % 6:
        raise SphError("%s: regions must be [R, 6]" % what)
    return rg.reshape(-1, 6)


def _field_index(field, names, what):
    """A field given by its name in `names` or by its number -> the number (the library checks a number's range)."""
    if isinstance(field, str):
        if field not in names:
            raise SphError("%s: field must be one of %s" % (what, names))
        field = names.index(field)
    return int(field)


def stats_lattice(origin, spacing, dims, types=(1,)):
    """A statistics lattice as the one-element STATS_LATTICE_DTYPE array stats_define reads: origin and spacing of 3 floats, dims
    (nx, ny, nz) of 3 ints (anything else is refused here), the types as a mask for the library to judge."""
    o, sp, dm = np.asarray(origin, np.float32), np.asarray(spacing, np.float32), np.asarray(dims)
    if o.size != 3 or sp.size != 3 or dm.size != 3:
        raise SphError("stats_define: origin, spacing and dims must hold 3 values each")
    if dm.dtype.kind not in "iu":
        raise SphError("stats_define: dims must be integers")
    if (np.abs(dm.astype(np.int64)) > 0x7fffffff).any():
        raise SphError("stats_define: dims do not fit 32 bits")
    g = np.zeros(1, STATS_LATTICE_DTYPE)
    g["origin"], g["spacing"], g["dims"], g["typeMask"] = o.reshape(3), sp.reshape(3), dm.reshape(3), type_mask(types)
    return g


def bin_lattice(origin, spacing, dims, types=(1, 2)):
    """A lattice of bins as the one-element STATS_LATTICE_DTYPE array bin_diagnostics and bin_index read (sph_bin_lattice has the
    layout of sph_stats_lattice): edge i of axis a is origin[a] + (float32)i * spacing[a], bin (i, j, k) is the half-open box
    between consecutive edges, dims = (nx, ny, nz). dims 1 with spacing 0 is the whole axis. Shapes and integer dims are checked
    here, everything else by the library. frames.bin_edges / bin_boxes give the edges and the boxes."""
    o, sp, dm = np.asarray(origin, np.float32), np.asarray(spacing, np.float32), np.asarray(dims)
    if o.size != 3 or sp.size != 3 or dm.size != 3:
        raise SphError("bin_lattice: origin, spacing and dims must hold 3 values each")
    if dm.dtype.kind not in "iu":
        raise SphError("bin_lattice: dims must be integers")
    if (np.abs(dm.astype(np.int64)) > 0x7fffffff).any():
        raise SphError("bin_lattice: dims do not fit 32 bits")
    g = np.zeros(1, STATS_LATTICE_DTYPE)
    g["origin"], g["spacing"], g["dims"], g["typeMask"] = o.reshape(3), sp.reshape(3), dm.reshape(3), type_mask(types)
    return g


def _bin_lattice(lattice, what):
    g = np.ascontiguousarray(lattice)
    if g.dtype != STATS_LATTICE_DTYPE or g.size != 1:
        raise SphError("%s: the lattice must be what bin_lattice() returns" % what)
    return g.reshape(1)


def probe_lines(lines):
    """Level-probe lines as the contiguous PROBE_LINE_DTYPE array probes_set_lines reads: an array of that dtype (any shape is
    refused but [L]), a SphProbeLine, or a sequence of SphProbeLine or of dicts (origin, step, count, field = name or 0..5, iso,
    types or typeMask). None or nothing: no lines."""
    from . import frames
    if lines is None:
        return np.zeros(0, PROBE_LINE_DTYPE)
    if isinstance(lines, np.ndarray):
        if lines.dtype != PROBE_LINE_DTYPE or lines.ndim != 1:
            raise SphError("probes_set_lines: a line array must be [L] of PROBE_LINE_DTYPE (40 bytes a line)")
        return np.ascontiguousarray(lines)
    if isinstance(lines, (SphProbeLine, dict)):
        lines = [lines]
    out = np.zeros(len(lines), PROBE_LINE_DTYPE)
    for i, ln in enumerate(lines):
        if isinstance(ln, SphProbeLine):
            out[i] = (tuple(ln.origin), tuple(ln.step), ln.count, ln.field, ln.iso, ln.typeMask)
            continue
        if not isinstance(ln, dict):
            raise SphError("probes_set_lines: line %d is neither a SphProbeLine nor a dict" % i)
        for name in ("origin", "step"):
            a = np.asarray(ln[name], np.float32).reshape(-1)
            if a.size != 3:
                raise SphError("probes_set_lines: line %d: %s must hold 3 floats" % (i, name))
            out[i][name] = a
        out[i]["count"] = int(ln["count"])
        out[i]["field"] = _field_index(ln.get("field", "shepard"), frames.GRID_FIELDS[:SURFACE_FIELDS], "probes_set_lines")
        out[i]["iso"] = np.float32(ln.get("iso", 0.5))
        out[i]["typeMask"] = int(ln["typeMask"]) if "typeMask" in ln else type_mask(ln.get("types", (1,)))
    return out


def build_info():
    """sph_build_info() of the loaded libsphmi.so ("DIAG" in it: a timing-only variant with invalid results)."""
    return device_lib().sph_build_info().decode()


class owHIPSolver:
    """Counterpart of owOpenCLSolver (src/owOpenCLSolver.h:28-62): same methods, backed by libsphmi.so."""

    def __init__(self, cfg, position_cpp, velocity_cpp, elasticConnectionsData_cpp=None, membraneData_cpp=None,
                 particleMembranesList_cpp=None):
        self._L = device_lib()
        self.cfg = cfg
        self.N = cfg.particleCount
        pos = np.ascontiguousarray(position_cpp, np.float32)
        vel = np.ascontiguousarray(velocity_cpp, np.float32)
        if pos.size != 4 * self.N or vel.size != 4 * self.N:
            raise SphError("position/velocity must hold 4*particleCount floats")
        el = None if elasticConnectionsData_cpp is None else np.ascontiguousarray(elasticConnectionsData_cpp, np.float32)
        mb = None if membraneData_cpp is None else np.ascontiguousarray(membraneData_cpp, np.int32)
        pm = None if particleMembranesList_cpp is None else np.ascontiguousarray(particleMembranesList_cpp, np.int32)
        # the C ABI sees pointers only: the lengths the library will read are checked here
        for name, a, want, rule in (("elasticConnectionsData", el, 4 * 32 * cfg.numOfElasticP, "4*32*numOfElasticP"),
                                    ("membraneData", mb, 3 * cfg.numOfMembranes, "3*numOfMembranes"),
                                    ("particleMembranesList", pm, 7 * cfg.numOfElasticP, "7*numOfElasticP")):
            if a is not None and a.size != max(want, 0):
                raise SphError("%s holds %d words, the configuration asks for %s = %d" % (name, a.size, rule, want))
        h = C.c_void_p()
        self._chk(self._L.sph_create(C.byref(cfg), _ptr(pos), _ptr(vel), _ptr(el), _ptr(mb), _ptr(pm), C.byref(h)))
        self._h = h

    def _chk(self, rc):
        if rc != 0:
            raise SphError("libsphmi: %s (status %d)" % (self._L.sph_last_error().decode(), rc))
        return 0

    def close(self):
        if getattr(self, "_h", None):
            self._L.sph_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # --- owOpenCLSolver::_run* (owOpenCLSolver.h:37-56) ---
    def _runClearBuffers(self): return self._chk(self._L.sph_run_clear_buffers(self._h))
    def _runHashParticles(self): return self._chk(self._L.sph_run_hash_particles(self._h))
    def _runSort(self): return self._chk(self._L.sph_run_sort(self._h))
    def _runSortPostPass(self): return self._chk(self._L.sph_run_sort_post_pass(self._h))
    def _runIndexx(self): return self._chk(self._L.sph_run_indexx(self._h))
    def _runIndexPostPass(self): return self._chk(self._L.sph_run_index_post_pass(self._h))
    def _runFindNeighbors(self): return self._chk(self._L.sph_run_find_neighbors(self._h))
    def _run_pcisph_computeDensity(self): return self._chk(self._L.sph_run_pcisph_compute_density(self._h))
    def _run_pcisph_computeForcesAndInitPressure(self): return self._chk(self._L.sph_run_pcisph_compute_forces_and_init_pressure(self._h))
    def _run_pcisph_computeElasticForces(self): return self._chk(self._L.sph_run_pcisph_compute_elastic_forces(self._h))
    def _run_pcisph_predictPositions(self): return self._chk(self._L.sph_run_pcisph_predict_positions(self._h))
    def _run_pcisph_predictDensity(self): return self._chk(self._L.sph_run_pcisph_predict_density(self._h))
    def _run_pcisph_correctPressure(self): return self._chk(self._L.sph_run_pcisph_correct_pressure(self._h))
    def _run_pcisph_computePressureForceAcceleration(self): return self._chk(self._L.sph_run_pcisph_compute_pressure_force_acceleration(self._h))
    def _run_pcisph_integrate(self, iterationCount): return self._chk(self._L.sph_run_pcisph_integrate(self._h, iterationCount))
    def _run_clearMembraneBuffers(self): return self._chk(self._L.sph_run_clear_membrane_buffers(self._h))
    def _run_computeInteractionWithMembranes(self): return self._chk(self._L.sph_run_compute_interaction_with_membranes(self._h))
    def _run_computeInteractionWithMembranes_finalize(self): return self._chk(self._L.sph_run_compute_interaction_with_membranes_finalize(self._h))

    def updateMuscleActivityData(self, signal):
        s = np.ascontiguousarray(signal, np.float32)
        return self._chk(self._L.sph_update_muscles(self._h, _ptr(s), s.size))

    def read_position_buffer(self, out=None):
        out = np.empty((self.N, 4), np.float32) if out is None else out
        self._chk(self._L.sph_read_position(self._h, _ptr(out)))
        return out

    def read_position_buffer_async(self, out):
        """read_position_buffer without the wait (sph_read_position_async): the copy runs under the next step; `out` (C-contiguous
        float32, 4N) is valid after wait_position_buffer(). The array is page-locked in place on first use and kept alive here."""
        if not (isinstance(out, np.ndarray) and out.dtype == np.float32 and out.flags.c_contiguous and out.size == 4 * self.N):
            raise SphError("read_position_buffer_async needs a C-contiguous float32 array of 4*N elements")
        self._async_out = out
        self._chk(self._L.sph_read_position_async(self._h, _ptr(out)))
        return out

    def wait_position_buffer(self):
        return self._chk(self._L.sph_read_position_wait(self._h))

    def read_velocity_buffer(self, out=None):
        out = np.empty((self.N, 4), np.float32) if out is None else out
        self._chk(self._L.sph_read_velocity(self._h, _ptr(out)))
        return out

    def read_density_buffer(self, out=None):
        out = np.empty(self.N, np.float32) if out is None else out
        self._chk(self._L.sph_read_density(self._h, _ptr(out)))
        return out

    def read_particleIndex_buffer(self, out=None):
        out = np.empty((self.N, 2), np.uint32) if out is None else out
        self._chk(self._L.sph_read_particle_index(self._h, _ptr(out)))
        return out

    # --- field sampling (sph_sample_points / sph_sample_grid): the sorted state of the last completed step ---
    def sample_points(self, points, types=(1, 2, 3)):
        """SPH interpolation at `points` ([Q, 3] or [Q, 4], scene units) over the particles of the given types:
        float32[Q, 8] records (density, shepard, vx, vy, vz, pressure, count, 0), include/sphmi.h."""
        p4 = _points4(points, "sample_points")
        out = np.empty((p4.shape[0], SAMPLE_WORDS), np.float32)
        self._chk(self._L.sph_sample_points(self._h, _ptr(p4), p4.shape[0], type_mask(types), _ptr(out)))
        return out

    def sample_grid(self, origin, spacing, dims, types=(1, 2, 3)):
        """The same on the lattice origin + (float)i * spacing, i < dims = (nx, ny, nz): float32[nz, ny, nx, 8]."""
        o, sp, dm = _lattice(origin, spacing, dims)
        size = int(dm[0]) * int(dm[1]) * int(dm[2]) if (dm > 0).all() else 0
        out = np.empty((max(int(dm[2]), 0), max(int(dm[1]), 0), max(int(dm[0]), 0), SAMPLE_WORDS) if size else (1, SAMPLE_WORDS),
                       np.float32)
        self._chk(self._L.sph_sample_grid(self._h, _ptr(o), _ptr(sp), _ptr(dm), type_mask(types), _ptr(out)))
        return out

    # --- isosurface extraction (sph_extract_surface / sph_read_surface): marching cubes over a sampled field ---
    def extract_surface(self, origin, spacing, dims, iso=0.5, field="shepard", types=(1,)):
        """Triangle mesh of {f >= iso} for word `field` (a name from frames.GRID_FIELDS[:6] or 0..5) of sample_grid(origin,
        spacing, dims, types), extracted on the device: (vertices float32[V, 3], triangles int32[T, 3]), triangles wound with
        normals toward lower f (include/sphmi.h)."""
        from . import frames
        field = _field_index(field, frames.GRID_FIELDS[:SURFACE_FIELDS], "extract_surface")
        o, sp, dm = _lattice(origin, spacing, dims)
        counts = np.zeros(2, np.int64)
        self._mesh_vertices = 0  # (a failed extraction leaves no mesh behind)
        self._shells = 0  # (and any extraction drops the measure of the mesh before)
        self._chk(self._L.sph_extract_surface(self._h, _ptr(o), _ptr(sp), _ptr(dm), type_mask(types), int(field), float(iso),
                                              _ptr(counts)))
        self._mesh_vertices = int(counts[0])
        verts = np.empty((int(counts[0]), 3), np.float32)
        tris = np.empty((int(counts[1]), 3), np.int32)
        self._chk(self._L.sph_read_surface(self._h, _ptr(verts) if verts.size else None, _ptr(tris) if tris.size else None))
        return verts, tris

    # --- gradient sampling (sph_sample_gradient_points / sph_sample_gradient_grid) and surface normals ---
    def sample_gradient_points(self, points, types=(1, 2, 3)):
        """sample_points with the SPH gradients: float32[Q, 32] records (the 8 sample words, grad rho, grad shepard, grad u
        row-major, grad p, vorticity, divergence, Q, 0; frames.GRADIENT_FIELDS, include/sphmi.h). Gradients are per metre of
        simulation-scaled space."""
        p4 = _points4(points, "sample_gradient_points")
        out = np.empty((p4.shape[0], GRADIENT_WORDS), np.float32)
        self._chk(self._L.sph_sample_gradient_points(self._h, _ptr(p4), p4.shape[0], type_mask(types), _ptr(out)))
        return out

    def sample_gradient_grid(self, origin, spacing, dims, types=(1, 2, 3)):
        """The same on sample_grid's lattice: float32[nz, ny, nx, 32]."""
        o, sp, dm = _lattice(origin, spacing, dims)
        size = int(dm[0]) * int(dm[1]) * int(dm[2]) if (dm > 0).all() else 0
        out = np.empty((int(dm[2]), int(dm[1]), int(dm[0]), GRADIENT_WORDS) if size else (1, GRADIENT_WORDS), np.float32)
        self._chk(self._L.sph_sample_gradient_grid(self._h, _ptr(o), _ptr(sp), _ptr(dm), type_mask(types), _ptr(out)))
        return out

    def surface_normals(self):
        """float32[V, 3] unit normals (toward lower f) of the vertices of the last extract_surface, from the gradient of the
        contoured field at each vertex; (0, 0, 0) where that gradient vanishes. Refused once the solver has stepped since."""
        n = getattr(self, "_mesh_vertices", 0)  # 0 without a mesh: the library reports SPH_ERR_ORDER
        out = np.empty((n, 3), np.float32)
        self._chk(self._L.sph_surface_normals(self._h, _ptr(out) if out.size else None))
        return out

    # --- surface measures (sph_measure_surface / sph_read_shells): shells, area and enclosed volume of the extracted mesh ---
    def measure_surface(self):
        """Measure the mesh of the last extract_surface on the device: the shells it consists of (connected pieces: drops,
        cavities, sheets cut by the lattice border), their open sides, and per shell exact integer sums of area, signed volume
        and area moment (include/sphmi.h). Returns {"shells", "closed", "open_sides", "bad_triangles", "kA", "kV", "kM"}; the
        table stays on the device until the next extract_surface (surface_shells()). Legal after further steps: it is a
        function of the mesh alone. frames.shell_summary turns the table into areas, volumes and centroids."""
        counts = np.zeros(4, np.int64)
        exps = np.zeros(3, np.int32)
        self._shells = 0  # (a failed measure leaves none behind)
        self._chk(self._L.sph_measure_surface(self._h, _ptr(counts), _ptr(exps)))
        self._shells = int(counts[0])
        return {"shells": int(counts[0]), "closed": int(counts[1]), "open_sides": int(counts[2]), "bad_triangles": int(counts[3]),
                "kA": int(exps[0]), "kV": int(exps[1]), "kM": int(exps[2])}

    def surface_shells(self):
        """The last measure_surface: (vertexShell int32[V], table int64[S, 10], bbox float32[S, 6]); the table's columns are
        named by SHELL_FIELDS, bbox is min x, y, z, max x, y, z of each shell's vertices."""
        n = getattr(self, "_mesh_vertices", 0)
        c = getattr(self, "_shells", 0)  # 0 without a measure: the library reports SPH_ERR_ORDER
        vs = np.empty(n, np.int32)
        table = np.empty((c, SHELL_WORDS), np.int64)
        bb = np.empty((c, 6), np.float32)
        self._chk(self._L.sph_read_shells(self._h, _ptr(vs) if n else None, _ptr(table) if c else None, _ptr(bb) if c else None))
        return vs, table, bb

    # --- flow diagnostics (sph_diagnostics / sph_histogram): the sorted state of the last completed step ---
    def diagnostics(self, regions=None, types=(1, 2)):
        """Reductions over the particles of the given types inside each region (x0, y0, z0, x1, y1, z1; lower bounds
        inclusive, upper exclusive, +-inf allowed; None = one region holding everything): float64[R, 32] records named by
        frames.DIAG_FIELDS (count, sums of position, velocity, angular momentum, v2, density, squared density error and
        pressure, then extremes; include/sphmi.h). The sums are added in a fixed tree, so a record depends on the state and
        its region alone. The default types are the moving matter: a boundary particle's `velocity` holds the wall normal,
        so sums over type 3 are legal but are not momenta. frames.diagnostics_summary turns a record into physical numbers."""
        rg = _regions(regions, "diagnostics")
        out = np.zeros((max(rg.shape[0], 1), DIAG_WORDS), np.float64)
        self._chk(self._L.sph_diagnostics(self._h, _ptr(rg), rg.shape[0], type_mask(types), _ptr(out)))
        return out

    def histogram(self, field, lo, hi, bins, region=None, types=(1, 2)):
        """Distribution of one per-particle quantity (a name from HIST_FIELDS or 0..6) over the same selection as
        diagnostics(): uint32[bins + 2] = values below lo, `bins` equal bins of [lo, hi), values at or above hi.
        histogram("neighbors", 0, 33, 33)[1:-1] is the exact neighbour-count distribution."""
        field = _field_index(field, HIST_FIELDS, "histogram")
        rg = _region(region, "histogram")
        out = np.zeros(max(int(bins), 0) + 2, np.uint32)
        self._chk(self._L.sph_histogram(self._h, field, float(np.float32(lo)), float(np.float32(hi)), int(bins), _ptr(rg),
                                        type_mask(types), _ptr(out)))
        return out

    # --- binned diagnostics (sph_bin_diagnostics / sph_bin_index): maps and profiles of particle sums ---
    def bin_diagnostics(self, lattice):
        """float64[nz, ny, nx, 32]: the diagnostics() record of every bin of `lattice` (bin_lattice()), each bit for bit the record
        diagnostics() returns for the bin's box (frames.bin_boxes) with the lattice's types, in one call and without a pass over
        the particles per bin. A particle on an edge belongs to the upper bin; the counts add up to the count over the outer box.
        frames.bin_profile / bin_column_depth turn the records into means and depths."""
        g = _bin_lattice(lattice, "bin_diagnostics")
        nx, ny, nz = (int(x) for x in g["dims"][0])
        bins = nx * ny * nz if min(nx, ny, nz) > 0 and nx * ny * nz <= BIN_MAX_BINS else 0
        out = np.zeros((nz, ny, nx, DIAG_WORDS) if bins else (1, DIAG_WORDS), np.float64)
        self._chk(self._L.sph_bin_diagnostics(self._h, _ptr(g), _ptr(out)))
        return out

    def bin_index(self, lattice):
        """int32[N], sorted order: the flat bin (k * ny + j) * nx + i of every particle under bin_diagnostics' rule, -1 for a
        particle that is unselected by type or key or lies in no bin."""
        g = _bin_lattice(lattice, "bin_index")
        out = np.empty(max(self.N, 1), np.int32)
        self._chk(self._L.sph_bin_index(self._h, _ptr(g), _ptr(out)))
        return out[:self.N]

    # --- connected components (sph_label_components / sph_read_components / sph_component_diagnostics) ---
    def label_components(self, link_radius=np.inf, types=(1, 2)):
        """Label the connected components of the graph of the last step's neighbour rows over the particles of the given types:
        two selected particles are linked when either has the other in its row and (for a finite `link_radius`, scene units)
        they are closer than it. Returns (n_selected, n_components); the labelling stays on the device until the next call
        (components(), component_diagnostics()). Components are numbered by ascending lowest sorted index (include/sphmi.h)."""
        counts = np.zeros(2, np.int64)
        self._components = 0  # (a failed labelling leaves none behind)
        self._chk(self._L.sph_label_components(self._h, float(np.float32(link_radius)), type_mask(types), _ptr(counts)))
        self._components = int(counts[1])
        return int(counts[0]), int(counts[1])

    def components(self):
        """The last labelling: labels int32[N] in sorted order (-1 = not selected), root_count int32[C, 2] (lowest sorted
        index, members), bbox float32[C, 6] (min x, y, z, max x, y, z). frames.labels_in_original_order maps the labels to
        the original particle order."""
        c = getattr(self, "_components", 0)  # 0 without a labelling: the library reports SPH_ERR_ORDER
        labels = np.empty(self.N, np.int32)
        rc = np.empty((c, 2), np.int32)
        bb = np.empty((c, 6), np.float32)
        self._chk(self._L.sph_read_components(self._h, _ptr(labels), _ptr(rc) if c else None, _ptr(bb) if c else None))
        return labels, rc, bb

    def component_diagnostics(self, ids):
        """float64[R, 32]: the diagnostics() record of the particles of each listed component (1..16 ids of the last labelling;
        ids may repeat). Refused once the solver has stepped since the labelling."""
        comp = np.ascontiguousarray(ids, np.int32).reshape(-1)
        out = np.zeros((max(comp.size, 1), DIAG_WORDS), np.float64)
        self._chk(self._L.sph_component_diagnostics(self._h, _ptr(comp) if comp.size else None, comp.size, _ptr(out)))
        return out[:comp.size]

    # --- particle selection (sph_particle_measure / sph_select_particles / sph_read_selection) ---
    def particle_measure(self):
        """float32[N], sorted order: the surface measure of every particle, the distance to the kernel-weighted centroid of the
        neighbours the last step used, in units of h (0 in a symmetric neighbourhood, 1 without neighbours; include/sphmi.h)."""
        out = np.empty(self.N, np.float32)
        self._chk(self._L.sph_particle_measure(self._h, _ptr(out)))
        return out

    def select(self, region=None, types=(1, 2), terms=(), component=None):
        """Select particles on the device: those diagnostics() selects for `region` and `types` that also satisfy every term
        (field, lo, hi) -- lo <= q < hi in float32, field a name from SELECT_FIELDS (HIST_FIELDS plus "surface", the
        particle_measure() value) or 0..7, +-inf allowed -- and, if `component` is given, belong to that component of the last
        label_components(). Returns the number selected; selection() reads them back. Up to 4 terms."""
        rg = _region(region, "select")
        terms = list(terms)
        arr = (SphSelectTerm * max(len(terms), 1))()
        for k, (field, lo, hi) in enumerate(terms):
            arr[k].field, arr[k].lo, arr[k].hi = _field_index(field, SELECT_FIELDS, "select"), float(np.float32(lo)), float(np.float32(hi))
        count = np.zeros(1, np.int64)
        self._selected = 0  # (a failed selection leaves none behind)
        self._chk(self._L.sph_select_particles(self._h, _ptr(rg), type_mask(types), C.cast(arr, C.c_void_p) if terms else None,
                                               len(terms), -1 if component is None else int(component), _ptr(count)))
        self._selected = int(count[0])
        return self._selected

    def select_surface(self, threshold=0.10, types=(1,)):
        """select() of the particles of `types` whose surface measure is at least `threshold` (the free surface of the liquid
        by default). 0.10 separates the outermost layer of a resting lattice from its interior; it is not calibrated for
        disordered flows -- look at particle_measure() first."""
        return self.select(types=types, terms=(("surface", threshold, np.inf),))

    def selection(self):
        """The last select(): (sorted_index int32[n] ascending, orig_id uint32[n], records float32[n, 12] named by
        frames.SELECT_FIELDS). Refused once the solver has stepped since the selection."""
        n = getattr(self, "_selected", 0)  # 0 without a selection: the library reports SPH_ERR_ORDER
        idx = np.empty(n, np.int32)
        ids = np.empty(n, np.uint32)
        rec = np.empty((n, SELECT_WORDS), np.float32)
        self._chk(self._L.sph_read_selection(self._h, _ptr(idx) if n else None, _ptr(ids) if n else None, _ptr(rec) if n else None))
        return idx, ids, rec

    # --- elastic-matter diagnostics (sph_elastic_measure / sph_muscle_diagnostics / sph_membrane_measure) ---
    def elastic_measure(self, connections=True):
        """Spring strain of every elastic particle in the state of the last completed step, rows in connection-table order:
        (sorted_index int32[E], orig_id uint32[E], records float32[E, 12] named by frames.ELASTIC_FIELDS -- live connections,
        those in a muscle group, min / max / sum of the strain (r - L0) / L0, sum of (r - L0)^2 and the spring and contraction
        accelerations the step applied -- and, unless connections=False, float32[E, 32, 2] holding (r, r - L0) per slot, (-1, 0)
        for an empty slot; None otherwise). Connections are directed: a spring listed from both ends counts twice
        (include/sphmi.h)."""
        E = int(self.cfg.numOfElasticP)
        idx = np.empty(E, np.int32)
        ids = np.empty(E, np.uint32)
        rec = np.empty((E, ELASTIC_WORDS), np.float32)
        con = np.empty((E, MAX_NEIGHBOR_COUNT, 2), np.float32) if connections else None
        self._chk(self._L.sph_elastic_measure(self._h, _ptr(idx) if E else None, _ptr(ids) if E else None, _ptr(rec) if E else None,
                                              _ptr(con) if (connections and E) else None))
        return idx, ids, rec, con

    def muscle_diagnostics(self):
        """float64[muscleCount + 1, 16] records named by frames.MUSCLE_FIELDS: record 0 the connections of no muscle group, record
        m those of muscle m (count, signal, sums of rest length, length, elongation, strain and forces, strain extremes, position
        sums of the owning ends). The sums are added in the fixed tree of diagnostics(), so a record depends on the state, the
        tables and the signal alone. frames.muscle_summary turns the records into per-group means."""
        out = np.zeros((int(self.cfg.muscleCount) + 1, MUSCLE_WORDS), np.float64)
        self._chk(self._L.sph_muscle_diagnostics(self._h, _ptr(out)))
        return out

    def membrane_measure(self, records=True):
        """(records float32[M, 8] -- area, unit normal, centroid, 0 per membrane triangle; None with records=False --,
        totals float64[4] = count, total area (fixed tree), min area, max area)."""
        M = int(self.cfg.numOfMembranes)
        rec = np.empty((M, MEMBRANE_WORDS), np.float32) if records else None
        totals = np.zeros(4, np.float64)
        self._chk(self._L.sph_membrane_measure(self._h, _ptr(rec) if (records and M) else None, _ptr(totals)))
        return rec, totals

    # --- force decomposition (sph_force_measure / sph_force_diagnostics) ---
    def force_measure(self, selection=False):
        """The viscous, surface-tension and pressure accelerations the last completed step computed for every sorted particle
        (selection=False: float32[N, 40]) or for the particles of the last select(), in its order (selection=True), kept apart
        by the class of the neighbour that exerted them: records named by frames.FORCE_FIELDS -- nine words per class (liquid,
        elastic, boundary), the three neighbour counts, the step's own viscous + gravity + tension acceleration and its
        pressure acceleration. Accelerations of the particle; times cfg.mass they are forces (include/sphmi.h).
        select(types=(2,)) then force_measure(selection=True) is the load on a body without exporting the liquid."""
        n = getattr(self, "_selected", 0) if selection else self.N  # without a selection the library reports SPH_ERR_ORDER
        out = np.zeros((n, FORCE_WORDS), np.float32)
        self._chk(self._L.sph_force_measure(self._h, 1 if selection else 0, _ptr(out) if n else None))
        return out

    def force_diagnostics(self, regions=None, types=(1, 2)):
        """Totals of force_measure() over the particles diagnostics() selects for each region: float64[R, 64] records named by
        frames.FORCE_DIAG_FIELDS (count, the 27 per-class sums, the step's two accelerations, torque about the origin and power
        per class, neighbour counts), added in the fixed tree of diagnostics(). frames.force_summary turns a record into
        newtons, newton metres and watts."""
        rg = _regions(regions, "force_diagnostics")
        out = np.zeros((max(rg.shape[0], 1), FORCE_DIAG_WORDS), np.float64)
        self._chk(self._L.sph_force_diagnostics(self._h, _ptr(rg), rg.shape[0], type_mask(types), _ptr(out)))
        return out

    # --- wall loads (sph_wall_measure / sph_wall_diagnostics) ---
    def wall_measure(self, slot, selection=False):
        """What the wall set `slot` (a body slot 0..15, WALL_ALL or WALL_NO_BODY) did to every sorted particle in the last
        completed step (selection=False: float32[N, 32]) or to the particles of the last select(), in its order: records named by
        frames.WALL_FIELDS -- the set's share of the position shift and of the velocity change of the contact inside integrate,
        the share and its weights, the set's nine K7 / K12 words of force_measure(), the position and velocity integrate stored,
        and the contact / reflected flags. Per unit mass: cfg.mass * dv / timeStep is the contact's force (include/sphmi.h)."""
        n = getattr(self, "_selected", 0) if selection else self.N  # without a selection the library reports SPH_ERR_ORDER
        out = np.zeros((n, WALL_WORDS), np.float32)
        self._chk(self._L.sph_wall_measure(self._h, int(slot), 1 if selection else 0, _ptr(out) if n else None))
        return out

    def wall_diagnostics(self, slot, regions=None, types=(1, 2)):
        """Totals of wall_measure(slot) over the particles diagnostics() selects for each region: float64[R, 32] records named by
        frames.WALL_DIAG_FIELDS, added in the fixed tree of diagnostics(). frames.wall_summary turns a record into newtons and
        newton metres on the liquid and, negated, on the body."""
        rg = _regions(regions, "wall_diagnostics")
        out = np.zeros((max(rg.shape[0], 1), WALL_DIAG_WORDS), np.float64)
        self._chk(self._L.sph_wall_diagnostics(self._h, int(slot), _ptr(rg), rg.shape[0], type_mask(types), _ptr(out)))
        return out

    # --- particle rendering (sph_render_particles / sph_read_render) ---
    def render(self, view, region=None, types=(1, 2), thickness=False):
        """Draw the particles of `types` inside `region` (as diagnostics(); the box doubles as a cut-away) as shaded spheres
        through `view` (an SphRenderView; frames.render_view makes one) into images kept on the device: nearest fragment per
        pixel, ties to the lower sorted index, and with thickness=True the summed chord of every fragment. Returns (particles
        drawn, covered pixels); rendered() reads the images. The state is the sorted state of the last completed step
        (include/sphmi.h)."""
        rg = _region(region, "render")
        counts = np.zeros(2, np.int64)
        self._render_shape = None  # (a failed render leaves no image behind)
        self._render_triangles = False
        self._chk(self._L.sph_render_particles(self._h, C.byref(view) if view is not None else None, _ptr(rg), type_mask(types),
                                               1 if thickness else 0, _ptr(counts)))
        self._render_shape = (int(view.height), int(view.width))
        return int(counts[0]), int(counts[1])

    def render_mesh(self, view, source="surface", shading="flat", colour=(0.8, 0.8, 0.8), field=None, lo=0.0, hi=1.0, compose=False):
        """Draw triangles through `view` into the images of render(): the mesh of the last extract_surface (source="surface") or
        the membrane triangles (source="membranes"), flat or (surface only) smooth shaded, two-sided, in the constant `colour`
        or, with `field` given, in the ramp of render()'s field mode over a per-vertex scalar between lo and hi (surface: a name
        from RENDER_MESH_SURFACE_FIELDS or 0..6, sampled at the vertices; membranes: a name from HIST_FIELDS or 0..6 of the
        corner particles). compose=True draws over the images of the last render by depth (same width .. near plane); otherwise
        the result is a fresh render. Returns (triangles drawn, triangles skipped, pixels the mesh holds, covered pixels);
        rendered(triangle=True) reads the images (include/sphmi.h)."""
        if not isinstance(view, SphRenderView):
            raise SphError("render_mesh: view must be an SphRenderView")
        st = SphRenderMeshStyle()
        st.source = _field_index(source, RENDER_MESH_SOURCES, "render_mesh")
        st.shading = _field_index(shading, RENDER_MESH_SHADINGS, "render_mesh")
        col = np.asarray(colour, np.float32).reshape(-1)
        if col.size != 3:
            raise SphError("render_mesh: colour holds %d values, not 3" % col.size)
        for k in range(3):
            st.colour[k] = float(col[k])
        if field is not None:
            st.colourMode = 1
            st.field = _field_index(field, HIST_FIELDS if st.source == 1 else RENDER_MESH_SURFACE_FIELDS, "render_mesh")
            st.lo, st.hi = float(lo), float(hi)
        if not isinstance(compose, (bool, np.bool_)):
            raise SphError("render_mesh: compose must be a bool")
        st.compose = 1 if compose else 0
        counts = np.zeros(4, np.int64)
        if not compose:
            self._render_shape = None  # (a failed fresh render leaves no image behind)
            self._render_triangles = False
        self._chk(self._L.sph_render_mesh(self._h, C.byref(view), C.byref(st), _ptr(counts)))
        self._render_shape = (int(view.height), int(view.width))
        self._render_triangles = True
        return tuple(int(c) for c in counts)

    def rendered(self, depth=True, index=True, orig_id=True, rgba=True, thickness=False, triangle=False):
        """The images of the last render() / render_mesh() as a dict of the ones asked for: depth float32[H, W] (+inf where
        uncovered), index int32[H, W] (the winner's sorted index, -1), orig_id uint32[H, W] (0xFFFFFFFF), rgba uint8[H, W, 4]
        (the view's background), thickness uint32[H, W] (units of radius / 128; frames.thickness_in_scene_units) and triangle
        int32[H, W] (the winning triangle of the last render_mesh, -1). They stay readable after further steps."""
        shape = getattr(self, "_render_shape", None) or (1, 1)  # without a render the library reports SPH_ERR_ORDER
        out = {}
        if depth: out["depth"] = np.empty(shape, np.float32)
        if index: out["index"] = np.empty(shape, np.int32)
        if orig_id: out["orig_id"] = np.empty(shape, np.uint32)
        if rgba: out["rgba"] = np.empty(shape + (4,), np.uint8)
        if thickness: out["thickness"] = np.empty(shape, np.uint32)
        self._chk(self._L.sph_read_render(self._h, *[_ptr(out.get(k)) for k in ("depth", "index", "orig_id", "rgba", "thickness")]))
        if triangle:
            out["triangle"] = np.empty(shape, np.int32)
            self._chk(self._L.sph_read_render_triangles(self._h, _ptr(out["triangle"])))
        return out

    # --- particle editing (sph_remove_* / sph_add_particles / sph_emit_lattice / sph_read_edit_map) ---
    def _edited(self):
        """Every wrapper sizes its outputs from self.N: refresh it, and forget what an edit invalidated."""
        n = self._L.sph_particle_count(self._h)
        if n != self.N:
            self._selected = 0
            self._components = 0
        self.N = n
        return n

    def remove_region(self, region=None, types=(1,), count_only=False):
        """Remove the particles of `types` whose current position (read_position_buffer's, original order) lies in the half-open
        box `region` (x0, y0, z0, x1, y1, z1; +-inf allowed; None = everywhere). The survivors keep their order; edit_map()
        tells where each went. Returns the number removed. With count_only=True nothing changes and the number that WOULD be
        removed is returned. An edit that changes the set invalidates the analysis state until the next step (include/sphmi.h)."""
        rg = _region(region, "remove_region")
        removed = np.zeros(1, np.int64)
        n0 = self.N
        self._chk(self._L.sph_remove_region(self._h, _ptr(rg), type_mask(types), 1 if count_only else 0, _ptr(removed)))
        if not count_only:
            self._map_len = n0
            self._edited()
        return int(removed[0])

    def remove_selection(self):
        """Remove the particles of the last select() (refused once the solver has stepped since). Returns the number removed."""
        removed = np.zeros(1, np.int64)
        n0 = self.N
        self._chk(self._L.sph_remove_selection(self._h, _ptr(removed)))
        self._map_len = n0
        self._edited()
        return int(removed[0])

    def remove_ids(self, ids):
        """Remove the particles with the listed original ids (duplicates allowed; an id >= N is refused). Returns the number
        removed."""
        a = np.ascontiguousarray(ids, np.int64).reshape(-1)
        if a.size and (a.min() < 0 or a.max() > 0xffffffff):
            raise SphError("remove_ids: ids must be unsigned 32-bit integers")
        a = a.astype(np.uint32)
        removed = np.zeros(1, np.int64)
        n0 = self.N
        self._chk(self._L.sph_remove_ids(self._h, _ptr(a) if a.size else None, a.size, _ptr(removed)))
        self._map_len = n0
        self._edited()
        return int(removed[0])

    def add_particles(self, position, velocity):
        """Append particles ([K, 4] each: x, y, z, type 1 or 3 / vx, vy, vz, 0) at ids N .. N+K-1. Returns the new count.
        Validated as the constructor validates; refused beyond cfg.capacity."""
        pos = np.ascontiguousarray(position, np.float32).reshape(-1, 4)
        vel = np.ascontiguousarray(velocity, np.float32).reshape(-1, 4)
        if pos.shape != vel.shape:
            raise SphError("add_particles: position and velocity must both be [K, 4]")
        k = pos.shape[0]
        self._chk(self._L.sph_add_particles(self._h, _ptr(pos) if k else None, _ptr(vel) if k else None, k))
        return self._edited()

    def emit_lattice(self, origin, spacing, dims, velocity=(0, 0, 0), type_value=1.0):
        """Append the lattice origin + (float)i * spacing, i < dims = (nx, ny, nz), x fastest, generated on the device, every
        particle with position.w = type_value and the given velocity. Returns the number added."""
        o, sp, dm = _lattice(origin, spacing, dims)
        v = np.ascontiguousarray(velocity, np.float32).reshape(3)
        added = np.zeros(1, np.int64)
        self._chk(self._L.sph_emit_lattice(self._h, _ptr(o), _ptr(sp), _ptr(dm), _ptr(v), float(np.float32(type_value)), _ptr(added)))
        self._edited()
        return int(added[0])

    def edit_map(self):
        """int32[count before the last removal]: the new id of every old particle, -1 for a removed one. Refused once a stage,
        a step or another edit has run since. frames.track_ids carries particle identities across edits with it."""
        # the count before the last SUCCESSFUL removal: a refused one leaves the library's map, and this length, as they were
        n = getattr(self, "_map_len", 0)  # 0 without a removal: the library reports SPH_ERR_ORDER
        out = np.empty(max(n, 1), np.int32)
        self._chk(self._L.sph_read_edit_map(self._h, _ptr(out)))
        return out[:n]

    # --- kinematic bodies (sph_body_*): groups of boundary particles placed by a pose between two steps ---
    def body_define_ids(self, slot, ids):
        """Make body `slot` (0..MAX_BODIES-1) of the boundary particles with the listed original ids, in that order; their current
        position and normal become the body's reference placement. An id >= N, a particle that is not a boundary particle and
        an id listed twice are refused. Returns the member count."""
        a = np.ascontiguousarray(ids, np.int64).reshape(-1)
        if a.size and (a.min() < 0 or a.max() > 0xffffffff):
            raise SphError("body_define_ids: ids must be unsigned 32-bit integers")
        a = a.astype(np.uint32)
        self._chk(self._L.sph_body_define_ids(self._h, int(slot), _ptr(a) if a.size else None, a.size))
        return int(a.size)

    def body_define_region(self, slot, region=None):
        """Make body `slot` of every boundary particle whose current position lies in the half-open box `region` (remove_region's
        compare; None = everywhere), in ascending original id. An empty result is refused. Returns the member count."""
        rg = _region(region, "body_define_region")
        count = np.zeros(1, np.int64)
        self._chk(self._L.sph_body_define_region(self._h, int(slot), _ptr(rg), _ptr(count)))
        return int(count[0])

    def body_release(self, slot):
        self._chk(self._L.sph_body_release(self._h, int(slot)))

    def body_count(self, slot):
        """The member count of body `slot`; 0 for a free slot."""
        count = np.zeros(1, np.int64)
        self._chk(self._L.sph_body_count(self._h, int(slot), _ptr(count)))
        return int(count[0])

    def body_read(self, slot):
        """(ids uint32[M], reference position float32[M, 4], reference normal float32[M, 4]) of body `slot`, in member order."""
        m = self.body_count(slot)
        ids, pos, nrm = np.empty(max(m, 1), np.uint32), np.empty((max(m, 1), 4), np.float32), np.empty((max(m, 1), 4), np.float32)
        self._chk(self._L.sph_body_read(self._h, int(slot), _ptr(ids), _ptr(pos), _ptr(nrm)))
        return ids[:m], pos[:m], nrm[:m]

    def body_set_pose(self, slot, pose):
        """Place the members of body `slot` at pose (float32[3, 4] = (R | t), frames.pose_*) applied to their REFERENCE placement:
        position and wall normal (include/sphmi.h states the float expression). All or nothing: if a new position is not finite,
        or with wide cell ids outside the box, nothing moves and the SphError carries `offenders` and `lowest_member`. Returns
        max_move, the largest displacement of a member against its current position in units of r0: from about 1 on the wall
        tunnels through liquid."""
        p = np.ascontiguousarray(pose, np.float32).reshape(-1)
        if p.size != 12:
            raise SphError("body_set_pose: pose must be 3 x 4 (R | t)")
        counts = np.zeros(2, np.int64)
        move = np.zeros(1, np.float32)
        rc = self._L.sph_body_set_pose(self._h, int(slot), _ptr(p), _ptr(counts[0:1]), _ptr(counts[1:2]), _ptr(move))
        if rc != 0:
            e = SphError("libsphmi: %s (status %d)" % (self._L.sph_last_error().decode(), rc))
            e.offenders, e.lowest_member = int(counts[0]), int(counts[1])
            raise e
        return np.float32(move[0])

    # --- free bodies (sph_body_set_dynamics / sph_bodies_advance): rigid-body dynamics driven by the wall loads ---
    _BODY_VEC = {"com": 3, "inertiaInv": 6, "position": 3, "orientation": 4, "velocity": 3, "angularMomentum": 3, "spin": 3,
                 "gravity": 3, "force": 3, "torque": 3}

    def body_set_dynamics(self, slot, **params):
        """Give body `slot` a dynamic state (include/sphmi.h: sph_body_dynamics; keyword = field name). `mass`, `com` and
        `position` are required; inertiaInv, velocity, angularMomentum, spin, force and torque default to zero, orientation to
        (1, 0, 0, 0), gravity to cfg.gravity_*, the gains to 1; `locks` is the bit word or a string of the letters x, y, z, r.
        With no keyword at all the body is kinematic again. Two dynamic bodies may not share a member."""
        if not params:
            self._chk(self._L.sph_body_set_dynamics(self._h, int(slot), None))
            return
        d = SphBodyDynamics()
        for need in ("mass", "com", "position"):
            if need not in params:
                raise SphError("body_set_dynamics: %s is required" % need)
        vals = {"orientation": (1.0, 0.0, 0.0, 0.0), "gravity": (self.cfg.gravity_x, self.cfg.gravity_y, self.cfg.gravity_z),
                "contactGain": 1.0, "forceGain": 1.0, "locks": 0}
        vals.update(params)
        for k, v in vals.items():
            if k in self._BODY_VEC:
                a = np.asarray(v, np.float64).reshape(-1)
                if a.size != self._BODY_VEC[k]:
                    raise SphError("body_set_dynamics: %s takes %d numbers" % (k, self._BODY_VEC[k]))
                setattr(d, k, (C.c_double * a.size)(*a))
            elif k in ("mass", "contactGain", "forceGain"):
                setattr(d, k, float(v))
            elif k == "locks":
                if isinstance(v, str):
                    if set(v) - set("xyzr"):
                        raise SphError("body_set_dynamics: locks is a string of the letters x, y, z, r")
                    v = sum(1 << "xyzr".index(ch) for ch in set(v))
                d.locks = int(v)
            else:
                raise SphError("body_set_dynamics: unknown parameter %s" % k)
        self._chk(self._L.sph_body_set_dynamics(self._h, int(slot), C.byref(d)))

    def body_dynamics(self, slot):
        """The live dynamic state of body `slot` as a dict of float64 arrays / numbers named like sph_body_dynamics, or None for
        a body that is not dynamic. Blocking."""
        d = SphBodyDynamics()
        flag = np.zeros(1, np.int32)
        self._chk(self._L.sph_body_get_dynamics(self._h, int(slot), C.byref(d), _ptr(flag)))
        if not flag[0]:
            return None
        out = {k: np.array(getattr(d, k), np.float64) for k in self._BODY_VEC}
        out.update(mass=d.mass, contactGain=d.contactGain, forceGain=d.forceGain, locks=int(d.locks))
        return out

    def bodies_advance(self, read=True):
        """One step of rigid-body dynamics for every dynamic body, on the GPU: the load of the last completed step on the body,
        the new state, the new placement of the members (include/sphmi.h states every operation). read=True waits once and returns
        float64[MAX_BODIES, 48] records (BODY_STATE_FIELDS); read=False enqueues everything and returns None without a wait."""
        if not read:
            self._chk(self._L.sph_bodies_advance(self._h, None))
            return None
        out = np.zeros((MAX_BODIES, BODY_STATE_WORDS), np.float64)
        self._chk(self._L.sph_bodies_advance(self._h, _ptr(out)))
        return out

    # --- flow gauges (sph_gauge_* / sph_gauges_*): particle crossings of oriented gates, per completed step ---
    def gauge_define(self, slot, origin=None, u=None, v=None, types=(1,), field=None, plane=False):
        """Define gauge `slot` (0..15) as the parallelogram origin + alpha u + beta v, 0 <= alpha, beta < 1 (plane=True: the whole
        plane), counting particles of `types` (1 liquid, 2 elastic) that cross it, positive along u x v; `field`: a carried field
        whose values the crossings sum, or None. origin=None releases the slot. A definition clears the slot's totals.
        frames.gauge_rect / frames.gauge_plane build the arguments: gauge_define(slot, **frames.gauge_rect(...))."""
        if origin is None:
            self._chk(self._L.sph_gauge_define(self._h, int(slot), None))
            return
        g = SphGauge()
        for name, val in (("origin", origin), ("u", u), ("v", v)):
            a = np.asarray(val, np.float32).reshape(-1)
            if a.size != 3:
                raise SphError("gauge_define: %s must hold 3 floats" % name)
            setattr(g, name, (C.c_float * 3)(*[float(x) for x in a]))
        g.typeMask = type_mask(types)
        g.fieldSlot = -1 if field is None else int(field)
        g.flags = GAUGE_PLANE if plane else 0
        self._chk(self._L.sph_gauge_define(self._h, int(slot), C.byref(g)))

    def gauge(self, slot):
        """The definition of gauge `slot` as a dict (origin, u, v float32[3]; typeMask; field or None; plane), or None."""
        g = SphGauge()
        flag = np.zeros(1, np.int32)
        self._chk(self._L.sph_gauge_get(self._h, int(slot), C.byref(g), _ptr(flag)))
        if not flag[0]:
            return None
        return dict(origin=np.array(g.origin, np.float32), u=np.array(g.u, np.float32), v=np.array(g.v, np.float32),
                    typeMask=int(g.typeMask), field=None if g.fieldSlot < 0 else int(g.fieldSlot), plane=bool(g.flags & GAUGE_PLANE))

    def gauges_accumulate(self, read=True):
        """The crossings of the last completed step through every defined gauge: added to the totals and the history on the device.
        read=True waits once and returns the records, float64[MAX_GAUGES, 16] (frames.GAUGE_FIELDS; a free slot is all zero);
        read=False enqueues everything and returns None without a wait. Once per step: a second call counts the step again."""
        if not read:
            self._chk(self._L.sph_gauges_accumulate(self._h, None))
            return None
        out = np.zeros((MAX_GAUGES, GAUGE_WORDS), np.float64)
        self._chk(self._L.sph_gauges_accumulate(self._h, _ptr(out)))
        return out

    def gauges(self):
        """(totals float64[MAX_GAUGES, 20] named by frames.GAUGE_TOTAL_FIELDS, the number of accumulate calls so far). Blocking."""
        out = np.zeros((MAX_GAUGES, GAUGE_TOTAL_WORDS), np.float64)
        calls = np.zeros(1, np.int64)
        self._chk(self._L.sph_gauges_read(self._h, _ptr(out), _ptr(calls)))
        return out, int(calls[0])

    def gauges_reset(self, slot=-1):
        """Clear the totals of gauge `slot`, or of all gauges."""
        self._chk(self._L.sph_gauges_reset(self._h, int(slot)))

    def gauges_history(self, rows):
        """Keep the records of the last `rows` accumulate calls in a ring on the device (0 releases it)."""
        self._chk(self._L.sph_gauges_history(self._h, int(rows)))

    def gauge_history(self, first, count):
        """float64[count, MAX_GAUGES, 16]: the records of accumulate calls first .. first + count - 1, while the ring holds them."""
        out = np.zeros((max(int(count), 1), MAX_GAUGES, GAUGE_WORDS), np.float64)
        self._chk(self._L.sph_gauges_read_history(self._h, int(first), int(count), _ptr(out), None))
        return out[:max(int(count), 0)]

    def gauge_crossings(self, slot):
        """The counted crossings of gauge `slot` in the last completed step, in ascending sorted index: (sorted index int32[n],
        original id uint32[n], direction int32[n] (+1, -1), float32[n, 3] of t, alpha, beta). The ids can go to remove_ids."""
        n = np.zeros(1, np.int64)
        self._chk(self._L.sph_gauge_crossings(self._h, int(slot), _ptr(n)))
        n = int(n[0])
        idx, ids, way = np.zeros(max(n, 1), np.int32), np.zeros(max(n, 1), np.uint32), np.zeros(max(n, 1), np.int32)
        tab = np.zeros((max(n, 1), 3), np.float32)
        self._chk(self._L.sph_read_gauge_crossings(self._h, _ptr(idx), _ptr(ids), _ptr(way), _ptr(tab)))
        return idx[:n], ids[:n], way[:n], tab[:n]

    # --- probes (sph_probes_*): point samples and water levels on lines, recorded per call, with a history ring on the device ---
    def probes_set_points(self, points, types=(1, 2, 3)):
        """Replace the point probes by `points` ([P, 3] or [P, 4]; None or nothing releases them), sampled over `types`."""
        p4 = _points4(points, "probes_set_points") if points is not None and np.size(points) else np.zeros((0, 4), np.float32)
        self._chk(self._L.sph_probes_set_points(self._h, _ptr(p4) if p4.size else None, p4.shape[0], type_mask(types)))

    def probes_set_lines(self, lines):
        """Replace the level probes by `lines` (see probe_lines; frames.level_columns builds them; None or nothing releases them)."""
        ln = probe_lines(lines)
        self._chk(self._L.sph_probes_set_lines(self._h, _ptr(ln) if ln.size else None, ln.shape[0]))

    def probes_count(self):
        """(point probes, level probes) the solver holds."""
        c = np.zeros(2, np.int32)
        self._chk(self._L.sph_probes_count(self._h, _ptr(c)))
        return int(c[0]), int(c[1])

    def probes_record(self, read=True):
        """Every probe's record of the last completed step, written to the history ring on the device. read=True waits once and
        returns (points float32[P, 8], the sample_points records; levels float32[L, 8], frames.LEVEL_FIELDS); read=False enqueues
        everything and returns None without a wait."""
        if not read:
            self._chk(self._L.sph_probes_record(self._h, None, None))
            return None
        P, L = self.probes_count()
        pts, lev = np.zeros((P, SAMPLE_WORDS), np.float32), np.zeros((L, PROBE_LEVEL_WORDS), np.float32)
        one = np.zeros(PROBE_LEVEL_WORDS, np.float32)  # (a non-NULL pointer even with nothing to copy: this call waits)
        self._chk(self._L.sph_probes_record(self._h, _ptr(pts) if P else _ptr(one), _ptr(lev) if L else _ptr(one)))
        return pts, lev

    def probes_history(self, rows):
        """Keep the records of the last `rows` probes_record calls in a ring on the device (0 releases it)."""
        self._chk(self._L.sph_probes_history(self._h, int(rows)))

    def probe_history(self, first, count):
        """(points float32[count, P, 8], levels float32[count, L, 8]): the records of probes_record calls first .. first + count - 1,
        while the ring holds them."""
        P, L = self.probes_count()
        n = max(int(count), 0)
        pts, lev = np.zeros((n, P, SAMPLE_WORDS), np.float32), np.zeros((n, L, PROBE_LEVEL_WORDS), np.float32)
        self._chk(self._L.sph_probes_read_history(self._h, int(first), int(count), _ptr(pts) if pts.size else None,
                                                  _ptr(lev) if lev.size else None, None))
        return pts, lev

    # --- time statistics on a lattice (sph_stats_*): per-node sums, call indices and extremes that stay on the device ---
    def stats_define(self, slot, origin, spacing, dims, types=(1,)):
        """Give statistics slot `slot` (0..3) the lattice origin + (float)i * spacing, i < dims = (nx, ny, nz), sampled over `types`
        as sample_grid samples it; its accumulators start empty, with no call made."""
        g = stats_lattice(origin, spacing, dims, types)
        self._chk(self._L.sph_stats_define(self._h, int(slot), _ptr(g)))

    def stats_release(self, slot):
        self._chk(self._L.sph_stats_define(self._h, int(slot), None))

    def stats_get(self, slot):
        """(lattice, calls): the slot's definition as a dict (origin, spacing, dims, typeMask), or None while it has none, and
        the accumulate calls it has taken."""
        g, has, calls = np.zeros(1, STATS_LATTICE_DTYPE), np.zeros(1, np.int32), np.zeros(1, np.int64)
        self._chk(self._L.sph_stats_get(self._h, int(slot), _ptr(g), _ptr(has), _ptr(calls)))
        if not has[0]:
            return None, int(calls[0])
        return {"origin": g["origin"][0].copy(), "spacing": g["spacing"][0].copy(), "dims": tuple(int(v) for v in g["dims"][0]),
                "typeMask": int(g["typeMask"][0])}, int(calls[0])

    def stats_accumulate(self, slot=-1):
        """Fold the sample record of the last completed step at every node of slot `slot` (-1: every defined slot) into its
        accumulators. Enqueued; never waits for the host. Once per step: a second call counts the step again."""
        self._chk(self._L.sph_stats_accumulate(self._h, int(slot)))

    def stats_reset(self, slot=-1):
        """Empty the numbers and the call count of slot `slot`, or of every defined slot; the definitions stay."""
        self._chk(self._L.sph_stats_reset(self._h, int(slot)))

    def _stats_window(self, slot, first, count, what):
        g, calls = self.stats_get(slot)
        if g is None:
            raise SphError("%s: slot %d is not defined" % (what, int(slot)))
        nx, ny, nz = g["dims"]
        nodes = nx * ny * nz
        whole = first is None and count is None
        first = 0 if first is None else int(first)
        count = nodes - first if count is None else int(count)
        return first, count, ((nz, ny, nx) if whole else (max(count, 0),))  # (the library judges the window)

    def stats(self, slot, first=None, count=None):
        """(float64[nz, ny, nx, 24] named by STATS_FIELDS, calls). With first / count: the nodes first .. first + count - 1 of the
        node-major order (x fastest), float64[count, 24]. Blocking."""
        first, count, shape = self._stats_window(slot, first, count, "stats")
        out, calls = np.zeros(shape + (STATS_WORDS,), np.float64), np.zeros(1, np.int64)
        self._chk(self._L.sph_stats_read(self._h, int(slot), first, count, _ptr(out) if count else None, _ptr(calls)))
        return out, int(calls[0])

    def stats_moments(self, slot, first=None, count=None):
        """(float32[nz, ny, nx, 16] named by STATS_MOMENT_FIELDS, calls), computed on the device; windows as stats(). Blocking."""
        first, count, shape = self._stats_window(slot, first, count, "stats_moments")
        out, calls = np.zeros(shape + (STATS_MOMENT_WORDS,), np.float32), np.zeros(1, np.int64)
        self._chk(self._L.sph_stats_read_moments(self._h, int(slot), first, count, _ptr(out) if count else None, _ptr(calls)))
        return out, int(calls[0])

    # --- carried particle fields (sph_field_*): a scalar of the user's own per particle, in original-id order ---
    def _field_values(self, values, what):
        a = np.ascontiguousarray(values, np.float32).reshape(-1)
        if a.size != self.N:
            raise SphError("%s: values must hold one float per particle (%d)" % (what, self.N))
        return a

    def field_create(self, slot, values=None, inflow=0.0):
        """Create carried field `slot` (0..3): float32[N] `values` in original-id order (the order of read_position_buffer;
        None = all zero). Particles added later start at `inflow`. A step never touches a field; remove_*, add_particles
        and emit_lattice carry it along (include/sphmi.h)."""
        a = None if values is None else self._field_values(values, "field_create")
        self._chk(self._L.sph_field_create(self._h, int(slot), _ptr(a), float(np.float32(inflow))))

    def field_release(self, slot):
        self._chk(self._L.sph_field_release(self._h, int(slot)))

    def field_read(self, slot):
        """float32[N]: the field of the current particle set, in original-id order."""
        out = np.empty(max(self.N, 1), np.float32)
        self._chk(self._L.sph_field_read(self._h, int(slot), _ptr(out)))
        return out[:self.N]

    def field_write(self, slot, values):
        self._chk(self._L.sph_field_write(self._h, int(slot), _ptr(self._field_values(values, "field_write"))))

    def field_set_region(self, slot, value, region=None, types=(1,)):
        """Set the field to `value` on the particles remove_region(region, types) would remove, by their current position.
        Returns their number."""
        rg = _region(region, "field_set_region")
        painted = np.zeros(1, np.int64)
        self._chk(self._L.sph_field_set_region(self._h, int(slot), _ptr(rg), type_mask(types), float(np.float32(value)), _ptr(painted)))
        return int(painted[0])

    def field_set_selection(self, slot, value):
        """Set the field to `value` on the particles of the last select() (refused once the solver has stepped since).
        Returns their number."""
        painted = np.zeros(1, np.int64)
        self._chk(self._L.sph_field_set_selection(self._h, int(slot), float(np.float32(value)), _ptr(painted)))
        return int(painted[0])

    def field_diffuse(self, slot, coefficient, substeps=1, types=(1,)):
        """`substeps` Jacobi substeps of c_i += a_i * sum_j ((c_j - c_i) * (hs - r_ij)) / rho_j over the neighbour rows of the
        last completed step, among the particles of `types` (K7's viscous sum with the scalar in place of a velocity
        component; `coefficient` = diffusivity * time in the units of cfg.viscosity). Returns the stability number sigma =
        max_i a_i * sum_j (hs - r_ij) / rho_j: for sigma <= 1 the field keeps its bounds. substeps=0 only measures it."""
        sigma = np.zeros(1, np.float32)
        self._chk(self._L.sph_field_diffuse(self._h, int(slot), float(np.float32(coefficient)), int(substeps), type_mask(types), _ptr(sigma)))
        return float(sigma[0])

    def field_diagnostics(self, slot, regions=None, types=(1,)):
        """Reductions of the field over the particles diagnostics() selects for each region: float64[R, 8] records named by
        frames.FIELD_DIAG_FIELDS (count, sum, sum of squares, min, max, particles with a non-zero value), added in the fixed
        tree of diagnostics(). frames.field_summary turns a record into mean and variance."""
        rg = _regions(regions, "field_diagnostics")
        out = np.zeros((max(rg.shape[0], 1), FIELD_DIAG_WORDS), np.float64)
        self._chk(self._L.sph_field_diagnostics(self._h, int(slot), _ptr(rg), rg.shape[0], type_mask(types), _ptr(out)))
        return out

    # --- integral curves (sph_trace_streamlines / sph_tracers_*): streamlines of the frozen field, tracers carried with a run ---
    def _trace_params(self, what, step, mode, integrator, max_steps, min_speed, dt):
        """The sph_trace_params of a call: `step` as it is, or dt seconds as dt / simulationScale (mode "time" only)."""
        mode = _field_index(mode, TRACE_MODES, what)
        if dt is not None:
            if step is not None or mode != TRACE_TIME:
                raise SphError("%s: dt replaces step, in mode \"time\"" % what)
            step = np.float32(dt) / np.float32(self.cfg.simulationScale)
        if step is None:
            raise SphError("%s: step or dt must be given" % what)
        return SphTraceParams(float(np.float32(step)), float(np.float32(min_speed)), int(max_steps), mode,
                              _field_index(integrator, TRACE_INTEGRATORS, what))

    def streamlines(self, seeds, types=(1,), step=None, mode="arc", integrator="midpoint", max_steps=256, min_speed=0.0, region=None,
                    dt=None):
        """Streamlines of the velocity field sample_points interpolates over the particles of `types`, frozen at the last completed
        step, one from each of `seeds` ([Q, 3] or [Q, 4]), traced on the device in one call (include/sphmi.h): mode "arc"
        advances by chords of length `step` (scene units), "time" by step * velocity (or give dt in seconds); a negative step goes
        upstream. Returns (vertices float32[Q, max_steps + 1, 4]: x, y, z and the speed there, +0 behind a curve's end;
        lengths int32[Q]; status int32[Q], the TRACE_* code each curve stopped with)."""
        p4 = _points4(seeds, "streamlines")
        prm = self._trace_params("streamlines", step, mode, integrator, max_steps, min_speed, dt)
        rg = _region(region, "streamlines")
        Q, M = p4.shape[0], max(int(max_steps), 0)
        verts = np.empty((Q, M + 1, 4), np.float32)
        lengths = np.empty(Q, np.int32)
        status = np.empty(Q, np.int32)
        self._chk(self._L.sph_trace_streamlines(self._h, _ptr(p4), Q, type_mask(types), C.byref(prm), _ptr(rg), _ptr(verts),
                                                _ptr(lengths), _ptr(status)))
        return verts, lengths, status

    def tracers_set(self, points):
        """Replace the solver's tracers by `points` ([Q, 3] or [Q, 4]; none releases them): points on the device that
        tracers_advect moves and that steps and edits leave alone."""
        p4 = _points4(points, "tracers_set") if points is not None and np.size(points) else np.zeros((0, 4), np.float32)
        self._chk(self._L.sph_tracers_set(self._h, _ptr(p4) if p4.size else None, p4.shape[0]))
        self._tracers = p4.shape[0]

    def tracers_advect(self, types=(1,), step=None, mode="time", integrator="midpoint", min_speed=0.0, region=None, dt=None):
        """One step of the streamline rule for every tracer that is still moving, through the field of the last completed step
        (dt: seconds, e.g. cfg.timeStep after every step()). Returns (still moving, stopped)."""
        prm = self._trace_params("tracers_advect", step, mode, integrator, 0, min_speed, dt)
        rg = _region(region, "tracers_advect")
        counts = np.zeros(2, np.int64)
        self._chk(self._L.sph_tracers_advect(self._h, type_mask(types), C.byref(prm), _ptr(rg), _ptr(counts)))
        return int(counts[0]), int(counts[1])

    def tracers(self):
        """(positions float32[Q, 4]: x, y, z and the speed at the tracer's last sample; status int32[Q], TRACE_MOVING or the code it
        stopped with; steps int32[Q], the advects it took part in)."""
        n = getattr(self, "_tracers", 0)  # 0 without tracers: the library reports SPH_ERR_ORDER
        pos = np.empty((n, 4), np.float32)
        status = np.empty(n, np.int32)
        steps = np.empty(n, np.int32)
        self._chk(self._L.sph_tracers_read(self._h, _ptr(pos) if n else None, _ptr(status) if n else None, _ptr(steps) if n else None))
        return pos, status, steps

    # --- extras ---
    def step(self, iterationCount=0):
        """Fused fast path == the stage sequence of simulationStep()."""
        return self._chk(self._L.sph_step(self._h, iterationCount))

    def synchronize(self):
        return self._chk(self._L.sph_synchronize(self._h))

    def buffer(self, name):
        need = C.c_size_t()
        self._chk(self._L.sph_read_buffer(self._h, name.encode(), None, 0, C.byref(need)))
        out = np.empty(need.value // np.dtype(_BUF_DTYPE[name]).itemsize, _BUF_DTYPE[name])
        self._chk(self._L.sph_read_buffer(self._h, name.encode(), _ptr(out), need.value, None))
        return out

    def neighbor_rows(self, first, count):
        """Neighbour ids and scaled distances of the sorted particles [first, first + count): two (count, 32) arrays."""
        ids = np.empty((count, 32), np.int32)
        dist = np.empty((count, 32), np.float32)
        self._chk(self._L.sph_read_neighbor_rows(self._h, first, count, _ptr(ids), _ptr(dist)))
        return ids, dist

    # --- slab decomposition (include/sphmi.h, "Spatial decomposition") ---
    def slab_init(self, slab, global_ids):
        g = np.ascontiguousarray(global_ids, np.uint32)
        return self._chk(self._L.sph_slab_init(self._h, C.byref(slab), _ptr(g)))

    def slab_pack(self, msg_down_ptr, msg_up_ptr, cap_records):
        counts = (C.c_int32 * 3)()
        self._chk(self._L.sph_slab_pack(self._h, msg_down_ptr, msg_up_ptr, cap_records, counts))
        return counts[0], counts[1], counts[2]

    def slab_pack_framed(self, frame_down_ptr, frame_up_ptr, cap_records):
        counts = (C.c_int32 * 3)()
        self._chk(self._L.sph_slab_pack_framed(self._h, frame_down_ptr, frame_up_ptr, cap_records, counts))
        return counts[0], counts[1], counts[2]

    def slab_step_begin(self, iterationCount, frame_down_ptr, frame_up_ptr, cap_records):
        self._chk(self._L.sph_slab_step_begin(self._h, iterationCount, frame_down_ptr, frame_up_ptr, cap_records))

    def slab_step_messages(self):
        counts = (C.c_int32 * 2)()
        self._chk(self._L.sph_slab_step_messages(self._h, counts))
        return counts[0], counts[1]

    def slab_rebuild(self, recv_down_ptr, n_down, recv_up_ptr, n_up):
        self._chk(self._L.sph_slab_rebuild(self._h, recv_down_ptr, n_down, recv_up_ptr, n_up))
        self.N = self._L.sph_particle_count(self._h)
        return self.N

    def slab_rebuild_framed(self, frame_down_ptr, cap_down_records, frame_up_ptr, cap_up_records):
        """Asynchronous rebuild from complete received frames; the new count arrives with slab_rebuild_finish()."""
        self._chk(self._L.sph_slab_rebuild_framed(self._h, frame_down_ptr, cap_down_records, frame_up_ptr, cap_up_records))

    def slab_rebuild_finish(self):
        """(kept, records from below, records from above, nothing_merged) of the last slab_rebuild_framed; blocks."""
        c = (C.c_int32 * 4)()
        self._chk(self._L.sph_slab_rebuild_finish(self._h, c))
        if not c[3]:
            self.N = self._L.sph_particle_count(self._h)
        return c[0], c[1], c[2], bool(c[3])

    def slab_liquid_signature(self):
        b = C.c_uint32()
        self._chk(self._L.sph_slab_liquid_signature(self._h, C.byref(b)))
        return b.value

    def slab_set_record_format(self, words, type_bits=0):
        return self._chk(self._L.sph_slab_set_record_format(self._h, words, type_bits))

    def stream_wait_event(self, hip_event_handle):
        return self._chk(self._L.sph_stream_wait_event(self._h, C.c_void_p(hip_event_handle)))

    def slab_read(self):
        n = self._L.sph_particle_count(self._h)
        pos, vel = np.empty((n, 4), np.float32), np.empty((n, 4), np.float32)
        gid, owned = np.empty(n, np.uint32), np.empty(n, np.uint32)
        self._chk(self._L.sph_slab_read(self._h, _ptr(pos), _ptr(vel), _ptr(gid), _ptr(owned)))
        return pos, vel, gid, owned

    def set_stage_timing(self, enable=True):
        return self._chk(self._L.sph_set_stage_timing(self._h, int(enable)))

    def set_step_chunks(self, chunks=0):
        """How many ranges of sorted particles step() overlaps density and the record pack with findNeighbors by: 0 automatic
        (by particle count), 1 never, 2..16 forced (tests use it on small scenes). Results do not depend on the chunk count."""
        return self._chk(self._L.sph_set_step_chunks(self._h, int(chunks)))

    def set_step_pipeline(self, depth=-1):
        """How many of the kernels behind the search the chunked step() runs chunk by chunk under it (forces, then predicted
        density and pressure force per iteration): -1 the built-in depth, 0 none, 1..6 forced (clamped to the stages the step
        has, and to 1 with elastic matter). Results do not depend on it."""
        if not hasattr(self._L, "sph_set_step_pipeline"):
            raise SphError("this libsphmi has no sph_set_step_pipeline")
        return self._chk(self._L.sph_set_step_pipeline(self._h, int(depth)))

    def set_wave_skip(self, mode=0):
        """The per-wave skipping of the predict-correct loop: 0 the built-in policy, 1 the writers always mark and the consumers
        always consult, 2 off. Results do not depend on it."""
        if not hasattr(self._L, "sph_set_wave_skip"):
            raise SphError("this libsphmi has no sph_set_wave_skip")
        return self._chk(self._L.sph_set_wave_skip(self._h, int(mode)))

    def set_search_bands(self, mode=0):
        """The search bands of step(): 0 automatic (used wherever they are provably a superset of the neighbours), 1 off.
        Results do not depend on it."""
        if not hasattr(self._L, "sph_set_search_bands"):
            raise SphError("this libsphmi has no sph_set_search_bands")
        return self._chk(self._L.sph_set_search_bands(self._h, int(mode)))

    def reset_stage_times(self):
        return self._chk(self._L.sph_reset_stage_times(self._h))

    def step_sort_passes(self):
        """Radix passes the sort of the fused step takes for this solver (24 algorithmic bytes per particle each)."""
        n = self._L.sph_step_sort_passes(self._h)
        if n < 0:
            self._chk(n)
        return n

    def stage_times(self):
        n = len(STAGE_NAMES)
        if not hasattr(self._L, "sph_set_search_bands"):  # (an A/B library built from an older csrc/: no band stage)
            n -= 1
        ms = (C.c_double * n)()
        cnt = (C.c_int64 * n)()
        self._chk(self._L.sph_get_stage_times(self._h, ms, cnt, n))
        return {STAGE_NAMES[i]: (ms[i], cnt[i]) for i in range(n)}


class owPhysicsFluidSimulator:
    """Stage order of owPhysicsFluidSimulator::simulationStep() (owPhysicsFluidSimulator.cpp:79-149)."""

    def __init__(self, cfg, position_cpp, velocity_cpp, elasticConnectionsData_cpp=None, membraneData_cpp=None,
                 particleMembranesList_cpp=None, fused=True, muscles=False):
        self.ocl_solver = owHIPSolver(cfg, position_cpp, velocity_cpp, elasticConnectionsData_cpp, membraneData_cpp,
                                      particleMembranesList_cpp)
        self.cfg = cfg
        self.iterationCount = 0
        self.fused = fused
        self.muscles = muscles
        self.position_cpp = np.array(position_cpp, np.float32).reshape(-1, 4)

    def simulationStep(self, read_back=True, async_read_back=False):
        s = self.ocl_solver
        if self.fused:
            s.step(self.iterationCount)
        else:
            s._runClearBuffers(); s._runHashParticles(); s._runSort(); s._runSortPostPass(); s._runIndexx()
            s._runIndexPostPass(); s._runFindNeighbors()
            s._run_pcisph_computeDensity(); s._run_pcisph_computeForcesAndInitPressure()
            s._run_pcisph_computeElasticForces()
            it = 0
            while True:
                s._run_pcisph_predictPositions(); s._run_pcisph_predictDensity(); s._run_pcisph_correctPressure()
                s._run_pcisph_computePressureForceAcceleration()
                it += 1
                if it >= self.cfg.maxIteration:
                    break
            s._run_pcisph_integrate(self.iterationCount)
            s._run_clearMembraneBuffers(); s._run_computeInteractionWithMembranes()
            s._run_computeInteractionWithMembranes_finalize()
        if read_back and self.position_cpp.shape[0] != s.N:  # an edit changed the particle count
            # (waits for a copy in flight, then releases the page lock read_position_buffer_async put on the old array)
            s._chk(s._L.sph_host_unregister(s._h, _ptr(self.position_cpp)))
            self.position_cpp = np.empty((s.N, 4), np.float32)
        if read_back and async_read_back:  # the copy overlaps the next step; getPosition_cpp() waits for it
            s.read_position_buffer_async(self.position_cpp)
        elif read_back:
            s.read_position_buffer(self.position_cpp)
        if self.muscles:  # signals computed after step t drive step t+1 (owPhysicsFluidSimulator.cpp:134-141)
            s.updateMuscleActivityData(muscle_signal(self.iterationCount, self.cfg.muscleCount))
        self.iterationCount += 1

    def getPosition_cpp(self):
        self.ocl_solver.wait_position_buffer()  # (no-op unless simulationStep(async_read_back=True) left a copy in flight)
        return self.position_cpp

    def getDensity_cpp(self): return self.ocl_solver.read_density_buffer()
    def getParticleIndex_cpp(self): return self.ocl_solver.read_particleIndex_buffer()

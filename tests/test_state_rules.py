"""The two rules of the solver's host side through the Python wrapper: every call that rewrites the state says
so in one place, and every result derived from the state (mesh, labelling, selection, id map, image) is dropped, stamped and
checked in one way. The golden scenes `tiny` and `tiny_elastic` with room for 64 more particles; the status codes are the
numeric ones, as in test_edit.py."""
import numpy as np
import pytest

import edit_ref as er
import scenes
import sphmi
from sphmi import frames
from scenes import error_status as _status

pytestmark = pytest.mark.gpu

ERR_INVALID, ERR_ORDER = -1, -3
f32 = np.float32
NOWHERE = (0, 0, 0, 0, 0, 0)  # a half-open box that holds no point

# the texts of csrc/sph_api_analysis.hip and sph_api_edit.hip before the derived results had one rule, literally
STALE = {
    "surface_normals": "sph_surface_normals: the solver's state has changed since the surface was extracted",
    "component_diagnostics": "sph_component_diagnostics: the solver's state has changed since the labelling",
    "selection": "sph_read_selection: the solver's state has changed since the selection",
    "remove_selection": "sph_remove_selection: the solver's state has changed since the selection",
    "edit_map": "sph_read_edit_map: a stage, step or edit has run since the removal",
}
# Entry points that the stage sequence calls on a scene without reaching their launcher: without membrane lists
# sph_run_compute_interaction_with_membranes returns before anything runs, and says nothing has changed.
NOT_REACHED = {"tiny": {"computeInteractionWithMembranes"}, "tiny_elastic": set()}


def _solver(name, steps=2):
    sc = scenes.SCENES[name]()
    n = sc["cfg"].particleCount
    hip = sphmi.owHIPSolver(er.with_count(sc["cfg"], n, n + 64), sc["position"], sc["velocity"], sc["elastic"], sc["membranes"],
                            sc["particle_membranes"])
    for it in range(steps):
        hip.step(it)
    return sc, hip


def _refused(call, status, text=None):
    with pytest.raises(sphmi.SphError) as ei:
        call()
    assert _status(ei) == status, str(ei.value)
    if text is not None:
        assert text in str(ei.value)


def _liquid_box(hip):
    pos = hip.read_position_buffer()
    liq = pos[pos[:, 3].astype(np.int32) == 1, :3]
    return liq.min(0), liq.max(0)


def _extract(hip, dims=(8, 8, 8)):
    """The liquid's surface on a lattice over its bounding box, one h of margin around it so that the outermost points lie
    outside the liquid (on the bounding box itself every point is inside, and the mesh is empty)."""
    lo, hi = _liquid_box(hip)
    lo, hi = lo - f32(hip.cfg.h), hi + f32(hip.cfg.h)
    return hip.extract_surface(lo, (hi - lo) / f32(7), dims, iso=0.5, types=(1,))


def _read_surface(hip, vertices):
    """sph_read_surface alone (the wrapper only calls it from extract_surface)."""
    out = np.empty((vertices, 3), f32)
    hip._chk(hip._L.sph_read_surface(hip._h, sphmi._ptr(out), None))
    return out


def _make_results(hip):
    """A mesh, a labelling, an (empty) selection and an (identity) id map, all current; returns the mesh's vertices."""
    n = hip.N
    verts, _ = _extract(hip)
    assert verts.shape[0] > 0
    assert hip.label_components()[1] > 0
    assert hip.select() > 0
    assert hip.selection()[0].size == hip._selected
    assert hip.select(region=NOWHERE) == 0
    assert hip.remove_region(NOWHERE, (1,)) == 0 and hip.N == n
    return verts


def _readers(hip):
    return {"surface_normals": hip.surface_normals, "component_diagnostics": lambda: hip.component_diagnostics([0]),
            "selection": hip.selection, "remove_selection": hip.remove_selection, "edit_map": hip.edit_map}


@pytest.mark.parametrize("name", ["tiny", "tiny_elastic"])
def test_every_stage_entry_point_marks_the_state_changed(name):
    sc, hip = _solver(name)
    n = hip.N
    reached = set()
    for st in scenes.STAGE_SEQUENCE:
        assert hip.remove_region(NOWHERE, (1,)) == 0 and hip.N == n  # leaves the state and its epoch alone
        assert np.array_equal(hip.edit_map(), np.arange(n))
        m = getattr(hip, scenes.HIP_STAGE_METHOD[st])
        m(0) if st == "integrate" else m()
        if st in NOT_REACHED[name]:
            assert np.array_equal(hip.edit_map(), np.arange(n)), st
            continue
        _refused(hip.edit_map, ERR_ORDER, STALE["edit_map"])
        reached.add(st)
    assert reached == set(scenes.HIP_STAGE_METHOD) - NOT_REACHED[name] and len(scenes.HIP_STAGE_METHOD) == 18
    hip.close()


def test_every_derived_result_follows_one_rule():
    sc, hip = _solver("tiny")
    n = hip.N
    verts = _make_results(hip)
    lo, hi = _liquid_box(hip)
    assert hip.render(frames.render_view(lo, hi, 32, 24))[0] > 0
    image = hip.rendered()
    assert hip.surface_normals().shape == verts.shape
    assert hip.component_diagnostics([0])[0, 0] > 0
    assert hip.selection()[0].size == 0
    assert hip.remove_selection() == 0 and hip.N == n  # (the empty selection: nothing is removed, nothing changes)
    assert np.array_equal(hip.edit_map(), np.arange(n))
    hip.step(2)
    for what, call in _readers(hip).items():
        _refused(call, ERR_ORDER, STALE[what])
    # self-contained by contract: the mesh and the images outlive the state they were made from
    assert scenes.bits_equal(_read_surface(hip, verts.shape[0]), verts)
    again = hip.rendered()
    assert all(scenes.bits_equal(again[k], image[k]) for k in image)
    hip.close()


def test_a_failed_producer_leaves_nothing_behind():
    sc, hip = _solver("tiny")
    assert hip.label_components()[1] > 0 and hip.select() > 0
    hip.components()
    hip.selection()
    _refused(lambda: hip.label_components(types=()), ERR_INVALID)
    _refused(lambda: hip.select(types=()), ERR_INVALID)
    _refused(hip.components, ERR_ORDER, "sph_read_components: no labelling has been made")
    _refused(hip.selection, ERR_ORDER, "sph_read_selection: no selection has been made")
    assert _extract(hip)[0].shape[0] > 0
    hip.surface_normals()
    _refused(lambda: _extract(hip, dims=(1, 1, 1)), ERR_INVALID)
    _refused(hip.surface_normals, ERR_ORDER, "sph_surface_normals: no surface has been extracted")
    hip.close()


def _add_one(hip, sc):
    r0 = f32(sc["cfg"].r0)
    lo, hi = _liquid_box(hip)
    above = np.array([[(lo[0] + hi[0]) / 2, hi[1] + 2 * r0, (lo[2] + hi[2]) / 2, 1.0]], f32)
    assert hip.add_particles(above, np.zeros((1, 4), f32)) == sc["cfg"].particleCount + 1


def _emit_block(hip, sc):
    r0 = f32(sc["cfg"].r0)
    lo, hi = _liquid_box(hip)
    assert hip.emit_lattice((lo[0], hi[1] + 2 * r0, lo[2]), (r0,) * 3, (2, 2, 2)) == 8


@pytest.mark.parametrize("edit", ["add_particles", "emit_lattice", "remove_ids", "count_only"])
def test_edits_mark_the_state_changed(edit):
    sc, hip = _solver("tiny")
    n = hip.N
    _make_results(hip)
    readers = _readers(hip)
    if edit == "count_only":
        assert hip.remove_region(None, (1,), count_only=True) > 0 and hip.N == n
        hip.surface_normals()
        hip.component_diagnostics([0])
        assert hip.selection()[0].size == 0 and hip.remove_selection() == 0
        assert np.array_equal(hip.edit_map(), np.arange(n))
    else:
        gone = [n - 1, n - 3]
        {"add_particles": lambda: _add_one(hip, sc), "emit_lattice": lambda: _emit_block(hip, sc),
         "remove_ids": lambda: hip.remove_ids(gone)}[edit]()
        for what in ("surface_normals", "component_diagnostics", "selection", "remove_selection"):
            _refused(readers[what], ERR_ORDER)
        if edit == "remove_ids":
            # the removal made a map of its own, which is the current one: the identity map of before is gone with the rest
            m = hip.edit_map()
            assert m.size == n and (m[gone] == -1).all() and np.array_equal(np.delete(m, gone), np.arange(n - 2))
        else:
            _refused(readers["edit_map"], ERR_ORDER, STALE["edit_map"])
    hip.close()

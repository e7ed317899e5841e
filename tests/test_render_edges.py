"""GPU tests that pin the two renderers (sph_render_particles in csrc/sph_render.hip, sph_render_mesh in csrc/sph_render_mesh.hip)
to their edge states: the hand-made scenes and views of tests/render_edge_cases.py, every word of every image and every count
equal to the restatements through test_render.check_render / test_render_mesh.check_mesh (depths as bit patterns, no tolerance
anywhere), and the condition each case exists for asserted again on the device's own output. tests/test_render_edges_host.py
proves on the CPU that the cases meet those conditions, so that the comparison here is not trivially true.

What the cases reach: the second trip of both drain loops (more queued items than the 4096 waves of the fixed grid, drawn twice
to show that the order of arrival does not matter); label -1 and labels past the palette; the lane / queue switch at box sides
of exactly 8 and 9 pixels, by size and by clipping, in x and y separately; the strict and non-strict comparisons at equality
(cz and depth against nearPlane, R against maxRadiusPx, |u| against 2^20, d2 == R2, a depth tie in compose); pixel centres on
owning and non-owning edges and on shared vertices for both windings; negative snapped corners; corners just below 2^20
pixels; ramp end points and knots; images of 1 x 1, 1 x H and W x 1 and counts that are no multiple of 64.

Known uncovered states: smooth shading (it needs an extraction, whose vertices cannot be placed by hand); the density colour
thresholds (rho cannot be placed exactly); thickness saturation past 2^32 (about 16.7 M fragments on one pixel); and of the
surface source's vertex kernel whatever the natural scenes of tests/test_render_mesh.py do not reach."""
import numpy as np
import pytest

import render_edge_cases as ec
import scenes
from scenes import staged_step
from test_render import Snapshot, check_render
from render_edge_checks import expected_labels, splat_image_conditions, triangle_image_conditions
from test_render_mesh import Snapshot as MeshSnapshot
from test_render_mesh import COLOUR, check_mesh, membrane_mesh

pytestmark = pytest.mark.gpu


def stepped(sc, snapshot, staged=False):
    """(solver, snapshot) after one step; the sorted state of that step is the input, bit for bit."""
    hip = scenes.hip_for(sc)
    staged_step(hip, 0) if staged else hip.step(0)
    snap = snapshot(hip)
    ids = snap.state["ids"]
    assert np.array_equal(snap.state["pos"].view(np.uint32), sc["position"][ids, :3].view(np.uint32))
    return hip, snap


def same_bytes(a, b, what):
    assert a.keys() == b.keys()
    for k in a:
        assert np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), (what, k)


def draw_splats(hip, snap, case, who=None):
    """One case against the restatement, then its condition on the device's images; returns them."""
    labels = None
    if case.label is not None:
        link, types = case.label
        hip.label_components(link, types)
        labels = hip.components()[0]
        assert np.array_equal(labels, expected_labels(snap.state, types, hip.N))
    want = check_render(hip, snap, case.view, case.name, case.region, case.types, case.thickness, labels)
    got = hip.rendered(thickness=case.thickness)
    if who is not None:
        splat_image_conditions(case, got, want["drawn"], want["covered"], snap.state, who, labels)  # (the device's counts equal want's)
    return want, got


def test_splat_edge_cases():
    sc, who = ec.splat_scene()
    hip, snap = stepped(sc, Snapshot)
    fused = {}
    for case in ec.splat_cases(sc, who):
        fused[case.name] = draw_splats(hip, snap, case, who)[1]
    hip.close()
    assert len(fused) == 21
    hip, snap = stepped(sc, Snapshot, staged=True)
    case = ec.splat_cases(sc, who)[0]
    same_bytes(draw_splats(hip, snap, case, who)[1], fused[case.name], "staged " + case.name)
    hip.close()


def test_deep_splat_queue_is_drained_in_more_than_one_trip():
    sc = ec.deep_splat_scene()
    hip, snap = stepped(sc, Snapshot)
    for case in ec.deep_splat_cases():
        want, first = draw_splats(hip, snap, case)
        assert want["queued"] == want["drawn"] == hip.N > ec.DRAIN_WAVES and first["thickness"].max() == 15 * 256
        winners = np.unique(first["index"][first["index"] >= 0])
        assert winners.size == 17 * 17 and ((winners >= ec.DRAIN_WAVES).sum() >= 64) == (case.name == "deep_queue_back")
        assert hip.render(case.view, case.region, case.types, case.thickness) == (want["drawn"], want["covered"])
        same_bytes(hip.rendered(thickness=case.thickness), first, case.name + " drawn twice")
    hip.close()


def draw_triangles(hip, mesh, case, conditions=None):
    want, got = check_mesh(hip, mesh, case.view, case.name, "flat", case.field, case.compose, case.bounds)
    if conditions is not None:
        who, spheres, coverage = conditions
        triangle_image_conditions(case, got, want["counts"], mesh.snap.state, who, spheres, coverage)  # (the device's counts equal want's)
    return want, got


def test_triangle_edge_cases():
    sc, who, spheres = ec.triangle_scene()
    hip, snap = stepped(sc, MeshSnapshot)
    mesh = membrane_mesh(hip, snap, sc["membranes"])
    fused = {}
    for case in ec.triangle_cases():
        want, fused[case.name] = draw_triangles(hip, mesh, case, (who, spheres, fused.get("coverage")))
        if case.name == "coverage":
            assert (want["queued"], want["unusable"], want["degenerate"], want["partly_outside"]) == (20, 2, 2, 8)
    hip.close()
    assert len(fused) == 12
    hip, snap = stepped(sc, MeshSnapshot, staged=True)
    mesh = membrane_mesh(hip, snap, sc["membranes"])
    case = ec.triangle_cases()[0]
    same_bytes(draw_triangles(hip, mesh, case, (who, spheres, None))[1], fused[case.name], "staged " + case.name)
    hip.close()


def test_sheet_queue_is_drained_in_more_than_one_trip():
    sc = ec.sheet_scene()
    hip, snap = stepped(sc, MeshSnapshot)
    mesh = membrane_mesh(hip, snap, sc["membranes"])
    for case in ec.sheet_cases():
        want, first = draw_triangles(hip, mesh, case)
        if case.name == "deep_queue":
            assert want["queued"] == 4418 > ec.DRAIN_WAVES and want["counts"] == (4418, 0, 376 * 47, 376 * 47)
            assert np.unique(first["triangle"][first["triangle"] >= 0]).size == 4418  # every triangle of the queue holds pixels
        if case.name == "deep_131x67":
            assert want["counts"] == (4418, 0, 131 * 28, 131 * 28) and (want["queued"], want["partly_outside"]) == (870, 146)
            assert (first["triangle"][0:28] >= 0).all() and (first["triangle"][28:] == -1).all()
        if case.name == "deep_1x1":
            assert want["counts"] == (4418, 0, 1, 1)
        assert hip.render_mesh(case.view, "membranes", "flat", COLOUR) == want["counts"]
        same_bytes(hip.rendered(triangle=True), first, case.name + " drawn twice")
    hip.close()

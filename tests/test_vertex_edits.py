"""Incremental vertex updates (gi_build.cpp updateVertices, gi_refit.hip): with GI_C_SCENE_OPTION_VERTEX_UPDATES a giCSetMeshVertices on a
mesh of the built scene no longer rebuilds the scene.  The next render re-sends the mesh's vertex and shading records, makes its flattened triangles again
and refits the resident BVH on the device -- same topology, new conservative boxes.  By the traversal contract the image does not depend on the tree: colour
and AOVs must be bit-identical to a scene built from scratch from the edited description, and to the oracle's render of it.  No tolerance anywhere.

CPU: the header and the harness declare the setter, option 12, the counter and both check hooks; the API version is unchanged; the host form of the refit
(gi_refit.h, the arithmetic the kernels run) keeps a tree conservative under a smooth displacement, a random scatter, a collapse to one point, coordinates near
1e17 and no move at all.
GPU: an edit sequence on every layout (host-built, device-built, partitioned, two-level), the scene bounds, the option off, the fallbacks, the composition
with transform, visibility and material edits, the look-ahead window, two device contexts, random edit sequences against the oracle.

The scene, the comparison and the helpers are those of tests/test_visibility_edits.py: the small look-development interior (6 412 flattened triangles), 24 x 14
pixels, spp 2, 3 bounces, NEE.  After the last step of the sequence every original array is back, and on the flat layouts the digest of the resident node and
triangle bytes is the build's again: the refit and both builders run the same box arithmetic (giCDebugSceneRefitCheck holds that after every step)."""
import copy
import os
import re
import subprocess
import sys
import textwrap

import numpy as np
import pytest

from gatling_amd import capi
from gatling_amd.scene import RenderSettings
from gatling_amd.scenes import _look_at_camera

from test_hostile_inputs import sanitised
from test_visibility_edits import (A, AOVS, B, CUT, DIFFUSE_MATERIAL, H, MOVED, REASSIGNED, RS, W, _bits_equal, _check, _fresh_image, _lookdev_scene, _oracle,
                                   _partition, _translate)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
def test_header_declares_the_setter_the_option_the_counter_and_the_hooks_and_keeps_api_version_8():
    text = open(os.path.join(ROOT, "include", "gi_c.h")).read()
    assert re.search(r"int\s+giCSetMeshVertices\s*\(\s*GiCMesh\s*\*\s*\w+\s*,\s*uint32_t\s+\w+\s*,\s*const\s+GiCVertex\s*\*", text)
    assert re.search(r"#define\s+GI_C_SCENE_OPTION_VERTEX_UPDATES\s+12\b", text)
    assert re.search(r"int\s+giCDebugSceneVertexUpdateCount\s*\(\s*const\s+GiCScene\s*\*", text)
    assert re.search(r"int\s+giCDebugRefitBvh\s*\(\s*const\s+float\s*\*", text)
    assert re.search(r"int\s+giCDebugSceneRefitCheck\s*\(\s*const\s+GiCScene\s*\*", text)
    assert re.search(r"#define\s+GI_C_API_VERSION\s+8u?\b", text)
    L = capi.load_library()
    assert L.giCGetApiVersion() == 8
    for name in ("giCSetMeshVertices", "giCDebugSceneVertexUpdateCount", "giCDebugRefitBvh", "giCDebugSceneRefitCheck"):
        assert hasattr(L, name), name


def test_harness_exposes_the_option_the_setter_and_the_counter():
    assert capi.OPTION_VERTEX_UPDATES == 12
    assert callable(capi.Scene.set_mesh_vertices) and callable(capi.Scene.vertex_update_count) and callable(capi.Scene.refit_check)


def test_vertex_setter_raises_the_flags_of_a_geometry_edit():
    L = capi.load_library()
    for built in (0, 1):
        assert L.giCDebugEditDirtyFlags(16, built) == 1 | 2  # DIRTY_BVH | DIRTY_FRAMEBUFFER


def _soup(n, seed):
    """n small triangles scattered through a 10 m cube: float32 [n, 3, 3]."""
    rng = np.random.default_rng(seed)
    c = rng.uniform(-5.0, 5.0, (n, 1, 3))
    return (c + rng.uniform(-0.2, 0.2, (n, 3, 3))).astype(np.float32)


def _moved(a, case, seed):
    rng = np.random.default_rng(seed + 1)
    if case == "smooth":
        return (a + 0.15 * np.sin(1.3 * a[..., ::-1] + 0.7)).astype(np.float32)
    if case == "scatter":  # every triangle thrown to a random place: the refit's worst case
        return (a - a.mean(axis=1, keepdims=True) + rng.uniform(-50.0, 50.0, (len(a), 1, 3))).astype(np.float32)
    if case == "collapsed":  # zero extents: the -126 exponent
        return np.broadcast_to(np.float32([0.25, -1.5, 3.0]), a.shape).copy()
    if case == "far":
        return (a * np.float32(1.0e16)).astype(np.float32)  # coordinates near 1e17, inside the usable range
    assert case == "same"
    return a.copy()


@pytest.mark.parametrize("case", ["smooth", "scatter", "collapsed", "far", "same"])
@pytest.mark.parametrize("n", [1, 3, 46, 777, 20000])
def test_host_refit_keeps_the_tree_conservative(n, case):
    L = capi.load_library()
    a = _soup(n, 100 + n)
    b = _moved(a, case, n)
    assert np.isfinite(b).all() and np.abs(b).max() < 1.0e18
    fp = lambda x: np.ascontiguousarray(x, np.float32).ctypes.data_as(capi._FP)
    nodes_a, depth_a, nodes_r, depth_r = capi.C.c_uint32(0), capi.C.c_uint32(0), capi.C.c_uint32(0), capi.C.c_uint32(0)
    assert L.giCDebugValidateBvh(fp(a), n, capi.C.byref(nodes_a), capi.C.byref(depth_a)) == 0
    violations = L.giCDebugRefitBvh(fp(a), fp(b), n, capi.C.byref(nodes_r), capi.C.byref(depth_r))
    assert violations == 0, (n, case, violations)
    assert (nodes_r.value, depth_r.value) == (nodes_a.value, depth_a.value)  # the topology is the build's


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# the edits
# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
def _deformed(vertices, amplitude, seed):
    """The array with every position displaced smoothly (topology and attributes stay)."""
    rng = np.random.default_rng(seed)
    v = np.array(vertices, copy=True)
    p = v["pos"].astype(np.float64)
    k, phase = rng.uniform(2.0, 9.0, (3, 3)), rng.uniform(0.0, 6.28, 3)
    v["pos"] = (p + amplitude * np.sin(p @ k + phase)).astype(np.float32)
    return v


def _reshaded(vertices):
    """Positions stay; normals lean over and texture coordinates shift."""
    v = np.array(vertices, copy=True)
    n = v["norm"].astype(np.float64) + np.float64([0.35, -0.2, 0.1])
    v["norm"] = (n / np.maximum(np.linalg.norm(n, axis=1, keepdims=True), 1e-9)).astype(np.float32)
    v["u"] = v["u"] + np.float32(0.25); v["v"] = v["v"] * np.float32(0.5)
    return v


def _s1(sc, start):
    sc.set_mesh_vertices(A, _deformed(start.meshes[A].vertices, 0.12, 1))


def _s2(sc, start):
    sc.set_mesh_vertices(A, _deformed(sc.desc.meshes[A].vertices, 0.2, 2))


def _s3(sc, start):
    sc.set_mesh_vertices(CUT, _deformed(start.meshes[CUT].vertices, 0.15, 3))


def _s4(sc, start):
    sc.set_mesh_vertices(MOVED, _reshaded(start.meshes[MOVED].vertices))


def _s5(sc, start):
    for i in (A, CUT, MOVED):
        sc.set_mesh_vertices(i, start.meshes[i].vertices)


# (name, edit, positions moved: the render must differ from the start's)
SEQUENCE = [("vx-1-deform-A", _s1, True), ("vx-2-deform-A-again", _s2, True), ("vx-3-deform-cutout", _s3, True), ("vx-4-normals-uvs", _s4, False),
            ("start", _s5, False)]


def _make(layout, option_on=True, visibility=False, desc=None):
    sc = capi.Scene(desc if desc is not None else _lookdev_scene())
    if option_on:
        sc.set_option(capi.OPTION_VERTEX_UPDATES, 1)
    if visibility:
        sc.set_option(capi.OPTION_VISIBILITY_UPDATES, 1)
    if layout == "device":
        sc.set_option(capi.OPTION_BVH_BUILD, 1)
    if layout == "two_level":
        sc.set_option(capi.OPTION_TWO_LEVEL, 1)
    return sc


def _tree_checks(sc, key):
    v = sc.validate_bvh()
    assert v["violations"] == 0, (key, v)
    r = sc.refit_check()
    assert r["differing"] == 0 and r["nodes"] > 0, (key, r)
    return v


def _run_sequence(orc, layout, option_on=True):
    sc = _make(layout, option_on)
    start = copy.deepcopy(sc.desc)
    try:
        first = sc.render_aovs(RS, W, H, AOVS)
        assert sc.stats()["bvhBuildMs"] > 0.0 and sc.vertex_update_count() == 0
        _check(orc, sc, "start", first)
        if layout == "partitioned":
            _partition(sc)
        built = _tree_checks(sc, "built") if layout != "two_level" else None
        for step, edit, moved in SEQUENCE:
            before, vx_before = sc.update_counts(), sc.vertex_update_count()
            edit(sc, start)
            got = sc.render_aovs(RS, W, H, AOVS)
            st, after, vx_after = sc.stats(), sc.update_counts(), sc.vertex_update_count()
            print(f"{layout} option {int(option_on)} {step}: bvhBuildMs {st['bvhBuildMs']:.3f} uploadMs {st['uploadMs']:.3f} counts {after} vertex {vx_after}")
            if not option_on:  # a vertex edit rebuilds
                assert st["bvhBuildMs"] > 0.0 and after["full"] == before["full"] + 1 and vx_after == 0, (layout, step, st, after, vx_after)
            elif layout != "two_level":  # (two-level: only the images are held)
                assert after == before and vx_after == vx_before + 1, (layout, step, before, after, vx_after)
                assert st["bvhBuildMs"] == 0.0 and st["triangleCount"] == 6412, (layout, step, st)
                _tree_checks(sc, step)
            _check(orc, sc, step, got)
            if moved:
                assert not _bits_equal(got["color"], first["color"]) and not _bits_equal(got["depth"], first["depth"]), f"{layout} {step}: nothing moved"
        for k in ["color"] + AOVS:
            assert _bits_equal(got[k], first[k]), f"{layout}: {k} after the restore differs from the first render"
        if option_on and built is not None:  # the refit and the builders run the same box arithmetic: the resident bytes are the build's again
            after = sc.validate_bvh()
            assert after["digest"] == built["digest"] and after["nodes"] == built["nodes"], (layout, built, after)
    finally:
        sc.close()


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["host", "device", "partitioned", "two_level"])
def test_vertex_edits_refit_the_resident_tree_bit_exactly(gi, orc, layout):
    _run_sequence(orc, layout)


@pytest.mark.gpu
def test_with_the_option_off_the_same_edits_rebuild_and_give_the_same_bits(gi, orc):
    _run_sequence(orc, "host", option_on=False)


def _stretched_beyond_the_room(desc):
    """Mesh A with the corners of its first face moved (instance 0) to a 3 m triangle outside the room, beside and above it."""
    m = desc.meshes[A]
    world = np.asarray(m.transform, np.float64).reshape(4, 4) @ np.asarray(m.instance_transforms, np.float64).reshape(-1, 4, 4)[0]  # USD row vectors
    inv = np.linalg.inv(world)
    v = np.array(m.vertices, copy=True)
    for vi, target in zip(np.asarray(m.faces)[0], [(6.5, 0.0, 2.0), (9.5, 0.0, 2.0), (8.0, 0.0, 5.5)]):
        v["pos"][vi] = (np.float64(list(target) + [1.0]) @ inv)[:3].astype(np.float32)
    return v


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["host", "device", "partitioned"])
def test_a_mesh_stretched_beyond_the_old_bounds_is_seen_by_a_camera_that_looks_past_the_scene(gi, orc, layout):
    """Bounds retire drops camera rays that miss the scene bounds: bounds forgotten by the update would cut the stretched triangle out of the image."""
    d = _lookdev_scene()
    d.camera = _look_at_camera((0.0, -30.0, 1.5), (0.0, 0.0, 1.5), (0, 0, 1), 40.0)
    sc = _make(layout, desc=d)
    try:
        first = sc.render_aovs(RS, W, H, AOVS)
        if layout == "partitioned":
            _partition(sc)
        full = sc.update_counts()["full"]
        sc.set_mesh_vertices(A, _stretched_beyond_the_room(sc.desc))
        got = sc.render_aovs(RS, W, H, AOVS)
        assert sc.update_counts()["full"] == full and sc.vertex_update_count() == 1 and sc.stats()["bvhBuildMs"] == 0.0
        _check(orc, sc, "vx-stretched", got)
        # the triangle is seen where the first render saw past the scene (depth AOV: the clear value there)
        changed = got["depth"].view(np.uint32) != first["depth"].view(np.uint32)
        beside = changed.reshape(H, W, -1).any(axis=2)[:, 16:]  # (the room's wall at x = 5 projects to column 15)
        assert beside.any(), "the stretched triangle is not in the frame: the case does not test the bounds"
        _tree_checks(sc, "vx-stretched")
    finally:
        sc.close()


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# fallbacks
# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
def _expect_rebuild(orc, sc, key, full, oracle_desc=None):
    """`oracle_desc`: the description the oracle renders where the scene's own holds hostile values (tests/test_hostile_inputs.py sanitised)."""
    img = sc.render(RS, W, H)
    assert sc.stats()["bvhBuildMs"] > 0.0 and sc.update_counts()["full"] == full and sc.vertex_update_count() == 0, (key, sc.update_counts(), sc.vertex_update_count())
    assert _bits_equal(img, _fresh_image(sc.desc)), f"{key}: differs from a scene built from scratch"
    assert _bits_equal(img, _oracle(orc, key, oracle_desc if oracle_desc is not None else sc.desc)[0]), f"{key}: differs from the oracle"


@pytest.mark.gpu
def test_wrong_vertex_count_is_an_error_and_changes_nothing(gi, orc):
    sc = _make("host")
    try:
        first = sc.render(RS, W, H)
        v = sc.desc.meshes[A].vertices
        for wrong in (v[:-1], np.concatenate([v, v[:1]])):
            with pytest.raises(capi.GiError, match="vertices"):
                sc.set_mesh_vertices(A, wrong)
        assert len(sc.desc.meshes[A].vertices) == len(v)
        img = sc.render(RS, W, H)
        assert _bits_equal(img, first) and sc.update_counts() == {"full": 1, "transform": 0, "material": 0} and sc.vertex_update_count() == 0
    finally:
        sc.close()


@pytest.mark.gpu
@pytest.mark.parametrize("bad", [float("nan"), 1.0e19])
def test_unusable_position_rebuilds_and_matches_the_oracle(gi, orc, bad):
    sc = _make("host")
    try:
        sc.render(RS, W, H)
        v = _deformed(sc.desc.meshes[A].vertices, 0.1, 7)
        v["pos"][5, 1] = bad
        sc.set_mesh_vertices(A, v)
        _expect_rebuild(orc, sc, f"vx-unusable-{bad}", 2, sanitised(sc.desc))  # the oracle is fed ordinary geometry in place of the inactive faces
        assert sc.stats()["inactiveTriangleCount"] > 0
        sc.set_mesh_vertices(A, _deformed(sc.desc.meshes[A].vertices, 0.05, 8))  # still unusable, and the scene now holds inactive triangles
        _expect_rebuild(orc, sc, f"vx-unusable-{bad}-2", 3, sanitised(sc.desc))
    finally:
        sc.close()


@pytest.mark.gpu
def test_mesh_invisible_at_the_build_rebuilds(gi, orc):
    d = _lookdev_scene()
    d.meshes[B].visible = False
    sc = _make("host", desc=d)
    try:
        sc.render(RS, W, H)
        sc.set_mesh_vertices(B, _deformed(sc.desc.meshes[B].vertices, 0.1, 9))  # no records on the device
        _expect_rebuild(orc, sc, "vx-invisible-deformed", 2)
        sc.set_mesh_vertices(A, _deformed(sc.desc.meshes[A].vertices, 0.1, 10))  # a mesh of the scene: refitted
        img = sc.render(RS, W, H)
        assert sc.update_counts()["full"] == 2 and sc.vertex_update_count() == 1 and _bits_equal(img, _fresh_image(sc.desc))
    finally:
        sc.close()


@pytest.mark.gpu
def test_mesh_hidden_by_the_visibility_path_rebuilds(gi, orc):
    sc = _make("host", visibility=True)
    try:
        sc.render(RS, W, H)
        sc.set_mesh_visibility(A, False)
        sc.render(RS, W, H)
        assert sc.visibility_update_count() == 1 and sc.update_counts()["full"] == 1
        sc.set_mesh_vertices(A, _deformed(sc.desc.meshes[A].vertices, 0.1, 11))
        _expect_rebuild(orc, sc, "vx-hidden-deformed", 2)
        sc.set_mesh_visibility(A, True)  # invisible at that build: the show rebuilds, with the deformed points
        _expect_rebuild(orc, sc, "vx-hidden-deformed-shown", 3)
    finally:
        sc.close()


@pytest.mark.gpu
def test_refit_of_a_flat_tree_that_holds_a_hidden_mesh_keeps_its_boxes(gi, orc):
    """B is hidden in a flat tree (zero edges in its records), another mesh is deformed, then B is shown: the refit must have kept B's boxes."""
    sc = _make("host", visibility=True)
    try:
        sc.render(RS, W, H)
        sc.set_mesh_visibility(B, False)
        sc.render(RS, W, H)
        sc.set_mesh_vertices(A, _deformed(sc.desc.meshes[A].vertices, 0.1, 12))
        got = sc.render_aovs(RS, W, H, AOVS)
        assert sc.update_counts()["full"] == 1 and sc.vertex_update_count() == 1 and sc.visibility_update_count() == 1
        _check(orc, sc, "vx-deformed-beside-hidden", got)
        sc.set_mesh_visibility(B, True)
        got = sc.render_aovs(RS, W, H, AOVS)
        assert sc.update_counts()["full"] == 1 and sc.visibility_update_count() == 2
        _check(orc, sc, "vx-deformed-hidden-shown", got)
        _tree_checks(sc, "vx-deformed-hidden-shown")
    finally:
        sc.close()


@pytest.mark.gpu
def test_scene_under_the_triangle_floor_rebuilds(gi, orc):
    d = _lookdev_scene()
    for i in (A, B, MOVED, REASSIGNED):
        d.meshes[i].visible = False
    assert d.triangle_count() < 4096
    sc = _make("host", desc=d)
    try:
        sc.render(RS, W, H)
        sc.set_mesh_vertices(CUT, _deformed(sc.desc.meshes[CUT].vertices, 0.1, 13))
        _expect_rebuild(orc, sc, "vx-under-the-floor", 2)
    finally:
        sc.close()


@pytest.mark.gpu
def test_incremental_0_rebuilds(gi, orc, monkeypatch):
    sc = _make("host")
    try:
        sc.render(RS, W, H)
        monkeypatch.setenv("GATLING_OPTIONS", "incremental=0")
        sc.set_mesh_vertices(A, _deformed(sc.desc.meshes[A].vertices, 0.1, 14))
        _expect_rebuild(orc, sc, "vx-incremental-0", 2)
    finally:
        sc.close()


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# composition with the other incremental paths
# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
def _move(sc, i, x):
    sc.set_mesh_transform(i, np.asarray(sc.desc.meshes[i].transform, np.float32).reshape(4, 4) @ _translate(x, 0.05, -0.1))


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["host", "device", "partitioned"])
def test_deform_move_hide_and_assign_compose_in_one_render_and_undo_in_another_order(gi, orc, layout):
    sc = _make(layout, visibility=True)
    start = copy.deepcopy(sc.desc)
    try:
        first = sc.render_aovs(RS, W, H, AOVS)
        if layout == "partitioned":
            _partition(sc)
        before = sc.update_counts()
        sc.set_mesh_vertices(A, _deformed(start.meshes[A].vertices, 0.12, 21)); _move(sc, MOVED, 0.15)
        sc.set_mesh_visibility(B, False); sc.set_mesh_material(REASSIGNED, DIFFUSE_MATERIAL)
        got = sc.render_aovs(RS, W, H, AOVS)
        after = sc.update_counts()
        assert after == {"full": before["full"], "transform": before["transform"] + 1, "material": before["material"] + 1}, (before, after)
        assert sc.vertex_update_count() == 1 and sc.visibility_update_count() == 1
        _check(orc, sc, "vx-compose-1", got)
        sc.set_mesh_visibility(B, True); sc.set_mesh_material(REASSIGNED, start.meshes[REASSIGNED].material)  # partitioned by now: the parts of A are refitted next
        got = sc.render_aovs(RS, W, H, AOVS); _check(orc, sc, "vx-compose-2", got)
        sc.set_mesh_vertices(A, start.meshes[A].vertices); sc.set_mesh_vertices(MOVED, _deformed(start.meshes[MOVED].vertices, 0.1, 22))  # the moved mesh deforms
        got = sc.render_aovs(RS, W, H, AOVS); _check(orc, sc, "vx-compose-3", got)
        assert sc.vertex_update_count() == 2
        sc.set_mesh_transform(MOVED, np.asarray(start.meshes[MOVED].transform, np.float32).reshape(4, 4))  # a transform edit after a refit of that mesh's parts
        got = sc.render_aovs(RS, W, H, AOVS); _check(orc, sc, "vx-compose-4", got)
        sc.set_mesh_vertices(MOVED, start.meshes[MOVED].vertices)
        got = sc.render_aovs(RS, W, H, AOVS); _check(orc, sc, "start", got)
        assert sc.update_counts()["full"] == before["full"] and sc.vertex_update_count() == 3
        assert sc.validate_bvh()["violations"] == 0 and sc.refit_check()["differing"] == 0
        for k in got:
            assert _bits_equal(got[k], first[k]), k
    finally:
        sc.close()


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["host", "device"])
def test_transform_edit_after_a_flat_refit_lays_out_the_deformed_scene(gi, orc, layout):
    """The refit of a flat host-built tree drops the host copies of nodes and triangles; the re-layout of the first transform edit must make them anew from the
    deformed meshes -- no stale host copy reaches the device."""
    sc = _make(layout)
    try:
        sc.render(RS, W, H)
        sc.set_mesh_vertices(A, _deformed(sc.desc.meshes[A].vertices, 0.12, 31))
        got = sc.render_aovs(RS, W, H, AOVS); _check(orc, sc, "vx-flat-refit", got)
        _move(sc, MOVED, 0.2)
        got = sc.render_aovs(RS, W, H, AOVS); _check(orc, sc, "vx-flat-refit-moved", got)
        _move(sc, A, -0.15)  # the deformed mesh itself moves: its parts are rebuilt from the new points
        got = sc.render_aovs(RS, W, H, AOVS); _check(orc, sc, "vx-flat-refit-moved-2", got)
        sc.set_mesh_vertices(CUT, _deformed(sc.desc.meshes[CUT].vertices, 0.1, 32))  # ... and a mesh deforms where something has moved: no fallback
        got = sc.render_aovs(RS, W, H, AOVS); _check(orc, sc, "vx-flat-refit-moved-3", got)
        assert sc.update_counts() == {"full": 1, "transform": 2, "material": 0} and sc.vertex_update_count() == 2
        assert sc.stats()["bvhBuildMs"] == 0.0 and sc.validate_bvh()["violations"] == 0 and sc.refit_check()["differing"] == 0
    finally:
        sc.close()


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# look-ahead, two device contexts, random sequences
# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_vertex_edit_discards_the_look_ahead_window(gi, orc):
    rs = RenderSettings(spp=1, max_bounces=3, next_event_estimation=True)  # progressive
    sc = _make("host")
    try:
        sc.set_option(capi.OPTION_SAMPLE_LOOKAHEAD, 4)
        for _ in range(5):  # windows of 1 and 2; the fourth call traces a window of 4, the fifth is served from it
            sc.render(rs, W, H)
        la = sc.lookahead_stats()
        assert (la["windowCalls"], la["windowServed"], la["traced"]) == (4, 2, 0) and la["windowsDiscarded"] == 0, la
        sc.set_mesh_vertices(A, _deformed(sc.desc.meshes[A].vertices, 0.12, 41))  # in the middle of the window: two of its four calls were never asked for
        img = sc.render(rs, W, H)
        la2 = sc.lookahead_stats()
        assert la2["windowsDiscarded"] == 1 and la2["samplesUnused"] == 2 and la2["traced"] == 1, la2
        assert sc.stats()["bvhBuildMs"] == 0.0 and sc.update_counts() == {"full": 1, "transform": 0, "material": 0} and sc.vertex_update_count() == 1
        ref, _ = orc.render(sc.desc, rs, W, H, threads=8)  # the accumulation restarted: the oracle's first frame of the deformed scene
        assert _bits_equal(img, ref)
    finally:
        sc.close()


TWO_CONTEXTS = textwrap.dedent("""
    import copy, sys
    sys.path.insert(0, %(root)r)
    sys.path.insert(0, %(tests)r)
    from gatling_amd import capi
    import test_vertex_edits as T
    L = capi.initialize(0)                      # $GATLING_DEVICES = "0,0": two contexts on the one GPU
    assert L.giCGetDeviceCount() == 2
    multi = T._make("host")
    single = T._make("host"); single.set_option(capi.OPTION_DEVICES, 1)
    start = copy.deepcopy(multi.desc)
    for sc in (multi, single):
        sc.render_aovs(T.RS, T.W, T.H, T.AOVS)
    for step, edit, _ in T.SEQUENCE[:3]:
        out = []
        for sc in (multi, single):
            edit(sc, start)
            out.append(sc.render_aovs(T.RS, T.W, T.H, T.AOVS))
            assert sc.stats()["bvhBuildMs"] == 0.0, (step, sc.stats()["bvhBuildMs"])
        for k in out[0]:
            assert T._bits_equal(out[0][k], out[1][k]), step + ": " + k + " differs between two device contexts and one"
    assert multi.update_counts() == {"full": 1, "transform": 0, "material": 0} and multi.vertex_update_count() == 3
    for d in (0, 1):
        assert multi.validate_bvh(d)["digest"] == single.validate_bvh(0)["digest"] and multi.refit_check(d)["differing"] == 0
    fresh = capi.Scene(copy.deepcopy(multi.desc)); fresh.set_option(capi.OPTION_DEVICES, 1)
    ref = fresh.render_aovs(T.RS, T.W, T.H, T.AOVS)
    for k in ref:
        assert T._bits_equal(out[0][k], ref[k]), k + " differs from a scene built from scratch"
    multi.close(); single.close(); fresh.close()
    print("two contexts ok")
""")


@pytest.mark.gpu
def test_vertex_edits_reach_every_device_context():
    env = dict(os.environ); env["GATLING_DEVICES"] = "0,0"
    out = subprocess.run([sys.executable, "-c", TWO_CONTEXTS % {"root": ROOT, "tests": os.path.join(ROOT, "tests")}], capture_output=True, text=True, timeout=300,
                         env=env)
    assert out.returncode == 0 and "two contexts ok" in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]


def _random_edit(rng, sc):
    d = sc.desc
    kind = int(rng.choice(5, p=np.float64([4, 1, 1, 1, 1]) / 8.0))
    meshes = [i for i, m in enumerate(d.meshes) if m.name.startswith("/Clutter")]
    mi, other = (int(x) for x in rng.choice(meshes, 2, replace=False))
    deform = lambda i: sc.set_mesh_vertices(i, _deformed(d.meshes[i].vertices, float(rng.uniform(0.02, 0.3)), int(rng.integers(1 << 30))))
    if kind == 0:
        deform(mi); return "deform"
    if kind == 1:
        deform(mi); deform(other); return "deform-two"
    if kind == 2:
        deform(mi); sc.set_mesh_transform(other, np.asarray(d.meshes[other].transform, np.float32).reshape(4, 4) @ _translate(*rng.uniform(-0.2, 0.2, 3)))
        return "deform+transform"
    if kind == 3:
        deform(mi); sc.set_mesh_visibility(other, not d.meshes[other].visible); return "deform+visibility"
    deform(mi); sc.set_mesh_material(other, int(rng.integers(len(d.materials)))); return "deform+assign"


@pytest.mark.gpu
def test_random_edit_sequences_match_the_oracle(gi, orc):
    """20 sequences of four random edits each, every one with a deformation, both options on and the builders alternating; every render is compared with the
    oracle's render of the description at that point."""
    rs = RenderSettings(spp=1, max_bounces=3, next_event_estimation=True, progressive_accumulation=False)
    rng = np.random.default_rng(31337)
    kinds, counts = {}, {"full": 0, "transform": 0, "material": 0, "visibility": 0, "vertex": 0}
    scenes = 20
    for seq in range(scenes):
        sc = _make("device" if seq % 2 else "host", visibility=True)
        try:
            sc.render(rs, W, H)
            for k in range(4):
                kind = _random_edit(rng, sc)
                kinds[kind] = kinds.get(kind, 0) + 1
                img = sc.render(rs, W, H)
                ref, _ = orc.render(sc.desc, rs, W, H, threads=8)
                assert _bits_equal(img, ref), (seq, k, kind)
            # the tree check wants every triangle reachable (a partitioned tree leaves the parts of hidden meshes out of its top tree): everything is shown first
            hidden = [i for i, m in enumerate(sc.desc.meshes) if not m.visible]
            for i in hidden:
                sc.set_mesh_visibility(i, True)
            img = sc.render(rs, W, H)
            ref, _ = orc.render(sc.desc, rs, W, H, threads=8)
            assert _bits_equal(img, ref), (seq, "show", hidden)
            v, r = sc.validate_bvh(), sc.refit_check()
            print(f"sequence {seq}: shown again {hidden}, counts {sc.update_counts()} vertex {sc.vertex_update_count()} visibility {sc.visibility_update_count()}, tree {v}, refit check {r}")
            assert v["violations"] == 0 and r["differing"] == 0, (seq, hidden, v, r)
            c = sc.update_counts()
            for name in ("full", "transform", "material"):
                counts[name] += c[name]
            counts["visibility"] += sc.visibility_update_count(); counts["vertex"] += sc.vertex_update_count()
        finally:
            sc.close()
    print("random vertex edit sequences:", kinds, counts)
    assert counts["vertex"] > scenes and counts["transform"] > 0 and counts["visibility"] > 0 and counts["material"] > 0


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# CPU: the host refit and the host builder under AddressSanitizer + UBSan, as a program of its own (tests/cpp/refit_sanitize.cpp)
# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
def test_host_refit_and_builder_run_clean_under_the_sanitizers(tmp_path):
    # (the sanitizer runtimes are linked statically: the program stands alone whatever else the process environment loads)
    exe = str(tmp_path / "refit_sanitize")
    csrc = os.path.join(ROOT, "gatling_amd", "csrc")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-pthread", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-I", csrc, "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "cpp", "refit_sanitize.cpp"), os.path.join(csrc, "bvh8.cpp"), "-o", exe]
    probe = subprocess.run(["g++", "-fsanitize=address,undefined", "-static-libasan", "-static-libubsan", "-x", "c++", "-", "-o", str(tmp_path / "probe")], input="int main(){return 0;}", text=True,
                           capture_output=True)
    if probe.returncode != 0:
        pytest.skip("the toolchain has no sanitizer runtimes")
    built = subprocess.run(cmd, capture_output=True, text=True)
    assert built.returncode == 0, built.stderr[-4000:]
    env = dict(os.environ); env["GATLING_BUILD_THREADS"] = "4"
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    assert out.returncode == 0 and "refit sanitize ok" in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]

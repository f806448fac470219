"""Vertex edits on the two-level layout without a rebuild (gi_build.cpp updateVerticesTwoLevel, gi_blas.h, gi_blas.hip k_blas_tris /
k_blas_refit_level): with GI_C_SCENE_OPTION_BLAS_UPDATES beside GI_C_SCENE_OPTION_VERTEX_UPDATES a giCSetMeshVertices on a mesh of a built two-level scene no
longer rebuilds it.  The next render re-sends the mesh's vertex records, makes its shading records and BLAS triangles again on the device, refits the mesh's
one BLAS level by level, makes the world boxes of its instances, builds the TLAS again and refits the flat tree that AOVs and giCTraceRays walk.  The image
and the AOVs must be bit-identical to a scene built from scratch and to the oracle's render of the description; the resident BLAS must be bytewise what the
host form of the refit gives, conservative, and after a restore bytewise a fresh build's.  No tolerance anywhere.

CPU: the header, the library and the harness declare option 17, the counter and the three hooks; the API version and the vertex setter's dirty flags are
unchanged; the host form of the BLAS refit keeps a BLAS conservative and its topology under the five motions of tests/test_vertex_edits.py, and leaves the
build's bytes where nothing moved; the same under AddressSanitizer + UBSan as a program of its own (tests/cpp/blas_refit_sanitize.cpp).
GPU: the edit sequence of tests/test_vertex_edits.py with the option on and off, the kernels' shapes, the declines, the composition with a transform edit, a
material edit and the look-ahead window, giCTraceRays, two device contexts, random edit sequences against the oracle.

The scene, the render settings and the helpers are those of tests/test_visibility_edits.py, test_vertex_edits.py and test_tlas_edits.py (6 412 flattened
triangles in 21 instances of 12 meshes; GI_C_SCENE_OPTION_TWO_LEVEL = 1 gives the two-level layout)."""
import copy
import os
import re
import subprocess
import sys
import textwrap

import numpy as np
import pytest

from gatling_amd import capi
from gatling_amd.scene import VERTEX_DTYPE, RenderSettings

from test_hostile_inputs import sanitised
from test_tlas_edits import _description_is_usable, _instances, _scale, _transform
from test_vertex_edits import SEQUENCE, _deformed, _moved, _soup
from test_visibility_edits import (A, AOVS, B, CUT, DIFFUSE_MATERIAL, H, MOVED, REASSIGNED, RS, W, _bits_equal, _check, _fresh_image, _lookdev_scene, _oracle,
                                   _translate)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COUNTS_AS_BUILT = {"full": 1, "transform": 0, "material": 0}


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
def test_header_declares_the_option_the_counter_and_the_hooks_and_keeps_api_version_8():
    text = open(os.path.join(ROOT, "include", "gi_c.h")).read()
    assert re.search(r"#define\s+GI_C_SCENE_OPTION_BLAS_UPDATES\s+17\b", text)
    assert re.search(r"int\s+giCDebugSceneBlasUpdateCount\s*\(\s*const\s+GiCScene\s*\*\s*\w+\s*,\s*uint64_t\s*\*", text)
    assert re.search(r"int\s+giCDebugSceneBlasCheck\s*\(\s*const\s+GiCScene\s*\*\s*\w+\s*,\s*uint32_t\s+\w+\s*,\s*uint32_t\s*\*", text)
    assert re.search(r"int\s+giCDebugBlasRefit\s*\(\s*const\s+GiCVertex\s*\*", text)
    assert re.search(r"int\s+giCDebugBlasRefitHost\s*\(\s*const\s+GiCVertex\s*\*", text)
    assert re.search(r"#define\s+GI_C_API_VERSION\s+8u?\b", text)


def test_library_exports_the_symbols():
    L = capi.load_library()
    assert L.giCGetApiVersion() == 8
    for name in ("giCDebugSceneBlasUpdateCount", "giCDebugSceneBlasCheck", "giCDebugBlasRefit", "giCDebugBlasRefitHost"):
        assert hasattr(L, name), name


def test_harness_exposes_the_option_and_the_methods():
    assert capi.OPTION_BLAS_UPDATES == 17
    assert callable(capi.Scene.blas_update_count) and callable(capi.Scene.blas_check) and callable(capi.debug_blas_refit)


def test_vertex_setter_keeps_its_dirty_flags():
    L = capi.load_library()
    for built in (0, 1):
        assert L.giCDebugEditDirtyFlags(16, built) == 1 | 2  # DIRTY_BVH | DIRTY_FRAMEBUFFER


def _mesh_of(tris):
    """A triangle soup (float32 [n, 3, 3]) as an unindexed mesh: vertices (VERTEX_DTYPE) and faces."""
    v = np.zeros(3 * len(tris), VERTEX_DTYPE)
    v["pos"] = np.asarray(tris, np.float32).reshape(-1, 3)
    v["norm"][:, 2] = 1.0; v["tangent"][:, 0] = 1.0; v["bitangentSign"] = 1.0
    return v, np.arange(3 * len(tris), dtype=np.uint32).reshape(-1, 3)


CASES = ["smooth", "scatter", "collapsed", "far", "same"]


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("n", [1, 3, 46, 777, 20000])
def test_host_blas_refit_keeps_the_blas_conservative_and_its_topology(n, case):
    a = _soup(n, 100 + n)
    b = _moved(a, case, n)
    assert np.isfinite(b).all() and np.abs(b).max() < 1.0e18
    (va, f), (vb, _) = _mesh_of(a), _mesh_of(b)
    differing, nodes, violations = capi.debug_blas_refit(va, vb, f, host_only=True)
    assert violations == 0, (n, case, violations)
    assert differing == 0 and nodes >= 1, (n, case, differing)  # the topology is the build's; for "same" every byte is


def test_host_blas_refit_and_box_builder_run_clean_under_the_sanitizers(tmp_path):
    # (the sanitizer runtimes are linked statically: the program stands alone whatever else the process environment loads)
    exe = str(tmp_path / "blas_refit_sanitize")
    csrc = os.path.join(ROOT, "gatling_amd", "csrc")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-pthread", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-I", csrc, "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "cpp", "blas_refit_sanitize.cpp"), os.path.join(csrc, "bvh8.cpp"), "-o", exe]
    probe = subprocess.run(["g++", "-fsanitize=address,undefined", "-static-libasan", "-static-libubsan", "-x", "c++", "-", "-o", str(tmp_path / "probe")], input="int main(){return 0;}", text=True,
                           capture_output=True)
    if probe.returncode != 0:
        pytest.skip("the toolchain has no sanitizer runtimes")
    built = subprocess.run(cmd, capture_output=True, text=True)
    assert built.returncode == 0, built.stderr[-4000:]
    env = dict(os.environ); env["GATLING_BUILD_THREADS"] = "4"
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    assert out.returncode == 0 and "blas refit sanitize ok" in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# the edit sequence of tests/test_vertex_edits.py on the two-level layout
# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
def _make(option_on=True, vertex_updates=True, tlas_updates=False, desc=None):
    sc = capi.Scene(desc if desc is not None else _lookdev_scene())
    sc.set_option(capi.OPTION_TWO_LEVEL, 1)
    if vertex_updates:
        sc.set_option(capi.OPTION_VERTEX_UPDATES, 1)
    if option_on:
        sc.set_option(capi.OPTION_BLAS_UPDATES, 1)
    if tlas_updates:
        sc.set_option(capi.OPTION_TLAS_UPDATES, 1)
    return sc


def _resident_checks(sc, key, devices=(0,)):
    for d in devices:
        c = sc.blas_check(d)
        meshes = [m for m in sc.desc.meshes if m.visible and len(m.instance_transforms)]  # one BLAS per mesh of the built scene, over its faces
        assert c == 0 and c.two_level == 1 and c.violations == 0 and c.blas_nodes >= len(meshes) and c.blas_tris == sum(len(m.faces) for m in meshes), (
            key, d, int(c), c.two_level, c.violations, c.blas_nodes, c.blas_tris)
        assert sc.validate_bvh(d)["violations"] == 0, (key, d)


def _run_sequence(orc, option_on):
    sc = _make(option_on)
    start = copy.deepcopy(sc.desc)
    try:
        first = sc.render_aovs(RS, W, H, AOVS)
        built_ms = sc.stats()["bvhBuildMs"]  # the flat tree over 6 412 triangles, twelve BLASes and the TLAS
        assert sc.update_counts() == COUNTS_AS_BUILT and sc.blas_update_count() == 0 and sc.vertex_update_count() == 0 and built_ms > 0.0
        _resident_checks(sc, "start")
        assert sc.tlas_check() == 0
        _check(orc, sc, "start", first)
        for step, edit, moved in SEQUENCE:
            before, blas_before = sc.update_counts(), sc.blas_update_count()
            edit(sc, start)
            got = sc.render_aovs(RS, W, H, AOVS)
            st, after, blas_after = sc.stats(), sc.update_counts(), sc.blas_update_count()
            print(f"option {int(option_on)} {step}: bvhBuildMs {st['bvhBuildMs']:.3f} uploadMs {st['uploadMs']:.3f} counts {after} blas {blas_after}")
            if option_on:
                assert after == before and blas_after == blas_before + 1, (step, before, after, blas_after)
                # the host TLAS build over 21 boxes alone: a part of what the scene build ran, over 1 / 300 of its items
                assert 0.0 <= st["bvhBuildMs"] < built_ms, (step, st["bvhBuildMs"], built_ms)
            else:  # the parent's behaviour: every vertex edit of a two-level scene rebuilds
                assert after == {"full": before["full"] + 1, "transform": 0, "material": 0} and blas_after == 0 and st["bvhBuildMs"] > 0.0, (step, after, blas_after)
            assert sc.vertex_update_count() == 0 and st["triangleCount"] == 6412, (step, sc.vertex_update_count(), st)
            _resident_checks(sc, step)
            _check(orc, sc, step, got)
            if moved:
                assert not _bits_equal(got["color"], first["color"]) and not _bits_equal(got["depth"], first["depth"]), f"{step}: nothing moved"
        assert sc.tlas_check() == 0  # the whole two-level set, BLAS nodes and triangles included, is bytewise a fresh build's again
        for k in ["color"] + AOVS:
            assert _bits_equal(got[k], first[k]), f"{k} after the restore differs from the first render"
    finally:
        sc.close()


@pytest.mark.gpu
def test_vertex_edits_refit_the_blas_of_a_two_level_scene_in_place_and_bit_exactly(gi, orc):
    _run_sequence(orc, True)


@pytest.mark.gpu
def test_with_the_option_off_the_same_edits_rebuild_and_give_the_same_bits(gi, orc):
    _run_sequence(orc, False)


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# the kernels: lane, wave, workgroup, leaf-size and level edges
# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("faces", [1, 2, 7, 8, 9, 63, 64, 65, 255, 256, 257, 4097, 20000])
def test_blas_refit_kernels_match_the_host_form_at_every_edge(gi, faces):
    a = _soup(faces, 300 + faces)
    va, f = _mesh_of(a)
    for case in CASES:
        vb, _ = _mesh_of(_moved(a, case, faces))
        differing, nodes, violations = capi.debug_blas_refit(va, vb, f)
        print(f"{faces} faces, {case}: {nodes} node(s), differing {differing}, violations {violations}")
        assert differing == 0 and violations == 0 and nodes >= 1, (faces, case, differing, violations)  # ("same": the build's bytes as well)


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# declines
# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
def _expect_rebuild(orc, sc, key, full, blas, oracle_desc=None):
    img = sc.render(RS, W, H)
    assert sc.update_counts()["full"] == full and sc.blas_update_count() == blas and sc.vertex_update_count() == 0, (key, sc.update_counts(), sc.blas_update_count())
    assert sc.stats()["bvhBuildMs"] > 0.0
    assert _bits_equal(img, _fresh_image(sc.desc)), f"{key}: differs from a scene built from scratch"
    assert _bits_equal(img, _oracle(orc, key, oracle_desc if oracle_desc is not None else sc.desc)[0]), f"{key}: differs from the oracle"


def _expect_update(sc, key, full, blas, mesh=A, seed=50):
    sc.set_mesh_vertices(mesh, _deformed(sc.desc.meshes[mesh].vertices, 0.05, seed))
    img = sc.render(RS, W, H)
    assert sc.update_counts()["full"] == full and sc.blas_update_count() == blas and sc.vertex_update_count() == 0, (key, sc.update_counts(), sc.blas_update_count())
    _resident_checks(sc, key)
    assert _bits_equal(img, _fresh_image(sc.desc)), f"{key}: differs from a scene built from scratch"


@pytest.mark.gpu
@pytest.mark.parametrize("bad", [float("nan"), 1.0e19])
def test_unusable_position_rebuilds_and_matches_the_oracle(gi, orc, bad):
    sc = _make()
    start = copy.deepcopy(sc.desc)
    try:
        sc.render(RS, W, H)
        v = _deformed(sc.desc.meshes[A].vertices, 0.1, 7)
        v["pos"][5, 1] = bad
        sc.set_mesh_vertices(A, v)
        _expect_rebuild(orc, sc, f"vx-unusable-{bad}", 2, 0, sanitised(sc.desc))  # the oracle is fed ordinary geometry in place of the inactive faces
        assert sc.stats()["inactiveTriangleCount"] > 0
        sc.set_mesh_vertices(A, start.meshes[A].vertices)  # (the resident scene holds inactive triangles: the restore rebuilds too)
        _expect_rebuild(orc, sc, "start", 3, 0)
        _expect_update(sc, f"bl-unusable-{bad}-after", 3, 1)
    finally:
        sc.close()


def _scaled_cutout_scene():
    """The scene with the cutout mesh's one instance eight times as large where it stands: object-space coordinates reach the world 2.4 times as large."""
    d = _lookdev_scene()
    t = _instances(d, CUT); assert len(t) == 1
    t[0] = _scale(8.0, 8.0, 8.0) @ t[0]
    d.meshes[CUT].instance_transforms = t
    return d


@pytest.mark.gpu
def test_position_usable_in_object_space_but_not_in_world_space_rebuilds(gi, orc):
    """The status of k_inst_bounds declines (WORLD): nothing resident was written, the rebuild holds the faces as inactive ones."""
    d = _scaled_cutout_scene()
    sc = _make(desc=d)
    start = copy.deepcopy(sc.desc)
    try:
        sc.render(RS, W, H)
        assert sc.blas_check() == 0 and sc.blas_check().two_level == 1
        m = sc.desc.meshes[CUT]
        xf = _transform(sc.desc, CUT) @ _instances(sc.desc, CUT)[0]
        col = int(np.argmax(np.abs(xf[:3, :3]).sum(axis=0)))
        p = (np.float32(9.0e17) * np.sign(xf[:3, col])).astype(np.float32)
        world = p @ xf[:3, :3] + xf[3, :3]
        assert np.abs(p).max() <= 1.0e18 and np.abs(world).max() > 1.0e18, (p, world)  # usable in object space, beyond the range in the world
        v = np.array(m.vertices, copy=True); v["pos"][5] = p
        sc.set_mesh_vertices(CUT, v)
        oracle_desc = copy.deepcopy(sc.desc)
        ov = np.array(oracle_desc.meshes[CUT].vertices, copy=True); ov["pos"][5, 0] = np.nan  # (the faces on that vertex are inactive under the one instance)
        oracle_desc.meshes[CUT].vertices = ov
        _expect_rebuild(orc, sc, "bl-world-unusable", 2, 0, sanitised(oracle_desc))
        assert sc.stats()["inactiveTriangleCount"] > 0
        sc.set_mesh_vertices(CUT, start.meshes[CUT].vertices)
        _expect_rebuild(orc, sc, "bl-scaled-cutout-start", 3, 0)
        _expect_update(sc, "bl-world-unusable-after", 3, 1, mesh=CUT)
    finally:
        sc.close()


@pytest.mark.gpu
def test_mesh_invisible_at_the_build_rebuilds(gi, orc):
    d = _lookdev_scene()
    d.meshes[B].visible = False
    sc = _make(desc=d)
    try:
        sc.render(RS, W, H)
        sc.set_mesh_vertices(B, _deformed(sc.desc.meshes[B].vertices, 0.1, 9))  # no records on the device
        _expect_rebuild(orc, sc, "vx-invisible-deformed", 2, 0)
        _expect_update(sc, "bl-invisible-after", 2, 1)
    finally:
        sc.close()


@pytest.mark.gpu
def test_scene_below_the_triangle_floor_rebuilds(gi, orc):
    d = _lookdev_scene()
    d.meshes = d.meshes[:8]  # the room and seven clutter meshes, 3 852 flattened triangles: below the 4 096 floor, still beyond LDS
    assert 128 < d.triangle_count() < 4096
    sc = _make(desc=d)
    try:
        sc.render(RS, W, H)
        assert sc.blas_check().two_level == 1
        sc.set_mesh_vertices(A, _deformed(sc.desc.meshes[A].vertices, 0.1, 13))
        _expect_rebuild(orc, sc, "bl-below-the-floor", 2, 0)
    finally:
        sc.close()


@pytest.mark.gpu
def test_incremental_0_rebuilds(gi, orc, monkeypatch):
    sc = _make()
    try:
        sc.render(RS, W, H)
        monkeypatch.setenv("GATLING_OPTIONS", "incremental=0")
        sc.set_mesh_vertices(A, _deformed(sc.desc.meshes[A].vertices, 0.1, 14))
        _expect_rebuild(orc, sc, "vx-incremental-0", 2, 0)
        monkeypatch.delenv("GATLING_OPTIONS")
        _expect_update(sc, "bl-incremental-0-after", 2, 1)
    finally:
        sc.close()


@pytest.mark.gpu
def test_option_17_without_vertex_updates_rebuilds(gi, orc):
    sc = _make(option_on=True, vertex_updates=False)
    try:
        sc.render(RS, W, H)
        sc.set_mesh_vertices(A, _deformed(sc.desc.meshes[A].vertices, 0.1, 15))
        _expect_rebuild(orc, sc, "bl-option-12-off", 2, 0)
        sc.set_option(capi.OPTION_VERTEX_UPDATES, 1)
        _expect_update(sc, "bl-option-12-on-after", 2, 1)
    finally:
        sc.close()


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# composition: a transform edit, a material edit, the look-ahead window, giCTraceRays
# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_deform_and_instance_move_compose_in_one_render(gi, orc):
    sc = _make(tlas_updates=True)
    start = copy.deepcopy(sc.desc)
    try:
        sc.render(RS, W, H)
        sc.set_mesh_vertices(A, _deformed(start.meshes[A].vertices, 0.12, 21))
        t = _instances(sc.desc, A); t[1] = t[1] @ _translate(0.2, 0.1, -0.1)  # the deformed mesh's own instance moves ...
        sc.set_mesh_instance_transforms(A, t)
        t = _instances(sc.desc, MOVED); t[0] = t[0] @ _translate(-0.1, 0.1, 0.1)  # ... and another mesh's
        sc.set_mesh_instance_transforms(MOVED, t)
        got = sc.render_aovs(RS, W, H, AOVS)
        assert sc.update_counts() == COUNTS_AS_BUILT and sc.blas_update_count() == 1 and sc.tlas_update_count() == 1, (sc.update_counts(), sc.blas_update_count(),
                                                                                                                       sc.tlas_update_count())
        _resident_checks(sc, "bl-deform-and-move")
        _check(orc, sc, "bl-deform-and-move", got)
    finally:
        sc.close()


@pytest.mark.gpu
def test_deform_and_material_reassignment_compose_in_one_render(gi, orc):
    sc = _make()
    try:
        sc.render(RS, W, H)
        sc.set_mesh_vertices(REASSIGNED, _deformed(sc.desc.meshes[REASSIGNED].vertices, 0.12, 22))
        sc.set_mesh_material(REASSIGNED, DIFFUSE_MATERIAL)  # (the deformed mesh's word changes: InstTrav::matFlags of its instances with it)
        got = sc.render_aovs(RS, W, H, AOVS)
        assert sc.update_counts() == {"full": 1, "transform": 0, "material": 1} and sc.blas_update_count() == 1, (sc.update_counts(), sc.blas_update_count())
        _resident_checks(sc, "bl-deform-and-assign")
        _check(orc, sc, "bl-deform-and-assign", got)
    finally:
        sc.close()


@pytest.mark.gpu
def test_deform_discards_the_look_ahead_window(gi, orc):
    rs = RenderSettings(spp=1, max_bounces=3, next_event_estimation=True)  # progressive
    sc = _make()
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
        assert sc.update_counts() == COUNTS_AS_BUILT and sc.blas_update_count() == 1
        ref, _ = orc.render(sc.desc, rs, W, H, threads=8)  # the accumulation restarted: the oracle's first frame of the deformed scene
        assert _bits_equal(img, ref)
    finally:
        sc.close()


@pytest.mark.gpu
def test_trace_rays_after_a_deform_answers_like_a_fresh_scene(gi):
    rng = np.random.default_rng(78)
    origins = np.tile(np.float32([0.0, 1.2, 0.0]), (256, 1)) + rng.uniform(-0.3, 0.3, (256, 3)).astype(np.float32)
    dirs = rng.normal(size=(256, 3)); dirs = (dirs / np.linalg.norm(dirs, axis=1, keepdims=True)).astype(np.float32)
    sc = _make()
    try:
        sc.render(RS, W, H)
        before = sc.trace_rays(origins, dirs)
        for i in (A, B, MOVED, CUT):
            sc.set_mesh_vertices(i, _deformed(sc.desc.meshes[i].vertices, 0.2, 60 + i))
        sc.render(RS, W, H)
        assert sc.update_counts()["full"] == 1 and sc.blas_update_count() == 1
        got = sc.trace_rays(origins, dirs)
        fresh = capi.Scene(copy.deepcopy(sc.desc))
        try:
            fresh.render(RS, W, H)
            want = fresh.trace_rays(origins, dirs)
        finally:
            fresh.close()
        moved = False
        for a, b, c in zip(got, want, before):
            assert _bits_equal(np.asarray(a), np.asarray(b))
            moved = moved or not _bits_equal(np.asarray(a), np.asarray(c))
        assert moved, "no ray met what was deformed"
    finally:
        sc.close()


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# two device contexts
# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
TWO_CONTEXTS = textwrap.dedent("""
    import copy, sys
    sys.path.insert(0, %(root)r)
    sys.path.insert(0, %(tests)r)
    from gatling_amd import capi
    import test_blas_edits as T
    L = capi.initialize(0)                      # $GATLING_DEVICES = "0,0": two contexts on the one GPU
    assert L.giCGetDeviceCount() == 2
    multi = T._make()
    single = T._make(); single.set_option(capi.OPTION_DEVICES, 1)
    start = copy.deepcopy(multi.desc)
    for sc in (multi, single):
        sc.render_aovs(T.RS, T.W, T.H, T.AOVS)
    for step, edit, _ in T.SEQUENCE[:3]:
        out = []
        for sc in (multi, single):
            edit(sc, start)
            out.append(sc.render_aovs(T.RS, T.W, T.H, T.AOVS))
        for k in out[0]:
            assert T._bits_equal(out[0][k], out[1][k]), step + ": " + k + " differs between two device contexts and one"
        T._resident_checks(multi, step, devices=(0, 1))
        assert multi.validate_bvh(0)["digest"] == multi.validate_bvh(1)["digest"] == single.validate_bvh(0)["digest"], step
    assert multi.update_counts() == {"full": 1, "transform": 0, "material": 0} and multi.blas_update_count() == 3
    fresh = capi.Scene(copy.deepcopy(multi.desc)); fresh.set_option(capi.OPTION_DEVICES, 1)
    ref = fresh.render_aovs(T.RS, T.W, T.H, T.AOVS)
    for k in ref:
        assert T._bits_equal(out[0][k], ref[k]), k + " differs from a scene built from scratch"
    multi.close(); single.close(); fresh.close()
    print("two contexts ok")
""")


@pytest.mark.gpu
def test_blas_edits_reach_every_device_context():
    env = dict(os.environ); env["GATLING_DEVICES"] = "0,0"
    out = subprocess.run([sys.executable, "-c", TWO_CONTEXTS % {"root": ROOT, "tests": os.path.join(ROOT, "tests")}], capture_output=True, text=True, timeout=300,
                         env=env)
    assert out.returncode == 0 and "two contexts ok" in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# random sequences
# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
def _random_edit(rng, sc):
    """tests/test_vertex_edits.py _random_edit without the visibility kind (a toggle rebuilds on this layout): every edit deforms a clutter mesh by 0.02 - 0.3."""
    d = sc.desc
    kind = int(rng.choice(4, p=np.float64([4, 1, 1, 1]) / 7.0))
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
    deform(mi); sc.set_mesh_material(other, int(rng.integers(len(d.materials)))); return "deform+assign"


@pytest.mark.gpu
def test_random_edit_sequences_match_the_oracle(gi, orc):
    """20 sequences of four random edits each, every one with a deformation, options 12, 16 and 17 on; every render is compared with the oracle's render of
    the description at that point, and the resident BLASes are checked after each.  The drawn inputs keep every position finite and within a few units
    (displacements of at most 0.3 of points inside the room, translations of at most 0.2 per edit), which is checked on the description's own boxes before
    every render; the depth rule is out of reach of 21 instances.  So no drawn case may decline: the scene's first build must stay its only one."""
    rs = RenderSettings(spp=1, max_bounces=3, next_event_estimation=True, progressive_accumulation=False)
    rng = np.random.default_rng(171717)
    kinds, totals = {}, {"blas": 0, "tlas": 0, "material": 0}
    for seq in range(20):
        sc = _make(tlas_updates=True)
        try:
            sc.render(rs, W, H)
            for k in range(4):
                kind = _random_edit(rng, sc)
                kinds[kind] = kinds.get(kind, 0) + 1
                assert _description_is_usable(sc.desc), (seq, k, kind)
                img = sc.render(rs, W, H)
                ref, _ = orc.render(sc.desc, rs, W, H, threads=8)
                assert _bits_equal(img, ref), (seq, k, kind)
                assert sc.blas_check() == 0, (seq, k, kind)
            c = sc.update_counts()
            assert c["full"] == 1 and c["transform"] == 0 and sc.vertex_update_count() == 0, (seq, c)
            assert sc.blas_update_count() == 4, (seq, sc.blas_update_count())
            totals["blas"] += sc.blas_update_count(); totals["tlas"] += sc.tlas_update_count(); totals["material"] += c["material"]
        finally:
            sc.close()
    print("random BLAS edit sequences:", kinds, totals)
    assert totals["blas"] > 0 and totals["tlas"] > 0 and totals["material"] > 0

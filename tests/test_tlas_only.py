"""Two-level scenes without the flat tree (gi_build.cpp buildSceneTreeless, gi_aov2.hip k_aov2, gi_tlas.h tlas_scene_bounds): with
GI_C_SCENE_OPTION_TLAS_ONLY, read at the build of a scene that wants the two-level layout, the flat BVH8 over all flattened triangles is neither built nor
sent nor kept.  The flat records stay in scene order, the non-colour AOVs find their primary hits with the two-level walk (k_aov2 instead of k_aov), the scene
bounds are the union of the instance boxes, and the edits in place of options 16, 17 and 18 run without the flat refit.  Nothing may change in an image: the
colour and every AOV must be bit-identical to the same description rendered with the option off (the flat k_aov), to a scene built from scratch and to the
oracle's render.  No tolerance anywhere.

CPU: the header, the library and the harness declare the option and the hook; the API version is unchanged; the bounds function runs clean under the
sanitizers as a program of its own, held to a brute-force union.
GPU: the state of the scene with the option on and off, colour and nine AOVs, the AOV kernel at the edges of its launch (fewer lanes than a wave, a partial
wave in the last block, exactly one block, spp 1 and 3, a progressive second call, a row share, waves whose every lane misses, the cutout test, the
instantiation without it), giCTraceRays, the edits in place and the same edits as rebuilds, hide / move / show of a far instance, the declines to the flat build, two device contexts, random
edit sequences.

The scene, the render settings and the helpers are those of tests/test_visibility_edits.py (6 412 flattened triangles in 21 instances of 12 meshes, one of
them bound to a cutout material: above the 4 096 floor of the edits in place and beyond LDS)."""
import copy
import os
import re
import subprocess
import sys
import textwrap

import numpy as np
import pytest

from gatling_amd import capi
from gatling_amd.scene import MAT_DIFFUSE, RenderSettings
from gatling_amd.scenes import _look_at_camera, cornell_box

from test_hostile_inputs import sanitised
from test_tlas_edits import _instances, _scale, _transform
from test_tlas_visibility_edits import _random_edit
from test_vertex_edits import _deformed
from test_visibility_edits import (AOVS, B, CUT, CUTOUT_MATERIAL, DIFFUSE_MATERIAL, H, MOVED, REASSIGNED, RS, W, _bits_equal, _check, _lookdev_scene, _translate)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TREELESS = {"two_level": 1, "treeless": 1, "resident_nodes": 0, "host_node_bytes": 0}
EDIT_OPTIONS = ("OPTION_VISIBILITY_UPDATES", "OPTION_VERTEX_UPDATES", "OPTION_TLAS_UPDATES", "OPTION_BLAS_UPDATES", "OPTION_TLAS_VISIBILITY")  # 11, 12, 16, 17, 18


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
def test_header_declares_the_option_and_the_hook_and_keeps_api_version_8():
    text = open(os.path.join(ROOT, "include", "gi_c.h")).read()
    assert re.search(r"#define\s+GI_C_SCENE_OPTION_TLAS_ONLY\s+19\b", text)
    assert re.search(r"int\s+giCDebugSceneFlatTreeState\s*\(\s*const\s+GiCScene\s*\*\s*\w+\s*,\s*uint32_t\s+\w+\s*,\s*uint64_t\s+\w+\s*\[\s*4\s*\]\s*\)", text)
    assert re.search(r"#define\s+GI_C_API_VERSION\s+8u?\b", text)


def test_library_exports_the_symbol():
    L = capi.load_library()
    assert L.giCGetApiVersion() == 8
    assert hasattr(L, "giCDebugSceneFlatTreeState")


def test_harness_exposes_the_option_and_the_method():
    assert capi.OPTION_TLAS_ONLY == 19
    assert callable(capi.Scene.flat_tree_state)


def test_scene_bounds_from_instance_boxes_run_clean_under_the_sanitizers(tmp_path):
    # (the sanitizer runtimes are linked statically: the program stands alone whatever else the process environment loads)
    exe = str(tmp_path / "tlas_bounds_sanitize")
    csrc = os.path.join(ROOT, "gatling_amd", "csrc")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-I", csrc, "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "cpp", "tlas_bounds_sanitize.cpp"), "-o", exe]
    probe = subprocess.run(["g++", "-fsanitize=address,undefined", "-static-libasan", "-static-libubsan", "-x", "c++", "-", "-o", str(tmp_path / "probe")], input="int main(){return 0;}", text=True,
                           capture_output=True)
    if probe.returncode != 0:
        pytest.skip("the toolchain has no sanitizer runtimes")
    built = subprocess.run(cmd, capture_output=True, text=True)
    assert built.returncode == 0, built.stderr[-4000:]
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "tlas bounds sanitize ok" in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# the scenes
# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
def _make(tlas_only=True, two_level=True, edits=False, desc=None):
    sc = capi.Scene(desc if desc is not None else _lookdev_scene())
    if two_level:
        sc.set_option(capi.OPTION_TWO_LEVEL, 1)
    if tlas_only:
        sc.set_option(capi.OPTION_TLAS_ONLY, 1)
    if edits:
        for name in EDIT_OPTIONS:
            sc.set_option(getattr(capi, name), 1)
    return sc


def _treeless_checks(sc, key, devices=(0,), deformed=False):
    """What every case asserts of a scene without the flat tree: the state, no flat node in the statistics, the two-level arrays bytewise a fresh build's
    (blas_check while a mesh's points are not the build's: its BLAS is then a refitted one), the flat records' ids and the id table."""
    st = sc.stats()
    assert st["nodeCount"] == 0 and st["triangleCount"] == 6412, (key, st)
    for d in devices:
        assert sc.flat_tree_state(d) == TREELESS, (key, d, sc.flat_tree_state(d))
        c, f = sc.blas_check(d) if deformed else sc.tlas_check(d), sc.flat_id_check(d)
        assert c == 0 and c.two_level == 1, (key, d, int(c), c.two_level)
        assert f == 0 and f.two_level == 1 and f.resident_tris == 6412, (key, d, int(f), f.visible_tris, f.resident_tris, f.hidden_instances)


CLEAR = {"objectId": -1, "instanceId": -1, "faceId": -1}  # (the room's object id is 0: a pixel without a hit must not look like it)


def _aov_only(sc, rs, w, h, **kw):
    return sc.render_aovs(rs, w, h, AOVS, CLEAR, with_color=False, **kw)


def _same_aovs(got, want, key, what):
    assert set(got) == set(want), (key, sorted(got), sorted(want))
    for k in want:
        assert _bits_equal(got[k], want[k]), f"{key}: {k} differs from {what}"


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# 1. the state
# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_option_on_builds_no_flat_tree(gi):
    sc = _make()
    try:
        sc.render(RS, W, H)
        assert sc.update_counts() == {"full": 1, "transform": 0, "material": 0}
        assert sc.flat_tree_state() == TREELESS
        st = sc.stats()
        assert st["nodeCount"] == 0 and st["triangleCount"] == 6412 and st["inactiveTriangleCount"] == 0 and st["bvhBuildMs"] > 0.0, st
        c, f = sc.tlas_check(), sc.flat_id_check()
        assert c == 0 and c.two_level == 1 and c.instances == 21 and c.tlas_nodes >= 1, (int(c), c.two_level, c.instances, c.tlas_nodes)
        assert f == 0 and f.two_level == 1 and (f.visible_tris, f.resident_tris, f.hidden_instances) == (6412, 6412, 0), (int(f), f.visible_tris, f.resident_tris)
        with pytest.raises(capi.GiError, match="without the flat tree"):  # no made-up result: there is no tree to validate
            sc.validate_bvh()
    finally:
        sc.close()


@pytest.mark.gpu
def test_option_off_keeps_the_flat_tree(gi):
    sc = _make(tlas_only=False)
    try:
        sc.render(RS, W, H)
        state, st = sc.flat_tree_state(), sc.stats()
        assert state["two_level"] == 1 and state["treeless"] == 0 and state["resident_nodes"] > 0 and state["host_node_bytes"] == 80 * state["resident_nodes"], state
        assert st["nodeCount"] == state["resident_nodes"] and st["triangleCount"] == 6412, (st, state)
        v = sc.validate_bvh()
        assert v["violations"] == 0 and v["nodes"] == state["resident_nodes"], v
        assert sc.tlas_check() == 0 and sc.flat_id_check() == 0
    finally:
        sc.close()


@pytest.mark.gpu
def test_option_on_without_the_two_level_layout_is_a_flat_scene(gi):
    sc = _make(two_level=False)
    try:
        sc.render(RS, W, H)
        state = sc.flat_tree_state()
        assert state["two_level"] == 0 and state["treeless"] == 0 and state["resident_nodes"] > 0, state
        assert sc.stats()["nodeCount"] == state["resident_nodes"] and sc.validate_bvh()["violations"] == 0
    finally:
        sc.close()


@pytest.mark.gpu
def test_option_through_the_environment_wins(gi, monkeypatch):
    on, off = _make(tlas_only=False), _make(tlas_only=True)
    try:
        monkeypatch.setenv("GATLING_OPTIONS", "tlas_only=1")
        on.render(RS, W, H)
        monkeypatch.setenv("GATLING_OPTIONS", "tlas_only=0")
        off.render(RS, W, H)
        monkeypatch.delenv("GATLING_OPTIONS")
        assert on.flat_tree_state() == TREELESS and off.flat_tree_state()["treeless"] == 0 and off.flat_tree_state()["resident_nodes"] > 0
    finally:
        on.close(); off.close()


@pytest.mark.gpu
def test_switching_the_option_on_a_built_scene_rebuilds_and_releases_the_flat_nodes(gi):
    sc = _make(tlas_only=False)
    try:
        first = sc.render_aovs(RS, W, H, AOVS)
        assert sc.flat_tree_state()["resident_nodes"] > 0
        sc.set_option(capi.OPTION_TLAS_ONLY, 1)
        second = sc.render_aovs(RS, W, H, AOVS)
        assert sc.update_counts()["full"] == 2 and sc.flat_tree_state() == TREELESS
        _same_aovs(second, first, "switched on", "the render before the switch")
        sc.set_option(capi.OPTION_TLAS_ONLY, 0)
        third = sc.render_aovs(RS, W, H, AOVS)
        assert sc.update_counts()["full"] == 3 and sc.flat_tree_state()["treeless"] == 0 and sc.validate_bvh()["violations"] == 0
        _same_aovs(third, first, "switched off", "the first render")
    finally:
        sc.close()


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# 2. colour and nine AOVs
# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_colour_and_aovs_equal_the_flat_tree_scene_and_the_oracle(gi, orc):
    on, off = _make(), _make(tlas_only=False)
    try:
        got, ref = on.render_aovs(RS, W, H, AOVS), off.render_aovs(RS, W, H, AOVS)
        assert on.flat_tree_state() == TREELESS and off.flat_tree_state()["treeless"] == 0
        assert on.stats()["inactiveTriangleCount"] == off.stats()["inactiveTriangleCount"] == 0
        _same_aovs(got, ref, "to-start", "the scene with the flat tree")
        _check(orc, on, "start", got)  # a scene built from scratch, and the oracle (the description is the start's of tests/test_visibility_edits.py)
        assert len(np.unique(got["objectId"])) > 3 and len(np.unique(got["instanceId"])) > 1  # (the comparison is not one of two empty images)
    finally:
        on.close(); off.close()


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# 3. the kernel's edges (AOV-only renders: k_aov2 against k_aov and the oracle)
# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
def _edge(orc, desc, rs, w, h, key, calls=1, rows=None, row_stride=1, expect_cutouts=True, coverage=None):
    on, off = _make(desc=copy.deepcopy(desc)), _make(tlas_only=False, desc=copy.deepcopy(desc))
    try:
        prev, offset = None, 0
        for call in range(calls):
            kw = {} if rows is None else {"rows": rows, "row_stride": row_stride}
            got, ref = _aov_only(on, rs, w, h, **kw), _aov_only(off, rs, w, h, **kw)
            assert on.flat_tree_state() == TREELESS and off.flat_tree_state()["treeless"] == 0, key
            assert bool(on.class_state()["hasCutouts"]) == expect_cutouts == bool(off.class_state()["hasCutouts"]), key
            want = orc.render_aovs(desc, rs, w, h, AOVS, CLEAR, sample_offset=offset, prev=prev)
            prev, offset = want, offset + rs.spp
            if rows is not None:
                want = {k: v[rows[0]:rows[1]:row_stride] for k, v in want.items()}
            _same_aovs(got, ref, f"{key} call {call}", "the scene with the flat tree")
            _same_aovs(got, want, f"{key} call {call}", "the oracle")
        if coverage is not None:
            hit = (got["objectId"] >= 0).mean()
            assert coverage[0] <= hit <= coverage[1], (key, hit)
        return got
    finally:
        on.close(); off.close()


@pytest.mark.gpu
@pytest.mark.parametrize("spp", [1, 3])
@pytest.mark.parametrize("size", [(7, 5), (33, 19), (16, 16)])  # 35 pixels: less than a wave; 627: two blocks + a full and a partial wave; 256: one block
def test_aov_kernel_at_the_edges_of_its_launch(gi, orc, size, spp):
    rs = RenderSettings(spp=spp, max_bounces=3, progressive_accumulation=False)
    _edge(orc, _lookdev_scene(), rs, size[0], size[1], f"to-edge-{size[0]}x{size[1]}-spp{spp}")


@pytest.mark.gpu
def test_aov_kernel_progressive_second_call_blends_normal_and_albedo(gi, orc):
    rs = RenderSettings(spp=2, max_bounces=3)  # progressive: the second call starts at sampleOffset 2 and reads what the first left
    _edge(orc, _lookdev_scene(), rs, 33, 19, "to-edge-progressive", calls=2)


@pytest.mark.gpu
def test_aov_kernel_row_share(gi, orc):
    rs = RenderSettings(spp=2, max_bounces=3, progressive_accumulation=False)
    _edge(orc, _lookdev_scene(), rs, 33, 19, "to-edge-rows", rows=(1, 19), row_stride=3)


@pytest.mark.gpu
def test_aov_kernel_with_waves_whose_every_lane_misses(gi, orc):
    """The camera outside the room (x in [-5, 5], y in [-4, 4], z in [0, 3]; z is up), turned so that the room fills a part of the image only: whole waves of
    pixels see nothing and never walk."""
    d = _lookdev_scene()
    d.camera = _look_at_camera((0.0, -20.0, 1.5), (9.0, 0.0, 1.5), (0, 0, 1), 60.0)
    rs = RenderSettings(spp=2, max_bounces=3, progressive_accumulation=False)
    got = _edge(orc, d, rs, 64, 40, "to-edge-misses", coverage=(0.01, 0.6))
    hit = (got["objectId"] >= 0).reshape(-1)
    waves = hit.reshape(-1, 64).any(axis=1)  # 64 consecutive pixels: whatever the tile order, 40 groups of which most must be empty and some not
    assert (~waves).sum() >= 4 and waves.sum() >= 2, (int(waves.sum()), len(waves))


@pytest.mark.gpu
def test_aov_kernel_close_up_of_the_cutout_mesh(gi, orc):
    """Opacity, and the stochastic accept of the any-hit test: the camera looks at the one mesh bound to the cutout material from nearby."""
    d = _lookdev_scene()
    xf = _transform(d, CUT).astype(np.float64) @ _instances(d, CUT)[0].astype(np.float64)  # (row vectors: the mesh's transform, then the instance's)
    q = np.asarray(d.meshes[CUT].vertices["pos"], np.float64) @ xf[:3, :3] + xf[3, :3]
    centre, radius = q.mean(axis=0), float(np.linalg.norm(q - q.mean(axis=0), axis=1).max())
    d.camera = _look_at_camera(tuple(centre + np.float64([0.4, -1.0, 0.5]) / np.linalg.norm([0.4, -1.0, 0.5]) * 2.5 * radius), tuple(centre), (0, 0, 1), 60.0)
    rs = RenderSettings(spp=3, max_bounces=3, progressive_accumulation=False)
    got = _edge(orc, d, rs, 33, 19, "to-edge-cutout")
    op = got["opacity"][..., :3]
    cut = ~((op == np.float32([1.0, 0.0, 0.0])).all(axis=-1))  # (1, 0, 0) is what a hit on an opaque material writes, and the clear value is 0
    assert cut.mean() > 0.05, cut.mean()  # pixels whose accepted hit lies on the cutout material (or that saw through everything)


@pytest.mark.gpu
def test_aov_kernel_without_the_cutout_test(gi, orc):
    d = _lookdev_scene()
    d.materials[CUTOUT_MATERIAL] = copy.deepcopy(d.materials[DIFFUSE_MATERIAL])  # every material opaque: the CUTOUT = false instantiation
    rs = RenderSettings(spp=2, max_bounces=3, progressive_accumulation=False)
    _edge(orc, d, rs, 33, 19, "to-edge-opaque", expect_cutouts=False)


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# 4. giCTraceRays
# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_trace_rays_answer_like_the_scene_with_the_flat_tree(gi):
    on, off = _make(), _make(tlas_only=False)
    try:
        on.render(RS, W, H); off.render(RS, W, H)
        rng = np.random.default_rng(1919)
        p = np.concatenate([np.asarray(m.vertices["pos"], np.float32) for m in on.desc.meshes if not m.name.startswith("/Clutter")])
        lo, hi = p.min(axis=0), p.max(axis=0)
        origins = rng.uniform(lo + 0.1 * (hi - lo), hi - 0.1 * (hi - lo), (4096, 3)).astype(np.float32)
        dirs = rng.normal(size=(4096, 3)); dirs = (dirs / np.linalg.norm(dirs, axis=1, keepdims=True)).astype(np.float32)
        tuv, ip = on.trace_rays(origins, dirs)
        want_tuv, want_ip = off.trace_rays(origins, dirs)
        assert on.flat_tree_state() == TREELESS and off.flat_tree_state()["treeless"] == 0
        assert _bits_equal(tuv, want_tuv) and np.array_equal(ip, want_ip)
        assert (ip[:, 0] >= 0).mean() > 0.9 and len(np.unique(ip[:, 0])) > 5
    finally:
        on.close(); off.close()


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# 5. the edits in place
# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
HIDDEN = 5


def _e_move(sc, start):
    t = _instances(sc.desc, MOVED); t[1] = t[1] @ _translate(0.3, 0.1, -0.2)
    sc.set_mesh_instance_transforms(MOVED, t)


def _e_deform(sc, start):
    sc.set_mesh_vertices(B, _deformed(start.meshes[B].vertices, 0.05, 19))


def _e_restore(sc, start):
    sc.set_mesh_vertices(B, np.array(start.meshes[B].vertices, copy=True))


def _e_hide(sc, start):
    sc.set_mesh_visibility(HIDDEN, False)


def _e_show(sc, start):
    sc.set_mesh_visibility(HIDDEN, True)


def _e_material(sc, start):
    m = copy.deepcopy(sc.desc.materials[DIFFUSE_MATERIAL]); m.params[0:3] = np.float32([0.9, 0.1, 0.4])
    sc.replace_material(DIFFUSE_MATERIAL, m)


def _e_move_and_material(sc, start):
    sc.set_mesh_transform(REASSIGNED, _transform(sc.desc, REASSIGNED) @ _translate(0.1, 0.1, -0.1))
    sc.set_mesh_material(REASSIGNED, DIFFUSE_MATERIAL)


# (name, edit, the counter of its own path -- None: update_counts()["material"] --, a mesh's points are not the build's afterwards, a material update runs)
EDITS = [("to-1-move-one-instance", _e_move, "tlas_update_count", False, False), ("to-2-deform", _e_deform, "blas_update_count", True, False),
         ("to-3-restore", _e_restore, "blas_update_count", False, False), ("to-4-hide", _e_hide, "tlas_visibility_update_count", False, False),
         ("to-5-show", _e_show, "tlas_visibility_update_count", False, False), ("to-6-material", _e_material, None, False, True),
         ("to-7-move-and-material", _e_move_and_material, "tlas_update_count", False, True)]


def _own_counters(sc):
    return {name: getattr(sc, name)() for name in ("tlas_update_count", "blas_update_count", "tlas_visibility_update_count")}


@pytest.mark.gpu
def test_edits_in_place_keep_the_scene_without_the_flat_tree(gi, orc):
    sc = _make(edits=True)
    start = copy.deepcopy(sc.desc)
    try:
        first = sc.render_aovs(RS, W, H, AOVS)
        _treeless_checks(sc, "to-edits-start")
        _check(orc, sc, "start", first)
        for key, edit, counter, deformed, with_material in EDITS:
            before, own_before = sc.update_counts(), _own_counters(sc)
            edit(sc, start)
            got = sc.render_aovs(RS, W, H, AOVS)
            after, own_after = sc.update_counts(), _own_counters(sc)
            print(f"{key}: counts {after} own {own_after} bvhBuildMs {sc.stats()['bvhBuildMs']:.3f} uploadMs {sc.stats()['uploadMs']:.3f}")
            assert after["full"] == 1 and after["transform"] == 0, (key, after)
            assert after["material"] == before["material"] + int(with_material), (key, after)
            for name in own_after:  # the path's own counter advanced, no other did
                assert own_after[name] == own_before[name] + int(name == counter), (key, name, own_before, own_after)
            assert sc.visibility_update_count() == 0 and sc.vertex_update_count() == 0, key
            _treeless_checks(sc, key, deformed=deformed)
            _check(orc, sc, key, got)
    finally:
        sc.close()


@pytest.mark.gpu
def test_with_the_edit_options_off_the_same_edits_rebuild_without_the_flat_tree(gi, orc):
    """Every geometry-side step is a full build, and every build is one without the flat tree again.  The material replacement has no option: it stays the
    material update it is on every layout (step 6), and in step 7 it runs in front of the move, which then rebuilds."""
    sc = _make()
    start = copy.deepcopy(sc.desc)
    try:
        sc.render_aovs(RS, W, H, AOVS)
        _treeless_checks(sc, "to-rebuilds-start")
        for key, edit, counter, deformed, with_material in EDITS:
            before = sc.update_counts()
            edit(sc, start)
            got = sc.render_aovs(RS, W, H, AOVS)
            after, st = sc.update_counts(), sc.stats()
            geometry = counter is not None
            assert after["full"] == before["full"] + int(geometry) and after["transform"] == 0, (key, before, after)
            assert after["material"] == before["material"] + int(with_material), (key, before, after)
            assert _own_counters(sc) == {"tlas_update_count": 0, "blas_update_count": 0, "tlas_visibility_update_count": 0}, key
            assert (st["bvhBuildMs"] > 0.0) == geometry, (key, st)
            assert sc.flat_tree_state() == TREELESS and st["nodeCount"] == 0 and st["triangleCount"] == sc.desc.triangle_count(), (key, sc.flat_tree_state(), st)
            assert sc.tlas_check() == 0 and sc.flat_id_check() == 0, key  # (a rebuilt BLAS is a fresh build's whatever the points are)
            _check(orc, sc, key, got)
    finally:
        sc.close()


@pytest.mark.gpu
def test_hide_then_move_then_show_of_a_far_instance(gi, orc):
    """The bounds of a scene without the flat tree are the VISIBLE instances' boxes, made again behind every edit in place: a far instance is hidden, another
    edit in place makes the bounds anew without it, and the show makes them again with it.  No render reads the bounds of a two-level scene today (the
    bounds retire of k_raygen is not applied on this layout), so an image cannot show a stale box: tests/cpp/tlas_bounds_sanitize.cpp holds the function, and
    this case holds the sequence's images, counters and resident state -- seen from outside the room, where the far instance has nothing behind it."""
    d = _lookdev_scene()
    t = _instances(d, HIDDEN); t[0] = _scale(5.0, 5.0, 5.0) @ t[0] @ _translate(0.0, 0.0, 6.0)  # five times its size, high above the room where nothing else is
    d.meshes[HIDDEN].instance_transforms = t
    d.camera = _look_at_camera((0.0, -10.0, 6.0), (-0.7, 0.7, 5.5), (0, 0, 1), 60.0)  # from outside: the room below, the far instance above it
    far_id = d.meshes[HIDDEN].id
    sc = _make(edits=True, desc=d)
    try:
        first = sc.render_aovs(RS, W, H, AOVS)
        assert (first["objectId"] == far_id).sum() >= 4, "the camera sees the far instance"
        steps = [("to-far-hide", lambda: sc.set_mesh_visibility(HIDDEN, False), False),
                 ("to-far-hidden-move", lambda: _e_move(sc, None), False),
                 ("to-far-show", lambda: sc.set_mesh_visibility(HIDDEN, True), True)]
        for key, edit, seen in steps:
            edit()
            got = sc.render_aovs(RS, W, H, AOVS)
            assert sc.update_counts()["full"] == 1, (key, sc.update_counts())
            assert bool((got["objectId"] == far_id).any()) == seen, key
            _treeless_checks(sc, key)
            _check(orc, sc, key, got)
        assert _own_counters(sc) == {"tlas_update_count": 1, "blas_update_count": 0, "tlas_visibility_update_count": 2}
    finally:
        sc.close()


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# 6. declines to the flat build
# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_scene_with_an_inactive_triangle_keeps_the_flat_tree(gi, orc):
    d = _lookdev_scene()
    v = np.array(d.meshes[MOVED].vertices, copy=True); v["pos"][7, 1] = np.nan  # one non-finite vertex: the faces that use it are inactive
    d.meshes[MOVED].vertices = v
    on, off = _make(desc=copy.deepcopy(d)), _make(tlas_only=False, desc=copy.deepcopy(d))
    try:
        got, ref = on.render_aovs(RS, W, H, AOVS), off.render_aovs(RS, W, H, AOVS)
        state = on.flat_tree_state()
        assert state["treeless"] == 0 and state["resident_nodes"] > 0 and state == off.flat_tree_state(), (state, off.flat_tree_state())
        assert on.stats()["inactiveTriangleCount"] == off.stats()["inactiveTriangleCount"] > 0 and on.stats()["nodeCount"] == off.stats()["nodeCount"] > 0
        assert on.validate_bvh()["digest"] == off.validate_bvh()["digest"] and on.validate_bvh()["violations"] == 0
        _same_aovs(got, ref, "to-inactive", "the scene with the option off")
        clean = sanitised(d)
        img, _ = orc.render(clean, RS, W, H, threads=8)
        want = orc.render_aovs(clean, RS, W, H, AOVS)
        assert _bits_equal(got["color"], img), "to-inactive: colour differs from the oracle"
        _same_aovs({k: got[k] for k in AOVS}, want, "to-inactive", "the oracle")
    finally:
        on.close(); off.close()


@pytest.mark.gpu
def test_scene_that_fits_lds_keeps_the_flat_tree(gi, orc):
    d = cornell_box(MAT_DIFFUSE)
    assert d.triangle_count() <= 128
    rs = RenderSettings(spp=2, max_bounces=3, progressive_accumulation=False)
    on, off = _make(desc=copy.deepcopy(d)), _make(tlas_only=False, desc=copy.deepcopy(d))
    try:
        got, ref = on.render_aovs(rs, W, H, AOVS), off.render_aovs(rs, W, H, AOVS)
        state = on.flat_tree_state()
        assert state["treeless"] == 0 and state["two_level"] == 0 and state["resident_nodes"] > 0 and state == off.flat_tree_state(), (state, off.flat_tree_state())
        assert on.validate_bvh()["digest"] == off.validate_bvh()["digest"]
        _same_aovs(got, ref, "to-lds", "the scene with the option off")
        img, _ = orc.render(d, rs, W, H, threads=8)
        assert _bits_equal(got["color"], img), "to-lds: colour differs from the oracle"
        _same_aovs({k: got[k] for k in AOVS}, orc.render_aovs(d, rs, W, H, AOVS), "to-lds", "the oracle")
    finally:
        on.close(); off.close()


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# 7. two device contexts
# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
TWO_CONTEXTS = textwrap.dedent("""
    import copy, sys
    sys.path.insert(0, %(root)r)
    sys.path.insert(0, %(tests)r)
    from gatling_amd import capi
    import test_tlas_only as T
    L = capi.initialize(0)                      # $GATLING_DEVICES = "0,0": two contexts on the one GPU
    assert L.giCGetDeviceCount() == 2
    multi = T._make(edits=True)
    single = T._make(edits=True); single.set_option(capi.OPTION_DEVICES, 1)
    start = copy.deepcopy(multi.desc)
    for sc in (multi, single):
        sc.render_aovs(T.RS, T.W, T.H, T.AOVS)
    T._treeless_checks(multi, "start", devices=(0, 1))
    for key, edit, counter, deformed, with_material in T.EDITS:
        out = []
        for sc in (multi, single):
            edit(sc, start)
            out.append(sc.render_aovs(T.RS, T.W, T.H, T.AOVS))
        for k in out[0]:
            assert T._bits_equal(out[0][k], out[1][k]), key + ": " + k + " differs between two device contexts and one"
        T._treeless_checks(multi, key, devices=(0, 1), deformed=deformed)
        T._treeless_checks(single, key, deformed=deformed)
    assert multi.update_counts() == single.update_counts() == {"full": 1, "transform": 0, "material": 2}
    assert T._own_counters(multi) == T._own_counters(single) == {"tlas_update_count": 2, "blas_update_count": 2, "tlas_visibility_update_count": 2}
    fresh = capi.Scene(copy.deepcopy(multi.desc)); fresh.set_option(capi.OPTION_DEVICES, 1)
    ref = fresh.render_aovs(T.RS, T.W, T.H, T.AOVS)
    for k in ref:
        assert T._bits_equal(out[0][k], ref[k]), k + " differs from a scene built from scratch"
    multi.close(); single.close(); fresh.close()
    print("two contexts ok")
""")


@pytest.mark.gpu
def test_scene_without_the_flat_tree_on_two_device_contexts():
    env = dict(os.environ); env["GATLING_DEVICES"] = "0,0"
    out = subprocess.run([sys.executable, "-c", TWO_CONTEXTS % {"root": ROOT, "tests": os.path.join(ROOT, "tests")}], capture_output=True, text=True, timeout=300,
                         env=env)
    assert out.returncode == 0 and "two contexts ok" in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# 8. random edit sequences
# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("seq", range(8))
def test_random_edit_sequences_match_a_fresh_build_and_the_oracle(gi, orc, seq):
    """The draw of tests/test_tlas_visibility_edits.py's random case -- toggles of random clutter meshes, sometimes with a material or a transform edit of another
    mesh in the same render -- with the option and options 11, 16 and 18 on: five edits, every frame against a scene built from scratch and the oracle.  Moves
    of hidden meshes and hides below the floor are drawn too: they rebuild, and the rebuilt scene has no flat tree either."""
    rs = RenderSettings(spp=1, max_bounces=3, next_event_estimation=True, progressive_accumulation=False)
    rng = np.random.default_rng(19000 + seq)
    sc = _make()
    for name in ("OPTION_VISIBILITY_UPDATES", "OPTION_TLAS_UPDATES", "OPTION_TLAS_VISIBILITY"):
        sc.set_option(getattr(capi, name), 1)
    try:
        sc.render(rs, W, H)
        for k in range(5):
            kind = _random_edit(rng, sc)
            got = sc.render_aovs(rs, W, H, AOVS)
            key = (seq, k, kind, [m.visible for m in sc.desc.meshes])
            fresh = capi.Scene(copy.deepcopy(sc.desc))
            try:
                ref = fresh.render_aovs(rs, W, H, AOVS)
            finally:
                fresh.close()
            _same_aovs(got, ref, key, "a scene built from scratch")
            img, _ = orc.render(sc.desc, rs, W, H, threads=8)
            assert _bits_equal(got["color"], img), (key, "colour differs from the oracle")
            _same_aovs({a: got[a] for a in AOVS}, orc.render_aovs(sc.desc, rs, W, H, AOVS), key, "the oracle")
            state, st = sc.flat_tree_state(), sc.stats()
            assert state == TREELESS and st["nodeCount"] == 0, (key, state, st)
            c, f = sc.tlas_check(), sc.flat_id_check()
            assert c == 0 and c.two_level == 1 and f == 0 and f.resident_tris == st["triangleCount"], (key, int(c), int(f), f.resident_tris, st["triangleCount"])
            assert f.visible_tris == sum(len(m.faces) * len(m.instance_transforms) for m in sc.desc.meshes if m.visible), key
        assert sc.update_counts()["transform"] == 0 and sc.visibility_update_count() == 0
        print("random sequence", seq, sc.update_counts(), _own_counters(sc))
    finally:
        sc.close()

"""Incremental material updates (gi_build.cpp updateMaterials, gi_patch.hip k_patch_mat_flags): after an edit of a material, a material
assignment, a texture binding or a primvar the next render rebuilds the material / texture / scene-data tables and patches one word per flattened triangle in
device memory instead of rebuilding the scene.  The image and the AOVs must be bit-identical to a scene built from scratch from the edited description, and to
the oracle's render of it; the class masks and the cutout flag (gi_build.cpp deriveSceneClasses; Scene.class_state), which pick a render's kernel variants and
cannot be seen in an image, must equal those of the scene built from scratch.

CPU: which dirty flags every entry point raises before and after the first build (giCDebugEditDirtyFlags).
GPU: an edit sequence on every layout (host-built, device-built, partitioned, two-level), the fallbacks, the look-ahead window, two device contexts, random
edit sequences against the oracle, and the cost of an edit on config C5's interior.

`bvhBuildMs == 0.0` after an edit is the sign of the incremental material path, and giCDebugSceneUpdateCounts must not count a full build.  One step of the
sequence, (g), makes a material edit AND a transform edit before the same render: the transform path reports the subtrees it rebuilt in bvhBuildMs (as it
always has, tests/test_incremental.py), so that step asserts through the counters that both incremental paths ran and no full build did; on the two-level
layout, which the transform path does not cover, it asserts the rebuild."""
import copy
import os
import re
import subprocess
import sys
import textwrap
import time

import numpy as np
import pytest

from gatling_amd import capi
from gatling_amd.scene import (INTERP_CONSTANT, INTERP_VERTEX, MAT_DIFFUSE, MAT_OPEN_PBR, MAT_USD_PREVIEW_SURFACE, PRIMVAR_VEC3, TEX_BASE_COLOR, TEX_ROUGHNESS,
                               MaterialDesc, Primvar, RenderSettings, TextureBinding)
from gatling_amd.scenes import cornell_box, interior_scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIRTY_BVH, DIRTY_FRAMEBUFFER, DIRTY_LIGHTS, DIRTY_MATERIALS, DIRTY_XFORM = 1, 2, 4, 8, 16
AOVS = ["albedo", "opacity", "thinWalled", "doubleSided", "normal", "objectId", "instanceId", "faceId", "depth"]


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# CPU: host logic
# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
MATERIAL_SIDE = {0: "giCCreateMaterial", 1: "giCDestroyMaterial", 2: "giCSetMeshMaterial", 3: "giCSetMaterialPrimvarInput", 4: "giCSetMaterialTexture",
                 5: "giCSetMaterialTextureTransform", 6: "giCCreateTexture", 7: "giCDestroyTexture", 8: "giCSetMeshPrimvars", 9: "giCSetMeshInstancerPrimvars"}
GEOMETRY_SIDE = {11: "giCSetMeshVisibility", 12: "giCSetMeshInstanceIds", 13: "giCCreateMesh", 14: "giCDestroyMesh", 15: "giCSetMeshInstanceTransforms (count)"}


@pytest.mark.parametrize("edit", sorted(MATERIAL_SIDE))
def test_material_side_edits_stop_raising_the_rebuild_flag_once_the_scene_is_built(edit):
    L = capi.load_library()
    before, after = L.giCDebugEditDirtyFlags(edit, 0), L.giCDebugEditDirtyFlags(edit, 1)
    assert after == DIRTY_MATERIALS | DIRTY_FRAMEBUFFER, (MATERIAL_SIDE[edit], after)
    # before the first build there is nothing to patch: the flags lead to the full build (giCCreateTexture never raised the rebuild flag by itself)
    assert before & DIRTY_FRAMEBUFFER and before & (DIRTY_BVH | DIRTY_MATERIALS), (MATERIAL_SIDE[edit], before)
    if edit != 6:
        assert before & DIRTY_BVH, (MATERIAL_SIDE[edit], before)


@pytest.mark.parametrize("edit", sorted(GEOMETRY_SIDE))
def test_geometry_side_edits_keep_the_rebuild_flag(edit):
    L = capi.load_library()
    for built in (0, 1):
        assert L.giCDebugEditDirtyFlags(edit, built) == DIRTY_BVH | DIRTY_FRAMEBUFFER, (GEOMETRY_SIDE[edit], built)


def test_transform_edit_flags_are_unchanged():
    L = capi.load_library()
    assert L.giCDebugEditDirtyFlags(10, 0) == DIRTY_BVH | DIRTY_FRAMEBUFFER and L.giCDebugEditDirtyFlags(10, 1) == DIRTY_XFORM | DIRTY_FRAMEBUFFER
    assert L.giCDebugEditDirtyFlags(99, 1) < 0


def test_header_keeps_api_version_8_and_declares_the_debug_queries():
    text = open(os.path.join(ROOT, "include", "gi_c.h")).read()
    assert re.search(r"#define\s+GI_C_API_VERSION\s+8u?\b", text)
    assert "giCDebugEditDirtyFlags" in text and "giCDebugSceneUpdateCounts" in text
    assert capi.load_library().giCGetApiVersion() == 8
    for name in ("set_mesh_material", "replace_material", "set_material_primvar_input", "set_mesh_primvars", "set_material_texture", "add_texture"):
        assert callable(getattr(capi.Scene, name))


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# the look-development scene and its edits
# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
def _image(seed, h=8, w=8):
    rng = np.random.default_rng(seed)
    a = np.ones((h, w, 4), np.float32); a[..., :3] = rng.uniform(0.05, 0.95, (h, w, 3))
    return a


def _lookdev_scene(**kw):
    """The small interior (>= 4096 flattened triangles, instanced clutter) with a textured, a primvar-driven, a cutout, a diffuse and an OpenPBR BASE material
    bound to clutter meshes.  Materials 0..8 are the interior's; 9 textured, 10 primvar-driven, 11 cutout, 12 diffuse, 13 OpenPBR BASE."""
    args = dict(clutter_instances=60, subdivisions=3, prototypes=5, material_count=8)
    args.update(kw)
    d = interior_scene(**args)
    n0 = len(d.materials)
    d.textures = [_image(1), _image(2, 4, 16)]
    tex = MaterialDesc.usd_preview_surface(name="textured", diffuseColor=(0.5, 0.5, 0.5), roughness=0.4)
    tex.textures = {TEX_BASE_COLOR: TextureBinding(texture=0)}
    pv = MaterialDesc.open_pbr(name="primvar", base_color=(0.4, 0.4, 0.4), specular_roughness=0.5)
    pv.primvar_inputs = {TEX_BASE_COLOR: "tint"}
    cut = MaterialDesc.usd_preview_surface(name="cutout", diffuseColor=(0.8, 0.3, 0.2), roughness=0.6, opacity=0.5)
    dif = MaterialDesc.usd_preview_surface(name="diffuse", diffuseColor=(0.3, 0.6, 0.8), klass=MAT_DIFFUSE)
    base = MaterialDesc.open_pbr(name="base", base_color=(0.7, 0.6, 0.2), specular_roughness=0.35)
    d.materials += [tex, pv, cut, dif, base]
    clutter = [i for i, m in enumerate(d.meshes) if m.name.startswith("/Clutter")]
    assert len(clutter) >= 5
    for k, mi in enumerate(clutter[:5]):
        d.meshes[mi].material = n0 + k
    d.meshes[clutter[1]].primvars = [Primvar("tint", PRIMVAR_VEC3, INTERP_CONSTANT, np.float32([0.9, 0.2, 0.3]))]
    return d


def _instanced(desc):
    """The most-instanced clutter mesh that is not one of the five bound to the special materials."""
    clutter = [i for i, m in enumerate(desc.meshes) if m.name.startswith("/Clutter")][5:]
    return max(clutter, key=lambda i: len(desc.meshes[i].instance_transforms))


def _translate(x, y, z):
    m = np.eye(4, dtype=np.float32); m[3, :3] = (x, y, z)
    return m


def _e_reassign(sc):       # (a) another existing material of a different shade class; the mesh is instanced
    mi = _instanced(sc.desc)
    assert len(sc.desc.meshes[mi].instance_transforms) > 1
    assert capi.shade_class(sc.desc.materials[sc.desc.meshes[mi].material]) != 0
    sc.set_mesh_material(mi, 12)


def _e_colour(sc):         # (b) destroy + create + assign, same class
    m = copy.deepcopy(sc.desc.materials[3]); m.params[0:3] = (0.05, 0.9, 0.35); m.params[11] = 0.77
    sc.replace_material(3, m)


def _e_class_up(sc):       # (c) OpenPBR BASE -> OpenPBR with every lobe
    assert capi.shade_class(sc.desc.materials[13]) == 3
    m = MaterialDesc.open_pbr(name="base", base_color=(0.7, 0.6, 0.2), specular_roughness=0.35, coat_weight=1.0, coat_roughness=0.1)
    assert capi.shade_class(m) == 2
    sc.replace_material(13, m)


def _e_class_down(sc):     # (c) UsdPreviewSurface / OpenPBR -> diffuse
    sc.replace_material(0, MaterialDesc.usd_preview_surface(name="walls", diffuseColor=(0.6, 0.65, 0.7), klass=MAT_DIFFUSE))


def _e_cutout_off(sc):     # (d) hasCutouts true -> false
    sc.replace_material(11, MaterialDesc.usd_preview_surface(name="cutout", diffuseColor=(0.8, 0.3, 0.2), roughness=0.6, opacity=1.0))


def _e_cutout_on(sc):      # (d) ... -> true
    sc.replace_material(11, MaterialDesc.open_pbr(name="cutout", base_color=(0.8, 0.3, 0.2), geometry_opacity=0.4))


def _e_unbind(sc):         # (e) the only texture binding goes
    sc.set_material_texture(9, TEX_BASE_COLOR, None)


def _e_new_texture(sc):    # (e) a new image, bound to two inputs
    t = sc.add_texture(_image(3, 16, 4))
    sc.set_material_texture(9, TEX_BASE_COLOR, TextureBinding(texture=t, scale=(0.9, 0.8, 0.7, 1.0), bias=(0.05, 0.0, 0.1, 0.0)))
    sc.set_material_texture(9, TEX_ROUGHNESS, TextureBinding(texture=1, channel=1))


def _e_primvar(sc):        # (f) the input reads another name; the mesh's primvar data changes
    clutter = [i for i, m in enumerate(sc.desc.meshes) if m.material == 10]
    sc.set_material_primvar_input(10, TEX_BASE_COLOR, "shade")
    nv = len(sc.desc.meshes[clutter[0]].vertices)
    ramp = np.stack([np.linspace(0.1, 0.9, nv), np.linspace(0.8, 0.2, nv), np.full(nv, 0.5)], axis=1).astype(np.float32)
    sc.set_mesh_primvars(clutter[0], [Primvar("tint", PRIMVAR_VEC3, INTERP_CONSTANT, np.float32([0.1, 0.1, 0.9])), Primvar("shade", PRIMVAR_VEC3, INTERP_VERTEX, ramp)])


def _e_both(sc):           # (g) a material edit and a transform edit before the same render
    m = copy.deepcopy(sc.desc.materials[5]); m.params[0:3] = (0.9, 0.1, 0.6)
    sc.replace_material(5, m)
    mi = _instanced(sc.desc)
    it = np.asarray(sc.desc.meshes[mi].instance_transforms, np.float32).reshape(-1, 4, 4).copy()
    it[0] = it[0] @ _translate(0.2, -0.1, 0.1)
    sc.set_mesh_instance_transforms(mi, it)


SEQUENCE = [("a-reassign", _e_reassign), ("b-colour", _e_colour), ("c-base-to-full", _e_class_up), ("c-to-diffuse", _e_class_down), ("d-cutout-off", _e_cutout_off),
            ("d-cutout-on", _e_cutout_on), ("e-unbind", _e_unbind), ("e-new-texture", _e_new_texture), ("f-primvar", _e_primvar), ("g-material-and-transform", _e_both)]
RS = RenderSettings(spp=2, max_bounces=4, next_event_estimation=True, progressive_accumulation=False)
W, H = 64, 36
_oracle_cache = {}


def _bits_equal(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def _oracle(orc, step, desc):
    """The oracle's image and AOVs of the description after `step` (the same for every layout: rendered once)."""
    if step not in _oracle_cache:
        img, _ = orc.render(desc, RS, W, H, threads=8)
        _oracle_cache[step] = (img, orc.render_aovs(desc, RS, W, H, AOVS))
    return _oracle_cache[step]


def _check(orc, sc, step, got):
    fresh = capi.Scene(copy.deepcopy(sc.desc))
    try:
        ref = fresh.render_aovs(RS, W, H, AOVS)
        fresh_classes = fresh.class_state()
    finally:
        fresh.close()
    assert sc.class_state() == fresh_classes, f"{step}: class state {sc.class_state()} differs from a scene built from scratch, {fresh_classes}"
    oimg, oaov = _oracle(orc, step, sc.desc)
    for k in ["color"] + AOVS:
        assert _bits_equal(got[k], ref[k]), f"{step}: {k} differs from a scene built from scratch"
        assert _bits_equal(got[k], oimg if k == "color" else oaov[k]), f"{step}: {k} differs from the oracle"


def _run_sequence(orc, layout, incremental=True):
    sc = capi.Scene(_lookdev_scene())
    assert sc.desc.triangle_count() >= 4096
    try:
        if layout == "device":
            sc.set_option(capi.OPTION_BVH_BUILD, 1)
        if layout == "two_level":
            sc.set_option(capi.OPTION_TWO_LEVEL, 1)
        got = sc.render_aovs(RS, W, H, AOVS)
        assert sc.stats()["bvhBuildMs"] > 0.0
        if layout == "device":
            assert sc.validate_bvh()["device_built"]
        _check(orc, sc, "start", got)
        if layout == "partitioned":  # a transform edit (and its reverse: the description is the start's again) re-lays the tree out as per-instance subtrees
            mi = _instanced(sc.desc)
            t0 = np.asarray(sc.desc.meshes[mi].transform, np.float32).reshape(4, 4).copy()
            sc.set_mesh_transform(mi, t0 @ _translate(0.1, 0.0, 0.05)); sc.render(RS, W, H)
            sc.set_mesh_transform(mi, t0); sc.render(RS, W, H)
            assert sc.update_counts() == {"full": 1, "transform": 2, "material": 0}
        for step, edit in SEQUENCE:
            before = sc.update_counts()
            edit(sc)
            got = sc.render_aovs(RS, W, H, AOVS)
            st, after = sc.stats(), sc.update_counts()
            print(f"{layout} {step}: bvhBuildMs {st['bvhBuildMs']:.3f} uploadMs {st['uploadMs']:.3f} counts {after}")
            both = step.startswith("g-")
            if not incremental:
                assert st["bvhBuildMs"] > 0.0 and after["full"] == before["full"] + 1 and after["material"] == before["material"], (layout, step, st, after)
            elif both and layout == "two_level":  # the transform path does not cover the two-level layout: that half of the edit rebuilds
                assert st["bvhBuildMs"] > 0.0 and after["full"] == before["full"] + 1, (layout, step, after)
            elif both:
                assert after == {"full": before["full"], "transform": before["transform"] + 1, "material": before["material"] + 1}, (layout, step, after)
            else:
                assert st["bvhBuildMs"] == 0.0, (layout, step, st["bvhBuildMs"])
                assert after == {"full": before["full"], "transform": before["transform"], "material": before["material"] + 1}, (layout, step, after)
            _check(orc, sc, step, got)
    finally:
        sc.close()


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["host", "device", "partitioned", "two_level"])
def test_material_edits_update_incrementally_and_bit_exactly(gi, orc, layout):
    _run_sequence(orc, layout)


@pytest.mark.gpu
def test_with_incremental_switched_off_the_same_edits_rebuild_and_give_the_same_bits(gi, orc, monkeypatch):
    monkeypatch.setenv("GATLING_OPTIONS", "incremental=0")
    _run_sequence(orc, "host", incremental=False)


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# fallbacks
# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_scene_below_the_triangle_floor_rebuilds(gi, orc):
    rs = RenderSettings(spp=2, max_bounces=4, progressive_accumulation=False)
    sc = capi.Scene(cornell_box())
    try:
        assert sc.desc.triangle_count() < 4096
        sc.render(rs, 48, 48)
        m = copy.deepcopy(sc.desc.materials[0]); m.params[0:3] = (0.2, 0.7, 0.9)
        sc.replace_material(0, m)
        img = sc.render(rs, 48, 48)
        assert sc.stats()["bvhBuildMs"] > 0.0 and sc.update_counts() == {"full": 2, "transform": 0, "material": 0}
        ref, _ = orc.render(sc.desc, rs, 48, 48, threads=8)
        assert _bits_equal(img, ref)
    finally:
        sc.close()


def _fresh_image(desc, rs, w, h):
    fresh = capi.Scene(copy.deepcopy(desc))
    try:
        return fresh.render(rs, w, h)
    finally:
        fresh.close()


@pytest.mark.gpu
@pytest.mark.parametrize("how", ["null", "destroyed"])
def test_mesh_without_a_valid_material_drops_out_and_comes_back(gi, how):
    sc = capi.Scene(_lookdev_scene())
    try:
        base = sc.render(RS, W, H)
        mi = _instanced(sc.desc)
        was = sc.desc.meshes[mi].material
        bound = [i for i, m in enumerate(sc.desc.meshes) if m.material == was]
        if how == "null":
            sc.set_mesh_material(mi, -1)
        else:  # every mesh bound to the material loses it
            sc.destroy_material(was)
            for i in bound:
                sc.desc.meshes[i].material = -1
        gone = sc.render(RS, W, H)
        assert sc.stats()["bvhBuildMs"] > 0.0 and sc.update_counts() == {"full": 2, "transform": 0, "material": 0}
        assert sc.stats()["triangleCount"] == sc.desc.triangle_count() - sum(len(sc.desc.meshes[i].faces) * len(sc.desc.meshes[i].instance_transforms)
                                                                               for i in (bound if how == "destroyed" else [mi]))
        assert not _bits_equal(gone, base)
        assert _bits_equal(gone, _fresh_image(sc.desc, RS, W, H)), "scene without the mesh differs from a fresh build"
        for i in (bound if how == "destroyed" else [mi]):
            sc.set_mesh_material(i, 4 if was != 4 else 5)
        back = sc.render(RS, W, H)
        assert sc.stats()["bvhBuildMs"] > 0.0 and sc.update_counts()["full"] == 3
        assert _bits_equal(back, _fresh_image(sc.desc, RS, W, H)), "scene with the mesh back differs from a fresh build"
        # ... and from here on the mesh is part of the scene again: the next assignment is incremental
        sc.set_mesh_material(mi, 12)
        last = sc.render(RS, W, H)
        assert sc.stats()["bvhBuildMs"] == 0.0 and sc.update_counts() == {"full": 3, "transform": 0, "material": 1}
        assert _bits_equal(last, _fresh_image(sc.desc, RS, W, H))
    finally:
        sc.close()


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# look-ahead, two device contexts
# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_material_edit_discards_the_look_ahead_window(gi, orc):
    rs = RenderSettings(spp=1, max_bounces=5, next_event_estimation=True)  # progressive
    w, h = 48, 27
    sc = capi.Scene(_lookdev_scene())
    try:
        sc.set_option(capi.OPTION_SAMPLE_LOOKAHEAD, 16)
        for _ in range(9):  # windows of 1, 2, 4; the eighth call traces a window of 8, the ninth is served from it
            sc.render(rs, w, h)
        la = sc.lookahead_stats()
        assert (la["windowCalls"], la["windowServed"], la["traced"]) == (8, 2, 0) and la["windowsDiscarded"] == 0
        m = copy.deepcopy(sc.desc.materials[2]); m.params[0:3] = (0.95, 0.05, 0.05)
        sc.replace_material(2, m)
        img = sc.render(rs, w, h)
        la2 = sc.lookahead_stats()
        assert la2["windowsDiscarded"] == 1 and la2["samplesUnused"] == 6 and la2["traced"] == 1, la2
        assert sc.stats()["bvhBuildMs"] == 0.0 and sc.update_counts() == {"full": 1, "transform": 0, "material": 1}
        ref, _ = orc.render(sc.desc, rs, w, h, threads=8)  # the accumulation restarted: the oracle's first frame of the edited scene
        assert _bits_equal(img, ref)
    finally:
        sc.close()


TWO_CONTEXTS = textwrap.dedent("""
    import copy, sys, numpy as np
    sys.path.insert(0, %(root)r)
    sys.path.insert(0, %(tests)r)
    from gatling_amd import capi
    import test_material_edits as T
    L = capi.initialize(0)                      # $GATLING_DEVICES = "0,0": two contexts on the one GPU
    assert L.giCGetDeviceCount() == 2
    multi = capi.Scene(T._lookdev_scene())
    single = capi.Scene(T._lookdev_scene()); single.set_option(capi.OPTION_DEVICES, 1)
    for sc in (multi, single):
        sc.render_aovs(T.RS, T.W, T.H, T.AOVS)
    for step, edit in T.SEQUENCE[:9]:
        out = []
        for sc in (multi, single):
            edit(sc)
            out.append(sc.render_aovs(T.RS, T.W, T.H, T.AOVS))
            assert sc.stats()["bvhBuildMs"] == 0.0, (step, sc.stats()["bvhBuildMs"])
        for k in out[0]:
            assert T._bits_equal(out[0][k], out[1][k]), step + ": " + k + " differs between two device contexts and one"
    assert multi.update_counts() == {"full": 1, "transform": 0, "material": 9}
    fresh = capi.Scene(copy.deepcopy(multi.desc)); fresh.set_option(capi.OPTION_DEVICES, 1)
    ref = fresh.render_aovs(T.RS, T.W, T.H, T.AOVS)
    for k in ref:
        assert T._bits_equal(out[0][k], ref[k]), k + " differs from a scene built from scratch"
    multi.close(); single.close(); fresh.close()
    print("two contexts ok")
""")


@pytest.mark.gpu
def test_material_edits_reach_every_device_context():
    env = dict(os.environ); env["GATLING_DEVICES"] = "0,0"
    out = subprocess.run([sys.executable, "-c", TWO_CONTEXTS % {"root": ROOT, "tests": os.path.join(ROOT, "tests")}], capture_output=True, text=True, timeout=600,
                         env=env)
    assert out.returncode == 0 and "two contexts ok" in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# random sequences
# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
def _random_edit(rng, sc):
    d = sc.desc
    kind = int(rng.integers(9))
    meshes = [i for i, m in enumerate(d.meshes) if m.name.startswith("/Clutter")]
    mi = int(rng.choice(meshes))
    mat = int(rng.integers(len(d.materials)))
    if kind == 0:
        sc.set_mesh_material(mi, mat); return "assign"
    if kind == 1:
        m = copy.deepcopy(d.materials[mat]); m.params[0:3] = rng.uniform(0.05, 0.95, 3).astype(np.float32)
        sc.replace_material(mat, m); return "colour"
    if kind == 2:
        colour = tuple(float(x) for x in rng.uniform(0.05, 0.95, 3))
        choice = int(rng.integers(4))
        m = [MaterialDesc.usd_preview_surface(name="r", diffuseColor=colour, klass=MAT_DIFFUSE), MaterialDesc.usd_preview_surface(name="r", diffuseColor=colour, roughness=0.4),
             MaterialDesc.open_pbr(name="r", base_color=colour), MaterialDesc.open_pbr(name="r", base_color=colour, coat_weight=1.0)][choice]
        sc.replace_material(mat, m); return "class"
    if kind == 3:
        m = copy.deepcopy(d.materials[mat]); m.params[14] = 0.5 if m.params[14] >= 1.0 else 1.0  # P_OPACITY
        sc.replace_material(mat, m); return "cutout"
    if kind == 4:
        if d.materials[mat].textures:
            sc.set_material_texture(mat, next(iter(d.materials[mat].textures)), None); return "unbind"
        t = sc.add_texture(_image(int(rng.integers(1 << 30)), 4, 4)) if rng.uniform() < 0.5 else int(rng.integers(len(d.textures)))
        sc.set_material_texture(mat, TEX_BASE_COLOR, TextureBinding(texture=t)); return "bind"
    if kind == 5:
        sc.set_material_primvar_input(mat, TEX_BASE_COLOR, None if d.materials[mat].primvar_inputs else "tint")
        sc.set_mesh_primvars(mi, [Primvar("tint", PRIMVAR_VEC3, INTERP_CONSTANT, rng.uniform(0.05, 0.95, 3).astype(np.float32))]); return "primvar"
    if kind == 6:
        t = np.asarray(d.meshes[mi].transform, np.float32).reshape(4, 4) @ _translate(*rng.uniform(-0.2, 0.2, 3))
        sc.set_mesh_transform(mi, t); return "transform"
    if kind == 7:
        sc.set_mesh_visibility(mi, not d.meshes[mi].visible); return "visibility"
    a, b = rng.choice(meshes, 2, replace=False)  # two edits before one render: an assignment and a transform or a visibility toggle
    sc.set_mesh_material(int(a), mat)
    if rng.uniform() < 0.5:
        sc.set_mesh_visibility(int(b), not d.meshes[int(b)].visible); return "assign+visibility"
    sc.set_mesh_transform(int(b), np.asarray(d.meshes[int(b)].transform, np.float32).reshape(4, 4) @ _translate(0.1, 0.1, 0.0)); return "assign+transform"


@pytest.mark.gpu
def test_random_edit_sequences_match_the_oracle(gi, orc):
    """200 sequences of four random edits each -- material-side edits, transforms and visibility toggles (a full rebuild) in random order -- on a scene of
    6 412 flattened triangles; every render is compared with the oracle's render of the description at that point.  Small image, one sample per pixel."""
    rs = RenderSettings(spp=1, max_bounces=3, next_event_estimation=True, progressive_accumulation=False)
    w, h = 24, 14
    rng = np.random.default_rng(20241)
    kinds, counts = {}, {"full": 0, "transform": 0, "material": 0}
    for seq in range(200):
        sc = capi.Scene(_lookdev_scene(clutter_instances=20, subdivisions=2, prototypes=3, material_count=4))
        try:
            sc.render(rs, w, h)
            for k in range(4):
                kind = _random_edit(rng, sc)
                kinds[kind] = kinds.get(kind, 0) + 1
                if sc.desc.triangle_count() < 4096:  # (too many meshes hidden: the floor's fallback, still compared)
                    kind += " (below the floor)"
                img = sc.render(rs, w, h)
                ref, _ = orc.render(sc.desc, rs, w, h, threads=8)
                assert _bits_equal(img, ref), (seq, k, kind)
            c = sc.update_counts()
            for name in counts:
                counts[name] += c[name]
        finally:
            sc.close()
    print("random edit sequences:", kinds, counts)
    assert counts["material"] > 0 and counts["transform"] > 0 and counts["full"] > 200  # every path was taken (each scene's first render is a full build)


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# cost
# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_material_edits_on_c5_cost_a_fraction_of_a_rebuild(gi):
    """Config C5's interior (10.24 M instanced triangles): the full build against (i) a colour-only replacement of one material and (ii) a re-assignment that
    changes one large mesh's shade class.  Measured on an MI355X: full build 2 235 + 919 ms; the replacement 19.7 ms (18.5 ms
    host, 1.15 ms device: 9.0 M triangles get a new word); the re-assignment 17.1 ms (16.9 host, 0.28 device)."""
    desc = interior_scene()
    rs = RenderSettings(spp=1, max_bounces=2, next_event_estimation=True, progressive_accumulation=False)
    w, h = 160, 90
    sc = capi.Scene(desc)
    try:
        sc.render(rs, w, h)
        full = sc.stats()
        full_ms = full["bvhBuildMs"] + full["uploadMs"]
        m = copy.deepcopy(desc.materials[7]); m.params[0:3] = (0.9, 0.15, 0.1)
        sc.replace_material(7, m)
        t0 = time.perf_counter(); sc.render(rs, w, h); call_i = (time.perf_counter() - t0) * 1e3
        colour = sc.stats()
        big = max(range(len(desc.meshes)), key=lambda i: len(desc.meshes[i].faces) * len(desc.meshes[i].instance_transforms))
        cls = capi.shade_class(desc.materials[desc.meshes[big].material])
        other = next(i for i, mm in enumerate(desc.materials) if not mm.textures and capi.shade_class(mm) != cls)
        sc.set_mesh_material(big, other)
        t0 = time.perf_counter(); img = sc.render(rs, w, h); call_ii = (time.perf_counter() - t0) * 1e3
        assign = sc.stats()
        print(f"C5 full build {full['bvhBuildMs']:.0f} + {full['uploadMs']:.0f} ms; colour-only replacement of one material {colour['uploadMs']:.2f} ms "
              f"(render call {call_i:.1f} ms); re-assignment of a {len(desc.meshes[big].faces) * len(desc.meshes[big].instance_transforms)}-triangle mesh to another "
              f"shade class {assign['uploadMs']:.2f} ms (render call {call_ii:.1f} ms)")
        assert colour["bvhBuildMs"] == 0.0 and assign["bvhBuildMs"] == 0.0 and sc.update_counts() == {"full": 1, "transform": 0, "material": 2}
        assert colour["uploadMs"] < 0.1 * full_ms
        assert assign["uploadMs"] < 0.1 * full_ms
        assert assign["triangleCount"] == full["triangleCount"] and assign["nodeCount"] == full["nodeCount"]
        fresh = capi.Scene(copy.deepcopy(sc.desc))
        try:
            ref = fresh.render(rs, w, h)
        finally:
            fresh.close()
        assert _bits_equal(img, ref)
    finally:
        sc.close()

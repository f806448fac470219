"""Incremental visibility updates (gi_build.cpp updateVisibility, gi_patch.hip k_patch_visibility): with GI_C_SCENE_OPTION_VISIBILITY_UPDATES
a giCSetMeshVisibility on a mesh of the built scene no longer rebuilds the scene.  The next render renumbers the scene-order ids of the triangles behind the
mesh, as a fresh build without it would number them, and makes the mesh's own triangles unhittable (flat layouts) or leaves its parts out of the top tree
(partitioned layout).  The image and the AOVs must be bit-identical to a scene built from scratch from the description with `visible` flipped, and to the
oracle's render of it.  No tolerance anywhere.

The class masks and the cutout flag (gi_build.cpp deriveSceneClasses; Scene.class_state) pick a render's kernel variants and cannot be seen in an image: after
every step they must equal those of the scene built from scratch.

CPU: the header and the harness declare the option, the counter and the class-state query; the API version is unchanged.
GPU: an edit sequence on every layout (host-built, device-built, partitioned, two-level), the same sequence with the option off, the fallbacks, the cutout
flag, a material assigned to a hidden mesh, the look-ahead window, two device contexts, random edit sequences against the oracle.

The scene is the look-development interior of tests/test_material_edits.py at its small size (6 412 flattened triangles: above the 4 096 floor of the
incremental paths and beyond LDS).  Scene order there: mesh 1 (two instances, 640 triangles) lies in front of mesh 3, the only mesh bound to the cutout
material -- hiding mesh 1 shifts the ids the cutout test hashes, so a hide that does not renumber changes pixels.

Two places where the sequence asserts through the counters instead of `bvhBuildMs == 0.0`: steps 5 and 6 contain a transform edit, and the transform path
reports the subtrees it rebuilt in bvhBuildMs (as it always has, tests/test_incremental.py).  There the counters show that the visibility and the transform
path ran and no full build did.  Step 6 shows every mesh AND puts the re-assigned material and the moved mesh back, so that the description is the start's
and the image can be compared with the first render's bit for bit.  The digest of the resident records is compared on a sequence of visibility edits alone
(steps 1-3, then show everything): step 4 changes a material word and step 5 re-lays a flat tree out as per-instance subtrees, which a digest of the node
and triangle bytes rightly sees."""
import copy
import os
import re
import subprocess
import sys
import textwrap

import numpy as np
import pytest

from gatling_amd import capi
from gatling_amd.scene import INTERP_CONSTANT, MAT_DIFFUSE, PRIMVAR_VEC3, TEX_BASE_COLOR, MaterialDesc, Primvar, RenderSettings, TextureBinding
from gatling_amd.scenes import interior_scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AOVS = ["albedo", "opacity", "thinWalled", "doubleSided", "normal", "objectId", "instanceId", "faceId", "depth"]


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
def test_header_declares_the_option_and_the_counter_and_keeps_api_version_8():
    text = open(os.path.join(ROOT, "include", "gi_c.h")).read()
    assert re.search(r"#define\s+GI_C_SCENE_OPTION_VISIBILITY_UPDATES\s+11\b", text)
    assert re.search(r"int\s+giCDebugSceneVisibilityUpdateCount\s*\(\s*const\s+GiCScene\s*\*", text)
    assert re.search(r"#define\s+GI_C_API_VERSION\s+8u?\b", text)
    L = capi.load_library()
    assert L.giCGetApiVersion() == 8
    assert hasattr(L, "giCDebugSceneVisibilityUpdateCount")


def test_harness_exposes_the_option_and_the_counter():
    assert capi.OPTION_VISIBILITY_UPDATES == 11
    assert callable(capi.Scene.set_mesh_visibility) and callable(capi.Scene.visibility_update_count)


def test_header_and_harness_declare_the_class_state_query():
    text = open(os.path.join(ROOT, "include", "gi_c.h")).read()
    assert re.search(r"int\s+giCDebugSceneClassState\s*\(\s*const\s+GiCScene\s*\*", text)
    assert hasattr(capi.load_library(), "giCDebugSceneClassState") and callable(capi.Scene.class_state)


def test_visibility_setter_keeps_raising_the_rebuild_flag():
    L = capi.load_library()
    for built in (0, 1):
        assert L.giCDebugEditDirtyFlags(11, built) == 1 | 2  # DIRTY_BVH | DIRTY_FRAMEBUFFER


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# the scene (tests/test_material_edits.py _lookdev_scene at its small size) and the edits
# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
def _image(seed, h=8, w=8):
    rng = np.random.default_rng(seed)
    a = np.ones((h, w, 4), np.float32); a[..., :3] = rng.uniform(0.05, 0.95, (h, w, 3))
    return a


def _lookdev_scene():
    """The small interior with a textured, a primvar-driven, a cutout, a diffuse and an OpenPBR BASE material bound to the first five clutter meshes."""
    d = interior_scene(clutter_instances=20, subdivisions=2, prototypes=3, material_count=4)
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


A, CUT, MOVED, B, REASSIGNED = 1, 3, 4, 8, 10  # mesh indices; CUT is the only mesh bound to the cutout material
CUTOUT_MATERIAL, DIFFUSE_MATERIAL = 7, 8


def test_scene_is_the_one_the_cases_are_written_for():
    d = _lookdev_scene()
    tris = lambda i: len(d.meshes[i].faces) * len(d.meshes[i].instance_transforms)
    assert d.triangle_count() == 6412
    assert d.materials[CUTOUT_MATERIAL].name == "cutout" and [i for i, m in enumerate(d.meshes) if m.material == CUTOUT_MATERIAL] == [CUT]
    assert A < CUT and len(d.meshes[A].instance_transforms) > 1 and d.meshes[A].name.startswith("/Clutter")  # instanced, in front of the cutout mesh
    assert d.triangle_count() - tris(A) - tris(B) >= 4096                                                    # both hidden: still above the floor
    assert d.triangle_count() - tris(A) - tris(B) - tris(MOVED) - tris(REASSIGNED) < 4096                    # the floor's fallback
    assert d.meshes[REASSIGNED].material != DIFFUSE_MATERIAL and len(d.meshes[MOVED].instance_transforms) > 1


def _translate(x, y, z):
    m = np.eye(4, dtype=np.float32); m[3, :3] = (x, y, z)
    return m


def _s1(sc, start):
    sc.set_mesh_visibility(A, False)


def _s2(sc, start):
    sc.set_mesh_visibility(B, False)


def _s3(sc, start):
    sc.set_mesh_visibility(A, True)


def _s4(sc, start):
    sc.set_mesh_visibility(A, False)
    sc.set_mesh_material(REASSIGNED, DIFFUSE_MATERIAL)


def _s5(sc, start):
    sc.set_mesh_visibility(B, False)  # (hidden since step 2: the setter raises the rebuild flag all the same, and the update finds no word to change)
    sc.set_mesh_transform(MOVED, np.asarray(start.meshes[MOVED].transform, np.float32).reshape(4, 4) @ _translate(0.2, -0.1, 0.1))


def _s6(sc, start):
    for i in range(len(sc.desc.meshes)):
        sc.set_mesh_visibility(i, True)
    sc.set_mesh_material(REASSIGNED, start.meshes[REASSIGNED].material)
    sc.set_mesh_transform(MOVED, np.asarray(start.meshes[MOVED].transform, np.float32).reshape(4, 4))


# (name, edit, a material edit rides along, a transform edit rides along)
SEQUENCE = [("1-hide-A", _s1, False, False), ("2-hide-B", _s2, False, False), ("3-show-A", _s3, False, False), ("4-hide-A-and-assign", _s4, True, False),
            ("5-hide-B-and-move", _s5, False, True), ("6-show-all-and-undo", _s6, True, True)]
RS = RenderSettings(spp=2, max_bounces=3, next_event_estimation=True, progressive_accumulation=False)
W, H = 24, 14
_oracle_cache = {}


def _bits_equal(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def _oracle(orc, key, desc):
    """The oracle's image and AOVs of the description at `key` (the same for every layout: rendered once, never changed)."""
    if key not in _oracle_cache:
        img, _ = orc.render(desc, RS, W, H, threads=8)
        _oracle_cache[key] = (img, orc.render_aovs(desc, RS, W, H, AOVS))
    return _oracle_cache[key]


def _check(orc, sc, key, got):
    fresh = capi.Scene(copy.deepcopy(sc.desc))
    try:
        ref = fresh.render_aovs(RS, W, H, AOVS)
        fresh_classes = fresh.class_state()
    finally:
        fresh.close()
    assert sc.class_state() == fresh_classes, f"{key}: class state {sc.class_state()} differs from a scene built from scratch, {fresh_classes}"
    oimg, oaov = _oracle(orc, key, sc.desc)
    for k in ["color"] + AOVS:
        assert _bits_equal(got[k], ref[k]), f"{key}: {k} differs from a scene built from scratch"
        assert _bits_equal(got[k], oimg if k == "color" else oaov[k]), f"{key}: {k} differs from the oracle"


def _make(layout, option_on=True):
    sc = capi.Scene(_lookdev_scene())
    if option_on:
        sc.set_option(capi.OPTION_VISIBILITY_UPDATES, 1)
    if layout == "device":
        sc.set_option(capi.OPTION_BVH_BUILD, 1)
    if layout == "two_level":
        sc.set_option(capi.OPTION_TWO_LEVEL, 1)
    return sc


def _partition(sc):
    """A transform edit and its reverse (the description is the start's again) re-lay the tree out as per-instance subtrees."""
    t0 = np.asarray(sc.desc.meshes[MOVED].transform, np.float32).reshape(4, 4).copy()
    sc.set_mesh_transform(MOVED, t0 @ _translate(0.1, 0.0, 0.05)); sc.render(RS, W, H)
    sc.set_mesh_transform(MOVED, t0); sc.render(RS, W, H)
    assert sc.update_counts() == {"full": 1, "transform": 2, "material": 0}


def _run_sequence(orc, layout, option_on=True):
    sc = _make(layout, option_on)
    start = copy.deepcopy(sc.desc)
    try:
        first = sc.render_aovs(RS, W, H, AOVS)
        assert sc.stats()["bvhBuildMs"] > 0.0 and sc.visibility_update_count() == 0
        if layout == "device":
            assert sc.validate_bvh()["device_built"]
        _check(orc, sc, "start", first)
        if layout == "partitioned":
            _partition(sc)
        for step, edit, with_material, with_transform in SEQUENCE:
            before, vis_before = sc.update_counts(), sc.visibility_update_count()
            edit(sc, start)
            got = sc.render_aovs(RS, W, H, AOVS)
            st, after, vis_after = sc.stats(), sc.update_counts(), sc.visibility_update_count()
            print(f"{layout} option {int(option_on)} {step}: bvhBuildMs {st['bvhBuildMs']:.3f} uploadMs {st['uploadMs']:.3f} counts {after} visibility {vis_after}")
            if not option_on:  # the parent's behaviour: every visibility edit rebuilds
                assert st["bvhBuildMs"] > 0.0 and after["full"] == before["full"] + 1 and vis_after == 0, (layout, step, st, after, vis_after)
            elif layout != "two_level":  # (two-level: either path is allowed, only the images are held)
                assert after["full"] == before["full"], (layout, step, after)
                assert vis_after == vis_before + 1, (layout, step, vis_after)
                assert after["material"] == before["material"] + int(with_material) and after["transform"] == before["transform"] + int(with_transform), (layout, step, after)
                if not with_transform:  # (the transform path reports the subtrees it rebuilt in bvhBuildMs: module docstring)
                    assert st["bvhBuildMs"] == 0.0, (layout, step, st["bvhBuildMs"])
                assert st["triangleCount"] == 6412  # what is resident, hidden triangles included
            _check(orc, sc, step, got)
        for k in ["color"] + AOVS:
            assert _bits_equal(got[k], first[k]), f"{layout}: {k} after the last step differs from the first render"
    finally:
        sc.close()


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["host", "device", "partitioned", "two_level"])
def test_visibility_edits_update_incrementally_and_bit_exactly(gi, orc, layout):
    _run_sequence(orc, layout)


@pytest.mark.gpu
def test_with_the_option_off_the_same_edits_rebuild_and_give_the_same_bits(gi, orc):
    _run_sequence(orc, "host", option_on=False)


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["host", "device"])
def test_hide_then_show_leaves_the_resident_records_bytewise_as_built(gi, layout):
    """Visibility edits alone (steps 1-3, then show everything) on the flat layouts: the digest of the resident node and triangle bytes is the build's again."""
    sc = _make(layout)
    try:
        sc.render(RS, W, H)
        built = sc.validate_bvh()
        assert built["violations"] == 0
        for _, edit, _, _ in SEQUENCE[:3]:
            edit(sc, None)
            sc.render(RS, W, H)
        assert sc.validate_bvh()["digest"] != built["digest"]  # B is hidden: zero edges, shifted ids behind it
        for i in range(len(sc.desc.meshes)):
            sc.set_mesh_visibility(i, True)
        sc.render(RS, W, H)
        after = sc.validate_bvh()
        assert sc.update_counts() == {"full": 1, "transform": 0, "material": 0} and sc.visibility_update_count() == 4
        assert after["violations"] == 0 and after["digest"] == built["digest"] and after["nodes"] == built["nodes"]
    finally:
        sc.close()


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# fallbacks, cutouts
# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
def _fresh_image(desc):
    fresh = capi.Scene(copy.deepcopy(desc))
    try:
        return fresh.render(RS, W, H)
    finally:
        fresh.close()


def _expect_rebuild(orc, sc, key, full):
    img = sc.render(RS, W, H)
    assert sc.stats()["bvhBuildMs"] > 0.0 and sc.update_counts()["full"] == full and sc.visibility_update_count() == 0, (key, sc.update_counts())
    assert _bits_equal(img, _fresh_image(sc.desc)), f"{key}: differs from a scene built from scratch"
    assert _bits_equal(img, _oracle(orc, key, sc.desc)[0]), f"{key}: differs from the oracle"


@pytest.mark.gpu
def test_hiding_below_the_triangle_floor_rebuilds(gi, orc):
    sc = _make("host")
    try:
        sc.render(RS, W, H)
        for i in (A, B, MOVED, REASSIGNED):
            sc.set_mesh_visibility(i, False)
        assert sc.desc.triangle_count() < 4096
        _expect_rebuild(orc, sc, "below-the-floor", 2)
        assert sc.stats()["triangleCount"] == sc.desc.triangle_count()
    finally:
        sc.close()


@pytest.mark.gpu
def test_mesh_invisible_at_the_first_build_rebuilds_when_shown(gi, orc):
    d = _lookdev_scene()
    d.meshes[B].visible = False
    sc = capi.Scene(d)
    try:
        sc.set_option(capi.OPTION_VISIBILITY_UPDATES, 1)
        sc.render(RS, W, H)
        assert sc.stats()["triangleCount"] == sc.desc.triangle_count() < 6412
        sc.set_mesh_visibility(B, True)
        _expect_rebuild(orc, sc, "start", 2)  # (the description is the start's)
        sc.set_mesh_visibility(B, False)      # ... and from here on the mesh has records on the device: the next hide is incremental
        img = sc.render(RS, W, H)
        assert sc.stats()["bvhBuildMs"] == 0.0 and sc.update_counts()["full"] == 2 and sc.visibility_update_count() == 1
        assert _bits_equal(img, _fresh_image(sc.desc))
    finally:
        sc.close()


@pytest.mark.gpu
def test_hiding_every_mesh_rebuilds(gi, orc):
    sc = _make("host")
    try:
        sc.render(RS, W, H)
        for i in range(len(sc.desc.meshes)):
            sc.set_mesh_visibility(i, False)
        _expect_rebuild(orc, sc, "nothing-visible", 2)
        for i in range(len(sc.desc.meshes)):
            sc.set_mesh_visibility(i, True)
        _expect_rebuild(orc, sc, "start", 3)
    finally:
        sc.close()


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["host", "partitioned"])
def test_hiding_the_only_cutout_mesh_and_showing_it_again(gi, orc, layout):
    """hasCutouts flips with the hide (the walks lose their any-hit test, the shadow order is chosen anew) and back with the show."""
    sc = _make(layout)
    try:
        first = sc.render_aovs(RS, W, H, AOVS)
        if layout == "partitioned":
            _partition(sc)
        full = sc.update_counts()["full"]
        sc.set_mesh_visibility(CUT, False)
        got = sc.render_aovs(RS, W, H, AOVS)
        assert sc.stats()["bvhBuildMs"] == 0.0 and sc.update_counts()["full"] == full and sc.visibility_update_count() == 1
        _check(orc, sc, "cutout-mesh-hidden", got)
        sc.set_mesh_visibility(CUT, True)
        got = sc.render_aovs(RS, W, H, AOVS)
        assert sc.stats()["bvhBuildMs"] == 0.0 and sc.update_counts()["full"] == full and sc.visibility_update_count() == 2
        _check(orc, sc, "start", got)
        for k in got:
            assert _bits_equal(got[k], first[k])
    finally:
        sc.close()


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["host", "partitioned"])
def test_material_assigned_to_a_hidden_mesh_counts_only_once_it_is_shown(gi, orc, layout):
    """The cutout mesh is hidden and, before the same render, bound to a material of a class no visible mesh uses: neither the cutout flag nor that class's bit
    may be set while it is hidden (a fresh build leaves the mesh out), and the class's bit appears with the show."""
    sc = _make(layout)
    try:
        sc.render(RS, W, H)
        if layout == "partitioned":
            _partition(sc)
        assert [i for i, m in enumerate(sc.desc.meshes) if m.material == DIFFUSE_MATERIAL] == [MOVED] and sc.desc.materials[DIFFUSE_MATERIAL].klass == MAT_DIFFUSE
        sc.set_mesh_material(MOVED, 4)  # the only mesh of the diffuse class leaves it
        got = sc.render_aovs(RS, W, H, AOVS)
        _check(orc, sc, "diffuse-class-unused", got)
        assert sc.class_state()["classMask"] & (1 << MAT_DIFFUSE) == 0 and sc.class_state()["hasCutouts"]
        before, vis_before = sc.update_counts(), sc.visibility_update_count()
        sc.set_mesh_visibility(CUT, False)
        sc.set_mesh_material(CUT, DIFFUSE_MATERIAL)  # the cutout material is bound to no mesh, the diffuse one to a hidden mesh alone
        got = sc.render_aovs(RS, W, H, AOVS)
        assert sc.stats()["bvhBuildMs"] == 0.0 and sc.visibility_update_count() == vis_before + 1
        assert sc.update_counts() == {"full": before["full"], "transform": before["transform"], "material": before["material"] + 1}
        _check(orc, sc, "hidden-mesh-reassigned", got)
        assert sc.class_state()["classMask"] & (1 << MAT_DIFFUSE) == 0 and not sc.class_state()["hasCutouts"]
        sc.set_mesh_visibility(CUT, True)
        got = sc.render_aovs(RS, W, H, AOVS)
        assert sc.stats()["bvhBuildMs"] == 0.0 and sc.update_counts()["full"] == before["full"] and sc.visibility_update_count() == vis_before + 2
        _check(orc, sc, "reassigned-mesh-shown", got)
        assert sc.class_state()["classMask"] & (1 << MAT_DIFFUSE) and not sc.class_state()["hasCutouts"]
    finally:
        sc.close()


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["host", "device"])
def test_hide_and_move_compose_in_one_render_and_across_renders(gi, orc, layout):
    """A flat scene with a hidden mesh is re-laid out by the first move; a hide and a move arrive before the same render; a hidden mesh is moved, then shown."""
    sc = _make(layout)
    try:
        sc.render(RS, W, H)
        move = lambda i, x: sc.set_mesh_transform(i, np.asarray(sc.desc.meshes[i].transform, np.float32).reshape(4, 4) @ _translate(x, 0.05, -0.1))
        sc.set_mesh_visibility(A, False); move(MOVED, 0.15)                # flat -> partitioned, with A hidden in the same render
        got = sc.render_aovs(RS, W, H, AOVS); _check(orc, sc, "move-1", got)
        sc.set_mesh_visibility(B, False); move(A, -0.2)                    # partitioned: a hide, and the hidden A moves
        got = sc.render_aovs(RS, W, H, AOVS); _check(orc, sc, "move-2", got)
        sc.set_mesh_visibility(A, True); move(B, 0.1)                      # A comes back where it was moved to; the hidden B moves
        got = sc.render_aovs(RS, W, H, AOVS); _check(orc, sc, "move-3", got)
        sc.set_mesh_visibility(B, True)
        got = sc.render_aovs(RS, W, H, AOVS); _check(orc, sc, "move-4", got)
        assert sc.update_counts() == {"full": 1, "transform": 3, "material": 0} and sc.visibility_update_count() == 4
    finally:
        sc.close()


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# look-ahead, two device contexts
# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_hide_discards_the_look_ahead_window(gi, orc):
    rs = RenderSettings(spp=1, max_bounces=3, next_event_estimation=True)  # progressive
    sc = _make("host")
    try:
        sc.set_option(capi.OPTION_SAMPLE_LOOKAHEAD, 4)
        for _ in range(5):  # windows of 1 and 2; the fourth call traces a window of 4, the fifth is served from it
            sc.render(rs, W, H)
        la = sc.lookahead_stats()
        assert (la["windowCalls"], la["windowServed"], la["traced"]) == (4, 2, 0) and la["windowsDiscarded"] == 0, la
        sc.set_mesh_visibility(A, False)  # in the middle of the window: two of its four calls were never asked for
        img = sc.render(rs, W, H)
        la2 = sc.lookahead_stats()
        assert la2["windowsDiscarded"] == 1 and la2["samplesUnused"] == 2 and la2["traced"] == 1, la2
        assert sc.stats()["bvhBuildMs"] == 0.0 and sc.update_counts() == {"full": 1, "transform": 0, "material": 0} and sc.visibility_update_count() == 1
        ref, _ = orc.render(sc.desc, rs, W, H, threads=8)  # the accumulation restarted: the oracle's first frame of the scene without the mesh
        assert _bits_equal(img, ref)
    finally:
        sc.close()


TWO_CONTEXTS = textwrap.dedent("""
    import copy, sys
    sys.path.insert(0, %(root)r)
    sys.path.insert(0, %(tests)r)
    from gatling_amd import capi
    import test_visibility_edits as T
    L = capi.initialize(0)                      # $GATLING_DEVICES = "0,0": two contexts on the one GPU
    assert L.giCGetDeviceCount() == 2
    multi = T._make("host")
    single = T._make("host"); single.set_option(capi.OPTION_DEVICES, 1)
    start = copy.deepcopy(multi.desc)
    for sc in (multi, single):
        sc.render_aovs(T.RS, T.W, T.H, T.AOVS)
    for step, edit, _, _ in T.SEQUENCE[:4]:
        out = []
        for sc in (multi, single):
            edit(sc, start)
            out.append(sc.render_aovs(T.RS, T.W, T.H, T.AOVS))
            assert sc.stats()["bvhBuildMs"] == 0.0, (step, sc.stats()["bvhBuildMs"])
        for k in out[0]:
            assert T._bits_equal(out[0][k], out[1][k]), step + ": " + k + " differs between two device contexts and one"
    assert multi.update_counts() == {"full": 1, "transform": 0, "material": 1} and multi.visibility_update_count() == 4
    for d in (0, 1):
        assert multi.validate_bvh(d)["digest"] == single.validate_bvh(0)["digest"]
    fresh = capi.Scene(copy.deepcopy(multi.desc)); fresh.set_option(capi.OPTION_DEVICES, 1)
    ref = fresh.render_aovs(T.RS, T.W, T.H, T.AOVS)
    for k in ref:
        assert T._bits_equal(out[0][k], ref[k]), k + " differs from a scene built from scratch"
    multi.close(); single.close(); fresh.close()
    print("two contexts ok")
""")


@pytest.mark.gpu
def test_visibility_edits_reach_every_device_context():
    env = dict(os.environ); env["GATLING_DEVICES"] = "0,0"
    out = subprocess.run([sys.executable, "-c", TWO_CONTEXTS % {"root": ROOT, "tests": os.path.join(ROOT, "tests")}], capture_output=True, text=True, timeout=300,
                         env=env)
    assert out.returncode == 0 and "two contexts ok" in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# random sequences
# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
def _random_edit(rng, sc):
    d = sc.desc
    kind = int(rng.choice(6, p=np.float64([3, 1, 1, 1, 1, 1]) / 8.0))
    meshes = [i for i, m in enumerate(d.meshes) if m.name.startswith("/Clutter")]
    mi, other = (int(x) for x in rng.choice(meshes, 2, replace=False))
    mat = int(rng.integers(len(d.materials)))
    toggle = lambda i: sc.set_mesh_visibility(i, not d.meshes[i].visible)
    move = lambda i: sc.set_mesh_transform(i, np.asarray(d.meshes[i].transform, np.float32).reshape(4, 4) @ _translate(*rng.uniform(-0.2, 0.2, 3)))
    if kind == 0:
        toggle(mi); return "visibility"
    if kind == 1:
        sc.set_mesh_material(mi, mat); return "assign"
    if kind == 2:
        m = copy.deepcopy(d.materials[mat]); m.params[0:3] = rng.uniform(0.05, 0.95, 3).astype(np.float32)
        sc.replace_material(mat, m); return "colour"
    if kind == 3:
        move(mi); return "transform"
    if kind == 4:
        toggle(mi); sc.set_mesh_material(other, mat); return "visibility+assign"
    toggle(mi); move(other); return "visibility+transform"


@pytest.mark.gpu
def test_random_edit_sequences_match_the_oracle(gi, orc):
    """60 sequences of four random edits each with the option on; every render is compared with the oracle's render of the description at that point.  Every
    scene starts with one random clutter mesh invisible: showing it is the "no records on the device" fallback, so full builds beyond each scene's first
    happen as well (and hiding enough falls under the floor)."""
    rs = RenderSettings(spp=1, max_bounces=3, next_event_estimation=True, progressive_accumulation=False)
    rng = np.random.default_rng(20250)
    kinds, counts = {}, {"full": 0, "transform": 0, "material": 0, "visibility": 0}
    scenes = 60
    for seq in range(scenes):
        d = _lookdev_scene()
        d.meshes[int(rng.integers(1, len(d.meshes)))].visible = False
        sc = capi.Scene(d)
        try:
            sc.set_option(capi.OPTION_VISIBILITY_UPDATES, 1)
            sc.render(rs, W, H)
            for k in range(4):
                kind = _random_edit(rng, sc)
                kinds[kind] = kinds.get(kind, 0) + 1
                img = sc.render(rs, W, H)
                ref, _ = orc.render(sc.desc, rs, W, H, threads=8)
                assert _bits_equal(img, ref), (seq, k, kind, [m.visible for m in sc.desc.meshes])
            c = sc.update_counts()
            for name in ("full", "transform", "material"):
                counts[name] += c[name]
            counts["visibility"] += sc.visibility_update_count()
        finally:
            sc.close()
    print("random edit sequences:", kinds, counts)
    assert counts["visibility"] > 0 and counts["material"] > 0 and counts["transform"] > 0  # every incremental path was taken ...
    assert counts["full"] > scenes                                                         # ... and so were fallbacks (each scene's first render is a full build)

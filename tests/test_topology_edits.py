"""Incremental topology updates (gi_build.cpp updateTopology, gi_patch.hip k_place_part): with GI_C_SCENE_OPTION_TOPOLOGY_UPDATES a
giCCreateMesh or giCDestroyMesh after the build no longer rebuilds the scene.  A destroyed mesh of the built scene is retired -- its parts leave the top tree,
the triangles behind it are renumbered as a fresh build would number them -- and a new mesh is appended: records at the ends of the device arrays, one subtree
per instance (built by the host, or on the device and put in place by k_place_part).  This is what hdGatling does for every points, primvar or topology change
of a prim: destroy, create, every setter again.  The image and the AOVs must be bit-identical to a scene built from scratch from the edited description, and
to the oracle's render of it.  No tolerance anywhere.

CPU: the header and the harness declare the option, the counter and the three methods; the API version is unchanged; every edit raises the dirty flags it
raised before.
GPU: an edit sequence on the host-built, device-built and partitioned layouts, the same sequence with the option off, the declines, a retired mesh whose
material is destroyed, a vertex refit of an appended mesh, parts built on the device, the look-ahead window, two device contexts, random edit sequences
against the oracle, and the cost of a destroy + create on config C5's interior.

The scene is the look-development interior of tests/test_material_edits.py at its small size (6 412 flattened triangles in 12 meshes and 21 instances: above
the 4 096 floor of the incremental paths and beyond LDS).  Scene order there: mesh 1 (two instances, 640 triangles) lies in front of mesh 3, the only mesh
bound to the cutout material -- destroying mesh 1 shifts the ids the cutout test hashes, so a destroy that does not renumber changes pixels.  Meshes are found
by name: a destroy shifts the indices behind it."""
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
from gatling_amd.scene import INTERP_CONSTANT, MAT_DIFFUSE, PRIMVAR_VEC3, TEX_BASE_COLOR, MaterialDesc, MeshDesc, Primvar, RenderSettings, TextureBinding
from gatling_amd.scenes import interior_scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AOVS = ["albedo", "opacity", "thinWalled", "doubleSided", "normal", "objectId", "instanceId", "faceId", "depth"]
DIRTY_BVH, DIRTY_FRAMEBUFFER, DIRTY_MATERIALS, DIRTY_XFORM = 1, 2, 8, 16


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
def test_header_declares_the_option_and_the_counter_and_keeps_api_version_8():
    text = open(os.path.join(ROOT, "include", "gi_c.h")).read()
    assert re.search(r"#define\s+GI_C_SCENE_OPTION_TOPOLOGY_UPDATES\s+13\b", text)
    assert re.search(r"int\s+giCDebugSceneTopologyUpdateCount\s*\(\s*const\s+GiCScene\s*\*\s*\w+\s*,\s*uint64_t\s*\*", text)
    assert re.search(r"#define\s+GI_C_API_VERSION\s+8u?\b", text)
    L = capi.load_library()
    assert L.giCGetApiVersion() == 8
    assert hasattr(L, "giCDebugSceneTopologyUpdateCount")


def test_harness_exposes_the_option_and_the_three_methods():
    assert capi.OPTION_TOPOLOGY_UPDATES == 13
    assert "giCDebugSceneTopologyUpdateCount" in [name for name, _, _ in capi.SYMBOLS]
    assert callable(capi.Scene.create_mesh) and callable(capi.Scene.destroy_mesh) and callable(capi.Scene.topology_update_count)


# giCDebugEditDirtyFlags(edit, built) as the parent answers it: material-side edits (0-9), the transform (10), the geometry side (11-16)
_M, _G = DIRTY_MATERIALS | DIRTY_FRAMEBUFFER, DIRTY_BVH | DIRTY_FRAMEBUFFER
PARENT_FLAGS = {0: (_M | DIRTY_BVH, _M), 1: (_M | DIRTY_BVH, _M), 2: (_G, _M), 3: (_M | DIRTY_BVH, _M), 4: (_M | DIRTY_BVH, _M), 5: (_M | DIRTY_BVH, _M),
                6: (_M, _M), 7: (_M | DIRTY_BVH, _M), 8: (_G, _M), 9: (_G, _M), 10: (_G, DIRTY_XFORM | DIRTY_FRAMEBUFFER), 11: (_G, _G), 12: (_G, _G), 13: (_G, _G),
                14: (_G, _G), 15: (_G, _G), 16: (_G, _G)}


@pytest.mark.parametrize("edit", sorted(PARENT_FLAGS))
def test_every_edit_raises_the_dirty_flags_it_raised_before(edit):
    L = capi.load_library()
    assert (L.giCDebugEditDirtyFlags(edit, 0), L.giCDebugEditDirtyFlags(edit, 1)) == PARENT_FLAGS[edit]


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


A, CUT, MOVED, B, REASSIGNED = "/Clutter/p0_m1", "/Clutter/p0_m3", "/Clutter/p0_m4", "/Clutter/p2_m1", "/Clutter/p2_m3"  # scene-order indices 1, 3, 4, 8, 10
CUTOUT_MATERIAL, DIFFUSE_MATERIAL = 7, 8
PARTS = 21  # flattened instances of the scene: the re-layout reserves a top range of 2 * (2 * 21 + 16) = 116 nodes with the option on


def _idx(sc_or_desc, name):
    d = getattr(sc_or_desc, "desc", sc_or_desc)
    return next(i for i, m in enumerate(d.meshes) if m.name == name)


def _tris(d, i):
    return len(d.meshes[i].faces) * len(d.meshes[i].instance_transforms)


def test_scene_is_the_one_the_cases_are_written_for():
    d = _lookdev_scene()
    assert d.triangle_count() == 6412 and sum(len(m.instance_transforms) for m in d.meshes) == PARTS
    assert [_idx(d, n) for n in (A, CUT, MOVED, B, REASSIGNED)] == [1, 3, 4, 8, 10]
    assert d.materials[CUTOUT_MATERIAL].name == "cutout" and [m.name for m in d.meshes if m.material == CUTOUT_MATERIAL] == [CUT]
    assert len(d.meshes[1].instance_transforms) > 1                                     # instanced, in front of the cutout mesh
    assert d.triangle_count() - _tris(d, 1) - _tris(d, 8) >= 4096                       # both destroyed: still above the floor
    assert d.triangle_count() - _tris(d, 1) - _tris(d, 8) - _tris(d, 4) < 4096          # the floor's decline
    assert all(len(m.faces) > 128 for m in d.meshes[1:])                                 # every clutter part may go to the device builder


def _translate(x, y, z):
    m = np.eye(4, dtype=np.float32); m[3, :3] = (x, y, z)
    return m


def _displaced(vertices, amount, seed):
    rng = np.random.default_rng(seed)
    v = np.array(vertices, copy=True)
    p = v["pos"].astype(np.float64)
    k, phase = rng.uniform(2.0, 6.0, (3, 3)), rng.uniform(0.0, 6.28, 3)
    v["pos"] = (p + amount * np.sin(p @ k + phase)).astype(np.float32)
    return v


def _new_mesh(d, name, like, material, places, mesh_id, seed=5):
    """A clutter mesh of the scene's kind: the geometry of mesh `like` with displaced points, `places` = one (x, y, z, scale) per instance."""
    src = d.meshes[_idx(d, like)] if isinstance(like, str) else d.meshes[like]
    xf = []
    for x, y, z, s in places:
        m = np.eye(4, dtype=np.float32); m[0, 0] = m[1, 1] = m[2, 2] = s; m[3, :3] = (x, y, z)
        xf.append(m)
    return MeshDesc(name=name, vertices=_displaced(src.vertices, 0.08, seed), faces=np.array(src.faces, copy=True), material=material, id=mesh_id,
                    instance_transforms=np.stack(xf), instance_ids=np.arange(len(xf), dtype=np.int32))


def _resync(sc, name, seed):
    """hdGatling's answer to DirtyPoints / DirtyTopology (mesh.cpp:484-509): the mesh destroyed, created again from the new points, every setter again."""
    i = _idx(sc, name)
    md = copy.deepcopy(sc.desc.meshes[i])
    md.vertices = _displaced(md.vertices, 0.05, seed)
    sc.destroy_mesh(i)
    return sc.create_mesh(md)


def _s1(sc):
    sc.destroy_mesh(_idx(sc, A))


def _s2(sc):
    sc.create_mesh(_new_mesh(sc.desc, "/New/cutout", CUT, CUTOUT_MATERIAL, [(-1.0, -0.5, 1.1, 0.45), (1.2, 0.4, 1.4, 0.35)], 100))


def _s3(sc):
    _resync(sc, B, 11)


def _s4(sc):
    sc.destroy_mesh(_idx(sc, "/Clutter/p1_m2"))
    m = copy.deepcopy(sc.desc.materials[2]); m.params[0:3] = (0.9, 0.1, 0.6)
    sc.replace_material(2, m)  # destroyed and created: a new material, at the end of the library's table
    sc.create_mesh(_new_mesh(sc.desc, "/New/recoloured", MOVED, 2, [(0.3, -1.2, 0.9, 0.4)], 101, seed=6))


def _s5(sc):
    sc.create_mesh(_new_mesh(sc.desc, "/New/third", REASSIGNED, DIFFUSE_MATERIAL, [(-2.0, 1.0, 1.2, 0.3), (2.2, -1.4, 0.8, 0.3), (0.0, 0.0, 2.0, 0.25)], 102, seed=7))
    i = _idx(sc, MOVED)
    sc.set_mesh_transform(i, np.asarray(sc.desc.meshes[i].transform, np.float32).reshape(4, 4) @ _translate(0.2, -0.1, 0.1))
    sc.set_mesh_visibility(_idx(sc, "/Clutter/p1_m1"), False)
    sc.set_mesh_material(_idx(sc, REASSIGNED), DIFFUSE_MATERIAL)


# (name, edit, a material update rides along, a transform update rides along, a visibility update rides along)
SEQUENCE = [("1-destroy-A", _s1, False, False, False), ("2-create-cutout", _s2, False, False, False), ("3-resync-B", _s3, False, False, False),
            ("4-destroy-create-new-material", _s4, True, False, False), ("5-create-move-hide-assign", _s5, True, True, True)]
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
        sc.set_option(capi.OPTION_TOPOLOGY_UPDATES, 1)
    sc.set_option(capi.OPTION_VISIBILITY_UPDATES, 1)
    if layout == "device":
        sc.set_option(capi.OPTION_BVH_BUILD, 1)
    if layout == "two_level":
        sc.set_option(capi.OPTION_TWO_LEVEL, 1)
    return sc


def _partition(sc):
    """A transform edit and its reverse (the description is the start's again) re-lay the tree out as per-instance subtrees."""
    i = _idx(sc, MOVED)
    t0 = np.asarray(sc.desc.meshes[i].transform, np.float32).reshape(4, 4).copy()
    sc.set_mesh_transform(i, t0 @ _translate(0.1, 0.0, 0.05)); sc.render(RS, W, H)
    sc.set_mesh_transform(i, t0); sc.render(RS, W, H)
    assert sc.update_counts() == {"full": 1, "transform": 2, "material": 0}


def _run_sequence(orc, layout, option_on=True):
    sc = _make(layout, option_on)
    outputs = []
    try:
        first = sc.render_aovs(RS, W, H, AOVS)
        assert sc.stats()["bvhBuildMs"] > 0.0 and sc.topology_update_count() == 0
        if layout == "device":
            assert sc.validate_bvh()["device_built"]
        _check(orc, sc, "start", first)
        if layout == "partitioned":
            _partition(sc)
        for step, edit, with_material, with_transform, with_visibility in SEQUENCE:
            before, topo_before, vis_before = sc.update_counts(), sc.topology_update_count(), sc.visibility_update_count()
            edit(sc)
            got = sc.render_aovs(RS, W, H, AOVS)
            st, after, topo_after, vis_after = sc.stats(), sc.update_counts(), sc.topology_update_count(), sc.visibility_update_count()
            print(f"{layout} option {int(option_on)} {step}: bvhBuildMs {st['bvhBuildMs']:.3f} uploadMs {st['uploadMs']:.3f} counts {after} topology {topo_after} "
                  f"resident {st['triangleCount']} triangles, {st['nodeCount']} nodes")
            if not option_on:  # the parent's behaviour: every creation and destruction rebuilds
                assert st["bvhBuildMs"] > 0.0 and after["full"] == before["full"] + 1 and topo_after == 0, (layout, step, st, after, topo_after)
                assert st["triangleCount"] == sc.desc.triangle_count()
            else:
                assert after["full"] == before["full"], (layout, step, after)
                assert topo_after == topo_before + 1, (layout, step, topo_after)
                assert after["material"] == before["material"] + int(with_material) and after["transform"] == before["transform"] + int(with_transform), (layout, step, after)
                assert vis_after == vis_before + int(with_visibility), (layout, step, vis_after)
                assert st["triangleCount"] >= sc.desc.triangle_count()  # what is resident: retired triangles included
                v = sc.validate_bvh()
                assert v["violations"] == 0 and v["nodes"] == st["nodeCount"], (layout, step, v)
            _check(orc, sc, step, got)
            outputs.append(got)
    finally:
        sc.close()
    return outputs


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["host", "device", "partitioned"])
def test_topology_edits_update_incrementally_and_bit_exactly(gi, orc, layout):
    _run_sequence(orc, layout)


@pytest.mark.gpu
def test_with_the_option_off_the_same_edits_rebuild_and_give_the_same_bits(gi, orc):
    _run_sequence(orc, "host", option_on=False)


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# declines: each renders correctly through a counted full build
# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
def _fresh_image(desc):
    fresh = capi.Scene(copy.deepcopy(desc))
    try:
        return fresh.render(RS, W, H)
    finally:
        fresh.close()


def _expect_rebuild(orc, sc, key, full, topology):
    img = sc.render(RS, W, H)
    assert sc.stats()["bvhBuildMs"] > 0.0 and sc.update_counts()["full"] == full and sc.topology_update_count() == topology, (key, sc.update_counts(),
                                                                                                                               sc.topology_update_count())
    assert _bits_equal(img, _fresh_image(sc.desc)), f"{key}: differs from a scene built from scratch"
    assert _bits_equal(img, _oracle(orc, key, sc.desc)[0]), f"{key}: differs from the oracle"


def _expect_update(orc, sc, key, full, topology):
    img = sc.render(RS, W, H)
    assert sc.update_counts()["full"] == full and sc.topology_update_count() == topology, (key, sc.update_counts(), sc.topology_update_count())
    assert _bits_equal(img, _fresh_image(sc.desc)), f"{key}: differs from a scene built from scratch"
    assert _bits_equal(img, _oracle(orc, key, sc.desc)[0]), f"{key}: differs from the oracle"


@pytest.mark.gpu
def test_two_level_layout_declines(gi, orc):
    sc = _make("two_level")
    try:
        sc.render(RS, W, H)
        _s1(sc)
        _expect_rebuild(orc, sc, "1-destroy-A", 2, 0)
    finally:
        sc.close()


@pytest.mark.gpu
def test_incremental_switched_off_declines(gi, orc, monkeypatch):
    sc = _make("host")
    try:
        sc.render(RS, W, H)
        monkeypatch.setenv("GATLING_OPTIONS", "incremental=0")
        _s1(sc)
        _expect_rebuild(orc, sc, "1-destroy-A", 2, 0)
    finally:
        sc.close()


@pytest.mark.gpu
def test_destroying_below_the_triangle_floor_declines(gi, orc):
    sc = _make("host")
    try:
        sc.render(RS, W, H)
        for name in (A, B):
            sc.destroy_mesh(_idx(sc, name))
        _expect_update(orc, sc, "destroy-A-B", 1, 1)
        sc.destroy_mesh(_idx(sc, MOVED))
        assert sc.desc.triangle_count() < 4096
        _expect_rebuild(orc, sc, "below-the-floor", 2, 1)
        assert sc.stats()["triangleCount"] == sc.desc.triangle_count()
    finally:
        sc.close()


@pytest.mark.gpu
def test_flat_scene_that_loses_more_than_it_keeps_declines(gi, orc):
    """The first topology edit re-lays a flat scene out, which costs about a build: not worth it when most of what was built is leaving.  3 840 of the 6 412
    built triangles go and 1 600 new ones keep the scene above the floor."""
    sc = _make("host")
    try:
        sc.render(RS, W, H)
        for name in (A, "/Clutter/p0_m2", MOVED, "/Clutter/p1_m1", B):
            sc.destroy_mesh(_idx(sc, name))
        sc.create_mesh(_new_mesh(sc.desc, "/New/five", CUT, 3, [(-2.0 + k, -1.0 + 0.5 * k, 1.0, 0.35) for k in range(5)], 100))
        assert sc.desc.triangle_count() == 6412 - 3840 + 1600 >= 4096
        _expect_rebuild(orc, sc, "most-of-the-scene-replaced", 2, 0)
        _s2(sc)  # ... and the rebuilt scene takes the next edit in place
        _expect_update(orc, sc, "then-create-cutout", 2, 1)
    finally:
        sc.close()


@pytest.mark.gpu
def test_created_mesh_made_invisible_and_then_shown_declines(gi, orc):
    """A mesh created invisible is left out, as a fresh build leaves it out.  Shown later, it lies in front of a mesh the path appended meanwhile: its ids
    would not be a fresh build's at the tail, and showing a mesh without records on the device is the visibility path's rebuild anyway."""
    sc = _make("host")
    try:
        sc.render(RS, W, H)
        hidden = _new_mesh(sc.desc, "/New/hidden", CUT, CUTOUT_MATERIAL, [(-1.0, -0.5, 1.1, 0.45)], 100)
        hidden.visible = False
        sc.create_mesh(hidden)
        sc.create_mesh(_new_mesh(sc.desc, "/New/behind", MOVED, 3, [(0.3, -1.2, 0.9, 0.4)], 101, seed=6))
        _expect_update(orc, sc, "invisible-and-behind", 1, 1)
        assert sc.stats()["triangleCount"] == 6412 + 320
        sc.set_mesh_visibility(_idx(sc, "/New/hidden"), True)
        _expect_rebuild(orc, sc, "shown", 2, 1)
        assert sc.stats()["triangleCount"] == 6412 + 640
    finally:
        sc.close()


@pytest.mark.gpu
def test_instance_count_change_on_a_built_mesh_declines(gi, orc):
    sc = _make("host")
    try:
        sc.render(RS, W, H)
        _s2(sc)  # a topology edit is due as well: the count change decides
        i = _idx(sc, B)
        it = np.asarray(sc.desc.meshes[i].instance_transforms, np.float32).reshape(-1, 4, 4)[:-1].copy()
        sc.desc.meshes[i].instance_ids = np.asarray(sc.desc.meshes[i].instance_ids, np.int32)[:len(it)].copy()
        sc.set_mesh_instance_transforms(i, it)
        _expect_rebuild(orc, sc, "count-change", 2, 0)
    finally:
        sc.close()


@pytest.mark.gpu
def test_outgrowing_the_top_range_declines(gi, orc):
    """The re-layout reserves 2 * (2 * 21 + 16) = 116 top nodes; the path keeps to parts * 2 + 16 <= 116, that is 50 parts.  21 + 28 fit, one more mesh of
    two instances does not."""
    sc = _make("host")
    try:
        sc.render(RS, W, H)
        rng = np.random.default_rng(3)
        places = [(float(rng.uniform(-4, 4)), float(rng.uniform(-3, 3)), float(rng.uniform(0.4, 2.4)), 0.05) for _ in range(28)]
        tiny = _new_mesh(sc.desc, "/New/many", CUT, 3, places, 100)
        tiny.vertices, tiny.faces = tiny.vertices[:3].copy(), np.uint32([[0, 1, 2]])  # one triangle per instance
        sc.create_mesh(tiny)
        _expect_update(orc, sc, "28-small-parts", 1, 1)
        assert sc.validate_bvh()["violations"] == 0
        sc.create_mesh(_new_mesh(sc.desc, "/New/two-more", CUT, 3, [(-1.0, -0.5, 1.1, 0.3), (1.0, 0.5, 1.1, 0.3)], 101))
        _expect_rebuild(orc, sc, "two-more-parts", 2, 1)
    finally:
        sc.close()


@pytest.mark.gpu
def test_more_retired_than_live_triangles_declines_and_the_rebuild_compacts(gi, orc):
    """Every resync of mesh B retires 960 triangles.  6 412 live: six resyncs stay incremental (5 760 retired), the seventh (6 720) rebuilds, and the rebuild
    holds the live triangles alone."""
    sc = _make("host")
    try:
        sc.render(RS, W, H)
        for k in range(6):
            _resync(sc, B, 20 + k)
            sc.render(RS, W, H)
            assert sc.update_counts()["full"] == 1 and sc.topology_update_count() == k + 1 and sc.stats()["triangleCount"] == 6412 + 960 * (k + 1)
        assert sc.validate_bvh()["violations"] == 0
        _resync(sc, B, 26)
        _expect_rebuild(orc, sc, "seventh-resync", 2, 6)
        assert sc.stats()["triangleCount"] == sc.desc.triangle_count() == 6412
    finally:
        sc.close()


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# a retired mesh's material destroyed; a vertex refit of an appended mesh; parts built on the device
# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_retired_mesh_whose_material_is_destroyed(gi, orc):
    sc = _make("host")
    try:
        sc.render(RS, W, H)
        sc.destroy_mesh(_idx(sc, CUT))         # the only mesh bound to the cutout material ...
        sc.destroy_material(CUTOUT_MATERIAL)   # ... which goes too: the retired mesh is left without one
        got = sc.render_aovs(RS, W, H, AOVS)
        assert sc.update_counts() == {"full": 1, "transform": 0, "material": 1} and sc.topology_update_count() == 1
        assert not sc.class_state()["hasCutouts"]
        # (the description keeps the material, bound to no mesh: a scene built from it holds the same triangles with the same ids)
        _check(orc, sc, "cutout-mesh-and-material-destroyed", got)
        m = copy.deepcopy(sc.desc.materials[2]); m.params[0:3] = (0.2, 0.9, 0.3)
        sc.replace_material(2, m)
        got = sc.render_aovs(RS, W, H, AOVS)
        assert sc.update_counts() == {"full": 1, "transform": 0, "material": 2} and sc.topology_update_count() == 1 and sc.stats()["bvhBuildMs"] == 0.0
        _check(orc, sc, "then-another-material-edited", got)
    finally:
        sc.close()


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["host", "partitioned"])
def test_material_destroyed_mesh_created_and_mesh_hidden_in_one_render(gi, orc, layout):
    """The LAST material of the table goes (its only mesh re-assigned first), so the table shrinks; a mesh is created and another hidden before the same
    render.  The topology, visibility and material updates run in that order: between the first and the last the resident words index the previous, longer
    table, and nobody may derive the class state from them."""
    sc = _make(layout)
    try:
        sc.render(RS, W, H)
        if layout == "partitioned":
            _partition(sc)
        last = len(sc.desc.materials) - 1
        users = [i for i, m in enumerate(sc.desc.meshes) if m.material == last]
        assert sc.desc.materials[last].name == "base" and len(users) == 1
        before, topo, vis = sc.update_counts(), sc.topology_update_count(), sc.visibility_update_count()
        sc.set_mesh_material(users[0], 1)
        sc.destroy_material(last)
        sc.create_mesh(_new_mesh(sc.desc, "/New/beside", CUT, 2, [(-1.0, -0.5, 1.1, 0.45)], 100))
        sc.set_mesh_visibility(_idx(sc, A), False)
        got = sc.render_aovs(RS, W, H, AOVS)
        assert sc.update_counts() == {"full": before["full"], "transform": before["transform"], "material": before["material"] + 1}
        assert sc.topology_update_count() == topo + 1 and sc.visibility_update_count() == vis + 1
        assert sc.validate_bvh()["violations"] == 0
        _check(orc, sc, "material-destroyed-mesh-created-mesh-hidden", got)  # (the description keeps the material, bound to no mesh)
    finally:
        sc.close()


@pytest.mark.gpu
def test_move_then_destroy_in_one_frame_leaves_no_part_to_rebuild(gi, orc, monkeypatch, capfd):
    """A mesh moved and destroyed before the same render is retired without its transform flag: later moves of other meshes rebuild their own parts alone."""
    monkeypatch.setenv("GATLING_BUILD_TIMING", "1")
    sc = _make("host")
    try:
        sc.render(RS, W, H)
        i = _idx(sc, B)
        sc.set_mesh_transform(i, np.asarray(sc.desc.meshes[i].transform, np.float32).reshape(4, 4) @ _translate(0.1, 0.0, 0.1))
        sc.destroy_mesh(i)
        capfd.readouterr()
        sc.render(RS, W, H)
        # (the move raised the scene's transform flag: the transform path runs behind the topology update, is counted, and finds no part to rebuild)
        assert sc.update_counts() == {"full": 1, "transform": 1, "material": 0} and sc.topology_update_count() == 1
        lines = [ln for ln in capfd.readouterr().err.splitlines() if "transform update:" in ln]
        assert len(lines) == 1 and re.search(r"incremental, 0 part\(s\) rebuilt of 21", lines[0]), lines
        i = _idx(sc, CUT)  # one instance
        sc.set_mesh_transform(i, np.asarray(sc.desc.meshes[i].transform, np.float32).reshape(4, 4) @ _translate(0.1, 0.0, 0.1))
        got = sc.render_aovs(RS, W, H, AOVS)
        lines = [ln for ln in capfd.readouterr().err.splitlines() if "transform update:" in ln]
        assert len(lines) == 1 and re.search(r"incremental, 1 part\(s\) rebuilt of 21", lines[0]), lines
        _check(orc, sc, "B-destroyed-cutout-mesh-moved", got)
    finally:
        sc.close()


@pytest.mark.gpu
def test_vertex_edit_on_an_appended_mesh_refits(gi, orc):
    sc = _make("host")
    try:
        sc.set_option(capi.OPTION_VERTEX_UPDATES, 1)
        sc.render(RS, W, H)
        _s2(sc)
        sc.render(RS, W, H)
        assert sc.update_counts()["full"] == 1 and sc.topology_update_count() == 1
        i = _idx(sc, "/New/cutout")
        sc.set_mesh_vertices(i, _displaced(sc.desc.meshes[i].vertices, 0.04, 31))
        got = sc.render_aovs(RS, W, H, AOVS)
        assert sc.update_counts()["full"] == 1 and sc.vertex_update_count() == 1 and sc.topology_update_count() == 1 and sc.stats()["bvhBuildMs"] == 0.0
        rc = sc.refit_check()
        assert rc["differing"] == 0 and rc["nodes"] > 0, rc
        assert sc.validate_bvh()["violations"] == 0
        _check(orc, sc, "appended-mesh-deformed", got)
    finally:
        sc.close()


def _timing_lines(capfd):
    return [ln for ln in capfd.readouterr().err.splitlines() if "topology update:" in ln]


@pytest.mark.gpu
def test_appended_parts_built_on_the_device(gi, orc, monkeypatch, capfd):
    """GI_C_SCENE_OPTION_BVH_BUILD = 1 and device_parts_min = 1: the parts of the meshes steps 2 and 3 append are built by the device builder over their own
    records and put in place by k_place_part -- the library's timing line says how many."""
    host_route = _run_sequence(orc, "host")
    monkeypatch.setenv("GATLING_OPTIONS", "device_parts_min=1")
    monkeypatch.setenv("GATLING_BUILD_TIMING", "1")
    sc = _make("device")
    try:
        sc.render(RS, W, H)
        capfd.readouterr()
        for k, (step, edit, _, _, _) in enumerate(SEQUENCE[:3]):
            edit(sc)
            got = sc.render_aovs(RS, W, H, AOVS)
            lines = _timing_lines(capfd)
            assert len(lines) == 1, lines
            m = re.search(r"(\d+) part\(s\) built, (\d+) of them on the device \(k_place_part\)", lines[0])
            assert m, lines[0]
            expected = [0, 2, 3][k]  # the cutout mesh has two instances, mesh B three
            assert (int(m.group(1)), int(m.group(2))) == (expected, expected), lines[0]
            assert sc.update_counts()["full"] == 1 and sc.topology_update_count() == k + 1
            v = sc.validate_bvh()
            assert v["violations"] == 0, (step, v)
            _check(orc, sc, step, got)
            for name in ["color"] + AOVS:
                assert _bits_equal(got[name], host_route[k][name]), f"{step}: {name} differs from the host-built route"
        # a later vertex refit needs the device builder's levels; a later move rebuilds the part on the host
        sc.set_option(capi.OPTION_VERTEX_UPDATES, 1)
        i = _idx(sc, "/New/cutout")
        sc.set_mesh_vertices(i, _displaced(sc.desc.meshes[i].vertices, 0.04, 31))
        got = sc.render_aovs(RS, W, H, AOVS)
        assert sc.update_counts()["full"] == 1 and sc.vertex_update_count() == 1 and sc.refit_check()["differing"] == 0
        _check(orc, sc, "device-part-deformed", got)
        sc.set_mesh_transform(i, _translate(0.1, 0.1, -0.1))  # (the host's subtree may outgrow the range sized for the device's: then the scene rebuilds)
        got = sc.render_aovs(RS, W, H, AOVS)
        print("device-part-moved:", sc.update_counts())
        assert sc.validate_bvh()["violations"] == 0
        _check(orc, sc, "device-part-moved", got)
    finally:
        sc.close()


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# look-ahead, two device contexts
# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_topology_edit_discards_the_look_ahead_window(gi, orc):
    rs = RenderSettings(spp=1, max_bounces=3, next_event_estimation=True)  # progressive
    sc = _make("host")
    try:
        sc.set_option(capi.OPTION_SAMPLE_LOOKAHEAD, 4)
        for _ in range(5):  # windows of 1 and 2; the fourth call traces a window of 4, the fifth is served from it
            sc.render(rs, W, H)
        la = sc.lookahead_stats()
        assert (la["windowCalls"], la["windowServed"], la["traced"]) == (4, 2, 0) and la["windowsDiscarded"] == 0, la
        _s1(sc)  # in the middle of the window: two of its four calls were never asked for
        _s2(sc)
        img = sc.render(rs, W, H)
        la2 = sc.lookahead_stats()
        assert la2["windowsDiscarded"] == 1 and la2["samplesUnused"] == 2 and la2["traced"] == 1, la2
        assert sc.update_counts() == {"full": 1, "transform": 0, "material": 0} and sc.topology_update_count() == 1
        ref, _ = orc.render(sc.desc, rs, W, H, threads=8)  # the accumulation restarted: the oracle's first frame of the edited scene
        assert _bits_equal(img, ref)
    finally:
        sc.close()


TWO_CONTEXTS = textwrap.dedent("""
    import copy, sys
    sys.path.insert(0, %(root)r)
    sys.path.insert(0, %(tests)r)
    from gatling_amd import capi
    import test_topology_edits as T
    L = capi.initialize(0)                      # $GATLING_DEVICES = "0,0": two contexts on the one GPU
    assert L.giCGetDeviceCount() == 2
    multi = T._make("host")
    single = T._make("host"); single.set_option(capi.OPTION_DEVICES, 1)
    for sc in (multi, single):
        sc.render_aovs(T.RS, T.W, T.H, T.AOVS)
    for step, edit, _, _, _ in T.SEQUENCE[:4]:
        out = []
        for sc in (multi, single):
            edit(sc)
            out.append(sc.render_aovs(T.RS, T.W, T.H, T.AOVS))
        for k in out[0]:
            assert T._bits_equal(out[0][k], out[1][k]), step + ": " + k + " differs between two device contexts and one"
    assert multi.update_counts() == {"full": 1, "transform": 0, "material": 1} and multi.topology_update_count() == 4
    for d in (0, 1):
        v = multi.validate_bvh(d)
        assert v["violations"] == 0 and v["digest"] == single.validate_bvh(0)["digest"], (d, v)
    fresh = capi.Scene(copy.deepcopy(multi.desc)); fresh.set_option(capi.OPTION_DEVICES, 1)
    ref = fresh.render_aovs(T.RS, T.W, T.H, T.AOVS)
    for k in ref:
        assert T._bits_equal(out[0][k], ref[k]), k + " differs from a scene built from scratch"
    multi.close(); single.close(); fresh.close()
    print("two contexts ok")
""")


@pytest.mark.gpu
def test_topology_edits_reach_every_device_context():
    env = dict(os.environ); env["GATLING_DEVICES"] = "0,0"
    out = subprocess.run([sys.executable, "-c", TWO_CONTEXTS % {"root": ROOT, "tests": os.path.join(ROOT, "tests")}], capture_output=True, text=True, timeout=300,
                         env=env)
    assert out.returncode == 0 and "two contexts ok" in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# random sequences
# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
def _random_edit(rng, sc, serial):
    d = sc.desc
    kind = ("create", "destroy", "move", "hide", "assign")[int(rng.integers(5))]
    clutter = [i for i, m in enumerate(d.meshes) if not m.name.startswith("/Room")]
    mi = int(rng.choice(clutter))
    mat = int(rng.integers(len(d.materials)))
    if kind == "create":
        places = [(float(rng.uniform(-4, 4)), float(rng.uniform(-3, 3)), float(rng.uniform(0.4, 2.4)), float(rng.uniform(0.2, 0.5))) for _ in range(int(rng.integers(1, 4)))]
        sc.create_mesh(_new_mesh(d, f"/New/r{serial}", mi, mat, places, 200 + serial, seed=serial))
    elif kind == "destroy":
        sc.destroy_mesh(mi)
    elif kind == "move":
        sc.set_mesh_transform(mi, np.asarray(d.meshes[mi].transform, np.float32).reshape(4, 4) @ _translate(*rng.uniform(-0.2, 0.2, 3)))
    elif kind == "hide":
        sc.set_mesh_visibility(mi, not d.meshes[mi].visible)
    else:
        sc.set_mesh_material(mi, mat)
    return kind


@pytest.mark.gpu
@pytest.mark.parametrize("case", range(8))
def test_random_edit_sequences_match_the_oracle(gi, orc, case):
    """40 seeded sequences (five per case) of six steps drawn from create / destroy / move / hide / assign, options 13 and 11 on; every render is compared
    with the oracle's render of the description at that point.  Declines happen as well: destroys fall under the floor, shows of meshes created hidden."""
    rs = RenderSettings(spp=1, max_bounces=3, next_event_estimation=True, progressive_accumulation=False)
    rng = np.random.default_rng(20260 + case)
    kinds, counts = {}, {"full": 0, "transform": 0, "material": 0, "visibility": 0, "topology": 0}
    for seq in range(5):
        sc = _make(("host", "device")[seq % 2])
        try:
            sc.render(rs, W, H)
            for k in range(6):
                kind = _random_edit(rng, sc, 10 * seq + k)
                kinds[kind] = kinds.get(kind, 0) + 1
                img = sc.render(rs, W, H)
                ref, _ = orc.render(sc.desc, rs, W, H, threads=8)
                assert _bits_equal(img, ref), (case, seq, k, kind, [m.name for m in sc.desc.meshes], [m.visible for m in sc.desc.meshes])
            c = sc.update_counts()
            for name in ("full", "transform", "material"):
                counts[name] += c[name]
            counts["visibility"] += sc.visibility_update_count(); counts["topology"] += sc.topology_update_count()
        finally:
            sc.close()
    print("random edit sequences:", kinds, counts)
    assert counts["topology"] > 0


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# cost
# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_destroy_and_create_on_c5_costs_a_fraction_of_a_rebuild(gi):
    """Config C5's interior (10.24 M instanced triangles): the full build against hdGatling's resync -- destroy + create -- of one 40 960-triangle clutter mesh
    (8 instances of 5 120 faces), in one process.  The first topology edit pays the one-time re-layout (about a build); the second is what every later
    frame of a deforming mesh pays, and it must stay under 10 % of the full build."""
    desc = interior_scene()
    rs = RenderSettings(spp=1, max_bounces=2, next_event_estimation=True, progressive_accumulation=False)
    w, h = 160, 90
    tris = lambda i: len(desc.meshes[i].faces) * len(desc.meshes[i].instance_transforms)
    clutter = [i for i, m in enumerate(desc.meshes) if m.name.startswith("/Clutter")]
    name = desc.meshes[min(clutter, key=lambda i: abs(tris(i) - 40960))].name
    sc = capi.Scene(desc)
    try:
        sc.set_option(capi.OPTION_TOPOLOGY_UPDATES, 1)
        sc.render(rs, w, h)
        full = sc.stats()
        full_ms = full["bvhBuildMs"] + full["uploadMs"]
        edited = _tris(sc.desc, _idx(sc, name))
        _resync(sc, name, 1); sc.render(rs, w, h)
        relayout = sc.stats()
        _resync(sc, name, 2)
        t0 = time.perf_counter(); img = sc.render(rs, w, h); call = (time.perf_counter() - t0) * 1e3
        edit = sc.stats()
        edit_ms = edit["bvhBuildMs"] + edit["uploadMs"]
        print(f"C5 full build {full['bvhBuildMs']:.0f} + {full['uploadMs']:.0f} ms; first topology edit (re-layout) {relayout['bvhBuildMs']:.0f} + {relayout['uploadMs']:.0f} ms; "
              f"destroy + create of a {edited}-triangle mesh {edit['bvhBuildMs']:.1f} + {edit['uploadMs']:.1f} ms = {100.0 * edit_ms / full_ms:.1f} % of the build "
              f"(render call {call:.1f} ms)")
        assert sc.update_counts() == {"full": 1, "transform": 0, "material": 0} and sc.topology_update_count() == 2
        assert edit_ms < 0.1 * full_ms
        assert edit["triangleCount"] == full["triangleCount"] + 2 * edited
        fresh = capi.Scene(copy.deepcopy(sc.desc))
        try:
            ref = fresh.render(rs, w, h)
        finally:
            fresh.close()
        assert _bits_equal(img, ref)
    finally:
        sc.close()

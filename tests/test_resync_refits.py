"""Resyncs as refits (gi_build.cpp adoptResyncs, gi_refit.hip k_gather_shade): with GI_C_SCENE_OPTION_RESYNC_REFITS on top of topology and
vertex updates, hdGatling's answer to a points or primvar change of a prim -- giCDestroyMesh, giCCreateMesh, every setter again -- of a mesh whose faces did not
change is recognised: the new mesh adopts the resident records of the destroyed one, new points refit the resident subtree, and nothing is retired or appended.
The resident scene does not grow, so playback of a deforming mesh never reaches the rebuild that compacts retired triangles.  The adopting mesh sits where it
was created in scene order: its triangles and those of the meshes behind the destroyed one are renumbered as a fresh build numbers them.  Every vertex update
gathers the shading records on the device from the vertex records it has sent; giCDebugSceneShadeCheck compares both arrays, whole, with the host's copies.

Every image is compared bit for bit -- colour and nine AOVs -- with a scene built from scratch from the edited description and with the oracle's render of it.
The scene, sizes and settings are those of tests/test_topology_edits.py (6 412 flattened triangles, 24 x 14 pixels, 2 spp).  No tolerance anywhere."""
import copy
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest

from gatling_amd import capi
from gatling_amd.scene import INTERP_CONSTANT, PRIMVAR_VEC3, Primvar, RenderSettings

import test_topology_edits as T
from test_topology_edits import A, AOVS, B, CUT, CUTOUT_MATERIAL, DIFFUSE_MATERIAL, H, MOVED, RS, W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAYOUTS = ["host", "device", "partitioned"]
PRIMVAR_MESH = "/Clutter/p0_m2"  # the mesh bound to the primvar-driven material (the second clutter mesh of _lookdev_scene)


def _make(layout, vertex=True, resync=True, desc=None):
    sc = capi.Scene(desc if desc is not None else T._lookdev_scene())
    sc.set_option(capi.OPTION_TOPOLOGY_UPDATES, 1)
    sc.set_option(capi.OPTION_VISIBILITY_UPDATES, 1)
    sc.set_option(capi.OPTION_VERTEX_UPDATES, int(vertex))
    sc.set_option(capi.OPTION_RESYNC_REFITS, int(resync))
    if layout == "device":
        sc.set_option(capi.OPTION_BVH_BUILD, 1)
    return sc


def _start(layout, **kw):
    sc = _make(layout, **kw)
    sc.render(RS, W, H)
    if layout == "partitioned":
        T._partition(sc)
    return sc


def _resync(sc, name, seed=None, amount=0.05, **changes):
    """T._resync with a choice: `seed` None keeps the points; `changes` are set on the new mesh's description."""
    i = T._idx(sc, name)
    md = copy.deepcopy(sc.desc.meshes[i])
    if seed is not None:
        md.vertices = T._displaced(md.vertices, amount, seed)
    for k, v in changes.items():
        setattr(md, k, v)
    sc.destroy_mesh(i)
    return sc.create_mesh(md)


def _counters(sc):
    c = sc.update_counts()
    c.update(topology=sc.topology_update_count(), vertex=sc.vertex_update_count(), visibility=sc.visibility_update_count(), resync=sc.resync_count())
    return c


def _resident_is_sound(sc, key):
    assert sc.shade_check() == 0, key
    rc = sc.refit_check()
    assert rc["differing"] == 0 and rc["nodes"] > 0, (key, rc)
    v = sc.validate_bvh()
    assert v["violations"] == 0 and v["nodes"] == sc.stats()["nodeCount"], (key, v)


def test_the_scene_has_the_meshes_the_cases_name():
    d = T._lookdev_scene()
    assert d.meshes[T._idx(d, PRIMVAR_MESH)].primvars and d.materials[d.meshes[T._idx(d, PRIMVAR_MESH)].material].name == "primvar"
    assert T._idx(d, A) < T._idx(d, CUT) and len(d.meshes[T._idx(d, A)].instance_transforms) > 1
    # the clutter meshes share their faces and differ in id: two of them resynced in one frame can only pair with their own successors
    a, b = d.meshes[T._idx(d, MOVED)], d.meshes[T._idx(d, B)]
    assert np.array_equal(a.faces, b.faces) and a.id != b.id
    assert len(a.faces) == 320  # a multiple of 64: the gather-shapes case brings meshes of its own


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# 4. playback
# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("layout", LAYOUTS)
def test_playback_of_a_deforming_mesh_refits_and_never_rebuilds(gi, orc, layout):
    """Eight resyncs of mesh B with different points.  Without the option the seventh rebuilds (test_topology_edits: more retired than live triangles)."""
    sc = _start(layout)
    try:
        resident = None
        for k in range(8):
            before = _counters(sc)
            _resync(sc, B, 40 + k)
            got = sc.render_aovs(RS, W, H, AOVS)
            after, st = _counters(sc), sc.stats()
            print(f"{layout} playback {k}: {after} resident {st['triangleCount']} triangles, {st['nodeCount']} nodes, bvhBuildMs {st['bvhBuildMs']:.3f} uploadMs {st['uploadMs']:.3f}")
            assert after["full"] == 1, (k, after)
            assert after["resync"] == before["resync"] + 1 and after["vertex"] == before["vertex"] + 1 and after["topology"] == before["topology"] + 1, (k, before, after)
            if resident is None:
                resident = (st["triangleCount"], st["nodeCount"])  # after the first resync's re-layout
                assert st["triangleCount"] == 6412
            assert (st["triangleCount"], st["nodeCount"]) == resident, (k, st, resident)
            _resident_is_sound(sc, k)
            T._check(orc, sc, f"playback-{k}", got)
    finally:
        sc.close()


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# 5. scene order
# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("layout", LAYOUTS)
def test_adopting_mesh_takes_its_new_place_in_scene_order(gi, orc, layout):
    """Mesh A (two instances) lies in front of the cutout mesh; its successor lies behind every mesh.  The cutout test hashes the scene-order triangle id: an
    id base that stayed where A's was shows in the cutout pattern.  Then the cutout mesh itself is resynced."""
    sc = _start(layout)
    try:
        for step, name, seed in (("order-resync-A", A, 51), ("order-resync-cutout", CUT, 52)):
            before = _counters(sc)
            _resync(sc, name, seed)
            assert sc.desc.meshes[-1].name == name
            got = sc.render_aovs(RS, W, H, AOVS)
            after = _counters(sc)
            assert after["full"] == 1 and after["resync"] == before["resync"] + 1 and after["vertex"] == before["vertex"] + 1, (step, after)
            assert sc.stats()["triangleCount"] == 6412
            _resident_is_sound(sc, step)
            T._check(orc, sc, step, got)
    finally:
        sc.close()


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# 6. riders, 7. points unchanged, 8. two at once
# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("layout", LAYOUTS)
def test_resync_with_another_material_and_moved_transforms_is_adopted(gi, orc, layout):
    sc = _start(layout)
    try:
        before = _counters(sc)
        src = sc.desc.meshes[T._idx(sc, B)]
        it = np.array(src.instance_transforms, np.float32, copy=True).reshape(-1, 4, 4)
        it[1] = it[1] @ T._translate(0.15, -0.1, 0.05)
        xf = np.asarray(src.transform, np.float32).reshape(4, 4) @ T._translate(-0.1, 0.2, 0.1)
        _resync(sc, B, 61, material=DIFFUSE_MATERIAL, transform=xf, instance_transforms=it)
        got = sc.render_aovs(RS, W, H, AOVS)
        after = _counters(sc)
        assert after["resync"] == before["resync"] + 1 and after["full"] == 1, after
        assert after["material"] == before["material"] + 1 and after["transform"] == before["transform"] + 1 and after["vertex"] == before["vertex"] + 1, (before, after)
        assert sc.stats()["triangleCount"] == 6412 and sc.shade_check() == 0 and sc.validate_bvh()["violations"] == 0
        T._check(orc, sc, "riders", got)
    finally:
        sc.close()


@pytest.mark.gpu
@pytest.mark.parametrize("layout", LAYOUTS)
def test_resync_with_the_same_points_and_another_primvar_refits_nothing(gi, orc, layout):
    sc = _start(layout)
    try:
        before = _counters(sc)
        _resync(sc, PRIMVAR_MESH, None, primvars=[Primvar("tint", PRIMVAR_VEC3, INTERP_CONSTANT, np.float32([0.1, 0.8, 0.4]))])
        got = sc.render_aovs(RS, W, H, AOVS)
        after = _counters(sc)
        assert after["resync"] == before["resync"] + 1 and after["vertex"] == before["vertex"] and after["full"] == 1, (before, after)
        assert after["material"] == before["material"] + 1, (before, after)
        assert sc.stats()["triangleCount"] == 6412 and sc.shade_check() == 0 and sc.validate_bvh()["violations"] == 0
        T._check(orc, sc, "primvar-only", got)
    finally:
        sc.close()


@pytest.mark.gpu
@pytest.mark.parametrize("layout", LAYOUTS)
def test_two_meshes_with_the_same_faces_resynced_in_swapped_order(gi, orc, layout):
    sc = _start(layout)
    try:
        before = _counters(sc)
        first, second = (copy.deepcopy(sc.desc.meshes[T._idx(sc, n)]) for n in (MOVED, B))  # MOVED lies in front of B
        first.vertices, second.vertices = T._displaced(first.vertices, 0.05, 71), T._displaced(second.vertices, 0.05, 72)
        sc.destroy_mesh(T._idx(sc, MOVED)); sc.destroy_mesh(T._idx(sc, B))
        sc.create_mesh(second); sc.create_mesh(first)
        got = sc.render_aovs(RS, W, H, AOVS)
        after = _counters(sc)
        assert after["resync"] == before["resync"] + 2 and after["vertex"] == before["vertex"] + 1 and after["topology"] == before["topology"] + 1, (before, after)
        assert after["full"] == 1 and sc.stats()["triangleCount"] == 6412
        _resident_is_sound(sc, "two-at-once")
        T._check(orc, sc, "two-at-once", got)
    finally:
        sc.close()


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# 9. pairs that are retired and appended as before
# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
def _one_face_index_changed(sc):
    f = np.array(sc.desc.meshes[T._idx(sc, B)].faces, copy=True); f[7] = f[7][[1, 2, 0]]
    _resync(sc, B, 81, faces=f)
    return 960


def _another_instance_count(sc):
    m = sc.desc.meshes[T._idx(sc, B)]
    it = np.array(m.instance_transforms, np.float32, copy=True).reshape(-1, 4, 4)[:-1]
    _resync(sc, B, 81, instance_transforms=it, instance_ids=np.asarray(m.instance_ids, np.int32)[:len(it)].copy())
    return 640


def _other_instance_ids(sc):
    _resync(sc, B, 81, instance_ids=np.asarray(sc.desc.meshes[T._idx(sc, B)].instance_ids, np.int32) + 7)
    return 960


def _other_face_ids(sc):
    _resync(sc, B, 81, face_ids=np.arange(320, dtype=np.int32), max_face_id=319)
    return 960


def _double_sided_flipped(sc):
    _resync(sc, B, 81, double_sided=not sc.desc.meshes[T._idx(sc, B)].double_sided)
    return 960


def _unrelated_mesh_created_first(sc):
    md = copy.deepcopy(sc.desc.meshes[T._idx(sc, B)])
    md.vertices = T._displaced(md.vertices, 0.05, 81)
    sc.destroy_mesh(T._idx(sc, B))
    sc.create_mesh(T._new_mesh(sc.desc, "/New/unrelated", CUT, 3, [(0.3, -1.2, 0.9, 0.4)], 100))
    sc.create_mesh(md)
    return 960 + 320


def _plain_resync(sc):
    _resync(sc, B, 81)
    return 960


FALLBACKS = {"face-index": (_one_face_index_changed, {}), "instance-count": (_another_instance_count, {}), "instance-ids": (_other_instance_ids, {}),
             "face-ids": (_other_face_ids, {}), "double-sided": (_double_sided_flipped, {}), "unrelated-first": (_unrelated_mesh_created_first, {}),
             "vertex-updates-off": (_plain_resync, {"vertex": False}), "resync-refits-off": (_plain_resync, {"resync": False})}


@pytest.mark.gpu
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("case", sorted(FALLBACKS))
def test_pair_that_does_not_qualify_is_retired_and_appended(gi, orc, layout, case):
    edit, options = FALLBACKS[case]
    sc = _start(layout, **options)
    try:
        before = _counters(sc)
        appended = edit(sc)
        got = sc.render_aovs(RS, W, H, AOVS)
        after = _counters(sc)
        assert after["resync"] == 0 and after["full"] == 1 and after["topology"] == before["topology"] + 1 and after["vertex"] == before["vertex"], (case, before, after)
        assert sc.stats()["triangleCount"] == 6412 + appended, (case, sc.stats())
        assert sc.validate_bvh()["violations"] == 0 and sc.shade_check() == 0
        T._check(orc, sc, "fallback-" + case, got)
    finally:
        sc.close()


@pytest.mark.gpu
@pytest.mark.parametrize("layout", LAYOUTS)
def test_mesh_hidden_by_the_visibility_path_is_retired_and_appended(gi, orc, layout):
    sc = _start(layout)
    try:
        sc.set_mesh_visibility(T._idx(sc, B), False)
        sc.render(RS, W, H)
        before = _counters(sc)
        assert before["visibility"] == 1 and before["full"] == 1
        _resync(sc, B, 81, visible=True)
        got = sc.render_aovs(RS, W, H, AOVS)
        after = _counters(sc)
        assert after["resync"] == 0 and after["full"] == 1 and after["topology"] == before["topology"] + 1 and after["vertex"] == before["vertex"], (before, after)
        assert sc.stats()["triangleCount"] == 6412 + 960 and sc.validate_bvh()["violations"] == 0
        T._check(orc, sc, "fallback-hidden", got)
    finally:
        sc.close()


@pytest.mark.gpu
def test_with_the_option_off_the_sequence_counts_what_it_counted(gi, orc):
    """test_topology_edits' sequence with topology, visibility and vertex updates on and resync_refits off: the counters of _run_sequence, step by step."""
    sc = _make("host", resync=False)
    try:
        sc.render(RS, W, H)
        for step, edit, with_material, with_transform, with_visibility in T.SEQUENCE:
            before = _counters(sc)
            edit(sc)
            got = sc.render_aovs(RS, W, H, AOVS)
            after, st = _counters(sc), sc.stats()
            assert after["full"] == before["full"] and after["topology"] == before["topology"] + 1 and after["resync"] == 0 and after["vertex"] == 0, (step, after)
            assert after["material"] == before["material"] + int(with_material) and after["transform"] == before["transform"] + int(with_transform), (step, after)
            assert after["visibility"] == before["visibility"] + int(with_visibility), (step, after)
            assert st["triangleCount"] >= sc.desc.triangle_count()
            v = sc.validate_bvh()
            assert v["violations"] == 0 and v["nodes"] == st["nodeCount"], (step, v)
            T._check(orc, sc, step, got)
        assert sc.stats()["triangleCount"] == 6412 + 640 + 960 + 320 + 960  # every created mesh appended, the resynced mesh B among them
    finally:
        sc.close()


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# 10. parts the device builder made
# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_resync_of_a_mesh_whose_parts_the_device_built(gi, orc, monkeypatch, capfd):
    """The first resync appends mesh B with resync_refits switched off by the environment: its three parts go through buildBvh8Device and k_place_part, which
    leaves the records in leaf order on the device.  Two adopted resyncs then refit those parts."""
    monkeypatch.setenv("GATLING_BUILD_TIMING", "1")
    monkeypatch.setenv("GATLING_OPTIONS", "device_parts_min=1,resync_refits=0")
    sc = _make("device")
    try:
        sc.render(RS, W, H)
        capfd.readouterr()
        _resync(sc, B, 90)
        sc.render(RS, W, H)
        lines = [ln for ln in capfd.readouterr().err.splitlines() if "topology update:" in ln]
        assert len(lines) == 1 and "3 part(s) built, 3 of them on the device (k_place_part)" in lines[0] and " 0 adopted" in lines[0], lines
        assert sc.resync_count() == 0 and sc.stats()["triangleCount"] == 6412 + 960
        monkeypatch.setenv("GATLING_OPTIONS", "device_parts_min=1")
        for k in range(2):
            before = _counters(sc)
            _resync(sc, B, 91 + k)
            got = sc.render_aovs(RS, W, H, AOVS)
            after = _counters(sc)
            lines = [ln for ln in capfd.readouterr().err.splitlines() if "topology update:" in ln]
            assert len(lines) == 1 and " 1 adopted" in lines[0] and "0 part(s) built" in lines[0], lines
            assert after["resync"] == before["resync"] + 1 and after["vertex"] == before["vertex"] + 1 and after["full"] == 1, (before, after)
            assert sc.stats()["triangleCount"] == 6412 + 960
            _resident_is_sound(sc, k)
            T._check(orc, sc, f"device-parts-{k}", got)
    finally:
        sc.close()


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# 11. gather shapes: plain vertex updates
# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
def _scene_with_odd_meshes():
    """The lookdev scene and two meshes of 301 and 77 faces behind it -- no multiple of 64, nor of the gather's 256-thread block at nine threads a face (2 709
    and 693 threads) -- the first with two instances.  The clutter meshes have 320 faces, a multiple of 64, and do not qualify.  Both meshes lie behind
    others in the vertex array (vertexOffset != 0)."""
    d = T._lookdev_scene()
    for name, faces, places, mesh_id in (("/Odd/301", 301, [(-1.0, -0.5, 1.1, 0.45), (1.2, 0.4, 1.4, 0.35)], 300), ("/Odd/77", 77, [(0.3, -1.2, 0.9, 0.5)], 301)):
        m = T._new_mesh(d, name, CUT, 3, places, mesh_id)
        m.faces = np.array(m.faces[:faces], copy=True)
        d.meshes.append(m)
    return d


@pytest.mark.gpu
@pytest.mark.parametrize("layout", LAYOUTS)
def test_vertex_update_of_two_meshes_gathers_their_shading_records(gi, orc, layout):
    sc = _start(layout, desc=_scene_with_odd_meshes())
    try:
        assert sc.stats()["triangleCount"] == 6412 + 2 * 301 + 77 and sc.shade_check() == 0
        before = _counters(sc)
        for name, seed in (("/Odd/301", 95), ("/Odd/77", 96)):
            i = T._idx(sc, name)
            assert len(sc.desc.meshes[i].faces) % 64 != 0 and (9 * len(sc.desc.meshes[i].faces)) % 256 != 0
            sc.set_mesh_vertices(i, T._displaced(sc.desc.meshes[i].vertices, 0.05, seed))
        got = sc.render_aovs(RS, W, H, AOVS)
        after = _counters(sc)
        assert after["vertex"] == before["vertex"] + 1 and after["full"] == 1 and after["topology"] == before["topology"], (before, after)
        _resident_is_sound(sc, "gather-shapes")
        T._check(orc, sc, "gather-shapes", got)
    finally:
        sc.close()


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# 12. every device context
# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
TWO_CONTEXTS = textwrap.dedent("""
    import copy, sys
    sys.path.insert(0, %(root)r)
    sys.path.insert(0, %(tests)r)
    from gatling_amd import capi
    import test_topology_edits as T
    import test_resync_refits as R
    L = capi.initialize(0)                      # $GATLING_DEVICES = "0,0": two contexts on the one GPU
    assert L.giCGetDeviceCount() == 2
    multi = R._make("host")
    single = R._make("host"); single.set_option(capi.OPTION_DEVICES, 1)
    for sc in (multi, single):
        sc.render_aovs(T.RS, T.W, T.H, T.AOVS)
    for k in range(3):
        out = []
        for sc in (multi, single):
            R._resync(sc, T.B, 40 + k)
            out.append(sc.render_aovs(T.RS, T.W, T.H, T.AOVS))
        for name in out[0]:
            assert T._bits_equal(out[0][name], out[1][name]), "frame %%d: %%s differs between two device contexts and one" %% (k, name)
        assert multi.resync_count() == k + 1 and multi.vertex_update_count() == k + 1 and multi.update_counts()["full"] == 1
        for d in (0, 1):
            assert multi.shade_check(d) == 0, (k, d)
            assert multi.refit_check(d)["differing"] == 0, (k, d)
            v = multi.validate_bvh(d)
            assert v["violations"] == 0 and v["digest"] == single.validate_bvh(0)["digest"], (k, d, v)
    fresh = capi.Scene(copy.deepcopy(multi.desc)); fresh.set_option(capi.OPTION_DEVICES, 1)
    ref = fresh.render_aovs(T.RS, T.W, T.H, T.AOVS)
    for name in ref:
        assert T._bits_equal(out[0][name], ref[name]), name + " differs from a scene built from scratch"
    multi.close(); single.close(); fresh.close()
    print("two contexts ok")
""")


@pytest.mark.gpu
def test_resyncs_reach_every_device_context():
    env = dict(os.environ); env["GATLING_DEVICES"] = "0,0"
    out = subprocess.run([sys.executable, "-c", TWO_CONTEXTS % {"root": ROOT, "tests": os.path.join(ROOT, "tests")}], capture_output=True, text=True, timeout=300,
                         env=env)
    assert out.returncode == 0 and "two contexts ok" in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# 13. random sequences
# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
def _random_edit(rng, sc, serial):
    """test_topology_edits' generator with resyncs mixed in: every other draw, of a clutter mesh, with new points, the same points, or another material."""
    if rng.integers(2) == 0:
        return T._random_edit(rng, sc, serial)
    d = sc.desc
    clutter = [m.name for m in d.meshes if not m.name.startswith("/Room")]
    name = clutter[int(rng.integers(len(clutter)))]
    flavour = int(rng.integers(3))
    if flavour == 2:
        _resync(sc, name, 300 + serial, material=int(rng.integers(len(d.materials))))
    else:
        _resync(sc, name, 300 + serial if flavour == 0 else None)
    return "resync"


@pytest.mark.gpu
@pytest.mark.parametrize("seed", range(6))
def test_random_edit_sequences_with_resyncs_match_the_oracle(gi, orc, seed):
    """Two sequences of six steps per seed (host- and device-built), all four edit options on; EVERY frame is compared with the oracle's render of the
    description at that point."""
    rs = RenderSettings(spp=1, max_bounces=3, next_event_estimation=True, progressive_accumulation=False)
    rng = np.random.default_rng(77000 + seed)
    kinds, frames, adopted = {}, 0, 0
    for seq in range(2):
        sc = _make(("host", "device")[seq])
        try:
            sc.render(rs, W, H)
            for k in range(6):
                kind = _random_edit(rng, sc, 10 * seq + k)
                kinds[kind] = kinds.get(kind, 0) + 1
                img = sc.render(rs, W, H)
                ref, _ = orc.render(sc.desc, rs, W, H, threads=8)
                assert T._bits_equal(img, ref), (seed, seq, k, kind, [m.name for m in sc.desc.meshes], [m.visible for m in sc.desc.meshes], _counters(sc))
                assert sc.shade_check() == 0 and sc.validate_bvh()["violations"] == 0, (seed, seq, k, kind)
                frames += 1
            adopted += sc.resync_count()
        finally:
            sc.close()
    print("random sequences with resyncs:", kinds, "adopted", adopted)
    assert frames == 12 and kinds.get("resync", 0) > 0
    assert adopted > 0  # the adopted path ran, not only its declines

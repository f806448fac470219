"""Transform edits on the two-level layout without a rebuild (gi_build.cpp updateTransformsTwoLevel, gi_tlas.h, gi_tlas.hip k_inst_bounds /
k_inst_finish): with GI_C_SCENE_OPTION_TLAS_UPDATES a giCSetMeshTransform, or a giCSetMeshInstanceTransforms with an unchanged count, on a built two-level
scene no longer rebuilds it.  The next render re-sends the moved instances' records, makes their world boxes on the device, builds the TLAS again over the
instance boxes and refits the flat tree that AOVs and giCTraceRays walk.  The image and the AOVs must be bit-identical to a scene built from scratch and to the
oracle's render of the description; the resident two-level arrays must be bytewise what the scene build's own code makes from the current meshes
(Scene.tlas_check).  No tolerance anywhere.

CPU: the header, the library and the harness declare the option, the counter and the two hooks; the API version and the transform setters' dirty flags are
unchanged.
GPU: an edit sequence with the option on and off, the kernels' shapes, the declines, the composition with a material edit and with the look-ahead window,
giCTraceRays, two device contexts, random edit sequences against the oracle.

The scene, the render settings and the helpers are those of tests/test_visibility_edits.py (6 412 flattened triangles in 21 instances of 12 meshes: above the
4 096 floor, beyond LDS, so GI_C_SCENE_OPTION_TWO_LEVEL = 1 gives the two-level layout).  Instance transforms are USD row vectors: `S @ inst` changes an
instance in its own object space (it stays where it stands), `inst @ T` moves it in the world."""
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
from test_visibility_edits import (A, AOVS, B, CUT, DIFFUSE_MATERIAL, H, MOVED, REASSIGNED, RS, W, _bits_equal, _check, _fresh_image, _lookdev_scene, _oracle,
                                   _translate)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
def test_header_declares_the_option_the_counter_and_the_hooks_and_keeps_api_version_8():
    text = open(os.path.join(ROOT, "include", "gi_c.h")).read()
    assert re.search(r"#define\s+GI_C_SCENE_OPTION_TLAS_UPDATES\s+16\b", text)
    assert re.search(r"int\s+giCDebugSceneTlasUpdateCount\s*\(\s*const\s+GiCScene\s*\*", text)
    assert re.search(r"int\s+giCDebugSceneTlasCheck\s*\(\s*const\s+GiCScene\s*\*", text)
    assert re.search(r"int\s+giCDebugInstanceBounds\s*\(\s*const\s+GiCVertex\s*\*", text)
    assert re.search(r"#define\s+GI_C_API_VERSION\s+8u?\b", text)


def test_library_exports_the_symbols():
    L = capi.load_library()
    assert L.giCGetApiVersion() == 8
    for name in ("giCDebugSceneTlasUpdateCount", "giCDebugSceneTlasCheck", "giCDebugInstanceBounds"):
        assert hasattr(L, name), name


def test_harness_exposes_the_option_and_the_methods():
    assert capi.OPTION_TLAS_UPDATES == 16
    assert callable(capi.Scene.tlas_update_count) and callable(capi.Scene.tlas_check) and callable(capi.debug_instance_bounds)


def test_transform_setters_keep_their_dirty_flags():
    L = capi.load_library()
    assert L.giCDebugEditDirtyFlags(10, 0) == 1 | 2   # giCSetMeshTransform before the build: DIRTY_BVH | DIRTY_FRAMEBUFFER
    assert L.giCDebugEditDirtyFlags(10, 1) == 16 | 2  # ... on a built mesh: DIRTY_XFORM | DIRTY_FRAMEBUFFER, the incremental paths
    assert L.giCDebugEditDirtyFlags(15, 0) == 1 | 2   # giCSetMeshInstanceTransforms with another count: the rebuild flag either way
    assert L.giCDebugEditDirtyFlags(15, 1) == 1 | 2


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# the edits
# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
def _rotation(axis, angle):
    a = np.asarray(axis, np.float64); a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    R = np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)
    m = np.eye(4, dtype=np.float32); m[:3, :3] = R.T.astype(np.float32)  # (row vectors)
    return m


def _scale(x, y, z):
    return np.diag(np.float32([x, y, z, 1.0]))


def _instances(desc, i):
    return np.asarray(desc.meshes[i].instance_transforms, np.float32).reshape(-1, 4, 4).copy()


def _transform(desc, i):
    return np.asarray(desc.meshes[i].transform, np.float32).reshape(4, 4).copy()


def _s1(sc, start):  # one instance of an instanced mesh moves
    t = _instances(sc.desc, MOVED); t[1] = t[1] @ _translate(0.3, 0.1, -0.2)
    sc.set_mesh_instance_transforms(MOVED, t)


def _s2(sc, start):  # every instance of A turns and is scaled non-uniformly where it stands
    t = _instances(sc.desc, A)
    for k in range(len(t)):
        t[k] = (_scale(1.3, 0.7, 1.1) @ _rotation((0.3, 1.0, 0.2), 0.7 + 0.4 * k)) @ t[k]
    sc.set_mesh_instance_transforms(A, t)


def _s3(sc, start):  # the cutout mesh's instance is mirrored: a negative determinant
    t = _instances(sc.desc, CUT); t[0] = _scale(-1.0, 1.0, 1.0) @ t[0]
    assert np.linalg.det(t[0][:3, :3].astype(np.float64)) < 0
    sc.set_mesh_instance_transforms(CUT, t)


def _s4(sc, start):  # giCSetMeshTransform of an instanced mesh: all its instances move
    sc.set_mesh_transform(MOVED, _transform(sc.desc, MOVED) @ _translate(0.2, -0.1, 0.1))


def _s5(sc, start):  # two meshes before one render, one through each setter
    t = _instances(sc.desc, B); t[0] = t[0] @ _translate(-0.15, 0.05, 0.2)
    sc.set_mesh_instance_transforms(B, t)
    sc.set_mesh_transform(REASSIGNED, _transform(sc.desc, REASSIGNED) @ _translate(0.1, 0.1, -0.1))


def _s6(sc, start):  # everything back where it started
    for i in (MOVED, A, CUT, B):
        sc.set_mesh_instance_transforms(i, _instances(start, i))
    for i in (MOVED, REASSIGNED):
        sc.set_mesh_transform(i, _transform(start, i))


SEQUENCE = [("tl-1-translate-one-instance", _s1), ("tl-2-rotate-and-scale-A", _s2), ("tl-3-mirror-the-cutout", _s3), ("tl-4-mesh-transform", _s4),
            ("tl-5-two-meshes", _s5), ("tl-6-undo", _s6)]


def _make(option_on=True, two_level=True, desc=None):
    sc = capi.Scene(desc if desc is not None else _lookdev_scene())
    if two_level:
        sc.set_option(capi.OPTION_TWO_LEVEL, 1)
    if option_on:
        sc.set_option(capi.OPTION_TLAS_UPDATES, 1)
    return sc


def _resident_checks(sc, key, devices=(0,)):
    for d in devices:
        c = sc.tlas_check(d)
        assert c == 0 and c.two_level == 1 and c.instances == 21 and c.tlas_nodes >= 1, (key, d, int(c), c.two_level, c.instances, c.tlas_nodes, c.tlas_depth)
        assert sc.validate_bvh(d)["violations"] == 0, (key, d)


def _run_sequence(orc, option_on):
    sc = _make(option_on)
    start = copy.deepcopy(sc.desc)
    try:
        first = sc.render_aovs(RS, W, H, AOVS)
        assert sc.update_counts() == {"full": 1, "transform": 0, "material": 0} and sc.tlas_update_count() == 0
        _resident_checks(sc, "start")
        _check(orc, sc, "start", first)
        for step, edit in SEQUENCE:
            before, tlas_before = sc.update_counts(), sc.tlas_update_count()
            edit(sc, start)
            got = sc.render_aovs(RS, W, H, AOVS)
            st, after, tlas_after = sc.stats(), sc.update_counts(), sc.tlas_update_count()
            print(f"option {int(option_on)} {step}: bvhBuildMs {st['bvhBuildMs']:.3f} uploadMs {st['uploadMs']:.3f} counts {after} tlas {tlas_after}, TLAS {sc.tlas_check().tlas_nodes} node(s) in {sc.tlas_check().tlas_depth} level(s)")
            if option_on:
                assert after == before and tlas_after == tlas_before + 1, (step, before, after, tlas_after)
            else:  # the parent's behaviour: every transform edit of a two-level scene rebuilds
                assert after == {"full": before["full"] + 1, "transform": 0, "material": 0} and tlas_after == 0, (step, after, tlas_after)
            assert st["triangleCount"] == 6412
            _resident_checks(sc, step)
            _check(orc, sc, step, got)
            if step != SEQUENCE[-1][0]:
                assert not _bits_equal(got["color"], first["color"]) and not _bits_equal(got["depth"], first["depth"]), f"{step}: nothing moved in the image"
        for k in ["color"] + AOVS:
            assert _bits_equal(got[k], first[k]), f"{k} after the last step differs from the first render"
    finally:
        sc.close()


@pytest.mark.gpu
def test_transform_edits_update_the_two_level_scene_in_place_and_bit_exactly(gi, orc):
    _run_sequence(orc, True)


@pytest.mark.gpu
def test_with_the_option_off_the_same_edits_rebuild_and_give_the_same_bits(gi, orc):
    _run_sequence(orc, False)


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# the kernels: lane, wave, workgroup and chunk edges
# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
def _soup(n, seed):
    rng = np.random.default_rng(seed)
    v = np.zeros(3 * n, VERTEX_DTYPE)
    v["pos"] = rng.uniform(-5.0, 5.0, (3 * n, 3)).astype(np.float32)  # random triangles in a 10-unit cube
    return v, np.arange(3 * n, dtype=np.uint32).reshape(n, 3)


def _shape_transforms():
    t = [np.eye(4, dtype=np.float32), _translate(3.0, -2.0, 7.5), _rotation((1.0, 2.0, 3.0), 1.1), _scale(2.0, 0.25, 7.0), _scale(1.0, -1.0, 1.0),
         _scale(1e-6, 1e-6, 1e-6), _translate(1e17, -1e17, 1e17), _translate(3e18, 0.0, 0.0)]
    return np.stack(t).astype(np.float32)


@pytest.mark.gpu
@pytest.mark.parametrize("faces", [1, 2, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097, 9000])
def test_instance_bounds_kernels_match_the_host_form_at_every_edge(gi, faces):
    v, f = _soup(faces, 100 + faces)
    xf = _shape_transforms()
    differing, boxes, status = capi.debug_instance_bounds(v, f, xf)
    print(f"{faces} faces: differing {differing}, status {status.tolist()}")
    assert differing == 0
    assert status[:7].tolist() == [0] * 7 and status[7] != 0  # only the translation beyond 1e18 leaves the usable range
    p = v["pos"].astype(np.float64)
    for k in range(len(xf)):
        q = p @ xf[k, :3, :3].astype(np.float64) + xf[k, 3, :3].astype(np.float64)  # the float64-transformed corners
        assert np.all(boxes[k, :3].astype(np.float64) <= q.min(axis=0)) and np.all(boxes[k, 3:].astype(np.float64) >= q.max(axis=0)), (faces, k, boxes[k], q.min(axis=0), q.max(axis=0))
    # one NaN vertex: every transform reports it
    v2 = v.copy(); v2["pos"][len(v2) // 2, 1] = np.nan
    differing, _, status = capi.debug_instance_bounds(v2, f, xf)
    assert differing == 0 and np.all(status != 0), (faces, differing, status)


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# declines
# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
def _expect_rebuild(orc, sc, key, full, tlas, oracle_desc=None):
    """`oracle_desc`: the scene the library renders written with ordinary geometry (tests/test_hostile_inputs.py sanitised), where the description holds an
    unusable instance -- the oracle takes no hostile input."""
    img = sc.render(RS, W, H)
    assert sc.update_counts()["full"] == full and sc.tlas_update_count() == tlas and sc.update_counts()["transform"] == 0, (key, sc.update_counts(), sc.tlas_update_count())
    assert sc.stats()["bvhBuildMs"] > 0.0
    assert _bits_equal(img, _fresh_image(sc.desc)), f"{key}: differs from a scene built from scratch"
    assert _bits_equal(img, _oracle(orc, key, oracle_desc if oracle_desc is not None else sc.desc)[0]), f"{key}: differs from the oracle"


def _expect_update(orc, sc, key, full, tlas):
    t = _instances(sc.desc, A); t[0] = t[0] @ _translate(0.05, 0.0, 0.05)
    sc.set_mesh_instance_transforms(A, t)
    img = sc.render(RS, W, H)
    assert sc.update_counts() == {"full": full, "transform": 0, "material": 0} and sc.tlas_update_count() == tlas, (key, sc.update_counts(), sc.tlas_update_count())
    assert sc.tlas_check() == 0 and sc.tlas_check().two_level == 1
    assert _bits_equal(img, _fresh_image(sc.desc)), f"{key}: differs from a scene built from scratch"


@pytest.mark.gpu
def test_instance_pushed_beyond_the_usable_range_rebuilds(gi, orc):
    sc = _make()
    start = copy.deepcopy(sc.desc)
    try:
        sc.render(RS, W, H)
        t = _instances(sc.desc, B); t[2] = t[2] @ _translate(0.0, 4e18, 0.0)
        sc.set_mesh_instance_transforms(B, t)
        _expect_rebuild(orc, sc, "tl-beyond-the-range", 2, 0)  # (a fresh build of this scene keeps the flat layout: its triangles there are inactive)
        assert sc.tlas_check().two_level == 0 and sc.stats()["inactiveTriangleCount"] == 320
        sc.set_mesh_instance_transforms(B, _instances(start, B))  # back: the resident scene is a flat one now, and its transform path takes the edit
        img = sc.render(RS, W, H)
        assert sc.update_counts() == {"full": 2, "transform": 1, "material": 0} and sc.tlas_update_count() == 0, sc.update_counts()
        assert _bits_equal(img, _fresh_image(sc.desc)) and _bits_equal(img, _oracle(orc, "start", sc.desc)[0])
    finally:
        sc.close()


@pytest.mark.gpu
def test_non_invertible_instance_transform_rebuilds(gi, orc):
    sc = _make()
    start = copy.deepcopy(sc.desc)
    try:
        sc.render(RS, W, H)
        t = _instances(sc.desc, MOVED); t[0] = _scale(1.0, 0.0, 1.0) @ t[0]
        sc.set_mesh_instance_transforms(MOVED, t)
        _expect_rebuild(orc, sc, "tl-singular", 2, 0, oracle_desc=sanitised(sc.desc))
        assert sc.tlas_check().two_level == 1 and sc.stats()["inactiveTriangleCount"] == 320  # (its triangles are inactive; the layout stays)
        sc.set_mesh_instance_transforms(MOVED, _instances(start, MOVED))
        _expect_rebuild(orc, sc, "start", 3, 0)  # (the resident scene held the singular instance's triangles as inactive ones)
        _expect_update(orc, sc, "tl-singular-after", 3, 1)
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
        assert sc.tlas_check().two_level == 1
        t = _instances(sc.desc, A); t[0] = t[0] @ _translate(0.1, 0.0, 0.1)
        sc.set_mesh_instance_transforms(A, t)
        _expect_rebuild(orc, sc, "tl-below-the-floor", 2, 0)
    finally:
        sc.close()


@pytest.mark.gpu
def test_incremental_0_rebuilds(gi, orc, monkeypatch):
    sc = _make()
    try:
        sc.render(RS, W, H)
        monkeypatch.setenv("GATLING_OPTIONS", "incremental=0")
        t = _instances(sc.desc, A); t[1] = t[1] @ _translate(0.1, 0.05, 0.1)
        sc.set_mesh_instance_transforms(A, t)
        _expect_rebuild(orc, sc, "tl-incremental-0", 2, 0)
        monkeypatch.delenv("GATLING_OPTIONS")
        _expect_update(orc, sc, "tl-incremental-0-after", 2, 1)
    finally:
        sc.close()


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# composition: a material edit in the same render, the look-ahead window, giCTraceRays
# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_material_replacement_and_move_compose_in_one_render(gi, orc):
    sc = _make()
    try:
        sc.render(RS, W, H)
        m = copy.deepcopy(sc.desc.materials[DIFFUSE_MATERIAL]); m.params[0:3] = np.float32([0.9, 0.1, 0.4])
        sc.replace_material(DIFFUSE_MATERIAL, m)
        sc.set_mesh_material(REASSIGNED, DIFFUSE_MATERIAL)  # (a mesh's word changes: InstTrav::matFlags of its instances with it)
        t = _instances(sc.desc, REASSIGNED); t[0] = t[0] @ _translate(0.1, 0.1, -0.1)
        sc.set_mesh_instance_transforms(REASSIGNED, t)
        got = sc.render_aovs(RS, W, H, AOVS)
        assert sc.update_counts() == {"full": 1, "transform": 0, "material": 1} and sc.tlas_update_count() == 1, (sc.update_counts(), sc.tlas_update_count())
        assert sc.tlas_check() == 0 and sc.validate_bvh()["violations"] == 0
        _check(orc, sc, "tl-material-and-move", got)
    finally:
        sc.close()


@pytest.mark.gpu
def test_move_discards_the_look_ahead_window(gi, orc):
    rs = RenderSettings(spp=1, max_bounces=3, next_event_estimation=True)  # progressive
    sc = _make()
    try:
        sc.set_option(capi.OPTION_SAMPLE_LOOKAHEAD, 4)
        for _ in range(5):  # windows of 1 and 2; the fourth call traces a window of 4, the fifth is served from it
            sc.render(rs, W, H)
        la = sc.lookahead_stats()
        assert (la["windowCalls"], la["windowServed"], la["traced"]) == (4, 2, 0) and la["windowsDiscarded"] == 0, la
        t = _instances(sc.desc, MOVED); t[1] = t[1] @ _translate(0.3, 0.1, -0.2)
        sc.set_mesh_instance_transforms(MOVED, t)  # in the middle of the window: two of its four calls were never asked for
        img = sc.render(rs, W, H)
        la2 = sc.lookahead_stats()
        assert la2["windowsDiscarded"] == 1 and la2["samplesUnused"] == 2 and la2["traced"] == 1, la2
        assert sc.update_counts() == {"full": 1, "transform": 0, "material": 0} and sc.tlas_update_count() == 1
        ref, _ = orc.render(sc.desc, rs, W, H, threads=8)  # the accumulation restarted: the oracle's first frame of the scene after the move
        assert _bits_equal(img, ref)
    finally:
        sc.close()


@pytest.mark.gpu
def test_trace_rays_after_a_move_answers_like_a_fresh_scene(gi):
    rng = np.random.default_rng(77)
    origins = np.tile(np.float32([0.0, 1.2, 0.0]), (256, 1)) + rng.uniform(-0.3, 0.3, (256, 3)).astype(np.float32)
    dirs = rng.normal(size=(256, 3)); dirs = (dirs / np.linalg.norm(dirs, axis=1, keepdims=True)).astype(np.float32)
    sc = _make()
    try:
        sc.render(RS, W, H)
        before = sc.trace_rays(origins, dirs)
        _s1(sc, None); _s2(sc, None); _s4(sc, None)
        sc.render(RS, W, H)
        assert sc.update_counts()["full"] == 1 and sc.tlas_update_count() == 1
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
        assert moved, "no ray met what moved"
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
    import test_tlas_edits as T
    L = capi.initialize(0)                      # $GATLING_DEVICES = "0,0": two contexts on the one GPU
    assert L.giCGetDeviceCount() == 2
    multi = T._make()
    single = T._make(); single.set_option(capi.OPTION_DEVICES, 1)
    start = copy.deepcopy(multi.desc)
    for sc in (multi, single):
        sc.render_aovs(T.RS, T.W, T.H, T.AOVS)
    for step, edit in T.SEQUENCE:
        out = []
        for sc in (multi, single):
            edit(sc, start)
            out.append(sc.render_aovs(T.RS, T.W, T.H, T.AOVS))
        for k in out[0]:
            assert T._bits_equal(out[0][k], out[1][k]), step + ": " + k + " differs between two device contexts and one"
        T._resident_checks(multi, step, devices=(0, 1))
        assert multi.validate_bvh(0)["digest"] == multi.validate_bvh(1)["digest"] == single.validate_bvh(0)["digest"], step
    assert multi.update_counts() == {"full": 1, "transform": 0, "material": 0} and multi.tlas_update_count() == len(T.SEQUENCE)
    fresh = capi.Scene(copy.deepcopy(multi.desc)); fresh.set_option(capi.OPTION_DEVICES, 1)
    ref = fresh.render_aovs(T.RS, T.W, T.H, T.AOVS)
    for k in ref:
        assert T._bits_equal(out[0][k], ref[k]), k + " differs from a scene built from scratch"
    multi.close(); single.close(); fresh.close()
    print("two contexts ok")
""")


@pytest.mark.gpu
def test_transform_edits_reach_every_device_context():
    env = dict(os.environ); env["GATLING_DEVICES"] = "0,0"
    out = subprocess.run([sys.executable, "-c", TWO_CONTEXTS % {"root": ROOT, "tests": os.path.join(ROOT, "tests")}], capture_output=True, text=True, timeout=300,
                         env=env)
    assert out.returncode == 0 and "two contexts ok" in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# random sequences
# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
def _random_local(rng):
    """A change of an instance where it stands: a rotation and a scale in [0.5, 2] per axis."""
    return _scale(*rng.uniform(0.5, 2.0, 3)) @ _rotation(rng.normal(size=3) + 1e-3, rng.uniform(0.0, 2.0 * np.pi))


def _random_edit(rng, sc, start):
    d = sc.desc
    kind = int(rng.choice(4, p=np.float64([3, 2, 2, 1]) / 8.0))
    clutter = [i for i, m in enumerate(d.meshes) if m.name.startswith("/Clutter")]
    mi = int(rng.choice(clutter))
    if kind == 0:  # one instance
        t = _instances(d, mi); k = int(rng.integers(len(t)))
        t[k] = (_random_local(rng) @ t[k]) @ _translate(*rng.uniform(-2.0, 2.0, 3))
        sc.set_mesh_instance_transforms(mi, t); return "instance"
    if kind == 1:  # a whole mesh
        sc.set_mesh_transform(mi, _transform(d, mi) @ _translate(*rng.uniform(-2.0, 2.0, 3))); return "mesh"
    if kind == 2:  # a material edit, alone or with a move
        mat = int(rng.integers(len(d.materials)))
        m = copy.deepcopy(d.materials[mat]); m.params[0:3] = rng.uniform(0.05, 0.95, 3).astype(np.float32)
        sc.replace_material(mat, m)
        if rng.integers(2):
            sc.set_mesh_transform(mi, _transform(d, mi) @ _translate(*rng.uniform(-0.5, 0.5, 3))); return "material+mesh"
        return "material"
    for i in clutter:  # undo: every transform back to the start's
        sc.set_mesh_instance_transforms(i, _instances(start, i)); sc.set_mesh_transform(i, _transform(start, i))
    return "undo"


def _description_is_usable(desc):
    """The instance boxes of the description, on the CPU: every transformed corner finite and far inside the usable range (1e18), every instance transform
    invertible with a finite inverse in fp32 -- nothing an update declines for."""
    for m in desc.meshes:
        p = np.asarray(m.vertices["pos"], np.float32)
        prim = np.asarray(m.transform, np.float32).reshape(4, 4)
        for inst in np.asarray(m.instance_transforms, np.float32).reshape(-1, 4, 4):
            xf = prim @ inst
            q = p @ xf[:3, :3] + xf[3, :3]
            lo, hi = q.min(axis=0), q.max(axis=0)
            det = np.linalg.det(xf[:3, :3].astype(np.float64))
            if not (np.all(np.isfinite(q)) and np.all(np.abs(lo) < 1e6) and np.all(np.abs(hi) < 1e6) and abs(det) > 1e-6):
                return False
    return True


@pytest.mark.gpu
def test_random_edit_sequences_match_the_oracle(gi, orc):
    """20 sequences of six random edits each -- moves of single instances, moves of whole meshes, material edits, undo -- with the option on; every render is
    compared with the oracle's render of the description at that point.  The drawn transforms (translations up to 2 units, rotations, scales in [0.5, 2]) keep
    every instance usable, which is checked here on the description's own boxes before every render.  The depth rule (2 x TLAS depth + BLAS depth + 1 <= 16) is
    out of reach of 21 instance boxes in a room of a few units -- the 1 024 instances of config C4 build a TLAS of 4 levels, the 13 225 of the 67.7 M-triangle
    scene one of 5.  So no drawn case may decline: the scene's first build must stay its only one, which is asserted."""
    rs = RenderSettings(spp=1, max_bounces=3, next_event_estimation=True, progressive_accumulation=False)
    rng = np.random.default_rng(20261)
    kinds, updates, materials = {}, 0, 0
    for seq in range(20):
        sc = _make()
        start = copy.deepcopy(sc.desc)
        try:
            sc.render(rs, W, H)
            for k in range(6):
                kind = _random_edit(rng, sc, start)
                kinds[kind] = kinds.get(kind, 0) + 1
                assert _description_is_usable(sc.desc), (seq, k, kind)
                img = sc.render(rs, W, H)
                ref, _ = orc.render(sc.desc, rs, W, H, threads=8)
                assert _bits_equal(img, ref), (seq, k, kind)
                assert sc.tlas_check() == 0, (seq, k, kind)
            c = sc.update_counts()
            assert c["full"] == 1 and c["transform"] == 0, (seq, c)
            assert sc.tlas_update_count() >= 1, (seq, kinds)
            updates += sc.tlas_update_count(); materials += c["material"]
        finally:
            sc.close()
    print("random edit sequences:", kinds, {"tlas": updates, "material": materials})
    assert materials > 0

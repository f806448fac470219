"""Mesh creations and destructions on a two-level scene without the flat tree, applied in place (gi_build.cpp updateTopologyTwoLevel,
gi_append.hip k_append_shade_index / k_append_blas_tris / k_append_records, gi_append.h): with GI_C_SCENE_OPTION_TLAS_TOPOLOGY = 20, read with option 13 wanted on
a scene built with options 2-level and 19, a giCDestroyMesh retires the mesh as a visibility update hides one and a giCCreateMesh appends the mesh -- one BLAS
from the host, everything per face and per flattened triangle made on the device.  Nothing may change in an image: colour and the nine AOVs must be
bit-identical to a scene built from scratch from the edited description and to the oracle's render.  No tolerance anywhere.

CPU: the header, the library and the harness declare the option, the counter and the hooks; the API version is unchanged; the host forms of the kernels
(giCDebugAppendRecordsHost) give the scene build's bytes on the shapes the kernels are run at; gi_append.h runs clean under the sanitizers as a program of its
own, held to a separately written restatement.
GPU: the kernels against the host at the edges of their mapping (k_append_records gives a lane one 16-byte piece, four lanes a record: a wave holds 16 items
and a block 64; the two per-face kernels give a lane a face: 64 and 256), an edit sequence with the checks after every step, the same sequence with the option
off (today's behaviour: every creation and destruction rebuilds), the declines, two device contexts, random edit sequences against the oracle.

The scene, the render settings and the helpers are those of tests/test_visibility_edits.py (6 412 flattened triangles in 21 instances of 12 meshes; mesh 1
lies in front of the cutout mesh 3, so a retire that does not renumber changes pixels); new meshes are made by tests/test_topology_edits.py's helper."""
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

import test_topology_edits as TT
from test_tlas_edits import _instances, _transform
from test_vertex_edits import _deformed
from test_visibility_edits import AOVS, CUT, CUTOUT_MATERIAL, DIFFUSE_MATERIAL, H, MOVED, RS, W, _bits_equal, _check, _lookdev_scene, _translate

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TREELESS = {"two_level": 1, "treeless": 1, "resident_nodes": 0, "host_node_bytes": 0}
EDIT_OPTIONS = ("OPTION_VISIBILITY_UPDATES", "OPTION_VERTEX_UPDATES", "OPTION_TLAS_UPDATES", "OPTION_BLAS_UPDATES", "OPTION_TLAS_VISIBILITY")  # 11, 12, 16, 17, 18
A_NAME, B_NAME, MOVED_NAME = "/Clutter/p0_m1", "/Clutter/p2_m1", "/Clutter/p0_m4"  # (looked up by name: indices shift when a mesh is destroyed)


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
def test_header_declares_the_option_and_the_hooks_and_keeps_api_version_8():
    text = open(os.path.join(ROOT, "include", "gi_c.h")).read()
    assert re.search(r"#define\s+GI_C_SCENE_OPTION_TLAS_TOPOLOGY\s+20\b", text)
    assert re.search(r"int\s+giCDebugSceneTlasTopologyUpdateCount\s*\(\s*const\s+GiCScene\s*\*\s*\w+\s*,\s*uint64_t\s*\*\s*\w+\s*\)", text)
    assert re.search(r"int\s+giCDebugAppendRecords\s*\(\s*const\s+GiCVertex\s*\*", text) and re.search(r"int\s+giCDebugAppendRecordsHost\s*\(\s*const\s+GiCVertex\s*\*", text)
    assert re.search(r"#define\s+GI_C_API_VERSION\s+8u?\b", text)


def test_library_exports_the_symbols():
    L = capi.load_library()
    assert L.giCGetApiVersion() == 8
    for name in ("giCDebugSceneTlasTopologyUpdateCount", "giCDebugAppendRecords", "giCDebugAppendRecordsHost"):
        assert hasattr(L, name), name


def test_harness_exposes_the_option_and_the_methods():
    assert capi.OPTION_TLAS_TOPOLOGY == 20
    assert callable(capi.Scene.tlas_topology_update_count) and callable(capi.debug_append_records)


def test_scene_names_are_the_ones_the_cases_are_written_for():
    d = _lookdev_scene()
    assert [TT._idx(d, n) for n in (A_NAME, MOVED_NAME, B_NAME)] == [1, MOVED, 8] and TT._tris(d, 8) == 960 and d.meshes[CUT].material == CUTOUT_MATERIAL and d.triangle_count() == 6412
    assert len(d.meshes[1].instance_transforms) == 2 and TT._tris(d, 1) == 640


# the shapes (faces, instances): one item; the edges of a wave and of a block under both mappings (16 / 64 items of four lanes each; 64 / 256 faces of one
# lane each); an instance boundary inside a wave and inside a block; several instances of a mesh larger than a block
SHAPES = [(1, 1), (15, 1), (16, 1), (17, 1), (63, 1), (64, 1), (65, 1), (255, 1), (256, 1), (257, 1), (7, 37), (300, 3)]


def _mesh(nf, seed):
    """An indexed strip of `nf` faces over nf + 2 random vertices with unit normals and tangents."""
    rng = np.random.default_rng(seed)
    nv = nf + 2
    v = np.zeros(nv, VERTEX_DTYPE)
    v["pos"] = rng.uniform(-2.0, 2.0, (nv, 3)).astype(np.float32)
    n = rng.normal(size=(nv, 3)); n /= np.linalg.norm(n, axis=1)[:, None]
    v["norm"], v["tangent"] = n.astype(np.float32), np.roll(n, 1, axis=1).astype(np.float32)
    v["u"], v["v"], v["bitangentSign"] = rng.uniform(size=nv), rng.uniform(size=nv), np.where(rng.uniform(size=nv) < 0.5, -1.0, 1.0)
    f = np.stack([np.arange(nf), np.arange(nf) + 1, np.arange(nf) + 2], 1).astype(np.uint32)
    return v, f


def _xforms(k, seed, mirrored=False):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(k):
        m = np.eye(4, dtype=np.float32)
        m[:3, :3] = (rng.uniform(-0.4, 0.4, (3, 3)) + 1.5 * np.eye(3)).astype(np.float32)
        m[3, :3] = rng.uniform(-3.0, 3.0, 3)
        if mirrored:
            m[:3, 0] *= -1.0  # negative determinant
            assert np.linalg.det(m[:3, :3].astype(np.float64)) < 0.0
        out.append(m)
    return np.stack(out)


# (name, keyword arguments): zero bases and no face ids; a mirrored transform, a flip-facing and double-sided mesh, non-zero vertex offset, shade base and id
# base, face ids with a one-byte stride; the two- and four-byte strides of the face-id AOV
def _variants(nf):
    return [("plain", dict()),
            ("mirrored-flags-bases-ids", dict(mirrored=True, face_ids=np.arange(nf) % 200, max_face_id=199, flip_facing=True, double_sided=True, vertex_offset=3, shade_base=5,
                                              id_base=1000, mat_flags=0xC1000006)),
            ("ids-two-bytes", dict(face_ids=np.arange(nf) * 7 % 60000, max_face_id=60000, vertex_offset=1, id_base=64, mat_flags=0x41000002)),
            ("ids-four-bytes", dict(face_ids=np.arange(nf) * 70001 % 2000000, max_face_id=2000000, flip_facing=True, shade_base=1, mat_flags=0x12000001))]


def _append_differs(nf, k, variant, host_only):
    kw = dict(variant)
    v, f = _mesh(nf, 100 * nf + k)
    return capi.debug_append_records(v, f, _xforms(k, nf + 7 * k, kw.pop("mirrored", False)), host_only=host_only, **kw)


@pytest.mark.parametrize("nf,k", SHAPES)
def test_host_forms_of_the_append_kernels_give_the_scene_builds_bytes(nf, k):
    for name, variant in _variants(nf):
        assert _append_differs(nf, k, variant, host_only=True) == 0, (nf, k, name)


def test_append_forms_run_clean_under_the_sanitizers(tmp_path):
    # (the sanitizer runtimes are linked statically: the program stands alone whatever else the process environment loads)
    exe = str(tmp_path / "append_records_sanitize")
    csrc = os.path.join(ROOT, "gatling_amd", "csrc")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-I", csrc, "-I",
           os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "append_records_sanitize.cpp"), "-o", exe]
    probe = subprocess.run(["g++", "-fsanitize=address,undefined", "-static-libasan", "-static-libubsan", "-x", "c++", "-", "-o", str(tmp_path / "probe")], input="int main(){return 0;}", text=True,
                           capture_output=True)
    if probe.returncode != 0:
        pytest.skip("the toolchain has no sanitizer runtimes")
    built = subprocess.run(cmd, capture_output=True, text=True)
    assert built.returncode == 0, built.stderr[-4000:]
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "append records sanitize ok" in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# GPU: the kernels against the host
# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("nf,k", SHAPES)
def test_append_kernels_give_the_scene_builds_bytes(gi, nf, k):
    for name, variant in _variants(nf):
        assert _append_differs(nf, k, variant, host_only=False) == 0, (nf, k, name)


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# GPU: scenes
# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
def _make(option_on=True, tlas_only=True, desc=None):
    sc = capi.Scene(desc if desc is not None else _lookdev_scene())
    sc.set_option(capi.OPTION_TWO_LEVEL, 1)
    if tlas_only:
        sc.set_option(capi.OPTION_TLAS_ONLY, 1)
    sc.set_option(capi.OPTION_TOPOLOGY_UPDATES, 1)
    if option_on:
        sc.set_option(capi.OPTION_TLAS_TOPOLOGY, 1)
    for name in EDIT_OPTIONS:
        sc.set_option(getattr(capi, name), 1)
    return sc


def _own_counters(sc):
    return {"topology": sc.tlas_topology_update_count(), "tlas": sc.tlas_update_count(), "blas": sc.blas_update_count(), "visibility": sc.tlas_visibility_update_count()}


def _resident_checks(sc, key, devices=(0,), deformed=False):
    """What every step asserts of the resident scene: no flat tree, the two-level arrays a fresh build's in storage order (blas_check once a mesh's points are not
    the build's: its BLAS is then a refitted one), the flat records' ids and the id table, the visible count."""
    st = sc.stats()
    assert st["nodeCount"] == 0, (key, st)
    visible = sum(len(m.faces) * len(m.instance_transforms) for m in sc.desc.meshes if m.visible)
    for d in devices:
        assert sc.flat_tree_state(d) == TREELESS, (key, d, sc.flat_tree_state(d))
        b, f = sc.blas_check(d), sc.flat_id_check(d)
        assert b == 0 and b.two_level == 1, (key, d, "blas_check", int(b), b.violations)
        if not deformed:
            c = sc.tlas_check(d)
            assert c == 0 and c.two_level == 1, (key, d, "tlas_check", int(c))
        assert f == 0 and f.two_level == 1 and f.resident_tris == st["triangleCount"] and f.visible_tris == visible, (key, d, int(f), f.visible_tris, visible, f.resident_tris)


def _new(sc, name, like, material, places, mesh_id, seed=5):
    return sc.create_mesh(TT._new_mesh(sc.desc, name, like, material, places, mesh_id, seed))


def _e1(sc):
    sc.destroy_mesh(TT._idx(sc, A_NAME))


def _e2(sc):
    _new(sc, "/New/diffuse", MOVED, DIFFUSE_MATERIAL, [(-1.0, -0.5, 1.1, 0.45), (1.2, 0.4, 1.4, 0.35)], 100)


def _e3(sc):
    _new(sc, "/New/cutout", CUT, CUTOUT_MATERIAL, [(0.4, -1.0, 1.0, 0.4)], 101, seed=6)


def _e4(sc):
    sc.destroy_mesh(TT._idx(sc, B_NAME))
    _new(sc, "/New/third", 10, 3, [(-2.0, 1.0, 1.2, 0.3), (2.2, -1.4, 0.8, 0.3), (0.0, 0.0, 2.0, 0.25)], 102, seed=7)


def _e5(sc):
    sc.destroy_mesh(TT._idx(sc, "/New/cutout"))


def _e6(sc):
    i = TT._idx(sc, "/New/third")
    sc.set_mesh_vertices(i, _deformed(sc.desc.meshes[i].vertices, 0.04, 31))


def _e7(sc):
    i = TT._idx(sc, "/New/diffuse")
    t = _instances(sc.desc, i); t[1] = t[1] @ _translate(0.3, 0.1, -0.2)
    sc.set_mesh_instance_transforms(i, t)
    j = TT._idx(sc, "/New/third")
    sc.set_mesh_transform(j, _transform(sc.desc, j) @ _translate(-0.1, 0.2, 0.05))


def _e8(sc):
    sc.set_mesh_visibility(TT._idx(sc, "/New/diffuse"), False)


def _e9(sc):
    sc.set_mesh_visibility(TT._idx(sc, "/New/diffuse"), True)


def _e10(sc):
    m = copy.deepcopy(sc.desc.materials[2]); m.params[0:3] = (0.9, 0.1, 0.6)
    sc.replace_material(2, m)  # destroyed and created: a new material, at the end of the library's table
    _new(sc, "/New/recoloured", MOVED, 2, [(0.3, -1.2, 0.9, 0.4)], 103, seed=8)


# (name, edit, the counter of its own that rises by one, a material update rides along, a mesh's points are no longer the build's from here on)
SEQUENCE = [("1-destroy-A", _e1, "topology", False, False), ("2-create-diffuse-two-instances", _e2, "topology", False, False), ("3-create-cutout", _e3, "topology", False, False),
            ("4-destroy-and-create", _e4, "topology", False, False), ("5-destroy-appended", _e5, "topology", False, False), ("6-deform-appended", _e6, "blas", False, True),
            ("7-move-appended", _e7, "tlas", False, True), ("8-hide-appended", _e8, "visibility", False, True), ("9-show-appended", _e9, "visibility", False, True),
            ("10-replace-material-and-create", _e10, "topology", True, True)]


def _run_sequence(orc, option_on):
    sc = _make(option_on)
    outputs = []
    try:
        first = sc.render_aovs(RS, W, H, AOVS)
        assert sc.update_counts()["full"] == 1 and _own_counters(sc) == {"topology": 0, "tlas": 0, "blas": 0, "visibility": 0}
        _check(orc, sc, "tlas-topology start", first)
        _resident_checks(sc, "start")
        for step, edit, counter, with_material, deformed in SEQUENCE:
            before, own_before = sc.update_counts(), _own_counters(sc)
            edit(sc)
            got = sc.render_aovs(RS, W, H, AOVS)
            st, after, own_after = sc.stats(), sc.update_counts(), _own_counters(sc)
            print(f"option {int(option_on)} {step}: bvhBuildMs {st['bvhBuildMs']:.3f} uploadMs {st['uploadMs']:.3f} counts {after} own {own_after} resident {st['triangleCount']}")
            if option_on or counter != "topology":  # in place: the counter of its own rises, nothing is built in full
                assert after["full"] == before["full"], (step, after)
                assert own_after == {k: v + int(k == counter) for k, v in own_before.items()}, (step, own_before, own_after)
                assert after["material"] == before["material"] + int(with_material), (step, after)
                assert st["triangleCount"] >= sc.desc.triangle_count()  # what is resident: retired triangles included
            else:  # today's behaviour: every creation and destruction rebuilds
                assert after["full"] == before["full"] + 1 and own_after["topology"] == 0, (step, after, own_after)
                assert st["triangleCount"] == sc.desc.triangle_count()
            assert sc.topology_update_count() == 0  # (the flat path's counter keeps counting what it counted)
            _resident_checks(sc, step, deformed=deformed)
            _check(orc, sc, "tlas-topology " + step, got)
            outputs.append(got)
    finally:
        sc.close()
    return outputs


_sequence_outputs = {}


@pytest.mark.gpu
def test_creations_and_destructions_are_applied_in_place_bit_exactly(gi, orc):
    _sequence_outputs[True] = _run_sequence(orc, True)


@pytest.mark.gpu
def test_with_the_option_off_the_same_edits_rebuild_and_give_the_same_bits(gi, orc):
    _sequence_outputs[False] = _run_sequence(orc, False)
    if True in _sequence_outputs:
        for (step, *_), on, off in zip(SEQUENCE, _sequence_outputs[True], _sequence_outputs[False]):
            for k in on:
                assert _bits_equal(on[k], off[k]), f"{step}: {k} differs between the option on and off"


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# declines: each renders correctly through a counted full build
# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
def _fresh_image(desc):
    fresh = capi.Scene(copy.deepcopy(desc))
    try:
        return fresh.render(RS, W, H)
    finally:
        fresh.close()


def _expect_rebuild(sc, key, full, topology, orc=None):
    img = sc.render(RS, W, H)
    assert sc.update_counts()["full"] == full and sc.tlas_topology_update_count() == topology, (key, sc.update_counts(), sc.tlas_topology_update_count())
    assert sc.stats()["triangleCount"] == sum(len(m.faces) * len(m.instance_transforms) for m in sc.desc.meshes if m.visible), (key, sc.stats())
    assert _bits_equal(img, _fresh_image(sc.desc)), f"{key}: differs from a scene built from scratch"
    if orc is not None:
        assert _bits_equal(img, orc.render(sc.desc, RS, W, H, threads=8)[0]), f"{key}: differs from the oracle"


def _expect_update(sc, key, full, topology):
    img = sc.render(RS, W, H)
    assert sc.update_counts()["full"] == full and sc.tlas_topology_update_count() == topology, (key, sc.update_counts(), sc.tlas_topology_update_count())
    assert _bits_equal(img, _fresh_image(sc.desc)), f"{key}: differs from a scene built from scratch"


@pytest.mark.gpu
def test_two_level_scene_with_a_flat_tree_declines(gi, orc):
    sc = _make(tlas_only=False)
    try:
        sc.render(RS, W, H)
        assert sc.flat_tree_state()["treeless"] == 0
        _e1(sc); _e2(sc)
        _expect_rebuild(sc, "flat-tree", 2, 0, orc)
    finally:
        sc.close()


@pytest.mark.gpu
def test_incremental_switched_off_declines(gi, orc, monkeypatch):
    sc = _make()
    try:
        sc.render(RS, W, H)
        monkeypatch.setenv("GATLING_OPTIONS", "incremental=0")
        _e1(sc); _e2(sc)
        _expect_rebuild(sc, "incremental=0", 2, 0, orc)
    finally:
        sc.close()


@pytest.mark.gpu
def test_option_through_the_environment_wins(gi, monkeypatch):
    on, off = _make(option_on=False), _make(option_on=True)
    try:
        for sc in (on, off):
            sc.render(RS, W, H)
            _e1(sc)
        monkeypatch.setenv("GATLING_OPTIONS", "tlas_topology=1")
        _expect_update(on, "environment on", 1, 1)
        monkeypatch.setenv("GATLING_OPTIONS", "tlas_topology=0")
        _expect_rebuild(off, "environment off", 2, 0)
    finally:
        on.close(); off.close()


@pytest.mark.gpu
def test_destroying_below_the_triangle_floor_declines(gi, orc):
    sc = _make()
    try:
        sc.render(RS, W, H)
        for name in (A_NAME, B_NAME):
            sc.destroy_mesh(TT._idx(sc, name))
        _expect_update(sc, "destroy-A-B", 1, 1)
        _resident_checks(sc, "destroy-A-B")
        sc.destroy_mesh(TT._idx(sc, MOVED_NAME))
        assert sc.desc.triangle_count() < 4096
        _expect_rebuild(sc, "below-the-floor", 2, 1, orc)
    finally:
        sc.close()


@pytest.mark.gpu
def test_more_retired_than_live_triangles_declines_and_the_rebuild_compacts(gi, orc):
    """Every destroy + create of mesh B retires 960 triangles.  6 412 live: six stay in place (5 760 retired), the seventh (6 720) rebuilds, and the rebuild holds
    the live triangles alone."""
    sc = _make()
    try:
        sc.render(RS, W, H)
        for k in range(6):
            TT._resync(sc, B_NAME, 20 + k)
            sc.render(RS, W, H)
            assert sc.update_counts()["full"] == 1 and sc.tlas_topology_update_count() == k + 1 and sc.stats()["triangleCount"] == 6412 + 960 * (k + 1)
        _resident_checks(sc, "six resyncs")
        TT._resync(sc, B_NAME, 26)
        _expect_rebuild(sc, "seventh-resync", 2, 6, orc)
        assert sc.stats()["triangleCount"] == sc.desc.triangle_count() == 6412
    finally:
        sc.close()


@pytest.mark.gpu
def test_new_mesh_with_a_vertex_that_is_not_finite_declines(gi):
    sc = _make()
    try:
        sc.render(RS, W, H)
        md = TT._new_mesh(sc.desc, "/New/hostile", MOVED, DIFFUSE_MATERIAL, [(0.3, -1.2, 0.9, 0.4)], 100)
        md.vertices["pos"][5, 1] = np.nan
        sc.create_mesh(md)
        img = sc.render(RS, W, H)
        assert sc.update_counts()["full"] == 2 and sc.tlas_topology_update_count() == 0
        assert _bits_equal(img, _fresh_image(sc.desc)), "differs from a scene built from scratch"
    finally:
        sc.close()


@pytest.mark.gpu
def test_new_instance_with_a_singular_transform_declines(gi):
    sc = _make()
    try:
        sc.render(RS, W, H)
        md = TT._new_mesh(sc.desc, "/New/flat", MOVED, DIFFUSE_MATERIAL, [(0.3, -1.2, 0.9, 0.4), (1.0, 1.0, 1.0, 0.3)], 100)
        md.instance_transforms[1][2, :3] = 0.0  # a row of zeros: no inverse
        sc.create_mesh(md)
        img = sc.render(RS, W, H)
        assert sc.update_counts()["full"] == 2 and sc.tlas_topology_update_count() == 0
        assert _bits_equal(img, _fresh_image(sc.desc)), "differs from a scene built from scratch"
    finally:
        sc.close()


@pytest.mark.gpu
def test_new_mesh_in_front_of_a_built_one_declines(gi, orc):
    """A mesh created invisible is left out, as a fresh build leaves it out; shown after another mesh was appended, it lies in front of a built mesh."""
    sc = _make()
    try:
        sc.render(RS, W, H)
        hidden = TT._new_mesh(sc.desc, "/New/hidden", CUT, CUTOUT_MATERIAL, [(-1.0, -0.5, 1.1, 0.45)], 100)
        hidden.visible = False
        sc.create_mesh(hidden)
        _new(sc, "/New/behind", MOVED, 3, [(0.3, -1.2, 0.9, 0.4)], 101, seed=6)
        _expect_update(sc, "invisible-and-behind", 1, 1)
        _resident_checks(sc, "invisible-and-behind")
        sc.set_mesh_visibility(TT._idx(sc, "/New/hidden"), True)
        _expect_rebuild(sc, "shown", 2, 1, orc)
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
    import test_tlas_topology_edits as T
    L = capi.initialize(0)                      # $GATLING_DEVICES = "0,0": two contexts on the one GPU
    assert L.giCGetDeviceCount() == 2
    multi = T._make()
    single = T._make(); single.set_option(capi.OPTION_DEVICES, 1)
    for sc in (multi, single):
        sc.render_aovs(T.RS, T.W, T.H, T.AOVS)
    T._resident_checks(multi, "start", devices=(0, 1))
    for step, edit, counter, with_material, deformed in T.SEQUENCE:
        out = []
        for sc in (multi, single):
            edit(sc)
            out.append(sc.render_aovs(T.RS, T.W, T.H, T.AOVS))
        for k in out[0]:
            assert T._bits_equal(out[0][k], out[1][k]), step + ": " + k + " differs between two device contexts and one"
        T._resident_checks(multi, step, devices=(0, 1), deformed=deformed)
        T._resident_checks(single, step, deformed=deformed)
    assert multi.update_counts() == single.update_counts() == {"full": 1, "transform": 0, "material": 1}
    assert T._own_counters(multi) == T._own_counters(single) == {"topology": 6, "tlas": 1, "blas": 1, "visibility": 2}
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
# random edit sequences
# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
RANDOM_SEEDS = [20000, 20001, 20002, 20004, 20006, 20009, 20011, 20013]  # (chosen so that no drawn sequence reaches a decline: the CPU test below holds that)
RANDOM_EDITS = 6


def _draw_edits(seed):
    """The edit list of one sequence, drawn from the seed alone against a shadow of the description: (kind, arguments) per edit and whether the sequence reaches a
    decline -- fewer than 4 096 visible triangles, or more retired than live ones -- before its last edit.  Meshes are named: indices shift.  Moves, deforms and
    hides are drawn among visible meshes (options 16 and 17 decline an edit of a hidden mesh, and a deform beside a toggle rebuilds: one kind per edit)."""
    rng = np.random.default_rng(seed)
    d = _lookdev_scene()
    meshes = {m.name: [len(m.faces) * len(m.instance_transforms), True] for m in d.meshes if m.name.startswith("/Clutter")}  # name -> [triangles, visible]
    room = d.triangle_count() - sum(t for t, _ in meshes.values())
    retired, serial, edits, declines_at = 0, 0, [], None
    source_tris = {m.name: len(m.faces) for m in d.meshes}
    for k in range(RANDOM_EDITS):
        visible_names = sorted(n for n, (_, vis) in meshes.items() if vis)
        hidden_names = sorted(n for n, (_, vis) in meshes.items() if not vis)
        kinds = ["create", "create", "material"] + (["destroy", "destroy", "move", "deform", "hide"] if len(visible_names) > 1 else []) + (["show"] if hidden_names else [])  # (creations and destructions twice as likely)
        kind = kinds[int(rng.integers(len(kinds)))]
        if kind == "create":
            live_names = sorted(meshes)  # (the geometry of a mesh the scene holds at that time)
            like, count = live_names[int(rng.integers(len(live_names)))], int(rng.integers(1, 4))
            places = [(float(rng.uniform(-2, 2)), float(rng.uniform(-1.5, 1.5)), float(rng.uniform(0.6, 2.0)), float(rng.uniform(0.2, 0.45))) for _ in range(count)]
            name = f"/New/r{serial}"; serial += 1
            edits.append((kind, (name, like, int(rng.integers(1, 10)), places, 200 + serial, int(rng.integers(1000)))))
            meshes[name] = [source_tris[like] * count, True]; source_tris[name] = source_tris[like]
        elif kind == "material":
            edits.append((kind, (int(rng.integers(1, 5)), tuple(float(x) for x in rng.uniform(0.1, 0.9, 3)))))
        else:
            pool = hidden_names if kind == "show" else visible_names
            name = pool[int(rng.integers(len(pool)))]
            edits.append((kind, (name, int(rng.integers(1000)))))
            if kind == "destroy":
                retired += meshes.pop(name)[0]
            elif kind in ("hide", "show"):
                meshes[name][1] = kind == "show"
        live = room + sum(t for t, _ in meshes.values())
        visible = room + sum(t for t, vis in meshes.values() if vis)
        if (visible < 4096 or retired > live) and declines_at is None:
            declines_at = k
    return edits, declines_at


def _apply(sc, kind, args):
    if kind == "create":
        name, like, material, places, mesh_id, seed = args
        _new(sc, name, like, material, places, mesh_id, seed)
    elif kind == "material":
        index, colour = args
        m = copy.deepcopy(sc.desc.materials[index]); m.params[0:3] = colour
        sc.replace_material(index, m)
    else:
        name, seed = args
        i = TT._idx(sc, name)
        if kind == "destroy":
            sc.destroy_mesh(i)
        elif kind == "move":
            rng = np.random.default_rng(seed)
            sc.set_mesh_transform(i, _transform(sc.desc, i) @ _translate(*rng.uniform(-0.2, 0.2, 3)))
        elif kind == "deform":
            sc.set_mesh_vertices(i, _deformed(sc.desc.meshes[i].vertices, 0.03, seed))
        else:
            sc.set_mesh_visibility(i, kind == "show")


def test_no_random_sequence_reaches_a_decline_before_its_last_edit():
    kinds = set()
    for seed in RANDOM_SEEDS:
        edits, declines_at = _draw_edits(seed)
        assert declines_at is None or declines_at == RANDOM_EDITS - 1, (seed, declines_at, [k for k, _ in edits])
        kinds |= {k for k, _ in edits}
    assert kinds == {"create", "destroy", "move", "deform", "hide", "show", "material"}, kinds


_random_full_builds = {}


def _run_random(seq, orc):
    """One drawn sequence: every frame against a scene built from scratch and -- with `orc` -- the oracle, the checks after every edit.  Returns the full builds
    behind the first."""
    rs = RenderSettings(spp=2, max_bounces=3, next_event_estimation=True, progressive_accumulation=False)
    w, h = 48, 32
    edits, _ = _draw_edits(RANDOM_SEEDS[seq])
    sc = _make()
    try:
        sc.render(rs, w, h)
        deformed = False
        for k, (kind, args) in enumerate(edits):
            _apply(sc, kind, args)
            deformed = deformed or kind == "deform"
            got = sc.render_aovs(rs, w, h, AOVS)
            key = (seq, k, kind, args[0])
            fresh = capi.Scene(copy.deepcopy(sc.desc))
            try:
                ref = fresh.render_aovs(rs, w, h, AOVS)
            finally:
                fresh.close()
            for a in ref:
                assert _bits_equal(got[a], ref[a]), (key, a, "differs from a scene built from scratch")
            if orc is not None:
                img, _ = orc.render(sc.desc, rs, w, h, threads=8)
                assert _bits_equal(got["color"], img), (key, "colour differs from the oracle")
                oaov = orc.render_aovs(sc.desc, rs, w, h, AOVS)
                for a in AOVS:
                    assert _bits_equal(got[a], oaov[a]), (key, a, "differs from the oracle")
            _resident_checks(sc, key, deformed=deformed)
        full = sc.update_counts()["full"] - 1
        print(f"sequence {seq}: {[k for k, _ in edits]} full builds after the first {full} own counters {_own_counters(sc)}")
        return full
    finally:
        sc.close()


@pytest.mark.gpu
@pytest.mark.parametrize("seq", range(len(RANDOM_SEEDS)))
def test_random_edit_sequences_match_a_fresh_build_and_the_oracle(gi, orc, seq):
    _random_full_builds[seq] = _run_random(seq, orc)


@pytest.mark.gpu
def test_most_random_sequences_end_without_a_full_build(gi):
    """At least 6 of the 8 drawn sequences end with no full build behind the first.  The counts are those of the cases above; a sequence that did not run in this
    session is run here, without the oracle."""
    for seq in range(len(RANDOM_SEEDS)):
        if seq not in _random_full_builds:
            _random_full_builds[seq] = _run_random(seq, None)
    clean = sum(1 for v in _random_full_builds.values() if v == 0)
    assert clean >= 6, _random_full_builds

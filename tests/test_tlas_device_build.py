"""The TLAS of an edit in place built on the device (DESIGN.md section 6 "TLAS build on the device"; gi_tlas_build.hip, its host form gi_tlas_build_host.cpp, the
shared arithmetic gi_bvh_stages.h, gi_build.cpp buildEditTlas): with GI_C_SCENE_OPTION_TLAS_DEVICE_BUILD = 22 the update paths of options 16, 17, 18, 20 and 21
build their TLAS on the primary device -- Morton sort, PLOC, a cost-optimal 8-wide collapse whose depth is bounded by the 16-entry stack of the two-level walk --
instead of with the host's binned-SAH builder.  Nothing may change in an image: colour and the nine AOVs must be bit-identical to a scene built from scratch
with the option off and to the oracle's render.  No tolerance anywhere but the quality guard, which is the issue's.

CPU: the header, the options table, the library and the harness declare the option and the three entries; the API version is unchanged; the host form builds
valid trees (giCDebugBuildTlasHost: every active item once, inactive ones behind in input order, breadth-first nodes, contiguous children, every item inside
every ancestor slot, depth within the budget) over 0 .. 4 097 boxes, identical boxes, flat boxes and masked / NaN / out-of-range ones; the depth budget is
kept (2 116 boxes: four levels hold 8^4 * 3 = 12 288, three hold 1 536 -- infeasible by counting alone) and the SAH model cost stays within 1.5 x the host
builder's, far below the 2.3 - 10.6 x of a tree packed in Morton order.
GPU: the device builder's bytes are the host form's on every one of those cases, at the LDS tail's threshold (2 048 clusters) and one above, at radius 1, 16
and 64; its host waits stay within the bound that does not depend on n; edits of every kind on a 400-instance scene (one tail launch) and a 2 116-instance scene
(multi-block passes first) with the checks after every step; the budget override and the too-deep fallback; the look-ahead window; two device contexts; the
option alone and the option off; 20 random sequences."""
import copy
import os
import re
import subprocess
import sys
import textwrap

import numpy as np
import pytest

from gatling_amd import capi
from gatling_amd.scenes import sphere_grid

import test_topology_edits as T
from test_topology_edits import AOVS, H, RS, W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TAIL = 2048          # gi_tlas_build.h kTlasTailClusters
MAX_WAITS = 16 + 2   # gi_tlas_build.h kTlasMaxHostWaits: one per batch of passes (at most 16), the status, the read-back
# options 6 (two-level) and 19 (no flat tree) at the build; 11 and 12 are the switches options 17 and 18 are read with; 13, 15, 16 - 18, 20, 21: the edits in place
EDIT_OPTIONS = ("OPTION_VISIBILITY_UPDATES", "OPTION_VERTEX_UPDATES", "OPTION_TOPOLOGY_UPDATES", "OPTION_INSTANCE_UPDATES", "OPTION_TLAS_UPDATES", "OPTION_BLAS_UPDATES",
                "OPTION_TLAS_VISIBILITY", "OPTION_TLAS_TOPOLOGY", "OPTION_TLAS_INSTANCES")


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# boxes
# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
def _grid(n):
    """n unit boxes on a square grid in the xz plane, spacing 2.5, row by row."""
    k = int(np.ceil(np.sqrt(max(n, 1))))
    ij = np.array([(i, j) for i in range(k) for j in range(k)][:n], np.float32).reshape(-1, 2)
    c = np.stack([ij[:, 0] * 2.5, np.zeros(len(ij), np.float32), ij[:, 1] * 2.5], 1)
    return np.concatenate([c - 0.5, c + 0.5], 1).astype(np.float32)


def _random(n, seed=1):
    """n seeded boxes: centres uniform in a 300 x 30 x 300 volume, half-extents 0.2 - 2.2."""
    r = np.random.default_rng(seed)
    c, h = r.uniform([0, 0, 0], [300, 30, 300], (n, 3)), r.uniform(0.2, 2.2, (n, 3))
    return np.concatenate([c - h, c + h], 1).astype(np.float32)


def _flat(n):
    b = _random(n, 5)
    b[:, 4] = b[:, 1]  # zero extent in y
    return b


def _masked(n):
    """Every third box masked (gi_vispatch.h tlasMaskHiddenBoxes: the inverted box), one NaN side, one side beyond 1e18."""
    b = _random(n, 7)
    b[0::3, 0:3], b[0::3, 3:6] = 3.0e38, -3.0e38
    b[4, 2], b[10, 3] = np.nan, 2.0e18
    return b


COUNTS = [0, 1, 2, 3, 4, 9, 25, 257, 2049, 4097]
CASES = [(f"grid-{n}", lambda n=n: _grid(n)) for n in COUNTS] + [(f"random-{n}", lambda n=n: _random(n)) for n in COUNTS] + [
    ("identical-300", lambda: np.tile(_grid(1), (300, 1))), ("flat-500", lambda: _flat(500)), ("masked-400", lambda: _masked(400))]
GPU_CASES = CASES + [(f"random-{n}", lambda n=n: _random(n, 3)) for n in (TAIL, TAIL + 1)] + [("masked-4097", lambda: _masked(4097))]


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
def test_header_declares_the_option_and_the_entries_and_keeps_api_version_8():
    text = open(os.path.join(ROOT, "include", "gi_c.h")).read()
    assert re.search(r"#define\s+GI_C_SCENE_OPTION_TLAS_DEVICE_BUILD\s+22\b", text)
    for name in ("giCDebugBuildTlasHost", "giCDebugBuildTlas"):
        assert re.search(r"int\s+" + name + r"\s*\(\s*const\s+float\s*\*\s*\w+\s*,\s*uint32_t\s+\w+\s*,\s*uint32_t\s+\w+\s*,\s*uint32_t\s+\w+\s*,\s*double\s*\*", text), name
    assert re.search(r"int\s+giCDebugSceneTlasBuildStats\s*\(\s*const\s+GiCScene\s*\*\s*\w+\s*,\s*uint64_t\s+\w+\[16\]\s*\)", text)
    assert re.search(r"#define\s+GI_C_API_VERSION\s+8u?\b", text)
    comment = text[:text.index("#define GI_C_API_VERSION")]
    for name in ("GI_C_SCENE_OPTION_TLAS_DEVICE_BUILD", "giCDebugBuildTlasHost", "giCDebugBuildTlas", "giCDebugSceneTlasBuildStats"):
        assert name in comment, name  # (the additions a caller probes for are listed above the version)


def test_options_table_documents_the_overrides():
    text = open(os.path.join(ROOT, "gatling_amd", "csrc", "gi_options.h")).read()
    assert re.search(r"^//\s+tlas_device_build\s+-1\s+-1 = the scene option decides \(GI_C_SCENE_OPTION_TLAS_DEVICE_BUILD\), 0 / 1 = ", text, re.M)
    assert re.search(r"^//\s+tlas_device_min\s", text, re.M) and re.search(r"^//\s+tlas_depth_budget\s", text, re.M)


def test_library_exports_the_symbols():
    L = capi.load_library()
    assert L.giCGetApiVersion() == 8
    for name in ("giCDebugBuildTlasHost", "giCDebugBuildTlas", "giCDebugSceneTlasBuildStats"):
        assert hasattr(L, name), name


def test_harness_exposes_the_option_and_the_methods():
    assert capi.OPTION_TLAS_DEVICE_BUILD == 22
    assert callable(capi.Scene.tlas_build_stats) and callable(capi.debug_build_tlas)


def _expect_valid(r, boxes, budget):
    active = int(sum(1 for b in boxes if np.all(np.abs(b) <= 1.0e18) and np.all(b[:3] <= b[3:])))
    assert r["violations"] == 0 and r["active"] == active and 1 <= r["depth"] <= budget and r["nodes"] >= 1, r


@pytest.mark.parametrize("name,make", CASES, ids=[c[0] for c in CASES])
def test_host_form_builds_valid_trees(name, make):
    boxes = make()
    for radius in (1, 16, 64):
        _expect_valid(capi.debug_build_tlas(boxes, 7, radius, host_only=True), boxes, 7)


def test_host_form_keeps_the_depth_budget():
    r = capi.debug_build_tlas(_grid(2116), 4, 16, host_only=True)
    assert r["violations"] == 0 and r["depth"] <= 4, r
    assert capi.debug_build_tlas(_grid(2116), 3, 16, host_only=True)["violations"] == capi.TLAS_BUILD_TOO_DEEP  # three levels hold 8^3 * 3 = 1 536 < 2 116
    assert capi.debug_build_tlas(_grid(2116), 0, 16, host_only=True)["violations"] == capi.TLAS_BUILD_TOO_DEEP
    r = capi.debug_build_tlas(_grid(13225), 5, 16, host_only=True)
    assert r["violations"] == 0 and r["depth"] <= 5 and r["active"] == 13225, r


@pytest.mark.parametrize("name,make", [("grid", lambda: _grid(13225)), ("random", lambda: _random(13225))])
def test_model_cost_stays_near_the_host_builders(name, make):
    """The guard against a packing-grade tree (2.3 - 10.6 x the host builder's SAH model cost): at most 1.5 x, budget 6.  Measured: 1.263 (grid), 1.208 (random);
    at budget 5: 1.269 and 1.215."""
    r = capi.debug_build_tlas(make(), 6, 16, host_only=True)
    print(f"{name}: cost {r['cost']:.1f} / host builder {r['host_cost']:.1f} = {r['cost'] / r['host_cost']:.3f}, depth {r['depth']} / {r['host_depth']}, {r['passes']} passes")
    assert r["violations"] == 0 and r["depth"] <= 6, r
    assert r["cost"] <= 1.5 * r["host_cost"], r


def test_build_hooks_refuse_bad_arguments():
    L = capi.load_library()
    out = (capi.C.c_double * 8)()
    assert L.giCDebugBuildTlasHost(None, 3, 7, 16, out) == -1 and L.giCDebugBuildTlasHost(None, 0, 7, 16, None) == -1
    assert L.giCDebugBuildTlasHost(None, 0, 7, 16, out) == 0  # (no boxes: the empty root)
    big = np.zeros((1 << 17) + 1, np.float32)  # (a count beyond what the builder is sized for is refused before anything is read)
    assert L.giCDebugBuildTlasHost(big.ctypes.data_as(capi._FP), (1 << 17) + 1, 7, 16, out) == -1


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# GPU: the builder against its host form
# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name,make", GPU_CASES, ids=[c[0] + ("" if i < len(CASES) else "-gpu") for i, c in enumerate(GPU_CASES)])
def test_device_builder_gives_the_host_forms_bytes(gi, name, make):
    boxes = make()
    for radius in (1, 16, 64):
        r = capi.debug_build_tlas(boxes, 7, radius)
        _expect_valid(r, boxes, 7)
        assert r["host_waits"] <= MAX_WAITS, (radius, r)


@pytest.mark.gpu
def test_host_waits_do_not_grow_with_the_box_count(gi):
    """Waits of the host on the device inside one build: none per PLOC pass or level.  25 boxes: the tail launch and the emission go out blind -- the status, then
    the read-back; 4 097 boxes: one batch of multi-block passes in front of them."""
    small, large = capi.debug_build_tlas(_random(25), 7, 16), capi.debug_build_tlas(_random(4097), 7, 16)
    print(f"host waits: {small['host_waits']} at 25 boxes ({small['passes']} passes), {large['host_waits']} at 4 097 ({large['passes']} passes)")
    assert small["violations"] == 0 and large["violations"] == 0
    assert small["host_waits"] == 2 and large["host_waits"] <= 2 + 2 and large["passes"] > 20, (small, large)
    assert max(small["host_waits"], large["host_waits"]) <= MAX_WAITS


@pytest.mark.gpu
def test_device_builder_is_deterministic_and_agrees_on_too_deep(gi):
    boxes = _random(4097, 11)
    a, b = capi.debug_build_tlas(boxes, 7, 16), capi.debug_build_tlas(boxes, 7, 16)
    assert a == b and a["violations"] == 0, (a, b)  # (both runs are bytewise the host form's, so each other's)
    assert capi.debug_build_tlas(_grid(2116), 3, 16)["violations"] == capi.TLAS_BUILD_TOO_DEEP
    r = capi.debug_build_tlas(_grid(2116), 4, 16)
    assert r["violations"] == 0 and r["depth"] <= 4, r


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# GPU: scenes
# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
def _make(grid=20, option_on=True, edits=True):
    sc = capi.Scene(sphere_grid(grid, 0, 4))
    sc.set_option(capi.OPTION_TWO_LEVEL, 1)
    sc.set_option(capi.OPTION_TLAS_ONLY, 1)
    if edits:
        for name in EDIT_OPTIONS:
            sc.set_option(getattr(capi, name), 1)
    if option_on:
        sc.set_option(capi.OPTION_TLAS_DEVICE_BUILD, 1)
    return sc


def _translate(x, y, z):
    m = np.eye(4, dtype=np.float32); m[3, :3] = (x, y, z)
    return m


def _instances(sc, i):
    m = sc.desc.meshes[i]
    return np.asarray(m.instance_transforms, np.float32).reshape(-1, 4, 4).copy(), np.asarray(m.instance_ids, np.int32).copy()


def _move_instance(sc, i=1, k=17, by=(0.3, 0.2, -0.4)):
    t, _ = _instances(sc, i); t[k] = t[k] @ _translate(*by)
    sc.set_mesh_instance_transforms(i, t)


def _move_mesh(sc, i=2):
    sc.set_mesh_transform(i, np.asarray(sc.desc.meshes[i].transform, np.float32).reshape(4, 4) @ _translate(0.1, -0.3, 0.2))


def _recreate(sc, i=0):
    m = copy.deepcopy(sc.desc.meshes[i]); m.name += "/again"
    sc.destroy_mesh(i)
    sc.create_mesh(m)


def _grow(sc, i=3):
    t, ids = _instances(sc, i)
    sc.set_mesh_instance_transforms(i, np.concatenate([t, (t[-1] @ _translate(0.0, -2.0, 0.5))[None]]))
    sc.set_mesh_instance_ids(i, np.concatenate([ids, np.int32([int(ids.max()) + 1])]))


def _shrink(sc, i=3):
    t, ids = _instances(sc, i)
    sc.set_mesh_instance_transforms(i, t[:-1])
    sc.set_mesh_instance_ids(i, ids[:-1])


SEQUENCE = [("1-move-an-instance", _move_instance), ("2-move-a-mesh", _move_mesh), ("3-hide", lambda sc: sc.set_mesh_visibility(1, False)),
            ("4-show", lambda sc: sc.set_mesh_visibility(1, True)), ("5-destroy-and-create", _recreate), ("6-one-instance-more", _grow), ("7-one-instance-fewer", _shrink)]
FALLBACKS = ("too_deep", "out_of_memory", "error", "under_min")


def _resident_checks(sc, key, devices=(0,)):
    for d in devices:
        c, b, f = sc.tlas_check(d), sc.blas_check(d), sc.flat_id_check(d)
        assert c == 0 and c.two_level == 1, (key, d, "tlas_check", int(c))
        assert b == 0 and b.two_level == 1, (key, d, "blas_check", int(b))
        assert f == 0 and f.two_level == 1, (key, d, "flat_id_check", int(f))


def _step(orc, sc, key, edit, builds=1, fallback=None):
    """One edit, one render, every check: in place (no second full build), `builds` device builds more, no fallback but `fallback`, the resident arrays what the
    scene's own code makes anew, the image a fresh build's (option 22 off there) and the oracle's."""
    before = sc.tlas_build_stats()
    edit(sc)
    got = sc.render_aovs(RS, W, H, AOVS)
    after = sc.tlas_build_stats()
    print(f"{key}: {after}")
    assert sc.update_counts()["full"] == 1, (key, sc.update_counts())
    assert after["device_builds"] - before["device_builds"] == builds, (key, before, after)
    for k in FALLBACKS:
        assert after[k] - before[k] == (1 if k == fallback else 0), (key, k, before, after)
    assert after["resident_device_built"] == (1 if builds else 0), (key, after)
    _resident_checks(sc, key)
    T._check(orc, sc, "tlas-device-build " + key, got)
    return got, after


@pytest.mark.gpu
def test_edits_of_every_kind_build_their_tlas_on_the_device(gi, orc, monkeypatch):
    monkeypatch.setenv("GATLING_OPTIONS", "tlas_device_min=0")
    sc = _make()
    try:
        assert sc.desc.triangle_count() == 8000 and sum(len(m.instance_transforms) for m in sc.desc.meshes) == 400 and len(sc.desc.meshes) == 4
        sc.render(RS, W, H)
        assert sc.tlas_build_stats()["device_builds"] == 0 and sc.tlas_build_stats()["resident_device_built"] == 0  # (the scene build keeps the host builder)
        for key, edit in SEQUENCE:
            _, st = _step(orc, sc, key, edit)
            assert st["host_waits"] == 2 and 1 <= st["depth"] <= st["budget"] <= 7, (key, st)  # (400 instances: the tail alone, no batch)
        # (the workspace: the slab of the first build, and one twice its size when the re-created mesh brought the storage slots to 500 -- 501 boxes fit it)
        assert sc.tlas_build_stats()["allocations"] == 2
    finally:
        sc.close()


@pytest.mark.gpu
def test_a_scene_beyond_the_tail_threshold(gi, orc, monkeypatch):
    monkeypatch.setenv("GATLING_OPTIONS", "tlas_device_min=0")
    sc = _make(46)
    try:
        assert sum(len(m.instance_transforms) for m in sc.desc.meshes) == 2116 > TAIL
        sc.render(RS, W, H)
        _, st = _step(orc, sc, "46-move", _move_instance)
        assert 3 <= st["host_waits"] <= MAX_WAITS and st["passes"] > 10, st  # (at least one batch of multi-block passes)
    finally:
        sc.close()


@pytest.mark.gpu
def test_the_default_minimum_keeps_small_scenes_on_the_host_builder(gi, orc):
    sc = _make()
    try:
        sc.render(RS, W, H)
        _step(orc, sc, "under-min", _move_instance, builds=0, fallback="under_min")
    finally:
        sc.close()


@pytest.mark.gpu
def test_depth_budget_override_and_the_too_deep_fallback(gi, orc, monkeypatch):
    sc = _make(46)
    try:
        sc.render(RS, W, H)
        monkeypatch.setenv("GATLING_OPTIONS", "tlas_device_min=0,tlas_depth_budget=4")
        _, st = _step(orc, sc, "budget-4", _move_instance)
        assert st["depth"] <= 4 and st["budget"] == 4, st
        monkeypatch.setenv("GATLING_OPTIONS", "tlas_device_min=0,tlas_depth_budget=3")
        _step(orc, sc, "budget-3", lambda s: _move_instance(s, 2, 5), builds=0, fallback="too_deep")  # (applied in place by the host builder)
        assert sc.tlas_update_count() == 2
    finally:
        sc.close()


@pytest.mark.gpu
def test_with_the_sample_lookahead_window(gi, orc, monkeypatch):
    monkeypatch.setenv("GATLING_OPTIONS", "tlas_device_min=0")
    sc = _make()
    try:
        sc.set_option(capi.OPTION_SAMPLE_LOOKAHEAD, 4)
        sc.render(RS, W, H)
        _step(orc, sc, "lookahead-move", _move_instance)
        _step(orc, sc, "lookahead-hide", lambda s: s.set_mesh_visibility(2, False))
    finally:
        sc.close()


@pytest.mark.gpu
def test_the_option_alone_changes_nothing(gi, orc, monkeypatch):
    """Without options 16 - 21 nothing reads option 22: every edit rebuilds, as on the parent, and the counters of the device builder stay zero."""
    monkeypatch.setenv("GATLING_OPTIONS", "tlas_device_min=0")
    on, off = _make(edits=False), _make(option_on=False, edits=False)
    try:
        for sc in (on, off):
            sc.render(RS, W, H)
        for key, edit in SEQUENCE[:4]:
            out = []
            for sc in (on, off):
                edit(sc)
                out.append(sc.render_aovs(RS, W, H, AOVS))
            for k in out[0]:
                assert T._bits_equal(out[0][k], out[1][k]), (key, k)
            assert on.update_counts() == off.update_counts() and on.tlas_update_count() == off.tlas_update_count() == 0, key
            assert on.tlas_visibility_update_count() == off.tlas_visibility_update_count() == 0
        assert on.update_counts()["full"] == 5
        for sc in (on, off):
            assert not any(sc.tlas_build_stats()[k] for k in ("device_builds", "allocations", "resident_device_built") + FALLBACKS), sc.tlas_build_stats()
    finally:
        on.close(); off.close()


@pytest.mark.gpu
def test_with_the_option_off_the_statistics_stay_zero(gi, orc, monkeypatch):
    monkeypatch.setenv("GATLING_OPTIONS", "tlas_device_min=0")
    sc = _make(option_on=False)
    try:
        sc.render(RS, W, H)
        for key, edit in SEQUENCE:
            edit(sc)
            got = sc.render_aovs(RS, W, H, AOVS)
            assert sc.update_counts()["full"] == 1, key
            _resident_checks(sc, key)
        T._check(orc, sc, "tlas-device-build " + SEQUENCE[-1][0], got)  # (the description, and so the oracle's image, is the sequence's last)
        st = sc.tlas_build_stats()
        assert all(v == 0 for v in st.values() if not isinstance(v, list)) and st["stage_us"] == [0, 0, 0, 0], st
    finally:
        sc.close()


TWO_CONTEXTS = textwrap.dedent("""
    import sys
    sys.path.insert(0, %(root)r)
    sys.path.insert(0, %(tests)r)
    from gatling_amd import capi
    import test_tlas_device_build as D
    L = capi.initialize(0)                      # $GATLING_DEVICES = "0,0": two contexts on the one GPU
    assert L.giCGetDeviceCount() == 2
    multi = D._make()
    single = D._make(); single.set_option(capi.OPTION_DEVICES, 1)
    for sc in (multi, single):
        sc.render_aovs(D.RS, D.W, D.H, D.AOVS)
    for key, edit in D.SEQUENCE:
        out = []
        for sc in (multi, single):
            edit(sc)
            out.append(sc.render_aovs(D.RS, D.W, D.H, D.AOVS))
        for k in out[0]:
            assert D.T._bits_equal(out[0][k], out[1][k]), key + ": " + k + " differs between two device contexts and one"
        D._resident_checks(multi, key, devices=(0, 1))
        D._resident_checks(single, key)
    for sc in (multi, single):
        st = sc.tlas_build_stats()
        assert sc.update_counts()["full"] == 1 and st["device_builds"] == len(D.SEQUENCE) and not any(st[k] for k in D.FALLBACKS), st
    multi.close(); single.close()
    print("two contexts ok")
""")


@pytest.mark.gpu
def test_device_built_tlas_reaches_every_device_context():
    env = dict(os.environ); env["GATLING_DEVICES"] = "0,0"; env["GATLING_OPTIONS"] = "tlas_device_min=0"
    out = subprocess.run([sys.executable, "-c", TWO_CONTEXTS % {"root": ROOT, "tests": os.path.join(ROOT, "tests")}], capture_output=True, text=True, timeout=300, env=env)
    assert out.returncode == 0 and "two contexts ok" in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# random edit sequences
# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
RANDOM_SEEDS = list(range(23000, 23020))
RANDOM_EDITS = 6


def _draw_edits(seed):
    """Six edits drawn from the seed alone against a shadow of the scene: (kind, mesh name, argument).  Meshes are named: indices shift when one is destroyed.
    At most one mesh is hidden at a time and a hidden mesh is only shown again (options 16 and 21 decline an edit of a hidden mesh), so at least 6 000 of the
    8 000 triangles stay visible, above the floor of 4 096; a sequence destroys at most two meshes of about 2 000 triangles against 8 000 live ones, far
    from the rule "more retired than live"."""
    rng = np.random.default_rng(seed)
    names = [f"/Spheres/m{i}" for i in range(4)]
    count = {n: 100 for n in names}
    hidden, serial, retired, edits = None, 0, 0, []
    for _ in range(RANDOM_EDITS):
        kinds = ["move", "move-mesh", "grow", "shrink"] + (["recreate"] if serial < 2 else []) + (["show"] if hidden else ["hide"])
        kind = kinds[int(rng.integers(len(kinds)))]
        free = [n for n in names if n != hidden]
        name = hidden if kind == "show" else free[int(rng.integers(len(free)))]
        arg = None
        if kind == "move":
            arg = (int(rng.integers(count[name])), tuple(float(v) for v in rng.uniform(-0.6, 0.6, 3)))
        elif kind == "move-mesh":
            arg = tuple(float(v) for v in rng.uniform(-0.4, 0.4, 3))
        elif kind == "grow":
            count[name] += 1
        elif kind == "shrink":
            count[name] -= 1
        elif kind == "recreate":
            serial += 1; retired += 20 * count[name]
            new = f"{name.split('#')[0]}#{serial}"
            names[names.index(name)] = new; count[new] = count.pop(name); arg = new
            names.append(names.pop(names.index(new)))  # (a created mesh is appended)
        hidden = name if kind == "hide" else (None if kind == "show" else hidden)
        edits.append((kind, name, arg))
    return edits, retired


def _apply(sc, kind, name, arg):
    i = T._idx(sc, name)
    if kind == "move":
        _move_instance(sc, i, arg[0], arg[1])
    elif kind == "move-mesh":
        sc.set_mesh_transform(i, np.asarray(sc.desc.meshes[i].transform, np.float32).reshape(4, 4) @ _translate(*arg))
    elif kind == "grow":
        _grow(sc, i)
    elif kind == "shrink":
        _shrink(sc, i)
    elif kind == "recreate":
        m = copy.deepcopy(sc.desc.meshes[i]); m.name = arg
        sc.destroy_mesh(i)
        sc.create_mesh(m)
    else:
        sc.set_mesh_visibility(i, kind == "show")


def test_random_sequences_are_the_ones_the_cases_are_written_for():
    kinds = set()
    for seed in RANDOM_SEEDS:
        edits, retired = _draw_edits(seed)
        assert len(edits) == RANDOM_EDITS and retired <= 2 * 20 * 106, (seed, retired)  # (never more retired than live triangles)
        kinds |= {k for k, _, _ in edits}
    assert kinds == {"move", "move-mesh", "grow", "shrink", "recreate", "hide", "show"}, kinds


@pytest.mark.gpu
@pytest.mark.parametrize("seed", RANDOM_SEEDS)
def test_random_edit_sequences_match_the_oracle(gi, orc, monkeypatch, seed):
    monkeypatch.setenv("GATLING_OPTIONS", "tlas_device_min=0")
    edits, _ = _draw_edits(seed)
    sc = _make()
    try:
        sc.render(RS, W, H)
        for k, (kind, name, arg) in enumerate(edits):
            _apply(sc, kind, name, arg)
            got = sc.render_aovs(RS, W, H, AOVS)
            st = sc.tlas_build_stats()
            assert sc.update_counts()["full"] == 1, (seed, k, kind, sc.update_counts())
            assert st["device_builds"] >= k + 1 and not any(st[f] for f in FALLBACKS), (seed, k, kind, st)
            _resident_checks(sc, f"{seed}/{k} {kind}")
            T._check(orc, sc, f"tlas-device-build random {seed}/{k}", got)
    finally:
        sc.close()

"""GPU parity (-m gpu): every traversal stack filled to its last row and held to the oracle.  The host sizes each per-lane stack from the tree's depth
(bvhDepth = levels - 1, "the most entries a walk pushes"): k_path and k_trace 4 or 8 rows, k_trace_dyn 8, 12, 16 or 16 plus a scratch spill, k_aov 8, 16 or 16
plus spill; k_path keeps its parked glossy hits in the rows directly above row bvhDepth - 1; and a push beyond the last row is clamped onto it -- nothing
faults, a subtree goes missing.  Only a walk that reaches the last row can show such a defect, so the scenes of tests/stack_fill_scenes.py are built to make
one (tests/test_stack_fill_host.py pins them on the CPU), and a counting render proves it here: giCDebugTraversalStackHigh reports the stack pointer after a
push, maximum over every walk of the render, closest-hit and shadow walks apart.  Every image, `segments`, `shadowRays`, ray result and AOV is the oracle's bit
for bit.  Not counted but inferred from the counting render of the same scene and frame: the hot (single-class) variants of k_path, every non-counting
variant, and the walks of camera rays under the bounds retire (counting builds trace every camera ray).  k_aov has no counting variant either: it replays the
frame's camera rays through the same node pick, so what it holds is what a counting render of the camera rays alone (one bounce) holds -- counted per scene in
test_aovs_against_the_oracle: the last row of its 8-row variant at bvhDepth 8, of its 16-row variant at 16, five spilled entries at 22; in the other scenes its
stack has rows to spare (bvhDepth 4 .. 7 of 8 rows, 12 of 16; the bvhDepth-9 scene's camera rays hold 7 of 16)."""
import copy
import dataclasses

import numpy as np
import pytest

import stack_fill_scenes as S
from gatling_amd.scene import MAT_DIFFUSE, MaterialDesc, RenderSettings

pytestmark = pytest.mark.gpu

W, H = 32, 18
RS = RenderSettings(spp=2, max_bounces=4, progressive_accumulation=False)
RS_NEE = dataclasses.replace(RS, next_event_estimation=True)
FUSED_SCENES = [f for f in S.SCENES if f.fused]
IDS = lambda fs: [f.name for f in fs]


def assert_image_parity(img, ref, what):
    assert img.shape == ref.shape and np.isfinite(img).all(), what
    bad = int((img.view(np.uint32) != ref.view(np.uint32)).any(axis=-1).sum())
    assert bad == 0, f"{what}: {bad} pixels differ bitwise"


_oracle = {}


def _reference(orc, key, desc, rs):
    key = (key, rs.next_event_estimation)
    if key not in _oracle:
        _oracle[key] = orc.render(desc, rs, W, H, threads=4)
    return _oracle[key]


def _render(gi, monkeypatch, desc, rs, fused, count=False, options=""):
    monkeypatch.setenv("GATLING_OPTIONS", options)
    sc = gi.Scene(copy.deepcopy(desc))
    try:
        if fused is not None:  # (None: the option stays at its default, the library decides)
            sc.set_option(gi.OPTION_FUSED_PATH, fused)
        if count:
            sc.set_option(gi.OPTION_COUNT_TRAVERSAL, 1)
        img = sc.render(rs, W, H).copy()
        return img, sc.stats(), sc.traversal_stack_high(), sc.path_lobe_stats(), sc.class_state()
    finally:
        sc.close()


def _held(img, st, ref, cnt, what):
    assert (st["segments"], st["shadowRays"], st["samples"]) == (cnt["segments"], cnt["shadow_rays"], cnt["samples"]), (what, st, cnt)
    assert_image_parity(img, ref, what)


@pytest.mark.parametrize("f", S.SCENES, ids=IDS(S.SCENES))
def test_counting_render_reaches_the_last_row(gi, orc, monkeypatch, f):
    """(a) NEE off: the closest-hit high equals the scene's target exactly (group 3: reported; group 5: at least 18, two entries or more in the spill) and never
    exceeds bvhDepth, the rows are the expected variant's, the render is the oracle's.  (e) NEE on, the light at the big end: the shadow high is reported
    (test_shadow_walk_reaches_the_last_row holds the two scenes that must fill their stack in a shadow walk)."""
    for fused in ((1, 0) if f.fused else (0,)):
        kernel = "k_path" if fused else f.kernel
        desc = S.scene(f)
        ref, cnt = _reference(orc, f.name, desc, RS)
        img, st, high, _, _ = _render(gi, monkeypatch, desc, RS, fused, count=True)
        print(f"{f.name} {kernel}: bvhDepth {f.depth}, closest high {high['closest']}, rows {high['rows']}, spill {high['spill']}, nodes {st['nodesVisited']}")
        assert st["fusedPath"] == fused and high["rows"] == f.rows and high["shadow"] == 0
        assert high["closest"] <= f.depth
        if f.group == 5:
            assert high["closest"] >= f.high and high["spill"] == high["closest"] - 16 >= 2
        else:
            assert high["spill"] == 0
            if f.group != 3:
                assert high["closest"] == f.high == f.depth
        _held(img, st, ref, cnt, (f.name, kernel))
        desc = S.scene(f, light=True)
        ref, cnt = _reference(orc, f.name + "+light", desc, RS_NEE)
        img, st, high, _, _ = _render(gi, monkeypatch, desc, RS_NEE, fused, count=True)
        print(f"{f.name} {kernel} NEE: closest high {high['closest']}, shadow high {high['shadow']}, shadow rays {st['shadowRays']}")
        assert st["shadowRays"] > 0 and high["shadow"] <= f.depth and high["closest"] <= f.depth
        _held(img, st, ref, cnt, (f.name, kernel, "nee"))


@pytest.mark.parametrize("name,fused", [("d8", 1), ("d16", 0)])
def test_shadow_walk_reaches_the_last_row(gi, monkeypatch, name, fused):
    """(e) the stack-8 k_path scene and the 16-row k_trace_dyn scene reach their last row in a SHADOW walk too.  An any-hit walk ends at its first hit, and a
    shadow ray that skims the triangles' plane is ended by a large triangle in an upper node before it has descended the chain (a light at slopes 0 .. 0.02
    gave 6 of 8 and 2 of 16); the light of stack_fill_scenes.scene spans the slopes at which a ray passes over every larger triangle inside their boxes.
    (The other scenes, reported by test_counting_render_reaches_the_last_row: the shadow high equals the closest-hit high except in d9, 6 of 7, and d12,
    11 of 12.)"""
    f = S.BY_NAME[name]
    _, st, high, _, _ = _render(gi, monkeypatch, S.scene(f, light=True), RS_NEE, fused, count=True)
    print(f"{name} fused {fused}: shadow high {high['shadow']} of bvhDepth {f.depth}, {st['shadowRays']} shadow rays")
    assert st["fusedPath"] == fused and high["shadow"] == f.depth


@pytest.mark.parametrize("option", [None, 1])
def test_fused_kernel_declines_the_depth_nine_scene(gi, orc, monkeypatch, option):
    """Group 3, the 8 | 9 hand-over: the bvhDepth-9 scene is LDS-resident, and with the fused option at its default or asked for outright it is the library
    (pathKernelSupports: bvhDepth <= 8) that declines -- fusedPath == 0 --, k_trace_dyn runs with 12 rows, counting and plain, NEE off and on, and the render
    is the oracle's.  (Every other test of this scene sets the option to 0 itself.)"""
    f = S.BY_NAME["d9"]
    for rs, light in ((RS, False), (RS_NEE, True)):
        desc = S.scene(f, light=light)
        ref, cnt = _reference(orc, f.name + ("+light" if light else ""), desc, rs)
        for count in (True, False):
            img, st, high, _, _ = _render(gi, monkeypatch, desc, rs, option, count=count)
            print(f"d9 fused option {option} count {count} light {light}: fusedPath {st['fusedPath']}, {high}")
            assert st["fusedPath"] == 0
            assert high["rows"] == (12 if count else 0) and high["spill"] == 0 and high["closest"] <= f.depth
            _held(img, st, ref, cnt, (f.name, option, count, light))


def test_counter_is_zero_without_the_option(gi, monkeypatch):
    f = S.BY_NAME["d8"]
    for fused in (1, 0):
        _, _, high, _, _ = _render(gi, monkeypatch, S.scene(f), RS, fused)
        assert high == {"closest": 0, "shadow": 0, "rows": 0, "spill": 0}


@pytest.mark.parametrize("f", S.SCENES, ids=IDS(S.SCENES))
def test_plain_render_equals_the_oracle(gi, orc, monkeypatch, f):
    """(b) the kernels that do not count, same scene and frame: the wavefront kernels, and for the k_path scenes the walk carry off / default / most eager,
    the ring carry off / on and the lobe parking off / most eager / laziest."""
    desc = S.scene(f)
    ref, cnt = _reference(orc, f.name, desc, RS)
    img, st, _, _, _ = _render(gi, monkeypatch, desc, RS, 0)
    assert st["fusedPath"] == 0
    _held(img, st, ref, cnt, (f.name, f.kernel))
    if not f.fused:
        return
    for walk in ("walk_carry=0", "", "walk_carry=63"):
        for ring in ("ring_carry=0", "ring_carry=1"):
            for park in ("lobe_park=0", "lobe_park=1", "lobe_park=64"):
                options = ",".join(k for k in (walk, ring, park) if k)
                img, st, _, _, _ = _render(gi, monkeypatch, desc, RS, 1, options=options)
                assert st["fusedPath"] == 1
                _held(img, st, ref, cnt, (f.name, options))


RAY_SCENES = [f for f in S.SCENES if f.rays_comparable]


@pytest.mark.parametrize("f", RAY_SCENES, ids=IDS(RAY_SCENES))
def test_outward_rays_against_the_oracle(gi, orc, f):
    """(c) a few thousand rays from the small end outward (the bundle whose host walk reaches the last row): ids equal, (t, u, v) bits equal on hits.  The
    scenes whose smallest triangles lie below 1e-7 of the scene's size are held by image only (stack_fill_scenes.Fill.rays_comparable)."""
    desc = S.scene(f)
    o, d = S.bundle(f, m=3000)
    sc = gi.Scene(desc)
    try:
        tuv, ip = sc.trace_rays(o, d)
    finally:
        sc.close()
    rtuv, rip = orc.trace_rays(desc, o, d)
    hit = rip[:, 0] >= 0
    print(f"{f.name}: {int(hit.sum())} of {len(o)} outward rays hit")
    assert np.array_equal(ip, rip)
    assert 0.02 < hit.mean() and np.array_equal(tuv[hit].view(np.uint32), rtuv[hit].view(np.uint32))


AOVS = ["instanceId", "faceId", "objectId", "depth"]
AOV_CLEAR = {"instanceId": -1, "faceId": -1, "objectId": -1, "depth": 1.0}


@pytest.mark.parametrize("f", S.SCENES, ids=IDS(S.SCENES))
def test_aovs_against_the_oracle(gi, orc, monkeypatch, f):
    """(d) k_aov has no counting variant.  It replays this frame's camera rays (same pixels, samples and random streams) through the same node pick, so what its
    walks hold is what the camera rays of a counting render hold: a counting render of ONE bounce, in which nothing but camera rays walks, must reach the
    scene's target row from this camera (d9: reported, its camera rays hold 7 of k_aov's 16 rows) -- then the AOVs of the same frame are held to the oracle."""
    desc = S.scene(f)
    _, st, high, _, _ = _render(gi, monkeypatch, desc, dataclasses.replace(RS, max_bounces=1), 0, count=True)
    print(f"{f.name}: camera rays alone hold {high['closest']} entries (bvhDepth {f.depth}, k_aov rows {8 if f.depth <= 8 else 16}), spill {high['spill']}")
    assert st["segments"] == st["samples"] == W * H * RS.spp  # nothing but camera rays
    assert high["closest"] <= f.depth
    if f.group == 5:
        assert high["closest"] >= f.high and high["spill"] >= 2
    elif f.group != 3:
        assert high["closest"] == f.high == f.depth
    sc = gi.Scene(desc)
    try:
        got = sc.render_aovs(RS, W, H, AOVS, AOV_CLEAR, with_color=False)
    finally:
        sc.close()
    ref = orc.render_aovs(desc, RS, W, H, AOVS, AOV_CLEAR)
    for name in AOVS:
        assert np.array_equal(got[name], np.asarray(ref[name]).reshape(got[name].shape), equal_nan=got[name].dtype.kind == "f"), (f.name, name)
    assert 0.02 < (got["faceId"] >= 0).mean() < 1.0


@pytest.mark.parametrize("f", FUSED_SCENES, ids=IDS(FUSED_SCENES))
@pytest.mark.parametrize("park", ["lobe_park=1", "lobe_park=64"])
def test_lot_next_to_a_full_stack(gi, orc, monkeypatch, f, park):
    """k_path, NEE off, one UsdPreviewSurface material: the parked hits lie in the rows from bvhDepth on.  At bvhDepth 5, 6 and 7 one counting render shows
    both hits parked and a walk in row bvhDepth - 1, the row below the lot; at 4 and 8 the stack has no row to spare and nothing is parked."""
    desc = S.scene(f)
    ref, cnt = _reference(orc, f.name, desc, RS)
    img, st, high, lobes, _ = _render(gi, monkeypatch, desc, RS, 1, count=True, options=park)
    print(f"{f.name} [{park}]: high {high['closest']} of {high['rows']} rows, {lobes}")
    assert st["fusedPath"] == 1 and high["closest"] == f.depth
    if f.depth in (4, 8):
        assert lobes["parked"] == 0 and lobes["adopted"] == 0
    else:
        assert lobes["parked"] > 0 and lobes["adopted"] == lobes["parked"]
    _held(img, st, ref, cnt, (f.name, park))


MATERIALS = {0: lambda: MaterialDesc.usd_preview_surface(diffuseColor=(0.8, 0.7, 0.6), klass=MAT_DIFFUSE),
             1: lambda: MaterialDesc.usd_preview_surface(diffuseColor=(0.8, 0.7, 0.6), roughness=0.5),
             2: lambda: MaterialDesc.open_pbr(base_color=(0.8, 0.7, 0.6))}


@pytest.mark.parametrize("nee", [0, 1])
@pytest.mark.parametrize("klass", [0, 1, 2])
def test_hot_stack8_variants(gi, orc, monkeypatch, klass, nee):
    """The six single-class instantiations k_path<0 | 1 | 2, no texture, NEE off | on, no cutout, no counters, 8>: the bvhDepth-8 scene with one material of
    each class.  Hot variants have no counters: that their walks reach row 7 is inferred from the counting render of the same scene, frame and material
    (the general variant walks the same rays), which runs here too.  From this camera the camera rays themselves reach row 7, so the high does not hang on
    which bounce rays a material draws."""
    f = S.BY_NAME["d8"]
    desc = S.scene(f, material=MATERIALS[klass](), light=bool(nee))
    rs = RS_NEE if nee else RS
    ref, cnt = _reference(orc, (f.name, klass, nee), desc, rs)
    img, st, high, _, cls = _render(gi, monkeypatch, desc, rs, 1)
    assert st["fusedPath"] == 1 and high["rows"] == 0
    assert cls["classMask"] == 1 << klass and cls["classTextured"] == 0 and not cls["hasCutouts"]  # pickPathKernel: the hot family
    _held(img, st, ref, cnt, ("hot", klass, nee))
    img, st, high, _, _ = _render(gi, monkeypatch, desc, rs, 1, count=True)
    assert (high["closest"], high["rows"]) == (8, 8)
    _held(img, st, ref, cnt, ("hot, counted", klass, nee))

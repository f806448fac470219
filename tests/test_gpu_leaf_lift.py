"""The leaf lift of small flat trees on the GPU (gatling_amd/csrc/leaf_lift.cpp; gi_build.cpp buildScene; GI_C_SCENE_OPTION_LEAF_LIFT = 25,
GATLING_OPTIONS=leaf_lift; tests/test_leaf_lift_host.py holds the pass itself on the CPU).  Scene sync hands the flat tree of a scene the fused kernel walks
out of LDS to the pass, which on cornell moves the ceiling's leaf slot out of the light's node into the root's free slot.  By the traversal contract the image
does not depend on the tree: every render here must be byte-equal with leaf_lift=0 (the builder's tree) and leaf_lift=1 / the key absent (the lifted one),
`segments` included, and equal to the CPU oracle bit for bit -- classes 0 and 1 through the fused kernel, next-event estimation, the AOV kernel.  That the
pass acted is read from giCDebugSceneLeafLift, and what it buys from a counting build: fewer nodes visited for the same segments.

Cornell at 96 x 54, spp 4, 8 bounces throughout; every oracle frame is computed once."""
import copy

import numpy as np
import pytest

import path_matrix_cases as M
from gatling_amd.scene import RenderSettings

gpu = pytest.mark.gpu

W, H = 96, 54
RS = RenderSettings(spp=4, max_bounces=8, progressive_accumulation=False)
RS_NEE = RenderSettings(spp=4, max_bounces=8, progressive_accumulation=False, next_event_estimation=True)
KEYS = ("leaf_lift=0", "leaf_lift=1", "")  # the builder's tree / the lifted tree / the default: lifted
AOVS = ["normal", "objectId", "faceId", "depth"]


def assert_image_parity(img, ref, what):
    assert img.shape == ref.shape and np.isfinite(img).all(), what
    bad = int((img.view(np.uint32) != ref.view(np.uint32)).any(axis=-1).sum())
    assert bad == 0, f"{what}: {bad} pixels differ bitwise"


_oracle = {}


def _reference(orc, name, desc, rs):
    """The oracle's frame of a scene, computed once for all the tests that need it."""
    if name not in _oracle:
        img, cnt = orc.render(desc, rs, W, H, threads=4)
        img.setflags(write=False)
        _oracle[name] = (img, cnt)
    return _oracle[name]


def _render(gi, monkeypatch, options, desc, rs, count=False, option=None):
    """Two renders of a fresh scene; returns the image, the counters, what the scene build lifted and the resident tree's check."""
    monkeypatch.setenv("GATLING_OPTIONS", options)
    sc = gi.Scene(copy.deepcopy(desc))
    try:
        if count:
            sc.set_option(gi.OPTION_COUNT_TRAVERSAL, 1)
        if option is not None:
            sc.set_option(gi.OPTION_LEAF_LIFT, option)
        img = sc.render(rs, W, H).copy()
        st, lift, tree = sc.stats(), sc.leaf_lift(), sc.validate_bvh()
        again = sc.render(rs, W, H).copy()
        assert sc.stats()["segments"] == st["segments"] and again.tobytes() == img.tobytes() and sc.leaf_lift() == lift, options
    finally:
        sc.close()
    assert tree["violations"] == 0, (options, tree)
    return img, st, lift, tree


@gpu
@pytest.mark.parametrize("name", ["A1", "A2"], ids=["class0", "class1"])
def test_fused_image_is_the_same_with_and_without_the_pass(gi, orc, monkeypatch, name):
    desc = M.scene(name)
    ref, cnt = _reference(orc, name, desc, RS)
    got = {k: _render(gi, monkeypatch, k, desc, RS) for k in KEYS}
    for k, (img, st, lift, tree) in got.items():
        print(f"{name} [{k or 'default'}]: lifted {lift['lifted']}, depth {lift['depth']}, {tree['nodes']} nodes, digest {tree['digest']:#x}, segments {st['segments']} / {cnt['segments']}")
        assert st["fusedPath"] == 1 and (st["nodeCount"], st["triangleCount"], lift["depth"]) == (4, 46, 2), (k, st, lift)
        assert img.tobytes() == got["leaf_lift=0"][0].tobytes() and st["segments"] == got["leaf_lift=0"][1]["segments"], (name, k)
        assert (st["segments"], st["samples"]) == (cnt["segments"], cnt["samples"]), (name, k, st, cnt)
        assert_image_parity(img, ref, (name, k))
    assert got["leaf_lift=0"][2]["lifted"] == 0 and got["leaf_lift=1"][2]["lifted"] >= 1 and got[""][2] == got["leaf_lift=1"][2]
    assert got["leaf_lift=0"][3]["digest"] != got["leaf_lift=1"][3]["digest"] == got[""][3]["digest"]  # another tree is resident


@gpu
def test_counting_build_visits_fewer_nodes(gi, orc, monkeypatch):
    desc = M.scene("A2")
    ref, cnt = _reference(orc, "A2", desc, RS)
    got = {k: _render(gi, monkeypatch, k, desc, RS, count=True) for k in ("leaf_lift=0", "leaf_lift=1")}
    for k, (img, st, lift, _) in got.items():
        print(f"A2 counting build [{k}]: lifted {lift['lifted']}, segments {st['segments']}, nodesVisited {st['nodesVisited']} "
              f"({st['nodesVisited'] / st['segments']:.4f} per segment), trisTested {st['trisTested']} ({st['trisTested'] / st['segments']:.4f} per segment)")
        assert_image_parity(img, ref, ("A2 counting", k))
        assert st["segments"] == cnt["segments"] and st["nodesVisited"] >= st["segments"] > 0, (k, st)
    assert got["leaf_lift=1"][1]["nodesVisited"] < got["leaf_lift=0"][1]["nodesVisited"]


@gpu
def test_nee_and_aovs_are_the_same(gi, orc, monkeypatch):
    desc = M.scene("A2", nee=True)
    ref, cnt = _reference(orc, "A2-nee", desc, RS_NEE)
    got = {k: _render(gi, monkeypatch, k, desc, RS_NEE) for k in ("leaf_lift=0", "leaf_lift=1")}
    for k, (img, st, lift, _) in got.items():
        assert st["fusedPath"] == 1 and lift["lifted"] == (0 if k == "leaf_lift=0" else got["leaf_lift=1"][2]["lifted"]) and got["leaf_lift=1"][2]["lifted"] >= 1
        assert (st["segments"], st["shadowRays"], st["samples"]) == (cnt["segments"], cnt["shadow_rays"], cnt["samples"]), (k, st, cnt)
        assert_image_parity(img, ref, ("A2 nee", k))
    assert got["leaf_lift=0"][0].tobytes() == got["leaf_lift=1"][0].tobytes()
    # the AOV kernel walks the same tree
    plain = M.scene("A2")
    want = orc.render_aovs(plain, RS, W, H, AOVS, clear_values={"depth": 1.0})
    aovs = {}
    for k in ("leaf_lift=0", "leaf_lift=1"):
        monkeypatch.setenv("GATLING_OPTIONS", k)
        sc = gi.Scene(copy.deepcopy(plain))
        try:
            aovs[k] = sc.render_aovs(RS, W, H, AOVS, clear_values={"depth": 1.0})
            assert (sc.leaf_lift()["lifted"] >= 1) == (k == "leaf_lift=1")
        finally:
            sc.close()
        for name in AOVS:
            got = aovs[k][name]
            assert np.array_equal(got, np.asarray(want[name]).reshape(got.shape), equal_nan=got.dtype.kind == "f"), (k, name)
    for name in AOVS + ["color"]:
        assert aovs["leaf_lift=0"][name].tobytes() == aovs["leaf_lift=1"][name].tobytes(), name
    assert_image_parity(aovs["leaf_lift=1"]["color"], _reference(orc, "A2", plain, RS)[0], "A2 colour beside the AOVs")


@gpu
def test_scene_option_switches_the_pass_and_the_key_overrides_it(gi, orc, monkeypatch):
    desc = M.scene("A2")
    ref, _ = _reference(orc, "A2", desc, RS)
    off = _render(gi, monkeypatch, "", desc, RS, option=0)
    on = _render(gi, monkeypatch, "", desc, RS, option=1)
    forced = _render(gi, monkeypatch, "leaf_lift=1", desc, RS, option=0)
    assert off[2]["lifted"] == 0 and on[2]["lifted"] >= 1 and forced[2] == on[2]
    for img, _, _, _ in (off, on, forced):
        assert_image_parity(img, ref, "A2 scene option")
    # setting the option on a built scene rebuilds it at the next render
    monkeypatch.setenv("GATLING_OPTIONS", "")
    sc = gi.Scene(copy.deepcopy(desc))
    try:
        a = sc.render(RS, W, H).copy(); la = sc.leaf_lift()
        sc.set_option(gi.OPTION_LEAF_LIFT, 0)
        b = sc.render(RS, W, H).copy(); lb = sc.leaf_lift()
        assert la["lifted"] >= 1 and lb["lifted"] == 0 and a.tobytes() == b.tobytes() and sc.validate_bvh()["digest"] == off[3]["digest"]
    finally:
        sc.close()


@gpu
def test_a_deeper_tree_is_left_alone(gi, orc, monkeypatch):
    desc = M.scene("C")  # the telescope: 100 triangles, 7 levels, LDS-resident, the fused kernel's 8-entry stack
    ref, cnt = _reference(orc, "C", desc, RS)
    got = {k: _render(gi, monkeypatch, k, desc, RS) for k in ("leaf_lift=0", "leaf_lift=1")}
    for k, (img, st, lift, tree) in got.items():
        assert st["fusedPath"] == 1 and lift["depth"] > 2 and lift["lifted"] == 0, (k, st, lift)
        assert st["segments"] == cnt["segments"]
        assert_image_parity(img, ref, ("C", k))
    assert got["leaf_lift=0"][3]["digest"] == got["leaf_lift=1"][3]["digest"]  # the builder's bytes either way

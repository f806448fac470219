"""GPU parity (-m gpu): the lobe parking of the fused persistent kernel k_path (gi_path.hip).  In most trips a wave sets the hits that drew a glossy lobe of a
UsdPreviewSurface material aside (16-dword records in the free rows of its traversal stack) and shades them together, with the hits of a later trip, once
lobe_park of them wait.  A parked hit is shaded from the state it was parked with, so every render must be byte-equal with GATLING_OPTIONS=lobe_park=0 (off), the
default, lobe_park=1 (most eager) and lobe_park=64 (as late as the lot allows: it fills, and the overflow rule runs), segment and sample counts included; the
default is also held to the CPU oracle bit for bit.  That hits really are parked is shown by counting builds (giCDebugPathLobeStats)."""
import copy

import numpy as np
import pytest

from gatling_amd.scene import P_CLEARCOAT, P_METALLIC, P_ROUGHNESS, RenderSettings
from gatling_amd.scenes import cornell_box
from test_gpu_path_walk_carry import _telescope

pytestmark = pytest.mark.gpu

KEYS = ("lobe_park=0", "", "lobe_park=1", "lobe_park=64")  # off, the default, the most eager form, the laziest
PARK_STATS = ("liteTrips", "fullTrips", "parked", "adopted", "reruns", "rerunHits")


def scene_a():
    """Cornell with its UsdPreviewSurface materials (the benchmark's scene): about one hit in twelve draws the specular lobe."""
    return cornell_box()


def scene_m():
    """Every material a metal: nearly every hit goes glossy, so a LITE trip's deferred hits do not fit the lot and its shade is run again on the spot."""
    d = cornell_box()
    for m in d.materials:
        m.params[P_METALLIC] = 1.0; m.params[P_ROUGHNESS] = 0.2
    return d


def scene_k():
    """Clearcoat on the white material: lobe 0 (the coat) is taken."""
    d = cornell_box()
    d.materials[1].params[P_CLEARCOAT] = 1.0
    return d


def scene_e():
    """The light's material is a metal too: a parked hit on the emitter must add its emission exactly once (the oracle decides)."""
    d = cornell_box()
    d.materials[0].params[P_METALLIC] = 1.0; d.materials[0].params[P_ROUGHNESS] = 0.2
    return d


def scene_t():
    """The 100-triangle telescope: seven levels, the 8-entry stack, one free row -- a lot of 8 records."""
    return _telescope(100, 1.1)


def assert_image_parity(img, ref, what):
    assert img.shape == ref.shape and np.isfinite(img).all(), what
    bad = int((img.view(np.uint32) != ref.view(np.uint32)).any(axis=-1).sum())
    assert bad == 0, f"{what}: {bad} pixels differ bitwise"


def _render(gi, monkeypatch, options, desc, rs, w, h, count=False):
    """Two renders of a fresh scene (the second reuses every device buffer of the first), the counters and, for a counting build, the lobe counters."""
    monkeypatch.setenv("GATLING_OPTIONS", options)
    sc = gi.Scene(copy.deepcopy(desc))
    try:
        if count:
            sc.set_option(gi.OPTION_COUNT_TRAVERSAL, 1)
        img = sc.render(rs, w, h).copy()
        st, lobes = sc.stats(), sc.path_lobe_stats()
        again = sc.render(rs, w, h).copy()
        st2 = sc.stats()
    finally:
        sc.close()
    assert st["fusedPath"] == 1, st
    assert st2["segments"] == st["segments"] and again.tobytes() == img.tobytes(), options
    return img, st, lobes


_oracle = {}


def _reference(orc, name, desc, rs, w, h):
    key = (name, w, h, rs.spp, rs.max_bounces, rs.next_event_estimation)
    if key not in _oracle:
        _oracle[key] = orc.render(desc, rs, w, h, threads=4)
    return _oracle[key]


def _check(gi, orc, monkeypatch, name, desc, rs, w, h, extra=""):
    ref, cnt = _reference(orc, name, desc, rs, w, h)
    got = {k: _render(gi, monkeypatch, ",".join(x for x in (extra, k) if x), desc, rs, w, h) for k in KEYS}
    for k, (img, st, _) in got.items():
        print(f"{name} {w}x{h} spp {rs.spp} [{extra}] [{k or 'default'}]: segments {st['segments']} / {cnt['segments']}, samples {st['samples']} / {cnt['samples']}")
    off = got["lobe_park=0"]
    for k in KEYS:
        assert got[k][0].tobytes() == off[0].tobytes(), (name, extra, k)
        assert [got[k][1][f] for f in ("segments", "samples", "fusedPath")] == [off[1][f] for f in ("segments", "samples", "fusedPath")], (name, extra, k)
    img, st, _ = got[""]
    assert st["segments"] == cnt["segments"] and st["samples"] == cnt["samples"], (name, st, cnt)
    assert_image_parity(img, ref, name)


RS8 = RenderSettings(spp=8, max_bounces=8, progressive_accumulation=False)


@pytest.mark.parametrize("carry", ["", "walk_carry=0", "walk_carry=63"])
def test_cornell_many_trips(gi, orc, monkeypatch, carry):
    """Scene A, 96x54, spp 8, 8 bounces: every wave runs many LITE trips and several FULL ones; crossed with the walk carry off and at its most eager."""
    _check(gi, orc, monkeypatch, "A", scene_a(), RS8, 96, 54, carry)


@pytest.mark.parametrize("carry", ["", "walk_carry=0", "walk_carry=63"])
def test_cornell_tail_drains_the_lot(gi, orc, monkeypatch, carry):
    """8x8 at spp 1: fewer work items than lanes.  No threshold is ever reached; what is parked leaves through the exit rule (the trip loop ends only with the lot empty)."""
    _check(gi, orc, monkeypatch, "A", scene_a(), RenderSettings(spp=1, max_bounces=8, progressive_accumulation=False), 8, 8, carry)


@pytest.mark.parametrize("carry", ["", "walk_carry=0", "walk_carry=63"])
def test_cornell_paths_end_in_the_parked_shade(gi, orc, monkeypatch, carry):
    """max_bounces = 1: the shade that was parked is the path's last step, its sample is finished by the lane that adopted it."""
    _check(gi, orc, monkeypatch, "A", scene_a(), RenderSettings(spp=8, max_bounces=1, progressive_accumulation=False), 96, 54, carry)


@pytest.mark.parametrize("name,make", [("M", scene_m), ("K", scene_k), ("E", scene_e)])
def test_cornell_material_variants(gi, orc, monkeypatch, name, make):
    """M: all metal (the overflow rule on every LITE trip); K: clearcoat (lobe 0); E: a metal emitter (emission added once)."""
    _check(gi, orc, monkeypatch, name, make(), RS8, 96, 54)


def test_tree_deeper_than_four_levels(gi, orc, monkeypatch):
    """Scene T: the 8-entry-stack instantiation with rows 0 .. 6 the walks' and row 7 the lot's 8 records; lobe_park=64 is clamped to 8."""
    _check(gi, orc, monkeypatch, "T", scene_t(), RenderSettings(spp=4, max_bounces=4, progressive_accumulation=False), 64, 36)


def test_every_camera_ray_enters_the_loop(gi, orc, monkeypatch):
    """miss_rect=0, bounds_retire=0: the lanes that miss are camera rays looking past the scene -- the free lanes the parked hits are adopted by."""
    _check(gi, orc, monkeypatch, "A", scene_a(), RS8, 96, 54, "miss_rect=0,bounds_retire=0")


def test_path_following_aovs_bound(gi, orc, monkeypatch):
    """Bounces and ClockCycles AOVs bound: a parked path's record carries rec and the bounce count, whichever lane finishes it.  All three buffers byte-equal
    across the keys, the colour the oracle's."""
    desc, w, h = scene_a(), 96, 54
    ref, _ = _reference(orc, "A", desc, RS8, w, h)
    got = {}
    for k in KEYS:
        monkeypatch.setenv("GATLING_OPTIONS", k)
        sc = gi.Scene(copy.deepcopy(desc))
        try:
            got[k] = sc.render_aovs(RS8, w, h, ["bounces", "clockCycles"])
            assert sc.stats()["fusedPath"] == 1
        finally:
            sc.close()
    for k in KEYS:
        for name in ("color", "bounces", "clockCycles"):
            assert got[k][name].tobytes() == got["lobe_park=0"][name].tobytes(), (k, name)
    assert_image_parity(got[""]["color"], ref, "A with AOVs")


def test_nee_renders_never_park(gi, orc, monkeypatch):
    """The NEE variants are compiled without the parking: with the key set the render is byte-equal to lobe_park=0, and the oracle's."""
    desc = scene_a()
    rs = RenderSettings(spp=4, max_bounces=8, next_event_estimation=True, progressive_accumulation=False)
    off, st0, _ = _render(gi, monkeypatch, "lobe_park=0", desc, rs, 64, 36)
    for k in KEYS[1:]:
        img, st, _ = _render(gi, monkeypatch, k, desc, rs, 64, 36)
        assert img.tobytes() == off.tobytes(), k
        assert (st["segments"], st["shadowRays"], st["samples"]) == (st0["segments"], st0["shadowRays"], st0["samples"]), k
    ref, cnt = _reference(orc, "A", desc, rs, 64, 36)
    assert st0["segments"] == cnt["segments"] and st0["shadowRays"] == cnt["shadow_rays"]
    assert_image_parity(off, ref, "A with NEE")


def test_counting_build_shows_the_parked_hits(gi, orc, monkeypatch):
    """Counting builds take the key when it is set explicitly.  A at 16: hits are parked and adopted, all of them (the lot is empty at the end); M at 16: the
    overflow rule ran; with lobe_park=0 and with the key absent nothing is parked; the image, the segments and the per-ray node and triangle counts do not
    depend on the key."""
    for name, make in (("A", scene_a), ("M", scene_m)):
        desc = make()
        ref, cnt = _reference(orc, name, desc, RS8, 96, 54)
        got = {k: _render(gi, monkeypatch, k, desc, RS8, 96, 54, count=True) for k in ("lobe_park=0", "", "lobe_park=1", "lobe_park=16", "lobe_park=64")}
        for k, (img, st, lobes) in got.items():
            print(f"{name} counting build [{k or 'key absent'}]: {lobes}, segments {st['segments']}, nodesVisited {st['nodesVisited']}, trisTested {st['trisTested']}")
        off = got["lobe_park=0"]
        for k, (img, st, lobes) in got.items():
            assert_image_parity(img, ref, (name, k))
            assert (st["segments"], st["samples"]) == (cnt["segments"], cnt["samples"]), (name, k)
            assert (st["nodesVisited"], st["trisTested"]) == (off[1]["nodesVisited"], off[1]["trisTested"]), (name, k)
            # every hit is shaded once and every glossy one is counted once, whatever the trip it is shaded in
            assert (lobes["shaded"], lobes["glossy"]) == (off[2]["shaded"], off[2]["glossy"]) and 0 < lobes["glossy"] < lobes["shaded"], (name, k, lobes)
            assert lobes["adopted"] == lobes["parked"], (name, k, lobes)  # nothing is left in a lot
            if k in ("lobe_park=0", ""):
                assert all(lobes[f] == 0 for f in PARK_STATS), (name, k, lobes)
            else:
                assert lobes["liteTrips"] > 0 and lobes["fullTrips"] > 0, (name, k, lobes)
        assert got["lobe_park=16"][2]["parked"] > 0 and got["lobe_park=16"][2]["adopted"] > 0, name
        if name == "A":  # fewer trips run the GGX block than without the parking
            assert got["lobe_park=16"][2]["glossyTrips"] < off[2]["glossyTrips"], got["lobe_park=16"][2]
        else:
            assert got["lobe_park=16"][2]["reruns"] > 0 and got["lobe_park=16"][2]["rerunHits"] > 0, got["lobe_park=16"][2]

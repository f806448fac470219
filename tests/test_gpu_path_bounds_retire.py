"""GPU parity (-m gpu): FLAG_BOUNDS_RETIRE in the fused persistent kernel k_path (gi_path.hip).  A camera ray whose slab interval against the scene's bounds is empty
(ray_misses_bounds, gi_stages.h: the test k_raygen applies on the wavefront pipeline) retires where k_path prepares the rays of its ring: the lane stores the
sample such a path ends with and counts its one segment, the other rays take consecutive ring slots.  Every comparison is bit for bit against the CPU oracle;
GATLING_OPTIONS=bounds_retire=0 traces every camera ray as before."""
import copy

import numpy as np
import pytest

from gatling_amd.scene import MAT_DIFFUSE, RenderSettings, SphereLight
from gatling_amd.scenes import _look_at_camera, cornell_box

pytestmark = pytest.mark.gpu

W, H = 96, 54
SWITCHES = ("0", "1")  # bounds_retire: off, the per-ray test


def assert_image_parity(img, ref, exact=True):
    """Bit-identical images (the exact form of test_gpu_parity.assert_image_parity: no tolerance here)."""
    assert exact and img.shape == ref.shape and np.isfinite(img).all()
    bad = int((img.view(np.uint32) != ref.view(np.uint32)).any(axis=-1).sum())
    assert bad == 0, f"{bad} pixels differ bitwise"


def _cameras():
    stock = cornell_box(MAT_DIFFUSE).camera
    cams = {
        "stock": stock,                                                                         # the frame is wider than the box: most rays miss
        "wide": _look_at_camera((0, -6, 0.3), (0, 0, 0), (0, 0, 1), 70.0),
        "away": _look_at_camera((0, -4, 0), (0, -9, 0.5), (0, 0, 1), 40.0),                     # every ray misses: the waves only retire
        "inside": _look_at_camera((0.1, 0.2, -0.1), (1, 1, 0.2), (0, 0, 1), 60.0),              # no ray misses
        "axis": _look_at_camera((0, -4, 0), (0, 0, 0), (0, 0, 1), 40.0),                        # direction components exactly 0
        "far": _look_at_camera((3000, -20000, 900), (0, 0, 0), (0, 0, 1), 0.02),                # the slab arithmetic at 1e4 x the scene's size
        "rolled": _look_at_camera((2.5, -5, 1.5), (0, 0, 0), (0.6, 0.1, 0.8), 55.0),            # up not axis-aligned
    }
    cams["dof"] = copy.copy(cams["wide"]); cams["dof"].f_stop = 1.4; cams["dof"].focus_distance = 6.0; cams["dof"].focal_length = 0.6  # lens radius 0.21
    cams["clipped"] = copy.copy(cams["axis"]); cams["clipped"].clip_start = 0.1; cams["clipped"].clip_end = 2.5  # the box begins 3 units away
    return cams


CAMERAS = _cameras()


def _render_fused(gi, desc, rs, w, h, twice=True, **kw):
    sc = gi.Scene(desc)
    try:
        img = sc.render(rs, w, h, **kw).copy()
        st = sc.stats()
        again = sc.render(rs, w, h, **kw).copy() if twice else img
    finally:
        sc.close()
    assert st["fusedPath"] == 1, st
    return img, again, st


@pytest.mark.parametrize("name", sorted(CAMERAS))
def test_fused_kernel_retires_camera_rays_that_miss_the_bounds(gi, orc, monkeypatch, name):
    """The cornell box (46 triangles, LDS resident) under cameras that make the test bite in every way, NEE off and on, switch off and on, two renders of one scene:
    device == oracle bit for bit, same segment and shadow-ray counts.  (The stock camera also with a sphere light, so that the NEE leg traces shadow rays.)"""
    legs = [(False, False), (True, False)] + ([(True, True)] if name == "stock" else [])
    for nee, lit in legs:
        desc = cornell_box(MAT_DIFFUSE); desc.camera = CAMERAS[name]
        if lit:
            desc.sphere_lights = [SphereLight(pos=(0.3, -0.2, 0.4), base_emission=(6, 5, 4), radius=(0.15, 0.1, 0.2))]
        rs = RenderSettings(spp=3, max_bounces=5, next_event_estimation=nee, progressive_accumulation=False, depth_of_field=name == "dof",
                            clipping_planes=name == "clipped")
        ref, cnt = orc.render(desc, rs, W, H, threads=4)
        if name in ("away", "clipped"):
            assert cnt["segments"] == W * H * rs.spp  # every path is its camera ray
        if name == "inside":
            assert cnt["hits"] >= W * H * rs.spp      # every camera ray hits
        if lit:
            assert cnt["shadow_rays"] > 0
        for switch in SWITCHES:
            monkeypatch.setenv("GATLING_OPTIONS", f"bounds_retire={switch}")
            img, again, st = _render_fused(gi, desc, rs, W, H)
            print(f"{name} nee={nee} lit={lit} bounds_retire={switch}: segments {st['segments']} / {cnt['segments']}, shadow rays {st['shadowRays']} / {cnt['shadow_rays']}")
            assert st["segments"] == cnt["segments"] and st["shadowRays"] == cnt["shadow_rays"] and st["samples"] == cnt["samples"], (nee, lit, switch, st, cnt)
            assert_image_parity(img, ref, exact=True)
            assert_image_parity(again, ref, exact=True)


@pytest.mark.parametrize("switch", SWITCHES)
def test_fused_bounds_retire_edges(gi, orc, monkeypatch, switch):
    """Fewer work items than one wave (5x3, spp 1); a row share of an odd-width frame (67x41, rows 3, 6, .. 36: the work items are tile pixels, the rays those of
    the image pixels); a frame of several batches (sample buffer capped at 1 MiB)."""
    monkeypatch.setenv("GATLING_OPTIONS", f"bounds_retire={switch}")
    desc = cornell_box(MAT_DIFFUSE)
    rs = RenderSettings(spp=1, max_bounces=5, progressive_accumulation=False)
    ref, cnt = orc.render(desc, rs, 5, 3, threads=1)
    img, again, st = _render_fused(gi, desc, rs, 5, 3)
    assert st["segments"] == cnt["segments"] and st["samples"] == 15
    assert_image_parity(img, ref, exact=True)
    assert_image_parity(again, ref, exact=True)

    rs = RenderSettings(spp=3, max_bounces=5, next_event_estimation=True, progressive_accumulation=False)
    rows = list(range(3, 38, 3))
    ref, cnt = orc.render(desc, rs, 67, 41, threads=4, row_list=rows)
    img, again, st = _render_fused(gi, desc, rs, 67, 41, rows=(3, 38), row_stride=3)
    assert img.shape == ref.shape and st["segments"] == cnt["segments"] and st["shadowRays"] == cnt["shadow_rays"]
    assert_image_parity(img, ref, exact=True)
    assert_image_parity(again, ref, exact=True)

    rs = RenderSettings(spp=24, max_bounces=5, progressive_accumulation=False)
    w, h = 128, 72
    ref, cnt = orc.render(desc, rs, w, h, threads=4)
    sc = gi.Scene(desc)
    try:
        sc.set_option(gi.OPTION_SAMPLE_BUFFER_MB, 1)
        img = sc.render(rs, w, h).copy()
        st = sc.stats()
    finally:
        sc.close()
    assert st["fusedPath"] == 1 and st["batches"] >= 3 and st["segments"] == cnt["segments"], st
    assert_image_parity(img, ref, exact=True)


def test_path_following_aov_switches_the_fused_retire_off(gi, orc, monkeypatch):
    """A render that binds a debug AOV which follows whole paths (Bounces: the inferno colour of the last sample's bounce count, also for a path that is only its
    camera ray) keeps the route that traces every camera ray: equal to the oracle, and byte-identical with the switch on and off."""
    desc = cornell_box(MAT_DIFFUSE)
    rs = RenderSettings(spp=3, max_bounces=5, progressive_accumulation=False)
    clear = {"bounces": (0.0, 0.0, 0.0, 0.0)}
    ref = orc.render_aovs(desc, rs, W, H, ["bounces"], clear_values=clear)
    ref_color, cnt = orc.render(desc, rs, W, H, threads=4)
    got = {}
    for switch in ("0", "1"):
        monkeypatch.setenv("GATLING_OPTIONS", f"bounds_retire={switch}")
        sc = gi.Scene(desc)
        try:
            got[switch] = sc.render_aovs(rs, W, H, ["bounces"], clear_values=clear)
            st = sc.stats()
        finally:
            sc.close()
        assert st["fusedPath"] == 1 and st["segments"] == cnt["segments"], st
        assert np.array_equal(got[switch]["bounces"][..., :3], ref["bounces"][..., :3])
        assert_image_parity(got[switch]["color"], ref_color, exact=True)
    for k in ("bounces", "color"):
        assert got["0"][k].tobytes() == got["1"][k].tobytes(), k

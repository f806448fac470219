"""GPU parity (-m gpu): the miss rectangle of fused frames (gi_miss_rect.h; FLAG_MISS_RECT in k_path and k_accumulate).  Pixels outside the rectangle get no
work items and no sample records; k_accumulate sums the retired sample's constant for them with the loop it runs over records.  Every comparison is bit for bit
against the CPU oracle, counters included, with GATLING_OPTIONS=miss_rect=0 (every pixel enumerated, as before) and 1, and two renders per scene."""
import copy

import numpy as np
import pytest

from gatling_amd.scene import MAT_DIFFUSE, RenderSettings, SphereLight
from gatling_amd.scenes import _look_at_camera, cornell_box

pytestmark = pytest.mark.gpu

W, H = 96, 54
SWITCHES = ("0", "1")  # miss_rect: off, on


def assert_image_parity(img, ref):
    assert img.shape == ref.shape and np.isfinite(img).all()
    bad = int((img.view(np.uint32) != ref.view(np.uint32)).any(axis=-1).sum())
    assert bad == 0, f"{bad} pixels differ bitwise"


def _cameras():
    """The table of tests/test_gpu_path_bounds_retire.py, plus `edge`: the box against the left edge of the frame (the rectangle starts at column 0)."""
    stock = cornell_box(MAT_DIFFUSE).camera
    cams = {
        "stock": stock,
        "wide": _look_at_camera((0, -6, 0.3), (0, 0, 0), (0, 0, 1), 70.0),
        "away": _look_at_camera((0, -4, 0), (0, -9, 0.5), (0, 0, 1), 40.0),                     # empty rectangle: k_path is not launched
        "inside": _look_at_camera((0.1, 0.2, -0.1), (1, 1, 0.2), (0, 0, 1), 60.0),              # full frame
        "axis": _look_at_camera((0, -4, 0), (0, 0, 0), (0, 0, 1), 40.0),
        "far": _look_at_camera((3000, -20000, 900), (0, 0, 0), (0, 0, 1), 0.02),                # the margin scales with the float spacing of the image plane
        "rolled": _look_at_camera((2.5, -5, 1.5), (0, 0, 0), (0.6, 0.1, 0.8), 55.0),
        "edge": _look_at_camera((0, -4, 0), (1.6, 0, 0), (0, 0, 1), 40.0),
    }
    cams["dof"] = copy.copy(cams["wide"]); cams["dof"].f_stop = 1.4; cams["dof"].focus_distance = 6.0; cams["dof"].focal_length = 0.6  # full frame
    cams["clipped"] = copy.copy(cams["axis"]); cams["clipped"].clip_start = 0.1; cams["clipped"].clip_end = 2.5
    return cams


CAMERAS = _cameras()


def _render_fused(gi, desc, rs, w, h, twice=True, **kw):
    sc = gi.Scene(desc)
    try:
        img = sc.render(rs, w, h, **kw).copy()
        st = sc.stats()
        again = sc.render(rs, w, h, **kw).copy() if twice else img
        st2 = sc.stats()
    finally:
        sc.close()
    assert st["fusedPath"] == 1, st
    assert (st2["segments"], st2["shadowRays"], st2["samples"]) == (st["segments"], st["shadowRays"], st["samples"])
    return img, again, st


def _check(gi, monkeypatch, desc, rs, w, h, ref, cnt, label, **kw):
    for switch in SWITCHES:
        monkeypatch.setenv("GATLING_OPTIONS", f"miss_rect={switch}")
        img, again, st = _render_fused(gi, desc, rs, w, h, **kw)
        print(f"{label} miss_rect={switch}: segments {st['segments']} / {cnt['segments']}, shadow rays {st['shadowRays']} / {cnt['shadow_rays']}, "
              f"samples {st['samples']} / {cnt['samples']}")
        assert st["segments"] == cnt["segments"] and st["shadowRays"] == cnt["shadow_rays"] and st["samples"] == cnt["samples"], (label, switch, st, cnt)
        assert_image_parity(img, ref)
        assert_image_parity(again, ref)


@pytest.mark.parametrize("name", sorted(CAMERAS))
def test_fused_kernel_skips_pixels_outside_the_miss_rectangle(gi, orc, monkeypatch, name):
    """The camera table at 96x54, spp 3, 5 bounces, NEE off and on (the stock camera also with a sphere light, so that shadow rays are traced)."""
    legs = [(False, False), (True, False)] + ([(True, True)] if name == "stock" else [])
    for nee, lit in legs:
        desc = cornell_box(MAT_DIFFUSE); desc.camera = CAMERAS[name]
        if lit:
            desc.sphere_lights = [SphereLight(pos=(0.3, -0.2, 0.4), base_emission=(6, 5, 4), radius=(0.15, 0.1, 0.2))]
        rs = RenderSettings(spp=3, max_bounces=5, next_event_estimation=nee, progressive_accumulation=False, depth_of_field=name == "dof",
                            clipping_planes=name == "clipped")
        ref, cnt = orc.render(desc, rs, W, H, threads=4)
        if name == "away":
            assert cnt["segments"] == W * H * rs.spp
        if lit:
            assert cnt["shadow_rays"] > 0
        _check(gi, monkeypatch, desc, rs, W, H, ref, cnt, f"{name} nee={nee} lit={lit}")


def test_small_frame(gi, orc, monkeypatch):
    """5x3 at spp 1: fewer work items than one wave, and the rectangle's widening covers the whole frame."""
    desc = cornell_box(MAT_DIFFUSE)
    rs = RenderSettings(spp=1, max_bounces=5, progressive_accumulation=False)
    ref, cnt = orc.render(desc, rs, 5, 3, threads=1)
    _check(gi, monkeypatch, desc, rs, 5, 3, ref, cnt, "5x3")


def test_row_share_whose_rows_straddle_the_rectangle(gi, orc, monkeypatch):
    """67x41, image rows 3, 6 .. 36 (the tile's rows are three image rows apart): the rectangle's first image row falls between two rows of the share, and the
    work items are pixels of the tile, the rays those of the image.  `rolled` has rows above and below the rectangle at this size."""
    for name in ("stock", "rolled"):
        desc = cornell_box(MAT_DIFFUSE); desc.camera = CAMERAS[name]
        rs = RenderSettings(spp=3, max_bounces=5, next_event_estimation=True, progressive_accumulation=False)
        rows = list(range(3, 38, 3))
        ref, cnt = orc.render(desc, rs, 67, 41, threads=4, row_list=rows)
        _check(gi, monkeypatch, desc, rs, 67, 41, ref, cnt, f"row share {name}", rows=(3, 38), row_stride=3)


def test_several_batches_carry_the_constant_sum(gi, orc, monkeypatch):
    """128x72 at spp 24 with the per-sample buffer capped at 1 MiB: three batches or more, so the constant path's running sum goes through `accum`.  With a
    clear colour that is not black the constant is not zero and the carried sum has rounding to keep."""
    desc = cornell_box(MAT_DIFFUSE)
    w, h = 128, 72
    for clear in ((0.0, 0.0, 0.0, 0.0), (0.3, 0.6, 0.9, 1.0)):
        rs = RenderSettings(spp=24, max_bounces=5, progressive_accumulation=False)
        rs.clear_color = clear
        ref, cnt = orc.render(desc, rs, w, h, threads=4)
        for switch in SWITCHES:
            monkeypatch.setenv("GATLING_OPTIONS", f"miss_rect={switch}")
            sc = gi.Scene(desc)
            try:
                sc.set_option(gi.OPTION_SAMPLE_BUFFER_MB, 1)
                img = sc.render(rs, w, h).copy()
                st = sc.stats()
                again = sc.render(rs, w, h).copy()
            finally:
                sc.close()
            assert st["fusedPath"] == 1 and st["batches"] >= 3 and st["segments"] == cnt["segments"] and st["samples"] == cnt["samples"], st
            assert_image_parity(img, ref)
            assert_image_parity(again, ref)


def test_non_black_background(gi, orc, monkeypatch):
    """The retired sample's constant is the clear colour as RGBA8 unorm; with a sample clamp below it the clamp of the finish applies to the constant as well."""
    for name, max_value in (("stock", 1.0e6), ("rolled", 0.4)):
        desc = cornell_box(MAT_DIFFUSE); desc.camera = CAMERAS[name]
        rs = RenderSettings(spp=3, max_bounces=5, progressive_accumulation=False, max_sample_value=max_value)
        rs.clear_color = (0.25, 0.5, 0.75, 1.0)
        ref, cnt = orc.render(desc, rs, W, H, threads=4)
        assert ref[0, 0, 2] > 0.0
        _check(gi, monkeypatch, desc, rs, W, H, ref, cnt, f"background {name} clamp {max_value}")


def test_two_progressive_calls_blend_over_the_colour_buffer(gi, orc, monkeypatch):
    """Progressive accumulation: the second call blends its samples over what the first left in the colour buffer, for the pixels summed from the constant too."""
    desc = cornell_box(MAT_DIFFUSE)
    rs = RenderSettings(spp=3, max_bounces=5, progressive_accumulation=True)
    rs.clear_color = (0.25, 0.5, 0.75, 1.0)
    ref0, cnt0 = orc.render(desc, rs, W, H, threads=4)
    ref1, cnt1 = orc.render(desc, rs, W, H, threads=4, sample_offset=rs.spp, prev_color=ref0)
    for switch in SWITCHES:
        monkeypatch.setenv("GATLING_OPTIONS", f"miss_rect={switch}")
        sc = gi.Scene(desc)
        try:
            img0 = sc.render(rs, W, H).copy(); st0 = sc.stats()
            img1 = sc.render(rs, W, H).copy(); st1 = sc.stats()
        finally:
            sc.close()
        assert st0["fusedPath"] == 1 and st0["segments"] == cnt0["segments"] and st1["segments"] == cnt1["segments"], (st0, st1)
        assert_image_parity(img0, ref0)
        assert_image_parity(img1, ref1)


def test_look_ahead_window_keeps_the_whole_frame(gi, orc, monkeypatch):
    """A look-ahead window is folded by later calls from every pixel's records: renders that trace one keep the full frame, and are equal with the option on and
    off (and to the oracle's progressive frames)."""
    desc = cornell_box(MAT_DIFFUSE)
    rs = RenderSettings(spp=1, max_bounces=5, progressive_accumulation=True)
    refs, prev = [], None
    for k in range(6):
        prev, _ = orc.render(desc, rs, W, H, threads=4, sample_offset=k * rs.spp, prev_color=prev)
        refs.append(prev)
    got = {}
    for switch in SWITCHES:
        monkeypatch.setenv("GATLING_OPTIONS", f"miss_rect={switch}")
        sc = gi.Scene(desc)
        try:
            sc.set_option(gi.OPTION_SAMPLE_LOOKAHEAD, 4)
            got[switch] = [sc.render(rs, W, H).copy() for _ in range(6)]
            la = sc.lookahead_stats()
        finally:
            sc.close()
        assert la["callsServed"] >= 2, la  # windows of 1, 2 and 4 calls: calls 2 and 4 .. 5 are served from a window
        for k in range(6):
            assert_image_parity(got[switch][k], refs[k])
    for k in range(6):
        assert got["0"][k].tobytes() == got["1"][k].tobytes(), k


def test_bounces_aov_switches_the_rectangle_off(gi, orc, monkeypatch):
    """A render that binds the Bounces AOV traces every camera ray (the rule of the per-ray retire, which the rectangle inherits): byte-identical with the option
    on and off, equal to the oracle."""
    desc = cornell_box(MAT_DIFFUSE)
    rs = RenderSettings(spp=3, max_bounces=5, progressive_accumulation=False)
    clear = {"bounces": (0.0, 0.0, 0.0, 0.0)}
    ref = orc.render_aovs(desc, rs, W, H, ["bounces"], clear_values=clear)
    ref_color, cnt = orc.render(desc, rs, W, H, threads=4)
    got = {}
    for switch in SWITCHES:
        monkeypatch.setenv("GATLING_OPTIONS", f"miss_rect={switch}")
        sc = gi.Scene(desc)
        try:
            got[switch] = sc.render_aovs(rs, W, H, ["bounces"], clear_values=clear)
            st = sc.stats()
        finally:
            sc.close()
        assert st["fusedPath"] == 1 and st["segments"] == cnt["segments"], st
        assert np.array_equal(got[switch]["bounces"][..., :3], ref["bounces"][..., :3])
        assert_image_parity(got[switch]["color"], ref_color)
    for k in ("bounces", "color"):
        assert got["0"][k].tobytes() == got["1"][k].tobytes(), k


def test_zero_bounces_stay_black(gi, orc, monkeypatch):
    """max-bounces 0 traces nothing and every sample is black, whatever the clear colour: the constant path must not take such a frame."""
    desc = cornell_box(MAT_DIFFUSE)
    rs = RenderSettings(spp=2, max_bounces=0, progressive_accumulation=False)
    rs.clear_color = (0.25, 0.5, 0.75, 1.0)
    ref, _ = orc.render(desc, rs, W, H, threads=4)
    for switch in SWITCHES:
        monkeypatch.setenv("GATLING_OPTIONS", f"miss_rect={switch}")
        sc = gi.Scene(desc)
        try:
            img = sc.render(rs, W, H).copy()
        finally:
            sc.close()
        assert_image_parity(img, ref)

"""The miss rectangle of fused frames (gi_miss_rect.h, giCDebugMissRect), without a GPU: outside the rectangle every camera ray make_camera_ray can produce for a
pixel misses the scene's bounds, so k_path gives those pixels no work and k_accumulate sums the constant their samples are.  Held here against the CPU oracle
(every pixel outside the rectangle is, bit for bit, that constant), against a float64 brute force over the sub-pixel offsets, and for its shape (a rectangle that
is conservative by being useless fails)."""
import copy
import os

import numpy as np
import pytest

from gatling_amd import capi
from gatling_amd.scene import MAT_DIFFUSE, RenderSettings
from gatling_amd.scenes import _look_at_camera, cornell_box

SIZES = ((480, 270), (96, 54))
FIS_REACH = 4.97  # gi_fis_gauss: 0.375 * sqrt(-2 ln 1e-38) = 4.961


def _cameras():
    """The table of tests/test_gpu_path_bounds_retire.py, plus `edge`: the box against the left edge of the frame."""
    stock = cornell_box(MAT_DIFFUSE).camera
    cams = {
        "stock": stock,
        "wide": _look_at_camera((0, -6, 0.3), (0, 0, 0), (0, 0, 1), 70.0),
        "away": _look_at_camera((0, -4, 0), (0, -9, 0.5), (0, 0, 1), 40.0),
        "inside": _look_at_camera((0.1, 0.2, -0.1), (1, 1, 0.2), (0, 0, 1), 60.0),
        "axis": _look_at_camera((0, -4, 0), (0, 0, 0), (0, 0, 1), 40.0),
        "far": _look_at_camera((3000, -20000, 900), (0, 0, 0), (0, 0, 1), 0.02),
        "rolled": _look_at_camera((2.5, -5, 1.5), (0, 0, 0), (0.6, 0.1, 0.8), 55.0),
        "edge": _look_at_camera((0, -4, 0), (1.6, 0, 0), (0, 0, 1), 40.0),
    }
    cams["dof"] = copy.copy(cams["wide"]); cams["dof"].f_stop = 1.4; cams["dof"].focus_distance = 6.0; cams["dof"].focal_length = 0.6
    cams["clipped"] = copy.copy(cams["axis"]); cams["clipped"].clip_start = 0.1; cams["clipped"].clip_end = 2.5
    return cams


CAMERAS = _cameras()


def _settings(name, **kw):
    return RenderSettings(progressive_accumulation=False, depth_of_field=name == "dof", clipping_planes=name == "clipped", **kw)


def scene_bounds(desc):
    """Axis-aligned bounds of the scene's geometry (row-vector transforms, as the scene description holds them): inside the padded root bounds the device tests
    against, so a rectangle that is conservative for these is what the renders need -- every triangle lies inside them."""
    pts = []
    for m in desc.meshes:
        p = np.asarray(m.vertices)["pos"].reshape(-1, 3).astype(np.float64)
        p4 = np.concatenate([p, np.ones((len(p), 1))], axis=1) @ np.asarray(m.transform, np.float64).reshape(4, 4)
        for inst in np.asarray(m.instance_transforms, np.float64).reshape(-1, 4, 4):
            pts.append((p4 @ inst)[:, :3])
    p = np.concatenate(pts).astype(np.float32)
    return np.concatenate([p.min(0), p.max(0)])


def camera_terms(cam, w, h):
    """The image-plane terms of makeUniforms (gi_render.cpp), in float32 as the device holds them, returned as float64: camPos, A0 = L - camPos, A1 = camRight WX,
    A2 = camUp HY.  A ray through (u, v) pixels has the direction A0 + u A1 + v A2."""
    f32 = np.float32
    fwd = np.asarray(cam.forward, f32); fwd = fwd * (f32(1) / np.sqrt((fwd[0] * fwd[0] + fwd[1] * fwd[1]) + fwd[2] * fwd[2], dtype=f32))
    up = np.asarray(cam.up, f32); up = up * (f32(1) / np.sqrt((up[0] * up[0] + up[1] * up[1]) + up[2] * up[2], dtype=f32))
    pos = np.asarray(cam.position, f32)
    right = np.array([fwd[1] * up[2] - fwd[2] * up[1], fwd[2] * up[0] - fwd[0] * up[2], fwd[0] * up[1] - fwd[1] * up[0]], f32)
    H = f32(1); W = H * (f32(w) / f32(h))
    d = H / (f32(2) * np.tan(f32(cam.vfov) * f32(0.5), dtype=f32))
    WX, HY = W / f32(w), H / f32(h)
    L = ((pos + fwd * d) - right * W * f32(0.5)) - up * H * f32(0.5)
    return pos.astype(np.float64), L.astype(np.float64) - pos.astype(np.float64), right.astype(np.float64) * float(WX), up.astype(np.float64) * float(HY)


def projected_bounds(bounds, cam, w, h):
    """(uMin, vMin, uMax, vMax) of the bounds' eight corners on the image plane, in pixels; None when a corner is not in front of the camera."""
    o, A0, A1, A2 = camera_terms(cam, w, h)
    M = np.stack([A0, A1, A2], axis=1)
    uv = []
    for k in range(8):
        c = np.array([bounds[3 * ((k >> a) & 1) + a] for a in range(3)], np.float64)
        t, tu, tv = np.linalg.solve(M, c - o)
        if t <= 0:
            return None
        uv.append((tu / t, tv / t))
    uv = np.asarray(uv)
    return uv[:, 0].min(), uv[:, 1].min(), uv[:, 0].max(), uv[:, 1].max()


def constant_pixel(rs):
    """What a pixel is when every one of its samples is a camera ray that left the scene, by the device's sequence of float32 operations: the sample
    0 + 1 x background (the clear colour as RGBA8 unorm), the clamp on the largest channel, max(0); summed spp times as pixel + sample * invSpp; the blend of a
    first frame (prev = pixel, sample offset 0); alpha 1."""
    f32 = np.float32
    bg = np.array([f32(min(max(int(f32(c) * f32(255.0)), 0), 255)) / f32(255.0) for c in rs.clear_color[:3]], f32)
    c = f32(0) + f32(1) * bg
    mv = max(c[0], max(c[1], c[2]))
    if mv > f32(rs.max_sample_value):
        c = c * (f32(rs.max_sample_value) / mv)
    c = np.maximum(f32(0), c).astype(f32)
    inv_spp = f32(1) / f32(rs.spp)
    pixel = np.zeros(3, f32)
    for _ in range(rs.spp):
        pixel = (pixel + c * inv_spp).astype(f32)
    out = ((pixel * f32(0) + pixel * f32(rs.spp)) * (f32(1) / f32(0 + rs.spp))).astype(f32)
    return np.array([out[0], out[1], out[2], 1.0], f32)


def outside_mask(rect, w, h):
    x0, y0, x1, y1 = rect
    m = np.ones((h, w), bool)
    m[y0:y1, x0:x1] = False
    return m


@pytest.fixture(scope="module")
def bounds():
    return scene_bounds(cornell_box(MAT_DIFFUSE))


@pytest.mark.parametrize("name", sorted(CAMERAS))
def test_pixels_outside_the_rectangle_are_the_constant_pixel_of_the_oracle(orc, bounds, name):
    """Jitter + filter importance sampling, spp 8: every pixel the rectangle rules out equals the constant pixel bit for bit in the oracle's render."""
    desc = cornell_box(MAT_DIFFUSE); desc.camera = CAMERAS[name]
    for clear in ((0.0, 0.0, 0.0, 0.0), (0.25, 0.5, 0.75, 1.0)):
        rs = _settings(name, spp=8, max_bounces=3)
        rs.clear_color = clear
        want = constant_pixel(rs)
        for w, h in SIZES if clear[0] == 0.0 else SIZES[1:]:
            rect = capi.miss_rect(bounds, desc.camera, rs, w, h)
            ref, _ = orc.render(desc, rs, w, h, threads=min(8, os.cpu_count() or 1))
            out = outside_mask(rect, w, h)
            bad = int((ref.view(np.uint32)[out] != want.view(np.uint32)).any(axis=-1).sum())
            print(f"{name} {w}x{h} clear {clear}: rect {rect}, {int(out.sum())} pixels outside, {bad} differ from {want}")
            assert bad == 0


@pytest.mark.parametrize("name", sorted(CAMERAS))
def test_every_offset_of_a_pixel_outside_the_rectangle_fails_the_slab_test(bounds, name):
    """float64 brute force: a 9 x 9 grid of sub-pixel offsets spanning 0.5 +- 4.97 for every pixel outside the rectangle -- each ray's slab interval against the
    bounds is empty."""
    cam = CAMERAS[name]
    rs = _settings(name, spp=1)
    lo, hi = bounds[:3].astype(np.float64), bounds[3:].astype(np.float64)
    offs = 0.5 + np.linspace(-FIS_REACH, FIS_REACH, 9)
    for w, h in SIZES:
        rect = capi.miss_rect(bounds, cam, rs, w, h)
        ys, xs = np.nonzero(outside_mask(rect, w, h))
        if len(xs) == 0:
            continue
        o, A0, A1, A2 = camera_terms(cam, w, h)
        u = (xs[:, None, None] + offs[None, :, None]) + np.zeros((1, 1, 9))
        v = (ys[:, None, None] + offs[None, None, :]) + np.zeros((1, 9, 1))
        D = A0[None, None, None, :] + u[..., None] * A1 + v[..., None] * A2
        D /= np.linalg.norm(D, axis=-1, keepdims=True)
        with np.errstate(divide="ignore", invalid="ignore"):
            t0, t1 = (lo - o) / D, (hi - o) / D
        near, far = np.minimum(t0, t1), np.maximum(t0, t1)
        parallel_out = ((D == 0.0) & ((o < lo) | (o > hi))).any(axis=-1)
        near = np.where(D == 0.0, -np.inf, near); far = np.where(D == 0.0, np.inf, far)
        tn, tf = np.maximum(near.max(axis=-1), 0.0), far.min(axis=-1)
        hits = int((~(parallel_out | (tn > tf))).sum())
        print(f"{name} {w}x{h}: rect {rect}, {len(xs)} pixels outside x 81 offsets, {hits} rays reach the bounds")
        assert hits == 0


def test_rectangle_shape(bounds):
    rs = _settings("stock", spp=1)
    for w, h in SIZES:
        assert capi.miss_rect(bounds, CAMERAS["away"], rs, w, h) == (0, 0, 0, 0)                      # the camera looks away: nothing to trace
        assert capi.miss_rect(bounds, CAMERAS["inside"], rs, w, h) == (0, 0, w, h)                    # the camera is inside the bounds
        assert capi.miss_rect(bounds, CAMERAS["dof"], _settings("dof", spp=1), w, h) == (0, 0, w, h)  # thin-lens rays do not start at the camera position
        assert capi.miss_rect(bounds, CAMERAS["dof"], rs, w, h) != (0, 0, w, h)                       # (the same camera with depth of field switched off)
    # the stock camera at 480 x 270: at most 7 pixels per side beyond the projected bounds (offset reach 5.47 + margin 1.0x), which cover 0.463 x 0.823 of the frame
    w, h = 480, 270
    x0, y0, x1, y1 = capi.miss_rect(bounds, CAMERAS["stock"], rs, w, h)
    u0, v0, u1, v1 = projected_bounds(bounds, CAMERAS["stock"], w, h)
    print(f"stock {w}x{h}: rect {(x0, y0, x1, y1)}, projected bounds u [{u0:.2f}, {u1:.2f}] v [{v0:.2f}, {v1:.2f}]")
    assert 0 < x0 < x1 < w
    assert u0 - 7 <= x0 <= u0 and u1 <= x1 <= u1 + 7
    assert (max(0.0, v0 - 7) <= y0 <= max(0.0, v0)) and (min(h, v1) <= y1 <= min(h, v1 + 7))
    assert (x1 - x0) * (y1 - y0) <= 0.44 * w * h
    # narrower sampling, narrower rectangle: plain jitter reaches [0, 1), no jitter exactly 0.5
    jit = _settings("stock", spp=1, filter_importance_sampling=False)
    fixed = _settings("stock", spp=1, filter_importance_sampling=False, jittered_sampling=False)
    rj, rf = capi.miss_rect(bounds, CAMERAS["stock"], jit, w, h), capi.miss_rect(bounds, CAMERAS["stock"], fixed, w, h)
    assert x0 < rj[0] <= rf[0] and rf[2] <= rj[2] < x1
    assert u0 - 3 <= rj[0] <= u0 and u0 - 2 <= rf[0] <= u0


def test_rectangle_falls_back_on_values_it_cannot_use(bounds):
    rs = _settings("stock", spp=1)
    w, h = 96, 54
    bad = bounds.copy(); bad[0] = np.nan
    assert capi.miss_rect(bad, CAMERAS["stock"], rs, w, h) == (0, 0, w, h)
    bad = bounds.copy(); bad[3] = np.inf
    assert capi.miss_rect(bad, CAMERAS["stock"], rs, w, h) == (0, 0, w, h)
    flipped = np.concatenate([bounds[3:], bounds[:3]])  # min > max: no valid bounds
    assert capi.miss_rect(flipped, CAMERAS["stock"], rs, w, h) == (0, 0, w, h)
    beside = _look_at_camera((0, -1.5, 0), (5, -1.5, 0), (0, 0, 1), 90.0)  # the bounds straddle the camera's plane: corners in front and behind
    assert capi.miss_rect(bounds, beside, rs, w, h) == (0, 0, w, h)


def test_entry_point_is_declared_and_host_only():
    import re
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "gi_c.h")).read()
    assert re.search(r"int\s+giCDebugMissRect\s*\(\s*const\s+float\s*\*", text)
    assert re.search(r"#define\s+GI_C_API_VERSION\s+8u", text)
    src = open(os.path.join(os.path.dirname(capi.__file__), "csrc", "gi_options.h")).read()
    assert re.search(r"//\s+miss_rect\s+1\s", src)

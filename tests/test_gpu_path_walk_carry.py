"""GPU parity (-m gpu): the walk carry of the fused persistent kernel k_path (gi_path.hip).  The closest-hit loop of a trip ends once at most K lanes are
still walking (and more than K entered); those lanes skip the trip's shading and finish and go on walking in the next trip's loop.  A ray's walk is the same
sequence of steps cut in two, so every render must be byte-equal with GATLING_OPTIONS=walk_carry=0 (every loop runs to its end), the default K and
walk_carry=63 (carry whenever a lane has finished), segment count included; the default is also held to the CPU oracle bit for bit."""
import numpy as np
import pytest

from gatling_amd.scene import CameraDesc, MaterialDesc, MeshDesc, RectLight, RenderSettings, SceneDesc
from gatling_amd.scenes import cornell_box

pytestmark = pytest.mark.gpu

KEYS = ("walk_carry=0", "", "walk_carry=63")  # off, the default, the most eager form


def assert_image_parity(img, ref):
    assert img.shape == ref.shape and np.isfinite(img).all()
    bad = int((img.view(np.uint32) != ref.view(np.uint32)).any(axis=-1).sum())
    assert bad == 0, f"{bad} pixels differ bitwise"


def _render(gi, monkeypatch, options, desc, rs, w, h):
    """Two renders of a fresh scene (the second reuses every device buffer of the first) and the counters."""
    monkeypatch.setenv("GATLING_OPTIONS", options)
    sc = gi.Scene(desc)
    try:
        img = sc.render(rs, w, h).copy()
        st = sc.stats()
        again = sc.render(rs, w, h).copy()
        st2 = sc.stats()
    finally:
        sc.close()
    assert st["fusedPath"] == 1, st
    assert st2["segments"] == st["segments"] and again.tobytes() == img.tobytes(), options
    return img, st


def _check(gi, orc, monkeypatch, desc, rs, w, h, label):
    ref, cnt = orc.render(desc, rs, w, h, threads=4)
    got = {k: _render(gi, monkeypatch, k, desc, rs, w, h) for k in KEYS}
    for k, (img, st) in got.items():
        print(f"{label} [{k or 'default'}]: segments {st['segments']} / {cnt['segments']}, samples {st['samples']} / {cnt['samples']}")
    for k in KEYS:
        assert got[k][0].tobytes() == got["walk_carry=0"][0].tobytes(), (label, k)
        assert got[k][1]["segments"] == got["walk_carry=0"][1]["segments"], (label, k)
    img, st = got[""]
    assert st["segments"] == cnt["segments"] and st["samples"] == cnt["samples"], (label, st, cnt)
    assert_image_parity(img, ref)


def test_many_trips(gi, orc, monkeypatch):
    """Cornell with the benchmark's camera and material, 96x54, spp 16, 8 bounces: every wave runs many trips, with carried lanes at every K."""
    _check(gi, orc, monkeypatch, cornell_box(), RenderSettings(spp=16, max_bounces=8, progressive_accumulation=False), 96, 54, "96x54 spp 16")


def test_fewer_work_items_than_one_wave(gi, orc, monkeypatch):
    """8x4 at spp 1: 32 work items.  With K = 63 no more than K lanes ever enter a loop, with the default the frame's tail does not: both run to completion."""
    _check(gi, orc, monkeypatch, cornell_box(), RenderSettings(spp=1, max_bounces=8, progressive_accumulation=False), 8, 4, "8x4 spp 1")


def _telescope(n, ratio):
    """n triangles whose sizes and distances from the origin shrink geometrically (the scene of test_deep_trees_parity): SAH peels them off one cluster at a
    time; 100 triangles at ratio 1.1 give a tree of 7 levels, which the fused kernel runs with its 8-entry stack."""
    from gatling_amd.meshprep import bake_vertices
    i = np.arange(n, dtype=np.float64)
    s = ratio ** (-i)
    c = np.stack([s * 3.0, 0.3 * s * ((i % 5) - 2), 0.05 * s * (i % 3)], 1)
    tri = np.array([[0, -0.5, 0], [1, 0, 0.1], [0, 0.5, 0]])
    p = (c[:, None, :] + tri[None] * s[:, None, None]).astype(np.float32).reshape(-1, 3)
    nrm = np.cross(p[1::3] - p[0::3], p[2::3] - p[0::3]); nrm /= np.maximum(np.linalg.norm(nrm, axis=1, keepdims=True), 1e-30)
    desc = SceneDesc(meshes=[MeshDesc("telescope", bake_vertices(p, np.repeat(nrm.astype(np.float32), 3, axis=0)), np.arange(3 * n, dtype=np.uint32).reshape(-1, 3), 0,
                                      double_sided=True)],
                     materials=[MaterialDesc.usd_preview_surface(diffuseColor=(0.8, 0.7, 0.6), roughness=0.5)],
                     camera=CameraDesc(position=(1.6, 0.0, 3.2), forward=(-0.05, 0.0, -1.0), up=(0, 1, 0), vfov=0.9))
    desc.rect_lights.append(RectLight(origin=(1.0, 0.0, 3.0), t0=(1, 0, 0), t1=(0, 1, 0), base_emission=(9, 9, 9), width=2.0, height=2.0))
    return desc


def test_tree_deeper_than_four_levels(gi, orc, monkeypatch):
    """The 8-entry-stack instantiation: a carried lane's stack column holds its entries across the trip boundary.  How many is not counted here: the host walk of
    test_deep_trees_parity's ray bundle, another ray family over this tree, holds 2 at most (tests/test_stack_fill_host.py), the tree's depth allows six; tests/test_gpu_stack_fill.py carries walks with the stack full.  64x36, spp 4."""
    _check(gi, orc, monkeypatch, _telescope(100, 1.1), RenderSettings(spp=4, max_bounces=4, progressive_accumulation=False), 64, 36, "telescope 64x36 spp 4")


def test_nee_renders_ignore_the_key(gi, orc, monkeypatch):
    """The NEE variants never carry (their shadow walk reuses the lane's walk state): with the key set the render is byte-equal to the key being absent."""
    desc = cornell_box()
    rs = RenderSettings(spp=4, max_bounces=8, next_event_estimation=True, progressive_accumulation=False)
    plain, st0 = _render(gi, monkeypatch, "", desc, rs, 64, 36)
    keyed, st1 = _render(gi, monkeypatch, "walk_carry=63", desc, rs, 64, 36)
    assert keyed.tobytes() == plain.tobytes()
    assert (st1["segments"], st1["shadowRays"]) == (st0["segments"], st0["shadowRays"])
    ref, cnt = orc.render(desc, rs, 64, 36, threads=4)
    assert st0["segments"] == cnt["segments"] and st0["shadowRays"] == cnt["shadow_rays"]
    assert_image_parity(plain, ref)

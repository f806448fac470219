"""The ring carry of the fused persistent kernel k_path (gi_path.hip, gi_traversal.h wave_step_ring).  The pending (ray, triangle) pairs of a wave live
across the steps of a trip's closest-hit loop: a triangle batch runs when 64 pairs are pending and ONE flush in the loop's last step tests the rest, instead of
a partial batch at the end of every step.  The hit key under atomicMin does not depend on when a pair is tested, so every render must be byte-equal with
GATLING_OPTIONS=ring_carry=0 (every step empties the ring) and with the key absent (the carry), `segments` included, whatever the walk carry and the lobe
parking do beside it; every image is also held to the CPU oracle bit for bit.  That the ring really is carried is shown by counting builds
(giCDebugPathRingStats), which take the key only when it is set explicitly."""
import copy
import os
import re

import numpy as np
import pytest

import path_matrix_cases as M
from gatling_amd.meshprep import bake_vertices
from gatling_amd.scene import CameraDesc, MaterialDesc, MeshDesc, RenderSettings, SceneDesc
from test_gpu_path_walk_carry import _telescope

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
gpu = pytest.mark.gpu

RS8 = RenderSettings(spp=8, max_bounces=8, progressive_accumulation=False)
RING = ("ring_carry=0", "")  # every step empties the ring / the default: the ring is carried
WALK = ("walk_carry=0", "", "walk_carry=63")
# name -> (scene, width, height, lobe_park values crossed in): the C2 cornell (class 1, the hot variant the benchmark runs, with the lobe parking), the diffuse
# cornell (class 0), the mixed-class box with cutouts and textures (the general variant) and the 7-level telescope (the 8-entry stack)
SCENES = {"A2": (lambda: M.scene("A2"), 96, 54, ("lobe_park=0", "")), "A1": (lambda: M.scene("A1"), 96, 54, ("",)),
          "B": (lambda: M.scene("B"), 96, 54, ("",)), "T": (lambda: _telescope(100, 1.1), 64, 36, ("",))}


def assert_image_parity(img, ref, what):
    assert img.shape == ref.shape and np.isfinite(img).all(), what
    bad = int((img.view(np.uint32) != ref.view(np.uint32)).any(axis=-1).sum())
    assert bad == 0, f"{what}: {bad} pixels differ bitwise"


def _render(gi, monkeypatch, options, desc, rs, w, h, count=False):
    """Two renders of a fresh scene (the second reuses every device buffer of the first); returns the image, the render's counters, the ring counters and
    the walk counters."""
    monkeypatch.setenv("GATLING_OPTIONS", options)
    sc = gi.Scene(copy.deepcopy(desc))
    try:
        if count:
            sc.set_option(gi.OPTION_COUNT_TRAVERSAL, 1)
        img = sc.render(rs, w, h).copy()
        st, ring, walk = sc.stats(), sc.path_ring_stats(), sc.path_walk_stats()
        again = sc.render(rs, w, h).copy()
        st2 = sc.stats()
    finally:
        sc.close()
    assert st["fusedPath"] == 1, st
    assert st2["segments"] == st["segments"] and again.tobytes() == img.tobytes(), options
    return img, st, ring, walk


_oracle = {}


def _reference(orc, name, desc, rs, w, h):
    """The oracle's frame of a scene, computed once for all the tests that need it."""
    if name not in _oracle:
        _oracle[name] = orc.render(desc, rs, w, h, threads=4)
    return _oracle[name]


# --- 1. same bits
@gpu
@pytest.mark.parametrize("walk", WALK, ids=[k or "walk_carry-default" for k in WALK])
@pytest.mark.parametrize("name", list(SCENES))
def test_same_bits(gi, orc, monkeypatch, name, walk):
    make, w, h, parks = SCENES[name]
    desc = make()
    ref, cnt = _reference(orc, name, desc, RS8, w, h)
    got = {}
    for park in parks:
        for ring in RING:
            key = ",".join(k for k in (walk, park, ring) if k)
            got[key] = _render(gi, monkeypatch, key, desc, RS8, w, h)
            print(f"{name} {w}x{h} [{key or 'default'}]: segments {got[key][1]['segments']} / {cnt['segments']}")
    first = next(iter(got.values()))
    for key, (img, st, ring, _) in got.items():
        assert img.tobytes() == first[0].tobytes() and st["segments"] == first[1]["segments"], (name, key)
        assert (st["segments"], st["samples"]) == (cnt["segments"], cnt["samples"]), (name, key, st, cnt)
        assert_image_parity(img, ref, (name, key))
        assert all(v == 0 for v in ring.values()), (name, key, ring)  # no counters without OPTION_COUNT_TRAVERSAL


# --- 2. the append that overflows the ring
QUADS = 6        # 12 triangles: one BVH8 node (8 slots of up to 3 triangles)
QUAD_HALF = 20.0


def _stack_scene():
    """QUADS quads of 40 x 40 units facing a camera at the origin, at z = -2, -2 again, -2.5, -3, -3.5 and -4.  At 4 units the frustum of the 64 x 36 frame is 6 x
    3.4 units wide, so every quad covers every pixel, whatever the pixel filter adds: every camera ray pierces all of them, and with an unbounded culling distance
    its one node step finds every leaf that holds a pierced triangle.  Quads 0 and 1 are exact duplicates with different materials: the same t in both, so the
    lower scene-order id (quad 0, red) must win wherever it is the nearest."""
    depths = [2.0, 2.0, 2.5, 3.0, 3.5, 4.0][:QUADS]
    colours = [(0.9, 0.1, 0.1), (0.1, 0.9, 0.1), (0.1, 0.1, 0.9), (0.8, 0.8, 0.1), (0.1, 0.8, 0.8), (0.8, 0.1, 0.8)]
    meshes = []
    for k, z in enumerate(depths):
        a = QUAD_HALF
        p = np.array([(-a, -a, -z), (a, -a, -z), (a, a, -z), (-a, -a, -z), (a, a, -z), (-a, a, -z)], np.float32)
        n = np.tile(np.array([(0.0, 0.0, 1.0)], np.float32), (6, 1))
        meshes.append(MeshDesc(f"quad{k}", bake_vertices(p, n), np.arange(6, dtype=np.uint32).reshape(-1, 3), k, id=k, double_sided=True))
    return SceneDesc(meshes=meshes, materials=[MaterialDesc.usd_preview_surface(diffuseColor=c, roughness=0.6) for c in colours],
                     camera=CameraDesc(position=(0, 0, 0), forward=(0, 0, -1), up=(0, 1, 0), vfov=0.8))


@gpu
def test_append_that_overflows_the_ring(gi, orc, monkeypatch):
    desc, w, h = _stack_scene(), 64, 36
    rs = RenderSettings(spp=8, max_bounces=8, progressive_accumulation=False)
    rs.clear_color = (0.25, 0.5, 0.75, 1.0)  # a path ends in the background: the image shows which duplicate was hit
    # on the CPU first: every quad covers the frustum at its depth with room to spare, so a camera segment tests at least one triangle of each quad (the leaf
    # that holds the pierced one); with the oracle's own segment count that is QUADS * samples / segments triangles per segment over the frame, or more
    half_w = np.tan(0.5 * desc.camera.vfov) * w / h
    assert all(QUAD_HALF > 4.0 * half_w * float(-m.vertices["pos"][:, 2].min()) for m in desc.meshes)
    ref, cnt = _reference(orc, "stack", desc, rs, w, h)
    assert cnt["samples"] == w * h * rs.spp and QUADS * cnt["samples"] >= 3 * cnt["segments"], cnt
    assert np.abs(ref[..., 0] - ref[..., 1]).max() > 0.0  # red and green differ: the duplicates can be told apart

    off = _render(gi, monkeypatch, "ring_carry=0", desc, rs, w, h)
    on = _render(gi, monkeypatch, "ring_carry=1", desc, rs, w, h)
    default = _render(gi, monkeypatch, "", desc, rs, w, h)
    for img, st, _, _ in (off, on, default):
        assert st["nodeCount"] == 1 and st["triangleCount"] == 2 * QUADS, st
        assert img.tobytes() == off[0].tobytes() and st["segments"] == off[1]["segments"]
    assert (default[1]["segments"], default[1]["samples"]) == (cnt["segments"], cnt["samples"])
    assert_image_parity(default[0], ref, "stack")

    counted = {k: _render(gi, monkeypatch, k, desc, rs, w, h, count=True) for k in ("ring_carry=0", "ring_carry=1")}
    for k, (img, st, ring, walk) in counted.items():
        print(f"stack counting build [{k}]: {ring}, trips {walk['phaseTrips']}, segments {st['segments']}, nodesVisited {st['nodesVisited']}, trisTested {st['trisTested']}")
        assert_image_parity(img, ref, ("stack", k))
        assert st["segments"] == cnt["segments"] and ring["pairs"] == st["trisTested"], (k, st, ring)
        assert st["trisTested"] >= 3 * st["segments"], (k, st)
        assert ring["ballotSteps"] > 0, (k, ring)  # a full wave's single step yields more than 128 pairs
    assert counted["ring_carry=0"][2]["flushes"] == 0


# --- 3. the carry really happens
@gpu
def test_counting_build_shows_the_carried_ring(gi, orc, monkeypatch):
    desc, w, h = M.scene("A2"), 96, 54
    ref, cnt = _reference(orc, "A2", desc, RS8, w, h)
    got = {k: _render(gi, monkeypatch, k, desc, RS8, w, h, count=True) for k in ("ring_carry=0", "ring_carry=1", "")}
    for k, (img, st, ring, walk) in got.items():
        print(f"A2 counting build [{k or 'key absent'}]: {ring}, trips {walk['phaseTrips']}, segments {st['segments']}, nodesVisited {st['nodesVisited']}, "
              f"trisTested {st['trisTested']}")
        assert_image_parity(img, ref, ("A2", k))
        assert (st["segments"], st["samples"]) == (cnt["segments"], cnt["samples"]), (k, st, cnt)
        assert ring["batches"] > 0 and ring["pairs"] == st["trisTested"], (k, st, ring)  # every tested pair went through a batch
    off, on, absent = (got[k][2] for k in ("ring_carry=0", "ring_carry=1", ""))
    trips = got["ring_carry=1"][3]["phaseTrips"]
    assert 0 < on["partialBatches"] <= on["flushes"] <= trips, (on, trips)  # partial batches happen in flushes only, and a trip has at most one flush
    assert on["batches"] < off["batches"], (on, off)
    # a lagging culling distance can only add work
    assert got["ring_carry=1"][1]["nodesVisited"] >= got["ring_carry=0"][1]["nodesVisited"] and on["pairs"] >= off["pairs"]
    # the key absent: a counting build does not carry, and its counters are those of ring_carry=0
    assert absent["flushes"] == 0 and off["flushes"] == 0 and absent == off, (absent, off)
    assert [got[""][1][f] for f in ("nodesVisited", "trisTested")] == [got["ring_carry=0"][1][f] for f in ("nodesVisited", "trisTested")]


# --- 4. host
def test_header_declares_the_query():
    text = open(os.path.join(ROOT, "include", "gi_c.h")).read()
    assert re.search(r"int\s+giCDebugPathRingStats\(const GiCScene\*\s*scene,\s*uint64_t\*\s*out\s*/\*\s*5\s*\*/\);", text)
    assert re.search(r"#define\s+GI_C_API_VERSION\s+8u?\b", text)


def test_library_exports_the_symbol():
    from gatling_amd import capi
    lib = capi.load_library()
    assert hasattr(lib, "giCDebugPathRingStats")
    assert lib.giCGetApiVersion() == 8


@gpu
def test_query_answers_zeros_without_counting(gi, monkeypatch):
    _, st, ring, walk = _render(gi, monkeypatch, "ring_carry=1", M.scene("A2"), RenderSettings(spp=1, max_bounces=4, progressive_accumulation=False), 32, 18)
    assert st["segments"] > 0 and all(v == 0 for v in ring.values()) and walk["phaseTrips"] == 0, (ring, walk)

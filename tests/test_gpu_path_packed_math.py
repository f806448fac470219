"""GPU parity (-m gpu): the fused kernel k_path (gi_path.hip) with the lean arithmetic of gi_device_math.h -- the division without the steps ordinary operands do
not need, beside the square root -- against the CPU oracle, which divides with the host's `/`: colour byte-equal, segments and samples equal, over the material
classes with NEE off and on, a scene whose every hit runs the GGX block, the general variant with its 8-entry stack, cutouts and a texture, and geometry that
sends operands out of the lean range (zero-area and edge-on triangles: det == 0; coincident triangles: the tie-break; unusable vertices).  Counting builds are
the dynamic-class instantiations: their images are held to the oracle too, their node and triangle counts to those of the same walks without the walk carry."""
import copy

import numpy as np
import pytest

from gatling_amd.meshprep import bake_vertices
from gatling_amd.scene import TEX_BASE_COLOR, TEX_WRAP_REPEAT, MeshDesc, RenderSettings, TextureBinding
from gatling_amd.scenes import cornell_box
from path_matrix_cases import scene as matrix_scene
from test_gpu_path_lobe_park import _reference, _render, assert_image_parity, scene_m
from test_hostile_inputs import sanitised

pytestmark = pytest.mark.gpu


def _settings(spp, bounces, nee=False):
    return RenderSettings(spp=spp, max_bounces=bounces, next_event_estimation=nee, progressive_accumulation=False)


def _hold(gi, orc, monkeypatch, name, desc, rs, w, h, ref_desc=None, count=False, options=""):
    ref, cnt = _reference(orc, name, ref_desc if ref_desc is not None else desc, rs, w, h)
    img, st, _ = _render(gi, monkeypatch, options, desc, rs, w, h, count=count)
    print(f"{name} {w}x{h} spp {rs.spp} nee {rs.next_event_estimation} count {count}: segments {st['segments']} / {cnt['segments']}, samples {st['samples']} / "
          f"{cnt['samples']}, nodesVisited {st['nodesVisited']}, trisTested {st['trisTested']}")
    assert (st["segments"], st["samples"]) == (cnt["segments"], cnt["samples"]), (name, st, cnt)
    if rs.next_event_estimation:
        assert st["shadowRays"] == cnt["shadow_rays"], (name, st, cnt)
    assert_image_parity(img, ref, name)
    return st


@pytest.mark.parametrize("nee", [False, True])
@pytest.mark.parametrize("klass", [0, 1, 2])
def test_cornell_by_class(gi, orc, monkeypatch, klass, nee):
    """Cornell, 96 x 54, spp 8, 8 bounces, one material class: the hot instantiations k_path<0 | 1 | 2, NEE off | on>."""
    name = ("A1", "A2", "A3")[klass]
    # (A2 without its light is the scene tests/test_gpu_path_lobe_park.py calls "A": one oracle render serves both files)
    _hold(gi, orc, monkeypatch, "A" if (klass, nee) == (1, False) else f"{name}-nee{int(nee)}", matrix_scene(name, nee), _settings(8, 8, nee), 96, 54)


def test_all_metal_cornell(gi, orc, monkeypatch):
    """Every hit draws a glossy lobe: ggx_sample's normalizes, its 1 / sqrt and its five quotients on every segment."""
    _hold(gi, orc, monkeypatch, "M", scene_m(), _settings(8, 8), 96, 54)


def _telescope_cutouts_textured():
    d = matrix_scene("C")
    yy, xx = np.mgrid[0:8, 0:8]
    checker = np.zeros((8, 8, 4), np.float32)
    checker[..., :3] = (0.2 + 0.7 * ((xx + yy) % 2))[..., None] * np.array([0.9, 0.8, 0.3], np.float32); checker[..., 3] = 1.0
    d.textures = [checker]
    d.materials[0].textures = {TEX_BASE_COLOR: TextureBinding(texture=0, wrap_s=TEX_WRAP_REPEAT, wrap_t=TEX_WRAP_REPEAT)}
    m = d.meshes[0]
    m.vertices = m.vertices.copy()
    m.vertices["u"] = m.vertices["pos"][:, 0] * 3.0; m.vertices["v"] = m.vertices["pos"][:, 1] * 3.0
    return d


@pytest.mark.parametrize("nee", [False, True])
def test_telescope_with_cutouts_and_a_texture(gi, orc, monkeypatch, nee):
    """100 triangles, a tree of 7 levels, every other triangle a stochastic cutout, the others textured: the general variant with the 8-entry stack."""
    _hold(gi, orc, monkeypatch, f"C-tex-nee{int(nee)}", _telescope_cutouts_textured(), _settings(4, 6, nee), 64, 36)


def _hostile_cornell():
    d = cornell_box()
    cam = np.asarray(d.camera.position, np.float64); fwd = np.asarray(d.camera.forward, np.float64); up = np.asarray(d.camera.up, np.float64)
    twin = [(-0.6, 0.5, -0.2), (0.1, 0.5, -0.2), (-0.6, 0.5, 0.6)]
    tris = [[(0.3, 0.2, 0.1)] * 3,                                                   # zero area: three times the same point
            [(-0.5, 0.0, 0.0), (0.0, 0.0, 0.0), (0.5, 0.0, 0.0)],                    # zero area: collinear
            [tuple(cam + 5.0 * fwd - 0.3 * up), tuple(cam + 6.0 * fwd), tuple(cam + 5.0 * fwd + 0.3 * up)],  # edge-on: its plane holds the camera
            twin, twin,                                                              # coincident within one mesh: the lower scene-order id wins
            [(0.2, -0.2, 0.3), (1e30, 0.0, 0.3), (0.2, 0.4, 0.3)],                   # a vertex at 1e30
            [(0.0, -0.5, -0.5), (0.3, -0.5, -0.5), (0.0, float("nan"), -0.2)]]        # a NaN vertex
    p = np.asarray(tris, np.float32).reshape(-1, 3)
    n = np.tile(np.array([0.0, -1.0, 0.0], np.float32), (len(p), 1))
    d.meshes.append(MeshDesc("hostile", bake_vertices(p, n), np.arange(len(p), dtype=np.uint32).reshape(-1, 3), 2, id=8, double_sided=True))
    d.meshes.append(MeshDesc("twin of another mesh", bake_vertices(np.asarray(twin, np.float32), n[:3]), np.arange(3, dtype=np.uint32).reshape(-1, 3), 3, id=9,
                             double_sided=True))
    return d


@pytest.mark.parametrize("nee", [False, True])
def test_hostile_geometry(gi, orc, monkeypatch, nee):
    """Zero-area triangles, a triangle edge-on to the camera, coincident triangles inside a mesh and across meshes, a vertex at 1e30 and a NaN vertex in the cornell
    box (the library drops the faces of unusable vertices; the oracle renders the scene written that way)."""
    d = _hostile_cornell()
    if nee:
        d.rect_lights = matrix_scene("A2", True).rect_lights
    st = _hold(gi, orc, monkeypatch, f"H-nee{int(nee)}", d, _settings(8, 8, nee), 96, 54, ref_desc=sanitised(copy.deepcopy(d)))
    assert st["inactiveTriangleCount"] == 2, st


@pytest.mark.parametrize("name,make", [("A", lambda: matrix_scene("A2")), ("M", scene_m), ("H-nee0", _hostile_cornell)])
def test_counting_builds(gi, orc, monkeypatch, name, make):
    """The counting (dynamic-class) instantiations: the oracle's image, and node / triangle counts that do not depend on the trip a walk is finished in."""
    ref_desc = sanitised(make()) if name.startswith("H") else None
    a = _hold(gi, orc, monkeypatch, name, make(), _settings(8, 8), 96, 54, ref_desc=ref_desc, count=True)
    b = _hold(gi, orc, monkeypatch, name, make(), _settings(8, 8), 96, 54, ref_desc=ref_desc, count=True, options="walk_carry=0")
    assert a["nodesVisited"] > 0 and (a["nodesVisited"], a["trisTested"]) == (b["nodesVisited"], b["trisTested"]), (a, b)

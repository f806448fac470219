"""The case table of tests/test_gpu_path_matrix.py (GPU) and tests/test_path_matrix_inputs.py (CPU): scenes, settings and the explicit list of cases that hold
k_path's kernel variants and schedule switches to the CPU oracle TOGETHER.  No test lives here.

Scenes (all LDS-resident):
  A1 / A2 / A3  cornell with one material class (diffuse / UsdPreviewSurface / OpenPBR): the hot variants k_path<0>, <1>, <2>
  B             cornell with the three classes mixed, a stochastic cutout (opacity 0.4) on the white material and a textured colour + textured opacity on the red
                wall: the general variant, 4-entry stack
  C / C1        the telescope of tests/test_gpu_path_walk_carry.py (100 triangles, ratio 1.1, a tree of 7 levels) as two meshes, every other triangle with a
                cutout material: the general variant, 8-entry stack -- how full is not counted here (the host walk of test_deep_trees_parity's ray bundle over this tree
                holds 2 entries, tests/test_stack_fill_host.py; the stack is filled in tests/test_gpu_stack_fill.py).  C1 is C through the camera of the 33 x 1 frame (a slice along the telescope's axis)
  D / D1        a cluster of 6 quads (12 triangles) right of the view axis.  D at 32 x 18: a miss rectangle 2 .. 20 columns wide.  D1 at 1 x 36: activeWidth == 1.
                Twelve triangles fit one BVH8 node, so every walk there is ONE step and no lane can be carried; D2 / D3 are the same cluster and cameras with
                14 quads (28 triangles, a root with three child nodes) for the cases that claim carried lanes under a narrow rectangle.
                The rectangle keeps a margin of a pixel (and the filter's reach) either side of the projected bounds, so inside a WIDER frame a rectangle one
                column wide holds no pixel a ray can hit the scene through; a frame one pixel wide is the only one in which activeWidth == 1 and rays hit.  Its
                rows make the rectangle a proper subset, and a wave's 64 work items there are 64 (row, sample) pairs of that one column.

Axes (a Case's fields, in order):
  carry   GATLING_OPTIONS walk_carry: "0", "1", "d" (key absent: the default, 8), "63"
  mr, br, wo   miss_rect, bounds_retire, work_order: 0 | 1, always set explicitly
  nee     next-event estimation, with one rect light
  share   0: the whole frame; 1: image rows 1, 4, 7 ... (rank 1 of 3 of an interleaved row share)
  calls   "one": one call of `spp` samples, no progressive accumulation; "prog2": two progressive calls of spp 1; "win4": seven progressive calls of spp 1 with
          a sample look-ahead of 4 -- windows of 1, 2 and 4 calls, the last served over four calls
  mb      max_bounces 1 | 8;  rr: rr_bounce_offset "0" | "d" (the default, 3);  bg: clear colour "black" | "colour" (0.25, 0.5, 0.75, 1)

The table covers every pair of axis values at least once per kernel family (test_path_matrix_inputs.py checks that and prints the coverage), holds one "many trips"
case (96 x 54, spp 8) per kernel variant the scenes select (A1 .. A3, B, C with NEE off and on: ten of the twenty instantiations; no scene here is one class
over a tree deeper than four levels, so the six hot stack-8 instantiations have no case here -- tests/test_gpu_stack_fill.py runs them --, and the counting ones run in the carry proofs), and the combinations
marked NAMED.

work_order is INERT in the fused kernel: gi_render.cpp reads it for the wavefront pipeline only, k_path always hands work out sample-major.  The axis is here
because a switch that is promised to do nothing to fused frames must go on doing nothing; its pairs, and "look-ahead window + sample-major order", are no
coverage of kernel code.

Which rows carry lanes.  Every row with NEE off and walk_carry != 0 claims carried lanes (carries(c)), and the table may hold such a row only where lanes CAN be
carried: not on D / D1 (one node: a walk is one step), and with K = 63 only with bounds_retire = 0 on a frame of 512 pixels or more -- with bounds_retire = 1 a
wave of these frames holds only the rays that reach the bounds, fewer than 64, and K = 63 (carry when 64 entered and one has finished) never triggers.  The
pairs of (carry, x) those rules exclude are covered by NEE rows, where the key is ignored by design and the row holds exactly that.  Every claiming row below
96 x 54 x 8 proves its claim on the GPU with a counting build at its own scene, frame, rows, settings and K (test_gpu_path_matrix.py); the 96 x 54 rows
inherit the proof of test_counting_build_shows_the_carried_lanes.  test_path_matrix_inputs.py rejects a claiming row that breaks these rules."""
from __future__ import annotations

from collections import namedtuple

import numpy as np

from gatling_amd.meshprep import bake_vertices
from gatling_amd.scene import (MAT_DIFFUSE, MAT_OPEN_PBR, MAT_USD_PREVIEW_SURFACE, TEX_BASE_COLOR, TEX_OPACITY, TEX_WRAP_CLAMP, TEX_WRAP_REPEAT, CameraDesc,
                               MaterialDesc, MeshDesc, RectLight, RenderSettings, SceneDesc, TextureBinding)
from gatling_amd.scenes import _look_at_camera, cornell_box

Case = namedtuple("Case", "id scene w h spp carry mr br wo nee share calls mb rr bg")
AXES = {"carry": ("0", "1", "d", "63"), "mr": (0, 1), "br": (0, 1), "wo": (0, 1), "nee": (0, 1), "share": (0, 1), "calls": ("one", "prog2", "win4"),
        "mb": (1, 8), "rr": ("0", "d"), "bg": ("black", "colour")}
CALLS = {"one": 1, "prog2": 2, "win4": 7}
FAMILY = {"A1": "hot", "A2": "hot", "A3": "hot", "D": "hot", "D1": "hot", "D2": "hot", "D3": "hot", "B": "general-4", "C": "general-8", "C1": "general-8"}
CLASS_MASK = {"A1": 1 << MAT_DIFFUSE, "A2": 1 << MAT_USD_PREVIEW_SURFACE, "A3": 1 << MAT_OPEN_PBR, "D": 1 << MAT_USD_PREVIEW_SURFACE,
              "D1": 1 << MAT_USD_PREVIEW_SURFACE, "D2": 1 << MAT_USD_PREVIEW_SURFACE, "D3": 1 << MAT_USD_PREVIEW_SURFACE, "B": 7, "C": 1 << MAT_USD_PREVIEW_SURFACE, "C1": 1 << MAT_USD_PREVIEW_SURFACE}
RECT_WIDTH = {"D": (2, 20), "D1": (1, 1), "D2": (2, 20), "D3": (1, 1)}  # activeWidth the case's frame must give

CASES = [
    # --- hot (one material class, no texture, no cutout: k_path<0 | 1 | 2, ...>): 18 cases
    Case("h01", "A1", 96, 54, 8, "0", 0, 0, 1, 0, 0, "one", 8, "0", "colour"),  # many trips, <0, no NEE>
    Case("h02", "A1", 96, 54, 8, "63", 1, 1, 0, 1, 0, "one", 8, "d", "black"),  # many trips, <0, NEE>
    Case("h03", "A2", 96, 54, 8, "1", 1, 0, 0, 0, 0, "one", 8, "0", "black"),  # many trips, <1, no NEE>
    Case("h04", "A2", 96, 54, 8, "d", 0, 1, 1, 1, 0, "one", 8, "d", "colour"),  # many trips, <1, NEE>
    Case("h05", "A3", 96, 54, 8, "63", 1, 0, 1, 0, 0, "one", 8, "d", "colour"),  # NAMED: <2, no NEE> at walk_carry=63, many trips; every camera ray enters a loop, so 64 lanes do
    Case("h06", "A3", 96, 54, 8, "1", 0, 1, 1, 1, 0, "one", 8, "0", "black"),  # many trips, <2, NEE>
    Case("h07", "D", 32, 18, 4, "0", 1, 1, 0, 0, 0, "one", 1, "d", "black"),  # narrow rectangle (activeWidth 2..20): a wave's work items span several rows
    Case("h08", "D1", 1, 36, 4, "d", 1, 1, 0, 1, 0, "one", 1, "0", "colour"),  # activeWidth == 1 (12 triangles: one node, walks of one step)
    Case("h09", "D3", 1, 36, 4, "1", 1, 1, 0, 0, 0, "one", 8, "d", "colour"),  # NAMED: carried lanes + activeWidth == 1
    Case("h10", "A2", 64, 36, 1, "d", 0, 0, 0, 0, 1, "win4", 8, "d", "black"),  # NAMED: carried lanes + look-ahead window + sample-major order
    Case("h11", "D2", 32, 18, 3, "1", 1, 1, 1, 0, 1, "one", 8, "0", "colour"),  # narrow rectangle cut by the row share, lanes carried
    Case("h12", "A1", 64, 36, 1, "63", 0, 0, 1, 1, 1, "prog2", 1, "0", "black"),  # pair coverage
    Case("h13", "A2", 48, 27, 1, "1", 1, 1, 1, 1, 0, "win4", 1, "0", "colour"),  # pair coverage
    Case("h14", "A3", 64, 36, 1, "d", 1, 1, 0, 0, 0, "prog2", 8, "d", "colour"),  # pair coverage
    Case("h15", "D", 32, 18, 1, "0", 1, 1, 0, 1, 1, "prog2", 8, "0", "colour"),  # pair coverage
    Case("h16", "A1", 64, 36, 1, "0", 1, 1, 1, 1, 1, "win4", 1, "0", "black"),  # pair coverage
    Case("h17", "A2", 48, 27, 1, "1", 0, 0, 0, 1, 1, "prog2", 8, "d", "black"),  # pair coverage
    Case("h18", "A3", 64, 36, 1, "63", 1, 1, 0, 1, 0, "win4", 1, "d", "black"),  # pair coverage
    # --- general-4 (scene B: k_path<KLASS_DYNAMIC, TEXTURED, CUTOUT>, 4-entry stack): 14 cases
    Case("g01", "B", 96, 54, 8, "d", 1, 0, 1, 0, 0, "one", 8, "d", "colour"),  # many trips, general variant, stack 4, no NEE
    Case("g02", "B", 96, 54, 8, "63", 0, 1, 0, 1, 0, "one", 8, "0", "black"),  # many trips, general variant, stack 4, NEE
    Case("g03", "B", 8, 4, 1, "1", 1, 1, 0, 0, 0, "one", 8, "0", "colour"),  # fewer work items than a wave
    Case("g04", "B", 64, 36, 3, "1", 0, 0, 1, 0, 1, "one", 8, "d", "black"),  # NAMED: carried lanes + cutout + row share
    Case("g05", "B", 64, 36, 1, "0", 1, 1, 1, 1, 1, "prog2", 1, "d", "colour"),  # pair coverage
    Case("g06", "B", 40, 23, 1, "d", 0, 0, 0, 1, 1, "win4", 1, "0", "black"),  # pair coverage
    Case("g07", "B", 64, 36, 1, "0", 0, 0, 0, 0, 0, "prog2", 8, "0", "black"),  # pair coverage
    Case("g08", "B", 40, 23, 1, "63", 1, 0, 1, 0, 0, "win4", 1, "d", "black"),  # pair coverage
    Case("g09", "B", 64, 36, 1, "1", 0, 1, 0, 1, 1, "win4", 1, "d", "colour"),  # pair coverage
    Case("g10", "B", 40, 23, 1, "63", 0, 1, 1, 1, 1, "prog2", 8, "0", "colour"),  # pair coverage
    Case("g11", "B", 64, 36, 1, "0", 0, 1, 1, 0, 1, "win4", 8, "0", "colour"),  # pair coverage
    Case("g12", "B", 40, 23, 1, "d", 0, 1, 1, 0, 0, "prog2", 8, "0", "colour"),  # pair coverage
    Case("g13", "B", 64, 36, 3, "0", 0, 0, 0, 0, 0, "one", 1, "d", "black"),  # pair coverage
    Case("g14", "B", 40, 23, 1, "1", 0, 1, 0, 0, 0, "prog2", 8, "d", "black"),  # pair coverage
    # --- general-8 (scene C: the same variant with the 8-entry stack): 13 cases
    Case("t01", "C", 96, 54, 8, "d", 0, 0, 0, 0, 0, "one", 8, "0", "colour"),  # many trips, general variant, stack 8, no NEE
    Case("t02", "C", 96, 54, 8, "0", 1, 1, 1, 1, 0, "one", 8, "d", "black"),  # many trips, general variant, stack 8, NEE
    Case("t03", "C1", 33, 1, 2, "1", 1, 0, 0, 1, 0, "one", 1, "0", "black"),  # one row, 33 work items per sample: scene C through a lens that cuts a thin slice along its axis
    Case("t04", "C", 64, 36, 4, "d", 0, 1, 1, 0, 1, "one", 8, "d", "colour"),  # NAMED: carried lanes + cutout + row share, 8-entry stack
    Case("t05", "C", 64, 36, 1, "63", 1, 0, 0, 0, 1, "prog2", 1, "d", "colour"),  # pair coverage
    Case("t06", "C", 47, 29, 1, "63", 0, 1, 1, 1, 1, "win4", 1, "0", "black"),  # pair coverage
    Case("t07", "C", 64, 36, 1, "1", 1, 0, 1, 0, 1, "win4", 8, "d", "colour"),  # pair coverage
    Case("t08", "C", 47, 29, 1, "0", 0, 1, 0, 0, 1, "prog2", 1, "0", "black"),  # pair coverage
    Case("t09", "C", 64, 36, 1, "1", 0, 1, 1, 1, 0, "prog2", 8, "d", "colour"),  # pair coverage
    Case("t10", "C", 47, 29, 1, "d", 1, 0, 0, 1, 0, "win4", 1, "d", "black"),  # pair coverage
    Case("t11", "C", 64, 36, 4, "63", 0, 1, 0, 1, 0, "one", 8, "0", "black"),  # pair coverage
    Case("t12", "C", 47, 29, 1, "0", 0, 0, 0, 0, 1, "win4", 1, "0", "colour"),  # pair coverage
    Case("t13", "C", 64, 36, 1, "d", 0, 1, 1, 1, 0, "prog2", 1, "d", "colour"),  # pair coverage
]
assert len(CASES) <= 48 and len({c.id for c in CASES}) == len(CASES)
BY_ID = {c.id: c for c in CASES}


def _cornell_light():
    return RectLight(origin=(0, 0, 0.9), t0=(1, 0, 0), t1=(0, -1, 0), base_emission=(10, 10, 10), width=0.7, height=0.5)


def _cornell_open_pbr():
    d = cornell_box()
    d.materials = [MaterialDesc.open_pbr(name="Light", base_color=(0.8, 0.8, 0.8), emission_luminance=1.0, emission_color=(8.5, 6, 4)),
                   MaterialDesc.open_pbr(name="White", base_color=(0.8, 0.8, 0.8)), MaterialDesc.open_pbr(name="Red", base_color=(1, 0, 0), specular_roughness=0.5),
                   MaterialDesc.open_pbr(name="Green", base_color=(0, 1, 0), coat_weight=0.5, coat_roughness=0.2)]
    return d


def _scene_b(opacity=0.4):
    """`opacity`: the control renders of the CPU test replace both cutouts by 1 (nothing is ever rejected) or 0 (nothing is ever accepted)."""
    d = cornell_box()
    yy, xx = np.mgrid[0:8, 0:8]
    checker = np.zeros((8, 8, 4), np.float32)
    checker[..., :3] = (0.2 + 0.7 * ((xx + yy) % 2))[..., None] * np.array([1.0, 0.3, 0.2], np.float32); checker[..., 3] = 1.0
    ramp = np.zeros((4, 16, 4), np.float32)
    ramp[..., 1] = np.linspace(0.15, 0.95, 16, dtype=np.float32)[None, :]; ramp[..., 3] = 1.0   # green channel: opacity 0.15 .. 0.95 along u
    d.textures = [checker, ramp]
    d.materials[1].params[14] = opacity                                   # White (floor, ceiling, back wall, tall box): stochastic cutout
    red = d.materials[2]
    red.textures = {TEX_BASE_COLOR: TextureBinding(texture=0, wrap_s=TEX_WRAP_REPEAT, wrap_t=TEX_WRAP_REPEAT)}
    if opacity == 0.4:
        red.textures[TEX_OPACITY] = TextureBinding(texture=1, wrap_s=TEX_WRAP_CLAMP, wrap_t=TEX_WRAP_CLAMP, channel=1)
    else:
        red.params[14] = opacity
    d.materials[3] = MaterialDesc.open_pbr(name="Green", base_color=(0, 1, 0), specular_roughness=0.4)
    d.materials.append(MaterialDesc.usd_preview_surface(name="Chalk", diffuseColor=(0.7, 0.7, 0.5), klass=MAT_DIFFUSE))
    d.meshes[7].material = 4                                              # the short box: the diffuse class
    left = d.meshes[4]                                                    # the red wall gets texture coordinates: (y, z) of the wall, two tiles each way
    left.vertices = left.vertices.copy()
    left.vertices["u"] = left.vertices["pos"][:, 1] + 1.0; left.vertices["v"] = left.vertices["pos"][:, 2] + 1.0
    return d


def _scene_c(opacity=0.4, n=100, ratio=1.1):
    i = np.arange(n, dtype=np.float64)
    s = ratio ** (-i)
    c = np.stack([s * 3.0, 0.3 * s * ((i % 5) - 2), 0.05 * s * (i % 3)], 1)
    tri = np.array([[0, -0.5, 0], [1, 0, 0.1], [0, 0.5, 0]])
    p = (c[:, None, :] + tri[None] * s[:, None, None]).astype(np.float32)
    nrm = np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]); nrm /= np.maximum(np.linalg.norm(nrm, axis=1, keepdims=True), 1e-30)
    meshes = []
    for k in (0, 1):                                                      # even triangles: opaque; odd triangles: the cutout material
        pk = p[k::2].reshape(-1, 3)
        meshes.append(MeshDesc(f"telescope{k}", bake_vertices(pk, np.repeat(nrm[k::2].astype(np.float32), 3, axis=0)),
                               np.arange(len(pk), dtype=np.uint32).reshape(-1, 3), k, id=k, double_sided=True))
    d = SceneDesc(meshes=meshes,
                  materials=[MaterialDesc.usd_preview_surface(diffuseColor=(0.8, 0.7, 0.6), roughness=0.5),
                             MaterialDesc.usd_preview_surface(diffuseColor=(0.5, 0.7, 0.9), roughness=0.4, opacity=opacity)],
                  camera=CameraDesc(position=(1.6, 0.0, 3.2), forward=(-0.05, 0.0, -1.0), up=(0, 1, 0), vfov=0.9))
    d.rect_lights.append(RectLight(origin=(1.0, 0.0, 3.0), t0=(1, 0, 0), t1=(0, 1, 0), base_emission=(9, 9, 9), width=2.0, height=2.0))
    return d


def _scene_d(narrow, quads=6, ratio=1.0):
    """`quads` quads stacked along z over [-1.9, 1.9] (heights shrinking by `ratio`), x from 1.0 to at most 2.2, alternately at y = 0 and y = 0.4 and
    overlapping a little, so that some bounces meet a neighbour.  Six quads (12 triangles) fit ONE BVH8 node: every walk through them is a single step and no
    lane can ever be carried.  Fourteen at ratio 1.15 (28 triangles) give a root with three child nodes, walks of one to four steps: the cases that claim carried
    lanes under a narrow rectangle use those (D2, D3)."""
    pts, nrm = [], []
    unit = 3.8 / sum(ratio ** -k for k in range(quads))
    z = -1.9
    for k in range(quads):
        s = ratio ** -k
        z0, z1, y, x1 = z, z + 1.19 * unit * s, 0.4 * (k % 2), 1.0 + 1.2 * max(s, 0.3)
        z += unit * s
        q = [(1.0, y, z0), (x1, y + 0.1, z0), (x1, y + 0.1, z1), (1.0, y, z0), (x1, y + 0.1, z1), (1.0, y, z1)]
        e = np.cross(np.subtract(q[1], q[0]), np.subtract(q[2], q[0])); e /= np.linalg.norm(e)
        pts += q; nrm += [e] * 6
    d = SceneDesc(meshes=[MeshDesc("cluster", bake_vertices(np.asarray(pts, np.float32), np.asarray(nrm, np.float32)),
                                   np.arange(6 * quads, dtype=np.uint32).reshape(-1, 3), 0, double_sided=True)],
                  materials=[MaterialDesc.usd_preview_surface(diffuseColor=(0.7, 0.6, 0.3), roughness=0.6)])
    # D: the cluster right of the view axis of a 40 degree lens.  D1: a 90 degree lens over a frame one pixel wide, the column through the cluster, looking up a little
    d.camera = _look_at_camera((1.6, -6, 0), (1.6, 0, 1.5), (0, 0, 1), 90.0) if narrow else _look_at_camera((0, -6, 0), (0, 0, 0), (0, 0, 1), 40.0)
    return d


def scene(name, nee=False, opacity=0.4):
    """A fresh SceneDesc of the named scene; with `nee` the cornell boxes and the cluster get their rect light (the telescope always has one)."""
    if name in ("A1", "A2", "A3"):
        d = {"A1": lambda: cornell_box(MAT_DIFFUSE), "A2": cornell_box, "A3": _cornell_open_pbr}[name]()
    elif name == "B":
        d = _scene_b(opacity)
    elif name in ("C", "C1"):
        d = _scene_c(opacity)
        if name == "C1":  # for the 33 x 1 frame (one pixel high, 33 wide): a pixel is 0.12 units at the telescope, the row a slice along its axis from x = 0 to 4
            d.camera = CameraDesc(position=(2.0, 0.0, 3.2), forward=(0.0, 0.0, -1.0), up=(0, 1, 0), vfov=0.0375)
        return d
    else:
        d = _scene_d(name in ("D1", "D3"), *((14, 1.15) if name in ("D2", "D3") else (6, 1.0)))
        if nee:
            d.rect_lights = [RectLight(origin=(1.6, -3.0, 0.0), t0=(1, 0, 0), t1=(0, 0, 1), base_emission=(12, 12, 12), width=1.5, height=1.5)]
        return d
    if nee:
        d.rect_lights = [_cornell_light()]
    return d


def case_scene(c, opacity=0.4):
    return scene(c.scene, bool(c.nee), opacity)


def settings(c):
    rs = RenderSettings(spp=c.spp, max_bounces=c.mb, next_event_estimation=bool(c.nee), progressive_accumulation=c.calls != "one")
    if c.rr == "0":
        rs.rr_bounce_offset = 0
    rs.clear_color = (0.0, 0.0, 0.0, 0.0) if c.bg == "black" else (0.25, 0.5, 0.75, 1.0)
    return rs


def options(c, carry=None):
    """GATLING_OPTIONS of a case (`carry`: override the case's walk_carry)."""
    k = c.carry if carry is None else str(carry)
    return f"miss_rect={c.mr},bounds_retire={c.br},work_order={c.wo}" + ("" if k == "d" else f",walk_carry={k}")


def rows_of(c):
    """(row_list for the oracle or None, keyword arguments of Scene.render)"""
    if not c.share:
        return None, {}
    return list(range(1, c.h, 3)), {"rows": (1, c.h), "row_stride": 3}


_frames = {}


def oracle_frames(orc, c, opacity=0.4, calls=None):
    """[(image, counters)] of the case's calls by the oracle (progressive calls blend over the previous image).  Computed once per distinct input, never changed."""
    n = CALLS[c.calls] if calls is None else calls
    key = (c.scene, c.w, c.h, c.spp, c.nee, c.share, c.calls, c.mb, c.rr, c.bg, opacity, n)
    if key not in _frames:
        desc, rs = case_scene(c, opacity), settings(c)
        row_list, _ = rows_of(c)
        out, prev = [], None
        for k in range(n):
            img, cnt = orc.render(desc, rs, c.w, c.h, threads=4, row_list=row_list, sample_offset=k * rs.spp, prev_color=prev)
            img.setflags(write=False)
            out.append((img, cnt)); prev = img if c.calls != "one" else None
        _frames[key] = out
    return _frames[key]


def carries(c):
    """The row claims that lanes are carried: the NEE-off variants carry, the NEE ones ignore the key."""
    return not c.nee and c.carry != "0"


def proof_k(c):
    """K of the row's own carry proof, or None: rows that do not claim, and the 96 x 54 x 8 rows (proven by test_counting_build_shows_the_carried_lanes)."""
    if not carries(c) or (c.w, c.h, c.spp) == (96, 54, 8):
        return None
    return 8 if c.carry == "d" else int(c.carry)


def pair_coverage():
    """{family: {((axis, value), (axis, value)): [case ids]}} over the table"""
    import itertools
    cov = {}
    for c in CASES:
        f = cov.setdefault(FAMILY[c.scene], {})
        for a, b in itertools.combinations(AXES, 2):
            f.setdefault(((a, getattr(c, a)), (b, getattr(c, b))), []).append(c.id)
    return cov

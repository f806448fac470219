"""The matrix of tests/test_gpu_path_matrix.py is not vacuous (no GPU needed): conditions on its INPUTS, shown by the CPU oracle and the host's rectangle code
alone.  For every case of the table (tests/path_matrix_cases.py):
  * the camera sees the scene and its surroundings: the fraction of camera rays that hit lies strictly between 0.05 and 0.95;
  * scenes B and C: some cutout candidate is rejected and some is accepted -- the case's first frame (image or counters) differs from the control render with every cutout opaque
    (opacity 1: nothing is ever rejected) and from the one with every cutout at opacity 0 (nothing is ever accepted);
  * scene D: the miss rectangle is a proper subset of the frame and as wide as the case says (2 .. 20 columns, or exactly 1);
  * next-event estimation traces shadow rays.
And for the table as a whole: every pair of axis values occurs in every kernel family, each kernel variant the scenes select has its many-trips case, every row that claims carried lanes can carry them, the sizes stay small."""
import dataclasses
import itertools

import numpy as np
import pytest

import path_matrix_cases as M
from gatling_amd import capi
from test_miss_rect_host import scene_bounds


@pytest.mark.parametrize("case", M.CASES, ids=[c.id for c in M.CASES])
def test_case_inputs_exercise_what_the_case_is_for(orc, case):
    c = case
    frame, cnt = M.oracle_frames(orc, c, calls=1)[0]
    row_list, _ = M.rows_of(c)
    # camera rays alone: one bounce, no shadow rays -- every segment is a camera ray, `hits` counts those that met a triangle they were not let through
    rs1 = dataclasses.replace(M.settings(c), max_bounces=1, next_event_estimation=False, spp=min(c.spp, 2), progressive_accumulation=False)
    _, cam = orc.render(M.case_scene(c), rs1, c.w, c.h, threads=4, row_list=row_list)
    assert cam["segments"] == cam["samples"] > 0
    hit = cam["hits"] / cam["segments"]
    print(f"{c.id}: {c.scene} {c.w}x{c.h}: {cam['hits']} of {cam['segments']} camera rays hit ({hit:.3f}); first call: {cnt['segments']} segments, "
          f"{cnt['shadow_rays']} shadow rays")
    assert 0.05 < hit < 0.95
    if c.nee:
        assert cnt["shadow_rays"] > 0
    if c.scene in ("B", "C", "C1"):
        # (image and counters: with one bounce over a black background every image is black, but a rejected candidate still changes what is hit)
        what = lambda img, n: (img.tobytes(), n["hits"], n["segments"], n["shadow_rays"])
        assert what(*M.oracle_frames(orc, c, opacity=1.0, calls=1)[0]) != what(frame, cnt), "no cutout candidate was rejected"
        assert what(*M.oracle_frames(orc, c, opacity=0.0, calls=1)[0]) != what(frame, cnt), "no cutout candidate was accepted"
    if c.scene in M.RECT_WIDTH:
        desc = M.case_scene(c)
        x0, y0, x1, y1 = capi.miss_rect(scene_bounds(desc), desc.camera, M.settings(c), c.w, c.h)
        lo, hi = M.RECT_WIDTH[c.scene]
        print(f"{c.id}: miss rectangle {(x0, y0, x1, y1)} of {c.w}x{c.h}")
        assert lo <= x1 - x0 <= hi and y1 > y0
        assert (x1 - x0) * (y1 - y0) < c.w * c.h
        if c.share:  # the share's rows straddle the rectangle or lie inside it: some row of the share is in it
            assert any(y0 <= r < y1 for r in row_list)


def test_table_covers_every_pair_of_axis_values_in_every_kernel_family():
    cov = M.pair_coverage()
    assert set(cov) == {"hot", "general-4", "general-8"}
    for fam, seen in cov.items():
        missing = [(a, va, b, vb) for a, b in itertools.combinations(M.AXES, 2) for va in M.AXES[a] for vb in M.AXES[b] if ((a, va), (b, vb)) not in seen]
        n = sum(1 for c in M.CASES if M.FAMILY[c.scene] == fam)
        print(f"{fam}: {n} cases, {len(seen)} (axis value, axis value) pairs seen, {len(missing)} missing")
        assert not missing, (fam, missing)


def test_table_holds_the_named_cases_and_stays_small():
    cs = M.CASES
    assert len(cs) <= 48
    many = {(c.scene, c.nee) for c in cs if (c.w, c.h, c.spp, c.calls, c.mb) == (96, 54, 8, "one", 8)}
    assert many >= {(s, n) for s in ("A1", "A2", "A3", "B", "C") for n in (0, 1)}                     # every kernel variant these scenes select runs many trips once
    for c in cs:
        assert c.spp <= 4 and c.w * c.h <= 64 * 36 or (c.w, c.h, c.spp) == (96, 54, 8), c
        assert c.calls == "one" or c.spp == 1, c
        assert all(getattr(c, a) in vs for a, vs in M.AXES.items()), c
    carried = [c for c in cs if M.carries(c)]
    for c in carried:  # a row that claims carried lanes sits where lanes can be carried, and is proven: at 96 x 54 x 8 by the counting runs there, else by its own
        assert c.scene not in ("D", "D1"), c                                                           # one BVH8 node: every walk is one step
        assert c.carry != "63" or (c.br == 0 and c.w * c.h >= 512), c                                  # K = 63 needs 64 lanes in a loop: every camera ray traced
        assert M.proof_k(c) is not None or (c.w, c.h, c.spp) == (96, 54, 8), c
    assert all(M.proof_k(c) is None for c in cs if not M.carries(c))
    assert any(c.scene in ("B", "C") and c.share for c in carried)                                     # carried lanes + cutout + row share
    assert any(c.scene == "D3" and c.mr and c.br and c.carry == "1" for c in carried)                   # carried lanes + activeWidth == 1 (a tree of two levels)
    assert any(c.scene == "D1" and c.mr and c.br for c in cs)                                          # activeWidth == 1 on the cluster of 12 triangles
    assert any(c.calls == "win4" and c.wo == 0 for c in carried)                                       # carried lanes + look-ahead window + sample-major order
    assert any(c.scene == "A3" and c.carry == "63" and c.br == 0 and (c.w, c.h, c.spp) == (96, 54, 8) for c in carried)  # <2, no NEE> at walk_carry=63
    assert any((c.scene, c.w, c.h, c.spp) == ("B", 8, 4, 1) for c in cs) and any((c.scene, c.w, c.h) == ("C1", 33, 1) for c in cs)
    assert any(c.scene == "D" and c.mr and c.br for c in cs)


def _tree_depth(desc):
    """Depth of the host builder's BVH8 over the scene's triangles in scene order (giCDebugValidateBvh: host only)."""
    import ctypes as C
    tris = []
    for m in desc.meshes:
        p = np.asarray(m.vertices)["pos"].reshape(-1, 3).astype(np.float64)
        p = (np.concatenate([p, np.ones((len(p), 1))], axis=1) @ np.asarray(m.transform, np.float64).reshape(4, 4))[:, :3]
        tris.append(p[np.asarray(m.faces, np.int64).reshape(-1)])
    v = np.ascontiguousarray(np.concatenate(tris), np.float32)
    nodes, depth = C.c_uint32(0), C.c_uint32(0)
    assert capi.load_library().giCDebugValidateBvh(v.ctypes.data_as(capi._FP), len(v) // 3, C.byref(nodes), C.byref(depth)) == 0
    return depth.value


def test_scenes_select_the_kernel_families_on_the_host():
    """What the class-state query will say on the device is decided by the materials: one class each for A1 .. A3 and D, three for B, a cutout in B and C, a
    texture in B; C's tree is deeper than four levels (the 8-entry stack) and the others' are not; the 12-triangle cluster D is a single node."""
    for name in ("A1", "A2", "A3", "D", "D1", "D2", "D3"):
        d = M.scene(name, nee=True)
        used = {d.materials[m.material].klass for m in d.meshes}
        assert {1 << k for k in used} == {M.CLASS_MASK[name]}
        assert all(d.materials[m.material].params[14] == 1.0 and not d.materials[m.material].textures for m in d.meshes)
        assert d.triangle_count() <= 46 and (name[0] != "D" or d.triangle_count() <= (12 if name in ("D", "D1") else 28))
    b = M.scene("B")
    assert {b.materials[m.material].klass for m in b.meshes} == {0, 1, 2}
    assert any(b.materials[m.material].params[14] == np.float32(0.4) for m in b.meshes) and any(b.materials[m.material].textures for m in b.meshes)
    depth = {name: _tree_depth(M.scene(name)) for name in ("A1", "B", "C", "D", "D2", "D3")}
    print("tree depths", depth)
    assert 4 < depth["C"] <= 8 and all(depth[n] <= 4 for n in ("A1", "B", "D"))
    assert depth["D"] == 1 and depth["D2"] == depth["D3"] == 2   # 12 triangles are one node: walks of one step, nothing to carry; the carry cases get two levels
    c = M.scene("C")
    assert [len(m.faces) for m in c.meshes] == [50, 50] and c.materials[1].params[14] == np.float32(0.4) and c.materials[0].params[14] == 1.0

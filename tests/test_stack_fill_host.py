"""How full a traversal stack can get, without a GPU: the host builder's tree and the host's ordered walk (giCDebugBvhStackReach, an UPPER bound: it culls
nothing) for the scenes of tests/stack_fill_scenes.py -- pinned here, so that a builder change that flattens one of them fails on the CPU and not vacuously on
the GPU -- and for the telescopes the older deep-tree tests use, whose walks stay far from the last row of their stacks.  The device counter
(giCDebugTraversalStackHigh, tests/test_gpu_stack_fill.py) is the proof that a render filled a stack; these figures are host simulation."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

import stack_fill_scenes as S
from gatling_amd import capi

ROOT = Path(__file__).resolve().parent.parent


@pytest.mark.parametrize("f", S.SCENES, ids=[f.name for f in S.SCENES])
def test_scene_tree_and_reach_are_pinned(f):
    """Levels, bvhDepth and the reach of the outward bundle; the scene that is rendered has the triangles the walk was run on; the variant the host picks."""
    tris = S.telescope_tris(f.n, f.ratio)
    assert np.array_equal(S.scene_tris(S.scene(f)), tris)
    o, d = S.bundle(f)
    levels, nodes, reach = capi.bvh_stack_reach(tris, o, d)
    full = int((reach == reach.max()).sum())
    print(f"{f.name}: telescope({f.n}, {f.ratio}) {levels} levels, {nodes} nodes, reach {int(reach.max())} by {full} of {len(reach)} outward rays")
    assert (levels, int(reach.max())) == (f.levels, f.reach)
    assert reach.max() <= f.depth and f.high <= f.reach  # one entry per level below the root at most; the target lies within what the rays can hold
    assert full >= len(reach) // 50                      # not one lucky ray: a render's few thousand rays find such walks too
    lds = f.n <= 128 and nodes <= 384                    # gi_traversal.h LDS_TRIS / LDS_NODES
    assert lds == (f.group <= 3) and f.fused == (1 if lds and f.depth <= 8 else 0)
    rows = (4 if f.depth <= 4 else 8) if f.fused else 8 if f.depth <= 8 else 12 if f.depth <= 12 else 16
    assert rows == f.rows and (f.high == f.depth if f.group != 5 and f.group != 3 else True)
    assert f.group != 5 or (17 <= f.depth < 48 and f.high >= 18)
    assert f.n <= 4000
    lot = (C.c_uint32 * 4)()
    if f.fused:  # the lot begins in the row above the walks' last one
        assert capi.load_library().giCDebugPathLot(f.depth, nodes, f.n, lot) == capi.GI_C_OK
        assert (lot[0], lot[1], lot[2]) == (f.rows, f.depth, (f.rows - f.depth) * 8)


# the telescopes of test_deep_trees_parity, test_tree_deeper_than_four_levels (walk carry, lobe parking, ring carry) and scene C of the path matrix:
# (n, ratio) -> levels, rows of the variant they run, reach of rays from the camera region those tests use, reach of the outward bundle (the seeded
# draw of test_deep_trees_parity's ray bundle at 20 000 rays; an unseeded draw of the same family gave 6 where this one gives 7 for the deepest tree).
# These are figures of that BUNDLE family, an upper bound for it; the cameras and bounce rays of those tests' renders are not walked here.
OLDER = {(100, 1.1): (7, 8, 2, 5), (120, 1.2): (13, 12, 2, 8), (400, 1.03): (11, 16, 8, 10), (2000, 1.006): (12, 16, 8, 11), (400, 1.2): (39, 16, 7, 17)}


@pytest.mark.parametrize("n,ratio", list(OLDER), ids=[f"{n}-{r}" for n, r in OLDER])
def test_older_telescopes_do_not_fill_their_stacks(n, ratio):
    """Host simulation, 20 000 rays per family: from where those tests' cameras and ray bundles are, a walk holds 2 to 8 entries; even outward rays stay a row
    or more below the last one (and below the scratch spill: 17 entries of 16 + 40 would be one spilled entry, which the camera-region rays never reach)."""
    levels, rows, cam, out = OLDER[(n, ratio)]
    tris = S.telescope_tris(n, ratio, u=1.0)  # as those tests build it
    rng = np.random.default_rng(n)
    m = 20000
    o = np.stack([rng.uniform(-0.2, 3.5, m), rng.uniform(-0.6, 0.6, m), rng.uniform(0.3, 2.0, m)], 1).astype(np.float32)
    j = rng.integers(0, n, m); sj = ratio ** (-j.astype(np.float64))
    t = np.stack([3.3 * sj, 0.3 * sj * ((j % 5) - 2), 0.05 * sj * (j % 3)], 1)
    d = t - o; d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    lv, _, reach_cam = capi.bvh_stack_reach(tris, o, d)
    f = S.Fill("older", n, ratio, levels, 0, 0, "", rows, 0, 0)
    _, _, reach_out = capi.bvh_stack_reach(tris, *S.bundle(f, m=20000, u=1.0))
    print(f"telescope({n}, {ratio}): {lv} levels, {rows} rows; camera-region rays hold {int(reach_cam.max())}, outward rays {int(reach_out.max())}")
    assert lv == levels
    assert (int(reach_cam.max()), int(reach_out.max())) == (cam, out)  # (the draws are seeded: the table itself, so that a builder change shows)
    assert int(reach_cam.max()) < min(rows, levels - 1)


def test_walk_reads_the_tree_as_the_kernels_do():
    """One triangle: a root of one leaf, nothing is ever pushed.  Rays that miss the scene's box hold nothing; an empty bundle and an empty scene are fine."""
    tri = np.array([[[0, 0, 0], [1, 0, 0], [0, 1, 0]]], np.float32)
    o = np.array([[0.2, 0.2, -1], [5, 5, -1]], np.float32); d = np.array([[0, 0, 1], [0, 0, 1]], np.float32)
    levels, nodes, reach = capi.bvh_stack_reach(tri, o, d)
    assert (levels, nodes, reach.tolist()) == (1, 1, [0, 0])
    assert capi.bvh_stack_reach(tri, o[:0], d[:0])[2].size == 0
    assert capi.bvh_stack_reach(tri[:0], o, d)[2].tolist() == [0, 0]
    # a ray's reach does not depend on the rays beside it, and a reversed ray (inward) holds fewer entries than the outward one on the same line
    f = S.BY_NAME["d8"]
    tris = S.telescope_tris(f.n, f.ratio)
    o, d = S.bundle(f, m=200)
    _, _, a = capi.bvh_stack_reach(tris, o, d)
    _, _, b = capi.bvh_stack_reach(tris, o[::-1], d[::-1])
    assert np.array_equal(a, b[::-1])
    k = int(np.argmax(a))
    far = o[k] + d[k] * 10.0
    assert capi.bvh_stack_reach(tris, far[None], -d[k][None])[2][0] < a[k] == f.depth


def test_abi_and_bindings_move_together():
    text = (ROOT / "include" / "gi_c.h").read_text()
    assert re.search(r"#define\s+GI_C_API_VERSION\s+8u?\b", text)
    assert re.search(r"int\s+giCDebugTraversalStackHigh\(const GiCScene\*\s*scene,\s*uint32_t\*\s*out\s*/\*\s*4\s*\*/\);", text)
    assert re.search(r"int\s+giCDebugBvhStackReach\(const float\*\s*triVerts,\s*uint32_t\s+triCount,\s*const float\*\s*origins,\s*const float\*\s*dirs,\s*"
                     r"uint32_t\s+rayCount,\s*uint32_t\*\s*out", text)
    comment = text[:text.index("#define GI_C_API_VERSION")]
    assert "giCDebugTraversalStackHigh" in comment and "giCDebugBvhStackReach" in comment
    names = [n for n, _, _ in capi.SYMBOLS]
    lib = capi.load_library()
    for n in ("giCDebugTraversalStackHigh", "giCDebugBvhStackReach"):
        assert names.count(n) == 1 and hasattr(lib, n)
    assert "UPPER BOUND" in capi.bvh_stack_reach.__doc__

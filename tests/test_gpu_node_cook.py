"""k_path's cooked nodes on the GPU (gatling_amd/csrc/gi_node_cook.h, gi_traversal.h trav_node_test_cooked, gi_path.hip launchPath; GATLING_OPTIONS=node_cook;
tests/test_node_cook_host.py holds the cooked form itself on the CPU).  The hot variants without next-event estimation stage their nodes cooked: the word a
child adds to the hit mask comes from a table, and the child loop covers the occupied slots up to a bound of the wave.  The box test's arithmetic is untouched,
so for every (node, ray) the hit mask, R.G and the triangle group are the same words; a walk is the same sequence of visits, and images and `segments` are those
of node_cook=0.

1. giCDebugCheckNodeCook runs both node tests on (node, ray) pairs and counts the pairs whose groups differ: 0 for the named nodes (cornell's, the hand-made
   shapes) and for seeded random nodes x rays -- all eight octants, zero and denormal direction components, origins inside, on and outside the boxes, tBest
   from 1e-3 to FLT_MAX.
2. Renders at 96 x 54, spp 4, 8 bounces: cornell of class 0 and of class 1, with the leaf lift and without (the root then has an empty slot in the middle), each
   with node_cook 0, 1 and absent, and crossed once with walk_carry=0, ring_carry=0 and lobe_park=0: byte-equal with each other and with the oracle, `segments`
   equal, giCDebugSceneNodeCook reporting the variant that ran.
3. Not cooked: the mixed-class box with cutouts (the general kernel), a render with next-event estimation, a counting build -- and the 7-level telescope of 100
   triangles, by the derived LDS rule: its 14 nodes take 14 x 112 + 13 x 256 bytes cooked against 14 x 80, which with the 8-row stack, the triangles and the
   kernel's static LDS leaves 2 resident blocks per CU where the raw image leaves 3.  A telescope of 60 triangles (11 nodes, 7 levels) keeps its 3 blocks and
   runs the cooked 8-row kernel.
4. A one-triangle scene (a root with one occupied slot) and an empty scene render as before."""
import copy
import os
import re

import numpy as np
import pytest

import leaf_lift_trees as T
import node_cook_nodes as N
import path_matrix_cases as M
import stack_fill_scenes as S
from gatling_amd.meshprep import bake_vertices
from gatling_amd.scene import CameraDesc, MaterialDesc, MeshDesc, RenderSettings, SceneDesc
from gatling_amd.scenes import cornell_box
from test_gpu_path_walk_carry import _telescope

gpu = pytest.mark.gpu

W, H = 96, 54
RS = RenderSettings(spp=4, max_bounces=8, progressive_accumulation=False)
RS_NEE = RenderSettings(spp=4, max_bounces=8, progressive_accumulation=False, next_event_estimation=True)
FLT_MAX = np.float32(3.4028234663852886e38)
STATIC_LDS = 28672  # k_path: one WaveTri and one ring of prepared camera rays per wave
_KERNELS_H = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gatling_amd", "csrc", "gi_kernels.h")).read()
DEFAULT_ON = int(re.search(r"constexpr long NODE_COOK_DEFAULT = (\d+);", _KERNELS_H).group(1)) != 0  # what a render without the key does


def wanted(options):
    """Does this GATLING_OPTIONS string ask for cooked nodes?"""
    m = re.search(r"node_cook=(\d+)", options)
    return int(m.group(1)) != 0 if m else DEFAULT_ON


def blocks_per_cu(stack, nodes, tris, cooked):
    """gi_path.hip launchPath / gi_trace.hip blocksPerCuByLds: what 160 KiB hold of a block's dynamic + static LDS + 256 bytes of allocation slack."""
    image = nodes * 112 + max(nodes - 1, 0) * 256 if cooked else nodes * 80
    return (160 * 1024) // (stack * 256 * 8 + image + tris * 48 + STATIC_LDS + 256)


def rays_for(nodes, count, seed):
    """`count` rays, ray i aimed at node i % len(nodes): origins inside the node's frame, exactly on a child's plane, and outside it; directions over all eight
    octants with zero, negative-zero and denormal components mixed in; tMin 0 or 1e-3; tBest from 1e-3 to FLT_MAX."""
    rng = np.random.default_rng(seed)
    n = len(nodes)
    idx = np.arange(count) % n
    p = nodes["p"][idx].astype(np.float64)
    scale = np.ldexp(1.0, nodes["e"][idx].astype(np.int64) - 127)
    kind = rng.integers(0, 3, count)
    u = np.where(kind[:, None] == 0, rng.uniform(0.0, 255.0, (count, 3)), rng.uniform(-300.0, 555.0, (count, 3)))
    slot = rng.integers(0, 8, count)
    on = np.where(rng.integers(0, 2, (count, 3)) == 0, nodes["qlo"][idx, :, slot], nodes["qhi"][idx, :, slot]).astype(np.float64)
    u = np.where(kind[:, None] == 1, on, u)
    o = (p.astype(np.float32) + (u.astype(np.float32) * scale.astype(np.float32))).astype(np.float32)  # (a plane exactly as the kernel dequantises it)
    d = rng.normal(0.0, 1.0, (count, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    d = np.abs(d).astype(np.float32)
    d *= np.where(np.arange(count)[:, None] >> np.arange(3)[None] & 1, np.float32(1.0), np.float32(-1.0))  # ray i: octant i & 7 ...
    special = rng.integers(0, 16, (count, 3))
    for code, value in ((0, np.float32(0.0)), (1, np.float32(-0.0)), (2, np.float32(1e-40)), (3, np.float32(-1e-40))):
        d = np.where(special == code, value, d).astype(np.float32)                                         # ... before the zeros and denormals
    t_min = np.where(rng.integers(0, 2, count) == 0, np.float32(0.0), np.float32(1e-3)).astype(np.float32)
    t_best = np.exp(rng.uniform(np.log(1e-3), np.log(1e4), count)).astype(np.float32)
    t_best[rng.integers(0, 8, count) == 0] = FLT_MAX
    t_best[::97] = np.float32(1e-3)
    return np.concatenate([o, d, t_min[:, None], t_best[:, None]], 1).astype(np.float32)


@pytest.fixture(scope="module")
def named_nodes(gi):
    tris = S.scene_tris(cornell_box())
    built, lifted = gi.leaf_lift(tris, 0), gi.leaf_lift(tris, 1)
    return np.concatenate([T.decode(built["nodes"]), T.decode(lifted["nodes"]), N.hand_made()])


@gpu
def test_check_kernel_named_nodes(gi, named_nodes):
    rays = rays_for(named_nodes, 1 << 15, 3)
    octants = {int(v) for v in ((rays[:, 3] >= 0) + 2 * (rays[:, 4] >= 0) + 4 * (rays[:, 5] >= 0))}
    assert octants == set(range(8)) and (rays[:, 3:6] == 0).any() and (np.abs(rays[:, 3:6]) == np.float32(1e-40)).any() and (rays[:, 7] == FLT_MAX).any()
    bad = gi.check_node_cook(named_nodes.tobytes(), rays)
    print(f"{len(named_nodes)} named nodes x {len(rays)} rays: {bad} pairs differ")
    assert bad == 0


@gpu
def test_check_kernel_random_nodes(gi):
    total = 0
    for batch in range(8):  # 8 x 64 nodes, 8 x 16 384 pairs: about 1.3e5
        nodes = N.random_nodes(64, 100 + batch)
        rays = rays_for(nodes, 1 << 14, 200 + batch)
        bad = gi.check_node_cook(nodes.tobytes(), rays)
        assert bad == 0, (batch, bad)
        total += len(rays)
    # a wave of one node, and fewer pairs than a wave
    one = N.hand_made()[3:4]
    assert gi.check_node_cook(one.tobytes(), rays_for(one, 4096, 5)) == 0 and gi.check_node_cook(one.tobytes(), rays_for(one, 7, 6)) == 0
    print(f"{total} random (node, ray) pairs: 0 differ")
    with pytest.raises(gi.GiError):
        gi.check_node_cook(N.random_nodes(65, 1).tobytes(), rays_for(one, 8, 7))


def assert_image_parity(img, ref, what):
    assert img.shape == ref.shape and np.isfinite(img).all(), what
    bad = int((img.view(np.uint32) != ref.view(np.uint32)).any(axis=-1).sum())
    assert bad == 0, f"{what}: {bad} pixels differ bitwise"


_oracle = {}


def _reference(orc, name, desc, rs, w=W, h=H):
    """The oracle's frame of a scene, computed once for all the tests that need it."""
    if name not in _oracle:
        img, cnt = orc.render(desc, rs, w, h, threads=4)
        img.setflags(write=False)
        _oracle[name] = (img, cnt)
    return _oracle[name]


def _render(gi, monkeypatch, options, desc, rs, count=False, w=W, h=H):
    monkeypatch.setenv("GATLING_OPTIONS", options)
    sc = gi.Scene(copy.deepcopy(desc))
    try:
        if count:
            sc.set_option(gi.OPTION_COUNT_TRAVERSAL, 1)
        img = sc.render(rs, w, h).copy()
        st, cooked = sc.stats(), sc.node_cook()
    finally:
        sc.close()
    return img, st, cooked


KEYS = ["node_cook=0", "node_cook=1", "", "leaf_lift=0,node_cook=0", "leaf_lift=0,node_cook=1", "leaf_lift=0",
        "node_cook=1,walk_carry=0", "node_cook=1,ring_carry=0", "node_cook=1,lobe_park=0", "node_cook=1,ups_plain=0"]


@gpu
@pytest.mark.parametrize("name", ["A1", "A2"], ids=["class0", "class1"])
def test_fused_image_is_the_same_cooked_and_raw(gi, orc, monkeypatch, name):
    desc = M.scene(name)
    ref, cnt = _reference(orc, name, desc, RS)
    first = None
    for k in KEYS:
        img, st, cooked = _render(gi, monkeypatch, k, desc, RS)
        print(f"{name} [{k or 'default'}]: cooked {cooked}, segments {st['segments']} / {cnt['segments']}")
        assert st["fusedPath"] == 1 and (st["nodeCount"], st["triangleCount"]) == (4, 46), (k, st)
        assert cooked == wanted(k), (name, k)  # cornell: 4 x 112 + 3 x 256 bytes against 4 x 80 keep the four blocks per CU
        assert (st["segments"], st["samples"]) == (cnt["segments"], cnt["samples"]), (name, k, st, cnt)
        assert_image_parity(img, ref, (name, k))
        first = img if first is None else first
        assert img.tobytes() == first.tobytes(), (name, k)
    assert blocks_per_cu(4, 4, 46, True) == blocks_per_cu(4, 4, 46, False) == 4


@gpu
def test_kernels_without_a_cooked_variant(gi, orc, monkeypatch):
    for what, key, desc, rs, count in (("mixed classes, cutouts", "B", M.scene("B"), RS, False),
                                       ("next-event estimation", "A2-nee", M.scene("A2", nee=True), RS_NEE, False),
                                       ("counting build", "A2", M.scene("A2"), RS, True)):
        ref, cnt = _reference(orc, key, desc, rs)
        img, st, cooked = _render(gi, monkeypatch, "node_cook=1", desc, rs, count=count)
        assert st["fusedPath"] == 1 and not cooked and st["segments"] == cnt["segments"], (what, st, cooked)
        assert_image_parity(img, ref, what)


@gpu
def test_deep_trees_follow_the_lds_rule(gi, orc, monkeypatch):
    rs = RenderSettings(spp=4, max_bounces=4, progressive_accumulation=False)
    # 100 triangles: 14 nodes, 7 levels -- cooked, the block's LDS would leave 2 blocks per CU instead of 3: the raw kernel runs
    # 60 triangles at ratio 1.3: 11 nodes, 7 levels -- 3 blocks either way: the cooked 8-row kernel runs
    for n, ratio, nodes, want in ((100, 1.1, 14, False), (60, 1.3, 11, True)):
        desc = _telescope(n, ratio)
        ref, cnt = _reference(orc, ("telescope", n), desc, rs, 64, 36)
        got = {k: _render(gi, monkeypatch, k, desc, rs, w=64, h=36) for k in ("node_cook=0", "node_cook=1", "")}
        st = got["node_cook=1"][1]
        assert st["fusedPath"] == 1 and (st["nodeCount"], st["triangleCount"]) == (nodes, n), st
        rule = blocks_per_cu(8, nodes, n, True) >= blocks_per_cu(8, nodes, n, False)
        print(f"telescope({n}, {ratio}): {nodes} nodes, blocks per CU raw {blocks_per_cu(8, nodes, n, False)} / cooked {blocks_per_cu(8, nodes, n, True)}: cooked {got['node_cook=1'][2]}")
        assert rule == want and got["node_cook=1"][2] == want and got[""][2] == (want and DEFAULT_ON) and not got["node_cook=0"][2]
        for k, (img, s, _) in got.items():
            assert s["segments"] == cnt["segments"], (n, k)
            assert_image_parity(img, ref, ("telescope", n, k))


@gpu
def test_one_triangle_and_empty_scene(gi, orc, monkeypatch):
    cam = CameraDesc(position=(0, 0, 5))
    p = np.array([[-1, -1, 0], [1, -1, 0], [0, 1, 0]], np.float32)
    nrm = np.repeat(np.array([[0, 0, 1]], np.float32), 3, axis=0)
    one = SceneDesc(meshes=[MeshDesc("tri", bake_vertices(p, nrm), np.arange(3, dtype=np.uint32).reshape(-1, 3), 0, double_sided=True)],
                    materials=[MaterialDesc.usd_preview_surface(diffuseColor=(0.8, 0.3, 0.2))], camera=cam)
    empty = SceneDesc(materials=[MaterialDesc.usd_preview_surface()], camera=cam)
    rs = RenderSettings(spp=4, max_bounces=4, progressive_accumulation=False, clear_color=(0.5, 0.25, 1.0, 1.0))
    for what, desc, fused in (("one triangle", one, 1), ("empty", empty, 0)):
        ref, cnt = _reference(orc, what, desc, rs, 32, 18)
        for k in ("node_cook=0", "node_cook=1", ""):
            img, st, cooked = _render(gi, monkeypatch, k, desc, rs, w=32, h=18)
            assert (fused == 0 or st["fusedPath"] == 1) and cooked == (fused == 1 and wanted(k)), (what, k, st, cooked)
            assert st["segments"] == cnt["segments"], (what, k)
            assert_image_parity(img, ref, (what, k))

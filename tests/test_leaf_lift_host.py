"""The leaf lift of small flat trees (gatling_amd/csrc/leaf_lift.cpp liftLeafSlots; gi_build.cpp buildScene; GI_C_SCENE_OPTION_LEAF_LIFT = 25,
GATLING_OPTIONS=leaf_lift) without a GPU, through giCDebugLeafLift: the host builder's tree -- or a hand-made one -- goes through the pass, and the nodes and the
leaf order come back.

The pass moves a leaf slot of an internal child into a free slot of the child's parent while the builder's cost model, evaluated over the dequantised slot boxes,
strictly decreases.  Cornell (46 triangles): the binned split left the ceiling's two triangles in the light's subtree, whose box in the root therefore spans
the whole ceiling; the root has one free slot.  The lifted tree must reference every triangle once, keep every box conservative, keep node count, levels and
imask, cost strictly less, answer every ray as brute force does and visit no more nodes doing so; a second run must change nothing; leaf_lift=0 must hand out
the builder's bytes.  Trees the pass must leave alone: no free slot in the root, a child with a single slot, a node of 24 references, one node, no triangle,
three levels.  (With a free slot and an internal child a node holds at most 6 leaf slots, 18 references: a lifted slot makes 21, so the 24-reference limit
cannot bind in a well-formed tree -- the case here is the full node, which has neither.)

The same under AddressSanitizer + UBSan as a program of its own (tests/cpp/leaf_lift_sanitize.cpp)."""
import os
import re
import subprocess

import numpy as np
import pytest

import leaf_lift_trees as T
import stack_fill_scenes as S
from gatling_amd import capi
from gatling_amd.scenes import cornell_box

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def cornell():
    tris = S.scene_tris(cornell_box())
    assert tris.shape == (46, 3, 3)
    old_env = os.environ.pop("GATLING_OPTIONS", None)
    try:
        built, lifted = capi.leaf_lift(tris, 0), capi.leaf_lift(tris, 1)
    finally:
        if old_env is not None:
            os.environ["GATLING_OPTIONS"] = old_env
    return tris, built, lifted


def _leaf_slots(nodes):
    for i, nd in enumerate(nodes):
        for s in range(8):
            if T.is_leaf(nd, s):
                yield i, s, T.leaf_range(nd, s)


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# cornell
# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
def test_cornell_every_triangle_is_referenced_once(cornell):
    tris, built, lifted = cornell
    for r in (built, lifted):
        nodes = T.decode(r["nodes"])
        positions = [p for _, _, rng in _leaf_slots(nodes) for p in rng]
        assert sorted(positions) == list(range(46)) and r["active"] == 46 and r["violations"] == 0
        assert sorted(r["order"].tolist()) == list(range(46))
        # the builder's layout: triangles in node order, slot order within a node
        assert positions == list(range(46))


def test_cornell_boxes_stay_conservative(cornell):
    """Leaf slots hold their triangles' padded boxes.  Internal slots: the builder's contract is that a child's box holds the padded boxes of everything BELOW it
    (bvh8.cpp) -- checked for every internal slot.  The stronger property, that it also holds the child's own dequantised slot boxes, the builder does not give:
    a child rounds its slots outward on its own finer grid, past the plane its parent rounded to (cornell's root slot 2 ends at z = 0.40608537, the child's
    slot 1 at 0.40624774, both around the triangles' 0.40600...).  The pass computes a child's box from the child's remaining dequantised slots, so the slots it
    WROTE have the stronger property, and that is asserted for them; the slots it did not write are the builder's bytes, which is asserted too."""
    tris, built, lifted = cornell
    nodes, order, before = T.decode(lifted["nodes"]), lifted["order"], T.decode(built["nodes"])
    for i, s, rng in _leaf_slots(nodes):
        lo, hi = T.slot_box(nodes[i], s)
        for p in rng:  # a leaf slot's dequantised box holds its triangles' padded boxes
            tlo, thi = T.padded_box(tris[order[p]])
            assert (lo <= tlo).all() and (hi >= thi).all(), (i, s, p)
    rewritten = 0
    for i in range(len(nodes)):
        for s, c in T.children(nodes, i).items():
            lo, hi = T.slot_box(nodes[i], s)
            for _, _, rng in _leaf_slots(nodes[c:c + 1]):  # everything below (two levels: the child's leaves)
                for p in rng:
                    tlo, thi = T.padded_box(tris[order[p]])
                    assert (lo <= tlo).all() and (hi >= thi).all(), (i, s, c, p)
            if nodes[c]["meta"].tobytes() == before[c]["meta"].tobytes():  # the child lost nothing: the parent's slot is the builder's
                assert nodes[i]["qlo"][:, s].tobytes() == before[i]["qlo"][:, s].tobytes() and nodes[i]["qhi"][:, s].tobytes() == before[i]["qhi"][:, s].tobytes()
                continue
            rewritten += 1
            for cs in range(8):  # a slot the pass wrote holds its child's slots
                if nodes[c]["meta"][cs] != 0:
                    clo, chi = T.slot_box(nodes[c], cs)
                    assert (lo <= clo).all() and (hi >= chi).all(), (i, s, c, cs, lo, hi, clo, chi)
    assert rewritten == lifted["lifted"] >= 1


def test_cornell_keeps_topology_and_gets_cheaper(cornell):
    _, built, lifted = cornell
    a, b = T.decode(built["nodes"]), T.decode(lifted["nodes"])
    assert len(a) == len(b) == 4 and built["depth"] == lifted["depth"] == 2
    assert T.levels(a).tolist() == T.levels(b).tolist()
    for f in ("imask", "childBase", "p", "e"):
        assert a[f].tobytes() == b[f].tobytes(), f
    assert built["lifted"] == 0 and lifted["lifted"] >= 1
    ca, cb = T.model_cost(a), T.model_cost(b)
    print(f"cornell: {lifted['lifted']} leaf slot(s) lifted, model cost {ca:.4f} -> {cb:.4f} (library: {lifted['cost_before']:.4f} -> {lifted['cost_after']:.4f})")
    assert cb < ca and lifted["cost_after"] < lifted["cost_before"]
    assert abs(ca - lifted["cost_before"]) < 1e-3 * ca and abs(cb - lifted["cost_after"]) < 1e-3 * cb  # (fp32 areas in the library, float64 here)
    # what moved: the root gained a leaf slot, one child lost one, nothing else changed
    occupied = lambda n: [int((nd["meta"] != 0).sum()) for nd in n]
    assert occupied(b)[0] == occupied(a)[0] + lifted["lifted"] and sum(occupied(a)) == sum(occupied(b))


def test_cornell_second_run_changes_nothing(cornell):
    tris, _, lifted = cornell
    again = capi.leaf_lift(tris[lifted["order"]], 1, tree_nodes=lifted["nodes"].tobytes(), tree_depth=lifted["depth"])
    assert again["lifted"] == 0 and again["violations"] == 0
    assert again["nodes"].tobytes() == lifted["nodes"].tobytes() and again["order"].tolist() == list(range(46))
    # and from the builder's tree handed in as a tree: the same result as behind the builder
    built = cornell[1]
    via = capi.leaf_lift(tris[built["order"]], 1, tree_nodes=built["nodes"].tobytes(), tree_depth=built["depth"])
    assert via["nodes"].tobytes() == lifted["nodes"].tobytes() and built["order"][via["order"]].tolist() == lifted["order"].tolist()


def test_cornell_leaf_lift_0_returns_the_builders_bytes(cornell, monkeypatch):
    tris, built, lifted = cornell
    monkeypatch.setenv("GATLING_OPTIONS", "leaf_lift=0")
    off = capi.leaf_lift(tris, -1)
    assert off["lifted"] == 0 and off["nodes"].tobytes() == built["nodes"].tobytes() and off["order"].tolist() == built["order"].tolist()
    monkeypatch.setenv("GATLING_OPTIONS", "leaf_lift=1")
    on = capi.leaf_lift(tris, -1)
    monkeypatch.delenv("GATLING_OPTIONS")
    default = capi.leaf_lift(tris, -1)
    for r in (on, default):  # the default is on
        assert r["lifted"] == lifted["lifted"] and r["nodes"].tobytes() == lifted["nodes"].tobytes() and r["order"].tolist() == lifted["order"].tolist()


def test_cornell_walk_equals_brute_force_and_visits_no_more_nodes(cornell):
    tris, built, lifted = cornell
    rng = np.random.default_rng(28)
    n = 4000
    o = rng.uniform(-0.95, 0.95, (n, 3))
    d = rng.normal(size=(n, 3)); d /= np.linalg.norm(d, axis=1, keepdims=True)
    o[: n // 4] = (0.0, -7.0, 0.0)  # a quarter from the camera's place, into the box and past it
    d[: n // 4] = rng.uniform(-0.3, 0.3, (n // 4, 3)) + (0.0, 1.0, 0.0)
    ref_t, ref_id = T.brute_force(tris, np.arange(46), o, d)
    assert np.isfinite(ref_t).sum() > n // 2
    visited = {}
    for name, r in (("built", built), ("lifted", lifted)):
        t, hit, visited[name] = T.walk(T.decode(r["nodes"]), tris[r["order"]], r["order"].astype(np.int64), o, d)
        assert np.array_equal(hit, ref_id) and np.array_equal(t, ref_t), name
    print(f"cornell, {n} rays: nodes visited {visited['built']} -> {visited['lifted']} ({visited['built'] / n:.3f} -> {visited['lifted'] / n:.3f} per ray)")
    assert visited["lifted"] <= visited["built"]


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# trees the pass must leave alone (and, beside each, the tree that differs in the one thing and IS changed)
# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
def _tri(x, y, z, size=0.1):
    return np.array([(x, y, z), (x + size, y, z), (x, y + size, z + size)], np.float32)


SMALL_A, SMALL_B, BIG, OTHER = _tri(0, 0, 0), _tri(0.2, 0.1, 0), _tri(0, 0, 0, 10.0), _tri(20, 0, 0, 1.0)


def _child():
    """Two small leaves and one that stretches the node's box over 10 units: lifting the big one pays whenever the parent has room."""
    return {0: [SMALL_A], 1: [SMALL_B], 2: [BIG]}


def _run(spec):
    nodes, tris, depth = T.make_tree(spec)
    r = capi.leaf_lift(tris, 1, tree_nodes=nodes, tree_depth=depth)
    assert r["violations"] == 0 and r["depth"] == depth
    return r, nodes, tris


def _unchanged(r, nodes, tris):
    return r["lifted"] == 0 and r["nodes"].tobytes() == nodes and r["order"].tolist() == list(range(len(tris))) and r["cost_after"] == r["cost_before"]


def _root(free):
    """A root of the child in slot 0 and one-triangle leaves elsewhere, `free` slots left empty (the last ones)."""
    spec = {0: _child()}
    spec.update({s: [_tri(20 + 2 * s, 0, 0, 1.0)] for s in range(1, 8 - free)})
    return spec


def test_control_a_root_with_room_takes_the_stretching_leaf():
    r, nodes, tris = _run(_root(1))
    assert r["lifted"] == 1 and r["cost_after"] < r["cost_before"] and r["nodes"].tobytes() != nodes
    out = T.decode(r["nodes"])
    assert int((out[0]["meta"] != 0).sum()) == 8 and int((out[1]["meta"] != 0).sum()) == 2 and out[0]["imask"] == 1
    assert sorted(r["order"].tolist()) == list(range(len(tris)))
    # the big triangle is now the root's; the child's box in the root shrank to the small ones
    root_tris = [p for s in range(8) if T.is_leaf(out[0], s) for p in T.leaf_range(out[0], s)]
    assert any(np.array_equal(tris[r["order"][p]], BIG) for p in root_tris)
    lo, hi = T.slot_box(out[0], 0)
    assert (hi - lo).max() < 1.0
    # with two free slots the second-best move follows (a small leaf: the child's box shrinks once more), and the child keeps its last slot
    r2, _, _ = _run(_root(2))
    assert r2["lifted"] == 2 and r2["cost_after"] < r2["cost_before"] and int((T.decode(r2["nodes"])[1]["meta"] != 0).sum()) == 1


def test_a_root_without_a_free_slot_is_left_alone():
    assert _unchanged(*_run(_root(0)))


def test_a_child_with_a_single_slot_keeps_it():
    assert _unchanged(*_run({0: {2: [BIG]}, 1: [OTHER]}))
    # two slots: one may go (the big one), the last one stays
    r, _, _ = _run({0: {0: [SMALL_A], 2: [BIG]}, 1: [OTHER]})
    assert r["lifted"] == 1 and int((T.decode(r["nodes"])[1]["meta"] != 0).sum()) == 1


def test_a_node_of_24_references_is_left_alone():
    full = {s: [_tri(3 * s, 0, 0), _tri(3 * s, 1, 0), _tri(3 * s, 2, 0)] for s in range(8)}
    assert _unchanged(*_run(full))
    # and the fullest node that can still take a slot: 6 x 3 references, a child, a free slot -- the lifted leaf's 3 make 21
    spec = {s: [_tri(30 + 3 * s, 0, 0), _tri(30 + 3 * s, 1, 0), _tri(30 + 3 * s, 2, 0)] for s in range(1, 7)}
    spec[0] = {0: [SMALL_A], 1: [SMALL_B], 2: [BIG, _tri(0, 0, 1, 10.0), _tri(0, 0, 2, 10.0)]}
    r, _, _ = _run(spec)
    root = T.decode(r["nodes"])[0]
    refs = sum(len(T.leaf_range(root, s)) for s in range(8) if T.is_leaf(root, s))
    assert r["lifted"] == 1 and refs == 21 and max(int(root["meta"][s]) & 31 for s in range(8) if T.is_leaf(root, s)) == 18


def test_a_one_node_tree_and_an_empty_scene_are_left_alone():
    five = np.stack([_tri(k, 0, 0) for k in range(5)])
    a, b = capi.leaf_lift(five, 0), capi.leaf_lift(five, 1)
    assert (a["depth"], len(a["nodes"]), b["lifted"]) == (1, 1, 0) and a["nodes"].tobytes() == b["nodes"].tobytes() and a["order"].tolist() == b["order"].tolist()
    a, b = capi.leaf_lift(five[:0], 0), capi.leaf_lift(five[:0], 1)
    assert (len(a["nodes"]), b["lifted"], b["active"], b["violations"]) == (1, 0, 0, 0) and a["nodes"].tobytes() == b["nodes"].tobytes()


def test_a_tree_of_three_levels_is_left_alone():
    deep = {0: {0: {0: [SMALL_A], 1: [_tri(0.05, 0, 0)]}, 1: [SMALL_B], 2: [BIG]}, 1: [OTHER]}
    r, nodes, tris = _run(deep)
    assert r["depth"] == 3 and _unchanged(r, nodes, tris)


def test_random_small_scenes_keep_the_contract():
    """The builder's trees over random clusters and over rooms of cornell's family (five walls, a flat box under the ceiling, one or two boxes on the floor):
    whatever the pass does, the tree stays valid, never costs more, and a second run changes nothing."""
    rng = np.random.default_rng(2028)
    acted = 0

    def quad(a, b, c, d):
        return [(a, b, c), (a, c, d)]

    def box(lo, hi):
        c = [[(hi if (i >> a) & 1 else lo)[a] for a in range(3)] for i in range(8)]
        return [t for f in ((0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)) for t in quad(*(c[k] for k in f))]

    def room():
        r = 1.0 + rng.uniform(-0.02, 0.02)
        c = [[(r if (i >> a) & 1 else -r) for a in range(3)] for i in range(8)]
        t = [x for f in ((0, 1, 3, 2), (4, 5, 7, 6), (2, 3, 7, 6), (0, 2, 6, 4), (1, 3, 7, 5)) for x in quad(*(c[k] for k in f))]
        hx, hy, cx, cy = rng.uniform(0.15, 0.7), rng.uniform(0.15, 0.7), rng.uniform(-0.2, 0.2), rng.uniform(-0.2, 0.2)
        t += box((cx - hx, cy - hy, r - 0.02), (cx + hx, cy + hy, r))
        for _ in range(int(rng.integers(1, 3))):
            bx, by, bh = rng.uniform(-0.5, 0.5), rng.uniform(-0.5, 0.5), rng.uniform(0.15, 0.3)
            t += box((bx - bh, by - bh, -r), (bx + bh, by + bh, -r + rng.uniform(0.3, 1.4)))
        return np.asarray(t, np.float32)

    def clusters():
        n = int(rng.integers(9, 60))
        centres = rng.uniform(-1, 1, (int(rng.integers(2, 6)), 3))
        c = centres[rng.integers(0, len(centres), n)] + rng.normal(scale=0.05, size=(n, 3))
        return (c[:, None, :] + rng.normal(scale=rng.choice([0.03, 0.6], size=(n, 1, 1)), size=(n, 3, 3))).astype(np.float32)

    for case in range(40):
        tris = room() if case % 2 else clusters()
        n = len(tris)
        a, b = capi.leaf_lift(tris, 0), capi.leaf_lift(tris, 1)
        assert a["violations"] == 0 and b["violations"] == 0 and sorted(b["order"].tolist()) == list(range(n))
        if a["depth"] > 2:
            assert b["lifted"] == 0
        if b["lifted"] == 0:
            assert a["nodes"].tobytes() == b["nodes"].tobytes() and a["order"].tolist() == b["order"].tolist()
            continue
        acted += 1
        assert b["cost_after"] < b["cost_before"] == a["cost_before"]
        again = capi.leaf_lift(tris[b["order"]], 1, tree_nodes=b["nodes"].tobytes(), tree_depth=b["depth"])
        assert again["lifted"] == 0 and again["nodes"].tobytes() == b["nodes"].tobytes()
    print(f"random small scenes: the pass acted on {acted} of 40")
    assert acted > 0


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# declarations
# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
def test_header_and_harness_declare_the_option_and_the_hooks():
    text = open(os.path.join(ROOT, "include", "gi_c.h")).read()
    assert re.search(r"#define\s+GI_C_SCENE_OPTION_LEAF_LIFT\s+25\b", text)
    assert re.search(r"int\s+giCDebugSceneLeafLift\(const GiCScene\*\s*scene,\s*uint32_t\*\s*out\s*/\*\s*2\s*\*/\);", text)
    assert re.search(r"int\s+giCDebugLeafLift\(const float\*\s*triVerts", text)
    assert re.search(r"#define\s+GI_C_API_VERSION\s+8u?\b", text)
    opts = open(os.path.join(ROOT, "gatling_amd", "csrc", "gi_options.h")).read()
    assert re.search(r"^//\s+leaf_lift\s+1\s+scene build: ", opts, re.M)
    lib = capi.load_library()
    assert lib.giCGetApiVersion() == 8 and hasattr(lib, "giCDebugSceneLeafLift") and hasattr(lib, "giCDebugLeafLift")
    assert capi.OPTION_LEAF_LIFT == 25 and callable(capi.Scene.leaf_lift) and callable(capi.leaf_lift)


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# the pass and the builder under AddressSanitizer + UBSan, as a program of its own (tests/cpp/leaf_lift_sanitize.cpp)
# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
def test_pass_runs_clean_under_the_sanitizers(tmp_path):
    # (the sanitizer runtimes are linked statically: the program stands alone whatever else the process environment loads)
    exe = str(tmp_path / "leaf_lift_sanitize")
    csrc = os.path.join(ROOT, "gatling_amd", "csrc")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-pthread", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
           "-I", csrc, "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "leaf_lift_sanitize.cpp"), os.path.join(csrc, "bvh8.cpp"),
           os.path.join(csrc, "leaf_lift.cpp"), "-o", exe]
    probe = subprocess.run(["g++", "-fsanitize=address,undefined", "-static-libasan", "-static-libubsan", "-x", "c++", "-", "-o", str(tmp_path / "probe")],
                           input="int main(){return 0;}", text=True, capture_output=True)
    if probe.returncode != 0:
        pytest.skip("the toolchain has no sanitizer runtimes")
    built = subprocess.run(cmd, capture_output=True, text=True)
    assert built.returncode == 0, built.stderr[-4000:]
    env = dict(os.environ); env["GATLING_BUILD_THREADS"] = "4"
    tris = S.scene_tris(cornell_box()).astype("<f4")
    (tmp_path / "cornell.f32").write_bytes(tris.tobytes())
    out = subprocess.run([exe, str(tmp_path / "cornell.f32")], capture_output=True, text=True, timeout=300, env=env)
    assert out.returncode == 0 and "leaf lift sanitize ok" in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]
    assert re.search(r"cornell: 46 triangles, [1-9]\d* leaf slot\(s\) lifted", out.stdout), out.stdout[-2000:]

"""The cooked form of a BVH8 node (gatling_amd/csrc/gi_node_cook.h; k_path's COOK variants stage it in LDS: gi_traversal.h stage_scene_cooked) without a GPU,
through giCDebugNodeCook, which runs the function the kernel stages with.  A cooked node keeps Node8's header words and plane bytes, enumerates the occupied
slots first, and carries per ray octant the word each child adds to the hit mask -- what trav_node_test decodes from the meta bytes on every visit:
  a leaf child      (meta >> 5) << (meta & 31)
  an internal child 1 << (24 + (slot ^ (octinv & 7)))
  an empty child    0
Held here for cornell's four nodes with and without the leaf lift and for hand-made nodes with 0, 1, 3, 6 and 8 occupied slots, empty slots at the front, in
the middle and at the end, internal children in high slots and leaves of 1, 2 and 3 triangles: the permutation is a bijection of the occupied slots, plane
bytes travel with their child, every table entry is the formula's for each of the eight octants, the count is right and the header words are unchanged.

The same function under AddressSanitizer + UBSan as a program of its own (tests/cpp/node_cook_sanitize.cpp)."""
import os
import re
import subprocess

import numpy as np
import pytest

import leaf_lift_trees as T
import node_cook_nodes as N
import stack_fill_scenes as S
from gatling_amd import capi
from gatling_amd.scenes import cornell_box

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def cornell():
    tris = S.scene_tris(cornell_box())
    old_env = os.environ.pop("GATLING_OPTIONS", None)
    try:
        built, lifted = capi.leaf_lift(tris, 0), capi.leaf_lift(tris, 1)
    finally:
        if old_env is not None:
            os.environ["GATLING_OPTIONS"] = old_env
    return T.decode(built["nodes"]), T.decode(lifted["nodes"])


@pytest.mark.parametrize("which", [0, 1], ids=["builder", "lifted"])
def test_cornell_nodes(cornell, which):
    nodes = cornell[which]
    assert len(nodes) == 4
    cooked = capi.node_cook(nodes.tobytes())
    assert cooked["records"].shape == (4, 28) and cooked["oct"].shape == (3, 8, 8) and cooked["stride"] == 112
    perms = N.check_image(nodes, cooked)
    occupied = [sum(1 for m in nd["meta"] if m) for nd in nodes]
    print(f"cornell ({'lifted' if which else 'builder'}): occupied slots {occupied}, permutations {perms}")
    # the root alone has internal children: one block of the octant area is taken, the other two stay zero
    assert [int(r[6]) & 0xFFFF for r in cooked["records"]] == [0xE0, 0, 0, 0] and not cooked["oct"][1:].any()
    # the builder's root has its empty slot in the middle (slot 3); the lift fills it
    assert occupied[0] == (8 if which else 7) and (which == 1 or perms[0] == [0, 1, 2, 4, 5, 6, 7])
    # an image of 4 x 112 + 3 x 256 bytes against 4 x 80
    assert cooked["records"].nbytes + cooked["oct"].nbytes == 1216


def test_hand_made_nodes():
    nodes = N.hand_made()
    cooked = capi.node_cook(nodes.tobytes(), oct_blocks=len(nodes))  # (no tree: every node may take a block)
    perms = N.check_image(nodes, cooked)
    counts = [int(r[6]) >> 16 for r in cooked["records"]]
    print("occupied, rounded up to 2:", counts, "permutations:", perms)
    assert counts == [0, 2, 4, 6, 6, 8, 8, 4, 4]
    assert perms[1] == [5] and perms[2] == [0, 3, 7] and perms[3] == [2, 3, 4, 5, 6, 7] and perms[7] == [1, 6, 7]
    # a node without internal children has one table whatever the octant; with one, eight that differ in the internal children's bits alone
    for i, nd in enumerate(nodes):
        if not nd["imask"]:
            continue
        block = sum(1 for other in nodes[:i] if other["imask"])
        t = cooked["oct"][block]
        assert (t & 0x00FFFFFF == t[0] & 0x00FFFFFF).all() and len({t[o].tobytes() for o in range(8)}) == 8


def test_random_nodes_and_the_octant_area_bound():
    nodes = N.random_nodes(300, 11)
    cooked = capi.node_cook(nodes.tobytes(), oct_blocks=len(nodes))
    N.check_image(nodes, cooked)
    # a tree of n nodes has at most n - 1 with an internal child; an array that claims more is no tree: the nodes beyond the area are cooked without their
    # octant tables, inside the image
    three = N.hand_made()[[6, 6, 6]]
    cooked = capi.node_cook(three.tobytes())
    assert cooked["oct"].shape == (2, 8, 8) and [int(r[6]) & 0xFFFF for r in cooked["records"]] == [0xE0, 0xE0, 0]
    assert int(cooked["records"][2][7]) == 80
    with pytest.raises(capi.GiError):
        capi.node_cook(b"")


def test_api_text_and_binding():
    text = open(os.path.join(ROOT, "include", "gi_c.h")).read()
    assert re.search(r"int\s+giCDebugSceneNodeCook\(const GiCScene\*\s*scene,\s*uint32_t\*\s*out\s*/\*\s*1\s*\*/\);", text)
    assert re.search(r"int\s+giCDebugNodeCook\(const void\*\s*nodes,", text) and re.search(r"int64_t\s+giCDebugCheckNodeCook\(const void\*\s*nodes,", text)
    opts = open(os.path.join(ROOT, "gatling_amd", "csrc", "gi_options.h")).read()
    assert re.search(r"//\s+node_cook\s+1\s", opts)
    lib = capi.load_library()
    assert all(hasattr(lib, n) for n in ("giCDebugSceneNodeCook", "giCDebugNodeCook", "giCDebugCheckNodeCook")) and callable(capi.Scene.node_cook)


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# cook_node under AddressSanitizer + UBSan, as a program of its own (tests/cpp/node_cook_sanitize.cpp)
# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
def test_cook_runs_clean_under_the_sanitizers(tmp_path, cornell):
    # (the sanitizer runtimes are linked statically: the program stands alone whatever else the process environment loads)
    exe = str(tmp_path / "node_cook_sanitize")
    csrc = os.path.join(ROOT, "gatling_amd", "csrc")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
           "-I", csrc, "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "node_cook_sanitize.cpp"), "-o", exe]
    probe = subprocess.run(["g++", "-fsanitize=address,undefined", "-static-libasan", "-static-libubsan", "-x", "c++", "-", "-o", str(tmp_path / "probe")],
                           input="int main(){return 0;}", text=True, capture_output=True)
    if probe.returncode != 0:
        pytest.skip("the toolchain has no sanitizer runtimes")
    built = subprocess.run(cmd, capture_output=True, text=True)
    assert built.returncode == 0, built.stderr[-4000:]
    given = np.concatenate([cornell[0], cornell[1], N.hand_made()])
    (tmp_path / "nodes.bin").write_bytes(given.tobytes())
    out = subprocess.run([exe, str(tmp_path / "nodes.bin")], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "node cook sanitize ok" in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]
    assert re.search(rf"{len(given)} given nodes, 4000 random nodes", out.stdout), out.stdout[-2000:]

"""Where the fused path kernel keeps its parked hits (gi_kernels.h pathLotPlacement, through giCDebugPathLot), without a GPU: the lot lies in the rows of the
per-lane traversal stack that no walk reaches -- a walk pushes at most bvhDepth entries -- and a launch asks for no LDS beyond those rows."""
import ctypes as C
import os
import re

import pytest

from gatling_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TRACE_BLOCK, ENTRY_BYTES, NODE_BYTES, TRI_BYTES, RECORD_BYTES = 256, 8, 80, 48, 64


def _lot(depth, nodes=5, tris=46):
    out = (C.c_uint32 * 4)()
    assert capi.load_library().giCDebugPathLot(depth, nodes, tris, out) == capi.GI_C_OK
    return tuple(int(v) for v in out)


@pytest.mark.parametrize("depth", range(1, 9))
def test_lot_rows_are_beyond_the_walks(depth):
    stack, row, cap, _ = _lot(depth)
    assert stack == (4 if depth <= 4 else 8)           # launchPath's rule, unchanged
    assert row >= depth                                # rows [0, depth) are the walks'
    records_per_row = 64 * ENTRY_BYTES // RECORD_BYTES  # a wave's 64 columns of one row
    assert cap == (stack - row) * records_per_row and row + cap // records_per_row <= stack


def test_capacities_of_the_trees_the_tests_use():
    assert _lot(1)[1:3] == (1, 24)   # cornell: rows 1 .. 3
    assert _lot(2)[1:3] == (2, 16)
    assert _lot(3)[1:3] == (3, 8)
    assert _lot(4)[1:3] == (4, 0)    # nothing free: the parking is off
    assert _lot(7)[1:3] == (7, 8)    # the telescope: row 7
    assert _lot(8)[1:3] == (8, 0)


@pytest.mark.parametrize("depth,nodes,tris", [(1, 5, 46), (4, 9, 128), (7, 30, 100), (8, 1, 1)])
def test_launch_lds_is_the_stack_and_the_staged_scene(depth, nodes, tris):
    """The parent's figure: stack rows + staged nodes + staged triangles, nothing for the lot (C2: 8 192 + 400 + 2 208 bytes)."""
    stack, _, _, lds = _lot(depth, nodes, tris)
    assert lds == stack * TRACE_BLOCK * ENTRY_BYTES + nodes * NODE_BYTES + tris * TRI_BYTES
    if (depth, nodes, tris) == (1, 5, 46):
        assert lds == 10800


def test_option_default_is_documented():
    hdr = open(os.path.join(ROOT, "gatling_amd", "csrc", "gi_kernels.h")).read()
    opt = open(os.path.join(ROOT, "gatling_amd", "csrc", "gi_options.h")).read()
    default = re.search(r"LOBE_PARK_DEFAULT\s*=\s*(\d+)", hdr).group(1)
    assert re.search(r"//\s+lobe_park\s+" + default + r"\s", opt)

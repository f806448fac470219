"""Helpers of tests/test_node_cook_host.py and tests/test_gpu_node_cook.py: hand-made and random Node8 records (they need not form a tree: the cooked form is made
node by node), the word a child adds to the hit mask, and the check of a cooked image against its nodes.  No test lives here."""
from __future__ import annotations

import numpy as np

import leaf_lift_trees as T

RECORD_DWORDS, TABLE_AT, OCT_MASK = 28, 20, 0xE0  # gi_node_cook.h


def contrib(meta: int, octant: int) -> int:
    """What trav_node_test ORs into the hit mask for a child with this meta byte when the ray's octant word (octinv & 7) is `octant`."""
    if meta == 0:
        return 0
    if (meta & 0x18) == 0x18:  # an internal child: (1 << 5) | (24 + slot)
        slot = (meta & 31) - 24
        return 1 << (24 + (slot ^ octant))
    return (meta >> 5) << (meta & 31)


def node(slots: dict, rng, child_base=1, tri_base=0):
    """One Node8 from {slot: "n" (an internal child) | 1 | 2 | 3 (a leaf of that many triangles)}; random frame and plane bytes, empty slots inverted
    (qlo 255, qhi 0) as the builder leaves them."""
    nd = np.zeros(1, T.NODE)[0]
    nd["p"] = rng.uniform(-1.0, 1.0, 3).astype(np.float32)
    nd["e"] = rng.integers(110, 125, 3)
    nd["childBase"], nd["triBase"] = child_base, tri_base
    nd["qlo"][:] = 255
    nd["qhi"][:] = 0
    off = 0
    for s in sorted(slots):
        lo = rng.integers(0, 200, 3)
        nd["qlo"][:, s] = lo
        nd["qhi"][:, s] = lo + rng.integers(1, 56, 3)
        if slots[s] == "n":
            nd["imask"] |= 1 << s
            nd["meta"][s] = (1 << 5) | (24 + s)
        else:
            nd["meta"][s] = (((1 << slots[s]) - 1) << 5) | off
            off += slots[s]
    assert off <= 24
    return nd


def hand_made(seed=7):
    """The node shapes the issue names: 0, 1, 3, 6 and 8 occupied slots; empty slots at the front, in the middle and at the end; internal children in high
    slots; leaves of 1, 2 and 3 triangles."""
    rng = np.random.default_rng(seed)
    shapes = [
        {},                                                          # no occupied slot
        {5: 2},                                                      # one, empty slots either side
        {0: 1, 3: "n", 7: 3},                                        # three: empty slots in the middle
        {2: 1, 3: 2, 4: 3, 5: "n", 6: "n", 7: 1},                     # six: empty slots at the front, internal children in high slots
        {0: 3, 1: 3, 2: "n", 3: 1, 4: 2, 5: 3},                       # six: empty slots at the end
        {0: 1, 1: 2, 2: 3, 3: 1, 4: 2, 5: 3, 6: 1, 7: 2},             # eight leaves, none internal
        {0: "n", 1: "n", 2: "n", 3: "n", 4: "n", 5: "n", 6: "n", 7: "n"},  # eight internal children
        {1: 3, 6: "n", 7: "n"},                                      # internal children in the two highest slots only
        {0: 2, 2: 2, 4: 2, 6: 2},                                    # every other slot
    ]
    return np.array([node(s, rng) for s in shapes], T.NODE)


def random_nodes(n, seed):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        slots = {}
        for s in range(8):
            kind = rng.integers(0, 4)
            if kind == 1:
                slots[s] = "n"
            elif kind >= 2:
                slots[s] = int(rng.integers(1, 4))
        out.append(node(slots, rng))
    return np.array(out, T.NODE)


def check_image(nodes, cooked):
    """Holds the cooked image of `nodes` (capi.node_cook) to its contract; returns the permutation of every node (child k of the record = slot perm[k])."""
    raw = np.frombuffer(nodes.tobytes(), "<u4").reshape(len(nodes), 20)
    recs, octs = cooked["records"], cooked["oct"]
    n, perms, inner_seen = len(nodes), [], 0
    for i, nd in enumerate(nodes):
        rec = recs[i]
        meta = [int(m) for m in nd["meta"]]
        occupied = [s for s in range(8) if meta[s] != 0]
        inner = any((m & 0x18) == 0x18 for m in meta)
        assert rec[:6].tobytes() == raw[i][:6].tobytes(), (i, "p, e | imask, childBase, triBase are copied")
        assert int(rec[6]) >> 16 == (len(occupied) + 1) & ~1 and int(rec[6]) & 0xFFFF == (OCT_MASK if inner else 0), (i, hex(int(rec[6])))
        if inner:
            assert i * RECORD_DWORDS * 4 + int(rec[7]) == n * RECORD_DWORDS * 4 + inner_seen * 256, (i, int(rec[7]), "its block of the octant area")
            tables = octs[inner_seen]
            assert not rec[TABLE_AT:].any()
            inner_seen += 1
        else:
            assert int(rec[7]) == TABLE_AT * 4
            tables = np.broadcast_to(rec[TABLE_AT:], (8, 8))
        # the table of octant 0 names each child's slot: a leaf's word starts at its triangle offset, an internal child's bit is 24 + slot
        perm = []
        for k in range(8):
            w = int(tables[0][k])
            if w == 0:
                continue
            idx = (w & -w).bit_length() - 1
            m = ((w >> idx) << 5) | idx
            assert m in meta, (i, k, hex(w))
            perm.append(meta.index(m))
        assert len(perm) == len(occupied) and sorted(perm) == occupied, (i, perm, occupied, "a bijection of the occupied slots")
        assert all(int(tables[0][k]) != 0 for k in range(len(occupied))), (i, "occupied slots come first")
        planes = rec[8:20].view(np.uint8).reshape(6, 8)
        want = np.concatenate([nd["qlo"], nd["qhi"]])
        for k, s in enumerate(perm):
            assert planes[:, k].tobytes() == want[:, s].tobytes(), (i, k, s, "plane bytes travel with their child")
        for o in range(8):
            for k in range(8):
                assert int(tables[o][k]) == (contrib(meta[perm[k]], o) if k < len(perm) else 0), (i, o, k)
        perms.append(perm)
    return perms

"""Helpers of tests/test_leaf_lift_host.py: Node8 decoding, the builder's padding and outward quantisation in numpy, hand-made
trees, the model cost, and a CPU walk with culling.  No test lives here."""
from __future__ import annotations

import numpy as np

NODE = np.dtype([("p", "<f4", 3), ("e", "u1", 3), ("imask", "u1"), ("childBase", "<u4"), ("triBase", "<u4"), ("meta", "u1", 8), ("qlo", "u1", (3, 8)),
                 ("qhi", "u1", (3, 8))])
assert NODE.itemsize == 80  # gi_types.h Node8
C_PRIM = 0.5               # bvh8.cpp cPrim of the flat tree


def decode(node_bytes):
    return np.frombuffer(np.ascontiguousarray(node_bytes).tobytes(), NODE).copy()


def slot_box(nd, s):
    """The fp32 planes the traversal evaluates for slot s: (lo, hi)."""
    scale = np.ldexp(np.float32(1.0), nd["e"].astype(np.int32) - 127).astype(np.float32)
    return (nd["p"] + nd["qlo"][:, s].astype(np.float32) * scale).astype(np.float32), (nd["p"] + nd["qhi"][:, s].astype(np.float32) * scale).astype(np.float32)


def is_internal(nd, s):
    return nd["meta"][s] != 0 and (nd["imask"] >> s) & 1 == 1


def is_leaf(nd, s):
    return nd["meta"][s] != 0 and (nd["imask"] >> s) & 1 == 0


def leaf_range(nd, s):
    """Positions in the tree's triangle order of leaf slot s."""
    cnt = bin(int(nd["meta"][s]) >> 5).count("1")
    first = int(nd["triBase"]) + (int(nd["meta"][s]) & 31)
    return list(range(first, first + cnt))


def children(nodes, i):
    """{slot: node index} of node i's internal slots."""
    out, rel = {}, 0
    for s in range(8):
        if is_internal(nodes[i], s):
            out[s] = int(nodes[i]["childBase"]) + rel; rel += 1
    return out


def levels(nodes):
    depth = np.zeros(len(nodes), np.int64); depth[0] = 1
    for i in range(len(nodes)):
        for c in children(nodes, i).values():
            depth[c] = depth[i] + 1
    return depth


def padded_box(tri):
    """bvh8.cpp Builder::prepareRange in fp32: the box of {v0, v0 + e1, v0 + e2} with e = v - v0, padded by 2^-20 of its magnitude."""
    t = np.asarray(tri, np.float32).reshape(3, 3)
    e1, e2 = (t[1] - t[0]).astype(np.float32), (t[2] - t[0]).astype(np.float32)
    pts = np.stack([t[0], (t[0] + e1).astype(np.float32), (t[0] + e2).astype(np.float32)])
    lo, hi = pts.min(0), pts.max(0)
    mag = (np.maximum(np.abs(lo), np.abs(hi)) + (hi - lo)).astype(np.float32)
    pad = (mag * np.float32(9.5367431640625e-7) + np.float32(1.0e-30)).astype(np.float32)
    return (lo - pad).astype(np.float32), (hi + pad).astype(np.float32)


def model_cost(nodes):
    """Sum over occupied slots of area(dequantised box) x (1 | cPrim x references), in float64."""
    cost = 0.0
    for nd in nodes:
        for s in range(8):
            if nd["meta"][s] == 0:
                continue
            lo, hi = slot_box(nd, s)
            d = (hi.astype(np.float64) - lo.astype(np.float64))
            area = 2.0 * (d[0] * d[1] + d[1] * d[2] + d[2] * d[0])
            cost += area if is_internal(nd, s) else area * C_PRIM * len(leaf_range(nd, s))
    return cost


# --- hand-made trees ---------------------------------------------------------------------------------------------------------------------------------------
def _exponent(extent):
    e = -126
    while 255.0 * np.ldexp(1.0, e) < float(extent) and e < 127:
        e += 1
    return e


def make_tree(spec):
    """spec: {slot: [triangles] | spec} -- a leaf slot's triangles (1 .. 3 arrays of 3 x 3) or a child node.  Returns (node bytes, triangles in leaf order, levels):
    breadth-first nodes, triangles in node order and slot order within a node, boxes quantised outward as the builder does."""
    order, tris = [spec], []
    i = 0
    while i < len(order):
        order += [v for _, v in sorted(order[i].items()) if isinstance(v, dict)]
        i += 1
    index = {id(n): k for k, n in enumerate(order)}

    def bounds(v):
        if isinstance(v, dict):
            bs = [bounds(c) for c in v.values()]
        else:
            bs = [padded_box(t) for t in v]
        return np.min([b[0] for b in bs], 0), np.max([b[1] for b in bs], 0)

    nodes = np.zeros(len(order), NODE)
    depth = {id(spec): 1}
    for k, n in enumerate(order):
        nd = nodes[k]
        lo, hi = bounds(n)
        nd["p"] = lo
        ex = [_exponent(hi[a] - lo[a]) for a in range(3)]
        nd["e"] = [x + 127 for x in ex]
        scale = [np.float32(np.ldexp(1.0, x)) for x in ex]
        kids = [v for _, v in sorted(n.items()) if isinstance(v, dict)]
        nd["childBase"] = index[id(kids[0])] if kids else len(order)
        nd["triBase"] = len(tris)
        off = 0
        for s in range(8):
            nd["qlo"][:, s] = 255; nd["qhi"][:, s] = 0
        for s, v in sorted(n.items()):
            blo, bhi = bounds(v)
            for a in range(3):
                ql = int(np.floor((float(blo[a]) - float(lo[a])) / float(scale[a]))); qh = int(np.ceil((float(bhi[a]) - float(lo[a])) / float(scale[a])))
                ql, qh = min(max(ql, 0), 255), min(max(qh, 0), 255)
                while ql > 0 and np.float32(lo[a] + np.float32(ql) * scale[a]) > blo[a]:
                    ql -= 1
                while qh < 255 and np.float32(lo[a] + np.float32(qh) * scale[a]) < bhi[a]:
                    qh += 1
                nd["qlo"][a, s] = ql; nd["qhi"][a, s] = qh
            if isinstance(v, dict):
                nd["imask"] |= 1 << s
                nd["meta"][s] = (1 << 5) | (24 + s)
                depth[id(v)] = depth[id(n)] + 1
            else:
                assert 1 <= len(v) <= 3
                nd["meta"][s] = (((1 << len(v)) - 1) << 5) | off
                tris += [np.asarray(t, np.float32).reshape(3, 3) for t in v]; off += len(v)
        assert off <= 24
    return nodes.tobytes(), np.asarray(tris, np.float32).reshape(-1, 3, 3), max(depth.values())


# --- closest hits ---------------------------------------------------------------------------------------------------------------------------------------------
def _hit_t(o, d, tri):
    """Moeller-Trumbore in float64, elementwise over rays (o, d: n x 3) against one triangle; t (inf: no hit)."""
    v0, e1, e2 = tri[0].astype(np.float64), (tri[1] - tri[0]).astype(np.float64), (tri[2] - tri[0]).astype(np.float64)
    px = d[:, 1] * e2[2] - d[:, 2] * e2[1]; py = d[:, 2] * e2[0] - d[:, 0] * e2[2]; pz = d[:, 0] * e2[1] - d[:, 1] * e2[0]
    det = e1[0] * px + e1[1] * py + e1[2] * pz
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = 1.0 / det
        tx, ty, tz = o[:, 0] - v0[0], o[:, 1] - v0[1], o[:, 2] - v0[2]
        u = (tx * px + ty * py + tz * pz) * inv
        qx = ty * e1[2] - tz * e1[1]; qy = tz * e1[0] - tx * e1[2]; qz = tx * e1[1] - ty * e1[0]
        v = (d[:, 0] * qx + d[:, 1] * qy + d[:, 2] * qz) * inv
        t = (e2[0] * qx + e2[1] * qy + e2[2] * qz) * inv
    ok = (np.abs(det) > 1e-300) & (u >= 0.0) & (v >= 0.0) & (u + v <= 1.0) & (t > 1e-9)
    return np.where(ok, t, np.inf)


def brute_force(tris, ids, o, d):
    """(t, id) of the closest hit per ray over every triangle; equal t: the lower id."""
    best_t = np.full(len(o), np.inf); best_id = np.full(len(o), -1, np.int64)
    for k in np.argsort(ids):
        t = _hit_t(o, d, tris[k])
        take = t < best_t  # (ids ascend: an equal t keeps the lower one)
        best_t = np.where(take, t, best_t); best_id = np.where(take, ids[k], best_id)
    return best_t, best_id


def _box_span(o, inv, lo, hi):
    t0 = (lo.astype(np.float64)[None, :] - o) * inv; t1 = (hi.astype(np.float64)[None, :] - o) * inv
    tn = np.maximum(np.minimum(t0, t1).max(1), 0.0); tf = np.maximum(t0, t1).min(1)
    return tn, tf


def walk(nodes, tris, ids, o, d):
    """Closest hits by a walk of the tree with culling: at a node the leaf slots whose box the ray meets in front of its best hit are tested, then the internal
    children near to far, each only if its box still begins in front of the best hit.  Returns (t, id, nodes visited in total).  Trees of up to two levels."""
    n = len(o)
    inv = 1.0 / np.where(np.abs(d) < 1e-30, np.where(d < 0, -1e-30, 1e-30), d)
    best_t = np.full(n, np.inf); best_id = np.full(n, -1, np.int64)

    def leaves(nd, active):
        nonlocal best_t, best_id
        for s in range(8):
            if not is_leaf(nd, s):
                continue
            tn, tf = _box_span(o, inv, *slot_box(nd, s))
            m = active & (tn * (1.0 - 1e-9) <= tf * (1.0 + 1e-9)) & (tn * (1.0 - 1e-9) <= best_t)
            for k in leaf_range(nd, s):
                t = np.where(m, _hit_t(o, d, tris[k]), np.inf)
                take = (t < best_t) | ((t == best_t) & np.isfinite(t) & (ids[k] < best_id))
                best_t = np.where(take, t, best_t); best_id = np.where(take, ids[k], best_id)

    visited = n
    leaves(nodes[0], np.ones(n, bool))
    kids = children(nodes, 0)
    if kids:
        slots = sorted(kids)
        near = np.full((n, len(slots)), np.inf)
        for j, s in enumerate(slots):
            assert nodes[kids[s]]["imask"] == 0
            tn, tf = _box_span(o, inv, *slot_box(nodes[0], s))
            near[:, j] = np.where(tn * (1.0 - 1e-9) <= tf * (1.0 + 1e-9), tn, np.inf)
        rank = np.argsort(near, axis=1, kind="stable")
        for r in range(len(slots)):
            for j, s in enumerate(slots):
                m = (rank[:, r] == j) & np.isfinite(near[:, j]) & (near[:, j] * (1.0 - 1e-9) <= best_t)
                visited += int(m.sum())
                leaves(nodes[kids[s]], m)
    return best_t, best_id, visited

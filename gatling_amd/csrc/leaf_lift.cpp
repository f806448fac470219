// leaf_lift.cpp -- liftLeafSlots (bvh8.h): a pass over a FINISHED Bvh8 that moves leaf slots of an internal child into free slots of its parent where the
// builder's own cost model says the tree gets cheaper to walk.
//
// Why: the binned top-down split of bvh8.cpp decides which triangles share a SUBTREE; the collapse then only chooses how a subtree is cut into 8-wide nodes.
// A leaf that the split put into a subtree it does not belong to (cornell: the two ceiling triangles beside the light's twelve) stretches that child's box in
// the parent over everything the leaf spans, and every ray through the stretched box pays a node visit for it.  When the parent has an empty slot, testing the
// leaf THERE costs the same triangle tests and lets the child's box shrink to the rest.  For trees the fused kernel walks out of LDS (a root and one level
// below it) a node visit is a whole wave-wide step of the closest-hit loop (gi_path.hip), so fewer second visits are fewer steps per trip.
//
// What a move leaves alone: node count, childBase, imask, levelStart, maxDepth, breadth-first order, every node's quantisation frame (p, e), origId of every
// record.  What it changes: two slots of the parent (the child's box, the lifted leaf), one slot of the child (emptied), and the order of `tris`, which is
// laid out again by the builder's rule (node order, slot order within a node) so that triBase + offset names every leaf's triangles.  The boxes it writes are
// quantised outward with the builder's arithmetic, so the conservativeness contract of bvh8.cpp holds; images do not depend on the tree (DESIGN.md "Traversal
// contract").
//
// The model: sum over occupied slots of area(dequantised slot box) x (1 for an internal slot | cPrim x references for a leaf slot) -- the collapse's cost
// (bvh8.cpp dpNode) over the planes the traversal tests, as gi_debug.cpp's tlasModelCost evaluates it.  A move is applied only when that sum strictly
// decreases; the best move first, until none is left.  Equal cost: no move -- the pass is deterministic and a second run changes nothing.

#include "bvh8.h"

#include <algorithm>
#include <cmath>
#include <cstring>

namespace gi {
namespace {

constexpr float kCPrim = 0.5f;          // bvh8.cpp cPrim of the flat tree (gi_bvh_stages.h kBvhCPrim)
constexpr uint32_t kMaxNodeRefs = 24u;  // leaf references of one node: offsets 24 .. 31 of the 5-bit field name internal slots (gi_types.h Node8::meta)

struct Box3 {
  float lo[3], hi[3];
  void reset() { for (int a = 0; a < 3; a++) { lo[a] = 3.0e38f; hi[a] = -3.0e38f; } }
  void grow(const Box3& b) { for (int a = 0; a < 3; a++) { lo[a] = std::min(lo[a], b.lo[a]); hi[a] = std::max(hi[a], b.hi[a]); } }
  void grow(const float* p) { for (int a = 0; a < 3; a++) { lo[a] = std::min(lo[a], p[a]); hi[a] = std::max(hi[a], p[a]); } }
  bool contains(const Box3& b) const { for (int a = 0; a < 3; a++) if (b.lo[a] < lo[a] || b.hi[a] > hi[a]) return false; return true; }
  float area() const {
    float dx = hi[0] - lo[0], dy = hi[1] - lo[1], dz = hi[2] - lo[2];
    if (dx < 0.0f) return 0.0f;
    return 2.0f * (dx * dy + dy * dz + dz * dx);
  }
};

// the padded box the builder gives a triangle (bvh8.cpp Builder::prepareRange, operation for operation)
Box3 paddedTriBox(const TriRec& t)
{
  Box3 b; b.reset();
  float p1[3], p2[3];
  for (int a = 0; a < 3; a++) { p1[a] = t.v0[a] + t.e1[a]; p2[a] = t.v0[a] + t.e2[a]; }
  b.grow(t.v0); b.grow(p1); b.grow(p2);
  for (int a = 0; a < 3; a++) {
    float mag = std::max(std::fabs(b.lo[a]), std::fabs(b.hi[a])) + (b.hi[a] - b.lo[a]);
    float pad = mag * 9.5367431640625e-7f /* 2^-20 */ + 1.0e-30f;
    b.lo[a] -= pad; b.hi[a] += pad;
  }
  return b;
}

float slotScale(const Node8& n, int a) { uint32_t eb = (uint32_t)n.e[a] << 23; float scale; memcpy(&scale, &eb, 4); return scale; }

// the fp32 planes the traversal evaluates for slot s
Box3 slotBox(const Node8& n, int s)
{
  Box3 b;
  for (int a = 0; a < 3; a++) { const float scale = slotScale(n, a); b.lo[a] = n.p[a] + (float)n.qlo[a][s] * scale; b.hi[a] = n.p[a] + (float)n.qhi[a][s] * scale; }
  return b;
}

struct QBox { uint8_t lo[3], hi[3]; };

// `box` quantised outward in n's frame (bvh8.cpp's emit loop, operation for operation); false: the frame cannot hold it
bool quantiseOutward(const Node8& n, const Box3& box, QBox& q)
{
  for (int a = 0; a < 3; a++) {
    const float scale = slotScale(n, a);
    int lo = (int)std::floor(((double)box.lo[a] - (double)n.p[a]) / (double)scale);
    int hi = (int)std::ceil(((double)box.hi[a] - (double)n.p[a]) / (double)scale);
    lo = std::min(std::max(lo, 0), 255); hi = std::min(std::max(hi, 0), 255);
    while (lo > 0 && n.p[a] + (float)lo * scale > box.lo[a]) lo--;
    while (hi < 255 && n.p[a] + (float)hi * scale < box.hi[a]) hi++;
    if (n.p[a] + (float)lo * scale > box.lo[a] || n.p[a] + (float)hi * scale < box.hi[a]) return false;
    q.lo[a] = (uint8_t)lo; q.hi[a] = (uint8_t)hi;
  }
  return true;
}

Box3 dequantised(const Node8& n, const QBox& q)
{
  Box3 b;
  for (int a = 0; a < 3; a++) { const float scale = slotScale(n, a); b.lo[a] = n.p[a] + (float)q.lo[a] * scale; b.hi[a] = n.p[a] + (float)q.hi[a] * scale; }
  return b;
}

bool isInternal(const Node8& n, int s) { return n.meta[s] != 0 && ((n.imask >> s) & 1u); }
bool isLeaf(const Node8& n, int s) { return n.meta[s] != 0 && !((n.imask >> s) & 1u); }
uint32_t leafCount(const Node8& n, int s) { uint32_t c = 0; for (uint32_t u = n.meta[s] >> 5; u; u >>= 1) c += u & 1u; return c; }

struct Move { uint32_t parent, child; int childSlot, leafSlot, freeSlot; QBox childBox, leafBox; double gain; };

} // namespace

double bvh8ModelCost(const std::vector<Node8>& nodes)
{
  double cost = 0.0;
  for (const Node8& n : nodes)
    for (int s = 0; s < 8; s++) {
      if (n.meta[s] == 0) continue;
      const double area = (double)slotBox(n, s).area();
      cost += isInternal(n, s) ? area : area * (double)kCPrim * (double)leafCount(n, s);
    }
  return cost;
}

uint32_t liftLeafSlots(Bvh8& bvh)
{
  std::vector<Node8>& nodes = bvh.nodes;
  if (bvh.maxDepth > kLeafLiftMaxDepth || nodes.size() < 2u || bvh.activeTris == 0u) return 0u;
  for (size_t i = 0; i < nodes.size(); i++) { // (not a tree of the builder's -- a child in front of its parent or outside the array: left alone)
    const uint32_t internal = (uint32_t)__builtin_popcount(nodes[i].imask);
    if (internal && ((size_t)nodes[i].childBase <= i || (size_t)nodes[i].childBase + internal > nodes.size())) return 0u;
  }
  // every leaf slot's records, by position in bvh.tris (the records move once, at the end)
  std::vector<uint32_t> slotTris(nodes.size() * 8u * 3u, 0u);
  for (size_t i = 0; i < nodes.size(); i++)
    for (int s = 0; s < 8; s++) {
      if (!isLeaf(nodes[i], s)) continue;
      const uint32_t cnt = leafCount(nodes[i], s), first = nodes[i].triBase + (nodes[i].meta[s] & 31u);
      if (cnt > 3u || (size_t)first + cnt > bvh.activeTris) return 0u; // (not a tree of the builder's: left alone)
      for (uint32_t k = 0; k < cnt; k++) slotTris[(i * 8u + (size_t)s) * 3u + k] = first + k;
    }
  uint32_t lifted = 0u;
  for (size_t round = 0; round < nodes.size() * 8u; round++) { // (every move empties a slot below the root level: the loop ends long before)
    Move best{}; best.gain = 0.0; bool found = false;
    for (uint32_t pi = 0; pi < (uint32_t)nodes.size(); pi++) {
      const Node8& P = nodes[pi];
      if (P.imask == 0u) continue;
      uint32_t refs = 0; bool anyFree = false;
      Box3 pb; pb.reset();
      for (int s = 0; s < 8; s++) { if (P.meta[s] == 0) { anyFree = true; continue; } pb.grow(slotBox(P, s)); if (isLeaf(P, s)) refs += leafCount(P, s); }
      if (!anyFree) continue;
      uint32_t rel = 0;
      for (int sc = 0; sc < 8; sc++) {
        if (!isInternal(P, sc)) continue;
        const uint32_t ci = P.childBase + rel; rel++;
        if (ci >= nodes.size() || ci <= pi) continue; // (checked above for every node; kept beside the access)
        const Node8& C = nodes[ci];
        int occupied = 0; for (int s = 0; s < 8; s++) if (C.meta[s] != 0) occupied++;
        if (occupied < 2) continue; // the child keeps at least one slot
        const Box3 childOld = slotBox(P, sc);
        for (int sl = 0; sl < 8; sl++) {
          if (!isLeaf(C, sl)) continue;
          const uint32_t cnt = leafCount(C, sl);
          if (refs + cnt > kMaxNodeRefs) continue;
          // the child's box from what it keeps, the leaf's from its triangles' padded boxes (as the builder makes a leaf slot's box), both in P's frame
          Box3 rest; rest.reset();
          for (int s = 0; s < 8; s++) if (s != sl && C.meta[s] != 0) rest.grow(slotBox(C, s));
          Box3 leaf; leaf.reset();
          for (uint32_t k = 0; k < cnt; k++) leaf.grow(paddedTriBox(bvh.tris[slotTris[((size_t)ci * 8u + (size_t)sl) * 3u + k]]));
          Move m{}; m.parent = pi; m.child = ci; m.childSlot = sc; m.leafSlot = sl;
          if (!quantiseOutward(P, rest, m.childBox) || !quantiseOutward(P, leaf, m.leafBox)) continue;
          const double before = (double)childOld.area() + (double)slotBox(C, sl).area() * (double)kCPrim * (double)cnt;
          const double after = (double)dequantised(P, m.childBox).area() + (double)dequantised(P, m.leafBox).area() * (double)kCPrim * (double)cnt;
          m.gain = before - after;
          if (!(m.gain > best.gain)) continue; // (equal cost: no move; equal gains: the first candidate in node, slot order)
          // the free slot the builder's octant assignment prefers: the largest projection of the leaf's centre, seen from the node's, on the slot's direction
          float d[3]; for (int a = 0; a < 3; a++) d[a] = 0.5f * (leaf.lo[a] + leaf.hi[a]) - 0.5f * (pb.lo[a] + pb.hi[a]);
          int bs = -1; float bc = -3.0e38f;
          for (int s = 0; s < 8; s++) {
            if (P.meta[s] != 0) continue;
            const float c = ((s & 1) ? d[0] : -d[0]) + ((s & 2) ? d[1] : -d[1]) + ((s & 4) ? d[2] : -d[2]);
            if (c > bc) { bc = c; bs = s; }
          }
          if (bs < 0) continue;
          m.freeSlot = bs; best = m; found = true;
        }
      }
    }
    if (!found) break;
    Node8& P = nodes[best.parent]; Node8& C = nodes[best.child];
    const uint32_t cnt = leafCount(C, best.leafSlot);
    for (int a = 0; a < 3; a++) {
      P.qlo[a][best.childSlot] = best.childBox.lo[a]; P.qhi[a][best.childSlot] = best.childBox.hi[a];
      P.qlo[a][best.freeSlot] = best.leafBox.lo[a]; P.qhi[a][best.freeSlot] = best.leafBox.hi[a];
      C.qlo[a][best.leafSlot] = 255; C.qhi[a][best.leafSlot] = 0; // an empty slot as the builder writes it
    }
    P.meta[best.freeSlot] = (uint8_t)(C.meta[best.leafSlot] & 0xe0u); // the unary count; the offset is assigned below
    C.meta[best.leafSlot] = 0;
    for (uint32_t k = 0; k < cnt; k++)
      slotTris[((size_t)best.parent * 8u + (size_t)best.freeSlot) * 3u + k] = slotTris[((size_t)best.child * 8u + (size_t)best.leafSlot) * 3u + k];
    lifted++;
  }
  if (lifted == 0u) return 0u;
  // the builder's layout again: triangles in node order, slot order within a node; inactive records stay behind the active ones
  std::vector<TriRec> laid(bvh.tris.size());
  uint32_t next = 0;
  for (size_t i = 0; i < nodes.size(); i++) {
    Node8& n = nodes[i];
    n.triBase = next;
    uint32_t off = 0;
    for (int s = 0; s < 8; s++) {
      if (!isLeaf(n, s)) continue;
      const uint32_t cnt = leafCount(n, s);
      n.meta[s] = (uint8_t)((n.meta[s] & 0xe0u) | off);
      for (uint32_t k = 0; k < cnt; k++) laid[next + off + k] = bvh.tris[slotTris[(i * 8u + (size_t)s) * 3u + k]];
      off += cnt;
    }
    next += off;
  }
  for (size_t i = next; i < bvh.tris.size(); i++) laid[i] = bvh.tris[i];
  bvh.tris.swap(laid);
  return lifted;
}

} // namespace gi

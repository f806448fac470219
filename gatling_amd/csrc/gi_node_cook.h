// gi_node_cook.h -- the cooked form of a Node8 (gi_types.h) that k_path's COOK variants read out of LDS, and cook_node, the one function that makes it: on
// the device when a block stages its scene (gi_traversal.h stage_scene_cooked), on the host for the tests (giCDebugNodeCook, tests/cpp/node_cook_sanitize.cpp).
//
// What trav_node_test decodes per visit and per lane is a function of the node and the ray's octant alone: for each child, the word that goes into the hit
// mask when its box is hit.  A cooked node carries those words as a table, and its children are enumerated occupied slots first, so that a wave can leave the
// child loop once no lane has an occupied slot left.  The quantised plane bytes, the frame and every floating-point operation of the box test are untouched.
//
// A cooked node is COOK_NODE_DWORDS dwords at a fixed stride:
//   [0..2]   p[3]                       as in Node8
//   [3]      e[3] | imask << 24         as in Node8
//   [4], [5] childBase, triBase         as in Node8
//   [6]      occupied slots, rounded up to 2, << 16 | COOK_OCT_MASK when the node has an internal child (else 0)
//   [7]      byte offset from the record's start to its table of octant 0
//   [8..19]  qlo[3][8], qhi[3][8] in Node8's order of planes, child k of the record = slot perm[k] of the node: occupied slots first, in slot order
//   [20..27] the table of a node without internal children: entry k = the word trav_node_test ORs into the hit mask for child k
// A node with an internal child has eight tables, one per ray octant (octinv & 7), COOK_TABLE_DWORDS apart, in the octant area behind the records ([7] points
// there; its [20..27] are zero).  The j-th such node of the array owns the j-th block of the area, so a record's place depends on the nodes before it only
// through cook_inner_before.  The table address of a lane is record + [7] + ((octinv >> 3) & [6]): bits 5-7 of that word are the octant times 32.
#pragma once

#include <stdint.h>

#include "gi_types.h"

#if defined(__HIP__)
#define GI_COOK_HD __host__ __device__
#else
#define GI_COOK_HD
#endif

namespace gi {

constexpr uint32_t COOK_NODE_DWORDS = 28, COOK_NODE_BYTES = COOK_NODE_DWORDS * 4u; // 112: seven 16-byte pieces
constexpr uint32_t COOK_TABLE_DWORDS = 8, COOK_OCT_DWORDS = 8u * COOK_TABLE_DWORDS;  // the eight tables of a node with internal children: 256 bytes
constexpr uint32_t COOK_OCT_MASK = 0xe0u;
constexpr uint32_t COOK_TABLE_AT = 20; // dword of the inline table

// the 20 dwords of a Node8, read as words (p[] is copied, never computed with)
GI_COOK_HD inline uint32_t cook_meta(const uint32_t* w, uint32_t slot) { return (w[6u + (slot >> 2)] >> (8u * (slot & 3u))) & 0xffu; }
// an internal child's meta byte is (1 << 5) | (24 + slot): bits 4 and 3 set, which no triangle offset (< 24) has -- trav_node_test's `inner4`
GI_COOK_HD inline bool cook_meta_inner(uint32_t m) { return (m & 0x18u) == 0x18u; }
GI_COOK_HD inline bool cook_has_inner(const uint32_t* w)
{
  for (uint32_t s = 0; s < 8u; s++) if (cook_meta_inner(cook_meta(w, s))) return true;
  return false;
}
// how many of the nodes [0, i) have an internal child: the block of the octant area node i takes when it has one itself
GI_COOK_HD inline uint32_t cook_inner_before(const Node8* nodes, uint32_t i)
{
  uint32_t n = 0;
  for (uint32_t j = 0; j < i; j++) n += cook_has_inner(reinterpret_cast<const uint32_t*>(&nodes[j])) ? 1u : 0u;
  return n;
}
// Octant blocks an array of n nodes can need: a node with an internal child has a child node, and every node but the root is the child of one node, so at most
// n - 1 nodes have one (a chain).  The launch sizes the area by this bound: it knows the node count, not the nodes.
GI_COOK_HD inline uint32_t cook_oct_blocks_max(uint32_t n) { return n ? n - 1u : 0u; }
GI_COOK_HD inline uint32_t cook_image_bytes(uint32_t n) { return n * COOK_NODE_BYTES + cook_oct_blocks_max(n) * COOK_OCT_DWORDS * 4u; }
// the word trav_node_test ORs into the hit mask for a child with meta byte m when the ray's octant word is oct (octinv & 7)
GI_COOK_HD inline uint32_t cook_contrib(uint32_t m, uint32_t oct)
{
  const uint32_t idx = cook_meta_inner(m) ? (m ^ oct) & 0x1fu : m & 0x1fu;
  return (m >> 5) << idx;
}

// Cooks `node` into rec[COOK_NODE_DWORDS].  tableOff: the byte offset from rec to where the node's table of octant 0 lies -- COOK_TABLE_AT * 4 for a node
// without internal children, whose table is written into the record; for a node with one, the offset of oct[COOK_OCT_DWORDS], which gets the eight tables.
// `oct` is not touched for a node without internal children.
GI_COOK_HD inline void cook_node(const Node8& node, uint32_t tableOff, uint32_t* rec, uint32_t* oct)
{
  const uint32_t* w = reinterpret_cast<const uint32_t*>(&node);
  uint32_t perm[8], meta[8], n = 0;
  for (uint32_t s = 0; s < 8u; s++) if (cook_meta(w, s) != 0u) perm[n++] = s;
  const uint32_t occupied = n;
  for (uint32_t s = 0; s < 8u; s++) if (cook_meta(w, s) == 0u) perm[n++] = s;
  for (uint32_t k = 0; k < 8u; k++) meta[k] = cook_meta(w, perm[k]);
  const bool inner = oct != nullptr && cook_has_inner(w);
  for (uint32_t i = 0; i < 6u; i++) rec[i] = w[i];
  rec[6] = (((occupied + 1u) & ~1u) << 16) | (inner ? COOK_OCT_MASK : 0u);
  rec[7] = tableOff;
  for (uint32_t plane = 0; plane < 6u; plane++) { // qlo x, y, z, qhi x, y, z: two words of four children each
    for (uint32_t h = 0; h < 2u; h++) {
      uint32_t v = 0u;
      for (uint32_t k = 0; k < 4u; k++) {
        const uint32_t s = perm[4u * h + k];
        v |= ((w[8u + 2u * plane + (s >> 2)] >> (8u * (s & 3u))) & 0xffu) << (8u * k);
      }
      rec[8u + 2u * plane + h] = v;
    }
  }
  for (uint32_t k = 0; k < 8u; k++) rec[COOK_TABLE_AT + k] = inner ? 0u : cook_contrib(meta[k], 0u);
  if (inner) for (uint32_t o = 0; o < 8u; o++) for (uint32_t k = 0; k < 8u; k++) oct[o * COOK_TABLE_DWORDS + k] = cook_contrib(meta[k], o);
}

// Node i of the image of n nodes as a block stages it: n records, then an octant area of `blocks` blocks (a tree: cook_oct_blocks_max(n), which makes
// cook_image_bytes(n) bytes; blocks no node takes stay as they are).
GI_COOK_HD inline void cook_place(const Node8* nodes, uint32_t i, uint32_t n, uint32_t blocks, uint32_t* image)
{
  uint32_t* rec = image + i * COOK_NODE_DWORDS;
  const uint32_t block = cook_has_inner(reinterpret_cast<const uint32_t*>(&nodes[i])) ? cook_inner_before(nodes, i) : 0xffffffffu;
  // (a block beyond the bound: the array is no tree -- the record stays inside the image and the walk inside the array, whatever it then computes)
  if (block >= blocks) { cook_node(nodes[i], COOK_TABLE_AT * 4u, rec, nullptr); return; }
  uint32_t* oct = image + n * COOK_NODE_DWORDS + block * COOK_OCT_DWORDS;
  cook_node(nodes[i], (uint32_t)(oct - rec) * 4u, rec, oct);
}

} // namespace gi

// gi_refit.h -- the per-node arithmetic of a BVH8 refit (gi_refit.hip k_refit_level, gi_build.cpp updateVertices), shared by the device
// kernels and the host: a tree keeps its topology (imask, meta, childBase, triBase) and gets the conservative boxes of moved triangles.  Every operation is
// the one bvh8.cpp (prepareRange, exponentFor, the outward rounding and its fix-up loops) and gi_bvh_build.hip (k_bvh_boxes, exponent_for, k_bvh_write) run,
// in their order, without contraction: a refit of unchanged triangles writes the bytes either builder wrote, and the host reproduces the device's bytes
// (giCDebugSceneRefitCheck).  Minima and maxima are spelled out (no fminf / std::min) so that both sides pick the same operand.
#pragma once

#include <cmath>
#include <cstdint>

#include "gi_types.h"

#if defined(__HIP__)
#define GI_REFIT_HD __host__ __device__
#else
#define GI_REFIT_HD
#endif

namespace gi {

GI_REFIT_HD inline float refit_min(float a, float b) { return b < a ? b : a; }
GI_REFIT_HD inline float refit_max(float a, float b) { return a < b ? b : a; }
GI_REFIT_HD inline bool refit_usable(float x) { return fabsf(x) <= 1.0e18f; } // bvh8.cpp Builder::usable (false for NaN)

// bvh8.cpp exponentFor: smallest e with 255 * 2^e >= extent
GI_REFIT_HD inline int refit_exponent_for(float extent)
{
  if (!(extent > 0.0f)) return -126;
  int e; const float m = frexpf(extent / 255.0f, &e);
  if (m == 0.5f) e -= 1;
  e = e < -126 ? -126 : (e > 127 ? 127 : e);
  while (255.0f * ldexpf(1.0f, e) < extent && e < 127) e++;
  return e;
}

// gi_build.cpp flattenTriangle: the world-space record of a mesh triangle with object-space corners p under the 3x4 affine o2w (xformPoint's operation order)
GI_REFIT_HD inline void refit_flatten(const float* o2w, const float p[3][3], float v0[3], float e1[3], float e2[3])
{
  float q[3][3];
  for (int k = 0; k < 3; k++)
    for (int r = 0; r < 3; r++) q[k][r] = ((o2w[4 * r] * p[k][0] + o2w[4 * r + 1] * p[k][1]) + o2w[4 * r + 2] * p[k][2]) + o2w[4 * r + 3];
  for (int a = 0; a < 3; a++) { v0[a] = q[0][a]; e1[a] = q[1][a] - q[0][a]; e2[a] = q[2][a] - q[0][a]; }
}

// An instance update (gi_build.cpp updateTopology, gi_patch.hip k_clone_parts) makes a new instance of a resident mesh from a live sibling instance: the
// record `src` of the sibling becomes the record of instance `instance` (transform o2w) at the same position of its own range.  prim, matFlags and vi are
// the mesh's and stay; the id is the new instance's base + prim (flattenInstance numbers an instance's triangles in face order); v0 / e1 / e2 are made from
// the mesh triangle's object-space corners p (TriShade::p of the record vi[0] names) by flattenTriangle's operations in its order, so the 64 bytes are a fresh
// build's.  The caller has established that the new instance is usable (no inactive marker to carry).
GI_REFIT_HD inline TriRec refit_clone_record(const TriRec& src, const float* o2w, const float p[3][3], uint32_t instance, uint32_t idBase)
{
  TriRec t = src;
  t.instance = instance; t.origId = idBase + src.prim;
  refit_flatten(o2w, p, t.v0, t.e1, t.e2);
  return t;
}

// bvh8.cpp prepareRange: the padded box of the triangle {v0, v0 + e1, v0 + e2}; false (and no box) for an inactive one
GI_REFIT_HD inline bool refit_tri_box(const float v0[3], const float e1[3], const float e2[3], float lo[3], float hi[3])
{
  float p1[3], p2[3]; bool dead = false;
  for (int a = 0; a < 3; a++) { p1[a] = v0[a] + e1[a]; p2[a] = v0[a] + e2[a]; if (!refit_usable(v0[a]) || !refit_usable(p1[a]) || !refit_usable(p2[a])) dead = true; }
  if (dead) return false;
  for (int a = 0; a < 3; a++) {
    float l = refit_min(refit_min(refit_min(3.0e38f, v0[a]), p1[a]), p2[a]), h = refit_max(refit_max(refit_max(-3.0e38f, v0[a]), p1[a]), p2[a]);
    const float mag = refit_max(fabsf(l), fabsf(h)) + (h - l);
    const float pad = mag * 9.5367431640625e-7f /* 2^-20 */ + 1.0e-30f;
    lo[a] = l - pad; hi[a] = h + pad;
  }
  return true;
}

// gi_build.cpp packTriShade as a gather: the shading record of a mesh face is the FVertex records of its three corners (named by vi[k], absolute indices)
// laid out per attribute.  packVertex and packTriShade run the same sanitising and the same encode / decode on the same inputs, so the gathered words are
// bytewise packTriShade's (giCDebugGatherShade holds that).  Words 0..35 of the 40-word record are gathered -- p 0..8, n 9..17, t 18..26, uv 27..32, bsign
// 33..35 --, vi and pad (36..39) are read, never written.  A record with a corner outside the vertex array is left as it is (cannot happen: giCCreateMesh
// checks the faces).  Words are moved as integers: no float operation touches them.
constexpr uint32_t kShadeGatherWords = 36u;
GI_REFIT_HD inline bool refit_shade_corners_ok(const uint32_t vi[3], uint32_t vertCount) { return vi[0] < vertCount && vi[1] < vertCount && vi[2] < vertCount; }
// word w < 36 of the record with corners vi (all three inside the array)
GI_REFIT_HD inline uint32_t refit_shade_word(const FVertex* verts, const uint32_t vi[3], uint32_t w)
{
  uint32_t k, src; // corner, word of its FVertex (pos 0..2, bsign 3, normal 4..6, u 7, tangent 8..10, v 11)
  if (w < 27u) { k = (w % 9u) / 3u; src = (w / 9u) * 4u + w % 3u; }
  else if (w < 33u) { k = (w - 27u) >> 1; src = ((w - 27u) & 1u) ? 11u : 7u; }
  else { k = w - 33u; src = 3u; }
  uint32_t out;
  __builtin_memcpy(&out, reinterpret_cast<const char*>(verts + vi[k]) + 4u * src, 4);
  return out;
}
GI_REFIT_HD inline void refit_gather_shade(const FVertex* verts, uint32_t vertCount, TriShade& q)
{
  if (!refit_shade_corners_ok(q.vi, vertCount)) return;
  char* words = reinterpret_cast<char*>(&q);
  for (uint32_t w = 0; w < kShadeGatherWords; w++) { const uint32_t x = refit_shade_word(verts, q.vi, w); __builtin_memcpy(words + 4u * w, &x, 4); }
}

// What a refit reads beside the nodes.  `instances` / `triShade` may be null (a tree over bare triangles, giCDebugRefitBvh): they give a record whose edges
// the incremental visibility path zeroed (gi_patch.hip k_patch_visibility, flat layouts) the box of the triangle it will be again when the mesh is shown.
struct RefitScene {
  const TriRec* tris; uint32_t triCount;
  const InstanceRec* instances; uint32_t instanceCount;
  const TriShade* triShade; uint32_t shadeCount;
};

// the box of the resident record `ti` (false: inactive, or out of range -- which cannot happen in a tree that validates)
GI_REFIT_HD inline bool refit_record_box(const RefitScene& S, uint32_t ti, float lo[3], float hi[3])
{
  if (ti >= S.triCount) return false;
  const TriRec& t = S.tris[ti];
  float v0[3], e1[3], e2[3]; bool zero = true;
  for (int a = 0; a < 3; a++) { v0[a] = t.v0[a]; e1[a] = t.e1[a]; e2[a] = t.e2[a]; if (e1[a] != 0.0f || e2[a] != 0.0f) zero = false; }
  if (zero && S.triShade && S.instances && t.vi[0] < S.shadeCount && t.instance < S.instanceCount) {
    float w0[3];
    refit_flatten(S.instances[t.instance].o2w, S.triShade[t.vi[0]].p, w0, e1, e2); // (v0 is never zeroed: it stays the record's)
  }
  return refit_tri_box(v0, e1, e2, lo, hi);
}

// One node.  boxes: 8 floats per node (min xyz, -, max xyz, -), indexed like the nodes; the entries of the node's internal children must have been written
// (they lie one level down: an earlier launch, or a higher index on the host).  Takes each occupied slot's exact float box -- a leaf slot's: the union of its
// records' padded boxes; an internal slot's: the child's entry --, writes the node's own entry (their union) and requantises the node against it: p = the
// box minimum, e = exponent_for(extent), qlo / qhi rounded outwards and fixed up against the fp32 planes the traversal evaluates.  Empty slots keep 255 / 0;
// imask, meta, childBase and triBase are not touched.  A node without an occupied slot (the empty root, a reserved slot of a partitioned range) is left as
// it is and gets an inverted box.
// `leaf(ti, lo, hi)` is the leaf-box provider: the padded box of the item a leaf slot names, false where it contributes nothing.  The flat tree's is
// refit_record_box over the resident records (RefitSceneLeaf, refit_node below); a BLAS of the two-level layout has its own (gi_blas.h).
template <class Leaf>
GI_REFIT_HD inline void refit_node_with(Node8* nodes, uint32_t nodeCount, uint32_t ni, float* boxes, const Leaf& leaf)
{
  Node8 n = nodes[ni];
  float slo[8][3], shi[8][3]; uint32_t occupied = 0, rel = 0;
  float nlo[3] = {3.0e38f, 3.0e38f, 3.0e38f}, nhi[3] = {-3.0e38f, -3.0e38f, -3.0e38f};
  for (int s = 0; s < 8; s++) {
    const uint32_t meta = n.meta[s];
    if (meta == 0u) continue;
    float lo[3] = {3.0e38f, 3.0e38f, 3.0e38f}, hi[3] = {-3.0e38f, -3.0e38f, -3.0e38f};
    if ((n.imask >> s) & 1u) {
      const uint32_t c = n.childBase + rel; rel++;
      if (c <= ni || c >= nodeCount) continue; // (cannot happen: children lie behind their parent)
      for (int a = 0; a < 3; a++) { lo[a] = boxes[8 * (size_t)c + a]; hi[a] = boxes[8 * (size_t)c + 4 + a]; }
    } else {
      const uint32_t unary = meta >> 5, off = meta & 31u, cnt = unary == 1u ? 1u : unary == 3u ? 2u : unary == 7u ? 3u : 0u;
      for (uint32_t k = 0; k < cnt; k++) {
        float tl[3], th[3];
        if (!leaf(n.triBase + off + k, tl, th)) continue;
        for (int a = 0; a < 3; a++) { lo[a] = refit_min(lo[a], tl[a]); hi[a] = refit_max(hi[a], th[a]); }
      }
    }
    if (!(lo[0] <= hi[0])) continue; // nothing below: the slot keeps its planes
    occupied |= 1u << s;
    for (int a = 0; a < 3; a++) { slo[s][a] = lo[a]; shi[s][a] = hi[a]; nlo[a] = refit_min(nlo[a], lo[a]); nhi[a] = refit_max(nhi[a], hi[a]); }
  }
  for (int a = 0; a < 3; a++) { boxes[8 * (size_t)ni + a] = nlo[a]; boxes[8 * (size_t)ni + 4 + a] = nhi[a]; }
  boxes[8 * (size_t)ni + 3] = 0.0f; boxes[8 * (size_t)ni + 7] = 0.0f;
  if (!occupied) return;
  float scale[3];
  for (int a = 0; a < 3; a++) { n.p[a] = nlo[a]; const int ex = refit_exponent_for(nhi[a] - nlo[a]); n.e[a] = (uint8_t)(ex + 127); scale[a] = ldexpf(1.0f, ex); }
  for (int s = 0; s < 8; s++) {
    if (!((occupied >> s) & 1u)) continue;
    for (int a = 0; a < 3; a++) {
      int lo = (int)floor(((double)slo[s][a] - (double)n.p[a]) / (double)scale[a]);
      int hi = (int)ceil(((double)shi[s][a] - (double)n.p[a]) / (double)scale[a]);
      lo = lo < 0 ? 0 : (lo > 255 ? 255 : lo); hi = hi < 0 ? 0 : (hi > 255 ? 255 : hi);
      while (lo > 0 && n.p[a] + (float)lo * scale[a] > slo[s][a]) lo--;
      while (hi < 255 && n.p[a] + (float)hi * scale[a] < shi[s][a]) hi++;
      n.qlo[a][s] = (uint8_t)lo; n.qhi[a][s] = (uint8_t)hi;
    }
  }
  nodes[ni] = n;
}
struct RefitSceneLeaf {
  const RefitScene& S;
  GI_REFIT_HD bool operator()(uint32_t ti, float lo[3], float hi[3]) const { return refit_record_box(S, ti, lo, hi); }
};
GI_REFIT_HD inline void refit_node(Node8* nodes, uint32_t nodeCount, uint32_t ni, float* boxes, const RefitScene& S)
{
  refit_node_with(nodes, nodeCount, ni, boxes, RefitSceneLeaf{S});
}

// The whole refit on the host: every node from `firstNode` on, children before parents (both builders and the partitioned layout place children behind
// their parent, so descending index order is a valid one).  `boxes`: 8 floats per node of the array.
inline void refitHost(Node8* nodes, uint32_t nodeCount, uint32_t firstNode, float* boxes, const RefitScene& S)
{
  for (uint32_t i = nodeCount; i-- > firstNode;) refit_node(nodes, nodeCount, i, boxes, S);
}

} // namespace gi

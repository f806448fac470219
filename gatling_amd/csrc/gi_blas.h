// gi_blas.h -- the arithmetic of a BLAS refit on the two-level layout (gi_blas.hip k_blas_tris / k_blas_refit_level; gi_build.cpp updateVerticesTwoLevel,
// giCDebugSceneBlasCheck), shared by the host and the device kernels as gi_refit.h and gi_tlas.h are.  The points of a mesh moved: its
// BLAS keeps the topology buildTwoLevel gave it, its BlasTri records get the new object-space corners, and its nodes get new conservative boxes.  A leaf
// slot's box is what buildTwoLevel gives a face -- the minimum / maximum of the three object-space corners, padded by tlas_pad_box --, and the node
// arithmetic is refit_node's (gi_refit.h refit_node_with: the exponent rule, the outward rounding and the fix-up loops buildBvh8Boxes ran), so a refit of
// unchanged points writes the bytes the build wrote and the host reproduces the device's bytes.
#pragma once

#include <cmath>
#include <cstdint>
#include <cstring>

#include "gi_refit.h"
#include "gi_tlas.h"
#include "gi_types.h"

namespace gi {

// buildTwoLevel's box of one face with object-space corners p; false (and no box) where a corner is not a usable coordinate: the builder leaves such a face out
GI_REFIT_HD inline bool blas_face_box(const float p[3][3], float lo[3], float hi[3])
{
  bool ok = true;
  for (int a = 0; a < 3; a++) { lo[a] = 3.0e38f; hi[a] = -3.0e38f; }
  for (int k = 0; k < 3; k++)
    for (int a = 0; a < 3; a++) { lo[a] = refit_min(lo[a], p[k][a]); hi[a] = refit_max(hi[a], p[k][a]); ok = ok && refit_usable(p[k][a]); }
  if (!ok) return false;
  tlas_pad_box(lo, hi);
  return true;
}

// the leaf-box provider of a BLAS (gi_refit.h refit_node_with): a leaf slot names BlasTri records by absolute index
struct BlasLeaf {
  const BlasTri* tris; uint32_t triCount;
  GI_REFIT_HD bool operator()(uint32_t ti, float lo[3], float hi[3]) const
  {
    if (ti >= triCount) return false; // (cannot happen in a tree that validates)
    const BlasTri& t = tris[ti];
    const float p[3][3] = {{t.p0[0], t.p0[1], t.p0[2]}, {t.p1[0], t.p1[1], t.p1[2]}, {t.p2[0], t.p2[1], t.p2[2]}};
    return blas_face_box(p, lo, hi);
  }
};

// One BLAS node.  nodes / boxes: the whole BLAS node array and 8 floats per node of it (child and triangle indices are absolute)
GI_REFIT_HD inline void blas_refit_node(Node8* nodes, uint32_t nodeCount, uint32_t ni, float* boxes, const BlasTri* tris, uint32_t triCount)
{
  refit_node_with(nodes, nodeCount, ni, boxes, BlasLeaf{tris, triCount});
}

// One BLAS triangle: the record keeps its place and its `prim` (the order the builder left) and takes the corners of face shadeBase + prim from the shading
// records (TriShade::p: the FVertex positions, which packVertex copies bit for bit).  False: the face lies outside the shading records (cannot happen)
GI_REFIT_HD inline bool blas_tri_from_shade(BlasTri& t, const TriShade* triShade, uint32_t shadeCount, uint32_t shadeBase, uint32_t faceCount)
{
  const uint32_t prim = t.prim;
  if (prim >= faceCount || shadeBase > shadeCount || prim >= shadeCount - shadeBase) return false;
  const TriShade& q = triShade[shadeBase + prim];
  for (int a = 0; a < 3; a++) { t.p0[a] = q.p[0][a]; t.p1[a] = q.p[1][a]; t.p2[a] = q.p[2][a]; }
  return true;
}

// The host form of the BLAS refit: the nodes [firstNode, firstNode + count) of one BLAS, children before parents (buildBvh8Boxes places children behind their
// parent, so descending index order is a valid one).  `boxes`: 8 floats per node of the whole array.
inline void blasRefitHost(Node8* nodes, uint32_t nodeCount, uint32_t firstNode, uint32_t count, float* boxes, const BlasTri* tris, uint32_t triCount)
{
  if (firstNode > nodeCount || count > nodeCount - firstNode) return;
  for (uint32_t i = firstNode + count; i-- > firstNode;) blas_refit_node(nodes, nodeCount, i, boxes, tris, triCount);
}

// The conservative check of one BLAS, independent of the refit's own scratch: every occupied slot's DEQUANTISED box (the planes the traversal evaluates) must
// contain the padded box of every usable face below it; every usable face of [firstTri, firstTri + faceCount) must be named by exactly one leaf slot, an
// unusable one by none; children lie behind their parent and inside the BLAS.  Returns the number of violations.  `under`: scratch, 6 floats per node of the
// whole array.
inline uint32_t blasConservativeViolations(const Node8* nodes, uint32_t nodeCount, uint32_t firstNode, uint32_t count, const BlasTri* tris, uint32_t triCount,
    uint32_t firstTri, uint32_t faceCount, float* under, uint8_t* seen /* faceCount, zeroed */)
{
  uint32_t violations = 0;
  if (firstNode > nodeCount || count > nodeCount - firstNode || firstTri > triCount || faceCount > triCount - firstTri) return 1u;
  for (uint32_t ni = firstNode + count; ni-- > firstNode;) {
    const Node8& n = nodes[ni];
    float nlo[3] = {3.0e38f, 3.0e38f, 3.0e38f}, nhi[3] = {-3.0e38f, -3.0e38f, -3.0e38f};
    uint32_t rel = 0;
    for (int s = 0; s < 8; s++) {
      const uint32_t meta = n.meta[s];
      if (meta == 0u) { if ((n.imask >> s) & 1u) violations++; continue; }
      float lo[3] = {3.0e38f, 3.0e38f, 3.0e38f}, hi[3] = {-3.0e38f, -3.0e38f, -3.0e38f};
      if ((n.imask >> s) & 1u) {
        const uint32_t c = n.childBase + rel; rel++;
        if (c <= ni || c >= firstNode + count) { violations++; continue; }
        for (int a = 0; a < 3; a++) { lo[a] = under[6 * (size_t)c + a]; hi[a] = under[6 * (size_t)c + 3 + a]; }
      } else {
        const uint32_t unary = meta >> 5, off = meta & 31u, cnt = unary == 1u ? 1u : unary == 3u ? 2u : unary == 7u ? 3u : 0u;
        if (cnt == 0u || off + cnt > 24u) { violations++; continue; }
        for (uint32_t k = 0; k < cnt; k++) {
          const uint32_t ti = n.triBase + off + k;
          if (ti < firstTri || ti - firstTri >= faceCount) { violations++; continue; }
          if (seen[ti - firstTri]) violations++;
          seen[ti - firstTri] = 1;
          float tl[3], th[3];
          if (!BlasLeaf{tris, triCount}(ti, tl, th)) { violations++; continue; } // an unusable face below a leaf slot
          for (int a = 0; a < 3; a++) { lo[a] = tl[a] < lo[a] ? tl[a] : lo[a]; hi[a] = th[a] > hi[a] ? th[a] : hi[a]; }
        }
      }
      if (!(lo[0] <= hi[0])) continue; // nothing below
      for (int a = 0; a < 3; a++) {
        const uint32_t eb = (uint32_t)n.e[a] << 23; float scale; memcpy(&scale, &eb, 4);
        const float qlo = n.p[a] + (float)n.qlo[a][s] * scale, qhi = n.p[a] + (float)n.qhi[a][s] * scale;
        if (!(qlo <= lo[a]) || !(qhi >= hi[a])) violations++;
        nlo[a] = lo[a] < nlo[a] ? lo[a] : nlo[a]; nhi[a] = hi[a] > nhi[a] ? hi[a] : nhi[a];
      }
    }
    for (int a = 0; a < 3; a++) { under[6 * (size_t)ni + a] = nlo[a]; under[6 * (size_t)ni + 3 + a] = nhi[a]; }
  }
  for (uint32_t f = 0; f < faceCount; f++) {
    float tl[3], th[3];
    const bool usable = BlasLeaf{tris, triCount}(firstTri + f, tl, th);
    if (usable != (seen[f] != 0)) violations++;
  }
  return violations;
}

} // namespace gi

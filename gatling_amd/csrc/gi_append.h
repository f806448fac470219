// gi_append.h -- the per-item arithmetic of a mesh appended to a resident two-level scene without the flat tree (gi_append.hip k_append_shade_index /
// k_append_blas_tris / k_append_records; gi_build.cpp updateTopologyTwoLevel, giCDebugAppendRecords), shared by the host and the device
// kernels as gi_refit.h, gi_blas.h and gi_vispatch.h are.  An appended mesh brings nf faces and any number of instances: everything per face and per
// flattened triangle is made where it lives, from what the host sends per VERTEX, per FACE and per INSTANCE -- the mesh's FVertex records, its face indices,
// the builder's face order, its AOV face ids and its InstanceRecs.  Every form is spelled out once here and runs on both sides, so the device's bytes are the
// host's, and the host's are what flattenInstance, buildSceneTreeless, packTriShade, makeBlasTri and faceIdAovOf leave (giCDebugAppendRecordsHost holds that).
// Words are moved as integers but where flattenTriangle computes (refit_flatten: its operations in its order; the library is built without contraction).
#pragma once

#include <cstddef>
#include <cstdint>

#include "gi_refit.h"
#include "gi_types.h"

namespace gi {

// What k_append_records is given for one mesh: where its records go, what they name, and the sizes every index is checked against
struct AppendMesh {
  uint32_t triFirst, faceCount, instFirst, instCount; // flat records [triFirst, triFirst + instCount * faceCount), instances-major; InstanceRecs [instFirst, + instCount)
  uint32_t shadeBase, idBase, matFlags, pad;          // the mesh's first shading record, the scene-order id of its first triangle, TriRec::matFlags
  uint32_t triCount, instanceCount, shadeCount, flatCount; // records of the flat arrays (and the face-id table), InstanceRecs, shading records, words of the id table
};
static_assert(sizeof(TriRec) == 64 && offsetof(TriRec, e1) == 12 && offsetof(TriRec, origId) == 36 && offsetof(TriRec, vi) == 48 && offsetof(TriRec, prim) == 60,
    "append_record_piece: 16-byte pieces of a TriRec");
static_assert(sizeof(TriShade) == 160 && offsetof(TriShade, vi) == 144 && offsetof(TriShade, pad) == 156, "append_shade_index: the tenth piece of a TriShade");
static_assert(sizeof(BlasTri) == 64 && offsetof(BlasTri, p1) == 12 && offsetof(BlasTri, p2) == 24 && offsetof(BlasTri, prim) == 36, "append_blas_tri: 16-byte pieces of a BlasTri");

GI_REFIT_HD inline uint32_t append_bits(float x) { uint32_t u; __builtin_memcpy(&u, &x, 4); return u; }

// The tenth 16-byte piece of a face's shading record: TriShade::vi = vertexOffset + the face's indices, pad as packTriShade leaves it (0).  k_gather_shade
// (gi_refit.h refit_gather_shade) fills the other nine pieces from the vertex records these name
GI_REFIT_HD inline void append_shade_index(const uint32_t face[3], uint32_t vertexOffset, uint32_t out[4])
{
  out[0] = vertexOffset + face[0]; out[1] = vertexOffset + face[1]; out[2] = vertexOffset + face[2]; out[3] = 0u;
}

// The BLAS record of face `prim`, whole: the corners of its shading record (TriShade::p: the FVertex positions, which packVertex copies bit for bit), prim,
// six words of zero -- bytewise makeBlasTri's.  16 words
GI_REFIT_HD inline void append_blas_tri(const TriShade& q, uint32_t prim, uint32_t out[16])
{
  for (int k = 0; k < 3; k++) for (int a = 0; a < 3; a++) out[3 * k + a] = append_bits(q.p[k][a]);
  out[9] = prim;
  for (int w = 10; w < 16; w++) out[w] = 0u;
}

// Item `item` of a mesh's flat records, instances-major: instance-in-mesh item / faceCount, face item % faceCount
GI_REFIT_HD inline void append_item(const AppendMesh& M, uint32_t item, uint32_t& instInMesh, uint32_t& prim) { instInMesh = item / M.faceCount; prim = item % M.faceCount; }
// ... the scene-order id of its record (flattenInstance: an instance's triangles are numbered in face order from its base)
GI_REFIT_HD inline uint32_t append_orig_id(const AppendMesh& M, uint32_t instInMesh, uint32_t prim) { return M.idBase + instInMesh * M.faceCount + prim; }
// ... and whether everything it reads and writes lies inside its array (false cannot happen: the host asks appendMeshRangesOk first)
GI_REFIT_HD inline bool append_item_ok(const AppendMesh& M, uint32_t item)
{
  if (M.faceCount == 0u || item / M.faceCount >= M.instCount) return false;
  const uint32_t ii = item / M.faceCount, prim = item % M.faceCount;
  return M.triFirst <= M.triCount && item < M.triCount - M.triFirst && M.instFirst <= M.instanceCount && ii < M.instanceCount - M.instFirst &&
      M.shadeBase <= M.shadeCount && prim < M.shadeCount - M.shadeBase && append_orig_id(M, ii, prim) < M.flatCount;
}

// 16-byte piece `piece` (0..3) of the 64-byte TriRec of (instance-in-mesh ii, face prim): v0 / e1 / e2 by refit_flatten over the face's object-space corners
// (q.p) and the instance's o2w; origId; the instance's index; matFlags; vi as buildSceneTreeless leaves it (vi[0] names the shading record, vi[1] / vi[2] the
// absolute vertex indices the shading record holds); prim.  Pieces 0 and 1 and the first word of 2 are the nine floats
GI_REFIT_HD inline void append_record_piece(const AppendMesh& M, uint32_t ii, uint32_t prim, const float* o2w, const TriShade& q, uint32_t piece, uint32_t out[4])
{
  if (piece == 3u) { out[0] = M.shadeBase + prim; out[1] = q.vi[1]; out[2] = q.vi[2]; out[3] = prim; return; }
  float v0[3], e1[3], e2[3];
  refit_flatten(o2w, q.p, v0, e1, e2);
  if (piece == 0u) { out[0] = append_bits(v0[0]); out[1] = append_bits(v0[1]); out[2] = append_bits(v0[2]); out[3] = append_bits(e1[0]); }
  else if (piece == 1u) { out[0] = append_bits(e1[1]); out[1] = append_bits(e1[2]); out[2] = append_bits(e2[0]); out[3] = append_bits(e2[1]); }
  else { out[0] = append_bits(e2[2]); out[1] = append_orig_id(M, ii, prim); out[2] = M.instFirst + ii; out[3] = M.matFlags; }
}

// the ranges of one mesh against the arrays' sizes, and an item count (x 4 pieces) that fits a launch: what the host asks before it launches anything
inline bool appendMeshRangesOk(const AppendMesh& M)
{
  const uint64_t items = (uint64_t)M.faceCount * M.instCount;
  return M.faceCount != 0u && M.instCount != 0u && items < (1ull << 28) && M.triFirst <= M.triCount && items <= M.triCount - M.triFirst &&
      M.instFirst <= M.instanceCount && M.instCount <= M.instanceCount - M.instFirst && M.shadeBase <= M.shadeCount && M.faceCount <= M.shadeCount - M.shadeBase &&
      (uint64_t)M.idBase + items <= M.flatCount;
}

// The host forms of the three kernels, item by item through the functions above.  appendRecordsHost: items [first, last) of the mesh's flat records -- the
// caller may split the range over threads (one writer per word)
inline void appendShadeIndexHost(TriShade* triShade, uint32_t shadeCount, uint32_t shadeBase, const uint32_t* faces3, uint32_t faceCount, uint32_t vertexOffset)
{
  if (shadeBase > shadeCount || faceCount > shadeCount - shadeBase) return;
  for (uint32_t f = 0; f < faceCount; f++) { uint32_t w[4]; append_shade_index(faces3 + 3u * (size_t)f, vertexOffset, w); __builtin_memcpy(triShade[shadeBase + f].vi, w, 16); }
}
inline void appendBlasTrisHost(BlasTri* blasTris, uint32_t blasTriCount, uint32_t first, const uint32_t* order, uint32_t faceCount, const TriShade* triShade,
    uint32_t shadeCount, uint32_t shadeBase)
{
  if (first > blasTriCount || faceCount > blasTriCount - first || shadeBase > shadeCount || faceCount > shadeCount - shadeBase) return;
  for (uint32_t i = 0; i < faceCount; i++) {
    const uint32_t prim = order[i];
    if (prim >= faceCount) continue; // (cannot happen: the builder's order is a permutation of the faces)
    uint32_t w[16]; append_blas_tri(triShade[shadeBase + prim], prim, w); __builtin_memcpy(&blasTris[first + i], w, 64);
  }
}
inline void appendRecordsHost(const AppendMesh& M, uint32_t first, uint32_t last, TriRec* tris, int32_t* triFaceId, uint32_t* flatOfOrig, const InstanceRec* instances,
    const TriShade* triShade, const int32_t* faceIdOfFace)
{
  for (uint32_t item = first; item < last; item++) {
    if (!append_item_ok(M, item)) continue;
    uint32_t ii, prim; append_item(M, item, ii, prim);
    const TriShade& q = triShade[M.shadeBase + prim];
    const float* o2w = instances[M.instFirst + ii].o2w;
    for (uint32_t piece = 0; piece < 4u; piece++) {
      uint32_t w[4]; append_record_piece(M, ii, prim, o2w, q, piece, w);
      __builtin_memcpy(reinterpret_cast<char*>(&tris[M.triFirst + item]) + 16u * piece, w, 16);
    }
    if (triFaceId) triFaceId[M.triFirst + item] = faceIdOfFace[prim];
    if (flatOfOrig) flatOfOrig[append_orig_id(M, ii, prim)] = M.triFirst + item;
  }
}

} // namespace gi

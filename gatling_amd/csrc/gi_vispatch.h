// gi_vispatch.h -- the per-record and per-instance arithmetic of a visibility edit applied in place (gi_build.cpp updateVisibility and
// updateVisibilityTwoLevel; gi_patch.hip k_patch_visibility, k_patch_visibility2 and k_patch_inst_trav), shared by the host and the
// device kernels as gi_refit.h and gi_tlas.h are.  The two-level forms are spelled out once here and run on both sides, so the device's words are bytewise
// the host's (giCDebugPatchVisibilityTwoLevel holds that).
#pragma once

#include <cstddef>
#include <cstdint>

#include "gi_refit.h"
#include "gi_types.h"

namespace gi {

// One VisPatch per flattened instance: the change of its triangles' scene-order ids, and whether its records are left alone, made unhittable (both edges
// zeroed) or given their edges back (recomputed from the mesh triangle's shading record and the instance transform with the scene build's operations in its
// order).  VIS_HIDDEN_AFTER (the two-level table alone; k_patch_visibility never sees it): the instance is hidden once the edit is applied -- VIS_KEEP does
// not say whether an untouched instance is visible, and a hidden instance's records must not write the id table.
struct VisPatch { int32_t idDelta; uint32_t action; };
constexpr uint32_t VIS_KEEP = 0u, VIS_HIDE = 1u, VIS_SHOW = 2u, VIS_ACTION_MASK = 3u, VIS_HIDDEN_AFTER = 4u;

// The inverted box buildTwoLevel gives an instance the TLAS must not name: the box builder leaves it out (bvh8.h "Inactive items").  boxes: 6 floats per
// instance; hiddenOfInstance[i] != 0: instance i belongs to a hidden mesh
inline void tlasMaskHiddenBoxes(float* boxes, const uint8_t* hiddenOfInstance, size_t instanceCount)
{
  for (size_t i = 0; i < instanceCount; i++)
    if (hiddenOfInstance[i]) for (int a = 0; a < 3; a++) { boxes[6 * i + a] = 3.0e38f; boxes[6 * i + 3 + a] = -3.0e38f; }
}

// Record i of the flat triangles of a two-level scene under the table `patch` (k_patch_visibility2, one thread per record):
//   the id moves by idDelta; a hide zeroes both edges, a show makes them again (refit_flatten: flattenTriangle's operations in its order; v0 is never touched);
//   a record whose instance is visible AFTER the edit and whose id or visibility changed names itself in flatOfOrig at its NEW id.  Records of hidden
//   instances never write the table: their stale ids overlap the ids the meshes behind them just received.  The visible ids are a permutation of
//   [0, visibleTris): one writer per word, in any order.  A visible record with an unchanged id was named there before and still is (the induction every edit
//   keeps: flatOfOrig[origId] == i for every visible record), so it stores nothing.
// Only words that change are stored.  An id outside the table (cannot happen: the table has one word per resident triangle) is not written.
GI_REFIT_HD inline void vis2_patch_record(TriRec* tris, uint32_t i, const InstanceRec* instances, uint32_t instanceCount, const VisPatch* patch,
    const TriShade* triShade, uint32_t shadeCount, uint32_t* flatOfOrig, uint32_t flatCount)
{
  TriRec& t = tris[i];
  const uint32_t inst = t.instance;
  if (inst >= instanceCount) return; // (cannot happen: the build numbers instances densely)
  const VisPatch vp = patch[inst];
  const uint32_t action = vp.action & VIS_ACTION_MASK;
  uint32_t id = t.origId;
  if (vp.idDelta != 0) { id += (uint32_t)vp.idDelta; t.origId = id; }
  if (action == VIS_HIDE) {
    for (int a = 0; a < 3; a++) { t.e1[a] = 0.0f; t.e2[a] = 0.0f; }
  } else if (action == VIS_SHOW) {
    const uint32_t rec = t.vi[0];
    if (rec < shadeCount) { // (cannot fail: scenes beyond LDS name their shading record there)
      float v0[3], e1[3], e2[3];
      refit_flatten(instances[inst].o2w, triShade[rec].p, v0, e1, e2);
      for (int a = 0; a < 3; a++) { t.e1[a] = e1[a]; t.e2[a] = e2[a]; }
    }
  }
  if (!(vp.action & VIS_HIDDEN_AFTER) && (vp.idDelta != 0 || action == VIS_SHOW) && id < flatCount) flatOfOrig[id] = i;
}

// InstTrav::triBase of instance i (k_patch_inst_trav, one thread per instance): the scene-order id of its first triangle moves with its records' ids.  One
// dword of the 128-byte record, where it changes; the matrices, blasRoot, matFlags and slack are not touched.
GI_REFIT_HD inline void vis2_patch_inst_trav(InstTrav* instTrav, uint32_t i, const VisPatch* patch)
{
  const int32_t delta = patch[i].idDelta;
  if (delta != 0) instTrav[i].triBase += (uint32_t)delta;
}

// The host forms of the two kernels
inline void patchVisibilityTwoLevelHost(TriRec* tris, uint32_t triCount, const InstanceRec* instances, uint32_t instanceCount, const VisPatch* patch,
    const TriShade* triShade, uint32_t shadeCount, uint32_t* flatOfOrig, uint32_t flatCount)
{ for (uint32_t i = 0; i < triCount; i++) vis2_patch_record(tris, i, instances, instanceCount, patch, triShade, shadeCount, flatOfOrig, flatCount); }
inline void patchInstTravHost(InstTrav* instTrav, uint32_t instanceCount, const VisPatch* patch)
{ for (uint32_t i = 0; i < instanceCount; i++) vis2_patch_inst_trav(instTrav, i, patch); }

// What giCDebugSceneFlatIdCheck counts over arrays as they are resident: records of visible instances whose ids are not a permutation of [0, visibleTris),
// that flatOfOrig does not name at their id, or whose id is not their instance's triBase + prim; records of hidden instances with an edge that is not zero.
// hiddenOfInstance: one byte per instance.  `seen`: scratch, one byte per resident triangle.  visibleTris receives the count of records of visible instances
inline uint32_t flatIdViolations(const TriRec* tris, uint32_t triCount, const uint32_t* flatOfOrig, uint32_t flatCount, const InstTrav* instTrav,
    const uint8_t* hiddenOfInstance, uint32_t instanceCount, uint8_t* seen, uint32_t& visibleTris)
{
  uint32_t bad = 0; visibleTris = 0;
  for (uint32_t i = 0; i < triCount; i++) { seen[i] = 0; if (tris[i].instance < instanceCount && !hiddenOfInstance[tris[i].instance]) visibleTris++; }
  for (uint32_t i = 0; i < triCount; i++) {
    const TriRec& t = tris[i];
    if (t.instance >= instanceCount) { bad++; continue; }
    if (hiddenOfInstance[t.instance]) {
      for (int a = 0; a < 3; a++) if (t.e1[a] != 0.0f || t.e2[a] != 0.0f) { bad++; break; }
      continue;
    }
    if (t.origId >= visibleTris || seen[t.origId]) bad++; else seen[t.origId] = 1;
    if (t.origId >= flatCount || flatOfOrig[t.origId] != i) bad++;
    if (instTrav[t.instance].triBase + t.prim != t.origId) bad++;
  }
  return bad;
}

} // namespace gi

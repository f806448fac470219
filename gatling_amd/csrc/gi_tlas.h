// gi_tlas.h -- the per-instance arithmetic of the two-level layout (gi_build.cpp buildTwoLevel, updateTransformsTwoLevel; gi_tlas.hip k_inst_bounds /
// k_inst_finish), shared by the host and the device kernels: the world box of an instance is the minimum / maximum over its mesh's
// triangles under the instance's transform, padded; its InstTrav record is the instance's matrices beside four constants of its mesh.  Every operation is
// spelled out once here and runs in this order on both sides, without contraction, so the device's padded boxes are bytewise the host loop's
// (giCDebugInstanceBounds holds that) and a TLAS built over them is a fresh build's (giCDebugSceneTlasCheck).
#pragma once

#include <cmath>
#include <cstdint>

#include "gi_refit.h"
#include "gi_types.h"

namespace gi {

// world = o2w * (p, 1): rows of the 3x4 affine (gi_build.cpp xformPoint's operations in its order)
GI_REFIT_HD inline void tlas_xform_point(const float a[12], const float p[3], float out[3])
{
  out[0] = ((a[0] * p[0] + a[1] * p[1]) + a[2] * p[2]) + a[3];
  out[1] = ((a[4] * p[0] + a[5] * p[1]) + a[6] * p[2]) + a[7];
  out[2] = ((a[8] * p[0] + a[9] * p[1]) + a[10] * p[2]) + a[11];
}

// as bvh8.cpp pads triangle boxes: 2^-20 relative, covers the rounding of the exact test's inputs.  The pad is positive, so a box side that is a zero
// leaves here with the same bits whatever its sign was: -0 - pad and +0 - pad are the same float, and so are the magnitudes.
GI_REFIT_HD inline void tlas_pad_box(float* lo, float* hi)
{
  for (int a = 0; a < 3; a++) {
    const float mag = refit_max(fabsf(lo[a]), fabsf(hi[a])) + (hi[a] - lo[a]);
    const float pad = mag * 9.5367431640625e-7f + 1.0e-30f;
    lo[a] -= pad; hi[a] += pad;
  }
}

// What makes an instance unusable for the two-level walk or for an update in place (status word, 0 = usable):
//   OBJECT  a corner of a mesh triangle is not a usable coordinate in object space (the BLAS builder leaves the face out; the face stays out of the box)
//   WORLD   ... in world space under this transform (buildTwoLevel's rule: the flat tree holds the triangle as inactive, the walk here would reach it)
//   TRIBOX  the builders' own rule on the builders' own operands refuses the flattened record (gi_refit.h refit_tri_box over refit_flatten's v0 / e1 / e2:
//           what updateVertices applies) -- a refit of the flat tree would meet an inactive triangle
//   RANGE   the job named triangles outside the BLAS array (cannot happen: set by the kernels' guards only)
constexpr uint32_t TLAS_STATUS_OBJECT = 1u, TLAS_STATUS_WORLD = 2u, TLAS_STATUS_TRIBOX = 4u, TLAS_STATUS_RANGE = 8u;

struct TlasBounds { float lo[3], hi[3]; uint32_t status; };
GI_REFIT_HD inline void tlas_bounds_init(TlasBounds& b)
{
  for (int a = 0; a < 3; a++) { b.lo[a] = 3.0e38f; b.hi[a] = -3.0e38f; }
  b.status = 0u;
}
// Minima and maxima pick by comparison (gi_refit.h refit_min / refit_max): a NaN operand is never picked and the accumulator never becomes one, so the
// result is the minimum / maximum over the comparable values in any order -- up to the sign of a zero, which tlas_pad_box removes.
GI_REFIT_HD inline void tlas_bounds_merge(TlasBounds& b, const float lo[3], const float hi[3], uint32_t status)
{
  for (int a = 0; a < 3; a++) { b.lo[a] = refit_min(b.lo[a], lo[a]); b.hi[a] = refit_max(b.hi[a], hi[a]); }
  b.status |= status;
}
// one mesh triangle with object-space corners p under o2w.  builderRule: TRIBOX is evaluated (an update in place; the scene build reads OBJECT and WORLD
// alone -- its flat tree holds such a triangle as inactive, which is the builder's business there)
GI_REFIT_HD inline void tlas_bounds_add_tri(const float* o2w, const float p[3][3], TlasBounds& b, bool builderRule)
{
  float q[3][3]; bool objectOk = true, worldOk = true;
  for (int k = 0; k < 3; k++) {
    tlas_xform_point(o2w, p[k], q[k]);
    for (int a = 0; a < 3; a++) { objectOk = objectOk && refit_usable(p[k][a]); worldOk = worldOk && refit_usable(q[k][a]); }
  }
  if (!objectOk) { b.status |= TLAS_STATUS_OBJECT; return; }
  if (!worldOk) b.status |= TLAS_STATUS_WORLD;
  if (builderRule) {
    float v0[3], e1[3], e2[3], tl[3], th[3];
    for (int a = 0; a < 3; a++) { v0[a] = q[0][a]; e1[a] = q[1][a] - q[0][a]; e2[a] = q[2][a] - q[0][a]; } // (refit_flatten's, from the same corners)
    if (!refit_tri_box(v0, e1, e2, tl, th)) b.status |= TLAS_STATUS_TRIBOX;
  }
  for (int k = 0; k < 3; k++) for (int a = 0; a < 3; a++) { b.lo[a] = refit_min(b.lo[a], q[k][a]); b.hi[a] = refit_max(b.hi[a], q[k][a]); }
}

// The host form of k_inst_bounds + k_inst_finish: the padded world box and the status of one instance over its mesh's BLAS triangles
inline uint32_t tlasInstanceBoundsHost(const float* o2w, const BlasTri* tris, size_t count, float box[6])
{
  TlasBounds b; tlas_bounds_init(b);
  for (size_t i = 0; i < count; i++) {
    const float p[3][3] = {{tris[i].p0[0], tris[i].p0[1], tris[i].p0[2]}, {tris[i].p1[0], tris[i].p1[1], tris[i].p1[2]}, {tris[i].p2[0], tris[i].p2[1], tris[i].p2[2]}};
    tlas_bounds_add_tri(o2w, p, b, true);
  }
  tlas_pad_box(b.lo, b.hi);
  for (int a = 0; a < 3; a++) { box[a] = b.lo[a]; box[3 + a] = b.hi[a]; }
  return b.status;
}

// An instance's InstTrav: its matrices beside the constants of its mesh, none of which a transform changes -- the BLAS root, the scene-order id of the
// instance's first triangle, the mesh's TriRec::matFlags, the object-space magnitude `slack`
inline InstTrav tlasMakeInstTrav(const InstanceRec& ir, uint32_t blasRoot, uint32_t triBase, uint32_t matFlags, float slack)
{
  InstTrav tv{};
  for (int i = 0; i < 12; i++) tv.o2w[i] = ir.o2w[i];
  for (int i = 0; i < 9; i++) tv.w2o[i] = ir.w2o[i];
  tv.blasRoot = blasRoot; tv.triBase = triBase; tv.matFlags = matFlags; tv.slack = slack;
  return tv;
}

// The bounds of a two-level scene without the flat tree (GI_C_SCENE_OPTION_TLAS_ONLY; gi_build.cpp): the union of the padded world boxes of the instances
// the TLAS names -- not hidden (`hidden` may be null: none is), not inverted (the box an unusable instance keeps; the builder leaves it out) -- run through the
// pad the flat root's bounds get (gi_build.cpp setSceneBounds: 1e-5 of magnitude and extent, plus 1e-30).  Every box contains every world-space corner of
// its instance, so k_raygen's bounds retire stays conservative.  valid = false, as there: no box in the union, or a side that is not finite -- a box with
// such a side makes the whole answer invalid (a built scene holds none: buildTwoLevel declines for them), never a smaller union.
inline void tlas_scene_bounds(const float* instBoxes, const uint8_t* hidden, size_t n, float out[6], bool& valid)
{
  float lo[3] = {3.0e38f, 3.0e38f, 3.0e38f}, hi[3] = {-3.0e38f, -3.0e38f, -3.0e38f};
  valid = false;
  for (int a = 0; a < 6; a++) out[a] = 0.0f;
  bool any = false;
  for (size_t i = 0; i < n; i++) {
    if (hidden && hidden[i]) continue;
    const float* b = instBoxes + 6u * i;
    bool finite = true, inverted = false;
    for (int a = 0; a < 3; a++) { finite = finite && std::isfinite(b[a]) && std::isfinite(b[3 + a]); inverted = inverted || !(b[a] <= b[3 + a]); }
    if (!finite) return;
    if (inverted) continue;
    for (int a = 0; a < 3; a++) { lo[a] = refit_min(lo[a], b[a]); hi[a] = refit_max(hi[a], b[3 + a]); }
    any = true;
  }
  if (!any) return;
  for (int a = 0; a < 3; a++) {
    const float pad = (std::fabs(lo[a]) + std::fabs(hi[a]) + (hi[a] - lo[a])) * 1.0e-5f + 1.0e-30f;
    out[a] = lo[a] - pad; out[3 + a] = hi[a] + pad;
    if (!std::isfinite(out[a]) || !std::isfinite(out[3 + a])) return;
  }
  valid = true;
}

} // namespace gi

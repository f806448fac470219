// gi_blas_build_host.cpp -- the host form of the device BLAS builder (gi_blas_build.h): the face boxes by blas_face_box as k_blas_face_boxes makes them, then
// the host form of the shared box-tree stages (gi_tlas_build_host.cpp buildBoxTreeHost) under the BLAS limits, so that the two produce the same bytes
// (giCDebugBuildBlas).
#include <algorithm>

#include "gi_blas.h"
#include "gi_blas_build.h"

namespace gi {

int buildBlasHost(const GiCVertex* vertices, size_t vertexCount, const GiCFace* faces, size_t nf, uint32_t budget, uint32_t radius, Bvh8& out,
    std::vector<uint32_t>& order, float mlo[3], float mhi[3], BlasBuildInfo& info)
{
  info = BlasBuildInfo{}; out = Bvh8{}; order.clear();
  for (int a = 0; a < 3; a++) { mlo[a] = 3.0e38f; mhi[a] = -3.0e38f; }
  if (nf > kBlasMaxItems) { info.error = "more items than the builder is sized for"; return TLAS_BUILD_ERROR; }
  for (size_t f = 0; f < nf; f++)
    for (int k = 0; k < 3; k++) if (faces[f].v_i[k] >= vertexCount) { info.error = "a face index outside the vertices"; return TLAS_BUILD_ERROR; }
  std::vector<float> boxes(6 * nf);
  for (size_t f = 0; f < nf; f++) {
    float p[3][3], lo[3], hi[3];
    for (int k = 0; k < 3; k++) for (int a = 0; a < 3; a++) p[k][a] = vertices[faces[f].v_i[k]].pos[a];
    const bool ok = blas_face_box(p, lo, hi);
    if (!ok) for (int a = 0; a < 3; a++) { lo[a] = 3.0e38f; hi[a] = -3.0e38f; }
    for (int a = 0; a < 3; a++) { boxes[6 * f + a] = lo[a]; boxes[6 * f + 3 + a] = hi[a]; }
    if (ok) for (int a = 0; a < 3; a++) { mlo[a] = refit_min(mlo[a], lo[a]); mhi[a] = refit_max(mhi[a], hi[a]); }
  }
  const int rc = buildBoxTreeHost(boxes.data(), nf, budget, radius, kBlasBuildLimits, out.nodes, order, info);
  if (rc != TLAS_BUILD_OK) { out = Bvh8{}; order.clear(); return rc; }
  out.maxDepth = info.maxDepth; out.activeTris = info.active;
  out.levelStart.assign(info.levelStart, info.levelStart + info.maxDepth + 1u);
  return TLAS_BUILD_OK;
}

} // namespace gi

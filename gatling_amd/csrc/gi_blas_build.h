// gi_blas_build.h -- the BLAS of one mesh of a two-level scene built on the device (gi_blas_build.hip; GI_C_SCENE_OPTION_BLAS_DEVICE_BUILD, DESIGN.md section 6
// "BLAS build on the device") and the host form of the same builder (gi_blas_build_host.cpp), which the device's bytes are held to.
//
// Input: a mesh's vertices and faces as giCCreateMesh took them.  Output: buildMeshBlas's (gi_build.cpp) -- `out.nodes` breadth-first with children behind their
// parent, `out.levelStart` / `out.maxDepth`, `order`: the active faces in leaf order (what triBase + offset names), the inactive ones behind in input order,
// mlo / mhi: the union of the usable faces' padded boxes.  A face's box is blas_face_box's (gi_blas.h): a face with an unusable corner keeps the inverted box
// and is left out.
//
// Stages: the face boxes are made on the device from the uploaded positions and indices, in the pass that makes every workgroup's centroid bounds; from there
// the build is the TLAS builder's (gi_tlas_build.h buildBoxTreeDevice: Morton sort, PLOC, the depth-bounded cost-optimal collapse, level-wise emission), run
// under the limits below.  The emission quantises a node as refit_node_with (gi_refit.h) does, so a BLAS refit over unchanged points writes the build's bytes.
//
// Workspace: the scene's TlasBuildWorkspace slab.  Per face (budget B, L = B + 1 layers of the DP): 88 L bytes of DP records + 356 bytes of the builder's other
// arrays + 12 bytes of indices -- 1 512 bytes at B = 12, 1.59 GB at 2^20 faces --; per vertex 12 bytes; rocprim's sort and scan scratch beside them (DESIGN.md
// section 6 lists the arrays).
#pragma once

#include "bvh8.h"
#include "gi_c.h"
#include "gi_tlas_build.h"

namespace gi {

constexpr uint32_t kBlasMaxBudget = 12;       // 15 - 2 * tlasDepth at tlasDepth 1 is 13; twelve levels of 8-wide nodes hold any mesh the cap admits
constexpr uint32_t kBlasMaxItems = 1u << 22;  // what the indices and the packed scan words of the stages were reviewed for; blas_device_max lies below it
constexpr BoxBuildLimits kBlasBuildLimits{kBlasMaxItems, kBlasMaxBudget};

using BlasBuildInfo = TlasBuildInfo;

// B = min(kBlasMaxBudget, 15 - 2 T): the deepest BLAS the stack rule 2 * tlasDepth + blasDepth + 1 <= 16 admits under a TLAS of depth T
inline uint32_t blasDepthBudget(uint32_t tlasDepth) { return 2u * tlasDepth >= 15u ? 0u : (15u - 2u * tlasDepth < kBlasMaxBudget ? 15u - 2u * tlasDepth : kBlasMaxBudget); }

// the host form: one thread, plain C++ over gi_bvh_stages.h.  TLAS_BUILD_ERROR for a face index outside the vertices
int buildBlasHost(const GiCVertex* vertices, size_t vertexCount, const GiCFace* faces, size_t nf, uint32_t budget, uint32_t radius, Bvh8& out,
    std::vector<uint32_t>& order, float mlo[3], float mhi[3], BlasBuildInfo& info);

// The device builder on the current device.  The nodes and the order are read back (the caller rebases them and sends them to every device of the scene as it
// sends a host-built BLAS).  The bytes are buildBlasHost's.  A face index outside the vertices never reaches a kernel: TLAS_BUILD_ERROR.
int buildBlasDevice(TlasBuildWorkspace& ws, hipStream_t st, const GiCVertex* vertices, size_t vertexCount, const GiCFace* faces, size_t nf, uint32_t budget,
    uint32_t radius, Bvh8& out, std::vector<uint32_t>& order, float mlo[3], float mhi[3], BlasBuildInfo& info);

} // namespace gi

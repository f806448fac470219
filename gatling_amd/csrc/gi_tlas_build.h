// gi_tlas_build.h -- the TLAS of an edited two-level scene built on the device (gi_tlas_build.hip; GI_C_SCENE_OPTION_TLAS_DEVICE_BUILD, DESIGN.md section 6
// "TLAS build on the device") and the host form of the same builder (gi_tlas_build_host.cpp), which the device's bytes are held to.
//
// Input: n padded instance boxes (6 floats each; hidden, retired and free-slot instances already carry the inverted box of gi_vispatch.h
// tlasMaskHiddenBoxes).  Output: buildBvh8Boxes's contract -- Node8 nodes breadth-first, items[]: the active items in leaf order (what triBase + offset
// names), the inactive ones (bvh8.h "Inactive items": an inverted box, a non-finite side, a magnitude beyond 1e18) behind in input order.
//
// Stages: centroid bounds -> 63-bit Morton codes -> stable sort -> PLOC (radius positions either side, the (distance, pair hash, position) tie-break) ->
// the DEPTH-BOUNDED cost-optimal collapse (gi_bvh_stages.h bvh_dp_internal_bounded: cPrim 0.5, at most 3 items per leaf slot) -> level-wise emission.  The
// tree has at most `budget` levels by construction; a root that does not fit answers TLAS_BUILD_TOO_DEEP.
//
// The stages are a box-tree builder of their own (buildBoxTreeDevice / buildBoxTreeHost below): where the boxes come from, the item limit and the largest
// budget are parameters of a build.  The TLAS builder is that builder over uploaded boxes under kTlasBuildLimits; the BLAS builder of gi_blas_build.h is the
// same one over face boxes made on the device, under limits of its own.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <vector>

#include "gi_types.h"

namespace gi {

enum TlasBuildStatus : int { TLAS_BUILD_OK = 0, TLAS_BUILD_OUT_OF_MEMORY = 1, TLAS_BUILD_TOO_DEEP = 2, TLAS_BUILD_ERROR = -1 };

constexpr uint32_t kTlasMaxBudget = 7;        // floor((15 - blasDepth) / 2) at blasDepth 1: the 16-entry stack of the two-level walk
constexpr uint32_t kTlasMaxItems = 1u << 17;  // (the stack rule keeps a TLAS to roughly 1e5 instances)
constexpr uint32_t kTlasTailClusters = 2048;  // at or below this many clusters one workgroup finishes PLOC in LDS (28 bytes per cluster: 56 KiB)
constexpr uint32_t kTlasPassBatch = 8;        // multi-block PLOC passes launched between two reads of the cluster count
constexpr uint32_t kTlasMaxBatches = 16;      // batches before the build gives up with TLAS_BUILD_ERROR (128 passes; a pass merges 30 - 40 % of the clusters)
// Host waits of one device build, whatever n: one per batch of multi-block passes (none when n <= kTlasTailClusters), one for the status behind the
// emission, one for the nodes and items.
constexpr uint32_t kTlasMaxHostWaits = kTlasMaxBatches + 2u;

// What a build is sized for: the most items it takes and the deepest budget it honours.  The TLAS of an edit has the two constants above; the BLAS of a mesh
// (gi_blas_build.h) runs the same stages under its own.
struct BoxBuildLimits { uint32_t maxItems, maxBudget; };
constexpr BoxBuildLimits kTlasBuildLimits{kTlasMaxItems, kTlasMaxBudget};
constexpr uint32_t kBoxBuildMaxLevels = 16;   // levels any build of these stages may emit (the 16-entry traversal stack bounds every budget)

struct TlasBuildInfo {
  uint32_t nodeCount = 0, maxDepth = 0, active = 0, passes = 0, hostWaits = 0;
  uint32_t levelStart[kBoxBuildMaxLevels + 1] = {}; // first node of every breadth-first level, then the node count: maxDepth + 1 entries (Bvh8::levelStart)
  float ms[4] = {0, 0, 0, 0}; // device: upload + boxes + sort, PLOC (+ the DP it fills), emission, read-back
  const char* error = "";
};

// D = floor((15 - blasDepth) / 2): the deepest TLAS the stack rule 2 * tlasDepth + blasDepth + 1 <= 16 admits
inline uint32_t tlasDepthBudget(uint32_t blasDepth) { return blasDepth >= 15u ? 0u : (15u - blasDepth) / 2u; }

// the host form: plain C++ over gi_bvh_stages.h, one thread
int buildBoxTreeHost(const float* boxes6, size_t n, uint32_t budget, uint32_t radius, const BoxBuildLimits& limits, std::vector<Node8>& nodes,
    std::vector<uint32_t>& items, TlasBuildInfo& info);
int buildTlasHost(const float* boxes6, size_t n, uint32_t budget, uint32_t radius, std::vector<Node8>& nodes, std::vector<uint32_t>& items, TlasBuildInfo& info);

// What a scene keeps on its primary device for these builds: one slab, carved anew by every build, that grows geometrically and is released with the scene
// -- a steady-state build allocates nothing.
struct TlasBuildWorkspace {
  void* mem = nullptr; size_t bytes = 0; uint64_t allocations = 0;
  hipEvent_t ev[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
  void release();
};

// The device builder on the current device, `boxes6` on the host.  The nodes and items are read back (the caller sends them to every device of the scene as
// it sends a host-built TLAS).  The bytes are buildTlasHost's.
int buildTlasDevice(TlasBuildWorkspace& ws, hipStream_t st, const float* boxes6, uint32_t n, uint32_t budget, uint32_t radius, std::vector<Node8>& nodes,
    std::vector<uint32_t>& items, TlasBuildInfo& info);

// The stages behind buildTlasDevice for any source of boxes.  `fill` enqueues on the stream what leaves the n padded boxes (6 floats each; an item the tree
// leaves out: the inverted box), their float4 pairs and every workgroup's centroid bounds and active count (gi_bvh_stages.h stage_item_box,
// stage_block_bounds; one workgroup per kStageBlock items) in the places BoxStage names.  `extraBytes` of the slab are the source's own (BoxStage::extra,
// 256-byte aligned): a source allocates nothing.  Behind the emission `backBytes` bytes at extra + backOffset are read back to backHost with the nodes and items.
struct BoxStage { float* boxes6; float4 *lo4, *hi4, *blockLo, *blockHi; uint32_t* blockAlive; void* extra; };
struct BoxSource {
  hipError_t (*fill)(void* ctx, const BoxStage& stage, uint32_t n, hipStream_t st) = nullptr; void* ctx = nullptr;
  size_t extraBytes = 0, backOffset = 0, backBytes = 0; void* backHost = nullptr;
};
int buildBoxTreeDevice(TlasBuildWorkspace& ws, hipStream_t st, const BoxSource& source, uint32_t n, uint32_t budget, uint32_t radius, const BoxBuildLimits& limits,
    std::vector<Node8>& nodes, std::vector<uint32_t>& items, TlasBuildInfo& info);

} // namespace gi

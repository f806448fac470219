// gi_bvh_build.h -- the device builder of the scene BVH8 (gi_bvh_build.hip): the same tree format bvh8.cpp produces, built on the GPU from the
// scene-order triangles (GI_C_SCENE_OPTION_BVH_BUILD).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <vector>

#include "gi_types.h"

namespace gi {

enum DeviceBvhStatus : int { DEVICE_BVH_OK = 0, DEVICE_BVH_OUT_OF_MEMORY = 1, DEVICE_BVH_TOO_DEEP = 2, DEVICE_BVH_ERROR = -1 };

struct DeviceBvhResult {
  Node8* nodes = nullptr;   // hipMalloc'd, exactly nodeCount nodes (the caller owns it)
  uint32_t nodeCount = 0, maxDepth = 0, activeTris = 0;
  Node8 root{};             // node 0, read back for the scene bounds
  double ms[4] = {0, 0, 0, 0}; // boxes, sort, PLOC (+ the collapse DP it fills), emission (+ the inactive tail)
  uint32_t plocIterations = 0;
  std::vector<uint32_t> levelStart; // first node of every breadth-first level, then nodeCount: maxDepth + 1 entries (Bvh8::levelStart)
  const char* error = "";
};

// `tris`: `n` TriRec in scene order on the current device (origId = position); `faceId`: the per-triangle side table in the same order.  Both are rewritten in
// leaf order: active triangles first (as the tree references them), the inactive ones behind in input order (bvh8.h "Inactive items").  The tree is a
// function of the input bytes alone.  Every temporary is freed before return; out of memory releases what was allocated and returns
// DEVICE_BVH_OUT_OF_MEMORY, a tree of more than `maxLevels` levels DEVICE_BVH_TOO_DEEP -- in both cases the contents of `tris` / `faceId` are unspecified
// (the caller falls back to the host builder, which uploads them anew).
int buildBvh8Device(hipStream_t st, TriRec* tris, int32_t* faceId, uint32_t n, uint32_t maxLevels, DeviceBvhResult& out);

} // namespace gi

// gi_refit.hip -- a vertex edit applied to the device-resident scene BVH (opt-in: GI_C_SCENE_OPTION_VERTEX_UPDATES; gi_build.cpp updateVertices, DESIGN.md
// section 6).  The points of a mesh moved and its topology stayed: the tree keeps its shape and gets new conservative boxes, which under the traversal
// contract (results do not depend on the tree) gives the image of a fresh build.
//
//   k_refit_tris    one thread per resident triangle record, in whatever order the builder left them.  The record names its instance; a table with one word
//                   per instance says whether the instance's mesh was edited.  Edited records get v0 / e1 / e2 made again from the mesh triangle's
//                   object-space corners (TriShade::p, named by vi[0] -- the host has sent the new shading records) and the instance's o2w with
//                   flattenTriangle's operations in its order (gi_refit.h refit_flatten; the library is built without contraction).  Only edited records
//                   are stored: nine dwords.  Memory-bound like the patch kernels: triangle count x one 64-byte line read.
//   k_refit_level   one launch per tree level, deepest first; one thread per node of the level (gi_refit.h refit_node).  A node reads its leaf triangles
//                   and, for internal children, the float boxes the PREVIOUS launch wrote (32 bytes per node), writes its own box and requantises itself.
//                   The level's nodes are given as ranges -- one per refit unit: the whole flat tree, or every part of an edited mesh in the partitioned
//                   layout -- in a table the host uploads; a thread finds its range by bisection.
//   k_gather_shade  the shading records of an edited mesh made again from the vertex records the host has just sent (gi_refit.h refit_shade_word: TriShade
//                   is FVertex gathered by vi[k]), in front of k_refit_tris, which reads TriShade::p.  Mapping: one thread per 16-byte PIECE -- nine per
//                   record, the gathered words 0..35; the tenth piece (vi, pad) is read by all nine and written by none.  Consecutive lanes store consecutive
//                   16-byte pieces (a wave covers 7.1 records = 1 024 contiguous bytes but for the skipped tenths), each piece has one writer, and the
//                   loads of a lane are four dwords out of at most two 48-byte vertex records that its neighbours read as well.  Memory-bound: per record
//                   144 bytes stored and one 64-byte line (vi) read, plus the mesh's vertex records once (48 bytes each; an indexed mesh has about half as
//                   many vertices as faces, and the repeats hit in L2): ~230 bytes per face against the 160 the host used to send over the link.
//
// No hand-off between workgroups inside a launch: a kernel boundary is the only one (the device builder's rule -- the per-XCD L2s are not coherent within a
// launch).  No arrival counters, no spinning, no fences; a 49-level tree is at most 49 thin launches.  No atomics; every node and record has one writer.
#include <cstddef>

#include "gi_kernels.h"
#include "gi_refit.h"

namespace gi {
namespace {

constexpr uint32_t kRefitBlock = 256;

__global__ __launch_bounds__(kRefitBlock) void k_refit_tris(TriRec* __restrict__ tris, uint32_t triCount, const InstanceRec* __restrict__ instances,
    uint32_t instanceCount, const uint32_t* __restrict__ editedOfInstance, const TriShade* __restrict__ triShade, uint32_t shadeCount)
{
  const uint32_t i = blockIdx.x * kRefitBlock + threadIdx.x;
  if (i >= triCount) return;
  TriRec& t = tris[i];
  const uint32_t inst = t.instance;
  if (inst >= instanceCount) return; // (cannot happen: the build numbers instances densely)
  if (editedOfInstance[inst] == 0u) return;
  const uint32_t rec = t.vi[0];
  if (rec >= shadeCount) return; // (cannot happen: scenes beyond LDS name their shading record there)
  float v0[3], e1[3], e2[3];
  refit_flatten(instances[inst].o2w, triShade[rec].p, v0, e1, e2);
  for (int a = 0; a < 3; a++) { t.v0[a] = v0[a]; t.e1[a] = e1[a]; t.e2[a] = e2[a]; }
}

constexpr uint32_t kShadePieces = kShadeGatherWords / 4u; // 16-byte pieces gathered per record
static_assert(sizeof(TriShade) == 160 && kShadeGatherWords % 4u == 0u && offsetof(TriShade, vi) == 4u * kShadeGatherWords, "k_gather_shade: pieces of a TriShade");

__global__ __launch_bounds__(kRefitBlock) void k_gather_shade(TriShade* __restrict__ triShade, uint32_t shadeCount, uint32_t first, uint32_t count,
    const FVertex* __restrict__ verts, uint32_t vertCount)
{
  const uint32_t i = blockIdx.x * kRefitBlock + threadIdx.x; // (count < 2^26 faces: 9 * count fits)
  if (i >= count * kShadePieces) return;
  const uint32_t rec = first + i / kShadePieces, piece = i % kShadePieces;
  if (rec >= shadeCount) return; // (cannot happen: the host checks the range against the array)
  TriShade* q = triShade + rec;
  const uint32_t vi[3] = {q->vi[0], q->vi[1], q->vi[2]};
  if (!refit_shade_corners_ok(vi, vertCount)) return; // (cannot happen: giCCreateMesh checks the faces)
  uint4 out;
  out.x = refit_shade_word(verts, vi, 4u * piece); out.y = refit_shade_word(verts, vi, 4u * piece + 1u);
  out.z = refit_shade_word(verts, vi, 4u * piece + 2u); out.w = refit_shade_word(verts, vi, 4u * piece + 3u);
  reinterpret_cast<uint4*>(q)[piece] = out; // 160-byte records in a hipMalloc block: every piece is 16-byte aligned
}

__global__ __launch_bounds__(kRefitBlock) void k_refit_level(Node8* __restrict__ nodes, uint32_t nodeCount, float* __restrict__ boxes,
    const RefitRange* __restrict__ ranges, uint32_t rangeCount, uint32_t threads, RefitScene S)
{
  const uint32_t i = blockIdx.x * kRefitBlock + threadIdx.x;
  if (i >= threads || rangeCount == 0u) return;
  uint32_t lo = 0, hi = rangeCount; // the last range whose threadBase <= i (ranges[0].threadBase == 0)
  while (hi - lo > 1u) { const uint32_t mid = (lo + hi) >> 1; if (ranges[mid].threadBase <= i) lo = mid; else hi = mid; }
  const uint32_t node = ranges[lo].nodeFirst + (i - ranges[lo].threadBase);
  if (node >= nodeCount) return; // (cannot happen: the ranges are levels of trees inside the node array)
  refit_node(nodes, nodeCount, node, boxes, S);
}

} // namespace

void launchRefitTris(hipStream_t s, TriRec* tris, uint32_t triCount, const InstanceRec* instances, uint32_t instanceCount, const uint32_t* editedOfInstance,
    const TriShade* triShade, uint32_t shadeCount)
{
  if (triCount == 0u) return;
  hipLaunchKernelGGL(k_refit_tris, dim3((triCount + kRefitBlock - 1u) / kRefitBlock), dim3(kRefitBlock), 0, s, tris, triCount, instances, instanceCount,
      editedOfInstance, triShade, shadeCount);
}

bool gatherShadeRangeOk(uint32_t shadeCount, uint32_t first, uint32_t count) { return first <= shadeCount && count <= shadeCount - first && count < (1u << 26); }

bool launchGatherShade(hipStream_t s, TriShade* triShade, uint32_t shadeCount, uint32_t first, uint32_t count, const FVertex* verts, uint32_t vertCount)
{
  if (!gatherShadeRangeOk(shadeCount, first, count)) return false;
  if (count == 0u) return true;
  const uint32_t threads = count * kShadePieces;
  hipLaunchKernelGGL(k_gather_shade, dim3((threads + kRefitBlock - 1u) / kRefitBlock), dim3(kRefitBlock), 0, s, triShade, shadeCount, first, count, verts, vertCount);
  return true;
}

void launchRefitLevel(hipStream_t s, Node8* nodes, uint32_t nodeCount, float* boxes, const RefitRange* ranges, uint32_t rangeCount, uint32_t threads,
    const TriRec* tris, uint32_t triCount, const InstanceRec* instances, uint32_t instanceCount, const TriShade* triShade, uint32_t shadeCount)
{
  if (threads == 0u || rangeCount == 0u) return;
  const RefitScene S{tris, triCount, instances, instanceCount, triShade, shadeCount};
  hipLaunchKernelGGL(k_refit_level, dim3((threads + kRefitBlock - 1u) / kRefitBlock), dim3(kRefitBlock), 0, s, nodes, nodeCount, boxes, ranges, rangeCount,
      threads, S);
}

} // namespace gi

// gi_blas.hip -- a vertex edit applied to the resident BLAS of a two-level scene (opt-in: GI_C_SCENE_OPTION_BLAS_UPDATES; gi_build.cpp
// updateVerticesTwoLevel).  The points of a mesh moved and its faces stayed: the mesh's one BLAS -- shared by all its instances, so the
// work is nf triangles, not nf x instances -- keeps its topology and gets the new corners and new conservative boxes.  The walk rebuilds the world-space
// triangle from BlasTri + InstTrav and tests it against the world-space ray, so hits do not depend on the BLAS's shape: the image is a fresh build's.
//
//   k_blas_tris          one thread per BLAS triangle of one edited mesh's range [first, first + nf), in the order the builder left.  A lane reads the third
//                        16-byte piece of its 64-byte record (p2.z, prim, two words of padding), takes the three object-space corners of face `prim` from
//                        the shading record shadeBase + prim (TriShade::p, the first 36 bytes of a 160-byte record: two 16-byte loads and a dword --
//                        k_gather_shade has just made those records from the re-sent vertex records) and rewrites the 48 used bytes as three 16-byte
//                        vector stores; prim and the padding are carried through, the fourth piece is never touched.  Memory-bound: 16 + 36 bytes read
//                        (the shading records by prim: scattered 64-byte lines), 48 bytes stored per face, consecutive lanes storing consecutive lines.
//   k_blas_refit_level   one launch per BLAS level, deepest first; one thread per node of the level over ALL edited meshes' BLASes at once: the level's
//                        nodes are ranges (one per edited BLAS that has the level) in a table the host uploads, and a thread finds its range by bisection
//                        -- gi_refit.hip k_refit_level's scheme, planned by the same host function.  The node arithmetic is gi_refit.h refit_node_with
//                        with the BLAS's leaf-box provider (gi_blas.h): a leaf slot's box is the padded minimum / maximum of the face's three corners,
//                        an internal slot's the 32-byte float box the child wrote in the PREVIOUS launch.
//
// Children's boxes cross a KERNEL BOUNDARY, never a hand-off inside a launch (gi_refit.hip's rule: the per-XCD L2s are not coherent within one).  No atomics,
// no counters, no fences; every node, record and scratch word has one writer.  Every index is checked against its array's count: a "cannot happen" returns.
#include <cstddef>

#include "gi_blas.h"
#include "gi_kernels.h"

namespace gi {
namespace {

constexpr uint32_t kBlasBlock = 256;
static_assert(sizeof(BlasTri) == 64 && offsetof(BlasTri, prim) == 36 && sizeof(TriShade) == 160 && offsetof(TriShade, p) == 0, "k_blas_tris: 16-byte pieces of its records");

__global__ __launch_bounds__(kBlasBlock) void k_blas_tris(BlasTri* __restrict__ blasTris, uint32_t blasTriCount, uint32_t first, uint32_t count,
    const TriShade* __restrict__ triShade, uint32_t shadeCount, uint32_t shadeBase)
{
  const uint32_t i = blockIdx.x * kBlasBlock + threadIdx.x;
  if (i >= count) return;
  if (first > blasTriCount || i >= blasTriCount - first) return; // (cannot happen: the host takes the range from the mesh's own BLAS)
  float4* rec = reinterpret_cast<float4*>(blasTris + first + i); // 64-byte records in a hipMalloc block: 16-byte aligned pieces
  float4 r2 = rec[2]; // p2 z, prim, -, -
  const uint32_t prim = __float_as_uint(r2.y);
  if (prim >= count || shadeBase > shadeCount || prim >= shadeCount - shadeBase) return; // (cannot happen: prim is a face of the mesh, whose records the host checked)
  const float4* q = reinterpret_cast<const float4*>(triShade + shadeBase + prim); // 160-byte records: 16-byte aligned
  const float4 q0 = q[0], q1 = q[1]; // p0 xyz p1 x | p1 yz p2 xy
  r2.x = reinterpret_cast<const float*>(q)[8]; // p2 z
  rec[0] = q0; rec[1] = q1; rec[2] = r2;
}

__global__ __launch_bounds__(kBlasBlock) void k_blas_refit_level(Node8* __restrict__ nodes, uint32_t nodeCount, float* __restrict__ boxes,
    const RefitRange* __restrict__ ranges, uint32_t rangeCount, uint32_t threads, const BlasTri* __restrict__ blasTris, uint32_t blasTriCount)
{
  const uint32_t i = blockIdx.x * kBlasBlock + threadIdx.x;
  if (i >= threads || rangeCount == 0u) return;
  uint32_t lo = 0, hi = rangeCount; // the last range whose threadBase <= i (ranges[0].threadBase == 0)
  while (hi - lo > 1u) { const uint32_t mid = (lo + hi) >> 1; if (ranges[mid].threadBase <= i) lo = mid; else hi = mid; }
  const uint32_t node = ranges[lo].nodeFirst + (i - ranges[lo].threadBase);
  if (node >= nodeCount) return; // (cannot happen: the ranges are levels of BLASes inside the node array)
  blas_refit_node(nodes, nodeCount, node, boxes, blasTris, blasTriCount);
}

} // namespace

bool blasTrisRangeOk(uint32_t blasTriCount, uint32_t first, uint32_t count, uint32_t shadeCount, uint32_t shadeBase)
{
  return first <= blasTriCount && count <= blasTriCount - first && shadeBase <= shadeCount && count <= shadeCount - shadeBase && count < (1u << 26);
}

bool launchBlasTris(hipStream_t s, BlasTri* blasTris, uint32_t blasTriCount, uint32_t first, uint32_t count, const TriShade* triShade, uint32_t shadeCount,
    uint32_t shadeBase)
{
  if (!blasTrisRangeOk(blasTriCount, first, count, shadeCount, shadeBase)) return false;
  if (count == 0u) return true;
  hipLaunchKernelGGL(k_blas_tris, dim3((count + kBlasBlock - 1u) / kBlasBlock), dim3(kBlasBlock), 0, s, blasTris, blasTriCount, first, count, triShade,
      shadeCount, shadeBase);
  return true;
}

void launchBlasRefitLevel(hipStream_t s, Node8* nodes, uint32_t nodeCount, float* boxes, const RefitRange* ranges, uint32_t rangeCount, uint32_t threads,
    const BlasTri* blasTris, uint32_t blasTriCount)
{
  if (threads == 0u || rangeCount == 0u) return;
  hipLaunchKernelGGL(k_blas_refit_level, dim3((threads + kBlasBlock - 1u) / kBlasBlock), dim3(kBlasBlock), 0, s, nodes, nodeCount, boxes, ranges, rangeCount,
      threads, blasTris, blasTriCount);
}

} // namespace gi

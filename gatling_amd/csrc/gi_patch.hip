// gi_patch.hip -- k_patch_mat_flags: TriRec::matFlags rewritten in place after a material edit (gi_build.cpp updateMaterials).
//
// A material or assignment edit changes one word per flattened triangle -- material index | shade class << 24 | cutout << 28 | facing << 30 -- and nothing
// else of the 64-byte record.  The triangles lie in whatever order their builder left them (leaf order of the host or the device builder, scene order inside
// the ranges of a partitioned tree); order does not matter here: a triangle names its instance, the instance its mesh, and the mesh's new word comes from a
// table the host uploads for the purpose.
//
// Layouts: the flat one in its three forms (host-built, device-built, partitioned) -- SceneDevice::dTris.  A two-level scene keeps the same flat triangles
// (k_shade and k_aov read them) and is patched the same way; its second copy of the word, InstTrav::matFlags, is one 128-byte record per INSTANCE and is
// re-sent by the host (BlasTri carries no material word).
//
// Memory: one thread per triangle reads the 8 bytes (instance, matFlags) at offset 40 of its record and, where the word differs, stores one dword.  A wave
// touches 64 different 64-byte records, so the pass is bound by the lines it touches (triangle count x 64 bytes read; written lines only for meshes whose
// word changed), not by the 8 + 4 bytes it uses.  InstanceRec::mesh and the table are read by every triangle of an instance and stay in the caches.
#include <cstddef>

#include "gi_kernels.h"

namespace gi {
namespace {

constexpr uint32_t kPatchBlock = 256;

__global__ __launch_bounds__(kPatchBlock) void k_patch_mat_flags(TriRec* __restrict__ tris, uint32_t triCount, const InstanceRec* __restrict__ instances,
    uint32_t instanceCount, const uint32_t* __restrict__ wordOfMesh, uint32_t meshCount)
{
  const uint32_t i = blockIdx.x * kPatchBlock + threadIdx.x;
  if (i >= triCount) return;
  static_assert(offsetof(TriRec, instance) == 40 && offsetof(TriRec, matFlags) == 44, "(instance, matFlags) is one aligned 8-byte piece");
  const uint2 im = *reinterpret_cast<const uint2*>(&tris[i].instance);
  if (im.x >= instanceCount) return; // (cannot happen: the build numbers instances densely)
  const uint32_t mesh = instances[im.x].mesh;
  if (mesh >= meshCount) return;
  const uint32_t word = wordOfMesh[mesh];
  if (word != im.y) tris[i].matFlags = word; // a plain vector store of the one dword
}

} // namespace

void launchPatchMatFlags(hipStream_t s, TriRec* tris, uint32_t triCount, const InstanceRec* instances, uint32_t instanceCount, const uint32_t* wordOfMesh,
    uint32_t meshCount)
{
  if (triCount == 0u) return;
  hipLaunchKernelGGL(k_patch_mat_flags, dim3((triCount + kPatchBlock - 1u) / kPatchBlock), dim3(kPatchBlock), 0, s, tris, triCount, instances, instanceCount,
      wordOfMesh, meshCount);
}

} // namespace gi

// gi_patch.hip -- edits applied in place to the device-resident triangle records:
//   k_patch_mat_flags   TriRec::matFlags rewritten after a material edit (gi_build.cpp updateMaterials)
//   k_patch_visibility  scene-order ids renumbered, records of hidden instances made unhittable / restored (gi_build.cpp updateVisibility; below)
//   k_patch_visibility2 the same on a two-level scene, with the id -> record table made again in the pass (gi_build.cpp updateVisibilityTwoLevel; below)
//   k_patch_inst_trav   InstTrav::triBase of renumbered instances of a two-level scene (the same edit; below)
//   k_place_part        a device-built part of an appended mesh moved into the scene's node array, its ids made scene-order (gi_build.cpp updateTopology; below)
//   k_clone_parts       new instances of resident meshes made from live sibling instances: records and subtrees copied and rebased (gi_build.cpp updateTopology; below)
//
// k_patch_mat_flags.
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
#include "gi_refit.h"

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

// k_patch_visibility.  Hiding or showing a mesh (opt-in: GI_C_SCENE_OPTION_VISIBILITY_UPDATES) changes two things in the records: the triangles of the meshes
// behind it in scene order get the ids a fresh build would give them (the cutout hash and the tie-break read TriRec::origId), and -- on the flat layouts,
// where one tree holds every instance -- the records of the mesh itself must stop being hit, and be hit again later.
//   hide: e1 = e2 = 0.  tri_test (gi_traversal.h, the one intersection routine of every walk) then computes det = dot(0, cross(d, 0)): +-0 for a finite
//         direction, NaN otherwise; `det != 0` fails for the zero, and with a NaN det u = NaN fails `u >= 0`.  No ray accepts the record.
//   show: e1 and e2 are made again from the mesh triangle's object-space corners (TriShade::p, named by vi[0]) and the instance's o2w exactly as
//         flattenTriangle makes them on the host -- xformPoint's ((a0 x + a1 y) + a2 z) + a3, then p1 - p0 and p2 - p0; the library is built without
//         contraction, so these are the host's IEEE operations in the host's order and the record is bytewise what it was.  v0 is never touched (it carries
//         the inactive marker of an unusable instance).
// The host uploads one VisPatch per instance; a thread reads its record's instance word, then the entry, and stores only words that change: one dword for a renumbering, six for a
// hide or a show.  No atomics; order does not matter.  Memory-bound like k_patch_mat_flags: triangle count x one 64-byte line read, lines written only for
// instances whose entry is not (0, keep).  A partitioned tree leaves hidden parts out of its top tree instead, so there only ids are renumbered.
__global__ __launch_bounds__(kPatchBlock) void k_patch_visibility(TriRec* __restrict__ tris, uint32_t triCount, const InstanceRec* __restrict__ instances,
    uint32_t instanceCount, const VisPatch* __restrict__ patchOfInstance, const TriShade* __restrict__ triShade, uint32_t shadeCount)
{
  const uint32_t i = blockIdx.x * kPatchBlock + threadIdx.x;
  if (i >= triCount) return;
  TriRec& t = tris[i];
  const uint32_t inst = t.instance;
  if (inst >= instanceCount) return; // (cannot happen: the build numbers instances densely)
  const VisPatch vp = patchOfInstance[inst];
  if (vp.idDelta != 0) t.origId = t.origId + (uint32_t)vp.idDelta;
  if (vp.action == VIS_HIDE) {
    for (int a = 0; a < 3; a++) { t.e1[a] = 0.0f; t.e2[a] = 0.0f; }
  } else if (vp.action == VIS_SHOW) {
    const uint32_t rec = t.vi[0];
    if (rec >= shadeCount) return; // (cannot happen: scenes beyond LDS name their shading record there)
    const float* m = instances[inst].o2w;
    float p[3][3];
    for (int k = 0; k < 3; k++) {
      const float x = triShade[rec].p[k][0], y = triShade[rec].p[k][1], z = triShade[rec].p[k][2];
      for (int r = 0; r < 3; r++) p[k][r] = ((m[4 * r] * x + m[4 * r + 1] * y) + m[4 * r + 2] * z) + m[4 * r + 3];
    }
    for (int a = 0; a < 3; a++) { t.e1[a] = p[1][a] - p[0][a]; t.e2[a] = p[2][a] - p[0][a]; }
  }
}

// k_patch_visibility2 / k_patch_inst_trav.  The same edit on a resident TWO-LEVEL scene (opt-in: GI_C_SCENE_OPTION_TLAS_VISIBILITY; gi_build.cpp
// updateVisibilityTwoLevel).  The flat records take k_patch_visibility's treatment (k_aov walks the flat tree, k_shade reads its records); in the same pass
// every record whose instance is visible AFTER the edit, and whose id or visibility changed, stores its own index at its NEW id in flatOfOrig -- the table
// k_trace_dyn2 turns a scene-order id (InstTrav::triBase + BlasTri::prim) into a flat record index with.  Records of hidden instances never store there:
// their stale ids overlap the ids the meshes behind them just received, and that overlap is the one way this pass can go wrong.  The visible ids are a
// permutation of [0, visibleTris), so every word has one writer: no atomics, any order; entries at and beyond visibleTris are never read and stay stale.
// The per-record form is gi_vispatch.h vis2_patch_record, which the host runs too (giCDebugPatchVisibilityTwoLevel compares the words).
// Memory: the pass reads one 64-byte line per resident triangle (origId, instance, vi[0] share it) and stores one dword into it per renumbered record, six
// more per hidden / shown record, and one SCATTERED dword into flatOfOrig per renumbered or shown visible record: records lie in leaf order, ids in scene
// order, so a wave's 64 stores touch up to 64 lines of the table.  The table and the VisPatch entries are read by nobody else in the pass.
// k_patch_inst_trav: one thread per instance, InstTrav::triBase += idDelta where it is not zero -- one dword of the 128-byte record; matFlags stays.
__global__ __launch_bounds__(kPatchBlock) void k_patch_visibility2(TriRec* __restrict__ tris, uint32_t triCount, const InstanceRec* __restrict__ instances,
    uint32_t instanceCount, const VisPatch* __restrict__ patchOfInstance, const TriShade* __restrict__ triShade, uint32_t shadeCount,
    uint32_t* __restrict__ flatOfOrig, uint32_t flatCount)
{
  const uint32_t i = blockIdx.x * kPatchBlock + threadIdx.x;
  if (i >= triCount) return;
  vis2_patch_record(tris, i, instances, instanceCount, patchOfInstance, triShade, shadeCount, flatOfOrig, flatCount);
}

__global__ __launch_bounds__(kPatchBlock) void k_patch_inst_trav(InstTrav* __restrict__ instTrav, uint32_t instanceCount, const VisPatch* __restrict__ patchOfInstance)
{
  const uint32_t i = blockIdx.x * kPatchBlock + threadIdx.x;
  if (i >= instanceCount) return;
  vis2_patch_inst_trav(instTrav, i, patchOfInstance);
}

// k_place_part.  A mesh appended to a partitioned scene (opt-in: GI_C_SCENE_OPTION_TOPOLOGY_UPDATES) whose parts the device builder made: buildBvh8Device ran
// over the part's own records at tris + triFirst and left (a) a tree in a block of its own whose child and triangle bases count from 0, (b) the records in
// leaf order with origId = position in the part.  Thread i < partNodeCount copies node i to nodes[nodeOff + i] with childBase += nodeOff and triBase +=
// triFirst -- placePart's two additions on the host -- and thread i < nf adds idAdd (the instance's first scene-order id) to record i's id.  One grid over
// max(partNodeCount, nf) threads: a tree has fewer nodes than triangles, so the node copy rides along with the id pass.  Plain vector loads and stores, no
// atomics: every thread owns its node and its record.  Memory-bound and small: 80 bytes read + written per node, one 64-byte line touched per record.
__global__ __launch_bounds__(kPatchBlock) void k_place_part(const Node8* __restrict__ partNodes, uint32_t partNodeCount, Node8* __restrict__ nodes, uint32_t nodeOff,
    TriRec* __restrict__ tris, uint32_t triFirst, uint32_t nf, uint32_t idAdd)
{
  const uint32_t i = blockIdx.x * kPatchBlock + threadIdx.x;
  if (i < partNodeCount) {
    Node8 n = partNodes[i];
    n.childBase += nodeOff; n.triBase += triFirst;
    nodes[nodeOff + i] = n;
  }
  if (i < nf) tris[triFirst + i].origId += idAdd;
}

// k_clone_parts.  A mesh of a partitioned scene gets more instances (opt-in: GI_C_SCENE_OPTION_INSTANCE_UPDATES).  Everything a new instance needs but its
// 96-byte InstanceRec is resident (the host sends that record and a zeroing of the node range, nothing per node or per triangle): the mesh's shading records, and a live sibling instance's part -- `nf` records in the order its builder left them and a
// subtree over exactly those positions.  One launch makes all new instances of an update from a table with one CloneEntry each; a thread finds its entry by
// bisection over threadBase (a multiple of 64: a wave never straddles two entries) and is thread j of it.
//   j < nf:        the sibling's record srcTri + j is read whole (4 x 16 bytes), becomes the new instance's by refit_clone_record -- instance, id = idBase +
//                  prim, v0 / e1 / e2 from TriShade::p of the record vi[0] names and the new instance's o2w with flattenTriangle's operations in its order (the
//                  library is built without contraction: the bytes are a fresh build's) -- and is stored whole at dstTri + j; the face id rides along.
//   j < nodeCount: the sibling's node srcNode + j is stored at dstNode + j with childBase and triBase moved by the distance between the ranges -- k_place_part's
//                  two additions, as deltas.  Its boxes are the sibling's until k_refit_level has run over the new range (the host launches it next).
// Plain vector loads and stores, no atomics: every thread owns its record and its node; source and destination ranges are disjoint (the destination lies
// behind everything resident).  Lane j of a wave touches record j and node j of consecutive 64-byte and 80-byte records: a wave reads and writes 4 KiB of
// records and 5 KiB of nodes as whole lines.  Memory-bound and small: per record 64 bytes read + 64 written, the 36 bytes of TriShade::p (one line of a
// 160-byte record, shared with no neighbour) and 4 + 4 bytes of face id; per node 80 bytes read + 80 written.  o2w is read by every lane and stays in the caches.
__global__ __launch_bounds__(kPatchBlock) void k_clone_parts(const CloneEntry* __restrict__ entries, uint32_t entryCount, uint32_t threads, TriRec* __restrict__ tris,
    uint32_t triCount, int32_t* __restrict__ triFaceId, Node8* __restrict__ nodes, uint32_t nodeCount, const InstanceRec* __restrict__ instances,
    uint32_t instanceCount, const TriShade* __restrict__ triShade, uint32_t shadeCount)
{
  const uint32_t i = blockIdx.x * kPatchBlock + threadIdx.x;
  if (i >= threads || entryCount == 0u) return;
  uint32_t lo = 0, hi = entryCount; // the last entry whose threadBase <= i (entries[0].threadBase == 0)
  while (hi - lo > 1u) { const uint32_t mid = (lo + hi) >> 1; if (entries[mid].threadBase <= i) lo = mid; else hi = mid; }
  const CloneEntry c = entries[lo];
  const uint32_t j = i - c.threadBase;
  if (j < c.nf && c.srcTri + j < triCount && c.dstTri + j < triCount && c.instance < instanceCount) { // (the ranges cannot lie outside: the host checks them)
    static_assert(sizeof(TriRec) == 64 && alignof(uint4) == 16, "a TriRec is four 16-byte pieces");
    union { TriRec t; uint4 q[4]; } in, out;
    const uint4* src = reinterpret_cast<const uint4*>(tris + c.srcTri + j);
    for (int k = 0; k < 4; k++) in.q[k] = src[k];
    const uint32_t rec = in.t.vi[0];
    if (rec < shadeCount) { // (cannot fail: scenes beyond LDS name their shading record there)
      out.t = refit_clone_record(in.t, instances[c.instance].o2w, triShade[rec].p, c.instance, c.idBase);
      uint4* dst = reinterpret_cast<uint4*>(tris + c.dstTri + j);
      for (int k = 0; k < 4; k++) dst[k] = out.q[k];
      triFaceId[c.dstTri + j] = triFaceId[c.srcTri + j];
    }
  }
  if (j < c.nodeCount && c.srcNode + j < nodeCount && c.dstNode + j < nodeCount) {
    Node8 n = nodes[c.srcNode + j];
    n.childBase += c.dstNode - c.srcNode; n.triBase += c.dstTri - c.srcTri;
    nodes[c.dstNode + j] = n;
  }
}

} // namespace

void launchCloneParts(hipStream_t s, const CloneEntry* entries, uint32_t entryCount, uint32_t threads, TriRec* tris, uint32_t triCount, int32_t* triFaceId,
    Node8* nodes, uint32_t nodeCount, const InstanceRec* instances, uint32_t instanceCount, const TriShade* triShade, uint32_t shadeCount)
{
  if (threads == 0u || entryCount == 0u) return;
  hipLaunchKernelGGL(k_clone_parts, dim3((threads + kPatchBlock - 1u) / kPatchBlock), dim3(kPatchBlock), 0, s, entries, entryCount, threads, tris, triCount,
      triFaceId, nodes, nodeCount, instances, instanceCount, triShade, shadeCount);
}

void launchPlacePart(hipStream_t s, const Node8* partNodes, uint32_t partNodeCount, Node8* nodes, uint32_t nodeOff, TriRec* tris, uint32_t triFirst, uint32_t nf,
    uint32_t idAdd)
{
  const uint32_t threads = partNodeCount > nf ? partNodeCount : nf;
  if (threads == 0u) return;
  hipLaunchKernelGGL(k_place_part, dim3((threads + kPatchBlock - 1u) / kPatchBlock), dim3(kPatchBlock), 0, s, partNodes, partNodeCount, nodes, nodeOff, tris,
      triFirst, nf, idAdd);
}

void launchPatchVisibility(hipStream_t s, TriRec* tris, uint32_t triCount, const InstanceRec* instances, uint32_t instanceCount, const VisPatch* patchOfInstance,
    const TriShade* triShade, uint32_t shadeCount)
{
  if (triCount == 0u) return;
  hipLaunchKernelGGL(k_patch_visibility, dim3((triCount + kPatchBlock - 1u) / kPatchBlock), dim3(kPatchBlock), 0, s, tris, triCount, instances, instanceCount,
      patchOfInstance, triShade, shadeCount);
}

void launchPatchVisibility2(hipStream_t s, TriRec* tris, uint32_t triCount, const InstanceRec* instances, uint32_t instanceCount, const VisPatch* patchOfInstance,
    const TriShade* triShade, uint32_t shadeCount, uint32_t* flatOfOrig, uint32_t flatCount)
{
  if (triCount == 0u) return;
  hipLaunchKernelGGL(k_patch_visibility2, dim3((triCount + kPatchBlock - 1u) / kPatchBlock), dim3(kPatchBlock), 0, s, tris, triCount, instances, instanceCount,
      patchOfInstance, triShade, shadeCount, flatOfOrig, flatCount);
}

void launchPatchInstTrav(hipStream_t s, InstTrav* instTrav, uint32_t instanceCount, const VisPatch* patchOfInstance)
{
  if (instanceCount == 0u) return;
  hipLaunchKernelGGL(k_patch_inst_trav, dim3((instanceCount + kPatchBlock - 1u) / kPatchBlock), dim3(kPatchBlock), 0, s, instTrav, instanceCount, patchOfInstance);
}

void launchPatchMatFlags(hipStream_t s, TriRec* tris, uint32_t triCount, const InstanceRec* instances, uint32_t instanceCount, const uint32_t* wordOfMesh,
    uint32_t meshCount)
{
  if (triCount == 0u) return;
  hipLaunchKernelGGL(k_patch_mat_flags, dim3((triCount + kPatchBlock - 1u) / kPatchBlock), dim3(kPatchBlock), 0, s, tris, triCount, instances, instanceCount,
      wordOfMesh, meshCount);
}

} // namespace gi

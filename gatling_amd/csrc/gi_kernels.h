// gi_kernels.h -- host-side launch interface of the stage kernels (gi_kernels.hip,
// gi_trace.hip, gi_shade.hip, gi_aov.hip, gi_patch.hip, gi_refit.hip, gi_tlas.hip) and of the fused one (gi_path.hip).
#pragma once

#include <type_traits>
#include <hip/hip_runtime.h>

#include "gi_types.h"
#include "gi_vispatch.h"

namespace gi {

// Launch selection: calls f with one std::bool_constant per bool, so that a generic lambda can name the kernel instantiation the run-time values pick
// (constexpr bool X = decltype(xC)::value).  Every combination the lambda's body can be called with is instantiated.
template <class F>
auto dispatchBools(F&& f) { return f(); }
template <class F, class... Bools>
auto dispatchBools(F&& f, bool b, Bools... rest)
{
  return b ? dispatchBools([&](auto... cs) { return f(std::true_type{}, cs...); }, rest...)
           : dispatchBools([&](auto... cs) { return f(std::false_type{}, cs...); }, rest...);
}

void launchInit(hipStream_t s, const PathState& st, const QueueSet& qs, Counters* cnt, uint32_t n, bool resetStats);
// `par` = iteration parity: k_raygen reads REGEN[par] and appends TRACE[par]; k_trace reads TRACE[par] and appends HIT and
// REGEN[par^1]; k_shade reads HIT and appends TRACE[par^1], REGEN[par^1], SHADOW.
void launchRaygen(hipStream_t s, uint32_t blocks, const FrameUniforms& U, const PathState& st, const QueueSet& qs, Counters* cnt, uint32_t par, F4* sampleBuf);
void launchAccumulate(hipStream_t s, const FrameUniforms& U, const F4* sampleBuf, F4* accum, F4* colorOut, bool firstBatch, bool lastBatch);
// sample look-ahead: folds the samples [first, first + U.spp) of a window of `windowSamples` samples per pixel into the colour AOV of the call `U` describes
void launchFoldWindow(hipStream_t s, const FrameUniforms& U, const F4* sampleBuf, F4* colorOut, uint32_t windowSamples, uint32_t first, bool pixelMajor);
// launchTrace runs the block-synchronous k_trace on this scene (staged whole in LDS, at most 8 levels deep) rather than k_trace_dyn + k_route
bool traceBlockSync(const SceneView& sc);
// a tree of this many nodes and triangles is staged whole in LDS (gi_traversal.h LDS_NODES / LDS_TRIS); beyond it the host packs shading records, sizes a
// larger path pool and may build the two-level layout
bool sceneFitsLds(size_t nodeCount, size_t triCount);
// dynamic LDS bytes of a traversal block: `stackEntries` stack entries per lane + staged nodes + staged triangles (gi_traversal.h StagedScene)
uint32_t traceLdsBytes(uint32_t stackEntries, uint32_t ldsNodes, uint32_t ldsTris);
// resident blocks per CU that the 160 KiB of LDS allow a kernel with this much dynamic and static LDS (256 bytes per block of allocation slack)
uint32_t blocksPerCuByLds(uint32_t dynamicBytes, uint32_t staticBytes);
uint32_t traceStaticLdsBytes(); // static LDS of the traversal kernels on top of traceLdsLayout's dynamic bytes
// what one k_trace block stages of this scene and the dynamic LDS bytes it needs for it
void traceLdsLayout(const SceneView& sc, uint32_t& ldsNodes, uint32_t& ldsTris, uint32_t& bytes);
// the per-lane stack rows of the traversal kernel launchTrace picks for this scene (k_trace: 4 or 8; k_trace_dyn: 8, 12 or 16; k_trace_dyn2: 16) and whether
// that variant spills entries beyond its rows to scratch (gi_traversal.h OVF_STACK)
uint32_t traceStackRows(const SceneView& sc, bool& spills);
void launchTrace(hipStream_t s, uint32_t blocks, bool anyHit, bool count, const SceneView& sc, const PathState& st, const QueueSet& qs, Counters* cnt,
                 uint32_t qIn, uint32_t qMiss, uint32_t dynRefill, uint32_t routeBlocks, const FrameUniforms& U, F4* sampleBuf);
void launchRoute(hipStream_t s, uint32_t blocks, const SceneView& sc, const PathState& st, const QueueSet& qs, Counters* cnt, uint32_t qIn, uint32_t qMiss,
    const FrameUniforms& U,
                 F4* sampleBuf); // (called by launchTrace behind a k_trace_dyn launch)
// most records a thread appends per trip of a streaming kernel (k_route ROUTE_ITEMS,
// k_raygen RAYGEN_ITEMS): sizes the queue shards' slack, gi_render.cpp shardCapacity
constexpr uint32_t APPEND_ITEMS_MAX = 4u;
// flag in dynRefill (shadow launches): children are visited in slot order instead of near-to-far (k_trace_dyn: DYN_SLOT_ORDER)
constexpr uint32_t TRACE_DYN_SLOT_ORDER = 0x200u;
// dynRefill: N in 1..64 = a k_trace_dyn wave refills once N of its lanes are idle
// one launch per material class present in the scene (the class is the sort key between k_trace and k_shade)
void launchShade(hipStream_t s, uint32_t blocks, uint32_t klass, bool textured /* some material of the class has textured inputs */,
    bool volume /* mediumStackSize > 0 */, const FrameUniforms& U, const SceneView& sc, const PathState& st, const QueueSet& qs, Counters* cnt, uint32_t par);

// Fused persistent path kernel (gi_path.hip) for LDS-resident scenes; launchPath returns the resident blocks per CU it launched with
bool pathKernelSupports(const SceneView& sc);
// lobePark: k_path's class-1 variants without NEE park hits that drew a glossy lobe and shade them together once this many are parked (0: off); the general
// variant takes it in counting builds only, every other variant ignores it
// ringCarry: the variants without NEE carry the triangle ring across the steps of a trip's closest-hit loop and flush it once (0: every step empties it)
// upsTraits: what the scene's class-1 materials have in common (gi_types.h UPS_*; 0: nothing, or the switch is off).  pathUpsVariant is the rule: the traits the
// kernel launchPath picks is compiled for -- the hot class-1 kernel without NEE takes them, every other one is the general text (0)
// nodeCook: the kernels pathCookVariant names run their COOK instantiation -- the nodes staged in the cooked form of gi_node_cook.h, the node test reading
// each child's hit-mask word from a table and only the occupied slots -- when the cooked image leaves blocksPerCuByLds what it is with the raw one (0: never).
// *cooked (may be null): whether the launch ran one
int launchPath(hipStream_t s, uint32_t cuCount, uint32_t classMask, bool textured, bool count, uint32_t chunk, uint32_t walkCarry, uint32_t lobePark,
               uint32_t ringCarry, uint32_t upsTraits, uint32_t nodeCook, const FrameUniforms& U, const SceneView& sc, const PathState& st, Counters* cnt,
               F4* sampleBuf, uint32_t* cooked);
// the kernels that have a COOK instantiation: the hot variants of class 0 and class 1 (the latter with or without UPS_NOCOAT) without NEE
inline bool pathCookVariant(uint32_t classMask, bool textured, bool nee, bool cutout, bool count)
{
  return (classMask == 1u || classMask == 2u) && !textured && !cutout && !count && !nee;
}
// traceLdsBytes with the nodes in their cooked form (gi_node_cook.h cook_image_bytes)
uint32_t pathCookedLdsBytes(uint32_t stackEntries, uint32_t ldsNodes, uint32_t ldsTris);
constexpr long NODE_COOK_DEFAULT = 1;  // GATLING_OPTIONS=node_cook (gi_options.h)
inline uint32_t pathUpsVariant(uint32_t classMask, bool textured, bool nee, bool cutout, bool count, uint32_t upsTraits)
{
  return (classMask == 2u && !textured && !cutout && !count && !nee) ? upsTraits : 0u;
}
constexpr long UPS_PLAIN_DEFAULT = 1;  // GATLING_OPTIONS=ups_plain (gi_options.h)
constexpr long WALK_CARRY_DEFAULT = 8; // GATLING_OPTIONS=walk_carry (gi_options.h)
constexpr long LOBE_PARK_DEFAULT = 8;  // GATLING_OPTIONS=lobe_park (gi_options.h)
constexpr long RING_CARRY_DEFAULT = 1; // GATLING_OPTIONS=ring_carry (gi_options.h)
constexpr long LEAF_LIFT_DEFAULT = 1;  // GATLING_OPTIONS=leaf_lift (gi_options.h; read at the scene build: gi_build.cpp leafLiftWanted)
// Where k_path keeps its parked hits (the lot): in the rows of its per-lane traversal stack that no walk of the tree reaches.  A walk pushes at most bvhDepth
// entries, so of the `stack` rows (4 for trees of depth <= 4, else 8) the rows from `row` = bvhDepth on are free; a row of a wave's 64 columns holds 8 records
// of 16 dwords.  capacity 0: nothing is free, the parking is off for this tree.  The launch's LDS is traceLdsBytes(stack, ...) as ever: the lot adds nothing.
// k_path clamps its threshold to the capacity (cornell, depth 1: 24 records; depth 2: 16; depth 3, 7: 8; depth 4, 8: none).
struct PathLot { uint32_t stack, row, capacity; };
inline PathLot pathLotPlacement(uint32_t bvhDepth)
{
  const uint32_t stack = bvhDepth <= 4u ? 4u : 8u;
  const uint32_t row = bvhDepth < stack ? bvhDepth : stack;
  return PathLot{stack, row, (stack - row) * 8u};
}

void launchAov(hipStream_t s, const FrameUniforms& U, const SceneView& sc, const AovTargets& A);
// gi_aov2.hip: the same AOVs for a two-level scene without the flat tree (sc.twoLevel, sc.nodeCount == 0); launchAov picks it
void launchAov2(hipStream_t s, const FrameUniforms& U, const SceneView& sc, const AovTargets& A);
void launchResolveNee(hipStream_t s, const FrameUniforms& U, const unsigned long long* key, F4* aov, uint32_t pixelCount);
void launchZeroClosest(hipStream_t s, Counters* cnt, uint32_t par); // FLAG_TWO_STREAM: in front of every closest-hit launch
// gi_patch.hip: rewrites TriRec::matFlags of the `triCount` device-resident triangles to wordOfMesh[instances[t.instance].mesh] where it differs
void launchPatchMatFlags(hipStream_t s, TriRec* tris, uint32_t triCount, const InstanceRec* instances, uint32_t instanceCount, const uint32_t* wordOfMesh,
    uint32_t meshCount);
// gi_patch.hip: a visibility edit applied to the device-resident triangles (gi_build.cpp updateVisibility).  One VisPatch per flattened instance: the change
// of its triangles' scene-order ids, and whether its records are left alone, made unhittable (both edges zeroed) or given their edges back (recomputed from
// the mesh triangle's shading record and the instance transform with the scene build's operations in its order) -- gi_vispatch.h has the record
void launchPatchVisibility(hipStream_t s, TriRec* tris, uint32_t triCount, const InstanceRec* instances, uint32_t instanceCount, const VisPatch* patchOfInstance,
    const TriShade* triShade, uint32_t shadeCount);
// gi_patch.hip: a visibility edit applied to a resident two-level scene (gi_build.cpp updateVisibilityTwoLevel, GI_C_SCENE_OPTION_TLAS_VISIBILITY).
// launchPatchVisibility2 is launchPatchVisibility over the flat records plus, in the same pass, flatOfOrig[new id] = i for every record whose instance is
// visible after the edit (VisPatch::action carries VIS_HIDDEN_AFTER for the others; `flatCount`: words of the table); launchPatchInstTrav moves
// InstTrav::triBase of every instance by its idDelta (gi_vispatch.h has both per-item forms)
void launchPatchVisibility2(hipStream_t s, TriRec* tris, uint32_t triCount, const InstanceRec* instances, uint32_t instanceCount, const VisPatch* patchOfInstance,
    const TriShade* triShade, uint32_t shadeCount, uint32_t* flatOfOrig, uint32_t flatCount);
void launchPatchInstTrav(hipStream_t s, InstTrav* instTrav, uint32_t instanceCount, const VisPatch* patchOfInstance);
// gi_patch.hip: a part the device builder made over the `nf` records at tris + triFirst (gi_build.cpp updateTopology) put where it lives: its `partNodes`
// nodes copied from the builder's block to nodes + nodeOff with child and triangle bases made absolute, and `idAdd` added to the ids of its records (the
// builder numbered them by position in the part).  The caller has checked both ranges against the arrays' sizes
void launchPlacePart(hipStream_t s, const Node8* partNodes, uint32_t partNodeCount, Node8* nodes, uint32_t nodeOff, TriRec* tris, uint32_t triFirst, uint32_t nf,
    uint32_t idAdd);
// gi_patch.hip: new instances of resident meshes made from live sibling instances (gi_build.cpp updateTopology, GI_C_SCENE_OPTION_INSTANCE_UPDATES).  One
// CloneEntry per new instance: the sibling's `nf` records at srcTri and `nodeCount` nodes at srcNode are copied to dstTri / dstNode -- records re-transformed by
// instances[instance].o2w and renumbered from idBase (gi_refit.h refit_clone_record), face ids copied, nodes with child and triangle bases moved by the
// distance between the ranges.  threadBase: first thread of the entry (ascending from 0, a multiple of 64; max(nf, nodeCount) threads each).  The caller has
// checked every range against the arrays' sizes and uploaded the new InstanceRecs; launchRefitLevel over the copied ranges follows
struct CloneEntry { uint32_t threadBase, srcTri, dstTri, nf, srcNode, dstNode, nodeCount, instance, idBase; };
inline uint32_t cloneEntryThreads(uint32_t nf, uint32_t nodeCount) { return ((nf > nodeCount ? nf : nodeCount) + 63u) & ~63u; }
void launchCloneParts(hipStream_t s, const CloneEntry* entries, uint32_t entryCount, uint32_t threads, TriRec* tris, uint32_t triCount, int32_t* triFaceId,
    Node8* nodes, uint32_t nodeCount, const InstanceRec* instances, uint32_t instanceCount, const TriShade* triShade, uint32_t shadeCount);
// gi_refit.hip: a vertex edit applied to the device-resident scene (gi_build.cpp updateVertices).  launchRefitTris makes the world-space corners of the records
// of edited instances (editedOfInstance[t.instance] != 0) again from their shading records and instance transforms; launchRefitLevel refits one tree level:
// thread i handles node ranges[r].nodeFirst + (i - ranges[r].threadBase) of the last range r with threadBase <= i, reading the float boxes (8 floats per
// node) of the level below and writing its own.  launchGatherShade makes the shading records [first, first + count) again from the vertex records they
// name (TriShade::vi; gi_refit.h refit_gather_shade): it runs behind the vertex upload and in front of launchRefitTris.
// gatherShadeRangeOk: the range lies inside the array and its nine threads per record fit a launch; launchGatherShade returns false, and launches nothing, where
// it does not hold -- the records would stay stale, so updateVertices asks first and declines to the rebuild
struct RefitRange { uint32_t threadBase, nodeFirst; };
void launchRefitTris(hipStream_t s, TriRec* tris, uint32_t triCount, const InstanceRec* instances, uint32_t instanceCount, const uint32_t* editedOfInstance,
    const TriShade* triShade, uint32_t shadeCount);
bool gatherShadeRangeOk(uint32_t shadeCount, uint32_t first, uint32_t count);
bool launchGatherShade(hipStream_t s, TriShade* triShade, uint32_t shadeCount, uint32_t first, uint32_t count, const FVertex* verts, uint32_t vertCount);
void launchRefitLevel(hipStream_t s, Node8* nodes, uint32_t nodeCount, float* boxes, const RefitRange* ranges, uint32_t rangeCount, uint32_t threads,
    const TriRec* tris, uint32_t triCount, const InstanceRec* instances, uint32_t instanceCount, const TriShade* triShade, uint32_t shadeCount);
// gi_tlas.hip: the padded world boxes of moved instances of a two-level scene (gi_build.cpp updateTransformsTwoLevel, GI_C_SCENE_OPTION_TLAS_UPDATES).  One
// 64-byte job per instance: its new o2w, its mesh's BLAS triangles [firstTri, firstTri + faceCount) and its instance index (carried for the host).
// launchInstBounds runs k_inst_bounds over jobCount x chunksPerJob workgroups (chunksPerJob = instBoundsChunks of the longest job; `partials`: 8 floats per
// workgroup) and k_inst_finish behind it, which writes 7 words per job to `out`: the padded box (lo xyz, hi xyz) and the status (gi_tlas.h TLAS_STATUS_*,
// 0 = usable).  Scratch only.  False, and nothing launched: the grid would not fit a launch.
struct InstBoundsJob { float o2w[12]; uint32_t firstTri, faceCount, instance, pad; };
constexpr uint32_t kInstBoundsChunk = 4096u;
uint32_t instBoundsChunks(uint32_t faceCount);
bool launchInstBounds(hipStream_t s, const InstBoundsJob* jobs, uint32_t jobCount, uint32_t chunksPerJob, const BlasTri* blasTris, uint32_t blasTriCount,
    float* partials, uint32_t* out);
// gi_blas.hip: a vertex edit applied to the resident BLAS of a two-level scene (gi_build.cpp updateVerticesTwoLevel, GI_C_SCENE_OPTION_BLAS_UPDATES).
// launchBlasTris gives the BLAS triangles [first, first + count) of one mesh -- count = its face count -- the object-space corners of the faces they name
// (BlasTri::prim) from the shading records shadeBase + prim, behind launchGatherShade on the same stream; blasTrisRangeOk: both ranges lie inside their
// arrays and the threads fit a launch -- launchBlasTris returns false, and launches nothing, where it does not hold.  launchBlasRefitLevel refits one level
// of the edited BLASes (launchRefitLevel's ranges and thread mapping; `boxes`: 8 floats per node of the whole BLAS node array), deepest level first
bool blasTrisRangeOk(uint32_t blasTriCount, uint32_t first, uint32_t count, uint32_t shadeCount, uint32_t shadeBase);
bool launchBlasTris(hipStream_t s, BlasTri* blasTris, uint32_t blasTriCount, uint32_t first, uint32_t count, const TriShade* triShade, uint32_t shadeCount,
    uint32_t shadeBase);
void launchBlasRefitLevel(hipStream_t s, Node8* nodes, uint32_t nodeCount, float* boxes, const RefitRange* ranges, uint32_t rangeCount, uint32_t threads,
    const BlasTri* blasTris, uint32_t blasTriCount);
// gi_append.hip: a mesh appended to a resident two-level scene without the flat tree (gi_build.cpp updateTopologyTwoLevel, GI_C_SCENE_OPTION_TLAS_TOPOLOGY;
// gi_append.h has every per-item form and AppendMesh).  On one stream, in this order: launchAppendShadeIndex writes TriShade::vi / pad of the mesh's faces
// (`faces3`: three indices per face, relative to the mesh), launchGatherShade fills the rest of those records from the vertex records, then
// launchAppendBlasTris writes the mesh's whole BlasTri records in the builder's `order` and launchAppendRecords the flat records, face-id words and id-table
// words of all its instances.  Each returns false, and launches nothing, where a range lies outside its array or the threads do not fit a launch
struct AppendMesh;
bool launchAppendShadeIndex(hipStream_t s, TriShade* triShade, uint32_t shadeCount, uint32_t shadeBase, const uint32_t* faces3, uint32_t faceCount,
    uint32_t vertexOffset);
bool launchAppendBlasTris(hipStream_t s, BlasTri* blasTris, uint32_t blasTriCount, uint32_t first, const uint32_t* order, uint32_t faceCount,
    const TriShade* triShade, uint32_t shadeCount, uint32_t shadeBase);
bool launchAppendRecords(hipStream_t s, const AppendMesh& M, TriRec* tris, int32_t* triFaceId, uint32_t* flatOfOrig, const InstanceRec* instances,
    const TriShade* triShade, const int32_t* faceIdOfFace);
// gi_instances.hip: the flat records, face-id words and id-table words of all new instances of built meshes of one sync, in one launch (gi_build.cpp
// updateInstancesTwoLevel, GI_C_SCENE_OPTION_TLAS_INSTANCES; gi_instances.h has every per-item form, InstanceJob and InstanceJobSizes).  `hostJobs`: the table
// `deviceJobs` holds, for the range check (instanceJobsOk): false, and nothing launched, for a job outside its arrays, 2^28 or more items, or a workgroup
// prefix that is not the job sizes'.  The caller keeps the jobs' ranges disjoint
struct InstanceJob; struct InstanceJobSizes;
bool launchInstanceRecords(hipStream_t s, const InstanceJob* hostJobs, const InstanceJob* deviceJobs, const InstanceJobSizes& Z, TriRec* tris, int32_t* triFaceId,
    uint32_t* flatOfOrig, const InstanceRec* instances, const TriShade* triShade, const int32_t* faceIdTable);
// gi_compact.hip: the live ranges of ONE array kind of a resident two-level scene moved to the front of a new allocation, their indices rebased, in one launch
// (gi_build.cpp compactTwoLevel, GI_C_SCENE_OPTION_TLAS_COMPACTION; gi_compact.h has every per-item form, CompactRange and CompactSizes).  `hostRanges`: the
// table `deviceRanges` holds, for the range check (compactRangesOk): false, and nothing launched, for a range outside the old array, destinations that do not
// ascend without gaps to Z.dstCount, a prefix that is not the range sizes', or src == dst.  `table`: the new id table (COMPACT_TRIS), else null
struct CompactRange; struct CompactSizes;
bool launchCompactRanges(hipStream_t s, const CompactRange* hostRanges, const CompactRange* deviceRanges, const CompactSizes& Z, const void* src, void* dst,
    uint32_t* table);
void launchSpin(hipStream_t s, unsigned long long ns);           // test hook: occupies a stream for ~ns nanoseconds
void launchDebugBsdf(hipStream_t s, const MaterialRec* mat, uint32_t shadeClass, uint32_t count, const float* in, float* out);
void launchDebugSqrt(hipStream_t s, uint32_t first, unsigned long long count, unsigned long long* mismatches); // gi_sqrt against sqrtf over bit patterns
void launchDebugDiv(hipStream_t s, uint32_t mode, unsigned long long count, uint32_t seed, const uint32_t* words, unsigned long long* mismatches); // gi_div against `/`
// trav_node_test against trav_node_test_cooked on `count` (node i % nodeCount, ray i) pairs (gi_path.hip k_debug_node_cook); -1: more nodes than a block cooks
int launchDebugNodeCook(hipStream_t s, const Node8* nodes, uint32_t nodeCount, const float* rays, unsigned long long count, unsigned long long* mismatches);
void launchDebugTex(hipStream_t s, const float* texels, uint32_t w, uint32_t h, uint32_t d, uint32_t count, const float* queries, float* out);

} // namespace gi

// gi_options.h -- the library's environment interface in one place.
//
// Environment variables (all optional):
//   GATLING_DEVICE         HIP device ordinal for gtl::giInitialize (the reference picks its Vulkan device itself, CgpuVk.cpp:892-909)          [gtl_shim.cpp]
//   GATLING_DEVICES        "0,1,2,3" or "all": one process drives several devices inside the library                     [gi_c.cpp]
//   GATLING_BUILD_THREADS  host threads of the BVH build (default: all, at most 32; the tree does not depend on it)                      [bvh8.cpp, gi_c.cpp]
//   GATLING_BUILD_TIMING   log scene-build / transform-update timings to stderr
//   GATLING_ITER_LOG       with kernel timers on every iteration: one line per bounce iteration (queue sizes, stage times) to stderr
//   GATLING_OPTIONS        "key=value,key=value": the debug / test switches below.  None changes an image (tests hold every one of them to the oracle
//                          bit for bit); they select between equivalent schedules, or pin sizes the library otherwise plans itself.
//
//   key                  default   meaning
//   trace_dyn            8         refill threshold of k_trace_dyn, 1 .. 64; 0 or below = the default
//                                  (same as GI_C_SCENE_OPTION_TRACE_DYNAMIC)
//   two_level            -1        -1 = automatic (from 2^26 flattened triangles), 0 / 1 = force the flat / the two-level layout
//   work_order           1         1 = pixel-major work items, 0 = sample-major
//   defer_slot           1         path slots are written where a path first hits
//   bounds_retire        1         camera rays that cannot reach the scene's bounds retire where they are generated: in k_raygen (wavefront pipeline,
//                                  deferred slots) and in k_path's ring preparation (fused kernel); 0 = every camera ray is traced
//   miss_rect            1         fused frames with bounds_retire: pixels whose every camera ray misses the scene's bounds (outside an image-space rectangle
//                                  the host derives per render, gi_miss_rect.h) get no work items and no sample records; 0 = every pixel is enumerated
//   walk_carry           8         fused frames without next-event estimation: the closest-hit loop of a k_path trip ends once at most this many lanes are
//                                  still walking (and more entered); they go on walking in the next trip's loop (gi_path.hip).  0 = every loop runs until
//                                  its last ray is done; 63 (tests) = carry whenever a lane has finished.  Counting builds run with 0 unless the key is set
//                                  explicitly: then it reaches them too (giCDebugPathWalkStats shows what it did)
//   lobe_park            8         fused frames without next-event estimation whose materials are all UsdPreviewSurface: a k_path wave sets hits that drew a
//                                  glossy lobe aside and shades them together once this many are parked (gi_path.hip), clamped to what the free rows of
//                                  the traversal stack hold (gi_kernels.h pathLotPlacement).  0 = every hit is shaded in the trip that found it; 1 (tests) =
//                                  most eager; 64 (tests) = as late as the lot allows.  Counting builds run with 0 unless the key is set explicitly
//                                  (giCDebugPathLobeStats shows what it did)
//   ring_carry           1         fused frames without next-event estimation: the ring of (ray, triangle) pairs of a k_path wave is carried across the steps
//                                  of a trip's closest-hit loop -- a triangle batch runs when 64 pairs are pending, and one flush at the loop's end tests the
//                                  rest (gi_path.hip).  0 = every step ends with a batch over whatever is pending.  Counting builds run with 0 unless the
//                                  key is set explicitly: a lagging culling distance moves their node and triangle counts (giCDebugPathRingStats shows
//                                  the batches either way)
//   ups_plain            1         fused frames without next-event estimation whose materials are all untextured UsdPreviewSurface: k_path runs the variant
//                                  compiled for what those materials have in common -- no coat (clearcoat +0 in every one) -- which leaves out the
//                                  operations that are exact identities then (gi_shading.h bsdf_sample; the traits: gi_build.cpp
//                                  deriveSceneClasses, giCDebugSceneUpsPlain).  0 = the general class-1 kernel.  Counting builds never run the variant
//   leaf_lift            1         scene build: the flat tree of a scene the fused kernel walks out of LDS (LDS-resident, not two-level, a root and one level
//                                  below it) goes through liftLeafSlots (leaf_lift.cpp): leaf slots that stretch a child's box move into free slots of the
//                                  root while the builder's cost model strictly decreases.  0 = the builder's tree, byte for byte.  Overrides
//                                  GI_C_SCENE_OPTION_LEAF_LIFT; read at the scene build (giCDebugSceneLeafLift shows what it did)
//   node_cook            1         fused frames without next-event estimation whose materials are all of one class, 0 or 1, and untextured: k_path runs the
//                                  variant that stages its nodes cooked (gi_node_cook.h) -- the word each child adds to the hit mask comes from a per-octant
//                                  table made once per block instead of a decode per visit, and the child loop covers the occupied slots only -- provided
//                                  the larger node image costs no resident block (gi_path.hip launchPath).  0 = the kernel that decodes the meta bytes.
//                                  Counting builds never run the variant (giCDebugSceneNodeCook shows which one ran)
//   fused                1         LDS-resident scenes run the fused persistent kernel
//   pool_slots           0         pin the path pool (slots); 0 = the memory plan decides
//   sample_buffer_mb     0         pin the per-sample buffer (MiB); 0 = the memory plan decides
//   assume_free_mb       0         tests: plan as if this many MiB were free on the device
//   incremental          1         transform-only edits update the tree in place
//   device_build         -1        -1 = the scene option decides (GI_C_SCENE_OPTION_BVH_BUILD), 0 / 1 = force the host / the device BVH builder
//                                  (flat-layout scenes of more than 128 triangles; read at build time)
//   ploc_radius          16        device builder: PLOC's nearest-neighbour search radius (positions either side in Morton order, 1 .. 256)
//   shadow_order         -1        visiting order of shadow walks: -1 = measured per scene (gi_render.cpp shadowOrder), 0 = near-to-far, 1 = slot order
//   peer_copies          1         multi-device gather: 0 = stage every device's row share through pinned host memory even where peer access exists
//   shade_variants       1         OpenPBR materials without optional lobes are binned and shaded by the BASE variant of k_shade (gi_shading.h);
//                                  0 = the full kernel for all
//   merge_shade_variants -1        -1 = thin batches (work fits the pool, <= 8 Mi items) bin BASE hits with the full OpenPBR class (one launch fewer
//                                  per iteration); 0 / 1 = never / always
//   two_stream           1         batches whose work fits the pool run their shadow launches on a second stream beside the next closest-hit launch
//                                  (gi_render.cpp "two streams")
//   two_stream_delay     0         tests: 1 / 2 = hold the main / the second stream back 0.3 ms per iteration so that the other one runs ahead
//   lookahead            -1        sample look-ahead of progressive low-spp calls: -1 = the scene option decides (GI_C_SCENE_OPTION_SAMPLE_LOOKAHEAD),
//                                  0 / 1 = off, N >= 2 = a call may trace the samples of up to N calls in one batch (gi_render.cpp planLookahead)
//   visibility_updates   -1        -1 = the scene option decides (GI_C_SCENE_OPTION_VISIBILITY_UPDATES), 0 / 1 = visibility edits rebuild the scene / are
//                                  applied to the resident scene (gi_build.cpp updateVisibility)
//   vertex_updates       -1        -1 = the scene option decides (GI_C_SCENE_OPTION_VERTEX_UPDATES), 0 / 1 = vertex edits (giCSetMeshVertices) rebuild the
//                                  scene / refit the resident tree on the device (gi_build.cpp updateVertices, gi_refit.hip)
//   topology_updates     -1        -1 = the scene option decides (GI_C_SCENE_OPTION_TOPOLOGY_UPDATES), 0 / 1 = mesh creations and destructions rebuild the
//                                  scene / are applied to the resident scene (gi_build.cpp updateTopology)
//   resync_refits        -1        -1 = the scene option decides (GI_C_SCENE_OPTION_RESYNC_REFITS), 0 / 1 = a destroyed and a created mesh with the same
//                                  faces are retired and appended / become a vertex refit of the resident records (gi_build.cpp adoptResyncs); read
//                                  only with topology_updates and vertex_updates wanted
//   instance_updates     -1        -1 = the scene option decides (GI_C_SCENE_OPTION_INSTANCE_UPDATES), 0 / 1 = new instance ids or another instance count
//                                  of a built mesh rebuild the scene / are applied to the resident scene (gi_build.cpp updateTopology); read only with
//                                  topology_updates wanted
//   instance_clone       0         instance updates: 1 = an appended instance is made from a resident sibling on the device (gi_patch.hip k_clone_parts);
//                                  0 = it is built as an appended mesh's part is (cheaper to walk: DESIGN.md section 9)
//   device_parts_min     4096      topology updates with the device builder on: an appended part of at least this many faces (and more than 128) is built
//                                  on the device (buildBvh8Device + gi_patch.hip k_place_part), a smaller one by the host (buildPart).  The measured
//                                  crossover for one part
//   tlas_updates         -1        -1 = the scene option decides (GI_C_SCENE_OPTION_TLAS_UPDATES), 0 / 1 = transform edits of a two-level scene rebuild it /
//                                  are applied to the resident scene (gi_build.cpp updateTransformsTwoLevel)
//   blas_updates         -1        -1 = the scene option decides (GI_C_SCENE_OPTION_BLAS_UPDATES), 0 / 1 = vertex edits of a two-level scene rebuild it / are
//                                  applied to the resident scene (gi_build.cpp updateVerticesTwoLevel); read only with vertex_updates wanted
//   tlas_visibility      -1        -1 = the scene option decides (GI_C_SCENE_OPTION_TLAS_VISIBILITY), 0 / 1 = visibility edits of a two-level scene rebuild it
//                                  / are applied to the resident scene (gi_build.cpp updateVisibilityTwoLevel); read only with visibility_updates wanted
//   tlas_only            -1        -1 = the scene option decides (GI_C_SCENE_OPTION_TLAS_ONLY), 0 / 1 = a scene that wants the two-level layout builds the flat
//                                  tree beside it / builds, sends and keeps no flat tree (gi_build.cpp buildScene; AOVs walk the TLAS: gi_aov2.hip); read at
//                                  the scene build, and only with the two-level layout wanted
//   tlas_topology        -1        -1 = the scene option decides (GI_C_SCENE_OPTION_TLAS_TOPOLOGY), 0 / 1 = mesh creations and destructions on a two-level
//                                  scene built without the flat tree rebuild it / are applied to the resident scene (gi_build.cpp updateTopologyTwoLevel; the
//                                  per-triangle records are made on the device: gi_append.hip); read only with topology_updates wanted
//   tlas_instances       -1        -1 = the scene option decides (GI_C_SCENE_OPTION_TLAS_INSTANCES), 0 / 1 = instance-count and instance-id edits of built
//                                  meshes on a two-level scene built without the flat tree rebuild it / are applied to the resident scene (gi_build.cpp
//                                  updateInstancesTwoLevel; the flat records of all new instances are made on the device in one launch: gi_instances.hip);
//                                  read only with topology_updates, instance_updates and tlas_topology wanted
//   tlas_device_build    -1        -1 = the scene option decides (GI_C_SCENE_OPTION_TLAS_DEVICE_BUILD), 0 / 1 = the edits in place of a two-level scene build
//                                  their TLAS with the host builder / on the primary device (gi_tlas_build.hip; gi_build.cpp buildEditTlas); read only
//                                  where tlas_updates, blas_updates, tlas_visibility, tlas_topology or tlas_instances applies an edit
//   tlas_device_min      TLAS_DEVICE_MIN_DEFAULT   with tlas_device_build: scenes of fewer instances keep the host builder (the crossover)
//   tlas_depth_budget    -         with tlas_device_build: lowers the device builder's depth budget below the stack rule's (tests)
//   blas_device_build    -1        -1 = the scene option decides (GI_C_SCENE_OPTION_BLAS_DEVICE_BUILD), 0 / 1 = the BLAS of a mesh of a two-level scene is built
//                                  by the host builder / on the primary device (gi_blas_build.hip; gi_build.cpp makeMeshBlas); read where a BLAS is built:
//                                  at the scene build (buildTwoLevel) and where tlas_topology applies a mesh create (updateTopologyTwoLevel)
//   blas_device_min      BLAS_DEVICE_MIN_DEFAULT   with blas_device_build: meshes of fewer faces keep the host builder (the crossover)
//   blas_device_max      BLAS_DEVICE_MAX_DEFAULT   with blas_device_build: meshes of more faces keep the host builder (the slab: about 1.5 KB per face)
//   blas_depth_budget    -         with blas_device_build: lowers the device builder's depth budget below the stack rule's (tests)
//   tlas_compaction      -1        -1 = the scene option decides (GI_C_SCENE_OPTION_TLAS_COMPACTION), 0 / 1 = the retired ranges topology and instancer edits in
//                                  place leave on a two-level scene without the flat tree stay until the scene is rebuilt / are compacted on the device
//                                  when they outgrow tlas_compact_percent (gi_compact.hip; gi_build.cpp compactTwoLevel); read only where tlas_topology or
//                                  tlas_instances is about to apply an edit
//   tlas_compact_percent 100       with tlas_compaction: the resident scene is compacted before an edit in place when retired x 100 > live x P on the planned
//                                  after-edit triangle counts; 100 is the point at which the edit declines and the scene is rebuilt without the option, 0
//                                  compacts whenever anything is retired (tests)
//   denoise_form         0         giCDenoise: where k_denoise_pass takes its taps from (gi_denoise.hip; every form stores the same bytes): 0 = an LDS tile with
//                                  a 2 x step halo at steps 1 and 2, direct 16-byte loads above (the measured choice); 1 = direct loads at
//                                  every step; 2 = the tile at steps 1, 2 and 4.  giCDenoiseVariance reads it the same way (gi_denoise_var.hip) and knows
//                                  3 = form 0 with the 3 x 3 variance average of the direct-load steps written by a launch of its own (giCDenoise: as 0)
//   phase_stats          0         counting builds: print k_path's phase split / k_trace_dyn's lane accounting
#pragma once

#include <cstdlib>
#include <cstring>

namespace gi {

// instances below which an edit's TLAS stays with the host builder although GI_C_SCENE_OPTION_TLAS_DEVICE_BUILD is on (GATLING_OPTIONS=tlas_device_min): the
// measured crossover of a steady transform edit (tools/time_tlas_device_build.py --crossover, profiles/r23_tlas_device_build.txt: the host builder wins at
// 4 096 instances, 1.39 against 2.48 ms, the device builder from 8 281 on, 2.74 against 3.27 ms)
constexpr long TLAS_DEVICE_MIN_DEFAULT = 8192;

// faces below which a mesh's BLAS stays with the host builder although GI_C_SCENE_OPTION_BLAS_DEVICE_BUILD is on (GATLING_OPTIONS=blas_device_min): the
// measured crossover of one BLAS at a scene build (tools/time_blas_device_build.py --crossover, profiles/r25_blas_device_build.txt: the host builder wins at
// 5 120 faces, 2.69 against 3.38 ms, the device builder from 20 480 on, 3.89 against 11.71 ms)
constexpr long BLAS_DEVICE_MIN_DEFAULT = 20480;
// ... and above which it does (GATLING_OPTIONS=blas_device_max): the builder's slab takes about 1.5 KB per face at depth budget 12
constexpr long BLAS_DEVICE_MAX_DEFAULT = 1L << 20;

// value of `key` in $GATLING_OPTIONS, or `def`.  Read at every call (tests change the variable between renders of one process).
inline long optionValue(const char* key, long def)
{
  const char* s = getenv("GATLING_OPTIONS");
  if (!s) return def;
  const size_t n = strlen(key);
  while (*s) {
    while (*s == ',' || *s == ' ') s++;
    if (!strncmp(s, key, n) && s[n] == '=') return strtol(s + n + 1, nullptr, 10);
    while (*s && *s != ',') s++;
  }
  return def;
}
inline bool optionSet(const char* key) { return optionValue(key, -0x7fffffffL) != -0x7fffffffL; }

} // namespace gi

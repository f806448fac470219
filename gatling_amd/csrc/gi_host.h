// gi_host.h -- shared declarations of the host side (gi_c.cpp, gi_scene.cpp, gi_textures.cpp, gi_lights.cpp, gi_build.cpp, gi_render.cpp, gi_debug.cpp, gi_denoise_host.cpp): host
// side of the MI355X-native gi core: scene containers, dirty flags, host packing, BVH build,
// uploads, the wavefront bounce loop, render buffers.  Implements include/gi_c.h.
//
// Restates the host logic of /root/reference/src/gi/impl/Gi.cpp behind the same API shape:
//   giCreateMesh/giSetMesh* (:620-782)          -> MeshData + dirty flags
//   _giBuildGeometryStructures/_giCreateBvh (:784-1315) -> flatten instances, pack FVertex, build BVH8, upload
//   giRender (:1989-2524)                        -> dirty handling, uniforms (:2373-2426), bounce loop, D2H
//   light setters (:2573-2976)                   -> CPU mirrors of the 48-byte device structs, dense stores
//   render buffers (:2978-3006)
// GPU plumbing (src/cgpu, src/ggpu in the reference) is the HIP runtime: hipMalloc / hipMemcpyAsync / streams.

#pragma once

// the C ABI keeps default visibility; everything else in the host translation units is built with -fvisibility=hidden (gatling_amd/build.py)
#pragma GCC visibility push(default)
#include "../../include/gi_c.h"
#pragma GCC visibility pop


#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <condition_variable>
#include <functional>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "bvh8.h"
#include "gi_tlas_build.h"
#include "gi_kernels.h"
#include "gi_image.h"
#include "gi_options.h"
#include "gi_pack.h"
#include "gi_types.h"

using namespace gi;

// ---------------------------------------------------------------------------------------------------------------
// global state (one giCInitialize per process, like Gi.cpp:244-259)
// ---------------------------------------------------------------------------------------------------------------

constexpr bool WORK_ORDER_PIXEL_MAJOR_DEFAULT = true;  // (GATLING_OPTIONS work_order) FLAG_PIXEL_MAJOR, gi_queues.h work_item

extern thread_local std::string t_lastError;
void setError(const std::string& e);

#define HIP_TRY(expr)                                                                                      \
  do {                                                                                                     \
    hipError_t _e = (expr);                                                                                \
    if (_e != hipSuccess) { setError(std::string(#expr) + ": " + hipGetErrorString(_e)); return GI_C_ERROR; } \
  } while (0)

// One entry per HIP device the library renders on (giCInitializeDevices / $GATLING_DEVICES; giCInitialize: one).  devs[0] is the PRIMARY device:
// render buffers, textures and every single-device entry point live there; the others hold replicas of the scene and render row shares.
struct DevCtx { int device = 0; int cuCount = 256; hipStream_t stream = nullptr; hipStream_t stream2 = nullptr;
    /* the shadow launches of two-stream batches (gi_render.cpp scheduleFrame "Two streams", runWavefrontBatch) */
                /* 1: the primary device and this one address each other's memory (peer access enabled both ways, or the same physical device); 0: no peer
                   access -- the device's row shares travel through pinned host memory; -1: hipDeviceCanAccessPeer / EnablePeerAccess failed with an error */
                int peer = 1; };
// One host thread per further device, created with the first multi-device render and kept until giCTerminate (a frame's share is handed to it as a job; until
// r04 every frame created and joined its own std::threads).  The thread binds its HIP device once.
struct DeviceWorker {
  std::thread th; std::mutex m; std::condition_variable cv;
  std::function<void()> job; bool busy = false, stop = false;
  void start() { th = std::thread([this] { std::unique_lock<std::mutex> lk(m);
      for (;;) { cv.wait(lk, [this] { return busy || stop; }); if (stop) return; lk.unlock(); job(); lk.lock(); busy = false; cv.notify_all(); } }); }
  void post(std::function<void()> fn) { { std::lock_guard<std::mutex> lk(m); job = std::move(fn); busy = true; } cv.notify_all(); }
  void wait() { std::unique_lock<std::mutex> lk(m); cv.wait(lk, [this] { return !busy; }); }
  void shutdown() { { std::lock_guard<std::mutex> lk(m); stop = true; } cv.notify_all(); if (th.joinable()) th.join(); }
  ~DeviceWorker() { shutdown(); } // (a process that exits without giCTerminate must not meet a joinable std::thread in a static destructor)
};
struct Context {
  bool initialized = false;
  int device = 0;               // == devs[0].device
  int cuCount = 256;            // == devs[0].cuCount
  hipStream_t stream = nullptr; // == devs[0].stream
  std::vector<DevCtx> devs;
  std::vector<std::unique_ptr<DeviceWorker>> workers; // [slot - 1], made on demand (renderOnDevices)
  std::mutex workerMutex;   // one multi-device frame at a time owns the workers (two scenes may render concurrently)
  std::mutex resourceMutex; // GPU resource destruction from sync threads (Gi.cpp:679-683)
};
extern Context g_ctx;

double nowMs();

constexpr int GI_C_OUT_OF_MEMORY_INTERNAL = -77; // DeviceBuffer::alloc: hipErrorOutOfMemory (never returned through the C ABI)
template <typename T>
struct DeviceBuffer {
  T* ptr = nullptr;
  size_t count = 0;
  int alloc(size_t n)
  {
    if (n <= count && ptr) return GI_C_OK;
    release();
    if (n == 0) n = 1;
    const hipError_t e = hipMalloc((void**)&ptr, n * sizeof(T));
    if (e != hipSuccess) {
      ptr = nullptr;
      // out of memory is an answer the render loop acts on (more batches, a smaller pool: gi_render.cpp allocatePathPlan), not yet an error
      if (e == hipErrorOutOfMemory) { (void)hipGetLastError(); t_lastError = "hipMalloc: out of memory"; return GI_C_OUT_OF_MEMORY_INTERNAL; }
      setError(std::string("hipMalloc: ") + hipGetErrorString(e)); return GI_C_ERROR;
    }
    count = n;
    return GI_C_OK;
  }
  size_t bytes() const { return ptr ? count * sizeof(T) : 0; }
  int upload(const std::vector<T>& v, hipStream_t s)
  {
    if (const int rc = alloc(v.size())) {
      if (rc == GI_C_OUT_OF_MEMORY_INTERNAL) setError("hipMalloc: out of device memory (" + std::to_string(v.size() * sizeof(T)) + " bytes)");
      return GI_C_ERROR;
    }
    if (!v.empty()) HIP_TRY(hipMemcpyAsync(ptr, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice, s));
    return GI_C_OK;
  }
  // Content-preserving grow (gi_build.cpp updateTopology): at least `n` elements, the first `count` kept.  A new block with 25 % slack, a device-to-device copy
  // on `s`; the old block goes into `old` and is freed by the caller once the stream is synchronised (the copy reads it).  Same answers as alloc.
  int grow(size_t n, hipStream_t s, std::vector<void*>& old)
  {
    if (n <= count && ptr) return GI_C_OK;
    T* fresh = nullptr;
    const size_t cap = n + n / 4u + 1u;
    const hipError_t e = hipMalloc((void**)&fresh, cap * sizeof(T));
    if (e != hipSuccess) {
      if (e == hipErrorOutOfMemory) { (void)hipGetLastError(); t_lastError = "hipMalloc: out of memory"; return GI_C_OUT_OF_MEMORY_INTERNAL; }
      setError(std::string("hipMalloc: ") + hipGetErrorString(e)); return GI_C_ERROR;
    }
    if (ptr && count && hipMemcpyAsync(fresh, ptr, count * sizeof(T), hipMemcpyDeviceToDevice, s) != hipSuccess) {
      (void)hipFree(fresh); setError("hipMemcpyAsync failed (device buffer grow)"); return GI_C_ERROR;
    }
    if (ptr) old.push_back(ptr);
    ptr = fresh; count = cap;
    return GI_C_OK;
  }
  void release() { if (ptr) { (void)hipFree(ptr); ptr = nullptr; count = 0; } }
};


// host-side arithmetic shared by the scene build, the light setters and the debug hooks (gi_c.cpp)
uint16_t f32ToF16(float f);
float f16ToF32(uint16_t h);
uint32_t packHalf2x16(float a, float b);
// (encodeDirection, decodeDirection, packVertex, packTriShade: gi_pack.h)
void turboColormap(float x, float* rgb);
float cutoutOpacity(const MaterialRec& m);
void deriveMaterialConstants(MaterialRec& m);

// ---------------------------------------------------------------------------------------------------------------
// handle types
// ---------------------------------------------------------------------------------------------------------------
// DIRTY_XFORM: only transforms of meshes that are part of the built scene changed -- the incremental path (updateTransforms) handles it unless a full
// rebuild is due anyway.  The reference keeps each mesh's BLAS and rebuilds the TLAS (Gi.cpp:1180-1202).
// DIRTY_MATERIALS without DIRTY_BVH: materials, assignments, texture bindings or primvars of a built scene changed -- updateMaterials rebuilds the small
// tables and patches TriRec::matFlags on the device; with DIRTY_BVH (or when that path declines) the scene is rebuilt.
enum DirtyFlags : uint32_t { DIRTY_BVH = 1u, DIRTY_FRAMEBUFFER = 2u, DIRTY_LIGHTS = 4u, DIRTY_MATERIALS = 8u, DIRTY_ALL = 0xfu, DIRTY_XFORM = 16u };

struct GiCTexture { GiCScene* scene; uint32_t width, height; std::vector<float> rgba; std::string cacheKey; uint32_t refs = 1;
    uint64_t serial = 0; /* unique per scene, never reused: names the image in a device's texel arrays (SceneDevice::dTexelSerial) */ };
struct GiCPrimvar { std::string name; int32_t type, interpolation; std::vector<float> data; };
struct GiCMaterial { GiCScene* scene; std::string name; GiCMaterialDesc desc; GiCTextureBinding tex[GI_C_TEX_SLOT_COUNT] = {};
    std::string primvarInput[GI_C_TEX_SLOT_COUNT];
                     float texXf[GI_C_TEX_SLOT_COUNT][6] = {}; bool hasTexXf[GI_C_TEX_SLOT_COUNT] = {}; /* giCSetMaterialTextureTransform */ };

struct GiCMesh {
  GiCScene* scene;
  std::string name;
  std::vector<GiCVertex> vertices;
  std::vector<GiCFace> faces;
  std::vector<int32_t> faceIds;
  int32_t id = 0;
  bool doubleSided = false, flipFacing = false, visible = true;
  uint32_t maxFaceId = 0;
  float transform[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
  std::vector<float> instanceTransforms; // 16 per instance; empty until giCSetMeshInstanceTransforms (as in Gi.cpp:620-638)
  std::vector<int32_t> instanceIds;
  std::vector<GiCPrimvar> primvars, instancerPrimvars;
  GiCMaterial* material = nullptr;
  bool xformDirty = false;  // transform / instance transforms changed since the last build or update ...
  std::vector<uint8_t> instDirty; // ... and which instances (empty: all of them)
  uint32_t builtInstances = 0xffffffffu; // instance count the built scene holds for this mesh (0xffffffff: not part of it)
  bool visToggled = false;  // giCSetMeshVisibility was called since the last syncSceneGeometry
  bool vertsEdited = false; // giCSetMeshVertices was called since the last syncSceneGeometry
  // giCSetMeshInstanceIds, or giCSetMeshInstanceTransforms with another count, was called on this mesh of the built scene since the last syncSceneGeometry
  bool instEdited = false;
  // giCDestroyMesh on a mesh of the built scene with topology updates wanted: the mesh left GiCScene::meshes and is kept (GiCScene::retiredMeshes) until the
  // next buildScene, because the resident scene still holds its records (MeshBuild::m).  Invisible for good
  bool retired = false;
};

// swap-remove dense store (GgpuDenseDataStore, src/ggpu/impl/DenseDataStore.cpp:35-93): the arrays stay dense so
// the *LightCount uniforms are the live counts.
template <typename Rec, typename Handle>
struct DenseStore {
  std::vector<Rec> recs;
  std::vector<Handle*> owners;
  uint32_t add(Handle* h, const Rec& r) { recs.push_back(r); owners.push_back(h); return (uint32_t)recs.size() - 1u; }
  void remove(uint32_t idx);
};

struct GiCSphereLight { GiCScene* scene; uint32_t index; };
struct GiCDistantLight { GiCScene* scene; uint32_t index; };
struct GiCRectLight { GiCScene* scene; uint32_t index; };
struct GiCDiskLight { GiCScene* scene; uint32_t index; };
struct GiCDomeLight { GiCScene* scene; std::string filePath; GiCTexture* texture = nullptr; bool ownsTexture = false; float rotation[4] = {0, 0, 0, 1};
    float baseEmission[3] = {1, 1, 1}; float diffuse = 1.0f, specular = 1.0f; };

template <typename Rec, typename Handle>
void DenseStore<Rec, Handle>::remove(uint32_t idx)
{
  uint32_t last = (uint32_t)recs.size() - 1u;
  if (idx != last) { recs[idx] = recs[last]; owners[idx] = owners[last]; owners[idx]->index = idx; }
  recs.pop_back(); owners.pop_back();
}

struct GiCRenderBuffer {
  uint32_t width, height, stride;
  size_t size;
  void* deviceMem = nullptr; // on the primary device
  void* hostMem = nullptr; // pinned (hipHostMalloc): the reference maps a HostVisible|HostCached buffer (Gi.cpp:2019-2031)
  bool deviceOnly = false;
  bool scratch = false; // internal stand-in that lives in the rendering device's own scratch memory (no replicas)
  std::vector<void*> replicaMem; // [slot - 1]: the same buffer on the other devices (multi-device renders), allocated on first use
  void* stageMem = nullptr; // pinned, rb->size: where the row shares of devices WITHOUT peer access to the primary pass through (allocated on first use)
  // the last giCRender that bound the buffer rendered the WHOLE frame on the primary device alone: deviceMem holds what hostMem holds (or would, deviceOnly).
  // giCRender sets it; row shares, multi-device renders and failed renders clear it (giCDenoise GI_C_DENOISE_SOURCE_AUTO reads such a copy in place)
  bool wholeFrame = false;
  bool hostOnly = false; // giCCreateHostRenderBuffer: hostMem is plain host memory, there is no deviceMem
  int32_t format = GI_C_FORMAT_FLOAT32_VEC4; // GiCRenderBufferFormat it was created with (stride alone does not tell Int32 from Float32)
  // GI_C_AOV_EXT_MOMENTS: the accumulation whose moments the buffer holds -- its epoch (GiCScene::accumEpoch: a process-wide number drawn anew whenever a
  // scene's sample offset restarts at 0, never 0 itself) and the sample offset the last successful giCRender that bound the buffer left that scene at.  A
  // progressive call of the SAME accumulation at exactly that offset continues the moments; any other starts them from zero (gi_moments.h)
  uint64_t momentsEpoch = 0, momentsNext = 0;
};
// gi_denoise_host.cpp: the library's denoiser scratch on the primary device (giCTerminate frees it)
void releaseDenoiseScratch();

// Sample look-ahead (GI_C_SCENE_OPTION_SAMPLE_LOOKAHEAD; gi_render.cpp planLookahead / serveFromWindow): the window one device holds in its per-sample buffer --
// the samples [firstOffset, firstOffset + calls * spp) of every pixel of its rows, traced as ONE batch by the window's first call -- and what it was traced
// with.  A call is served from it only if it would have traced the same samples: `key` is everything the path kernels were given, compared whole.
struct LookaheadKey {
  FrameUniforms U;          // the call's uniforms before the schedule adds its flags, without the fields derived from the sample offset (camera, settings,
                            // spp, image size, rows, light counts)
  SceneView view;           // the device arrays, the dome light, the background, the frame number
  uint64_t generation;      // GiCScene::generation: the contents of the device arrays
};
struct Lookahead {
  bool valid = false;       // `key`, `calls` ... describe what sampleBuf holds (a window of one call holds nothing: it is only the ramp's memory)
  uint32_t calls = 0, served = 0, firstOffset = 0;
  uint32_t pixelMajor = 0;  // layout of the window in sampleBuf: [pixel][calls * spp] or [calls * spp][pixel]
  LookaheadKey key{};
  uint32_t traced = 0;      // the last render on this device traced (1) or was served (0)
  uint64_t windowsTraced = 0, callsServed = 0, windowsDiscarded = 0, samplesUnused = 0;
  // the window is gone (an edit, another size, the buffer released or about to be written): calls nobody asked for are counted as thrown away
  void drop()
  {
    if (valid && served < calls) { windowsDiscarded++; samplesUnused += (uint64_t)(calls - served) * key.U.spp; }
    valid = false; calls = served = 0;
  }
};

// Everything a scene keeps in ONE device's memory: the scene arrays, the path pool, the queues, the per-render scratch.  GiCScene IS the primary
// device's (inheritance keeps the single-device code reading `s->dNodes`); multi-device renders add one replica per further device.
struct SceneDevice {
  uint32_t slot = 0; // index into g_ctx.devs
  DeviceBuffer<MeshRec> dMeshes; DeviceBuffer<float> dSceneData;
  std::vector<DeviceBuffer<float>*> dTexels; DeviceBuffer<TextureRec> dTextures; // device copies (rebuilt with the materials)
  std::vector<uint64_t> dTexelSerial; // GiCTexture::serial of the image dTexels[i] holds (gi_build.cpp uploadTexturesTo)
  DeviceBuffer<Node8> dNodes; DeviceBuffer<TriRec> dTris; DeviceBuffer<InstanceRec> dInstances;
  DeviceBuffer<FVertex> dVerts; DeviceBuffer<MaterialRec> dMaterials; DeviceBuffer<int32_t> dTriFaceId; DeviceBuffer<TriShade> dTriShade;
      DeviceBuffer<F4> dTriGeomNormal;
  DeviceBuffer<SphereLightRec> dSphere; DeviceBuffer<DistantLightRec> dDistant; DeviceBuffer<RectLightRec> dRect; DeviceBuffer<DiskLightRec> dDisk;
  DeviceBuffer<LightFrame> dRectFrames, dDiskFrames; // decoded tangents + normal per rect / disk light (uploadLights)
  DeviceBuffer<Node8> dTlasNodes, dBlasNodes; DeviceBuffer<uint32_t> dTlasItems, dFlatOfOrig; DeviceBuffer<BlasTri> dBlasTris; DeviceBuffer<InstTrav> dInstTrav;
  TlasBuildWorkspace tlasWorkspace; // the device TLAS builder's slab (primary device only; GI_C_SCENE_OPTION_TLAS_DEVICE_BUILD): grows geometrically, released with the scene
  // path state
  DeviceBuffer<Slot> slots;
  DeviceBuffer<float> media; // per-slot medium stack + walkSegmentPdf (mediumStackSize > 0)
  DeviceBuffer<F4> scratchColor; DeviceBuffer<unsigned long long> neeKey; // NEE / Bounces AOVs bound without / with the colour AOV
  DeviceBuffer<uint32_t> pathSegments;                                    // ClockCycles AOV (cost proxy)
  // per-sample colours of the current batch (rgb, -): [pixel][sample] under the pixel-major work order of the stage kernels, [sample][pixel] otherwise
  // (gi_queues.h sample_record)
  DeviceBuffer<F4> sampleBuf;
  Lookahead lookahead;           // the look-ahead window sampleBuf holds between calls
  DeviceBuffer<F4> accum;        // per-pixel running sum across batches
  DeviceBuffer<uint32_t> qSlot[Q_COUNT]; // NSHARD segments of queueCap records each
  DeviceBuffer<F4> qA[Q_COUNT], qB[Q_COUNT], qC[Q_COUNT];
  DeviceBuffer<FreshRec> qFresh[2]; // beside TRACE_A / TRACE_B: (rng, work item) of camera rays whose Slot is written only when they hit (FLAG_DEFER_SLOT)
  uint32_t queueCap = 0;
  DeviceBuffer<Counters> dCounters;
  Counters* hCounters = nullptr; // pinned
  uint64_t memTotalMb = 0;       // the device's memory (hipMemGetInfo, asked once): sizes the default sample-buffer budget
  // drain test of the bounce loop: iteration it reads the queue sizes of iteration it - POLL_LAG (gi_render.cpp runWavefrontBatch)
  static constexpr uint32_t POLL_RING = 4, POLL_LAG = 2;
  PaddedCounter* hPoll = nullptr; hipEvent_t pollEvent[POLL_RING] = {}; // pinned ring of queue-size snapshots + their completion events
  // two-stream batches: k_shade(i) done (the second stream's shadow launch waits for it) / shadow launch (i) done (k_raygen(i + 1) waits for it)
  hipEvent_t evShade = nullptr, evShadow = nullptr;
  GiCRenderStats stats{};
  uint64_t pathWalkStats[18] = {}; // giCDebugPathWalkStats: k_path's trips and walk-step tables of the last render (counting builds; fillStats)
  uint64_t pathLobeStats[9] = {};  // giCDebugPathLobeStats: Counters::lobeStats of the last render (counting builds; fillStats)
  uint64_t pathRingStats[5] = {};  // giCDebugPathRingStats: Counters::ringStats of the last render (counting builds; fillStats)
  // giCDebugTraversalStackHigh: Counters::stackHigh of the last render, the stack rows of the traversal variant it ran and the scratch-spill entries its
  // walks used at most (counting builds; fillStats)
  uint32_t traversalStackHigh[4] = {};
  std::vector<hipEvent_t> eventPool;
  // the resizable path state (what the memory plan of a render sizes: slots, media, sampleBuf, the queues) -- the ONE list of these buffers
  template <typename Fn> void forEachPathBuffer(Fn&& fn)
  {
    fn(slots); fn(media); fn(sampleBuf);
    for (uint32_t q = 0; q < Q_COUNT; q++) { fn(qSlot[q]); fn(qA[q]); fn(qB[q]); fn(qC[q]); }
    fn(qFresh[0]); fn(qFresh[1]);
  }
  uint64_t pathStateBytes() { uint64_t n = 0; forEachPathBuffer([&](auto& b) { n += b.bytes(); }); return n; }
  void releasePathState() { forEachPathBuffer([](auto& b) { b.release(); }); queueCap = 0; lookahead.drop(); }
  void releaseAll();
};

// The scene as host arrays (built once per scene change, kept for incremental transform updates) ...
struct TwoLevelHost { std::vector<Node8> tlasNodes, blasNodes; std::vector<uint32_t> tlasItems; std::vector<BlasTri> blasTris; std::vector<InstTrav> instTrav;
    // transform updates in place (gi_build.cpp updateTransformsTwoLevel): the padded world box of every instance (6 floats each: what the TLAS is built
    // over), the first BLAS triangle of every mesh by meshIdx, and the depths the layout's stack rule reads
    std::vector<float> instBoxes; std::vector<uint32_t> meshBlasTri; uint32_t tlasDepth = 0, blasDepth = 0;
    // vertex updates in place (gi_build.cpp updateVerticesTwoLevel): the first BLAS node of every mesh by meshIdx and the first node of every level of its
    // BLAS relative to that, then the BLAS's node count (Bvh8::levelStart; empty for a mesh without instances).  After such an update blasNodes keeps the
    // build's TOPOLOGY (imask, meta, childBase, triBase) while its planes (p, e, qlo, qhi) go stale: nothing reads them before the next buildScene -- the
    // device refits its own copy, and giCDebugSceneBlasCheck runs the host refit over a copy of the topology
    std::vector<uint32_t> meshBlasNode; std::vector<std::vector<uint32_t>> meshBlasLevels;
    // GI_C_SCENE_OPTION_TLAS_DEVICE_BUILD: the device builder (gi_tlas_build.hip) made the resident TLAS, under this depth budget -- an edit in place sets both,
    // a scene build clears them; giCDebugSceneTlasCheck makes its comparison TLAS with the same builder
    bool tlasDeviceBuilt = false; uint32_t tlasBuildBudget = 0;
    // GI_C_SCENE_OPTION_BLAS_DEVICE_BUILD: by meshIdx, the depth budget under which the device builder (gi_blas_build.hip) made the mesh's resident BLAS; 0 (or no
    // entry): the host builder made it.  Whatever makes a BLAS anew for comparison (buildTwoLevel under giCDebugSceneTlasCheck / giCDebugSceneBlasCheck) runs
    // the host form of the builder that made the resident one, under this budget
    std::vector<uint32_t> meshBlasBudget; };
struct MeshBuild { const GiCMesh* m; uint32_t vertexOffset, matFlags, instFirst, instCount, triFirst; uint32_t meshIdx; std::vector<int32_t> faceIdAov;
    uint32_t shadeBase = 0;
    // the InstanceRec of every live instance, inst[instInMesh]: instFirst + instInMesh (and triangles at triFirst + instInMesh * faces) as the build leaves
    // them; an instance update (gi_build.cpp updateTopology) appends records at the end of the array and retires others, which stay resident (retiredInst)
    std::vector<uint32_t> inst; uint32_t retiredInst = 0;
    // a two-level scene without the flat tree under instancer edits in place (gi_build.cpp updateInstancesTwoLevel): the first flat record of every live
    // instance, instTri[instInMesh] -- a mesh's records are no longer one run once an instance sits in a reused slot --, and the slots its retired instances
    // left (InstanceRec / InstTrav index and first flat record, ascending by index; retiredInst counts them): out of the TLAS, edges zero, no id-table word,
    // as the instances of a hidden mesh, until a later grow of the SAME mesh takes them
    struct FreeSlot { uint32_t inst, tri; };
    std::vector<uint32_t> instTri; std::vector<FreeSlot> freeSlots;
    void numberInstances() { inst.resize(instCount); instTri.resize(instCount);
        for (uint32_t ii = 0; ii < instCount; ii++) { inst[ii] = instFirst + ii; instTri[ii] = triFirst + ii * (uint32_t)m->faces.size(); } }
    // incremental visibility updates (gi_build.cpp updateVisibility): the mesh is part of the resident scene but hidden; the scene-order id of its first
    // triangle as the resident records hold it (triFirst until a mesh in front of it is hidden; triFirst stays the POSITION of a partitioned scene's ranges)
    bool hidden = false; uint32_t idBase = 0; };
// One flattened mesh instance of a PARTITIONED scene (after the first transform edit): its own subtree in its own node range, its triangles in its own
// (scene-order) range, joined by a top tree over the subtree roots (bvh8.h buildTopBvh8).  Moving it rebuilds these ranges and the top tree only.
struct InstPart { uint32_t meshBuild, instInMesh; uint32_t triFirst, nf; uint32_t nodeOff, nodeCount, nodeCap, depth; float box[6];
    // vertex updates (gi_build.cpp updateVertices): triangles the subtree holds (nf unless some were inactive when it was built), and the first node of every
    // level of the subtree relative to nodeOff, then nodeCount (Bvh8::levelStart)
    uint32_t activeTris = 0; std::vector<uint32_t> levelStart;
    // its instance was retired by an instance update: the ranges stay resident and out of the top tree, like those of a hidden mesh, for good
    bool retired = false; };
struct SceneHost {
  std::vector<FVertex> verts; std::vector<InstanceRec> instances; std::vector<MaterialRec> mats; std::vector<MeshRec> meshRecs; std::vector<float> sceneData;
  Bvh8 bvh; std::vector<int32_t> triFaceId; std::vector<uint32_t> flatOfOrig; TwoLevelHost two;
  std::vector<MeshBuild> meshBuilds;
  std::vector<F4> triGeomNormal; // LDS-resident scenes: per flattened triangle (gi_build.cpp)
  std::vector<TriShade> triShade; bool shadePacked = false; // one-line shading records per mesh triangle (scenes beyond LDS): TriRec::vi[0] indexes them
  bool partitioned = false; std::vector<InstPart> parts; uint32_t topCap = 0; // partitioned layout: nodes [0, topCap) = top tree, then the parts' ranges
  // the device builder made the tree: it exists only in device memory (dNodes / dTris / dTriFaceId); `bvh` keeps its sizes (maxDepth, activeTris) alone
  bool deviceBuilt = false;
  // a vertex update refitted a flat host-built tree in device memory: the host copies of its nodes, triangles and face ids were dropped (they would be
  // stale), and the scene is treated as a device-built one is -- the re-layout of the first transform edit makes them anew
  bool hostTreeDropped = false;
  // a mesh adopted the records of the one it replaced (updateTopology, GI_C_SCENE_OPTION_RESYNC_REFITS): the order of meshBuilds is no longer the scene's, and
  // scene-order ids are accumulated over GiCScene::meshes (gi_build.cpp sceneOrder)
  bool reordered = false;
  // a two-level scene built without the flat tree (GI_C_SCENE_OPTION_TLAS_ONLY): bvh.nodes / levelStart are empty and no device holds flat nodes
  // (GiCScene::nodeCount is 0); bvh.tris are the flat records in scene order (origId == index, flatOfOrig the identity); the scene bounds come from the
  // instance boxes (gi_tlas.h tlas_scene_bounds); k_aov2 makes the AOVs
  bool treeless = false;
};

enum : uint32_t { UPDATE_FULL = 0, UPDATE_TRANSFORM = 1, UPDATE_MATERIAL = 2, UPDATE_VISIBILITY = 3, UPDATE_VERTEX = 4, UPDATE_TOPOLOGY = 5, UPDATE_TLAS = 6, UPDATE_BLAS = 7, UPDATE_TLAS_VISIBILITY = 8, UPDATE_TLAS_TOPOLOGY = 9 }; // GiCScene::updateCounts
struct GiCScene : SceneDevice {
  std::mutex mutex;
  uint32_t dirty = DIRTY_ALL;
  std::vector<GiCMesh*> meshes;       // creation order (deterministic triangle ids; the reference uses an unordered_set)
  std::vector<GiCMaterial*> materials;
  std::vector<GiCTexture*> textures;  // creation order
  uint64_t nextTextureSerial = 1;
  DenseStore<SphereLightRec, GiCSphereLight> sphereLights;
  DenseStore<DistantLightRec, GiCDistantLight> distantLights;
  DenseStore<RectLightRec, GiCRectLight> rectLights;
  DenseStore<DiskLightRec, GiCDiskLight> diskLights;
  // sphere / distant / rect / disk lights the device arrays hold (uploadLights: the stores' records minus the unusable ones)
  uint32_t lightCounts[4] = {0, 0, 0, 0};
  uint32_t sampleOffset = 0;
  uint64_t accumEpoch = 0; // which accumulation sampleOffset counts: nextAccumEpoch() wherever sampleOffset restarts at 0 (giCRender); 0 = none yet
  bool haveOldParams = false;
  GiCCameraDesc oldCamera{};
  GiCRenderSettings oldSettings{};
  uint8_t oldClear[GI_C_MAX_AOV_COMP_SIZE] = {0};
  uint32_t oldRowBegin = 0, oldRowEnd = 0, oldRowStride = 1;
  GiCDomeLight* oldDome = nullptr;
  float oldDomeEmission[3] = {0, 0, 0};
  // the scene as built (the same on every device)
  uint32_t nodeCount = 0, triCount = 0, bvhDepth = 0;
  // the flat tree's root bounds (nodeBounds + a relative pad) -- on a scene without the flat tree the union of the instance boxes under the same pad
  // (gi_tlas.h tlas_scene_bounds) --, for FLAG_BOUNDS_RETIRE
  float bounds[6] = {0, 0, 0, 0, 0, 0}; bool boundsValid = false;
  int optBvhBuild = 0; // GI_C_SCENE_OPTION_BVH_BUILD: 1 = the device builder for flat-layout scenes beyond LDS (gi_bvh_build.hip)
  bool twoLevel = false; int optTwoLevel = -1; // 1: build and use the two-level layout (scenes beyond LDS); otherwise the flat one
  bool hasCutouts = false;
  bool shadePacked = false; // the built scene carries TriShade records (beyond LDS)
  uint32_t classMask = 0; // material classes that own at least one triangle (one k_shade launch per class)
  uint32_t classTextured = 0; // classes with at least one textured material in use (k_shade<class, TEXTURED>)
  // the same per SHADE class (gi_types.h: the HIT queues of the wavefront pipeline; classMask / classTextured pick the fused kernels)
  uint32_t shadeClassMask = 0, shadeClassTextured = 0;
  // what every class-1 material in use has in common (gi_types.h UPS_NOCOAT; 0 when the class is textured or absent): the fused kernel's plain
  // UsdPreviewSurface variant.  upsPlainLaunched: the traits the last render's k_path launch was compiled for (0: the general text, or no fused launch)
  uint32_t upsTraits = 0, upsPlainLaunched = 0;
  uint32_t nodeCookLaunched = 0; // giCDebugSceneNodeCook: 1 when the last render's k_path launch staged cooked nodes (gi_node_cook.h; launchPath's rule)
  std::unique_ptr<SceneHost> host; // the scene as host arrays, kept for incremental transform updates
  std::vector<std::unique_ptr<SceneDevice>> replicas; // devices 1 .. N-1 (created with the first build when the library runs on several devices)
  // options + stats
  bool countTraversal = false, kernelTimers = false;
  uint32_t kernelTimerStride = 1;
  uint64_t optPoolSlots = 0, optSampleBufferMb = 0; // 0 = default
  // -1 (default), 1, 2: LDS-resident scenes run the fused persistent kernel k_path; 0 = always the wavefront stage kernels
  int32_t optFusedPath = -1;
  int32_t optTraceDyn = -1; // k_trace_dyn refill threshold N in 1..64; -1 or 0 = default
  // Visiting order of shadow walks (k_trace_dyn<any>; any order gives the same image): -1 = not chosen yet -- launches alternate between near-to-far (0) and
  // slot order (1) and the frame's node-visit counts are added up below; once both orders have walked enough rays the cheaper one is kept until the tree is
  // rebuilt.
  std::atomic<int32_t> shadowOrder{-1};
      /* read by every device worker at the start of its render, written by the primary at the end of its own */ uint64_t shadowOrderRays[2] = {0, 0},
      shadowOrderSteps[2] = {0, 0};
  int32_t optDevices = 0;   // 0 = every device the library was initialised on; N = at most N of them
  // devices the previous giCRender used: progressive accumulation blends against each device's own buffer, so a change restarts it
  uint32_t lastRenderDevices = 0;
  int32_t optLookahead = 0; // GI_C_SCENE_OPTION_SAMPLE_LOOKAHEAD: calls a look-ahead window may hold; 0 = off
  // contents of the device arrays: bumped by every scene build, transform update, material update and light upload --
  // a look-ahead window traced under another generation is not served from
  uint64_t generation = 0;
  // syncSceneGeometry, by UPDATE_*: full builds and incremental updates (giCDebugSceneUpdateCounts: the first three; giCDebugSceneVisibilityUpdateCount,
  // giCDebugSceneVertexUpdateCount, giCDebugSceneTopologyUpdateCount, giCDebugSceneTlasUpdateCount, giCDebugSceneBlasUpdateCount, giCDebugSceneTlasVisibilityUpdateCount,
  // giCDebugSceneTlasTopologyUpdateCount)
  uint64_t updateCounts[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  int32_t optVisibilityUpdates = 0; // GI_C_SCENE_OPTION_VISIBILITY_UPDATES: 1 = visibility edits are applied to the resident scene (updateVisibility)
  int32_t optVertexUpdates = 0; // GI_C_SCENE_OPTION_VERTEX_UPDATES: 1 = vertex edits refit the resident tree (updateVertices)
  // DIRTY_BVH was raised by something other than giCSetMeshVisibility / giCSetMeshVertices since the last syncSceneGeometry (raiseRebuild): the rebuild is due
  // whatever was toggled or deformed
  bool rebuildDue = true;
  int32_t optTopologyUpdates = 0; // GI_C_SCENE_OPTION_TOPOLOGY_UPDATES: 1 = meshes are created and destroyed in the resident scene (updateTopology)
  // DIRTY_BVH was raised by giCCreateMesh, giCDestroyMesh or a setter on a mesh that is not part of the built scene (raiseTopology): syncSceneGeometry may
  // answer with updateTopology; without the option it turns this into rebuildDue
  bool topologyDue = false;
  // GI_C_SCENE_OPTION_RESYNC_REFITS: 1 = a destroyed mesh and a created one with the same faces become a vertex edit of the resident records (updateTopology
  // adoptResyncs; read only with topology and vertex updates wanted); meshes adopted since the scene was created (giCDebugSceneResyncCount)
  int32_t optResyncRefits = 0; uint64_t resyncCount = 0;
  // GI_C_SCENE_OPTION_INSTANCE_UPDATES: 1 = instance ids and counts of built meshes are edited in the resident scene (updateTopology; read only with
  // topology updates wanted); giCDebugSceneInstanceUpdateCount: syncs that applied such an edit, instances appended, of those cloned, instances retired
  int32_t optInstanceUpdates = 0; uint64_t instanceCounts[4] = {0, 0, 0, 0};
  // DIRTY_BVH was raised by giCSetMeshInstanceIds or a count change of giCSetMeshInstanceTransforms on a mesh of the built scene (raiseInstances):
  // syncSceneGeometry lets updateTopology answer it; without the option it turns this into rebuildDue
  bool instancesDue = false;
  // GI_C_SCENE_OPTION_TLAS_UPDATES: 1 = transform edits of a two-level scene are applied to the resident scene (updateTransformsTwoLevel)
  int32_t optTlasUpdates = 0;
  // GI_C_SCENE_OPTION_BLAS_UPDATES: 1 = vertex edits of a two-level scene are applied to the resident scene (updateVerticesTwoLevel; read only with vertex
  // updates wanted)
  int32_t optBlasUpdates = 0;
  // GI_C_SCENE_OPTION_TLAS_VISIBILITY: 1 = visibility edits of a two-level scene are applied to the resident scene (updateVisibilityTwoLevel; read only with
  // visibility updates wanted)
  int32_t optTlasVisibility = 0;
  // GI_C_SCENE_OPTION_TLAS_ONLY: 1 = a scene that takes the two-level layout is built without the flat tree (buildScene; SceneHost::treeless); read at the
  // build only, and only with the two-level layout wanted
  int32_t optTlasOnly = 0;
  // GI_C_SCENE_OPTION_TLAS_TOPOLOGY: 1 = meshes are created and destroyed in a resident two-level scene that was built without the flat tree
  // (updateTopologyTwoLevel; read only with topology updates wanted)
  int32_t optTlasTopology = 0;
  // GI_C_SCENE_OPTION_TLAS_INSTANCES: 1 = instance ids and counts of built meshes are edited in a resident two-level scene that was built without the flat
  // tree (updateInstancesTwoLevel; read only with topology, instance and two-level topology updates wanted); giCDebugSceneTlasInstanceUpdateStats: syncs
  // that applied such an edit, instances appended, of those into reused slots, instances retired
  int32_t optTlasInstances = 0; uint64_t tlasInstanceCounts[4] = {0, 0, 0, 0};
  // GI_C_SCENE_OPTION_TLAS_DEVICE_BUILD: 1 = the edits in place of a two-level scene build their TLAS on the primary device (gi_build.cpp buildEditTlas);
  // giCDebugSceneTlasBuildStats: device builds, fallbacks (too deep, memory, error, under tlas_device_min), the last device build's figures
  int32_t optTlasDeviceBuild = 0; uint64_t tlasBuildStats[16] = {};
  // GI_C_SCENE_OPTION_BLAS_DEVICE_BUILD: 1 = the BLAS of a mesh of blas_device_min .. blas_device_max faces is built on the primary device (gi_build.cpp
  // makeMeshBlas: the scene build's buildTwoLevel and updateTopologyTwoLevel); giCDebugSceneBlasBuildStats: device builds, fallbacks (under the minimum, over
  // the maximum, too deep, memory, error), the last device build's figures
  int32_t optBlasDeviceBuild = 0; uint64_t blasBuildStats[16] = {};
  // GI_C_SCENE_OPTION_TLAS_COMPACTION: 1 = the ranges options 20 and 21 retired are compacted on the device when they outgrow tlas_compact_percent (gi_build.cpp
  // compactTwoLevel: read only where updateTopologyTwoLevel / updateInstancesTwoLevel is about to apply an edit); giCDebugSceneCompactionCount: compactions
  // applied, records moved, bytes released on the primary device, compactions that declined
  int32_t optTlasCompaction = 0; uint64_t compactionStats[4] = {0, 0, 0, 0};
  // GI_C_SCENE_OPTION_LEAF_LIFT: -1 = the default (LEAF_LIFT_DEFAULT, gi_kernels.h), 0 / 1 = the flat tree of a small scene stays the builder's / goes through
  // liftLeafSlots (leaf_lift.cpp; gi_build.cpp buildScene); giCDebugSceneLeafLift: the leaf slots the last scene build moved
  int32_t optLeafLift = -1; uint32_t liftedLeafSlots = 0;
  std::vector<GiCMesh*> retiredMeshes; // destroyed meshes the resident scene still refers to (GiCMesh::retired): freed by buildScene and with the scene
  ~GiCScene() { for (GiCMesh* m : retiredMeshes) delete m; }
};
// every geometry-side edit but a visibility toggle, a vertex edit and the topology edits below
inline void raiseRebuild(GiCScene* s) { s->dirty |= DIRTY_BVH | DIRTY_FRAMEBUFFER; s->rebuildDue = true; }
// a mesh created or destroyed, or a setter on a mesh that is not part of the built scene: the same flags
inline void raiseTopology(GiCScene* s) { s->dirty |= DIRTY_BVH | DIRTY_FRAMEBUFFER; s->topologyDue = true; }
// instance ids or the instance count of a mesh of the built scene changed: the same flags
inline void raiseInstances(GiCMesh* m) { m->instEdited = true; m->scene->dirty |= DIRTY_BVH | DIRTY_FRAMEBUFFER; m->scene->instancesDue = true; }


// ---------------------------------------------------------------------------------------------------------------
// functions the translation units share
// ---------------------------------------------------------------------------------------------------------------
// gi_textures.cpp asset reader -> loader hook -> in-library decoders
extern "C++" bool loadImage(const char* path, bool srgbToLinear, bool keepHdr, uint32_t& w, uint32_t& h, std::vector<float>& px);
// gi_lights.cpp
int uploadLights(GiCScene* s);
// gi_build.cpp
uint32_t shadeClassOf(const MaterialRec& m);                 // shade class (k_shade variant) of a derived material record
uint32_t upsTraitsOf(const MaterialRec& m);                  // UPS_* traits of one derived class-1 record (the scene's: their intersection, deriveSceneClasses)
uint32_t sceneDeviceCount(const GiCScene* s);                // devices a render of this scene may use
SceneDevice& sceneDevice(GiCScene* s, uint32_t slot);
bool usableVertexPositions(const GiCVertex* v, size_t count);  // every position finite and within 1e18 (bvh8.h "Inactive items")
void nodeBounds(const Node8& n, float box[6]);               // dequantised bounds of a node's children (+ an ulp-scale pad)
bool instanceUpdatesWanted(const GiCScene* s);               // GI_C_SCENE_OPTION_INSTANCE_UPDATES / GATLING_OPTIONS=instance_updates (with topology updates wanted)
bool tlasUpdatesWanted(const GiCScene* s);                   // GI_C_SCENE_OPTION_TLAS_UPDATES / GATLING_OPTIONS=tlas_updates
bool blasUpdatesWanted(const GiCScene* s);                   // GI_C_SCENE_OPTION_BLAS_UPDATES / GATLING_OPTIONS=blas_updates
bool leafLiftWanted(const GiCScene* s);                      // GI_C_SCENE_OPTION_LEAF_LIFT / GATLING_OPTIONS=leaf_lift (read at the scene build)
bool tlasOnlyWanted(const GiCScene* s);                   // GI_C_SCENE_OPTION_TLAS_ONLY / GATLING_OPTIONS=tlas_only (read at the build, with the two-level layout wanted)
bool tlasVisibilityWanted(const GiCScene* s);               // GI_C_SCENE_OPTION_TLAS_VISIBILITY / GATLING_OPTIONS=tlas_visibility (with visibility updates wanted)
bool topologyUpdatesWanted(const GiCScene* s);               // GI_C_SCENE_OPTION_TOPOLOGY_UPDATES / GATLING_OPTIONS=topology_updates
bool tlasTopologyWanted(const GiCScene* s);                  // GI_C_SCENE_OPTION_TLAS_TOPOLOGY / GATLING_OPTIONS=tlas_topology (with topology updates wanted)
bool tlasDeviceBuildWanted(const GiCScene* s);               // GI_C_SCENE_OPTION_TLAS_DEVICE_BUILD / GATLING_OPTIONS=tlas_device_build (read where options 16 - 18, 20, 21 apply an edit)
bool blasDeviceBuildWanted(const GiCScene* s);               // GI_C_SCENE_OPTION_BLAS_DEVICE_BUILD / GATLING_OPTIONS=blas_device_build (read where a BLAS is built)
// the host builder's BLAS of one mesh: padded face boxes, buildBvh8Boxes; mlo / mhi: the union of the usable faces' boxes
void buildMeshBlas(const GiCVertex* vertices, const GiCFace* faces, size_t nf, Bvh8& b, std::vector<uint32_t>& order, float mlo[3], float mhi[3]);
BlasTri makeBlasTri(const GiCVertex* vertices, const GiCFace* faces, uint32_t f); // its record of face f
bool tlasCompactionWanted(const GiCScene* s);                // GI_C_SCENE_OPTION_TLAS_COMPACTION / GATLING_OPTIONS=tlas_compaction (read where options 20 and 21 apply an edit)
bool tlasInstancesWanted(const GiCScene* s);                 // GI_C_SCENE_OPTION_TLAS_INSTANCES / GATLING_OPTIONS=tlas_instances (with options 13, 15 and 20 wanted)
int syncSceneGeometry(GiCScene* s);                          // brings the device scene up to date with the host-side edits (incremental or full build)
// dirty flags of a material-side edit: DIRTY_MATERIALS alone once the scene / the mesh is part of a built scene (the incremental path), else with DIRTY_BVH
inline uint32_t materialEditFlags(bool built) { return DIRTY_MATERIALS | DIRTY_FRAMEBUFFER | (built ? 0u : (uint32_t)DIRTY_BVH); }
// gi_render.cpp
SceneView makeView(GiCScene* s, SceneDevice& D);
SceneView makeView(GiCScene* s);
uint32_t traceDynRefill(const GiCScene* s);
int ensurePathState(SceneDevice* s, size_t slots, uint32_t gridA, uint32_t gridB);
QueueSet makeQueueSet(SceneDevice* s);


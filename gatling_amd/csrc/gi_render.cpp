// gi_render.cpp -- giCRender (Gi.cpp:1989-2524): validation and dirty handling (giCRenderImpl), the rows dealt to several devices (renderOnDevices), and one
// device's render (renderOnDevice) as a sequence of phases: bindAovs, makeUniforms, makeFrameView, planLookahead, then either serveFromWindow or the colour
// pass (traceColour: planPathMemory / allocatePathPlan, scheduleFrame / scheduleBatch, runFusedBatch | runZeroBounceBatch | runWavefrontBatch (the bounce
// loop), finishPathAovs), runAovPass, readBackAndWait, the statistics
// (one of the translation units gi_c.cpp was split into in round 6; shared declarations: gi_host.h)
#include "gi_host.h"
#include "gi_miss_rect.h"
#include "gi_moments.h"

bool settingsEqual(const GiCRenderSettings& a, const GiCRenderSettings& b) { return memcmp(&a, &b, sizeof(a)) == 0; }

SceneView makeView(GiCScene* s, SceneDevice& D)
{
  SceneView v{};
  v.textures = D.dTextures.ptr; v.meshes = D.dMeshes.ptr; v.sceneData = D.dSceneData.ptr;
  v.nodes = D.dNodes.ptr; v.tris = D.dTris.ptr; v.instances = D.dInstances.ptr;
  v.verts = D.dVerts.ptr; v.triShade = D.dTriShade.ptr; v.triGeomNormal = D.dTriGeomNormal.ptr; v.shadePacked = s->shadePacked ? 1u : 0u;
      v.materials = D.dMaterials.ptr;
      v.sphereLights = D.dSphere.ptr; v.distantLights = D.dDistant.ptr;
  v.tlasNodes = D.dTlasNodes.ptr; v.tlasItems = D.dTlasItems.ptr; v.blasNodes = D.dBlasNodes.ptr; v.blasTris = D.dBlasTris.ptr; v.instTrav = D.dInstTrav.ptr;
      v.flatOfOrig = D.dFlatOfOrig.ptr; v.twoLevel = s->twoLevel ? 1u : 0u;
  v.rectLights = D.dRect.ptr; v.diskLights = D.dDisk.ptr; v.rectFrames = D.dRectFrames.ptr; v.diskFrames = D.dDiskFrames.ptr; v.triFaceId = D.dTriFaceId.ptr;
      v.nodeCount = s->nodeCount; v.triCount = s->triCount;
      v.bvhDepth = s->bvhDepth; v.hasCutouts = s->hasCutouts ? 1u : 0u;
  return v;
}
SceneView makeView(GiCScene* s) { return makeView(s, *s); }

// k_trace_dyn refill threshold, 1..64 (0 or below: the default, 8)
uint32_t traceDynRefill(const GiCScene* s)
{
  long r = s->optTraceDyn;
  if (optionSet("trace_dyn")) r = optionValue("trace_dyn", 8);
  return r > 0 ? (uint32_t)std::min(64L, r) : 8u;
}

uint32_t shardCapacity(size_t slots, uint32_t gridA, uint32_t gridB)
{
  // A queue holds at most `slots` records in total (a path sits in one queue at a time), but it is fed by SEVERAL launches before it is consumed -- TRACE[par]
  // by k_raygen and one k_shade per material class, REGEN by k_trace / k_route, every k_shade and k_raygen (maxBounces == 0) -- and every launch starts dealing
  // its blocks at shard 0. A launch of G blocks that appends n records gives one shard at most ceil(G/NSHARD) * ceil(n/(256 G)) * 256 <= n/NSHARD + n/G + 32 G
  // + 256 of them; summed over P producers with sum(n) <= slots this is slots/NSHARD + P * (slots/Gmin + 32 Gmax + 256). block_append also raises
  // Counters::overflow if a shard ever runs past its capacity (giCRender then fails instead of returning a corrupt image). (a producer that appends I records
  // per thread and trip -- k_route: ROUTE_ITEMS, k_raygen: RAYGEN_ITEMS, gi_kernels.h APPEND_ITEMS_MAX -- deals 256 * I records per block and trip: the slack
  // term is 32 * I * G + 256 * I)
  const size_t P = 2 + MAT_CLASS_COUNT, I = APPEND_ITEMS_MAX;
  const size_t gMin = std::max<size_t>(1, std::min(gridA, gridB)), gMax = std::max<size_t>(1, std::max(gridA, gridB));
  const size_t cap = (slots + NSHARD - 1) / NSHARD + P * ((slots + gMin - 1) / gMin + 32 * I * gMax + 256 * I);
  return (uint32_t)std::min<size_t>(cap, slots + 256); // a shard can never hold more than the pool
}

int ensurePathState(SceneDevice* s, size_t slots, uint32_t gridA, uint32_t gridB)
{
  const uint32_t cap = shardCapacity(slots, gridA, gridB);
  int rc;
#define GI_ALLOC(x) do { rc = (x); if (rc != GI_C_OK) return rc; } while (0) /* GI_C_ERROR, or GI_C_OUT_OF_MEMORY_INTERNAL for the caller's fallback */
  GI_ALLOC(s->slots.alloc(slots));
  if (!s->dCounters.ptr) { GI_ALLOC(s->dCounters.alloc(1)); HIP_TRY(hipMemset(s->dCounters.ptr, 0, sizeof(Counters))); } // AOV-only renders never run k_init
  if (cap > s->queueCap) {
    const size_t n = (size_t)cap * NSHARD;
    for (uint32_t q = 0; q < Q_COUNT; q++) {
      const bool hasRecord = (q == Q_TRACE_A || q == Q_TRACE_B || q == Q_SHADOW); // (the HIT queues hold indices into the TRACE queue: gi_queues.h)
      GI_ALLOC(s->qSlot[q].alloc(n));
      if (hasRecord) { GI_ALLOC(s->qA[q].alloc(n)); GI_ALLOC(s->qB[q].alloc(n)); }
      if (q == Q_SHADOW) GI_ALLOC(s->qC[q].alloc(n));
      if (q == Q_TRACE_A || q == Q_TRACE_B) GI_ALLOC(s->qFresh[q - Q_TRACE_A].alloc(n));
    }
    s->queueCap = cap;
  }
#undef GI_ALLOC
  if (!s->hCounters) HIP_TRY(hipHostMalloc((void**)&s->hCounters, sizeof(Counters), hipHostMallocDefault));
  if (!s->hPoll) {
    HIP_TRY(hipHostMalloc((void**)&s->hPoll, sizeof(PaddedCounter) * Q_COUNT * NSHARD * SceneDevice::POLL_RING, hipHostMallocDefault));
    for (hipEvent_t& e : s->pollEvent) HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
  }
  return GI_C_OK;
}

QueueSet makeQueueSet(SceneDevice* s)
{
  QueueSet qs{};
  for (uint32_t q = 0; q < Q_COUNT; q++) { qs.slot[q] = s->qSlot[q].ptr; qs.a[q] = s->qA[q].ptr; qs.b[q] = s->qB[q].ptr; qs.c[q] = s->qC[q].ptr; }
  qs.fresh[0] = s->qFresh[0].ptr; qs.fresh[1] = s->qFresh[1].ptr;
  qs.cap = s->queueCap;
  return qs;
}

hipEvent_t poolEvent(SceneDevice* s, size_t idx)
{
  while (s->eventPool.size() <= idx) { hipEvent_t e; (void)hipEventCreate(&e); s->eventPool.push_back(e); }
  return s->eventPool[idx];
}

// ---------------------------------------------------------------------------------------------------------------
// giCRender
// ---------------------------------------------------------------------------------------------------------------
// C++ exceptions (allocation failure on a huge scene) must not cross the C ABI: the heavy entry points run through a guarded wrapper
static int giCRenderImpl(const GiCRenderParams* params);
extern "C" int giCRender(const GiCRenderParams* params)
{
  try { return giCRenderImpl(params); }
  catch (const std::exception& e) { setError(std::string("giCRender: ") + e.what()); return GI_C_ERROR; }
}
// One device's part of a render: the rows rowBegin, rowBegin + rowStride, ... < rowEnd of the frame, on device D.slot with D's copy of the scene.  Called
// under the scene mutex, after the dirty handling; with several devices, once per device from its own host thread (the bounce loop polls the queue sizes).
struct RenderJob { const GiCRenderParams* params; const GiCAovBinding* colorBinding; uint32_t width, height, rowBegin, rowEnd, rowStride, tileRows;
    uint8_t clear[GI_C_MAX_AOV_COMP_SIZE]; bool readback;
    bool momentsContinue = false; }; // GI_C_AOV_EXT_MOMENTS: the bound buffer holds the moments of the call before this one (giCRenderImpl)

static void* rbMem(GiCRenderBuffer* rb, uint32_t slot) { return (slot == 0u || rb->scratch) ? rb->deviceMem : rb->replicaMem[slot - 1u]; }

// ---------------------------------------------------------------------------------------------------------------
// renderOnDevice and its phases, in the order they run
// ---------------------------------------------------------------------------------------------------------------
// What the bindings of a render resolve to on one device (Gi.h:36-56).  NEE, Bounces and ClockCycles follow whole paths: they are filled by the colour pass
// (clear value first), see PathState.  ClockCycles is a deterministic cost proxy (ray segments per pixel), heat-mapped like the reference.
struct BoundAovs {
  AovTargets targets{};                          // what k_aov writes ...
  std::vector<GiCRenderBuffer*> produced;        // ... and the buffers behind it
  GiCRenderBuffer* nee = nullptr; GiCRenderBuffer* bounces = nullptr; GiCRenderBuffer* clock = nullptr; // the path-following AOVs
  GiCRenderBuffer* moments = nullptr;            // GI_C_AOV_EXT_MOMENTS: filled beside every batch's accumulation (gi_moments.hip)
  GiCRenderBuffer* color = nullptr;              // the colour AOV's buffer, or `scratchColor` when only path-following AOVs need the colour pass
  GiCRenderBuffer scratchColor{};
};

static int bindAovs(SceneDevice& D, const RenderJob& job, hipStream_t st, BoundAovs& A)
{
  const GiCRenderParams* params = job.params;
  for (uint32_t i = 0; i < params->aovBindingCount; i++) {
    const GiCAovBinding& b = params->aovBindings[i];
    if (b.aovId == GI_C_AOV_COLOR) continue;
    GiCRenderBuffer* rb = b.renderBuffer;
    if (rb->width != job.width || rb->height != job.height) { setError("giCRender: AOV buffers must share one size"); return GI_C_ERROR; }
    if (b.aovId == GI_C_AOV_EXT_MOMENTS) { // outside the enum: neither k_aov's nor a path-following AOV; no clear value
      if (rb->stride != 16 || rb->format != GI_C_FORMAT_FLOAT32_VEC4) { setError("giCRender: the moments AOV needs a Float32Vec4 buffer"); return GI_C_ERROR; }
      if (A.moments) { setError("giCRender: the moments AOV is bound twice"); return GI_C_ERROR; }
      A.moments = rb;
      continue;
    }
    if (b.aovId < 0 || b.aovId >= GI_C_AOV_COUNT) { setError("giCRender: bad AOV id"); return GI_C_ERROR; }
    AovTargets& T = A.targets;
    memcpy(T.clear[b.aovId], b.clearValue, 16);
    const bool vec = rb->stride == 16;
    F4* v4 = vec ? reinterpret_cast<F4*>(rbMem(rb, D.slot)) : nullptr;
    bool produced = true;
    switch (b.aovId) {
      case GI_C_AOV_NORMAL: T.normal = v4; break; case GI_C_AOV_BARYCENTRICS: T.barycentrics = v4; break;
      case GI_C_AOV_TEXCOORDS: T.texcoords = v4; break; case GI_C_AOV_OPACITY: T.opacity = v4; break;
      case GI_C_AOV_TANGENTS: T.tangents = v4; break; case GI_C_AOV_BITANGENTS: T.bitangents = v4; break;
      case GI_C_AOV_THIN_WALLED: T.thinWalled = v4; break; case GI_C_AOV_DOUBLE_SIDED: T.doubleSided = v4; break;
      case GI_C_AOV_ALBEDO: T.albedo = v4; break;
      case GI_C_AOV_DEPTH: T.depth = vec ? nullptr : reinterpret_cast<float*>(rbMem(rb, D.slot)); break;
      case GI_C_AOV_OBJECT_ID: T.objectId = vec ? nullptr : reinterpret_cast<int32_t*>(rbMem(rb, D.slot)); break;
      case GI_C_AOV_FACE_ID: T.faceId = vec ? nullptr : reinterpret_cast<int32_t*>(rbMem(rb, D.slot)); break;
      case GI_C_AOV_INSTANCE_ID: T.instanceId = vec ? nullptr : reinterpret_cast<int32_t*>(rbMem(rb, D.slot)); break;
      case GI_C_AOV_NEE: if (vec) A.nee = rb; produced = false; break;
      case GI_C_AOV_BOUNCES: if (vec) A.bounces = rb; produced = false; break;
      case GI_C_AOV_CLOCK_CYCLES: if (vec) A.clock = rb; produced = false; break;
      default: produced = false; break;
    }
    if (produced) {
      const bool wantsVec = !(b.aovId == GI_C_AOV_DEPTH || b.aovId == GI_C_AOV_OBJECT_ID || b.aovId == GI_C_AOV_FACE_ID || b.aovId == GI_C_AOV_INSTANCE_ID);
      if (wantsVec != vec) { setError("giCRender: AOV render buffer format does not match the AOV (Gi.cpp:302-316)"); return GI_C_ERROR; }
      A.produced.push_back(rb);
    } else { // clear value everywhere (the host copy was filled by fillClearValues before the device threads started)
      HIP_TRY(hipMemcpyAsync(rbMem(rb, D.slot), rb->hostMem, rb->size, hipMemcpyHostToDevice, st));
    }
  }
  A.color = job.colorBinding ? job.colorBinding->renderBuffer : nullptr;
  if (!A.color && (A.nee || A.bounces || A.clock || A.moments)) { // the path-following debug AOVs need the colour pass: render it into a scratch buffer
    const size_t n = (size_t)job.width * job.height;
    if (D.scratchColor.alloc(n)) return GI_C_ERROR;
    GiCRenderBuffer& c = A.scratchColor;
    c.width = job.width; c.height = job.height; c.stride = 16; c.size = n * 16;
    c.deviceMem = D.scratchColor.ptr; c.deviceOnly = true; c.scratch = true;
    A.color = &c;
  }
  if (A.color && A.color->stride != 16) { setError("giCRender: colour AOV needs a Float32Vec4 buffer"); return GI_C_ERROR; }
  return GI_C_OK;
}

// device -> host copy of the tile's rows (one 2D copy: the rows are rowStride image rows apart)
static hipError_t copyTileRows(GiCRenderBuffer* rb, size_t texel, const RenderJob& job, uint32_t slot, hipStream_t st)
{
  const size_t off = (size_t)job.rowBegin * job.width * texel, rowBytes = (size_t)job.width * texel, pitch = rowBytes * job.rowStride;
  if (job.rowStride == 1u) {
    return hipMemcpyAsync((uint8_t*)rb->hostMem + off, (uint8_t*)rbMem(rb, slot) + off, rowBytes * job.tileRows, hipMemcpyDeviceToHost, st);
  }
  return hipMemcpy2DAsync((uint8_t*)rb->hostMem + off, pitch, (uint8_t*)rbMem(rb, slot) + off, pitch, rowBytes, job.tileRows, hipMemcpyDeviceToHost, st);
}

// Uniforms (Gi.cpp:2373-2426; camera terms rp_main.rgen:199-212 evaluated once on the host).  The schedule adds its flags later (scheduleFrame /
// scheduleBatch).
// (the camera terms alone: giCDebugMissRect needs them without a scene)
static void cameraUniforms(const GiCCameraDesc& c, uint32_t width, uint32_t height, FrameUniforms& U)
{
  auto norm3 = [](const float* v, float* o) {
    float inv = 1.0f / sqrtf((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]);
    o[0] = v[0] * inv; o[1] = v[1] * inv; o[2] = v[2] * inv;
  };
  norm3(c.forward, U.camFwd); norm3(c.up, U.camUp);
  memcpy(U.camPos, c.position, 12);
  U.camRight[0] = U.camFwd[1] * U.camUp[2] - U.camFwd[2] * U.camUp[1];
  U.camRight[1] = U.camFwd[2] * U.camUp[0] - U.camFwd[0] * U.camUp[2];
  U.camRight[2] = U.camFwd[0] * U.camUp[1] - U.camFwd[1] * U.camUp[0];
  float aspect = (float)width / (float)height;
  float H = 1.0f, W = H * aspect;
  float d = H / (2.0f * tanf(c.vfov * 0.5f));
  U.WX = W / (float)width; U.HY = H / (float)height;
  for (int a = 0; a < 3; a++) {
    float C = U.camPos[a] + U.camFwd[a] * d;
    U.L[a] = (C - U.camRight[a] * W * 0.5f) - U.camUp[a] * H * 0.5f;
  }
  U.lensRadius = (c.fStop > 0.0f) ? c.focalLength / (2.0f * c.fStop) : 0.0f;
  U.focusDistance = c.focusDistance;
  uint32_t cr = packHalf2x16(c.clipStart, c.clipEnd);
  U.clipNear = f16ToF32((uint16_t)(cr & 0xffffu)); U.clipFar = f16ToF32((uint16_t)(cr >> 16));
}
static uint32_t samplingFlags(const GiCRenderSettings& rs)
{
  return (rs.jitteredSampling ? FLAG_JITTER : 0u) | (rs.filterImportanceSampling ? FLAG_FIS : 0u) | (rs.depthOfField ? FLAG_DOF : 0u);
}
static FrameUniforms makeUniforms(const GiCRenderParams& params, const RenderJob& job, const GiCScene* s)
{
  const GiCRenderSettings& rs = params.renderSettings;
  const GiCCameraDesc& c = params.camera;
  const uint32_t width = job.width, height = job.height;
  FrameUniforms U{};
  cameraUniforms(c, width, height, U);
  float cv[4]; memcpy(cv, job.clear, 16);
  for (int a = 0; a < 3; a++) { // fallback dome texel: glm::u8vec4(bg * 255) as RGBA8 unorm (Gi.cpp:2194-2199)
    int q = (int)(cv[a] * 255.0f); if (q < 0) q = 0; if (q > 255) q &= 255;
    U.background[a] = (float)q / 255.0f;
  }
  U.exposureScale = exp2f(c.exposure);
  U.spp = rs.spp; U.sampleOffset = s->sampleOffset; U.invSpp = 1.0f / (float)rs.spp; U.sppF = (float)rs.spp; U.sampleOffsetF = (float)s->sampleOffset;
  U.invTotalSampleCount = 1.0f / float(s->sampleOffset + rs.spp);
  U.maxSampleValue = rs.maxSampleValue; U.rrInvMinTermProb = rs.rrInvMinTermProb; U.lightIntensityMultiplier = rs.lightIntensityMultiplier;
  U.metersPerSceneUnit = rs.metersPerSceneUnit;
  U.mediumStackSize = rs.mediumStackSize; U.maxVolumeWalkLength = rs.maxVolumeWalkLength;
  U.maxBounces = std::min(rs.maxBounces, 0xfffu); U.rrBounceOffset = rs.rrBounceOffset & 0xffffu;
  U.imageWidth = width; U.imageHeight = height; U.rowBegin = job.rowBegin; U.rowStride = job.rowStride; U.pixelCount = (uint32_t)((size_t)job.tileRows * width);
  U.flags = samplingFlags(rs) |
            (rs.clippingPlanes ? FLAG_CLIP : 0u) | (rs.nextEventEstimation ? FLAG_NEE : 0u) | (rs.progressiveAccumulation ? FLAG_PROGRESSIVE : 0u);
  U.sphereCount = s->lightCounts[0]; U.distantCount = s->lightCounts[1]; U.rectCount = s->lightCounts[2]; U.diskCount = s->lightCounts[3]; // (uploadLights)
  U.totalLightCount = U.sphereCount + U.distantCount + U.rectCount + U.diskCount;
  return U;
}

// The scene as this render sees it: D's arrays plus the dome light (Gi.cpp:2201-2238, 2384-2396): an image-less dome light is ignored, like one whose file
// failed to load.  (mediumStackSize is the colour pass's: renderOnDevice sets it there.)
static SceneView makeFrameView(GiCScene* s, SceneDevice& D, const GiCRenderParams& params, const FrameUniforms& U)
{
  SceneView view = makeView(s, D);
  const GiCDomeLight* dl = params.domeLight;
  auto tit = (dl && dl->texture) ? std::find(s->textures.begin(), s->textures.end(), dl->texture) : s->textures.end();
  view.domeTexture = tit != s->textures.end() ? (uint32_t)(tit - s->textures.begin()) + 1u : 0u;
  view.domeCameraVisible = params.renderSettings.domeLightCameraVisible ? 1u : 0u;
  for (int a = 0; a < 4; a++) view.domeRotation[a] = dl ? dl->rotation[a] : (a == 3 ? 1.0f : 0.0f);
  for (int a = 0; a < 3; a++) {
    view.domeEmission[a] = dl ? dl->baseEmission[a] : 1.0f; view.background[a] = U.background[a];
    view.cameraPosition[a] = params.camera.position[a];
  }
  view.frame = params.renderSettings.frame;
  return view;
}

// --- memory plan (r04).  Work decomposition (DESIGN.md "Persistent path pool"): work item = (pixel, sample); the frame is cut into batches of
// consecutive samples whose per-sample colour buffer fits the budget; a pool of `slots` paths is kept full from a running
// work counter until the batch's items run out.
struct PathPlan {
  size_t slots = 1;                            // paths in the pool (the fused kernel keeps its paths in registers: 1)
  uint64_t batchSamples = 1;                   // samples per pixel and batch: sizes the per-sample colour buffer
  uint32_t wideBlocks = 1u, traceBlocks = 1u;  // persistent grids of the streaming kernels / of the traversal kernels
  uint32_t mediaStride = 0u;                   // floats of a slot's medium stack
  bool fused = false;                          // the batches run k_path (gi_path.hip) instead of the stage kernels
  bool pinned = false;                         // the caller gave the pool or the sample buffer a size: taken as given
};
// what the plan's arithmetic needs to know of the frame and the device
struct PlanInputs { size_t pixels; uint32_t cuCount, tracePerCu; };

static uint64_t optionU64(const char* key, uint64_t def) { return optionSet(key) ? (uint64_t)optionValue(key, 0) : def; }

// persistent grids: blocks per CU limited by registers (<= 6 waves/SIMD for k_trace) and, for k_trace, by the LDS it stages
static uint32_t traceBlocksPerCu(const SceneView& v)
{
  if (!traceBlockSync(v)) return 8u; // k_trace_dyn is persistent per wave: blocks beyond what is resident find the cursor exhausted
  uint32_t ln, lt, ldsBytes; traceLdsLayout(v, ln, lt, ldsBytes);
  return std::max(1u, std::min<uint32_t>(6u, blocksPerCuByLds(ldsBytes, traceStaticLdsBytes())));
}
static void sizeGrids(PathPlan& p, const PlanInputs& in)
{
  p.wideBlocks = (uint32_t)std::min<size_t>((p.slots + 255) / 256, (size_t)in.cuCount * 8u);
  p.traceBlocks = (uint32_t)std::min<size_t>((p.slots + 255) / 256, (size_t)in.cuCount * in.tracePerCu);
}
// what a plan costs: the slot pool with its queues (per slot: the Slot, the medium stack, and a share of every queue's records) and the sample buffer
static uint64_t planBytes(const PathPlan& p, size_t pixels)
{
  const uint64_t cap = shardCapacity(p.slots, p.wideBlocks, p.traceBlocks);
  const uint64_t perQueueEntry = 4ull * Q_COUNT + 32ull * (2 + 1) + 16ull + 8ull * 2;
  return (p.fused ? 0ull : (uint64_t)p.slots * (sizeof(Slot) + 4ull * p.mediaStride) + cap * NSHARD * perQueueEntry) + (uint64_t)pixels * p.batchSamples * 16ull
         + (uint64_t)pixels * 16ull;
}
// the next smaller plan: halve the sample buffer down to 64 MiB (more batches), then the pool down to 64 Ki slots (the caller sizes the grids again)
static bool shrinkPlan(PathPlan& p, size_t pixels)
{
  if (p.batchSamples > 1 && (uint64_t)pixels * p.batchSamples * 16ull > (64ull << 20)) {
    p.batchSamples = std::max<uint64_t>(1, p.batchSamples / 2);
    if (!p.fused) p.slots = (size_t)std::min<uint64_t>(p.slots, (uint64_t)pixels * p.batchSamples);
    return true;
  }
  if (!p.fused && p.slots > (64u << 10)) { p.slots /= 2; return true; }
  return false;
}

// The plan's arithmetic. The per-sample colour buffer wants to hold the whole frame's samples (every batch ends in a drain / a kernel tail: C2's 34 GB for 1024
// spp at 1080p in one batch 213.4 ms per step, in four 215.5) and scenes beyond LDS want a 64 Mi-slot pool (17 GB with its queues) -- on an empty 288 GB
// device. A Hydra plugin shares the device with other scenes, other processes and the host application, so the plan starts from what is FREE now (plus what
// this scene already holds in these buffers, which is reused), and an allocation that still fails (someone else was faster) is answered with a smaller plan
// -- more batches first, then a smaller pool -- never with a failed render while a workable plan exists (allocatePathPlan). Results do not depend on the plan
// (test_pool_and_batch_invariance).
// `samples`: samples per pixel the render wants in its buffer -- the call's spp, or a look-ahead window's.
static PathPlan planPathMemory(const GiCScene* s, const GiCRenderSettings& rs, uint64_t samples, const SceneView& view, const PlanInputs& in,
                               uint64_t freeBytes, uint64_t heldBytes, uint64_t memTotalMb)
{
  const size_t pixels = in.pixels;
  const uint64_t availMb = (freeBytes + heldBytes) >> 20;
  const uint64_t capMb = std::max<uint64_t>(1024, std::min<uint64_t>(49152, memTotalMb / 6)); // the budget of an empty device: 48 GiB of 288 GB
  const uint64_t defaultMb = std::max<uint64_t>(256, std::min<uint64_t>(capMb, availMb / 3));  // ... and a third of what is available now, 256 MiB at least
  const uint64_t budgetBytes = optionU64("sample_buffer_mb", s->optSampleBufferMb ? s->optSampleBufferMb : defaultMb) << 20;
  // Pool size: a launch of k_trace_dyn ends when its longest ray ends, and ray cost is heavy-tailed in scenes beyond LDS
  // (a 100-step ray outlives the average one six times over), so those scenes get a pool large enough to amortise that
  // tail (measured on C3 at spp 64 / 256: 4 Mi slots 630, 16 Mi 790, 32 Mi 831 / 810, 64 Mi - / 868 Msamples/s); LDS-resident scenes have uniform, short
  // rays.
  const uint64_t poolDefault = sceneFitsLds(s->nodeCount, s->triCount) ? (4u << 20) : (64u << 20);
  const uint64_t poolMax = std::min<uint64_t>((1ull << 30) - 1ull, // regen-queue entries keep two flag bits above the slot index (REGEN_MISSED, REGEN_FRESH)
                                              std::max<uint64_t>(64, optionU64("pool_slots", s->optPoolSlots ? s->optPoolSlots : poolDefault)));
  PathPlan p;
  p.batchSamples = std::min<uint64_t>(samples, std::max<uint64_t>(1, budgetBytes / (pixels * 16)));
  p.batchSamples = std::min<uint64_t>(p.batchSamples, std::max<uint64_t>(1, 0xffffffffull / pixels)); // work ids stay 32-bit
  // LDS-resident scenes without medium stacks / dome images: the fused persistent kernel k_path (gi_path.hip) keeps the paths in
  // registers -- no pool, no queues; the stage kernels remain the path for everything else (and on request: option / env)
  p.fused = pathKernelSupports(view) && s->optFusedPath != 0 && optionValue("fused", 1) != 0;
  p.slots = p.fused ? 1 : (size_t)std::min<uint64_t>(poolMax, (uint64_t)pixels * p.batchSamples);
  sizeGrids(p, in);
  // HIT-queue entries (and giCTraceRays) hold a TRACE-queue RECORD index in 30 bits (HIT_INDEX_MASK); records run up to shardCapacity * NSHARD, which exceeds
  // the slot count by the shards' slack -- a pinned pool near 2^30 would push indices past the mask and k_shade would gather the wrong record
  while (!p.fused && (uint64_t)shardCapacity(p.slots, p.wideBlocks, p.traceBlocks) * NSHARD > 0x3fffffffull /* HIT_INDEX_MASK, gi_queues.h */) {
    p.slots -= p.slots / 8;
    sizeGrids(p, in);
  }
  p.mediaStride = rs.mediumStackSize ? rs.mediumStackSize * MEDIUM_FLOATS + 4u : 0u;
  // the caller's sizes are taken as given
  p.pinned = optionSet("pool_slots") || s->optPoolSlots || optionSet("sample_buffer_mb") || s->optSampleBufferMb;
  // (leave 512 MiB, or half of a tiny remainder)
  if (!p.pinned) while (planBytes(p, pixels) > (availMb << 20) - std::min<uint64_t>(availMb << 19, 512ull << 20) && shrinkPlan(p, pixels)) sizeGrids(p, in);
  return p;
}

// Plans from what is free on the device now and allocates the plan; an allocation that fails with out-of-memory releases the resizable path state and tries
// the next smaller plan.
static int allocatePathPlan(GiCScene* s, SceneDevice& D, const GiCRenderSettings& rs, uint64_t samples, const SceneView& view, const PlanInputs& in,
                            PathPlan& plan)
{
  size_t memFree = 0, memTotal = 0; (void)hipMemGetInfo(&memFree, &memTotal);
  // tests: plan as if this much were free (a planner overtaken by another allocation: the fallback below must recover)
  if (optionSet("assume_free_mb")) memFree = (size_t)optionValue("assume_free_mb", 0) << 20;
  if (!D.memTotalMb) D.memTotalMb = std::max<uint64_t>(1, (uint64_t)(memTotal >> 20));
  plan = planPathMemory(s, rs, samples, view, in, memFree, D.pathStateBytes(), D.memTotalMb);
  for (int attempt = 0;; attempt++) {
    int rc = plan.fused ? GI_C_OK : ensurePathState(&D, plan.slots, plan.wideBlocks, plan.traceBlocks);
    if (rc == GI_C_OK) rc = D.sampleBuf.alloc(in.pixels * plan.batchSamples);
    if (rc == GI_C_OK) rc = D.accum.alloc(in.pixels);
    if (rc == GI_C_OK && plan.mediaStride) rc = D.media.alloc(plan.slots * plan.mediaStride);
    // (a smaller plan fitted: the "out of memory" of the larger ones is not this render's error)
    if (rc == GI_C_OK) { if (attempt > 0) t_lastError.clear(); return GI_C_OK; }
    if (rc != GI_C_OUT_OF_MEMORY_INTERNAL) return GI_C_ERROR;
    // out of memory: drop what this scene holds in the resizable buffers (a half-grown plan must not stand in the way of the smaller one) and try the next
    // plan
    D.releasePathState();
    if (attempt >= 40 || !shrinkPlan(plan, in.pixels)) {
      setError("giCRender: out of device memory even with the smallest sample buffer and path pool");
      return GI_C_ERROR;
    }
    sizeGrids(plan, in);
  }
}

// --- stage timers: HIP events around the stage launches of every `stride`-th iteration (events on every launch cost ~16 % of the
// frame); per-stage totals are scaled back up by the sampling factor.
struct StageTimers {
  enum Kind { RAYGEN = 0, TRACE = 1, SHADE = 2, SHADOW = 3 };
  struct IterRow { size_t evEnd; uint64_t traced, hits, shadow, ended, cont; };
  SceneDevice& D;
  bool on; uint32_t stride;
  bool iterLog;                  // GATLING_ITER_LOG, with timers on every iteration: one row per iteration (and one sync: for measurements only)
  bool sampling = false;         // the current iteration's launches are timed
  size_t ev = 0; std::vector<int> evKind;
  std::vector<IterRow> iterRows;
  uint64_t totalIters = 0, sampledIters = 0;

  StageTimers(const GiCScene* s, SceneDevice& d) : D(d), on(s->kernelTimers), stride(std::max(1u, s->kernelTimerStride)),
      iterLog(on && stride == 1u && getenv("GATLING_ITER_LOG") && atoi(getenv("GATLING_ITER_LOG")) != 0) {}
  void beginIteration(bool always = false) { sampling = on && (always || (totalIters % stride) == 0u); if (sampling) sampledIters++; }
  template <typename Fn> void timed(hipStream_t stream, int kind, Fn&& fn)
  {
    if (!sampling) { fn(); return; }
    (void)hipEventRecord(poolEvent(&D, ev), stream); fn(); (void)hipEventRecord(poolEvent(&D, ev + 1), stream);
    ev += 2; evKind.push_back(kind);
  }
  void finish(GiCRenderStats& S) const;
};

void StageTimers::finish(GiCRenderStats& S) const
{
  S.traceMs = S.shadeMs = S.raygenMs = S.shadowMs = 0.0;
  if (!on) return;
  auto elapsed = [&](size_t k) { float ms = 0.0f; (void)hipEventElapsedTime(&ms, D.eventPool[2 * k], D.eventPool[2 * k + 1]); return ms; };
  for (size_t k = 0; k < evKind.size(); k++) {
    const float ms = elapsed(k);
    if (evKind[k] == RAYGEN) S.raygenMs += ms; else if (evKind[k] == TRACE) S.traceMs += ms; else if (evKind[k] == SHADE) S.shadeMs += ms;
    else S.shadowMs += ms;
  }
  size_t k = 0;
  for (size_t r = 0; r < iterRows.size(); r++) { // per iteration: the stage times of its launches and what its queues held
    const IterRow& row = iterRows[r];
    double ms4[4] = {0.0, 0.0, 0.0, 0.0};
    for (; 2 * k < row.evEnd && k < evKind.size(); k++) ms4[evKind[k]] += elapsed(k);
    fprintf(stderr, "[gatling_gi] iter %3zu: rays %9llu hits %9llu shadow %9llu ended %9llu continuing %9llu | raygen %7.3f trace+route %7.3f shade %7.3f "
                    "shadow %7.3f ms\n", r,
            (unsigned long long)row.traced, (unsigned long long)row.hits, (unsigned long long)row.shadow, (unsigned long long)row.ended,
            (unsigned long long)row.cont, ms4[0], ms4[1], ms4[2], ms4[3]);
  }
  // scale the sampled totals to the whole frame (the early-exit poll can leave one raygen-only iteration unsampled)
  const double scale = sampledIters ? (double)totalIters / (double)sampledIters : 1.0;
  S.raygenMs *= scale; S.traceMs *= scale; S.shadeMs *= scale; S.shadowMs *= scale;
}

// --- what the phases of the colour pass share
struct Schedule {
  bool twoStreamOk = false;     // batches whose work fits the pool may run their shadow launches on the second stream (scheduleFrame)
  long twoStreamDelay = 0;      // test hook: 1 | 2 holds the main | the second stream back
  uint32_t dynRefill = 8u;      // k_trace_dyn refill threshold
  uint32_t walkCarry = 0u;      // k_path: the closest-hit loop of a trip ends once at most this many lanes are still walking (0: never early)
  uint32_t lobePark = 0u;       // k_path: hits that drew a glossy lobe are parked and shaded together once this many wait (0: shaded where they are)
  uint32_t ringCarry = 0u;      // k_path: the triangle ring is carried across the steps of a trip's closest-hit loop (0: every step empties it)
  uint32_t nodeCook = 0u;       // k_path: the variants that have one stage their nodes cooked (gi_node_cook.h; 0: never)
  uint32_t upsTraits = 0u;      // k_path: the traits of the scene's class-1 materials its plain variant may be compiled for (0: the general kernel)
  int32_t shadowOrderNow = -1;  // visiting order of the shadow walks; -1: not chosen yet -- alternate, and count (chooseShadowOrder)
};
struct Frame {
  GiCScene* s; SceneDevice& D; const DevCtx& ctx; const RenderJob& job; const GiCRenderSettings& rs;
  hipStream_t st;
  size_t pixels;
  StageTimers tm;
  FrameUniforms U{}; SceneView view{};
  PathPlan plan; PathState ps{}; QueueSet qs{}; Schedule sch;
  F4* colorOut = nullptr;
  GiCRenderBuffer* moments = nullptr; // GI_C_AOV_EXT_MOMENTS bound: k_moments runs beside every fold of this render
  bool stackHighCounted = false; // this render zeroed Counters::stackHigh and ran walks that raise it (traceColour)
  uint32_t numBatches = 0;
  uint32_t iters = 0, traceLaunches = 0; // GiCRenderStats::iterations / traceLaunches
  double tStart = 0.0;
  uint32_t windowCalls = 0;     // sample look-ahead: >= 2 = the colour pass traces ONE batch of windowCalls * spp samples; this call folds the first spp
  bool served = false;          // ... or this call traced nothing: its samples came out of the window (serveFromWindow)
  uint64_t skippedSegments = 0; // FLAG_MISS_RECT: samples of the pixels k_path was given no work for -- each is a path of one segment (fillStats)
};

// The PathState of the colour pass: the pool, and what the path-following AOVs bound to this render need beside it.
static int bindPathAovs(Frame& f, const BoundAovs& A)
{
  SceneDevice& D = f.D;
  f.ps = PathState{D.slots.ptr, D.media.ptr, f.plan.mediaStride, nullptr, 0u, nullptr};
  if (A.nee && f.rs.nextEventEstimation) { // the reference compiles the NEE AOV write out with NEXT_EVENT_ESTIMATION (rp_main.rgen:397, 431)
    if (D.neeKey.alloc(f.pixels)) return GI_C_ERROR;
    HIP_TRY(hipMemsetAsync(D.neeKey.ptr, 0, f.pixels * sizeof(unsigned long long), f.st));
    f.ps.neeKey = D.neeKey.ptr;
  }
  if (A.bounces) f.ps.bouncesAov = reinterpret_cast<F4*>(rbMem(A.bounces, D.slot));
  if (A.clock) {
    if (D.pathSegments.alloc(f.pixels)) return GI_C_ERROR;
    HIP_TRY(hipMemsetAsync(D.pathSegments.ptr, 0, f.pixels * sizeof(uint32_t), f.st));
    f.ps.pathSegments = D.pathSegments.ptr;
  }
  return GI_C_OK;
}

// --- the schedule: every rule that decides HOW the planned work runs, derived from (plan, view, settings, options).  scheduleFrame: once per render;
// scheduleBatch: the two bits that depend on a batch's size.
static Schedule scheduleFrame(Frame& f)
{
  const GiCScene* s = f.s; const GiCRenderSettings& rs = f.rs; FrameUniforms& U = f.U;
  const bool fused = f.plan.fused;
  // work order of the wavefront pipeline and layout of its per-sample buffer (gi_queues.h work_item); the fused kernels hand work out sample-major
  if (!fused && optionValue("work_order", WORK_ORDER_PIXEL_MAJOR_DEFAULT ? 1 : 0) != 0) U.flags |= FLAG_PIXEL_MAJOR;
  // Deferred Slot initialisation (r04): k_raygen hands a camera ray its (rng, work item) beside the ray record instead of writing the path's 64-byte Slot;
  // the slot is written where the first segment hits (k_route / k_trace) and a camera ray that leaves the scene retires there without ever touching one. The
  // debug AOVs that follow whole paths read the slot when a sample retires (NEE / Bounces / ClockCycles): renders that bind them keep the eager form.
  if (!fused && optionValue("defer_slot", 1) != 0 && !f.ps.neeKey && !f.ps.bouncesAov && !f.ps.pathSegments) U.flags |= FLAG_DEFER_SLOT;
  // Bounds retire (r04n): on the k_trace_dyn path (k_route zeroes the regen counter k_raygen then appends to) a deferred-slot camera ray that cannot reach
  // the scene's bounds is retired by k_raygen itself (C4: 58 % of the camera rays, C3: ~45 %) -- same sample, same segment count, no ray record, no traversal
  // step, no routing. Not with a dome image / medium stack (a miss needs the slot), not in counting builds (the root visit of such a ray is part of
  // nodes-per-ray), not on the two-level layout (bounds of the TLAS root: not kept).
  if ((U.flags & FLAG_DEFER_SLOT) && !traceBlockSync(f.view) && !f.view.twoLevel && f.view.domeTexture == 0u && rs.mediumStackSize == 0u && !s->countTraversal
      && s->boundsValid && optionValue("bounds_retire", 1) != 0) {
    U.flags |= FLAG_BOUNDS_RETIRE;
    for (int a = 0; a < 3; a++) { U.sceneLo[a] = s->bounds[a]; U.sceneHi[a] = s->bounds[3 + a]; }
  }
  // ... and in the fused kernel: k_path applies the same test where it prepares camera rays for its ring, and stores the retired sample there (gi_path.hip).
  // With work handed out sample-major a wave holds 64 adjacent pixels of a row, so where the frame is wider than the scene whole waves would otherwise spend
  // whole trips on rays that miss (C2: 62 % of the camera rays). pathKernelSupports has excluded dome image, medium stack and two-level; the path-following
  // debug AOVs keep today's route (the rule of defer_slot above), and so do counting builds.
  if (fused && s->boundsValid && optionValue("bounds_retire", 1) != 0 && !s->countTraversal && !f.ps.neeKey && !f.ps.bouncesAov && !f.ps.pathSegments) {
    U.flags |= FLAG_BOUNDS_RETIRE;
    for (int a = 0; a < 3; a++) { U.sceneLo[a] = s->bounds[a]; U.sceneHi[a] = s->bounds[3 + a]; }
  }
  // The miss rectangle (gi_miss_rect.h): k_path still prepared the full-width camera ray of every one of those samples -- hash, two draws, the filter's log / sqrt
  // / sincos, the normalise, the slab test's divisions, a 16-byte record -- and k_accumulate read the identical records back.  For a pixel whose every possible
  // camera ray misses the bounds none of that reaches the image: such pixels get no work items (k_path enumerates the rectangle's pixels only) and no records
  // (k_accumulate sums the constant in their place, same loop).  It rests on the per-ray retire (the pixels INSIDE the rectangle are still tested ray by ray),
  // so it inherits every condition of FLAG_BOUNDS_RETIRE above.  A look-ahead window keeps the whole frame: later calls fold its records with k_fold_window,
  // which reads every pixel's.  With max-bounces 0 no kernel traces anything (runZeroBounceBatch: every sample is black, not the background).
  if (fused) {
    U.rectX0 = 0u; U.rectX1 = U.imageWidth; U.rectTy0 = 0u; U.rectTy1 = f.job.tileRows;
    if ((U.flags & FLAG_BOUNDS_RETIRE) && U.maxBounces > 0u && f.windowCalls < 2u && optionValue("miss_rect", 1) != 0) {
      const MissRect r = computeMissRect(U.sceneLo, U.sceneHi, U, U.imageWidth, U.imageHeight);
      uint32_t ty0, ty1; missRectTileRows(r, U.rowBegin, U.rowStride, f.job.tileRows, ty0, ty1);
      if (r.empty() || ty1 <= ty0) { U.rectX0 = U.rectX1 = U.rectTy0 = U.rectTy1 = 0u; }
      else { U.rectX0 = r.x0; U.rectX1 = r.x1; U.rectTy0 = ty0; U.rectTy1 = ty1; }
    }
    U.activeWidth = U.rectX1 - U.rectX0; U.activeCount = U.activeWidth * (U.rectTy1 - U.rectTy0);
    if (U.activeCount < U.pixelCount) U.flags |= FLAG_MISS_RECT;
  }
  Schedule sch;
  // Walk carry of k_path (gi_path.hip): lanes still walking when at most this many are left go on in the next trip's loop.  Counting builds run every loop
  // to its end by default, so that the phase counters (lanes per phase and trip) and the step histogram describe whole walks; an explicit walk_carry key
  // reaches them too (the counters are then how a test sees that lanes were carried: giCDebugPathWalkStats).
  sch.walkCarry = s->countTraversal && !optionSet("walk_carry") ? 0u : (uint32_t)std::min(std::max(optionValue("walk_carry", WALK_CARRY_DEFAULT), 0L), 63L);
  // Lobe parking of k_path (gi_path.hip): the threshold at which a wave shades its parked glossy hits.  walk_carry's rule for counting builds: off unless the
  // key is set, so that the phase tables keep describing plain trips (giCDebugPathLobeStats then shows what the parking did).
  sch.lobePark = s->countTraversal && !optionSet("lobe_park") ? 0u : (uint32_t)std::min(std::max(optionValue("lobe_park", LOBE_PARK_DEFAULT), 0L), 64L);
  // Ring carry of k_path (gi_path.hip): pending (ray, triangle) pairs wait for a full batch across the steps of a trip.  A walk then culls with a distance
  // that may lag by a step, so a counting build's nodesVisited / trisTested move with it: the same rule again, off there unless the key is set.
  sch.ringCarry = s->countTraversal && !optionSet("ring_carry") ? 0u : (optionValue("ring_carry", RING_CARRY_DEFAULT) != 0 ? 1u : 0u);
  // The plain UsdPreviewSurface variant of k_path (gi_path.hip): the scene's traits (deriveSceneClasses) unless switched off.  Which kernels take them is
  // launchPath's rule (pathUpsVariant); counting builds run the general kernel, whose counters the tests read.
  f.s->upsPlainLaunched = 0u; // giCDebugSceneUpsPlain: until a fused batch of this render launches (runFusedBatch)
  sch.upsTraits = !s->countTraversal && optionValue("ups_plain", UPS_PLAIN_DEFAULT) != 0 ? s->upsTraits : 0u;
  // Cooked nodes of k_path (gi_node_cook.h): wanted unless switched off; which kernels have the variant and whether the tree's cooked image may take its
  // place in LDS is launchPath's rule (counting builds run the general kernel, which has none).
  f.s->nodeCookLaunched = 0u; // giCDebugSceneNodeCook: until a fused batch of this render launches (runFusedBatch)
  sch.nodeCook = optionValue("node_cook", NODE_COOK_DEFAULT) != 0 ? 1u : 0u;
  sch.dynRefill = traceDynRefill(s);
  // (GATLING_OPTIONS=shadow_order=0|1 pins it)
  sch.shadowOrderNow = optionSet("shadow_order") ? (int32_t)optionValue("shadow_order", -1) : s->shadowOrder.load();
  // Two streams (the reference's default frame is ONE sample per pixel, renderDelegate.cpp:93-110). In a batch
  // whose work fits the pool every path starts in iteration 0, so from iteration 1 on k_raygen only FINISHES samples and the closest-hit launch of iteration
  // i + 1 needs nothing from the shadow launch of iteration i -- which k_raygen(i + 1) (it reads the radiance of paths that ended) and k_shade(i + 1) (it
  // goes on adding to it: the float order of rp_main.rgen:397-480) do need. Such batches run
  //     main stream:    Z(i)  [R(0)]  T(i) + route(i)   <wait for Sh(i-1)>   [R(i), i > 0]   S(i)
  //     second stream:                                  <wait for S(i)>  Sh(i)
  // so that Sh(i) runs beside T(i + 1): an iteration lasts max(trace, shadow) + raygen + shade instead of their sum. Per-path arithmetic and per-pixel sample
  // order are untouched (same kernels, same records); what changes is who zeroes which queue counter (gi_queues.h zero_next_counters / zero_closest_counters:
  // Z = k_zero_closest). Not with a dome image (a miss adds the dome's radiance to the Slot in k_route while the previous bounce's shadow launch may still be
  // adding to it: two float additions in an order that would depend on timing) or a medium stack. GATLING_OPTIONS=two_stream=0 switches it off;
  // two_stream_delay=1|2 (tests) holds the main | the second stream back for 0.3 ms per iteration so that the other one runs ahead.
  // Invariant this rests on: with cutouts T(i + 1) reads Slot::rad.w (the any-hit rng) while Sh(i) may be doing its 16-byte read-modify-write of the same
  // Slot::rad -- the shadow kernels write rad.w back with the value they read, so the closest-hit launch sees ONE value whatever the timing. A shadow kernel
  // that ever changes rad.w must store .xyz alone, or scenes with cutouts must leave this rule.
  sch.twoStreamOk = rs.nextEventEstimation != 0 && rs.mediumStackSize == 0u && f.view.domeTexture == 0u && optionValue("two_stream", 1) != 0
                    && f.ctx.stream2 != nullptr;
  sch.twoStreamDelay = optionValue("two_stream_delay", 0);
  return sch;
}
// `rounds`: k_raygen rounds the batch needs to hand out all its work (1: the work fits the pool).  Returns whether the batch runs on two streams.
static bool scheduleBatch(Frame& f, uint64_t rounds)
{
  const GiCScene* s = f.s; FrameUniforms& U = f.U;
  // A thin batch (its work fits the pool and is small: the delegate's one sample per
  // pixel and call) launches every kernel of an iteration for a few thousand hits:
  // a further k_shade launch per iteration costs it more (C4: 13 x ~9 us of a 2.7 ms call) than the BASE variant saves, so its BASE hits are binned with
  // class 2 (GATLING_OPTIONS=merge_shade_variants=0 | 1: never | always)
  const long mergeOpt = optionValue("merge_shade_variants", -1);
  const bool thinBatch = rounds == 1 && U.workTotal <= (8u << 20);
  if ((mergeOpt < 0 ? thinBatch : mergeOpt != 0) && (s->shadeClassMask & (1u << SHADE_CLASS_OPBR_BASE)) && (s->shadeClassMask & 4u)) {
    U.flags |= FLAG_MERGE_SHADE_VARIANTS;
  } else U.flags &= ~FLAG_MERGE_SHADE_VARIANTS;
  // (the iteration log synchronises the main stream every iteration: it would only ever see one stream's work)
  const bool two = f.sch.twoStreamOk && rounds == 1 && !f.tm.iterLog;
  if (two) U.flags |= FLAG_TWO_STREAM; else U.flags &= ~FLAG_TWO_STREAM;
  return two;
}

// --- the three kinds of batch.  renderOnDevice has set the batch's uniforms and launched k_init; each ends in the batch's accumulation.
static void accumulateBatch(Frame& f, uint32_t batch)
{
  // the moments AOV: the same records, before the next batch overwrites them (a window: this call's share, its first spp; later batches continue the first's)
  if (f.moments) launchMoments(f.st, f.U, f.D.sampleBuf.ptr, reinterpret_cast<F4*>(rbMem(f.moments, f.D.slot)), f.U.batchSamples, 0u,
                               f.windowCalls >= 2u ? f.U.spp : f.U.batchSamples, (f.U.flags & FLAG_PIXEL_MAJOR) != 0u, batch > 0u || f.job.momentsContinue);
  if (f.windowCalls >= 2u) { // a look-ahead window (one batch): this call's samples are its first spp
    launchFoldWindow(f.st, f.U, f.D.sampleBuf.ptr, f.colorOut, f.U.batchSamples, 0u, (f.U.flags & FLAG_PIXEL_MAJOR) != 0u);
    return;
  }
  launchAccumulate(f.st, f.U, f.D.sampleBuf.ptr, f.D.accum.ptr, f.colorOut, batch == 0, batch + 1 == f.numBatches);
}

// LDS-resident scenes: one launch of the fused persistent kernel k_path runs the batch's paths from camera ray to retirement
static int runFusedBatch(Frame& f, uint32_t batch)
{
  GiCScene* s = f.s; SceneDevice& D = f.D; const FrameUniforms& U = f.U;
  // work items are claimed in chunks of consecutive ids; small frames get small chunks so that every resident wave finds work
  uint32_t chunk = 2048u;
  const uint64_t waves = (uint64_t)f.ctx.cuCount * 16u;
  // (a wave's last chunk is the launch's tail: 16 claims per wave keep it at ~6 % of a small frame -- C1 5 895 -> 6 360 Msamples/s; C2 does not care, 256
  // ... 2048 measure the same)
  chunk = (uint32_t)std::min<uint64_t>(chunk, std::max<uint64_t>(64u, ((uint64_t)U.workTotal / (waves * 16u)) & ~63ull));
  f.tm.beginIteration(true); // one launch per batch: timed whatever the stride
  uint32_t cooked = 0u;
  f.tm.timed(f.st, StageTimers::TRACE, [&] {
    launchPath(f.st, (uint32_t)f.ctx.cuCount, s->classMask, s->classTextured != 0u, s->countTraversal, chunk, f.sch.walkCarry, f.sch.lobePark, f.sch.ringCarry,
               f.sch.upsTraits, f.sch.nodeCook, U, f.view, f.ps, D.dCounters.ptr, D.sampleBuf.ptr, &cooked);
  });
  s->nodeCookLaunched = cooked; // (every device of the render launches the same variant, as below)
  // (every device of the render launches the same variant: one value, whoever writes it)
  s->upsPlainLaunched = pathUpsVariant(s->classMask, s->classTextured != 0u, (U.flags & FLAG_NEE) != 0u, f.view.hasCutouts != 0u, s->countTraversal, f.sch.upsTraits);
  f.iters++; f.tm.totalIters++; f.traceLaunches++;
  accumulateBatch(f, batch);
  return GI_C_OK;
}

// rp_main.rgen:298-304: the bounce loop's exit test comes first, so with max-bounces 0 no ray is traced at all and every sample is
// black (no emission at the primary hit, no dome / background term); the accumulation still runs (progressive blend, alpha 1)
static int runZeroBounceBatch(Frame& f, uint32_t batch)
{
  HIP_TRY(hipMemsetAsync(f.D.sampleBuf.ptr, 0, f.pixels * f.U.batchSamples * sizeof(F4), f.st));
  accumulateBatch(f, batch);
  return GI_C_OK;
}

// The bounce loop (rp_main.rgen:215, 295) of the wavefront pipeline: every pool slot advances one stage per iteration, until the batch's work is handed out and
// the pool has drained.  This function owns the second stream: whichever way it returns, no shadow launch of its is still running unjoined -- on success the
// main stream waits for the last one (an event wait, as ever); on an error it makes the second stream idle first (JoinShadow), so that the caller's error
// and shrink paths never release buffers under a running kernel.
static int runWavefrontBatch(Frame& f, uint32_t batch, uint32_t poolNow)
{
  GiCScene* s = f.s; SceneDevice& D = f.D; FrameUniforms& U = f.U; StageTimers& tm = f.tm;
  const GiCRenderSettings& rs = f.rs; const PathPlan& plan = f.plan; const Schedule& sch = f.sch;
  hipStream_t st = f.st, st2 = f.ctx.stream2;
  const uint64_t rounds = ((uint64_t)U.workTotal + poolNow - 1) / poolNow; // raygen rounds needed to hand out all work
  const uint64_t maxIters = (rounds + 2) * (std::max(1u, U.maxBounces) + 1) + 8;
  const bool two = scheduleBatch(f, rounds);
  const bool nee = rs.nextEventEstimation != 0;
  bool shadowInFlight = false; // a shadow launch on st2 that st has not been made to wait for yet
  struct JoinShadow {
    hipStream_t st2; const bool& inFlight;
    ~JoinShadow() { if (inFlight) (void)hipStreamSynchronize(st2); } // (false on every successful return: nothing is added there)
  } joinOnError{st2, shadowInFlight};
  auto joinShadow = [&]() -> hipError_t { // the main stream goes on behind the shadow launch in flight
    if (!shadowInFlight) return hipSuccess;
    const hipError_t e = hipStreamWaitEvent(st, D.evShadow, 0);
    if (e == hipSuccess) shadowInFlight = false;
    return e;
  };
  for (uint64_t it = 0; it < maxIters; it++) {
    const uint32_t par = (uint32_t)(it & 1u);
    tm.beginIteration();
    auto raygen = [&] { tm.timed(st, StageTimers::RAYGEN, [&] { launchRaygen(st, plan.wideBlocks, U, f.ps, f.qs, D.dCounters.ptr, par, D.sampleBuf.ptr); }); };
    if (two) launchZeroClosest(st, D.dCounters.ptr, par);
    if (!two || it == 0) raygen();
    // (the last k_raygen of the batch: the test below ends the loop) k_raygen(it) after the shadow launch of it - 1 (two streams, it > 0)
    else if (rounds == 1 && it == (uint64_t)std::max(1u, U.maxBounces)) { HIP_TRY(joinShadow()); raygen(); }
    // A batch whose work fits the pool (a low-spp frame: hdGatling renders ONE sample per pixel and call) starts every path in iteration 0, a path traces
    // at most maxBounces segments, one per iteration (the bounce counter, rp_main.rgen:298-304) -- so k_raygen(maxBounces) has just retired the last
    // samples and nothing is in flight: no need to find that out two empty iterations later through the poll below (10 launches of ~90 in a spp-1 call).
    if (rounds == 1 && it == (uint64_t)std::max(1u, U.maxBounces) && rs.mediumStackSize == 0u) { tm.totalIters++; break; }
    if (it >= rounds) {
      // All work cannot be handed out earlier. From here on every iteration snapshots the queue sizes behind its k_raygen (asynchronous copy into a pinned
      // ring) and tests the snapshot of POLL_LAG iterations ago: the wait is for work the GPU finished long ago -- it still holds the iterations in
      // between, so the stream never runs dry -- and the loop stops at most POLL_LAG empty iterations after the pool drained. (Until r03 the loop
      // synchronised every 16th iteration: C4 ran 15 empty iterations of 0.2 ms each, `tools/exp_iter_log.py`.)
      constexpr uint32_t R = SceneDevice::POLL_RING, LAG = SceneDevice::POLL_LAG;
      constexpr size_t snapshot = (size_t)Q_COUNT * NSHARD;
      HIP_TRY(hipMemcpyAsync(D.hPoll + (it % R) * snapshot, D.dCounters.ptr, sizeof(PaddedCounter) * snapshot, hipMemcpyDeviceToHost, st));
      HIP_TRY(hipEventRecord(D.pollEvent[it % R], st));
      if (it >= rounds + LAG) {
        const uint64_t j = it - LAG;
        HIP_TRY(hipEventSynchronize(D.pollEvent[j % R]));
        const PaddedCounter* snap = D.hPoll + (j % R) * snapshot + (size_t)(Q_TRACE_A + (uint32_t)(j & 1u)) * NSHARD;
        // (FLAG_BOUNDS_RETIRE: a k_raygen whose camera rays all miss the scene's bounds queues no ray either, but hands its slots on -- REGEN[(j&1)^1],
        // zero at this point otherwise -- and work is left)
        const PaddedCounter* again = D.hPoll + (j % R) * snapshot + (size_t)(Q_REGEN_A + (uint32_t)((j & 1u) ^ 1u)) * NSHARD;
        uint32_t pending = 0; for (uint32_t k = 0; k < NSHARD; k++) pending += snap[k].v + again[k].v;
        if (pending == 0) { tm.totalIters++; break; } // k_raygen(j) consumed the regen queue and produced no rays: the pool had drained
      }
    }
    if (two && sch.twoStreamDelay == 1) launchSpin(st, 300000ull);
    tm.timed(st, StageTimers::TRACE, [&] {
      launchTrace(st, plan.traceBlocks, false, s->countTraversal, f.view, f.ps, f.qs, D.dCounters.ptr, Q_TRACE_A + par, Q_REGEN_A + (par ^ 1u), sch.dynRefill,
                  plan.wideBlocks, U, D.sampleBuf.ptr);
    });
    f.traceLaunches++;
    if (two && it > 0) { HIP_TRY(joinShadow()); raygen(); } // k_raygen(it) runs behind this iteration's closest-hit launch, after the shadow launch of it - 1
    // one launch per shade class in use (scattering events inside a medium are routed to class 2, k_route: it is launched whenever a medium stack exists
    // and OpenPBR does)
    uint32_t shadeMask = s->shadeClassMask | ((rs.mediumStackSize != 0u && (s->shadeClassMask & (1u << SHADE_CLASS_OPBR_BASE))) ? 4u : 0u);
    // BASE hits sit in class 2's queue
    if (U.flags & FLAG_MERGE_SHADE_VARIANTS) shadeMask = (shadeMask & ~(1u << SHADE_CLASS_OPBR_BASE)) | ((shadeMask >> SHADE_CLASS_OPBR_BASE) & 1u) << 2;
    for (uint32_t klass = 0; klass < MAT_CLASS_COUNT; klass++) {
      if (!(shadeMask & (1u << klass))) continue;
      tm.timed(st, StageTimers::SHADE, [&] {
        launchShade(st, plan.wideBlocks, klass, (s->shadeClassTextured & (1u << klass)) != 0u, rs.mediumStackSize != 0u, U, f.view, f.ps, f.qs, D.dCounters.ptr,
                    par);
      });
    }
    if (nee) {
      // not chosen yet: alternate, and count (chooseShadowOrder)
      const int32_t order = sch.shadowOrderNow >= 0 ? sch.shadowOrderNow : (int32_t)(tm.totalIters & 1u);
      hipStream_t on = st;
      if (two) { // the shadow launch moves to the second stream, behind this iteration's k_shade
        HIP_TRY(hipEventRecord(D.evShade, st)); HIP_TRY(hipStreamWaitEvent(st2, D.evShade, 0));
        if (sch.twoStreamDelay == 2) launchSpin(st2, 300000ull);
        on = st2;
      }
      tm.timed(on, StageTimers::SHADOW, [&] {
        launchTrace(on, plan.traceBlocks, true, s->countTraversal, f.view, f.ps, f.qs, D.dCounters.ptr, Q_SHADOW, Q_SHADOW,
                    sch.dynRefill | (order ? TRACE_DYN_SLOT_ORDER : 0u), plan.wideBlocks, U, D.sampleBuf.ptr);
      });
      if (two) { shadowInFlight = true; HIP_TRY(hipEventRecord(D.evShadow, st2)); }
    }
    // (GATLING_ITER_LOG, with kernel timers on every iteration: what each iteration's queues held -- one sync per iteration, for measurements only)
    if (tm.iterLog) {
      HIP_TRY(hipMemcpyAsync(D.hCounters, D.dCounters.ptr, sizeof(PaddedCounter) * Q_COUNT * NSHARD, hipMemcpyDeviceToHost, st));
      HIP_TRY(hipStreamSynchronize(st));
      auto total = [&](uint32_t q) { uint64_t n = 0; for (uint32_t k = 0; k < NSHARD; k++) n += D.hCounters->count[q][k].v; return n; };
      uint64_t hits = 0; for (uint32_t c = 0; c < MAT_CLASS_COUNT; c++) hits += total(Q_HIT + c);
      tm.iterRows.push_back({tm.ev, total(Q_TRACE_A + par), hits, total(Q_SHADOW), total(Q_REGEN_A + (par ^ 1u)), total(Q_TRACE_A + (par ^ 1u))});
    }
    f.iters++; tm.totalIters++;
  }
  HIP_TRY(joinShadow()); // (a batch that ended through the poll: its last shadow launches were empty)
  accumulateBatch(f, batch);
  return GI_C_OK;
}

// --- epilogue: the path-following AOVs are finished on the host (NEE resolve on the device, ClockCycles heat map, Bounces NaN fill) and their rows read back
static int finishPathAovs(Frame& f, const BoundAovs& A)
{
  SceneDevice& D = f.D; const RenderJob& job = f.job; hipStream_t st = f.st;
  const size_t pixels = f.pixels; const uint32_t width = job.width, rowBegin = job.rowBegin, rowStride = job.rowStride;
  if (A.nee && f.ps.neeKey) launchResolveNee(st, f.U, D.neeKey.ptr, reinterpret_cast<F4*>(rbMem(A.nee, D.slot)), (uint32_t)pixels);
  if (GiCRenderBuffer* clockRb = A.clock) {
    // ClockCycles: per-pixel cost -> heat map normalised to the frame maximum, on the host like _EncodeRenderBufferAsHeatmap (Gi.cpp:327-343)
    std::vector<uint32_t> counts(pixels);
    HIP_TRY(hipMemcpyAsync(counts.data(), D.pathSegments.ptr, pixels * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    float maxValue = 0.0f;
    for (uint32_t c : counts) maxValue = std::max(maxValue, (float)c);
    float* img = reinterpret_cast<float*>(clockRb->hostMem);
    for (size_t p = 0; p < pixels; p++) {
      const size_t y = rowBegin + (p / width) * rowStride, x = p % width;
      float* o = img + (y * width + x) * 4;
      if (maxValue > 0.0f) {
        const int idx = std::min((int)(((float)counts[p] / maxValue) * 255.0), 255);
        turboColormap((float)idx / 255.0f, o);
        o[3] = 255.0f;
      } else { o[0] = (float)counts[p]; o[1] = 0.0f; o[2] = 0.0f; }
    }
    HIP_TRY(hipMemcpyAsync(rbMem(clockRb, D.slot), clockRb->hostMem, clockRb->size, hipMemcpyHostToDevice, st));
  }
  if (A.bounces && f.U.maxBounces == 0u) { // rp_main.rgen:483-486 evaluates inferno(0 / 0) = NaN for every pixel of the tile
    float* img = reinterpret_cast<float*>(A.bounces->hostMem);
    for (size_t p = 0; p < pixels; p++) { float* o = img + ((rowBegin + (p / width) * rowStride) * width + p % width) * 4; o[0] = o[1] = o[2] = NAN; }
    HIP_TRY(hipMemcpyAsync(rbMem(A.bounces, D.slot), A.bounces->hostMem, A.bounces->size, hipMemcpyHostToDevice, st));
  }
  for (GiCRenderBuffer* rb : {A.nee, A.bounces}) {
    if (!rb || rb->deviceOnly || !job.readback) continue;
    HIP_TRY(copyTileRows(rb, rb->stride, job, D.slot, st));
  }
  return GI_C_OK;
}

// the non-colour AOV pass (k_aov) + read-back of the rows of this tile
static int runAovPass(Frame& f, const BoundAovs& A)
{
  launchAov(f.st, f.U, f.view, A.targets);
  if (hipGetLastError() != hipSuccess) { setError("k_aov launch failed"); return GI_C_ERROR; }
  for (GiCRenderBuffer* rb : A.produced) {
    if (rb->deviceOnly || !f.job.readback) continue;
    HIP_TRY(copyTileRows(rb, rb->stride, f.job, f.D.slot, f.st));
  }
  return GI_C_OK;
}

// the counters and the colour rows come back, and the render ends: everything this device was given has run
static int readBackAndWait(Frame& f, GiCRenderBuffer* colorRb)
{
  SceneDevice& D = f.D;
  HIP_TRY(hipMemcpyAsync(D.hCounters, D.dCounters.ptr, sizeof(Counters), hipMemcpyDeviceToHost, f.st));
  if (colorRb && !colorRb->deviceOnly && f.job.readback) HIP_TRY(copyTileRows(colorRb, 16, f.job, D.slot, f.st));
  if (f.moments && !f.moments->deviceOnly && f.job.readback) HIP_TRY(copyTileRows(f.moments, 16, f.job, D.slot, f.st));
  HIP_TRY(hipStreamSynchronize(f.st));
  HIP_TRY(hipGetLastError());
  return GI_C_OK;
}

static void fillStats(const Frame& f, double tEnd)
{
  GiCRenderStats& S = f.D.stats; const Counters& c = *f.D.hCounters;
  S.renderMs = tEnd - f.tStart; S.samples = (uint64_t)f.pixels * f.rs.spp; S.iterations = f.iters; S.traceLaunches = f.traceLaunches;
  uint64_t* W = f.D.pathWalkStats; // giCDebugPathWalkStats (all zero unless a counting build's k_path ran in this render)
  for (int k = 0; k < 18; k++) W[k] = 0u;
  for (int k = 0; k < 9; k++) f.D.pathLobeStats[k] = 0u; // giCDebugPathLobeStats, likewise
  for (int k = 0; k < 5; k++) f.D.pathRingStats[k] = 0u; // giCDebugPathRingStats, likewise
  for (int k = 0; k < 4; k++) f.D.traversalStackHigh[k] = 0u; // giCDebugTraversalStackHigh, likewise
  if (f.served) { // nothing was launched but the fold: the counters on the device are still those of the call that traced the window
    S.fusedPath = S.batches = S.poolSlots = 0u;
    S.segments = S.shadowRays = S.nodesVisited = S.trisTested = S.shadowNodesVisited = S.shadowTrisTested = 0u;
    return;
  }
  S.fusedPath = f.plan.fused ? 1u : 0u;
  S.segments = c.segments + f.skippedSegments; S.shadowRays = c.shadowRays; S.nodesVisited = c.nodesVisited; S.trisTested = c.trisTested;
  S.shadowNodesVisited = c.shadowNodesVisited; S.shadowTrisTested = c.shadowTrisTested;
  W[0] = c.phaseTrips; W[17] = c.walkFewLaneSteps;
  for (int k = 0; k < 9; k++) f.D.pathLobeStats[k] = c.lobeStats[k];
  for (int k = 0; k < 5; k++) f.D.pathRingStats[k] = c.ringStats[k];
  if (f.stackHighCounted) {
    bool spills = false;
    const uint32_t rows = f.plan.fused ? pathLotPlacement(f.view.bvhDepth).stack : traceStackRows(f.view, spills);
    const uint32_t high = std::max(c.stackHigh[0], c.stackHigh[1]);
    uint32_t* H = f.D.traversalStackHigh;
    H[0] = c.stackHigh[0]; H[1] = c.stackHigh[1]; H[2] = rows; H[3] = spills && high > rows ? high - rows : 0u;
  }
  for (int k = 0; k < 8; k++) { W[1 + k] = c.walkStepTrips[k]; W[9 + k] = c.walkStepLanes[k]; }
}

// giCDebugMissRect: the rectangle scheduleFrame would give a whole-frame render of this camera over these bounds (before the rules that switch it off: options,
// debug AOVs, look-ahead windows).  Host only: no device, no scene.  out = x0, y0, x1, y1; an empty rectangle is 0, 0, 0, 0.
extern "C" int giCDebugMissRect(const float* bounds, const GiCCameraDesc* camera, const GiCRenderSettings* settings, uint32_t width, uint32_t height, uint32_t* out)
{
  if (!bounds || !camera || !settings || !out || width == 0u || height == 0u) { setError("giCDebugMissRect: bad arguments"); return GI_C_ERROR; }
  FrameUniforms U{};
  cameraUniforms(*camera, width, height, U);
  U.flags = samplingFlags(*settings);
  const MissRect r = computeMissRect(bounds, bounds + 3, U, width, height);
  out[0] = r.x0; out[1] = r.y0; out[2] = r.x1; out[3] = r.y1;
  return GI_C_OK;
}

// choose the shadow walks' order once both have been measured on enough rays of this scene: fewer node visits per ray wins
static void chooseShadowOrder(GiCScene* s, const Counters& c)
{
  if (s->shadowOrder.load() >= 0) return;
  for (int m = 0; m < 2; m++) {
    s->shadowOrderRays[m] += c.shadowOrderRays[m];
    for (int k = 0; k < 16; k++) s->shadowOrderSteps[m] += c.shadowOrderSteps[m][k].v;
  }
  constexpr uint64_t ENOUGH = 1u << 16;
  if (s->shadowOrderRays[0] < ENOUGH || s->shadowOrderRays[1] < ENOUGH) return;
  s->shadowOrder = (double)s->shadowOrderSteps[1] * (double)s->shadowOrderRays[0] < (double)s->shadowOrderSteps[0] * (double)s->shadowOrderRays[1] ? 1 : 0;
  if (getenv("GATLING_BUILD_TIMING")) {
    fprintf(stderr, "[gatling_gi] shadow walks: near-to-far %.3f node visits per ray (%llu rays), slot order %.3f (%llu rays) -> %s\n",
            (double)s->shadowOrderSteps[0] / (double)s->shadowOrderRays[0], (unsigned long long)s->shadowOrderRays[0],
            (double)s->shadowOrderSteps[1] / (double)s->shadowOrderRays[1], (unsigned long long)s->shadowOrderRays[1],
            s->shadowOrder.load() ? "slot order" : "near-to-far");
  }
}

// counting builds with GATLING_OPTIONS=phase_stats=1: k_path's phase split, k_trace_dyn's lane accounting
static void printPhaseStats(const GiCScene* s, const Counters& c)
{
  if (!s->countTraversal || !optionValue("phase_stats", 0)) return;
  if (c.phaseTrips) { // k_path's phase split
    const double tot = (double)(c.phaseCycles[0] + c.phaseCycles[1] + c.phaseCycles[2] + c.phaseCycles[3]);
    static const char* names[4] = {"regen", "trace", "shade", "shadow+finish"};
    for (int k = 0; k < 4; k++) {
      fprintf(stderr, "[gatling_gi] k_path phase %-14s %5.1f %% of wave cycles, %5.1f of 64 lanes busy per trip\n", names[k],
              100.0 * (double)c.phaseCycles[k] / tot, (double)c.phaseLanes[k] / (double)c.phaseTrips);
    }
    fprintf(stderr, "[gatling_gi] k_path trips %llu, %.0f cycles per trip and wave\n", (unsigned long long)c.phaseTrips, tot / (double)c.phaseTrips);
    unsigned long long steps = 0ull;
    for (int k = 0; k < 8; k++) steps += c.walkStepTrips[k];
    for (int k = 0; k < 8 && c.walkStepTrips[k]; k++) {
      fprintf(stderr, "[gatling_gi] k_path walk step %d%s reached by %5.1f %% of the trips (%4.1f %% of all wave steps), %5.2f of 64 lanes walking\n", k,
              k == 7 ? "+" : " ", 100.0 * (double)c.walkStepTrips[k] / (double)c.phaseTrips, 100.0 * (double)c.walkStepTrips[k] / (double)steps,
              (double)c.walkStepLanes[k] / (double)c.walkStepTrips[k]);
    }
  }
  if (c.dynStats[0]) { // k_trace_dyn's lane accounting (closest-hit launches)
    const unsigned long long* d = c.dynStats; const double st = (double)d[0];
    fprintf(stderr, "[gatling_gi] k_trace_dyn<closest> %llu wave steps: per step %.1f lanes hold a ray, %.1f run the node test, %.1f wait for the triangle "
                    "ring; %.3f batches per step of %.1f pairs; "
                    "a refill every %.2f steps, %.1f lanes each\n",
            d[0], (double)d[1] / st, (double)d[2] / st, (double)d[3] / st, (double)d[4] / st, d[4] ? (double)d[5] / (double)d[4] : 0.0,
            d[6] ? st / (double)d[6] : 0.0, d[6] ? (double)d[7] / (double)d[6] : 0.0);
  }
}


// ---------------------------------------------------------------------------------------------------------------
// Sample look-ahead (GI_C_SCENE_OPTION_SAMPLE_LOOKAHEAD, GATLING_OPTIONS=lookahead=N).  A path's arithmetic depends on its GLOBAL sample
// index alone, never on spp (the Bounces AOV apart), so K consecutive progressive calls of spp samples are, to the path kernels, one batch of K * spp samples
// starting at the first call's sample offset -- only the fold into the image differs per call.  planLookahead decides what this call does with that:
//   serve   the device holds a window traced with exactly what this call would trace with, and this call's samples are the next in it: fold them
//           (serveFromWindow), launch nothing else of the colour pass;
//   trace   a window of `calls` calls -- 1 after any reset (the first frame after an edit costs what it costs today), then 2, 4, 8 ... N as long as every call
//           continues the previous window -- through the colour pass with batchSamples = calls * spp, as ONE batch (traceColour bounds it by the memory plan);
//   decline calls == 0: the call renders as without the option and leaves no window.
// Validity is never inferred from which setter ran: the window keeps what it was traced WITH (LookaheadKey) and the call compares what it would trace with.
// ---------------------------------------------------------------------------------------------------------------
struct LookaheadPlan { bool serve = false; uint32_t calls = 0; LookaheadKey key{}; };

static long lookaheadOption(const GiCScene* s)
{
  const long o = optionSet("lookahead") ? optionValue("lookahead", -1) : -1;
  return o >= 0 ? o : (long)s->optLookahead;
}

static LookaheadPlan planLookahead(Frame& f, const BoundAovs& A)
{
  Lookahead& L = f.D.lookahead;
  const GiCRenderSettings& rs = f.rs;
  LookaheadPlan la;
  const uint64_t N = (uint64_t)std::max(0L, lookaheadOption(f.s));
  // the path-following AOVs read path state when a sample retires, Bounces reads U.spp: such renders keep today's form
  if (N < 2u || !rs.progressiveAccumulation || A.nee || A.bounces || A.clock) { L.drop(); return la; }
  memset(&la.key, 0, sizeof(la.key));
  la.key.U = f.U; la.key.view = f.view; la.key.generation = f.s->generation;
  la.key.U.sampleOffset = 0u; la.key.U.sampleOffsetF = 0.0f; la.key.U.invTotalSampleCount = 0.0f; // (spp, invSpp, sppF stay: another spp is another window)
  // this call's samples are the next the previous window's calls left off at, and everything else is what that window was traced with
  const bool continues = L.valid && (uint64_t)f.U.sampleOffset == (uint64_t)L.firstOffset + (uint64_t)L.served * rs.spp
                         && memcmp(&la.key.U, &L.key.U, sizeof(FrameUniforms)) == 0 && memcmp(&la.key.view, &L.key.view, sizeof(SceneView)) == 0
                         && la.key.generation == L.key.generation;
  if (continues && L.served < L.calls) { la.serve = true; la.calls = L.calls; return la; }
  // a new window: twice the previous one's calls if this call continues it, else one call.  One batch: 32-bit work ids, and the sample index must not wrap
  uint64_t want = continues ? std::min<uint64_t>(N, 2ull * L.calls) : 1ull;
  want = std::min<uint64_t>(want, 0xffffffffull / ((uint64_t)f.pixels * rs.spp));
  want = std::min<uint64_t>(want, (0xffffffffull - f.U.sampleOffset) / rs.spp);
  L.drop(); // (whatever this call traces is written over the old window)
  la.calls = (uint32_t)std::max<uint64_t>(1, want);
  return la;
}

// the serve phase: this call's spp samples out of the window, blended with its own sample offset
static int serveFromWindow(Frame& f, const BoundAovs& A)
{
  SceneDevice& D = f.D; Lookahead& L = D.lookahead;
  const uint64_t windowSamples = (uint64_t)L.calls * f.rs.spp, first = (uint64_t)L.served * f.rs.spp;
  if (!D.sampleBuf.ptr || (uint64_t)f.pixels * windowSamples > D.sampleBuf.count || first + f.rs.spp > windowSamples) {
    setError("giCRender: the look-ahead window does not lie inside the per-sample buffer (internal error)");
    return GI_C_ERROR;
  }
  f.served = true;
  f.colorOut = reinterpret_cast<F4*>(rbMem(A.color, D.slot));
  launchFoldWindow(f.st, f.U, D.sampleBuf.ptr, f.colorOut, (uint32_t)windowSamples, (uint32_t)first, L.pixelMajor != 0u);
  if (hipGetLastError() != hipSuccess) { setError("k_fold_window launch failed"); return GI_C_ERROR; }
  if (f.moments) { // the moments ride along with the window: the same slice
    launchMoments(f.st, f.U, D.sampleBuf.ptr, reinterpret_cast<F4*>(rbMem(f.moments, D.slot)), (uint32_t)windowSamples, (uint32_t)first, f.rs.spp,
                  L.pixelMajor != 0u, f.job.momentsContinue);
    if (hipGetLastError() != hipSuccess) { setError("k_moments launch failed"); return GI_C_ERROR; }
  }
  L.served++; L.callsServed++; L.traced = 0u;
  return GI_C_OK;
}

// the colour pass: the memory plan, the schedule, the batches -- the call's own spp samples, or (la.calls >= 2) a look-ahead window of la.calls * spp samples
// as one batch, of which this call folds the first spp -- and the path-following AOVs
static int traceColour(Frame& f, const BoundAovs& aov, const LookaheadPlan& la)
{
  GiCScene* s = f.s; SceneDevice& D = f.D; const DevCtx& ctx = f.ctx; const GiCRenderSettings& rs = f.rs; hipStream_t st = f.st;
  const size_t pixels = f.pixels;
  D.lookahead.traced = 1u;
  const PlanInputs in{pixels, (uint32_t)ctx.cuCount, traceBlocksPerCu(f.view)};
  if (allocatePathPlan(s, D, rs, (uint64_t)std::max(1u, la.calls) * rs.spp, f.view, in, f.plan) != GI_C_OK) return GI_C_ERROR;
  const uint64_t batchSamples = f.plan.batchSamples;
  // the window is what the plan's buffer holds of it (SAMPLE_BUFFER_MB, assume_free_mb, the shrink on out-of-memory); a call that needs several batches
  // itself declines
  const uint32_t calls = (uint32_t)std::min<uint64_t>(la.calls, batchSamples / rs.spp);
  f.windowCalls = calls >= 2u ? calls : 0u;
  const uint64_t samples = calls >= 2u ? (uint64_t)calls * rs.spp : (uint64_t)rs.spp;
  f.numBatches = (uint32_t)((samples + batchSamples - 1) / batchSamples);
  D.stats.poolSlots = f.plan.fused ? 0u : (uint32_t)f.plan.slots; D.stats.batches = f.numBatches;
  if (bindPathAovs(f, aov) != GI_C_OK) return GI_C_ERROR;
  f.sch = scheduleFrame(f);
  f.qs = makeQueueSet(&D);
  f.colorOut = reinterpret_cast<F4*>(rbMem(aov.color, D.slot));

  HIP_TRY(hipStreamSynchronize(st));
  f.tStart = nowMs();
  if (f.sch.twoStreamOk && !D.evShade) {
    HIP_TRY(hipEventCreateWithFlags(&D.evShade, hipEventDisableTiming));
    HIP_TRY(hipEventCreateWithFlags(&D.evShadow, hipEventDisableTiming));
  }
  FrameUniforms& U = f.U;
  for (uint32_t batch = 0; batch < f.numBatches; batch++) {
    U.batchFirstSample = (uint32_t)(batch * batchSamples);
    U.batchSamples = (uint32_t)std::min<uint64_t>(batchSamples, samples - (uint64_t)batch * batchSamples);
    U.workTotal = (uint32_t)(pixels * U.batchSamples);
    if (f.plan.fused && U.maxBounces > 0u) { // the fused kernel's work items are the active rectangle's pixels (scheduleFrame); a skipped sample is one segment
      U.workTotal = (uint32_t)((uint64_t)U.activeCount * U.batchSamples);
      f.skippedSegments += (uint64_t)(pixels - U.activeCount) * U.batchSamples;
    }
    f.ps.neeSampleBase = U.batchFirstSample;
    const uint32_t poolNow = (uint32_t)std::min<uint64_t>(f.plan.slots, U.workTotal);
    U.poolSlots = poolNow;
    launchInit(st, f.ps, f.qs, D.dCounters.ptr, f.plan.fused ? 0u : poolNow, batch == 0);
    if (batch == 0 && s->countTraversal) { // (Counters::stackHigh is not k_init's to zero: that kernel is shared with the builds that do not count)
      HIP_TRY(hipMemsetAsync(D.dCounters.ptr->stackHigh, 0, sizeof(Counters::stackHigh), st));
      f.stackHighCounted = U.maxBounces != 0u;
    }
    const int rc = U.maxBounces == 0u ? runZeroBounceBatch(f, batch) : f.plan.fused ? runFusedBatch(f, batch) : runWavefrontBatch(f, batch, poolNow);
    if (rc != GI_C_OK) return rc;
  }
  if (calls >= 1u) { // what the device now holds (a window of one call holds nothing: it is where the ramp starts)
    Lookahead& L = D.lookahead;
    L.valid = true; L.calls = calls; L.served = 1u; L.firstOffset = U.sampleOffset; L.pixelMajor = (U.flags & FLAG_PIXEL_MAJOR) ? 1u : 0u; L.key = la.key;
    L.windowsTraced++;
  }
  U.flags &= ~FLAG_TWO_STREAM;
  return finishPathAovs(f, aov);
}

static int renderOnDevice(GiCScene* s, SceneDevice& D, const RenderJob& job)
{
  const DevCtx& ctx = g_ctx.devs[D.slot];
  HIP_TRY(hipSetDevice(ctx.device));
  hipStream_t st = ctx.stream;
  const GiCRenderSettings& rs = job.params->renderSettings;
  D.stats.bvhBuildMs = s->stats.bvhBuildMs; D.stats.uploadMs = s->stats.uploadMs;

  BoundAovs aov;
  if (bindAovs(D, job, st, aov) != GI_C_OK) return GI_C_ERROR;
  if (!aov.color && aov.produced.empty()) { HIP_TRY(hipStreamSynchronize(st)); return GI_C_OK; } // (nothing this library produces is bound)
  const size_t pixels = (size_t)job.tileRows * job.width;
  if (pixels == 0) return GI_C_OK;

  Frame f{s, D, ctx, job, rs, st, pixels, StageTimers(s, D)};
  f.U = makeUniforms(*job.params, job, s);
  f.tStart = nowMs();
  f.moments = aov.color ? aov.moments : nullptr;
  f.view = makeFrameView(s, D, *job.params, f.U);
  if (ensurePathState(&D, 1, 1, 1) != GI_C_OK) return GI_C_ERROR; // counters / pinned mirror exist even for AOV-only renders
  LookaheadPlan la;
  if (aov.color) {
    f.view.mediumStackSize = rs.mediumStackSize;
    la = planLookahead(f, aov);
    const int rc = la.serve ? serveFromWindow(f, aov) : traceColour(f, aov, la);
    if (rc != GI_C_OK) { D.lookahead.drop(); return rc; }
  }
  if (!aov.produced.empty() && runAovPass(f, aov) != GI_C_OK) { D.lookahead.drop(); return GI_C_ERROR; }
  if (readBackAndWait(f, aov.color) != GI_C_OK) { D.lookahead.drop(); return GI_C_ERROR; }
  const double tEnd = nowMs();

  fillStats(f, tEnd);
  // (aov.color: an AOV-only render never ran k_init -- the counters would be the previous render's; so would a served call's)
  if (D.slot == 0u && aov.color && !f.served) chooseShadowOrder(s, *D.hCounters);
  if (!f.served) printPhaseStats(s, *D.hCounters);
  if (D.hCounters->overflow && !f.served) {
    D.lookahead.drop();
    setError("giCRender: a work-queue shard overflowed its capacity (internal sizing error); the image is invalid");
    return GI_C_ERROR;
  }
  f.tm.finish(D.stats);
  return GI_C_OK;
}

// The frame on nDev devices: rows d, d + nDev, ... on device d (interleaved shares cost the same), every device from its own host thread;
// then the shares of devices 1 .. n-1 are copied INTO PLACE in the primary device's render buffers (strided 2-D peer copies over xGMI: no staging buffer, no
// re-interleave pass) and the primary does the one D2H.  Per-pixel arithmetic does not depend on which device renders a row (RNG streams use the global
// pixel index), so the image is bit-identical to a one-device render.
static int renderOnDevices(GiCScene* s, uint32_t nDev, const RenderJob& frame)
{
  const GiCRenderParams* params = frame.params;
  // per-device copies of every bound render buffer
  for (uint32_t i = 0; i < params->aovBindingCount; i++) {
    GiCRenderBuffer* rb = params->aovBindings[i].renderBuffer;
    if (rb->replicaMem.size() + 1u < g_ctx.devs.size()) rb->replicaMem.resize(g_ctx.devs.size() - 1u, nullptr);
    for (uint32_t d = 1; d < nDev; d++) {
      if (rb->replicaMem[d - 1u]) continue;
      HIP_TRY(hipSetDevice(g_ctx.devs[d].device));
      HIP_TRY(hipMalloc(&rb->replicaMem[d - 1u], rb->size ? rb->size : 16));
      HIP_TRY(hipMemset(rb->replicaMem[d - 1u], 0, rb->size ? rb->size : 16));
    }
  }
  HIP_TRY(hipSetDevice(g_ctx.device));
  std::vector<int> rcs(nDev, GI_C_OK); std::vector<std::string> errs(nDev);
  auto work = [&](uint32_t d) {
    RenderJob job = frame;
    job.rowBegin = d; job.rowEnd = frame.height; job.rowStride = nDev; job.tileRows = (frame.height - d + nDev - 1u) / nDev; job.readback = false;
    try { rcs[d] = renderOnDevice(s, sceneDevice(s, d), job); }
    catch (const std::exception& e) { rcs[d] = GI_C_ERROR; t_lastError = e.what(); }
    if (rcs[d] != GI_C_OK) errs[d] = t_lastError; // (thread-local)
  };
  {
    std::lock_guard<std::mutex> own(g_ctx.workerMutex);
    while (g_ctx.workers.size() + 1u < nDev) { g_ctx.workers.emplace_back(new DeviceWorker()); g_ctx.workers.back()->start(); }
    for (uint32_t d = 1; d < nDev; d++) g_ctx.workers[d - 1u]->post([&work, d] { work(d); });
    work(0u);
    for (uint32_t d = 1; d < nDev; d++) g_ctx.workers[d - 1u]->wait();
  }
  HIP_TRY(hipSetDevice(g_ctx.device));
  for (uint32_t d = 0; d < nDev; d++) if (rcs[d] != GI_C_OK) { setError("device " + std::to_string(g_ctx.devs[d].device) + ": " + errs[d]); return GI_C_ERROR; }
  // gather: rows d::nDev of device d -> the same rows of the primary's buffer, then the D2H of the whole frame
  hipStream_t st = g_ctx.stream;
  for (uint32_t i = 0; i < params->aovBindingCount; i++) {
    GiCRenderBuffer* rb = params->aovBindings[i].renderBuffer;
    const size_t rowBytes = (size_t)rb->width * rb->stride, pitch = rowBytes * nDev;
    for (uint32_t d = 1; d < nDev; d++) {
      const uint32_t rows = (rb->height - d + nDev - 1u) / nDev;
      const size_t off = (size_t)d * rowBytes;
      if (g_ctx.devs[d].peer == 1 && optionValue("peer_copies", 1) != 0) { // strided 2-D peer copy over xGMI, straight into place
        HIP_TRY(hipMemcpy2DAsync((uint8_t*)rb->deviceMem + off, pitch, (uint8_t*)rb->replicaMem[d - 1u] + off, pitch, rowBytes, rows, hipMemcpyDefault, st));
      } else { // no peer access (or GATLING_OPTIONS=peer_copies=0): the share's rows -> pinned staging frame -> the primary's buffer, both strided, in place
        if (!rb->stageMem) HIP_TRY(hipHostMalloc(&rb->stageMem, rb->size ? rb->size : 16, hipHostMallocPortable));
        HIP_TRY(hipSetDevice(g_ctx.devs[d].device));
        HIP_TRY(hipMemcpy2DAsync((uint8_t*)rb->stageMem + off, pitch, (uint8_t*)rb->replicaMem[d - 1u] + off, pitch, rowBytes, rows, hipMemcpyDeviceToHost,
            g_ctx.devs[d].stream));
        HIP_TRY(hipStreamSynchronize(g_ctx.devs[d].stream));
        HIP_TRY(hipSetDevice(g_ctx.device));
        HIP_TRY(hipMemcpy2DAsync((uint8_t*)rb->deviceMem + off, pitch, (uint8_t*)rb->stageMem + off, pitch, rowBytes, rows, hipMemcpyHostToDevice, st));
      }
    }
    if (!rb->deviceOnly) HIP_TRY(hipMemcpyAsync(rb->hostMem, rb->deviceMem, rb->size, hipMemcpyDeviceToHost, st));
  }
  HIP_TRY(hipStreamSynchronize(st));
  // statistics: counts add up, times are the slowest device's
  GiCRenderStats S = s->stats; // (device 0's, written by its renderOnDevice)
  for (uint32_t d = 1; d < nDev; d++) {
    const GiCRenderStats& R = sceneDevice(s, d).stats;
    S.samples += R.samples; S.segments += R.segments; S.shadowRays += R.shadowRays; S.nodesVisited += R.nodesVisited; S.trisTested += R.trisTested;
    S.shadowNodesVisited += R.shadowNodesVisited; S.shadowTrisTested += R.shadowTrisTested;
    S.renderMs = std::max(S.renderMs, R.renderMs); S.traceMs = std::max(S.traceMs, R.traceMs); S.shadeMs = std::max(S.shadeMs, R.shadeMs);
    S.raygenMs = std::max(S.raygenMs, R.raygenMs); S.shadowMs = std::max(S.shadowMs, R.shadowMs); S.iterations = std::max(S.iterations, R.iterations);
    S.traceLaunches = std::max(S.traceLaunches, R.traceLaunches);
  }
  s->stats = S;
  return GI_C_OK;
}

static int giCRenderImpl(const GiCRenderParams* params)
{
  if (!g_ctx.initialized) { setError("giCRender before giCInitialize"); return GI_C_ERROR; }
  if (!params || !params->scene) { setError("giCRender: null params/scene"); return GI_C_ERROR; }
  GiCScene* s = params->scene;
  const GiCRenderSettings& rs = params->renderSettings;
  const GiCAovBinding* colorBinding = nullptr;
  for (uint32_t i = 0; i < params->aovBindingCount; i++) {
    if (!params->aovBindings[i].renderBuffer) { setError("giCRender: AOV binding without render buffer"); return GI_C_ERROR; }
    if (params->aovBindings[i].renderBuffer->hostOnly) { setError("giCRender: a host render buffer (giCCreateHostRenderBuffer) cannot be rendered into"); return GI_C_ERROR; }
    if (params->aovBindings[i].aovId == GI_C_AOV_COLOR) colorBinding = &params->aovBindings[i];
  }
  if (params->aovBindingCount == 0) { setError("giCRender: no AOV bindings"); return GI_C_ERROR; }
  if (rs.spp == 0) { setError("giCRender: spp must be > 0"); return GI_C_ERROR; }
  if (rs.mediumStackSize > MAX_MEDIUM_STACK) {
    setError("giCRender: mediumStackSize > 15 cannot be addressed (the payload's medium index has four bits, rp_main_payload.glsl:4-5)");
    return GI_C_ERROR;
  }
  const GiCRenderBuffer* sizeRb = (colorBinding ? colorBinding : &params->aovBindings[0])->renderBuffer;
  const uint32_t width = sizeRb->width, height = sizeRb->height;
  if (width == 0 || height == 0) return GI_C_OK; // Render.Empty-style degenerate target: nothing to do
  if (width > 65535u || height > 65535u) { setError("giCRender: image dimensions exceed 65535 (imageDims packing, rp_main.h:38)"); return GI_C_ERROR; }
  // a camera the ray generation can use (the reference passes whatever Hydra hands it, Gi.cpp:2373-2426; a NaN there is a NaN image): refused, with the field
  // named
  {
    const GiCCameraDesc& c = params->camera;
    const float fields[] = {c.position[0], c.position[1], c.position[2], c.forward[0], c.forward[1], c.forward[2], c.up[0], c.up[1], c.up[2],
                            c.vfov, c.fStop, c.focusDistance, c.focalLength, c.clipStart, c.clipEnd, c.exposure};
    for (float f : fields) if (!std::isfinite(f)) { setError("giCRender: the camera has a non-finite field"); return GI_C_ERROR; }
    const float f2 = (c.forward[0] * c.forward[0] + c.forward[1] * c.forward[1]) + c.forward[2] * c.forward[2],
        u2 = (c.up[0] * c.up[0] + c.up[1] * c.up[1]) + c.up[2] * c.up[2];
    if (!(f2 > 0.0f) || !(u2 > 0.0f) || !std::isfinite(f2) || !std::isfinite(u2) || !std::isfinite(1.0f / sqrtf(f2)) || !std::isfinite(1.0f / sqrtf(u2))) {
      setError("giCRender: the camera's forward or up vector cannot be normalised (zero, denormal or overflowing length)");
      return GI_C_ERROR;
    }
    if (!(c.vfov > 0.0f && c.vfov < 3.14159265f)) { setError("giCRender: the camera's vertical field of view must lie inside (0, pi) radians");
        return GI_C_ERROR; }
    if (!std::isfinite(1.0f / (2.0f * tanf(c.vfov * 0.5f)))) {
      setError("giCRender: the camera's vertical field of view is too small for the image plane distance to be finite");
      return GI_C_ERROR;
    }
  }
  if (const GiCDomeLight* dl = params->domeLight) { // (the dome light's setters take whatever they are given, like the reference's)
    const float fields[] = {dl->rotation[0], dl->rotation[1], dl->rotation[2], dl->rotation[3], dl->baseEmission[0], dl->baseEmission[1], dl->baseEmission[2],
        dl->diffuse, dl->specular};
    for (float f : fields) if (!std::isfinite(f)) { setError("giCRender: the dome light has a non-finite field"); return GI_C_ERROR; }
  }
  { // render settings that enter the arithmetic as floats
    const float fields[] = {rs.rrInvMinTermProb, rs.lightIntensityMultiplier, rs.metersPerSceneUnit, rs.frame};
    for (float f : fields) if (!std::isfinite(f)) { setError("giCRender: the render settings have a non-finite field"); return GI_C_ERROR; }
    if (std::isnan(rs.maxSampleValue)) { setError("giCRender: maxSampleValue is NaN"); return GI_C_ERROR; } // (+inf: no clamp)
  }
  uint32_t rowBegin = params->rowBegin, rowEnd = params->rowEnd ? params->rowEnd : height;
  const uint32_t rowStride = params->rowStride ? params->rowStride : 1u;
  if (rowBegin > rowEnd || rowEnd > height) { setError("giCRender: bad row range"); return GI_C_ERROR; }
  const uint32_t tileRows = rowEnd > rowBegin ? (rowEnd - rowBegin + rowStride - 1u) / rowStride : 0u; // rows rowBegin + k * rowStride < rowEnd

  std::lock_guard<std::mutex> guard(s->mutex);
  HIP_TRY(hipSetDevice(g_ctx.device));

  // --- dirty handling (_CalcDirtyFlagsForRenderParams, Gi.cpp:1859-1987; sample offset reset :2125-2129)
  uint8_t clear[GI_C_MAX_AOV_COMP_SIZE] = {0};
  if (colorBinding) memcpy(clear, colorBinding->clearValue, GI_C_MAX_AOV_COMP_SIZE);
  const float* domeEm = params->domeLight ? params->domeLight->baseEmission : nullptr;
  if (!s->haveOldParams || memcmp(&s->oldCamera, &params->camera, sizeof(GiCCameraDesc)) != 0 || !settingsEqual(s->oldSettings, rs) ||
      memcmp(s->oldClear, clear, sizeof(clear)) != 0 || s->oldRowBegin != rowBegin || s->oldRowEnd != rowEnd || s->oldRowStride != rowStride
          || s->oldDome != params->domeLight ||
      (domeEm && memcmp(domeEm, s->oldDomeEmission, 12) != 0))
    s->dirty |= DIRTY_FRAMEBUFFER;
  s->haveOldParams = true; s->oldCamera = params->camera; s->oldSettings = rs; memcpy(s->oldClear, clear, sizeof(clear));
  s->oldRowBegin = rowBegin; s->oldRowEnd = rowEnd; s->oldRowStride = rowStride; s->oldDome = params->domeLight;
  if (domeEm) memcpy(s->oldDomeEmission, domeEm, 12);

  s->stats.bvhBuildMs = 0.0; s->stats.uploadMs = 0.0; s->stats.nodeCount = s->nodeCount; s->stats.triangleCount = s->triCount;
  if (syncSceneGeometry(s) != GI_C_OK) return GI_C_ERROR;
  if (s->dirty & DIRTY_LIGHTS) { if (uploadLights(s) != GI_C_OK) return GI_C_ERROR; s->dirty &= ~DIRTY_LIGHTS; s->dirty |= DIRTY_FRAMEBUFFER; }
  if (!rs.progressiveAccumulation) s->dirty |= DIRTY_FRAMEBUFFER;
  // --- one device, or the rows dealt to all of them
  // Multi-device: a whole-frame render (the caller does not shard rows itself) with at least as many rows as devices.  ClockCycles is normalised to the
  // frame maximum on the host (Gi.cpp:327-343), a cross-device reduction nobody needs fast: such renders stay on the primary device.
  bool wantsClock = false;
  for (uint32_t i = 0; i < params->aovBindingCount; i++) if (params->aovBindings[i].aovId == GI_C_AOV_CLOCK_CYCLES) wantsClock = true;
  uint32_t nDev = std::min<uint32_t>(sceneDeviceCount(s), (uint32_t)s->replicas.size() + 1u);
  if (rowStride != 1u || rowBegin != 0u || rowEnd != height || wantsClock || height < nDev) nDev = 1u;
  // every device blends progressive frames against ITS OWN copy of the render buffers: when the device count of this call differs from the previous call's
  // (a ClockCycles binding came or went, the DEVICES option changed) the copies disagree, so the accumulation restarts
  if (s->lastRenderDevices != nDev) s->dirty |= DIRTY_FRAMEBUFFER;
  s->lastRenderDevices = nDev;
  if (s->dirty & DIRTY_FRAMEBUFFER) { s->sampleOffset = 0; s->dirty &= ~DIRTY_FRAMEBUFFER; }
  // a new accumulation: its own number, process-wide (a scene allocated where a destroyed one lay never repeats one), so that what a buffer holds of an
  // earlier accumulation -- the moments AOV -- is never continued by this one, whatever the sample offsets happen to be
  if (s->sampleOffset == 0u) { static std::atomic<uint64_t> nextAccumEpoch{1}; s->accumEpoch = nextAccumEpoch.fetch_add(1); }


  RenderJob job{params, colorBinding, width, height, rowBegin, rowEnd, rowStride, tileRows, {0}, true};
  memcpy(job.clear, clear, sizeof(job.clear));
  // the moments AOV continues what its buffer holds only if that is the moments of THIS accumulation's samples [0, sampleOffset) (gi_moments.h)
  GiCRenderBuffer* momentsRb = nullptr;
  for (uint32_t i = 0; i < params->aovBindingCount; i++) if (params->aovBindings[i].aovId == GI_C_AOV_EXT_MOMENTS) momentsRb = params->aovBindings[i].renderBuffer;
  job.momentsContinue = momentsRb && rs.progressiveAccumulation && s->sampleOffset > 0 && momentsRb->momentsEpoch == s->accumEpoch &&
      momentsRb->momentsNext == (uint64_t)s->sampleOffset;
  // AOVs the colour pass fills along whole paths (NEE, Bounces, ClockCycles) and unknown ids start from their clear value: host copy filled once, here
  for (uint32_t i = 0; i < params->aovBindingCount; i++) {
    const GiCAovBinding& b = params->aovBindings[i];
    GiCRenderBuffer* rb = b.renderBuffer;
    const bool pathAov = b.aovId == GI_C_AOV_NEE || b.aovId == GI_C_AOV_BOUNCES || b.aovId == GI_C_AOV_CLOCK_CYCLES || b.aovId < 0 || b.aovId >= GI_C_AOV_COUNT;
    if (b.aovId == GI_C_AOV_COLOR || !pathAov || b.aovId == GI_C_AOV_EXT_MOMENTS) continue; // (the moments have no clear value: rows outside the share stay)
    const size_t n = (size_t)rb->width * rb->height;
    for (size_t k = 0; k < n; k++) memcpy((uint8_t*)rb->hostMem + k * rb->stride, b.clearValue, rb->stride);
  }
  int rc = GI_C_OK;
  if (nDev == 1u) {
    rc = renderOnDevice(s, *s, job);
  } else {
    rc = renderOnDevices(s, nDev, job);
  }
  // whose device copy on the primary device is the whole frame now (GiCRenderBuffer::wholeFrame; giCDenoise reads such a copy in place): the colour AOV and
  // the AOVs the AOV kernels make, after a render of every row on the primary device alone
  for (uint32_t i = 0; i < params->aovBindingCount; i++) {
    const GiCAovBinding& b = params->aovBindings[i];
    const bool pathAov = b.aovId != GI_C_AOV_EXT_MOMENTS &&
        (b.aovId == GI_C_AOV_NEE || b.aovId == GI_C_AOV_BOUNCES || b.aovId == GI_C_AOV_CLOCK_CYCLES || b.aovId < 0 || b.aovId >= GI_C_AOV_COUNT);
    b.renderBuffer->wholeFrame = rc == GI_C_OK && nDev == 1u && rowStride == 1u && rowBegin == 0u && rowEnd == height && !pathAov &&
        b.renderBuffer->width == width && b.renderBuffer->height == height;
  }
  if (momentsRb) { momentsRb->momentsEpoch = rc == GI_C_OK ? s->accumEpoch : 0u; momentsRb->momentsNext = (uint64_t)s->sampleOffset + rs.spp; }
  if (rc != GI_C_OK) return rc;
  s->sampleOffset += rs.spp; // Gi.cpp:2515
  return GI_C_OK;
}


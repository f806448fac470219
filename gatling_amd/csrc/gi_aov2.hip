// gi_aov2.hip -- k_aov2, the non-colour AOVs of a two-level scene that was built without the flat tree (gfx950; GI_C_SCENE_OPTION_TLAS_ONLY, gi_build.cpp
// buildSceneTreeless).  k_aov (gi_aov.hip) finds a sample's primary hit with a per-lane walk of the flat BVH8; such a scene has none, so this kernel finds it
// with the walk the path tracer uses on this layout -- gi_traversal.h wave_step2 over the TLAS and the per-mesh BLASes, the step of k_trace_dyn2 -- and then
// runs the same per-hit body (gi_aov_body.h).  A candidate is rebuilt in world space and tested by tri_test against the world-space ray, ties go to the lower
// scene-order id under atomicMin: the hit is the flat walk's, bit for bit, and so is every AOV value.
// Built with -ffp-contract=off like every kernel unit (arithmetic contract, gi_device_math.h).

#include <type_traits>
#include <hip/hip_runtime.h>

#include "gi_device_math.h"
#include "gi_kernels.h"
#include "gi_types.h"
#include "gi_queues.h"
#include "gi_traversal.h"
#include "gi_shading.h"
#include "gi_stages.h"
#include "gi_aov_body.h"

namespace gi {

// ------------------------------------------------------------------------------------------------
// k_aov2: one pixel per lane, blocks of TRACE_BLOCK threads, one WaveTri per wave in static LDS, the 16-entry stacks in dynamic LDS (traceLdsBytes(16, 0, 0)).
// Per sample every live lane makes its camera ray (make_camera_ray: the streams k_aov and the colour pass use) and is primed as trace_dyn_body primes a lane
// it hands a ray (trav2_init, wave_ray_begin, the miss record); the wave then steps until no lane walks.  wave_step2, owner_ray and the ballots are
// wave-uniform: a lane beyond the last pixel does NOT leave the kernel -- it stays in every loop, is never alive, and only helps testing triangles.
// The result is read where the winning lane of a triangle batch left it: t from the hit key, (u, v, scene-order id | class << 28) from the record; the flat
// record of the id (SceneView::flatOfOrig; the identity on such a scene, read all the same) carries the material word traverse<> returns as outMat (TriRec::
// matFlags, the .w of the record's third 16-byte piece).  Plain C++: no hand-written assembly; the triangle test is tri_test through wave_tri_batch2.
// ------------------------------------------------------------------------------------------------
template <bool CUTOUT>
__global__ __launch_bounds__(TRACE_BLOCK) void k_aov2(FrameUniforms U, SceneView sc, AovTargets A)
{
  __shared__ WaveTri s_wave[TRACE_BLOCK / 64];
  WaveTri& W = s_wave[threadIdx.x >> 6];
  const StagedScene S = stage_stack(); // nothing of the scene is staged
  const uint32_t lane = __lane_id();
  const uint32_t p = blockIdx.x * TRACE_BLOCK + threadIdx.x;
  const bool live = p < U.pixelCount;
  AovPixel P; P.pixelIndex = 0u; P.curNormal = v3(0.0f, 0.0f, 0.0f); P.curAlbedo = P.curNormal; P.blend = false;
  if (live) aov_pixel_begin(U, A, tile_to_image_pixel(U, p), P);
  TraceCounters tc{0u, 0u};
  RayTrav2 R; trav2_init(R, v3(0.0f, 0.0f, 0.0f), v3(0.0f, 0.0f, 1.0f), 0.0f, 0.0f);
  for (uint32_t s = 0; s < U.spp; s++) { // (wave-uniform trip count)
    V3 dir = v3(0.0f, 0.0f, 1.0f); uint32_t rng = 0u;
    bool alive = false;
    if (live) {
      V3 origin; float tMin, tMax;
      make_camera_ray(U, P.pixelIndex, U.sampleOffset + s, origin, dir, tMin, tMax, rng);
      trav2_init(R, origin, dir, tMin, tMax);
      wave_ray_begin(W, R.tBest);
      wt_hit_put(W, lane, f2u(origin.x), f2u(origin.y), MISS, 0u); // the record if nothing is hit
      alive = true;
    }
    while (__ballot(alive)) {
      if (wave_step2<false, false, CUTOUT>(R, alive, W, sc, S.stack, tc, rng)) alive = false;
    }
    if (live) {
      const uint4 h = wt_hit_get(W, lane); // (u, v, scene-order id | class << 28), or the miss record
      if (h.z != MISS) { // a miss skips the sample, as in k_aov
        const float t = u2f(wt_best_t(W, lane));
        const uint32_t tri = sc.flatOfOrig[h.z & 0x0fffffffu];
        const uint32_t matWord = (reinterpret_cast<const uint4*>(sc.tris) + (size_t)tri * 4u)[2].w;
        aov_hit<true>(U, sc, A, P, dir, t, u2f(h.x), u2f(h.y), tri, matWord); // (beyond LDS: the scene carries TriShade records)
      }
    }
  }
  if (live) aov_pixel_end(A, P);
}

// ------------------------------------------------------------------------------------------------
// host-callable launcher (gi_aov.hip launchAov picks it: sc.twoLevel && sc.nodeCount == 0)
// ------------------------------------------------------------------------------------------------
void launchAov2(hipStream_t s, const FrameUniforms& U, const SceneView& sc, const AovTargets& A)
{
  const uint32_t blocks = (U.pixelCount + TRACE_BLOCK - 1u) / TRACE_BLOCK;
  dispatchBools([&](auto cutoutC) {
    hipLaunchKernelGGL((k_aov2<decltype(cutoutC)::value>), dim3(blocks), dim3(TRACE_BLOCK), traceLdsBytes(16u, 0u, 0u), s, U, sc, A);
  }, sc.hasCutouts != 0u);
}

} // namespace gi

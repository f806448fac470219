// gi_aov.hip -- k_aov, the non-colour AOVs of a frame (gfx950): replays the camera rays of every sample in order and writes what the reference's ray generation
// and closest-hit shaders write for the primary hit (/root/reference/src/gi/shaders/rp_main.rgen:132-183, 517-520; rp_main.chit:192-290).

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
// k_aov: the non-colour AOVs (rp_main.rgen:132-183, 517-520; rp_main.chit:192-290).  They depend only on the primary hit
// of each sample and are overwritten sample after sample, so they are produced by a separate per-pixel pass that
// replays the camera rays of samples 0..spp-1 in order (same RNG streams) -- exact, and off the colour path's hot loop.  The pixel's prologue, the per-hit
// body and the epilogue are gi_aov_body.h's, shared with k_aov2 (gi_aov2.hip: two-level scenes without the flat tree).
// ------------------------------------------------------------------------------------------------
template <uint32_t STACK, bool OVERFLOW, bool PACKED>
__global__ __launch_bounds__(TRACE_BLOCK) void k_aov(FrameUniforms U, SceneView sc, AovTargets A, uint32_t ldsNodes, uint32_t ldsTris)
{
  const StagedScene S = stage_scene<STACK>(sc, ldsNodes, ldsTris);
  const uint32_t p = blockIdx.x * TRACE_BLOCK + threadIdx.x;
  if (p >= U.pixelCount) return;
  AovPixel P;
  aov_pixel_begin(U, A, tile_to_image_pixel(U, p), P);
  TraceCounters tc{0u, 0u};
  for (uint32_t s = 0; s < U.spp; s++) {
    V3 origin, dir; float tMin, tMax; uint32_t rng;
    make_camera_ray(U, P.pixelIndex, U.sampleOffset + s, origin, dir, tMin, tMax, rng);
    float t, u, v; uint32_t tri;
    uint32_t matWord;
    if (!traverse<false, false, STACK, OVERFLOW, STAGED_SOME, true>(sc, S, origin, dir, tMin, tMax, t, u, v, tri, matWord, tc, rng)) continue;
    aov_hit<PACKED>(U, sc, A, P, dir, t, u, v, tri, matWord);
  }
  aov_pixel_end(A, P);
}

// ------------------------------------------------------------------------------------------------
// host-callable launchers
// ------------------------------------------------------------------------------------------------
void launchAov(hipStream_t s, const FrameUniforms& U, const SceneView& sc, const AovTargets& A)
{
  if (sc.twoLevel && sc.nodeCount == 0u) { launchAov2(s, U, sc, A); return; } // a two-level scene without the flat tree: the walk of the TLAS (gi_aov2.hip)
  uint32_t ln, lt, bytes; traceLdsLayout(sc, ln, lt, bytes);
  bytes = traceLdsBytes(sc.bvhDepth <= 8u ? 8u : 16u, ln, lt); // k_aov has no 4-entry variant
  const uint32_t blocks = (U.pixelCount + TRACE_BLOCK - 1u) / TRACE_BLOCK;
  dispatchBools([&](auto packedC) {
    constexpr bool PACKED = decltype(packedC)::value;
    if (sc.bvhDepth <= 8u) hipLaunchKernelGGL((k_aov<8, false, PACKED>), dim3(blocks), dim3(TRACE_BLOCK), bytes, s, U, sc, A, ln, lt);
    else if (sc.bvhDepth <= 16u) hipLaunchKernelGGL((k_aov<16, false, PACKED>), dim3(blocks), dim3(TRACE_BLOCK), bytes, s, U, sc, A, ln, lt);
    else hipLaunchKernelGGL((k_aov<16, true, PACKED>), dim3(blocks), dim3(TRACE_BLOCK), bytes, s, U, sc, A, ln, lt);
  }, sc.shadePacked != 0u);
}

} // namespace gi

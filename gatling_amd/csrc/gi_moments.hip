// gi_moments.hip -- k_moments: the sample-moments AOV (opt-in: a binding with GI_C_AOV_EXT_MOMENTS; gi_moments.h has the per-pixel form and the contract).
// Launched beside a batch's accumulation (gi_render.cpp accumulateBatch / serveFromWindow) on the same stream: it reads the per-sample buffer the batch left,
// before the next batch overwrites it.  One thread per pixel of the tile, every record has one writer: no atomics, no LDS.
// Built with -ffp-contract=off (arithmetic contract, see gi_device_math.h).

#include <hip/hip_runtime.h>

#include "gi_device_math.h"
#include "gi_kernels.h"
#include "gi_types.h"
#include "gi_queues.h"
#include "gi_traversal.h"
#include "gi_shading.h"
#include "gi_stages.h"
#include "gi_moments.h"

namespace gi {

__global__ __launch_bounds__(BLOCK) void k_moments(FrameUniforms U, const F4* __restrict__ sampleBuf, F4* __restrict__ M, MomentsFold F)
{
  const uint32_t p = blockIdx.x * BLOCK + threadIdx.x;
  if (p >= U.pixelCount) return;
  if (F.missRect) { const V3 c = retired_miss_sample(U); F.missSample[0] = c.x; F.missSample[1] = c.y; F.missSample[2] = c.z; } // k_accumulate's constant
  F4* dst = &M[tile_to_image_pixel(U, p)];
  F4 prev = F4{0.0f, 0.0f, 0.0f, 0.0f};
  if (F.continues) prev = ld4(dst);
  const F4 m = mo_pixel(F, p, sampleBuf, prev);
  st4(dst, m.x, m.y, m.z, 0.0f);
}

void launchMoments(hipStream_t s, const FrameUniforms& U, const F4* sampleBuf, F4* M, uint32_t bufferSamples, uint32_t first, uint32_t count, bool pixelMajor,
    bool continues)
{
  MomentsFold F{};
  F.pixelCount = U.pixelCount; F.imageWidth = U.imageWidth; F.rowBegin = U.rowBegin; F.rowStride = U.rowStride;
  F.bufferSamples = bufferSamples; F.first = first; F.count = count; F.pixelMajor = pixelMajor ? 1u : 0u; F.continues = continues ? 1u : 0u;
  F.missRect = (U.flags & FLAG_MISS_RECT) ? 1u : 0u; F.rectX0 = U.rectX0; F.rectX1 = U.rectX1; F.rectTy0 = U.rectTy0; F.rectTy1 = U.rectTy1;
  hipLaunchKernelGGL(k_moments, dim3((U.pixelCount + BLOCK - 1u) / BLOCK), dim3(BLOCK), 0, s, U, sampleBuf, M, F);
}

} // namespace gi

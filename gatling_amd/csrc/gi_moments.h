// gi_moments.h -- the per-pixel arithmetic of the sample-moments AOV (opt-in: a binding with GI_C_AOV_EXT_MOMENTS, include/gi_c.h; gi_moments.hip k_moments;
// DESIGN.md section 6 "Sample moments"), shared by the device kernel and the host form as gi_denoise.h, gi_vispatch.h and gi_blas.h are.  Per pixel the buffer
// holds M = (S1, S2, n, 0) over the samples of the running accumulation:
//   L  = (0.2126 r + 0.7152 g) + 0.0722 b of a sample record AS IT LIES in the per-sample buffer (after the clamp to maxSampleValue, before the 1 / spp of the
//        colour's fold), without a fused multiply-add (the units are built with -ffp-contract=off);
//   S1 = sum of L, S2 = sum of (L L), n = sum of 1.0f -- the samples added ONE BY ONE in sample order, from zero.
// Because a pixel's samples are folded one at a time in sample order, M is a function of the samples alone: not of how they were cut into calls, batches or
// look-ahead windows, nor of the buffer's layout.  The three sources are k_accumulate's (gi_kernels.hip): the miss-rectangle constant, the pixel-major run
// (128-byte lines, eight records per round) and the sample-major strided reads; a look-ahead window's slice [first, first + count) is k_fold_window's.
// A call CONTINUES the accumulation (starts from the record the buffer holds) when it is progressive with a sample offset > 0 and this buffer received the
// moments of the call before it OF THE SAME ACCUMULATION (giCRender stamps the buffer with the accumulation's epoch and the next sample offset; both must
// match -- the offset alone recurs after a reset); otherwise it starts from zero -- so a buffer first bound at a sample offset > 0 starts from zero at that
// call, and its n then counts fewer samples than the colour holds.
#pragma once

#include <cstddef>
#include <cstdint>

#if !defined(GI_MOMENTS_HOST_ONLY) // (a program that checks the per-pixel form with a plain C++ compiler defines it and sees everything but the launcher)
#include <hip/hip_runtime.h>
#endif

#include "gi_types.h"

#if defined(__HIP__)
#define GI_MOMENTS_HD __host__ __device__
#else
#define GI_MOMENTS_HD
#endif

namespace gi {

GI_MOMENTS_HD inline float mo_lum(float r, float g, float b) { return (0.2126f * r + 0.7152f * g) + 0.0722f * b; }
// one sample of luminance L into M
GI_MOMENTS_HD inline void mo_add(F4& m, float L) { m.x = m.x + L; m.y = m.y + L * L; m.z = m.z + 1.0f; }

// `count` samples that are all the constant (r, g, b): the pixels outside the miss rectangle.  The same loop as the records', the constant in their place
GI_MOMENTS_HD inline void mo_fold_constant(F4& m, float r, float g, float b, uint32_t count)
{
  const float L = mo_lum(r, g, b);
  for (uint32_t s = 0; s < count; s++) mo_add(m, L);
}
// `count` records that lie one behind the other (pixel-major): eight records, one 128-byte line, per round
GI_MOMENTS_HD inline void mo_fold_run(F4& m, const F4* src, uint32_t count)
{
  uint32_t s = 0;
  for (; s + 8u <= count; s += 8u) {
    F4 r[8];
#pragma unroll
    for (uint32_t k = 0; k < 8u; k++) r[k] = src[s + k];
#pragma unroll
    for (uint32_t k = 0; k < 8u; k++) mo_add(m, mo_lum(r[k].x, r[k].y, r[k].z));
  }
  for (; s < count; s++) { const F4 r = src[s]; mo_add(m, mo_lum(r.x, r.y, r.z)); }
}
// `count` records `stride` records apart (sample-major)
GI_MOMENTS_HD inline void mo_fold_strided(F4& m, const F4* src, size_t stride, uint32_t count)
{
  for (uint32_t s = 0; s < count; s++) { const F4 r = src[(size_t)s * stride]; mo_add(m, mo_lum(r.x, r.y, r.z)); }
}

// What one fold is given beside the per-sample buffer and the moments image (by value: uniform over the launch).  The tile is `pixelCount` pixels, row-major
// over rows rowBegin, rowBegin + rowStride, ... of an image `imageWidth` wide; the buffer holds `bufferSamples` records per pixel, [pixel][bufferSamples]
// (pixelMajor) or [bufferSamples][pixel], of which the fold takes [first, first + count).
struct MomentsFold {
  uint32_t pixelCount, imageWidth, rowBegin, rowStride;
  uint32_t bufferSamples, first, count, pixelMajor;
  uint32_t continues;                           // 1: start from the record M holds, 0: from zero
  uint32_t missRect, rectX0, rectX1, rectTy0, rectTy1; // missRect 1: pixels outside [rectX0, rectX1) x tile rows [rectTy0, rectTy1) have no records ...
  float missSample[3];                          // ... every sample of theirs is this constant
};

// One pixel of the tile: its new record (w = 0).  `prev`: the record M holds for it, read only with F.continues
GI_MOMENTS_HD inline F4 mo_pixel(const MomentsFold& F, uint32_t p, const F4* sampleBuf, const F4& prev)
{
  F4 m; m.x = m.y = m.z = m.w = 0.0f;
  if (F.continues) { m.x = prev.x; m.y = prev.y; m.z = prev.z; }
  const uint32_t row = p / F.imageWidth, col = p - row * F.imageWidth;
  if (F.missRect && (col < F.rectX0 || col >= F.rectX1 || row < F.rectTy0 || row >= F.rectTy1)) mo_fold_constant(m, F.missSample[0], F.missSample[1], F.missSample[2], F.count);
  else if (F.pixelMajor) mo_fold_run(m, sampleBuf + ((size_t)p * F.bufferSamples + F.first), F.count);
  else mo_fold_strided(m, sampleBuf + ((size_t)F.first * F.pixelCount + p), (size_t)F.pixelCount, F.count);
  return m;
}
GI_MOMENTS_HD inline size_t mo_image_pixel(const MomentsFold& F, uint32_t p) // (gi_queues.h tile_to_image_pixel)
{
  const uint32_t row = p / F.imageWidth, x = p - row * F.imageWidth;
  return (size_t)(F.rowBegin + row * F.rowStride) * F.imageWidth + x;
}

// ---- the host form of the kernel (giCDebugSampleMomentsHost) ------------------------------------------------------------------------------------------------
inline void momentsHost(const MomentsFold& F, const F4* sampleBuf, F4* M)
{
  for (uint32_t p = 0; p < F.pixelCount; p++) {
    const size_t at = mo_image_pixel(F, p);
    F4 prev; prev.x = prev.y = prev.z = prev.w = 0.0f;
    if (F.continues) prev = M[at];
    M[at] = mo_pixel(F, p, sampleBuf, prev);
  }
}

// ---- gi_moments.hip ------------------------------------------------------------------------------------------------------------------------------------------
#if !defined(GI_MOMENTS_HOST_ONLY)
// k_moments over the tile `U` describes, one thread per pixel: folds the samples [first, first + count) of every pixel's `bufferSamples` records into M (the
// bound buffer's device copy, indexed by image pixel).  The miss rectangle is U's (FLAG_MISS_RECT, retired_miss_sample(U)), the layout the caller's.
void launchMoments(hipStream_t s, const FrameUniforms& U, const F4* sampleBuf, F4* M, uint32_t bufferSamples, uint32_t first, uint32_t count, bool pixelMajor,
    bool continues);
#endif

} // namespace gi

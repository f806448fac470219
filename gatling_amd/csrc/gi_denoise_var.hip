// gi_denoise_var.hip -- the variance-guided a-trous denoiser (opt-in: giCDenoiseVariance; gi_denoise_host.cpp runs the launches, DESIGN.md section 6 "Denoiser").
// gi_denoise.h has the filter and every per-pixel form, which the host form runs as well; gi_denoise.hip has the fixed-sigma filter's kernels and is not touched:
// these are new kernels in a unit of their own.
//
//   k_denoise_prepare_var     one thread per pixel: reads the X record prepare left (its guided flag), the moments and (optional) albedo records, stores the
//                             8-byte V record (v, known).  Streaming: 48 bytes read, 8 stored per pixel.
//   k_denoise_var_pass<TILE>  k_denoise_pass with the third plane: workgroups of 32 x 8 pixels, one launch per iteration over ping-pong X and V planes.
//                               TILE = 0   every tap is direct global loads: 16 bytes of X, 16 of G where the tap is guided, 8 of V where the pixel's variance
//                                          is known; the 3 x 3 average of v at unit spacing is nine more 8-byte loads (neighbouring lanes' neighbours: L1 hits).
//                               TILE = S   (S = 1, 2, 4) the (32 + 4 S) x (8 + 4 S) records of all three planes in LDS -- 40 bytes a texel: 16.9, 25 and 45 KiB
//                                          against the two-plane tile's 13.5, 20 and 36; at step 2 six workgroups fit a CU's 160 KiB where eight of the two-plane
//                                          kernel's did (24 of 32 waves); the halo of 2 S covers the unit-spacing 3 x 3.
//                             The last pass fuses the finish and stores no V.
//   k_denoise_vt              (GATLING_OPTIONS=denoise_form=3 alone) the 3 x 3 average of a direct-load pass as a launch of its own: one thread per pixel, nine
//                             8-byte loads, one 4-byte store; the pass after it (k_denoise_var_pass<0, true>) reads that word.  Same bytes; DESIGN section 9
//                             row 29 has what either costs.
//
// No atomics, no counters, no fences; every record has one writer, a pass never reads a plane it writes.  Every index is checked against the image.  The
// arithmetic is gi_denoise.h's, compiled without contraction.  Plain HIP C++.
#include <cstddef>

#include "gi_denoise.h"

namespace gi {
namespace {

constexpr uint32_t kDvBlock = 256, kDvTileW = 32, kDvTileH = 8;

__device__ inline float4 dv_pack(const F4& v) { return make_float4(v.x, v.y, v.z, v.w); }
__device__ inline F4 dv_unpack(const float4& v) { F4 r; r.x = v.x; r.y = v.y; r.z = v.z; r.w = v.w; return r; }
__device__ inline DnV dv_load(const DnV* p) { const float2 v = *reinterpret_cast<const float2*>(p); DnV r; r.v = v.x; r.known = v.y; return r; }
__device__ inline void dv_store(DnV* p, const DnV& v) { *reinterpret_cast<float2*>(p) = make_float2(v.v, v.known); }

__global__ __launch_bounds__(kDvBlock) void k_denoise_prepare_var(const F4* __restrict__ X, const F4* __restrict__ moments, const F4* __restrict__ albedo,
    size_t pixels, float albedoFloor, uint32_t minSamples, DnV* __restrict__ V)
{
  const size_t p = (size_t)blockIdx.x * kDvBlock + threadIdx.x;
  if (p >= pixels) return;
  F4 B{};
  if (albedo) B = albedo[p];
  dv_store(&V[p], dn_prepare_variance(moments[p], minSamples, X[p].w != 0.0f, albedo != nullptr, B, albedoFloor));
}

// vt of every pixel whose variance is known (0 elsewhere: never read), for the passes that take it from a plane.  Same 32 x 8 mapping as the passes
__global__ __launch_bounds__(kDvBlock) void k_denoise_vt(uint32_t width, uint32_t height, const DnV* __restrict__ V, float* __restrict__ vt)
{
  const uint32_t px = blockIdx.x * kDvTileW + threadIdx.x % kDvTileW, py = blockIdx.y * kDvTileH + threadIdx.x / kDvTileW;
  if (px >= width || py >= height) return;
  const size_t p = (size_t)py * width + px;
  float r = 0.0f;
  if (dv_load(&V[p]).known != 0.0f) r = dn_variance_average(width, height, px, py, [&](uint32_t qx, uint32_t qy) { return dv_load(&V[(size_t)qy * width + qx]); });
  vt[p] = r;
}

// VT_PLANE (TILE = 0 only): vt comes from the plane k_denoise_vt wrote, not from nine loads here
template <uint32_t TILE, bool VT_PLANE = false>
__global__ __launch_bounds__(kDvBlock) void k_denoise_var_pass(DenoiseVarPass Q, const F4* __restrict__ X, const F4* __restrict__ G, const DnV* __restrict__ V,
    F4* __restrict__ dst, DnV* __restrict__ Vnext, const F4* __restrict__ color, const F4* __restrict__ albedo, const float* __restrict__ vt)
{
  DenoisePass& P = Q.base;
  const uint32_t tx = threadIdx.x % kDvTileW, ty = threadIdx.x / kDvTileW;
  const uint32_t px = blockIdx.x * kDvTileW + tx, py = blockIdx.y * kDvTileH + ty;
  const bool inside = px < P.width && py < P.height;
  const size_t p = (size_t)py * P.width + px;
  F4 r{}; DnV vNew{}; bool guided = false;
  if constexpr (TILE == 0u) {
    if (!inside) return;
    const F4 xp = X[p];
    const DnV vp = dv_load(&V[p]);
    guided = xp.w != 0.0f; r = xp; vNew = vp;
    if (guided) {
      const auto fetchV = [&](uint32_t qx, uint32_t qy) { return dv_load(&V[(size_t)qy * P.width + qx]); };
      r = dn_filter_pixel_var(Q, px, py, xp, G[p], vp, [&](uint32_t qx, uint32_t qy) { return X[(size_t)qy * P.width + qx]; },
          [&](uint32_t qx, uint32_t qy) { return G[(size_t)qy * P.width + qx]; }, fetchV,
          [&] { if constexpr (VT_PLANE) return vt[p]; else return dn_variance_average(P.width, P.height, px, py, fetchV); }, vNew);
      r.w = xp.w;
    }
  } else {
    P.step = TILE; // (a constant: the tap offsets are folded)
    constexpr uint32_t HALO = 2u * TILE, TW = kDvTileW + 2u * HALO, TH = kDvTileH + 2u * HALO;
    __shared__ float4 sx[TW * TH], sg[TW * TH];
    __shared__ float2 sv[TW * TH];
    const int32_t ox = (int32_t)(blockIdx.x * kDvTileW) - (int32_t)HALO, oy = (int32_t)(blockIdx.y * kDvTileH) - (int32_t)HALO;
    for (uint32_t t = threadIdx.x; t < TW * TH; t += kDvBlock) {
      const int32_t gx = ox + (int32_t)(t % TW), gy = oy + (int32_t)(t / TW);
      F4 xr{}, gr{}; DnV vr{}; // outside the image: unguided, variance not known
      if (gx >= 0 && gy >= 0 && gx < (int32_t)P.width && gy < (int32_t)P.height) {
        const size_t q = (size_t)gy * P.width + (size_t)gx;
        xr = X[q];
        if (xr.w != 0.0f) { gr = G[q]; vr = dv_load(&V[q]); }
      }
      sx[t] = dv_pack(xr); sg[t] = dv_pack(gr); sv[t] = make_float2(vr.v, vr.known);
    }
    __syncthreads();
    if (!inside) return;
    const uint32_t c = (ty + HALO) * TW + (tx + HALO);
    const F4 xp = dv_unpack(sx[c]);
    guided = xp.w != 0.0f; r = xp;
    const DnV vp = guided ? DnV{sv[c].x, sv[c].y} : dv_load(&V[p]); // (an unguided pixel's record was not staged: it is carried through from the plane)
    vNew = vp;
    if (guided) {
      // (a tap inside the image lies inside the tile: |q - p| <= 2 step = HALO >= 1 in both axes)
      const auto at = [&](uint32_t qx, uint32_t qy) { return (uint32_t)((int32_t)qy - oy) * TW + (uint32_t)((int32_t)qx - ox); };
      const auto fetchV = [&](uint32_t qx, uint32_t qy) { const float2 v = sv[at(qx, qy)]; return DnV{v.x, v.y}; };
      r = dn_filter_pixel_var(Q, px, py, xp, dv_unpack(sg[c]), vp, [&](uint32_t qx, uint32_t qy) { return dv_unpack(sx[at(qx, qy)]); },
          [&](uint32_t qx, uint32_t qy) { return dv_unpack(sg[at(qx, qy)]); }, fetchV, [&] { return dn_variance_average(P.width, P.height, px, py, fetchV); }, vNew);
      r.w = xp.w;
    }
  }
  F4 C{}, B{};
  if (P.last) { C = color[p]; if (albedo && guided) B = albedo[p]; }
  dst[p] = dn_store_pixel(P, r, guided, C, albedo != nullptr, B);
  if (!P.last) dv_store(&Vnext[p], vNew);
}

} // namespace

bool launchDenoisePrepareVariance(hipStream_t s, const F4* X, const F4* moments, const F4* albedo, uint32_t width, uint32_t height, float albedoFloor,
    uint32_t minSamples, DnV* V)
{
  if (!X || !moments || !V || width == 0u || height == 0u || width > 65535u || height > 65535u || minSamples < 2u) return false;
  const size_t pixels = (size_t)width * height;
  hipLaunchKernelGGL(k_denoise_prepare_var, dim3((uint32_t)((pixels + kDvBlock - 1u) / kDvBlock)), dim3(kDvBlock), 0, s, X, moments, albedo, pixels, albedoFloor,
      minSamples, V);
  return true;
}

bool launchDenoiseVarPass(hipStream_t s, const DenoiseVarPass& Q, const F4* X, const F4* G, const DnV* V, F4* dst, DnV* Vnext, const F4* color, const F4* albedo,
    uint32_t form, float* vt)
{
  const DenoisePass& P = Q.base;
  if (!X || !G || !V || !dst || dst == X || dst == G || X == G || V == Vnext || P.width == 0u || P.height == 0u || P.width > 65535u || P.height > 65535u) return false;
  if (P.step == 0u || P.step > (1u << (kDenoiseMaxIterations - 1u)) || (P.step & (P.step - 1u)) || P.normalSquarings > kDenoiseMaxSquarings) return false;
  if (P.last ? (!color || dst == color || dst == albedo) : !Vnext) return false;
  const dim3 grid((P.width + kDvTileW - 1u) / kDvTileW, (P.height + kDvTileH - 1u) / kDvTileH), block(kDvBlock);
  const uint32_t tile = form == 1u ? 0u : (P.step <= 2u || (form == 2u && P.step == 4u)) ? P.step : 0u;
  if (tile == 0u && form == 3u) {
    if (!vt) return false;
    hipLaunchKernelGGL(k_denoise_vt, grid, block, 0, s, P.width, P.height, V, vt);
    hipLaunchKernelGGL((k_denoise_var_pass<0u, true>), grid, block, 0, s, Q, X, G, V, dst, Vnext, color, albedo, (const float*)vt);
    return true;
  }
  const float* none = nullptr;
  switch (tile) {
    case 1u: hipLaunchKernelGGL(k_denoise_var_pass<1u>, grid, block, 0, s, Q, X, G, V, dst, Vnext, color, albedo, none); break;
    case 2u: hipLaunchKernelGGL(k_denoise_var_pass<2u>, grid, block, 0, s, Q, X, G, V, dst, Vnext, color, albedo, none); break;
    case 4u: hipLaunchKernelGGL(k_denoise_var_pass<4u>, grid, block, 0, s, Q, X, G, V, dst, Vnext, color, albedo, none); break;
    default: hipLaunchKernelGGL(k_denoise_var_pass<0u>, grid, block, 0, s, Q, X, G, V, dst, Vnext, color, albedo, none); break;
  }
  return true;
}

} // namespace gi

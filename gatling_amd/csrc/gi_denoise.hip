// gi_denoise.hip -- the a-trous denoiser of the colour AOV, guided by the normal, depth and albedo AOVs (opt-in: giCDenoise; gi_denoise_host.cpp runs the launches,
// DESIGN.md section 6 "Denoiser").  gi_denoise.h has the filter and every per-pixel form, which the host form runs as well: the kernels only map pixels to
// lanes and decide where a tap's record comes from.
//
//   k_denoise_prepare     one thread per pixel, 256 consecutive pixels per workgroup: reads the colour, normal and (optional) albedo records and the depth
//                         word, stores the two 16-byte planes X = (colour / max(albedo, floor), guided) and G = (2 normal - 1, depth).  Streaming: 52 bytes
//                         read, 32 stored per pixel.
//   k_denoise_pass<TILE>  one thread per pixel, workgroups of 32 x 8 pixels (a wave covers two rows of 32: a tap row is 512 contiguous bytes); one launch per
//                         iteration over ping-pong X planes, step = 2^i.  25 taps x 32 bytes per pixel is all reuse:
//                           TILE = 0   every tap is two direct 16-byte global loads (the G record only where the tap's X record says guided), served by the
//                                      vector L1 / the L2: at large steps a dense tile would load as many texels as the taps need.
//                           TILE = S   (S = 1, 2, 4: the step) the workgroup first stages the (32 + 4 S) x (8 + 4 S) records of both planes its taps reach in
//                                      LDS -- 13.5, 20 and 36 KiB --, texels outside the image as unguided; a tap is then two ds_read_b128 of consecutive lanes'
//                                      consecutive 16-byte records (conflict-free in the instruction's 16-lane groups).
//                         The LAST pass fuses the finish: it reads the colour (alpha; an unguided pixel's whole record) and the albedo again and stores the
//                         output image instead of an X plane.  Every pixel of the destination is stored: unguided records are carried through.
//
// No atomics, no counters, no fences; every record has one writer, and a pass never reads the plane it writes (Jacobi).  Every index is checked against the
// image.  The arithmetic is gi_denoise.h's, compiled without contraction.  Plain HIP C++.
#include <cstddef>

#include "gi_denoise.h"

namespace gi {
namespace {

constexpr uint32_t kDnBlock = 256, kDnTileW = 32, kDnTileH = 8;

// LDS holds the records as the vector type (one ds_read_b128 / ds_write_b128 each, nothing through private memory)
__device__ inline float4 dn_pack(const F4& v) { return make_float4(v.x, v.y, v.z, v.w); }
__device__ inline F4 dn_unpack(const float4& v) { F4 r; r.x = v.x; r.y = v.y; r.z = v.z; r.w = v.w; return r; }

__global__ __launch_bounds__(kDnBlock) void k_denoise_prepare(const F4* __restrict__ color, const F4* __restrict__ normal, const float* __restrict__ depth,
    const F4* __restrict__ albedo, size_t pixels, float albedoFloor, float backgroundDepth, F4* __restrict__ X, F4* __restrict__ G)
{
  const size_t p = (size_t)blockIdx.x * kDnBlock + threadIdx.x;
  if (p >= pixels) return;
  F4 B{};
  if (albedo) B = albedo[p];
  F4 x, g;
  dn_prepare_pixel(color[p], normal[p], depth[p], albedo != nullptr, B, albedoFloor, backgroundDepth, x, g);
  X[p] = x; G[p] = g;
}

template <uint32_t TILE>
__global__ __launch_bounds__(kDnBlock) void k_denoise_pass(DenoisePass P, const F4* __restrict__ X, const F4* __restrict__ G, F4* __restrict__ dst,
    const F4* __restrict__ color, const F4* __restrict__ albedo)
{
  const uint32_t tx = threadIdx.x % kDnTileW, ty = threadIdx.x / kDnTileW;
  const uint32_t px = blockIdx.x * kDnTileW + tx, py = blockIdx.y * kDnTileH + ty;
  const bool inside = px < P.width && py < P.height;
  const size_t p = (size_t)py * P.width + px;
  F4 r{}; bool guided = false;
  if constexpr (TILE == 0u) {
    if (!inside) return;
    const F4 xp = X[p];
    guided = xp.w != 0.0f; r = xp;
    if (guided) {
      r = dn_filter_pixel(P, px, py, xp, G[p], [&](uint32_t qx, uint32_t qy) { return X[(size_t)qy * P.width + qx]; },
          [&](uint32_t qx, uint32_t qy) { return G[(size_t)qy * P.width + qx]; });
      r.w = xp.w;
    }
  } else {
    P.step = TILE; // (a constant: the tap offsets are folded)
    constexpr uint32_t HALO = 2u * TILE, TW = kDnTileW + 2u * HALO, TH = kDnTileH + 2u * HALO;
    __shared__ float4 sx[TW * TH], sg[TW * TH];
    // the tile's origin in the image may be negative: texel (i, j) of the tile is pixel (ox + i, oy + j)
    const int32_t ox = (int32_t)(blockIdx.x * kDnTileW) - (int32_t)HALO, oy = (int32_t)(blockIdx.y * kDnTileH) - (int32_t)HALO;
    for (uint32_t t = threadIdx.x; t < TW * TH; t += kDnBlock) {
      const int32_t gx = ox + (int32_t)(t % TW), gy = oy + (int32_t)(t / TW);
      F4 xr{}, gr{}; // outside the image: unguided
      if (gx >= 0 && gy >= 0 && gx < (int32_t)P.width && gy < (int32_t)P.height) {
        const size_t q = (size_t)gy * P.width + (size_t)gx;
        xr = X[q];
        if (xr.w != 0.0f) gr = G[q];
      }
      sx[t] = dn_pack(xr); sg[t] = dn_pack(gr);
    }
    __syncthreads();
    if (!inside) return;
    const uint32_t c = (ty + HALO) * TW + (tx + HALO);
    const F4 xp = dn_unpack(sx[c]);
    guided = xp.w != 0.0f; r = xp;
    if (guided) {
      // (a tap inside the image lies inside the tile: |q - p| <= 2 step = HALO in both axes)
      r = dn_filter_pixel(P, px, py, xp, dn_unpack(sg[c]), [&](uint32_t qx, uint32_t qy) { return dn_unpack(sx[(uint32_t)((int32_t)qy - oy) * TW + (uint32_t)((int32_t)qx - ox)]); },
          [&](uint32_t qx, uint32_t qy) { return dn_unpack(sg[(uint32_t)((int32_t)qy - oy) * TW + (uint32_t)((int32_t)qx - ox)]); });
      r.w = xp.w;
    }
  }
  F4 C{}, B{};
  if (P.last) { C = color[p]; if (albedo && guided) B = albedo[p]; }
  dst[p] = dn_store_pixel(P, r, guided, C, albedo != nullptr, B);
}

} // namespace

bool launchDenoisePrepare(hipStream_t s, const F4* color, const F4* normal, const float* depth, const F4* albedo, uint32_t width, uint32_t height,
    float albedoFloor, float backgroundDepth, F4* X, F4* G)
{
  if (!color || !normal || !depth || !X || !G || X == G || width == 0u || height == 0u || width > 65535u || height > 65535u) return false;
  const size_t pixels = (size_t)width * height;
  hipLaunchKernelGGL(k_denoise_prepare, dim3((uint32_t)((pixels + kDnBlock - 1u) / kDnBlock)), dim3(kDnBlock), 0, s, color, normal, depth, albedo, pixels,
      albedoFloor, backgroundDepth, X, G);
  return true;
}

bool launchDenoisePass(hipStream_t s, const DenoisePass& P, const F4* X, const F4* G, F4* dst, const F4* color, const F4* albedo, uint32_t form)
{
  if (!X || !G || !dst || dst == X || dst == G || X == G || P.width == 0u || P.height == 0u || P.width > 65535u || P.height > 65535u) return false;
  if (P.step == 0u || P.step > (1u << (kDenoiseMaxIterations - 1u)) || (P.step & (P.step - 1u)) || P.normalSquarings > kDenoiseMaxSquarings) return false;
  if (P.last && (!color || dst == color || dst == albedo)) return false;
  const dim3 grid((P.width + kDnTileW - 1u) / kDnTileW, (P.height + kDnTileH - 1u) / kDnTileH), block(kDnBlock);
  const uint32_t tile = form == 1u ? 0u : (P.step <= 2u || (form == 2u && P.step == 4u)) ? P.step : 0u;
  switch (tile) {
    case 1u: hipLaunchKernelGGL(k_denoise_pass<1u>, grid, block, 0, s, P, X, G, dst, color, albedo); break;
    case 2u: hipLaunchKernelGGL(k_denoise_pass<2u>, grid, block, 0, s, P, X, G, dst, color, albedo); break;
    case 4u: hipLaunchKernelGGL(k_denoise_pass<4u>, grid, block, 0, s, P, X, G, dst, color, albedo); break;
    default: hipLaunchKernelGGL(k_denoise_pass<0u>, grid, block, 0, s, P, X, G, dst, color, albedo); break;
  }
  return true;
}

} // namespace gi

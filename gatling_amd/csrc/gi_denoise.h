// gi_denoise.h -- the per-pixel arithmetic of the a-trous denoiser of the colour AOV (opt-in: giCDenoise, include/gi_c.h; gi_denoise.hip k_denoise_prepare and
// k_denoise_pass; DESIGN.md section 6 "Denoiser"), shared by the device kernels and the host form as gi_vispatch.h and gi_blas.h are.  The filter is this
// project's own: nothing in the reference pins it.  It is written with + - x / and a spelled-out maximum on fp32 alone, in ONE association, without exp, pow
// or a fused multiply-add (the units are built with -ffp-contract=off), so the device, the host form and a NumPy float32 restatement
// (tests/denoise_ref.py) agree bit for bit.  Edge-stopping weights are rational, 1 / (1 + d^2), for that reason.
//
//   prepare   n = 2 A.xyz - 1 (the normal AOV stores (n + 1) / 2); d = max(B.xyz, albedoFloor) per channel, 1 without an albedo buffer (then nothing is
//             divided); x = C.xyz / d.  A pixel is GUIDED when z is finite and not the background depth (exact compare) and all of x and n are finite.  Two
//             16-byte planes: X = (x, guided ? 1 : 0), G = (n, z).
//   pass i    step = 2^i; Jacobi: reads plane i everywhere, writes plane i + 1.  A guided pixel visits the 5 x 5 taps q = p + step (dx, dy), dy outer and
//             dx inner, skipping taps outside the image and unguided ones:
//               wn = max(dot(n_p, n_q), 0), squared K times;  dz = (z_p - z_q) invSz, wz = 1 / (1 + dz dz);
//               dc = x_p - x_q, wc = 1 / (1 + dot(dc, dc) invSc);  w = (h[dy] h[dx]) ((wn wz) wc), h = {1/16, 1/4, 3/8, 1/4, 1/16};
//               acc += w x_q, wsum += w;  x' = acc / wsum where wsum > 0, else x.
//             dot is (ax bx + ay by) + az bz.  An unguided pixel's record is carried through and contributes to no other pixel.
//   finish    (fused into the last pass) out.xyz = x d with prepare's d, out.w = C.w; an unguided pixel's output is its colour record, bytewise.
//
// The VARIANCE-GUIDED filter (giCDenoiseVariance; gi_denoise_var.hip) is the same filter with the colour weight's fixed sigma replaced, per pixel, by the
// variance of the pixel's mean, taken from the sample-moments AOV M = (S1, S2, n, 0) (gi_moments.h).  lum(a) = (0.2126 a.x + 0.7152 a.y) + 0.0722 a.z.
//   prepare   x, n, z, d, guided as above.  With cnt = M.z: if cnt >= minSamples and S1, S2 are finite: m = S1 / cnt; var = max(S2 / cnt - m m, 0);
//             vm = var / (cnt - 1); dl = lum(d) (1 without albedo); v = vm / (dl dl); known = 1 if the pixel is guided and v <= 1e30.  Otherwise v = 0,
//             known = 0.  A third plane V = (v, known), 8 bytes a pixel.  (An unguided pixel never takes part, so its known is stored as 0.  The bound keeps
//             every v of every pass finite -- a pass at most doubles the largest -- because an infinite v would meet a zero weight further on and make a
//             NaN, whose sign differs between processors; no radiance anyone renders has such a variance, and the pixel uses the fixed weight.)
//   pass i    a guided p with known_p: vt = (sum of g[dy] g[dx] v_q) / (sum of g[dy] g[dx]) over the in-image q = p + (dx, dy), dy outer and dx inner in
//             -1 .. 1 at UNIT spacing whatever the step, with known_q, in the CURRENT V plane, g = {1/4, 1/2, 1/4} (p itself always counts);
//             den = sv2 (vt + varianceFloor), sv2 = sigmaVariance sigmaVariance made on the host;
//             per tap dl = lum(x_p) - lum(x_q), wc = 1 / (1 + (dl dl) / den).  A guided p with known_p = 0 uses wc of the fixed filter, invSc of pass i; so
//             does, for that pass, a p whose den or lum(x_p) is not finite (Inf / Inf and Inf - Inf would be NaN).
//             wn, wz, the tap order and w = (h h)((wn wz) wc) are the fixed filter's, and so are acc, wsum and x'.
//             Variance travels with the colour: over the taps with known_q, vs += (w w) v_q, vw += w; v'_p = vs / (vw vw) where vw vw > 0 (the product, not
//             vw alone: a sum of weights so small that its square underflows would divide 0 by 0), else v_p.  known never changes; a pixel with
//             known_p = 0 (unguided ones among them) keeps its V record.  The last pass stores no V.
//   finish    as above.
#pragma once

#include <cmath>
#include <cstddef>
#include <cstdint>

#if !defined(GI_DENOISE_HOST_ONLY) // (a program that checks the per-pixel forms with a plain C++ compiler defines it and sees everything but the launchers)
#include <hip/hip_runtime.h>
#endif

#include "gi_types.h"

#if defined(__HIP__)
#define GI_DENOISE_HD __host__ __device__
#else
#define GI_DENOISE_HD
#endif

namespace gi {

constexpr uint32_t kDenoiseMaxIterations = 6, kDenoiseMaxSquarings = 6;
constexpr float kDenoiseMaxVariance = 1.0e30f; // a larger v counts as not known (the variance-guided filter's prepare)

// What a pass is given beside its planes (by value: uniform over the launch)
struct DenoisePass {
  uint32_t width, height, step, normalSquarings;
  float invSz, invSc;       // 1 / sigmaDepth; (1 / sigmaColor^2) 4^i, both made on the host in fp32
  float albedoFloor;
  uint32_t last;            // 1: the pass writes the output buffer (finish) instead of an x plane
};

GI_DENOISE_HD inline float dn_max(float a, float b) { return a < b ? b : a; }
GI_DENOISE_HD inline bool dn_finite(float v) { return fabsf(v) <= 3.402823466e38f; } // false for NaN
GI_DENOISE_HD inline float dn_dot(float ax, float ay, float az, float bx, float by, float bz) { return (ax * bx + ay * by) + az * bz; }

// invSc of pass i
inline float denoiseInvSc(float sigmaColor, uint32_t i) { return (1.0f / (sigmaColor * sigmaColor)) * (float)(1u << (2u * i)); }

// the 5-tap B3-spline kernel {1/16, 1/4, 3/8, 1/4, 1/16} by tap offset -2 .. 2 (spelled as selects: an indexed local array would live in scratch memory)
GI_DENOISE_HD inline float dn_h(int d) { return d == 0 ? 0.375f : ((d == 1 || d == -1) ? 0.25f : 0.0625f); }

// d of a pixel (B: its albedo record, read only with an albedo buffer)
GI_DENOISE_HD inline F4 dn_divisor(bool hasAlbedo, const F4& B, float albedoFloor)
{
  F4 d; d.x = d.y = d.z = d.w = 1.0f;
  if (hasAlbedo) { d.x = dn_max(B.x, albedoFloor); d.y = dn_max(B.y, albedoFloor); d.z = dn_max(B.z, albedoFloor); }
  return d;
}

GI_DENOISE_HD inline void dn_prepare_pixel(const F4& C, const F4& A, float z, bool hasAlbedo, const F4& B, float albedoFloor, float backgroundDepth, F4& X, F4& G)
{
  const float nx = 2.0f * A.x - 1.0f, ny = 2.0f * A.y - 1.0f, nz = 2.0f * A.z - 1.0f;
  float x0 = C.x, x1 = C.y, x2 = C.z;
  if (hasAlbedo) { const F4 d = dn_divisor(true, B, albedoFloor); x0 = C.x / d.x; x1 = C.y / d.y; x2 = C.z / d.z; }
  const bool guided = dn_finite(z) && z != backgroundDepth && dn_finite(x0) && dn_finite(x1) && dn_finite(x2) && dn_finite(nx) && dn_finite(ny) && dn_finite(nz);
  X.x = x0; X.y = x1; X.z = x2; X.w = guided ? 1.0f : 0.0f;
  G.x = nx; G.y = ny; G.z = nz; G.w = z;
}

// One guided pixel of one pass.  fetchX(qx, qy) -> the X record of an in-image pixel; fetchG(qx, qy) -> its G record (asked only for guided taps).
// Returns x' (w is not set)
template <typename FetchX, typename FetchG>
GI_DENOISE_HD inline F4 dn_filter_pixel(const DenoisePass& P, uint32_t px, uint32_t py, const F4& xp, const F4& gp, FetchX&& fetchX, FetchG&& fetchG)
{
  float a0 = 0.0f, a1 = 0.0f, a2 = 0.0f, wsum = 0.0f;
  for (int dy = -2; dy <= 2; dy++) {
    const int32_t qy = (int32_t)py + dy * (int32_t)P.step; // (sides are at most 65535 and steps at most 32: giCDenoise)
    if (qy < 0 || qy >= (int32_t)P.height) continue;
    for (int dx = -2; dx <= 2; dx++) {
      const int32_t qx = (int32_t)px + dx * (int32_t)P.step;
      if (qx < 0 || qx >= (int32_t)P.width) continue;
      const F4 xq = fetchX((uint32_t)qx, (uint32_t)qy);
      if (xq.w == 0.0f) continue;
      const F4 gq = fetchG((uint32_t)qx, (uint32_t)qy);
      float wn = dn_max(dn_dot(gp.x, gp.y, gp.z, gq.x, gq.y, gq.z), 0.0f);
      for (uint32_t k = 0; k < P.normalSquarings; k++) wn = wn * wn;
      const float dz = (gp.w - gq.w) * P.invSz;
      const float wz = 1.0f / (1.0f + dz * dz);
      const float c0 = xp.x - xq.x, c1 = xp.y - xq.y, c2 = xp.z - xq.z;
      const float wc = 1.0f / (1.0f + dn_dot(c0, c1, c2, c0, c1, c2) * P.invSc);
      const float w = (dn_h(dy) * dn_h(dx)) * ((wn * wz) * wc);
      a0 = a0 + w * xq.x; a1 = a1 + w * xq.y; a2 = a2 + w * xq.z;
      wsum = wsum + w;
    }
  }
  F4 r = xp;
  if (wsum > 0.0f) { r.x = a0 / wsum; r.y = a1 / wsum; r.z = a2 / wsum; }
  return r;
}

// What a pass stores for pixel p given its new x (guided) or its carried record (unguided): the next plane's record, or with P.last the output
// (C, B: the pixel's colour and albedo records, read only with P.last)
GI_DENOISE_HD inline F4 dn_store_pixel(const DenoisePass& P, const F4& xNew, bool guided, const F4& C, bool hasAlbedo, const F4& B)
{
  if (!P.last) return xNew;
  if (!guided) return C;
  const F4 d = dn_divisor(hasAlbedo, B, P.albedoFloor);
  F4 o; o.x = xNew.x * d.x; o.y = xNew.y * d.y; o.z = xNew.z * d.z; o.w = C.w;
  return o;
}

// ---- the variance-guided filter (giCDenoiseVariance) -------------------------------------------------------------------------------------------------------------
struct DnV { float v, known; }; // the third plane's record
struct DenoiseVarPass {
  DenoisePass base;
  float sv2, varianceFloor; // sigmaVariance^2, made on the host in fp32
};

GI_DENOISE_HD inline float dn_lum(float r, float g, float b) { return (0.2126f * r + 0.7152f * g) + 0.0722f * b; }
// the 3-tap kernel {1/4, 1/2, 1/4} by tap offset -1 .. 1
GI_DENOISE_HD inline float dn_g(int d) { return d == 0 ? 0.5f : 0.25f; }

// V of a pixel (M: its moments record; B: its albedo record, read only with an albedo buffer)
GI_DENOISE_HD inline DnV dn_prepare_variance(const F4& M, uint32_t minSamples, bool guided, bool hasAlbedo, const F4& B, float albedoFloor)
{
  DnV r; r.v = 0.0f; r.known = 0.0f;
  const float cnt = M.z;
  if (guided && cnt >= (float)minSamples && dn_finite(M.x) && dn_finite(M.y)) {
    const float m = M.x / cnt;
    const float var = dn_max(M.y / cnt - m * m, 0.0f);
    const float vm = var / (cnt - 1.0f);
    float dl = 1.0f;
    if (hasAlbedo) { const F4 d = dn_divisor(true, B, albedoFloor); dl = dn_lum(d.x, d.y, d.z); }
    const float v = vm / (dl * dl);
    if (v <= kDenoiseMaxVariance) { r.v = v; r.known = 1.0f; } // (false for NaN)
  }
  return r;
}

// vt of a pixel whose variance is known: the 3 x 3 average of v over the known in-image pixels at unit spacing (the pixel itself counts: gsum >= 1/4)
template <typename FetchV>
GI_DENOISE_HD inline float dn_variance_average(uint32_t width, uint32_t height, uint32_t px, uint32_t py, FetchV&& fetchV)
{
  float acc = 0.0f, gsum = 0.0f;
  for (int dy = -1; dy <= 1; dy++) {
    const int32_t qy = (int32_t)py + dy;
    if (qy < 0 || qy >= (int32_t)height) continue;
    for (int dx = -1; dx <= 1; dx++) {
      const int32_t qx = (int32_t)px + dx;
      if (qx < 0 || qx >= (int32_t)width) continue;
      const DnV vq = fetchV((uint32_t)qx, (uint32_t)qy);
      if (vq.known == 0.0f) continue;
      const float g = dn_g(dy) * dn_g(dx);
      acc = acc + g * vq.v; gsum = gsum + g;
    }
  }
  return acc / gsum;
}

// One guided pixel of one pass of the variance-guided filter.  fetchX / fetchG as dn_filter_pixel's; fetchV(qx, qy) -> the V record of an in-image pixel;
// vtOf() -> the pixel's vt (asked only where its variance is known): dn_variance_average on the spot, or the word a launch of its own stored.
// Returns x' (w is not set); vOut: the pixel's record of the next V plane
template <typename FetchX, typename FetchG, typename FetchV, typename VtOf>
GI_DENOISE_HD inline F4 dn_filter_pixel_var(const DenoiseVarPass& Q, uint32_t px, uint32_t py, const F4& xp, const F4& gp, const DnV& vp, FetchX&& fetchX,
    FetchG&& fetchG, FetchV&& fetchV, VtOf&& vtOf, DnV& vOut)
{
  const DenoisePass& P = Q.base;
  vOut = vp;
  const bool known = vp.known != 0.0f;
  bool byVariance = false; // this pass weighs the pixel's taps by its variance
  float den = 1.0f, lp = 0.0f;
  if (known) {
    den = Q.sv2 * (vtOf() + Q.varianceFloor);
    lp = dn_lum(xp.x, xp.y, xp.z);
    byVariance = dn_finite(den) && dn_finite(lp);
  }
  float a0 = 0.0f, a1 = 0.0f, a2 = 0.0f, wsum = 0.0f, vs = 0.0f, vw = 0.0f;
  for (int dy = -2; dy <= 2; dy++) {
    const int32_t qy = (int32_t)py + dy * (int32_t)P.step;
    if (qy < 0 || qy >= (int32_t)P.height) continue;
    for (int dx = -2; dx <= 2; dx++) {
      const int32_t qx = (int32_t)px + dx * (int32_t)P.step;
      if (qx < 0 || qx >= (int32_t)P.width) continue;
      const F4 xq = fetchX((uint32_t)qx, (uint32_t)qy);
      if (xq.w == 0.0f) continue;
      const F4 gq = fetchG((uint32_t)qx, (uint32_t)qy);
      float wn = dn_max(dn_dot(gp.x, gp.y, gp.z, gq.x, gq.y, gq.z), 0.0f);
      for (uint32_t k = 0; k < P.normalSquarings; k++) wn = wn * wn;
      const float dz = (gp.w - gq.w) * P.invSz;
      const float wz = 1.0f / (1.0f + dz * dz);
      float wc;
      if (byVariance) { const float dl = lp - dn_lum(xq.x, xq.y, xq.z); wc = 1.0f / (1.0f + (dl * dl) / den); }
      else { const float c0 = xp.x - xq.x, c1 = xp.y - xq.y, c2 = xp.z - xq.z; wc = 1.0f / (1.0f + dn_dot(c0, c1, c2, c0, c1, c2) * P.invSc); }
      const float w = (dn_h(dy) * dn_h(dx)) * ((wn * wz) * wc);
      a0 = a0 + w * xq.x; a1 = a1 + w * xq.y; a2 = a2 + w * xq.z;
      wsum = wsum + w;
      if (known) {
        const DnV vq = fetchV((uint32_t)qx, (uint32_t)qy);
        if (vq.known != 0.0f) { vs = vs + (w * w) * vq.v; vw = vw + w; }
      }
    }
  }
  F4 r = xp;
  if (wsum > 0.0f) { r.x = a0 / wsum; r.y = a1 / wsum; r.z = a2 / wsum; }
  if (known) { const float s2 = vw * vw; if (s2 > 0.0f) vOut.v = vs / s2; }
  return r;
}

inline void denoisePrepareVarianceHost(const F4* X, const F4* moments, const F4* albedo, uint32_t width, uint32_t height, float albedoFloor, uint32_t minSamples, DnV* V)
{
  const size_t n = (size_t)width * height;
  for (size_t p = 0; p < n; p++) V[p] = dn_prepare_variance(moments[p], minSamples, X[p].w != 0.0f, albedo != nullptr, albedo ? albedo[p] : F4{}, albedoFloor);
}

// `dst`: the next x plane, or with the last pass the output image; Vnext: the next V plane (not written by the last pass; may then be null)
inline void denoiseVarPassHost(const DenoiseVarPass& Q, const F4* X, const F4* G, const DnV* V, F4* dst, DnV* Vnext, const F4* color, const F4* albedo)
{
  const DenoisePass& P = Q.base;
  for (uint32_t py = 0; py < P.height; py++)
    for (uint32_t px = 0; px < P.width; px++) {
      const size_t p = (size_t)py * P.width + px;
      const F4 xp = X[p];
      const bool guided = xp.w != 0.0f;
      F4 r = xp; DnV vNew = V[p];
      if (guided) {
        const auto fetchV = [&](uint32_t qx, uint32_t qy) { return V[(size_t)qy * P.width + qx]; };
        r = dn_filter_pixel_var(Q, px, py, xp, G[p], V[p], [&](uint32_t qx, uint32_t qy) { return X[(size_t)qy * P.width + qx]; },
            [&](uint32_t qx, uint32_t qy) { return G[(size_t)qy * P.width + qx]; }, fetchV, [&] { return dn_variance_average(P.width, P.height, px, py, fetchV); }, vNew);
        r.w = xp.w;
      }
      dst[p] = dn_store_pixel(P, r, guided, color[p], albedo != nullptr, albedo ? albedo[p] : F4{});
      if (!P.last) Vnext[p] = vNew;
    }
}

// ---- the host forms of the two kernels (GI_C_DENOISE_SOURCE_HOST_FORM) ------------------------------------------------------------------------------------
inline void denoisePrepareHost(const F4* color, const F4* normal, const float* depth, const F4* albedo, uint32_t width, uint32_t height, float albedoFloor,
    float backgroundDepth, F4* X, F4* G)
{
  const size_t n = (size_t)width * height;
  for (size_t p = 0; p < n; p++) dn_prepare_pixel(color[p], normal[p], depth[p], albedo != nullptr, albedo ? albedo[p] : F4{}, albedoFloor, backgroundDepth, X[p], G[p]);
}

// `dst`: the next x plane, or with P.last the output image
inline void denoisePassHost(const DenoisePass& P, const F4* X, const F4* G, F4* dst, const F4* color, const F4* albedo)
{
  for (uint32_t py = 0; py < P.height; py++)
    for (uint32_t px = 0; px < P.width; px++) {
      const size_t p = (size_t)py * P.width + px;
      const F4 xp = X[p];
      const bool guided = xp.w != 0.0f;
      F4 r = xp;
      if (guided) {
        r = dn_filter_pixel(P, px, py, xp, G[p], [&](uint32_t qx, uint32_t qy) { return X[(size_t)qy * P.width + qx]; },
            [&](uint32_t qx, uint32_t qy) { return G[(size_t)qy * P.width + qx]; });
        r.w = xp.w;
      }
      dst[p] = dn_store_pixel(P, r, guided, color[p], albedo != nullptr, albedo ? albedo[p] : F4{});
    }
}

// ---- gi_denoise.hip ------------------------------------------------------------------------------------------------------------------------------------
#if !defined(GI_DENOISE_HOST_ONLY)
// Every pointer is a device block of width x height records (F4; depth: float); albedo may be null.  X, G, Xnext: three different blocks.
bool launchDenoisePrepare(hipStream_t s, const F4* color, const F4* normal, const float* depth, const F4* albedo, uint32_t width, uint32_t height,
    float albedoFloor, float backgroundDepth, F4* X, F4* G);
// form: 0 = the default (an LDS tile with a 2 x step halo at steps 1 and 2, direct 16-byte loads above), 1 = direct loads at every step, 2 = the tile wherever
// it fits (steps 1, 2 and 4).  Every form stores the same bytes.  With P.last, dst is the output image and color / albedo (may be null) are read again
bool launchDenoisePass(hipStream_t s, const DenoisePass& P, const F4* X, const F4* G, F4* dst, const F4* color, const F4* albedo, uint32_t form);
// ---- gi_denoise_var.hip: the variance-guided filter's kernels.  V, Vnext: blocks of width x height DnV records (Vnext may be null with the last pass)
bool launchDenoisePrepareVariance(hipStream_t s, const F4* X, const F4* moments, const F4* albedo, uint32_t width, uint32_t height, float albedoFloor,
    uint32_t minSamples, DnV* V);
// form: as launchDenoisePass (the tile holds three planes); 3 = the default's tiling with vt of the direct-load steps made by a launch of its own
// (k_denoise_vt into `vt`, width x height floats; with any other form `vt` may be null) instead of nine loads in the pass.  Every form stores the same bytes
bool launchDenoiseVarPass(hipStream_t s, const DenoiseVarPass& Q, const F4* X, const F4* G, const DnV* V, F4* dst, DnV* Vnext, const F4* color, const F4* albedo,
    uint32_t form, float* vt);
#endif

} // namespace gi

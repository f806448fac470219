// gi_miss_rect.h -- the miss rectangle of a fused frame (host only, no device call): an image-space rectangle [x0, x1) x [y0, y1) outside which EVERY camera
// ray make_camera_ray (gi_stages.h) can produce for the pixel fails ray_misses_box against the scene's bounds.  k_path hands out no work for such pixels and
// k_accumulate sums the constant their samples are (gi_render.cpp scheduleFrame).
//
// Why the rectangle is conservative.  The kernel's ray through image-plane position (u, v) -- u = px + sox, v = py + soy in pixels -- has the direction
// D(u, v) = A0 + u A1 + v A2 with A0 = L - camPos, A1 = camRight WX, A2 = camUp HY (the float values of FrameUniforms, taken to double here).
//  1. A point X is on that ray iff X - camPos = t (A0 + u A1 + v A2) with t > 0: solving the 3 x 3 system for (t, t u, t v) projects X to (u, v).  On the
//     half space t > 0 this projection maps convex sets to convex sets, so a box whose eight corners all have t > 0 projects INTO the bounding rectangle
//     [uMin, uMax] x [vMin, vMax] of its projected corners: a ray whose (u, v) lies outside that rectangle meets no point of the box.  A box whose corners all
//     have t < 0 lies behind every ray (rays run towards t > 0): the rectangle is empty.  Anything else -- a corner near or across t = 0, the camera inside the
//     box, a singular system, a non-finite value -- gives the full frame.
//  2. The box projected is not the scene's bounds but the box ray_misses_box effectively tests: it moves every plane out by (|o| + max(|lo|, |hi|)) x 4e-6 and
//     widens the slab interval by 1e-5 of |t|, which is a plane moved by at most (|o| + max(|lo|, |hi|)) x 1e-5 more; its own float rounding is a thirtieth
//     of that (gi_stages.h).  Here every plane moves out by 3e-5 of that magnitude -- twice what the device test can reach.
//  3. The device builds its ray in float: P = (L + camRight (px + sox) WX) + camUp (py + soy) HY, D = normalize(P - camPos).  Every operation rounds by at most
//     2^-24 of its result, all results are bounded by S = |L| + |camPos| + |A0| + (width + 10) |A1| + (height + 10) |A2|, and fewer than eight roundings reach
//     a component of D (the common scale factor of the normalisation does not turn the ray): the float ray is the exact ray of a position less than
//     4 x 2^-23 x S / min(|A1|, |A2|) pixels away.  The margin is ONE PIXEL PLUS FOUR TIMES THAT (a camera 20 000 units away with a 0.02 degree lens, where a
//     pixel step nears the float spacing of L, gets a margin of several pixels; ordinary cameras 1.0x).
//  4. The sub-pixel offset: sox, soy lie in 0.5 +- 4.97 with filter importance sampling (gi_fis_gauss clamps its uniform at 1e-38: the radius is at most
//     0.375 sqrt(-2 ln 1e-38) = 4.961), in [0, 1] with plain jitter, and are 0.5 without.  Pixel px is left of the rectangle when px + offHi < uMin - margin and
//     right of it when px + offLo > uMax + margin; rows alike.
// Clipping planes need nothing: they shrink [tMin, tMax], and an empty slab interval stays empty.  Thin-lens rays (depth of field with a lens radius) do not
// start at camPos: full frame.
#pragma once

#include <cmath>
#include <cstdint>

#include "gi_types.h"

namespace gi {

struct MissRect { uint32_t x0, y0, x1, y1; bool empty() const { return x1 <= x0 || y1 <= y0; } };

inline MissRect missRectFull(uint32_t width, uint32_t height) { return MissRect{0u, 0u, width, height}; }

// `U`: the camera terms and FLAG_JITTER / FLAG_FIS / FLAG_DOF of makeUniforms; `lo`, `hi`: the bounds the device tests against (FrameUniforms::sceneLo / sceneHi)
inline MissRect computeMissRect(const float lo[3], const float hi[3], const FrameUniforms& U, uint32_t width, uint32_t height)
{
  const MissRect full = missRectFull(width, height);
  if (width == 0u || height == 0u) return full;
  if ((U.flags & FLAG_DOF) && U.lensRadius > 0.0f) return full;
  double o[3], A[3][3], blo[3], bhi[3]; // A[k] = column k of the system
  bool inside = true;
  for (int a = 0; a < 3; a++) {
    o[a] = U.camPos[a];
    A[0][a] = (double)U.L[a] - o[a]; A[1][a] = (double)U.camRight[a] * (double)U.WX; A[2][a] = (double)U.camUp[a] * (double)U.HY;
    if (!(lo[a] <= hi[a])) return full;
    const double pad = (std::fabs(o[a]) + std::fmax(std::fabs((double)lo[a]), std::fabs((double)hi[a]))) * 3.0e-5 + 1.0e-30;
    blo[a] = (double)lo[a] - pad; bhi[a] = (double)hi[a] + pad;
    if (!std::isfinite(blo[a]) || !std::isfinite(bhi[a]) || !std::isfinite(o[a])) return full;
    inside = inside && o[a] >= blo[a] && o[a] <= bhi[a];
  }
  if (inside) return full;
  auto cross = [](const double* x, const double* y, double* r) { r[0] = x[1] * y[2] - x[2] * y[1]; r[1] = x[2] * y[0] - x[0] * y[2]; r[2] = x[0] * y[1] - x[1] * y[0]; };
  auto dot = [](const double* x, const double* y) { return x[0] * y[0] + x[1] * y[1] + x[2] * y[2]; };
  auto len = [&](const double* x) { return std::sqrt(dot(x, x)); };
  double c12[3], c20[3], c01[3];
  cross(A[1], A[2], c12); cross(A[2], A[0], c20); cross(A[0], A[1], c01);
  const double det = dot(A[0], c12), n0 = len(A[0]), n1 = len(A[1]), n2 = len(A[2]);
  if (!std::isfinite(det) || !(n0 > 0.0) || !(n1 > 0.0) || !(n2 > 0.0) || !(std::fabs(det) > 1.0e-9 * n0 * n1 * n2)) return full;
  // t = 1 is the image plane: a corner counts as in front / behind only a thousandth of that distance clear of the camera's plane
  const double tSafe = 1.0e-3;
  double uMin = INFINITY, uMax = -INFINITY, vMin = INFINITY, vMax = -INFINITY;
  int front = 0, behind = 0;
  for (int k = 0; k < 8; k++) {
    const double x[3] = {((k & 1) ? bhi[0] : blo[0]) - o[0], ((k & 2) ? bhi[1] : blo[1]) - o[1], ((k & 4) ? bhi[2] : blo[2]) - o[2]};
    const double t = dot(x, c12) / det, tu = dot(x, c20) / det, tv = dot(x, c01) / det;
    if (!std::isfinite(t) || !std::isfinite(tu) || !std::isfinite(tv)) return full;
    if (t > tSafe) {
      front++;
      const double u = tu / t, v = tv / t;
      if (!std::isfinite(u) || !std::isfinite(v)) return full;
      uMin = std::fmin(uMin, u); uMax = std::fmax(uMax, u); vMin = std::fmin(vMin, v); vMax = std::fmax(vMax, v);
    } else if (t < -tSafe) behind++;
  }
  if (behind == 8) return MissRect{0u, 0u, 0u, 0u};
  if (front != 8) return full;
  double nL = 0.0, nO = 0.0;
  for (int a = 0; a < 3; a++) { nL += (double)U.L[a] * (double)U.L[a]; nO += o[a] * o[a]; }
  const double S = std::sqrt(nL) + std::sqrt(nO) + n0 + ((double)width + 10.0) * n1 + ((double)height + 10.0) * n2;
  const double margin = 1.0 + 4.0 * (4.0 * 1.1920929e-7 * S / std::fmin(n1, n2));
  if (!std::isfinite(margin)) return full;
  double offLo = 0.5, offHi = 0.5;
  if (U.flags & FLAG_JITTER) { if (U.flags & FLAG_FIS) { offLo = 0.5 - 4.97; offHi = 0.5 + 4.97; } else { offLo = 0.0; offHi = 1.0; } }
  // first pixel that is not certainly left of / above the box, one past the last that is not certainly right of / below it, clamped to the frame
  auto first = [](double edge, uint32_t n) { const double f = std::ceil(edge); return f <= 0.0 ? 0u : (f >= (double)n ? n : (uint32_t)f); };
  auto past = [](double edge, uint32_t n) { const double f = std::floor(edge) + 1.0; return f <= 0.0 ? 0u : (f >= (double)n ? n : (uint32_t)f); };
  MissRect r{first(uMin - margin - offHi, width), first(vMin - margin - offHi, height), past(uMax + margin - offLo, width), past(vMax + margin - offLo, height)};
  if (r.empty()) return MissRect{0u, 0u, 0u, 0u};
  return r;
}

// The rectangle in the rows of a tile (image rows rowBegin, rowBegin + rowStride, ...: `tileRows` of them): tile rows [ty0, ty1)
inline void missRectTileRows(const MissRect& r, uint32_t rowBegin, uint32_t rowStride, uint32_t tileRows, uint32_t& ty0, uint32_t& ty1)
{
  auto firstRowAtOrAfter = [&](uint32_t y) { // smallest k with rowBegin + k * rowStride >= y
    if (y <= rowBegin) return 0u;
    const uint64_t k = ((uint64_t)(y - rowBegin) + rowStride - 1u) / rowStride;
    return (uint32_t)(k < tileRows ? k : tileRows);
  };
  ty0 = firstRowAtOrAfter(r.y0); ty1 = firstRowAtOrAfter(r.y1);
  if (r.empty() || ty1 < ty0) { ty0 = 0u; ty1 = 0u; }
}

} // namespace gi

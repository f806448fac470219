// moments_sanitize.cpp -- the host form of the sample-moments AOV (gi_moments.h: what gi_moments.hip's k_moments and giCDebugSampleMomentsHost run) under
// AddressSanitizer + UBSan, as a program of its own:
//   g++ -O1 -g -std=c++17 -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all -static-libasan -static-libubsan -Igatling_amd/csrc -Iinclude \
//       tests/cpp/moments_sanitize.cpp -o moments_sanitize && ./moments_sanitize
// Tiles of 1, 15 and 2 470 pixels with 1, 2, 9 and 17 samples per pixel, in both layouts, whole and as a slice with first > 0, with and without a previous M and
// a miss rectangle, are folded through arrays allocated at their exact sizes: a record read or a store outside them is the sanitizer's to see.  The records hold
// 0, denormals, 3e38, Inf and NaN.  Held here as well: a fold from zero does not look at M (it starts as NaN bytes), the layouts agree bytewise, n counts the
// samples, and 8 + 8 + 1 folds give the bytes of one fold of 17.
#define GI_MOMENTS_HOST_ONLY 1
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "gi_moments.h"

using namespace gi;

static uint32_t g_state = 12345u;
static float rnd() { g_state = g_state * 1664525u + 1013904223u; return (float)(g_state >> 8) * (1.0f / 16777216.0f); }

static int fail(const char* what, uint32_t w, uint32_t r, uint32_t spp) { printf("FAILED: %s at %u x %u, spp %u\n", what, w, r, spp); return 1; }

// per-pixel samples [pixel][spp] -> the layout asked for
static std::vector<F4> layout(const std::vector<F4>& pp, uint32_t pixels, uint32_t spp, bool pixelMajor)
{
  std::vector<F4> out(pp.size());
  for (uint32_t p = 0; p < pixels; p++) for (uint32_t s = 0; s < spp; s++) out[pixelMajor ? (size_t)p * spp + s : (size_t)s * pixels + p] = pp[(size_t)p * spp + s];
  return out;
}

static std::vector<F4> fold(MomentsFold F, const std::vector<F4>& buf, const std::vector<F4>* prev)
{
  std::vector<F4> M(F.pixelCount);
  if (prev) M = *prev; else memset(static_cast<void*>(M.data()), 0xff, M.size() * sizeof(F4));
  F.continues = prev ? 1u : 0u;
  momentsHost(F, buf.data(), M.data());
  return M;
}
static bool same(const std::vector<F4>& a, const std::vector<F4>& b) { return a.size() == b.size() && memcmp(a.data(), b.data(), a.size() * sizeof(F4)) == 0; }

int main()
{
  const uint32_t tiles[3][2] = {{1, 1}, {5, 3}, {65, 38}}, spps[4] = {1, 2, 9, 17};
  const float special[6] = {0.0f, 1e-41f, 3e-39f, 3e38f, std::numeric_limits<float>::infinity(), std::numeric_limits<float>::quiet_NaN()};
  for (const auto& t : tiles) for (uint32_t spp : spps) {
    const uint32_t w = t[0], r = t[1], pixels = w * r;
    std::vector<F4> pp((size_t)pixels * spp);
    for (size_t i = 0; i < pp.size(); i++) {
      pp[i] = F4{rnd() * 4.0f, rnd() * 4.0f, rnd() * 4.0f, 0.0f};
      if (i % 5 == 0) (&pp[i].x)[i % 3] = special[(i / 5) % 6];
    }
    std::vector<F4> byLayout[2];
    for (int pm = 0; pm < 2; pm++) {
      MomentsFold F{};
      F.pixelCount = pixels; F.imageWidth = w; F.rowBegin = 0u; F.rowStride = 1u; F.bufferSamples = spp; F.first = 0u; F.count = spp; F.pixelMajor = (uint32_t)pm;
      const std::vector<F4> buf = layout(pp, pixels, spp, pm != 0);
      const std::vector<F4> whole = fold(F, buf, nullptr);
      byLayout[pm] = whole;
      for (const F4& m : whole) if (m.z != (float)spp || m.w != 0.0f) return fail("n does not count the samples", w, r, spp);
      // a previous M, and a miss rectangle (one pixel: everything outside)
      const std::vector<F4> again = fold(F, buf, &whole);
      for (const F4& m : again) if (m.z != (float)(2u * spp)) return fail("a continued fold does not count on", w, r, spp);
      MomentsFold R = F;
      R.missRect = 1u; R.rectX0 = w > 1u ? 1u : 0u; R.rectX1 = w > 1u ? w - 1u : 0u; R.rectTy0 = 0u; R.rectTy1 = r > 1u ? r - 1u : 0u;
      R.missSample[0] = 0.25f; R.missSample[1] = 0.5f; R.missSample[2] = 1.0f;
      const std::vector<F4> rect = fold(R, buf, nullptr);
      const float Lc = mo_lum(0.25f, 0.5f, 1.0f);
      float s1 = 0.0f; for (uint32_t s = 0; s < spp; s++) s1 = s1 + Lc;
      if (rect[pixels - 1u].x != s1) return fail("the miss constant's sum", w, r, spp);
      // slices: [first, first + count) of the same buffer, continued piece by piece, give the whole fold's bytes
      const uint32_t cuts17[3] = {8u, 8u, 1u};
      std::vector<F4> acc; bool have = false; uint32_t at = 0u;
      for (uint32_t k = 0; at < spp; k++) {
        const uint32_t n = spp == 17u ? cuts17[k] : 1u;
        MomentsFold S = F; S.first = at; S.count = n;
        acc = fold(S, buf, have ? &acc : nullptr); have = true; at += n;
      }
      if (!same(acc, whole)) return fail("slices do not give the whole fold's bytes", w, r, spp);
      // ... and so do buffers of their own, of exactly the slice's size
      have = false; at = 0u;
      for (uint32_t k = 0; at < spp; k++) {
        const uint32_t n = spp == 17u ? cuts17[k] : 1u;
        std::vector<F4> part((size_t)pixels * n);
        for (uint32_t p = 0; p < pixels; p++) for (uint32_t s = 0; s < n; s++) part[(size_t)p * n + s] = pp[(size_t)p * spp + at + s];
        MomentsFold S = F; S.bufferSamples = n; S.count = n;
        acc = fold(S, layout(part, pixels, n, pm != 0), have ? &acc : nullptr); have = true; at += n;
      }
      if (!same(acc, whole)) return fail("separate buffers do not give the whole fold's bytes", w, r, spp);
    }
    if (!same(byLayout[0], byLayout[1])) return fail("the layouts disagree", w, r, spp);
  }
  // a row share: rows 1, 3, 5 of a 4 x 7 image; the other rows keep their bytes
  {
    MomentsFold F{};
    F.pixelCount = 12u; F.imageWidth = 4u; F.rowBegin = 1u; F.rowStride = 2u; F.bufferSamples = 3u; F.count = 3u; F.pixelMajor = 1u;
    std::vector<F4> buf(36u, F4{1.0f, 1.0f, 1.0f, 0.0f}), M(28u, F4{-1.0f, -1.0f, -1.0f, -1.0f});
    momentsHost(F, buf.data(), M.data());
    for (uint32_t y = 0; y < 7u; y++) for (uint32_t x = 0; x < 4u; x++) {
      const F4& m = M[y * 4u + x];
      if ((y % 2u == 1u) != (m.z == 3.0f) || (y % 2u == 0u && m.x != -1.0f)) return fail("a row share writes other rows", 4u, 7u, 3u);
    }
  }
  printf("moments sanitize ok\n");
  return 0;
}

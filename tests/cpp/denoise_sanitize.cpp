// denoise_sanitize.cpp -- the host form of the a-trous denoiser (gi_denoise.h: what gi_denoise.hip's kernels and giCDenoise's GI_C_DENOISE_SOURCE_HOST_FORM run)
// under AddressSanitizer + UBSan, as a program of its own:
//   g++ -O1 -g -std=c++17 -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all -static-libasan -static-libubsan -Igatling_amd/csrc -Iinclude \
//       tests/cpp/denoise_sanitize.cpp -o denoise_sanitize && ./denoise_sanitize
// Images of 1 x 1, 5 x 3, 37 x 19 and 130 x 70 pixels, 1 .. 6 iterations (at 6 the taps reach 64 pixels either side: past every one of these images), with
// and without albedo, are filtered through arrays allocated at their exact sizes: a tap read or a store outside the image is the sanitizer's to see.  The
// inputs hold background pixels, NaN and Inf colours, Inf depths, zero albedo and huge colours.  Held here as well: unguided pixels come out bytewise as
// they went in, alpha is passed through, and a constant colour over constant guides comes out as that constant (the weights are a partition of one).
// Exit status 0 and "denoise sanitize ok" on success.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <random>
#include <vector>

#define GI_DENOISE_HOST_ONLY
#include "gi_denoise.h"

using namespace gi;

static int failures = 0;
#define CHECK(c) do { if (!(c)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); failures++; } } while (0)

static std::vector<F4> run(uint32_t w, uint32_t h, uint32_t iterations, const std::vector<F4>& color, const std::vector<F4>& normal, const std::vector<float>& depth,
    const std::vector<F4>* albedo, std::vector<F4>& X0)
{
  const size_t n = (size_t)w * h;
  std::vector<F4> X[2] = {std::vector<F4>(n), std::vector<F4>(n)}, G(n), out(n);
  denoisePrepareHost(color.data(), normal.data(), depth.data(), albedo ? albedo->data() : nullptr, w, h, 1.0e-3f, 1.0f, X[0].data(), G.data());
  X0 = X[0];
  for (uint32_t i = 0; i < iterations; i++) {
    DenoisePass P{};
    P.width = w; P.height = h; P.step = 1u << i; P.normalSquarings = 4u; P.invSz = 1.0f / 0.02f; P.invSc = denoiseInvSc(2.0f, i); P.albedoFloor = 1.0e-3f;
    P.last = i + 1u == iterations;
    denoisePassHost(P, X[i & 1u].data(), G.data(), P.last ? out.data() : X[(i + 1u) & 1u].data(), color.data(), albedo ? albedo->data() : nullptr);
  }
  return out;
}

int main()
{
  const uint32_t sizes[4][2] = {{1, 1}, {5, 3}, {37, 19}, {130, 70}};
  std::mt19937 rng(7);
  std::uniform_real_distribution<float> U(0.0f, 1.0f);
  const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
  for (const auto& sz : sizes)
    for (uint32_t iterations = 1; iterations <= kDenoiseMaxIterations; iterations++)
      for (int withAlbedo = 0; withAlbedo < 2; withAlbedo++) {
        const uint32_t w = sz[0], h = sz[1];
        const size_t n = (size_t)w * h;
        std::vector<F4> color(n), normal(n), albedo(n);
        std::vector<float> depth(n);
        for (size_t p = 0; p < n; p++) {
          color[p] = F4{U(rng) * 2.0f, U(rng) * 2.0f, U(rng) * 2.0f, U(rng)};
          normal[p] = F4{U(rng), U(rng), U(rng), 0.0f};
          albedo[p] = F4{U(rng), U(rng), U(rng), 1.0f};
          depth[p] = 0.2f + 0.5f * U(rng);
        }
        if (n >= 15) {
          depth[0] = 1.0f; depth[n - 1] = 1.0f; color[1].x = nan; color[2].y = inf; depth[3] = inf; albedo[4] = F4{0, 0, 0, 1};
          color[5] = F4{3.0e38f, 3.0e38f, 3.0e38f, 0.5f}; albedo[5] = F4{0, 0, 0, 1}; normal[6].z = nan; depth[7] = -inf;
        }
        std::vector<F4> X0;
        const std::vector<F4> out = run(w, h, iterations, color, normal, depth, withAlbedo ? &albedo : nullptr, X0);
        for (size_t p = 0; p < n; p++) {
          CHECK(memcmp(&out[p].w, &color[p].w, 4) == 0);
          if (X0[p].w == 0.0f) CHECK(memcmp(&out[p], &color[p], 16) == 0);
        }
      }
  { // a constant image over constant guides is a fixed point up to the rounding of acc / wsum and of the albedo round trip
    const uint32_t w = 37, h = 19; const size_t n = (size_t)w * h;
    std::vector<F4> color(n, F4{0.5f, 0.25f, 0.125f, 1.0f}), normal(n, F4{0.5f, 0.5f, 1.0f, 0.0f}), X0;
    std::vector<float> depth(n, 0.5f);
    const std::vector<F4> out = run(w, h, 5, color, normal, depth, nullptr, X0);
    for (size_t p = 0; p < n; p++) CHECK(fabsf(out[p].x - 0.5f) <= 1.0e-6f && fabsf(out[p].y - 0.25f) <= 1.0e-6f && fabsf(out[p].z - 0.125f) <= 1.0e-6f);
  }
  if (failures) { printf("%d checks failed\n", failures); return 1; }
  printf("denoise sanitize ok\n");
  return 0;
}

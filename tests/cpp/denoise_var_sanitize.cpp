// denoise_var_sanitize.cpp -- the host form of the variance-guided denoiser (gi_denoise.h: what gi_denoise_var.hip's kernels and giCDenoiseVariance's
// GI_C_DENOISE_SOURCE_HOST_FORM run) under AddressSanitizer + UBSan, as a program of its own:
//   g++ -O1 -g -std=c++17 -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all -static-libasan -static-libubsan -Igatling_amd/csrc -Iinclude \
//       tests/cpp/denoise_var_sanitize.cpp -o denoise_var_sanitize && ./denoise_var_sanitize
// Images of 1 x 1, 5 x 3, 37 x 19 and 130 x 70 pixels, 1 .. 6 iterations, with and without albedo, through arrays allocated at their exact sizes (three planes:
// a tap read, a read of the 3 x 3 variance average or a store outside the image is the sanitizer's to see).  The moments hold n = 0, 1, 2, 64 and sums that are
// Inf and NaN; the guides hold background pixels, NaN and Inf colours, Inf depths, zero albedo and huge colours.  Held here as well: unguided pixels come out
// bytewise, alpha is passed through, `known` never changes, and with no pixel's variance known the result is the fixed filter's, bytewise.
// Exit status 0 and "denoise variance sanitize ok" on success.
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

static DenoisePass makePass(uint32_t w, uint32_t h, uint32_t i, uint32_t iterations)
{
  DenoisePass P{};
  P.width = w; P.height = h; P.step = 1u << i; P.normalSquarings = 4u; P.invSz = 1.0f / 0.02f; P.invSc = denoiseInvSc(2.0f, i); P.albedoFloor = 1.0e-3f;
  P.last = i + 1u == iterations;
  return P;
}

// moments == nullptr: the fixed filter
static std::vector<F4> run(uint32_t w, uint32_t h, uint32_t iterations, const std::vector<F4>& color, const std::vector<F4>& normal, const std::vector<float>& depth,
    const std::vector<F4>* albedo, const std::vector<F4>* moments, std::vector<F4>& X0)
{
  const size_t n = (size_t)w * h;
  std::vector<F4> X[2] = {std::vector<F4>(n), std::vector<F4>(n)}, G(n), out(n);
  std::vector<DnV> V[2] = {std::vector<DnV>(n), std::vector<DnV>(n)};
  const F4* alb = albedo ? albedo->data() : nullptr;
  denoisePrepareHost(color.data(), normal.data(), depth.data(), alb, w, h, 1.0e-3f, 1.0f, X[0].data(), G.data());
  if (moments) denoisePrepareVarianceHost(X[0].data(), moments->data(), alb, w, h, 1.0e-3f, 2u, V[0].data());
  X0 = X[0];
  const std::vector<DnV> V0 = V[0];
  for (uint32_t i = 0; i < iterations; i++) {
    const DenoisePass P = makePass(w, h, i, iterations);
    F4* dst = P.last ? out.data() : X[(i + 1u) & 1u].data();
    if (moments) {
      denoiseVarPassHost(DenoiseVarPass{P, 16.0f, 1.0e-6f}, X[i & 1u].data(), G.data(), V[i & 1u].data(), dst, P.last ? nullptr : V[(i + 1u) & 1u].data(), color.data(), alb);
      if (!P.last) for (size_t p = 0; p < n; p++) {
        const DnV& a = V[(i + 1u) & 1u][p];
        CHECK(a.known == V0[p].known && (a.known != 0.0f || a.v == 0.0f) && a.v >= 0.0f);
      }
    } else denoisePassHost(P, X[i & 1u].data(), G.data(), dst, color.data(), alb);
  }
  return out;
}

int main()
{
  const uint32_t sizes[4][2] = {{1, 1}, {5, 3}, {37, 19}, {130, 70}};
  std::mt19937 rng(11);
  std::uniform_real_distribution<float> U(0.0f, 1.0f);
  const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
  const float counts[4] = {0.0f, 1.0f, 2.0f, 64.0f};
  for (const auto& sz : sizes)
    for (uint32_t iterations = 1; iterations <= kDenoiseMaxIterations; iterations++)
      for (int withAlbedo = 0; withAlbedo < 2; withAlbedo++) {
        const uint32_t w = sz[0], h = sz[1];
        const size_t n = (size_t)w * h;
        std::vector<F4> color(n), normal(n), albedo(n), moments(n), none(n, F4{0.0f, 0.0f, 0.0f, 0.0f});
        std::vector<float> depth(n);
        for (size_t p = 0; p < n; p++) {
          color[p] = F4{U(rng) * 2.0f, U(rng) * 2.0f, U(rng) * 2.0f, U(rng)};
          normal[p] = F4{U(rng), U(rng), U(rng), 0.0f};
          albedo[p] = F4{U(rng), U(rng), U(rng), 1.0f};
          depth[p] = 0.2f + 0.5f * U(rng);
          const float c = n == 1 ? 2.0f : counts[p % 4], L = dn_lum(color[p].x, color[p].y, color[p].z);
          moments[p] = F4{c * L, c * (L * L + U(rng) * L * L), c, 0.0f};
        }
        if (n >= 15) {
          depth[0] = 1.0f; depth[n - 1] = 1.0f; color[1].x = nan; color[2].y = inf; depth[3] = inf; albedo[4] = F4{0, 0, 0, 1};
          color[5] = F4{3.0e38f, 3.0e38f, 3.0e38f, 0.5f}; albedo[5] = F4{0, 0, 0, 1}; normal[6].z = nan; depth[7] = -inf;
          moments[8].x = inf; moments[9].y = inf; moments[10].x = nan; moments[11].y = nan; moments[12] = F4{2.0f, 3.0e38f, 2.0f, 0.0f};
        }
        std::vector<F4> X0, X1;
        const std::vector<F4>* alb = withAlbedo ? &albedo : nullptr;
        const std::vector<F4> out = run(w, h, iterations, color, normal, depth, alb, &moments, X0);
        for (size_t p = 0; p < n; p++) {
          CHECK(memcmp(&out[p].w, &color[p].w, 4) == 0);
          if (X0[p].w == 0.0f) CHECK(memcmp(&out[p], &color[p], 16) == 0);
        }
        // no pixel's variance known: the fixed filter, bytewise
        const std::vector<F4> viaVar = run(w, h, iterations, color, normal, depth, alb, &none, X1), fixed = run(w, h, iterations, color, normal, depth, alb, nullptr, X1);
        CHECK(memcmp(viaVar.data(), fixed.data(), n * sizeof(F4)) == 0);
      }
  if (failures) { printf("%d checks failed\n", failures); return 1; }
  printf("denoise variance sanitize ok\n");
  return 0;
}

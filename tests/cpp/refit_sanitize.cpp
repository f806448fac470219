// refit_sanitize.cpp -- the host form of the BVH refit (gi_refit.h) and the host builder (bvh8.cpp) under AddressSanitizer + UBSan, as a program of its own:
//   g++ -O1 -g -std=c++17 -pthread -fsanitize=address,undefined -fno-sanitize-recover=all -static-libasan -static-libubsan -Igatling_amd/csrc -Iinclude tests/cpp/refit_sanitize.cpp \
//       gatling_amd/csrc/bvh8.cpp -o refit_sanitize && ./refit_sanitize
// Builds trees over random triangle soups of several sizes, moves the triangles (smoothly, scattered, collapsed to a point, near 1e17, not at all), refits,
// and checks that every triangle lies inside the dequantised box of its leaf slot.  Exit status 0 and "refit sanitize ok" on success.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "bvh8.h"
#include "gi_refit.h"

using namespace gi;

static int leafViolations(const std::vector<Node8>& nodes, const std::vector<TriRec>& tris)
{
  int bad = 0;
  for (const Node8& n : nodes)
    for (int s = 0; s < 8; s++) {
      const uint32_t meta = n.meta[s];
      if (meta == 0u || ((n.imask >> s) & 1u)) continue;
      const uint32_t unary = meta >> 5, off = meta & 31u, cnt = unary == 1u ? 1u : unary == 3u ? 2u : unary == 7u ? 3u : 0u;
      for (uint32_t k = 0; k < cnt; k++) {
        const TriRec& t = tris[n.triBase + off + k];
        for (int a = 0; a < 3; a++) {
          uint32_t eb = (uint32_t)n.e[a] << 23; float scale; memcpy(&scale, &eb, 4);
          const float lo = n.p[a] + (float)n.qlo[a][s] * scale, hi = n.p[a] + (float)n.qhi[a][s] * scale;
          const float x[3] = {t.v0[a], t.v0[a] + t.e1[a], t.v0[a] + t.e2[a]};
          for (float v : x) if (v < lo || v > hi) bad++;
        }
      }
    }
  return bad;
}

int main()
{
  std::mt19937 rng(4711);
  std::uniform_real_distribution<float> centre(-5.0f, 5.0f), corner(-0.2f, 0.2f), far(-50.0f, 50.0f);
  const uint32_t sizes[] = {1u, 3u, 46u, 777u, 20000u};
  int bad = 0;
  for (uint32_t n : sizes)
    for (int motion = 0; motion < 5; motion++) {
      std::vector<float> A(9 * (size_t)n), B(9 * (size_t)n);
      for (uint32_t i = 0; i < n; i++) {
        const float c[3] = {centre(rng), centre(rng), centre(rng)}, to[3] = {far(rng), far(rng), far(rng)};
        for (int k = 0; k < 9; k++) {
          float& a = A[9 * (size_t)i + k]; float& b = B[9 * (size_t)i + k];
          a = c[k % 3] + corner(rng);
          b = motion == 0 ? a + 0.15f * std::sin(1.3f * a + 0.7f) : motion == 1 ? a - c[k % 3] + to[k % 3] : motion == 2 ? 0.25f : motion == 3 ? a * 1.0e16f : a;
        }
      }
      std::vector<TriRec> tris(n);
      for (uint32_t i = 0; i < n; i++) {
        const float* p = &A[9 * (size_t)i];
        for (int a = 0; a < 3; a++) { tris[i].v0[a] = p[a]; tris[i].e1[a] = p[3 + a] - p[a]; tris[i].e2[a] = p[6 + a] - p[a]; }
        tris[i].instance = 0; tris[i].prim = i; tris[i].origId = i; tris[i].matFlags = 0; tris[i].vi[0] = tris[i].vi[1] = tris[i].vi[2] = 0;
      }
      Bvh8 bvh; buildBvh8(tris, bvh);
      for (TriRec& t : bvh.tris) {
        const float* p = &B[9 * (size_t)t.origId];
        for (int a = 0; a < 3; a++) { t.v0[a] = p[a]; t.e1[a] = p[3 + a] - p[a]; t.e2[a] = p[6 + a] - p[a]; }
      }
      std::vector<float> boxes(bvh.nodes.size() * 8u, 0.0f);
      const RefitScene S{bvh.tris.data(), (uint32_t)bvh.tris.size(), nullptr, 0u, nullptr, 0u};
      refitHost(bvh.nodes.data(), (uint32_t)bvh.nodes.size(), 0u, boxes.data(), S);
      const int v = leafViolations(bvh.nodes, bvh.tris);
      if (v || bvh.levelStart.size() != (size_t)bvh.maxDepth + 1u || bvh.levelStart.back() != bvh.nodes.size()) {
        printf("n %u motion %d: %d violation(s), %zu level starts for %u levels\n", n, motion, v, bvh.levelStart.size(), bvh.maxDepth); bad++; }
    }
  if (bad) return 1;
  printf("refit sanitize ok\n");
  return 0;
}

// blas_refit_sanitize.cpp -- the host form of the BLAS refit of the two-level layout (gi_blas.h) and the box-mode host builder (bvh8.cpp buildBvh8Boxes) under
// AddressSanitizer + UBSan, as a program of its own:
//   g++ -O1 -g -std=c++17 -pthread -fsanitize=address,undefined -fno-sanitize-recover=all -static-libasan -static-libubsan -Igatling_amd/csrc -Iinclude \
//       tests/cpp/blas_refit_sanitize.cpp gatling_amd/csrc/bvh8.cpp -o blas_refit_sanitize && ./blas_refit_sanitize
// Builds one BLAS over random triangle soups of several sizes as the scene build does (padded object-space face boxes), moves the points (smoothly,
// scattered, collapsed to a point, near 1e17, not at all), gives the records their new corners by prim, refits, and runs the conservative check; a refit of
// unchanged points must leave the build's bytes.  Exit status 0 and "blas refit sanitize ok" on success.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "bvh8.h"
#include "gi_blas.h"

using namespace gi;

int main()
{
  std::mt19937 rng(1717);
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
      // the build: padded face boxes, the tree over them, the records in the builder's order
      std::vector<float> faceBoxes(6 * (size_t)n);
      for (uint32_t f = 0; f < n; f++) {
        float p[3][3], lo[3], hi[3];
        memcpy(p, &A[9 * (size_t)f], 36);
        if (!blas_face_box(p, lo, hi)) { printf("n %u: an unusable face in the input\n", n); return 1; }
        for (int a = 0; a < 3; a++) { faceBoxes[6 * (size_t)f + a] = lo[a]; faceBoxes[6 * (size_t)f + 3 + a] = hi[a]; }
      }
      Bvh8 bvh; std::vector<uint32_t> order;
      buildBvh8Boxes(faceBoxes.data(), n, bvh, order);
      std::vector<BlasTri> tris(n);
      for (uint32_t i = 0; i < n; i++) { BlasTri t{}; const float* p = &A[9 * (size_t)order[i]]; memcpy(t.p0, p, 12); memcpy(t.p1, p + 3, 12); memcpy(t.p2, p + 6, 12); t.prim = order[i]; tris[i] = t; }
      const std::vector<Node8> builtNodes(bvh.nodes); const std::vector<BlasTri> builtTris(tris);
      // the edit: shading records with the new corners, the records by prim, the refit children before parents
      std::vector<TriShade> shade(n);
      for (uint32_t f = 0; f < n; f++) { TriShade q{}; memcpy(q.p, &B[9 * (size_t)f], 36); shade[f] = q; }
      int moved = 0;
      for (uint32_t i = 0; i < n; i++) if (!blas_tri_from_shade(tris[i], shade.data(), n, 0u, n)) moved++;
      const uint32_t nodeCount = (uint32_t)bvh.nodes.size();
      std::vector<float> boxes(8 * (size_t)nodeCount, 0.0f), under(6 * (size_t)nodeCount, 0.0f); std::vector<uint8_t> seen(n, 0);
      blasRefitHost(bvh.nodes.data(), nodeCount, 0u, nodeCount, boxes.data(), tris.data(), n);
      const uint32_t v = blasConservativeViolations(bvh.nodes.data(), nodeCount, 0u, nodeCount, tris.data(), n, 0u, n, under.data(), seen.data());
      const bool sameBytes = motion != 4 || (memcmp(bvh.nodes.data(), builtNodes.data(), nodeCount * sizeof(Node8)) == 0 && memcmp(tris.data(), builtTris.data(), n * sizeof(BlasTri)) == 0);
      if (v || moved || !sameBytes || bvh.levelStart.size() != (size_t)bvh.maxDepth + 1u || bvh.levelStart.back() != nodeCount) {
        printf("n %u motion %d: %u violation(s), %d record(s) refused, same bytes %d, %zu level starts for %u levels\n", n, motion, v, moved, (int)sameBytes,
               bvh.levelStart.size(), bvh.maxDepth); bad++; }
    }
  if (bad) return 1;
  printf("blas refit sanitize ok\n");
  return 0;
}

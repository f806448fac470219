// blas_build_host_main.cpp -- the host form of the device BLAS builder (gi_blas_build_host.cpp over gi_tlas_build_host.cpp and gi_bvh_stages.h) under
// AddressSanitizer + UBSan, as a program of its own (only the declarations of the HIP headers are used; nothing touches a device):
//   g++ -O1 -g -std=c++17 -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all -static-libasan -static-libubsan -D__HIP_PLATFORM_AMD__ \
//       -I${ROCM_PATH:-/opt/rocm}/include -Igatling_amd/csrc -Iinclude tests/cpp/blas_build_host_main.cpp gatling_amd/csrc/gi_blas_build_host.cpp \
//       gatling_amd/csrc/gi_tlas_build_host.cpp -o blas_build_host_main && ./blas_build_host_main
// Builds the BLAS of triangle soups of 0 .. 6 000 faces, of identical faces, of faces without area, of meshes with NaN and out-of-range corners and of a long
// thin strip, under budgets 12, 7 and the smallest feasible one; holds every tree to the level table, to the conservative check of gi_blas.h and to the refit
// identity (a BLAS refit over the unchanged points changes no byte); a face index outside the vertices must be refused.  Exit status 0 and "blas build host
// ok" on success.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <random>
#include <vector>

#include "gi_blas.h"
#include "gi_blas_build.h"

using namespace gi;

namespace {

struct Mesh { std::vector<GiCVertex> v; std::vector<GiCFace> f; };

Mesh soup(uint32_t nf, uint32_t seed)
{
  std::mt19937 rng(seed);
  std::uniform_real_distribution<float> centre(-20.0f, 20.0f), corner(-0.3f, 0.3f);
  Mesh m; m.v.resize(3 * (size_t)nf); m.f.resize(nf);
  for (uint32_t i = 0; i < nf; i++) {
    const float c[3] = {centre(rng), centre(rng), centre(rng)};
    for (uint32_t k = 0; k < 3; k++) { GiCVertex x{}; for (int a = 0; a < 3; a++) x.pos[a] = c[a] + corner(rng); m.v[3 * (size_t)i + k] = x; m.f[i].v_i[k] = 3 * i + k; }
  }
  return m;
}
Mesh strip(uint32_t nf)
{
  const uint32_t q = (nf + 1) / 2;
  Mesh m; m.v.resize(2 * (size_t)(q + 1));
  for (uint32_t i = 0; i <= q; i++) { GiCVertex a{}, b{}; a.pos[0] = b.pos[0] = 0.25f * (float)i; b.pos[1] = 0.01f; m.v[2 * i] = a; m.v[2 * i + 1] = b; }
  for (uint32_t i = 0; i < q && m.f.size() < nf; i++) {
    m.f.push_back(GiCFace{{2 * i, 2 * i + 2, 2 * i + 1}});
    if (m.f.size() < nf) m.f.push_back(GiCFace{{2 * i + 1, 2 * i + 2, 2 * i + 3}});
  }
  return m;
}

// one build and its checks; returns the violations (TLAS_BUILD_TOO_DEEP is reported through `deep`)
int check(const Mesh& m, uint32_t budget, bool& deep)
{
  Bvh8 b; std::vector<uint32_t> order; float mlo[3], mhi[3]; BlasBuildInfo info;
  const uint32_t nf = (uint32_t)m.f.size();
  const int rc = buildBlasHost(m.v.data(), m.v.size(), m.f.data(), nf, budget, 16, b, order, mlo, mhi, info);
  deep = rc == TLAS_BUILD_TOO_DEEP;
  if (deep) return 0;
  if (rc != TLAS_BUILD_OK) return 1;
  int bad = 0;
  const uint32_t nodeCount = (uint32_t)b.nodes.size();
  if (order.size() != nf || nodeCount == 0u || b.maxDepth == 0u || b.maxDepth > budget || b.levelStart.size() != (size_t)b.maxDepth + 1u || b.levelStart.front() != 0u ||
      b.levelStart.back() != nodeCount) return 1;
  std::vector<BlasTri> tris(nf);
  for (uint32_t i = 0; i < nf; i++) {
    const uint32_t f = order[i];
    if (f >= nf) return 1;
    BlasTri t{}; memcpy(t.p0, m.v[m.f[f].v_i[0]].pos, 12); memcpy(t.p1, m.v[m.f[f].v_i[1]].pos, 12); memcpy(t.p2, m.v[m.f[f].v_i[2]].pos, 12); t.prim = f;
    tris[i] = t;
  }
  std::vector<float> under(6 * (size_t)nodeCount, 0.0f); std::vector<uint8_t> seen(nf + 1u, 0);
  bad += (int)blasConservativeViolations(b.nodes.data(), nodeCount, 0u, nodeCount, tris.data(), nf, 0u, nf, under.data(), seen.data());
  std::vector<Node8> refitted(b.nodes); std::vector<float> boxes(8 * (size_t)nodeCount, 0.0f);
  blasRefitHost(refitted.data(), nodeCount, 0u, nodeCount, boxes.data(), tris.data(), nf);
  if (memcmp(refitted.data(), b.nodes.data(), (size_t)nodeCount * sizeof(Node8)) != 0) bad++;
  return bad;
}

} // namespace

int main()
{
  int bad = 0;
  std::vector<Mesh> meshes;
  for (uint32_t nf : {0u, 1u, 3u, 4u, 24u, 25u, 2048u, 2049u, 6000u}) meshes.push_back(soup(nf, 1u + nf));
  { Mesh m = soup(1, 3); m.f.assign(300, m.f[0]); meshes.push_back(m); }                                       // identical faces
  { Mesh m = soup(500, 5); for (uint32_t i = 0; i < 500; i += 2) m.v[3 * i + 1] = m.v[3 * i + 2] = m.v[3 * i]; meshes.push_back(m); } // no area
  { Mesh m = soup(400, 7); m.v[22].pos[2] = std::numeric_limits<float>::quiet_NaN(); m.v[633].pos[0] = 2.0e18f; meshes.push_back(m); }
  meshes.push_back(strip(600));
  for (const Mesh& m : meshes) {
    uint32_t feasible = 0;
    for (uint32_t budget = 0; budget <= kBlasMaxBudget; budget++) {
      bool deep = false;
      const int v = check(m, budget, deep);
      if (v) { printf("%zu faces, budget %u: %d violation(s)\n", m.f.size(), budget, v); bad += v; }
      if (!deep && feasible == 0u) feasible = budget;
      if (deep && feasible != 0u) { printf("%zu faces: too deep at budget %u above a feasible one\n", m.f.size(), budget); bad++; }
    }
    if (feasible == 0u) { printf("%zu faces: no budget is feasible\n", m.f.size()); bad++; }
  }
  { // a stray index never reaches the stages
    Mesh m = soup(10, 9); m.f[4].v_i[1] = (uint32_t)m.v.size();
    Bvh8 b; std::vector<uint32_t> order; float mlo[3], mhi[3]; BlasBuildInfo info;
    if (buildBlasHost(m.v.data(), m.v.size(), m.f.data(), m.f.size(), 12, 16, b, order, mlo, mhi, info) != TLAS_BUILD_ERROR) { printf("a stray index was accepted\n"); bad++; }
  }
  if (bad) { printf("blas build host: %d problem(s)\n", bad); return 1; }
  printf("blas build host ok\n");
  return 0;
}

// vispatch_sanitize.cpp -- the host forms of the kernels of a visibility update of the two-level layout (gi_vispatch.h: patchVisibilityTwoLevelHost,
// patchInstTravHost, flatIdViolations) and the masked-box TLAS plan (tlasMaskHiddenBoxes + bvh8.cpp buildBvh8Boxes) under AddressSanitizer + UBSan, as a
// program of its own:
//   g++ -O1 -g -std=c++17 -pthread -fsanitize=address,undefined -fno-sanitize-recover=all -static-libasan -static-libubsan -Igatling_amd/csrc -Iinclude \
//       tests/cpp/vispatch_sanitize.cpp gatling_amd/csrc/bvh8.cpp -o vispatch_sanitize && ./vispatch_sanitize
// Synthetic scenes of 1 .. 257 instances with face counts drawn so that the resident triangles hit 1, 255, 256, 257 and 4 097, laid out in a shuffled flat
// order, go through chains of edits (first hidden, last hidden, alternate, the complement, everything shown, nothing changed); after every edit the rules the
// walk relies on must hold (visible ids a permutation, the table names them, triBase + prim is the id, hidden records have zero edges, shown records are
// whole again), and after "everything shown" the arrays must be bytewise the build's.  The TLAS over masked boxes must name exactly the visible instances.
// Exit status 0 and "vispatch sanitize ok" on success.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "bvh8.h"
#include "gi_vispatch.h"

using namespace gi;

namespace {

struct Scene {
  std::vector<uint32_t> nf, first, base; std::vector<uint8_t> hidden;
  std::vector<InstanceRec> instances; std::vector<InstTrav> instTrav; std::vector<TriShade> shade; std::vector<TriRec> tris; std::vector<uint32_t> flat;
  std::vector<float> boxes;
};

// per-instance face counts that sum to `total` (every instance at least one face where total allows it; the rest spread unevenly)
std::vector<uint32_t> faceCounts(uint32_t instances, uint32_t total, std::mt19937& rng)
{
  std::vector<uint32_t> nf(instances, 0u);
  for (uint32_t k = 0; k < total; k++) nf[k < instances ? k : rng() % instances]++;
  return nf;
}

Scene build(const std::vector<uint32_t>& nf, std::mt19937& rng)
{
  Scene S; S.nf = nf;
  const uint32_t ni = (uint32_t)nf.size();
  std::uniform_real_distribution<float> coord(-2.0f, 2.0f);
  S.shade.resize(31);
  for (TriShade& q : S.shade) { q = TriShade{}; for (int k = 0; k < 3; k++) for (int a = 0; a < 3; a++) q.p[k][a] = coord(rng); }
  S.first.resize(ni); S.base.resize(ni); S.hidden.assign(ni, 0); S.instances.resize(ni); S.instTrav.resize(ni); S.boxes.resize(6u * ni);
  uint32_t n = 0;
  for (uint32_t i = 0; i < ni; i++) {
    InstanceRec ir{}; const float o2w[12] = {1.0f, 0.1f, 0.0f, coord(rng), 0.0f, 0.9f, 0.2f, coord(rng), -0.1f, 0.0f, 1.1f, coord(rng)};
    memcpy(ir.o2w, o2w, sizeof(o2w)); ir.mesh = i; S.instances[i] = ir;
    InstTrav tv{}; memcpy(tv.o2w, o2w, sizeof(o2w)); tv.triBase = n; tv.matFlags = i; S.instTrav[i] = tv;
    for (int a = 0; a < 3; a++) { S.boxes[6u * i + a] = o2w[4 * a + 3] - 1.0f; S.boxes[6u * i + 3 + a] = o2w[4 * a + 3] + 1.0f; }
    S.first[i] = S.base[i] = n; n += nf[i];
  }
  std::vector<uint32_t> place(n);
  for (uint32_t i = 0; i < n; i++) place[i] = i;
  std::shuffle(place.begin(), place.end(), rng);
  S.tris.resize(n); S.flat.assign(n, 0u);
  for (uint32_t i = 0; i < ni; i++)
    for (uint32_t f = 0; f < nf[i]; f++) {
      TriRec t{}; t.instance = i; t.prim = f; t.origId = S.base[i] + f; t.vi[0] = (S.first[i] + f) % (uint32_t)S.shade.size();
      refit_flatten(S.instances[i].o2w, S.shade[t.vi[0]].p, t.v0, t.e1, t.e2);
      S.tris[place[S.first[i] + f]] = t; S.flat[t.origId] = place[S.first[i] + f];
    }
  return S;
}

// one edit: planVisibility's table for the new hidden set, the host forms, the checks.  Returns the number of problems
int edit(Scene& S, const std::vector<uint8_t>& hide, const char* what)
{
  const uint32_t ni = (uint32_t)S.nf.size(), n = (uint32_t)S.tris.size();
  std::vector<VisPatch> patch(ni);
  uint32_t visible = 0;
  for (uint32_t i = 0; i < ni; i++) {
    const uint32_t newBase = hide[i] ? S.base[i] : visible;
    if (!hide[i]) visible += S.nf[i];
    const uint32_t action = (hide[i] != 0) == (S.hidden[i] != 0) ? VIS_KEEP : (hide[i] ? VIS_HIDE : VIS_SHOW);
    patch[i] = VisPatch{(int32_t)(newBase - S.base[i]), action | (hide[i] ? VIS_HIDDEN_AFTER : 0u)};
    S.base[i] = newBase; S.hidden[i] = hide[i];
  }
  patchVisibilityTwoLevelHost(S.tris.data(), n, S.instances.data(), ni, patch.data(), S.shade.data(), (uint32_t)S.shade.size(), S.flat.data(), n);
  patchInstTravHost(S.instTrav.data(), ni, patch.data());
  std::vector<uint8_t> seen(n, 0); uint32_t counted = 0;
  int bad = (int)flatIdViolations(S.tris.data(), n, S.flat.data(), n, S.instTrav.data(), S.hidden.data(), ni, seen.data(), counted);
  if (counted != visible) bad++;
  for (uint32_t i = 0; i < n; i++) {
    const TriRec& t = S.tris[i];
    if (S.hidden[t.instance]) continue;
    TriRec w{}; refit_flatten(S.instances[t.instance].o2w, S.shade[t.vi[0]].p, w.v0, w.e1, w.e2);
    if (memcmp(w.v0, t.v0, 36) != 0 || t.origId != S.base[t.instance] + t.prim) bad++;
  }
  // the masked-box TLAS plan: exactly the visible instances are named
  std::vector<float> masked(S.boxes);
  tlasMaskHiddenBoxes(masked.data(), S.hidden.data(), ni);
  Bvh8 tlas; std::vector<uint32_t> items;
  buildBvh8Boxes(masked.data(), ni, tlas, items);
  uint32_t visibleInstances = 0;
  for (uint32_t i = 0; i < ni; i++) visibleInstances += S.hidden[i] ? 0u : 1u;
  if (tlas.activeTris != visibleInstances || items.size() != ni) bad++;
  for (uint32_t k = 0; k < (uint32_t)items.size(); k++) if (items[k] >= ni || (k < tlas.activeTris) == (S.hidden[items[k]] != 0)) bad++;
  if (bad) printf("%u instance(s), %u triangle(s), %s: %d problem(s)\n", ni, n, what, bad);
  return bad;
}

} // namespace

int main()
{
  std::mt19937 rng(1818);
  const uint32_t instanceCounts[] = {1u, 2u, 63u, 64u, 65u, 256u, 257u}, totals[] = {1u, 255u, 256u, 257u, 4097u};
  int bad = 0, cases = 0;
  for (uint32_t ni : instanceCounts)
    for (uint32_t total : totals) {
      const Scene built = build(faceCounts(ni, total, rng), rng);
      Scene S = built;
      std::vector<uint8_t> none(ni, 0), firstOnly(ni, 0), lastOnly(ni, 0), alternate(ni, 0), complement(ni, 0), allButOne(ni, 1);
      firstOnly[0] = 1; lastOnly[ni - 1] = 1; allButOne[ni / 2] = 0;
      for (uint32_t i = 0; i < ni; i++) { alternate[i] = (uint8_t)(i & 1u); complement[i] = (uint8_t)(1u - (i & 1u)); }
      bad += edit(S, firstOnly, "none -> first");
      bad += edit(S, none, "first -> none");
      bad += edit(S, lastOnly, "none -> last");
      bad += edit(S, alternate, "last -> alternate");
      bad += edit(S, complement, "alternate -> complement");
      bad += edit(S, allButOne, "complement -> all but one");
      bad += edit(S, allButOne, "all but one again");
      bad += edit(S, none, "all but one -> none");
      bad += edit(S, none, "none -> none");
      cases += 9;
      // hide and show of everything: the build's bytes again
      if (memcmp(S.tris.data(), built.tris.data(), S.tris.size() * sizeof(TriRec)) != 0 || memcmp(S.flat.data(), built.flat.data(), S.flat.size() * 4u) != 0 ||
          memcmp(S.instTrav.data(), built.instTrav.data(), S.instTrav.size() * sizeof(InstTrav)) != 0) {
        printf("%u instance(s), %u triangle(s): the arrays are not the build's after everything is shown\n", ni, total); bad++; }
    }
  if (bad) return 1;
  printf("vispatch sanitize ok (%d edits)\n", cases);
  return 0;
}

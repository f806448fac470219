// tlas_bounds_sanitize.cpp -- the bounds of a two-level scene without the flat tree (gi_tlas.h tlas_scene_bounds: what gi_build.cpp sets at the build of such a
// scene and after every edit in place of it) under AddressSanitizer + UBSan, as a program of its own:
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all -static-libasan -static-libubsan -Igatling_amd/csrc -Iinclude \
//       tests/cpp/tlas_bounds_sanitize.cpp -o tlas_bounds_sanitize && ./tlas_bounds_sanitize
// Random boxes of 1 .. 257 instances are held to a brute-force union written without the function's helpers: hidden instances masked, an inverted box among
// the others (left out, as the TLAS builder leaves it out), everything hidden (invalid), one box with a side that is not finite (invalid), no instance at all
// (invalid).  A valid answer must be the union under the pad the flat root's bounds get -- 1e-5 of magnitude and extent, plus 1e-30 -- bit for bit, and must
// contain every box it was made from.  The arrays are allocated at their exact sizes, so a read past either end is the sanitizer's to see.
// Exit status 0 and "tlas bounds sanitize ok" on success.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <random>
#include <vector>

#include "gi_tlas.h"

using namespace gi;

namespace {

// the union the function must give, the slow way: per axis the smallest low side and the largest high side over the boxes that count
bool bruteForce(const std::vector<float>& boxes, const std::vector<unsigned char>& hidden, float out[6])
{
  const size_t n = hidden.size();
  double lo[3] = {1.0e300, 1.0e300, 1.0e300}, hi[3] = {-1.0e300, -1.0e300, -1.0e300};
  size_t counted = 0;
  for (size_t i = 0; i < n; i++) {
    if (hidden[i]) continue;
    bool finite = true, inverted = false;
    for (int a = 0; a < 3; a++) {
      const float l = boxes[6 * i + a], h = boxes[6 * i + 3 + a];
      if (!std::isfinite(l) || !std::isfinite(h)) finite = false;
      else if (l > h) inverted = true;
    }
    if (!finite) return false;
    if (inverted) continue;
    for (int a = 0; a < 3; a++) { if (boxes[6 * i + a] < lo[a]) lo[a] = boxes[6 * i + a]; if (boxes[6 * i + 3 + a] > hi[a]) hi[a] = boxes[6 * i + 3 + a]; }
    counted++;
  }
  if (!counted) return false;
  for (int a = 0; a < 3; a++) {
    const float l = (float)lo[a], h = (float)hi[a]; // (exact: both are floats of the input)
    const float pad = (std::fabs(l) + std::fabs(h) + (h - l)) * 1.0e-5f + 1.0e-30f;
    out[a] = l - pad; out[3 + a] = h + pad;
  }
  return true;
}

int check(const std::vector<float>& boxes, const std::vector<unsigned char>& hidden, bool passNull, const char* what)
{
  const size_t n = hidden.size();
  float got[6] = {7.0f, 7.0f, 7.0f, 7.0f, 7.0f, 7.0f}, want[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
  bool valid = true;
  tlas_scene_bounds(boxes.data(), passNull ? nullptr : hidden.data(), n, got, valid);
  const bool wantValid = bruteForce(boxes, hidden, want);
  int bad = 0;
  if (valid != wantValid) bad++;
  if (valid && wantValid) {
    if (memcmp(got, want, sizeof(got)) != 0) bad++;
    for (size_t i = 0; i < n; i++) { // conservative: every box that counts lies inside
      if (hidden[i]) continue;
      bool inverted = false;
      for (int a = 0; a < 3; a++) inverted = inverted || boxes[6 * i + a] > boxes[6 * i + 3 + a];
      if (inverted) continue;
      for (int a = 0; a < 3; a++) if (!(got[a] <= boxes[6 * i + a]) || !(got[3 + a] >= boxes[6 * i + 3 + a])) bad++;
    }
  }
  if (bad) printf("%zu instance(s), %s: %d problem(s) (valid %d, expected %d)\n", n, what, bad, (int)valid, (int)wantValid);
  return bad;
}

} // namespace

int main()
{
  std::mt19937 rng(1919);
  std::uniform_real_distribution<float> centre(-50.0f, 50.0f), half(0.0f, 4.0f);
  const size_t counts[] = {1u, 2u, 3u, 21u, 63u, 64u, 65u, 256u, 257u};
  int bad = 0, cases = 0;
  { // no instance at all: invalid, and nothing is read
    std::vector<float> boxes; std::vector<unsigned char> hidden;
    bad += check(boxes, hidden, false, "no instance"); bad += check(boxes, hidden, true, "no instance, no table"); cases += 2;
  }
  for (const size_t n : counts)
    for (int round = 0; round < 8; round++) {
      std::vector<float> boxes(6 * n);
      for (size_t i = 0; i < n; i++) for (int a = 0; a < 3; a++) { const float c = centre(rng), h = half(rng); boxes[6 * i + a] = c - h; boxes[6 * i + 3 + a] = c + h; }
      if (round == 7) for (int a = 0; a < 3; a++) { boxes[a] = -0.0f; boxes[3 + a] = 0.0f; } // a box that is a point at the origin, with a negative zero
      std::vector<unsigned char> none(n, 0), some(n, 0), all(n, 1), onlyLast(n, 1);
      for (size_t i = 0; i < n; i++) some[i] = (unsigned char)(rng() % 3u == 0u);
      onlyLast[n - 1] = 0;
      bad += check(boxes, none, false, "nothing hidden");
      bad += check(boxes, none, true, "no table");
      bad += check(boxes, some, false, "some hidden");
      bad += check(boxes, onlyLast, false, "all but the last hidden");
      bad += check(boxes, all, false, "everything hidden");
      cases += 5;
      // an inverted box (the one an unusable instance keeps) among the others: left out; alone: invalid
      std::vector<float> withInverted(boxes);
      const size_t k = rng() % n;
      for (int a = 0; a < 3; a++) { withInverted[6 * k + a] = 3.0e38f; withInverted[6 * k + 3 + a] = -3.0e38f; }
      bad += check(withInverted, none, false, "an inverted box");
      std::vector<unsigned char> onlyK(n, 1); onlyK[k] = 0;
      bad += check(withInverted, onlyK, false, "the inverted box alone");
      // inverted on one axis only
      std::vector<float> oneAxis(boxes);
      std::swap(oneAxis[6 * k + 1], oneAxis[6 * k + 4]);
      if (oneAxis[6 * k + 1] > oneAxis[6 * k + 4]) { bad += check(oneAxis, none, false, "a box inverted on one axis"); cases++; }
      cases += 2;
      // one box with a side that is not finite: the whole answer is invalid -- unless that instance is hidden
      const float poison[] = {std::numeric_limits<float>::quiet_NaN(), std::numeric_limits<float>::infinity(), -std::numeric_limits<float>::infinity()};
      for (const float p : poison) {
        std::vector<float> nonFinite(boxes);
        nonFinite[6 * k + (rng() % 6u)] = p;
        bad += check(nonFinite, none, false, "a side that is not finite");
        std::vector<unsigned char> hideK(n, 0); hideK[k] = 1;
        bad += check(nonFinite, hideK, false, "a side that is not finite, hidden");
        cases += 2;
      }
    }
  if (bad) return 1;
  printf("tlas bounds sanitize ok (%d cases)\n", cases);
  return 0;
}

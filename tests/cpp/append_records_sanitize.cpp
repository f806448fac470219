// append_records_sanitize.cpp -- the per-item forms of a mesh appended to a two-level scene without the flat tree (gi_append.h: what gi_append.hip's kernels
// and gi_build.cpp updateTopologyTwoLevel's host copies run) under AddressSanitizer + UBSan, as a program of its own:
//   g++ -O1 -g -std=c++17 -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all -static-libasan -static-libubsan -Igatling_amd/csrc -Iinclude \
//       tests/cpp/append_records_sanitize.cpp -o append_records_sanitize && ./append_records_sanitize
// Random meshes of 1 .. 300 faces under 1 .. 37 instance transforms (mirrored ones among them), behind non-zero offsets in every array, are held to a
// restatement written without the header's helpers: the records field by field (the world-space corner as ((a*x + b*y) + c*z) + d per row, edges as
// differences, the id as base + instance x faces + face, the instance index, the word, the shading record's index and the two absolute vertex indices, the
// face), the BLAS records in a shuffled order, the shading records' index piece, the face-id words and the id table.  Every array is allocated at its exact
// size and starts as 0xa5 bytes: a read or a store past a range is the sanitizer's to see, a store outside the mesh's ranges shows as a changed byte, and the
// range predicate must refuse a mesh that does not fit.  Exit status 0 and "append records sanitize ok" on success.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "gi_append.h"

using namespace gi;

namespace {

int failures = 0;
void expect(bool ok, const char* what, unsigned a = 0, unsigned b = 0) { if (!ok) { if (failures < 20) printf("FAILED: %s (%u, %u)\n", what, a, b); failures++; } }

template <class T> std::vector<T> filled(size_t n) { std::vector<T> v(n); if (n) memset(static_cast<void*>(v.data()), 0xa5, n * sizeof(T)); return v; }

void runCase(std::mt19937& rng, uint32_t nf, uint32_t instCount, uint32_t vertexOffset, uint32_t shadeBase, uint32_t idBase, uint32_t triFirst, uint32_t instFirst,
    uint32_t blasFirst, uint32_t matFlags, bool mirrored)
{
  std::uniform_real_distribution<float> coord(-3.0f, 3.0f);
  const uint32_t nv = nf + 2u, items = nf * instCount;
  const uint32_t shadeCount = shadeBase + nf, triCount = triFirst + items, instanceCount = instFirst + instCount, flatCount = idBase + items, blasCount = blasFirst + nf;
  // the mesh: positions, faces (relative indices), AOV face ids, a shuffled BLAS order
  std::vector<float> pos(3u * nv); for (float& x : pos) x = coord(rng);
  std::vector<uint32_t> faces3(3u * (size_t)nf);
  for (uint32_t f = 0; f < nf; f++) { faces3[3 * f] = f; faces3[3 * f + 1] = (f * 7u + 1u) % nv; faces3[3 * f + 2] = (f * 13u + 2u) % nv; }
  std::vector<int32_t> faceId(nf); for (uint32_t f = 0; f < nf; f++) faceId[f] = (int32_t)(f * 3u + 1u);
  std::vector<uint32_t> order(nf); for (uint32_t f = 0; f < nf; f++) order[f] = f;
  std::shuffle(order.begin(), order.end(), rng);
  std::vector<InstanceRec> instances = filled<InstanceRec>(instanceCount);
  for (uint32_t i = 0; i < instCount; i++) {
    InstanceRec ir{};
    for (int r = 0; r < 3; r++) for (int c = 0; c < 4; c++) ir.o2w[4 * r + c] = (r == c ? 1.5f : 0.0f) + 0.3f * coord(rng);
    if (mirrored) for (int c = 0; c < 3; c++) ir.o2w[c] = -ir.o2w[c];
    ir.mesh = 2u; ir.instanceId = (int32_t)i;
    instances[instFirst + i] = ir;
  }
  // --- the shading records: the index piece by the header, the corners as the gather leaves them (positions copied bit for bit)
  std::vector<TriShade> shade = filled<TriShade>(shadeCount), shadeBefore = shade;
  appendShadeIndexHost(shade.data(), shadeCount, shadeBase, faces3.data(), nf, vertexOffset);
  for (uint32_t r = 0; r < shadeCount; r++) {
    if (r < shadeBase) { expect(memcmp(&shade[r], &shadeBefore[r], sizeof(TriShade)) == 0, "a shading record in front of the mesh changed", r); continue; }
    const uint32_t f = r - shadeBase;
    expect(memcmp(&shade[r], &shadeBefore[r], 144) == 0, "the index piece wrote outside its 16 bytes", r);
    for (int k = 0; k < 3; k++) expect(shade[r].vi[k] == vertexOffset + faces3[3 * f + k], "TriShade::vi", r, (unsigned)k);
    expect(shade[r].pad == 0u, "TriShade::pad", r);
    for (int k = 0; k < 3; k++) memcpy(shade[r].p[k], &pos[3u * faces3[3 * f + k]], 12);
  }
  // --- the BLAS records
  std::vector<BlasTri> blas = filled<BlasTri>(blasCount), blasBefore = blas;
  appendBlasTrisHost(blas.data(), blasCount, blasFirst, order.data(), nf, shade.data(), shadeCount, shadeBase);
  for (uint32_t r = 0; r < blasCount; r++) {
    if (r < blasFirst) { expect(memcmp(&blas[r], &blasBefore[r], sizeof(BlasTri)) == 0, "a BLAS record in front of the mesh changed", r); continue; }
    const uint32_t f = order[r - blasFirst];
    BlasTri want; memset(&want, 0, sizeof(want));
    memcpy(want.p0, &pos[3u * faces3[3 * f]], 12); memcpy(want.p1, &pos[3u * faces3[3 * f + 1]], 12); memcpy(want.p2, &pos[3u * faces3[3 * f + 2]], 12); want.prim = f;
    expect(memcmp(&blas[r], &want, sizeof(BlasTri)) == 0, "a BLAS record", r, f);
  }
  // --- the flat records, the face-id words, the id table: in two halves, as the host's thread pool splits the items
  AppendMesh M{}; M.triFirst = triFirst; M.faceCount = nf; M.instFirst = instFirst; M.instCount = instCount; M.shadeBase = shadeBase; M.idBase = idBase; M.matFlags = matFlags;
  M.triCount = triCount; M.instanceCount = instanceCount; M.shadeCount = shadeCount; M.flatCount = flatCount;
  expect(appendMeshRangesOk(M), "the range predicate refuses a mesh that fits");
  { AppendMesh bad = M; bad.triCount--; expect(!appendMeshRangesOk(bad), "the range predicate accepts one record too few");
    bad = M; bad.flatCount--; expect(!appendMeshRangesOk(bad), "the range predicate accepts an id table one word short");
    bad = M; bad.shadeCount--; expect(!appendMeshRangesOk(bad), "the range predicate accepts one shading record too few");
    bad = M; bad.instanceCount--; expect(!appendMeshRangesOk(bad), "the range predicate accepts one instance record too few");
    expect(!append_item_ok(M, items), "an item past the last one is accepted"); }
  std::vector<TriRec> tris = filled<TriRec>(triCount), trisBefore = tris;
  std::vector<int32_t> triFaceId = filled<int32_t>(triCount), faceIdBefore = triFaceId;
  std::vector<uint32_t> flat = filled<uint32_t>(flatCount), flatBefore = flat;
  const uint32_t half = items / 2u;
  appendRecordsHost(M, half, items, tris.data(), triFaceId.data(), flat.data(), instances.data(), shade.data(), faceId.data());
  appendRecordsHost(M, 0u, half, tris.data(), triFaceId.data(), flat.data(), instances.data(), shade.data(), faceId.data());
  appendRecordsHost(M, items, items + 64u, tris.data(), triFaceId.data(), flat.data(), instances.data(), shade.data(), faceId.data()); // (past the end: nothing)
  for (uint32_t r = 0; r < triFirst; r++)
    expect(memcmp(&tris[r], &trisBefore[r], sizeof(TriRec)) == 0 && triFaceId[r] == faceIdBefore[r], "a flat record in front of the mesh changed", r);
  for (uint32_t r = 0; r < idBase; r++) expect(flat[r] == flatBefore[r], "an id-table word in front of the mesh changed", r);
  for (uint32_t i = 0; i < instCount; i++)
    for (uint32_t f = 0; f < nf; f++) {
      const uint32_t at = triFirst + i * nf + f, id = idBase + i * nf + f;
      const float* m = instances[instFirst + i].o2w;
      float w[3][3];
      for (int k = 0; k < 3; k++) {
        const float* p = &pos[3u * faces3[3 * f + k]];
        for (int r = 0; r < 3; r++) { float acc = m[4 * r] * p[0] + m[4 * r + 1] * p[1]; acc = acc + m[4 * r + 2] * p[2]; w[k][r] = acc + m[4 * r + 3]; }
      }
      TriRec want; memset(&want, 0, sizeof(want));
      for (int a = 0; a < 3; a++) { want.v0[a] = w[0][a]; want.e1[a] = w[1][a] - w[0][a]; want.e2[a] = w[2][a] - w[0][a]; }
      want.origId = id; want.instance = instFirst + i; want.matFlags = matFlags;
      want.vi[0] = shadeBase + f; want.vi[1] = vertexOffset + faces3[3 * f + 1]; want.vi[2] = vertexOffset + faces3[3 * f + 2]; want.prim = f;
      expect(memcmp(&tris[at], &want, sizeof(TriRec)) == 0, "a flat record", i, f);
      expect(triFaceId[at] == faceId[f], "a face-id word", i, f);
      expect(flat[id] == at, "an id-table word", i, f);
    }
}

} // namespace

int main()
{
  std::mt19937 rng(20);
  const uint32_t shapes[][2] = {{1, 1}, {15, 1}, {16, 1}, {17, 1}, {63, 1}, {64, 1}, {65, 1}, {255, 1}, {256, 1}, {257, 1}, {7, 37}, {300, 3}};
  for (const auto& s : shapes) {
    runCase(rng, s[0], s[1], 0u, 0u, 0u, 0u, 0u, 0u, 0u, false);
    runCase(rng, s[0], s[1], 3u, 5u, 1000u, 7u, 5u, 3u, 0xc1000006u, true);
  }
  if (failures) { printf("%d check(s) failed\n", failures); return 1; }
  printf("append records sanitize ok\n");
  return 0;
}

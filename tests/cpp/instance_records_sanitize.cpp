// instance_records_sanitize.cpp -- the per-item forms of new instances of built meshes on a two-level scene without the flat tree (gi_instances.h: what
// gi_instances.hip's kernel and gi_build.cpp updateInstancesTwoLevel's host copies run) under AddressSanitizer + UBSan, as a program of its own:
//   g++ -O1 -g -std=c++17 -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all -static-libasan -static-libubsan -Igatling_amd/csrc -Iinclude \
//       tests/cpp/instance_records_sanitize.cpp -o instance_records_sanitize && ./instance_records_sanitize
// Job lists -- one job per new instance; faces per job 1, 15 .. 17, 63 .. 65, 255 .. 257, 37 jobs of 7 faces of one mesh, a mixed launch of 1, 17, 64, 65 and
// 300 faces with two meshes named twice, and that list with its slots in descending storage order with gaps -- are held to a restatement written without the
// header's helpers: the records field by field (the world-space corner as ((a*x + b*y) + c*z) + d per row, edges as differences, the id as base + face, the
// instance slot, the word, the shading record's index and the two absolute vertex indices, the face), the face-id words and the id table.  Every array is
// allocated at its exact size and starts as 0xa5 bytes: a read or a store past a range is the sanitizer's to see, a store outside the jobs' ranges shows as
// a changed byte, and the range check must refuse a job that does not fit, a prefix that is not the job sizes' and 2^28 items.  Exit status 0 and "instance
// records sanitize ok" on success.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "gi_instances.h"

using namespace gi;

namespace {

int failures = 0;
void expect(bool ok, const char* what, unsigned a = 0, unsigned b = 0) { if (!ok) { if (failures < 20) printf("FAILED: %s (%u, %u)\n", what, a, b); failures++; } }

template <class T> std::vector<T> filled(size_t n) { std::vector<T> v(n); if (n) memset(static_cast<void*>(v.data()), 0xa5, n * sizeof(T)); return v; }

struct Mesh { uint32_t nf, vertexOffset, shadeBase, faceIdFirst, matFlags; std::vector<float> pos; std::vector<uint32_t> faces3; };

// jobMesh[k]: the mesh of job k (faces[m]: faces of mesh m).  descending: storage slots handed out from the top down, with gaps between the ranges
void runCase(std::mt19937& rng, const std::vector<uint32_t>& faces, const std::vector<uint32_t>& jobMesh, bool descending, bool mirrored)
{
  std::uniform_real_distribution<float> coord(-3.0f, 3.0f);
  // --- the meshes, one behind the other in the per-face arrays
  std::vector<Mesh> meshes;
  uint32_t vertexOffset = 3u, shadeCount = 5u, faceIdCount = 2u;
  for (size_t m = 0; m < faces.size(); m++) {
    Mesh M; M.nf = faces[m]; M.vertexOffset = vertexOffset; M.shadeBase = shadeCount; M.faceIdFirst = faceIdCount; M.matFlags = 0xc1000006u + (uint32_t)m;
    const uint32_t nv = M.nf + 2u;
    M.pos.resize(3u * nv); for (float& x : M.pos) x = coord(rng);
    M.faces3.resize(3u * (size_t)M.nf);
    for (uint32_t f = 0; f < M.nf; f++) { M.faces3[3 * f] = f; M.faces3[3 * f + 1] = (f * 7u + 1u) % nv; M.faces3[3 * f + 2] = (f * 13u + 2u) % nv; }
    vertexOffset += nv; shadeCount += M.nf; faceIdCount += M.nf;
    meshes.push_back(M);
  }
  std::vector<TriShade> shade = filled<TriShade>(shadeCount); std::vector<int32_t> faceIdTable = filled<int32_t>(faceIdCount);
  for (const Mesh& M : meshes) for (uint32_t f = 0; f < M.nf; f++) {
    TriShade& q = shade[M.shadeBase + f];
    for (int k = 0; k < 3; k++) { memcpy(q.p[k], &M.pos[3u * M.faces3[3 * f + k]], 12); q.vi[k] = M.vertexOffset + M.faces3[3 * f + k]; }
    faceIdTable[M.faceIdFirst + f] = (int32_t)(f * 3u + 1u + M.shadeBase);
  }
  // --- the jobs: record ranges and instance slots in ascending or descending storage order, ids in job order
  const uint32_t jobCount = (uint32_t)jobMesh.size(), gap = descending ? 3u : 0u;
  uint32_t records = 7u, items = 0;
  for (uint32_t k = 0; k < jobCount; k++) { records += meshes[jobMesh[k]].nf + gap; items += meshes[jobMesh[k]].nf; }
  const uint32_t triCount = records + 2u, instanceCount = 5u + 2u * jobCount + 1u, idFirst = descending ? 1000u : 0u, flatCount = idFirst + items + 3u;
  std::vector<InstanceJob> jobs(jobCount);
  std::vector<InstanceRec> instances = filled<InstanceRec>(instanceCount);
  {
    uint32_t up = 7u, down = records, id = idFirst;
    for (uint32_t k = 0; k < jobCount; k++) {
      const Mesh& M = meshes[jobMesh[k]];
      InstanceJob& j = jobs[k];
      if (descending) { down -= M.nf + gap; j.triFirst = down + gap; j.instance = 5u + 2u * (jobCount - 1u - k); } else { j.triFirst = up; up += M.nf; j.instance = 5u + k; }
      j.idBase = id; id += M.nf; j.shadeBase = M.shadeBase; j.faceCount = M.nf; j.matFlags = M.matFlags; j.faceIdFirst = M.faceIdFirst; j.wgFirst = 0xdeadu;
      InstanceRec ir{};
      for (int r = 0; r < 3; r++) for (int c = 0; c < 4; c++) ir.o2w[4 * r + c] = (r == c ? 1.5f : 0.0f) + 0.3f * coord(rng);
      if (mirrored) for (int c = 0; c < 3; c++) ir.o2w[c] = -ir.o2w[c];
      ir.mesh = jobMesh[k]; ir.instanceId = (int32_t)k;
      instances[j.instance] = ir;
    }
  }
  InstanceJobSizes Z{}; Z.jobCount = jobCount; Z.triCount = triCount; Z.instanceCount = instanceCount; Z.shadeCount = shadeCount; Z.flatCount = flatCount;
  Z.faceIdCount = faceIdCount;
  expect(!instanceJobsOk(jobs.data(), Z), "the range check accepts a prefix that was never made");
  Z.wgCount = instanceJobsNumber(jobs.data(), jobCount);
  uint32_t wantWg = 0;
  for (uint32_t k = 0; k < jobCount; k++) { expect(jobs[k].wgFirst == wantWg, "the workgroup prefix", k); wantWg += (4u * jobs[k].faceCount + 255u) / 256u; }
  expect(Z.wgCount == wantWg && wantWg != 0u, "the launch's workgroups");
  expect(instanceJobsOk(jobs.data(), Z), "the range check refuses jobs that fit");
  for (uint32_t wg = 0; wg < Z.wgCount; wg++) { // the search: the last job that starts at or in front of the workgroup
    uint32_t want = 0; for (uint32_t k = 0; k < jobCount; k++) if (jobs[k].wgFirst <= wg) want = k;
    expect(instance_job_of(jobs.data(), jobCount, wg) == want, "the job of a workgroup", wg, want);
  }
  { // the refusals
    uint32_t top = 0, topId = 0, topInst = 0, lastMesh = 0;
    for (uint32_t k = 0; k < jobCount; k++) { if (jobs[k].triFirst > jobs[top].triFirst) top = k; if (jobs[k].idBase > jobs[topId].idBase) topId = k;
        if (jobs[k].instance > jobs[topInst].instance) topInst = k; if (jobs[k].shadeBase > jobs[lastMesh].shadeBase) lastMesh = k; }
    InstanceJobSizes bad = Z; bad.triCount = jobs[top].triFirst + jobs[top].faceCount - 1u; expect(!instanceJobsOk(jobs.data(), bad), "the range check accepts one record too few");
    bad = Z; bad.flatCount = jobs[topId].idBase + jobs[topId].faceCount - 1u; expect(!instanceJobsOk(jobs.data(), bad), "the range check accepts an id table one word short");
    bad = Z; bad.shadeCount--; expect(!instanceJobsOk(jobs.data(), bad), "the range check accepts one shading record too few");
    bad = Z; bad.faceIdCount--; expect(!instanceJobsOk(jobs.data(), bad), "the range check accepts a face-id table one word short");
    bad = Z; bad.instanceCount = jobs[topInst].instance; expect(!instanceJobsOk(jobs.data(), bad), "the range check accepts one instance record too few");
    bad = Z; bad.wgCount++; expect(!instanceJobsOk(jobs.data(), bad), "the range check accepts a workgroup too many");
    std::vector<InstanceJob> shifted(jobs); shifted.back().wgFirst++; expect(jobCount == 1u || !instanceJobsOk(shifted.data(), Z), "the range check accepts a prefix that is not the job sizes'");
    std::vector<InstanceJob> huge(2, jobs[0]); huge[0].faceCount = huge[1].faceCount = 1u << 27;
    expect(instanceJobsNumber(huge.data(), 2u) == 0u, "2^28 items are numbered");
    (void)lastMesh;
  }
  // --- the kernel's host form: in two halves, as the host's thread pool splits the workgroups, and past the end
  std::vector<TriRec> tris = filled<TriRec>(triCount), trisBefore = tris;
  std::vector<int32_t> triFaceId = filled<int32_t>(triCount), faceIdBefore = triFaceId;
  std::vector<uint32_t> flat = filled<uint32_t>(flatCount), flatBefore = flat;
  const uint32_t half = Z.wgCount / 2u;
  instanceRecordsHost(jobs.data(), Z, half, Z.wgCount, tris.data(), triFaceId.data(), flat.data(), instances.data(), shade.data(), faceIdTable.data());
  instanceRecordsHost(jobs.data(), Z, 0u, half, tris.data(), triFaceId.data(), flat.data(), instances.data(), shade.data(), faceIdTable.data());
  instanceRecordsHost(jobs.data(), Z, Z.wgCount, Z.wgCount + 3u, tris.data(), triFaceId.data(), flat.data(), instances.data(), shade.data(), faceIdTable.data()); // (nothing)
  std::vector<uint8_t> recOwned(triCount, 0), idOwned(flatCount, 0);
  for (uint32_t k = 0; k < jobCount; k++) {
    const InstanceJob& j = jobs[k];
    const Mesh& M = meshes[jobMesh[k]];
    const float* m = instances[j.instance].o2w;
    for (uint32_t f = 0; f < M.nf; f++) {
      const uint32_t at = j.triFirst + f, id = j.idBase + f;
      recOwned[at] = 1; idOwned[id] = 1;
      float w[3][3];
      for (int c = 0; c < 3; c++) {
        const float* p = &M.pos[3u * M.faces3[3 * f + c]];
        for (int r = 0; r < 3; r++) { float acc = m[4 * r] * p[0] + m[4 * r + 1] * p[1]; acc = acc + m[4 * r + 2] * p[2]; w[c][r] = acc + m[4 * r + 3]; }
      }
      TriRec want; memset(&want, 0, sizeof(want));
      for (int a = 0; a < 3; a++) { want.v0[a] = w[0][a]; want.e1[a] = w[1][a] - w[0][a]; want.e2[a] = w[2][a] - w[0][a]; }
      want.origId = id; want.instance = j.instance; want.matFlags = M.matFlags;
      want.vi[0] = M.shadeBase + f; want.vi[1] = M.vertexOffset + M.faces3[3 * f + 1]; want.vi[2] = M.vertexOffset + M.faces3[3 * f + 2]; want.prim = f;
      expect(memcmp(&tris[at], &want, sizeof(TriRec)) == 0, "a flat record", k, f);
      expect(triFaceId[at] == faceIdTable[M.faceIdFirst + f], "a face-id word", k, f);
      expect(flat[id] == at, "an id-table word", k, f);
    }
  }
  for (uint32_t r = 0; r < triCount; r++)
    if (!recOwned[r]) expect(memcmp(&tris[r], &trisBefore[r], sizeof(TriRec)) == 0 && triFaceId[r] == faceIdBefore[r], "a flat record outside every job's range changed", r);
  for (uint32_t r = 0; r < flatCount; r++) if (!idOwned[r]) expect(flat[r] == flatBefore[r], "an id-table word outside every job's range changed", r);
}

} // namespace

int main()
{
  std::mt19937 rng(21);
  for (const uint32_t nf : {1u, 15u, 16u, 17u, 63u, 64u, 65u, 255u, 256u, 257u}) { runCase(rng, {nf}, {0u}, false, false); runCase(rng, {nf}, {0u}, true, true); }
  runCase(rng, {7u}, std::vector<uint32_t>(37, 0u), false, false);
  runCase(rng, {7u}, std::vector<uint32_t>(37, 0u), true, true);
  const std::vector<uint32_t> mixed{1u, 17u, 64u, 65u, 300u};
  runCase(rng, mixed, {0u, 1u, 2u, 3u, 4u}, false, false);
  runCase(rng, mixed, {0u, 1u, 2u, 3u, 4u, 1u, 4u}, false, true);
  runCase(rng, mixed, {0u, 1u, 2u, 3u, 4u}, true, false);
  runCase(rng, mixed, {4u, 1u, 0u, 3u, 2u, 1u, 4u}, true, true);
  if (failures) { printf("%d check(s) failed\n", failures); return 1; }
  printf("instance records sanitize ok\n");
  return 0;
}

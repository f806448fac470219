// gather_sanitize.cpp -- the gather of shading records a vertex update runs (gi_refit.h refit_gather_shade, what gi_refit.hip k_gather_shade runs per word)
// against the packers of the scene build (gi_pack.h packVertex, packTriShade) under AddressSanitizer + UBSan, as a program of its own:
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all -static-libasan -static-libubsan -Igatling_amd/csrc -Iinclude \
//       tests/cpp/gather_sanitize.cpp -o gather_sanitize && ./gather_sanitize
// Random indexed meshes of several sizes behind a vertex offset, with hostile shading attributes, zero-length normals and faces that repeat a vertex: every
// gathered record must equal the packed one byte for byte, a record with a corner outside the vertex array must stay as it was, and the arrays are sized
// exactly so that a read or a store past either end is the sanitizer's finding.  Exit status 0 and "gather sanitize ok" on success.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "gi_pack.h"
#include "gi_refit.h"

using namespace gi;

int main()
{
  std::mt19937 rng(1234);
  std::uniform_real_distribution<float> U(-3.0f, 3.0f);
  int bad = 0; size_t records = 0;
  for (uint32_t nv : {3u, 7u, 157u, 4099u}) {
    for (uint32_t vertexOffset : {0u, 5u}) {
      std::vector<GiCVertex> v(nv);
      for (GiCVertex& x : v) {
        for (int a = 0; a < 3; a++) { x.pos[a] = U(rng); x.norm[a] = U(rng); x.tangent[a] = U(rng); }
        x.u = U(rng); x.v = U(rng); x.bitangentSign = (rng() & 1u) ? 1.0f : -1.0f;
      }
      v[0].norm[1] = NAN; v[1].tangent[2] = INFINITY; v[2].u = NAN; v[2].v = -INFINITY; v[2].bitangentSign = -INFINITY; v[0].pos[0] = NAN;
      v[nv - 1].norm[0] = v[nv - 1].norm[1] = v[nv - 1].norm[2] = 0.0f;
      std::vector<GiCFace> faces(nv * 3u + 1u);
      for (GiCFace& f : faces) for (int k = 0; k < 3; k++) f.v_i[k] = rng() % nv;
      faces[0].v_i[0] = faces[0].v_i[1] = faces[0].v_i[2] = nv - 1u; // one vertex three times, the last of the array
      std::vector<FVertex> verts(vertexOffset + (size_t)nv); // exactly the vertices: nothing behind the last one
      for (uint32_t i = 0; i < vertexOffset; i++) memset(&verts[i], 0x5a, sizeof(FVertex));
      for (uint32_t i = 0; i < nv; i++) verts[vertexOffset + i] = packVertex(v[i]);
      std::vector<TriShade> gathered(faces.size());
      for (size_t f = 0; f < faces.size(); f++) {
        const TriShade packed = packTriShade(v.data(), faces[f], vertexOffset);
        memset(&gathered[f], 0xa5, sizeof(TriShade)); // (every gathered word must be written)
        for (int k = 0; k < 3; k++) gathered[f].vi[k] = packed.vi[k];
        gathered[f].pad = packed.pad;
        refit_gather_shade(verts.data(), (uint32_t)verts.size(), gathered[f]);
        if (memcmp(&gathered[f], &packed, sizeof(TriShade)) != 0) bad++;
        records++;
      }
      // a corner outside the array: the record is left as it is
      TriShade q; memset(&q, 0xa5, sizeof(q)); q.vi[0] = 0u; q.vi[1] = (uint32_t)verts.size(); q.vi[2] = 1u;
      const TriShade before = q;
      refit_gather_shade(verts.data(), (uint32_t)verts.size(), q);
      if (memcmp(&q, &before, sizeof(TriShade)) != 0) bad++;
    }
  }
  // the word map: every word below kShadeGatherWords names one corner and one FVertex word, and together they cover p, n, t, uv and bsign once
  {
    FVertex three[3]; uint32_t tag = 0;
    for (FVertex& fv : three) { uint32_t w[12]; for (uint32_t& x : w) x = tag++; memcpy(&fv, w, sizeof(fv)); }
    const uint32_t vi[3] = {0u, 1u, 2u};
    std::vector<int> seen(36, 0);
    for (uint32_t w = 0; w < kShadeGatherWords; w++) { const uint32_t x = refit_shade_word(three, vi, w); if (x >= 36u || seen[x]++) bad++; }
  }
  if (bad) { printf("gather sanitize FAILED: %d\n", bad); return 1; }
  printf("gather sanitize ok: %zu records\n", records);
  return 0;
}

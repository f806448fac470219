// gi_pack.h -- host packing of mesh vertices into the records the kernels read (Gi.cpp:848-861): the octahedral encode / decode of directions, the
// sanitising of hostile shading attributes, the FVertex of a vertex and the TriShade of a face.  Host only and free of the HIP runtime, so that the
// stand-alone sanitizer program (tests/cpp/gather_sanitize.cpp) compiles the code the library runs; gi_host.h includes it for every host unit.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>

#pragma GCC visibility push(default)
#include "../../include/gi_c.h"
#pragma GCC visibility pop
#include "gi_types.h"

// _EncodeDirection, Gi.cpp:287-300 (glm::packUnorm2x16 rounds)
inline uint32_t encodeDirection(const float* vin)
{
  float x = vin[0], y = vin[1], z = vin[2];
  float inv = 1.0f / sqrtf((x * x + y * y) + z * z);
  x *= inv; y *= inv; z *= inv;
  float s = fabsf(x) + fabsf(y) + fabsf(z);
  x /= s; y /= s; z /= s;
  float px = x >= 0.0f ? 1.0f : -1.0f, py = y >= 0.0f ? 1.0f : -1.0f, ex, ey;
  if (z < 0.0f) { ex = (1.0f - fabsf(y)) * px; ey = (1.0f - fabsf(x)) * py; } else { ex = x; ey = y; }
  ex = ex * 0.5f + 0.5f; ey = ey * 0.5f + 0.5f;
  ex = std::min(std::max(ex, 0.0f), 1.0f); ey = std::min(std::max(ey, 0.0f), 1.0f);
  return (uint32_t)nearbyintf(ex * 65535.0f) | ((uint32_t)nearbyintf(ey * 65535.0f) << 16);
}

// decode_direction (common.glsl:198-207) evaluated once per vertex on the host, operation for operation what
// gi_decode_direction / the oracle execute (IEEE fp32, no contraction), so results stay bit-identical.
inline void decodeDirection(uint32_t e, float out[3])
{
  float ex = (float)(e & 0xffffu) / 65535.0f, ey = (float)(e >> 16) / 65535.0f;
  ex = ex * 2.0f - 1.0f; ey = ey * 2.0f - 1.0f;
  float x = ex, y = ey, z = 1.0f - fabsf(ex) - fabsf(ey);
  float t = (-z > 0.0f) ? -z : 0.0f;
  x += (x >= 0.0f) ? -t : t;
  y += (y >= 0.0f) ? -t : t;
  float inv = 1.0f / sqrtf((x * x + y * y) + z * z);
  out[0] = x * inv; out[1] = y * inv; out[2] = z * inv;
}

// Shading attributes of a vertex as the scene build takes them: a normal or tangent with a non-finite component becomes +Z, a non-finite texture coordinate 0,
// a non-finite bitangent sign +1 (the position is left alone: it decides whether the triangle is active). The reference uploads what it is given
// (Gi.cpp:848-861) and a NaN attribute is a NaN pixel there; here hostile attributes cost the shading of the faces that use them, nothing else.
inline GiCVertex usableShadingAttributes(const GiCVertex& in)
{
  GiCVertex v = in;
  auto direction = [](float* d) { if (!std::isfinite(d[0]) || !std::isfinite(d[1]) || !std::isfinite(d[2])) { d[0] = 0.0f; d[1] = 0.0f; d[2] = 1.0f; } };
  direction(v.norm); direction(v.tangent);
  if (!std::isfinite(v.u)) v.u = 0.0f;
  if (!std::isfinite(v.v)) v.v = 0.0f;
  if (!std::isfinite(v.bitangentSign)) v.bitangentSign = 1.0f;
  return v;
}
// The FVertex of one mesh vertex (Gi.cpp:848-861: normal and tangent quantised to octahedral unorm2x16, then decoded once) and the TriShade record of one mesh
// face (`vertices`: the mesh's): buildScene, buildShadeRecords, updateTopology's append and (packVertex) updateVertices -- the one copy of this code
inline gi::FVertex packVertex(const GiCVertex& vIn)
{
  const GiCVertex v = usableShadingAttributes(vIn);
  gi::FVertex fv; memcpy(fv.pos, v.pos, 12); fv.bsign = v.bitangentSign;
  decodeDirection(encodeDirection(v.norm), fv.normal); decodeDirection(encodeDirection(v.tangent), fv.tangent);
  fv.u = v.u; fv.v = v.v;
  return fv;
}
inline gi::TriShade packTriShade(const GiCVertex* vertices, const GiCFace& f, uint32_t vertexOffset)
{
  gi::TriShade q{};
  for (int k = 0; k < 3; k++) {
    const GiCVertex v = usableShadingAttributes(vertices[f.v_i[k]]);
    // (Gi.cpp:848-861: quantised, then decoded once)
    memcpy(q.p[k], v.pos, 12); decodeDirection(encodeDirection(v.norm), q.n[k]); decodeDirection(encodeDirection(v.tangent), q.t[k]);
    q.uv[k][0] = v.u; q.uv[k][1] = v.v; q.bsign[k] = v.bitangentSign; q.vi[k] = vertexOffset + f.v_i[k];
  }
  return q;
}

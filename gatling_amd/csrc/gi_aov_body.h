// gi_aov_body.h -- what the two AOV kernels share (gi_aov.hip k_aov: per-lane walk of the flat tree; gi_aov2.hip k_aov2: wave-cooperative walk of the TLAS
// and the BLASes): a pixel's prologue (clear values, the running Normal / Albedo of a progressive call), the body that turns ONE primary hit into AOV values,
// and the epilogue.  The kernels differ in how they find the hit and in nothing else, so the values are the same bits whichever kernel wrote them.
// Restates what the reference's ray generation and closest-hit shaders write for the primary hit (rp_main.rgen:132-183, 517-520;
// rp_main.chit:192-290).  Included by gi_aov.hip and gi_aov2.hip, after gi_shading.h and gi_stages.h.
#pragma once

namespace gi {

__device__ inline V3 bsdf_albedo(const MaterialRec* m, const ShState& st, V3 k1)
{
  float nk1 = fmax2(dot(st.normal, k1), 1e-4f);
  if (m->klass == 0u) return diffuse_class_color(m, st);
  if (m->klass == 1u) {
    UpsParams u = ups_params(m, st);
    float Fc = u.coat * (0.04f + 0.96f * schlick_w(nk1));
    V3 Fs = schlick3(u.F0, nk1);
    V3 diffuse = (u.albedo * (v3(1.0f, 1.0f, 1.0f) - Fs)) * (1.0f - Fc);
    V3 glossy = v3(Fc, Fc, Fc) + Fs * (1.0f - Fc);
    return diffuse + glossy;
  }
  OpbrParams o = opbr_params(m, st);
  float eta = relative_eta(st, o.eta);
  const float nk1c = st.hasCoatFrame ? fmax2(dot(st.coatNormal, k1), 1e-4f) : nk1; // the coat's Fresnel term in its own frame (geometry_coat_normal)
  float Fc = o.coat * (o.coatF0 + (1.0f - o.coatF0) * schlick_w(nk1c));
  float Fd = fresnel_dielectric(nk1, eta);
  float base = 1.0f - Fc, diel = 1.0f - o.metalness;
  V3 diffuse = (o.albedo * o.coatTint) * (base * diel * (1.0f - Fd) * (1.0f - o.tw));
  V3 glossy = v3(Fc, Fc, Fc) + ((schlick_f82(o.albedo, o.metalTint, nk1) * o.specWeight) * o.coatTint) * (base * o.metalness)
              + (o.specColor * o.coatTint) * (base * diel * Fd);
  if (o.filmWeight > 0.0f) { // thin film: the two Fresnel factors carry the film's reflectance, what lies beneath the interface its complement
    const V3 Fdf = opbr_film_dielectric(o, nk1, eta, Fd);
    diffuse = ((o.albedo * o.coatTint) * (v3(1.0f, 1.0f, 1.0f) - Fdf)) * (base * diel * (1.0f - o.tw));
    glossy = v3(Fc, Fc, Fc) + ((opbr_film_metal(o, nk1, schlick_f82(o.albedo, o.metalTint, nk1)) * o.specWeight) * o.coatTint) * (base * o.metalness)
             + ((o.specColor * o.coatTint) * Fdf) * (base * diel);
  }
  if (o.fuzzWeight > 0.0f) { // the fuzz layer keeps P = fuzz_weight * min(E, 1) of the light (tinted), what is beneath gets 1 - P
    const float Pf = o.fuzzWeight * fmin2(fuzz_albedo(nk1, o.fuzzAlpha), 1.0f);
    return (diffuse + glossy) * (1.0f - Pf) + o.fuzzColor * Pf;
  }
  return diffuse + glossy;
}

// what a lane keeps of its pixel across the samples
struct AovPixel { uint32_t pixelIndex; V3 curNormal, curAlbedo; bool blend; };

__device__ __forceinline__ void aov_put3(F4* buf, uint32_t pixelIndex, V3 v)
{
  if (buf) { float* d = reinterpret_cast<float*>(&buf[pixelIndex]); d[0] = v.x; d[1] = v.y; d[2] = v.z; }
}

// the pixel before its first sample: every bound AOV gets its clear value; Normal and Albedo start from it, or -- a progressive call behind others -- from
// what the calls before left
__device__ __forceinline__ void aov_pixel_begin(const FrameUniforms& U, const AovTargets& A, uint32_t pixelIndex, AovPixel& P)
{
  P.pixelIndex = pixelIndex;
  auto clr3 = [&](F4* buf, int id) { aov_put3(buf, pixelIndex, v3(A.clear[id][0], A.clear[id][1], A.clear[id][2])); };
  clr3(A.barycentrics, 3); clr3(A.texcoords, 4); clr3(A.opacity, 7); clr3(A.tangents, 8); clr3(A.bitangents, 9); clr3(A.thinWalled, 10);
  if (A.objectId) A.objectId[pixelIndex] = (int)f2u(A.clear[11][0]);
  if (A.depth) A.depth[pixelIndex] = A.clear[12][0];
  if (A.faceId) A.faceId[pixelIndex] = (int)f2u(A.clear[13][0]);
  if (A.instanceId) A.instanceId[pixelIndex] = (int)f2u(A.clear[14][0]);
  clr3(A.doubleSided, 15);
  P.curNormal = v3(0.0f, 0.0f, 0.0f); P.curAlbedo = P.curNormal;
  if (U.sampleOffset == 0u) { clr3(A.normal, 1); clr3(A.albedo, 16); P.curNormal = v3(A.clear[1][0], A.clear[1][1], A.clear[1][2]);
      P.curAlbedo = v3(A.clear[16][0], A.clear[16][1], A.clear[16][2]); }
  else {
    if (A.normal) { const F4 q = ld4(&A.normal[pixelIndex]); P.curNormal = v3(q.x, q.y, q.z); }
    if (A.albedo) { const F4 q = ld4(&A.albedo[pixelIndex]); P.curAlbedo = v3(q.x, q.y, q.z); }
  }
  P.blend = (U.flags & FLAG_PROGRESSIVE) && U.sampleOffset > 0u;
}

// one sample's primary hit: triangle `tri` (index of its flat record) at (t, u, v) along `dir`; matWord is that record's material word (TriRec::matFlags)
template <bool PACKED>
__device__ __forceinline__ void aov_hit(const FrameUniforms& U, const SceneView& sc, const AovTargets& A, AovPixel& P, V3 dir, float t, float u, float v,
                                        uint32_t tri, uint32_t matWord)
{
  const uint32_t pixelIndex = P.pixelIndex;
  auto put3 = [&](F4* buf, V3 val) { aov_put3(buf, pixelIndex, val); };
  ShState ss;
  setup_shading_state<PACKED>(sc, tri, u, v, dir, ss);
  const uint4* tp = reinterpret_cast<const uint4*>(sc.tris) + (size_t)tri * 4u;
  const uint32_t instIdx = tp[2].z;
  if (A.opacity) {
    // rp_main.chit:199-205 writes (1,0,0) for materials without cutout transparency; for the others the any-hit shader has written
    // viridis(opacity) (white for 0) of its last candidate (rp_main.ahit:45-49) -- restated as the ACCEPTED primary hit's opacity
    V3 c = v3(1.0f, 0.0f, 0.0f);
    if (matWord & (1u << 28)) { const float op = cutout_opacity_at(sc, matWord, tri, u, v); c = (op == 0.0f) ? v3(1.0f, 1.0f, 1.0f) : gi_colormap_viridis(op);
        }
    put3(A.opacity, c);
  }
  put3(A.tangents, (ss.tangentU + v3(1.0f, 1.0f, 1.0f)) * 0.5f);
  put3(A.bitangents, (ss.tangentV + v3(1.0f, 1.0f, 1.0f)) * 0.5f);
  put3(A.barycentrics, v3(1.0f - u - v, u, v));
  if (A.texcoords) {
    const uint4 td = tp[3];
    const float bx = 1.0f - u - v;
    if (PACKED) { const TriShade& q = sc.triShade[td.x];
        put3(A.texcoords, v3((bx * q.uv[0][0] + u * q.uv[1][0]) + v * q.uv[2][0], (bx * q.uv[0][1] + u * q.uv[1][1]) + v * q.uv[2][1], 0.0f)); }
    else {
    const FVertex* va = &sc.verts[td.x]; const FVertex* vb = &sc.verts[td.y]; const FVertex* vc = &sc.verts[td.z];
    put3(A.texcoords, v3((bx * va->u + u * vb->u) + v * vc->u, (bx * va->v + u * vb->v) + v * vc->v, 0.0f));
    }
  }
  // rp_main.chit:218-220
  { const MaterialRec* tm = &sc.materials[ss.material];
      put3(A.thinWalled, (tm->klass == 2u && ((uint32_t)tm->p[MP_FEATURES] & MATF_THIN_WALLED) != 0u) ? v3(1.0f, 0.0f, 0.0f) : v3(0.0f, 1.0f, 0.0f)); }
  if (A.objectId) A.objectId[pixelIndex] = (int)sc.instances[instIdx].pad;
  if (A.depth) A.depth[pixelIndex] = 2.0f * gi_logf(t / U.clipNear) / gi_logf(U.clipFar / U.clipNear) - 1.0f;
  if (A.faceId) A.faceId[pixelIndex] = sc.triFaceId[tri];
  if (A.instanceId) A.instanceId[pixelIndex] = sc.instances[instIdx].instanceId;
  put3(A.doubleSided, (ss.meshFlags & 2u) ? v3(0.0f, 1.0f, 0.0f) : v3(1.0f, 0.0f, 0.0f));
  if (A.normal) {
    const V3 pos = (ss.normal + v3(1.0f, 1.0f, 1.0f)) * 0.5f;
    const V3 prev = P.blend ? P.curNormal : pos;
    P.curNormal = (prev * U.sampleOffsetF + pos * U.sppF) * U.invTotalSampleCount;
  }
  if (A.albedo) {
    const MaterialRec* am = &sc.materials[ss.material];
    if (am->flags & MAT_FLAG_TEXTURED) resolve_material_textures(sc, am, dir, ss);
    const V3 al = bsdf_albedo(am, ss, -dir);
    const V3 prev = P.blend ? P.curAlbedo : al;
    P.curAlbedo = (prev * U.sampleOffsetF + al * U.sppF) * U.invTotalSampleCount;
  }
}

// the pixel behind its last sample
__device__ __forceinline__ void aov_pixel_end(const AovTargets& A, const AovPixel& P)
{
  aov_put3(A.albedo, P.pixelIndex, P.curAlbedo);
  if (A.normal) { // rp_main.rgen:517-520
    const V3 n = P.curNormal * 2.0f - v3(1.0f, 1.0f, 1.0f);
    aov_put3(A.normal, P.pixelIndex, (normalize(n) + v3(1.0f, 1.0f, 1.0f)) * 0.5f);
  }
}

} // namespace gi

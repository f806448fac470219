// gi_build.cpp -- scene build (flatten, pack, BVH8, two-level layout, upload) and incremental transform updates (Gi.cpp:784-1315)
// (one of the translation units gi_c.cpp was split into in round 6; shared declarations: gi_host.h)
#include "gi_host.h"
#include "gi_bvh_build.h"
#include "gi_refit.h"
#include "gi_tlas.h"
#include "gi_blas.h"
#include "gi_blas_build.h"
#include "gi_pack.h"
#include "gi_vispatch.h"
#include "gi_append.h"
#include "gi_instances.h"
#include "gi_compact.h"

#include <random>
#include <unordered_map>
constexpr uint32_t kIncrementalMinTris = 4096; // scenes with fewer triangles are not edited in place: they rebuild in no time (and must stay LDS-resident)
// levels of a scene BVH: the deepest traversal variant keeps 16 stack entries in LDS and OVF_STACK = 40 in scratch; trav_node_pick does not bound-check the
// spill.  The limit stays at 1 + 8 + 40 levels, the depth the 8-entry spilling variant of earlier versions could hold
constexpr uint32_t kMaxBvhDepth = 1u + 8u + 40u;

// ---------------------------------------------------------------------------------------------------------------
// scene build: flatten instances into world space, pack vertex data, build + upload the BVH8
// ---------------------------------------------------------------------------------------------------------------

// world = local * M_prim * M_instance with USD row vectors (Gi.cpp:641-658, 1191); returns rows of the 3x4
// column-vector affine.  Same operation order as glm's mat4 * mat4.
void composeTransform(const float* prim, const float* inst, float out[12])
{
  for (int c = 0; c < 3; c++)
    for (int r = 0; r < 4; r++) {
      float acc = prim[r * 4 + 0] * inst[0 * 4 + c];
      acc = acc + prim[r * 4 + 1] * inst[1 * 4 + c];
      acc = acc + prim[r * 4 + 2] * inst[2 * 4 + c];
      acc = acc + prim[r * 4 + 3] * inst[3 * 4 + c];
      out[c * 4 + r] = acc;
    }
}

void invert3x3(const float a[12], float inv[9])
{
  double m[3][3] = {{a[0], a[1], a[2]}, {a[4], a[5], a[6]}, {a[8], a[9], a[10]}};
  double c00 = m[1][1] * m[2][2] - m[1][2] * m[2][1];
  double c01 = m[1][2] * m[2][0] - m[1][0] * m[2][2];
  double c02 = m[1][0] * m[2][1] - m[1][1] * m[2][0];
  double det = m[0][0] * c00 + m[0][1] * c01 + m[0][2] * c02;
  double id = 1.0 / det;
  inv[0] = (float)(c00 * id);
  inv[1] = (float)((m[0][2] * m[2][1] - m[0][1] * m[2][2]) * id);
  inv[2] = (float)((m[0][1] * m[1][2] - m[0][2] * m[1][1]) * id);
  inv[3] = (float)(c01 * id);
  inv[4] = (float)((m[0][0] * m[2][2] - m[0][2] * m[2][0]) * id);
  inv[5] = (float)((m[0][2] * m[1][0] - m[0][0] * m[1][2]) * id);
  inv[6] = (float)(c02 * id);
  inv[7] = (float)((m[0][1] * m[2][0] - m[0][0] * m[2][1]) * id);
  inv[8] = (float)((m[0][0] * m[1][1] - m[0][1] * m[1][0]) * id);
}

inline void xformPoint(const float a[12], const float p[3], float out[3])
{
  out[0] = ((a[0] * p[0] + a[1] * p[1]) + a[2] * p[2]) + a[3];
  out[1] = ((a[4] * p[0] + a[5] * p[1]) + a[6] * p[2]) + a[7];
  out[2] = ((a[8] * p[0] + a[9] * p[1]) + a[10] * p[2]) + a[11];
}

// Shade class of a material (gi_types.h MAT_CLASS_COUNT): its BSDF class, or -- the reference's per-material feature #defines done the wavefront way,
// GlslShaderGen.cpp:204-274, Gi.cpp:1545-1562 -- the specialised variant its hits are binned and shaded by. OpenPBR BASE: every optional lobe absent (no coat,
// fuzz, thin film, anisotropy, transmission, subsurface, not thin-walled), no bound texture / primvar input, every parameter finite (the variant drops products
// with exact zeros, which a NaN or an infinity would not honour). GATLING_OPTIONS=shade_variants=0 keeps every material in its full kernel (tests: same bits).
uint32_t shadeClassOf(const MaterialRec& m)
{
  if (m.klass != GI_C_MAT_OPEN_PBR || optionValue("shade_variants", 1) == 0) return m.klass & 0xfu;
  if (m.flags & MAT_FLAG_TEXTURED) return m.klass;
  for (uint32_t i = 0; i < MAT_PARAM_COUNT; i++) if (!std::isfinite(m.p[i])) return m.klass;
  if ((uint32_t)m.p[MP_FEATURES] != 0u) return m.klass;
  if (m.p[MP_COAT] != 0.0f || m.p[GI_C_P_CLEARCOAT] != 0.0f || m.p[GI_C_P_TRANSMISSION_WEIGHT] != 0.0f) return m.klass;
  return SHADE_CLASS_OPBR_BASE;
}

// Traits of one derived UsdPreviewSurface record (gi_types.h UPS_*), for the fused kernel's plain class-1 variant.  The variant drops the `coat * x` products,
// which is the same arithmetic only for the exact word of +0.0f: -0.0f would make the coat Fresnel -0 (and 1 - Fc, z - Fc other operations), a NaN stays a NaN.
// A textured record has no trait: the class then runs the textured kernel, whose ups_params recomputes the constants from the hit's texture values.
uint32_t upsTraitsOf(const MaterialRec& m)
{
  if (m.klass != GI_C_MAT_USD_PREVIEW_SURFACE || (m.flags & MAT_FLAG_TEXTURED)) return 0u;
  uint32_t coat; memcpy(&coat, &m.p[MP_COAT], 4);
  return coat == 0u ? UPS_NOCOAT : 0u;
}

// Hostile geometry (bvh8.h "Inactive items").  A coordinate the build works with: finite, at most 1e18 in magnitude.
inline bool usableCoordinate(float x) { return std::fabs(x) <= 1.0e18f; } // (false for NaN)
// An instance the flattening can use: every entry of its affine finite and its 3x3 invertible with an inverse that is finite in fp32 (w2o transforms normals
// and, in the two-level layout, rays). Every triangle of an instance that is not -- a NaN or singular giCSetMeshTransform / instance transform -- is inactive.
inline bool usableInstance(const InstanceRec& ir)
{
  for (int i = 0; i < 12; i++) if (!std::isfinite(ir.o2w[i])) return false;
  for (int i = 0; i < 9; i++) if (!std::isfinite(ir.w2o[i])) return false;
  return true;
}
// giCDebugGatherShade: packVertex + the gather a vertex update runs (gi_refit.h refit_gather_shade) against packTriShade, bytewise.  Host only.
extern "C" int giCDebugGatherShade(const GiCVertex* vertices, uint32_t vertexCount, const GiCFace* faces, uint32_t faceCount)
{
  if ((vertexCount && !vertices) || (faceCount && !faces)) return -1;
  for (uint32_t f = 0; f < faceCount; f++) for (int k = 0; k < 3; k++) if (faces[f].v_i[k] >= vertexCount) return -1;
  try {
    constexpr uint32_t vertexOffset = 3u; // (as a mesh behind others in the scene's arrays: vi holds absolute indices)
    std::vector<FVertex> verts(vertexOffset + (size_t)vertexCount, FVertex{});
    for (uint32_t i = 0; i < vertexCount; i++) verts[vertexOffset + i] = packVertex(vertices[i]);
    int differ = 0;
    for (uint32_t f = 0; f < faceCount; f++) {
      const TriShade packed = packTriShade(vertices, faces[f], vertexOffset);
      TriShade gathered; memset(&gathered, 0xa5, sizeof(gathered)); // (every gathered word must be written)
      for (int k = 0; k < 3; k++) gathered.vi[k] = packed.vi[k];
      gathered.pad = packed.pad;
      refit_gather_shade(verts.data(), (uint32_t)verts.size(), gathered);
      if (memcmp(&gathered, &packed, sizeof(TriShade)) != 0) differ++;
    }
    return differ;
  } catch (const std::exception&) { return -1; }
}
bool usableVertexPositions(const GiCVertex* v, size_t count)
{
  for (size_t i = 0; i < count; i++) for (int a = 0; a < 3; a++) if (!usableCoordinate(v[i].pos[a])) return false;
  return true;
}
// one flattened triangle (Gi.cpp:1188-1202 hands the instance transform to the TLAS; here it is applied); `usable` false: marked inactive for the builder
inline void flattenTriangle(const InstanceRec& ir, bool usable, const GiCMesh* m, uint32_t f, TriRec& t)
{
  float p0[3], p1[3], p2[3];
  xformPoint(ir.o2w, m->vertices[m->faces[f].v_i[0]].pos, p0);
  xformPoint(ir.o2w, m->vertices[m->faces[f].v_i[1]].pos, p1);
  xformPoint(ir.o2w, m->vertices[m->faces[f].v_i[2]].pos, p2);
  for (int a = 0; a < 3; a++) { t.v0[a] = p0[a]; t.e1[a] = p1[a] - p0[a]; t.e2[a] = p2[a] - p0[a]; }
  if (!usable) t.v0[0] = std::numeric_limits<float>::quiet_NaN();
}

// InstanceRec of instance `instInMesh` of mesh `m`, the scene's meshIdx-th (Gi.cpp:1188-1202)
static InstanceRec makeInstanceRec(const GiCMesh* m, uint32_t meshIdx, size_t instInMesh)
{
  InstanceRec ir{};
  composeTransform(m->transform, &m->instanceTransforms[16 * instInMesh], ir.o2w);
  invert3x3(ir.o2w, ir.w2o);
  ir.mesh = meshIdx; ir.instanceId = instInMesh < m->instanceIds.size() ? m->instanceIds[instInMesh] : (int32_t)instInMesh;
  ir.pad = (uint32_t)m->id; // object id
  return ir;
}
// The TriRecs of one flattened instance, out[f] for face f.  idBase: scene-order id of its first triangle; shadeBase: the mesh's first TriShade record where
// vi[0] names the triangle's (scenes beyond LDS), else NOT_PACKED.  buildScene and buildPart: an edited scene and a fresh one hold the same bits through this.
constexpr uint32_t NOT_PACKED = 0xffffffffu;
static void flattenInstance(const InstanceRec& ir, uint32_t instIdx, const GiCMesh* m, uint32_t vertexOffset, uint32_t matFlags, uint32_t idBase, uint32_t shadeBase, TriRec* out)
{
  const bool usable = usableInstance(ir);
  for (uint32_t f = 0; f < (uint32_t)m->faces.size(); f++) {
    TriRec& t = out[f];
    flattenTriangle(ir, usable, m, f, t);
    for (int a = 0; a < 3; a++) t.vi[a] = vertexOffset + m->faces[f].v_i[a];
    t.instance = instIdx; t.prim = f; t.origId = idBase + f; t.matFlags = matFlags;
    if (shadeBase != NOT_PACKED) t.vi[0] = shadeBase + f;
  }
}

// giCDebugCloneInstance: the mesh flattened under instance transform A, every record cloned to instance transform B (gi_refit.h refit_clone_record, what
// gi_patch.hip k_clone_parts runs) under another instance index and id base, against flattenInstance with B, bytewise.  Host only.
extern "C" int giCDebugCloneInstance(const GiCVertex* vertices, uint32_t vertexCount, const GiCFace* faces, uint32_t faceCount, int32_t isLeftHanded,
    const float* xformA, const float* xformB)
{
  if ((vertexCount && !vertices) || (faceCount && !faces) || !xformA || !xformB) return -1;
  for (uint32_t f = 0; f < faceCount; f++) for (int k = 0; k < 3; k++) if (faces[f].v_i[k] >= vertexCount) return -1;
  try {
    GiCMesh m; m.scene = nullptr; m.flipFacing = isLeftHanded != 0; m.id = 11;
    m.vertices.assign(vertices, vertices + vertexCount); m.faces.assign(faces, faces + faceCount);
    m.instanceTransforms.assign(xformA, xformA + 16); m.instanceTransforms.insert(m.instanceTransforms.end(), xformB, xformB + 16);
    constexpr uint32_t vertexOffset = 3u, shadeBase = 5u, meshIdx = 2u, instA = 4u, instB = 9u, idBaseA = 1000u, idBaseB = 77777u; // (as a mesh behind others)
    const uint32_t matFlags = 6u | (m.flipFacing ? 1u << 30 : 0u);
    const InstanceRec a = makeInstanceRec(&m, meshIdx, 0), b = makeInstanceRec(&m, meshIdx, 1);
    if (!usableInstance(a) || !usableInstance(b)) return -1;
    std::vector<TriShade> shade(shadeBase + (size_t)faceCount, TriShade{});
    for (uint32_t f = 0; f < faceCount; f++) shade[shadeBase + f] = packTriShade(vertices, faces[f], vertexOffset);
    std::vector<TriRec> recA(faceCount), recB(faceCount);
    flattenInstance(a, instA, &m, vertexOffset, matFlags, idBaseA, shadeBase, recA.data());
    flattenInstance(b, instB, &m, vertexOffset, matFlags, idBaseB, shadeBase, recB.data());
    int differ = 0;
    for (uint32_t f = 0; f < faceCount; f++) {
      const TriRec cloned = refit_clone_record(recA[f], b.o2w, shade[recA[f].vi[0]].p, instB, idBaseB);
      if (memcmp(&cloned, &recB[f], sizeof(TriRec)) != 0) differ++;
    }
    return differ;
  } catch (const std::exception&) { return -1; }
}

// The MaterialRec table of the scene's materials, in creation order (buildScene and updateMaterials: the one copy of this code)
static void buildMaterialRecords(const GiCScene* s, std::vector<MaterialRec>& mats)
{
  mats.assign(s->materials.size(), MaterialRec{});
  for (size_t i = 0; i < s->materials.size(); i++) {
    mats[i].klass = s->materials[i]->desc.klass; mats[i].flags = s->materials[i]->desc.flags & ~(MAT_FLAG_TEXTURED | MAT_FLAG_OPACITY_TEX);
    for (uint32_t slot = 0; slot < TEX_SLOT_COUNT; slot++) {
      const GiCTextureBinding& b = s->materials[i]->tex[slot];
      TexBindingRec& r = mats[i].tex[slot];
      r = TexBindingRec{};
      auto tit = b.texture ? std::find(s->textures.begin(), s->textures.end(), b.texture) : s->textures.end();
      if (tit == s->textures.end()) {
        if (!s->materials[i]->primvarInput[slot].empty()) {
          r.mode = TEX_MODE_PRIMVAR; mats[i].flags |= MAT_FLAG_TEXTURED;
          // Frontend.cpp:251-252: named scene data answered from the UBO
          if (s->materials[i]->primvarInput[slot] == "CAMERA_POSITION") r.mode |= TEX_MODE_CAMERA_POSITION;
          if (s->materials[i]->primvarInput[slot] == "FRAME") r.mode |= TEX_MODE_FRAME;
        }
        continue;
      }
      r.tex = (uint32_t)(tit - s->textures.begin()) + 1u;
      r.mode = (uint32_t)b.wrapS | ((uint32_t)b.wrapT << 8) | (((uint32_t)b.channel & 3u) << 16);
      memcpy(r.scale, b.scale, 16); memcpy(r.bias, b.bias, 16);
      if (s->materials[i]->hasTexXf[slot]) { r.mode |= TEX_MODE_XFORM; memcpy(r.xf, s->materials[i]->texXf[slot], sizeof(r.xf)); }
      mats[i].flags |= slot == TEX_OPACITY ? MAT_FLAG_OPACITY_TEX : MAT_FLAG_TEXTURED; // opacity is looked up by the any-hit test, not by k_shade
    }
    memcpy(mats[i].p, s->materials[i]->desc.p, sizeof(float) * MAT_PARAM_COUNT);
    deriveMaterialConstants(mats[i]);
  }
}

// Scene data one mesh's material reads (Gi.cpp:905-1019): instancer primvars first, mesh primvars override, by name.  Appends the mesh's MeshRec and its
// primvar arrays (buildScene and updateMaterials: the one copy of this code)
static void appendMeshSceneData(const GiCMesh* m, const GiCMaterial* mat, uint32_t vertexOffset, std::vector<MeshRec>& meshRecs, std::vector<float>& sceneData)
{
  MeshRec mr{}; mr.vertexOffset = vertexOffset;
  for (uint32_t slot = 0; slot < TEX_SLOT_COUNT; slot++) {
    const std::string& want = mat->primvarInput[slot];
    if (want.empty()) continue;
    const GiCPrimvar* pv = nullptr;
    for (const GiCPrimvar& p : m->instancerPrimvars) if (p.name == want && !p.data.empty()) { pv = &p; break; }
    for (const GiCPrimvar& p : m->primvars) if (p.name == want && !p.data.empty()) { pv = &p; break; }
    if (!pv) continue; // SCENE_DATA_INVALID
    const bool isInt = pv->type > GI_C_PRIMVAR_VEC4; // Int .. Int4 (Gi.h:76-79)
    const uint32_t stride = (uint32_t)(isInt ? pv->type - GI_C_PRIMVAR_INT : pv->type) + 1u;
    size_t entries = 1; // what a lookup can index: zero-padded so that short arrays read 0 like the oracle
    if (pv->interpolation == GI_C_INTERP_VERTEX) entries = m->vertices.size();
    else if (pv->interpolation == GI_C_INTERP_UNIFORM) entries = m->faces.size();
    else if (pv->interpolation == GI_C_INTERP_INSTANCE) { int32_t mx = (int32_t)(m->instanceTransforms.size() / 16) - 1;
        for (int32_t id : m->instanceIds) mx = std::max(mx, id); entries = (size_t)std::max(mx, 0) + 1; }
    mr.sdOffset[slot] = (uint32_t)sceneData.size();
    mr.sdInfo[slot] = 1u | ((stride - 1u) << 1) | ((uint32_t)pv->interpolation << 3) | (isInt ? SD_INFO_INT : 0u);
    // (+ 2: a three-component lookup of a one- or two-component primvar reads up to two floats past its last entry -- the reference's stride arithmetic,
    // mdl_interface.glsl:343-349, finds its neighbour in the packed buffer there; here, as in the oracle, zeros.  Found by tests/fuzz_parity.py)
    const size_t need = std::max(entries * stride, pv->data.size()) + 2u;
    sceneData.insert(sceneData.end(), pv->data.begin(), pv->data.end());
    sceneData.resize(mr.sdOffset[slot] + need, 0.0f);
  }
  meshRecs.push_back(mr);
}

// ... for every mesh of the built scene, in MeshBuild order (MeshRec i belongs to meshIdx i): a retired mesh -- destroyed, its records resident until the next
// build, its material possibly gone -- keeps an empty record (updateMaterials and updateTopology: the one copy of this loop)
static void appendBuiltMeshSceneData(const MeshBuild& mb, std::vector<MeshRec>& meshRecs, std::vector<float>& sceneData)
{
  if (mb.m->retired) meshRecs.push_back(MeshRec{}); else appendMeshSceneData(mb.m, mb.m->material, mb.vertexOffset, meshRecs, sceneData);
}
static void remakeSceneData(SceneHost& H)
{
  std::vector<MeshRec> meshRecs; std::vector<float> sceneData;
  for (const MeshBuild& mb : H.meshBuilds) appendBuiltMeshSceneData(mb, meshRecs, sceneData);
  H.meshRecs.swap(meshRecs); H.sceneData.swap(sceneData);
}

// TriRec::matFlags of a mesh bound to material `material` (record `mr`): material index | shade class << 24 | cutout << 28 | mesh flags << 30
static uint32_t meshMatFlags(const MaterialRec& mr, uint32_t material, const GiCMesh* m)
{
  const bool cutoutMat = mr.p[MP_CUTOUT] < 1.0f || (mr.flags & MAT_FLAG_OPACITY_TEX) != 0u;
  return material | (shadeClassOf(mr) << 24) | (cutoutMat ? (1u << 28) : 0u) | (((m->flipFacing ? 1u : 0u) | (m->doubleSided ? 2u : 0u)) << 30);
}

// FaceId AOV values of a mesh's faces, bug-compatible: face ids are stored with a 1/2/4-byte stride chosen from maxFaceId (Gi.cpp:878-885); the shader fetches
// the 32-bit word prim / (4/stride), shifts it by (prim % (4/stride)) * 8 bits (sic) and masks it with (stride*8 - 1) (rp_main.chit:231-240).  Evaluated once
// per primitive here (buildScene and updateTopology: the one copy of this code)
static std::vector<int32_t> faceIdAovOf(const GiCMesh* m)
{
  std::vector<int32_t> meshFaceIdAov(m->faces.size());
  const int stride = m->maxFaceId <= 255u ? 1 : (m->maxFaceId <= 65535u ? 2 : 4), invStride = 4 / stride;
  std::vector<uint8_t> packed(((size_t)m->faces.size() * stride + 3) / 4 * 4, 0);
  for (size_t i = 0; i < m->faces.size(); i++) { int32_t fid = i < m->faceIds.size() ? m->faceIds[i] : 0; memcpy(&packed[i * stride], &fid, stride); }
  for (size_t i = 0; i < m->faces.size(); i++) {
    int32_t word; memcpy(&word, &packed[(i / (size_t)invStride) * 4], 4);
    word >>= (int)((i % (size_t)invStride) * 8);
    meshFaceIdAov[i] = word & (stride * 8 - 1);
  }
  return meshFaceIdAov;
}

// the shadow walks' order is chosen anew
static void resetShadowOrder(GiCScene* s) { s->shadowOrder = -1; s->shadowOrderRays[0] = s->shadowOrderRays[1] = s->shadowOrderSteps[0] = s->shadowOrderSteps[1] = 0; }

// The scene's class masks and cutout flag: which kernel variants a render launches and whether walks run the any-hit test.  The one place that writes them:
// every build, and every update that changes a mesh's word or visibility, ends here.  Taken from the words of the meshes a fresh build would hold (a hidden mesh
// launches no kernel variant) and the material table they index.  The shadow order was chosen for one tree and for walks with / without the any-hit test.
static void deriveSceneClasses(GiCScene* s, const SceneHost& H, bool newTree)
{
  const bool hadCutouts = s->hasCutouts;
  s->classMask = 0; s->classTextured = 0; s->shadeClassMask = 0; s->shadeClassTextured = 0; s->hasCutouts = false;
  uint32_t ups = UPS_NOCOAT; // what the class-1 materials in use have in common
  for (const MeshBuild& mb : H.meshBuilds) {
    if (mb.hidden) continue;
    const MaterialRec& mr = H.mats[mb.matFlags & 0x00ffffffu];
    const uint32_t klassBit = 1u << (mr.klass & 0xfu), shadeBit = 1u << ((mb.matFlags >> 24) & 0xfu);
    s->classMask |= klassBit; s->shadeClassMask |= shadeBit;
    if (mr.flags & MAT_FLAG_TEXTURED) { s->classTextured |= klassBit; s->shadeClassTextured |= shadeBit; }
    if (mb.matFlags & (1u << 28)) s->hasCutouts = true;
    if (mr.klass == GI_C_MAT_USD_PREVIEW_SURFACE) ups &= upsTraitsOf(mr);
  }
  s->upsTraits = (s->classMask & 2u) ? ups : 0u;
  if (newTree || s->hasCutouts != hadCutouts) resetShadowOrder(s);
}

// Two-level layout (SceneView::tlasNodes ...): built next to the flat BVH for instanced scenes that do not fit LDS.  The flat
// arrays stay (k_shade reads the hit's TriRec, k_aov / giCTraceRays traverse them); the two-level ones are what k_trace_dyn2 walks,
// and they are small: one BLAS per MESH instead of one subtree per instance, so traversal stays in the caches.  (With GI_C_SCENE_OPTION_TLAS_ONLY the flat
// NODES are not built at all -- buildSceneTreeless below: the flat records stay, in scene order, and k_aov2 walks these arrays for the AOVs as well.)
// The BLAS of one mesh (buildTwoLevel; giCDebugBlasRefit): a tree over the padded object-space boxes of its faces.  A face with an unusable corner keeps an
// inverted box: the builder leaves it out, and it does not widen mlo / mhi, the union of the usable faces' boxes
void buildMeshBlas(const GiCVertex* vertices, const GiCFace* faces, size_t nf, Bvh8& b, std::vector<uint32_t>& order, float mlo[3], float mhi[3])
{
  std::vector<float> boxes(nf * 6);
  for (int a = 0; a < 3; a++) { mlo[a] = 3.0e38f; mhi[a] = -3.0e38f; }
  for (size_t f = 0; f < nf; f++) {
    float lo[3] = {3.0e38f, 3.0e38f, 3.0e38f}, hi[3] = {-3.0e38f, -3.0e38f, -3.0e38f};
    bool faceOk = true; // (an unusable face keeps an inverted box: the builder leaves it out, and it must not widen the mesh magnitude below)
    for (int k = 0; k < 3; k++) { const float* p = vertices[faces[f].v_i[k]].pos;
        for (int a = 0; a < 3; a++) { lo[a] = std::min(lo[a], p[a]); hi[a] = std::max(hi[a], p[a]); faceOk = faceOk && usableCoordinate(p[a]); } }
    if (faceOk) tlas_pad_box(lo, hi); else for (int a = 0; a < 3; a++) { lo[a] = 3.0e38f; hi[a] = -3.0e38f; }
    for (int a = 0; a < 3; a++) { boxes[6 * f + a] = lo[a]; boxes[6 * f + 3 + a] = hi[a]; }
    if (faceOk) for (int a = 0; a < 3; a++) { mlo[a] = std::min(mlo[a], lo[a]); mhi[a] = std::max(mhi[a], hi[a]); }
  }
  buildBvh8Boxes(boxes.data(), nf, b, order);
}
// ... and its record of face f, as the builder's order places it
BlasTri makeBlasTri(const GiCVertex* vertices, const GiCFace* faces, uint32_t f)
{
  BlasTri bt{};
  memcpy(bt.p0, vertices[faces[f].v_i[0]].pos, 12); memcpy(bt.p1, vertices[faces[f].v_i[1]].pos, 12); memcpy(bt.p2, vertices[faces[f].v_i[2]].pos, 12);
  bt.prim = f;
  return bt;
}

// The BLAS of one mesh that will sit under a TLAS of depth `tlasDepth` (defined behind onSceneDevices): the ONE place the scene's code chooses the builder.
// Returns the depth budget of a device build, 0 where the host builder made the tree
static uint32_t makeMeshBlas(GiCScene* s, bool deviceWanted, uint32_t tlasDepth, const GiCMesh* m, Bvh8& b, std::vector<uint32_t>& order, float mlo[3], float mhi[3]);
// ... made anew by the builder that made the resident one (the checks): the host form under `budget`, or the host builder where budget is 0
static bool remakeMeshBlas(uint32_t budget, const GiCMesh* m, Bvh8& b, std::vector<uint32_t>& order, float mlo[3], float mhi[3]);

// ... and where the slot is free (MeshBuild::freeSlots: an instancer edit in place of the two-level layout retired its instance)
template <class MB>
static void markFreeSlots(const std::vector<MB>& meshBuilds, std::vector<uint8_t>& hidden)
{
  for (const MB& mb : meshBuilds) for (const auto& fs : mb.freeSlots) if (fs.inst < hidden.size()) hidden[fs.inst] = 1;
}
// one byte per flattened instance: 1 where its mesh is hidden (MeshBuild::hidden: visibility updates in place)
template <class MB>
static std::vector<uint8_t> hiddenOfInstances(const std::vector<MB>& meshBuilds, size_t instanceCount)
{
  std::vector<uint8_t> hidden(instanceCount, 0);
  for (const MB& mb : meshBuilds) if (mb.hidden) for (const uint32_t inst : mb.inst) if (inst < instanceCount) hidden[inst] = 1;
  markFreeSlots(meshBuilds, hidden); // (the slots of retired instances: hidden until a grow of their mesh takes them, updateInstancesTwoLevel)
  return hidden;
}

// flatNodes == 0: the caller has no flat tree (buildScene's route for GI_C_SCENE_OPTION_TLAS_ONLY, and the checks of a scene built that way).  "Beyond LDS" is
// then what sceneFitsLds answers for the triangles alone -- more than LDS_TRIS of them --, and the automatic rule on node bytes is not consulted.
// sceneBuild: the call is buildScene's -- with GI_C_SCENE_OPTION_BLAS_DEVICE_BUILD wanted makeMeshBlas may take a mesh's BLAS to the device, under the budget the
// TLAS of this same build leaves (instance boxes do not depend on a BLAS's shape, so the TLAS is built first).  Otherwise (the checks of a resident scene) every
// BLAS is made anew by the builder that made the resident one (TwoLevelHost::meshBlasBudget).
template <class MB>
int buildTwoLevel(GiCScene* s, const std::vector<MB>& meshBuilds, const std::vector<InstanceRec>& instances, size_t flatTris, size_t flatNodes,
    TwoLevelHost& out, bool sceneBuild = false)
{
  s->twoLevel = false;
  int want = s->optTwoLevel;
  want = (int)optionValue("two_level", want);
  const bool beyondLds = !sceneFitsLds(flatNodes, flatTris);
  // Opt-in only. Measured (r01k): although its working set is tiny (C4: 1.5 MB of BLAS nodes + 2.6 MB of mesh triangles instead of 41 + 335 MB) the first
  // version is SLOWER than the flat layout -- C4 trace 185 -> 207 ms, C5 834 -> 1945 ms (29 instead of 20 nodes per ray: overlapping instance boxes, each visit
  // pays a ray transform, a BLAS root and a restore; candidates cost a rebuild). ... except where the flat traversal cannot address the scene: its
  // wave-cooperative triangle ring packs (lane, flat triangle) into 32 bits, 2^26 triangles; the two-level walk queues MESH triangles there (one BLAS per
  // mesh), so heavily instanced scenes beyond that bound take it automatically (r04; the hit record's triangle word, flat index | class << 28, then bounds the
  // scene at 2^28 flattened triangles)
  if (flatTris >= ((size_t)1 << 26) && want < 0) want = 1;
  // (the flat walk addresses nodes by 32-bit byte offset, gi_traversal.h node_load: 53 M nodes -- beyond any 2^26-triangle tree)
  if (flatNodes * sizeof(Node8) >= ((size_t)1 << 32) && want < 0) want = 1;
  if (want <= 0 || instances.empty() || !beyondLds) return GI_C_OK;
  std::vector<Node8> blasNodes; std::vector<BlasTri> blasTris; std::vector<InstTrav> instTrav(instances.size());
  uint32_t blasDepth = 0;
  std::vector<float> instBoxes(instances.size() * 6); std::vector<uint32_t> meshBlasTri(meshBuilds.size(), 0u), meshBlasNode(meshBuilds.size(), 0u);
  std::vector<std::vector<uint32_t>> meshBlasLevels(meshBuilds.size());
  std::vector<uint32_t> meshBlasBudget(meshBuilds.size(), 0u);
  const std::vector<uint32_t>* residentBudget = !sceneBuild && s->host ? &s->host->two.meshBlasBudget : nullptr;
  // (gi_tlas.h: the point transform, the pad, the status rule and the InstTrav record are shared with the transform update in place and its kernels)
  auto padBox = [](float* lo, float* hi) { tlas_pad_box(lo, hi); };
  // the instances' world boxes first: they read the meshes' points, never a BLAS
  for (const MB& mb : meshBuilds) {
    if (mb.instCount == 0) continue;
    const GiCMesh* m = mb.m;
    const size_t nf = m->faces.size();
    for (uint32_t ii = 0; ii < mb.instCount; ii++) {
      const uint32_t inst = mb.inst[ii];
      // inactive triangles (bvh8.h): a face with an unusable OBJECT-space vertex is left out of the BLAS by the builder and out of this box; an unusable
      // instance keeps the inverted box (the builder leaves it out of the TLAS). A usable face whose WORLD-space vertex is unusable is inactive in the flat
      // tree but would be walked here: such scenes keep the flat layout
      TlasBounds wb; tlas_bounds_init(wb);
      if (usableInstance(instances[inst]))
        for (size_t f = 0; f < nf && !(wb.status & TLAS_STATUS_WORLD); f++) {
          float p[3][3];
          for (int k = 0; k < 3; k++) memcpy(p[k], m->vertices[m->faces[f].v_i[k]].pos, 12);
          tlas_bounds_add_tri(instances[inst].o2w, p, wb, false);
        }
      if (wb.status & TLAS_STATUS_WORLD) {
        if (want > 0) fprintf(stderr,
            "[gatling_gi] two-level layout not used: an instance carries triangles that leave the usable coordinate range in world space\n");
        return GI_C_OK;
      }
      float* lo = wb.lo; float* hi = wb.hi;
      padBox(lo, hi);
      for (int a = 0; a < 3; a++) { instBoxes[6 * inst + a] = lo[a]; instBoxes[6 * inst + 3 + a] = hi[a]; }
    }
  }
  Bvh8 tlas; std::vector<uint32_t> tlasItems;
  { // the hidden rule (never at a build: buildScene leaves invisible meshes out; giCDebugSceneTlasCheck / giCDebugSceneBlasCheck over a resident scene whose
    // meshes updateVisibilityTwoLevel hid): the TLAS does not name the instances of a hidden mesh; `instBoxes` keeps their true boxes
    std::vector<uint8_t> hidden = hiddenOfInstances(meshBuilds, instances.size());
    if (std::find(hidden.begin(), hidden.end(), (uint8_t)1) == hidden.end()) buildBvh8Boxes(instBoxes.data(), instances.size(), tlas, tlasItems);
    else {
      std::vector<float> masked(instBoxes);
      tlasMaskHiddenBoxes(masked.data(), hidden.data(), instances.size());
      buildBvh8Boxes(masked.data(), instances.size(), tlas, tlasItems);
    }
  }
  // the BLASes, under the TLAS they will sit under
  const bool blasOnDevice = sceneBuild && blasDeviceBuildWanted(s);
  for (const MB& mb : meshBuilds) {
    if (mb.instCount == 0) continue;
    const GiCMesh* m = mb.m;
    const size_t nf = m->faces.size();
    float mlo[3], mhi[3];
    Bvh8 b; std::vector<uint32_t> order;
    uint32_t budget = 0u;
    if (sceneBuild) budget = makeMeshBlas(s, blasOnDevice, tlas.maxDepth, m, b, order, mlo, mhi);
    else {
      budget = residentBudget && mb.meshIdx < residentBudget->size() ? (*residentBudget)[mb.meshIdx] : 0u;
      if (!remakeMeshBlas(budget, m, b, order, mlo, mhi)) { setError("the host form of the device BLAS builder failed on a mesh the device built"); return GI_C_ERROR; }
    }
    const uint32_t nodeBase = (uint32_t)blasNodes.size(), triBase = (uint32_t)blasTris.size();
    if (mb.meshIdx < meshBlasTri.size()) { meshBlasTri[mb.meshIdx] = triBase; meshBlasNode[mb.meshIdx] = nodeBase; meshBlasLevels[mb.meshIdx] = b.levelStart;
        meshBlasBudget[mb.meshIdx] = budget; }
    for (Node8 n : b.nodes) { n.childBase += nodeBase; n.triBase += triBase; blasNodes.push_back(n); }
    for (uint32_t f : order) blasTris.push_back(makeBlasTri(m->vertices.data(), m->faces.data(), f));
    blasDepth = std::max(blasDepth, b.maxDepth);
    // object-space magnitude the transformed ray's rounding error scales with inside this mesh (see wave_step2)
    const float extent = (std::fabs(mlo[0]) + std::fabs(mlo[1]) + std::fabs(mlo[2])) + (std::fabs(mhi[0]) + std::fabs(mhi[1]) + std::fabs(mhi[2]));
    // (idBase is triFirst at a build; after visibility updates in place -- updateVisibilityTwoLevel, which giCDebugSceneTlasCheck holds to this function --
    // it is the id a fresh build of the visible meshes gives the mesh's first triangle, and a hidden mesh keeps the one it had)
    for (uint32_t ii = 0; ii < mb.instCount; ii++)
      instTrav[mb.inst[ii]] = tlasMakeInstTrav(instances[mb.inst[ii]], nodeBase, mb.idBase + ii * (uint32_t)nf, mb.matFlags, extent);
  }
  // per-lane stack: a TLAS level can leave a node group and an instance group behind, a BLAS level a node group
  if (blasTris.size() >= ((size_t)1 << 26)) {
    if (want > 0) fprintf(stderr, "[gatling_gi] two-level layout not used: 2^26 or more unique mesh triangles\n");
    return GI_C_OK;
  }
  if (2u * tlas.maxDepth + blasDepth + 1u > 16u) {
    if (want > 0) fprintf(stderr, "[gatling_gi] two-level layout not used: trees too deep for the 16-entry stack\n");
    return GI_C_OK;
  }
  s->twoLevel = true;
  if (getenv("GATLING_BUILD_TIMING")) {
    if (flatNodes) fprintf(stderr,
      "[gatling_gi] two-level: TLAS %zu nodes over %zu instances, %zu BLAS nodes, %zu mesh triangles (flat: %zu nodes, %zu triangles)\n",
                                              tlas.nodes.size(), instances.size(), blasNodes.size(), blasTris.size(), flatNodes, flatTris);
    else fprintf(stderr, "[gatling_gi] two-level: TLAS %zu nodes over %zu instances, %zu BLAS nodes, %zu mesh triangles (no flat tree was built; %zu flat "
                         "records in scene order)\n", tlas.nodes.size(), instances.size(), blasNodes.size(), blasTris.size(), flatTris);
  }
  out.tlasNodes.swap(tlas.nodes); out.tlasItems.swap(tlasItems); out.blasNodes.swap(blasNodes); out.blasTris.swap(blasTris); out.instTrav.swap(instTrav);
  out.instBoxes.swap(instBoxes); out.meshBlasTri.swap(meshBlasTri); out.tlasDepth = tlas.maxDepth; out.blasDepth = blasDepth;
  out.tlasDeviceBuilt = false; out.tlasBuildBudget = 0u; // (a build's TLAS is the host builder's)
  out.meshBlasNode.swap(meshBlasNode); out.meshBlasLevels.swap(meshBlasLevels); out.meshBlasBudget.swap(meshBlasBudget);
  return GI_C_OK;
}

// Textures of one device: one device array per image + the TextureRec table.  An image the device already holds (GiCTexture::serial; texels never change
// after giCCreateTexture) keeps its array, so a scene build or a material update sends only new images; arrays of textures that are gone are released.
static int uploadTexturesTo(GiCScene* s, SceneDevice& D, hipStream_t st)
{
  std::vector<DeviceBuffer<float>*> old; old.swap(D.dTexels);
  std::vector<uint64_t> oldSerial; oldSerial.swap(D.dTexelSerial);
  std::vector<TextureRec> recs(s->textures.size());
  int rc = GI_C_OK;
  for (size_t i = 0; i < s->textures.size() && rc == GI_C_OK; i++) {
    DeviceBuffer<float>* b = nullptr;
    for (size_t k = 0; k < old.size(); k++) if (old[k] && oldSerial[k] == s->textures[i]->serial) { b = old[k]; old[k] = nullptr; break; }
    const bool resident = b != nullptr;
    if (!resident) b = new DeviceBuffer<float>();
    D.dTexels.push_back(b); D.dTexelSerial.push_back(s->textures[i]->serial);
    if (!resident && b->upload(s->textures[i]->rgba, st)) rc = GI_C_ERROR;
    recs[i] = TextureRec{b->ptr, s->textures[i]->width, s->textures[i]->height};
  }
  // (the stream is drained first: a render that read the released arrays was synchronised by giCRender, an upload above may still be in flight)
  if (rc == GI_C_OK && D.dTextures.upload(recs, st)) rc = GI_C_ERROR;
  if (hipStreamSynchronize(st) != hipSuccess && rc == GI_C_OK) { setError("hipStreamSynchronize failed (texture upload)"); rc = GI_C_ERROR; } // `recs` goes out of scope
  for (auto* b : old) if (b) { b->release(); delete b; }
  return rc;
}

// ... and its upload into one device's memory (the primary's and every replica's: multi-device renders replicate the scene); onSceneDevices made it current
static int uploadSceneTo(GiCScene* s, SceneDevice& D, const SceneHost& H, hipStream_t st)
{
  if (s->twoLevel) {
    if (D.dTlasNodes.upload(H.two.tlasNodes, st) || D.dTlasItems.upload(H.two.tlasItems, st) || D.dBlasNodes.upload(H.two.blasNodes, st)
        || D.dBlasTris.upload(H.two.blasTris, st) ||
        D.dInstTrav.upload(H.two.instTrav, st) || D.dFlatOfOrig.upload(H.flatOfOrig, st))
      return GI_C_ERROR;
  }
  if ((!H.deviceBuilt && D.dTriFaceId.upload(H.triFaceId, st)) || D.dTriShade.upload(H.triShade, st) || D.dTriGeomNormal.upload(H.triGeomNormal, st))
    return GI_C_ERROR;
  if (D.dMeshes.upload(H.meshRecs, st) || D.dSceneData.upload(H.sceneData, st)) return GI_C_ERROR;
  if (uploadTexturesTo(s, D, st) != GI_C_OK) return GI_C_ERROR;
  if (H.treeless) { D.dNodes.release(); if (D.dTris.upload(H.bvh.tris, st)) return GI_C_ERROR; } // (no flat tree: no device holds flat nodes)
  else if (!H.deviceBuilt && (D.dNodes.upload(H.bvh.nodes, st) || D.dTris.upload(H.bvh.tris, st))) return GI_C_ERROR; // (device-built: the builder writes them)
  if (D.dInstances.upload(H.instances, st) || D.dVerts.upload(H.verts, st) || D.dMaterials.upload(H.mats, st)) return GI_C_ERROR;
  HIP_TRY(hipStreamSynchronize(st)); // host vectors may go out of scope
  return GI_C_OK;
}

// devices a render of this scene may use (replicas exist for slots 1 .. n-1 after buildScene)
uint32_t sceneDeviceCount(const GiCScene* s)
{
  uint32_t n = (uint32_t)g_ctx.devs.size();
  if (s->optDevices > 0) n = std::min<uint32_t>(n, (uint32_t)s->optDevices);
  return std::max(n, 1u);
}
SceneDevice& sceneDevice(GiCScene* s, uint32_t slot) { return slot == 0u ? static_cast<SceneDevice&>(*s) : *s->replicas[slot - 1u]; }

// one copy of the scene per device this scene renders on (a build); a new replica has no lights yet
static void ensureReplicas(GiCScene* s)
{
  while (s->replicas.size() + 1u < sceneDeviceCount(s)) { s->replicas.emplace_back(new SceneDevice()); s->replicas.back()->slot = (uint32_t)s->replicas.size();
      s->dirty |= DIRTY_LIGHTS; }
}
static uint32_t residentDeviceCount(const GiCScene* s) { return std::min<uint32_t>(sceneDeviceCount(s), (uint32_t)s->replicas.size() + 1u); } // (an update)

// The frame of all per-device work: fn(SceneDevice&, hipStream_t) -> int runs for the scene's first nDev devices in turn, each made current, until one does
// not answer GI_C_OK; that answer is returned.  The primary device is current again on every exit.
template <class Fn> int onSceneDevices(GiCScene* s, uint32_t nDev, Fn&& fn)
{
  int rc = GI_C_OK;
  auto makeCurrent = [&rc](int device) { if (hipSetDevice(device) != hipSuccess && rc == GI_C_OK) { setError("hipSetDevice failed"); rc = GI_C_ERROR; } };
  for (uint32_t d = 0; d < nDev && rc == GI_C_OK; d++) {
    SceneDevice& D = sceneDevice(s, d);
    makeCurrent(g_ctx.devs[D.slot].device);
    if (rc == GI_C_OK) rc = fn(D, g_ctx.devs[D.slot].stream);
  }
  makeCurrent(g_ctx.device);
  return rc;
}

// GI_C_SCENE_OPTION_BLAS_DEVICE_BUILD / GATLING_OPTIONS=blas_device_build
bool blasDeviceBuildWanted(const GiCScene* s)
{
  const long o = optionValue("blas_device_build", -1);
  return o >= 0 ? o == 1 : s->optBlasDeviceBuild == 1;
}
// 0: a mesh of nf faces is the device builder's; 1: under blas_device_min; 2: over blas_device_max (the indices of the fallback counters in blasBuildStats)
static int blasDeviceRange(size_t nf)
{
  const long lo = optionValue("blas_device_min", BLAS_DEVICE_MIN_DEFAULT), hi = std::min(optionValue("blas_device_max", BLAS_DEVICE_MAX_DEFAULT), (long)kBlasMaxItems);
  return (long)nf < lo ? 1 : (long)nf > hi ? 2 : 0;
}
// With the option wanted a mesh of blas_device_min .. blas_device_max faces gets its BLAS from the primary device (gi_blas_build.hip; the scene's slab) under
// B = min(kBlasMaxBudget, 15 - 2 * tlasDepth); the nodes and the order are read back, and the caller goes on as behind the host builder.  Outside the range,
// on a tree that does not fit the budget, out of memory or on an error status the host builder runs instead (counted in GiCScene::blasBuildStats): a build
// never fails because of the option, and the render is the same.
static uint32_t makeMeshBlas(GiCScene* s, bool deviceWanted, uint32_t tlasDepth, const GiCMesh* m, Bvh8& b, std::vector<uint32_t>& order, float mlo[3], float mhi[3])
{
  const size_t nf = m->faces.size();
  if (deviceWanted) {
    uint64_t* stats = s->blasBuildStats;
    const bool timing = getenv("GATLING_BUILD_TIMING") != nullptr;
    uint32_t budget = blasDepthBudget(tlasDepth);
    if (optionSet("blas_depth_budget")) budget = std::min(budget, (uint32_t)std::max(optionValue("blas_depth_budget", 0), 0L));
    const int range = blasDeviceRange(nf);
    const double t0 = nowMs();
    if (range != 0) {
      stats[range]++;
      buildMeshBlas(m->vertices.data(), m->faces.data(), nf, b, order, mlo, mhi);
      if (timing) fprintf(stderr, "[gatling_gi] BLAS of %zu faces: the host builder (%s), %.3f ms\n", nf, range == 1 ? "under blas_device_min" : "over blas_device_max",
          nowMs() - t0);
      return 0u;
    } else {
      const uint32_t radius = (uint32_t)std::min(std::max(optionValue("ploc_radius", 16), 1L), 256L);
      BlasBuildInfo info; int rc = budget == 0u ? TLAS_BUILD_TOO_DEEP : TLAS_BUILD_ERROR;
      if (budget != 0u) (void)onSceneDevices(s, 1u, [&](SceneDevice& D, hipStream_t st) -> int {
        rc = buildBlasDevice(D.tlasWorkspace, st, m->vertices.data(), m->vertices.size(), m->faces.data(), nf, budget, radius, b, order, mlo, mhi, info);
        return GI_C_OK;
      });
      if (rc == TLAS_BUILD_OK) {
        stats[0]++;
        for (int k = 0; k < 4; k++) stats[6 + k] = (uint64_t)(info.ms[k] * 1000.0f);
        stats[10] = info.passes; stats[11] = info.hostWaits; stats[12] = info.maxDepth; stats[13] = info.nodeCount; stats[14] = budget;
        if (timing) fprintf(stderr, "[gatling_gi] BLAS of %zu faces: the device builder, %.3f ms, %u node(s), depth %u of %u, %u PLOC pass(es), %u host wait(s); upload + "
            "boxes + sort %.3f ms, PLOC %.3f ms, emission %.3f ms, read-back %.3f ms\n", nf, nowMs() - t0, info.nodeCount, info.maxDepth, budget, info.passes,
            info.hostWaits, info.ms[0], info.ms[1], info.ms[2], info.ms[3]);
        return budget;
      }
      stats[rc == TLAS_BUILD_TOO_DEEP ? 3 : rc == TLAS_BUILD_OUT_OF_MEMORY ? 4 : 5]++;
      if (timing) fprintf(stderr, "[gatling_gi] BLAS of %zu faces: the host builder (device build after %.3f ms: %s)\n", nf, nowMs() - t0, rc == TLAS_BUILD_TOO_DEEP ?
          "the tree does not fit the depth budget" : rc == TLAS_BUILD_OUT_OF_MEMORY ? "out of device memory" : info.error);
    }
  }
  buildMeshBlas(m->vertices.data(), m->faces.data(), nf, b, order, mlo, mhi);
  return 0u;
}
static bool remakeMeshBlas(uint32_t budget, const GiCMesh* m, Bvh8& b, std::vector<uint32_t>& order, float mlo[3], float mhi[3])
{
  if (budget == 0u) { buildMeshBlas(m->vertices.data(), m->faces.data(), m->faces.size(), b, order, mlo, mhi); return true; }
  const uint32_t radius = (uint32_t)std::min(std::max(optionValue("ploc_radius", 16), 1L), 256L);
  BlasBuildInfo info;
  return buildBlasHost(m->vertices.data(), m->vertices.size(), m->faces.data(), m->faces.size(), budget, radius, b, order, mlo, mhi, info) == TLAS_BUILD_OK;
}

static int uploadTopTree(SceneDevice& D, const SceneHost& H, hipStream_t st) // the top tree of a partitioned scene: nodes [0, topCap)
{ HIP_TRY(hipMemcpyAsync(D.dNodes.ptr, H.bvh.nodes.data(), (size_t)H.topCap * sizeof(Node8), hipMemcpyHostToDevice, st)); return GI_C_OK; }

// The flat tree's root bounds for FLAG_BOUNDS_RETIRE: the dequantised child boxes of node 0 (which contain every triangle's padded box), padded once more by
// 1e-5 of their magnitude and extent -- k_raygen's slab test adds its own per-ray rounding allowance on top.
static void setSceneBounds(GiCScene* s, const std::vector<Node8>& nodes)
{
  s->boundsValid = false;
  if (nodes.empty()) return;
  float b[6]; nodeBounds(nodes[0], b);
  for (int a = 0; a < 3; a++) {
    if (!(b[a] <= b[3 + a]) || !std::isfinite(b[a]) || !std::isfinite(b[3 + a])) return; // empty root (no triangles) or overflowing planes: no early retire
    const float pad = (std::fabs(b[a]) + std::fabs(b[3 + a]) + (b[3 + a] - b[a])) * 1.0e-5f + 1.0e-30f;
    s->bounds[a] = b[a] - pad; s->bounds[3 + a] = b[3 + a] + pad;
  }
  s->boundsValid = true;
}

// ... and of a two-level scene without the flat tree (SceneHost::treeless), at its build and after every edit in place: the union of the padded world boxes of
// the instances the TLAS names (gi_tlas.h tlas_scene_bounds), under the same pad and the same validity rule
static void setSceneBoundsFromInstances(GiCScene* s, const SceneHost& H)
{
  const size_t n = H.instances.size();
  s->boundsValid = false;
  if (H.two.instBoxes.size() != 6u * n) return; // (cannot happen)
  const std::vector<uint8_t> hidden = hiddenOfInstances(H.meshBuilds, n);
  float b[6]; bool valid = false;
  tlas_scene_bounds(H.two.instBoxes.data(), hidden.data(), n, b, valid);
  if (valid) memcpy(s->bounds, b, sizeof(b));
  s->boundsValid = valid;
}

// inactive triangles among scene-order records by bvh8.cpp's rule (prepareRange); perMesh[meshIdx] = the mesh's count
static uint32_t countInactive(const std::vector<TriRec>& tris, const SceneHost& H, std::vector<uint32_t>& perMesh)
{
  uint32_t inactive = 0;
  perMesh.assign(H.meshBuilds.size(), 0u);
  for (const TriRec& t : tris) {
    bool ok = true;
    for (int a = 0; a < 3; a++) ok = ok && usableCoordinate(t.v0[a]) && usableCoordinate(t.v0[a] + t.e1[a]) && usableCoordinate(t.v0[a] + t.e2[a]);
    if (!ok) { inactive++; perMesh[H.instances[t.instance].mesh]++; }
  }
  return inactive;
}

// one line per mesh with inactive triangles (bvh8.h "Inactive items"); perMesh[meshIdx] = its inactive count
static void warnInactive(const std::vector<MeshBuild>& meshBuilds, const std::vector<uint32_t>& perMesh)
{
  for (const MeshBuild& mb : meshBuilds)
    if (perMesh[mb.meshIdx]) fprintf(stderr, "[gatling_gi] warning: mesh %s: %u of %zu instanced triangle(s) have a non-finite or out-of-range (> 1e18) "
                                              "vertex or a non-invertible transform and are inactive\n",
                                     mb.m->name.c_str(), perMesh[mb.meshIdx], mb.m->faces.size() * (size_t)mb.instCount);
}

// Scenes beyond LDS: one 160-byte shading record per mesh triangle (gi_types.h TriShade), meshes in build order; returns each mesh's first record by meshIdx
static std::vector<uint32_t> buildShadeRecords(SceneHost& H)
{
  std::vector<uint32_t> shadeBaseOfMesh(H.meshBuilds.size(), 0u);
  for (MeshBuild& mb : H.meshBuilds) {
    mb.shadeBase = (uint32_t)H.triShade.size(); shadeBaseOfMesh[mb.meshIdx] = mb.shadeBase;
    const GiCMesh* m = mb.m;
    for (const GiCFace& f : m->faces) H.triShade.push_back(packTriShade(m->vertices.data(), f, mb.vertexOffset));
  }
  return shadeBaseOfMesh;
}

// What either builder leaves behind a tree that every device holds (H.bvh.maxDepth levels; `top`: its root node first): the scene's sizes, bounds and class
// state, the statistics; the scene owns the host copy from here.
static int finishBuild(GiCScene* s, std::unique_ptr<SceneHost>& hostPtr, uint32_t nodes, uint32_t tris, const std::vector<Node8>& top, double buildMs,
    double uploadMs, const char* how)
{
  const uint32_t levels = hostPtr->bvh.maxDepth;
  s->shadePacked = hostPtr->shadePacked; deriveSceneClasses(s, *hostPtr, true); // (a new tree)
  // stack entries a walk can need: a pick at level L pushes the rest of level L-1's group (gi_traversal.h trav_node_pick), the root level pushes nothing
  s->nodeCount = nodes; s->triCount = tris; s->bvhDepth = levels > 1u ? levels - 1u : 1u;
  setSceneBounds(s, top);
  s->stats.bvhBuildMs = buildMs; s->stats.uploadMs = uploadMs; s->stats.nodeCount = nodes; s->stats.triangleCount = tris;
  if (getenv("GATLING_BUILD_TIMING")) fprintf(stderr, "[gatling_gi] scene%s: %u nodes, %u triangles, %u levels (traversal stack need %u)\n", how, nodes, tris,
      levels, s->bvhDepth);
  s->host = std::move(hostPtr);
  return GI_C_OK;
}

// The device builder's side of buildScene (GI_C_SCENE_OPTION_BVH_BUILD; gi_bvh_build.hip): the flattened scene-order triangles and face ids are uploaded to
// every device and each device builds its own tree over them (the builder is deterministic: the copies are identical).  Nothing of the tree is kept on the
// host.  Returns GI_C_OK / GI_C_ERROR, or DEVICE_BUILD_FALLBACK when the host builder must take over (out of device memory, a tree deeper than the traversal
// stack): not an error.
constexpr int DEVICE_BUILD_FALLBACK = 2; // (neither GI_C_OK nor GI_C_ERROR)
static int buildSceneOnDevice(GiCScene* s, std::unique_ptr<SceneHost>& hostPtr, std::vector<TriRec>& tris, const std::vector<int32_t>& faceIdOf, double t0)
{
  SceneHost& H = *hostPtr;
  const uint32_t n = (uint32_t)tris.size();
  // inactive triangles by bvh8.cpp's rule (prepareRange), counted here as well: the statistic and the per-mesh warnings are the host path's
  std::vector<uint32_t> perMesh;
  const uint32_t inactive = countInactive(tris, H, perMesh);
  s->twoLevel = false;
  // (bvhBuildMs / uploadMs split as on the host path: flattening and the build, then the shading records and the uploads)
  double buildMs = nowMs() - t0;
  // beyond LDS by construction (more than 128 triangles): shading records, and TriRec::vi[0] names the triangle's record -- set in scene order, the gather
  // carries it along
  H.shadePacked = true; H.triShade.clear(); H.triGeomNormal.clear();
  const std::vector<uint32_t> shadeBaseOfMesh = buildShadeRecords(H);
  for (TriRec& t : tris) t.vi[0] = shadeBaseOfMesh[H.instances[t.instance].mesh] + t.prim;
  H.deviceBuilt = true;
  const bool timing = getenv("GATLING_BUILD_TIMING") != nullptr;
  double uploadMs = nowMs() - t0 - buildMs;
  ensureReplicas(s);
  DeviceBvhResult first;
  const int rc = onSceneDevices(s, sceneDeviceCount(s), [&](SceneDevice& D, hipStream_t st) -> int {
    const double ta = nowMs();
    if (uploadSceneTo(s, D, H, st) != GI_C_OK || D.dTris.upload(tris, st) || D.dTriFaceId.upload(faceIdOf, st)) return GI_C_ERROR;
    HIP_TRY(hipStreamSynchronize(st));
    const double tb = nowMs();
    DeviceBvhResult r;
    const int built = buildBvh8Device(st, D.dTris.ptr, D.dTriFaceId.ptr, n, kMaxBvhDepth, r);
    uploadMs += tb - ta; buildMs += nowMs() - tb;
    if (built == DEVICE_BVH_OUT_OF_MEMORY || built == DEVICE_BVH_TOO_DEEP) {
      if (timing || built == DEVICE_BVH_TOO_DEEP) fprintf(stderr, "[gatling_gi] device BVH build on device %u: %s; the host builder takes over\n", D.slot,
          built == DEVICE_BVH_TOO_DEEP ? "the tree is deeper than the traversal stack (49 levels)" : "out of device memory");
      for (uint32_t k = 0; k <= D.slot; k++) sceneDevice(s, k).dNodes.release(); // (no tree of the wrong shape left behind)
      H.deviceBuilt = false; H.triShade.clear();
      return DEVICE_BUILD_FALLBACK;
    }
    if (built != DEVICE_BVH_OK) { setError(std::string("device BVH build failed: ") + r.error); return GI_C_ERROR; }
    D.dNodes.release(); D.dNodes.ptr = r.nodes; D.dNodes.count = r.nodeCount;
    if (D.slot == 0) first = r;
    else if (r.nodeCount != first.nodeCount || r.maxDepth != first.maxDepth) { setError("internal: device BVH builds differ between devices"); return GI_C_ERROR; }
    if (timing) fprintf(stderr, "[gatling_gi] device bvh8 (device %u): boxes %.1f ms, sort %.1f ms, PLOC + collapse DP %.1f ms (%u passes; the DP is filled by "
                                "the merge kernel), emission %.1f ms (%u levels, %u nodes, %u active of %u triangles)\n", D.slot, r.ms[0], r.ms[1], r.ms[2],
                        r.plocIterations, r.ms[3], r.maxDepth, r.nodeCount, r.activeTris, n);
    return GI_C_OK;
  });
  if (rc != GI_C_OK) return rc;
  if (first.activeTris != n - inactive) { setError("internal: device and host disagree on the inactive triangles"); return GI_C_ERROR; }
  s->stats.inactiveTriangleCount = inactive;
  if (inactive) warnInactive(H.meshBuilds, perMesh);
  H.bvh = Bvh8{}; H.bvh.maxDepth = first.maxDepth; H.bvh.activeTris = first.activeTris; H.bvh.levelStart = first.levelStart;
  H.triFaceId.clear(); H.flatOfOrig.clear();
  return finishBuild(s, hostPtr, first.nodeCount, n, std::vector<Node8>{first.root}, buildMs, uploadMs, " (device build)");
}

// GI_C_SCENE_OPTION_TLAS_ONLY / GATLING_OPTIONS=tlas_only: a scene that wants the two-level layout is built without the flat tree (buildSceneTreeless below)
bool tlasOnlyWanted(const GiCScene* s)
{
  const long o = optionValue("tlas_only", -1);
  return o >= 0 ? o == 1 : s->optTlasOnly == 1;
}
// GI_C_SCENE_OPTION_LEAF_LIFT / GATLING_OPTIONS=leaf_lift: the flat tree of a small scene goes through liftLeafSlots (buildScene below; default on)
bool leafLiftWanted(const GiCScene* s)
{
  const long o = optionValue("leaf_lift", -1);
  return o >= 0 ? o == 1 : (s->optLeafLift < 0 ? LEAF_LIFT_DEFAULT != 0 : s->optLeafLift == 1);
}
// is the two-level layout wanted for a scene of `flatTris` flattened triangles, before any flat tree exists?  buildTwoLevel's rules but the one on node bytes,
// which needs that tree
static bool twoLevelWantedWithoutTree(const GiCScene* s, size_t flatTris)
{
  const long want = optionValue("two_level", s->optTwoLevel);
  return want > 0 || (want < 0 && flatTris >= ((size_t)1 << 26));
}

// buildScene's route for two-level scenes without the flat tree (GI_C_SCENE_OPTION_TLAS_ONLY): the TLAS and the BLASes are built over the meshes, the flat
// RECORDS are the flattening loop's, in scene order (origId == index: flatOfOrig is the identity, the face ids are faceIdOf), and no flat node is built, sent
// or kept.  The caller has established: the option and the layout are wanted, more than LDS_TRIS triangles, none of them inactive.  DEVICE_BUILD_FALLBACK:
// buildTwoLevel declined (it has said why) and nothing was changed -- buildScene goes on as without the option.
static int buildSceneTreeless(GiCScene* s, std::unique_ptr<SceneHost>& hostPtr, std::vector<TriRec>& tris, std::vector<int32_t>& faceIdOf, double t0)
{
  SceneHost& H = *hostPtr;
  if (buildTwoLevel(s, H.meshBuilds, H.instances, tris.size(), 0u, H.two, true) != GI_C_OK) return GI_C_ERROR;
  if (!s->twoLevel) { H.two = TwoLevelHost{}; return DEVICE_BUILD_FALLBACK; }
  if (tris.size() >= (1u << 28)) {
    setError("scene has 2^28 or more triangles after instancing: the hit record packs (triangle, material class) into 32 bits");
    return GI_C_ERROR;
  }
  const uint32_t n = (uint32_t)tris.size();
  s->stats.inactiveTriangleCount = 0u;
  H.treeless = true;
  H.bvh = Bvh8{}; H.bvh.maxDepth = 1u; H.bvh.activeTris = n;
  H.flatOfOrig.resize(n);
  for (uint32_t i = 0; i < n; i++) H.flatOfOrig[i] = i;
  const double t1 = nowMs();
  // beyond LDS by construction: shading records, and TriRec::vi[0] names the triangle's record
  H.shadePacked = true; H.triShade.clear(); H.triGeomNormal.clear();
  const std::vector<uint32_t> shadeBaseOfMesh = buildShadeRecords(H);
  for (TriRec& t : tris) t.vi[0] = shadeBaseOfMesh[H.instances[t.instance].mesh] + t.prim;
  H.bvh.tris.swap(tris); H.triFaceId.swap(faceIdOf);
  ensureReplicas(s);
  if (onSceneDevices(s, sceneDeviceCount(s), [&](SceneDevice& D, hipStream_t st) { return uploadSceneTo(s, D, H, st); }) != GI_C_OK) return GI_C_ERROR;
  const int rc = finishBuild(s, hostPtr, 0u, n, std::vector<Node8>{}, t1 - t0, nowMs() - t1, " (two-level, no flat tree)");
  setSceneBoundsFromInstances(s, *s->host);
  return rc;
}

int buildScene(GiCScene* s)
{
  double t0 = nowMs();
  std::unique_ptr<SceneHost> hostPtr(new SceneHost());
  SceneHost& H = *hostPtr;
  s->host.reset(); // (a failed build leaves no stale host copy behind)
  s->liftedLeafSlots = 0u; // (giCDebugSceneLeafLift: what this build's tree got; only the host-built flat tree below is offered to the pass)
  for (GiCMesh* m : s->retiredMeshes) delete m; // (nothing refers to them any more: updateTopology kept them for the host copy that is gone)
  s->retiredMeshes.clear();
  for (GiCMesh* m : s->meshes) { m->builtInstances = 0xffffffffu; m->xformDirty = false; m->instDirty.clear(); m->visToggled = false; m->vertsEdited = false;
      m->instEdited = false; }
  std::vector<FVertex>& verts = H.verts; std::vector<InstanceRec>& instances = H.instances; std::vector<TriRec> tris; std::vector<int32_t> faceIdOf;
  buildMaterialRecords(s, H.mats);
  uint32_t meshIdx = 0;
  std::vector<MeshBuild>& meshBuilds = H.meshBuilds; // visible meshes in scene order (two-level layout, incremental updates)
  std::vector<MeshRec>& meshRecs = H.meshRecs; std::vector<float>& sceneData = H.sceneData;
  size_t upper = 0; // one allocation for the flattened triangles (an upper bound: a visible mesh may yet be left out)
  for (const GiCMesh* m : s->meshes) if (m->visible) upper += m->faces.size() * (m->instanceTransforms.size() / 16);
  tris.reserve(upper); faceIdOf.reserve(upper);
  for (GiCMesh* m : s->meshes) {
    if (!m->visible) continue; // Gi.cpp:801-804
    if (m->faces.empty()) continue;
    auto mit = std::find(s->materials.begin(), s->materials.end(), m->material);
    if (mit == s->materials.end()) { fprintf(stderr, "[gatling_gi] invalid BLAS material for mesh %s\n", m->name.c_str()); continue; } // Gi.cpp:818-822
    const uint32_t material = (uint32_t)(mit - s->materials.begin());
    if (material > 0x00ffffffu) { setError("too many materials"); return GI_C_ERROR; }
    const uint32_t matFlags = meshMatFlags(H.mats[material], material, m);
    const uint32_t vertexOffset = (uint32_t)verts.size();
    appendMeshSceneData(m, *mit, vertexOffset, meshRecs, sceneData);
    for (const GiCVertex& vIn : m->vertices) verts.push_back(packVertex(vIn));
    const std::vector<int32_t> meshFaceIdAov = faceIdAovOf(m);
    size_t instCount = m->instanceTransforms.size() / 16;
    m->builtInstances = (uint32_t)instCount;
    meshBuilds.push_back(MeshBuild{m, vertexOffset, matFlags, (uint32_t)instances.size(), (uint32_t)instCount, (uint32_t)tris.size(), meshIdx, meshFaceIdAov});
    meshBuilds.back().idBase = meshBuilds.back().triFirst; meshBuilds.back().numberInstances();
    const size_t nf = m->faces.size(), first = tris.size();
    tris.resize(first + instCount * nf);
    for (size_t ii = 0; ii < instCount; ii++) {
      const uint32_t instIdx = (uint32_t)instances.size(), idBase = (uint32_t)(first + ii * nf);
      instances.push_back(makeInstanceRec(m, meshIdx, ii));
      flattenInstance(instances.back(), instIdx, m, vertexOffset, matFlags, idBase, NOT_PACKED, &tris[idBase]); // (packed or not is known once the BVH is built)
      faceIdOf.insert(faceIdOf.end(), meshFaceIdAov.begin(), meshFaceIdAov.end());
    }
    meshIdx++;
  }
  { // the device builder (GI_C_SCENE_OPTION_BVH_BUILD / device_build): scenes that take the flat layout and do not fit LDS.  (Fewer triangles than 2^32 / 80
    // bytes: the automatic two-level rules below cannot apply -- an 8-wide tree has fewer nodes than triangles.)
    const long want = optionValue("device_build", -1);
    const bool device = (want < 0 ? s->optBvhBuild == 1 : want == 1) && tris.size() > 128u && optionValue("two_level", s->optTwoLevel) <= 0
        && tris.size() * sizeof(Node8) < ((size_t)1 << 32);
    if (device) {
      const int rc = buildSceneOnDevice(s, hostPtr, tris, faceIdOf, t0);
      if (rc != DEVICE_BUILD_FALLBACK) return rc;
    }
  }
  // two-level scenes without the flat tree (GI_C_SCENE_OPTION_TLAS_ONLY / tlas_only): read only when the layout is wanted, for scenes beyond LDS (more than
  // LDS_TRIS triangles; a smaller scene could be LDS-resident) without inactive triangles.  A decline of buildTwoLevel falls through to the flat build
  if (tlasOnlyWanted(s) && twoLevelWantedWithoutTree(s, tris.size()) && !instances.empty() && !sceneFitsLds(0u, tris.size())) {
    std::vector<uint32_t> perMesh;
    if (countInactive(tris, H, perMesh) == 0u) {
      const int rc = buildSceneTreeless(s, hostPtr, tris, faceIdOf, t0);
      if (rc != DEVICE_BUILD_FALLBACK) return rc;
    }
  }
  Bvh8& bvh = H.bvh;
  buildBvh8(tris, bvh);
  { std::vector<TriRec>().swap(tris); } // the BVH holds its own (leaf-ordered) copy
  s->stats.inactiveTriangleCount = (uint32_t)bvh.tris.size() - bvh.activeTris;
  if (bvh.activeTris < bvh.tris.size()) { // one line per mesh (bvh8.h "Inactive items")
    std::vector<uint32_t> perMesh(meshBuilds.size(), 0u);
    for (size_t i = bvh.activeTris; i < bvh.tris.size(); i++) perMesh[instances[bvh.tris[i].instance].mesh]++;
    warnInactive(meshBuilds, perMesh);
  }
  if (buildTwoLevel(s, meshBuilds, instances, bvh.tris.size(), bvh.nodes.size(), H.two, true) != GI_C_OK) return GI_C_ERROR;
  // Leaf lift (leaf_lift.cpp; GI_C_SCENE_OPTION_LEAF_LIFT / GATLING_OPTIONS=leaf_lift, default on): the flat tree of a scene the fused kernel walks out of LDS
  // -- LDS-resident, not two-level, a root and one level below it -- hands leaf slots that stretch a child's box to free slots of the root.  Before anything
  // is derived from the triangle order (flatOfOrig, triFaceId, triGeomNormal below).  Scenes this small rebuild on every geometry edit (kIncrementalMinTris),
  // so the pass reruns with them and no edit in place ever meets a lifted tree.
  if (leafLiftWanted(s) && !s->twoLevel && sceneFitsLds(bvh.nodes.size(), bvh.tris.size())) s->liftedLeafSlots = liftLeafSlots(bvh);
  if (s->twoLevel) {
    H.flatOfOrig.resize(bvh.tris.size());
    for (size_t i = 0; i < bvh.tris.size(); i++) H.flatOfOrig[bvh.tris[i].origId] = (uint32_t)i;
  }
  double t1 = nowMs();
  if (bvh.maxDepth > kMaxBvhDepth) { setError("scene BVH is deeper than the traversal stack (49 levels): degenerate geometry (long chains of nested splits)");
      return GI_C_ERROR; }
  if (bvh.tris.size() >= (1u << 26) && !s->twoLevel) {
    setError("scene has 2^26 or more triangles after instancing and no two-level layout (it is switched off, or its unique mesh triangles exceed 2^26 too): "
             "the traversal queues pack (lane, triangle) into 32 bits");
    return GI_C_ERROR;
  }
  if (bvh.tris.size() >= (1u << 28)) {
    setError("scene has 2^28 or more triangles after instancing: the hit record packs (triangle, material class) into 32 bits");
    return GI_C_ERROR;
  }
  H.triFaceId.resize(bvh.tris.size());
  for (size_t i = 0; i < bvh.tris.size(); i++) H.triFaceId[i] = faceIdOf[bvh.tris[i].origId];
  // Scenes beyond LDS: one 160-byte shading record per mesh triangle (gi_types.h TriShade); the flattened triangles name theirs in vi[0].  LDS-resident
  // scenes keep vertex indices there: the fused kernels are VALU-bound and read the host-decoded FVertex records.
  H.shadePacked = !sceneFitsLds(bvh.nodes.size(), bvh.tris.size());
  H.triShade.clear();
  if (H.shadePacked) {
    const std::vector<uint32_t> shadeBaseOfMesh = buildShadeRecords(H);
    for (TriRec& t : bvh.tris) t.vi[0] = shadeBaseOfMesh[instances[t.instance].mesh] + t.prim;
  }
  // LDS-resident scenes (the fused kernels' and k_trace's shading path reads FVertex records): the world-space geometric normal of every flattened triangle,
  // made here with setup_shading_state's operations in its order (mdl_shading_state.glsl:27-28: normalize(cross(pb - pa, pc - pa)) in object space, the normal
  // transform, normalize again) -- two normalisations, a cross product and a transform per hit that depend on nothing but the triangle.  Same bits: IEEE + - *
  // / sqrt without contraction on both sides, as for the decoded FVertex normals.
  H.triGeomNormal.clear();
  if (!H.shadePacked) {
    H.triGeomNormal.resize(bvh.tris.size());
    auto normalize3 = [](float* a) { const float inv = 1.0f / sqrtf((a[0] * a[0] + a[1] * a[1]) + a[2] * a[2]); a[0] = a[0] * inv; a[1] = a[1] * inv;
        a[2] = a[2] * inv; };
    for (size_t i = 0; i < bvh.tris.size(); i++) {
      const TriRec& t = bvh.tris[i];
      const float* pa = verts[t.vi[0]].pos; const float* pb = verts[t.vi[1]].pos; const float* pc = verts[t.vi[2]].pos;
      const float e1[3] = {pb[0] - pa[0], pb[1] - pa[1], pb[2] - pa[2]}, e2[3] = {pc[0] - pa[0], pc[1] - pa[1], pc[2] - pa[2]};
      float g[3] = {e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]};
      normalize3(g);
      const float* w = instances[t.instance].w2o;
      float n[3] = {(g[0] * w[0] + g[1] * w[3]) + g[2] * w[6], (g[0] * w[1] + g[1] * w[4]) + g[2] * w[7], (g[0] * w[2] + g[1] * w[5]) + g[2] * w[8]};
      normalize3(n);
      H.triGeomNormal[i] = F4{n[0], n[1], n[2], 0.0f};
    }
  }
  ensureReplicas(s);
  if (onSceneDevices(s, sceneDeviceCount(s), [&](SceneDevice& D, hipStream_t st) { return uploadSceneTo(s, D, H, st); }) != GI_C_OK) return GI_C_ERROR;
  return finishBuild(s, hostPtr, (uint32_t)bvh.nodes.size(), (uint32_t)bvh.tris.size(), bvh.nodes, t1 - t0, nowMs() - t1, "");
}

// ---------------------------------------------------------------------------------------------------------------
// Incremental transform updates (the reference keeps every mesh's BLAS and rebuilds only the TLAS, Gi.cpp:1180-1202).
//
// A scene is first built as ONE tree over all instanced triangles (buildScene: the best tree).  The first time only transforms change, it is re-laid out
// PARTITIONED: every flattened mesh instance gets its own subtree in its own node range and keeps its triangles in its own (scene-order) range; a top tree
// over the subtree roots (buildTopBvh8: the roots are copied in as ordinary internal children) makes it one ordinary BVH8 again -- the traversal kernels, the
// shading code and the triangle ids do not change, so images stay bit-identical to a full rebuild (traversal contract: results do not depend on the tree).
// From then on moving an instance costs: its triangles re-transformed, its subtree rebuilt (a few thousand triangles), the top tree rebuilt (one item per
// instance), and those ranges uploaded -- not a 10 M-triangle SAH build and a 0.7 GB upload.  Material, assignment, texture and primvar edits have a path of
// their own (updateMaterials below) that leaves the tree alone, partitioned or not, and so have -- opt-in -- visibility edits (updateVisibility below: ids
// renumbered in place; a partitioned tree leaves the parts of hidden meshes out of its top tree), vertex edits (updateVertices: a refit) and mesh creations
// and destructions (updateTopology: parts appended and retired) and instance counts and ids of a built mesh (updateTopology as well: instances appended,
// cloned and retired).  Any other edit (a show of a mesh that was invisible at the build, and the opt-in kinds without their option) raises DIRTY_BVH and the
// next render rebuilds everything as one tree again.
// ---------------------------------------------------------------------------------------------------------------
void nodeBounds(const Node8& n, float box[6])
{
  for (int a = 0; a < 3; a++) { box[a] = 3.0e38f; box[3 + a] = -3.0e38f; }
  for (int sl = 0; sl < 8; sl++) {
    if (n.meta[sl] == 0) continue;
    for (int a = 0; a < 3; a++) {
      uint32_t eb = (uint32_t)n.e[a] << 23; float scale; memcpy(&scale, &eb, 4);
      box[a] = std::min(box[a], n.p[a] + (float)n.qlo[a][sl] * scale); box[3 + a] = std::max(box[3 + a], n.p[a] + (float)n.qhi[a][sl] * scale);
    }
  }
  // the dequantised planes are evaluated in fp32 here and with an fma on the device: one more ulp-scale pad keeps the item box outside both
  for (int a = 0; a < 3; a++) { const float pad = (std::fabs(box[a]) + std::fabs(box[3 + a])) * 2.4e-7f + 1.0e-30f; box[a] -= pad; box[3 + a] += pad; }
}

// One instance's InstanceRec, world-space triangles (scene order) and subtree
struct PartBuild { InstanceRec inst; Bvh8 bvh; };
void buildPart(const MeshBuild& mb, uint32_t instInMesh, bool packed, PartBuild& out)
{
  out.inst = makeInstanceRec(mb.m, mb.meshIdx, instInMesh);
  std::vector<TriRec> tris(mb.m->faces.size());
  // (ids from 0: placePart adds the instance's base)
  flattenInstance(out.inst, mb.inst[instInMesh], mb.m, mb.vertexOffset, mb.matFlags, 0u, packed ? mb.shadeBase : NOT_PACKED, tris.data());
  buildBvh8(tris, out.bvh);
}

// writes a built part into the scene arrays at the part's ranges (node / triangle indices rebased to absolute)
void placePart(SceneHost& H, InstPart& P, const PartBuild& B)
{
  const MeshBuild& mb = H.meshBuilds[P.meshBuild];
  P.nodeCount = (uint32_t)B.bvh.nodes.size(); P.depth = B.bvh.maxDepth; P.activeTris = B.bvh.activeTris; P.levelStart = B.bvh.levelStart;
  for (uint32_t i = 0; i < P.nodeCount; i++) { Node8 n = B.bvh.nodes[i]; n.childBase += P.nodeOff; n.triBase += P.triFirst; H.bvh.nodes[P.nodeOff + i] = n; }
  for (uint32_t k = 0; k < P.nf; k++) {
    TriRec t = B.bvh.tris[k];
    H.triFaceId[P.triFirst + k] = mb.faceIdAov[t.prim];
    // scene-order id: the instance's triangles are numbered in face order, as in buildScene -- from triFirst, or from where a fresh build of the visible
    // meshes would start it once meshes in front of it are hidden (updateVisibility)
    t.origId += mb.idBase + P.instInMesh * P.nf;
    H.bvh.tris[P.triFirst + k] = t;
  }
  H.instances[mb.inst[P.instInMesh]] = B.inst;
  nodeBounds(H.bvh.nodes[P.nodeOff], P.box);
}

template <class Fn> void parallelOver(size_t n, Fn&& fn)
{
  int workers = (int)std::thread::hardware_concurrency();
  if (const char* e = getenv("GATLING_BUILD_THREADS")) workers = atoi(e);
  workers = (int)std::min<size_t>((size_t)std::min(std::max(workers, 1), 32), std::max<size_t>(n, 1));
  if (workers <= 1) { for (size_t i = 0; i < n; i++) fn(i); return; }
  std::atomic<size_t> next{0};
  std::vector<std::thread> th;
  for (int w = 0; w < workers; w++) th.emplace_back([&] { for (size_t i; (i = next.fetch_add(1)) < n;) fn(i); });
  for (auto& t : th) t.join();
}

int rebuildTop(GiCScene* s, SceneHost& H)
{
  std::vector<float> boxes(H.parts.size() * 6); std::vector<Node8> roots(H.parts.size());
  uint32_t subDepth = 0;
  for (size_t i = 0; i < H.parts.size(); i++) { memcpy(&boxes[6 * i], H.parts[i].box, 24); roots[i] = H.bvh.nodes[H.parts[i].nodeOff];
      subDepth = std::max(subDepth, H.parts[i].depth);
      // the parts of a hidden mesh (updateVisibility) and of a retired instance (updateTopology) keep their ranges and stay out of the top tree, like a part
      // whose triangles are all inactive
      if (H.meshBuilds[H.parts[i].meshBuild].hidden || H.parts[i].retired) for (int a = 0; a < 3; a++) { boxes[6 * i + a] = 3.0e38f; boxes[6 * i + 3 + a] = -3.0e38f; } }
  Bvh8 top;
  buildTopBvh8(boxes.data(), H.parts.size(), roots.data(), top);
  if (top.nodes.size() > H.topCap) { setError("internal: top tree larger than its reserved range"); return GI_C_ERROR; }
  std::copy(top.nodes.begin(), top.nodes.end(), H.bvh.nodes.begin());
  for (size_t i = top.nodes.size(); i < H.topCap; i++) memset(&H.bvh.nodes[i], 0, sizeof(Node8));
  H.bvh.maxDepth = top.maxDepth + (subDepth > 0u ? subDepth - 1u : 0u); // the copied roots are the subtrees' first level
  if (H.bvh.maxDepth > kMaxBvhDepth) { setError("scene BVH is deeper than the traversal stack (49 levels)"); return GI_C_ERROR; }
  s->bvhDepth = H.bvh.maxDepth > 1u ? H.bvh.maxDepth - 1u : 1u;
  return GI_C_OK;
}

struct UpdateCost { double buildMs = 0.0, uploadMs = 0.0; }; // what an update spent on host-side tree building, and on everything else (syncSceneGeometry)
// The host copy of a scene that may be edited in place, or null: no host copy, or GATLING_OPTIONS=incremental=0.  (The floor of kIncrementalMinTris triangles
// stays with each update: what it counts differs -- the resident triangles, or for a visibility edit the visible ones.)
static SceneHost* incrementalHost(GiCScene* s) { return optionValue("incremental", 1) ? s->host.get() : nullptr; }

// The one-time re-layout of a flat scene (host-built, device-built or with its host tree dropped): every instance its own subtree + ranges (costs about one
// full build, in parallel over the instances).  updateTransforms and updateTopology.  False: the scene has no instance, nothing was done; true: the host
// copy is partitioned and host-built from here on, and the caller sends every array (uploadSceneTo).  With topology updates wanted the top range is twice
// what the parts need: appended parts find room there.
static bool relayoutPartitioned(GiCScene* s, SceneHost& H)
{
  std::vector<InstPart> parts;
  for (uint32_t b = 0; b < (uint32_t)H.meshBuilds.size(); b++) {
    const MeshBuild& mb = H.meshBuilds[b];
    const uint32_t nf = (uint32_t)mb.m->faces.size();
    // (the live instances: all of them, unless an instance update has just retired the last ones of a flat scene -- those keep a part without a subtree)
    for (uint32_t ii = 0; ii < (uint32_t)mb.inst.size() + mb.retiredInst; ii++) { InstPart P{}; P.meshBuild = b; P.instInMesh = ii; P.triFirst = mb.triFirst + ii * nf;
        P.nf = nf; P.retired = ii >= (uint32_t)mb.inst.size(); parts.push_back(P); }
  }
  if (parts.empty()) return false;
  // (a device-built tree has no host copy, and a vertex update dropped that of a host-built one: placePart fills them)
  if (H.deviceBuilt || H.hostTreeDropped) { H.bvh.tris.resize(s->triCount); H.triFaceId.resize(s->triCount); H.hostTreeDropped = false; }
  std::vector<PartBuild> built(parts.size());
  parallelOver(parts.size(), [&](size_t i) { if (!parts[i].retired) buildPart(H.meshBuilds[parts[i].meshBuild], parts[i].instInMesh, H.shadePacked, built[i]); });
  H.topCap = (uint32_t)parts.size() * 2u + 16u; // top nodes <= internal top nodes + one copied root per part
  if (topologyUpdatesWanted(s)) H.topCap *= 2u;
  uint32_t off = H.topCap;
  for (size_t i = 0; i < parts.size(); i++) { const uint32_t n = (uint32_t)built[i].bvh.nodes.size(); parts[i].nodeOff = off;
      parts[i].nodeCap = n + n / 4u + 8u; off += parts[i].nodeCap; }
  H.bvh.nodes.assign(off, Node8{});
  H.parts.swap(parts);
  parallelOver(H.parts.size(), [&](size_t i) {
    InstPart& P = H.parts[i];
    if (!P.retired) { placePart(H, P, built[i]); return; }
    // no subtree: unhittable records that nothing refers to, an empty box (nodeOff names the first part's root, never read through this part)
    for (uint32_t k = 0; k < P.nf; k++) { TriRec t{}; t.prim = k; H.bvh.tris[P.triFirst + k] = t; H.triFaceId[P.triFirst + k] = 0; }
    P.nodeOff = H.topCap; P.nodeCount = 0; P.nodeCap = 0; P.depth = 0;
    for (int a = 0; a < 3; a++) { P.box[a] = 3.0e38f; P.box[3 + a] = -3.0e38f; }
  });
  H.partitioned = true; H.deviceBuilt = false; // host-built from here on
  return true;
}

// GI_C_SCENE_OPTION_TLAS_UPDATES / GATLING_OPTIONS=tlas_updates: transform edits of a two-level scene are applied in place (updateTransformsTwoLevel below)
bool tlasUpdatesWanted(const GiCScene* s)
{
  const long o = optionValue("tlas_updates", -1);
  return o >= 0 ? o == 1 : s->optTlasUpdates == 1;
}
static int updateTransformsTwoLevel(GiCScene* s, SceneHost& H, bool& handled, UpdateCost& cost);

// handled true: done incrementally; left false: the caller must run a full buildScene (not an error)
static int updateTransforms(GiCScene* s, bool& handled, UpdateCost& cost)
{
  SceneHost* host = incrementalHost(s);
  if (host && s->twoLevel && tlasUpdatesWanted(s)) return updateTransformsTwoLevel(s, *host, handled, cost);
  if (!host || s->twoLevel || s->triCount < kIncrementalMinTris) return GI_C_OK; // (the floor: resident triangles)
  SceneHost& H = *host;
  for (const MeshBuild& mb : H.meshBuilds) if (mb.m->builtInstances != mb.instCount) return GI_C_OK; // (cannot happen: count changes raise DIRTY_BVH)
  const double t0 = nowMs();
  std::vector<uint32_t> dirtyParts;
  bool converted = false;
  if (!H.partitioned) {
    if (!relayoutPartitioned(s, H)) return GI_C_OK;
    converted = true;
  } else {
    for (uint32_t i = 0; i < (uint32_t)H.parts.size(); i++) {
      const GiCMesh* m = H.meshBuilds[H.parts[i].meshBuild].m;
      if (m->xformDirty && !H.parts[i].retired && (m->instDirty.empty() || m->instDirty[H.parts[i].instInMesh])) dirtyParts.push_back(i);
    }
    std::vector<PartBuild> built(dirtyParts.size());
    parallelOver(dirtyParts.size(),
        [&](size_t k) { const InstPart& P = H.parts[dirtyParts[k]]; buildPart(H.meshBuilds[P.meshBuild], P.instInMesh, H.shadePacked, built[k]); });
    for (size_t k = 0; k < dirtyParts.size(); k++)
      // a subtree outgrew its range (rare): full rebuild
      if (built[k].bvh.nodes.size() > H.parts[dirtyParts[k]].nodeCap) { H.partitioned = false; H.parts.clear(); return GI_C_OK; }
    parallelOver(dirtyParts.size(), [&](size_t k) { placePart(H, H.parts[dirtyParts[k]], built[k]); });
  }
  if (rebuildTop(s, H) != GI_C_OK) return GI_C_ERROR;
  for (GiCMesh* m : s->meshes) { m->xformDirty = false; m->instDirty.clear(); }
  const double t1 = nowMs();
  // --- upload: everything after the re-layout, else the moved parts' ranges, their InstanceRecs and the top region
  s->nodeCount = (uint32_t)H.bvh.nodes.size();
  setSceneBounds(s, H.bvh.nodes);
  if (onSceneDevices(s, residentDeviceCount(s), [&](SceneDevice& D, hipStream_t st) -> int {
    if (converted) return uploadSceneTo(s, D, H, st);
    if (uploadTopTree(D, H, st) != GI_C_OK) return GI_C_ERROR;
    for (uint32_t i : dirtyParts) {
      const InstPart& P = H.parts[i];
      const uint32_t instIdx = H.meshBuilds[P.meshBuild].inst[P.instInMesh];
      HIP_TRY(hipMemcpyAsync(D.dNodes.ptr + P.nodeOff, &H.bvh.nodes[P.nodeOff], (size_t)P.nodeCount * sizeof(Node8), hipMemcpyHostToDevice, st));
      HIP_TRY(hipMemcpyAsync(D.dTris.ptr + P.triFirst, &H.bvh.tris[P.triFirst], (size_t)P.nf * sizeof(TriRec), hipMemcpyHostToDevice, st));
      HIP_TRY(hipMemcpyAsync(D.dTriFaceId.ptr + P.triFirst, &H.triFaceId[P.triFirst], (size_t)P.nf * sizeof(int32_t), hipMemcpyHostToDevice, st));
      HIP_TRY(hipMemcpyAsync(D.dInstances.ptr + instIdx, &H.instances[instIdx], sizeof(InstanceRec), hipMemcpyHostToDevice, st));
    }
    HIP_TRY(hipStreamSynchronize(st));
    return GI_C_OK;
  }) != GI_C_OK) return GI_C_ERROR;
  cost.buildMs = t1 - t0; cost.uploadMs = nowMs() - t1;
  if (getenv("GATLING_BUILD_TIMING")) fprintf(stderr, "[gatling_gi] transform update: %s, %zu part(s) rebuilt of %zu, host %.1f ms, upload %.1f ms\n",
                                              converted ? "scene re-laid out as per-instance subtrees" : "incremental", converted
                                                  ? H.parts.size() : dirtyParts.size(), H.parts.size(), cost.buildMs, cost.uploadMs);
  handled = true;
  return GI_C_OK;
}

// ---------------------------------------------------------------------------------------------------------------
// Incremental material updates.  An edit of a material, a material assignment, a texture binding or a primvar changes no vertex, box or triangle id: the
// MaterialRec table, the texture table, the per-mesh scene data and ONE word per flattened triangle (TriRec::matFlags) change, and the scene flags derived
// from them.  The small arrays are rebuilt by the functions buildScene uses and re-sent whole; the word is patched where it lives, in device memory
// (gi_patch.hip k_patch_mat_flags) -- a device-built scene keeps no host copy of its triangles, and re-sending them would be the full upload again.
// Covered: the flat layout in all its forms (host-built, device-built, partitioned) and the two-level layout (same flat triangles + InstTrav::matFlags, one
// record per instance, re-sent).  Falls back to buildScene (handled = false, not an error): no host copy of the scene, fewer than kIncrementalMinTris
// triangles (as updateTransforms), GATLING_OPTIONS=incremental=0, or the set of meshes in the scene changes -- a mesh that was left out for an invalid material gets a
// valid one or the reverse (the scene-order ids of every later triangle shift).
// ---------------------------------------------------------------------------------------------------------------
static int updateMaterials(GiCScene* s, bool& handled, UpdateCost& cost)
{
  SceneHost* host = incrementalHost(s);
  if (!host || s->triCount < kIncrementalMinTris) return GI_C_OK; // (the floor: resident triangles)
  SceneHost& H = *host;
  const double t0 = nowMs();
  if (!H.reordered) { // the same meshes, in the same order, as the built scene holds?
    size_t b = 0;
    // (a retired mesh -- destroyed, its records still resident until the next build: updateTopology -- is no longer among s->meshes)
    auto skipRetired = [&] { while (b < H.meshBuilds.size() && H.meshBuilds[b].m->retired) b++; };
    for (const GiCMesh* m : s->meshes) {
      skipRetired();
      // (a mesh hidden by updateVisibility is still part of the resident scene: its word is patched like any other)
      const bool hiddenInScene = b < H.meshBuilds.size() && H.meshBuilds[b].m == m && H.meshBuilds[b].hidden;
      const bool inScene = (m->visible || hiddenInScene) && !m->faces.empty() && std::find(s->materials.begin(), s->materials.end(), m->material) != s->materials.end();
      if (inScene != (m->builtInstances != 0xffffffffu)) return GI_C_OK;
      if (!inScene) continue;
      if (b >= H.meshBuilds.size() || H.meshBuilds[b].m != m || H.meshBuilds[b].instCount != m->builtInstances) return GI_C_OK;
      b++;
    }
    skipRetired();
    if (b != H.meshBuilds.size() || H.meshRecs.size() != H.meshBuilds.size()) return GI_C_OK;
  } else { // a mesh adopted the records of the one it replaced (updateTopology adoptResyncs): the same meshes, each found by its handle
    std::unordered_map<const GiCMesh*, size_t> buildOf;
    size_t retired = 0, found = 0;
    for (size_t b = 0; b < H.meshBuilds.size(); b++) { if (H.meshBuilds[b].m->retired) retired++; else buildOf[H.meshBuilds[b].m] = b; }
    for (const GiCMesh* m : s->meshes) {
      const auto it = buildOf.find(m);
      const bool hiddenInScene = it != buildOf.end() && H.meshBuilds[it->second].hidden;
      const bool inScene = (m->visible || hiddenInScene) && !m->faces.empty() && std::find(s->materials.begin(), s->materials.end(), m->material) != s->materials.end();
      if (inScene != (m->builtInstances != 0xffffffffu)) return GI_C_OK;
      if (!inScene) continue;
      if (it == buildOf.end() || H.meshBuilds[it->second].instCount != m->builtInstances) return GI_C_OK;
      found++;
    }
    if (found + retired != H.meshBuilds.size() || H.meshRecs.size() != H.meshBuilds.size()) return GI_C_OK;
  }
  if (s->materials.size() > 0x01000000u) { setError("too many materials"); return GI_C_ERROR; }
  // --- host: material records, scene data, every mesh's word, the scene's class masks
  buildMaterialRecords(s, H.mats);
  std::vector<MeshRec> meshRecs; std::vector<float> sceneData;
  std::vector<uint32_t> wordOfMesh(H.meshBuilds.size(), 0u);
  std::vector<uint8_t> changed(H.meshBuilds.size(), 0);
  uint32_t meshesChanged = 0; uint64_t trisPatched = 0;
  for (MeshBuild& mb : H.meshBuilds) {
    // a retired mesh is hidden for good and its material may be gone: it keeps its word (never read: no ray reaches its triangles) and an empty record
    appendBuiltMeshSceneData(mb, meshRecs, sceneData);
    if (mb.m->retired) { wordOfMesh[mb.meshIdx] = mb.matFlags; continue; }
    const uint32_t material = (uint32_t)(std::find(s->materials.begin(), s->materials.end(), mb.m->material) - s->materials.begin());
    const uint32_t word = meshMatFlags(H.mats[material], material, mb.m);
    wordOfMesh[mb.meshIdx] = word;
    if (word != mb.matFlags) { changed[mb.meshIdx] = 1; meshesChanged++; trisPatched += (uint64_t)mb.m->faces.size() * mb.instCount; mb.matFlags = word; }
  }
  H.meshRecs.swap(meshRecs); H.sceneData.swap(sceneData);
  if (meshesChanged) {
    // host copies of the triangles (host-built and partitioned trees, the two-level records): a later transform update uploads from them
    for (TriRec& t : H.bvh.tris) { const uint32_t mesh = H.instances[t.instance].mesh; if (changed[mesh]) t.matFlags = wordOfMesh[mesh]; }
    for (size_t i = 0; i < H.two.instTrav.size(); i++) H.two.instTrav[i].matFlags = wordOfMesh[H.instances[i].mesh];
  }
  deriveSceneClasses(s, H, false);
  const double t1 = nowMs();
  // --- every device of the scene, on its own stream: the small arrays, then the patch kernel
  double textureMs = 0.0, patchMs = 0.0;
  if (onSceneDevices(s, residentDeviceCount(s), [&](SceneDevice& D, hipStream_t st) -> int {
    const double ta = nowMs();
    int rc = uploadTexturesTo(s, D, st);
    const double tb = nowMs();
    if (rc == GI_C_OK && (D.dMaterials.upload(H.mats, st) || D.dMeshes.upload(H.meshRecs, st) || D.dSceneData.upload(H.sceneData, st))) rc = GI_C_ERROR;
    DeviceBuffer<uint32_t> dWords;
    if (rc == GI_C_OK && meshesChanged) {
      if (s->twoLevel && D.dInstTrav.upload(H.two.instTrav, st)) rc = GI_C_ERROR;
      if (rc == GI_C_OK && D.dTris.count < s->triCount) { setError("internal: the device holds fewer triangles than the scene"); rc = GI_C_ERROR; }
      if (rc == GI_C_OK && dWords.upload(wordOfMesh, st)) rc = GI_C_ERROR;
      if (rc == GI_C_OK) launchPatchMatFlags(st, D.dTris.ptr, s->triCount, D.dInstances.ptr, (uint32_t)H.instances.size(), dWords.ptr, (uint32_t)wordOfMesh.size());
    }
    if (rc == GI_C_OK && (hipGetLastError() != hipSuccess || hipStreamSynchronize(st) != hipSuccess)) { setError("material update: device error"); rc = GI_C_ERROR; }
    dWords.release();
    textureMs += tb - ta; patchMs += nowMs() - tb;
    return rc;
  }) != GI_C_OK) return GI_C_ERROR;
  const double t2 = nowMs();
  cost.uploadMs = t2 - t0; // (no tree was built: buildMs stays 0)
  if (getenv("GATLING_BUILD_TIMING")) fprintf(stderr, "[gatling_gi] material update: %u mesh(es) with a new word of %zu, %llu triangle(s) patched, host %.2f ms, "
                                              "device %.2f ms (texture table %.2f ms, other tables + patch kernel %.2f ms)\n", meshesChanged, H.meshBuilds.size(),
                                              (unsigned long long)trisPatched, t1 - t0, t2 - t1, textureMs, patchMs);
  handled = true;
  return GI_C_OK;
}

// ---------------------------------------------------------------------------------------------------------------
// Incremental visibility updates (opt-in: GI_C_SCENE_OPTION_VISIBILITY_UPDATES / GATLING_OPTIONS=visibility_updates=1).  Hiding a mesh of the built scene
// changes no tree, vertex or shading record.  Its triangles must stop being hit, and the triangles of the meshes behind it in scene order get the ids a
// fresh build -- which leaves invisible meshes out (Gi.cpp:801-804) -- would give them: the cutout test hashes that id and the tie-break orders by it.  Both
// are one pass over the resident triangle records (gi_patch.hip k_patch_visibility) driven by a table with one entry per flattened instance.
//   flat layouts (host-built, device-built): the records of a hidden instance get zero edges, which no walk accepts, and are recomputed at the show.  The
//       tree keeps the boxes of the hidden geometry until the next full build: walks still descend into them and reject the triangles.
//   partitioned layout: the parts of a hidden mesh are left out of the top tree (rebuildTop) and their records are left alone; only ids are renumbered.
// MeshBuild::hidden / idBase hold the state; updateTransforms and updateMaterials respect it, so a hide composes with a move and a material edit, before
// the same render too.  Falls back to buildScene (handled = false, not an error): no host copy of the scene, GATLING_OPTIONS=incremental=0, the two-level
// layout without GI_C_SCENE_OPTION_TLAS_VISIBILITY (SceneView::flatOfOrig is indexed by the ids this renumbers: updateVisibilityTwoLevel below), a toggled mesh that is not part of the built scene (it was invisible or had no valid
// material when the scene was built: it has no records on the device), fewer than kIncrementalMinTris visible flattened triangles after the edit (every mesh
// hidden included).  The caller has established that nothing but visibility toggles asked for the rebuild.
// ---------------------------------------------------------------------------------------------------------------
static bool visibilityUpdatesWanted(const GiCScene* s)
{
  const long o = optionValue("visibility_updates", -1);
  return o >= 0 ? o == 1 : s->optVisibilityUpdates == 1;
}

// What a new set of hidden meshes does to the resident records (updateVisibility; updateTopology retires meshes through it): per instance, the id base a fresh
// build of the visible meshes gives it against the one the resident records hold, and what happens to its records.  hide(mb): the mesh is to be hidden.
struct VisibilityPlan { std::vector<VisPatch> patch; std::vector<uint32_t> newBase; std::vector<uint8_t> hide; uint64_t visibleTris = 0;
    uint32_t hides = 0, shows = 0, renumbered = 0; bool launch = false; };
// The built meshes in the order a fresh build meets them: the position in GiCScene::meshes.  That is the order of H.meshBuilds until a mesh adopts the records
// of the one it replaced (updateTopology, SceneHost::reordered): it sits where it was created, its records where the replaced mesh's sat.  Retired meshes
// are no longer in the scene and come last (they are hidden: they take no ids).
static std::vector<uint32_t> sceneOrder(const GiCScene* s, const SceneHost& H)
{
  std::vector<uint32_t> order(H.meshBuilds.size());
  for (uint32_t b = 0; b < (uint32_t)order.size(); b++) order[b] = b;
  if (!H.reordered) return order;
  std::unordered_map<const GiCMesh*, size_t> at;
  for (size_t i = 0; i < s->meshes.size(); i++) at[s->meshes[i]] = i;
  std::vector<size_t> key(order.size());
  for (size_t b = 0; b < key.size(); b++) { const auto it = at.find(H.meshBuilds[b].m); key[b] = it == at.end() ? (size_t)-1 : it->second; }
  std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return key[a] < key[b]; });
  return order;
}
template <class Hide> static bool planVisibility(const GiCScene* s, const SceneHost& H, Hide&& hideOf, VisibilityPlan& P)
{
  P.patch.assign(H.instances.size(), VisPatch{0, VIS_KEEP}); P.newBase.assign(H.meshBuilds.size(), 0u); P.hide.assign(H.meshBuilds.size(), 0);
  for (const uint32_t b : sceneOrder(s, H)) {
    const MeshBuild& mb = H.meshBuilds[b];
    if (mb.m->builtInstances != mb.instCount) return false;
    const bool hide = hideOf(mb);
    P.hide[mb.meshIdx] = hide ? 1 : 0;
    // (the ids of a hidden mesh are never read: they stay what they are until it is shown)
    P.newBase[mb.meshIdx] = hide ? mb.idBase : (uint32_t)P.visibleTris;
    if (!hide) P.visibleTris += (uint64_t)mb.instCount * mb.m->faces.size();
  }
  for (const MeshBuild& mb : H.meshBuilds) {
    const bool hide = P.hide[mb.meshIdx] != 0;
    const int32_t delta = (int32_t)(P.newBase[mb.meshIdx] - mb.idBase);
    // a partitioned tree drops the parts from its top tree: their records stay whole
    const uint32_t action = hide == mb.hidden || H.partitioned ? VIS_KEEP : (hide ? VIS_HIDE : VIS_SHOW);
    if (hide != mb.hidden) { if (hide) P.hides++; else P.shows++; }
    if (delta != 0) P.renumbered++;
    if (delta != 0 || action != VIS_KEEP) { P.launch = true; for (const uint32_t rec : mb.inst) P.patch[rec] = VisPatch{delta, action}; }
  }
  return true;
}
// ... applied to the triangles' host copies where they exist (host-built and partitioned trees; a later transform update uploads from them) and to the state
// the MeshBuilds keep; the device's records take the same table through k_patch_visibility
static void applyVisibilityPlanOnHost(SceneHost& H, const VisibilityPlan& P)
{
  if (P.launch && !H.bvh.tris.empty()) {
    constexpr size_t CHUNK = 65536;
    const size_t n = H.bvh.tris.size();
    parallelOver((n + CHUNK - 1) / CHUNK, [&](size_t c) {
      for (size_t i = c * CHUNK; i < std::min(n, (c + 1) * CHUNK); i++) {
        TriRec& t = H.bvh.tris[i];
        const VisPatch vp = P.patch[t.instance];
        t.origId += (uint32_t)vp.idDelta;
        if (vp.action == VIS_HIDE) for (int a = 0; a < 3; a++) { t.e1[a] = 0.0f; t.e2[a] = 0.0f; }
        else if (vp.action == VIS_SHOW) {
          const InstanceRec& ir = H.instances[t.instance];
          TriRec whole; flattenTriangle(ir, true, H.meshBuilds[ir.mesh].m, t.prim, whole); // (meshBuilds[i].meshIdx == i)
          memcpy(t.e1, whole.e1, 12); memcpy(t.e2, whole.e2, 12);
        }
      }
    });
  }
  for (MeshBuild& mb : H.meshBuilds) { mb.hidden = P.hide[mb.meshIdx] != 0; mb.idBase = P.newBase[mb.meshIdx]; }
}

// GI_C_SCENE_OPTION_TLAS_VISIBILITY / GATLING_OPTIONS=tlas_visibility: visibility edits of a two-level scene are applied in place (updateVisibilityTwoLevel below)
bool tlasVisibilityWanted(const GiCScene* s)
{
  const long o = optionValue("tlas_visibility", -1);
  return o >= 0 ? o == 1 : s->optTlasVisibility == 1;
}
static int updateVisibilityTwoLevel(GiCScene* s, SceneHost& H, bool& handled, UpdateCost& cost);

static int updateVisibility(GiCScene* s, bool& handled, UpdateCost& cost)
{
  SceneHost* host = incrementalHost(s);
  if (host && s->twoLevel && host->shadePacked && tlasVisibilityWanted(s)) return updateVisibilityTwoLevel(s, *host, handled, cost);
  if (!host || s->twoLevel || !host->shadePacked) return GI_C_OK;
  SceneHost& H = *host;
  const double t0 = nowMs();
  for (const GiCMesh* m : s->meshes) if (m->visToggled && m->builtInstances == 0xffffffffu) return GI_C_OK; // no records on the device: showing it rebuilds
  VisibilityPlan plan;
  if (!planVisibility(s, H, [](const MeshBuild& mb) { return !mb.m->visible; }, plan)) return GI_C_OK; // (cannot happen: count changes ask for the rebuild)
  if (plan.visibleTris < kIncrementalMinTris) return GI_C_OK; // (the floor: VISIBLE triangles, what a fresh build of the edited scene would hold)
  const std::vector<VisPatch>& patch = plan.patch;
  const uint64_t visibleTris = plan.visibleTris; const uint32_t hides = plan.hides, shows = plan.shows, renumbered = plan.renumbered; const bool launch = plan.launch;
  applyVisibilityPlanOnHost(H, plan);
  const bool topChanged = H.partitioned && (hides || shows);
  if (topChanged) {
    if (rebuildTop(s, H) != GI_C_OK) return GI_C_ERROR;
    setSceneBounds(s, H.bvh.nodes);
  }
  // words and table of the last sync; a material edit that is due as well runs behind this update and derives the classes itself -- and must: an
  // updateTopology in front of this update has then already replaced H.mats by the current table, which the resident words do not index yet
  if (!(s->dirty & DIRTY_MATERIALS)) deriveSceneClasses(s, H, false);
  const double t1 = nowMs();
  // --- every device of the scene, on its own stream: the table and the patch kernel, the top tree of a partitioned scene.  Nothing when no word changes
  if (onSceneDevices(s, launch || topChanged ? residentDeviceCount(s) : 0u, [&](SceneDevice& D, hipStream_t st) -> int {
    int rc = GI_C_OK;
    DeviceBuffer<VisPatch> dPatch;
    if (D.dTris.count < s->triCount || D.dInstances.count < H.instances.size() || D.dTriShade.count < H.triShade.size() || D.dNodes.count < H.topCap) {
      setError("internal: the device holds less than the scene"); rc = GI_C_ERROR; }
    if (rc == GI_C_OK && topChanged && uploadTopTree(D, H, st) != GI_C_OK) { setError("visibility update: top tree upload failed"); rc = GI_C_ERROR; }
    if (rc == GI_C_OK && launch) {
      if (dPatch.upload(patch, st)) rc = GI_C_ERROR;
      if (rc == GI_C_OK) launchPatchVisibility(st, D.dTris.ptr, s->triCount, D.dInstances.ptr, (uint32_t)H.instances.size(), dPatch.ptr, D.dTriShade.ptr,
          (uint32_t)H.triShade.size());
    }
    if (rc == GI_C_OK && (hipGetLastError() != hipSuccess || hipStreamSynchronize(st) != hipSuccess)) { setError("visibility update: device error"); rc = GI_C_ERROR; }
    dPatch.release();
    return rc;
  }) != GI_C_OK) return GI_C_ERROR;
  const double t2 = nowMs();
  cost.uploadMs = t2 - t0; // (no tree was built: buildMs stays 0; triangleCount / nodeCount keep describing what is resident, hidden triangles included)
  if (getenv("GATLING_BUILD_TIMING")) fprintf(stderr, "[gatling_gi] visibility update: %u mesh(es) hidden, %u shown, %u renumbered of %zu, %llu visible "
                                              "triangle(s) of %u resident, host %.2f ms, device %.2f ms\n", hides, shows, renumbered, H.meshBuilds.size(),
                                              (unsigned long long)visibleTris, s->triCount, t1 - t0, t2 - t1);
  handled = true;
  return GI_C_OK;
}

// ---------------------------------------------------------------------------------------------------------------
// Visibility updates on the two-level layout (opt-in: GI_C_SCENE_OPTION_TLAS_VISIBILITY / GATLING_OPTIONS=tlas_visibility=1, read with visibility updates
// wanted).  Hiding a mesh of a built two-level scene changes no BLAS, vertex, shading record or instance box.  What changes:
//   the scene-order ids behind the hidden mesh become a fresh build's -- TriRec::origId of the flat records (k_shade, k_aov and the tie-break read them) and
//       InstTrav::triBase (k_trace_dyn2 forms triBase + prim, hashes it for cutouts and orders ties by it);
//   SceneView::flatOfOrig, the table that turns such an id into a flat record, changes with them;
//   the TLAS no longer names the hidden instances.
// The flat tree of a two-level scene is unpartitioned and takes the flat layouts' treatment: zero edges at a hide, edges recomputed at a show, the boxes stay.
//   host: planVisibility's table with VIS_HIDDEN_AFTER set for the instances of hidden meshes; the TLAS built over a copy of T.instBoxes in which those
//       instances carry the inverted box (the builder leaves them out); the depth rule.  T.instBoxes keeps the true boxes: a show needs no bounds kernel.
//   every device, on its own stream: the table, k_patch_visibility2 over the flat records and the id table, k_patch_inst_trav over the instances' records
//       (gi_patch.hip; gi_vispatch.h has the per-item forms), the TLAS nodes and items.  Nothing is read back; the scene bounds stay the flat root's
//       (conservative, as after a flat hide) -- on a scene without the flat tree (SceneHost::treeless) they are made again from the boxes of the instances
//       that are visible after the edit (setSceneBoundsFromInstances): another edit in place may have narrowed them to the visible ones in between.
//   host copies: MeshBuild::hidden / idBase, H.bvh.tris where still held, T.instTrav's triBase, the TLAS; H.flatOfOrig is made again from the host records
//       or, where an update in place dropped them (H.hostTreeDropped), dropped with them -- only a build's upload reads it.
// Every decision comes before the first resident write.  Declines (handled = false, not an error): what updateVisibility declines for but the layout, a scene
// built with inactive triangles, the depth rule (a fresh build would leave the two-level layout), missing T.instTrav / T.instBoxes, the option off (the caller).
// While a mesh is hidden, updateTransformsTwoLevel and updateVerticesTwoLevel keep its instances out of the TLAS they build (planTwoLevelEdit) and decline an
// edit OF the hidden mesh.
// ---------------------------------------------------------------------------------------------------------------
struct TlasMade { bool device = false; uint32_t budget = 0; }; // which builder made an edit's TLAS, and the device builder's depth budget
static TlasMade buildEditTlas(GiCScene* s, uint32_t blasDepth, const float* masked, size_t count, Bvh8& tlas, std::vector<uint32_t>& items);
static void noteTlasMade(TwoLevelHost& T, const TlasMade& made);
static int updateVisibilityTwoLevel(GiCScene* s, SceneHost& H, bool& handled, UpdateCost& cost)
{
  TwoLevelHost& T = H.two;
  const uint32_t instanceCount = (uint32_t)H.instances.size();
  const bool timing = getenv("GATLING_BUILD_TIMING") != nullptr;
  const double t0 = nowMs();
  for (const GiCMesh* m : s->meshes) if (m->visToggled && m->builtInstances == 0xffffffffu) return GI_C_OK; // no records on the device: showing it rebuilds
  if (s->stats.inactiveTriangleCount != 0u || H.partitioned || H.deviceBuilt) return GI_C_OK;
  if (T.instTrav.size() != instanceCount || T.instBoxes.size() != 6u * (size_t)instanceCount) return GI_C_OK; // (cannot happen)
  VisibilityPlan plan;
  if (!planVisibility(s, H, [](const MeshBuild& mb) { return !mb.m->visible; }, plan)) return GI_C_OK; // (cannot happen: count changes ask for the rebuild)
  if (plan.visibleTris < kIncrementalMinTris) return GI_C_OK; // (the floor: VISIBLE triangles, what a fresh build of the edited scene would hold)
  const uint64_t visibleTris = plan.visibleTris; const uint32_t hides = plan.hides, shows = plan.shows, renumbered = plan.renumbered; const bool launch = plan.launch;
  // --- the TLAS over the boxes of the instances that stay visible.  Nothing changes (a hidden mesh hidden again): nothing is built
  std::vector<uint8_t> hiddenAfter(instanceCount, 0);
  for (const MeshBuild& mb : H.meshBuilds) if (plan.hide[mb.meshIdx]) for (const uint32_t inst : mb.inst) if (inst < instanceCount) hiddenAfter[inst] = 1;
  markFreeSlots(H.meshBuilds, hiddenAfter);
  Bvh8 tlas; std::vector<uint32_t> tlasItems; double tlasMs = 0.0; TlasMade tlasMade;
  if (launch) {
    std::vector<float> masked(T.instBoxes);
    tlasMaskHiddenBoxes(masked.data(), hiddenAfter.data(), instanceCount);
    const double ta = nowMs();
    tlasMade = buildEditTlas(s, T.blasDepth, masked.data(), instanceCount, tlas, tlasItems);
    tlasMs = nowMs() - ta;
    if (2u * tlas.maxDepth + T.blasDepth + 1u > 16u) {
      if (timing) fprintf(stderr, "[gatling_gi] visibility update (two-level): the new TLAS is too deep for the 16-entry stack; the scene is rebuilt\n");
      return GI_C_OK;
    }
  }
  // --- decided.  The host copies: the records where they are still held, the MeshBuilds' state; then the table's extra bit for the kernel
  applyVisibilityPlanOnHost(H, plan);
  for (uint32_t i = 0; i < instanceCount; i++) if (hiddenAfter[i]) plan.patch[i].action |= VIS_HIDDEN_AFTER;
  const std::vector<VisPatch>& patch = plan.patch;
  if (launch) {
    patchInstTravHost(T.instTrav.data(), instanceCount, patch.data());
    if (!H.bvh.tris.empty() && H.flatOfOrig.size() == H.bvh.tris.size()) {
      constexpr size_t CHUNK = 65536;
      const size_t n = H.bvh.tris.size();
      parallelOver((n + CHUNK - 1) / CHUNK, [&](size_t c) { // (one writer per word: the visible ids are a permutation)
        for (size_t i = c * CHUNK; i < std::min(n, (c + 1) * CHUNK); i++) {
          const TriRec& t = H.bvh.tris[i];
          if (!hiddenAfter[t.instance] && t.origId < n) H.flatOfOrig[t.origId] = (uint32_t)i;
        }
      });
    } else std::vector<uint32_t>().swap(H.flatOfOrig); // (stale with the dropped host records; nothing reads it before the next build makes it anew)
  }
  if (!(s->dirty & DIRTY_MATERIALS)) deriveSceneClasses(s, H, false); // (as updateVisibility: a material edit due as well runs behind and derives them itself)
  const double t1 = nowMs();
  // --- every device of the scene, on its own stream
  const size_t bytesSent = launch ? patch.size() * sizeof(VisPatch) + tlas.nodes.size() * sizeof(Node8) + tlasItems.size() * sizeof(uint32_t) : 0u;
  if (onSceneDevices(s, launch ? residentDeviceCount(s) : 0u, [&](SceneDevice& D, hipStream_t st) -> int {
    int rc = GI_C_OK;
    DeviceBuffer<VisPatch> dPatch;
    if (D.dTris.count < s->triCount || D.dInstances.count < instanceCount || D.dTriShade.count < H.triShade.size() || D.dInstTrav.count < instanceCount ||
        D.dFlatOfOrig.count < s->triCount) { setError("internal: the device holds less than the scene"); rc = GI_C_ERROR; }
    if (rc == GI_C_OK && dPatch.upload(patch, st)) rc = GI_C_ERROR;
    if (rc == GI_C_OK) {
      launchPatchVisibility2(st, D.dTris.ptr, s->triCount, D.dInstances.ptr, instanceCount, dPatch.ptr, D.dTriShade.ptr, (uint32_t)H.triShade.size(),
          D.dFlatOfOrig.ptr, s->triCount);
      if (renumbered) launchPatchInstTrav(st, D.dInstTrav.ptr, instanceCount, dPatch.ptr);
      if (hipGetLastError() != hipSuccess) rc = GI_C_ERROR;
    }
    if (rc == GI_C_OK && (D.dTlasNodes.upload(tlas.nodes, st) || D.dTlasItems.upload(tlasItems, st))) rc = GI_C_ERROR;
    if (hipStreamSynchronize(st) != hipSuccess) rc = GI_C_ERROR;
    if (rc != GI_C_OK) setError("visibility update (two-level): device error");
    dPatch.release();
    return rc;
  }) != GI_C_OK) return GI_C_ERROR;
  const size_t tlasNodeCount = launch ? tlas.nodes.size() : T.tlasNodes.size();
  if (launch) { T.tlasNodes.swap(tlas.nodes); T.tlasItems.swap(tlasItems); T.tlasDepth = tlas.maxDepth; noteTlasMade(T, tlasMade); }
  // (without the flat tree the bounds are the visible instances' boxes: a show must widen them again where an edit in between narrowed them)
  if (launch && H.treeless) setSceneBoundsFromInstances(s, H);
  const double t2 = nowMs();
  cost.uploadMs = t2 - t0; // (no scene tree was built: buildMs stays 0, the TLAS build over the instance boxes is part of the update's cost here)
  if (timing) fprintf(stderr, "[gatling_gi] visibility update (two-level): %u mesh(es) hidden, %u shown, %u renumbered of %zu, %llu visible triangle(s) of %u "
                              "resident, TLAS %zu node(s), host TLAS build %.2f ms, host rest %.2f ms, device %.2f ms, %zu bytes sent per device\n", hides, shows,
                      renumbered, H.meshBuilds.size(), (unsigned long long)visibleTris, s->triCount, tlasNodeCount, tlasMs, (t1 - t0) - tlasMs, t2 - t1, bytesSent);
  handled = true;
  return GI_C_OK;
}

// ---------------------------------------------------------------------------------------------------------------
// Incremental vertex updates (opt-in: GI_C_SCENE_OPTION_VERTEX_UPDATES / GATLING_OPTIONS=vertex_updates=1).  giCSetMeshVertices moved the points of meshes
// of the built scene; topology, ids, materials and transforms stayed.  The tree keeps its shape and is REFITTED where it lives, in device memory
// (gi_refit.hip): under the traversal contract a tree with the same topology and new conservative boxes gives the bits of a fresh build.
//   host, per edited mesh: its range of H.verts made again by the code buildScene runs (packVertex) and sent to every device; its range of H.triShade
//       gathered from it (gi_refit.h refit_gather_shade: bytewise what packTriShade makes) and NOT sent.
//   device: k_gather_shade makes the mesh's shading records again from the vertex records just sent (the same gather); k_refit_tris makes the flattened records of the edited instances again (TriShade::p, InstanceRec::o2w: flattenTriangle's operations);
//       k_refit_level refits one level per launch, deepest first, over the refit units -- the whole tree (flat layouts, host- or device-built), or every
//       part of an edited mesh (partitioned layout; the part roots are read back, rebuildTop + uploadTopTree run as after a transform edit).
//   afterwards: the root is read back for the scene bounds (bounds retire and the miss rectangle read them).  The class state is untouched.
// Host copies of the tree.  Flat host-built: dropped (H.hostTreeDropped) -- nodes, triangles and face ids would be stale, nothing reads them until the
// re-layout of the first transform edit, which then makes them anew as it does for a device-built scene.  Partitioned: the triangles of the edited parts
// are re-flattened on the host by the same code and the part roots are read back, so everything rebuildTop and later uploads read is current; the interior
// nodes of a refitted part are stale on the host and are never read -- the only upload of a part's node range follows placePart, which rewrites the range.
// Falls back to buildScene (handled = false, not an error): no host copy, GATLING_OPTIONS=incremental=0, the two-level layout, a scene within LDS, fewer
// than kIncrementalMinTris resident triangles, an edited mesh without records on the device (invisible or without a valid material at the build) or hidden
// by updateVisibility, a position that is not finite or beyond 1e18 in object or world space (a fresh build would leave the triangle out of the tree), a scene
// or a part that had inactive triangles when it was built, out of device memory for the float boxes (32 bytes per node).  The caller has established that
// nothing but vertex edits (and visibility toggles, which run behind this update) asked for the rebuild.
// ---------------------------------------------------------------------------------------------------------------
static bool vertexUpdatesWanted(const GiCScene* s)
{
  const long o = optionValue("vertex_updates", -1);
  return o >= 0 ? o == 1 : s->optVertexUpdates == 1;
}

// The launches of a refit (updateVertices; the cloned parts of updateTopology): units = trees with their levels (Bvh8::levelStart, relative to nodeOff);
// per level, deepest first (levels[0]), the thread ranges of launchRefitLevel -- one range per unit that has the level.  False: a level lies outside the
// node array of `nodeCount` nodes (cannot happen)
struct RefitUnit { uint32_t nodeOff; const std::vector<uint32_t>* levelStart; };
struct RefitLevel { uint32_t first, ranges, threads; };
static bool planRefitLevels(const std::vector<RefitUnit>& units, uint32_t nodeCount, std::vector<RefitRange>& ranges, std::vector<RefitLevel>& levels)
{
  size_t maxLevels = 0;
  for (const RefitUnit& u : units) maxLevels = std::max(maxLevels, u.levelStart->size() - 1u);
  for (size_t L = maxLevels; L-- > 0;) {
    RefitLevel lv{(uint32_t)ranges.size(), 0u, 0u};
    for (const RefitUnit& u : units) {
      if (L + 1u >= u.levelStart->size()) continue;
      const uint32_t a = (*u.levelStart)[L], e = (*u.levelStart)[L + 1u];
      if (e <= a || (size_t)u.nodeOff + e > nodeCount) return false;
      ranges.push_back(RefitRange{lv.threads, u.nodeOff + a}); lv.ranges++; lv.threads += e - a;
    }
    levels.push_back(lv);
  }
  return true;
}

// GI_C_SCENE_OPTION_BLAS_UPDATES / GATLING_OPTIONS=blas_updates: vertex edits of a two-level scene are applied in place (updateVerticesTwoLevel below)
bool blasUpdatesWanted(const GiCScene* s)
{
  const long o = optionValue("blas_updates", -1);
  return o >= 0 ? o == 1 : s->optBlasUpdates == 1;
}
static int updateVerticesTwoLevel(GiCScene* s, SceneHost& H, bool& handled, UpdateCost& cost);

static int updateVertices(GiCScene* s, bool& handled, UpdateCost& cost)
{
  SceneHost* host = incrementalHost(s);
  if (host && s->twoLevel && blasUpdatesWanted(s)) return updateVerticesTwoLevel(s, *host, handled, cost);
  if (!host || s->twoLevel || !host->shadePacked || s->triCount < kIncrementalMinTris) return GI_C_OK; // (the floor: resident triangles)
  SceneHost& H = *host;
  if (s->stats.inactiveTriangleCount != 0u) return GI_C_OK;
  if (!H.partitioned && (H.bvh.levelStart.size() < 2u || H.bvh.levelStart.back() != s->nodeCount)) return GI_C_OK;
  const double t0 = nowMs();
  // --- which meshes, and may they be refitted?
  std::vector<uint32_t> edited; // indices into H.meshBuilds
  for (const GiCMesh* m : s->meshes) {
    if (!m->vertsEdited) continue;
    uint32_t b = 0;
    while (b < (uint32_t)H.meshBuilds.size() && H.meshBuilds[b].m != m) b++;
    if (b == (uint32_t)H.meshBuilds.size()) return GI_C_OK; // no records on the device
    const MeshBuild& mb = H.meshBuilds[b];
    if (mb.hidden || m->builtInstances != mb.instCount) return GI_C_OK;
    if ((size_t)mb.vertexOffset + m->vertices.size() > H.verts.size() || (size_t)mb.shadeBase + m->faces.size() > H.triShade.size()) return GI_C_OK;
    // (the shading records are no longer sent: a range the gather kernel would refuse goes to the rebuild, never to stale records)
    if (m->faces.size() > 0xffffffffu || !gatherShadeRangeOk((uint32_t)H.triShade.size(), mb.shadeBase, (uint32_t)m->faces.size())) return GI_C_OK;
    if (!usableVertexPositions(m->vertices.data(), m->vertices.size())) return GI_C_OK;
    edited.push_back(b);
  }
  if (edited.empty()) return GI_C_OK;
  std::vector<uint32_t> editedOfInstance(H.instances.size(), 0u);
  std::atomic<bool> worldOk{true};
  for (uint32_t b : edited) {
    const MeshBuild& mb = H.meshBuilds[b];
    for (uint32_t ii = 0; ii < mb.instCount; ii++) { editedOfInstance[mb.inst[ii]] = 1u; if (!usableInstance(H.instances[mb.inst[ii]])) return GI_C_OK; }
    // every flattened triangle must stay active, by the builders' own rule on the builders' own operands (prepareRange: v0, v0 + e1, v0 + e2)
    const size_t nf = mb.m->faces.size();
    parallelOver(mb.instCount, [&](size_t ii) {
      const InstanceRec& ir = H.instances[mb.inst[ii]];
      for (size_t f = 0; f < nf; f++) {
        TriRec t; flattenTriangle(ir, true, mb.m, (uint32_t)f, t);
        float lo[3], hi[3];
        if (!refit_tri_box(t.v0, t.e1, t.e2, lo, hi)) { worldOk = false; return; }
      }
    });
  }
  if (!worldOk) return GI_C_OK;
  // --- refit units and their levels
  std::vector<RefitUnit> units; std::vector<uint32_t> editedParts;
  if (!H.partitioned) units.push_back(RefitUnit{0u, &H.bvh.levelStart});
  else {
    std::vector<uint8_t> isEdited(H.meshBuilds.size(), 0);
    for (uint32_t b : edited) isEdited[b] = 1;
    for (uint32_t i = 0; i < (uint32_t)H.parts.size(); i++) {
      const InstPart& P = H.parts[i];
      if (!isEdited[P.meshBuild] || P.retired) continue; // (a retired instance's part is unreachable)
      if (P.activeTris != P.nf || P.levelStart.size() < 2u || P.levelStart.back() != P.nodeCount || (size_t)P.nodeOff + P.nodeCount > H.bvh.nodes.size()) return GI_C_OK;
      units.push_back(RefitUnit{P.nodeOff, &P.levelStart}); editedParts.push_back(i);
    }
    if (units.empty()) return GI_C_OK;
  }
  std::vector<RefitRange> ranges; std::vector<RefitLevel> levels;
  if (!planRefitLevels(units, s->nodeCount, ranges, levels)) return GI_C_OK; // (cannot happen: the levels of a tree inside the node array)
  // --- host: the edited meshes' vertex and shading records; the partitioned layout's host triangles
  // (the shading records are a gather of the vertex records, gi_refit.h refit_gather_shade: the host copy by the function the device runs over its own)
  for (uint32_t b : edited) {
    const MeshBuild& mb = H.meshBuilds[b];
    constexpr size_t CHUNK = 4096;
    const size_t nv = mb.m->vertices.size(), nf = mb.m->faces.size();
    parallelOver((nv + CHUNK - 1) / CHUNK, [&](size_t c) {
      for (size_t i = c * CHUNK; i < std::min(nv, (c + 1) * CHUNK); i++) H.verts[mb.vertexOffset + i] = packVertex(mb.m->vertices[i]); });
    parallelOver((nf + CHUNK - 1) / CHUNK, [&](size_t c) {
      for (size_t f = c * CHUNK; f < std::min(nf, (c + 1) * CHUNK); f++) refit_gather_shade(H.verts.data(), (uint32_t)H.verts.size(), H.triShade[mb.shadeBase + f]); });
  }
  for (uint32_t i : editedParts) {
    const InstPart& P = H.parts[i];
    const MeshBuild& mb = H.meshBuilds[P.meshBuild];
    const InstanceRec& ir = H.instances[mb.inst[P.instInMesh]];
    for (uint32_t k = 0; k < P.nf; k++) {
      TriRec& t = H.bvh.tris[P.triFirst + k];
      TriRec whole; flattenTriangle(ir, true, mb.m, t.prim, whole);
      memcpy(t.v0, whole.v0, 12); memcpy(t.e1, whole.e1, 12); memcpy(t.e2, whole.e2, 12);
    }
  }
  const double t1 = nowMs();
  // --- every device of the scene, on its own stream.  Out of memory for the temporaries: the edit goes to buildScene (which sends everything anew)
  bool outOfMemory = false; Node8 root{}; std::vector<Node8> partRoots(editedParts.size());
  const uint32_t instanceCount = (uint32_t)H.instances.size(), shadeCount = (uint32_t)H.triShade.size();
  const int rcDev = onSceneDevices(s, residentDeviceCount(s), [&](SceneDevice& D, hipStream_t st) -> int {
    if (D.dTris.count < s->triCount || D.dNodes.count < s->nodeCount || D.dInstances.count < instanceCount || D.dTriShade.count < shadeCount ||
        D.dVerts.count < H.verts.size()) { setError("internal: the device holds less than the scene"); return GI_C_ERROR; }
    DeviceBuffer<float> dBoxes; DeviceBuffer<uint32_t> dEdited; DeviceBuffer<RefitRange> dRanges;
    auto releaseAll = [&] { dBoxes.release(); dEdited.release(); dRanges.release(); };
    const int a = dBoxes.alloc((size_t)s->nodeCount * 8u), b2 = a ? a : dEdited.alloc(editedOfInstance.size()), c = b2 ? b2 : dRanges.alloc(ranges.size());
    if (c != GI_C_OK) { releaseAll(); if (c == GI_C_OUT_OF_MEMORY_INTERNAL) { outOfMemory = true; return DEVICE_BUILD_FALLBACK; } return GI_C_ERROR; }
    int rc = GI_C_OK;
    auto copy = [&](void* dst, const void* src, size_t bytes, hipMemcpyKind kind) {
      if (rc == GI_C_OK && bytes && hipMemcpyAsync(dst, src, bytes, kind, st) != hipSuccess) { setError("vertex update: copy failed"); rc = GI_C_ERROR; } };
    for (uint32_t b : edited) {
      const MeshBuild& mb = H.meshBuilds[b];
      copy(D.dVerts.ptr + mb.vertexOffset, &H.verts[mb.vertexOffset], mb.m->vertices.size() * sizeof(FVertex), hipMemcpyHostToDevice);
    }
    // (behind the vertex uploads on the same stream, in front of k_refit_tris, which reads TriShade::p)
    if (rc == GI_C_OK) for (uint32_t b : edited) {
      const MeshBuild& mb = H.meshBuilds[b];
      if (!launchGatherShade(st, D.dTriShade.ptr, shadeCount, mb.shadeBase, (uint32_t)mb.m->faces.size(), D.dVerts.ptr, (uint32_t)H.verts.size())) {
        setError("internal: shading records outside the array"); rc = GI_C_ERROR; break; } // (cannot happen: asked above)
    }
    copy(dEdited.ptr, editedOfInstance.data(), editedOfInstance.size() * sizeof(uint32_t), hipMemcpyHostToDevice);
    copy(dRanges.ptr, ranges.data(), ranges.size() * sizeof(RefitRange), hipMemcpyHostToDevice);
    if (rc == GI_C_OK) {
      launchRefitTris(st, D.dTris.ptr, s->triCount, D.dInstances.ptr, instanceCount, dEdited.ptr, D.dTriShade.ptr, shadeCount);
      for (const RefitLevel& lv : levels) launchRefitLevel(st, D.dNodes.ptr, s->nodeCount, dBoxes.ptr, dRanges.ptr + lv.first, lv.ranges, lv.threads, D.dTris.ptr,
          s->triCount, D.dInstances.ptr, instanceCount, D.dTriShade.ptr, shadeCount);
      if (hipGetLastError() != hipSuccess) { setError("vertex update: launch failed"); rc = GI_C_ERROR; }
    }
    if (D.slot == 0u) { // (the refit is deterministic: every device holds the same bytes)
      if (!H.partitioned) copy(&root, D.dNodes.ptr, sizeof(Node8), hipMemcpyDeviceToHost);
      for (size_t k = 0; k < editedParts.size(); k++) copy(&partRoots[k], D.dNodes.ptr + H.parts[editedParts[k]].nodeOff, sizeof(Node8), hipMemcpyDeviceToHost);
    }
    if (hipStreamSynchronize(st) != hipSuccess && rc == GI_C_OK) { setError("vertex update: device error"); rc = GI_C_ERROR; }
    releaseAll(); // (before the render's memory plan reads free memory)
    return rc;
  });
  if (rcDev == DEVICE_BUILD_FALLBACK && outOfMemory) {
    if (getenv("GATLING_BUILD_TIMING")) fprintf(stderr, "[gatling_gi] vertex update: out of device memory for the refit's boxes; the scene is rebuilt\n");
    return GI_C_OK;
  }
  if (rcDev != GI_C_OK) return GI_C_ERROR;
  // --- the scene bounds; the top tree of a partitioned scene; the host copies
  if (!H.partitioned) {
    setSceneBounds(s, std::vector<Node8>{root});
    if (!H.deviceBuilt && !H.hostTreeDropped) { // the host copies of a host-built tree are stale from here on: dropped
      std::vector<Node8>().swap(H.bvh.nodes); std::vector<TriRec>().swap(H.bvh.tris); std::vector<int32_t>().swap(H.triFaceId);
      H.hostTreeDropped = true;
    }
  } else {
    for (size_t k = 0; k < editedParts.size(); k++) { InstPart& P = H.parts[editedParts[k]]; H.bvh.nodes[P.nodeOff] = partRoots[k]; nodeBounds(partRoots[k], P.box); }
    if (rebuildTop(s, H) != GI_C_OK) return GI_C_ERROR;
    setSceneBounds(s, H.bvh.nodes);
    if (onSceneDevices(s, residentDeviceCount(s), [&](SceneDevice& D, hipStream_t st) -> int {
      if (uploadTopTree(D, H, st) != GI_C_OK) return GI_C_ERROR;
      HIP_TRY(hipStreamSynchronize(st));
      return GI_C_OK;
    }) != GI_C_OK) return GI_C_ERROR;
  }
  const double t2 = nowMs();
  cost.uploadMs = t2 - t0; // (no tree was built: buildMs stays 0)
  if (getenv("GATLING_BUILD_TIMING")) {
    size_t sent = editedOfInstance.size() * sizeof(uint32_t) + ranges.size() * sizeof(RefitRange), gathered = 0; // per device
    for (uint32_t b : edited) { sent += H.meshBuilds[b].m->vertices.size() * sizeof(FVertex); gathered += H.meshBuilds[b].m->faces.size() * sizeof(TriShade); }
    fprintf(stderr, "[gatling_gi] vertex update: %zu mesh(es), %zu refit unit(s), %zu level launch(es), host %.2f ms, device %.2f ms, %zu bytes sent per device, "
                    "%zu bytes of shading records gathered there\n", edited.size(), units.size(), levels.size(), t1 - t0, t2 - t1, sent, gathered);
  }
  handled = true;
  return GI_C_OK;
}

// ---------------------------------------------------------------------------------------------------------------
// Incremental topology updates (opt-in: GI_C_SCENE_OPTION_TOPOLOGY_UPDATES / GATLING_OPTIONS=topology_updates=1).  Meshes were created or destroyed (what
// hdGatling does on every points, primvar or topology change of a prim: giDestroyMesh, giCreateMesh and every setter again, mesh.cpp:458-509); nothing else
// asked for the rebuild.  The partitioned layout already gives every flattened instance its own subtree and ranges under a rebuilt top tree, so the SET of
// parts may change as well:
//   re-layout: a flat scene (host-built, device-built, host tree dropped) is first re-laid out as updateTransforms does (relayoutPartitioned) and sent whole.
//   retire:    a destroyed mesh of the built scene was kept (GiCMesh::retired, GiCScene::retiredMeshes).  Its MeshBuild becomes hidden for good: its parts
//              drop out of the top tree and the meshes behind it are renumbered -- updateVisibility's plan, host pass and k_patch_visibility.  Its records
//              stay resident until the next buildScene, which frees the mesh too.
//   append:    every mesh a fresh build would hold that has no MeshBuild gets one at the ends of the arrays (vertices, shading records, instances, triangles,
//              face ids, one node range per instance with the usual reserve), made by the code buildScene runs.  Its parts are built by buildPart / placePart
//              in parallel, or -- with the scene's device builder on (GI_C_SCENE_OPTION_BVH_BUILD / device_build) and at least device_parts_min faces -- where
//              they live: buildBvh8Device over the part's own records, then k_place_part (gi_patch.hip).  The host copy of a device-built part holds its
//              records in scene order and only the root of its subtree: the interior is stale on the host and never read, as after a vertex refit -- the
//              only upload of a part's node range follows placePart, which rewrites it.
//   device:    the arrays grow in place (DeviceBuffer::grow: contents kept, 25 % slack); only the appended ranges, the top tree, the mesh records and the
//              scene data are sent.
// The image is that of a fresh build: the only thing of the tree that reaches an image is the scene-order triangle id, and an appended mesh lies behind every
// live built mesh, so its ids are the visible triangles in front of it.
// Falls back to buildScene (handled = false, not an error): no host copy, GATLING_OPTIONS=incremental=0, the two-level layout, a scene within LDS, fewer
// than kIncrementalMinTris visible triangles after the edit, an appended mesh with a position that is not finite or beyond 1e18 in object or world space (or
// an unusable instance transform), a mesh to append in front of a live built mesh, the top tree outgrowing its range, 2^26 resident triangles, more retired
// triangles than live ones (resident memory stays within twice the live scene, and the rebuild that compacts it is amortised), a flat scene that retires more
// than it keeps of what was built (the re-layout would not pay), out of device memory.
// ---------------------------------------------------------------------------------------------------------------
bool topologyUpdatesWanted(const GiCScene* s)
{
  const long o = optionValue("topology_updates", -1);
  return o >= 0 ? o == 1 : s->optTopologyUpdates == 1;
}
// Instance updates (opt-in on top of topology updates: GI_C_SCENE_OPTION_INSTANCE_UPDATES / GATLING_OPTIONS=instance_updates=1).  The delegate answers every
// DirtyInstancer / DirtyInstanceIndex sync of a prim with giSetMeshInstanceTransforms, giSetMeshInstancerPrimvars and giSetMeshInstanceIds (mesh.cpp:530-572):
// an animated point instancer.  giCSetMeshInstanceIds, and giCSetMeshInstanceTransforms with another count, on a mesh of the built scene note the edit on the
// mesh (GiCMesh::instEdited, GiCScene::instancesDue) and updateTopology applies it, in front of its other work and sharing it:
//   ids:     InstanceRec::instanceId of the kept instances [0, min(old, new)) whose id changed is set and the records are re-sent; equal ids send nothing.
//            Works on every layout updateTopology accepts: ids alone re-lay nothing out.
//   moves:   a kept instance whose transform differs from the resident record is marked in GiCMesh::instDirty and DIRTY_XFORM is raised: updateTransforms
//            rebuilds those parts behind this update, as after an adoption.
//   shrink:  the instances [new, old) retire: InstPart::retired takes their parts out of the top tree for good, their records stay resident until the next
//            build (MeshBuild::retiredInst: counted as retired triangles in the retired > live rule), the meshes behind are renumbered by the plan.
//   grow:    the instances [old, new) are appended as the instances of a new mesh are: one InstanceRec, nf records and face ids at the ends of the arrays, one
//            node range and one part each; ids are the mesh's id base + instance-in-mesh x nf + prim, the meshes behind shift by the plan's idDelta.  A new
//            part is CLONED from a live sibling part of the mesh where one qualifies -- it was resident before this update, is whole with its levels
//            (refitsWith's conditions on the part), the mesh is not hidden -- and GATLING_OPTIONS=instance_clone=1 asks for it (default off, see the
//            measurement in DESIGN.md section 9): k_clone_parts (gi_patch.hip) copies the sibling's records and nodes in device memory, re-transformed, renumbered and rebased,
//            k_refit_level gives the copied subtree its boxes, level by level over all clones together, and the part roots are read back for the top tree.
//            The host keeps the records by the function the kernel runs (gi_refit.h refit_clone_record) and the root; the interior is stale on the host and
//            never read, as after a vertex refit.  A cloned topology is a valid one: only scene-order ids reach an image and the refit is conservative.
//            Otherwise the part is built by buildPart, or by the device builder from device_parts_min faces on.
//   scene data: a mesh whose material reads primvars gets the MeshRec / scene-data tables made again (appendMeshSceneData sizes instance-interpolated
//            entries from the count and the ids).
// MeshBuild::inst names the InstanceRec of every live instance: after a grow they are no longer one run.  Declines (to buildScene, not an error): whatever
// updateTopology declines for, a new count of 0, a mesh hidden by the visibility path, an unusable transform of a new instance.
bool instanceUpdatesWanted(const GiCScene* s)
{
  if (!topologyUpdatesWanted(s)) return false;
  const long o = optionValue("instance_updates", -1);
  return o >= 0 ? o == 1 : s->optInstanceUpdates == 1;
}
// Resyncs (opt-in on top of topology and vertex updates: GI_C_SCENE_OPTION_RESYNC_REFITS / GATLING_OPTIONS=resync_refits=1).  The delegate answers a points or
// primvar change of a prim with destroy + create of a mesh whose faces did not change: retire + append would leave N dead triangles behind per frame and
// build a subtree whose topology the resident one already has.  adoptResyncs pairs each retiring mesh R (retired, its MeshBuild not hidden) with a fresh mesh
// F (no records, visible, with faces and a valid material), both taken in creation order, the first partner that qualifies wins; F ADOPTS R's resident
// records: the MeshBuild points at F, F counts as built, R is freed, nothing is retired or appended for the pair.  What differs between the two goes down the
// paths that run behind updateTopology: vertices -> GiCMesh::vertsEdited (only if the bytes differ) -> updateVertices' refit; material assignment and primvars
// -> DIRTY_MATERIALS -> updateMaterials; transforms -> xformDirty / instDirty -> updateTransforms.
// A pair qualifies if faces (count and bytes), face ids, maxFaceId, vertex count, handedness, sidedness, id, instance count and instance ids are equal; if
// updateVertices could refit R's records with F's points (not hidden; positions usable in object and world space; every part whole with its levels; no
// inactive triangle at the scene's build); and if no fresh mesh that is not itself adopted precedes F in GiCScene::meshes (appended meshes lie behind every
// built one).  Any other pair is retired and appended as before.
// Scene order: F sits where it was created, its records where R's sat.  From the first adoption on (SceneHost::reordered) id bases are accumulated in the
// order of GiCScene::meshes (sceneOrder, planVisibility), and the plan's idDelta renumbers F's triangles and those of every mesh that was behind R through
// k_patch_visibility.  Storage -- instFirst, triFirst, shadeBase, vertexOffset, meshIdx, node ranges -- stays where it is.
static bool resyncRefitsWanted(const GiCScene* s)
{
  if (!topologyUpdatesWanted(s) || !vertexUpdatesWanted(s)) return false;
  const long o = optionValue("resync_refits", -1);
  return o >= 0 ? o == 1 : s->optResyncRefits == 1;
}
// R's resident records fit F: everything the records, the tree's topology and the AOV tables were made from is equal
static bool sameRecords(const GiCMesh* r, const GiCMesh* f)
{
  return r->faces.size() == f->faces.size() && memcmp(r->faces.data(), f->faces.data(), r->faces.size() * sizeof(GiCFace)) == 0 && r->faceIds == f->faceIds &&
      r->maxFaceId == f->maxFaceId && r->vertices.size() == f->vertices.size() && r->flipFacing == f->flipFacing && r->doubleSided == f->doubleSided &&
      r->id == f->id && r->instanceTransforms.size() == f->instanceTransforms.size() && r->instanceIds == f->instanceIds;
}
static bool samePrimvars(const std::vector<GiCPrimvar>& a, const std::vector<GiCPrimvar>& b)
{
  if (a.size() != b.size()) return false;
  for (size_t i = 0; i < a.size(); i++) if (a[i].name != b[i].name || a[i].type != b[i].type || a[i].interpolation != b[i].interpolation ||
      a[i].data.size() != b[i].data.size() || memcmp(a[i].data.data(), b[i].data.data(), a[i].data.size() * sizeof(float)) != 0) return false;
  return true;
}
// updateVertices' preconditions for the MeshBuild `b` with F's points and transforms; the instance records F gives are left in `inst`
// (The world-space pass is knowingly run twice in a sync that adopts: here with the transforms F brings, and again in updateVertices with the resident
// ones, which are R's until updateTransforms has run -- the two differ whenever the resync moved the mesh, so neither result stands in for the other.  On
// C5 this pass is part of the 1.7 ms a topology update that adopts a 40 960-triangle mesh takes.)
static bool refitsWith(const GiCScene* s, const SceneHost& H, uint32_t b, const GiCMesh* f, std::vector<InstanceRec>& inst)
{
  const MeshBuild& mb = H.meshBuilds[b];
  if (mb.hidden || s->stats.inactiveTriangleCount != 0u || !usableVertexPositions(f->vertices.data(), f->vertices.size())) return false;
  if ((size_t)mb.vertexOffset + f->vertices.size() > H.verts.size() || (size_t)mb.shadeBase + f->faces.size() > H.triShade.size()) return false;
  if (H.partitioned) for (const InstPart& P : H.parts)
    if (P.meshBuild == b && !P.retired && (P.activeTris != P.nf || P.levelStart.size() < 2u || P.levelStart.back() != P.nodeCount)) return false;
  inst.resize(mb.instCount);
  for (uint32_t ii = 0; ii < mb.instCount; ii++) { inst[ii] = makeInstanceRec(f, mb.meshIdx, ii); if (!usableInstance(inst[ii])) return false; }
  std::atomic<bool> worldOk{true};
  const size_t nf = f->faces.size();
  parallelOver(mb.instCount, [&](size_t ii) {
    for (size_t k = 0; k < nf; k++) {
      TriRec t; flattenTriangle(inst[ii], true, f, (uint32_t)k, t);
      float lo[3], hi[3];
      if (!refit_tri_box(t.v0, t.e1, t.e2, lo, hi)) { worldOk = false; return; }
    }
  });
  return worldOk;
}
static uint32_t adoptResyncs(GiCScene* s, SceneHost& H)
{
  std::vector<uint32_t> retiring; // indices into H.meshBuilds, creation order
  for (uint32_t b = 0; b < (uint32_t)H.meshBuilds.size(); b++) if (H.meshBuilds[b].m->retired && !H.meshBuilds[b].hidden) retiring.push_back(b);
  uint32_t adopted = 0;
  if (retiring.empty()) return 0u;
  std::vector<InstanceRec> inst;
  for (GiCMesh* f : s->meshes) {
    if (f->builtInstances != 0xffffffffu || !f->visible || f->faces.empty()) continue; // (as updateTopology: not a fresh mesh)
    if (std::find(s->materials.begin(), s->materials.end(), f->material) == s->materials.end()) continue;
    size_t k = 0;
    while (k < retiring.size() && !(sameRecords(H.meshBuilds[retiring[k]].m, f) && refitsWith(s, H, retiring[k], f, inst))) k++;
    if (k == retiring.size()) break; // this mesh will be appended: every fresh mesh behind it lies behind an appended one
    MeshBuild& mb = H.meshBuilds[retiring[k]];
    GiCMesh* r = const_cast<GiCMesh*>(mb.m);
    // what differs goes down the paths behind this update.  (An edit of R that was still due when it was destroyed: its vertices are not the resident ones;
    // its material-side edits raised DIRTY_MATERIALS themselves; transforms are compared with the resident instance records.)
    f->vertsEdited = r->vertsEdited || memcmp(r->vertices.data(), f->vertices.data(), f->vertices.size() * sizeof(GiCVertex)) != 0;
    if (r->material != f->material || !samePrimvars(r->primvars, f->primvars) || !samePrimvars(r->instancerPrimvars, f->instancerPrimvars)) s->dirty |= DIRTY_MATERIALS;
    f->xformDirty = false; f->instDirty.assign(mb.instCount, 0);
    for (uint32_t ii = 0; ii < mb.instCount; ii++)
      if (memcmp(inst[ii].o2w, H.instances[mb.inst[ii]].o2w, sizeof(inst[ii].o2w)) != 0) { f->instDirty[ii] = 1; f->xformDirty = true; }
    if (f->xformDirty) s->dirty |= DIRTY_XFORM; else f->instDirty.clear();
    f->builtInstances = mb.instCount; f->visToggled = false;
    mb.m = f;
    s->retiredMeshes.erase(std::remove(s->retiredMeshes.begin(), s->retiredMeshes.end(), r), s->retiredMeshes.end());
    delete r;
    retiring.erase(retiring.begin() + (ptrdiff_t)k);
    H.reordered = true; adopted++;
    if (retiring.empty()) break;
  }
  return adopted;
}

// faces from which an appended part is built on the device when the scene's device builder is on (GATLING_OPTIONS=device_parts_min).  Measured for ONE part
// (tools/time_topology_edit.py): buildPart 0.57 / 1.2 / 2.4 / 5.0 / 11.3 ms at 1 / 2 / 4 / 8 / 16 Ki faces, the device route 2.1 / 2.3 /
// 2.4 / 3.1 / 3.2 ms (a floor of ~2 ms of launches and stream synchronisations): they cross at 4 Ki.  Several parts are built in parallel by the host and
// one after another on the device, so an edit of many mid-sized parts is faster on the host (C5, 8 parts of 5 120 faces: 5 ms against 21 ms)
constexpr long kDevicePartsMinDefault = 4096;

// GI_C_SCENE_OPTION_TLAS_TOPOLOGY / GATLING_OPTIONS=tlas_topology: mesh creations and destructions on a two-level scene without the flat tree are applied in
// place (updateTopologyTwoLevel below); read only with topology updates wanted
bool tlasTopologyWanted(const GiCScene* s)
{
  if (!topologyUpdatesWanted(s)) return false;
  const long o = optionValue("tlas_topology", -1);
  return o >= 0 ? o == 1 : s->optTlasTopology == 1;
}
static int updateTopologyTwoLevel(GiCScene* s, SceneHost& H, bool& handled, UpdateCost& cost, bool afterCompaction = false);

static int updateTopology(GiCScene* s, bool& handled, UpdateCost& cost)
{
  SceneHost* host = incrementalHost(s);
  if (s->twoLevel && tlasTopologyWanted(s)) {
    if (host && host->treeless && host->shadePacked) return updateTopologyTwoLevel(s, *host, handled, cost);
    if (getenv("GATLING_BUILD_TIMING")) fprintf(stderr, "[gatling_gi] topology update (two-level): %s; the scene is rebuilt\n",
        host ? "the scene keeps its flat tree (built without GI_C_SCENE_OPTION_TLAS_ONLY)" : "no host copy of the scene, or GATLING_OPTIONS=incremental=0");
    return GI_C_OK;
  }
  if (!host || s->twoLevel || !host->shadePacked) return GI_C_OK;
  SceneHost& H = *host;
  if (H.meshRecs.size() != H.meshBuilds.size()) return GI_C_OK;
  for (const MeshBuild& mb : H.meshBuilds) if (mb.m->builtInstances != mb.instCount) return GI_C_OK; // (cannot happen: count changes ask for the rebuild)
  const double t0 = nowMs();
  // --- resyncs: a retiring and a fresh mesh with the same faces become a vertex edit of the resident records
  // adoptResyncs changes the scene at once -- MeshBuild::m repointed, R freed, F counted as built, dirty bits raised -- so EVERY decline behind this point must
  // lead to the full build (it does: a decline raises DIRTY_BVH and rebuildDue, and buildScene makes all of that state anew from GiCScene::meshes).  Until
  // updateVertices has run behind this update, H.verts / H.triShade still hold R's points while a re-layout below builds the parts from F's: F is marked
  // vertsEdited whenever the bytes differ, and an updateVertices that declines rebuilds as well.
  const uint32_t adopted = resyncRefitsWanted(s) ? adoptResyncs(s, H) : 0u;
  // --- instance edits of built meshes (the caller has established that the option is wanted): which, and what they add and retire
  struct InstEdit { uint32_t b, oldCount, newCount; };
  std::vector<InstEdit> instEdits;
  uint64_t grownTris = 0, grownParts = 0, shrunkTris = 0, shrunkParts = 0; bool sceneDataStale = false;
  for (uint32_t b = 0; b < (uint32_t)H.meshBuilds.size(); b++) {
    const MeshBuild& mb = H.meshBuilds[b];
    if (!mb.m->instEdited || mb.m->retired) continue;
    const size_t newCount = mb.m->instanceTransforms.size() / 16;
    if (newCount == 0u || newCount >= 0xffffffffu || mb.hidden) return GI_C_OK; // (a mesh without instances leaves the scene; a hidden one has ids to come back to)
    instEdits.push_back(InstEdit{b, mb.instCount, (uint32_t)newCount});
    const uint64_t nf = mb.m->faces.size();
    if (newCount > mb.instCount) { grownParts += newCount - mb.instCount; grownTris += (newCount - mb.instCount) * nf; }
    else { shrunkParts += mb.instCount - newCount; shrunkTris += (mb.instCount - newCount) * nf; }
    if (mb.m->material) for (uint32_t slot = 0; slot < TEX_SLOT_COUNT; slot++) if (!mb.m->material->primvarInput[slot].empty()) sceneDataStale = true;
  }
  const bool countsChange = grownParts != 0u || shrunkParts != 0u;
  // --- the meshes to append: what a fresh build would hold and the resident scene does not, all of them behind every live built mesh
  struct NewMesh { GiCMesh* m; uint32_t material; };
  std::vector<NewMesh> fresh;
  uint64_t appendedTris = grownTris, appendedParts = grownParts;
  for (GiCMesh* m : s->meshes) {
    if (m->builtInstances != 0xffffffffu) { if (!fresh.empty()) return GI_C_OK; continue; }
    if (!m->visible || m->faces.empty()) continue; // (as buildScene)
    auto mit = std::find(s->materials.begin(), s->materials.end(), m->material);
    if (mit == s->materials.end()) continue;
    const uint32_t material = (uint32_t)(mit - s->materials.begin());
    if (material > 0x00ffffffu) return GI_C_OK;
    if (!usableVertexPositions(m->vertices.data(), m->vertices.size())) return GI_C_OK;
    fresh.push_back(NewMesh{m, material});
    const uint64_t instCount = m->instanceTransforms.size() / 16;
    appendedTris += instCount * m->faces.size(); appendedParts += instCount;
  }
  // --- what the scene holds after the edit
  uint64_t live = appendedTris, retired = 0, visible = appendedTris, partsNow = 0; uint32_t retiring = 0;
  for (const MeshBuild& mb : H.meshBuilds) {
    const uint64_t n = (uint64_t)mb.instCount * mb.m->faces.size(), gone = (uint64_t)mb.retiredInst * mb.m->faces.size(); // (gone: instances retired earlier)
    partsNow += mb.instCount + mb.retiredInst;
    if (mb.m->retired) { retired += n + gone; if (!mb.hidden) retiring++; } else { live += n; retired += gone; if (!mb.hidden) visible += n; }
  }
  live -= shrunkTris; visible -= shrunkTris; retired += shrunkTris; // (the instances this update retires: of live, visible meshes)
  if (visible < kIncrementalMinTris || retired > live || partsNow == 0u) return GI_C_OK;
  // a flat scene that loses more than it keeps: the re-layout would spend its time on subtrees for what is leaving (measured on C3, one mesh resynced: 809 ms
  // against the 580 ms of the build that follows anyway once the retired triangles outnumber the live ones)
  if (!H.partitioned && retired > live - appendedTris) return GI_C_OK;
  if ((uint64_t)s->triCount + appendedTris >= ((uint64_t)1 << 26)) return GI_C_OK;
  const uint64_t topCap = H.partitioned ? H.topCap : (partsNow * 2u + 16u) * 2u; // (what relayoutPartitioned reserves)
  if (appendedParts && (partsNow + appendedParts) * 2u + 16u > topCap) return GI_C_OK; // the top tree may outgrow its range
  const uint32_t nDev = residentDeviceCount(s);
  const bool timing = getenv("GATLING_BUILD_TIMING") != nullptr;
  if (fresh.empty() && retiring == 0u && adopted == 0u && instEdits.empty()) { // the edited meshes are not part of a fresh build either (invisible, no faces, no valid material)
    for (GiCMesh* m : s->meshes) if (m->builtInstances == 0xffffffffu) { m->visToggled = false; m->vertsEdited = false; }
    handled = true;
    return GI_C_OK;
  }
  // --- instance edits, committed: from here on the MeshBuilds and the meshes hold the new counts (every decline behind this point leads to the full build, as
  // after an adoption).  Ids and moves of the kept instances; the retired instances' parts; the records of appended instances follow the plan below
  std::vector<uint32_t> idRecords; // InstanceRecs to re-send
  uint32_t movedInstances = 0;
  for (const InstEdit& e : instEdits) {
    MeshBuild& mb = H.meshBuilds[e.b];
    GiCMesh* m = const_cast<GiCMesh*>(mb.m);
    const uint32_t kept = std::min(e.oldCount, e.newCount);
    const bool all = m->xformDirty && m->instDirty.empty(); // (a giCSetMeshTransform is due as well: every part is rebuilt anyway)
    if (!all) m->instDirty.resize(e.newCount, 0);
    for (uint32_t ii = 0; ii < kept; ii++) {
      InstanceRec& resident = H.instances[mb.inst[ii]];
      const InstanceRec want = makeInstanceRec(m, mb.meshIdx, ii);
      if (want.instanceId != resident.instanceId) { resident.instanceId = want.instanceId; idRecords.push_back(mb.inst[ii]); }
      if (memcmp(want.o2w, resident.o2w, sizeof(want.o2w)) != 0) { movedInstances++; m->xformDirty = true; if (!all) m->instDirty[ii] = 1; }
    }
    if (m->xformDirty) s->dirty |= DIRTY_XFORM; else m->instDirty.clear();
    if (H.partitioned) for (InstPart& P : H.parts) if (P.meshBuild == e.b && !P.retired && P.instInMesh >= e.newCount) P.retired = true;
    if (e.newCount < e.oldCount) { mb.inst.resize(e.newCount); mb.retiredInst += e.oldCount - e.newCount; }
    mb.instCount = e.newCount; m->builtInstances = e.newCount; m->instEdited = false;
  }
  // --- ids alone (and moves, which updateTransforms takes): nothing is laid out, appended or retired.  Every layout
  if (fresh.empty() && retiring == 0u && adopted == 0u && !countsChange) {
    if (sceneDataStale && !(s->dirty & DIRTY_MATERIALS)) remakeSceneData(H); // (with a material edit due updateMaterials makes the tables behind this update)
    else sceneDataStale = false;
    if (onSceneDevices(s, idRecords.empty() && !sceneDataStale ? 0u : nDev, [&](SceneDevice& D, hipStream_t st) -> int {
      if (D.dInstances.count < H.instances.size()) { setError("internal: the device holds less than the scene"); return GI_C_ERROR; }
      for (const uint32_t rec : idRecords) HIP_TRY(hipMemcpyAsync(D.dInstances.ptr + rec, &H.instances[rec], sizeof(InstanceRec), hipMemcpyHostToDevice, st));
      if (sceneDataStale && (D.dMeshes.upload(H.meshRecs, st) || D.dSceneData.upload(H.sceneData, st))) return GI_C_ERROR;
      HIP_TRY(hipStreamSynchronize(st));
      return GI_C_OK;
    }) != GI_C_OK) return GI_C_ERROR;
    cost.uploadMs = nowMs() - t0;
    if (timing) fprintf(stderr, "[gatling_gi] instance update: 0 instance(s) retired, 0 appended (0 cloned, 0 built), %zu instance record(s) re-sent for their ids, %u moved, "
                                "0 node and record byte(s) sent for the new parts, builds 0.00 ms, rest %.2f ms\n", idRecords.size(), movedInstances, cost.uploadMs);
    s->instanceCounts[0]++;
    handled = true;
    return GI_C_OK;
  }
  // --- a flat scene: re-laid out and sent whole first
  bool converted = false;
  if (!H.partitioned) {
    if (!relayoutPartitioned(s, H)) return GI_C_OK;
    converted = true;
    s->nodeCount = (uint32_t)H.bvh.nodes.size();
    if (onSceneDevices(s, nDev, [&](SceneDevice& D, hipStream_t st) { return uploadSceneTo(s, D, H, st); }) != GI_C_OK) return GI_C_ERROR;
  }
  if (H.bvh.tris.size() != s->triCount || H.triFaceId.size() != s->triCount) return GI_C_OK; // (cannot happen: a partitioned scene keeps its host triangles)
  double buildMs = converted ? nowMs() - t0 : 0.0;
  // --- retire: hidden for good, the meshes behind renumbered
  VisibilityPlan plan;
  if (!planVisibility(s, H, [](const MeshBuild& mb) { return mb.hidden || mb.m->retired; }, plan)) return GI_C_OK;
  applyVisibilityPlanOnHost(H, plan);
  const uint32_t oldTris = s->triCount, oldInstances = (uint32_t)H.instances.size();
  // --- append, host side: the MeshBuilds and everything that does not depend on a tree
  if (s->dirty & DIRTY_MATERIALS) buildMaterialRecords(s, H.mats); // the new meshes' words come from the current table; updateMaterials runs behind this update
  const size_t vert0 = H.verts.size(), shade0 = H.triShade.size(), node0 = H.bvh.nodes.size(), part0 = H.parts.size();
  uint64_t idBase = plan.visibleTris; // the visible triangles in front of the next appended mesh
  // (25 % slack, as on the device: a std::vector would double 0.7 GB of triangles on the first append to C5 and copy them on every later doubling)
  auto grown = [](auto& v, size_t n) { if (v.capacity() < n) v.reserve(n + n / 4u); v.resize(n); };
  for (const NewMesh& nm : fresh) {
    GiCMesh* m = nm.m;
    const uint32_t matFlags = meshMatFlags(H.mats[nm.material], nm.material, m);
    const uint32_t vertexOffset = (uint32_t)H.verts.size(), meshIdx = (uint32_t)H.meshBuilds.size();
    const uint32_t instCount = (uint32_t)(m->instanceTransforms.size() / 16), nf = (uint32_t)m->faces.size(), triFirst = (uint32_t)H.bvh.tris.size();
    appendMeshSceneData(m, m->material, vertexOffset, H.meshRecs, H.sceneData);
    for (const GiCVertex& vIn : m->vertices) H.verts.push_back(packVertex(vIn));
    H.meshBuilds.push_back(MeshBuild{m, vertexOffset, matFlags, (uint32_t)H.instances.size(), instCount, triFirst, meshIdx, faceIdAovOf(m)});
    H.meshBuilds.back().shadeBase = (uint32_t)H.triShade.size(); H.meshBuilds.back().idBase = (uint32_t)idBase;
    for (const GiCFace& f : m->faces) H.triShade.push_back(packTriShade(m->vertices.data(), f, vertexOffset));
    grown(H.instances, H.instances.size() + instCount); grown(H.bvh.tris, (size_t)triFirst + (size_t)instCount * nf); grown(H.triFaceId, H.bvh.tris.size());
    for (uint32_t ii = 0; ii < instCount; ii++) { InstPart P{}; P.meshBuild = meshIdx; P.instInMesh = ii; P.triFirst = triFirst + ii * nf; P.nf = nf;
        H.parts.push_back(P); }
    idBase += (uint64_t)instCount * nf;
    H.meshBuilds.back().numberInstances();
  }
  // --- append, instances of built meshes: one record, one triangle range and one part each; the part it may be cloned from
  // (the sibling itself must be whole: inactive triangles elsewhere in the scene do not concern a clone, whose refit reads its own range alone)
  // Opt-in (GATLING_OPTIONS=instance_clone=1): measured on C5, 64 clones cost 16 - 22 % of traceMs against a tree built from scratch
  const bool cloneWanted = optionValue("instance_clone", 0) == 1;
  std::vector<int64_t> siblingOfPart; // per new part: the resident part to clone, or -1
  siblingOfPart.assign(H.parts.size() - part0, -1);
  for (const InstEdit& e : instEdits) {
    if (e.newCount <= e.oldCount) continue;
    MeshBuild& mb = H.meshBuilds[e.b];
    const uint32_t nf = (uint32_t)mb.m->faces.size();
    int64_t sibling = -1;
    if (cloneWanted) for (size_t i = 0; i < part0 && sibling < 0; i++) {
      const InstPart& P = H.parts[i];
      if (P.meshBuild == e.b && !P.retired && P.nf == nf && P.activeTris == P.nf && P.levelStart.size() >= 2u && P.levelStart.back() == P.nodeCount && P.nodeCount != 0u &&
          (size_t)P.nodeOff + P.nodeCount <= node0 && (size_t)P.triFirst + P.nf <= oldTris) sibling = (int64_t)i;
    }
    for (uint32_t ii = e.oldCount; ii < e.newCount; ii++) {
      mb.inst.push_back((uint32_t)H.instances.size());
      grown(H.instances, H.instances.size() + 1u);
      InstPart P{}; P.meshBuild = e.b; P.instInMesh = ii; P.triFirst = (uint32_t)H.bvh.tris.size(); P.nf = nf;
      grown(H.bvh.tris, (size_t)P.triFirst + nf); grown(H.triFaceId, H.bvh.tris.size());
      H.parts.push_back(P); siblingOfPart.push_back(sibling);
    }
  }
  // the tables of a mesh whose material reads primvars are sized from its instance count and ids (with a material edit due updateMaterials makes them anew)
  if (sceneDataStale && !(s->dirty & DIRTY_MATERIALS)) remakeSceneData(H);
  // --- the new parts: built on the host here, flattened for the device builder, or cloned from a resident sibling
  const long wantDevice = optionValue("device_build", -1);
  const bool deviceParts = wantDevice < 0 ? s->optBvhBuild == 1 : wantDevice == 1;
  const size_t devicePartsMin = (size_t)std::max(optionValue("device_parts_min", kDevicePartsMinDefault), 1L);
  struct NewPart { bool onDevice = false, ok = true; int64_t sibling = -1; PartBuild built; std::vector<TriRec> flat; DeviceBvhResult dev; };
  std::vector<NewPart> newParts(H.parts.size() - part0);
  const double tb0 = nowMs();
  parallelOver(newParts.size(), [&](size_t k) {
    NewPart& np = newParts[k];
    const InstPart& P = H.parts[part0 + k];
    const MeshBuild& mb = H.meshBuilds[P.meshBuild];
    np.sibling = siblingOfPart[k];
    if (np.sibling >= 0) {
      // a clone: the sibling's records (as the host holds them) under the new instance, by the function k_clone_parts runs over the device's; every triangle
      // must be active by the builders' rule, as on the other routes
      const InstPart& S = H.parts[(size_t)np.sibling];
      np.built.inst = makeInstanceRec(mb.m, mb.meshIdx, P.instInMesh);
      np.ok = usableInstance(np.built.inst);
      np.flat.resize(P.nf);
      for (uint32_t j = 0; j < P.nf && np.ok; j++) {
        const TriRec& src = H.bvh.tris[S.triFirst + j];
        if (src.vi[0] >= H.triShade.size()) { np.ok = false; break; }
        np.flat[j] = refit_clone_record(src, np.built.inst.o2w, H.triShade[src.vi[0]].p, mb.inst[P.instInMesh], mb.idBase + P.instInMesh * P.nf);
        float lo[3], hi[3];
        np.ok = refit_tri_box(np.flat[j].v0, np.flat[j].e1, np.flat[j].e2, lo, hi);
      }
      return;
    }
    np.onDevice = deviceParts && P.nf >= devicePartsMin && P.nf > 128u; // (more than 128 faces: the size from which the scene's own device build runs)
    if (!np.onDevice) { buildPart(mb, P.instInMesh, true, np.built); np.ok = np.built.bvh.activeTris == P.nf; return; }
    // (ids from 0, as buildPart: k_place_part adds the instance's base)
    np.built.inst = makeInstanceRec(mb.m, mb.meshIdx, P.instInMesh);
    np.flat.resize(P.nf);
    flattenInstance(np.built.inst, mb.inst[P.instInMesh], mb.m, mb.vertexOffset, mb.matFlags, 0u, mb.shadeBase, np.flat.data());
    for (const TriRec& t : np.flat) // inactive by the builders' rule (bvh8.cpp prepareRange)
      for (int a = 0; a < 3; a++) np.ok = np.ok && usableCoordinate(t.v0[a]) && usableCoordinate(t.v0[a] + t.e1[a]) && usableCoordinate(t.v0[a] + t.e2[a]);
  });
  for (const NewPart& np : newParts) if (!np.ok) return GI_C_OK; // a fresh build would leave triangles out of the tree
  buildMs += nowMs() - tb0;
  // --- devices, first pass: the arrays grown, what does not depend on node ranges sent, the retired meshes' patch, the device builder over its parts
  std::vector<std::vector<Node8*>> partNodes(nDev, std::vector<Node8*>(newParts.size(), nullptr)); // the builder's blocks, per device
  auto freePartNodes = [&] { for (auto& v : partNodes) for (Node8*& p : v) if (p) { (void)hipFree(p); p = nullptr; } };
  bool outOfMemory = false; double deviceBuildMs = 0.0; uint32_t builtOnDevice = 0; size_t devicePartBytesSent = 0;
  int rc = onSceneDevices(s, nDev, [&](SceneDevice& D, hipStream_t st) -> int {
    if (D.slot >= nDev) { setError("internal: device slot out of range"); return GI_C_ERROR; }
    if (D.dTris.count < oldTris || D.dInstances.count < oldInstances || D.dTriShade.count < shade0 || D.dVerts.count < vert0 || D.dTriFaceId.count < oldTris ||
        D.dNodes.count < node0) { setError("internal: the device holds less than the scene"); return GI_C_ERROR; }
    std::vector<void*> old; DeviceBuffer<VisPatch> dPatch;
    int r = D.dVerts.grow(H.verts.size(), st, old);
    if (r == GI_C_OK) r = D.dTriShade.grow(H.triShade.size(), st, old);
    if (r == GI_C_OK) r = D.dInstances.grow(H.instances.size(), st, old);
    if (r == GI_C_OK) r = D.dTris.grow(H.bvh.tris.size(), st, old);
    if (r == GI_C_OK) r = D.dTriFaceId.grow(H.triFaceId.size(), st, old);
    if (r == GI_C_OUT_OF_MEMORY_INTERNAL) { outOfMemory = true; r = DEVICE_BUILD_FALLBACK; }
    auto copy = [&](void* dst, const void* src, size_t bytes) {
      if (r == GI_C_OK && bytes && hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, st) != hipSuccess) { setError("topology update: copy failed"); r = GI_C_ERROR; } };
    copy(D.dVerts.ptr + vert0, H.verts.data() + vert0, (H.verts.size() - vert0) * sizeof(FVertex));
    copy(D.dTriShade.ptr + shade0, H.triShade.data() + shade0, (H.triShade.size() - shade0) * sizeof(TriShade));
    for (const uint32_t rec : idRecords) copy(D.dInstances.ptr + rec, &H.instances[rec], sizeof(InstanceRec)); // (instance ids of built meshes: rec < oldInstances)
    if (r == GI_C_OK && plan.launch) {
      if (dPatch.upload(plan.patch, st)) r = GI_C_ERROR;
      else launchPatchVisibility(st, D.dTris.ptr, oldTris, D.dInstances.ptr, oldInstances, dPatch.ptr, D.dTriShade.ptr, (uint32_t)H.triShade.size());
    }
    for (size_t k = 0; k < newParts.size() && r == GI_C_OK; k++) {
      NewPart& np = newParts[k];
      if (!np.onDevice) continue;
      const InstPart& P = H.parts[part0 + k];
      const MeshBuild& mb = H.meshBuilds[P.meshBuild];
      if ((size_t)P.triFirst + P.nf > D.dTris.count || (size_t)P.triFirst + P.nf > D.dTriFaceId.count) { setError("internal: part outside the arrays"); r = GI_C_ERROR; break; }
      copy(D.dTris.ptr + P.triFirst, np.flat.data(), (size_t)P.nf * sizeof(TriRec));
      copy(D.dTriFaceId.ptr + P.triFirst, mb.faceIdAov.data(), (size_t)P.nf * sizeof(int32_t));
      if (D.slot == 0u) devicePartBytesSent += (size_t)P.nf * (sizeof(TriRec) + sizeof(int32_t));
      if (r != GI_C_OK) break;
      const double ta = nowMs();
      DeviceBvhResult res;
      const int built = buildBvh8Device(st, D.dTris.ptr + P.triFirst, D.dTriFaceId.ptr + P.triFirst, P.nf, kMaxBvhDepth, res);
      deviceBuildMs += nowMs() - ta;
      if (built == DEVICE_BVH_OUT_OF_MEMORY || built == DEVICE_BVH_TOO_DEEP) {
        // the first device decides for all: buildPart takes the part over (its records are sent anew); a later device that cannot follow gives the edit up
        if (D.slot == 0u) { np.onDevice = false; continue; }
        outOfMemory = true; r = DEVICE_BUILD_FALLBACK; break;
      }
      if (built != DEVICE_BVH_OK) { setError(std::string("device BVH build of an appended part failed: ") + res.error); r = GI_C_ERROR; break; }
      partNodes[D.slot][k] = res.nodes;
      if (res.activeTris != P.nf) { setError("internal: device and host disagree on the inactive triangles of an appended part"); r = GI_C_ERROR; break; }
      if (D.slot == 0u) { np.dev = res; builtOnDevice++; }
      else if (res.nodeCount != np.dev.nodeCount || res.maxDepth != np.dev.maxDepth) { setError("internal: device BVH builds differ between devices"); r = GI_C_ERROR; break; }
    }
    if (r == GI_C_OK && (hipGetLastError() != hipSuccess)) { setError("topology update: launch failed"); r = GI_C_ERROR; }
    if (hipStreamSynchronize(st) != hipSuccess && r == GI_C_OK) { setError("topology update: device error"); r = GI_C_ERROR; }
    dPatch.release();
    for (void* p : old) (void)hipFree(p); // (the copies out of the old blocks are done)
    return r;
  });
  if (rc != GI_C_OK) {
    freePartNodes();
    if (rc == DEVICE_BUILD_FALLBACK && outOfMemory) {
      if (timing) fprintf(stderr, "[gatling_gi] topology update: out of device memory; the scene is rebuilt\n");
      return GI_C_OK;
    }
    return GI_C_ERROR;
  }
  buildMs += deviceBuildMs;
  // --- host: parts the device builder gave back, node ranges at the end of the node array, the parts placed, the top tree
  const double tb1 = nowMs();
  for (size_t k = 0; k < newParts.size(); k++) {
    NewPart& np = newParts[k];
    if (np.onDevice || np.sibling >= 0 || !np.built.bvh.nodes.empty()) continue;
    const InstPart& P = H.parts[part0 + k];
    buildPart(H.meshBuilds[P.meshBuild], P.instInMesh, true, np.built);
    if (np.built.bvh.activeTris != P.nf) { freePartNodes(); return GI_C_OK; }
  }
  buildMs += nowMs() - tb1;
  size_t off = node0;
  for (size_t k = 0; k < newParts.size(); k++) {
    InstPart& P = H.parts[part0 + k];
    const uint32_t n = newParts[k].sibling >= 0 ? H.parts[(size_t)newParts[k].sibling].nodeCount
        : newParts[k].onDevice ? newParts[k].dev.nodeCount : (uint32_t)newParts[k].built.bvh.nodes.size();
    P.nodeOff = (uint32_t)off; P.nodeCap = n + n / 4u + 8u; off += P.nodeCap;
  }
  if (off * sizeof(Node8) >= ((size_t)1 << 32)) { freePartNodes(); return GI_C_OK; } // (the flat walk addresses nodes by 32-bit byte offset)
  H.bvh.nodes.resize(off, Node8{});
  parallelOver(newParts.size(), [&](size_t k) {
    const NewPart& np = newParts[k];
    InstPart& P = H.parts[part0 + k];
    if (np.sibling >= 0) {
      // a clone: the sibling's shape; the records by the kernel's function, in the order the host holds the sibling's; the root and the box follow the
      // device's refit below.  The interior is stale on the host and never read: the only upload of a part's node range follows placePart, which rewrites it
      const InstPart& S = H.parts[(size_t)np.sibling];
      P.nodeCount = S.nodeCount; P.depth = S.depth; P.activeTris = S.activeTris; P.levelStart = S.levelStart;
      for (uint32_t j = 0; j < P.nf; j++) { H.bvh.tris[P.triFirst + j] = np.flat[j]; H.triFaceId[P.triFirst + j] = H.triFaceId[S.triFirst + j]; }
      H.instances[H.meshBuilds[P.meshBuild].inst[P.instInMesh]] = np.built.inst;
      return;
    }
    if (!np.onDevice) { placePart(H, P, np.built); return; }
    // a device-built part: the root (rebased as k_place_part rebases it) for the top tree, the records in scene order with their final ids -- the order
    // differs from the device's leaf order, and nothing uploads these records before a placePart has rewritten them
    const MeshBuild& mb = H.meshBuilds[P.meshBuild];
    P.nodeCount = np.dev.nodeCount; P.depth = np.dev.maxDepth; P.activeTris = np.dev.activeTris; P.levelStart = np.dev.levelStart;
    Node8 root = np.dev.root; root.childBase += P.nodeOff; root.triBase += P.triFirst;
    H.bvh.nodes[P.nodeOff] = root;
    for (uint32_t f = 0; f < P.nf; f++) { TriRec t = np.flat[f]; t.origId += mb.idBase + P.instInMesh * P.nf; H.bvh.tris[P.triFirst + f] = t;
        H.triFaceId[P.triFirst + f] = mb.faceIdAov[f]; }
    H.instances[mb.inst[P.instInMesh]] = np.built.inst;
    nodeBounds(root, P.box);
  });
  // the clones: one table entry each, and the levels of their refit (the sibling's), all clones together in one launch per level
  std::vector<CloneEntry> cloneEntries; std::vector<uint32_t> cloneParts; std::vector<RefitUnit> cloneUnits; uint32_t cloneThreads = 0;
  for (size_t k = 0; k < newParts.size(); k++) {
    if (newParts[k].sibling < 0) continue;
    const InstPart& P = H.parts[part0 + k]; const InstPart& S = H.parts[(size_t)newParts[k].sibling];
    const MeshBuild& mb = H.meshBuilds[P.meshBuild];
    cloneEntries.push_back(CloneEntry{cloneThreads, S.triFirst, P.triFirst, P.nf, S.nodeOff, P.nodeOff, P.nodeCount, mb.inst[P.instInMesh], mb.idBase + P.instInMesh * P.nf});
    cloneThreads += cloneEntryThreads(P.nf, P.nodeCount);
    cloneParts.push_back((uint32_t)(part0 + k)); cloneUnits.push_back(RefitUnit{P.nodeOff, &P.levelStart});
  }
  std::vector<RefitRange> cloneRanges; std::vector<RefitLevel> cloneLevels; std::vector<Node8> cloneRoots(cloneEntries.size());
  if (!planRefitLevels(cloneUnits, (uint32_t)H.bvh.nodes.size(), cloneRanges, cloneLevels)) { freePartNodes(); return GI_C_OK; } // (cannot happen)
  // (with clones the top tree waits for their roots: built and sent behind the second pass)
  if (cloneEntries.empty()) {
    if (rebuildTop(s, H) != GI_C_OK) { freePartNodes(); return GI_C_ERROR; }
    setSceneBounds(s, H.bvh.nodes);
  }
  // (with a material edit due as well the resident words index the previous table: updateMaterials derives the classes behind this update)
  if (!(s->dirty & DIRTY_MATERIALS)) deriveSceneClasses(s, H, false);
  for (const NewMesh& nm : fresh) { nm.m->builtInstances = (uint32_t)(nm.m->instanceTransforms.size() / 16); nm.m->xformDirty = false; nm.m->instDirty.clear(); }
  // (hdGatling calls the visibility setter on every new mesh; a mesh that stays out of the scene has nothing to toggle or refit)
  for (const NewMesh& nm : fresh) { nm.m->visToggled = false; nm.m->vertsEdited = false; }
  for (GiCMesh* m : s->meshes) if (m->builtInstances == 0xffffffffu) { m->visToggled = false; m->vertsEdited = false; }
  s->triCount = (uint32_t)H.bvh.tris.size(); s->nodeCount = (uint32_t)H.bvh.nodes.size();
  size_t partBytesSent = 0; // node, record and face-id bytes the host sent for the new parts, per device (a clone: none)
  // --- devices, second pass: the node array grown, the new ranges, the device-built parts placed, the top tree, the small tables
  rc = onSceneDevices(s, nDev, [&](SceneDevice& D, hipStream_t st) -> int {
    std::vector<void*> old;
    int r = D.dNodes.grow(H.bvh.nodes.size(), st, old);
    if (r == GI_C_OUT_OF_MEMORY_INTERNAL) { outOfMemory = true; r = DEVICE_BUILD_FALLBACK; }
    auto copy = [&](void* dst, const void* src, size_t bytes) {
      if (r == GI_C_OK && bytes && hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, st) != hipSuccess) { setError("topology update: copy failed"); r = GI_C_ERROR; } };
    // (every new node range whole, reserves included: zeros where no node lives; k_place_part then writes the device-built parts over their ranges.  The
    // ranges tile [node0, end).  A CLONE gets nothing from the host per node or per triangle: its range is zeroed where it lives and k_clone_parts fills it)
    if (r == GI_C_OK && D.dNodes.count < H.bvh.nodes.size()) { setError("internal: the device holds less than the scene"); r = GI_C_ERROR; }
    copy(D.dInstances.ptr + oldInstances, H.instances.data() + oldInstances, (H.instances.size() - oldInstances) * sizeof(InstanceRec));
    for (size_t k = 0; k < newParts.size() && r == GI_C_OK; k++) {
      const InstPart& P = H.parts[part0 + k];
      if ((size_t)P.nodeOff + P.nodeCap > D.dNodes.count || P.nodeCount > P.nodeCap || (size_t)P.triFirst + P.nf > D.dTris.count || (size_t)P.triFirst + P.nf > D.dTriFaceId.count) {
        setError("internal: part outside the arrays"); r = GI_C_ERROR; break; }
      if (newParts[k].sibling >= 0) {
        if (hipMemsetAsync(D.dNodes.ptr + P.nodeOff, 0, (size_t)P.nodeCap * sizeof(Node8), st) != hipSuccess) { setError("topology update: memset failed"); r = GI_C_ERROR; }
        continue;
      }
      copy(D.dNodes.ptr + P.nodeOff, &H.bvh.nodes[P.nodeOff], (size_t)P.nodeCap * sizeof(Node8));
      if (D.slot == 0u) partBytesSent += (size_t)P.nodeCap * sizeof(Node8);
      if (newParts[k].onDevice) {
        const MeshBuild& mb = H.meshBuilds[P.meshBuild];
        launchPlacePart(st, partNodes[D.slot][k], P.nodeCount, D.dNodes.ptr, P.nodeOff, D.dTris.ptr, P.triFirst, P.nf, mb.idBase + P.instInMesh * P.nf);
      } else {
        copy(D.dTris.ptr + P.triFirst, &H.bvh.tris[P.triFirst], (size_t)P.nf * sizeof(TriRec));
        copy(D.dTriFaceId.ptr + P.triFirst, &H.triFaceId[P.triFirst], (size_t)P.nf * sizeof(int32_t));
        if (D.slot == 0u) partBytesSent += (size_t)P.nf * (sizeof(TriRec) + sizeof(int32_t));
      }
    }
    // the clones, behind the uploads of the new InstanceRecs and node ranges on the same stream: copied, refitted level by level, the roots read back
    DeviceBuffer<CloneEntry> dClones; DeviceBuffer<RefitRange> dRanges; DeviceBuffer<float> dBoxes;
    if (r == GI_C_OK && !cloneEntries.empty()) {
      const uint32_t nodeCount = (uint32_t)H.bvh.nodes.size(), triCount = (uint32_t)H.bvh.tris.size(), instanceCount = (uint32_t)H.instances.size(),
          shadeCount = (uint32_t)H.triShade.size();
      for (const CloneEntry& c : cloneEntries) // both ranges of every clone inside what the device holds
        if ((size_t)c.srcTri + c.nf > oldTris || (size_t)c.dstTri + c.nf > D.dTris.count || (size_t)c.dstTri + c.nf > D.dTriFaceId.count || (size_t)c.srcNode + c.nodeCount > node0 ||
            (size_t)c.dstNode + c.nodeCount > D.dNodes.count || c.instance >= D.dInstances.count || c.dstTri < oldTris || c.dstNode < node0) {
          setError("internal: clone outside the arrays"); r = GI_C_ERROR; break; }
      if (r == GI_C_OK && (D.dNodes.count < nodeCount || D.dTris.count < triCount || D.dTriShade.count < shadeCount)) { setError("internal: the device holds less than the scene"); r = GI_C_ERROR; }
      if (r == GI_C_OK) {
        const int a = dBoxes.alloc((size_t)nodeCount * 8u), b = a ? a : dClones.alloc(cloneEntries.size()), c = b ? b : dRanges.alloc(cloneRanges.size());
        if (c == GI_C_OUT_OF_MEMORY_INTERNAL) { outOfMemory = true; r = DEVICE_BUILD_FALLBACK; } else if (c != GI_C_OK) r = GI_C_ERROR;
      }
      copy(dClones.ptr, cloneEntries.data(), cloneEntries.size() * sizeof(CloneEntry));
      copy(dRanges.ptr, cloneRanges.data(), cloneRanges.size() * sizeof(RefitRange));
      if (r == GI_C_OK) {
        launchCloneParts(st, dClones.ptr, (uint32_t)cloneEntries.size(), cloneThreads, D.dTris.ptr, triCount, D.dTriFaceId.ptr, D.dNodes.ptr, nodeCount, D.dInstances.ptr,
            instanceCount, D.dTriShade.ptr, shadeCount);
        for (const RefitLevel& lv : cloneLevels) launchRefitLevel(st, D.dNodes.ptr, nodeCount, dBoxes.ptr, dRanges.ptr + lv.first, lv.ranges, lv.threads, D.dTris.ptr,
            triCount, D.dInstances.ptr, instanceCount, D.dTriShade.ptr, shadeCount);
        if (D.slot == 0u) // (the clone and the refit are deterministic: every device holds the same bytes)
          for (size_t k = 0; k < cloneEntries.size() && r == GI_C_OK; k++)
            if (hipMemcpyAsync(&cloneRoots[k], D.dNodes.ptr + cloneEntries[k].dstNode, sizeof(Node8), hipMemcpyDeviceToHost, st) != hipSuccess) {
              setError("topology update: copy failed"); r = GI_C_ERROR; }
      }
    }
    if (r == GI_C_OK && cloneEntries.empty() && uploadTopTree(D, H, st) != GI_C_OK) r = GI_C_ERROR;
    if (r == GI_C_OK && (D.dMeshes.upload(H.meshRecs, st) || D.dSceneData.upload(H.sceneData, st))) r = GI_C_ERROR;
    if (r == GI_C_OK && hipGetLastError() != hipSuccess) { setError("topology update: launch failed"); r = GI_C_ERROR; }
    if (hipStreamSynchronize(st) != hipSuccess && r == GI_C_OK) { setError("topology update: device error"); r = GI_C_ERROR; }
    dClones.release(); dRanges.release(); dBoxes.release(); // (before the render's memory plan reads free memory)
    for (Node8*& p : partNodes[D.slot]) if (p) { (void)hipFree(p); p = nullptr; } // the builder's blocks
    for (void* p : old) (void)hipFree(p);
    return r;
  });
  freePartNodes();
  if (rc == DEVICE_BUILD_FALLBACK && outOfMemory) {
    if (timing) fprintf(stderr, "[gatling_gi] topology update: out of device memory; the scene is rebuilt\n");
    return GI_C_OK;
  }
  if (rc != GI_C_OK) return GI_C_ERROR;
  if (!cloneEntries.empty()) { // the clones' roots and boxes as the device refitted them, then the top tree over all parts
    for (size_t k = 0; k < cloneParts.size(); k++) { InstPart& P = H.parts[cloneParts[k]]; H.bvh.nodes[P.nodeOff] = cloneRoots[k]; nodeBounds(cloneRoots[k], P.box); }
    if (rebuildTop(s, H) != GI_C_OK) return GI_C_ERROR;
    setSceneBounds(s, H.bvh.nodes);
    if (onSceneDevices(s, nDev, [&](SceneDevice& D, hipStream_t st) -> int {
      if (uploadTopTree(D, H, st) != GI_C_OK) return GI_C_ERROR;
      HIP_TRY(hipStreamSynchronize(st));
      return GI_C_OK;
    }) != GI_C_OK) return GI_C_ERROR;
  }
  const double t2 = nowMs();
  cost.buildMs = buildMs; cost.uploadMs = std::max(t2 - t0 - buildMs, 0.0);
  s->resyncCount += adopted;
  if (!instEdits.empty()) {
    s->instanceCounts[0]++; s->instanceCounts[1] += grownParts; s->instanceCounts[2] += cloneEntries.size(); s->instanceCounts[3] += shrunkParts;
    if (timing) fprintf(stderr, "[gatling_gi] instance update: %llu instance(s) retired, %llu appended (%zu cloned, %llu built), %zu instance record(s) re-sent for their ids, "
                                "%u moved, %zu node and record byte(s) sent for the new parts, builds %.2f ms, rest %.2f ms\n", (unsigned long long)shrunkParts,
                        (unsigned long long)grownParts, cloneEntries.size(), (unsigned long long)(grownParts - cloneEntries.size()), idRecords.size(), movedInstances,
                        partBytesSent + devicePartBytesSent, cost.buildMs, cost.uploadMs);
  }
  if (timing) fprintf(stderr, "[gatling_gi] topology update:%s %u mesh(es) retired, %u adopted by their resync, %zu appended, %zu part(s) built, %u of them on the "
                              "device (k_place_part), %llu live + %llu retired triangle(s), %u resident, builds %.2f ms, rest %.2f ms\n", converted
                                  ? " scene re-laid out as per-instance subtrees," : "", retiring, adopted, fresh.size(), newParts.size() - cloneEntries.size(), builtOnDevice,
                      (unsigned long long)live, (unsigned long long)retired, s->triCount, cost.buildMs, cost.uploadMs);
  handled = true;
  return GI_C_OK;
}

// ---------------------------------------------------------------------------------------------------------------
// Transform updates on the two-level layout (opt-in: GI_C_SCENE_OPTION_TLAS_UPDATES / GATLING_OPTIONS=tlas_updates=1).  Instances of a built two-level scene
// moved (giCSetMeshTransform, giCSetMeshInstanceTransforms with the same count); nothing else asked for a rebuild.  Moving an instance is the edit a TLAS is
// for: every BLAS stays, and
//   device, primary, scratch only: the padded world box and the status of every moved instance, from the mesh's resident BLAS triangles under the new
//       transform (gi_tlas.hip k_inst_bounds / k_inst_finish; gi_tlas.h is buildTwoLevel's arithmetic).  28 bytes per moved instance are read back.
//   host: the decision (below), then the TLAS built again over ALL instance boxes by the builder buildTwoLevel uses -- N boxes, not triangles.
//   every device: the moved instances' InstanceRec and InstTrav records in runs, the TLAS nodes and items, and -- the flat tree stays (k_shade reads its
//       records, k_aov and giCTraceRays walk it) -- k_refit_tris over the flat records of the moved instances and k_refit_level over the whole flat tree,
//       deepest level first: what updateVertices does for an unpartitioned tree.  The flat root is read back for the scene bounds.
//   host copies: H.instances and H.two are brought up to date; the flat host tree is dropped as after a vertex refit (H.hostTreeDropped).
// The arrays k_trace_dyn2 walks are then bytewise a fresh build's (giCDebugSceneTlasCheck); the flat tree has the build's topology and conservative boxes, and
// the image is a fresh build's under the traversal contract.
// Declines (handled = false, not an error; the resident scene is untouched but where noted): no host copy or GATLING_OPTIONS=incremental=0 (the caller),
// fewer than kIncrementalMinTris resident triangles, a scene built with inactive triangles, a flat tree without its level table (device-built), a moved
// instance that is unusable (usableInstance) or whose status is set (gi_tlas.h: a corner unusable in object or world space, a flattened triangle the
// builders would leave out), a TLAS too deep for the layout's stack (2 x TLAS depth + BLAS depth + 1 > 16: a fresh build would leave the two-level layout),
// out of device memory for the scratch or the refit's boxes (a later device of several: the earlier ones are committed, and buildScene sends everything anew).
// ---------------------------------------------------------------------------------------------------------------
// What the updates in place of the two-level layout share behind their bounds jobs (updateTransformsTwoLevel, updateVerticesTwoLevel): the padded world
// boxes and statuses of the jobs' instances from the primary device, the TLAS over all boxes with the decision, the plan of the flat tree's refit, the
// per-device commit and the host copies.  On a scene built without the flat tree (SceneHost::treeless, GI_C_SCENE_OPTION_TLAS_ONLY) there is no refit to plan,
// allocate for or launch and no root to read back: k_refit_tris alone keeps the flat records a fresh build's bytes, and the scene bounds are made again from
// the instance boxes (setSceneBoundsFromInstances).
struct TwoLevelEdit {
  std::vector<float> boxes; Bvh8 tlas; std::vector<uint32_t> tlasItems; // all instance boxes with the jobs' new ones; the TLAS over them
  std::vector<uint32_t> editedOfInstance; std::vector<std::pair<uint32_t, uint32_t>> runs; // the jobs' instances: one word each; (first, count) of consecutive ones
  std::vector<RefitRange> ranges; std::vector<RefitLevel> levels; // the flat tree's refit
  double tlasMs = 0.0; TlasMade tlasMade;
};
struct FlatRefitScratch {
  DeviceBuffer<float> boxes; DeviceBuffer<uint32_t> edited; DeviceBuffer<RefitRange> ranges;
  // (a scene without the flat tree -- nodeCount 0 -- has no level to refit: k_refit_tris's table alone)
  int alloc(uint32_t nodeCount, const TwoLevelEdit& E)
  {
    if (nodeCount == 0u) return edited.alloc(E.editedOfInstance.size());
    const int a = boxes.alloc((size_t)nodeCount * 8u), b = a ? a : edited.alloc(E.editedOfInstance.size()); return b ? b : ranges.alloc(E.ranges.size());
  }
  void release() { boxes.release(); edited.release(); ranges.release(); }
};

// primary device, scratch only: padded boxes and statuses, 7 words per job.  scratchTris: the BLAS triangles the jobs name (a vertex edit: the edited meshes'
// records with their new points, which are not resident yet), or null for the resident ones
static int instanceBoundsOnPrimary(GiCScene* s, const std::vector<InstBoundsJob>& jobs, uint32_t chunksPerJob, const std::vector<BlasTri>* scratchTris,
    std::vector<uint32_t>& result, bool& outOfMemory, const char* what)
{
  const uint32_t jobCount = (uint32_t)jobs.size();
  result.assign((size_t)jobCount * 7u, 0u);
  return onSceneDevices(s, 1u, [&](SceneDevice& D, hipStream_t st) -> int {
    const size_t triCount = scratchTris ? scratchTris->size() : s->host->two.blasTris.size();
    if (!scratchTris && D.dBlasTris.count < triCount) { setError("internal: the device holds less than the scene"); return GI_C_ERROR; }
    DeviceBuffer<InstBoundsJob> dJobs; DeviceBuffer<float> dPartials; DeviceBuffer<uint32_t> dOut; DeviceBuffer<BlasTri> dScratch;
    auto releaseAll = [&] { dJobs.release(); dPartials.release(); dOut.release(); dScratch.release(); };
    const int a = dJobs.alloc(jobCount), b = a ? a : dPartials.alloc((size_t)jobCount * chunksPerJob * 8u), c0 = b ? b : dOut.alloc(result.size());
    const int c = c0 ? c0 : (scratchTris && !scratchTris->empty() ? dScratch.alloc(scratchTris->size()) : GI_C_OK);
    if (c != GI_C_OK) { releaseAll(); if (c == GI_C_OUT_OF_MEMORY_INTERNAL) { outOfMemory = true; return DEVICE_BUILD_FALLBACK; } return GI_C_ERROR; }
    int rc = GI_C_OK;
    if (hipMemcpyAsync(dJobs.ptr, jobs.data(), jobs.size() * sizeof(InstBoundsJob), hipMemcpyHostToDevice, st) != hipSuccess) rc = GI_C_ERROR;
    if (rc == GI_C_OK && dScratch.ptr && hipMemcpyAsync(dScratch.ptr, scratchTris->data(), scratchTris->size() * sizeof(BlasTri), hipMemcpyHostToDevice, st) != hipSuccess)
      rc = GI_C_ERROR;
    const BlasTri* tris = scratchTris ? dScratch.ptr : D.dBlasTris.ptr;
    if (rc == GI_C_OK && !launchInstBounds(st, dJobs.ptr, jobCount, chunksPerJob, tris, (uint32_t)triCount, dPartials.ptr, dOut.ptr)) rc = GI_C_ERROR; // (asked by the caller)
    if (rc == GI_C_OK && (hipGetLastError() != hipSuccess ||
        hipMemcpyAsync(result.data(), dOut.ptr, result.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, st) != hipSuccess)) rc = GI_C_ERROR;
    if (hipStreamSynchronize(st) != hipSuccess) rc = GI_C_ERROR;
    if (rc != GI_C_OK) setError(std::string(what) + ": instance bounds failed on the device");
    releaseAll();
    return rc;
  });
}

// The TLAS of an edit in place over `masked` (the instance boxes, hidden / retired / free-slot instances masked): the ONE place the update paths of the
// two-level layout build it.  With GI_C_SCENE_OPTION_TLAS_DEVICE_BUILD wanted the primary device builds it (gi_tlas_build.hip) under the depth budget the
// stack rule leaves beside BLASes of depth `blasDepth`, and the nodes and items are read back -- the caller decides and sends them to every device as it does
// a host-built TLAS, so a decline leaves the scene untouched.  Under tlas_device_min instances, on a tree that does not fit the budget, out of memory or on an
// error status the host builder runs instead (counted in GiCScene::tlasBuildStats): the edit never fails because of the option.
static void noteTlasMade(TwoLevelHost& T, const TlasMade& made) { T.tlasDeviceBuilt = made.device; T.tlasBuildBudget = made.budget; } // (with the committed host copies)
static TlasMade buildEditTlas(GiCScene* s, uint32_t blasDepth, const float* masked, size_t count, Bvh8& tlas, std::vector<uint32_t>& items)
{
  TlasMade made;
  if (tlasDeviceBuildWanted(s)) {
    uint64_t* stats = s->tlasBuildStats;
    uint32_t budget = std::min(tlasDepthBudget(blasDepth), kTlasMaxBudget);
    if (optionSet("tlas_depth_budget")) budget = std::min(budget, (uint32_t)std::max(optionValue("tlas_depth_budget", 0), 0L));
    if ((long)count < optionValue("tlas_device_min", TLAS_DEVICE_MIN_DEFAULT)) stats[4]++;
    else if (count > kTlasMaxItems) stats[3]++;
    else {
      const uint32_t radius = (uint32_t)std::min(std::max(optionValue("ploc_radius", 16), 1L), 256L);
      TlasBuildInfo info; int rc = TLAS_BUILD_ERROR;
      std::vector<Node8> nodes;
      (void)onSceneDevices(s, 1u, [&](SceneDevice& D, hipStream_t st) -> int {
        rc = buildTlasDevice(D.tlasWorkspace, st, masked, (uint32_t)count, budget, radius, nodes, items, info);
        return GI_C_OK;
      });
      if (rc == TLAS_BUILD_OK) {
        tlas = Bvh8{}; tlas.nodes.swap(nodes); tlas.maxDepth = info.maxDepth; tlas.activeTris = info.active;
        stats[0]++;
        for (int k = 0; k < 4; k++) stats[5 + k] = (uint64_t)(info.ms[k] * 1000.0f);
        stats[9] = info.passes; stats[10] = info.hostWaits; stats[11] = info.maxDepth; stats[12] = info.nodeCount;
        made.device = true; made.budget = budget;
        if (getenv("GATLING_BUILD_TIMING")) fprintf(stderr, "[gatling_gi] device TLAS build: %zu boxes, %u node(s), depth %u of %u, %u PLOC pass(es), %u host wait(s); upload + "
            "boxes + sort %.3f ms, PLOC %.3f ms, emission %.3f ms, read-back %.3f ms\n", count, info.nodeCount, info.maxDepth, budget, info.passes, info.hostWaits,
            info.ms[0], info.ms[1], info.ms[2], info.ms[3]);
        return made;
      }
      stats[rc == TLAS_BUILD_TOO_DEEP ? 1 : rc == TLAS_BUILD_OUT_OF_MEMORY ? 2 : 3]++;
      if (getenv("GATLING_BUILD_TIMING")) fprintf(stderr, "[gatling_gi] device TLAS build: %s; the host builder runs\n", rc == TLAS_BUILD_TOO_DEEP ?
          "the tree does not fit the depth budget" : rc == TLAS_BUILD_OUT_OF_MEMORY ? "out of device memory" : info.error);
    }
  }
  buildBvh8Boxes(masked, count, tlas, items);
  return made;
}

// boxes -> TLAS -> decision -> the flat refit's plan.  False: the edit declines (every job's instance must be usable; the TLAS over all boxes must stay
// within the stack rule)
static bool planTwoLevelEdit(const GiCScene* s, const SceneHost& H, const std::vector<InstBoundsJob>& jobs, const std::vector<uint32_t>& result, const char* what,
    bool timing, TwoLevelEdit& E)
{
  const TwoLevelHost& T = H.two;
  const uint32_t jobCount = (uint32_t)jobs.size(), instanceCount = (uint32_t)H.instances.size();
  for (uint32_t k = 0; k < jobCount; k++)
    if (result[7u * k + 6u] != 0u) {
      if (timing) fprintf(stderr, "[gatling_gi] %s: instance %u is not usable after the edit (status %u); the scene is rebuilt\n", what, jobs[k].instance,
                          result[7u * k + 6u]);
      return false;
    }
  E.boxes = T.instBoxes;
  for (uint32_t k = 0; k < jobCount; k++) memcpy(&E.boxes[6u * (size_t)jobs[k].instance], &result[7u * (size_t)k], 24);
  const double t1 = nowMs();
  { // the instances of meshes updateVisibilityTwoLevel hid stay out of the TLAS (E.boxes, the host copy behind the edit, keeps their true boxes)
    const std::vector<uint8_t> hidden = hiddenOfInstances(H.meshBuilds, instanceCount);
    GiCScene* scene = const_cast<GiCScene*>(s); // (the device builder's workspace and counters)
    if (std::find(hidden.begin(), hidden.end(), (uint8_t)1) == hidden.end()) E.tlasMade = buildEditTlas(scene, T.blasDepth, E.boxes.data(), instanceCount, E.tlas, E.tlasItems);
    else {
      std::vector<float> masked(E.boxes);
      tlasMaskHiddenBoxes(masked.data(), hidden.data(), instanceCount);
      E.tlasMade = buildEditTlas(scene, T.blasDepth, masked.data(), instanceCount, E.tlas, E.tlasItems);
    }
  }
  E.tlasMs = nowMs() - t1;
  if (2u * E.tlas.maxDepth + T.blasDepth + 1u > 16u) {
    if (timing) fprintf(stderr, "[gatling_gi] %s: the new TLAS is too deep for the 16-entry stack; the scene is rebuilt\n", what);
    return false;
  }
  E.editedOfInstance.assign(instanceCount, 0u);
  for (uint32_t k = 0; k < jobCount; k++) E.editedOfInstance[jobs[k].instance] = 1u;
  for (uint32_t i = 0; i < instanceCount; i++)
    if (E.editedOfInstance[i]) { if (!E.runs.empty() && E.runs.back().first + E.runs.back().second == i) E.runs.back().second++; else E.runs.emplace_back(i, 1u); }
  if (H.treeless) return true; // (no flat tree: nothing to refit)
  std::vector<RefitUnit> units{RefitUnit{0u, &H.bvh.levelStart}};
  return planRefitLevels(units, s->nodeCount, E.ranges, E.levels); // (false cannot happen: the levels of a tree inside the node array)
}

// one device, behind whatever the edit itself sent on `st`: the instances' records in runs (`instances` may be null: a vertex edit changes none), the TLAS,
// k_refit_tris over the flat records of the edited instances and k_refit_level over the whole flat tree; the primary reads the flat root back.  Not
// synchronised: the caller drains the stream and releases `scratch`
static int commitTwoLevelEdit(GiCScene* s, const SceneHost& H, SceneDevice& D, hipStream_t st, const TwoLevelEdit& E, const std::vector<InstanceRec>* instances,
    const std::vector<InstTrav>& instTrav, FlatRefitScratch& scratch, Node8& root, const char* what)
{
  const uint32_t instanceCount = (uint32_t)H.instances.size(), shadeCount = (uint32_t)H.triShade.size();
  int rc = GI_C_OK;
  auto copy = [&](void* dst, const void* src, size_t bytes, hipMemcpyKind kind) {
    if (rc == GI_C_OK && bytes && hipMemcpyAsync(dst, src, bytes, kind, st) != hipSuccess) { setError(std::string(what) + ": copy failed"); rc = GI_C_ERROR; } };
  for (const auto& r : E.runs) {
    if (instances) copy(D.dInstances.ptr + r.first, &(*instances)[r.first], (size_t)r.second * sizeof(InstanceRec), hipMemcpyHostToDevice);
    copy(D.dInstTrav.ptr + r.first, &instTrav[r.first], (size_t)r.second * sizeof(InstTrav), hipMemcpyHostToDevice);
  }
  if (rc == GI_C_OK && (D.dTlasNodes.upload(E.tlas.nodes, st) || D.dTlasItems.upload(E.tlasItems, st))) rc = GI_C_ERROR;
  copy(scratch.edited.ptr, E.editedOfInstance.data(), E.editedOfInstance.size() * sizeof(uint32_t), hipMemcpyHostToDevice);
  if (!H.treeless) copy(scratch.ranges.ptr, E.ranges.data(), E.ranges.size() * sizeof(RefitRange), hipMemcpyHostToDevice);
  if (rc == GI_C_OK) {
    // (the flat records stay a fresh build's bytes on every scene; the levels and the root belong to the flat tree: a scene without it has neither)
    launchRefitTris(st, D.dTris.ptr, s->triCount, D.dInstances.ptr, instanceCount, scratch.edited.ptr, D.dTriShade.ptr, shadeCount);
    if (!H.treeless) for (const RefitLevel& lv : E.levels) launchRefitLevel(st, D.dNodes.ptr, s->nodeCount, scratch.boxes.ptr, scratch.ranges.ptr + lv.first, lv.ranges, lv.threads,
        D.dTris.ptr, s->triCount, D.dInstances.ptr, instanceCount, D.dTriShade.ptr, shadeCount);
    if (hipGetLastError() != hipSuccess) { setError(std::string(what) + ": launch failed"); rc = GI_C_ERROR; }
  }
  if (D.slot == 0u && !H.treeless) copy(&root, D.dNodes.ptr, sizeof(Node8), hipMemcpyDeviceToHost); // (the refit is deterministic: every device holds the same bytes)
  return rc;
}

// the host copies behind a committed edit: the two-level arrays, the scene bounds; the flat host tree is dropped as after a vertex refit
static void finishTwoLevelEdit(GiCScene* s, SceneHost& H, TwoLevelEdit& E, std::vector<InstTrav>& instTrav, const Node8& root)
{
  TwoLevelHost& T = H.two;
  T.instTrav.swap(instTrav); T.instBoxes.swap(E.boxes); T.tlasNodes.swap(E.tlas.nodes); T.tlasItems.swap(E.tlasItems); T.tlasDepth = E.tlas.maxDepth; noteTlasMade(T, E.tlasMade);
  if (H.treeless) setSceneBoundsFromInstances(s, H); // (the boxes just swapped in; hidden instances stay out, as out of the TLAS)
  else setSceneBounds(s, std::vector<Node8>{root});
  if (!H.hostTreeDropped) {
    std::vector<Node8>().swap(H.bvh.nodes); std::vector<TriRec>().swap(H.bvh.tris); std::vector<int32_t>().swap(H.triFaceId);
    H.hostTreeDropped = true;
  }
}

static int updateTransformsTwoLevel(GiCScene* s, SceneHost& H, bool& handled, UpdateCost& cost)
{
  TwoLevelHost& T = H.two;
  const char* const what = "transform update (two-level)";
  const uint32_t instanceCount = (uint32_t)H.instances.size(), shadeCount = (uint32_t)H.triShade.size();
  if (s->triCount < kIncrementalMinTris || !H.shadePacked || s->stats.inactiveTriangleCount != 0u) return GI_C_OK; // (the floor: resident triangles)
  if (H.deviceBuilt || H.partitioned || (!H.treeless && (H.bvh.levelStart.size() < 2u || H.bvh.levelStart.back() != s->nodeCount))) return GI_C_OK;
  if (T.instTrav.size() != instanceCount || T.instBoxes.size() != 6u * (size_t)instanceCount || T.meshBlasTri.size() != H.meshBuilds.size()) return GI_C_OK; // (cannot happen)
  const bool timing = getenv("GATLING_BUILD_TIMING") != nullptr;
  const double t0 = nowMs();
  // --- the moved instances: their records and one bounds job each
  std::vector<InstBoundsJob> jobs; std::vector<InstanceRec> moved;
  uint32_t chunksPerJob = 0;
  for (const MeshBuild& mb : H.meshBuilds) {
    if (mb.m->builtInstances != mb.instCount) return GI_C_OK; // (cannot happen: count changes raise DIRTY_BVH)
    if (!mb.m->xformDirty) continue;
    const size_t nf = mb.m->faces.size();
    const uint32_t first = T.meshBlasTri[mb.meshIdx];
    // a moved mesh that updateVisibilityTwoLevel hid declines to the rebuild: k_refit_tris would give its flat records their edges back.  (The rest cannot
    // happen on this layout.)
    if (mb.hidden || mb.m->retired || nf >= ((size_t)1 << 26) || (size_t)first + nf > T.blasTris.size()) return GI_C_OK;
    for (uint32_t ii = 0; ii < mb.instCount; ii++) {
      if (!mb.m->instDirty.empty() && !(ii < mb.m->instDirty.size() && mb.m->instDirty[ii])) continue;
      const InstanceRec ir = makeInstanceRec(mb.m, mb.meshIdx, ii);
      if (!usableInstance(ir)) return GI_C_OK;
      InstBoundsJob j{}; memcpy(j.o2w, ir.o2w, sizeof(j.o2w)); j.firstTri = first; j.faceCount = (uint32_t)nf; j.instance = mb.inst[ii];
      if (j.instance >= instanceCount) return GI_C_OK; // (cannot happen)
      jobs.push_back(j); moved.push_back(ir);
      chunksPerJob = std::max(chunksPerJob, instBoundsChunks(j.faceCount));
    }
  }
  const uint32_t jobCount = (uint32_t)jobs.size();
  if (jobCount == 0u) { // the setters were called with the transforms the scene holds
    for (GiCMesh* m : s->meshes) { m->xformDirty = false; m->instDirty.clear(); }
    handled = true;
    return GI_C_OK;
  }
  if ((uint64_t)jobCount * chunksPerJob >= (1ull << 31)) return GI_C_OK; // (more workgroups than a launch takes)
  // --- primary device, scratch only: padded boxes and statuses
  std::vector<uint32_t> result;
  bool outOfMemory = false;
  int rcDev = instanceBoundsOnPrimary(s, jobs, chunksPerJob, nullptr, result, outOfMemory, what);
  if (rcDev == DEVICE_BUILD_FALLBACK && outOfMemory) return GI_C_OK;
  if (rcDev != GI_C_OK) return GI_C_ERROR;
  // --- the decision: every moved instance usable; the TLAS over all boxes within the stack rule; the flat refit's plan
  const double t1 = nowMs();
  TwoLevelEdit E;
  if (!planTwoLevelEdit(s, H, jobs, result, what, timing, E)) return GI_C_OK;
  const double t2 = nowMs();
  // --- the new records
  std::vector<InstanceRec> instances(H.instances); std::vector<InstTrav> instTrav(T.instTrav);
  for (uint32_t k = 0; k < jobCount; k++) {
    const uint32_t i = jobs[k].instance;
    const InstTrav& was = T.instTrav[i]; // (the mesh's constants: a transform changes none; matFlags is the last material update's)
    instances[i] = moved[k]; instTrav[i] = tlasMakeInstTrav(moved[k], was.blasRoot, was.triBase, was.matFlags, was.slack);
  }
  // --- every device of the scene, on its own stream.  The temporaries are allocated before anything resident changes
  Node8 root{}; size_t bytesSent = 0;
  rcDev = onSceneDevices(s, residentDeviceCount(s), [&](SceneDevice& D, hipStream_t st) -> int {
    if (D.dTris.count < s->triCount || D.dNodes.count < s->nodeCount || D.dInstances.count < instanceCount || D.dInstTrav.count < instanceCount ||
        D.dTriShade.count < shadeCount) { setError("internal: the device holds less than the scene"); return GI_C_ERROR; }
    FlatRefitScratch scratch;
    const int c = scratch.alloc(s->nodeCount, E);
    if (c != GI_C_OK) { scratch.release(); if (c == GI_C_OUT_OF_MEMORY_INTERNAL) { outOfMemory = true; return DEVICE_BUILD_FALLBACK; } return GI_C_ERROR; }
    int rc = commitTwoLevelEdit(s, H, D, st, E, &instances, instTrav, scratch, root, what);
    if (hipStreamSynchronize(st) != hipSuccess && rc == GI_C_OK) { setError("transform update (two-level): device error"); rc = GI_C_ERROR; }
    scratch.release(); // (before the render's memory plan reads free memory)
    return rc;
  });
  if (rcDev == DEVICE_BUILD_FALLBACK && outOfMemory) {
    if (timing) fprintf(stderr, "[gatling_gi] transform update (two-level): out of device memory for the refit's boxes; the scene is rebuilt\n");
    return GI_C_OK;
  }
  if (rcDev != GI_C_OK) return GI_C_ERROR;
  // --- the host copies
  bytesSent = (size_t)jobCount * (sizeof(InstBoundsJob) + sizeof(InstanceRec) + sizeof(InstTrav)) + E.tlas.nodes.size() * sizeof(Node8) + E.tlasItems.size() * sizeof(uint32_t) +
      E.editedOfInstance.size() * sizeof(uint32_t) + E.ranges.size() * sizeof(RefitRange);
  const size_t tlasNodeCount = E.tlas.nodes.size(), levelLaunches = E.levels.size();
  H.instances.swap(instances);
  finishTwoLevelEdit(s, H, E, instTrav, root);
  for (GiCMesh* m : s->meshes) { m->xformDirty = false; m->instDirty.clear(); }
  const double t3 = nowMs();
  cost.buildMs = E.tlasMs; cost.uploadMs = std::max(t3 - t0 - cost.buildMs, 0.0);
  if (timing) fprintf(stderr, "[gatling_gi] transform update (two-level): %u instance(s) moved of %u, TLAS %zu node(s) in %u level(s), %zu level launch(es) over the flat "
                              "tree, host TLAS build %.2f ms, bounds kernels + read-back %.2f ms, commit %.2f ms, %zu bytes sent per device\n", jobCount,
                      instanceCount, tlasNodeCount, T.tlasDepth, levelLaunches, E.tlasMs, t1 - t0, t3 - t2, bytesSent);
  handled = true;
  return GI_C_OK;
}

// ---------------------------------------------------------------------------------------------------------------
// Vertex updates on the two-level layout (opt-in: GI_C_SCENE_OPTION_BLAS_UPDATES / GATLING_OPTIONS=blas_updates=1, read with vertex updates wanted).  The
// points of meshes of a built two-level scene moved (giCSetMeshVertices); nothing else asked for a rebuild.  One BLAS is shared by all instances of a mesh,
// so the edit touches nf triangles, not nf x instances; and the walk tests the world-space triangle it rebuilds from BlasTri + InstTrav against the
// world-space ray, so hits do not depend on the BLAS's shape: a BLAS with the build's topology and new conservative boxes gives a fresh build's bits.
//   host: the edited meshes' BlasTri records with their new points, in the builder's order (a copy by prim).
//   device, primary, scratch only: those records are sent to a scratch block and k_inst_bounds / k_inst_finish make the padded world box and the status of
//       EVERY instance of every edited mesh from them (the resident records still hold the old points: every decision is made before the first resident
//       write).  28 bytes per instance are read back.
//   host: the decision -- a set status (OBJECT / WORLD / TRIBOX: the rule a fresh build and the flat refit apply) declines --, the TLAS built again over all
//       instance boxes, the depth rule (the BLAS depth cannot change).
//   every device: the edited meshes' FVertex ranges; k_gather_shade; k_blas_tris; k_blas_refit_level level by level over all edited BLASes (gi_blas.hip);
//       the primary reads the refitted BLAS roots' float boxes back (32 bytes per mesh): the union of the padded face boxes, buildTwoLevel's mlo / mhi up to
//       the sign of a zero, from which InstTrav::slack is formed with buildTwoLevel's expression; then the instances' InstTrav records with the new slack,
//       the TLAS, and k_refit_tris + k_refit_level over the whole flat tree (commitTwoLevelEdit: what a transform update of this layout runs).
//   host copies: H.verts, H.triShade, T.blasTris, T.instTrav, T.instBoxes and the TLAS are brought up to date; the flat host tree is dropped; T.blasNodes keeps
//       the build's topology and stale planes (gi_host.h).
// A refitted BLAS degrades like a refitted flat tree until the next full build.
// Declines (handled = false, not an error; the resident scene is untouched but where noted): what updateVertices and updateTransformsTwoLevel decline for --
// no host copy or incremental=0 (the caller), fewer than kIncrementalMinTris resident triangles, no packed shading records, a scene built with inactive
// triangles, a flat tree that is device-built, partitioned or without its level table, an edited mesh that is not built, hidden, without faces or with
// another instance count, an unusable position, an unusable instance, a set status, the depth rule --, a visibility toggle due in the same sync (it rebuilds
// on this layout), out of device memory (a later device of several: the earlier ones are committed, and buildScene sends everything anew).
// ---------------------------------------------------------------------------------------------------------------
static int updateVerticesTwoLevel(GiCScene* s, SceneHost& H, bool& handled, UpdateCost& cost)
{
  TwoLevelHost& T = H.two;
  const char* const what = "vertex update (two-level)";
  const uint32_t instanceCount = (uint32_t)H.instances.size(), shadeCount = (uint32_t)H.triShade.size();
  const uint32_t blasNodeCount = (uint32_t)T.blasNodes.size(), blasTriCount = (uint32_t)T.blasTris.size();
  if (s->triCount < kIncrementalMinTris || !H.shadePacked || s->stats.inactiveTriangleCount != 0u) return GI_C_OK; // (the floor: resident triangles)
  if (H.deviceBuilt || H.partitioned || (!H.treeless && (H.bvh.levelStart.size() < 2u || H.bvh.levelStart.back() != s->nodeCount))) return GI_C_OK;
  if (T.instTrav.size() != instanceCount || T.instBoxes.size() != 6u * (size_t)instanceCount || T.meshBlasTri.size() != H.meshBuilds.size() ||
      T.meshBlasNode.size() != H.meshBuilds.size() || T.meshBlasLevels.size() != H.meshBuilds.size()) return GI_C_OK; // (cannot happen)
  const bool timing = getenv("GATLING_BUILD_TIMING") != nullptr;
  const double t0 = nowMs();
  // --- which meshes, and may their BLASes be refitted?
  struct Edited { uint32_t build, firstTri, nodeBase, scratchFirst, nf; };
  std::vector<Edited> edited;
  uint32_t scratchCount = 0;
  for (const GiCMesh* m : s->meshes) {
    if (m->visToggled) return GI_C_OK; // (a vertex edit together with a toggle in one sync keeps rebuilding on this layout)
    if (!m->vertsEdited) continue;
    uint32_t b = 0;
    while (b < (uint32_t)H.meshBuilds.size() && H.meshBuilds[b].m != m) b++;
    if (b == (uint32_t)H.meshBuilds.size()) return GI_C_OK; // no records on the device
    const MeshBuild& mb = H.meshBuilds[b];
    const size_t nf = m->faces.size();
    // (an edited mesh that updateVisibilityTwoLevel hid declines to the rebuild: k_refit_tris would give its flat records their edges back)
    if (mb.hidden || m->retired || mb.instCount == 0u || m->builtInstances != mb.instCount || mb.meshIdx >= T.meshBlasTri.size()) return GI_C_OK;
    if ((size_t)mb.vertexOffset + m->vertices.size() > H.verts.size() || nf == 0u || nf >= ((size_t)1 << 26)) return GI_C_OK;
    if (!gatherShadeRangeOk(shadeCount, mb.shadeBase, (uint32_t)nf)) return GI_C_OK; // (a range the kernels would refuse goes to the rebuild, never to stale records)
    const uint32_t first = T.meshBlasTri[mb.meshIdx], nodeBase = T.meshBlasNode[mb.meshIdx];
    const std::vector<uint32_t>& lv = T.meshBlasLevels[mb.meshIdx];
    if (!blasTrisRangeOk(blasTriCount, first, (uint32_t)nf, shadeCount, mb.shadeBase)) return GI_C_OK;
    if (lv.size() < 2u || lv[0] != 0u || (size_t)nodeBase + lv.back() > blasNodeCount) return GI_C_OK; // (cannot happen: the build kept them)
    if (!usableVertexPositions(m->vertices.data(), m->vertices.size())) return GI_C_OK;
    for (uint32_t ii = 0; ii < mb.instCount; ii++) if (mb.inst[ii] >= instanceCount || !usableInstance(H.instances[mb.inst[ii]])) return GI_C_OK;
    edited.push_back(Edited{b, first, nodeBase, scratchCount, (uint32_t)nf});
    scratchCount += (uint32_t)nf;
    if (scratchCount >= (1u << 26)) return GI_C_OK;
  }
  if (edited.empty()) return GI_C_OK;
  // --- the BLAS records with their new points (the builder's order: a copy by prim), one bounds job per instance, the BLAS refit's plan
  std::vector<BlasTri> scratchTris(scratchCount);
  std::vector<InstBoundsJob> jobs; uint32_t chunksPerJob = 0;
  std::vector<RefitUnit> units;
  for (const Edited& e : edited) {
    const MeshBuild& mb = H.meshBuilds[e.build];
    const GiCMesh* m = mb.m;
    std::atomic<bool> primOk{true};
    constexpr size_t CHUNK = 4096;
    parallelOver(((size_t)e.nf + CHUNK - 1) / CHUNK, [&](size_t c) {
      for (size_t i = c * CHUNK; i < std::min((size_t)e.nf, (c + 1) * CHUNK); i++) {
        BlasTri bt = T.blasTris[e.firstTri + i];
        if (bt.prim >= e.nf) { primOk = false; return; } // (cannot happen)
        const GiCFace& f = m->faces[bt.prim];
        memcpy(bt.p0, m->vertices[f.v_i[0]].pos, 12); memcpy(bt.p1, m->vertices[f.v_i[1]].pos, 12); memcpy(bt.p2, m->vertices[f.v_i[2]].pos, 12);
        scratchTris[e.scratchFirst + i] = bt;
      }
    });
    if (!primOk) return GI_C_OK;
    for (uint32_t ii = 0; ii < mb.instCount; ii++) {
      InstBoundsJob j{}; memcpy(j.o2w, H.instances[mb.inst[ii]].o2w, sizeof(j.o2w)); j.firstTri = e.scratchFirst; j.faceCount = e.nf; j.instance = mb.inst[ii];
      jobs.push_back(j);
    }
    chunksPerJob = std::max(chunksPerJob, instBoundsChunks(e.nf));
    units.push_back(RefitUnit{e.nodeBase, &T.meshBlasLevels[mb.meshIdx]});
  }
  const uint32_t jobCount = (uint32_t)jobs.size();
  if ((uint64_t)jobCount * chunksPerJob >= (1ull << 31)) return GI_C_OK; // (more workgroups than a launch takes)
  std::vector<RefitRange> blasRanges; std::vector<RefitLevel> blasLevels;
  if (!planRefitLevels(units, blasNodeCount, blasRanges, blasLevels)) return GI_C_OK; // (cannot happen: the levels of BLASes inside the node array)
  // --- primary device, scratch only: padded boxes and statuses of every instance of every edited mesh
  std::vector<uint32_t> result;
  bool outOfMemory = false;
  const double tA = nowMs();
  int rcDev = instanceBoundsOnPrimary(s, jobs, chunksPerJob, &scratchTris, result, outOfMemory, what);
  if (rcDev == DEVICE_BUILD_FALLBACK && outOfMemory) return GI_C_OK;
  if (rcDev != GI_C_OK) return GI_C_ERROR;
  // --- the decision; from here on nothing declines but out of device memory
  const double t1 = nowMs();
  TwoLevelEdit E;
  if (!planTwoLevelEdit(s, H, jobs, result, what, timing, E)) return GI_C_OK;
  const double tP = nowMs();
  // --- host: the edited meshes' vertex and shading records, as updateVertices makes them
  for (const Edited& e : edited) {
    const MeshBuild& mb = H.meshBuilds[e.build];
    constexpr size_t CHUNK = 4096;
    const size_t nv = mb.m->vertices.size(), nf = e.nf;
    parallelOver((nv + CHUNK - 1) / CHUNK, [&](size_t c) {
      for (size_t i = c * CHUNK; i < std::min(nv, (c + 1) * CHUNK); i++) H.verts[mb.vertexOffset + i] = packVertex(mb.m->vertices[i]); });
    parallelOver((nf + CHUNK - 1) / CHUNK, [&](size_t c) {
      for (size_t f = c * CHUNK; f < std::min(nf, (c + 1) * CHUNK); f++) refit_gather_shade(H.verts.data(), (uint32_t)H.verts.size(), H.triShade[mb.shadeBase + f]); });
  }
  const double t2 = nowMs();
  // --- every device of the scene, on its own stream.  The temporaries are allocated before anything resident changes
  Node8 root{}; std::vector<InstTrav> instTrav(T.instTrav); std::vector<float> rootBoxes(8u * edited.size(), 0.0f);
  rcDev = onSceneDevices(s, residentDeviceCount(s), [&](SceneDevice& D, hipStream_t st) -> int {
    if (D.dTris.count < s->triCount || D.dNodes.count < s->nodeCount || D.dInstances.count < instanceCount || D.dInstTrav.count < instanceCount ||
        D.dTriShade.count < shadeCount || D.dVerts.count < H.verts.size() || D.dBlasTris.count < blasTriCount || D.dBlasNodes.count < blasNodeCount) {
      setError("internal: the device holds less than the scene"); return GI_C_ERROR; }
    FlatRefitScratch scratch; DeviceBuffer<float> dBlasBoxes; DeviceBuffer<RefitRange> dBlasRanges;
    auto releaseAll = [&] { scratch.release(); dBlasBoxes.release(); dBlasRanges.release(); };
    const int a = scratch.alloc(s->nodeCount, E), b = a ? a : dBlasBoxes.alloc((size_t)blasNodeCount * 8u), c = b ? b : dBlasRanges.alloc(blasRanges.size());
    if (c != GI_C_OK) { releaseAll(); if (c == GI_C_OUT_OF_MEMORY_INTERNAL) { outOfMemory = true; return DEVICE_BUILD_FALLBACK; } return GI_C_ERROR; }
    int rc = GI_C_OK;
    auto copy = [&](void* dst, const void* src, size_t bytes, hipMemcpyKind kind) {
      if (rc == GI_C_OK && bytes && hipMemcpyAsync(dst, src, bytes, kind, st) != hipSuccess) { setError("vertex update (two-level): copy failed"); rc = GI_C_ERROR; } };
    for (const Edited& e : edited) {
      const MeshBuild& mb = H.meshBuilds[e.build];
      copy(D.dVerts.ptr + mb.vertexOffset, &H.verts[mb.vertexOffset], mb.m->vertices.size() * sizeof(FVertex), hipMemcpyHostToDevice);
    }
    copy(dBlasRanges.ptr, blasRanges.data(), blasRanges.size() * sizeof(RefitRange), hipMemcpyHostToDevice);
    // (behind the vertex uploads on the same stream: the shading records, then the BLAS records that read TriShade::p, then the BLAS levels)
    if (rc == GI_C_OK) for (const Edited& e : edited) {
      const MeshBuild& mb = H.meshBuilds[e.build];
      if (!launchGatherShade(st, D.dTriShade.ptr, shadeCount, mb.shadeBase, e.nf, D.dVerts.ptr, (uint32_t)H.verts.size()) ||
          !launchBlasTris(st, D.dBlasTris.ptr, blasTriCount, e.firstTri, e.nf, D.dTriShade.ptr, shadeCount, mb.shadeBase)) {
        setError("internal: an edited mesh's records outside their arrays"); rc = GI_C_ERROR; break; } // (cannot happen: asked above)
    }
    if (rc == GI_C_OK) {
      for (const RefitLevel& lv : blasLevels) launchBlasRefitLevel(st, D.dBlasNodes.ptr, blasNodeCount, dBlasBoxes.ptr, dBlasRanges.ptr + lv.first, lv.ranges,
          lv.threads, D.dBlasTris.ptr, blasTriCount);
      if (hipGetLastError() != hipSuccess) { setError("vertex update (two-level): launch failed"); rc = GI_C_ERROR; }
    }
    if (D.slot == 0u) { // (the refit is deterministic: every device holds the same bytes) the BLAS roots' float boxes -> the meshes' object-space magnitude
      for (size_t k = 0; k < edited.size(); k++) copy(&rootBoxes[8u * k], dBlasBoxes.ptr + 8u * (size_t)edited[k].nodeBase, 32u, hipMemcpyDeviceToHost);
      if (rc == GI_C_OK && hipStreamSynchronize(st) != hipSuccess) { setError("vertex update (two-level): device error"); rc = GI_C_ERROR; }
      if (rc == GI_C_OK) for (size_t k = 0; k < edited.size(); k++) {
        const float* lo = &rootBoxes[8u * k]; const float* hi = lo + 4;
        const float extent = (std::fabs(lo[0]) + std::fabs(lo[1]) + std::fabs(lo[2])) + (std::fabs(hi[0]) + std::fabs(hi[1]) + std::fabs(hi[2])); // (buildTwoLevel's)
        const MeshBuild& mb = H.meshBuilds[edited[k].build];
        for (uint32_t ii = 0; ii < mb.instCount; ii++) instTrav[mb.inst[ii]].slack = extent; // (the matrices, blasRoot, triBase and matFlags stay)
      }
    }
    if (rc == GI_C_OK) rc = commitTwoLevelEdit(s, H, D, st, E, nullptr, instTrav, scratch, root, what);
    if (hipStreamSynchronize(st) != hipSuccess && rc == GI_C_OK) { setError("vertex update (two-level): device error"); rc = GI_C_ERROR; }
    releaseAll(); // (before the render's memory plan reads free memory)
    return rc;
  });
  if (rcDev == DEVICE_BUILD_FALLBACK && outOfMemory) {
    if (timing) fprintf(stderr, "[gatling_gi] vertex update (two-level): out of device memory for the refits' boxes; the scene is rebuilt\n");
    return GI_C_OK;
  }
  if (rcDev != GI_C_OK) return GI_C_ERROR;
  // --- the host copies
  size_t bytesSent = scratchTris.size() * sizeof(BlasTri) /* the primary alone */ + (size_t)jobCount * (sizeof(InstBoundsJob) + sizeof(InstTrav)) +
      E.tlas.nodes.size() * sizeof(Node8) + E.tlasItems.size() * sizeof(uint32_t) + E.editedOfInstance.size() * sizeof(uint32_t) +
      (E.ranges.size() + blasRanges.size()) * sizeof(RefitRange);
  for (const Edited& e : edited) {
    bytesSent += H.meshBuilds[e.build].m->vertices.size() * sizeof(FVertex);
    std::copy(scratchTris.begin() + e.scratchFirst, scratchTris.begin() + e.scratchFirst + e.nf, T.blasTris.begin() + e.firstTri);
  }
  const size_t tlasNodeCount = E.tlas.nodes.size(), flatLaunches = E.levels.size();
  finishTwoLevelEdit(s, H, E, instTrav, root);
  const double t3 = nowMs();
  cost.buildMs = E.tlasMs; cost.uploadMs = std::max(t3 - t0 - cost.buildMs, 0.0);
  if (timing) fprintf(stderr, "[gatling_gi] vertex update (two-level): %zu mesh(es), %zu BLAS level launch(es), %u instance(s) re-bounded of %u, TLAS %zu node(s), "
                              "%zu level launch(es) over the flat tree, host %.2f ms (records + plans %.2f, TLAS build %.2f, vertex packing %.2f), device %.2f ms "
                              "(bounds kernels + read-back %.2f, refits + commit %.2f), %zu bytes sent to the primary device\n", edited.size(), blasLevels.size(),
                      jobCount, instanceCount, tlasNodeCount, flatLaunches, (tA - t0) + (t2 - t1), (tA - t0) + (tP - t1 - E.tlasMs), E.tlasMs, t2 - tP, (t1 - tA) + (t3 - t2),
                      t1 - tA, t3 - t2, bytesSent);
  handled = true;
  return GI_C_OK;
}

// ---------------------------------------------------------------------------------------------------------------
// Instancer edits on the two-level layout (opt-in: GI_C_SCENE_OPTION_TLAS_INSTANCES / GATLING_OPTIONS=tlas_instances=1, read with topology, instance and
// two-level topology updates wanted, on a scene built without the flat tree).  Instance ids or counts of built meshes changed (GiCMesh::instEdited): the
// delegate's answer to every DirtyInstancer / DirtyInstanceIndex sync.  The BLAS of a built mesh is resident and shared by its instances, so one more
// instance costs one InstanceRec, one InstTrav, one box in the TLAS and nf flat records.  updateTopologyTwoLevel runs this in front of its other work, with
// the semantics instance updates have on the flat layouts (above instanceUpdatesWanted):
//   ids:     InstanceRec::instanceId of the kept instances whose id changed is set and those records are re-sent; equal ids send nothing.
//   moves:   a kept instance whose transform differs from the resident record is marked in GiCMesh::instDirty and DIRTY_XFORM is raised:
//            updateTransformsTwoLevel applies it behind this update.  Without GI_C_SCENE_OPTION_TLAS_UPDATES wanted a sync with a move declines.
//   shrink:  the instances [new, old) retire as the instances of a hidden mesh do -- VIS_HIDE | VIS_HIDDEN_AFTER in their VisPatch: both edges zeroed, no
//            id-table word; masked out of the TLAS --, the kept instances of the meshes behind are renumbered by the plan (idDelta; k_patch_visibility2 and
//            k_patch_inst_trav), and their SLOTS -- InstanceRec / InstTrav index and nf flat records -- go on the mesh's free list (MeshBuild::freeSlots).
//            They count as retired triangles in updateTopologyTwoLevel's retired > live rule until they are reused.
//   grow:    the instances [old, new) take free slots of the SAME mesh first, lowest index first -- never one retired in this very sync --, then the ends of
//            the arrays (DeviceBuffer::grow).  Per new instance the host makes and sends the InstanceRec, the InstTrav (blasRoot and slack of a live sibling,
//            triBase = the mesh's new id base + instance-in-mesh x nf) and one 32-byte job; per mesh that grows the per-FACE faceIdAov table once.  The world
//            boxes and statuses come from k_inst_bounds / k_inst_finish over the RESIDENT BLAS triangles (instanceBoundsOnPrimary, scratch outputs only)
//            before anything resident changes; a set status declines.  The TLAS is built again over all boxes, hidden and free slots masked, and held to
//            the 16-entry stack rule.  k_instance_records (gi_instances.hip) makes the flat records, face-id words and id-table words of all new instances of
//            all meshes in ONE launch: an instancer that goes up and down reuses its slots instead of leaving a retired range behind per frame.
//   scene data: a mesh whose material reads primvars gets the MeshRec / scene-data tables made again (with a material edit due updateMaterials makes them).
// MeshBuild::inst / instTri name the InstanceRec and the first flat record of every live instance: a mesh's records are no longer one run.  The paths of
// options 16 - 18 and 20 address records through TriRec::instance and MeshBuild::inst alone; everything that masks hidden instances masks free slots too
// (hiddenOfInstances, markFreeSlots, retiredRangesOf).  Host copies: H.instances, T.instTrav, T.instBoxes and the TLAS are brought up to date; the flat
// records, face ids and id table where the host still holds them are written by the kernels' own host forms (vis2_patch_record, instanceRecordsHost), and stay
// dropped where an edit in place dropped them.
// Every decision comes before the first resident write.  Declines (applied = false, not an error, one line under GATLING_BUILD_TIMING; the caller rebuilds):
// what updateTopologyTwoLevel declines for on the scene as it is, a new count of 0, a mesh hidden by the visibility path, a built mesh without an instance
// (it has no BLAS), an unusable transform of a new instance, a move without option 16, a set status, the depth rule, 2^28 flat records, fewer than
// kIncrementalMinTris visible triangles, more retired than live triangles, out of device memory.
// ---------------------------------------------------------------------------------------------------------------
bool tlasDeviceBuildWanted(const GiCScene* s)
{
  const long o = optionValue("tlas_device_build", -1);
  return o >= 0 ? o == 1 : s->optTlasDeviceBuild == 1;
}

bool tlasInstancesWanted(const GiCScene* s)
{
  if (!instanceUpdatesWanted(s) || !tlasTopologyWanted(s)) return false;
  const long o = optionValue("tlas_instances", -1);
  return o >= 0 ? o == 1 : s->optTlasInstances == 1;
}

// ---------------------------------------------------------------------------------------------------------------
// Compaction of the retired ranges of a two-level scene without the flat tree (opt-in: GI_C_SCENE_OPTION_TLAS_COMPACTION / GATLING_OPTIONS=tlas_compaction=1;
// read where updateTopologyTwoLevel or updateInstancesTwoLevel is about to apply an edit and retired x 100 > live x tlas_compact_percent holds on the planned
// after-edit counts: compactBeforeEdit below).  Those edits retire by hiding: the vertex, shading, BLAS, instance and flat records of a destroyed mesh and
// the slots of retired instances stay resident, and once they outnumber the live records the edit declines and the scene is rebuilt.  Here they leave:
//   dropped: every MeshBuild retired by an EARLIER sync (m->retired && hidden) with all its ranges; every free instance slot with its flat records.
//   kept:    live meshes, meshes hidden by the visibility path, meshes the current sync retires (still visible resident records: the edit that follows
//            retires them as ever).  Storage order is preserved; nothing is sorted back into scene order, and scene-order ids do not change.
//   device:  one range table per array kind (gi_compact.h CompactTable: runs of kept items with equal deltas are one range) and ONE launch per kind
//            (gi_compact.hip) into NEW allocations sized as DeviceBuffer::grow sizes them, which are swapped in behind the launches -- FVertex, BlasTri and
//            face-id words moved; TriShade::vi, Node8::childBase / triBase, InstanceRec::mesh, InstTrav::blasRoot, TriRec::instance / vi rebased; the new
//            id table written by the flat records' own lanes.  The new blocks of EVERY device are allocated before the first resident change: out of
//            memory declines with nothing touched.  The old blocks are freed before the render's memory plan reads free memory.  Host waits: one stream
//            synchronisation per device whatever the scene size (two on the primary under GATLING_BUILD_TIMING), plus those of the device TLAS builder
//            where GI_C_SCENE_OPTION_TLAS_DEVICE_BUILD is wanted.
//   host:    the MeshBuilds renumbered (meshIdx == index again; inst / instTri renamed, free lists emptied, vertexOffset / shadeBase / instFirst / triFirst
//            moved), H.verts, H.triShade, H.instances, the BLAS arrays, the traversal records and -- where still held -- the flat records, face ids and id
//            table WHERE THEY LIE through the kernel's per-piece form (a stable compaction moves towards the front: ranges that stay are not touched); the
//            instance boxes; MeshRec and the scene-data tables made again (appendBuiltMeshSceneData); the TLAS by
//            buildEditTlas over the compacted boxes, hidden instances masked; blasDepth over the kept meshes; retired GiCMeshes nothing names any more freed.
// Declines (compacted = false, not an error, counted, one line under GATLING_BUILD_TIMING; the scene is untouched and the caller goes on as without the
// option): whatever updateTopologyTwoLevel declines for on the scene as it is; a count that does not add up; a TLAS too deep; out of device memory.
// With nothing to drop the call is a no-op and is not counted.
// ---------------------------------------------------------------------------------------------------------------
bool tlasCompactionWanted(const GiCScene* s)
{
  const long o = optionValue("tlas_compaction", -1);
  return o >= 0 ? o == 1 : s->optTlasCompaction == 1;
}

static int compactTwoLevel(GiCScene* s, SceneHost& H, bool& compacted, UpdateCost& cost)
{
  compacted = false;
  TwoLevelHost& T = H.two;
  const bool timing = getenv("GATLING_BUILD_TIMING") != nullptr;
  auto decline = [&](const char* why) { s->compactionStats[3]++; if (timing) fprintf(stderr, "[gatling_gi] compaction (two-level): %s; nothing is moved\n", why); return GI_C_OK; };
  const char* const mismatch = "a count of the host copy does not add up";
  const uint32_t oldInstances = (uint32_t)H.instances.size(), oldTris = s->triCount, oldShade = (uint32_t)H.triShade.size(), oldVerts = (uint32_t)H.verts.size();
  const uint32_t oldBlasNodes = (uint32_t)T.blasNodes.size(), oldBlasTris = (uint32_t)T.blasTris.size(), oldMeshes = (uint32_t)H.meshBuilds.size();
  // --- what leaves: nothing, and this is not a compaction
  std::vector<uint8_t> keep(oldMeshes, 1); std::vector<uint32_t> newMeshIdx(oldMeshes, 0xffffffffu);
  uint32_t keptMeshes = 0; uint64_t droppedTris = 0;
  for (uint32_t b = 0; b < oldMeshes; b++) {
    const MeshBuild& mb = H.meshBuilds[b];
    const uint64_t nf = mb.m->faces.size();
    keep[b] = !(mb.m->retired && mb.hidden);
    if (keep[b]) { newMeshIdx[b] = keptMeshes++; droppedTris += mb.freeSlots.size() * nf; } else droppedTris += (mb.instCount + mb.freeSlots.size()) * nf;
  }
  if (keptMeshes == oldMeshes && droppedTris == 0u) return GI_C_OK;
  // --- the scene as updateTopologyTwoLevel wants it
  if (s->stats.inactiveTriangleCount != 0u) return decline("the scene was built with inactive triangles");
  if (H.deviceBuilt || H.partitioned || !H.treeless || !H.shadePacked || H.reordered) return decline("the scene is not a two-level scene without the flat tree");
  if (T.instTrav.size() != oldInstances || T.instBoxes.size() != 6u * (size_t)oldInstances || T.meshBlasTri.size() != oldMeshes || T.meshBlasNode.size() != oldMeshes ||
      T.meshBlasLevels.size() != oldMeshes || H.meshRecs.size() != oldMeshes) return decline("the host copy is not the built scene's"); // (cannot happen)
  for (const MeshBuild& mb : H.meshBuilds)
    if (mb.inst.size() != mb.instCount || mb.instTri.size() != mb.instCount || mb.meshIdx != (uint32_t)(&mb - H.meshBuilds.data())) return decline(mismatch); // (cannot happen)
  const double t0 = nowMs();
  // --- the per-mesh arrays, in storage order: every range must lie where the ranges before it end
  CompactTable tVerts(COMPACT_VERTS), tShade(COMPACT_SHADE), tNodes(COMPACT_BLAS_NODES), tBlasTris(COMPACT_BLAS_TRIS), tInst(COMPACT_INSTANCES), tTrav(COMPACT_INST_TRAV),
      tTris(COMPACT_TRIS), tWords(COMPACT_WORDS);
  struct Place { uint32_t vertexOffset = 0, shadeBase = 0, blasNode = 0, blasTri = 0; };
  std::vector<Place> place(oldMeshes);
  uint32_t blasDepth = 0;
  {
    uint64_t vAt = 0, sAt = 0, nAt = 0, bAt = 0;
    for (uint32_t b = 0; b < oldMeshes; b++) {
      const MeshBuild& mb = H.meshBuilds[b];
      const std::vector<uint32_t>& lv = T.meshBlasLevels[b];
      const uint64_t nv = mb.m->vertices.size(), nf = mb.m->faces.size(), nn = lv.empty() ? 0u : lv.back();
      if (mb.vertexOffset != vAt || mb.shadeBase != sAt || vAt + nv > oldVerts || sAt + nf > oldShade) return decline(mismatch);
      if (lv.empty() ? mb.instCount != 0u : (lv.size() < 2u || T.meshBlasNode[b] != nAt || T.meshBlasTri[b] != bAt || nAt + nn > oldBlasNodes || bAt + nf > oldBlasTris)) return decline(mismatch);
      if (keep[b]) {
        Place& P = place[b];
        P.vertexOffset = tVerts.Z.dstCount; P.shadeBase = tShade.Z.dstCount; P.blasNode = tNodes.Z.dstCount; P.blasTri = tBlasTris.Z.dstCount;
        tVerts.add((uint32_t)vAt, (uint32_t)nv);
        tShade.add((uint32_t)sAt, (uint32_t)nf, P.vertexOffset - (uint32_t)vAt);
        if (!lv.empty()) {
          tNodes.add((uint32_t)nAt, (uint32_t)nn, P.blasNode - (uint32_t)nAt, P.blasTri - (uint32_t)bAt);
          tBlasTris.add((uint32_t)bAt, (uint32_t)nf);
          blasDepth = std::max(blasDepth, (uint32_t)lv.size() - 1u); // (Bvh8::levelStart: maxDepth + 1 entries)
        }
      }
      vAt += nv; sAt += nf; if (!lv.empty()) { nAt += nn; bAt += nf; }
    }
    if (vAt != oldVerts || sAt != oldShade || nAt != oldBlasNodes || bAt != oldBlasTris) return decline(mismatch);
  }
  // --- the instance slots: every slot is a live instance's or a free one, once; the kept ones keep their order
  constexpr uint32_t NONE = 0xffffffffu;
  std::vector<uint32_t> slotMesh(oldInstances, NONE), newSlot(oldInstances, NONE), newTriOfSlot(oldInstances, NONE);
  {
    std::vector<uint8_t> seen(oldInstances, 0); uint64_t slots = 0;
    auto take = [&](uint32_t slot) { if (slot >= oldInstances || seen[slot]) return false; seen[slot] = 1; slots++; return true; };
    for (uint32_t b = 0; b < oldMeshes; b++) {
      const MeshBuild& mb = H.meshBuilds[b];
      for (const uint32_t slot : mb.inst) { if (!take(slot)) return decline(mismatch); if (keep[b]) slotMesh[slot] = b; }
      for (const MeshBuild::FreeSlot& fs : mb.freeSlots) if (!take(fs.inst)) return decline(mismatch);
    }
    if (slots != oldInstances) return decline(mismatch);
  }
  for (uint32_t slot = 0; slot < oldInstances; slot++) {
    const uint32_t b = slotMesh[slot];
    if (b == NONE) continue;
    if (H.instances[slot].mesh != b) return decline(mismatch); // (cannot happen)
    newSlot[slot] = tInst.Z.dstCount;
    tInst.add(slot, 1u, newMeshIdx[b] - b);
    tTrav.add(slot, 1u, place[b].blasNode - T.meshBlasNode[b]);
  }
  // --- the flat records: one run per kept instance, in the order they lie; with the runs of what leaves they cover the array
  struct Run { uint32_t src, nf, slot, b; };
  std::vector<Run> runs;
  {
    uint64_t covered = 0;
    for (uint32_t b = 0; b < oldMeshes; b++) {
      const MeshBuild& mb = H.meshBuilds[b];
      const uint64_t nf = mb.m->faces.size();
      if (nf >= ((uint64_t)1 << 26)) return decline(mismatch); // (cannot happen)
      covered += (mb.instCount + mb.freeSlots.size()) * nf;
      if (keep[b]) for (uint32_t ii = 0; ii < mb.instCount; ii++) runs.push_back(Run{mb.instTri[ii], (uint32_t)nf, mb.inst[ii], b});
    }
    if (covered != oldTris) return decline(mismatch);
    std::sort(runs.begin(), runs.end(), [](const Run& a, const Run& c) { return a.src < c.src; });
    uint64_t end = 0;
    for (const Run& r : runs) {
      if (r.src < end || (uint64_t)r.src + r.nf > oldTris) return decline(mismatch);
      end = (uint64_t)r.src + r.nf;
      const MeshBuild& mb = H.meshBuilds[r.b];
      newTriOfSlot[r.slot] = tTris.Z.dstCount;
      tTris.add(r.src, r.nf, newSlot[r.slot] - r.slot, place[r.b].shadeBase - mb.shadeBase, place[r.b].vertexOffset - mb.vertexOffset, mb.hidden ? COMPACT_RANGE_HIDDEN : 0u);
      tWords.add(r.src, r.nf);
    }
  }
  const uint32_t newInstances = tInst.Z.dstCount, newTris = tTris.Z.dstCount;
  if (newInstances == 0u || newTris == 0u) return decline("nothing would stay");
  if (!tVerts.finish(oldVerts, 0u) || !tShade.finish(oldShade, 0u) || !tNodes.finish(oldBlasNodes, 0u) || !tBlasTris.finish(oldBlasTris, 0u) || !tInst.finish(oldInstances, 0u) ||
      !tTrav.finish(oldInstances, 0u) || !tTris.finish(oldTris, newTris) || !tWords.finish(oldTris, 0u)) return decline("a range table does not pass its check"); // (cannot happen)
  CompactTable* const tables[8] = {&tVerts, &tShade, &tNodes, &tBlasTris, &tInst, &tTrav, &tTris, &tWords};
  uint64_t movedRecords = 0; size_t rangeCount = 0;
  for (const CompactTable* t : tables) { movedRecords += t->Z.dstCount; rangeCount += t->ranges.size(); }
  // --- the MeshBuilds after the compaction (staged), and the tables that are made from them
  std::vector<MeshBuild> meshBuilds; meshBuilds.reserve(keptMeshes);
  std::vector<uint32_t> meshBlasTri, meshBlasNode, meshBlasBudget; std::vector<std::vector<uint32_t>> meshBlasLevels;
  {
    std::vector<uint32_t> keptSlotsBelow(oldInstances + 1u, 0u); // for a mesh without an instance: where its (empty) runs would lie
    for (uint32_t slot = 0; slot < oldInstances; slot++) keptSlotsBelow[slot + 1u] = keptSlotsBelow[slot] + (newSlot[slot] != NONE ? 1u : 0u);
    for (uint32_t b = 0; b < oldMeshes; b++) {
      if (!keep[b]) continue;
      MeshBuild nb = H.meshBuilds[b];
      nb.meshIdx = newMeshIdx[b]; nb.vertexOffset = place[b].vertexOffset; nb.shadeBase = place[b].shadeBase;
      for (uint32_t ii = 0; ii < nb.instCount; ii++) { const uint32_t slot = nb.inst[ii]; nb.inst[ii] = newSlot[slot]; nb.instTri[ii] = newTriOfSlot[slot]; }
      nb.freeSlots.clear(); nb.retiredInst = 0u;
      if (nb.instCount != 0u) { nb.instFirst = nb.inst[0]; nb.triFirst = nb.instTri[0]; }
      else {
        nb.instFirst = keptSlotsBelow[std::min(nb.instFirst, oldInstances)];
        const auto it = std::lower_bound(runs.begin(), runs.end(), nb.triFirst, [](const Run& r, uint32_t x) { return r.src < x; });
        nb.triFirst = it == runs.end() ? newTris : newTriOfSlot[it->slot];
      }
      meshBuilds.push_back(std::move(nb));
      meshBlasTri.push_back(place[b].blasTri); meshBlasNode.push_back(place[b].blasNode); meshBlasLevels.push_back(T.meshBlasLevels[b]);
      meshBlasBudget.push_back(b < T.meshBlasBudget.size() ? T.meshBlasBudget[b] : 0u);
    }
  }
  std::vector<MeshRec> meshRecs; std::vector<float> sceneData;
  for (const MeshBuild& mb : meshBuilds) appendBuiltMeshSceneData(mb, meshRecs, sceneData);
  // --- the TLAS over the compacted boxes, hidden instances masked; the depth rule with the BLASes that stay
  std::vector<float> boxes(6u * (size_t)newInstances);
  std::vector<uint8_t> hiddenAfter(newInstances, 0);
  for (uint32_t slot = 0; slot < oldInstances; slot++)
    if (newSlot[slot] != NONE) { memcpy(&boxes[6u * (size_t)newSlot[slot]], &T.instBoxes[6u * (size_t)slot], 24); hiddenAfter[newSlot[slot]] = H.meshBuilds[slotMesh[slot]].hidden ? 1 : 0; }
  Bvh8 tlas; std::vector<uint32_t> tlasItems; TlasMade tlasMade;
  const double tt0 = nowMs();
  {
    std::vector<float> masked(boxes);
    tlasMaskHiddenBoxes(masked.data(), hiddenAfter.data(), newInstances);
    tlasMade = buildEditTlas(s, blasDepth, masked.data(), newInstances, tlas, tlasItems);
  }
  const double tlasMs = nowMs() - tt0;
  if (2u * tlas.maxDepth + blasDepth + 1u > 16u) return decline("the TLAS over the compacted boxes is too deep for the 16-entry stack");
  // --- every device of the scene: ALL new blocks first, sized as a growth to the kept count would size them
  struct Fresh { DeviceBuffer<FVertex> verts; DeviceBuffer<TriShade> shade; DeviceBuffer<Node8> blasNodes; DeviceBuffer<BlasTri> blasTris; DeviceBuffer<InstanceRec> instances;
      DeviceBuffer<InstTrav> instTrav; DeviceBuffer<TriRec> tris; DeviceBuffer<int32_t> faceIds; DeviceBuffer<uint32_t> flat; DeviceBuffer<CompactRange> ranges;
      void release() { verts.release(); shade.release(); blasNodes.release(); blasTris.release(); instances.release(); instTrav.release(); tris.release(); faceIds.release();
          flat.release(); ranges.release(); }
      size_t bytes() const { return verts.bytes() + shade.bytes() + blasNodes.bytes() + blasTris.bytes() + instances.bytes() + instTrav.bytes() + tris.bytes() + faceIds.bytes() + flat.bytes(); } };
  std::vector<CompactRange> allRanges; size_t rangeFirst[8];
  for (int k = 0; k < 8; k++) { rangeFirst[k] = allRanges.size(); allRanges.insert(allRanges.end(), tables[k]->ranges.begin(), tables[k]->ranges.end()); }
  const uint32_t nDev = residentDeviceCount(s);
  std::vector<Fresh> fresh(nDev);
  auto slack = [](size_t n) { return n + n / 4u + 1u; }; // (DeviceBuffer::grow's)
  bool outOfMemory = false;
  const double t1 = nowMs();
  int rcDev = onSceneDevices(s, nDev, [&](SceneDevice& D, hipStream_t) -> int {
    if (D.dTris.count < oldTris || D.dTriFaceId.count < oldTris || D.dFlatOfOrig.count < oldTris || D.dInstances.count < oldInstances || D.dInstTrav.count < oldInstances ||
        D.dTriShade.count < oldShade || D.dVerts.count < oldVerts || D.dBlasNodes.count < oldBlasNodes || D.dBlasTris.count < oldBlasTris) {
      setError("internal: the device holds less than the scene"); return GI_C_ERROR; }
    Fresh& F = fresh[D.slot]; // (SceneDevice::slot is its index among the scene's devices)
    int r = F.ranges.alloc(allRanges.size());
    if (r == GI_C_OK) r = F.verts.alloc(slack(tVerts.Z.dstCount));
    if (r == GI_C_OK) r = F.shade.alloc(slack(tShade.Z.dstCount));
    if (r == GI_C_OK) r = F.blasNodes.alloc(slack(tNodes.Z.dstCount));
    if (r == GI_C_OK) r = F.blasTris.alloc(slack(tBlasTris.Z.dstCount));
    if (r == GI_C_OK) r = F.instances.alloc(slack(newInstances));
    if (r == GI_C_OK) r = F.instTrav.alloc(slack(newInstances));
    if (r == GI_C_OK) r = F.tris.alloc(slack(newTris));
    if (r == GI_C_OK) r = F.faceIds.alloc(slack(newTris));
    if (r == GI_C_OK) r = F.flat.alloc(slack(newTris));
    if (r == GI_C_OUT_OF_MEMORY_INTERNAL) { outOfMemory = true; return DEVICE_BUILD_FALLBACK; }
    return r;
  });
  if (rcDev != GI_C_OK) { // (nothing resident was touched on any device)
    (void)onSceneDevices(s, nDev, [&](SceneDevice& D, hipStream_t) -> int { fresh[D.slot].release(); return GI_C_OK; });
    if (rcDev == DEVICE_BUILD_FALLBACK && outOfMemory) return decline("out of device memory");
    return GI_C_ERROR;
  }
  // --- decided.  One launch per array kind behind the tables' copy, the small arrays the host made, one wait, the swap
  double deviceMs = 0.0; uint64_t releasedBytes = 0, oldBytes = 0, newBytes = 0; // (of the primary device: both sets of blocks are resident until the swap)
  rcDev = onSceneDevices(s, nDev, [&](SceneDevice& D, hipStream_t st) -> int {
    Fresh& F = fresh[D.slot];
    int r = GI_C_OK;
    if (hipMemcpyAsync(F.ranges.ptr, allRanges.data(), allRanges.size() * sizeof(CompactRange), hipMemcpyHostToDevice, st) != hipSuccess ||
        hipMemsetAsync(F.flat.ptr, 0, F.flat.count * sizeof(uint32_t), st) != hipSuccess) { setError("compaction (two-level): copy failed"); r = GI_C_ERROR; }
    double tk = 0.0;
    if (r == GI_C_OK && timing && D.slot == 0u) { if (hipStreamSynchronize(st) != hipSuccess) r = GI_C_ERROR; tk = nowMs(); }
    const void* const src[8] = {D.dVerts.ptr, D.dTriShade.ptr, D.dBlasNodes.ptr, D.dBlasTris.ptr, D.dInstances.ptr, D.dInstTrav.ptr, D.dTris.ptr, D.dTriFaceId.ptr};
    void* const dst[8] = {F.verts.ptr, F.shade.ptr, F.blasNodes.ptr, F.blasTris.ptr, F.instances.ptr, F.instTrav.ptr, F.tris.ptr, F.faceIds.ptr};
    for (int k = 0; k < 8 && r == GI_C_OK; k++)
      if (!launchCompactRanges(st, tables[k]->ranges.data(), F.ranges.ptr + rangeFirst[k], tables[k]->Z, src[k], dst[k], tables[k]->Z.kind == COMPACT_TRIS ? F.flat.ptr : nullptr)) {
        setError("internal: a compaction range outside its array"); r = GI_C_ERROR; } // (cannot happen: the tables passed their check)
    if (r == GI_C_OK && hipGetLastError() != hipSuccess) { setError("compaction (two-level): launch failed"); r = GI_C_ERROR; }
    if (r == GI_C_OK && (D.dTlasNodes.upload(tlas.nodes, st) || D.dTlasItems.upload(tlasItems, st) || D.dMeshes.upload(meshRecs, st) || D.dSceneData.upload(sceneData, st))) r = GI_C_ERROR;
    if (hipStreamSynchronize(st) != hipSuccess && r == GI_C_OK) { setError("compaction (two-level): device error"); r = GI_C_ERROR; }
    if (timing && D.slot == 0u && r == GI_C_OK) deviceMs = nowMs() - tk;
    if (r == GI_C_OK) { // the swap: the scene owns the new blocks, `F` the old ones
      const size_t before = D.dVerts.bytes() + D.dTriShade.bytes() + D.dBlasNodes.bytes() + D.dBlasTris.bytes() + D.dInstances.bytes() + D.dInstTrav.bytes() + D.dTris.bytes() +
          D.dTriFaceId.bytes() + D.dFlatOfOrig.bytes(), after = F.bytes();
      if (D.slot == 0u) { oldBytes = before; newBytes = after; if (before > after) releasedBytes = before - after; }
      std::swap(D.dVerts, F.verts); std::swap(D.dTriShade, F.shade); std::swap(D.dBlasNodes, F.blasNodes); std::swap(D.dBlasTris, F.blasTris); std::swap(D.dInstances, F.instances);
      std::swap(D.dInstTrav, F.instTrav); std::swap(D.dTris, F.tris); std::swap(D.dTriFaceId, F.faceIds); std::swap(D.dFlatOfOrig, F.flat);
    }
    F.release(); // (the old blocks, or after an error the new ones; before the render's memory plan reads free memory)
    return r;
  });
  if (rcDev != GI_C_OK) { // (a device is half done: the error path of the sync rebuilds the scene)
    (void)onSceneDevices(s, nDev, [&](SceneDevice& D, hipStream_t) -> int { fresh[D.slot].release(); return GI_C_OK; });
    return GI_C_ERROR;
  }
  const double t2 = nowMs();
  // --- the host copies behind the committed compaction, where they lie (gi_compact.h compactRangesInPlaceHost: the kernel's per-piece form, ranges that stay
  // where they are untouched); the arrays keep their capacity
  const bool hostRecords = !H.hostTreeDropped && H.bvh.tris.size() == oldTris && H.triFaceId.size() == oldTris && H.flatOfOrig.size() == oldTris;
  {
    struct HostMove { const CompactTable* t; void* data; uint32_t* table; };
    std::vector<HostMove> moves = {{&tVerts, H.verts.data(), nullptr}, {&tShade, H.triShade.data(), nullptr}, {&tNodes, T.blasNodes.data(), nullptr},
        {&tBlasTris, T.blasTris.data(), nullptr}, {&tInst, H.instances.data(), nullptr}, {&tTrav, T.instTrav.data(), nullptr}};
    if (hostRecords) { moves.push_back({&tTris, H.bvh.tris.data(), H.flatOfOrig.data()}); moves.push_back({&tWords, H.triFaceId.data(), nullptr}); }
    parallelOver(moves.size(), [&](size_t k) { compactRangesInPlaceHost(moves[k].t->ranges.data(), moves[k].t->Z, moves[k].data, moves[k].table); }); // (one thread per array)
    H.verts.resize(tVerts.Z.dstCount); H.triShade.resize(tShade.Z.dstCount); T.blasNodes.resize(tNodes.Z.dstCount); T.blasTris.resize(tBlasTris.Z.dstCount);
    H.instances.resize(newInstances); T.instTrav.resize(newInstances);
  }
  if (hostRecords) { H.bvh.tris.resize(newTris); H.triFaceId.resize(newTris); H.flatOfOrig.resize(newTris); }
  else { // dropped by an edit in place before: they stay dropped, and the id table goes with them
    std::vector<uint32_t>().swap(H.flatOfOrig);
    if (!H.hostTreeDropped) { std::vector<TriRec>().swap(H.bvh.tris); std::vector<int32_t>().swap(H.triFaceId); H.hostTreeDropped = true; } // (cannot happen)
  }
  H.meshBuilds.swap(meshBuilds); H.meshRecs.swap(meshRecs); H.sceneData.swap(sceneData);
  T.meshBlasTri.swap(meshBlasTri); T.meshBlasNode.swap(meshBlasNode); T.meshBlasLevels.swap(meshBlasLevels); T.meshBlasBudget.swap(meshBlasBudget);
  T.instBoxes.swap(boxes); T.tlasNodes.swap(tlas.nodes); T.tlasItems.swap(tlasItems); T.tlasDepth = tlas.maxDepth; T.blasDepth = blasDepth; noteTlasMade(T, tlasMade);
  { // the destroyed meshes nothing refers to any more
    std::vector<GiCMesh*> still;
    for (GiCMesh* m : s->retiredMeshes) {
      bool named = false;
      for (const MeshBuild& mb : H.meshBuilds) if (mb.m == m) { named = true; break; }
      if (named) still.push_back(m); else delete m;
    }
    s->retiredMeshes.swap(still);
  }
  s->triCount = newTris; H.bvh.activeTris = newTris;
  if (!(s->dirty & DIRTY_MATERIALS)) deriveSceneClasses(s, H, false); // (with a material edit due updateMaterials derives the classes behind the edit)
  setSceneBoundsFromInstances(s, H);
  const double t3 = nowMs();
  cost.buildMs += tlasMs; cost.uploadMs += std::max(t3 - t0 - tlasMs, 0.0);
  s->compactionStats[0]++; s->compactionStats[1] += movedRecords; s->compactionStats[2] += releasedBytes;
  if (timing) fprintf(stderr, "[gatling_gi] compaction (two-level): %zu range(s) of 8 array kinds, %llu record(s) moved (%u of %u flat record(s), %u of %u instance(s), %u of %u "
                              "mesh(es) stay), %llu byte(s) freed on the primary device (%llu old + %llu new resident during the swap), host %.2f ms (of which TLAS build %.2f), device %.2f ms "
                              "(launches + wait %.3f)\n",
                      rangeCount, (unsigned long long)movedRecords, newTris, oldTris, newInstances, oldInstances, keptMeshes, oldMeshes, (unsigned long long)releasedBytes,
                      (unsigned long long)oldBytes, (unsigned long long)newBytes, (t1 - t0) + (t3 - t2), tlasMs, t2 - t1, deviceMs);
  compacted = true;
  return GI_C_OK;
}

// The trigger, where an edit in place has planned its after-edit counts and is about to test "retired triangles outnumber live ones": with the option wanted
// and retired x 100 > live x tlas_compact_percent the resident scene is compacted.  True: it was -- every index the caller has planned with is stale, and it
// starts over on the compacted scene (where it does not ask again).  rc: GI_C_ERROR on a device error
static bool compactBeforeEdit(GiCScene* s, SceneHost& H, uint64_t retired, uint64_t live, UpdateCost& cost, int& rc)
{
  rc = GI_C_OK;
  if (!tlasCompactionWanted(s)) return false;
  const uint64_t percent = (uint64_t)std::max(optionValue("tlas_compact_percent", 100), 0L);
  if (!(retired * 100u > live * percent)) return false;
  bool compacted = false;
  rc = compactTwoLevel(s, H, compacted, cost);
  return rc == GI_C_OK && compacted;
}

static int updateInstancesTwoLevel(GiCScene* s, SceneHost& H, bool& applied, UpdateCost& cost, bool mayCompact = true)
{
  TwoLevelHost& T = H.two;
  const char* const what = "instance update (two-level)";
  const bool timing = getenv("GATLING_BUILD_TIMING") != nullptr;
  auto decline = [&](const char* why) { if (timing) fprintf(stderr, "[gatling_gi] %s: %s; the scene is rebuilt\n", what, why); return GI_C_OK; };
  const uint32_t oldInstances = (uint32_t)H.instances.size(), oldTris = s->triCount, shadeCount = (uint32_t)H.triShade.size(), meshCount = (uint32_t)H.meshBuilds.size();
  if (s->stats.inactiveTriangleCount != 0u) return decline("the scene was built with inactive triangles");
  if (H.deviceBuilt || H.partitioned || !H.treeless || !H.shadePacked || H.reordered) return decline("the scene is not a two-level scene without the flat tree");
  if (T.instTrav.size() != oldInstances || T.instBoxes.size() != 6u * (size_t)oldInstances || T.meshBlasTri.size() != meshCount || H.meshRecs.size() != meshCount)
    return decline("the host copy is not the built scene's"); // (cannot happen)
  for (const MeshBuild& mb : H.meshBuilds)
    if (mb.m->builtInstances != mb.instCount || mb.inst.size() != mb.instCount || mb.instTri.size() != mb.instCount || mb.meshIdx != (uint32_t)(&mb - H.meshBuilds.data()))
      return decline("a built mesh with another instance count"); // (cannot happen)
  const double t0 = nowMs();
  // --- the edits: which meshes, what they add and retire; ids and moves of the kept instances (planned: nothing is written yet)
  struct InstEdit { uint32_t b, oldCount, newCount, reuse; };
  struct IdEdit { uint32_t rec; int32_t id; };
  struct Move { uint32_t b, ii; };
  std::vector<InstEdit> edits; std::vector<IdEdit> idEdits; std::vector<Move> moves;
  std::vector<uint32_t> newCountOf(meshCount);
  uint64_t grownInst = 0, shrunkInst = 0, reusedInst = 0, grownTris = 0, shrunkTris = 0, reusedTris = 0; bool sceneDataStale = false;
  for (uint32_t b = 0; b < meshCount; b++) {
    const MeshBuild& mb = H.meshBuilds[b];
    newCountOf[b] = mb.instCount;
    if (!mb.m->instEdited || mb.m->retired) continue;
    const size_t newCount = mb.m->instanceTransforms.size() / 16;
    const uint64_t nf = mb.m->faces.size();
    if (newCount == 0u) return decline("a new count of 0");
    if (newCount >= 0xffffffffu || nf == 0u || nf >= ((uint64_t)1 << 26)) return decline("an instance count or face count beyond the layout's"); // (cannot happen)
    if (mb.hidden) return decline("an instancer edit of a mesh hidden by the visibility path");
    if (mb.instCount == 0u) return decline("a built mesh without an instance has no BLAS");
    InstEdit e{b, mb.instCount, (uint32_t)newCount, 0u};
    if (e.newCount > e.oldCount) {
      e.reuse = (uint32_t)std::min<size_t>(e.newCount - e.oldCount, mb.freeSlots.size());
      grownInst += e.newCount - e.oldCount; grownTris += (e.newCount - e.oldCount) * nf; reusedInst += e.reuse; reusedTris += e.reuse * nf;
    } else { shrunkInst += e.oldCount - e.newCount; shrunkTris += (e.oldCount - e.newCount) * nf; }
    newCountOf[b] = e.newCount;
    edits.push_back(e);
    if (mb.m->material) for (uint32_t slot = 0; slot < TEX_SLOT_COUNT; slot++) if (!mb.m->material->primvarInput[slot].empty()) sceneDataStale = true;
    const uint32_t kept = std::min(e.oldCount, e.newCount);
    for (uint32_t ii = 0; ii < kept; ii++) {
      if (mb.inst[ii] >= oldInstances) return decline("the host copy is not the built scene's"); // (cannot happen)
      const InstanceRec& resident = H.instances[mb.inst[ii]];
      const InstanceRec want = makeInstanceRec(mb.m, mb.meshIdx, ii);
      if (want.instanceId != resident.instanceId) idEdits.push_back(IdEdit{mb.inst[ii], want.instanceId});
      if (memcmp(want.o2w, resident.o2w, sizeof(want.o2w)) != 0) moves.push_back(Move{b, ii});
    }
  }
  if (edits.empty()) { applied = true; return GI_C_OK; } // (the edited meshes are retired: updateTopologyTwoLevel takes them out)
  if (!moves.empty() && !tlasUpdatesWanted(s)) return decline("a kept instance moved and transform updates of the two-level layout are not wanted");
  const bool countsChange = grownInst != 0u || shrunkInst != 0u;
  const uint64_t appendedInst = grownInst - reusedInst, appendedTris = grownTris - reusedTris;
  // --- what the scene holds after the edit
  {
    uint64_t live = 0, retired = 0, visible = 0;
    for (const MeshBuild& mb : H.meshBuilds) {
      const uint64_t n = (uint64_t)mb.instCount * mb.m->faces.size(), gone = (uint64_t)mb.retiredInst * mb.m->faces.size();
      if (mb.m->retired) retired += n + gone; else { live += n; retired += gone; if (!mb.hidden) visible += n; }
    }
    live += grownTris; live -= shrunkTris; visible += grownTris; visible -= shrunkTris; retired += shrunkTris; retired -= reusedTris;
    if (visible < kIncrementalMinTris) return decline("fewer than 4096 visible triangles after the edit");
    if (mayCompact) { // (GI_C_SCENE_OPTION_TLAS_COMPACTION: the plan above names slots and meshes of the scene as it was -- it is made again)
      int rc = GI_C_OK;
      if (compactBeforeEdit(s, H, retired, live, cost, rc)) return updateInstancesTwoLevel(s, H, applied, cost, false);
      if (rc != GI_C_OK) return GI_C_ERROR;
    }
    if (retired > live) return decline("retired triangles outnumber live ones");
  }
  if ((uint64_t)oldTris + appendedTris >= ((uint64_t)1 << 28)) return decline("2^28 or more flat records after the append");
  if ((uint64_t)oldInstances + appendedInst >= 0xffffffffull) return decline("the arrays outgrow 32-bit indices");
  const uint32_t newInstances = oldInstances + (uint32_t)appendedInst, newTris = oldTris + (uint32_t)appendedTris;
  // --- the ids after the edit, in the order a fresh build meets the meshes (a hidden mesh keeps the ids it has; a mesh destroyed in this very sync is still
  // part of the scene here: updateTopologyTwoLevel retires it behind this update) ...
  std::vector<uint32_t> newBase(meshCount, 0u);
  uint64_t visibleTris = 0;
  for (const MeshBuild& mb : H.meshBuilds) {
    newBase[mb.meshIdx] = mb.hidden ? mb.idBase : (uint32_t)visibleTris;
    if (!mb.hidden) visibleTris += (uint64_t)newCountOf[mb.meshIdx] * mb.m->faces.size();
  }
  if (visibleTris > newTris) return decline("the host copy is not the built scene's"); // (cannot happen: the id table has one word per resident record)
  // ... and the table of the device pass over what is resident: kept instances move with their mesh, retiring ones are hidden for good
  std::vector<VisPatch> patch(oldInstances, VisPatch{0, VIS_KEEP});
  std::vector<uint8_t> hiddenAfter(newInstances, 0);
  bool launchPatch = false, renumbered = false;
  for (const MeshBuild& mb : H.meshBuilds) {
    const int32_t delta = (int32_t)(newBase[mb.meshIdx] - mb.idBase);
    const uint32_t kept = std::min(mb.instCount, newCountOf[mb.meshIdx]);
    if (mb.hidden) for (const uint32_t inst : mb.inst) hiddenAfter[inst] = 1;
    if (delta != 0) { launchPatch = renumbered = true; for (uint32_t ii = 0; ii < kept; ii++) patch[mb.inst[ii]].idDelta = delta; }
    for (uint32_t ii = kept; ii < mb.instCount; ii++) { patch[mb.inst[ii]] = VisPatch{0, VIS_HIDE}; hiddenAfter[mb.inst[ii]] = 1; launchPatch = true; }
  }
  // --- the new instances: their slots, records and jobs
  struct NewInst { uint32_t b, ii, slot, tri; InstanceRec rec; };
  std::vector<NewInst> fresh; fresh.reserve(grownInst);
  std::vector<InstanceJob> jobs; jobs.reserve(grownInst);
  std::vector<InstBoundsJob> boundsJobs; boundsJobs.reserve(grownInst);
  std::vector<int32_t> faceIdAll;
  uint32_t chunksPerJob = 0;
  {
    uint32_t nextInst = oldInstances, nextTri = oldTris;
    for (const InstEdit& e : edits) {
      if (e.newCount <= e.oldCount) continue;
      const MeshBuild& mb = H.meshBuilds[e.b];
      const uint32_t nf = (uint32_t)mb.m->faces.size(), blasFirst = T.meshBlasTri[mb.meshIdx];
      if (mb.faceIdAov.size() != nf || (size_t)blasFirst + nf > T.blasTris.size()) return decline("the host copy is not the built scene's"); // (cannot happen)
      const uint32_t faceIdFirst = (uint32_t)faceIdAll.size();
      faceIdAll.insert(faceIdAll.end(), mb.faceIdAov.begin(), mb.faceIdAov.end());
      for (uint32_t ii = e.oldCount; ii < e.newCount; ii++) {
        NewInst ni{}; ni.b = e.b; ni.ii = ii;
        const uint32_t k = ii - e.oldCount;
        if (k < e.reuse) { ni.slot = mb.freeSlots[k].inst; ni.tri = mb.freeSlots[k].tri; }
        else { ni.slot = nextInst++; ni.tri = nextTri; nextTri += nf; }
        ni.rec = makeInstanceRec(mb.m, mb.meshIdx, ii);
        if (!usableInstance(ni.rec)) return decline("a new instance has a transform that is not usable");
        if (ni.slot >= newInstances || (uint64_t)ni.tri + nf > newTris) return decline("the host copy is not the built scene's"); // (cannot happen)
        InstanceJob j{}; j.instance = ni.slot; j.triFirst = ni.tri; j.idBase = newBase[mb.meshIdx] + ii * nf; j.shadeBase = mb.shadeBase; j.faceCount = nf; j.matFlags = mb.matFlags;
        j.faceIdFirst = faceIdFirst;
        InstBoundsJob bj{}; memcpy(bj.o2w, ni.rec.o2w, sizeof(bj.o2w)); bj.firstTri = blasFirst; bj.faceCount = nf; bj.instance = ni.slot;
        fresh.push_back(ni); jobs.push_back(j); boundsJobs.push_back(bj);
        hiddenAfter[ni.slot] = 0;
      }
      chunksPerJob = std::max(chunksPerJob, instBoundsChunks(nf));
    }
  }
  // (the free slots that stay free; those of this sync's retiring instances were marked above)
  for (uint32_t b = 0; b < meshCount; b++) {
    const MeshBuild& mb = H.meshBuilds[b];
    uint32_t taken = 0;
    for (const InstEdit& e : edits) if (e.b == b) taken = e.reuse;
    for (size_t k = taken; k < mb.freeSlots.size(); k++) hiddenAfter[mb.freeSlots[k].inst] = 1;
  }
  InstanceJobSizes Z{}; Z.jobCount = (uint32_t)jobs.size(); Z.triCount = newTris; Z.instanceCount = newInstances; Z.shadeCount = shadeCount; Z.flatCount = newTris;
  Z.faceIdCount = (uint32_t)faceIdAll.size(); Z.wgCount = instanceJobsNumber(jobs.data(), Z.jobCount);
  if (!jobs.empty() && (Z.wgCount == 0u || !instanceJobsOk(jobs.data(), Z))) return decline("a new instance's records outside their arrays"); // (cannot happen)
  if ((uint64_t)boundsJobs.size() * chunksPerJob >= (1ull << 31)) return decline("more bounds workgroups than a launch takes");
  // --- primary device, scratch only: padded world boxes and statuses of the new instances over the resident BLAS triangles
  std::vector<uint32_t> result;
  bool outOfMemory = false;
  const double tA = nowMs();
  if (!boundsJobs.empty()) {
    const int rcB = instanceBoundsOnPrimary(s, boundsJobs, chunksPerJob, nullptr, result, outOfMemory, what);
    if (rcB == DEVICE_BUILD_FALLBACK && outOfMemory) return decline("out of device memory");
    if (rcB != GI_C_OK) return GI_C_ERROR;
  }
  const double boundsMs = nowMs() - tA;
  for (size_t k = 0; k < boundsJobs.size(); k++)
    if (result[7u * k + 6u] != 0u) return decline("a new instance carries triangles that leave the usable coordinate range in world space");
  // --- the TLAS over all boxes, hidden instances and free slots masked; the depth rule (the BLASes do not change)
  std::vector<float> boxes; Bvh8 tlas; std::vector<uint32_t> tlasItems; double tlasMs = 0.0; TlasMade tlasMade;
  if (countsChange) {
    boxes = T.instBoxes; boxes.resize(6u * (size_t)newInstances, 0.0f);
    for (size_t k = 0; k < boundsJobs.size(); k++) memcpy(&boxes[6u * (size_t)boundsJobs[k].instance], &result[7u * k], 24);
    std::vector<float> masked(boxes);
    tlasMaskHiddenBoxes(masked.data(), hiddenAfter.data(), newInstances);
    const double tt0 = nowMs();
    tlasMade = buildEditTlas(s, T.blasDepth, masked.data(), newInstances, tlas, tlasItems);
    tlasMs = nowMs() - tt0;
    if (2u * tlas.maxDepth + T.blasDepth + 1u > 16u) return decline("the new TLAS is too deep for the 16-entry stack");
  }
  // --- the records after the edit, staged: ids, the renumbered id bases, the new instances
  std::vector<InstanceRec> instances(H.instances); instances.resize(newInstances, InstanceRec{});
  std::vector<InstTrav> instTrav(T.instTrav); instTrav.resize(newInstances, InstTrav{});
  for (const IdEdit& e : idEdits) instances[e.rec].instanceId = e.id;
  if (renumbered) patchInstTravHost(instTrav.data(), oldInstances, patch.data());
  for (const NewInst& ni : fresh) {
    const MeshBuild& mb = H.meshBuilds[ni.b];
    const InstTrav& sibling = T.instTrav[mb.inst[0]]; // (the mesh's constants: its resident BLAS, the slack of its current points, the last material update's word)
    instances[ni.slot] = ni.rec;
    instTrav[ni.slot] = tlasMakeInstTrav(ni.rec, sibling.blasRoot, newBase[mb.meshIdx] + ni.ii * (uint32_t)mb.m->faces.size(), sibling.matFlags, sibling.slack);
  }
  for (uint32_t i = 0; i < oldInstances; i++) if (hiddenAfter[i]) patch[i].action |= VIS_HIDDEN_AFTER;
  // the tables of a mesh whose material reads primvars are sized from its instance count and ids (with a material edit due updateMaterials makes them anew)
  std::vector<MeshRec> meshRecs; std::vector<float> sceneData;
  if (sceneDataStale && !(s->dirty & DIRTY_MATERIALS)) for (const MeshBuild& mb : H.meshBuilds) appendBuiltMeshSceneData(mb, meshRecs, sceneData);
  else sceneDataStale = false;
  const double t1 = nowMs();
  // --- every device of the scene, on its own stream: the arrays grown and the temporaries allocated before anything resident changes
  double recordsKernelMs = 0.0;
  const size_t bytesSent = (launchPatch ? patch.size() * sizeof(VisPatch) : 0u) + idEdits.size() * sizeof(InstanceRec) +
      fresh.size() * (sizeof(InstanceRec) + sizeof(InstTrav) + sizeof(InstanceJob)) + faceIdAll.size() * 4u + tlas.nodes.size() * sizeof(Node8) + tlasItems.size() * 4u +
      meshRecs.size() * sizeof(MeshRec) + sceneData.size() * sizeof(float);
  const bool anythingToSend = countsChange || !idEdits.empty() || sceneDataStale;
  const int rcDev = onSceneDevices(s, anythingToSend ? residentDeviceCount(s) : 0u, [&](SceneDevice& D, hipStream_t st) -> int {
    if (D.dTris.count < oldTris || D.dTriFaceId.count < oldTris || D.dFlatOfOrig.count < oldTris || D.dInstances.count < oldInstances || D.dInstTrav.count < oldInstances ||
        D.dTriShade.count < shadeCount) { setError("internal: the device holds less than the scene"); return GI_C_ERROR; }
    std::vector<void*> old;
    DeviceBuffer<VisPatch> dPatch; DeviceBuffer<InstanceJob> dJobs; DeviceBuffer<int32_t> dFaceIds;
    auto releaseAll = [&] { dPatch.release(); dJobs.release(); dFaceIds.release(); for (void* p : old) (void)hipFree(p); old.clear(); };
    int r = launchPatch ? dPatch.alloc(patch.size()) : GI_C_OK;
    if (r == GI_C_OK && !jobs.empty()) { r = dJobs.alloc(jobs.size()); if (r == GI_C_OK) r = dFaceIds.alloc(faceIdAll.size()); }
    if (r == GI_C_OK) r = D.dInstances.grow(newInstances, st, old);
    if (r == GI_C_OK) r = D.dInstTrav.grow(newInstances, st, old);
    if (r == GI_C_OK) r = D.dTris.grow(newTris, st, old);
    if (r == GI_C_OK) r = D.dTriFaceId.grow(newTris, st, old);
    if (r == GI_C_OK) r = D.dFlatOfOrig.grow(newTris, st, old);
    if (r != GI_C_OK) { // (the copies out of the old blocks must finish before they are freed)
      (void)hipStreamSynchronize(st); releaseAll();
      if (r == GI_C_OUT_OF_MEMORY_INTERNAL) { outOfMemory = true; return DEVICE_BUILD_FALLBACK; }
      return GI_C_ERROR;
    }
    auto copy = [&](void* dst, const void* src, size_t bytes) {
      if (r == GI_C_OK && bytes && hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, st) != hipSuccess) { setError("instance update (two-level): copy failed"); r = GI_C_ERROR; } };
    // the retire and the renumbering: ids, edges, the id table and the instances' id bases, over what was resident before
    if (launchPatch) {
      copy(dPatch.ptr, patch.data(), patch.size() * sizeof(VisPatch));
      if (r == GI_C_OK) {
        launchPatchVisibility2(st, D.dTris.ptr, oldTris, D.dInstances.ptr, oldInstances, dPatch.ptr, D.dTriShade.ptr, shadeCount, D.dFlatOfOrig.ptr, newTris);
        if (renumbered) launchPatchInstTrav(st, D.dInstTrav.ptr, oldInstances, dPatch.ptr);
      }
    }
    // what the host made per instance and per face ...
    for (const IdEdit& e : idEdits) copy(D.dInstances.ptr + e.rec, &instances[e.rec], sizeof(InstanceRec));
    for (const NewInst& ni : fresh) { copy(D.dInstances.ptr + ni.slot, &instances[ni.slot], sizeof(InstanceRec)); copy(D.dInstTrav.ptr + ni.slot, &instTrav[ni.slot], sizeof(InstTrav)); }
    copy(dJobs.ptr, jobs.data(), jobs.size() * sizeof(InstanceJob)); copy(dFaceIds.ptr, faceIdAll.data(), faceIdAll.size() * 4u);
    if (r == GI_C_OK && countsChange && (D.dTlasNodes.upload(tlas.nodes, st) || D.dTlasItems.upload(tlasItems, st))) r = GI_C_ERROR;
    if (r == GI_C_OK && sceneDataStale && (D.dMeshes.upload(meshRecs, st) || D.dSceneData.upload(sceneData, st))) r = GI_C_ERROR;
    // ... and everything per flattened triangle of all new instances, made where it lives in one launch (gi_instances.hip), behind those copies on the stream
    double tk = 0.0;
    if (r == GI_C_OK && timing && D.slot == 0u) { if (hipStreamSynchronize(st) != hipSuccess) r = GI_C_ERROR; tk = nowMs(); }
    if (r == GI_C_OK && !jobs.empty() &&
        !launchInstanceRecords(st, jobs.data(), dJobs.ptr, Z, D.dTris.ptr, D.dTriFaceId.ptr, D.dFlatOfOrig.ptr, D.dInstances.ptr, D.dTriShade.ptr, dFaceIds.ptr)) {
      setError("internal: a new instance's records outside their arrays"); r = GI_C_ERROR; } // (cannot happen: asked above)
    if (r == GI_C_OK && hipGetLastError() != hipSuccess) { setError("instance update (two-level): launch failed"); r = GI_C_ERROR; }
    if (hipStreamSynchronize(st) != hipSuccess && r == GI_C_OK) { setError("instance update (two-level): device error"); r = GI_C_ERROR; }
    if (timing && D.slot == 0u && r == GI_C_OK) recordsKernelMs = nowMs() - tk;
    releaseAll(); // (before the render's memory plan reads free memory)
    return r;
  });
  if (rcDev == DEVICE_BUILD_FALLBACK && outOfMemory) return decline("out of device memory");
  if (rcDev != GI_C_OK) return GI_C_ERROR;
  const double t2 = nowMs();
  // --- the host copies behind the committed edit: the flat records, face ids and id table where they are still held, by the kernels' own host forms
  const bool hostRecords = !H.hostTreeDropped && H.bvh.tris.size() == oldTris && H.triFaceId.size() == oldTris && H.flatOfOrig.size() == oldTris;
  if (countsChange) {
    if (hostRecords) {
      auto grown = [](auto& v, size_t n) { if (v.capacity() < n) v.reserve(n + n / 4u); v.resize(n); }; // (25 % slack, as updateTopologyTwoLevel)
      grown(H.bvh.tris, newTris); grown(H.triFaceId, newTris); grown(H.flatOfOrig, newTris);
      if (launchPatch) {
        constexpr size_t CHUNK = 65536;
        parallelOver(((size_t)oldTris + CHUNK - 1) / CHUNK, [&](size_t c) { // (one writer per word: the visible ids are a permutation)
          for (size_t i = c * CHUNK; i < std::min((size_t)oldTris, (c + 1) * CHUNK); i++)
            vis2_patch_record(H.bvh.tris.data(), (uint32_t)i, H.instances.data(), oldInstances, patch.data(), H.triShade.data(), shadeCount, H.flatOfOrig.data(), newTris);
        });
      }
      constexpr uint32_t WGS = 1024;
      parallelOver(((size_t)Z.wgCount + WGS - 1) / WGS, [&](size_t c) {
        instanceRecordsHost(jobs.data(), Z, (uint32_t)c * WGS, std::min(Z.wgCount, ((uint32_t)c + 1u) * WGS), H.bvh.tris.data(), H.triFaceId.data(), H.flatOfOrig.data(),
            instances.data(), H.triShade.data(), faceIdAll.data());
      });
    } else { // dropped by an edit in place before: they stay dropped, and the id table -- one word per resident record -- goes with them
      std::vector<uint32_t>().swap(H.flatOfOrig);
      if (!H.hostTreeDropped) { std::vector<TriRec>().swap(H.bvh.tris); std::vector<int32_t>().swap(H.triFaceId); H.hostTreeDropped = true; } // (cannot happen)
    }
  }
  H.instances.swap(instances); T.instTrav.swap(instTrav);
  if (countsChange) { T.instBoxes.swap(boxes); T.tlasNodes.swap(tlas.nodes); T.tlasItems.swap(tlasItems); T.tlasDepth = tlas.maxDepth; noteTlasMade(T, tlasMade); }
  if (sceneDataStale) { H.meshRecs.swap(meshRecs); H.sceneData.swap(sceneData); }
  // --- the MeshBuilds and the meshes: counts, slots, id bases; the moves go to updateTransformsTwoLevel
  for (MeshBuild& mb : H.meshBuilds) mb.idBase = newBase[mb.meshIdx];
  size_t nextFresh = 0;
  for (const InstEdit& e : edits) {
    MeshBuild& mb = H.meshBuilds[e.b];
    GiCMesh* m = const_cast<GiCMesh*>(mb.m);
    if (e.newCount < e.oldCount) {
      for (uint32_t ii = e.newCount; ii < e.oldCount; ii++) mb.freeSlots.push_back(MeshBuild::FreeSlot{mb.inst[ii], mb.instTri[ii]});
      std::sort(mb.freeSlots.begin(), mb.freeSlots.end(), [](const MeshBuild::FreeSlot& a, const MeshBuild::FreeSlot& c) { return a.inst < c.inst; });
      mb.inst.resize(e.newCount); mb.instTri.resize(e.newCount);
    } else if (e.newCount > e.oldCount) {
      mb.freeSlots.erase(mb.freeSlots.begin(), mb.freeSlots.begin() + e.reuse);
      for (uint32_t ii = e.oldCount; ii < e.newCount; ii++, nextFresh++) { mb.inst.push_back(fresh[nextFresh].slot); mb.instTri.push_back(fresh[nextFresh].tri); }
    }
    mb.retiredInst = (uint32_t)mb.freeSlots.size();
    mb.instCount = e.newCount; m->builtInstances = e.newCount; m->instEdited = false;
    const bool all = m->xformDirty && m->instDirty.empty(); // (a giCSetMeshTransform is due as well: every instance is re-bounded anyway)
    if (!all) m->instDirty.resize(e.newCount, 0);
    for (const Move& mv : moves) if (mv.b == e.b) { m->xformDirty = true; if (!all) m->instDirty[mv.ii] = 1; }
    if (m->xformDirty) s->dirty |= DIRTY_XFORM; else m->instDirty.clear();
  }
  if (countsChange) { s->triCount = newTris; H.bvh.activeTris = newTris; setSceneBoundsFromInstances(s, H); }
  const double t3 = nowMs();
  cost.buildMs += tlasMs; cost.uploadMs += std::max(t3 - t0 - tlasMs, 0.0);
  s->tlasInstanceCounts[0]++; s->tlasInstanceCounts[1] += grownInst; s->tlasInstanceCounts[2] += reusedInst; s->tlasInstanceCounts[3] += shrunkInst;
  if (timing) fprintf(stderr, "[gatling_gi] instance update (two-level): %llu instance(s) retired, %llu appended (%llu into reused slots, %llu flat record(s) made on the "
                              "device by %u workgroup(s) of one launch), %zu instance record(s) re-sent for their ids, %zu moved, %u resident triangle(s), %u instance "
                              "slot(s), TLAS %zu node(s), host TLAS build %.2f ms, host rest %.2f ms, device %.2f ms (bounds kernels + read-back %.2f, commit %.2f of "
                              "which the records kernel %.3f), %zu bytes sent per device\n", (unsigned long long)shrunkInst, (unsigned long long)grownInst,
                      (unsigned long long)reusedInst, (unsigned long long)grownTris, Z.wgCount, idEdits.size(), moves.size(), s->triCount, newInstances, T.tlasNodes.size(),
                      tlasMs, std::max((t1 - t0) - tlasMs - boundsMs + (t3 - t2), 0.0), boundsMs + (t2 - t1), boundsMs, t2 - t1, recordsKernelMs, bytesSent);
  applied = true;
  return GI_C_OK;
}

// ---------------------------------------------------------------------------------------------------------------
// Topology updates on the two-level layout (opt-in: GI_C_SCENE_OPTION_TLAS_TOPOLOGY / GATLING_OPTIONS=tlas_topology=1, read with topology updates wanted, on a
// scene built without the flat tree: SceneHost::treeless).  Meshes were created or destroyed; nothing else asked for the rebuild.  With no flat tree to grow,
//   retire:  a destroyed mesh of the built scene (GiCMesh::retired) becomes hidden for good through updateVisibilityTwoLevel's machinery -- planVisibility
//            with the predicate hidden || retired, k_patch_visibility2 and k_patch_inst_trav over the resident records, its instances masked out of the TLAS.
//            Its BLAS nodes and triangles, flat records and shading records stay resident as retired ranges until the next buildScene, which frees the mesh.
//   append:  every mesh a fresh build would hold that has no MeshBuild, all of them behind every built one, goes to the ends of the arrays.  The host makes
//            and sends what the mesh has per vertex, per face and per instance: FVertex records (packVertex), the faces, the AOV face ids (faceIdAovOf), the
//            InstanceRecs (makeInstanceRec), the InstTrav records (tlasMakeInstTrav, triBase = the plan's id base), its ONE BLAS (buildMeshBlas, as
//            buildTwoLevel runs it, rebased onto the ends of the BLAS arrays) with the builder's face order, the MeshRec / scene-data tables.  The instances'
//            world boxes and statuses come from k_inst_bounds / k_inst_finish over the new BLAS triangles in scratch memory (instanceBoundsOnPrimary) before
//            anything resident changes; the TLAS is built again by buildBvh8Boxes over all boxes, hidden and retired instances masked.
//   device:  the arrays grow in place (DeviceBuffer::grow); gi_append.hip makes everything per face and per flattened triangle where it lives --
//            k_append_shade_index, k_gather_shade, k_append_blas_tris, k_append_records: shading records, BLAS triangles, the flat TriRecs, their face-id
//            words and their words of the id table.  Nothing per flattened triangle crosses the link.
//   host copies: the MeshBuilds, H.verts, H.triShade, H.instances, the tables, H.two with meshBlasTri / meshBlasNode / meshBlasLevels (a later BLAS refit
//            finds the mesh); the flat records, face ids and id table where the host still holds them (gi_append.h appendRecordsHost, the kernels' form) --
//            where an edit in place dropped them they stay dropped.
// Every decision comes before the first resident write.  Declines (handled = false, not an error, one line under GATLING_BUILD_TIMING): the option off, a
// scene with a flat tree, no host copy or incremental=0 (updateTopology); an instance-count or instance-id edit of a built mesh due; a scene built with
// inactive triangles; fewer than kIncrementalMinTris visible triangles after the edit; more retired than live triangles; a new mesh in front of a built one;
// an unusable vertex position; an unusable instance transform; a set status (triangles that leave the usable range in world space); a material index above
// 2^24; 2^26 unique BLAS triangles or 2^28 flat records; a TLAS too deep (2 x TLAS depth + BLAS depth + 1 > 16, the new BLAS included); out of device
// memory (a later device of several: the earlier ones are committed, and buildScene sends everything anew).
// ---------------------------------------------------------------------------------------------------------------
static int updateTopologyTwoLevel(GiCScene* s, SceneHost& H, bool& handled, UpdateCost& cost, bool afterCompaction)
{
  TwoLevelHost& T = H.two;
  const char* const what = "topology update (two-level)";
  const bool timing = getenv("GATLING_BUILD_TIMING") != nullptr;
  auto decline = [&](const char* why) { if (timing) fprintf(stderr, "[gatling_gi] %s: %s; the scene is rebuilt\n", what, why); return GI_C_OK; };
  // --- instancer edits of built meshes come first (GI_C_SCENE_OPTION_TLAS_INSTANCES: updateInstancesTwoLevel above): committed whole, or declined with nothing
  // resident touched.  The meshes created and destroyed in the same sync are then applied to the scene it leaves; a decline below rebuilds, as ever
  // (afterCompaction: the call started over behind a compaction of its own -- the instancer edits are applied, and it does not ask for another)
  if (s->instancesDue && !afterCompaction) {
    if (!tlasInstancesWanted(s)) return decline("an instance-count or instance-id edit of a built mesh is due");
    bool applied = false;
    if (updateInstancesTwoLevel(s, H, applied, cost) != GI_C_OK) return GI_C_ERROR;
    if (!applied) return GI_C_OK;
  }
  const UpdateCost instancerCost = cost;
  const uint32_t oldInstances = (uint32_t)H.instances.size(), oldTris = s->triCount, shade0 = (uint32_t)H.triShade.size(), vert0 = (uint32_t)H.verts.size();
  const uint32_t blasNode0 = (uint32_t)T.blasNodes.size(), blasTri0 = (uint32_t)T.blasTris.size(), mesh0 = (uint32_t)H.meshBuilds.size();
  if (s->stats.inactiveTriangleCount != 0u) return decline("the scene was built with inactive triangles");
  if (H.deviceBuilt || H.partitioned || !H.treeless || !H.shadePacked || H.reordered) return decline("the scene is not a two-level scene without the flat tree");
  if (T.instTrav.size() != oldInstances || T.instBoxes.size() != 6u * (size_t)oldInstances || T.meshBlasTri.size() != mesh0 || T.meshBlasNode.size() != mesh0 ||
      T.meshBlasLevels.size() != mesh0 || H.meshRecs.size() != mesh0) return decline("the host copy is not the built scene's"); // (cannot happen)
  for (const MeshBuild& mb : H.meshBuilds) if (mb.m->builtInstances != mb.instCount) return decline("a built mesh with another instance count"); // (cannot happen)
  const double t0 = nowMs();
  // --- the meshes to append: updateTopology's selection loop -- what a fresh build would hold and the resident scene does not, all behind every built mesh
  struct NewMesh { GiCMesh* m; uint32_t material, matFlags, vertexOffset, shadeBase, instFirst, instCount, nf, triFirst, idBase, blasNode, blasTri, faceFirst; float extent;
      Bvh8 blas; std::vector<uint32_t> order; std::vector<int32_t> faceIdAov; uint32_t blasBudget = 0; };
  std::vector<NewMesh> fresh;
  uint64_t appendedTris = 0, appendedFaces = 0, appendedInstances = 0, appendedVerts = 0;
  for (GiCMesh* m : s->meshes) {
    if (m->builtInstances != 0xffffffffu) { if (!fresh.empty()) return decline("a new mesh lies in front of a built one"); continue; }
    if (!m->visible || m->faces.empty()) continue; // (as buildScene)
    auto mit = std::find(s->materials.begin(), s->materials.end(), m->material);
    if (mit == s->materials.end()) continue;
    const uint32_t material = (uint32_t)(mit - s->materials.begin());
    if (material > 0x00ffffffu) return decline("a material index above 2^24");
    if (!usableVertexPositions(m->vertices.data(), m->vertices.size())) return decline("a new mesh has a vertex position that is not usable");
    const uint64_t instCount = m->instanceTransforms.size() / 16;
    if (instCount == 0u) continue; // (no instance: a fresh build holds a MeshBuild without records; the next build takes it up)
    NewMesh nm{}; nm.m = m; nm.material = material; nm.instCount = (uint32_t)instCount; nm.nf = (uint32_t)m->faces.size();
    fresh.push_back(std::move(nm));
    appendedTris += instCount * m->faces.size(); appendedFaces += m->faces.size(); appendedInstances += instCount; appendedVerts += m->vertices.size();
  }
  // --- what the scene holds after the edit
  uint64_t live = appendedTris, retired = 0, visible = appendedTris; uint32_t retiring = 0;
  for (const MeshBuild& mb : H.meshBuilds) {
    const uint64_t n = (uint64_t)mb.instCount * mb.m->faces.size(), gone = (uint64_t)mb.retiredInst * mb.m->faces.size(); // (gone: the free slots of retired instances)
    if (mb.m->retired) { retired += n + gone; if (!mb.hidden) retiring++; } else { live += n; retired += gone; if (!mb.hidden) visible += n; }
  }
  if (visible < kIncrementalMinTris) return decline("fewer than 4096 visible triangles after the edit");
  // (GI_C_SCENE_OPTION_TLAS_COMPACTION, where this stage has an edit of its own to apply -- a sync of instancer edits alone asked above, before it retired its
  // slots: the counts and bases above are those of the scene as it was, and they are taken again)
  if (!afterCompaction && (!fresh.empty() || retiring != 0u)) {
    int rc = GI_C_OK;
    if (compactBeforeEdit(s, H, retired, live, cost, rc)) return updateTopologyTwoLevel(s, H, handled, cost, true);
    if (rc != GI_C_OK) return GI_C_ERROR;
  }
  if (retired > live) return decline("retired triangles outnumber live ones");
  if ((uint64_t)oldTris + appendedTris >= ((uint64_t)1 << 28)) return decline("2^28 or more flat records after the append");
  if ((uint64_t)blasTri0 + appendedFaces >= ((uint64_t)1 << 26)) return decline("2^26 or more unique BLAS triangles after the append");
  if ((uint64_t)oldInstances + appendedInstances >= 0xffffffffull || (uint64_t)vert0 + appendedVerts >= 0xffffffffull) return decline("the arrays outgrow 32-bit indices");
  if (fresh.empty() && retiring == 0u) { // the edited meshes are not part of a fresh build either (invisible, no faces, no instance, no valid material)
    for (GiCMesh* m : s->meshes) if (m->builtInstances == 0xffffffffu) { m->visToggled = false; m->vertsEdited = false; }
    handled = true;
    return GI_C_OK;
  }
  // --- retire: the plan (nothing resident is touched yet)
  VisibilityPlan plan;
  if (!planVisibility(s, H, [](const MeshBuild& mb) { return mb.hidden || mb.m->retired; }, plan)) return decline("a built mesh with another instance count");
  // --- append, planned: the new meshes' words come from the current material table (updateMaterials runs behind this update when an edit is due)
  std::vector<MaterialRec> mats;
  const bool matsRemade = (s->dirty & DIRTY_MATERIALS) != 0u;
  if (matsRemade) buildMaterialRecords(s, mats);
  const std::vector<MaterialRec>& matTable = matsRemade ? mats : H.mats;
  const uint32_t newInstances = oldInstances + (uint32_t)appendedInstances, newTris = oldTris + (uint32_t)appendedTris;
  std::vector<FVertex> newVerts; newVerts.reserve(appendedVerts);
  std::vector<InstanceRec> newInst; newInst.reserve(appendedInstances);
  std::vector<uint32_t> faces3, orderAll; std::vector<int32_t> faceIdAll; // the per-face temporaries of all new meshes, one upload each
  faces3.reserve(3u * appendedFaces); orderAll.reserve(appendedFaces); faceIdAll.reserve(appendedFaces);
  std::vector<MeshRec> meshRecs(H.meshRecs); std::vector<float> sceneData(H.sceneData);
  {
    uint64_t idBase = plan.visibleTris; uint32_t vertexOffset = vert0, shadeBase = shade0, instFirst = oldInstances, triFirst = oldTris, faceFirst = 0;
    for (NewMesh& nm : fresh) {
      GiCMesh* m = nm.m;
      if (nm.material >= matTable.size()) return decline("a new mesh's material is not in the material table"); // (cannot happen: creating a material raises DIRTY_MATERIALS)
      nm.matFlags = meshMatFlags(matTable[nm.material], nm.material, m);
      nm.vertexOffset = vertexOffset; nm.shadeBase = shadeBase; nm.instFirst = instFirst; nm.triFirst = triFirst; nm.idBase = (uint32_t)idBase; nm.faceFirst = faceFirst;
      appendMeshSceneData(m, m->material, vertexOffset, meshRecs, sceneData);
      for (const GiCVertex& vIn : m->vertices) newVerts.push_back(packVertex(vIn));
      for (const GiCFace& f : m->faces) { faces3.push_back(f.v_i[0]); faces3.push_back(f.v_i[1]); faces3.push_back(f.v_i[2]); }
      nm.faceIdAov = faceIdAovOf(m);
      faceIdAll.insert(faceIdAll.end(), nm.faceIdAov.begin(), nm.faceIdAov.end());
      for (uint32_t ii = 0; ii < nm.instCount; ii++) {
        newInst.push_back(makeInstanceRec(m, mesh0 + (uint32_t)(&nm - fresh.data()), ii));
        if (!usableInstance(newInst.back())) return decline("a new instance has a transform that is not usable");
      }
      vertexOffset += (uint32_t)m->vertices.size(); shadeBase += nm.nf; instFirst += nm.instCount; triFirst += nm.instCount * nm.nf; faceFirst += nm.nf;
      idBase += (uint64_t)nm.instCount * nm.nf;
    }
  }
  // --- the new BLASes, by the host builder exactly as buildTwoLevel runs it; their records in the builder's order (the bounds kernels read them from scratch).
  // With GI_C_SCENE_OPTION_BLAS_DEVICE_BUILD wanted the meshes within blas_device_min .. blas_device_max go through makeMeshBlas first, one after the other on
  // the build stream with the scene's one slab, under the budget the resident TLAS's depth leaves; the others stay with the host builder, in parallel
  const double tb0 = nowMs();
  std::vector<uint8_t> blasOk(fresh.size(), 1), blasMade(fresh.size(), 0);
  std::vector<float> blasExtent(fresh.size(), 0.0f);
  if (blasDeviceBuildWanted(s))
    for (size_t k = 0; k < fresh.size(); k++) {
      NewMesh& nm = fresh[k];
      const int range = blasDeviceRange(nm.nf);
      if (range != 0) {
        s->blasBuildStats[range]++;
        if (timing) fprintf(stderr, "[gatling_gi] BLAS of %u faces: the host builder (%s)\n", nm.nf, range == 1 ? "under blas_device_min" : "over blas_device_max");
        continue;
      }
      float mlo[3], mhi[3];
      nm.blasBudget = makeMeshBlas(s, true, T.tlasDepth, nm.m, nm.blas, nm.order, mlo, mhi);
      blasExtent[k] = (std::fabs(mlo[0]) + std::fabs(mlo[1]) + std::fabs(mlo[2])) + (std::fabs(mhi[0]) + std::fabs(mhi[1]) + std::fabs(mhi[2]));
      blasMade[k] = 1;
    }
  parallelOver(fresh.size(), [&](size_t k) {
    NewMesh& nm = fresh[k];
    float mlo[3], mhi[3];
    if (!blasMade[k]) buildMeshBlas(nm.m->vertices.data(), nm.m->faces.data(), nm.nf, nm.blas, nm.order, mlo, mhi);
    if (blasMade[k]) nm.extent = blasExtent[k]; else
    nm.extent = (std::fabs(mlo[0]) + std::fabs(mlo[1]) + std::fabs(mlo[2])) + (std::fabs(mhi[0]) + std::fabs(mhi[1]) + std::fabs(mhi[2])); // (buildTwoLevel's)
    blasOk[k] = nm.order.size() == nm.nf && !nm.blas.nodes.empty() && nm.blas.levelStart.size() >= 2u && nm.blas.levelStart.back() == nm.blas.nodes.size();
    for (const uint32_t f : nm.order) if (f >= nm.nf) blasOk[k] = 0;
  });
  const double blasMs = nowMs() - tb0;
  for (const uint8_t ok : blasOk) if (!ok) return decline("a new mesh's BLAS has no level table"); // (cannot happen)
  std::vector<Node8> newBlasNodes; std::vector<BlasTri> newBlasTris; newBlasTris.reserve(appendedFaces);
  std::vector<InstTrav> newTrav; newTrav.reserve(appendedInstances);
  std::vector<InstBoundsJob> jobs; jobs.reserve(appendedInstances);
  uint32_t blasDepth = T.blasDepth, chunksPerJob = 0;
  for (NewMesh& nm : fresh) {
    nm.blasNode = blasNode0 + (uint32_t)newBlasNodes.size(); nm.blasTri = blasTri0 + (uint32_t)newBlasTris.size();
    const uint32_t scratchFirst = (uint32_t)newBlasTris.size();
    for (Node8 n : nm.blas.nodes) { n.childBase += nm.blasNode; n.triBase += nm.blasTri; newBlasNodes.push_back(n); }
    for (const uint32_t f : nm.order) { newBlasTris.push_back(makeBlasTri(nm.m->vertices.data(), nm.m->faces.data(), f)); orderAll.push_back(f); }
    blasDepth = std::max(blasDepth, nm.blas.maxDepth);
    for (uint32_t ii = 0; ii < nm.instCount; ii++) {
      const InstanceRec& ir = newInst[nm.instFirst - oldInstances + ii];
      newTrav.push_back(tlasMakeInstTrav(ir, nm.blasNode, nm.idBase + ii * nm.nf, nm.matFlags, nm.extent));
      InstBoundsJob j{}; memcpy(j.o2w, ir.o2w, sizeof(j.o2w)); j.firstTri = scratchFirst; j.faceCount = nm.nf; j.instance = nm.instFirst + ii;
      jobs.push_back(j);
    }
    chunksPerJob = std::max(chunksPerJob, instBoundsChunks(nm.nf));
  }
  if ((uint64_t)jobs.size() * chunksPerJob >= (1ull << 31)) return decline("more bounds workgroups than a launch takes");
  // --- primary device, scratch only: padded world boxes and statuses of the new instances
  std::vector<uint32_t> result;
  bool outOfMemory = false;
  const double tA = nowMs();
  if (!jobs.empty()) {
    const int rcB = instanceBoundsOnPrimary(s, jobs, chunksPerJob, &newBlasTris, result, outOfMemory, what);
    if (rcB == DEVICE_BUILD_FALLBACK && outOfMemory) return decline("out of device memory");
    if (rcB != GI_C_OK) return GI_C_ERROR;
  }
  const double boundsMs = nowMs() - tA;
  for (size_t k = 0; k < jobs.size(); k++)
    if (result[7u * k + 6u] != 0u) return decline("a new instance carries triangles that leave the usable coordinate range in world space");
  // --- the TLAS over all boxes, hidden and retired instances masked; the depth rule with the new BLASes
  std::vector<float> boxes(T.instBoxes); boxes.resize(6u * (size_t)newInstances);
  for (size_t k = 0; k < jobs.size(); k++) memcpy(&boxes[6u * (size_t)jobs[k].instance], &result[7u * k], 24);
  std::vector<uint8_t> hiddenAfter(newInstances, 0);
  for (const MeshBuild& mb : H.meshBuilds) if (plan.hide[mb.meshIdx]) for (const uint32_t inst : mb.inst) if (inst < oldInstances) hiddenAfter[inst] = 1;
  markFreeSlots(H.meshBuilds, hiddenAfter);
  Bvh8 tlas; std::vector<uint32_t> tlasItems; TlasMade tlasMade;
  const double tt0 = nowMs();
  {
    std::vector<float> masked(boxes);
    tlasMaskHiddenBoxes(masked.data(), hiddenAfter.data(), newInstances);
    tlasMade = buildEditTlas(s, blasDepth, masked.data(), newInstances, tlas, tlasItems);
  }
  const double tlasMs = nowMs() - tt0;
  if (2u * tlas.maxDepth + blasDepth + 1u > 16u) return decline("the new TLAS is too deep for the 16-entry stack");
  // --- decided.  The host copies of the retire: the records where they are still held, the MeshBuilds' state; then the table's extra bit for the kernel
  const bool hostRecords = !H.hostTreeDropped && H.bvh.tris.size() == oldTris && H.triFaceId.size() == oldTris && H.flatOfOrig.size() == oldTris;
  applyVisibilityPlanOnHost(H, plan);
  for (uint32_t i = 0; i < oldInstances; i++) if (hiddenAfter[i]) plan.patch[i].action |= VIS_HIDDEN_AFTER;
  const std::vector<VisPatch>& patch = plan.patch;
  const uint32_t newShade = shade0 + (uint32_t)appendedFaces, newVertCount = vert0 + (uint32_t)appendedVerts;
  const uint32_t newBlasNodeCount = blasNode0 + (uint32_t)newBlasNodes.size(), newBlasTriCount = blasTri0 + (uint32_t)newBlasTris.size();
  const double t1 = nowMs();
  // --- every device of the scene, on its own stream: the arrays grown and the temporaries allocated before anything resident changes
  double appendKernelMs = 0.0;
  const size_t bytesSent = (plan.launch ? patch.size() * sizeof(VisPatch) : 0u) + newVerts.size() * sizeof(FVertex) + newInst.size() * (sizeof(InstanceRec) + sizeof(InstTrav)) +
      newBlasNodes.size() * sizeof(Node8) + faces3.size() * 4u + orderAll.size() * 4u + faceIdAll.size() * 4u + tlas.nodes.size() * sizeof(Node8) + tlasItems.size() * 4u +
      meshRecs.size() * sizeof(MeshRec) + sceneData.size() * sizeof(float);
  const int rcDev = onSceneDevices(s, residentDeviceCount(s), [&](SceneDevice& D, hipStream_t st) -> int {
    if (D.dTris.count < oldTris || D.dTriFaceId.count < oldTris || D.dFlatOfOrig.count < oldTris || D.dInstances.count < oldInstances || D.dInstTrav.count < oldInstances ||
        D.dTriShade.count < shade0 || D.dVerts.count < vert0 || D.dBlasNodes.count < blasNode0 || D.dBlasTris.count < blasTri0) {
      setError("internal: the device holds less than the scene"); return GI_C_ERROR; }
    std::vector<void*> old;
    DeviceBuffer<VisPatch> dPatch; DeviceBuffer<uint32_t> dFaces, dOrder; DeviceBuffer<int32_t> dFaceIds;
    auto releaseAll = [&] { dPatch.release(); dFaces.release(); dOrder.release(); dFaceIds.release(); for (void* p : old) (void)hipFree(p); old.clear(); };
    int r = plan.launch ? dPatch.alloc(patch.size()) : GI_C_OK;
    if (r == GI_C_OK && !fresh.empty()) { r = dFaces.alloc(faces3.size()); if (r == GI_C_OK) r = dOrder.alloc(orderAll.size()); if (r == GI_C_OK) r = dFaceIds.alloc(faceIdAll.size()); }
    if (r == GI_C_OK) r = D.dVerts.grow(newVertCount, st, old);
    if (r == GI_C_OK) r = D.dTriShade.grow(newShade, st, old);
    if (r == GI_C_OK) r = D.dInstances.grow(newInstances, st, old);
    if (r == GI_C_OK) r = D.dInstTrav.grow(newInstances, st, old);
    if (r == GI_C_OK) r = D.dBlasNodes.grow(newBlasNodeCount, st, old);
    if (r == GI_C_OK) r = D.dBlasTris.grow(newBlasTriCount, st, old);
    if (r == GI_C_OK) r = D.dTris.grow(newTris, st, old);
    if (r == GI_C_OK) r = D.dTriFaceId.grow(newTris, st, old);
    if (r == GI_C_OK) r = D.dFlatOfOrig.grow(newTris, st, old);
    if (r != GI_C_OK) { // (the copies out of the old blocks must finish before they are freed)
      (void)hipStreamSynchronize(st); releaseAll();
      if (r == GI_C_OUT_OF_MEMORY_INTERNAL) { outOfMemory = true; return DEVICE_BUILD_FALLBACK; }
      return GI_C_ERROR;
    }
    auto copy = [&](void* dst, const void* src, size_t bytes) {
      if (r == GI_C_OK && bytes && hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, st) != hipSuccess) { setError("topology update (two-level): copy failed"); r = GI_C_ERROR; } };
    // the retire: ids, the id table and the instances' id bases, over what was resident before the append
    if (plan.launch) {
      copy(dPatch.ptr, patch.data(), patch.size() * sizeof(VisPatch));
      if (r == GI_C_OK) {
        launchPatchVisibility2(st, D.dTris.ptr, oldTris, D.dInstances.ptr, oldInstances, dPatch.ptr, D.dTriShade.ptr, shade0, D.dFlatOfOrig.ptr, newTris);
        if (plan.renumbered) launchPatchInstTrav(st, D.dInstTrav.ptr, oldInstances, dPatch.ptr);
      }
    }
    // the append: what the host made per vertex, per face and per instance ...
    copy(D.dVerts.ptr + vert0, newVerts.data(), newVerts.size() * sizeof(FVertex));
    copy(D.dInstances.ptr + oldInstances, newInst.data(), newInst.size() * sizeof(InstanceRec));
    copy(D.dInstTrav.ptr + oldInstances, newTrav.data(), newTrav.size() * sizeof(InstTrav));
    copy(D.dBlasNodes.ptr + blasNode0, newBlasNodes.data(), newBlasNodes.size() * sizeof(Node8));
    copy(dFaces.ptr, faces3.data(), faces3.size() * 4u); copy(dOrder.ptr, orderAll.data(), orderAll.size() * 4u); copy(dFaceIds.ptr, faceIdAll.data(), faceIdAll.size() * 4u);
    if (r == GI_C_OK && (D.dTlasNodes.upload(tlas.nodes, st) || D.dTlasItems.upload(tlasItems, st) || D.dMeshes.upload(meshRecs, st) || D.dSceneData.upload(sceneData, st))) r = GI_C_ERROR;
    // ... and everything per face and per flattened triangle, made where it lives (gi_append.hip), behind those copies on the same stream
    double tk = 0.0;
    if (r == GI_C_OK && timing && D.slot == 0u) { if (hipStreamSynchronize(st) != hipSuccess) r = GI_C_ERROR; tk = nowMs(); }
    for (const NewMesh& nm : fresh) {
      if (r != GI_C_OK) break;
      AppendMesh M{}; M.triFirst = nm.triFirst; M.faceCount = nm.nf; M.instFirst = nm.instFirst; M.instCount = nm.instCount; M.shadeBase = nm.shadeBase; M.idBase = nm.idBase;
      M.matFlags = nm.matFlags; M.triCount = newTris; M.instanceCount = newInstances; M.shadeCount = newShade; M.flatCount = newTris;
      if (!launchAppendShadeIndex(st, D.dTriShade.ptr, newShade, nm.shadeBase, dFaces.ptr + 3u * (size_t)nm.faceFirst, nm.nf, nm.vertexOffset) ||
          !launchGatherShade(st, D.dTriShade.ptr, newShade, nm.shadeBase, nm.nf, D.dVerts.ptr, newVertCount) ||
          !launchAppendBlasTris(st, D.dBlasTris.ptr, newBlasTriCount, nm.blasTri, dOrder.ptr + nm.faceFirst, nm.nf, D.dTriShade.ptr, newShade, nm.shadeBase) ||
          !launchAppendRecords(st, M, D.dTris.ptr, D.dTriFaceId.ptr, D.dFlatOfOrig.ptr, D.dInstances.ptr, D.dTriShade.ptr, dFaceIds.ptr + nm.faceFirst)) {
        setError("internal: an appended mesh's records outside their arrays"); r = GI_C_ERROR; } // (cannot happen: the arrays were grown to hold them)
    }
    if (r == GI_C_OK && hipGetLastError() != hipSuccess) { setError("topology update (two-level): launch failed"); r = GI_C_ERROR; }
    if (hipStreamSynchronize(st) != hipSuccess && r == GI_C_OK) { setError("topology update (two-level): device error"); r = GI_C_ERROR; }
    if (timing && D.slot == 0u && r == GI_C_OK) appendKernelMs = nowMs() - tk;
    releaseAll(); // (before the render's memory plan reads free memory)
    return r;
  });
  if (rcDev == DEVICE_BUILD_FALLBACK && outOfMemory) return decline("out of device memory");
  if (rcDev != GI_C_OK) return GI_C_ERROR;
  const double t2 = nowMs();
  // --- the host copies behind the committed edit: the retire ...
  if (plan.launch) {
    patchInstTravHost(T.instTrav.data(), oldInstances, patch.data());
    if (hostRecords) {
      constexpr size_t CHUNK = 65536;
      const size_t n = oldTris;
      parallelOver((n + CHUNK - 1) / CHUNK, [&](size_t c) { // (one writer per word: the visible ids are a permutation)
        for (size_t i = c * CHUNK; i < std::min(n, (c + 1) * CHUNK); i++) {
          const TriRec& t = H.bvh.tris[i];
          if (t.instance < oldInstances && !hiddenAfter[t.instance] && t.origId < n) H.flatOfOrig[t.origId] = (uint32_t)i;
        }
      });
    } else std::vector<uint32_t>().swap(H.flatOfOrig); // (stale with the dropped host records; nothing reads it before the next build makes it anew)
  }
  // ... and the append
  H.verts.insert(H.verts.end(), newVerts.begin(), newVerts.end());
  H.instances.insert(H.instances.end(), newInst.begin(), newInst.end());
  H.meshRecs.swap(meshRecs); H.sceneData.swap(sceneData);
  if (matsRemade) H.mats.swap(mats);
  T.blasNodes.insert(T.blasNodes.end(), newBlasNodes.begin(), newBlasNodes.end()); T.blasTris.insert(T.blasTris.end(), newBlasTris.begin(), newBlasTris.end());
  T.instTrav.insert(T.instTrav.end(), newTrav.begin(), newTrav.end());
  T.instBoxes.swap(boxes); T.tlasNodes.swap(tlas.nodes); T.tlasItems.swap(tlasItems); T.tlasDepth = tlas.maxDepth; T.blasDepth = blasDepth; noteTlasMade(T, tlasMade);
  // (25 % slack, as on the device and as updateTopology grows its host arrays: a std::vector would double 4.3 GB of records on the first append to a
  // 67.7 M-triangle scene and copy them on every later doubling)
  auto grown = [](auto& v, size_t n) { if (v.capacity() < n) v.reserve(n + n / 4u); v.resize(n); };
  if (hostRecords) { grown(H.bvh.tris, newTris); grown(H.triFaceId, newTris); grown(H.flatOfOrig, newTris); }
  else { // dropped by an edit in place before: they stay dropped, and the id table -- one word per resident record -- goes with them
    std::vector<uint32_t>().swap(H.flatOfOrig);
    if (!H.hostTreeDropped) { std::vector<TriRec>().swap(H.bvh.tris); std::vector<int32_t>().swap(H.triFaceId); H.hostTreeDropped = true; } // (cannot happen)
  }
  for (NewMesh& nm : fresh) {
    GiCMesh* m = nm.m;
    const uint32_t meshIdx = (uint32_t)H.meshBuilds.size();
    for (const GiCFace& f : m->faces) H.triShade.push_back(packTriShade(m->vertices.data(), f, nm.vertexOffset));
    H.meshBuilds.push_back(MeshBuild{m, nm.vertexOffset, nm.matFlags, nm.instFirst, nm.instCount, nm.triFirst, meshIdx, nm.faceIdAov});
    H.meshBuilds.back().shadeBase = nm.shadeBase; H.meshBuilds.back().idBase = nm.idBase; H.meshBuilds.back().numberInstances();
    T.meshBlasTri.push_back(nm.blasTri); T.meshBlasNode.push_back(nm.blasNode); T.meshBlasLevels.push_back(nm.blas.levelStart);
    T.meshBlasBudget.resize(T.meshBlasNode.size() - 1u, 0u); T.meshBlasBudget.push_back(nm.blasBudget);
    if (hostRecords) { // the flat records, face ids and id-table words by the kernels' own form
      AppendMesh M{}; M.triFirst = nm.triFirst; M.faceCount = nm.nf; M.instFirst = nm.instFirst; M.instCount = nm.instCount; M.shadeBase = nm.shadeBase; M.idBase = nm.idBase;
      M.matFlags = nm.matFlags; M.triCount = newTris; M.instanceCount = newInstances; M.shadeCount = (uint32_t)H.triShade.size(); M.flatCount = newTris;
      constexpr uint32_t CHUNK = 65536;
      const uint32_t items = nm.nf * nm.instCount;
      parallelOver(((size_t)items + CHUNK - 1) / CHUNK, [&](size_t c) {
        appendRecordsHost(M, (uint32_t)c * CHUNK, std::min(items, ((uint32_t)c + 1u) * CHUNK), H.bvh.tris.data(), H.triFaceId.data(), H.flatOfOrig.data(), H.instances.data(),
            H.triShade.data(), nm.faceIdAov.data());
      });
    }
    m->builtInstances = nm.instCount; m->xformDirty = false; m->instDirty.clear();
  }
  // (hdGatling calls the visibility setter on every new mesh; a mesh that stays out of the scene has nothing to toggle or refit)
  for (const NewMesh& nm : fresh) { nm.m->visToggled = false; nm.m->vertsEdited = false; }
  for (GiCMesh* m : s->meshes) if (m->builtInstances == 0xffffffffu) { m->visToggled = false; m->vertsEdited = false; }
  s->triCount = newTris; H.bvh.activeTris = newTris;
  // (with a material edit due as well the resident words index the previous table: updateMaterials derives the classes behind this update)
  if (!(s->dirty & DIRTY_MATERIALS)) deriveSceneClasses(s, H, false);
  setSceneBoundsFromInstances(s, H);
  const double t3 = nowMs();
  cost.buildMs = instancerCost.buildMs + tlasMs + blasMs; cost.uploadMs = instancerCost.uploadMs + std::max(t3 - t0 - tlasMs - blasMs, 0.0);
  if (timing) fprintf(stderr, "[gatling_gi] topology update (two-level): %u mesh(es) retired, %zu appended (%llu face(s), %llu instance(s), %llu flat record(s) made on the "
                              "device), %llu live + %llu retired triangle(s), %u resident, TLAS %zu node(s), host TLAS build %.2f ms, host BLAS build %.2f ms, host rest "
                              "%.2f ms, device %.2f ms (bounds kernels + read-back %.2f, commit %.2f of which append kernels %.3f), %zu bytes sent per device\n",
                      retiring, fresh.size(), (unsigned long long)appendedFaces, (unsigned long long)appendedInstances, (unsigned long long)appendedTris,
                      (unsigned long long)live, (unsigned long long)retired, s->triCount, T.tlasNodes.size(), tlasMs, blasMs,
                      std::max((t1 - t0) - tlasMs - blasMs - boundsMs + (t3 - t2), 0.0), boundsMs + (t2 - t1), boundsMs, t2 - t1, appendKernelMs, bytesSent);
  handled = true;
  return GI_C_OK;
}

// What the checks of a resident two-level scene ignore once updateTopologyTwoLevel has retired meshes: one byte per BLAS node, per BLAS triangle and per
// instance, 1 inside the ranges of a retired mesh (destroyed: its records stay resident until the next build and nothing reaches them -- its instances are
// out of the TLAS).  `layout`: first BLAS node / triangle and levels by meshIdx, of arrays laid out in storage order.  Empty masks: no mesh is retired
struct RetiredRanges { std::vector<uint8_t> node, tri, inst; };
static RetiredRanges retiredRangesOf(const SceneHost& H, const TwoLevelHost& layout, size_t nodeCount, size_t triCount)
{
  RetiredRanges R;
  auto begin = [&] { if (R.inst.empty()) { R.node.assign(nodeCount, 0); R.tri.assign(triCount, 0); R.inst.assign(H.instances.size(), 0); } };
  // (the slots retired instances of a live mesh left, updateInstancesTwoLevel: their traversal records are stale until a grow takes them)
  for (const MeshBuild& mb : H.meshBuilds) for (const MeshBuild::FreeSlot& fs : mb.freeSlots) { begin(); if (fs.inst < R.inst.size()) R.inst[fs.inst] = 1; }
  for (const MeshBuild& mb : H.meshBuilds) {
    if (!mb.m->retired || mb.instCount == 0u) continue;
    begin();
    if (mb.meshIdx >= layout.meshBlasNode.size() || mb.meshIdx >= layout.meshBlasTri.size() || mb.meshIdx >= layout.meshBlasLevels.size()) continue;
    const std::vector<uint32_t>& lv = layout.meshBlasLevels[mb.meshIdx];
    const size_t n0 = layout.meshBlasNode[mb.meshIdx], t0 = layout.meshBlasTri[mb.meshIdx], nn = lv.empty() ? 0u : lv.back(), nf = mb.m->faces.size();
    for (size_t i = n0; i < std::min(n0 + nn, nodeCount); i++) R.node[i] = 1;
    for (size_t i = t0; i < std::min(t0 + nf, triCount); i++) R.tri[i] = 1;
    for (const uint32_t inst : mb.inst) if (inst < R.inst.size()) R.inst[inst] = 1;
  }
  return R;
}

// "What the scene's own code makes anew" where the device builder made the resident TLAS (GI_C_SCENE_OPTION_TLAS_DEVICE_BUILD; TwoLevelHost::tlasDeviceBuilt):
// the comparison TLAS of giCDebugSceneTlasCheck / giCDebugSceneBlasCheck is then the host form of that builder over the same masked boxes under the same depth
// budget, in place of buildTwoLevel's.  Nothing changes otherwise.
static bool freshTlasOfResidentBuilder(const SceneHost& H, size_t instanceCount, TwoLevelHost& fresh)
{
  if (!H.two.tlasDeviceBuilt) return true;
  std::vector<float> masked(fresh.instBoxes);
  const std::vector<uint8_t> hidden = hiddenOfInstances(H.meshBuilds, instanceCount);
  tlasMaskHiddenBoxes(masked.data(), hidden.data(), instanceCount);
  TlasBuildInfo info;
  const uint32_t radius = (uint32_t)std::min(std::max(optionValue("ploc_radius", 16), 1L), 256L);
  if (masked.size() != 6u * instanceCount || buildTlasHost(masked.data(), instanceCount, H.two.tlasBuildBudget, radius, fresh.tlasNodes, fresh.tlasItems, info) != TLAS_BUILD_OK) return false;
  fresh.tlasDepth = info.maxDepth;
  return true;
}

// giCDebugSceneTlasCheck: the two-level arrays resident on a device against the arrays buildTwoLevel makes anew from the scene's current meshes, bytewise
// (storage order: retired meshes and appended ones included, as updateTopologyTwoLevel leaves them; the ranges and records of a retired mesh are ignored)
extern "C" int giCDebugSceneTlasCheck(const GiCScene* scene, uint32_t deviceIndex, uint32_t* out)
{
  GiCScene* s = const_cast<GiCScene*>(scene);
  if (!g_ctx.initialized || !s || !out) { setError("giCDebugSceneTlasCheck: bad arguments"); return -1; }
  std::lock_guard<std::mutex> guard(s->mutex);
  if (!s->host) { setError("giCDebugSceneTlasCheck: the scene has not been built (render it once)"); return -1; }
  if (deviceIndex > s->replicas.size() || deviceIndex >= sceneDeviceCount(s)) { setError("giCDebugSceneTlasCheck: no such device copy"); return -1; }
  const SceneHost& H = *s->host;
  out[0] = s->twoLevel ? 1u : 0u; out[1] = (uint32_t)H.instances.size(); out[2] = (uint32_t)H.two.tlasNodes.size(); out[3] = H.two.tlasDepth;
  if (!s->twoLevel) { out[2] = out[3] = 0u; return 0; }
  try {
    std::vector<InstanceRec> instances(H.instances.size());
    for (const MeshBuild& mb : H.meshBuilds) {
      if (mb.m->instanceTransforms.size() != (size_t)mb.instCount * 16u) { setError("giCDebugSceneTlasCheck: a mesh's instance count is not the built one (render first)"); return -1; }
      for (uint32_t ii = 0; ii < mb.instCount; ii++) instances[mb.inst[ii]] = makeInstanceRec(mb.m, mb.meshIdx, ii);
    }
    TwoLevelHost fresh;
    const int rc = buildTwoLevel(s, H.meshBuilds, instances, s->triCount, s->nodeCount, fresh);
    const bool stillTwoLevel = s->twoLevel;
    s->twoLevel = true; // (buildTwoLevel answers through it: the resident scene is what it was)
    if (rc != GI_C_OK || !stillTwoLevel) { setError("giCDebugSceneTlasCheck: a fresh build of the current meshes would not use the two-level layout"); return -1; }
    if (!freshTlasOfResidentBuilder(H, instances.size(), fresh)) { setError("giCDebugSceneTlasCheck: the host form of the device TLAS builder failed"); return -1; }
    SceneDevice& D = sceneDevice(s, deviceIndex);
    std::vector<Node8> tlasNodes(fresh.tlasNodes.size()), blasNodes(fresh.blasNodes.size()); std::vector<uint32_t> tlasItems(fresh.tlasItems.size());
    std::vector<BlasTri> blasTris(fresh.blasTris.size()); std::vector<InstTrav> instTrav(fresh.instTrav.size());
    int differ = 0;
    // (a resident array shorter than the fresh one: every missing record differs; the TLAS buffers may be longer -- they keep their block when the tree shrinks)
    auto fetch = [&](auto& host, const auto& dev) -> bool {
      using R = typename std::remove_reference<decltype(host)>::type::value_type;
      const size_t n = std::min(host.size(), dev.ptr ? dev.count : (size_t)0);
      differ += (int)(host.size() - n);
      host.resize(n);
      return n == 0u || hipMemcpy(host.data(), dev.ptr, n * sizeof(R), hipMemcpyDeviceToHost) == hipSuccess;
    };
    bool ok = hipSetDevice(g_ctx.devs[D.slot].device) == hipSuccess;
    ok = ok && fetch(tlasNodes, D.dTlasNodes) && fetch(tlasItems, D.dTlasItems) && fetch(instTrav, D.dInstTrav) && fetch(blasNodes, D.dBlasNodes) && fetch(blasTris, D.dBlasTris);
    (void)hipSetDevice(g_ctx.device);
    if (!ok) { setError("giCDebugSceneTlasCheck: download failed"); return -1; }
    if (H.two.tlasNodes.size() != fresh.tlasNodes.size()) differ++; // (the host copy the next update starts from)
    // (a retired mesh is a hidden one whose ranges are ignored: the fresh arrays hold it in storage order, so every live and appended mesh's BLAS range is
    // compared where it lies; the TLAS, which names no instance of it, and the live instances' records are compared whole)
    const RetiredRanges ignored = retiredRangesOf(H, fresh, fresh.blasNodes.size(), fresh.blasTris.size());
    const std::vector<uint8_t> none;
    auto compare = [&](const auto& got, const auto& want, const std::vector<uint8_t>& skip) {
      using R = typename std::remove_reference<decltype(got)>::type::value_type;
      for (size_t i = 0; i < got.size(); i++) if (!(i < skip.size() && skip[i]) && memcmp(&got[i], &want[i], sizeof(R)) != 0) differ++;
    };
    compare(tlasNodes, fresh.tlasNodes, none); compare(tlasItems, fresh.tlasItems, none); compare(instTrav, fresh.instTrav, ignored.inst);
    compare(blasNodes, fresh.blasNodes, ignored.node); compare(blasTris, fresh.blasTris, ignored.tri);
    out[2] = (uint32_t)fresh.tlasNodes.size(); out[3] = fresh.tlasDepth;
    return differ;
  } catch (const std::exception& e) { s->twoLevel = true; setError(std::string("giCDebugSceneTlasCheck: ") + e.what()); return -1; }
}

// giCDebugSceneFlatIdCheck: the flat records, the id table and the InstTrav records resident on a device against the rules a visibility update in place of the
// two-level layout must keep (gi_vispatch.h flatIdViolations)
extern "C" int giCDebugSceneFlatIdCheck(const GiCScene* scene, uint32_t deviceIndex, uint32_t* out)
{
  GiCScene* s = const_cast<GiCScene*>(scene);
  if (!g_ctx.initialized || !s || !out) { setError("giCDebugSceneFlatIdCheck: bad arguments"); return -1; }
  std::lock_guard<std::mutex> guard(s->mutex);
  if (!s->host) { setError("giCDebugSceneFlatIdCheck: the scene has not been built (render it once)"); return -1; }
  if (deviceIndex > s->replicas.size() || deviceIndex >= sceneDeviceCount(s)) { setError("giCDebugSceneFlatIdCheck: no such device copy"); return -1; }
  const SceneHost& H = *s->host;
  const uint32_t instanceCount = (uint32_t)H.instances.size();
  out[0] = 0u; out[1] = s->triCount; out[2] = 0u; out[3] = s->twoLevel ? 1u : 0u;
  if (!s->twoLevel) return 0;
  try {
    const std::vector<uint8_t> hidden = hiddenOfInstances(H.meshBuilds, instanceCount);
    for (const uint8_t h : hidden) out[2] += h;
    SceneDevice& D = sceneDevice(s, deviceIndex);
    if (D.dTris.count < s->triCount || D.dFlatOfOrig.count < s->triCount || D.dInstTrav.count < instanceCount) { setError("giCDebugSceneFlatIdCheck: the device holds less than the scene"); return -1; }
    std::vector<TriRec> tris(s->triCount); std::vector<uint32_t> flat(s->triCount); std::vector<InstTrav> instTrav(instanceCount);
    bool ok = hipSetDevice(g_ctx.devs[D.slot].device) == hipSuccess;
    ok = ok && (tris.empty() || hipMemcpy(tris.data(), D.dTris.ptr, tris.size() * sizeof(TriRec), hipMemcpyDeviceToHost) == hipSuccess);
    ok = ok && (flat.empty() || hipMemcpy(flat.data(), D.dFlatOfOrig.ptr, flat.size() * sizeof(uint32_t), hipMemcpyDeviceToHost) == hipSuccess);
    ok = ok && (instTrav.empty() || hipMemcpy(instTrav.data(), D.dInstTrav.ptr, instTrav.size() * sizeof(InstTrav), hipMemcpyDeviceToHost) == hipSuccess);
    (void)hipSetDevice(g_ctx.device);
    if (!ok) { setError("giCDebugSceneFlatIdCheck: download failed"); return -1; }
    std::vector<uint8_t> seen(tris.size(), 0);
    uint32_t bad = flatIdViolations(tris.data(), (uint32_t)tris.size(), flat.data(), (uint32_t)flat.size(), instTrav.data(), hidden.data(), instanceCount, seen.data(), out[0]);
    // (the host copies the next update starts from: the instances' id bases, and the records and the table where they are still held)
    for (uint32_t i = 0; i < instanceCount && i < (uint32_t)H.two.instTrav.size(); i++) if (H.two.instTrav[i].triBase != instTrav[i].triBase) bad++;
    if (H.bvh.tris.size() == tris.size() && H.flatOfOrig.size() == flat.size())
      for (size_t i = 0; i < tris.size(); i++) {
        if (memcmp(&H.bvh.tris[i], &tris[i], sizeof(TriRec)) != 0) bad++;
        if (tris[i].instance < instanceCount && !hidden[tris[i].instance] && tris[i].origId < flat.size() && H.flatOfOrig[tris[i].origId] != flat[tris[i].origId]) bad++;
      }
    return (int)bad;
  } catch (const std::exception& e) { setError(std::string("giCDebugSceneFlatIdCheck: ") + e.what()); return -1; }
}

// giCDebugPatchVisibilityTwoLevel: k_patch_visibility2 + k_patch_inst_trav over synthetic records against the host form of the same code (gi_vispatch.h), and
// the host form against the numbering a fresh build of the instances visible after the edit gives
extern "C" int giCDebugPatchVisibilityTwoLevel(const uint32_t* faceCounts, const uint8_t* hiddenBefore, const uint8_t* hiddenAfter, uint32_t instanceCount,
    uint32_t seed, uint32_t* outTris)
{
  if (!g_ctx.initialized) { setError("giCDebugPatchVisibilityTwoLevel before giCInitialize"); return -1; }
  if (!faceCounts || !hiddenBefore || !hiddenAfter || instanceCount == 0u) { setError("giCDebugPatchVisibilityTwoLevel: bad arguments"); return -1; }
  uint64_t total = 0;
  for (uint32_t i = 0; i < instanceCount; i++) total += faceCounts[i];
  if (total == 0u || total >= (1ull << 26)) { setError("giCDebugPatchVisibilityTwoLevel: no triangles, or 2^26 and more"); return -1; }
  try {
    const uint32_t n = (uint32_t)total;
    std::mt19937 rng(seed);
    std::uniform_real_distribution<float> coord(-2.0f, 2.0f);
    // --- the scene: a pool of shading records (their corners alone), one instance record each, id bases before and after as planVisibility forms them --
    // a hidden instance keeps the base it had; before the edit that is the build's (all visible): it overlaps the ids of what lies behind it
    constexpr uint32_t kPool = 97u;
    std::vector<TriShade> shade(kPool);
    for (TriShade& q : shade) { q = TriShade{}; for (int k = 0; k < 3; k++) for (int a = 0; a < 3; a++) q.p[k][a] = coord(rng); }
    std::vector<InstanceRec> instances(instanceCount); std::vector<InstTrav> instTrav(instanceCount); std::vector<VisPatch> patch(instanceCount);
    std::vector<uint32_t> baseBefore(instanceCount), first(instanceCount);
    uint32_t built = 0, before = 0, after = 0;
    for (uint32_t i = 0; i < instanceCount; i++) {
      InstanceRec ir{}; const float o2w[12] = {1.0f + 0.01f * (float)(i % 7u), 0.1f, 0.0f, coord(rng), 0.0f, 0.9f, 0.2f, coord(rng), -0.1f, 0.0f, 1.1f, coord(rng)};
      memcpy(ir.o2w, o2w, sizeof(o2w)); ir.mesh = i; instances[i] = ir;
      first[i] = built;
      baseBefore[i] = hiddenBefore[i] ? built : before;
      const uint32_t baseAfter = hiddenAfter[i] ? baseBefore[i] : after;
      const bool hb = hiddenBefore[i] != 0, ha = hiddenAfter[i] != 0;
      patch[i] = VisPatch{(int32_t)(baseAfter - baseBefore[i]), (hb == ha ? VIS_KEEP : (ha ? VIS_HIDE : VIS_SHOW)) | (ha ? VIS_HIDDEN_AFTER : 0u)};
      InstTrav tv{}; memcpy(tv.o2w, o2w, sizeof(o2w)); tv.blasRoot = i; tv.triBase = baseBefore[i]; tv.matFlags = 0x01000000u | i; tv.slack = 1.0f; instTrav[i] = tv;
      built += faceCounts[i]; if (!hb) before += faceCounts[i]; if (!ha) after += faceCounts[i];
    }
    // --- the records in a shuffled flat order; the table as the build and the edits before leave it: visible records named, every other word stale
    std::vector<uint32_t> place(n);
    for (uint32_t i = 0; i < n; i++) place[i] = i;
    std::shuffle(place.begin(), place.end(), rng);
    std::vector<TriRec> tris(n); std::vector<uint32_t> flat(n, 0xdeadbeefu); std::vector<uint8_t> hiddenA(instanceCount);
    for (uint32_t i = 0; i < instanceCount; i++) {
      hiddenA[i] = hiddenAfter[i] ? 1 : 0;
      for (uint32_t f = 0; f < faceCounts[i]; f++) {
        TriRec t{}; t.instance = i; t.prim = f; t.origId = baseBefore[i] + f; t.matFlags = instTrav[i].matFlags; t.vi[0] = (first[i] + f) % kPool;
        refit_flatten(instances[i].o2w, shade[t.vi[0]].p, t.v0, t.e1, t.e2);
        if (hiddenBefore[i]) for (int a = 0; a < 3; a++) { t.e1[a] = 0.0f; t.e2[a] = 0.0f; }
        const uint32_t at = place[first[i] + f];
        tris[at] = t;
        if (!hiddenBefore[i]) flat[t.origId] = at;
      }
    }
    // --- the device
    std::vector<TriRec> devTris(n); std::vector<uint32_t> devFlat(n); std::vector<InstTrav> devTrav(instanceCount);
    DeviceBuffer<TriRec> dTris; DeviceBuffer<InstanceRec> dInstances; DeviceBuffer<VisPatch> dPatch; DeviceBuffer<TriShade> dShade; DeviceBuffer<uint32_t> dFlat;
    DeviceBuffer<InstTrav> dTrav;
    hipStream_t st = g_ctx.stream;
    bool ok = hipSetDevice(g_ctx.device) == hipSuccess && dTris.upload(tris, st) == GI_C_OK && dInstances.upload(instances, st) == GI_C_OK &&
        dPatch.upload(patch, st) == GI_C_OK && dShade.upload(shade, st) == GI_C_OK && dFlat.upload(flat, st) == GI_C_OK && dTrav.upload(instTrav, st) == GI_C_OK;
    if (ok) {
      launchPatchVisibility2(st, dTris.ptr, n, dInstances.ptr, instanceCount, dPatch.ptr, dShade.ptr, kPool, dFlat.ptr, n);
      launchPatchInstTrav(st, dTrav.ptr, instanceCount, dPatch.ptr);
      ok = hipGetLastError() == hipSuccess;
    }
    ok = ok && hipMemcpyAsync(devTris.data(), dTris.ptr, (size_t)n * sizeof(TriRec), hipMemcpyDeviceToHost, st) == hipSuccess &&
        hipMemcpyAsync(devFlat.data(), dFlat.ptr, (size_t)n * sizeof(uint32_t), hipMemcpyDeviceToHost, st) == hipSuccess &&
        hipMemcpyAsync(devTrav.data(), dTrav.ptr, (size_t)instanceCount * sizeof(InstTrav), hipMemcpyDeviceToHost, st) == hipSuccess;
    ok = hipStreamSynchronize(st) == hipSuccess && ok;
    dTris.release(); dInstances.release(); dPatch.release(); dShade.release(); dFlat.release(); dTrav.release();
    if (!ok) { setError("giCDebugPatchVisibilityTwoLevel: device error"); return -1; }
    // --- the host form, and the words that differ
    patchVisibilityTwoLevelHost(tris.data(), n, instances.data(), instanceCount, patch.data(), shade.data(), kPool, flat.data(), n);
    patchInstTravHost(instTrav.data(), instanceCount, patch.data());
    int differ = 0;
    for (uint32_t i = 0; i < n; i++) {
      differ += devTris[i].origId != tris[i].origId;
      differ += devFlat[i] != flat[i];
      for (int a = 0; a < 3; a++) differ += (memcmp(&devTris[i].e1[a], &tris[i].e1[a], 4) != 0) + (memcmp(&devTris[i].e2[a], &tris[i].e2[a], 4) != 0);
      TriRec a = devTris[i], b = tris[i]; // (every other word of the record stays)
      a.origId = b.origId = 0u; memset(a.e1, 0, 24); memset(b.e1, 0, 24);
      differ += memcmp(&a, &b, sizeof(TriRec)) != 0;
    }
    for (uint32_t i = 0; i < instanceCount; i++) {
      differ += devTrav[i].triBase != instTrav[i].triBase;
      InstTrav a = devTrav[i], b = instTrav[i]; a.triBase = b.triBase = 0u;
      differ += memcmp(&a, &b, sizeof(InstTrav)) != 0;
    }
    // --- the host form against a fresh numbering of the instances visible after the edit
    std::vector<uint8_t> seen(n, 0); uint32_t visible = 0;
    uint32_t bad = flatIdViolations(tris.data(), n, flat.data(), n, instTrav.data(), hiddenA.data(), instanceCount, seen.data(), visible);
    if (visible != after) bad++;
    for (uint32_t i = 0; i < n; i++) {
      const TriRec& t = tris[i];
      if (hiddenA[t.instance]) continue;
      TriRec w{}; refit_flatten(instances[t.instance].o2w, shade[t.vi[0]].p, w.v0, w.e1, w.e2);
      if (memcmp(w.v0, t.v0, 36) != 0) bad++; // (v0, e1, e2: the record is whole again)
    }
    if (outTris) *outTris = n;
    return differ + (int)bad;
  } catch (const std::exception& e) { setError(std::string("giCDebugPatchVisibilityTwoLevel: ") + e.what()); return -1; }
}

// giCDebugInstanceBounds: k_inst_bounds + k_inst_finish over one mesh under `xformCount` instance transforms against the host form of the same arithmetic
// (gi_tlas.h tlasInstanceBoundsHost), bytewise
extern "C" int giCDebugInstanceBounds(const GiCVertex* vertices, uint32_t vertexCount, const GiCFace* faces, uint32_t faceCount, const float* xforms16,
    uint32_t xformCount, float* outBoxes6, uint32_t* outStatus)
{
  if (!g_ctx.initialized) { setError("giCDebugInstanceBounds before giCInitialize"); return -1; }
  if ((vertexCount && !vertices) || (faceCount && !faces) || (xformCount && !xforms16) || faceCount >= (1u << 26)) { setError("giCDebugInstanceBounds: bad arguments"); return -1; }
  for (uint32_t f = 0; f < faceCount; f++) for (int k = 0; k < 3; k++) if (faces[f].v_i[k] >= vertexCount) { setError("giCDebugInstanceBounds: a face index outside the vertices"); return -1; }
  if (xformCount == 0u) return 0;
  try {
    std::vector<BlasTri> tris(faceCount);
    for (uint32_t f = 0; f < faceCount; f++) {
      BlasTri bt{};
      memcpy(bt.p0, vertices[faces[f].v_i[0]].pos, 12); memcpy(bt.p1, vertices[faces[f].v_i[1]].pos, 12); memcpy(bt.p2, vertices[faces[f].v_i[2]].pos, 12);
      bt.prim = f; tris[f] = bt;
    }
    GiCMesh m; m.scene = nullptr; m.id = 0;
    m.instanceTransforms.assign(xforms16, xforms16 + (size_t)xformCount * 16u);
    std::vector<InstBoundsJob> jobs(xformCount);
    for (uint32_t i = 0; i < xformCount; i++) {
      const InstanceRec ir = makeInstanceRec(&m, 0u, i);
      jobs[i] = InstBoundsJob{}; memcpy(jobs[i].o2w, ir.o2w, sizeof(ir.o2w)); jobs[i].firstTri = 0u; jobs[i].faceCount = faceCount; jobs[i].instance = i;
    }
    const uint32_t chunksPerJob = std::max(instBoundsChunks(faceCount), 1u);
    std::vector<uint32_t> result((size_t)xformCount * 7u, 0xa5a5a5a5u);
    DeviceBuffer<InstBoundsJob> dJobs; DeviceBuffer<BlasTri> dTris; DeviceBuffer<float> dPartials; DeviceBuffer<uint32_t> dOut;
    hipStream_t st = g_ctx.stream;
    bool ok = hipSetDevice(g_ctx.device) == hipSuccess && dJobs.upload(jobs, st) == GI_C_OK && dTris.upload(tris, st) == GI_C_OK &&
        dPartials.alloc((size_t)xformCount * chunksPerJob * 8u) == GI_C_OK && dOut.upload(result, st) == GI_C_OK;
    ok = ok && launchInstBounds(st, dJobs.ptr, xformCount, chunksPerJob, dTris.ptr, faceCount, dPartials.ptr, dOut.ptr) && hipGetLastError() == hipSuccess;
    ok = ok && hipMemcpyAsync(result.data(), dOut.ptr, result.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, st) == hipSuccess;
    ok = hipStreamSynchronize(st) == hipSuccess && ok;
    dJobs.release(); dTris.release(); dPartials.release(); dOut.release();
    if (!ok) { setError("giCDebugInstanceBounds: device error"); return -1; }
    int differ = 0;
    for (uint32_t i = 0; i < xformCount; i++) {
      float box[6];
      const uint32_t status = tlasInstanceBoundsHost(jobs[i].o2w, tris.data(), tris.size(), box);
      if (memcmp(box, &result[7u * (size_t)i], 24) != 0 || status != result[7u * (size_t)i + 6u]) differ++;
      if (outBoxes6) memcpy(outBoxes6 + 6u * (size_t)i, &result[7u * (size_t)i], 24);
      if (outStatus) outStatus[i] = result[7u * (size_t)i + 6u];
    }
    return differ;
  } catch (const std::exception& e) { setError(std::string("giCDebugInstanceBounds: ") + e.what()); return -1; }
}

// giCDebugSceneBlasCheck: the two-level arrays resident on a device after vertex updates in place, against the scene's current meshes (include/gi_c.h has
// the five parts).  The BLAS nodes are compared with the HOST form of the refit over the host's topology copy and the current points; the TLAS, its items
// and the InstTrav records with a fresh buildTwoLevel, whose instance boxes do not depend on a BLAS's shape.
extern "C" int giCDebugSceneBlasCheck(const GiCScene* scene, uint32_t deviceIndex, uint32_t* out)
{
  GiCScene* s = const_cast<GiCScene*>(scene);
  if (!g_ctx.initialized || !s || !out) { setError("giCDebugSceneBlasCheck: bad arguments"); return -1; }
  std::lock_guard<std::mutex> guard(s->mutex);
  if (!s->host) { setError("giCDebugSceneBlasCheck: the scene has not been built (render it once)"); return -1; }
  if (deviceIndex > s->replicas.size() || deviceIndex >= sceneDeviceCount(s)) { setError("giCDebugSceneBlasCheck: no such device copy"); return -1; }
  const SceneHost& H = *s->host; const TwoLevelHost& T = H.two;
  out[0] = s->twoLevel ? 1u : 0u; out[1] = out[2] = out[3] = 0u;
  if (!s->twoLevel) return 0;
  try {
    std::vector<InstanceRec> instances(H.instances.size());
    for (const MeshBuild& mb : H.meshBuilds) {
      if (mb.m->instanceTransforms.size() != (size_t)mb.instCount * 16u) { setError("giCDebugSceneBlasCheck: a mesh's instance count is not the built one (render first)"); return -1; }
      for (uint32_t ii = 0; ii < mb.instCount; ii++) instances[mb.inst[ii]] = makeInstanceRec(mb.m, mb.meshIdx, ii);
    }
    TwoLevelHost fresh;
    const int rc = buildTwoLevel(s, H.meshBuilds, instances, s->triCount, s->nodeCount, fresh);
    const bool stillTwoLevel = s->twoLevel;
    s->twoLevel = true; // (buildTwoLevel answers through it: the resident scene is what it was)
    if (rc != GI_C_OK || !stillTwoLevel) { setError("giCDebugSceneBlasCheck: a fresh build of the current meshes would not use the two-level layout"); return -1; }
    if (!freshTlasOfResidentBuilder(H, instances.size(), fresh)) { setError("giCDebugSceneBlasCheck: the host form of the device TLAS builder failed"); return -1; }
    if (T.meshBlasTri.size() != H.meshBuilds.size() || T.meshBlasNode.size() != H.meshBuilds.size() || T.meshBlasLevels.size() != H.meshBuilds.size() ||
        fresh.instTrav.size() != T.instTrav.size() || fresh.blasTris.size() != T.blasTris.size()) { setError("giCDebugSceneBlasCheck: the host copy is not the built scene's"); return -1; }
    SceneDevice& D = sceneDevice(s, deviceIndex);
    std::vector<Node8> tlasNodes(fresh.tlasNodes.size()), blasNodes(T.blasNodes.size()); std::vector<uint32_t> tlasItems(fresh.tlasItems.size());
    std::vector<BlasTri> blasTris(T.blasTris.size()); std::vector<InstTrav> instTrav(fresh.instTrav.size());
    int differ = 0;
    auto fetch = [&](auto& host, const auto& dev) -> bool { // (a resident array shorter than expected: every missing record differs)
      using R = typename std::remove_reference<decltype(host)>::type::value_type;
      const size_t n = std::min(host.size(), dev.ptr ? dev.count : (size_t)0);
      differ += (int)(host.size() - n);
      host.resize(n);
      return n == 0u || hipMemcpy(host.data(), dev.ptr, n * sizeof(R), hipMemcpyDeviceToHost) == hipSuccess;
    };
    bool ok = hipSetDevice(g_ctx.devs[D.slot].device) == hipSuccess;
    ok = ok && fetch(tlasNodes, D.dTlasNodes) && fetch(tlasItems, D.dTlasItems) && fetch(instTrav, D.dInstTrav) && fetch(blasNodes, D.dBlasNodes) && fetch(blasTris, D.dBlasTris);
    (void)hipSetDevice(g_ctx.device);
    if (!ok) { setError("giCDebugSceneBlasCheck: download failed"); return -1; }
    if (blasNodes.size() != T.blasNodes.size() || blasTris.size() != T.blasTris.size()) return differ; // (nothing further can be compared)
    // (a) the records: the build's prim at its place, the current corners; and the expected arrays of (b)
    std::vector<BlasTri> wantTris(T.blasTris); std::vector<Node8> wantNodes(T.blasNodes);
    std::vector<float> boxes(8u * wantNodes.size(), 0.0f), under(6u * wantNodes.size(), 0.0f);
    uint32_t violations = 0;
    const RetiredRanges ignored = retiredRangesOf(H, T, T.blasNodes.size(), T.blasTris.size());
    for (const MeshBuild& mb : H.meshBuilds) {
      if (mb.instCount == 0u || mb.m->retired) continue; // (a retired mesh -- updateTopologyTwoLevel -- is hidden for good: its ranges are ignored)
      const GiCMesh* m = mb.m;
      const uint32_t first = T.meshBlasTri[mb.meshIdx], nodeBase = T.meshBlasNode[mb.meshIdx], nf = (uint32_t)m->faces.size();
      const std::vector<uint32_t>& lv = T.meshBlasLevels[mb.meshIdx];
      if ((size_t)first + nf > wantTris.size() || lv.size() < 2u || (size_t)nodeBase + lv.back() > wantNodes.size()) { differ++; continue; }
      for (uint32_t i = 0; i < nf; i++) {
        const uint32_t prim = T.blasTris[first + i].prim;
        if (prim >= nf) { differ++; continue; }
        wantTris[first + i] = makeBlasTri(m->vertices.data(), m->faces.data(), prim);
        if (memcmp(&blasTris[first + i], &wantTris[first + i], sizeof(BlasTri)) != 0) differ++;
      }
      // (b) the host form of the refit over the host's topology copy; (c) the conservative check of what is resident
      blasRefitHost(wantNodes.data(), (uint32_t)wantNodes.size(), nodeBase, lv.back(), boxes.data(), wantTris.data(), (uint32_t)wantTris.size());
      for (uint32_t i = 0; i < lv.back(); i++) if (memcmp(&blasNodes[nodeBase + i], &wantNodes[nodeBase + i], sizeof(Node8)) != 0) differ++;
      std::vector<uint8_t> seen(nf, 0);
      violations += blasConservativeViolations(blasNodes.data(), (uint32_t)blasNodes.size(), nodeBase, lv.back(), blasTris.data(), (uint32_t)blasTris.size(), first, nf,
          under.data(), seen.data());
      // (e) the fresh records with the resident BLAS's root
      for (uint32_t ii = 0; ii < mb.instCount; ii++) if (mb.inst[ii] < fresh.instTrav.size()) fresh.instTrav[mb.inst[ii]].blasRoot = nodeBase;
    }
    // (d), (e)
    if (T.tlasNodes.size() != fresh.tlasNodes.size()) differ++; // (the host copy the next update starts from)
    const std::vector<uint8_t> none;
    auto compare = [&](const auto& got, const auto& want, const std::vector<uint8_t>& skip) {
      using R = typename std::remove_reference<decltype(got)>::type::value_type;
      for (size_t i = 0; i < got.size(); i++) if (!(i < skip.size() && skip[i]) && memcmp(&got[i], &want[i], sizeof(R)) != 0) differ++;
    };
    compare(tlasNodes, fresh.tlasNodes, none); compare(tlasItems, fresh.tlasItems, none); compare(instTrav, fresh.instTrav, ignored.inst);
    for (size_t i = 0; i < instTrav.size(); i++) // (the host copy)
      if (!(i < ignored.inst.size() && ignored.inst[i]) && memcmp(&T.instTrav[i], &fresh.instTrav[i], sizeof(InstTrav)) != 0) differ++;
    out[1] = (uint32_t)blasNodes.size(); out[2] = violations; out[3] = (uint32_t)blasTris.size();
    return differ + (int)violations;
  } catch (const std::exception& e) { s->twoLevel = true; setError(std::string("giCDebugSceneBlasCheck: ") + e.what()); return -1; }
}

// giCDebugBlasRefit / giCDebugBlasRefitHost: one BLAS built over points a, refitted to points b by the host form (gi_blas.h) and -- onDevice -- by k_blas_tris +
// k_blas_refit_level, compared bytewise
static int debugBlasRefit(const char* name, bool onDevice, const GiCVertex* a, const GiCVertex* b, uint32_t vertexCount, const GiCFace* faces, uint32_t faceCount,
    uint32_t* outNodes, uint32_t* outViolations)
{
  if (onDevice && !g_ctx.initialized) { setError(std::string(name) + " before giCInitialize"); return -1; }
  if (!a || !b || !faces || vertexCount == 0u || faceCount == 0u || faceCount >= (1u << 26)) { setError(std::string(name) + ": bad arguments"); return -1; }
  for (uint32_t f = 0; f < faceCount; f++) for (int k = 0; k < 3; k++) if (faces[f].v_i[k] >= vertexCount) { setError(std::string(name) + ": a face index outside the vertices"); return -1; }
  try {
    bool same = true;
    for (uint32_t i = 0; i < vertexCount && same; i++) same = memcmp(a[i].pos, b[i].pos, 12) == 0;
    Bvh8 built; std::vector<uint32_t> order; float mlo[3], mhi[3];
    buildMeshBlas(a, faces, faceCount, built, order, mlo, mhi);
    std::vector<BlasTri> builtTris; builtTris.reserve(faceCount);
    for (uint32_t f : order) builtTris.push_back(makeBlasTri(a, faces, f));
    const uint32_t nodeCount = (uint32_t)built.nodes.size();
    if (builtTris.size() != faceCount || built.levelStart.size() < 2u || built.levelStart.back() != nodeCount) { setError(std::string(name) + ": the builder's tree has no level table"); return -1; }
    std::vector<TriShade> shade(faceCount); // (the corners alone: what the refit reads of a shading record)
    for (uint32_t f = 0; f < faceCount; f++) { TriShade q{}; for (int k = 0; k < 3; k++) memcpy(q.p[k], b[faces[f].v_i[k]].pos, 12); shade[f] = q; }
    // --- the host form
    std::vector<Node8> hostNodes(built.nodes); std::vector<BlasTri> hostTris(builtTris); std::vector<float> boxes(8u * (size_t)nodeCount, 0.0f);
    int differ = 0;
    for (uint32_t i = 0; i < faceCount; i++) if (!blas_tri_from_shade(hostTris[i], shade.data(), faceCount, 0u, faceCount)) differ += (int)sizeof(BlasTri);
    blasRefitHost(hostNodes.data(), nodeCount, 0u, nodeCount, boxes.data(), hostTris.data(), faceCount);
    std::vector<Node8> nodes(hostNodes); std::vector<BlasTri> tris(hostTris); // what is checked below: the host's result, or the device's
    if (onDevice) {
      std::vector<RefitUnit> units{RefitUnit{0u, &built.levelStart}};
      std::vector<RefitRange> ranges; std::vector<RefitLevel> levels;
      if (!planRefitLevels(units, nodeCount, ranges, levels)) { setError(std::string(name) + ": the level table lies outside the tree"); return -1; }
      DeviceBuffer<Node8> dNodes; DeviceBuffer<BlasTri> dTris; DeviceBuffer<TriShade> dShade; DeviceBuffer<float> dBoxes; DeviceBuffer<RefitRange> dRanges;
      hipStream_t st = g_ctx.stream;
      bool ok = hipSetDevice(g_ctx.device) == hipSuccess && dNodes.upload(built.nodes, st) == GI_C_OK && dTris.upload(builtTris, st) == GI_C_OK &&
          dShade.upload(shade, st) == GI_C_OK && dBoxes.alloc(8u * (size_t)nodeCount) == GI_C_OK && dRanges.upload(ranges, st) == GI_C_OK;
      ok = ok && launchBlasTris(st, dTris.ptr, faceCount, 0u, faceCount, dShade.ptr, faceCount, 0u);
      if (ok) for (const RefitLevel& lv : levels) launchBlasRefitLevel(st, dNodes.ptr, nodeCount, dBoxes.ptr, dRanges.ptr + lv.first, lv.ranges, lv.threads, dTris.ptr, faceCount);
      ok = ok && hipGetLastError() == hipSuccess;
      ok = ok && hipMemcpyAsync(nodes.data(), dNodes.ptr, nodes.size() * sizeof(Node8), hipMemcpyDeviceToHost, st) == hipSuccess &&
          hipMemcpyAsync(tris.data(), dTris.ptr, tris.size() * sizeof(BlasTri), hipMemcpyDeviceToHost, st) == hipSuccess;
      ok = hipStreamSynchronize(st) == hipSuccess && ok;
      dNodes.release(); dTris.release(); dShade.release(); dBoxes.release(); dRanges.release();
      if (!ok) { setError(std::string(name) + ": device error"); return -1; }
    }
    auto bytesDiffering = [](const void* x, const void* y, size_t n) { int d = 0; for (size_t i = 0; i < n; i++) d += ((const uint8_t*)x)[i] != ((const uint8_t*)y)[i]; return d; };
    if (onDevice) differ += bytesDiffering(nodes.data(), hostNodes.data(), nodes.size() * sizeof(Node8)) + bytesDiffering(tris.data(), hostTris.data(), tris.size() * sizeof(BlasTri));
    if (same) differ += bytesDiffering(nodes.data(), built.nodes.data(), nodes.size() * sizeof(Node8)) + bytesDiffering(tris.data(), builtTris.data(), tris.size() * sizeof(BlasTri));
    else { // the topology is the build's
      for (uint32_t i = 0; i < nodeCount; i++) {
        const Node8& x = nodes[i]; const Node8& y = built.nodes[i];
        differ += (x.imask != y.imask) + bytesDiffering(x.meta, y.meta, 8) + bytesDiffering(&x.childBase, &y.childBase, 4) + bytesDiffering(&x.triBase, &y.triBase, 4);
      }
      for (uint32_t i = 0; i < faceCount; i++) differ += bytesDiffering(&tris[i].prim, &builtTris[i].prim, 4);
    }
    std::vector<float> under(6u * (size_t)nodeCount, 0.0f); std::vector<uint8_t> seen(faceCount, 0);
    const uint32_t violations = blasConservativeViolations(nodes.data(), nodeCount, 0u, nodeCount, tris.data(), faceCount, 0u, faceCount, under.data(), seen.data());
    if (outNodes) *outNodes = nodeCount;
    if (outViolations) *outViolations = violations;
    return differ;
  } catch (const std::exception& e) { setError(std::string(name) + ": " + e.what()); return -1; }
}
extern "C" int giCDebugBlasRefit(const GiCVertex* a, const GiCVertex* b, uint32_t vertexCount, const GiCFace* faces, uint32_t faceCount, uint32_t* outNodes,
    uint32_t* outViolations)
{ return debugBlasRefit("giCDebugBlasRefit", true, a, b, vertexCount, faces, faceCount, outNodes, outViolations); }
extern "C" int giCDebugBlasRefitHost(const GiCVertex* a, const GiCVertex* b, uint32_t vertexCount, const GiCFace* faces, uint32_t faceCount, uint32_t* outNodes,
    uint32_t* outViolations)
{ return debugBlasRefit("giCDebugBlasRefitHost", false, a, b, vertexCount, faces, faceCount, outNodes, outViolations); }

// giCDebugAppendRecords / giCDebugAppendRecordsHost: one mesh appended behind `vertexOffset` vertex records, `shadeBase` shading records, a few BLAS and flat
// records and the scene-order id `idBase` -- its shading records, BLAS records, flat records, face-id words and id-table words made by the host forms of
// gi_append.h and, onDevice, by k_append_shade_index + k_gather_shade + k_append_blas_tris + k_append_records on scratch arrays, against the scene build's own
// code (packTriShade, makeBlasTri in buildMeshBlas's order, flattenInstance as buildSceneTreeless leaves its records, faceIdAovOf, flatOfOrig[id] = position).
// Every array starts as 0xa5 bytes on both sides: a store outside the mesh's ranges is seen.  Returns the bytes that differ
static int debugAppendRecords(const char* name, bool onDevice, const GiCVertex* vertices, uint32_t vertexCount, const GiCFace* faces, uint32_t faceCount,
    const int32_t* faceIds, uint32_t maxFaceId, uint32_t flags, const float* xforms16, uint32_t xformCount, uint32_t vertexOffset, uint32_t shadeBase, uint32_t idBase,
    uint32_t matFlags)
{
  if (onDevice && !g_ctx.initialized) { setError(std::string(name) + " before giCInitialize"); return -1; }
  if (!vertices || !faces || !xforms16 || vertexCount == 0u || faceCount == 0u || xformCount == 0u || (uint64_t)faceCount * xformCount >= (1ull << 24) ||
      vertexOffset >= (1u << 20) || shadeBase >= (1u << 20) || idBase >= (1u << 24)) { setError(std::string(name) + ": bad arguments"); return -1; }
  for (uint32_t f = 0; f < faceCount; f++) for (int k = 0; k < 3; k++) if (faces[f].v_i[k] >= vertexCount) { setError(std::string(name) + ": a face index outside the vertices"); return -1; }
  try {
    GiCMesh m; m.scene = nullptr; m.id = 11; m.flipFacing = (flags & 1u) != 0u; m.doubleSided = (flags & 2u) != 0u; m.maxFaceId = maxFaceId;
    m.vertices.assign(vertices, vertices + vertexCount); m.faces.assign(faces, faces + faceCount);
    if (faceIds) m.faceIds.assign(faceIds, faceIds + faceCount);
    m.instanceTransforms.assign(xforms16, xforms16 + (size_t)xformCount * 16u);
    constexpr uint32_t meshIdx = 2u, instFirst = 5u, triFirst = 7u, blasFirst = 3u; // (as a mesh behind others in every array)
    const uint32_t items = faceCount * xformCount, triCount = triFirst + items, instanceCount = instFirst + xformCount, shadeCount = shadeBase + faceCount;
    const uint32_t vertCount = vertexOffset + vertexCount, blasCount = blasFirst + faceCount, flatCount = idBase + items;
    std::vector<InstanceRec> instances(instanceCount, InstanceRec{});
    for (uint32_t i = 0; i < xformCount; i++) { instances[instFirst + i] = makeInstanceRec(&m, meshIdx, i);
        if (!usableInstance(instances[instFirst + i])) { setError(std::string(name) + ": an instance transform is not usable"); return -1; } }
    std::vector<FVertex> verts(vertCount, FVertex{});
    for (uint32_t i = 0; i < vertexCount; i++) verts[vertexOffset + i] = packVertex(vertices[i]);
    std::vector<uint32_t> faces3(3u * (size_t)faceCount);
    for (uint32_t f = 0; f < faceCount; f++) for (int k = 0; k < 3; k++) faces3[3u * (size_t)f + k] = faces[f].v_i[k];
    Bvh8 blas; std::vector<uint32_t> order; float mlo[3], mhi[3];
    buildMeshBlas(vertices, faces, faceCount, blas, order, mlo, mhi);
    if (order.size() != faceCount) { setError(std::string(name) + ": the builder left faces out (an unusable position)"); return -1; }
    const std::vector<int32_t> faceIdAov = faceIdAovOf(&m);
    // --- the scene build's forms over arrays of 0xa5 bytes
    auto filled = [](auto& v, size_t n) { v.resize(n); if (n) memset(static_cast<void*>(v.data()), 0xa5, n * sizeof(v[0])); };
    std::vector<TriShade> wantShade, gotShade; std::vector<BlasTri> wantBlas, gotBlas; std::vector<TriRec> wantTris, gotTris; std::vector<int32_t> wantFaceId, gotFaceId;
    std::vector<uint32_t> wantFlat, gotFlat;
    filled(wantShade, shadeCount); filled(gotShade, shadeCount); filled(wantBlas, blasCount); filled(gotBlas, blasCount); filled(wantTris, triCount); filled(gotTris, triCount);
    filled(wantFaceId, triCount); filled(gotFaceId, triCount); filled(wantFlat, flatCount); filled(gotFlat, flatCount);
    for (uint32_t f = 0; f < faceCount; f++) wantShade[shadeBase + f] = packTriShade(vertices, faces[f], vertexOffset);
    for (uint32_t i = 0; i < faceCount; i++) wantBlas[blasFirst + i] = makeBlasTri(vertices, faces, order[i]);
    for (uint32_t i = 0; i < xformCount; i++) {
      const uint32_t at = triFirst + i * faceCount, base = idBase + i * faceCount;
      flattenInstance(instances[instFirst + i], instFirst + i, &m, vertexOffset, matFlags, base, shadeBase, &wantTris[at]);
      for (uint32_t f = 0; f < faceCount; f++) { wantFaceId[at + f] = faceIdAov[f]; wantFlat[base + f] = at + f; }
    }
    AppendMesh M{}; M.triFirst = triFirst; M.faceCount = faceCount; M.instFirst = instFirst; M.instCount = xformCount; M.shadeBase = shadeBase; M.idBase = idBase;
    M.matFlags = matFlags; M.triCount = triCount; M.instanceCount = instanceCount; M.shadeCount = shadeCount; M.flatCount = flatCount;
    if (!appendMeshRangesOk(M)) { setError(std::string(name) + ": internal: ranges"); return -1; }
    if (!onDevice) {
      appendShadeIndexHost(gotShade.data(), shadeCount, shadeBase, faces3.data(), faceCount, vertexOffset);
      for (uint32_t f = 0; f < faceCount; f++) refit_gather_shade(verts.data(), vertCount, gotShade[shadeBase + f]);
      appendBlasTrisHost(gotBlas.data(), blasCount, blasFirst, order.data(), faceCount, gotShade.data(), shadeCount, shadeBase);
      appendRecordsHost(M, 0u, items, gotTris.data(), gotFaceId.data(), gotFlat.data(), instances.data(), gotShade.data(), faceIdAov.data());
    } else {
      DeviceBuffer<TriShade> dShade; DeviceBuffer<BlasTri> dBlas; DeviceBuffer<TriRec> dTris; DeviceBuffer<int32_t> dFaceId, dFaceIdOfFace; DeviceBuffer<uint32_t> dFlat, dFaces, dOrder;
      DeviceBuffer<InstanceRec> dInstances; DeviceBuffer<FVertex> dVerts;
      hipStream_t st = g_ctx.stream;
      bool ok = hipSetDevice(g_ctx.device) == hipSuccess && dShade.upload(gotShade, st) == GI_C_OK && dBlas.upload(gotBlas, st) == GI_C_OK && dTris.upload(gotTris, st) == GI_C_OK &&
          dFaceId.upload(gotFaceId, st) == GI_C_OK && dFlat.upload(gotFlat, st) == GI_C_OK && dFaces.upload(faces3, st) == GI_C_OK && dOrder.upload(order, st) == GI_C_OK &&
          dFaceIdOfFace.upload(faceIdAov, st) == GI_C_OK && dInstances.upload(instances, st) == GI_C_OK && dVerts.upload(verts, st) == GI_C_OK;
      ok = ok && launchAppendShadeIndex(st, dShade.ptr, shadeCount, shadeBase, dFaces.ptr, faceCount, vertexOffset) &&
          launchGatherShade(st, dShade.ptr, shadeCount, shadeBase, faceCount, dVerts.ptr, vertCount) &&
          launchAppendBlasTris(st, dBlas.ptr, blasCount, blasFirst, dOrder.ptr, faceCount, dShade.ptr, shadeCount, shadeBase) &&
          launchAppendRecords(st, M, dTris.ptr, dFaceId.ptr, dFlat.ptr, dInstances.ptr, dShade.ptr, dFaceIdOfFace.ptr);
      ok = ok && hipGetLastError() == hipSuccess;
      ok = ok && hipMemcpyAsync(gotShade.data(), dShade.ptr, gotShade.size() * sizeof(TriShade), hipMemcpyDeviceToHost, st) == hipSuccess &&
          hipMemcpyAsync(gotBlas.data(), dBlas.ptr, gotBlas.size() * sizeof(BlasTri), hipMemcpyDeviceToHost, st) == hipSuccess &&
          hipMemcpyAsync(gotTris.data(), dTris.ptr, gotTris.size() * sizeof(TriRec), hipMemcpyDeviceToHost, st) == hipSuccess &&
          hipMemcpyAsync(gotFaceId.data(), dFaceId.ptr, gotFaceId.size() * sizeof(int32_t), hipMemcpyDeviceToHost, st) == hipSuccess &&
          hipMemcpyAsync(gotFlat.data(), dFlat.ptr, gotFlat.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, st) == hipSuccess;
      ok = hipStreamSynchronize(st) == hipSuccess && ok;
      dShade.release(); dBlas.release(); dTris.release(); dFaceId.release(); dFaceIdOfFace.release(); dFlat.release(); dFaces.release(); dOrder.release();
      dInstances.release(); dVerts.release();
      if (!ok) { setError(std::string(name) + ": device error"); return -1; }
    }
    auto bytesDiffering = [](const void* x, const void* y, size_t n) { int d = 0; for (size_t i = 0; i < n; i++) d += ((const uint8_t*)x)[i] != ((const uint8_t*)y)[i]; return d; };
    return bytesDiffering(gotShade.data(), wantShade.data(), gotShade.size() * sizeof(TriShade)) + bytesDiffering(gotBlas.data(), wantBlas.data(), gotBlas.size() * sizeof(BlasTri)) +
        bytesDiffering(gotTris.data(), wantTris.data(), gotTris.size() * sizeof(TriRec)) + bytesDiffering(gotFaceId.data(), wantFaceId.data(), gotFaceId.size() * sizeof(int32_t)) +
        bytesDiffering(gotFlat.data(), wantFlat.data(), gotFlat.size() * sizeof(uint32_t));
  } catch (const std::exception& e) { setError(std::string(name) + ": " + e.what()); return -1; }
}
extern "C" int giCDebugAppendRecords(const GiCVertex* vertices, uint32_t vertexCount, const GiCFace* faces, uint32_t faceCount, const int32_t* faceIds, uint32_t maxFaceId,
    uint32_t flags, const float* xforms16, uint32_t xformCount, uint32_t vertexOffset, uint32_t shadeBase, uint32_t idBase, uint32_t matFlags)
{ return debugAppendRecords("giCDebugAppendRecords", true, vertices, vertexCount, faces, faceCount, faceIds, maxFaceId, flags, xforms16, xformCount, vertexOffset, shadeBase, idBase, matFlags); }
extern "C" int giCDebugAppendRecordsHost(const GiCVertex* vertices, uint32_t vertexCount, const GiCFace* faces, uint32_t faceCount, const int32_t* faceIds, uint32_t maxFaceId,
    uint32_t flags, const float* xforms16, uint32_t xformCount, uint32_t vertexOffset, uint32_t shadeBase, uint32_t idBase, uint32_t matFlags)
{ return debugAppendRecords("giCDebugAppendRecordsHost", false, vertices, vertexCount, faces, faceCount, faceIds, maxFaceId, flags, xforms16, xformCount, vertexOffset, shadeBase, idBase, matFlags); }

// giCDebugInstanceRecords / giCDebugInstanceRecordsHost: new instances of several meshes at arbitrary storage slots -- their flat records, face-id words and
// id-table words made by k_instance_records in ONE launch (onDevice) or by its host form (gi_instances.h) on scratch arrays, against the scene build's own
// code (flattenInstance as buildSceneTreeless leaves its records, faceIdAovOf, flatOfOrig[id] = position).  Every array starts as 0xa5 bytes on both sides: a
// store outside the jobs' ranges is seen.  Returns the bytes that differ
static int debugInstanceRecords(const char* name, bool onDevice, const GiCDebugInstanceMesh* meshes, uint32_t meshCount, const GiCDebugInstanceJob* jobsIn, uint32_t jobCount)
{
  if (onDevice && !g_ctx.initialized) { setError(std::string(name) + " before giCInitialize"); return -1; }
  if (!meshes || !jobsIn || meshCount == 0u || jobCount == 0u || meshCount > (1u << 16) || jobCount > (1u << 20)) { setError(std::string(name) + ": bad arguments"); return -1; }
  uint64_t faceTotal = 0;
  for (uint32_t k = 0; k < meshCount; k++) {
    const GiCDebugInstanceMesh& dm = meshes[k];
    if (!dm.vertices || !dm.faces || dm.vertexCount == 0u || dm.faceCount == 0u || dm.faceCount >= (1u << 22) || dm.vertexCount >= (1u << 24)) { setError(std::string(name) + ": bad arguments"); return -1; }
    for (uint32_t f = 0; f < dm.faceCount; f++) for (int c = 0; c < 3; c++) if (dm.faces[f].v_i[c] >= dm.vertexCount) { setError(std::string(name) + ": a face index outside the vertices"); return -1; }
    faceTotal += dm.faceCount;
  }
  if (faceTotal >= (1u << 24)) { setError(std::string(name) + ": bad arguments"); return -1; }
  try {
    // --- the meshes, one behind the other in the per-face arrays, as meshes behind others in every array
    struct Mesh { GiCMesh m; uint32_t vertexOffset, shadeBase, faceIdFirst, matFlags; std::vector<int32_t> faceIdAov; };
    std::vector<Mesh> built(meshCount);
    uint32_t vertexOffset = 3u, shadeCount = 5u, faceIdCount = 2u;
    for (uint32_t k = 0; k < meshCount; k++) {
      const GiCDebugInstanceMesh& dm = meshes[k];
      Mesh& B = built[k];
      B.m.scene = nullptr; B.m.id = 11 + (int32_t)k; B.m.flipFacing = (dm.flags & 1u) != 0u; B.m.doubleSided = (dm.flags & 2u) != 0u; B.m.maxFaceId = dm.maxFaceId;
      B.m.vertices.assign(dm.vertices, dm.vertices + dm.vertexCount); B.m.faces.assign(dm.faces, dm.faces + dm.faceCount);
      if (dm.faceIds) B.m.faceIds.assign(dm.faceIds, dm.faceIds + dm.faceCount);
      B.vertexOffset = vertexOffset; B.shadeBase = shadeCount; B.faceIdFirst = faceIdCount; B.matFlags = (6u + k) | ((dm.flags & 3u) << 30);
      B.faceIdAov = faceIdAovOf(&B.m);
      vertexOffset += dm.vertexCount; shadeCount += dm.faceCount; faceIdCount += dm.faceCount;
    }
    // --- the jobs: ranges inside sane sizes, usable transforms, no slot named twice and no two ranges overlapping
    uint32_t triCount = 0, flatCount = 0, instanceCount = 0;
    for (uint32_t k = 0; k < jobCount; k++) {
      const GiCDebugInstanceJob& dj = jobsIn[k];
      if (dj.mesh >= meshCount || dj.instanceSlot >= (1u << 20) || dj.recordSlot >= (1u << 24) || dj.idBase >= (1u << 24)) { setError(std::string(name) + ": bad arguments"); return -1; }
      const uint32_t nf = meshes[dj.mesh].faceCount;
      triCount = std::max(triCount, dj.recordSlot + nf); flatCount = std::max(flatCount, dj.idBase + nf); instanceCount = std::max(instanceCount, dj.instanceSlot + 1u);
    }
    triCount += 5u; flatCount += 3u; instanceCount += 2u; // (untouched words behind the last range)
    {
      std::vector<uint8_t> recUsed(triCount, 0), idUsed(flatCount, 0), instUsed(instanceCount, 0);
      for (uint32_t k = 0; k < jobCount; k++) {
        const GiCDebugInstanceJob& dj = jobsIn[k];
        const uint32_t nf = meshes[dj.mesh].faceCount;
        bool overlap = instUsed[dj.instanceSlot] != 0; instUsed[dj.instanceSlot] = 1;
        for (uint32_t f = 0; f < nf; f++) { overlap = overlap || recUsed[dj.recordSlot + f] || idUsed[dj.idBase + f]; recUsed[dj.recordSlot + f] = 1; idUsed[dj.idBase + f] = 1; }
        if (overlap) { setError(std::string(name) + ": overlapping slots"); return -1; }
      }
    }
    std::vector<InstanceRec> instances(instanceCount, InstanceRec{});
    std::vector<InstanceJob> jobs(jobCount);
    for (uint32_t k = 0; k < jobCount; k++) {
      const GiCDebugInstanceJob& dj = jobsIn[k];
      Mesh& B = built[dj.mesh];
      B.m.instanceTransforms.assign(dj.transform, dj.transform + 16);
      instances[dj.instanceSlot] = makeInstanceRec(&B.m, dj.mesh, 0);
      instances[dj.instanceSlot].instanceId = (int32_t)k;
      if (!usableInstance(instances[dj.instanceSlot])) { setError(std::string(name) + ": an instance transform is not usable"); return -1; }
      InstanceJob& j = jobs[k];
      j.instance = dj.instanceSlot; j.triFirst = dj.recordSlot; j.idBase = dj.idBase; j.shadeBase = B.shadeBase; j.faceCount = meshes[dj.mesh].faceCount; j.matFlags = B.matFlags;
      j.faceIdFirst = B.faceIdFirst; j.wgFirst = 0u;
    }
    InstanceJobSizes Z{}; Z.jobCount = jobCount; Z.triCount = triCount; Z.instanceCount = instanceCount; Z.shadeCount = shadeCount; Z.flatCount = flatCount;
    Z.faceIdCount = faceIdCount; Z.wgCount = instanceJobsNumber(jobs.data(), jobCount);
    if (Z.wgCount == 0u || !instanceJobsOk(jobs.data(), Z)) { setError(std::string(name) + ": internal: ranges"); return -1; }
    // --- the scene build's forms over arrays of 0xa5 bytes
    auto filled = [](auto& v, size_t n) { v.resize(n); if (n) memset(static_cast<void*>(v.data()), 0xa5, n * sizeof(v[0])); };
    std::vector<TriShade> shade(shadeCount, TriShade{}); std::vector<int32_t> faceIdTable(faceIdCount, 0);
    for (const Mesh& B : built) for (uint32_t f = 0; f < (uint32_t)B.m.faces.size(); f++) {
      shade[B.shadeBase + f] = packTriShade(B.m.vertices.data(), B.m.faces[f], B.vertexOffset); faceIdTable[B.faceIdFirst + f] = B.faceIdAov[f]; }
    std::vector<TriRec> wantTris, gotTris; std::vector<int32_t> wantFaceId, gotFaceId; std::vector<uint32_t> wantFlat, gotFlat;
    filled(wantTris, triCount); filled(gotTris, triCount); filled(wantFaceId, triCount); filled(gotFaceId, triCount); filled(wantFlat, flatCount); filled(gotFlat, flatCount);
    for (uint32_t k = 0; k < jobCount; k++) {
      const InstanceJob& j = jobs[k];
      const Mesh& B = built[jobsIn[k].mesh];
      flattenInstance(instances[j.instance], j.instance, &B.m, B.vertexOffset, B.matFlags, j.idBase, B.shadeBase, &wantTris[j.triFirst]);
      for (uint32_t f = 0; f < j.faceCount; f++) { wantFaceId[j.triFirst + f] = B.faceIdAov[f]; wantFlat[j.idBase + f] = j.triFirst + f; }
    }
    if (!onDevice) {
      instanceRecordsHost(jobs.data(), Z, 0u, Z.wgCount, gotTris.data(), gotFaceId.data(), gotFlat.data(), instances.data(), shade.data(), faceIdTable.data());
    } else {
      DeviceBuffer<TriShade> dShade; DeviceBuffer<TriRec> dTris; DeviceBuffer<int32_t> dFaceId, dFaceIdTable; DeviceBuffer<uint32_t> dFlat; DeviceBuffer<InstanceRec> dInstances;
      DeviceBuffer<InstanceJob> dJobs;
      hipStream_t st = g_ctx.stream;
      bool ok = hipSetDevice(g_ctx.device) == hipSuccess && dShade.upload(shade, st) == GI_C_OK && dTris.upload(gotTris, st) == GI_C_OK && dFaceId.upload(gotFaceId, st) == GI_C_OK &&
          dFlat.upload(gotFlat, st) == GI_C_OK && dFaceIdTable.upload(faceIdTable, st) == GI_C_OK && dInstances.upload(instances, st) == GI_C_OK && dJobs.upload(jobs, st) == GI_C_OK;
      ok = ok && launchInstanceRecords(st, jobs.data(), dJobs.ptr, Z, dTris.ptr, dFaceId.ptr, dFlat.ptr, dInstances.ptr, dShade.ptr, dFaceIdTable.ptr);
      ok = ok && hipGetLastError() == hipSuccess;
      ok = ok && hipMemcpyAsync(gotTris.data(), dTris.ptr, gotTris.size() * sizeof(TriRec), hipMemcpyDeviceToHost, st) == hipSuccess &&
          hipMemcpyAsync(gotFaceId.data(), dFaceId.ptr, gotFaceId.size() * sizeof(int32_t), hipMemcpyDeviceToHost, st) == hipSuccess &&
          hipMemcpyAsync(gotFlat.data(), dFlat.ptr, gotFlat.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, st) == hipSuccess;
      ok = hipStreamSynchronize(st) == hipSuccess && ok;
      dShade.release(); dTris.release(); dFaceId.release(); dFaceIdTable.release(); dFlat.release(); dInstances.release(); dJobs.release();
      if (!ok) { setError(std::string(name) + ": device error"); return -1; }
    }
    auto bytesDiffering = [](const void* x, const void* y, size_t n) { int d = 0; for (size_t i = 0; i < n; i++) d += ((const uint8_t*)x)[i] != ((const uint8_t*)y)[i]; return d; };
    return bytesDiffering(gotTris.data(), wantTris.data(), gotTris.size() * sizeof(TriRec)) + bytesDiffering(gotFaceId.data(), wantFaceId.data(), gotFaceId.size() * sizeof(int32_t)) +
        bytesDiffering(gotFlat.data(), wantFlat.data(), gotFlat.size() * sizeof(uint32_t));
  } catch (const std::exception& e) { setError(std::string(name) + ": " + e.what()); return -1; }
}
extern "C" int giCDebugInstanceRecords(const GiCDebugInstanceMesh* meshes, uint32_t meshCount, const GiCDebugInstanceJob* jobs, uint32_t jobCount)
{ return debugInstanceRecords("giCDebugInstanceRecords", true, meshes, meshCount, jobs, jobCount); }
extern "C" int giCDebugInstanceRecordsHost(const GiCDebugInstanceMesh* meshes, uint32_t meshCount, const GiCDebugInstanceJob* jobs, uint32_t jobCount)
{ return debugInstanceRecords("giCDebugInstanceRecordsHost", false, meshes, meshCount, jobs, jobCount); }

// brings the device scene up to date with the host-side edits: incremental for DIRTY_BVH raised by vertex edits alone (opt-in: the tree refitted on the
// device), by visibility toggles alone (opt-in: ids renumbered, the
// toggled meshes' triangles hidden / shown in place), for material-side edits alone (the small arrays + one word per triangle) and for transform edits alone
// (those instances re-transformed / re-braided) -- all four may be due, and run in this order -- else a full build
int syncSceneGeometry(GiCScene* s)
{
  UpdateCost spent; bool updated = false; // what the updates that ran spent: all of them go into the statistics
  // One update path: it runs when `due`, and either handles the edit (its dirty bits are cleared, it is counted), declines (not an error) or fails.  The paths
  // differ in the dirty bits: a visibility update is due BECAUSE a rebuild is asked for, so it clears DIRTY_BVH and a decline has nothing to raise; a material
  // or transform update that declines raises DIRTY_BVH (and rebuildDue) to get the full build below; DIRTY_XFORM is cleared at the end for every path.  An
  // error leaves half-updated arrays: the next render rebuilds (rebuildDue; after a material update DIRTY_BVH as well, its own bit would try the update again).
  auto run = [&](bool due, int (*update)(GiCScene*, bool&, UpdateCost&), uint32_t counter, uint32_t handledClears, uint32_t declineRaises, uint32_t errorRaises) -> int {
    if (!due) return GI_C_OK;
    bool handled = false; UpdateCost cost; s->generation++;
    if (update(s, handled, cost) != GI_C_OK) { s->dirty |= errorRaises; s->rebuildDue = true; return GI_C_ERROR; }
    if (handled) { s->dirty &= ~handledClears; s->updateCounts[counter]++; spent.buildMs += cost.buildMs; spent.uploadMs += cost.uploadMs; updated = true; }
    else if (declineRaises) { s->dirty |= declineRaises; s->rebuildDue = true; }
    s->dirty |= DIRTY_FRAMEBUFFER;
    return GI_C_OK;
  };
  // DIRTY_BVH without rebuildDue: visibility toggles and vertex edits alone raised it.  Each kind needs its option, else the rebuild is due; a vertex update
  // that declines makes it due as well (the visibility update behind it must not clear the flag).  With both kinds due the vertex update leaves DIRTY_BVH to
  // the visibility update.
  // DIRTY_BVH with topologyDue: meshes were created or destroyed, or meshes outside the built scene edited.  Without the option that is the rebuild, in today's
  // order of events.  With it updateTopology runs in front of every other path (the meshes it appends are part of the scene for them) and clears DIRTY_BVH
  // unless toggles or vertex edits of other meshes are due as well; a decline makes the rebuild due.
  // DIRTY_BVH with instancesDue: instance ids or counts of built meshes changed (GiCMesh::instEdited).  The same shape: without
  // GI_C_SCENE_OPTION_INSTANCE_UPDATES that is the rebuild; with it updateTopology applies them in front of its other work.
  if (s->topologyDue && !topologyUpdatesWanted(s)) s->rebuildDue = true;
  if (s->instancesDue && !instanceUpdatesWanted(s)) s->rebuildDue = true;
  const bool topologyRuns = (s->dirty & DIRTY_BVH) && !s->rebuildDue && (s->topologyDue || s->instancesDue);
  // (a topology update of the two-level layout has a counter of its own: giCDebugSceneTopologyUpdateCount keeps counting what it counted)
  const uint32_t topologyCounter = s->twoLevel && tlasTopologyWanted(s) && incrementalHost(s) ? (uint32_t)UPDATE_TLAS_TOPOLOGY : (uint32_t)UPDATE_TOPOLOGY;
  int rc = run(topologyRuns, updateTopology, topologyCounter, 0u, DIRTY_BVH, 0u);
  bool anyVis = false, anyVerts = false;
  for (const GiCMesh* m : s->meshes) { anyVis = anyVis || m->visToggled; anyVerts = anyVerts || m->vertsEdited; }
  if (rc == GI_C_OK && topologyRuns && !s->rebuildDue && !anyVis && !anyVerts) s->dirty &= ~DIRTY_BVH;
  if ((s->dirty & DIRTY_BVH) && anyVerts && (!vertexUpdatesWanted(s) || (anyVis && !visibilityUpdatesWanted(s)))) s->rebuildDue = true;
  // (a vertex update of the two-level layout has a counter of its own as well: giCDebugSceneVertexUpdateCount keeps counting what it counted)
  const uint32_t vertexCounter = s->twoLevel && blasUpdatesWanted(s) && incrementalHost(s) ? (uint32_t)UPDATE_BLAS : (uint32_t)UPDATE_VERTEX;
  if (rc == GI_C_OK) rc = run((s->dirty & DIRTY_BVH) && !s->rebuildDue && anyVerts, updateVertices, vertexCounter, anyVis ? 0u : (uint32_t)DIRTY_BVH, DIRTY_BVH, 0u);
  // (a visibility update of the two-level layout has a counter of its own as well: giCDebugSceneVisibilityUpdateCount keeps counting what it counted)
  const uint32_t visibilityCounter = s->twoLevel && tlasVisibilityWanted(s) && incrementalHost(s) ? (uint32_t)UPDATE_TLAS_VISIBILITY : (uint32_t)UPDATE_VISIBILITY;
  if (rc == GI_C_OK) rc = run((s->dirty & DIRTY_BVH) && !s->rebuildDue && visibilityUpdatesWanted(s), updateVisibility, visibilityCounter, DIRTY_BVH, 0u, 0u);
  if (rc == GI_C_OK) rc = run((s->dirty & DIRTY_MATERIALS) && !(s->dirty & DIRTY_BVH), updateMaterials, UPDATE_MATERIAL, DIRTY_MATERIALS, DIRTY_BVH, DIRTY_BVH);
  // (a transform update of the two-level layout has a counter of its own: giCDebugSceneUpdateCounts keeps counting what it counted)
  const uint32_t transformCounter = s->twoLevel && tlasUpdatesWanted(s) && incrementalHost(s) ? (uint32_t)UPDATE_TLAS : (uint32_t)UPDATE_TRANSFORM;
  if (rc == GI_C_OK) rc = run((s->dirty & DIRTY_XFORM) && !(s->dirty & (DIRTY_BVH | DIRTY_MATERIALS)), updateTransforms, transformCounter, 0u, DIRTY_BVH, 0u);
  if (updated) { s->stats.bvhBuildMs = spent.buildMs; s->stats.uploadMs = spent.uploadMs; s->stats.nodeCount = s->nodeCount;
      s->stats.triangleCount = s->triCount; } // (a full build below overrides all four)
  if (rc != GI_C_OK) return rc;
  if (s->dirty & (DIRTY_BVH | DIRTY_MATERIALS)) {
    s->generation++;
    if (buildScene(s) != GI_C_OK) return GI_C_ERROR;
    s->updateCounts[UPDATE_FULL]++;
    s->dirty &= ~(DIRTY_BVH | DIRTY_MATERIALS); s->dirty |= DIRTY_FRAMEBUFFER;
  }
  s->dirty &= ~DIRTY_XFORM; s->rebuildDue = false; s->topologyDue = false; s->instancesDue = false;
  for (GiCMesh* m : s->meshes) { m->visToggled = false; m->vertsEdited = false; m->instEdited = false; }
  return GI_C_OK;
}

// gi_scene.cpp -- scene, material and mesh containers with their dirty flags, primvars (Gi.cpp:620-782, Gi.h:76-92)
// (one of the translation units gi_c.cpp was split into in round 6; shared declarations: gi_host.h)
#include "gi_host.h"

extern "C" {
// ---------------------------------------------------------------------------------------------------------------
// scene / material / mesh
// ---------------------------------------------------------------------------------------------------------------
GiCScene* giCCreateScene(void)
{
  if (!g_ctx.initialized) { setError("giCCreateScene before giCInitialize"); return nullptr; }
  return new GiCScene();
}

void giCDestroyScene(GiCScene* s)
{
  if (!s) return;
  std::lock_guard<std::mutex> g(g_ctx.resourceMutex);
  for (auto& r : s->replicas) {
    (void)hipSetDevice(g_ctx.devs[r->slot].device);
    (void)hipStreamSynchronize(g_ctx.devs[r->slot].stream);
    r->releaseAll();
  }
  (void)hipSetDevice(g_ctx.device);
  (void)hipStreamSynchronize(g_ctx.stream);
  s->releaseAll();
  delete s;
}

GiCMaterial* giCCreateMaterial(GiCScene* scene, const char* name, const GiCMaterialDesc* desc)
{
  if (!scene || !desc) { setError("giCCreateMaterial: null argument"); return nullptr; }
  if (desc->klass > GI_C_MAT_OPEN_PBR) { setError("giCCreateMaterial: unsupported material class"); return nullptr; }
  // Hostile input (include/gi_c.h): a non-finite parameter would be NaN radiance on every path that meets the material.  Refused like a material the reference
  // fails to compile (giCreateMaterialFrom* return nullptr there, and hdGatling falls back to its default material, material.cpp)
  for (uint32_t i = 0; i < MAT_PARAM_COUNT; i++)
    if (!std::isfinite(desc->p[i])) { setError("giCCreateMaterial: parameter " + std::to_string(i) + " of material '" + (name ? name : "") + "' is not finite");
        return nullptr; }
  GiCMaterial* m = new GiCMaterial{scene, name ? name : "", *desc};
  // (subsurface_radius / subsurface_radius_scale, slots 32..35, are taken as given -- zeros included: the per-channel mean free path is clamped to 1e-6, as the
  // oracle does.  Round 5 read an all-zero radius AND scale as "unset"; that guess belongs
  // to the front ends, which set OpenPBR's defaults themselves: gtl_shim.cpp -- ADVICE r05)
  std::lock_guard<std::mutex> g(scene->mutex);
  scene->materials.push_back(m);
  scene->dirty |= materialEditFlags(scene->host != nullptr); // (material indices shift: the per-triangle word is patched, nothing is rebuilt)
  return m;
}

void giCDestroyMaterial(GiCMaterial* mat)
{
  if (!mat) return;
  GiCScene* s = mat->scene;
  {
    std::lock_guard<std::mutex> g(s->mutex);
    s->materials.erase(std::remove(s->materials.begin(), s->materials.end(), mat), s->materials.end());
    for (GiCMesh* m : s->meshes) if (m->material == mat) m->material = nullptr;
    for (GiCMesh* m : s->retiredMeshes) if (m->material == mat) m->material = nullptr;
    s->dirty |= materialEditFlags(s->host != nullptr); // (a mesh left without a material drops out of the scene: updateMaterials sees it and rebuilds)
  }
  delete mat;
}

static GiCMesh* createMeshImpl(GiCScene* scene, const GiCMeshDesc* d);
GiCMesh* giCCreateMesh(GiCScene* scene, const GiCMeshDesc* d)
{
  try { return createMeshImpl(scene, d); }
  catch (const std::exception& e) { setError(std::string("giCCreateMesh: ") + e.what()); return nullptr; }
}
static GiCMesh* createMeshImpl(GiCScene* scene, const GiCMeshDesc* d)
{
  if (!scene || !d) { setError("giCCreateMesh: null argument"); return nullptr; }
  if ((d->faceCount && !d->faces) || (d->vertexCount && !d->vertices)) { setError("giCCreateMesh: null arrays"); return nullptr; }
  for (uint32_t i = 0; i < d->faceCount; i++)
    for (int k = 0; k < 3; k++)
      if (d->faces[i].v_i[k] >= d->vertexCount) { setError("giCCreateMesh: face index out of range"); return nullptr; }
  std::unique_ptr<GiCMesh> m(new GiCMesh());
  m->scene = scene; m->name = d->name ? d->name : "";
  m->vertices.assign(d->vertices, d->vertices + d->vertexCount); // copies, like giProcessMeshData (Gi.cpp:628)
  m->faces.assign(d->faces, d->faces + d->faceCount);
  if (d->faceIds) m->faceIds.assign(d->faceIds, d->faceIds + d->faceCount);
  m->id = d->id; m->doubleSided = d->isDoubleSided != 0; m->flipFacing = d->isLeftHanded != 0; m->maxFaceId = d->maxFaceId;
  std::lock_guard<std::mutex> g(scene->mutex);
  scene->meshes.push_back(m.get());
  raiseTopology(scene); // (the flags of a rebuild; with GI_C_SCENE_OPTION_TOPOLOGY_UPDATES the mesh may be appended to the resident scene instead)
  return m.release();
}

void giCSetMeshTransform(GiCMesh* mesh, const float* mat4x4)
{
  if (!mesh || !mat4x4) return;
  std::lock_guard<std::mutex> g(mesh->scene->mutex); // buildScene reads the mesh under this lock (giCRender on another thread)
  memcpy(mesh->transform, mat4x4, sizeof(float) * 16);
  // same triangles elsewhere: incremental update (every instance of the mesh moves)
  if (mesh->builtInstances != 0xffffffffu) { mesh->xformDirty = true; mesh->instDirty.clear(); mesh->scene->dirty |= DIRTY_XFORM | DIRTY_FRAMEBUFFER; }
  else raiseTopology(mesh->scene);
}

void giCSetMeshInstanceTransforms(GiCMesh* mesh, uint32_t count, const float* transforms)
{
  try { // (a copy of the caller's array: an allocation failure must not cross the C ABI)
  if (!mesh || (count && !transforms)) return;
  std::vector<float> copy(transforms, transforms + (size_t)count * 16); // copy outside the lock, swap inside
  std::lock_guard<std::mutex> g(mesh->scene->mutex);
  mesh->instanceTransforms.swap(copy); // (`copy` now holds the previous transforms)
  if (mesh->builtInstances == count && copy.size() == (size_t)count * 16) { // same instance count: instances moved -- note which
    const bool all = mesh->xformDirty && mesh->instDirty.empty();
    if (!all) {
      if (mesh->instDirty.size() != count) mesh->instDirty.assign(count, 0);
      for (uint32_t i = 0; i < count; i++) if (memcmp(&copy[16 * (size_t)i], &mesh->instanceTransforms[16 * (size_t)i], 64) != 0) mesh->instDirty[i] = 1;
    }
    mesh->xformDirty = true; mesh->scene->dirty |= DIRTY_XFORM | DIRTY_FRAMEBUFFER;
  }
  else if (mesh->builtInstances == 0xffffffffu) raiseTopology(mesh->scene);
  else raiseInstances(mesh); // (another instance count of a mesh of the built scene: which of the kept instances moved is found against the resident records)
  } catch (const std::exception& e) { setError(std::string("giCSetMeshInstanceTransforms: ") + e.what()); }
}

void giCSetMeshInstanceIds(GiCMesh* mesh, uint32_t count, const int32_t* ids)
{
  try { // (a copy of the caller's array: an allocation failure must not cross the C ABI)
  if (!mesh || (count && !ids)) return;
  std::vector<int32_t> copy(ids, ids + count);
  std::lock_guard<std::mutex> g(mesh->scene->mutex);
  mesh->instanceIds.swap(copy);
  if (mesh->builtInstances == 0xffffffffu) raiseTopology(mesh->scene); else raiseInstances(mesh);
  } catch (const std::exception& e) { setError(std::string("giCSetMeshInstanceIds: ") + e.what()); }
}

void giCSetMeshMaterial(GiCMesh* mesh, GiCMaterial* mat)
{
  if (!mesh) return;
  std::lock_guard<std::mutex> g(mesh->scene->mutex);
  mesh->material = mat;
  // a mesh of the built scene keeps its triangles: only their material word changes.  One that is not part of it (new, invisible, left out for an invalid
  // material) may enter the scene now: rebuild
  if (mesh->builtInstances != 0xffffffffu) mesh->scene->dirty |= materialEditFlags(true); else raiseTopology(mesh->scene);
}

void giCSetMeshVisibility(GiCMesh* mesh, int32_t visible)
{
  if (!mesh) return;
  std::lock_guard<std::mutex> g(mesh->scene->mutex);
  mesh->visible = visible != 0;
  // the same flags as any geometry-side edit; the scene notes which meshes were toggled, and syncSceneGeometry may answer with updateVisibility instead of
  // the rebuild when nothing else asked for one (GI_C_SCENE_OPTION_VISIBILITY_UPDATES)
  mesh->visToggled = true;
  mesh->scene->dirty |= DIRTY_BVH | DIRTY_FRAMEBUFFER;
}

int giCSetMeshVertices(GiCMesh* mesh, uint32_t vertexCount, const GiCVertex* vertices)
{
  try { // (a copy of the caller's array: an allocation failure must not cross the C ABI)
  if (!mesh || (vertexCount && !vertices)) { setError("giCSetMeshVertices: null argument"); return GI_C_ERROR; }
  if ((size_t)vertexCount != mesh->vertices.size()) { // (the faces index the array: the topology stays)
    setError("giCSetMeshVertices: mesh '" + mesh->name + "' has " + std::to_string(mesh->vertices.size()) + " vertices, not " + std::to_string(vertexCount));
    return GI_C_ERROR;
  }
  std::vector<GiCVertex> copy(vertices, vertices + vertexCount); // copy outside the lock, swap inside
  std::lock_guard<std::mutex> g(mesh->scene->mutex);
  mesh->vertices.swap(copy);
  // the flags a geometry edit always raised; the scene notes which meshes were deformed, and syncSceneGeometry may answer with updateVertices instead of the
  // rebuild when nothing else asked for one (GI_C_SCENE_OPTION_VERTEX_UPDATES)
  mesh->vertsEdited = true;
  mesh->scene->dirty |= DIRTY_BVH | DIRTY_FRAMEBUFFER;
  return GI_C_OK;
  } catch (const std::exception& e) { setError(std::string("giCSetMeshVertices: ") + e.what()); return GI_C_ERROR; }
}

void giCDestroyMesh(GiCMesh* mesh)
{
  if (!mesh) return;
  GiCScene* s = mesh->scene;
  {
    std::lock_guard<std::mutex> g(s->mutex);
    s->meshes.erase(std::remove(s->meshes.begin(), s->meshes.end(), mesh), s->meshes.end());
    const bool built = mesh->builtInstances != 0xffffffffu && s->host != nullptr;
    if (built && topologyUpdatesWanted(s)) {
      // retired: the resident scene keeps referring to it (MeshBuild::m) until updateTopology has taken its triangles out and the next buildScene frees it.
      // For every loop over the built meshes it is a mesh hidden for good
      mesh->visible = false; mesh->retired = true;
      mesh->xformDirty = false; mesh->instDirty.clear(); // (a move of the same frame: its parts are unreachable, no transform update rebuilds them)
      s->retiredMeshes.push_back(mesh);
      raiseTopology(s);
      return;
    }
    // (a mesh of the built scene deleted at once leaves MeshBuild::m dangling: only the rebuild may follow, whatever the option says by then)
    if (built) raiseRebuild(s); else raiseTopology(s);
  }
  delete mesh;
}

// ---------------------------------------------------------------------------------------------------------------
// scene data (primvars): Gi.h:76-92, 134, 213
// ---------------------------------------------------------------------------------------------------------------
static int setPrimvarsImpl(GiCMesh* mesh, std::vector<GiCPrimvar>& dst, uint32_t count, const GiCPrimvarData* pv);
static int setPrimvars(GiCMesh* mesh, std::vector<GiCPrimvar>& dst, uint32_t count, const GiCPrimvarData* pv)
{
  try { return setPrimvarsImpl(mesh, dst, count, pv); }
  catch (const std::exception& e) { setError(std::string("giCSetMesh*Primvars: ") + e.what()); return GI_C_ERROR; }
}
static int setPrimvarsImpl(GiCMesh* mesh, std::vector<GiCPrimvar>& dst, uint32_t count, const GiCPrimvarData* pv)
{
  if (!mesh || (count && !pv)) { setError("giCSetMesh*Primvars: bad arguments"); return GI_C_ERROR; }
  std::vector<GiCPrimvar> v;
  for (uint32_t i = 0; i < count; i++) {
    if (!pv[i].name || pv[i].type < 0 || pv[i].type > GI_C_PRIMVAR_INT4 || pv[i].interpolation < 0
        || pv[i].interpolation > GI_C_INTERP_VERTEX) { setError("giCSetMesh*Primvars: bad primvar"); return GI_C_ERROR; }
    GiCPrimvar p{pv[i].name, pv[i].type, pv[i].interpolation, {}};
    // float and int32 elements are both 4 bytes: integer primvars keep their bit patterns in the float array (scene_data_lookup_int reads them back)
    if (pv[i].data) p.data.assign((const float*)pv[i].data, (const float*)pv[i].data + pv[i].dataSize / 4);
    v.push_back(std::move(p));
  }
  std::lock_guard<std::mutex> g(mesh->scene->mutex);
  dst = std::move(v);
  // Gi.cpp:685-700; primvars feed the per-mesh scene data, not the tree
  if (mesh->builtInstances != 0xffffffffu) mesh->scene->dirty |= materialEditFlags(true); else raiseTopology(mesh->scene);
  return GI_C_OK;
}
int giCSetMeshPrimvars(GiCMesh* mesh, uint32_t count, const GiCPrimvarData* pv) { return mesh
    ? setPrimvars(mesh, mesh->primvars, count, pv) : (setError("giCSetMeshPrimvars: null mesh"), GI_C_ERROR); }
int giCSetMeshInstancerPrimvars(GiCMesh* mesh, uint32_t count, const GiCPrimvarData* pv) { return mesh
    ? setPrimvars(mesh, mesh->instancerPrimvars, count, pv) : (setError("giCSetMeshInstancerPrimvars: null mesh"), GI_C_ERROR); }
int giCSetMaterialPrimvarInput(GiCMaterial* mat, int32_t input, const char* name)
{
  if (!mat || input < 0 || input >= GI_C_TEX_SLOT_COUNT || input == GI_C_TEX_NORMAL || input == GI_C_TEX_OPACITY
      || input == GI_C_TEX_COAT_NORMAL) { setError("giCSetMaterialPrimvarInput: bad arguments"); return GI_C_ERROR; }
  std::lock_guard<std::mutex> g(mat->scene->mutex);
  mat->primvarInput[input] = name ? name : "";
  mat->scene->dirty |= materialEditFlags(mat->scene->host != nullptr);
  return GI_C_OK;
}

} // extern "C"

// gi_blas_build.hip -- the BLAS of one mesh built on the device (gi_blas_build.h; DESIGN.md section 6 "BLAS build on the device").  This unit is the SOURCE of
// a box-tree build (gi_tlas_build.h BoxSource): it uploads the mesh's positions and face indices into its share of the scene's slab and makes, in one pass,
// the padded face boxes (blas_face_box, gi_blas.h), their float4 pairs, every workgroup's centroid bounds and every workgroup's share of mlo / mhi; a second
// launch of k_bvh_bounds reduces the latter (minima and maxima are exact in any order: the bytes are the host's).  Everything behind that -- Morton codes, the
// sort, PLOC, the depth-bounded collapse, the emission, the State record every kernel reads, the bound on host waits -- is gi_tlas_build.hip's, under
// kBlasBuildLimits.  No allocation outside the slab, no cooperative launch, no wait of one workgroup for another.
#include <algorithm>
#include <cstring>

#include "gi_blas.h"
#include "gi_blas_build.h"
#define GI_BVH_STAGE_KERNELS
#include "gi_bvh_stages.h"

namespace gi {
namespace {

constexpr uint32_t kBlock = kStageBlock;

// One face per thread.  pos: 3 floats per vertex; faces3: 3 indices per face (checked by the host; a stray one gives the inverted box all the same).
__global__ __launch_bounds__(kBlock) void k_blas_face_boxes(const float* __restrict__ pos, uint32_t vertexCount, const uint32_t* __restrict__ faces3, uint32_t nf,
    float* __restrict__ boxes6, float4* __restrict__ lo4, float4* __restrict__ hi4, float4* __restrict__ blockLo, float4* __restrict__ blockHi,
    uint32_t* __restrict__ blockAlive, float4* __restrict__ meshLo, float4* __restrict__ meshHi, uint32_t* __restrict__ meshUsable)
{
  __shared__ float4 sLo[kBlock], sHi[kBlock]; __shared__ uint32_t sAlive[kBlock];
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  float4 cLo = make_float4(3.0e38f, 3.0e38f, 3.0e38f, 0.0f), cHi = make_float4(-3.0e38f, -3.0e38f, -3.0e38f, 0.0f), mLo = cLo, mHi = cHi;
  uint32_t alive = 0, usable = 0;
  if (i < nf) {
    float b[6] = {3.0e38f, 3.0e38f, 3.0e38f, -3.0e38f, -3.0e38f, -3.0e38f};
    const uint32_t v0 = faces3[3u * (size_t)i], v1 = faces3[3u * (size_t)i + 1u], v2 = faces3[3u * (size_t)i + 2u];
    if (v0 < vertexCount && v1 < vertexCount && v2 < vertexCount) {
      const uint32_t v[3] = {v0, v1, v2};
      float p[3][3], lo[3], hi[3];
      for (int k = 0; k < 3; k++) for (int a = 0; a < 3; a++) p[k][a] = pos[3u * (size_t)v[k] + a];
      if (blas_face_box(p, lo, hi)) {
        for (int a = 0; a < 3; a++) { b[a] = lo[a]; b[3 + a] = hi[a]; }
        mLo = make_float4(lo[0], lo[1], lo[2], 0.0f); mHi = make_float4(hi[0], hi[1], hi[2], 0.0f); usable = 1;
      }
    }
    for (int a = 0; a < 6; a++) boxes6[6u * (size_t)i + a] = b[a];
    float4 bl, bh;
    stage_item_box(b, bl, bh, cLo, cHi, alive);
    lo4[i] = bl; hi4[i] = bh;
  }
  stage_block_bounds(cLo, cHi, alive, sLo, sHi, sAlive, blockLo, blockHi, blockAlive);
  __syncthreads(); // (thread 0 has read the first reduction's result)
  stage_block_bounds(mLo, mHi, usable, sLo, sHi, sAlive, meshLo, meshHi, meshUsable);
}

inline uint32_t blocksFor(uint32_t n) { return (n + kBlock - 1u) / kBlock; }
inline size_t align256(size_t x) { return (x + 255u) & ~(size_t)255u; }

// this source's share of the slab
struct Extra { size_t pos, faces, meshLo, meshHi, meshUsable, bounds, usable, bytes; };
Extra extraLayout(size_t vertexCount, size_t nf)
{
  Extra E{}; size_t at = 0; const size_t nb = std::max<size_t>(blocksFor((uint32_t)nf), 1u);
  auto take = [&](size_t bytes) { const size_t p = at; at = align256(at + std::max<size_t>(bytes, 1u)); return p; };
  E.pos = take(12u * vertexCount); E.faces = take(12u * nf); E.meshLo = take(16u * nb); E.meshHi = take(16u * nb); E.meshUsable = take(4u * nb);
  E.bounds = take(32u); E.usable = take(4u); E.bytes = at;
  return E;
}

struct MeshSource { const float* pos; size_t vertexCount; const GiCFace* faces; Extra E; };
hipError_t fillFromMesh(void* ctx, const BoxStage& stage, uint32_t n, hipStream_t st)
{
  const MeshSource& M = *static_cast<const MeshSource*>(ctx);
  uint8_t* x = static_cast<uint8_t*>(stage.extra);
  float* dPos = reinterpret_cast<float*>(x + M.E.pos); uint32_t* dFaces = reinterpret_cast<uint32_t*>(x + M.E.faces);
  float4 *dMeshLo = reinterpret_cast<float4*>(x + M.E.meshLo), *dMeshHi = reinterpret_cast<float4*>(x + M.E.meshHi), *dBounds = reinterpret_cast<float4*>(x + M.E.bounds);
  uint32_t *dMeshUsable = reinterpret_cast<uint32_t*>(x + M.E.meshUsable), *dUsable = reinterpret_cast<uint32_t*>(x + M.E.usable);
  hipError_t e = hipSuccess;
  if (M.vertexCount) e = hipMemcpyAsync(dPos, M.pos, 12u * M.vertexCount, hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = hipMemcpyAsync(dFaces, M.faces, 12u * (size_t)n, hipMemcpyHostToDevice, st);
  if (e != hipSuccess) return e;
  const uint32_t nb = blocksFor(n);
  k_blas_face_boxes<<<nb, kBlock, 0, st>>>(dPos, (uint32_t)M.vertexCount, dFaces, n, stage.boxes6, stage.lo4, stage.hi4, stage.blockLo, stage.blockHi, stage.blockAlive,
      dMeshLo, dMeshHi, dMeshUsable);
  k_bvh_bounds<<<1, kBlock, 0, st>>>(dMeshLo, dMeshHi, dMeshUsable, nb, dBounds, dUsable);
  return hipGetLastError();
}

} // namespace

int buildBlasDevice(TlasBuildWorkspace& ws, hipStream_t st, const GiCVertex* vertices, size_t vertexCount, const GiCFace* faces, size_t nf, uint32_t budget,
    uint32_t radius, Bvh8& out, std::vector<uint32_t>& order, float mlo[3], float mhi[3], BlasBuildInfo& info)
{
  info = BlasBuildInfo{}; out = Bvh8{}; order.clear();
  for (int a = 0; a < 3; a++) { mlo[a] = 3.0e38f; mhi[a] = -3.0e38f; }
  if (nf > kBlasMaxItems || vertexCount > 0xffffffffull) { info.error = "more items than the builder is sized for"; return TLAS_BUILD_ERROR; }
  static_assert(sizeof(GiCFace) == 12, "faces are uploaded as three indices each");
  for (size_t f = 0; f < nf; f++)
    for (int k = 0; k < 3; k++) if (faces[f].v_i[k] >= vertexCount) { info.error = "a face index outside the vertices"; return TLAS_BUILD_ERROR; }
  std::vector<float> pos(3 * vertexCount);
  for (size_t v = 0; v < vertexCount; v++) memcpy(&pos[3 * v], vertices[v].pos, 12);
  MeshSource M{pos.data(), vertexCount, faces, extraLayout(vertexCount, nf)};
  float bounds[8] = {3.0e38f, 3.0e38f, 3.0e38f, 0.0f, -3.0e38f, -3.0e38f, -3.0e38f, 0.0f};
  BoxSource source; source.fill = fillFromMesh; source.ctx = &M;
  source.extraBytes = M.E.bytes; source.backOffset = M.E.bounds; source.backBytes = sizeof(bounds); source.backHost = bounds;
  const int rc = buildBoxTreeDevice(ws, st, source, (uint32_t)nf, budget, radius, kBlasBuildLimits, out.nodes, order, info);
  if (rc != TLAS_BUILD_OK) { out = Bvh8{}; order.clear(); return rc; }
  for (int a = 0; a < 3; a++) { mlo[a] = bounds[a]; mhi[a] = bounds[4 + a]; }
  out.maxDepth = info.maxDepth; out.activeTris = info.active;
  out.levelStart.assign(info.levelStart, info.levelStart + info.maxDepth + 1u);
  return TLAS_BUILD_OK;
}

} // namespace gi

// gi_append.hip -- a mesh appended to a resident two-level scene without the flat tree (opt-in: GI_C_SCENE_OPTION_TLAS_TOPOLOGY; gi_build.cpp
// updateTopologyTwoLevel).  The host sends what the mesh has per vertex, per face and per instance; everything per face and per
// flattened triangle is made here, in device memory (gi_append.h has every per-item form, which the host runs as well):
//
//   k_append_shade_index  one thread per face: the tenth 16-byte piece of the face's 160-byte shading record -- TriShade::vi = vertexOffset + the face's three
//                         indices, pad 0 -- as ONE 16-byte store; 12 bytes read (consecutive lanes read consecutive faces), 16 stored per face.  The
//                         existing k_gather_shade (gi_refit.hip) then fills the other nine pieces from the vertex records just sent.
//   k_append_blas_tris    one thread per BLAS triangle of the mesh, in the builder's order: record i is face order[i].  THE WHOLE 64-byte record is written
//                         here (the corners from TriShade::p of the face's shading record, prim, six words of zero: bytewise makeBlasTri's) as four 16-byte
//                         stores per lane, as k_blas_tris stores its three -- k_blas_tris is NOT run behind it.  4 + 36 bytes read (the shading records by
//                         prim: scattered lines), 64 stored per face; nf faces however many instances there are.
//   k_append_records      the hot one: per (instance of the mesh, face), instances-major, the whole 64-byte TriRec, the record's face-id word and its word of
//                         the id table (flatOfOrig[origId] = position).  Mapping: ONE 16-BYTE PIECE PER LANE, four lanes per record (k_gather_shade's
//                         scheme, not k_blas_tris's record per lane): consecutive lanes store consecutive 16-byte pieces, so a wave's one store instruction
//                         covers 16 records = 1 024 contiguous bytes, the widest access there is; a record per lane would put every lane of a store 64 bytes
//                         apart.  Each lane forms its own piece: the three lanes with floats run refit_flatten (27 multiply-adds, nothing against the
//                         stores), the fourth copies indices.  The lane of piece 2 holds origId and stores the id-table word, the lane of piece 3 holds prim
//                         and stores the face-id word: 16 consecutive dwords per wave each.  Bytes per item (one record): 64 + 4 + 4 = 72 stored, 36 of
//                         TriShade::p and 8 of TriShade::vi read (nf records shared by all instances: they hit in L2), 4 of the face-id table per record and
//                         48 of one InstanceRec per instance.  Instances-major order keeps o2w uniform over a wave for all but the waves that hold an
//                         instance boundary (16 records per wave: one wave in nf / 16).
//
// Order on one stream: k_append_shade_index, k_gather_shade, then the other two (both read TriShade::p).  A kernel boundary is the only hand-off: nothing
// crosses workgroups inside a launch.  No atomics, no counters, no fences; every word has one writer.  Every index is checked against its array's count: a
// "cannot happen" returns.  Plain HIP C++.
#include <cstddef>

#include "gi_append.h"
#include "gi_kernels.h"

namespace gi {
namespace {

constexpr uint32_t kAppendBlock = 256;

__global__ __launch_bounds__(kAppendBlock) void k_append_shade_index(TriShade* __restrict__ triShade, uint32_t shadeCount, uint32_t shadeBase,
    const uint32_t* __restrict__ faces3, uint32_t faceCount, uint32_t vertexOffset)
{
  const uint32_t f = blockIdx.x * kAppendBlock + threadIdx.x;
  if (f >= faceCount) return;
  if (shadeBase > shadeCount || f >= shadeCount - shadeBase) return; // (cannot happen: the host checks the range against the array)
  const uint32_t face[3] = {faces3[3u * (size_t)f], faces3[3u * (size_t)f + 1u], faces3[3u * (size_t)f + 2u]};
  uint32_t w[4];
  append_shade_index(face, vertexOffset, w);
  reinterpret_cast<uint4*>(triShade + shadeBase + f)[9] = make_uint4(w[0], w[1], w[2], w[3]); // 160-byte records in a hipMalloc block: every piece is 16-byte aligned
}

__global__ __launch_bounds__(kAppendBlock) void k_append_blas_tris(BlasTri* __restrict__ blasTris, uint32_t blasTriCount, uint32_t first,
    const uint32_t* __restrict__ order, uint32_t faceCount, const TriShade* __restrict__ triShade, uint32_t shadeCount, uint32_t shadeBase)
{
  const uint32_t i = blockIdx.x * kAppendBlock + threadIdx.x;
  if (i >= faceCount) return;
  if (first > blasTriCount || i >= blasTriCount - first) return; // (cannot happen: the host grew the array to hold the range)
  const uint32_t prim = order[i];
  if (prim >= faceCount || shadeBase > shadeCount || prim >= shadeCount - shadeBase) return; // (cannot happen: the builder's order is a permutation of the faces)
  uint32_t w[16];
  append_blas_tri(triShade[shadeBase + prim], prim, w);
  uint4* rec = reinterpret_cast<uint4*>(blasTris + first + i); // 64-byte records in a hipMalloc block: 16-byte aligned pieces
  rec[0] = make_uint4(w[0], w[1], w[2], w[3]); rec[1] = make_uint4(w[4], w[5], w[6], w[7]);
  rec[2] = make_uint4(w[8], w[9], w[10], w[11]); rec[3] = make_uint4(w[12], w[13], w[14], w[15]);
}

__global__ __launch_bounds__(kAppendBlock) void k_append_records(AppendMesh M, TriRec* __restrict__ tris, int32_t* __restrict__ triFaceId,
    uint32_t* __restrict__ flatOfOrig, const InstanceRec* __restrict__ instances, const TriShade* __restrict__ triShade, const int32_t* __restrict__ faceIdOfFace)
{
  const uint32_t i = blockIdx.x * kAppendBlock + threadIdx.x; // (fewer than 2^28 items: 4 * items fits)
  const uint32_t item = i >> 2, piece = i & 3u;
  if (!append_item_ok(M, item)) return; // (past the last item; anything else cannot happen: the host asks appendMeshRangesOk first)
  uint32_t ii, prim;
  append_item(M, item, ii, prim);
  const TriShade& q = triShade[M.shadeBase + prim];
  uint32_t w[4];
  append_record_piece(M, ii, prim, instances[M.instFirst + ii].o2w, q, piece, w);
  const uint32_t at = M.triFirst + item;
  reinterpret_cast<uint4*>(tris + at)[piece] = make_uint4(w[0], w[1], w[2], w[3]); // 64-byte records in a hipMalloc block: 16-byte aligned pieces
  if (piece == 2u) flatOfOrig[w[1]] = at;               // (w[1]: the record's origId, inside the table by append_item_ok)
  else if (piece == 3u) triFaceId[at] = faceIdOfFace[prim];
}

} // namespace

bool launchAppendShadeIndex(hipStream_t s, TriShade* triShade, uint32_t shadeCount, uint32_t shadeBase, const uint32_t* faces3, uint32_t faceCount,
    uint32_t vertexOffset)
{
  if (shadeBase > shadeCount || faceCount > shadeCount - shadeBase || faceCount >= (1u << 26)) return false;
  if (faceCount == 0u) return true;
  hipLaunchKernelGGL(k_append_shade_index, dim3((faceCount + kAppendBlock - 1u) / kAppendBlock), dim3(kAppendBlock), 0, s, triShade, shadeCount, shadeBase, faces3,
      faceCount, vertexOffset);
  return true;
}

bool launchAppendBlasTris(hipStream_t s, BlasTri* blasTris, uint32_t blasTriCount, uint32_t first, const uint32_t* order, uint32_t faceCount,
    const TriShade* triShade, uint32_t shadeCount, uint32_t shadeBase)
{
  if (first > blasTriCount || faceCount > blasTriCount - first || shadeBase > shadeCount || faceCount > shadeCount - shadeBase || faceCount >= (1u << 26)) return false;
  if (faceCount == 0u) return true;
  hipLaunchKernelGGL(k_append_blas_tris, dim3((faceCount + kAppendBlock - 1u) / kAppendBlock), dim3(kAppendBlock), 0, s, blasTris, blasTriCount, first, order,
      faceCount, triShade, shadeCount, shadeBase);
  return true;
}

bool launchAppendRecords(hipStream_t s, const AppendMesh& M, TriRec* tris, int32_t* triFaceId, uint32_t* flatOfOrig, const InstanceRec* instances,
    const TriShade* triShade, const int32_t* faceIdOfFace)
{
  if (!appendMeshRangesOk(M)) return false;
  const uint32_t threads = M.faceCount * M.instCount * 4u;
  hipLaunchKernelGGL(k_append_records, dim3((threads + kAppendBlock - 1u) / kAppendBlock), dim3(kAppendBlock), 0, s, M, tris, triFaceId, flatOfOrig, instances,
      triShade, faceIdOfFace);
  return true;
}

} // namespace gi

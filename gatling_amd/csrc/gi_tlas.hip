// gi_tlas.hip -- the world boxes of moved instances of a two-level scene (opt-in: GI_C_SCENE_OPTION_TLAS_UPDATES; gi_build.cpp updateTransformsTwoLevel,
// DESIGN.md section 6).  An instance moved: its mesh's BLAS stays, its InstTrav record and its world box change, and the TLAS is built again over all boxes.
// The box is a minimum / maximum over every BLAS triangle of the mesh under the new transform -- nf x 3 point transforms per instance, the one loop of the
// edit that grows with the scene -- and is made here, from the BlasTri records the device already holds.
//
//   k_inst_bounds   one workgroup of 256 threads per (job, chunk of 4 096 BLAS triangles); a job is one dirty instance: its new o2w, its mesh's first BLAS
//                   triangle and face count (a 64-byte entry of a table the host uploads).  A lane reads the 48 used bytes of a 64-byte BlasTri as three
//                   16-byte loads, transforms the three corners (gi_tlas.h tlas_bounds_add_tri: the host's operations in its order), folds them into its
//                   own (lo, hi, status) and strides by 256 to the next triangle of the chunk.  Per triangle a wave reads 64 consecutive records = 4 KiB
//                   of which 3 KiB are used (the other 16 bytes of each line are never requested) and writes nothing; per chunk the workgroup writes one
//                   32-byte partial.  The lanes' results are folded across the wave with cross-lane shuffles (64 lanes, six steps), across the four waves
//                   through 128 bytes of LDS, and lane 0 stores the partial with two 16-byte vector stores.  Memory-bound: 48 bytes and 27 multiplies per
//                   triangle; the BLAS records of a mesh are shared by all its instances and stay in L2 / the Infinity Cache from the second job on.
//   k_inst_finish   one thread per job: folds the job's partials in chunk order, pads the box (gi_tlas.h tlas_pad_box) and stores six floats and the status.
//
// Why the padded box is bytewise the host loop's whatever the order of the fold: the lanes transform with the host's operations (no contraction), and the fold
// is minimum / maximum by comparison, which never picks a NaN and is associative and commutative over comparable floats but for the sign of a zero; the pad
// that follows is positive and turns -0 and +0 into the same bits (gi_tlas.h).  The status is an OR.
//
// The chunk partials cross a KERNEL BOUNDARY between the two launches, never a hand-off inside one (the device builder's and gi_refit.hip's rule: the per-XCD
// L2s are not coherent within a launch; k_bvh_boxes / k_bvh_bounds reduce the same way).  No atomics, no counters, no fences; every word has one writer.  Both
// kernels write scratch only: nothing resident changes before the host has read the statuses.
#include <cstddef>

#include "gi_kernels.h"
#include "gi_tlas.h"

namespace gi {
namespace {

constexpr uint32_t kBoundsBlock = 256, kBoundsWaves = kBoundsBlock / 64u;
static_assert(sizeof(InstBoundsJob) == 64 && sizeof(BlasTri) == 64 && offsetof(BlasTri, prim) == 36, "k_inst_bounds: 16-byte pieces of its records");

__device__ inline float shfl_min(float v, int delta) { return refit_min(v, __shfl_xor(v, delta, 64)); }
__device__ inline float shfl_max(float v, int delta) { return refit_max(v, __shfl_xor(v, delta, 64)); }

// partial (job, chunk): lo xyz, status bits | hi xyz, 0 -- 8 words at 8 * (job * chunksPerJob + chunk)
__global__ __launch_bounds__(kBoundsBlock) void k_inst_bounds(const InstBoundsJob* __restrict__ jobs, uint32_t jobCount, uint32_t chunksPerJob,
    const BlasTri* __restrict__ blasTris, uint32_t blasTriCount, float4* __restrict__ partials)
{
  __shared__ float4 sm[kBoundsWaves][2];
  const uint32_t job = blockIdx.x / chunksPerJob, chunk = blockIdx.x % chunksPerJob;
  if (job >= jobCount) return; // (cannot happen: the grid is jobCount * chunksPerJob blocks; uniform over the workgroup)
  const uint32_t firstTri = jobs[job].firstTri, faceCount = jobs[job].faceCount;
  const uint32_t chunkFirst = chunk * kInstBoundsChunk;
  if (chunkFirst >= faceCount) return; // a job with fewer chunks than the longest one: k_inst_finish never reads this partial (uniform)
  TlasBounds b; tlas_bounds_init(b);
  // (cannot happen: the host takes the range from the mesh's own BLAS) -- no load, and a status the host declines on
  const bool inRange = firstTri <= blasTriCount && faceCount <= blasTriCount - firstTri;
  if (!inRange) b.status = TLAS_STATUS_RANGE;
  else {
    float o2w[12];
    for (int i = 0; i < 12; i++) o2w[i] = jobs[job].o2w[i];
    const uint32_t chunkEnd = faceCount - chunkFirst < kInstBoundsChunk ? faceCount : chunkFirst + kInstBoundsChunk;
    for (uint32_t t = chunkFirst + threadIdx.x; t < chunkEnd; t += kBoundsBlock) {
      const float4* rec = reinterpret_cast<const float4*>(blasTris + firstTri + t); // 64-byte records in a hipMalloc block: 16-byte aligned pieces
      const float4 r0 = rec[0], r1 = rec[1], r2 = rec[2]; // p0 xyz p1 x | p1 yz p2 xy | p2 z, prim, -, -
      const float p[3][3] = {{r0.x, r0.y, r0.z}, {r0.w, r1.x, r1.y}, {r1.z, r1.w, r2.x}};
      tlas_bounds_add_tri(o2w, p, b, true);
    }
  }
  for (int delta = 32; delta > 0; delta >>= 1) {
    for (int a = 0; a < 3; a++) { b.lo[a] = shfl_min(b.lo[a], delta); b.hi[a] = shfl_max(b.hi[a], delta); }
    b.status |= (uint32_t)__shfl_xor((int)b.status, delta, 64);
  }
  const uint32_t wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63u) == 0u) { sm[wave][0] = make_float4(b.lo[0], b.lo[1], b.lo[2], __uint_as_float(b.status)); sm[wave][1] = make_float4(b.hi[0], b.hi[1], b.hi[2], 0.0f); }
  __syncthreads();
  if (threadIdx.x != 0u) return;
  for (uint32_t w = 1; w < kBoundsWaves; w++) {
    const float4 l = sm[w][0], h = sm[w][1];
    const float lo[3] = {l.x, l.y, l.z}, hi[3] = {h.x, h.y, h.z};
    tlas_bounds_merge(b, lo, hi, __float_as_uint(l.w));
  }
  float4* out = partials + 2u * ((size_t)job * chunksPerJob + chunk);
  out[0] = make_float4(b.lo[0], b.lo[1], b.lo[2], __uint_as_float(b.status));
  out[1] = make_float4(b.hi[0], b.hi[1], b.hi[2], 0.0f);
}

// out: 7 words per job -- the padded box (lo xyz, hi xyz) and the status
__global__ __launch_bounds__(kBoundsBlock) void k_inst_finish(const InstBoundsJob* __restrict__ jobs, uint32_t jobCount, uint32_t chunksPerJob,
    const float4* __restrict__ partials, uint32_t* __restrict__ out)
{
  const uint32_t job = blockIdx.x * kBoundsBlock + threadIdx.x;
  if (job >= jobCount) return;
  const uint32_t faceCount = jobs[job].faceCount;
  uint32_t chunks = faceCount / kInstBoundsChunk + (faceCount % kInstBoundsChunk ? 1u : 0u);
  TlasBounds b; tlas_bounds_init(b);
  if (chunks > chunksPerJob) { chunks = 0u; b.status = TLAS_STATUS_RANGE; } // (cannot happen: chunksPerJob is the longest job's count)
  for (uint32_t c = 0; c < chunks; c++) {
    const float4 l = partials[2u * ((size_t)job * chunksPerJob + c)], h = partials[2u * ((size_t)job * chunksPerJob + c) + 1u];
    const float lo[3] = {l.x, l.y, l.z}, hi[3] = {h.x, h.y, h.z};
    tlas_bounds_merge(b, lo, hi, __float_as_uint(l.w));
  }
  tlas_pad_box(b.lo, b.hi);
  uint32_t* o = out + 7u * (size_t)job;
  for (int a = 0; a < 3; a++) { o[a] = __float_as_uint(b.lo[a]); o[3 + a] = __float_as_uint(b.hi[a]); }
  o[6] = b.status;
}

} // namespace

uint32_t instBoundsChunks(uint32_t faceCount) { return faceCount / kInstBoundsChunk + (faceCount % kInstBoundsChunk ? 1u : 0u); }

bool launchInstBounds(hipStream_t s, const InstBoundsJob* jobs, uint32_t jobCount, uint32_t chunksPerJob, const BlasTri* blasTris, uint32_t blasTriCount,
    float* partials, uint32_t* out)
{
  if (jobCount == 0u) return true;
  if (chunksPerJob == 0u || (uint64_t)jobCount * chunksPerJob >= (1ull << 31)) return false;
  hipLaunchKernelGGL(k_inst_bounds, dim3(jobCount * chunksPerJob), dim3(kBoundsBlock), 0, s, jobs, jobCount, chunksPerJob, blasTris, blasTriCount,
      reinterpret_cast<float4*>(partials));
  hipLaunchKernelGGL(k_inst_finish, dim3((jobCount + kBoundsBlock - 1u) / kBoundsBlock), dim3(kBoundsBlock), 0, s, jobs, jobCount, chunksPerJob,
      reinterpret_cast<const float4*>(partials), out);
  return true;
}

} // namespace gi

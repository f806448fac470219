// gi_instances.hip -- new instances of built meshes on a resident two-level scene without the flat tree (opt-in: GI_C_SCENE_OPTION_TLAS_INSTANCES; gi_build.cpp
// updateInstancesTwoLevel).  The BLAS of a built mesh is resident and shared, so one more instance costs one InstanceRec, one InstTrav and
// one TLAS box from the host, and nf flat records made here (gi_instances.h has every per-item form, which the host runs as well):
//
//   k_instance_records    ONE launch for all new instances of all meshes of a sync.  Input: a table of 32-byte jobs, one per new instance -- its InstanceRec,
//                         its first flat record (a slot a retired instance left, or the end of the array: the ranges lie anywhere, in any order), the
//                         scene-order id of its first triangle, its mesh's shadeBase / faceCount / matFlags / face-id table offset, and its first workgroup, a
//                         prefix over ceil(4 x faceCount / 256).  Nothing per triangle and nothing per workgroup crosses the link.
//                         Mapping: one 16-BYTE PIECE PER LANE, four lanes per record, as k_append_records (gi_append.hip): consecutive lanes store
//                         consecutive pieces, a wave's one store instruction covers 16 records = 1 024 contiguous bytes.  A WORKGROUP BELONGS TO ONE JOB: it
//                         finds it by binary search over the prefix with blockIdx.x -- ceil(log2(jobs)) steps over a table that stays in the scalar cache,
//                         the same in every lane, so the job record and the instance's o2w are uniform over the whole workgroup and no instance boundary falls
//                         inside a wave (k_append_records has one such wave in nf / 16).  The last workgroup of a job is partly filled: at most 63 idle
//                         record slots per job.  The lane of piece 2 holds origId and stores the id-table word, the lane of piece 3 holds prim and stores the
//                         face-id word: 16 consecutive dwords per wave each.
//                         Bytes per item (one record): 64 + 4 + 4 = 72 stored; 36 of TriShade::p and 8 of TriShade::vi read (nf records shared by all
//                         instances of a mesh: they hit in L2), 4 of the face-id table; per workgroup 32 of the job and 48 of one InstanceRec, uniform.
//
// No atomics, no counters, no fences, no LDS; every word has one writer (the host refuses overlapping ranges).  Every index is checked against its array's
// count: a "cannot happen" returns.  Plain HIP C++.
#include <cstddef>

#include "gi_instances.h"
#include "gi_kernels.h"

namespace gi {
namespace {

__global__ __launch_bounds__(kInstanceRecordsBlock) void k_instance_records(const InstanceJob* __restrict__ jobs, InstanceJobSizes Z, TriRec* __restrict__ tris,
    int32_t* __restrict__ triFaceId, uint32_t* __restrict__ flatOfOrig, const InstanceRec* __restrict__ instances, const TriShade* __restrict__ triShade,
    const int32_t* __restrict__ faceIdTable)
{
  instance_records_thread(jobs, Z, blockIdx.x, threadIdx.x, tris, triFaceId, flatOfOrig, instances, triShade, faceIdTable);
}

} // namespace

bool launchInstanceRecords(hipStream_t s, const InstanceJob* hostJobs, const InstanceJob* deviceJobs, const InstanceJobSizes& Z, TriRec* tris, int32_t* triFaceId,
    uint32_t* flatOfOrig, const InstanceRec* instances, const TriShade* triShade, const int32_t* faceIdTable)
{
  if (!instanceJobsOk(hostJobs, Z)) return false;
  if (Z.jobCount == 0u) return true;
  hipLaunchKernelGGL(k_instance_records, dim3(Z.wgCount), dim3(kInstanceRecordsBlock), 0, s, deviceJobs, Z, tris, triFaceId, flatOfOrig, instances, triShade, faceIdTable);
  return true;
}

} // namespace gi

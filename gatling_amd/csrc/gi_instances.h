// gi_instances.h -- the per-item arithmetic of new instances of BUILT meshes on a resident two-level scene without the flat tree (gi_instances.hip
// k_instance_records; gi_build.cpp updateInstancesTwoLevel, giCDebugInstanceRecords), shared by the host and the device kernel as
// gi_append.h is.  An instancer whose count goes up and down reuses the storage slots its retired instances left, so the new instances of one sync lie at
// arbitrary InstanceRec indices and arbitrary flat-record ranges, of any number of meshes: one JOB per new instance names them, and one launch makes the flat
// records, face-id words and id-table words of all jobs.  The record itself is gi_append.h's (append_record_piece over refit_flatten): a job is presented to it
// as an AppendMesh of ONE instance, so the device's bytes are the host's and the host's are flattenInstance's (giCDebugInstanceRecordsHost holds that).
#pragma once

#include <cstddef>
#include <cstdint>

#include "gi_append.h"

namespace gi {

constexpr uint32_t kInstanceRecordsBlock = 256; // threads of a workgroup: 64 records of four 16-byte pieces

// One new instance: where its records go, what they name.  32 bytes; the host sends nothing per triangle and nothing per workgroup
struct InstanceJob {
  uint32_t instance, triFirst, idBase, shadeBase; // its InstanceRec; its first flat record; the scene-order id of its first triangle; its mesh's first shading record
  uint32_t faceCount, matFlags, faceIdFirst, wgFirst; // its mesh's faces and TriRec::matFlags; the mesh's first word of the face-id table; the job's first workgroup
};
static_assert(sizeof(InstanceJob) == 32, "InstanceJob: two 16-byte pieces");
// The sizes every index is checked against
struct InstanceJobSizes { uint32_t jobCount, triCount, instanceCount, shadeCount, flatCount, faceIdCount, wgCount, pad; };

GI_REFIT_HD inline uint32_t instance_job_workgroups(uint32_t faceCount) { return (faceCount + kInstanceRecordsBlock / 4u - 1u) / (kInstanceRecordsBlock / 4u); } // ceil(4 x faceCount / 256)

// The job of workgroup `wg`: the last one whose first workgroup is not behind it (wgFirst is the prefix over the jobs' workgroup counts, so it ascends
// strictly: every job has a face).  The same answer in every lane of a workgroup
GI_REFIT_HD inline uint32_t instance_job_of(const InstanceJob* jobs, uint32_t jobCount, uint32_t wg)
{
  uint32_t lo = 0u, hi = jobCount; // (jobs[lo].wgFirst <= wg < jobs[hi].wgFirst, the count standing for "past the end")
  while (hi - lo > 1u) { const uint32_t mid = lo + (hi - lo) / 2u; if (jobs[mid].wgFirst <= wg) lo = mid; else hi = mid; }
  return lo;
}

// The job as the one-instance mesh gi_append.h's forms take
GI_REFIT_HD inline AppendMesh instance_job_mesh(const InstanceJob& j, const InstanceJobSizes& Z)
{
  AppendMesh M{}; M.triFirst = j.triFirst; M.faceCount = j.faceCount; M.instFirst = j.instance; M.instCount = 1u; M.shadeBase = j.shadeBase; M.idBase = j.idBase;
  M.matFlags = j.matFlags; M.triCount = Z.triCount; M.instanceCount = Z.instanceCount; M.shadeCount = Z.shadeCount; M.flatCount = Z.flatCount;
  return M;
}
// ... and whether face `prim` of it reads and writes inside every array (false cannot happen: the host asks instanceJobsOk first)
GI_REFIT_HD inline bool instance_item_ok(const InstanceJob& j, const InstanceJobSizes& Z, uint32_t prim)
{
  return append_item_ok(instance_job_mesh(j, Z), prim) && j.faceIdFirst <= Z.faceIdCount && prim < Z.faceIdCount - j.faceIdFirst;
}

// Thread (workgroup wg, lane-in-workgroup t): piece t & 3 of record t >> 2 of the workgroup's 64, of the job the workgroup belongs to.  The record, its
// face-id word (the lane of piece 3) and its id-table word (the lane of piece 2).  One writer per word
GI_REFIT_HD inline void instance_records_thread(const InstanceJob* jobs, const InstanceJobSizes& Z, uint32_t wg, uint32_t t, TriRec* tris, int32_t* triFaceId,
    uint32_t* flatOfOrig, const InstanceRec* instances, const TriShade* triShade, const int32_t* faceIdTable)
{
  if (Z.jobCount == 0u || wg >= Z.wgCount) return;
  const InstanceJob j = jobs[instance_job_of(jobs, Z.jobCount, wg)];
  if (wg < j.wgFirst) return; // (cannot happen: the first job starts at workgroup 0)
  const uint32_t prim = (wg - j.wgFirst) * (kInstanceRecordsBlock / 4u) + (t >> 2), piece = t & 3u;
  if (!instance_item_ok(j, Z, prim)) return; // (past the job's last face: its last workgroup is partly filled)
  const AppendMesh M = instance_job_mesh(j, Z);
  uint32_t w[4];
  append_record_piece(M, 0u, prim, instances[j.instance].o2w, triShade[j.shadeBase + prim], piece, w);
  const uint32_t at = j.triFirst + prim;
  // (64-byte records in a hipMalloc block, a std::vector's on the host: 16-byte aligned pieces, ONE 16-byte store per lane)
  __builtin_memcpy(__builtin_assume_aligned(reinterpret_cast<char*>(&tris[at]) + 16u * piece, 16), w, 16);
  if (piece == 2u) flatOfOrig[w[1]] = at;                    // (w[1]: the record's origId, inside the table by append_item_ok)
  else if (piece == 3u) triFaceId[at] = faceIdTable[j.faceIdFirst + prim];
}

// The range check: every job inside its arrays, fewer than 2^28 items in all, the prefix the job sizes'.  What the host asks before it launches anything
inline bool instanceJobsOk(const InstanceJob* jobs, const InstanceJobSizes& Z)
{
  if (Z.jobCount == 0u) return Z.wgCount == 0u;
  if (!jobs) return false;
  uint64_t items = 0, wg = 0;
  for (uint32_t k = 0; k < Z.jobCount; k++) {
    const InstanceJob& j = jobs[k];
    if (j.faceCount == 0u || j.wgFirst != wg) return false;
    const AppendMesh M = instance_job_mesh(j, Z);
    if (!appendMeshRangesOk(M) || j.faceIdFirst > Z.faceIdCount || j.faceCount > Z.faceIdCount - j.faceIdFirst) return false;
    items += j.faceCount; wg += instance_job_workgroups(j.faceCount);
    if (items >= (1ull << 28)) return false;
  }
  return wg == Z.wgCount;
}
// ... the prefix, filled in: returns the launch's workgroups (0: 2^28 or more items)
inline uint32_t instanceJobsNumber(InstanceJob* jobs, uint32_t jobCount)
{
  uint64_t wg = 0, items = 0;
  for (uint32_t k = 0; k < jobCount; k++) { jobs[k].wgFirst = (uint32_t)wg; wg += instance_job_workgroups(jobs[k].faceCount); items += jobs[k].faceCount;
      if (items >= (1ull << 28)) return 0u; }
  return (uint32_t)wg;
}

// The host form of the kernel, workgroups [first, last): the caller may split the range over threads (one writer per word)
inline void instanceRecordsHost(const InstanceJob* jobs, const InstanceJobSizes& Z, uint32_t first, uint32_t last, TriRec* tris, int32_t* triFaceId, uint32_t* flatOfOrig,
    const InstanceRec* instances, const TriShade* triShade, const int32_t* faceIdTable)
{
  for (uint32_t wg = first; wg < last; wg++)
    for (uint32_t t = 0; t < kInstanceRecordsBlock; t++) instance_records_thread(jobs, Z, wg, t, tris, triFaceId, flatOfOrig, instances, triShade, faceIdTable);
}

} // namespace gi

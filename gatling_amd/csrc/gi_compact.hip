// gi_compact.hip -- the retired ranges of a resident two-level scene without the flat tree, compacted (opt-in: GI_C_SCENE_OPTION_TLAS_COMPACTION; gi_build.cpp
// compactTwoLevel, DESIGN.md section 6 "Compaction of retired ranges").  Every array of the scene is a sequence of live and dead ranges; the live ones move
// to the front of a NEW allocation in storage order, and the indices their records hold are rebased (gi_compact.h has every per-item form, which the host
// runs as well):
//
//   k_compact_ranges<KIND>  ONE launch per array kind for all its ranges.  Input: a table of 32-byte ranges -- first item in the old array, first item in the
//                         new one, items, three deltas, flags, and the range's first workgroup, a prefix over ceil(items x pieces / 256).  Nothing per item
//                         and nothing per workgroup crosses the link.
//                         Mapping: k_instance_records's (gi_instances.hip) -- one 16-BYTE PIECE PER LANE, consecutive lanes hold consecutive pieces, so a
//                         wave's one load and one store instruction cover 1 024 contiguous bytes each whatever the record size (48, 64, 80, 96, 128, 160
//                         bytes); A WORKGROUP BELONGS TO ONE RANGE and finds it by binary search over the prefix with blockIdx.x, the same in every lane, so
//                         the range record is uniform over the workgroup.  The last workgroup of a range is partly filled.  The lane that holds an index adds
//                         the range's delta to it (uint32, unconditionally); the lane that holds a flat record's origId also stores the record's new index
//                         into the new id table -- one more dword store in one lane of four, unless the range belongs to a hidden instance.  The face-id
//                         words move a dword per lane.
//                         Bytes per item: the record read once and stored once; 32 of the range table per workgroup, uniform.
//
// The old and the new place of a range overlap, so the kernel never moves inside one allocation: `src` and `dst` are different blocks (the caller swaps them in
// behind the launch, as DeviceBuffer::grow does).  No atomics, no counters, no fences, no LDS; every word has one writer (compactRangesOk: the destinations
// ascend without gaps).  Every index is checked against its array's count: a "cannot happen" returns.  Plain HIP C++.
#include <cstddef>

#include "gi_compact.h"
#include "gi_kernels.h"

namespace gi {
namespace {

template <uint32_t KIND>
__global__ __launch_bounds__(kCompactBlock) void k_compact_ranges(const CompactRange* __restrict__ ranges, CompactSizes Z, const void* __restrict__ src,
    void* __restrict__ dst, uint32_t* __restrict__ table)
{
  Z.kind = KIND; // (a constant: the pieces per item and the rebase are folded)
  compact_thread(ranges, Z, blockIdx.x, threadIdx.x, src, dst, table);
}

template <uint32_t KIND>
void launchKind(hipStream_t s, const CompactRange* ranges, const CompactSizes& Z, const void* src, void* dst, uint32_t* table)
{
  hipLaunchKernelGGL(k_compact_ranges<KIND>, dim3(Z.wgCount), dim3(kCompactBlock), 0, s, ranges, Z, src, dst, table);
}

} // namespace

bool launchCompactRanges(hipStream_t s, const CompactRange* hostRanges, const CompactRange* deviceRanges, const CompactSizes& Z, const void* src, void* dst,
    uint32_t* table)
{
  if (!compactRangesOk(hostRanges, Z) || (Z.wgCount != 0u && (!src || !dst || src == dst))) return false;
  if (Z.wgCount == 0u) return true;
  switch (Z.kind) {
    case COMPACT_VERTS: launchKind<COMPACT_VERTS>(s, deviceRanges, Z, src, dst, table); break;
    case COMPACT_BLAS_TRIS: launchKind<COMPACT_BLAS_TRIS>(s, deviceRanges, Z, src, dst, table); break;
    case COMPACT_WORDS: launchKind<COMPACT_WORDS>(s, deviceRanges, Z, src, dst, table); break;
    case COMPACT_SHADE: launchKind<COMPACT_SHADE>(s, deviceRanges, Z, src, dst, table); break;
    case COMPACT_BLAS_NODES: launchKind<COMPACT_BLAS_NODES>(s, deviceRanges, Z, src, dst, table); break;
    case COMPACT_INSTANCES: launchKind<COMPACT_INSTANCES>(s, deviceRanges, Z, src, dst, table); break;
    case COMPACT_INST_TRAV: launchKind<COMPACT_INST_TRAV>(s, deviceRanges, Z, src, dst, table); break;
    case COMPACT_TRIS: launchKind<COMPACT_TRIS>(s, deviceRanges, Z, src, dst, table); break;
    default: return false;
  }
  return true;
}

} // namespace gi

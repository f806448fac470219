// gi_compact.h -- the per-item arithmetic of compacting the retired ranges of a resident two-level scene without the flat tree (gi_compact.hip k_compact_ranges;
// gi_build.cpp compactTwoLevel, giCDebugCompactRanges; DESIGN.md section 6 "Compaction of retired ranges"), shared by the host and the device kernel as
// gi_append.h and gi_instances.h are.  Topology and instancer edits in place leave dead ranges in every array of the scene (the records of destroyed meshes,
// the slots of retired instances).  A compaction moves what is live to the front of NEW arrays, in storage order, and rebases the indices the moved records
// hold.  One RANGE TABLE per array kind: an entry names a run of live items -- its first item in the old array, its first item in the new one, its length,
// what is added to the indices its records hold, its first workgroup.  One launch per array kind serves all its ranges.
//   Mapping (k_instance_records's): one 16-byte piece per lane, consecutive lanes hold consecutive pieces of consecutive items, a workgroup belongs to ONE
//   range and finds it by binary search over the workgroup prefix.  The face-id words are the one kind whose piece is a dword.
//   One writer per word: the destinations of a table ascend without gaps (compactRangesOk), so no two ranges share an item.  No atomics, no LDS, no fences.
//   Source and destination are different allocations: the old and the new place of a range overlap, and workgroups run in any order.
// Rebasing is uint32 addition, unconditionally, as the append rebases a BLAS (n.childBase += ...): a leaf node's childBase moves with the others, so the bytes
// are those a build's loop leaves.
#pragma once

#include <cstddef>
#include <cstdint>
#include <vector>

#include "gi_refit.h"
#include "gi_types.h"

namespace gi {

constexpr uint32_t kCompactBlock = 256; // threads of a workgroup = pieces it holds

// The array kinds.  What a move does besides copying:
//   COMPACT_VERTS (FVertex), COMPACT_BLAS_TRIS (BlasTri), COMPACT_WORDS (face-id words): nothing
//   COMPACT_SHADE (TriShade): vi[k] += delta[0], the mesh's vertex delta
//   COMPACT_BLAS_NODES (Node8): childBase += delta[0], triBase += delta[1]
//   COMPACT_INSTANCES (InstanceRec): mesh += delta[0]
//   COMPACT_INST_TRAV (InstTrav): blasRoot += delta[0]; triBase is a scene-order id and stays
//   COMPACT_TRIS (TriRec): instance += delta[0], vi[0] += delta[1] (its shading record), vi[1] and vi[2] += delta[2] (absolute vertex indices, as
//       flattenInstance leaves them); origId stays, and the lane that holds it names the record's NEW index in the id table at origId -- unless the range is
//       COMPACT_RANGE_HIDDEN: the stale ids of a hidden instance overlap live ones (gi_vispatch.h)
enum : uint32_t { COMPACT_VERTS = 0, COMPACT_BLAS_TRIS = 1, COMPACT_WORDS = 2, COMPACT_SHADE = 3, COMPACT_BLAS_NODES = 4, COMPACT_INSTANCES = 5, COMPACT_INST_TRAV = 6,
    COMPACT_TRIS = 7, COMPACT_KIND_COUNT = 8 };
constexpr uint32_t COMPACT_RANGE_HIDDEN = 1u;

struct CompactRange {
  uint32_t src, dst, count, wgFirst; // first item in the old array, in the new one; items; the range's first workgroup (prefix over compact_range_workgroups)
  uint32_t delta[3], flags;          // added to the indices the records hold (by kind, above); COMPACT_RANGE_*
};
static_assert(sizeof(CompactRange) == 32, "CompactRange: two 16-byte pieces");
// The sizes every index is checked against: items of the old array, of the new one, words of the id table (COMPACT_TRIS; 0 otherwise)
struct CompactSizes { uint32_t kind, rangeCount, srcCount, dstCount, tableCount, wgCount, pad[2]; };

static_assert(sizeof(FVertex) == 48 && sizeof(BlasTri) == 64 && sizeof(TriShade) == 160 && sizeof(Node8) == 80 && sizeof(InstanceRec) == 96 && sizeof(InstTrav) == 128 &&
    sizeof(TriRec) == 64, "compact_pieces: 16-byte pieces per record");
static_assert(offsetof(TriShade, vi) == 144 && offsetof(Node8, childBase) == 16 && offsetof(Node8, triBase) == 20 && offsetof(InstanceRec, mesh) == 84 &&
    offsetof(InstTrav, blasRoot) == 84 && offsetof(TriRec, origId) == 36 && offsetof(TriRec, instance) == 40 && offsetof(TriRec, vi) == 48,
    "compact_rebase_piece: where the indices lie");

// 16-byte pieces per item (COMPACT_WORDS: its one piece is a dword); 0: no such kind
GI_REFIT_HD inline uint32_t compact_pieces(uint32_t kind)
{
  switch (kind) {
    case COMPACT_VERTS: return 3u; case COMPACT_BLAS_TRIS: return 4u; case COMPACT_WORDS: return 1u; case COMPACT_SHADE: return 10u; case COMPACT_BLAS_NODES: return 5u;
    case COMPACT_INSTANCES: return 6u; case COMPACT_INST_TRAV: return 8u; case COMPACT_TRIS: return 4u; default: return 0u;
  }
}
GI_REFIT_HD inline uint32_t compact_piece_bytes(uint32_t kind) { return kind == COMPACT_WORDS ? 4u : 16u; }
// whole items a wave / a workgroup holds under the mapping (a Node8 has five pieces: the 13th item of a wave ends in the next one)
GI_REFIT_HD inline uint32_t compact_items_per_wave(uint32_t kind) { const uint32_t p = compact_pieces(kind); return p ? 64u / p : 0u; }
GI_REFIT_HD inline uint32_t compact_items_per_block(uint32_t kind) { const uint32_t p = compact_pieces(kind); return p ? kCompactBlock / p : 0u; }
// workgroups of a range of `count` items: ceil(count x pieces / 256); an empty range has none
GI_REFIT_HD inline uint32_t compact_range_workgroups(uint32_t kind, uint32_t count)
{
  return (uint32_t)(((uint64_t)count * compact_pieces(kind) + kCompactBlock - 1u) / kCompactBlock);
}

// The range of workgroup `wg`: the last one whose first workgroup is not behind it.  Empty ranges share their prefix with the range behind them, so the
// last of equals is the one that owns the workgroup.  The same answer in every lane of a workgroup
GI_REFIT_HD inline uint32_t compact_range_of(const CompactRange* ranges, uint32_t rangeCount, uint32_t wg)
{
  uint32_t lo = 0u, hi = rangeCount; // (ranges[lo].wgFirst <= wg < ranges[hi].wgFirst, the count standing for "past the end")
  while (hi - lo > 1u) { const uint32_t mid = lo + (hi - lo) / 2u; if (ranges[mid].wgFirst <= wg) lo = mid; else hi = mid; }
  return lo;
}

// Piece `piece` of a record of `kind` that moves with range R: the indices it holds, rebased
GI_REFIT_HD inline void compact_rebase_piece(uint32_t kind, const CompactRange& R, uint32_t piece, uint32_t w[4])
{
  if (kind == COMPACT_SHADE) { if (piece == 9u) { w[0] += R.delta[0]; w[1] += R.delta[0]; w[2] += R.delta[0]; } }
  else if (kind == COMPACT_BLAS_NODES) { if (piece == 1u) { w[0] += R.delta[0]; w[1] += R.delta[1]; } }
  else if (kind == COMPACT_INSTANCES || kind == COMPACT_INST_TRAV) { if (piece == 5u) w[1] += R.delta[0]; }
  else if (kind == COMPACT_TRIS) { if (piece == 2u) w[2] += R.delta[0]; else if (piece == 3u) { w[0] += R.delta[1]; w[1] += R.delta[2]; w[2] += R.delta[2]; } }
}

// Thread (workgroup wg, lane-in-workgroup t): one piece of one item of the range the workgroup belongs to, loaded from the old array, rebased, stored to the
// new one; the id-table word of a flat record.  `src` and `dst` must not overlap.  Every index is checked against its array's count: a "cannot happen" returns
// Piece `piece` of item `item` of range R: loaded from the old array, rebased, stored to the new one; the id-table word of a flat record
GI_REFIT_HD inline void compact_piece(const CompactRange& R, const CompactSizes& Z, uint32_t P, uint32_t item, uint32_t piece, const void* src, void* dst, uint32_t* table)
{
  if (R.src > Z.srcCount || item >= Z.srcCount - R.src || R.dst > Z.dstCount || item >= Z.dstCount - R.dst) return; // (cannot happen: the host asks compactRangesOk first)
  const size_t from = ((size_t)R.src + item) * P + piece, to = ((size_t)R.dst + item) * P + piece;
  if (Z.kind == COMPACT_WORDS) { static_cast<uint32_t*>(dst)[to] = static_cast<const uint32_t*>(src)[from]; return; }
  uint32_t w[4];
  // (records of 16-byte multiples in a hipMalloc block, a std::vector's on the host: 16-byte aligned pieces, ONE 16-byte load and store per lane)
  __builtin_memcpy(w, __builtin_assume_aligned(static_cast<const char*>(src) + 16u * from, 16), 16);
  compact_rebase_piece(Z.kind, R, piece, w);
  __builtin_memcpy(__builtin_assume_aligned(static_cast<char*>(dst) + 16u * to, 16), w, 16);
  if (Z.kind == COMPACT_TRIS && piece == 2u && !(R.flags & COMPACT_RANGE_HIDDEN) && table && w[1] < Z.tableCount) table[w[1]] = R.dst + item; // (w[1]: origId)
}
GI_REFIT_HD inline void compact_thread(const CompactRange* ranges, const CompactSizes& Z, uint32_t wg, uint32_t t, const void* src, void* dst, uint32_t* table)
{
  const uint32_t P = compact_pieces(Z.kind);
  if (Z.rangeCount == 0u || wg >= Z.wgCount || P == 0u) return;
  const CompactRange R = ranges[compact_range_of(ranges, Z.rangeCount, wg)];
  if (wg < R.wgFirst) return; // (cannot happen: the first range starts at workgroup 0)
  const uint32_t at = (wg - R.wgFirst) * kCompactBlock + t; // (a range has fewer than 2^32 pieces: compactRangesOk)
  const uint32_t item = at / P, piece = at % P;
  if (item >= R.count) return; // (past the range's last item: its last workgroup is partly filled)
  compact_piece(R, Z, P, item, piece, src, dst, table);
}

// The prefix, filled in: returns the launch's workgroups (0xffffffff: more than a launch takes)
inline uint32_t compactRangesNumber(uint32_t kind, CompactRange* ranges, uint32_t rangeCount)
{
  uint64_t wg = 0;
  for (uint32_t k = 0; k < rangeCount; k++) { ranges[k].wgFirst = (uint32_t)wg; wg += compact_range_workgroups(kind, ranges[k].count); if (wg >= (1ull << 31)) return 0xffffffffu; }
  return (uint32_t)wg;
}
// The range check, what the host asks before it launches anything: a known kind; every range inside the old array, the sources ascending without overlap
// (stable order); the destinations ascending WITHOUT GAPS from 0 to dstCount (one writer per item, every item of the new array written); the prefix the
// range sizes'; an id table only where the kind has one
inline bool compactRangesOk(const CompactRange* ranges, const CompactSizes& Z)
{
  if (compact_pieces(Z.kind) == 0u || (Z.rangeCount != 0u && !ranges) || (Z.kind != COMPACT_TRIS && Z.tableCount != 0u)) return false;
  uint64_t wg = 0, srcEnd = 0, dstEnd = 0;
  for (uint32_t k = 0; k < Z.rangeCount; k++) {
    const CompactRange& R = ranges[k];
    if (R.wgFirst != wg || R.src < srcEnd || (uint64_t)R.src + R.count > Z.srcCount || R.dst != dstEnd) return false;
    if ((uint64_t)R.count * compact_pieces(Z.kind) + kCompactBlock >= (1ull << 32)) return false;
    srcEnd = (uint64_t)R.src + R.count; dstEnd += R.count; wg += compact_range_workgroups(Z.kind, R.count);
    if (wg >= (1ull << 31)) return false;
  }
  return dstEnd == Z.dstCount && wg == Z.wgCount;
}

// The host form of the kernel, workgroups [first, last): the caller may split the range over threads (one writer per word)
inline void compactRangesHost(const CompactRange* ranges, const CompactSizes& Z, uint32_t first, uint32_t last, const void* src, void* dst, uint32_t* table)
{
  for (uint32_t wg = first; wg < last; wg++) for (uint32_t t = 0; t < kCompactBlock; t++) compact_thread(ranges, Z, wg, t, src, dst, table);
}

// The host's OWN arrays are compacted where they lie (gi_build.cpp compactTwoLevel), through the same per-piece form.  A stable compaction only moves records
// towards the front (dst <= src: compactRangesOk's ascending sources and gapless destinations), so one thread that takes the ranges, the items of a range
// and the pieces of an item in ascending order never overwrites what it has yet to read.  A range that stays where it is with nothing to rebase is not
// touched -- on a scene whose edited meshes lie at the ends of the arrays that is nearly everything --, and its flat records' id-table words are already the
// table's: `table` is the OLD table (flatOfOrig[origId] == position for every visible record, the induction every edit keeps), of which the first
// Z.tableCount words are the new one.  The caller shortens the arrays to Z.dstCount and the table to Z.tableCount
inline void compactRangesInPlaceHost(const CompactRange* ranges, const CompactSizes& Z, void* data, uint32_t* table)
{
  const uint32_t P = compact_pieces(Z.kind);
  if (P == 0u) return;
  for (uint32_t k = 0; k < Z.rangeCount; k++) {
    const CompactRange& R = ranges[k];
    if (R.dst > R.src) return; // (cannot happen: the host asks compactRangesOk first)
    if (R.dst == R.src && R.delta[0] == 0u && R.delta[1] == 0u && R.delta[2] == 0u) continue;
    for (uint32_t item = 0; item < R.count; item++) for (uint32_t piece = 0; piece < P; piece++) compact_piece(R, Z, P, item, piece, data, data, table);
  }
}

// A table under construction: runs that continue the one before them -- next in the old array, the same deltas and flags -- are joined, so a mesh's instances
// in consecutive slots are one range.  Destinations are handed out in the order of the calls (ascending sources: the caller's)
struct CompactTable {
  std::vector<CompactRange> ranges; CompactSizes Z{};
  explicit CompactTable(uint32_t kind) { Z.kind = kind; }
  uint32_t add(uint32_t src, uint32_t count, uint32_t d0 = 0u, uint32_t d1 = 0u, uint32_t d2 = 0u, uint32_t flags = 0u) // returns the run's first new index
  {
    const uint32_t dst = Z.dstCount;
    if (count == 0u) return dst;
    if (!ranges.empty()) {
      CompactRange& L = ranges.back();
      if (L.src + L.count == src && L.delta[0] == d0 && L.delta[1] == d1 && L.delta[2] == d2 && L.flags == flags) { L.count += count; Z.dstCount += count; return dst; }
    }
    ranges.push_back(CompactRange{src, dst, count, 0u, {d0, d1, d2}, flags});
    Z.dstCount += count;
    return dst;
  }
  // sizes and prefix; false: more workgroups than a launch takes, or the table does not pass its own check
  bool finish(uint32_t srcCount, uint32_t tableCount)
  {
    Z.rangeCount = (uint32_t)ranges.size(); Z.srcCount = srcCount; Z.tableCount = tableCount;
    Z.wgCount = compactRangesNumber(Z.kind, ranges.data(), Z.rangeCount);
    return Z.wgCount != 0xffffffffu && compactRangesOk(ranges.data(), Z);
  }
};

} // namespace gi

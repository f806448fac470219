// compact_ranges_sanitize.cpp -- the per-item forms of a compaction of the retired ranges of a two-level scene (gi_compact.h: what gi_compact.hip's kernel and
// gi_build.cpp compactTwoLevel's host copies run) under AddressSanitizer + UBSan, as a program of its own:
//   g++ -O1 -g -std=c++17 -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all -static-libasan -static-libubsan -Igatling_amd/csrc -Iinclude \
//       tests/cpp/compact_ranges_sanitize.cpp -o compact_ranges_sanitize && ./compact_ranges_sanitize
// For each of the eight array kinds, lists of live and dead ranges -- one live item; live ranges of W - 1 .. W + 1 and B - 1 .. B + 1 items (W, B: the items a
// wave and a workgroup hold) between dead ones; the first range dead; the last range dead; 37 alternating ranges of 7 items; a zero-length live range between
// two dead ones; nothing dead; everything dead but one item -- are held to a restatement written without the header's helpers: the records of the live ranges
// copied in order through their types, then the index fields rebased by name, and the id table written at the ids of the flat records that are not hidden.
// Every array is allocated at its exact size and the destination starts as 0xa5 bytes: a read or a store past a range is the sanitizer's to see.  The range
// check must refuse a prefix that was never made, a range past the old array, a gap or an overlap in the destinations, sources that go backwards, a wrong
// workgroup count, an id table on a kind without one and an unknown kind.  CompactTable must join runs that continue each other and keep apart those that do
// not.  The host's own form, compactRangesInPlaceHost, must leave the same records at the front of the array it is given.  Exit status 0 and "compact ranges sanitize ok" on success.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "gi_compact.h"

using namespace gi;

namespace {

int failures = 0;
void expect(bool ok, const char* what, unsigned a = 0, unsigned b = 0) { if (!ok) { if (failures < 20) printf("FAILED: %s (%u, %u)\n", what, a, b); failures++; } }

struct In { uint32_t count; bool live; uint32_t d0, d1, d2; bool hidden; };

template <class Rec> void rebaseByName(uint32_t, Rec&, const In&) {}
template <> void rebaseByName<TriShade>(uint32_t, TriShade& q, const In& r) { q.vi[0] += r.d0; q.vi[1] += r.d0; q.vi[2] += r.d0; }
template <> void rebaseByName<Node8>(uint32_t, Node8& n, const In& r) { n.childBase += r.d0; n.triBase += r.d1; }
template <> void rebaseByName<InstanceRec>(uint32_t, InstanceRec& ir, const In& r) { ir.mesh += r.d0; }
template <> void rebaseByName<InstTrav>(uint32_t, InstTrav& tv, const In& r) { tv.blasRoot += r.d0; }
template <> void rebaseByName<TriRec>(uint32_t, TriRec& t, const In& r) { t.instance += r.d0; t.vi[0] += r.d1; t.vi[1] += r.d2; t.vi[2] += r.d2; }

template <class Rec> void runCase(uint32_t kind, std::mt19937& rng, const std::vector<In>& list)
{
  expect(compact_pieces(kind) * compact_piece_bytes(kind) == sizeof(Rec), "the pieces of a record", kind);
  uint32_t total = 0, live = 0;
  for (const In& r : list) { total += r.count; if (r.live) live += r.count; }
  // --- the old array: random bytes; a flat record's id: the visible ones a permutation of [0, visible), the hidden ones anywhere inside it
  std::vector<Rec> src(total);
  for (Rec& rec : src) { unsigned char* p = reinterpret_cast<unsigned char*>(&rec); for (size_t i = 0; i < sizeof(Rec); i++) p[i] = (unsigned char)rng(); }
  if (kind == COMPACT_TRIS) {
    std::vector<uint32_t> ids;
    uint32_t at = 0, visible = 0;
    for (const In& r : list) if (r.live && !r.hidden) visible += r.count;
    for (uint32_t i = 0; i < visible; i++) ids.push_back(i);
    std::shuffle(ids.begin(), ids.end(), rng);
    uint32_t next = 0;
    for (const In& r : list) for (uint32_t i = 0; i < r.count; i++, at++) {
      TriRec t; memcpy(&t, &src[at], sizeof(t));
      t.origId = r.live && !r.hidden ? ids[next++] : (visible ? (uint32_t)rng() % visible : 0u);
      memcpy(&src[at], &t, sizeof(t));
    }
  }
  // --- the restatement: filter, then rebase
  std::vector<Rec> want; std::vector<uint32_t> wantTable(kind == COMPACT_TRIS ? live : 0u, 0xa5a5a5a5u);
  {
    std::vector<const In*> rangeOf;
    uint32_t at = 0;
    for (const In& r : list) { if (r.live) for (uint32_t i = 0; i < r.count; i++) { want.push_back(src[at + i]); rangeOf.push_back(&r); } at += r.count; }
    for (size_t i = 0; i < want.size(); i++) {
      rebaseByName<Rec>(kind, want[i], *rangeOf[i]);
      if (kind == COMPACT_TRIS && !rangeOf[i]->hidden) { TriRec t; memcpy(&t, &want[i], sizeof(t)); if (t.origId < live) wantTable[t.origId] = (uint32_t)i; }
    }
  }
  // --- the table, one entry per live range (the empty ones too)
  std::vector<CompactRange> ranges;
  CompactSizes Z{}; Z.kind = kind; Z.srcCount = total; Z.dstCount = live; Z.tableCount = kind == COMPACT_TRIS ? live : 0u;
  { uint32_t s = 0, d = 0;
    for (const In& r : list) { if (r.live) { ranges.push_back(CompactRange{s, d, r.count, 0xdeadu, {r.d0, r.d1, r.d2}, r.hidden ? COMPACT_RANGE_HIDDEN : 0u}); d += r.count; } s += r.count; } }
  Z.rangeCount = (uint32_t)ranges.size();
  bool anyWork = false; for (const CompactRange& R : ranges) anyWork = anyWork || R.count != 0u;
  expect(ranges.empty() || !compactRangesOk(ranges.data(), Z), "the range check accepts a prefix that was never made");
  Z.wgCount = compactRangesNumber(kind, ranges.data(), Z.rangeCount);
  uint32_t wantWg = 0;
  for (size_t k = 0; k < ranges.size(); k++) { expect(ranges[k].wgFirst == wantWg, "the workgroup prefix", (unsigned)k); wantWg += (ranges[k].count * compact_pieces(kind) + 255u) / 256u; }
  expect(Z.wgCount == wantWg, "the launch's workgroups", Z.wgCount, wantWg);
  expect(compactRangesOk(ranges.data(), Z), "the range check refuses ranges that fit");
  for (uint32_t wg = 0; wg < Z.wgCount; wg++) { // the search: the last range that starts at or in front of the workgroup, which is never an empty one
    uint32_t w = 0; for (uint32_t k = 0; k < Z.rangeCount; k++) if (ranges[k].wgFirst <= wg) w = k;
    expect(compact_range_of(ranges.data(), Z.rangeCount, wg) == w && ranges[w].count != 0u, "the range of a workgroup", wg, w);
  }
  if (anyWork) { // the refusals
    CompactSizes bad = Z; bad.srcCount = ranges.back().src + ranges.back().count - 1u; expect(ranges.back().count == 0u || !compactRangesOk(ranges.data(), bad), "the range check accepts a range past the old array");
    bad = Z; bad.dstCount++; expect(!compactRangesOk(ranges.data(), bad), "the range check accepts a new array with an item nobody writes");
    bad = Z; bad.dstCount--; expect(!compactRangesOk(ranges.data(), bad), "the range check accepts a new array one item short");
    bad = Z; bad.wgCount++; expect(!compactRangesOk(ranges.data(), bad), "the range check accepts a workgroup too many");
    bad = Z; bad.kind = COMPACT_KIND_COUNT; expect(!compactRangesOk(ranges.data(), bad), "the range check accepts an unknown kind");
    if (kind != COMPACT_TRIS) { bad = Z; bad.tableCount = 1u; expect(!compactRangesOk(ranges.data(), bad), "the range check accepts an id table on a kind without one"); }
    std::vector<CompactRange> moved(ranges); moved.back().dst++; expect(!compactRangesOk(moved.data(), Z), "the range check accepts a gap in the destinations");
    if (ranges.size() > 1u && ranges[1].count != 0u && ranges[0].count != 0u) {
      moved = ranges; moved[1].src = moved[0].src; expect(!compactRangesOk(moved.data(), Z), "the range check accepts sources that go backwards");
      moved = ranges; moved[1].dst--; expect(!compactRangesOk(moved.data(), Z), "the range check accepts destinations that overlap");
    }
  }
  // --- the kernel's host form: in two halves, as the host's thread pool splits the workgroups, and past the end
  std::vector<Rec> dst(live); std::vector<uint32_t> table(Z.tableCount, 0xa5a5a5a5u);
  if (live) memset(static_cast<void*>(dst.data()), 0xa5, live * sizeof(Rec));
  const uint32_t half = Z.wgCount / 2u;
  compactRangesHost(ranges.data(), Z, half, Z.wgCount, src.data(), dst.data(), table.data());
  compactRangesHost(ranges.data(), Z, 0u, half, src.data(), dst.data(), table.data());
  compactRangesHost(ranges.data(), Z, Z.wgCount, Z.wgCount + 3u, src.data(), dst.data(), table.data()); // (nothing)
  for (uint32_t i = 0; i < live; i++) expect(memcmp(&dst[i], &want[i], sizeof(Rec)) == 0, "a moved record", kind, i);
  for (uint32_t i = 0; i < Z.tableCount; i++) expect(table[i] == wantTable[i], "an id-table word", kind, i);
  // --- the host's own form: the array compacted where it lies, the table the old one (every visible record named at its OLD position), ranges that stay
  // where they are skipped; the first `live` records and the visible ids' words must be the restatement's
  {
    std::vector<Rec> inPlace(src); std::vector<uint32_t> oldTable(Z.tableCount, 0xa5a5a5a5u);
    if (kind == COMPACT_TRIS) { uint32_t at = 0; for (const In& r : list) for (uint32_t i = 0; i < r.count; i++, at++) if (r.live && !r.hidden) { TriRec t; memcpy(&t, &src[at], sizeof(t)); if (t.origId < Z.tableCount) oldTable[t.origId] = at; } }
    compactRangesInPlaceHost(ranges.data(), Z, inPlace.data(), oldTable.data());
    expect(inPlace.size() == total && (live == 0u || memcmp(inPlace.data(), want.data(), live * sizeof(Rec)) == 0), "the records compacted in place", kind);
    for (uint32_t i = 0; i < Z.tableCount; i++) expect(oldTable[i] == wantTable[i], "an id-table word behind the compaction in place", kind, i);
  }
  // --- the same ranges through CompactTable: runs that continue each other are one range, and the bytes do not change
  CompactTable T(kind);
  { uint32_t s = 0; for (const In& r : list) { if (r.live) T.add(s, r.count, r.d0, r.d1, r.d2, r.hidden ? COMPACT_RANGE_HIDDEN : 0u); s += r.count; } }
  expect(T.finish(total, Z.tableCount) && T.Z.dstCount == live && T.ranges.size() <= ranges.size(), "the table under construction");
  for (size_t k = 1; k < T.ranges.size(); k++) {
    const CompactRange& a = T.ranges[k - 1]; const CompactRange& b = T.ranges[k];
    expect(a.count != 0u && b.count != 0u && !(a.src + a.count == b.src && memcmp(a.delta, b.delta, 12) == 0 && a.flags == b.flags), "two ranges that should be one", (unsigned)k);
  }
  std::vector<Rec> dst2(live); std::vector<uint32_t> table2(Z.tableCount, 0xa5a5a5a5u);
  if (live) memset(static_cast<void*>(dst2.data()), 0xa5, live * sizeof(Rec));
  compactRangesHost(T.ranges.data(), T.Z, 0u, T.Z.wgCount, src.data(), dst2.data(), table2.data());
  expect(live == 0u || memcmp(dst2.data(), want.data(), live * sizeof(Rec)) == 0, "the joined ranges' records", kind);
  for (uint32_t i = 0; i < Z.tableCount; i++) expect(table2[i] == wantTable[i], "the joined ranges' id-table word", kind, i);
}

template <class Rec> void runKind(uint32_t kind, std::mt19937& rng)
{
  const uint32_t W = compact_items_per_wave(kind), B = compact_items_per_block(kind);
  expect(W == 64u / compact_pieces(kind) && B == 256u / compact_pieces(kind) && W >= 1u, "the items of a wave and a workgroup", W, B);
  auto L = [&](uint32_t n, uint32_t k = 1u, bool hidden = false) { return In{n, true, 0u - (k + 1u), 0u - (2u * k + 5u), 7u + 3u * k, hidden}; };
  auto D = [](uint32_t n) { return In{n, false, 0u, 0u, 0u, false}; };
  runCase<Rec>(kind, rng, {L(1)});
  for (const uint32_t n : {W - 1u, W, W + 1u, B - 1u, B, B + 1u}) runCase<Rec>(kind, rng, {D(3), L(n, 2), D(2), L(5, 3, true)});
  runCase<Rec>(kind, rng, {D(5), L(9, 1), L(4, 2)});
  runCase<Rec>(kind, rng, {L(9, 1), L(4, 2, true), D(5)});
  { std::vector<In> alt; for (uint32_t k = 0; k < 37u; k++) alt.push_back(k % 2u ? D(7) : L(7, k, k % 6u == 4u)); runCase<Rec>(kind, rng, alt); }
  runCase<Rec>(kind, rng, {L(5, 1), D(3), L(0, 2), D(4), L(6, 3)});
  runCase<Rec>(kind, rng, {In{11, true, 0, 0, 0, false}, In{300, true, 0, 0, 0, false}});
  runCase<Rec>(kind, rng, {D(200), L(1, 4), D(300)});
  runCase<Rec>(kind, rng, {L(3, 1), D(1), L(7, 2), D(2), L(1, 3)}); // (a Node8's five pieces: piece counts that are no multiple of four)
  runCase<Rec>(kind, rng, {D(4)});
  runCase<Rec>(kind, rng, {});
}

} // namespace

int main()
{
  std::mt19937 rng(24);
  runKind<FVertex>(COMPACT_VERTS, rng); runKind<BlasTri>(COMPACT_BLAS_TRIS, rng); runKind<int32_t>(COMPACT_WORDS, rng); runKind<TriShade>(COMPACT_SHADE, rng);
  runKind<Node8>(COMPACT_BLAS_NODES, rng); runKind<InstanceRec>(COMPACT_INSTANCES, rng); runKind<InstTrav>(COMPACT_INST_TRAV, rng); runKind<TriRec>(COMPACT_TRIS, rng);
  { // 2^31 workgroups are not numbered
    std::vector<CompactRange> huge(200, CompactRange{0u, 0u, 0xffffffffu / 10u, 0u, {0u, 0u, 0u}, 0u});
    expect(compactRangesNumber(COMPACT_SHADE, huge.data(), (uint32_t)huge.size()) == 0xffffffffu, "2^31 workgroups are numbered");
  }
  if (failures) { printf("%d check(s) failed\n", failures); return 1; }
  printf("compact ranges sanitize ok\n");
  return 0;
}

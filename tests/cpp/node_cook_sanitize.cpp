// node_cook_sanitize.cpp -- cook_node / cook_place (gatling_amd/csrc/gi_node_cook.h) under AddressSanitizer + UBSan, as a program of its own (built and run by
// tests/test_node_cook_host.py).  The nodes of the file named on the command line (80-byte records: cornell's with and without the leaf lift, the hand-made
// shapes) and 4000 random ones are cooked into heap buffers of exactly the image's size, so a write outside the image is an error of the run, and every record
// is held to the contract on the spot: header words copied, occupied slots first, plane bytes with their child, every table entry the decode's word.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "gi_node_cook.h"

using namespace gi;

static int g_bad = 0;
#define CHECK(c) do { if (!(c)) { if (g_bad++ < 20) fprintf(stderr, "line %d: %s (node %u)\n", __LINE__, #c, i); } } while (0)

// the word trav_node_test assembles for a child, written the way the kernel decodes it: four meta bytes at a time
static uint32_t decode_word(uint32_t m4, uint32_t k, uint32_t oct)
{
  const uint32_t oct4 = oct * 0x01010101u;
  const uint32_t inner4 = ((m4 & (m4 << 1)) >> 4) & 0x01010101u;
  const uint32_t idx4 = (m4 ^ (oct4 & ((inner4 << 8) - inner4))) & 0x1f1f1f1fu;
  const uint32_t bits4 = (m4 >> 5) & 0x07070707u;
  const uint32_t sh = 8u * k;
  return ((bits4 >> sh) & 0xffu) << ((idx4 >> sh) & 0xffu);
}

static void check_array(const std::vector<Node8>& nodes, uint32_t blocks)
{
  const uint32_t n = (uint32_t)nodes.size();
  std::vector<uint32_t> image((size_t)n * COOK_NODE_DWORDS + (size_t)blocks * COOK_OCT_DWORDS, 0u);
  for (uint32_t i = 0; i < n; i++) cook_place(nodes.data(), i, n, blocks, image.data());
  uint32_t innerSeen = 0;
  for (uint32_t i = 0; i < n; i++) {
    uint32_t w[20];
    memcpy(w, &nodes[i], sizeof(w));
    const uint32_t* rec = &image[(size_t)i * COOK_NODE_DWORDS];
    uint32_t occupied = 0; bool inner = false;
    for (uint32_t s = 0; s < 8u; s++) { const uint32_t m = cook_meta(w, s); occupied += m != 0u; inner = inner || cook_meta_inner(m); }
    const bool placed = inner && innerSeen < blocks;
    for (uint32_t k = 0; k < 6u; k++) CHECK(rec[k] == w[k]);
    CHECK((rec[6] >> 16) == ((occupied + 1u) & ~1u));
    CHECK((rec[6] & 0xffffu) == (placed ? COOK_OCT_MASK : 0u));
    const uint32_t* tables = placed ? &image[(size_t)n * COOK_NODE_DWORDS + (size_t)innerSeen * COOK_OCT_DWORDS] : rec + COOK_TABLE_AT;
    CHECK(reinterpret_cast<const char*>(rec) + rec[7] == reinterpret_cast<const char*>(tables));
    // child k of the record is the k-th occupied slot (then the empty ones)
    uint32_t perm[8], c = 0;
    for (uint32_t s = 0; s < 8u; s++) if (cook_meta(w, s) != 0u) perm[c++] = s;
    for (uint32_t s = 0; s < 8u; s++) if (cook_meta(w, s) == 0u) perm[c++] = s;
    const uint8_t* planes = reinterpret_cast<const uint8_t*>(rec + 8);
    const uint8_t* from = reinterpret_cast<const uint8_t*>(w + 8);
    for (uint32_t p = 0; p < 6u; p++) for (uint32_t k = 0; k < 8u; k++) CHECK(planes[p * 8u + k] == from[p * 8u + perm[k]]);
    for (uint32_t o = 0; o < (placed ? 8u : 1u); o++)
      for (uint32_t k = 0; k < 8u; k++) CHECK(tables[o * COOK_TABLE_DWORDS + k] == decode_word(w[6u + (perm[k] >> 2)], perm[k] & 3u, placed ? o : 0u));
    if (!inner) for (uint32_t o = 1; o < 8u; o++) for (uint32_t k = 0; k < 8u; k++) CHECK(decode_word(w[6u + (perm[k] >> 2)], perm[k] & 3u, o) == rec[COOK_TABLE_AT + k]);
    if (placed) innerSeen++;
  }
}

int main(int argc, char** argv)
{
  std::vector<Node8> given;
  if (argc > 1) {
    FILE* f = fopen(argv[1], "rb");
    if (!f) { fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
    Node8 nd;
    while (fread(&nd, sizeof(nd), 1, f) == 1) given.push_back(nd);
    fclose(f);
  }
  if (!given.empty()) {
    check_array(given, (uint32_t)given.size());
    check_array(given, cook_oct_blocks_max((uint32_t)given.size()));
    check_array(given, 0u); // no octant area at all: every record stays inside its 112 bytes
    for (size_t k = 0; k < given.size(); k++) check_array(std::vector<Node8>(1, given[k]), 1u);
  }
  std::mt19937 rng(20250u);
  std::vector<Node8> random(4000);
  for (Node8& nd : random) {
    uint32_t w[20];
    for (uint32_t& x : w) x = rng();
    memcpy(&nd, w, sizeof(nd));
    uint32_t off = 0;
    nd.imask = 0;
    for (uint32_t s = 0; s < 8u; s++) {
      const uint32_t kind = rng() & 3u;
      if (kind == 0u) nd.meta[s] = 0;
      else if (kind == 1u) { nd.meta[s] = (uint8_t)((1u << 5) | (24u + s)); nd.imask |= (uint8_t)(1u << s); }
      else { const uint32_t cnt = 1u + rng() % 3u; nd.meta[s] = (uint8_t)((((1u << cnt) - 1u) << 5) | off); off += cnt; }
    }
  }
  check_array(random, (uint32_t)random.size());
  check_array(random, cook_oct_blocks_max((uint32_t)random.size()));
  for (uint32_t first = 0; first + 64u <= (uint32_t)random.size(); first += 64u) // blocks of 64, as the device check stages them
    check_array(std::vector<Node8>(random.begin() + first, random.begin() + first + 64), 64u);
  printf("%zu given nodes, %zu random nodes\n", given.size(), random.size());
  if (g_bad) { printf("%d check(s) failed\n", g_bad); return 1; }
  printf("node cook sanitize ok\n");
  return 0;
}

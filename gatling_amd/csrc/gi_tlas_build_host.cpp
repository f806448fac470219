// gi_tlas_build_host.cpp -- the host form of the device TLAS builder (gi_tlas_build.h): every stage of gi_tlas_build.hip in plain C++ over the shared
// arithmetic of gi_bvh_stages.h, pass by pass and level by level in the device's order, so that the two produce the same bytes (giCDebugBuildTlas).
#include <algorithm>
#include <numeric>

#include "gi_tlas_build.h"
#include "gi_bvh_stages.h"

namespace gi {

int buildTlasHost(const float* boxes6, size_t n, uint32_t budget, uint32_t radius, std::vector<Node8>& nodes, std::vector<uint32_t>& items, TlasBuildInfo& info)
{
  return buildBoxTreeHost(boxes6, n, budget, radius, kTlasBuildLimits, nodes, items, info);
}

int buildBoxTreeHost(const float* boxes6, size_t n, uint32_t budget, uint32_t radius, const BoxBuildLimits& limits, std::vector<Node8>& nodes,
    std::vector<uint32_t>& items, TlasBuildInfo& info)
{
  info = TlasBuildInfo{}; nodes.clear(); items.clear();
  if (n > limits.maxItems) { info.error = "more items than the builder is sized for"; return TLAS_BUILD_ERROR; }
  budget = std::min(std::min(budget, limits.maxBudget), kBoxBuildMaxLevels); radius = std::min(std::max(radius, 1u), 256u);
  if (budget == 0u) return TLAS_BUILD_TOO_DEEP;
  const uint32_t layers = budget + 1u;
  // ---- 1. active items, centroid bounds
  std::vector<uint8_t> active(n, 0); uint32_t A = 0;
  float cl[3] = {3.0e38f, 3.0e38f, 3.0e38f}, chh[3] = {-3.0e38f, -3.0e38f, -3.0e38f};
  for (size_t i = 0; i < n; i++) {
    const float* b = boxes6 + 6 * i;
    if (!tlas_box_active(b)) continue;
    active[i] = 1; A++;
    for (int a = 0; a < 3; a++) { const float c = 0.5f * (b[a] + b[3 + a]); cl[a] = refit_min(cl[a], c); chh[a] = refit_max(chh[a], c); }
  }
  info.active = A;
  // ---- 2. Morton codes, stable sort (inactive: all ones, behind in input order)
  std::vector<uint64_t> keys(n); std::vector<uint32_t> sorted(n);
  for (size_t i = 0; i < n; i++) {
    const float* b = boxes6 + 6 * i;
    const float c[3] = {0.5f * (b[0] + b[3]), 0.5f * (b[1] + b[4]), 0.5f * (b[2] + b[5])};
    keys[i] = active[i] ? bvh_morton63(c, cl, chh) : ~0ull;
  }
  std::iota(sorted.begin(), sorted.end(), 0u);
  std::stable_sort(sorted.begin(), sorted.end(), [&](uint32_t a, uint32_t b) { return keys[a] < keys[b]; });
  if (A == 0u) {
    Node8 root; bvh_empty_root(root); nodes.push_back(root); items = sorted;
    info.nodeCount = 1; info.maxDepth = 1; info.levelStart[0] = 0u; info.levelStart[1] = 1u;
    return TLAS_BUILD_OK;
  }
  // ---- 3. PLOC, 4. the depth-bounded DP inside the merge
  const uint32_t nodes2 = 2u * A - 1u;
  std::vector<float> box(6u * (size_t)nodes2); std::vector<uint32_t> left(nodes2, 0u), right(nodes2, 0u), total(nodes2, 0u);
  std::vector<Dp> dp((size_t)nodes2 * layers);
  std::vector<uint32_t> cl0(A), cl1(A), nn(A); std::vector<uint64_t> flags(A);
  for (uint32_t k = 0; k < A; k++) {
    const float* b = boxes6 + 6u * (size_t)sorted[k];
    for (int a = 0; a < 6; a++) box[6u * (size_t)k + a] = b[a];
    total[k] = 1u; cl0[k] = k;
    bvh_dp_leaf_bounded(&dp[(size_t)k * layers], layers, tlas_box_area(b));
  }
  uint32_t m = A, nodeBase = A, passes = 0;
  uint32_t* cur = cl0.data(); uint32_t* nxt = cl1.data();
  while (m > 1u) {
    for (uint32_t i = 0; i < m; i++) {
      const float* bi = &box[6u * (size_t)cur[i]];
      const uint32_t j0 = i > radius ? i - radius : 0u, j1 = std::min(m - 1u, i + radius);
      float bestD = 3.4e38f; uint32_t bestH = 0xffffffffu, best = 0xffffffffu;
      for (uint32_t j = j0; j <= j1; j++) { if (j == i) continue; bvh_nn_consider(i, j, tlas_union_area(bi, &box[6u * (size_t)cur[j]]), bestD, bestH, best); }
      nn[i] = best;
    }
    uint32_t merges = 0, keeps = 0;
    for (uint32_t i = 0; i < m; i++) { const uint32_t j = nn[i]; flags[i] = bvh_ploc_flags(i, j, j < m && nn[j] == i); }
    for (uint32_t i = 0; i < m; i++) {
      const uint64_t f = flags[i];
      if (!(f & 1ull)) continue;
      if (!(f >> 32)) { nxt[keeps++] = cur[i]; continue; }
      const uint32_t node = nodeBase + merges++;
      tlas_merge_node(box.data(), left.data(), right.data(), total.data(), dp.data(), layers, node, cur[i], cur[nn[i]]);
      nxt[keeps++] = node;
    }
    if (merges == 0u || nodeBase + merges > nodes2) { info.error = "PLOC made no progress"; return TLAS_BUILD_ERROR; }
    nodeBase += merges; m = keeps; std::swap(cur, nxt); passes++;
  }
  info.passes = passes;
  const uint32_t root2 = cur[0];
  const TlasTree2 T{box.data(), left.data(), right.data(), total.data(), dp.data(), A, layers};
  if (!tlas_root_feasible(T, root2)) return TLAS_BUILD_TOO_DEEP;
  // ---- 5. emission, one breadth-first level at a time
  items.assign(n, 0u);
  std::vector<uint32_t> level{root2}, next; std::vector<Plan> plans; std::vector<uint64_t> counts;
  uint32_t levelStart = 0, itemCount = 0, levels = 0;
  nodes.resize(1);
  while (!level.empty()) {
    if (levels == budget) { info.error = "emission outgrew the depth budget"; return TLAS_BUILD_ERROR; } // (cannot happen: the DP bounds the depth)
    const uint32_t mm = (uint32_t)level.size(), nodeEnd = levelStart + mm;
    plans.resize(mm); counts.resize(mm);
    uint32_t internal = 0, itemsHere = 0;
    for (uint32_t li = 0; li < mm; li++) { tlas_plan_node(T, level[li], levels == 0u, budget - levels, plans[li], counts[li]);
        internal += (uint32_t)(counts[li] >> 32); itemsHere += (uint32_t)(counts[li] & 0xffffffffull); }
    if (itemCount + itemsHere > A) { info.error = "emission outgrew its bounds"; return TLAS_BUILD_ERROR; }
    nodes.resize((size_t)nodeEnd + internal); next.assign(internal, 0u);
    uint32_t childBase = nodeEnd, itemBase = itemCount;
    for (uint32_t li = 0; li < mm; li++) {
      tlas_write_node(T, plans[li], childBase, itemBase, nodeEnd, sorted.data(), nodes[(size_t)levelStart + li], items.data(), next.data());
      childBase += (uint32_t)(counts[li] >> 32); itemBase += (uint32_t)(counts[li] & 0xffffffffull);
    }
    info.levelStart[levels] = levelStart;
    levelStart = nodeEnd; itemCount += itemsHere; levels++;
    level.swap(next);
  }
  if (itemCount != A) { info.error = "emission lost items"; return TLAS_BUILD_ERROR; }
  for (size_t k = A; k < n; k++) items[k] = sorted[k];
  info.nodeCount = (uint32_t)nodes.size(); info.maxDepth = levels; info.levelStart[levels] = (uint32_t)nodes.size();
  return TLAS_BUILD_OK;
}

} // namespace gi

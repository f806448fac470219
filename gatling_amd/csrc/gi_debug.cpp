// gi_debug.cpp -- giCTraceRays and the debug / self-check entry points
// (one of the translation units gi_c.cpp was split into in round 6; shared declarations: gi_host.h)
#include "gi_host.h"
#include "gi_refit.h"
#include "gi_tlas_build.h"
#include "gi_blas.h"
#include "gi_blas_build.h"
#include "gi_bvh_stages.h"
#include "gi_compact.h"
#include "gi_moments.h"
#include "gi_node_cook.h"
#include "bvh8.h"

// ---------------------------------------------------------------------------------------------------------------
// giCTraceRays: closest hits through the device traversal kernel (parity tests of the BVH8 path)
// ---------------------------------------------------------------------------------------------------------------
static int giCTraceRaysImpl(GiCScene* s, uint32_t count, const float* origins, const float* dirs, float tMin, float tMax, float* outTUV, int32_t* outInstPrim);
extern "C" int giCTraceRays(GiCScene* s, uint32_t count, const float* origins, const float* dirs, float tMin, float tMax, float* outTUV, int32_t* outInstPrim)
{
  try { return giCTraceRaysImpl(s, count, origins, dirs, tMin, tMax, outTUV, outInstPrim); }
  catch (const std::exception& e) { setError(std::string("giCTraceRays: ") + e.what()); return -1; }
}
static int giCTraceRaysImpl(GiCScene* s, uint32_t count, const float* origins, const float* dirs, float tMin, float tMax, float* outTUV, int32_t* outInstPrim)
{
  if (!g_ctx.initialized || !s || (count && (!origins || !dirs || !outTUV || !outInstPrim))) { setError("giCTraceRays: bad arguments"); return -1; }
  if (count == 0) return 0;
  std::lock_guard<std::mutex> guard(s->mutex);
  hipStream_t st = g_ctx.stream;
  if (syncSceneGeometry(s) != GI_C_OK) return -1;
  // the render loop's grids: k_trace_dyn (scenes beyond LDS) is persistent per wave and wants every resident wave slot filled (8 blocks per CU offered)
  const bool inLds = sceneFitsLds(s->nodeCount, s->triCount);
  const uint32_t blocks = std::min<uint32_t>((count + 255u) / 256u, (uint32_t)g_ctx.cuCount * (inLds ? 3u : 8u));
  if (ensurePathState(s, count, blocks, blocks) != GI_C_OK) return -1;
  // ray records go straight into the TRACE_A queue (segment k holds rays [k*per, (k+1)*per))
  const size_t qn = (size_t)s->queueCap * NSHARD;
  std::vector<uint32_t> qslot(qn, 0u); std::vector<F4> qa(qn), qb(qn);
  Counters c{};
  const uint32_t per = (count + NSHARD - 1u) / NSHARD;
  for (uint32_t k = 0; k < NSHARD; k++) { uint32_t lo = k * per; c.count[Q_TRACE_A][k].v = lo < count ? std::min(per, count - lo) : 0u; }
  for (uint32_t i = 0; i < count; i++) {
    size_t r = (size_t)(i / per) * s->queueCap + (i % per);
    qslot[r] = i;
    qa[r] = F4{origins[3 * i], origins[3 * i + 1], origins[3 * i + 2], tMin};
    qb[r] = F4{dirs[3 * i], dirs[3 * i + 1], dirs[3 * i + 2], tMax};
  }
  if (hipMemcpyAsync(s->qSlot[Q_TRACE_A].ptr, qslot.data(), qn * 4, hipMemcpyHostToDevice, st) != hipSuccess ||
      hipMemcpyAsync(s->qA[Q_TRACE_A].ptr, qa.data(), qn * sizeof(F4), hipMemcpyHostToDevice, st) != hipSuccess ||
      hipMemcpyAsync(s->qB[Q_TRACE_A].ptr, qb.data(), qn * sizeof(F4), hipMemcpyHostToDevice, st) != hipSuccess ||
      hipMemcpyAsync(s->dCounters.ptr, &c, sizeof(c), hipMemcpyHostToDevice, st) != hipSuccess) { setError("giCTraceRays: upload failed"); return -1; }
  // Cut-out materials: the any-hit test of a closest-hit walk draws from the path's random state, which it reads from the ray's Slot -- here slot i of a pool no
  // path has written (or that an earlier render left behind).  The rays of this entry point carry the state 0, like the oracle's (found by tests/fuzz_parity.py:
  // a quarter of the random scenes with cut-outs answered giCTraceRays with other triangles than the oracle, and not the same ones twice).
  if (hipMemsetAsync(s->slots.ptr, 0, (size_t)count * sizeof(Slot), st) != hipSuccess) { setError("giCTraceRays: clearing the slots failed"); return -1; }
  PathState ps{s->slots.ptr, nullptr, 0u, nullptr, 0u, nullptr};
  // (no TRACE_FRESH entries: the uniforms are not read)
  launchTrace(st, blocks, false, false, makeView(s), ps, makeQueueSet(s), s->dCounters.ptr, Q_TRACE_A, Q_REGEN_B, traceDynRefill(s), blocks, FrameUniforms{},
      nullptr);
  std::vector<TriRec> tris(s->triCount);
  if (hipMemcpyAsync(&c, s->dCounters.ptr, sizeof(c), hipMemcpyDeviceToHost, st) != hipSuccess ||
      (s->triCount && hipMemcpyAsync(tris.data(), s->dTris.ptr, s->triCount * sizeof(TriRec), hipMemcpyDeviceToHost, st) != hipSuccess) ||
      hipStreamSynchronize(st) != hipSuccess) { setError("giCTraceRays: readback failed"); return -1; }
  std::vector<F4> hit(count, F4{tMax, 0.0f, 0.0f, 0.0f});
  for (uint32_t i = 0; i < count; i++) { uint32_t m = 0xffffffffu; memcpy(&hit[i].w, &m, 4); }
  // results stay in the ray records (a = t, u, v, triangle | class << 28); the class queues hold their indices
  std::vector<uint32_t> hitIdx(qn);
  if (hipMemcpy(qa.data(), s->qA[Q_TRACE_A].ptr, qn * sizeof(F4), hipMemcpyDeviceToHost) != hipSuccess) {
    setError("giCTraceRays: readback failed");
    return -1;
  }
  for (uint32_t klass = 0; klass < MAT_CLASS_COUNT; klass++) {
    if (hipMemcpy(hitIdx.data(), s->qSlot[Q_HIT + klass].ptr, qn * 4, hipMemcpyDeviceToHost) != hipSuccess) {
      setError("giCTraceRays: readback failed");
      return -1;
    }
    for (uint32_t k = 0; k < NSHARD; k++)
      for (uint32_t j = 0; j < c.count[Q_HIT + klass][k].v; j++) {
        const uint32_t ri = hitIdx[(size_t)k * s->queueCap + j] & 0x3fffffffu;
        if (ri < qn && qslot[ri] < count) { F4 h = qa[ri]; uint32_t w; memcpy(&w, &h.w, 4); w &= 0x0fffffffu; memcpy(&h.w, &w, 4); hit[qslot[ri]] = h; }
      }
  }
  int hits = 0;
  for (uint32_t i = 0; i < count; i++) {
    uint32_t tri; memcpy(&tri, &hit[i].w, 4);
    outTUV[3 * i] = hit[i].x; outTUV[3 * i + 1] = hit[i].y; outTUV[3 * i + 2] = hit[i].z;
    if (tri == 0xffffffffu || tri >= s->triCount) { outInstPrim[2 * i] = -1; outInstPrim[2 * i + 1] = -1; }
    else { outInstPrim[2 * i] = (int32_t)tris[tri].instance; outInstPrim[2 * i + 1] = (int32_t)tris[tri].prim; hits++; }
  }
  return hits;
}

// ---------------------------------------------------------------------------------------------------------------
// giCDebugValidateBvh: host-only check of the builder's conservativeness contract
// ---------------------------------------------------------------------------------------------------------------
// `left`: per record, nonzero where the record belongs to a part that was left out of the top tree (a hidden or retired mesh of a partitioned scene): no leaf
// may reference it, and its id -- stale, never read -- is not one of the `triCount` live ones
static int validateTree(const std::vector<Node8>& nodes, const std::vector<TriRec>& trisArr, uint32_t triCount, const std::vector<uint8_t>* left = nullptr)
{
  int violations = 0;
  std::vector<uint8_t> seen(triCount, 0);
  struct Item { uint32_t node; float lo[3], hi[3]; };
  std::vector<Item> stack;
  Item root; root.node = 0; for (int a = 0; a < 3; a++) { root.lo[a] = -3.0e38f; root.hi[a] = 3.0e38f; }
  stack.push_back(root);
  while (!stack.empty()) {
    Item it = stack.back(); stack.pop_back();
    if (it.node >= nodes.size()) { violations++; continue; }
    const Node8& n = nodes[it.node];
    uint32_t rel = 0;
    for (int s = 0; s < 8; s++) {
      uint8_t meta = n.meta[s];
      if (meta == 0) { if (n.imask & (1u << s)) violations++; continue; }
      float lo[3], hi[3];
      for (int a = 0; a < 3; a++) {
        uint32_t eb = (uint32_t)n.e[a] << 23; float scale; memcpy(&scale, &eb, 4);
        lo[a] = n.p[a] + (float)n.qlo[a][s] * scale; hi[a] = n.p[a] + (float)n.qhi[a][s] * scale;
      }
      bool inner = (n.imask >> s) & 1u;
      if (inner) {
        if ((meta >> 5) != 1u || (meta & 31u) != 24u + (uint32_t)s) violations++;
        Item c; c.node = n.childBase + rel; rel++;
        for (int a = 0; a < 3; a++) { c.lo[a] = lo[a]; c.hi[a] = hi[a]; }
        // every triangle below must also be inside all ancestors: intersect the constraint boxes
        for (int a = 0; a < 3; a++) { c.lo[a] = std::max(c.lo[a], it.lo[a]); c.hi[a] = std::min(c.hi[a], it.hi[a]); }
        stack.push_back(c);
      } else {
        uint32_t unary = meta >> 5, off = meta & 31u, cnt = unary == 1u ? 1u : unary == 3u ? 2u : unary == 7u ? 3u : 0u;
        if (cnt == 0u || off + cnt > 24u) { violations++; continue; }
        for (uint32_t k = 0; k < cnt; k++) {
          uint32_t ti = n.triBase + off + k;
          if (ti >= trisArr.size() || (left && (*left)[ti])) { violations++; continue; }
          const TriRec& t = trisArr[ti];
          if (t.origId >= triCount || seen[t.origId]) { violations++; continue; }
          seen[t.origId] = 1;
          for (int v = 0; v < 3; v++)
            for (int a = 0; a < 3; a++) {
              float x = t.v0[a] + (v == 1 ? t.e1[a] : v == 2 ? t.e2[a] : 0.0f);
              float blo = std::max(lo[a], it.lo[a]), bhi = std::min(hi[a], it.hi[a]);
              if (x < blo || x > bhi) violations++;
            }
        }
      }
    }
  }
  // every active triangle sits in exactly one leaf; an inactive one (bvh8.h: a vertex that is not finite or beyond 1e18) in none
  std::vector<uint8_t> inactive(triCount, 0);
  for (size_t i = 0; i < trisArr.size(); i++) {
    const TriRec& t = trisArr[i];
    if (left && (*left)[i]) continue;
    if (t.origId >= triCount) { violations++; continue; }
    for (int a = 0; a < 3; a++) {
      const float x0 = t.v0[a], x1 = t.v0[a] + t.e1[a], x2 = t.v0[a] + t.e2[a];
      if (!(std::fabs(x0) <= 1.0e18f) || !(std::fabs(x1) <= 1.0e18f) || !(std::fabs(x2) <= 1.0e18f)) inactive[t.origId] = 1;
    }
  }
  for (uint32_t i = 0; i < triCount; i++) if ((seen[i] != 0) == (inactive[i] != 0)) violations++;
  return violations;
}

extern "C" int giCDebugValidateBvh(const float* triVerts, uint32_t triCount, uint32_t* outNodeCount, uint32_t* outMaxDepth)
{
  if (triCount && !triVerts) return -1;
  std::vector<TriRec> tris(triCount);
  for (uint32_t i = 0; i < triCount; i++) {
    const float* p = triVerts + 9 * (size_t)i;
    for (int a = 0; a < 3; a++) { tris[i].v0[a] = p[a]; tris[i].e1[a] = p[3 + a] - p[a]; tris[i].e2[a] = p[6 + a] - p[a]; }
    tris[i].instance = 0; tris[i].prim = i; tris[i].origId = i;
  }
  Bvh8 bvh; buildBvh8(tris, bvh);
  if (outNodeCount) *outNodeCount = (uint32_t)bvh.nodes.size();
  if (outMaxDepth) *outMaxDepth = bvh.maxDepth;
  return validateTree(bvh.nodes, bvh.tris, triCount);
}

// giCDebugLeafLift / giCDebugSceneLeafLift: the leaf lift of small flat trees (leaf_lift.cpp; gi_build.cpp buildScene).  Host only.
extern "C" int giCDebugLeafLift(const float* triVerts, uint32_t triCount, int32_t mode, const void* treeNodes, uint32_t treeNodeCount, uint32_t treeDepth,
    void* outNodes, uint32_t nodeCap, uint32_t* outOrder, uint32_t* outInfo, double* outCost)
{
  if ((triCount && (!triVerts || !outOrder)) || !outNodes || !outInfo || !outCost || (treeNodes && treeNodeCount == 0u)) return -1;
  std::vector<TriRec> tris(triCount);
  for (uint32_t i = 0; i < triCount; i++) {
    const float* p = triVerts + 9 * (size_t)i;
    for (int a = 0; a < 3; a++) { tris[i].v0[a] = p[a]; tris[i].e1[a] = p[3 + a] - p[a]; tris[i].e2[a] = p[6 + a] - p[a]; }
    tris[i].instance = 0; tris[i].prim = i; tris[i].origId = i;
  }
  Bvh8 bvh;
  if (treeNodes) { // a tree of the caller's making: every triangle is taken as referenced, the level table is derived from the child indices
    bvh.nodes.resize(treeNodeCount); memcpy(bvh.nodes.data(), treeNodes, (size_t)treeNodeCount * sizeof(Node8));
    bvh.tris = tris; bvh.activeTris = triCount; bvh.maxDepth = treeDepth;
    std::vector<uint32_t> depth(treeNodeCount, 0u); depth[0] = 1u;
    for (uint32_t i = 0; i < treeNodeCount; i++) {
      const uint32_t internal = (uint32_t)__builtin_popcount(bvh.nodes[i].imask);
      for (uint32_t k = 0; k < internal; k++) {
        const uint64_t c = (uint64_t)bvh.nodes[i].childBase + k;
        if (c <= i || c >= treeNodeCount || depth[i] == 0u) return -1;
        depth[c] = depth[i] + 1u;
      }
    }
    for (uint32_t i = 0; i < treeNodeCount; i++) if (depth[i] == 0u || depth[i] > treeDepth || (i && depth[i] < depth[i - 1u])) return -1;
    for (uint32_t i = 0; i < treeNodeCount; i++) if (i == 0u || depth[i] != depth[i - 1u]) bvh.levelStart.push_back(i);
    bvh.levelStart.push_back(treeNodeCount);
  } else buildBvh8(tris, bvh);
  outCost[0] = bvh8ModelCost(bvh.nodes);
  const std::vector<uint32_t> levels = bvh.levelStart;
  uint32_t lifted = 0u;
  // -1: the scene build's rule but the layout (no scene here: a flat tree by construction)
  const bool run = mode == 1 || (mode < 0 && optionValue("leaf_lift", LEAF_LIFT_DEFAULT) != 0 && sceneFitsLds(bvh.nodes.size(), bvh.tris.size()));
  if (run) lifted = liftLeafSlots(bvh);
  outCost[1] = bvh8ModelCost(bvh.nodes);
  if (bvh.nodes.size() > nodeCap) return -2;
  if (bvh.levelStart != levels || bvh.tris.size() != triCount) return -3; // (the pass leaves the level table and the record count alone)
  memcpy(outNodes, bvh.nodes.data(), bvh.nodes.size() * sizeof(Node8));
  for (uint32_t i = 0; i < triCount; i++) outOrder[i] = bvh.tris[i].origId;
  outInfo[0] = (uint32_t)bvh.nodes.size(); outInfo[1] = bvh.maxDepth; outInfo[2] = lifted; outInfo[3] = bvh.activeTris;
  return validateTree(bvh.nodes, bvh.tris, triCount);
}

extern "C" int giCDebugSceneLeafLift(const GiCScene* scene, uint32_t* out)
{
  GiCScene* s = const_cast<GiCScene*>(scene);
  if (!s || !out) { setError("giCDebugSceneLeafLift: bad arguments"); return GI_C_ERROR; }
  std::lock_guard<std::mutex> guard(s->mutex);
  out[0] = s->liftedLeafSlots;
  out[1] = s->host && !s->host->treeless ? s->host->bvh.maxDepth : 0u;
  return GI_C_OK;
}

// giCDebugBvhStackReach: the ordered walk of gi_traversal.h (trav_node_pick / trav_pop: a node's hit internal children in octant-flipped slot order, highest
// bit first, the rest pushed) over the host-built tree, boxes only -- how many stack entries a ray's walk holds at most.  Nothing is culled: no triangle is
// tested, so the distance never shrinks and every internal child whose box the ray meets counts; the box test is the device's with a wider margin (a box the
// device accepts by rounding is accepted here).  The result is therefore an UPPER bound on what a device walk of that ray holds, and exact for a ray that hits
// no triangle.  Host only.
extern "C" int giCDebugBvhStackReach(const float* triVerts, uint32_t triCount, const float* origins, const float* dirs, uint32_t rayCount, uint32_t* out)
{
  if (!out || (triCount && !triVerts) || (rayCount && (!origins || !dirs))) return -1;
  std::vector<TriRec> tris(triCount);
  for (uint32_t i = 0; i < triCount; i++) {
    const float* p = triVerts + 9 * (size_t)i;
    for (int a = 0; a < 3; a++) { tris[i].v0[a] = p[a]; tris[i].e1[a] = p[3 + a] - p[a]; tris[i].e2[a] = p[6 + a] - p[a]; }
    tris[i].instance = 0; tris[i].prim = i; tris[i].origId = i;
  }
  Bvh8 bvh; buildBvh8(tris, bvh);
  const std::vector<Node8>& nodes = bvh.nodes;
  out[0] = bvh.maxDepth; out[1] = (uint32_t)nodes.size();
  std::vector<std::pair<uint32_t, uint32_t>> stack; // (first child, unvisited hit internal children in bits 24-31 | the node's internal-child mask)
  for (uint32_t r = 0; r < rayCount; r++) {
    double o[3], inv[3]; uint32_t oct = 0u;
    for (int a = 0; a < 3; a++) {
      o[a] = origins[3 * (size_t)r + a];
      const float d = dirs[3 * (size_t)r + a];
      inv[a] = 1.0 / (std::fabs(d) < 1e-30f ? (d < 0.0f ? -1e-30 : 1e-30) : (double)d); // (walk_set_ray's guard)
      if (d >= 0.0f) oct |= 1u << a;
    }
    stack.clear();
    uint32_t high = 0u;
    std::pair<uint32_t, uint32_t> G(0u, 0x80000000u); // virtual group holding only the root
    for (;;) {
      if (G.second & 0xff000000u) {
        const uint32_t bit = 31u - (uint32_t)__builtin_clz(G.second & 0xff000000u);
        G.second &= ~(1u << bit);
        if (G.second & 0xff000000u) { stack.push_back(G); high = std::max(high, (uint32_t)stack.size()); }
        const uint32_t slot = (bit - 24u) ^ oct;
        const uint32_t nodeIdx = G.first + (uint32_t)__builtin_popcount((G.second & 0xffu) & ((1u << slot) - 1u));
        if (nodeIdx >= nodes.size()) return -1;
        const Node8& n = nodes[nodeIdx];
        uint32_t hit = 0u;
        for (uint32_t s = 0; s < 8u; s++) {
          if (!((n.imask >> s) & 1u)) continue;
          double tn = 0.0, tf = 3.0e38;
          for (int a = 0; a < 3; a++) {
            const uint32_t eb = (uint32_t)n.e[a] << 23; float scale; memcpy(&scale, &eb, 4);
            const double t0 = (((double)n.p[a] + (double)n.qlo[a][s] * (double)scale) - o[a]) * inv[a];
            const double t1 = (((double)n.p[a] + (double)n.qhi[a][s] * (double)scale) - o[a]) * inv[a];
            tn = std::max(tn, std::min(t0, t1)); tf = std::min(tf, std::max(t0, t1));
          }
          if (tn * (1.0 - 1.0e-4) <= tf * (1.0 + 1.0e-4)) hit |= 1u << (24u + (s ^ oct));
        }
        G = std::make_pair(n.childBase, hit | (uint32_t)n.imask);
      }
      if (!(G.second & 0xff000000u)) {
        if (stack.empty()) break;
        G = stack.back(); stack.pop_back();
      }
    }
    out[2 + (size_t)r] = high;
  }
  return 0;
}

// The same check for the PARTITIONED layout of incremental updates: the triangles are cut into `partCount` consecutive ranges, every range gets its own
// subtree in its own node range, and a top tree over the subtree roots (buildTopBvh8) joins them.  Returns the violations of the assembled tree.
extern "C" int giCDebugValidatePartitionedBvh(const float* triVerts, uint32_t triCount, uint32_t partCount, uint32_t* outNodeCount, uint32_t* outMaxDepth)
{
  if (!triVerts || triCount == 0 || partCount == 0 || partCount > triCount) return -1;
  const uint32_t topCap = partCount * 2u + 16u;
  std::vector<Node8> nodes(topCap, Node8{}); std::vector<TriRec> trisAll(triCount);
  std::vector<float> boxes(6 * (size_t)partCount); std::vector<Node8> roots(partCount);
  uint32_t subDepth = 0;
  for (uint32_t pi = 0; pi < partCount; pi++) {
    const uint32_t first = (uint32_t)((uint64_t)triCount * pi / partCount), end = (uint32_t)((uint64_t)triCount * (pi + 1) / partCount);
    std::vector<TriRec> tris(end - first);
    for (uint32_t i = first; i < end; i++) {
      const float* p = triVerts + 9 * (size_t)i; TriRec& t = tris[i - first];
      for (int a = 0; a < 3; a++) { t.v0[a] = p[a]; t.e1[a] = p[3 + a] - p[a]; t.e2[a] = p[6 + a] - p[a]; }
      t.instance = pi; t.prim = i - first; t.origId = i - first;
    }
    Bvh8 b; buildBvh8(tris, b);
    const uint32_t off = (uint32_t)nodes.size();
    for (Node8 n : b.nodes) { n.childBase += off; n.triBase += first; nodes.push_back(n); }
    for (uint32_t k = 0; k < end - first; k++) { TriRec t = b.tris[k]; t.origId += first; trisAll[first + k] = t; }
    roots[pi] = nodes[off]; nodeBounds(nodes[off], &boxes[6 * (size_t)pi]);
    subDepth = std::max(subDepth, b.maxDepth);
  }
  Bvh8 top; buildTopBvh8(boxes.data(), partCount, roots.data(), top);
  if (top.nodes.size() > topCap) return -2;
  std::copy(top.nodes.begin(), top.nodes.end(), nodes.begin());
  if (outNodeCount) *outNodeCount = (uint32_t)nodes.size();
  if (outMaxDepth) *outMaxDepth = top.maxDepth + subDepth - 1u;
  return validateTree(nodes, trisAll, triCount);
}

// giCDebugValidateSceneBvh: the tree a device holds for a built scene -- whichever builder made it -- downloaded, checked and hashed
extern "C" int giCDebugValidateSceneBvh(const GiCScene* scene, uint32_t deviceIndex, uint32_t* outNodeCount, uint32_t* outMaxDepth, int32_t* outBuiltOnDevice,
    uint64_t* outDigest)
{
  GiCScene* s = const_cast<GiCScene*>(scene);
  if (!g_ctx.initialized || !s) { setError("giCDebugValidateSceneBvh: bad arguments"); return -1; }
  std::lock_guard<std::mutex> guard(s->mutex);
  if (!s->host) { setError("giCDebugValidateSceneBvh: the scene has not been built (render it once)"); return -1; }
  if (deviceIndex > s->replicas.size() || deviceIndex >= sceneDeviceCount(s)) { setError("giCDebugValidateSceneBvh: no such device copy"); return -1; }
  // (a result here would be made up: there is no tree to download, check or hash -- giCDebugSceneTlasCheck and giCDebugSceneBlasCheck hold what the scene walks)
  if (s->host->treeless) { setError("giCDebugValidateSceneBvh: the scene was built without the flat tree (GI_C_SCENE_OPTION_TLAS_ONLY): there is no flat BVH to "
                                    "validate"); return -1; }
  SceneDevice& D = sceneDevice(s, deviceIndex);
  const uint32_t nodeCount = s->nodeCount, triCount = s->triCount;
  std::vector<Node8> nodes(nodeCount); std::vector<TriRec> tris(triCount);
  if (hipSetDevice(g_ctx.devs[D.slot].device) != hipSuccess || D.dNodes.count < nodeCount || D.dTris.count < triCount ||
      (nodeCount && hipMemcpy(nodes.data(), D.dNodes.ptr, (size_t)nodeCount * sizeof(Node8), hipMemcpyDeviceToHost) != hipSuccess) ||
      (triCount && hipMemcpy(tris.data(), D.dTris.ptr, (size_t)triCount * sizeof(TriRec), hipMemcpyDeviceToHost) != hipSuccess)) {
    (void)hipSetDevice(g_ctx.device); setError("giCDebugValidateSceneBvh: download failed"); return -1;
  }
  (void)hipSetDevice(g_ctx.device);
  // digest of the node and triangle bytes (64-bit FNV-1a over 8-byte words)
  uint64_t h = 0xcbf29ce484222325ull;
  auto mix = [&h](const void* p, size_t bytes) { const uint8_t* b = (const uint8_t*)p;
      for (size_t i = 0; i + 8 <= bytes; i += 8) { uint64_t w; memcpy(&w, b + i, 8); h = (h ^ w) * 0x100000001b3ull; } };
  mix(nodes.data(), nodes.size() * sizeof(Node8)); mix(tris.data(), tris.size() * sizeof(TriRec));
  int violations = 0;
  // depth, and every internal child after its parent (both layouts place children behind their parent, which also keeps the walks below finite)
  uint32_t maxDepth = 0;
  if (nodeCount) {
    std::vector<uint32_t> depth(nodeCount, 0u); depth[0] = 1u;
    for (uint32_t i = 0; i < nodeCount; i++) {
      if (depth[i] == 0u) continue; // (partitioned layout: reserved, unused node slots)
      maxDepth = std::max(maxDepth, depth[i]);
      const uint32_t internal = (uint32_t)__builtin_popcount(nodes[i].imask);
      for (uint32_t k = 0; k < internal; k++) {
        const uint64_t c = (uint64_t)nodes[i].childBase + k;
        if (c <= i || c >= nodeCount) { violations++; continue; }
        depth[c] = depth[i] + 1u;
      }
    }
  }
  if (maxDepth > 1u + 8u + 40u) violations++;
  uint32_t activeTris = triCount;
  if (!s->host->partitioned) {
    // breadth-first: in index order, every node's internal children are the next unassigned indices and its leaf triangles the next unreferenced ones
    uint32_t nextChild = 1, nextTri = 0;
    for (uint32_t i = 0; i < nodeCount; i++) {
      const Node8& n = nodes[i];
      const uint32_t internal = (uint32_t)__builtin_popcount(n.imask);
      if (internal && n.childBase != nextChild) violations++;
      nextChild += internal;
      if (n.triBase != nextTri) violations++;
      uint32_t off = 0;
      for (int sl = 0; sl < 8; sl++) {
        if (n.meta[sl] == 0 || ((n.imask >> sl) & 1u)) continue;
        const uint32_t unary = n.meta[sl] >> 5, cnt = unary == 1u ? 1u : unary == 3u ? 2u : unary == 7u ? 3u : 0u;
        if ((n.meta[sl] & 31u) != off) violations++;
        off += cnt;
      }
      nextTri = n.triBase + off;
    }
    if (nextChild != nodeCount || nextTri > triCount) violations++;
    activeTris = std::min(nextTri, triCount);
    // every active id once in [0, activeTris); the inactive ones behind, ids in increasing (input) order
    std::vector<uint8_t> seen(triCount, 0);
    for (uint32_t k = 0; k < activeTris; k++) { const uint32_t id = tris[k].origId; if (id >= triCount || seen[id]) violations++; else seen[id] = 1; }
    for (uint32_t k = activeTris; k < triCount; k++) if (tris[k].origId >= triCount || (k > activeTris && tris[k].origId <= tris[k - 1].origId)) violations++;
  }
  // a partitioned scene leaves the parts of hidden and retired meshes out of its top tree (updateVisibility, updateTopology): their records stay resident,
  // unreachable, and the live ids are those of a fresh build of the visible meshes
  std::vector<uint8_t> left; uint32_t liveIds = triCount;
  if (s->host->partitioned) {
    left.assign(triCount, 0);
    for (const InstPart& P : s->host->parts) {
      if (!s->host->meshBuilds[P.meshBuild].hidden && !P.retired) continue; // (a retired instance of a live mesh: gi_build.cpp updateTopology)
      if ((uint64_t)P.triFirst + P.nf > triCount) { violations++; continue; }
      std::fill(left.begin() + P.triFirst, left.begin() + P.triFirst + P.nf, (uint8_t)1);
      liveIds -= P.nf;
    }
  }
  if (violations == 0) violations = validateTree(nodes, tris, liveIds, s->host->partitioned ? &left : nullptr); // (reachability + conservativeness; needs a well-formed tree)
  if (outNodeCount) *outNodeCount = nodeCount;
  if (outMaxDepth) *outMaxDepth = maxDepth;
  if (outBuiltOnDevice) *outBuiltOnDevice = s->host->deviceBuilt ? 1 : 0;
  if (outDigest) *outDigest = h;
  return violations;
}

// giCDebugSceneFlatTreeState: what a built scene holds of the flat tree (GI_C_SCENE_OPTION_TLAS_ONLY)
extern "C" int giCDebugSceneFlatTreeState(const GiCScene* scene, uint32_t deviceIndex, uint64_t out[4])
{
  GiCScene* s = const_cast<GiCScene*>(scene);
  if (!g_ctx.initialized || !s || !out) { setError("giCDebugSceneFlatTreeState: bad arguments"); return GI_C_ERROR; }
  std::lock_guard<std::mutex> guard(s->mutex);
  if (!s->host) { setError("giCDebugSceneFlatTreeState: the scene has not been built (render it once)"); return GI_C_ERROR; }
  if (deviceIndex > s->replicas.size() || deviceIndex >= sceneDeviceCount(s)) { setError("giCDebugSceneFlatTreeState: no such device copy"); return GI_C_ERROR; }
  const SceneDevice& D = sceneDevice(s, deviceIndex);
  out[0] = s->twoLevel ? 1u : 0u; out[1] = s->host->treeless ? 1u : 0u;
  out[2] = D.dNodes.ptr ? (uint64_t)D.dNodes.count : 0u;
  out[3] = (uint64_t)s->host->bvh.nodes.size() * sizeof(Node8);
  return GI_C_OK;
}

// giCDebugRefitBvh: the refit's arithmetic (gi_refit.h, what gi_refit.hip's kernels run) on the host -- a tree built over A, refitted to B, validated against B
extern "C" int giCDebugRefitBvh(const float* triVertsA, const float* triVertsB, uint32_t triCount, uint32_t* outNodeCount, uint32_t* outMaxDepth)
{
  if (triCount && (!triVertsA || !triVertsB)) return -1;
  std::vector<TriRec> tris(triCount);
  for (uint32_t i = 0; i < triCount; i++) {
    const float* p = triVertsA + 9 * (size_t)i;
    for (int a = 0; a < 3; a++) { tris[i].v0[a] = p[a]; tris[i].e1[a] = p[3 + a] - p[a]; tris[i].e2[a] = p[6 + a] - p[a]; }
    tris[i].instance = 0; tris[i].prim = i; tris[i].origId = i;
  }
  Bvh8 bvh; buildBvh8(tris, bvh);
  const size_t nodesBefore = bvh.nodes.size();
  for (TriRec& t : bvh.tris) { // the records where the builder left them; the id names the triangle
    if (t.origId >= triCount) return -1;
    const float* p = triVertsB + 9 * (size_t)t.origId;
    for (int a = 0; a < 3; a++) { t.v0[a] = p[a]; t.e1[a] = p[3 + a] - p[a]; t.e2[a] = p[6 + a] - p[a]; }
  }
  std::vector<float> boxes(bvh.nodes.size() * 8u, 0.0f);
  const RefitScene S{bvh.tris.data(), (uint32_t)bvh.tris.size(), nullptr, 0u, nullptr, 0u};
  refitHost(bvh.nodes.data(), (uint32_t)bvh.nodes.size(), 0u, boxes.data(), S);
  if (outNodeCount) *outNodeCount = (uint32_t)bvh.nodes.size();
  if (outMaxDepth) *outMaxDepth = bvh.maxDepth;
  if (bvh.nodes.size() != nodesBefore || bvh.levelStart.size() != (size_t)bvh.maxDepth + 1u || bvh.levelStart.back() != bvh.nodes.size()) return -1;
  return validateTree(bvh.nodes, bvh.tris, triCount);
}

// giCDebugSceneRefitCheck: the resident nodes and triangles downloaded, the host refit run over a copy: a refit is a function of topology and triangles alone
extern "C" int giCDebugSceneRefitCheck(const GiCScene* scene, uint32_t deviceIndex, uint32_t* outNodes)
{
  GiCScene* s = const_cast<GiCScene*>(scene);
  if (!g_ctx.initialized || !s) { setError("giCDebugSceneRefitCheck: bad arguments"); return -1; }
  std::lock_guard<std::mutex> guard(s->mutex);
  if (!s->host) { setError("giCDebugSceneRefitCheck: the scene has not been built (render it once)"); return -1; }
  if (deviceIndex > s->replicas.size() || deviceIndex >= sceneDeviceCount(s)) { setError("giCDebugSceneRefitCheck: no such device copy"); return -1; }
  SceneDevice& D = sceneDevice(s, deviceIndex);
  const SceneHost& H = *s->host;
  const uint32_t nodeCount = s->nodeCount, triCount = s->triCount;
  std::vector<Node8> nodes(nodeCount); std::vector<TriRec> tris(triCount);
  if (hipSetDevice(g_ctx.devs[D.slot].device) != hipSuccess || D.dNodes.count < nodeCount || D.dTris.count < triCount ||
      (nodeCount && hipMemcpy(nodes.data(), D.dNodes.ptr, (size_t)nodeCount * sizeof(Node8), hipMemcpyDeviceToHost) != hipSuccess) ||
      (triCount && hipMemcpy(tris.data(), D.dTris.ptr, (size_t)triCount * sizeof(TriRec), hipMemcpyDeviceToHost) != hipSuccess)) {
    (void)hipSetDevice(g_ctx.device); setError("giCDebugSceneRefitCheck: download failed"); return -1;
  }
  (void)hipSetDevice(g_ctx.device);
  // Flat layouts: every node.  Partitioned layout: the live nodes of every part, [nodeOff, nodeOff + nodeCount) -- the top tree is built over padded part
  // bounds, not refitted, and the reserve behind a part's nodes may hold what an earlier, larger subtree left there
  std::vector<std::pair<uint32_t, uint32_t>> spans; // (first, count)
  if (!H.partitioned) spans.emplace_back(0u, nodeCount);
  else for (const InstPart& P : H.parts) {
    if ((uint64_t)P.nodeOff + P.nodeCount > nodeCount) { setError("giCDebugSceneRefitCheck: a part lies outside the node array"); return -1; }
    spans.emplace_back(P.nodeOff, P.nodeCount);
  }
  for (uint32_t i = 0; i < nodeCount; i++) { // refitHost walks by descending index: every internal child must lie behind its parent
    const uint32_t internal = (uint32_t)__builtin_popcount(nodes[i].imask);
    if (internal && ((uint64_t)nodes[i].childBase <= i || (uint64_t)nodes[i].childBase + internal > nodeCount)) { setError("giCDebugSceneRefitCheck: malformed tree"); return -1; }
  }
  std::vector<Node8> refitted(nodes);
  std::vector<float> boxes((size_t)nodeCount * 8u, 0.0f);
  // shading records only where the triangle records name them (scenes beyond LDS)
  const RefitScene S{tris.data(), triCount, H.shadePacked ? H.instances.data() : nullptr, (uint32_t)H.instances.size(), H.shadePacked ? H.triShade.data() : nullptr,
      (uint32_t)H.triShade.size()};
  int differ = 0; uint32_t compared = 0;
  for (const auto& sp : spans) { // (children before parents: descending index inside a tree)
    for (uint32_t i = sp.first + sp.second; i-- > sp.first;) refit_node(refitted.data(), nodeCount, i, boxes.data(), S);
    for (uint32_t i = sp.first; i < sp.first + sp.second; i++) if (memcmp(&refitted[i], &nodes[i], sizeof(Node8)) != 0) differ++;
    compared += sp.second;
  }
  if (outNodes) *outNodes = compared;
  return differ;
}

// giCDebugSceneShadeCheck: the resident vertex and shading records against the host's copies, whole arrays (a vertex update sends the former and gathers
// the latter on the device: gi_refit.hip k_gather_shade)
extern "C" int giCDebugSceneShadeCheck(const GiCScene* scene, uint32_t deviceIndex, uint32_t* outRecords)
{
  GiCScene* s = const_cast<GiCScene*>(scene);
  if (!g_ctx.initialized || !s) { setError("giCDebugSceneShadeCheck: bad arguments"); return -1; }
  std::lock_guard<std::mutex> guard(s->mutex);
  if (!s->host) { setError("giCDebugSceneShadeCheck: the scene has not been built (render it once)"); return -1; }
  if (deviceIndex > s->replicas.size() || deviceIndex >= sceneDeviceCount(s)) { setError("giCDebugSceneShadeCheck: no such device copy"); return -1; }
  SceneDevice& D = sceneDevice(s, deviceIndex);
  const SceneHost& H = *s->host;
  std::vector<TriShade> shade(H.triShade.size()); std::vector<FVertex> verts(H.verts.size());
  if (hipSetDevice(g_ctx.devs[D.slot].device) != hipSuccess || D.dTriShade.count < shade.size() || D.dVerts.count < verts.size() ||
      (!shade.empty() && hipMemcpy(shade.data(), D.dTriShade.ptr, shade.size() * sizeof(TriShade), hipMemcpyDeviceToHost) != hipSuccess) ||
      (!verts.empty() && hipMemcpy(verts.data(), D.dVerts.ptr, verts.size() * sizeof(FVertex), hipMemcpyDeviceToHost) != hipSuccess)) {
    (void)hipSetDevice(g_ctx.device); setError("giCDebugSceneShadeCheck: download failed"); return -1;
  }
  (void)hipSetDevice(g_ctx.device);
  int differ = 0;
  for (size_t i = 0; i < shade.size(); i++) if (memcmp(&shade[i], &H.triShade[i], sizeof(TriShade)) != 0) differ++;
  for (size_t i = 0; i < verts.size(); i++) if (memcmp(&verts[i], &H.verts[i], sizeof(FVertex)) != 0) differ++;
  if (outRecords) *outRecords = (uint32_t)shade.size();
  return differ;
}

// giCDebugShadeClass: which k_shade variant an (untextured) material's hits are binned for -- host only
extern "C" int giCDebugShadeClass(const GiCMaterialDesc* desc)
{
  if (!desc) return -1;
  MaterialRec m{}; m.klass = desc->klass; m.flags = desc->flags & ~(MAT_FLAG_TEXTURED | MAT_FLAG_OPACITY_TEX); memcpy(m.p, desc->p, sizeof(m.p));
  deriveMaterialConstants(m);
  return (int)shadeClassOf(m);
}

// ---------------------------------------------------------------------------------------------------------------
// giCDebugEvalBsdf: closed-form BSDF sample/evaluate on the device for explicit shading frames
// ---------------------------------------------------------------------------------------------------------------
extern "C" int giCDebugEvalBsdf(const GiCMaterialDesc* desc, uint32_t count, const float* in, float* out)
{
  if (!g_ctx.initialized || !desc || (count && (!in || !out))) { setError("giCDebugEvalBsdf: bad arguments"); return GI_C_ERROR; }
  if (count == 0) return GI_C_OK;
  MaterialRec m{}; m.klass = desc->klass; m.flags = desc->flags & ~(MAT_FLAG_TEXTURED | MAT_FLAG_OPACITY_TEX); memcpy(m.p, desc->p, sizeof(m.p));
  deriveMaterialConstants(m);
  // the variant the render would shade this material's hits with (GATLING_OPTIONS=shade_variants=0: always the full closed form)
  const uint32_t shadeClass = shadeClassOf(m);
  MaterialRec* dm = nullptr; float* din = nullptr; float* dout = nullptr;
  hipStream_t st = g_ctx.stream;
  int rc = GI_C_ERROR;
  if (hipMalloc((void**)&dm, sizeof(m)) == hipSuccess && hipMalloc((void**)&din, (size_t)count * 22 * 4) == hipSuccess &&
      hipMalloc((void**)&dout, (size_t)count * 15 * 4) == hipSuccess &&
      hipMemcpyAsync(dm, &m, sizeof(m), hipMemcpyHostToDevice, st) == hipSuccess &&
      hipMemcpyAsync(din, in, (size_t)count * 22 * 4, hipMemcpyHostToDevice, st) == hipSuccess) {
    launchDebugBsdf(st, dm, shadeClass, count, din, dout);
    if (hipMemcpyAsync(out, dout, (size_t)count * 15 * 4, hipMemcpyDeviceToHost, st) == hipSuccess && hipStreamSynchronize(st) == hipSuccess) rc = GI_C_OK;
  }
  if (rc != GI_C_OK) setError("giCDebugEvalBsdf: HIP failure");
  if (dm) (void)hipFree(dm); if (din) (void)hipFree(din); if (dout) (void)hipFree(dout);
  return rc;
}

// ---------------------------------------------------------------------------------------------------------------
// giCDebugTexRuntime: the MDL renderer runtime's remaining texture entry points (tex_texel_float4_2d, tex_resolution_2d, tex_lookup_float4_3d,
// tex_texel_float4_3d) on the device, for explicit queries
// ---------------------------------------------------------------------------------------------------------------
extern "C" int giCDebugTexRuntime(const float* rgba, uint32_t width, uint32_t height, uint32_t depth, uint32_t count, const float* queries, float* out)
{
  if (!g_ctx.initialized || !rgba || !width || !height || !depth || (count && (!queries || !out))) { setError("giCDebugTexRuntime: bad arguments");
      return GI_C_ERROR; }
  if (count == 0) return GI_C_OK;
  const size_t texFloats = (size_t)width * height * depth * 4;
  float* dt = nullptr; float* dq = nullptr; float* dout = nullptr;
  hipStream_t st = g_ctx.stream;
  int rc = GI_C_ERROR;
  if (hipMalloc((void**)&dt, texFloats * 4) == hipSuccess && hipMalloc((void**)&dq, (size_t)count * 32) == hipSuccess
      && hipMalloc((void**)&dout, (size_t)count * 16) == hipSuccess &&
      hipMemcpyAsync(dt, rgba, texFloats * 4, hipMemcpyHostToDevice, st) == hipSuccess
          && hipMemcpyAsync(dq, queries, (size_t)count * 32, hipMemcpyHostToDevice, st) == hipSuccess) {
    launchDebugTex(st, dt, width, height, depth, count, dq, dout);
    if (hipMemcpyAsync(out, dout, (size_t)count * 16, hipMemcpyDeviceToHost, st) == hipSuccess && hipStreamSynchronize(st) == hipSuccess) rc = GI_C_OK;
  }
  if (rc != GI_C_OK) setError("giCDebugTexRuntime: HIP failure");
  if (dt) (void)hipFree(dt); if (dq) (void)hipFree(dq); if (dout) (void)hipFree(dout);
  return rc;
}


// ---------------------------------------------------------------------------------------------------------------
// giCDebugCheckSqrt: the kernels' square root (gi_device_math.h gi_sqrt) against the compiler's correctly rounded sqrtf for the `count` bit patterns from `first` on
// (count = 2^32: every float).  Returns the number of arguments whose results differ, or -1 on error.
// ---------------------------------------------------------------------------------------------------------------
extern "C" int64_t giCDebugCheckSqrt(uint32_t first, uint64_t count)
{
  if (!g_ctx.initialized) { setError("giCDebugCheckSqrt before giCInitialize"); return -1; }
  unsigned long long* d = nullptr; unsigned long long h = 0ull;
  if (hipMalloc(&d, sizeof(h)) != hipSuccess) { setError("giCDebugCheckSqrt: hipMalloc failed"); return -1; }
  bool ok = hipMemsetAsync(d, 0, sizeof(h), g_ctx.stream) == hipSuccess;
  if (ok) { launchDebugSqrt(g_ctx.stream, first, (unsigned long long)count, d); ok = hipMemcpyAsync(&h, d, sizeof(h), hipMemcpyDeviceToHost, g_ctx.stream) == hipSuccess; }
  ok = ok && hipStreamSynchronize(g_ctx.stream) == hipSuccess;
  (void)hipFree(d);
  if (!ok) { setError("giCDebugCheckSqrt: device error"); return -1; }
  return (int64_t)h;
}

// ---------------------------------------------------------------------------------------------------------------
// giCDebugCheckDiv: the fused kernels' division (gi_device_math.h gi_div, V3 / float, normalize) against the compiler's correctly rounded `/` (gi_path.hip
// k_debug_div has the modes).  Returns the number of items with a differing result, or -1 on error.
// ---------------------------------------------------------------------------------------------------------------
extern "C" int64_t giCDebugCheckDiv(uint32_t mode, uint64_t count, uint32_t seed, const uint32_t* words)
{
  if (!g_ctx.initialized) { setError("giCDebugCheckDiv before giCInitialize"); return -1; }
  const bool given = mode == 0u || mode == 2u;
  if (mode > 4u || (given && (!words || count > (1ull << 28)))) { setError("giCDebugCheckDiv: bad arguments"); return -1; }
  const size_t bytes = given ? (size_t)count * (mode == 0u ? 2u : 4u) * sizeof(uint32_t) : 0u;
  unsigned long long* d = nullptr; unsigned long long h = 0ull; uint32_t* dw = nullptr;
  if (hipMalloc(&d, sizeof(h)) != hipSuccess) { setError("giCDebugCheckDiv: hipMalloc failed"); return -1; }
  bool ok = bytes == 0u || hipMalloc(&dw, bytes) == hipSuccess;
  ok = ok && (bytes == 0u || hipMemcpyAsync(dw, words, bytes, hipMemcpyHostToDevice, g_ctx.stream) == hipSuccess);
  ok = ok && hipMemsetAsync(d, 0, sizeof(h), g_ctx.stream) == hipSuccess;
  if (ok) { launchDebugDiv(g_ctx.stream, mode, (unsigned long long)count, seed, dw, d); ok = hipMemcpyAsync(&h, d, sizeof(h), hipMemcpyDeviceToHost, g_ctx.stream) == hipSuccess; }
  ok = ok && hipStreamSynchronize(g_ctx.stream) == hipSuccess;
  (void)hipFree(d); if (dw) (void)hipFree(dw);
  if (!ok) { setError("giCDebugCheckDiv: device error"); return -1; }
  return (int64_t)h;
}

// ---------------------------------------------------------------------------------------------------------------
// Cooked nodes (gi_node_cook.h; k_path's COOK variants): giCDebugSceneNodeCook -- whether the last fused launch ran one (gi_render.cpp runFusedBatch);
// giCDebugNodeCook -- the cooked image of given nodes, made by the function the kernel stages with (host only); giCDebugCheckNodeCook -- the cooked node test
// against trav_node_test on the device (gi_path.hip k_debug_node_cook).
// ---------------------------------------------------------------------------------------------------------------
extern "C" int giCDebugSceneNodeCook(const GiCScene* scene, uint32_t* out)
{
  const GiCScene* s = scene;
  if (!s || !out) { setError("giCDebugSceneNodeCook: bad arguments"); return GI_C_ERROR; }
  out[0] = s->nodeCookLaunched;
  return GI_C_OK;
}

extern "C" int giCDebugNodeCook(const void* nodes, uint32_t nodeCount, int32_t octBlocks, void* outImage, uint32_t imageCap, uint32_t* outInfo)
{
  if (!nodes || !outImage || !outInfo || nodeCount == 0u || nodeCount > (1u << 16)) { setError("giCDebugNodeCook: bad arguments"); return GI_C_ERROR; }
  const uint32_t blocks = octBlocks < 0 ? gi::cook_oct_blocks_max(nodeCount) : (uint32_t)octBlocks;
  if (blocks > (1u << 16)) { setError("giCDebugNodeCook: bad arguments"); return GI_C_ERROR; }
  const uint32_t bytes = nodeCount * gi::COOK_NODE_BYTES + blocks * gi::COOK_OCT_DWORDS * 4u;
  if (imageCap < bytes) { setError("giCDebugNodeCook: the image needs more room"); return GI_C_ERROR; }
  std::vector<gi::Node8> in(nodeCount);
  memcpy(in.data(), nodes, (size_t)nodeCount * sizeof(gi::Node8));
  std::vector<uint32_t> image(bytes / 4u, 0u);
  for (uint32_t i = 0; i < nodeCount; i++) gi::cook_place(in.data(), i, nodeCount, blocks, image.data());
  memcpy(outImage, image.data(), bytes);
  outInfo[0] = bytes; outInfo[1] = gi::COOK_NODE_BYTES; outInfo[2] = gi::COOK_OCT_DWORDS * 4u;
  return GI_C_OK;
}

extern "C" int64_t giCDebugCheckNodeCook(const void* nodes, uint32_t nodeCount, const float* rays, uint64_t count)
{
  if (!g_ctx.initialized) { setError("giCDebugCheckNodeCook before giCInitialize"); return -1; }
  if (!nodes || !rays || nodeCount == 0u || nodeCount > 64u || count == 0u || count > (1ull << 26)) { setError("giCDebugCheckNodeCook: bad arguments"); return -1; }
  const size_t nodeBytes = (size_t)nodeCount * sizeof(gi::Node8), rayBytes = (size_t)count * 8u * sizeof(float);
  unsigned long long* d = nullptr; unsigned long long h = 0ull; gi::Node8* dn = nullptr; float* dr = nullptr;
  bool ok = hipMalloc(&d, sizeof(h)) == hipSuccess && hipMalloc(&dn, nodeBytes) == hipSuccess && hipMalloc(&dr, rayBytes) == hipSuccess;
  ok = ok && hipMemcpyAsync(dn, nodes, nodeBytes, hipMemcpyHostToDevice, g_ctx.stream) == hipSuccess;
  ok = ok && hipMemcpyAsync(dr, rays, rayBytes, hipMemcpyHostToDevice, g_ctx.stream) == hipSuccess;
  ok = ok && hipMemsetAsync(d, 0, sizeof(h), g_ctx.stream) == hipSuccess;
  if (ok) {
    ok = launchDebugNodeCook(g_ctx.stream, dn, nodeCount, dr, (unsigned long long)count, d) == 0;
    ok = ok && hipMemcpyAsync(&h, d, sizeof(h), hipMemcpyDeviceToHost, g_ctx.stream) == hipSuccess;
  }
  ok = hipStreamSynchronize(g_ctx.stream) == hipSuccess && ok;
  if (d) (void)hipFree(d);
  if (dn) (void)hipFree(dn);
  if (dr) (void)hipFree(dr);
  if (!ok) { setError("giCDebugCheckNodeCook: device error"); return -1; }
  return (int64_t)h;
}

// ---------------------------------------------------------------------------------------------------------------
// giCDebugEditDirtyFlags / giCDebugSceneUpdateCounts: which edits take the incremental paths (host only)
// ---------------------------------------------------------------------------------------------------------------
// A scratch scene of one texture, two materials and one one-triangle mesh is made through the C ABI's own entry points; with `built` it is marked the way a
// successful buildScene leaves it (a host copy, the mesh part of it, no dirty flag).  Then the one edit runs and the flags it raised are returned.  No device
// is touched: the scene is never rendered.
extern "C" int32_t giCDebugEditDirtyFlags(int32_t edit, int32_t built)
{
  std::unique_ptr<GiCScene> scene(new GiCScene());
  GiCScene* s = scene.get();
  const float texel[4] = {1.0f, 1.0f, 1.0f, 1.0f};
  GiCTextureDesc td{1u, 1u, texel};
  GiCMaterialDesc md{}; md.klass = GI_C_MAT_USD_PREVIEW_SURFACE;
  GiCVertex verts[3] = {}; verts[1].pos[0] = 1.0f; verts[2].pos[1] = 1.0f;
  GiCFace face{}; face.v_i[0] = 0; face.v_i[1] = 1; face.v_i[2] = 2;
  GiCMeshDesc meshDesc{}; meshDesc.faceCount = 1; meshDesc.faces = &face; meshDesc.vertexCount = 3; meshDesc.vertices = verts; meshDesc.name = "debug";
  const float identity[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
  GiCTexture* tex = giCCreateTexture(s, &td);
  GiCMaterial* matA = giCCreateMaterial(s, "a", &md);
  GiCMaterial* matB = giCCreateMaterial(s, "b", &md);
  GiCMesh* mesh = giCCreateMesh(s, &meshDesc);
  if (!tex || !matA || !matB || !mesh) return -1;
  giCSetMeshInstanceTransforms(mesh, 1, identity);
  giCSetMeshMaterial(mesh, matA);
  if (built) { s->host.reset(new SceneHost()); mesh->builtInstances = 1; }
  s->dirty = 0;
  GiCMaterial* made = nullptr; GiCTexture* madeTex = nullptr; GiCMesh* madeMesh = nullptr;
  GiCTextureBinding binding{}; binding.texture = tex; for (int i = 0; i < 4; i++) binding.scale[i] = 1.0f;
  const float xf[6] = {1, 0, 0, 0, 1, 0};
  const float one = 1.0f; const int32_t id = 7;
  GiCPrimvarData pv{}; pv.name = "k"; pv.type = GI_C_PRIMVAR_FLOAT; pv.interpolation = GI_C_INTERP_CONSTANT; pv.data = &one; pv.dataSize = 4;
  int32_t result = 0;
  switch (edit) {
    case 0: made = giCCreateMaterial(s, "c", &md); break;
    case 1: giCDestroyMaterial(matB); matB = nullptr; break;
    case 2: giCSetMeshMaterial(mesh, matB); break;
    case 3: giCSetMaterialPrimvarInput(matA, GI_C_TEX_BASE_COLOR, "k"); break;
    case 4: giCSetMaterialTexture(matA, GI_C_TEX_BASE_COLOR, &binding); break;
    case 5: giCSetMaterialTextureTransform(matA, GI_C_TEX_BASE_COLOR, xf); break;
    case 6: madeTex = giCCreateTexture(s, &td); break;
    case 7: giCDestroyTexture(tex); tex = nullptr; break;
    case 8: giCSetMeshPrimvars(mesh, 1, &pv); break;
    case 9: giCSetMeshInstancerPrimvars(mesh, 1, &pv); break;
    case 10: giCSetMeshTransform(mesh, identity); break;
    case 11: giCSetMeshVisibility(mesh, 0); break;
    case 12: giCSetMeshInstanceIds(mesh, 1, &id); break;
    case 13: madeMesh = giCCreateMesh(s, &meshDesc); break;
    case 14: giCDestroyMesh(mesh); mesh = nullptr; break;
    case 15: giCSetMeshInstanceTransforms(mesh, 0, nullptr); break;
    case 16: if (giCSetMeshVertices(mesh, 3, verts) != GI_C_OK) result = -1; break;
    default: result = -1; break;
  }
  if (result == 0) result = (int32_t)s->dirty;
  if (madeMesh) giCDestroyMesh(madeMesh);
  if (mesh) giCDestroyMesh(mesh);
  if (made) giCDestroyMaterial(made);
  if (matA) giCDestroyMaterial(matA);
  if (matB) giCDestroyMaterial(matB);
  if (madeTex) giCDestroyTexture(madeTex);
  if (tex) giCDestroyTexture(tex);
  return result;
}

extern "C" int giCDebugSceneUpdateCounts(const GiCScene* scene, uint64_t* outCounts)
{
  GiCScene* s = const_cast<GiCScene*>(scene);
  if (!s || !outCounts) { setError("giCDebugSceneUpdateCounts: bad arguments"); return GI_C_ERROR; }
  std::lock_guard<std::mutex> guard(s->mutex);
  outCounts[0] = s->updateCounts[UPDATE_FULL]; outCounts[1] = s->updateCounts[UPDATE_TRANSFORM]; outCounts[2] = s->updateCounts[UPDATE_MATERIAL];
  return GI_C_OK;
}

extern "C" int giCDebugSceneVisibilityUpdateCount(const GiCScene* scene, uint64_t* outCount)
{
  GiCScene* s = const_cast<GiCScene*>(scene);
  if (!s || !outCount) { setError("giCDebugSceneVisibilityUpdateCount: bad arguments"); return GI_C_ERROR; }
  std::lock_guard<std::mutex> guard(s->mutex);
  *outCount = s->updateCounts[UPDATE_VISIBILITY];
  return GI_C_OK;
}

extern "C" int giCDebugSceneVertexUpdateCount(const GiCScene* scene, uint64_t* outCount)
{
  GiCScene* s = const_cast<GiCScene*>(scene);
  if (!s || !outCount) { setError("giCDebugSceneVertexUpdateCount: bad arguments"); return GI_C_ERROR; }
  std::lock_guard<std::mutex> guard(s->mutex);
  *outCount = s->updateCounts[UPDATE_VERTEX];
  return GI_C_OK;
}

extern "C" int giCDebugSceneTopologyUpdateCount(const GiCScene* scene, uint64_t* outCount)
{
  GiCScene* s = const_cast<GiCScene*>(scene);
  if (!s || !outCount) { setError("giCDebugSceneTopologyUpdateCount: bad arguments"); return GI_C_ERROR; }
  std::lock_guard<std::mutex> guard(s->mutex);
  *outCount = s->updateCounts[UPDATE_TOPOLOGY];
  return GI_C_OK;
}

extern "C" int giCDebugSceneTlasUpdateCount(const GiCScene* scene, uint64_t* outCount)
{
  GiCScene* s = const_cast<GiCScene*>(scene);
  if (!s || !outCount) { setError("giCDebugSceneTlasUpdateCount: bad arguments"); return GI_C_ERROR; }
  std::lock_guard<std::mutex> guard(s->mutex);
  *outCount = s->updateCounts[UPDATE_TLAS];
  return GI_C_OK;
}

extern "C" int giCDebugSceneBlasUpdateCount(const GiCScene* scene, uint64_t* outCount)
{
  GiCScene* s = const_cast<GiCScene*>(scene);
  if (!s || !outCount) { setError("giCDebugSceneBlasUpdateCount: bad arguments"); return GI_C_ERROR; }
  std::lock_guard<std::mutex> guard(s->mutex);
  *outCount = s->updateCounts[UPDATE_BLAS];
  return GI_C_OK;
}

extern "C" int giCDebugSceneTlasVisibilityUpdateCount(const GiCScene* scene, uint64_t* outCount)
{
  GiCScene* s = const_cast<GiCScene*>(scene);
  if (!s || !outCount) { setError("giCDebugSceneTlasVisibilityUpdateCount: bad arguments"); return GI_C_ERROR; }
  std::lock_guard<std::mutex> guard(s->mutex);
  *outCount = s->updateCounts[UPDATE_TLAS_VISIBILITY];
  return GI_C_OK;
}

extern "C" int giCDebugSceneTlasTopologyUpdateCount(const GiCScene* scene, uint64_t* outCount)
{
  GiCScene* s = const_cast<GiCScene*>(scene);
  if (!s || !outCount) { setError("giCDebugSceneTlasTopologyUpdateCount: bad arguments"); return GI_C_ERROR; }
  std::lock_guard<std::mutex> guard(s->mutex);
  *outCount = s->updateCounts[UPDATE_TLAS_TOPOLOGY];
  return GI_C_OK;
}

extern "C" int giCDebugSceneTlasInstanceUpdateStats(const GiCScene* scene, uint64_t* out)
{
  GiCScene* s = const_cast<GiCScene*>(scene);
  if (!s || !out) { setError("giCDebugSceneTlasInstanceUpdateStats: bad arguments"); return GI_C_ERROR; }
  std::lock_guard<std::mutex> guard(s->mutex);
  for (int i = 0; i < 4; i++) out[i] = s->tlasInstanceCounts[i];
  return GI_C_OK;
}

extern "C" int giCDebugSceneCompactionCount(const GiCScene* scene, uint64_t* out)
{
  GiCScene* s = const_cast<GiCScene*>(scene);
  if (!s || !out) { setError("giCDebugSceneCompactionCount: bad arguments"); return GI_C_ERROR; }
  std::lock_guard<std::mutex> guard(s->mutex);
  for (int i = 0; i < 4; i++) out[i] = s->compactionStats[i];
  return GI_C_OK;
}

// giCDebugCompactRanges / giCDebugCompactRangesHost: k_compact_ranges (onDevice) or its host form (gi_compact.h) over the caller's records and live / dead
// ranges, against a restatement written without the header's per-piece forms: the live ranges' records filtered in order, then the fields that hold indices
// rebased one by one through the record types, the id table written at the ids of the flat records that are not hidden.  Scratch arrays start as 0xa5 bytes
template <class Rec, class Rebase>
static void compactRestated(const void* records, const GiCDebugCompactRange* ranges, uint32_t rangeCount, std::vector<uint8_t>& want, Rebase&& rebase)
{
  const Rec* in = static_cast<const Rec*>(records);
  std::vector<Rec> live; std::vector<uint32_t> rangeOf;
  uint32_t at = 0;
  for (uint32_t k = 0; k < rangeCount; at += ranges[k].count, k++)
    if (ranges[k].live) for (uint32_t i = 0; i < ranges[k].count; i++) { live.push_back(in[at + i]); rangeOf.push_back(k); } // filter ...
  for (size_t i = 0; i < live.size(); i++) rebase(live[i], ranges[rangeOf[i]], (uint32_t)i);                            // ... then rebase
  want.resize(live.size() * sizeof(Rec));
  if (!live.empty()) memcpy(want.data(), live.data(), want.size());
}
static int debugCompactRanges(const char* name, bool onDevice, uint32_t kind, const void* records, uint32_t recordCount, const GiCDebugCompactRange* rangesIn,
    uint32_t rangeCount, uint32_t* outInfo)
{
  if (onDevice && !g_ctx.initialized) { setError(std::string(name) + " before giCInitialize"); return -1; }
  const uint32_t P = compact_pieces(kind);
  if (P == 0u || (recordCount && !records) || (rangeCount && !rangesIn)) { setError(std::string(name) + ": bad arguments"); return -1; }
  try {
    const size_t recBytes = (size_t)P * compact_piece_bytes(kind);
    uint64_t covered = 0, liveCount = 0;
    for (uint32_t k = 0; k < rangeCount; k++) { covered += rangesIn[k].count; if (rangesIn[k].live) liveCount += rangesIn[k].count; }
    if (covered != recordCount || liveCount >= (1ull << 28)) { setError(std::string(name) + ": the ranges do not cover the records"); return -1; }
    const uint32_t live = (uint32_t)liveCount, tableCount = kind == COMPACT_TRIS ? live : 0u;
    // --- the restatement
    std::vector<uint8_t> want; std::vector<uint32_t> wantTable(tableCount, 0xa5a5a5a5u);
    switch (kind) {
      case COMPACT_VERTS: compactRestated<FVertex>(records, rangesIn, rangeCount, want, [](FVertex&, const GiCDebugCompactRange&, uint32_t) {}); break;
      case COMPACT_BLAS_TRIS: compactRestated<BlasTri>(records, rangesIn, rangeCount, want, [](BlasTri&, const GiCDebugCompactRange&, uint32_t) {}); break;
      case COMPACT_WORDS: compactRestated<int32_t>(records, rangesIn, rangeCount, want, [](int32_t&, const GiCDebugCompactRange&, uint32_t) {}); break;
      case COMPACT_SHADE: compactRestated<TriShade>(records, rangesIn, rangeCount, want, [](TriShade& q, const GiCDebugCompactRange& r, uint32_t) {
          for (int k = 0; k < 3; k++) q.vi[k] += r.delta[0]; }); break;
      case COMPACT_BLAS_NODES: compactRestated<Node8>(records, rangesIn, rangeCount, want, [](Node8& n, const GiCDebugCompactRange& r, uint32_t) {
          n.childBase += r.delta[0]; n.triBase += r.delta[1]; }); break;
      case COMPACT_INSTANCES: compactRestated<InstanceRec>(records, rangesIn, rangeCount, want, [](InstanceRec& ir, const GiCDebugCompactRange& r, uint32_t) { ir.mesh += r.delta[0]; }); break;
      case COMPACT_INST_TRAV: compactRestated<InstTrav>(records, rangesIn, rangeCount, want, [](InstTrav& tv, const GiCDebugCompactRange& r, uint32_t) { tv.blasRoot += r.delta[0]; }); break;
      default: compactRestated<TriRec>(records, rangesIn, rangeCount, want, [&](TriRec& t, const GiCDebugCompactRange& r, uint32_t at) {
          t.instance += r.delta[0]; t.vi[0] += r.delta[1]; t.vi[1] += r.delta[2]; t.vi[2] += r.delta[2];
          if (!r.hidden && t.origId < tableCount) wantTable[t.origId] = at; }); break;
    }
    // --- the table of the live ranges, as gi_build.cpp compactTwoLevel makes it (one entry per live range: empty ones keep theirs; nothing is joined)
    std::vector<CompactRange> ranges;
    CompactSizes Z{}; Z.kind = kind; Z.srcCount = recordCount; Z.dstCount = live; Z.tableCount = tableCount;
    uint32_t src = 0, dst = 0;
    for (uint32_t k = 0; k < rangeCount; src += rangesIn[k].count, k++) {
      if (!rangesIn[k].live) continue;
      ranges.push_back(CompactRange{src, dst, rangesIn[k].count, 0u, {rangesIn[k].delta[0], rangesIn[k].delta[1], rangesIn[k].delta[2]}, rangesIn[k].hidden ? COMPACT_RANGE_HIDDEN : 0u});
      dst += rangesIn[k].count;
    }
    Z.rangeCount = (uint32_t)ranges.size(); Z.wgCount = compactRangesNumber(kind, ranges.data(), Z.rangeCount);
    if (Z.wgCount == 0xffffffffu || !compactRangesOk(ranges.data(), Z)) { setError(std::string(name) + ": the range table does not pass its check"); return -1; }
    if (outInfo) { outInfo[0] = compact_items_per_wave(kind); outInfo[1] = compact_items_per_block(kind); outInfo[2] = live; outInfo[3] = Z.wgCount; }
    // --- the kernel or its host form, into arrays of the exact size
    std::vector<uint8_t> got((size_t)live * recBytes, 0xa5); std::vector<uint32_t> gotTable(tableCount, 0xa5a5a5a5u);
    int inPlaceDiffer = 0;
    if (!onDevice) {
      // (16-byte aligned pieces: the records as the type they are)
      std::vector<F4> srcAligned(((size_t)recordCount * recBytes + 15u) / 16u + 1u), dstAligned(((size_t)live * recBytes + 15u) / 16u + 1u);
      if (recordCount) memcpy(srcAligned.data(), records, (size_t)recordCount * recBytes);
      memset(static_cast<void*>(dstAligned.data()), 0xa5, dstAligned.size() * sizeof(F4));
      const uint32_t half = Z.wgCount / 2u; // (in two halves, as the host's thread pool splits the workgroups, and past the end)
      compactRangesHost(ranges.data(), Z, half, Z.wgCount, srcAligned.data(), dstAligned.data(), gotTable.data());
      compactRangesHost(ranges.data(), Z, 0u, half, srcAligned.data(), dstAligned.data(), gotTable.data());
      compactRangesHost(ranges.data(), Z, Z.wgCount, Z.wgCount + 3u, srcAligned.data(), dstAligned.data(), gotTable.data());
      if (!got.empty()) memcpy(got.data(), dstAligned.data(), got.size());
      // the host's own form (gi_build.cpp compactTwoLevel): the array compacted where it lies, the table the OLD one -- every visible record named at its old
      // position -- whose first words become the new one; its differing bytes are counted with the others
      std::vector<uint32_t> oldTable(tableCount, 0xa5a5a5a5u);
      if (kind == COMPACT_TRIS) {
        uint32_t at = 0;
        for (uint32_t k = 0; k < rangeCount; k++) for (uint32_t i = 0; i < rangesIn[k].count; i++, at++)
          if (rangesIn[k].live && !rangesIn[k].hidden) { TriRec t; memcpy(&t, reinterpret_cast<const char*>(srcAligned.data()) + (size_t)at * recBytes, sizeof(t)); if (t.origId < tableCount) oldTable[t.origId] = at; }
      }
      compactRangesInPlaceHost(ranges.data(), Z, srcAligned.data(), oldTable.data());
      for (size_t i = 0; i < got.size(); i++) inPlaceDiffer += reinterpret_cast<const uint8_t*>(srcAligned.data())[i] != want[i];
      for (uint32_t i = 0; i < tableCount; i++) inPlaceDiffer += 4 * (oldTable[i] != wantTable[i]);
    } else {
      DeviceBuffer<uint8_t> dSrc, dDst; DeviceBuffer<uint32_t> dTable; DeviceBuffer<CompactRange> dRanges;
      hipStream_t st = g_ctx.stream;
      bool ok = hipSetDevice(g_ctx.device) == hipSuccess && dSrc.alloc((size_t)recordCount * recBytes) == GI_C_OK && dDst.alloc(got.size()) == GI_C_OK &&
          dTable.alloc(tableCount) == GI_C_OK && dRanges.upload(ranges, st) == GI_C_OK;
      ok = ok && (recordCount == 0u || hipMemcpyAsync(dSrc.ptr, records, (size_t)recordCount * recBytes, hipMemcpyHostToDevice, st) == hipSuccess) &&
          (got.empty() || hipMemcpyAsync(dDst.ptr, got.data(), got.size(), hipMemcpyHostToDevice, st) == hipSuccess) &&
          (tableCount == 0u || hipMemcpyAsync(dTable.ptr, gotTable.data(), (size_t)tableCount * 4u, hipMemcpyHostToDevice, st) == hipSuccess);
      ok = ok && launchCompactRanges(st, ranges.data(), dRanges.ptr, Z, dSrc.ptr, dDst.ptr, tableCount ? dTable.ptr : nullptr) && hipGetLastError() == hipSuccess;
      ok = ok && (got.empty() || hipMemcpyAsync(got.data(), dDst.ptr, got.size(), hipMemcpyDeviceToHost, st) == hipSuccess) &&
          (tableCount == 0u || hipMemcpyAsync(gotTable.data(), dTable.ptr, (size_t)tableCount * 4u, hipMemcpyDeviceToHost, st) == hipSuccess);
      ok = hipStreamSynchronize(st) == hipSuccess && ok;
      dSrc.release(); dDst.release(); dTable.release(); dRanges.release();
      if (!ok) { setError(std::string(name) + ": device error"); return -1; }
    }
    int differ = inPlaceDiffer;
    for (size_t i = 0; i < got.size(); i++) differ += got[i] != want[i];
    for (uint32_t i = 0; i < tableCount; i++) for (int b = 0; b < 4; b++) differ += ((gotTable[i] >> (8 * b)) & 0xffu) != ((wantTable[i] >> (8 * b)) & 0xffu);
    return differ;
  } catch (const std::exception& e) { setError(std::string(name) + ": " + e.what()); return -1; }
}
extern "C" int giCDebugCompactRanges(uint32_t kind, const void* records, uint32_t recordCount, const GiCDebugCompactRange* ranges, uint32_t rangeCount, uint32_t* outInfo)
{ return debugCompactRanges("giCDebugCompactRanges", true, kind, records, recordCount, ranges, rangeCount, outInfo); }
extern "C" int giCDebugCompactRangesHost(uint32_t kind, const void* records, uint32_t recordCount, const GiCDebugCompactRange* ranges, uint32_t rangeCount, uint32_t* outInfo)
{ return debugCompactRanges("giCDebugCompactRangesHost", false, kind, records, recordCount, ranges, rangeCount, outInfo); }

extern "C" int giCDebugSceneInstanceUpdateCount(const GiCScene* scene, uint64_t* out)
{
  GiCScene* s = const_cast<GiCScene*>(scene);
  if (!s || !out) { setError("giCDebugSceneInstanceUpdateCount: bad arguments"); return GI_C_ERROR; }
  std::lock_guard<std::mutex> guard(s->mutex);
  for (int k = 0; k < 4; k++) out[k] = s->instanceCounts[k];
  return GI_C_OK;
}

extern "C" int giCDebugSceneResyncCount(const GiCScene* scene, uint64_t* outCount)
{
  GiCScene* s = const_cast<GiCScene*>(scene);
  if (!s || !outCount) { setError("giCDebugSceneResyncCount: bad arguments"); return GI_C_ERROR; }
  std::lock_guard<std::mutex> guard(s->mutex);
  *outCount = s->resyncCount;
  return GI_C_OK;
}

// giCDebugPathWalkStats: how the closest-hit loops of the fused kernel's trips ran in the last render of a counting build (Counters::phaseTrips, walkStepTrips,
// walkStepLanes, walkFewLaneSteps of the primary device; gi_path.hip).  All zero after a render that did not run k_path with counters.
extern "C" int giCDebugPathWalkStats(const GiCScene* scene, uint64_t* out)
{
  GiCScene* s = const_cast<GiCScene*>(scene);
  if (!s || !out) { setError("giCDebugPathWalkStats: bad arguments"); return GI_C_ERROR; }
  std::lock_guard<std::mutex> guard(s->mutex);
  for (int k = 0; k < 18; k++) out[k] = s->pathWalkStats[k];
  return GI_C_OK;
}

// giCDebugPathLobeStats: the glossy-lobe counters of the fused kernel's shade phase and what its lobe parking did in the last render of a counting build
// (Counters::lobeStats of the primary device; gi_path.hip).  All zero after a render that did not run k_path with counters.
extern "C" int giCDebugPathLobeStats(const GiCScene* scene, uint64_t* out)
{
  GiCScene* s = const_cast<GiCScene*>(scene);
  if (!s || !out) { setError("giCDebugPathLobeStats: bad arguments"); return GI_C_ERROR; }
  std::lock_guard<std::mutex> guard(s->mutex);
  for (int k = 0; k < 9; k++) out[k] = s->pathLobeStats[k];
  return GI_C_OK;
}

// giCDebugPathRingStats: what the triangle ring of the fused kernel's closest-hit loops did in the last render of a counting build (Counters::ringStats of the
// primary device; gi_path.hip).  All zero after a render that did not run k_path with counters.
extern "C" int giCDebugPathRingStats(const GiCScene* scene, uint64_t* out)
{
  GiCScene* s = const_cast<GiCScene*>(scene);
  if (!s || !out) { setError("giCDebugPathRingStats: bad arguments"); return GI_C_ERROR; }
  std::lock_guard<std::mutex> guard(s->mutex);
  for (int k = 0; k < 5; k++) out[k] = s->pathRingStats[k];
  return GI_C_OK;
}

// giCDebugTraversalStackHigh: how full the per-lane traversal stack got in the last render of a counting build (Counters::stackHigh of the primary device, raised
// by the COUNT instantiations of k_path, k_trace and k_trace_dyn: gi_traversal.h trav_node), the rows of the variant that ran and the spill entries used.  All
// zero after a render that did not count.
extern "C" int giCDebugTraversalStackHigh(const GiCScene* scene, uint32_t* out)
{
  GiCScene* s = const_cast<GiCScene*>(scene);
  if (!s || !out) { setError("giCDebugTraversalStackHigh: bad arguments"); return GI_C_ERROR; }
  std::lock_guard<std::mutex> guard(s->mutex);
  for (int k = 0; k < 4; k++) out[k] = s->traversalStackHigh[k];
  return GI_C_OK;
}

// giCDebugPathLot: where k_path keeps parked hits for a tree of this depth (gi_kernels.h pathLotPlacement) and the dynamic LDS its launch asks for.  Host only.
extern "C" int giCDebugPathLot(uint32_t bvhDepth, uint32_t nodeCount, uint32_t triCount, uint32_t* out)
{
  if (!out) { setError("giCDebugPathLot: bad arguments"); return GI_C_ERROR; }
  const gi::PathLot lot = gi::pathLotPlacement(bvhDepth);
  out[0] = lot.stack; out[1] = lot.row; out[2] = lot.capacity; out[3] = gi::traceLdsBytes(lot.stack, nodeCount, triCount);
  return GI_C_OK;
}

// giCDebugSceneClassState: what picks a render's kernel variants (gi_build.cpp deriveSceneClasses), as the last scene sync left it.  Host only.
extern "C" int giCDebugSceneClassState(const GiCScene* scene, uint32_t* out)
{
  GiCScene* s = const_cast<GiCScene*>(scene);
  if (!s || !out) { setError("giCDebugSceneClassState: bad arguments"); return GI_C_ERROR; }
  std::lock_guard<std::mutex> guard(s->mutex);
  out[0] = s->classMask; out[1] = s->classTextured; out[2] = s->shadeClassMask; out[3] = s->shadeClassTextured; out[4] = s->hasCutouts ? 1u : 0u;
  return GI_C_OK;
}

// giCDebugSceneUpsPlain: the traits of the scene's class-1 materials (gi_build.cpp deriveSceneClasses) as the last scene sync left them, and the traits the
// last render's fused launch was compiled for.  Host only.
extern "C" int giCDebugSceneUpsPlain(const GiCScene* scene, uint32_t* out)
{
  GiCScene* s = const_cast<GiCScene*>(scene);
  if (!s || !out) { setError("giCDebugSceneUpsPlain: bad arguments"); return GI_C_ERROR; }
  std::lock_guard<std::mutex> guard(s->mutex);
  out[0] = s->upsTraits; out[1] = s->upsPlainLaunched;
  return GI_C_OK;
}

// giCDebugUpsTraits: the same rule on a material table alone -- what a scene whose visible meshes use exactly these materials would report.  `derive`: the
// descriptions are a caller's, and their constants are derived as a build derives them; 0: they are derived records already (MaterialRec::p word for word).
// A description's flags are taken as they are (MAT_FLAG_TEXTURED: a record with a bound input).  Host only: no scene.
extern "C" int giCDebugUpsTraits(const GiCMaterialDesc* descs, uint32_t count, int derive, uint32_t* out)
{
  if (!out || (count && !descs)) { setError("giCDebugUpsTraits: bad arguments"); return GI_C_ERROR; }
  uint32_t ups = UPS_NOCOAT; bool any = false;
  for (uint32_t i = 0; i < count; i++) {
    MaterialRec m{}; m.klass = descs[i].klass; m.flags = descs[i].flags; memcpy(m.p, descs[i].p, sizeof(m.p));
    if (derive) deriveMaterialConstants(m);
    if (m.klass != GI_C_MAT_USD_PREVIEW_SURFACE) continue;
    any = true; ups &= upsTraitsOf(m);
  }
  *out = any ? ups : 0u;
  return GI_C_OK;
}

// ---- the TLAS builders of an edit (gi_tlas_build.h): giCDebugBuildTlasHost / giCDebugBuildTlas ---------------------------------------------------------------
namespace {

// the dequantised box of slot s: the fp32 planes the traversal evaluates
void tlasSlotBox(const Node8& nd, int s, float box[6])
{
  for (int a = 0; a < 3; a++) {
    const float scale = ldexpf(1.0f, (int)nd.e[a] - 127);
    box[a] = nd.p[a] + (float)nd.qlo[a][s] * scale; box[3 + a] = nd.p[a] + (float)nd.qhi[a][s] * scale;
  }
}
bool tlasSlotUsed(const Node8& nd, int s) { return nd.meta[s] != 0; }

// the SAH model cost of a tree over its dequantised slot boxes: root area + per internal slot its area + per leaf slot cPrim * items * its area
double tlasModelCost(const std::vector<Node8>& nodes)
{
  if (nodes.empty()) return 0.0;
  double cost = 0.0;
  float root[6] = {3.0e38f, 3.0e38f, 3.0e38f, -3.0e38f, -3.0e38f, -3.0e38f}; bool any = false;
  for (size_t i = 0; i < nodes.size(); i++) {
    const Node8& nd = nodes[i];
    for (int s = 0; s < 8; s++) {
      if (!tlasSlotUsed(nd, s)) continue;
      float b[6]; tlasSlotBox(nd, s, b);
      if (i == 0) { any = true; for (int a = 0; a < 3; a++) { root[a] = std::min(root[a], b[a]); root[3 + a] = std::max(root[3 + a], b[3 + a]); } }
      const double area = (double)tlas_box_area(b);
      if (nd.imask & (1u << s)) cost += area;
      else { uint32_t cnt = 0; for (uint32_t u = nd.meta[s] >> 5; u; u >>= 1) cnt += u & 1u; cost += area * (double)kBvhCPrim * (double)cnt; }
    }
  }
  if (any) cost += (double)tlas_box_area(root);
  return cost;
}

// the rules of giCDebugBuildTlasHost; `depth` is the builder's answer
int tlasViolations(const float* boxes6, uint32_t n, const std::vector<Node8>& nodes, const std::vector<uint32_t>& items, uint32_t depth, uint32_t budget)
{
  int bad = 0;
  std::vector<uint32_t> inactive; uint32_t A = 0;
  for (uint32_t i = 0; i < n; i++) { if (tlas_box_active(boxes6 + 6u * (size_t)i)) A++; else inactive.push_back(i); }
  if (items.size() != n) return 1 + (int)n;
  std::vector<uint32_t> seen(n, 0u);
  for (uint32_t k = 0; k < A; k++) { const uint32_t id = items[k]; if (id >= n || !tlas_box_active(boxes6 + 6u * (size_t)id)) bad++; else seen[id]++; }
  for (uint32_t i = 0; i < n; i++) if (tlas_box_active(boxes6 + 6u * (size_t)i) && seen[i] != 1u) bad++;
  for (uint32_t k = A; k < n; k++) if (items[k] != inactive[k - A]) bad++;
  if (nodes.empty()) return bad + 1;
  if (depth > budget || depth == 0u) bad++;
  // breadth-first walk: the next internal child must be the next node; every item inside every ancestor slot
  struct Anc { float box[6]; };
  std::vector<std::vector<Anc>> chain(nodes.size()); std::vector<uint32_t> levelOf(nodes.size(), 0u);
  uint32_t nextNode = 1, itemsNamed = 0, maxLevel = 1; std::vector<uint32_t> named(n, 0u);
  levelOf[0] = 1;
  for (uint32_t i = 0; i < nodes.size(); i++) {
    const Node8& nd = nodes[i];
    if (i >= nextNode) { bad++; break; } // (a node nothing names)
    maxLevel = std::max(maxLevel, levelOf[i]);
    uint32_t child = nd.childBase;
    for (int s = 0; s < 8; s++) {
      if (!tlasSlotUsed(nd, s)) { if (nd.imask & (1u << s)) bad++; continue; }
      Anc me; tlasSlotBox(nd, s, me.box);
      if (nd.imask & (1u << s)) {
        if (child != nextNode || child >= nodes.size()) { bad++; child++; continue; }
        chain[child] = chain[i]; chain[child].push_back(me); levelOf[child] = levelOf[i] + 1u;
        child++; nextNode++;
        continue;
      }
      uint32_t cnt = 0; for (uint32_t u = nd.meta[s] >> 5; u; u >>= 1) cnt += u & 1u;
      const uint32_t first = nd.triBase + (nd.meta[s] & 31u);
      if (cnt == 0u || cnt > kBvhMaxLeaf || (size_t)first + cnt > A) { bad++; continue; }
      for (uint32_t k = 0; k < cnt; k++) {
        const uint32_t id = items[first + k];
        if (id >= n) { bad++; continue; }
        named[id]++; itemsNamed++;
        const float* b = boxes6 + 6u * (size_t)id;
        auto inside = [&](const float* o) { for (int a = 0; a < 3; a++) if (!(o[a] <= b[a] && b[3 + a] <= o[3 + a])) return false; return true; };
        if (!inside(me.box)) bad++;
        for (const Anc& an : chain[i]) if (!inside(an.box)) bad++;
      }
    }
  }
  if (nextNode != nodes.size()) bad++;
  if (itemsNamed != A) bad++;
  for (uint32_t i = 0; i < n; i++) if (tlas_box_active(boxes6 + 6u * (size_t)i) && named[i] != 1u) bad++;
  if (maxLevel != depth && A != 0u) bad++;
  return bad;
}

void tlasFillOut(const float* boxes6, uint32_t count, const std::vector<Node8>& nodes, const TlasBuildInfo& info, double* out)
{
  Bvh8 ref; std::vector<uint32_t> order;
  buildBvh8Boxes(boxes6, count, ref, order);
  out[0] = (double)info.nodeCount; out[1] = (double)info.maxDepth; out[2] = (double)info.passes; out[3] = tlasModelCost(nodes); out[4] = tlasModelCost(ref.nodes);
  out[5] = (double)info.hostWaits; out[6] = (double)ref.maxDepth; out[7] = (double)info.active;
}

} // namespace

extern "C" int giCDebugBuildTlasHost(const float* boxes6, uint32_t count, uint32_t depthBudget, uint32_t radius, double* out)
{
  if ((count && !boxes6) || !out) { setError("giCDebugBuildTlasHost: bad arguments"); return -1; }
  try {
    for (int k = 0; k < 8; k++) out[k] = 0.0;
    std::vector<Node8> nodes; std::vector<uint32_t> items; TlasBuildInfo info;
    const int rc = buildTlasHost(boxes6, count, depthBudget, radius, nodes, items, info);
    if (rc == TLAS_BUILD_TOO_DEEP) return GI_C_TLAS_BUILD_TOO_DEEP;
    if (rc != TLAS_BUILD_OK) { setError(std::string("giCDebugBuildTlasHost: ") + info.error); return -1; }
    tlasFillOut(boxes6, count, nodes, info, out);
    return tlasViolations(boxes6, count, nodes, items, info.maxDepth, std::min(depthBudget, kTlasMaxBudget));
  } catch (const std::exception& e) { setError(std::string("giCDebugBuildTlasHost: ") + e.what()); return -1; }
}

extern "C" int giCDebugBuildTlas(const float* boxes6, uint32_t count, uint32_t depthBudget, uint32_t radius, double* out)
{
  if (!g_ctx.initialized || (count && !boxes6) || !out) { setError("giCDebugBuildTlas: bad arguments"); return -1; }
  try {
    for (int k = 0; k < 8; k++) out[k] = 0.0;
    std::vector<Node8> nodes, hostNodes; std::vector<uint32_t> items, hostItems; TlasBuildInfo info, hostInfo;
    TlasBuildWorkspace ws;
    const int rc = buildTlasDevice(ws, g_ctx.stream, boxes6, count, depthBudget, radius, nodes, items, info);
    ws.release();
    const int hostRc = buildTlasHost(boxes6, count, depthBudget, radius, hostNodes, hostItems, hostInfo);
    out[5] = (double)info.hostWaits;
    if (rc == TLAS_BUILD_TOO_DEEP) { if (hostRc != TLAS_BUILD_TOO_DEEP) { setError("giCDebugBuildTlas: too deep on the device alone"); return -1; } return GI_C_TLAS_BUILD_TOO_DEEP; }
    if (rc != TLAS_BUILD_OK) { setError(std::string("giCDebugBuildTlas: ") + info.error); return -1; }
    if (hostRc != TLAS_BUILD_OK) { setError("giCDebugBuildTlas: the host form failed where the device did not"); return -1; }
    tlasFillOut(boxes6, count, nodes, info, out);
    int differ = tlasViolations(boxes6, count, nodes, items, info.maxDepth, std::min(depthBudget, kTlasMaxBudget));
    if (nodes.size() != hostNodes.size()) differ += 1 + (int)std::max(nodes.size(), hostNodes.size()) - (int)std::min(nodes.size(), hostNodes.size());
    for (size_t i = 0; i < std::min(nodes.size(), hostNodes.size()); i++) if (memcmp(&nodes[i], &hostNodes[i], sizeof(Node8)) != 0) differ++;
    if (items.size() != hostItems.size()) differ++;
    for (size_t i = 0; i < std::min(items.size(), hostItems.size()); i++) if (items[i] != hostItems[i]) differ++;
    if (info.maxDepth != hostInfo.maxDepth || info.passes != hostInfo.passes || info.active != hostInfo.active) differ++;
    return differ;
  } catch (const std::exception& e) { setError(std::string("giCDebugBuildTlas: ") + e.what()); return -1; }
}

extern "C" int giCDebugSceneTlasBuildStats(const GiCScene* scene, uint64_t* out)
{
  GiCScene* s = const_cast<GiCScene*>(scene);
  if (!s || !out) { setError("giCDebugSceneTlasBuildStats: bad arguments"); return GI_C_ERROR; }
  std::lock_guard<std::mutex> guard(s->mutex);
  for (int k = 0; k < 16; k++) out[k] = s->tlasBuildStats[k];
  out[13] = s->tlasWorkspace.allocations;
  out[14] = s->host && s->host->two.tlasDeviceBuilt ? 1u : 0u;
  out[15] = s->host && s->host->two.tlasDeviceBuilt ? s->host->two.tlasBuildBudget : 0u;
  return GI_C_OK;
}

// ---- the BLAS builders of GI_C_SCENE_OPTION_BLAS_DEVICE_BUILD (gi_blas_build.h): giCDebugBuildBlasHost / giCDebugBuildBlas / giCDebugSceneBlasBuildStats -------
namespace {

int bytesDiffering(const void* x, const void* y, size_t n) { int d = 0; for (size_t i = 0; i < n; i++) d += ((const uint8_t*)x)[i] != ((const uint8_t*)y)[i]; return d; }

// the rules of giCDebugBuildBlasHost over one tree (the host form's or the device's); fills out[0 .. 14] and returns the violations
int blasBuildChecks(const GiCVertex* vertices, uint32_t vertexCount, const GiCFace* faces, uint32_t nf, uint32_t budget, uint32_t radius, const Bvh8& b,
    const std::vector<uint32_t>& order, const float mlo[3], const float mhi[3], const BlasBuildInfo& info, double* out)
{
  const uint32_t nodeCount = (uint32_t)b.nodes.size();
  std::vector<float> boxes6(6u * (size_t)nf);
  for (uint32_t f = 0; f < nf; f++) {
    float p[3][3], lo[3], hi[3];
    for (int k = 0; k < 3; k++) memcpy(p[k], vertices[faces[f].v_i[k]].pos, 12);
    if (!blas_face_box(p, lo, hi)) for (int a = 0; a < 3; a++) { lo[a] = 3.0e38f; hi[a] = -3.0e38f; }
    for (int a = 0; a < 3; a++) { boxes6[6u * (size_t)f + a] = lo[a]; boxes6[6u * (size_t)f + 3 + a] = hi[a]; }
  }
  Bvh8 ref; std::vector<uint32_t> refOrder; float rlo[3], rhi[3];
  buildMeshBlas(vertices, faces, nf, ref, refOrder, rlo, rhi);
  out[0] = (double)info.nodeCount; out[1] = (double)info.maxDepth; out[2] = (double)info.passes; out[3] = tlasModelCost(b.nodes); out[4] = tlasModelCost(ref.nodes);
  out[5] = (double)info.hostWaits; out[6] = (double)ref.maxDepth; out[7] = (double)info.active; out[14] = (double)std::min(budget, kBlasMaxBudget);
  // [8] the conservative check of gi_blas.h over the mesh's records in the builder's order
  int conservative = 1;
  if (order.size() == nf && nodeCount != 0u) {
    bool inRange = true; for (const uint32_t f : order) if (f >= nf) inRange = false;
    if (inRange) {
      std::vector<BlasTri> tris; tris.reserve(nf);
      for (const uint32_t f : order) tris.push_back(makeBlasTri(vertices, faces, f));
      std::vector<float> under(6u * (size_t)nodeCount, 0.0f); std::vector<uint8_t> seen(std::max(nf, 1u), 0);
      conservative = (int)blasConservativeViolations(b.nodes.data(), nodeCount, 0u, nodeCount, tris.data(), nf, 0u, nf, under.data(), seen.data());
      // [13] a refit over the unchanged points writes the build's bytes
      std::vector<Node8> refitted(b.nodes); std::vector<float> scratch(8u * (size_t)nodeCount, 0.0f);
      blasRefitHost(refitted.data(), nodeCount, 0u, nodeCount, scratch.data(), tris.data(), nf);
      out[13] = (double)bytesDiffering(refitted.data(), b.nodes.data(), (size_t)nodeCount * sizeof(Node8));
    }
  }
  out[8] = (double)conservative;
  // [9] the builder's contract over the boxes
  out[9] = (double)tlasViolations(boxes6.data(), nf, b.nodes, order, b.maxDepth, std::min(budget, kBlasMaxBudget));
  // [10] the level table: maxDepth + 1 entries from 0 to the node count, every internal child one level below its parent
  int levelBad = 0;
  const std::vector<uint32_t>& ls = b.levelStart;
  if (ls.size() != (size_t)b.maxDepth + 1u || ls.empty() || ls.front() != 0u || ls.back() != nodeCount || b.maxDepth != info.maxDepth) levelBad++;
  else {
    for (size_t l = 0; l + 1u < ls.size(); l++) if (!(ls[l] < ls[l + 1u])) levelBad++;
    for (size_t l = 0; l + 1u < ls.size() && !levelBad; l++)
      for (uint32_t i = ls[l]; i < ls[l + 1u]; i++) {
        uint32_t rel = 0;
        for (int s = 0; s < 8; s++) if ((b.nodes[i].imask >> s) & 1u) {
          const uint32_t c = b.nodes[i].childBase + rel++;
          if (l + 2u >= ls.size() || c < ls[l + 1u] || c >= ls[l + 2u]) levelBad++;
        }
      }
  }
  out[10] = (double)levelBad;
  // [11] mlo / mhi against the host builder's
  out[11] = (double)(bytesDiffering(mlo, rlo, 12) + bytesDiffering(mhi, rhi, 12));
  // [12] the generalisation did not move the TLAS builder: the same boxes under a TLAS budget give the same records
  out[12] = 0.0;
  if (budget <= kTlasMaxBudget && nf <= kTlasMaxItems) {
    std::vector<Node8> tn; std::vector<uint32_t> ti; TlasBuildInfo tinfo;
    int differ = 0;
    if (buildTlasHost(boxes6.data(), nf, budget, radius, tn, ti, tinfo) != TLAS_BUILD_OK) differ = 1;
    else {
      if (tn.size() != b.nodes.size() || ti.size() != order.size()) differ++;
      for (size_t i = 0; i < std::min(tn.size(), b.nodes.size()); i++) if (memcmp(&tn[i], &b.nodes[i], sizeof(Node8)) != 0) differ++;
      for (size_t i = 0; i < std::min(ti.size(), order.size()); i++) if (ti[i] != order[i]) differ++;
    }
    out[12] = (double)differ;
  }
  return (int)out[8] + (int)out[9] + (int)out[10] + (int)out[11] + (int)out[13] + (out[12] > 0.0 ? 1 : 0);
}

bool blasDebugArgsOk(const GiCVertex* vertices, uint32_t vertexCount, const GiCFace* faces, uint32_t faceCount, const double* out)
{
  return out && (vertices || vertexCount == 0u) && (faces || faceCount == 0u);
}

} // namespace

extern "C" int giCDebugBuildBlasHost(const GiCVertex* vertices, uint32_t vertexCount, const GiCFace* faces, uint32_t faceCount, uint32_t depthBudget, uint32_t radius,
    double* out)
{
  if (!blasDebugArgsOk(vertices, vertexCount, faces, faceCount, out)) { setError("giCDebugBuildBlasHost: bad arguments"); return -1; }
  try {
    for (int k = 0; k < 16; k++) out[k] = 0.0;
    Bvh8 b; std::vector<uint32_t> order; float mlo[3], mhi[3]; BlasBuildInfo info;
    const int rc = buildBlasHost(vertices, vertexCount, faces, faceCount, depthBudget, radius, b, order, mlo, mhi, info);
    if (rc == TLAS_BUILD_TOO_DEEP) return GI_C_TLAS_BUILD_TOO_DEEP;
    if (rc != TLAS_BUILD_OK) { setError(std::string("giCDebugBuildBlasHost: ") + info.error); return -1; }
    return blasBuildChecks(vertices, vertexCount, faces, faceCount, depthBudget, radius, b, order, mlo, mhi, info, out);
  } catch (const std::exception& e) { setError(std::string("giCDebugBuildBlasHost: ") + e.what()); return -1; }
}

extern "C" int giCDebugBuildBlas(const GiCVertex* vertices, uint32_t vertexCount, const GiCFace* faces, uint32_t faceCount, uint32_t depthBudget, uint32_t radius,
    double* out)
{
  if (!g_ctx.initialized || !blasDebugArgsOk(vertices, vertexCount, faces, faceCount, out)) { setError("giCDebugBuildBlas: bad arguments"); return -1; }
  try {
    for (int k = 0; k < 16; k++) out[k] = 0.0;
    Bvh8 b, hb; std::vector<uint32_t> order, horder; float mlo[3], mhi[3], hlo[3], hhi[3]; BlasBuildInfo info, hinfo;
    TlasBuildWorkspace ws;
    const int rc = buildBlasDevice(ws, g_ctx.stream, vertices, vertexCount, faces, faceCount, depthBudget, radius, b, order, mlo, mhi, info);
    ws.release();
    const int hostRc = buildBlasHost(vertices, vertexCount, faces, faceCount, depthBudget, radius, hb, horder, hlo, hhi, hinfo);
    out[5] = (double)info.hostWaits;
    if (rc == TLAS_BUILD_TOO_DEEP) { if (hostRc != TLAS_BUILD_TOO_DEEP) { setError("giCDebugBuildBlas: too deep on the device alone"); return -1; } return GI_C_TLAS_BUILD_TOO_DEEP; }
    if (rc != TLAS_BUILD_OK) { setError(std::string("giCDebugBuildBlas: ") + info.error); return -1; }
    if (hostRc != TLAS_BUILD_OK) { setError("giCDebugBuildBlas: the host form failed where the device did not"); return -1; }
    const int violations = blasBuildChecks(vertices, vertexCount, faces, faceCount, depthBudget, radius, b, order, mlo, mhi, info, out);
    int differ = 0;
    if (b.nodes.size() != hb.nodes.size()) differ += (int)sizeof(Node8) * (int)(std::max(b.nodes.size(), hb.nodes.size()) - std::min(b.nodes.size(), hb.nodes.size()));
    differ += bytesDiffering(b.nodes.data(), hb.nodes.data(), std::min(b.nodes.size(), hb.nodes.size()) * sizeof(Node8));
    if (order.size() != horder.size()) differ += 4;
    differ += bytesDiffering(order.data(), horder.data(), std::min(order.size(), horder.size()) * sizeof(uint32_t));
    differ += bytesDiffering(mlo, hlo, 12) + bytesDiffering(mhi, hhi, 12);
    if (b.levelStart != hb.levelStart || b.maxDepth != hb.maxDepth || info.passes != hinfo.passes || info.active != hinfo.active) differ++;
    out[15] = (double)differ;
    return differ + violations;
  } catch (const std::exception& e) { setError(std::string("giCDebugBuildBlas: ") + e.what()); return -1; }
}

extern "C" int giCDebugSceneBlasBuildStats(const GiCScene* scene, uint64_t* out)
{
  GiCScene* s = const_cast<GiCScene*>(scene);
  if (!s || !out) { setError("giCDebugSceneBlasBuildStats: bad arguments"); return GI_C_ERROR; }
  std::lock_guard<std::mutex> guard(s->mutex);
  for (int k = 0; k < 16; k++) out[k] = s->blasBuildStats[k];
  uint64_t deviceBuilt = 0;
  if (s->host) for (const uint32_t budget : s->host->two.meshBlasBudget) deviceBuilt += budget != 0u;
  out[15] = deviceBuilt;
  return GI_C_OK;
}

// giCDebugSampleMoments / giCDebugSampleMomentsHost: k_moments (onDevice) or its host form (gi_moments.h) over the caller's per-sample buffer.  The tile is the
// whole image; the miss constant reaches the kernel the way a render's does, through retired_miss_sample(U): the background IS the constant and nothing clamps
static int debugSampleMoments(const char* name, bool onDevice, const GiCDebugMomentsDesc* d, const float* samples, const float* prevM, const uint32_t* rect,
    const float* missRgb, float* outM)
{
  auto refuse = [&](const char* what) { setError(std::string(name) + ": " + what); return GI_C_ERROR; };
  if (onDevice && !g_ctx.initialized) return refuse("called before giCInitialize");
  if (!d || !samples || !outM) return refuse("a required argument is NULL");
  if (d->width == 0u || d->rows == 0u || d->bufferSamples == 0u || d->count == 0u) return refuse("an empty tile, buffer or slice");
  if ((uint64_t)d->first + d->count > d->bufferSamples) return refuse("the slice does not lie inside the buffer");
  const uint64_t pixels64 = (uint64_t)d->width * d->rows;
  if (d->width > 65535u || d->rows > 65535u || pixels64 * d->bufferSamples > 0xffffffffull) return refuse("more than 2^32 - 1 records, or a side above 65535");
  if (rect) {
    if (!missRgb) return refuse("a miss rectangle without its constant");
    if (rect[0] > rect[2] || rect[1] > rect[3] || rect[2] > d->width || rect[3] > d->rows) return refuse("the miss rectangle does not lie inside the image");
    for (int a = 0; a < 3; a++) if (!(missRgb[a] >= 0.0f) || std::signbit(missRgb[a]) || !std::isfinite(missRgb[a])) return refuse("the miss constant must be finite and not negative");
  }
  try {
    const uint32_t pixels = (uint32_t)pixels64;
    const size_t records = (size_t)pixels * d->bufferSamples;
    MomentsFold F{};
    F.pixelCount = pixels; F.imageWidth = d->width; F.rowBegin = 0u; F.rowStride = 1u;
    F.bufferSamples = d->bufferSamples; F.first = d->first; F.count = d->count; F.pixelMajor = d->pixelMajor ? 1u : 0u; F.continues = prevM ? 1u : 0u;
    if (rect) { F.missRect = 1u; F.rectX0 = rect[0]; F.rectTy0 = rect[1]; F.rectX1 = rect[2]; F.rectTy1 = rect[3]; for (int a = 0; a < 3; a++) F.missSample[a] = missRgb[a]; }
    if (!onDevice) {
      std::vector<F4> buf(records), M(pixels);
      memcpy(static_cast<void*>(buf.data()), samples, records * sizeof(F4));
      if (prevM) memcpy(static_cast<void*>(M.data()), prevM, (size_t)pixels * sizeof(F4));
      else memset(static_cast<void*>(M.data()), 0xa5, (size_t)pixels * sizeof(F4)); // (a fold from zero must not look at it)
      momentsHost(F, buf.data(), M.data());
      memcpy(outM, M.data(), (size_t)pixels * sizeof(F4));
      return GI_C_OK;
    }
    FrameUniforms U{};
    U.pixelCount = pixels; U.imageWidth = d->width; U.imageHeight = d->rows; U.rowBegin = 0u; U.rowStride = 1u;
    U.maxSampleValue = INFINITY;
    if (rect) { U.flags |= FLAG_MISS_RECT; U.rectX0 = rect[0]; U.rectTy0 = rect[1]; U.rectX1 = rect[2]; U.rectTy1 = rect[3]; for (int a = 0; a < 3; a++) U.background[a] = missRgb[a]; }
    DeviceBuffer<F4> dBuf, dM;
    hipStream_t st = g_ctx.stream;
    std::vector<uint8_t> fill((size_t)pixels * sizeof(F4), 0xa5);
    bool ok = hipSetDevice(g_ctx.device) == hipSuccess && dBuf.alloc(records) == GI_C_OK && dM.alloc(pixels) == GI_C_OK;
    ok = ok && hipMemcpyAsync(dBuf.ptr, samples, records * sizeof(F4), hipMemcpyHostToDevice, st) == hipSuccess &&
        hipMemcpyAsync(dM.ptr, prevM ? static_cast<const void*>(prevM) : static_cast<const void*>(fill.data()), (size_t)pixels * sizeof(F4), hipMemcpyHostToDevice, st) == hipSuccess;
    if (ok) { launchMoments(st, U, dBuf.ptr, dM.ptr, d->bufferSamples, d->first, d->count, d->pixelMajor != 0u, prevM != nullptr); ok = hipGetLastError() == hipSuccess; }
    ok = ok && hipMemcpyAsync(outM, dM.ptr, (size_t)pixels * sizeof(F4), hipMemcpyDeviceToHost, st) == hipSuccess;
    ok = hipStreamSynchronize(st) == hipSuccess && ok;
    dBuf.release(); dM.release();
    if (!ok) return refuse("device error");
    return GI_C_OK;
  } catch (const std::exception& e) { setError(std::string(name) + ": " + e.what()); return GI_C_ERROR; }
}
extern "C" int giCDebugSampleMoments(const GiCDebugMomentsDesc* desc, const float* samples, const float* prevM, const uint32_t* rect, const float* missRgb, float* outM)
{ return debugSampleMoments("giCDebugSampleMoments", true, desc, samples, prevM, rect, missRgb, outM); }
extern "C" int giCDebugSampleMomentsHost(const GiCDebugMomentsDesc* desc, const float* samples, const float* prevM, const uint32_t* rect, const float* missRgb, float* outM)
{ return debugSampleMoments("giCDebugSampleMomentsHost", false, desc, samples, prevM, rect, missRgb, outM); }

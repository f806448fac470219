// gi_bvh_build.hip -- the scene BVH8 built on the device (GI_C_SCENE_OPTION_BVH_BUILD = 1).  Output: the format bvh8.cpp writes
// (80-byte Node8 breadth-first, leaf-ordered TriRec, inactive triangles behind), so the traversal kernels cannot tell the builders apart -- and, under the
// traversal contract (accept tMin < t < tBest, ties to the lower scene-order id, conservative boxes), images do not depend on the tree.
//
//   1. k_bvh_boxes    padded triangle boxes + the inactive rule of bvh8.cpp prepareRange; per-block centroid bounds (k_bvh_bounds finishes the reduction)
//   2. k_bvh_morton   63-bit Morton codes of the centroids (inactive: all ones), stable radix sort of (code, scene-order id): ties stay in id order
//   3. PLOC           Meister & Bittner 2018, implemented from the paper: every cluster finds its nearest neighbour (surface area of the union) within
//                     +-16 positions (GATLING_OPTIONS ploc_radius), mutual pairs merge, the cluster list is compacted by a scan -- until one cluster is left.  BVH2 node indices come from
//                     the scan (leaves 0 .. A-1 in Morton order, internal nodes A .. 2A-2 in merge order), never from an atomic.
//   4. collapse DP    bvh8.cpp's cost-optimal 8-wide collapse (Ylitie, Karras, Laine 2017, section 3.1): filled bottom-up inside the merge kernel -- a
//                     merged node's children were completed by earlier launches, so no arrival counter (and no cross-workgroup hand-off) is needed
//   5. emission       top down, one breadth-first level per pair of launches: k_bvh_plan gathers each node's children through the DP and assigns slots
//                     (bvh8.cpp's greedy octant rule), a scan hands out childBase / triBase, k_bvh_write quantises (exponentFor, outward rounding and the
//                     fix-up loops of bvh8.cpp) and gathers the TriRec / face-id records.  The host reads one 8-byte counter per level.
//
// Determinism: every output position is a function of the input (scans, a stable sort, index-ordered tie-breaks), so the same scene gives the same bytes on
// every run and every device.
#include <cstring> // (before rocprim: its texture iterator calls memset in host code)
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#include <chrono>
#include <vector>

#include "gi_bvh_build.h"
#include "gi_options.h"
#define GI_BVH_STAGE_KERNELS
#include "gi_bvh_stages.h" // the arithmetic and the stage kernels shared with gi_tlas_build.hip

namespace gi {
namespace {

constexpr uint32_t kBlock = kStageBlock;
constexpr uint32_t kMaxLeaf = kBvhMaxLeaf;

__device__ inline bool usable(float x) { return fabsf(x) <= 1.0e18f; } // bvh8.cpp Builder::usable (false for NaN)

// ---- 1. boxes -----------------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void k_bvh_boxes(const TriRec* __restrict__ tris, uint32_t n, float4* __restrict__ triLo, float4* __restrict__ triHi,
    float4* __restrict__ blockLo, float4* __restrict__ blockHi, uint32_t* __restrict__ blockAlive)
{
  __shared__ float4 sLo[kBlock], sHi[kBlock]; __shared__ uint32_t sAlive[kBlock];
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  float4 cLo = make_float4(3.0e38f, 3.0e38f, 3.0e38f, 0.0f), cHi = make_float4(-3.0e38f, -3.0e38f, -3.0e38f, 0.0f);
  uint32_t alive = 0;
  if (i < n) {
    const TriRec t = tris[i];
    float lo[3], hi[3]; bool dead = false;
    for (int a = 0; a < 3; a++) {
      const float p1 = t.v0[a] + t.e1[a], p2 = t.v0[a] + t.e2[a];
      if (!usable(t.v0[a]) || !usable(p1) || !usable(p2)) dead = true;
      lo[a] = fminf(fminf(fminf(3.0e38f, t.v0[a]), p1), p2); hi[a] = fmaxf(fmaxf(fmaxf(-3.0e38f, t.v0[a]), p1), p2);
    }
    float4 bl = make_float4(3.0e38f, 3.0e38f, 3.0e38f, 0.0f), bh = make_float4(-3.0e38f, -3.0e38f, -3.0e38f, 0.0f);
    if (!dead) {
      float c[3];
      for (int a = 0; a < 3; a++) { // bvh8.cpp prepareRange: 2^-20 relative pad
        const float mag = fmaxf(fabsf(lo[a]), fabsf(hi[a])) + (hi[a] - lo[a]);
        const float pad = mag * 9.5367431640625e-7f + 1.0e-30f;
        lo[a] -= pad; hi[a] += pad; c[a] = 0.5f * (lo[a] + hi[a]);
      }
      bl = make_float4(lo[0], lo[1], lo[2], 0.0f); bh = make_float4(hi[0], hi[1], hi[2], 0.0f);
      cLo = make_float4(c[0], c[1], c[2], 0.0f); cHi = cLo; alive = 1;
    }
    triLo[i] = bl; triHi[i] = bh;
  }
  stage_block_bounds(cLo, cHi, alive, sLo, sHi, sAlive, blockLo, blockHi, blockAlive);
}

// ---- 3. PLOC + 4. collapse DP (gi_bvh_stages.h) ---------------------------------------------------------------------------------------------------------
// BVH2 leaves 0 .. A-1: the sorted active triangles
__global__ __launch_bounds__(kBlock) void k_bvh_leaves(const uint32_t* __restrict__ sortedIds, uint32_t A, const float4* __restrict__ triLo,
    const float4* __restrict__ triHi, float4* __restrict__ nLo, float4* __restrict__ nHi, uint32_t* __restrict__ total, Dp* __restrict__ dp,
    uint32_t* __restrict__ clusters)
{
  const uint32_t k = blockIdx.x * kBlock + threadIdx.x;
  if (k >= A) return;
  const uint32_t id = sortedIds[k];
  const float4 lo = triLo[id], hi = triHi[id];
  nLo[k] = lo; nHi[k] = hi; total[k] = 1u; clusters[k] = k;
  Dp d; bvh_dp_leaf(d, box_area(lo, hi)); dp[k] = d;
}

__global__ __launch_bounds__(kBlock) void k_ploc_nn(const uint32_t* __restrict__ clusters, uint32_t m, uint32_t radius, const float4* __restrict__ nLo,
    const float4* __restrict__ nHi, uint32_t* __restrict__ nn)
{
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= m) return;
  const uint32_t ci = clusters[i];
  const float4 lo = nLo[ci], hi = nHi[ci];
  const uint32_t j0 = i > radius ? i - radius : 0u, j1 = min(m - 1u, i + radius);
  float bestD = 3.4e38f; uint32_t bestH = 0xffffffffu, best = 0xffffffffu;
  for (uint32_t j = j0; j <= j1; j++) {
    if (j == i) continue;
    const uint32_t cj = clusters[j];
    const float d = box_area(min4(lo, nLo[cj]), max4(hi, nHi[cj]));
    bvh_nn_consider(i, j, d, bestD, bestH, best);
  }
  nn[i] = best;
}
// flags[i] = (merges here << 32) | (cluster survives here): a mutual pair merges into its lower position
__global__ __launch_bounds__(kBlock) void k_ploc_flags(const uint32_t* __restrict__ nn, uint32_t m, uint64_t* __restrict__ flags)
{
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= m) return;
  const uint32_t j = nn[i];
  const bool mutual = j < m && nn[j] == i;
  flags[i] = bvh_ploc_flags(i, j, mutual);
}
__global__ __launch_bounds__(kBlock) void k_ploc_merge(const uint32_t* __restrict__ clusters, uint32_t m, const uint32_t* __restrict__ nn,
    const uint64_t* __restrict__ flags, const uint64_t* __restrict__ incl, uint32_t nodeBase, float4* __restrict__ nLo, float4* __restrict__ nHi,
    uint32_t* __restrict__ left, uint32_t* __restrict__ right, uint32_t* __restrict__ total, Dp* __restrict__ dp, uint32_t* __restrict__ next)
{
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= m) return;
  const uint64_t f = flags[i], ex = incl[i] - f;
  if (!(f & 1ull)) return;
  const uint32_t keepAt = (uint32_t)(ex & 0xffffffffull);
  if (!(f >> 32)) { next[keepAt] = clusters[i]; return; }
  const uint32_t node = nodeBase + (uint32_t)(ex >> 32);
  const uint32_t a = clusters[i], b = clusters[nn[i]];
  const float4 lo = min4(nLo[a], nLo[b]), hi = max4(nHi[a], nHi[b]);
  const uint32_t t = total[a] + total[b];
  nLo[node] = lo; nHi[node] = hi; left[node] = a; right[node] = b; total[node] = t;
  const Dp L = dp[a], R = dp[b];
  Dp d; bvh_dp_internal(d, L, R, box_area(lo, hi), t); dp[node] = d;
  next[keepAt] = node;
}

// ---- 5. emission --------------------------------------------------------------------------------------------------------------------------------------
struct Tree2 { const float4* lo; const float4* hi; const uint32_t* left; const uint32_t* right; const uint32_t* total; const Dp* dp; uint32_t A; };

__global__ __launch_bounds__(kBlock) void k_bvh_plan(Tree2 T, const uint32_t* __restrict__ level, uint32_t m, bool rootLevel, Plan* __restrict__ plans,
    uint64_t* __restrict__ counts)
{
  const uint32_t li = blockIdx.x * kBlock + threadIdx.x;
  if (li >= m) return;
  const uint32_t n2 = level[li];
  uint32_t ch[8]; bool chLeaf[8]; int n = 0;
  if (n2 < T.A || (rootLevel && T.total[n2] <= kMaxLeaf)) { ch[0] = n2; chLeaf[0] = true; n = 1; } // a root that is itself a leaf (bvh8.cpp: level 0 only)
  else n = bvh_gather_optimal(T.left, T.right, n2, [&](uint32_t x, bool) -> const Dp& { return T.dp[x]; }, ch, chLeaf);
  // node box + slot assignment (greedy max of the centroid projection on the slot's octant direction)
  float4 nbLo = make_float4(3.0e38f, 3.0e38f, 3.0e38f, 0.0f), nbHi = make_float4(-3.0e38f, -3.0e38f, -3.0e38f, 0.0f);
  for (int i = 0; i < n; i++) { nbLo = min4(nbLo, T.lo[ch[i]]); nbHi = max4(nbHi, T.hi[ch[i]]); }
  const float center[3] = {0.5f * (nbLo.x + nbHi.x), 0.5f * (nbLo.y + nbHi.y), 0.5f * (nbLo.z + nbHi.z)};
  float clo[8][3], chi[8][3];
  for (int i = 0; i < n; i++) {
    const float4 bl = T.lo[ch[i]], bh = T.hi[ch[i]];
    clo[i][0] = bl.x; clo[i][1] = bl.y; clo[i][2] = bl.z; chi[i][0] = bh.x; chi[i][1] = bh.y; chi[i][2] = bh.z;
  }
  int slotOf[8];
  bvh_assign_slots(n, clo, chi, center, slotOf);
  Plan P;
  for (int s = 0; s < 8; s++) { P.childInSlot[s] = -1; P.ch[s] = 0; }
  uint32_t internal = 0, trisHere = 0; P.leafMask = 0; P.n = (uint8_t)n; P.pad[0] = P.pad[1] = 0;
  P.lo[0] = nbLo.x; P.lo[1] = nbLo.y; P.lo[2] = nbLo.z; P.hi[0] = nbHi.x; P.hi[1] = nbHi.y; P.hi[2] = nbHi.z;
  for (int i = 0; i < n; i++) {
    P.ch[i] = ch[i]; P.childInSlot[slotOf[i]] = (int8_t)i;
    if (chLeaf[i]) { P.leafMask |= (uint8_t)(1u << i); trisHere += T.total[ch[i]]; } else internal++;
  }
  plans[li] = P;
  counts[li] = ((uint64_t)internal << 32) | trisHere;
}

__global__ __launch_bounds__(kBlock) void k_bvh_write(Tree2 T, const uint32_t* __restrict__ level, uint32_t m, uint32_t levelStart,
    const Plan* __restrict__ plans, const uint64_t* __restrict__ counts, const uint64_t* __restrict__ incl, uint32_t nodeEnd, uint32_t triStart,
    const uint32_t* __restrict__ sortedIds, const TriRec* __restrict__ inTris, const int32_t* __restrict__ inFace, Node8* __restrict__ nodes,
    TriRec* __restrict__ outTris, int32_t* __restrict__ outFace, uint32_t* __restrict__ nextLevel)
{
  const uint32_t li = blockIdx.x * kBlock + threadIdx.x;
  if (li >= m) return;
  const Plan P = plans[li];
  const uint64_t ex = incl[li] - counts[li];
  const uint32_t childBase = nodeEnd + (uint32_t)(ex >> 32), triBase = triStart + (uint32_t)(ex & 0xffffffffull);
  Node8 node; memset(&node, 0, sizeof(node));
  float scale[3];
  bvh_node_frame(node, P, scale);
  node.childBase = childBase; node.triBase = triBase;
  uint32_t triOffset = 0, childIdx = childBase;
  for (int s = 0; s < 8; s++) {
    const int i = P.childInSlot[s];
    if (i < 0) { bvh_empty_slot(node, s); continue; }
    const uint32_t c = P.ch[i];
    const float4 cl4 = T.lo[c], ch4 = T.hi[c];
    const float clo[3] = {cl4.x, cl4.y, cl4.z}, chi[3] = {ch4.x, ch4.y, ch4.z};
    bvh_quantise_slot(node, s, clo, chi, scale);
    if (P.leafMask & (1u << i)) { // leaf slot: unary count in the high 3 bits, triangle offset in the low 5; the BVH2 leaves below, left to right
      uint32_t leaves[kMaxLeaf];
      const uint32_t cnt = bvh_leaves_below(T.left, T.right, T.A, c, leaves);
      node.meta[s] = bvh_leaf_meta(cnt, triOffset);
      for (uint32_t k = 0; k < cnt; k++) {
        const uint32_t ref = sortedIds[leaves[k]], dst = triBase + triOffset + k;
        TriRec t = inTris[ref]; t.origId = ref; outTris[dst] = t; outFace[dst] = inFace[ref];
      }
      triOffset += cnt;
    } else {
      node.imask |= (uint8_t)(1u << s);
      node.meta[s] = bvh_internal_meta(s);
      nextLevel[childIdx - nodeEnd] = c;
      childIdx++;
    }
  }
  nodes[levelStart + li] = node;
}

// inactive triangles behind the active ones, in input order (the stable sort left them there)
__global__ __launch_bounds__(kBlock) void k_bvh_inactive(const uint32_t* __restrict__ sortedIds, uint32_t A, uint32_t n, const TriRec* __restrict__ inTris,
    const int32_t* __restrict__ inFace, TriRec* __restrict__ outTris, int32_t* __restrict__ outFace)
{
  const uint32_t k = A + blockIdx.x * kBlock + threadIdx.x;
  if (k >= n) return;
  const uint32_t ref = sortedIds[k];
  TriRec t = inTris[ref]; t.origId = ref; outTris[k] = t; outFace[k] = inFace[ref];
}

inline uint32_t blocksFor(uint32_t n) { return (n + kBlock - 1u) / kBlock; }

// every temporary of one build; out of memory frees them all
struct Arena {
  std::vector<void*> ptrs; bool oom = false; hipError_t err = hipSuccess;
  template <class T> T* get(size_t count)
  {
    if (oom || err != hipSuccess) return nullptr;
    void* p = nullptr;
    const hipError_t e = hipMalloc(&p, std::max<size_t>(count, 1) * sizeof(T));
    if (e != hipSuccess) { (void)hipGetLastError(); if (e == hipErrorOutOfMemory) oom = true; else err = e; return nullptr; }
    ptrs.push_back(p);
    return (T*)p;
  }
  void release() { for (void* p : ptrs) (void)hipFree(p); ptrs.clear(); }
  ~Arena() { release(); }
};

double nowMsDev() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

} // namespace

int buildBvh8Device(hipStream_t st, TriRec* tris, int32_t* faceId, uint32_t n, uint32_t maxLevels, DeviceBvhResult& out)
{
  out = DeviceBvhResult{};
  Arena ar;
#define DB_TRY(expr) do { const hipError_t _e = (expr); if (_e != hipSuccess) { out.error = #expr; return _e == hipErrorOutOfMemory ? DEVICE_BVH_OUT_OF_MEMORY \
    : DEVICE_BVH_ERROR; } } while (0)
#define DB_ALLOC_CHECK() do { if (ar.oom) return DEVICE_BVH_OUT_OF_MEMORY; if (ar.err != hipSuccess) { out.error = "hipMalloc failed"; \
    return DEVICE_BVH_ERROR; } } while (0)
  const double t0 = nowMsDev();
  const uint32_t nb = std::max(blocksFor(n), 1u);
  // inputs in scene order (the outputs are written over `tris` / `faceId`)
  TriRec* inTris = ar.get<TriRec>(n); int32_t* inFace = ar.get<int32_t>(n);
  float4* triLo = ar.get<float4>(n); float4* triHi = ar.get<float4>(n);
  float4* blockLo = ar.get<float4>(nb); float4* blockHi = ar.get<float4>(nb); uint32_t* blockAlive = ar.get<uint32_t>(nb);
  float4* bounds = ar.get<float4>(2); uint32_t* dAlive = ar.get<uint32_t>(1);
  uint64_t* keys = ar.get<uint64_t>(n); uint64_t* keys2 = ar.get<uint64_t>(n); uint32_t* ids = ar.get<uint32_t>(n); uint32_t* sortedIds = ar.get<uint32_t>(n);
  DB_ALLOC_CHECK();
  if (n) {
    DB_TRY(hipMemcpyAsync(inTris, tris, (size_t)n * sizeof(TriRec), hipMemcpyDeviceToDevice, st));
    DB_TRY(hipMemcpyAsync(inFace, faceId, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToDevice, st));
    k_bvh_boxes<<<nb, kBlock, 0, st>>>(inTris, n, triLo, triHi, blockLo, blockHi, blockAlive);
  }
  k_bvh_bounds<<<1, kBlock, 0, st>>>(blockLo, blockHi, blockAlive, n ? nb : 0u, bounds, dAlive);
  uint32_t A = 0;
  DB_TRY(hipMemcpyAsync(&A, dAlive, 4, hipMemcpyDeviceToHost, st));
  DB_TRY(hipStreamSynchronize(st));
  const double t1 = nowMsDev();
  // ---- sort
  if (n) {
    k_bvh_morton<<<nb, kBlock, 0, st>>>(triLo, triHi, n, bounds, keys, ids);
    size_t tmpBytes = 0;
    DB_TRY(rocprim::radix_sort_pairs(nullptr, tmpBytes, keys, keys2, ids, sortedIds, n, 0, 64, st));
    void* tmp = ar.get<uint8_t>(tmpBytes); DB_ALLOC_CHECK();
    DB_TRY(rocprim::radix_sort_pairs(tmp, tmpBytes, keys, keys2, ids, sortedIds, n, 0, 64, st));
  }
  DB_TRY(hipStreamSynchronize(st));
  const double t2 = nowMsDev();
  // ---- PLOC (+ the collapse DP in its merge kernel)
  const uint32_t nodes2 = A ? 2u * A - 1u : 1u;
  float4* nLo = ar.get<float4>(nodes2); float4* nHi = ar.get<float4>(nodes2);
  uint32_t* left = ar.get<uint32_t>(nodes2); uint32_t* right = ar.get<uint32_t>(nodes2); uint32_t* total = ar.get<uint32_t>(nodes2);
  Dp* dp = ar.get<Dp>(nodes2);
  uint32_t* clA = ar.get<uint32_t>(A); uint32_t* clB = ar.get<uint32_t>(A); uint32_t* nn = ar.get<uint32_t>(A);
  uint64_t* flags = ar.get<uint64_t>(A); uint64_t* incl = ar.get<uint64_t>(A);
  DB_ALLOC_CHECK();
  size_t scanBytes = 0;
  DB_TRY(rocprim::inclusive_scan(nullptr, scanBytes, flags, incl, std::max(A, 1u), rocprim::plus<uint64_t>(), st));
  void* scanTmp = ar.get<uint8_t>(scanBytes); DB_ALLOC_CHECK();
  uint32_t root2 = 0, plocIters = 0;
  if (A) {
    k_bvh_leaves<<<blocksFor(A), kBlock, 0, st>>>(sortedIds, A, triLo, triHi, nLo, nHi, total, dp, clA);
    uint32_t m = A, nodeBase = A;
    // PLOC's search radius (positions either side in Morton order; GATLING_OPTIONS ploc_radius, default 16 as in the paper)
    const uint32_t radius = (uint32_t)std::min(std::max(optionValue("ploc_radius", 16), 1L), 256L);
    while (m > 1u) {
      k_ploc_nn<<<blocksFor(m), kBlock, 0, st>>>(clA, m, radius, nLo, nHi, nn);
      k_ploc_flags<<<blocksFor(m), kBlock, 0, st>>>(nn, m, flags);
      DB_TRY(rocprim::inclusive_scan(scanTmp, scanBytes, flags, incl, m, rocprim::plus<uint64_t>(), st));
      k_ploc_merge<<<blocksFor(m), kBlock, 0, st>>>(clA, m, nn, flags, incl, nodeBase, nLo, nHi, left, right, total, dp, clB);
      uint64_t sums = 0;
      DB_TRY(hipMemcpyAsync(&sums, incl + (m - 1u), 8, hipMemcpyDeviceToHost, st));
      DB_TRY(hipStreamSynchronize(st));
      const uint32_t merges = (uint32_t)(sums >> 32), keeps = (uint32_t)(sums & 0xffffffffull);
      if (merges == 0u || keeps + merges != m || nodeBase + merges > nodes2) { out.error = "PLOC made no progress"; return DEVICE_BVH_ERROR; }
      nodeBase += merges; m = keeps; std::swap(clA, clB); plocIters++;
    }
    DB_TRY(hipMemcpyAsync(&root2, clA, 4, hipMemcpyDeviceToHost, st));
    DB_TRY(hipStreamSynchronize(st));
  }
  const double t3 = nowMsDev();
  // ---- emission, one breadth-first level at a time
  const uint32_t nodeCap = A + 1u; // an 8-wide node per BVH2 internal node at most (or the one root)
  Node8* nodesTmp = ar.get<Node8>(nodeCap); uint32_t* lvA = ar.get<uint32_t>(nodeCap); uint32_t* lvB = ar.get<uint32_t>(nodeCap);
  Plan* plans = ar.get<Plan>(nodeCap); uint64_t* counts = ar.get<uint64_t>(nodeCap); uint64_t* cincl = ar.get<uint64_t>(nodeCap);
  DB_ALLOC_CHECK();
  size_t scan2Bytes = 0;
  DB_TRY(rocprim::inclusive_scan(nullptr, scan2Bytes, counts, cincl, nodeCap, rocprim::plus<uint64_t>(), st));
  void* scan2Tmp = ar.get<uint8_t>(scan2Bytes); DB_ALLOC_CHECK();
  uint32_t nodeCount = 1, triCount = 0, levels = 0;
  if (A == 0u) { // bvh8.cpp emptyRoot: a single empty node
    Node8 root; bvh_empty_root(root);
    DB_TRY(hipMemcpyAsync(nodesTmp, &root, sizeof(root), hipMemcpyHostToDevice, st));
    DB_TRY(hipStreamSynchronize(st)); // (`root` leaves scope)
    levels = 1; out.levelStart.push_back(0u);
  } else {
    const Tree2 T{nLo, nHi, left, right, total, dp, A};
    DB_TRY(hipMemcpyAsync(lvA, &root2, 4, hipMemcpyHostToDevice, st));
    uint32_t levelStart = 0, m = 1;
    while (m > 0u) {
      if (++levels > maxLevels) return DEVICE_BVH_TOO_DEEP;
      out.levelStart.push_back(levelStart);
      k_bvh_plan<<<blocksFor(m), kBlock, 0, st>>>(T, lvA, m, levels == 1u, plans, counts);
      DB_TRY(rocprim::inclusive_scan(scan2Tmp, scan2Bytes, counts, cincl, m, rocprim::plus<uint64_t>(), st));
      uint64_t sums = 0;
      DB_TRY(hipMemcpyAsync(&sums, cincl + (m - 1u), 8, hipMemcpyDeviceToHost, st));
      DB_TRY(hipStreamSynchronize(st));
      const uint32_t internal = (uint32_t)(sums >> 32), trisHere = (uint32_t)(sums & 0xffffffffull);
      const uint32_t nodeEnd = levelStart + m;
      if (nodeEnd + internal > nodeCap || triCount + trisHere > A) { out.error = "emission outgrew its bounds"; return DEVICE_BVH_ERROR; }
      k_bvh_write<<<blocksFor(m), kBlock, 0, st>>>(T, lvA, m, levelStart, plans, counts, cincl, nodeEnd, triCount, sortedIds, inTris, inFace, nodesTmp,
          tris, faceId, lvB);
      levelStart = nodeEnd; m = internal; triCount += trisHere; nodeCount = nodeEnd + internal;
      std::swap(lvA, lvB);
    }
    if (triCount != A) { out.error = "emission lost triangles"; return DEVICE_BVH_ERROR; }
  }
  if (n > A) k_bvh_inactive<<<blocksFor(n - A), kBlock, 0, st>>>(sortedIds, A, n, inTris, inFace, tris, faceId);
  DB_TRY(hipGetLastError());
  // the tree in a buffer of its own size (the memory plan of the first render reads free memory after this)
  Node8* tree = nullptr;
  {
    const hipError_t e = hipMalloc((void**)&tree, (size_t)nodeCount * sizeof(Node8));
    if (e != hipSuccess) { (void)hipGetLastError(); out.error = "hipMalloc (nodes)"; return e == hipErrorOutOfMemory ? DEVICE_BVH_OUT_OF_MEMORY : DEVICE_BVH_ERROR; }
  }
  if (hipMemcpyAsync(tree, nodesTmp, (size_t)nodeCount * sizeof(Node8), hipMemcpyDeviceToDevice, st) != hipSuccess ||
      hipMemcpyAsync(&out.root, tree, sizeof(Node8), hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess) {
    (void)hipFree(tree); out.error = "copying the tree"; return DEVICE_BVH_ERROR;
  }
  ar.release();
  const double t4 = nowMsDev();
  out.levelStart.push_back(nodeCount);
  out.nodes = tree; out.nodeCount = nodeCount; out.maxDepth = levels; out.activeTris = A;
  out.ms[0] = t1 - t0; out.ms[1] = t2 - t1; out.ms[2] = t3 - t2; out.ms[3] = t4 - t3; out.plocIterations = plocIters;
  return DEVICE_BVH_OK;
#undef DB_TRY
#undef DB_ALLOC_CHECK
}

} // namespace gi

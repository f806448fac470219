// gi_tlas_build.hip -- the TLAS of an edited two-level scene built on the device (gi_tlas_build.h; DESIGN.md section 6 "TLAS build on the device").  Stages 1-3
// are gi_bvh_build.hip's (centroid bounds, Morton codes, stable radix sort, PLOC; the kernels and the arithmetic live in gi_bvh_stages.h), the collapse is the
// depth-bounded DP, and the whole build is shaped for an edit of a millisecond instead of a scene build of seconds:
//
//   no allocation    every buffer is carved out of the scene's TlasBuildWorkspace, which grows geometrically and is released with the scene
//   no wait per pass every kernel reads the cluster count, the level size and the status from a State record in device memory; its grid is sized by n, the
//                    bound of both.  PLOC passes are launched in batches of kTlasPassBatch with ONE read of the State behind each batch; once the count is at or
//                    below kTlasTailClusters one workgroup finishes PLOC in LDS (k_tlas_tail), which a build of n <= kTlasTailClusters reaches without a
//                    single read.  The `budget` levels of the emission are launched blind.  Host waits: batches (<= kTlasMaxBatches, else the build gives up
//                    with an error status) + 1 for the State behind the emission + 1 for the nodes and items -- a bound that does not depend on n.
//   no spinning      no cooperative launch, no grid-wide barrier, no workgroup waits for another's store: the order is the stream's
//   bounded loops    a pass merges at least one pair (the smallest pair is mutual); a pass without a merge sets the error status, and every kernel behind it
//                    returns at once
//
// One builder, two sources: buildBoxTreeDevice runs these stages for any BoxSource (gi_tlas_build.h) under the limits of the call -- buildTlasDevice with the
// caller's boxes under kTlasBuildLimits, gi_blas_build.hip with a mesh's face boxes under kBlasBuildLimits.  Indices and offsets are written for 2^22 items.
//
// Determinism: every position comes from a scan, the sort is stable, ties are broken by index: the bytes are a function of the input, and they are the host
// form's (gi_tlas_build_host.cpp; giCDebugBuildTlas holds that).
#include <cstring> // (before rocprim: its texture iterator calls memset in host code)
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#include <algorithm>

#include "gi_tlas_build.h"
#define GI_BVH_STAGE_KERNELS
#include "gi_bvh_stages.h"

namespace gi {
namespace {

constexpr uint32_t kBlock = kStageBlock;
constexpr uint32_t kTailThreads = 1024, kTailPer = kTlasTailClusters / kTailThreads; // 2 clusters per thread
static_assert(kTailPer * kTailThreads == kTlasTailClusters && kTlasTailClusters <= 0xffffu, "the tail's scan packs two 16-bit counts");

// what the kernels of one build hand each other (device memory; the host reads it behind a batch and behind the emission)
struct State {
  uint32_t A;           // active items (k_bvh_bounds)
  uint32_t m;           // clusters left
  uint32_t nodeBase;    // next BVH2 internal node
  uint32_t parity;      // which cluster list is current
  uint32_t passes;
  int32_t status;       // TlasBuildStatus; anything but OK stops every later kernel
  uint32_t root2;
  uint32_t levelM, levelStart, levelParity, levels, nodeCount, itemCount;
  uint32_t pad[3];
  uint32_t levelStartOf[kBoxBuildMaxLevels + 1]; // first node of every emitted level, then the node count (Bvh8::levelStart)
};

struct Tree { float* box; uint32_t* left; uint32_t* right; uint32_t* total; Dp* dp; uint32_t layers; };

// ---- 1. boxes: the caller's boxes as float4 pairs (inactive: inverted, which k_bvh_morton reads as "behind"), the block's centroid bounds ------------------
__global__ __launch_bounds__(kBlock) void k_tlas_boxes(const float* __restrict__ boxes6, uint32_t n, float4* __restrict__ lo4, float4* __restrict__ hi4,
    float4* __restrict__ blockLo, float4* __restrict__ blockHi, uint32_t* __restrict__ blockAlive)
{
  __shared__ float4 sLo[kBlock], sHi[kBlock]; __shared__ uint32_t sAlive[kBlock];
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  float4 cLo = make_float4(3.0e38f, 3.0e38f, 3.0e38f, 0.0f), cHi = make_float4(-3.0e38f, -3.0e38f, -3.0e38f, 0.0f);
  uint32_t alive = 0;
  if (i < n) {
    float b[6]; for (int a = 0; a < 6; a++) b[a] = boxes6[6u * (size_t)i + a];
    float4 bl, bh;
    stage_item_box(b, bl, bh, cLo, cHi, alive);
    lo4[i] = bl; hi4[i] = bh;
  }
  stage_block_bounds(cLo, cHi, alive, sLo, sHi, sAlive, blockLo, blockHi, blockAlive);
}

// ---- 3. PLOC ------------------------------------------------------------------------------------------------------------------------------------------------
// BVH2 leaves 0 .. A-1: the sorted active items; thread 0 starts the State
__global__ __launch_bounds__(kBlock) void k_tlas_leaves(const uint32_t* __restrict__ sortedIds, uint32_t n, const float* __restrict__ boxes6, Tree T,
    uint32_t* __restrict__ clusters, State* __restrict__ S)
{
  const uint32_t k = blockIdx.x * kBlock + threadIdx.x;
  const uint32_t A = min(S->A, n);
  if (k == 0u) { S->m = A; S->nodeBase = A; S->parity = 0u; S->passes = 0u; S->root2 = 0u; }
  if (k >= A) return;
  const uint32_t id = sortedIds[k];
  if (id >= n) return; // (cannot happen: the sort permutes 0 .. n-1)
  float b[6]; for (int a = 0; a < 6; a++) { b[a] = boxes6[6u * (size_t)id + a]; T.box[6u * (size_t)k + a] = b[a]; }
  T.total[k] = 1u; clusters[k] = k;
  bvh_dp_leaf_bounded(T.dp + (size_t)k * T.layers, T.layers, tlas_box_area(b));
}

// a multi-block pass runs while more clusters are left than the tail takes
__device__ inline bool pass_runs(const State* S, uint32_t n, uint32_t& m) { m = S->m; return S->status == TLAS_BUILD_OK && m > kTlasTailClusters && m <= n; }

__global__ __launch_bounds__(kBlock) void k_tlas_nn(const uint32_t* __restrict__ clA, const uint32_t* __restrict__ clB, uint32_t n, uint32_t radius,
    const float* __restrict__ box, uint32_t* __restrict__ nn, const State* __restrict__ S)
{
  uint32_t m; if (!pass_runs(S, n, m)) return;
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= m) return;
  const uint32_t* clusters = S->parity ? clB : clA;
  float bi[6]; { const float* p = box + 6u * (size_t)clusters[i]; for (int a = 0; a < 6; a++) bi[a] = p[a]; }
  const uint32_t j0 = i > radius ? i - radius : 0u, j1 = min(m - 1u, i + radius);
  float bestD = 3.4e38f; uint32_t bestH = 0xffffffffu, best = 0xffffffffu;
  for (uint32_t j = j0; j <= j1; j++) {
    if (j == i) continue;
    bvh_nn_consider(i, j, tlas_union_area(bi, box + 6u * (size_t)clusters[j]), bestD, bestH, best);
  }
  nn[i] = best;
}
// flags over all n positions (zero behind the clusters: the scan runs over n whatever m is)
__global__ __launch_bounds__(kBlock) void k_tlas_flags(const uint32_t* __restrict__ nn, uint32_t n, uint64_t* __restrict__ flags, const State* __restrict__ S)
{
  uint32_t m; if (!pass_runs(S, n, m)) return;
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  if (i >= m) { flags[i] = 0ull; return; }
  const uint32_t j = nn[i];
  flags[i] = bvh_ploc_flags(i, j, j < m && nn[j] == i);
}
__global__ __launch_bounds__(kBlock) void k_tlas_merge(uint32_t* __restrict__ clA, uint32_t* __restrict__ clB, uint32_t n, const uint32_t* __restrict__ nn,
    const uint64_t* __restrict__ flags, const uint64_t* __restrict__ incl, Tree T, const State* __restrict__ S)
{
  uint32_t m; if (!pass_runs(S, n, m)) return;
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= m) return;
  const uint32_t* clusters = S->parity ? clB : clA; uint32_t* next = S->parity ? clA : clB;
  const uint64_t f = flags[i], ex = incl[i] - f;
  if (!(f & 1ull)) return;
  const uint32_t keepAt = (uint32_t)(ex & 0xffffffffull);
  if (keepAt >= n) return; // (cannot happen)
  if (!(f >> 32)) { next[keepAt] = clusters[i]; return; }
  const uint32_t node = S->nodeBase + (uint32_t)(ex >> 32), j = nn[i];
  if (node >= 2u * n || j >= m) return; // (cannot happen: at most A - 1 merges in all; k_tlas_advance checks the sums)
  tlas_merge_node(T.box, T.left, T.right, T.total, T.dp, T.layers, node, clusters[i], clusters[j]);
  next[keepAt] = node;
}
// one thread: the pass's sums into the State; a pass without a merge ends the build
__global__ void k_tlas_advance(const uint64_t* __restrict__ incl, uint32_t n, State* __restrict__ S)
{
  uint32_t m; if (!pass_runs(S, n, m)) return;
  const uint64_t sums = incl[n - 1u];
  const uint32_t merges = (uint32_t)(sums >> 32), keeps = (uint32_t)(sums & 0xffffffffull);
  if (merges == 0u || keeps + merges != m || S->nodeBase + merges > 2u * S->A - 1u) { S->status = TLAS_BUILD_ERROR; return; }
  S->nodeBase += merges; S->m = keeps; S->parity ^= 1u; S->passes += 1u;
}

// One workgroup finishes PLOC once at most kTlasTailClusters clusters are left: their ids and boxes (28 bytes each) live in LDS, a pass is the multi-block
// pass's arithmetic on them -- nearest neighbour, mutual pairs, a block scan for the new positions and node indices --, merged nodes go to device memory (a
// later pass of this workgroup reads their DP records back behind the barrier).  Then the root and whether it fits the budget.
__global__ __launch_bounds__(kTailThreads) void k_tlas_tail(const uint32_t* __restrict__ clA, const uint32_t* __restrict__ clB, uint32_t n, uint32_t radius,
    Tree T, State* __restrict__ S)
{
  __shared__ float sBox[6][kTlasTailClusters];
  __shared__ uint32_t sId[kTlasTailClusters], sNn[kTlasTailClusters], sScan[kTailThreads];
  __shared__ uint32_t sBad;
  const uint32_t t = threadIdx.x;
  uint32_t m = S->m;
  const uint32_t A = S->A;
  if (S->status != TLAS_BUILD_OK || m > kTlasTailClusters || m > n || A == 0u || A > n) return; // (uniform: nothing wrote the State since the launch began)
  uint32_t nodeBase = S->nodeBase, passes = 0;
  const uint32_t* clusters = S->parity ? clB : clA;
  for (uint32_t q = 0; q < kTailPer; q++) {
    const uint32_t i = t * kTailPer + q;
    if (i < m) { const uint32_t c = clusters[i]; sId[i] = c; for (int a = 0; a < 6; a++) sBox[a][i] = T.box[6u * (size_t)c + a]; }
  }
  if (t == 0u) sBad = 0u;
  __syncthreads();
  for (uint32_t pass = 0; pass < kTlasTailClusters && m > 1u; pass++) {
    // nearest neighbours
    for (uint32_t q = 0; q < kTailPer; q++) {
      const uint32_t i = t * kTailPer + q;
      if (i >= m) continue;
      float bi[6]; for (int a = 0; a < 6; a++) bi[a] = sBox[a][i];
      const uint32_t j0 = i > radius ? i - radius : 0u, j1 = min(m - 1u, i + radius);
      float bestD = 3.4e38f; uint32_t bestH = 0xffffffffu, best = 0xffffffffu;
      for (uint32_t j = j0; j <= j1; j++) {
        if (j == i) continue;
        float bj[6]; for (int a = 0; a < 6; a++) bj[a] = sBox[a][j];
        bvh_nn_consider(i, j, tlas_union_area(bi, bj), bestD, bestH, best);
      }
      sNn[i] = best;
    }
    __syncthreads();
    // flags of this thread's positions, packed counts (merges << 16 | keeps), inclusive block scan
    uint64_t f[kTailPer]; uint32_t mine = 0;
    for (uint32_t q = 0; q < kTailPer; q++) {
      const uint32_t i = t * kTailPer + q;
      f[q] = 0ull;
      if (i < m) { const uint32_t j = sNn[i]; f[q] = bvh_ploc_flags(i, j, j < m && sNn[j] == i); }
      mine += ((uint32_t)(f[q] >> 32) << 16) | (uint32_t)(f[q] & 1ull);
    }
    sScan[t] = mine;
    __syncthreads();
    for (uint32_t s = 1; s < kTailThreads; s <<= 1) {
      const uint32_t v = t >= s ? sScan[t - s] : 0u;
      __syncthreads();
      sScan[t] += v;
      __syncthreads();
    }
    const uint32_t sums = sScan[kTailThreads - 1u], merges = sums >> 16, keeps = sums & 0xffffu;
    uint32_t ex = sScan[t] - mine;
    if (merges == 0u || keeps + merges != m || nodeBase + merges > 2u * A - 1u) { if (t == 0u) sBad = 1u; __syncthreads(); break; } // (uniform)
    // merges into device memory; the survivors' new places are held in registers until every read of the old list is done
    uint32_t newId[kTailPer], newAt[kTailPer]; float newBox[kTailPer][6];
    for (uint32_t q = 0; q < kTailPer; q++) {
      const uint32_t i = t * kTailPer + q;
      newAt[q] = 0xffffffffu; newId[q] = 0u;
      if (f[q] & 1ull) {
        newAt[q] = ex & 0xffffu;
        if (f[q] >> 32) {
          const uint32_t node = nodeBase + (ex >> 16);
          tlas_merge_node(T.box, T.left, T.right, T.total, T.dp, T.layers, node, sId[i], sId[sNn[i]]);
          newId[q] = node;
          for (int a = 0; a < 6; a++) newBox[q][a] = T.box[6u * (size_t)node + a];
        } else { newId[q] = sId[i]; for (int a = 0; a < 6; a++) newBox[q][a] = sBox[a][i]; }
      }
      ex += ((uint32_t)(f[q] >> 32) << 16) | (uint32_t)(f[q] & 1ull);
    }
    __syncthreads();
    for (uint32_t q = 0; q < kTailPer; q++)
      if (newAt[q] < kTlasTailClusters) { sId[newAt[q]] = newId[q]; for (int a = 0; a < 6; a++) sBox[a][newAt[q]] = newBox[q][a]; }
    nodeBase += merges; m = keeps; passes++;
    __syncthreads();
  }
  if (t == 0u) {
    S->passes += passes; S->nodeBase = nodeBase; S->m = m;
    if (sBad || m != 1u) S->status = TLAS_BUILD_ERROR;
    else {
      const uint32_t root = sId[0];
      S->root2 = root;
      const TlasTree2 R{T.box, T.left, T.right, T.total, T.dp, A, T.layers};
      if (!tlas_root_feasible(R, root)) S->status = TLAS_BUILD_TOO_DEEP;
    }
  }
}

// ---- 5. emission --------------------------------------------------------------------------------------------------------------------------------------------
// one thread: the first level is the root (no active item: bvh8.cpp's empty root, and no level to emit)
__global__ void k_tlas_emit_init(uint32_t* __restrict__ lvA, Node8* __restrict__ nodes, State* __restrict__ S)
{
  S->levelM = 0u; S->levelStart = 0u; S->levelParity = 0u; S->levels = 0u; S->nodeCount = 0u; S->itemCount = 0u;
  if (S->A == 0u) { Node8 root; bvh_empty_root(root); nodes[0] = root; S->levels = 1u; S->nodeCount = 1u; S->levelStartOf[0] = 0u; S->levelStartOf[1] = 1u; return; }
  if (S->status != TLAS_BUILD_OK) return;
  if (S->m > 1u) { S->status = TLAS_BUILD_ERROR; return; } // (the tail did not run: cannot happen)
  lvA[0] = S->root2; S->levelM = 1u; S->nodeCount = 1u;
}
// plans of the current level; counts over all `cap` positions (zero behind the level: the scan runs over cap)
__global__ __launch_bounds__(kBlock) void k_tlas_plan(Tree T, const uint32_t* __restrict__ lvA, const uint32_t* __restrict__ lvB, uint32_t cap, uint32_t budget,
    Plan* __restrict__ plans, uint64_t* __restrict__ counts, const State* __restrict__ S)
{
  const uint32_t li = blockIdx.x * kBlock + threadIdx.x;
  if (li >= cap) return;
  const uint32_t m = S->levelM, levels = S->levels;
  if (S->status != TLAS_BUILD_OK || li >= m || levels >= budget) { counts[li] = 0ull; return; }
  const uint32_t* level = S->levelParity ? lvB : lvA;
  const TlasTree2 R{T.box, T.left, T.right, T.total, T.dp, S->A, T.layers};
  Plan P; uint64_t c;
  tlas_plan_node(R, level[li], levels == 0u, budget - levels, P, c);
  plans[li] = P; counts[li] = c;
}
__global__ __launch_bounds__(kBlock) void k_tlas_write(Tree T, uint32_t* __restrict__ lvA, uint32_t* __restrict__ lvB, uint32_t cap, uint32_t budget,
    const Plan* __restrict__ plans, const uint64_t* __restrict__ counts, const uint64_t* __restrict__ incl, const uint32_t* __restrict__ sortedIds,
    Node8* __restrict__ nodes, uint32_t* __restrict__ items, const State* __restrict__ S)
{
  const uint32_t li = blockIdx.x * kBlock + threadIdx.x;
  const uint32_t m = S->levelM;
  if (S->status != TLAS_BUILD_OK || li >= m || li >= cap || S->levels >= budget) return;
  uint32_t* next = S->levelParity ? lvA : lvB;
  const uint64_t c = counts[li], ex = incl[li] - c, sums = incl[cap - 1u];
  const uint32_t nodeEnd = S->levelStart + m, childBase = nodeEnd + (uint32_t)(ex >> 32), itemBase = S->itemCount + (uint32_t)(ex & 0xffffffffull);
  // (k_tlas_level refuses a level that outgrows the arrays; until it has, nothing is written past them)
  if (nodeEnd + (uint32_t)(sums >> 32) > cap || S->itemCount + (uint32_t)(sums & 0xffffffffull) > S->A || S->levelStart + li >= cap) return;
  const TlasTree2 R{T.box, T.left, T.right, T.total, T.dp, S->A, T.layers};
  Node8 node;
  tlas_write_node(R, plans[li], childBase, itemBase, nodeEnd, sortedIds, node, items, next);
  nodes[S->levelStart + li] = node;
}
// one thread: the level's sums into the State
__global__ void k_tlas_level(const uint64_t* __restrict__ incl, uint32_t cap, uint32_t budget, State* __restrict__ S)
{
  const uint32_t m = S->levelM;
  if (S->status != TLAS_BUILD_OK || m == 0u) return;
  if (S->levels >= budget) { S->status = TLAS_BUILD_ERROR; return; } // (cannot happen: the DP bounds the depth)
  const uint64_t sums = incl[cap - 1u];
  const uint32_t internal = (uint32_t)(sums >> 32), itemsHere = (uint32_t)(sums & 0xffffffffull), nodeEnd = S->levelStart + m;
  if (nodeEnd + internal > cap || S->itemCount + itemsHere > S->A) { S->status = TLAS_BUILD_ERROR; return; }
  if (S->levels < kBoxBuildMaxLevels) { S->levelStartOf[S->levels] = S->levelStart; S->levelStartOf[S->levels + 1u] = nodeEnd; } // (the last level has no internal child)
  S->levelStart = nodeEnd; S->levelM = internal; S->itemCount += itemsHere; S->nodeCount = nodeEnd + internal; S->levels += 1u; S->levelParity ^= 1u;
}
// inactive items behind the active ones, in input order (the stable sort left them there); thread 0 closes the build
__global__ __launch_bounds__(kBlock) void k_tlas_inactive(const uint32_t* __restrict__ sortedIds, uint32_t n, uint32_t* __restrict__ items, State* __restrict__ S)
{
  const uint32_t k = blockIdx.x * kBlock + threadIdx.x;
  const uint32_t A = S->A;
  if (k == 0u && S->status == TLAS_BUILD_OK && A != 0u && (S->levelM != 0u || S->itemCount != A)) S->status = TLAS_BUILD_ERROR; // (levels left over, items lost)
  if (k >= n || k < A) return;
  items[k] = sortedIds[k];
}

inline uint32_t blocksFor(uint32_t n) { return (n + kBlock - 1u) / kBlock; }

// the slab's layout for one build
struct Carver {
  uint8_t* base; size_t at = 0;
  template <class T> T* get(size_t count) { at = (at + 255u) & ~(size_t)255u; T* p = base ? (T*)(base + at) : nullptr; at += std::max<size_t>(count, 1) * sizeof(T); return p; }
};
struct Layout {
  float* boxes6; float4 *lo4, *hi4, *blockLo, *blockHi, *bounds; uint32_t* blockAlive; uint64_t *keys, *keys2; uint32_t *ids, *sortedIds;
  Tree T; uint32_t *clA, *clB, *nn; uint64_t *flags, *incl; Node8* nodes; uint32_t *items, *lvA, *lvB; Plan* plans; uint64_t *counts, *cincl; State* S;
  void *sortTmp, *scanTmp, *scan2Tmp, *extra; size_t bytes;
};
Layout carve(void* mem, uint32_t n, uint32_t layers, size_t sortBytes, size_t scanBytes, size_t scan2Bytes, size_t extraBytes)
{
  Carver c{(uint8_t*)mem}; Layout L{};
  const size_t nb = std::max(blocksFor(n), 1u), nodes2 = 2u * (size_t)std::max(n, 1u), cap = (size_t)n + 1u;
  L.boxes6 = c.get<float>(6u * (size_t)n); L.lo4 = c.get<float4>(n); L.hi4 = c.get<float4>(n);
  L.blockLo = c.get<float4>(nb); L.blockHi = c.get<float4>(nb); L.bounds = c.get<float4>(2); L.blockAlive = c.get<uint32_t>(nb);
  L.keys = c.get<uint64_t>(n); L.keys2 = c.get<uint64_t>(n); L.ids = c.get<uint32_t>(n); L.sortedIds = c.get<uint32_t>(n);
  L.T.box = c.get<float>(6u * nodes2); L.T.left = c.get<uint32_t>(nodes2); L.T.right = c.get<uint32_t>(nodes2); L.T.total = c.get<uint32_t>(nodes2);
  L.T.dp = c.get<Dp>(nodes2 * layers); L.T.layers = layers;
  L.clA = c.get<uint32_t>(n); L.clB = c.get<uint32_t>(n); L.nn = c.get<uint32_t>(n); L.flags = c.get<uint64_t>(n); L.incl = c.get<uint64_t>(n);
  L.nodes = c.get<Node8>(cap); L.items = c.get<uint32_t>(n); L.lvA = c.get<uint32_t>(cap); L.lvB = c.get<uint32_t>(cap);
  L.plans = c.get<Plan>(cap); L.counts = c.get<uint64_t>(cap); L.cincl = c.get<uint64_t>(cap); L.S = c.get<State>(1);
  L.sortTmp = c.get<uint8_t>(sortBytes); L.scanTmp = c.get<uint8_t>(scanBytes); L.scan2Tmp = c.get<uint8_t>(scan2Bytes);
  L.extra = extraBytes ? c.get<uint8_t>(extraBytes) : nullptr; // (a source without arrays of its own leaves the slab's size what it was)
  L.bytes = c.at + 256u;
  return L;
}

} // namespace

void TlasBuildWorkspace::release()
{
  if (mem) (void)hipFree(mem);
  mem = nullptr; bytes = 0;
  for (hipEvent_t& e : ev) { if (e) (void)hipEventDestroy(e); e = nullptr; }
}

namespace {
// the TLAS's source: the caller's boxes, uploaded as they are
struct HostBoxes { const float* boxes6; };
hipError_t fillFromHostBoxes(void* ctx, const BoxStage& stage, uint32_t n, hipStream_t st)
{
  const hipError_t e = hipMemcpyAsync(stage.boxes6, static_cast<const HostBoxes*>(ctx)->boxes6, (size_t)n * 24u, hipMemcpyHostToDevice, st);
  if (e != hipSuccess) return e;
  k_tlas_boxes<<<blocksFor(n), kBlock, 0, st>>>(stage.boxes6, n, stage.lo4, stage.hi4, stage.blockLo, stage.blockHi, stage.blockAlive);
  return hipSuccess;
}
} // namespace

int buildTlasDevice(TlasBuildWorkspace& ws, hipStream_t st, const float* boxes6, uint32_t n, uint32_t budget, uint32_t radius, std::vector<Node8>& nodes,
    std::vector<uint32_t>& items, TlasBuildInfo& info)
{
  HostBoxes host{boxes6};
  BoxSource source; source.fill = fillFromHostBoxes; source.ctx = &host;
  return buildBoxTreeDevice(ws, st, source, n, budget, radius, kTlasBuildLimits, nodes, items, info);
}

int buildBoxTreeDevice(TlasBuildWorkspace& ws, hipStream_t st, const BoxSource& source, uint32_t n, uint32_t budget, uint32_t radius, const BoxBuildLimits& limits,
    std::vector<Node8>& nodes, std::vector<uint32_t>& items, TlasBuildInfo& info)
{
  info = TlasBuildInfo{}; nodes.clear(); items.clear();
  if (n > limits.maxItems || n > 0x7fffffffu || !source.fill) { info.error = "more items than the builder is sized for"; return TLAS_BUILD_ERROR; }
  if (source.backBytes && (!source.backHost || source.backOffset > source.extraBytes || source.backBytes > source.extraBytes - source.backOffset)) {
    info.error = "the source's read-back lies outside its share of the slab"; return TLAS_BUILD_ERROR; }
  budget = std::min(std::min(budget, limits.maxBudget), kBoxBuildMaxLevels); radius = std::min(std::max(radius, 1u), 256u);
  if (budget == 0u) return TLAS_BUILD_TOO_DEEP;
  const uint32_t layers = budget + 1u, cap = n + 1u;
#define TB_TRY(expr) do { const hipError_t _e = (expr); if (_e != hipSuccess) { (void)hipGetLastError(); info.error = #expr; \
    return _e == hipErrorOutOfMemory ? TLAS_BUILD_OUT_OF_MEMORY : TLAS_BUILD_ERROR; } } while (0)
  // ---- the workspace: sizes first (rocprim's queries launch nothing), then the slab if this build outgrows it
  size_t sortBytes = 0, scanBytes = 0, scan2Bytes = 0;
  if (n) {
    TB_TRY(rocprim::radix_sort_pairs(nullptr, sortBytes, (uint64_t*)nullptr, (uint64_t*)nullptr, (uint32_t*)nullptr, (uint32_t*)nullptr, n, 0, 64, st));
    TB_TRY(rocprim::inclusive_scan(nullptr, scanBytes, (uint64_t*)nullptr, (uint64_t*)nullptr, n, rocprim::plus<uint64_t>(), st));
  }
  TB_TRY(rocprim::inclusive_scan(nullptr, scan2Bytes, (uint64_t*)nullptr, (uint64_t*)nullptr, cap, rocprim::plus<uint64_t>(), st));
  const size_t need = carve(nullptr, n, layers, sortBytes, scanBytes, scan2Bytes, source.extraBytes).bytes;
  if (need > ws.bytes) {
    TB_TRY(hipStreamSynchronize(st)); // (nothing of an earlier build is in flight: builds end with a wait; a foreign stream's work is the caller's)
    const size_t want = std::max(need, 2u * ws.bytes);
    if (ws.mem) { (void)hipFree(ws.mem); ws.mem = nullptr; ws.bytes = 0; }
    void* p = nullptr;
    hipError_t e = hipMalloc(&p, want);
    if (e != hipSuccess && want > need) { (void)hipGetLastError(); e = hipMalloc(&p, need); if (e == hipSuccess) { ws.mem = p; ws.bytes = need; } }
    else if (e == hipSuccess) { ws.mem = p; ws.bytes = want; }
    if (e != hipSuccess) { (void)hipGetLastError(); info.error = "hipMalloc (workspace)"; return e == hipErrorOutOfMemory ? TLAS_BUILD_OUT_OF_MEMORY : TLAS_BUILD_ERROR; }
    ws.allocations++;
  }
  for (hipEvent_t& e : ws.ev) if (!e) TB_TRY(hipEventCreate(&e));
  const Layout L = carve(ws.mem, n, layers, sortBytes, scanBytes, scan2Bytes, source.extraBytes);
  const uint32_t nb = std::max(blocksFor(n), 1u);
  uint32_t waits = 0;
  // ---- 1. boxes and bounds, 2. codes and sort
  TB_TRY(hipEventRecord(ws.ev[0], st));
  TB_TRY(hipMemsetAsync(L.S, 0, sizeof(State), st));
  if (n) {
    const BoxStage stage{L.boxes6, L.lo4, L.hi4, L.blockLo, L.blockHi, L.blockAlive, L.extra};
    TB_TRY(source.fill(source.ctx, stage, n, st));
  }
  k_bvh_bounds<<<1, kBlock, 0, st>>>(L.blockLo, L.blockHi, L.blockAlive, n ? nb : 0u, L.bounds, &L.S->A);
  if (n) {
    k_bvh_morton<<<nb, kBlock, 0, st>>>(L.lo4, L.hi4, n, L.bounds, L.keys, L.ids);
    TB_TRY(rocprim::radix_sort_pairs(L.sortTmp, sortBytes, L.keys, L.keys2, L.ids, L.sortedIds, n, 0, 64, st));
  }
  TB_TRY(hipEventRecord(ws.ev[1], st));
  // ---- 3. PLOC with the DP in its merges: batches of multi-block passes, then the tail
  State S{};
  if (n) {
    k_tlas_leaves<<<nb, kBlock, 0, st>>>(L.sortedIds, n, L.boxes6, L.T, L.clA, L.S);
    uint32_t batches = 0;
    bool tailDue = n <= kTlasTailClusters; // (then A <= the tail's size whatever the boxes are: no read is needed to know)
    while (!tailDue) {
      if (batches == kTlasMaxBatches) { info.error = "PLOC did not come down to the tail's size within the batches allowed"; info.hostWaits = waits; return TLAS_BUILD_ERROR; }
      for (uint32_t p = 0; p < kTlasPassBatch; p++) {
        k_tlas_nn<<<nb, kBlock, 0, st>>>(L.clA, L.clB, n, radius, L.T.box, L.nn, L.S);
        k_tlas_flags<<<nb, kBlock, 0, st>>>(L.nn, n, L.flags, L.S);
        TB_TRY(rocprim::inclusive_scan(L.scanTmp, scanBytes, L.flags, L.incl, n, rocprim::plus<uint64_t>(), st));
        k_tlas_merge<<<nb, kBlock, 0, st>>>(L.clA, L.clB, n, L.nn, L.flags, L.incl, L.T, L.S);
        k_tlas_advance<<<1, 1, 0, st>>>(L.incl, n, L.S);
      }
      batches++;
      TB_TRY(hipMemcpyAsync(&S, L.S, sizeof(State), hipMemcpyDeviceToHost, st));
      TB_TRY(hipStreamSynchronize(st)); waits++;
      tailDue = S.status != TLAS_BUILD_OK || S.m <= kTlasTailClusters;
    }
    k_tlas_tail<<<1, kTailThreads, 0, st>>>(L.clA, L.clB, n, radius, L.T, L.S);
  }
  TB_TRY(hipEventRecord(ws.ev[2], st));
  // ---- 5. emission: `budget` levels, launched blind
  k_tlas_emit_init<<<1, 1, 0, st>>>(L.lvA, L.nodes, L.S);
  if (n) {
    const uint32_t cb = blocksFor(cap);
    for (uint32_t lv = 0; lv < budget; lv++) {
      k_tlas_plan<<<cb, kBlock, 0, st>>>(L.T, L.lvA, L.lvB, cap, budget, L.plans, L.counts, L.S);
      TB_TRY(rocprim::inclusive_scan(L.scan2Tmp, scan2Bytes, L.counts, L.cincl, cap, rocprim::plus<uint64_t>(), st));
      k_tlas_write<<<cb, kBlock, 0, st>>>(L.T, L.lvA, L.lvB, cap, budget, L.plans, L.counts, L.cincl, L.sortedIds, L.nodes, L.items, L.S);
      k_tlas_level<<<1, 1, 0, st>>>(L.cincl, cap, budget, L.S);
    }
    k_tlas_inactive<<<nb, kBlock, 0, st>>>(L.sortedIds, n, L.items, L.S);
  }
  TB_TRY(hipGetLastError());
  TB_TRY(hipEventRecord(ws.ev[3], st));
  TB_TRY(hipMemcpyAsync(&S, L.S, sizeof(State), hipMemcpyDeviceToHost, st));
  TB_TRY(hipStreamSynchronize(st)); waits++;
  info.hostWaits = waits; info.active = S.A; info.passes = S.passes;
  if (S.status != TLAS_BUILD_OK) { if (S.status != TLAS_BUILD_TOO_DEEP) info.error = "the device build ended with an error status"; return S.status == TLAS_BUILD_TOO_DEEP ? TLAS_BUILD_TOO_DEEP : TLAS_BUILD_ERROR; }
  if (S.nodeCount == 0u || S.nodeCount > cap || S.levels == 0u || S.levels > budget) { info.error = "the device build left an impossible state"; return TLAS_BUILD_ERROR; }
  nodes.resize(S.nodeCount); items.resize(n);
  TB_TRY(hipMemcpyAsync(nodes.data(), L.nodes, (size_t)S.nodeCount * sizeof(Node8), hipMemcpyDeviceToHost, st));
  if (n) TB_TRY(hipMemcpyAsync(items.data(), L.items, (size_t)n * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  if (n && source.backBytes) TB_TRY(hipMemcpyAsync(source.backHost, (const uint8_t*)L.extra + source.backOffset, source.backBytes, hipMemcpyDeviceToHost, st));
  TB_TRY(hipEventRecord(ws.ev[4], st));
  TB_TRY(hipStreamSynchronize(st)); waits++;
  info.hostWaits = waits; info.nodeCount = S.nodeCount; info.maxDepth = S.levels;
  for (uint32_t lv = 0; lv <= S.levels && lv <= kBoxBuildMaxLevels; lv++) info.levelStart[lv] = S.levelStartOf[lv];
  for (int k = 0; k < 4; k++) { float ms = 0.0f; if (hipEventElapsedTime(&ms, ws.ev[k], ws.ev[k + 1]) == hipSuccess) info.ms[k] = ms; else (void)hipGetLastError(); }
  return TLAS_BUILD_OK;
#undef TB_TRY
}

} // namespace gi

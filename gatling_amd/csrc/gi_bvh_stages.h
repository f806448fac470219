// gi_bvh_stages.h -- the arithmetic the two device builders (gi_bvh_build.hip: the flat scene tree; gi_tlas_build.hip: the TLAS of an edit, DESIGN.md
// section 6 "TLAS build on the device") and the host form of the TLAS builder (gi_tlas_build_host.cpp) share, written once for host and device (the
// GI_REFIT_HD pattern of gi_refit.h), without contraction: Morton codes, PLOC's pair order, the collapse DP (Ylitie, Karras, Laine 2017, section 3.1) with
// and without a depth index, the gather of an 8-wide node's children through it, bvh8.cpp's slot assignment and quantisation.  A translation unit that
// defines GI_BVH_STAGE_KERNELS before the include also gets the stage kernels both device builders launch (centroid bounds, Morton codes).
#pragma once

#include <cmath>
#include <cstdint>
#include <cstring>

#include "gi_refit.h"
#include "gi_types.h"

namespace gi {

constexpr uint32_t kBvhMaxLeaf = 3;      // bvh8.cpp kMaxLeaf: 3-bit unary item count in Node8::meta
constexpr float kBvhCPrim = 0.5f;        // bvh8.cpp cPrim of the flat tree and of box mode
constexpr float kBvhInfeasible = 3.0e38f; // bvh8.cpp's stand-in for "cannot be a leaf"; the depth-bounded DP's "does not fit the budget"

// bvh8.cpp struct Dp (44 bytes per BVH2 node; per BVH2 node and depth layer in the depth-bounded form)
struct Dp { float c[7]; uint8_t eff[7]; uint8_t split[7]; uint8_t leaf; };
// one node's emission plan (bvh8.cpp Plan): children (BVH2 ids), slot of each, leaf mask, node box
struct Plan { uint32_t ch[8]; int8_t childInSlot[8]; float lo[3], hi[3]; uint8_t leafMask, n, pad[2]; };

// ---- Morton codes ----------------------------------------------------------------------------------------------------------------------------------------
GI_REFIT_HD inline uint64_t bvh_spread21(uint32_t x)
{
  uint64_t v = x & 0x1fffffu;
  v = (v | v << 32) & 0x1f00000000ffffull;
  v = (v | v << 16) & 0x1f0000ff0000ffull;
  v = (v | v << 8) & 0x100f00f00f00f00full;
  v = (v | v << 4) & 0x10c30c30c30c30c3ull;
  v = (v | v << 2) & 0x1249249249249249ull;
  return v;
}
// 63-bit code of the centroid c inside the centroid bounds [l, h]
GI_REFIT_HD inline uint64_t bvh_morton63(const float c[3], const float l[3], const float h[3])
{
  uint64_t code = 0;
  for (int a = 0; a < 3; a++) {
    const float ext = h[a] - l[a];
    float u = ext > 0.0f ? (c[a] - l[a]) / ext : 0.0f;
    u = fminf(fmaxf(u, 0.0f), 1.0f);
    const uint32_t q = (uint32_t)fminf(u * 2097152.0f, 2097151.0f);
    code |= bvh_spread21(q) << (2 - a);
  }
  return code;
}

// ---- PLOC ------------------------------------------------------------------------------------------------------------------------------------------------
// Tie-break of equal distances: a hash of the PAIR, then the partner's position.  (distance, pairHash, lower, upper) orders all pairs totally and the same
// way seen from either end, so the smallest pair in the list is always mutual (progress); the hash keeps runs of equal boxes (coincident centroids) from
// merging one pair per pass.
GI_REFIT_HD inline uint32_t bvh_pair_hash(uint32_t a, uint32_t b)
{
  uint32_t h = a * 0x9e3779b1u ^ (b + 0x7f4a7c15u) * 0x85ebca77u;
  h ^= h >> 16; h *= 0x7feb352du; h ^= h >> 15; h *= 0x846ca68bu; h ^= h >> 16;
  return h;
}
// candidate j (distance d) seen from position i against the best so far
GI_REFIT_HD inline void bvh_nn_consider(uint32_t i, uint32_t j, float d, float& bestD, uint32_t& bestH, uint32_t& best)
{
  const uint32_t h = bvh_pair_hash(i < j ? i : j, i < j ? j : i);
  if (d < bestD || (d == bestD && (h < bestH || (h == bestH && j < best)))) { bestD = d; bestH = h; best = j; }
}
// flags word of position i: (merges here << 32) | (cluster survives here); a mutual pair merges into its lower position
GI_REFIT_HD inline uint64_t bvh_ploc_flags(uint32_t i, uint32_t j, bool mutual) { return ((uint64_t)(mutual && i < j) << 32) | (uint64_t)!(mutual && i > j); }

// ---- collapse DP -----------------------------------------------------------------------------------------------------------------------------------------
GI_REFIT_HD inline void bvh_dp_leaf(Dp& d, float area)
{
  for (int i = 0; i < 7; i++) { d.c[i] = area * kBvhCPrim; d.eff[i] = 1; d.split[i] = 0; }
  d.leaf = 1;
}
// the cheapest split of j slots over the two children: dist = min_k L.c[k-1] + R.c[j-k-1]
GI_REFIT_HD inline float bvh_dp_split(const Dp& L, const Dp& R, int j, uint8_t& split)
{
  float best = kBvhInfeasible; int bk = 1;
  const int k0 = j - 7 > 1 ? j - 7 : 1, k1 = j - 1 < 7 ? j - 1 : 7;
  for (int k = k0; k <= k1; k++) { const float c = L.c[k - 1] + R.c[j - k - 1]; if (c < best) { best = c; bk = k; } }
  split = (uint8_t)bk;
  return best;
}
// bvh8.cpp Builder::dpNode behind the splits: dist[2..7] the forests, dist[8] the child list of the subtree's own 8-wide node
GI_REFIT_HD inline void bvh_dp_finish(Dp& d, const float dist[9], float area, uint32_t total)
{
  const float cLeaf = total <= kBvhMaxLeaf ? area * kBvhCPrim * (float)total : kBvhInfeasible;
  const float cInt = area + dist[8];
  d.leaf = (total <= kBvhMaxLeaf && cLeaf <= cInt) ? 1 : 0;
  d.c[0] = d.leaf ? cLeaf : cInt; d.eff[0] = 1;
  for (int i = 2; i <= 7; i++) {
    if (dist[i] < d.c[i - 2]) { d.c[i - 1] = dist[i]; d.eff[i - 1] = (uint8_t)i; }
    else { d.c[i - 1] = d.c[i - 2]; d.eff[i - 1] = d.eff[i - 2]; }
  }
}
// the unbounded step of an internal node (the flat tree)
GI_REFIT_HD inline void bvh_dp_internal(Dp& d, const Dp& L, const Dp& R, float area, uint32_t total)
{
  float dist[9];
  for (int j = 2; j <= 8; j++) dist[j] = bvh_dp_split(L, R, j, d.split[j - 2]);
  bvh_dp_finish(d, dist, area, total);
}
// The depth-bounded step: `layers` Dp records per BVH2 node, layer t answering C(n, i, t) -- the cheapest forest of <= i roots with at most t levels of
// 8-wide nodes below the roots' slots.  The forests split over the children's SAME layer; the subtree's own node takes one level, so its child list comes
// from the children's layer t - 1, and at t = 0 only a leaf slot is feasible.
GI_REFIT_HD inline void bvh_dp_leaf_bounded(Dp* d, uint32_t layers, float area) { for (uint32_t t = 0; t < layers; t++) bvh_dp_leaf(d[t], area); }
GI_REFIT_HD inline void bvh_dp_internal_bounded(Dp* d, const Dp* L, const Dp* R, uint32_t layers, float area, uint32_t total)
{
  for (uint32_t t = 0; t < layers; t++) {
    float dist[9];
    for (int j = 2; j <= 7; j++) dist[j] = bvh_dp_split(L[t], R[t], j, d[t].split[j - 2]);
    if (t > 0u) dist[8] = bvh_dp_split(L[t - 1u], R[t - 1u], 8, d[t].split[6]);
    else { dist[8] = kBvhInfeasible; d[t].split[6] = 1; }
    bvh_dp_finish(d[t], dist, area, total);
  }
}

// bvh8.cpp gatherOptimal: the child list of the 8-wide node rooted at BVH2 node `root`.  dpOf(n, own) is the Dp record the walk reads: own = true for the
// root (whose split of 8 slots is taken), false for everything below it (the depth-bounded form reads the layer under the root's there)
template <class DpOf>
GI_REFIT_HD inline int bvh_gather_optimal(const uint32_t* left, const uint32_t* right, uint32_t root, DpOf dpOf, uint32_t* ch, bool* chLeaf)
{
  int n = 0;
  uint32_t tn[32]; int8_t ts[32]; bool te[32]; int tp = 0;
  tn[tp] = root; ts[tp] = 8; te[tp] = true; tp++;
  while (tp > 0) {
    tp--; const uint32_t n2 = tn[tp]; const int slots = ts[tp]; const bool expand = te[tp];
    const Dp& d = dpOf(n2, expand);
    int j = slots;
    if (!expand) { j = d.eff[slots - 1]; if (j == 1) { ch[n] = n2; chLeaf[n] = d.leaf != 0; n++; continue; } }
    const int k = d.split[j - 2];
    tn[tp] = right[n2]; ts[tp] = (int8_t)(j - k); te[tp] = false; tp++;
    tn[tp] = left[n2]; ts[tp] = (int8_t)k; te[tp] = false; tp++;
  }
  return n;
}

// ---- emission --------------------------------------------------------------------------------------------------------------------------------------------
// bvh8.cpp's slot assignment: greedy max of the child centroid's projection on the slot's octant direction, seen from the node's centre
GI_REFIT_HD inline void bvh_assign_slots(int n, const float (*clo)[3], const float (*chi)[3], const float center[3], int slotOf[8])
{
  float cost[8][8];
  for (int i = 0; i < n; i++) {
    const float d[3] = {0.5f * (clo[i][0] + chi[i][0]) - center[0], 0.5f * (clo[i][1] + chi[i][1]) - center[1], 0.5f * (clo[i][2] + chi[i][2]) - center[2]};
    for (int s = 0; s < 8; s++) cost[i][s] = ((s & 1) ? d[0] : -d[0]) + ((s & 2) ? d[1] : -d[1]) + ((s & 4) ? d[2] : -d[2]);
  }
  bool slotUsed[8] = {false, false, false, false, false, false, false, false};
  bool childDone[8] = {false, false, false, false, false, false, false, false};
  for (int k = 0; k < n; k++) {
    int bi = -1, bs = -1; float bc = -3.0e38f;
    for (int i = 0; i < n; i++) if (!childDone[i]) for (int s = 0; s < 8; s++) if (!slotUsed[s] && cost[i][s] > bc) { bc = cost[i][s]; bi = i; bs = s; }
    if (bi < 0) { // (non-finite costs: first free child, first free slot)
      for (int i = 0; i < n && bi < 0; i++) if (!childDone[i]) bi = i;
      for (int s = 0; s < 8 && bs < 0; s++) if (!slotUsed[s]) bs = s;
    }
    slotOf[bi] = bs; slotUsed[bs] = true; childDone[bi] = true;
  }
}
// a node's origin, exponents and scales out of its plan
GI_REFIT_HD inline void bvh_node_frame(Node8& node, const Plan& P, float scale[3])
{
  for (int a = 0; a < 3; a++) { node.p[a] = P.lo[a]; const int e = refit_exponent_for(P.hi[a] - P.lo[a]); node.e[a] = (uint8_t)(e + 127); scale[a] = ldexpf(1.0f, e); }
}
// slot s of `node` holds the box [clo, chi]: outward rounding, then bvh8.cpp's fix-up loops against the fp32 planes the traversal evaluates
GI_REFIT_HD inline void bvh_quantise_slot(Node8& node, int s, const float clo[3], const float chi[3], const float scale[3])
{
  for (int a = 0; a < 3; a++) {
    int lo = (int)floor(((double)clo[a] - (double)node.p[a]) / (double)scale[a]);
    int hi = (int)ceil(((double)chi[a] - (double)node.p[a]) / (double)scale[a]);
    lo = lo < 0 ? 0 : (lo > 255 ? 255 : lo); hi = hi < 0 ? 0 : (hi > 255 ? 255 : hi);
    while (lo > 0 && node.p[a] + (float)lo * scale[a] > clo[a]) lo--;
    while (hi < 255 && node.p[a] + (float)hi * scale[a] < chi[a]) hi++;
    node.qlo[a][s] = (uint8_t)lo; node.qhi[a][s] = (uint8_t)hi;
  }
}
GI_REFIT_HD inline void bvh_empty_slot(Node8& node, int s) { for (int a = 0; a < 3; a++) { node.qlo[a][s] = 255; node.qhi[a][s] = 0; } }
GI_REFIT_HD inline uint8_t bvh_leaf_meta(uint32_t cnt, uint32_t triOffset) { return (uint8_t)((((1u << cnt) - 1u) << 5) | triOffset); }
GI_REFIT_HD inline uint8_t bvh_internal_meta(int s) { return (uint8_t)((1u << 5) | (24u + (uint32_t)s)); }
// the BVH2 leaves below a leaf slot's subtree c, left to right (at most kBvhMaxLeaf; leaves are the nodes below A)
GI_REFIT_HD inline uint32_t bvh_leaves_below(const uint32_t* left, const uint32_t* right, uint32_t A, uint32_t c, uint32_t leaves[kBvhMaxLeaf])
{
  uint32_t cnt = 0;
  uint32_t stack[2 * kBvhMaxLeaf]; int sp = 0; stack[sp++] = c;
  while (sp > 0 && cnt < kBvhMaxLeaf) {
    const uint32_t x = stack[--sp];
    if (x < A) { leaves[cnt++] = x; continue; }
    if (sp + 2 > (int)(2 * kBvhMaxLeaf)) break; // (cannot happen: a leaf slot holds at most three BVH2 leaves)
    stack[sp++] = right[x]; stack[sp++] = left[x];
  }
  return cnt;
}
// bvh8.cpp emptyRoot
GI_REFIT_HD inline void bvh_empty_root(Node8& root)
{
  memset(&root, 0, sizeof(root));
  for (int a = 0; a < 3; a++) { root.e[a] = 127; for (int s = 0; s < 8; s++) { root.qlo[a][s] = 255; root.qhi[a][s] = 0; } }
}

// ---- the TLAS builder's own steps (gi_tlas_build.hip and its host form): boxes as 6 floats (lo, hi), minima and maxima spelled out -----------------------
// bvh8.cpp prepareRange in box mode: the caller's box is taken as it is; inactive if a side is unusable or inverted
GI_REFIT_HD inline bool tlas_box_active(const float* b)
{
  for (int a = 0; a < 3; a++) if (!refit_usable(b[a]) || !refit_usable(b[3 + a]) || !(b[a] <= b[3 + a])) return false;
  return true;
}
GI_REFIT_HD inline float tlas_box_area(const float* b)
{
  const float dx = b[3] - b[0], dy = b[4] - b[1], dz = b[5] - b[2];
  if (dx < 0.0f) return 0.0f;
  return 2.0f * (dx * dy + dy * dz + dz * dx);
}
GI_REFIT_HD inline void tlas_box_union(const float* a, const float* b, float* out)
{
  for (int k = 0; k < 3; k++) { out[k] = refit_min(a[k], b[k]); out[3 + k] = refit_max(a[3 + k], b[3 + k]); }
}
GI_REFIT_HD inline float tlas_union_area(const float* a, const float* b) { float u[6]; tlas_box_union(a, b, u); return tlas_box_area(u); }

// the BVH2 of one build: 6 floats, children, item count and `layers` Dp records per node; leaves are the nodes below A
struct TlasTree2 { const float* box; const uint32_t* left; const uint32_t* right; const uint32_t* total; const Dp* dp; uint32_t A, layers; };

// a merged node: box, children, count and every layer of the DP (the children were completed by earlier passes)
GI_REFIT_HD inline void tlas_merge_node(float* box, uint32_t* left, uint32_t* right, uint32_t* total, Dp* dp, uint32_t layers, uint32_t node, uint32_t a, uint32_t b)
{
  float u[6]; tlas_box_union(box + 6u * (size_t)a, box + 6u * (size_t)b, u);
  for (int k = 0; k < 6; k++) box[6u * (size_t)node + k] = u[k];
  const uint32_t t = total[a] + total[b];
  left[node] = a; right[node] = b; total[node] = t;
  bvh_dp_internal_bounded(dp + (size_t)node * layers, dp + (size_t)a * layers, dp + (size_t)b * layers, layers, tlas_box_area(u), t);
}
// the root fits the budget: a leaf root, or a node whose child list the top layer could form
GI_REFIT_HD inline bool tlas_root_feasible(const TlasTree2& T, uint32_t root)
{
  if (root < T.A || T.total[root] <= kBvhMaxLeaf) return T.layers >= 2u;
  const Dp& d = T.dp[(size_t)root * T.layers + (T.layers - 1u)];
  return T.layers >= 2u && !d.leaf && d.c[0] < kBvhInfeasible;
}
// the plan of the 8-wide node rooted at BVH2 node n2, which may form its child list with `layer` levels (itself included); counts = internal << 32 | items
GI_REFIT_HD inline void tlas_plan_node(const TlasTree2& T, uint32_t n2, bool rootLevel, uint32_t layer, Plan& P, uint64_t& counts)
{
  uint32_t ch[8]; bool chLeaf[8]; int n = 0;
  if (n2 < T.A || (rootLevel && T.total[n2] <= kBvhMaxLeaf)) { ch[0] = n2; chLeaf[0] = true; n = 1; } // a root that is itself a leaf (bvh8.cpp: level 0 only)
  else {
    const Dp* dp = T.dp; const uint32_t layers = T.layers;
    n = bvh_gather_optimal(T.left, T.right, n2, [dp, layers, layer](uint32_t x, bool own) -> const Dp& { return dp[(size_t)x * layers + (own ? layer : layer - 1u)]; },
        ch, chLeaf);
  }
  float nb[6] = {3.0e38f, 3.0e38f, 3.0e38f, -3.0e38f, -3.0e38f, -3.0e38f};
  float clo[8][3], chi[8][3];
  for (int i = 0; i < n; i++) {
    const float* b = T.box + 6u * (size_t)ch[i];
    for (int a = 0; a < 3; a++) { clo[i][a] = b[a]; chi[i][a] = b[3 + a]; nb[a] = refit_min(nb[a], b[a]); nb[3 + a] = refit_max(nb[3 + a], b[3 + a]); }
  }
  const float center[3] = {0.5f * (nb[0] + nb[3]), 0.5f * (nb[1] + nb[4]), 0.5f * (nb[2] + nb[5])};
  int slotOf[8];
  bvh_assign_slots(n, clo, chi, center, slotOf);
  for (int s = 0; s < 8; s++) { P.childInSlot[s] = -1; P.ch[s] = 0; }
  uint32_t internal = 0, itemsHere = 0; P.leafMask = 0; P.n = (uint8_t)n; P.pad[0] = P.pad[1] = 0;
  for (int a = 0; a < 3; a++) { P.lo[a] = nb[a]; P.hi[a] = nb[3 + a]; }
  for (int i = 0; i < n; i++) {
    P.ch[i] = ch[i]; P.childInSlot[slotOf[i]] = (int8_t)i;
    if (chLeaf[i]) { P.leafMask |= (uint8_t)(1u << i); itemsHere += T.total[ch[i]]; } else internal++;
  }
  counts = ((uint64_t)internal << 32) | itemsHere;
}
// the node of a plan: internal children from childBase on in slot order (their BVH2 ids go to nextLevel[child - nodeEnd]), items from itemBase on
GI_REFIT_HD inline void tlas_write_node(const TlasTree2& T, const Plan& P, uint32_t childBase, uint32_t itemBase, uint32_t nodeEnd, const uint32_t* sortedIds,
    Node8& node, uint32_t* items, uint32_t* nextLevel)
{
  memset(&node, 0, sizeof(node));
  float scale[3];
  bvh_node_frame(node, P, scale);
  node.childBase = childBase; node.triBase = itemBase;
  uint32_t offset = 0, childIdx = childBase;
  for (int s = 0; s < 8; s++) {
    const int i = P.childInSlot[s];
    if (i < 0) { bvh_empty_slot(node, s); continue; }
    const uint32_t c = P.ch[i];
    const float* b = T.box + 6u * (size_t)c;
    bvh_quantise_slot(node, s, b, b + 3, scale);
    if (P.leafMask & (1u << i)) {
      uint32_t leaves[kBvhMaxLeaf];
      const uint32_t cnt = bvh_leaves_below(T.left, T.right, T.A, c, leaves);
      node.meta[s] = bvh_leaf_meta(cnt, offset);
      for (uint32_t k = 0; k < cnt; k++) items[itemBase + offset + k] = sortedIds[leaves[k]];
      offset += cnt;
    } else {
      node.imask |= (uint8_t)(1u << s);
      node.meta[s] = bvh_internal_meta(s);
      nextLevel[childIdx - nodeEnd] = c;
      childIdx++;
    }
  }
}

} // namespace gi

#if defined(GI_BVH_STAGE_KERNELS)
namespace gi {
namespace {

constexpr uint32_t kStageBlock = 256;

__device__ inline float box_area(const float4& lo, const float4& hi)
{
  const float dx = hi.x - lo.x, dy = hi.y - lo.y, dz = hi.z - lo.z;
  if (dx < 0.0f) return 0.0f;
  return 2.0f * (dx * dy + dy * dz + dz * dx);
}
__device__ inline float4 min4(const float4& a, const float4& b) { return make_float4(fminf(a.x, b.x), fminf(a.y, b.y), fminf(a.z, b.z), 0.0f); }
__device__ inline float4 max4(const float4& a, const float4& b) { return make_float4(fmaxf(a.x, b.x), fmaxf(a.y, b.y), fmaxf(a.z, b.z), 0.0f); }

// one item's padded box b (6 floats) as the box builders' stages take it: the float4 pair k_bvh_morton reads (inverted where the tree leaves the item out),
// the item's share of the centroid bounds, whether it is active
__device__ inline void stage_item_box(const float b[6], float4& bl, float4& bh, float4& cLo, float4& cHi, uint32_t& alive)
{
  bl = make_float4(3.0e38f, 3.0e38f, 3.0e38f, 0.0f); bh = make_float4(-3.0e38f, -3.0e38f, -3.0e38f, 0.0f);
  if (tlas_box_active(b)) {
    bl = make_float4(b[0], b[1], b[2], 0.0f); bh = make_float4(b[3], b[4], b[5], 0.0f);
    cLo = make_float4(0.5f * (b[0] + b[3]), 0.5f * (b[1] + b[4]), 0.5f * (b[2] + b[5]), 0.0f); cHi = cLo; alive = 1;
  }
}

// the block's share of the centroid bounds and of the active count (every thread calls it; thread 0 writes the block's partials)
__device__ inline void stage_block_bounds(float4 cLo, float4 cHi, uint32_t alive, float4* sLo, float4* sHi, uint32_t* sAlive, float4* __restrict__ blockLo,
    float4* __restrict__ blockHi, uint32_t* __restrict__ blockAlive)
{
  sLo[threadIdx.x] = cLo; sHi[threadIdx.x] = cHi; sAlive[threadIdx.x] = alive;
  __syncthreads();
  for (uint32_t s = kStageBlock / 2; s > 0; s >>= 1) {
    if (threadIdx.x < s) { sLo[threadIdx.x] = min4(sLo[threadIdx.x], sLo[threadIdx.x + s]); sHi[threadIdx.x] = max4(sHi[threadIdx.x], sHi[threadIdx.x + s]);
        sAlive[threadIdx.x] += sAlive[threadIdx.x + s]; }
    __syncthreads();
  }
  if (threadIdx.x == 0) { blockLo[blockIdx.x] = sLo[0]; blockHi[blockIdx.x] = sHi[0]; blockAlive[blockIdx.x] = sAlive[0]; }
}

// one block: the centroid bounds and the active count out of the per-block partials (min / max / integer sums: the order does not matter)
__global__ __launch_bounds__(kStageBlock) void k_bvh_bounds(const float4* __restrict__ blockLo, const float4* __restrict__ blockHi,
    const uint32_t* __restrict__ blockAlive, uint32_t blocks, float4* __restrict__ bounds, uint32_t* __restrict__ alive)
{
  __shared__ float4 sLo[kStageBlock], sHi[kStageBlock]; __shared__ uint32_t sAlive[kStageBlock];
  float4 lo = make_float4(3.0e38f, 3.0e38f, 3.0e38f, 0.0f), hi = make_float4(-3.0e38f, -3.0e38f, -3.0e38f, 0.0f); uint32_t cnt = 0;
  for (uint32_t b = threadIdx.x; b < blocks; b += kStageBlock) { lo = min4(lo, blockLo[b]); hi = max4(hi, blockHi[b]); cnt += blockAlive[b]; }
  sLo[threadIdx.x] = lo; sHi[threadIdx.x] = hi; sAlive[threadIdx.x] = cnt;
  __syncthreads();
  for (uint32_t s = kStageBlock / 2; s > 0; s >>= 1) {
    if (threadIdx.x < s) { sLo[threadIdx.x] = min4(sLo[threadIdx.x], sLo[threadIdx.x + s]); sHi[threadIdx.x] = max4(sHi[threadIdx.x], sHi[threadIdx.x + s]);
        sAlive[threadIdx.x] += sAlive[threadIdx.x + s]; }
    __syncthreads();
  }
  if (threadIdx.x == 0) { bounds[0] = sLo[0]; bounds[1] = sHi[0]; *alive = sAlive[0]; }
}

// 63-bit Morton codes of the box centroids (an inverted box: all ones, sorted behind every active item, in id order since the sort is stable)
// (a source of boxes -- gi_blas_build.hip -- includes the stage kernels for the bounds alone)
[[maybe_unused]] __global__ __launch_bounds__(kStageBlock) void k_bvh_morton(const float4* __restrict__ triLo, const float4* __restrict__ triHi, uint32_t n,
    const float4* __restrict__ bounds, uint64_t* __restrict__ keys, uint32_t* __restrict__ ids)
{
  const uint32_t i = blockIdx.x * kStageBlock + threadIdx.x;
  if (i >= n) return;
  ids[i] = i;
  const float4 lo = triLo[i], hi = triHi[i];
  if (!(lo.x <= hi.x)) { keys[i] = ~0ull; return; }
  const float4 bl = bounds[0], bh = bounds[1];
  const float c[3] = {0.5f * (lo.x + hi.x), 0.5f * (lo.y + hi.y), 0.5f * (lo.z + hi.z)};
  const float l[3] = {bl.x, bl.y, bl.z}, h[3] = {bh.x, bh.y, bh.z};
  keys[i] = bvh_morton63(c, l, h);
}

} // namespace
} // namespace gi
#endif

// gi_path.hip -- k_path: the fused persistent path kernel for scenes whose whole BVH lives in LDS (cornell: 4 nodes -- a root and three children --, 46
// triangles).  The tree it walks is the host builder's after the leaf lift (leaf_lift.cpp; gi_build.cpp buildScene): for a tree of two levels every second
// node visit is a wave-wide step of the closest-hit loop below, so scene sync moves leaf slots that stretch a child's box into free slots of the root.
//
// The wavefront pipeline (gi_kernels.hip) streams every path through HBM once per stage and bounce: ray record out, hit record in,
// 64-byte slot gathered and scattered -- on config C2 1.6 TB per frame for a scene of 2.6 KB.  When the scene is LDS-resident none
// of that traffic buys anything: there is no memory latency to hide behind a queue and no incoherent fetch to sort for.  k_path
// keeps the PATH in registers instead.  Every wave is persistent; a lane carries one (pixel, sample) work item through
// camera ray -> [closest hit -> shade -> shadow ray]* and, the moment its path ends, writes the finished sample and takes the next
// work item, so all 64 lanes trace on every trip ("persistent threads with path regeneration"; the regeneration replaces the
// wavefront loop's compaction).  HBM sees one 16-byte record per SAMPLE (per-sample colour buffer, summed in sample order by
// k_accumulate exactly as before) instead of ~340 bytes per SEGMENT.
//
// Replaces, for such scenes, the same reference code as the stage kernels: rp_main.rgen:185-521 (whole loop), traceRayEXT
// (:381-393, 412-424), rp_main.chit, rp_main.miss:68-86, rp_main_shadow.miss.  All per-path arithmetic is the SHARED stage code
// (make_camera_ray, wave_step, shade_segment, finish_sample), so images are bit-identical to the wavefront pipeline's and the
// oracle's; work items are claimed in chunks of consecutive ids (sample-major: adjacent pixels of one sample index), one atomic per
// chunk on one cursor.
//
// Camera rays that cannot reach the scene's bounds (FLAG_BOUNDS_RETIRE, ray_misses_bounds in gi_stages.h: the test k_raygen applies) retire where they are
// prepared: the lane stores the sample such a path ends with (0 + 1 x background, finished) and counts its one segment; only the other rays enter the ring.
// A wave's 64 work items are adjacent pixels of a row, so in a frame wider than the scene whole trips of whole waves were such rays (C2: 62 % of them).
// Renders that bind a path-following debug AOV (NEE, Bounces, ClockCycles) and counting builds trace every camera ray as before (gi_render.cpp scheduleFrame).
// Pixels whose EVERY camera ray misses (FLAG_MISS_RECT: outside the host's rectangle, gi_miss_rect.h) are not work items at all: the ids enumerate the pixels
// of the active rectangle, the records of the others are never written, and k_accumulate sums their constant.
//
// Hits that drew a glossy lobe of a UsdPreviewSurface material are parked (the NEE-off class-1 variant; "Lobe parking" in the trip loop): most trips skip the
// GGX block of the sample, the few hits that need it wait as 16-dword records in the traversal-stack rows the tree's walks never reach, and every few trips the
// wave shades them together with that trip's own.  A path's sequence of draws and operations is unchanged -- only the trip in which it advances differs; carried
// walker and free are exclusive lane states and only free lanes adopt; every trip retires a segment, adds to a bounded lot or takes from it; the kernel ends
// with the lot empty; lobePark = 0 is the kernel without parking.
//
// The (ray, triangle) pairs a step leaves over after its full batches wait for the next step of the trip (the NEE-off variants; "Ring carry" in the trip loop):
// a triangle batch runs whenever 64 pairs are pending and one flush in the loop's last step tests the rest, instead of a partial batch at the end of every
// step.  Hit keys do not depend on when a pair is tested; ringCarry = 0 flushes in every step.
//
// A scene whose class-1 materials are all untextured and have no coat (UPS_NOCOAT, gi_types.h; the host derives it: gi_build.cpp deriveSceneClasses) runs the
// instantiation whose class-1 sample leaves the coat lobe out (the NEE-off class-1 variant; UPS, the last template argument; gi_shading.h ups_plain_sample): the
// operations dropped are exact identities when coat is the word of +0, so the bits are the same.  UPS = 0 is the kernel as it was; ups_plain=0 selects it.
//
// The hot variants of classes 0 and 1 without NEE have a COOK instantiation (the last template argument; launchPath picks it, GATLING_OPTIONS=node_cook=0 does
// not): the block stages its nodes in the cooked form of gi_node_cook.h -- made from sc.nodes by its own threads before the barrier, nothing of it in HBM -- and
// the node test reads the word each child adds to the hit mask from a per-octant table instead of decoding the meta bytes on every visit, over the occupied
// slots only (gi_traversal.h trav_node_test_cooked).  The box arithmetic is untouched: hit masks, walks, images and `segments` are the same.
//
// Not handled here (the host falls back to the wavefront pipeline): medium stacks (mediumStackSize > 0), dome-light images,
// scenes beyond LDS, trees deeper than 8 levels.

#include <hip/hip_runtime.h>
#include <cassert>

#define GI_LEAN_MATH 1 // gi_device_math.h gi_sqrt / gi_div: the correctly rounded square root and division without the steps ordinary operands do not need
#include "gi_device_math.h"
#include "gi_kernels.h"
#include "gi_types.h"
#include "gi_queues.h"
#include "gi_traversal.h"
#include "gi_shading.h"
#include "gi_stages.h"

namespace gi {

constexpr uint32_t PRE_FIELDS = 10; // prepared camera ray: origin, direction, tMin, tMax, rng state, record index of its sample
constexpr uint32_t PATH_STACK_MAX = 8; // LDS traversal-stack entries per lane: 4 for trees of depth <= 4 (cornell), else 8 (the host checks bvhDepth <= 8)

constexpr int PATH_WAVES = 4; // resident waves per SIMD the register allocation aims for (114 VGPRs without a hint; 3 cost 11 %, 5 spill 26 registers: r03)
template <uint32_t KLASS, bool TEXTURED, bool NEE, bool CUTOUT, bool COUNT, uint32_t PATH_STACK, uint32_t UPS = 0u, bool COOK = false>
__global__ __launch_bounds__(TRACE_BLOCK) __attribute__((amdgpu_waves_per_eu(PATH_WAVES, 8))) void k_path(FrameUniforms U, SceneView sc, PathState st,
    Counters* cnt, F4* __restrict__ sampleBuf, uint32_t ldsNodes, uint32_t ldsTris, uint32_t chunk, uint32_t walkCarry, uint32_t lobePark, uint32_t lotRow,
    uint32_t lotCap, uint32_t ringCarry)
{
  // Walk carry (NEE off): see the closest-hit loop.  The NEE variants' shadow walk reuses R and WaveTri::best[lane], so they never carry.
  constexpr bool CARRY = !NEE;
  // Lobe parking (NEE off, class 1 -- and the counting build, which is how tests see it): see "shade" below.  Every other variant is compiled without it.
  constexpr bool PARK = !NEE && (KLASS == 1u || (KLASS == KLASS_DYNAMIC && COUNT));
  constexpr bool DEFER = PARK || COUNT; // shade_segment's deferring form: PARK needs it; counting builds use it to count the glossy hits (lite never set)
  static_assert(!COOK || (!NEE && !COUNT), "cooked nodes: the hot variants without NEE (wave_step_ring)");
  // the only barrier: from here on the waves of a block are independent
  const StagedScene S = COOK ? stage_scene_cooked<PATH_STACK>(sc, ldsNodes, ldsTris) : stage_scene<PATH_STACK>(sc, ldsNodes, ldsTris);
  __shared__ WaveTri s_wave[TRACE_BLOCK / 64];
  WaveTri& W = s_wave[threadIdx.x >> 6];

  const uint32_t lane = __lane_id();
  const unsigned long long below = (1ull << lane) - 1ull;
  // the path this lane carries (rp_main_payload.glsl:20-33) and its next ray
  V3 thr = v3(0.0f, 0.0f, 0.0f), rad = thr, ro = thr, rdv = v3(0.0f, 0.0f, 1.0f);
  float tMin = 0.0f, tMax = 0.0f;
  uint32_t bitfield = 0u, rng = 0u, rec = 0u; // rec: the record index of the lane's sample, sample * pixelCount + tile pixel -- the path's identity
  bool alive = false, tAlive = false; // tAlive outlives a trip: a lane still walking when the closest-hit loop ends early is carried into the next one
  uint32_t chunkNext = 0u, chunkEnd = 0u; bool exhausted = false; // wave-uniform: the claimed work items not handed out yet
  uint32_t nSeg = 0u, nShadow = 0u;
  WalkCounters<COUNT> tc{}, tcs{};
  uint2 overflow[1];
  RayTrav R; R.G = make_uint2(0u, 0u); R.sp = 0u;
  // Camera rays are generated 64 at a time, by ALL lanes, into a per-wave LDS ring (r03): a trip regenerates only the ~45 % of the lanes whose path just ended,
  // and make_camera_ray (hash, two draws, the Gaussian filter's log / sqrt / sincos, normalise) then ran at that lane utilisation on every trip.  Now the wave
  // prepares the next 64 work items' rays whenever fewer than 64 are pending (one full-width pass every ~2 trips) and idle lanes just pop them.
  __shared__ uint32_t s_pre[TRACE_BLOCK / 64][PRE_FIELDS][128]; // ring of 128 prepared rays per wave
  GI_LDS uint32_t (*pre)[128] = (GI_LDS uint32_t (*)[128])&s_pre[threadIdx.x >> 6][0][0];
  uint32_t preHead = 0u, preTail = 0u; // wave-uniform ring positions (monotonic; slot = position & 127)
  // FLAG_BOUNDS_RETIRE: a camera ray that cannot reach the scene's bounds (ray_misses_bounds, gi_stages.h) never enters the ring -- its sample is stored where the
  // ray is prepared, so a wave whose 64 adjacent pixels all look past the scene spends no trip (ring round trip, root-node step, miss branch) on them
  const bool boundsRetire = (U.flags & FLAG_BOUNDS_RETIRE) != 0u;

  unsigned long long pc[4] = {0ull, 0ull, 0ull, 0ull}, pl[4] = {0ull, 0ull, 0ull, 0ull}, trips = 0ull, tPrev = COUNT ? __builtin_readcyclecounter() : 0ull;
  uint32_t whLanes[8] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u}, whTrips[8] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u}; // COUNT: lanes walking at step 0 .. 7+ of a trip's loop
  uint32_t whFew = 0u; // COUNT: steps that began with fewer than 8 lanes walking
  uint32_t lobeN[9] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u}; // COUNT: Counters::lobeStats of this wave
  RingStats ringN{0u, 0u, 0u, 0u, 0u}; // COUNT: Counters::ringStats of this wave
  // The lot: the parked hits of this wave, 16-dword records in the rows of the traversal stack that no walk of this tree reaches.  Record k lies in row
  // lotRow + k / 8, in the 8 columns from k % 8 * 8 of the wave's 64 (a row of a wave: 64 columns x 8 bytes = 8 records).  The host passes the first free row
  // and the capacity (launchPath: lotRow >= bvhDepth, the most entries a walk pushes); clamped here once more to what PATH_STACK rows hold.
  const uint32_t lotFit = (PATH_STACK - (lotRow < PATH_STACK ? lotRow : PATH_STACK)) * 8u;
  const uint32_t lotMax = PARK ? (lotCap < lotFit ? lotCap : lotFit) : 0u;
  const uint32_t parkAt = PARK ? (lobePark < lotMax ? lobePark : lotMax) : 0u; // FULL once the lot holds this many (0: parking off, today's trips)
  uint32_t lotCount = 0u; // wave-uniform
  auto lot_record = [&](uint32_t k) __attribute__((always_inline)) {
    return (volatile GI_LDS gi_u4*)(GI_LDS gi_u4*)&S.stack[lotRow + (k >> 3)][(threadIdx.x & ~63u) + ((k & 7u) << 3)];
  };
  auto phase = [&](int k,
      unsigned long long lanes) { if (COUNT) { const unsigned long long t = __builtin_readcyclecounter(); pc[k] += t - tPrev; tPrev = t; pl[k] += lanes; } };
  for (;;) {
    __atomic_signal_fence(__ATOMIC_SEQ_CST); // (compiler only) the ring is exchanged between the lanes of this wave through LDS
    // --- regeneration (rp_main.rgen:213-283): idle lanes take the next work items w = sample * A + (pixel of the active rectangle)
    unsigned long long idle = __ballot(!alive);
    const uint32_t nIdle = (uint32_t)__popcll(idle);
    if (nIdle) {
      // top the ring up to at least 64 prepared rays (or whatever work is left): every lane prepares one
      while (preTail - preHead < 64u && !exhausted) {
        if (chunkNext == chunkEnd) {
          uint32_t b = 0u;
          if (lane == 0u) b = atomicAdd(&cnt->cursor[0][0].v, chunk);
          b = (uint32_t)__shfl((int)b, 0);
          if (b >= U.workTotal) { exhausted = true; break; }
          chunkNext = b; chunkEnd = (U.workTotal - b) < chunk ? U.workTotal : b + chunk;
        }
        const uint32_t avail = chunkEnd - chunkNext, take = avail < 64u ? avail : 64u;
        uint32_t nKept = 0u;
        if (lane < take) {
          // work item w = sample * activeCount + (pixel of the active rectangle, row-major): the whole tile, or with FLAG_MISS_RECT the part of it outside which every
          // camera ray misses the bounds -- those pixels get no work and no record (k_accumulate sums their constant).  The sample's record keeps its place in
          // the per-sample buffer, sample * pixelCount + tile pixel, and that index is what the ring carries.
          const uint32_t w = chunkNext + lane;
          const uint32_t sl = w / U.activeCount, a = w - sl * U.activeCount;
          const uint32_t ar = a / U.activeWidth, row = U.rectTy0 + ar, px = U.rectX0 + (a - ar * U.activeWidth);
          const uint32_t rec = sl * U.pixelCount + (row * U.imageWidth + px); // (< 2^32: the memory plan's clamp)
          const uint32_t py = U.rowBegin + row * U.rowStride;
          V3 o, d; float t0, t1; uint32_t r;
          // :195 (global pixel index: the RNG is tile independent)
          make_camera_ray_at(U, px, py, py * U.imageWidth + px, U.sampleOffset + U.batchFirstSample + sl, o, d, t0, t1, r);
          // (the bounds and the retired sample are wave-uniform; read through an empty asm they stay in scalar registers here -- left to itself the compiler
          // hoists what it derives from them out of the trip loop, into a dozen vector registers that then stay live through the walk and the shading)
          float lo[3] = {U.sceneLo[0], U.sceneLo[1], U.sceneLo[2]}, hi[3] = {U.sceneHi[0], U.sceneHi[1], U.sceneHi[2]};
          asm volatile("" : "+s"(lo[0]), "+s"(lo[1]), "+s"(lo[2]), "+s"(hi[0]), "+s"(hi[1]), "+s"(hi[2]));
          const bool keep = !(boundsRetire && ray_misses_box(lo, hi, o, d, t0, t1));
          const unsigned long long kept = __ballot(keep); // (of the lanes below `take`) the rays that go on take consecutive ring slots: < 64 pending + <= 64 new
          nKept = (uint32_t)__popcll(kept);
          if (keep) {
            const uint32_t slot = (preTail + (uint32_t)__popcll(kept & below)) & 127u;
            pre[0][slot] = f2u(o.x); pre[1][slot] = f2u(o.y); pre[2][slot] = f2u(o.z); pre[3][slot] = f2u(d.x); pre[4][slot] = f2u(d.y); pre[5][slot] = f2u(d.z);
            pre[6][slot] = f2u(t0); pre[7][slot] = f2u(t1); pre[8][slot] = r; pre[9][slot] = rec;
          } else { // the whole path is this one segment: its sample is the constant retire_fresh_miss stores (the miss branch + finish_sample below)
            float bg[3] = {U.background[0], U.background[1], U.background[2]}, maxv = U.maxSampleValue;
            asm volatile("" : "+s"(bg[0]), "+s"(bg[1]), "+s"(bg[2]), "+s"(maxv));
            V3 c = v3(0.0f, 0.0f, 0.0f) + v3(1.0f, 1.0f, 1.0f) * v3(bg[0], bg[1], bg[2]);
            const float mv = fmax2(c.x, fmax2(c.y, c.z));
            if (mv > maxv) c = c * (maxv / mv);
            st4(&sampleBuf[rec], fmax2(0.0f, c.x), fmax2(0.0f, c.y), fmax2(0.0f, c.z), 0.0f);
            nSeg++;
          }
        }
        chunkNext += take; preTail += (uint32_t)__builtin_amdgcn_readfirstlane((int)nKept); // (take >= 1: lane 0 was in)
      }
      __atomic_signal_fence(__ATOMIC_SEQ_CST);
      const uint32_t have = preTail - preHead, take = nIdle < have ? nIdle : have;
      const uint32_t rank = (uint32_t)__popcll(idle & below);
      if (!alive && rank < take) {
        const uint32_t slot = (preHead + rank) & 127u;
        ro = v3(u2f(pre[0][slot]), u2f(pre[1][slot]), u2f(pre[2][slot])); rdv = v3(u2f(pre[3][slot]), u2f(pre[4][slot]), u2f(pre[5][slot]));
        tMin = u2f(pre[6][slot]); tMax = u2f(pre[7][slot]); rng = pre[8][slot];
        rec = pre[9][slot];
        thr = v3(1.0f, 1.0f, 1.0f); rad = v3(0.0f, 0.0f, 0.0f); bitfield = 0u; // :274-276
        alive = true;
      }
      preHead += take;
    }
    if (!__ballot(alive) && (!PARK || lotCount == 0u)) break; // (PARK: no work left, no ray pending, but parked hits: a trip without a walk shades them)
    phase(0, nIdle); trips++;

    // --- closest hit (traceRayEXT, rp_main.rgen:381-393): all rays of the wave advance in steps, triangles are tested cooperatively
    // Walk carry: the loop below runs until the SLOWEST of the wave's 64 incoherent rays is done, and its last steps pay the whole per-step cost (8-box node
    // test, scan, ring append, a partial triangle batch, pop) for a handful of lanes.  So once at most walkCarry lanes are still walking -- and more than that
    // entered, i.e. some lane has finished -- the loop ends; the stragglers skip this trip's shading and finish and go on walking in the NEXT trip's loop, beside
    // the new rays.  Their walk state is per lane already: group and stack pointer in R, the stack column in LDS, the nearest hit in W.best / W.hit[lane]; ro, rdv
    // and tMin stay put because a carried lane does nothing after the loop, and what trav_init derives from them is derived again.  Per-ray arithmetic, culling
    // distance and the atomicMin key are what they were: the walk of a ray is the same sequence of steps, cut in two.  If no more than walkCarry lanes enter (the
    // frame's tail) the loop runs to completion, so every trip retires at least one segment.  walkCarry = 0: every loop runs to completion.
    // Ring carry (NEE off): a step yields fewer (ray, triangle) pairs than a batch holds -- a trip's two to three steps make ~180 pairs, three batches' worth
    // -- and wave_step ends every step with a batch over whatever is pending, so a trip paid a partial batch per step on top of the full ones.  With ringCarry
    // the pending pairs live across the steps of this loop (wave_step_ring, gi_traversal.h): a batch runs whenever 64 are pending, and ONE flush in the loop's
    // last step -- the loop run to completion or ended early by the walk carry -- tests the rest.  Every lane of the trip reads its key at the end of every
    // step, so a lane whose walk ended in an early step has its final hit after that flush; it keeps R.o / R.d / tMin / rng untouched until then, which is
    // what its pending pairs read.  Nothing is pending at a trip boundary, so carried walks, adoption from the lot and regeneration see nothing of it.  Hit
    // keys do not depend on when a pair is tested: images and `segments` are the same; a walk may cull with a distance one step old, so nodes visited and
    // triangles tested can only grow.  ringCarry = 0: every step ends with that flush (the kernel before the carry).
    {
      const bool carried = CARRY && tAlive;
      const uint2 G = R.G; const uint32_t sp = R.sp;
      trav_init(R, ro, rdv, tMin, alive ? tMax : 0.0f);
      if (carried) { R.G = G; R.sp = sp; R.tBest = u2f(wt_best_t(W, lane)); }
      else wave_ray_begin(W, R.tBest);
    }
    tAlive = alive;
    if (CARRY) {
      unsigned long long walking = __ballot(tAlive);
      const uint32_t stop = (uint32_t)__popcll(walking) > walkCarry ? walkCarry : 0u;
      uint32_t step = 0u;
      uint32_t pend = 0u; // wave-uniform: pairs waiting in the queue (none when a trip's loop begins, none when it has ended)
      if ((uint32_t)__popcll(walking) > stop) for (;;) {
        if (COUNT) {
          const uint32_t n = (uint32_t)__popcll(walking);
          whLanes[step] += n; whTrips[step]++; step = step < 7u ? step + 1u : 7u;
          if (n < 8u) whFew++;
        }
        if (wave_step_ring<COUNT, PATH_STACK, STAGED_ALL, CUTOUT, COOK>(R, tAlive, W, sc, S, overflow, tc, rng, pend, ringN)) tAlive = false;
        walking = __ballot(tAlive);
        const bool last = (uint32_t)__popcll(walking) <= stop;
        if ((last || ringCarry == 0u) && pend != 0u) { // the one flush of the trip (ringCarry = 0: of every step)
          if (COUNT && ringCarry != 0u) ringN.flushes++;
          wave_ring_batch<COUNT, STAGED_ALL, CUTOUT>(W, pend, pend, R, rng, sc, S, tc, ringN);
        }
        // every lane of the trip picks up what the batches have found: a walking lane its culling distance, a lane whose walk has ended -- in this step or
        // an earlier one -- its hit, which is final after the flush of the last step
        __atomic_signal_fence(__ATOMIC_SEQ_CST);
        if (alive) wave_ring_refresh(R, W);
        if (last) break;
      }
    } else {
      while (__ballot(tAlive)) {
        if (wave_step<false, COUNT, PATH_STACK, false, STAGED_ALL, CUTOUT>(R, tAlive, W, sc, S, overflow, tc, rng)) tAlive = false;
      }
    }
    const bool walked = CARRY ? alive && !tAlive : alive; // this trip ended the lane's segment
    bool ended = false;
    ShadeIO io; io.shadow = false; io.shadowFirst = false; io.cont = false;
    if (DEFER) { io.lite = false; io.glossyLobe = false; io.deferred = false; }
    phase(1, (unsigned long long)__popcll(__ballot(walked)));
    // PARK: the per-sample finish (below) as a function -- a lane about to adopt a parked hit finishes its sample ahead of the trip's end
    auto finish_path = [&]() __attribute__((always_inline)) {
      const uint32_t bounces = bitfield & 0x00000fffu;
      if (st.bouncesAov && U.batchFirstSample + rec / U.pixelCount == U.spp - 1u) {
        const uint32_t maxB = U.maxBounces < 0x00000fffu ? U.maxBounces : 0x00000fffu;
        const V3 c = gi_colormap_inferno((float)bounces / (float)maxB);
        F4* dst = &st.bouncesAov[tile_to_image_pixel(U, rec % U.pixelCount)];
        dst->x = c.x; dst->y = c.y; dst->z = c.z;
      }
      if (st.pathSegments) atomicAdd(&st.pathSegments[rec % U.pixelCount], bounces);
      const V3 c = finish_sample(U, rad);
      st4(&sampleBuf[rec], c.x, c.y, c.z, 0.0f);
      alive = false;
    };
    bool shaded = false; // PARK: this trip shaded a hit of the lane's path (not always the segment the lane walked)
    uint32_t nEarly = 0u; // PARK (wave-uniform): samples finished ahead of the trip's end, by lanes about to adopt
    if (walked) {
      nSeg++;
      wave_ray_end(W, R);
      if (R.found) { // rp_main.chit + rp_main.rgen:397-480
        if constexpr (!PARK) {
          io.throughput = thr; io.radiance = rad; io.bitfield = bitfield; io.rng = rng;
          const F4 h = F4{R.tBest, R.bestU, R.bestV, u2f(R.bestTri)}, rd = F4{rdv.x, rdv.y, rdv.z, 0.0f};
          shade_segment<KLASS, TEXTURED, false, NEE, false, DEFER, UPS>(U, sc, nullptr, h, rd, io);
          thr = io.throughput; rad = io.radiance; bitfield = io.bitfield; rng = io.rng;
          // untraced shadow ray == "not shadowed" (rp_main.rgen:431-435)
          if (NEE && st.neeKey && io.shadowFirst && !io.shadow) nee_aov_record_px(st, rec % U.pixelCount, rec / U.pixelCount, false);
          ended = !io.cont;
          shaded = true;
        } // (PARK: below)
      } else { // rp_main.miss:68-86: uniform fallback dome == colour clear value; the loop's bounce++ still happens (rp_main.rgen:480)
        rad = rad + thr * v3(U.background);
        if (st.neeKey && (bitfield & 0x00000fffu) == 0u) nee_aov_record_px(st, rec % U.pixelCount, rec / U.pixelCount, false);
        bitfield++;
        ended = true;
      }
    }
    // Lobe parking.  A class-1 hit draws its lobe from x2, and the glossy ones (coat, specular: ggx_sample, two normalisations, eight more square roots, nine
    // divisions -- a fifth of this kernel's VALU instructions) are few: on C2 3 .. 4 of a trip's ~40 hits, yet nearly every trip has one, so the wave issued
    // that block on every trip for a twentieth of its lanes.  Now most trips are LITE: shade_segment leaves a hit that drew a glossy lobe untouched (`deferred`),
    // the lane writes the hit's pre-shade state -- throughput, radiance, bitfield, rng, rec, ray direction, (t, u, v, triangle): 16 dwords -- to the lot by
    // ballot rank and is free; the next trip's regeneration gives it a camera ray.  Once the lot holds parkAt records, or the wave is draining (no work left to
    // claim, ring empty), the trip is FULL: the lanes whose segment missed finish their sample first, free lanes adopt the top records of the lot -- an adopting
    // lane becomes that path, rec included -- and shade_segment runs with lite = false for the trip's own hits and the adopted ones together.
    // Overflow rule: the lot never takes part of a trip's deferred hits.  If they do not all fit (a material whose hits nearly all go glossy: a metal), the
    // trip's shade is run again on the spot as FULL for exactly those hits, beside whatever the lot holds; no lane keeps a hit across trips outside the lot.
    // Invariants: a path's sequence of draws and operations is what it was -- shading from the parked state repeats the same arithmetic; only the trip in which
    // the path advances differs, and nSeg counts a segment where its walk ends, not again at adoption.  Carried walker (alive, still walking) and free are
    // exclusive lane states, and only free lanes adopt.  Every trip retires a segment, or adds to the lot (at most lotMax records), or -- FULL -- takes from
    // it; the trip loop ends only with no lane alive AND the lot empty, so a launch hands nothing to the next.  parkAt = 0: every trip is FULL over an empty
    // lot, which is the kernel without parking.
    if constexpr (PARK) {
      bool hit = walked && R.found; // the lane holds a hit to shade
      // the shade of the hit in R for the path in the lane's registers; a deferred hit (io.lite) leaves everything as it was
      auto shade_hit = [&]() __attribute__((always_inline)) {
        io.throughput = thr; io.radiance = rad; io.bitfield = bitfield; io.rng = rng;
        const F4 h = F4{R.tBest, R.bestU, R.bestV, u2f(R.bestTri)}, rd = F4{rdv.x, rdv.y, rdv.z, 0.0f};
        shade_segment<KLASS, TEXTURED, false, NEE, false, DEFER, UPS>(U, sc, nullptr, h, rd, io);
        if (io.deferred) return;
        thr = io.throughput; rad = io.radiance; bitfield = io.bitfield; rng = io.rng;
        ended = !io.cont;
        shaded = true;
        // (the next ray is taken here and not at the trip's end: a second pass of the shade would otherwise hold every out field of the first alive)
        if (!ended) { ro = io.no; rdv = io.k2; tMin = 0.0f; tMax = io.tMaxNext; }
      };
      // (a trip without a hit of its own has nothing to set aside: FULL, so that a wave left with parked hits alone always takes from the lot)
      bool lite = lotCount < parkAt && !(exhausted && preTail == preHead) && __ballot(hit) != 0ull;
      if (COUNT && parkAt) lobeN[lite ? 3 : 4]++;
      for (;;) {
        if (!lite && lotCount) {
          nEarly += (uint32_t)__popcll(__ballot(ended));
          if (ended) { finish_path(); ended = false; }
          const unsigned long long freeLanes = __ballot(!alive);
          const uint32_t nFree = (uint32_t)__popcll(freeLanes), nAdopt = nFree < lotCount ? nFree : lotCount;
          const uint32_t rank = (uint32_t)__popcll(freeLanes & below);
          __atomic_signal_fence(__ATOMIC_SEQ_CST); // (compiler only) the records were written by other lanes of this wave
          if (!alive && rank < nAdopt) {
            volatile GI_LDS gi_u4* p = lot_record(lotCount - nAdopt + rank);
            const gi_u4 a = p[0], b = p[1], c = p[2], d = p[3];
            thr = v3(u2f(a.x), u2f(a.y), u2f(a.z)); bitfield = a.w; rad = v3(u2f(b.x), u2f(b.y), u2f(b.z)); rng = b.w;
            rdv = v3(u2f(c.x), u2f(c.y), u2f(c.z)); rec = c.w; R.tBest = u2f(d.x); R.bestU = u2f(d.y); R.bestV = u2f(d.z); R.bestTri = d.w;
            alive = true; hit = true;
          }
          lotCount -= nAdopt;
          if (COUNT) lobeN[6] += nAdopt;
        }
        io.lite = lite;
        if (hit) shade_hit();
        const unsigned long long deferred = lite ? __ballot(hit && io.deferred) : 0ull;
        if (!deferred) break;
        const uint32_t nDeferred = (uint32_t)__popcll(deferred);
        if (lotCount + nDeferred <= lotMax) {
          if (hit && io.deferred) {
            volatile GI_LDS gi_u4* p = lot_record(lotCount + (uint32_t)__popcll(deferred & below));
            p[0] = gi_u4{f2u(thr.x), f2u(thr.y), f2u(thr.z), bitfield}; p[1] = gi_u4{f2u(rad.x), f2u(rad.y), f2u(rad.z), rng};
            // (a deferring lane walked this trip: its hit is still in the wave's record, so (t, u, v, triangle) need not stay in registers through the shade)
            const uint4 wh = wt_hit_get(W, lane);
            p[2] = gi_u4{f2u(rdv.x), f2u(rdv.y), f2u(rdv.z), rec}; p[3] = gi_u4{wt_best_t(W, lane), wh.y, wh.z, wh.x};
            alive = false;
          }
          __atomic_signal_fence(__ATOMIC_SEQ_CST);
          lotCount += nDeferred;
          if (COUNT) lobeN[5] += nDeferred;
          break;
        }
        hit = hit && io.deferred; lite = false; // the overflow rule: this trip's deferred hits are shaded now
        if (COUNT) { lobeN[7]++; lobeN[8] += nDeferred; }
      }
    }
    if (COUNT) {
      const unsigned long long glossy = __ballot(shaded && io.glossyLobe);
      lobeN[0] += (uint32_t)__popcll(__ballot(shaded)); lobeN[1] += (uint32_t)__popcll(glossy); lobeN[2] += glossy ? 1u : 0u;
    }
    phase(2, (unsigned long long)__popcll(__ballot(PARK ? shaded : walked && R.found)));

    // --- shadow ray of this bounce (rp_main.rgen:397-429): origin = next ray origin, tMin 0.01, tMax = distance to the light sample
    if (NEE) {
      bool sAlive = alive && io.shadow;
      if (__ballot(sAlive)) {
        trav_init(R, io.no, io.sdir, 0.01f, sAlive ? io.ld : 0.0f);
        wave_ray_begin(W, R.tBest);
        const bool traced = sAlive;
        while (__ballot(sAlive)) {
          if (wave_step<true, COUNT, PATH_STACK, false, STAGED_ALL, CUTOUT>(R, sAlive, W, sc, S, overflow, tcs, io.rngShadow)) sAlive = false;
        }
        if (traced) {
          nShadow++;
          if (!R.found) rad = rad + io.nee;
          if (st.neeKey && io.shadowFirst) nee_aov_record_px(st, rec % U.pixelCount, rec / U.pixelCount, R.found);
        }
      }
    }

    // --- next segment, or the per-sample finish (rp_main.rgen:483-496) -> per-sample colour buffer
    if constexpr (PARK) { if (ended) finish_path(); } // (a path that goes on took its next ray where it was shaded)
    else if (walked) {
      if (!ended) { ro = io.no; rdv = io.k2; tMin = 0.0f; tMax = io.tMaxNext; }
      else {
        const uint32_t bounces = bitfield & 0x00000fffu;
        if (st.bouncesAov && U.batchFirstSample + rec / U.pixelCount == U.spp - 1u) { // Bounces AOV: the pixel's last sample (:483-486)
          const uint32_t maxB = U.maxBounces < 0x00000fffu ? U.maxBounces : 0x00000fffu;
          const V3 c = gi_colormap_inferno((float)bounces / (float)maxB);
          F4* dst = &st.bouncesAov[tile_to_image_pixel(U, rec % U.pixelCount)];
          dst->x = c.x; dst->y = c.y; dst->z = c.z;
        }
        if (st.pathSegments) atomicAdd(&st.pathSegments[rec % U.pixelCount], bounces); // ClockCycles proxy: integer sum, order-free
        const V3 c = finish_sample(U, rad);
        st4(&sampleBuf[rec], c.x, c.y, c.z, 0.0f);
        alive = false;
      }
    }
    phase(3, (unsigned long long)__popcll(__ballot(ended)) + nEarly);
  }

  if (COUNT
      && lane == 0u) { for (int k = 0; k < 4; k++) { atomicAdd(&cnt->phaseCycles[k], pc[k]); atomicAdd(&cnt->phaseLanes[k], pl[k]);
      } atomicAdd(&cnt->phaseTrips, trips);
      for (int k = 0; k < 8; k++) { atomicAdd(&cnt->walkStepLanes[k], (unsigned long long)whLanes[k]); atomicAdd(&cnt->walkStepTrips[k], (unsigned long long)whTrips[k]); }
      atomicAdd(&cnt->walkFewLaneSteps, (unsigned long long)whFew);
      for (int k = 0; k < 9; k++) atomicAdd(&cnt->lobeStats[k], (unsigned long long)lobeN[k]);
      if (CARRY) { atomicAdd(&cnt->ringStats[0], (unsigned long long)ringN.batches); atomicAdd(&cnt->ringStats[1], (unsigned long long)ringN.pairs);
        atomicAdd(&cnt->ringStats[2], (unsigned long long)ringN.partial); atomicAdd(&cnt->ringStats[3], (unsigned long long)ringN.flushes);
        atomicAdd(&cnt->ringStats[4], (unsigned long long)ringN.ballotSteps); } }
  // statistics: one atomic per wave and counter
  unsigned long long a = nSeg, b = nShadow, c = tc.nodes, d = tc.tris, e = tcs.nodes, f = tcs.tris;
  for (int off = 32; off > 0; off >>= 1) {
    a += __shfl_down(a, off); b += __shfl_down(b, off);
    if (COUNT) { c += __shfl_down(c, off); d += __shfl_down(d, off); e += __shfl_down(e, off); f += __shfl_down(f, off); }
  }
  if (lane == 0u) {
    atomicAdd(&cnt->segments, a);
    if (NEE) atomicAdd(&cnt->shadowRays, b);
    if (COUNT) { atomicAdd(&cnt->nodesVisited, c); atomicAdd(&cnt->trisTested, d); atomicAdd(&cnt->shadowNodesVisited, e); atomicAdd(&cnt->shadowTrisTested, f);
        }
  }
  if constexpr (COUNT) { // Counters::stackHigh: the fullest stack of any lane's walks
    uint32_t hc = tc.high, hs = tcs.high;
    for (int off = 32; off > 0; off >>= 1) {
      const uint32_t oc = (uint32_t)__shfl_down((int)hc, off), os = (uint32_t)__shfl_down((int)hs, off);
      hc = oc > hc ? oc : hc; hs = os > hs ? os : hs;
    }
    if (lane == 0u) { atomicMax(&cnt->stackHigh[0], hc); if (NEE) atomicMax(&cnt->stackHigh[1], hs); }
  }
}

// ------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------
bool pathKernelSupports(const SceneView& sc)
{
  return sc.triCount > 0u && sceneFitsLds(sc.nodeCount, sc.triCount) && sc.bvhDepth <= PATH_STACK_MAX && sc.mediumStackSize == 0u
      && sc.domeTexture == 0u && !sc.twoLevel
         // (a scene whose shading records are packed -- never an LDS-resident one today:
         // TriRec::vi[0] is a shading-record index there, the fused kernels read vertex indices)
         && !sc.shadePacked;
}

uint32_t pathCookedLdsBytes(uint32_t stackEntries, uint32_t ldsNodes, uint32_t ldsTris)
{
  return stackEntries * TRACE_BLOCK * (uint32_t)sizeof(uint2) + cook_image_bytes(ldsNodes) + ldsTris * LDS_TRI_BYTES;
}

using PathKernel = void (*)(FrameUniforms, SceneView, PathState, Counters*, F4*, uint32_t, uint32_t, uint32_t, uint32_t, uint32_t, uint32_t, uint32_t, uint32_t);
// Hot variants: one material class, no textures, no cutouts, no counters (the C1 / C2 paths).  Everything else runs the general
// variant (class read from the material record, textures and cutouts compiled in).
// cook: the COOK instantiation of the kernel the other arguments pick, or nullptr where there is none (pathCookVariant)
template <uint32_t STACK>
static PathKernel pickPathKernel(uint32_t classMask, bool textured, bool nee, bool cutout, bool count, uint32_t upsTraits, bool cook = false)
{
  const bool hot = (classMask == 1u || classMask == 2u || classMask == 4u) && !textured && !cutout && !count;
  const uint32_t ups = pathUpsVariant(classMask, textured, nee, cutout, count, upsTraits);
  if (cook) {
    if (!pathCookVariant(classMask, textured, nee, cutout, count)) return nullptr;
    if (classMask == 1u) return k_path<0u, false, false, false, false, STACK, 0u, true>;
    if (ups == UPS_NOCOAT) return k_path<1u, false, false, false, false, STACK, UPS_NOCOAT, true>;
    return k_path<1u, false, false, false, false, STACK, 0u, true>;
  }
  return dispatchBools([&](auto neeC) -> PathKernel {
    constexpr bool NEE = decltype(neeC)::value;
    if (hot) {
      if (classMask == 1u) return k_path<0u, false, NEE, false, false, STACK>;
      if constexpr (!NEE) { // the plain UsdPreviewSurface variant (gi_shading.h ups_plain_sample)
        if (ups == UPS_NOCOAT) return k_path<1u, false, false, false, false, STACK, UPS_NOCOAT>;
      }
      if (classMask == 2u) return k_path<1u, false, NEE, false, false, STACK>;
      return k_path<2u, false, NEE, false, false, STACK>;
    }
    return dispatchBools([](auto countC) -> PathKernel { return k_path<KLASS_DYNAMIC, true, NEE, true, decltype(countC)::value, STACK>; }, count);
  }, nee);
}

int launchPath(hipStream_t s, uint32_t cuCount, uint32_t classMask, bool textured, bool count, uint32_t chunk, uint32_t walkCarry, uint32_t lobePark,
               uint32_t ringCarry, uint32_t upsTraits, uint32_t nodeCook, const FrameUniforms& U, const SceneView& sc, const PathState& st, Counters* cnt,
               F4* sampleBuf, uint32_t* cooked)
{
  if (cooked) *cooked = 0u;
  if (U.workTotal == 0u) return 0; // an empty active rectangle (FLAG_MISS_RECT, the camera looks away): no pixel needs a path
  const uint32_t ldsNodes = sc.nodeCount, ldsTris = sc.triCount;
  const PathLot lot = pathLotPlacement(sc.bvhDepth); // the stack rows, and in them the home of k_path's parked hits: no LDS of its own
  const uint32_t stack = lot.stack;
  assert(sc.bvhDepth <= stack && lot.row >= sc.bvhDepth && lot.row + (lot.capacity + 7u) / 8u <= stack); // the walks own rows [0, bvhDepth), the lot the rest
  uint32_t bytes = traceLdsBytes(stack, ldsNodes, ldsTris);
  const bool neeOn = (U.flags & FLAG_NEE) != 0u;
  PathKernel k = stack == 4u
      ? pickPathKernel<4u>(classMask, textured, neeOn, sc.hasCutouts != 0u, count, upsTraits)
      : pickPathKernel<8u>(classMask, textured, neeOn, sc.hasCutouts != 0u, count, upsTraits);
  // Cooked nodes (gi_node_cook.h, trav_node_test_cooked): the COOK instantiation of the same kernel, where there is one and the larger node image costs no
  // resident block -- the instructions a node test saves are worth less than a wave per SIMD.  Derived from the two LDS sizes, nothing tuned.
  if (nodeCook != 0u) {
    PathKernel kc = stack == 4u
        ? pickPathKernel<4u>(classMask, textured, neeOn, sc.hasCutouts != 0u, count, upsTraits, true)
        : pickPathKernel<8u>(classMask, textured, neeOn, sc.hasCutouts != 0u, count, upsTraits, true);
    hipFuncAttributes fr{}, fc{};
    if (kc && hipFuncGetAttributes(&fr, reinterpret_cast<const void*>(k)) == hipSuccess
        && hipFuncGetAttributes(&fc, reinterpret_cast<const void*>(kc)) == hipSuccess) {
      const uint32_t cookedBytes = pathCookedLdsBytes(stack, ldsNodes, ldsTris);
      if (blocksPerCuByLds(cookedBytes, (uint32_t)fc.sharedSizeBytes) >= blocksPerCuByLds(bytes, (uint32_t)fr.sharedSizeBytes)) {
        k = kc; bytes = cookedBytes;
        if (cooked) *cooked = 1u;
      }
    }
  }
  // Resident blocks per CU (4 waves per block = 1 wave per SIMD and block): the smaller of what the 160 KiB of LDS and the 512-entry
  // register file of a SIMD hold.  (hipOccupancyMaxActiveBlocksPerMultiprocessor answered 3 for a 35 KiB block: it does not know gfx950's LDS size.)
  int perCu = 2;
  hipFuncAttributes fa{};
  if (hipFuncGetAttributes(&fa, reinterpret_cast<const void*>(k)) == hipSuccess && fa.numRegs > 0) {
    const uint32_t regs = ((uint32_t)fa.numRegs + 7u) & ~7u, byRegs = 512u / regs;
    const uint32_t byLds = blocksPerCuByLds(bytes, (uint32_t)fa.sharedSizeBytes);
    perCu = (int)(byRegs < byLds ? byRegs : byLds);
    if (perCu > 8) perCu = 8;
    if (perCu < 1) perCu = 1;
  }
  // persistent grid: what is resident, but never more waves than chunks of work
  const uint64_t chunks = ((uint64_t)U.workTotal + chunk - 1u) / chunk;
  uint64_t blocks = (uint64_t)cuCount * (uint64_t)perCu;
  const uint64_t needed = (chunks + (TRACE_BLOCK / 64u) - 1u) / (TRACE_BLOCK / 64u);
  if (blocks > needed) blocks = needed;
  if (blocks == 0u) blocks = 1u;
  hipLaunchKernelGGL(k, dim3((uint32_t)blocks), dim3(TRACE_BLOCK), bytes, s, U, sc, st, cnt, sampleBuf, ldsNodes, ldsTris, chunk, walkCarry, lobePark, lot.row, lot.capacity, ringCarry);
  return perCu;
}

// k_debug_sqrt: gi_sqrt (gi_device_math.h) against sqrtf over a range of bit patterns; counts the arguments whose results differ in a bit (NaN against NaN is equal
// whatever the payload: both come out of v_sqrt_f32 here, but the contract does not say so)
__global__ void k_debug_sqrt(uint32_t first, unsigned long long count, unsigned long long* mismatches)
{
  unsigned long long bad = 0ull;
  for (unsigned long long i = blockIdx.x * (unsigned long long)blockDim.x + threadIdx.x; i < count; i += (unsigned long long)gridDim.x * blockDim.x) {
    const float x = u2f(first + (uint32_t)i);
    const float a = gi_sqrt(x), b = sqrtf(x);
    if (f2u(a) != f2u(b) && !(a != a && b != b)) bad++;
  }
  if (bad) atomicAdd(mismatches, bad);
}

void launchDebugSqrt(hipStream_t s, uint32_t first, unsigned long long count, unsigned long long* mismatches)
{
  hipLaunchKernelGGL(k_debug_sqrt, dim3(4096), dim3(256), 0, s, first, count, mismatches);
}

// k_debug_div: the lean division (gi_device_math.h gi_div, the three-quotient V3 / float and normalize) against the compiler's `/`; counts the items for which any
// result differs in a bit (NaN against NaN is equal whatever the payload).  Both forms of the range test run: the wave's (what the kernels execute -- one
// out-of-range lane sends all 64 to `/`) and the lane's (so an in-range item is held to the lean sequence whatever its neighbours are).
// Items: mode 0 -- `count` pairs (n, d) of `words`; mode 1 -- pairs drawn from a hash of (seed, index), every bit pattern equally likely; mode 2 -- `count` vectors
// (x, y, z, s) of `words`: normalize(x, y, z) and (x, y, z) / s; mode 3 -- vectors from the hash: each component's exponent is uniform over all 256 in one item of
// four and within +-24 of 1.0 in the others, and of the latter every eighth component is a zero or a denormal; mode 4 -- the reciprocal (gi_rcp) and the
// reciprocal square root (gi_rsqrt) of the `count` bit patterns from `seed` on.  Modes 0 and 1 also hold gi_rcp of the denominator to 1 / d.
__device__ __forceinline__ bool debug_same(float a, float b) { return f2u(a) == f2u(b) || (a != a && b != b); }
__device__ __forceinline__ bool debug_same(V3 a, V3 b) { return debug_same(a.x, b.x) && debug_same(a.y, b.y) && debug_same(a.z, b.z); }
__global__ void k_debug_div(uint32_t mode, unsigned long long count, uint32_t seed, const uint32_t* __restrict__ words, unsigned long long* mismatches)
{
  unsigned long long bad = 0ull;
  for (unsigned long long i = blockIdx.x * (unsigned long long)blockDim.x + threadIdx.x; i < count; i += (unsigned long long)gridDim.x * blockDim.x) {
    uint32_t w[4];
    if (mode == 4u) { w[0] = w[1] = w[2] = w[3] = 0u; }
    else if (mode == 0u) { w[0] = words[2ull * i]; w[1] = words[2ull * i + 1ull]; w[2] = w[3] = 0u; }
    else if (mode == 2u) { for (int k = 0; k < 4; k++) w[k] = words[4ull * i + k]; }
    else {
      for (uint32_t k = 0; k < 4u; k++) w[k] = gi_hash_init(gi_hash_init(seed + k) ^ (uint32_t)i) + gi_hash_init((uint32_t)(i >> 32) + 0x9e3779b9u * (k + 1u));
      if (mode == 3u && (w[3] & 3u)) {
        const uint32_t sel = gi_hash_init(w[0] ^ w[3]);
        for (uint32_t k = 0; k < 4u; k++) {
          const uint32_t e = 103u + ((w[k] >> 23) & 0xffu) % 49u;
          w[k] = (w[k] & 0x807fffffu) | (e << 23);
          const uint32_t c = (sel >> (8u * k)) & 0xffu;
          if ((c & 7u) == 0u) w[k] &= (c & 8u) ? 0x80000000u : 0x807fffffu;
        }
      }
    }
    bool same;
    if (mode == 4u) { // the reciprocal of the bit pattern seed + index (count = 2^32: every float)
      const float d = u2f(seed + (uint32_t)i), q = 1.0f / d, rs = 1.0f / sqrtf(d);
      same = debug_same(gi_rcp<true>(d), q) && debug_same(gi_rcp<false>(d), q) && debug_same(gi_rsqrt<true>(d), rs) && debug_same(gi_rsqrt<false>(d), rs);
    } else if (mode < 2u) {
      const float n = u2f(w[0]), d = u2f(w[1]), q = n / d, rq = 1.0f / d;
      same = debug_same(gi_div<true>(n, d), q) && debug_same(gi_div<false>(n, d), q) && debug_same(gi_rcp<true>(d), rq) && debug_same(gi_rcp<false>(d), rq);
    } else {
      const V3 a = v3(u2f(w[0]), u2f(w[1]), u2f(w[2])); const float s = u2f(w[3]);
      const V3 nrm = a * (1.0f / sqrtf(dot(a, a))), quo = V3{a.x / s, a.y / s, a.z / s};
      same = debug_same(normalize<true>(a), nrm) && debug_same(normalize<false>(a), nrm) && debug_same(gi_div3<true>(a, s), quo) && debug_same(gi_div3<false>(a, s), quo);
    }
    if (!same) bad++;
  }
  if (bad) atomicAdd(mismatches, bad);
}

void launchDebugDiv(hipStream_t s, uint32_t mode, unsigned long long count, uint32_t seed, const uint32_t* words, unsigned long long* mismatches)
{
  hipLaunchKernelGGL(k_debug_div, dim3(4096), dim3(256), 0, s, mode, count, seed, words, mismatches);
}

// k_debug_node_cook: trav_node_test against trav_node_test_cooked.  Every block cooks the `nodeCount` (<= DEBUG_COOK_NODES) nodes into its LDS as k_path's stage
// does (cook_place) and then takes pairs: pair i = ray i (eight words: origin, direction, tMin, tBest) on node i % nodeCount.  Counts the pairs for which R.G or
// the returned triangle group differ in a bit.  The cooked test's child loop ends at a bound of the wave, so a wave of mixed nodes is part of what is held.
constexpr uint32_t DEBUG_COOK_NODES = 64;
__global__ __launch_bounds__(TRACE_BLOCK) void k_debug_node_cook(const Node8* __restrict__ nodes, uint32_t nodeCount, const float* __restrict__ rays,
                                                                 unsigned long long count, unsigned long long* mismatches)
{
  __shared__ uint4 s_image[(DEBUG_COOK_NODES * COOK_NODE_BYTES + DEBUG_COOK_NODES * COOK_OCT_DWORDS * 4u) / sizeof(uint4)];
  if (nodeCount == 0u || nodeCount > DEBUG_COOK_NODES) return;
  for (uint32_t i = threadIdx.x; i < nodeCount; i += TRACE_BLOCK) cook_place(nodes, i, nodeCount, DEBUG_COOK_NODES, reinterpret_cast<uint32_t*>(s_image));
  __syncthreads();
  unsigned long long bad = 0ull;
  for (unsigned long long i = blockIdx.x * (unsigned long long)blockDim.x + threadIdx.x; i < count; i += (unsigned long long)gridDim.x * blockDim.x) {
    const float* r = rays + 8ull * i;
    const uint32_t nodeIdx = (uint32_t)(i % nodeCount);
    RayWalk A, B;
    walk_init(A, v3(r[0], r[1], r[2]), v3(r[3], r[4], r[5]), r[6], r[7]);
    B = A;
    const uint4* p = reinterpret_cast<const uint4*>(nodes) + nodeIdx * 5u;
    const uint2 ga = trav_node_test<false, true>(A, p[0], p[1], p[2], p[3], p[4]);
    const uint2 gb = trav_node_test_cooked(B, (const GI_LDS gi_u4*)((const GI_LDS char*)s_image + __umul24(nodeIdx, COOK_NODE_BYTES)));
    if (A.G.x != B.G.x || A.G.y != B.G.y || ga.x != gb.x || ga.y != gb.y) bad++;
  }
  if (bad) atomicAdd(mismatches, bad);
}

int launchDebugNodeCook(hipStream_t s, const Node8* nodes, uint32_t nodeCount, const float* rays, unsigned long long count, unsigned long long* mismatches)
{
  if (nodeCount == 0u || nodeCount > DEBUG_COOK_NODES) return -1;
  hipLaunchKernelGGL(k_debug_node_cook, dim3(256), dim3(TRACE_BLOCK), 0, s, nodes, nodeCount, rays, count, mismatches);
  return 0;
}

} // namespace gi

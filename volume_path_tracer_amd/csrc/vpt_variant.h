// vpt_variant.h — which instantiations of the integrate kernel exist, and what a launch of render() looks like: the
// kernel variant (KernelVariant, variant_valid: the one statement of the rule; DESIGN.md "Kernel variants and the launch
// plan") and the launch plan (plan_launch: grid size, kernel, gate set, job order -- host arithmetic without a HIP call,
// so tests/native/launch_plan_host.cpp runs it on the CPU).  Includes no HIP header.  The kernel (vpt_kernels.h) takes its
// static_assert, launch bound and evaluation split from here; vpt_gpu.hip builds its kernel table from variant_valid.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>

#include "../../include/vpt_gpu.h"
#include "vpt_launch.h"

namespace vpt {

// Minimum waves per SIMD (launch bounds): 7 for the production density-only kernel (72 VGPRs; the
// cold lane state lives in LDS, see LaneCold), 6 for the temperature kernel (C4: 3748 Msps at its
// natural 5, 3809 at 6, 3684 at 7), 4 for the per-sample-record / event variants.  The kernel is latency-bound enough that occupancy pays: persistent grids of 3/4/5
// blocks per CU measured 802/956/1067 Msps on C3 with one binary; 6 waves 1155, 7 waves 1194.
#ifndef VPT_WAVES_FAST
#define VPT_WAVES_FAST 7
#endif
#ifndef VPT_WAVES_SLOW
#define VPT_WAVES_SLOW 4
#endif
#ifndef VPT_WAVES_TEMP
#define VPT_WAVES_TEMP 6
#endif
// The latency kernel (partly filled and latency-bound launches: C1, C2, a GPU's small share of a frame):
// at most VPT_WAVES_LAT waves per SIMD run anyway there, so it trades occupancy for registers -- the
// lane's cold state in VGPRs instead of LDS (no LDS round trips on the per-pixel / per-bounce chain)
// and a 512 / VPT_WAVES_LAT register budget.
#ifndef VPT_WAVES_LAT
#define VPT_WAVES_LAT 4
#endif

// The compacting kernel's exchange (vpt_kernels.h xchg_pack): words per lane, and its dynamic LDS.
constexpr int kXWords = 60;  // 54 state words (58 with a temperature grid), padded to uint4
// Dynamic LDS of the compacting kernel: [kXWords / 4][kBlockThreads] uint4 (61 440 B).
constexpr size_t kXchgBytes = (size_t)kXWords * kBlockThreads * sizeof(uint32_t);
// Latency-bound launches: at most this many work items per wavefront of the grid (see plan_launch).
constexpr uint64_t kSpreadLanes = 6;
// A cost-ordered launch's group unless it takes the same-tile order: vpt_integrator.h's kOrderGroup (a header of device
// code; vpt_gpu.hip asserts the two equal).
constexpr uint32_t kPlanOrderGroup = 64;

// One instantiation of vpt_integrate_kernel: its template bools, in the template's order.
struct KernelVariant {
  bool temp = false, debug = false, runs = false, lat = false, compact = false, feed = false, band = false, gang = false,
       groups = false, shutter = false;
};
constexpr int kVariantFlags = 10;
constexpr uint32_t kVariantCount = 1u << kVariantFlags;

// The instantiations that exist: three base kernels (temperature, run-skipping, plain) times records / events; the
// latency kernel and its compacting form; a feed's; a gang's; light groups and / or a shutter on the throughput kernel;
// and band launches of all but the debug, feed and gang ones.  15 per base kernel, 45 in all.
constexpr bool variant_valid(const KernelVariant& v) {
  const bool axes = v.lat || v.compact || v.band || v.groups || v.shutter;  // (what follows Runs, but feed and gang)
  return !(v.temp && v.runs) &&                // a temperature grid has no run-skipping kernel
         !(v.compact && !v.lat) &&             // compaction runs in the latency kernel only
         !(v.debug && (axes || v.feed || v.gang)) &&  // records / events: the three base kernels alone (no band either)
         !(v.feed && (axes || v.gang)) &&      // feeds run the throughput kernels only; band launches are no feeds
         !(v.gang && (axes || v.feed)) &&      // gang launches run the plain throughput kernels only
         !((v.groups || v.shutter) && v.lat);  // light groups and a shutter run the throughput kernels, plain or band
}

// The instantiations that split the density evaluation: the density-only production kernels of the throughput
// family -- plain, run-skipping, feed, band and gang.  The stencil's eight registers fit across the rare blocks of
// the 72-VGPR kernel only: the temperature kernel (80 VGPRs at 6 waves, none to spare), the records / events kernels
// and the latency and compacting kernels (the lane's cold state in VGPRs) evaluate whole, with the code they had.
constexpr bool variant_eval_split(const KernelVariant& v) { return !v.temp && !v.debug && !v.lat; }

// The kernel's launch bound: minimum waves per SIMD (VPT_WAVES_*; the compacting kernel's LDS exchange allows 2).
constexpr int variant_waves_per_simd(const KernelVariant& v) {
  return v.compact ? 2 : (v.lat ? VPT_WAVES_LAT : (v.debug ? VPT_WAVES_SLOW : (v.temp ? VPT_WAVES_TEMP : VPT_WAVES_FAST)));
}

// A variant's index: its flags as binary digits, HasTemp the most significant -- the digit string of the kernel's
// mangled name (tools/isa_blocks.py) read as a number.
constexpr uint32_t variant_index(const KernelVariant& v) {
  const bool f[kVariantFlags] = {v.temp, v.debug, v.runs, v.lat, v.compact, v.feed, v.band, v.gang, v.groups, v.shutter};
  uint32_t i = 0;
  for (int k = 0; k < kVariantFlags; ++k) i = 2 * i + (f[k] ? 1u : 0u);
  return i;
}
constexpr KernelVariant variant_decode(uint32_t i) {
  auto bit = [i](int k) { return ((i >> (kVariantFlags - 1 - k)) & 1u) != 0; };
  return KernelVariant{bit(0), bit(1), bit(2), bit(3), bit(4), bit(5), bit(6), bit(7), bit(8), bit(9)};
}

// The base kernel of a context's grids: temperature, else run-skipping where the context chose it, else plain.
constexpr KernelVariant base_variant(bool has_temperature, bool use_runs) {
  KernelVariant v;
  v.temp = has_temperature;
  v.runs = !has_temperature && use_runs;
  return v;
}

// What render()'s decisions read: the job range, the context's sizes and knobs, and what is attached to the launch.
struct LaunchInputs {
  uint64_t jid_begin = 0, jid_count = 0, T = 1;
  uint32_t tile_area = 1;
  int grid_blocks = 0, grid_user = 0, cus = 1, lat_per_cu = 0, lat_mode = -1, lat_ungated = 0, compact_every = 0,
      compact_per_cu = 0;
  bool has_temperature = false, use_runs = false, pixel_mode = false;
  int pixel_chunk = 0;
  int order_mode = VPT_ORDER_COST_SAME_TILE, order_tail_waves = 0, film_order = VPT_FILM_ORDERED;
  uint64_t frame_waves = 0;
  bool records = false, events = false, feed = false, band = false;
  bool groups = false, shutter = false, moments = false;  // attached to the context (a feed ignores groups and moments)
};

struct LaunchPlan {
  KernelVariant variant;
  uint32_t blocks = 0;
  size_t lds_bytes = 0;           // dynamic LDS
  int gate_set = VPT_GATES_CONTEXT;  // the scene copy the kernel reads (VPT_GATES_*)
  bool latency = false;           // a latency-bound launch
  uint32_t pixel_chunk = 1;
  uint64_t items = 0;             // work items (KernelArgs::jid_count)
  bool ordered = false;           // an ordered production launch of the reference RNG mode
  bool cost_order = false;        // takes the jobs in cost order (KernelArgs::order)
  uint32_t order_group = kPlanOrderGroup, order_tail_n = 0, order_tail_k0 = 0, compact_every = 0;
  bool zero_region1 = false;      // light groups without a temperature grid: the emission region is the host's
};

// Light groups reach the launch (a feed never writes them).
inline bool launch_groups(const LaunchInputs& in) { return in.groups && !in.feed; }
// The ordered film: production launches of the reference RNG mode (debug launches and feeds add atomically).
inline bool launch_ordered(const LaunchInputs& in) {
  return in.film_order == VPT_FILM_ORDERED && !in.feed && !in.records && !in.events && !in.pixel_mode;
}
// An attachment refuses the launch.  The moment plane (vpt_gpu_set_film_moments) and the light-group planes are written
// by the ordered film passes only: a launch that would add with film atomics fails instead of leaving the planes behind
// the film (feeds never write them).  The shutter (vpt_gpu_set_shutter) is honoured by the ordered production launches'
// Shutter kernels only; any other launch fails instead of rendering the still camera.
inline bool attachments_refuse(const LaunchInputs& in) {
  return (((in.moments || in.groups) && !in.feed) || in.shutter) && (!launch_ordered(in) || in.frame_waves);
}

// The launch of a job range that passed render()'s checks: every decision between the arguments and the HIP calls.
inline LaunchPlan plan_launch(const LaunchInputs& in) {
  LaunchPlan p;
  const bool groups = launch_groups(in);
  p.ordered = launch_ordered(in);
  p.items = in.jid_count;
  if (in.pixel_mode) {  // work items are chunks of pixel_chunk pixels of one job
    const uint64_t area = in.tile_area;
    const uint64_t items = in.jid_count * area;
    // One work item per pixel makes every pixel a device-wide atomic on the launch's job counter, and a
    // wavefront's fetches then serialise there (C3: 530 M pixels, 546 ms vs 348 in the reference mode,
    // r03zf).  Pixels are taken pixel_chunk at a time: the largest power of two dividing the tile area that
    // still leaves >= 32 chunks per resident lane (C3 / C5: 32 pixels; C2, C1: 1 -- C2 ran 41.6 ms with 1
    // pixel per item, 43.7 with 4, r03zg), or the vpt_gpu_set_pixel_chunk value.  Every pixel keeps its own
    // stream: samples do not depend on it.
    uint64_t K = 1;
    if (in.pixel_chunk > 0) {
      K = (uint64_t)in.pixel_chunk;
    } else {
      const uint64_t lanes = (uint64_t)in.grid_blocks * kBlockThreads;
      while (area % (2 * K) == 0 && items / (2 * K) >= 32 * lanes) K *= 2;
    }
    p.pixel_chunk = (uint32_t)K;
    p.items = items / K;
  }
  // Partly filled launches (a few work items per resident lane: small frames, few waves, a GPU's share
  // of a frame dealt over several): a launch lasts as long as its slowest jobs, and a job's lane runs
  // faster with fewer waves per SIMD, so the grid is sized to round(1 + 1.8 x) blocks per CU (at most
  // the resident capacity), x = items per resident lane.  Same jobs, same samples.  Measured (r03h,
  // profiles/archive/r03h_grid_sweep.txt; C3 frames of spp waves, 4 / 5 / 6 / 7 blocks per CU, ms): spp 16
  // (x 1.1) 54.5 / 55.0 / 55.4 / 57.5 (3: 51.5); spp 24 (x 1.7) 57.3 / 61.0 / 64.7 / 65.7; spp 32
  // (x 2.3, the 8-GPU share) 70.4 / 66.9 / 67.5 / 71.2; spp 48 (x 3.4) 92.2 / 90.8 / 89.7 / 87.9; from
  // spp 96 on (and C5's shares) the full grid is best.  C2 (262 144 jobs, x 0.57 -> 2 blocks per CU,
  // r02g: 1 / 1.5 / 1.75 / 2 / 2.5 / 3 / 4 / 5 blocks per CU 167.7 / 124.4 / 112.9 / 98.7-99.3 / 104.4 /
  // 104.5-105.3 / 106.7 / 109.9 ms).  (r02's rule, ~2 items per lane, gave 7 blocks from x 1.9 on.)
  uint32_t blocks = (uint32_t)in.grid_blocks;
  // Latency-bound launch (at most kSpreadLanes items per wavefront of the grid, e.g. C1's 4 096 jobs):
  // the launch lasts as long as its slowest job, and a job runs fastest on a wavefront with few other
  // paths (the wavefront executes every block any of its lanes needs).  Such a launch keeps the whole
  // grid, the first ~items / wavefronts lanes of each wavefront take the jobs, and it runs with the
  // latency gates (every block runs for one lane).  Measured, C1 (r02): 43.3 ms (256 blocks x 64
  // lanes) -> 20.5 ms (1 792 blocks, one lane per wavefront, gates 1:65:1:1).  Same jobs, same samples.
  const bool latency = p.items <= kSpreadLanes * ((uint64_t)blocks * (kBlockThreads / 64));
  const uint64_t cus = (uint64_t)in.cus;
  if (!in.grid_user && !latency) {
    const uint64_t resident_per_cu = std::max<uint64_t>(1, blocks / cus);
    const double x = (double)p.items / ((double)blocks * kBlockThreads);  // items per resident lane
    const uint64_t per_cu = std::min<uint64_t>(resident_per_cu, (uint64_t)std::max(1.0, std::floor(1.5 + 1.8 * x)));
    blocks = (uint32_t)std::min<uint64_t>(blocks, cus * per_cu);
  }
#ifdef VPT_JOB_LOG
  const bool dbg = in.events;  // records = the job log
#else
  const bool dbg = in.records || in.events;
#endif
  // The latency kernel (lane cold state in VGPRs, VPT_WAVES_LAT waves per SIMD) for launches that fill at
  // most its resident grid anyway: latency-bound ones on its whole grid with the latency gates (C1 20.7-21.2
  // -> 19.2-19.7 ms, r04e / r04z), and partly filled ones whose rule above gives <= lat_per_cu blocks per CU
  // with the context's gates (C2 100.0-101.3 -> 95.7-96.6 ms, the 8-GPU C3 share of 32 waves 66.1-66.6 ->
  // 65.1-65.3; with the latency gates they ran slower, 108.3-109.8 / 75.2-76.1 ms: its one-lane blocks add
  // wave instructions to launches that are issue-bound; r04k, profiles/archive/r04k_lat_gated_ab.txt).  lat_mode 1
  // forces it.  Same jobs, same samples.
  const uint64_t lat_blocks = cus * (uint64_t)in.lat_per_cu;
  // (a launch with light groups or a shutter always takes the throughput kernel: samples do not depend on the kernel)
  const bool use_lat = !dbg && !in.feed && !groups && !in.shutter && in.lat_mode != 0 &&
                       (in.lat_mode == 1 || (!in.grid_user && (latency || blocks <= lat_blocks)));
  if (use_lat) blocks = (uint32_t)std::min<uint64_t>(latency ? lat_blocks : blocks, lat_blocks);
  // Live-path compaction (vpt_gpu_set_compaction): partly filled launches of the latency kernel whose grid fits
  // the compacting kernel's occupancy (its LDS exchange: 2 blocks per CU; C2 runs 2).
  const bool compact = use_lat && !latency && in.compact_every > 0 &&
                       (uint64_t)blocks <= cus * (uint64_t)std::max(0, in.compact_per_cu);
  const uint64_t T = in.T;
  // (a band launch takes the same-tile order restricted to the band, band_job, whatever the context's job order: the
  // sample layout is built on it)
  if (!in.band && !in.feed && in.order_mode != VPT_ORDER_JID && in.jid_begin % T == 0 && in.jid_count % T == 0 &&
      in.jid_count < (1ULL << 32)) {
    // whole waves: take the jobs in cost order (same jobs, same samples)
    const uint32_t n = (uint32_t)(in.jid_count / T);
    uint32_t tail = 0;  // VPT_ORDER_COST_WAVE_MAJOR
    // Same-tile order only where each sample has a slot of its own (the ordered film): with film atomics a
    // wavefront's 64 lanes would add to one pixel at once.  And not in partly filled launches (a few jobs per
    // lane, the latency kernel with the context's gates), which last as long as their costliest jobs: r06ze, C2
    // 98.1-98.5 vs 96.4-96.9 ms, C3's 8-GPU share (32 waves) 65.0-65.7 vs 62.6-63.6 with the cost tail.  Full
    // launches: C3 321.8-322.0 vs 334.3-334.5 ms, C4 71.0-71.2 vs 80.2-80.7 (profiles/r06ze_same_tile_ab.txt).
    const bool same_tile = in.order_mode == VPT_ORDER_COST_SAME_TILE && p.ordered && !in.frame_waves &&
                           !(use_lat && !latency);
    if (in.order_mode == VPT_ORDER_COST_TILE_MAJOR || same_tile) tail = n;
    if (same_tile) p.order_group = 1;
    if (in.order_mode == VPT_ORDER_COST_TAIL || (in.order_mode == VPT_ORDER_COST_SAME_TILE && !same_tile)) {
      // the last ~6 x (resident lanes / T) waves (C3: 61 of 256): measured best of 2x..16x
      const uint64_t lanes = (uint64_t)blocks * kBlockThreads;
      const uint64_t want = in.order_tail_waves > 0 ? (uint64_t)in.order_tail_waves : (6 * lanes + T - 1) / T;
      tail = (uint32_t)std::min<uint64_t>(n, want);
    }
    p.cost_order = true;
    p.order_tail_n = tail;
    p.order_tail_k0 = (n - tail) * (uint32_t)T;
  }
  // The kernel: a base kernel of the grids and the launch's axes.  Band instantiations follow the same rules as the
  // launches of whole frames; light groups and a shutter ride the throughput kernels, plain or band (never a debug
  // launch or a feed: render() refused those).
  p.variant = base_variant(in.has_temperature, in.use_runs);
  p.variant.debug = dbg;
  p.variant.lat = use_lat;
  p.variant.compact = compact;
  p.variant.feed = in.feed;
  p.variant.band = in.band;
  p.variant.groups = groups;
  p.variant.shutter = in.shutter;
  p.blocks = blocks;
  p.latency = latency;
  p.lds_bytes = compact ? kXchgBytes : 0;
  p.compact_every = use_lat ? (uint32_t)std::max(1, in.compact_every) : 0;
  // (a compacting launch reads the context's scene, whose wave_lanes is 64: a path moved into another thread's
  // slot must be able to fetch there -- with fewer fetching lanes per wavefront, live paths packed into the
  // first slots would leave the fetching slots to finished ones)
  p.gate_set = latency || (use_lat && in.lat_ungated && !compact) ? VPT_GATES_LATENCY : VPT_GATES_CONTEXT;
  // (production launches of the throughput kernel read the full-launch gates, vpt_gpu_set_full_tuning; a
  // latency-bound one on it keeps the latency copy: its wave_lanes)
  if (!use_lat && !in.feed && !dbg && p.gate_set == VPT_GATES_CONTEXT) p.gate_set = VPT_GATES_FULL;
  // no temperature grid: no emission.  The kernel leaves region 1 alone; the film pass adds its +0.0 samples.
  p.zero_region1 = groups && !in.has_temperature;
  return p;
}

}  // namespace vpt

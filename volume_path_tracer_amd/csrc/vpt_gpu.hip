// vpt_gpu.hip — the integrator context and the C ABI around the kernels (include/vpt_gpu.h): grid upload,
// scene constants, render() (its checks, the ordered film's sample buffer and film passes), counters and knobs.
// The launch choices of render() -- kernel variant, grid size, gate set, job order -- are plan_launch's, and the
// rule for which kernel variants exist is variant_valid's (both vpt_variant.h; DESIGN.md "Kernel variants and the
// launch plan"); integrate_kernel() here is the one table of instantiations.  The device code is vpt_kernels.h
// (included here, the one translation unit that launches it); the feeds' host protocol is vpt_feed.cpp; the state
// both share is vpt_ctx.h.
//
// Kernel shape: a persistent grid sized to the device's resident capacity.  Every lane runs the state machine
// of vpt_integrator.h; when its (tile, wave) job ends it takes the next job id from a device counter, so lanes
// are refilled until the job range is drained and every wave reaches ST_DONE.
#include <hip/hip_runtime.h>
#include <pthread.h>
#include <sched.h>
#include <unistd.h>

#include <algorithm>
#include <array>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <functional>
#include <memory>
#include <atomic>
#include <mutex>
#include <chrono>
#include <string>
#include <thread>
#include <utility>
#include <vector>

#include "vpt_ctx.h"
#include "vpt_kernels.h"
#include "vpt_denoise.h"
#include "vpt_temporal.h"

namespace vpt {

static thread_local std::string g_last_error;

int set_error(int code, const std::string& msg) {
  g_last_error = msg;
  return code;
}

}  // namespace vpt

using vpt::host::ctx_device;
using vpt::host::render;

namespace vpt {
static int upload(const void* src, size_t n, void** dst, size_t& bytes) {
  *dst = nullptr;
  if (n == 0) return VPT_OK;
  VPT_HIP(hipMalloc(dst, n));
  VPT_HIP(hipMemcpy(*dst, src, n, hipMemcpyHostToDevice));
  bytes += n;
  return VPT_OK;
}

static int upload_grid(const HostGrid& h, DeviceGrid& d) {
  d.dev = h.dev;
  int rc;
  // The stencil pool is 9 KiB per leaf (4.5x the voxels): a large sparse volume can exceed the
  // device's memory.  Say so before the first allocation instead of failing inside hipMalloc.
  const size_t need = h.cells8.size() * sizeof(int2) + h.runs8.size() + h.walk8.size() * sizeof(uint32_t) +
                      h.cells128.size() * sizeof(int2) + h.root.size() * sizeof(RootTileDev) +
                      h.bricks.size() * sizeof(float);
  size_t free_b = 0, total_b = 0;
  VPT_HIP(hipMemGetInfo(&free_b, &total_b));
  if (need > free_b)
    return set_error(VPT_E_NOMEM, "grid upload: needs " + std::to_string(need >> 20) + " MiB (" +
                                      std::to_string(h.dev.leaf_count) + " leaves x 9 KiB stencil pool + tables), " +
                                      std::to_string(free_b >> 20) + " MiB free on the device");
  if ((rc = upload(h.cells8.data(), h.cells8.size() * sizeof(int2), &d.cells8, d.bytes))) return rc;
  if ((rc = upload(h.runs8.data(), h.runs8.size(), &d.runs8, d.bytes))) return rc;
  if ((rc = upload(h.walk8.data(), h.walk8.size() * sizeof(uint32_t), &d.walk8, d.bytes))) return rc;
  d.run_fraction = h.run_fraction;
  if ((rc = upload(h.cells128.data(), h.cells128.size() * sizeof(int2), &d.cells128, d.bytes))) return rc;
  if ((rc = upload(h.root.data(), h.root.size() * sizeof(RootTileDev), &d.root, d.bytes))) return rc;
  if ((rc = upload(h.bricks.data(), h.bricks.size() * sizeof(float), &d.bricks, d.bytes))) return rc;
  d.dev.cells8 = (const int2*)d.cells8;
  d.dev.runs8 = (const uint8_t*)d.runs8;
  d.dev.walk8 = (const uint32_t*)d.walk8;
  d.dev.cells128 = (const int2*)d.cells128;
  d.dev.root = (const RootTileDev*)d.root;
  d.dev.bricks = (const float*)d.bricks;
  d.dev.dense = nullptr;
  d.brick_bytes = h.bricks.size() * sizeof(float);
  return VPT_OK;
}

static void free_grid(DeviceGrid& d) {
  (void)hipFree(d.cells8);
  (void)hipFree(d.runs8);
  (void)hipFree(d.walk8);
  (void)hipFree(d.cells128);
  (void)hipFree(d.root);
  (void)hipFree(d.bricks);
  (void)hipFree(d.dense);
  d = DeviceGrid{};
}

// The direct-addressed pool of an uploaded grid (vpt_gpu_set_pool_layout): table cells x 9216 bytes.
static uint64_t dense_pool_bytes(const DeviceGrid& d) {
  if (!d.cells8) return 0;
  return (uint64_t)d.dev.r8_n[0] * (uint64_t)d.dev.r8_n[1] * (uint64_t)d.dev.r8_n[2] * kBrickVox * sizeof(float);
}

static void free_dense(DeviceGrid& d) {
  (void)hipFree(d.dense);
  d.dense = nullptr;
  d.dense_bytes = 0;
  d.dev.dense = nullptr;
}

// Allocates d's dense pool and enqueues its expansion on the null stream.  VPT_E_NOMEM (nothing allocated) when the
// device has no room for it.
static int expand_dense(DeviceGrid& d) {
  const uint64_t bytes = dense_pool_bytes(d);
  if (bytes == 0) return VPT_OK;
  const hipError_t e = hipMalloc(&d.dense, bytes);
  if (e != hipSuccess) {
    d.dense = nullptr;
    (void)hipGetLastError();
    return set_error(VPT_E_NOMEM, "dense stencil pool: " + std::to_string(bytes >> 20) + " MiB: " + hipGetErrorString(e));
  }
  d.dense_bytes = bytes;
  const uint64_t cells = bytes / (kBrickVox * sizeof(float));
  DevGrid g = d.dev;
  g.dense = nullptr;
  hipLaunchKernelGGL(vpt_dense_expand_kernel, dim3((unsigned)std::min<uint64_t>(cells, 1u << 20)), dim3(256), 0, nullptr,
                     g, (float*)d.dense, cells);
  VPT_HIP(hipGetLastError());
  return VPT_OK;
}

}  // namespace vpt

namespace {

constexpr int kProfWords = 2 * vpt::PB_COUNT + vpt::PT_COUNT;
constexpr uint32_t kLaunchSlots = 64;

int wait_ctx(vpt_gpu_ctx* ctx);

// What every call that launches, or derives a scene, returns while the context has no volume (vpt_gpu_set_grids).
int volume_gone() {
  return vpt::set_error(VPT_E_STATE, "the context has no volume: a vpt_gpu_set_grids failed after the old volume was "
                                     "freed (a later vpt_gpu_set_grids that succeeds restores it)");
}

// The scene of `cfg` on the context's uploaded grids, with the context's overrides: the one derivation of creation
// (create_on), vpt_gpu_set_scene and vpt_gpu_set_grids.  From cfg: build_scene's constants; from the grids: their
// descriptors as uploaded (the stencil pool's layout included), scene_finalize's constants (the density map), and
// bb_lds_ok (the temperature grid's value extremes against cfg's scale and offset); from the context: the blackbody
// and CIE tables and, read from ctx->scene, what its setters own -- the gates (vpt_gpu_set_tuning), pixel_mode
// (vpt_gpu_set_rng_mode) and wave_lanes.  Writes S alone, so a failure leaves the context as it was.
int derive_scene(const vpt_gpu_ctx* ctx, const vpt_configuration& cfg, vpt::DevScene& S) {
  if (int rc = vpt::build_scene(cfg, S)) return rc;
  S.density = ctx->density.dev;
  vpt::scene_finalize(S);  // uses only the density map (host copy of the values)
  S.temperature = ctx->temperature.dev;
  S.has_temperature = ctx->has_temperature ? 1 : 0;
  S.bb_lds_ok = ctx->has_temperature ? vpt::blackbody_rows_suffice(ctx->temp_range, cfg.volume_parameters.temperature_scale,
                                                                   cfg.volume_parameters.temperature_offset, vpt::kBbLdsRows)
                                     : 0;
  S.bb = ctx->bb;
  S.cie = ctx->cie;
  S.gate_min = ctx->scene.gate_min;
  S.gate_idle = ctx->scene.gate_idle;
  S.gate_eval = ctx->scene.gate_eval;
  S.gate_walk = ctx->scene.gate_walk;
  S.pixel_mode = ctx->scene.pixel_mode;
  S.wave_lanes = ctx->scene.wave_lanes;
  S.tile_area = (uint32_t)(S.tw * S.th);
  return VPT_OK;
}

// The tile costs and everything ranked by them belong to the scene that was replaced: dropped, and recomputed by the
// next call that needs them (ensure_order).  The device buffers stay.  An explicit job permutation goes too.  The
// caller has waited for the context's launches.
void drop_order(vpt_gpu_ctx* ctx) {
  ctx->order_valid = false;
  ctx->tile_cost.clear();
  ctx->tile_rank.clear();
  ctx->band_rank_lo = ctx->band_rank_hi = 0;
  ctx->list_ranked = false;
  if (ctx->perm) {
    (void)hipFree(ctx->perm);
    ctx->perm = nullptr;
    ctx->perm_n = 0;
  }
}

// Device copy of the scene constants, which every in-flight launch of this context reads: wait for
// the context's launches (wait_ctx), copy on the context's stream and wait for the copy (the next
// render may use another stream).
int push_scene(vpt_gpu_ctx* ctx) {
  int rc = wait_ctx(ctx);
  if (rc) return rc;
  vpt::DevScene lat = ctx->scene;
  lat.gate_min = ctx->lat_gate[0];
  lat.gate_idle = ctx->lat_gate[1];
  lat.gate_eval = ctx->lat_gate[2];
  lat.gate_walk = ctx->lat_gate[3];
  lat.wave_lanes = ctx->lat_wave_lanes;
  VPT_HIP(hipMemcpyAsync(ctx->scene_dev, &ctx->scene, sizeof(vpt::DevScene), hipMemcpyHostToDevice, ctx->stream));
  VPT_HIP(hipMemcpyAsync(ctx->scene_lat_dev, &lat, sizeof(vpt::DevScene), hipMemcpyHostToDevice, ctx->stream));
  vpt::DevScene full = ctx->scene;
  full.gate_min = ctx->full_gate[0];
  full.gate_idle = ctx->full_gate[1];
  full.gate_eval = ctx->full_gate[2];
  full.gate_walk = ctx->full_gate[3];
  VPT_HIP(hipMemcpyAsync(ctx->scene_full_dev, &full, sizeof(vpt::DevScene), hipMemcpyHostToDevice, ctx->stream));
  VPT_HIP(hipStreamSynchronize(ctx->stream));
  return VPT_OK;
}

// The counter pair of the next launch on stream s: ordered after the previous launch that used the
// same ring slot (whatever stream it ran on), then zeroed on s.
int take_slot(vpt_gpu_ctx* ctx, hipStream_t s, uint32_t& slot) {
  std::lock_guard<std::mutex> lock(ctx->slot_mu);
  slot = ctx->next_slot;
  ctx->next_slot = (ctx->next_slot + 1) % kLaunchSlots;
  if (ctx->slot_used[slot]) VPT_HIP(hipStreamWaitEvent(s, ctx->slot_done[slot], 0));
  VPT_HIP(hipMemsetAsync(ctx->job_counter + 2 * slot, 0, 2 * sizeof(unsigned long long), s));
  return VPT_OK;
}

int release_slot(vpt_gpu_ctx* ctx, hipStream_t s, uint32_t slot) {
  std::lock_guard<std::mutex> lock(ctx->slot_mu);
  VPT_HIP(hipEventRecord(ctx->slot_done[slot], s));
  ctx->slot_used[slot] = true;
  return VPT_OK;
}

// Waits for every launch of this context, whatever stream it was enqueued on, and for the context's
// own stream -- not for other contexts' work on the device (a context per thread never stalls
// behind another's frames).  Each launch records its ring slot's event after its kernels
// (release_slot), and a launch that reuses a slot is ordered after the slot's previous launch
// (take_slot), so the latest event of every used slot covers all of them.
// The events are snapshotted under the lock and waited for after it is released, so a wait never
// blocks another thread's take_slot.
int wait_ctx(vpt_gpu_ctx* ctx) {
  if (ctx->open_feeds.load() > 0)
    return vpt::set_error(VPT_E_STATE, "a feed of this context is open: close it before calls that wait for the "
                                       "context's launches (ADVICE r04)");
  hipEvent_t ev[kLaunchSlots];
  uint32_t n = 0;
  {
    std::lock_guard<std::mutex> lock(ctx->slot_mu);
    for (uint32_t i = 0; i < kLaunchSlots; ++i)
      if (ctx->slot_used[i]) ev[n++] = ctx->slot_done[i];
  }
  for (uint32_t i = 0; i < n; ++i) VPT_HIP(hipEventSynchronize(ev[i]));
  if (ctx->stream) VPT_HIP(hipStreamSynchronize(ctx->stream));
  return VPT_OK;
}


void destroy(vpt_gpu_ctx* ctx) {
  if (!ctx) return;
  vpt::host::feed_pool_free(ctx);
  (void)hipSetDevice(ctx->device);
  vpt::free_grid(ctx->density);
  vpt::free_grid(ctx->temperature);
  (void)hipFree(ctx->bb);
  (void)hipFree(ctx->cie);
  (void)hipFree(ctx->film);
  (void)hipFree(ctx->job_counter);
  (void)hipFree(ctx->counters);
  (void)hipFree(ctx->prof);
  (void)hipFree(ctx->scene_dev);
  (void)hipFree(ctx->scene_lat_dev);
  (void)hipFree(ctx->scene_full_dev);
  (void)hipFree(ctx->order);
  (void)hipFree(ctx->cost_dev);
  (void)hipFree(ctx->band_rank);
  (void)hipFree(ctx->list_dev);
  (void)hipFree(ctx->list_slot_dev);
  (void)hipFree(ctx->tile_err);
  (void)hipFree(ctx->gang_scratch);
  (void)hipFree(ctx->gang_waves);
  (void)hipFree(ctx->denoise_scratch);
  (void)hipFree(ctx->perm);
  (void)hipFree(ctx->samples);
  (void)hipFree(ctx->frame_film);
  (void)hipFree(ctx->shutter_dev);
  if (ctx->samples_done) (void)hipEventDestroy(ctx->samples_done);
  if (ctx->denoise_done) (void)hipEventDestroy(ctx->denoise_done);
  for (uint32_t i = 0; i < kLaunchSlots; ++i)
    if (ctx->slot_done[i]) (void)hipEventDestroy(ctx->slot_done[i]);
  if (ctx->stream) (void)hipStreamDestroy(ctx->stream);
  if (ctx->staging) (void)hipHostFree(ctx->staging);
  delete ctx;
}

// The descending-cost tile ranks of ctx->tile_cost, uploaded as the job order.
int rank_tiles(vpt_gpu_ctx* ctx) {
  const uint64_t T = ctx->scene.T;
  ctx->tile_rank.resize(T);
  for (uint64_t i = 0; i < T; ++i) ctx->tile_rank[i] = (uint32_t)i;
  std::stable_sort(ctx->tile_rank.begin(), ctx->tile_rank.end(),
                   [&](uint32_t a, uint32_t b) { return ctx->tile_cost[a] > ctx->tile_cost[b]; });
  // The context's one buffer (T is fixed for its life), overwritten in place: every caller has waited for the
  // launches that read the previous ranks (wait_ctx), so a sequence of scene updates allocates nothing per frame.
  ctx->order_valid = false;
  if (!ctx->order) VPT_HIP(hipMalloc((void**)&ctx->order, T * sizeof(uint32_t)));
  const hipError_t e = hipMemcpy(ctx->order, ctx->tile_rank.data(), T * sizeof(uint32_t), hipMemcpyHostToDevice);
  if (e != hipSuccess) return vpt::set_error(VPT_E_HIP, std::string("tile order upload: ") + hipGetErrorString(e));
  ctx->order_valid = true;
  // (band launches' filtered ranks: the context's one buffer, so that no launch allocates)
  if (!ctx->band_rank) VPT_HIP(hipMalloc((void**)&ctx->band_rank, T * sizeof(uint32_t)));
  ctx->band_rank_lo = ctx->band_rank_hi = 0;
  // (tile-list launches' list and slot map, vpt_gpu_tile_errors' results: likewise)
  if (!ctx->list_dev) VPT_HIP(hipMalloc((void**)&ctx->list_dev, T * sizeof(uint32_t)));
  if (!ctx->list_slot_dev) VPT_HIP(hipMalloc((void**)&ctx->list_slot_dev, T * sizeof(uint32_t)));
  if (!ctx->tile_err) VPT_HIP(hipMalloc((void**)&ctx->tile_err, T * sizeof(float)));
  ctx->list_ranked = false;
  return VPT_OK;
}

// Tile costs (vpt_tile_cost_kernel) and the descending-cost tile ranks, once per scene: a context's first call that
// needs them, and the first one after a scene or volume update dropped them (drop_order).
int ensure_order(vpt_gpu_ctx* ctx) {
  if (ctx->order && ctx->order_valid) return VPT_OK;
  if (!ctx->volume_ok) return volume_gone();
  const auto t0 = std::chrono::steady_clock::now();
  struct Lap {  // (the cost pass's time, vpt_gpu_setup_timings)
    vpt_gpu_ctx* c;
    std::chrono::steady_clock::time_point t0;
    ~Lap() { c->setup_ms[3] += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); }
  } lap{ctx, t0};
  if (ctx->open_feeds.load() > 0)  // the cost pass and its copy would wait for the feed's launch
    return vpt::set_error(VPT_E_STATE, "tile costs: a feed of this context is open (compute them before)");
  const uint64_t T = ctx->scene.T;
  if (!ctx->cost_dev) VPT_HIP(hipMalloc((void**)&ctx->cost_dev, T * sizeof(float)));  // (kept: one pass per frame of a sequence)
  float* const cost = ctx->cost_dev;
  hipLaunchKernelGGL(vpt::vpt_tile_cost_kernel, dim3((unsigned)((T + 255) / 256)), dim3(256), 0, nullptr,
                     ctx->scene_dev, cost);
  ctx->tile_cost.assign(T, 0.0f);
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) e = hipMemcpy(ctx->tile_cost.data(), cost, T * sizeof(float), hipMemcpyDeviceToHost);
  if (e != hipSuccess) return vpt::set_error(VPT_E_HIP, std::string("tile cost pass: ") + hipGetErrorString(e));
  return rank_tiles(ctx);
}

// The ordered film's sample buffer for a launch of `bytes`: the context's, grown if needed.  nullptr (VPT_OK)
// when it must grow while a feed of the context is open -- freeing or allocating device memory could wait for
// the feed's launch -- and that launch then adds into the film with atomics.
int ensure_samples(vpt_gpu_ctx* ctx, uint64_t bytes, float*& out) {
  out = nullptr;
  if (ctx->samples_bytes >= bytes) {
    out = ctx->samples;
    return VPT_OK;
  }
  if (ctx->open_feeds.load() > 0) return VPT_OK;
  if (ctx->samples_used) VPT_HIP(hipEventSynchronize(ctx->samples_done));  // (ordered launches are serialised)
  if (ctx->samples) {
    (void)hipFree(ctx->samples);
    ctx->samples = nullptr;
    ctx->samples_bytes = 0;
  }
  const hipError_t e = hipMalloc((void**)&ctx->samples, bytes);
  if (e != hipSuccess) {
    ctx->samples = nullptr;
    (void)hipGetLastError();
    return vpt::set_error(VPT_E_NOMEM, "ordered film: " + std::to_string(bytes >> 20) + " MiB sample buffer: " +
                                           hipGetErrorString(e) + " (vpt_gpu_set_film_order's max_bytes splits launches)");
  }
  ctx->samples_bytes = bytes;
  out = ctx->samples;
  return VPT_OK;
}

// The largest sample buffer an ordered launch may use (bytes).
uint64_t ordered_cap(vpt_gpu_ctx* ctx, uint64_t want) {
  if (ctx->film_order_max) return ctx->film_order_max;
  if (want <= ctx->samples_bytes) return ctx->samples_bytes;
  size_t free_b = 0, total_b = 0;
  if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) return ctx->samples_bytes;
  return (uint64_t)(free_b + ctx->samples_bytes) / 4 * 3;
}

// The stencil pool's layout for `policy` (vpt_gpu_set_pool_layout), the context's launches waited for by the caller:
// builds or frees the dense pools of the context's grids and points the host copy of the scene at them (the caller
// pushes it).  VPT_POOL_AUTO never fails for want of memory: it stays sparse.
int apply_pool_layout(vpt_gpu_ctx* ctx, int policy) {
  vpt::DeviceGrid* grids[2] = {&ctx->density, ctx->temperature.cells8 || ctx->temperature.bricks ? &ctx->temperature : nullptr};
  uint64_t need = 0;
  for (vpt::DeviceGrid* d : grids)
    if (d) need += vpt::dense_pool_bytes(*d);
  bool dense = policy == VPT_POOL_DENSE && need > 0;
  if (policy == VPT_POOL_AUTO && need > 0) {
    uint64_t cap = ctx->pool_cap;
    if (cap == 0) {
      size_t free_b = 0, total_b = 0;
      VPT_HIP(hipMemGetInfo(&free_b, &total_b));
      cap = (uint64_t)total_b / 8;
    }
    dense = need <= cap;
  }
  const bool have = ctx->density.dense != nullptr;
  int rc = VPT_OK;
  if (dense && !have) {
    hipEvent_t ev[2] = {nullptr, nullptr};
    VPT_HIP(hipEventCreate(&ev[0]));
    VPT_HIP(hipEventCreate(&ev[1]));
    (void)hipEventRecord(ev[0], nullptr);
    for (vpt::DeviceGrid* d : grids)
      if (d && rc == VPT_OK) rc = vpt::expand_dense(*d);
    (void)hipEventRecord(ev[1], nullptr);
    const hipError_t e = hipEventSynchronize(ev[1]);
    if (rc == VPT_OK && e != hipSuccess) rc = vpt::set_error(VPT_E_HIP, std::string("dense stencil pool: ") + hipGetErrorString(e));
    if (rc == VPT_OK) (void)hipEventElapsedTime(&ctx->pool_expand_ms, ev[0], ev[1]);
    (void)hipEventDestroy(ev[0]);
    (void)hipEventDestroy(ev[1]);
    if (rc != VPT_OK) {
      dense = false;
      if (rc == VPT_E_NOMEM && policy == VPT_POOL_AUTO) rc = VPT_OK;  // (sparse, silently: vpt_gpu_pool_info tells)
    }
  }
  for (vpt::DeviceGrid* d : grids) {
    if (!d) continue;
    if (!dense) vpt::free_dense(*d);
    d->dev.dense = (const float*)d->dense;
  }
  ctx->scene.density.dense = ctx->density.dev.dense;
  ctx->scene.temperature.dense = ctx->temperature.dev.dense;
  return rc;
}

// A context's first layout: VPT_POOL_AUTO, or what the environment variable VPT_POOL_LAYOUT names.
int default_pool_policy() {
  const char* v = std::getenv("VPT_POOL_LAYOUT");
  if (v && !std::strcmp(v, "sparse")) return VPT_POOL_SPARSE;
  if (v && !std::strcmp(v, "dense")) return VPT_POOL_DENSE;
  return VPT_POOL_AUTO;
}

// The integrate kernel of a variant, or null where variant_valid says there is none: a table over the 1 024 flag
// combinations, built at compile time.  Entry i's template arguments and its validity test read the one decoded
// value, so an entry cannot name another variant's kernel, and the valid entries are the library's instantiations.
using IntegrateKernel = void (*)(vpt::KernelArgs, const vpt::DevScene*, unsigned long long*);
template <uint32_t I>
constexpr IntegrateKernel integrate_entry() {
  constexpr vpt::KernelVariant v = vpt::variant_decode(I);
  if constexpr (vpt::variant_valid(v))
    return &vpt::vpt_integrate_kernel<v.temp, v.debug, v.runs, v.lat, v.compact, v.feed, v.band, v.gang, v.groups, v.shutter>;
  else
    return nullptr;
}
template <uint32_t... I>
constexpr std::array<IntegrateKernel, sizeof...(I)> integrate_table(std::integer_sequence<uint32_t, I...>) {
  return {integrate_entry<I>()...};
}
IntegrateKernel integrate_kernel(const vpt::KernelVariant& v) {
  static constexpr auto table = integrate_table(std::make_integer_sequence<uint32_t, vpt::kVariantCount>());
  return table[vpt::variant_index(v)];
}
static_assert(vpt::kPlanOrderGroup == vpt::kOrderGroup, "the launch plan's default group is the integrator's");

// Launches the integrate kernel of `v`: the one place that records which gate set and evaluation the launch ran with
// (vpt_gpu_gate_info) and checks the launch.
int launch_integrate(vpt_gpu_ctx* ctx, const vpt::KernelVariant& v, uint32_t blocks, size_t shmem, hipStream_t s,
                     const vpt::KernelArgs& args, const vpt::DevScene* scene) {
  const IntegrateKernel kernel = integrate_kernel(v);
  if (!kernel) return vpt::set_error(VPT_E_INVALID, "launch: no integrate kernel of variant " + std::to_string(vpt::variant_index(v)));
  hipLaunchKernelGGL(kernel, dim3(blocks), dim3(vpt::kBlockThreads), shmem, s, args, scene, ctx->counters);
  ctx->last_gate_set = scene == ctx->scene_full_dev ? VPT_GATES_FULL
                       : scene == ctx->scene_lat_dev ? VPT_GATES_LATENCY : VPT_GATES_CONTEXT;  // (vpt_gpu_gate_info)
  // (the instantiation just launched splits the evaluation: a density-only production launch of a throughput kernel)
  ctx->last_eval_split = vpt::variant_eval_split(v) ? 1 : 0;
  VPT_HIP(hipGetLastError());
  return VPT_OK;
}

// What plan_launch reads of a render() call.
vpt::LaunchInputs launch_inputs(const vpt_gpu_ctx* ctx, uint64_t jid_begin, uint64_t jid_count, const float* records,
                                const vpt_event* events, const vpt::FeedLaunch* feed, const vpt::BandLaunch* band) {
  vpt::LaunchInputs in;
  in.jid_begin = jid_begin;
  in.jid_count = jid_count;
  in.T = ctx->scene.T;
  in.tile_area = ctx->scene.tile_area;
  in.grid_blocks = ctx->grid_blocks;
  in.grid_user = ctx->grid_user;
  in.cus = ctx->cus;
  in.lat_per_cu = ctx->lat_per_cu;
  in.lat_mode = ctx->lat_mode;
  in.lat_ungated = ctx->lat_ungated;
  in.compact_every = ctx->compact_every;
  in.compact_per_cu = ctx->compact_per_cu;
  in.has_temperature = ctx->scene.has_temperature != 0;
  in.use_runs = ctx->use_runs;
  in.pixel_mode = ctx->scene.pixel_mode != 0;
  in.pixel_chunk = ctx->pixel_chunk;
  in.order_mode = ctx->order_mode;
  in.order_tail_waves = ctx->order_tail_waves;
  in.film_order = ctx->film_order;
  in.frame_waves = ctx->frame_waves;
  in.records = records != nullptr;
  in.events = events != nullptr;
  in.feed = feed != nullptr;
  in.band = band != nullptr;
  in.groups = ctx->groups != nullptr;
  in.shutter = !ctx->shutter.empty();
  in.moments = ctx->m2 != nullptr;
  return in;
}

// What only an ordered launch with a sample buffer honours -- the moment plane, the light groups, the shutter, in the
// order they are reported -- and the two refusals each of them makes (vpt_variant.h attachments_refuse has the why).
struct Attachments {
  struct One {
    bool on;
    const char *subject, *cannot, *detach;
  } a[3];
  explicit Attachments(const vpt::LaunchInputs& in)
      : a{{in.moments && !in.feed, "a moment plane is", "would add with film atomics", "it (vpt_gpu_set_film_moments NULL)"},
          {vpt::launch_groups(in), "light groups are", "would add with film atomics", "them (vpt_gpu_set_light_groups NULL)"},
          {in.shutter, "a shutter is", "cannot honour it", "it (vpt_gpu_set_shutter NULL, 0)"}} {}
  const One* first() const {
    for (const One& x : a)
      if (x.on) return &x;
    return nullptr;
  }
  // The launch is no ordered one, or a frame is open.
  int refuse(const vpt::LaunchInputs& in) const {
    const One& x = *first();
    const char* const open_or_debug = in.frame_waves ? "a frame is open" : in.records || in.events ? "a debug launch" : nullptr;
    const char* const why = &x != &a[2]   ? (open_or_debug ? open_or_debug : "not an ordered launch of the reference RNG mode")
                            : in.feed     ? "a feed's launch"
                            : open_or_debug ? open_or_debug
                            : in.pixel_mode ? "the pixel RNG mode"
                                            : "VPT_FILM_ATOMIC";
    return vpt::set_error(VPT_E_STATE, std::string("render: ") + x.subject + " attached and this launch " + x.cannot + " (" +
                                           why + "): detach " + x.detach);
  }
  // The launch got no sample buffer.
  int refuse_grow() const {
    return vpt::set_error(VPT_E_STATE, std::string("render: ") + first()->subject +
                                           " attached and the sample buffer would have to grow while a feed of the context "
                                           "is open (the launch would add with film atomics)");
  }
};

// A band launch's tile ranks and its arguments.  The whole frame's ranks are the job order itself; another band's are
// filtered from it on the launch's stream -- after the wait for the sample buffer's previous launch, so after the previous
// band launch has read the buffer -- unless the buffer still holds this band's.
int band_ranks(vpt_gpu_ctx* ctx, const vpt::BandLaunch& band, hipStream_t s, vpt::KernelArgs& env) {
  const uint64_t T = ctx->scene.T;
  env.band_rank = ctx->order;
  env.band_slot_map = nullptr;
  if (band.list) {
    // a tile list (uploaded by vpt_gpu_render_tile_list): its ranks are filtered by the slot map, once per list
    if (!ctx->band_rank || !ctx->list_dev || !ctx->list_slot_dev)
      return vpt::set_error(VPT_E_NOMEM, "vpt_gpu_render_tile_list: no tile-list buffers (their allocation failed)");
    if (!ctx->list_ranked) {
      hipLaunchKernelGGL(vpt::vpt_band_rank_kernel, dim3(1), dim3(256), 0, s, ctx->order, (uint32_t)T, 0u, band.tiles,
                         ctx->band_rank, ctx->list_slot_dev);
      VPT_HIP(hipGetLastError());
      ctx->band_rank_lo = ctx->band_rank_hi = 0;  // (no longer a band's)
      ctx->list_ranked = true;
    }
    env.band_rank = ctx->band_rank;
    env.band_slot_map = ctx->list_slot_dev;
  } else if (band.tile_lo != 0 || band.tiles != T) {
    if (!ctx->band_rank) return vpt::set_error(VPT_E_NOMEM, "vpt_gpu_render_tiles: no tile-rank buffer (its allocation failed)");
    if (ctx->band_rank_lo != band.tile_lo || ctx->band_rank_hi != band.tile_lo + band.tiles) {
      hipLaunchKernelGGL(vpt::vpt_band_rank_kernel, dim3(1), dim3(256), 0, s, ctx->order, (uint32_t)T, band.tile_lo,
                         band.tile_lo + band.tiles, ctx->band_rank, (const uint32_t*)nullptr);
      VPT_HIP(hipGetLastError());
      ctx->band_rank_lo = band.tile_lo;
      ctx->band_rank_hi = band.tile_lo + band.tiles;
      ctx->list_ranked = false;
    }
    env.band_rank = ctx->band_rank;
  }
  env.band_waves = band.waves;
  env.band_T = (uint32_t)T;
  env.band_tile_lo = band.tile_lo;
  env.band_groups = vpt::band_groups(band.waves, band.group);
  env.band_group = band.group;
  return VPT_OK;
}

// The ordered film's passes over a launch's sample buffer: the film -- a band's pixels, or the frame's pixel by pixel --
// in wave order (sample counts and the moment plane included), then with light groups the same pass over each group's
// region into its plane (w += 1, xyz += imaging_ratio * Lg, in wave order).
int film_passes(vpt_gpu_ctx* ctx, const vpt::KernelArgs& env, const vpt::BandLaunch* band, bool groups, uint64_t jid_begin,
                uint64_t jid_count, hipStream_t s) {
  auto pass = [&](float* film, const float* samples, float* m2) {
    if (band) {
      const uint32_t chunks = (ctx->scene.tile_area + 63u) / 64u;
      const uint32_t* const list = band->list ? ctx->list_dev : nullptr;
      hipLaunchKernelGGL(m2 ? vpt::vpt_band_order_kernel<true> : vpt::vpt_band_order_kernel<false>,
                         dim3(band->tiles * chunks), dim3(64), 0, s, ctx->scene_dev, film, samples, band->tile_lo,
                         band->waves, env.band_groups, band->group, list, m2);
    } else {
      const uint64_t threads = ctx->scene.T * (uint64_t)ctx->scene.tile_area;
      hipLaunchKernelGGL(m2 ? vpt::vpt_film_order_kernel<true> : vpt::vpt_film_order_kernel<false>,
                         dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, s, ctx->scene_dev, film, samples, jid_begin,
                         jid_count, m2);
    }
    return hipGetLastError();
  };
  const uint64_t npix = (uint64_t)ctx->scene.W * (uint64_t)ctx->scene.H;
  VPT_HIP(pass(env.film, env.samples, ctx->m2));
  for (uint64_t g = 0; groups && g < 3; ++g)
    VPT_HIP(pass(ctx->groups + g * npix * 4, env.samples + (g + 1) * env.group_stride, nullptr));
  VPT_HIP(hipEventRecord(ctx->samples_done, s));
  ctx->samples_used = true;
  return VPT_OK;
}

}  // namespace

int vpt::host::ctx_device(vpt_gpu_ctx* ctx) {
  hipError_t e = hipSetDevice(ctx->device);
  if (e != hipSuccess) return vpt::set_error(VPT_E_HIP, std::string("hipSetDevice: ") + hipGetErrorString(e));
  return VPT_OK;
}

int vpt::host::launch_tile_counts(vpt_gpu_ctx* ctx, float* film, const uint32_t* counts_dev, hipStream_t s) {
  const uint64_t npix = (uint64_t)ctx->scene.W * (uint64_t)ctx->scene.H;
  hipLaunchKernelGGL(vpt::vpt_tile_count_kernel, dim3((unsigned)((npix + 255) / 256)), dim3(256), 0, s, ctx->scene_dev,
                     film, counts_dev);
  VPT_HIP(hipGetLastError());
  return VPT_OK;
}

int vpt::host::render(vpt_gpu_ctx* ctx, uint64_t jid_begin, uint64_t jid_count, float* film, float* records,
                      void* stream_ptr, vpt_event* events, uint64_t event_cap, uint32_t* slot_out,
                      const vpt::FeedLaunch* feed, const vpt::BandLaunch* band) {
  // 1. the arguments and the attachments
  if (!ctx) return vpt::set_error(VPT_E_INVALID, "render: null context");
  int rc = ctx_device(ctx);
  if (rc) return rc;
  if (jid_count == 0) return VPT_OK;
  if (!ctx->volume_ok) return volume_gone();
  if (feed && (ctx->scene.pixel_mode || records || events))
    return vpt::set_error(VPT_E_INVALID, "render: feeds run the reference RNG mode's production kernels only");
  if (band && (feed || records || events || ctx->scene.pixel_mode || ctx->film_order != VPT_FILM_ORDERED || ctx->frame_waves))
    return vpt::set_error(VPT_E_INVALID, "render: band launches are ordered production launches of the reference RNG mode");
  const vpt::LaunchInputs in = launch_inputs(ctx, jid_begin, jid_count, records, events, feed, band);
  const Attachments attached(in);
  if (vpt::attachments_refuse(in)) return attached.refuse(in);
  // 2. The ordered film: production launches of the reference RNG mode (debug launches and feeds add atomically).
  // A launch whose sample buffer would exceed the cap is rendered as consecutive launches (whole waves where it
  // can); each adds its own waves in order, so the film is the same.
  // Light groups (vpt_gpu_set_light_groups): four regions of the sample layout instead of one (kGroupRegions).
  const bool groups = vpt::launch_groups(in);
  const uint64_t per_job = (uint64_t)ctx->scene.tile_area * 3 * sizeof(float) * (groups ? vpt::kGroupRegions : 1);
  const uint64_t T = ctx->scene.T;
  if (vpt::launch_ordered(in) && !band) {  // (vpt_gpu_render_tiles splits its launches itself: by waves)
    const uint64_t max_jobs = std::min<uint64_t>(ordered_cap(ctx, jid_count * per_job) / per_job, 0xffffffffULL);
    if (max_jobs == 0) return vpt::set_error(VPT_E_NOMEM, "ordered film: no room for one job's samples");
    if (jid_count > max_jobs) {
      const uint64_t chunk = max_jobs >= T ? max_jobs / T * T : max_jobs;
      for (uint64_t b = 0; b < jid_count; b += chunk)
        if ((rc = render(ctx, jid_begin + b, std::min(chunk, jid_count - b), film, nullptr, stream_ptr))) return rc;
      return VPT_OK;
    }
  }
  if (in.pixel_mode && jid_count > UINT64_MAX / in.tile_area) return vpt::set_error(VPT_E_INVALID, "render: job range too large");
  // 3. the launch's decisions (vpt_variant.h)
  const vpt::LaunchPlan plan = vpt::plan_launch(in);
  // 4. the buffers and the kernel's arguments
  hipStream_t s = (hipStream_t)stream_ptr;  // NULL = the null stream (HIP convention)
  vpt::KernelArgs env{};
  env.jid_begin = jid_begin;
  env.jid_count = plan.items;
  env.pixel_chunk = plan.pixel_chunk;
  env.film = film ? film : ctx->film;
  env.records = records;
  env.tile_area = ctx->scene.tw * ctx->scene.th;
  env.prof_buf = ctx->prof;
  if ((band || plan.cost_order) && (rc = ensure_order(ctx))) return rc;  // (a band's sample layout is built on the ranks)
  env.order = plan.cost_order ? ctx->order : nullptr;
  env.order_tail_k0 = plan.order_tail_k0;
  env.order_tail_n = plan.order_tail_n;
  env.order_group = plan.order_group;
  env.perm = !feed && !band && ctx->perm && ctx->perm_n == jid_count && !ctx->scene.pixel_mode ? ctx->perm : nullptr;
  float* samples = nullptr;
  // (while the drop-in's ordered frame is open its feeds own the sample buffer: other launches add with atomics)
  if (band) {
    const uint64_t bytes = vpt::band_sample_floats(band->tiles, band->waves, ctx->scene.tile_area, band->group) * sizeof(float) *
                           (groups ? vpt::kGroupRegions : 1);
    if ((rc = ensure_samples(ctx, bytes, samples))) return rc;
    if (!samples)
      return vpt::set_error(VPT_E_STATE, "vpt_gpu_render_tiles: the sample buffer would have to grow (" +
                                             std::to_string(bytes >> 20) + " MiB) while a feed of the context is open");
  } else if (plan.ordered && !ctx->frame_waves && (rc = ensure_samples(ctx, jid_count * per_job, samples))) {
    return rc;
  }
  if (!samples && attached.first()) return attached.refuse_grow();
  env.shutter = ctx->shutter_dev;
  env.shutter_n = (uint32_t)ctx->shutter.size();
  env.samples = samples;
  env.group_stride = band ? vpt::band_sample_floats(band->tiles, band->waves, ctx->scene.tile_area, band->group)
                          : jid_count * (uint64_t)ctx->scene.tile_area * 3;
  if (samples) {
    ++ctx->ordered_launches;
    if (ctx->samples_used) VPT_HIP(hipStreamWaitEvent(s, ctx->samples_done, 0));  // the buffer's previous launch
  } else if (!feed) {
    ++ctx->atomic_launches;
  }
  if (band && (rc = band_ranks(ctx, *band, s, env))) return rc;
  uint32_t slot = 0;
  if ((rc = take_slot(ctx, s, slot))) return rc;
  env.job_counter = ctx->job_counter + 2 * slot;
  env.events = events;
  env.feed_word = feed ? feed->word : nullptr;
  env.feed_ring = feed ? feed->ring : nullptr;
  env.feed_mask = feed ? feed->mask : 0;
  env.feed_error = feed ? feed->error : nullptr;
  env.feed_started = feed ? feed->started : nullptr;
  env.feed_waiting = feed ? feed->waiting : nullptr;
  env.feed_hint_mask = (uint32_t)(vpt::kHintSlots - 1);
  env.tile_done = feed ? feed->tile_done : nullptr;
  env.frame = feed && ctx->frame_waves ? ctx->samples : nullptr;  // (the drop-in's ordered frame, vpt_gpu_frame_open)
  env.frame_w0 = ctx->frame_jid_lo / ctx->scene.T;
  env.frame_slots = env.frame ? ctx->frame_waves * ctx->frame_tiles : 0;
  env.frame_tile_lo = ctx->frame_tile_lo;
  env.frame_tiles = ctx->frame_tiles;
  env.compact_every = plan.compact_every;
  env.event_count = ctx->job_counter + 2 * slot + 1;
  env.event_cap = event_cap;
  if (slot_out) *slot_out = slot;
  // 5. the launch and the film passes
  if (plan.zero_region1) VPT_HIP(hipMemsetAsync(samples + env.group_stride, 0, env.group_stride * sizeof(float), s));
  const vpt::DevScene* const scene = plan.gate_set == VPT_GATES_FULL      ? ctx->scene_full_dev
                                     : plan.gate_set == VPT_GATES_LATENCY ? ctx->scene_lat_dev
                                                                          : ctx->scene_dev;
  if ((rc = launch_integrate(ctx, plan.variant, plan.blocks, plan.lds_bytes, s, env, scene))) return rc;
  if (samples) {
    if ((rc = film_passes(ctx, env, band, groups, jid_begin, jid_count, s))) return rc;
  } else if (!feed) {  // a feed adds its sample counts when it is closed (vpt_tile_count_kernel)
    const uint64_t npix = (uint64_t)ctx->scene.W * (uint64_t)ctx->scene.H;
    hipLaunchKernelGGL(vpt::vpt_count_kernel, dim3((unsigned)((npix + 255) / 256)), dim3(256), 0, s, ctx->scene_dev,
                       env.film, jid_begin, jid_count);
    VPT_HIP(hipGetLastError());
  }
  return release_slot(ctx, s, slot);
}

extern "C" {

const char* vpt_last_error(void) { return vpt::g_last_error.c_str(); }
int vpt_abi_version(void) { return VPT_ABI_VERSION; }

int vpt_gpu_device_count(int* count) {
  if (!count) return vpt::set_error(VPT_E_INVALID, "vpt_gpu_device_count: null argument");
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) n = 0;
  *count = n;
  return VPT_OK;
}

int vpt_gpu_find_seeds(int device, uint32_t out0, uint32_t out1, uint32_t* seeds, int max_seeds, int* n_found) {
  if (!n_found || max_seeds < 0 || (max_seeds > 0 && !seeds))
    return vpt::set_error(VPT_E_INVALID, "vpt_gpu_find_seeds: bad argument");
  *n_found = 0;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
    return vpt::set_error(VPT_E_HIP, "vpt_gpu_find_seeds: no HIP device");
  if (device < 0 || device >= ndev) return vpt::set_error(VPT_E_INVALID, "vpt_gpu_find_seeds: bad device index");
  VPT_HIP(hipSetDevice(device));
  constexpr uint32_t kCap = 64, kPerThread = 1024, kThreads = 256;
  hipStream_t s = nullptr;
  VPT_HIP(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
  uint32_t* d = nullptr;
  uint32_t host[kCap + 1] = {};
  hipError_t e = hipMalloc((void**)&d, (kCap + 1) * sizeof(uint32_t));
  if (e == hipSuccess) e = hipMemsetAsync(d, 0, (kCap + 1) * sizeof(uint32_t), s);
  if (e == hipSuccess) {
    const uint64_t blocks = ((1ULL << 32) / kPerThread + kThreads - 1) / kThreads;
    hipLaunchKernelGGL(vpt::vpt_seed_search_kernel, dim3((unsigned)blocks), dim3(kThreads), 0, s, out0, out1, kPerThread,
                       d + 1, d, kCap);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpyAsync(host, d, sizeof host, hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  (void)hipFree(d);
  (void)hipStreamDestroy(s);
  if (e != hipSuccess) return vpt::set_error(VPT_E_HIP, std::string("vpt_gpu_find_seeds: ") + hipGetErrorString(e));
  const uint32_t n = std::min(host[0], kCap);
  std::sort(host + 1, host + 1 + n);
  for (uint32_t i = 0; i < n && (int)i < max_seeds; ++i) seeds[i] = host[1 + i];
  *n_found = (int)host[0];
  return VPT_OK;
}

}  // extern "C"

// The host side of Volume::Volume: the grids flattened (leaf-slot and walk tables, the stencil pool) with the
// density's majorants fixed for interpolation (volume.cpp:162-170; temperature is only sampled) -- the ABI's
// vpt_host_grids (vpt_grids_flatten), uploaded by create_on.
struct vpt_host_grids {
  vpt::HostGrid density, temperature;
  bool has_temperature = false;
  vpt::ValueRange temp_range;  // the temperature grid's value extremes (blackbody_rows_suffice)
  double flatten_ms = 0;
};

namespace {
using HostGrids = vpt_host_grids;
// ms[0] += the time taken.
int build_grids(const vpt_grid_desc* density, const vpt_grid_desc* temperature, HostGrids& g, double* ms) {
  const auto t0 = std::chrono::steady_clock::now();
  // The temperature grid is flattened on a thread of its own beside the density's: each build has serial
  // stretches (node sets, leaf loops) and page-faults its fresh tables in (vpt_last_error is per thread: the
  // temperature's message is carried back).
  int trc = VPT_OK;
  std::string tmsg;
  std::thread temp_build;
  if (temperature)
    temp_build = std::thread([&] {
      if ((trc = vpt::build_host_grid(*temperature, false, 0, g.temperature)))
        tmsg = vpt_last_error();
      else
        g.temp_range = vpt::value_range(*temperature, 0);
    });
  int rc = vpt::build_host_grid(*density, true, 0, g.density);
  if (rc == VPT_OK) vpt::compute_runs(g.density, 0);
  if (temp_build.joinable()) temp_build.join();
  if (rc) return rc;
  if (trc) return vpt::set_error(trc, tmsg);
  g.has_temperature = temperature != nullptr;
  if (ms) *ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  return VPT_OK;
}

// The run-skipping variant as the context's grids choose it (vpt_gpu_set_run_skipping's -1).
bool auto_run_skipping(const vpt_gpu_ctx* ctx) {
  return !ctx->has_temperature && ctx->density.run_fraction >= VPT_RUNS_MIN_FRACTION;
}

// Persistent grid: as many blocks as are resident at once, of the production kernel the grids choose (runs: the
// run-skipping variant); the latency and the compacting kernel's resident blocks per CU.  A grid set by
// vpt_gpu_set_tuning stays.
int size_grid(vpt_gpu_ctx* ctx, bool runs) {
  const bool has_temperature = ctx->has_temperature;
  int per_cu = 0, cus = 0;
  // sized for the production kernel of this scene; the debug variant is launched with the same grid
  vpt::KernelVariant v = vpt::base_variant(has_temperature, runs);
  VPT_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, integrate_kernel(v), vpt::kBlockThreads, 0));
  VPT_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, ctx->device));
  if (per_cu < 1) per_cu = 1;
  if (!ctx->grid_user) ctx->grid_blocks = per_cu * cus;
  int lat_per_cu = 0;
  v.lat = true;
  VPT_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&lat_per_cu, integrate_kernel(v), vpt::kBlockThreads, 0));
  ctx->lat_per_cu = std::max(1, std::min(lat_per_cu, per_cu));
  int compact_per_cu = 0;
  v.compact = true;
  VPT_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&compact_per_cu, integrate_kernel(v), vpt::kBlockThreads, vpt::kXchgBytes));
  ctx->compact_per_cu = compact_per_cu;
  ctx->cus = cus > 0 ? cus : 1;
  return VPT_OK;
}

// A context on `device` from grids already flattened (vpt_gpu_create, vpt_gpu_create_many).
int create_on(const vpt_configuration* cfg, const HostGrids& grids, const float* blackbody_500x3, int device,
              vpt_gpu_ctx** out) {
  *out = nullptr;
  std::unique_ptr<vpt_gpu_ctx, void (*)(vpt_gpu_ctx*)> ctx(new vpt_gpu_ctx(), destroy);
  ctx->device = device;
  ctx->cfg = *cfg;
  ctx->setup_ms[0] = grids.flatten_ms;
  using clk = std::chrono::steady_clock;
  auto t = clk::now();
  auto lap = [&](int i) {  // setup phases (vpt_gpu_setup_timings)
    const auto now = clk::now();
    ctx->setup_ms[i] += std::chrono::duration<double, std::milli>(now - t).count();
    t = now;
  };
  int rc = ctx_device(ctx.get());
  if (rc) return rc;
  lap(4);
  {  // (the configuration is checked before anything is uploaded)
    vpt::DevScene probe;
    if ((rc = vpt::build_scene(*cfg, probe))) return rc;
  }
  if ((rc = vpt::upload_grid(grids.density, ctx->density))) return rc;
  if (grids.has_temperature && (rc = vpt::upload_grid(grids.temperature, ctx->temperature))) return rc;
  lap(1);
  const bool has_temperature = grids.has_temperature;
  ctx->has_temperature = has_temperature;
  ctx->temp_range = grids.temp_range;
  // The run-skipping kernel variant is for grids with large equal-majorant regions (C2's constant
  // cube: 36 % of the interior cells have run radius >= 2; the 512^3 cloud: 4 %, where the variant
  // would cost more than it skips).  vpt_gpu_set_run_skipping overrides the choice.
  ctx->use_runs = auto_run_skipping(ctx.get());
  // The direct-addressed stencil pool, expanded on the device from the tables just uploaded (part of the upload's
  // lap; its kernels' own time: vpt_gpu_pool_info).
  ctx->pool_policy = default_pool_policy();
  if ((rc = apply_pool_layout(ctx.get(), ctx->pool_policy))) return rc;
  lap(1);

  std::vector<float> bb(501 * 3, 0.0f);  // row 500 = 0 (reference reads past its table)
  if (blackbody_500x3)
    std::memcpy(bb.data(), blackbody_500x3, 500 * 3 * sizeof(float));
  else
    vpt::blackbody_table(bb.data());
  size_t scratch = 0;
  if ((rc = vpt::upload(bb.data(), bb.size() * sizeof(float), (void**)&ctx->bb, scratch))) return rc;
  if ((rc = vpt::upload(vpt::cie_table(), 471 * 3 * sizeof(float), (void**)&ctx->cie, scratch))) return rc;

  ctx->film_count = (uint64_t)cfg->output_size[0] * (uint64_t)cfg->output_size[1] * 4;
  VPT_HIP(hipMalloc((void**)&ctx->film, ctx->film_count * sizeof(float)));
  VPT_HIP(hipMemset(ctx->film, 0, ctx->film_count * sizeof(float)));
  VPT_HIP(hipMalloc((void**)&ctx->job_counter, kLaunchSlots * 2 * sizeof(unsigned long long)));  // jobs, events
  for (uint32_t i = 0; i < kLaunchSlots; ++i)
    VPT_HIP(hipEventCreateWithFlags(&ctx->slot_done[i], hipEventDisableTiming));
  VPT_HIP(hipMalloc((void**)&ctx->counters, vpt::kCounterCount * sizeof(unsigned long long)));
  VPT_HIP(hipMemset(ctx->counters, 0, vpt::kCounterCount * sizeof(unsigned long long)));
  VPT_HIP(hipMalloc((void**)&ctx->prof, kProfWords * sizeof(unsigned long long)));
  VPT_HIP(hipMemset(ctx->prof, 0, kProfWords * sizeof(unsigned long long)));
  VPT_HIP(hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking));
  VPT_HIP(hipEventCreateWithFlags(&ctx->samples_done, hipEventDisableTiming));

  if ((rc = size_grid(ctx.get(), ctx->use_runs))) return rc;
  // Scheduling defaults from tools/tune.py sweeps on MI355X (C3, 256 spp): rare states run for >= 6
  // waiting lanes, density evaluations (with the deferred exact draw) for >= 36, everything runs when
  // < 8 lanes are walking; the walk loops while >= 4 lanes walk (r02 sweep: 6:8:36:4 363.7 ms vs
  // 6:12:32:4 366.6 ms, C4 103.7 vs 104.4).  The temperature kernel's rare blocks wait for 8 lanes since the film
  // regroup (C4 83.3-83.6 vs 83.9-84.3 ms over 4 alternating runs, profiles/archive/r05gates2_c4_gate_min.txt).
  ctx->scene.gate_min = has_temperature ? 8 : 6;
  // The temperature kernel runs its rare blocks at any count only once no lane walks (same-tile order; C4 at
  // gate_idle 8 / 4 / 2 / 1: 67.2-67.4 / 64.2-64.3 / 62.8 / 61.5 ms, profiles/r06zj_c4_gates.txt,
  // r06zk_gates_idle.txt).  The density kernel's partly filled launches -- C2, a GPU's share -- were tuned at 8
  // and keep it; its full launches read a gate set of their own (full_gate, below).
  ctx->scene.gate_idle = has_temperature ? 1 : 8;
  ctx->scene.gate_eval = 36;
  // The temperature kernel's walk loops while any lane walks (gate_walk 1) since the same-tile order: C4 67.3-67.8
  // ms vs 71.1-71.3 at 4, best of 3 twice (r06zg, profiles/r06zg_gates_same_tile.txt); C3 stays at 4 (1-3: flat).
  ctx->scene.gate_walk = has_temperature ? 1 : 4;
  ctx->scene.pixel_mode = 0;
  ctx->scene.wave_lanes = 64;
  {  // (the defaults above are the context's overrides, which the derivation carries over)
    vpt::DevScene S;
    if ((rc = derive_scene(ctx.get(), *cfg, S))) return rc;
    ctx->scene = S;
  }
  VPT_HIP(hipMalloc((void**)&ctx->scene_dev, sizeof(vpt::DevScene)));
  VPT_HIP(hipMalloc((void**)&ctx->scene_lat_dev, sizeof(vpt::DevScene)));
  VPT_HIP(hipMalloc((void**)&ctx->scene_full_dev, sizeof(vpt::DevScene)));
  // Full launches' gates (vpt_gpu_set_full_tuning): the context's, and for the density kernel gate_idle
  // VPT_DEFAULT_FULL_GATE_IDLE (DESIGN.md section 4 has the sweep).
  ctx->full_gate[0] = ctx->scene.gate_min;
  ctx->full_gate[1] = has_temperature ? ctx->scene.gate_idle : VPT_DEFAULT_FULL_GATE_IDLE;
  ctx->full_gate[2] = ctx->scene.gate_eval;
  ctx->full_gate[3] = ctx->scene.gate_walk;
  if ((rc = push_scene(ctx.get()))) return rc;
  lap(2);
  *out = ctx.release();
  return VPT_OK;
}

int check_device(int device, const char* what) {
  int ndev = 0;
  hipError_t e = hipGetDeviceCount(&ndev);
  if (e != hipSuccess || ndev <= 0)
    return vpt::set_error(VPT_E_HIP, std::string(what) + ": no HIP device (the integrator has no CPU fallback)");
  if (device < 0 || device >= ndev) return vpt::set_error(VPT_E_INVALID, std::string(what) + ": bad device index");
  return VPT_OK;
}

// The launches of vpt_gpu_render_tiles and vpt_gpu_render_tile_list (list: the context's uploaded list, B tiles;
// tile_lo 0), arguments checked: `wave_count` > 0 waves from wave_begin of the band's B tiles.
// The cap (vpt_gpu_set_film_order's max_bytes, else what the device has free): consecutive blocks of waves, each
// with its own film pass, in wave order -- the same film.  Whole groups of 64 waves where the cap allows; below
// that a block's group is as wide as the block, so its buffer is no larger than its waves' samples.
int render_band_waves(vpt_gpu_ctx* ctx, uint32_t tile_lo, uint32_t B, bool list, uint64_t wave_begin, uint64_t wave_count,
                      float* film_device, void* hip_stream) {
  const uint64_t T = ctx->scene.T, G = vpt::kBandGroup;
  const uint64_t per_wave = (uint64_t)B * (uint64_t)ctx->scene.tile_area * 3 * sizeof(float) *
                            (ctx->groups ? vpt::kGroupRegions : 1);
  const uint64_t max_waves = ordered_cap(ctx, (wave_count + G - 1) / G * G * per_wave) / per_wave;
  if (max_waves == 0) return vpt::set_error(VPT_E_NOMEM, "ordered film: no room for one wave of the band's samples");
  const uint64_t chunk = max_waves >= G ? max_waves / G * G : max_waves;
  for (uint64_t b = 0; b < wave_count; b += chunk) {
    const uint64_t n = std::min(chunk, wave_count - b);
    const vpt::BandLaunch band{tile_lo, B, (uint32_t)n, (uint32_t)(max_waves >= G ? G : n), list};
    if (int rc = render(ctx, (wave_begin + b) * T, (uint64_t)B * n, film_device, nullptr, hip_stream, nullptr, 0, nullptr,
                        nullptr, &band))
      return rc;
  }
  return VPT_OK;
}

// vpt_gpu_denoise: byte ranges that share an address; one iteration's launch.
bool ranges_overlap(const void* a, size_t an, const void* b, size_t bn) {
  const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
  return a && b && a0 < b0 + bn && b0 < a0 + an;
}

template <int G>
void launch_denoise_atrous(bool last, dim3 grid, dim3 block, hipStream_t s, const vpt::DenoiseArgs& A, int32_t step,
                           const float4* src, const float4* gd, float4* dst, const float4* film, float4* out_film,
                           float* var_out) {
  if (last)
    hipLaunchKernelGGL((vpt::vpt_denoise_atrous_kernel<G, true>), grid, block, 0, s, A, step, src, gd, dst, film, out_film,
                       var_out);
  else
    hipLaunchKernelGGL((vpt::vpt_denoise_atrous_kernel<G, false>), grid, block, 0, s, A, step, src, gd, dst, film, out_film,
                       var_out);
}

// The matte passes' launch (vpt_gpu_render_alpha, vpt_gpu_render_depth), after the entry `fn` has checked its own
// arguments: the context's state, the tile ranks, a launch slot, and launch(blocks, stream) -- one wavefront per
// (tile slot, chunk of 64 pixels).  `noun` is what a shutter would leave the scene camera's alone.
template <class Launch>
int matte_pass(vpt_gpu_ctx* ctx, const char* fn, const char* noun, void* hip_stream, Launch launch) {
  int rc = ctx_device(ctx);
  if (rc) return rc;
  const auto refuse = [fn](int code, const std::string& what) { return vpt::set_error(code, std::string(fn) + ": " + what); };
  if (ctx->open_feeds.load() > 0)  // (the launch would queue behind the feed's, which holds the device)
    return refuse(VPT_E_STATE, "a feed of this context is open");
  if (!ctx->shutter.empty())
    return refuse(VPT_E_STATE, std::string("a shutter is attached and the ") + noun +
                                   " would be the scene camera's alone: detach it (vpt_gpu_set_shutter NULL, 0)");
  if (!ctx->volume_ok) return volume_gone();
  if ((rc = ensure_order(ctx))) return rc;  // (the tile ranks: computed by the context's first call that needs them)
  const uint64_t blocks = ctx->scene.T * (((uint64_t)ctx->scene.tile_area + 63u) / 64u);
  if (blocks >= (1ULL << 31)) return refuse(VPT_E_INVALID, "2^31 or more pixel chunks");
  hipStream_t s = (hipStream_t)hip_stream;
  uint32_t slot = 0;  // (a ring slot, so that vpt_gpu_sync and scene updates wait for the pass as for any launch)
  if ((rc = take_slot(ctx, s, slot))) return rc;
  launch(dim3((unsigned)blocks), s);
  const hipError_t e = hipGetLastError();
  if ((rc = release_slot(ctx, s, slot))) return rc;
  if (e != hipSuccess) return refuse(VPT_E_HIP, hipGetErrorString(e));
  return VPT_OK;
}
}  // namespace

extern "C" {

int vpt_gpu_create(const vpt_configuration* cfg, const vpt_grid_desc* density, const vpt_grid_desc* temperature,
                   const float* blackbody_500x3, int device, vpt_gpu_ctx** out) {
  if (!cfg || !density || !out) return vpt::set_error(VPT_E_INVALID, "vpt_gpu_create: null argument");
  *out = nullptr;
  if (int rc = check_device(device, "vpt_gpu_create")) return rc;
  HostGrids g;
  if (int rc = build_grids(density, temperature, g, &g.flatten_ms)) return rc;
  return create_on(cfg, g, blackbody_500x3, device, out);
}

int vpt_gpu_create_many(const vpt_configuration* cfg, const vpt_grid_desc* density, const vpt_grid_desc* temperature,
                        const float* blackbody_500x3, const int* devices, int n, vpt_gpu_ctx** out) {
  if (!cfg || !density || !out || !devices || n <= 0) return vpt::set_error(VPT_E_INVALID, "vpt_gpu_create_many: bad argument");
  for (int i = 0; i < n; ++i) out[i] = nullptr;
  for (int i = 0; i < n; ++i)
    if (int rc = check_device(devices[i], "vpt_gpu_create_many")) return rc;
  vpt_host_grids* g = nullptr;
  if (int rc = vpt_grids_flatten(density, temperature, &g)) return rc;
  const int rc = vpt_gpu_create_from(cfg, g, blackbody_500x3, devices, n, out);
  vpt_grids_free(g);
  return rc;
}

int vpt_grids_flatten(const vpt_grid_desc* density, const vpt_grid_desc* temperature, vpt_host_grids** out) {
  if (!density || !out) return vpt::set_error(VPT_E_INVALID, "vpt_grids_flatten: null argument");
  *out = nullptr;
  std::unique_ptr<vpt_host_grids> g(new vpt_host_grids());
  if (int rc = build_grids(density, temperature, *g, &g->flatten_ms)) return rc;
  *out = g.release();
  return VPT_OK;
}

void vpt_grids_free(vpt_host_grids* grids) { delete grids; }

int vpt_gpu_create_from(const vpt_configuration* cfg, const vpt_host_grids* grids, const float* blackbody_500x3,
                        const int* devices, int n, vpt_gpu_ctx** out) {
  if (!cfg || !grids || !out || !devices || n <= 0) return vpt::set_error(VPT_E_INVALID, "vpt_gpu_create_from: bad argument");
  for (int i = 0; i < n; ++i) out[i] = nullptr;
  for (int i = 0; i < n; ++i)
    if (int rc = check_device(devices[i], "vpt_gpu_create_from")) return rc;
  // one thread per device: each uploads the same host grids (vpt_last_error is per thread: the first failure's
  // message is carried back)
  std::vector<int> rcs((size_t)n, VPT_OK);
  std::vector<std::string> msgs((size_t)n);
  std::vector<std::thread> pool;
  for (int i = 0; i < n; ++i)
    pool.emplace_back([&, i] {
      rcs[(size_t)i] = create_on(cfg, *grids, blackbody_500x3, devices[i], &out[i]);
      if (rcs[(size_t)i]) msgs[(size_t)i] = vpt_last_error();
    });
  for (auto& th : pool) th.join();
  for (int i = 0; i < n; ++i)
    if (rcs[(size_t)i]) {
      for (int k = 0; k < n; ++k) {
        destroy(out[k]);
        out[k] = nullptr;
      }
      return vpt::set_error(rcs[(size_t)i], "device " + std::to_string(devices[i]) + ": " + msgs[(size_t)i]);
    }
  return VPT_OK;
}

int vpt_gpu_setup_timings(const vpt_gpu_ctx* ctx, double* ms, int n) {
  if (!ctx || !ms || n < 0) return vpt::set_error(VPT_E_INVALID, "vpt_gpu_setup_timings: bad argument");
  for (int i = 0; i < n && i < 5; ++i) ms[i] = ctx->setup_ms[i];
  return VPT_OK;
}

int vpt_gpu_destroy(vpt_gpu_ctx* ctx) {
  destroy(ctx);
  return VPT_OK;
}

int vpt_gpu_set_scene(vpt_gpu_ctx* ctx, const vpt_configuration* cfg) {
  if (!ctx || !cfg) return vpt::set_error(VPT_E_INVALID, "vpt_gpu_set_scene: null argument");
  int rc = ctx_device(ctx);
  if (rc) return rc;
  if (ctx->open_feeds.load() > 0) return vpt::set_error(VPT_E_STATE, "vpt_gpu_set_scene: a feed of this context is open");
  if (ctx->frame_waves) return vpt::set_error(VPT_E_STATE, "vpt_gpu_set_scene: a frame is open");
  if (!ctx->volume_ok) return volume_gone();
  for (int i = 0; i < 2; ++i) {
    if (cfg->output_size[i] != ctx->cfg.output_size[i])
      return vpt::set_error(VPT_E_INVALID, "vpt_gpu_set_scene: output_size differs from the context's (the film, the "
                                           "tiles and every buffer sized by them are fixed at creation)");
    if (cfg->tile_size[i] != ctx->cfg.tile_size[i])
      return vpt::set_error(VPT_E_INVALID, "vpt_gpu_set_scene: tile_size differs from the context's (the job space is "
                                           "fixed at creation)");
  }
  vpt::DevScene S;  // built aside: any error above or here leaves the context's scene as it was
  if ((rc = derive_scene(ctx, *cfg, S))) return rc;
  if ((rc = wait_ctx(ctx))) return rc;  // (launches in flight read the scene and the ranks about to change)
  ctx->scene = S;
  ctx->cfg = *cfg;
  drop_order(ctx);
  return push_scene(ctx);
}

int vpt_gpu_set_grids(vpt_gpu_ctx* ctx, const vpt_host_grids* grids) {
  if (!ctx || !grids) return vpt::set_error(VPT_E_INVALID, "vpt_gpu_set_grids: null argument");
  int rc = ctx_device(ctx);
  if (rc) return rc;
  if (ctx->open_feeds.load() > 0) return vpt::set_error(VPT_E_STATE, "vpt_gpu_set_grids: a feed of this context is open");
  if (ctx->frame_waves) return vpt::set_error(VPT_E_STATE, "vpt_gpu_set_grids: a frame is open");
  if (grids->has_temperature != ctx->has_temperature)
    return vpt::set_error(VPT_E_INVALID, ctx->has_temperature
                                             ? "vpt_gpu_set_grids: the context has a temperature grid and the new volume has none "
                                               "(the kernel family is chosen at creation)"
                                             : "vpt_gpu_set_grids: the context has no temperature grid and the new volume has one "
                                               "(the kernel family is chosen at creation)");
  if ((rc = wait_ctx(ctx))) return rc;  // (launches in flight read the tables and pools about to be freed)
  VPT_HIP(hipDeviceSynchronize());      // (launches on the caller's streams and the null stream too)
  // The old volume goes first, so that the peak is one volume and not two.  From here on a failure leaves the
  // context without a volume (volume_ok false: no device pointer of the freed tables stays in use).
  ctx->volume_ok = false;
  drop_order(ctx);
  vpt::free_grid(ctx->density);
  vpt::free_grid(ctx->temperature);
  ctx->scene.density = ctx->density.dev;
  ctx->scene.temperature = ctx->temperature.dev;
  auto fail = [&](int code) {
    const std::string msg = vpt_last_error();  // (the frees and the push below must not replace the cause)
    vpt::free_grid(ctx->density);
    vpt::free_grid(ctx->temperature);
    ctx->scene.density = ctx->density.dev;
    ctx->scene.temperature = ctx->temperature.dev;
    (void)push_scene(ctx);
    return vpt::set_error(code, "vpt_gpu_set_grids: " + msg + " (the context has no volume now)");
  };
  // (vpt_gpu_debug_fail_upload: the n-th upload from the call on is refused as a device without room refuses it)
  auto upload = [&](const vpt::HostGrid& h, vpt::DeviceGrid& d) {
    if (ctx->debug_fail_upload > 0 && --ctx->debug_fail_upload == 0)
      return vpt::set_error(VPT_E_NOMEM, "grid upload: refused (vpt_gpu_debug_fail_upload)");
    return vpt::upload_grid(h, d);
  };
  if ((rc = upload(grids->density, ctx->density))) return fail(rc);
  if (grids->has_temperature && (rc = upload(grids->temperature, ctx->temperature))) return fail(rc);
  ctx->temp_range = grids->temp_range;
  // What creation derives from the grids: the run-skipping choice (a forced one stays), the occupancy-sized grid (of
  // the kernel the grids choose, as at creation; a grid set by vpt_gpu_set_tuning stays), the pool's layout under the
  // kept policy and cap, and the scene.
  const bool auto_runs = auto_run_skipping(ctx);
  ctx->use_runs = ctx->runs_mode < 0 ? auto_runs : ctx->runs_mode == 1;
  if ((rc = size_grid(ctx, auto_runs))) return fail(rc);
  if ((rc = apply_pool_layout(ctx, ctx->pool_policy))) return fail(rc);
  vpt::DevScene S;
  if ((rc = derive_scene(ctx, ctx->cfg, S))) return fail(rc);
  ctx->scene = S;
  if ((rc = push_scene(ctx))) return fail(rc);
  ctx->volume_ok = true;
  return VPT_OK;
}

int vpt_gpu_job_space(const vpt_gpu_ctx* ctx, uint64_t* jobs_per_wave, uint64_t* total_jobs) {
  if (!ctx) return vpt::set_error(VPT_E_INVALID, "null context");
  if (jobs_per_wave) *jobs_per_wave = ctx->scene.T;
  if (total_jobs) *total_jobs = ctx->scene.T * (uint64_t)ctx->cfg.num_waves;
  return VPT_OK;
}

int vpt_gpu_render_jobs(vpt_gpu_ctx* ctx, uint64_t jid_begin, uint64_t jid_count, float* film_device,
                        void* hip_stream) {
  return render(ctx, jid_begin, jid_count, film_device, nullptr, hip_stream);
}

int vpt_gpu_render_tiles(vpt_gpu_ctx* ctx, uint32_t tile_lo, uint32_t tile_hi, uint64_t wave_begin, uint64_t wave_count,
                         float* film_device, void* hip_stream) {
  if (!ctx) return vpt::set_error(VPT_E_INVALID, "vpt_gpu_render_tiles: null context");
  int rc = ctx_device(ctx);
  if (rc) return rc;
  const uint64_t T = ctx->scene.T;
  if (tile_lo >= tile_hi || tile_hi > T) return vpt::set_error(VPT_E_INVALID, "vpt_gpu_render_tiles: bad tile range");
  if (ctx->scene.pixel_mode)
    return vpt::set_error(VPT_E_INVALID, "vpt_gpu_render_tiles: band launches run the reference RNG mode");
  // 32-bit work items, job offsets (w * T + tile) and wave slots (tiles x waves padded to whole groups)
  const uint64_t B = tile_hi - tile_lo, G = vpt::kBandGroup;
  if (wave_count >= (1ULL << 32) || (wave_count + G - 1) / G * G * std::max(B, T) >= (1ULL << 32) ||
      wave_begin > (UINT64_MAX / T) - wave_count)
    return vpt::set_error(VPT_E_INVALID, "vpt_gpu_render_tiles: 2^32 or more sample slots (render fewer waves per call)");
  if (ctx->film_order != VPT_FILM_ORDERED)
    return vpt::set_error(VPT_E_STATE, "vpt_gpu_render_tiles: band launches need the ordered film "
                                       "(vpt_gpu_set_film_order: VPT_FILM_ORDERED)");
  if (ctx->frame_waves)
    return vpt::set_error(VPT_E_STATE, "vpt_gpu_render_tiles: a frame is open (vpt_gpu_frame_open owns the sample buffer)");
  if (wave_count == 0) return VPT_OK;
  return render_band_waves(ctx, tile_lo, (uint32_t)B, false, wave_begin, wave_count, film_device, hip_stream);
}

int vpt_gpu_render_tile_list(vpt_gpu_ctx* ctx, const uint32_t* tiles, uint32_t n, uint64_t wave_begin, uint64_t wave_count,
                             float* film_device, void* hip_stream) {
  if (!ctx) return vpt::set_error(VPT_E_INVALID, "vpt_gpu_render_tile_list: null context");
  if (n && !tiles) return vpt::set_error(VPT_E_INVALID, "vpt_gpu_render_tile_list: null tile list");
  int rc = ctx_device(ctx);
  if (rc) return rc;
  const uint64_t T = ctx->scene.T;
  for (uint32_t i = 0; i < n; ++i)
    if (tiles[i] >= T || (i && tiles[i] <= tiles[i - 1]))
      return vpt::set_error(VPT_E_INVALID, "vpt_gpu_render_tile_list: the list must be strictly ascending tile indices < T");
  if (ctx->scene.pixel_mode)
    return vpt::set_error(VPT_E_INVALID, "vpt_gpu_render_tile_list: list launches run the reference RNG mode");
  const uint64_t G = vpt::kBandGroup;  // (the same 32-bit limits as vpt_gpu_render_tiles)
  if (wave_count >= (1ULL << 32) || (wave_count + G - 1) / G * G * T >= (1ULL << 32) || wave_begin > (UINT64_MAX / T) - wave_count)
    return vpt::set_error(VPT_E_INVALID, "vpt_gpu_render_tile_list: 2^32 or more sample slots (render fewer waves per call)");
  if (ctx->film_order != VPT_FILM_ORDERED)
    return vpt::set_error(VPT_E_STATE, "vpt_gpu_render_tile_list: list launches need the ordered film "
                                       "(vpt_gpu_set_film_order: VPT_FILM_ORDERED)");
  if (ctx->frame_waves)
    return vpt::set_error(VPT_E_STATE, "vpt_gpu_render_tile_list: a frame is open (vpt_gpu_frame_open owns the sample buffer)");
  if (ctx->open_feeds.load() > 0)  // (the upload below would wait for the feed's launch, which holds the device)
    return vpt::set_error(VPT_E_STATE, "vpt_gpu_render_tile_list: a feed of this context is open");
  if (wave_count == 0 || n == 0) return VPT_OK;
  if ((rc = ensure_order(ctx))) return rc;  // (allocates the list's buffers with the tile ranks)
  if (ctx->list_host.size() != n || !std::equal(tiles, tiles + n, ctx->list_host.begin())) {
    // The previous ordered launch may still read the list and the map (its film pass, its kernels' job starts).
    if (ctx->samples_used) VPT_HIP(hipEventSynchronize(ctx->samples_done));
    ctx->list_host.clear();  // (nothing valid on the device until both copies are done)
    ctx->list_ranked = false;
    ctx->list_slot_host.assign(T, vpt::kNoListSlot);
    for (uint32_t i = 0; i < n; ++i) ctx->list_slot_host[tiles[i]] = i;
    VPT_HIP(hipMemcpy(ctx->list_dev, tiles, (size_t)n * sizeof(uint32_t), hipMemcpyHostToDevice));
    VPT_HIP(hipMemcpy(ctx->list_slot_dev, ctx->list_slot_host.data(), T * sizeof(uint32_t), hipMemcpyHostToDevice));
    ctx->list_host.assign(tiles, tiles + n);
  }
  return render_band_waves(ctx, 0, n, true, wave_begin, wave_count, film_device, hip_stream);
}

int vpt_gpu_render_alpha(vpt_gpu_ctx* ctx, uint32_t sub, float* alpha_device, float* tau_device, void* hip_stream) {
  if (!ctx) return vpt::set_error(VPT_E_INVALID, "vpt_gpu_render_alpha: null context");
  if (!alpha_device) return vpt::set_error(VPT_E_INVALID, "vpt_gpu_render_alpha: null alpha plane");
  if (sub < 1 || sub > vpt::kAlphaMaxSub)
    return vpt::set_error(VPT_E_INVALID, "vpt_gpu_render_alpha: sub-rays per axis must be 1..8");
  return matte_pass(ctx, "vpt_gpu_render_alpha", "matte", hip_stream, [&](dim3 blocks, hipStream_t s) {
    hipLaunchKernelGGL(vpt::vpt_alpha_kernel, blocks, dim3(64), 0, s, ctx->scene_dev, (const uint32_t*)ctx->order, sub,
                       alpha_device, tau_device);
  });
}

int vpt_gpu_render_depth(vpt_gpu_ctx* ctx, uint32_t sub, uint32_t n_levels, const float* opacity_host, float* depth_device,
                         float* reach_device, void* hip_stream) {
  if (!ctx) return vpt::set_error(VPT_E_INVALID, "vpt_gpu_render_depth: null context");
  if (!depth_device) return vpt::set_error(VPT_E_INVALID, "vpt_gpu_render_depth: null depth plane");
  if (sub < 1 || sub > vpt::kAlphaMaxSub)
    return vpt::set_error(VPT_E_INVALID, "vpt_gpu_render_depth: sub-rays per axis must be 1..8");
  vpt::DepthLevels levels;  // (tau_k = -log1p(-a_k), once, here)
  if (const char* why = vpt::depth_levels(n_levels, opacity_host, levels))
    return vpt::set_error(VPT_E_INVALID, std::string("vpt_gpu_render_depth: ") + why);
  return matte_pass(ctx, "vpt_gpu_render_depth", "depth", hip_stream, [&](dim3 blocks, hipStream_t s) {
    hipLaunchKernelGGL(vpt::vpt_depth_kernel, blocks, dim3(64), 0, s, ctx->scene_dev, (const uint32_t*)ctx->order, sub,
                       levels, depth_device, reach_device);
  });
}

int vpt_gpu_denoise(vpt_gpu_ctx* ctx, const vpt_denoise_params* p, const float* film_device, const float* m2_device,
                    const float* const* guides_device, float* out_film_device, float* var_out_device, void* hip_stream) {
  // (the arguments are checked before the context, so that every refusal is testable without a device)
  if (!p) return vpt::set_error(VPT_E_INVALID, "vpt_gpu_denoise: null params");
  if (!film_device || !m2_device || !out_film_device)
    return vpt::set_error(VPT_E_INVALID, "vpt_gpu_denoise: null film, moment plane or output film");
  if (p->iterations < 1 || p->iterations > vpt::kDenoiseMaxIterations)
    return vpt::set_error(VPT_E_INVALID, "vpt_gpu_denoise: iterations must be 1..6");
  if (p->n_guides > vpt::kDenoiseMaxGuides) return vpt::set_error(VPT_E_INVALID, "vpt_gpu_denoise: at most 4 guides");
  if (!(p->sigma_l > 0.0f) || !(p->rel_floor > 0.0f))
    return vpt::set_error(VPT_E_INVALID, "vpt_gpu_denoise: sigma_l and rel_floor must be > 0");
  if (p->n_guides && !guides_device) return vpt::set_error(VPT_E_INVALID, "vpt_gpu_denoise: null guide array");
  for (uint32_t k = 0; k < p->n_guides; ++k) {
    if (!guides_device[k]) return vpt::set_error(VPT_E_INVALID, "vpt_gpu_denoise: null guide plane");
    if (!(p->guide_sigma[k] > 0.0f)) return vpt::set_error(VPT_E_INVALID, "vpt_gpu_denoise: guide_sigma must be > 0");
  }
  // (float4 loads and stores on the films; the planes are read and written as floats)
  bool aligned = ((uintptr_t)film_device | (uintptr_t)out_film_device) % 16 == 0 &&
                 ((uintptr_t)m2_device | (uintptr_t)var_out_device) % 4 == 0;
  for (uint32_t k = 0; k < p->n_guides; ++k) aligned = aligned && (uintptr_t)guides_device[k] % 4 == 0;
  if (!aligned)
    return vpt::set_error(VPT_E_INVALID, "vpt_gpu_denoise: the films must be 16-byte aligned, the planes 4-byte aligned");
  if (!ctx) return vpt::set_error(VPT_E_INVALID, "vpt_gpu_denoise: null context");
  const size_t N = (size_t)ctx->scene.W * (size_t)ctx->scene.H, fb = N * 4 * sizeof(float), pb = N * sizeof(float);
  bool alias = ranges_overlap(out_film_device, fb, film_device, fb) || ranges_overlap(out_film_device, fb, m2_device, pb) ||
               ranges_overlap(out_film_device, fb, var_out_device, pb) ||
               ranges_overlap(var_out_device, pb, film_device, fb) || ranges_overlap(var_out_device, pb, m2_device, pb);
  for (uint32_t k = 0; k < p->n_guides; ++k)
    alias = alias || ranges_overlap(out_film_device, fb, guides_device[k], pb) ||
            ranges_overlap(var_out_device, pb, guides_device[k], pb);
  if (alias) return vpt::set_error(VPT_E_INVALID, "vpt_gpu_denoise: an output overlaps an input or the other output");
  int rc = ctx_device(ctx);
  if (rc) return rc;
  if (ctx->open_feeds.load() > 0)  // (the call allocates, and its launches would queue behind the feed's)
    return vpt::set_error(VPT_E_STATE, "vpt_gpu_denoise: a feed of this context is open");
  const uint32_t G = p->n_guides;
  const uint64_t bytes = (uint64_t)N * sizeof(float4) * (G ? 3u : 2u);
  // The packed planes are the context's, shared by every call: from here to the record below one call at a time.
  std::lock_guard<std::mutex> scratch_lock(ctx->denoise_mu);
  if (!ctx->denoise_done) VPT_HIP(hipEventCreateWithFlags(&ctx->denoise_done, hipEventDisableTiming));
  if (ctx->denoise_scratch_bytes < bytes) {
    if (ctx->denoise_used) VPT_HIP(hipEventSynchronize(ctx->denoise_done));  // no earlier call still uses the planes
    (void)hipFree(ctx->denoise_scratch);
    ctx->denoise_scratch = nullptr;
    ctx->denoise_scratch_bytes = 0;
    const hipError_t e = hipMalloc(&ctx->denoise_scratch, bytes);
    if (e != hipSuccess) {
      ctx->denoise_scratch = nullptr;
      (void)hipGetLastError();
      return vpt::set_error(VPT_E_NOMEM, "vpt_gpu_denoise: " + std::to_string(bytes >> 20) + " MiB of packed planes: " +
                                             hipGetErrorString(e));
    }
    ctx->denoise_scratch_bytes = bytes;
  }
  vpt::DenoiseArgs A{};
  A.W = ctx->scene.W;
  A.H = ctx->scene.H;
  A.sigma_l = p->sigma_l;
  A.rel_floor = p->rel_floor;
  vpt::DenoiseGuidePtrs gp{};
  for (uint32_t k = 0; k < 4; ++k) {
    A.guide_sigma[k] = k < G ? p->guide_sigma[k] : 1.0f;
    gp.g[k] = k < G ? guides_device[k] : nullptr;
  }
  float4* const plane0 = (float4*)ctx->denoise_scratch;
  float4* const plane1 = plane0 + N;
  float4* const gd = G ? plane1 + N : nullptr;
  const dim3 block(vpt::kDenoiseBlockX, vpt::kDenoiseBlockY);
  const dim3 grid((unsigned)(((uint64_t)A.W + vpt::kDenoiseBlockX - 1) / vpt::kDenoiseBlockX),
                  (unsigned)(((uint64_t)A.H + vpt::kDenoiseBlockY - 1) / vpt::kDenoiseBlockY));
  if (grid.y > 65535u) return vpt::set_error(VPT_E_INVALID, "vpt_gpu_denoise: more than 262140 rows");
  hipStream_t s = (hipStream_t)hip_stream;
  uint32_t slot = 0;  // (a ring slot, so that vpt_gpu_sync and scene updates wait for the filter as for any launch)
  if ((rc = take_slot(ctx, s, slot))) return rc;
  // The previous call's kernels, on whatever stream they ran, are done with the planes before prepare overwrites them.
  if (ctx->denoise_used) VPT_HIP(hipStreamWaitEvent(s, ctx->denoise_done, 0));
  const float4* const film4 = reinterpret_cast<const float4*>(film_device);
  hipLaunchKernelGGL(vpt::vpt_denoise_prepare_kernel, grid, block, 0, s, A, G, film4, m2_device, gp, plane0, gd);
  float4 *src = plane0, *dst = plane1;
  for (uint32_t i = 0; i < p->iterations; ++i) {
    const bool last = i + 1 == p->iterations;
    const int32_t step = (int32_t)(1u << i);
    float4* const of = reinterpret_cast<float4*>(out_film_device);
    switch (G) {
      case 0: launch_denoise_atrous<0>(last, grid, block, s, A, step, src, gd, dst, film4, of, var_out_device); break;
      case 1: launch_denoise_atrous<1>(last, grid, block, s, A, step, src, gd, dst, film4, of, var_out_device); break;
      case 2: launch_denoise_atrous<2>(last, grid, block, s, A, step, src, gd, dst, film4, of, var_out_device); break;
      case 3: launch_denoise_atrous<3>(last, grid, block, s, A, step, src, gd, dst, film4, of, var_out_device); break;
      default: launch_denoise_atrous<4>(last, grid, block, s, A, step, src, gd, dst, film4, of, var_out_device); break;
    }
    std::swap(src, dst);
  }
  const hipError_t e = hipGetLastError();
  const hipError_t er = hipEventRecord(ctx->denoise_done, s);  // (recorded whatever was launched: the next call waits)
  if (er == hipSuccess) ctx->denoise_used = true;
  if ((rc = release_slot(ctx, s, slot))) return rc;
  if (e != hipSuccess) return vpt::set_error(VPT_E_HIP, std::string("vpt_gpu_denoise: ") + hipGetErrorString(e));
  if (er != hipSuccess) return vpt::set_error(VPT_E_HIP, std::string("vpt_gpu_denoise: ") + hipGetErrorString(er));
  return VPT_OK;
}

int vpt_gpu_temporal(vpt_gpu_ctx* ctx, const vpt_temporal_params* p, const float* film_device, const float* m2_device,
                     const float* depth_device, const vpt_shutter_camera* prev_cam, const float* hist_film_device,
                     const float* hist_m2_device, const float* hist_depth_device, float* out_film_device,
                     float* out_m2_device, float* motion_out_device, float* hist_n_out_device, void* hip_stream) {
  // (the arguments are checked before the context, so that every refusal is testable without a device)
  if (!p) return vpt::set_error(VPT_E_INVALID, "vpt_gpu_temporal: null params");
  if (!film_device || !m2_device || !depth_device)
    return vpt::set_error(VPT_E_INVALID, "vpt_gpu_temporal: null film, moment plane or depth planes");
  if (!out_film_device || !out_m2_device)
    return vpt::set_error(VPT_E_INVALID, "vpt_gpu_temporal: null output film or output plane");
  if (!prev_cam) return vpt::set_error(VPT_E_INVALID, "vpt_gpu_temporal: null previous camera");
  const int n_hist = (hist_film_device != nullptr) + (hist_m2_device != nullptr) + (hist_depth_device != nullptr);
  if (n_hist != 0 && n_hist != 3)
    return vpt::set_error(VPT_E_INVALID, "vpt_gpu_temporal: a history is a film, a plane and depth planes, or all three NULL");
  if (p->n_levels < 1 || p->n_levels > vpt::kTemporalMaxLevels)
    return vpt::set_error(VPT_E_INVALID, "vpt_gpu_temporal: n_levels must be 1..4");
  if (!(p->max_history > 0.0f) || !(p->depth_tol > 0.0f) || !(p->sigma_r > 0.0f) || !(p->rel_floor > 0.0f))
    return vpt::set_error(VPT_E_INVALID, "vpt_gpu_temporal: max_history, depth_tol, sigma_r and rel_floor must be > 0");
  // (float4 loads and stores on the films; the planes are read and written as floats)
  if (((uintptr_t)film_device | (uintptr_t)hist_film_device | (uintptr_t)out_film_device) % 16 != 0 ||
      ((uintptr_t)m2_device | (uintptr_t)depth_device | (uintptr_t)hist_m2_device | (uintptr_t)hist_depth_device |
       (uintptr_t)out_m2_device | (uintptr_t)motion_out_device | (uintptr_t)hist_n_out_device) % 4 != 0)
    return vpt::set_error(VPT_E_INVALID, "vpt_gpu_temporal: the films must be 16-byte aligned, the planes 4-byte aligned");
  if (const char* why = vpt::camera_invalid(prev_cam->position, prev_cam->look, prev_cam->up, prev_cam->vfov_deg))
    return vpt::set_error(VPT_E_INVALID, std::string("vpt_gpu_temporal: previous camera: ") + why);
  if (!ctx) return vpt::set_error(VPT_E_INVALID, "vpt_gpu_temporal: null context");
  const size_t N = (size_t)ctx->scene.W * (size_t)ctx->scene.H, pb = N * sizeof(float);
  {
    const struct { const void* ptr; size_t bytes; } in[6] = {{film_device, 4 * pb}, {m2_device, pb},
        {depth_device, p->n_levels * pb}, {hist_film_device, 4 * pb}, {hist_m2_device, pb},
        {hist_depth_device, p->n_levels * pb}},
        out[4] = {{out_film_device, 4 * pb}, {out_m2_device, pb}, {motion_out_device, 2 * pb}, {hist_n_out_device, pb}};
    bool alias = false;
    for (int o = 0; o < 4; ++o) {
      for (int i = 0; i < 6; ++i) alias = alias || ranges_overlap(out[o].ptr, out[o].bytes, in[i].ptr, in[i].bytes);
      for (int o2 = o + 1; o2 < 4; ++o2) alias = alias || ranges_overlap(out[o].ptr, out[o].bytes, out[o2].ptr, out[o2].bytes);
    }
    if (alias) return vpt::set_error(VPT_E_INVALID, "vpt_gpu_temporal: an output overlaps an input or another output");
  }
  int rc = ctx_device(ctx);
  if (rc) return rc;
  vpt::TemporalArgs A{};
  A.W = ctx->scene.W;
  A.H = ctx->scene.H;
  A.n_levels = p->n_levels;
  A.has_history = n_hist == 3;
  A.max_history = p->max_history;
  A.depth_tol = p->depth_tol;
  A.sigma_r = p->sigma_r;
  A.rel_floor = p->rel_floor;
  // The current camera is the scene's, in a shutter entry's layout; the previous one by the shutter's own derivation.
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j) A.cur[4 * i + j] = ctx->scene.cam_L[3 * i + j];
    A.cur[4 * i + 3] = ctx->scene.cam_t[i];
    A.cur[12 + i] = ctx->scene.cam_pos[i];
  }
  float prev[16];
  vpt::shutter_entry(*prev_cam, A.W, A.H, prev);
  vpt::temporal_prev_constants(prev, A);
  const dim3 block(vpt::kTemporalBlockX, vpt::kTemporalBlockY);
  const dim3 grid((unsigned)(((uint64_t)A.W + vpt::kTemporalBlockX - 1) / vpt::kTemporalBlockX),
                  (unsigned)(((uint64_t)A.H + vpt::kTemporalBlockY - 1) / vpt::kTemporalBlockY));
  if (grid.y > 65535u) return vpt::set_error(VPT_E_INVALID, "vpt_gpu_temporal: more than 262140 rows");
  hipStream_t s = (hipStream_t)hip_stream;
  uint32_t slot = 0;  // (a ring slot, so that vpt_gpu_sync and scene updates wait for the pass as for any launch)
  if ((rc = take_slot(ctx, s, slot))) return rc;
  hipLaunchKernelGGL(vpt::vpt_temporal_kernel, grid, block, 0, s, A, reinterpret_cast<const float4*>(film_device), m2_device,
                     depth_device, reinterpret_cast<const float4*>(hist_film_device), hist_m2_device, hist_depth_device,
                     reinterpret_cast<float4*>(out_film_device), out_m2_device, motion_out_device, hist_n_out_device);
  const hipError_t e = hipGetLastError();
  if ((rc = release_slot(ctx, s, slot))) return rc;
  if (e != hipSuccess) return vpt::set_error(VPT_E_HIP, std::string("vpt_gpu_temporal: ") + hipGetErrorString(e));
  return VPT_OK;
}

int vpt_gpu_set_film_moments(vpt_gpu_ctx* ctx, float* m2_device) {
  if (!ctx) return vpt::set_error(VPT_E_INVALID, "vpt_gpu_set_film_moments: null context");
  if (m2_device && ctx->film_order != VPT_FILM_ORDERED)
    return vpt::set_error(VPT_E_STATE, "vpt_gpu_set_film_moments: the plane is written by the ordered film passes "
                                       "(vpt_gpu_set_film_order: VPT_FILM_ORDERED)");
  if (m2_device && ctx->frame_waves)
    return vpt::set_error(VPT_E_STATE, "vpt_gpu_set_film_moments: a frame is open (its launches add with film atomics)");
  ctx->m2 = m2_device;  // read by the next render's host code only: no wait
  return VPT_OK;
}

int vpt_gpu_set_light_groups(vpt_gpu_ctx* ctx, float* groups_device) {
  if (!ctx) return vpt::set_error(VPT_E_INVALID, "vpt_gpu_set_light_groups: null context");
  if (groups_device && (uintptr_t)groups_device % 16 != 0)
    return vpt::set_error(VPT_E_INVALID, "vpt_gpu_set_light_groups: the planes must be 16-byte aligned");
  if (groups_device && ctx->film_order != VPT_FILM_ORDERED)
    return vpt::set_error(VPT_E_STATE, "vpt_gpu_set_light_groups: the planes are written by the ordered film passes "
                                       "(vpt_gpu_set_film_order: VPT_FILM_ORDERED)");
  if (groups_device && ctx->frame_waves)
    return vpt::set_error(VPT_E_STATE, "vpt_gpu_set_light_groups: a frame is open (its launches add with film atomics)");
  ctx->groups = groups_device;  // read by the next render's host code only: no wait
  return VPT_OK;
}

int vpt_gpu_relight(vpt_gpu_ctx* ctx, const float* groups_device, const float gains[9], float* film_out_device,
                    void* hip_stream) {
  if (!ctx || !groups_device || !gains || !film_out_device)
    return vpt::set_error(VPT_E_INVALID, "vpt_gpu_relight: null argument");
  if (((uintptr_t)groups_device | (uintptr_t)film_out_device) % 16 != 0)
    return vpt::set_error(VPT_E_INVALID, "vpt_gpu_relight: the planes must be 16-byte aligned");
  const uint64_t npix = (uint64_t)ctx->scene.W * (uint64_t)ctx->scene.H;
  if (ranges_overlap(film_out_device, npix * 16, groups_device, 3 * npix * 16))
    return vpt::set_error(VPT_E_INVALID, "vpt_gpu_relight: the output aliases the group planes");
  int rc = ctx_device(ctx);
  if (rc) return rc;
  vpt::RelightGains K;
  for (int i = 0; i < 9; ++i) K.k[i] = gains[i];
  hipLaunchKernelGGL(vpt::vpt_relight_kernel, dim3((unsigned)((npix + 255) / 256)), dim3(256), 0, (hipStream_t)hip_stream,
                     reinterpret_cast<const float4*>(groups_device), K, npix, reinterpret_cast<float4*>(film_out_device));
  VPT_HIP(hipGetLastError());
  return VPT_OK;
}

int vpt_gpu_set_shutter(vpt_gpu_ctx* ctx, const vpt_shutter_camera* cams, uint32_t n) {
  if (!ctx) return vpt::set_error(VPT_E_INVALID, "vpt_gpu_set_shutter: null context");
  if ((cams == nullptr) != (n == 0))
    return vpt::set_error(VPT_E_INVALID, "vpt_gpu_set_shutter: cameras and a count of 1 .. 65536, or NULL and 0 to detach");
  if (n > VPT_SHUTTER_MAX) return vpt::set_error(VPT_E_INVALID, "vpt_gpu_set_shutter: more than 65536 entries");
  int rc = ctx_device(ctx);
  if (rc) return rc;
  if (ctx->open_feeds.load() > 0) return vpt::set_error(VPT_E_STATE, "vpt_gpu_set_shutter: a feed of this context is open");
  if (ctx->frame_waves) return vpt::set_error(VPT_E_STATE, "vpt_gpu_set_shutter: a frame is open");
  // The table is built aside: an entry that fails leaves the context's shutter as it was.
  std::vector<float> table((size_t)n * 16);
  for (uint32_t i = 0; i < n; ++i) {
    if (const char* why = vpt::camera_invalid(cams[i].position, cams[i].look, cams[i].up, cams[i].vfov_deg))
      return vpt::set_error(VPT_E_INVALID, "vpt_gpu_set_shutter: entry " + std::to_string(i) + ": " + why);
    vpt::shutter_entry(cams[i], ctx->scene.W, ctx->scene.H, table.data() + (size_t)i * 16);
  }
  float* dev = nullptr;
  if (n) {
    VPT_HIP(hipMalloc(&dev, table.size() * sizeof(float)));  // (256-byte aligned: every entry on a 64-byte line)
    const hipError_t e = hipMemcpy(dev, table.data(), table.size() * sizeof(float), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
      (void)hipFree(dev);
      return vpt::set_error(VPT_E_HIP, std::string("vpt_gpu_set_shutter: upload: ") + hipGetErrorString(e));
    }
  }
  if ((rc = wait_ctx(ctx))) {  // (launches in flight read the table about to be freed)
    if (dev) (void)hipFree(dev);
    return rc;
  }
  if (ctx->shutter_dev) (void)hipFree(ctx->shutter_dev);
  ctx->shutter_dev = dev;
  ctx->shutter.assign(cams, cams + n);
  return VPT_OK;
}

int vpt_gpu_shutter_info(const vpt_gpu_ctx* ctx, uint32_t* n) {
  if (!ctx || !n) return vpt::set_error(VPT_E_INVALID, "vpt_gpu_shutter_info: null argument");
  *n = (uint32_t)ctx->shutter.size();
  return VPT_OK;
}

int vpt_gpu_tile_errors(vpt_gpu_ctx* ctx, const float* film_device, const float* m2_device, float abs_floor,
                        float* err_T_host, void* hip_stream) {
  if (!ctx) return vpt::set_error(VPT_E_INVALID, "vpt_gpu_tile_errors: null context");
  if (!m2_device || !err_T_host || !(abs_floor > 0.0f))
    return vpt::set_error(VPT_E_INVALID, "vpt_gpu_tile_errors: needs a moment plane, an output array and abs_floor > 0");
  int rc = ctx_device(ctx);
  if (rc) return rc;
  if (ctx->open_feeds.load() > 0)  // (the call waits for its kernel, which would wait for the feed's launch)
    return vpt::set_error(VPT_E_STATE, "vpt_gpu_tile_errors: a feed of this context is open");
  uint32_t P = 1;
  while (P < ctx->scene.tile_area) P <<= 1;
  if (P > vpt::kTileErrorMaxP)
    return vpt::set_error(VPT_E_INVALID, "vpt_gpu_tile_errors: tiles of more than " + std::to_string(vpt::kTileErrorMaxP) +
                                             " pixels are not supported (the tree is reduced in LDS)");
  if ((rc = ensure_order(ctx))) return rc;  // (allocates the result buffer with the tile ranks)
  hipStream_t s = (hipStream_t)hip_stream;
  const uint32_t T = (uint32_t)ctx->scene.T;
  hipLaunchKernelGGL(vpt::vpt_tile_error_kernel, dim3(T), dim3(vpt::kTileErrorThreads), 2 * (size_t)P * sizeof(float), s,
                     ctx->scene_dev, film_device ? film_device : (const float*)ctx->film, m2_device, abs_floor, P,
                     ctx->tile_err);
  VPT_HIP(hipGetLastError());
  VPT_HIP(hipMemcpyAsync(err_T_host, ctx->tile_err, (size_t)T * sizeof(float), hipMemcpyDeviceToHost, s));
  VPT_HIP(hipStreamSynchronize(s));
  return VPT_OK;
}

int vpt_gpu_render_adaptive(vpt_gpu_ctx* ctx, const vpt_adaptive_params* p, float* film_device, float* m2_device,
                            uint32_t* waves_T_host, float* err_T_host, vpt_adaptive_result* out, void* hip_stream) {
  if (!ctx || !p || !m2_device || !waves_T_host || !err_T_host)
    return vpt::set_error(VPT_E_INVALID, "vpt_gpu_render_adaptive: null argument");
  if (p->min_waves < 2 || p->step_waves == 0 || p->max_waves < p->min_waves || !(p->target_error >= 0.0f) ||
      !(p->abs_floor > 0.0f))
    return vpt::set_error(VPT_E_INVALID, "vpt_gpu_render_adaptive: needs min_waves >= 2, step_waves >= 1, max_waves >= "
                                         "min_waves, target_error >= 0 and abs_floor > 0");
  int rc = ctx_device(ctx);
  if (rc) return rc;
  const uint32_t T = (uint32_t)ctx->scene.T;
  float* const film = film_device ? film_device : ctx->film;
  float* const prev = ctx->m2;
  if ((rc = vpt_gpu_set_film_moments(ctx, m2_device))) return rc;
  struct Restore {  // the previous attachment, on every return
    vpt_gpu_ctx* c;
    float* m2;
    ~Restore() { c->m2 = m2; }
  } restore{ctx, prev};
  vpt_adaptive_result res{};
  res.jobs_uniform = (uint64_t)p->max_waves * T;
  // Round 0: the first min_waves waves of every tile.
  if ((rc = vpt_gpu_render_tiles(ctx, 0, T, 0, p->min_waves, film, hip_stream))) return rc;
  std::fill(waves_T_host, waves_T_host + T, p->min_waves);
  res.rounds = 1;
  res.jobs_rendered = (uint64_t)p->min_waves * T;
  // Later rounds: the tiles still above the target and below the cap, all at the same wave count (a tile that
  // leaves the list never returns), get the next step_waves waves in one list launch.
  std::vector<uint32_t> list(T), next;
  for (uint32_t t = 0; t < T; ++t) list[t] = t;
  uint32_t done = p->min_waves;
  for (;;) {
    if ((rc = vpt_gpu_tile_errors(ctx, film, m2_device, p->abs_floor, err_T_host, hip_stream))) return rc;
    if (done >= p->max_waves) break;
    next.clear();
    const bool never = p->target_error == 0.0f;  // (no tile stops: black tiles, whose estimate is 0, neither)
    for (uint32_t t : list)
      if (never || err_T_host[t] > p->target_error) next.push_back(t);
    list.swap(next);
    if (list.empty()) break;
    const uint32_t step = std::min(p->step_waves, p->max_waves - done);
    if ((rc = vpt_gpu_render_tile_list(ctx, list.data(), (uint32_t)list.size(), done, step, film, hip_stream))) return rc;
    for (uint32_t t : list) waves_T_host[t] += step;
    done += step;
    ++res.rounds;
    res.jobs_rendered += (uint64_t)step * list.size();
  }
  for (uint32_t t = 0; t < T; ++t) {
    if (waves_T_host[t] >= p->max_waves) ++res.tiles_at_max;
    res.max_error = std::max(res.max_error, err_T_host[t]);
  }
  if (out) *out = res;
  return VPT_OK;
}

int vpt_gpu_render_adaptive_fused(vpt_gpu_ctx* ctx, const vpt_adaptive_params* p, float* film_device, float* m2_device,
                                  uint32_t* waves_T_host, float* err_T_host, vpt_adaptive_result* out, void* hip_stream) {
  if (!ctx || !p || !m2_device || !waves_T_host || !err_T_host)
    return vpt::set_error(VPT_E_INVALID, "vpt_gpu_render_adaptive_fused: null argument");
  if (p->min_waves < 2 || p->step_waves == 0 || p->max_waves < p->min_waves || !(p->target_error >= 0.0f) ||
      !(p->abs_floor > 0.0f))
    return vpt::set_error(VPT_E_INVALID, "vpt_gpu_render_adaptive_fused: needs min_waves >= 2, step_waves >= 1, max_waves "
                                         ">= min_waves, target_error >= 0 and abs_floor > 0");
  int rc = ctx_device(ctx);
  if (rc) return rc;
  if (!ctx->shutter.empty())
    return vpt::set_error(VPT_E_STATE, "vpt_gpu_render_adaptive_fused: a shutter is attached and gang launches do not honour "
                                       "it: detach it (vpt_gpu_set_shutter NULL, 0) or use vpt_gpu_render_adaptive");
  if (ctx->groups)
    return vpt::set_error(VPT_E_STATE, "vpt_gpu_render_adaptive_fused: light groups are attached and gang launches do not "
                                       "write them: detach them (vpt_gpu_set_light_groups NULL) or use vpt_gpu_render_adaptive");
  if (ctx->scene.pixel_mode)
    return vpt::set_error(VPT_E_INVALID, "vpt_gpu_render_adaptive_fused: gang launches run the reference RNG mode");
  if (ctx->scene.tile_area > vpt::kGangMaxArea)
    return vpt::set_error(VPT_E_INVALID, "vpt_gpu_render_adaptive_fused: tiles of more than " + std::to_string(vpt::kGangMaxArea) +
                                             " pixels are not supported (the error tree is held in registers); "
                                             "vpt_gpu_render_adaptive renders them");
  if (ctx->film_order != VPT_FILM_ORDERED)
    return vpt::set_error(VPT_E_STATE, "vpt_gpu_render_adaptive_fused: gang launches need the ordered film "
                                       "(vpt_gpu_set_film_order: VPT_FILM_ORDERED)");
  if (ctx->frame_waves)
    return vpt::set_error(VPT_E_STATE, "vpt_gpu_render_adaptive_fused: a frame is open (its launches add with film atomics)");
  if (ctx->open_feeds.load() > 0)  // (the call allocates and waits for its launch, which would wait for the feed's)
    return vpt::set_error(VPT_E_STATE, "vpt_gpu_render_adaptive_fused: a feed of this context is open");
  const uint32_t T = (uint32_t)ctx->scene.T;
  if (!ctx->volume_ok) return volume_gone();
  if ((rc = ensure_order(ctx))) return rc;  // (the tile ranks; allocates tile_err with them)
  // The full resident grid of the throughput kernel; every wavefront has a scratch slot of one group's samples.
  const uint32_t blocks = (uint32_t)ctx->grid_blocks;
  const uint64_t bytes = (uint64_t)blocks * vpt::kBlockThreads * ctx->scene.tile_area * 3 * sizeof(float);
  if (ctx->gang_scratch_bytes < bytes) {
    (void)hipFree(ctx->gang_scratch);
    ctx->gang_scratch = nullptr;
    ctx->gang_scratch_bytes = 0;
    const hipError_t e = hipMalloc((void**)&ctx->gang_scratch, bytes);
    if (e != hipSuccess) {
      ctx->gang_scratch = nullptr;
      (void)hipGetLastError();
      return vpt::set_error(VPT_E_NOMEM, "vpt_gpu_render_adaptive_fused: " + std::to_string(bytes >> 20) +
                                             " MiB of wavefront scratch: " + hipGetErrorString(e));
    }
    ctx->gang_scratch_bytes = bytes;
  }
  if (!ctx->gang_waves) VPT_HIP(hipMalloc((void**)&ctx->gang_waves, (size_t)T * sizeof(uint32_t)));
  if (!ctx->tile_err) return vpt::set_error(VPT_E_NOMEM, "vpt_gpu_render_adaptive_fused: no tile-error buffer (its allocation failed)");
  hipStream_t s = (hipStream_t)hip_stream;
  vpt::KernelArgs env{};
  env.jid_begin = 0;
  env.jid_count = T;  // (work items: the tiles)
  env.pixel_chunk = 1;
  env.film = film_device ? film_device : ctx->film;
  env.tile_area = ctx->scene.tw * ctx->scene.th;
  env.prof_buf = ctx->prof;
  env.order = ctx->order;
  env.order_group = 1;
  env.gang_scratch = ctx->gang_scratch;
  env.gang_m2 = m2_device;  // (the context's attachment is neither used nor changed)
  env.gang_waves = ctx->gang_waves;
  env.gang_err = ctx->tile_err;
  env.gang_target = p->target_error;
  env.gang_floor = p->abs_floor;
  env.gang_min = p->min_waves;
  env.gang_step = p->step_waves;
  env.gang_max = p->max_waves;
  uint32_t slot = 0;
  if ((rc = take_slot(ctx, s, slot))) return rc;
  env.job_counter = ctx->job_counter + 2 * slot;
  env.event_count = ctx->job_counter + 2 * slot + 1;
  vpt::KernelVariant gang = vpt::base_variant(ctx->scene.has_temperature != 0, ctx->use_runs);
  gang.gang = true;
  if ((rc = launch_integrate(ctx, gang, blocks, 0, s, env, ctx->scene_full_dev))) return rc;
  ++ctx->ordered_launches;
  VPT_HIP(hipMemcpyAsync(waves_T_host, ctx->gang_waves, (size_t)T * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
  VPT_HIP(hipMemcpyAsync(err_T_host, ctx->tile_err, (size_t)T * sizeof(float), hipMemcpyDeviceToHost, s));
  if ((rc = release_slot(ctx, s, slot))) return rc;
  VPT_HIP(hipStreamSynchronize(s));
  vpt_adaptive_result res{};
  res.jobs_uniform = (uint64_t)p->max_waves * T;
  uint32_t longest = p->min_waves;
  for (uint32_t t = 0; t < T; ++t) {
    res.jobs_rendered += waves_T_host[t];
    longest = std::max(longest, waves_T_host[t]);
    if (waves_T_host[t] >= p->max_waves) ++res.tiles_at_max;
    res.max_error = std::max(res.max_error, err_T_host[t]);
  }
  // round 0 and the later boundaries the longest-running tile crossed: the rounds driver's count
  res.rounds = 1 + (uint32_t)(((uint64_t)(longest - p->min_waves) + p->step_waves - 1) / p->step_waves);
  if (out) *out = res;
  return VPT_OK;
}

int vpt_gpu_render_jobs_records(vpt_gpu_ctx* ctx, uint64_t jid_begin, uint64_t jid_count, float* film_device,
                                float* records_device, void* hip_stream) {
  return render(ctx, jid_begin, jid_count, film_device, records_device, hip_stream);
}

int vpt_gpu_trace_jobs(vpt_gpu_ctx* ctx, uint64_t jid_begin, uint64_t jid_count, float* film_device,
                       vpt_event* events_device, uint64_t capacity, uint64_t* count, void* hip_stream) {
  if (!ctx || !events_device || !count) return vpt::set_error(VPT_E_INVALID, "vpt_gpu_trace_jobs: null argument");
  *count = 0;
  uint32_t slot = 0;
  int rc = render(ctx, jid_begin, jid_count, film_device, nullptr, hip_stream, events_device, capacity, &slot);
  if (rc) return rc;
  if (jid_count == 0) return VPT_OK;
  unsigned long long n = 0;
  VPT_HIP(hipMemcpyAsync(&n, ctx->job_counter + 2 * slot + 1, sizeof n, hipMemcpyDeviceToHost, (hipStream_t)hip_stream));
  VPT_HIP(hipStreamSynchronize((hipStream_t)hip_stream));
  *count = n;
  return VPT_OK;
}

int vpt_gpu_majorant_trace(vpt_gpu_ctx* ctx, const float origin[3], const float direction[3], float* rows_host,
                           int max_rows, int* n_rows) {
  if (!ctx || !origin || !direction || !n_rows || (max_rows > 0 && !rows_host) || max_rows < 0)
    return vpt::set_error(VPT_E_INVALID, "vpt_gpu_majorant_trace: bad argument");
  int rc = ctx_device(ctx);
  if (rc) return rc;
  if (!ctx->volume_ok) return volume_gone();
  float* rows = nullptr;
  int* n = nullptr;
  VPT_HIP(hipMalloc((void**)&rows, (size_t)(max_rows > 0 ? max_rows : 1) * 9 * sizeof(float)));
  if (hipMalloc((void**)&n, sizeof(int)) != hipSuccess) {
    (void)hipFree(rows);
    return vpt::set_error(VPT_E_HIP, "vpt_gpu_majorant_trace: hipMalloc failed");
  }
  hipLaunchKernelGGL(vpt::vpt_majorant_trace_kernel, dim3(1), dim3(64), 0, nullptr, ctx->scene_dev, origin[0],
                     origin[1], origin[2], direction[0], direction[1], direction[2], rows, max_rows, n);
  hipError_t e = hipGetLastError();
  int nn = 0;
  if (e == hipSuccess) e = hipMemcpy(&nn, n, sizeof nn, hipMemcpyDeviceToHost);
  if (e == hipSuccess && max_rows > 0)
    e = hipMemcpy(rows_host, rows, (size_t)std::min(nn, max_rows) * 9 * sizeof(float), hipMemcpyDeviceToHost);
  (void)hipFree(rows);
  (void)hipFree(n);
  if (e != hipSuccess) return vpt::set_error(VPT_E_HIP, std::string("vpt_gpu_majorant_trace: ") + hipGetErrorString(e));
  *n_rows = nn;
  return VPT_OK;
}

int vpt_gpu_set_rng_mode(vpt_gpu_ctx* ctx, int mode) {
  if (!ctx || (mode != VPT_RNG_REFERENCE && mode != VPT_RNG_PIXEL))
    return vpt::set_error(VPT_E_INVALID, "vpt_gpu_set_rng_mode: bad argument");
  int rc = ctx_device(ctx);
  if (rc) return rc;
  if (mode == VPT_RNG_PIXEL && (int64_t)ctx->scene.tw * ctx->scene.th >= (int64_t)vpt::kPixelTaken)
    return vpt::set_error(VPT_E_INVALID, "vpt_gpu_set_rng_mode: tile too large for the pixel mode");
  ctx->scene.pixel_mode = mode == VPT_RNG_PIXEL ? 1 : 0;
  ctx->scene.tile_area = (uint32_t)(ctx->scene.tw * ctx->scene.th);
  return push_scene(ctx);
}

int vpt_gpu_set_pixel_chunk(vpt_gpu_ctx* ctx, int chunk) {
  if (!ctx || chunk < 0 || (chunk & (chunk - 1)) != 0 || (chunk > 0 && ctx->scene.tile_area % (uint32_t)chunk != 0))
    return vpt::set_error(VPT_E_INVALID, "vpt_gpu_set_pixel_chunk: 0 or a power of two dividing the tile area");
  ctx->pixel_chunk = chunk;  // read by the next render's host code only: no wait
  return VPT_OK;
}

int vpt_gpu_set_run_skipping(vpt_gpu_ctx* ctx, int mode) {
  if (!ctx || mode < -1 || mode > 1) return vpt::set_error(VPT_E_INVALID, "vpt_gpu_set_run_skipping: bad argument");
  if (mode == 1 && ctx->scene.has_temperature)
    return vpt::set_error(VPT_E_INVALID, "vpt_gpu_set_run_skipping: no run-skipping variant with a temperature grid");
  ctx->runs_mode = mode;  // (kept: vpt_gpu_set_grids re-derives "auto" from the new grid, a forced choice stays)
  ctx->use_runs = mode < 0 ? auto_run_skipping(ctx) : mode == 1;
  return VPT_OK;
}

int vpt_gpu_kernel_variant(const vpt_gpu_ctx* ctx, int* has_temperature, int* run_skipping) {
  if (!ctx) return vpt::set_error(VPT_E_INVALID, "null context");
  if (has_temperature) *has_temperature = ctx->scene.has_temperature ? 1 : 0;
  if (run_skipping) *run_skipping = ctx->use_runs ? 1 : 0;
  return VPT_OK;
}

int vpt_gpu_last_launch_variant(const vpt_gpu_ctx* ctx, int* eval_split) {
  if (!ctx) return vpt::set_error(VPT_E_INVALID, "null context");
  if (eval_split) *eval_split = ctx->last_eval_split;
  return VPT_OK;
}

int vpt_gpu_set_pool_layout(vpt_gpu_ctx* ctx, int layout) {
  if (!ctx || layout < VPT_POOL_SPARSE || layout > VPT_POOL_AUTO)
    return vpt::set_error(VPT_E_INVALID, "vpt_gpu_set_pool_layout: bad argument");
  if (ctx->open_feeds.load() > 0) return vpt::set_error(VPT_E_STATE, "vpt_gpu_set_pool_layout: a feed of this context is open");
  if (ctx->frame_waves) return vpt::set_error(VPT_E_STATE, "vpt_gpu_set_pool_layout: a frame is open");
  int rc = ctx_device(ctx);
  if (rc) return rc;
  if ((rc = wait_ctx(ctx))) return rc;  // (launches in flight read the pool about to change)
  VPT_HIP(hipDeviceSynchronize());      // (launches on the caller's streams and the null stream too)
  ctx->pool_policy = layout;
  rc = apply_pool_layout(ctx, layout);
  const int prc = push_scene(ctx);
  return rc ? rc : prc;
}

int vpt_gpu_set_pool_cap(vpt_gpu_ctx* ctx, uint64_t max_bytes) {
  if (!ctx) return vpt::set_error(VPT_E_INVALID, "vpt_gpu_set_pool_cap: null context");
  ctx->pool_cap = max_bytes;
  return VPT_OK;
}

int vpt_gpu_pool_info(const vpt_gpu_ctx* ctx, int* layout, int* policy, uint64_t* sparse_bytes, uint64_t* dense_bytes,
                      double* expand_ms) {
  if (!ctx) return vpt::set_error(VPT_E_INVALID, "null context");
  if (layout) *layout = ctx->density.dense ? VPT_POOL_DENSE : VPT_POOL_SPARSE;
  if (policy) *policy = ctx->pool_policy;
  if (sparse_bytes) sparse_bytes[0] = ctx->density.brick_bytes, sparse_bytes[1] = ctx->temperature.brick_bytes;
  if (dense_bytes) dense_bytes[0] = ctx->density.dense_bytes, dense_bytes[1] = ctx->temperature.dense_bytes;
  if (expand_ms) *expand_ms = ctx->pool_expand_ms;
  return VPT_OK;
}

int vpt_gpu_debug_read_pool(vpt_gpu_ctx* ctx, int grid, uint64_t cell_begin, uint64_t cell_count, float* out) {
  if (!ctx || !out || grid < 0 || grid > 1) return vpt::set_error(VPT_E_INVALID, "vpt_gpu_debug_read_pool: bad argument");
  const vpt::DeviceGrid& d = grid ? ctx->temperature : ctx->density;
  if (!d.dense) return vpt::set_error(VPT_E_STATE, "vpt_gpu_debug_read_pool: the grid has no dense pool");
  const uint64_t brick = vpt::kBrickVox * sizeof(float), cells = d.dense_bytes / brick;
  if (cell_begin > cells || cell_count > cells - cell_begin)
    return vpt::set_error(VPT_E_INVALID, "vpt_gpu_debug_read_pool: cells outside the table");
  int rc = ctx_device(ctx);
  if (rc) return rc;
  if (cell_count) VPT_HIP(hipMemcpy(out, (const char*)d.dense + cell_begin * brick, cell_count * brick, hipMemcpyDeviceToHost));
  return VPT_OK;
}

int vpt_gpu_set_film_order(vpt_gpu_ctx* ctx, int mode, uint64_t max_bytes) {
  if (!ctx || (mode != VPT_FILM_ATOMIC && mode != VPT_FILM_ORDERED))
    return vpt::set_error(VPT_E_INVALID, "vpt_gpu_set_film_order: bad argument");
  int rc = ctx_device(ctx);
  if (rc) return rc;
  ctx->film_order = mode;
  ctx->film_order_max = max_bytes;
  if (mode == VPT_FILM_ATOMIC && ctx->samples && ctx->open_feeds.load() == 0) {  // the buffer is not needed
    if (ctx->samples_used) VPT_HIP(hipEventSynchronize(ctx->samples_done));
    (void)hipFree(ctx->samples);
    ctx->samples = nullptr;
    ctx->samples_bytes = 0;
  }
  return VPT_OK;
}

int vpt_gpu_film_order_info(const vpt_gpu_ctx* ctx, int* mode, uint64_t* buffer_bytes, uint64_t* ordered_launches,
                            uint64_t* atomic_launches) {
  if (!ctx) return vpt::set_error(VPT_E_INVALID, "null context");
  if (mode) *mode = ctx->film_order;
  if (buffer_bytes) *buffer_bytes = ctx->samples_bytes;
  if (ordered_launches) *ordered_launches = ctx->ordered_launches;
  if (atomic_launches) *atomic_launches = ctx->atomic_launches;
  return VPT_OK;
}

int vpt_gpu_set_job_order(vpt_gpu_ctx* ctx, int mode) {
  if (!ctx || mode < VPT_ORDER_JID || mode > VPT_ORDER_COST_SAME_TILE)
    return vpt::set_error(VPT_E_INVALID, "vpt_gpu_set_job_order: bad argument");
  ctx->order_mode = mode;
  return VPT_OK;
}

int vpt_gpu_set_job_order_tail(vpt_gpu_ctx* ctx, int waves) {
  if (!ctx || waves < 0) return vpt::set_error(VPT_E_INVALID, "vpt_gpu_set_job_order_tail: bad argument");
  ctx->order_tail_waves = waves;
  return VPT_OK;
}

int vpt_gpu_tile_costs(vpt_gpu_ctx* ctx, float* cost, uint32_t* rank) {
  if (!ctx) return vpt::set_error(VPT_E_INVALID, "null context");
  int rc = ctx_device(ctx);
  if (rc) return rc;
  if ((rc = ensure_order(ctx))) return rc;
  if (cost) std::memcpy(cost, ctx->tile_cost.data(), ctx->tile_cost.size() * sizeof(float));
  if (rank) std::memcpy(rank, ctx->tile_rank.data(), ctx->tile_rank.size() * sizeof(uint32_t));
  return VPT_OK;
}

int vpt_gpu_set_tile_costs(vpt_gpu_ctx* ctx, const float* cost) {
  if (!ctx || !cost) return vpt::set_error(VPT_E_INVALID, "vpt_gpu_set_tile_costs: null argument");
  int rc = ctx_device(ctx);
  if (rc) return rc;
  if (!ctx->volume_ok) return volume_gone();  // (costs describe a scene, and there is none to render)
  for (uint64_t i = 0; i < ctx->scene.T; ++i)  // NaN would break the sort's strict weak ordering
    if (!std::isfinite(cost[i])) return vpt::set_error(VPT_E_INVALID, "vpt_gpu_set_tile_costs: non-finite cost");
  if ((rc = wait_ctx(ctx))) return rc;  // in-flight launches read the current order
  ctx->tile_cost.assign(cost, cost + ctx->scene.T);
  return rank_tiles(ctx);
}

int vpt_gpu_set_job_permutation(vpt_gpu_ctx* ctx, const uint32_t* perm, uint64_t n) {
  if (!ctx || (n && !perm)) return vpt::set_error(VPT_E_INVALID, "vpt_gpu_set_job_permutation: null argument");
  if (n >= (1ULL << 32)) return vpt::set_error(VPT_E_INVALID, "vpt_gpu_set_job_permutation: too many jobs");
  int rc = ctx_device(ctx);
  if (rc) return rc;
  std::vector<uint8_t> seen(n, 0);
  for (uint64_t i = 0; i < n; ++i) {
    if (perm[i] >= n || seen[perm[i]]) return vpt::set_error(VPT_E_INVALID, "vpt_gpu_set_job_permutation: not a permutation");
    seen[perm[i]] = 1;
  }
  if ((rc = wait_ctx(ctx))) return rc;  // in-flight launches may read the current one
  (void)hipFree(ctx->perm);
  ctx->perm = nullptr;
  ctx->perm_n = 0;
  if (n == 0) return VPT_OK;
  VPT_HIP(hipMalloc((void**)&ctx->perm, n * sizeof(uint32_t)));
  VPT_HIP(hipMemcpy(ctx->perm, perm, n * sizeof(uint32_t), hipMemcpyHostToDevice));
  ctx->perm_n = n;
  return VPT_OK;
}

int vpt_gpu_job_permutation_info(const vpt_gpu_ctx* ctx, uint64_t* n) {
  if (!ctx || !n) return vpt::set_error(VPT_E_INVALID, "vpt_gpu_job_permutation_info: null argument");
  *n = ctx->perm ? ctx->perm_n : 0;
  return VPT_OK;
}

int vpt_gpu_debug_fail_upload(vpt_gpu_ctx* ctx, int nth) {
  if (!ctx || nth < 0) return vpt::set_error(VPT_E_INVALID, "vpt_gpu_debug_fail_upload: bad argument");
  ctx->debug_fail_upload = nth;
  return VPT_OK;
}

int vpt_gpu_sync(vpt_gpu_ctx* ctx) {
  if (!ctx) return vpt::set_error(VPT_E_INVALID, "null context");
  int rc = ctx_device(ctx);
  if (rc) return rc;
  return wait_ctx(ctx);
}

int vpt_gpu_stream_create(vpt_gpu_ctx* ctx, void** hip_stream) {
  if (!ctx || !hip_stream) return vpt::set_error(VPT_E_INVALID, "vpt_gpu_stream_create: null argument");
  int rc = ctx_device(ctx);
  if (rc) return rc;
  hipStream_t s = nullptr;
  VPT_HIP(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
  *hip_stream = s;
  return VPT_OK;
}

int vpt_gpu_bind_thread_near(vpt_gpu_ctx* ctx, int* node_out) {
  if (node_out) *node_out = -1;
  if (!ctx) return vpt::set_error(VPT_E_INVALID, "vpt_gpu_bind_thread_near: null context");
  char bus[64] = {};
  if (hipDeviceGetPCIBusId(bus, (int)sizeof bus, ctx->device) != hipSuccess) return VPT_OK;
  for (char* c = bus; *c; ++c) *c = (char)std::tolower((unsigned char)*c);
  int node = -1;
  {
    std::ifstream in(std::string("/sys/bus/pci/devices/") + bus + "/numa_node");
    if (!(in >> node) || node < 0) return VPT_OK;
  }
  std::ifstream in("/sys/devices/system/node/node" + std::to_string(node) + "/cpulist");
  std::string list;
  if (!std::getline(in, list)) return VPT_OK;
  // Allowed: the process's CPUs (its main thread's set: taskset / numactl restrict it), not this thread's own --
  // a thread inherits its creator's set, and a caller bound to the far node would otherwise pin its helpers
  // there too (r05n: a taker on node 1 made the pusher it started run there).
  cpu_set_t cur, near;
  CPU_ZERO(&near);
  if (sched_getaffinity(getpid(), sizeof cur, &cur) != 0) return VPT_OK;
  // "0-63,128-191"
  for (size_t pos = 0; pos < list.size();) {
    size_t end = list.find(',', pos);
    if (end == std::string::npos) end = list.size();
    const std::string r = list.substr(pos, end - pos);
    const size_t dash = r.find('-');
    const int a = std::atoi(r.c_str()), b = dash == std::string::npos ? a : std::atoi(r.c_str() + dash + 1);
    for (int c = a; c <= b && c < CPU_SETSIZE; ++c)
      if (c >= 0 && CPU_ISSET(c, &cur)) CPU_SET(c, &near);
    pos = end + 1;
  }
  if (CPU_COUNT(&near) == 0) return VPT_OK;
  if (pthread_setaffinity_np(pthread_self(), sizeof near, &near) != 0) return VPT_OK;
  if (node_out) *node_out = node;
  return VPT_OK;
}

int vpt_gpu_stream_destroy(vpt_gpu_ctx* ctx, void* hip_stream) {
  if (!ctx || !hip_stream) return vpt::set_error(VPT_E_INVALID, "vpt_gpu_stream_destroy: null argument");
  int rc = ctx_device(ctx);
  if (rc) return rc;
  VPT_HIP(hipStreamDestroy((hipStream_t)hip_stream));
  return VPT_OK;
}

int vpt_gpu_stream_sync(vpt_gpu_ctx* ctx, void* hip_stream) {
  if (!ctx) return vpt::set_error(VPT_E_INVALID, "vpt_gpu_stream_sync: null context");
  int rc = ctx_device(ctx);
  if (rc) return rc;
  VPT_HIP(hipStreamSynchronize((hipStream_t)hip_stream));
  return VPT_OK;
}

int vpt_gpu_film_alloc(vpt_gpu_ctx* ctx, float** film_device) {
  if (!ctx || !film_device) return vpt::set_error(VPT_E_INVALID, "vpt_gpu_film_alloc: null argument");
  int rc = ctx_device(ctx);
  if (rc) return rc;
  float* f = nullptr;
  VPT_HIP(hipMalloc((void**)&f, ctx->film_count * sizeof(float)));
  const hipError_t e = hipMemset(f, 0, ctx->film_count * sizeof(float));
  if (e != hipSuccess) {
    (void)hipFree(f);
    return vpt::set_error(VPT_E_HIP, std::string("vpt_gpu_film_alloc: ") + hipGetErrorString(e));
  }
  *film_device = f;
  return VPT_OK;
}

int vpt_gpu_film_free(vpt_gpu_ctx* ctx, float* film_device) {
  if (!ctx || !film_device || film_device == ctx->film)
    return vpt::set_error(VPT_E_INVALID, "vpt_gpu_film_free: not a film from vpt_gpu_film_alloc");
  int rc = ctx_device(ctx);
  if (rc) return rc;
  VPT_HIP(hipFree(film_device));
  return VPT_OK;
}

// The largest ordered-frame buffer (the 4K, 1 024-spp C5 frame on one GPU needs 102 GB).
constexpr uint64_t kFrameMaxBytes = 128ULL << 30;

int vpt_gpu_frame_open(vpt_gpu_ctx* ctx, uint64_t jid_lo, uint64_t* waves_io, uint32_t tile_lo, uint32_t tile_hi) {
  if (!ctx || !waves_io) return vpt::set_error(VPT_E_INVALID, "vpt_gpu_frame_open: null argument");
  uint64_t waves = *waves_io;
  *waves_io = 0;
  int rc = ctx_device(ctx);
  if (rc) return rc;
  if (ctx->open_feeds.load() > 0)  // (allocating could wait for a running feed's launch)
    return vpt::set_error(VPT_E_STATE, "vpt_gpu_frame_open: a feed of the context is open");
  const vpt::DevScene& S = ctx->scene;
  if (S.pixel_mode) return vpt::set_error(VPT_E_INVALID, "vpt_gpu_frame_open: frames run the reference RNG mode");
  ctx->frame_waves = 0;
  if (waves == 0) return VPT_OK;
  if (!ctx->shutter.empty())
    return vpt::set_error(VPT_E_STATE, "vpt_gpu_frame_open: a shutter is attached and a frame's feeds render the scene's "
                                       "camera: detach it (vpt_gpu_set_shutter NULL, 0)");
  if (tile_lo >= tile_hi || tile_hi > S.T) return vpt::set_error(VPT_E_INVALID, "vpt_gpu_frame_open: bad tile range");
  const uint64_t per_wave = (uint64_t)(tile_hi - tile_lo) * (uint64_t)S.tile_area * 3 * sizeof(float);
  // as many of the waves asked for as fit 3/4 of the device's free memory (the buffer already held counted in), at
  // most kFrameMaxBytes
  size_t free_b = 0, total_b = 0;
  VPT_HIP(hipMemGetInfo(&free_b, &total_b));
  const uint64_t avail = std::min<uint64_t>(kFrameMaxBytes, (uint64_t)free_b / 4 * 3 + ctx->samples_bytes);
  waves = std::min<uint64_t>(waves, avail / per_wave);
  if (waves == 0) return vpt::set_error(VPT_E_NOMEM, "vpt_gpu_frame_open: not one wave of the frame fits the device");
  if (ctx->samples_used) VPT_HIP(hipEventSynchronize(ctx->samples_done));  // (an ordered launch's film pass)
  float* buf = nullptr;
  if ((rc = ensure_samples(ctx, waves * per_wave, buf))) return rc;
  if (!buf) return vpt::set_error(VPT_E_STATE, "vpt_gpu_frame_open: the sample buffer cannot grow now");
  if (!ctx->frame_film) VPT_HIP(hipMalloc((void**)&ctx->frame_film, ctx->film_count * sizeof(float)));
  if (!ctx->staging) VPT_HIP(hipHostMalloc((void**)&ctx->staging, ctx->film_count * sizeof(float), hipHostMallocDefault));
  ctx->frame_jid_lo = jid_lo;
  ctx->frame_tile_lo = tile_lo;
  ctx->frame_tiles = tile_hi - tile_lo;
  ctx->frame_waves = waves;
  *waves_io = waves;
  return VPT_OK;
}

int vpt_gpu_frame_finish(vpt_gpu_ctx* ctx, uint64_t jid_end, const float* prior, float* film_host) {
  if (!ctx || !film_host) return vpt::set_error(VPT_E_INVALID, "vpt_gpu_frame_finish: null argument");
  int rc = ctx_device(ctx);
  if (rc) return rc;
  const uint64_t waves = ctx->frame_waves, lo = ctx->frame_jid_lo;
  if (!waves) return VPT_OK;  // no frame open
  ctx->frame_waves = 0;       // (closed, whatever follows)
  const vpt::DevScene& S = ctx->scene;
  const uint64_t w0 = lo / S.T;
  if (jid_end < lo || (jid_end > lo && (jid_end - 1) / S.T - w0 >= waves))
    return vpt::set_error(VPT_E_INVALID, "vpt_gpu_frame_finish: jobs beyond the frame's waves");
  if (ctx->open_feeds.load() > 0) return vpt::set_error(VPT_E_STATE, "vpt_gpu_frame_finish: a feed of the context is open");
  if (jid_end == lo) return VPT_OK;
  const size_t bytes = ctx->film_count * sizeof(float);
  if (prior)
    VPT_HIP(hipMemcpyAsync(ctx->frame_film, prior, bytes, hipMemcpyHostToDevice, ctx->stream));
  else
    VPT_HIP(hipMemsetAsync(ctx->frame_film, 0, bytes, ctx->stream));
  const uint32_t tile_lo = ctx->frame_tile_lo, tiles = ctx->frame_tiles, tile_hi = tile_lo + tiles;
  const uint64_t threads = (uint64_t)tiles * (uint64_t)S.tile_area;
  hipLaunchKernelGGL(vpt::vpt_frame_order_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, ctx->stream,
                     ctx->scene_dev, ctx->frame_film, ctx->samples, w0, tile_lo, tiles, lo, jid_end);
  VPT_HIP(hipGetLastError());
  VPT_HIP(hipEventRecord(ctx->samples_done, ctx->stream));  // (the next ordered launch waits for this pass)
  ctx->samples_used = true;
  VPT_HIP(hipMemcpyAsync(ctx->staging, ctx->frame_film, bytes, hipMemcpyDeviceToHost, ctx->stream));
  VPT_HIP(hipStreamSynchronize(ctx->stream));
  // the tiles' pixels into the host film, one contiguous run per image row and tile row (tiles are row-major)
  const uint64_t W = (uint64_t)S.W;
  auto put = [&](uint64_t y, uint64_t x0, uint64_t x1) {
    std::memcpy(film_host + (y * W + x0) * 4, ctx->staging + (y * W + x0) * 4, (x1 - x0) * 4 * sizeof(float));
  };
  if (S.single_pixel_enabled) {  // only that pixel has samples (worker.cpp:113-116)
    if (S.sp_x >= 0 && S.sp_y >= 0 && S.sp_x < S.W && S.sp_y < S.H) {
      const uint64_t t = (uint64_t)(S.sp_y / S.th) * S.ntx + (uint64_t)(S.sp_x / S.tw);
      if (t >= tile_lo && t < tile_hi) put((uint64_t)S.sp_y, (uint64_t)S.sp_x, (uint64_t)S.sp_x + 1);
    }
    return VPT_OK;
  }
  // image row y's run of the band: the band's tiles in tile row y / th (tiles are row-major)
  const uint64_t ntx = (uint64_t)S.ntx, y0 = tile_lo / ntx * (uint64_t)S.th,
                 y1 = std::min<uint64_t>((tile_hi + ntx - 1) / ntx * (uint64_t)S.th, (uint64_t)S.H);
  auto rows = [&](uint64_t ya, uint64_t yb) {
    for (uint64_t y = ya; y < yb; ++y) {
      const uint64_t ty = y / (uint64_t)S.th;
      const uint64_t a = std::max<uint64_t>(tile_lo, ty * ntx) - ty * ntx, b = std::min<uint64_t>(tile_hi, (ty + 1) * ntx) - ty * ntx;
      if (a < b) put(y, a * (uint64_t)S.tw, std::min<uint64_t>(b * (uint64_t)S.tw, W));
    }
  };
  const uint64_t nt = (y1 - y0) * W < (1u << 18) ? 1 : 8;  // (a 1080p film: 33 MB, copied by 8 threads)
  std::vector<std::thread> pool;
  for (uint64_t i = 1; i < nt; ++i) pool.emplace_back(rows, y0 + (y1 - y0) * i / nt, y0 + (y1 - y0) * (i + 1) / nt);
  rows(y0, y0 + (y1 - y0) / nt);
  for (auto& t : pool) t.join();
  return VPT_OK;
}

int vpt_gpu_film_flush_to_host(vpt_gpu_ctx* ctx, float* film_device, float* film_host) {
  if (!ctx || !film_host) return vpt::set_error(VPT_E_INVALID, "vpt_gpu_film_flush_to_host: null argument");
  int rc = ctx_device(ctx);
  if (rc) return rc;
  float* f = film_device ? film_device : ctx->film;
  const size_t bytes = ctx->film_count * sizeof(float);
  if (!ctx->staging) VPT_HIP(hipHostMalloc((void**)&ctx->staging, bytes, hipHostMallocDefault));
  VPT_HIP(hipMemcpyAsync(ctx->staging, f, bytes, hipMemcpyDeviceToHost, ctx->stream));
  VPT_HIP(hipMemsetAsync(f, 0, bytes, ctx->stream));
  VPT_HIP(hipStreamSynchronize(ctx->stream));
  const float* src = ctx->staging;
  for (uint64_t i = 0; i < ctx->film_count; ++i) film_host[i] += src[i];
  return VPT_OK;
}

}  // extern "C"

namespace {
// The setters' conventions for one gate set (gate_min, gate_idle, gate_eval, gate_walk): gate_min and gate_eval
// <= 0, gate_idle and gate_walk < 0 keep the value (gate_idle 0 is rejected by the callers).
void apply_gates(int g[4], int gate_min, int gate_idle, int gate_eval, int gate_walk) {
  if (gate_min > 0) g[0] = gate_min;
  if (gate_idle >= 0) g[1] = gate_idle;
  if (gate_eval > 0) g[2] = gate_eval;
  if (gate_walk >= 0) g[3] = gate_walk;
}
}  // namespace

extern "C" {

int vpt_gpu_film_clear(vpt_gpu_ctx* ctx) {
  if (!ctx) return vpt::set_error(VPT_E_INVALID, "null context");
  int rc = ctx_device(ctx);
  if (rc) return rc;
  if ((rc = wait_ctx(ctx))) return rc;  // renders into the film may be in flight on any stream
  VPT_HIP(hipMemsetAsync(ctx->film, 0, ctx->film_count * sizeof(float), ctx->stream));
  VPT_HIP(hipStreamSynchronize(ctx->stream));
  return VPT_OK;
}

int vpt_gpu_film_device_ptr(vpt_gpu_ctx* ctx, float** film_device, uint64_t* count) {
  if (!ctx) return vpt::set_error(VPT_E_INVALID, "null context");
  if (film_device) *film_device = ctx->film;
  if (count) *count = ctx->film_count;
  return VPT_OK;
}

int vpt_gpu_film_add_to_host(vpt_gpu_ctx* ctx, float* film_host) {
  if (!ctx || !film_host) return vpt::set_error(VPT_E_INVALID, "null argument");
  int rc = ctx_device(ctx);
  if (rc) return rc;
  if ((rc = wait_ctx(ctx))) return rc;
  std::vector<float> tmp(ctx->film_count);
  VPT_HIP(hipMemcpy(tmp.data(), ctx->film, ctx->film_count * sizeof(float), hipMemcpyDeviceToHost));
  for (uint64_t i = 0; i < ctx->film_count; ++i) film_host[i] += tmp[i];
  return VPT_OK;
}

int vpt_gpu_counters(vpt_gpu_ctx* ctx, vpt_counters* out, int reset) {
  if (!ctx || !out) return vpt::set_error(VPT_E_INVALID, "null argument");
  int rc = ctx_device(ctx);
  if (rc) return rc;
  if ((rc = wait_ctx(ctx))) return rc;
  unsigned long long c[vpt::kCounterCount];
  VPT_HIP(hipMemcpy(c, ctx->counters, sizeof c, hipMemcpyDeviceToHost));
  uint64_t* o = reinterpret_cast<uint64_t*>(out);
  for (int i = 0; i < vpt::kCounterCount; ++i) o[i] = c[i];
  if (reset) VPT_HIP(hipMemset(ctx->counters, 0, sizeof c));
  return VPT_OK;
}

int vpt_gpu_set_tuning(vpt_gpu_ctx* ctx, int gate_min, int gate_idle, int grid_blocks, int gate_eval, int gate_walk) {
  if (!ctx) return vpt::set_error(VPT_E_INVALID, "null context");
  int rc = ctx_device(ctx);
  if (rc) return rc;
  // gate_idle >= 1 is what guarantees progress: with no lane walking, every waiting block runs.
  if (gate_idle == 0) return vpt::set_error(VPT_E_INVALID, "gate_idle must be >= 1 (0 can stall a wavefront)");
  int own[4] = {ctx->scene.gate_min, ctx->scene.gate_idle, ctx->scene.gate_eval, ctx->scene.gate_walk};
  apply_gates(own, gate_min, gate_idle, gate_eval, gate_walk);
  ctx->scene.gate_min = own[0];
  ctx->scene.gate_idle = own[1];
  ctx->scene.gate_eval = own[2];
  ctx->scene.gate_walk = own[3];
  // (the full-launch set follows: existing callers tune every launch of the throughput kernel with this call)
  apply_gates(ctx->full_gate, gate_min, gate_idle, gate_eval, gate_walk);
  if ((rc = push_scene(ctx))) return rc;
  if (grid_blocks > 0) {
    ctx->grid_blocks = grid_blocks;
    ctx->grid_user = true;
  }
  return VPT_OK;
}

int vpt_gpu_set_latency_tuning(vpt_gpu_ctx* ctx, int wave_lanes, int gate_min, int gate_idle, int gate_eval,
                               int gate_walk) {
  if (!ctx) return vpt::set_error(VPT_E_INVALID, "null context");
  if (wave_lanes > 64) return vpt::set_error(VPT_E_INVALID, "wave_lanes must be <= 64");
  if (gate_idle == 0) return vpt::set_error(VPT_E_INVALID, "gate_idle must be >= 1 (0 can stall a wavefront)");
  int rc = ctx_device(ctx);
  if (rc) return rc;
  if (wave_lanes >= 0) ctx->lat_wave_lanes = wave_lanes;
  apply_gates(ctx->lat_gate, gate_min, gate_idle, gate_eval, gate_walk);
  return push_scene(ctx);
}

int vpt_gpu_set_full_tuning(vpt_gpu_ctx* ctx, int gate_min, int gate_idle, int gate_eval, int gate_walk) {
  if (!ctx) return vpt::set_error(VPT_E_INVALID, "null context");
  if (gate_idle == 0) return vpt::set_error(VPT_E_INVALID, "gate_idle must be >= 1 (0 can stall a wavefront)");
  int rc = ctx_device(ctx);
  if (rc) return rc;
  apply_gates(ctx->full_gate, gate_min, gate_idle, gate_eval, gate_walk);
  return push_scene(ctx);
}

int vpt_gpu_gate_info(const vpt_gpu_ctx* ctx, int set, int* gates, int* last_launch_set) {
  if (!ctx || set < VPT_GATES_CONTEXT || set > VPT_GATES_FULL)
    return vpt::set_error(VPT_E_INVALID, "vpt_gpu_gate_info: bad argument");
  if (gates) {
    const int own[4] = {ctx->scene.gate_min, ctx->scene.gate_idle, ctx->scene.gate_eval, ctx->scene.gate_walk};
    const int* g = set == VPT_GATES_CONTEXT ? own : set == VPT_GATES_LATENCY ? ctx->lat_gate : ctx->full_gate;
    for (int i = 0; i < 4; ++i) gates[i] = g[i];
  }
  if (last_launch_set) *last_launch_set = ctx->last_gate_set;
  return VPT_OK;
}

int vpt_gpu_set_latency_kernel(vpt_gpu_ctx* ctx, int mode, int ungated) {
  if (!ctx || mode < -1 || mode > 1 || ungated < -1 || ungated > 1)
    return vpt::set_error(VPT_E_INVALID, "vpt_gpu_set_latency_kernel: bad argument");
  ctx->lat_mode = mode;  // read by the next render's host code only: no wait
  if (ungated >= 0) ctx->lat_ungated = ungated;
  return VPT_OK;
}

int vpt_gpu_profile(vpt_gpu_ctx* ctx, uint64_t* out, int n, int reset) {
  if (!ctx || !out) return vpt::set_error(VPT_E_INVALID, "null argument");
  int rc = ctx_device(ctx);
  if (rc) return rc;
  if ((rc = wait_ctx(ctx))) return rc;
  std::vector<unsigned long long> v(kProfWords);
  VPT_HIP(hipMemcpy(v.data(), ctx->prof, v.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
  if (n < (int)v.size()) return vpt::set_error(VPT_E_INVALID, "vpt_gpu_profile: output too small");
  for (size_t i = 0; i < v.size(); ++i) out[i] = v[i];
  if (reset) VPT_HIP(hipMemset(ctx->prof, 0, v.size() * sizeof(unsigned long long)));
  return VPT_OK;
}

int vpt_gpu_launch_info(const vpt_gpu_ctx* ctx, int* grid_blocks, int* block_threads) {
  if (!ctx) return vpt::set_error(VPT_E_INVALID, "null context");
  if (grid_blocks) *grid_blocks = ctx->grid_blocks;
  if (block_threads) *block_threads = vpt::kBlockThreads;
  return VPT_OK;
}

int vpt_gpu_set_compaction(vpt_gpu_ctx* ctx, int every) {
  if (!ctx || every < 0) return vpt::set_error(VPT_E_INVALID, "vpt_gpu_set_compaction: bad argument");
  ctx->compact_every = every;  // read by the next render's host code only: no wait
  return VPT_OK;
}

int vpt_gpu_latency_kernel_info(const vpt_gpu_ctx* ctx, int* mode, int* resident_blocks_per_cu) {
  if (!ctx) return vpt::set_error(VPT_E_INVALID, "null context");
  if (mode) *mode = ctx->lat_mode;
  if (resident_blocks_per_cu) *resident_blocks_per_cu = ctx->lat_per_cu;
  return VPT_OK;
}

}  // extern "C"

// matte_host.cpp — TEST HARNESS: the matte march (volume_path_tracer_amd/csrc/vpt_alpha.h and vpt_depth.h, the code
// vpt_alpha_kernel and vpt_depth_kernel run per lane) on the CPU.  Built like band_host (hipcc, host only) as one shared
// library bound by tests/alpha_lib.py and tests/depth_lib.py:
//   vpta_render(cfg, density, sub, alpha, tau)                 the whole frame, float[H][W] each (tau may be null)
//   vpta_tau_at(cfg, density, rx, ry, n, tau)                  the optical depths of the camera rays of n raster points
//   vptd_levels(n, opacity, tau)                               the library's opacity -> optical depth conversion
//   vptd_render(cfg, density, sub, n, opacity, depth, reach)   the whole frame, float[n][H][W] each (reach may be null)
//   vptd_tau_upto(cfg, density, x, y, z, count, tau)           the optical depth of pixel (x, y)'s centre ray up to the
//                                                              world distance z: the same march, cut at z
// and with -DALPHA_HOST_MAIN or -DDEPTH_HOST_MAIN as one stand-alone program (also under AddressSanitizer + UBSan) that
// marches a fixed set of rays over vpt_synth_grid volumes and exits 0 when every optical depth is finite and
// non-negative and every depth finite, positive and ascending.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../volume_path_tracer_amd/csrc/vpt_depth.h"
#include "../../volume_path_tracer_amd/csrc/vpt_internal.h"

namespace vpt {
static thread_local std::string g_err;
int set_error(int code, const std::string& msg) {
  g_err = msg;
  return code;
}
}  // namespace vpt

namespace {
// The host DevScene of (cfg, density), as hostsim.cpp builds it; the grid's tables live in `hd`.
int host_scene(const vpt_configuration* cfg, const vpt_grid_desc* density, vpt::HostGrid& hd, vpt::DevScene& S) {
  if (!cfg || !density) return VPT_E_INVALID;
  int rc = vpt::build_scene(*cfg, S);
  if (rc) return rc;
  if ((rc = vpt::build_host_grid(*density, true, 0, hd))) return rc;
  S.density = hd.dev;
  vpt::scene_finalize(S);
  S.tile_area = (uint32_t)(S.tw * S.th);
  return VPT_OK;
}

// fn(px, py, row-major pixel index) for every pixel a pass writes: in single-pixel mode only that one.
template <class Fn>
void each_pixel(const vpt::DevScene& S, Fn fn) {
  for (int32_t py = 0; py < S.H; ++py)
    for (int32_t px = 0; px < S.W; ++px)
      if (!S.single_pixel_enabled || (px == S.sp_x && py == S.sp_y)) fn(px, py, (size_t)py * S.W + px);
}
}  // namespace

extern "C" int vpta_render(const vpt_configuration* cfg, const vpt_grid_desc* density, uint32_t sub, float* alpha,
                           float* tau) {
  if (!alpha || sub < 1 || sub > vpt::kAlphaMaxSub) return VPT_E_INVALID;
  vpt::HostGrid hd;
  vpt::DevScene S{};
  if (int rc = host_scene(cfg, density, hd, S)) return rc;
  each_pixel(S, [&](int32_t px, int32_t py, size_t p) {
    float a, t;
    vpt::alpha_pixel(S, px, py, sub, a, t);
    alpha[p] = a;
    if (tau) tau[p] = t;
  });
  return VPT_OK;
}

extern "C" int vpta_tau_at(const vpt_configuration* cfg, const vpt_grid_desc* density, const float* rx, const float* ry,
                           uint64_t n, float* tau) {
  if (!rx || !ry || !tau) return VPT_E_INVALID;
  vpt::HostGrid hd;
  vpt::DevScene S{};
  if (int rc = host_scene(cfg, density, hd, S)) return rc;
  for (uint64_t q = 0; q < n; ++q) {
    float dv[3];
    vpt::alpha_camera_dir(S, rx[q], ry[q], dv);
    tau[q] = vpt::optical_depth(S, S.cam_pos, dv);
  }
  return VPT_OK;
}

extern "C" int vptd_levels(uint32_t n, const float* opacity, float* tau) {
  vpt::DepthLevels L;
  if (!tau || vpt::depth_levels(n, opacity, L)) return VPT_E_INVALID;
  for (uint32_t k = 0; k < n; ++k) tau[k] = L.tau[k];
  return VPT_OK;
}

extern "C" int vptd_render(const vpt_configuration* cfg, const vpt_grid_desc* density, uint32_t sub, uint32_t n,
                           const float* opacity, float* depth, float* reach) {
  if (!depth || sub < 1 || sub > vpt::kAlphaMaxSub) return VPT_E_INVALID;
  vpt::DepthLevels L;
  if (vpt::depth_levels(n, opacity, L)) return VPT_E_INVALID;
  vpt::HostGrid hd;
  vpt::DevScene S{};
  if (int rc = host_scene(cfg, density, hd, S)) return rc;
  const size_t plane = (size_t)S.H * (size_t)S.W;
  each_pixel(S, [&](int32_t px, int32_t py, size_t p) {
    float d[vpt::kDepthMaxLevels], r[vpt::kDepthMaxLevels];
    vpt::depth_pixel(S, px, py, sub, L, d, r);
    for (uint32_t k = 0; k < n; ++k) {
      depth[k * plane + p] = d[k];
      if (reach) reach[k * plane + p] = r[k];
    }
  });
  return VPT_OK;
}

extern "C" int vptd_tau_upto(const vpt_configuration* cfg, const vpt_grid_desc* density, const int32_t* x, const int32_t* y,
                             const float* z, uint64_t count, float* tau) {
  if (!x || !y || !z || !tau) return VPT_E_INVALID;
  vpt::HostGrid hd;
  vpt::DevScene S{};
  if (int rc = host_scene(cfg, density, hd, S)) return rc;
  for (uint64_t q = 0; q < count; ++q) {
    float dv[3], scale = 0.0f;
    vpt::alpha_camera_dir(S, (float)x[q] + 0.5f, (float)y[q] + 0.5f, dv);
    vpt::optical_depth_upto(S, S.cam_pos, dv, 0.0f, &scale);
    // the cut in ray time: the largest t whose world distance t * scale does not exceed z (z = t * scale rounds,
    // so several t may share one z; the depth pass's own t is among them)
    float t = vpt::math::div_rn(z[q], scale);
    if (!(scale > 0.0f) || !std::isfinite(t)) {
      tau[q] = 0.0f;
      continue;
    }
    for (int i = 0; i < 8 && t * scale > z[q]; ++i) t = std::nextafterf(t, 0.0f);
    for (int i = 0; i < 8 && std::nextafterf(t, INFINITY) * scale <= z[q]; ++i) t = std::nextafterf(t, INFINITY);
    tau[q] = vpt::optical_depth_upto(S, S.cam_pos, dv, t, nullptr);
  }
  return VPT_OK;
}

#if defined(ALPHA_HOST_MAIN) || defined(DEPTH_HOST_MAIN)
namespace {
int g_fail = 0;

void fail(const char* what, const char* where, int a, int b, double u, double v) {
  std::printf("FAIL %s %s (%d, %d): %g %g\n", what, where, a, b, u, v);
  ++g_fail;
}

vpt_configuration base_config() {
  vpt_configuration c;
  std::memset(&c, 0, sizeof c);
  c.num_waves = 1;
  c.output_size[0] = c.output_size[1] = 16;
  c.tile_size[0] = c.tile_size[1] = 8;
  const float pos[3] = {0.0f, 0.0f, -200.0f}, up[3] = {0.0f, 1.0f, 0.0f};
  for (int i = 0; i < 3; ++i) {
    c.camera_parameters.position[i] = pos[i];
    c.camera_parameters.up[i] = up[i];
  }
  c.camera_parameters.vfov_deg = 30.0f;
  c.camera_parameters.imaging_ratio = 1.0f;
  c.volume_parameters.sigma_a = 0.5f;
  c.volume_parameters.sigma_s = 1.5f;
  return c;
}

// Marches the rays (o, d) [n][3] (world units of voxel size 1, scaled by `voxel`) over the synthetic grid `kind`
// of n^3 voxels of size `voxel` centred at the world origin: the optical depth of each, then its depths at four levels.
void march(const char* what, int kind, int n, float voxel, const float (*o)[3], const float (*d)[3], int rays) {
  vpt_grid_desc* g = vpt_synth_grid(kind, n);
  if (!g) return fail(what, "vpt_synth_grid", 0, 0, 0.0, 0.0);
  for (int i = 0; i < 9; ++i) {
    g->map_mat[i] = (i % 4 == 0) ? voxel : 0.0f;
    g->map_inv_mat[i] = (i % 4 == 0) ? 1.0f / voxel : 0.0f;
  }
  for (int i = 0; i < 3; ++i) g->map_vec[i] = -0.5f * (float)n * voxel;
  vpt_configuration cfg = base_config();
  cfg.volume_parameters.sigma_a /= voxel;  // (sigma is per world unit)
  cfg.volume_parameters.sigma_s /= voxel;
  vpt::HostGrid hd;
  vpt::DevScene S{};
  const float op[4] = {1.0f / 255.0f, 0.5f, 0.500001f, 0.9f};
  vpt::DepthLevels L;
  if (host_scene(&cfg, g, hd, S) || vpt::depth_levels(4, op, L)) {
    std::printf("%s: host_scene or depth_levels: %s\n", what, vpt::g_err.c_str());
    vpt_synth_free(g);
    return fail(what, "setup", 0, 0, 0.0, 0.0);
  }
  for (int r = 0; r < rays; ++r) {
    const float ow[3] = {o[r][0] * voxel, o[r][1] * voxel, o[r][2] * voxel};
    const float tau = vpt::optical_depth(S, ow, d[r]);
    std::printf("%s ray %d: tau %.9g\n", what, r, (double)tau);
    if (!(std::isfinite(tau) && tau >= 0.0f)) fail(what, "ray tau", r, 0, (double)tau, 0.0);
    float z[vpt::kDepthMaxLevels];
    const uint32_t got = vpt::depth_ray(S, ow, d[r], L, z);
    std::printf("%s ray %d: reached %u z %.9g %.9g %.9g %.9g\n", what, r, got, (double)z[0], (double)z[1], (double)z[2],
                (double)z[3]);
    bool ok = got <= 4;
    for (uint32_t k = 0; k < got && ok; ++k) ok = std::isfinite(z[k]) && z[k] > 0.0f && (k == 0 || z[k] >= z[k - 1]);
    for (uint32_t k = got; k < 4 && ok; ++k) ok = z[k] == 0.0f;  // (a level not reached: +0.0, never stale)
    if (!ok) fail(what, "ray depths", r, (int)got, (double)z[0], (double)z[3]);
  }
  // the frame through the pixel helpers as well (alpha and reach in [0, 1], tau and depth finite and >= 0)
  for (int32_t py = 0; py < S.H; py += 5)
    for (int32_t px = 0; px < S.W; px += 5) {
      float a, t, dp[vpt::kDepthMaxLevels], rc[vpt::kDepthMaxLevels];
      vpt::alpha_pixel(S, px, py, 2, a, t);
      if (!(std::isfinite(t) && t >= 0.0f && a >= 0.0f && a <= 1.0f)) fail(what, "pixel alpha, tau", px, py, (double)a, (double)t);
      vpt::depth_pixel(S, px, py, 2, L, dp, rc);
      for (int k = 0; k < 4; ++k)
        if (!(std::isfinite(dp[k]) && dp[k] >= 0.0f && rc[k] >= 0.0f && rc[k] <= 1.0f))
          fail(what, "pixel depth, reach", px, py, (double)dp[k], (double)rc[k]);
    }
  vpt_synth_free(g);
}
}  // namespace

int main() {
  const float s = 0.70710678f;
  // rays 0-2 axis-aligned (two zero components, +0 and -0); 3 and 4 in the bbox faces x = 0 and x = n (index); 5 and 6
  // start inside; 7 and 8 miss; 9 oblique; 10 has no direction
  const float o[][3] = {{0.0f, 0.0f, -200.0f}, {200.0f, 3.0f, 1.0f},  {-1.5f, 200.0f, 2.5f}, {-32.0f, 0.0f, -200.0f},
                        {32.0f, 1.0f, -200.0f}, {1.25f, -2.5f, 3.75f}, {0.0f, 0.0f, 0.0f},    {0.0f, 100.0f, -200.0f},
                        {0.0f, 0.0f, -200.0f},  {-150.0f, 7.0f, -150.0f}, {0.0f, 0.0f, -200.0f}};
  const float d[][3] = {{0.0f, 0.0f, 1.0f},  {-1.0f, -0.0f, 0.0f}, {0.0f, -1.0f, -0.0f}, {0.0f, 0.0f, 1.0f},
                        {0.0f, 0.0f, 1.0f},  {0.36f, 0.48f, 0.8f}, {-s, 0.0f, s},        {0.0f, 0.0f, 1.0f},
                        {0.0f, 0.0f, -1.0f}, {s, 0.0f, s},         {0.0f, 0.0f, 0.0f}};
  const int rays = (int)(sizeof o / sizeof o[0]);
  march("cloud", 1, 64, 1.0f, o, d, rays);
  march("cube", 0, 64, 1.0f, o, d, rays);
  march("voxel 2^-20", 1, 64, 0x1p-20f, o, d, rays);
  march("voxel 2^27", 1, 64, 0x1p27f, o, d, rays);
  if (g_fail) {
    std::printf("matte_host: %d checks failed\n", g_fail);
    return 1;
  }
  std::printf("alpha_host ok\ndepth_host ok\n");
  return 0;
}
#endif

// alpha_host.cpp — TEST HARNESS: the coverage pass's march (volume_path_tracer_amd/csrc/vpt_alpha.h, the code
// vpt_alpha_kernel runs per lane) on the CPU.  Built by tests/test_alpha_host.py like band_host (hipcc, host only)
// as a shared library bound by tests/alpha_lib.py:
//   vpta_render(cfg, density, sub, alpha, tau)        the whole frame, float[H][W] each (tau may be null)
//   vpta_tau_at(cfg, density, rx, ry, n, tau)         the optical depths of the camera rays of n raster points
// and with -DALPHA_HOST_MAIN as a stand-alone program (also under AddressSanitizer + UBSan) that marches a fixed
// set of rays over vpt_synth_grid volumes and exits 0 when every optical depth is finite and non-negative.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../volume_path_tracer_amd/csrc/vpt_alpha.h"
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
}  // namespace

extern "C" int vpta_render(const vpt_configuration* cfg, const vpt_grid_desc* density, uint32_t sub, float* alpha,
                           float* tau) {
  if (!alpha || sub < 1 || sub > vpt::kAlphaMaxSub) return VPT_E_INVALID;
  vpt::HostGrid hd;
  vpt::DevScene S{};
  if (int rc = host_scene(cfg, density, hd, S)) return rc;
  for (int32_t py = 0; py < S.H; ++py)
    for (int32_t px = 0; px < S.W; ++px) {
      if (S.single_pixel_enabled && (px != S.sp_x || py != S.sp_y)) continue;  // (only that pixel is written)
      float a, t;
      vpt::alpha_pixel(S, px, py, sub, a, t);
      alpha[(size_t)py * S.W + px] = a;
      if (tau) tau[(size_t)py * S.W + px] = t;
    }
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

#ifdef ALPHA_HOST_MAIN
namespace {
int g_fail = 0;

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
// of n^3 voxels of size `voxel` centred at the world origin.
void march(const char* what, int kind, int n, float voxel, const float (*o)[3], const float (*d)[3], int rays) {
  vpt_grid_desc* g = vpt_synth_grid(kind, n);
  if (!g) {
    std::printf("FAIL %s: vpt_synth_grid\n", what);
    ++g_fail;
    return;
  }
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
  if (host_scene(&cfg, g, hd, S)) {
    std::printf("FAIL %s: host_scene: %s\n", what, vpt::g_err.c_str());
    ++g_fail;
    vpt_synth_free(g);
    return;
  }
  for (int r = 0; r < rays; ++r) {
    const float ow[3] = {o[r][0] * voxel, o[r][1] * voxel, o[r][2] * voxel};
    const float tau = vpt::optical_depth(S, ow, d[r]);
    std::printf("%s ray %d: tau %.9g\n", what, r, (double)tau);
    if (!(std::isfinite(tau) && tau >= 0.0f)) {
      std::printf("FAIL %s ray %d: tau %g\n", what, r, (double)tau);
      ++g_fail;
    }
  }
  // the frame through the camera helper as well (alpha in [0, 1], tau finite)
  for (int32_t py = 0; py < S.H; py += 5)
    for (int32_t px = 0; px < S.W; px += 5) {
      float a, t;
      vpt::alpha_pixel(S, px, py, 2, a, t);
      if (!(std::isfinite(t) && t >= 0.0f && a >= 0.0f && a <= 1.0f)) {
        std::printf("FAIL %s pixel (%d, %d): alpha %g tau %g\n", what, px, py, (double)a, (double)t);
        ++g_fail;
      }
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
    std::printf("alpha_host: %d checks failed\n", g_fail);
    return 1;
  }
  std::printf("alpha_host ok\n");
  return 0;
}
#endif

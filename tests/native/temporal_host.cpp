// temporal_host.cpp — TEST HARNESS: the temporal pass's per-pixel function (volume_path_tracer_amd/csrc/vpt_temporal.h,
// the code vpt_temporal_kernel runs per lane) over a frame on the CPU.  Built by tests/temporal_lib.py (hipcc, host
// only) as a shared library:
//   vptt_temporal(W, H, params, cur16, prev16, film, m2, depth, hist film, hist m2, hist depth, out film, out m2,
//                 motion, hist_n)      the whole call, host arrays, the cameras as their 16 floats (vpt_shutter_entry)
//   vptt_constants(prev16, out12)      the previous camera's projection constants n, a, b, tn, ta, tb
// and with -DTEMPORAL_HOST_MAIN as a stand-alone program (also under AddressSanitizer + UBSan) that accumulates a few
// small frames with unrendered pixels through several previous cameras and exits 0 when every output is as it must be.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../include/vpt_gpu.h"
#define VPT_TEMPORAL_NO_KERNELS  // no device code object in a host-only build
#include "../../volume_path_tracer_amd/csrc/vpt_temporal.h"

extern "C" int vptt_constants(const float* prev16, float* out12) {
  if (!prev16 || !out12) return VPT_E_INVALID;
  vpt::TemporalArgs A{};
  vpt::temporal_prev_constants(prev16, A);
  for (int i = 0; i < 3; ++i) {
    out12[i] = A.pn[i];
    out12[3 + i] = A.pa[i];
    out12[6 + i] = A.pb[i];
  }
  out12[9] = A.ptn;
  out12[10] = A.pta;
  out12[11] = A.ptb;
  return VPT_OK;
}

extern "C" int vptt_temporal(int32_t W, int32_t H, const vpt_temporal_params* p, const float* cur16, const float* prev16,
                             const float* film, const float* m2, const float* depth, const float* hist_film,
                             const float* hist_m2, const float* hist_depth, float* out_film, float* out_m2, float* motion,
                             float* hist_n) {
  if (!p || !cur16 || !prev16 || !film || !m2 || !depth || !out_film || !out_m2 || W < 1 || H < 1) return VPT_E_INVALID;
  const int n_hist = (hist_film != nullptr) + (hist_m2 != nullptr) + (hist_depth != nullptr);
  if ((n_hist != 0 && n_hist != 3) || p->n_levels < 1 || p->n_levels > vpt::kTemporalMaxLevels) return VPT_E_INVALID;
  const size_t N = (size_t)W * (size_t)H;
  vpt::TemporalArgs A{};
  A.W = W;
  A.H = H;
  A.n_levels = p->n_levels;
  A.has_history = n_hist == 3;
  A.max_history = p->max_history;
  A.depth_tol = p->depth_tol;
  A.sigma_r = p->sigma_r;
  A.rel_floor = p->rel_floor;
  std::memcpy(A.cur, cur16, sizeof A.cur);
  vpt::temporal_prev_constants(prev16, A);
  // (float4 views of the caller's films: copies, so that no alignment is asked of a host array)
  std::vector<float4> f(N), hf(n_hist ? N : 0);
  std::memcpy(f.data(), film, N * sizeof(float4));
  if (n_hist) std::memcpy(hf.data(), hist_film, N * sizeof(float4));
  for (int32_t y = 0; y < H; ++y)
    for (int32_t x = 0; x < W; ++x) {
      const size_t q = (size_t)y * W + x;
      const vpt::TemporalPixel o =
          vpt::temporal_pixel(A, f.data(), m2, depth, n_hist ? hf.data() : nullptr, hist_m2, hist_depth, x, y);
      std::memcpy(out_film + 4 * q, &o.film, sizeof o.film);
      out_m2[q] = o.m2;
      if (motion) {
        motion[2 * q] = o.mx;
        motion[2 * q + 1] = o.my;
      }
      if (hist_n) hist_n[q] = o.hn;
    }
  return VPT_OK;
}

#ifdef TEMPORAL_HOST_MAIN
namespace {
// A camera at `pos` looking along the unit vector `fwd` (up = +y, fwd has no y part) on a W x H raster, tan(vfov / 2) =
// tv, in the shutter entry's layout: the map raster point -> direction that Camera::Camera derives, written out.
void camera16(const float pos[3], const float fwd[3], float tv, int W, int H, float out[16]) {
  const float left[3] = {fwd[2], 0.0f, -fwd[0]}, up[3] = {0.0f, 1.0f, 0.0f};  // left = up x fwd
  const float ar = (float)W / (float)H, hx = (float)W / 2.0f, hy = (float)H / 2.0f;
  for (int i = 0; i < 3; ++i) {
    out[4 * i + 0] = -(left[i] * ar * tv) / hx;
    out[4 * i + 1] = -(up[i] * tv) / hy;
    out[4 * i + 2] = 0.0f;
    out[4 * i + 3] = left[i] * ar * tv + up[i] * tv + fwd[i];
    out[12 + i] = pos[i];
  }
  out[15] = 0.0f;
}
}  // namespace

int main() {
  const int sizes[4][2] = {{37, 21}, {1, 1}, {3, 70}, {130, 9}};
  const float cs2 = std::cos(0.0349066f), sn2 = std::sin(0.0349066f);
  const float cur_pos[3] = {0.0f, 0.0f, -300.0f}, cur_fwd[3] = {0.0f, 0.0f, 1.0f};
  // previous cameras: the same, a 2-degree orbit, a dolly, a turn away, the volume behind it
  const float prev_pos[5][3] = {{0, 0, -300}, {-300 * sn2, 0, -300 * cs2}, {0, 0, -220}, {0, 0, -300}, {0, 0, 20}};
  const float prev_fwd[5][3] = {{0, 0, 1}, {sn2, 0, cs2}, {0, 0, 1}, {0.8660254f, 0, -0.5f}, {0, 0, 1}};
  int bad = 0;
  for (const auto& wh : sizes)
    for (uint32_t K = 1; K <= 2; ++K)
      for (int pc = 0; pc < 5; ++pc)
        for (int with_hist = 0; with_hist < 2; ++with_hist) {
          const int W = wh[0], H = wh[1];
          const size_t N = (size_t)W * H;
          float cur[16], prev[16];
          camera16(cur_pos, cur_fwd, 0.2679492f, W, H, cur);
          camera16(prev_pos[pc], prev_fwd[pc], 0.2679492f, W, H, prev);
          std::vector<float> film(4 * N), m2(N), depth(K * N), hfilm(4 * N), hm2(N), hdepth(K * N);
          std::vector<float> out(4 * N, NAN), om2(N, NAN), mv(2 * N, NAN), hn(N, NAN);
          uint32_t r = 12345u + (uint32_t)pc;
          auto rnd = [&r]() {
            r = r * 1664525u + 1013904223u;
            return (float)(r >> 8) / 16777216.0f;
          };
          auto fill = [&](std::vector<float>& f, std::vector<float>& m, std::vector<float>& d, size_t shift) {
            for (size_t q = 0; q < N; ++q) {
              const size_t s = q + shift;
              const float n = (float)(N > 1 && s % 7 == 3 ? 0 : s % 5 == 1 ? 1 : 2 + s % 30);
              const float y = 0.5f + rnd();
              f[4 * q + 0] = n ? 0.5f * y * n : NAN;
              f[4 * q + 1] = n ? y * n : NAN;
              f[4 * q + 2] = n ? 2.0f * y * n : NAN;
              f[4 * q + 3] = n;
              m[q] = n ? n * (y * y + 0.1f * rnd()) : NAN;
              // a slab in the middle of the frame at about the distance to the origin, its core one level deeper
              const int x = (int)(q % W), yy = (int)(q / W);
              const bool slab = W < 4 || (x > W / 4 && x < 3 * W / 4), core = slab && yy > H / 4 && yy < 3 * H / 4;
              d[q] = !n ? NAN : slab ? 240.0f + 20.0f * rnd() : 0.0f;
              if (K > 1) d[N + q] = !n ? NAN : core ? 280.0f + 10.0f * rnd() : 0.0f;
            }
          };
          fill(film, m2, depth, 0);
          fill(hfilm, hm2, hdepth, 2);
          vpt_temporal_params p{K, 64.0f, 0.1f, 4.0f, 1e-3f};
          const int rc = vptt_temporal(W, H, &p, cur, prev, film.data(), m2.data(), depth.data(),
                                       with_hist ? hfilm.data() : nullptr, with_hist ? hm2.data() : nullptr,
                                       with_hist ? hdepth.data() : nullptr, out.data(), om2.data(), mv.data(), hn.data());
          if (rc != VPT_OK) ++bad;
          size_t used = 0;
          for (size_t q = 0; q < N; ++q) {
            if (!(hn[q] >= 0.0f) || hn[q] > 64.0f) ++bad;  // written, never NaN, capped
            const bool through = hn[q] == 0.0f;
            if (!with_hist && !through) ++bad;
            if (!(film[4 * q + 3] >= 1.0f) && !through) ++bad;
            if (through) {
              if (std::memcmp(&out[4 * q], &film[4 * q], 16) != 0 || std::memcmp(&om2[q], &m2[q], 4) != 0) ++bad;
            } else {
              ++used;
              for (int c = 0; c < 4; ++c)
                if (!std::isfinite(out[4 * q + c])) ++bad;
              if (!std::isfinite(om2[q]) || !(out[4 * q + 3] > film[4 * q + 3])) ++bad;
            }
            if (std::isnan(mv[2 * q]) != std::isnan(mv[2 * q + 1])) ++bad;
            if (pc == 0 && !(std::fabs(mv[2 * q]) < 1e-2f && std::fabs(mv[2 * q + 1]) < 1e-2f)) ++bad;  // the same camera
            if (pc == 4 && depth[q] > 0.0f && !std::isnan(mv[2 * q])) ++bad;  // a point behind the camera
          }
          if (with_hist && pc == 0 && N > 1 && used == 0) ++bad;  // (the same camera accumulates)
        }
  std::printf("temporal_host: %d bad values\n", bad);
  return bad ? 1 : 0;
}
#endif

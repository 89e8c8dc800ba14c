// denoise_host.cpp — TEST HARNESS: the denoiser's per-pixel functions (volume_path_tracer_amd/csrc/vpt_denoise.h, the
// code vpt_denoise_prepare_kernel and vpt_denoise_atrous_kernel run per lane) over a frame on the CPU.  Built by
// tests/denoise_lib.py (hipcc, host only) as a shared library:
//   vptd_denoise(W, H, params, film, m2, guides, out_film, var_out)      the whole call, host arrays
// and with -DDENOISE_HOST_MAIN as a stand-alone program (also under AddressSanitizer + UBSan) that filters a few
// small frames with unrendered pixels and exits 0 when every valid output is finite.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <utility>
#include <vector>

#include "../../include/vpt_gpu.h"
#define VPT_DENOISE_NO_KERNELS  // no device code object in a host-only build
#include "../../volume_path_tracer_amd/csrc/vpt_denoise.h"

namespace {
template <int G>
void iterate(const vpt::DenoiseArgs& A, int32_t step, const float4* src, const float4* gd, float4* dst) {
  for (int32_t y = 0; y < A.H; ++y)
    for (int32_t x = 0; x < A.W; ++x) dst[(size_t)y * A.W + x] = vpt::denoise_atrous_pixel<G>(src, gd, A, x, y, step);
}
}  // namespace

extern "C" int vptd_denoise(int32_t W, int32_t H, const vpt_denoise_params* p, const float* film, const float* m2,
                            const float* const* guides, float* out_film, float* var_out) {
  if (!p || !film || !m2 || !out_film || W < 1 || H < 1) return VPT_E_INVALID;
  if (p->iterations < 1 || p->iterations > vpt::kDenoiseMaxIterations || p->n_guides > vpt::kDenoiseMaxGuides)
    return VPT_E_INVALID;
  if (p->n_guides && !guides) return VPT_E_INVALID;
  const size_t N = (size_t)W * (size_t)H;
  const uint32_t G = p->n_guides;
  vpt::DenoiseArgs A{};
  A.W = W;
  A.H = H;
  A.sigma_l = p->sigma_l;
  A.rel_floor = p->rel_floor;
  for (uint32_t k = 0; k < 4; ++k) A.guide_sigma[k] = k < G ? p->guide_sigma[k] : 1.0f;
  std::vector<float4> a(N), b(N), gd(G ? N : 0);
  for (size_t q = 0; q < N; ++q) {
    float4 f;
    std::memcpy(&f, film + 4 * q, sizeof f);
    a[q] = vpt::denoise_prepare_pixel(f, m2[q]);
    if (G) {
      float g[4] = {0.0f, 0.0f, 0.0f, 0.0f};
      for (uint32_t k = 0; k < G; ++k) g[k] = guides[k][q];
      gd[q] = make_float4(g[0], g[1], g[2], g[3]);
    }
  }
  float4 *src = a.data(), *dst = b.data();
  for (uint32_t i = 0; i < p->iterations; ++i) {
    const int32_t step = (int32_t)(1u << i);
    switch (G) {
      case 0: iterate<0>(A, step, src, gd.data(), dst); break;
      case 1: iterate<1>(A, step, src, gd.data(), dst); break;
      case 2: iterate<2>(A, step, src, gd.data(), dst); break;
      case 3: iterate<3>(A, step, src, gd.data(), dst); break;
      default: iterate<4>(A, step, src, gd.data(), dst); break;
    }
    std::swap(src, dst);
  }
  for (size_t q = 0; q < N; ++q) {
    float4 f;
    std::memcpy(&f, film + 4 * q, sizeof f);
    float var;
    const float4 o = vpt::denoise_finish_pixel(src[q], f, var);
    std::memcpy(out_film + 4 * q, &o, sizeof o);
    if (var_out) var_out[q] = var;
  }
  return VPT_OK;
}

#ifdef DENOISE_HOST_MAIN
int main() {
  const int sizes[4][2] = {{37, 21}, {1, 1}, {3, 70}, {130, 9}};
  int bad = 0;
  for (const auto& wh : sizes)
    for (uint32_t G = 0; G <= 4; G += 2) {
      const int W = wh[0], H = wh[1];
      const size_t N = (size_t)W * H;
      std::vector<float> film(4 * N), m2(N), out(4 * N, NAN), var(N, NAN);
      std::vector<std::vector<float>> g(G, std::vector<float>(N));
      uint32_t r = 12345u;
      auto rnd = [&r]() {
        r = r * 1664525u + 1013904223u;
        return (float)(r >> 8) / 16777216.0f;
      };
      for (size_t q = 0; q < N; ++q) {
        const float n = (float)(q % 7 == 3 ? 0 : q % 5 == 1 ? 1 : 2 + q % 30);
        const float y = 0.5f + rnd();
        film[4 * q + 0] = n ? 0.5f * y * n : NAN;
        film[4 * q + 1] = n ? y * n : NAN;
        film[4 * q + 2] = n ? 2.0f * y * n : NAN;
        film[4 * q + 3] = n;
        m2[q] = n ? n * (y * y + 0.1f * rnd()) : NAN;
        for (uint32_t k = 0; k < G; ++k) g[k][q] = n ? rnd() : NAN;
      }
      const float* gp[4] = {nullptr, nullptr, nullptr, nullptr};
      for (uint32_t k = 0; k < G; ++k) gp[k] = g[k].data();
      vpt_denoise_params p{5, G, 4.0f, 1e-3f, {0.2f, 0.2f, 0.2f, 0.2f}};
      if (vptd_denoise(W, H, &p, film.data(), m2.data(), gp, out.data(), var.data()) != VPT_OK) ++bad;
      for (size_t q = 0; q < N; ++q) {
        const bool valid = film[4 * q + 3] >= 1.0f;
        for (int c = 0; c < 4; ++c)
          if (valid ? !std::isfinite(out[4 * q + c]) : std::memcmp(&out[4 * q + c], &film[4 * q + c], 4) != 0) ++bad;
        if (!std::isfinite(var[q])) ++bad;
      }
    }
  std::printf("denoise_host: %d bad values\n", bad);
  return bad ? 1 : 0;
}
#endif

// vpt_depth.h — the depth pass: the distances at which a primary ray's optical depth first reaches given levels.
//
// The coverage pass (vpt_alpha.h) knows the optical depth tau(t) of a primary ray at every cut of its march, hence
// the probability 1 - exp(-tau(t)) that the first real collision lies before t.  depth_ray() is that march --
// matte_march() itself, not a copy -- with a test after every lattice piece: the accumulated tau, formed by the very
// expression that forms optical_depth()'s result, against the next level tau_k = -log1p(-a_k) (converted once, on the
// host).  In the piece where the test first passes a fixed bisection finds the time -- the partial integral over
// [ta, t] is again Simpson's rule, exact because the field is one cubic on the whole piece -- and the ray stops
// marching when its last level is reached.
//
// __host__ __device__: vpt_depth_kernel (vpt_kernels.h) and the host harness (tests/native/matte_host.cpp) run the
// same code.  Only +, *, comparisons and the correctly rounded helpers of vpt_math.h, contraction off, no expf: the
// same bits on both.
#pragma once

#include "vpt_alpha.h"

namespace vpt {

constexpr uint32_t kDepthMaxLevels = VPT_DEPTH_MAX_LEVELS;
constexpr int kDepthBisectSteps = 16;  // halvings of the piece [ta, tb] per level (include/vpt_gpu.h states it)

// The levels as optical depths, ascending; passed by value (kernel arguments: scalar loads, no per-lane table).
struct DepthLevels {
  uint32_t n;
  float tau[kDepthMaxLevels];
};

// The caller's opacities 0 < a_0 < a_1 < ... < 1 as optical depths, tau_k = (float)(-log1p(-(double)a_k)), once, on
// the host.  Returns null, or what is wrong with the list.
inline const char* depth_levels(uint32_t n, const float* opacity, DepthLevels& L) {
  L.n = 0;
  for (uint32_t k = 0; k < kDepthMaxLevels; ++k) L.tau[k] = 3.40282347e+38f;
  if (n < 1 || n > kDepthMaxLevels) return "1..4 opacity levels";
  if (!opacity) return "null opacity array";
  for (uint32_t k = 0; k < n; ++k) {
    if (!(opacity[k] > 0.0f && opacity[k] < 1.0f)) return "an opacity outside (0, 1)";  // (also a NaN)
    if (k && !(opacity[k] > opacity[k - 1])) return "opacities not strictly ascending";
    L.tau[k] = (float)(-log1p(-(double)opacity[k]));
  }
  L.n = n;
  return nullptr;
}

// tau[k] by selects (k is per lane; an indexed read would put the table into scratch).
__host__ __device__ __forceinline__ float depth_level(const DepthLevels& L, uint32_t k) {
  return k == 0u ? L.tau[0] : (k == 1u ? L.tau[1] : (k == 2u ? L.tau[2] : L.tau[3]));
}

// optical_depth()'s final expression on the ray's sum so far (`total`: the finished segments) plus the running
// segment's (`sum`): at the ray's last piece these are the bits of the matte's tau (before its clamp at 0).
__host__ __device__ __forceinline__ float depth_tau(float c, float total, float sum) {
  return c * math::div_rn(total + sum, 6.0f);
}

// The depths of one world ray: z[k] = (index-space time at which tau first reaches L.tau[k]) * scale for the levels
// reached, which are the first `return value` ones (the levels ascend and are tested in turn); +0.0 for the others.
// matte_march() with the level test as its visitor: after each piece, while the accumulated tau reaches the next
// level, that level's time is bisected within the piece; the ray stops when the last level is reached.  With negative
// densities (a signed grid) "first reaches" is the first piece whose test passes and the bisection returns one
// crossing in it.
__host__ __device__ inline uint32_t depth_ray(const DevScene& S, const float o[3], const float dir[3], const DepthLevels& L,
                                              float z[kDepthMaxLevels]) {
  float t_hit[kDepthMaxLevels] = {0.0f, 0.0f, 0.0f, 0.0f};
  uint32_t next = 0;
  float total, scale;
  const bool ray = matte_march<false>(S, o, dir, 0.0f, total, scale, [&](const MattePiece& p, const Lane& ln, StencilCell& sc) {
    const DevGrid& G = S.density;
    const float acc = depth_tau(p.c, p.total, p.sum);
    for (uint32_t lv = 0; lv < kDepthMaxLevels; ++lv) {  // several levels may fall into one piece: in turn
      if (!(next < L.n)) break;
      const float thr = depth_level(L, next);
      if (!(acc >= thr)) break;  // (also a NaN)
      // Bisection on [ta, tb]; the upper end always passes the test: at tb the partial sum is the piece's own
      // expression, and a midpoint becomes the upper end only after it has passed.
      float lo = p.ta, hi = p.tb;
      for (int i = 0; i < kDepthBisectSteps; ++i) {
        const float tm = lo + 0.5f * (hi - lo);
        const float hm = tm - p.ta;
        const float f1 = alpha_field(G, ln, sc, p.ta + 0.5f * hm), f2 = alpha_field(G, ln, sc, tm);
        const bool ok = depth_tau(p.c, p.total, p.before + hm * ((p.fa + 4.0f * f1) + f2)) >= thr;
        hi = ok ? tm : hi;
        lo = ok ? lo : tm;
      }
      t_hit[0] = next == 0u ? hi : t_hit[0];
      t_hit[1] = next == 1u ? hi : t_hit[1];
      t_hit[2] = next == 2u ? hi : t_hit[2];
      t_hit[3] = next == 3u ? hi : t_hit[3];
      ++next;
    }
    return !(next < L.n);
  });
  for (uint32_t k = 0; k < kDepthMaxLevels; ++k) z[k] = ray ? t_hit[k] * scale : 0.0f;
  return next;
}

// One pixel of the depth planes over alpha_pixel()'s sub-rays (matte_subrays): per level the sum of the depths of the
// sub-rays that reached it, in that order, divided by their count (+0.0 when none did), and count / n.
__host__ __device__ inline void depth_pixel(const DevScene& S, int32_t px, int32_t py, uint32_t s, const DepthLevels& L,
                                            float depth[kDepthMaxLevels], float reach[kDepthMaxLevels]) {
  float sum[kDepthMaxLevels] = {0.0f, 0.0f, 0.0f, 0.0f};
  uint32_t cnt[kDepthMaxLevels] = {0u, 0u, 0u, 0u};
  const uint32_t sub = matte_subrays(S, px, py, s, [&](const float dv[3]) {
    float z[kDepthMaxLevels];
    const uint32_t got = depth_ray(S, S.cam_pos, dv, L, z);
    for (uint32_t k = 0; k < kDepthMaxLevels; ++k) {
      const bool in = k < got;
      sum[k] = in ? sum[k] + z[k] : sum[k];
      cnt[k] += in ? 1u : 0u;
    }
  });
  const float n = (float)(sub * sub), rn = math::recip_for_div(n);
  for (uint32_t k = 0; k < kDepthMaxLevels; ++k) {
    depth[k] = cnt[k] ? math::div_rn(sum[k], (float)cnt[k]) : 0.0f;
    reach[k] = math::div_by_recip((float)cnt[k], n, rn);
  }
}

}  // namespace vpt

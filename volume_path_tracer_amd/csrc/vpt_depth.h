// vpt_depth.h — the depth pass: the distances at which a primary ray's optical depth first reaches given levels.
//
// The coverage pass (vpt_alpha.h) knows the optical depth tau(t) of a primary ray at every cut of its march, hence
// the probability 1 - exp(-tau(t)) that the first real collision lies before t.  depth_ray() is that march with a
// test after every lattice piece: the accumulated tau, formed by the very expression that forms optical_depth()'s
// result, against the next level tau_k = -log1p(-a_k) (converted once, on the host).  In the piece where the test
// first passes a fixed bisection finds the time -- the partial integral over [ta, t] is again Simpson's rule, exact
// because the field is one cubic on the whole piece -- and the ray stops marching when its last level is reached.
//
// __host__ __device__: vpt_depth_kernel (vpt_kernels.h) and the host harness (tests/native/depth_host.cpp) run the
// same code.  Only +, *, comparisons and the correctly rounded helpers of vpt_math.h, contraction off, no expf: the
// same bits on both.  Nothing here changes what optical_depth / alpha_segment / alpha_pixel compute.
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

// alpha_segment() with the piece test: the same cuts, the same sum.  After each piece, while the accumulated tau
// reaches the next level, that level's time is bisected within the piece and stored (index-space ray time) in
// t_hit[level]; `next` counts the levels reached.  Returns when the segment ends or the last level is reached.
// c = sigma_t * scale, total = the ray's sum over its earlier segments.
__host__ __device__ inline float depth_segment(const DevGrid& G, const Lane& ln, StencilCell& sc, const float inv[3], float t0,
                                               float t1, float c, float total, const DepthLevels& L, uint32_t& next,
                                               float t_hit[kDepthMaxLevels]) {
  if (!(t1 > t0)) return 0.0f;
  int32_t k[3], st[3];
  float tc[3], ext = 8.0f;
  for (int a = 0; a < 3; ++a) {
    const float p = ln.e[a] + ln.d[a] * t0;
    st[a] = hdda_stp(ln.d[a], inv[a]);
    if (!(fabsf(p) < 0x1p30f)) return 0.0f;
    const int32_t fl = (int32_t)floorf(p);
    k[a] = st[a] > 0 ? fl + 1 : fl;
    tc[a] = st[a] == 0 ? 3.40282347e+38f : ((float)k[a] - ln.e[a]) * inv[a];
    ext = ext + fabsf(ln.d[a]) * (t1 - t0);
  }
  const uint32_t bound = (uint32_t)(ext < kAlphaMaxPieces ? ext : kAlphaMaxPieces);
  float ta = t0, fa = alpha_field(G, ln, sc, t0), sum = 0.0f;
  for (uint32_t n = 0; n < bound; ++n) {
    const float m12 = tc[1] < tc[2] ? tc[1] : tc[2];
    const float tn = tc[0] < m12 ? tc[0] : m12;
    const bool last = !(tn < t1);  // (also a NaN time)
    float tb = last ? t1 : tn;
    if (tb < ta) tb = ta;
    for (int a = 0; a < 3; ++a) {
      const bool hit = !last && st[a] != 0 && tc[a] <= tn;
      k[a] += hit ? st[a] : 0;
      tc[a] = hit ? ((float)k[a] - ln.e[a]) * inv[a] : tc[a];
    }
    const float h = tb - ta;
    const float fm = alpha_field(G, ln, sc, ta + 0.5f * h), fb = alpha_field(G, ln, sc, tb);
    const float before = sum;
    sum = sum + h * ((fa + 4.0f * fm) + fb);
    const float acc = depth_tau(c, total, sum);
    for (uint32_t lv = 0; lv < kDepthMaxLevels; ++lv) {  // several levels may fall into one piece: in turn
      if (!(next < L.n)) break;
      const float thr = depth_level(L, next);
      if (!(acc >= thr)) break;  // (also a NaN)
      // Bisection on [ta, tb]; the upper end always passes the test: at tb the partial sum is the piece's own
      // expression, and a midpoint becomes the upper end only after it has passed.
      float lo = ta, hi = tb;
      for (int i = 0; i < kDepthBisectSteps; ++i) {
        const float tm = lo + 0.5f * (hi - lo);
        const float hm = tm - ta;
        const float f1 = alpha_field(G, ln, sc, ta + 0.5f * hm), f2 = alpha_field(G, ln, sc, tm);
        const bool ok = depth_tau(c, total, before + hm * ((fa + 4.0f * f1) + f2)) >= thr;
        hi = ok ? tm : hi;
        lo = ok ? lo : tm;
      }
      t_hit[0] = next == 0u ? hi : t_hit[0];
      t_hit[1] = next == 1u ? hi : t_hit[1];
      t_hit[2] = next == 2u ? hi : t_hit[2];
      t_hit[3] = next == 3u ? hi : t_hit[3];
      ++next;
    }
    ta = tb;
    fa = fb;
    if (last || !(next < L.n)) break;
  }
  return sum;
}

// The depths of one world ray: z[k] = (index-space time at which tau first reaches L.tau[k]) * scale for the levels
// reached, which are the first `return value` ones (the levels ascend and are tested in turn).  optical_depth()'s
// loop, bounds and exits; it ends early when the last level is reached.  With negative densities (a signed grid)
// "first reaches" is the first piece whose test passes and the bisection returns one crossing in it.
__host__ __device__ inline uint32_t depth_ray(const DevScene& S, const float o[3], const float dir[3], const DepthLevels& L,
                                              float z[kDepthMaxLevels]) {
  const DevGrid& G = S.density;
  Lane ln;
  lane_init(ln);
  const RayDir rd = ray_dir_setup(G, dir);
  if (!(rd.len > 0.0f && rd.len < 3.40282347e+38f)) return 0u;  // a zero or non-finite direction: no ray
  if (!begin_ray(G, ln, o, rd)) return 0u;
  const float inv[3] = {math::rcp_rn(ln.d[0]), math::rcp_rn(ln.d[1]), math::rcp_rn(ln.d[2])};
  StencilCell sc = {kNoCell, kNoCell, kNoCell, -1};
  const float c = S.sigma_t * ln.scale;
  float t_hit[kDepthMaxLevels] = {0.0f, 0.0f, 0.0f, 0.0f};
  int32_t steps = 0;
  uint32_t next = 0;
  float total = 0.0f;
  while (next < L.n && ln.s_t1 < ln.T1 && steps < kAlphaMaxSteps) {
    begin_segment(ln);
    bool done;
    do {
      ++steps;
      done = hdda_step(G, ln);
    } while (!done && steps < kAlphaMaxSteps);
    if (ln.s_dmaj <= 0.0f) continue;  // no draw there (SM_NEED_SEG's rule)
    total = total + depth_segment(G, ln, sc, inv, ln.s_t0, ln.s_t1, c, total, L, next, t_hit);
  }
  for (uint32_t k = 0; k < kDepthMaxLevels; ++k) z[k] = t_hit[k] * ln.scale;
  return next;
}

// The optical depth of one world ray up to the index-space time t_cut: optical_depth()'s march with every positive
// segment cut at t_cut, so the last piece is [ta, t_cut] -- the expression the bisection tests.  (Test harness.)
__host__ __device__ inline float optical_depth_upto(const DevScene& S, const float o[3], const float dir[3], float t_cut,
                                                    float* scale_out) {
  const DevGrid& G = S.density;
  Lane ln;
  lane_init(ln);
  const RayDir rd = ray_dir_setup(G, dir);
  if (scale_out) *scale_out = rd.scale;
  if (!(rd.len > 0.0f && rd.len < 3.40282347e+38f)) return 0.0f;
  if (!begin_ray(G, ln, o, rd)) return 0.0f;
  const float inv[3] = {math::rcp_rn(ln.d[0]), math::rcp_rn(ln.d[1]), math::rcp_rn(ln.d[2])};
  StencilCell sc = {kNoCell, kNoCell, kNoCell, -1};
  int32_t steps = 0;
  float total = 0.0f;
  while (ln.s_t1 < ln.T1 && ln.s_t1 < t_cut && steps < kAlphaMaxSteps) {
    begin_segment(ln);
    bool done;
    do {
      ++steps;
      done = hdda_step(G, ln);
    } while (!done && steps < kAlphaMaxSteps);
    if (ln.s_dmaj <= 0.0f) continue;
    total = total + alpha_segment(G, ln, sc, inv, ln.s_t0, ln.s_t1 < t_cut ? ln.s_t1 : t_cut);
  }
  return (S.sigma_t * ln.scale) * math::div_rn(total, 6.0f);
}

// One pixel of the depth planes: alpha_pixel()'s sub-rays in its order; per level the sum of the depths of the
// sub-rays that reached it, in that order, divided by their count (+0.0 when none did), and count / n.
__host__ __device__ inline void depth_pixel(const DevScene& S, int32_t px, int32_t py, uint32_t s, const DepthLevels& L,
                                            float depth[kDepthMaxLevels], float reach[kDepthMaxLevels]) {
  const uint32_t sub = S.jitter_scale != 0.0f ? s : 1u;
  const float fs = (float)sub, rs = math::recip_for_div(fs);
  float sum[kDepthMaxLevels] = {0.0f, 0.0f, 0.0f, 0.0f};
  uint32_t cnt[kDepthMaxLevels] = {0u, 0u, 0u, 0u};
  for (uint32_t j = 0; j < sub; ++j)
    for (uint32_t i = 0; i < sub; ++i) {
      const float rx = ((float)px + 0.5f) + S.jitter_scale * math::div_by_recip((float)i + 0.5f, fs, rs);
      const float ry = ((float)py + 0.5f) + S.jitter_scale * math::div_by_recip((float)j + 0.5f, fs, rs);
      float dv[3], z[kDepthMaxLevels];
      alpha_camera_dir(S, rx, ry, dv);
      const uint32_t got = depth_ray(S, S.cam_pos, dv, L, z);
      for (uint32_t k = 0; k < kDepthMaxLevels; ++k) {
        const bool in = k < got;
        sum[k] = in ? sum[k] + z[k] : sum[k];
        cnt[k] += in ? 1u : 0u;
      }
    }
  const float n = (float)(sub * sub), rn = math::recip_for_div(n);
  for (uint32_t k = 0; k < kDepthMaxLevels; ++k) {
    depth[k] = cnt[k] ? math::div_rn(sum[k], (float)cnt[k]) : 0.0f;
    reach[k] = math::div_by_recip((float)cnt[k], n, rn);
  }
}

}  // namespace vpt

// vpt_alpha.h — the coverage (alpha) pass: the optical depth of a primary ray by a deterministic march.
//
// Under delta tracking a primary ray has no real collision with probability exp(-sigma_t * integral of rho ds),
// the integral running over the positive-majorant segments of RayMajorantIterator (a segment with majorant <= 0
// draws nothing, vpt_integrator.h SM_NEED_SEG).  optical_depth() walks those segments with the integrator's own
// begin_ray / begin_segment / hdda_step, evaluates the integrator's trilinear field at e + d * t (eval_collision's
// expression) and integrates it exactly: between two crossings of the integer lattice planes the field along the
// ray is a cubic of t, which Simpson's rule integrates without error.  No random numbers: a matte without noise.
//
// The march is written once: matte_march() walks the segments, matte_segment() a segment's lattice pieces, and a
// visitor sees every piece.  The coverage pass's visitor does nothing; the depth pass's (vpt_depth.h) tests the
// accumulated optical depth against its levels and stops the ray at the last one.  Both passes therefore make the
// same cuts and form the same sums, which is what "a depth level is reached exactly where the matte's tau reaches
// it" and the temporal pass's reprojection rest on.
//
// __host__ __device__: vpt_alpha_kernel (vpt_kernels.h) and the host harness (tests/native/matte_host.cpp) run the
// same code.  Only +, * and the correctly rounded helpers of vpt_math.h, contraction off: the same bits on both.
// (expf in alpha_pixel is the platform's: the alpha plane agrees within 2^-22, the tau plane bit for bit.)
#pragma once

#include "../../include/vpt_gpu.h"
#include "vpt_integrator.h"

namespace vpt {

constexpr uint32_t kAlphaMaxSub = 8;          // sub-rays per axis: 1..8
constexpr int32_t kAlphaMaxSteps = 1 << 16;   // HDDA steps per ray (vpt_tile_cost_kernel's guard)
constexpr float kAlphaMaxPieces = 1048576.f;  // lattice pieces per segment

// The camera ray of a raster point: ST_PIXEL's expressions (Camera::generate_ray, camera.hpp:14-23), in its order.
__host__ __device__ inline void alpha_camera_dir(const DevScene& S, float rx, float ry, float dv[3]) {
  for (int i = 0; i < 3; ++i) dv[i] = S.cam_t[i] + (S.cam_L[i * 3] * rx + (S.cam_L[i * 3 + 1] * ry + S.cam_L[i * 3 + 2] * 0.0f));
  const float n2 = dv[0] * dv[0] + (dv[1] * dv[1] + dv[2] * dv[2]);
  if (n2 > 0.0f) {
    const float s = math::sqrt_rn(n2), rs = math::recip_for_div(s);
    dv[0] = math::div_by_recip(dv[0], s, rs);
    dv[1] = math::div_by_recip(dv[1], s, rs);
    dv[2] = math::div_by_recip(dv[2], s, rs);
  }
}

// The density at time t of the lane's index-space ray.
__host__ __device__ __forceinline__ float alpha_field(const DevGrid& G, const Lane& ln, StencilCell& sc, float t) {
  float v;
  trilinear(G, sc, ln.e[0] + ln.d[0] * t, ln.e[1] + ln.d[1] * t, ln.e[2] + ln.d[2] * t, v);
  return v;
}

// What matte_segment's visitor sees after each lattice piece; c = sigma_t * scale and total = the ray's sum over its
// earlier segments are what it needs to form the ray's tau so far.
struct MattePiece {
  float ta, tb, fa;   // the piece [ta, tb] (index-space ray time) and the field at ta
  float before, sum;  // the segment's sum before and with the piece
  float total, c;
};

// 6 x the integral of the field over [t0, t1] of the lane's ray (index-space time).  The segment is cut where
// the ray crosses an integer plane of any axis: per axis the next plane k (an integer) and its time
// (k - e) * inv -- computed from k every time, never accumulated, so the times of one axis are monotone in k and
// the cut sequence (their running minimum, clamped to [ta, t1]) never steps back.  Each piece adds
// (tb - ta) * ((f(ta) + 4 f(tm)) + f(tb)); f(tb) is the next piece's f(ta).  The loop runs at most `bound` times,
// a count taken from the segment's extent before it starts.  After each piece piece(MattePiece, ln, sc) sees it and
// returns whether the ray stops there (`stop`: the segment ends, and matte_march's walk with it).
template <class Piece>
__host__ __device__ inline float matte_segment(const DevGrid& G, const Lane& ln, StencilCell& sc, const float inv[3], float t0,
                                               float t1, float c, float total, bool& stop, Piece& piece) {
  if (!(t1 > t0)) return 0.0f;
  int32_t k[3], st[3];
  float tc[3], ext = 8.0f;  // pieces <= 4 + sum |d_a| (t1 - t0); the rest covers this sum's own rounding
  for (int a = 0; a < 3; ++a) {
    const float p = ln.e[a] + ln.d[a] * t0;
    st[a] = hdda_stp(ln.d[a], inv[a]);
    if (!(fabsf(p) < 0x1p30f)) return 0.0f;  // (no lattice to walk: a degenerate ray)
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
    for (int a = 0; a < 3; ++a) {  // the planes reached: every axis whose time is tn (selects, as hdda_advance)
      const bool hit = !last && st[a] != 0 && tc[a] <= tn;
      k[a] += hit ? st[a] : 0;
      tc[a] = hit ? ((float)k[a] - ln.e[a]) * inv[a] : tc[a];
    }
    const float h = tb - ta;
    const float fm = alpha_field(G, ln, sc, ta + 0.5f * h), fb = alpha_field(G, ln, sc, tb);
    const float before = sum;
    sum = sum + h * ((fa + 4.0f * fm) + fb);
    stop = piece(MattePiece{ta, tb, fa, before, sum, total, c}, ln, sc);
    ta = tb;
    fa = fb;
    if (last || stop) break;
  }
  return sum;
}

// The march of one world ray (o, dir) over its positive-majorant segments; with Cut each is cut at the index-space
// time t_cut, without it t_cut is not read and the whole ray is marched (compile time: the passes' kernels pay no
// compare for a cut they do not make, and a segment's end reaches matte_segment as hdda_step left it).  Two-level sum:
// pieces into their segment (matte_segment), segments into the ray's `total`, which is 6 / (sigma_t * scale) x the
// optical depth; scale = the ray's world length per unit of index-space time, set for every direction.  Ends when the
// ray does, at t_cut, or when the visitor says stop.  Returns false, total = 0, for no ray.
template <bool Cut, class Piece>
__host__ __device__ inline bool matte_march(const DevScene& S, const float o[3], const float dir[3], float t_cut, float& total,
                                            float& scale, Piece piece) {
  const DevGrid& G = S.density;
  Lane ln;
  lane_init(ln);
  const RayDir rd = ray_dir_setup(G, dir);
  scale = rd.scale;
  total = 0.0f;
  if (!(rd.len > 0.0f && rd.len < 3.40282347e+38f)) return false;  // a zero or non-finite direction: no ray
  if (!begin_ray(G, ln, o, rd)) return false;                      // (it misses the clip box)
  const float inv[3] = {math::rcp_rn(ln.d[0]), math::rcp_rn(ln.d[1]), math::rcp_rn(ln.d[2])};
  StencilCell sc = {kNoCell, kNoCell, kNoCell, -1};
  const float c = S.sigma_t * ln.scale;
  int32_t steps = 0;
  bool stop = false;
  while (!stop && ln.s_t1 < ln.T1 && (!Cut || ln.s_t1 < t_cut) && steps < kAlphaMaxSteps) {
    begin_segment(ln);
    bool done;
    do {
      ++steps;
      done = hdda_step(G, ln);
    } while (!done && steps < kAlphaMaxSteps);
    if (ln.s_dmaj <= 0.0f) continue;  // no draw there (SM_NEED_SEG's rule)
    const float t1 = Cut ? (ln.s_t1 < t_cut ? ln.s_t1 : t_cut) : ln.s_t1;
    total = total + matte_segment(G, ln, sc, inv, ln.s_t0, t1, c, total, stop, piece);
  }
  return true;
}

// The optical depth of one world ray up to the index-space time t_cut, before its clamp at 0: with every positive
// segment cut at t_cut the last piece is [ta, t_cut] -- the expression the depth pass's bisection tests.  (Without
// Cut: of the whole ray.)  +0.0 for no ray; *scale_out (if not null) = the ray's scale.
template <bool Cut = true>
__host__ __device__ inline float optical_depth_upto(const DevScene& S, const float o[3], const float dir[3], float t_cut,
                                                    float* scale_out) {
  float total, scale;
  const bool ray =
      matte_march<Cut>(S, o, dir, t_cut, total, scale, [](const MattePiece&, const Lane&, StencilCell&) { return false; });
  if (scale_out) *scale_out = scale;
  return ray ? (S.sigma_t * scale) * math::div_rn(total, 6.0f) : 0.0f;
}

// The optical depth sigma_t * integral of rho ds of one world ray over its positive-majorant segments; +0.0 for a
// ray that misses the clip box.
__host__ __device__ inline float optical_depth(const DevScene& S, const float o[3], const float dir[3]) {
  const float tau = optical_depth_upto<false>(S, o, dir, 0.0f, nullptr);
  return tau > 0.0f ? tau : 0.0f;  // (a NaN as well)
}

// The sub-rays of pixel (px, py): s x s camera directions in row-major order over the jitter's footprint
// [px + 0.5, px + 0.5 + jitter_scale) (one ray without jitter), each handed to fn(dv).  Returns the rays per axis.
template <class Fn>
__host__ __device__ inline uint32_t matte_subrays(const DevScene& S, int32_t px, int32_t py, uint32_t s, Fn fn) {
  const uint32_t sub = S.jitter_scale != 0.0f ? s : 1u;
  const float fs = (float)sub, rs = math::recip_for_div(fs);
  for (uint32_t j = 0; j < sub; ++j)
    for (uint32_t i = 0; i < sub; ++i) {
      const float rx = ((float)px + 0.5f) + S.jitter_scale * math::div_by_recip((float)i + 0.5f, fs, rs);
      const float ry = ((float)py + 0.5f) + S.jitter_scale * math::div_by_recip((float)j + 0.5f, fs, rs);
      float dv[3];
      alpha_camera_dir(S, rx, ry, dv);
      fn(dv);
    }
  return sub;
}

// One pixel of the matte over its sub-rays: T = (sum exp(-tau_k)) / n in their order, alpha = 1 - T,
// tau = (sum tau_k) / n.
__host__ __device__ inline void alpha_pixel(const DevScene& S, int32_t px, int32_t py, uint32_t s, float& alpha, float& tau) {
  float sum_t = 0.0f, sum_tau = 0.0f;
  const uint32_t sub = matte_subrays(S, px, py, s, [&](const float dv[3]) {
    const float t = optical_depth(S, S.cam_pos, dv);
    sum_tau = sum_tau + t;
    sum_t = sum_t + expf(-t);
  });
  const float n = (float)(sub * sub), rn = math::recip_for_div(n);
  alpha = 1.0f - math::div_by_recip(sum_t, n, rn);
  tau = math::div_by_recip(sum_tau, n, rn);
}

}  // namespace vpt

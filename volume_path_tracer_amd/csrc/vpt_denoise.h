// vpt_denoise.h — the denoiser: a variance-guided a-trous (with holes) filter over a film and its moment plane.
//
// The ordered film passes keep, per pixel, the sum of (imaging_ratio * L.y)^2 (the moment plane), so the variance of
// every pixel's mean Y is known per pixel whatever wave count its tile stopped at.  The filter smooths the means
// c = xyz / n with a 5 x 5 B3-spline kernel at steps 1, 2, 4, ..: a tap's weight falls off rationally,
// 1 / (1 + d^2), with its distance in Y measured in local standard deviations and with its distance in each guide
// plane (the matte's alpha and tau / (1 + tau): a cloud's stand-ins for albedo and normal), and the variance of the
// mean is propagated through every iteration (v' = sum w^2 v / (sum w)^2), so later, wider iterations see a
// smaller sigma and stop blurring what the earlier ones have already resolved.
//
// The arithmetic (normative; include/vpt_gpu.h "Denoise" states it, tests/denoise_ref.py restates it in numpy):
// fp32, not contracted, only + - * /, sqrtf, fabsf and comparisons, in the order written below, divisions and
// square roots correctly rounded -- the same bits from vpt_denoise_*_kernel, from the host build of these
// functions (tests/native/denoise_host.cpp) and from numpy.
//
// Planes.  prepare packs (c.x, c.y, c.z, v) into one float4 per pixel and the G guides into a second (unused lanes
// +0); an invalid pixel (not n >= 1: unrendered, NaN) is packed as (0, 0, 0, -1): v < 0 marks it, v >= 0 (or NaN)
// is a valid pixel, so a tap is one 16-byte load (two with guides) and needs no third plane.  An invalid pixel is
// never a tap (a select, not a multiplication by 0) and its output is its input, copied.
#pragma once

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

namespace vpt {

constexpr uint32_t kDenoiseMaxIterations = 6;
constexpr uint32_t kDenoiseMaxGuides = 4;
constexpr uint32_t kDenoiseBlockX = 64, kDenoiseBlockY = 4;  // a wavefront owns 64 consecutive pixels of one row

struct DenoiseArgs {
  int32_t W, H;
  float sigma_l, rel_floor;
  float guide_sigma[4];
};

__host__ __device__ __forceinline__ bool denoise_valid(const float4& cv) { return !(cv.w < 0.0f); }

// Prepare: c = xyz / n;  n >= 2: v = max(m2 / n - c.y c.y, 0) / (n - 1)  (vpt_gpu_tile_errors' se^2, its order);
// n == 1 (any 1 <= n < 2): v = c.y c.y.
__host__ __device__ inline float4 denoise_prepare_pixel(const float4& f, float m2) {
  const float n = f.w;
  if (!(n >= 1.0f)) return make_float4(0.0f, 0.0f, 0.0f, -1.0f);
  float4 cv;
  cv.x = f.x / n;
  cv.y = f.y / n;
  cv.z = f.z / n;
  if (n >= 2.0f) {
    const float ex2 = m2 / n;
    float v = ex2 - cv.y * cv.y;
    if (!(v > 0.0f)) v = 0.0f;
    cv.w = v / (n - 1.0f);
  } else {
    cv.w = cv.y * cv.y;
  }
  return cv;
}

__host__ __device__ __forceinline__ float denoise_lane(const float4& g, int k) {
  return k == 0 ? g.x : k == 1 ? g.y : k == 2 ? g.z : g.w;
}

// One iteration at pixel (x, y), step s, of the packed planes `cv` and `gd` ([H][W] float4; gd unused when G == 0):
//   gv  = (sum b v_q) / (sum b) over the valid in-image 3 x 3 neighbours at unit spacing, row-major,
//         b = b3[dy] * b3[dx], b3 = {1/4, 1/2, 1/4};
//   den = (sigma_l * sqrtf(gv) + rel_floor * c_p.y) + 1e-20f;
//   for dy = -2..2, dx = -2..2 (dy outer), q = p + s (dx, dy) in the image and valid:
//     d = fabsf(c_p.y - c_q.y) / den;  w = (h[dy] * h[dx]) / (1 + d d),  h = {1/16, 1/4, 3/8, 1/4, 1/16};
//     for k < G: e = (g_k[p] - g_k[q]) / guide_sigma[k];  w = w / (1 + e e);
//     acc += w c_q;  accv += (w w) v_q;  ws += w;
//   c' = acc / ws;  v' = accv / (ws ws).
// The centre tap always counts: ws > 0.  An invalid p returns its own packed value.
template <int G>
__host__ __device__ inline float4 denoise_atrous_pixel(const float4* cv, const float4* gd, const DenoiseArgs& A, int32_t x,
                                                       int32_t y, int32_t s) {
  const size_t p = (size_t)y * (size_t)A.W + (size_t)x;
  const float4 cp = cv[p];
  if (!denoise_valid(cp)) return cp;
  float4 gp = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  if (G > 0) gp = gd[p];
  const float b3[3] = {0.25f, 0.5f, 0.25f};
  const float h5[5] = {0.0625f, 0.25f, 0.375f, 0.25f, 0.0625f};
  float gs = 0.0f, gw = 0.0f;
#pragma unroll
  for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
    for (int dx = -1; dx <= 1; ++dx) {
      const int32_t qx = x + dx, qy = y + dy;
      if (qx < 0 || qx >= A.W || qy < 0 || qy >= A.H) continue;
      const float4 cq = cv[(size_t)qy * (size_t)A.W + (size_t)qx];
      if (!denoise_valid(cq)) continue;
      const float b = b3[dy + 1] * b3[dx + 1];
      gs = gs + b * cq.w;
      gw = gw + b;
    }
  const float gv = gs / gw;
  const float den = (A.sigma_l * sqrtf(gv) + A.rel_floor * cp.y) + 1e-20f;
  float ax = 0.0f, ay = 0.0f, az = 0.0f, av = 0.0f, ws = 0.0f;
#pragma unroll
  for (int dy = -2; dy <= 2; ++dy)
#pragma unroll
    for (int dx = -2; dx <= 2; ++dx) {
      // (64-bit: a step of 32 times a tap offset of 2 leaves int32 only for images no plane could hold, but the
      // bounds test must not depend on that)
      const int64_t qx = (int64_t)x + (int64_t)s * dx, qy = (int64_t)y + (int64_t)s * dy;
      if (qx < 0 || qx >= A.W || qy < 0 || qy >= A.H) continue;
      const size_t q = (size_t)qy * (size_t)A.W + (size_t)qx;
      const float4 cq = cv[q];
      if (!denoise_valid(cq)) continue;
      const float d = fabsf(cp.y - cq.y) / den;
      float w = (h5[dy + 2] * h5[dx + 2]) / (1.0f + d * d);
      if (G > 0) {
        const float4 gq = gd[q];
#pragma unroll
        for (int k = 0; k < G; ++k) {
          const float e = (denoise_lane(gp, k) - denoise_lane(gq, k)) / A.guide_sigma[k];
          w = w / (1.0f + e * e);
        }
      }
      ax = ax + w * cq.x;
      ay = ay + w * cq.y;
      az = az + w * cq.z;
      av = av + (w * w) * cq.w;
      ws = ws + w;
    }
  return make_float4(ax / ws, ay / ws, az / ws, av / (ws * ws));
}

// Finish: a valid pixel's film is (c n, n) with the input's n; an invalid pixel's is the input, copied.  The
// variance plane receives the final v, +0 at an invalid pixel.
__host__ __device__ inline float4 denoise_finish_pixel(const float4& cv, const float4& f, float& var) {
  if (!denoise_valid(cv)) {
    var = 0.0f;
    return f;
  }
  var = cv.w;
  return make_float4(cv.x * f.w, cv.y * f.w, cv.z * f.w, f.w);
}

#if defined(__HIPCC__) && !defined(VPT_DENOISE_NO_KERNELS)  // (the host harness takes the per-pixel functions alone)
// Blocks of 64 x 4 threads; thread (tx, ty) of block (bx, by) owns pixel (64 bx + tx, 4 by + ty).  Fixed bounds,
// no atomics, nothing shared between blocks or lanes; no kernel reads a plane it writes.
struct DenoiseGuidePtrs {
  const float* g[4];
};

__global__ __launch_bounds__(256) void vpt_denoise_prepare_kernel(DenoiseArgs A, uint32_t n_guides, const float4* film,
                                                                  const float* m2, DenoiseGuidePtrs guides, float4* cv,
                                                                  float4* gd) {
  const int32_t x = (int32_t)(blockIdx.x * kDenoiseBlockX + threadIdx.x), y = (int32_t)(blockIdx.y * kDenoiseBlockY + threadIdx.y);
  if (x >= A.W || y >= A.H) return;
  const size_t p = (size_t)y * (size_t)A.W + (size_t)x;
  cv[p] = denoise_prepare_pixel(film[p], m2[p]);
  if (n_guides) {  // (uniform)
    float4 g = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    g.x = guides.g[0][p];
    if (n_guides > 1) g.y = guides.g[1][p];
    if (n_guides > 2) g.z = guides.g[2][p];
    if (n_guides > 3) g.w = guides.g[3][p];
    gd[p] = g;
  }
}

// One iteration.  LAST: the finish is fused -- the result goes to the caller's film (and variance plane, when
// given) instead of the other packed plane.
template <int G, bool LAST>
__global__ __launch_bounds__(256) void vpt_denoise_atrous_kernel(DenoiseArgs A, int32_t step, const float4* src,
                                                                 const float4* gd, float4* dst, const float4* film,
                                                                 float4* out_film, float* var_out) {
  const int32_t x = (int32_t)(blockIdx.x * kDenoiseBlockX + threadIdx.x), y = (int32_t)(blockIdx.y * kDenoiseBlockY + threadIdx.y);
  if (x >= A.W || y >= A.H) return;
  const size_t p = (size_t)y * (size_t)A.W + (size_t)x;
  const float4 r = denoise_atrous_pixel<G>(src, gd, A, x, y, step);
  if (LAST) {
    float var;
    out_film[p] = denoise_finish_pixel(r, film[p], var);
    if (var_out) var_out[p] = var;
  } else {
    dst[p] = r;
  }
}
#endif  // kernels

}  // namespace vpt

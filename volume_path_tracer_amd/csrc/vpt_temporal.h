// vpt_temporal.h — temporal accumulation: the previous frame's accumulated film, reprojected through the current
// frame's depth plane and added to the current film.
//
// A film is sums and a count, so history is added, not blended: a pixel's depth gives its world point, the previous
// camera gives the raster point that point had, four bilinear taps of the history there give a mean, a second moment
// and a sample count, a rational rejection on the distance in Y (in standard deviations of both estimates) scales the
// count down, and n_h samples of that mean are added to the pixel's sums.  The result is an ordinary film with a
// matching moment plane: every film consumer, the denoiser included, takes it unchanged, and it is the next frame's
// history together with this frame's depth planes and camera.
//
// The arithmetic (normative; include/vpt_gpu.h "Temporal" states it, tests/temporal_ref.py restates it in numpy): fp32,
// not contracted, only + - * /, sqrtf, floorf, fabsf, comparisons and selects, in the order written below, divisions
// and square roots correctly rounded -- the same bits from vpt_temporal_kernel, from the host build of these functions
// (tests/native/temporal_host.cpp) and from numpy.  dot(u, v) below is always u0 v0 + (u1 v1 + u2 v2).
#pragma once

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

namespace vpt {

constexpr uint32_t kTemporalMaxLevels = 4;                     // VPT_DEPTH_MAX_LEVELS
constexpr uint32_t kTemporalBlockX = 64, kTemporalBlockY = 4;  // a wavefront owns 64 consecutive pixels of one row
constexpr float kTemporalMinWeight = 0.25f;  // usable bilinear weight below which there is no history: one far corner
                                             // tap is not blown up by the renormalisation
constexpr float kTemporalFltMax = 3.40282347e+38f;

// Kernel arguments (by value: scalar loads).  cur: the current camera in the shutter table's layout,
// [4 i .. 4 i + 3] = cam_L[3 i], cam_L[3 i + 1], cam_L[3 i + 2], cam_t[i] (i = 0, 1, 2), [12 .. 14] = cam_pos.
// The previous camera as its projection constants (temporal_prev_constants).
struct TemporalArgs {
  int32_t W, H;
  uint32_t n_levels;
  int32_t has_history;
  float max_history, depth_tol, sigma_r, rel_floor;
  float cur[16];
  float pn[3], pa[3], pb[3];  // n = L0' x L1',  a = (L1' x n) / (n . n),  b = (n x L0') / (n . n)
  float ptn, pta, ptb;        // t' . n,  t' . a,  t' . b
  float ppos[3];
};

// The previous camera's constants from its 16 floats, once, on the host, in fp32 in this order (L0', L1': the first
// two columns of cam_L, t' = cam_t).  A raster point (rx, ry) of that camera sees the direction t' + L0' rx + L1' ry;
// for a direction q, lambda = (t' . n) / (q . n), rx = lambda (q . a) - t' . a, ry = lambda (q . b) - t' . b solve
// t' + L0' rx + L1' ry = lambda q  (L0' . a = L1' . b = 1, L1' . a = L0' . b = 0, n is normal to both).
inline void temporal_cross(const float u[3], const float v[3], float o[3]) {
  o[0] = u[1] * v[2] - u[2] * v[1];
  o[1] = u[2] * v[0] - u[0] * v[2];
  o[2] = u[0] * v[1] - u[1] * v[0];
}
__host__ __device__ __forceinline__ float temporal_dot(const float u[3], const float v[3]) {
  return u[0] * v[0] + (u[1] * v[1] + u[2] * v[2]);
}
inline void temporal_prev_constants(const float prev[16], TemporalArgs& A) {
  const float c0[3] = {prev[0], prev[4], prev[8]}, c1[3] = {prev[1], prev[5], prev[9]}, t[3] = {prev[3], prev[7], prev[11]};
  float a[3], b[3];
  temporal_cross(c0, c1, A.pn);
  const float nn = temporal_dot(A.pn, A.pn);
  temporal_cross(c1, A.pn, a);
  temporal_cross(A.pn, c0, b);
  for (int i = 0; i < 3; ++i) {
    A.pa[i] = a[i] / nn;
    A.pb[i] = b[i] / nn;
    A.ppos[i] = prev[12 + i];
  }
  A.ptn = temporal_dot(t, A.pn);
  A.pta = temporal_dot(t, A.pa);
  A.ptb = temporal_dot(t, A.pb);
}

// z(p): depth[k][p] for the largest k < n_levels with depth[k][p] > 0, +0 when none is (background).  Selects over a
// fixed trip count (k is uniform; an indexed read of a per-lane level would go to scratch).
__host__ __device__ __forceinline__ float temporal_depth(const float* depth, uint32_t n_levels, size_t N, size_t p) {
  float z = 0.0f;
#pragma unroll
  for (uint32_t k = 0; k < kTemporalMaxLevels; ++k)
    if (k < n_levels) {
      const float dk = depth[(size_t)k * N + p];
      z = dk > 0.0f ? dk : z;
    }
  return z;
}

__host__ __device__ __forceinline__ bool temporal_finite(float v) { return fabsf(v) <= kTemporalFltMax; }

struct TemporalPixel {
  float4 film;
  float m2, mx, my, hn;
};

// One pixel p = (x, y).
//   z = temporal_depth(depth, p); foreground iff z > 0.
//   rx = (float)x + 0.5f, ry = (float)y + 0.5f;  dv_i = t_i + (L_i0 rx + (L_i1 ry + L_i2 0.0f));
//   n2 = dv0 dv0 + (dv1 dv1 + dv2 dv2);  n2 > 0: d = dv / sqrtf(n2)      (Camera::generate_ray, the integrator's order)
//   foreground: q = (pos + z d) - pos',  r = sqrtf(q . q);   background: q = d.
//   lambda = ptn / (q . pn);  px = lambda (q . pa) - pta;  py = lambda (q . pb) - ptb;
//   projected iff lambda > 0 and lambda, px, py are finite;  motion = (px - rx, py - ry), else a NaN pair.
//   fx = px - 0.5f, fy = py - 0.5f; in range iff -1 < fx < W and -1 < fy < H; x0 = floorf(fx), ax = fx - x0 (y alike).
//   Taps (x0, y0), (x0 + 1, y0), (x0, y0 + 1), (x0 + 1, y0 + 1) with w = (1 - ax)(1 - ay), ax (1 - ay), (1 - ax) ay,
//   ax ay; usable iff in the image, n_q >= 1 and: foreground z_q > 0 and fabsf(z_q - r) <= depth_tol r; background
//   not z_q > 0.  Per usable tap, in turn:
//     ws += w;  s.xyz += w (xyz_q / n_q);  sm += w (m2_q / n_q);  sn += w n_q.
//   History iff has_history, n_c >= 1, projected, in range and ws >= 0.25f:
//     c_h = s / ws;  s_h = sm / ws;  n_0 = sn / ws;  c_c = xyz / n_c;
//     v_c = n_c >= 2 ? max(m2 / n_c - c_c.y c_c.y, 0) / (n_c - 1) : c_c.y c_c.y         (the denoiser's prepare)
//     v_h = max(s_h - c_h.y c_h.y, 0) / max(n_0 - 1, 1);
//     e = fabsf(c_c.y - c_h.y) / ((sigma_r sqrtf(v_c + v_h) + rel_floor c_c.y) + 1e-20f);
//     n_h = min(n_0, max_history) / (1 + e e);
//   and iff n_h > 0 (a NaN or a fully rejected history adds nothing):
//     out.xyz = xyz + n_h c_h;  out.w = n_c + n_h;  out_m2 = m2 + n_h s_h;  hist_n = n_h.
//   Every other pixel passes through: film and plane are the inputs' bytes, hist_n = +0.
__host__ __device__ inline TemporalPixel temporal_pixel(const TemporalArgs& A, const float4* film, const float* m2,
                                                        const float* depth, const float4* hist_film, const float* hist_m2,
                                                        const float* hist_depth, int32_t x, int32_t y) {
  const size_t N = (size_t)A.W * (size_t)A.H, p = (size_t)y * (size_t)A.W + (size_t)x;
  const float4 f = film[p];
  const float mp = m2[p];
  TemporalPixel o;
  o.film = f;
  o.m2 = mp;
  o.hn = 0.0f;
  const float z = temporal_depth(depth, A.n_levels, N, p);
  const bool fg = z > 0.0f;
  const float rx = (float)x + 0.5f, ry = (float)y + 0.5f;
  float d[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) d[i] = A.cur[4 * i + 3] + (A.cur[4 * i] * rx + (A.cur[4 * i + 1] * ry + A.cur[4 * i + 2] * 0.0f));
  const float n2 = d[0] * d[0] + (d[1] * d[1] + d[2] * d[2]);
  if (n2 > 0.0f) {
    const float s = sqrtf(n2);
    d[0] = d[0] / s;
    d[1] = d[1] / s;
    d[2] = d[2] / s;
  }
  float q[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) q[i] = fg ? (A.cur[12 + i] + z * d[i]) - A.ppos[i] : d[i];
  const float r = sqrtf(temporal_dot(q, q));
  const float lam = A.ptn / temporal_dot(q, A.pn);
  const float px = lam * temporal_dot(q, A.pa) - A.pta, py = lam * temporal_dot(q, A.pb) - A.ptb;
  const bool proj = lam > 0.0f && temporal_finite(lam) && temporal_finite(px) && temporal_finite(py);
  const float nanv = __builtin_nanf("");
  o.mx = proj ? px - rx : nanv;
  o.my = proj ? py - ry : nanv;
  const float nc = f.w;
  const float fx = px - 0.5f, fy = py - 0.5f;
  // (the range is tested before any conversion to an integer)
  const bool in = proj && fx > -1.0f && fx < (float)A.W && fy > -1.0f && fy < (float)A.H;
  if (!A.has_history || !(nc >= 1.0f) || !in) return o;
  const float x0f = floorf(fx), y0f = floorf(fy);
  const float ax = fx - x0f, ay = fy - y0f;
  const int32_t x0 = (int32_t)x0f, y0 = (int32_t)y0f;
  const float bx = 1.0f - ax, by = 1.0f - ay;
  const float w4[4] = {bx * by, ax * by, bx * ay, ax * ay};
  const float tol = A.depth_tol * r;
  float ws = 0.0f, sx = 0.0f, sy = 0.0f, sz = 0.0f, sm = 0.0f, sn = 0.0f;
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const int32_t tx = x0 + (t & 1), ty = y0 + (t >> 1);
    if (tx < 0 || tx >= A.W || ty < 0 || ty >= A.H) continue;
    const size_t tq = (size_t)ty * (size_t)A.W + (size_t)tx;
    const float4 hf = hist_film[tq];
    const float hm = hist_m2[tq];
    const float zq = temporal_depth(hist_depth, A.n_levels, N, tq);
    const float nq = hf.w;
    const bool agree = fg ? (zq > 0.0f && fabsf(zq - r) <= tol) : !(zq > 0.0f);
    const bool ok = nq >= 1.0f && agree;
    const float w = w4[t];
    // (selects: what an excluded tap holds is computed with and dropped)
    const float cx = hf.x / nq, cy = hf.y / nq, cz = hf.z / nq, cm = hm / nq;
    ws = ok ? ws + w : ws;
    sx = ok ? sx + w * cx : sx;
    sy = ok ? sy + w * cy : sy;
    sz = ok ? sz + w * cz : sz;
    sm = ok ? sm + w * cm : sm;
    sn = ok ? sn + w * nq : sn;
  }
  if (!(ws >= kTemporalMinWeight)) return o;
  const float hx = sx / ws, hy = sy / ws, hz = sz / ws, sh = sm / ws, n0 = sn / ws;
  const float ccy = f.y / nc;
  float vc;
  if (nc >= 2.0f) {
    float v = mp / nc - ccy * ccy;
    if (!(v > 0.0f)) v = 0.0f;
    vc = v / (nc - 1.0f);
  } else {
    vc = ccy * ccy;
  }
  float dh = sh - hy * hy;
  if (!(dh > 0.0f)) dh = 0.0f;
  float nm1 = n0 - 1.0f;
  if (!(nm1 > 1.0f)) nm1 = 1.0f;
  const float vh = dh / nm1;
  const float e = fabsf(ccy - hy) / ((A.sigma_r * sqrtf(vc + vh) + A.rel_floor * ccy) + 1e-20f);
  const float nm = n0 < A.max_history ? n0 : A.max_history;
  const float nh = nm / (1.0f + e * e);
  if (!(nh > 0.0f)) return o;
  o.film = make_float4(f.x + nh * hx, f.y + nh * hy, f.z + nh * hz, nc + nh);
  o.m2 = mp + nh * sh;
  o.hn = nh;
  return o;
}

#if defined(__HIPCC__) && !defined(VPT_TEMPORAL_NO_KERNELS)  // (the host harness takes the per-pixel function alone)
// Blocks of 64 x 4 threads; thread (tx, ty) of block (bx, by) owns pixel (64 bx + tx, 4 by + ty).  A tap is one
// 16-byte film load plus the plane's and the depth planes' dwords.  Fixed bounds, no LDS, no atomics, nothing shared
// between blocks or lanes; the kernel reads its inputs only and writes the four outputs.
__global__ __launch_bounds__(256) void vpt_temporal_kernel(TemporalArgs A, const float4* film, const float* m2,
                                                           const float* depth, const float4* hist_film, const float* hist_m2,
                                                           const float* hist_depth, float4* out_film, float* out_m2,
                                                           float* motion_out, float* hist_n_out) {
  const int32_t x = (int32_t)(blockIdx.x * kTemporalBlockX + threadIdx.x), y = (int32_t)(blockIdx.y * kTemporalBlockY + threadIdx.y);
  if (x >= A.W || y >= A.H) return;
  const size_t p = (size_t)y * (size_t)A.W + (size_t)x;
  const TemporalPixel o = temporal_pixel(A, film, m2, depth, hist_film, hist_m2, hist_depth, x, y);
  out_film[p] = o.film;
  out_m2[p] = o.m2;
  if (motion_out) {
    motion_out[2 * p] = o.mx;
    motion_out[2 * p + 1] = o.my;
  }
  if (hist_n_out) hist_n_out[p] = o.hn;
}
#endif  // kernel

}  // namespace vpt

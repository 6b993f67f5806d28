// Device functions of the forward-backward check: the sampling rule S, the
// inside test, the check rule and the point form built from them.  The rule
// itself is written down in csrc/fb_check.hip; csrc/fb_check.hip,
// csrc/multi_flow.hip and csrc/dense_flow.hip all inline these functions, so
// their kernels cannot drift apart.
#pragma once

#include "common.h"

namespace rs {
namespace fb {

__device__ __forceinline__ void tap(const float* __restrict__ fx, const float* __restrict__ fy, int H, int W,
                                    int xi, int yi, float w, float& u, float& v) {
  if (w != 0.f && xi >= 0 && xi < W && yi >= 0 && yi < H) {
    const int i = yi * W + xi;
    u += w * fx[i];
    v += w * fy[i];
  }
}

// fx, fy: the two planes of one image
__device__ __forceinline__ void sample(const float* __restrict__ fx, const float* __restrict__ fy, int H, int W,
                                       float x, float y, float& u, float& v) {
  u = 0.f;
  v = 0.f;
  if (!(x > -1.f && x < (float)W && y > -1.f && y < (float)H)) return;
  const float xf = floorf(x), yf = floorf(y);
  const float wx = x - xf, wy = y - yf;
  const float ux = 1.f - wx, uy = 1.f - wy;
  const int x0 = (int)xf, y0 = (int)yf;  // [-1, W-1], [-1, H-1]
  tap(fx, fy, H, W, x0, y0, __fmul_rn(ux, uy), u, v);
  tap(fx, fy, H, W, x0 + 1, y0, __fmul_rn(wx, uy), u, v);
  tap(fx, fy, H, W, x0, y0 + 1, __fmul_rn(ux, wy), u, v);
  tap(fx, fy, H, W, x0 + 1, y0 + 1, __fmul_rn(wx, wy), u, v);
}

__device__ __forceinline__ bool inside(float x, float y, int H, int W) {
  return x >= 0.f && x <= (float)(W - 1) && y >= 0.f && y <= (float)(H - 1);
}

__device__ __forceinline__ void check(const float* __restrict__ bx, const float* __restrict__ by, int H, int W,
                                      float px, float py, float u, float v, float a1, float a2, float& err,
                                      bool& ok) {
  const float qx = px + u, qy = py + v;
  err = INFINITY;
  ok = false;
  if (!inside(qx, qy, H, W)) return;
  float bu, bv;
  sample(bx, by, H, W, qx, qy, bu, bv);
  const float su = u + bu, sv = v + bv;
  const float e2 = su * su + sv * sv;
  const float m2 = u * u + v * v + bu * bu + bv * bv;
  err = sqrtf(e2);
  ok = e2 <= a1 * m2 + a2;
}

// The point form.  fx, bx: one image's forward and backward field, two planes
// each; (px, py) the start.  (ox, oy) = start + S(fw, start) always; a start
// outside [0,W-1]x[0,H-1] or non-finite gives ok = 0, err = +inf.
__device__ __forceinline__ void track_point(const float* __restrict__ fx, const float* __restrict__ bx,
                                            size_t plane, int H, int W, float px, float py, float a1, float a2,
                                            float& ox, float& oy, float& err, bool& ok) {
  float u, v;
  sample(fx, fx + plane, H, W, px, py, u, v);
  ox = px + u;
  oy = py + v;
  err = INFINITY;
  ok = false;
  if (inside(px, py, H, W)) check(bx, bx + plane, H, W, px, py, u, v, a1, a2, err, ok);
}

}  // namespace fb
}  // namespace rs

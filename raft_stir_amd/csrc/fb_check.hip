// Forward-backward consistency check of two optical-flow fields (Sundaram et
// al. 2010; the occlusion criterion of UnFlow): follow a point along the
// forward flow, read the backward flow where it lands and see whether it comes
// home.  Per image of two (B,2,H,W) fp32 flows fw (t -> t+1) and bw (t+1 -> t).
//
// Sampling rule S(f, x, y), bilinear in pixel coordinates (grid_sample with
// align_corners=True and zero padding, the rule of export/pointtrack.py
// sample_points):
//   live = x > -1 && x < W && y > -1 && y < H      (NaN / Inf / huge fail: S = 0, nothing is read)
//   x0 = floor(x), wx = x - x0, y0 = floor(y), wy = y - y0                       (fp32)
//   weights w00 = fl((1-wx)*(1-wy)), w01 = fl(wx*(1-wy)), w10 = fl((1-wx)*wy), w11 = fl(wx*wy)
//   S = w00*f[y0][x0] + w01*f[y0][x0+1] + w10*f[y0+1][x0] + w11*f[y0+1][x0+1]    (in this order)
//   a tap outside the image or of weight zero contributes nothing and is not read.
// Every comparison is made in float before any conversion to int, so x0 and y0
// are in [-1, W-1] / [-1, H-1] when they become ints and every address is
// checked against the image again.
//
// Check rule for a start (px, py) with forward vector (u, v):
//   qx = px + u, qy = py + v                                                      (fp32 sums)
//   inside = 0 <= qx <= W-1 && 0 <= qy <= H-1       (NaN fails)
//   not inside: err = +inf, ok = 0
//   inside:     (bu, bv) = S(bw, qx, qy)
//               e2 = (u+bu)^2 + (v+bv)^2,  m2 = u^2 + v^2 + bu^2 + bv^2
//               err = sqrt(e2),  ok = e2 <= alpha1*m2 + alpha2   (inclusive; any NaN gives 0)
//
//   fb_dense_kernel   every pixel centre is a start with (u, v) = fw at that pixel, read directly.
//                     One thread per pixel in 32x8 tiles, so that the eight gathers of neighbouring
//                     threads (which land near each other for a smooth flow) share cache lines.
//   fb_points_kernel  (B,N,2) xy points: (u, v) = S(fw, px, py), new = p + (u, v) always; a start
//                     outside [0,W-1]x[0,H-1] or non-finite gives ok = 0, err = +inf.  One thread
//                     per point.
// Both call fb::check, so the two forms cannot drift apart; the device
// functions are in csrc/fb_device.h, which csrc/multi_flow.hip shares.  No
// atomics and no dependence on the launch order: the ops are deterministic.
#include "common.h"
#include "fb_device.h"

namespace rs {
namespace fb {

constexpr int TILE_X = 32, TILE_Y = 8;
constexpr int THREADS = 256;

__global__ __launch_bounds__(TILE_X* TILE_Y) void fb_dense_kernel(const float* __restrict__ fw,
                                                                   const float* __restrict__ bw, int H, int W,
                                                                   float a1, float a2, float* __restrict__ err,
                                                                   bool* __restrict__ ok) {
  const int x = blockIdx.x * TILE_X + threadIdx.x;
  const int y = blockIdx.y * TILE_Y + threadIdx.y;
  if (x >= W || y >= H) return;
  const size_t plane = (size_t)H * W;
  const size_t b = blockIdx.z;
  const float* fx = fw + b * 2 * plane;
  const float* bx = bw + b * 2 * plane;
  const int i = y * W + x;
  float e;
  bool k;
  check(bx, bx + plane, H, W, (float)x, (float)y, fx[i], fx[plane + i], a1, a2, e, k);
  err[b * plane + i] = e;
  ok[b * plane + i] = k;
}

// points, out: [B][N][2]; err, ok: [B][N]
__global__ __launch_bounds__(THREADS) void fb_points_kernel(const float* __restrict__ fw,
                                                             const float* __restrict__ bw,
                                                             const float* __restrict__ points, int H, int W, int N,
                                                             float a1, float a2, float* __restrict__ out,
                                                             float* __restrict__ err, bool* __restrict__ ok) {
  const int n = blockIdx.x * THREADS + threadIdx.x;
  if (n >= N) return;
  const size_t plane = (size_t)H * W;
  const size_t b = blockIdx.y;
  const float* fx = fw + b * 2 * plane;
  const float* bx = bw + b * 2 * plane;
  const size_t p = b * N + n;
  const float px = points[2 * p], py = points[2 * p + 1];
  float ox, oy, e;
  bool k;
  track_point(fx, bx, plane, H, W, px, py, a1, a2, ox, oy, e, k);
  out[2 * p] = ox;
  out[2 * p + 1] = oy;
  err[p] = e;
  ok[p] = k;
}

}  // namespace fb

void fb_dense_launch(const float* fw, const float* bw, int B, int H, int W, float a1, float a2, float* err,
                     bool* ok, hipStream_t s) {
  hipLaunchKernelGGL(fb::fb_dense_kernel, dim3(cdiv(W, fb::TILE_X), cdiv(H, fb::TILE_Y), B),
                     dim3(fb::TILE_X, fb::TILE_Y), 0, s, fw, bw, H, W, a1, a2, err, ok);
}

void fb_points_launch(const float* fw, const float* bw, const float* points, int B, int H, int W, int N, float a1,
                      float a2, float* out, float* err, bool* ok, hipStream_t s) {
  hipLaunchKernelGGL(fb::fb_points_kernel, dim3(cdiv(N, fb::THREADS), B), dim3(fb::THREADS), 0, s, fw, bw, points,
                     H, W, N, a1, a2, out, err, ok);
}

}  // namespace rs

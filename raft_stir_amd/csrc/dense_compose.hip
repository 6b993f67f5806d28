// Composition of two dense track fields and the point form of reading one
// (ops/reference.py: dense_compose and dense_query are the rules).  The
// per-point rule is csrc/query_device.h, which a host program runs too
// (tests/host/dense_compose_host.cpp).
//
//   base_pos   [2][H][W]  where every pixel of the first anchor is in the
//                         frame of the current anchor (x, then y)
//   base_score [H][W]     finite iff the pixel is visible there
//   pos, score, delta, err  the inner field, current anchor -> t, planar
//   points     [N][2]     interleaved xy (the point form)
//
// dense_compose_kernel: one thread per pixel n.  Coalesced loads of the three
// base planes, up to four taps of the inner pos / score planes and one of
// delta / err (the only scattered reads; a smooth base keeps neighbouring
// threads on neighbouring cells), coalesced stores of the six output planes.
// dense_query_kernel: one thread per point, the same read of the field.
//
// One launch each on the caller's stream: no atomics, no LDS, no allocation,
// no synchronisation, so the op can be captured in a graph.  The result does
// not depend on any order: every thread writes its own outputs only.
//
// Safety:
//   * a position is converted to an integer only after the inside test on the
//     floats, and a tap's index is formed only after the bounds test on the
//     integers (query::read), so every gather lands in its plane;
//   * there is no data-dependent loop: four taps per thread;
//   * a thread beyond H*W (beyond N) returns before it reads or writes.
#include "common.h"
#include "query_device.h"

namespace rs {
namespace query {

constexpr int THREADS = 256;

__global__ __launch_bounds__(THREADS) void dense_compose_kernel(
    const float* __restrict__ base_pos, const float* __restrict__ base_score, const float* __restrict__ pos,
    const float* __restrict__ score, const int32_t* __restrict__ delta, const float* __restrict__ err, int H, int W,
    float* __restrict__ pos_c, float* __restrict__ score_c, bool* __restrict__ vis_c, int32_t* __restrict__ delta_c,
    float* __restrict__ err_c) {
  const int N = H * W;  // < 2^31: checked on the host
  const unsigned i = blockIdx.x * THREADS + threadIdx.x;  // N + 255 < 2^32
  if (i >= (unsigned)N) return;
  const int n = (int)i;
  const float bx = base_pos[n], by = base_pos[(size_t)N + n], bs = base_score[n];
  float ox, oy, s, e;
  int32_t d;
  const bool vis = compose(pos, pos + (size_t)N, score, delta, err, H, W, bx, by, bs, ox, oy, s, d, e);
  pos_c[n] = ox;
  pos_c[(size_t)N + n] = oy;
  score_c[n] = s;
  vis_c[n] = vis;
  delta_c[n] = d;
  err_c[n] = e;
}

__global__ __launch_bounds__(THREADS) void dense_query_kernel(const float* __restrict__ pos,
                                                              const float* __restrict__ score,
                                                              const float* __restrict__ points, int H, int W, int N,
                                                              float* __restrict__ out, bool* __restrict__ vis,
                                                              float* __restrict__ out_score) {
  const unsigned i = blockIdx.x * THREADS + threadIdx.x;
  if (i >= (unsigned)N) return;
  const size_t n = i;
  const float x = points[2 * n], y = points[2 * n + 1];  // no wider load: a view may start at an odd float
  float ox, oy, s;
  const bool seen = read(pos, pos + (size_t)H * W, score, H, W, x, y, ox, oy, s);
  out[2 * n] = ox;
  out[2 * n + 1] = oy;
  vis[n] = seen;
  out_score[n] = s;
}

}  // namespace query

void dense_compose_launch(const float* base_pos, const float* base_score, const float* pos, const float* score,
                          const int32_t* delta, const float* err, int H, int W, float* pos_c, float* score_c,
                          bool* vis_c, int32_t* delta_c, float* err_c, hipStream_t s) {
  const int N = H * W;
  const dim3 grid((unsigned)((N - 1) / query::THREADS + 1)), block(query::THREADS);
  hipLaunchKernelGGL(query::dense_compose_kernel, grid, block, 0, s, base_pos, base_score, pos, score, delta, err, H,
                     W, pos_c, score_c, vis_c, delta_c, err_c);
}

// N >= 1
void dense_query_launch(const float* pos, const float* score, const float* points, int H, int W, int N, float* out,
                        bool* vis, float* out_score, hipStream_t s) {
  const dim3 grid((unsigned)((N - 1) / query::THREADS + 1)), block(query::THREADS);
  hipLaunchKernelGGL(query::dense_query_kernel, grid, block, 0, s, pos, score, points, H, W, N, out, vis, out_score);
}

}  // namespace rs

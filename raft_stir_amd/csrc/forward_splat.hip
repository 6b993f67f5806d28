// Dense forward splatting (ops/reference.py: forward_splat is the rule): for
// every cell of the frame a dense track field points to, the anchor pixel
// that sits there.  The per-pixel rule is csrc/splat_device.h, which a host
// program runs too (tests/host/forward_splat_host.cpp).
//
//   pos    [2][H][W]  where every anchor pixel is in the target frame (x, then y)
//   score  [H][W]     finite iff the pixel is visible there
//   values [C][H][W]  carried along (C may be 0)
//   keys   [H][W] 64-bit, the caller's workspace: per cell the smallest offer
//
// Three launches on one stream:
//   1. clear    keys = kHole (all ones), one thread per cell
//   2. scatter  one thread per anchor pixel n: coalesced reads of x, y, s; if
//               n is a source, up to four atomicMin of its packed key
//               (class << 62 | score bits << 31 | n) on the cells it offers
//               itself to.  No thread reads keys.
//   3. resolve  one thread per cell: reads its key and writes src_index (-1 at
//               holes), covered, inv_pos (NaN at holes) and out[c] =
//               values[c][win] (fill at holes).  Coalesced stores; the gathers
//               of pos[win] and values[c][win] are the only scattered reads.
//
// Determinism: a cell's key is the minimum of the keys offered to it, and the
// integer minimum does not depend on the order of its operands.  So the result
// is the same bits as the oracle's in every run, with atomics and in any
// launch order of the blocks; the anchor index in the low bits makes every key
// unique, so there is no tie left to break.
//
// Plain mapping: 256 threads, no LDS.  A field that sends every source to one
// cell serialises its atomics on one address; that is a correctness case, not
// a speed target (a wave-level pre-reduction of equal cells would be the
// remedy if a smooth field ever ran far above its byte floor).
//
// Safety:
//   * a position or score is converted to an integer only after the source
//     test on the floats, and every cell index is formed only after the bounds
//     test on the integers (splat::offer), so every atomic lands in keys;
//   * every decoded winner is clamped to [0, N-1] whatever keys holds, so the
//     gathers stay inside pos and values even on a workspace that was not
//     cleared;
//   * there is no data-dependent loop: at most four offers per source, C
//     channels per cell;
//   * a thread beyond H*W returns before it reads or writes anything;
//   * the op allocates nothing and synchronises nothing: the three launches go
//     to the caller's stream and can be captured in a graph.
#include "common.h"
#include "splat_device.h"

namespace rs {
namespace splat {

constexpr int THREADS = 256;

__global__ __launch_bounds__(THREADS) void splat_clear_kernel(unsigned long long* __restrict__ keys, int N) {
  const unsigned i = blockIdx.x * THREADS + threadIdx.x;  // N + 255 < 2^32
  if (i >= (unsigned)N) return;
  keys[i] = kHole;
}

__global__ __launch_bounds__(THREADS) void splat_scatter_kernel(const float* __restrict__ pos,
                                                                const float* __restrict__ score, int footprint, int H,
                                                                int W, unsigned long long* keys) {
  const int N = H * W;  // < 2^31: checked on the host
  const unsigned i = blockIdx.x * THREADS + threadIdx.x;
  if (i >= (unsigned)N) return;
  const int n = (int)i;
  const float x = pos[n], y = pos[(size_t)N + n], s = score[n];
  if (!is_source(x, y, s, H, W)) return;
  const uint32_t bits = score_bits(s);
  int cell[kMaxOffers], cls[kMaxOffers];
  const int k = offers(x, y, footprint, H, W, cell, cls);
#pragma unroll
  for (int j = 0; j < kMaxOffers; ++j)
    if (j < k) atomicMin(keys + cell[j], (unsigned long long)make_key(cls[j], bits, n));
}

__global__ __launch_bounds__(THREADS) void splat_resolve_kernel(const unsigned long long* __restrict__ keys,
                                                                const float* __restrict__ pos,
                                                                const float* __restrict__ values, int C, float fill,
                                                                int H, int W, int* __restrict__ src_index,
                                                                bool* __restrict__ cov, float* __restrict__ inv_pos,
                                                                float* __restrict__ out) {
  const int N = H * W;
  const unsigned i = blockIdx.x * THREADS + threadIdx.x;
  if (i >= (unsigned)N) return;
  const int c = (int)i;
  const uint64_t key = keys[c];
  const bool hit = covered(key);
  const int win = winner(key, N);  // in [0, N-1] at a hole too
  float ix = NAN, iy = NAN;
  if (hit) {
    ix = inverse(win % W, c % W, pos[win]);
    iy = inverse(win / W, c / W, pos[(size_t)N + win]);
  }
  src_index[c] = hit ? win : -1;
  cov[c] = hit;
  inv_pos[c] = ix;
  inv_pos[(size_t)N + c] = iy;
  for (int ch = 0; ch < C; ++ch) out[(size_t)ch * N + c] = hit ? values[(size_t)ch * N + win] : fill;
}

}  // namespace splat

// keys: H*W 64-bit words; values and out: nullptr iff C == 0
void forward_splat_launch(const float* pos, const float* score, const float* values, int C, int footprint, float fill,
                          int H, int W, unsigned long long* keys, int* src_index, bool* covered, float* inv_pos,
                          float* out, hipStream_t s) {
  const int N = H * W;
  const dim3 grid((unsigned)((N - 1) / splat::THREADS + 1)), block(splat::THREADS);
  hipLaunchKernelGGL(splat::splat_clear_kernel, grid, block, 0, s, keys, N);
  hipLaunchKernelGGL(splat::splat_scatter_kernel, grid, block, 0, s, pos, score, footprint, H, W, keys);
  hipLaunchKernelGGL(splat::splat_resolve_kernel, grid, block, 0, s, keys, pos, values, C, fill, H, W, src_index,
                     covered, inv_pos, out);
}

}  // namespace rs

// Backward warp of an image through a field of positions
// (ops/reference.py: backward_warp is the rule).  The per-pixel rule is
// csrc/warp_device.h, which a host program runs too
// (tests/host/backward_warp_host.cpp).
//
//   image   T[...]: C channels of Hs x Ws, float or uint8_t, read in place
//           through its element strides (channel, row, column): planar or
//           channels-last
//   coords  [2][H][W]  x, then y: where every output cell reads the image
//   valid   [H][W] bytes or null
//   warped  T[C][H][W] planar; ok [H][W]
//
// backward_warp_kernel: one thread per output cell n, looping over the
// channels.  Coalesced loads of the two coords planes and of valid, coalesced
// stores of the C output planes and of ok; the only scattered reads are the up
// to four taps, which a smooth field keeps on neighbouring pixels for
// neighbouring threads.  A channels-last source puts a tap's C values next to
// each other (PACK: warp::pixel_packed, the taps outside, the channels
// inside): with C = 4 and an aligned image they are one 4-byte (uint8) or
// 16-byte (fp32) load per tap, with C = 3 one 12-byte load (fp32) or a 2-byte
// and a 1-byte load (uint8: a tap's three bytes start at any address, and a
// 4-byte load would read past the last pixel).  C = 1, 3, 4 are compile-time
// loop counts; any other C <= 16 runs the same loop with the count at run
// time.
//
// No LDS and some tens of VGPRs: the block size is not what limits occupancy.
// 256 threads are four waves, a row segment of 256 cells: 1 KiB per coords
// plane and per fp32 output plane.
//
// One launch on the caller's stream: no atomics, no allocation, no
// synchronisation, so the op can be captured in a graph.  Every thread writes
// its own outputs only.
//
// Safety:
//   * a position is converted to an integer only after the inside test on the
//     floats, and a tap's offset is formed only after the bounds test on the
//     integers (warp::taps), so every read lands in the image;
//   * there is no data-dependent loop: four taps and C channels per thread;
//   * a thread beyond H*W returns before it reads or writes.
#include "common.h"
#include "warp_device.h"

namespace rs {
namespace warp {

constexpr int THREADS = 256;

template <typename T, int CT, bool PACK>
__global__ __launch_bounds__(THREADS) void backward_warp_kernel(const T* __restrict__ img, int64_t sc, int64_t sy,
                                                                int64_t sx, int C, int Hs, int Ws,
                                                                const float* __restrict__ coords,
                                                                const uint8_t* __restrict__ valid, int N, T fill,
                                                                T* __restrict__ out, bool* __restrict__ ok) {
  const unsigned i = blockIdx.x * THREADS + threadIdx.x;  // N + 255 < 2^32
  if (i >= (unsigned)N) return;
  const int n = (int)i;
  const float x = coords[n], y = coords[(size_t)N + n];
  const bool v = valid ? valid[n] != 0 : true;
  if (PACK)  // four channels: the whole group is aligned; three: its elements are
    ok[n] = pixel_packed<T, CT ? CT : 1, (CT == 4 ? 4 : 1) * (int)sizeof(T)>(img, sy, sx, Hs, Ws, x, y, v, fill, out,
                                                                            (int64_t)N, (int64_t)n);
  else
    ok[n] = pixel(img, sc, sy, sx, CT ? CT : C, Hs, Ws, x, y, v, fill, out, (int64_t)N, (int64_t)n);
}

template <typename T>
void launch(const T* img, int64_t sc, int64_t sy, int64_t sx, int C, int Hs, int Ws, const float* coords,
            const uint8_t* valid, int H, int W, T fill, T* out, bool* ok, hipStream_t s) {
  const int N = H * W;  // < 2^31: checked on the host
  const dim3 grid((unsigned)((N - 1) / THREADS + 1)), block(THREADS);
  // channels that lie together: one read of the group per tap; four need every pixel's group aligned
  const bool pack4 = C == 4 && sc == 1 && sx == 4 && sy % 4 == 0 && (uintptr_t)img % (4 * sizeof(T)) == 0;
  const bool pack3 = C == 3 && sc == 1 && sx == 3;
#define RS_WARP_LAUNCH(CT, PACK)                                                                                   \
  hipLaunchKernelGGL((backward_warp_kernel<T, CT, PACK>), grid, block, 0, s, img, sc, sy, sx, C, Hs, Ws, coords, \
                     valid, N, fill, out, ok)
  if (pack4)
    RS_WARP_LAUNCH(4, true);
  else if (pack3)
    RS_WARP_LAUNCH(3, true);
  else if (C == 1)
    RS_WARP_LAUNCH(1, false);
  else if (C == 3)
    RS_WARP_LAUNCH(3, false);
  else if (C == 4)
    RS_WARP_LAUNCH(4, false);
  else
    RS_WARP_LAUNCH(0, false);
#undef RS_WARP_LAUNCH
}

}  // namespace warp

void backward_warp_f32_launch(const float* img, int64_t sc, int64_t sy, int64_t sx, int C, int Hs, int Ws,
                              const float* coords, const uint8_t* valid, int H, int W, float fill, float* out,
                              bool* ok, hipStream_t s) {
  warp::launch(img, sc, sy, sx, C, Hs, Ws, coords, valid, H, W, fill, out, ok, s);
}

void backward_warp_u8_launch(const uint8_t* img, int64_t sc, int64_t sy, int64_t sx, int C, int Hs, int Ws,
                             const float* coords, const uint8_t* valid, int H, int W, uint8_t fill, uint8_t* out,
                             bool* ok, hipStream_t s) {
  warp::launch(img, sc, sy, sx, C, Hs, Ws, coords, valid, H, W, fill, out, ok, s);
}

}  // namespace rs

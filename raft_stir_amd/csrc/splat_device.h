// The per-pixel rule of dense forward splatting (ops/reference.py:
// forward_splat), written once as inline functions for the kernels of
// csrc/forward_splat.hip and for a plain C++ program on the host
// (tests/host/forward_splat_host.cpp), which runs the same index arithmetic
// under AddressSanitizer and UBSan.  Nothing from HIP is included: under hipcc
// the functions are __host__ __device__, under any other compiler plain inline.
//
//   source  0 <= s < +inf  &&  -1 < x < W  &&  -1 < y < H, decided on the
//           floats before any conversion to int (NaN fails every comparison;
//           converting NaN, an infinity or 1e30 would be undefined)
//   bits    the bit pattern of s + 0.0f, taken without arithmetic (-0 -> +0),
//           so no float mode can flush a denormal score
//   offers  footprint 1: the nearest cell (rintf: halves to even), class 0;
//           footprint 2: the cells (floor + {0,1}) whose bilinear weight, one
//           fp32 product as fb::sample forms it, is != 0; class 0 iff the
//           cell is the nearest cell.  An offer outside the image is dropped,
//           tested on the integers, and only then is the cell index formed.
//   key     class << 62 | bits << 31 | n, compared as unsigned 64-bit; kHole,
//           all ones, is above every key
//   decode  covered = key != kHole; win = key & 0x7fffffff, clamped to
//           [0, N-1] whatever the key holds; inv = g(win) + (g(cell) - pos[win])
#pragma once

#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define RS_SPLAT_FN __host__ __device__ inline
#else
#define RS_SPLAT_FN inline
#endif

namespace rs {
namespace splat {

constexpr uint64_t kHole = ~uint64_t(0);
constexpr int kMaxOffers = 4;

RS_SPLAT_FN bool is_source(float x, float y, float s, int H, int W) {
  return s >= 0.f && s < INFINITY && x > -1.f && x < (float)W && y > -1.f && y < (float)H;
}

// of a source's score: s >= 0, finite, so bit 31 is clear once -0 is +0
RS_SPLAT_FN uint32_t score_bits(float s) {
  uint32_t b;
  __builtin_memcpy(&b, &s, sizeof(b));
  return b == 0x80000000u ? 0u : b;
}

// one fp32 product, rounded once
RS_SPLAT_FN float weight(float a, float b) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __fmul_rn(a, b);
#else
  return a * b;  // nothing to contract with; host callers build with contraction off all the same
#endif
}

RS_SPLAT_FN uint64_t make_key(int cls, uint32_t bits, int n) {
  return ((uint64_t)cls << 62) | ((uint64_t)bits << 31) | (uint64_t)(uint32_t)n;
}

// (xi, yi) offered by a source whose nearest cell is (nx, ny); made: its weight
// is != 0.  True iff the offer is made and lands in the image; cell and cls
// are set only then.
RS_SPLAT_FN bool offer(int xi, int yi, bool made, int nx, int ny, int H, int W, int& cell, int& cls) {
  if (!(made && xi >= 0 && xi < W && yi >= 0 && yi < H)) return false;
  cell = yi * W + xi;  // H*W < 2^31: checked by the caller
  cls = (xi != nx || yi != ny) ? 1 : 0;
  return true;
}

// The offers of a source (is_source holds, so every conversion below is of a
// float in (-1, W) or (-1, H)).  -> their number, at most kMaxOffers.
RS_SPLAT_FN int offers(float x, float y, int footprint, int H, int W, int (&cell)[kMaxOffers],
                       int (&cls)[kMaxOffers]) {
  const int nx = (int)rintf(x), ny = (int)rintf(y);  // [-1, W], [-1, H]
  int k = 0;
  if (footprint == 1) {
    if (offer(nx, ny, true, nx, ny, H, W, cell[k], cls[k])) ++k;
    return k;
  }
  const float xf = floorf(x), yf = floorf(y);
  const float wx = x - xf, wy = y - yf;
  const float ux = 1.f - wx, uy = 1.f - wy;
  const int x0 = (int)xf, y0 = (int)yf;  // [-1, W-1], [-1, H-1]
  if (offer(x0, y0, weight(ux, uy) != 0.f, nx, ny, H, W, cell[k], cls[k])) ++k;
  if (offer(x0 + 1, y0, weight(wx, uy) != 0.f, nx, ny, H, W, cell[k], cls[k])) ++k;
  if (offer(x0, y0 + 1, weight(ux, wy) != 0.f, nx, ny, H, W, cell[k], cls[k])) ++k;
  if (offer(x0 + 1, y0 + 1, weight(wx, wy) != 0.f, nx, ny, H, W, cell[k], cls[k])) ++k;
  return k;
}

RS_SPLAT_FN bool covered(uint64_t key) { return key != kHole; }

// the winner of a key, in [0, N-1] whatever the key holds
RS_SPLAT_FN int winner(uint64_t key, int N) {
  const int w = (int)(key & 0x7fffffffu);
  return w < N ? w : N - 1;
}

// one axis of inv_pos: the winner's grid coordinate, the cell's, and the
// winner's position; two fp32 operations in this order
RS_SPLAT_FN float inverse(int g_win, int g_cell, float p_win) { return (float)g_win + ((float)g_cell - p_win); }

}  // namespace splat
}  // namespace rs

// The per-pixel rule of the backward warp of an image (ops/reference.py:
// backward_warp), written once as inline functions for the kernels of
// csrc/backward_warp.hip and for a plain C++ program on the host
// (tests/host/backward_warp_host.cpp), which runs the same index arithmetic
// under AddressSanitizer and UBSan.  The sampling rule is that of
// query_device.h (inside, taps, sample), whose mul, add and inside are used
// here; nothing from HIP is included.
//
//   image   T = float or uint8_t, C channels of Hs x Ws pixels, addressed by
//           three element strides (channel, row, column): a planar image is
//           (Hs*Ws, Ws, 1), a channels-last one (1, Ws*C, C).  Offsets are
//           64-bit: Hs*Ws < 2^31 and C <= 16.
//   taps    decided once per pixel: which of the four are read, their weights
//           and their offsets.  A tap's offset is formed only after the
//           bounds test on the integers; a tap that is not read has none.
//   sample  per channel u = 0; u = u + w * f[i] per tap read, in tap order,
//           products and sums rounded once.  The packed form (three or four
//           channels that lie together, read as one group per tap) walks the
//           taps outside and the channels inside: per channel the same sums
//           in the same order, so the same bits.
//   store   float: u.  uint8_t: clamp(rint(u), 0, 255), halves to even.
#pragma once

#include <string.h>

#include "query_device.h"

namespace rs {
namespace warp {

using query::add;
using query::mul;

struct Taps {
  float w[4];
  int64_t off[4];  // element offset of channel 0; 0 for a tap that is not read
  unsigned use;    // bit j: tap j is read
};

// (x, y) must be inside (query::inside with Hs, Ws): the conversions are defined
RS_QUERY_FN Taps taps(float x, float y, int Hs, int Ws, int64_t sy, int64_t sx) {
  const float xf = floorf(x), yf = floorf(y);
  const float wx = x - xf, wy = y - yf;
  const float ux = 1.f - wx, uy = 1.f - wy;
  const int x0 = (int)xf, y0 = (int)yf;  // [0, Ws-1], [0, Hs-1]
  Taps t;
  t.w[0] = mul(ux, uy);
  t.w[1] = mul(wx, uy);
  t.w[2] = mul(ux, wy);
  t.w[3] = mul(wx, wy);
  t.use = 0;
  for (int j = 0; j < 4; ++j) {
    const int xi = x0 + (j & 1), yi = y0 + (j >> 1);  // >= 0
    t.off[j] = 0;
    if (t.w[j] != 0.f && xi < Ws && yi < Hs) {
      t.off[j] = yi * sy + xi * sx;
      t.use |= 1u << j;
    }
  }
  return t;
}

RS_QUERY_FN float store(float u, float) { return u; }
RS_QUERY_FN uint8_t store(float u, uint8_t) {
  const float r = rintf(u);  // u is a finite sum of at most four products in [0, 255]
  return (uint8_t)(r < 0.f ? 0.f : r > 255.f ? 255.f : r);
}

// one channel whose first element is ``img``
template <typename T>
RS_QUERY_FN T sample(const T* img, const Taps& t) {
  float u = 0.f;
  for (int j = 0; j < 4; ++j)
    if (t.use >> j & 1) u = add(u, mul(t.w[j], (float)img[t.off[j]]));
  return store(u, T());
}

// One pixel n of the output: C channels to out[c * N + n], fill where not ok.
// valid: one byte per pixel or null.  -> ok
template <typename T>
RS_QUERY_FN bool pixel(const T* img, int64_t sc, int64_t sy, int64_t sx, int C, int Hs, int Ws, float x, float y,
                       bool valid, T fill, T* out, int64_t N, int64_t n) {
  const bool in = query::inside(x, y, Hs, Ws);
  const bool ok = valid && in;
  Taps t;
  if (ok) t = taps(x, y, Hs, Ws, sy, sx);
  for (int c = 0; c < C; ++c) out[c * N + n] = ok ? sample(img + c * sc, t) : fill;
  return ok;
}

// The same pixel for C channels that lie together (sc = 1), every pixel's
// group aligned to ALIGN bytes: one read of the group per tap, C * sizeof(T)
// bytes (one load instruction where the alignment allows it).
template <typename T, int C, int ALIGN>
RS_QUERY_FN bool pixel_packed(const T* img, int64_t sy, int64_t sx, int Hs, int Ws, float x, float y, bool valid,
                              T fill, T* out, int64_t N, int64_t n) {
  const bool in = query::inside(x, y, Hs, Ws);
  const bool ok = valid && in;
  if (!ok) {
    for (int c = 0; c < C; ++c) out[c * N + n] = fill;
    return false;
  }
  const Taps t = taps(x, y, Hs, Ws, sy, sx);
  float u[C];
  for (int c = 0; c < C; ++c) u[c] = 0.f;
  for (int j = 0; j < 4; ++j)
    if (t.use >> j & 1) {
      T v[C];
      memcpy(v, __builtin_assume_aligned(img + t.off[j], ALIGN), C * sizeof(T));
      for (int c = 0; c < C; ++c) u[c] = add(u[c], mul(t.w[j], (float)v[c]));
    }
  for (int c = 0; c < C; ++c) out[c * N + n] = store(u[c], T());
  return true;
}

}  // namespace warp
}  // namespace rs

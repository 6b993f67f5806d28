// The per-point rule of reading a dense track field (ops/reference.py:
// dense_query) and of composing two of them (dense_compose), written once as
// inline functions for the kernels of csrc/dense_compose.hip and for a plain
// C++ program on the host (tests/host/dense_compose_host.cpp), which runs the
// same index arithmetic under AddressSanitizer and UBSan.  Nothing from HIP is
// included: under hipcc the functions are __host__ __device__, under any other
// compiler plain inline.
//
//   inside  0 <= x <= W-1 && 0 <= y <= H-1, decided on the floats before any
//           conversion to int (NaN fails every comparison; converting NaN, an
//           infinity or 1e30 would be undefined).  A point that is not inside
//           comes back unchanged, not visible, with score +inf.
//   taps    (floor x + {0,1}, floor y + {0,1}) in the order (0,0), (1,0),
//           (0,1), (1,1); a weight is one fp32 product of (1 - wx | wx) and
//           (1 - wy | wy).  A tap of weight 0, or at column W or row H, is
//           never read; only after that test on the integers is its index
//           formed.
//   sample  u = 0; u = u + w * f[i] per tap read, every product and every sum
//           rounded once (never contracted to an FMA): at an integer point the
//           stored value itself.
//   worst   the maximum of the scores at the taps read, NaN if one of them is
//           NaN (fmaxf would drop it); visible iff worst < +inf
//   compose s = base_score + worst, one fp32 sum; visible iff s < +inf; the
//           class-0 cell (rintf: halves to even) of an inside position is a
//           pixel of the frame
#pragma once

#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define RS_QUERY_FN __host__ __device__ inline
#else
#define RS_QUERY_FN inline
#endif

namespace rs {
namespace query {

// One fp32 product and one fp32 sum, each rounded once.  Not __fmul_rn and
// __fadd_rn: hipcc's headers define them as the plain operators, compiled with
// the default -ffp-contract=fast-honor-pragmas, so that a product inlined next
// to a sum is fused into an FMA all the same.  The pragma takes the contract
// flag off the operation itself, here, where it is written; host callers build
// with -ffp-contract=off.
RS_QUERY_FN float mul(float a, float b) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  return a * b;
}

RS_QUERY_FN float add(float a, float b) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  return a + b;
}

RS_QUERY_FN bool inside(float x, float y, int H, int W) {
  return x >= 0.f && x <= (float)(W - 1) && y >= 0.f && y <= (float)(H - 1);
}

// the larger of two scores, NaN if either is (as torch.maximum)
RS_QUERY_FN float worse(float m, float s) {
  if (m != m || s != s) return NAN;
  return s > m ? s : m;
}

// px, py, sc: the two position planes and the score plane of one field, H*W
// each (H*W < 2^31: checked by the caller).  (x, y) -> the position (ox, oy)
// and the score; true iff visible.
RS_QUERY_FN bool read(const float* px, const float* py, const float* sc, int H, int W, float x, float y, float& ox,
                      float& oy, float& score) {
  ox = x;
  oy = y;
  score = INFINITY;
  if (!inside(x, y, H, W)) return false;
  const float xf = floorf(x), yf = floorf(y);
  const float wx = x - xf, wy = y - yf;
  const float ux = 1.f - wx, uy = 1.f - wy;
  const int x0 = (int)xf, y0 = (int)yf;  // [0, W-1], [0, H-1]
  const float w[4] = {mul(ux, uy), mul(wx, uy), mul(ux, wy), mul(wx, wy)};
  float u = 0.f, v = 0.f, m = -INFINITY;
  for (int j = 0; j < 4; ++j) {
    const int xi = x0 + (j & 1), yi = y0 + (j >> 1);  // >= 0
    if (w[j] != 0.f && xi < W && yi < H) {
      const int i = yi * W + xi;
      u = add(u, mul(w[j], px[i]));
      v = add(v, mul(w[j], py[i]));
      m = worse(m, sc[i]);
    }
  }
  ox = u;
  oy = v;
  score = m;
  return m < INFINITY;
}

// the class-0 cell of a position for which inside() holds
RS_QUERY_FN int nearest_cell(float x, float y, int W) { return (int)rintf(y) * W + (int)rintf(x); }

// One pixel of the composition.  (bx, by, bs): the base field at this pixel;
// delta, err: the inner field's planes.  -> true iff visible.
RS_QUERY_FN bool compose(const float* px, const float* py, const float* sc, const int32_t* delta, const float* err,
                         int H, int W, float bx, float by, float bs, float& ox, float& oy, float& score,
                         int32_t& d, float& e) {
  float q;
  const bool seen = read(px, py, sc, H, W, bx, by, ox, oy, q);
  const float s = add(bs, q);
  const bool vis = seen && s < INFINITY;
  score = INFINITY;
  d = -1;
  e = INFINITY;
  if (vis) {
    const int c = nearest_cell(bx, by, W);  // seen: (bx, by) is inside
    score = s;
    d = delta[c];
    e = err[c];
  }
  return vis;
}

}  // namespace query
}  // namespace rs

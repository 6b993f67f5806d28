// The per-cell rule of hole in-painting after a forward splat (ops/reference.py:
// splat_inpaint), written once as inline functions for the kernels of
// csrc/splat_inpaint.hip and for a plain C++ program on the host
// (tests/host/splat_inpaint_host.cpp), which runs the same index arithmetic
// under AddressSanitizer and UBSan.  Nothing from HIP is included: under hipcc
// the functions are __host__ __device__, under any other compiler plain inline.
//
//   entry    an entry s of src_index counts as clamp(s, -1, N-1): below 0 a
//            hole, N and above the last anchor pixel; never trusted as an index
//   covered  s >= 0
//   column   for cell (x, y) the nearest covered row y' of column x with
//            |y - y'| <= R, y - d tested before y + d (the lower cell index
//            wins the tie); -1 if there is none.  d runs to min(R, H-1).
//   key      d2 << 31 | c', d2 = dx^2 + dy^2 < 2^31, c' < 2^31, compared as
//            unsigned 64-bit; kNone, all ones, is above every key
//   row      for cell (x, y) the smallest key over x' = x -+ dx, dx = 0 ..
//            min(R, W-1), of column x''s row at y, taken only if d2 <= R*R.
//            The scan stops once dx*dx exceeds the best d2 so far (every later
//            key is larger; dx <= R keeps dx*dx <= R*R).  A column's nearest row minimises d2
//            for every x, and its tie went to the lower index, so the minimum
//            over the columns' keys is the minimum over all covered cells.
//   decode   donor = key & 0x7fffffff, dist2 = key >> 31, both -1 at kNone;
//            donor and the anchor pixel it names are clamped to [0, N-1]
//            before anything is read through them
//   fill     inv = g(win) + (g(cell) - pos[win]) per axis: splat::inverse
#pragma once

#include "splat_device.h"

namespace rs {
namespace inpaint {

constexpr uint64_t kNone = ~uint64_t(0);
constexpr int kMaxSide = 32767;  // H, W and R: d2 <= 2 * 32766^2 < 2^31, R*R < 2^31, H*W < 2^31

// an entry of src_index as the rule reads it: in [-1, N-1]
RS_SPLAT_FN int clamp_src(int s, int N) { return s < 0 ? -1 : (s < N ? s : N - 1); }

// a cell or anchor index, in [0, N-1] whatever i holds
RS_SPLAT_FN int clamp_cell(int i, int N) { return i < 0 ? 0 : (i < N ? i : N - 1); }

RS_SPLAT_FN bool covered(int s) { return s >= 0; }

// the nearest covered row of column x for row y, or -1; src: src_index[H*W].
// At most 2 * min(R, H-1) + 1 reads, each of a row tested to be in [0, H-1].
RS_SPLAT_FN int column_nearest(const int* src, int x, int y, int R, int H, int W) {
  const int dmax = R < H - 1 ? R : H - 1;
  for (int d = 0; d <= dmax; ++d) {
    const int up = y - d, down = y + d;
    if (up >= 0 && covered(src[up * W + x])) return up;  // H*W < 2^31: checked by the caller
    if (d > 0 && down < H && covered(src[down * W + x])) return down;
  }
  return -1;
}

RS_SPLAT_FN uint64_t make_key(int d2, int cell) { return ((uint64_t)(uint32_t)d2 << 31) | (uint64_t)(uint32_t)cell; }

// the d2 of a key, for the scan's stop test: above every d2 at kNone
RS_SPLAT_FN int64_t key_d2(uint64_t key) { return (int64_t)(key >> 31); }

// Column xc offers its row yc (-1: nothing; anything else outside [0, H-1] is
// dropped too) to cell (x, y), dx = |x - xc|: the smaller of best and its key.
RS_SPLAT_FN uint64_t candidate(uint64_t best, int xc, int yc, int dx, int y, int R2, int H, int W) {
  if (yc < 0 || yc >= H) return best;
  const int dy = y - yc;
  const int d2 = dx * dx + dy * dy;  // < 2^31: both below 32767
  if (d2 > R2) return best;
  const uint64_t key = make_key(d2, yc * W + xc);
  return key < best ? key : best;
}

// The smallest key of cell (x, y).  row[xc - base] is column xc's row at y for
// every xc in [lo, hi), a range that holds every xc in [x - R, x + R] that is
// in [0, W-1]; nothing outside [lo, hi) is read.  At most 2 * min(R, W-1) + 1
// steps.
RS_SPLAT_FN uint64_t row_nearest(const int* row, int base, int lo, int hi, int x, int y, int R, int H, int W) {
  const int R2 = R * R;
  const int dmax = R < W - 1 ? R : W - 1;
  uint64_t best = kNone;
  for (int dx = 0; dx <= dmax; ++dx) {
    if ((int64_t)dx * dx > key_d2(best)) break;  // dx <= R: dx*dx <= R*R already
    const int left = x - dx, right = x + dx;
    if (left >= lo && left < hi) best = candidate(best, left, row[left - base], dx, y, R2, H, W);
    if (dx > 0 && right >= lo && right < hi) best = candidate(best, right, row[right - base], dx, y, R2, H, W);
  }
  return best;
}

RS_SPLAT_FN int donor_of(uint64_t key) { return key == kNone ? -1 : (int)(key & 0x7fffffffu); }
RS_SPLAT_FN int dist2_of(uint64_t key) { return key == kNone ? -1 : (int)((key >> 31) & 0x7fffffffu); }

// What the apply pass writes at cell c = (x, y) from its donor (-1: none).
// Every index is clamped before it is used; inv_in is read at c only.
struct Filled {
  int src;       // the anchor pixel, -1 at a hole
  int win;       // in [0, N-1] at a hole too
  float ix, iy;  // NaN at a hole
};

RS_SPLAT_FN Filled apply(int c, int donor, const int* src, const float* pos, const float* inv_in, int H, int W) {
  const int N = H * W;
  const int dn = clamp_cell(donor, N);
  const int s = clamp_src(src[dn], N);
  const bool hit = donor >= 0 && covered(s);
  Filled f;
  f.win = clamp_cell(s, N);
  f.src = hit ? s : -1;
  f.ix = NAN;
  f.iy = NAN;
  if (hit && dn == c) {  // its own donor: the input's value, bit for bit
    f.ix = inv_in[c];
    f.iy = inv_in[(size_t)N + c];
  } else if (hit) {
    f.ix = splat::inverse(f.win % W, c % W, pos[f.win]);
    f.iy = splat::inverse(f.win / W, c / W, pos[(size_t)N + f.win]);
  }
  return f;
}

}  // namespace inpaint
}  // namespace rs

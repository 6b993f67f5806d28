// Coordinate -> cell index conversion shared by the correlation kernels
// (corr_lookup.hip, corr_onthefly.hip).
#pragma once

#include "common.h"

namespace rs {

// floor(coordinate) -> integer cell index.  The value is clamped in float to
// +-2^24 first (exactly representable, far outside any pyramid level), so the
// conversion is defined for every input -- huge, infinite, NaN (fmaxf maps it
// to the lower bound) -- and index arithmetic of a few window widths on the
// result cannot overflow.  A clamped index lies outside every level: zero
// padding in the forward, nothing touched in the backward.  The fractional
// weights come from the unclamped value (0 for a huge coordinate, NaN for a
// non-finite one, which turns that pixel's output into NaN).
constexpr float kCellClamp = 16777216.f;
__device__ __forceinline__ int cell_index(float floored) {
  return (int)fminf(fmaxf(floored, -kCellClamp), kCellClamp);
}

// Bounding box of a 4 x 4 query tile's windows: true when it has at most
// max_cells cells.  Each extent is tested before the product is formed (the
// origins are cell_index values, so an extent is at most 2^25 + E and the
// product of two extents <= max_cells fits an int).
__device__ __forceinline__ bool box_fits(int bw, int bh, int max_cells) {
  return bw <= max_cells && bh <= max_cells && bw * bh <= max_cells;
}

}  // namespace rs

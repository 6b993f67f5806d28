// In-painting of the holes a forward splat leaves (ops/reference.py:
// splat_inpaint is the rule): every cell takes the nearest covered cell within
// max_dist as its donor, in exact integer Euclidean distance, the lowest cell
// index among equals.  The per-cell rule is csrc/inpaint_device.h, which a
// host program runs too (tests/host/splat_inpaint_host.cpp).
//
//   src_index [H][W] int32  the splat's anchor pixel per cell, < 0 at holes
//   pos       [2][H][W]     where every anchor pixel is in the target frame
//   inv_in    [2][H][W]     the splat's inv_pos, kept at covered cells
//   values    [C][H][W]     carried along (C may be 0)
//   col       [H][W] int32  the caller's workspace: per cell the nearest covered
//                           row of its column within R, or -1
//
// Three launches on one stream:
//   1. column  one thread per cell: walks d = 0 .. min(R, H-1) up and down its
//              column of src_index and stops at the first covered row.  A wave
//              reads 64 neighbouring cells of one row per step; the rows it
//              returns to stay in L2.
//   2. row     one block per (row, segment of SEG = 256 cells), one thread per
//              cell: the minimum packed key over the columns x -+ dx of its
//              row, stopping once dx*dx exceeds the best d2.  The block reads
//              col for [x0 - R, x0 + SEG + R), clipped to the row.  When that
//              span, at most min(W, SEG + 2R) cells, fits the tile of
//              STAGE = 2048 cells (8 KiB of LDS: W <= 2048, or R <= 896) it is
//              staged in LDS with coalesced loads and the scan reads LDS;
//              consecutive lanes read consecutive words, so there is no bank
//              conflict beyond the wave's own divergence.  A wider span is
//              read in place through L2.  RS_INPAINT_STAGE=0 selects the
//              in-place scan for every shape, to compare the two
//              (profiles/splat_inpaint).  Writes donor and dist2.
//   3. apply   one thread per cell: src_index, inv_pos and out from the donor.
//
// Determinism: every cell's result is a minimum over integers that only its
// own thread forms; there is no atomic and no value passed between threads
// except col, which launch 1 completes before launch 2 reads it.
//
// Safety:
//   * every loop is bounded by R, H or W (2 * min(R, H-1) + 1 column steps,
//     2 * min(R, W-1) + 1 row steps, C channels), never by data alone;
//   * every index is formed only after its bounds test on the integers: a row
//     y -+ d against [0, H-1], a column x -+ dx against the staged range, which
//     lies in [0, W-1]; a col entry outside [0, H-1] is dropped, so a workspace
//     of garbage cannot send a read anywhere;
//   * an entry of src_index is read as clamp(s, -1, N-1) and a donor as
//     clamp(d, 0, N-1) before pos, values or src_index are read through them;
//   * a thread beyond H*W (launches 1, 3) returns before it reads or writes;
//     in launch 2 a thread beyond the row takes part in the staging loop and
//     the barrier and returns after it;
//   * the outputs must not alias the inputs (checked on the host): launch 3
//     reads src_index at other cells than its own;
//   * the op allocates nothing and synchronises nothing: the three launches go
//     to the caller's stream and can be captured in a graph.
#include "common.h"
#include "inpaint_device.h"

#include <cstdlib>

namespace rs {
namespace inpaint {

constexpr int THREADS = 256;
constexpr int SEG = THREADS;  // cells of a row per block of the row pass
constexpr int STAGE = 2048;   // cells of col a block stages in LDS

__global__ __launch_bounds__(THREADS) void inpaint_column_kernel(const int* __restrict__ src, int R, int H, int W,
                                                                 int* __restrict__ col) {
  const int N = H * W;  // < 2^31: checked on the host
  const unsigned i = blockIdx.x * THREADS + threadIdx.x;
  if (i >= (unsigned)N) return;
  const int c = (int)i;
  col[c] = column_nearest(src, c % W, c / W, R, H, W);
}

template <bool STAGED>
__global__ __launch_bounds__(THREADS) void inpaint_row_kernel(const int* __restrict__ col, int R, int H, int W,
                                                              int* __restrict__ donor, int* __restrict__ dist2) {
  __shared__ int tile[STAGED ? STAGE : 1];
  const int y = (int)blockIdx.y;  // < H: the grid's
  const int x0 = (int)blockIdx.x * SEG;
  // R, x0 + SEG <= 2 * 32767: no overflow
  const int lo = x0 - R > 0 ? x0 - R : 0;
  const int hi = x0 + SEG + R < W ? x0 + SEG + R : W;  // lo < hi <= W; hi - lo <= STAGE when STAGED (host)
  const int* row = col + (size_t)y * W;
  if (STAGED) {
    for (int j = (int)threadIdx.x; j < hi - lo && j < STAGE; j += THREADS) tile[j] = row[lo + j];
    __syncthreads();
  }
  const int x = x0 + (int)threadIdx.x;
  if (x >= W) return;
  const uint64_t key =
      STAGED ? row_nearest(tile, lo, lo, hi, x, y, R, H, W) : row_nearest(row, 0, lo, hi, x, y, R, H, W);
  const size_t c = (size_t)y * W + x;
  donor[c] = donor_of(key);
  dist2[c] = dist2_of(key);
}

__global__ __launch_bounds__(THREADS) void inpaint_apply_kernel(const int* __restrict__ donor,
                                                                const int* __restrict__ src,
                                                                const float* __restrict__ pos,
                                                                const float* __restrict__ inv_in,
                                                                const float* __restrict__ values, int C, float fill,
                                                                int H, int W, int* __restrict__ src_out,
                                                                float* __restrict__ inv_pos, float* __restrict__ out) {
  const int N = H * W;
  const unsigned i = blockIdx.x * THREADS + threadIdx.x;
  if (i >= (unsigned)N) return;
  const int c = (int)i;
  const Filled f = apply(c, donor[c], src, pos, inv_in, H, W);
  src_out[c] = f.src;
  inv_pos[c] = f.ix;
  inv_pos[(size_t)N + c] = f.iy;
  for (int ch = 0; ch < C; ++ch) out[(size_t)ch * N + c] = f.src >= 0 ? values[(size_t)ch * N + f.win] : fill;
}

// RS_INPAINT_STAGE=0: the row pass reads col in place whatever the shape
bool stage_allowed() {
  static const bool on = [] {
    const char* e = getenv("RS_INPAINT_STAGE");
    return !(e && e[0] == '0');
  }();
  return on;
}

}  // namespace inpaint

// the widest span of col a block of the row pass reads
int splat_inpaint_span(int R, int W) {
  const int64_t span = (int64_t)inpaint::SEG + 2 * (int64_t)R;
  return (int)(span < W ? span : W);
}

bool splat_inpaint_staged(int R, int W) {
  return inpaint::stage_allowed() && splat_inpaint_span(R, W) <= inpaint::STAGE;
}

// col: H*W int32; values and out: nullptr iff C == 0; 2 <= H, W <= 32767, 0 <= R <= 32767
void splat_inpaint_launch(const int* src_index, const float* pos, const float* inv_in, const float* values, int C,
                          int R, float fill, int H, int W, int* col, int* donor, int* dist2, int* src_out,
                          float* inv_pos, float* out, hipStream_t s) {
  const int N = H * W;
  const dim3 flat((unsigned)((N - 1) / inpaint::THREADS + 1)), block(inpaint::THREADS);
  const dim3 rows((unsigned)((W - 1) / inpaint::SEG + 1), (unsigned)H);  // H <= 32767 < 65536
  hipLaunchKernelGGL(inpaint::inpaint_column_kernel, flat, block, 0, s, src_index, R, H, W, col);
  if (splat_inpaint_staged(R, W))
    hipLaunchKernelGGL(inpaint::inpaint_row_kernel<true>, rows, block, 0, s, col, R, H, W, donor, dist2);
  else
    hipLaunchKernelGGL(inpaint::inpaint_row_kernel<false>, rows, block, 0, s, col, R, H, W, donor, dist2);
  hipLaunchKernelGGL(inpaint::inpaint_apply_kernel, flat, block, 0, s, donor, src_index, pos, inv_in, values, C, fill,
                     H, W, src_out, inv_pos, out);
}

}  // namespace rs

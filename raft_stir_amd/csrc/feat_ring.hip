// Feature ring of the trackers that encode every frame once
// (export/multiflow.py, export/pointtrack.py with cache_features): one launch
// stores the new frame's features in the ring and assembles the refinement
// batch of a bidirectional pass over K (stored frame, new frame) pairs.
//
//   ring_f [R][P][C], ring_c [R][P][Cc]   feature / context rows (P = h*w, NHWC)
//   f_new [P][C], c_new [P][Cc]           the new frame's features
//   idx [K+1] int32 on the device         src[0..K), then dst
//   x [3K][P][C], ctx [2K][P][Cc]         outputs
//
// "put, then gather":
//   ring_f[dst] = f_new, ring_c[dst] = c_new
//   x[k] = ring_f[src[k]],  x[K+k] = f_new,  x[2K+k] = x[k]
//   ctx[k] = ring_c[src[k]],  ctx[K+k] = c_new
// so x[0:2K] and x[K:3K] are fmap1 and fmap2 of the pass without a cat.
//
// Every index is clamped to [0, R-1]: the table lives in device memory and the
// host cannot check it.  A slot whose source is the row being written reads
// f_new / c_new itself, so no thread reads a row that this launch writes and
// the result does not depend on the order of the blocks.
//
// blockIdx.y is the destination image: 3K of x, 2K of ctx, the two ring rows.
// The block reads its one or two indices through addresses that are the same
// in every lane, then its threads copy 16-byte vectors along the channel axis
// in a grid-stride loop over blockIdx.x.
#include "common.h"

namespace rs {
namespace ring {

constexpr int THREADS = 256;
constexpr int PER_THREAD = 4;  // vectors per thread before the grid stride repeats

__device__ __forceinline__ int clamp_row(int i, int R) { return min(max(i, 0), R - 1); }

// T: the element type; V: 16 bytes of it.  nf, nc: vectors per feature / context image.
template <typename T, typename V>
__global__ __launch_bounds__(THREADS) void feature_ring_kernel(V* __restrict__ ring_f, V* __restrict__ ring_c,
                                                               const V* __restrict__ f_new,
                                                               const V* __restrict__ c_new,
                                                               const int* __restrict__ idx, V* __restrict__ x,
                                                               V* __restrict__ ctx, int K, int R, int nf, int nc) {
  static_assert(sizeof(V) == 16 && sizeof(V) % sizeof(T) == 0, "16-byte vectors of whole elements");
  const int j = blockIdx.y;  // [0,3K): x; [3K,5K): ctx; 5K: ring_f[dst]; 5K+1: ring_c[dst]
  const int dst = clamp_row(idx[K], R);
  const V* from;
  V* to;
  int n;
  if (j < 3 * K) {
    n = nf;
    to = x + (size_t)j * nf;
    const int k = j < K ? j : j - 2 * K;  // [K,2K): the new frame
    from = f_new;
    if (k >= 0 && k < K) {
      const int src = clamp_row(idx[k], R);
      if (src != dst) from = ring_f + (size_t)src * nf;
    }
  } else if (j < 5 * K) {
    n = nc;
    to = ctx + (size_t)(j - 3 * K) * nc;
    const int k = j - 3 * K;
    from = c_new;
    if (k < K) {
      const int src = clamp_row(idx[k], R);
      if (src != dst) from = ring_c + (size_t)src * nc;
    }
  } else if (j == 5 * K) {
    n = nf;
    to = ring_f + (size_t)dst * nf;
    from = f_new;
  } else {
    n = nc;
    to = ring_c + (size_t)dst * nc;
    from = c_new;
  }
  for (int i = blockIdx.x * THREADS + threadIdx.x; i < n; i += gridDim.x * THREADS) to[i] = from[i];
}

template <typename T, typename V>
static void launch(void* ring_f, void* ring_c, const void* f_new, const void* c_new, const int* idx, void* x,
                   void* ctx, int K, int R, int nf, int nc, hipStream_t s) {
  const int nmax = nf > nc ? nf : nc;
  const dim3 grid(cdiv(nmax, THREADS * PER_THREAD), 5 * K + 2);
  hipLaunchKernelGGL((feature_ring_kernel<T, V>), grid, dim3(THREADS), 0, s, (V*)ring_f, (V*)ring_c, (const V*)f_new,
                     (const V*)c_new, idx, (V*)x, (V*)ctx, K, R, nf, nc);
}

}  // namespace ring

// nf, nc: 16-byte vectors per image (h*w*C*elemsize/16, checked on the host to fit an int).
void feature_ring_launch(bool bf16, void* ring_f, void* ring_c, const void* f_new, const void* c_new, const int* idx,
                         void* x, void* ctx, int K, int R, int nf, int nc, hipStream_t s) {
  if (bf16)
    ring::launch<bf16_t, bf16x8_t>(ring_f, ring_c, f_new, c_new, idx, x, ctx, K, R, nf, nc, s);
  else
    ring::launch<float, f32x4_t>(ring_f, ring_c, f_new, c_new, idx, x, ctx, K, R, nf, nc, s);
}

}  // namespace rs

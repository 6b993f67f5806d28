// Forward interpolation of a flow field for RAFT's video warm start
// (reference core/utils/utils.py:26-54, scipy griddata 'nearest'): every sample
// of the 1/8-resolution flow is moved to where it points, and every grid cell
// takes the flow of the nearest moved sample.
//
// Exact rule, per image of a (B,2,H,W) fp32 flow, N = H*W:
//   sample s at cell (x, y):  x1 = float(x) + dx[s],  y1 = float(y) + dy[s]   (fp32 sums)
//   valid(s) = x1 > 0 && x1 < W && y1 > 0 && y1 < H    (strict; NaN / Inf fail the comparisons)
//   d2(q, s) = fl(fl(ex*ex) + fl(ey*ey)),  ex = qx - x1,  ey = qy - y1       (fp32, no FMA)
//   out[q]   = flow[s*],  s* = the valid sample of smallest d2, lowest row-major index among equals;
//              all zeros when the image has no valid sample.
// The rule does not depend on the launch order, so the op is deterministic and
// can be checked bit for bit against ops/reference.py: forward_interpolate.
//
// Brute force over all N x N pairs (N is 5-7 thousand at 1/8 resolution):
//   fi_search_kernel  a block of 256 queries walks one chunk of the samples, staged 256 at a
//                     time in LDS as float2 positions (+inf for invalid ones; every lane reads
//                     the same address, a broadcast).  The sample range is split over
//                     gridDim.y chunks so that a small field still fills the chip.  Each
//                     (chunk, query) writes a packed key (bits(d2) << 32) | index: d2 >= 0, so
//                     its bit pattern orders like the float and an unsigned 64-bit minimum is
//                     "smallest d2, then lowest index".
//   fi_gather_kernel  takes the minimum key over the chunks and copies flow[index], or writes 0
//                     where no chunk held a valid sample.
#include "common.h"

namespace rs {
namespace fi {

constexpr int THREADS = 256;
constexpr int TILE = THREADS;  // samples staged per step: one per thread
constexpr unsigned NONE = 0xffffffffu;

// keys: [B][gridDim.y][N]
__global__ __launch_bounds__(THREADS) void fi_search_kernel(const float* __restrict__ flow, int H, int W,
                                                             int chunk, unsigned long long* __restrict__ keys) {
  __shared__ float2 pos[TILE];
  const int N = H * W;
  const int b = blockIdx.z, c = blockIdx.y;
  const float* fx = flow + (size_t)b * 2 * N;
  const float* fy = fx + N;
  const int q = blockIdx.x * THREADS + threadIdx.x;  // q >= N: takes part in the staging only
  const int qy = q / W;
  const float qxf = (float)(q - qy * W), qyf = (float)qy;
  const float wf = (float)W, hf = (float)H;
  const int s0 = c * chunk, s1 = min(N, s0 + chunk);
  float best = INFINITY;
  unsigned bi = NONE;
  for (int t = s0; t < s1; t += TILE) {
    const int s = t + threadIdx.x;
    float2 p = make_float2(INFINITY, INFINITY);
    if (s < s1) {
      const int sy = s / W;
      const float x1 = (float)(s - sy * W) + fx[s];
      const float y1 = (float)sy + fy[s];
      if (x1 > 0.f && x1 < wf && y1 > 0.f && y1 < hf) p = make_float2(x1, y1);
    }
    __syncthreads();  // the previous tile has been read
    pos[threadIdx.x] = p;
    __syncthreads();
#pragma unroll 8
    for (int j = 0; j < TILE; ++j) {
      const float2 sp = pos[j];
      const float ex = qxf - sp.x, ey = qyf - sp.y;
      const float d2 = __fadd_rn(__fmul_rn(ex, ex), __fmul_rn(ey, ey));  // never contracted to an FMA
      if (d2 < best) {  // strict: the walk is in index order, so the lowest index keeps a tie
        best = d2;
        bi = (unsigned)(t + j);
      }
    }
  }
  if (q < N)
    keys[((size_t)b * gridDim.y + c) * N + q] = ((unsigned long long)__float_as_uint(best) << 32) | bi;
}

__global__ __launch_bounds__(THREADS) void fi_gather_kernel(const float* __restrict__ flow,
                                                             const unsigned long long* __restrict__ keys,
                                                             int N, int chunks, float* __restrict__ out) {
  const int q = blockIdx.x * THREADS + threadIdx.x;
  const int b = blockIdx.y;
  if (q >= N) return;
  const unsigned long long* k = keys + (size_t)b * chunks * N + q;
  unsigned long long m = k[0];
  for (int c = 1; c < chunks; ++c) {
    const unsigned long long v = k[(size_t)c * N];
    m = v < m ? v : m;
  }
  const unsigned idx = (unsigned)m;
  const float* fx = flow + (size_t)b * 2 * N;
  float* ox = out + (size_t)b * 2 * N;
  const bool hit = idx != NONE;
  ox[q] = hit ? fx[idx] : 0.f;
  ox[q + N] = hit ? fx[idx + N] : 0.f;
}

}  // namespace fi

// Samples per chunk, a multiple of the tile: about 1024 blocks in all, so that the
// 1/8 field of a small image (28 query blocks at 64x80) still covers the 256 CUs.
int forward_interp_chunk(int B, int N) {
  const int qblocks = cdiv(N, fi::THREADS);
  const long want = 1024 / ((long)qblocks * B);
  const int chunks = (int)(want < 1 ? 1 : (want > qblocks ? qblocks : want));
  return round_up(cdiv(N, chunks), fi::TILE);
}

// keys: B * cdiv(N, chunk) * N entries
void forward_interp_launch(const float* flow, int B, int H, int W, int chunk, unsigned long long* keys,
                           float* out, hipStream_t s) {
  const int N = H * W;
  const int chunks = cdiv(N, chunk);
  const int qblocks = cdiv(N, fi::THREADS);
  hipLaunchKernelGGL(fi::fi_search_kernel, dim3(qblocks, chunks, B), dim3(fi::THREADS), 0, s, flow, H, W,
                     chunk, keys);
  hipLaunchKernelGGL(fi::fi_gather_kernel, dim3(qblocks, B), dim3(fi::THREADS), 0, s, flow, keys, N, chunks,
                     out);
}

}  // namespace rs

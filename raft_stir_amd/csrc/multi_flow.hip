// Multi-delta point tracking (MFT, Neoral et al., WACV 2024): K flow pairs that
// all end in the current frame t, slot k spanning t-D_k -> t, each with the
// tracked positions of its own start frame.  Every point takes the candidate
// of the most reliable slot.
//
// Per slot k and point n the candidate (c, e, ok) is fb::track_point on
// (flow_fw[k], flow_bw[k], starts[k][n]): exactly what fb_points_kernel of
// csrc/fb_check.hip computes, from the same inlined device functions
// (csrc/fb_device.h).  Then
//   s_k      = start_score[k][n] + e_k                                   (one fp32 add)
//   eligible = active[k] && start_visible[k][n] && ok_k && s_k < +inf    (NaN fails)
//   some slot eligible:  choice = the eligible slot of smallest s, the lowest k among equals; visible = 1
//   none, some active:   choice = the lowest active k; visible = 0
//   none active:         choice = -1, point = starts[0][n], score = start_score[0][n], err = +inf, visible = 0
//   otherwise point = c_choice, score = s_choice, err = e_choice.
// cand_err[k][n] = e_k for every slot, active or not.
//
// One thread per (point, slot): lane = point * KP + k with KP = K rounded up to
// a power of two (at most 16), so the slots of a point are KP neighbouring
// lanes of one wave and all 16 K gathers of a point are in flight together.
// The arg-min over the slots is a log2(KP)-step xor butterfly inside those
// lanes; padded lanes (k >= K or n >= N) take part as inactive slots and read
// and write nothing.  The lane of the chosen slot writes the point's outputs.
// No atomics: the result does not depend on the launch order.  `active` is
// read on the device, so a captured graph replays with it changed.
#include "common.h"
#include "fb_device.h"

namespace rs {
namespace mf {

constexpr int THREADS = 256;
constexpr int NONE = 64;  // above every slot index

// flows: [K][2][H][W]; starts: [K][N][2]; start_score, start_visible, cand_err: [K][N]; active: [K];
// points: [N][2]; score, visible, choice, err: [N].  kp_log2: log2(KP).
__global__ __launch_bounds__(THREADS) void multi_flow_kernel(
    const float* __restrict__ fw, const float* __restrict__ bw, const float* __restrict__ starts,
    const float* __restrict__ start_score, const bool* __restrict__ start_visible, const bool* __restrict__ active,
    int K, int kp_log2, int H, int W, int N, float a1, float a2, float* __restrict__ points,
    float* __restrict__ score, bool* __restrict__ visible, int* __restrict__ choice, float* __restrict__ err,
    float* __restrict__ cand_err) {
  const int KP = 1 << kp_log2;
  const int tid = blockIdx.x * THREADS + threadIdx.x;  // N * KP < 2^31: checked on the host
  const int k = tid & (KP - 1);
  const int n = tid >> kp_log2;
  const bool live = k < K && n < N;

  float px = 0.f, py = 0.f, cx = 0.f, cy = 0.f, e = INFINITY, s0 = 0.f, s = INFINITY;
  bool act = false, elig = false;
  if (live) {
    const size_t plane = (size_t)H * W;
    const size_t i = (size_t)k * N + n;
    px = starts[2 * i];
    py = starts[2 * i + 1];
    bool ok;
    fb::track_point(fw + (size_t)k * 2 * plane, bw + (size_t)k * 2 * plane, plane, H, W, px, py, a1, a2, cx, cy, e,
                    ok);
    cand_err[i] = e;
    s0 = start_score[i];
    s = __fadd_rn(s0, e);
    act = active[k];
    elig = act && start_visible[i] && ok && s < INFINITY;
  }

  // arg-min of (s, k) over the eligible slots and the lowest active slot, in the point's KP lanes
  float best_s = s;
  int best_k = elig ? k : NONE;
  int first_k = act ? k : NONE;
  for (int off = 1; off < KP; off <<= 1) {
    const float o_s = __shfl_xor(best_s, off);
    const int o_k = __shfl_xor(best_k, off);
    const int o_first = __shfl_xor(first_k, off);
    if (o_k != NONE && (best_k == NONE || o_s < best_s || (o_s == best_s && o_k < best_k))) {
      best_s = o_s;
      best_k = o_k;
    }
    first_k = min(first_k, o_first);
  }

  if (!live) return;
  const int chosen = best_k != NONE ? best_k : (first_k != NONE ? first_k : -1);
  if (chosen >= 0) {
    if (k != chosen) return;
    points[2 * (size_t)n] = cx;
    points[2 * (size_t)n + 1] = cy;
    score[n] = s;
    err[n] = e;
  } else {
    if (k != 0) return;
    points[2 * (size_t)n] = px;
    points[2 * (size_t)n + 1] = py;
    score[n] = s0;
    err[n] = INFINITY;
  }
  visible[n] = best_k != NONE;
  choice[n] = chosen;
}

}  // namespace mf

void multi_flow_launch(const float* fw, const float* bw, const float* starts, const float* start_score,
                       const bool* start_visible, const bool* active, int K, int H, int W, int N, float a1, float a2,
                       float* points, float* score, bool* visible, int* choice, float* err, float* cand_err,
                       hipStream_t s) {
  int kp_log2 = 0;
  while ((1 << kp_log2) < K) ++kp_log2;
  hipLaunchKernelGGL(mf::multi_flow_kernel, dim3(cdiv(N << kp_log2, mf::THREADS)), dim3(mf::THREADS), 0, s, fw, bw,
                     starts, start_score, start_visible, active, K, kp_log2, H, W, N, a1, a2, points, score, visible,
                     choice, err, cand_err);
}

}  // namespace rs

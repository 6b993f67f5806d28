// Dense multi-delta tracking: the selection rule of csrc/multi_flow.hip at
// every pixel of the anchor frame, on a planar state ring that stays on the
// device (export/denseflow.py: DenseMultiFlowTracker).
//
//   ring_pos   [R][2][H][W]  for every anchor pixel (y,x), its position (x', y') in the stored frame
//   ring_score [R][H][W]     the stored score; +inf: the pixel was not visible in that frame
//   idx [K+1] int32, active [K] bool, both on the device: src[0..K), then dst
//   fw, bw     [K][2][H][W]  slot k spans (the frame of row src[k]) -> t and back
//
// The rows are those of the feature ring (csrc/feat_ring.hip): R = L + 2,
// frame t in row t % (L+1), row L+1 the anchor, chosen by the same index table.
//
// Per pixel n and slot k the candidate (c, e, ok) is fb::track_point on
// (fw[k], bw[k], ring_pos[src_k][:, n]), from the device functions of
// csrc/fb_device.h that csrc/multi_flow.hip and csrc/fb_check.hip inline too.
// Then, as written at the top of csrc/multi_flow.hip,
//   s_k      = ring_score[src_k][n] + e_k                                  (one fp32 add)
//   eligible = active_k && start_visible && ok_k && s_k < +inf             (NaN fails)
//   some slot eligible:  choice = the eligible slot of smallest s, the lowest k among equals; visible = 1
//   none, some active:   choice = the lowest active k; visible = 0
//   none active:         choice = -1, pos = ring_pos[src_0][:, n], err = +inf, visible = 0
// with start_visible := ring_score[src_k][n] < +inf.  There is no ring of
// visibility flags: the tracker stores +inf as the score of every pixel that
// is not visible and an eligible slot needs s < +inf, so a stored score is
// finite iff the pixel was visible.  For the same reason the score written is
// s_choice where visible and +inf elsewhere (the none-active case included),
// and no torch.where follows the launch.
//
// Outputs: pos [2][H][W], score, err [H][W], visible [H][W] bool, choice
// [H][W] int32, and pos / score again into ring row dst.  cand_err [K][H][W]
// (e_k of every slot, active or not) only in the CAND instantiation, so the
// default step does not pay K planes of stores.
//
// Thread mapping: one thread per pixel, looping over the K slots.  The other
// candidate, multi_flow.hip's lane per (point, slot) with a butterfly, suits a
// short list of array-of-structs points; here the state is planar, so the
// three state reads of a slot and all stores are coalesced over the 64 pixels
// of a wave, and the 2x2 gathers of neighbouring pixels fall into the same
// cache lines because a tracked position field is the pixel grid plus a smooth
// flow.  With (point, slot) lanes a wave would cover 64/KP pixels and read KP
// rows at a stride of a whole plane, and the outputs would be written by one
// lane in KP.  The arg-min is a strict "<" in growing k: the lowest k among
// equals without any cross-lane traffic.  A 512x640 plane is 5120 waves, so
// the serial chain of K gathers per thread is hidden by the other waves.
//
// Safety (the launch is replayed from a captured graph with idx and active
// changed on the device, where the host cannot check them):
//   * every index is clamped to [0, R-1];
//   * a slot that is not active reads nothing (with CAND every slot is read,
//     for its cand_err; with no active slot, slot 0's state is read);
//   * a slot whose clamped source row is the row being written counts as
//     inactive.  It could not go wrong either way: a thread reads and writes
//     the state of its own pixel only, all reads before its writes, so no
//     thread reads what another writes whatever idx holds;
//   * a non-finite or out-of-image start goes through track_point's guards;
//   * no atomics and no dependence on the launch order.
#include "common.h"
#include "fb_device.h"

namespace rs {
namespace dense {

constexpr int THREADS = 256;

__device__ __forceinline__ int clamp_row(int i, int R) { return min(max(i, 0), R - 1); }

template <bool CAND>
__global__ __launch_bounds__(THREADS) void dense_multi_flow_kernel(
    const float* __restrict__ fw, const float* __restrict__ bw, float* ring_pos, float* ring_score,
    const int* __restrict__ idx, const bool* __restrict__ active, int K, int R, int H, int W, float a1, float a2,
    float* pos, float* score, bool* visible, int* choice, float* err, float* cand_err) {
  const int plane = H * W;  // K * H * W < 2^31: checked on the host
  const int n = blockIdx.x * THREADS + threadIdx.x;
  if (n >= plane) return;
  const size_t P = (size_t)plane;
  const int dst = clamp_row(idx[K], R);

  int best_k = -1, first_k = -1;
  float best_x = 0.f, best_y = 0.f, best_s = INFINITY, best_e = INFINITY;
  float first_x = 0.f, first_y = 0.f, first_e = INFINITY;
  for (int k = 0; k < K; ++k) {
    const int src = clamp_row(idx[k], R);  // the same in every lane
    const bool act = active[k] && src != dst;
    if (!CAND && !act) continue;
    const float px = ring_pos[(size_t)src * 2 * P + n];
    const float py = ring_pos[(size_t)src * 2 * P + P + n];
    const float s0 = ring_score[(size_t)src * P + n];
    float cx, cy, e;
    bool ok;
    fb::track_point(fw + (size_t)k * 2 * P, bw + (size_t)k * 2 * P, P, H, W, px, py, a1, a2, cx, cy, e, ok);
    if (CAND) cand_err[(size_t)k * P + n] = e;
    if (!act) continue;
    const float s = __fadd_rn(s0, e);
    if (first_k < 0) {
      first_k = k;
      first_x = cx;
      first_y = cy;
      first_e = e;
    }
    const bool elig = s0 < INFINITY && ok && s < INFINITY;
    if (elig && (best_k < 0 || s < best_s)) {
      best_k = k;
      best_x = cx;
      best_y = cy;
      best_s = s;
      best_e = e;
    }
  }

  float ox, oy, oe;
  int oc;
  if (best_k >= 0) {
    ox = best_x, oy = best_y, oe = best_e, oc = best_k;
  } else if (first_k >= 0) {
    ox = first_x, oy = first_y, oe = first_e, oc = first_k;
  } else {
    const int src = clamp_row(idx[0], R);
    ox = ring_pos[(size_t)src * 2 * P + n];
    oy = ring_pos[(size_t)src * 2 * P + P + n];
    oe = INFINITY;
    oc = -1;
  }
  const float os = best_k >= 0 ? best_s : INFINITY;  // a lost pixel: nothing chains from it with a finite score
  pos[n] = ox;
  pos[P + n] = oy;
  score[n] = os;
  visible[n] = best_k >= 0;
  choice[n] = oc;
  err[n] = oe;
  ring_pos[(size_t)dst * 2 * P + n] = ox;
  ring_pos[(size_t)dst * 2 * P + P + n] = oy;
  ring_score[(size_t)dst * P + n] = os;
}

}  // namespace dense

// cand_err: nullptr unless asked for
void dense_multi_flow_launch(const float* fw, const float* bw, float* ring_pos, float* ring_score, const int* idx,
                             const bool* active, int K, int R, int H, int W, float a1, float a2, float* pos,
                             float* score, bool* visible, int* choice, float* err, float* cand_err, hipStream_t s) {
  const dim3 grid(cdiv(H * W, dense::THREADS)), block(dense::THREADS);
  if (cand_err)
    hipLaunchKernelGGL(dense::dense_multi_flow_kernel<true>, grid, block, 0, s, fw, bw, ring_pos, ring_score, idx,
                       active, K, R, H, W, a1, a2, pos, score, visible, choice, err, cand_err);
  else
    hipLaunchKernelGGL(dense::dense_multi_flow_kernel<false>, grid, block, 0, s, fw, bw, ring_pos, ring_score, idx,
                       active, K, R, H, W, a1, a2, pos, score, visible, choice, err, cand_err);
}

}  // namespace rs

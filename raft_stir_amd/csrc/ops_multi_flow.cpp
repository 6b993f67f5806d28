// torch.ops.raft_stir.multi_flow_track_points (csrc/multi_flow.hip).
#include <ATen/ATen.h>
#include "host_common.h"
#include <c10/core/DeviceGuard.h>
#include <torch/library.h>

#include <hip/hip_runtime.h>

#include <cmath>
#include <tuple>

namespace rs {
void multi_flow_launch(const float* fw, const float* bw, const float* starts, const float* start_score,
                       const bool* start_visible, const bool* active, int K, int H, int W, int N, float a1, float a2,
                       float* points, float* score, bool* visible, int* choice, float* err, float* cand_err,
                       hipStream_t s);
}  // namespace rs

namespace {
using at::Tensor;

constexpr int64_t kMaxSlots = 16;                 // the slots of a point share one wave
constexpr int64_t kMaxCells = int64_t(1) << 30;   // exclusive: pixel indices stay ints
constexpr int64_t kMaxPoints = int64_t(1) << 26;  // 16 lanes per point, thread indices stay ints

const char* const kOp = "multi_flow_track_points";

// No host synchronisation: `active` is read on the device, the outputs come
// from the caching allocator and the kernel goes to the current stream, so the
// op can be captured in a hipGraph and replayed with every input changed.
std::tuple<Tensor, Tensor, Tensor, Tensor, Tensor, Tensor> multi_flow_track_points(
    const Tensor& fw, const Tensor& bw, const Tensor& starts, const Tensor& start_score, const Tensor& start_visible,
    const Tensor& active, double alpha1, double alpha2) {
  TORCH_CHECK(fw.is_cuda(), kOp, ": GPU tensors expected");
  for (const Tensor* t : {&bw, &starts, &start_score, &start_visible, &active})
    TORCH_CHECK(t->device() == fw.device(), kOp, ": all tensors must be on the same device, got ", fw.device(),
                " and ", t->device());
  TORCH_CHECK(fw.scalar_type() == at::kFloat && bw.scalar_type() == at::kFloat, kOp, ": fp32 flows expected");
  TORCH_CHECK(fw.dim() == 4 && fw.size(1) == 2, kOp, ": flow_fw must be (K,2,H,W)");
  TORCH_CHECK(bw.sizes() == fw.sizes(), kOp, ": flow_fw and flow_bw must have the same shape, got ", fw.sizes(),
              " and ", bw.sizes());
  TORCH_CHECK(fw.is_contiguous() && bw.is_contiguous(), kOp, ": contiguous flows expected");
  const int64_t K = fw.size(0), H = fw.size(2), W = fw.size(3);
  TORCH_CHECK(K >= 1, kOp, ": no slots");
  TORCH_CHECK(K <= kMaxSlots, kOp, ": at most ", kMaxSlots, " slots, got K = ", K);
  TORCH_CHECK(H >= 2 && W >= 2, kOp, ": H, W >= 2 expected, got H = ", H, ", W = ", W);
  TORCH_CHECK(H * W < kMaxCells, kOp, ": H*W = ", H * W, " must be below 2^30");
  // NaN fails the comparisons, +inf the finiteness test
  TORCH_CHECK(alpha1 >= 0.0 && alpha2 >= 0.0 && std::isfinite(alpha1) && std::isfinite(alpha2), kOp,
              ": alpha1 and alpha2 must be finite and >= 0, got ", alpha1, " and ", alpha2);
  TORCH_CHECK(starts.scalar_type() == at::kFloat, kOp, ": fp32 starts expected");
  TORCH_CHECK(starts.dim() == 3 && starts.size(0) == K && starts.size(1) >= 1 && starts.size(2) == 2, kOp,
              ": starts must be (K,N,2) with K = ", K, " and N >= 1, got ", starts.sizes());
  TORCH_CHECK(starts.is_contiguous(), kOp, ": contiguous starts expected");
  const int64_t N = starts.size(1);
  TORCH_CHECK(N <= kMaxPoints, kOp, ": at most ", kMaxPoints, " points");
  TORCH_CHECK(start_score.scalar_type() == at::kFloat, kOp, ": fp32 start_score expected");
  TORCH_CHECK(start_score.dim() == 2 && start_score.size(0) == K && start_score.size(1) == N &&
                  start_score.is_contiguous(),
              kOp, ": start_score must be a contiguous (K,N) = (", K, ",", N, "), got ", start_score.sizes());
  TORCH_CHECK(start_visible.scalar_type() == at::kBool, kOp, ": bool start_visible expected");
  TORCH_CHECK(start_visible.dim() == 2 && start_visible.size(0) == K && start_visible.size(1) == N &&
                  start_visible.is_contiguous(),
              kOp, ": start_visible must be a contiguous (K,N) = (", K, ",", N, "), got ", start_visible.sizes());
  TORCH_CHECK(active.scalar_type() == at::kBool, kOp, ": bool active expected");
  TORCH_CHECK(active.dim() == 1 && active.size(0) == K && active.is_contiguous(), kOp,
              ": active must be a contiguous (K,) = (", K, ",), got ", active.sizes());
  const c10::DeviceGuard guard(fw.device());
  Tensor points = at::empty({1, N, 2}, fw.options());
  Tensor score = at::empty({1, N}, fw.options());
  Tensor visible = at::empty({1, N}, fw.options().dtype(at::kBool));
  Tensor choice = at::empty({1, N}, fw.options().dtype(at::kInt));
  Tensor err = at::empty({1, N}, fw.options());
  Tensor cand_err = at::empty({K, N}, fw.options());
  rs::multi_flow_launch(fw.data_ptr<float>(), bw.data_ptr<float>(), starts.data_ptr<float>(),
                        start_score.data_ptr<float>(), start_visible.data_ptr<bool>(), active.data_ptr<bool>(), (int)K,
                        (int)H, (int)W, (int)N, (float)alpha1, (float)alpha2, points.data_ptr<float>(),
                        score.data_ptr<float>(), visible.data_ptr<bool>(), choice.data_ptr<int>(),
                        err.data_ptr<float>(), cand_err.data_ptr<float>(), rs::current_stream());
  RS_CHECK_LAUNCH();
  return {points, score, visible, choice, err, cand_err};
}
}  // namespace

TORCH_LIBRARY_FRAGMENT(raft_stir, m) {
  m.def(
      "multi_flow_track_points(Tensor flow_fw, Tensor flow_bw, Tensor starts, Tensor start_score, "
      "Tensor start_visible, Tensor active, float alpha1, float alpha2) -> "
      "(Tensor points, Tensor score, Tensor visible, Tensor choice, Tensor err, Tensor cand_err)");
}

TORCH_LIBRARY_IMPL(raft_stir, CUDA, m) { m.impl("multi_flow_track_points", &multi_flow_track_points); }

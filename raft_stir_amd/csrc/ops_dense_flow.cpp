// torch.ops.raft_stir.dense_multi_flow_step (csrc/dense_flow.hip).
#include <ATen/ATen.h>
#include "host_common.h"
#include <c10/core/DeviceGuard.h>
#include <torch/library.h>

#include <hip/hip_runtime.h>

#include <cmath>
#include <optional>

namespace rs {
void dense_multi_flow_launch(const float* fw, const float* bw, float* ring_pos, float* ring_score, const int* idx,
                             const bool* active, int K, int R, int H, int W, float a1, float a2, float* pos,
                             float* score, bool* visible, int* choice, float* err, float* cand_err, hipStream_t s);
}  // namespace rs

namespace {
using at::Tensor;

constexpr int64_t kMaxSlots = 16;                 // as multi_flow_track_points
constexpr int64_t kMaxCells = int64_t(1) << 31;   // exclusive: K*H*W, the largest index of cand_err, stays an int

const char* const kOp = "dense_multi_flow_step";

void check_out(const Tensor& t, const char* what, at::ScalarType dt, at::IntArrayRef shape) {
  TORCH_CHECK(t.scalar_type() == dt && t.sizes() == shape && t.is_contiguous(), kOp, ": ", what,
              " must be a contiguous ", dt, " tensor of shape ", shape, ", got ", t.scalar_type(), " ", t.sizes());
}

// No host synchronisation: `idx` and `active` are read on the device, nothing
// is allocated and the kernel goes to the current stream, so the op can be
// captured in a hipGraph and replayed with another index row, another set of
// active slots, other flows and another ring content.
void dense_multi_flow_step(const Tensor& fw, const Tensor& bw, const Tensor& ring_pos, const Tensor& ring_score,
                           const Tensor& idx, const Tensor& active, double alpha1, double alpha2, const Tensor& pos,
                           const Tensor& score, const Tensor& visible, const Tensor& choice, const Tensor& fb_err,
                           const std::optional<Tensor>& cand_err) {
  TORCH_CHECK(fw.is_cuda(), kOp, ": GPU tensors expected");
  for (const Tensor* t : {&bw, &ring_pos, &ring_score, &idx, &active, &pos, &score, &visible, &choice, &fb_err})
    TORCH_CHECK(t->device() == fw.device(), kOp, ": all tensors must be on the same device, got ", fw.device(),
                " and ", t->device());
  TORCH_CHECK(fw.scalar_type() == at::kFloat && bw.scalar_type() == at::kFloat, kOp, ": fp32 flows expected");
  TORCH_CHECK(fw.dim() == 4 && fw.size(1) == 2, kOp, ": flow_fw must be (K,2,H,W)");
  TORCH_CHECK(bw.sizes() == fw.sizes(), kOp, ": flow_fw and flow_bw must have the same shape, got ", fw.sizes(),
              " and ", bw.sizes());
  const int64_t K = fw.size(0), H = fw.size(2), W = fw.size(3);
  TORCH_CHECK(K >= 1, kOp, ": no slots");
  TORCH_CHECK(K <= kMaxSlots, kOp, ": at most ", kMaxSlots, " slots, got K = ", K);
  TORCH_CHECK(H >= 2 && W >= 2, kOp, ": H, W >= 2 expected, got H = ", H, ", W = ", W);
  TORCH_CHECK(K * H * W < kMaxCells, kOp, ": K*H*W = ", K * H * W, " must be below 2^31");
  TORCH_CHECK(fw.is_contiguous() && bw.is_contiguous(), kOp, ": contiguous flows expected");
  // NaN fails the comparisons, +inf the finiteness test
  TORCH_CHECK(alpha1 >= 0.0 && alpha2 >= 0.0 && std::isfinite(alpha1) && std::isfinite(alpha2), kOp,
              ": alpha1 and alpha2 must be finite and >= 0, got ", alpha1, " and ", alpha2);
  TORCH_CHECK(ring_pos.scalar_type() == at::kFloat && ring_score.scalar_type() == at::kFloat, kOp,
              ": fp32 rings expected");
  TORCH_CHECK(ring_pos.dim() == 4 && ring_pos.size(1) == 2 && ring_pos.size(2) == H && ring_pos.size(3) == W, kOp,
              ": ring_pos must be (R,2,H,W) = (R,2,", H, ",", W, "), got ", ring_pos.sizes());
  const int64_t R = ring_pos.size(0);
  TORCH_CHECK(R >= 2, kOp, ": a ring of R >= 2 rows expected, got R = ", R);
  TORCH_CHECK(ring_score.dim() == 3 && ring_score.size(0) == R && ring_score.size(1) == H && ring_score.size(2) == W,
              kOp, ": ring_score must be (R,H,W) = (", R, ",", H, ",", W, "), got ", ring_score.sizes());
  TORCH_CHECK(ring_pos.is_contiguous() && ring_score.is_contiguous(), kOp, ": contiguous rings expected");
  TORCH_CHECK(idx.scalar_type() == at::kInt, kOp, ": int32 idx expected, got ", idx.scalar_type());
  TORCH_CHECK(idx.dim() == 1 && idx.size(0) == K + 1 && idx.is_contiguous(), kOp,
              ": idx must be a contiguous (K+1,) = (", K + 1, ",), got ", idx.sizes());
  TORCH_CHECK(active.scalar_type() == at::kBool, kOp, ": bool active expected");
  TORCH_CHECK(active.dim() == 1 && active.size(0) == K && active.is_contiguous(), kOp,
              ": active must be a contiguous (K,) = (", K, ",), got ", active.sizes());
  check_out(pos, "pos", at::kFloat, {1, 2, H, W});
  check_out(score, "score", at::kFloat, {1, 1, H, W});
  check_out(visible, "visible", at::kBool, {1, 1, H, W});
  check_out(choice, "choice", at::kInt, {1, 1, H, W});
  check_out(fb_err, "fb_err", at::kFloat, {1, 1, H, W});
  float* cand = nullptr;
  if (cand_err.has_value() && cand_err->defined()) {
    TORCH_CHECK(cand_err->device() == fw.device(), kOp, ": all tensors must be on the same device, got ",
                fw.device(), " and ", cand_err->device());
    check_out(*cand_err, "cand_err", at::kFloat, {K, H, W});
    cand = cand_err->data_ptr<float>();
  }
  const c10::DeviceGuard guard(fw.device());
  rs::dense_multi_flow_launch(fw.data_ptr<float>(), bw.data_ptr<float>(), ring_pos.data_ptr<float>(),
                              ring_score.data_ptr<float>(), idx.data_ptr<int>(), active.data_ptr<bool>(), (int)K,
                              (int)R, (int)H, (int)W, (float)alpha1, (float)alpha2, pos.data_ptr<float>(),
                              score.data_ptr<float>(), visible.data_ptr<bool>(), choice.data_ptr<int>(),
                              fb_err.data_ptr<float>(), cand, rs::current_stream());
  RS_CHECK_LAUNCH();
}
}  // namespace

TORCH_LIBRARY_FRAGMENT(raft_stir, m) {
  m.def(
      "dense_multi_flow_step(Tensor flow_fw, Tensor flow_bw, Tensor(a!) ring_pos, Tensor(b!) ring_score, Tensor idx, "
      "Tensor active, float alpha1, float alpha2, Tensor(c!) pos, Tensor(d!) score, Tensor(e!) visible, "
      "Tensor(f!) choice, Tensor(g!) fb_err, Tensor(h!)? cand_err=None) -> ()");
}

TORCH_LIBRARY_IMPL(raft_stir, CUDA, m) { m.impl("dense_multi_flow_step", &dense_multi_flow_step); }

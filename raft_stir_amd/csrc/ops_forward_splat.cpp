// torch.ops.raft_stir.forward_splat (csrc/forward_splat.hip).
#include <ATen/ATen.h>
#include "host_common.h"
#include <c10/core/DeviceGuard.h>
#include <torch/library.h>

#include <hip/hip_runtime.h>

#include <optional>

namespace rs {
void forward_splat_launch(const float* pos, const float* score, const float* values, int C, int footprint, float fill,
                          int H, int W, unsigned long long* keys, int* src_index, bool* covered, float* inv_pos,
                          float* out, hipStream_t s);
}  // namespace rs

namespace {
using at::Tensor;

constexpr int64_t kMaxCells = int64_t(1) << 31;  // exclusive: an anchor index takes the low 31 bits of a key

const char* const kOp = "forward_splat";

void check_in(const Tensor& t, const char* what, at::IntArrayRef shape) {
  TORCH_CHECK(t.scalar_type() == at::kFloat && t.sizes() == shape && t.is_contiguous(), kOp, ": ", what,
              " must be a contiguous fp32 tensor of shape ", shape, ", got ", t.scalar_type(), " ", t.sizes(),
              t.is_contiguous() ? "" : " (not contiguous)");
}

void check_out(const Tensor& t, const char* what, at::ScalarType dt, at::IntArrayRef shape) {
  TORCH_CHECK(t.scalar_type() == dt && t.sizes() == shape && t.is_contiguous(), kOp, ": ", what,
              " must be a contiguous ", dt, " tensor of shape ", shape, ", got ", t.scalar_type(), " ", t.sizes());
}

// No host synchronisation and no allocation: the workspace and the outputs are
// the caller's and the three launches go to the current stream, so the op can
// be captured in a hipGraph and replayed on other fields.
void forward_splat(const Tensor& pos, const Tensor& score, const std::optional<Tensor>& values, int64_t footprint,
                   double fill, const Tensor& keys, const Tensor& src_index, const Tensor& covered,
                   const Tensor& inv_pos, const std::optional<Tensor>& out) {
  TORCH_CHECK(pos.is_cuda(), kOp, ": GPU tensors expected");
  const bool has_values = values.has_value() && values->defined();
  const bool has_out = out.has_value() && out->defined();
  for (const Tensor* t : {&score, &keys, &src_index, &covered, &inv_pos})
    TORCH_CHECK(t->device() == pos.device(), kOp, ": all tensors must be on the same device, got ", pos.device(),
                " and ", t->device());
  for (const std::optional<Tensor>* t : {&values, &out})
    if (t->has_value() && (*t)->defined())
      TORCH_CHECK((*t)->device() == pos.device(), kOp, ": all tensors must be on the same device, got ",
                  pos.device(), " and ", (*t)->device());
  TORCH_CHECK(pos.dim() == 4 && pos.size(0) == 1 && pos.size(1) == 2, kOp, ": pos must be (1,2,H,W), got ",
              pos.sizes());
  const int64_t H = pos.size(2), W = pos.size(3);
  TORCH_CHECK(H >= 2 && W >= 2, kOp, ": H, W >= 2 expected, got H = ", H, ", W = ", W);
  TORCH_CHECK(H * W < kMaxCells, kOp, ": H*W = ", H * W, " must be below 2^31");
  TORCH_CHECK(footprint == 1 || footprint == 2, kOp, ": footprint must be 1 or 2, got ", footprint);
  check_in(pos, "pos", {1, 2, H, W});
  check_in(score, "score", {1, 1, H, W});
  TORCH_CHECK(has_values == has_out, kOp, ": out is expected iff values are given, got ",
              has_values ? "values without out" : "out without values");
  int64_t C = 0;
  if (has_values) {
    TORCH_CHECK(values->dim() == 4 && values->size(0) == 1 && values->size(1) >= 1, kOp,
                ": values must be (1,C,H,W) with C >= 1, got ", values->sizes());
    C = values->size(1);
    TORCH_CHECK(C * H * W < (int64_t(1) << 40), kOp, ": C*H*W = ", C * H * W, " is too large");
    check_in(*values, "values", {1, C, H, W});
    check_out(*out, "out", at::kFloat, {1, C, H, W});
  }
  TORCH_CHECK(keys.scalar_type() == at::kLong && keys.numel() == H * W && keys.is_contiguous(), kOp,
              ": keys must be a contiguous int64 tensor of H*W = ", H * W, " elements, got ", keys.scalar_type(), " ",
              keys.sizes());
  check_out(src_index, "src_index", at::kInt, {1, 1, H, W});
  check_out(covered, "covered", at::kBool, {1, 1, H, W});
  check_out(inv_pos, "inv_pos", at::kFloat, {1, 2, H, W});
  const c10::DeviceGuard guard(pos.device());
  rs::forward_splat_launch(pos.data_ptr<float>(), score.data_ptr<float>(),
                           has_values ? values->data_ptr<float>() : nullptr, (int)C, (int)footprint, (float)fill,
                           (int)H, (int)W, reinterpret_cast<unsigned long long*>(keys.data_ptr<int64_t>()),
                           src_index.data_ptr<int>(), covered.data_ptr<bool>(), inv_pos.data_ptr<float>(),
                           has_out ? out->data_ptr<float>() : nullptr, rs::current_stream());
  RS_CHECK_LAUNCH();
}
}  // namespace

TORCH_LIBRARY_FRAGMENT(raft_stir, m) {
  m.def(
      "forward_splat(Tensor pos, Tensor score, Tensor? values, int footprint, float fill, Tensor(a!) keys, "
      "Tensor(b!) src_index, Tensor(c!) covered, Tensor(d!) inv_pos, Tensor(e!)? out) -> ()");
}

TORCH_LIBRARY_IMPL(raft_stir, CUDA, m) { m.impl("forward_splat", &forward_splat); }

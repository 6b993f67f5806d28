// torch.ops.raft_stir.splat_inpaint (csrc/splat_inpaint.hip).
#include <ATen/ATen.h>
#include "host_common.h"
#include <c10/core/DeviceGuard.h>
#include <torch/library.h>

#include <hip/hip_runtime.h>

#include <optional>

namespace rs {
void splat_inpaint_launch(const int* src_index, const float* pos, const float* inv_in, const float* values, int C,
                          int R, float fill, int H, int W, int* col, int* donor, int* dist2, int* src_out,
                          float* inv_pos, float* out, hipStream_t s);
}  // namespace rs

namespace {
using at::Tensor;

constexpr int64_t kMaxSide = 32767;  // H, W and max_dist: d2, max_dist^2 and H*W stay below 2^31

const char* const kOp = "splat_inpaint";

void check(const Tensor& t, const char* what, at::ScalarType dt, at::IntArrayRef shape) {
  TORCH_CHECK(t.scalar_type() == dt && t.sizes() == shape && t.is_contiguous(), kOp, ": ", what,
              " must be a contiguous ", dt, " tensor of shape ", shape, ", got ", t.scalar_type(), " ", t.sizes(),
              t.is_contiguous() ? "" : " (not contiguous)");
}

// No host synchronisation and no allocation: the workspace and the outputs are
// the caller's and the three launches go to the current stream, so the op can
// be captured in a hipGraph and replayed on other maps.
void splat_inpaint(const Tensor& src_index, const Tensor& pos, const Tensor& inv_pos_in,
                   const std::optional<Tensor>& values, int64_t max_dist, double fill, const Tensor& col,
                   const Tensor& donor, const Tensor& dist2, const Tensor& src_out, const Tensor& inv_pos,
                   const std::optional<Tensor>& out) {
  TORCH_CHECK(src_index.is_cuda(), kOp, ": GPU tensors expected");
  const bool has_values = values.has_value() && values->defined();
  const bool has_out = out.has_value() && out->defined();
  for (const Tensor* t : {&pos, &inv_pos_in, &col, &donor, &dist2, &src_out, &inv_pos})
    TORCH_CHECK(t->device() == src_index.device(), kOp, ": all tensors must be on the same device, got ",
                src_index.device(), " and ", t->device());
  for (const std::optional<Tensor>* t : {&values, &out})
    if (t->has_value() && (*t)->defined())
      TORCH_CHECK((*t)->device() == src_index.device(), kOp, ": all tensors must be on the same device, got ",
                  src_index.device(), " and ", (*t)->device());
  TORCH_CHECK(src_index.dim() == 4 && src_index.size(0) == 1 && src_index.size(1) == 1, kOp,
              ": src_index must be (1,1,H,W), got ", src_index.sizes());
  const int64_t H = src_index.size(2), W = src_index.size(3);
  TORCH_CHECK(H >= 2 && W >= 2 && H <= kMaxSide && W <= kMaxSide, kOp, ": H, W in [2, ", kMaxSide,
              "] expected, got H = ", H, ", W = ", W);
  TORCH_CHECK(max_dist >= 0 && max_dist <= kMaxSide, kOp, ": max_dist must be in [0, ", kMaxSide, "], got ", max_dist);
  check(src_index, "src_index", at::kInt, {1, 1, H, W});
  check(pos, "pos", at::kFloat, {1, 2, H, W});
  check(inv_pos_in, "inv_pos_in", at::kFloat, {1, 2, H, W});
  TORCH_CHECK(has_values == has_out, kOp, ": out is expected iff values are given, got ",
              has_values ? "values without out" : "out without values");
  int64_t C = 0;
  if (has_values) {
    TORCH_CHECK(values->dim() == 4 && values->size(0) == 1 && values->size(1) >= 1, kOp,
                ": values must be (1,C,H,W) with C >= 1, got ", values->sizes());
    C = values->size(1);
    TORCH_CHECK(C * H * W < (int64_t(1) << 40), kOp, ": C*H*W = ", C * H * W, " is too large");
    check(*values, "values", at::kFloat, {1, C, H, W});
    check(*out, "out", at::kFloat, {1, C, H, W});
  }
  TORCH_CHECK(col.scalar_type() == at::kInt && col.numel() == H * W && col.is_contiguous(), kOp,
              ": col must be a contiguous int32 tensor of H*W = ", H * W, " elements, got ", col.scalar_type(), " ",
              col.sizes());
  check(donor, "donor", at::kInt, {1, 1, H, W});
  check(dist2, "dist2", at::kInt, {1, 1, H, W});
  check(src_out, "src_out", at::kInt, {1, 1, H, W});
  check(inv_pos, "inv_pos", at::kFloat, {1, 2, H, W});
  // the apply pass reads src_index and pos at other cells than the one it writes
  TORCH_CHECK(!src_out.is_alias_of(src_index) && !col.is_alias_of(src_index) && !donor.is_alias_of(src_index) &&
                  !dist2.is_alias_of(src_index),
              kOp, ": col, donor, dist2 and src_out must not share memory with src_index");
  TORCH_CHECK(!col.is_alias_of(donor) && !col.is_alias_of(dist2) && !donor.is_alias_of(dist2) &&
                  !donor.is_alias_of(src_out) && !dist2.is_alias_of(src_out) && !col.is_alias_of(src_out),
              kOp, ": col, donor, dist2 and src_out must not share memory with each other");
  TORCH_CHECK(!inv_pos.is_alias_of(inv_pos_in) && !inv_pos.is_alias_of(pos), kOp,
              ": inv_pos must not share memory with inv_pos_in or pos");
  if (has_out) TORCH_CHECK(!out->is_alias_of(*values), kOp, ": out must not share memory with values");
  const c10::DeviceGuard guard(src_index.device());
  rs::splat_inpaint_launch(src_index.data_ptr<int>(), pos.data_ptr<float>(), inv_pos_in.data_ptr<float>(),
                           has_values ? values->data_ptr<float>() : nullptr, (int)C, (int)max_dist, (float)fill, (int)H,
                           (int)W, col.data_ptr<int>(), donor.data_ptr<int>(), dist2.data_ptr<int>(),
                           src_out.data_ptr<int>(), inv_pos.data_ptr<float>(),
                           has_out ? out->data_ptr<float>() : nullptr, rs::current_stream());
  RS_CHECK_LAUNCH();
}
}  // namespace

TORCH_LIBRARY_FRAGMENT(raft_stir, m) {
  m.def(
      "splat_inpaint(Tensor src_index, Tensor pos, Tensor inv_pos_in, Tensor? values, int max_dist, float fill, "
      "Tensor(a!) col, Tensor(b!) donor, Tensor(c!) dist2, Tensor(d!) src_out, Tensor(e!) inv_pos, "
      "Tensor(f!)? out) -> ()");
}

TORCH_LIBRARY_IMPL(raft_stir, CUDA, m) { m.impl("splat_inpaint", &splat_inpaint); }

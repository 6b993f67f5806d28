// torch.ops.raft_stir.dense_compose and dense_query (csrc/dense_compose.hip).
#include <ATen/ATen.h>
#include "host_common.h"
#include <c10/core/DeviceGuard.h>
#include <torch/library.h>

#include <hip/hip_runtime.h>

namespace rs {
void dense_compose_launch(const float* base_pos, const float* base_score, const float* pos, const float* score,
                          const int32_t* delta, const float* err, int H, int W, float* pos_c, float* score_c,
                          bool* vis_c, int32_t* delta_c, float* err_c, hipStream_t s);
void dense_query_launch(const float* pos, const float* score, const float* points, int H, int W, int N, float* out,
                        bool* vis, float* out_score, hipStream_t s);
}  // namespace rs

namespace {
using at::Tensor;

constexpr int64_t kMaxCells = int64_t(1) << 31;  // exclusive: a cell index is an int

void check(const char* op, const Tensor& t, const char* what, at::ScalarType dt, at::IntArrayRef shape,
           const Tensor& like) {
  TORCH_CHECK(t.device() == like.device(), op, ": all tensors must be on the same device, got ", like.device(),
              " and ", t.device(), " (", what, ")");
  TORCH_CHECK(t.scalar_type() == dt && t.sizes() == shape && t.is_contiguous(), op, ": ", what,
              " must be a contiguous ", dt, " tensor of shape ", shape, ", got ", t.scalar_type(), " ", t.sizes(),
              t.is_contiguous() ? "" : " (not contiguous)");
}

// (H, W) of a field's pos, checked
std::pair<int64_t, int64_t> field_size(const char* op, const Tensor& pos) {
  TORCH_CHECK(pos.is_cuda(), op, ": GPU tensors expected");
  TORCH_CHECK(pos.dim() == 4 && pos.size(0) == 1 && pos.size(1) == 2, op, ": pos must be (1,2,H,W), got ",
              pos.sizes());
  const int64_t H = pos.size(2), W = pos.size(3);
  TORCH_CHECK(H >= 2 && W >= 2, op, ": H, W >= 2 expected, got H = ", H, ", W = ", W);
  TORCH_CHECK(H * W < kMaxCells, op, ": H*W = ", H * W, " must be below 2^31");
  return {H, W};
}

// No host synchronisation and no allocation: the outputs are the caller's and
// the launch goes to the current stream, so the op can be captured in a graph.
void dense_compose(const Tensor& base_pos, const Tensor& base_score, const Tensor& pos, const Tensor& score,
                   const Tensor& delta, const Tensor& fb_err, const Tensor& pos_c, const Tensor& score_c,
                   const Tensor& visible_c, const Tensor& delta_c, const Tensor& fb_err_c) {
  const char* const op = "dense_compose";
  const auto [H, W] = field_size(op, pos);
  check(op, pos, "pos", at::kFloat, {1, 2, H, W}, pos);
  check(op, score, "score", at::kFloat, {1, 1, H, W}, pos);
  check(op, delta, "delta", at::kInt, {1, 1, H, W}, pos);
  check(op, fb_err, "fb_err", at::kFloat, {1, 1, H, W}, pos);
  check(op, base_pos, "base_pos", at::kFloat, {1, 2, H, W}, pos);
  check(op, base_score, "base_score", at::kFloat, {1, 1, H, W}, pos);
  check(op, pos_c, "out pos", at::kFloat, {1, 2, H, W}, pos);
  check(op, score_c, "out score", at::kFloat, {1, 1, H, W}, pos);
  check(op, visible_c, "out visible", at::kBool, {1, 1, H, W}, pos);
  check(op, delta_c, "out delta", at::kInt, {1, 1, H, W}, pos);
  check(op, fb_err_c, "out fb_err", at::kFloat, {1, 1, H, W}, pos);
  // a thread gathers what other threads' pixels hold: an output must not be an input
  for (const Tensor* o : {&pos_c, &score_c, &visible_c, &delta_c, &fb_err_c})
    for (const Tensor* i : {&base_pos, &base_score, &pos, &score, &delta, &fb_err})
      TORCH_CHECK(!o->is_alias_of(*i), op, ": an output shares its storage with an input");
  const c10::DeviceGuard guard(pos.device());
  rs::dense_compose_launch(base_pos.data_ptr<float>(), base_score.data_ptr<float>(), pos.data_ptr<float>(),
                           score.data_ptr<float>(), delta.data_ptr<int32_t>(), fb_err.data_ptr<float>(), (int)H,
                           (int)W, pos_c.data_ptr<float>(), score_c.data_ptr<float>(), visible_c.data_ptr<bool>(),
                           delta_c.data_ptr<int32_t>(), fb_err_c.data_ptr<float>(), rs::current_stream());
  RS_CHECK_LAUNCH();
}

void dense_query(const Tensor& pos, const Tensor& score, const Tensor& points, const Tensor& out,
                 const Tensor& visible, const Tensor& out_score) {
  const char* const op = "dense_query";
  const auto [H, W] = field_size(op, pos);
  check(op, pos, "pos", at::kFloat, {1, 2, H, W}, pos);
  check(op, score, "score", at::kFloat, {1, 1, H, W}, pos);
  TORCH_CHECK(points.dim() == 3 && points.size(0) == 1 && points.size(2) == 2, op,
              ": points must be (1,N,2), got ", points.sizes());
  const int64_t N = points.size(1);
  TORCH_CHECK(N < kMaxCells, op, ": N = ", N, " must be below 2^31");
  check(op, points, "points", at::kFloat, {1, N, 2}, pos);
  check(op, out, "out positions", at::kFloat, {1, N, 2}, pos);
  check(op, visible, "out visible", at::kBool, {1, N}, pos);
  check(op, out_score, "out score", at::kFloat, {1, N}, pos);
  for (const Tensor* o : {&out, &visible, &out_score})
    for (const Tensor* i : {&pos, &score})
      TORCH_CHECK(!o->is_alias_of(*i), op, ": an output shares its storage with the field");
  if (N == 0) return;
  const c10::DeviceGuard guard(pos.device());
  rs::dense_query_launch(pos.data_ptr<float>(), score.data_ptr<float>(), points.data_ptr<float>(), (int)H, (int)W,
                         (int)N, out.data_ptr<float>(), visible.data_ptr<bool>(), out_score.data_ptr<float>(),
                         rs::current_stream());
  RS_CHECK_LAUNCH();
}
}  // namespace

TORCH_LIBRARY_FRAGMENT(raft_stir, m) {
  m.def(
      "dense_compose(Tensor base_pos, Tensor base_score, Tensor pos, Tensor score, Tensor delta, Tensor fb_err, "
      "Tensor(a!) pos_c, Tensor(b!) score_c, Tensor(c!) visible_c, Tensor(d!) delta_c, Tensor(e!) fb_err_c) -> ()");
  m.def(
      "dense_query(Tensor pos, Tensor score, Tensor points, Tensor(a!) out, Tensor(b!) visible, "
      "Tensor(c!) out_score) -> ()");
}

TORCH_LIBRARY_IMPL(raft_stir, CUDA, m) {
  m.impl("dense_compose", &dense_compose);
  m.impl("dense_query", &dense_query);
}

// torch.ops.raft_stir.backward_warp (csrc/backward_warp.hip).
#include <ATen/ATen.h>
#include "host_common.h"
#include <c10/core/DeviceGuard.h>
#include <torch/library.h>

#include <hip/hip_runtime.h>

#include <cmath>

namespace rs {
void backward_warp_f32_launch(const float* img, int64_t sc, int64_t sy, int64_t sx, int C, int Hs, int Ws,
                              const float* coords, const uint8_t* valid, int H, int W, float fill, float* out,
                              bool* ok, hipStream_t s);
void backward_warp_u8_launch(const uint8_t* img, int64_t sc, int64_t sy, int64_t sx, int C, int Hs, int Ws,
                             const float* coords, const uint8_t* valid, int H, int W, uint8_t fill, uint8_t* out,
                             bool* ok, hipStream_t s);
}  // namespace rs

namespace {
using at::Tensor;

constexpr int64_t kMaxCells = int64_t(1) << 31;  // exclusive: a cell index is an int
constexpr int64_t kMaxChannels = 16;

void check(const char* op, const Tensor& t, const char* what, at::ScalarType dt, at::IntArrayRef shape,
           const Tensor& like) {
  TORCH_CHECK(t.device() == like.device(), op, ": all tensors must be on the same device, got ", like.device(),
              " and ", t.device(), " (", what, ")");
  TORCH_CHECK(t.scalar_type() == dt && t.sizes() == shape && t.is_contiguous(), op, ": ", what,
              " must be a contiguous ", dt, " tensor of shape ", shape, ", got ", t.scalar_type(), " ", t.sizes(),
              t.is_contiguous() ? "" : " (not contiguous)");
}

// No host synchronisation and no allocation: the outputs are the caller's and
// the launch goes to the current stream, so the op can be captured in a graph.
void backward_warp(const Tensor& image, const Tensor& coords, const c10::optional<Tensor>& valid, double fill,
                   const Tensor& warped, const Tensor& ok) {
  const char* const op = "backward_warp";
  TORCH_CHECK(image.is_cuda(), op, ": GPU tensors expected");
  TORCH_CHECK(image.dim() == 4 && image.size(0) == 1, op, ": image must be (1,C,Hs,Ws), got ", image.sizes());
  const int64_t C = image.size(1), Hs = image.size(2), Ws = image.size(3);
  TORCH_CHECK(C >= 1 && C <= kMaxChannels, op, ": 1 <= C <= ", kMaxChannels, " expected, got C = ", C);
  TORCH_CHECK(Hs >= 2 && Ws >= 2, op, ": Hs, Ws >= 2 expected, got Hs = ", Hs, ", Ws = ", Ws);
  TORCH_CHECK(Hs * Ws < kMaxCells, op, ": Hs*Ws = ", Hs * Ws, " must be below 2^31");
  const auto dt = image.scalar_type();
  TORCH_CHECK(dt == at::kFloat || dt == at::kByte, op, ": image must be float32 or uint8, got ", dt);
  // the element strides of (channel, row, column), from the layout: a dimension of size 1 may report any stride
  int64_t sc, sy, sx;
  if (image.is_contiguous()) {
    sc = Hs * Ws, sy = Ws, sx = 1;
  } else {
    TORCH_CHECK(image.is_contiguous(at::MemoryFormat::ChannelsLast), op,
                ": image must be contiguous or channels-last, got strides ", image.strides());
    sc = 1, sy = Ws * C, sx = C;
  }
  TORCH_CHECK(coords.dim() == 4 && coords.size(0) == 1 && coords.size(1) == 2, op,
              ": coords must be (1,2,H,W), got ", coords.sizes());
  const int64_t H = coords.size(2), W = coords.size(3);
  TORCH_CHECK(H >= 2 && W >= 2, op, ": H, W >= 2 expected, got H = ", H, ", W = ", W);
  TORCH_CHECK(H * W < kMaxCells, op, ": H*W = ", H * W, " must be below 2^31");
  check(op, coords, "coords", at::kFloat, {1, 2, H, W}, image);
  const bool has_valid = valid.has_value() && valid->defined();
  if (has_valid) check(op, *valid, "valid", at::kBool, {1, 1, H, W}, image);
  check(op, warped, "out warped", dt, {1, C, H, W}, image);
  check(op, ok, "out ok", at::kBool, {1, 1, H, W}, image);
  if (dt == at::kByte)
    TORCH_CHECK(fill >= 0 && fill <= 255 && fill == std::floor(fill), op,
                ": fill must be an integer in [0, 255] for a uint8 image, got ", fill);
  // a thread gathers what other threads' pixels hold: an output must not be an input
  for (const Tensor* o : {&warped, &ok}) {
    TORCH_CHECK(!o->is_alias_of(image) && !o->is_alias_of(coords) && !(has_valid && o->is_alias_of(*valid)), op,
                ": an output shares its storage with an input");
  }
  TORCH_CHECK(!warped.is_alias_of(ok), op, ": the two outputs share their storage");
  const c10::DeviceGuard guard(image.device());
  const uint8_t* vp = has_valid ? reinterpret_cast<const uint8_t*>(valid->data_ptr<bool>()) : nullptr;
  if (dt == at::kFloat)
    rs::backward_warp_f32_launch(image.data_ptr<float>(), sc, sy, sx, (int)C, (int)Hs, (int)Ws,
                                 coords.data_ptr<float>(), vp, (int)H, (int)W, (float)fill, warped.data_ptr<float>(),
                                 ok.data_ptr<bool>(), rs::current_stream());
  else
    rs::backward_warp_u8_launch(image.data_ptr<uint8_t>(), sc, sy, sx, (int)C, (int)Hs, (int)Ws,
                                coords.data_ptr<float>(), vp, (int)H, (int)W, (uint8_t)fill,
                                warped.data_ptr<uint8_t>(), ok.data_ptr<bool>(), rs::current_stream());
  RS_CHECK_LAUNCH();
}
}  // namespace

TORCH_LIBRARY_FRAGMENT(raft_stir, m) {
  m.def(
      "backward_warp(Tensor image, Tensor coords, Tensor? valid, float fill, Tensor(a!) warped, Tensor(b!) ok) "
      "-> ()");
}

TORCH_LIBRARY_IMPL(raft_stir, CUDA, m) { m.impl("backward_warp", &backward_warp); }

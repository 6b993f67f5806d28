// torch.ops.raft_stir.fb_consistency / fb_track_points (csrc/fb_check.hip).
#include <ATen/ATen.h>
#include "host_common.h"
#include <c10/core/DeviceGuard.h>
#include <torch/library.h>

#include <hip/hip_runtime.h>

#include <tuple>

namespace rs {
void fb_dense_launch(const float* fw, const float* bw, int B, int H, int W, float a1, float a2, float* err,
                     bool* ok, hipStream_t s);
void fb_points_launch(const float* fw, const float* bw, const float* points, int B, int H, int W, int N, float a1,
                      float a2, float* out, float* err, bool* ok, hipStream_t s);
}  // namespace rs

namespace {
using at::Tensor;

constexpr int64_t kMaxCells = int64_t(1) << 30;  // exclusive: pixel indices stay ints
constexpr int64_t kMaxBatch = 65535;             // one grid plane per image
constexpr int64_t kMaxRows = 8 * 65535;          // grid.y of the dense kernel's 32x8 tiles
constexpr int64_t kMaxPoints = int64_t(1) << 30;

void check_flows(const char* op, const Tensor& fw, const Tensor& bw, double alpha1, double alpha2) {
  TORCH_CHECK(fw.device() == bw.device(), op, ": flow_fw and flow_bw must be on the same device, got ",
              fw.device(), " and ", bw.device());
  TORCH_CHECK(fw.is_cuda(), op, ": GPU tensors expected");
  TORCH_CHECK(fw.scalar_type() == at::kFloat && bw.scalar_type() == at::kFloat, op, ": fp32 flows expected");
  TORCH_CHECK(fw.dim() == 4 && fw.size(1) == 2, op, ": flow_fw must be (B,2,H,W)");
  TORCH_CHECK(bw.sizes() == fw.sizes(), op, ": flow_fw and flow_bw must have the same shape, got ", fw.sizes(),
              " and ", bw.sizes());
  TORCH_CHECK(fw.is_contiguous() && bw.is_contiguous(), op, ": contiguous flows expected");
  const int64_t B = fw.size(0), H = fw.size(2), W = fw.size(3);
  TORCH_CHECK(B >= 1, op, ": empty batch");
  TORCH_CHECK(H >= 2 && W >= 2, op, ": H, W >= 2 expected, got H = ", H, ", W = ", W);
  TORCH_CHECK(B <= kMaxBatch, op, ": at most ", kMaxBatch, " images per call");
  TORCH_CHECK(H * W < kMaxCells && H <= kMaxRows, op, ": H*W = ", H * W, " must be below 2^30 (and H at most ",
              kMaxRows, ")");
  // NaN fails both comparisons
  TORCH_CHECK(alpha1 >= 0.0 && alpha2 >= 0.0, op, ": alpha1 and alpha2 must be >= 0, got ", alpha1, " and ",
              alpha2);
}

// No host synchronisation: outputs come from the caching allocator and the
// kernel goes to the current stream, so both ops can be captured in a hipGraph.
std::tuple<Tensor, Tensor> fb_consistency(const Tensor& fw, const Tensor& bw, double alpha1, double alpha2) {
  check_flows("fb_consistency", fw, bw, alpha1, alpha2);
  const int64_t B = fw.size(0), H = fw.size(2), W = fw.size(3);
  const c10::DeviceGuard guard(fw.device());
  Tensor err = at::empty({B, 1, H, W}, fw.options());
  Tensor ok = at::empty({B, 1, H, W}, fw.options().dtype(at::kBool));
  rs::fb_dense_launch(fw.data_ptr<float>(), bw.data_ptr<float>(), (int)B, (int)H, (int)W, (float)alpha1,
                      (float)alpha2, err.data_ptr<float>(), ok.data_ptr<bool>(), rs::current_stream());
  RS_CHECK_LAUNCH();
  return {err, ok};
}

std::tuple<Tensor, Tensor, Tensor> fb_track_points(const Tensor& fw, const Tensor& bw, const Tensor& points,
                                                   double alpha1, double alpha2) {
  check_flows("fb_track_points", fw, bw, alpha1, alpha2);
  const int64_t B = fw.size(0), H = fw.size(2), W = fw.size(3);
  TORCH_CHECK(points.is_cuda() && points.device() == fw.device(),
              "fb_track_points: points must be on the same device as the flows, got ", points.device(), " and ",
              fw.device());
  TORCH_CHECK(points.scalar_type() == at::kFloat, "fb_track_points: fp32 points expected");
  TORCH_CHECK(points.dim() == 3 && points.size(2) == 2 && points.size(0) == B && points.size(1) >= 1,
              "fb_track_points: points must be (B,N,2) with B = ", B, " and N >= 1, got ", points.sizes());
  TORCH_CHECK(points.is_contiguous(), "fb_track_points: contiguous points expected");
  const int64_t N = points.size(1);
  TORCH_CHECK(N <= kMaxPoints, "fb_track_points: at most ", kMaxPoints, " points per image");
  const c10::DeviceGuard guard(fw.device());
  Tensor out = at::empty_like(points);
  Tensor err = at::empty({B, N}, fw.options());
  Tensor ok = at::empty({B, N}, fw.options().dtype(at::kBool));
  rs::fb_points_launch(fw.data_ptr<float>(), bw.data_ptr<float>(), points.data_ptr<float>(), (int)B, (int)H, (int)W,
                       (int)N, (float)alpha1, (float)alpha2, out.data_ptr<float>(), err.data_ptr<float>(),
                       ok.data_ptr<bool>(), rs::current_stream());
  RS_CHECK_LAUNCH();
  return {out, err, ok};
}
}  // namespace

TORCH_LIBRARY_FRAGMENT(raft_stir, m) {
  m.def("fb_consistency(Tensor flow_fw, Tensor flow_bw, float alpha1, float alpha2) -> (Tensor err, Tensor ok)");
  m.def(
      "fb_track_points(Tensor flow_fw, Tensor flow_bw, Tensor points, float alpha1, float alpha2) -> "
      "(Tensor new_points, Tensor err, Tensor ok)");
}

TORCH_LIBRARY_IMPL(raft_stir, CUDA, m) {
  m.impl("fb_consistency", &fb_consistency);
  m.impl("fb_track_points", &fb_track_points);
}

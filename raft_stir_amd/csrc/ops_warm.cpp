// torch.ops.raft_stir.forward_interpolate (csrc/forward_interp.hip).
#include <ATen/ATen.h>
#include "host_common.h"
#include <c10/core/DeviceGuard.h>
#include <torch/library.h>

#include <hip/hip_runtime.h>

namespace rs {
int forward_interp_chunk(int B, int N);
void forward_interp_launch(const float* flow, int B, int H, int W, int chunk, unsigned long long* keys,
                           float* out, hipStream_t s);
}  // namespace rs

namespace {
using at::Tensor;

// the 1/8 field of a 2048x2048 image: keeps the quadratic search short
constexpr int64_t kMaxCells = 65536;
constexpr int64_t kMaxBatch = 65535;  // one grid plane per image

// No host synchronisation: the workspace comes from the caching allocator and
// both kernels go to the current stream, so the op can be captured in a hipGraph.
Tensor forward_interpolate(const Tensor& flow, const c10::optional<Tensor>& out_) {
  TORCH_CHECK(flow.is_cuda(), "forward_interpolate: GPU tensor expected");
  TORCH_CHECK(flow.scalar_type() == at::kFloat, "forward_interpolate: fp32 flow expected");
  TORCH_CHECK(flow.dim() == 4 && flow.size(1) == 2, "forward_interpolate: flow must be (B,2,H,W)");
  TORCH_CHECK(flow.is_contiguous(), "forward_interpolate: contiguous flow expected");
  const int64_t B = flow.size(0), H = flow.size(2), W = flow.size(3);
  TORCH_CHECK(B >= 1 && H >= 1 && W >= 1, "forward_interpolate: empty flow");
  TORCH_CHECK(B <= kMaxBatch, "forward_interpolate: at most ", kMaxBatch, " images per call");
  TORCH_CHECK(H * W <= kMaxCells, "forward_interpolate: H*W = ", H * W, " exceeds the limit of ", kMaxCells,
              " cells (the 1/8 field of a 2048x2048 image)");
  Tensor out;
  if (out_.has_value()) {
    out = *out_;
    TORCH_CHECK(out.is_cuda() && out.device() == flow.device() && out.scalar_type() == at::kFloat &&
                    out.is_contiguous() && out.sizes() == flow.sizes(),
                "forward_interpolate: out must be a contiguous fp32 tensor like flow");
    TORCH_CHECK(out.data_ptr() != flow.data_ptr(), "forward_interpolate: out must not alias flow");
  } else {
    out = at::empty_like(flow);
  }
  const c10::DeviceGuard guard(flow.device());
  const int N = (int)(H * W);
  const int chunk = rs::forward_interp_chunk((int)B, N);
  const int64_t chunks = (N + chunk - 1) / chunk;
  Tensor keys = at::empty({B, chunks, (int64_t)N}, flow.options().dtype(at::kLong));
  rs::forward_interp_launch(flow.data_ptr<float>(), (int)B, (int)H, (int)W, chunk,
                            reinterpret_cast<unsigned long long*>(keys.data_ptr<int64_t>()),
                            out.data_ptr<float>(), rs::current_stream());
  RS_CHECK_LAUNCH();
  return out;
}
}  // namespace

TORCH_LIBRARY_FRAGMENT(raft_stir, m) {
  m.def("forward_interpolate(Tensor flow, Tensor(a!)? out=None) -> Tensor");
}

TORCH_LIBRARY_IMPL(raft_stir, CUDA, m) { m.impl("forward_interpolate", &forward_interpolate); }

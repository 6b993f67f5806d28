// torch.ops.raft_stir.feature_ring_step (csrc/feat_ring.hip).
#include <ATen/ATen.h>
#include <ATen/MemoryOverlap.h>
#include "host_common.h"
#include <c10/core/DeviceGuard.h>
#include <torch/library.h>

#include <hip/hip_runtime.h>

#include <cstdint>

namespace rs {
void feature_ring_launch(bool bf16, void* ring_f, void* ring_c, const void* f_new, const void* c_new, const int* idx,
                         void* x, void* ctx, int K, int R, int nf, int nc, hipStream_t s);
}  // namespace rs

namespace {
using at::Tensor;

constexpr int64_t kMaxSlots = 16;                     // as multi_flow_track_points
constexpr int64_t kMaxImageBytes = int64_t(1) << 31;  // exclusive: vector indices within an image stay ints

const char* const kOp = "feature_ring_step";

// No host synchronisation: the indices are read on the device, nothing is
// allocated and the kernel goes to the current stream, so the op can be
// captured in a hipGraph and replayed with another index row.
void feature_ring_step(const Tensor& ring_f, const Tensor& ring_c, const Tensor& f_new, const Tensor& c_new,
                       const Tensor& idx, const Tensor& x, const Tensor& ctx) {
  TORCH_CHECK(ring_f.is_cuda(), kOp, ": GPU tensors expected");
  for (const Tensor* t : {&ring_c, &f_new, &c_new, &idx, &x, &ctx})
    TORCH_CHECK(t->device() == ring_f.device(), kOp, ": all tensors must be on the same device, got ",
                ring_f.device(), " and ", t->device());
  const auto dt = ring_f.scalar_type();
  TORCH_CHECK(dt == at::kBFloat16 || dt == at::kFloat, kOp, ": bf16 or fp32 features expected, got ", dt);
  for (const Tensor* t : {&ring_c, &f_new, &c_new, &x, &ctx})
    TORCH_CHECK(t->scalar_type() == dt, kOp, ": all feature tensors must have one dtype, got ", dt, " and ",
                t->scalar_type());
  TORCH_CHECK(idx.scalar_type() == at::kInt, kOp, ": int32 idx expected, got ", idx.scalar_type());
  for (const Tensor* t : {&ring_f, &ring_c, &f_new, &c_new, &idx, &x, &ctx})
    TORCH_CHECK(t->is_contiguous(), kOp, ": contiguous tensors expected");
  TORCH_CHECK(ring_f.dim() == 4 && ring_f.size(0) >= 1 && ring_f.numel() > 0, kOp,
              ": ring_f must be (R,h,w,C) with no empty dimension, got ", ring_f.sizes());
  const int64_t R = ring_f.size(0), h = ring_f.size(1), w = ring_f.size(2), C = ring_f.size(3);
  TORCH_CHECK(ring_c.dim() == 4 && ring_c.size(0) == R && ring_c.size(1) == h && ring_c.size(2) == w &&
                  ring_c.size(3) >= 1,
              kOp, ": ring_c must be (R,h,w,Cc) = (", R, ",", h, ",", w, ",Cc), got ", ring_c.sizes());
  const int64_t Cc = ring_c.size(3);
  TORCH_CHECK(f_new.sizes() == at::IntArrayRef({1, h, w, C}), kOp, ": f_new must be (1,h,w,C) = (1,", h, ",", w, ",",
              C, "), got ", f_new.sizes());
  TORCH_CHECK(c_new.sizes() == at::IntArrayRef({1, h, w, Cc}), kOp, ": c_new must be (1,h,w,Cc) = (1,", h, ",", w,
              ",", Cc, "), got ", c_new.sizes());
  TORCH_CHECK(idx.dim() == 1 && idx.size(0) >= 2, kOp, ": idx must be (K+1,) with K >= 1, got ", idx.sizes());
  const int64_t K = idx.size(0) - 1;
  TORCH_CHECK(K <= kMaxSlots, kOp, ": at most ", kMaxSlots, " slots, got K = ", K);
  TORCH_CHECK(x.sizes() == at::IntArrayRef({3 * K, h, w, C}), kOp, ": x must be (3K,h,w,C) = (", 3 * K, ",", h, ",",
              w, ",", C, "), got ", x.sizes());
  TORCH_CHECK(ctx.sizes() == at::IntArrayRef({2 * K, h, w, Cc}), kOp, ": ctx must be (2K,h,w,Cc) = (", 2 * K, ",", h,
              ",", w, ",", Cc, "), got ", ctx.sizes());
  const int64_t es = ring_f.element_size();
  TORCH_CHECK((C * es) % 16 == 0 && (Cc * es) % 16 == 0, kOp, ": C and Cc must be whole 16-byte vectors, got C = ", C,
              " and Cc = ", Cc, " of ", es, "-byte elements");
  const int64_t bf = h * w * C * es, bc = h * w * Cc * es;
  TORCH_CHECK(bf < kMaxImageBytes && bc < kMaxImageBytes, kOp, ": an image of ", bf > bc ? bf : bc,
              " bytes; must be below 2^31");
  for (const Tensor* t : {&ring_f, &ring_c, &f_new, &c_new, &x, &ctx})
    TORCH_CHECK(reinterpret_cast<uintptr_t>(t->data_ptr()) % 16 == 0, kOp, ": tensors must be 16-byte aligned");
  // the kernel's pointers are __restrict__, and a block may read what another writes
  const Tensor* feats[] = {&ring_f, &ring_c, &f_new, &c_new, &x, &ctx};
  for (int a = 0; a < 6; ++a)
    for (int b = a + 1; b < 6; ++b)
      TORCH_CHECK(at::get_overlap_status(*feats[a], *feats[b]) == at::MemOverlapStatus::No, kOp,
                  ": the feature tensors must not overlap in memory");
  const c10::DeviceGuard guard(ring_f.device());
  rs::feature_ring_launch(dt == at::kBFloat16, ring_f.data_ptr(), ring_c.data_ptr(), f_new.data_ptr(),
                          c_new.data_ptr(), idx.data_ptr<int>(), x.data_ptr(), ctx.data_ptr(), (int)K, (int)R,
                          (int)(bf / 16), (int)(bc / 16), rs::current_stream());
  RS_CHECK_LAUNCH();
}
}  // namespace

TORCH_LIBRARY_FRAGMENT(raft_stir, m) {
  m.def(
      "feature_ring_step(Tensor(a!) ring_f, Tensor(b!) ring_c, Tensor f_new, Tensor c_new, Tensor idx, "
      "Tensor(c!) x, Tensor(d!) ctx) -> ()");
}

TORCH_LIBRARY_IMPL(raft_stir, CUDA, m) { m.impl("feature_ring_step", &feature_ring_step); }

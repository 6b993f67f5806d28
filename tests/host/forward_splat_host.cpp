// The forward-splatting rule of csrc/splat_device.h as plain loops on the
// host: the scatter and the resolve pass of csrc/forward_splat.hip with the
// atomicMin replaced by a minimum, on buffers of exactly the kernels' sizes.
// Built with AddressSanitizer and UBSan by tests/test_forward_splat_host.py,
// it shows that the index arithmetic is in bounds and defined on every test
// field before a GPU runs it.
//
//   forward_splat_host IN OUT
//   IN : int32 H, W, footprint, C; float fill; x[N], y[N], s[N], values[C*N]   (N = H*W, fp32)
//   OUT: src_index int32[N], covered uint8[N], inv_pos float[2N], out float[C*N]
#include "splat_device.h"

#include <cstdint>
#include <cstdio>
#include <vector>

namespace sp = rs::splat;

template <typename T>
static bool read_n(FILE* f, T* p, size_t n) { return n == 0 || fread(p, sizeof(T), n, f) == n; }
template <typename T>
static bool write_n(FILE* f, const T* p, size_t n) { return n == 0 || fwrite(p, sizeof(T), n, f) == n; }

int main(int argc, char** argv) {
  if (argc != 3) {
    fprintf(stderr, "usage: %s IN OUT\n", argv[0]);
    return 2;
  }
  FILE* in = fopen(argv[1], "rb");
  if (!in) return 2;
  int32_t hdr[4];
  float fill;
  if (!read_n(in, hdr, 4) || !read_n(in, &fill, 1)) return 2;
  const int H = hdr[0], W = hdr[1], footprint = hdr[2], C = hdr[3];
  if (H < 2 || W < 2 || (int64_t)H * W >= (int64_t(1) << 31) || (footprint != 1 && footprint != 2) || C < 0) return 2;
  const int N = H * W;
  std::vector<float> pos(2 * (size_t)N), score(N), values((size_t)C * N);
  if (!read_n(in, pos.data(), pos.size()) || !read_n(in, score.data(), score.size()) ||
      !read_n(in, values.data(), values.size()))
    return 2;
  fclose(in);

  // clear
  std::vector<uint64_t> keys(N, sp::kHole);
  // scatter: one "thread" per anchor pixel
  for (int n = 0; n < N; ++n) {
    const float x = pos[n], y = pos[(size_t)N + n], s = score[n];
    if (!sp::is_source(x, y, s, H, W)) continue;
    const uint32_t bits = sp::score_bits(s);
    int cell[sp::kMaxOffers], cls[sp::kMaxOffers];
    const int k = sp::offers(x, y, footprint, H, W, cell, cls);
    for (int j = 0; j < k; ++j) {
      const uint64_t key = sp::make_key(cls[j], bits, n);
      uint64_t* at = keys.data() + cell[j];
      if (key < *at) *at = key;
    }
  }
  // resolve: one "thread" per cell
  std::vector<int32_t> src_index(N);
  std::vector<uint8_t> cov(N);
  std::vector<float> inv(2 * (size_t)N), out((size_t)C * N);
  for (int c = 0; c < N; ++c) {
    const uint64_t key = keys[c];
    const bool hit = sp::covered(key);
    const int win = sp::winner(key, N);
    float ix = NAN, iy = NAN;
    if (hit) {
      ix = sp::inverse(win % W, c % W, pos[win]);
      iy = sp::inverse(win / W, c / W, pos[(size_t)N + win]);
    }
    src_index[c] = hit ? win : -1;
    cov[c] = hit;
    inv[c] = ix;
    inv[(size_t)N + c] = iy;
    for (int ch = 0; ch < C; ++ch) out[(size_t)ch * N + c] = hit ? values[(size_t)ch * N + win] : fill;
  }

  FILE* o = fopen(argv[2], "wb");
  if (!o) return 2;
  const bool ok = write_n(o, src_index.data(), src_index.size()) && write_n(o, cov.data(), cov.size()) &&
                  write_n(o, inv.data(), inv.size()) && write_n(o, out.data(), out.size());
  return (fclose(o) == 0 && ok) ? 0 : 2;
}

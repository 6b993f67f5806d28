// The rule of csrc/query_device.h as plain loops on the host: the dense pass
// and the point pass of csrc/dense_compose.hip, one "thread" per pixel and per
// point, on buffers of exactly the kernels' sizes.  Built with AddressSanitizer
// and UBSan by tests/test_dense_compose_host.py, it shows that the index
// arithmetic is in bounds and defined on every test field before a GPU runs it.
//
//   dense_compose_host IN OUT
//   IN : int32 H, W, N; base x[HW], y[HW], s[HW]; inner x[HW], y[HW], s[HW],
//        delta int32[HW], err[HW]; points float[2N] interleaved   (fp32)
//   OUT: pos float[2HW], score float[HW], visible uint8[HW], delta int32[HW],
//        err float[HW]; then positions float[2N], visible uint8[N], score float[N]
#include "query_device.h"

#include <cstdint>
#include <cstdio>
#include <vector>

namespace q = rs::query;

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
  int32_t hdr[3];
  if (!read_n(in, hdr, 3)) return 2;
  const int H = hdr[0], W = hdr[1], N = hdr[2];
  if (H < 2 || W < 2 || (int64_t)H * W >= (int64_t(1) << 31) || N < 0) return 2;
  const int HW = H * W;
  std::vector<float> base_pos(2 * (size_t)HW), base_score(HW), pos(2 * (size_t)HW), score(HW), err(HW);
  std::vector<int32_t> delta(HW);
  std::vector<float> points(2 * (size_t)N);
  if (!read_n(in, base_pos.data(), base_pos.size()) || !read_n(in, base_score.data(), base_score.size()) ||
      !read_n(in, pos.data(), pos.size()) || !read_n(in, score.data(), score.size()) ||
      !read_n(in, delta.data(), delta.size()) || !read_n(in, err.data(), err.size()) ||
      !read_n(in, points.data(), points.size()))
    return 2;
  fclose(in);

  // the dense pass: one "thread" per pixel
  std::vector<float> pos_c(2 * (size_t)HW), score_c(HW), err_c(HW);
  std::vector<uint8_t> vis_c(HW);
  std::vector<int32_t> delta_c(HW);
  for (int n = 0; n < HW; ++n) {
    float ox, oy, s, e;
    int32_t d;
    const bool vis = q::compose(pos.data(), pos.data() + HW, score.data(), delta.data(), err.data(), H, W, base_pos[n],
                                base_pos[(size_t)HW + n], base_score[n], ox, oy, s, d, e);
    pos_c[n] = ox;
    pos_c[(size_t)HW + n] = oy;
    score_c[n] = s;
    vis_c[n] = vis;
    delta_c[n] = d;
    err_c[n] = e;
  }
  // the point pass: one "thread" per point
  std::vector<float> out(2 * (size_t)N), out_score(N);
  std::vector<uint8_t> out_vis(N);
  for (size_t n = 0; n < (size_t)N; ++n) {
    float ox, oy, s;
    const bool seen = q::read(pos.data(), pos.data() + HW, score.data(), H, W, points[2 * n], points[2 * n + 1], ox,
                              oy, s);
    out[2 * n] = ox;
    out[2 * n + 1] = oy;
    out_vis[n] = seen;
    out_score[n] = s;
  }

  FILE* o = fopen(argv[2], "wb");
  if (!o) return 2;
  const bool ok = write_n(o, pos_c.data(), pos_c.size()) && write_n(o, score_c.data(), score_c.size()) &&
                  write_n(o, vis_c.data(), vis_c.size()) && write_n(o, delta_c.data(), delta_c.size()) &&
                  write_n(o, err_c.data(), err_c.size()) && write_n(o, out.data(), out.size()) &&
                  write_n(o, out_vis.data(), out_vis.size()) && write_n(o, out_score.data(), out_score.size());
  return (fclose(o) == 0 && ok) ? 0 : 2;
}

// The in-painting rule of csrc/inpaint_device.h as plain loops on the host: the
// column, row and apply pass of csrc/splat_inpaint.hip, one "thread" per cell,
// on buffers of exactly the kernels' sizes.  The row pass runs both ways the
// kernel has: from a staged copy of the block's span of col, of exactly the
// span's size, and from col in place; the two must agree.  Built with
// AddressSanitizer and UBSan by tests/test_splat_inpaint_host.py, it shows that
// the index arithmetic is in bounds and defined on every test map before a GPU
// runs it.
//
//   splat_inpaint_host IN OUT
//   IN : int32 H, W, R, C; float fill; int32 src_index[N]; float pos[2N], inv_pos[2N], values[C*N]   (N = H*W)
//   OUT: int32 src_index[N], donor[N], dist2[N]; float inv_pos[2N], out[C*N]
#include "inpaint_device.h"

#include <cstdint>
#include <cstdio>
#include <vector>

namespace ip = rs::inpaint;

constexpr int SEG = 256;  // the row pass's segment

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
  const int H = hdr[0], W = hdr[1], R = hdr[2], C = hdr[3];
  if (H < 2 || W < 2 || H > ip::kMaxSide || W > ip::kMaxSide || R < 0 || R > ip::kMaxSide || C < 0) return 2;
  const int N = H * W;
  std::vector<int32_t> src(N);
  std::vector<float> pos(2 * (size_t)N), inv_in(2 * (size_t)N), values((size_t)C * N);
  if (!read_n(in, src.data(), src.size()) || !read_n(in, pos.data(), pos.size()) ||
      !read_n(in, inv_in.data(), inv_in.size()) || !read_n(in, values.data(), values.size()))
    return 2;
  fclose(in);

  // column pass
  std::vector<int32_t> col(N);
  for (int c = 0; c < N; ++c) col[c] = ip::column_nearest(src.data(), c % W, c / W, R, H, W);
  // row pass: one "block" per (row, segment)
  std::vector<int32_t> donor(N), dist2(N);
  for (int y = 0; y < H; ++y)
    for (int x0 = 0; x0 < W; x0 += SEG) {
      const int lo = x0 - R > 0 ? x0 - R : 0;
      const int hi = x0 + SEG + R < W ? x0 + SEG + R : W;
      const int32_t* row = col.data() + (size_t)y * W;
      const std::vector<int32_t> tile(row + lo, row + hi);
      for (int x = x0; x < x0 + SEG && x < W; ++x) {
        const uint64_t key = ip::row_nearest(tile.data(), lo, lo, hi, x, y, R, H, W);
        if (key != ip::row_nearest(row, 0, lo, hi, x, y, R, H, W)) {
          fprintf(stderr, "staged and in-place row pass differ at (%d, %d)\n", x, y);
          return 1;
        }
        donor[(size_t)y * W + x] = ip::donor_of(key);
        dist2[(size_t)y * W + x] = ip::dist2_of(key);
      }
    }
  // apply pass
  std::vector<int32_t> src_out(N);
  std::vector<float> inv(2 * (size_t)N), out((size_t)C * N);
  for (int c = 0; c < N; ++c) {
    const ip::Filled f = ip::apply(c, donor[c], src.data(), pos.data(), inv_in.data(), H, W);
    src_out[c] = f.src;
    inv[c] = f.ix;
    inv[(size_t)N + c] = f.iy;
    for (int ch = 0; ch < C; ++ch) out[(size_t)ch * N + c] = f.src >= 0 ? values[(size_t)ch * N + f.win] : fill;
  }

  FILE* o = fopen(argv[2], "wb");
  if (!o) return 2;
  const bool ok = write_n(o, src_out.data(), src_out.size()) && write_n(o, donor.data(), donor.size()) &&
                  write_n(o, dist2.data(), dist2.size()) && write_n(o, inv.data(), inv.size()) &&
                  write_n(o, out.data(), out.size());
  return (fclose(o) == 0 && ok) ? 0 : 2;
}

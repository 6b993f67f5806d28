// The rule of csrc/warp_device.h as a plain loop on the host: the pass of
// csrc/backward_warp.hip, one "thread" per output cell, on buffers of exactly
// the kernel's sizes, for both dtypes and both layouts of the image, with the
// kernel's choice between the generic and the packed form.  Built with
// AddressSanitizer and UBSan by tests/test_backward_warp_host.py, it shows that
// the index arithmetic is in bounds and defined on every test field before a
// GPU runs it.
//
//   backward_warp_host IN OUT
//   IN : int32 dtype (0: fp32, 1: uint8), layout (0: planar, 1: channels-last),
//        C, Hs, Ws, H, W, has_valid, fill (uint8 images); float fill (fp32
//        images); the image in its memory order, C*Hs*Ws elements; coords
//        float[2HW] (x plane, y plane); valid uint8[HW] if has_valid
//   OUT: warped T[C*HW] planar; ok uint8[HW]
#include "warp_device.h"

#include <cstdint>
#include <cstdio>
#include <vector>

namespace w = rs::warp;

template <typename T>
static bool read_n(FILE* f, T* p, size_t n) { return n == 0 || fread(p, sizeof(T), n, f) == n; }
template <typename T>
static bool write_n(FILE* f, const T* p, size_t n) { return n == 0 || fwrite(p, sizeof(T), n, f) == n; }

template <typename T>
static int run(FILE* in, const char* dst, int layout, int C, int Hs, int Ws, int H, int W, bool has_valid, T fill) {
  const int64_t N = (int64_t)H * W;
  std::vector<T> img((size_t)C * Hs * Ws);
  std::vector<float> coords(2 * (size_t)N);
  std::vector<uint8_t> valid(has_valid ? (size_t)N : 0);
  if (!read_n(in, img.data(), img.size()) || !read_n(in, coords.data(), coords.size()) ||
      !read_n(in, valid.data(), valid.size()))
    return 2;
  const int64_t sc = layout ? 1 : (int64_t)Hs * Ws, sy = layout ? (int64_t)Ws * C : Ws, sx = layout ? C : 1;
  // the launch's condition for the packed form
  const bool pack4 = C == 4 && sc == 1 && sx == 4 && sy % 4 == 0 && (uintptr_t)img.data() % (4 * sizeof(T)) == 0;
  const bool pack3 = C == 3 && sc == 1 && sx == 3;
  const bool pack = pack4 || pack3;
  std::vector<T> out((size_t)C * N);
  std::vector<uint8_t> ok(N);
  for (int64_t n = 0; n < N; ++n) {
    const float x = coords[n], y = coords[(size_t)N + n];
    const bool v = has_valid ? valid[n] != 0 : true;
    T* const o = out.data();
    ok[n] = pack4   ? w::pixel_packed<T, 4, 4 * (int)sizeof(T)>(img.data(), sy, sx, Hs, Ws, x, y, v, fill, o, N, n)
            : pack3 ? w::pixel_packed<T, 3, (int)sizeof(T)>(img.data(), sy, sx, Hs, Ws, x, y, v, fill, o, N, n)
                    : w::pixel(img.data(), sc, sy, sx, C, Hs, Ws, x, y, v, fill, o, N, n);
  }
  FILE* o = fopen(dst, "wb");
  if (!o) return 2;
  const bool good = write_n(o, out.data(), out.size()) && write_n(o, ok.data(), ok.size());
  if (fclose(o) != 0 || !good) return 2;
  return pack ? 10 : 0;  // the form taken, for the test to see
}

int main(int argc, char** argv) {
  if (argc != 3) {
    fprintf(stderr, "usage: %s IN OUT\n", argv[0]);
    return 2;
  }
  FILE* in = fopen(argv[1], "rb");
  if (!in) return 2;
  int32_t hdr[9];
  float fill;
  if (!read_n(in, hdr, 9) || !read_n(in, &fill, 1)) return 2;
  const int dtype = hdr[0], layout = hdr[1], C = hdr[2], Hs = hdr[3], Ws = hdr[4], H = hdr[5], W = hdr[6];
  const int64_t lim = int64_t(1) << 31;
  if ((dtype | 1) != 1 || (layout | 1) != 1 || C < 1 || C > 16 || Hs < 2 || Ws < 2 || H < 2 || W < 2 ||
      (int64_t)Hs * Ws >= lim || (int64_t)H * W >= lim || hdr[8] < 0 || hdr[8] > 255)
    return 2;
  const int res = dtype == 0 ? run<float>(in, argv[2], layout, C, Hs, Ws, H, W, hdr[7] != 0, fill)
                             : run<uint8_t>(in, argv[2], layout, C, Hs, Ws, H, W, hdr[7] != 0, (uint8_t)hdr[8]);
  fclose(in);
  return res;
}

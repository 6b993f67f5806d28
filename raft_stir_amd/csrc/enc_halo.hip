// Halo-tile 3x3 convolution for the encoder residual blocks
// (reference core/extractor.py:6-56: the stride-1 3x3 convs of layer1 (64 ch,
// 1/2 resolution) and layer2 (96 ch, 1/4)), forward and -- with the flipped,
// transposed packed weight -- input gradient.
//
// profiles/r2/enc_conv_tiles.txt: the implicit-GEMM tiles of conv.hip run the
// 1/2-res 64->64 conv at 125-140 us (53.8 GFLOP, 730k pixels): every block
// re-fetches the whole 64 x 576 weight matrix (73 KB) for its 64-128 pixels
// and every pixel row 9 times (once per tap), ~1.7 GB of L2->CU traffic for
// 186 MB of real HBM traffic.  Here
//  * the block's weights (COB output channels x 9 taps x CIN) are staged ONCE
//    in LDS and the block walks 12 consecutive tiles (~130 KB of LDS: one
//    block per CU at a time; pipelined: + 18 KB to stage output rows);
//  * a tile is 8 output rows x 32 pixels of one image; its 10 x 34 input
//    halo is loaded once (global -> registers, issued before or, pipelined,
//    behind the previous tile's MFMAs, written to LDS after them between two
//    barriers) and every tap reads its shifted window from LDS;
//  * v_mfma_f32_32x32x16_bf16: wave w owns output rows 2w, 2w+1 of the tile
//    (2 x 32 pixels) x COB channels; per 16-deep K slice 2 pixel-operand and
//    COB/32 weight-operand ds_read_b128 feed 2 * COB/32 MFMAs, the reads of
//    slice s+3 issued before the MFMAs of slice s (explicit lgkmcnt waits);
//  * LDS rows (a halo pixel, a weight row) are CIN*2 + 16 bytes: an odd
//    number of 16-B bank slots, so the 16 lanes of a ds_read_b128 group
//    (consecutive pixels / consecutive output channels) hit 16 distinct slots
//    at any tap shift.
// Zero padding: halo pixels outside the image are written as zeros.
#include <algorithm>
#include <cstdlib>
#include <type_traits>

#include "common.h"
#include "enc_epi.h"

namespace rs {
namespace ench {

struct HArgs {
  const bf16_t* x;  // NHWC input, xstr elements per pixel
  const bf16_t* w;  // packed [Cout_pad][9][Ktot]: (co, tap, ci) at co * 9 * Ktot + tap * Ktot + ci
  bf16_t* y;        // NHWC output, ystr elements per pixel
  int xstr, ystr, Ktot;
  int B, H, W, Cout;
  int tiles_w, tiles_img, ntiles;
  int tpb;  // consecutive tiles per block
  // optional epilogue extras (ops_conv.cpp conv3x3_halo):
  //   chs / shift: y = [relu](acc * chs + shift) [then relu(y + res)] (eval-mode BatchNorm)
  const float* chs;
  const float* shift;
  const bf16_t* res;
  int rstr, relu, res_relu;
};

template <int CIN, int COB>
struct Cfg {
  static constexpr int RPW = CIN >= 128 ? 1 : 2;  // output rows per wave (LDS: 128-ch halo rows are 272 B)
  static constexpr int TH = 4 * RPW, TW = 32;     // output tile
  static constexpr int HR = TH + 2, HC = TW + 2;  // input halo
  static constexpr int RB = CIN * 2 + 16;         // LDS bytes per halo pixel / weight row
  static constexpr int HALO_B = HR * HC * RB;
  static constexpr int W_B = 9 * COB * RB;
  static constexpr int LDS_B = W_B + HALO_B;      // one halo buffer: the next tile waits in registers
  static constexpr int CPP = CIN / 8;            // 16-B chunks per pixel
  static constexpr int NCH = HR * HC * CPP;      // chunks per halo
  static constexpr int NLD = (NCH + 255) / 256;  // per thread
  static constexpr int NMF = COB / 32;
  // pipelined epilogue (PIPE): one staged output row per wave, behind weights and halo
  static constexpr int OB = COB * 2 + 16;        // LDS bytes per staged output pixel
  static constexpr int STG_B = 4 * TW * OB;      // 4 waves x one row of TW pixels
  static constexpr int OCP = COB / 8;            // 16-B chunks per output pixel
  static constexpr int OPI = 64 / OCP;           // pixels per wave-wide 16-B access
  static constexpr int ONI = TW / OPI;           // such accesses per output row
  static_assert(CIN % 16 == 0 && COB % 32 == 0, "shape");
  static_assert(((RB / 16) & 1) == 1, "odd slot count per LDS row");
  static_assert(LDS_B + STG_B <= 160 * 1024, "LDS");
};

typedef unsigned int v4u __attribute__((ext_vector_type(4)));  // 16-B fragment (register vector)

template <int N>
__device__ __forceinline__ void wait_lgkm() {
  asm volatile("s_waitcnt lgkmcnt(%0)" ::"n"(N) : "memory");
}

// K slice S (16 deep) = tap S / (CIN/16), channels 16 * (S % (CIN/16)): one
// ds_read_b128 of the pixel operand and COB/32 of the weight operand into
// register slot S % 4 (prefetch distance 3: the reads of slice S + 3 are
// issued before the MFMAs of slice S).  Offsets are compile-time immediates.
// F[slot]: [0, RPW) pixel operands (one per output row of the wave), then NMF weight operands
template <int CIN, int COB, int S>
__device__ __forceinline__ void rd(v4u (&F)[4][4], uint32_t a0, uint32_t a1, uint32_t b) {
  using C = Cfg<CIN, COB>;
  constexpr int KS = CIN / 16, tap = S / KS, kk = S % KS, ky = tap / 3, kx = tap % 3;
  constexpr int boff = (ky * C::HC + kx) * C::RB + kk * 32;
  constexpr int aoff = (tap < 5 ? tap : tap - 5) * COB * C::RB + kk * 32;
  constexpr int sl = S % 4;
  const uint32_t ab = tap < 5 ? a0 : a1;
  asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(F[sl][0]) : "v"(b), "i"(boff) : "memory");
  if constexpr (C::RPW == 2)
    asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(F[sl][1]) : "v"(b), "i"(boff + C::HC * C::RB) : "memory");
  asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(F[sl][C::RPW]) : "v"(ab), "i"(aoff) : "memory");
  if constexpr (C::NMF == 2)
    asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(F[sl][C::RPW + 1]) : "v"(ab), "i"(aoff + 32 * C::RB) : "memory");
}

template <int CIN, int COB, int S>
struct Steps {
  using C = Cfg<CIN, COB>;
  static constexpr int NS = 9 * (CIN / 16), R = C::RPW + C::NMF;
  static_assert(3 * R <= 15, "lgkmcnt range");
  // hook(integral_constant<int, S>) runs behind slice S's MFMAs: vector work
  // placed there issues while they execute
  template <class Hook>
  __device__ __forceinline__ static void run(v4u (&F)[4][4], f32x16_t (&acc)[C::RPW][C::NMF], uint32_t a0,
                                             uint32_t a1, uint32_t b, Hook& hook) {
    if constexpr (S < NS) {
      if constexpr (S + 3 < NS) rd<CIN, COB, S + 3>(F, a0, a1, b);
      constexpr int ahead = (NS - 1 - S) < 3 ? (NS - 1 - S) : 3;  // slices issued after S
      wait_lgkm<ahead * R>();
      constexpr int sl = S % 4;
      // fence: the operands are only valid after the wait (the reads are inline asm)
      v4u f0 = F[sl][0], f1 = F[sl][1], f2 = F[sl][2], f3 = F[sl][3];
      if constexpr (R == 4)
        asm volatile("" : "+v"(f0), "+v"(f1), "+v"(f2), "+v"(f3));
      else if constexpr (R == 3)
        asm volatile("" : "+v"(f0), "+v"(f1), "+v"(f2));
      else
        asm volatile("" : "+v"(f0), "+v"(f1));
      const v4u fr[4] = {f0, f1, f2, f3};
#pragma unroll
      for (int r = 0; r < C::RPW; ++r)
#pragma unroll
        for (int mi = 0; mi < C::NMF; ++mi)
          acc[r][mi] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8_t, fr[C::RPW + mi]),
                                                               __builtin_bit_cast(bf16x8_t, fr[r]), acc[r][mi], 0, 0, 0);
      hook(std::integral_constant<int, S>{});
      Steps<CIN, COB, S + 1>::run(F, acc, a0, a1, b, hook);
    }
  }
};

// orders one wave's LDS accesses around a hand-over between its lanes (the LDS
// serves a wave's accesses in issue order; this only pins the compiler)
__device__ __forceinline__ void wave_lds_order() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// PIPE 0: the plain tile loop.  Its epilogue stores straight from the
// accumulator layout, 8 B per lane into 64 different pixels per store, and
// with a residual it loads in the same shape right before use: the compiler
// branches round every such load and waits vmcnt(0) after it, which also
// waits for the store before it, so a tile's 16 load / store pairs per lane
// run one after another.
// PIPE 1 (no residual) / 2 (residual): each wave stages its converted output
// row in LDS and stores whole pixels (16 B per lane, 8 or 16 pixels of COB
// channels per store); the residual comes in the same way; its loads and the
// next halo's go out one at a time behind the MFMAs of the K slices, none of
// them under a branch; and the barrier that publishes the next halo comes
// before the epilogue, so no wave waits on another's stores.  Same arithmetic,
// same bits (tests/test_enc_halo_pipe_gpu.py); what each step is worth:
// profiles/halo_pipe/README.md
template <int CIN, int COB, int PIPE>
__global__ __launch_bounds__(256) void enc_halo_kernel(HArgs a) {
  using C = Cfg<CIN, COB>;
  __shared__ __attribute__((aligned(16))) uint8_t lds[C::LDS_B + (PIPE ? C::STG_B : 0)];
  uint8_t* wl = lds;            // [9][COB] rows
  uint8_t* hl = lds + C::W_B;   // [HR * HC] rows
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int co0 = blockIdx.y * COB;

  // weights of this block's output channels, all taps, once
  constexpr int WCH = 9 * COB * C::CPP;
  for (int q = t; q < WCH; q += 256) {
    const int kc = q % C::CPP, r = q / C::CPP;  // r = co_local * 9 + tap
    const int col = r / 9, tap = r - col * 9;
    uint4 v = make_uint4(0u, 0u, 0u, 0u);
    if (co0 + col < a.Cout)
      v = *reinterpret_cast<const uint4*>(a.w + ((size_t)(co0 + col) * 9 + tap) * a.Ktot + kc * 8);
    *reinterpret_cast<uint4*>(wl + (tap * COB + col) * C::RB + kc * 16) = v;
  }

  uint4 pre[C::NLD];
  // chunk i of the halo of the tile at (image b, row ty0, column tx0).  PIPE:
  // every lane loads (outside the image: the tensor's first chunk) and masks,
  // so no load sits under a branch
  auto gload1 = [&](int i, int b, int ty0, int tx0) {
    const int q = t + 256 * i;
    uint4 v = make_uint4(0u, 0u, 0u, 0u);
    if constexpr (PIPE) {
      const int kc = q % C::CPP, hp = q / C::CPP;
      const int hr = hp / C::HC, hc = hp - hr * C::HC;
      const int iy = ty0 - 1 + hr, ix = tx0 - 1 + hc;
      const bool in = q < C::NCH && iy >= 0 && iy < a.H && ix >= 0 && ix < a.W;
      const size_t off = in ? ((size_t)(b * a.H + iy) * a.W + ix) * a.xstr + kc * 8 : 0;
      const uint4 ld = *reinterpret_cast<const uint4*>(a.x + off);
      const uint32_t m = in ? 0xffffffffu : 0u;
      v = make_uint4(ld.x & m, ld.y & m, ld.z & m, ld.w & m);
    } else if (q < C::NCH) {
      const int kc = q % C::CPP, hp = q / C::CPP;
      const int hr = hp / C::HC, hc = hp - hr * C::HC;
      const int iy = ty0 - 1 + hr, ix = tx0 - 1 + hc;
      if (iy >= 0 && iy < a.H && ix >= 0 && ix < a.W)
        v = *reinterpret_cast<const uint4*>(a.x + ((size_t)(b * a.H + iy) * a.W + ix) * a.xstr + kc * 8);
    }
    pre[i] = v;
  };
  auto gload = [&](int tile) {
    const int b = tile / a.tiles_img, r = tile - b * a.tiles_img;
    const int th = r / a.tiles_w;
    const int ty0 = th * C::TH, tx0 = (r - th * a.tiles_w) * C::TW;
#pragma unroll
    for (int i = 0; i < C::NLD; ++i) gload1(i, b, ty0, tx0);
  };
  auto lstore = [&]() {
    uint8_t* h = hl;
#pragma unroll
    for (int i = 0; i < C::NLD; ++i) {
      const int q = t + 256 * i;
      if (q < C::NCH) {
        const int kc = q % C::CPP, hp = q / C::CPP;
        *reinterpret_cast<uint4*>(h + hp * C::RB + kc * 16) = pre[i];
      }
    }
  };

  int tile = blockIdx.x * a.tpb;
  const int tend = min(a.ntiles, tile + a.tpb);
  if (tile < tend) {
    gload(tile);
    lstore();
  }
  if constexpr (PIPE) __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0), as in the loop below: no load is pending
  __syncthreads();
  // LDS byte addresses of this lane's fragment rows: weights (taps 0-4 / 5-8, so
  // every ds_read offset fits the 16-bit immediate) and the halo
  const uint32_t lds0 = (uint32_t)(size_t)(__attribute__((address_space(3))) uint8_t*)&lds[0];
  const uint32_t a0 = lds0 + (lane & 31) * C::RB + (lane >> 5) * 16;
  const uint32_t a1 = a0 + 5 * COB * C::RB;
  const uint32_t hb0 = lds0 + C::W_B + (wave * C::RPW * C::HC + (lane & 31)) * C::RB + (lane >> 5) * 16;
  // PIPE: this wave's staged output row, and this lane's place in a wave-wide
  // 16-B access to it (pixel sp of the access, 16-B chunk sc of the pixel)
  uint8_t* sg = lds + C::LDS_B + wave * (C::TW * C::OB);
  const int sp = lane / C::OCP, sc = lane % C::OCP;
  for (; tile < tend; ++tile) {
    const int nxt = tile + 1;
    if constexpr (!PIPE) {
      if (nxt < tend) gload(nxt);  // in flight during this tile's MFMAs
    }
    const int bi = tile / a.tiles_img, rr = tile - bi * a.tiles_img;
    const int th = rr / a.tiles_w;
    const int tx0 = (rr - th * a.tiles_w) * C::TW;
    // PIPE: the next halo's loads go out one by one behind the MFMAs of every
    // third K slice (their address arithmetic issues while the MFMAs run);
    // after the block's last tile that tile's own halo is loaded again, unused
    const int lt = nxt < tend ? nxt : tile;
    const int lb = lt / a.tiles_img, lr = lt - lb * a.tiles_img, lth = lr / a.tiles_w;
    const int lty0 = lth * C::TH, ltx0 = (lr - lth * a.tiles_w) * C::TW;
    // PIPE 2: so do the residual rows of this tile, as whole pixels
    uint4 rres[C::RPW][C::ONI];
    constexpr bool HAS_RES = PIPE == 2;
    auto rload1 = [&](int r, int i) {
      const int oy = th * C::TH + wave * C::RPW + r, ox = tx0 + i * C::OPI + sp;
      const bool in = oy < a.H && ox < a.W;
      const size_t off = in ? ((size_t)(bi * a.H + oy) * a.W + ox) * a.rstr + co0 + sc * 8 : 0;
      const uint4 ld = *reinterpret_cast<const uint4*>(a.res + off);
      const uint32_t m = in ? 0xffffffffu : 0u;
      rres[r][i] = make_uint4(ld.x & m, ld.y & m, ld.z & m, ld.w & m);
    };
    auto hook = [&](auto s) {
      constexpr int S = decltype(s)::value, k = S / 3;
      if constexpr (PIPE && S % 3 == 1 && k < C::NLD) gload1(k, lb, lty0, ltx0);
      if constexpr (HAS_RES && S % 3 == 2 && k < C::RPW * C::ONI) rload1(k / C::ONI, k % C::ONI);
    };
    static_assert(Steps<CIN, COB, 0>::NS >= 3 * C::NLD && Steps<CIN, COB, 0>::NS >= 3 * C::RPW * C::ONI,
                  "a K slice for every load");

    f32x16_t acc[C::RPW][C::NMF];
#pragma unroll
    for (int r = 0; r < C::RPW; ++r)
#pragma unroll
      for (int mi = 0; mi < C::NMF; ++mi)
#pragma unroll
        for (int j = 0; j < 16; ++j) acc[r][mi][j] = 0.f;
    const uint32_t b = hb0;
    v4u F[4][4];
    rd<CIN, COB, 0>(F, a0, a1, b);
    rd<CIN, COB, 1>(F, a0, a1, b);
    rd<CIN, COB, 2>(F, a0, a1, b);
    Steps<CIN, COB, 0>::run(F, acc, a0, a1, b, hook);

    // the next tile's halo goes to LDS BEFORE this tile's output stores: the
    // vmcnt wait for the prefetched loads then never waits on fresh stores
    // (vmcnt counts both), and the stores drain during the next tile's MFMAs
    if (nxt < tend) {
      __syncthreads();  // every wave is done reading this tile's halo
      lstore();
      // PIPE: the next halo is published here, so a wave that is through its
      // epilogue starts the next tile's MFMAs without waiting for the others'
      if constexpr (PIPE) __syncthreads();
    }
    // vmcnt(0): lstore has waited for every load of this tile, so this waits
    // for nothing (after the block's last tile: for the residual, which the
    // epilogue needs).  It tells the compiler so on the path round lstore as
    // well; without it, it puts a vmcnt(0) at the top of the loop, where it
    // waits for this tile's output stores before the next tile can start
    if constexpr (PIPE) __builtin_amdgcn_s_waitcnt(0x0F70);
    // epilogue: lane holds pixel (lane & 31) of row wave*RPW + r, channels
    // mi*32 + 8g + 4*(lane>>5) + 0..3 in acc[r][mi][4g .. 4g+3]
    {
      const int ox = tx0 + (lane & 31);
      if (a.chs) {  // eval-mode BatchNorm folded in: per-channel scale / shift (host-checked: padded, aligned)
#pragma unroll
        for (int mi = 0; mi < C::NMF; ++mi)
#pragma unroll
          for (int g = 0; g < 4; ++g) {
            const int c = co0 + mi * 32 + 8 * g + 4 * (lane >> 5);
            const float4 sv = *reinterpret_cast<const float4*>(a.chs + c);
            const float4 bv = *reinterpret_cast<const float4*>(a.shift + c);
            const float scv[4] = {sv.x, sv.y, sv.z, sv.w}, shv[4] = {bv.x, bv.y, bv.z, bv.w};
#pragma unroll
            for (int r = 0; r < C::RPW; ++r)
#pragma unroll
              for (int j = 0; j < 4; ++j) {
                float v = acc[r][mi][4 * g + j] * scv[j] + shv[j];
                acc[r][mi][4 * g + j] = a.relu ? fmaxf(v, 0.f) : v;
              }
          }
      }
      if constexpr (PIPE) {
        // per output row: [residual row -> LDS,] every lane converts its pixel's
        // channel groups into the staged row, the row leaves as whole pixels.
        // The row is this wave's own: no block barrier, issue order suffices
        uint8_t* mine = sg + (lane & 31) * C::OB + (lane >> 5) * 8;
#pragma unroll
        for (int r = 0; r < C::RPW; ++r) {
          const int oy = th * C::TH + wave * C::RPW + r;
          if (oy < a.H) {
            if constexpr (HAS_RES) {
#pragma unroll
              for (int i = 0; i < C::ONI; ++i)
                *reinterpret_cast<uint4*>(sg + (i * C::OPI + sp) * C::OB + sc * 16) = rres[r][i];
              wave_lds_order();
            }
#pragma unroll
            for (int mi = 0; mi < C::NMF; ++mi)
#pragma unroll
              for (int g = 0; g < 4; ++g) {
                uint2* q = reinterpret_cast<uint2*>(mine + (mi * 32 + 8 * g) * 2);
                float v[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) v[j] = acc[r][mi][4 * g + j];
                if constexpr (HAS_RES) {
                  const uint2 u = *q;
                  v[0] += __uint_as_float(u.x << 16);
                  v[1] += __uint_as_float(u.x & 0xffff0000u);
                  v[2] += __uint_as_float(u.y << 16);
                  v[3] += __uint_as_float(u.y & 0xffff0000u);
                  if (a.res_relu) {
#pragma unroll
                    for (int j = 0; j < 4; ++j) v[j] = fmaxf(v[j], 0.f);
                  }
                }
                *q = make_uint2(uint32_t(f2bf(v[0])) | (uint32_t(f2bf(v[1])) << 16),
                                uint32_t(f2bf(v[2])) | (uint32_t(f2bf(v[3])) << 16));
              }
            wave_lds_order();
            const size_t prow = (size_t)(bi * a.H + oy) * a.W;
#pragma unroll
            for (int i = 0; i < C::ONI; ++i) {
              const int px = i * C::OPI + sp;
              const uint4 v = *reinterpret_cast<const uint4*>(sg + px * C::OB + sc * 16);
              if (tx0 + px < a.W) *reinterpret_cast<uint4*>(a.y + (prow + tx0 + px) * a.ystr + co0 + sc * 8) = v;
            }
            wave_lds_order();  // the next row reuses the staging row
          }
        }
      } else {
#pragma unroll
      for (int r = 0; r < C::RPW; ++r) {
        const int oy = th * C::TH + wave * C::RPW + r;
        if (oy < a.H && ox < a.W) {
          const size_t pix = (size_t)(bi * a.H + oy) * a.W + ox;
          bf16_t* o = a.y + pix * a.ystr + co0;
          const bf16_t* rp = a.res ? a.res + pix * a.rstr + co0 : nullptr;
#pragma unroll
          for (int mi = 0; mi < C::NMF; ++mi)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
              const int cb = mi * 32 + 8 * g + 4 * (lane >> 5);
              if (co0 + cb < a.Cout) {
                float v[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) v[j] = acc[r][mi][4 * g + j];
                if (rp) {
                  const uint2 u = *reinterpret_cast<const uint2*>(rp + cb);
                  v[0] += __uint_as_float(u.x << 16);
                  v[1] += __uint_as_float(u.x & 0xffff0000u);
                  v[2] += __uint_as_float(u.y << 16);
                  v[3] += __uint_as_float(u.y & 0xffff0000u);
                  if (a.res_relu) {
#pragma unroll
                    for (int j = 0; j < 4; ++j) v[j] = fmaxf(v[j], 0.f);
                  }
                }
                const uint2 pk = make_uint2(uint32_t(f2bf(v[0])) | (uint32_t(f2bf(v[1])) << 16),
                                            uint32_t(f2bf(v[2])) | (uint32_t(f2bf(v[3])) << 16));
                *reinterpret_cast<uint2*>(o + cb) = pk;
              }
            }
        }
      }
      }
    }
    if constexpr (!PIPE) __syncthreads();
  }
}

// RS_HALO_PIPE=0 selects the unpipelined tile loop (A/B, tests); read once.
// enc_halo_set_pipe switches it in-process: 0 / 1, or < 0 for the environment's
int pipe_env() {
  static const int v = [] {
    const char* s = getenv("RS_HALO_PIPE");
    return s && s[0] == '0' && s[1] == 0 ? 0 : 1;
  }();
  return v;
}
int g_pipe = -1;
bool pipe_enabled() { return (g_pipe < 0 ? pipe_env() : g_pipe) != 0; }

// RS_HALO_TPB: in-situ A/B of the tiles per block of the >= 1024-block route; read once
int tpb_override() {
  static const int v = [] {
    const char* s = getenv("RS_HALO_TPB");
    return s ? atoi(s) : 0;
  }();
  return v;
}

}  // namespace ench

// Supported (cin, cout-block) instantiations; false = caller falls back.
bool enc_halo_supported(int cin, int cout) {
  return (cin == 64 && cout % 64 == 0) || (cin == 96 && cout % 32 == 0);
}

bool enc_halo_launch(const bf16_t* x, int xstr, const bf16_t* w, int Ktot, bf16_t* y, int ystr, int B, int H, int W,
                     int cin, int cout, int num_cus, const EncEpi& e, hipStream_t stream) {
  if (!enc_halo_supported(cin, cout)) return false;
  ench::HArgs a{};
  a.chs = e.chs; a.shift = e.shift; a.res = e.res; a.rstr = e.rstr; a.relu = e.relu; a.res_relu = e.res_relu;
  a.x = x; a.w = w; a.y = y;
  a.xstr = xstr; a.ystr = ystr; a.Ktot = Ktot;
  a.B = B; a.H = H; a.W = W; a.Cout = cout;
  a.tiles_w = cdiv(W, 32);
  static_assert(ench::Cfg<64, 64>::TH == ench::Cfg<96, 32>::TH, "one tile height for both channel counts");
  a.tiles_img = cdiv(H, ench::Cfg<64, 64>::TH) * a.tiles_w;
  a.ntiles = B * a.tiles_img;
  if (a.ntiles == 0) return true;
  const int cob = cin == 64 ? 64 : 32;
  const int gy = cdiv(cout, cob);
  // consecutive tiles per block (the LDS weights are loaded once per block),
  // picked by in-situ A/B (scripts/ab_halo_tpb.sh, ab_halo_tpb_infer.sh; paired
  // runs on one box): training (>= 1024 tile-blocks per conv) 12 tiles 383
  // pairs/s, 16: 380, 24: 374, 48 (~persistent): 350, 2-8: 368-379 -- the
  // encoders run these convs on two HIP streams at once and long-lived
  // CU-filling blocks of one stream serialise behind the other's; graphed
  // 1088x436 inference (< 1024) 4 tiles 286-289 FPS, 2: 278-281, 12: 266-268.
  // With the pipelined loop (RS_HALO_TPB, profiles/halo_pipe/README.md): 8 tiles
  // 17.07 ms/step, 12: 17.01, 16: 17.04, 24: 17.11 -- 12 stays
  a.tpb = a.ntiles * gy >= 1024 ? 12 : 4;
  if (ench::tpb_override() > 0 && a.ntiles * gy >= 1024) a.tpb = ench::tpb_override();
  const int gx = cdiv(a.ntiles, a.tpb);
  // the pipelined epilogue moves whole 16-B chunks of y (and res)
  const bool wide = ystr % 8 == 0 && (uintptr_t)y % 16 == 0 && (!e.res || (e.rstr % 8 == 0 && (uintptr_t)e.res % 16 == 0));
  const bool pipe = ench::pipe_enabled() && wide;
  const int mode = pipe ? (e.res ? 2 : 1) : 0;
#define HALO_GO(CI, CO, P) \
  hipLaunchKernelGGL((ench::enc_halo_kernel<CI, CO, P>), dim3(gx, gy), dim3(256), 0, stream, a)
  if (cin == 64) {
    if (mode == 2) HALO_GO(64, 64, 2);
    else if (mode == 1) HALO_GO(64, 64, 1);
    else HALO_GO(64, 64, 0);
  } else {
    if (mode == 2) HALO_GO(96, 32, 2);
    else if (mode == 1) HALO_GO(96, 32, 1);
    else HALO_GO(96, 32, 0);
  }
#undef HALO_GO
  return true;
}

void enc_halo_set_pipe(int on) { ench::g_pipe = on < 0 ? ench::pipe_env() : (on ? 1 : 0); }

}  // namespace rs

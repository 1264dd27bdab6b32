// Conv mode "f64" (5): every dot product accumulated in binary64 on the fp64 matrix cores, rounded ONCE to fp32.
//
//   out = fl32(bias + sum a * w)
//
// a, w are the fp32 blob / parameter values widened to binary64 in registers: a product of two fp32 values is exact in
// binary64 (24 + 24 significand bits <= 53), so the only errors are the K + 1 additions of the binary64 sum -- at most
// (K + 1) 2^-53 sum|a w| -- and the final rounding.  It is the best answer fp32 blobs can hold and serves as the
// on-device truth the drift of the other modes is measured against (tools/precision_ladder.py); it is not a fast path.
//
// One kernel takes every Convolution the graph loader accepts (stride 1, group 1, 1x1 pad 0, 3x3 pad == dilation, any
// Cin / Cout >= 1), from the NHWC activations or -- the first layer -- the NCHW image, with the RAW (Cout, Cin, k, k)
// weights: an implicit GEMM on v_mfma_f64_16x16x4_f64, M = 16 pixels of one image row, N = 16 output channels, K over
// (ky, kx, cin) flattened and zero-filled up to the 16-value chunk.  A block is 4 waves = a 4 x 16 pixel tile x 64 output
// channels; every chunk is staged through LDS as fp32 and widened when the fragments are read.  Edge tiles are masked in
// H, W and Cout.  The ConvK member table is the grouped launches' (conv_fill): one launch per layer over all units.
//
// Fragment maps of the f64 MFMA (NOT the f32 ones):  A: lane holds A[m = lane & 15][k = lane >> 4], B: B[k = lane >> 4]
// [n = lane & 15], C/D: register r of a lane is D[row = (lane >> 4) + 4 r][col = lane & 15].
#pragma once
#include "conv_common.h"

namespace shf {

typedef double f64x4 __attribute__((ext_vector_type(4)));
typedef float f64_stage4 __attribute__((ext_vector_type(4)));

constexpr int F64_KC = 16;               // K values per chunk: four MFMA steps
constexpr int F64_LD = F64_KC + 1;       // LDS row pitch in floats
constexpr int F64_TH = 4, F64_TW = 16;   // pixel tile: one 16-pixel row per wave
constexpr int F64_BN = 64;               // output channels per block: four 16-wide MFMA tiles per wave

// p.dil: the dilation of a 3x3 layer (pad == dilation), 0 for a 1x1 layer; p.wp: the raw weights
template <bool NCHW>
__global__ __launch_bounds__(256) void conv_mfma_f64_kernel(ConvK p) {
  __shared__ float As[F64_TH * F64_TW * F64_LD];   // [pixel][k]
  __shared__ float Bs[F64_BN * F64_LD];            // [cout][k]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int bid = blockIdx.x;
  const int ct = bid % p.nct;
  int pt = bid / p.nct;
  const int mi = conv_find_member(p, pt);
  const ConvMember& mem = p.m[mi];
  pt -= mem.tile_start;
  int b, ty_, tx_;
  conv_split_tile(mem, pt, b, ty_, tx_);
  const int ty0 = ty_ * F64_TH, tx0 = tx_ * F64_TW;
  const int H = mem.H, W = mem.W, Cin = p.Cin, Cout = p.Cout;
  const int dil = p.dil, taps = dil ? 9 : 1;
  const int K = taps * Cin;
  const float* __restrict__ gin = NCHW ? mem.img : mem.in;
  const float* __restrict__ gw = p.wp;
  float* __restrict__ gout = mem.out;

  // staging: per chunk a thread fetches K value `kk` of four pixels (tile row j, column r0) and of four output channels
  // (r0 + 16 j), into registers while the previous chunk's MFMAs run
  const int kk = tid & 15, r0 = tid >> 4;
  f64_stage4 ra, rb;
  auto fetch = [&](int k0) {
    const int kidx = k0 + kk;
    const bool kin = kidx < K;   // (the zero fill of the last chunk)
    const int tap = kin ? kidx / Cin : 0;
    const int ci = kin ? kidx - tap * Cin : 0;
    const int ky = tap / 3, kx = tap - ky * 3;
    const int ix = tx0 + r0 + (kx - 1) * dil;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int iy = ty0 + j + (ky - 1) * dil;
      float v = 0.f;
      if (kin && (unsigned)iy < (unsigned)H && (unsigned)ix < (unsigned)W)
        v = NCHW ? gin[((size_t)(b * Cin + ci) * H + iy) * W + ix] : gin[((size_t)(b * H + iy) * W + ix) * p.in_stride + ci];
      ra[j] = v;
      const int co = ct * F64_BN + r0 + 16 * j;
      rb[j] = (kin && co < Cout) ? gw[((size_t)co * Cin + ci) * taps + tap] : 0.f;
    }
  };

  f64x4 acc[4];
#pragma unroll
  for (int nt = 0; nt < 4; ++nt) acc[nt] = f64x4{0.0, 0.0, 0.0, 0.0};
  const int a_off = (wave * 16 + (lane & 15)) * F64_LD + (lane >> 4);
  const int b_off = (lane & 15) * F64_LD + (lane >> 4);

  fetch(0);
  for (int k0 = 0; k0 < K; k0 += F64_KC) {
    __syncthreads();   // every wave is done reading the previous chunk
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      As[(j * 16 + r0) * F64_LD + kk] = ra[j];
      Bs[(r0 + 16 * j) * F64_LD + kk] = rb[j];
    }
    __syncthreads();
    if (k0 + F64_KC < K) fetch(k0 + F64_KC);
#pragma unroll
    for (int ks = 0; ks < F64_KC / 4; ++ks) {
      const double a = (double)As[a_off + ks * 4];
#pragma unroll
      for (int nt = 0; nt < 4; ++nt) {
        if (ct * F64_BN + nt * 16 < Cout) {   // (wave-uniform: an MFMA tile wholly past Cout is skipped)
          const double w = (double)Bs[b_off + nt * 16 * F64_LD + ks * 4];
          acc[nt] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, w, acc[nt], 0, 0, 0);
        }
      }
    }
  }

  // epilogue: bias added in binary64, ONE rounding to fp32, then ReLU
  const int y = ty0 + wave;
#pragma unroll
  for (int nt = 0; nt < 4; ++nt) {
    const int co = ct * F64_BN + nt * 16 + (lane & 15);
    if (co >= Cout || y >= H) continue;
    const double bv = p.bias ? (double)p.bias[co] : 0.0;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int x = tx0 + (lane >> 4) + 4 * r;
      if (x >= W) continue;
      float v = (float)(acc[nt][r] + bv);
      if (p.flags & CONV_RELU) v = fmaxf(v, 0.f);
      gout[((size_t)(b * H + y) * W + x) * p.out_stride + co] = v;
    }
  }
}

static const ConvKernel kF64Kernels[2] = {{(const void*)conv_mfma_f64_kernel<false>, PC_CONV_F64, 0},   // (static __shared__)
                                          {(const void*)conv_mfma_f64_kernel<true>, PC_CONV_F64, 0}};

static ConvPlan plan_conv_f64(const ConvArgs* as, int n) {
  ConvPlan pl;
  const ConvArgs& a = as[0];
  const int nct = (a.out.C + F64_BN - 1) / F64_BN;
  const long long tiles = conv_fill(pl, as, n, nct, F64_TH, F64_TW, /*scalar_loads=*/true);
  if (tiles < 0) return pl;
  if (!((a.k == 3 && a.pad == a.dil && a.dil >= 1) || (a.k == 1 && a.pad == 0))) {
    pl.err = "conv (f64 mode): only 3x3 pad == dilation and 1x1 pad 0";
    return pl;
  }
  if (!a.wraw || a.pool.p) {
    pl.err = "conv (f64 mode): raw weights required, no fused pool";
    return pl;
  }
  for (int i = 1; i < n; ++i)
    if (as[i].wraw != a.wraw || as[i].pad != a.pad || !as[i].f64) {
      pl.err = "conv group: members must share the layer";
      return pl;
    }
  pl.k.wp = a.wraw;
  pl.k.dil = a.k == 3 ? a.dil : 0;
  pl.k.range_flag = nullptr;
  pl.l[pl.nl++] = {&kF64Kernels[a.img ? 1 : 0], dim3((unsigned)(tiles * nct)), dim3(256), 0, 0, 0, 1.0};
  return pl;
}

}  // namespace shf

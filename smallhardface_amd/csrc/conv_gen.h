// The general-geometry convolution: any square kernel k, any stride, pad and dilation, any Cin / Cout >= 1 (group 1).
//
// conv_mfma_gen_kernel takes every Convolution outside the "same" family the other kernels are written for (stride 1 and
// 3x3 pad == dilation or 1x1 pad 0): the stride-2 extra layers and shortcuts of SSD / ResNet style detectors, 7x7 stems on the
// image, 5x5 context branches, "valid" layers.  An implicit GEMM, M = output pixels, N = output channels, K flattened over
// (ky, kx, cin) with cin fastest and zero-filled up to the 32-value chunk:
//   * a block is 4 waves = a 4 x 16 patch of the OUTPUT map of one member x 64 output channels; tiles are masked in H, W, Cout;
//   * fp32 (every conv mode but f64): v_mfma_f32_32x32x2_f32, one 32 x 32 accumulator per wave (2 pixel halves x 2 cout
//     halves) -- issue interval and dependent latency of that form are both 64 cycles, one accumulator keeps the pipe busy;
//     bit for bit a k-ordered fmaf chain, bias added and ReLU applied in the epilogue;
//   * f64 mode: v_mfma_f64_16x16x4_f64 as in conv_f64.h, a wave = one 16-pixel row x four 16-cout tiles, the fp32 values
//     widened when the fragments are read, bias added in binary64, ONE rounding to fp32;
//   * per chunk a thread gathers 8 input values (one K index, 8 pixels: out-of-image taps and the K tail are zeros) and two
//     float4 of the weights into registers TWO chunks ahead of the MFMAs (two register sets), then parks them in the OTHER
//     LDS buffer: one barrier per chunk.  With NHWC activations and Cin >= 32 a wave's gather is two contiguous 128-byte runs; the NCHW form
//     (template bool, as conv_mfma_f64_kernel's) reads a stem's input straight from the net's image -- no layout pass;
//   * weights are re-packed on commit to [ceil(K / 32)][Cout][32] in that K order (pack_conv_weights_gen), zero-filled: a
//     block's B chunk is 64 contiguous 128-byte rows;
//   * LDS rows have a pitch of 33 floats (fragment reads walk rows: 33 i mod 64 hits every bank once but one); 2 x (A + B)
//     buffers = 33 KiB, static;
//   * the epilogue stores 4 bytes per lane, 32 consecutive channels per pixel (128-byte runs) into a view of any cstride /
//     coff (a Concat member), raises the fp16 range flag and publishes the unit's max |output| like conv_direct_kernel.
// One launch covers the <= 16 lanes of a pass through the member table of ConvGenK, which -- unlike ConvMember -- holds the
// input AND the output size of every member.
#pragma once
#include <climits>

#include "conv_common.h"

namespace shf {

typedef float gen_f32x16 __attribute__((ext_vector_type(16)));
typedef double gen_f64x4 __attribute__((ext_vector_type(4)));

constexpr int GEN_KC = 32;              // K values per chunk
constexpr int GEN_LD = GEN_KC + 1;      // LDS row pitch in floats
constexpr int GEN_TH = 4, GEN_TW = 16;  // output-pixel tile
constexpr int GEN_BM = GEN_TH * GEN_TW; // 64 pixels
constexpr int GEN_BN = 64;              // output channels per block

struct ConvGenMember {
  const float* in;    // NHWC: the view's first channel; NCHW: the image
  float* out;         // the view's first channel
  unsigned* out_amax; // activation-exponent slot of the output blob (fp16 modes) or null
  int B, H, W;        // input
  int Ho, Wo;         // output
  int tiles_x, tiles_per_img, tile_start;   // over the OUTPUT map
  unsigned inv_tiles_x, inv_tiles_per_img;  // conv_split_tile's multiply-high divisors
};

struct ConvGenK {
  const float* wp;    // [ceil(K / 32)][Cout][32], K order (ky, kx, cin)
  const float* bias;
  int Cin, Cout, k, stride, pad, dil;
  int K;              // k * k * Cin
  unsigned inv_cin, inv_k;   // K index -> (tap, cin) -> (ky, kx) with conv_div
  int in_stride, out_stride;   // floats per pixel of the NHWC buffers
  int relu, nct;
  int* range_flag;
  int tile_starts[MAX_GROUP];  // m[q].tile_start again, contiguous (unused entries INT_MAX): conv_find_member
  ConvGenMember m[MAX_GROUP];
};
static_assert(sizeof(ConvGenK) <= 4096, "kernel arguments are limited to 4 KiB");

template <bool NCHW, bool F64>
__global__ __launch_bounds__(256) void conv_mfma_gen_kernel(ConvGenK p) {
  __shared__ float As[2][GEN_BM * GEN_LD];   // [pixel][k]
  __shared__ float Bs[2][GEN_BN * GEN_LD];   // [cout][k]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int bid = blockIdx.x;
  const int ct = bid % p.nct;
  int pt = bid / p.nct;
  const int mi = conv_find_member(p, pt);
  const ConvGenMember& mem = p.m[mi];
  pt -= mem.tile_start;
  int b, ty_, tx_;
  conv_split_tile(mem, pt, b, ty_, tx_);
  const int ty0 = ty_ * GEN_TH, tx0 = tx_ * GEN_TW;
  const int H = mem.H, W = mem.W, Ho = mem.Ho, Wo = mem.Wo, Cin = p.Cin, Cout = p.Cout, K = p.K;
  const float* __restrict__ gin = mem.in;
  const float* __restrict__ gw = p.wp;
  float* __restrict__ gout = mem.out;

  // staging.  A: K value `kk` of the chunk for the 8 tile pixels r0 + 8 j (tile row j >> 1, column r0 + 8 (j & 1)).
  // B: 8 consecutive K values (two float4) of output channel ct * 64 + brow.
  const int kk = tid & 31, r0 = tid >> 5;
  const int brow = tid >> 2, bq = (tid & 3) * 8;
  const int bco = ct * GEN_BN + brow;
  // chunk-invariant geometry of the thread's 8 pixels: input row / column at tap (0, 0) and the element offset there (it may
  // point outside the image: only offsets of taps inside it are ever dereferenced).  The address is linear in (ky, kx, cin):
  // per chunk ONE offset is added for all 8.
  const int iy0 = ty0 * p.stride - p.pad;            // input row of tile row 0 at ky = 0
  const int ix0 = (tx0 + r0) * p.stride - p.pad;     // input column of the thread's first pixel at kx = 0
  const long long sy = NCHW ? (long long)W : (long long)W * p.in_stride;   // elements per input row / column / channel
  const long long sx = NCHW ? 1ll : (long long)p.in_stride;
  const long long sc = NCHW ? (long long)H * W : 1ll;
  const long long img0 = NCHW ? (long long)b * Cin * H * W : (long long)b * H * W * p.in_stride;
  long long poff[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) poff[j] = img0 + (iy0 + (j >> 1) * p.stride) * sy + (ix0 + (j & 1) * 8 * p.stride) * sx;
  const int bco_c = bco < Cout ? bco : Cout - 1;     // (rows past Cout read the last row and are zeroed)
  const float* const wrow = gw + (size_t)bco_c * GEN_KC + bq;
  const size_t wchunk = (size_t)Cout * GEN_KC;
  // two register sets: chunk c + 2 is requested while chunk c is multiplied and chunk c + 1 -- requested one chunk earlier --
  // is parked.  The requests are straight-line code (a tap outside the image reads element 0 of the member's input and is
  // zeroed by a select): address arithmetic and loads are scheduled between the MFMAs of the chunk in hand, which as one
  // dependent chain leave 60 of every 64 issue cycles free.
  struct Stage { float a[8]; float4 b0, b1; };
  Stage s0, s1;
  auto fetch = [&](Stage& st, int ch) {
    const int kidx = ch * GEN_KC + kk;
    const bool kin = kidx < K;   // (the zero fill of the last chunk)
    const int tap = kin ? (int)conv_div((unsigned)kidx, (unsigned)Cin, p.inv_cin) : 0;
    const int ci = kin ? kidx - tap * Cin : 0;
    const int ky = (int)conv_div((unsigned)tap, (unsigned)p.k, p.inv_k), kx = tap - ky * p.k;
    const int dy = ky * p.dil, dx = kx * p.dil;
    const long long koff = dy * sy + dx * sx + ci * sc;
    bool vy[4], vx[2];
#pragma unroll
    for (int r = 0; r < 4; ++r) vy[r] = kin && (unsigned)(iy0 + r * p.stride + dy) < (unsigned)H;
#pragma unroll
    for (int q = 0; q < 2; ++q) vx[q] = (unsigned)(ix0 + q * 8 * p.stride + dx) < (unsigned)W;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const bool ok = vy[j >> 1] && vx[j & 1];
      const float v = gin[ok ? poff[j] + koff : 0ll];
      st.a[j] = ok ? v : 0.f;
    }
    const float* wr = wrow + (size_t)ch * wchunk;
    const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
    const float4 w0 = *(const float4*)wr, w1 = *(const float4*)(wr + 4);
    st.b0 = bco < Cout ? w0 : z;
    st.b1 = bco < Cout ? w1 : z;
  };
  auto park = [&](const Stage& st, int buf) {
#pragma unroll
    for (int j = 0; j < 8; ++j) As[buf][(r0 + 8 * j) * GEN_LD + kk] = st.a[j];
    float* d = &Bs[buf][brow * GEN_LD + bq];
    d[0] = st.b0.x; d[1] = st.b0.y; d[2] = st.b0.z; d[3] = st.b0.w;
    d[4] = st.b1.x; d[5] = st.b1.y; d[6] = st.b1.z; d[7] = st.b1.w;
  };

  gen_f32x16 acc;
  gen_f64x4 acc64[4];
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll
  for (int nt = 0; nt < 4; ++nt) acc64[nt] = gen_f64x4{0.0, 0.0, 0.0, 0.0};
  // fp32: wave = (pixel half wm, cout half wn); lane holds A[pixel wm * 32 + (lane & 31)][k = lane >> 5] and B[k][cout]
  // f64:  wave = tile row; lane holds A[pixel wave * 16 + (lane & 15)][k = lane >> 4], B[k][cout nt * 16 + (lane & 15)]
  const int wm = wave >> 1, wn = wave & 1;
  const int a_off = F64 ? (wave * 16 + (lane & 15)) * GEN_LD + (lane >> 4) : (wm * 32 + (lane & 31)) * GEN_LD + (lane >> 5);
  const int b_off = F64 ? (lane & 15) * GEN_LD + (lane >> 4) : (wn * 32 + (lane & 31)) * GEN_LD + (lane >> 5);
  auto multiply = [&](int buf) {
    const float* Ap = As[buf] + a_off;
    const float* Bp = Bs[buf] + b_off;
    if constexpr (F64) {
#pragma unroll
      for (int ks = 0; ks < GEN_KC / 4; ++ks) {
        const double a = (double)Ap[ks * 4];
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) {
          if (ct * GEN_BN + nt * 16 < Cout) {   // (wave-uniform: an MFMA tile wholly past Cout is skipped)
            const double w = (double)Bp[nt * 16 * GEN_LD + ks * 4];
            acc64[nt] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, w, acc64[nt], 0, 0, 0);
          }
        }
      }
    } else {
#pragma unroll
      for (int ks = 0; ks < GEN_KC / 2; ++ks)
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(Ap[ks * 2], Bp[ks * 2], acc, 0, 0, 0);
    }
  };

  // chunk c lives in LDS buffer c & 1 and came through register set c & 1 (every condition below is block-uniform).  Past
  // the last chunk a request repeats the last one and is dropped: request and MFMAs stay one basic block.
  const int nch = (K + GEN_KC - 1) / GEN_KC, last = nch - 1;
  fetch(s0, 0);
  fetch(s1, 1 < last ? 1 : last);
  park(s0, 0);
  __syncthreads();
  for (int c = 0; c < nch; c += 2) {
    fetch(s0, c + 2 < last ? c + 2 : last);
    multiply(0);
    if (c + 1 < nch) park(s1, 1);   // buffer 1 was last read before the previous barrier
    __syncthreads();
    if (c + 1 >= nch) break;
    fetch(s1, c + 3 < last ? c + 3 : last);
    multiply(1);
    if (c + 2 < nch) park(s0, 0);   // buffer 0 was read before the barrier above
    __syncthreads();
  }

  float amax = 0.f;   // fp16 modes: range guard + activation exponent of the consumer (conv_common.h)
  if constexpr (F64) {
    // D register r of a lane: pixel column (lane >> 4) + 4 r of the wave's row, cout lane & 15.  Bias in binary64, ONE rounding
    const int y = ty0 + wave;
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) {
      const int co = ct * GEN_BN + nt * 16 + (lane & 15);
      if (co >= Cout || y >= Ho) continue;
      const double bv = p.bias ? (double)p.bias[co] : 0.0;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int x = tx0 + (lane >> 4) + 4 * r;
        if (x >= Wo) continue;
        float v = (float)(acc64[nt][r] + bv);
        if (p.relu) v = fmaxf(v, 0.f);
        gout[((size_t)(b * Ho + y) * Wo + x) * p.out_stride + co] = v;
      }
    }
  } else {
    // C register r of a lane: tile pixel wm * 32 + (r & 3) + 8 (r >> 2) + 4 (lane >> 5), cout wn * 32 + (lane & 31)
    const int co = ct * GEN_BN + wn * 32 + (lane & 31);
    if (co < Cout) {
      const float bv = p.bias ? p.bias[co] : 0.f;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int pj = wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
        const int y = ty0 + (pj >> 4), x = tx0 + (pj & 15);
        float v = acc[r] + bv;
        if (p.relu) v = fmaxf(v, 0.f);
        if (y < Ho && x < Wo) {
          // (only what is stored counts: the unit's max must not depend on how the launch tiles the map)
          amax = fmaxf(amax, v != v ? __builtin_inff() : fabsf(v));
          gout[((size_t)(b * Ho + y) * Wo + x) * p.out_stride + co] = v;
        }
      }
    }
    conv_raise_range_flag(p.range_flag, amax);   // (every lane takes part in the wave reduction of the publish)
    conv_publish_amax(mem.out_amax, nullptr, amax);
  }
}

// (Cout, Cin, k, k) -> [ceil(K / 32)][Cout][32], K index = (ky * k + kx) * Cin + cin, zero-filled
inline size_t gen_conv_weight_floats_impl(int Cout, int Cin, int k) {
  const size_t K = (size_t)k * k * Cin;
  return (K + GEN_KC - 1) / GEN_KC * Cout * GEN_KC;
}
inline void pack_conv_weights_gen_impl(const float* w, int Cout, int Cin, int k, float* dst) {
  const size_t n = gen_conv_weight_floats_impl(Cout, Cin, k);
  for (size_t i = 0; i < n; ++i) dst[i] = 0.f;
  for (int co = 0; co < Cout; ++co)
    for (int ci = 0; ci < Cin; ++ci)
      for (int t = 0; t < k * k; ++t) {
        const size_t kidx = (size_t)t * Cin + ci;
        dst[((kidx / GEN_KC) * Cout + co) * GEN_KC + kidx % GEN_KC] = w[((size_t)co * Cin + ci) * k * k + t];
      }
}

// grouped launch over 1..16 members that share the layer (f64 follows the arguments); `img` set: the input is the NCHW image
static int launch_conv_gen_impl(const ConvArgs* as, int n, hipStream_t s) {
  if (n < 1 || n > MAX_GROUP) { set_error("conv group: 1..16 members"); return -1; }
  const ConvArgs& a = as[0];
  if (!a.wgen) { set_error("conv (general geometry): its weight pack is missing"); return -1; }
  if (a.k < 1 || a.stride < 1 || a.dil < 1 || a.pad < 0 || a.pool.p) { set_error("conv (general geometry): bad geometry"); return -1; }
  ConvGenK p{};
  p.wp = a.wgen;
  p.bias = a.bias;
  p.Cin = a.in.C; p.Cout = a.out.C;
  p.k = a.k; p.stride = a.stride; p.pad = a.pad; p.dil = a.dil;
  const long long K = (long long)a.k * a.k * a.in.C;
  // conv_div's multiply-high quotients are exact while dividend x divisor < 2^32
  if (K * a.in.C >= (1ll << 32) || K >= (1ll << 31)) { set_error("conv (general geometry): k * k * Cin * Cin exceeds 2^32"); return -1; }
  p.K = (int)K;
  p.inv_cin = conv_inv32(p.Cin);
  p.inv_k = conv_inv32(p.k);
  p.in_stride = a.in.cstride; p.out_stride = a.out.cstride;
  p.relu = a.relu ? 1 : 0;
  p.nct = (p.Cout + GEN_BN - 1) / GEN_BN;
  p.range_flag = a.f64 ? nullptr : a.range_flag;
  for (int i = 0; i < MAX_GROUP; ++i) p.tile_starts[i] = INT_MAX;
  long long tiles = 0;
  const int kext = a.dil * (a.k - 1) + 1;
  for (int i = 0; i < n; ++i) {
    const ConvArgs& q = as[i];
    if (q.in.C != p.Cin || q.out.C != p.Cout || q.in.cstride != p.in_stride || q.out.cstride != p.out_stride || q.k != a.k ||
        q.dil != a.dil || q.pad != a.pad || q.stride != a.stride || q.wgen != a.wgen || !q.img != !a.img || q.f64 != a.f64 ||
        q.relu != a.relu) {
      set_error("conv group: members must share the layer");
      return -1;
    }
    ConvGenMember& m = p.m[i];
    m.in = q.img ? q.img : q.in.p + q.in.coff;
    m.out = q.out.p + q.out.coff;
    m.out_amax = q.f64 ? nullptr : q.out_amax;
    m.B = q.in.B; m.H = q.in.H; m.W = q.in.W;
    m.Ho = q.out.H; m.Wo = q.out.W;
    // the output the kernel masks its stores by must be the one Caffe's formula gives for this input (every gathered tap
    // is bounds-checked against H, W on its own)
    if (m.H + 2 * a.pad < kext || m.W + 2 * a.pad < kext || m.Ho != (m.H + 2 * a.pad - kext) / a.stride + 1 ||
        m.Wo != (m.W + 2 * a.pad - kext) / a.stride + 1 || q.out.B != m.B || m.B < 1) {
      set_error("conv (general geometry): the output view does not have the size the geometry gives");
      return -1;
    }
    if (!m.in || !m.out) { set_error("conv (general geometry): null view"); return -1; }
    m.tile_start = (int)tiles;
    p.tile_starts[i] = (int)tiles;
    m.tiles_x = (m.Wo + GEN_TW - 1) / GEN_TW;
    m.tiles_per_img = m.tiles_x * ((m.Ho + GEN_TH - 1) / GEN_TH);
    m.inv_tiles_x = conv_inv32(m.tiles_x);
    m.inv_tiles_per_img = conv_inv32(m.tiles_per_img);
    tiles += (long long)m.tiles_per_img * m.B;
    if ((unsigned long long)m.tiles_per_img * m.B * (unsigned long long)m.tiles_per_img >= (1ull << 32)) {
      set_error("conv: more than 2^32 / tiles-per-image pixel tiles in one member (shrink the batch or the map)");
      return -1;
    }
    if ((long long)m.B * m.H * m.W >= (1ll << 31) || (long long)m.B * m.Ho * m.Wo >= (1ll << 31)) {
      set_error("conv: 2^31 pixels or more in one member");
      return -1;
    }
  }
  if (tiles * p.nct >= (1ll << 31)) { set_error("conv: grid too large"); return -1; }
  const void* fn = a.f64 ? (a.img ? (const void*)conv_mfma_gen_kernel<true, true> : (const void*)conv_mfma_gen_kernel<false, true>)
                         : (a.img ? (const void*)conv_mfma_gen_kernel<true, false> : (const void*)conv_mfma_gen_kernel<false, false>);
  void* args[] = {&p};
  (void)hipLaunchKernel(fn, dim3((unsigned)(tiles * p.nct)), dim3(256), args, 0, s);
  SHF_HIP_OK(hipGetLastError());
  return 0;
}

}  // namespace shf

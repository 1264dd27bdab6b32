// The depthwise convolution: Convolution with group == Cin and Cout = m * Cin (channel multiplier m >= 1), any square
// kernel k, any stride, pad and dilation -- the 3x3 layers of MobileNet-style backbones (caffe/src/caffe/layers/
// base_conv_layer.cpp:255-270 with group_ == channels_: one k x k filter per output channel, output channel o reads input
// channel o / m).
//
// The layer is bandwidth-bound (a 3x3 does 9 multiply-adds per output element against 8 bytes of compulsory traffic): no
// matrix cores, no LDS.  Data path as the combine kernel's (eltwise.hip) and the deconvolution's (misc.hip):
//   * NHWC fp32 in and out through views of any pixel pitch and channel offset (a Concat member);
//   * vector form: a thread owns one channel quad as a float4, consecutive lanes take consecutive quads -- every request is
//     one coalesced dwordx4; scalar form: one OUTPUT channel per thread, whenever m != 1 or the channel count, a pitch or a
//     channel offset is no multiple of 4;
//   * a thread computes a strip of kDwRows output rows at one output column.  The 3x3 dilation-1 forms at stride 1 and 2
//     (template FORM) load every input row the strip needs ONCE into registers -- 6 x 3 values at stride 1, not 4 x 9 -- and
//     all of them, with the nine weights, before the first multiply-add; neighbouring columns' overlap is left to the
//     cache (the three threads that read a pixel sit in the same or the next wave).  Every other geometry takes the generic
//     form: the same strip, taps loaded as they are used;
//   * weights are re-packed on commit to tap-major [k*k][Cout] (pack_conv_weights_dw): a wave's read of one tap is one
//     contiguous run.
// Arithmetic (fp32 form, every conv mode but f64): acc = 0, acc = fmaf(x, w, acc) over the taps in (ky, kx) order, a tap
// outside the image contributing x = 0 through a select; then + bias, then the folded ReLU -- bit for bit what
// conv_mfma_gen_kernel gives for the same layer written densely with block-diagonal weights (its k-ordered chain adds exact
// zeros for the other channels).  f64 form: products and sum in binary64, the bias added in binary64, ONE rounding to fp32,
// ReLU on the rounded value.  Built with -ffp-contract=off: nothing here is fused or re-associated behind the source's back.
// The epilogue raises the fp16 range flag and publishes the unit's real max |output| (only stored elements; NaN counts as
// inf) into the top's activation-exponent slot, like every producer on the stream.
// One launch covers the <= 16 lanes of a pass; every member carries its own input and output size.
#include <algorithm>

#include "conv_common.h"
#include "shf_internal.h"

namespace shf {

constexpr int kDwRows = 4;   // output rows per thread

struct ConvDwMember {
  const float* in;      // the view's first channel
  float* out;           // the view's first channel
  unsigned* out_amax;   // activation-exponent slot of the output blob (fp16 modes) or null
  int B, H, W;          // input
  int Ho, Wo;           // output
  int strips;           // ceil(Ho / kDwRows): row strips per image
  int row_start;        // first grid row (blockIdx.y) of this member; it has B * strips of them
  int pad_;
};
struct ConvDwK {
  const float* wp;      // [k*k][Cout]
  const float* bias;    // [Cout] or null
  int C, mult;          // output channels, channel multiplier (input channels = C / mult)
  int k, stride, pad, dil;
  int in_pitch, out_pitch;   // floats per pixel of the NHWC buffers
  int relu, n_members;
  int* range_flag;
  ConvDwMember m[MAX_GROUP];
};
static_assert(sizeof(ConvDwK) <= 4096, "kernel arguments are limited to 4 KiB");

enum { DW_GENERIC = 0, DW_3X3_S1 = 1, DW_3X3_S2 = 2 };

// FORM: DW_3X3_S1 / DW_3X3_S2 = k 3, dilation 1, stride 1 / 2 with the strip's input rows held in registers; DW_GENERIC = any
template <bool VEC, typename ACC, int FORM>
__global__ void __launch_bounds__(256) conv_dw_kernel(ConvDwK g) {
  int mi = 0;
#pragma unroll
  for (int q = 1; q < MAX_GROUP; ++q) mi += (q < g.n_members && (int)blockIdx.y >= g.m[q].row_start) ? 1 : 0;
  const ConvDwMember& p = g.m[mi];
  constexpr int V = VEC ? 4 : 1;
  const unsigned CV = (unsigned)g.C / V;
  const unsigned n = blockIdx.x * blockDim.x + threadIdx.x;
  float amax = 0.f;
  if (n < (unsigned)p.Wo * CV) {   // (no early return: every lane takes part in the wave reduction at the end)
    const int cv = (int)(n % CV), ox = (int)(n / CV);
    const int co = cv * V;                          // first output channel of the thread
    const int ci = VEC ? co : co / g.mult;          // ... and the input channel it reads (the vector form has mult == 1)
    const int srow = (int)blockIdx.y - p.row_start;
    const int b = srow / p.strips, oy0 = (srow - b * p.strips) * kDwRows;
    const int H = p.H, W = p.W;
    const float* __restrict__ gin = p.in + (size_t)b * H * W * g.in_pitch + ci;
    const float* __restrict__ gw = g.wp + co;
    const int ix0 = ox * g.stride - g.pad, iy0 = oy0 * g.stride - g.pad;   // input column / row of tap (0, 0) of the strip's first row
    ACC acc[kDwRows][V];
#pragma unroll
    for (int q = 0; q < kDwRows; ++q)
#pragma unroll
      for (int j = 0; j < V; ++j) acc[q][j] = (ACC)0;
    // one input value (quad) at (iy, ix), zero outside the image: the load goes to the image's first pixel then and a select
    // drops it -- straight-line code, the multiply-add order never depends on where the window lies
    auto fetch = [&](int iy, int ix, float (&x)[V]) {
      const bool ok = (unsigned)iy < (unsigned)H && (unsigned)ix < (unsigned)W;
      const float* src = gin + (ok ? ((size_t)iy * W + ix) * g.in_pitch : (size_t)0);
      if constexpr (VEC) {
        const float4 v = *(const float4*)src;
        x[0] = ok ? v.x : 0.f; x[1] = ok ? v.y : 0.f; x[2] = ok ? v.z : 0.f; x[3] = ok ? v.w : 0.f;
      } else {
        const float v = *src;
        x[0] = ok ? v : 0.f;
      }
    };
    auto fetch_w = [&](int tap, float (&w)[V]) {
      const float* src = gw + (size_t)tap * g.C;
      if constexpr (VEC) {
        const float4 v = *(const float4*)src;
        w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
      } else {
        w[0] = *src;
      }
    };
    if constexpr (FORM != DW_GENERIC) {
      constexpr int S = FORM == DW_3X3_S1 ? 1 : 2;
      constexpr int NR = (kDwRows - 1) * S + 3;   // input rows of the strip: 6 at stride 1, 9 at stride 2
      float x[NR][3][V], w[9][V];
#pragma unroll
      for (int r = 0; r < NR; ++r)
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) fetch(iy0 + r, ix0 + kx, x[r][kx]);
#pragma unroll
      for (int t = 0; t < 9; ++t) fetch_w(t, w[t]);
#pragma unroll
      for (int q = 0; q < kDwRows; ++q)
#pragma unroll
        for (int ky = 0; ky < 3; ++ky)
#pragma unroll
          for (int kx = 0; kx < 3; ++kx)
#pragma unroll
            for (int j = 0; j < V; ++j) {
              if constexpr (sizeof(ACC) == 8) acc[q][j] = acc[q][j] + (ACC)x[q * S + ky][kx][j] * (ACC)w[ky * 3 + kx][j];
              else acc[q][j] = fmaf(x[q * S + ky][kx][j], w[ky * 3 + kx][j], acc[q][j]);
            }
    } else {
      const int k = g.k;
      for (int ky = 0; ky < k; ++ky)
        for (int kx = 0; kx < k; ++kx) {
          float w[V], x[kDwRows][V];
          fetch_w(ky * k + kx, w);
#pragma unroll
          for (int q = 0; q < kDwRows; ++q) fetch(iy0 + q * g.stride + ky * g.dil, ix0 + kx * g.dil, x[q]);
#pragma unroll
          for (int q = 0; q < kDwRows; ++q)
#pragma unroll
            for (int j = 0; j < V; ++j) {
              if constexpr (sizeof(ACC) == 8) acc[q][j] = acc[q][j] + (ACC)x[q][j] * (ACC)w[j];
              else acc[q][j] = fmaf(x[q][j], w[j], acc[q][j]);
            }
        }
    }
    float bv[V];
#pragma unroll
    for (int j = 0; j < V; ++j) bv[j] = g.bias ? g.bias[co + j] : 0.f;
#pragma unroll
    for (int q = 0; q < kDwRows; ++q) {
      const int oy = oy0 + q;
      if (oy >= p.Ho) break;
      float o[V];
#pragma unroll
      for (int j = 0; j < V; ++j) {
        float v = (float)(acc[q][j] + (ACC)bv[j]);   // (f64: the bias in binary64, ONE rounding)
        if (g.relu) v = fmaxf(v, 0.f);
        // (only what is stored counts: the unit's max must not depend on how the launch tiles the map)
        amax = fmaxf(amax, v != v ? __builtin_inff() : fabsf(v));
        o[j] = v;
      }
      float* dst = p.out + ((size_t)((size_t)b * p.Ho + oy) * p.Wo + ox) * g.out_pitch + co;
      if constexpr (VEC) *(float4*)dst = make_float4(o[0], o[1], o[2], o[3]);
      else *dst = o[0];
    }
  }
  conv_raise_range_flag(g.range_flag, amax);
  conv_publish_amax(p.out_amax, nullptr, amax);
}

// (Cout, 1, k, k) -> [k*k][Cout]
void pack_conv_weights_dw(const float* w, int Cout, int k, float* dst) {
  const int T = k * k;
  for (int o = 0; o < Cout; ++o)
    for (int t = 0; t < T; ++t) dst[(size_t)t * Cout + o] = w[(size_t)o * T + t];
}

template <bool VEC, typename ACC>
static const void* conv_dw_form(int form) {
  return form == DW_3X3_S1   ? (const void*)conv_dw_kernel<VEC, ACC, DW_3X3_S1>
         : form == DW_3X3_S2 ? (const void*)conv_dw_kernel<VEC, ACC, DW_3X3_S2>
                             : (const void*)conv_dw_kernel<VEC, ACC, DW_GENERIC>;
}

// grouped launch over 1..16 members that share the layer (f64 follows the arguments)
int launch_conv_dw(const ConvArgs* as, int n, hipStream_t s) {
  if (n < 1 || n > MAX_GROUP) { set_error("conv group: 1..16 members"); return -1; }
  const ConvArgs& a = as[0];
  if (!a.wdw || a.dw_mult < 1) { set_error("conv (depthwise): its weight pack is missing"); return -1; }
  if (a.k < 1 || a.stride < 1 || a.dil < 1 || a.pad < 0 || a.pool.p || a.img) { set_error("conv (depthwise): bad geometry"); return -1; }
  if (a.in.C < 1 || (long long)a.in.C * a.dw_mult != a.out.C) {
    set_error("conv (depthwise): the output view does not have multiplier x input channels");
    return -1;
  }
  ConvDwK g{};
  g.wp = a.wdw;
  g.bias = a.bias;
  g.C = a.out.C; g.mult = a.dw_mult;
  g.k = a.k; g.stride = a.stride; g.pad = a.pad; g.dil = a.dil;
  g.in_pitch = a.in.cstride; g.out_pitch = a.out.cstride;
  g.relu = a.relu ? 1 : 0;
  g.n_members = n;
  g.range_flag = a.f64 ? nullptr : a.range_flag;
  bool vec = a.dw_mult == 1 && g.C % 4 == 0 && g.in_pitch % 4 == 0 && g.out_pitch % 4 == 0 && (((uintptr_t)a.wdw) & 15) == 0;
  const long long kext = (long long)a.dil * (a.k - 1) + 1;
  long long rows = 0;
  unsigned long long per_row_max = 1;
  for (int i = 0; i < n; ++i) {
    const ConvArgs& q = as[i];
    if (q.in.C != a.in.C || q.out.C != a.out.C || q.in.cstride != g.in_pitch || q.out.cstride != g.out_pitch || q.k != a.k ||
        q.dil != a.dil || q.pad != a.pad || q.stride != a.stride || q.wdw != a.wdw || q.dw_mult != a.dw_mult || q.bias != a.bias ||
        q.f64 != a.f64 || q.relu != a.relu || q.img || q.pool.p) {
      set_error("conv group: members must share the layer");
      return -1;
    }
    ConvDwMember& m = g.m[i];
    if (!q.in.p || !q.out.p) { set_error("conv (depthwise): null view"); return -1; }
    if (q.in.coff < 0 || q.out.coff < 0 || q.in.coff + q.in.C > q.in.cstride || q.out.coff + q.out.C > q.out.cstride) {
      set_error("conv (depthwise): a view exceeds its buffer's pixel");
      return -1;
    }
    m.in = q.in.p + q.in.coff;
    m.out = q.out.p + q.out.coff;
    m.out_amax = q.f64 ? nullptr : q.out_amax;
    m.B = q.in.B; m.H = q.in.H; m.W = q.in.W;
    m.Ho = q.out.H; m.Wo = q.out.W;
    // the output the kernel masks its stores by must be the one Caffe's formula gives for this input (every tap is
    // bounds-checked against H, W on its own)
    if (m.B < 1 || m.H < 1 || m.W < 1 || m.H + 2ll * a.pad < kext || m.W + 2ll * a.pad < kext ||
        m.Ho != (m.H + 2ll * a.pad - kext) / a.stride + 1 || m.Wo != (m.W + 2ll * a.pad - kext) / a.stride + 1 || q.out.B != m.B) {
      set_error("conv (depthwise): the output view does not have the size the geometry gives");
      return -1;
    }
    if ((long long)m.B * m.H * m.W >= (1ll << 31) || (long long)m.B * m.Ho * m.Wo >= (1ll << 31)) {
      set_error("conv: 2^31 pixels or more in one member");
      return -1;
    }
    vec = vec && q.in.coff % 4 == 0 && q.out.coff % 4 == 0 && (((uintptr_t)q.in.p) & 15) == 0 && (((uintptr_t)q.out.p) & 15) == 0;
    m.strips = (m.Ho + kDwRows - 1) / kDwRows;
    m.row_start = (int)rows;
    m.pad_ = 0;
    rows += (long long)m.B * m.strips;
    if (rows > 65535) { set_error("conv (depthwise): more than 65535 row strips in one launch (shrink the batch or the map)"); return -1; }
    per_row_max = std::max(per_row_max, (unsigned long long)m.Wo * (unsigned long long)g.C);
  }
  for (int i = n; i < MAX_GROUP; ++i) g.m[i] = g.m[0];
  const unsigned long long per_row = vec ? per_row_max / 4 : per_row_max;
  if (per_row >= (1ull << 31)) { set_error("conv (depthwise): 2^31 or more values in one output row"); return -1; }
  const int form = (a.k == 3 && a.dil == 1 && a.stride == 1) ? DW_3X3_S1 : (a.k == 3 && a.dil == 1 && a.stride == 2) ? DW_3X3_S2 : DW_GENERIC;
  const void* fn = a.f64 ? (vec ? conv_dw_form<true, double>(form) : conv_dw_form<false, double>(form))
                         : (vec ? conv_dw_form<true, float>(form) : conv_dw_form<false, float>(form));
  void* args[] = {&g};
  (void)hipLaunchKernel(fn, dim3((unsigned)((per_row + 255) / 256), (unsigned)rows, 1), dim3(256), args, 0, s);
  SHF_HIP_OK(hipGetLastError());
  return 0;
}

}  // namespace shf

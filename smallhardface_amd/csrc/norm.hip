// The channel-affine kernel: BatchNorm (inference), Scale and the ReLU behind them on NHWC fp32 activations as ONE launch
//
//     out[c] = act( ((in[c] - m[c]) / d[c]) * g[c] + b[c] )
//
// Every stage is optional and rounds as the layer it stands for.  Reference counterparts:
//   BatchNorm  caffe/src/caffe/layers/batch_norm_layer.cpp:98-105, 117-123, 149-161 with use_global_stats: the mean is
//              subtracted (one rounding), the result divided by sqrt(var + eps) (one rounding); m and d are formed on the
//              host in the layer's operation order (net_graph.cpp derive_norm)
//   Scale      scale_layer.cpp:131-141: top = bottom * gamma[c] (caffe_cpu_scale), then top += beta[c] with bias_term
//   ReLU       relu_layer.cpp:9-19, as eltwise.hip states it
// Built with -ffp-contract=off, so no product is fused into the add behind it; the fp32 division is the compiler's
// correctly rounded one (HIP's default: no -fno-hip-fp32-correctly-rounded-divide-sqrt, no fast-math).
//
// Data path as the combine kernel's (eltwise.hip): a thread handles one channel quad of one pixel as a float4 (consecutive
// threads = consecutive quads) for kNormRows rows, all loads issued first; the scalar form handles one channel, for channel
// counts, pitches or offsets that are no multiple of 4.  Input and output carry their own pixel pitch and channel offset: a
// channel window of a zero-copy Concat works on either side, and the output may be the input's memory (every thread reads
// its elements before it writes them, and no other thread touches them).  The per-channel vectors are read from the device
// through the cache: 4 x 16 bytes per thread next to 2 x 64 bytes of activations.  One launch covers up to 16 members of
// different map sizes, stacked along the grid's row axis; the geometry comes in a by-value argument struct.  Conv mode
// "f64": the expression in binary64 from the fp32 blobs (m and d formed in binary64 on the host), rounded once; the
// activation works on the rounded value.  At the end: max |out| of the wave (NaN counts as inf) raises the range flag
// beyond 65504 in the fp16 modes and is published into the top's activation-exponent slot (conv_common.h).
#include <algorithm>

#include "conv_common.h"
#include "shf_internal.h"

namespace shf {

constexpr int kNormRows = 4;   // rows (pixel rows of the B * H stack) per block

struct NormGM {
  const float* in;               // first channel the view reads, of pixel (0, 0)
  float* out;
  unsigned* out_amax;
  int rows, W, in_pitch, out_pitch;   // rows = B * H
  int row_start, pad_;                // first grid row (blockIdx.y) of this member
};
struct NormGK {
  int n_members, C;
  int norm, scale, bias, act;
  float slope;
  int pad_;
  const float *m, *d, *g, *b;
  const double *m64, *d64;
  int* range_flag;
  NormGM mem[16];
};

template <bool VEC, bool F64>
__global__ void __launch_bounds__(256) channel_affine_kernel(NormGK g) {
  int mi = 0;
#pragma unroll
  for (int q = 1; q < 16; ++q) mi += (q < g.n_members && (int)blockIdx.y >= g.mem[q].row_start) ? 1 : 0;
  const NormGM& p = g.mem[mi];
  constexpr int V = VEC ? 4 : 1;
  const unsigned CV = (unsigned)g.C / V;
  const unsigned n = blockIdx.x * blockDim.x + threadIdx.x;
  float amax = 0.f;
  if (n < (unsigned)p.W * CV) {   // (no early return: every lane takes part in the wave reduction at the end)
    const int cv = (int)(n % CV), ox = (int)(n / CV), c = cv * V;
    const int r0 = ((int)blockIdx.y - p.row_start) * kNormRows;
    // every load is issued before the first value is formed: the block's rows, then the channel's constants
    float x[kNormRows][V];
#pragma unroll
    for (int q = 0; q < kNormRows; ++q) {
      const int r = r0 + q;
#pragma unroll
      for (int j = 0; j < V; ++j) x[q][j] = 0.f;
      if (r < p.rows) {
        const float* src = p.in + ((size_t)r * p.W + ox) * p.in_pitch + c;
        if constexpr (VEC) {
          const float4 v = *(const float4*)src;
          x[q][0] = v.x; x[q][1] = v.y; x[q][2] = v.z; x[q][3] = v.w;
        } else {
          x[q][0] = *src;
        }
      }
    }
    float m[V], d[V], sg[V], sb[V];
    double m64[V], d64[V];
#pragma unroll
    for (int j = 0; j < V; ++j) { m[j] = 0.f; d[j] = 1.f; sg[j] = 1.f; sb[j] = 0.f; m64[j] = 0.0; d64[j] = 1.0; }
    auto fetch = [&](const float* v, float (&o)[V]) {
      if constexpr (VEC) {
        const float4 t = *(const float4*)(v + c);
        o[0] = t.x; o[1] = t.y; o[2] = t.z; o[3] = t.w;
      } else {
        o[0] = v[c];
      }
    };
    if (g.norm) {
      if constexpr (F64) {
#pragma unroll
        for (int j = 0; j < V; ++j) { m64[j] = g.m64[c + j]; d64[j] = g.d64[c + j]; }
      } else {
        fetch(g.m, m);
        fetch(g.d, d);
      }
    }
    if (g.scale) fetch(g.g, sg);
    if (g.bias) fetch(g.b, sb);
#pragma unroll
    for (int q = 0; q < kNormRows; ++q) {
      const int r = r0 + q;
      if (r >= p.rows) break;
      float o[V];
#pragma unroll
      for (int j = 0; j < V; ++j) {
        float v;
        if constexpr (F64) {
          double a = (double)x[q][j];
          if (g.norm) a = (a - m64[j]) / d64[j];
          if (g.scale) a = a * (double)sg[j];
          if (g.bias) a = a + (double)sb[j];
          v = (float)a;
        } else {
          v = x[q][j];
          if (g.norm) v = (v - m[j]) / d[j];
          if (g.scale) v = v * sg[j];
          if (g.bias) v = v + sb[j];
        }
        // std::max(x, 0) + slope * std::min(x, 0) with std::max / std::min's operand order (a NaN stays a NaN)
        if (g.act) v = (v < 0.f ? 0.f : v) + g.slope * (0.f < v ? 0.f : v);
        o[j] = v;
        amax = fmaxf(amax, fabsf(v));
        if (v != v) amax = __builtin_inff();   // (fmaxf drops NaNs)
      }
      float* dst = p.out + ((size_t)r * p.W + ox) * p.out_pitch + c;
      if constexpr (VEC) *(float4*)dst = make_float4(o[0], o[1], o[2], o[3]);
      else *dst = o[0];
    }
  }
  if (g.range_flag && !(amax <= 65504.0f)) atomicOr(g.range_flag, 1);
  conv_publish_amax(p.out_amax, nullptr, amax);
}

int launch_channel_affine_group(const NormArgs* as, int n, const NormStages& st, int f64, int* range_flag, hipStream_t s) {
  if (n < 1 || n > 16) { set_error("channel affine group: 1..16 members"); return -1; }
  if (!st.norm && !st.scale && !st.act) { set_error("channel affine: no stage to apply"); return -1; }
  if (st.bias && !st.scale) { set_error("channel affine: a bias needs the scale stage"); return -1; }
  if ((st.norm && (f64 ? (!st.m64 || !st.d64) : (!st.m || !st.d))) || (st.scale && !st.g) || (st.bias && !st.b)) {
    set_error("channel affine: a stage's per-channel vector is missing (parameters not committed)");
    return -1;
  }
  auto aligned = [](const void* q) { return (((uintptr_t)q) & 15) == 0; };
  NormGK g;
  g.n_members = n; g.C = as[0].out.C;
  g.norm = st.norm; g.scale = st.scale; g.bias = st.bias; g.act = st.act; g.slope = st.slope; g.pad_ = 0;
  g.m = st.m; g.d = st.d; g.g = st.g; g.b = st.b; g.m64 = st.m64; g.d64 = st.d64;
  g.range_flag = range_flag;
  bool vec = g.C % 4 == 0 && (!st.norm || f64 || (aligned(st.m) && aligned(st.d))) && (!st.scale || aligned(st.g)) &&
             (!st.bias || aligned(st.b));
  long long rows = 0;
  unsigned long long per_row_max = 1;
  for (int m = 0; m < n; ++m) {
    const View &in = as[m].in, &out = as[m].out;
    if (!out.p || !in.p || out.B < 1 || out.H < 1 || out.W < 1 || out.C < 1) { set_error("channel affine: empty view"); return -1; }
    if (out.C != g.C) { set_error("channel affine group: members differ in the channel count"); return -1; }
    if (in.B != out.B || in.H != out.H || in.W != out.W || in.C != out.C) { set_error("channel affine: input and output differ in shape"); return -1; }
    // every element read or written lies inside its buffer's pixel
    if (in.coff < 0 || out.coff < 0 || in.coff + in.C > in.cstride || out.coff + out.C > out.cstride) {
      set_error("channel affine: a view exceeds its buffer's pixel");
      return -1;
    }
    vec = vec && in.cstride % 4 == 0 && in.coff % 4 == 0 && aligned(in.p) && out.cstride % 4 == 0 && out.coff % 4 == 0 && aligned(out.p);
    NormGM& gm = g.mem[m];
    gm.in = in.p + in.coff;
    gm.out = out.p + out.coff;
    gm.out_amax = as[m].out_amax;
    gm.rows = out.B * out.H; gm.W = out.W; gm.in_pitch = in.cstride; gm.out_pitch = out.cstride;
    gm.row_start = (int)rows;
    gm.pad_ = 0;
    rows += ((long long)gm.rows + kNormRows - 1) / kNormRows;
    per_row_max = std::max(per_row_max, (unsigned long long)out.W * (unsigned long long)out.C);
  }
  for (int m = n; m < 16; ++m) g.mem[m] = g.mem[0];
  const unsigned long long per_row = vec ? per_row_max / 4 : per_row_max;
  if (rows > 65535 || per_row >= (1ull << 31)) { set_error("channel affine: map too large"); return -1; }
  const dim3 grid((unsigned)((per_row + 255) / 256), (unsigned)rows, 1), block(256);
  if (f64) {
    if (vec) hipLaunchKernelGGL((channel_affine_kernel<true, true>), grid, block, 0, s, g);
    else hipLaunchKernelGGL((channel_affine_kernel<false, true>), grid, block, 0, s, g);
  } else {
    if (vec) hipLaunchKernelGGL((channel_affine_kernel<true, false>), grid, block, 0, s, g);
    else hipLaunchKernelGGL((channel_affine_kernel<false, false>), grid, block, 0, s, g);
  }
  SHF_HIP_OK(hipGetLastError());
  return 0;
}

}  // namespace shf

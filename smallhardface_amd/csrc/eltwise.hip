// The "combine" kernel family: Eltwise, Crop and a free-standing (leaky) ReLU on NHWC fp32 activations as ONE launch form
//
//     out[view] = act( op over i < n of  coeff_i * in_i[view_i shifted by (y0_i, x0_i, c0_i)] )
//
// n = 1 .. 4, op = SUM / PROD / MAX / COPY, act = identity or max(x, 0) + slope * min(x, 0).  Reference counterparts:
//   Eltwise   caffe/src/caffe/layers/eltwise_layer.cpp:42-80 (SUM: top = 0, then top += coeff_i * bottom_i in bottom order;
//             PROD and MAX left to right; MAX keeps the LATER operand on a tie or a NaN, like its `a > b ? a : b` chain)
//   Crop      crop_layer.cpp:80-130 (a copy from an offset window): COPY with n = 1
//   ReLU      relu_layer.cpp:9-19: COPY with n = 1 and the activation, possibly in place
// Built with -ffp-contract=off: coeff * x and the add round separately, as the reference's axpy over fp32 does.
//
// Every input carries its own source height, width, pixel pitch and crop origin: a View has no row pitch, so a spatial
// crop cannot be a zero-copy view, and folding a Crop into the Eltwise that reads it means reading through the offset.
// Data path as in misc.hip's deconvolution kernels: a thread handles one channel quad of one output pixel as a float4
// (consecutive threads = consecutive quads: one dwordx4 request per lane, coalesced) for kCombineRows rows, all loads issued first; the
// scalar form handles one channel, for channel counts, pitches or offsets that are no multiple of 4.  One launch covers up
// to 16 members of different sizes (the lanes of a grouped pass), stacked along the grid's row axis; the geometry comes in
// a by-value argument struct.  At the end: max |out| of the wave (NaN counts as inf) raises the range flag beyond 65504 in
// the fp16 modes and is published into the top's activation-exponent slot (conv_common.h) -- the REAL maximum, since a
// coefficient, a crop or a slope changes the bottoms' bound.
#include <algorithm>

#include "conv_common.h"
#include "shf_internal.h"

namespace shf {

constexpr int kCombineRows = 4;   // output rows per block

struct CombineIn {
  const float* p;          // first channel the view reads, of source pixel (0, 0)
  int H, W, pitch;         // source map size, floats per source pixel
  int y0, x0;              // crop origin inside the source
  int pad_;
};
struct CombineGM {
  CombineIn in[kCombineMaxIn];
  float* out;
  unsigned* out_amax;
  int rows, Ho, Wo, out_pitch;   // rows = B * Ho
  int row_start, pad_;           // first grid row (blockIdx.y) of this member
};
struct CombineGK {
  int n_members, n_in, op, act;
  float slope;
  float coeff[kCombineMaxIn];
  int C;                    // channels of the output view
  int* range_flag;
  CombineGM m[16];
};

// the value of one element from its n inputs; ACC = float, or double for conv mode "f64" (SUM and PROD accumulate in
// binary64 and round once; MAX and COPY select, the activation works on the rounded value)
template <typename ACC>
__device__ __forceinline__ float combine_value(const CombineGK& g, const float (&x)[kCombineMaxIn]) {
  float r;
  if (g.op == COMBINE_SUM) {
    ACC acc = (ACC)0;
#pragma unroll
    for (int i = 0; i < kCombineMaxIn; ++i)
      if (i < g.n_in) acc = acc + (ACC)g.coeff[i] * (ACC)x[i];
    r = (float)acc;
  } else if (g.op == COMBINE_PROD) {
    ACC acc = (ACC)x[0];
#pragma unroll
    for (int i = 1; i < kCombineMaxIn; ++i)
      if (i < g.n_in) acc = acc * (ACC)x[i];
    r = (float)acc;
  } else if (g.op == COMBINE_MAX) {
    r = x[0] > x[1] ? x[0] : x[1];
#pragma unroll
    for (int i = 2; i < kCombineMaxIn; ++i)
      if (i < g.n_in) r = x[i] > r ? x[i] : r;
  } else {
    r = x[0];
  }
  // std::max(x, 0) + slope * std::min(x, 0) with std::max / std::min's operand order (a NaN stays a NaN)
  if (g.act) r = (r < 0.f ? 0.f : r) + g.slope * (0.f < r ? 0.f : r);
  return r;
}

template <bool VEC, typename ACC>
__global__ void __launch_bounds__(256) combine_group_kernel(CombineGK g) {
  int mi = 0;
#pragma unroll
  for (int q = 1; q < 16; ++q) mi += (q < g.n_members && (int)blockIdx.y >= g.m[q].row_start) ? 1 : 0;
  const CombineGM& p = g.m[mi];
  constexpr int V = VEC ? 4 : 1;
  const unsigned CV = (unsigned)g.C / V;
  const unsigned n = blockIdx.x * blockDim.x + threadIdx.x;
  float amax = 0.f;
  if (n < (unsigned)p.Wo * CV) {   // (no early return: every lane takes part in the wave reduction at the end)
    const int cv = (int)(n % CV), ox = (int)(n / CV);
    // the block's rows: every load is issued before the first value is formed (a row at a time, the launch ran at the
    // latency of one request per thread)
    const int r0 = ((int)blockIdx.y - p.row_start) * kCombineRows;
    float x[kCombineRows][V][kCombineMaxIn];
#pragma unroll
    for (int q = 0; q < kCombineRows; ++q) {
      const int r = r0 + q, b = r / p.Ho, oy = r - b * p.Ho;
#pragma unroll
      for (int i = 0; i < kCombineMaxIn; ++i) {
#pragma unroll
        for (int j = 0; j < V; ++j) x[q][j][i] = 0.f;
        if (i < g.n_in && r < p.rows) {
          const CombineIn& s = p.in[i];
          const float* src = s.p + ((size_t)((size_t)b * s.H + oy + s.y0) * s.W + ox + s.x0) * s.pitch + cv * V;
          if constexpr (VEC) {
            const float4 v = *(const float4*)src;
            x[q][0][i] = v.x; x[q][1][i] = v.y; x[q][2][i] = v.z; x[q][3][i] = v.w;
          } else {
            x[q][0][i] = *src;
          }
        }
      }
    }
#pragma unroll
    for (int q = 0; q < kCombineRows; ++q) {
      const int r = r0 + q;
      if (r >= p.rows) break;
      float o[V];
#pragma unroll
      for (int j = 0; j < V; ++j) {
        o[j] = combine_value<ACC>(g, x[q][j]);
        amax = fmaxf(amax, fabsf(o[j]));
        if (o[j] != o[j]) amax = __builtin_inff();   // (fmaxf drops NaNs)
      }
      float* dst = p.out + ((size_t)r * p.Wo + ox) * p.out_pitch + cv * V;
      if constexpr (VEC) *(float4*)dst = make_float4(o[0], o[1], o[2], o[3]);
      else *dst = o[0];
    }
  }
  if (g.range_flag && !(amax <= 65504.0f)) atomicOr(g.range_flag, 1);
  conv_publish_amax(p.out_amax, nullptr, amax);
}

int launch_combine_group(const CombineArgs* as, int n, int f64, int* range_flag, hipStream_t s) {
  if (n < 1 || n > 16) { set_error("combine group: 1..16 members"); return -1; }
  const CombineArgs& a0 = as[0];
  if (a0.n_in < 1 || a0.n_in > kCombineMaxIn || (a0.op != COMBINE_COPY && a0.n_in < 2) || (a0.op == COMBINE_COPY && a0.n_in != 1)) {
    set_error("combine: 2..4 inputs (COPY: one)");
    return -1;
  }
  CombineGK g;
  g.n_members = n; g.n_in = a0.n_in; g.op = a0.op; g.act = a0.act; g.slope = a0.slope;
  for (int i = 0; i < kCombineMaxIn; ++i) g.coeff[i] = i < a0.n_in ? a0.coeff[i] : 0.f;
  g.C = a0.out.C;
  g.range_flag = range_flag;
  bool vec = g.C % 4 == 0;
  long long rows = 0;
  unsigned long long per_row_max = 1;
  for (int m = 0; m < n; ++m) {
    const CombineArgs& a = as[m];
    const View& out = a.out;
    if (a.n_in != g.n_in || a.op != g.op || a.act != g.act || out.C != g.C) { set_error("combine group: members differ in the operation"); return -1; }
    if (!out.p || out.B < 1 || out.H < 1 || out.W < 1 || out.C < 1) { set_error("combine: empty output"); return -1; }
    vec = vec && out.cstride % 4 == 0 && out.coff % 4 == 0 && (((uintptr_t)out.p) & 15) == 0;
    CombineGM& gm = g.m[m];
    for (int i = 0; i < kCombineMaxIn; ++i) {
      CombineIn& gi = gm.in[i];
      gi = CombineIn{nullptr, 1, 1, 1, 0, 0, 0};
      if (i >= g.n_in) continue;
      const View& in = a.in[i];
      // every element read lies inside the source view: the window (y0, x0, c0) + (Ho, Wo, C) fits (H, W, C) of the input
      if (!in.p || in.B != out.B || a.y0[i] < 0 || a.x0[i] < 0 || a.c0[i] < 0 || (long long)a.y0[i] + out.H > in.H ||
          (long long)a.x0[i] + out.W > in.W || (long long)a.c0[i] + out.C > in.C || in.coff + in.C > in.cstride) {
        set_error("combine: input " + std::to_string(i) + " window is out of the source's bounds");
        return -1;
      }
      vec = vec && in.cstride % 4 == 0 && (in.coff + a.c0[i]) % 4 == 0 && (((uintptr_t)in.p) & 15) == 0;
      gi.p = in.p + in.coff + a.c0[i];
      gi.H = in.H; gi.W = in.W; gi.pitch = in.cstride; gi.y0 = a.y0[i]; gi.x0 = a.x0[i];
    }
    if (out.coff + out.C > out.cstride) { set_error("combine: output view exceeds its buffer's pixel"); return -1; }
    gm.out = out.p + out.coff;
    gm.out_amax = a.out_amax;
    gm.rows = out.B * out.H; gm.Ho = out.H; gm.Wo = out.W; gm.out_pitch = out.cstride;
    gm.row_start = (int)rows;
    gm.pad_ = 0;
    rows += ((long long)gm.rows + kCombineRows - 1) / kCombineRows;
    per_row_max = std::max(per_row_max, (unsigned long long)out.W * (unsigned long long)out.C);
  }
  for (int m = n; m < 16; ++m) g.m[m] = g.m[0];
  const unsigned long long per_row = vec ? per_row_max / 4 : per_row_max;
  if (rows > 65535 || per_row >= (1ull << 31)) { set_error("combine: map too large"); return -1; }
  const dim3 grid((unsigned)((per_row + 255) / 256), (unsigned)rows, 1), block(256);
  if (f64) {
    if (vec) hipLaunchKernelGGL((combine_group_kernel<true, double>), grid, block, 0, s, g);
    else hipLaunchKernelGGL((combine_group_kernel<false, double>), grid, block, 0, s, g);
  } else {
    if (vec) hipLaunchKernelGGL((combine_group_kernel<true, float>), grid, block, 0, s, g);
    else hipLaunchKernelGGL((combine_group_kernel<false, float>), grid, block, 0, s, g);
  }
  SHF_HIP_OK(hipGetLastError());
  return 0;
}

}  // namespace shf

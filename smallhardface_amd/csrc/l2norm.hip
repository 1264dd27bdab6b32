// The channel-L2-norm kernel: Caffe's Normalize layer with across_spatial: false on NHWC fp32 activations as ONE launch
//
//     S = sum_c in[c]^2,   norm = sqrt(S + eps),   out[c] = (in[c] / norm) * scale[c]          per pixel (n, y, x)
//
// Reference counterpart: caffe/src/caffe/layers/normalize_layer.cpp:85-134 (Forward_cpu, the !across_spatial branch: the
// squares' sum over channels through a GEMV, pow 0.5, a division by the norm, the product with the scale).  One difference
// in the operation order: Caffe starts the sum from eps (norm_data is set to eps before the GEMV adds into it), here eps
// is added LAST, with one rounding, to the finished sum.  For eps far below the sum (the default 1e-10 against
// activations of order 1) both give the same fp32 value almost always; the worst case is one more rounding of the sum,
// inside the (C / 2 + 4) * 2^-24 relative bound the tests hold the kernel to.
// Built with -ffp-contract=off: the only fused operations are the fmaf calls written below.  sqrtf and the fp32
// division are the compiler's correctly rounded ones (HIP's default: no -fno-hip-fp32-correctly-rounded-divide-sqrt, no
// fast-math), so every step rounds once: + eps, sqrt, /, *.
//
// Data path.  A pixel's C channels are contiguous; the layer is bandwidth bound (8 bytes per element against 3 flops)
// and needs neither matrix cores nor LDS.  A pixel is owned by a group of LPP consecutive lanes of one wave (LPP a power
// of two <= 64, chosen on the host from C alone).  Lane l of the group takes the channel quads l, l + LPP, ... as float4,
// so consecutive lanes read consecutive 16-byte quads; NPL (1, 2, 4, 8 or 16, a template parameter) bounds the quads per
// lane.  All of a lane's loads -- its quads and the scale's -- are issued before the first square, and the values stay
// in registers between the reduction and the scaling: the input is read from memory ONCE for C <= 4096 (64 lanes x 16
// quads).  Wider pixels take the re-reading form (NPL == 0): a loop that sums, and a second one that loads again and
// scales.  The scalar form (VEC == false) takes one channel per lane slot, for channel counts, pitches, offsets or
// pointers that are no multiple of 4 floats / 16 bytes; it holds 64 x 16 = 1024 channels and re-reads beyond.  Input and
// output carry their own pixel pitch and channel offset: a channel window of a zero-copy Concat works on either side,
// and the output may be the input's memory (a lane reads each of its elements before it writes it -- in the re-reading
// form for the second time -- and no other lane touches them).
//
// Reduction.  Per lane s = fmaf(x, x, s) over its quads in ascending channel order, then an xor-butterfly over the
// group's LPP lanes with wave shuffles, masks 1, 2, 4, ...: both lanes of a pair add the same two values (a + b == b + a
// bit for bit), so every lane of the group ends with the same bits.  The order depends on C and the form (VEC, NPL, LPP:
// all functions of C and the alignment) alone, never on the pixel's position, the map size, the member or the grid: a
// grouped forward equals the single forwards bit for bit.  Lanes of a ragged last pixel group, lanes past their pixel's
// quads and lanes past the map hold zeros and take part in every shuffle (no early return).  No atomics on activations.
//
// Conv mode "f64": squares, sum, + eps, sqrt, division and product in binary64 from the fp32 values (eps: the fp32
// value the fp32 form uses), rounded once.  At the end: max |out| of the wave (NaN counts as inf) raises the range flag
// beyond 65504 in the fp16 modes and is published into the top's activation-exponent slot (conv_common.h).  One launch
// covers up to 16 members of different map sizes, stacked along the grid; the geometry comes in a by-value struct.
#include <algorithm>
#include <type_traits>

#include "conv_common.h"
#include "shf_internal.h"

namespace shf {

constexpr int kL2Threads = 256;
constexpr int kL2MaxNpl = 16;   // items (quads, or channels in the scalar form) a lane holds in registers at most

struct L2NormGM {
  const float* in;               // first channel the view reads, of pixel 0
  float* out;
  unsigned* out_amax;
  unsigned pixels;               // B * H * W
  unsigned block_start;          // first block (blockIdx.x) of this member
  int in_pitch, out_pitch;
};
struct L2NormGK {
  int n_members, C;
  int lpp, lpp_log2;             // lanes per pixel
  float eps;
  int pad_;
  const float* scale;            // C values (a channel_shared scale is broadcast on commit)
  int* range_flag;
  L2NormGM mem[16];
};
static_assert(sizeof(L2NormGK) <= 4096, "kernel arguments must fit the 4 KiB by-value limit");

template <bool VEC>
__device__ __forceinline__ void l2_load(const float* p, float (&o)[VEC ? 4 : 1]) {
  if constexpr (VEC) {
    const float4 v = *(const float4*)p;
    o[0] = v.x; o[1] = v.y; o[2] = v.z; o[3] = v.w;
  } else {
    o[0] = *p;
  }
}

// one output element, and its part in the lane's max |out|
template <bool F64>
__device__ __forceinline__ float l2_scale(float x, float sc, float nrm, double nrm64, float& amax) {
  float v;
  if constexpr (F64) v = (float)(((double)x / nrm64) * (double)sc);
  else v = (x / nrm) * sc;
  amax = fmaxf(amax, fabsf(v));
  if (v != v) amax = __builtin_inff();   // (fmaxf drops NaNs)
  return v;
}

template <bool VEC, bool F64, int NPL>
__global__ void __launch_bounds__(kL2Threads) channel_l2norm(L2NormGK g) {
  int mi = 0;
#pragma unroll
  for (int q = 1; q < 16; ++q) mi += (q < g.n_members && blockIdx.x >= g.mem[q].block_start) ? 1 : 0;
  const L2NormGM& p = g.mem[mi];
  constexpr int V = VEC ? 4 : 1;
  typedef typename std::conditional<F64, double, float>::type Acc;
  const int items = g.C / V;   // quads (or channels) per pixel
  const int l = (int)threadIdx.x & (g.lpp - 1);
  const unsigned pix = (blockIdx.x - p.block_start) * (unsigned)(kL2Threads >> g.lpp_log2) + (threadIdx.x >> g.lpp_log2);
  const bool live = pix < p.pixels;   // (no early return: every lane takes part in the shuffles and the wave reduction)
  const float* const src = p.in + (size_t)pix * p.in_pitch;
  float* const dst = p.out + (size_t)pix * p.out_pitch;
  float amax = 0.f;
  Acc s = 0;
  if constexpr (NPL > 0) {
    // every load is issued before the first square: the lane's quads, then their scales
    float x[NPL][V], sc[NPL][V];
#pragma unroll
    for (int j = 0; j < NPL; ++j) {
#pragma unroll
      for (int e = 0; e < V; ++e) x[j][e] = 0.f;
      const int it = l + j * g.lpp;
      if (live && it < items) l2_load<VEC>(src + it * V, x[j]);
    }
#pragma unroll
    for (int j = 0; j < NPL; ++j) {
#pragma unroll
      for (int e = 0; e < V; ++e) sc[j][e] = 0.f;
      const int it = l + j * g.lpp;
      if (live && it < items) l2_load<VEC>(g.scale + it * V, sc[j]);
    }
#pragma unroll
    for (int j = 0; j < NPL; ++j)
#pragma unroll
      for (int e = 0; e < V; ++e) {
        if constexpr (F64) s = fma((double)x[j][e], (double)x[j][e], s);
        else s = fmaf(x[j][e], x[j][e], s);
      }
    for (int m = 1; m < g.lpp; m <<= 1) s += __shfl_xor(s, m);
    float nrm = 0.f;
    double nrm64 = 0.0;
    if constexpr (F64) {
      nrm64 = sqrt(s + (double)g.eps);
    } else {
      const float se = s + g.eps;
      nrm = sqrtf(se);
    }
#pragma unroll
    for (int j = 0; j < NPL; ++j) {
      const int it = l + j * g.lpp;
      if (live && it < items) {
        float o[V];
#pragma unroll
        for (int e = 0; e < V; ++e) o[e] = l2_scale<F64>(x[j][e], sc[j][e], nrm, nrm64, amax);
        if constexpr (VEC) *(float4*)(dst + it * V) = make_float4(o[0], o[1], o[2], o[3]);
        else dst[it] = o[0];
      }
    }
  } else {
    // the re-reading form: the same per-lane order over as many items as the pixel has
    if (live)
      for (int it = l; it < items; it += g.lpp) {
        float x[V];
        l2_load<VEC>(src + it * V, x);
#pragma unroll
        for (int e = 0; e < V; ++e) {
          if constexpr (F64) s = fma((double)x[e], (double)x[e], s);
          else s = fmaf(x[e], x[e], s);
        }
      }
    for (int m = 1; m < g.lpp; m <<= 1) s += __shfl_xor(s, m);
    float nrm = 0.f;
    double nrm64 = 0.0;
    if constexpr (F64) {
      nrm64 = sqrt(s + (double)g.eps);
    } else {
      const float se = s + g.eps;
      nrm = sqrtf(se);
    }
    if (live)
      for (int it = l; it < items; it += g.lpp) {
        float x[V], sc[V], o[V];
        l2_load<VEC>(src + it * V, x);
        l2_load<VEC>(g.scale + it * V, sc);
#pragma unroll
        for (int e = 0; e < V; ++e) o[e] = l2_scale<F64>(x[e], sc[e], nrm, nrm64, amax);
        if constexpr (VEC) *(float4*)(dst + it * V) = make_float4(o[0], o[1], o[2], o[3]);
        else dst[it] = o[0];
      }
  }
  if (g.range_flag && !(amax <= 65504.0f)) atomicOr(g.range_flag, 1);
  conv_publish_amax(p.out_amax, nullptr, amax);
}

// lanes per pixel and items per lane for `items` quads (or channels): a function of the count alone.  Four items per lane
// where the pixel is wide enough (64 bytes in flight per lane in the vector form), but runs of at least 8 lanes; beyond
// 64 lanes x 4 the lanes take 8, then 16 items, then the re-reading form (npl 0)
static void l2norm_form(int items, int* lpp, int* npl) {
  auto pow2ceil = [](int v) { int r = 1; while (r < v) r <<= 1; return r; };
  int lanes = std::max(pow2ceil((items + 3) / 4), std::min(pow2ceil(items), 8));
  lanes = std::min(lanes, 64);
  const int need = (items + lanes - 1) / lanes;
  *lpp = lanes;
  *npl = need > kL2MaxNpl ? 0 : pow2ceil(need);
}

template <bool VEC, bool F64>
static void l2_launch(int npl, dim3 grid, hipStream_t s, const L2NormGK& g) {
  const dim3 block(kL2Threads);
  switch (npl) {
    case 1: hipLaunchKernelGGL((channel_l2norm<VEC, F64, 1>), grid, block, 0, s, g); break;
    case 2: hipLaunchKernelGGL((channel_l2norm<VEC, F64, 2>), grid, block, 0, s, g); break;
    case 4: hipLaunchKernelGGL((channel_l2norm<VEC, F64, 4>), grid, block, 0, s, g); break;
    case 8: hipLaunchKernelGGL((channel_l2norm<VEC, F64, 8>), grid, block, 0, s, g); break;
    case 16: hipLaunchKernelGGL((channel_l2norm<VEC, F64, 16>), grid, block, 0, s, g); break;
    default: hipLaunchKernelGGL((channel_l2norm<VEC, F64, 0>), grid, block, 0, s, g); break;
  }
}

int launch_channel_l2norm_group(const NormArgs* as, int n, const float* scale, float eps, int f64, int* range_flag, hipStream_t s) {
  if (n < 1 || n > 16) { set_error("channel l2norm group: 1..16 members"); return -1; }
  if (!scale) { set_error("channel l2norm: the scale vector is missing (parameters not committed)"); return -1; }
  if (!(eps >= 0.f) || !(eps < __builtin_inff())) { set_error("channel l2norm: eps must be finite and non-negative"); return -1; }
  auto aligned = [](const void* q) { return (((uintptr_t)q) & 15) == 0; };
  L2NormGK g;
  g.n_members = n; g.C = as[0].out.C;
  g.eps = eps; g.pad_ = 0;
  g.scale = scale;
  g.range_flag = range_flag;
  bool vec = g.C % 4 == 0 && aligned(scale);
  for (int m = 0; m < n; ++m) {
    const View &in = as[m].in, &out = as[m].out;
    if (!out.p || !in.p || out.B < 1 || out.H < 1 || out.W < 1 || out.C < 1) { set_error("channel l2norm: empty view"); return -1; }
    if (out.C != g.C) { set_error("channel l2norm group: members differ in the channel count"); return -1; }
    if (in.B != out.B || in.H != out.H || in.W != out.W || in.C != out.C) { set_error("channel l2norm: input and output differ in shape"); return -1; }
    // every element read or written lies inside its buffer's pixel
    if (in.coff < 0 || out.coff < 0 || in.coff + in.C > in.cstride || out.coff + out.C > out.cstride) {
      set_error("channel l2norm: a view exceeds its buffer's pixel");
      return -1;
    }
    vec = vec && in.cstride % 4 == 0 && in.coff % 4 == 0 && aligned(in.p) && out.cstride % 4 == 0 && out.coff % 4 == 0 && aligned(out.p);
  }
  int npl = 0;
  l2norm_form(vec ? g.C / 4 : g.C, &g.lpp, &npl);
  g.lpp_log2 = 0;
  while ((1 << g.lpp_log2) < g.lpp) ++g.lpp_log2;
  const unsigned long long ppb = (unsigned long long)(kL2Threads / g.lpp);   // pixels per block
  unsigned long long blocks = 0;
  for (int m = 0; m < n; ++m) {
    const View &in = as[m].in, &out = as[m].out;
    const unsigned long long pixels = (unsigned long long)out.B * (unsigned long long)out.H * (unsigned long long)out.W;
    if (pixels >= (1ull << 31)) { set_error("channel l2norm: map too large (2^31 pixels or more)"); return -1; }
    L2NormGM& gm = g.mem[m];
    gm.in = in.p + in.coff;
    gm.out = out.p + out.coff;
    gm.out_amax = as[m].out_amax;
    gm.pixels = (unsigned)pixels;
    gm.block_start = (unsigned)blocks;
    gm.in_pitch = in.cstride; gm.out_pitch = out.cstride;
    blocks += (pixels + ppb - 1) / ppb;
    if (blocks >= (1ull << 31)) { set_error("channel l2norm: grid too large (2^31 blocks or more)"); return -1; }
  }
  for (int m = n; m < 16; ++m) g.mem[m] = g.mem[0];
  const dim3 grid((unsigned)blocks, 1, 1);
  if (f64) {
    if (vec) l2_launch<true, true>(npl, grid, s, g);
    else l2_launch<false, true>(npl, grid, s, g);
  } else {
    if (vec) l2_launch<true, false>(npl, grid, s, g);
    else l2_launch<false, false>(npl, grid, s, g);
  }
  SHF_HIP_OK(hipGetLastError());
  return 0;
}

}  // namespace shf

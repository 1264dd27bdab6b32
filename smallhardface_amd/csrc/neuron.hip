// The neuron kernel: Caffe's elementwise activation layers other than ReLU on NHWC fp32 activations as ONE launch form
//
//     out[view] = f(in[view])        f chosen by the template parameter FORM (shf_internal.h: NeuronForm)
//
// Per element these are the reference Caffe's CPU formulas, each fp32 step rounded once in the order written there:
//   PReLU      caffe/src/caffe/layers/prelu_layer.cpp:83-88    max(x, 0) + a[c] * min(x, 0), std::max / std::min's operand
//              order (a NaN stays a NaN); the product is formed for every element (-0 for a positive x and a negative
//              slope), never replaced by a select
//   Sigmoid    sigmoid_layer.cpp:10                            0.5 * tanh(0.5 * x) + 0.5
//   TanH       tanh_layer.cpp:17                               tanh(x)
//   ELU        elu_layer.cpp:16-17                             max(x, 0) + alpha * (exp(min(x, 0)) - 1)
//   AbsVal     absval_layer.cpp:21                             fabs(x)
//   Threshold  threshold_layer.cpp:21                          x > t ? 1 : 0
//   BNLL       bnll_layer.cpp:17-19                            x > 0 ? x + log(1 + exp(-x)) : log(1 + exp(x))
//   Power      power_layer.cpp:20-41                           (shift + scale * x) ^ power: the scale only if != 1, the shift
//              only if != 0, pow only if != 1 (NEURON_POWER_LIN without it, NEURON_POWER_POW with it); power * scale == 0:
//              the constant the host formed (NEURON_CONST, the input is not read)
//   Exp        exp_layer.cpp:30-45                             outer * exp(inner * x); Caffe skips a factor that is 1, and
//              a product with 1 is its other operand bit for bit, so the kernel always multiplies
//   Log        log_layer.cpp:34-54                             base_scale * log(shift + scale * x); factors of 1 as for Exp,
//              the shift only if != 0 (it would turn a -0 into +0; log gives -inf for both, the select keeps the steps
//              Caffe's)
// inner, outer and base_scale come from the host (net_graph.cpp: binary64, rounded once).  Built with -ffp-contract=off, so
// no product is fused into the add behind it; no fast-math and no hardware-approximation intrinsics: expf, logf, tanhf and
// powf are the device library's.  The form is a template parameter: the exact forms (PReLU, AbsVal, Threshold, the linear
// Power, the constant) carry no transcendental code, and no form branches per element.
//
// Conv mode "f64": the same expression with the binary64 functions on the widened input, rounded once at the store.
//
// Data path as the combine and channel-affine kernels' (eltwise.hip, norm.hip): a thread handles one channel quad of one
// pixel as a float4 (consecutive threads = consecutive quads: one dwordx4 request per lane, coalesced) for kNeuronRows rows,
// all loads issued before the first value is formed -- the rows, then PReLU's slope quad, read through the cache as a
// float4 --; the scalar form handles one channel, for channel counts, pitches, offsets or pointers that are no multiple of
// 4 (16 bytes).  Input and output carry their own pixel pitch and channel offset: a channel window of a zero-copy Concat
// works on either side, and the output may be the input's memory (every thread reads its elements before it writes them,
// and no other thread touches them).  One launch covers up to 16 members of different map sizes (the lanes of a grouped
// pass), stacked along the grid's row axis; the geometry comes in a by-value argument struct.  No scratch, no LDS.  At the
// end: max |out| of the wave (NaN counts as inf) raises the range flag beyond 65504 in the fp16 modes and is published into
// the top's activation-exponent slot (conv_common.h) -- the REAL maximum, also where the function has a bound (Sigmoid's 1).
#include <algorithm>

#include "conv_common.h"
#include "shf_internal.h"

namespace shf {

constexpr int kNeuronRows = 4;   // rows (pixel rows of the B * H stack) per block

struct NeuronGM {
  const float* in;               // first channel the view reads, of pixel (0, 0)
  float* out;
  unsigned* out_amax;
  int rows, W, in_pitch, out_pitch;   // rows = B * H
  int row_start, pad_;                // first grid row (blockIdx.y) of this member
};
struct NeuronGK {
  int n_members, C;
  float a, b, c;                 // the form's constants (NeuronSpec)
  int pad_;
  const float* slope;            // PReLU: C values
  int* range_flag;
  NeuronGM mem[16];
};
static_assert(sizeof(NeuronGK) <= 4096, "kernel arguments are passed by value: at most 4 KiB");

// one element.  T = float: every step rounds once in fp32; T = double (conv mode "f64"): the widened input, rounded by the caller
template <int FORM, typename T>
__device__ __forceinline__ T neuron_value(const NeuronGK& g, T x, T slope) {
  const T zero = (T)0, one = (T)1;
  if constexpr (FORM == NEURON_PRELU) {
    return (x < zero ? zero : x) + slope * (zero < x ? zero : x);   // std::max(x, 0) + a * std::min(x, 0)
  } else if constexpr (FORM == NEURON_SIGMOID) {
    if constexpr (sizeof(T) == 8) return 0.5 * tanh(0.5 * x) + 0.5;
    else return 0.5f * tanhf(0.5f * x) + 0.5f;
  } else if constexpr (FORM == NEURON_TANH) {
    if constexpr (sizeof(T) == 8) return tanh(x);
    else return tanhf(x);
  } else if constexpr (FORM == NEURON_ELU) {
    const T m = zero < x ? zero : x;
    T e;
    if constexpr (sizeof(T) == 8) e = exp(m);
    else e = expf(m);
    return (x < zero ? zero : x) + (T)g.a * (e - one);
  } else if constexpr (FORM == NEURON_ABSVAL) {
    if constexpr (sizeof(T) == 8) return fabs(x);
    else return fabsf(x);
  } else if constexpr (FORM == NEURON_THRESHOLD) {
    return x > (T)g.a ? one : zero;
  } else if constexpr (FORM == NEURON_BNLL) {
    const bool pos = x > zero;
    const T t = pos ? -x : x;
    T l;
    if constexpr (sizeof(T) == 8) l = log(1.0 + exp(t));
    else l = logf(1.f + expf(t));
    return pos ? x + l : l;
  } else if constexpr (FORM == NEURON_POWER_LIN || FORM == NEURON_POWER_POW) {
    // a = power, b = scale, c = shift
    T v = x;
    v = g.b != 1.f ? v * (T)g.b : v;
    v = g.c != 0.f ? v + (T)g.c : v;
    if constexpr (FORM == NEURON_POWER_POW) {
      if constexpr (sizeof(T) == 8) v = pow(v, (double)g.a);
      else v = powf(v, g.a);
    }
    return v;
  } else if constexpr (FORM == NEURON_CONST) {
    return (T)g.a;
  } else if constexpr (FORM == NEURON_EXP) {
    // a = inner, b = outer
    const T v = (T)g.a * x;
    if constexpr (sizeof(T) == 8) return (T)g.b * exp(v);
    else return g.b * expf(v);
  } else {
    static_assert(FORM == NEURON_LOG, "unknown neuron form");
    // a = scale, b = shift, c = base_scale
    T v = (T)g.a * x;
    v = g.b != 0.f ? v + (T)g.b : v;
    if constexpr (sizeof(T) == 8) return (T)g.c * log(v);
    else return g.c * logf(v);
  }
}

template <int FORM, bool VEC, bool F64>
__global__ void __launch_bounds__(256) neuron_kernel(NeuronGK g) {
  int mi = 0;
#pragma unroll
  for (int q = 1; q < 16; ++q) mi += (q < g.n_members && (int)blockIdx.y >= g.mem[q].row_start) ? 1 : 0;
  const NeuronGM& p = g.mem[mi];
  constexpr int V = VEC ? 4 : 1;
  const unsigned CV = (unsigned)g.C / V;
  const unsigned n = blockIdx.x * blockDim.x + threadIdx.x;
  float amax = 0.f;
  if (n < (unsigned)p.W * CV) {   // (no early return: every lane takes part in the wave reduction at the end)
    const int cv = (int)(n % CV), ox = (int)(n / CV), c = cv * V;
    const int r0 = ((int)blockIdx.y - p.row_start) * kNeuronRows;
    // every load is issued before the first value is formed: the block's rows, then the channels' slopes
    float x[kNeuronRows][V];
#pragma unroll
    for (int q = 0; q < kNeuronRows; ++q) {
      const int r = r0 + q;
#pragma unroll
      for (int j = 0; j < V; ++j) x[q][j] = 0.f;
      if constexpr (FORM != NEURON_CONST) {
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
    }
    float sl[V];
#pragma unroll
    for (int j = 0; j < V; ++j) sl[j] = 0.f;
    if constexpr (FORM == NEURON_PRELU) {
      if constexpr (VEC) {
        const float4 t = *(const float4*)(g.slope + c);
        sl[0] = t.x; sl[1] = t.y; sl[2] = t.z; sl[3] = t.w;
      } else {
        sl[0] = g.slope[c];
      }
    }
#pragma unroll
    for (int q = 0; q < kNeuronRows; ++q) {
      const int r = r0 + q;
      if (r >= p.rows) break;
      float o[V];
#pragma unroll
      for (int j = 0; j < V; ++j) {
        float v;
        if constexpr (F64) v = (float)neuron_value<FORM, double>(g, (double)x[q][j], (double)sl[j]);
        else v = neuron_value<FORM, float>(g, x[q][j], sl[j]);
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

template <int FORM>
static void neuron_launch(const NeuronGK& g, bool vec, int f64, dim3 grid, dim3 block, hipStream_t s) {
  if (f64) {
    if (vec) hipLaunchKernelGGL((neuron_kernel<FORM, true, true>), grid, block, 0, s, g);
    else hipLaunchKernelGGL((neuron_kernel<FORM, false, true>), grid, block, 0, s, g);
  } else {
    if (vec) hipLaunchKernelGGL((neuron_kernel<FORM, true, false>), grid, block, 0, s, g);
    else hipLaunchKernelGGL((neuron_kernel<FORM, false, false>), grid, block, 0, s, g);
  }
}

int launch_neuron_group(const NormArgs* as, int n, const NeuronSpec& sp, int f64, int* range_flag, hipStream_t s) {
  if (n < 1 || n > 16) { set_error("neuron group: 1..16 members"); return -1; }
  if (sp.form < 0 || sp.form >= NEURON_FORMS) { set_error("neuron: unknown form"); return -1; }
  if (sp.form == NEURON_PRELU && !sp.slope) { set_error("neuron: PReLU's slope vector is missing (parameters not committed)"); return -1; }
  auto aligned = [](const void* q) { return (((uintptr_t)q) & 15) == 0; };
  NeuronGK g;
  g.n_members = n; g.C = as[0].out.C;
  g.a = sp.a; g.b = sp.b; g.c = sp.c; g.pad_ = 0;
  g.slope = sp.slope;
  g.range_flag = range_flag;
  bool vec = g.C % 4 == 0 && (sp.form != NEURON_PRELU || aligned(sp.slope));
  long long rows = 0;
  unsigned long long per_row_max = 1;
  for (int m = 0; m < n; ++m) {
    const View &in = as[m].in, &out = as[m].out;
    if (!out.p || !in.p || out.B < 1 || out.H < 1 || out.W < 1 || out.C < 1) { set_error("neuron: empty view"); return -1; }
    if (out.C != g.C) { set_error("neuron group: members differ in the channel count"); return -1; }
    if (in.B != out.B || in.H != out.H || in.W != out.W || in.C != out.C) { set_error("neuron: input and output differ in shape"); return -1; }
    // every element read or written lies inside its buffer's pixel
    if (in.coff < 0 || out.coff < 0 || in.coff + in.C > in.cstride || out.coff + out.C > out.cstride) {
      set_error("neuron: a view exceeds its buffer's pixel");
      return -1;
    }
    vec = vec && in.cstride % 4 == 0 && in.coff % 4 == 0 && aligned(in.p) && out.cstride % 4 == 0 && out.coff % 4 == 0 && aligned(out.p);
    NeuronGM& gm = g.mem[m];
    gm.in = in.p + in.coff;
    gm.out = out.p + out.coff;
    gm.out_amax = as[m].out_amax;
    gm.rows = out.B * out.H; gm.W = out.W; gm.in_pitch = in.cstride; gm.out_pitch = out.cstride;
    gm.row_start = (int)rows;
    gm.pad_ = 0;
    rows += ((long long)gm.rows + kNeuronRows - 1) / kNeuronRows;
    per_row_max = std::max(per_row_max, (unsigned long long)out.W * (unsigned long long)out.C);
  }
  for (int m = n; m < 16; ++m) g.mem[m] = g.mem[0];
  const unsigned long long per_row = vec ? per_row_max / 4 : per_row_max;
  if (rows > 65535 || per_row >= (1ull << 31)) { set_error("neuron: map too large"); return -1; }
  const dim3 grid((unsigned)((per_row + 255) / 256), (unsigned)rows, 1), block(256);
  switch (sp.form) {
    case NEURON_PRELU: neuron_launch<NEURON_PRELU>(g, vec, f64, grid, block, s); break;
    case NEURON_SIGMOID: neuron_launch<NEURON_SIGMOID>(g, vec, f64, grid, block, s); break;
    case NEURON_TANH: neuron_launch<NEURON_TANH>(g, vec, f64, grid, block, s); break;
    case NEURON_ELU: neuron_launch<NEURON_ELU>(g, vec, f64, grid, block, s); break;
    case NEURON_ABSVAL: neuron_launch<NEURON_ABSVAL>(g, vec, f64, grid, block, s); break;
    case NEURON_THRESHOLD: neuron_launch<NEURON_THRESHOLD>(g, vec, f64, grid, block, s); break;
    case NEURON_BNLL: neuron_launch<NEURON_BNLL>(g, vec, f64, grid, block, s); break;
    case NEURON_POWER_LIN: neuron_launch<NEURON_POWER_LIN>(g, vec, f64, grid, block, s); break;
    case NEURON_POWER_POW: neuron_launch<NEURON_POWER_POW>(g, vec, f64, grid, block, s); break;
    case NEURON_CONST: neuron_launch<NEURON_CONST>(g, vec, f64, grid, block, s); break;
    case NEURON_EXP: neuron_launch<NEURON_EXP>(g, vec, f64, grid, block, s); break;
    default: neuron_launch<NEURON_LOG>(g, vec, f64, grid, block, s); break;
  }
  SHF_HIP_OK(hipGetLastError());
  return 0;
}

}  // namespace shf

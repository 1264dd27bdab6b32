// Internal declarations shared by the HIP kernels and the Net runtime.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string>

namespace shf {

void set_error(const std::string& msg);
#define SHF_HIP_OK(expr)                                                              \
  do {                                                                                \
    hipError_t _e = (expr);                                                           \
    if (_e != hipSuccess) {                                                           \
      ::shf::set_error(std::string(#expr) + ": " + hipGetErrorString(_e));            \
      return -1;                                                                      \
    }                                                                                 \
  } while (0)

// ---- tensor view: NHWC fp32 on the device, possibly a channel slice of a wider buffer
struct View {
  float* p = nullptr;  // base of the buffer
  int B = 1, H = 1, W = 1, C = 1;
  int cstride = 1;  // floats per pixel in the underlying buffer (>= C)
  int coff = 0;     // first channel of this view inside a pixel
};

// ---- profiler classes: the conv classes are named after a kernel instantiation, like rocprofv3 prints them (kProfNames,
//      net_forward.cpp); the reduced arithmetic modes book their instantiations under the headline mode's name
enum ProfClass {
  PC_CONV_MFMA, PC_CONV_MFMA_7 = 7,   // the eight conv_mfma_f32_kernel instantiations (conv.hip)
  PC_CONV_F16X3_128, PC_CONV_F16X3_64, PC_CONV_F16X3_64_FUSE1, PC_CONV_F16X3_64_D2, PC_CONV_F16X3_64_D4, PC_CONV_F16X3_128_K1,
  PC_CONV_F16X3_64_K1, PC_CONV_F16X3_PC,
  PC_CONV_F16X3_W4D_0, PC_CONV_F16X3_W4D_7 = PC_CONV_F16X3_W4D_0 + 7,   // dual-tile family: + in_split * 4 + (rows == 8) * 2 + (tiles == 1)
  PC_CONV_F16X3_PCP, PC_CONV_F16X3_K1G, PC_CONV_F16X3_W4D_D2, PC_CONV_F16X3_W4D_D4, PC_CONV_F16X3_H3,
  PC_CONV_FIRST, PC_CONV_DIRECT, PC_CONV_F64, PC_POOL, PC_DECONV, PC_TAIL, PC_MERGE, PC_LAYOUT, PC_H2D, PC_D2H,
  PC_ELTWISE,   // the combine kernel (eltwise.hip): Eltwise, Crop, free-standing ReLU, a copying Concat
  PC_CONV_GEN,  // the general-geometry convolution (conv_gen.h), its fp32 and its f64 form
  PC_NORM,      // the channel-affine kernel (norm.hip): BatchNorm, Scale and the ReLU behind them, where they are not folded
  PC_CONV_DW,   // the depthwise convolution (conv_dw.hip), its fp32 and its f64 form
  PC_L2NORM,    // the channel-L2-norm kernel (l2norm.hip): Normalize with across_spatial: false
  PC_POOLGEN,   // the pooling kernel (pool.hip): AVE, global, rectangular and any-channel-count Pooling (PC_POOL: maxpool_kernel)
  PC_NEURON,    // the neuron kernel (neuron.hip): PReLU, Sigmoid, TanH, ELU, AbsVal, Threshold, BNLL, Power, Exp, Log
  PC_COUNT
};

// ---- convolution (stride 1, "same" geometry: pad == dil*(k-1)/2) ------------
struct ConvArgs {
  View in, out;
  const float* wpacked = nullptr;  // [Cin/32][k*k][Cout][32] (see pack_conv_weights)
  const float* wraw = nullptr;     // Caffe layout (Cout,Cin,k,k) for the direct kernels
  const float* wfirst = nullptr;   // first layer: weights transposed to [Cin*k*k][Cout]
  const void* wsplit16 = nullptr;  // split-fp16 pack [Cin/32][tap][Cout][hi32|lo32] (conv_f16x3.hip)
  const void* wsplit16r = nullptr; // fused first pair (conv_f16x3_pc.h): [Cin/32][tap][Cout][8 rotated 16-byte pieces], 128-byte rows
  const void* wsplit16h = nullptr; // dual-tile 4-wave kernel: [Cin/16][tap][Cout][hi16|lo16], lo UNSCALED, weights x 1/wscale_inv
  float wscale_inv = 1.f;          // ... and the power of two the epilogue multiplies back
  const float* wgen = nullptr;     // general-geometry kernel: [ceil(K/32)][Cout][32], K over (ky, kx, cin) (conv_gen.h)
  const float* wdw = nullptr;      // depthwise kernel: tap-major [k*k][Cout] (conv_dw.hip)
  int dw_mult = 0;                 // depthwise layers: the channel multiplier Cout / Cin (>= 1); 0 = not depthwise
  const float* bias = nullptr;     // [Cout] or null
  int k = 3, dil = 1, pad = 1;
  int stride = 1;                  // != 1 only on the general-geometry kernel
  int relu = 0;
  const float* img = nullptr;  // fused first layer (f16x3 only): raw NCHW image, transposed weights, bias
  const float* w1t = nullptr;
  const void* w1f = nullptr;   // first-layer weights as split-fp16 MFMA B fragments (pack_first_conv_frags)
  const float* b1 = nullptr;
  View pool;           // optional fused MAX 2x2/2 pool output (p == nullptr: none)
  int write_main = 1;  // 0: the un-pooled output has no other reader and is not written
  // split-fp16 activation format (fused path, conv_f16x3.hip): a blob whose only readers are 4-wave split-fp16
  // convs is stored as [pixel][32-channel chunk][hi 32 halfs | lo 32 halfs] -- the same 4 B per element, already
  // split, so the consumer's halo staging is a plain copy
  int in_split = 0, out_split = 0, pool_split = 0;
  int bf16 = 0;   // conv mode "bf16": one bf16 product per fp32 product (nprod = 1), the packs hold bf16 bit patterns, fp32
                  // activations in HBM, no fp16 range guard and no activation exponent (bf16 has fp32's range)
  int nprod = 3;  // split-fp16 kernels: fp16 products formed per fp32 product -- 3 (hi*hi + hi*lo + lo*hi: fp32-class),
                  // 2 (drops a_lo*b_hi: activations effectively fp16) or 1 (hi*hi only: plain fp16 operands)
  int f64 = 0;    // conv mode "f64": binary64 accumulation on the fp64 matrix cores from the raw weights (conv_f64.h); `img`
                  // then marks a first layer (the NCHW image is its input)
  int* range_flag = nullptr;  // split-fp16 kernels raise it when an output leaves the fp16 range (net_forward.cpp: fp32 re-run)
  // activation-exponent slots (conv_common.h ConvMember): max |value| of the input blob as left by its producers, and
  // where this launch raises the max of what it writes (main output / fused pool output); null = not tracked
  const unsigned* in_amax = nullptr;
  unsigned* out_amax = nullptr;
  unsigned* pool_amax = nullptr;
};
// which kernel class a conv will use: 0 = mfma implicit GEMM, 1 = first-layer direct (NCHW in), 2 = generic direct,
// 3 = general geometry (stride != 1, or neither 3x3 pad == dilation nor 1x1 pad 0: conv_gen.h), from either input layout
// 4 = depthwise (group == Cin, Cout = m * Cin: conv_dw.hip), decided by the graph from the layer's group, never by
// conv_kernel_class
constexpr int kConvClassGeneral = 3;
constexpr int kConvClassDepthwise = 4;
int conv_kernel_class(int Cin, int Cout, int k, int pad, int dil, bool in_nchw, int stride = 1);
// the general-geometry kernel: ONE launch over n <= 16 members that share the layer.  `img` set: the layer reads the NCHW
// net input itself; f64: binary64 accumulation, one rounding.  Its weight pack (made on commit for its layers only):
int launch_conv_gen(const ConvArgs* as, int n, hipStream_t s);
size_t gen_conv_weight_floats(int Cout, int Cin, int k);
void pack_conv_weights_gen(const float* w, int Cout, int Cin, int k, float* dst);
// the depthwise kernel: ONE launch over n <= 16 members that share the layer; any square kernel, stride, pad, dilation and
// channel multiplier; f64: binary64 accumulation, one rounding.  Its weight pack (made on commit for its layers only):
// (Cout, 1, k, k) -> [k*k][Cout]
int launch_conv_dw(const ConvArgs* as, int n, hipStream_t s);
void pack_conv_weights_dw(const float* w, int Cout, int k, float* dst);
// first layer: input is the NCHW 'data' blob (B,Cin,H,W), Cin <= 8, Cout % 16 == 0
int launch_conv_first(const float* in_nchw, const ConvArgs& a, hipStream_t s);
int launch_conv_direct(const ConvArgs& a, hipStream_t s);
int conv_init_attributes();
// Environment knobs of the split-fp16 kernels (experiments; the defaults are the measured best), read once
struct ConvKnobs {
  int w4_mode;      // SHF_F16X3_W4: -1 auto (Cin >= 64), 0 never, 1 always -- which layers take the 4-wave dual-tile family
  int w4_mt;        // SHF_F16X3_W4_MT: 0 auto, 2 / 4 force 8- / 16-row tiles
  int w4d_ntile;    // SHF_F16X3_W4D_NTILE: 0 auto (hybrid launches), 1 / 2 force single- / two-tile blocks
  int w4_slim;      // SHF_F16X3_W4_SLIM: 1 (default) = short-K single 8-row tiles take the slim form, three blocks per CU
                    // (conv_mfma_f16x3_w4d_slim_kernel); 0 = the two-per-CU form; bit-identical
  int pc_tab;       // SHF_F16X3_PC_TAB: 0 = the persistent first pair decodes its tiles one by one (the path launches with more
                    // than 300 tiles per block take anyway); bit-identical
  int heads3;       // SHF_F16X3_HEADS3: 1 (default) = the three shared-weight dilated heads as ONE launch (conv_f16x3_h3.h),
                    // 0 = one launch per head; bit-identical
  bool pc;          // SHF_F16X3_PC (default on): the fused first pair on the producer / consumer kernel
  bool pc_persist;  // SHF_F16X3_PC_PERSIST (default on): the fused first pair as one block per CU walking the tiles
  bool split_act;   // SHF_F16X3_SPLIT_ACT (default on): blobs read only by the dual-tile family are stored split (net_graph.cpp)
  int cus;          // the CU count the PLANNER cuts work by (16- or 8-row tiles, the dual-tile cover, the persistent first pair's
                    // grid): the device's (256 where it cannot be read or is under 4), or SHF_CONV_CUS where that is >= 1 -- a
                    // partition's count, or a small one under which the tests' maps reach every branch.  It changes how a layer
                    // is cut into launches, never a result; nothing but plan_conv_f16x3 reads it (calib.hip asks the device)
};
const ConvKnobs& conv_knobs();
bool conv_f16x3_eligible(int Cin, int Cout, int k, int pad, int dil);
// the shape-only half of plan_conv's choice in the split-fp16 modes: a layer of this shape runs on the dual-tile family
// (3x3: its DIL 1 / 2 / 4 forms; 1x1: the GEMM kernel), which takes the family's weight pack and reads the split activation
// format.  `pool`: a pool is fused into the layer; `aligned`: its output views are 16-byte aligned.  What the launch adds:
// an input under 4 GiB, no fused first layer, a 1x1 not in bf16 mode.
bool conv_f16x3_family_shape(int Cin, int Cout, int k, int pad, int dil, bool pool, bool aligned);
size_t split16_conv_weight_halfs(int Cout, int Cin, int k);
size_t split16h_conv_weight_halfs(int Cout, int Cin, int k);
size_t split16r_conv_weight_halfs(int Cout, int Cin, int k);
void pack_conv_weights_split16r(const float* w, int Cout, int Cin, int k, void* dst, bool bf = false);
float pack_conv_weights_split16h(const float* w, int Cout, int Cin, int k, void* dst, bool bf = false);  // returns 1 / scale
void pack_conv_weights_split16(const float* w, int Cout, int Cin, int k, void* dst, bool bf = false);
// first layer (64, 27) as the B operand of v_mfma_f32_32x32x16_f16: [n 2][kk 2][hi/lo 2][lane 64][8 halfs], K padded 27 -> 32
constexpr size_t kFirstConvFragHalfs = 2 * 2 * 2 * 64 * 8;
void pack_first_conv_frags(const float* w, void* dst, bool bf = false);
// host-side weight re-pack for the mfma kernel
void pack_conv_weights(const float* w, int Cout, int Cin, int k, float* dst);
size_t packed_conv_weight_floats(int Cout, int Cin, int k);

// ---- misc layers -------------------------------------------------------------
int launch_maxpool(const View& in, const View& out, int k, int stride, int pad, hipStream_t s);
int launch_amax_raise(unsigned* dst, const unsigned* src, hipStream_t s);
// depthwise transposed conv (group == C), weights (C,1,k,k) Caffe layout
int launch_deconv_depthwise(const View& in, const View& out, const float* w, const float* bias, int k,
                            int stride, int pad, hipStream_t s, int* range_flag = nullptr, unsigned* out_amax = nullptr);
// conv mode "f64": the same sum in binary64, rounded once to fp32 (any batch; one thread per output value)
int launch_deconv_depthwise_f64(const View& in, const View& out, const float* w, const float* bias, int k, int stride,
                                int pad, hipStream_t s);
int launch_deconv_depthwise_group(const View* ins, const View* outs, int n, const float* w, const float* bias, int k,
                                  int stride, int pad, hipStream_t s, int* range_flag = nullptr,
                                  unsigned* const* out_amax = nullptr);
int launch_copy_view(const View& in, const View& out, hipStream_t s);       // concat fallback
// the combine kernel (eltwise.hip): out = act(op over i < n_in of coeff[i] * in[i] shifted by (y0[i], x0[i], c0[i])).  Eltwise:
// n_in 2 .. 4; Crop: COPY of one input from an offset; free-standing ReLU: COPY with the activation (out may BE in[0]'s
// memory when no offset is set).  Input i's window (origin + the output's H, W, C) must lie inside in[i].
constexpr int kCombineMaxIn = 4;
enum CombineOp { COMBINE_SUM, COMBINE_PROD, COMBINE_MAX, COMBINE_COPY };
struct CombineArgs {
  int n_in = 1, op = COMBINE_COPY;
  int act = 0;              // 1: max(x, 0) + slope * min(x, 0) on the result
  float slope = 0.f;
  float coeff[kCombineMaxIn] = {1.f, 1.f, 1.f, 1.f};   // SUM only
  View in[kCombineMaxIn];
  int y0[kCombineMaxIn] = {0, 0, 0, 0}, x0[kCombineMaxIn] = {0, 0, 0, 0}, c0[kCombineMaxIn] = {0, 0, 0, 0};
  View out;
  unsigned* out_amax = nullptr;   // the output blob's activation-exponent slot (fp16 modes) or null
};
// ONE launch over n <= 16 members that share the operation and the channel count (the lanes of a grouped pass); f64: SUM
// and PROD accumulate in binary64 and round once; range_flag (fp16 modes): raised when an output leaves the fp16 range
int launch_combine_group(const CombineArgs* as, int n, int f64, int* range_flag, hipStream_t s);
// the channel-affine kernel (norm.hip): out = act(((in - m[c]) / d[c]) * g[c] + b[c]), every stage optional and rounded as the
// layer it stands for (BatchNorm: one subtraction, one division; Scale: a product, then an add; ReLU as the combine kernel's).
// The per-channel vectors live on the device, C values each, as the host derived them at commit time.
struct NormStages {
  int norm = 0, scale = 0, bias = 0, act = 0;   // BatchNorm; Scale's product; Scale's bias_term; ReLU
  float slope = 0.f;
  const float *m = nullptr, *d = nullptr, *g = nullptr, *b = nullptr;
  const double *m64 = nullptr, *d64 = nullptr;  // conv mode "f64": mean and denominator formed in binary64
};
struct NormArgs {
  View in, out;                   // the same B, H, W, C; each its own pixel pitch and channel offset; out may BE in
  unsigned* out_amax = nullptr;   // the output blob's activation-exponent slot (fp16 modes) or null
};
// ONE launch over n <= 16 members that share the stages and the channel count (the lanes of a grouped pass); f64: the
// expression in binary64, rounded once, the activation on the rounded value; range_flag as launch_combine_group's
int launch_channel_affine_group(const NormArgs* as, int n, const NormStages& st, int f64, int* range_flag, hipStream_t s);
// the channel-L2-norm kernel (l2norm.hip): out[c] = (in[c] / sqrt(sum_c in[c]^2 + eps)) * scale[c] per pixel, `scale` C values
// on the device.  ONE launch over n <= 16 members that share the layer (the lanes of a grouped pass); f64: the expression in
// binary64, rounded once; range_flag as launch_combine_group's
int launch_channel_l2norm_group(const NormArgs* as, int n, const float* scale, float eps, int f64, int* range_flag, hipStream_t s);
// the neuron kernel (neuron.hip): out = f(in) per element, f one of Caffe's activation layers other than ReLU.  A form is one
// instantiation of the kernel; Power is three of them (without pow, with it, and the constant of power * scale == 0).
enum NeuronForm {
  NEURON_PRELU,       // max(x, 0) + slope[c] * min(x, 0)
  NEURON_SIGMOID,     // 0.5 * tanh(0.5 * x) + 0.5
  NEURON_TANH,        // tanh(x)
  NEURON_ELU,         // max(x, 0) + a * (exp(min(x, 0)) - 1)                  a = alpha
  NEURON_ABSVAL,      // fabs(x)
  NEURON_THRESHOLD,   // x > a ? 1 : 0                                         a = threshold
  NEURON_BNLL,        // x > 0 ? x + log(1 + exp(-x)) : log(1 + exp(x))
  NEURON_POWER_LIN,   // shift + scale * x (each step only if it changes x)     b = scale, c = shift
  NEURON_POWER_POW,   // pow(shift + scale * x, power)                         a = power, b = scale, c = shift
  NEURON_CONST,       // a (the input is not read)
  NEURON_EXP,         // b * exp(a * x)                                        a = inner scale, b = outer scale
  NEURON_LOG,         // c * log(b + a * x)                                    a = scale, b = shift, c = 1 / log(base)
  NEURON_FORMS
};
struct NeuronSpec {
  int form = NEURON_ABSVAL;
  float a = 0.f, b = 0.f, c = 0.f;
  const float* slope = nullptr;   // NEURON_PRELU: C values on the device
};
// ONE launch over n <= 16 members that share the layer (the lanes of a grouped pass); f64: the expression with the binary64
// functions on the widened input, rounded once; range_flag as launch_combine_group's
int launch_neuron_group(const NormArgs* as, int n, const NeuronSpec& sp, int f64, int* range_flag, hipStream_t s);
// the pooling kernel (pool.hip): Caffe's MAX / AVE windows (pooling_layer.cpp:144-215) of any rectangular geometry, or the
// whole map (`global`: the kernel is each member's own H x W, pad 0, stride 1, the output (B, C, 1, 1)).  It raises each
// member's out_amax from its in_amax itself (every output is bounded by max |input|).  ONE launch over n <= 16 members that
// share the layer (the lanes of a grouped pass); f64: the AVE sum and division in binary64, rounded once.
enum PoolMethod { POOL_MAX, POOL_AVE };
struct PoolGeom {
  int method = POOL_MAX;
  int kh = 2, kw = 2, sh = 1, sw = 1, ph = 0, pw = 0;
  int global = 0;
};
struct PoolArgs {
  View in, out;
  const unsigned* in_amax = nullptr;   // the blobs' activation-exponent slots (fp16 modes) or null
  unsigned* out_amax = nullptr;
};
int launch_pool_group(const PoolArgs* as, int n, const PoolGeom& q, int f64, hipStream_t s);
int pool_global_threshold();   // pixels up to which a global layer runs the windowed form (above: the tree form)
int launch_nhwc_to_nchw(const View& in, float* out_nchw, hipStream_t s);    // blob.data read-back
int launch_nchw_to_nhwc(const float* in_nchw, const View& out, hipStream_t s);
// pyramid unit from the raw BGR uint8 image (pre.hip)
int launch_pyramid_level(const uint8_t* im, int im_h, int im_w, double scale, int flip, const double* means,
                         float* out, int H, int W, int lvl_h, int lvl_w, hipStream_t s);

// ---- detection tail ------------------------------------------------------------
constexpr int kTailMaxClasses = 8;   // class counts the tail kernels are instantiated for: 2 .. 8 (background + 1 .. 7)
constexpr int kTailMaxModules = 4;   // proposal layers ("modules": one per backbone stride of an SSH-style net) per launch
struct TailArgs {
  // per-anchor-set (dilation head) features and 1x1 weights
  int A = 3;                 // anchors per cell (== number of heads, or 1 head with A outputs)
  int C = 2;                 // classes, background first (proposal_layer.py:118)
  int heads = 3;             // number of distinct feature maps (3: one per dilation; 1: plain template)
  View feat[8];              // head feature maps (h,w,Cf)
  const float* wcls[8];      // heads==A: (C,Cf) per head ; heads==1: (C*A,Cf)
  const float* bcls[8];
  const float* wbox[8];      // heads==A: (4,Cf) per head ; heads==1: (4A,Cf)
  const float* bbox[8];
  int h = 0, w = 0, Cf = 128;
  float anchors[8 * 4];      // base anchors (A,4) as float32 (bbox_transform.py:37 casts)
  int feat_stride = 8;
  int sub_stride[8];         // per-anchor subsampling stride ratio (proposal_layer.py:160-169)
  float im_h = 0, im_w = 0, im_scale = 1;  // im_info
  float min_size = 0;        // cfg.TEST.ANCHOR_MIN_SIZE (scaled by im_scale in-kernel)
  float score_thresh = 0.002f;
  int pre_nms_topN = 10000;
  // optional materialised Caffe blobs (NCHW), may be null
  float* cls_prob_reshape_nchw = nullptr;  // (1,C*A,h,w)
  float* bbox_pred_nchw = nullptr;         // (1,4A,h,w)
  int f64 = 0;               // conv mode "f64": the predictors' dot products accumulate in binary64, one rounding to fp32
  int probs_given = 0;       // diagnostics: the logits workspace already holds the class probabilities (launch_tail_inject)
  // which proposal module of its net this entry belongs to (0 .. kTailMaxModules - 1): the entries of one module share A,
  // Cf, the weights, the anchors and the strides -- the launch takes them from the first entry of each module
  int module = 0;
};
struct TailWork {  // device workspace owned by the net, sized for the largest level seen
  float* logits = nullptr;           // [K][A][C + 4]
  float* rec = nullptr;              // [K*A][C + 4] = the C class probabilities, x1,y1,x2,y2
  unsigned long long* keys = nullptr;  // [pow2 >= K*A]
  int* counters = nullptr;           // [8]: 0 = n candidates, 1 = overflow flag, 2 = R, 3 = argmax idx
  size_t cap_anchors = 0, cap_keys = 0;
  // the lane's activation-exponent slots (conv_common.h): the tail's reset kernel runs behind the last convolution of
  // a pass and zeroes them for the next one (ten 6-us fill kernels per image otherwise)
  unsigned* amax = nullptr;
  int n_amax = 0;
};
// runs logits -> decode -> select -> sort; leaves R (device counters[2]) rows in out_boxes (R, 5) / out_probs (R, C)
int launch_tail(const TailArgs& a, TailWork& ws, float* out_boxes5, float* out_probs, hipStream_t s,
                hipEvent_t after_logits = nullptr, int phase = 0);
// diagnostics (shf_debug_proposal): fill the logits workspace from injected (1,C*A,h,w) probabilities and
// (1,4A,h,w) deltas (device pointers, NCHW) and raise the overflow flag; follow with launch_tail(phase 2, probs_given)
int launch_tail_inject(const TailArgs& a, TailWork& ws, const float* scores_nchw, const float* deltas_nchw,
                       hipStream_t s);
// after_logits: recorded once the feature maps are consumed; phase 1 = only up to there, 2 = only the rest

// the same for a GROUP of independent entries (the units of an image's pyramid, times the proposal modules of the net):
// ONE launch per stage.  phase 0: everything; 1: counters reset + logits kernel (after_logits recorded behind it); 2:
// decode -> sort -> gather.  The class count and the f64 flag are uniform; everything else an entry's module decides.
int launch_tail_group(const TailArgs* as, TailWork* const* wss, float* const* out_boxes5, float* const* out_probs,
                      int n, hipStream_t s, hipEvent_t after_logits = nullptr, int phase = 0);

// generic device sort of u64 keys, descending; n_dev points at the element count on the device,
// n_max is a host-known upper bound (sizes the launch sequence)
int launch_sort_desc_u64(unsigned long long* keys, const int* n_dev, size_t n_max, hipStream_t s);
int launch_sort_desc_u64_group(unsigned long long* const* keys, const int* const* n_dev, const size_t* n_max, int n,
                               hipStream_t s);

// append the >thresh detections of a group of finished units to an image list (test.py:52-66,163-167): flip fix,
// unscale, threshold cut.  count[pass & 1] = list length before the pass, count[(pass + 1) & 1] after it; with
// per_member != 0 every unit has its own (reset) list and count[1] receives its length.  Two-class units only: the list
// holds the one foreground class's score (probs2 = (R, 2) rows).
struct AppendUnit {
  const float* boxes5;
  const float* probs2;
  const int* counters;  // the unit's tail counters (TailWork::counters)
  int r_max;            // host-side bound of the unit's rows (sizes the launch)
  float im_w, im_scale;
  int flip;
  float* dets5;
  unsigned long long* keys;
  int* count;
  int cap;
};
int launch_append_dets_group(const AppendUnit* us, int n, int topN, float thresh, int pass, int per_member,
                             hipStream_t s);

// ---- score sort keys -------------------------------------------------------------
// Keys are (order bits of the score) << 32 | (0xFFFFFFFF - index), sorted descending as u64: score descending, then
// index ascending (the oracle's canonical_order).  The raw IEEE bits do not order by value once a score is negative,
// so -0.0 is folded onto +0.0 and then a negative value has all its bits flipped, a non-negative one its sign bit set.
// A key is never 0 (the low word is not 0 below 2^32 - 1 rows), so 0 stays free as a "no key" sentinel.
__device__ __forceinline__ unsigned score_order_bits(float f) {
  unsigned u = __float_as_uint(f);
  if (u == 0x80000000u) u = 0u;
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ unsigned long long score_key(float f, unsigned idx) {
  return ((unsigned long long)score_order_bits(f) << 32) | (unsigned long long)(0xFFFFFFFFu - idx);
}

// ---- box merging ----------------------------------------------------------------
constexpr int kMergeMaxBoxes = 262144;   // the greedy scan's removed bitmap: 4096 64-box words in LDS (merge.hip)
struct MergeWork {
  float* sorted = nullptr;                // [n][5] score-descending
  unsigned long long* mask = nullptr;     // [n][ceil(n/64)]
  int* cluster = nullptr;                 // [n] cluster head of each box (-1: none)
  int* heads = nullptr;                   // [n] kept head indices (sorted order)
  int* counters = nullptr;                // [4]: 0 = number of heads
  double* out = nullptr;                  // [n][5]
  int* out_idx = nullptr;                 // [n]
  size_t cap_n = 0, cap_mask_words = 0;
};
// dets sorted descending on the device -> greedy clustering.
// ge_pred: 1 -> IoU >= thr (bbox_vote), 0 -> IoU > thr (nms)
int launch_iou_mask(const float* sorted5, int n, float thr, int ge_pred, unsigned long long* mask, hipStream_t s);
int launch_greedy_scan(const unsigned long long* mask, int n, int* cluster, int* heads, int* counters, hipStream_t s);
int launch_vote_accumulate(const float* sorted5, const unsigned long long* mask, const int* cluster, int n,
                           const int* heads, const int* counters, double* out5, int* n_out, hipStream_t s);
int launch_gather_sorted(const float* dets5, const unsigned long long* keys, int n, float* sorted5, int* perm,
                         hipStream_t s);
int launch_make_keys(const float* dets5, int n, unsigned long long* keys, hipStream_t s);

}  // namespace shf

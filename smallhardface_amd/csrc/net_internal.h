// Internal declarations of the Net runtime (net_graph.cpp: build / shapes / parameters; net_forward.cpp: the layer walk
// of one lane or a group of lanes (run_pass), Net.forward() and the profiler classes; net_detect.cpp: the fused per-image
// detection pipeline; net_class_lists.cpp: the per-class lists of a multi-class image; net_api.cpp: the rest of the C ABI of
// include/shf_hip.h).  One struct, five translation units (split
// in round 5 out of a 2 400-line net.cpp).
#pragma once
#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdio>
#include <deque>
#include <map>
#include <memory>
#include <mutex>
#include <set>

#include "../../include/shf_hip.h"
#include "class_lists.h"
#include "conv_common.h"
#include "proto_text.h"
#include "shf_internal.h"

namespace shf {

extern thread_local std::string g_err;     // net_api.cpp (shf_last_error)

#define HIP_THROW(expr)                                                                        \
  do {                                                                                         \
    hipError_t _e = (expr);                                                                    \
    if (_e != hipSuccess) throw std::runtime_error(std::string(#expr) + ": " + hipGetErrorString(_e)); \
  } while (0)
#define CHECK_RC(expr)                                     \
  do {                                                     \
    if ((expr) != 0) throw std::runtime_error(g_err);      \
  } while (0)
// ... naming the layer (a launcher's message speaks of shapes and kernels, not of the graph)
#define CHECK_RC_LAYER(expr, lname)                                                           \
  do {                                                                                        \
    if ((expr) != 0) throw std::runtime_error("layer '" + std::string(lname) + "': " + g_err); \
  } while (0)

// hipMemset on the null stream may return before the fill has run, and the null stream is not ordered with the runtime's
// non-blocking streams: a fill that must be in place before the first kernel touches the buffer is waited for here.  (A
// lane cloned inside FusedDetector.submit launches its first convolutions microseconds after its slots are cleared: a
// late fill zeroed slots the first kernels had already published into -- the first image of a process then ran a unit with
// e = 0 and differed from the same image processed later in the last bit.)
inline void fill_now(void* p, int byte, size_t n) {
  HIP_THROW(hipMemsetAsync(p, byte, n, nullptr));
  HIP_THROW(hipStreamSynchronize(nullptr));
}

// SHF_POISON_ALLOC=<byte> (tests/test_gpu_buffer_history.py): fresh device allocations start filled with that byte (0xff:
// NaNs) instead of whatever the allocator hands out -- a kernel whose result depends on memory it never wrote shows up as a
// changed result.  Read once per process; -1 when the knob is unset (shf_debug_poison_byte).
inline int poison_byte() {
  static const int byte = [] {
    const char* s = getenv("SHF_POISON_ALLOC");
    return s ? (int)(strtol(s, nullptr, 0) & 0xff) : -1;
  }();
  return byte;
}
// ... applied to a fresh allocation of n bytes (DevBuf::ensure, and the evaluators' per-call buffers in net_api.cpp)
inline void poison_fresh(void* p, size_t n) {
  if (poison_byte() >= 0) fill_now(p, poison_byte(), n);
}

// (re)allocations made by the grow-only buffers of this process: a new level shape re-plans sizes and pointers and only
// allocates where a buffer has to grow (shf_alloc_counts; bench.py's mixed-shape leg reports them after its first pass)
extern std::atomic<long long> g_dev_allocs, g_host_allocs;   // net_api.cpp

struct DevBuf {
  void* p = nullptr;
  size_t cap = 0;
  void ensure(size_t bytes) {
    if (bytes <= cap) return;
    ++g_dev_allocs;
    if (p) HIP_THROW(hipFree(p));
    p = nullptr;
    size_t want = bytes + bytes / 8;  // grow-only with slack (Blob::Reshape never shrinks, blob.cpp:46-50)
    want = (want + 255) & ~(size_t)255;
    HIP_THROW(hipMalloc(&p, want));
    cap = want;
    poison_fresh(p, want);
  }
  ~DevBuf() {
    if (p) (void)hipFree(p);
  }
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
};

struct HostBuf {
  float* p = nullptr;
  size_t cap = 0;
  void ensure(size_t bytes) {
    if (bytes <= cap) return;
    float* np = nullptr;
    ++g_host_allocs;
    size_t want = std::max<size_t>(bytes + bytes / 8, 64);
    HIP_THROW(hipHostMalloc((void**)&np, want, hipHostMallocDefault));
    if (p) {
      memcpy(np, p, cap);
      (void)hipHostFree(p);
    }
    memset((char*)np + cap, 0, want - cap);
    p = np;
    cap = want;
  }
  ~HostBuf() {
    if (p) (void)hipHostFree(p);
  }
  HostBuf() = default;
  HostBuf(const HostBuf&) = delete;
  HostBuf& operator=(const HostBuf&) = delete;
};

struct ParamBlob {
  std::vector<int> shape;
  std::vector<float> host;
  DevBuf raw, packed, packed16, packed16h, packed16r, first_t, first_frag;   // (packed16r: the fused first pair's rotated-row pack)
  DevBuf packed_gen;   // the general-geometry kernel's pack (conv_gen.h): allocated for layers of that class only
  DevBuf packed_dw;    // the depthwise kernel's tap-major pack (conv_dw.hip): allocated for layers of that class only
  DevBuf packed16b, packed16hb, packed16rb, first_frag_b;   // the same three packs for conv mode "bf16" (built on first use of the mode)
  bool bf_stale = true;                         // ... and whether they hold the current weights
  float wscale_inv = 1.f;  // packed16h: the power of two its weights were scaled by, inverted
  bool dirty = true;
  bool split_stale = false;  // committed while the net was in fp32 mode: packed16 / packed16h hold OLDER weights
  // bumped whenever the host values may have been written (shf_net_param_data, load_caffemodel).  On a folded convolution's
  // effective bias: the versions of the blobs (its own, the BatchNorm's, the Scale's) its last commit folded
  unsigned long long version = 0;
  std::vector<unsigned long long> folded_from;
  size_t count() const {
    size_t c = 1;
    for (int d : shape) c *= (size_t)d;
    return c;
  }
};

enum BlobKind { BK_INPUT_NCHW, BK_NHWC, BK_FLAT, BK_NCHW_MAT, BK_FUSED };

struct Blob {
  std::string name;
  std::vector<int> shape;  // logical Caffe shape
  BlobKind kind = BK_NHWC;
  int owner = -1;  // blob owning the device buffer (channel-concat views)
  int coff = 0;
  DevBuf dev, stage;
  HostBuf host;
  bool host_newer = false, dev_newer = false;
  const float* ext_dev = nullptr;  // externally bound device input (fused path)
  bool split_fused = false;        // fused split-fp16 path: stored pre-split ([chunk][hi|lo] fp16), see ConvArgs::in_split
  // BK_FUSED blobs (tops of the layers folded into the detection tail) are materialised ON DEMAND when Blob.data is read
  // after Net.forward() (shf_net::materialize_fused): what they hold, and for a predictor's top which head it belongs to
  int fused_role = 0;              // FusedRole
  int fused_head = -1;
  int fused_mod = -1;              // ... and which proposal module's tail it was folded into
  size_t count() const {
    size_t c = 1;
    for (int d : shape) c *= (size_t)d;
    return c;
  }
};

// what a tail-fused blob holds (pycaffe exposes every blob after forward(), pycaffe.py:24-32 / _caffe.cpp:222-242)
enum FusedRole {
  FR_NONE = 0,
  FR_CLS_CONV,     // top of a class-score 1x1 conv: (1, C, h, w) per head, or (1, C*A, h, w) channel = cls * A + a (plain template)
  FR_BOX_CONV,     // top of a bbox 1x1 conv: (1, 4, h, w) per head, or (1, 4A, h, w) channel = 4a + j
  FR_CLS_PLANES,   // the pre-softmax (1, C, A*h, w) tensor: axis-2 Concat of the heads' scores, or the plain template's Reshape
  FR_PROB_PLANES   // the Softmax's top, (1, C, A*h, w): the memory of the materialised (1, C*A, h, w) cls_prob blob
};

void check_blob_dims(const std::vector<int>& shp, const std::string& name);   // net_graph.cpp: Blob::Reshape's limits

// OP_ELTWISE / OP_CROP / OP_RELU / OP_CONCAT_COPY: launches of the combine kernel (eltwise.hip).  OP_RELU: a ReLU that is not
// the in-place, slope-0 one behind a Convolution (that one is Layer::relu of the convolution, OP_SKIP); OP_CONCAT_COPY: a
// channel Concat that copies, because a later in-place ReLU rewrites its top (every other channel Concat is a zero-copy view)
// OP_NORM: a BatchNorm or Scale layer that runs the channel-affine kernel (norm.hip), alone or as the head or a member of an
// in-place chain; one that is folded into its producing convolution is OP_SKIP with Layer::norm_conv set
// OP_L2NORM: a Normalize layer (across_spatial: false): one launch of the channel-L2-norm kernel (l2norm.hip), never folded
// OP_POOL: a Pooling layer: maxpool_kernel (misc.hip) for MAX, square, quad-aligned layers, a 2x2/2 one possibly folded into
// its producing convolution on the fused path; the pooling kernel (pool.hip) for everything else
// OP_NEURON: a PReLU, Sigmoid, TanH, ELU, AbsVal, Threshold, BNLL, Power, Exp or Log layer: one launch of the neuron kernel
// (neuron.hip), never folded; in place it is a rewriter like OP_L2NORM
enum OpType { OP_SKIP, OP_CONV, OP_POOL, OP_DECONV, OP_TAIL, OP_ELTWISE, OP_CROP, OP_RELU, OP_CONCAT_COPY, OP_NORM, OP_L2NORM, OP_NEURON };

// what a BatchNorm / Scale layer's launch reads: per-channel vectors derived from its blobs at commit time (derive_norm),
// shared by the lanes of a net like a weight pack
struct NormVecs {
  DevBuf m, d, m64, d64;   // BatchNorm: mean * sf and sqrt(var * sf + eps), in fp32 (Caffe's operation order) and in binary64
  DevBuf g, b;             // Scale: its blobs.  Normalize: g = its scale, C values (a channel_shared one broadcast on commit)
                           // PReLU: g = its slopes, likewise
};

struct Layer {
  std::string name, type;
  const PMsg* msg = nullptr;
  std::vector<int> bottoms, tops;
  std::vector<std::shared_ptr<ParamBlob>> params;
  OpType op = OP_SKIP;
  // conv / deconv / pool hyper-parameters
  int k = 1, pad = 0, stride = 1, dil = 1, group = 1, nout = 0, relu = 0, bias_term = 1;
  int kclass = 0;
  // Pooling (PoolingLayer::LayerSetUp): the method and the window per axis; k / stride / pad above keep the square case's
  // values (a rectangular or global layer: those of the h axis).  global_pool: the window is the bottom's H x W at every reshape
  int pool_method = POOL_MAX;
  int kh = 2, kw = 2, sh = 1, sw = 1, ph = 0, pw = 0;
  bool global_pool = false;
  int fuse_pool = -1;      // conv: index of the 2x2/2 MAX pool folded into its epilogue (fused path only)
  bool pool_only = false;  // conv: its un-pooled top has no other reader
  int fused_into = -1;     // pool: index of the conv that produces it in the fused path
  int first_src = -1;      // conv: index of the first-layer conv computed inside this conv's halo staging (f16x3)
  int first_dst = -1;      // first-layer conv: index of the conv that absorbs it
  // the three shared-weight dilated heads (prototxt :480-552): on the dilation-1 layer, the indices of its dilation-2 / -4
  // siblings (same bottom, same parameter blobs); on those, the index of the dilation-1 layer.  One launch covers the three
  // when the shapes and the mode allow (plan_conv_heads3).
  int heads3_d2 = -1, heads3_d4 = -1, heads3_lead = -1;
  // the combine launches (eltwise.hip)
  int eop = COMBINE_COPY;          // Eltwise: its operation
  std::vector<float> coeff;        // Eltwise SUM: one per bottom (all 1 when the prototxt gives none)
  float slope = 0.f;               // ReLU: negative_slope
  int concat_axis = 1;             // Concat: the canonical axis (concat_param.axis, or its legacy spelling concat_dim)
  int crop_axis = 2;               // Crop: first cropped axis, and the origin per blob axis (set by shape inference)
  std::vector<int> crop_offsets;   //   as the prototxt gives them: none, one, or one per cropped axis
  int crop_origin[4] = {0, 0, 0, 0};
  // folds of the fused path (on the per-layer path every layer runs on its own and every blob holds Caffe's values):
  int fold_relu = -1;              // Eltwise / Crop / copying Concat: index of the in-place ReLU applied in its launch
  int folded_into = -1;            // ReLU: the layer whose launch applies it; Crop: the Eltwise that reads through its offsets
                                   // (a ReLU behind a copying Concat is folded on BOTH paths: the two are one launch per member)
  // BatchNorm / Scale.  Unfolded, consecutive in-place BatchNorm, Scale, ReLU on one blob with no reader in between are ONE
  // launch on both paths: the first is the chain's head, the others carry folded_into = head.  Folded, they are part of the
  // convolution's parameters and run no launch.
  bool is_bn = false;              // BatchNorm (else Scale)
  float eps = 1e-5f;               // BatchNorm: batch_norm_param.eps; Normalize: norm_param.eps (default 1e-10)
  bool l2_shared = false;          // Normalize: channel_shared (the blob has 0 axes and one value)
  float l2_fill = 1.f;             // Normalize: what the blob holds before a model is loaded (a constant scale_filler's value)
  // the neuron layers (neuron.hip): the kernel form and its constants as NeuronSpec names them; Exp's and Log's derived ones
  // (inner, outer, 1 / log(base)) are formed in binary64 at construction and rounded once
  int neuron_form = 0;
  float neuron_a = 0.f, neuron_b = 0.f, neuron_c = 0.f;
  bool prelu_shared = false;       // PReLU: channel_shared (the blob has 0 axes and one value)
  float prelu_fill = 0.25f;        // PReLU: what the blob holds before a model is loaded (a constant filler's value; none: 0.25)
  std::shared_ptr<NormVecs> nv;
  int chain_bn = -1, chain_sc = -1, chain_relu = -1;   // on a chain's head: its stages' layers (the head is one of them)
  int norm_conv = -1;              // BatchNorm / Scale: the convolution it is folded into
  int fold_bn = -1, fold_sc = -1;  // Convolution: the BatchNorm / Scale folded into its parameters
  std::shared_ptr<ParamBlob> fold_bias;   // ... and the effective bias its launches read (params keeps Caffe's unfolded blobs)
};

extern const char* const kProfNames[PC_COUNT];   // net_forward.cpp

struct Prof {
  bool on = false;
  int only = -1;   // >= 0: only launches of this class are bracketed (shf_prof_only)
  bool wants(int cls) const { return on && (only < 0 || only == cls); }
  struct Rec { int cls; hipEvent_t a, b; double flops, bytes; };
  std::vector<Rec> pending;
  std::vector<hipEvent_t> pool;
  int64_t launches[PC_COUNT] = {0};
  double ms[PC_COUNT] = {0}, flops[PC_COUNT] = {0}, bytes[PC_COUNT] = {0};
  hipEvent_t get() {
    if (!pool.empty()) {
      hipEvent_t e = pool.back();
      pool.pop_back();
      return e;
    }
    hipEvent_t e;
    HIP_THROW(hipEventCreate(&e));
    return e;
  }
  void drain() {
    for (auto& r : pending) {
      HIP_THROW(hipEventSynchronize(r.b));
      float t = 0;
      HIP_THROW(hipEventElapsedTime(&t, r.a, r.b));
      launches[r.cls]++;
      ms[r.cls] += t;
      flops[r.cls] += r.flops;
      bytes[r.cls] += r.bytes;
      pool.push_back(r.a);
      pool.push_back(r.b);
    }
    pending.clear();
  }
  ~Prof() {
    for (auto& r : pending) { (void)hipEventDestroy(r.a); (void)hipEventDestroy(r.b); }
    for (auto e : pool) (void)hipEventDestroy(e);
  }
};

struct ProfScope {
  Prof& p;
  hipStream_t s;
  Prof::Rec r;
  bool on;
  ProfScope(Prof& p_, hipStream_t s_, int cls, double flops, double bytes) : p(p_), s(s_), on(p_.wants(cls)) {
    if (!on) return;
    r.cls = cls; r.flops = flops; r.bytes = bytes;
    r.a = p.get(); r.b = p.get();
    HIP_THROW(hipEventRecord(r.a, s));
  }
  ~ProfScope() {
    if (!on) return;
    (void)hipEventRecord(r.b, s);
    p.pending.push_back(r);
  }
};

// a conv's launches, each bracketed by a ProfScope of its kernel's class and its share of the layer's flops / bytes
int run_conv_plan(const ConvPlan& pl, hipStream_t s, Prof& prof, double flops, double bytes);

// ---------------------------------------------------------------------------
// box merging context (also used stand-alone by shf_nms / shf_bbox_vote)
// ---------------------------------------------------------------------------
struct MergeCtx {
  DevBuf dets, keys, sorted, perm, mask, cluster, heads, counters, out;
  std::vector<double> hout;
  std::vector<int> hidx;

  // more boxes than the greedy scan holds: refused before anything is allocated or launched
  static int refuse_size(int n) {
    if (n <= kMergeMaxBoxes) return 0;
    set_error("merge: " + std::to_string(n) + " boxes exceed the limit of " + std::to_string(kMergeMaxBoxes) +
              " (the greedy scan's bitmap)");
    return -1;
  }

  // dets_dev: (n,5) fp32 on the device.  method 0 = vote (>=), 1 = nms (>).
  // vote: rows -> out5 (cap rows) ; nms: kept ORIGINAL indices -> keep
  int run(const float* dets_dev, int n, int method, float thr, double* out5, int cap, int* n_out, int32_t* keep,
          hipStream_t s) {
    *n_out = 0;
    if (n <= 0) return 0;
    CHECK_RC(refuse_size(n));
    size_t npad = 1;
    while (npad < (size_t)n) npad <<= 1;
    const size_t nw = ((size_t)n + 63) / 64;
    keys.ensure(npad * 8);
    sorted.ensure((size_t)n * 5 * 4);
    perm.ensure((size_t)n * 4);
    mask.ensure((size_t)n * nw * 8);
    cluster.ensure((size_t)n * 4);
    heads.ensure((size_t)n * 4);
    counters.ensure(64);
    out.ensure((size_t)n * 5 * 8 * 2 + (size_t)n * 4 + 64);
    int* cnt = (int*)counters.p;
    HIP_THROW(hipMemsetAsync(cnt, 0, 64, s));
    HIP_THROW(hipMemcpyAsync(cnt + 3, &n, sizeof(int), hipMemcpyHostToDevice, s));
    CHECK_RC(launch_make_keys(dets_dev, n, (unsigned long long*)keys.p, s));
    CHECK_RC(launch_sort_desc_u64((unsigned long long*)keys.p, cnt + 3, (size_t)n, s));
    CHECK_RC(launch_gather_sorted(dets_dev, (unsigned long long*)keys.p, n, (float*)sorted.p, (int*)perm.p, s));
    CHECK_RC(launch_iou_mask((float*)sorted.p, n, thr, method == 0 ? 1 : 0, (unsigned long long*)mask.p, s));
    CHECK_RC(launch_greedy_scan((unsigned long long*)mask.p, n, (int*)cluster.p, (int*)heads.p, cnt, s));
    if (method == 0) {
      CHECK_RC(launch_vote_accumulate((float*)sorted.p, (unsigned long long*)mask.p, (int*)cluster.p, n,
                                      (int*)heads.p, cnt, (double*)out.p, cnt + 1, s));
      int h[2];
      HIP_THROW(hipMemcpyAsync(h, cnt, 8, hipMemcpyDeviceToHost, s));
      HIP_THROW(hipStreamSynchronize(s));
      const int m = h[1];
      *n_out = m;
      const int w = std::min(m, cap);
      if (w > 0) HIP_THROW(hipMemcpy(out5, out.p, (size_t)w * 5 * 8, hipMemcpyDeviceToHost));
    } else {
      int nh = 0;
      HIP_THROW(hipMemcpyAsync(&nh, cnt, 4, hipMemcpyDeviceToHost, s));
      HIP_THROW(hipStreamSynchronize(s));
      hidx.resize((size_t)n * 2);
      HIP_THROW(hipMemcpy(hidx.data(), heads.p, (size_t)nh * 4, hipMemcpyDeviceToHost));
      HIP_THROW(hipMemcpy(hidx.data() + n, perm.p, (size_t)n * 4, hipMemcpyDeviceToHost));
      *n_out = nh;
      if (keep)
        for (int i = 0; i < nh; ++i) keep[i] = hidx[n + hidx[i]];
      if (out5) {
        std::vector<float> hs((size_t)n * 5);
        HIP_THROW(hipMemcpy(hs.data(), sorted.p, (size_t)n * 5 * 4, hipMemcpyDeviceToHost));
        for (int i = 0; i < std::min(nh, cap); ++i)
          for (int j = 0; j < 5; ++j) out5[i * 5 + j] = (double)hs[(size_t)hidx[i] * 5 + j];
      }
    }
    return 0;
  }
};

// net_graph.cpp
void gen_anchors(int base_size, const std::vector<double>& ratios, const std::vector<double>& scales,
                 const std::vector<double>& shifts, const std::vector<double>& strides, std::vector<double>& out);
std::map<std::string, std::vector<double>> parse_param_str(const std::string& s);
int conv_out(int n, int k, int pad, int stride, int dil);

}  // namespace shf

namespace shf {
int calib_matrix_pipe(int bf16, int zero_eighths, int constant, int iters, int reps, double* tflops);   // calib.hip
int conv_f16x3_plan_probe(int Cin, int Cout, int H, int W, int in_split, int pooled, long long* lds, long long* grid, int* slim);   // conv_f16x3.hip
int conv_f16x3_plan_probe_group(int n, const int* B, const int* H, const int* W, int Cin, int Cout, int in_split, int pooled, int first_pair,
                                int cus, long long* out, int* pc_tab);   // conv_f16x3.hip
}
using namespace shf;

// One ProposalLayer of the graph with the predictors fused into it: what the tail kernels need to know about it, its
// combined weights, its workspace and its output blobs.  Everything here was one-per-net while a net held one such layer.
constexpr int kMaxModules = kTailMaxModules;   // proposal layers per net (tail.hip TM)
struct TailModule {
  int layer = -1;                                   // the Python layer
  std::vector<int> cls_layers, box_layers;          // per head (or single)
  std::vector<int> feat_blobs;
  int A = 0, heads = 0, Cf = 0;
  int cls_blob = -1, box_blob = -1, boxes_blob = -1, prob_blob = -1;
  std::vector<double> anchors;
  std::vector<int> sub_stride;
  int feat_stride = 8;
  DevBuf W, b;                                      // [A][C + 4][Cf] / [A][C + 4] (build_tail_weights)
  bool w_dirty = true;
  int gen = -1;
  TailWork tw;
  DevBuf tw_logits, tw_rec, tw_keys, tw_counters;
  int last_R = -1;   // proposal rows of the last completed forward (record_forward); -1: none yet
};

// configuration shared by a net and every lane cloned from it: the arithmetic mode and what the reference's Python
// layer reads from the global cfg at every forward (lib/layers/proposal_layer.py:88-92)
struct NetShared {
  int conv_mode = 0;  // 0: exact fp32 MFMA everywhere; 1: split-fp16, 3 products (fp32-class accuracy); 2 / 3: the
                      // reduced ladder -- 2 products (activations rounded to fp16) / 1 product (plain fp16 operands); 4: bf16;
                      // 5: binary64 accumulation, one rounding to fp32 (conv_f64.h: the on-device truth for drift)
  std::map<std::string, int> layer_products;  // per-layer override of the number of fp16 products (shf_net_set_layer_products)
  int pre_nms_topN = 10000;
  float score_thresh = 0.002f, min_size = 0.f;
  bool weights_exceed_f16 = false;  // some conv weight is outside the fp16 range: split-fp16 mode refuses to run
  long long range_fallbacks = 0;    // forwards re-run on the exact fp32 kernels after a split-fp16 range overflow
  // image pipeline (shf_net_set_pipeline): ONE in-order stream carries the convolutions + logits kernels of every
  // image; each head's own (high-priority) stream carries the rest of its image's tails, appends and the merge
  hipStream_t conv_stream = nullptr;
  ~NetShared() {
    if (conv_stream) {
      (void)hipStreamSynchronize(conv_stream);
      (void)hipStreamDestroy(conv_stream);
    }
  }
};

// a shared setting changed for the length of a scope (conv_mode during the fp32 redo, pre_nms_topN in shf_debug_append)
template <typename T>
struct Restore {
  T& ref;
  const T saved;
  explicit Restore(T& r) : ref(r), saved(r) {}
  ~Restore() { ref = saved; }
  Restore(const Restore&) = delete;
  Restore& operator=(const Restore&) = delete;
};

// what a pass of the layer walk does at the proposal layer: the one step its callers differ in
enum TailStep {
  TAIL_NONE,      // nothing (ensure_plain: the intermediates only -- the tail's outputs stay the forward's own)
  TAIL_LANE,      // one phase-0 launch per lane; a fused pass records the lane's ev_logits behind its logits kernel
  TAIL_HANDOVER,  // the grouped pipeline's two phases with their hand-over events (shf_detect_add_levels)
  TAIL_GROUP      // both phases of the group as one launch per stage on the pass's stream, no events (shf_net_forward_group)
};

// a HIP event that lives as long as anyone holds it: a head's ev_convs is also what the lanes of its pass wait for later
// (shf_net::logits_done), and a head may go before the lanes that lent it their buffers
struct SharedEvent {
  hipEvent_t e = nullptr;
  ~SharedEvent() { if (e) (void)hipEventDestroy(e); }
};

struct shf_net {
  std::shared_ptr<NetShared> sh;
  int& conv_mode;
  int& pre_nms_topN;
  float& score_thresh;
  float& min_size;
  explicit shf_net(std::shared_ptr<NetShared> shared = nullptr)
      : sh(shared ? shared : std::make_shared<NetShared>()), conv_mode(sh->conv_mode), pre_nms_topN(sh->pre_nms_topN),
        score_thresh(sh->score_thresh), min_size(sh->min_size) {}
  std::shared_ptr<PMsg> root;
  std::deque<Blob> blobs;
  std::vector<Layer> layers;
  std::map<std::string, int> blob_index;
  std::vector<int> inputs, outputs;
  std::map<std::string, std::shared_ptr<ParamBlob>> shared_params;
  hipStream_t stream = nullptr;
  Prof prof;
  int phase = 1;
  // tail: one record per ProposalLayer of the graph ("module": the SSH-style detector has one per backbone stride, each with
  // its own boxes_<level> / cls_prob_<level> tops, lib/test.py:67-83), in prototxt order.  tail_layer: the LAST proposal
  // layer of the walk, where a pass issues the tails of all its modules as one launch sequence (-1: no tail).  The class
  // count is one number per net (Net.num_classes): modules that disagree are refused at construction.
  std::deque<TailModule> mods;
  int tail_layer = -1;
  int tail_C = 2;   // classes (background first), 2 .. kTailMaxClasses: from the predictors' output counts
  int im_info_blob = -1, data_blob = -1;
  int module_of_output(int bi) const {   // the module whose boxes / cls_prob top blob bi is, or -1
    for (size_t j = 0; j < mods.size(); ++j)
      if (bi == mods[j].boxes_blob || bi == mods[j].prob_blob) return (int)j;
    return -1;
  }
  bool is_feat_blob(int bi) const {
    for (auto& M : mods)
      if (std::count(M.feat_blobs.begin(), M.feat_blobs.end(), bi)) return true;
    return false;
  }
  std::string proto_text;
  shf_net* clone_src = nullptr;     // lanes share the parameter tensors of the net they were cloned from
  std::shared_ptr<int> wgen = std::make_shared<int>(0);  // bumped by every param commit
  hipEvent_t ev_mark = nullptr;
  hipEvent_t ev_logits = nullptr;  // recorded by every fused tail pass right after its logits kernel
  hipEvent_t logits_done = nullptr;  // what a later pass over this member waits for: its own ev_logits, or --
                                     // after a pipelined grouped pass -- the head's ev_convs (ONE record for the group:
                                     // ten event records in a row were ~90 us of idle conv stream per image)
  std::shared_ptr<SharedEvent> logits_keep;   // holds the head's ev_convs while logits_done is that event, else empty
  hipEvent_t ev_convs = nullptr;   // group pass: recorded on the head's stream after the last layer before the tails
  std::shared_ptr<SharedEvent> ev_convs_own;  // ... and its owner, shared with the lanes that wait for it
  hipEvent_t ev_group = nullptr;   // head of shf_blob_load_device_group: recorded behind the copy, awaited by the members' streams
  shf_net* pred = nullptr;         // shf_net_set_predecessor: the head lane whose image precedes this one's
  bool pipelined = false;   // shf_net_set_pipeline: convolutions go to sh->conv_stream, the rest stays on `stream`
  hipStream_t cstream() { return pipelined && sh->conv_stream ? sh->conv_stream : stream; }
  // an fp16 mode (split-fp16, f16x2, f16): its producers guard the fp16 range and it keeps activation-exponent slots (bf16
  // has fp32's exponent range)
  bool fp16_mode() const { return conv_mode >= 1 && conv_mode <= 3; }
  // a 16-bit mode (the fp16 modes and bf16): split weight packs, the fused path's kernels, the range flag's read-back
  bool split_mode() const { return conv_mode >= 1 && conv_mode <= 4; }
  // binary64 accumulation (conv_f64.h): always the per-layer path, like fp32 mode -- no packs, no slots, no range guard
  bool f64_mode() const { return conv_mode == 5; }
  // activation-exponent slots (conv_common.h): one u32 per blob of THIS lane = bit pattern of max |value| of the unit
  // it currently holds; zeroed at the start of every forward / unit, raised by the producers' epilogues, read by the
  // single-accumulator split-fp16 kernels.  Concat members share their owner's slot.
  DevBuf amax_slots;
  unsigned* amax_slot(int bi) const {
    if (!amax_slots.p || !fp16_mode()) return nullptr;
    const int o = blobs[bi].owner >= 0 ? blobs[bi].owner : bi;
    return (unsigned*)amax_slots.p + o;
  }
  void reset_amax(hipStream_t st) {
    if (fp16_mode() && amax_slots.p) HIP_THROW(hipMemsetAsync(amax_slots.p, 0, blobs.size() * 4, st));
  }
  DevBuf range_flag;  // device int: raised by a split-fp16 conv epilogue that produced |x| > 65504 (fp16 hi overflows)
  // Net.forward() in a split-fp16 mode on a detector graph runs the FUSED path's kernels (fused first pair, pools in the
  // convolutions' epilogues, split activation format -- the very pass shf_detect_add_level runs, so lib/test.py's ten
  // net.forward() calls give the detections of the device-resident path bit for bit) and leaves the intermediate blobs
  // unmaterialised: `plain_stale`.  Reading one of them (Blob.data) then runs the per-layer kernels once, everything but
  // the proposal tail (ensure_plain), so every name in net.blobs stays readable (pycaffe.py:24-32).
  bool plain_stale = false, inputs_reshaped = false;
  bool forwarded = false;   // forward() has run: the non-input blobs hold an activation (device_data)
  float last_im_info[3] = {0.f, 0.f, 1.f};
  bool forward_fast_eligible() const;
  void ensure_plain();
  std::vector<int> last_data_shape;
  // fused per-image path
  DevBuf img_dets, img_keys, img_count;
  int img_cap = 0, img_units = 0;
  int img_pass = 0;  // append passes since detect_begin: img_count[img_pass & 1] is the current list length
  MergeCtx merge;
  // per-class lists of a multi-class image (net_class_lists.cpp, shf_class_lists_*): tail_C - 1 lists of cl_cap rows each in
  // cl_dets (list c - 1 at row (c - 1) * cl_cap), their lengths in cl_len, the compaction's tile workspace, the staging of
  // shf_debug_class_lists_add; cl_units counts the units added since begin.  Grow-only, on the head only.
  DevBuf cl_dets, cl_len, cl_tiles, cl_stage;
  int cl_cap = 0, cl_units = 0;
  float cur_im_info[3] = {0, 0, 1};
  bool use_blob_im_info = true;

  ~shf_net() {
    if (ev_logits) (void)hipEventDestroy(ev_logits);
    if (ev_group) (void)hipEventDestroy(ev_group);
    if (ev_mark) (void)hipEventDestroy(ev_mark);
    if (stream) {
      (void)hipStreamSynchronize(stream);
      (void)hipStreamDestroy(stream);
    }
  }

  int add_blob(const std::string& name) {
    auto it = blob_index.find(name);
    if (it != blob_index.end()) return it->second;
    Blob b;
    b.name = name;
    blobs.emplace_back();
    blobs.back().name = name;
    blob_index[name] = (int)blobs.size() - 1;
    return (int)blobs.size() - 1;
  }

  View view_of(int bi) const {
    const Blob& b = blobs[bi];
    const int o = b.owner >= 0 ? b.owner : bi;
    const Blob& ob = blobs[o];
    View v;
    v.p = (float*)ob.dev.p;
    v.B = b.shape[0]; v.C = b.shape[1]; v.H = b.shape[2]; v.W = b.shape[3];
    v.cstride = ob.shape[1];
    v.coff = b.coff;
    return v;
  }
  // an NCHW net input on the device: bound externally (fused path) or its own buffer
  const float* nchw_input(int bi) const { return blobs[bi].ext_dev ? blobs[bi].ext_dev : (const float*)blobs[bi].dev.p; }

  void build(const std::string& text, const char* caffemodel);
  void infer_shapes();
  void alloc_buffers();
  void build_module(int mj, const std::map<int, int>& producer, std::map<int, int>& fused_by);   // the back-walk from mods[mj].layer
  void ensure_tail_workspace(TailModule& M, size_t total_anchors);
  void commit_params(int li);
  void build_tail_weights(TailModule& M);
  // the proposal stage's arguments (rebuilds the combined weights after a commit, sizes the workspace); `materialize`:
  // the tail also writes the cls_prob_reshape / bbox_pred blobs (Net.forward())
  TailArgs tail_args(int module, float im_h, float im_w, float im_scale, bool materialize);
  float* probs_out(int module = 0) {
    TailModule& M = mods[module];
    return M.prob_blob >= 0 ? (float*)blobs[M.prob_blob].dev.p : (float*)M.tw_rec.p;
  }
  // this lane's part of the layer walk (net_forward.cpp run_pass), none of which launches anything
  bool split16(const Layer& L) const;          // a split-fp16 kernel runs this conv (kclass 0, packed, eligible shape)
  bool absorbs_first(int li, bool fused) const;   // conv li computes its first-layer producer in its halo staging
  ConvArgs conv_args(int li, bool fused, int* flag) const;   // `flag`: the range flag of the pass
  // the combine launch of layer li (Eltwise, Crop, free-standing ReLU; `member`: which bottom of a copying Concat) with the
  // folds the path allows, and whether the layer runs a launch of its own on that path
  CombineArgs combine_args(int li, bool fused, int member = 0) const;
  bool combine_runs(int li, bool fused) const;
  // the channel-affine launch of the chain that layer li heads: its stages (the same on every lane) and this lane's views
  NormStages norm_stages(int li) const;
  NormArgs norm_args(int li) const;
  // a Pooling layer: whether maxpool_kernel keeps it, else the pooling kernel's geometry and this lane's views and slots
  bool pool_legacy(int li) const;
  PoolGeom pool_geom(int li) const;
  PoolArgs pool_args(int li) const;
  void plan_norm_layers(const std::map<int, int>& fused_by);   // net_graph.cpp: folds into convolutions, in-place chains
  void derive_norm(int li);                                    // a BatchNorm / Scale layer's device vectors from its blobs
  // a convolution's effective parameters with its BatchNorm / Scale folded in (binary64, one rounding per value)
  void fold_conv_params(int li, std::vector<float>& w_eff, std::vector<float>& b_eff) const;
  std::vector<unsigned long long> fold_versions(int li) const;   // the versions of every blob convolution li folds
  const float* conv_bias(const Layer& L) const {
    if (L.fold_bias) return (const float*)L.fold_bias->raw.p;
    return L.params.size() > 1 ? (const float*)L.params[1]->raw.p : nullptr;
  }
  void add_cost(int li, bool fused, int heads, double& flops, double& bytes) const;
  void tail_cost(int module, double& flops, double& bytes) const;   // one module's tail on this lane's unit
  // one unit on this lane: its own stream, range flag and profiler
  void run_unit(bool fused, const float im_info[3], TailStep tail, bool materialize = false);
  void prepare_unit(const float* data, int data_on_device, int H, int W, hipStream_t st);
  void ensure_img_cap(int units_after);
  // Net.forward(): a group of one (net_forward.cpp forward_members).  Per member of a forward: stage_forward before the
  // pass (shapes, host-newer inputs up on the pass's stream, im_info -> last_im_info), record_forward after it
  void forward();
  void stage_forward(hipStream_t st, Prof& pf);
  void record_forward(bool plain, const int* R);   // R[j]: module j's proposal rows
  const float* stage_nchw(int bi, bool is_input);   // an NHWC activation's NCHW image in `stage` (host_data, device_data)
  float* host_data(int bi);
  const float* device_data(int bi);   // Blob.gpu_data(): the blob's fp32 NCHW image on the device (shf_blob_device_data)
  void materialize_fused(int bi);   // Blob.data of a tail-fused blob, re-ordered on the host from the tail workspace
  void load_caffemodel(const std::string& path);
};

constexpr int kMaxGroup = 16;  // units per grouped pass (conv_common.h MAX_GROUP, tail.hip TG)

// One pass of the layer walk (net_forward.cpp run_pass): the layers of one net over the units of 1..16 of its lanes, every
// convolution as ONE launch over the group.  Everything a layer needs comes with the pass.
struct Pass {
  shf_net* head;   // its range flag and profiler serve the pass; TAIL_HANDOVER: its stream runs the tails, it owns ev_convs
  int n = 1;
  struct Unit { shf_net* lane; float im_h, im_w, im_scale; } u[kMaxGroup];   // a lane and its unit's im_info
  bool fused;   // the fused path's kernels (fused first pair, pools in the epilogues, split activations); false: per layer
  hipStream_t s;           // the layers' stream
  TailStep tail;
  bool materialize = false;  // TAIL_LANE / TAIL_GROUP: the tail also writes the cls_prob_reshape / bbox_pred blobs (Net.forward())
  int wait_logits_at = -1;   // before this layer the stream waits for every lane's logits_done (the grouped early start)
};
void run_pass(const Pass& p);

// net_forward.cpp: Net.forward() of n members (the head and / or lanes of its root) as ONE grouped pass on the head's
// stream (shf_net_forward_group): check_group, then the function shf_net::forward() runs with itself as the only member.
// The two differ in three things: the tail step (TAIL_LANE / TAIL_GROUP), the group filling the proposal outputs' host
// mirrors itself, and check_group -- its refusals, shared with shf_blob_load_device_group (net_api.cpp).
void check_group(const char* who, shf_net* head, int n, shf_net* const* members);
void forward_group(shf_net* head, int n, shf_net* const* members);

// net_detect.cpp: append a group of finished units to `net`'s image list (or, per_member, to each member's own) in ONE launch
void append_units(shf_net* net, shf_net* const* srcs, int n, const int* im_w, const float* im_scale, const int* flip,
                  float thresh, bool per_member, hipStream_t st = nullptr, Prof* pf = nullptr);
// ... whose rows carry ONE foreground score: throws, naming the class count, for a net with more than two classes
void refuse_multiclass_lists(const char* who, const shf_net* net);
// ... and that hold ONE list per net, fed from one proposal layer's outputs: throws, naming the entry point and the module
// count, for a net with several proposal layers (its levels go through Net.forward / forward_group and the host merge)
void refuse_multimodule(const char* who, const shf_net* net);

// ---------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------
#define API_BEGIN try {
#define API_END(failval)                  \
  }                                       \
  catch (const std::exception& e) {       \
    set_error(e.what());                  \
    return failval;                       \
  }                                       \
  catch (...) {                           \
    set_error("unknown error");           \
    return failval;                       \
  }

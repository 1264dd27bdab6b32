// Net runtime, part 4: the C ABI of include/shf_hip.h (everything but the detection pipeline, net_detect.cpp).
//
// A static-graph executor for the detector's TEST-phase prototxt: it replaces
// caffe::Net (caffe/src/caffe/net.cpp:28-257 Init, :421-513 AppendParam sharing,
// :516-532 ForwardFromTo, :733-768 CopyTrainedLayersFrom), Blob/SyncedMemory
// (blob.cpp:23-51, syncedmem.cpp:39-91) and the in-graph Python ProposalLayer
// trampoline (include/caffe/layers/python_layer.hpp:14-51) for the layer types that
// graph instantiates.  Differences by design (MI355X-first):
//   * activations stay NHWC on the device; only Blob.data read-back transposes;
//   * conv + bias + in-place ReLU are one kernel; channel concat is zero-copy
//     (producers write channel slices of the concat buffer);
//   * the 1x1 cls/reg convs, concats, softmax, reshape and the proposal layer are
//     one fused device-side tail (no D2H, no Python re-entry);
//   * buffers are grow-only and shape changes re-plan nothing but pointers/sizes.
#include "net_internal.h"
#include "blob_io.h"
#include "eval.h"

namespace shf {
thread_local std::string g_err;
void set_error(const std::string& msg) { g_err = msg; }
std::atomic<long long> g_dev_allocs{0}, g_host_allocs{0};
}  // namespace shf

static std::mutex g_box_mu;
static MergeCtx* g_box_ctx = nullptr;
static hipStream_t g_box_stream = nullptr;
static DevBuf* g_box_in = nullptr;

// device memory, stream and events of ONE shf_wider_eval_counts / shf_face_eval_match / shf_fddb_pair_counts call, on the
// device current at the call:
// nothing outlives it
namespace {
struct CallBuf {
  void* p = nullptr;
  void alloc(size_t bytes) {
    HIP_THROW(hipMalloc(&p, bytes ? bytes : 1));
    poison_fresh(p, bytes ? bytes : 1);
  }
  template <typename T> T* as() const { return (T*)p; }
  ~CallBuf() { if (p) (void)hipFree(p); }
  CallBuf() = default;
  CallBuf(const CallBuf&) = delete;
  CallBuf& operator=(const CallBuf&) = delete;
};
struct CallEvents {
  hipEvent_t e[4] = {nullptr, nullptr, nullptr, nullptr};
  void create() { for (auto& x : e) HIP_THROW(hipEventCreate(&x)); }
  ~CallEvents() { for (auto x : e) if (x) (void)hipEventDestroy(x); }
};
struct CallStream {
  hipStream_t s = nullptr;
  void create() { HIP_THROW(hipStreamCreateWithFlags(&s, hipStreamNonBlocking)); }
  ~CallStream() { if (s) (void)hipStreamDestroy(s); }
};

// offsets of n_images segments: 0 when they are non-negative and non-decreasing, else the message is set
int refuse_offsets(const int* off, int n_images, const char* name) {
  for (int i = 0; i <= n_images; ++i) {
    if (off[i] < 0) { set_error(std::string("wider_eval_counts: negative offset in ") + name); return -1; }
    if (i && off[i] < off[i - 1]) { set_error(std::string("wider_eval_counts: non-monotone offsets in ") + name); return -1; }
  }
  return 0;
}

// the refusals of a device load into input blob `blob` of `net` (argument checks only): the messages of shf_blob_load_device
// behind `prefix` ("member m: " in the grouped entry).  `nc`: the source's (n, c) where the entry receives them.
Blob& check_load(shf_net* net, int blob, const std::string& prefix, const float* src_dev, const int* nc, int h, int w, int flip) {
  Blob& b = net->blobs[blob];
  const std::string what = prefix + "blob_load_device: blob '" + b.name + "' ";
  if (!std::count(net->inputs.begin(), net->inputs.end(), blob) || b.shape.size() != 4)
    throw std::runtime_error(what + "is not a 4-D net input");
  if (!src_dev) throw std::runtime_error(what + "got a NULL source");
  if (nc && (nc[0] != b.shape[0] || nc[1] != b.shape[1]))
    throw std::runtime_error(what + "is (" + std::to_string(b.shape[0]) + ", " + std::to_string(b.shape[1]) +
                             ", ...), the source (" + std::to_string(nc[0]) + ", " + std::to_string(nc[1]) + ", ...)");
  if (h < 1 || w < 1 || h > b.shape[2] || w > b.shape[3])
    throw std::runtime_error(what + "holds " + std::to_string(b.shape[2]) + " x " + std::to_string(b.shape[3]) +
                             " planes, the source has " + std::to_string(h) + " x " + std::to_string(w));
  if (flip != 0 && flip != 1) throw std::runtime_error(what + "flip must be 0 or 1");
  if (b.count() == 0) throw std::runtime_error(what + "has zero elements");
  return b;
}

// ... and what a load leaves behind: the device copy is the blob's head
void mark_loaded(shf_net* net, Blob& b) {
  b.host_newer = false;
  b.dev_newer = true;
  b.ext_dev = nullptr;
  net->inputs_reshaped = true;   // (as after a reshape: the intermediates of the last forward no longer belong to this input)
}
}  // namespace

extern "C" {

const char* shf_last_error(void) { return g_err.c_str(); }
const char* shf_version(void) { return "smallhardface_amd 0.1 (gfx950)"; }
int shf_set_mode_gpu(void) { return 0; }

int shf_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

int shf_set_device(int device_id) {
  API_BEGIN
  HIP_THROW(hipSetDevice(device_id));
  return 0;
  API_END(-1)
}

shf_net* shf_net_create(const char* prototxt_path, const char* prototxt_text, const char* caffemodel_path,
                        int phase) {
  API_BEGIN
  std::string text;
  if (prototxt_text && prototxt_text[0]) {
    text = prototxt_text;
  } else {
    if (!prototxt_path) throw std::runtime_error("no prototxt given");
    std::ifstream f(prototxt_path);
    if (!f) throw std::runtime_error(std::string("Could not open file ") + prototxt_path);
    std::stringstream ss;
    ss << f.rdbuf();
    text = ss.str();
  }
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
    throw std::runtime_error("no HIP device available: the detection runtime has no CPU fallback");
  std::unique_ptr<shf_net> net(new shf_net());
  net->phase = phase;
  net->build(text, caffemodel_path);
  return net.release();
  API_END(nullptr)
}

shf_net* shf_net_clone(shf_net* src) {
  API_BEGIN
  std::unique_ptr<shf_net> net(new shf_net(src->sh));
  net->phase = src->phase;
  net->clone_src = src;
  net->build(src->proto_text, nullptr);
  net->clone_src = nullptr;
  return net.release();
  API_END(nullptr)
}

void shf_net_destroy(shf_net* net) { delete net; }

int shf_net_num_blobs(shf_net* net) { return (int)net->blobs.size(); }
const char* shf_net_blob_name(shf_net* net, int i) {
  if (i < 0 || i >= (int)net->blobs.size()) return nullptr;
  return net->blobs[i].name.c_str();
}
int shf_net_num_inputs(shf_net* net) { return (int)net->inputs.size(); }
int shf_net_input_blob(shf_net* net, int i) { return net->inputs[i]; }
int shf_net_num_outputs(shf_net* net) { return (int)net->outputs.size(); }
int shf_net_output_blob(shf_net* net, int i) { return net->outputs[i]; }
int shf_net_num_layers(shf_net* net) { return (int)net->layers.size(); }
int shf_net_num_classes(shf_net* net) { return net->tail_layer >= 0 ? net->tail_C : 0; }
int shf_net_num_modules(shf_net* net) { return (int)net->mods.size(); }
const char* shf_net_layer_name(shf_net* net, int i) { return net->layers[i].name.c_str(); }
const char* shf_net_layer_type(shf_net* net, int i) { return net->layers[i].type.c_str(); }
int shf_net_layer_num_params(shf_net* net, int layer) { return (int)net->layers[layer].params.size(); }

int shf_net_param_shape(shf_net* net, int layer, int idx, int* dims) {
  auto& p = *net->layers[layer].params[idx];
  for (size_t i = 0; i < p.shape.size(); ++i) dims[i] = p.shape[i];
  return (int)p.shape.size();
}

float* shf_net_param_data(shf_net* net, int layer, int idx) {
  auto& p = *net->layers[layer].params[idx];
  p.dirty = true;
  ++p.version;
  return p.host.data();
}

int shf_net_param_commit(shf_net* net, int layer) {
  API_BEGIN
  // a shared tensor is committed for every layer that holds it
  for (size_t li = 0; li < net->layers.size(); ++li) {
    bool share = (int)li == layer;
    for (auto& p : net->layers[li].params)
      for (auto& q : net->layers[layer].params)
        if (p == q) share = true;
    if (share) net->commit_params((int)li);
  }
  return 0;
  API_END(-1)
}

int shf_blob_reshape(shf_net* net, int blob, const int* dims, int ndim) {
  API_BEGIN
  if (blob < 0 || blob >= (int)net->blobs.size()) throw std::runtime_error("bad blob index");
  Blob& b = net->blobs[blob];
  if (ndim < 0 || ndim > 32) throw std::runtime_error("Blob.reshape: 0 .. 32 axes");
  std::vector<int> s(dims, dims + ndim);
  check_blob_dims(s, b.name);
  if (s != b.shape) {
    b.shape = s;
    if (std::count(net->inputs.begin(), net->inputs.end(), blob)) {
      b.dev.ensure(std::max<size_t>(b.count(), 1) * 4);
      b.host.ensure(std::max<size_t>(b.count(), 1) * 4);
      b.host_newer = true;
      net->inputs_reshaped = true;   // (the device copy of the last forward's input may have been re-allocated: ensure_plain)
    }
  }
  return 0;
  API_END(-1)
}

int shf_blob_shape(shf_net* net, int blob, int* dims) {
  Blob& b = net->blobs[blob];
  for (size_t i = 0; i < b.shape.size(); ++i) dims[i] = b.shape[i];
  return (int)b.shape.size();
}

float* shf_blob_mutable_host_data(shf_net* net, int blob) {
  API_BEGIN
  if (blob < 0 || blob >= (int)net->blobs.size()) throw std::runtime_error("bad blob index");
  return net->host_data(blob);
  API_END(nullptr)
}

// Blob::set_gpu_data with forward_net's pad and detect()'s flip folded in: a level that is already in HBM lands in the
// input blob through blob_io.hip's pad_flip_nchw_kernel on the net's stream, and the device copy becomes the blob's head.
int shf_blob_load_device(shf_net* net, int blob, const float* src_dev, int n, int c, int h, int w, int flip) {
  API_BEGIN
  if (blob < 0 || blob >= (int)net->blobs.size()) throw std::runtime_error("bad blob index");
  const int nc[2] = {n, c};
  Blob& b = check_load(net, blob, "", src_dev, nc, h, w, flip);
  b.dev.ensure(b.count() * 4);
  {
    ProfScope ps(net->prof, net->stream, PC_LAYOUT, 0, 4.0 * ((double)n * c * h * w + (double)b.count()));
    CHECK_RC(launch_pad_flip_nchw(src_dev, n, c, h, w, (float*)b.dev.p, b.shape[2], b.shape[3], flip, net->stream));
  }
  mark_loaded(net, b);
  return 0;
  API_END(-1)
}

// shf_blob_load_device for the same input blob of n members in ONE launch (blob_io.hip pad_flip_nchw_group_kernel) on the
// head's stream: every check of every member first, then the buffers, the launch and the state changes
int shf_blob_load_device_group(shf_net* net, int n, shf_net** members, int blob, const float* const* src_dev, const int* h,
                               const int* w, const int* flip) {
  API_BEGIN
  check_group("blob_load_device_group", net, n, members);
  if (!src_dev || !h || !w || !flip) throw std::runtime_error("blob_load_device_group: NULL argument list");
  if (blob < 0 || blob >= (int)net->blobs.size()) throw std::runtime_error("bad blob index");
  for (int m = 0; m < n; ++m)   // (n and c are the blob's own here: the entry does not receive them)
    check_load(members[m], blob, "member " + std::to_string(m) + ": ", src_dev[m], nullptr, h[m], w[m], flip[m]);
  PadFlipUnit u[kMaxGroup];
  double bytes = 0;
  for (int m = 0; m < n; ++m) {
    Blob& b = members[m]->blobs[blob];
    b.dev.ensure(b.count() * 4);
    u[m] = {src_dev[m], (float*)b.dev.p, b.shape[0], b.shape[1], h[m], w[m], b.shape[2], b.shape[3], flip[m]};
    bytes += 4.0 * ((double)b.shape[0] * b.shape[1] * h[m] * w[m] + (double)b.count());
  }
  // a member's own stream may still read or write its blob (an earlier single load, a read-back): ordered before this copy
  for (int m = 0; m < n; ++m)
    if (members[m]->stream != net->stream) HIP_THROW(hipStreamSynchronize(members[m]->stream));
  {
    ProfScope ps(net->prof, net->stream, PC_LAYOUT, 0, bytes);
    CHECK_RC(launch_pad_flip_nchw_group(u, n, net->stream));
  }
  // ... and a member's later reads of its blob (Blob.data, Blob.device, its own forward) run on its own stream: behind it
  if (!net->ev_group) HIP_THROW(hipEventCreateWithFlags(&net->ev_group, hipEventDisableTiming));
  HIP_THROW(hipEventRecord(net->ev_group, net->stream));
  for (int m = 0; m < n; ++m)
    if (members[m]->stream != net->stream) HIP_THROW(hipStreamWaitEvent(members[m]->stream, net->ev_group, 0));
  for (int m = 0; m < n; ++m) mark_loaded(members[m], members[m]->blobs[blob]);
  return 0;
  API_END(-1)
}

const float* shf_blob_device_data(shf_net* net, int blob) {
  API_BEGIN
  if (blob < 0 || blob >= (int)net->blobs.size()) throw std::runtime_error("bad blob index");
  return net->device_data(blob);
  API_END(nullptr)
}

int shf_net_forward(shf_net* net) {
  API_BEGIN
  net->forward();
  return 0;
  API_END(-1)
}

int shf_net_forward_group(shf_net* net, int n, shf_net** members) {
  API_BEGIN
  forward_group(net, n, members);
  return 0;
  API_END(-1)
}

int shf_net_set_proposal_cfg(shf_net* net, int pre_nms_topN, float score_thresh, float min_size) {
  API_BEGIN
  net->pre_nms_topN = pre_nms_topN;
  net->score_thresh = score_thresh;
  net->min_size = min_size;
  net->alloc_buffers();
  return 0;
  API_END(-1)
}

int shf_net_set_conv_mode(shf_net* net, int mode) {
  API_BEGIN
  if (mode < 0 || mode > 5)
    throw std::runtime_error("conv mode must be 0 (fp32), 1 (split-fp16 x3), 2 (x2), 3 (plain fp16), 4 (bf16) or 5 (f64)");
  if (net->conv_mode == mode) return 0;
  HIP_THROW(hipDeviceSynchronize());  // the mode is shared with every lane: nothing may be in flight while it flips
  net->conv_mode = mode;
  if (net->split_mode()) {   // (fp32 and f64 modes read the fp32 packs / the raw weights, which always exist)
    // the fp32 packs always exist; the split-fp16 packs are made on first use, re-made by every commit in a split
    // mode, and re-made here when a commit in fp32 mode left them stale (also re-runs the |w| <= 65504 check)
    try {
      for (size_t li = 0; li < net->layers.size(); ++li) {
        Layer& L = net->layers[li];
        if (L.type != "Convolution" || L.params.empty()) continue;
        ParamBlob& w = *L.params[0];
        if (L.kclass == 1 && mode == 4 && w.first_frag.p && (!w.first_frag_b.p || w.bf_stale)) net->commit_params((int)li);
        if (L.kclass != 0 || !conv_f16x3_eligible(w.shape[1], w.shape[0], L.k, L.pad, L.dil)) continue;
        if (mode == 4 ? (!w.packed16b.p || w.bf_stale) : (!w.packed16.p || w.split_stale)) net->commit_params((int)li);
      }
    } catch (...) {
      net->conv_mode = 0;  // e.g. a weight outside the fp16 range: stay on the exact kernels
      throw;
    }
  }
  return 0;
  API_END(-1)
}

int shf_net_get_conv_mode(shf_net* net) { return net->conv_mode; }

int shf_net_set_layer_products(shf_net* net, const char* layer, int nprod) {
  API_BEGIN
  if (!layer) throw std::runtime_error("set_layer_products: null layer name");
  if (nprod == 0) {
    net->sh->layer_products.erase(layer);
    return 0;
  }
  if (nprod < 1 || nprod > 3) throw std::runtime_error("set_layer_products: 1, 2 or 3 products (0 clears the override)");
  bool found = false;
  for (auto& L : net->layers) found = found || L.name == layer;
  if (!found) throw std::runtime_error(std::string("set_layer_products: no layer named '") + layer + "'");
  HIP_THROW(hipDeviceSynchronize());
  net->sh->layer_products[layer] = nprod;
  return 0;
  API_END(-1)
}

long long shf_net_range_fallbacks(shf_net* net) { return net->sh->range_fallbacks; }

void shf_alloc_counts(long long* device_allocs, long long* pinned_host_allocs) {
  if (device_allocs) *device_allocs = g_dev_allocs.load();
  if (pinned_host_allocs) *pinned_host_allocs = g_host_allocs.load();
}

int shf_debug_poison_byte(void) { return poison_byte(); }

static void box_ctx_init();

// _get_image_blob of a whole scale list (lib/test.py's detect(): the reference calls cv2.resize here -- a native library as
// well): the uint8 image goes up once and every level is formed by pre.hip's kernel (the arithmetic of the host mirror,
// bit for bit) on the box context's stream, as an UNPADDED (1,3,h,w) blob.  `to_host`: the levels are formed in a buffer of
// the runtime's and copied to out[i] on the host (shf_image_blobs); otherwise out[i] is a caller-owned DEVICE buffer and
// the kernel writes there (shf_image_blobs_device).
static int image_blobs(const char* who, const uint8_t* im_bgr_host, int im_h, int im_w, int n, const double* scales,
                       const double* pixel_means, float* const* out, const int* lvl_h, const int* lvl_w, bool to_host) {
  API_BEGIN
  if (!im_bgr_host || !scales || !pixel_means || !out || !lvl_h || !lvl_w || n < 1 || im_h < 1 || im_w < 1)
    throw std::runtime_error(std::string(who) + ": bad argument");
  std::lock_guard<std::mutex> lk(g_box_mu);
  box_ctx_init();
  static DevBuf* im_dev = new DevBuf();
  static DevBuf* lv_dev = new DevBuf();
  const size_t im_bytes = (size_t)im_h * im_w * 3;
  size_t total = 0;
  for (int i = 0; i < n; ++i) {
    if (lvl_h[i] < 1 || lvl_w[i] < 1 || !(scales[i] > 0)) throw std::runtime_error(std::string(who) + ": bad level geometry");
    if (!to_host && !out[i]) throw std::runtime_error(std::string(who) + ": NULL level buffer");
    total += (size_t)3 * lvl_h[i] * lvl_w[i];
  }
  im_dev->ensure(im_bytes);
  if (to_host) lv_dev->ensure(total * 4);
  HIP_THROW(hipMemcpyAsync(im_dev->p, im_bgr_host, im_bytes, hipMemcpyHostToDevice, g_box_stream));
  size_t off = 0;
  for (int i = 0; i < n; ++i) {
    float* o = to_host ? (float*)lv_dev->p + off : out[i];
    CHECK_RC(launch_pyramid_level((const uint8_t*)im_dev->p, im_h, im_w, scales[i], 0, pixel_means, o, lvl_h[i], lvl_w[i],
                                  lvl_h[i], lvl_w[i], g_box_stream));
    if (to_host)
      HIP_THROW(hipMemcpyAsync(out[i], o, (size_t)3 * lvl_h[i] * lvl_w[i] * 4, hipMemcpyDeviceToHost, g_box_stream));
    off += (size_t)3 * lvl_h[i] * lvl_w[i];
  }
  HIP_THROW(hipStreamSynchronize(g_box_stream));
  return 0;
  API_END(-1)
}

int shf_image_blobs(const uint8_t* im_bgr_host, int im_h, int im_w, int n, const double* scales, const double* pixel_means,
                    float* const* out_host, const int* lvl_h, const int* lvl_w) {
  return image_blobs("image_blobs", im_bgr_host, im_h, im_w, n, scales, pixel_means, out_host, lvl_h, lvl_w, true);
}

int shf_image_blobs_device(const uint8_t* im_bgr_host, int im_h, int im_w, int n, const double* scales,
                           const double* pixel_means, float* const* out_dev, const int* lvl_h, const int* lvl_w) {
  return image_blobs("image_blobs_device", im_bgr_host, im_h, im_w, n, scales, pixel_means, out_dev, lvl_h, lvl_w, false);
}

int shf_device_pci_bus_id(char* out, int cap) {
  API_BEGIN
  if (!out || cap < 16) throw std::runtime_error("device_pci_bus_id: buffer too small");
  int dev = 0;
  HIP_THROW(hipGetDevice(&dev));
  HIP_THROW(hipDeviceGetPCIBusId(out, cap, dev));
  return 0;
  API_END(-1)
}

int shf_net_record_event(shf_net* net) {
  API_BEGIN
  if (!net->ev_mark) HIP_THROW(hipEventCreateWithFlags(&net->ev_mark, hipEventDisableTiming));
  HIP_THROW(hipEventRecord(net->ev_mark, net->stream));
  return 0;
  API_END(-1)
}

int shf_net_wait_event(shf_net* net, shf_net* other) {
  API_BEGIN
  if (other->ev_mark) HIP_THROW(hipStreamWaitEvent(net->stream, other->ev_mark, 0));
  return 0;
  API_END(-1)
}

int shf_net_set_pipeline(shf_net* net, int enable) {
  API_BEGIN
  if (!enable) {
    net->pipelined = false;
    return 0;
  }
  HIP_THROW(hipDeviceSynchronize());
  if (!net->sh->conv_stream) HIP_THROW(hipStreamCreateWithFlags(&net->sh->conv_stream, hipStreamNonBlocking));
  // this head's own stream carries ~100 tiny kernels per image beside the convolutions of the next image:
  // highest priority, so the dispatcher never parks them behind a grid of thousands of workgroups
  int least = 0, greatest = 0;
  HIP_THROW(hipDeviceGetStreamPriorityRange(&least, &greatest));
  if (greatest != least) {
    hipStream_t hs = nullptr;
    HIP_THROW(hipStreamCreateWithPriority(&hs, hipStreamNonBlocking, greatest));
    (void)hipStreamDestroy(net->stream);
    net->stream = hs;
  }
  net->pipelined = true;
  return 0;
  API_END(-1)
}

int shf_net_set_predecessor(shf_net* net, shf_net* prev) {
  API_BEGIN
  net->pred = prev;
  return 0;
  API_END(-1)
}

static void box_ctx_init() {
  if (g_box_ctx) return;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
    throw std::runtime_error("no HIP device available: box merging has no CPU fallback");
  g_box_ctx = new MergeCtx();
  g_box_in = new DevBuf();
  HIP_THROW(hipStreamCreateWithFlags(&g_box_stream, hipStreamNonBlocking));
}

int shf_nms(const float* dets5, int n, float thresh, int device_id, int32_t* keep, int* n_keep) {
  API_BEGIN
  std::lock_guard<std::mutex> lk(g_box_mu);
  *n_keep = 0;
  if (n <= 0) return 0;
  if (device_id >= 0) {
    int cur = -1;
    HIP_THROW(hipGetDevice(&cur));
    if (cur != device_id) HIP_THROW(hipSetDevice(device_id));  // _set_device, nms_kernel.cu:91-100
  }
  CHECK_RC(MergeCtx::refuse_size(n));   // (before the input is staged)
  box_ctx_init();
  g_box_in->ensure((size_t)n * 5 * 4);
  HIP_THROW(hipMemcpyAsync(g_box_in->p, dets5, (size_t)n * 5 * 4, hipMemcpyHostToDevice, g_box_stream));
  return g_box_ctx->run((const float*)g_box_in->p, n, 1, thresh, nullptr, 0, n_keep, keep, g_box_stream);
  API_END(-1)
}

int shf_bbox_vote(const float* dets5, int n, float thresh, double* out5, int cap, int* n_out) {
  API_BEGIN
  std::lock_guard<std::mutex> lk(g_box_mu);
  *n_out = 0;
  if (n <= 0) {
    const double d[5] = {10, 10, 20, 20, 0.0001};
    if (cap > 0) memcpy(out5, d, sizeof(d));
    *n_out = 1;
    return 0;
  }
  CHECK_RC(MergeCtx::refuse_size(n));   // (before the input is staged)
  box_ctx_init();
  g_box_in->ensure((size_t)n * 5 * 4);
  HIP_THROW(hipMemcpyAsync(g_box_in->p, dets5, (size_t)n * 5 * 4, hipMemcpyHostToDevice, g_box_stream));
  return g_box_ctx->run((const float*)g_box_in->p, n, 0, thresh, out5, cap, n_out, nullptr, g_box_stream);
  API_END(-1)
}

int shf_wider_eval_counts(const double* pred5, const int* pred_off, const double* gt4, const int* gt_off,
                          const uint8_t* counted, int n_images, int n_settings, double iou_thresh, int mimic_eval_bug,
                          const double* thresh, int n_thresh, long long* totals, int* hits_out, uint8_t* proposal_out) {
  API_BEGIN
  // ---- refusals: argument checks only, before anything is allocated or launched
  if (!pred_off || !gt_off || !thresh || !totals || n_images < 0)
    throw std::runtime_error("wider_eval_counts: null argument or negative n_images");
  if (n_settings < 1 || n_settings > 8) throw std::runtime_error("wider_eval_counts: n_settings must be 1..8");
  if (!(iou_thresh > 0.0 && iou_thresh <= 1.0)) throw std::runtime_error("wider_eval_counts: iou_thresh must be in (0, 1]");
  if (n_thresh < 1 || n_thresh > (1 << 20)) throw std::runtime_error("wider_eval_counts: n_thresh must be 1..2^20");
  CHECK_RC(refuse_offsets(pred_off, n_images, "pred_off"));
  CHECK_RC(refuse_offsets(gt_off, n_images, "gt_off"));
  const long long N = pred_off[n_images], G = gt_off[n_images];
  if (N * n_settings >= (1ll << 31) || G * n_settings >= (1ll << 31))
    throw std::runtime_error("wider_eval_counts: n_settings x rows reaches 2^31 (detections " + std::to_string(N) +
                             ", ground-truth boxes " + std::to_string(G) + ")");
  long long n_tiles = 0;
  for (int i = 0; i < n_images; ++i) {
    const int g = gt_off[i + 1] - gt_off[i];
    if (g > kEvalMaxGtPerImage)
      throw std::runtime_error("wider_eval_counts: image " + std::to_string(i) + " has " + std::to_string(g) +
                               " ground-truth boxes, the cap per image is " + std::to_string(kEvalMaxGtPerImage));
    n_tiles += ((long long)pred_off[i + 1] - pred_off[i] + 63) / 64;
  }
  if ((N && !pred5) || (G && (!gt4 || !counted))) throw std::runtime_error("wider_eval_counts: null box array");
  const size_t S = (size_t)n_settings, T = (size_t)n_thresh;
  memset(totals, 0, S * T * 2 * sizeof(long long));
  if (N == 0 || G == 0) {   // nothing can be matched: every detection is a proposal of an image that is skipped
    if (hits_out) memset(hits_out, 0, S * (size_t)N * sizeof(int));
    if (proposal_out) memset(proposal_out, 1, S * (size_t)N);
    return 0;
  }
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
    throw std::runtime_error("no HIP device available: wider_eval_counts has no CPU fallback");

  std::vector<int> tile_img((size_t)n_tiles), tile_start((size_t)n_tiles);
  size_t k = 0;
  for (int i = 0; i < n_images; ++i)
    for (int h = pred_off[i]; h < pred_off[i + 1]; h += 64) { tile_img[k] = i; tile_start[k++] = h; }

  CallStream st;
  st.create();
  CallBuf d_pred, d_poff, d_gt4, d_goff, d_counted, d_thresh, d_tiles, d_gt5, d_first, d_match, d_hits, d_cprop, d_prop, d_tot;
  const size_t offb = ((size_t)n_images + 1) * sizeof(int);
  d_pred.alloc((size_t)N * 5 * 8); d_poff.alloc(offb); d_gt4.alloc((size_t)G * 4 * 8); d_goff.alloc(offb);
  d_counted.alloc(S * (size_t)G); d_thresh.alloc(T * 8); d_tiles.alloc((size_t)n_tiles * 2 * sizeof(int));
  d_gt5.alloc((size_t)G * 5 * 8); d_first.alloc((size_t)G * sizeof(int)); d_match.alloc((size_t)N * sizeof(int));
  d_hits.alloc(S * (size_t)N * sizeof(int)); d_cprop.alloc(S * (size_t)N * sizeof(int));
  if (proposal_out) d_prop.alloc(S * (size_t)N);
  d_tot.alloc(S * T * 2 * 8);
  auto up = [&](CallBuf& b, const void* src, size_t bytes) {
    HIP_THROW(hipMemcpyAsync(b.p, src, bytes, hipMemcpyHostToDevice, st.s));
  };
  up(d_pred, pred5, (size_t)N * 5 * 8); up(d_poff, pred_off, offb); up(d_gt4, gt4, (size_t)G * 4 * 8); up(d_goff, gt_off, offb);
  up(d_counted, counted, S * (size_t)G); up(d_thresh, thresh, T * 8);
  up(d_tiles, tile_img.data(), (size_t)n_tiles * sizeof(int));
  HIP_THROW(hipMemcpyAsync(d_tiles.as<int>() + n_tiles, tile_start.data(), (size_t)n_tiles * sizeof(int),
                           hipMemcpyHostToDevice, st.s));
  HIP_THROW(hipMemsetAsync(d_tot.p, 0, S * T * 2 * 8, st.s));
  CHECK_RC(launch_eval_prep(d_gt4.as<double>(), (int)G, d_gt5.as<double>(), d_first.as<int>(), st.s));
  CHECK_RC(launch_eval_match(d_pred.as<double>(), d_poff.as<int>(), d_goff.as<int>(), d_gt5.as<double>(), d_tiles.as<int>(),
                             d_tiles.as<int>() + n_tiles, (int)n_tiles, iou_thresh, mimic_eval_bug != 0, d_match.as<int>(),
                             d_first.as<int>(), st.s));
  CHECK_RC(launch_eval_counts(d_poff.as<int>(), d_match.as<int>(), d_first.as<int>(), d_counted.as<uint8_t>(), n_images,
                              n_settings, (int)N, (int)G, d_hits.as<int>(), d_cprop.as<int>(), d_prop.as<uint8_t>(), st.s));
  CHECK_RC(launch_eval_sweep(d_pred.as<double>(), d_poff.as<int>(), d_goff.as<int>(), d_hits.as<int>(), d_cprop.as<int>(),
                             n_images, n_settings, (int)N, d_thresh.as<double>(), n_thresh,
                             d_tot.as<unsigned long long>(), st.s));
  HIP_THROW(hipMemcpyAsync(totals, d_tot.p, S * T * 2 * 8, hipMemcpyDeviceToHost, st.s));
  if (hits_out) HIP_THROW(hipMemcpyAsync(hits_out, d_hits.p, S * (size_t)N * sizeof(int), hipMemcpyDeviceToHost, st.s));
  if (proposal_out) HIP_THROW(hipMemcpyAsync(proposal_out, d_prop.p, S * (size_t)N, hipMemcpyDeviceToHost, st.s));
  HIP_THROW(hipStreamSynchronize(st.s));
  return 0;
  API_END(-1)
}

int shf_face_eval_match(const double* det4, const long long* det_off, const double* gt4, const long long* gt_off,
                        const uint8_t* difficult, int n_images, double ovr, int* code_out, int* index_out) {
  API_BEGIN
  // ---- refusals: argument checks only, before anything is allocated or launched
  if (!det_off || !gt_off || n_images < 0) throw std::runtime_error("face_eval_match: null offsets or negative n_images");
  if (!(ovr > 0.0 && ovr <= 1.0)) throw std::runtime_error("face_eval_match: ovr must be in (0, 1]");
  for (const auto& [off, name] : {std::pair<const long long*, const char*>{det_off, "det_off"}, {gt_off, "gt_off"}})
    for (int i = 0; i <= n_images; ++i) {
      if (off[i] < 0) throw std::runtime_error(std::string("face_eval_match: negative offset in ") + name);
      if (i && off[i] < off[i - 1]) throw std::runtime_error(std::string("face_eval_match: non-monotone offsets in ") + name);
    }
  const long long N = det_off[n_images], G = gt_off[n_images];
  if (N >= (1ll << 31) || G >= (1ll << 31))
    throw std::runtime_error("face_eval_match: 2^31 rows or more (detections " + std::to_string(N) + ", ground-truth boxes " +
                             std::to_string(G) + ")");
  if ((N && (!det4 || !code_out || !index_out)) || (G && (!gt4 || !difficult)))
    throw std::runtime_error("face_eval_match: null box or output array");
  if (N == 0) return 0;
  if (G == 0) {   // no image has ground truth: every detection is a false positive
    std::fill(code_out, code_out + N, kFaceFalsePositive);
    std::fill(index_out, index_out + N, -1);
    return 0;
  }
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
    throw std::runtime_error("no HIP device available: face_eval_match has no CPU fallback");

  std::vector<int> off32(2 * ((size_t)n_images + 1));   // (the checked offsets fit 31 bits)
  for (int i = 0; i <= n_images; ++i) { off32[i] = (int)det_off[i]; off32[(size_t)n_images + 1 + i] = (int)gt_off[i]; }
  CallStream st;
  st.create();
  CallBuf d_det, d_off, d_gt, d_diff, d_taken, d_code, d_index;
  const size_t offb = off32.size() * sizeof(int);
  d_det.alloc((size_t)N * 4 * 8); d_off.alloc(offb); d_gt.alloc((size_t)G * 4 * 8); d_diff.alloc((size_t)G);
  d_taken.alloc((size_t)G); d_code.alloc((size_t)N * sizeof(int)); d_index.alloc((size_t)N * sizeof(int));
  HIP_THROW(hipMemcpyAsync(d_det.p, det4, (size_t)N * 4 * 8, hipMemcpyHostToDevice, st.s));
  HIP_THROW(hipMemcpyAsync(d_off.p, off32.data(), offb, hipMemcpyHostToDevice, st.s));
  HIP_THROW(hipMemcpyAsync(d_gt.p, gt4, (size_t)G * 4 * 8, hipMemcpyHostToDevice, st.s));
  HIP_THROW(hipMemcpyAsync(d_diff.p, difficult, (size_t)G, hipMemcpyHostToDevice, st.s));
  HIP_THROW(hipMemsetAsync(d_taken.p, 0, (size_t)G, st.s));
  CHECK_RC(launch_face_match(d_det.as<double>(), d_off.as<int>(), d_gt.as<double>(), d_off.as<int>() + n_images + 1,
                             d_diff.as<uint8_t>(), n_images, ovr, d_taken.as<uint8_t>(), d_code.as<int>(),
                             d_index.as<int>(), st.s));
  HIP_THROW(hipMemcpyAsync(code_out, d_code.p, (size_t)N * sizeof(int), hipMemcpyDeviceToHost, st.s));
  HIP_THROW(hipMemcpyAsync(index_out, d_index.p, (size_t)N * sizeof(int), hipMemcpyDeviceToHost, st.s));
  HIP_THROW(hipStreamSynchronize(st.s));
  return 0;
  API_END(-1)
}

int shf_fddb_pair_counts(const double* ell6, const int* ell_box, const long long* ann_off, const int* rect4,
                         const long long* det_off, int n_images, int* inter_out, int* area_out, double* phase_ms) {
  API_BEGIN
  // ---- refusals: argument checks only, before anything is allocated or launched
  if (!ann_off || !det_off || n_images < 0) throw std::runtime_error("fddb_pair_counts: null offsets or negative n_images");
  for (const auto& [off, name] : {std::pair<const long long*, const char*>{ann_off, "ann_off"}, {det_off, "det_off"}})
    for (int i = 0; i <= n_images; ++i) {
      if (off[i] < 0) throw std::runtime_error(std::string("fddb_pair_counts: negative offset in ") + name);
      if (i && off[i] < off[i - 1]) throw std::runtime_error(std::string("fddb_pair_counts: non-monotone offsets in ") + name);
    }
  const long long A = ann_off[n_images] - ann_off[0], D = det_off[n_images] - det_off[0];
  if (ann_off[0] != 0 || det_off[0] != 0) throw std::runtime_error("fddb_pair_counts: offsets must start at 0");
  if (A >= (1ll << 31) || D >= (1ll << 31))
    throw std::runtime_error("fddb_pair_counts: 2^31 rows or more (annotations " + std::to_string(A) + ", detections " +
                             std::to_string(D) + ")");
  long long P = 0;
  for (int i = 0; i < n_images; ++i) {
    P += (ann_off[i + 1] - ann_off[i]) * (det_off[i + 1] - det_off[i]);   // (each factor is below 2^31, P below 2^26 so far)
    if (P >= kFddbMaxPairs)
      throw std::runtime_error("fddb_pair_counts: 2^26 (annotation, detection) pairs or more (one wave per pair in one launch)");
  }
  if ((A && (!ell6 || !ell_box || !area_out)) || (D && !rect4) || (P && !inter_out))
    throw std::runtime_error("fddb_pair_counts: null shape or output array");
  for (const auto& [box, rows, name] : {std::tuple<const int*, long long, const char*>{ell_box, A, "scan box"},
                                        {rect4, D, "rectangle"}})
    for (long long k = 0; k < rows * 4; ++k)
      if (box[k] >= kFddbMaxCoord || box[k] <= -kFddbMaxCoord)
        throw std::runtime_error(std::string("fddb_pair_counts: a ") + name + " corner of 2^30 or more in magnitude (row " +
                                 std::to_string(k / 4) + ")");
  for (long long a = 0; a < A; ++a) {
    const long long w = (long long)ell_box[a * 4 + 2] - ell_box[a * 4 + 0] + 1, h = (long long)ell_box[a * 4 + 3] - ell_box[a * 4 + 1] + 1;
    if (w > 0 && h > 0 && w * h > kFddbMaxScanBox)
      throw std::runtime_error("fddb_pair_counts: annotation " + std::to_string(a) + " has a scan box of " + std::to_string(w) +
                               " x " + std::to_string(h) + " pixels, the cap is " + std::to_string(kFddbMaxScanBox));
  }
  if (phase_ms) phase_ms[0] = phase_ms[1] = phase_ms[2] = 0.0;
  if (A == 0) return 0;   // (no annotations: no pairs either)
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
    throw std::runtime_error("no HIP device available: fddb_pair_counts has no CPU fallback");

  // per annotation: where its pairs start (A + 1 offsets) and its image's first detection
  std::vector<int> pair_off((size_t)A + 1), det0((size_t)A);
  long long p = 0;
  for (int i = 0; i < n_images; ++i)
    for (long long a = ann_off[i]; a < ann_off[i + 1]; ++a) {
      pair_off[(size_t)a] = (int)p;
      det0[(size_t)a] = (int)det_off[i];
      p += det_off[i + 1] - det_off[i];
    }
  pair_off[(size_t)A] = (int)p;
  CallStream st;
  st.create();
  CallBuf d_ell, d_box, d_rect, d_poff, d_det0, d_inter, d_area;
  CallEvents ev;   // (only with phase_ms: start, uploads done, kernels done, read-back done)
  if (phase_ms) ev.create();
  auto mark = [&](int k) { if (phase_ms) HIP_THROW(hipEventRecord(ev.e[k], st.s)); };
  d_ell.alloc((size_t)A * 6 * 8); d_box.alloc((size_t)A * 4 * sizeof(int)); d_rect.alloc((size_t)D * 4 * sizeof(int));
  d_poff.alloc(((size_t)A + 1) * sizeof(int)); d_det0.alloc((size_t)A * sizeof(int));
  d_inter.alloc((size_t)P * sizeof(int)); d_area.alloc((size_t)A * sizeof(int));
  mark(0);
  HIP_THROW(hipMemcpyAsync(d_ell.p, ell6, (size_t)A * 6 * 8, hipMemcpyHostToDevice, st.s));
  HIP_THROW(hipMemcpyAsync(d_box.p, ell_box, (size_t)A * 4 * sizeof(int), hipMemcpyHostToDevice, st.s));
  if (D) HIP_THROW(hipMemcpyAsync(d_rect.p, rect4, (size_t)D * 4 * sizeof(int), hipMemcpyHostToDevice, st.s));
  HIP_THROW(hipMemcpyAsync(d_poff.p, pair_off.data(), ((size_t)A + 1) * sizeof(int), hipMemcpyHostToDevice, st.s));
  HIP_THROW(hipMemcpyAsync(d_det0.p, det0.data(), (size_t)A * sizeof(int), hipMemcpyHostToDevice, st.s));
  mark(1);
  CHECK_RC(launch_fddb_pairs(d_ell.as<double>(), d_box.as<int>(), d_rect.as<int>(), d_poff.as<int>(), d_det0.as<int>(), (int)A,
                             (int)P, d_inter.as<int>(), st.s));
  CHECK_RC(launch_fddb_areas(d_ell.as<double>(), d_box.as<int>(), (int)A, d_area.as<int>(), st.s));
  mark(2);
  if (P) HIP_THROW(hipMemcpyAsync(inter_out, d_inter.p, (size_t)P * sizeof(int), hipMemcpyDeviceToHost, st.s));
  HIP_THROW(hipMemcpyAsync(area_out, d_area.p, (size_t)A * sizeof(int), hipMemcpyDeviceToHost, st.s));
  mark(3);
  HIP_THROW(hipStreamSynchronize(st.s));
  if (phase_ms)
    for (int k = 0; k < 3; ++k) {
      float ms = 0;
      HIP_THROW(hipEventElapsedTime(&ms, ev.e[k], ev.e[k + 1]));
      phase_ms[k] = ms;
    }
  return 0;
  API_END(-1)
}

int shf_caffemodel_read_blob(const char* path, const char* layer, int idx, float* out, int cap, int* dims,
                             int* ndim) {
  API_BEGIN
  auto src = read_caffemodel(path);
  for (auto& L : src) {
    if (L.name != layer) continue;
    if (idx < 0 || idx >= (int)L.blobs.size()) throw std::runtime_error("caffemodel: blob index out of range");
    const WireBlob& b = L.blobs[idx];
    *ndim = (int)std::min<size_t>(b.shape.size(), 8);
    for (int i = 0; i < *ndim; ++i) dims[i] = (int)b.shape[i];
    if (out) std::copy(b.data.begin(), b.data.begin() + std::min<size_t>(b.data.size(), (size_t)cap), out);
    return (int)b.data.size();
  }
  throw std::runtime_error(std::string("caffemodel: no layer named '") + layer + "'");
  API_END(-1)
}

int shf_debug_handover_event(shf_net* net, int* waits, int* holds) {
  API_BEGIN
  if (!net || !waits || !holds) throw std::runtime_error("debug_handover_event: null argument");
  *waits = net->logits_done != nullptr;
  *holds = net->logits_done && (net->logits_done == net->ev_logits ||
                                (net->logits_keep && net->logits_keep->e == net->logits_done));
  return 0;
  API_END(-1)
}

// diagnostics: run the merge pipeline and hand back its intermediates (tests only)
int shf_debug_merge(const float* dets5, int n, float thresh, int ge_pred, unsigned long long* mask_out,
                    int* cluster_out, int* heads_out, int* n_heads, float* sorted_out, int* perm_out) {
  API_BEGIN
  std::lock_guard<std::mutex> lk(g_box_mu);
  CHECK_RC(MergeCtx::refuse_size(n));   // (before the input is staged)
  box_ctx_init();
  g_box_in->ensure((size_t)n * 5 * 4);
  HIP_THROW(hipMemcpyAsync(g_box_in->p, dets5, (size_t)n * 5 * 4, hipMemcpyHostToDevice, g_box_stream));
  int nk = 0;
  std::vector<int32_t> keep(n);
  std::vector<double> tmp((size_t)n * 5);
  CHECK_RC(g_box_ctx->run((const float*)g_box_in->p, n, ge_pred ? 0 : 1, thresh, tmp.data(), n, &nk, keep.data(),
                          g_box_stream));
  const size_t nw = ((size_t)n + 63) / 64;
  HIP_THROW(hipMemcpy(mask_out, g_box_ctx->mask.p, (size_t)n * nw * 8, hipMemcpyDeviceToHost));
  HIP_THROW(hipMemcpy(cluster_out, g_box_ctx->cluster.p, (size_t)n * 4, hipMemcpyDeviceToHost));
  HIP_THROW(hipMemcpy(sorted_out, g_box_ctx->sorted.p, (size_t)n * 5 * 4, hipMemcpyDeviceToHost));
  HIP_THROW(hipMemcpy(perm_out, g_box_ctx->perm.p, (size_t)n * 4, hipMemcpyDeviceToHost));
  int cnt[2];
  HIP_THROW(hipMemcpy(cnt, g_box_ctx->counters.p, 8, hipMemcpyDeviceToHost));
  *n_heads = cnt[0];
  HIP_THROW(hipMemcpy(heads_out, g_box_ctx->heads.p, (size_t)cnt[0] * 4, hipMemcpyDeviceToHost));
  return 0;
  API_END(-1)
}

// diagnostics: the proposal stage alone on injected blobs (tests only)
int shf_debug_proposal(shf_net* net, const float* scores, const float* deltas, int h, int w, const float* im_info3,
                       float* out_boxes5, float* out_probs, int cap, int* n_out, int* overflow) {
  API_BEGIN
  if (net->tail_layer < 0) throw std::runtime_error("net has no proposal layer");
  refuse_multimodule("debug_proposal", net);
  if (h < 1 || w < 1) throw std::runtime_error("debug_proposal: bad map size");
  // (any (h, w): the layer itself does not care that the real graph only produces even head maps)
  TailModule& M = net->mods[0];
  const int A = M.A, NC = net->tail_C;
  const size_t K = (size_t)h * w;
  net->ensure_tail_workspace(M, K * A);
  DevBuf ds, dd;
  ds.ensure(K * NC * A * 4);
  dd.ensure(K * 4 * A * 4);
  hipStream_t st = net->stream;
  HIP_THROW(hipMemcpyAsync(ds.p, scores, K * NC * A * 4, hipMemcpyHostToDevice, st));
  HIP_THROW(hipMemcpyAsync(dd.p, deltas, K * 4 * A * 4, hipMemcpyHostToDevice, st));
  TailArgs t;
  t.A = A; t.C = NC; t.heads = M.heads; t.Cf = M.Cf;
  t.h = h; t.w = w;
  for (int i = 0; i < A * 4; ++i) t.anchors[i] = (float)M.anchors[i];
  for (int i = 0; i < A; ++i) t.sub_stride[i] = M.sub_stride[i];
  t.feat_stride = M.feat_stride;
  t.im_h = im_info3[0]; t.im_w = im_info3[1]; t.im_scale = im_info3[2];
  t.min_size = net->min_size; t.score_thresh = net->score_thresh; t.pre_nms_topN = net->pre_nms_topN;
  t.probs_given = 1;
  float* boxes = (float*)net->blobs[M.boxes_blob].dev.p;
  float* probs = net->probs_out();
  CHECK_RC(launch_tail_inject(t, M.tw, (const float*)ds.p, (const float*)dd.p, st));
  CHECK_RC(launch_tail(t, M.tw, boxes, probs, st, nullptr, 2));
  int cnt[8];
  HIP_THROW(hipMemcpyAsync(cnt, M.tw.counters, sizeof(cnt), hipMemcpyDeviceToHost, st));
  HIP_THROW(hipStreamSynchronize(st));
  const int R = cnt[2];
  if (overflow) *overflow = cnt[1];
  // ProposalLayer's tops: (max(R,1), 5) with the dummy roi when R == 0, and (R, C)   proposal_layer.py:207-220
  const int rows_b = std::max(R, 1);
  if (n_out) *n_out = R;
  HIP_THROW(hipMemcpy(out_boxes5, boxes, (size_t)std::min(rows_b, cap) * 5 * 4, hipMemcpyDeviceToHost));
  if (R > 0) HIP_THROW(hipMemcpy(out_probs, probs, (size_t)std::min(R, cap) * NC * 4, hipMemcpyDeviceToHost));
  net->blobs[M.boxes_blob].shape = {rows_b, 5};
  if (M.prob_blob >= 0) net->blobs[M.prob_blob].shape = {R, NC};
  return 0;
  API_END(-1)
}

// diagnostics: forward_net's flip fix + unscale and detect()'s >thresh cut (append_dets_kernel) on injected
// proposals, appended to the current image's list (shf_detect_begin first; export with shf_detect_export)
int shf_debug_append(shf_net* net, const float* boxes5, const float* probs2, int R, int im_w, float im_scale,
                     int flip, float thresh) {
  API_BEGIN
  if (net->tail_layer < 0) throw std::runtime_error("net has no proposal layer");
  refuse_multimodule("debug_append", net);
  refuse_multiclass_lists("debug_append", net);
  if (R < 0) throw std::runtime_error("debug_append: R < 0");
  TailModule& M = net->mods[0];
  M.tw_counters.ensure(64);
  M.tw.counters = (int*)M.tw_counters.p;
  Blob& bb = net->blobs[M.boxes_blob];
  bb.dev.ensure((size_t)std::max(R, 1) * 5 * 4);
  float* probs;
  if (M.prob_blob >= 0) {
    net->blobs[M.prob_blob].dev.ensure((size_t)std::max(R, 1) * 2 * 4);
    probs = (float*)net->blobs[M.prob_blob].dev.p;
  } else {
    M.tw_rec.ensure((size_t)std::max(R, 1) * 2 * 4);
    probs = (float*)M.tw_rec.p;
  }
  hipStream_t st = net->stream;
  if (R > 0) {
    HIP_THROW(hipMemcpyAsync(bb.dev.p, boxes5, (size_t)R * 5 * 4, hipMemcpyHostToDevice, st));
    HIP_THROW(hipMemcpyAsync(probs, probs2, (size_t)R * 2 * 4, hipMemcpyHostToDevice, st));
  }
  const int cnt[8] = {R, 0, R, 0, 0, 0, 0, 0};  // C candidates (all kept: topN is raised below), published R
  HIP_THROW(hipMemcpyAsync(M.tw.counters, cnt, sizeof(cnt), hipMemcpyHostToDevice, st));
  HIP_THROW(hipStreamSynchronize(st));
  Restore<int> topN(net->pre_nms_topN);
  net->pre_nms_topN = std::max(R, 1);  // append_unit sizes its launch and the list growth from it
  append_units(net, &net, 1, &im_w, &im_scale, &flip, thresh, false);
  return 0;
  API_END(-1)
}

int shf_generate_anchors(int base_size, const double* ratios, int n_ratios, const double* scales, int n_scales,
                         const double* shifts, int n_shifts, const double* strides, double* out, int cap_rows) {
  API_BEGIN
  std::vector<double> a;
  gen_anchors(base_size, std::vector<double>(ratios, ratios + n_ratios), std::vector<double>(scales, scales + n_scales),
              std::vector<double>(shifts, shifts + n_shifts), std::vector<double>(strides, strides + n_scales), a);
  const int rows = (int)a.size() / 4;
  if (rows > cap_rows) throw std::runtime_error("anchor output buffer too small");
  std::copy(a.begin(), a.end(), out);
  return rows;
  API_END(-1)
}

int shf_prof_enable(shf_net* net, int enable) {
  net->prof.on = enable != 0;
  return 0;
}
int shf_prof_only(shf_net* net, int cls) {
  net->prof.only = (cls >= 0 && cls < PC_COUNT) ? cls : -1;
  return 0;
}
int shf_prof_num_classes(shf_net*) { return PC_COUNT; }
const char* shf_prof_class_name(shf_net*, int cls) {
  return (cls >= 0 && cls < PC_COUNT) ? kProfNames[cls] : nullptr;
}
int shf_prof_read(shf_net* net, int cls, int64_t* launches, double* total_ms, double* flops, double* bytes) {
  API_BEGIN
  if (cls < 0 || cls >= PC_COUNT) throw std::runtime_error("bad profile class");
  net->prof.drain();
  *launches = net->prof.launches[cls];
  *total_ms = net->prof.ms[cls];
  *flops = net->prof.flops[cls];
  *bytes = net->prof.bytes[cls];
  return 0;
  API_END(-1)
}
int shf_prof_reset(shf_net* net) {
  API_BEGIN
  net->prof.drain();
  for (int i = 0; i < PC_COUNT; ++i) {
    net->prof.launches[i] = 0;
    net->prof.ms[i] = net->prof.flops[i] = net->prof.bytes[i] = 0;
  }
  return 0;
  API_END(-1)
}
int shf_calib_matrix_pipe(int bf16, int zero_eighths, int constant_operands, int iters, int reps, double* tflops) {
  API_BEGIN
  if (!tflops || iters < 1 || reps < 1 || zero_eighths < 0 || zero_eighths > 8)
    throw std::runtime_error("calib_matrix_pipe: bad arguments");
  const int rc = calib_matrix_pipe(bf16, zero_eighths, constant_operands, iters, reps, tflops);
  if (rc != 0) throw std::runtime_error(std::string("calib_matrix_pipe: ") + hipGetErrorString((hipError_t)rc));
  return 0;
  API_END(-1)
}
int shf_debug_conv_plan(int cin, int cout, int h, int w, int in_split, int pooled, long long* lds_bytes, long long* grid_blocks,
                        int* slim) {
  API_BEGIN
  if (!lds_bytes || !grid_blocks || !slim || cin < 1 || cout < 1 || h < 1 || w < 1) throw std::runtime_error("debug_conv_plan: bad arguments");
  const int nl = conv_f16x3_plan_probe(cin, cout, h, w, in_split, pooled, lds_bytes, grid_blocks, slim);
  if (nl < 0) return -1;
  return nl;
  API_END(-1)
}
int shf_debug_conv_plan_group(int n, const int* b, const int* h, const int* w, int cin, int cout, int in_split, int pooled, int first_pair,
                              int cus, long long* launches, int* pc_tab) {
  API_BEGIN
  if (!h || !w || !launches || !pc_tab || n < 1 || cin < 1 || cout < 1 || cus < 0) throw std::runtime_error("debug_conv_plan_group: bad arguments");
  for (int i = 0; i < n; ++i)
    if (h[i] < 1 || w[i] < 1 || (b && b[i] < 1)) throw std::runtime_error("debug_conv_plan_group: bad arguments");
  if (first_pair && (cin != 64 || cout != 64)) throw std::runtime_error("debug_conv_plan_group: the first pair is 64 -> 64");
  const int nl = conv_f16x3_plan_probe_group(n, b, h, w, cin, cout, in_split, pooled, first_pair, cus, launches, pc_tab);
  if (nl < 0) return -1;
  return nl;
  API_END(-1)
}
int shf_net_sync(shf_net* net) {
  API_BEGIN
  HIP_THROW(hipStreamSynchronize(net->stream));
  return 0;
  API_END(-1)
}

}  // extern "C"

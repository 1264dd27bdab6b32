// Net runtime, part 1: the graph -- prototxt -> layers / blobs / parameter sharing, the fusion plans (conv + pool, fused
// first pair, split-format blobs, the three shared-weight heads), shape inference, buffers, parameter packs.
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

#include <cerrno>

namespace shf {

// generate_anchors.py:11-86 in double precision
void gen_anchors(int base_size, const std::vector<double>& ratios, const std::vector<double>& scales,
                        const std::vector<double>& shifts, const std::vector<double>& strides,
                        std::vector<double>& out) {
  out.clear();
  const double bw = base_size, bh = base_size;  // base anchor (0,0,base-1,base-1)
  const double bxc = 0 + 0.5 * (bw - 1), byc = 0 + 0.5 * (bh - 1);
  const double size = bw * bh;
  for (double r : ratios) {
    const double ws = std::nearbyint(std::sqrt(size / r));
    const double hs = std::nearbyint(ws * r);
    // ratio anchor
    const double rx1 = bxc - 0.5 * (ws - 1), ry1 = byc - 0.5 * (hs - 1);
    const double rx2 = bxc + 0.5 * (ws - 1), ry2 = byc + 0.5 * (hs - 1);
    const double w = rx2 - rx1 + 1, h = ry2 - ry1 + 1;
    const double xc = rx1 + 0.5 * (w - 1), yc = ry1 + 0.5 * (h - 1);
    const size_t ns = std::min(scales.size(), strides.size());  // zip(scales, strides)
    for (size_t j = 0; j < ns; ++j) {
      const double sw = w * scales[j], sh = h * scales[j];
      const double a[4] = {xc - 0.5 * (sw - 1), yc - 0.5 * (sh - 1), xc + 0.5 * (sw - 1), yc + 0.5 * (sh - 1)};
      for (double sy : shifts)
        for (double sx : shifts) {
          out.push_back(a[0] + sx * strides[j]);
          out.push_back(a[1] + sy * strides[j]);
          out.push_back(a[2] + sx * strides[j]);
          out.push_back(a[3] + sy * strides[j]);
        }
    }
  }
}

// "{'feat_stride': [8,8,8],'scales': [1,2,4], 'ratios':[1,]}" -> key -> numbers
std::map<std::string, std::vector<double>> parse_param_str(const std::string& s) {
  std::map<std::string, std::vector<double>> out;
  size_t i = 0;
  while (i < s.size()) {
    const size_t q = s.find_first_of("'\"", i);
    if (q == std::string::npos) break;
    const size_t q2 = s.find(s[q], q + 1);
    if (q2 == std::string::npos) break;
    const std::string key = s.substr(q + 1, q2 - q - 1);
    size_t c = s.find(':', q2);
    if (c == std::string::npos) break;
    ++c;
    while (c < s.size() && isspace((unsigned char)s[c])) ++c;
    std::vector<double> vals;
    size_t end = c;
    if (c < s.size() && (s[c] == '[' || s[c] == '(')) {
      end = s.find_first_of("])", c);
      if (end == std::string::npos) end = s.size();
      std::string body = s.substr(c + 1, end - c - 1);
      for (auto& ch : body)
        if (ch == ',') ch = ' ';
      std::stringstream ss(body);
      std::string tok;
      while (ss >> tok) {
        if (tok == "True" || tok == "true") vals.push_back(1);
        else if (tok == "False" || tok == "false") vals.push_back(0);
        else vals.push_back(std::strtod(tok.c_str(), nullptr));
      }
      ++end;
    } else {
      end = s.find_first_of(",}", c);
      if (end == std::string::npos) end = s.size();
      std::string tok = s.substr(c, end - c);
      while (!tok.empty() && isspace((unsigned char)tok.back())) tok.pop_back();
      if (tok == "True" || tok == "true") vals.push_back(1);
      else if (tok == "False" || tok == "false") vals.push_back(0);
      else vals.push_back(std::strtod(tok.c_str(), nullptr));
    }
    out[key] = vals;
    i = end;
  }
  return out;
}

int conv_out(int n, int k, int pad, int stride, int dil) {
  const int kext = dil * (k - 1) + 1;
  return (n + 2 * pad - kext) / stride + 1;
}

}  // namespace shf

static int geti(const PMsg* m, const char* n, int d) {
  if (!m) return d;
  const long v = m->num(n, d);          // (a value outside int would wrap: clamp, the range checks below refuse it by name)
  return v > 2147483647L ? 2147483647 : (v < -2147483647L ? -2147483647 : (int)v);
}

// ---- scalars that must parse completely as their field's type.  strtol / strtod stop at the first character they cannot use
// and atoi gives 0 for none: `kernel_size: 3.7` would be 3 and `pad: x` 0 without a word, where protobuf's text format fails
// the whole file.  Every scalar of the messages the graph reads is checked once, before anything reads it.
namespace {
struct TypedField { const char* msg; const char* field; char kind; };   // kind: i(nteger), f(loat), b(ool)
const TypedField kTypedFields[] = {
    {"convolution_param", "num_output", 'i'}, {"convolution_param", "bias_term", 'b'}, {"convolution_param", "pad", 'i'},
    {"convolution_param", "kernel_size", 'i'}, {"convolution_param", "stride", 'i'}, {"convolution_param", "dilation", 'i'},
    {"convolution_param", "pad_h", 'i'}, {"convolution_param", "pad_w", 'i'}, {"convolution_param", "kernel_h", 'i'},
    {"convolution_param", "kernel_w", 'i'}, {"convolution_param", "stride_h", 'i'}, {"convolution_param", "stride_w", 'i'},
    {"convolution_param", "group", 'i'}, {"convolution_param", "axis", 'i'}, {"convolution_param", "force_nd_im2col", 'b'},
    {"pooling_param", "pad", 'i'}, {"pooling_param", "pad_h", 'i'}, {"pooling_param", "pad_w", 'i'},
    {"pooling_param", "kernel_size", 'i'}, {"pooling_param", "kernel_h", 'i'}, {"pooling_param", "kernel_w", 'i'},
    {"pooling_param", "stride", 'i'}, {"pooling_param", "stride_h", 'i'}, {"pooling_param", "stride_w", 'i'},
    {"pooling_param", "global_pooling", 'b'}, {"relu_param", "negative_slope", 'f'}, {"eltwise_param", "coeff", 'f'},
    {"eltwise_param", "stable_prod_grad", 'b'}, {"crop_param", "axis", 'i'}, {"crop_param", "offset", 'i'},
    {"batch_norm_param", "use_global_stats", 'b'}, {"batch_norm_param", "moving_average_fraction", 'f'},
    {"batch_norm_param", "eps", 'f'}, {"scale_param", "axis", 'i'}, {"scale_param", "num_axes", 'i'},
    {"scale_param", "bias_term", 'b'}, {"norm_param", "across_spatial", 'b'}, {"norm_param", "channel_shared", 'b'},
    {"norm_param", "eps", 'f'}, {"concat_param", "axis", 'i'}, {"concat_param", "concat_dim", 'i'},
    {"softmax_param", "axis", 'i'}, {"reshape_param", "axis", 'i'}, {"reshape_param", "num_axes", 'i'},
    {"python_param", "share_in_parallel", 'b'}, {"shape", "dim", 'i'}, {"input_shape", "dim", 'i'},
    {"scale_filler", "value", 'f'},
    {"prelu_param", "channel_shared", 'b'}, {"elu_param", "alpha", 'f'}, {"threshold_param", "threshold", 'f'},
    {"power_param", "power", 'f'}, {"power_param", "scale", 'f'}, {"power_param", "shift", 'f'},
    {"exp_param", "base", 'f'}, {"exp_param", "scale", 'f'}, {"exp_param", "shift", 'f'},
    {"log_param", "base", 'f'}, {"log_param", "scale", 'f'}, {"log_param", "shift", 'f'},
};

// the layer types that run the neuron kernel (neuron.hip)
bool neuron_type(const std::string& t) {
  for (const char* n : {"PReLU", "Sigmoid", "TanH", "ELU", "AbsVal", "Threshold", "BNLL", "Power", "Exp", "Log"})
    if (t == n) return true;
  return false;
}

bool bool_text(const std::string& s, bool& v) {   // the spellings protobuf's text format takes for a bool
  if (s == "true" || s == "True" || s == "t" || s == "1") { v = true; return true; }
  if (s == "false" || s == "False" || s == "f" || s == "0") { v = false; return true; }
  return false;
}

void check_scalar(const std::string& who, const std::string& path, const PField& f, char kind) {
  const char* b = f.scalar.c_str();
  char* e = nullptr;
  bool ok = !f.quoted && !f.msg && *b;
  const char* what = kind == 'i' ? "an integer" : kind == 'f' ? "a number" : "a bool (true / false)";
  if (ok && kind == 'i') {          // (decimal only: a hexadecimal or octal literal is refused, not misread)
    errno = 0;
    std::strtoll(b, &e, 10);
    ok = e != b && *e == 0 && errno == 0;
  } else if (ok && kind == 'f') {   // (text format lets a float end in 'f')
    std::strtod(b, &e);
    ok = e != b && (*e == 0 || ((*e == 'f' || *e == 'F') && e[1] == 0));
  } else if (ok) {
    bool v;
    ok = bool_text(f.scalar, v);
  }
  if (!ok) throw std::runtime_error(who + path + ": '" + f.scalar + "' is not " + what);
}

// every typed scalar directly inside message `m` (named `mname` by its parent), and inside its sub-messages
void check_typed(const std::string& who, const std::string& mname, const PMsg* m, int depth = 0) {
  for (const PField& f : m->fields) {
    if (f.msg) {
      if (depth < 3) check_typed(who, f.name, f.msg.get(), depth + 1);
      continue;
    }
    for (const TypedField& t : kTypedFields)
      if (mname == t.msg && f.name == t.field) check_scalar(who, mname + "." + f.name, f, t.kind);
  }
}

bool getb(const PMsg* m, const char* n, bool d) {
  const PField* f = m ? m->get(n) : nullptr;
  bool v = d;
  if (f && !bool_text(f->scalar, v)) throw std::runtime_error(std::string(n) + ": '" + f->scalar + "' is not a bool");
  return v;
}

// One spatial hyper-parameter of a Convolution / Deconvolution by BaseConvolutionLayer::LayerSetUp's rules
// (base_conv_layer.cpp:36-117): the repeated field holds one value for both axes or one per axis, or the *_h / *_w pair
// stands in its place -- never both.  Only square geometry has kernels here: equal axes mean that square, unequal ones are
// refused by name.
int conv_spatial(const std::string& who, const PMsg* cp, const char* rep, const char* fh, const char* fw, int dflt, bool required) {
  auto val = [](const PField* f) {
    const long v = std::strtol(f->scalar.c_str(), nullptr, 10);
    return v > 2147483647L ? 2147483647 : (v < -2147483647L ? -2147483647 : (int)v);
  };
  const auto vals = cp->all(rep);
  const PField *h = fh ? cp->get(fh) : nullptr, *w = fw ? cp->get(fw) : nullptr;   // (dilation has no *_h / *_w form)
  const std::string hw = fh ? std::string(fh) + " / " + fw : std::string();
  if (h || w) {
    if (!vals.empty())
      throw std::runtime_error(who + "both " + rep + " and " + hw + " given: it is one or the other");
    if (!h || !w) throw std::runtime_error(who + (h ? fh : fw) + " without " + (h ? fw : fh) + ": give both");
    if (val(h) != val(w))
      throw std::runtime_error(who + "rectangular " + hw + " (" + std::to_string(val(h)) + " x " + std::to_string(val(w)) +
                               ") not supported: both axes must be equal");
    return val(h);
  }
  if (vals.empty()) {
    if (required) throw std::runtime_error(who + "no filter size: give " + rep + ", or " + fh + " and " + fw);
    return dflt;
  }
  if (vals.size() > 2)
    throw std::runtime_error(who + rep + " given " + std::to_string(vals.size()) + " times: give it once, or once per spatial axis (2)");
  if (vals.size() == 2 && val(vals[0]) != val(vals[1]))
    throw std::runtime_error(who + "rectangular " + rep + " (" + std::to_string(val(vals[0])) + " x " + std::to_string(val(vals[1])) +
                             ") not supported: both axes must be equal");
  return val(vals[0]);
}
}  // namespace

// Blob::Reshape (blob.cpp:23-51): at most 32 axes, every dim >= 0, count <= INT_MAX
void shf::check_blob_dims(const std::vector<int>& shp, const std::string& name) {
  if (shp.size() > 32) throw std::runtime_error("blob '" + name + "': more than 32 axes");
  long long count = 1;
  for (int d : shp) {
    if (d < 0) throw std::runtime_error("blob '" + name + "': negative dimension");
    if (d != 0 && count > 2147483647LL / d) throw std::runtime_error("blob '" + name + "': size exceeds INT_MAX");
    count *= d;
  }
}

// One proposal module: walk back from its ProposalLayer through the layers folded into the tail
void shf_net::build_module(int mj, const std::map<int, int>& producer, std::map<int, int>& fused_by) {
  TailModule& M = mods[mj];
  Layer& T = layers[M.layer];
  std::set<int> fused_layers;
  if (T.bottoms.size() != 3 || T.tops.empty())
    throw std::runtime_error("ProposalLayer: expected bottoms (cls_prob, bbox_pred, im_info)");
  M.cls_blob = T.bottoms[0];
  M.box_blob = T.bottoms[1];
  M.boxes_blob = T.tops[0];
  M.prob_blob = T.tops.size() > 1 ? T.tops[1] : -1;
  auto prod = [&](int blob, const char* want) -> int {
    auto it = producer.find(blob);
    if (it == producer.end() || layers[it->second].type != want)
      throw std::runtime_error(std::string("tail: expected a ") + want + " producing '" + blobs[blob].name + "'");
    return it->second;
  };
  // cls branch: Reshape <- Softmax <- (Concat axis2 of 1x1 convs | Reshape <- 1x1 conv)
  const int l_rs = prod(M.cls_blob, "Reshape");
  const int l_sm = prod(layers[l_rs].bottoms[0], "Softmax");
  fused_layers.insert(l_rs);
  fused_layers.insert(l_sm);
  int pre = layers[l_sm].bottoms[0], l_pre_rs = -1;
  auto pit = producer.find(pre);
  if (pit == producer.end()) throw std::runtime_error("tail: dangling softmax input");
  if (layers[pit->second].type == "Concat") {
    const int l_cc = pit->second;
    if (layers[l_cc].concat_axis != 2)
      throw std::runtime_error("tail: class-score concat must be on axis 2");
    fused_layers.insert(l_cc);
    for (int b : layers[l_cc].bottoms) M.cls_layers.push_back(prod(b, "Convolution"));
  } else if (layers[pit->second].type == "Reshape") {
    l_pre_rs = pit->second;
    fused_layers.insert(pit->second);
    M.cls_layers.push_back(prod(layers[pit->second].bottoms[0], "Convolution"));
  } else {
    throw std::runtime_error("tail: unsupported class-score branch");
  }
  // box branch: Concat axis1 of 1x1 convs | single 1x1 conv
  auto bit = producer.find(M.box_blob);
  if (bit == producer.end()) throw std::runtime_error("tail: dangling bbox input");
  if (layers[bit->second].type == "Concat") {
    if (layers[bit->second].concat_axis != 1)
      throw std::runtime_error("tail: bbox concat must be on axis 1");
    fused_layers.insert(bit->second);
    for (int b : layers[bit->second].bottoms) M.box_layers.push_back(prod(b, "Convolution"));
  } else if (layers[bit->second].type == "Convolution") {
    M.box_layers.push_back(bit->second);
  } else {
    throw std::runtime_error("tail: unsupported bbox branch");
  }
  if (M.cls_layers.size() != M.box_layers.size())
    throw std::runtime_error("tail: class / bbox branches disagree");
  M.heads = (int)M.cls_layers.size();
  for (int i = 0; i < M.heads; ++i) {
    Layer& c = layers[M.cls_layers[i]];
    Layer& b = layers[M.box_layers[i]];
    if (c.k != 1 || b.k != 1 || c.bottoms[0] != b.bottoms[0])
      throw std::runtime_error("ProposalLayer '" + T.name + "': predictors '" + c.name + "' / '" + b.name + "' (kernel_size " +
                               std::to_string(c.k) + " / " + std::to_string(b.k) + "): cls/bbox predictors must be 1x1 convs on the same head blob");
    // the tail's logits kernel is a matrix product per pixel: a predictor's pad or stride has no place in it, while the
    // blob shapes would still be computed with them
    for (const Layer* p : {&c, &b}) {
      const char* field = p->pad != 0 ? "pad" : p->stride != 1 ? "stride" : p->dil != 1 ? "dilation" : nullptr;
      if (field)
        throw std::runtime_error("ProposalLayer '" + T.name + "': predictor '" + p->name + "' has " + field + " " +
                                 std::to_string(p->pad != 0 ? p->pad : p->stride != 1 ? p->stride : p->dil) +
                                 ": the fused predictors must be 1x1 convolutions with pad 0, stride 1 and dilation 1");
    }
    M.feat_blobs.push_back(c.bottoms[0]);
    fused_layers.insert(M.cls_layers[i]);
    fused_layers.insert(M.box_layers[i]);
  }
  const PMsg* py = T.msg->sub("python_param");
  auto ps = parse_param_str(py->str("param_str"));
  std::vector<double> fs = ps.count("feat_stride") ? ps["feat_stride"] : std::vector<double>{16};
  std::vector<double> scales = ps.count("scales") ? ps["scales"] : std::vector<double>{8, 16, 32};
  std::vector<double> ratios = ps.count("ratios") ? ps["ratios"] : std::vector<double>{0.5, 1, 2};
  std::vector<double> shifts = ps.count("shifts") ? ps["shifts"] : std::vector<double>{0};
  const int base_size = ps.count("base_size") ? (int)ps["base_size"][0] : 16;
  const bool subsampled = ps.count("subsampled") ? ps["subsampled"][0] != 0 : true;
  if (ps.count("num_feats") && ps["num_feats"][0] != 1) throw std::runtime_error("tail: num_feats != 1 unsupported");
  // what the reference's layer cannot run is refused here with the layer's name, not answered: an empty list raises in its
  // setup, a stride below 1 divides by zero in the subsampling map (proposal_layer.py:163-164)
  if (fs.empty() || scales.empty() || ratios.empty() || shifts.empty())
    throw std::runtime_error("ProposalLayer '" + T.name + "': feat_stride, scales, ratios and shifts need at least one entry");
  for (double v : fs)
    if (!(v >= 1 && v <= 4096))
      throw std::runtime_error("ProposalLayer '" + T.name + "': feat_stride entries must be in 1 .. 4096");
  gen_anchors(base_size, ratios, scales, shifts, fs, M.anchors);
  M.A = (int)M.anchors.size() / 4;
  if (M.A < 1) throw std::runtime_error("ProposalLayer '" + T.name + "': the param string yields no anchors");
  if (M.A > 8) throw std::runtime_error("tail: more than 8 anchors per cell unsupported");
  M.feat_stride = (int)fs[0];
  M.sub_stride.assign(M.A, 1);
  if (subsampled) {
    // anchor i is kept on every (feat_stride[i // len(shifts)**2] // feat_stride[0])-th row and column
    // (proposal_layer.py:160-165): with fewer feat_stride entries than that index reaches the reference raises IndexError
    const size_t need = (size_t)(M.A - 1) / (shifts.size() * shifts.size()) + 1;
    if (fs.size() < need)
      throw std::runtime_error("ProposalLayer '" + T.name + "': feat_stride has " + std::to_string(fs.size()) +
                               " entries, the anchor subsampling of " + std::to_string(M.A) + " anchors indexes " +
                               std::to_string(need) + " (the reference raises IndexError); give one stride per anchor "
                               "group or 'subsampled': False");
    for (int i = 0; i < M.A; ++i) {
      const size_t idx = (size_t)i / (shifts.size() * shifts.size());
      M.sub_stride[i] = (int)fs[idx] / (int)fs[0];
      if (M.sub_stride[i] < 1)   // (a slice step of zero: ValueError in the reference)
        throw std::runtime_error("ProposalLayer '" + T.name + "': feat_stride entries must not be smaller than the first one");
    }
  }
  if (M.heads != 1 && M.heads != M.A) throw std::runtime_error("tail: heads must be 1 or == anchors");
  // the class count (proposal_layer.py:118: scores.shape[1] / A): every per-head predictor has C outputs, the single-blob
  // one C * A with channel c * A + a; the Reshapes around the softmax must say the same
  const std::string who = "ProposalLayer '" + T.name + "': ";
  const bool per_head = M.heads != 1;
  int C = -1;
  for (int i = 0; i < M.heads; ++i) {
    const Layer& c = layers[M.cls_layers[i]];
    if (!per_head && c.nout % M.A)
      throw std::runtime_error(who + "class predictor '" + c.name + "' has " + std::to_string(c.nout) + " outputs, not a multiple of the " +
                               std::to_string(M.A) + " anchors");
    const int ci = per_head ? c.nout : c.nout / M.A;
    if (C >= 0 && ci != C)
      throw std::runtime_error(who + "class predictors '" + layers[M.cls_layers[0]].name + "' and '" + c.name +
                               "' disagree on the class count (" + std::to_string(C) + " vs " + std::to_string(ci) + ")");
    C = ci;
    if (layers[M.box_layers[i]].nout != (per_head ? 4 : 4 * M.A))
      throw std::runtime_error(who + "bbox predictor '" + layers[M.box_layers[i]].name + "' channel count does not match the anchors");
  }
  auto reshape_dim1 = [&](int li2) {
    const PMsg* rp = layers[li2].msg->sub("reshape_param");
    std::vector<int> dims;
    if (rp && rp->sub("shape"))
      for (auto d : rp->sub("shape")->all("dim")) dims.push_back(atoi(d->scalar.c_str()));
    return dims.size() > 1 ? dims[1] : 0;
  };
  if (l_pre_rs >= 0 && reshape_dim1(l_pre_rs) != C)
    throw std::runtime_error(who + "Reshape '" + layers[l_pre_rs].name + "' makes " + std::to_string(reshape_dim1(l_pre_rs)) +
                             " class planes, the predictor has " + std::to_string(C) + " classes per anchor");
  if (reshape_dim1(l_rs) != C * M.A)
    throw std::runtime_error(who + "Reshape '" + layers[l_rs].name + "' makes " + std::to_string(reshape_dim1(l_rs)) +
                             " channels, the predictors give " + std::to_string(C) + " classes x " + std::to_string(M.A) + " anchors");
  if (C < 2) throw std::runtime_error(who + "at least 2 classes (background and one foreground class) are needed, the predictors have " + std::to_string(C));
  if (C > kTailMaxClasses)
    throw std::runtime_error(who + std::to_string(C) + " classes: the tail supports at most " + std::to_string(kTailMaxClasses));
  // Net.num_classes is one number, and the tail kernels are instantiated on it: the modules of a net agree on it
  if (mj > 0 && C != tail_C)
    throw std::runtime_error("ProposalLayers '" + layers[mods[0].layer].name + "' and '" + T.name + "' disagree on the class count (" +
                             std::to_string(tail_C) + " vs " + std::to_string(C) + "): the modules of a net share one class count");
  tail_C = C;
  // a layer folded into one module's tail has its top in that module's workspace alone: a predictor, score concat / reshape
  // or softmax that two proposal layers both read would have to live in both
  for (int li2 : fused_layers) {
    auto own = fused_by.find(li2);
    if (own != fused_by.end() && own->second != mj)
      throw std::runtime_error("ProposalLayers '" + layers[mods[own->second].layer].name + "' and '" + T.name + "' both fuse layer '" +
                               layers[li2].name + "' (blob '" + blobs[layers[li2].tops[0]].name + "'): every module needs its own "
                               "predictors, softmax and reshapes");
    fused_by[li2] = mj;
  }
  for (int li2 : fused_layers) {
    layers[li2].op = OP_SKIP;
    // what the top holds, for the on-demand read-back (shf_net::materialize_fused)
    int role = FR_NONE, head = -1;
    for (int i = 0; i < M.heads; ++i) {
      if (M.cls_layers[i] == li2) role = FR_CLS_CONV, head = i;
      if (M.box_layers[i] == li2) role = FR_BOX_CONV, head = i;
    }
    if (role == FR_NONE && layers[li2].type == "Softmax") role = FR_PROB_PLANES;
    if (role == FR_NONE && (layers[li2].type == "Concat" || layers[li2].type == "Reshape")) role = FR_CLS_PLANES;
    for (int t : layers[li2].tops) {
      blobs[t].kind = BK_FUSED;
      blobs[t].fused_role = role;
      blobs[t].fused_head = head;
      blobs[t].fused_mod = mj;
    }
  }
  blobs[M.cls_blob].kind = BK_NCHW_MAT;
  blobs[M.box_blob].kind = BK_NCHW_MAT;
  blobs[M.boxes_blob].kind = BK_FLAT;
  if (M.prob_blob >= 0) blobs[M.prob_blob].kind = BK_FLAT;
}

void shf_net::build(const std::string& text, const char* caffemodel) {
  proto_text = text;
  if (!clone_src && getenv("SHF_CONV_MODE")) conv_mode = atoi(getenv("SHF_CONV_MODE"));
  range_flag.ensure(64);
  fill_now(range_flag.p, 0, 64);
  TextParser tp(proto_text);
  root = tp.parse();
  HIP_THROW(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
  CHECK_RC(conv_init_attributes());

  // ---- inputs: legacy `input:` + input_shape / input_dim (upgrade_proto.cpp:966-1000)
  // legacy V1 `layers { ... }` entries (caffe.proto NetParameter.layers; Caffe upgrades them, upgrade_proto.cpp): not read
  // here, so a net that has any would silently lose them
  if (root->get("layers"))
    throw std::runtime_error("net: legacy V1 'layers' entries are not supported: write the net with 'layer' (LayerParameter)");
  for (auto s : root->all("input_shape"))
    if (s->msg) check_typed("net: ", "input_shape", s->msg.get());
  for (auto d : root->all("input_dim")) check_scalar("net: ", "input_dim", *d, 'i');
  auto in_names = root->all("input");
  auto in_shapes = root->all("input_shape");
  auto in_dims = root->all("input_dim");
  for (size_t i = 0; i < in_names.size(); ++i) {
    const int bi = add_blob(in_names[i]->scalar);
    inputs.push_back(bi);
    std::vector<int> shp;
    if (i < in_shapes.size() && in_shapes[i]->msg)
      for (auto d : in_shapes[i]->msg->all("dim")) shp.push_back(atoi(d->scalar.c_str()));
    else
      for (size_t j = 4 * i; j < 4 * i + 4 && j < in_dims.size(); ++j) shp.push_back(atoi(in_dims[j]->scalar.c_str()));
    if (shp.empty()) shp = {1};
    check_blob_dims(shp, in_names[i]->scalar);
    blobs[bi].shape = shp;
  }
  for (auto lf : root->all("layer")) {
    const PMsg* lm = lf->msg.get();
    if (!lm) continue;
    Layer L;
    L.msg = lm;
    L.name = lm->str("name");
    L.type = lm->str("type");
    {
      // Net::FilterNet (net.cpp:259-285) drops a layer whose include / exclude rules or phase do not meet the net's state;
      // nothing here filters, so a TRAIN-only layer would run: refused by name.  Inline `blobs` (Layer's constructor copies
      // them into the layer's parameters, layer.hpp:46-55) are not read either: the values come from a caffemodel
      const std::string who = "layer '" + L.name + "': ";
      for (const char* f : {"include", "exclude"})
        if (lm->get(f))
          throw std::runtime_error(who + f + " rules are not supported: write the TEST-phase net without them");
      const std::string phase = lm->str("phase", "TEST");
      if (phase != "TEST" && phase != "1")
        throw std::runtime_error(who + "phase " + phase + ": only TEST-phase layers are supported");
      if (lm->get("blobs"))
        throw std::runtime_error(who + "inline blobs are not read: give the parameters in a caffemodel or through Net.params");
      check_typed(who, "layer", lm);
    }
    if (L.type == "Input") {
      auto tops = lm->all("top");
      const PMsg* ip = lm->sub("input_param");
      auto shapes = ip ? ip->all("shape") : std::vector<const PField*>();
      for (size_t i = 0; i < tops.size(); ++i) {
        const int bi = add_blob(tops[i]->scalar);
        inputs.push_back(bi);
        std::vector<int> shp;
        if (i < shapes.size() && shapes[i]->msg)
          for (auto d : shapes[i]->msg->all("dim")) shp.push_back(atoi(d->scalar.c_str()));
        if (shp.empty()) shp = {1};
        check_blob_dims(shp, tops[i]->scalar);
        blobs[bi].shape = shp;
        L.tops.push_back(bi);
      }
      layers.push_back(L);
      continue;
    }
    for (auto b : lm->all("bottom")) {
      auto it = blob_index.find(b->scalar);
      if (it == blob_index.end())
        throw std::runtime_error("Unknown bottom blob '" + b->scalar + "' (layer '" + L.name + "')");
      L.bottoms.push_back(it->second);
    }
    for (auto t : lm->all("top")) L.tops.push_back(add_blob(t->scalar));
    layers.push_back(L);
  }
  for (int bi : inputs) {
    Blob& b = blobs[bi];
    b.kind = (b.shape.size() == 4) ? BK_INPUT_NCHW : BK_FLAT;
    if (b.name == "data") data_blob = bi;
    if (b.name == "im_info") im_info_blob = bi;
  }
  if (data_blob < 0) {
    for (int bi : inputs)
      if (blobs[bi].shape.size() == 4) { data_blob = bi; break; }
  }
  // outputs = blobs still "available" after the last layer (net.cpp:95-110,240-246): a bottom
  // takes a blob off the set, a top (also an in-place one) puts it back; the set is ordered
  // by NAME (std::set<string>), and an input nobody reads is an output too.
  {
    std::set<std::string> avail;
    for (int bi : inputs) avail.insert(blobs[bi].name);
    for (auto& L : layers) {
      if (L.type == "Input") continue;
      for (int b : L.bottoms) avail.erase(blobs[b].name);
      for (int t : L.tops) avail.insert(blobs[t].name);
    }
    for (auto& n : avail) outputs.push_back(blob_index[n]);
  }

  // ---- layer hyper-parameters, params, op assignment
  std::map<int, int> producer;  // blob -> last producing layer
  for (size_t li = 0; li < layers.size(); ++li) {
    Layer& L = layers[li];
    if (L.type == "Convolution" || L.type == "Deconvolution") {
      const PMsg* cp = L.msg->sub("convolution_param");
      if (!cp) throw std::runtime_error("layer '" + L.name + "': missing convolution_param");
      L.nout = geti(cp, "num_output", 0);
      const std::string who = "layer '" + L.name + "': ";
      L.k = conv_spatial(who, cp, "kernel_size", "kernel_h", "kernel_w", 0, true);
      L.pad = conv_spatial(who, cp, "pad", "pad_h", "pad_w", 0, false);
      L.stride = conv_spatial(who, cp, "stride", "stride_h", "stride_w", 1, false);
      L.dil = conv_spatial(who, cp, "dilation", nullptr, nullptr, 1, false);
      L.group = geti(cp, "group", 1);
      L.bias_term = getb(cp, "bias_term", true);
      // the channel axis is 1 and the spatial axes are the two behind it (base_conv_layer.cpp:24-33); another axis is an N-D
      // or a 1-D convolution, and force_nd_im2col only matters to those
      const int axis = geti(cp, "axis", 1);
      if (axis != 1 && axis != -3)
        throw std::runtime_error(who + "axis " + std::to_string(axis) + ": only 2-D convolution over the last two axes (axis 1) is supported");
      if (getb(cp, "force_nd_im2col", false)) throw std::runtime_error(who + "force_nd_im2col: true is not supported");
      // DeconvolutionLayer::compute_output_shape (deconv_layer.cpp:8-24) uses the dilated extent; the kernel here does not
      if (L.type == "Deconvolution" && L.dil != 1 && L.dil >= 1 && L.dil <= 64)
        throw std::runtime_error(who + "dilation " + std::to_string(L.dil) + ": a Deconvolution's dilation must be 1");
      // BaseConvolutionLayer::LayerSetUp's CHECKs (base_conv_layer.cpp:21-120): Caffe aborts on these, here the graph is refused
      // with the layer's name -- a hostile prototxt must not reach a division by a zero stride or a 2^31-channel allocation
      if (L.nout < 1 || L.nout > (1 << 20)) throw std::runtime_error("layer '" + L.name + "': num_output must be in 1 .. 2^20");
      if (L.k < 1 || L.k > 64) throw std::runtime_error("layer '" + L.name + "': kernel_size must be in 1 .. 64");
      if (L.stride < 1 || L.stride > 64) throw std::runtime_error("layer '" + L.name + "': stride must be in 1 .. 64");
      if (L.dil < 1 || L.dil > 64) throw std::runtime_error("layer '" + L.name + "': dilation must be in 1 .. 64");
      if (L.pad < 0 || L.pad > 4096) throw std::runtime_error("layer '" + L.name + "': pad must be in 0 .. 4096");
      if (L.group < 1 || L.nout % L.group) throw std::runtime_error("layer '" + L.name + "': group must divide num_output");
      L.op = (L.type == "Convolution") ? OP_CONV : OP_DECONV;
    } else if (L.type == "ReLU") {
      // relu_layer.cpp: max(x, 0) + negative_slope * min(x, 0), in place or not (NeuronLayer: one bottom, one top)
      if (L.bottoms.size() != 1 || L.tops.size() != 1)
        throw std::runtime_error("ReLU '" + L.name + "': takes exactly one bottom and one top (" + std::to_string(L.bottoms.size()) +
                                 " / " + std::to_string(L.tops.size()) + " given)");
      const double slope = L.msg->sub("relu_param") ? L.msg->sub("relu_param")->real("negative_slope", 0) : 0.0;
      L.slope = (float)slope;
      if (!std::isfinite(slope) || !std::isfinite(L.slope))
        throw std::runtime_error("ReLU '" + L.name + "': negative_slope is not a finite fp32 number");
      const bool in_place = L.bottoms[0] == L.tops[0];
      auto pit = producer.find(L.bottoms[0]);
      if (in_place && L.slope == 0.f && pit != producer.end() && layers[pit->second].type == "Convolution") {
        // the detector's own case: folded into the convolution's epilogue.  Nothing may read the pre-activation value
        // between the conv and this ReLU
        for (size_t lj = pit->second + 1; lj < li; ++lj)
          for (int b : layers[lj].bottoms)
            if (b == L.bottoms[0]) throw std::runtime_error("ReLU '" + L.name + "': blob read before activation");
        layers[pit->second].relu = 1;
        L.op = OP_SKIP;
      } else {
        if (std::count(inputs.begin(), inputs.end(), L.bottoms[0]))
          throw std::runtime_error("ReLU '" + L.name + "': bottom '" + blobs[L.bottoms[0]].name + "' is a net input: the layer reads NHWC "
                                   "activations, put a convolution in between");
        L.op = OP_RELU;
      }
    } else if (L.type == "Eltwise") {
      // EltwiseLayer::LayerSetUp / Reshape (eltwise_layer.cpp:10-40): Caffe CHECKs these and aborts, here the graph is refused
      const std::string who = "Eltwise '" + L.name + "': ";
      const PMsg* ep = L.msg->sub("eltwise_param");
      const std::string opn = ep ? ep->str("operation", "SUM") : "SUM";
      if (opn == "SUM" || opn == "1") L.eop = COMBINE_SUM;
      else if (opn == "PROD" || opn == "0") L.eop = COMBINE_PROD;
      else if (opn == "MAX" || opn == "2") L.eop = COMBINE_MAX;
      else throw std::runtime_error(who + "unknown operation '" + opn + "' (PROD, SUM or MAX)");
      if (L.bottoms.size() < 2)
        throw std::runtime_error(who + "needs at least 2 bottoms, " + std::to_string(L.bottoms.size()) + " given");
      if (L.bottoms.size() > (size_t)kCombineMaxIn)
        throw std::runtime_error(who + std::to_string(L.bottoms.size()) + " bottoms: at most " + std::to_string(kCombineMaxIn) +
                                 " are supported");
      if (L.tops.size() != 1) throw std::runtime_error(who + "takes exactly one top");
      if (ep)
        for (auto c : ep->all("coeff")) L.coeff.push_back((float)std::strtod(c->scalar.c_str(), nullptr));
      if (!L.coeff.empty() && L.coeff.size() != L.bottoms.size())
        throw std::runtime_error(who + std::to_string(L.coeff.size()) + " coeff values for " + std::to_string(L.bottoms.size()) +
                                 " bottoms: Eltwise takes one coefficient per bottom, or none");
      if (!L.coeff.empty() && L.eop != COMBINE_SUM)
        throw std::runtime_error(who + "takes coefficients only for summation (operation " + opn + ")");
      for (float c : L.coeff)
        if (!std::isfinite(c)) throw std::runtime_error(who + "a coeff is not a finite fp32 number");
      if (L.coeff.empty()) L.coeff.assign(L.bottoms.size(), 1.f);
      for (int b : L.bottoms) {
        if (std::count(inputs.begin(), inputs.end(), b))
          throw std::runtime_error(who + "bottom '" + blobs[b].name + "' is a net input: the layer reads NHWC activations, put a "
                                   "convolution in between");
        if (b == L.tops[0]) throw std::runtime_error(who + "cannot run in place on '" + blobs[b].name + "'");
      }
      L.op = OP_ELTWISE;
    } else if (L.type == "Crop") {
      // CropLayer::LayerSetUp (crop_layer.cpp:15-34)
      const std::string who = "Crop '" + L.name + "': ";
      if (L.bottoms.size() != 2 || L.tops.size() != 1)
        throw std::runtime_error(who + "takes exactly two bottoms (the data and the blob that gives the size) and one top, " +
                                 std::to_string(L.bottoms.size()) + " / " + std::to_string(L.tops.size()) + " given");
      const PMsg* cp = L.msg->sub("crop_param");
      int axis = geti(cp, "axis", 2);
      if (axis < 0) axis += 4;   // (CanonicalAxisIndex of a 4-D blob)
      if (axis < 0 || axis > 3) throw std::runtime_error(who + "axis " + std::to_string(geti(cp, "axis", 2)) + " is outside a 4-D blob");
      if (axis == 0) throw std::runtime_error(who + "axis 0: cropping the batch axis is not supported");
      L.crop_axis = axis;
      if (cp)
        for (auto o : cp->all("offset")) L.crop_offsets.push_back(atoi(o->scalar.c_str()));
      if (L.crop_offsets.size() > 1 && (int)L.crop_offsets.size() != 4 - axis)
        throw std::runtime_error(who + std::to_string(L.crop_offsets.size()) + " offsets for " + std::to_string(4 - axis) +
                                 " cropped axes (axis " + std::to_string(axis) + "): give none, one for all, or one per cropped axis");
      for (int b : L.bottoms)
        if (std::count(inputs.begin(), inputs.end(), b))
          throw std::runtime_error(who + "bottom '" + blobs[b].name + "' is a net input: the layer reads NHWC activations, "
                                   "put a convolution in between");
      if (L.bottoms[0] == L.tops[0] || L.bottoms[1] == L.tops[0])
        throw std::runtime_error(who + "cannot run in place on '" + blobs[L.tops[0]].name + "'");
      L.op = OP_CROP;
    } else if (L.type == "BatchNorm" || L.type == "Scale") {
      // BatchNormLayer::LayerSetUp (batch_norm_layer.cpp:10-50, inference only) / ScaleLayer::LayerSetUp (scale_layer.cpp:12-60)
      const std::string who = L.type + " '" + L.name + "': ";
      L.is_bn = L.type == "BatchNorm";
      if (!L.is_bn && L.bottoms.size() == 2)
        throw std::runtime_error(who + "the two-bottom form (the scale as a second bottom) is not supported: give the scale as the "
                                 "layer's parameter blob");
      if (L.bottoms.size() != 1 || L.tops.size() != 1)
        throw std::runtime_error(who + "takes exactly one bottom and one top (" + std::to_string(L.bottoms.size()) + " / " +
                                 std::to_string(L.tops.size()) + " given)");
      if (L.is_bn) {
        const PMsg* bp = L.msg->sub("batch_norm_param");
        if (!getb(bp, "use_global_stats", true))
          throw std::runtime_error(who + "use_global_stats: false asks for batch statistics, which is training: only inference "
                                   "with the stored statistics is supported");
        const double eps = bp ? bp->real("eps", 1e-5) : 1e-5;
        L.eps = (float)eps;
        if (!std::isfinite(eps) || !std::isfinite(L.eps) || eps < 0)
          throw std::runtime_error(who + "eps must be a finite, non-negative fp32 number");
      } else {
        const PMsg* sp = L.msg->sub("scale_param");
        const int axis = geti(sp, "axis", 1), num_axes = geti(sp, "num_axes", 1);
        if ((axis != 1 && axis != -3) || num_axes != 1)
          throw std::runtime_error(who + "axis " + std::to_string(axis) + " / num_axes " + std::to_string(num_axes) +
                                   ": only a per-channel scale (axis 1, num_axes 1) is supported");
        L.bias_term = getb(sp, "bias_term", false);
      }
      if (std::count(inputs.begin(), inputs.end(), L.bottoms[0]))
        throw std::runtime_error(who + "bottom '" + blobs[L.bottoms[0]].name + "' is a net input: the layer reads NHWC activations, put a "
                                 "convolution in between");
      L.op = OP_NORM;
    } else if (L.type == "Normalize") {
      // NormalizeLayer::LayerSetUp (normalize_layer.cpp:11-63), the per-pixel form only
      const std::string who = "Normalize '" + L.name + "': ";
      if (L.bottoms.size() != 1 || L.tops.size() != 1)
        throw std::runtime_error(who + "takes exactly one bottom and one top (" + std::to_string(L.bottoms.size()) + " / " +
                                 std::to_string(L.tops.size()) + " given)");
      const PMsg* np = L.msg->sub("norm_param");
      if (!np || getb(np, "across_spatial", true))
        throw std::runtime_error(who + "across_spatial: true (the default of norm_param) normalises over the whole image, which is "
                                 "not supported: write across_spatial: false for the per-pixel norm over channels");
      L.l2_shared = getb(np, "channel_shared", true);
      const double eps = np->real("eps", 1e-10);
      L.eps = (float)eps;
      if (!std::isfinite(eps) || !std::isfinite(L.eps) || eps < 0)
        throw std::runtime_error(who + "eps must be a finite, non-negative fp32 number");
      // the scale blob before a model is loaded: a constant filler's value; no filler, 1 (normalize_layer.cpp:44-51); any
      // other filler type is random in Caffe and stays 1 here -- the caffemodel brings the values
      const PMsg* sf = np->sub("scale_filler");
      if (sf && sf->str("type", "constant") == "constant") L.l2_fill = (float)sf->real("value", 0.0);
      if (std::count(inputs.begin(), inputs.end(), L.bottoms[0]))
        throw std::runtime_error(who + "bottom '" + blobs[L.bottoms[0]].name + "' is a net input: the layer reads NHWC activations, put a "
                                 "convolution in between");
      L.op = OP_L2NORM;
    } else if (neuron_type(L.type)) {
      // NeuronLayer::Reshape (neuron_layer.cpp:7-11: one bottom, one top of its shape, in place or not) and each type's
      // LayerSetUp; what Caffe CHECKs there and aborts on is a refusal here
      const std::string who = L.type + " '" + L.name + "': ";
      if (L.bottoms.size() != 1 || L.tops.size() != 1)
        throw std::runtime_error(who + "takes exactly one bottom and one top (" + std::to_string(L.bottoms.size()) + " / " +
                                 std::to_string(L.tops.size()) + " given)");
      // a float field of the layer's message, as the fp32 number Caffe holds
      auto field = [&](const PMsg* m, const char* f, double dflt) {
        const double v = m ? m->real(f, dflt) : dflt;
        const float r = (float)v;
        if (!std::isfinite(v) || !std::isfinite(r)) throw std::runtime_error(who + f + " is not a finite fp32 number");
        return r;
      };
      // Exp / Log (exp_layer.cpp:12-22, log_layer.cpp:12-27): log(base) in binary64 from the fp32 base; -1 stands for e
      auto log_of_base = [&](float base) {
        if (base != -1.f && !(base > 0.f))
          throw std::runtime_error(who + "base must be -1 (for e) or strictly positive");
        const double lb = base == -1.f ? 1.0 : std::log((double)base);
        if (lb == 0.0 || std::isnan(lb) || std::isinf(lb))
          throw std::runtime_error(who + "base: log(base) is 0, NaN or inf, no base of an exponential or a logarithm");
        return lb;
      };
      if (L.type == "PReLU") {
        // PReLULayer::LayerSetUp (prelu_layer.cpp:12-45): the slope blob from its filler -- a constant filler's value, no filler
        // 0.25; any other filler type is random in Caffe and stays 0.25 here, the caffemodel brings the values
        const PMsg* pp = L.msg->sub("prelu_param");
        L.prelu_shared = getb(pp, "channel_shared", false);
        const PMsg* fl = pp ? pp->sub("filler") : nullptr;
        if (fl && fl->str("type", "constant") == "constant") {
          if (const PField* v = fl->get("value")) check_scalar(who, "prelu_param.filler.value", *v, 'f');
          L.prelu_fill = (float)fl->real("value", 0.0);
        }
        L.neuron_form = NEURON_PRELU;
      } else if (L.type == "Sigmoid") {
        L.neuron_form = NEURON_SIGMOID;
      } else if (L.type == "TanH") {
        L.neuron_form = NEURON_TANH;
      } else if (L.type == "ELU") {
        L.neuron_form = NEURON_ELU;
        L.neuron_a = field(L.msg->sub("elu_param"), "alpha", 1.0);
      } else if (L.type == "AbsVal") {
        L.neuron_form = NEURON_ABSVAL;
      } else if (L.type == "Threshold") {
        L.neuron_form = NEURON_THRESHOLD;
        L.neuron_a = field(L.msg->sub("threshold_param"), "threshold", 0.0);
      } else if (L.type == "BNLL") {
        L.neuron_form = NEURON_BNLL;
      } else if (L.type == "Power") {
        // PowerLayer::LayerSetUp / Forward_cpu (power_layer.cpp:9-29): diff_scale_ = power * scale in fp32; where it is 0 the
        // top is a constant, formed here in binary64 and rounded once
        const PMsg* pp = L.msg->sub("power_param");
        const float power = field(pp, "power", 1.0), scale = field(pp, "scale", 1.0), shift = field(pp, "shift", 0.0);
        const float diff_scale = power * scale;
        if (diff_scale == 0.f) {
          L.neuron_form = NEURON_CONST;
          L.neuron_a = power == 0.f ? 1.f : (float)std::pow((double)shift, (double)power);
        } else {
          L.neuron_form = power != 1.f ? NEURON_POWER_POW : NEURON_POWER_LIN;
          L.neuron_a = power; L.neuron_b = scale; L.neuron_c = shift;
        }
      } else if (L.type == "Exp") {
        // ExpLayer::LayerSetUp (exp_layer.cpp:12-27): inner = log(base) * scale, outer = base ^ shift (1 for shift 0), in
        // binary64 from the fp32 fields, rounded once (Caffe: in fp32 from float library calls -- an ulp apart at most)
        const PMsg* ep = L.msg->sub("exp_param");
        const float base = field(ep, "base", -1.0), scale = field(ep, "scale", 1.0), shift = field(ep, "shift", 0.0);
        const double lb = log_of_base(base);
        L.neuron_form = NEURON_EXP;
        L.neuron_a = (float)(lb * (double)scale);
        L.neuron_b = shift == 0.f ? 1.f : (float)(base != -1.f ? std::pow((double)base, (double)shift) : std::exp((double)shift));
      } else {
        // LogLayer::LayerSetUp (log_layer.cpp:12-30): base_scale = 1 / log(base), likewise
        const PMsg* lp = L.msg->sub("log_param");
        const float base = field(lp, "base", -1.0), scale = field(lp, "scale", 1.0), shift = field(lp, "shift", 0.0);
        const double bs = 1.0 / log_of_base(base);
        if (std::isnan(bs) || std::isinf(bs) || !std::isfinite((float)bs))
          throw std::runtime_error(who + "base: 1 / log(base) is NaN or inf");
        L.neuron_form = NEURON_LOG;
        L.neuron_a = scale; L.neuron_b = shift; L.neuron_c = (float)bs;
      }
      if (std::count(inputs.begin(), inputs.end(), L.bottoms[0]))
        throw std::runtime_error(who + "bottom '" + blobs[L.bottoms[0]].name + "' is a net input: the layer reads NHWC activations, put a "
                                 "convolution in between");
      L.op = OP_NEURON;
    } else if (L.type == "Pooling") {
      // PoolingLayer::LayerSetUp (pooling_layer.cpp:14-77): Caffe CHECKs these and aborts, here the graph is refused
      const std::string who = "Pooling '" + L.name + "': ";
      const PMsg* pp = L.msg->sub("pooling_param");
      auto has = [&](const char* f) { return pp && pp->get(f) != nullptr; };
      if (L.tops.size() == 2)
        throw std::runtime_error(who + "the second top '" + blobs[L.tops[1]].name + "' (MAX pooling's mask) is not supported: give one top");
      if (L.bottoms.size() != 1 || L.tops.size() != 1)
        throw std::runtime_error(who + "takes exactly one bottom and one top (" + std::to_string(L.bottoms.size()) + " / " +
                                 std::to_string(L.tops.size()) + " given)");
      const std::string method = pp ? pp->str("pool", "MAX") : "MAX";
      if (method == "MAX" || method == "0") L.pool_method = POOL_MAX;
      else if (method == "AVE" || method == "1") L.pool_method = POOL_AVE;
      else throw std::runtime_error(who + "pool: " + method + ": only MAX and AVE pooling are supported");
      L.global_pool = getb(pp, "global_pooling", false);
      const bool k_sq = has("kernel_size"), k_hw = has("kernel_h") || has("kernel_w");
      if (L.global_pool) {
        // the window is the bottom's H x W (set at every reshape): no kernel field, pad 0, stride 1
        if (k_sq || k_hw) throw std::runtime_error(who + "with global_pooling the kernel is the bottom's size: give no kernel_size / kernel_h / kernel_w");
        if (geti(pp, "pad", 0) != 0 || geti(pp, "pad_h", 0) != 0 || geti(pp, "pad_w", 0) != 0 || geti(pp, "stride", 1) != 1 ||
            geti(pp, "stride_h", 1) != 1 || geti(pp, "stride_w", 1) != 1)
          throw std::runtime_error(who + "with global_pooling pad must be 0 and stride 1");
        L.kh = L.kw = L.k = 1;
        L.sh = L.sw = L.stride = 1;
        L.ph = L.pw = L.pad = 0;
      } else {
        if (k_sq && k_hw) throw std::runtime_error(who + "both kernel_size and kernel_h / kernel_w given: the filter size is one or the other");
        if (!k_sq && !(has("kernel_h") && has("kernel_w")))
          throw std::runtime_error(who + "no filter size: give kernel_size, or kernel_h and kernel_w");
        if ((has("pad_h") || has("pad_w")) && has("pad")) throw std::runtime_error(who + "both pad and pad_h / pad_w given: the pad is one or the other");
        if ((has("stride_h") || has("stride_w")) && has("stride"))
          throw std::runtime_error(who + "both stride and stride_h / stride_w given: the stride is one or the other");
        L.kh = k_sq ? geti(pp, "kernel_size", 1) : geti(pp, "kernel_h", 0);
        L.kw = k_sq ? geti(pp, "kernel_size", 1) : geti(pp, "kernel_w", 0);
        const bool p_hw = has("pad_h") || has("pad_w"), s_hw = has("stride_h") || has("stride_w");
        L.ph = p_hw ? geti(pp, "pad_h", 0) : geti(pp, "pad", 0);
        L.pw = p_hw ? geti(pp, "pad_w", 0) : geti(pp, "pad", 0);
        L.sh = s_hw ? geti(pp, "stride_h", 1) : geti(pp, "stride", 1);
        L.sw = s_hw ? geti(pp, "stride_w", 1) : geti(pp, "stride", 1);
        if (L.kh < 1 || L.kh > 64 || L.kw < 1 || L.kw > 64 || L.sh < 1 || L.sh > 64 || L.sw < 1 || L.sw > 64 || L.ph < 0 || L.pw < 0)
          throw std::runtime_error(who + "needs a kernel of 1 .. 64, a stride of 1 .. 64 and a pad >= 0 per axis");
        if (L.ph >= L.kh || L.pw >= L.kw)
          throw std::runtime_error(who + "pad " + std::to_string(L.ph) + " x " + std::to_string(L.pw) + " must be smaller than the kernel " +
                                   std::to_string(L.kh) + " x " + std::to_string(L.kw) + " (pad < kernel per axis)");
        L.k = L.kh; L.stride = L.sh; L.pad = L.ph;   // (the square case: what the convolution's fold and maxpool_kernel read)
      }
      if (L.bottoms[0] == L.tops[0]) throw std::runtime_error(who + "cannot run in place on '" + blobs[L.tops[0]].name + "'");
      if (std::count(inputs.begin(), inputs.end(), L.bottoms[0]))
        throw std::runtime_error(who + "bottom '" + blobs[L.bottoms[0]].name + "' is a net input: the layer reads NHWC activations, put a "
                                 "convolution in between");
      L.op = OP_POOL;
    } else if (L.type == "Python") {
      const PMsg* py = L.msg->sub("python_param");
      if (!py || py->str("layer") != "ProposalLayer")
        throw std::runtime_error("Python layer '" + L.name + "': only ProposalLayer has a native implementation");
      L.op = OP_TAIL;
      tail_layer = (int)li;
      mods.emplace_back();
      mods.back().layer = (int)li;
    } else if (L.type == "Concat") {
      // ConcatLayer::LayerSetUp / Reshape (concat_layer.cpp:10-30): `concat_dim` is the legacy spelling of `axis` (never
      // negative), giving both is an error; a negative axis counts from the end of the 4-D blob
      const std::string who = "Concat '" + L.name + "': ";
      const PMsg* cc = L.msg->sub("concat_param");
      const bool has_dim = cc && cc->get("concat_dim"), has_axis = cc && cc->get("axis");
      if (has_dim && has_axis) throw std::runtime_error(who + "both axis and concat_dim given: it is one or the other");
      int axis = has_dim ? geti(cc, "concat_dim", 1) : geti(cc, "axis", 1);
      if (has_dim && axis < 0) throw std::runtime_error(who + "concat_dim " + std::to_string(axis) + " must not be negative");
      if (axis < 0) axis += 4;
      if (axis < 0 || axis > 3)
        throw std::runtime_error(who + (has_dim ? "concat_dim " : "axis ") + std::to_string(geti(cc, has_dim ? "concat_dim" : "axis", 1)) +
                                 " is outside a 4-D blob");
      if (L.bottoms.empty() || L.tops.size() != 1) throw std::runtime_error(who + "takes at least one bottom and exactly one top");
      L.concat_axis = axis;
      L.op = OP_SKIP;
    } else if (L.type == "Softmax" || L.type == "Reshape" || L.type == "Split" || L.type == "Input") {
      // (the proposal tail computes the Softmax over the class planes that its Reshapes lay out: axis 1 of the 4-D score
      // blob, and a Reshape of the whole shape -- softmax_layer.cpp:12-16, reshape_layer.cpp:10-60)
      if (L.type == "Softmax") {
        const int axis = geti(L.msg->sub("softmax_param"), "axis", 1);
        if (axis != 1 && axis != -3)
          throw std::runtime_error("Softmax '" + L.name + "': axis " + std::to_string(axis) + ": only the softmax over axis 1 is supported");
      }
      if (L.type == "Reshape") {
        const PMsg* rp = L.msg->sub("reshape_param");
        if (geti(rp, "axis", 0) != 0 || geti(rp, "num_axes", -1) != -1)
          throw std::runtime_error("Reshape '" + L.name + "': axis " + std::to_string(geti(rp, "axis", 0)) + " / num_axes " +
                                   std::to_string(geti(rp, "num_axes", -1)) + ": only a reshape of the whole blob (axis 0, num_axes -1) is supported");
      }
      L.op = OP_SKIP;
    } else {
      throw std::runtime_error("Unsupported layer type '" + L.type + "' (layer '" + L.name + "')");
    }
    for (int t : L.tops) producer[t] = (int)li;
  }

  // ---- the fused tails: walk back from every proposal layer
  std::map<int, int> fused_by;   // layer folded into a tail -> its module
  if ((int)mods.size() > kMaxModules) {
    std::string names;
    for (auto& M : mods) names += (names.empty() ? "'" : ", '") + layers[M.layer].name + "'";
    throw std::runtime_error(std::to_string(mods.size()) + " ProposalLayers (" + names + "): a net holds at most " +
                             std::to_string(kMaxModules) + " proposal modules");
  }
  for (int mj = 0; mj < (int)mods.size(); ++mj) {
    const std::string lname = "'" + layers[mods[mj].layer].name + "'";
    try {
      build_module(mj, producer, fused_by);
    } catch (const std::runtime_error& e) {   // (every refusal of the walk names its module's layer)
      const std::string what = e.what();
      if (what.find(lname) != std::string::npos) throw;
      throw std::runtime_error(what + " (ProposalLayer " + lname + ")");
    }
    for (int q = 0; q < mj; ++q)
      for (int t : layers[mods[q].layer].tops)
        for (int u : layers[mods[mj].layer].tops)
          if (t == u)
            throw std::runtime_error("ProposalLayers '" + layers[mods[q].layer].name + "' and " + lname + " write the same top '" +
                                     blobs[t].name + "'");
  }
  // ---- channel-concat views (zero-copy): bottoms of a non-fused axis-1 Concat live inside the top
  for (size_t li = 0; li < layers.size(); ++li) {
    Layer& L = layers[li];
    if (L.type != "Concat" || fused_by.count((int)li)) continue;
    if (L.concat_axis != 1)
      throw std::runtime_error("Concat '" + L.name + "': axis " + std::to_string(L.concat_axis) + ": only channel concat (axis 1) is supported outside the tail");
    // Caffe's Concat copies: its bottoms keep their values when a later in-place ReLU rewrites the top.  As views they would
    // be rewritten with it, so such a Concat copies here too (one combine launch per member, the ReLU applied on the way
    // when it comes directly behind) and its members keep their own buffers.
    int rewriter = -1;
    for (size_t lj = li + 1; lj < layers.size() && rewriter < 0; ++lj) {
      const Layer& Q = layers[lj];
      if ((Q.op == OP_RELU || Q.op == OP_NORM || Q.op == OP_L2NORM || Q.op == OP_NEURON) && Q.bottoms[0] == Q.tops[0] && Q.tops[0] == L.tops[0])
        rewriter = (int)lj;
    }
    if (rewriter >= 0) {
      for (int b : L.bottoms)
        if (std::count(inputs.begin(), inputs.end(), b))
          throw std::runtime_error("Concat '" + L.name + "': bottom '" + blobs[b].name + "' is a net input and the top is rewritten "
                                   "in place by " + layers[rewriter].type + " '" + layers[rewriter].name + "': the copy reads NHWC activations");
      L.op = OP_CONCAT_COPY;
      continue;
    }
    for (int b : L.bottoms) {
      if (blobs[b].owner >= 0 || std::count(inputs.begin(), inputs.end(), b))
        throw std::runtime_error("Concat '" + L.name + "': bottom already aliased");
      blobs[b].owner = L.tops[0];
    }
  }
  // ---- what the combine launches read is a plain fp32 NHWC activation (not a blob of a proposal tail)
  for (const Layer& L : layers) {
    if (L.op != OP_ELTWISE && L.op != OP_CROP && L.op != OP_RELU && L.op != OP_CONCAT_COPY && L.op != OP_NORM && L.op != OP_L2NORM &&
        L.op != OP_POOL && L.op != OP_NEURON)
      continue;
    for (int b : L.bottoms)
      if (blobs[b].kind != BK_NHWC)
        throw std::runtime_error(L.type + " '" + L.name + "': bottom '" + blobs[b].name + "' is not an NHWC activation (it belongs to "
                                 "a proposal tail)");
  }
  // ---- folds of the combine launches.  An in-place ReLU directly behind an Eltwise, a Crop or a copying Concat (nothing
  //      reads the blob in between) is applied in that layer's launch: behind the Concat always (the two ARE one launch per
  //      member), behind the other two on the fused path.  A Crop whose only reader is an Eltwise, and which is no net
  //      output, is read through its offsets by that Eltwise on the fused path and never written.
  for (size_t li = 0; li < layers.size(); ++li) {
    Layer& R = layers[li];
    if ((R.op != OP_RELU && R.op != OP_NORM && R.op != OP_L2NORM && R.op != OP_NEURON) || R.bottoms[0] != R.tops[0]) continue;
    const int x = R.tops[0];
    if (blobs[x].owner >= 0)   // a member of a zero-copy Concat: rewriting it AFTER the Concat would rewrite the Concat's top
      for (size_t lc = 0; lc < li; ++lc)
        if (layers[lc].type == "Concat" && !layers[lc].tops.empty() && layers[lc].tops[0] == blobs[x].owner)
          throw std::runtime_error(R.type + " '" + R.name + "': rewrites '" + blobs[x].name + "' in place after Concat '" + layers[lc].name +
                                   "' has taken it as a bottom (the Concat's top is a view of its bottoms here)");
    if (R.op == OP_NORM) continue;   // (their chains and folds: plan_norm_layers)
    if (R.op == OP_L2NORM || R.op == OP_NEURON) continue;   // (a launch of its own, never folded)
    int prod = -1;
    bool read_between = false;
    for (int lj = (int)li - 1; lj >= 0 && prod < 0; --lj) {
      if (std::count(layers[lj].tops.begin(), layers[lj].tops.end(), x)) prod = lj;
      else if (std::count(layers[lj].bottoms.begin(), layers[lj].bottoms.end(), x)) read_between = true;
    }
    if (prod < 0 || read_between || layers[prod].fold_relu >= 0) continue;
    const OpType po = layers[prod].op;
    if (po != OP_ELTWISE && po != OP_CROP && po != OP_CONCAT_COPY) continue;
    layers[prod].fold_relu = (int)li;
    R.folded_into = prod;
  }
  for (size_t li = 0; li < layers.size(); ++li) {
    Layer& C = layers[li];
    if (C.op != OP_CROP || std::count(outputs.begin(), outputs.end(), C.tops[0])) continue;
    int reader = -1, readers = 0;
    for (size_t lj = 0; lj < layers.size(); ++lj)
      if (lj != li && std::count(layers[lj].bottoms.begin(), layers[lj].bottoms.end(), C.tops[0])) { ++readers; reader = (int)lj; }
    if (readers != 1 || reader < (int)li || layers[reader].op != OP_ELTWISE) continue;
    bool source_rewritten = false;   // (an in-place layer on the Crop's bottom between the two: the Eltwise would read the new values)
    for (int lj = (int)li + 1; lj < reader; ++lj)
      source_rewritten = source_rewritten || std::count(layers[lj].tops.begin(), layers[lj].tops.end(), C.bottoms[0]) > 0;
    if (!source_rewritten) C.folded_into = reader;
  }

  // ---- params (shapes need channel counts: run shape inference once)
  infer_shapes();
  // the per-head tail packs Cf weights per row from every head's predictors and reads Cf channels of every head blob at the
  // first one's map size (build_tail_weights, tail_logits_kernel): heads of another shape would be read out of bounds
  for (const TailModule& M : mods) {
    const std::vector<int>& s0 = blobs[M.feat_blobs[0]].shape;
    if (s0.size() != 4)
      throw std::runtime_error("ProposalLayer '" + layers[M.layer].name + "': head blob '" + blobs[M.feat_blobs[0]].name + "' is not 4-D");
    for (int fb : M.feat_blobs) {
      const std::vector<int>& s = blobs[fb].shape;
      if (s.size() != 4 || s[1] != s0[1])
        throw std::runtime_error("ProposalLayer '" + layers[M.layer].name + "': head blobs '" + blobs[M.feat_blobs[0]].name +
                                 "' and '" + blobs[fb].name + "' differ in channel count (" + std::to_string(s0[1]) + " vs " +
                                 std::to_string(s.size() == 4 ? s[1] : 0) + "): the per-head predictors must read heads of one width");
      if (s[2] != s0[2] || s[3] != s0[3])
        throw std::runtime_error("ProposalLayer '" + layers[M.layer].name + "': head blobs '" + blobs[M.feat_blobs[0]].name +
                                 "' and '" + blobs[fb].name + "' differ in map size");
    }
  }
  for (size_t li = 0; li < layers.size(); ++li) {
    Layer& L = layers[li];
    const bool l2 = L.type == "Normalize", prelu = L.type == "PReLU";
    const bool norm = L.type == "BatchNorm" || L.type == "Scale" || l2 || prelu;
    if (L.type != "Convolution" && L.type != "Deconvolution" && !norm) continue;
    const int cin = blobs[L.bottoms[0]].shape[1];
    std::vector<std::vector<int>> shapes;
    float fill = 0.f;
    if (l2) {
      // Normalize: the scale, (C) or with channel_shared a blob of 0 axes and one value (normalize_layer.cpp:36-41), from its filler
      shapes.push_back(L.l2_shared ? std::vector<int>() : std::vector<int>{cin});
      fill = L.l2_fill;
    } else if (prelu) {
      // PReLU: the slopes, (C) or with channel_shared a blob of 0 axes and one value (prelu_layer.cpp:22-37), from its filler
      shapes.push_back(L.prelu_shared ? std::vector<int>() : std::vector<int>{cin});
      fill = L.prelu_fill;
    } else if (norm) {
      // BatchNorm: mean (C), variance (C), the moving-average factor (1), zero as Caffe creates them; Scale: gamma (C) from
      // the default filler, the constant 1, and with bias_term beta (C), zero
      if (L.is_bn) shapes = {{cin}, {cin}, {1}};
      else {
        shapes.push_back({cin});
        if (L.bias_term) shapes.push_back({cin});
        fill = 1.f;
      }
    } else if (L.type == "Convolution") {
      // group 1, or depthwise: group == bottom channels, num_output a multiple of them (Layer setup checked that group divides
      // num_output); the blob is (Cout, Cin / group, k, k) as Caffe shapes it
      if (L.group != 1) {
        if (L.group != cin)
          throw std::runtime_error("Convolution '" + L.name + "': group != 1 unsupported unless depthwise (group == bottom channels); got group " +
                                   std::to_string(L.group) + " of " + std::to_string(cin));
        if (blobs[L.bottoms[0]].kind == BK_INPUT_NCHW)
          throw std::runtime_error("Convolution '" + L.name + "': depthwise (group " + std::to_string(L.group) + ") on bottom '" +
                                   blobs[L.bottoms[0]].name + "', a net input: the layer reads NHWC activations, put a convolution in between");
        if (fused_by.count((int)li))
          throw std::runtime_error("Convolution '" + L.name + "': depthwise (group " + std::to_string(L.group) + ") as a predictor of ProposalLayer '" +
                                   layers[mods[fused_by[(int)li]].layer].name + "': the tail's combined weight matrix takes dense predictors");
      }
      shapes.push_back({L.nout, cin / L.group, L.k, L.k});
    } else {
      if (L.group != cin || L.nout != cin)
        throw std::runtime_error("Deconvolution '" + L.name + "': only depthwise (group == channels) is supported");
      shapes.push_back({cin, 1, L.k, L.k});
    }
    if (!norm && L.bias_term) shapes.push_back({L.nout});
    auto pspecs = L.msg->all("param");
    for (size_t pi = 0; pi < shapes.size(); ++pi) {
      std::string pname = (pi < pspecs.size() && pspecs[pi]->msg) ? pspecs[pi]->msg->str("name") : "";
      std::shared_ptr<ParamBlob> pb;
      if (clone_src) {
        pb = clone_src->layers[li].params[pi];
      } else if (!pname.empty() && shared_params.count(pname)) {
        pb = shared_params[pname];
        if (pb->shape != shapes[pi]) throw std::runtime_error("Shared parameter '" + pname + "' shape mismatch");
      } else {
        pb = std::make_shared<ParamBlob>();
        pb->shape = shapes[pi];
        pb->host.assign(pb->count(), pi == 0 ? fill : 0.f);
        if (!pname.empty()) shared_params[pname] = pb;
      }
      L.params.push_back(pb);
    }
    if (L.type == "Convolution")
      // (class 3, the general geometry: any stride / pad / kernel outside the "same" family -- no fused pool, no fused first
      // pair, no split-format input or output: each of those plans asks for class 0 or 1)
      // (class 4, depthwise: likewise none of those plans, whatever its geometry)
      L.kclass = L.group != 1 ? kConvClassDepthwise
                              : conv_kernel_class(cin, L.nout, L.k, L.pad, L.dil, blobs[L.bottoms[0]].kind == BK_INPUT_NCHW, L.stride);
  }
  plan_norm_layers(fused_by);
  // ---- conv -> MAX 2x2/2 pool pairs that the fused (detect) path runs as one kernel
  for (size_t li = 0; li < layers.size(); ++li) {
    Layer& P = layers[li];
    if (P.op != OP_POOL || P.k != 2 || P.stride != 2 || P.pad != 0) continue;
    // ... MAX, square, not global: the epilogue takes a maximum over 2 x 2 (an AVE 2x2/2 must not be folded into it)
    if (P.pool_method != POOL_MAX || P.global_pool || P.kh != P.kw || P.sh != P.sw || P.ph != P.pw) continue;
    const int x = P.bottoms[0];
    int prod = -1, others = 0;
    for (size_t lj = 0; lj < layers.size(); ++lj) {
      if (lj == li) continue;
      Layer& Q = layers[lj];
      if (Q.type == "Convolution" && !Q.tops.empty() && Q.tops[0] == x) prod = (int)lj;
      if (Q.op == OP_SKIP && (Q.type == "ReLU" || Q.norm_conv >= 0)) continue;  // the in-place ReLU (and a folded BatchNorm / Scale) is part of the conv
      for (int bb : Q.bottoms)
        if (bb == x) ++others;
    }
    if (prod < 0 || layers[prod].op != OP_CONV || layers[prod].kclass != 0 || !layers[prod].relu) continue;
    if (blobs[x].owner >= 0 || blobs[P.tops[0]].owner >= 0) continue;
    // a layer between the two that rewrites x in place with a launch of its own (a BatchNorm / Scale that did not fold, a
    // ReLU that is not the convolution's epilogue): the pool must read the rewritten values, the epilogue would pool the
    // convolution's own
    bool rewritten = false;
    for (size_t lj = (size_t)prod + 1; lj < li; ++lj)
      rewritten = rewritten || (layers[lj].op != OP_SKIP && std::count(layers[lj].tops.begin(), layers[lj].tops.end(), x) > 0);
    if (rewritten) continue;
    layers[prod].fuse_pool = (int)li;
    layers[prod].pool_only = (others == 0);
    P.fused_into = prod;
  }
  // ---- first-layer conv (on the raw image) that the split-fp16 kernel of the NEXT conv can compute in place
  for (size_t li = 0; li < layers.size(); ++li) {
    Layer& F = layers[li];
    if (F.op != OP_CONV || F.kclass != 1 || !F.relu || F.k != 3 || F.pad != 1 || F.dil != 1 || F.nout != 64) continue;
    if (blobs[F.bottoms[0]].shape.size() != 4 || blobs[F.bottoms[0]].shape[1] != 3) continue;
    const int x = F.tops[0];
    int next = -1, readers = 0;
    for (size_t lj = 0; lj < layers.size(); ++lj) {
      Layer& Q = layers[lj];
      if (lj == li || (Q.op == OP_SKIP && (Q.type == "ReLU" || Q.norm_conv >= 0))) continue;
      for (int bb : Q.bottoms)
        if (bb == x) { ++readers; next = (int)lj; }
    }
    if (readers != 1 || layers[next].op != OP_CONV || layers[next].kclass != 0) continue;
    Layer& N = layers[next];
    if (N.k != 3 || N.dil != 1 || !conv_f16x3_eligible(64, N.nout, N.k, N.pad, N.dil) || blobs[x].owner >= 0) continue;
    N.first_src = (int)li;
    F.first_dst = next;
  }
  // ---- dilation-1 / 2 / 4 convolutions over one bottom with shared parameter blobs: the shared-weight heads
  for (size_t li = 0; li < layers.size(); ++li) {
    Layer& A = layers[li];
    if (A.op != OP_CONV || A.kclass != 0 || A.k != 3 || A.dil != 1 || A.pad != 1 || A.nout != 128 || A.params.empty() ||
        A.fuse_pool >= 0 || A.first_src >= 0)
      continue;
    int d2 = -1, d4 = -1;
    for (size_t lj = li + 1; lj < layers.size(); ++lj) {
      Layer& Q = layers[lj];
      if (Q.op != OP_CONV || Q.kclass != 0 || Q.k != 3 || Q.pad != Q.dil || Q.nout != A.nout || Q.bottoms[0] != A.bottoms[0] ||
          Q.params.size() != A.params.size() || Q.relu != A.relu || Q.fuse_pool >= 0)
        continue;
      bool same = true;
      for (size_t pi = 0; pi < A.params.size(); ++pi) same = same && Q.params[pi] == A.params[pi];
      if (!same) continue;
      if (Q.dil == 2 && d2 < 0) d2 = (int)lj;
      if (Q.dil == 4 && d4 < 0) d4 = (int)lj;
    }
    if (d2 < 0 || d4 < 0) continue;
    if (layers[d2].heads3_lead >= 0 || layers[d4].heads3_lead >= 0 || layers[d2].heads3_d2 >= 0 || layers[d4].heads3_d2 >= 0)
      continue;   // a sibling already claimed by another dilation-1 layer
    // the fused launch writes the siblings' tops at THIS layer's place in the schedule: legal only when nothing in between
    // reads or writes those tops, and nothing in between (or the siblings' own in-place ReLUs aside) rewrites the shared bottom
    bool safe = true;
    const int t2 = layers[d2].tops[0], t4 = layers[d4].tops[0], shared_bottom = A.bottoms[0];
    for (int lj = (int)li + 1; lj < std::max(d2, d4) && safe; ++lj) {
      if (lj == d2 || lj == d4) continue;
      const Layer& Q = layers[lj];
      // (the three convs' own in-place ReLUs are folded into them: Layer::relu)
      if (Q.op == OP_SKIP && Q.type == "ReLU" && Q.bottoms.size() == 1 && Q.tops.size() == 1 && Q.bottoms[0] == Q.tops[0] &&
          (Q.tops[0] == A.tops[0] || Q.tops[0] == t2 || Q.tops[0] == t4))
        continue;
      for (int bb : Q.bottoms) safe = safe && bb != t2 && bb != t4;
      for (int tt : Q.tops) safe = safe && tt != t2 && tt != t4 && tt != shared_bottom;
    }
    if (!safe) continue;
    A.heads3_d2 = d2;
    A.heads3_d4 = d4;
    layers[d2].heads3_lead = layers[d4].heads3_lead = (int)li;
  }
  // ---- blobs the fused split-fp16 path keeps in the pre-split activation format: produced by a split-fp16 conv
  //      (or by the pool fused into its epilogue) and read ONLY by convs that run on the 4-wave kernel
  {
    // (plan_conv's shape-only half, conv_f16x3_family_shape: what a reader writes -- its top and the top of a pool fused into
    // it -- must be a 16-byte aligned channel view; the launch-time half -- an input of 4 GiB or more -- fails the launch with
    // the layer's name)
    auto aligned_view = [&](int bi_) {
      const Blob& b_ = blobs[bi_];
      const Blob& ob_ = blobs[b_.owner >= 0 ? b_.owner : bi_];
      return ob_.shape.size() == 4 && ob_.shape[1] % 4 == 0 && b_.coff % 4 == 0;
    };
    auto w4_reader = [&](const Layer& Q, int cin) {
      if (Q.op != OP_CONV || Q.kclass != 0 || Q.first_src >= 0 || Q.tops.empty()) return false;
      const bool pool = Q.fuse_pool >= 0;
      const bool aligned = aligned_view(Q.tops[0]) && (!pool || aligned_view(layers[Q.fuse_pool].tops[0]));
      return conv_f16x3_family_shape(cin, Q.nout, Q.k, Q.pad, Q.dil, pool, aligned);
    };
    for (size_t bi = 0; bi < blobs.size() && conv_knobs().split_act; ++bi) {
      Blob& B = blobs[bi];
      if (B.owner >= 0 || B.kind != BK_NHWC || B.shape.size() != 4) continue;
      if (is_feat_blob((int)bi)) continue;
      bool concat_member = false;
      for (auto& O : blobs) concat_member = concat_member || O.owner == (int)bi;
      if (concat_member) continue;
      // producer: a kclass-0 conv eligible for a split-fp16 kernel, directly or through its fused pool
      int prod = -1;
      for (size_t lj = 0; lj < layers.size(); ++lj) {
        Layer& Q = layers[lj];
        if (Q.op == OP_CONV && Q.kclass == 0 && !Q.tops.empty() && Q.tops[0] == (int)bi) prod = (int)lj;
        if (Q.op == OP_POOL && Q.fused_into >= 0 && !Q.tops.empty() && Q.tops[0] == (int)bi) prod = Q.fused_into;
      }
      if (prod < 0) continue;
      const Layer& Pq = layers[prod];
      const int pcin = blobs[Pq.bottoms[0]].shape.size() == 4 ? blobs[Pq.bottoms[0]].shape[1] : 0;
      if (!conv_f16x3_eligible(Pq.first_src >= 0 ? 64 : pcin, Pq.nout, Pq.k, Pq.pad, Pq.dil)) continue;
      int readers = 0;
      bool all_w4 = true;
      for (size_t lj = 0; lj < layers.size(); ++lj) {
        Layer& Q = layers[lj];
        if (Q.op == OP_SKIP && (Q.type == "ReLU" || Q.norm_conv >= 0)) continue;   // in-place, part of the conv
        if (Q.op == OP_POOL && Q.fused_into >= 0 && Q.bottoms[0] == (int)bi) continue;  // folded into the producer
        for (int bb : Q.bottoms)
          if (bb == (int)bi) {
            ++readers;
            all_w4 = all_w4 && w4_reader(Q, B.shape[1]);
          }
      }
      B.split_fused = readers > 0 && all_w4;
    }
  }
  // ---- Softmax, Reshape and Split have no launch of their own: inside a tail the tail computes them, outside one their top
  //      would be a buffer that nothing writes.  (Checked last: what another layer refuses about the graph is said first.)
  for (size_t li = 0; li < layers.size(); ++li) {
    const Layer& L = layers[li];
    if ((L.type == "Softmax" || L.type == "Reshape" || L.type == "Split") && !fused_by.count((int)li))
      throw std::runtime_error(L.type + " '" + L.name + "': the layer type exists only inside a proposal tail (between the predictors "
                               "and a ProposalLayer); this one feeds none");
  }
  alloc_buffers();
  amax_slots.ensure(std::max<size_t>(blobs.size(), 1) * 4);
  fill_now(amax_slots.p, 0, std::max<size_t>(blobs.size(), 1) * 4);
  if (clone_src) {
    wgen = clone_src->wgen;
    return;
  }
  if (caffemodel && caffemodel[0]) load_caffemodel(caffemodel);
  for (size_t li = 0; li < layers.size(); ++li)
    if (layers[li].norm_conv < 0) commit_params((int)li);   // (a folded BatchNorm / Scale: its convolution's commit read its blobs)
}

void shf_net::infer_shapes() {
  // (a refusal below leaves some blobs at the refused input's shapes: whatever the next forward's input, it infers again)
  last_data_shape.clear();
  for (auto& L : layers) {
    if (L.type == "Input") continue;
    auto& bs = blobs[L.bottoms.empty() ? 0 : L.bottoms[0]].shape;
    if (L.type == "Convolution") {
      if (bs.size() != 4) throw std::runtime_error("Convolution '" + L.name + "': 4-D bottom expected");
      // BaseConvolutionLayer::compute_output_shape (base_conv_layer.cpp:17-29) would give a size <= 0: only a layer of the
      // general geometry can get here (3x3 pad == dilation and 1x1 pad 0 keep the map's size)
      const int kext = L.dil * (L.k - 1) + 1;
      if (kext > bs[2] + 2 * L.pad || kext > bs[3] + 2 * L.pad)
        throw std::runtime_error("Convolution '" + L.name + "': kernel extent " + std::to_string(kext) + " (dilation * (kernel_size - 1) + 1) exceeds "
                                 "the padded input " + std::to_string(bs[2] + 2 * L.pad) + " x " + std::to_string(bs[3] + 2 * L.pad) +
                                 " of bottom '" + blobs[L.bottoms[0]].name + "'");
      blobs[L.tops[0]].shape = {bs[0], L.nout, conv_out(bs[2], L.k, L.pad, L.stride, L.dil),
                                conv_out(bs[3], L.k, L.pad, L.stride, L.dil)};
    } else if (L.type == "Deconvolution") {
      blobs[L.tops[0]].shape = {bs[0], L.nout, L.stride * (bs[2] - 1) + L.k - 2 * L.pad,
                                L.stride * (bs[3] - 1) + L.k - 2 * L.pad};
    } else if (L.type == "Eltwise") {
      // EltwiseLayer::Reshape (eltwise_layer.cpp:32-40): every bottom has the first one's shape
      if (bs.size() != 4)
        throw std::runtime_error("Eltwise '" + L.name + "': bottom '" + blobs[L.bottoms[0]].name + "' is not 4-D");
      for (int b : L.bottoms)
        if (blobs[b].shape != bs) {
          auto txt = [](const std::vector<int>& s) {
            std::string o = "(";
            for (size_t i = 0; i < s.size(); ++i) o += (i ? ", " : "") + std::to_string(s[i]);
            return o + ")";
          };
          throw std::runtime_error("Eltwise '" + L.name + "': bottoms '" + blobs[L.bottoms[0]].name + "' " + txt(bs) + " and '" +
                                   blobs[b].name + "' " + txt(blobs[b].shape) + " differ in shape");
        }
      blobs[L.tops[0]].shape = bs;
    } else if (L.type == "Crop") {
      // CropLayer::Reshape (crop_layer.cpp:36-78): axes from `axis` on take the second bottom's size, from the offset
      const std::vector<int>& rs = blobs[L.bottoms[1]].shape;
      for (int b : L.bottoms)
        if (blobs[b].shape.size() != 4)
          throw std::runtime_error("Crop '" + L.name + "': bottom '" + blobs[b].name + "' is not 4-D");
      std::vector<int> s = bs;
      for (int ax = 0; ax < 4; ++ax) {
        int off = 0;
        if (ax >= L.crop_axis) {
          s[ax] = rs[ax];
          if (L.crop_offsets.size() == 1) off = L.crop_offsets[0];
          else if (L.crop_offsets.size() > 1) off = L.crop_offsets[ax - L.crop_axis];
          if (off < 0 || (long long)off + rs[ax] > bs[ax])
            throw std::runtime_error("Crop '" + L.name + "': axis " + std::to_string(ax) + ": size " + std::to_string(rs[ax]) +
                                     " at offset " + std::to_string(off) + " exceeds the " + std::to_string(bs[ax]) + " of bottom '" +
                                     blobs[L.bottoms[0]].name + "'");
        }
        L.crop_origin[ax] = off;
      }
      blobs[L.tops[0]].shape = s;
    } else if (L.type == "BatchNorm" || L.type == "Scale") {
      // per channel of a 4-D blob (batch_norm_layer.cpp:52-80; scale_layer.cpp:62-100 with axis 1, num_axes 1)
      if (bs.size() != 4)
        throw std::runtime_error(L.type + " '" + L.name + "': bottom '" + blobs[L.bottoms[0]].name + "' is not 4-D");
      blobs[L.tops[0]].shape = bs;
    } else if (L.type == "Normalize") {
      // per pixel of a 4-D blob, over its channels (normalize_layer.cpp:64-82)
      if (bs.size() != 4)
        throw std::runtime_error("Normalize '" + L.name + "': bottom '" + blobs[L.bottoms[0]].name + "' is not 4-D");
      blobs[L.tops[0]].shape = bs;
    } else if (L.op == OP_NEURON) {
      // elementwise on a 4-D blob (neuron_layer.cpp:7-11: the top takes the bottom's shape)
      if (bs.size() != 4)
        throw std::runtime_error(L.type + " '" + L.name + "': bottom '" + blobs[L.bottoms[0]].name + "' is not 4-D");
      blobs[L.tops[0]].shape = bs;
    } else if (L.type == "ReLU" || L.type == "Softmax" || L.type == "Split") {
      if (L.op == OP_RELU && bs.size() != 4)
        throw std::runtime_error("ReLU '" + L.name + "': bottom '" + blobs[L.bottoms[0]].name + "' is not 4-D");
      for (int t : L.tops) blobs[t].shape = bs;
    } else if (L.type == "Pooling") {
      // PoolingLayer::Reshape (pooling_layer.cpp:79-123): ceil sizing per axis; with a pad on either axis the last window of
      // BOTH axes must start inside the image or its padding, else it is dropped.  Global: the window is the bottom's H x W
      if (bs.size() != 4)
        throw std::runtime_error("Pooling '" + L.name + "': bottom '" + blobs[L.bottoms[0]].name + "' is not 4-D");
      if (L.global_pool) {
        L.kh = bs[2];
        L.kw = bs[3];
      }
      int ho = (int)std::ceil((bs[2] + 2 * L.ph - L.kh) / (double)L.sh) + 1;
      int wo = (int)std::ceil((bs[3] + 2 * L.pw - L.kw) / (double)L.sw) + 1;
      if (L.ph || L.pw) {
        if ((ho - 1) * L.sh >= bs[2] + L.ph) --ho;
        if ((wo - 1) * L.sw >= bs[3] + L.pw) --wo;
      }
      if (ho < 1 || wo < 1)
        throw std::runtime_error("Pooling '" + L.name + "': kernel " + std::to_string(L.kh) + " x " + std::to_string(L.kw) + " exceeds the padded "
                                 "input of bottom '" + blobs[L.bottoms[0]].name + "'");
      blobs[L.tops[0]].shape = {bs[0], bs[1], ho, wo};
    } else if (L.type == "Concat") {
      const int axis = L.concat_axis;
      std::vector<int> s = bs;
      int sum = 0;
      int off = 0;
      for (int b : L.bottoms) {
        if (blobs[b].owner == L.tops[0]) blobs[b].coff = off;
        off += blobs[b].shape[axis];
        sum += blobs[b].shape[axis];
      }
      s[axis] = sum;
      blobs[L.tops[0]].shape = s;
    } else if (L.type == "Reshape") {
      const PMsg* rp = L.msg->sub("reshape_param");
      std::vector<int> dims;
      if (rp && rp->sub("shape"))
        for (auto d : rp->sub("shape")->all("dim")) dims.push_back(atoi(d->scalar.c_str()));
      std::vector<int> out;
      int infer = -1;
      long total = 1, known = 1;
      for (int d : bs) total *= d;
      for (size_t i = 0; i < dims.size(); ++i) {
        if (dims[i] == 0) out.push_back(bs[i]);
        else if (dims[i] == -1) { infer = (int)i; out.push_back(1); }
        else out.push_back(dims[i]);
      }
      for (int d : out) known *= d;
      if (infer >= 0) out[infer] = (int)(total / std::max<long>(known, 1));
      blobs[L.tops[0]].shape = out;
    } else if (L.type == "Python") {
      if (blobs[L.tops[0]].shape.size() != 2) blobs[L.tops[0]].shape = {1, 5};
      if (L.tops.size() > 1 && blobs[L.tops[1]].shape.size() != 2) blobs[L.tops[1]].shape = {1, tail_C};
    }
  }
  if (data_blob >= 0) last_data_shape = blobs[data_blob].shape;
}

void shf_net::alloc_buffers() {
  for (size_t i = 0; i < blobs.size(); ++i) {
    Blob& b = blobs[i];
    if (b.kind == BK_FUSED) continue;
    if (b.owner >= 0) continue;  // view into a concat buffer
    if (b.kind == BK_FLAT && module_of_output((int)i) >= 0) continue;  // sized by the tail
    b.dev.ensure(std::max<size_t>(b.count(), 1) * sizeof(float));
  }
  for (TailModule& M : mods) {
    Blob& f = blobs[M.feat_blobs[0]];
    ensure_tail_workspace(M, (size_t)f.shape[2] * f.shape[3] * M.A);
  }
}

// module M's tail workspace + proposal output blobs for `total` anchors (grow-only)
void shf_net::ensure_tail_workspace(TailModule& M, size_t total) {
  size_t npad = 1;
  while (npad < total) npad <<= 1;
  const size_t rec = (size_t)tail_C + 4;   // floats per anchor: the class scores and four box values
  M.tw_logits.ensure(total * rec * 4);
  M.tw_rec.ensure(total * rec * 4);
  M.tw_keys.ensure(std::max<size_t>(npad, 16384) * 8);
  M.tw_counters.ensure(64);
  TailWork& tw = M.tw;
  tw.logits = (float*)M.tw_logits.p;
  tw.rec = (float*)M.tw_rec.p;
  tw.keys = (unsigned long long*)M.tw_keys.p;
  tw.counters = (int*)M.tw_counters.p;
  // (the tail's reset kernel zeroes the lane's slots for the next pass: once per lane, so the first module's entry carries them)
  tw.amax = fp16_mode() && &M == &mods[0] ? (unsigned*)amax_slots.p : nullptr;
  tw.n_amax = (int)blobs.size();
  tw.cap_anchors = total;
  tw.cap_keys = npad;
  const size_t rmax = (pre_nms_topN > 0) ? std::min<size_t>(total, (size_t)pre_nms_topN) : total;
  blobs[M.boxes_blob].dev.ensure(std::max<size_t>(rmax, 1) * 5 * 4);
  if (M.prob_blob >= 0) blobs[M.prob_blob].dev.ensure(std::max<size_t>(rmax, 1) * tail_C * 4);
}

void shf_net::build_tail_weights(TailModule& M) {
  M.Cf = blobs[M.feat_blobs[0]].shape[1];
  const int A = M.A, Cf = M.Cf, NC = tail_C, NO = tail_C + 4;
  std::vector<float> W((size_t)A * NO * Cf, 0.f), B((size_t)A * NO, 0.f);
  for (int a = 0; a < A; ++a) {
    const int h = M.heads == 1 ? 0 : a;
    Layer& c = layers[M.cls_layers[h]];
    Layer& b = layers[M.box_layers[h]];
    const float* cw = c.params[0]->host.data();
    const float* bw = b.params[0]->host.data();
    const float* cb = c.params.size() > 1 ? c.params[1]->host.data() : nullptr;
    const float* bb = b.params.size() > 1 ? b.params[1]->host.data() : nullptr;
    for (int cls = 0; cls < NC; ++cls) {
      // plain template: cls_score channel = cls*A + a (Reshape (0,C,-1,0)); dilation template: channel = cls
      const int row = M.heads == 1 ? cls * A + a : cls;
      memcpy(&W[((size_t)a * NO + cls) * Cf], cw + (size_t)row * Cf, Cf * sizeof(float));
      B[a * NO + cls] = cb ? cb[row] : 0.f;
    }
    for (int j = 0; j < 4; ++j) {
      const int row = M.heads == 1 ? a * 4 + j : j;
      memcpy(&W[((size_t)a * NO + NC + j) * Cf], bw + (size_t)row * Cf, Cf * sizeof(float));
      B[a * NO + NC + j] = bb ? bb[row] : 0.f;
    }
  }
  M.W.ensure(W.size() * 4);
  M.b.ensure(B.size() * 4);
  HIP_THROW(hipMemcpy(M.W.p, W.data(), W.size() * 4, hipMemcpyHostToDevice));
  HIP_THROW(hipMemcpy(M.b.p, B.data(), B.size() * 4, hipMemcpyHostToDevice));
  M.w_dirty = false;
  M.gen = *wgen;
}

// BatchNorm / Scale: which of them are folded into their producing convolution's parameters, and which run the channel-affine
// kernel (norm.hip), alone or as one launch of an in-place chain.  Runs behind the parameter blobs' creation (a fold needs to
// know who shares them) and before the passes that pair convolutions with pools and first layers (they read Layer::relu).
void shf_net::plan_norm_layers(const std::map<int, int>& fused_by) {
  const int nl = (int)layers.size();
  // the next layer after `from` that has blob x among its bottoms or tops, or -1
  auto next_touch = [&](int from, int x) {
    for (int lj = from + 1; lj < nl; ++lj) {
      const Layer& Q = layers[lj];
      if (std::count(Q.bottoms.begin(), Q.bottoms.end(), x) || std::count(Q.tops.begin(), Q.tops.end(), x)) return lj;
    }
    return -1;
  };
  auto in_place_on = [&](int lj, int x) {
    const Layer& Q = layers[lj];
    return Q.bottoms.size() == 1 && Q.tops.size() == 1 && Q.bottoms[0] == x && Q.tops[0] == x;
  };
  for (int li = 0; li < nl; ++li) {
    Layer& L = layers[li];
    if (L.op == OP_NORM || L.op == OP_L2NORM || L.op == OP_NEURON) L.nv = clone_src ? clone_src->layers[li].nv : std::make_shared<NormVecs>();
  }
  // ---- folds: an in-place BatchNorm, an in-place Scale, or the two in that order, directly on a Convolution's top.  The
  //      convolution is no predictor of a proposal tail and shares its parameter blobs with no other layer (their device
  //      tensors become the effective ones).  A slope-0 in-place ReLU right behind becomes the convolution's epilogue.
  for (int ci = 0; ci < nl; ++ci) {
    Layer& C = layers[ci];
    if (C.op != OP_CONV || C.type != "Convolution" || C.relu || fused_by.count(ci) || C.params.empty()) continue;
    bool shared = false;
    for (int lj = 0; lj < nl && !shared; ++lj)
      if (lj != ci)
        for (auto& q : layers[lj].params)
          for (auto& p : C.params) shared = shared || p == q;
    if (shared) continue;
    const int x = C.tops[0];
    int at = ci;
    for (int stage = 0; stage < 2; ++stage) {   // 0: BatchNorm, 1: Scale
      const int nx = next_touch(at, x);
      if (nx < 0 || layers[nx].op != OP_NORM || !in_place_on(nx, x) || layers[nx].is_bn != (stage == 0)) continue;
      (stage == 0 ? C.fold_bn : C.fold_sc) = nx;
      layers[nx].norm_conv = ci;
      layers[nx].op = OP_SKIP;
      at = nx;
    }
    if (at == ci) continue;
    C.fold_bias = clone_src ? clone_src->layers[ci].fold_bias : std::make_shared<ParamBlob>();
    if (!clone_src) {
      C.fold_bias->shape = {C.nout};
      C.fold_bias->host.assign(C.nout, 0.f);
    }
    const int nx = next_touch(at, x);
    if (nx >= 0 && layers[nx].op == OP_RELU && in_place_on(nx, x) && layers[nx].slope == 0.f && layers[nx].folded_into < 0) {
      C.relu = 1;
      layers[nx].op = OP_SKIP;
    }
  }
  // ---- chains of what is left: consecutive in-place BatchNorm -> Scale -> ReLU on the head's top, nothing reading in between
  for (int li = 0; li < nl; ++li) {
    Layer& Hd = layers[li];
    if (Hd.op != OP_NORM || Hd.folded_into >= 0) continue;
    (Hd.is_bn ? Hd.chain_bn : Hd.chain_sc) = li;
    const int x = Hd.tops[0];
    int at = li;
    for (;;) {
      const int nx = next_touch(at, x);
      if (nx < 0 || !in_place_on(nx, x) || layers[nx].folded_into >= 0) break;
      Layer& Q = layers[nx];
      if (Q.op == OP_NORM && !Q.is_bn && Hd.chain_sc < 0) {   // (a Scale behind the BatchNorm; never a second one, never a BatchNorm behind a Scale)
        Hd.chain_sc = nx;
        Q.folded_into = li;
        at = nx;
        continue;
      }
      if (Q.op == OP_RELU) {
        Hd.chain_relu = nx;
        Q.folded_into = li;
      }
      break;
    }
  }
}

// the per-channel vectors of a BatchNorm / Scale layer on the device, from its fp32 blobs.  BatchNorm in Caffe's operation
// order (batch_norm_layer.cpp:98-105, 117-123): sf = blob2 == 0 ? 0 : 1 / blob2, m = blob0 * sf, d = sqrt(blob1 * sf + eps),
// every step rounded to fp32; for conv mode "f64" the same steps in binary64.
void shf_net::derive_norm(int li) {
  Layer& L = layers[li];
  if (!L.nv) return;   // (folded into a convolution: its commit reads the blobs themselves)
  const size_t C = L.params[0]->count();
  auto up = [&](DevBuf& buf, const void* src, size_t bytes) {
    buf.ensure(bytes);
    HIP_THROW(hipMemcpy(buf.p, src, bytes, hipMemcpyHostToDevice));
  };
  if (L.is_bn) {
    const float* mean = L.params[0]->host.data();
    const float* var = L.params[1]->host.data();
    const float f = L.params[2]->host[0];
    const float sf = f == 0.f ? 0.f : 1.f / f;
    const double sf64 = f == 0.f ? 0.0 : 1.0 / (double)f;
    std::vector<float> m(C), d(C);
    std::vector<double> m64(C), d64(C);
    for (size_t c = 0; c < C; ++c) {
      m[c] = mean[c] * sf;
      const float v = var[c] * sf;
      const float ve = v + L.eps;
      d[c] = std::sqrt(ve);
      m64[c] = (double)mean[c] * sf64;
      d64[c] = std::sqrt((double)var[c] * sf64 + (double)L.eps);
    }
    up(L.nv->m, m.data(), C * 4);
    up(L.nv->d, d.data(), C * 4);
    up(L.nv->m64, m64.data(), C * 8);
    up(L.nv->d64, d64.data(), C * 8);
  } else {
    up(L.nv->g, L.params[0]->host.data(), C * 4);
    if (L.params.size() > 1) up(L.nv->b, L.params[1]->host.data(), C * 4);
  }
}

// W_eff[o, ...] = fp32(W[o, ...] * s[o]), b_eff[o] = fp32((b[o] - blob0[o] * sf) * s[o] + beta[o]) with
// s = gamma / sqrt(blob1 * sf + eps): binary64 from the fp32 blobs, one rounding per value (gamma = 1 without a Scale,
// s = gamma and no mean without a BatchNorm, b = 0 without a bias blob, beta = 0 without bias_term)
void shf_net::fold_conv_params(int li, std::vector<float>& w_eff, std::vector<float>& b_eff) const {
  const Layer& L = layers[li];
  const ParamBlob& w = *L.params[0];
  const int co = w.shape[0];
  const size_t K = w.count() / (size_t)co;
  const Layer* bn = L.fold_bn >= 0 ? &layers[L.fold_bn] : nullptr;
  const Layer* sc = L.fold_sc >= 0 ? &layers[L.fold_sc] : nullptr;
  double sf = 0.0;
  if (bn) {
    const float f = bn->params[2]->host[0];
    sf = f == 0.f ? 0.0 : 1.0 / (double)f;
  }
  w_eff.resize(w.count());
  b_eff.resize(co);
  for (int o = 0; o < co; ++o) {
    const double gamma = sc ? (double)sc->params[0]->host[o] : 1.0;
    const double s = bn ? gamma / std::sqrt((double)bn->params[1]->host[o] * sf + (double)bn->eps) : gamma;
    const double mean = bn ? (double)bn->params[0]->host[o] * sf : 0.0;
    const double b = L.params.size() > 1 ? (double)L.params[1]->host[o] : 0.0;
    const double beta = sc && sc->params.size() > 1 ? (double)sc->params[1]->host[o] : 0.0;
    for (size_t r = 0; r < K; ++r) w_eff[(size_t)o * K + r] = (float)((double)w.host[(size_t)o * K + r] * s);
    b_eff[o] = (float)((b - mean) * s + beta);
  }
}

std::vector<unsigned long long> shf_net::fold_versions(int li) const {
  const Layer& L = layers[li];
  std::vector<unsigned long long> v;
  for (int lj : {li, L.fold_bn, L.fold_sc})
    if (lj >= 0)
      for (auto& p : layers[lj].params) v.push_back(p->version);
  return v;
}

void shf_net::commit_params(int li) {
  Layer& L = layers[li];
  if (L.params.empty()) return;
  if (L.type == "BatchNorm" || L.type == "Scale") {
    // (the vectors are shared by every lane: nothing may be in flight on any stream)
    HIP_THROW(hipDeviceSynchronize());
    for (auto& p : L.params) p->dirty = false;
    if (L.norm_conv >= 0) {   // part of a convolution's parameters: re-fold and re-pack those
      // ... unless that convolution's last commit already folded these very values: a commit of the convolution, its
      // BatchNorm and its Scale after one load packs once, not three times
      if (layers[L.norm_conv].fold_bias->folded_from != fold_versions(L.norm_conv)) commit_params(L.norm_conv);
      return;
    }
    derive_norm(li);
    ++*wgen;
    return;
  }
  if (L.type == "Normalize" || L.type == "PReLU") {
    // the scale (PReLU: the slopes) the launch reads: C values, a channel_shared blob's one value broadcast, so that the
    // kernel has one form
    HIP_THROW(hipDeviceSynchronize());   // (shared by every lane: nothing may be in flight on any stream)
    ParamBlob& p = *L.params[0];
    const size_t C = (size_t)blobs[L.bottoms[0]].shape[1];
    const bool shared = L.type == "PReLU" ? L.prelu_shared : L.l2_shared;
    std::vector<float> sc(C);
    for (size_t c = 0; c < C; ++c) sc[c] = p.host[shared ? 0 : c];
    L.nv->g.ensure(C * 4);
    HIP_THROW(hipMemcpy(L.nv->g.p, sc.data(), C * 4, hipMemcpyHostToDevice));
    p.dirty = false;
    ++*wgen;
    return;
  }
  // a convolution with a BatchNorm / Scale folded in: every device tensor below is built from the effective parameters,
  // the blobs themselves (Net.params) keep Caffe's unfolded values
  std::vector<float> w_eff, b_eff;
  const bool folded = L.fold_bias != nullptr;
  if (folded) fold_conv_params(li, w_eff, b_eff);
  // the dual-tile family's weight pack (16-channel slabs, unscaled low parts): its 3x3 layers, and the 1x1 GEMM kernel's
  auto wants_family_pack = [](const Layer& Q, const ParamBlob& w) {
    return conv_f16x3_family_shape(w.shape[1], w.shape[0], Q.k, Q.pad, Q.dil, false, true);
  };
  // the raw / packed tensors are shared by every lane cloned from this net: nothing may be in flight on any stream
  HIP_THROW(hipDeviceSynchronize());
  bool in_tail = false;   // a predictor of some module: its weights go into that module's combined matrix
  for (TailModule& M : mods)
    if (std::count(M.cls_layers.begin(), M.cls_layers.end(), li) || std::count(M.box_layers.begin(), M.box_layers.end(), li)) {
      in_tail = true;
      M.w_dirty = true;
    }
  for (size_t pi = 0; pi < L.params.size(); ++pi) {
    ParamBlob& p = *L.params[pi];
    // what the device tensors are built from: the blob, or for a folded convolution its effective weights / bias
    const float* const src = !folded ? p.host.data() : pi == 0 ? w_eff.data() : b_eff.data();
    p.raw.ensure(p.count() * 4);
    HIP_THROW(hipMemcpy(p.raw.p, src, p.count() * 4, hipMemcpyHostToDevice));
    if (pi == 0 && L.type == "Convolution" && L.kclass == 1) {
      // first layer: (Cout, Cin*k*k) -> (Cin*k*k, Cout) so a wave's 16 output channels are one uniform run
      const int co = p.shape[0], K = (int)(p.count() / p.shape[0]);
      std::vector<float> t(p.count());
      for (int o = 0; o < co; ++o)
        for (int r = 0; r < K; ++r) t[(size_t)r * co + o] = src[(size_t)o * K + r];
      p.first_t.ensure(t.size() * 4);
      HIP_THROW(hipMemcpy(p.first_t.p, t.data(), t.size() * 4, hipMemcpyHostToDevice));
      if (co == 64 && K == 27) {  // the shape the fused producer/consumer kernel computes on the matrix cores
        std::vector<uint16_t> fr(kFirstConvFragHalfs);
        pack_first_conv_frags(src, fr.data());
        p.first_frag.ensure(fr.size() * 2);
        HIP_THROW(hipMemcpy(p.first_frag.p, fr.data(), fr.size() * 2, hipMemcpyHostToDevice));
        p.bf_stale = true;
        if (conv_mode == 4) {
          pack_first_conv_frags(src, fr.data(), true);
          p.first_frag_b.ensure(fr.size() * 2);
          HIP_THROW(hipMemcpy(p.first_frag_b.p, fr.data(), fr.size() * 2, hipMemcpyHostToDevice));
          p.bf_stale = false;
        }
      }
    }
    if (pi == 0 && L.type == "Convolution" && L.kclass == kConvClassGeneral && !in_tail) {
      // the general-geometry kernel's pack, K over (ky, kx, cin): its one parameter form in every conv mode
      std::vector<float> packed(gen_conv_weight_floats(p.shape[0], p.shape[1], p.shape[2]));
      pack_conv_weights_gen(src, p.shape[0], p.shape[1], p.shape[2], packed.data());
      p.packed_gen.ensure(packed.size() * 4);
      HIP_THROW(hipMemcpy(p.packed_gen.p, packed.data(), packed.size() * 4, hipMemcpyHostToDevice));
    }
    if (pi == 0 && L.type == "Convolution" && L.kclass == kConvClassDepthwise) {
      // the depthwise kernel's tap-major pack: its one parameter form in every conv mode
      std::vector<float> packed(p.count());
      pack_conv_weights_dw(src, p.shape[0], p.shape[2], packed.data());
      p.packed_dw.ensure(packed.size() * 4);
      HIP_THROW(hipMemcpy(p.packed_dw.p, packed.data(), packed.size() * 4, hipMemcpyHostToDevice));
    }
    if (pi == 0 && L.type == "Convolution" && L.kclass == 0 && !in_tail) {
      std::vector<float> packed(p.count());
      pack_conv_weights(src, p.shape[0], p.shape[1], p.shape[2], packed.data());
      p.packed.ensure(packed.size() * 4);
      HIP_THROW(hipMemcpy(p.packed.p, packed.data(), packed.size() * 4, hipMemcpyHostToDevice));
      // a commit in fp32 mode leaves the split-fp16 packs behind: shf_net_set_conv_mode re-packs them on the way back
      p.split_stale = p.packed16.p != nullptr;
      p.bf_stale = true;
      if (conv_mode == 4 && conv_f16x3_eligible(p.shape[1], p.shape[0], L.k, L.pad, L.dil)) {
        // bf16 mode: hi = bf16(w) bit patterns in the same layouts (no range check: bf16 has fp32's exponent range)
        std::vector<uint16_t> sp(split16_conv_weight_halfs(p.shape[0], p.shape[1], p.shape[2]));
        pack_conv_weights_split16(src, p.shape[0], p.shape[1], p.shape[2], sp.data(), true);
        p.packed16b.ensure(sp.size() * 2);
        HIP_THROW(hipMemcpy(p.packed16b.p, sp.data(), sp.size() * 2, hipMemcpyHostToDevice));
        if (L.first_src >= 0 && p.shape[0] == 64 && p.shape[1] == 64) {   // the fused first pair's own pack
          std::vector<uint16_t> sr(split16r_conv_weight_halfs(p.shape[0], p.shape[1], p.shape[2]));
          pack_conv_weights_split16r(src, p.shape[0], p.shape[1], p.shape[2], sr.data(), true);
          p.packed16rb.ensure(sr.size() * 2);
          HIP_THROW(hipMemcpy(p.packed16rb.p, sr.data(), sr.size() * 2, hipMemcpyHostToDevice));
        }
        if (wants_family_pack(L, p)) {
          std::vector<uint16_t> sh(split16h_conv_weight_halfs(p.shape[0], p.shape[1], p.shape[2]));
          pack_conv_weights_split16h(src, p.shape[0], p.shape[1], p.shape[2], sh.data(), true);
          p.packed16hb.ensure(sh.size() * 2);
          HIP_THROW(hipMemcpy(p.packed16hb.p, sh.data(), sh.size() * 2, hipMemcpyHostToDevice));
        }
        p.bf_stale = false;
      }
      if (conv_mode >= 1 && conv_mode <= 3 && conv_f16x3_eligible(p.shape[1], p.shape[0], L.k, L.pad, L.dil)) {
        // split-fp16 keeps hi = fp16(w): a weight beyond the fp16 range would become inf (the reference is fp32
        // everywhere, caffe/python/caffe/_caffe.cpp:46-48) -- refuse the mode instead of computing garbage
        for (size_t wi = 0; wi < p.count(); ++wi)
          if (!(std::fabs(src[wi]) <= 65504.f))
            throw std::runtime_error("layer '" + L.name + "': a weight is outside the fp16 range (|w| > 65504 or not "
                                     "finite); the split-fp16 conv mode cannot represent it -- use conv mode fp32");
        std::vector<uint16_t> sp(split16_conv_weight_halfs(p.shape[0], p.shape[1], p.shape[2]));
        pack_conv_weights_split16(src, p.shape[0], p.shape[1], p.shape[2], sp.data());
        p.packed16.ensure(sp.size() * 2);
        HIP_THROW(hipMemcpy(p.packed16.p, sp.data(), sp.size() * 2, hipMemcpyHostToDevice));
        if (L.first_src >= 0 && p.shape[0] == 64 && p.shape[1] == 64) {   // the fused first pair's own pack
          std::vector<uint16_t> sr(split16r_conv_weight_halfs(p.shape[0], p.shape[1], p.shape[2]));
          pack_conv_weights_split16r(src, p.shape[0], p.shape[1], p.shape[2], sr.data());
          p.packed16r.ensure(sr.size() * 2);
          HIP_THROW(hipMemcpy(p.packed16r.p, sr.data(), sr.size() * 2, hipMemcpyHostToDevice));
        }
        p.split_stale = false;
        if (wants_family_pack(L, p)) {
          std::vector<uint16_t> sh(split16h_conv_weight_halfs(p.shape[0], p.shape[1], p.shape[2]));
          p.wscale_inv = pack_conv_weights_split16h(src, p.shape[0], p.shape[1], p.shape[2], sh.data());
          p.packed16h.ensure(sh.size() * 2);
          HIP_THROW(hipMemcpy(p.packed16h.p, sh.data(), sh.size() * 2, hipMemcpyHostToDevice));
        }
      }
    }
    p.dirty = false;
  }
  if (folded) {   // the bias the launches read: a convolution without a bias blob gets one here
    ParamBlob& fb = *L.fold_bias;
    fb.host = b_eff;
    fb.folded_from = fold_versions(li);
    fb.raw.ensure(b_eff.size() * 4);
    HIP_THROW(hipMemcpy(fb.raw.p, b_eff.data(), b_eff.size() * 4, hipMemcpyHostToDevice));
  }
  ++*wgen;
}

void shf_net::load_caffemodel(const std::string& path) {
  // CopyTrainedLayersFrom (net.cpp:733-768): match by layer NAME, check shapes, copy blobs
  auto src = read_caffemodel(path);
  for (auto& sl : src) {
    for (auto& L : layers) {
      if (L.name != sl.name || L.params.empty()) continue;
      if (sl.blobs.size() != L.params.size())
        throw std::runtime_error("Incompatible number of blobs for layer " + L.name);
      for (size_t i = 0; i < L.params.size(); ++i) {
        ParamBlob& p = *L.params[i];
        if (sl.blobs[i].data.size() != p.count())
          throw std::runtime_error("Cannot copy param " + std::to_string(i) + " weights from layer '" + L.name +
                                   "'; shape mismatch.");
        std::copy(sl.blobs[i].data.begin(), sl.blobs[i].data.end(), p.host.begin());
        p.dirty = true;
        ++p.version;
      }
    }
  }
}

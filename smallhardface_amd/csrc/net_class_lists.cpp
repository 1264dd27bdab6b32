// Net runtime, part 4: the per-class detection lists of a multi-class image (shf_class_lists_*): what detect() does on the
// host after its forwards -- flip fix, unscale, per-class > thresh cut, per-class merge (lib/test.py:52-66,161-176) -- with
// the rows resident on the device from the proposal layer's outputs to the merged boxes.  The lists live on the head net,
// beside (and independent of) the single list of the fused path (net_detect.cpp).
#include "net_internal.h"

namespace {

// the refusals every entry shares: argument checks only, nothing is allocated or launched
void check_head(const char* who, const shf_net* net) {
  const std::string w = std::string(who) + ": ";
  if (!net) throw std::runtime_error(w + "NULL net");
  if (net->tail_layer < 0) throw std::runtime_error(w + "net has no proposal layer");
  refuse_multimodule(who, net);
  if (net->pipelined)
    throw std::runtime_error(w + "the head has shf_net_set_pipeline enabled: its stream belongs to the image pipeline");
}

void check_cls(const char* who, const shf_net* net, int cls) {
  if (cls < 1 || cls >= net->tail_C)
    throw std::runtime_error(std::string(who) + ": class " + std::to_string(cls) + " is outside 1.." +
                             std::to_string(net->tail_C - 1) + " (the net's foreground classes)");
}

void check_count(const char* who, int n) {
  if (n < 1 || n > kClassListsMaxUnits)
    throw std::runtime_error(std::string(who) + ": " + std::to_string(n) + " units: a group holds 1.." +
                             std::to_string(kClassListsMaxUnits));
}

void ensure_len(shf_net* net) {
  if (net->cl_len.p) return;
  net->cl_len.ensure(64);
  HIP_THROW(hipMemsetAsync(net->cl_len.p, 0, 64, net->stream));
}

// room for `units_after` units of rmax rows in every list (shf_net::ensure_img_cap's rule); what is gathered is kept
void ensure_lists(shf_net* net, int units_after) {
  ensure_len(net);
  const int nl = net->tail_C - 1;
  const long long rmax = std::max<long long>(1, net->pre_nms_topN > 0 ? net->pre_nms_topN : (long long)net->mods[0].tw.cap_anchors);
  const long long need = units_after * rmax;
  if (need <= net->cl_cap) return;
  const long long ncap = std::max(need, std::max<long long>(2LL * net->cl_cap, 16 * rmax));
  if (ncap > (1LL << 27))
    throw std::runtime_error("class lists: " + std::to_string(ncap) + " rows per class exceed the lists' limit of 2^27");
  DevBuf nd;
  nd.ensure((size_t)nl * ncap * 5 * 4);
  if (net->cl_dets.p && net->cl_cap > 0) {
    for (int c = 0; c < nl; ++c)
      HIP_THROW(hipMemcpyAsync((float*)nd.p + (size_t)c * ncap * 5, (const float*)net->cl_dets.p + (size_t)c * net->cl_cap * 5,
                               (size_t)net->cl_cap * 5 * 4, hipMemcpyDeviceToDevice, net->stream));
    HIP_THROW(hipStreamSynchronize(net->stream));
  }
  std::swap(net->cl_dets.p, nd.p); std::swap(net->cl_dets.cap, nd.cap);
  net->cl_cap = (int)ncap;
}

// the group's three launches on the head's stream
void add_units(shf_net* net, const ClassListsUnit* us, int n, float thresh) {
  ensure_lists(net, net->cl_units + n);
  const int nt = class_lists_tile_count(us, n);
  net->cl_tiles.ensure((size_t)std::max(nt, 1) * (net->tail_C - 1) * 4);
  ProfScope ps(net->prof, net->stream, PC_TAIL, 0, 0);
  CHECK_RC(launch_class_lists_add(us, n, net->tail_C, thresh, (float*)net->cl_dets.p, net->cl_cap, (int*)net->cl_tiles.p,
                                  (int*)net->cl_len.p, net->stream));
  net->cl_units += n;
}

void read_len(shf_net* net, int len[kTailMaxClasses]) {
  memset(len, 0, sizeof(int) * kTailMaxClasses);
  if (!net->cl_len.p) return;
  HIP_THROW(hipMemcpyAsync(len, net->cl_len.p, sizeof(int) * kTailMaxClasses, hipMemcpyDeviceToHost, net->stream));
  HIP_THROW(hipStreamSynchronize(net->stream));
}

}  // namespace

extern "C" {

int shf_class_lists_begin(shf_net* net) {
  API_BEGIN
  check_head("class_lists_begin", net);
  net->cl_len.ensure(64);
  HIP_THROW(hipMemsetAsync(net->cl_len.p, 0, 64, net->stream));
  net->cl_units = 0;
  return 0;
  API_END(-1)
}

int shf_class_lists_add(shf_net* net, int n, shf_net** members, const int* im_w, const float* im_scale, const int* flip,
                        float thresh) {
  API_BEGIN
  const char* who = "class_lists_add";
  check_head(who, net);
  check_count(who, n);
  if (!members || !im_w || !im_scale || !flip) throw std::runtime_error(std::string(who) + ": NULL argument");
  for (int m = 0; m < n; ++m) {
    const shf_net* s = members[m];
    const std::string w = std::string(who) + ": member " + std::to_string(m);
    if (!s) throw std::runtime_error(w + " is NULL");
    if (s->tail_layer < 0) throw std::runtime_error(w + " has no proposal layer");
    if (s->tail_C != net->tail_C)
      throw std::runtime_error(w + " has " + std::to_string(s->tail_C) + " classes, the head " + std::to_string(net->tail_C));
    if (s->mods.size() != 1) refuse_multimodule(who, s);
    if (!s->forwarded || s->mods[0].last_R < 0) throw std::runtime_error(w + " has not completed a forward");
  }
  ClassListsUnit us[kClassListsMaxUnits];
  for (int m = 0; m < n; ++m) {
    shf_net* s = members[m];
    us[m] = {(const float*)s->blobs[s->mods[0].boxes_blob].dev.p, s->probs_out(), s->mods[0].last_R, (float)im_w[m], im_scale[m],
             flip[m] ? 1 : 0};
  }
  add_units(net, us, n, thresh);
  return 0;
  API_END(-1)
}

int shf_debug_class_lists_add(shf_net* net, int n, const float* const* boxes5, const float* const* probs, const int* R,
                              const int* im_w, const float* im_scale, const int* flip, float thresh) {
  API_BEGIN
  const char* who = "debug_class_lists_add";
  check_head(who, net);
  check_count(who, n);
  if (!boxes5 || !probs || !R || !im_w || !im_scale || !flip) throw std::runtime_error(std::string(who) + ": NULL argument");
  const int C = net->tail_C;
  size_t floats = 0;
  for (int m = 0; m < n; ++m) {
    const std::string w = std::string(who) + ": unit " + std::to_string(m);
    if (R[m] < 0 || R[m] > kClassListsMaxRows)
      throw std::runtime_error(w + ": R = " + std::to_string(R[m]) + " is outside 0.." + std::to_string(kClassListsMaxRows));
    if (R[m] > 0 && (!boxes5[m] || !probs[m])) throw std::runtime_error(w + ": NULL boxes5 / probs");
    floats += (size_t)R[m] * (5 + C);
  }
  hipStream_t st = net->stream;
  net->cl_stage.ensure(std::max<size_t>(floats, 1) * 4);
  ClassListsUnit us[kClassListsMaxUnits];
  float* at = (float*)net->cl_stage.p;
  for (int m = 0; m < n; ++m) {
    const size_t nb = (size_t)R[m] * 5, np = (size_t)R[m] * C;
    us[m] = {at, at + nb, R[m], (float)im_w[m], im_scale[m], flip[m] ? 1 : 0};
    if (R[m] > 0) {
      HIP_THROW(hipMemcpyAsync(at, boxes5[m], nb * 4, hipMemcpyHostToDevice, st));
      HIP_THROW(hipMemcpyAsync(at + nb, probs[m], np * 4, hipMemcpyHostToDevice, st));
    }
    at += nb + np;
  }
  HIP_THROW(hipStreamSynchronize(st));   // (the caller's arrays are free again)
  add_units(net, us, n, thresh);
  return 0;
  API_END(-1)
}

int shf_class_lists_count(shf_net* net, int* counts) {
  API_BEGIN
  check_head("class_lists_count", net);
  if (!counts) throw std::runtime_error("class_lists_count: NULL argument");
  int len[kTailMaxClasses];
  read_len(net, len);
  for (int c = 0; c < net->tail_C - 1; ++c) counts[c] = len[c];
  return 0;
  API_END(-1)
}

int shf_class_lists_export(shf_net* net, int cls, float* dst_dev5, int cap_rows) {
  API_BEGIN
  check_head("class_lists_export", net);
  check_cls("class_lists_export", net, cls);
  if (cap_rows < 0 || (cap_rows > 0 && !dst_dev5)) throw std::runtime_error("class_lists_export: NULL argument");
  int len[kTailMaxClasses];
  read_len(net, len);
  const int n = len[cls - 1], w = std::min(n, cap_rows);
  if (w > 0) {
    HIP_THROW(hipMemcpyAsync(dst_dev5, (const float*)net->cl_dets.p + (size_t)(cls - 1) * net->cl_cap * 5, (size_t)w * 5 * 4,
                             hipMemcpyDeviceToDevice, net->stream));
    HIP_THROW(hipStreamSynchronize(net->stream));
  }
  return n;
  API_END(-1)
}

int shf_class_lists_finish(shf_net* net, int cls, int method, float nms_thresh, double* out5, int cap, int* n_out) {
  API_BEGIN
  check_head("class_lists_finish", net);
  check_cls("class_lists_finish", net, cls);
  if (!n_out || cap < 0 || (cap > 0 && !out5)) throw std::runtime_error("class_lists_finish: NULL argument");
  if (method != 0 && method != 1) throw std::runtime_error("class_lists_finish: method must be 0 (BBOX_VOTE) or 1 (NMS)");
  *n_out = 0;
  int len[kTailMaxClasses];
  read_len(net, len);
  const int n = len[cls - 1];
  if (n == 0) {
    if (method == 0) {  // bbox_vote on an empty set (test.py:184-186)
      const double d[5] = {10, 10, 20, 20, 0.0001};
      if (cap > 0) memcpy(out5, d, sizeof(d));
      *n_out = 1;
    }
    return 0;
  }
  ProfScope ps(net->prof, net->stream, PC_MERGE, 0, 0);
  // (NMS: with out5 given, MergeCtx::run writes the kept rows in keep order -- dets[keep])
  return net->merge.run((const float*)net->cl_dets.p + (size_t)(cls - 1) * net->cl_cap * 5, n, method, nms_thresh,
                        cap > 0 ? out5 : nullptr, cap, n_out, nullptr, net->stream);
  API_END(-1)
}

}  // extern "C"

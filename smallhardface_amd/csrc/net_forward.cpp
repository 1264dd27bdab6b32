// Net runtime, part 2: the layer walk (run_pass: one lane's unit, or one grouped pass over the units of several lanes),
// Net.forward() with its fp32 redo -- ONE function for 1..16 members (forward_members): shf_net::forward() is a group of
// one, forward_group is check_group plus that function --, Blob.data / Blob.gpu_data() read-back, and the profiler's kernel
// classes.
#include "net_internal.h"

namespace shf {

const char* const kProfNames[PC_COUNT] = {"conv_mfma_f32_kernel<3, 1, 128, 8, 16>", "conv_mfma_f32_kernel<3, 2, 128, 8, 16>",
                                           "conv_mfma_f32_kernel<3, 4, 128, 8, 16>", "conv_mfma_f32_kernel<3, 1, 64, 16, 16>",
                                           "conv_mfma_f32_kernel<3, 2, 64, 16, 16>", "conv_mfma_f32_kernel<3, 4, 64, 16, 16>",
                                           "conv_mfma_f32_kernel<1, 0, 128, 8, 16>", "conv_mfma_f32_kernel<1, 0, 64, 16, 16>",
                                           "conv_mfma_f16x3_kernel<128, false, 1, 3, 3, false>",
                                           "conv_mfma_f16x3_kernel<64, false, 1, 3, 3, false>",
                                           "conv_mfma_f16x3_kernel<64, true, 1, 3, 3, false>", "conv_mfma_f16x3_kernel<64, false, 2, 3, 3, false>",
                                           "conv_mfma_f16x3_kernel<64, false, 4, 3, 3, false>", "conv_mfma_f16x3_kernel<128, false, 1, 1, 3, false>",
                                           "conv_mfma_f16x3_kernel<64, false, 1, 1, 3, false>", "conv_mfma_f16x3_pc_kernel<3, false, false>",
                                           // dual-tile family <IN_SPLIT, rows / 4, tiles per block, products, bf16, dilation>: index = in_split * 4 + (rows == 8) * 2 + (tiles == 1)
                                           "conv_mfma_f16x3_w4d_kernel<false, 4, 2, 3, false, 1>", "conv_mfma_f16x3_w4d_kernel<false, 4, 1, 3, false, 1>",
                                           "conv_mfma_f16x3_w4d_kernel<false, 2, 2, 3, false, 1>", "conv_mfma_f16x3_w4d_kernel<false, 2, 1, 3, false, 1>",
                                           "conv_mfma_f16x3_w4d_kernel<true, 4, 2, 3, false, 1>", "conv_mfma_f16x3_w4d_kernel<true, 4, 1, 3, false, 1>",
                                           "conv_mfma_f16x3_w4d_kernel<true, 2, 2, 3, false, 1>", "conv_mfma_f16x3_w4d_kernel<true, 2, 1, 3, false, 1>",
                                           // kernels of their own (names: the headline mode's instantiation -- split-format input, three
                                           // products; the reduced modes run the same templates with other NP / BF arguments): the persistent
                                           // first pair, the 1x1 GEMM, the family's dilated forms, the three heads in one launch
                                           "conv_mfma_f16x3_pc_kernel<3, false, true>", "conv_mfma_f16x3_k1_kernel<true, 3>",
                                           "conv_mfma_f16x3_w4d_kernel<true, 4, 1, 3, false, 2>", "conv_mfma_f16x3_w4d_kernel<true, 4, 1, 3, false, 4>",
                                           "conv_mfma_f16x3_heads3_kernel<true, 3>",
                                           "conv_first_kernel", "conv_direct_kernel", "conv_mfma_f64_kernel", "maxpool_kernel",
                                           "deconv_depthwise", "detect_tail", "box_merge", "layout", "h2d_copy", "d2h_copy",
                                           "eltwise_combine", "conv_mfma_gen_kernel", "channel_affine", "conv_dw_kernel",
                                           "channel_l2norm", "pool_kernel", "neuron"};

int run_conv_plan(const ConvPlan& pl, hipStream_t s, Prof& prof, double flops, double bytes) {
  if (!pl.err.empty()) {
    set_error(pl.err);
    return -1;
  }
  for (int i = 0; i < pl.nl; ++i) {
    ProfScope ps(prof, s, pl.l[i].kern->prof, flops * pl.l[i].share, bytes * pl.l[i].share);
    if (launch_conv_plan(pl, i, s)) return -1;
  }
  return 0;
}
}  // namespace shf

static double conv_flops(const Layer& L, const std::vector<int>& in, const std::vector<int>& out) {
  return 2.0 * out[0] * out[2] * out[3] * (double)L.nout * (in[1] / std::max(L.group, 1)) * L.k * L.k;
}

// the proposal stage's arguments for the current shapes (also sizes the workspace: pre_nms_topN is shared with the
// other lanes and may have grown)
TailArgs shf_net::tail_args(int module, float im_h, float im_w, float im_scale, bool materialize) {
  TailModule& M = mods[module];
  if (M.w_dirty || M.gen != *wgen) build_tail_weights(M);
  TailArgs t;
  t.module = module;
  t.A = M.A; t.C = tail_C; t.heads = M.heads; t.Cf = M.Cf;
  for (int i = 0; i < M.heads; ++i) t.feat[i] = view_of(M.feat_blobs[i]);
  t.wcls[0] = (const float*)M.W.p;
  t.bcls[0] = (const float*)M.b.p;
  t.h = blobs[M.feat_blobs[0]].shape[2];
  t.w = blobs[M.feat_blobs[0]].shape[3];
  for (int i = 0; i < M.A * 4; ++i) t.anchors[i] = (float)M.anchors[i];
  for (int i = 0; i < M.A; ++i) t.sub_stride[i] = M.sub_stride[i];
  t.feat_stride = M.feat_stride;
  t.im_h = im_h; t.im_w = im_w; t.im_scale = im_scale;
  t.min_size = min_size; t.score_thresh = score_thresh; t.pre_nms_topN = pre_nms_topN;
  if (materialize) {
    t.cls_prob_reshape_nchw = (float*)blobs[M.cls_blob].dev.p;
    t.bbox_pred_nchw = (float*)blobs[M.box_blob].dev.p;
  }
  ensure_tail_workspace(M, (size_t)t.h * t.w * M.A);
  return t;
}

bool shf_net::split16(const Layer& L) const {
  const ParamBlob& w = *L.params[0];
  return split_mode() && L.kclass == 0 && (conv_mode == 4 ? w.packed16b.p : w.packed16.p) &&
         conv_f16x3_eligible(blobs[L.bottoms[0]].shape[1], L.nout, L.k, L.pad, L.dil);
}

// the fused first pair: conv li stages its halo from the raw image through the first-layer conv that feeds it, which then
// runs no launch of its own
bool shf_net::absorbs_first(int li, bool fused) const {
  const Layer& L = layers[li];
  if (!fused || L.first_src < 0 || !split16(L)) return false;
  // bf16 mode has the fused first pair on the producer/consumer kernel only: without its preconditions conv1_1 runs on
  // its own kernel and this layer as a plain bf16 convolution (the fp16 modes fall back to the 8-wave FUSE1 form instead)
  const Layer& F = layers[L.first_src];
  return conv_mode != 4 || (conv_knobs().pc && F.params[0]->first_frag_b.p != nullptr && F.nout == 64 && L.nout == 64);
}

ConvArgs shf_net::conv_args(int li, bool fused, int* flag) const {
  const Layer& L = layers[li];
  const ParamBlob& w = *L.params[0];
  const bool bf = conv_mode == 4, s16 = split16(L);
  ConvArgs a;
  a.in = view_of(L.bottoms[0]);   // (the first-layer kernel takes only its shape from it: its input is the NCHW image)
  a.out = view_of(L.tops[0]);
  a.k = L.k; a.dil = L.dil; a.pad = L.pad; a.relu = L.relu;
  a.bias = conv_bias(L);   // (with a BatchNorm / Scale folded in: the effective one)
  a.wraw = (const float*)w.raw.p;
  a.wpacked = (const float*)w.packed.p;
  a.wfirst = (const float*)w.first_t.p;
  a.wgen = (const float*)w.packed_gen.p;
  if (L.kclass == kConvClassDepthwise) {   // (group == bottom channels: the multiplier is what is left of num_output)
    a.wdw = (const float*)w.packed_dw.p;
    a.dw_mult = L.nout / L.group;
  }
  a.stride = L.stride;
  a.wsplit16 = s16 ? (bf ? w.packed16b.p : w.packed16.p) : nullptr;
  a.wsplit16h = s16 ? (bf ? w.packed16hb.p : w.packed16h.p) : nullptr;
  a.wsplit16r = s16 ? (bf ? w.packed16rb.p : w.packed16r.p) : nullptr;
  a.wscale_inv = bf ? 1.f : w.wscale_inv;
  a.bf16 = bf && s16 ? 1 : 0;
  a.f64 = f64_mode() ? 1 : 0;
  if (a.f64 && L.kclass == 1) a.img = nchw_input(L.bottoms[0]);   // (the one f64 kernel reads the first layer's NCHW image itself)
  // ... and so does the general-geometry kernel, in every mode (a stem on the image: no layout pass)
  if (L.kclass == kConvClassGeneral && blobs[L.bottoms[0]].kind == BK_INPUT_NCHW) a.img = nchw_input(L.bottoms[0]);
  // an fp16 mode: every producer of a map that a split-fp16 conv may read guards the fp16 range
  a.range_flag = fp16_mode() ? flag : nullptr;
  a.in_amax = amax_slot(L.bottoms[0]);
  a.out_amax = amax_slot(L.tops[0]);
  if (fused && L.fuse_pool >= 0) {
    const int pt = layers[L.fuse_pool].tops[0];
    a.pool = view_of(pt);
    a.write_main = L.pool_only ? 0 : 1;
    a.pool_split = s16 && !bf && blobs[pt].split_fused;
    a.pool_amax = amax_slot(pt);
  }
  if (s16) {  // how many of the three fp16 products this layer forms
    a.nprod = conv_mode == 1 ? 3 : conv_mode == 2 ? 2 : 1;   // (modes 3 "f16" and 4 "bf16": one product)
    auto it = sh->layer_products.find(L.name);
    if (it != sh->layer_products.end()) a.nprod = it->second;
  }
  if (fused && s16 && !bf) {   // (bf16 mode keeps fp32 activations in HBM)
    a.in_split = blobs[L.bottoms[0]].split_fused;
    a.out_split = blobs[L.tops[0]].split_fused;
  }
  if (absorbs_first(li, fused)) {
    const Layer& F = layers[L.first_src];
    a.img = nchw_input(F.bottoms[0]);
    a.w1t = (const float*)F.params[0]->first_t.p;
    a.w1f = bf ? F.params[0]->first_frag_b.p : F.params[0]->first_frag.p;
    a.b1 = conv_bias(F);
  }
  return a;
}

bool shf_net::combine_runs(int li, bool fused) const {
  const Layer& L = layers[li];
  if (L.folded_into < 0) return true;
  // a ReLU behind a copying Concat is part of the Concat's launches on both paths; the other folds are the fused path's
  // ... and so is one behind a BatchNorm / Scale chain
  return !(fused || layers[L.folded_into].op == OP_CONCAT_COPY || layers[L.folded_into].op == OP_NORM);
}

// the chain that layer li heads (plan_norm_layers): BatchNorm, Scale and ReLU stages with their layers' device vectors
NormStages shf_net::norm_stages(int li) const {
  const Layer& L = layers[li];
  NormStages st;
  if (L.chain_bn >= 0) {
    const NormVecs& v = *layers[L.chain_bn].nv;
    st.norm = 1;
    st.m = (const float*)v.m.p; st.d = (const float*)v.d.p;
    st.m64 = (const double*)v.m64.p; st.d64 = (const double*)v.d64.p;
  }
  if (L.chain_sc >= 0) {
    const Layer& S = layers[L.chain_sc];
    st.scale = 1;
    st.g = (const float*)S.nv->g.p;
    if (S.params.size() > 1) {
      st.bias = 1;
      st.b = (const float*)S.nv->b.p;
    }
  }
  if (L.chain_relu >= 0) {
    st.act = 1;
    st.slope = layers[L.chain_relu].slope;
  }
  return st;
}

NormArgs shf_net::norm_args(int li) const {
  const Layer& L = layers[li];
  NormArgs a;
  a.in = view_of(L.bottoms[0]);
  a.out = view_of(L.tops[0]);
  a.out_amax = amax_slot(L.tops[0]);
  return a;
}

// Pooling: what maxpool_kernel keeps -- MAX, square, not global, channel count and views multiples of 4 (its launches and its
// name in the profile are what they always were); every other layer runs the pooling kernel (pool.hip)
bool shf_net::pool_legacy(int li) const {
  const Layer& L = layers[li];
  // SHF_POOL_LEGACY=0 (measurements): every layer runs the pooling kernel.  Read once.
  static const bool keep = !(getenv("SHF_POOL_LEGACY") && atoi(getenv("SHF_POOL_LEGACY")) == 0);
  if (!keep) return false;
  if (L.pool_method != POOL_MAX || L.global_pool || L.kh != L.kw || L.sh != L.sw || L.ph != L.pw) return false;
  const View in = view_of(L.bottoms[0]), out = view_of(L.tops[0]);
  return !(in.C % 4 || in.cstride % 4 || in.coff % 4 || out.cstride % 4 || out.coff % 4);
}

PoolGeom shf_net::pool_geom(int li) const {
  const Layer& L = layers[li];
  PoolGeom q;
  q.method = L.pool_method;
  q.kh = L.kh; q.kw = L.kw; q.sh = L.sh; q.sw = L.sw; q.ph = L.ph; q.pw = L.pw;
  q.global = L.global_pool ? 1 : 0;
  return q;
}

PoolArgs shf_net::pool_args(int li) const {
  const Layer& L = layers[li];
  PoolArgs a;
  a.in = view_of(L.bottoms[0]);
  a.out = view_of(L.tops[0]);
  a.in_amax = amax_slot(L.bottoms[0]);
  a.out_amax = amax_slot(L.tops[0]);
  return a;
}

CombineArgs shf_net::combine_args(int li, bool fused, int member) const {
  const Layer& L = layers[li];
  CombineArgs a;
  a.out = view_of(L.tops[0]);
  a.out_amax = amax_slot(L.tops[0]);
  auto crop_window = [&](const Layer& C, int i) {
    a.in[i] = view_of(C.bottoms[0]);
    a.c0[i] = C.crop_origin[1]; a.y0[i] = C.crop_origin[2]; a.x0[i] = C.crop_origin[3];
  };
  switch (L.op) {
    case OP_ELTWISE:
      a.n_in = (int)L.bottoms.size();
      a.op = L.eop;
      for (int i = 0; i < a.n_in; ++i) {
        a.coeff[i] = L.coeff[i];
        int crop = -1;   // bottom i is the top of a Crop folded into this layer: read its source through the offsets
        for (size_t lj = 0; fused && lj < layers.size(); ++lj)
          if (layers[lj].op == OP_CROP && layers[lj].folded_into == li && layers[lj].tops[0] == L.bottoms[i]) crop = (int)lj;
        if (crop >= 0) crop_window(layers[crop], i);
        else a.in[i] = view_of(L.bottoms[i]);
      }
      break;
    case OP_CROP:
      crop_window(L, 0);
      break;
    case OP_RELU:
      a.in[0] = view_of(L.bottoms[0]);
      a.act = 1;
      a.slope = L.slope;
      break;
    case OP_CONCAT_COPY: {
      int off = 0;
      for (int j = 0; j < member; ++j) off += blobs[L.bottoms[j]].shape[1];
      a.in[0] = view_of(L.bottoms[member]);
      a.out.coff += off;
      a.out.C = a.in[0].C;
      break;
    }
    default:
      throw std::runtime_error("layer '" + L.name + "' is no combine launch");
  }
  if (L.fold_relu >= 0 && (fused || L.op == OP_CONCAT_COPY)) {
    a.act = 1;
    a.slope = layers[L.fold_relu].slope;
  }
  return a;
}

// the profiler's flops / bytes of layer li on this lane's unit, added to `flops` / `bytes`.  `heads` = 3: the three
// shared-weight heads of one launch; a conv that absorbs its first-layer producer is credited with that layer's flops too.
// A conv's weights are read once per launch, however many lanes it covers: run_pass counts them.
void shf_net::tail_cost(int module, double& flops, double& bytes) const {
  const TailModule& M = mods[module];
  const Blob& f = blobs[M.feat_blobs[0]];
  const double K = (double)f.shape[2] * f.shape[3];
  flops += 2.0 * K * M.A * (tail_C + 4) * M.Cf;
  bytes += 4.0 * K * (M.heads * M.Cf + M.A * 3 * (tail_C + 4));
}

void shf_net::add_cost(int li, bool fused, int heads, double& flops, double& bytes) const {
  const Layer& L = layers[li];
  if (L.op == OP_TAIL) {   // (booked at the last proposal layer, where the pass issues them: the tails of every module)
    if (li == tail_layer)
      for (int j = 0; j < (int)mods.size(); ++j) tail_cost(j, flops, bytes);
    return;
  }
  if (L.op == OP_ELTWISE || L.op == OP_CROP || L.op == OP_RELU || L.op == OP_CONCAT_COPY) {
    // the combine launch: n - 1 operations per output element, n reads and one write of it (a Crop folded into an Eltwise
    // is read through its offsets: the same count; a folded ReLU costs nothing more; a copying Concat: every member once)
    const double out = (double)blobs[L.tops[0]].count();
    const int n = L.op == OP_ELTWISE ? (int)L.bottoms.size() : 1;
    flops += (n - 1) * out;
    bytes += 4.0 * (n + 1) * out;
    return;
  }
  if (L.op == OP_NORM) {
    // the channel-affine launch: one read and one write per element, and one operation per stage of the chain (normalise,
    // scale, activation: 1 .. 3); a chain's members are booked with their head
    const double out = (double)blobs[L.tops[0]].count();
    if (L.folded_into < 0) {
      bytes += 8.0 * out;
      flops += ((L.chain_bn >= 0) + (L.chain_sc >= 0) + (L.chain_relu >= 0)) * out;
    }
    return;
  }
  if (L.op == OP_L2NORM) {
    // the channel-L2-norm launch: one read and one write per element; a square-and-add, a division and a product
    const double out = (double)blobs[L.tops[0]].count();
    bytes += 8.0 * out;
    flops += 3.0 * out;
    return;
  }
  if (L.op == OP_NEURON) {
    // the neuron launch: one read and one write per element (the constant form writes only, booked alike); operations per
    // element, a library call counted as one: PReLU 2 (product, add), Sigmoid 4, TanH 1, ELU 3, AbsVal 1, Threshold 1, BNLL
    // 4, Power 2 without pow and 3 with it, the constant 0, Exp 3, Log 4
    static const double kOps[NEURON_FORMS] = {2, 4, 1, 3, 1, 1, 4, 2, 3, 0, 3, 4};
    const double out = (double)blobs[L.tops[0]].count();
    bytes += 8.0 * out;
    flops += kOps[L.neuron_form] * out;
    return;
  }
  const Blob& ib = blobs[L.bottoms[0]];
  const Blob& ob = blobs[L.tops[0]];
  bytes += 4.0 * (ib.count() + heads * (double)ob.count());
  if (L.op == OP_DECONV) flops += 2.0 * ob.count() * 4;
  if (L.op != OP_CONV) return;
  flops += heads * conv_flops(L, ib.shape, ob.shape);
  if (absorbs_first(li, fused)) {
    const Layer& F = layers[L.first_src];
    flops += conv_flops(F, blobs[F.bottoms[0]].shape, blobs[F.tops[0]].shape);
  }
}

// The tails of a pass: every (unit, module) pair is one ENTRY of the grouped tail kernels (tail.hip), unit-major, and the
// entries go out as launch sequences of at most 16 (reset, logits, decode, sort stages, gather: one launch per stage and
// sequence) -- a single forward() of a net with up to four modules is always one sequence, as many launches as one module
// takes.  Called once per pass, at the LAST proposal layer of the walk: the feature maps of the earlier modules stay live
// until then (every blob owns its buffer, nothing is recycled).
//
// The reset kernel also zeroes each lane's activation-exponent slots for the next pass (TailWork::amax, carried by the
// lane's first module's entry alone: once per lane and pass).  It must run behind the last convolution of the walk, since
// a module's convolutions read the slots that the trunk published -- which is why the tails do not go out module by
// module at each proposal layer's own position.  What orders it there:
//   TAIL_LANE      the walk's layers and the lane's sequence share ONE in-order stream (p.s): the reset is enqueued after
//                  every convolution.  ev_logits is recorded behind the logits kernel, hence behind the reset: a later
//                  pass that waits for logits_done finds the slots zeroed.
//   TAIL_GROUP     the same stream order, all sequences on p.s; no events.
//   TAIL_HANDOVER  phase 1 (reset + logits) of every sequence is enqueued on the layers' stream p.s behind the last
//                  convolution; ev_convs is recorded on p.s AFTER phase 1, and it is the only thing the successor head's
//                  early start waits for before its first convolutions publish into the slots.  Phase 2 runs on the
//                  head's stream, which waits for ev_convs when it is not p.s, and touches the tail workspaces only.
static void run_tails(const Pass& p, bool f64) {
  if (p.tail == TAIL_NONE) return;
  shf_net& h = *p.head;
  const int nm = (int)p.u[0].lane->mods.size(), ne = p.n * nm;
  std::vector<TailArgs> t(ne);
  std::vector<TailWork*> tws(ne);
  std::vector<float*> boxes(ne), probs(ne);
  for (int m = 0; m < p.n; ++m) {
    shf_net& ln = *p.u[m].lane;
    for (int j = 0; j < nm; ++j) {
      const int e = m * nm + j;
      t[e] = ln.tail_args(j, p.u[m].im_h, p.u[m].im_w, p.u[m].im_scale, p.materialize);
      t[e].f64 = f64 ? 1 : 0;
      tws[e] = &ln.mods[j].tw;
      boxes[e] = (float*)ln.blobs[ln.mods[j].boxes_blob].dev.p;
      probs[e] = ln.probs_out(j);
    }
  }
  // the profiler's flops / bytes of entries e0 .. e1 - 1
  auto cost = [&](int e0, int e1) {
    double fl = 0, by = 0;
    for (int e = e0; e < e1; ++e) p.u[e / nm].lane->tail_cost(e % nm, fl, by);
    return std::make_pair(fl, by);
  };
  // one launch sequence over entries e0 .. e1 - 1 (launch_tail_group's phases)
  auto sequence = [&](int e0, int e1, hipStream_t s, hipEvent_t after_logits, int phase) {
    CHECK_RC(launch_tail_group(&t[e0], &tws[e0], &boxes[e0], &probs[e0], e1 - e0, s, after_logits, phase));
  };
  if (p.tail == TAIL_LANE) {   // per lane: its modules as one sequence
    for (int m = 0; m < p.n; ++m) {
      shf_net& ln = *p.u[m].lane;
      const auto c = cost(m * nm, (m + 1) * nm);
      ProfScope ps(h.prof, p.s, PC_TAIL, c.first, c.second);
      if (p.fused && !ln.ev_logits) HIP_THROW(hipEventCreateWithFlags(&ln.ev_logits, hipEventDisableTiming));
      sequence(m * nm, (m + 1) * nm, p.s, p.fused ? ln.ev_logits : nullptr, 0);
      if (p.fused) { ln.logits_done = ln.ev_logits; ln.logits_keep.reset(); }
    }
    return;
  }
  // the grouped steps: the lanes hold identical copies of a module's combined weights, one launch reads the first lane's
  for (int e = nm; e < ne; ++e) t[e].wcls[0] = t[e % nm].wcls[0], t[e].bcls[0] = t[e % nm].bcls[0];
  if (p.tail == TAIL_GROUP) {   // Net.forward() of a group: ONE launch per stage and sequence, all on the pass's stream
    for (int e0 = 0; e0 < ne; e0 += kMaxGroup) {
      const int e1 = std::min(ne, e0 + kMaxGroup);
      const auto c = cost(e0, e1);
      ProfScope ps(h.prof, p.s, PC_TAIL, c.first, c.second);
      sequence(e0, e1, p.s, nullptr, 0);
    }
    return;
  }
  // TAIL_HANDOVER: ~15 launches per image instead of ~100.  Phase 1 (reset + logits) is what reads the feature maps and
  // runs on the layers' stream; phase 2 works on the lanes' tail workspaces only and runs on the head's stream.
  if (!h.ev_convs) {
    h.ev_convs_own = std::make_shared<SharedEvent>();
    HIP_THROW(hipEventCreateWithFlags(&h.ev_convs_own->e, hipEventDisableTiming));
    h.ev_convs = h.ev_convs_own->e;
  }
  // the lanes' tail workspaces were last used by the predecessor head's tails (its own stream)
  if (h.pred && h.pred->ev_mark) HIP_THROW(hipStreamWaitEvent(p.s, h.pred->ev_mark, 0));
  for (int e0 = 0; e0 < ne; e0 += kMaxGroup) {
    const int e1 = std::min(ne, e0 + kMaxGroup);
    const auto c = cost(e0, e1);
    ProfScope ps(h.prof, p.s, PC_TAIL, c.first, c.second);
    sequence(e0, e1, p.s, nullptr, 1);
  }
  // recorded AFTER phase 1: its reset kernel zeroes the lanes' activation-exponent slots, which the successor head's
  // first convolutions (an early start waits for this event only) publish into and read
  HIP_THROW(hipEventRecord(h.ev_convs, p.s));
  // a pipelined head's layers ran on the shared conv stream: the feature maps are consumed and ev_convs is every
  // lane's hand-over mark; otherwise each lane gets its own, for passes issued from another head without a pipeline
  const bool shared = p.s != h.stream;
  if (shared) HIP_THROW(hipStreamWaitEvent(h.stream, h.ev_convs, 0));
  for (int m = 0; m < p.n; ++m) {
    shf_net& ln = *p.u[m].lane;
    if (!shared) {
      if (!ln.ev_logits) HIP_THROW(hipEventCreateWithFlags(&ln.ev_logits, hipEventDisableTiming));
      HIP_THROW(hipEventRecord(ln.ev_logits, h.stream));
    }
    ln.logits_done = shared ? h.ev_convs : ln.ev_logits;
    ln.logits_keep = shared ? h.ev_convs_own : nullptr;
  }
  for (int e0 = 0; e0 < ne; e0 += kMaxGroup) {
    ProfScope ps(h.prof, h.stream, PC_TAIL, 0, 0);
    sequence(e0, std::min(ne, e0 + kMaxGroup), h.stream, nullptr, 2);
  }
}

void run_pass(const Pass& p) {
  shf_net& h = *p.head;
  const shf_net& n0 = *p.u[0].lane;   // (every lane holds the same graph and parameter tensors)
  // f64 mode runs every pass layer by layer (one kernel for every conv class, pools and the first layer on their own)
  const bool f64 = h.f64_mode(), fused = p.fused && !f64;
  int* const flag = (int*)h.range_flag.p;
  // the profiler's flops / bytes of layer li on lanes m0 .. m1 - 1 in one launch: each lane's share, a conv's weights once
  auto cost = [&](int li, int m0, int m1, int heads) {
    const Layer& L = n0.layers[li];
    double fl = 0, by = L.op == OP_CONV ? 4.0 * L.params[0]->count() : 0;
    for (int m = m0; m < m1; ++m) p.u[m].lane->add_cost(li, fused, heads, fl, by);
    return std::make_pair(fl, by);
  };
  ConvArgs a1[kMaxGroup], a2[kMaxGroup], a4[kMaxGroup];
  int heads3_done = -1;   // index of a dilation-1 head whose launch also wrote its dilation-2 / -4 siblings
  for (int li = 0; li < (int)n0.layers.size(); ++li) {
    const Layer& L = n0.layers[li];
    if (li == p.wait_logits_at)
      for (int m = 0; m < p.n; ++m)
        if (p.u[m].lane->logits_done) HIP_THROW(hipStreamWaitEvent(p.s, p.u[m].lane->logits_done, 0));
    switch (L.op) {
      case OP_SKIP: break;
      case OP_CONV: {
        if (L.first_dst >= 0 && n0.absorbs_first(L.first_dst, fused)) break;   // computed inside the next conv's halo staging
        if (L.heads3_lead >= 0 && heads3_done == L.heads3_lead) break;        // written by the dilation-1 sibling's launch
        for (int m = 0; m < p.n; ++m) a1[m] = p.u[m].lane->conv_args(li, fused, flag);
        if (L.kclass == kConvClassDepthwise) {   // depthwise: one launch over the lanes, in every mode (f64: its binary64 form)
          const auto c = cost(li, 0, p.n, 1);
          ProfScope ps(h.prof, p.s, PC_CONV_DW, c.first, c.second);
          CHECK_RC_LAYER(launch_conv_dw(a1, p.n, p.s), L.name);
          break;
        }
        if (L.kclass == kConvClassGeneral) {   // the general geometry: one launch over the lanes, in every mode (f64: its binary64 form)
          const auto c = cost(li, 0, p.n, 1);
          ProfScope ps(h.prof, p.s, PC_CONV_GEN, c.first, c.second);
          CHECK_RC_LAYER(launch_conv_gen(a1, p.n, p.s), L.name);
          break;
        }
        if (L.kclass != 0 && !f64) {   // the first-layer kernel (NCHW image in) and the generic direct one: a launch per lane
          for (int m = 0; m < p.n; ++m) {
            const auto c = cost(li, m, m + 1, 1);
            ProfScope ps(h.prof, p.s, L.kclass == 1 ? PC_CONV_FIRST : PC_CONV_DIRECT, c.first, c.second);
            CHECK_RC(L.kclass == 1 ? launch_conv_first(p.u[m].lane->nchw_input(L.bottoms[0]), a1[m], p.s)
                                   : launch_conv_direct(a1[m], p.s));
          }
          break;
        }
        if (L.heads3_d2 >= 0 && !f64) {   // the three shared-weight heads in one launch (conv_f16x3_h3.h), if shapes and mode allow
          for (int m = 0; m < p.n; ++m) {
            a2[m] = p.u[m].lane->conv_args(L.heads3_d2, fused, flag);
            a4[m] = p.u[m].lane->conv_args(L.heads3_d4, fused, flag);
          }
          const ConvPlan pl = plan_conv_heads3(a1, a2, a4, p.n);
          if (pl.nl > 0 || !pl.err.empty()) {
            const auto c = cost(li, 0, p.n, 3);
            CHECK_RC_LAYER(run_conv_plan(pl, p.s, h.prof, c.first, c.second), L.name);
            heads3_done = li;
            break;
          }
        }
        const auto c = cost(li, 0, p.n, 1);
        CHECK_RC_LAYER(run_conv_plan(plan_conv(a1, p.n), p.s, h.prof, c.first, c.second), L.name);
        break;
      }
      case OP_POOL: {
        if (fused && L.fused_into >= 0) break;  // done by the producing conv's epilogue
        if (!n0.pool_legacy(li)) {
          // everything maxpool_kernel does not run (AVE, global, rectangular, channel counts or views off the quad grid): one
          // launch of the pooling kernel over the lanes of the pass, which raises the tops' activation-exponent slots itself
          PoolArgs pa[kMaxGroup];
          for (int m = 0; m < p.n; ++m) pa[m] = p.u[m].lane->pool_args(li);
          const auto c = cost(li, 0, p.n, 1);
          ProfScope ps(h.prof, p.s, PC_POOLGEN, c.first, c.second);
          CHECK_RC_LAYER(launch_pool_group(pa, p.n, n0.pool_geom(li), f64 ? 1 : 0, p.s), L.name);
          break;
        }
        for (int m = 0; m < p.n; ++m) {
          const shf_net& ln = *p.u[m].lane;
          const auto c = cost(li, m, m + 1, 1);
          ProfScope ps(h.prof, p.s, PC_POOL, c.first, c.second);
          CHECK_RC(launch_maxpool(ln.view_of(L.bottoms[0]), ln.view_of(L.tops[0]), L.k, L.stride, L.pad, p.s));
          if (ln.amax_slot(L.tops[0]))  // max |pooled| <= max |input|: the bound serves as the pooled blob's activation exponent
            CHECK_RC(launch_amax_raise(ln.amax_slot(L.tops[0]), ln.amax_slot(L.bottoms[0]), p.s));
        }
        break;
      }
      case OP_DECONV: {
        View in[kMaxGroup], out[kMaxGroup];
        unsigned* slot[kMaxGroup];
        bool batch1 = true;
        for (int m = 0; m < p.n; ++m) {
          const shf_net& ln = *p.u[m].lane;
          in[m] = ln.view_of(L.bottoms[0]);
          out[m] = ln.view_of(L.tops[0]);
          slot[m] = ln.amax_slot(L.tops[0]);
          batch1 = batch1 && in[m].B == 1;
        }
        const float* w = (const float*)L.params[0]->raw.p;
        const float* b = L.params.size() > 1 ? (const float*)L.params[1]->raw.p : nullptr;
        int* const dflag = h.fp16_mode() ? flag : nullptr;
        if (f64) {   // binary64 accumulation: one launch per unit
          for (int m = 0; m < p.n; ++m) {
            const auto c = cost(li, m, m + 1, 1);
            ProfScope ps(h.prof, p.s, PC_DECONV, c.first, c.second);
            CHECK_RC(launch_deconv_depthwise_f64(in[m], out[m], w, b, L.k, L.stride, L.pad, p.s));
          }
          break;
        }
        if (p.n > 1 && batch1) {   // the units' depthwise up-samplings as one launch (ten serial 5..60-us launches otherwise)
          const auto c = cost(li, 0, p.n, 1);
          ProfScope ps(h.prof, p.s, PC_DECONV, c.first, c.second);
          CHECK_RC(launch_deconv_depthwise_group(in, out, p.n, w, b, L.k, L.stride, L.pad, p.s, dflag, slot));
          break;
        }
        for (int m = 0; m < p.n; ++m) {
          const auto c = cost(li, m, m + 1, 1);
          ProfScope ps(h.prof, p.s, PC_DECONV, c.first, c.second);
          CHECK_RC(launch_deconv_depthwise(in[m], out[m], w, b, L.k, L.stride, L.pad, p.s, dflag, slot[m]));
        }
        break;
      }
      case OP_ELTWISE:
      case OP_CROP:
      case OP_RELU:
      case OP_CONCAT_COPY: {
        if (!n0.combine_runs(li, fused)) break;   // applied in another layer's launch on this path
        // one launch over the lanes of the pass; a copying Concat: one per member blob, into its channel window of the top
        const int parts = L.op == OP_CONCAT_COPY ? (int)L.bottoms.size() : 1;
        CombineArgs ca[kMaxGroup];
        for (int j = 0; j < parts; ++j) {
          for (int m = 0; m < p.n; ++m) ca[m] = p.u[m].lane->combine_args(li, fused, j);
          auto c = cost(li, 0, p.n, 1);
          if (L.op == OP_CONCAT_COPY) {   // (this member's share of the top)
            const double share = (double)ca[0].out.C / std::max(1, n0.blobs[L.tops[0]].shape[1]);
            c.first *= share; c.second *= share;
          }
          ProfScope ps(h.prof, p.s, PC_ELTWISE, c.first, c.second);
          CHECK_RC_LAYER(launch_combine_group(ca, p.n, f64 ? 1 : 0, h.fp16_mode() ? flag : nullptr, p.s), L.name);
        }
        break;
      }
      case OP_NORM: {
        if (L.folded_into >= 0) break;   // a member of an in-place chain: applied in its head's launch
        // one launch over the lanes of the pass (the stages and their vectors are the net's, shared by the lanes)
        NormArgs na[kMaxGroup];
        for (int m = 0; m < p.n; ++m) na[m] = p.u[m].lane->norm_args(li);
        const auto c = cost(li, 0, p.n, 1);
        ProfScope ps(h.prof, p.s, PC_NORM, c.first, c.second);
        CHECK_RC_LAYER(launch_channel_affine_group(na, p.n, n0.norm_stages(li), f64 ? 1 : 0, h.fp16_mode() ? flag : nullptr, p.s), L.name);
        break;
      }
      case OP_L2NORM: {
        // one launch over the lanes of the pass (the scale vector is the net's, shared by the lanes)
        NormArgs na[kMaxGroup];
        for (int m = 0; m < p.n; ++m) na[m] = p.u[m].lane->norm_args(li);
        const auto c = cost(li, 0, p.n, 1);
        ProfScope ps(h.prof, p.s, PC_L2NORM, c.first, c.second);
        CHECK_RC_LAYER(launch_channel_l2norm_group(na, p.n, (const float*)L.nv->g.p, L.eps, f64 ? 1 : 0, h.fp16_mode() ? flag : nullptr, p.s),
                       L.name);
        break;
      }
      case OP_NEURON: {
        // one launch over the lanes of the pass (PReLU's slope vector is the net's, shared by the lanes)
        NormArgs na[kMaxGroup];
        for (int m = 0; m < p.n; ++m) na[m] = p.u[m].lane->norm_args(li);
        NeuronSpec sp;
        sp.form = L.neuron_form; sp.a = L.neuron_a; sp.b = L.neuron_b; sp.c = L.neuron_c;
        sp.slope = L.neuron_form == NEURON_PRELU ? (const float*)L.nv->g.p : nullptr;
        const auto c = cost(li, 0, p.n, 1);
        ProfScope ps(h.prof, p.s, PC_NEURON, c.first, c.second);
        CHECK_RC_LAYER(launch_neuron_group(na, p.n, sp, f64 ? 1 : 0, h.fp16_mode() ? flag : nullptr, p.s), L.name);
        break;
      }
      case OP_TAIL:
        if (li == n0.tail_layer) run_tails(p, f64);
        break;
    }
  }
}

void shf_net::run_unit(bool fused, const float im_info[3], TailStep tail, bool materialize) {
  Pass p;
  p.head = this;
  p.u[0] = {this, im_info[0], im_info[1], im_info[2]};
  p.fused = fused;
  p.s = stream;
  p.tail = tail;
  p.materialize = materialize;
  run_pass(p);
}

// the fused path's kernels behind Net.forward(): a split-fp16 mode, a detector graph whose outputs are the proposal
// layer's (nothing else is an output: a conv top that is a net output must hold plain fp32 after forward())
bool shf_net::forward_fast_eligible() const {
  static const bool knob = !(getenv("SHF_FORWARD_FAST") && atoi(getenv("SHF_FORWARD_FAST")) == 0);
  if (!knob || !split_mode() || tail_layer < 0 || data_blob < 0) return false;
  for (int o : outputs)
    if (module_of_output(o) < 0) return false;
  return true;
}

// an input whose host copy is the newer one goes up on `st` (syncedmem.cpp:76-83 to_gpu); false: nothing to upload
static bool upload_host_newer(Blob& b, hipStream_t st, Prof& pf) {
  if (!b.host_newer || !b.host.p) return false;
  b.dev.ensure(b.count() * 4);
  ProfScope ps(pf, st, PC_H2D, 0, 4.0 * b.count());
  HIP_THROW(hipMemcpyAsync(b.dev.p, b.host.p, b.count() * 4, hipMemcpyHostToDevice, st));
  b.host_newer = false;
  return true;
}

// this net as a member of a forward on `st`: shapes for the data blob's current shape, its inputs on the device, its unit's
// im_info (from its own blob) in last_im_info
void shf_net::stage_forward(hipStream_t st, Prof& pf) {
  if (data_blob >= 0 && blobs[data_blob].shape != last_data_shape) {
    infer_shapes();
    alloc_buffers();
  }
  for (int bi : inputs) {
    blobs[bi].ext_dev = nullptr;
    upload_host_newer(blobs[bi], st, pf);
  }
  float ii[3] = {0, 0, 1};
  if (im_info_blob >= 0 && blobs[im_info_blob].host.p && blobs[im_info_blob].count() >= 3)
    memcpy(ii, blobs[im_info_blob].host.p, 12);
  memcpy(last_im_info, ii, 12);
  inputs_reshaped = false;
}

// ... and what the forward left in it: `plain` -- the per-layer kernels ran, every blob is materialised; R proposal rows
void shf_net::record_forward(bool plain, const int* R) {
  plain_stale = !plain;
  for (size_t j = 0; j < mods.size(); ++j) {
    TailModule& M = mods[j];
    blobs[M.boxes_blob].shape = {std::max(R[j], 1), 5};
    if (M.prob_blob >= 0) blobs[M.prob_blob].shape = {R[j], tail_C};
    M.last_R = R[j];
  }
  // (tail-fused blobs too: "newer" for them means the tail workspace holds this forward's logits -- read on demand)
  for (size_t i = 0; i < blobs.size(); ++i)
    if (!std::count(inputs.begin(), inputs.end(), (int)i)) blobs[i].dev_newer = true;
  forwarded = true;
}

// Net.forward() of n members as ONE pass on the head's stream, with the head's range flag and profiler.  Its two callers
// differ in the tail step, in whether the proposal outputs' host mirrors are filled here (`mirror_outputs`) or left to
// Blob.data, and in check_group, which only the group goes through.
static void forward_members(shf_net* head, int n, shf_net* const* members, TailStep tail, bool mirror_outputs) {
  hipStream_t st = head->stream;
  // a member's shf_blob_load_device was enqueued on its own stream: the pass is ordered after it
  for (int m = 0; m < n; ++m)
    if (members[m]->stream != st) HIP_THROW(hipStreamSynchronize(members[m]->stream));
  Pass p;
  p.head = head;
  p.n = n;
  p.s = st;
  p.tail = tail;
  p.materialize = true;
  for (int m = 0; m < n; ++m) {
    shf_net& ln = *members[m];
    ln.stage_forward(st, head->prof);
    p.u[m] = {&ln, ln.last_im_info[0], ln.last_im_info[1], ln.last_im_info[2]};
  }
  const bool fast = head->forward_fast_eligible(), has_tail = head->tail_layer >= 0, split = head->split_mode();
  const int nm = (int)head->mods.size();
  int cnt[kMaxGroup][kMaxModules][8] = {{{0}}}, flag = 0;
  auto run = [&](bool fused) {
    for (int m = 0; m < n; ++m) members[m]->reset_amax(st);
    p.fused = fused;
    run_pass(p);
  };
  auto copy_counters = [&]() {
    for (int m = 0; m < n; ++m)
      for (int j = 0; j < nm; ++j)
        HIP_THROW(hipMemcpyAsync(cnt[m][j], members[m]->mods[j].tw.counters, sizeof(cnt[m][j]), hipMemcpyDeviceToHost, st));
  };
  if (split) HIP_THROW(hipMemsetAsync(head->range_flag.p, 0, 4, st));
  run(fast);
  {
    ProfScope ps(head->prof, st, PC_D2H, 0, (double)n * nm * sizeof(cnt[0][0]) + 4);
    copy_counters();
    if (split) HIP_THROW(hipMemcpyAsync(&flag, head->range_flag.p, 4, hipMemcpyDeviceToHost, st));
  }
  HIP_THROW(hipStreamSynchronize(st));
  bool plain = !fast;
  if (flag && split) {
    // a convolution of SOME member produced |x| > 65504 (one flag per pass): fp16(hi) of the split overflowed somewhere
    // downstream.  The reference computes in fp32 (_caffe.cpp:46-48): redo THIS forward, the whole group, on the exact fp32
    // matrix-core kernels (per-layer path: every blob materialised).
    ++head->sh->range_fallbacks;
    Restore<int> mode(head->conv_mode);
    head->conv_mode = 0;
    run(false);
    copy_counters();
    HIP_THROW(hipStreamSynchronize(st));
    plain = true;
  }
  for (int m = 0; m < n; ++m) {
    int R[kMaxModules] = {0};
    for (int j = 0; j < nm; ++j) R[j] = cnt[m][j][2];
    members[m]->record_forward(plain, R);
  }
  if (!mirror_outputs || !has_tail) return;
  // the proposal outputs' host mirrors, now that the counts are known: every member's rows behind ONE synchronisation
  // (Blob.data of each would copy and synchronise on its own: 2 n round trips)
  {
    ProfScope ps(head->prof, st, PC_D2H, 0, 0);
    for (int m = 0; m < n; ++m) {
      shf_net& ln = *members[m];
      for (const TailModule& M : ln.mods)
        for (int bi : {M.boxes_blob, M.prob_blob}) {
          if (bi < 0) continue;
          Blob& b = ln.blobs[bi];
          const size_t c = b.count();
          b.host.ensure(std::max<size_t>(c, 1) * 4);
          if (c > 0) HIP_THROW(hipMemcpyAsync(b.host.p, b.dev.p, c * 4, hipMemcpyDeviceToHost, st));
        }
    }
  }
  HIP_THROW(hipStreamSynchronize(st));
  for (int m = 0; m < n; ++m) {
    shf_net& ln = *members[m];
    for (const TailModule& M : ln.mods) {
      ln.blobs[M.boxes_blob].dev_newer = false;
      if (M.prob_blob >= 0) ln.blobs[M.prob_blob].dev_newer = false;
    }
  }
}

// a single forward is a group of one on its own stream: TAIL_LANE, so that a fused pass records this lane's ev_logits and
// sets logits_done; no check_group, so a head with shf_net_set_pipeline enabled still runs
void shf_net::forward() {
  shf_net* self = this;
  forward_members(this, 1, &self, TAIL_LANE, false);
}

// shf_net_forward_group's refusals: argument checks only, nothing is allocated or launched
void check_group(const char* who, shf_net* head, int n, shf_net* const* members) {
  const std::string w = std::string(who) + ": ";
  if (!head) throw std::runtime_error(w + "NULL net");
  if (n < 1 || n > kMaxGroup)
    throw std::runtime_error(w + std::to_string(n) + " members: a group holds 1.." + std::to_string(kMaxGroup));
  if (!members) throw std::runtime_error(w + "NULL member list");
  for (int m = 0; m < n; ++m) {
    if (!members[m]) throw std::runtime_error(w + "member " + std::to_string(m) + " is NULL");
    for (int q = 0; q < m; ++q)
      if (members[q] == members[m])
        throw std::runtime_error(w + "members " + std::to_string(q) + " and " + std::to_string(m) + " are the same net: members must be distinct");
    // lanes of one root share its NetShared and its parameter generation counter (shf_net_clone)
    if (members[m]->sh != head->sh || members[m]->wgen != head->wgen || members[m]->layers.size() != head->layers.size())
      throw std::runtime_error(w + "member " + std::to_string(m) + " does not share the head's parameter tensors (not a lane of the same net)");
  }
  if (head->pipelined)
    throw std::runtime_error(w + "the head has shf_net_set_pipeline enabled: its convolutions belong to the shared stream of the image pipeline");
}

// the group: TAIL_GROUP (the tails as one launch per stage, no events) and the outputs' host mirrors filled eagerly
void forward_group(shf_net* head, int n, shf_net* const* members) {
  check_group("forward_group", head, n, members);
  forward_members(head, n, members, TAIL_GROUP, true);
}

// the intermediate blobs after a fast forward (see net_internal.h `plain_stale`): run the per-layer kernels once, in the
// forward's own arithmetic mode, on the inputs still resident on the device -- everything except the proposal tail
void shf_net::ensure_plain() {
  if (!plain_stale) return;
  if (inputs_reshaped || (data_blob >= 0 && blobs[data_blob].shape != last_data_shape))
    throw std::runtime_error("an input was reshaped after the last forward(): call forward() before reading intermediate blobs");
  reset_amax(stream);
  run_unit(false, last_im_info, TAIL_NONE);
  reset_amax(stream);   // (a pass without a tail leaves its slots raised: the next pass starts from zero, see prepare_unit)
  HIP_THROW(hipStreamSynchronize(stream));
  plain_stale = false;
}

// Blob.data of a blob whose producer was folded into the detection tail (the cls / bbox 1x1 convs, the score concat /
// reshape, the softmax): pycaffe exposes every blob after forward() (pycaffe.py:24-32, _caffe.cpp:222-242), and someone
// debugging through the shim reads them.  Nothing extra is computed in forward(): the logits kernel leaves
// [K][A][cls0 .. cls(C-1), dx, dy, dw, dh] in the tail workspace and the tail writes the softmax as the (1, C*A, h, w) blob the
// proposal layer reads; the read-back re-orders those on the host into the blob's own NCHW shape.
void shf_net::materialize_fused(int bi) {
  Blob& b = blobs[bi];
  const size_t n = b.count();
  b.host.ensure(std::max<size_t>(n, 1) * 4);
  if (!b.dev_newer || n == 0) return;          // (never forwarded: zeros, like a Caffe blob before its first forward)
  const TailModule& M = mods[b.fused_mod];   // the module whose tail the blob's producer was folded into
  const int A = M.A, NC = tail_C, NO = tail_C + 4;
  const int h = blobs[M.feat_blobs[0]].shape[2], w = blobs[M.feat_blobs[0]].shape[3];
  const size_t K = (size_t)h * w;
  float* out = b.host.p;
  if (b.fused_role == FR_PROB_PLANES) {
    if (n != K * A * NC) throw std::runtime_error("blob '" + b.name + "': unexpected shape for the softmax output");
    HIP_THROW(hipMemcpyAsync(out, blobs[M.cls_blob].dev.p, n * 4, hipMemcpyDeviceToHost, stream));
    HIP_THROW(hipStreamSynchronize(stream));
    b.dev_newer = false;
    return;
  }
  std::vector<float> lg(K * A * NO);
  HIP_THROW(hipMemcpyAsync(lg.data(), M.tw.logits, lg.size() * 4, hipMemcpyDeviceToHost, stream));
  HIP_THROW(hipStreamSynchronize(stream));
  auto L = [&](size_t k, int a, int o) { return lg[(k * A + a) * NO + o]; };
  const bool per_head = M.heads != 1;
  switch (b.fused_role) {
    case FR_CLS_CONV:
      if (n != (per_head ? NC : NC * (size_t)A) * K) throw std::runtime_error("blob '" + b.name + "': unexpected shape");
      if (per_head) {
        for (int c = 0; c < NC; ++c)
          for (size_t k = 0; k < K; ++k) out[c * K + k] = L(k, b.fused_head, c);
      } else {
        for (int c = 0; c < NC; ++c)
          for (int a = 0; a < A; ++a)
            for (size_t k = 0; k < K; ++k) out[((size_t)c * A + a) * K + k] = L(k, a, c);
      }
      break;
    case FR_BOX_CONV:
      if (n != (per_head ? 4 : 4 * (size_t)A) * K) throw std::runtime_error("blob '" + b.name + "': unexpected shape");
      if (per_head) {
        for (int j = 0; j < 4; ++j)
          for (size_t k = 0; k < K; ++k) out[j * K + k] = L(k, b.fused_head, NC + j);
      } else {
        for (int a = 0; a < A; ++a)
          for (int j = 0; j < 4; ++j)
            for (size_t k = 0; k < K; ++k) out[((size_t)a * 4 + j) * K + k] = L(k, a, NC + j);
      }
      break;
    case FR_CLS_PLANES:   // (1, C, A*h, w): plane c, rows a*h .. a*h + h - 1 = head / anchor a
      if (n != NC * (size_t)A * K) throw std::runtime_error("blob '" + b.name + "': unexpected shape");
      for (int c = 0; c < NC; ++c)
        for (int a = 0; a < A; ++a)
          for (size_t k = 0; k < K; ++k) out[((size_t)c * A + a) * K + k] = L(k, a, c);
      break;
    default:
      throw std::runtime_error("blob '" + b.name + "' is fused into the detection tail and has no read-back rule");
  }
  b.dev_newer = false;
}

// an NHWC activation's fp32 NCHW image in the blob's staging buffer, enqueued on the stream (what Blob.data copies to the
// host and Blob.gpu_data() hands out)
const float* shf_net::stage_nchw(int bi, bool is_input) {
  Blob& b = blobs[bi];
  if (!is_input) ensure_plain();   // (after a fast forward: the activations are not plain fp32 tensors yet)
  const size_t n = b.count();
  b.stage.ensure(n * 4);
  ProfScope ps(prof, stream, PC_LAYOUT, 0, 8.0 * n);
  CHECK_RC(launch_nhwc_to_nchw(view_of(bi), (float*)b.stage.p, stream));
  return (const float*)b.stage.p;
}

float* shf_net::host_data(int bi) {
  Blob& b = blobs[bi];
  if (b.kind == BK_FUSED) {
    materialize_fused(bi);
    return b.host.p;
  }
  const size_t n = b.count();
  b.host.ensure(std::max<size_t>(n, 1) * 4);
  const bool is_input = std::count(inputs.begin(), inputs.end(), bi) > 0;
  if (b.dev_newer && n > 0) {
    const void* src = b.kind == BK_NHWC ? stage_nchw(bi, is_input) : b.dev.p;
    {
      ProfScope ps(prof, stream, PC_D2H, 0, 4.0 * n);
      HIP_THROW(hipMemcpyAsync(b.host.p, src, n * 4, hipMemcpyDeviceToHost, stream));
    }
    HIP_THROW(hipStreamSynchronize(stream));
    b.dev_newer = false;
  }
  if (is_input) b.host_newer = true;
  return b.host.p;
}

// Blob.gpu_data() (syncedmem.cpp:110-119): the blob's fp32 NCHW image as a device pointer, valid until the next forward,
// reshape or load.  Inputs are their own NCHW buffer (uploaded first when the host copy is the head, to_gpu :76-83); flat
// and NCHW-matrix blobs likewise; an NHWC activation is transposed into the staging buffer Blob.data uses.  The stream is
// synchronised, so a consumer on any other stream may read.
const float* shf_net::device_data(int bi) {
  Blob& b = blobs[bi];
  if (b.kind == BK_FUSED)
    throw std::runtime_error("blob '" + b.name + "' is fused into the detection tail: it has no device image, read Blob.data");
  const size_t n = b.count();
  if (n == 0) throw std::runtime_error("blob '" + b.name + "' has zero elements");
  const bool is_input = std::count(inputs.begin(), inputs.end(), bi) > 0;
  const float* out = nullptr;
  if (is_input) {
    if (!upload_host_newer(b, stream, prof) && !b.dev_newer && !forwarded)
      throw std::runtime_error("blob '" + b.name + "' was never written: nothing to read on the device");
    out = (const float*)b.dev.p;
  } else {
    if (!forwarded) throw std::runtime_error("blob '" + b.name + "' was never forwarded: nothing to read on the device");
    if (b.kind == BK_NHWC) {
      if (b.shape.size() != 4) throw std::runtime_error("blob '" + b.name + "': an activation with " + std::to_string(b.shape.size()) + " axes has no NCHW image");
      out = stage_nchw(bi, false);
    } else {
      out = (const float*)b.dev.p;
    }
  }
  if (!out) throw std::runtime_error("blob '" + b.name + "' has no device buffer");
  HIP_THROW(hipStreamSynchronize(stream));
  return out;
}

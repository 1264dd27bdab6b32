"""Shared builders for the parity tests: the same graph + the same seeded synthetic
weights in the numpy oracle (CPU checker) and in the HIP runtime (through Net.params)."""
import numpy as np

from oracle import oracle as O
from smallhardface_amd import prototxt as P
from smallhardface_amd.config import cfg


def detector_msg(different_dilation=True):
    old = cfg.MODEL.DIFFERENT_DILATION.ENABLE
    cfg.MODEL.DIFFERENT_DILATION.ENABLE = different_dilation
    try:
        return P._add_dimension_reduction(P.build_test_template(different_dilation))
    finally:
        cfg.MODEL.DIFFERENT_DILATION.ENABLE = old


def load_params(gpu_net, params):
    for name, blobs in params.items():
        for i, arr in enumerate(blobs):
            gpu_net.params[name][i].data[...] = arr
    gpu_net.commit_params()


def make_pair(msg, seed=1234, cls_bias=4.0):
    """(gpu_net, oracle_net) holding identical parameters."""
    from smallhardface_amd import caffe
    params = O.synth_params(msg, seed=seed, cls_bias=cls_bias)
    onet = O.OracleNet(msg, params=params)
    gnet = caffe.Net(None, prototxt_text=P.dumps(msg))
    load_params(gnet, params)
    return gnet, onet


def run_both(gnet, onet, data, im_info):
    for net in (gnet, onet):
        net.blobs['data'].reshape(*data.shape)
        net.blobs['im_info'].reshape(*im_info.shape)
    go = gnet.forward(data=data, im_info=im_info)
    oo = onet.forward(data=data, im_info=im_info)
    return go, oo


def synth_image_blob(h, w, seed=0):
    rng = np.random.default_rng(seed)
    im = rng.integers(0, 256, (h, w, 3)).astype(np.float32) - np.array(cfg.PIXEL_MEANS, dtype=np.float32)[0]
    return np.ascontiguousarray(im.transpose(2, 0, 1)[None], dtype=np.float32)


def single_layer_net(layers_txt, cin, h=8, w=8):
    return ('name: "t"\ninput: "data"\ninput_shape { dim: 1 dim: %d dim: %d dim: %d }\n'
            'input: "im_info"\ninput_shape { dim: 1 dim: 3 }\n' % (cin, h, w)) + layers_txt


def _predictor(name, bottom, top, nout):
    return ('layer { name: "%s" type: "Convolution" bottom: "%s" top: "%s" convolution_param { num_output: %d '
            'kernel_size: 1 pad: 0 stride: 1 } }\n' % (name, bottom, top, nout))


def mini_detector(layers_txt, probe, feat_stride, cin=3, h=8, w=8, param_str=None):
    """`single_layer_net(layers_txt)` + a proposal tail on the blob(s) `probe`, so that Net.forward() takes the fused
    path (a graph without a tail never does) and the tail's fp32 logits kernel can copy the probed blob out.

    `probe` a name: the plain template's tail -- two 1x1 predictors `cls_score` / `bbox_pred` on that blob, Reshape,
    Softmax, Reshape, ProposalLayer with ratios [1,], eight scales and eight equal feat_stride entries: A = 8 anchors.
    `probe` a list of 2 .. 8 names (blobs of one size): the dilated template's tail -- per blob i the predictors
    `cls_score_<i>` (2 channels) / `bbox_pred_<i>` (4), scores concatenated on axis 2, deltas on axis 1, one anchor per
    blob.  Every probed blob needs C % 128 == 0 (the logits kernel's vector width).
    `param_str` (A, text): the ProposalLayer's param string and the A anchors it yields, instead of the default's; the
    single-blob tail then has 2A / 4A predictor outputs and the per-blob tail needs A blobs (`feat_stride` is unused)."""
    s = int(feat_stride)
    if isinstance(probe, str):
        A = 8 if param_str is None else int(param_str[0])
        tail = (_predictor("cls_score", probe, "cls_score_output", 2 * A) +
                _predictor("bbox_pred", probe, "bbox_pred_output", 4 * A) +
                'layer { name: "cls_reshape" type: "Reshape" bottom: "cls_score_output" top: "cls_score_reshape_output" '
                'reshape_param { shape { dim: 0 dim: 2 dim: -1 dim: 0 } } }\n')
    else:
        A = len(probe)
        assert 2 <= A <= 8 and (param_str is None or A == int(param_str[0]))
        tail = "".join(_predictor("cls_score_%d" % i, p, "cls_score_%d_output" % i, 2) +
                       _predictor("bbox_pred_%d" % i, p, "bbox_pred_%d_output" % i, 4) for i, p in enumerate(probe))
        tail += ('layer { name: "cls_score_output_concat" type: "Concat" %s top: "cls_score_reshape_output" '
                 'concat_param { axis: 2 } }\n' % " ".join('bottom: "cls_score_%d_output"' % i for i in range(A)))
        tail += ('layer { name: "bbox_pred_output_concat" type: "Concat" %s top: "bbox_pred_output" '
                 'concat_param { axis: 1 } }\n' % " ".join('bottom: "bbox_pred_%d_output"' % i for i in range(A)))
    tail += ('layer { name: "cls_prob" type: "Softmax" bottom: "cls_score_reshape_output" top: "cls_prob_output" }\n'
             'layer { name: "cls_prob_reshape" type: "Reshape" bottom: "cls_prob_output" top: "cls_prob_reshape_output" '
             'reshape_param { shape { dim: 0 dim: %d dim: -1 dim: 0 } } }\n' % (2 * A))
    tail += ('layer { name: "proposal" type: "Python" bottom: "cls_prob_reshape_output" bottom: "bbox_pred_output" '
             'bottom: "im_info" top: "boxes" top: "cls_prob" python_param { module: "lib.layers.proposal_layer" '
             'layer: "ProposalLayer" param_str: "%s" } }\n'
             % (param_str[1] if param_str is not None else "{'feat_stride': [%s],'scales': [%s], 'ratios':[1,]}"
                % (",".join([str(s)] * A), ",".join(str(i + 1) for i in range(A)))))
    return single_layer_net(layers_txt + tail, cin, h, w)


def _readout_heads(net):
    """0: the single-blob tail of `mini_detector`; n >= 2: its per-blob tail over n blobs."""
    if "cls_score" in net.params:
        return 0
    n = 0
    while "cls_score_%d" % n in net.params:
        n += 1
    assert n >= 2, "not a mini_detector graph"
    return n


def readout_forwards(onet):
    """Forwards `read_fused_blob` needs on this mini-detector: 32 channels each (single blob), 4 per blob otherwise."""
    heads = _readout_heads(onet)
    C = onet.params["cls_score" if heads == 0 else "cls_score_0"][0].shape[1]
    return -(-C // (32 if heads == 0 else 4))


def _readout_pairs(onet):
    heads = _readout_heads(onet)
    pairs = [("cls_score", "bbox_pred")] if heads == 0 else [("cls_score_%d" % i, "bbox_pred_%d" % i) for i in range(heads)]
    return heads, pairs, (8 if heads == 0 else 1), onet.params[pairs[0][0]][0].shape[1]


def readout_set_predictors(gnet, onet, c0):
    """One-hot predictor rows that copy channels c0 .. of the probed blob(s) into the logits (`read_fused_blob`): written
    to `onet.params` and, `gnet` given, to its parameters (a net's lanes share them)."""
    heads, pairs, A, C = _readout_pairs(onet)
    for cn, bn in pairs:
        wc = np.zeros((2 * A, C, 1, 1), np.float32)
        wb = np.zeros((4 * A, C, 1, 1), np.float32)
        for a in range(A):
            ch = c0 + 4 * a
            if ch + 3 < C:                       # (C % 128 == 0: whole groups of four)
                wc[a, ch] = wc[A + a, ch + 1] = 1.0          # cls_score channel = cls * A + a
                wb[4 * a, ch + 2] = wb[4 * a + 1, ch + 3] = 1.0
        for name, wt in ((cn, wc), (bn, wb)):
            onet.params[name][0][...] = wt
            onet.params[name][1][...] = 0
            if gnet is not None:
                gnet.params[name][0].data[...] = wt
                gnet.params[name][1].data[...] = 0


def readout_take(net, onet, outs, c0):
    """The channels `readout_set_predictors(.., c0)` copied, from the forwarded `net`'s predictor tops into `outs` (None:
    allocated here); returns `outs`, one (C, h, w) array per probed blob."""
    heads, pairs, A, C = _readout_pairs(onet)
    for i, (cn, bn) in enumerate(pairs):
        cs = np.array(net.blobs[cn + "_output"].data[0])
        bb = np.array(net.blobs[bn + "_output"].data[0])
        if outs is None:
            outs = [np.zeros((C,) + cs.shape[1:], np.float32) for _ in pairs]
        for a in range(A):
            ch = c0 + 4 * a
            if ch + 3 < C:
                outs[i][ch], outs[i][ch + 1] = cs[a], cs[A + a]
                outs[i][ch + 2], outs[i][ch + 3] = bb[4 * a], bb[4 * a + 1]
    return outs


def read_fused_blob(gnet, onet, data, im_info, mode="f16x3"):
    """What the probed blob(s) of a `mini_detector` hold after a FAST forward, exactly.

    After a split-fp16 forward on the fused path the intermediate blobs are recomputed by the per-layer kernels when read;
    the predictors' tops are not -- they are re-ordered from the logits the tail's plain fp32 kernel left.  With one-hot
    predictor rows and zero biases a logit is x * 1 + 0 * ... = x: per anchor the rows cls0, cls1, dx, dy each copy one
    channel (dw / dh stay zero: exp() in the decode cannot overflow), 32 channels per forward with the single-blob tail,
    4 per blob with the per-blob tail (exact one-hot rows there too, no random projection).  The predictors are written to
    `onet.params` and loaded into `gnet`, which forwards in conv mode `mode` (the logits kernel is fp32 arithmetic in every
    mode: the copy is exact in the reduced modes as well); `gnet` None forwards the oracle net instead (the CPU check of
    this read-out).  Returns the (C, h, w) blob, or the list of them for the per-blob tail."""
    heads, pairs, A, C = _readout_pairs(onet)
    net = gnet if gnet is not None else onet
    if gnet is not None:
        gnet.set_conv_mode(mode)
    for net_ in (gnet, onet):
        if net_ is not None:
            net_.blobs['data'].reshape(*data.shape)
            net_.blobs['im_info'].reshape(*im_info.shape)
    outs = None
    for c0 in range(0, C, 4 * A):
        readout_set_predictors(gnet, onet, c0)
        net.forward(data=data, im_info=im_info)
        outs = readout_take(net, onet, outs, c0)
    return outs[0] if heads == 0 else outs


def rel_err(a, b):
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / max(1e-12, np.abs(b).max()))

"""Builders for the multi-module tests (tests/test_gpu_modules.py): graphs with several ProposalLayers ("modules"), each
with its own class / bbox branch on a feature map of its own size, stride, channel count and anchor set, its tops named
``boxes_<level>`` / ``cls_prob_<level>`` as lib/test.py:67-83 of the reference collects them.  Text in the style of
``tests.helpers.mini_detector``; everything here runs without a GPU.

``three_module_mini(h, w)``: data (1, 128, h, w) -> 1x1 conv c0 (128 ch; module 1, stride 8) -> 2x2/2 MAX pool -> 1x1 conv
c1 (256 ch; module 2, stride 16) -> 2x2/2 MAX pool -> 1x1 convs c2, c2b (128 ch each; module 3, stride 32).  The modules
differ in everything the tail kernels' entry table carries: module 1 is a single-blob tail with A = 3 (scales 1, 2, 4),
module 2 a single-blob tail with A = 2 from two ratios and 'subsampled': False, module 3 a per-blob tail over two blobs
(heads == A == 2).

``ssh_shaped()``: the VGG trunk of ``build_test_template`` up to conv5_3 with a module on conv4_3 (stride 8), on conv5_3
(16) and on a pooled conv5_3 (32), each one 3x3 conv + ReLU of 128 channels before its single-blob predictors.
"""
import numpy as np

from oracle import oracle as O
from smallhardface_amd import prototxt as P
from tests import helpers as H

# module -> (feature blobs, A, ProposalLayer param string)
MINI_MODULES = {
    "1": (["c0"], 3, "{'feat_stride': [8,8,8],'scales': [1,2,4], 'ratios':[1,]}"),
    "2": (["c1"], 2, "{'feat_stride': [16],'scales': [2], 'ratios':[0.5,2], 'subsampled': False}"),
    "3": (["c2", "c2b"], 2, "{'feat_stride': [32,32],'scales': [1,2], 'ratios':[1,]}"),
}
SSH_MODULES = {
    "1": (["m1_conv"], 2, "{'feat_stride': [8,8],'scales': [1,2], 'ratios':[1,]}"),
    "2": (["m2_conv"], 2, "{'feat_stride': [16,16],'scales': [2,4], 'ratios':[1,]}"),
    "3": (["m3_conv"], 2, "{'feat_stride': [32,32],'scales': [4,8], 'ratios':[1,]}"),
}


def _conv1(name, bottom, nout):
    return ('layer { name: "%s" type: "Convolution" bottom: "%s" top: "%s" convolution_param { num_output: %d '
            'kernel_size: 1 pad: 0 } }\n' % (name, bottom, name, nout))


def _pool(name, bottom):
    return ('layer { name: "%s" type: "Pooling" bottom: "%s" top: "%s" pooling_param { pool: MAX kernel_size: 2 '
            'stride: 2 } }\n' % (name, bottom, name))


def module_tail(m, feats, A, param_str, C=2, tops=None):
    """The tail of module `m` on the blob(s) `feats`: one blob -- the plain template's single-blob tail (C A / 4 A predictor
    outputs, Reshape, Softmax, Reshape); several -- the dilated template's per-blob tail (C / 4 outputs per blob, scores
    concatenated on axis 2, deltas on axis 1).  Layer names carry ``_m<m>``, internal blobs the suffix ``_<m>``; the tops are
    ``boxes_<m>`` / ``cls_prob_<m>`` unless `tops` names them."""
    s = "_%s" % m
    if len(feats) == 1:
        t = (H._predictor("cls_score_m%s" % m, feats[0], "cls_score_output" + s, C * A) +
             H._predictor("bbox_pred_m%s" % m, feats[0], "bbox_pred_output" + s, 4 * A) +
             'layer { name: "cls_reshape_m%s" type: "Reshape" bottom: "cls_score_output%s" top: "cls_score_reshape_output%s" '
             'reshape_param { shape { dim: 0 dim: %d dim: -1 dim: 0 } } }\n' % (m, s, s, C))
    else:
        assert len(feats) == A
        t = "".join(H._predictor("cls_score_m%s_%d" % (m, i), f, "cls_score_%d_output%s" % (i, s), C) +
                    H._predictor("bbox_pred_m%s_%d" % (m, i), f, "bbox_pred_%d_output%s" % (i, s), 4) for i, f in enumerate(feats))
        t += ('layer { name: "cls_score_concat_m%s" type: "Concat" %s top: "cls_score_reshape_output%s" concat_param { axis: 2 } }\n'
              % (m, " ".join('bottom: "cls_score_%d_output%s"' % (i, s) for i in range(A)), s))
        t += ('layer { name: "bbox_pred_concat_m%s" type: "Concat" %s top: "bbox_pred_output%s" concat_param { axis: 1 } }\n'
              % (m, " ".join('bottom: "bbox_pred_%d_output%s"' % (i, s) for i in range(A)), s))
    t += ('layer { name: "cls_prob_m%s" type: "Softmax" bottom: "cls_score_reshape_output%s" top: "cls_prob_output%s" }\n'
          'layer { name: "cls_prob_reshape_m%s" type: "Reshape" bottom: "cls_prob_output%s" top: "cls_prob_reshape_output%s" '
          'reshape_param { shape { dim: 0 dim: %d dim: -1 dim: 0 } } }\n' % (m, s, s, m, s, s, C * A))
    tops = tops or ("boxes" + s, "cls_prob" + s)
    t += ('layer { name: "proposal_m%s" type: "Python" bottom: "cls_prob_reshape_output%s" bottom: "bbox_pred_output%s" '
          'bottom: "im_info" top: "%s" top: "%s" python_param { module: "lib.layers.proposal_layer" layer: "ProposalLayer" '
          'param_str: "%s" } }\n' % (m, s, s, tops[0], tops[1], param_str))
    return t


def mini_text(h, w, modules=("1", "2", "3"), cin=128):
    """The mini graph with the modules named, and of the trunk only what they read.  `cin`: channels of `data` (3: the
    graph takes the driver's image levels)."""
    trunk = _conv1("c0", "data", 128)
    if set(modules) & {"2", "3"}:
        trunk += _pool("p1", "c0") + _conv1("c1", "p1", 256)
    if "3" in modules:
        trunk += _pool("p2", "c1") + _conv1("c2", "p2", 128) + _conv1("c2b", "p2", 128)
    return H.single_layer_net(trunk + "".join(module_tail(m, *MINI_MODULES[m]) for m in modules), cin, h, w)


def three_module_mini(h, w):
    return mini_text(h, w)


def mini_params(seed=7, cls_bias=(0.0, 0.0, 0.0), cin=128):
    """Seeded parameters of the three-module mini graph (any size: the weights do not depend on it); module m's class
    predictors carry the bias +- cls_bias[m - 1]."""
    msg = P.parse(mini_text(16, 16, cin=cin))
    params = O.synth_params(msg, seed=seed, cls_bias=1.0)
    for name, blobs in params.items():
        if name.startswith("cls_score_m"):
            blobs[1] *= np.float32(cls_bias[int(name[len("cls_score_m")]) - 1])
    return params


def mini_map_sizes(h, w):
    """(h, w) of the three modules' feature maps under Caffe's ceil pooling."""
    h2, w2 = -(-h // 2), -(-w // 2)
    return {"1": (h, w), "2": (h2, w2), "3": (-(-h2 // 2), -(-w2 // 2))}


def ssh_shaped(h=64, w=96):
    """(Msg) the SSH-shaped graph at input size h x w."""
    tmpl = P.build_test_template(False)
    net = P.Msg()
    for k, v in tmpl.fields:
        if k == "layer" and str(v.get("name")) == "conv5_256":
            break
        net.add(k, v)
    txt = P.dumps(net)
    extra = _pool("pool5", "conv5_3")
    for m, bottom in (("1", "conv4_3"), ("2", "conv5_3"), ("3", "pool5")):
        name = "m%s_conv" % m
        extra += ('layer { name: "%s" type: "Convolution" bottom: "%s" top: "%s" convolution_param { num_output: 128 '
                  'kernel_size: 3 pad: 1 } }\nlayer { name: "%s_relu" type: "ReLU" bottom: "%s" top: "%s" }\n'
                  % (name, bottom, name, name, name, name))
        extra += module_tail(m, *SSH_MODULES[m])
    msg = P.parse(txt + "\n" + extra)
    msg.set_nth("input_shape", 0, P.Msg([("dim", 1), ("dim", 3), ("dim", h), ("dim", w)]))
    return msg


def module_params(param_str, **kw):
    """The oracle's ProposalParams of a module's param string."""
    import ast
    return O.ProposalParams(**dict(ast.literal_eval(param_str), **kw))


def levels_of(net):
    """The level order lib/test.py:71-72 derives from the blob names."""
    return [k.split('_')[-1] for k in net.blobs.keys() if k.startswith('boxes')]


def oracle_margins(onet, info, modules, min_size, score_thresh):
    """On a forwarded oracle net, per module: (distance of the nearest foreground score to the threshold, distance of the
    nearest box side to the min-size cut, whether two rows tie in score) -- what an end-to-end comparison of row sets
    hinges on."""
    out = {}
    for m, (feats, A, pstr) in modules.items():
        sc = onet.blobs["cls_prob_reshape_output_%s" % m].data
        dl = onet.blobs["bbox_pred_output_%s" % m].data
        b, p = O.proposal_forward(sc, dl, info, module_params(pstr, min_size=0, score_thresh=-1.0, pre_nms_topN=0))
        sides = np.concatenate([b[:, 3] - b[:, 1] + 1, b[:, 4] - b[:, 2] + 1])
        fg = p[:, 1:].max(axis=1)
        rows = onet.blobs["cls_prob_%s" % m].data
        ties = len(rows) > 0 and len(np.unique(rows[:, 1:].max(axis=1))) != len(rows)
        out[m] = (float(np.abs(fg - score_thresh).min()), float(np.abs(sides - min_size * info[0, 2]).min()), bool(ties))
    return out

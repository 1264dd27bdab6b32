"""Graphs and fixture access shared by tests/test_multiclass.py (CPU) and tests/test_gpu_multiclass_tail.py (GPU): a
proposal tail with C classes in both forms the templates use, restated from tests/helpers.py `mini_detector` (which
writes two classes into its predictors and Reshapes)."""
import ast

import numpy as np

from oracle import oracle as O
from tests import helpers as H

PSTR_A1 = "{'feat_stride': [8],'scales': [1], 'ratios':[1,]}"
PSTR_A3 = "{'feat_stride': [8,8,8],'scales': [1,2,4], 'ratios':[1,]}"
PSTR_A8 = "{'feat_stride': [8,16], 'scales': [1,2], 'ratios': [1,], 'shifts': [0,0.5]}"
PSTR = {1: PSTR_A1, 3: PSTR_A3, 8: PSTR_A8}


def conv1(name, bottom, nout):
    return ('layer { name: "%s" type: "Convolution" bottom: "%s" top: "%s" convolution_param { num_output: %d '
            'kernel_size: 1 pad: 0 } }\n' % (name, bottom, name, nout))


def conv3(name, bottom, nout, dil=1):
    return ('layer { name: "%s" type: "Convolution" bottom: "%s" top: "%s" convolution_param { num_output: %d '
            'kernel_size: 3 pad: %d dilation: %d } }\n'
            'layer { name: "%s_relu" type: "ReLU" bottom: "%s" top: "%s" }\n' % (name, bottom, name, nout, dil, dil, name, name, name))


def tail(probe, C, A, param_str, cls_nout=None, pre_dim=None, final_dim=None):
    """The proposal tail on `probe`: a blob name -- the plain template's single-blob form, one `cls_score` with C*A
    outputs (channel c*A + a), Reshape (0, C, -1, 0), Softmax, Reshape (0, C*A, -1, 0) -- or a list of A blob names -- the
    dilated template's per-head form, `cls_score_<i>` with C outputs each, Concat on axis 2, Softmax, the same Reshape.
    `cls_nout` (one number, or one per head), `pre_dim`, `final_dim` override what a consistent graph would say."""
    if isinstance(probe, str):
        t = (H._predictor("cls_score", probe, "cls_score_output", C * A if cls_nout is None else cls_nout) +
             H._predictor("bbox_pred", probe, "bbox_pred_output", 4 * A) +
             'layer { name: "cls_reshape" type: "Reshape" bottom: "cls_score_output" top: "cls_score_reshape_output" '
             'reshape_param { shape { dim: 0 dim: %d dim: -1 dim: 0 } } }\n' % (C if pre_dim is None else pre_dim))
    else:
        assert len(probe) == A
        nouts = [C] * A if cls_nout is None else ([cls_nout] * A if isinstance(cls_nout, int) else list(cls_nout))
        t = "".join(H._predictor("cls_score_%d" % i, p, "cls_score_%d_output" % i, nouts[i]) +
                    H._predictor("bbox_pred_%d" % i, p, "bbox_pred_%d_output" % i, 4) for i, p in enumerate(probe))
        t += ('layer { name: "cls_score_output_concat" type: "Concat" %s top: "cls_score_reshape_output" '
              'concat_param { axis: 2 } }\n' % " ".join('bottom: "cls_score_%d_output"' % i for i in range(A)))
        t += ('layer { name: "bbox_pred_output_concat" type: "Concat" %s top: "bbox_pred_output" '
              'concat_param { axis: 1 } }\n' % " ".join('bottom: "bbox_pred_%d_output"' % i for i in range(A)))
    t += ('layer { name: "cls_prob" type: "Softmax" bottom: "cls_score_reshape_output" top: "cls_prob_output" }\n'
          'layer { name: "cls_prob_reshape" type: "Reshape" bottom: "cls_prob_output" top: "cls_prob_reshape_output" '
          'reshape_param { shape { dim: 0 dim: %d dim: -1 dim: 0 } } }\n' % (C * A if final_dim is None else final_dim))
    t += ('layer { name: "proposal" type: "Python" bottom: "cls_prob_reshape_output" bottom: "bbox_pred_output" '
          'bottom: "im_info" top: "boxes" top: "cls_prob" python_param { module: "lib.layers.proposal_layer" '
          'layer: "ProposalLayer" param_str: "%s" } }\n' % param_str)
    return t


def one_hot_net_txt(Cf, h, w, C, A, per_head, **kw):
    """data (1, Cf, h, w) -> one-hot 1x1 convolutions c0 .. (one per head) -> a C-class tail of either form."""
    n = A if per_head else 1
    layers = "".join(conv1("c%d" % i, "data", Cf) for i in range(n))
    return H.single_layer_net(layers + tail(["c%d" % i for i in range(n)] if per_head else "c0", C, A, PSTR[A], **kw), Cf, h, w)


def whole_net_txt(C, per_head, h=9, w=13):
    """data (1, 16, h, w) -> 3x3 conv to 128 channels + ReLU -> per-head tail (three dilated 3x3 heads) or single-blob tail."""
    layers = conv3("conv_a", "data", 128)
    if per_head:
        layers += "".join(conv3("head_%d" % i, "conv_a", 128, dil=d) for i, d in enumerate((1, 2, 4)))
        probe = ["head_%d" % i for i in range(3)]
    else:
        probe = "conv_a"
    return H.single_layer_net(layers + tail(probe, C, 3, PSTR_A3), 16, h, w)


def whole_params(msg, seed=7):
    """`synth_params` with every cls_score* bias zero and the cls_score* weights times 8: `synth_params` splits the class
    biases in halves (bg / fg), which means nothing for C > 2, and its weights alone leave the classes near 1 / C."""
    params = O.synth_params(msg, seed=seed)
    for name, blobs in params.items():
        if name.startswith("cls_score"):
            blobs[0] *= np.float32(8)
            blobs[1][...] = 0
    return params


def whole_input(h=9, w=13):
    return np.random.default_rng(3).normal(0, 1, (1, 16, h, w)).astype(np.float32), np.array([[8 * h, 8 * w, 1.0]], np.float32)


def fixture_case(g, case):
    """(scores, deltas, im_info, ProposalParams, (topN, thresh, min_size), reference boxes, reference probs)"""
    topn, thresh, min_size = (float(v) for v in g[case + "_cfg"])
    pp = O.ProposalParams(**dict(ast.literal_eval(str(g[case + "_param_str"])), pre_nms_topN=int(topn), score_thresh=thresh,
                                 min_size=min_size))
    return (g[case + "_scores"], g[case + "_deltas"], g[case + "_im_info"], pp, (int(topn), thresh, min_size),
            g[case + "_boxes"], g[case + "_probs"])


CASES = ["c3_a3", "c3_a8", "c4_a8", "tie_classes", "class2_wins", "topn_cut", "none_at_thresh", "none_valid"]


def rows_sorted(a):
    a = np.asarray(a)
    return a if a.shape[0] == 0 else a[np.lexsort(a.T[::-1])]

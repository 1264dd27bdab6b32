"""Every field of the layer messages the graph reader accepts, with what becomes of it (tests/test_graph_fields_host.py on the
CPU, tests/test_gpu_graph_fields.py on the GPU).

The kernels are compared with their oracles per element; the step in front of them -- a prototxt's text into layer geometry --
was read by the runtime (csrc/net_graph.cpp) and by the oracles through the same product parser, so a field both ignored was a
wrong answer no comparison could see.  Here every field that Caffe's schema declares (tests/golden/caffe_layer_fields.json,
names only) has one disposition:

    HONOURED   a non-default value changes the result as Caffe says; `case` names the value case that proves it: an id of
               VALUE_CASES below, or "module:ATTRIBUTE" of an existing case table / test that already varies the field
               against a reference with explicit geometry
    REFUSED    a non-default or unsupported value is refused at caffe.Net() with the layer's and the field's name; `case` is
               an id of REFUSALS below
    INERT      the field cannot change an inference result; `why` says so in a line

Keys are (scope, field): scope is a layer type for the fields of its parameter message, "Layer" for LayerParameter's own
fields and "Net" for NetParameter's.  The geometry the value cases' reference uses comes from oracle/graph_reader.py, the
independent reading by Caffe's rules, never from the product's parser.
"""
import numpy as np

from oracle import graph_reader as R
from tests import helpers as H
from tests import pooling_cases as K

F32, F64 = np.float32, np.float64
HONOURED, REFUSED, INERT = "HONOURED", "REFUSED", "INERT"

# layer type -> (its parameter field in LayerParameter, the message of the census)
TYPE_MESSAGE = {
    "Convolution": ("convolution_param", "ConvolutionParameter"), "Deconvolution": ("convolution_param", "ConvolutionParameter"),
    "Pooling": ("pooling_param", "PoolingParameter"), "ReLU": ("relu_param", "ReLUParameter"),
    "Eltwise": ("eltwise_param", "EltwiseParameter"), "Crop": ("crop_param", "CropParameter"),
    "BatchNorm": ("batch_norm_param", "BatchNormParameter"), "Scale": ("scale_param", "ScaleParameter"),
    "Normalize": ("norm_param", "NormalizeParameter"), "Concat": ("concat_param", "ConcatParameter"),
    "Softmax": ("softmax_param", "SoftmaxParameter"), "Reshape": ("reshape_param", "ReshapeParameter"),
    "Python": ("python_param", "PythonParameter"), "Input": ("input_param", "InputParameter"),
    "Split": (None, None),                                  # (no parameter message)
}
ACCEPTED_TYPES = sorted(TYPE_MESSAGE)                       # what csrc/net_graph.cpp does not answer with "Unsupported layer type"

C, HW = 16, (7, 9)


# ---- layer text ---------------------------------------------------------------------------------------------------------------
def layer(name, type_, bottoms, tops, body=""):
    return 'layer { name: "%s" type: "%s" %s %s %s }\n' % (name, type_, " ".join('bottom: "%s"' % b for b in bottoms),
                                                           " ".join('top: "%s"' % t for t in tops), body)


def conv(name, bottom, fields, type_="Convolution", extra=""):
    return layer(name, type_, [bottom], [name], "convolution_param { %s } %s" % (fields, extra))


PRE = conv("pre", "data", "num_output: %d kernel_size: 1" % C)          # the identity: hands the grid on as NHWC activations
PRE2 = conv("pre2", "data", "num_output: %d kernel_size: 1" % C)         # a second, different map (a permutation)


def net(layers_txt, h=HW[0], w=HW[1]):
    return H.single_layer_net(PRE + layers_txt, C, h, w)


def g(fields):
    return net(conv("g", "pre", fields))


def up(fields):
    return net(conv("up", "pre", fields, "Deconvolution"))


# ---- value cases: (scope, field) proven by `text`, which must differ from `twin` (the field at its default, or -- where the
#      schema has no default -- at another value) -------------------------------------------------------------------------------
class Value(object):
    def __init__(self, scope, fields, text, twin):
        self.scope, self.fields, self.text, self.twin = scope, tuple(fields), text, twin


_DC = "num_output: %d group: %d " % (C, C)
VALUE_CASES = {
    "conv_num_output": Value("Convolution", ["num_output"], g("num_output: 12 kernel_size: 1"), g("num_output: 8 kernel_size: 1")),
    "conv_kernel_size": Value("Convolution", ["kernel_size"], g("num_output: 8 kernel_size: 3"), g("num_output: 8 kernel_size: 1")),
    "conv_pad": Value("Convolution", ["pad"], g("num_output: 8 kernel_size: 3 pad: 2"), g("num_output: 8 kernel_size: 3")),
    "conv_stride": Value("Convolution", ["stride"], g("num_output: 8 kernel_size: 3 pad: 1 stride: 2"), g("num_output: 8 kernel_size: 3 pad: 1")),
    "conv_dilation": Value("Convolution", ["dilation"], g("num_output: 8 kernel_size: 3 pad: 1 dilation: 2"), g("num_output: 8 kernel_size: 3 pad: 1")),
    "conv_bias_term": Value("Convolution", ["bias_term"], g("num_output: 8 kernel_size: 3 pad: 1 bias_term: false"), g("num_output: 8 kernel_size: 3 pad: 1")),
    "conv_bias_term_spelling": Value("Convolution", ["bias_term"], g("num_output: 8 kernel_size: 3 pad: 1 bias_term: False"), g("num_output: 8 kernel_size: 3 pad: 1")),
    "conv_kernel_hw": Value("Convolution", ["kernel_h", "kernel_w"], g("num_output: 8 kernel_h: 3 kernel_w: 3"), g("num_output: 8 kernel_size: 1")),
    "conv_pad_hw": Value("Convolution", ["pad_h", "pad_w"], g("num_output: 8 kernel_size: 3 pad_h: 1 pad_w: 1"), g("num_output: 8 kernel_size: 3")),
    "conv_stride_hw": Value("Convolution", ["stride_h", "stride_w"], g("num_output: 8 kernel_size: 3 stride_h: 2 stride_w: 2"), g("num_output: 8 kernel_size: 3")),
    "conv_kernel_size_twice": Value("Convolution", ["kernel_size"], g("num_output: 8 kernel_size: 3 kernel_size: 3"), g("num_output: 8 kernel_size: 1")),
    "conv_pad_twice": Value("Convolution", ["pad"], g("num_output: 8 kernel_size: 3 pad: 1 pad: 1"), g("num_output: 8 kernel_size: 3")),
    "conv_stride_twice": Value("Convolution", ["stride"], g("num_output: 8 kernel_size: 3 stride: [2, 2]"), g("num_output: 8 kernel_size: 3")),
    "conv_dilation_twice": Value("Convolution", ["dilation"], g("num_output: 8 kernel_size: 3 dilation: 2 dilation: 2"), g("num_output: 8 kernel_size: 3")),
    "conv_all_hw": Value("Convolution", ["kernel_h", "kernel_w", "pad_h", "pad_w", "stride_h", "stride_w"],
                         g("num_output: 8 kernel_h: 3 kernel_w: 3 pad_h: 1 pad_w: 1 stride_h: 2 stride_w: 2"), g("num_output: 8 kernel_size: 1")),
    "conv_group": Value("Convolution", ["group"], g("num_output: %d kernel_size: 3 pad: 1 group: %d" % (C, C)), g("num_output: %d kernel_size: 3 pad: 1" % C)),
    "deconv_kernel_size": Value("Deconvolution", ["kernel_size"], up(_DC + "kernel_size: 4 stride: 2 pad: 1"), up(_DC + "kernel_size: 2 stride: 2 pad: 0")),
    "deconv_pad": Value("Deconvolution", ["pad"], up(_DC + "kernel_size: 4 stride: 2 pad: 1"), up(_DC + "kernel_size: 4 stride: 2")),
    "deconv_stride": Value("Deconvolution", ["stride"], up(_DC + "kernel_size: 4 stride: 2 pad: 1"), up(_DC + "kernel_size: 4 pad: 1")),
    "deconv_bias_term": Value("Deconvolution", ["bias_term"], up(_DC + "kernel_size: 4 stride: 2 pad: 1 bias_term: false"), up(_DC + "kernel_size: 4 stride: 2 pad: 1")),
    "deconv_hw": Value("Deconvolution", ["kernel_h", "kernel_w", "pad_h", "pad_w", "stride_h", "stride_w"],
                       up(_DC + "kernel_h: 4 kernel_w: 4 stride_h: 2 stride_w: 2 pad_h: 1 pad_w: 1"), up(_DC + "kernel_size: 2")),
    "deconv_twice": Value("Deconvolution", ["kernel_size", "pad", "stride"], up(_DC + "kernel_size: [4, 4] stride: [2, 2] pad: [1, 1]"), up(_DC + "kernel_size: 2")),
    "concat_axis_negative": Value("Concat", ["axis"],
                                  net(PRE2 + layer("cat", "Concat", ["pre", "pre2"], ["cat"], "concat_param { axis: -3 }")),
                                  net(PRE2 + layer("cat", "Concat", ["pre2", "pre"], ["cat"], "concat_param { axis: 1 }"))),
    "net_input_dim": Value("Net", ["input_dim"],
                           'name: "t"\ninput: "data"\ninput_dim: 1\ninput_dim: %d\ninput_dim: 7\ninput_dim: 9\n' % C + PRE + conv("g", "pre", "num_output: 8 kernel_size: 3"),
                           'name: "t"\ninput: "data"\ninput_shape { dim: 1 dim: %d dim: 9 dim: 7 }\n' % C + PRE + conv("g", "pre", "num_output: 8 kernel_size: 3")),
    "concat_dim": Value("Concat", ["concat_dim"],
                        net(PRE2 + layer("cat", "Concat", ["pre", "pre2"], ["cat"], "concat_param { concat_dim: 1 }")),
                        net(PRE2 + layer("cat", "Concat", ["pre2", "pre"], ["cat"]))),
}
# (concat_axis_negative / concat_dim: outside a proposal tail only the channel axis has a kernel, so the non-default spelling
#  is what is honoured -- -3 and concat_dim: 1 are axis 1; the twin swaps the bottoms, so that a Concat that did nothing, or took
#  the members in another order, differs.  The class-score Concat of a tail on axis 2, and concat_dim: 2 in its place, are
#  TAIL_TWINS below.)

# A tail's class-score Concat written with the legacy field: the same blobs and outputs as with `axis: 2`
TAIL_TWINS = {
    "concat_dim_tail": ("concat_param { axis: 2 }", "concat_param { concat_dim: 2 }"),
}


def tail_text(old=None, new=None):
    """`helpers.mini_detector`'s per-blob tail on two 128-channel maps of 7 x 9 (the logits kernel's vector width is 128)."""
    txt = H.mini_detector(conv("f0", "data", "num_output: 128 kernel_size: 1") + conv("f1", "data", "num_output: 128 kernel_size: 1"),
                          ["f0", "f1"], 8, C, HW[0], HW[1])
    if old is not None:
        assert txt.count(old) == 1, old
        txt = txt.replace(old, new)
    return txt


# ---- refusals -----------------------------------------------------------------------------------------------------------------
class Refusal(object):
    """`text` is refused at caffe.Net() with a message matching `match` (a regex naming the layer and the field).  `python`:
    smallhardface_amd.prototxt.normalize_graph -- the path weights.py and the oracle nets read through -- refuses it too."""

    def __init__(self, text, match, python=True):
        self.text, self.match, self.python = text, match, python


def _tail_with(old, new):
    return tail_text(old, new)


_PRED = 'name: "cls_score_0" type: "Convolution" bottom: "f0" top: "cls_score_0_output" convolution_param { num_output: 2 kernel_size: 1 pad: 0 stride: 1 }'
_BN = layer("bn", "BatchNorm", ["pre"], ["bn"], "batch_norm_param { %s }")
REFUSALS = {
    # Convolution / Deconvolution: what only a rectangular kernel could compute
    "conv_kernel_hw_rect": Refusal(g("num_output: 8 kernel_h: 3 kernel_w: 5"), r"'g'.*rectangular kernel_h / kernel_w \(3 x 5\) not supported"),
    "conv_kernel_size_rect": Refusal(g("num_output: 8 kernel_size: 3 kernel_size: 5"), r"'g'.*rectangular kernel_size \(3 x 5\) not supported"),
    "conv_pad_hw_rect": Refusal(g("num_output: 8 kernel_size: 3 pad_h: 1 pad_w: 0"), r"'g'.*rectangular pad_h / pad_w \(1 x 0\) not supported"),
    "conv_pad_rect": Refusal(g("num_output: 8 kernel_size: 3 pad: 1 pad: 0"), r"'g'.*rectangular pad \(1 x 0\) not supported"),
    "conv_stride_hw_rect": Refusal(g("num_output: 8 kernel_size: 3 stride_h: 1 stride_w: 2"), r"'g'.*rectangular stride_h / stride_w \(1 x 2\) not supported"),
    "conv_stride_rect": Refusal(g("num_output: 8 kernel_size: 3 stride: 1 stride: 2"), r"'g'.*rectangular stride \(1 x 2\) not supported"),
    "conv_dilation_rect": Refusal(g("num_output: 8 kernel_size: 3 dilation: 1 dilation: 2"), r"'g'.*rectangular dilation \(1 x 2\) not supported"),
    "deconv_kernel_hw_rect": Refusal(up(_DC + "kernel_h: 4 kernel_w: 2 stride: 2"), r"'up'.*rectangular kernel_h / kernel_w \(4 x 2\) not supported"),
    # ... and Caffe's own CHECKs (base_conv_layer.cpp:26-108)
    "conv_kernel_both": Refusal(g("num_output: 8 kernel_size: 3 kernel_h: 3 kernel_w: 3"), r"'g'.*both kernel_size and kernel_h / kernel_w"),
    "conv_pad_both": Refusal(g("num_output: 8 kernel_size: 3 pad: 1 pad_h: 1 pad_w: 1"), r"'g'.*both pad and pad_h / pad_w"),
    "conv_stride_both": Refusal(g("num_output: 8 kernel_size: 3 stride: 1 stride_h: 1 stride_w: 1"), r"'g'.*both stride and stride_h / stride_w"),
    "conv_kernel_h_alone": Refusal(g("num_output: 8 kernel_h: 3"), r"'g'.*kernel_h without kernel_w"),
    "conv_pad_w_alone": Refusal(g("num_output: 8 kernel_size: 3 pad_w: 1"), r"'g'.*pad_w without pad_h"),
    "conv_stride_h_alone": Refusal(g("num_output: 8 kernel_size: 3 stride_h: 2"), r"'g'.*stride_h without stride_w"),
    "conv_kernel_size_thrice": Refusal(g("num_output: 8 kernel_size: 3 kernel_size: 3 kernel_size: 3"), r"'g'.*kernel_size given 3 times"),
    "conv_dilation_thrice": Refusal(g("num_output: 8 kernel_size: 3 dilation: [1, 1, 1]"), r"'g'.*dilation given 3 times"),
    "conv_no_kernel": Refusal(g("num_output: 8 pad: 1"), r"'g'.*no filter size.*kernel_size"),
    "conv_axis": Refusal(g("num_output: 8 kernel_size: 3 axis: 2"), r"'g'.*axis 2"),
    "conv_force_nd_im2col": Refusal(g("num_output: 8 kernel_size: 3 force_nd_im2col: true"), r"'g'.*force_nd_im2col"),
    "deconv_dilation": Refusal(up(_DC + "kernel_size: 4 stride: 2 pad: 1 dilation: 2"), r"'up'.*dilation 2.*Deconvolution"),
    "deconv_num_output": Refusal(up("num_output: 8 group: 8 kernel_size: 4 stride: 2 pad: 1"), r"Deconvolution 'up'.*depthwise \(group == channels\)", python=False),
    "deconv_group": Refusal(up("num_output: %d group: 4 kernel_size: 4 stride: 2 pad: 1" % C), r"Deconvolution 'up'.*depthwise \(group == channels\)", python=False),
    # values that are not of the field's type
    "type_kernel_size_real": Refusal(g("num_output: 8 kernel_size: 3.7"), r"'g'.*kernel_size: '3.7' is not an integer"),
    "type_pad_word": Refusal(g("num_output: 8 kernel_size: 3 pad: x"), r"'g'.*pad: 'x' is not an integer"),
    "type_stride_quoted": Refusal(g('num_output: 8 kernel_size: 3 stride: "2"'), r"'g'.*stride: '2' is not an integer"),
    "type_num_output_exp": Refusal(g("num_output: 8.0 kernel_size: 3"), r"'g'.*num_output: '8.0' is not an integer"),
    "type_bias_term_upper": Refusal(g("num_output: 8 kernel_size: 3 bias_term: TRUE"), r"'g'.*bias_term: 'TRUE' is not a bool"),
    "type_bias_term_yes": Refusal(g("num_output: 8 kernel_size: 3 bias_term: yes"), r"'g'.*bias_term: 'yes' is not a bool"),
    "type_slope_word": Refusal(net(layer("r", "ReLU", ["pre"], ["r"], "relu_param { negative_slope: abc }")), r"'r'.*negative_slope: 'abc' is not a number"),
    "type_eps_tail": Refusal(net(_BN % "eps: 1e-5x"), r"'bn'.*eps: '1e-5x' is not a number"),
    "type_global_pooling": Refusal(net(K.pool_txt("p", "pre", "AVE", extra=" global_pooling: on")), r"'p'.*global_pooling: 'on' is not a bool"),
    "type_pool_kernel": Refusal(net(K.pool_txt("p", "pre", "MAX", extra=" kernel_size: 2.0")), r"'p'.*kernel_size: '2.0' is not an integer"),
    "type_crop_offset": Refusal(net(PRE2 + layer("c", "Crop", ["pre", "pre2"], ["c"], "crop_param { offset: 1.5 }")), r"'c'.*offset: '1.5' is not an integer"),
    "type_coeff": Refusal(net(PRE2 + layer("e", "Eltwise", ["pre", "pre2"], ["e"], "eltwise_param { coeff: one coeff: 1 }")), r"'e'.*coeff: 'one' is not a number"),
    "type_concat_axis": Refusal(net(PRE2 + layer("cat", "Concat", ["pre", "pre2"], ["cat"], "concat_param { axis: 1.0 }")), r"'cat'.*axis: '1.0' is not an integer"),
    "type_input_dim": Refusal(H.single_layer_net(PRE, C, 7, 9).replace("dim: 7", "dim: 7.5"), r"input_shape.dim: '7.5' is not an integer"),
    # the other parameter messages
    "concat_axis_and_dim": Refusal(net(PRE2 + layer("cat", "Concat", ["pre", "pre2"], ["cat"], "concat_param { axis: 1 concat_dim: 1 }")),
                                   r"Concat 'cat'.*both axis and concat_dim"),
    "concat_axis_spatial": Refusal(net(PRE2 + layer("cat", "Concat", ["pre", "pre2"], ["cat"], "concat_param { axis: 2 }")),
                                   r"Concat 'cat'.*axis 2.*only channel concat", python=False),
    "concat_dim_spatial": Refusal(net(PRE2 + layer("cat", "Concat", ["pre", "pre2"], ["cat"], "concat_param { concat_dim: 3 }")),
                                  r"Concat 'cat'.*axis 3.*only channel concat", python=False),
    "scale_axis": Refusal(net(layer("s", "Scale", ["pre"], ["s"], "scale_param { axis: 2 }")), r"Scale 's'.*axis 2", python=False),
    "scale_num_axes": Refusal(net(layer("s", "Scale", ["pre"], ["s"], "scale_param { num_axes: 2 }")), r"Scale 's'.*num_axes 2", python=False),
    "bn_batch_stats": Refusal(net(_BN % "use_global_stats: false"), r"BatchNorm 'bn'.*use_global_stats", python=False),
    "normalize_across_spatial": Refusal(net(layer("n", "Normalize", ["pre"], ["n"], "norm_param { across_spatial: true }")),
                                        r"Normalize 'n'.*across_spatial", python=False),
    "python_other_layer": Refusal(net(layer("py", "Python", ["pre"], ["py"], 'python_param { module: "m" layer: "Other" }')),
                                  r"Python layer 'py'.*only ProposalLayer", python=False),
    "softmax_axis": Refusal(_tail_with('top: "cls_prob_output" }', 'top: "cls_prob_output" softmax_param { axis: 2 } }'), r"Softmax 'cls_prob'.*axis 2"),
    "reshape_axis": Refusal(_tail_with("reshape_param { shape { dim: 0 dim: 4 dim: -1 dim: 0 } }", "reshape_param { axis: 1 shape { dim: 0 dim: 4 dim: -1 dim: 0 } }"),
                            r"Reshape 'cls_prob_reshape'.*axis 1"),
    "reshape_num_axes": Refusal(_tail_with("reshape_param { shape { dim: 0 dim: 4 dim: -1 dim: 0 } }", "reshape_param { num_axes: 2 shape { dim: 0 dim: 4 dim: -1 dim: 0 } }"),
                                r"Reshape 'cls_prob_reshape'.*num_axes 2"),
    # a predictor fused into a proposal tail is a matrix product per pixel
    "tail_predictor_stride": Refusal(_tail_with(_PRED, _PRED.replace("stride: 1", "stride: 2")), r"ProposalLayer 'proposal'.*'cls_score_0' has stride 2", python=False),
    "tail_predictor_pad": Refusal(_tail_with(_PRED, _PRED.replace("pad: 0", "pad: 1")), r"ProposalLayer 'proposal'.*'cls_score_0' has pad 1", python=False),
    "tail_predictor_kernel": Refusal(_tail_with(_PRED, _PRED.replace("kernel_size: 1 pad: 0", "kernel_size: 3 pad: 1")),
                                     r"ProposalLayer 'proposal'.*'cls_score_0'.*kernel_size 3.*1x1", python=False),
    # layer types with no launch of their own outside a tail
    "free_softmax": Refusal(net(layer("sm", "Softmax", ["pre"], ["sm"])), r"Softmax 'sm'.*only inside a proposal tail", python=False),
    "free_reshape": Refusal(net(layer("rs", "Reshape", ["pre"], ["rs"], "reshape_param { shape { dim: 0 dim: -1 dim: 1 dim: 0 } }")),
                            r"Reshape 'rs'.*only inside a proposal tail", python=False),
    "free_split": Refusal(net(layer("sp", "Split", ["pre"], ["sp_a", "sp_b"])), r"Split 'sp'.*only inside a proposal tail", python=False),
    # layer- and net-level rules
    "layer_include": Refusal(net(conv("g", "pre", "num_output: 8 kernel_size: 1", extra="include { phase: TRAIN }")), r"'g'.*include rules"),
    "layer_exclude": Refusal(net(conv("g", "pre", "num_output: 8 kernel_size: 1", extra="exclude { phase: TEST }")), r"'g'.*exclude rules"),
    "layer_phase": Refusal(net(conv("g", "pre", "num_output: 8 kernel_size: 1", extra="phase: TRAIN")), r"'g'.*phase TRAIN"),
    "layer_blobs": Refusal(net(conv("g", "pre", "num_output: 8 kernel_size: 1", extra="blobs { shape { dim: 1 } data: 1 }")), r"'g'.*inline blobs"),
    "layer_type": Refusal(net(layer("lrn", "LRN", ["pre"], ["lrn"])), r"Unsupported layer type 'LRN' \(layer 'lrn'\)", python=False),
    "net_layers": Refusal(net("") + 'layers { name: "old" type: RELU bottom: "pre" top: "pre" }\n', r"legacy V1 'layers'"),
}
# accepted spellings that must keep constructing (a refusal must not catch them)
ACCEPTED = {
    "phase_test": net(conv("g", "pre", "num_output: 8 kernel_size: 1", extra="phase: TEST")),
    "bool_t": g("num_output: 8 kernel_size: 1 bias_term: t"),
    "bool_0": g("num_output: 8 kernel_size: 1 bias_term: 0"),
    "float_suffix": net(layer("r", "ReLU", ["pre"], ["r"], "relu_param { negative_slope: 0.5f }")),
    "axis_minus_3": g("num_output: 8 kernel_size: 1 axis: -3"),
    "deconv_dilation_1": up(_DC + "kernel_size: 4 stride: 2 pad: 1 dilation: 1"),
}

# values that are not of their field's type, for the independent reader (oracle/graph_reader.py): each raises GraphError
ILL_TYPED = [
    g("num_output: 8 kernel_size: 3.7"), g("num_output: 8 kernel_size: 3 pad: x"), g("num_output: 8 kernel_size: 3 pad: -1"),
    g('num_output: 8 kernel_size: 3 stride: "2"'), g("num_output: 1e1 kernel_size: 3"), g("num_output: 8 kernel_size: 3 bias_term: TRUE"),
    g("num_output: 8 kernel_size: 3 axis: x"), g("num_output: 8 kernel_size: 3 dilation: 4294967296"),
    net(layer("r", "ReLU", ["pre"], ["r"], "relu_param { negative_slope: abc }")), net(_BN % "eps: 1e-5x"),
    net(K.pool_txt("p", "pre", "AVE", extra=" global_pooling: on")), net(K.pool_txt("p", "pre", "MEDIAN", k=2)),
    net(PRE2 + layer("c", "Crop", ["pre", "pre2"], ["c"], "crop_param { axis: 2.0 }")),
    net(PRE2 + layer("cat", "Concat", ["pre", "pre2"], ["cat"], "concat_param { concat_dim: -1 }")),
    H.single_layer_net(PRE, C, 7, 9).replace("dim: 7", "dim: 7.5"), net(conv("g", "pre", "num_output: 8 kernel_size: 1", extra="name: g2")),
]


# ---- the dispositions ---------------------------------------------------------------------------------------------------------
def _h(case):
    return (HONOURED, case)


def _r(case):
    return (REFUSED, case)


def _i(why):
    return (INERT, why)


_FILLER = "initialises a training run; the fresh blob holds Caffe's default filler's value already and a caffemodel brings the rest"


def _conv_fields(t):
    p = "conv_" if t == "Convolution" else "deconv_"
    d = {
        "num_output": _h("conv_num_output") if t == "Convolution" else _r("deconv_num_output"),
        "group": _h("conv_group") if t == "Convolution" else _r("deconv_group"),
        "bias_term": _h(p + "bias_term"), "kernel_size": _h(p + "kernel_size"), "pad": _h(p + "pad"), "stride": _h(p + "stride"),
        "dilation": _h("conv_dilation") if t == "Convolution" else _r("deconv_dilation"),
        "weight_filler": _i(_FILLER + " (constant 0)"), "bias_filler": _i(_FILLER + " (constant 0)"),
        "engine": _i("picks Caffe's or cuDNN's implementation of the same function"),
        "axis": _r("conv_axis"), "force_nd_im2col": _r("conv_force_nd_im2col"),
    }
    hw = "conv_%s_hw" if t == "Convolution" else "deconv_hw"
    for f in ("kernel", "pad", "stride"):
        d[f + "_h"] = d[f + "_w"] = _h(hw % f if t == "Convolution" else hw)
    return d


_POOL = "tests.pooling_cases:WINDOW_CASES"
_PER_TYPE = {
    "Convolution": _conv_fields("Convolution"),
    "Deconvolution": _conv_fields("Deconvolution"),
    "Pooling": dict([(f, _h(_POOL)) for f in ("pool", "pad", "pad_h", "pad_w", "kernel_size", "kernel_h", "kernel_w", "stride", "stride_h", "stride_w")] +
                    [("global_pooling", _h("tests.pooling_cases:GLOBAL_CASES")), ("engine", _i("picks Caffe's or cuDNN's implementation of the same function"))]),
    "ReLU": {"negative_slope": _h("tests.test_gpu_fusion_layers:test_relu_in_place_and_not"),
             "engine": _i("picks Caffe's or cuDNN's implementation of the same function")},
    "Eltwise": {"operation": _h("tests.test_gpu_fusion_layers:test_eltwise_operations"), "coeff": _h("tests.test_gpu_fusion_layers:test_eltwise_operations"),
                "stable_prod_grad": _i("chooses how the backward pass of PROD divides: no forward effect")},
    "Crop": {"axis": _h("tests.test_gpu_fusion_layers:test_crop_is_an_exact_copy"), "offset": _h("tests.test_gpu_fusion_layers:test_crop_is_an_exact_copy")},
    "BatchNorm": {"use_global_stats": _r("bn_batch_stats"), "eps": _h("tests.norm_cases:FOLD_CASES"),
                  "moving_average_fraction": _i("the decay of the running statistics while training; inference reads the stored ones")},
    "Scale": {"axis": _r("scale_axis"), "num_axes": _r("scale_num_axes"), "bias_term": _h("tests.norm_cases:FOLD_VARIANTS"),
              "filler": _i(_FILLER + " (constant 1)"), "bias_filler": _i(_FILLER + " (constant 0)")},
    "Normalize": {"across_spatial": _r("normalize_across_spatial"), "channel_shared": _h("tests.l2norm_cases:LAYER_CASES"),
                  "eps": _h("tests.l2norm_cases:LAYER_CASES"), "scale_filler": _h("tests.l2norm_cases:filler_params")},
    "Concat": {"axis": _h("concat_axis_negative"), "concat_dim": _h("concat_dim")},
    "Softmax": {"axis": _r("softmax_axis"), "engine": _i("picks Caffe's or cuDNN's implementation of the same function")},
    "Reshape": {"shape": _h("tests.multiclass_cases:tail"), "axis": _r("reshape_axis"), "num_axes": _r("reshape_num_axes")},
    "Python": {"layer": _r("python_other_layer"), "param_str": _h("tests.modules_cases:module_tail"),
               "module": _i("names the Python file of the reference's layer; the native ProposalLayer is chosen by `layer`"),
               "share_in_parallel": _i("shares one layer object between the nets of a multi-GPU training run")},
    "Input": {"shape": _h("tests.buffer_history_cases:CASES")},
}

_OWN = "read by its layer type, whose fields are classified under that type; on a layer of another type Caffe never looks at it"
_FOREIGN = "the parameter message of a layer type that is refused by type (Refusal layer_type); on an accepted type Caffe never looks at it"
_LAYER = {
    "name": _h("tests.buffer_history_cases:CASES"), "type": _r("layer_type"), "bottom": _h("tests.buffer_history_cases:CASES"),
    "top": _h("tests.buffer_history_cases:CASES"), "phase": _r("layer_phase"), "include": _r("layer_include"), "exclude": _r("layer_exclude"),
    "blobs": _r("layer_blobs"), "param": _h("tests.test_gpu_fused_forms:GRAPHS"),
    "loss_weight": _i("weighs a top in the training objective"), "propagate_down": _i("prunes the backward pass"),
    "transform_param": _i("read by data layers only, which are refused by type"),
    "loss_param": _i("read by loss layers only, which are refused by type"),
}
_NET = {
    "name": _i("a label for logs and drawings; nothing reads it"), "input": _h("tests.buffer_history_cases:CASES"), "input_shape": _h("tests.buffer_history_cases:CASES"),
    "input_dim": _h("net_input_dim"), "layer": _h("tests.buffer_history_cases:CASES"), "layers": _r("net_layers"),
    "force_backward": _i("forces a backward pass to be planned; nothing here runs one"),
    "state": _i("phase / level / stage select layers through include and exclude rules, and every layer that has a rule is refused"),
    "debug_info": _i("prints blob statistics while Caffe runs"),
}


def dispositions(census):
    """DISPOSITION for the fields of `census` (tests/golden/caffe_layer_fields.json): the tables above, plus LayerParameter's
    `*_param` fields by rule -- an accepted type's own message, or a refused type's."""
    own = {pf for pf, _ in TYPE_MESSAGE.values() if pf}
    d = {}
    for t, fields in _PER_TYPE.items():
        for f, v in fields.items():
            d[(t, f)] = v
    for f, v in _LAYER.items():
        d[("Layer", f)] = v
    for f in census["LayerParameter"]:
        if f.endswith("_param") and f not in _LAYER:
            d[("Layer", f)] = _i(_OWN if f in own else _FOREIGN)
    for f, v in _NET.items():
        d[("Net", f)] = v
    return d


def census():
    import json
    import os
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "caffe_layer_fields.json")) as f:
        return json.load(f)


DISPOSITION = dispositions(census())


# ---- parameters, data and the float64 reference -------------------------------------------------------------------------------
def case_params(text, seed=0):
    """Integer parameters for every layer of `text`, shaped by the independent reader: `pre` the identity, `pre2` a
    permutation, `f0` / `f1` selections, convolutions weights in [-2, 2] and biases in [-8, 8], BatchNorm mean in [-3, 3] with
    variance 4 and factor 1, Scale gamma in [-2, 2] without 0 and beta in [-4, 4], Normalize a scale of 2."""
    graph = R.read(text)
    rng = np.random.default_rng(1234 + seed)
    out = {}
    for name, shapes in graph.param_shapes().items():
        L = graph.layer(name)
        if name in ("pre", "pre2", "f0", "f1"):
            co, ci = shapes[0][:2]
            w = np.zeros(shapes[0], F32)
            perm = np.arange(co) % ci if name == "pre" else np.random.default_rng(len(name) + co).permutation(max(co, ci))[:co] % ci
            w[np.arange(co), perm, 0, 0] = 1.0
            out[name] = [w] + [np.zeros(s, F32) for s in shapes[1:]]
        elif L.type in ("Convolution", "Deconvolution"):
            out[name] = [rng.integers(-2, 3, shapes[0]).astype(F32)] + [rng.integers(-8, 9, s).astype(F32) for s in shapes[1:]]
        elif L.type == "BatchNorm":
            out[name] = [rng.integers(-3, 4, shapes[0]).astype(F32), np.full(shapes[1], 4, F32), np.ones(shapes[2], F32)]
        elif L.type == "Scale":
            out[name] = [rng.choice([-2, -1, 1, 2], shapes[0]).astype(F32)] + [rng.integers(-4, 5, s).astype(F32) for s in shapes[1:]]
        elif L.type == "Normalize":
            out[name] = [np.full(shapes[0], 2, F32)]
    return out


def case_data(text, seed=0, unit=False):
    """Integers in [-4, 4] (`unit`: +-1, so that a 16-channel pixel has the L2 norm 4), and im_info."""
    shape = R.read(text).inputs["data"]
    rng = np.random.default_rng(99 + seed)
    data = (rng.integers(0, 2, shape) * 2 - 1 if unit else rng.integers(-4, 5, shape)).astype(F32)
    return data, np.array([[shape[2], shape[3], 1.0]], F32)


def case_inputs(text, seed=0, unit=False):
    """forward()'s keyword arguments: `data`, and `im_info` where the net declares it."""
    data, info = case_data(text, seed, unit)
    return dict(data=data, im_info=info) if "im_info" in R.read(text).inputs else dict(data=data)


def _conv64(x, w, b, hp, deconv):
    """Caffe's (de)convolution in binary64 with the reader's per-axis geometry: (top, sum of |products| + |bias|)."""
    (kh, kw), (sh, sw), (ph, pw), (dh, dw), grp = hp["kernel"], hp["stride"], hp["pad"], hp["dilation"], hp["group"]
    cin, hh, ww = x.shape
    nout = hp["num_output"]
    eh, ew = dh * (kh - 1) + 1, dw * (kw - 1) + 1
    ho, wo = ((sh * (hh - 1) + eh - 2 * ph, sw * (ww - 1) + ew - 2 * pw) if deconv else ((hh + 2 * ph - eh) // sh + 1, (ww + 2 * pw - ew) // sw + 1))
    top, mag = np.zeros((nout, ho, wo), F64), np.zeros((nout, ho, wo), F64)
    cig, cog = cin // grp, nout // grp
    for gi in range(grp):
        xs = x[gi * cig:(gi + 1) * cig].astype(F64)
        for ky in range(kh):
            for kx in range(kw):
                if deconv:       # weight (cin, nout / group, kh, kw): input pixel (y, x) adds into (y * s - p + ky * d, ...)
                    wk = w[gi * cig:(gi + 1) * cig, :, ky, kx].astype(F64)                     # (cig, cog)
                    for y in range(hh):
                        oy = y * sh - ph + ky * dh
                        if not 0 <= oy < ho:
                            continue
                        for xx in range(ww):
                            ox = xx * sw - pw + kx * dw
                            if 0 <= ox < wo:
                                top[gi * cog:(gi + 1) * cog, oy, ox] += wk.T @ xs[:, y, xx]
                                mag[gi * cog:(gi + 1) * cog, oy, ox] += np.abs(wk).T @ np.abs(xs[:, y, xx])
                else:            # weight (nout, cin / group, kh, kw): output pixel (oy, ox) reads (oy * s - p + ky * d, ...)
                    wk = w[gi * cog:(gi + 1) * cog, :, ky, kx].astype(F64)                     # (cog, cig)
                    for oy in range(ho):
                        y = oy * sh - ph + ky * dh
                        if not 0 <= y < hh:
                            continue
                        for ox in range(wo):
                            xx = ox * sw - pw + kx * dw
                            if 0 <= xx < ww:
                                top[gi * cog:(gi + 1) * cog, oy, ox] += wk @ xs[:, y, xx]
                                mag[gi * cog:(gi + 1) * cog, oy, ox] += np.abs(wk) @ np.abs(xs[:, y, xx])
    if b is not None:
        top += b.astype(F64)[:, None, None]
        mag += np.abs(b.astype(F64))[:, None, None]
    return top, mag


def reference(text, params, data):
    """Every blob of `text` in binary64, geometry from oracle/graph_reader.py: ({blob: (1, C, H, W) array}, the largest sum of
    magnitudes any dot product reaches).  Plain loops; batch 1."""
    graph = R.read(text)
    B = {"data": np.asarray(data, F64)}
    worst = 0.0
    for L in graph.layers:
        hp = L.hp
        if L.type == "Input":
            continue
        x = [B[b] for b in L.bottoms]
        if L.type in ("Convolution", "Deconvolution"):
            p = params[L.name]
            assert len(p) == 1 + hp["bias_term"] and hp["axis"] in (1, -3)
            top, mag = _conv64(x[0][0], p[0], p[1] if hp["bias_term"] else None, hp, L.type == "Deconvolution")
            worst = max(worst, float(mag.max()))
            out = top[None]
        elif L.type == "ReLU":
            out = np.maximum(x[0], 0) + hp["negative_slope"] * np.minimum(x[0], 0)
        elif L.type == "Pooling":
            k = hp["kernel"] or x[0].shape[2:]
            out = K.pool_ref(x[0].astype(F32), hp["pool"], k[0], k[1], hp["stride"][0], hp["stride"][1], hp["pad"][0], hp["pad"][1],
                             hp["global_pooling"], f64=True)[0].astype(F64)
        elif L.type == "Eltwise":
            if hp["operation"] == "SUM":
                out = sum(c * v for c, v in zip(hp["coeff"] or [1.0] * len(x), x))
            elif hp["operation"] == "PROD":
                out = np.prod(x, axis=0)
            else:
                out = np.max(x, axis=0)
        elif L.type == "Crop":
            ax = R.canonical_axis(hp["axis"], 4, L.name)
            off = [0 if i < ax else (0 if not hp["offset"] else hp["offset"][0] if len(hp["offset"]) == 1 else hp["offset"][i - ax]) for i in range(4)]
            size = [x[0].shape[i] if i < ax else x[1].shape[i] for i in range(4)]
            out = x[0][tuple(slice(o, o + s) for o, s in zip(off, size))]
        elif L.type == "BatchNorm":
            mean, var, f = [v.astype(F64) for v in params[L.name]]
            out = (x[0] - (mean / f[0])[None, :, None, None]) / np.sqrt(var / f[0] + hp["eps"])[None, :, None, None]
        elif L.type == "Scale":
            p = params[L.name]
            out = x[0] * p[0].astype(F64)[None, :, None, None] + (p[1].astype(F64)[None, :, None, None] if hp["bias_term"] else 0)
        elif L.type == "Normalize":
            assert not hp["across_spatial"]
            out = x[0] / np.sqrt((x[0] ** 2).sum(axis=1, keepdims=True) + hp["eps"]) * params[L.name][0].astype(F64).reshape(1, -1, 1, 1)
        elif L.type == "Concat":
            out = np.concatenate(x, axis=R.canonical_axis(hp["axis"], 4, L.name))
        else:
            raise NotImplementedError(L.type)
        B[L.tops[0]] = np.ascontiguousarray(out, F64)
    return B, worst


def on_grid(v):
    """Every value is a multiple of 1/4 below 2^11 in magnitude: its own fp16 value (and so its own split-fp16 high half, its own
    fp32 and bf16-summable operand); sums of products of such values below 2^24 are exact in every arithmetic the kernels use."""
    v = np.asarray(v, F64)
    return bool(np.all(v * 4 == np.round(v * 4)) and np.all(np.abs(v) < 2048))


# ---- every accepted layer type in a stand-alone position: its top is a net output ---------------------------------------------
_CONV3 = "num_output: 8 kernel_size: 3 pad: 1"
STANDALONE = {          # type -> (text, outputs compared, unit data)
    "Convolution": (g(_CONV3), ["g"], False),
    "Deconvolution": (up(_DC + "kernel_size: 4 stride: 2 pad: 1"), ["up"], False),
    "ReLU": (net(layer("r", "ReLU", ["pre"], ["r"], "relu_param { negative_slope: 0.25 }")), ["r"], False),
    "Pooling": (net(K.pool_txt("pm", "pre", "MAX", k=3, stride=2) + K.pool_txt("pa", "pre", "AVE", k=2, stride=2)), ["pm", "pa"], False),
    "Eltwise": (net(PRE2 + layer("e", "Eltwise", ["pre", "pre2"], ["e"], "eltwise_param { operation: SUM coeff: 2 coeff: -1 }")), ["e"], False),
    "Crop": (net(conv("small", "pre", "num_output: %d kernel_size: 3" % C) + layer("c", "Crop", ["pre", "small"], ["c"], "crop_param { axis: 2 offset: 1 offset: 2 }")), ["c"], False),
    "BatchNorm": (net(layer("bn", "BatchNorm", ["pre"], ["bn"], "batch_norm_param { eps: 0 }")), ["bn"], False),
    "Scale": (net(layer("s", "Scale", ["pre"], ["s"], "scale_param { bias_term: true }")), ["s"], False),
    "Normalize": (net(layer("n", "Normalize", ["pre"], ["n"], "norm_param { across_spatial: false channel_shared: false eps: 0 }")), ["n"], True),
    "Concat": (net(PRE2 + layer("cat", "Concat", ["pre", "pre2"], ["cat"])), ["cat"], False),
    "Input": (H.single_layer_net("", C, HW[0], HW[1]).replace('input: "data"\ninput_shape { dim: 1 dim: %d dim: %d dim: %d }\n' % (C, HW[0], HW[1]), "") +
              'layer { name: "in" type: "Input" top: "data" input_param { shape { dim: 1 dim: %d dim: %d dim: %d } } }\n' % (C, HW[0], HW[1]) +
              PRE, ["pre"], False),
}
STANDALONE_REFUSED = {"Softmax": "free_softmax", "Reshape": "free_reshape", "Split": "free_split"}
STANDALONE_TAIL = ("Python",)       # a ProposalLayer IS the tail: its tops are written by it (every tail test reads them)


# ---- INTEGRATION.md's table of refused and inert fields (tests/test_graph_fields_host.py holds the document to it) -------------
_REFUSED_WHEN = {
    "deconv_num_output": "other than the bottom's channel count (only depthwise)", "deconv_group": "other than the bottom's channel count (only depthwise)",
    "deconv_dilation": "other than 1", "conv_axis": "other than 1 (or -3)", "conv_force_nd_im2col": "`true`",
    "bn_batch_stats": "`false` (batch statistics are training)", "scale_axis": "other than 1 (or -3)", "scale_num_axes": "other than 1",
    "normalize_across_spatial": "`true`, which is also its default: write `across_spatial: false`", "softmax_axis": "other than 1 (or -3)",
    "reshape_axis": "other than 0", "reshape_num_axes": "other than -1", "python_other_layer": "other than `ProposalLayer`",
    "layer_type": "any type outside this table's", "layer_phase": "other than `TEST`", "layer_include": "present", "layer_exclude": "present",
    "layer_blobs": "present", "net_layers": "present (V1 layers)",
}


def integration_table():
    lines = ["| where | field | disposition | when / why |", "|---|---|---|---|"]
    foreign = []
    for (scope, field), (kind, what) in sorted(DISPOSITION.items(), key=lambda kv: (kv[0][0] in ("Layer", "Net"), kv[0])):
        if kind == HONOURED:
            continue
        if kind == INERT and what == _FOREIGN:
            foreign.append(field)
            continue
        where = {"Layer": "any layer", "Net": "the net"}.get(scope, scope)
        lines.append("| %s | `%s` | %s | %s |" % (where, field, kind.lower(), _REFUSED_WHEN[what] if kind == REFUSED else what))
    lines.append("| any layer | the `*_param` message of a type outside this table (%d fields, `%s` ... `%s`) | inert | %s |"
                 % (len(foreign), foreign[0], foreign[-1], _FOREIGN))
    return "\n".join(lines)

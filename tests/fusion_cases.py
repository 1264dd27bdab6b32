"""References and graphs for the layers that fuse maps by addition (tests/test_fusion_layers_host.py,
tests/test_gpu_fusion_layers.py): Eltwise, Crop and a ReLU that is not the in-place one behind a Convolution.  Everything
here runs without a GPU.

The numpy references state Caffe's layers in fp32, operation for operation:

``eltwise``  eltwise_layer.cpp:42-80.  SUM: ``top = 0; top += coeff[i] * bottom[i]`` in bottom order, every product and every
             add rounded to fp32 (coeff absent: all 1); PROD and MAX left to right, MAX with the layer's ``a > b ? a : b``.
``crop``     crop_layer.cpp:36-130: axes from ``axis`` on take the reference blob's size, from ``offset`` (none: 0; one: the
             same for every cropped axis; else one per cropped axis).
``relu``     relu_layer.cpp:9-19: ``max(x, 0) + negative_slope * min(x, 0)``, one product.

``FusionOracleNet`` walks a graph like ``oracle.OracleNet`` (whose convolution, deconvolution, pooling and proposal
functions it calls) and knows the three layers above; an in-place layer replaces its blob, a Concat copies, so a member
read after an in-place ReLU on the Concat's top still holds its pre-activation values.

``m1_shaped(h, w)``: the stride-8 branch of an SSH detector.  The VGG trunk of ``build_test_template`` up to conv5_3, 1x1
reductions of conv4_3 and conv5_3 to 128 channels, the deep one up-sampled by a depthwise Deconvolution (kernel 4, stride 2,
pad 1), Cropped to the shallow one's size, the two added by an Eltwise SUM, a 3x3 convolution, a context module (a 3x3
branch of 128 channels and two of 64 behind a shared 3x3 reduction, none with a ReLU of its own) ending in Concat + in-place
ReLU, and one ProposalLayer at stride 8 on the 256-channel result.
"""
import numpy as np

from oracle import oracle as O
from smallhardface_amd import prototxt as P
from tests import modules_cases as MC

F32 = np.float32

M1_MODULES = {"1": (["m1_out"], 2, "{'feat_stride': [8,8],'scales': [1,2], 'ratios':[1,]}")}


# ---- references ---------------------------------------------------------------------------------------------------------------
def eltwise(bottoms, op="SUM", coeff=None):
    bottoms = [np.asarray(b, F32) for b in bottoms]
    assert 2 <= len(bottoms) and all(b.shape == bottoms[0].shape for b in bottoms)
    if op == "SUM":
        coeff = [1.0] * len(bottoms) if coeff is None else coeff
        assert len(coeff) == len(bottoms)
        acc = np.zeros_like(bottoms[0])
        for c, b in zip(coeff, bottoms):
            acc = (acc + (F32(c) * b).astype(F32)).astype(F32)
        return acc
    assert coeff is None
    acc = bottoms[0]
    if op == "PROD":
        for b in bottoms[1:]:
            acc = (acc * b).astype(F32)
        return acc
    assert op == "MAX"
    acc = np.where(bottoms[0] > bottoms[1], bottoms[0], bottoms[1])
    for b in bottoms[2:]:
        acc = np.where(b > acc, b, acc)
    return acc.astype(F32)


def crop_origin(axis, offset, ndim=4):
    offset = list(offset)
    assert len(offset) in (0, 1, ndim - axis)
    return [0 if ax < axis else (0 if not offset else offset[0] if len(offset) == 1 else offset[ax - axis]) for ax in range(ndim)]


def crop(x, ref_shape, axis=2, offset=()):
    x = np.asarray(x, F32)
    org = crop_origin(axis, offset, x.ndim)
    size = [x.shape[ax] if ax < axis else ref_shape[ax] for ax in range(x.ndim)]
    assert all(o >= 0 and o + s <= d for o, s, d in zip(org, size, x.shape))
    return np.ascontiguousarray(x[tuple(slice(o, o + s) for o, s in zip(org, size))])


def relu(x, slope=0.0):
    x = np.asarray(x, F32)
    zero = F32(0)
    return (np.where(x < zero, zero, x) + (F32(slope) * np.where(zero < x, zero, x)).astype(F32)).astype(F32)


# ---- layer text ---------------------------------------------------------------------------------------------------------------
def eltwise_layer(name, bottoms, top=None, op=None, coeff=None, extra=""):
    param = ""
    if op is not None or coeff is not None or extra:
        param = " eltwise_param {%s%s%s }" % ("" if op is None else " operation: %s" % op,
                                              "".join(" coeff: %r" % float(c) for c in (coeff or [])), extra)
    return 'layer { name: "%s" type: "Eltwise" %s top: "%s"%s }\n' % (
        name, " ".join('bottom: "%s"' % b for b in bottoms), top or name, param)


def crop_layer(name, bottom, ref, top=None, axis=None, offset=()):
    param = ""
    if axis is not None or offset:
        param = " crop_param {%s%s }" % ("" if axis is None else " axis: %d" % axis, "".join(" offset: %d" % o for o in offset))
    return 'layer { name: "%s" type: "Crop" bottom: "%s" bottom: "%s" top: "%s"%s }\n' % (name, bottom, ref, top or name, param)


def relu_layer(name, bottom, top=None, slope=None):
    param = "" if slope is None else " relu_param { negative_slope: %s }" % (slope if isinstance(slope, str) else repr(float(slope)))
    return 'layer { name: "%s" type: "ReLU" bottom: "%s" top: "%s"%s }\n' % (name, bottom, top or bottom, param)


def conv_layer(name, bottom, nout, k, relu_=False, top=None):
    top = top or name
    s = ('layer { name: "%s" type: "Convolution" bottom: "%s" top: "%s" convolution_param { num_output: %d kernel_size: %d '
         'pad: %d } }\n' % (name, bottom, top, nout, k, k // 2))
    return s + (relu_layer(name + "_relu", top) if relu_ else "")


def deconv_layer(name, bottom, C, k=4, stride=2, pad=1, bias=False):
    return ('layer { name: "%s" type: "Deconvolution" bottom: "%s" top: "%s" convolution_param { kernel_size: %d stride: %d '
            'num_output: %d group: %d pad: %d%s } }\n' % (name, bottom, name, k, stride, C, C, pad, "" if bias else " bias_term: false"))


def pool_layer(name, bottom, k=2, stride=2, pad=0):
    return ('layer { name: "%s" type: "Pooling" bottom: "%s" top: "%s" pooling_param { pool: MAX kernel_size: %d stride: %d '
            'pad: %d } }\n' % (name, bottom, name, k, stride, pad))


def concat_layer(name, bottoms, top=None):
    return 'layer { name: "%s" type: "Concat" %s top: "%s" concat_param { axis: 1 } }\n' % (
        name, " ".join('bottom: "%s"' % b for b in bottoms), top or name)


# ---- the oracle net -------------------------------------------------------------------------------------------------------------
def _ints(msg, name, default):
    v = msg.getall(name) if msg is not None else []
    return int(v[0]) if v else default


class FusionOracleNet(O.OracleNet):
    """``oracle.OracleNet`` plus Eltwise, Crop and ReLU with a slope.  ``snapshots[(layer name, blob name)]`` keeps what every
    layer wrote, so that the value of a blob BEFORE a later in-place layer rewrote it stays at hand."""

    def forward(self, **kwargs):
        if kwargs:
            assert set(kwargs.keys()) == set(self.inputs)
            for in_, blob in kwargs.items():
                self.blobs[in_].data[...] = blob
        B = self.blobs
        self.snapshots = {}
        for L in self.layers:
            t, name = str(L.get("type")), str(L.get("name"))
            bots = [B[str(b)].data for b in L.getall("bottom")]
            tops = [str(x) for x in L.getall("top")]
            if t == "Input":
                continue
            if t == "Convolution":
                cp, p = L.get("convolution_param"), self.params[name]
                out = O.convolution(bots[0], p[0], p[1] if len(p) > 1 else None, pad=_ints(cp, "pad", 0), stride=_ints(cp, "stride", 1),
                                    dil=_ints(cp, "dilation", 1), group=_ints(cp, "group", 1))
            elif t == "Deconvolution":
                cp, p = L.get("convolution_param"), self.params[name]
                out = O.deconvolution(bots[0], p[0], p[1] if len(p) > 1 else None, pad=_ints(cp, "pad", 0),
                                      stride=_ints(cp, "stride", 1), group=_ints(cp, "group", 1))
            elif t == "ReLU":
                rp = L.get("relu_param")
                out = relu(bots[0], float(rp.get("negative_slope", 0.0)) if rp is not None else 0.0)
            elif t == "Pooling":
                pq = L.get("pooling_param")
                assert str(pq.get("pool", "MAX")) == "MAX"
                out = O.max_pool(bots[0], _ints(pq, "kernel_size", 2), _ints(pq, "stride", 1), _ints(pq, "pad", 0))
            elif t == "Concat":
                out = np.concatenate(bots, axis=_ints(L.get("concat_param"), "axis", 1))
            elif t == "Eltwise":
                ep = L.get("eltwise_param")
                op = str(ep.get("operation", "SUM")) if ep is not None else "SUM"
                coeff = [float(c) for c in ep.getall("coeff")] if ep is not None else []
                out = eltwise(bots, op, coeff or None)
            elif t == "Crop":
                cp = L.get("crop_param")
                out = crop(bots[0], bots[1].shape, _ints(cp, "axis", 2), [int(o) for o in cp.getall("offset")] if cp is not None else [])
            elif t == "Softmax":
                out = O.softmax(bots[0], axis=_ints(L.get("softmax_param"), "axis", 1))
            elif t == "Reshape":
                dims = [int(d) for d in L.get("reshape_param").get("shape").getall("dim")]
                out = bots[0].reshape(O.caffe_reshape(bots[0].shape, dims))
            elif t == "Python":
                pstr = O._parse_param_str(str(L.get("python_param").get("param_str")))
                pp = O.ProposalParams(feat_stride=pstr.get("feat_stride"), scales=pstr.get("scales", (8, 16, 32)),
                                      ratios=pstr.get("ratios", (0.5, 1, 2)), base_size=pstr.get("base_size", 16),
                                      shifts=pstr.get("shifts", [0]), subsampled=pstr.get("subsampled", True),
                                      num_feats=pstr.get("num_feats", 1), pre_nms_topN=self.pp.pre_nms_topN,
                                      score_thresh=self.pp.score_thresh, min_size=self.pp.min_size)
                boxes, probs = O.proposal_forward(bots[-3], bots[-2], bots[-1], pp)
                B[tops[0]].data = boxes
                if len(tops) > 1:
                    B[tops[1]].data = probs
                continue
            else:
                raise NotImplementedError("fusion oracle: layer type %s" % t)
            B[tops[0]].data = np.ascontiguousarray(out, dtype=F32)
            self.snapshots[(name, tops[0])] = B[tops[0]].data
        return {o: B[o].data for o in self.outputs}


# ---- graphs ---------------------------------------------------------------------------------------------------------------------
def chain_text(h, w, C=128, slope=None, head=True):
    """The fold under test on a 3-channel image of h x w: c0 (64) -> `hi` (C channels, h x w) -> 2x2 pool -> `lo` (C channels at
    the ceil-halved size); `lo` is up-sampled (kernel 4, stride 2, pad 1: twice its size, which is h x w rounded up to even),
    Cropped to `hi`'s size and added to it; an in-place ReLU (`slope`) follows and the 3x3 convolution `fuse` reads the sum.
    With `head` a single-blob proposal tail sits on `fuse`, so that a split-fp16 forward takes the fused path."""
    from tests import helpers as H
    txt = (conv_layer("c0", "data", 64, 3, True) + conv_layer("hi", "c0", C, 3, True) + pool_layer("p", "hi") +
           conv_layer("lo", "p", C, 3, True) + deconv_layer("up", "lo", C) + crop_layer("up_crop", "up", "hi") +
           eltwise_layer("sum", ["hi", "up_crop"]) + relu_layer("sum_relu", "sum", slope=slope) + conv_layer("fuse", "sum", 128, 3, True))
    if not head:
        return H.single_layer_net(txt, 3, h, w)
    return H.mini_detector(txt, "fuse", 8, 3, h, w)


def m1_shaped(h=64, w=96):
    """(Msg) the M1-shaped graph at input size h x w (see the module docstring)."""
    tmpl = P.build_test_template(False)
    net = P.Msg()
    for k, v in tmpl.fields:
        if k == "layer" and str(v.get("name")) == "conv5_256":
            break
        net.add(k, v)
    extra = (conv_layer("conv4_128", "conv4_3", 128, 1, True) + conv_layer("conv5_128", "conv5_3", 128, 1, True) +
             deconv_layer("conv5_128_up", "conv5_128", 128) + crop_layer("conv5_128_crop", "conv5_128_up", "conv4_128", axis=2, offset=(0,)) +
             eltwise_layer("conv4_fuse", ["conv4_128", "conv5_128_crop"], op="SUM") +
             conv_layer("conv4_fuse_final", "conv4_fuse", 128, 3, True) +
             conv_layer("m1_3x3", "conv4_fuse_final", 128, 3) + conv_layer("m1_dimred", "conv4_fuse_final", 64, 3, True) +
             conv_layer("m1_5x5", "m1_dimred", 64, 3) + conv_layer("m1_7x7_1", "m1_dimred", 64, 3, True) +
             conv_layer("m1_7x7", "m1_7x7_1", 64, 3) + concat_layer("m1_out", ["m1_3x3", "m1_5x5", "m1_7x7"]) +
             relu_layer("m1_out_relu", "m1_out") + MC.module_tail("1", *M1_MODULES["1"]))
    msg = P.parse(P.dumps(net) + "\n" + extra)
    msg.set_nth("input_shape", 0, P.Msg([("dim", 1), ("dim", 3), ("dim", h), ("dim", w)]))
    return msg

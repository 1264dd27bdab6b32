"""Caffe prototxt (protobuf text format) handling for the inference graph.

Replaces, for the inference path only, what the reference does with
``caffe_pb2`` + ``google.protobuf.text_format`` in
/root/reference/lib/prototxt/manipulate.py:

  * ``parse`` / ``dumps``      -- a small text-format reader/writer (no protoc in
    this image, so no generated ``caffe_pb2``);
  * ``manipulate_test``        -- manipulate.py:63-86: pick the template, insert the
    ``conv4_fuse_final_dim_red`` 512->128 3x3 conv + ReLU in front of the heads
    (``_add_dimension_reduction``, manipulate.py:166-188), write ``test.prototxt``;
  * ``build_test_template``    -- emits the detection graph the reference ships as
    models/test_different_dilation_template.prototxt / models/test_template.prototxt
    (VGG-16 trunk :17-367, unified head :369-478, heads + proposal :479-697), so the
    repo can run without the reference tree.  ``tests/test_prototxt.py`` checks it
    is structurally identical to the reference files when they are present.
"""
import re

from .config import cfg


class Enum(str):
    """A bare identifier value (``MAX``, ``true``) as opposed to a quoted string."""


class Msg(object):
    """Ordered multi-map: a protobuf message in text form."""

    def __init__(self, fields=None):
        self.fields = list(fields or [])  # [(name, value)]

    # -- access -----------------------------------------------------------
    def getall(self, name):
        return [v for k, v in self.fields if k == name]

    def get(self, name, default=None):
        for k, v in self.fields:
            if k == name:
                return v
        return default

    def has(self, name):
        return any(k == name for k, _ in self.fields)

    def add(self, name, value):
        self.fields.append((name, value))
        return value

    def set(self, name, value):
        for i, (k, _) in enumerate(self.fields):
            if k == name:
                self.fields[i] = (name, value)
                return
        self.fields.append((name, value))

    def set_nth(self, name, n, value):
        c = 0
        for i, (k, _) in enumerate(self.fields):
            if k == name:
                if c == n:
                    self.fields[i] = (name, value)
                    return
                c += 1
        raise IndexError(name)

    def clear(self, name):
        self.fields = [(k, v) for k, v in self.fields if k != name]

    def copy(self):
        return Msg([(k, v.copy() if isinstance(v, Msg) else v) for k, v in self.fields])

    def __eq__(self, other):
        return isinstance(other, Msg) and self.fields == other.fields

    def __repr__(self):
        return "Msg(%r)" % (self.fields,)


_TOKEN = re.compile(r"""
    \s+ | \#[^\n]* |
    (?P<str>"(?:\\.|[^"\\])*"|'(?:\\.|[^'\\])*') |
    (?P<punct>[{}:\[\],;<>]) |
    (?P<atom>[^\s{}:\[\],;<>"'#]+)
""", re.X)


def _tokens(text):
    pos = 0
    out = []
    while pos < len(text):
        m = _TOKEN.match(text, pos)
        if not m:
            raise ValueError("prototxt: bad character at offset %d: %r" % (pos, text[pos:pos + 20]))
        pos = m.end()
        if m.group("str") is not None:
            s = m.group("str")
            body = s[1:-1]
            body = re.sub(r"\\(.)", lambda mm: {"n": "\n", "t": "\t"}.get(mm.group(1), mm.group(1)), body)
            out.append(("str", body))
        elif m.group("punct") is not None:
            out.append(("punct", m.group("punct")))
        elif m.group("atom") is not None:
            out.append(("atom", m.group("atom")))
    return out


def _scalar(kind, tok):
    if kind == "str":
        return tok
    try:
        return int(tok)
    except ValueError:
        pass
    try:
        return float(tok)
    except ValueError:
        return Enum(tok)


def parse(text):
    """Parse protobuf text format into a ``Msg`` tree."""
    toks = _tokens(text)
    i = 0

    def message(close):
        nonlocal i
        msg = Msg()
        while i < len(toks):
            kind, tok = toks[i]
            if kind == "punct" and tok in (close or ""):
                i += 1
                return msg
            if kind == "punct" and tok in ",;":
                i += 1
                continue
            if kind != "atom":
                raise ValueError("prototxt: expected field name, got %r" % (tok,))
            name = tok
            i += 1
            kind, tok = toks[i]
            if kind == "punct" and tok == ":":
                i += 1
                kind, tok = toks[i]
            if kind == "punct" and tok in "{<":
                i += 1
                msg.add(name, message("}" if tok == "{" else ">"))
            elif kind == "punct" and tok == "[":
                i += 1
                while True:
                    kind, tok = toks[i]
                    i += 1
                    if kind == "punct" and tok == "]":
                        break
                    if kind == "punct" and tok == ",":
                        continue
                    msg.add(name, _scalar(kind, tok))
            else:
                i += 1
                val = _scalar(kind, tok)
                # adjacent string literals concatenate
                while kind == "str" and i < len(toks) and toks[i][0] == "str":
                    val += toks[i][1]
                    i += 1
                msg.add(name, val)
        if close:
            raise ValueError("prototxt: unterminated message")
        return msg

    return message(None)


def _fmt_scalar(v):
    if isinstance(v, Enum):
        return str(v)
    if isinstance(v, bool):
        return "true" if v else "false"
    if isinstance(v, str):
        return '"%s"' % v.replace("\\", "\\\\").replace('"', '\\"').replace("\n", "\\n")
    if isinstance(v, float):
        return repr(v) if v != int(v) else ("%.1f" % v if abs(v) < 1e16 else repr(v))
    return str(v)


def dumps(msg, indent=0):
    """Serialise a ``Msg`` tree the way ``str(pb_message)`` lays text format out."""
    pad = "  " * indent
    out = []
    for k, v in msg.fields:
        if isinstance(v, Msg):
            out.append("%s%s {\n%s%s}\n" % (pad, k, dumps(v, indent + 1), pad))
        else:
            out.append("%s%s: %s\n" % (pad, k, _fmt_scalar(v)))
    return "".join(out)


# --------------------------------------------------------------------------
# manipulate.py equivalents
# --------------------------------------------------------------------------
def _simple_conv_layer(name, bottom, top, num_output, kernel_size, pad, dilation=1,
                       std=0.01, bias=0.0, param_type=0):
    """manipulate.py:89-146 (same field order as the reference builds them)."""
    L = Msg()
    L.add("name", name)
    L.add("type", "Convolution")
    L.add("bottom", bottom)
    L.add("top", top)
    mults = {0: None, 1: ((1.0, 0.0), (2.0, 0.0)), 2: ((1.0, 1.0), (2.0, 0.0)),
             3: ((10.0, 1.0), (20.0, 0.0)), 4: ((1.0, 1.0), (2.0, 1.0))}[param_type]
    for j in range(2):
        p = Msg()
        if mults is not None:
            p.add("lr_mult", mults[j][0])
            p.add("decay_mult", mults[j][1])
        L.add("param", p)
    cp = Msg()
    cp.add("num_output", num_output)
    cp.add("pad", pad)
    cp.add("kernel_size", kernel_size)
    wf = Msg([("type", "gaussian"), ("std", std)])
    cp.add("weight_filler", wf)
    bf = Msg([("type", "constant"), ("value", bias)])
    cp.add("bias_filler", bf)
    cp.add("dilation", dilation)
    L.add("convolution_param", cp)
    return L


def _simple_relu_layer(name, bottom, top=None):
    """manipulate.py:149-155."""
    return Msg([("name", name), ("type", "ReLU"), ("bottom", bottom),
                ("top", top if top is not None else bottom)])


def _add_dimension_reduction(pb):
    """manipulate.py:166-188: 512->128 3x3 reduction in front of the first ``head*`` layer."""
    if not cfg.MODEL.DIFFERENT_DILATION.ENABLE:
        return pb
    layers = pb.getall("layer")
    split = min(i for i, x in enumerate(layers) if str(x.get("name", "")).startswith("head"))
    assert layers[split - 2].get("name") == "conv4_fuse_final"
    layers[split - 2].set_nth("top", 0, layers[split - 2].get("top") + "_tmp")
    layers[split - 1].set_nth("bottom", 0, layers[split - 1].get("bottom") + "_tmp")
    layers[split - 1].set_nth("top", 0, layers[split - 1].get("top") + "_tmp")
    new_layers = layers[:split] + [
        _simple_conv_layer("conv4_fuse_final_dim_red", "conv4_fuse_final_tmp",
                           "conv4_fuse_final", 128, 3, 1, param_type=4),
        _simple_relu_layer("conv4_fuse_final_dim_red_relu", "conv4_fuse_final"),
    ] + layers[split:]
    # ClearField('layer') + extend(): the layers end up after every other field
    pb.clear("layer")
    for L in new_layers:
        pb.add("layer", L)
    return pb


def manipulate_test(ori, target_test, **kwargs):
    """manipulate.py:63-86 without the cosmetic ``draw_net_to_file`` / tensorboard image.

    ``ori`` may be a path or ``None``/missing file, in which case the built-in
    template generator supplies the graph (the reference forces the template path
    when DIFFERENT_DILATION is enabled, manipulate.py:65-66).
    """
    import os
    if cfg.MODEL.DIFFERENT_DILATION.ENABLE:
        ori = 'models/test_different_dilation_template.prototxt'
    if ori and os.path.isfile(ori):
        with open(ori, 'r') as f:
            test_pb = parse(f.read())
    else:
        test_pb = build_test_template(bool(cfg.MODEL.DIFFERENT_DILATION.ENABLE))
    test_pb = _add_dimension_reduction(test_pb)
    with open(target_test, 'w') as f:
        f.write(dumps(test_pb))
    return None


# --------------------------------------------------------------------------
# the detection graph
# --------------------------------------------------------------------------
def _frozen(n):
    return [Msg([("lr_mult", 0), ("decay_mult", 0)]) for _ in range(n)]


def _conv(name, bottom, top, nout, k, pad, params, fillers=True, extra=None, flat=False):
    L = Msg([("name", name), ("type", "Convolution"), ("bottom", bottom), ("top", top)])
    for p in params:
        L.add("param", p)
    cp = Msg()
    cp.add("num_output", nout)
    if flat:  # the heads write kernel_size first, then pad/stride
        cp.add("kernel_size", k)
        cp.add("pad", pad)
        cp.add("stride", 1)
    else:
        cp.add("pad", pad)
        cp.add("kernel_size", k)
    for kk, vv in (extra or []):
        cp.add(kk, vv)
    if fillers:
        cp.add("weight_filler", Msg([("type", "gaussian"), ("std", 0.01)]))
        cp.add("bias_filler", Msg([("type", "constant"), ("value", 0)]))
    L.add("convolution_param", cp)
    return L


def _relu(name, blob):
    return Msg([("name", name), ("type", "ReLU"), ("bottom", blob), ("top", blob)])


def build_test_template(different_dilation=True):
    """The TEST-phase graph of the detector as a ``Msg`` (NetParameter)."""
    net = Msg()
    net.add("name", "face")
    net.add("input", "data")
    net.add("input_shape", Msg([("dim", 1), ("dim", 3), ("dim", 224), ("dim", 224)]))
    net.add("input", "im_info")
    net.add("input_shape", Msg([("dim", 1), ("dim", 3)]))
    # VGG-16 trunk
    prev = "data"
    cfg_vgg = [(1, 64, 2), (2, 128, 2), (3, 256, 3), (4, 512, 3), (5, 512, 3)]
    for stage, ch, n in cfg_vgg:
        for j in range(1, n + 1):
            name = "conv%d_%d" % (stage, j)
            pr = _frozen(2) if stage <= 2 else [Msg([("lr_mult", 1)]), Msg([("lr_mult", 2)])]
            net.add("layer", _conv(name, prev, name, ch, 3, 1, pr, fillers=False))
            net.add("layer", _relu("relu%d_%d" % (stage, j), name))
            prev = name
        if stage < 5:
            pool = "pool%d" % stage
            net.add("layer", Msg([("name", pool), ("type", "Pooling"), ("bottom", prev), ("top", pool),
                                  ("pooling_param", Msg([("pool", Enum("MAX")), ("kernel_size", 2),
                                                         ("stride", 2)]))]))
            prev = pool
    lr12 = lambda: [Msg([("lr_mult", 1)]), Msg([("lr_mult", 2)])]
    # unified head
    net.add("layer", _conv("conv5_256", "conv5_3", "conv5_256", 256, 1, 0, lr12()))
    net.add("layer", _relu("conv5_256_relu", "conv5_256"))
    net.add("layer", Msg([
        ("name", "conv5_256_up"), ("type", "Deconvolution"), ("bottom", "conv5_256"),
        ("top", "conv5_256_up"),
        ("convolution_param", Msg([("kernel_size", 4), ("stride", 2), ("num_output", 256),
                                   ("group", 256), ("pad", 1),
                                   ("weight_filler", Msg([("type", "bilinear")])),
                                   ("bias_term", Enum("false"))])),
        ("param", Msg([("lr_mult", 0), ("decay_mult", 0)]))]))
    net.add("layer", _conv("conv4_256", "conv4_3", "conv4_256", 256, 1, 0, lr12()))
    net.add("layer", _relu("conv4_256_relu", "conv4_256"))
    net.add("layer", Msg([("name", "conv4_fuse"), ("type", "Concat"), ("bottom", "conv5_256_up"),
                          ("bottom", "conv4_256"), ("top", "conv4_fuse"),
                          ("concat_param", Msg([("axis", 1)]))]))
    net.add("layer", _conv("conv4_fuse_final", "conv4_fuse", "conv4_fuse_final", 512, 3, 1, lr12()))
    net.add("layer", _relu("conv4_fuse_final_relu", "conv4_fuse_final"))

    wd = lambda: [Msg([("lr_mult", 1.0), ("decay_mult", 1.0)]), Msg([("lr_mult", 2.0), ("decay_mult", 0)])]
    if different_dilation:
        for d in (1, 2, 4):
            hp = [Msg([("name", "head_w"), ("lr_mult", 1.0), ("decay_mult", 1.0)]),
                  Msg([("name", "head_b"), ("lr_mult", 2.0), ("decay_mult", 0)])]
            L = Msg([("name", "head_%d" % d), ("type", "Convolution"), ("bottom", "conv4_fuse_final"),
                     ("top", "head_%d" % d)])
            for p in hp:
                L.add("param", p)
            L.add("convolution_param", Msg([
                ("num_output", 128), ("kernel_size", 3), ("pad", d), ("stride", 1), ("dilation", d),
                ("weight_filler", Msg([("type", "gaussian"), ("std", 0.01)])),
                ("bias_filler", Msg([("type", "constant"), ("value", 0)]))]))
            net.add("layer", L)
            net.add("layer", _relu("head_%d_relu" % d, "head_%d" % d))
        for d in (1, 2, 4):
            net.add("layer", _conv("cls_score_%d" % d, "head_%d" % d, "cls_score_%d_output" % d,
                                   2, 1, 0, wd(), flat=True))
            net.add("layer", _conv("bbox_pred_%d" % d, "head_%d" % d, "bbox_pred_%d_output" % d,
                                   4, 1, 0, wd(), flat=True))
        L = Msg([("name", "cls_score_output_concat")])
        for d in (1, 2, 4):
            L.add("bottom", "cls_score_%d_output" % d)
        L.add("top", "cls_score_reshape_output")
        L.add("type", "Concat")
        L.add("concat_param", Msg([("axis", 2)]))
        net.add("layer", L)
        L = Msg([("name", "bbox_pred_output_concat")])
        for d in (1, 2, 4):
            L.add("bottom", "bbox_pred_%d_output" % d)
        L.add("top", "bbox_pred_output")
        L.add("type", "Concat")
        L.add("concat_param", Msg([("axis", 1)]))
        net.add("layer", L)
    else:
        net.add("layer", _conv("head", "conv4_fuse_final", "head", 128, 3, 1, wd(), flat=True))
        net.add("layer", _relu("head_relu", "head"))
        net.add("layer", _conv("cls_score", "head", "cls_score_output", 6, 1, 0, wd(), flat=True))
        net.add("layer", _conv("bbox_pred", "head", "bbox_pred_output", 12, 1, 0, wd(), flat=True))
        net.add("layer", Msg([("bottom", "cls_score_output"), ("top", "cls_score_reshape_output"),
                              ("name", "cls_reshape"), ("type", "Reshape"),
                              ("reshape_param", Msg([("shape", Msg([("dim", 0), ("dim", 2), ("dim", -1),
                                                                    ("dim", 0)]))]))]))
    net.add("layer", Msg([("name", "cls_prob"), ("type", "Softmax"),
                          ("bottom", "cls_score_reshape_output"), ("top", "cls_prob_output")]))
    net.add("layer", Msg([("name", "cls_prob_reshape"), ("type", "Reshape"), ("bottom", "cls_prob_output"),
                          ("top", "cls_prob_reshape_output"),
                          ("reshape_param", Msg([("shape", Msg([("dim", 0), ("dim", 6), ("dim", -1),
                                                                ("dim", 0)]))]))]))
    net.add("layer", Msg([
        ("name", "proposal"), ("type", "Python"), ("bottom", "cls_prob_reshape_output"),
        ("bottom", "bbox_pred_output"), ("bottom", "im_info"), ("top", "boxes"), ("top", "cls_prob"),
        ("python_param", Msg([("module", "lib.layers.proposal_layer"), ("layer", "ProposalLayer"),
                              ("param_str", "{'feat_stride': [8,8,8],'scales': [1,2,4], 'ratios':[1,]}")]))]))
    return net


def write_test_prototxt(path, different_dilation=True, dim_red=True):
    """Convenience: template (+ dimension reduction) straight to a file."""
    pb = build_test_template(different_dilation)
    if dim_red and different_dilation:
        old = cfg.MODEL.DIFFERENT_DILATION.ENABLE
        cfg.MODEL.DIFFERENT_DILATION.ENABLE = True
        try:
            pb = _add_dimension_reduction(pb)
        finally:
            cfg.MODEL.DIFFERENT_DILATION.ENABLE = old
    with open(path, "w") as f:
        f.write(dumps(pb))
    return path


# --------------------------------------------------------------------------
# what the graph reader honours and refuses (csrc/net_graph.cpp), for the Python readers of the same text
# --------------------------------------------------------------------------
_TYPED = {
    "convolution_param": dict(num_output="i", bias_term="b", pad="i", kernel_size="i", stride="i", dilation="i", pad_h="i", pad_w="i",
                              kernel_h="i", kernel_w="i", stride_h="i", stride_w="i", group="i", axis="i", force_nd_im2col="b"),
    "pooling_param": dict(pad="i", pad_h="i", pad_w="i", kernel_size="i", kernel_h="i", kernel_w="i", stride="i", stride_h="i",
                          stride_w="i", global_pooling="b"),
    "relu_param": dict(negative_slope="f"), "eltwise_param": dict(coeff="f", stable_prod_grad="b"),
    "crop_param": dict(axis="i", offset="i"),
    "batch_norm_param": dict(use_global_stats="b", moving_average_fraction="f", eps="f"),
    "scale_param": dict(axis="i", num_axes="i", bias_term="b"),
    "norm_param": dict(across_spatial="b", channel_shared="b", eps="f"),
    "concat_param": dict(axis="i", concat_dim="i"), "softmax_param": dict(axis="i"),
    "reshape_param": dict(axis="i", num_axes="i"), "python_param": dict(share_in_parallel="b"),
    "shape": dict(dim="i"), "input_shape": dict(dim="i"), "scale_filler": dict(value="f"),
}
_WHAT = {"i": "an integer", "f": "a number", "b": "a bool (true / false)"}
_BOOLS = {"true": True, "True": True, "t": True, "1": True, "false": False, "False": False, "f": False, "0": False}


def _check_typed(who, mname, msg, depth=0):
    for k, v in msg.fields:
        if isinstance(v, Msg):
            if depth < 3:
                _check_typed(who, k, v, depth + 1)
            continue
        kind = _TYPED.get(mname, {}).get(k)
        if kind is None:
            continue
        bare = not isinstance(v, str) or isinstance(v, Enum)          # (a quoted string is no number)
        if kind == "i":
            ok = bare and isinstance(v, int) and not isinstance(v, bool)
        elif kind == "f":
            ok = bare and (isinstance(v, (int, float)) or re.match(r"^[-+]?(\d+\.?\d*|\.\d+)([eE][-+]?\d+)?[fF]$|^[-+]?(inf|nan)", str(v)) is not None)
        else:
            ok = bare and str(v) in _BOOLS
        if not ok:
            raise ValueError("%s%s.%s: '%s' is not %s" % (who, mname, k, v, _WHAT[kind]))


def as_bool(msg, name, default):
    """A bool field by the spellings protobuf's text format takes."""
    v = msg.get(name) if msg is not None else None
    if v is None:
        return default
    if str(v) not in _BOOLS:
        raise ValueError("%s: '%s' is not a bool" % (name, v))
    return _BOOLS[str(v)]


def _conv_spatial(who, cp, rep, fh, fw, default, required):
    """BaseConvolutionLayer::LayerSetUp's rules (base_conv_layer.cpp:36-117) for one spatial hyper-parameter, square only."""
    vals = [int(v) for v in cp.getall(rep)]
    h, w = (cp.get(fh), cp.get(fw)) if fh else (None, None)
    if h is not None or w is not None:
        hw = "%s / %s" % (fh, fw)
        if vals:
            raise ValueError("%sboth %s and %s given: it is one or the other" % (who, rep, hw))
        if h is None or w is None:
            raise ValueError("%s%s without %s: give both" % ((who,) + ((fh, fw) if h is not None else (fw, fh))))
        if int(h) != int(w):
            raise ValueError("%srectangular %s (%d x %d) not supported: both axes must be equal" % (who, hw, int(h), int(w)))
        return int(h)
    if not vals:
        if required:
            raise ValueError("%sno filter size: give %s, or %s and %s" % (who, rep, fh, fw))
        return default
    if len(vals) > 2:
        raise ValueError("%s%s given %d times: give it once, or once per spatial axis (2)" % (who, rep, len(vals)))
    if len(vals) == 2 and vals[0] != vals[1]:
        raise ValueError("%srectangular %s (%d x %d) not supported: both axes must be equal" % (who, rep, vals[0], vals[1]))
    return vals[0]


def normalize_graph(net_msg):
    """A copy of the net in which every field the Python readers take with ``_ints(msg, name, default)`` holds the value the
    graph reader of the runtime resolves (csrc/net_graph.cpp), and a ValueError in that reader's words for what it refuses:
    a Convolution / Deconvolution ends up with one ``kernel_size``, ``pad``, ``stride`` and ``dilation`` (from the repeated
    fields or the ``*_h`` / ``*_w`` pairs, equal axes only), a Concat with ``axis`` (from ``concat_dim``, negative axes made
    canonical), every bool with ``true`` / ``false``.  ``weights.py`` and the oracle nets read through it, so a field the
    runtime honours is honoured by them and one it refuses is refused by them."""
    if net_msg.has("layers"):
        raise ValueError("net: legacy V1 'layers' entries are not supported: write the net with 'layer' (LayerParameter)")
    for s in net_msg.getall("input_shape"):
        _check_typed("net: ", "input_shape", s)
    out = net_msg.copy()
    for L in out.getall("layer"):
        who = "layer '%s': " % L.get("name", "")
        for f in ("include", "exclude"):
            if L.has(f):
                raise ValueError("%s%s rules are not supported: write the TEST-phase net without them" % (who, f))
        if str(L.get("phase", "TEST")) not in ("TEST", "1"):
            raise ValueError("%sphase %s: only TEST-phase layers are supported" % (who, L.get("phase")))
        if L.has("blobs"):
            raise ValueError("%sinline blobs are not read: give the parameters in a caffemodel or through Net.params" % who)
        _check_typed(who, "layer", L)
        for sub, names in (("convolution_param", ("bias_term",)), ("scale_param", ("bias_term",)),
                           ("pooling_param", ("global_pooling",)), ("norm_param", ("across_spatial", "channel_shared")),
                           ("batch_norm_param", ("use_global_stats",))):
            m = L.get(sub)
            for n in names:
                if m is not None and m.has(n):
                    m.set(n, Enum("true" if as_bool(m, n, None) else "false"))
        t = str(L.get("type"))
        if t in ("Convolution", "Deconvolution") and L.get("convolution_param") is not None:
            cp = L.get("convolution_param")
            k = _conv_spatial(who, cp, "kernel_size", "kernel_h", "kernel_w", 0, True)
            pad = _conv_spatial(who, cp, "pad", "pad_h", "pad_w", 0, False)
            stride = _conv_spatial(who, cp, "stride", "stride_h", "stride_w", 1, False)
            dil = _conv_spatial(who, cp, "dilation", None, None, 1, False)
            axis = int(cp.get("axis", 1))
            if axis not in (1, -3):
                raise ValueError("%saxis %d: only 2-D convolution over the last two axes (axis 1) is supported" % (who, axis))
            if as_bool(cp, "force_nd_im2col", False):
                raise ValueError("%sforce_nd_im2col: true is not supported" % who)
            if t == "Deconvolution" and dil != 1:
                raise ValueError("%sdilation %d: a Deconvolution's dilation must be 1" % (who, dil))
            for n in ("kernel_size", "pad", "stride", "dilation", "kernel_h", "kernel_w", "pad_h", "pad_w", "stride_h", "stride_w"):
                cp.clear(n)
            for n, v in (("kernel_size", k), ("pad", pad), ("stride", stride), ("dilation", dil)):
                cp.add(n, v)
        elif t == "Concat":
            who = "Concat '%s': " % L.get("name", "")
            cc = L.get("concat_param")
            has_dim, has_axis = cc is not None and cc.has("concat_dim"), cc is not None and cc.has("axis")
            if has_dim and has_axis:
                raise ValueError("%sboth axis and concat_dim given: it is one or the other" % who)
            axis = int(cc.get("concat_dim")) if has_dim else int(cc.get("axis")) if has_axis else 1
            if has_dim and axis < 0:
                raise ValueError("%sconcat_dim %d must not be negative" % (who, axis))
            if not 0 <= (axis + 4 if axis < 0 else axis) <= 3:
                raise ValueError("%s%s %d is outside a 4-D blob" % (who, "concat_dim" if has_dim else "axis", axis))
            if cc is None:
                cc = L.add("concat_param", Msg())
            cc.clear("concat_dim")
            cc.clear("axis")
            cc.add("axis", axis + 4 if axis < 0 else axis)
        elif t == "Softmax":
            axis = int(L.get("softmax_param").get("axis", 1)) if L.get("softmax_param") is not None else 1
            if axis not in (1, -3):
                raise ValueError("Softmax '%s': axis %d: only the softmax over axis 1 is supported" % (L.get("name", ""), axis))
        elif t == "Reshape":
            rp = L.get("reshape_param")
            ax, na = (int(rp.get("axis", 0)), int(rp.get("num_axes", -1))) if rp is not None else (0, -1)
            if ax != 0 or na != -1:
                raise ValueError("Reshape '%s': axis %d / num_axes %d: only a reshape of the whole blob (axis 0, num_axes -1) is "
                                 "supported" % (L.get("name", ""), ax, na))
    return out

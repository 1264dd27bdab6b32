"""The graph reader held to Caffe field by field (``-m gpu``).  Cases, dispositions and the float64 reference:
tests/graph_field_cases.py; their CPU half: tests/test_graph_fields_host.py.

  * every HONOURED field: a 16-channel 7 x 9 net with the field at a non-default value, integer operands, forwarded in fp32
    and split-fp16 arithmetic, every blob equal element for element to a binary64 reference whose geometry comes from the
    independent reader (oracle/graph_reader.py) -- exact grids, no tolerance;
  * every REFUSED field: RuntimeError at caffe.Net() naming the layer and the field, and a good net constructs afterwards;
  * every accepted layer type in a stand-alone position with its top as a net output, in a child process whose fresh device
    allocations are NaN (SHF_POISON_ALLOC=255): the top equals the reference, so it was written;
  * the blob and parameter shapes of every graph family (tests/buffer_history_cases.py at its size A) and of both detector
    templates equal the independent reader's -- construction only.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import graph_reader as R
from tests import graph_field_cases as GF
from tests import helpers as H
from tests import test_graph_fields_host as TH

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = ("fp32", "f16x3")
GOOD = GF.g("num_output: 8 kernel_size: 3 pad: 1")


def _net(text, params=None):
    from smallhardface_amd import caffe
    caffe.set_mode_gpu()
    caffe.set_device(0)
    net = caffe.Net(None, prototxt_text=text)
    if params is not None:
        H.load_params(net, params)
    return net


def _assert_equals_reference(net, blobs, inputs, names=None, what=""):
    for mode in MODES:
        net.set_conv_mode(mode)
        out = net.forward(**inputs)
        for name in (names or [n for n in blobs if n != "data"]):
            got = np.asarray(out[name] if name in out else net.blobs[name].data)
            want = blobs[name].astype(np.float32)
            assert got.shape == want.shape, (what, mode, name, got.shape, want.shape)
            np.testing.assert_array_equal(got, want, err_msg="%s %s blob %s" % (what, mode, name))


# ---- C: values ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(GF.VALUE_CASES))
def test_honoured_field_changes_the_result_as_caffe_says(name):
    case = GF.VALUE_CASES[name]
    blobs, _, params, inputs = TH.value_reference(name)
    net = _net(case.text, params)
    graph = R.read(case.text)
    assert {n: tuple(net.blobs[n].shape) for n in graph.blob_shapes() if n in net.blobs} == dict(graph.blob_shapes())
    outputs = [n for n in net.outputs if n in blobs]
    assert graph.layers[-1].tops[0] in outputs
    _assert_equals_reference(net, blobs, inputs, what=name)


@pytest.mark.parametrize("name", sorted(GF.TAIL_TWINS))
def test_legacy_spelling_inside_a_proposal_tail_equals_the_current_one(name):
    """`concat_dim: 2` on a tail's class-score Concat: the blobs the reader derives (the scores stacked along axis 2) and,
    in both conv modes, the outputs of the same net written with `axis: 2`.  With the field ignored the Concat would be on
    axis 1, which the tail refuses."""
    old, new = GF.TAIL_TWINS[name]
    texts = GF.tail_text(), GF.tail_text(old, new)
    params, inputs = GF.case_params(texts[0]), GF.case_inputs(texts[0])
    assert {k: [a.shape for a in v] for k, v in GF.case_params(texts[1]).items()} == {k: [a.shape for a in v] for k, v in params.items()}
    nets = [_net(t, params) for t in texts]
    want = R.read(texts[1]).blob_shapes()
    assert want["cls_score_reshape_output"] == (1, 2, 2 * GF.HW[0], GF.HW[1])
    for n, shp in want.items():
        if shp is not None:
            assert tuple(nets[1].blobs[n].shape) == shp, n
    for mode in MODES:
        outs = []
        for net in nets:
            net.set_conv_mode(mode)
            outs.append(net.forward(**inputs))
        assert sorted(outs[0]) == sorted(outs[1]) and len(outs[0]["boxes"]) > 0
        for k in outs[0]:
            np.testing.assert_array_equal(outs[0][k], outs[1][k], err_msg="%s %s" % (mode, k))


# ---- C: refusals --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(GF.REFUSALS))
def test_refused_field_is_refused_by_layer_and_field(name):
    from smallhardface_amd import caffe
    r = GF.REFUSALS[name]
    with pytest.raises(RuntimeError, match=r.match):
        caffe.Net(None, prototxt_text=r.text)
    good = _net(GOOD)                                   # the process lives on
    assert tuple(good.blobs["g"].shape) == (1, 8) + GF.HW


@pytest.mark.parametrize("name", sorted(GF.ACCEPTED))
def test_spellings_of_text_format_are_accepted(name):
    text = GF.ACCEPTED[name]
    net = _net(text)
    for n, shp in R.read(text).blob_shapes().items():
        assert tuple(net.blobs[n].shape) == shp, n


def test_bool_spellings_mean_what_text_format_says():
    """`bias_term: f` / `0` / `False` make a layer without a bias blob, `t` / `1` / `True` one with it."""
    for word, n in (("f", 1), ("0", 1), ("False", 1), ("false", 1), ("t", 2), ("1", 2), ("True", 2), ("true", 2)):
        net = _net(GF.g("num_output: 8 kernel_size: 1 bias_term: %s" % word))
        assert len(net.params["g"]) == n, word


def test_fresh_parameter_blobs_hold_caffes_default_fillers():
    """What makes the filler fields inert: before a model is loaded a Convolution's and a Deconvolution's blobs are 0 (the
    constant filler's default value), a Scale's gamma 1 and beta 0 (scale_layer.cpp:41-47), whatever filler the text names."""
    filler = "weight_filler { type: \"gaussian\" std: 0.01 } bias_filler { type: \"constant\" value: 0 }"
    net = _net(GF.net(GF.conv("g", "pre", "num_output: 8 kernel_size: 3 pad: 1 " + filler) +
                      GF.conv("up", "pre", GF._DC + "kernel_size: 4 stride: 2 pad: 1 weight_filler { type: \"bilinear\" }", "Deconvolution") +
                      GF.layer("s", "Scale", ["pre"], ["s"], "scale_param { bias_term: true filler { type: \"constant\" value: 1 } }")))
    for name, want in (("g", (0, 0)), ("up", (0, 0)), ("s", (1, 0))):
        for blob, v in zip(net.params[name], want):
            assert np.all(np.asarray(blob.data) == v), (name, v)


# ---- every top is written -----------------------------------------------------------------------------------------------------
def _standalone_child():
    """Runs in a process of its own with SHF_POISON_ALLOC=255: every fresh device allocation is NaN."""
    from smallhardface_amd import _lib, caffe
    caffe.set_mode_gpu()
    caffe.set_device(0)
    assert int(_lib.load().shf_debug_poison_byte()) == 255
    for type_ in sorted(GF.STANDALONE):
        text, outs, unit = GF.STANDALONE[type_]
        params, inputs = GF.case_params(text), GF.case_inputs(text, unit=unit)
        blobs, _ = GF.reference(text, params, inputs["data"])
        net = _net(text, params)
        assert set(outs) <= set(net.outputs), (type_, net.outputs)
        _assert_equals_reference(net, blobs, inputs, names=outs, what=type_)
        print("written: %s %s" % (type_, outs), flush=True)
    for type_, ref in sorted(GF.STANDALONE_REFUSED.items()):
        with pytest.raises(RuntimeError, match=GF.REFUSALS[ref].match):
            caffe.Net(None, prototxt_text=GF.REFUSALS[ref].text)
        print("refused: %s" % type_, flush=True)
    # the ProposalLayer: a tail's tops, and the fused tops read back, hold no poison
    text = GF.tail_text()
    net = _net(text, GF.case_params(text))
    for mode in MODES:
        net.set_conv_mode(mode)
        out = net.forward(**GF.case_inputs(text))
        assert sorted(out) == ["boxes", "cls_prob"] and len(out["boxes"]) > 0
        for name in net.blobs.keys():
            assert np.isfinite(np.asarray(net.blobs[name].data)).all(), (mode, name)
    print("written: Python (tail)", flush=True)


def test_every_accepted_layer_type_writes_its_top():
    env = dict(os.environ, PYTHONPATH=ROOT, SHF_POISON_ALLOC="255")
    code = "from tests import test_gpu_graph_fields as M; M._standalone_child()"
    r = subprocess.run([sys.executable, "-c", code], env=env, cwd=ROOT, capture_output=True, text=True, timeout=300)
    # a child that faulted, aborted or timed out is a finding to be read for its cause, not re-run
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    for type_ in list(GF.STANDALONE) + list(GF.STANDALONE_TAIL):
        assert "written: %s" % type_ in r.stdout, r.stdout
    for type_ in GF.STANDALONE_REFUSED:
        assert "refused: %s" % type_ in r.stdout, r.stdout


# ---- B: shapes ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key,h,w", TH._family_texts(), ids=[k for k, _, _ in TH._family_texts()])
def test_net_shapes_equal_the_independent_readers(key, h, w):
    text, _ = TH.family_setup(key, h, w)
    graph = R.read(text)
    net = _net(text)
    for name, shp in graph.blob_shapes().items():
        if shp is not None:
            assert tuple(net.blobs[name].shape) == tuple(shp), name
    want = {k: [tuple(s) for s in v] for k, v in graph.param_shapes().items()}
    assert {k: [tuple(p.shape) for p in net.params[k]] for k in net.params.keys()} == want

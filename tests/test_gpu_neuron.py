"""The neuron layers (csrc/neuron.hip: neuron_kernel) -- PReLU, Sigmoid, TanH, ELU, AbsVal, Threshold, BNLL, Power, Exp, Log --
through caffe.Net, Net.forward and Net.forward_group (run on an MI355X: ``pytest -m gpu``).  Cases, graphs, references and
bounds: tests/neuron_cases.py; the references on their own: tests/test_neuron_host.py.

Without the layers every test here fails at ``caffe.Net(...)`` ("Unsupported layer type 'PReLU'", ...), the refusals for want
of their texts.

1. The exact ops (PReLU per channel and shared, AbsVal, Threshold 0 and 1.5, Power scale -1, Power scale 3 shift -2) on integer
   grids, every layer case, out of place and in place, Concat members: in conv modes fp32, f16x3 and bf16 value for value equal
   to ``neuron32``; in f64 mode within one fp32 ulp of fp32(``neuron64``), equal where the formula rounds once.
2. PReLU on trained-like grids, fp32 mode: ``neuron32`` bit for bit (one product, one add).
3. The library ops against ``neuron64``: fp32 mode within ``neuron_cases.bound`` (LIB_ULPS as a cap, no margin), f64 mode within
   one fp32 ulp of the rounded reference.  Each case prints the largest error in ulps (DESIGN.md 4.17 records them).
4. The census's value cases and refusals; fillers, shared blobs, caffemodel blobs, commits.
5. Neighbours on the fused path in f16x3; a Sigmoid top as a ProposalLayer's head blob; an in-place PReLU on a Concat's top.
6. ``Power { scale: 1e5 }`` lifts the output beyond 65504 in f16x3: the forward is redone in fp32.
7. forward_group over three lanes bit for bit, the profiler's count per pass, A-B-A buffer history.
8. A MobileFaceNet-shaped mini detector against ``NeuronOracleNet``.
"""
import numpy as np
import pytest

from smallhardface_amd import prototxt as P
from smallhardface_amd.config import cfg
from tests import fusion_cases as F
from tests import general_conv_cases as G
from tests import helpers as H
from tests import neuron_cases as L

pytestmark = pytest.mark.gpu

F32 = np.float32
F64 = np.float64
ACT_TOL = 2e-5          # tests/test_gpu_parity.py
SCORE_TOL = 1e-4
BOX_TOL = 1e-3
FP32_FORM_MODES = ["fp32", "f16x3", "bf16"]
KERNEL = L.KERNEL
FUSE1 = "conv_mfma_f16x3_kernel<64, true, 1, 3, 3, false>"          # tests/test_gpu_fused_forms.py


def W4(split, mt, nt):
    return "conv_mfma_f16x3_w4d_kernel<%s, %d, %d, 3, false, 1>" % ("true" if split else "false", mt, nt)


def _net(text, params):
    from smallhardface_amd import caffe
    net = caffe.Net(None, prototxt_text=text)
    H.load_params(net, params)
    return net


def _info(data):
    return np.array([[data.shape[2], data.shape[3], 1]], F32)


def _forward(net, data, info=None):
    net.blobs["data"].reshape(*data.shape)
    net.blobs["im_info"].reshape(1, 3)
    return {k: np.array(v) for k, v in net.forward(data=data, im_info=_info(data) if info is None else info).items()}


def _blob(net, name):
    return np.array(net.blobs[name].data)


def _bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


def _same(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    np.testing.assert_array_equal(_bits(got), _bits(want), err_msg=str(what))


def _equal(got, want, what):
    """Value for value (bit for bit but for the sign of a zero), and no NaN on either side."""
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert np.isfinite(got).all() and np.isfinite(want).all(), what
    np.testing.assert_array_equal(got, want, err_msg=str(what))


def _within_an_ulp(got, want64, what, equal=False):
    """conv mode f64: one fp32 ulp of the rounded reference; ``equal``: the rounded reference itself."""
    want = want64.astype(F32)
    assert got.shape == want.shape and np.isfinite(got).all(), what
    if equal:
        np.testing.assert_array_equal(got, want, err_msg=str(what))
        return 0
    near = (got == want) | (got == np.nextafter(want, F32(np.inf))) | (got == np.nextafter(want, F32(-np.inf)))
    assert near.all(), (what, int((~near).sum()))
    return int((got != want).sum())


def _profiled(head, fn):
    head.prof_enable(True)
    head.prof_reset()
    try:
        out = fn()
        prof = {k: int(v["launches"]) for k, v in head.prof_read().items()}
    finally:
        head.prof_enable(False)
        head.prof_reset()
    return out, prof


def _copy(params):
    return {k: [np.array(v) for v in blobs] for k, blobs in params.items()}


# ---- 1. the exact ops on integer grids ----------------------------------------------------------------------------------------
def _slope_of(i, sl, shared):
    return {0: sl, 1: shared}.get(i)            # (EXACT_SPECS: op0 is the per-channel PReLU, op1 the shared one)


@pytest.mark.parametrize("in_place", [False, True], ids=["out_of_place", "in_place"])
@pytest.mark.parametrize("case", L.LAYER_CASES, ids=L.case_id)
def test_exact_ops_on_integer_grids_in_every_mode(case, in_place):
    C, h, w = case
    data, sl, shared = L.int_inputs(case)
    params, perm = L.feeder_params(case)
    params.update(op0=[sl], op1=[shared])
    net = _net(L.ops_net_text(case, L.EXACT_SPECS, in_place), params)
    assert tuple(net.params["op0"][0].data.shape) == (C,) and tuple(net.params["op1"][0].data.shape) == ()
    x = data[:, perm]
    want32 = [L.neuron32(s, x, _slope_of(i, sl, shared)) for i, s in enumerate(L.EXACT_SPECS)]
    want64 = [L.neuron64(s, x, _slope_of(i, sl, shared)) for i, s in enumerate(L.EXACT_SPECS)]
    for mode in FP32_FORM_MODES:
        net.set_conv_mode(mode)
        redos = net.range_fallbacks
        _, prof = _profiled(net, lambda: _forward(net, data))
        assert net.range_fallbacks == redos
        assert prof[KERNEL] == len(L.EXACT_SPECS) * (2 if in_place else 1), (mode, prof[KERNEL])     # (in place: the copies too)
        _equal(_blob(net, L.feeder_txt(C)[1]), x, (mode, "the feeder keeps its values"))
        for i, spec in enumerate(L.EXACT_SPECS):
            assert tuple(net.blobs["n%d" % i].shape) == (1, C, h, w)
            _equal(_blob(net, "n%d" % i), want32[i], (mode, L.case_id(case), L.spec_id(spec)))
    net.set_conv_mode("f64")
    _forward(net, data)
    for i, spec in enumerate(L.EXACT_SPECS):
        _within_an_ulp(_blob(net, "n%d" % i), want64[i], ("f64", L.spec_id(spec)), equal=L.single_rounding(spec))


@pytest.mark.parametrize("C", [12, 6])
def test_concat_members_are_exact(C):
    rng = np.random.default_rng(12 + C)
    data = rng.integers(-4, 5, (1, 16, 7, 9)).astype(F32)
    s0, p0 = G.selection(C, 16, seed=5)
    s1, p1 = G.selection(C, 16, seed=6)
    sl0, sl1 = rng.integers(-2, 3, C).astype(F32), rng.integers(-2, 3, C).astype(F32)
    sl1[0], sl1[1] = -2, 0
    spec = ("PReLU", {})
    params = {"pre": G.feeder_params(16, False)[0]["pre"], "s0": [s0, np.zeros(C, F32)], "s1": [s1, np.zeros(C, F32)],
              "n0": [sl0], "n1": [sl1]}
    net = _net(L.concat_net_text(C, spec), params)
    wa, wb = L.neuron32(spec, data[:, p0], sl0), L.neuron32(spec, data[:, p1], sl1)
    assert np.abs(wb).max() > 1 and (wb != data[:, p1]).any()
    for mode in FP32_FORM_MODES + ["f64"]:
        net.set_conv_mode(mode)
        _forward(net, data)
        _equal(_blob(net, "cin"), np.concatenate([data[:, p0], data[:, p1]], axis=1), (mode, "cin"))
        _equal(_blob(net, "b"), wb, (mode, "b"))            # read at coff C of cstride 2 C, written at coff C of cstride 2 C
        _equal(_blob(net, "a"), wa, (mode, "a"))
        _equal(_blob(net, "cat"), np.concatenate([wa, wb], axis=1), (mode, "cat"))


def test_library_op_on_concat_members():
    """The scalar and the vector form of a library op through offset views, against the bound."""
    for C in (12, 6):
        rng = np.random.default_rng(3 + C)
        data = rng.uniform(-8, 8, (1, 16, 7, 9)).astype(F32)
        s0, p0 = G.selection(C, 16, seed=5)
        s1, p1 = G.selection(C, 16, seed=6)
        spec = ("Sigmoid", {})
        net = _net(L.concat_net_text(C, spec), {"pre": G.feeder_params(16, False)[0]["pre"], "s0": [s0, np.zeros(C, F32)], "s1": [s1, np.zeros(C, F32)]})
        _forward(net, data)
        x = np.concatenate([data[:, p0], data[:, p1]], axis=1)
        _same(_blob(net, "cin"), x, "cin")
        err = np.abs(_blob(net, "cat").astype(F64) - L.neuron64(spec, x))
        assert (err <= L.bound(spec, x)).all()


# ---- 2. PReLU on trained-like grids -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", L.LAYER_CASES, ids=L.case_id)
def test_prelu_on_random_grids_is_bit_equal_in_fp32(case):
    C = case[0]
    data, sl = L.random_inputs(case)
    params, perm = L.feeder_params(case)
    specs = [("PReLU", {}), ("PReLU", {"shared": True})]
    params.update(op0=[sl], op1=[np.array(sl[0], F32)])
    x = data[:, perm]
    assert (x != 0).all()
    for in_place in (False, True):
        net = _net(L.ops_net_text(case, specs, in_place), params)
        _forward(net, data)
        _same(_blob(net, L.feeder_txt(C)[1]), x, "the feeder")             # (x * 1 + 0 * ... is x in fp32)
        _same(_blob(net, "n0"), L.neuron32(specs[0], x, sl), (L.case_id(case), "per channel", in_place))
        _same(_blob(net, "n1"), L.neuron32(specs[1], x, sl[0]), (L.case_id(case), "shared", in_place))


# ---- 3. the library ops against binary64 ----------------------------------------------------------------------------------------
_LIB = {}


def _library_run(case):
    """{(mode, spec index): blob} of one net that holds every library op on the case's map, forwarded on the signed grid (the
    first ops) and on its magnitudes (Log, Power); computed once per case."""
    if case not in _LIB:
        C = case[0]
        data = L.library_inputs(case)
        params, perm = L.feeder_params(case)
        net = _net(L.ops_net_text(case, L.LIBRARY_SPECS), params)
        out = {"x": data[:, perm]}
        for mode in ("fp32", "f64"):
            net.set_conv_mode(mode)
            for grid, specs in ((data, L.SIGNED_SPECS), (np.abs(data), L.POSITIVE_SPECS)):
                _forward(net, grid)
                _same(_blob(net, L.feeder_txt(C)[1]), grid[:, perm], (mode, "the feeder"))
                for spec in specs:
                    out[(mode, L.spec_id(spec))] = _blob(net, "n%d" % L.LIBRARY_SPECS.index(spec))
        _LIB[case] = out
    return _LIB[case]


@pytest.mark.parametrize("spec", L.LIBRARY_SPECS, ids=L.spec_id)
@pytest.mark.parametrize("case", L.LAYER_CASES, ids=L.case_id)
def test_library_ops_against_binary64(case, spec):
    run = _library_run(case)
    x = np.abs(run["x"]) if spec in L.POSITIVE_SPECS else run["x"]
    ref, bnd = L.neuron64(spec, x), L.bound(spec, x)
    got = run[("fp32", L.spec_id(spec))]
    assert got.shape == ref.shape and np.isfinite(got).all() and np.isfinite(ref).all()
    err = np.abs(got.astype(F64) - ref)
    worst = int(np.argmax(err / bnd))
    print("ULPS %s %s fp32: max %.3f ulps, max err / bound %.3f (at x = %r)" % (
        L.spec_id(spec), L.case_id(case), float(L.ulps(got, ref).max()), float((err / bnd).max()), float(x.flat[worst])))
    assert (err <= bnd).all(), (float(x.flat[worst]), float(got.flat[worst]), float(ref.flat[worst]), float(err.flat[worst]), float(bnd.flat[worst]))
    off = _within_an_ulp(run[("f64", L.spec_id(spec))], ref, ("f64", L.spec_id(spec), L.case_id(case)))
    print("ULPS %s %s f64: %d of %d not the rounded reference" % (L.spec_id(spec), L.case_id(case), off, ref.size))


# ---- 4. the census's value cases and refusals; fillers, shared blobs, caffemodel blobs --------------------------------------------
@pytest.mark.parametrize("name", sorted(L.VALUE_CASES))
def test_value_case_differs_from_its_twin_and_matches_the_reference(name):
    from smallhardface_amd import caffe
    case = L.VALUE_CASES[name]
    pre = G.feeder_params(L.VC, False)[0]
    outs = []
    for text, spec, slope in ((case.text, case.spec, case.slopes[0]), (case.twin, case.twin_spec, case.slopes[1])):
        net = caffe.Net(None, prototxt_text=text)
        H.load_params(net, dict(pre, n=[slope]) if slope is not None else pre)
        x = L.value_input(case.spec)
        got = _forward(net, x)["n"]
        if spec[0] == "PReLU":
            blob = np.array(net.params["n"][0].data)
            assert blob.shape == (() if spec[1].get("shared") else (L.VC,))
            slope = blob
        if L.is_exact(spec):
            _equal(got, L.neuron32(spec, x, slope), (name, spec))
        else:
            err = np.abs(got.astype(F64) - L.neuron64(spec, x, slope))
            assert np.isfinite(got).all() and (err <= L.bound(spec, x)).all(), (name, spec)
        outs.append(got)
    assert not np.array_equal(outs[0], outs[1]), "the result does not depend on the field"


@pytest.mark.parametrize("name", sorted(L.REFUSALS))
def test_graphs_refused_at_construction_by_layer_name(name):
    from smallhardface_amd import caffe
    r = L.REFUSALS[name]
    with pytest.raises(Exception, match=r.match):
        caffe.Net(None, prototxt_text=L.refusal_net(r.layers))


@pytest.mark.parametrize("name", sorted(L.ACCEPTED))
def test_inert_fields_construct_and_change_nothing(name):
    from smallhardface_amd import caffe
    text = L.ACCEPTED[name]
    t = "Sigmoid" if "Sigmoid" in text else "TanH"
    x = L.value_data()
    pre = G.feeder_params(L.VC, False)[0]
    outs = []
    for txt in (text, L.field_net(L.neuron_layer("n", (t, {}), "pre", "n"))):
        net = caffe.Net(None, prototxt_text=txt)
        H.load_params(net, pre)
        outs.append(_forward(net, x)["n"])
    _same(outs[0], outs[1], name)


def test_a_bottom_of_a_proposal_tail_is_refused():
    from smallhardface_amd import caffe
    txt = H.mini_detector(F.conv_layer("c0", "data", 128, 3, True), "c0", 8, 3, 8, 8) + L.neuron_layer("s_tail", ("Sigmoid", {}), "cls_score_output", "y")
    with pytest.raises(Exception, match=r"Sigmoid 's_tail'.*'cls_score_output'.*proposal tail"):
        caffe.Net(None, prototxt_text=txt)


def test_a_sigmoid_inside_a_tails_score_branch_stays_refused():
    from smallhardface_amd import caffe
    txt = H.mini_detector(F.conv_layer("c0", "data", 128, 3, True), "c0", 8, 3, 8, 8)
    old = 'layer { name: "cls_prob" type: "Softmax" bottom: "cls_score_reshape_output" top: "cls_prob_output" }'
    assert txt.count(old) == 1
    with pytest.raises(Exception, match=r"expected a Softmax"):
        caffe.Net(None, prototxt_text=txt.replace(old, old.replace("Softmax", "Sigmoid")))


def test_the_other_types_stay_refused():
    from smallhardface_amd import caffe
    for t in ("LRN", "Dropout", "Slice", "InnerProduct"):
        with pytest.raises(Exception, match=r"Unsupported layer type '%s' \(layer 'x'\)" % t):
            caffe.Net(None, prototxt_text=L.field_net(L.BARE % ("x", t, 'bottom: "pre" top: "x"')))


def _bottoms():
    return G.conv_txt("pre", "data", 16, 1) + G.conv_txt("b0", "pre", 8, 1) + G.conv_txt("b1", "pre", 8, 1)


def test_fresh_blobs_are_the_fillers_and_commits_are_followed():
    """The filler's value is in Net.params before any load (none: 0.25; constant: its value; another type: 0.25); a shared blob
    has 0 axes; blobs shared by `param { name: }` and by lanes; a commit is followed by the next forward."""
    from smallhardface_amd import caffe
    C, h, w = 8, 3, 5
    pr = lambda name, bottom, kw, pnames=None: L.neuron_layer(name, ("PReLU", kw), bottom, name, pnames=pnames)    # noqa: E731
    txt = H.single_layer_net(_bottoms() + pr("a", "b0", {"fill": -1.5}, ["sl"]) + pr("b", "b1", {}, ["sl"]) + pr("plain", "b0", {}) +
                             pr("sh", "b0", {"shared": True, "fill": 2}) + pr("zero", "b0", {"filler": 'type: "constant"'}) +
                             pr("gauss", "b0", {"filler": 'type: "gaussian" std: 3'}), 16, h, w)
    net = caffe.Net(None, prototxt_text=txt)
    shapes = {k: tuple(net.params[k][0].data.shape) for k in ("a", "b", "plain", "sh", "zero", "gauss")}
    assert shapes == {"a": (C,), "b": (C,), "plain": (C,), "sh": (), "zero": (C,), "gauss": (C,)}, shapes
    first = {k: np.array(net.params[k][0].data).reshape(-1) for k in shapes}
    assert (first["a"] == -1.5).all() and (first["b"] == -1.5).all() and (first["plain"] == 0.25).all() and (first["sh"] == 2).all()
    assert (first["zero"] == 0).all() and (first["gauss"] == 0.25).all()
    assert all(len(net.params[k]) == 1 for k in shapes)
    rng = np.random.default_rng(6)
    data = rng.integers(-4, 5, (1, 16, h, w)).astype(F32)
    s0, p0 = G.selection(C, 16, seed=5)
    s1, p1 = G.selection(C, 16, seed=6)
    H.load_params(net, {"pre": G.feeder_params(16, False)[0]["pre"], "b0": [s0, np.zeros(C, F32)], "b1": [s1, np.zeros(C, F32)]})
    lane = net.clone()
    _forward(lane, data)
    x0, x1 = data[:, p0], data[:, p1]
    per, sh = ("PReLU", {}), ("PReLU", {"shared": True})
    _equal(_blob(lane, "a"), L.neuron32(per, x0, np.full(C, -1.5, F32)), "a")
    _equal(_blob(lane, "b"), L.neuron32(per, x1, np.full(C, -1.5, F32)), "b shares a's blob")
    _equal(_blob(lane, "plain"), L.neuron32(per, x0, np.full(C, 0.25, F32)), "plain")
    _equal(_blob(lane, "sh"), L.neuron32(sh, x0, np.array(2, F32)), "sh")
    _equal(_blob(lane, "zero"), np.maximum(x0, 0), "zero")
    new = rng.integers(-2, 3, C).astype(F32)
    net.params["b"][0].data[...] = new              # the shared blob, through the second layer
    net.params["sh"][0].data[...] = -2
    net.commit_params()
    _forward(lane, data)
    _equal(_blob(lane, "a"), L.neuron32(per, x0, new), "a follows the commit")
    _equal(_blob(lane, "b"), L.neuron32(per, x1, new), "b follows the commit")
    _equal(_blob(lane, "sh"), L.neuron32(sh, x0, np.array(-2, F32)), "sh follows the commit")


def test_caffemodel_blobs(tmp_path):
    from smallhardface_amd import caffe, caffemodel
    case = (12, 3, 5)
    data, sl, shared = L.int_inputs(case)
    feeder, perm = L.feeder_params(case)
    types = {"op0": "PReLU"}
    for sh in (False, True):
        spec = ("PReLU", {"shared": sh})
        txt = L.ops_net_text(case, [spec])
        p = dict(feeder, op0=[shared if sh else sl])
        path = caffemodel.write_caffemodel(str(tmp_path / ("n%d.caffemodel" % sh)), p, layer_types=types)
        assert caffemodel.read_blob(path, "op0", 0).shape == (() if sh else (12,))
        loaded = caffe.Net(None, path, caffe.TEST, prototxt_text=txt)
        assert tuple(loaded.params["op0"][0].data.shape) == (() if sh else (12,)) and len(loaded.params["op0"]) == 1
        _same(np.array(loaded.params["op0"][0].data), p["op0"][0], "the blob")
        _equal(_forward(loaded, data)["n0"], L.neuron32(spec, data[:, perm], p["op0"][0]), "the forward")
    # a (1,) blob for the per-channel layer, a (12,) blob for the shared one, two blobs
    txt = L.ops_net_text(case, [("PReLU", {})])
    caffemodel.write_caffemodel(str(tmp_path / "one.caffemodel"), dict(feeder, op0=[np.ones(1, F32)]), layer_types=types)
    with pytest.raises(Exception, match=r"Cannot copy param 0 weights from layer 'op0'; shape mismatch"):
        caffe.Net(None, str(tmp_path / "one.caffemodel"), caffe.TEST, prototxt_text=txt)
    with pytest.raises(Exception, match=r"Cannot copy param 0 weights from layer 'op0'; shape mismatch"):
        caffe.Net(None, str(tmp_path / "n0.caffemodel"), caffe.TEST, prototxt_text=L.ops_net_text(case, [("PReLU", {"shared": True})]))
    caffemodel.write_caffemodel(str(tmp_path / "two.caffemodel"), dict(feeder, op0=[sl, sl]), layer_types=types)
    with pytest.raises(Exception, match=r"Incompatible number of blobs for layer op0"):
        caffe.Net(None, str(tmp_path / "two.caffemodel"), caffe.TEST, prototxt_text=txt)


# ---- 5. neighbours on the fused path --------------------------------------------------------------------------------------------
NB_HW = (13, 19)


def _graph(text_fn, **kw):
    msg = P.parse(text_fn(*NB_HW, **kw))
    return msg, L.graph_params(msg, seed=5), H.synth_image_blob(*NB_HW, seed=3), np.array([[NB_HW[0], NB_HW[1], 1.0]], F32)


@pytest.mark.parametrize("relu", [True, False], ids=["conv_relu", "conv_bare"])
def test_split_fp16_neighbours_on_the_fused_path(relu):
    """``relu``: the convolution in front carries its in-place ReLU (the PReLU then changes no value: what is held is the plan);
    without it about half of the values take the slope."""
    msg, params, data, info = _graph(L.neighbours_text, relu=relu, fill=0.5)
    onet = L.NeuronOracleNet(msg, params=_copy(params))
    gnet = _net(P.dumps(msg), params)
    assert tuple(gnet.params["pr"][0].data.shape) == (128,) and (np.array(gnet.params["pr"][0].data) == 0.5).all()
    gnet.set_conv_mode("f16x3")
    redos = gnet.range_fallbacks
    _, prof = _profiled(gnet, lambda: H.run_both(gnet, onet, data, info))
    assert gnet.range_fallbacks == redos
    # the fused path ran (the first pair is one kernel); the PReLU is one launch; `c1`, which it rewrites, is plain fp32: both
    # family convolutions that read it run the fp32-input class, none the split-input one
    split_in = sum(prof.get(W4(True, mt, nt), 0) for mt in (2, 4) for nt in (1, 2))
    plain_in = sum(prof.get(W4(False, mt, nt), 0) for mt in (2, 4) for nt in (1, 2))
    assert prof[FUSE1] == 1 and prof[KERNEL] == 1 and (split_in, plain_in) == (0, 2), (prof[FUSE1], prof[KERNEL], split_in, plain_in)
    if not relu:
        assert (onet.blobs["c1"].data < 0).mean() > 0.2           # (the rewritten blob: its negative values took the slope)
    for name in L.NB_BLOBS:
        e = H.rel_err(_blob(gnet, name), onet.blobs[name].data)
        print("neighbours %s: max %.3g, rel err %.3g" % (name, float(np.abs(onet.blobs[name].data).max()), e))
        assert e < ACT_TOL, (name, e)
    # what the FUSED pass itself left in the last maps (the blobs above are re-run layer by layer when read)
    want = [onet.blobs[k].data[0].copy() for k in ("c2", "c2b")]
    fused = H.read_fused_blob(gnet, onet, data, info, mode="f16x3")
    for k, f, wnt in zip(("c2", "c2b"), fused, want):
        e = H.rel_err(f, wnt)
        print("neighbours %s of the fused pass: rel err %.3g" % (k, e))
        assert e < ACT_TOL, (k, e)
    assert gnet.range_fallbacks == redos


@pytest.fixture
def det_cfg():
    old = (cfg.TEST.SCORE_THRESH, cfg.TEST.ANCHOR_MIN_SIZE, cfg.TEST.N_DETS_PER_MODULE)
    cfg.TEST.SCORE_THRESH, cfg.TEST.ANCHOR_MIN_SIZE, cfg.TEST.N_DETS_PER_MODULE = G.S3FD_THRESH, G.S3FD_MIN_SIZE, 10000
    yield
    cfg.TEST.SCORE_THRESH, cfg.TEST.ANCHOR_MIN_SIZE, cfg.TEST.N_DETS_PER_MODULE = old


@pytest.fixture
def mfn_cfg():
    old = (cfg.TEST.SCORE_THRESH, cfg.TEST.ANCHOR_MIN_SIZE, cfg.TEST.N_DETS_PER_MODULE)
    cfg.TEST.SCORE_THRESH, cfg.TEST.ANCHOR_MIN_SIZE, cfg.TEST.N_DETS_PER_MODULE = L.MFN_THRESH, L.MFN_MIN_SIZE, 10000
    yield
    cfg.TEST.SCORE_THRESH, cfg.TEST.ANCHOR_MIN_SIZE, cfg.TEST.N_DETS_PER_MODULE = old


def _match_rows(gb, gs, ob, os_):
    """tests/test_gpu_modules.py: every row has a partner of the same score (within SCORE_TOL); the largest box difference."""
    worst = 0.0
    for (ab, as_), (bb, bs) in (((gb, gs), (ob, os_)), ((ob, os_), (gb, gs))):
        for i in range(len(as_)):
            near = np.where(np.abs(bs[:, 1] - as_[i, 1]) < SCORE_TOL)[0]
            assert len(near) > 0, (i, as_[i])
            worst = max(worst, float(np.abs(bb[near] - ab[i]).max(axis=1).min()))
    return worst


def _check_rows(what, gb, gs, ob, os_):
    assert gb.shape == ob.shape and gs.shape == os_.shape and len(os_) > 1, (what, gb.shape, ob.shape)
    ds = float(np.abs(np.sort(gs[:, 1])[::-1] - np.sort(os_[:, 1])[::-1]).max())
    db = _match_rows(gb, gs, ob, os_)
    print("%s: %d rows, max |dscore| %.3g, max |dbox| %.3g px" % (what, len(gs), ds, db))
    assert ds < SCORE_TOL and db < BOX_TOL, (what, ds, db)


@pytest.mark.parametrize("mode", ["fp32", "f16x3"])
def test_sigmoid_top_as_a_proposal_head_blob(det_cfg, mode):
    from oracle import oracle as O
    msg, params, data, info = _graph(L.head_text)
    onet = L.forwarded(L.NeuronOracleNet(msg, params=_copy(params), proposal_cfg=O.ProposalParams(
        pre_nms_topN=10000, score_thresh=G.S3FD_THRESH, min_size=G.S3FD_MIN_SIZE)), data, info)
    gnet = _net(P.dumps(msg), params)
    gnet.set_conv_mode(mode)
    go, prof = _profiled(gnet, lambda: _forward(gnet, data, info))
    assert prof[KERNEL] == 1 and prof["detect_tail"] >= 1
    _check_rows("head %s" % mode, go["boxes"], go["cls_prob"], onet.blobs["boxes"].data, onet.blobs["cls_prob"].data)
    got = _blob(gnet, "n")
    assert got.min() >= 0 and got.max() <= 1 and H.rel_err(got, onet.blobs["n"].data) < ACT_TOL


def test_a_concat_whose_top_is_rewritten_copies():
    """An in-place PReLU on a Concat's top: the Concat copies (Caffe's bottoms keep their values)."""
    C, h, w = 8, 3, 5
    rng = np.random.default_rng(9)
    data = rng.integers(-4, 5, (1, 16, h, w)).astype(F32)
    s0, p0 = G.selection(C, 16, seed=5)
    s1, p1 = G.selection(C, 16, seed=6)
    sl = rng.integers(-2, 3, 2 * C).astype(F32)
    sl[0] = -2
    txt = H.single_layer_net(_bottoms() + F.concat_layer("cc", ["b0", "b1"]) + L.neuron_layer("pr", ("PReLU", {}), "cc"), 16, h, w)
    net = _net(txt, {"pre": G.feeder_params(16, False)[0]["pre"], "b0": [s0, np.zeros(C, F32)], "b1": [s1, np.zeros(C, F32)], "pr": [sl]})
    _, prof = _profiled(net, lambda: _forward(net, data))
    assert prof[KERNEL] == 1 and prof["eltwise_combine"] == 2          # one copy per member
    cat = np.concatenate([data[:, p0], data[:, p1]], axis=1)
    _equal(_blob(net, "cc"), L.neuron32(("PReLU", {}), cat, sl), "cc")
    _equal(_blob(net, "b0"), data[:, p0], "b0 keeps its values")
    _equal(_blob(net, "b1"), data[:, p1], "b1 keeps its values")


def test_in_place_on_a_member_before_the_concat():
    """The member is rewritten before the Concat's view is read: accepted, and the Concat holds the rewritten values."""
    C, h, w = 8, 3, 5
    rng = np.random.default_rng(4)
    data = rng.integers(-4, 5, (1, 16, h, w)).astype(F32)
    s0, p0 = G.selection(C, 16, seed=5)
    s1, p1 = G.selection(C, 16, seed=6)
    txt = H.single_layer_net(G.conv_txt("pre", "data", 16, 1) + G.conv_txt("s0", "pre", C, 1) + G.conv_txt("s1", "pre", C, 1) +
                             L.neuron_layer("a", ("AbsVal", {}), "s1") + F.concat_layer("cc", ["s0", "s1"]), 16, h, w)
    net = _net(txt, {"pre": G.feeder_params(16, False)[0]["pre"], "s0": [s0, np.zeros(C, F32)], "s1": [s1, np.zeros(C, F32)]})
    (_, prof) = _profiled(net, lambda: _forward(net, data))
    assert prof[KERNEL] == 1
    _equal(_blob(net, "cc"), np.concatenate([data[:, p0], np.abs(data[:, p1])], axis=1), "cc")
    _same(_blob(net, "cc")[:, C:], _blob(net, "s1"), "the member is the view")


# ---- 6. the range guard -----------------------------------------------------------------------------------------------------------
def test_a_scale_beyond_the_fp16_range_redoes_the_forward_in_fp32():
    """`c1` is of order 1, the Power top 1e5 times that.  Its launch raises the range flag, the forward is redone on the fp32
    kernels: outputs and blobs equal fp32 mode's."""
    msg, params, data, info = _graph(L.range_text)
    params["c2"][0] = (params["c2"][0] * F32(2.0 ** -14)).astype(F32)
    onet = L.forwarded(L.NeuronOracleNet(msg, params=_copy(params)), data, info)
    m = {k: float(np.abs(onet.blobs[k].data).max()) for k in L.RANGE_BLOBS}
    print(m)
    assert m["n"] > 65504 * 1.5 and m["c1"] < 1000 and m["c2"] < 1000 and m["c2b"] < 1000
    gnet, fnet = _net(P.dumps(msg), params), _net(P.dumps(msg), params)
    gnet.set_conv_mode("f16x3")
    fnet.set_conv_mode("fp32")
    before = gnet.range_fallbacks
    (go, _), prof = _profiled(gnet, lambda: H.run_both(gnet, onet, data, info))
    fo = _forward(fnet, data, info)
    assert gnet.range_fallbacks == before + 1 and fnet.range_fallbacks == 0
    assert prof[KERNEL] == 2, prof[KERNEL]          # the launch, and once more in the fp32 redo
    for key in fo:
        _same(np.array(go[key]), fo[key], key)
    for name in L.RANGE_BLOBS:
        _same(_blob(gnet, name), _blob(fnet, name), name)
        assert H.rel_err(_blob(gnet, name), onet.blobs[name].data) < ACT_TOL, name


# ---- 7. / 8. the MobileFaceNet-shaped mini detector --------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def mfn():
    """The net, three lanes of it, and the units of the group's sizes."""
    root = _net(L.mfn_text(*L.MFN_SIZE), L.mfn_params())
    lanes = [root.clone() for _ in range(3)]
    units = [L.mfn_unit(h, w) for h, w in L.MFN_GROUP_SIZES]
    return root, lanes, units


def _stage_group(lanes, units):
    ins = []
    for lane, (x, info) in zip(lanes, units):
        lane.blobs["data"].reshape(*x.shape)
        lane.blobs["im_info"].reshape(1, 3)
        ins.append({"data": x, "im_info": info})
    return ins


@pytest.mark.parametrize("mode", ["fp32", "f16x3"])
def test_mini_detector_against_the_oracle(mfn, mfn_cfg, mode):
    root, lanes, units = mfn
    data, info = units[0]
    onet = L.forwarded(L.mfn_oracle(), data, info)
    root.set_conv_mode(mode)
    try:
        redos = root.range_fallbacks
        go, prof = _profiled(root, lambda: _forward(root, data, info))
        assert root.range_fallbacks == redos
        assert prof[KERNEL] == len(L.MFN_PRELUS) == 7, prof[KERNEL]
        assert list(root.blobs.keys()) == list(onet.blobs.keys())
        _check_rows("mini detector %s" % mode, go["boxes"], go["cls_prob"], onet.blobs["boxes"].data, onet.blobs["cls_prob"].data)
        for name in L.MFN_BLOBS:
            e = H.rel_err(_blob(root, name), onet.blobs[name].data)
            print("mini detector %s %s: rel err %.3g" % (mode, name, e))
            assert e < ACT_TOL, (name, e)
        assert (onet.blobs["f4"].data < 0).mean() > 0.2          # (the slopes matter: much of every map is negative)
    finally:
        root.set_conv_mode("fp32")


@pytest.mark.parametrize("mode", ["fp32", "f16x3", "f64"])
def test_forward_group_equals_the_units_one_at_a_time(mfn, mfn_cfg, mode):
    root, lanes, units = mfn
    root.set_conv_mode(mode)
    try:
        single = [_forward(root, x, info) for x, info in units]
        assert all(len(s) == 2 and len(s["cls_prob"]) > 1 for s in single)
        ins = _stage_group(lanes, units)
        redos = root.range_fallbacks
        root.prof_enable(True)
        root.prof_reset()
        outs = root.forward_group(lanes, ins)
        rec = root.prof_read()[KERNEL]
        root.prof_enable(False)
        assert root.range_fallbacks == redos
        # one launch per layer and pass, whatever the number of lanes
        assert int(rec["launches"]) == len(L.MFN_PRELUS), rec
        assert rec["flops"] > 0 and rec["bytes"] > 0
        for k, (lane, out) in enumerate(zip(lanes, outs)):
            assert sorted(out.keys()) == sorted(single[k].keys())
            for key in out:
                _same(np.array(out[key]), single[k][key], "unit %d %s" % (k, key))
    finally:
        root.prof_enable(False)
        root.set_conv_mode("fp32")


@pytest.mark.parametrize("mode", ["fp32", "f16x3"])
def test_results_ignore_buffer_history(mfn, mfn_cfg, mode):
    """A, then B (a smaller map: the buffers keep A's values beyond it), then A again."""
    root, lanes, units = mfn
    root.set_conv_mode(mode)
    try:
        (xa, ia), (xb, ib) = units[0], units[2]
        first = _forward(root, xa, ia)
        blobs = {k: _blob(root, k) for k in L.MFN_BLOBS}
        _forward(root, xb, ib)
        again = _forward(root, xa, ia)
        for key in first:
            _same(again[key], first[key], key)
        for k in L.MFN_BLOBS:
            _same(_blob(root, k), blobs[k], k)
    finally:
        root.set_conv_mode("fp32")


def test_profiler_books_none_for_a_graph_without_the_layers():
    net = _net(G.s3fd_text(*G.S3FD_SIZE), G.s3fd_params())
    data, info = G.s3fd_unit(*G.S3FD_SIZE)
    _forward(net, data, info)
    _, prof = _profiled(net, lambda: _forward(net, data, info))
    assert KERNEL in prof and prof[KERNEL] == 0

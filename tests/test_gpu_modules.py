"""Nets with several ProposalLayers ("modules": one per backbone stride of an SSH-style detector, tops ``boxes_<level>`` /
``cls_prob_<level>`` as lib/test.py:67-83 collects them) through caffe.Net, Net.forward, Net.forward_group, Blob.data and
detect()'s host merge (run on an MI355X: ``pytest -m gpu``).  Graphs and parameters: tests/modules_cases.py.

A pass issues the tails of all its (unit, module) pairs as ONE launch sequence of the grouped tail kernels (csrc/tail.hip),
the geometry looked up per entry from a table of module records; per module the arithmetic is what a single-module net runs.

1. Each module against the oracle's ProposalLayer on the probabilities and deltas the device itself produced: scores bit
   for bit, boxes within BOX_TOL, equal row counts -- with the three modules ending differently in one pass (cut by
   pre_nms_topN, many rows, the single best anchor), and with one module left without a valid anchor (dummy roi, no rows).
2. End to end against OracleNet on both graphs: output names, row counts, scores within SCORE_TOL, boxes within BOX_TOL,
   under seeds for which (asserted on the oracle) no score lies within 2 SCORE_TOL of the threshold, no side within 0.01 px
   of the min-size cut and no two rows of a module tie.
3. Module 2 in the three-module net equals the same branch alone in a single-module net, bit for bit.
4. Every blob reads after a fused forward, the tail-fused ones of every module against the oracle's; the activation-exponent
   slots are left zeroed across the module boundary (tests/test_gpu_parity.py:376-386 for one module).
5. forward_group: 15 entries (one sequence) and 18 (two), both member orders, each member equal to its own forward(); one
   forward() of the three-module net books as many tail launches with the profiler as the single-module net.
6. Refusals at construction and at the entry points built on one device list per net; num_modules.
7. The driver: detect() on the three-module net against the same loop over the oracle net, with a TEST.LEVEL subset, and
   with SHF_GROUPED_FORWARD=1 bit-equal to the ungrouped run.
"""
import numpy as np
import pytest

from oracle import oracle as O
from smallhardface_amd import prototxt as P
from smallhardface_amd.config import cfg
from tests import helpers as H
from tests import modules_cases as M

pytestmark = pytest.mark.gpu

SCORE_TOL = 1e-4        # tests/test_gpu_parity.py
BOX_TOL = 1e-3          # px: device expf vs numpy's float32 exp differ in the last ulp; everything else is op for op (tests/test_gpu_tail_geometry.py)
MODES = ["fp32", "f16x3"]
SIZES = [(13, 19), (16, 16)]      # 13 x 19: 7 x 10 and 4 x 5 maps under Caffe's ceil pooling
TOPN, THRESH = 100, 0.05
ENDING_BIAS = (0.0, 2.0, 12.0)    # class-score biases under which, at TOPN / THRESH, module 1 is cut, 2 is not, 3 has nothing above


def _info(h, w, scale=1.0):
    return np.array([[8 * h - 3, 8 * w - 5, scale]], np.float32)     # one to seven pixels smaller than the padded size


def _data(h, w, seed=3, c=128, std=64):
    return np.random.default_rng(seed).normal(0, std, (1, c, h, w)).astype(np.float32)   # (synth_params scales c0 by 1/64)


def _forward(net, data, info):
    net.blobs["data"].reshape(*data.shape)
    net.blobs["im_info"].reshape(1, 3)
    return {k: np.array(v) for k, v in net.forward(data=data, im_info=info).items()}


def _blob(net, name):
    return np.array(net.blobs[name].data)


def _mini(h, w, params, modules=("1", "2", "3"), cin=128):
    from smallhardface_amd import caffe
    net = caffe.Net(None, prototxt_text=M.mini_text(h, w, modules, cin))
    H.load_params(net, {k: v for k, v in params.items() if k in net.params})
    return net


@pytest.fixture(scope="module")
def mini():
    """The three-module mini net (forwards reshape it) and six lanes of it."""
    root = _mini(16, 16, M.mini_params(7, ENDING_BIAS))
    return [root] + [root.clone() for _ in range(6)]


# ---- 1. each module against the oracle on identical inputs ------------------------------------------------------------------
def _ending_params(config):
    params = M.mini_params(7, ENDING_BIAS)
    if config == "none_valid":      # module 3: dw = dh = -10 on every anchor, boxes of about one pixel under a 2 px minimum
        for i in range(2):
            params["bbox_pred_m3_%d" % i][0][2:] = 0
            params["bbox_pred_m3_%d" % i][1][2:] = -10.0
    return params


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("config", ["three_endings", "none_valid"])
def test_each_module_against_the_oracle_on_identical_inputs(mini, config, size, mode):
    net = mini[0]
    h, w = size
    min_size = 2.0 if config == "none_valid" else 0.0
    cfg.TEST.N_DETS_PER_MODULE, cfg.TEST.SCORE_THRESH, cfg.TEST.ANCHOR_MIN_SIZE = TOPN, THRESH, min_size
    H.load_params(net, _ending_params(config))
    data, info = _data(h, w), _info(h, w)
    net.set_conv_mode(mode)
    try:
        out = _forward(net, data, info)
        rows = {}
        for m, (feats, A, pstr) in M.MINI_MODULES.items():
            gp, gd = _blob(net, "cls_prob_reshape_output_" + m), _blob(net, "bbox_pred_output_" + m)
            mh, mw = M.mini_map_sizes(h, w)[m]
            assert gp.shape == (1, 2 * A, mh, mw) and gd.shape == (1, 4 * A, mh, mw), m
            if min_size:     # the kept set does not hinge on exp()'s last ulp
                b, _ = O.proposal_forward(gp, gd, info, M.module_params(pstr, min_size=0, score_thresh=-1.0, pre_nms_topN=0))
                sides = np.concatenate([b[:, 3] - b[:, 1] + 1, b[:, 4] - b[:, 2] + 1])
                assert np.abs(sides - min_size * info[0, 2]).min() > 0.01
            pb, ps = O.proposal_forward(gp, gd, info, M.module_params(pstr, pre_nms_topN=TOPN, score_thresh=THRESH, min_size=min_size))
            gb, gs = out["boxes_" + m], out["cls_prob_" + m]
            print("%s %s %dx%d module %s: %d rows of %d anchors" % (config, mode, h, w, m, len(ps), mh * mw * A))
            assert gb.shape == pb.shape and gs.shape == ps.shape, m
            np.testing.assert_array_equal(gs, ps, err_msg=m)
            assert np.abs(gb - pb).max() < BOX_TOL, m
            rows[m] = gs
        # the endings, which the parameters were chosen for
        assert len(rows["1"]) == TOPN                                                   # cut by pre_nms_topN
        assert 1 < len(rows["2"]) < TOPN and rows["2"][-1, 1] >= THRESH                   # every candidate above the threshold
        if config == "three_endings":
            assert rows["3"].shape == (1, 2) and rows["3"][0, 1] < THRESH               # none above: the single best anchor
        else:
            assert rows["3"].shape == (0, 2)                                            # none valid: no rows and the dummy roi
            np.testing.assert_array_equal(out["boxes_3"], [[0, 0, 0, 16, 16]])
    finally:
        net.set_conv_mode("fp32")
        H.load_params(net, M.mini_params(7, ENDING_BIAS))


# ---- 2. end to end against OracleNet -------------------------------------------------------------------------------------
E2E_MIN_SIZE = 3.0


def _e2e_case(graph):
    """(graph, parameters, modules, data, im_info, score threshold).  The mini graph's 741 + 140 + 40 anchors straddle any
    threshold: at the driver's 0.002, where a score moves by 0.002 per unit of logit, dozens lie within 2 SCORE_TOL of it under
    every seed, so the case runs at 0.3 (a handful of candidates per 1e-3) under seeds for which none does."""
    if graph == "mini":
        h, w = 13, 19
        msg = P.parse(M.three_module_mini(h, w))
        params = M.mini_params(11, (1.0, 1.0, 1.0))
        return msg, params, M.MINI_MODULES, _data(h, w, seed=7, std=16), _info(h, w, 0.75), 0.3
    msg = M.ssh_shaped(64, 96)
    params = O.synth_params(msg, seed=21, cls_bias=1.0)
    return msg, params, M.SSH_MODULES, H.synth_image_blob(64, 96, seed=4), np.array([[61, 93, 0.75]], np.float32), 0.002


def _match_rows(gb, gs, ob, os_):
    """Every device row has an oracle row with the same score (within SCORE_TOL) and box (returns the largest box
    difference over the best partners), and the other way round."""
    worst = 0.0
    for (ab, as_), (bb, bs) in (((gb, gs), (ob, os_)), ((ob, os_), (gb, gs))):
        for i in range(len(as_)):
            near = np.where(np.abs(bs[:, 1] - as_[i, 1]) < SCORE_TOL)[0]
            assert len(near) > 0, (i, as_[i])
            worst = max(worst, float(np.abs(bb[near] - ab[i]).max(axis=1).min()))
    return worst


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("graph", ["mini", "ssh"])
def test_end_to_end_against_the_oracle_net(graph, mode):
    from smallhardface_amd import caffe
    msg, params, modules, data, info, thresh = _e2e_case(graph)
    cfg.TEST.ANCHOR_MIN_SIZE, cfg.TEST.SCORE_THRESH = E2E_MIN_SIZE, thresh
    onet = O.OracleNet(msg, params=params, proposal_cfg=O.ProposalParams(
        pre_nms_topN=int(cfg.TEST.N_DETS_PER_MODULE), score_thresh=thresh, min_size=E2E_MIN_SIZE))
    gnet = caffe.Net(None, prototxt_text=P.dumps(msg))
    H.load_params(gnet, params)
    gnet.set_conv_mode(mode)
    go, oo = H.run_both(gnet, onet, data, info)
    # the seeds: on the oracle alone, the row sets do not hinge on the last digits
    for m, (d_score, d_side, ties) in M.oracle_margins(onet, info, modules, E2E_MIN_SIZE, thresh).items():
        assert d_score > 2 * SCORE_TOL and d_side > 0.01 and not ties, (m, d_score, d_side, ties)
    assert sorted(go.keys()) == sorted(onet.outputs) == sorted("%s_%s" % (k, m) for m in modules for k in ("boxes", "cls_prob"))
    assert list(gnet.blobs.keys()) == list(onet.blobs.keys())                 # prototxt order: the driver's level order
    assert M.levels_of(gnet) == ["1", "2", "3"]
    for m in modules:
        gb, gs, ob, os_ = go["boxes_" + m], go["cls_prob_" + m], oo["boxes_" + m], oo["cls_prob_" + m]
        assert gb.shape == ob.shape and gs.shape == os_.shape and len(os_) > 1, (m, gb.shape, ob.shape)
        ds = float(np.abs(np.sort(gs[:, 1])[::-1] - np.sort(os_[:, 1])[::-1]).max())
        db = _match_rows(gb, gs, ob, os_)
        print("%s %s module %s: %d rows, max |dscore| %.3g, max |dbox| %.3g px" % (graph, mode, m, len(gs), ds, db))
        assert ds < SCORE_TOL, (m, ds)
        assert db < BOX_TOL, (m, db)


# ---- 3. a module alone equals the module in company --------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
def test_a_module_alone_equals_the_module_in_company(mini, size, mode):
    h, w = size
    params = M.mini_params(7, ENDING_BIAS)
    alone = _mini(h, w, params, modules=("2",))
    assert alone.num_modules == 1 and mini[0].num_modules == 3
    data, info = _data(h, w, seed=9), _info(h, w)
    for net in (mini[0], alone):
        net.set_conv_mode(mode)
    try:
        both, one = _forward(mini[0], data, info), _forward(alone, data, info)
        assert sorted(one.keys()) == ["boxes_2", "cls_prob_2"] and len(one["cls_prob_2"]) > 1
        for key in one:
            np.testing.assert_array_equal(both[key], one[key], err_msg=key)
        for name in ("cls_prob_reshape_output_2", "bbox_pred_output_2", "cls_score_output_2", "c1"):
            np.testing.assert_array_equal(_blob(mini[0], name), _blob(alone, name), err_msg=name)
    finally:
        mini[0].set_conv_mode("fp32")


# ---- 4. every blob is readable after a fused forward ----------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_every_blob_reads_after_forward_and_the_slots_are_left_zeroed(mini, mode):
    net = mini[0]
    h, w = 13, 19
    params = M.mini_params(7, ENDING_BIAS)
    onet = O.OracleNet(P.parse(M.three_module_mini(h, w)), params=params)
    data, info = _data(h, w, seed=13), _info(h, w)
    net.set_conv_mode(mode)
    try:
        H.run_both(net, onet, data, info)
        fused = [n for n in net.blobs.keys() if n.startswith(("cls_score", "cls_prob_output", "bbox_pred_0", "bbox_pred_1"))]
        assert len(fused) == 3 + 3 + 6, fused      # two single-blob tails (3 names each), the per-blob one (2 x 2 + 2)
        for name in net.blobs.keys():
            a, b = _blob(net, name), onet.blobs[name].data
            if name in onet.outputs:      # (the proposal rows against the oracle net's: item 2)
                continue
            assert tuple(a.shape) == tuple(b.shape), (name, a.shape, b.shape)
            if name in fused:
                print("%s %s: max |d| %.3g of max %.3g" % (mode, name, float(np.abs(a - b).max()), float(np.abs(b).max())))
                assert np.abs(a - b).max() < SCORE_TOL, (name, float(np.abs(a - b).max()))
        for m in M.MINI_MODULES:
            np.testing.assert_array_equal(_blob(net, "cls_prob_output_" + m).reshape(-1), _blob(net, "cls_prob_reshape_output_" + m).reshape(-1))
        if mode == "f16x3":
            # a forward of 2^6 x larger activations (inside the fp16 range: no fp32 redo), a read of an intermediate between two
            # modules (a pass without the tails, which must leave the slots zeroed itself), then a forward that equals a fresh
            # lane's: no exponent of the earlier pass survives in a slot that a later module's convolutions read
            redos = net.range_fallbacks
            _forward(net, data * 64.0, info)
            assert net.range_fallbacks == redos
            net.blobs["c1"].data
            third = _forward(net, data, info)
            fresh = _forward(net.clone(), data, info)
            assert sorted(third.keys()) == sorted(fresh.keys()) and len(third) == 6
            for key in third:
                np.testing.assert_array_equal(third[key], fresh[key], err_msg=key)
    finally:
        net.set_conv_mode("fp32")


# ---- 5. forward_group ----------------------------------------------------------------------------------------------------
GROUP_SIZES = [(13, 19), (16, 16), (9, 12), (20, 11), (8, 8), (17, 23)]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("n", [5, 6], ids=["15_entries_one_sequence", "18_entries_two_sequences"])
def test_forward_group_members_equal_their_own_forward(mini, n, mode):
    root, lanes = mini[0], mini[1:]
    cfg.TEST.N_DETS_PER_MODULE, cfg.TEST.SCORE_THRESH = TOPN, THRESH
    units = [(_data(h, w, seed=30 + i), _info(h, w)) for i, (h, w) in enumerate(GROUP_SIZES[:n])]
    root.set_conv_mode(mode)
    try:
        single = [_forward(root, x, info) for x, info in units]
        assert any(len(s["cls_prob_1"]) == TOPN for s in single) and all(len(s) == 6 for s in single)
        for order in (list(range(n)), list(range(n))[::-1]):
            members = lanes[:n]
            ins = []
            for mnet, k in zip(members, order):
                x, info = units[k]
                mnet.blobs["data"].reshape(*x.shape)
                mnet.blobs["im_info"].reshape(1, 3)
                ins.append({"data": x, "im_info": info})
            outs = root.forward_group(members, ins)
            for mnet, k, out in zip(members, order, outs):
                assert sorted(out.keys()) == sorted(single[k].keys())
                for key in out:
                    assert out[key].shape == single[k][key].shape, (order, k, key)
                    np.testing.assert_array_equal(out[key], single[k][key], err_msg="unit %d %s" % (k, key))
                    np.testing.assert_array_equal(mnet.blobs[key].data, single[k][key])
    finally:
        root.set_conv_mode("fp32")


@pytest.mark.parametrize("mode", MODES)
def test_one_forward_books_the_tail_launches_of_a_single_module_net(mini, mode):
    h, w = 13, 19
    alone = _mini(h, w, M.mini_params(7, ENDING_BIAS), modules=("2",))
    data, info = _data(h, w), _info(h, w)
    counts = []
    for net in (mini[0], alone):
        net.set_conv_mode(mode)
        try:
            _forward(net, data, info)
            net.prof_enable(True)
            net.prof_reset()
            _forward(net, data, info)
            counts.append(int(net.prof_read()["detect_tail"]["launches"]))
        finally:
            net.prof_enable(False)
            net.set_conv_mode("fp32")
    assert counts[0] == counts[1] > 0, counts


# ---- 6. refusals, num_modules -------------------------------------------------------------------------------------------
def _trunk_and(tails, h=8, w=8):
    return H.single_layer_net(M._conv1("c0", "data", 128) + M._pool("p1", "c0") + M._conv1("c1", "p1", 256) + tails, 128, h, w)


def test_graphs_refused_at_construction():
    from smallhardface_amd import caffe
    one = M.MINI_MODULES["1"]
    with pytest.raises(RuntimeError, match=r"5 ProposalLayers \('proposal_m1', .*'proposal_m5'\): a net holds at most 4"):
        caffe.Net(None, prototxt_text=_trunk_and("".join(M.module_tail(str(m), *one) for m in range(1, 6))))
    with pytest.raises(RuntimeError, match=r"ProposalLayers 'proposal_m1' and 'proposal_m2' disagree on the class count \(2 vs 3\)"):
        caffe.Net(None, prototxt_text=_trunk_and(M.module_tail("1", *one) + M.module_tail("2", *M.MINI_MODULES["2"], C=3)))
    shared = ('layer { name: "proposal_x" type: "Python" bottom: "cls_prob_reshape_output_1" bottom: "bbox_pred_output_1" '
              'bottom: "im_info" top: "boxes_x" top: "cls_prob_x" python_param { module: "lib.layers.proposal_layer" '
              'layer: "ProposalLayer" param_str: "%s" } }\n' % one[2])
    with pytest.raises(RuntimeError, match=r"ProposalLayers 'proposal_m1' and 'proposal_x' both fuse layer '"):
        caffe.Net(None, prototxt_text=_trunk_and(M.module_tail("1", *one) + shared))
    with pytest.raises(RuntimeError, match=r"ProposalLayers 'proposal_m1' and 'proposal_m2' write the same top 'boxes_1'"):
        caffe.Net(None, prototxt_text=_trunk_and(M.module_tail("1", *one) +
                                                 M.module_tail("2", *M.MINI_MODULES["2"], tops=("boxes_1", "cls_prob_2"))))
    # a refusal of the per-module walk names its module's layer
    bad = M.module_tail("2", ["c1"], 2, "{'feat_stride': [16],'scales': [2], 'ratios':[0.5,2]}")      # subsampled: two strides needed
    with pytest.raises(RuntimeError, match=r"ProposalLayer 'proposal_m2': feat_stride has 1 entries.*indexes 2"):
        caffe.Net(None, prototxt_text=_trunk_and(M.module_tail("1", *one) + bad))
    # four modules are accepted, and the process lives on
    net = caffe.Net(None, prototxt_text=_trunk_and("".join(M.module_tail(str(m), *one) for m in range(1, 5))))
    assert net.num_modules == 4


def test_one_list_entry_points_refuse_a_two_module_net():
    from smallhardface_amd import caffe
    net = caffe.Net(None, prototxt_text=M.mini_text(8, 8, ("1", "2")))
    assert net.num_modules == 2
    x = np.zeros((1, 128, 8, 8), np.float32)
    unit = (x, 8, 8, 61, 59, 1.0, False)
    calls = {
        "detect_begin": lambda: net.detect_begin(),
        "detect_add_level": lambda: net.detect_add_level(x, 8, 8, 61, 59, 1.0, False, 0.05),
        "detect_add_levels": lambda: net.detect_add_levels([net], [unit], 0.05),
        "class_lists_begin": lambda: net.class_lists_begin(),
        "class_lists_add": lambda: net.class_lists_add([net], [59], [1.0], [False], 0.05),
        "debug_proposal": lambda: net.debug_proposal(np.zeros((1, 6, 8, 8), np.float32), np.zeros((1, 12, 8, 8), np.float32),
                                                     np.array([[61, 59, 1]], np.float32)),
        "debug_append": lambda: net.debug_append(np.zeros((1, 5), np.float32), np.zeros((1, 2), np.float32), 59, 1.0, False, 0.05),
    }
    for name, call in calls.items():
        with pytest.raises(RuntimeError, match=r"%s: the net has 2 proposal modules" % name):
            call()
    # nothing was staged or launched: the net forwards as before
    out = _forward(net, _data(8, 8), _info(8, 8))
    assert sorted(out.keys()) == ["boxes_1", "boxes_2", "cls_prob_1", "cls_prob_2"]


def test_num_modules(mini):
    from smallhardface_amd import caffe
    assert mini[0].num_modules == 3 and mini[1].num_modules == 3 and mini[0].clone().num_modules == 3
    tmpl = caffe.Net(None, prototxt_text=P.dumps(H.detector_msg(True)))
    assert tmpl.num_modules == 1 and tmpl.clone().num_modules == 1
    plain = caffe.Net(None, prototxt_text=H.single_layer_net(M._conv1("c0", "data", 128), 128))
    assert plain.num_modules == 0 and plain.clone().num_modules == 0 and plain.num_classes == 0


# ---- 7. the driver ---------------------------------------------------------------------------------------------------------
def _driver_cfg(level=()):
    # levels at scale 1.5 and 2 of the 40 x 56 image, each also flipped: 4 units.  (Not scale 1: the random boxes of this graph
    # are mostly clipped to the level's border, which unscaled by 1 is an integer -- a vote over rows clipped there averages
    # to that integer give or take a rounding, and compare_detection_lists compares the TRUNCATED coordinates.  55 / 1.5 and
    # 111 / 2 are no integers.)
    cfg.TEST.SCALES = [60, 80]
    cfg.TEST.PYRAMID_BASE_SIZE = [800, 1200]
    cfg.TEST.FLIP = True
    cfg.TEST.LEVEL = list(level)
    cfg.TEST.N_DETS_PER_MODULE, cfg.TEST.SCORE_THRESH, cfg.TEST.ANCHOR_MIN_SIZE = 300, 0.002, 0


def _driver_params():
    """The mini graph on a 3-channel image.  An image level is +-128 where `_data` is N(0, 64) and the 1x1 trunk has no
    ReLU, so the class predictors' weights are scaled down: the scores spread over (0, 1) instead of saturating at 1.0, where
    thousands of them tie and the order of the merge is anyone's."""
    params = M.mini_params(5, (1.0, 1.0, 1.0), cin=3)
    for name, blobs in params.items():
        if name.startswith("cls_score_m"):
            blobs[0] *= np.float32(0.1)
    return params


@pytest.mark.parametrize("level", [(), ("2",)], ids=["all_levels", "level_2"])
def test_detect_over_the_levels_equals_the_oracle_loop(level, monkeypatch):
    import smallhardface_amd.test as T
    from tests.test_gpu_fullsize import compare_detection_lists
    params = _driver_params()
    gnet = _mini(48, 64, params, cin=3)
    _driver_cfg(level)                                         # (the autouse fixture of conftest.py restores cfg afterwards)
    onet = O.OracleNet(P.parse(M.mini_text(48, 64, cin=3)), params=params, proposal_cfg=O.ProposalParams(
        pre_nms_topN=int(cfg.TEST.N_DETS_PER_MODULE), score_thresh=float(cfg.TEST.SCORE_THRESH), min_size=0))
    im = np.random.default_rng(77).integers(0, 256, (40, 56, 3)).astype(np.uint8)
    monkeypatch.delenv("SHF_GROUPED_FORWARD", raising=False)
    monkeypatch.delenv("SHF_DEVICE_MERGE", raising=False)
    with monkeypatch.context() as mp:
        mp.setattr(T, "bbox_vote", lambda d, thresh=None: np.asarray(O.bbox_vote(d, cfg.TEST.NMS_THRESH), dtype=np.float64))
        want, _ = T.detect(onet, None, thresh=0.05, pyramid=True, im=im)
    assert len(want) == 1 and len(want[0]) > 8
    for mode in MODES:
        gnet.set_conv_mode(mode)
        got, _ = T.detect(gnet, None, thresh=0.05, pyramid=True, im=im)
        assert len(got) == 1
        compare_detection_lists("modules_driver_%s_%s" % ("_".join(level) or "all", mode), got[0], want[0])
        monkeypatch.setenv("SHF_GROUPED_FORWARD", "1")
        grouped, _ = T.detect(gnet, None, thresh=0.05, pyramid=True, im=im)
        monkeypatch.delenv("SHF_GROUPED_FORWARD")
        np.testing.assert_array_equal(grouped[0], got[0])

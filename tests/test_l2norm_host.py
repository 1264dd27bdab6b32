"""The references, texts and feeders of tests/l2norm_cases.py on the CPU: what tests/test_gpu_l2norm.py holds the Normalize
layer (csrc/l2norm.hip) to must itself be right.

1. ``normalize32`` (the kernel's fixed fp32 order) and ``normalize`` (binary64) agree within the derived bound on random grids.
   On integer grids what is exact agrees bit for bit: the sum of squares, in the vector and in the scalar order.  The outputs
   there are NOT bit-equal -- behind the exact sum the fp32 chain still rounds four times (+ eps, sqrt, /, *) where binary64
   rounds once, measured up to 2 fp32 ulps apart on (64, 33, 67) -- so they are held to the same bound; an all-zero pixel
   gives zeros in both.
2. The order is the one the kernel's header states: lanes, items per lane and the re-reading threshold per case.
3. The net texts parse, and ``filler_params`` / ``norm_spec`` read the fillers as Caffe creates the blob.
4. ``caffemodel`` round-trips a (C,) and a shared (0-axis) blob.
5. The feeders hand an integer grid on unchanged (the oracle net), ``L2NormOracleNet`` runs the layer in and out of place.
"""
import numpy as np
import pytest

from smallhardface_amd import prototxt as P
from tests import depthwise_cases as D
from tests import general_conv_cases as G
from tests import l2norm_cases as L

F32 = np.float32
F64 = np.float64


@pytest.mark.parametrize("shared", [False, True], ids=["per_channel", "shared"])
@pytest.mark.parametrize("case", L.LAYER_CASES, ids=L.case_id)
def test_fp32_order_within_the_bound_of_binary64_on_random_grids(case, shared):
    C, h, w = case
    data, sc = L.random_inputs(case, shared)
    x = data[:, D.feeder_params(C)[1]]
    assert x.shape == (1, C, h, w)
    for eps in (L.EPS, 0.001):
        ref = L.normalize(x, sc, eps, shared)
        got = L.normalize32(x, sc, eps, shared).astype(F64)
        err, bnd = np.abs(got - ref), L.bound(ref, C)
        worst = int(np.argmax(err - bnd))
        print("%s eps %g: max err / bound %.3g" % (L.case_id(case), eps, float((err / bnd).max())))
        assert (err <= bnd).all(), (eps, float(err.flat[worst]), float(bnd.flat[worst]))
        assert np.abs(ref).max() > 0.1                      # (scales around 10 on a unit vector: no degenerate grid)


@pytest.mark.parametrize("shared", [False, True], ids=["per_channel", "shared"])
@pytest.mark.parametrize("case", L.LAYER_CASES, ids=L.case_id)
def test_references_agree_on_integer_grids(case, shared):
    C, h, w = case
    data, sc = L.int_inputs(case, shared)
    x = data[:, D.feeder_params(C)[1]]
    assert (h * w == 1 or (x[:, :, 0, 0] == 0).all()) and (shared or C == 1 or (np.asarray(sc) == 0).sum() == 1)
    # the sum of squares is exact in either vector / scalar order, so the two forms give the same bits
    S = (x.astype(F64) ** 2).sum(axis=1, keepdims=True)
    for vec in ([True, False] if C % 4 == 0 else [False]):
        assert (L.sum_squares32(x, vec).astype(F64) == S).all()
    for eps in (L.EPS, 0.001):
        y32, y64 = L.normalize32(x, sc, eps, shared), L.normalize(x, sc, eps, shared)
        assert (np.abs(y32.astype(F64) - y64) <= L.bound(y64, C)).all()
        assert (h * w == 1 or (y32[:, :, 0, 0] == 0).all()) and np.isfinite(y32).all()          # 0 / sqrt(eps), never NaN
        assert np.abs(y32).max() > 0.01


def test_the_order_per_case_is_the_headers():
    want = {512: (True, 32, 4), 256: (True, 16, 4), 4: (True, 1, 1), 1: (False, 1, 1), 5: (False, 8, 1), 6: (False, 8, 1),
            260: (True, 32, 4), 1028: (True, 64, 8), 64: (True, 8, 2), 4100: (True, 64, 0), 1030: (False, 64, 0)}
    assert sorted(want) == sorted(c[0] for c in L.LAYER_CASES)
    for C, f in want.items():
        assert L.form(C) == f, (C, L.form(C))
    assert L.form(4096) == (True, 64, 16) and L.form(1024, False) == (False, 64, 16) and L.form(1025) == (False, 64, 0)
    assert L.form(12, False) == (False, 8, 2)               # an unaligned view of a C % 4 == 0 layer: the scalar form
    # one lane per pixel adds in channel order; two lanes split the quads between them
    x = np.arange(1, 9, dtype=F32).reshape(1, 8, 1, 1)
    assert L.form(8) == (True, 2, 1) and float(L.sum_squares32(x)[0, 0, 0, 0]) == 204.0


def test_net_texts_parse_and_fillers_are_caffes():
    for case in L.LAYER_CASES:
        for shared in (False, True):
            msg = P.parse(L.layer_net_text(case, shared, eps=0.001, fill=3.0))
            n = [l for l in msg.getall("layer") if str(l.get("type")) == "Normalize"]
            assert len(n) == 1 and L.norm_spec(n[0]) == (shared, 0.001, 3.0)
            assert L.filler_params(msg)["n"][0].shape == (() if shared else (case[0],))
    msg = P.parse(L.concat_net_text(12))
    assert [str(l.get("name")) for l in msg.getall("layer") if str(l.get("type")) == "Normalize"] == ["n0", "n1"]
    for text in (L.neighbours_text(13, 19), L.head_text(13, 19), L.s3fd_norm_text(*G.S3FD_SIZE)):
        assert P.parse(P.dumps(P.parse(text))).getall("layer")
    # no filler: 1; a constant filler without a value: 0 (FillerParameter's default); any other type: left at 1
    specs = [(L.norm_layer("a", "x", "a"), 1.0), (L.norm_layer("a", "x", "a", filler='type: "constant"'), 0.0),
             (L.norm_layer("a", "x", "a", filler='type: "gaussian" std: 2'), 1.0), (L.norm_layer("a", "x", "a", fill=20), 20.0)]
    for txt, fill in specs:
        layer = P.parse(txt).getall("layer")[0]
        assert L.norm_spec(layer) == (False, L.EPS, fill), txt
    absent = P.parse(L.norm_layer("a", "x", "a", across=None)).getall("layer")[0]
    assert absent.get("norm_param").get("across_spatial", None) is None
    params = L.s3fd_norm_params()
    assert params["f8_norm"][0].shape == (128,) and (params["f8_norm"][0] == 10).all() and (params["f16_norm"][0] == 8).all()


def test_caffemodel_round_trips_a_vector_and_a_shared_blob(tmp_path):
    from smallhardface_amd import caffemodel
    vec = np.random.default_rng(2).normal(10, 3, 12).astype(F32)
    one = np.array(20.0, F32)
    assert one.shape == ()
    path = caffemodel.write_caffemodel(str(tmp_path / "n.caffemodel"), {"n0": [vec], "n1": [one]},
                                       layer_types={"n0": "Normalize", "n1": "Normalize"})
    back0, back1 = caffemodel.read_blob(path, "n0", 0), caffemodel.read_blob(path, "n1", 0)
    assert back0.shape == (12,) and back1.shape == () and back1.size == 1
    np.testing.assert_array_equal(back0.view(np.uint32), vec.view(np.uint32))
    assert float(back1) == 20.0


@pytest.mark.parametrize("case", [c for c in L.LAYER_CASES if c[1] * c[2] <= 64], ids=L.case_id)
def test_feeders_are_exact_and_the_oracle_net_runs_the_layer(case):
    C, h, w = case
    data, sc = L.int_inputs(case)
    params, perm = L.n_params(case, sc)
    info = np.array([[h, w, 1]], F32)
    x = data[:, perm]
    want = L.normalize32(x, sc)
    feeder = D.feeder_txt(C)[1]
    for in_place in (False, True):
        onet = L.forwarded(L.L2NormOracleNet(P.parse(L.layer_net_text(case, in_place=in_place)), params=params), data, info)
        out = L.out_blob(case, in_place)
        assert onet.blobs[out].data.shape == (1, C, h, w)
        np.testing.assert_array_equal(onet.blobs[out].data.view(np.uint32), want.view(np.uint32))
        np.testing.assert_array_equal(onet.snapshots[({"pre": "pre", "sel": "sel"}[feeder], feeder)], x)
        if not in_place:
            np.testing.assert_array_equal(onet.blobs[feeder].data, x)


def test_oracle_net_concat_members():
    C = 6
    rng = np.random.default_rng(3)
    data = rng.integers(-4, 5, (1, 16, 7, 9)).astype(F32)
    s0, p0 = G.selection(C, 16, seed=5)
    s1, p1 = G.selection(C, 16, seed=6)
    sc0, sc1 = rng.integers(-3, 4, C).astype(F32), rng.integers(-3, 4, C).astype(F32)
    params = {"pre": G.feeder_params(16, False)[0]["pre"], "s0": [s0, np.zeros(C, F32)], "s1": [s1, np.zeros(C, F32)],
              "n0": [sc0], "n1": [sc1]}
    onet = L.forwarded(L.L2NormOracleNet(P.parse(L.concat_net_text(C)), params=params), data, np.array([[7, 9, 1]], F32))
    want = np.concatenate([L.normalize32(data[:, p0], sc0), L.normalize32(data[:, p1], sc1, 0.001)], axis=1)
    np.testing.assert_array_equal(onet.blobs["cat"].data, want)

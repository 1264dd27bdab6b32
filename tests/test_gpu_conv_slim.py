"""The SLIM form of the 4-wave kernel (conv_mfma_f16x3_w4d_slim_kernel, conv_f16x3_w4d.h: single 8-row tiles of the
short-K layers, one halo buffer and a ring of four tap slabs, three blocks per compute unit) against the two-per-CU form it replaces and against the oracle
(``-m gpu``).

The planner gives every 3x3 / dilation-1 layer with 64 <= Cin <= 128 and Cout % 128 == 0 the slim form;
SHF_F16X3_W4_SLIM=0 keeps the present one.  The knobs are read once per process, so ALL cases run in two child processes,
one per form, once per session; the tests then compare, case by case:
  * slim == present form, ``assert_array_equal``: the convolution's output, its fused 2x2 pool, and what the next layers
    make of them -- a following family convolution lifts its input by the max |value| slot the layer under test published,
    and the pass's range_fallbacks count says whether its range flag was raised;
  * slim within 2e-5 of the blob's maximum of the oracle's convolution (the per-layer bar of the other parity tests).
Shapes: Cin 64 / 128 are 4 / 8 chunks of 16 channels (the ring of four slabs wraps at 36 and 72 slabs), Cout 256 is two
cout tiles; 8x16 is exactly one tile, 9x17 has a ragged last row and column and halo pieces outside the image on every
side, 23x40 is several ragged tiles; 256x416 is 832 tiles, more than three blocks on each of 256 compute units.
Inputs: the split activation format on the fused path (a mini-detector, read out through one-hot predictors:
helpers.read_fused_blob) and fp32 on the per-layer path (a graph without a tail).  Epilogues: plain, pool + full map,
pool only."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import oracle as O
from smallhardface_amd import prototxt as P
from tests import helpers as H
from tests.test_gpu_fused_forms import C0, conv, pool

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ACT_TOL = 2e-5
CHANNELS = [(64, 128), (128, 128), (128, 256)]
MAPS = [(8, 16), (9, 17), (23, 40)]
KNOB = "SHF_F16X3_W4_SLIM"


# ------------------------------------------------------------------------------------------------------------
# cases: name -> (kind, cin, cout, epilogue, h, w, magnitude); h x w = the map of the layer under test, "ct"
# ------------------------------------------------------------------------------------------------------------
def _cases():
    cs = {}
    for cin, cout in CHANNELS:
        for h, w in MAPS:
            for epi in ("plain", "main_pool", "pool_only"):
                cs["split_%d_%d_%s_%dx%d" % (cin, cout, epi, h, w)] = ("fused", cin, cout, epi, h, w, None)
            cs["fp32_%d_%d_%dx%d" % (cin, cout, h, w)] = ("layer", cin, cout, "plain", h, w, None)
    cs["coresident_64_128_256x416"] = ("layer", 64, 128, "plain", 256, 416, None)
    cs["small_128_128_9x17"] = ("fused", 128, 128, "main_pool", 9, 17, "small")
    cs["top_128_128_9x17"] = ("fused", 128, 128, "main_pool", 9, 17, "top")
    cs["overflow_64_128_9x17"] = ("layer", 64, 128, "plain", 9, 17, "overflow")
    return cs


CASES = _cases()


def _graph(kind, cin, cout, epi, h, w):
    """(prototxt text, convolutions with random biases, probed blobs, input size)."""
    if kind == "layer":      # no proposal tail: the per-layer kernels, fp32 activations
        pre = C0 if cin == 64 else C0 + conv("c1", "c0", 128)
        bottom, stack = ("c0", ["c0"]) if cin == 64 else ("c1", ["c0", "c1"])
        return H.single_layer_net(pre + conv("ct", bottom, cout), 3, h, w), stack + ["ct"], ["ct"], (h, w)
    if cin == 64:            # the producer/consumer first pair's pooled map, in the split format
        pre, bottom, stack, size = C0 + conv("c1", "c0", 64) + pool("p", "c1"), "p", ["c0", "c1"], (2 * h, 2 * w)
    else:                    # conv1_1 in the 8-wave kernel's halo staging, split-format output
        pre, bottom, stack, size = C0 + conv("c1", "c0", 128), "c1", ["c0", "c1"], (h, w)
    txt = pre + conv("ct", bottom, cout)
    if epi == "plain":
        probes, stack = "ct", stack + ["ct"]
    elif epi == "pool_only":
        txt += pool("q", "ct")
        probes, stack = "q", stack + ["ct"]
    else:                    # ct is read by its pool and by c3 (a family convolution: it takes ct's published maximum)
        txt += pool("q", "ct") + conv("c3", "ct", cout) + pool("q3", "c3")      # (cout again: the read-out wants blobs of one shape)
        probes, stack = ["q", "q3"], stack + ["ct", "c3"]
    return H.mini_detector(txt, probes, 2, 3, size[0], size[1]), stack, [probes] if isinstance(probes, str) else probes, size


def _setup(name, with_gpu, scale=1.0):
    kind, cin, cout, epi, h, w, mag = CASES[name]
    txt, stack, probes, (ih, iw) = _graph(kind, cin, cout, epi, h, w)
    msg = P.parse(txt)
    if with_gpu:
        gnet, onet = H.make_pair(msg, seed=5)
    else:
        gnet, onet = None, O.OracleNet(msg, params=O.synth_params(msg, seed=5))
    rng = np.random.default_rng(3)
    sc = np.float32(scale)
    for lname in stack:
        onet.params[lname][1][...] = rng.normal(0, 0.5, onet.params[lname][1].shape).astype(np.float32) * sc
    if mag == "overflow":    # one output channel of ct leaves the fp16 range, its input does not
        onet.params["ct"][1][0] = 9.0e4
    for lname, blobs in onet.params.items():
        if lname.startswith("cls_score") or lname.startswith("bbox_pred"):
            for b in blobs:
                b[...] = 0
    if with_gpu:
        H.load_params(gnet, onet.params)
    data = rng.normal(0, 1, (1, 3, ih, iw)).astype(np.float32) * sc
    return gnet, onet, data, np.array([[ih, iw, 1]], np.float32), stack, probes


_ORACLE = {}


def _oracle(name):
    """(scale of input and biases, {probe: the oracle's blob}), once per case."""
    if name in _ORACLE:
        return _ORACLE[name]
    mag = CASES[name][6]

    def run(scale):
        _, onet, data, info, stack, probes = _setup(name, False, scale)
        onet.blobs['data'].reshape(*data.shape)
        onet.blobs['im_info'].reshape(1, 3)
        onet.forward(data=data, im_info=info)
        return onet, stack, probes
    scale = 1.0
    if mag == "small":
        scale = 2.0 ** -12
    elif mag == "top":       # positively homogeneous stack: the largest |activation| lands near 6e4, inside the fp16 range
        onet, stack, _ = run(1.0)
        scale = float(np.float32(6.0e4 / max(float(np.abs(onet.blobs[n].data).max()) for n in stack)))
    onet, stack, probes = run(scale)
    top = max(float(np.abs(onet.blobs[n].data).max()) for n in stack)
    if mag == "top":
        assert 5.8e4 < top < 65504
    if mag == "small":
        assert 0 < top < 64 * scale
    if mag == "overflow":
        assert top > 65504 and max(float(np.abs(onet.blobs[n].data).max()) for n in stack[:-1]) < 6.0e4
    _ORACLE[name] = (scale, {p: onet.blobs[p].data[0].copy() for p in probes})
    return _ORACLE[name]


# ------------------------------------------------------------------------------------------------------------
# the GPU side: one child process per form runs every case
# ------------------------------------------------------------------------------------------------------------
def _plan_is_slim(cin, cout, h, w, in_split, pooled):
    from smallhardface_amd import _lib
    fn = _lib.load().shf_debug_conv_plan
    fn.restype = C.c_int
    fn.argtypes = [C.c_int] * 6 + [C.POINTER(C.c_longlong), C.POINTER(C.c_longlong), C.POINTER(C.c_int)]
    lds, grid, slim = (C.c_longlong * 2)(), (C.c_longlong * 2)(), (C.c_int * 2)()
    assert fn(cin, cout, h, w, in_split, pooled, lds, grid, slim) == 1
    return int(slim[0])


def _grouped_rows():
    """One grouped pass over two units of different sizes -- 9x17 and 23x40 at the layer under test, so that the launch's
    tile -> member decoding crosses a member boundary -- and the same units one at a time: the exported rows."""
    import torch
    from smallhardface_amd import test as T
    txt = C0 + conv("c1", "c0", 64) + pool("p", "c1") + conv("ct", "p", 128)
    gnet, onet = H.make_pair(P.parse(H.mini_detector(txt, "ct", 2, 3, 18, 34)), seed=5, cls_bias=1.0)
    rng = np.random.default_rng(3)
    for lname in ("c0", "c1", "ct"):
        onet.params[lname][1][...] = rng.normal(0, 0.5, onet.params[lname][1].shape).astype(np.float32)
    H.load_params(gnet, onet.params)
    gnet.set_conv_mode("f16x3")
    units = []
    for k, (h, w) in enumerate([(18, 34), (46, 80)]):
        g = np.float32([1.0, 2.0 ** -6][k])                      # units whose activation exponents differ
        units.append((rng.normal(0, 1, (1, 3, h, w)).astype(np.float32) * g, h, w, h, w, 1.0, False))
    fd = T.FusedDetector(gnet, n_lanes=2, mode="group")
    fd.lanes[0].detect_add_levels(fd.lanes[:2], units, 0.05, per_member_lists=True)
    fd.lanes[0].sync()
    buf = torch.empty((40000, 5), dtype=torch.float32, device="cuda")
    out = {}
    for m, u in enumerate(units):
        n = fd.lanes[m].detect_export(buf.data_ptr(), 40000)
        out["grouped_%d" % m] = buf[:n].cpu().numpy()
        gnet.detect_begin()
        gnet.detect_add_level(*u, 0.05)
        n = gnet.detect_export(buf.data_ptr(), 40000)
        out["single_%d" % m] = buf[:n].cpu().numpy()
    assert gnet.range_fallbacks == 0
    return out


def _whole_net_rows():
    """The detector's own graph, seeded: a 112x112 and a 304x304 unit in one fused grouped pass -> the rows per unit."""
    import torch
    from smallhardface_amd import test as T
    gnet, _ = H.make_pair(H.detector_msg(), seed=7, cls_bias=1.0)
    gnet.set_conv_mode("f16x3")
    units = [(H.synth_image_blob(s, s, seed=s), s, s, s, s, 1.0, False) for s in (112, 304)]
    fd = T.FusedDetector(gnet, n_lanes=2, mode="group")
    fd.lanes[0].detect_add_levels(fd.lanes[:2], units, 0.05, per_member_lists=True)
    fd.lanes[0].sync()
    buf = torch.empty((200000, 5), dtype=torch.float32, device="cuda")
    out = {}
    for m in range(2):
        n = fd.lanes[m].detect_export(buf.data_ptr(), 200000)
        out["net_%d" % m] = buf[:n].cpu().numpy()
    out["net_fallbacks"] = np.array([gnet.range_fallbacks])
    return out


def _child(out):
    """Entry of the two children: every case on the GPU -> out.npz (blobs, rows) / out.json (fallbacks, planner flags)."""
    arrays, meta = {}, {}
    for name, (kind, cin, cout, epi, h, w, mag) in CASES.items():
        scale = 1.0 if mag in (None, "overflow") else json.load(open(out + ".scales.json"))[name]
        gnet, onet, data, info, stack, probes = _setup(name, True, scale)
        gnet.set_conv_mode("f16x3")
        before = gnet.range_fallbacks
        if kind == "fused":
            got = H.read_fused_blob(gnet, onet, data, info)
            got = got if isinstance(got, list) else [got]
        else:
            for b, shp in (("data", data.shape), ("im_info", (1, 3))):
                gnet.blobs[b].reshape(*shp)
            gnet.forward(data=data, im_info=info)
            got = [np.array(gnet.blobs[p].data[0]) for p in probes]
        for p, a in zip(probes, got):
            arrays["%s__%s" % (name, p)] = a
        meta[name] = dict(range_fallbacks=int(gnet.range_fallbacks - before),
                          slim=_plan_is_slim(cin, cout, h, w, 1 if kind == "fused" else 0, 0 if epi == "plain" else 1))
    arrays.update(_grouped_rows())
    arrays.update(_whole_net_rows())
    np.savez(out + ".npz", **arrays)
    json.dump(meta, open(out + ".json", "w"))


@pytest.fixture(scope="module")
def forms(tmp_path_factory):
    """{"slim" / "present": (arrays, meta)}: both children, one after the other."""
    res = {}
    scales = {n: _oracle(n)[0] for n, c in CASES.items() if c[6] in ("small", "top")}
    for form, knob in (("slim", "1"), ("present", "0")):
        out = str(tmp_path_factory.mktemp(form) / "cases")
        json.dump(scales, open(out + ".scales.json", "w"))
        code = "from tests import test_gpu_conv_slim as M; M._child(%r)" % out
        r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, PYTHONPATH=ROOT, **{KNOB: knob}), cwd=ROOT,
                           capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, (form, r.stderr[-3000:])
        res[form] = (dict(np.load(out + ".npz")), json.load(open(out + ".json")))
    return res


@pytest.mark.parametrize("name", sorted(CASES))
def test_slim_equals_present_form_and_matches_oracle(forms, name):
    kind, cin, cout, epi, h, w, mag = CASES[name]
    _, want = _oracle(name)
    (sa, sm), (pa, pm) = forms["slim"], forms["present"]
    assert sm[name]["slim"] == 1 and pm[name]["slim"] == 0          # the planner really chose the two forms
    # the range flag: raised by both or by neither (a raised flag redoes the pass on the fp32 kernels)
    assert sm[name]["range_fallbacks"] == pm[name]["range_fallbacks"] == (1 if mag == "overflow" else 0)
    for p, ref in want.items():
        got, present = sa["%s__%s" % (name, p)], pa["%s__%s" % (name, p)]
        assert got.shape == ref.shape, (p, got.shape, ref.shape)
        err = H.rel_err(got, ref)
        print(name, p, "rel err vs oracle %.3g" % err, "max |ref| %.3g" % float(np.abs(ref).max()))
        np.testing.assert_array_equal(got, present)
        assert err < ACT_TOL, (name, p, err)
    if epi != "plain":       # (an odd map: the pooled map's last row / column is a clipped window)
        assert want["q"].shape[1:] == ((h + 1) // 2, (w + 1) // 2)


def test_grouped_launch_over_two_units(forms):
    (sa, _), (pa, _) = forms["slim"], forms["present"]
    rows = 0
    for m in range(2):
        np.testing.assert_array_equal(sa["grouped_%d" % m], pa["grouped_%d" % m])
        np.testing.assert_array_equal(sa["grouped_%d" % m], sa["single_%d" % m])     # grouped == one at a time, bit for bit
        rows += len(sa["grouped_%d" % m])
    assert rows > 0


def test_whole_net_detections_are_the_same(forms):
    (sa, _), (pa, _) = forms["slim"], forms["present"]
    for m in range(2):
        assert len(sa["net_%d" % m]) > 0
        np.testing.assert_array_equal(sa["net_%d" % m], pa["net_%d" % m])
    assert sa["net_fallbacks"][0] == pa["net_fallbacks"][0] == 0

"""Results must not depend on what the device buffers held before (``-m gpu``).  Cases: tests/buffer_history_cases.py.

Every device buffer of the runtime is grow-only and almost nothing is cleared, so a result is right only if no kernel reads a
byte that the pass did not write.  Three child processes, one after the other (SHF_POISON_ALLOC is read once per process): the
knob unset, 0xff (fp32 and fp16 NaN, int -1) and 0x7f (fp32 3.4e38, fp16 NaN, int 2139062143).  Each child runs

  * per graph and conv mode ONE long-lived net over the sizes A, B, A, C, B, and a newly constructed net per distinct size;
    at every visit: the forward's outputs (the fused pass where the graph has a tail), every blob of the family's list read
    afterwards (the per-layer path), the fused map through helpers.read_fused_blob where the graph's own test reads it so,
    the change in range_fallbacks, alloc_counts() and the set of kernel classes that launched;
  * a walk through the conv modes on one net; forward_group over three lanes with the sizes rotated twice;
  * the detector drivers (FusedDetector in group mode over a DevicePyramid) on three images in six orders, a driver each;
  * the multi-class tail's class lists on two images in both orders; the evaluators and the box merge, each first on its
    small input in a fresh process, then on a larger one, then on the small one again.

Every array is recorded as (shape, dtype, SHA-1 of its bytes) -- a 512-channel 128 x 256 map is 64 MiB, and there are hundreds
-- and equality below is equality of those triples: bit for bit, shapes included (stricter than assert_array_equal: -0.0 and
NaN payloads count).  Arrays up to 1 MiB, and the fresh nets' last feature blobs, travel whole, so that a mismatch of those is
reported element by element and the oracle comparison has its values.

Wall time of the children on an MI355X, measured there: 23.8 s (knob unset), 23.6 s (0xff), 23.5 s (0x7f), of which the two
templates take 7.6 s, the detector drivers 3.9 s, m1 2.5 s and fam16 2.0 s; the fixture prints each child's time per graph.
"""
import hashlib
import json
import os
import subprocess
import sys
import time

import numpy as np
import pytest

from tests import buffer_history_cases as B
from tests import helpers as H

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KNOB = "SHF_POISON_ALLOC"
CHILDREN = (("clean", None), ("ff", "0xff"), ("7f", "0x7f"))
KEEP_BYTES = 1 << 20


# ------------------------------------------------------------------------------------------------------------
# the child
# ------------------------------------------------------------------------------------------------------------
class _Rec(object):
    def __init__(self, keep_large=True):
        self.arrays, self.digest, self.finite, self.meta = {}, {}, {}, {}
        self.keep_large = keep_large                     # arrays beyond KEEP_BYTES that the oracle comparison needs

    def put(self, name, a, keep=False):
        a = np.ascontiguousarray(a)
        assert name not in self.digest, name
        self.digest[name] = [list(a.shape), str(a.dtype), hashlib.sha1(a.tobytes()).hexdigest()]
        self.finite[name] = bool(np.isfinite(a).all()) if a.dtype.kind == "f" else True
        if keep or a.nbytes <= KEEP_BYTES:
            self.arrays[name] = a


class _cfg_of(object):
    """cfg.TEST's three proposal settings of one case, restored afterwards."""

    def __init__(self, triple):
        self.triple = triple

    def __enter__(self):
        from smallhardface_amd.config import cfg
        self.old = (cfg.TEST.SCORE_THRESH, cfg.TEST.ANCHOR_MIN_SIZE, cfg.TEST.N_DETS_PER_MODULE)
        cfg.TEST.SCORE_THRESH, cfg.TEST.ANCHOR_MIN_SIZE, cfg.TEST.N_DETS_PER_MODULE = self.triple

    def __exit__(self, *exc):
        from smallhardface_amd.config import cfg
        cfg.TEST.SCORE_THRESH, cfg.TEST.ANCHOR_MIN_SIZE, cfg.TEST.N_DETS_PER_MODULE = self.old


_UNITS = {}


def _unit(case, size):
    """(prototxt text, parameters, data, im_info) of one size, once per child."""
    if (case.key, size) not in _UNITS:
        text, onet, data, info = case.setup(*size)
        _UNITS[(case.key, size)] = (text, onet.params, data, info)
    return _UNITS[(case.key, size)]


def _new_net(case, size, mode):
    from smallhardface_amd import caffe
    text, params, _, _ = _unit(case, size)
    net = caffe.Net(None, prototxt_text=text)
    H.load_params(net, params)
    net.set_conv_mode(mode)
    return net


def _classes(net):
    return sorted(k for k, v in net.prof_read().items() if int(v["launches"]) > 0)


def _record_net(rec, tag, case, net, keep_last=False):
    """Outputs are recorded by the caller; this reads the family's blobs of a forwarded net."""
    for name in case.blobs:
        rec.put("%s/blob/%s" % (tag, name), np.array(net.blobs[name].data), keep=keep_last and name in case.last)


def _visit(rec, tag, case, net, size, mode, keep_last=False):
    from smallhardface_amd import caffe
    keep_last = keep_last and rec.keep_large
    _, params, data, info = _unit(case, size)
    before = net.range_fallbacks
    net.prof_enable(True)
    net.prof_reset()
    net.blobs["data"].reshape(*data.shape)
    net.blobs["im_info"].reshape(*info.shape)
    out = net.forward(data=data, im_info=info)
    for k in sorted(out):
        rec.put("%s/out/%s" % (tag, k), np.array(out[k]))
    _record_net(rec, tag, case, net, keep_last)
    if case.fused and mode == "f16x3":
        fused = H.read_fused_blob(net, case.setup(*size)[1], data, info, mode)
        for j, a in enumerate(fused if isinstance(fused, list) else [fused]):
            rec.put("%s/fused/%d" % (tag, j), a, keep=keep_last)
        H.load_params(net, params)                       # (the read-out left one-hot predictors behind)
    rec.meta[tag] = dict(redo=int(net.range_fallbacks - before), allocs=list(caffe.alloc_counts()), classes=_classes(net))
    net.prof_enable(False)


def _size_tag(size):
    return "%dx%d" % size


def _run_nets(rec, keys):
    for key in keys:
        case = B.CASES[key]
        with _cfg_of(case.cfg):
            for mode in case.modes:
                net = _new_net(case, case.sizes[0], mode)
                for i, size in enumerate(case.sequence(mode)):
                    _visit(rec, "long/%s/%s/%d" % (key, mode, i), case, net, size, mode)
                del net
                for size in case.distinct_sizes(mode):
                    net = _new_net(case, size, mode)
                    _visit(rec, "fresh/%s/%s/%s" % (key, mode, _size_tag(size)), case, net, size, mode, keep_last=mode in B.MODES)
                    del net
            if key == "slim":
                rec.meta["plan/slim"] = {_size_tag(s): B.slim_plan(*s) for s in case.sizes}
            if key in B.EXTRA_KEYS:
                net = _new_net(case, case.sizes[0], B.MODE_WALK[0])
                for i, mode in enumerate(B.MODE_WALK):
                    net.set_conv_mode(mode)
                    _visit(rec, "walk/%s/%d" % (key, i), case, net, case.sizes[0], mode)
                del net
            if key in B.GROUP_KEYS:
                for mode in B.MODES:
                    root = _new_net(case, case.group_sizes[0], mode)
                    lanes = [root.clone() for _ in case.group_sizes]
                    for rot in range(3):
                        sizes = case.group_sizes[rot:] + case.group_sizes[:rot]
                        ins = []
                        for lane, size in zip(lanes, sizes):
                            _, _, data, info = _unit(case, size)
                            lane.blobs["data"].reshape(*data.shape)
                            lane.blobs["im_info"].reshape(*info.shape)
                            ins.append({"data": data, "im_info": info})
                        outs = root.forward_group(lanes, ins)
                        for k, (lane, out) in enumerate(zip(lanes, outs)):
                            tag = "group/%s/%s/%d/%d" % (key, mode, rot, k)
                            for name in sorted(out):
                                rec.put("%s/out/%s" % (tag, name), np.array(out[name]))
                            _record_net(rec, tag, case, lane)
                    del lanes, root


def _run_multiclass(rec):
    from smallhardface_amd import caffe
    from smallhardface_amd import prototxt as P
    from tests import multiclass_cases as M
    msg = P.parse(M.whole_net_txt(3, False))
    params = M.whole_params(msg)
    inputs = [M.whole_input(h, w) for h, w in B.MULTICLASS_SIZES]
    with _cfg_of((B.MULTICLASS_CFG["score_thresh"], 0.0, B.MULTICLASS_CFG["pre_nms_topN"])):
        for order in B.MULTICLASS_ORDERS:
            net = caffe.Net(None, prototxt_text=P.dumps(msg))
            H.load_params(net, params)
            net.set_conv_mode("f16x3")
            for n, c in enumerate(order):
                data, info = inputs[int(c)]
                net.blobs["data"].reshape(*data.shape)
                net.blobs["im_info"].reshape(*info.shape)
                out = net.forward(data=data, im_info=info)
                tag = "mc/%s/%d/im%s" % (order, n, c)
                for k in sorted(out):
                    rec.put("%s/out/%s" % (tag, k), np.array(out[k]))
                net.class_lists_begin()
                net.class_lists_add([net], [8 * data.shape[3]], [1.0], [False], B.MULTICLASS_THRESH)
                rec.meta[tag] = dict(counts=[int(v) for v in net.class_lists_count()])
                for cls in range(1, net.num_classes):
                    rec.put("%s/list/%d" % (tag, cls), np.array(net.class_lists_export(cls)))
            del net


def _eval_inputs():
    """name -> (small input, larger input of the same kind, fn(input) -> {array name: array}) of the four device entries."""
    from smallhardface_amd import face_eval as FE
    from smallhardface_amd import fddb_eval as FD
    from smallhardface_amd import wider_eval as W
    from smallhardface_amd.nms import bbox_vote, nms
    from tests import face_eval_cases as FK
    from tests import fddb_eval_cases as DK
    from tests import wider_eval_cases as WK

    def wider(inp):
        totals, hits, prop = W.device_counts(W.flatten_inputs(*inp), 0.5, True, W.sweep_thresholds(), diagnostics=True)
        return dict(totals=totals, hits=hits, proposal=prop)

    def face(inp):
        _, code, index = FK.one_round(inp[0], inp[1], 0.5, FE.match_device)
        return dict(code=code, index=index)

    def fddb(inp):
        res = FD.evaluate(inp[0], inp[1], sizes=inp[2], device=True)
        return {k: np.asarray(res[k]) for k in ("inter", "ann_area", "det_area", "m", "disc", "cont")}

    def merge(d):
        return dict(keep=np.asarray(nms(d, 0.4)), vote=np.asarray(bbox_vote(d, 0.4)))

    rng = np.random.default_rng(5)
    p, b = WK.make_image(rng, 3, 70, True)
    wider_small = ([p], [b], [[k] for k in WK.subsets(rng, 3)])
    return {
        "wider": (wider_small, WK.boundary_batch(20, False), wider),
        "face": (FK.batch(43, [(1, 1)]), FK.batch(41, FK.boundary_shapes()), face),
        "fddb": (DK.three_images() + (DK.THREE_SIZES,), DK.batch(11, [(a, d) for a in (0, 1, 3) for d in (0, 1, 64, 65)]), fddb),
        "merge": (B.nms_dets(B.NMS_N[0]), B.nms_dets(B.NMS_N[1]), merge),
    }


def _run_evaluators(rec):
    for name, (small, large, fn) in _eval_inputs().items():
        for tag, inp in (("fresh", small), ("large", large), ("after_large", small)):
            for k, a in fn(inp).items():
                rec.put("eval/%s/%s/%s" % (name, tag, k), a)


def _run_detector(rec):
    """The drivers last: they load the detector's own configuration into cfg."""
    from smallhardface_amd import caffe, weights
    from smallhardface_amd import prototxt as P
    from smallhardface_amd import test as T
    from smallhardface_amd.config import cfg, cfg_from_file
    cfg_from_file(os.path.join(ROOT, "configs", "smallhardface.toml"))
    cfg.TEST.SCALES = list(B.DETECTOR_SCALES)
    msg = H.detector_msg(True)
    params = weights.synth_params(msg, cls_bias=1.0)
    ims = B.detector_images()
    for order in B.DETECTOR_ORDERS:
        net = caffe.Net(None, prototxt_text=P.dumps(msg))
        H.load_params(net, params)
        net.set_conv_mode("f16x3")
        fd = T.FusedDetector(net, n_lanes=4, mode="group")
        dp = T.DevicePyramid(net, n_slots=2)
        queued, seen = [], {}

        def collect():
            j = queued.pop(0)
            seen[j] = seen.get(j, 0) + 1
            rec.put("det/%s/im%d/%d" % (order, j, seen[j] - 1), np.asarray(fd.collect()[0]))

        for c in order:
            fd.submit(dp.units(ims[int(c)], net=fd.next_head()), 0.05, on_device=True)
            queued.append(int(c))
            if fd.pending() > 1:
                collect()
        while queued:
            collect()
        rec.meta["det/%s" % order] = dict(redo=int(net.range_fallbacks))
        del fd, dp, net


def _child(out, want_byte):
    t0 = time.time()
    from smallhardface_amd import _lib, caffe
    caffe.set_mode_gpu()
    caffe.set_device(0)
    got = int(_lib.load().shf_debug_poison_byte())
    assert got == int(want_byte), "the library parsed %s = %r as %d" % (KNOB, os.environ.get(KNOB), got)
    rec = _Rec(keep_large=got < 0)
    timing = rec.meta["timing"] = {}

    def timed(name, fn, *args):
        t = time.time()
        fn(rec, *args)
        timing[name] = round(time.time() - t, 2)

    timed("evaluators", _run_evaluators)             # first: "fresh" is the first call of its kind in the process
    for key in B.KEYS:
        timed(key, _run_nets, [key])
    timed("multiclass", _run_multiclass)
    timed("detector", _run_detector)
    rec.meta["seconds"] = time.time() - t0
    rec.meta["poison_byte"] = got
    np.savez(out + ".npz", **rec.arrays)
    json.dump(dict(digest=rec.digest, finite=rec.finite, meta=rec.meta), open(out + ".json", "w"))
    print("buffer history child %s=%s: %.1f s, %d arrays" % (KNOB, os.environ.get(KNOB), rec.meta["seconds"], len(rec.digest)))


# ------------------------------------------------------------------------------------------------------------
# the three children, one after the other
# ------------------------------------------------------------------------------------------------------------
class _Result(object):
    def __init__(self, out):
        j = json.load(open(out + ".json"))
        self.digest, self.finite, self.meta = j["digest"], j["finite"], j["meta"]
        self.arrays = np.load(out + ".npz")

    def under(self, prefix):
        return sorted(k[len(prefix) + 1:] for k in self.digest if k.startswith(prefix + "/"))


_FIXTURE = {}


@pytest.fixture(scope="module")
def children(tmp_path_factory):
    # (pytest sets a module fixture up again for every test after it raised: a child that failed must not run again)
    if "error" in _FIXTURE:
        pytest.fail("the children did not finish: " + _FIXTURE["error"], pytrace=False)
    try:
        return _run_children(tmp_path_factory)
    except BaseException as e:
        _FIXTURE["error"] = "%s: %s" % (type(e).__name__, str(e)[:4000])
        raise


def _run_children(tmp_path_factory):
    res = {}
    for name, byte in CHILDREN:
        out = str(tmp_path_factory.mktemp(name) / "rec")
        env = {k: v for k, v in os.environ.items() if k != KNOB}
        env["PYTHONPATH"] = ROOT
        if byte is not None:
            env[KNOB] = byte
        code = "from tests import test_gpu_buffer_history as M; M._child(%r, %d)" % (out, -1 if byte is None else int(byte, 0))
        t0 = time.time()
        r = subprocess.run([sys.executable, "-c", code], env=env, cwd=ROOT, capture_output=True, text=True, timeout=900)
        # a child that faulted, aborted or timed out ends the fixture: a finding to be read for its cause, not re-run
        assert r.returncode == 0, (name, r.returncode, r.stdout[-1000:], r.stderr[-3000:])
        res[name] = _Result(out)
        print("child %s: %.1f s wall (%.1f s inside) %s" % (name, time.time() - t0, res[name].meta["seconds"], res[name].meta["timing"]))
    return res


def _same(ra, pa, rb, pb):
    """Every array under prefix pa of result ra equals, bit for bit, the one of the same name under pb of rb."""
    na, nb = ra.under(pa), rb.under(pb)
    assert na == nb and na, (pa, pb, sorted(set(na) ^ set(nb)))
    for n in na:
        a, b = pa + "/" + n, pb + "/" + n
        if ra.digest[a] == rb.digest[b]:
            continue
        assert ra.digest[a][:2] == rb.digest[b][:2], (a, b, ra.digest[a][:2], rb.digest[b][:2])       # shape, dtype
        if a in ra.arrays.files and b in rb.arrays.files:
            np.testing.assert_array_equal(ra.arrays[a].view(np.uint8), rb.arrays[b].view(np.uint8), err_msg="%s vs %s" % (a, b))
        raise AssertionError("%s differs from %s (%s, %s)" % (a, b, ra.digest[a], rb.digest[b]))


def _visits(key):
    """(tag of a long-lived visit, mode, size) of every visit of the key's sequences."""
    case = B.CASES[key]
    return [("long/%s/%s/%d" % (key, mode, i), mode, size) for mode in case.modes for i, size in enumerate(case.sequence(mode))]


# ---- 5. the knob reached the library (each child asserts it; here: the three differ as asked) ----------------------------------------
def test_the_knob_reached_the_library(children):
    assert [children[n].meta["poison_byte"] for n, _ in CHILDREN] == [-1, 0xff, 0x7f]


# ---- 1. history --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("child", [n for n, _ in CHILDREN])
@pytest.mark.parametrize("key", B.KEYS)
def test_every_visit_equals_a_fresh_net(children, key, child):
    r = children[child]
    case = B.CASES[key]
    for tag, mode, size in _visits(key):
        fresh = "fresh/%s/%s/%s" % (key, mode, _size_tag(size))
        _same(r, tag, r, fresh)
        assert r.meta[tag]["redo"] == r.meta[fresh]["redo"], (tag, r.meta[tag]["redo"], r.meta[fresh]["redo"])
    if key in B.EXTRA_KEYS:
        for i, mode in enumerate(B.MODE_WALK):
            tag, fresh = "walk/%s/%d" % (key, i), "fresh/%s/%s/%s" % (key, mode, _size_tag(case.sizes[0]))
            _same(r, tag, r, fresh)
            assert r.meta[tag]["redo"] == r.meta[fresh]["redo"], tag
    if key in B.GROUP_KEYS:
        for mode in B.MODES:
            for rot in range(3):
                sizes = case.group_sizes[rot:] + case.group_sizes[:rot]
                for k, size in enumerate(sizes):
                    _same(r, "group/%s/%s/%d/%d" % (key, mode, rot, k), r, "fresh/%s/%s/%s" % (key, mode, _size_tag(size)))


@pytest.mark.parametrize("child", [n for n, _ in CHILDREN])
def test_every_image_of_every_order_equals_the_image_alone(children, child):
    r = children[child]
    for order in B.DETECTOR_ORDERS:
        assert r.meta["det/%s" % order]["redo"] == 0
        for j in sorted(set(order)):
            runs = r.under("det/%s/im%s" % (order, j))
            assert len(runs) == order.count(j)
            for n in runs:
                a, b = "det/%s/im%s/%s" % (order, j, n), "det/%s/im%s/0" % (j, j)
                assert r.digest[a] == r.digest[b], (a, r.digest[a], r.digest[b])
            assert r.digest["det/%s/im%s/0" % (j, j)][0][0] > 0              # (the image has detections)
    for order in B.MULTICLASS_ORDERS:
        for n, c in enumerate(order):
            tag, alone = "mc/%s/%d/im%s" % (order, n, c), "mc/%s/0/im%s" % (c, c)
            _same(r, tag, r, alone)
            assert r.meta[tag]["counts"] == r.meta[alone]["counts"] and sum(r.meta[tag]["counts"]) > 0
    for name in ("wider", "face", "fddb", "merge"):
        _same(r, "eval/%s/after_large" % name, r, "eval/%s/fresh" % name)


# ---- 2. poison ---------------------------------------------------------------------------------------------------------------------
def _groups():
    return ["long/" + k for k in B.KEYS] + ["fresh/" + k for k in B.KEYS] + ["walk/" + k for k in B.EXTRA_KEYS] + \
        ["group/" + k for k in B.GROUP_KEYS] + ["det", "mc", "eval"]


@pytest.mark.parametrize("child", ["ff", "7f"])
@pytest.mark.parametrize("group", _groups())
def test_poisoned_allocations_change_nothing(children, group, child):
    clean, r = children["clean"], children[child]
    _same(r, group, clean, group)
    for res in (clean, r):
        bad = [k for k in res.digest if k.startswith(group + "/") and not res.finite[k]]
        assert not bad, bad[:8]
    for tag in [t for t in clean.meta if isinstance(clean.meta[t], dict) and t.startswith(group + "/") and "redo" in clean.meta[t]]:
        assert r.meta[tag]["redo"] == clean.meta[tag]["redo"], tag


def test_the_children_recorded_the_same_names(children):
    names = [sorted(children[n].digest) for n, _ in CHILDREN]
    assert names[0] == names[1] == names[2] and len(names[0]) > 1000


# ---- 3. not garbage against garbage ------------------------------------------------------------------------------------------------
_ORACLES = {}


def _oracle(key, size):
    if (key, size) not in _ORACLES:
        _ORACLES[(key, size)] = B.CASES[key].oracle(*size)
    return _ORACLES[(key, size)]


@pytest.mark.parametrize("key", B.KEYS)
def test_fresh_nets_against_the_oracle(children, key):
    r = children["clean"]
    case = B.CASES[key]
    for mode in B.MODES:
        for size in case.distinct_sizes(mode):
            tag = "fresh/%s/%s/%s" % (key, mode, _size_tag(size))
            onet = _oracle(key, size)
            for name in case.last:
                got, want = r.arrays["%s/blob/%s" % (tag, name)], onet.blobs[name].data
                assert got.shape == want.shape, (tag, name, got.shape, want.shape)
                err = H.rel_err(got, want)
                print(tag, name, "rel err %.3g" % err)
                assert err < B.ACT_TOL, (tag, name, err)
            if case.fused and mode == "f16x3":
                for j, name in enumerate(case.last):
                    got, want = r.arrays["%s/fused/%d" % (tag, j)], onet.blobs[name].data[0]
                    assert got.shape == want.shape and H.rel_err(got, want) < B.ACT_TOL, (tag, name, H.rel_err(got, want))
            outs = [n for n in r.under(tag) if n.startswith("out/cls_prob")]
            assert outs or key == "pool_group"
            for n in outs:
                assert r.digest[tag + "/" + n][0][0] > 1, (tag, n, r.digest[tag + "/" + n][0])


def test_evaluators_against_the_host(children):
    from smallhardface_amd import face_eval as FE
    from smallhardface_amd import fddb_eval as FD
    from tests import face_eval_cases as FK
    from tests import wider_eval_cases as WK
    r = children["clean"]
    ins = _eval_inputs()
    for tag, inp in (("fresh", ins["wider"][0]), ("large", ins["wider"][1])):
        want = dict(zip(("totals", "hits", "proposal"), WK.host_counts(inp[0], inp[1], inp[2], 0.5, True)))
        for k, w in want.items():
            np.testing.assert_array_equal(r.arrays["eval/wider/%s/%s" % (tag, k)], w)
    for tag, inp in (("fresh", ins["face"][0]), ("large", ins["face"][1])):
        _, code, index = FK.one_round(inp[0], inp[1], 0.5, FE.match_host)
        np.testing.assert_array_equal(r.arrays["eval/face/%s/code" % tag], code)
        np.testing.assert_array_equal(r.arrays["eval/face/%s/index" % tag], index)
    for tag, inp in (("fresh", ins["fddb"][0]), ("large", ins["fddb"][1])):
        want = FD.evaluate(inp[0], inp[1], sizes=inp[2])
        for k in ("inter", "ann_area", "det_area", "m", "disc", "cont"):
            np.testing.assert_array_equal(r.arrays["eval/fddb/%s/%s" % (tag, k)], np.asarray(want[k]))
    assert r.digest["eval/merge/fresh/keep"][0][0] > 1000 and r.digest["eval/merge/fresh/vote"][0][0] > 1000


# ---- 4. the sequence did what it is there for --------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", B.KEYS)
def test_the_large_size_reallocates(children, key):
    r = children["clean"]
    for mode in B.MODES:
        second_a, c = r.meta["long/%s/%s/2" % (key, mode)]["allocs"], r.meta["long/%s/%s/3" % (key, mode)]["allocs"]
        assert c[0] > second_a[0], (key, mode, second_a, c)


@pytest.mark.parametrize("key", B.FORM_KEYS)
def test_the_sizes_cross_a_kernel_form(children, key):
    """fam16 and template_dd: the sets of launched kernel classes differ between sizes of the sequence.  The other two forms
    cannot show there at any size, so they are held to what does change with their sizes: the profiler books the slim form
    under the family's <true, 2, 1> class, which every short-K layer takes at every size (w4_pick_mt, csrc/conv_f16x3.hip) --
    the planner must give the layer under test the slim form on one tile, four ragged tiles and nine; and both forms of a
    global pooling layer are `pool_kernel` launches -- the sizes must lie on both sides of pool.hip's kPoolGlobalT."""
    r = children["clean"]
    case = B.CASES[key]
    sets = {size: tuple(r.meta["long/%s/f16x3/%d" % (key, i)]["classes"]) for i, size in enumerate(case.sequence("f16x3"))}
    common = set.intersection(*map(set, sets.values()))
    print(key, {s: [c for c in v if c not in common] for s, v in sets.items()})
    if key == "slim":
        plans = [r.meta["plan/slim"][_size_tag(s)] for s in case.sizes]
        assert [p["slim"] for p in plans] == [1, 1, 1] and [p["grid"] for p in plans] == [4, 1, 9], plans
        assert "conv_mfma_f16x3_w4d_kernel<true, 2, 1, 3, false, 1>" in common
    elif key == "pool_group":
        from tests import pooling_cases as K
        assert [h * w > K.GLOBAL_T for h, w in case.sizes] == [True, False, True] and "pool_kernel" in common
    else:
        assert len(set(sets.values())) > 1, (key, sets)

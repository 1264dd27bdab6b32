"""The FUSED-PATH forms of the split-fp16 convolutions against the oracle, layer by layer (``-m gpu``).

Net.forward() takes the fused path -- the producer/consumer first pair, the 8-wave kernel's FUSE1 form, the 4-wave family
reading and writing the split activation format, the 2x2 max-pool in the epilogues, the 1x1 GEMM, the dilated and the
three-head kernels with split input -- only on a graph with a proposal tail, and reading an intermediate blob afterwards
re-runs the PER-LAYER kernels.  So every case here is a mini-detector (helpers.mini_detector): a stack of at most three
convolutions with random biases, then a tail whose one-hot predictors copy the probed blob into the logits exactly
(helpers.read_fused_blob; the per-blob tail uses exact one-hot rows as well, 4 channels per blob and forward).  The blob
the fused kernels produced is compared element for element with the oracle's at the per-layer tests' own bar, 2e-5 of
the blob's maximum, and the profiler must show that the kernel class the case is about ran -- and what it replaces did
not.  Every case's rel_err, next to the per-layer kernels' on the same graph and data (gnet.blobs[probe].data after the
fast forward IS the per-layer recomputation), goes to fused_forms_parity.json in the directory SHF_TEST_REPORT_DIR names
(default: test_reports/ in the repository root, which git ignores).

Knob-selected forms run in a child process each (conv_knobs() reads the environment once), one at a time.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import oracle as O
from smallhardface_amd import prototxt as P
from tests import helpers as H

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ACT_TOL = 2e-5
REPORT = {}

PCP = "conv_mfma_f16x3_pc_kernel<3, false, true>"
PC = "conv_mfma_f16x3_pc_kernel<3, false, false>"
FUSE1 = "conv_mfma_f16x3_kernel<64, true, 1, 3, 3, false>"
W8_64 = "conv_mfma_f16x3_kernel<64, false, 1, 3, 3, false>"
K1 = "conv_mfma_f16x3_k1_kernel<true, 3>"
HEADS3 = "conv_mfma_f16x3_heads3_kernel<true, 3>"
FIRST, POOLK = "conv_first_kernel", "maxpool_kernel"


def W4(split, mt, nt, dil=1):
    return "conv_mfma_f16x3_w4d_kernel<%s, %d, %d, 3, false, %d>" % ("true" if split else "false", mt, nt, dil)


W4_SPLIT_ANY = "any split-input family kernel"     # (the sum over the four <true, MT, NTILE> classes)


def _report(key, **kw):
    REPORT[key] = kw
    try:
        out = os.environ.get("SHF_TEST_REPORT_DIR") or os.path.join(ROOT, "test_reports")
        os.makedirs(out, exist_ok=True)
        json.dump(REPORT, open(os.path.join(out, "fused_forms_parity.json"), "w"), indent=1, sort_keys=True)
    except OSError:
        pass


# ------------------------------------------------------------------------------------------------------------
# graphs: (layers text, convolutions of the stack, probe)
# ------------------------------------------------------------------------------------------------------------
def conv(name, bottom, nout, k=3, dil=1, relu=True, shared=False):
    s = ('layer { name: "%s" type: "Convolution" bottom: "%s" top: "%s" %sconvolution_param { num_output: %d '
         'kernel_size: %d pad: %d dilation: %d } }\n'
         % (name, bottom, name, 'param { name: "hw" } param { name: "hb" } ' if shared else "", nout, k, dil if k == 3 else 0, dil))
    if relu:
        s += 'layer { name: "%s_relu" type: "ReLU" bottom: "%s" top: "%s" }\n' % (name, name, name)
    return s


def pool(name, bottom):
    return ('layer { name: "%s" type: "Pooling" bottom: "%s" top: "%s" pooling_param { pool: MAX kernel_size: 2 stride: 2 } }\n'
            % (name, bottom, name))


C0 = conv("c0", "data", 64)
GRAPHS = {
    # the first pair on the producer/consumer kernel (pool-only, pooled map in the split format), read by a family conv
    "first": (C0 + conv("c1", "c0", 64) + pool("p", "c1") + conv("c2", "p", 128), ["c0", "c1", "c2"], "c2"),
    # conv1_1 in the 8-wave kernel's halo staging (Cout != 64), without and with the pool in its epilogue
    "fuse1": (C0 + conv("c1", "c0", 128), ["c0", "c1"], "c1"),
    "fuse1_pool": (C0 + conv("c1", "c0", 128) + pool("p", "c1"), ["c0", "c1"], "p"),
    # the family, split in: short K (8-row single tiles) and 256 -> 512 (16-row tiles by the cost model)
    "fam8": (C0 + conv("c1", "c0", 128) + conv("c2", "c1", 128), ["c0", "c1", "c2"], "c2"),
    "fam16": (C0 + conv("c1", "c0", 256) + conv("c2", "c1", 512), ["c0", "c1", "c2"], "c2"),
    # the pool in the family's epilogue: pool-only (CONV_NO_MAIN) ...
    "pool_only": (C0 + conv("c1", "c0", 128) + conv("c2", "c1", 128) + pool("p", "c2"), ["c0", "c1", "c2"], "p"),
    # ... and main + pool: c2 is read by its pool and by c3.  Every blob of a fast-forward graph must be consumed (a
    # dangling one is a net output and switches the fused path off), and the blobs of a per-blob tail share one size:
    # c3 is observed through a pool of its own (also fused: pool-only with split input).
    "main_pool": (C0 + conv("c1", "c0", 128) + conv("c2", "c1", 128) + pool("p", "c2") + conv("c3", "c2", 128) +
                  pool("p3", "c3"), ["c0", "c1", "c2", "c3"], ["p", "p3"]),
    # negative values through the split store (c2 without ReLU, CONV_MAIN_SPLIT) into a family conv
    "neg": (C0 + conv("c1", "c0", 128) + conv("c2", "c1", 128, relu=False) + conv("c3", "c2", 128), ["c0", "c1", "c2", "c3"], "c3"),
    # fp32 input inside the fused path: c1 is also read by a non-family conv (Cout 64), so it stays plain fp32
    "fp32in": (C0 + conv("c1", "c0", 128) + conv("c2", "c1", 128) + conv("c2b", "c1", 64) + conv("c3b", "c2b", 128),
               ["c0", "c1", "c2", "c2b", "c3b"], ["c2", "c3b"]),
    "k1": (C0 + conv("c1", "c0", 512) + conv("c2", "c1", 256, k=1), ["c0", "c1", "c2"], "c2"),
    "dil2": (C0 + conv("c1", "c0", 128) + conv("c2", "c1", 128, dil=2), ["c0", "c1", "c2"], "c2"),
    "dil4": (C0 + conv("c1", "c0", 128) + conv("c2", "c1", 128, dil=4), ["c0", "c1", "c2"], "c2"),
    "heads3": (C0 + conv("c1", "c0", 128) + conv("c2", "c1", 128) + conv("h1", "c2", 128, shared=True) +
               conv("h2", "c2", 128, dil=2, shared=True) + conv("h4", "c2", 128, dil=4, shared=True),
               ["c0", "c1", "c2", "h1"], ["h1", "h2", "h4"]),
}


def _probes(graph):
    pr = GRAPHS[graph][2]
    return [pr] if isinstance(pr, str) else list(pr)


def _setup(graph, h, w, scale, with_gpu):
    """The mini-detector with seeded weights, random biases on every conv of the stack (x scale), zero predictors."""
    layers, convs, probe = GRAPHS[graph]
    msg = P.parse(H.mini_detector(layers, probe, 2, 3, h, w))
    if with_gpu:
        gnet, onet = H.make_pair(msg, seed=5)
    else:
        gnet, onet = None, O.OracleNet(msg, params=O.synth_params(msg, seed=5))
    rng = np.random.default_rng(3)
    sc = np.float32(scale)
    for name in convs:
        onet.params[name][1][...] = rng.normal(0, 0.5, onet.params[name][1].shape).astype(np.float32) * sc
    for name, blobs in onet.params.items():
        if name.startswith("cls_score") or name.startswith("bbox_pred"):
            for b in blobs:
                b[...] = 0
    if with_gpu:
        H.load_params(gnet, onet.params)
    data = rng.normal(0, 1, (1, 3, h, w)).astype(np.float32) * sc
    return gnet, onet, data, np.array([[h, w, 1]], np.float32)


_ORACLE = {}


def _oracle(graph, h, w, mag):
    """(scale of input and biases, the oracle's probed blobs), once per graph / size / magnitude."""
    key = (graph, h, w, mag)
    if key in _ORACLE:
        return _ORACLE[key]
    stack = GRAPHS[graph][1]

    def run(scale):
        _, onet, data, info = _setup(graph, h, w, scale, False)
        onet.blobs['data'].reshape(*data.shape)
        onet.blobs['im_info'].reshape(1, 3)
        onet.forward(data=data, im_info=info)
        return onet
    scale = 1.0
    if mag == "small":
        scale = 2.0 ** -12
    elif mag == "top":
        # conv + bias + ReLU + max-pool are positively homogeneous in (input, biases): the stack's largest |activation| at
        # scale 1 gives the scale that puts it at 2^14 (tests/test_gpu_magnitudes.py test_conv_large_magnitudes)
        onet = run(1.0)
        scale = float(np.float32(2.0 ** 14 / max(float(np.abs(onet.blobs[n].data).max()) for n in stack)))
    onet = run(scale)
    top = max(float(np.abs(onet.blobs[n].data).max()) for n in stack)
    if mag == "top":
        assert 0.98 * 2 ** 14 < top < 1.02 * 2 ** 14
    if mag == "small":
        assert 0 < top < 64 * scale
    _ORACLE[key] = (scale, {n: onet.blobs[n].data[0].copy() for n in set(_probes(graph)) | set(stack)})
    return _ORACLE[key]


def _gpu_run(graph, h, w, scale):
    gnet, onet, data, info = _setup(graph, h, w, scale, True)
    gnet.set_conv_mode("f16x3")
    before = gnet.range_fallbacks
    gnet.prof_enable(True)
    gnet.prof_reset()
    fused = H.read_fused_blob(gnet, onet, data, info)
    prof = {k: int(v["launches"]) for k, v in gnet.prof_read().items()}
    gnet.prof_enable(False)
    fused = fused if isinstance(fused, list) else [fused]
    redo = gnet.range_fallbacks - before
    plain = [np.array(gnet.blobs[p].data[0]) for p in _probes(graph)]      # the per-layer kernels' recomputation
    return dict(fused=fused, plain=plain, prof=prof, range_fallbacks=redo, forwards=H.readout_forwards(onet))


def _child(graph, h, w, scale, out):
    """Entry of the knob children: the GPU side of one case -> out.npz / out.json."""
    r = _gpu_run(graph, int(h), int(w), float(scale))
    np.savez(out + ".npz", **{"fused%d" % i: a for i, a in enumerate(r["fused"])},
             **{"plain%d" % i: a for i, a in enumerate(r["plain"])})
    json.dump(dict(prof=r["prof"], range_fallbacks=r["range_fallbacks"], forwards=r["forwards"]), open(out + ".json", "w"))


def _gpu_run_in_child(graph, h, w, scale, env, tmp_path):
    out = str(tmp_path / "case")
    code = "from tests import test_gpu_fused_forms as M; M._child(%r, %d, %d, %r, %r)" % (graph, h, w, float(scale), out)
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, PYTHONPATH=ROOT, **env), cwd=ROOT,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (env, r.stderr[-2000:])
    z = np.load(out + ".npz")
    meta = json.load(open(out + ".json"))
    n = len(_probes(graph))
    return dict(fused=[z["fused%d" % i] for i in range(n)], plain=[z["plain%d" % i] for i in range(n)], **meta)


def _check(key, graph, h, w, mag, expect, absent, env=None, tmp_path=None):
    scale, want = _oracle(graph, h, w, mag)
    r = _gpu_run_in_child(graph, h, w, scale, env, tmp_path) if env else _gpu_run(graph, h, w, scale)
    errs, plain_errs = {}, {}
    for name, f, pl in zip(_probes(graph), r["fused"], r["plain"]):
        assert f.shape == pl.shape == want[name].shape, (name, f.shape, want[name].shape)
        errs[name] = H.rel_err(f, want[name])
        plain_errs[name] = H.rel_err(pl, want[name])
    fam = sum(r["prof"].get(W4(True, mt, nt), 0) for mt in (2, 4) for nt in (1, 2))
    launches = {k: (fam if k == W4_SPLIT_ANY else r["prof"].get(k, 0)) for k in list(expect) + list(absent)}
    _report(key, graph=graph, h=h, w=w, magnitude=mag or "O(1)", env=env or {}, fused_rel_err=errs, per_layer_rel_err=plain_errs,
            forwards=r["forwards"], launches=launches, range_fallbacks=r["range_fallbacks"])
    print(key, "fused", errs, "per-layer", plain_errs, launches)
    assert r["range_fallbacks"] == 0            # (a redo would have run the per-layer fp32 kernels)
    # the kernel class this case is about ran once per forward per layer that has it, what it replaces never
    for k, n in expect.items():
        assert launches[k] == n * r["forwards"], (k, launches[k], n, r["forwards"], {a: b for a, b in r["prof"].items() if b})
    for k in absent:
        assert launches[k] == 0, (k, launches[k])
    for name, e in errs.items():
        assert e < ACT_TOL, (name, e, "per-layer kernels on the same data: %g" % plain_errs[name])
    return want


# ------------------------------------------------------------------------------------------------------------
# forms selected by shape and graph, in this process
# ------------------------------------------------------------------------------------------------------------
FIRST_PAIR = ({PCP: 1, W4(True, 2, 1): 1}, [FIRST, POOLK, FUSE1, PC])
FAM8 = ({FUSE1: 1, W4(True, 2, 1): 1}, [FIRST, POOLK, W4(False, 2, 1)])
CASES = [
    # whole tiles only / ragged in both directions with odd height and width / more tiles than compute units
    ("first", 64, 64, None) + FIRST_PAIR, ("first", 37, 53, None) + FIRST_PAIR, ("first", 272, 270, None) + FIRST_PAIR,
    ("first", 37, 53, "small") + FIRST_PAIR, ("first", 37, 53, "top") + FIRST_PAIR,
    ("fuse1", 32, 32, None, {FUSE1: 1}, [FIRST, PCP, PC]), ("fuse1", 37, 53, None, {FUSE1: 1}, [FIRST, PCP, PC]),
    ("fuse1_pool", 32, 32, None, {FUSE1: 1}, [FIRST, POOLK]), ("fuse1_pool", 37, 53, None, {FUSE1: 1}, [FIRST, POOLK]),
    ("fam8", 32, 48, None) + FAM8, ("fam8", 37, 53, None) + FAM8, ("fam8", 5, 6, None) + FAM8,
    # 256 -> 512 on 256 compute units: 64 tiles x 4 cout tiles fill one round of single-tile blocks, 128 tiles one of dual
    ("fam16", 128, 128, None, {FUSE1: 1, W4(True, 4, 1): 1}, [FIRST, W4(True, 4, 2), W4(True, 2, 1), W4(True, 2, 2)]),
    ("fam16", 128, 256, None, {FUSE1: 1, W4(True, 4, 2): 1}, [FIRST, W4(True, 4, 1), W4(True, 2, 1), W4(True, 2, 2)]),
    ("fam16", 37, 53, "small", {FUSE1: 1, W4_SPLIT_ANY: 1}, [FIRST]), ("fam16", 37, 53, "top", {FUSE1: 1, W4_SPLIT_ANY: 1}, [FIRST]),
    ("pool_only", 32, 32, None) + FAM8, ("pool_only", 37, 53, None) + FAM8, ("pool_only", 5, 6, None) + FAM8,
    ("main_pool", 32, 32, None, {FUSE1: 1, W4(True, 2, 1): 2}, [FIRST, POOLK]),
    ("main_pool", 37, 53, None, {FUSE1: 1, W4(True, 2, 1): 2}, [FIRST, POOLK]),
    ("neg", 32, 32, None, {FUSE1: 1, W4(True, 2, 1): 2}, [FIRST]), ("neg", 37, 53, None, {FUSE1: 1, W4(True, 2, 1): 2}, [FIRST]),
    ("fp32in", 37, 53, None, {FUSE1: 1, W4(False, 2, 1): 1, W4(True, 2, 1): 1, W8_64: 1}, [FIRST]),
    ("k1", 32, 32, None, {FUSE1: 1, K1: 1}, [FIRST]), ("k1", 23, 29, None, {FUSE1: 1, K1: 1}, [FIRST]),
    ("dil2", 32, 32, None, {W4(True, 4, 1, 2): 1}, [FIRST]), ("dil2", 37, 53, None, {W4(True, 4, 1, 2): 1}, [FIRST]),
    ("dil2", 5, 6, None, {W4(True, 4, 1, 2): 1}, [FIRST]),
    ("dil4", 32, 32, None, {W4(True, 4, 1, 4): 1}, [FIRST]), ("dil4", 37, 53, None, {W4(True, 4, 1, 4): 1}, [FIRST]),
    ("dil4", 5, 6, None, {W4(True, 4, 1, 4): 1}, [FIRST]),
    ("heads3", 64, 48, None, {HEADS3: 1, W4(True, 2, 1): 1}, [FIRST, W4(True, 4, 1, 2), W4(True, 4, 1, 4)]),
    ("heads3", 37, 53, None, {HEADS3: 1, W4(True, 2, 1): 1}, [FIRST, W4(True, 4, 1, 2), W4(True, 4, 1, 4)]),
    ("heads3", 5, 6, None, {HEADS3: 1, W4(True, 2, 1): 1}, [FIRST, W4(True, 4, 1, 2), W4(True, 4, 1, 4)]),
]


@pytest.mark.parametrize("graph,h,w,mag,expect,absent", CASES, ids=["%s-%dx%d%s" % (c[0], c[1], c[2], "-" + c[3] if c[3] else "") for c in CASES])
def test_fused_form_vs_oracle(graph, h, w, mag, expect, absent):
    want = _check("%s_%dx%d_%s" % (graph, h, w, mag or "unit"), graph, h, w, mag, expect, absent)
    if graph == "neg":
        assert (want["c2"] < 0).any()             # negative values really went through the split store
    if graph in ("first", "fuse1_pool", "pool_only", "main_pool"):
        # (an odd map: the pooled map's last row / column is a clipped window, and it was compared like every other)
        assert want[_probes(graph)[0]].shape[1:] == ((h + 1) // 2, (w + 1) // 2)


# ------------------------------------------------------------------------------------------------------------
# forms selected by a knob: one child process each
# ------------------------------------------------------------------------------------------------------------
MT4, MT2 = {"SHF_F16X3_W4_MT": "4"}, {"SHF_F16X3_W4_MT": "2"}
NT1, NT2 = {"SHF_F16X3_W4D_NTILE": "1"}, {"SHF_F16X3_W4D_NTILE": "2"}
KNOB_CASES = [
    ("first", 37, 53, {"SHF_F16X3_PC_TAB": "0"}, {PCP: 1}, [FIRST, POOLK, PC]),
    ("first", 272, 270, {"SHF_F16X3_PC_TAB": "0"}, {PCP: 1}, [FIRST, POOLK, PC]),
    ("first", 37, 53, {"SHF_F16X3_PC_PERSIST": "0"}, {PC: 1}, [FIRST, POOLK, PCP]),
    ("first", 272, 270, {"SHF_F16X3_PC_PERSIST": "0"}, {PC: 1}, [FIRST, POOLK, PCP]),
    ("first", 37, 53, {"SHF_F16X3_PC": "0"}, {FUSE1: 1}, [FIRST, POOLK, PCP, PC]),
    ("fam16", 37, 53, dict(MT4, **NT1), {W4(True, 4, 1): 1}, [W4(True, 4, 2), W4(True, 2, 1), W4(True, 2, 2)]),
    ("fam16", 5, 6, dict(MT4, **NT1), {W4(True, 4, 1): 1}, [W4(True, 4, 2), W4(True, 2, 1), W4(True, 2, 2)]),
    ("fam16", 37, 53, dict(MT4, **NT2), {W4(True, 4, 2): 1}, [W4(True, 4, 1), W4(True, 2, 1), W4(True, 2, 2)]),
    ("fam16", 5, 6, dict(MT4, **NT2), {W4(True, 4, 2): 1}, [W4(True, 4, 1), W4(True, 2, 1), W4(True, 2, 2)]),
    ("fam16", 37, 53, dict(MT2, **NT2), {W4(True, 2, 2): 1}, [W4(True, 4, 1), W4(True, 2, 1), W4(True, 4, 2)]),
    ("fam16", 5, 6, dict(MT2, **NT2), {W4(True, 2, 2): 1}, [W4(True, 4, 1), W4(True, 2, 1), W4(True, 4, 2)]),
    ("pool_only", 37, 53, dict(MT4, **NT2), {W4(True, 4, 2): 1}, [POOLK, W4(True, 2, 1)]),
]


@pytest.mark.parametrize("graph,h,w,env,expect,absent", KNOB_CASES,
                         ids=["%s-%dx%d-%s" % (c[0], c[1], c[2], "-".join("%s=%s" % (k[10:], v) for k, v in sorted(c[3].items()))) for c in KNOB_CASES])
def test_knob_selected_fused_form_vs_oracle(graph, h, w, env, expect, absent, tmp_path):
    tag = "_".join("%s=%s" % kv for kv in sorted(env.items()))
    _check("%s_%dx%d_%s" % (graph, h, w, tag), graph, h, w, None, expect, absent, env=env, tmp_path=tmp_path)


# ------------------------------------------------------------------------------------------------------------
# fp32 mode: the fused pool of conv_mfma_f32_kernel runs behind detect_add_level only
# ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("graph", ["first", "pool_only"])
def test_fp32_mode_fused_pool_detect_rows_vs_oracle(graph):
    """fp32 mode never forwards on the fused path, but detect_add_level does (the pool in conv_mfma_f32_kernel's
    epilogue), and its logits cannot be read through blobs: the exported rows of a ragged odd unit, with ordinary random
    predictors, against the oracle net's proposals above the threshold -- every box matched, scores within 1e-4."""
    import torch
    from tests.test_gpu_fullsize import compare_detection_lists
    h, w, thresh = 37, 53, 0.05
    layers, convs, probe = GRAPHS[graph]
    gnet, onet = H.make_pair(P.parse(H.mini_detector(layers, probe, 2, 3, h, w)), seed=5, cls_bias=1.0)
    rng = np.random.default_rng(3)
    for name in convs:
        onet.params[name][1][...] = rng.normal(0, 0.5, onet.params[name][1].shape).astype(np.float32)
    H.load_params(gnet, onet.params)
    gnet.set_conv_mode("fp32")
    data = rng.normal(0, 1, (1, 3, h, w)).astype(np.float32)
    for b, shp in (("data", data.shape), ("im_info", (1, 3))):
        onet.blobs[b].reshape(*shp)
    oo = onet.forward(data=data, im_info=np.array([[h, w, 1]], np.float32))
    keep = oo["cls_prob"][:, 1] > thresh
    want = np.hstack([oo["boxes"][keep, 1:5], oo["cls_prob"][keep, 1:2]])
    gnet.prof_enable(True)
    gnet.prof_reset()
    gnet.detect_begin()
    gnet.detect_add_level(data, h, w, h, w, 1.0, False, thresh)
    buf = torch.empty((len(oo["boxes"]) + 64, 5), dtype=torch.float32, device="cuda")
    n = gnet.detect_export(buf.data_ptr(), buf.shape[0])
    got = buf[:n].cpu().numpy()
    prof = {k: int(v["launches"]) for k, v in gnet.prof_read().items()}
    gnet.prof_enable(False)
    assert len(want) > 8 and len(want) < len(oo["boxes"])        # the cut really cuts
    compare_detection_lists("fused_forms_fp32_" + graph, got, want)
    assert prof[POOLK] == 0, prof
    assert sum(v for k, v in prof.items() if k.startswith("conv_mfma_f32_kernel")) == len(convs) - 1    # (c0: conv_first_kernel)
    assert prof[FIRST] == 1


# ------------------------------------------------------------------------------------------------------------
# a grouped pass over units of different ragged sizes
# ------------------------------------------------------------------------------------------------------------
def test_grouped_pass_over_ragged_units_equals_one_at_a_time():
    """One grouped pass (one grid per conv layer over the units: member tile tables, per-member exponents and pool views)
    over three units of different ragged, odd sizes gives per unit the rows of one-at-a-time passes, bit for bit."""
    import torch
    from smallhardface_amd import test as T
    layers, convs, probe = GRAPHS["first"]
    gnet, onet = H.make_pair(P.parse(H.mini_detector(layers, probe, 2, 3, 37, 53)), seed=5, cls_bias=1.0)
    rng = np.random.default_rng(3)
    for name in convs:
        onet.params[name][1][...] = rng.normal(0, 0.5, onet.params[name][1].shape).astype(np.float32)
    H.load_params(gnet, onet.params)
    gnet.set_conv_mode("f16x3")
    units = []
    for k, (h, w) in enumerate([(37, 53), (21, 70), (51, 19)]):
        g = np.float32([1.0, 2.0 ** -6, 4.0][k])                 # units whose activation exponents differ
        units.append((rng.normal(0, 1, (1, 3, h, w)).astype(np.float32) * g, h, w, h, w, 1.0, False))
    fd = T.FusedDetector(gnet, n_lanes=3, mode="group")
    gnet.prof_enable(True)
    gnet.prof_reset()
    fd.lanes[0].detect_add_levels(fd.lanes[:3], units, 0.05, per_member_lists=True)
    fd.lanes[0].sync()
    prof = {k: int(v["launches"]) for k, v in gnet.prof_read().items()}
    gnet.prof_enable(False)
    assert prof[PCP] == 1 and prof[W4(True, 2, 1)] == 1 and prof[POOLK] == 0 and prof[FIRST] == 0, prof   # one grid per layer
    buf = torch.empty((40000, 5), dtype=torch.float32, device="cuda")
    rows = 0
    for m, u in enumerate(units):
        n = fd.lanes[m].detect_export(buf.data_ptr(), 40000)
        got = buf[:n].cpu().numpy()
        gnet.detect_begin()
        gnet.detect_add_level(*u, 0.05)
        n2 = gnet.detect_export(buf.data_ptr(), 40000)
        np.testing.assert_array_equal(got, buf[:n2].cpu().numpy())
        rows += n
    assert rows > 0 and gnet.range_fallbacks == 0

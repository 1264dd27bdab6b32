"""The bandwidth-bound layers of csrc/misc.hip against asymmetric references: the three fp32 depthwise-deconvolution kernels
(deconv_dw_kernel, deconv_dw_group_kernel<true> for kernel 4 / stride 2 / pad 1, deconv_dw_group_kernel<false>), what a
deconvolution leaves for a split-fp16 consumer (range flag, activation exponent), and maxpool_kernel beyond 2x2 stride 2.

Why these weights.  A Deconvolution layer of `synth_params` holds the bilinear filler: f(a) f(b) with f = [.25, .75, .75,
.25], the same 16 numbers in every channel, no bias, taps that sum to 1.  A transposed or mirrored tap index, a wrong
channel offset of the weight fetch and a dropped bias all compute the same thing on it, and its output never exceeds its
input.  Here every channel and every tap gets its own number (`_asym_weights`: no channel equals its transpose, either
flip or another channel) and the bias is non-zero.

How outputs are observed.  The graphs have no proposal tail, so forward() and forward_group() run the per-layer kernels
and every blob holds what those kernels wrote; the profiler says which kernel ran.  The layer under test reads an NHWC
activation `c0` (a 1x1 convolution), and the reference is computed from the GPU's own `c0`: only the layer under test is
judged.  `c0` reads the net input through the first-layer kernel, which takes channel counts that are multiples of 16
(`test_first_layer_refuses_other_channel_counts`); for the smaller counts of the cases a 16-channel 1x1 layer `pre` comes
first and `c0` runs on the generic direct kernel.

Bounds.  Integer data in [-8, 8]: every partial sum is far below 2^24, nothing rounds, the result is exact.  Random data:
the kernels do T <= ceil(k / stride)^2 fused multiply-adds and one bias add in fp32, T + 1 roundings, so against float64

    |got - ref| <= (T + 2) 2^-24 (sum |x w| + |bias|)

for every element -- derived, not measured; a wrong tap, channel or bias is O(1) against it.  Max-pooling is pure selection:
exact.  The convolution that consumes a deconvolution or a pool in split-fp16 mode is held to the project's 2e-5 bar
(ACT_TOL of tests/test_gpu_parity.py) against the oracle.
"""
import numpy as np
import pytest

from oracle import oracle as O
from smallhardface_amd import prototxt as P
from tests import helpers as H

gpu = pytest.mark.gpu

ACT_TOL = 2e-5          # tests/test_gpu_parity.py
U32 = 2.0 ** -24        # unit roundoff of fp32
MODES = ["fp32", "f16x3"]

# (C, h, w, k, stride, pad)
DECONV_CASES = [
    (8, 3, 5, 4, 2, 1),       # the detector's geometry at a minimal size
    (64, 5, 7, 4, 2, 1),      # 16 channel quads: a wave spans four pixels of both parities, the four tap variants diverge inside it
    (256, 3, 4, 4, 2, 1),     # the wave-uniform case, as in the detector
    (4, 1, 1, 4, 2, 1),       # one input pixel: every output has exactly one tap
    (12, 4, 3, 2, 2, 0),      # non-overlapping taps
    (8, 5, 4, 3, 1, 1),       # stride 1, same size out
    (8, 3, 3, 5, 3, 2),       # stride 3: outputs with 1, 2 and 4 taps
    (4, 2, 3, 6, 4, 1),       # stride 4
    (64, 11, 67, 4, 2, 1),    # more than one block along x (134 x 16 quads > 256 threads) and 22 rows
    (64, 9, 33, 5, 3, 2),     # the same for the generic geometry
]
GROUP_GEOMETRIES = [(4, 2, 1), (2, 2, 0), (3, 1, 1), (5, 3, 2)]     # the first reaches <true>, the others <false>
GROUP_SIZES = {2: [(3, 5), (9, 4)], 3: [(3, 5), (5, 3), (9, 4)], 16: [(3, 5), (5, 3), (9, 4), (4, 7)] * 4}

# (C, h, w, k, stride, pad)
POOL_CASES = [
    (64, 7, 9, 3, 2, 0),      # ceil sizing, clipped last windows
    (64, 6, 8, 3, 2, 1),      # pad, k = 3
    (64, 3, 5, 2, 2, 1),      # the last window would start in the padding: one output less than the ceil formula
    (64, 5, 5, 3, 1, 1),      # stride 1 with pad
    (64, 7, 10, 3, 3, 0),     # stride = k with remainders
    (12, 1, 1, 2, 2, 0),      # one pixel, 3 channel quads
    (64, 4, 4, 4, 4, 0),      # one window = whole map
    (64, 37, 29, 3, 2, 1),    # 19 x 15 x 16 quads: eighteen blocks
]


# ---- graphs ---------------------------------------------------------------------------------------------------------------
def _conv(name, bottom, nout, k, pad, relu=False):
    s = ('layer { name: "%s" type: "Convolution" bottom: "%s" top: "%s" convolution_param { num_output: %d '
         'kernel_size: %d pad: %d } }\n' % (name, bottom, name, nout, k, pad))
    if relu:
        s += 'layer { name: "%s_relu" type: "ReLU" bottom: "%s" top: "%s" }\n' % (name, name, name)
    return s


def _deconv(C, k, stride, pad, bias=True):
    return ('layer { name: "up" type: "Deconvolution" bottom: "c0" top: "up" convolution_param { kernel_size: %d stride: %d '
            'num_output: %d group: %d pad: %d%s } }\n' % (k, stride, C, C, pad, "" if bias else " bias_term: false"))


def _pool(bottom, k, stride, pad):
    return ('layer { name: "p" type: "Pooling" bottom: "%s" top: "p" pooling_param { pool: MAX kernel_size: %d stride: %d '
            'pad: %d } }\n' % (bottom, k, stride, pad))


def _front(C, k=1):
    """(layers that end in the C-channel NHWC activation `c0`, channels of the net input).  k = 1: 1x1 layers on a C- (or
    16-) channel input; k = 3: 3x3 on a 3-channel input."""
    cin = 3 if k == 3 else (C if C % 16 == 0 else 16)
    if C % 16 == 0:
        return _conv("c0", "data", C, k, k // 2), cin
    return _conv("pre", "data", 16, k, k // 2) + _conv("c0", "pre", C, 1, 0), cin


def _identity_front(C):
    """Parameters of `_front(C)` under which c0[c] = data[c], exactly."""
    if C % 16 == 0:
        return {"c0": [np.eye(C, dtype=np.float32).reshape(C, C, 1, 1), np.zeros(C, np.float32)]}
    return {"pre": [np.eye(16, dtype=np.float32).reshape(16, 16, 1, 1), np.zeros(16, np.float32)],
            "c0": [np.eye(C, 16, dtype=np.float32).reshape(C, 16, 1, 1), np.zeros(C, np.float32)]}


def _random_front(rng, C, k=1):
    cin = 3 if k == 3 else (C if C % 16 == 0 else 16)
    out = {}
    for name, co, ci, kk in ([("c0", C, cin, k)] if C % 16 == 0 else [("pre", 16, cin, k), ("c0", C, 16, 1)]):
        out[name] = [rng.normal(0, 1.0 / np.sqrt(ci * kk * kk), (co, ci, kk, kk)).astype(np.float32),
                     rng.normal(0, 0.5, (co,)).astype(np.float32)]
    return out


def _net(txt):
    from smallhardface_amd import caffe
    return caffe.Net(None, prototxt_text=txt)


def _stage(net, data):
    net.blobs["data"].reshape(*data.shape)
    net.blobs["im_info"].reshape(1, 3)
    return {"data": data, "im_info": np.array([[data.shape[2], data.shape[3], 1]], np.float32)}


def _forward(net, data):
    return net.forward(**_stage(net, data))


def _profiled(head, fn):
    """(fn(), {kernel class: launches}) with the head's profiler on."""
    head.prof_enable(True)
    head.prof_reset()
    try:
        out = fn()
        prof = {k: int(v["launches"]) for k, v in head.prof_read().items()}
    finally:
        head.prof_enable(False)
        head.prof_reset()
    return out, prof


def _blob(net, name):
    return np.array(net.blobs[name].data)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ---- references -------------------------------------------------------------------------------------------------------------
def _symmetric(w2):
    return np.array_equal(w2, w2.T) or np.array_equal(w2, w2[::-1]) or np.array_equal(w2, w2[:, ::-1])


def _asym_weights(rng, C, k, integer):
    """(C, 1, k, k) depthwise weights, every channel and tap drawn on its own (integers in [-8, 8] or normal(0, 0.5)); a
    channel that came out equal to its transpose, to one of its flips or to an earlier channel is drawn again."""
    draw = (lambda: rng.integers(-8, 9, (k, k))) if integer else (lambda: rng.normal(0, 0.5, (k, k)))
    w = np.zeros((C, 1, k, k), np.float32)
    for c in range(C):
        while True:
            w[c, 0] = draw()
            if not _symmetric(w[c, 0]) and not any(np.array_equal(w[c, 0], w[j, 0]) for j in range(c)):
                break
    return w


def _assert_asymmetric(w):
    """The tensor differs from its transpose and from both axis flips -- in every channel -- and no two channels are equal."""
    assert not np.array_equal(w, w.transpose(0, 1, 3, 2))
    assert not np.array_equal(w, w[:, :, ::-1]) and not np.array_equal(w, w[:, :, :, ::-1])
    for c in range(w.shape[0]):
        assert not _symmetric(w[c, 0]), c
    assert len(np.unique(w.reshape(w.shape[0], -1), axis=0)) == w.shape[0]


def _deconv_shape(h, w, k, stride, pad):
    return stride * (h - 1) + k - 2 * pad, stride * (w - 1) + k - 2 * pad


def _deconv_ref(x, wt, bs, k, stride, pad, dtype):
    """Depthwise col2im in `dtype` (int64 or float64): out[c, s iy - pad + a, s ix - pad + b] += x[c, iy, ix] w[c, 0, a, b]
    on a canvas that keeps the padding, cropped afterwards; + bias.  x (C, h, w), wt (C, 1, k, k), bs (C,) or None.
    Returns (out, sum |x w|), both (C, Ho, Wo)."""
    C, h, w = x.shape
    Ho, Wo = _deconv_shape(h, w, k, stride, pad)
    ref = np.zeros((C, stride * (h - 1) + k, stride * (w - 1) + k), dtype)
    mag = np.zeros_like(ref)
    xx = x.astype(dtype)
    for a in range(k):
        for b in range(k):
            t = xx * wt[:, 0, a, b].astype(dtype)[:, None, None]
            ref[:, a:a + stride * (h - 1) + 1:stride, b:b + stride * (w - 1) + 1:stride] += t
            mag[:, a:a + stride * (h - 1) + 1:stride, b:b + stride * (w - 1) + 1:stride] += np.abs(t)
    ref = ref[:, pad:pad + Ho, pad:pad + Wo]
    mag = mag[:, pad:pad + Ho, pad:pad + Wo]
    if bs is not None:
        ref = ref + bs.astype(dtype)[:, None, None]
    return ref, mag


def _taps(k, stride):
    return (-(-k // stride)) ** 2


def _assert_within_fp32_bound(got, ref, mag, bs, T, what):
    """|got - ref| <= (T + 2) 2^-24 (sum |x w| + |bias|) for every element; the worst ratio is printed before the assertion."""
    absb = 0.0 if bs is None else np.abs(bs.astype(np.float64))[:, None, None]
    bound = (T + 2) * U32 * (mag + absb)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    err = np.abs(got.astype(np.float64) - ref)
    ratio = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))
    print("%s: T %d, %d elements, worst |err| / bound %.3f (max err %.3e)" % (what, T, err.size, float(ratio.max()), float(err.max())))
    assert np.isfinite(got).all(), what
    assert (err <= bound).all(), (what, float(ratio.max()))


def _check_up(c0, up, wt, bs, k, stride, pad, integer, what):
    """`up` (C, Ho, Wo) against the reference formed from the GPU's own `c0`."""
    if integer:
        np.testing.assert_array_equal(c0, np.rint(c0))
        ref, mag = _deconv_ref(c0, wt, bs, k, stride, pad, np.int64)
        assert int(mag.max()) + 8 < 2 ** 24 and (ref < 0).any() and (ref > 0).any()
        assert up.shape == ref.shape, (what, up.shape, ref.shape)
        np.testing.assert_array_equal(up, ref.astype(np.float32), err_msg=what)
    else:
        ref, mag = _deconv_ref(c0, wt, bs, k, stride, pad, np.float64)
        _assert_within_fp32_bound(up, ref, mag, bs, _taps(k, stride), what)


def _up_problem(seed, C, k, integer, bias=True):
    """(front parameters, deconvolution weights, bias or None, a function (h, w, seed) -> net input)."""
    rng = np.random.default_rng(seed)
    front = _identity_front(C) if integer else _random_front(rng, C)
    wt = _asym_weights(rng, C, k, integer)
    _assert_asymmetric(wt)
    if not bias:
        bs = None
    elif integer:
        bs = rng.integers(-8, 9, (C,)).astype(np.float32)
        bs[bs == 0] = 3
    else:
        bs = rng.normal(0, 1, (C,)).astype(np.float32)
    cin = C if C % 16 == 0 else 16

    def data(h, w, s):
        r = np.random.default_rng(1000 * seed + s)
        x = r.integers(-8, 9, (1, cin, h, w)) if integer else r.normal(0, 1, (1, cin, h, w))
        return x.astype(np.float32)
    return front, wt, bs, data


def _up_params(front, wt, bs):
    return dict(front, up=[wt] + ([bs] if bs is not None else []))


# ---- 6. CPU checks of the references above ----------------------------------------------------------------------------------
@pytest.mark.parametrize("C,h,w,k,stride,pad", DECONV_CASES)
def test_col2im_reference_agrees_with_the_oracle(C, h, w, k, stride, pad):
    for integer in (True, False):
        rng = np.random.default_rng(C + 10 * k + stride)
        wt = _asym_weights(rng, C, k, integer)
        bs = (rng.integers(-8, 9, (C,)) if integer else rng.normal(0, 1, (C,))).astype(np.float32)
        x = (rng.integers(-8, 9, (1, C, h, w)) if integer else rng.normal(0, 1, (1, C, h, w))).astype(np.float32)
        got = O.deconvolution(x, wt, bs, pad, stride, C)[0]
        assert got.shape == (C,) + _deconv_shape(h, w, k, stride, pad)
        if integer:
            ref, _ = _deconv_ref(x[0], wt, bs, k, stride, pad, np.int64)
            np.testing.assert_array_equal(got, ref.astype(np.float32))
        else:
            # (the oracle rounds each product and each of the T - 1 additions of a tap sum, then the bias add: T + 1 roundings)
            ref, mag = _deconv_ref(x[0], wt, bs, k, stride, pad, np.float64)
            _assert_within_fp32_bound(got, ref, mag, bs, _taps(k, stride), "oracle k%d s%d p%d" % (k, stride, pad))
    # without a bias, and the tap count the bound uses: no output collects more than T products
    ref, mag = _deconv_ref(np.ones((1, h, w)), np.ones((1, 1, k, k)), None, k, stride, pad, np.int64)
    np.testing.assert_array_equal(ref, mag)
    assert 1 <= ref.min() and ref.max() <= _taps(k, stride)
    np.testing.assert_array_equal(O.deconvolution(np.ones((1, 1, h, w), np.float32), np.ones((1, 1, k, k), np.float32), None, pad,
                                                  stride, 1)[0], ref.astype(np.float32))


@pytest.mark.parametrize("k", [2, 3, 4, 5, 6])
@pytest.mark.parametrize("integer", [True, False])
def test_weight_generator_is_asymmetric(k, integer):
    w = _asym_weights(np.random.default_rng(k), 256 if k > 2 else 64, k, integer)
    _assert_asymmetric(w)
    if integer:
        assert np.array_equal(w, np.rint(w)) and np.abs(w).max() == 8
    # ... and the check refuses what the bilinear filler gives
    with pytest.raises(AssertionError):
        _assert_asymmetric(O.bilinear_filler((4, 1, 4, 4)))
    sym = w.copy()
    sym[3, 0] = sym[3, 0] + sym[3, 0].T
    with pytest.raises(AssertionError):
        _assert_asymmetric(sym)
    dup = w.copy()
    dup[5] = dup[2]
    with pytest.raises(AssertionError):
        _assert_asymmetric(dup)


def test_bound_rejects_wrong_taps_channels_and_bias():
    """The mistakes the GPU tests are after, made in the reference itself: each leaves the bound by orders of magnitude."""
    C, h, w, k, stride, pad = 8, 3, 5, 4, 2, 1
    rng = np.random.default_rng(3)
    wt = _asym_weights(rng, C, k, False)
    bs = rng.normal(0, 1, (C,)).astype(np.float32)
    x = rng.normal(0, 1, (C, h, w)).astype(np.float32)
    ref, mag = _deconv_ref(x, wt, bs, k, stride, pad, np.float64)
    _assert_within_fp32_bound(ref.astype(np.float32), ref, mag, bs, 4, "itself")
    wrong = [wt.transpose(0, 1, 3, 2), wt[:, :, ::-1], wt[:, :, :, ::-1], np.roll(wt, 1, axis=0)]
    for bad_w, bad_b in [(v, bs) for v in wrong] + [(wt, None), (wt, np.roll(bs, 1))]:
        bad, _ = _deconv_ref(x, bad_w, bad_b, k, stride, pad, np.float64)
        with pytest.raises(AssertionError):
            _assert_within_fp32_bound(bad.astype(np.float32), ref, mag, bs, 4, "wrong")


def test_pool_cases_have_the_sizes_they_are_there_for():
    for C, h, w, k, stride, pad in POOL_CASES:
        y = O.max_pool(np.zeros((1, 4, h, w), np.float32), k, stride, pad)
        ceil = lambda n: -(-(n + 2 * pad - k) // stride) + 1
        if (C, h, w, k, stride, pad) == (64, 3, 5, 2, 2, 1):
            assert y.shape[2:] == (ceil(h) - 1, ceil(w) - 1) == (2, 3)    # the plain ceil formula gives one more row and column
        else:
            assert y.shape[2:] == (ceil(h), ceil(w))
    assert O.max_pool(np.zeros((1, 4, 7, 9), np.float32), 3, 2, 0).shape[2:] == (3, 4)     # (floor sizing would give 3 x 4 too ...
    assert O.max_pool(np.zeros((1, 4, 7, 10), np.float32), 3, 3, 0).shape[2:] == (3, 4)    # ... here it gives 2 x 3)


# ---- the graph of section 4 and its scaling recipes ---------------------------------------------------------------------------
EXP_HW = (9, 13)


def _exp_txt(h, w):
    return H.single_layer_net(_conv("c0", "data", 128, 3, 1, True) + _deconv(128, 4, 2, 1) + _conv("c2", "up", 256, 3, 1, True), 3, h, w)


def _oracle_forward(onet, data):
    onet.blobs["data"].reshape(*data.shape)
    onet.blobs["im_info"].reshape(1, 3)
    onet.forward(data=data, im_info=np.array([[data.shape[2], data.shape[3], 1]], np.float32))
    return {n: float(np.abs(b.data).max()) for n, b in onet.blobs.items() if n not in ("data", "im_info")}


def _exp_base(h=EXP_HW[0], w=EXP_HW[1], seed=21):
    """(net message, parameters, input): c0 is O(1), `up` has asymmetric random weights and a bias, so does c2."""
    msg = P.parse(_exp_txt(h, w))
    params = O.synth_params(msg, seed=seed)
    rng = np.random.default_rng(seed)
    params["c0"][1][...] = rng.normal(0, 0.02, 128)       # (small: a group member's magnitude follows its input)
    params["up"][0][...] = _asym_weights(rng, 128, 4, False)
    params["up"][1][...] = rng.normal(0, 0.1, 128)
    params["c2"][0][...] *= np.float32(0.25)       # (keeps c2's own outputs below `up`'s: only `up` decides the range flag)
    params["c2"][1][...] = rng.normal(0, 0.5, 256)
    return msg, params, H.synth_image_blob(h, w, seed=seed)


def _scale_up(params, s):
    """The deconvolution is linear in (weights, bias): `up` scales by s.  c2's bias follows its input's magnitude."""
    out = {n: [a.copy() for a in blobs] for n, blobs in params.items()}
    s = np.float32(s)
    out["up"][0] *= s
    out["up"][1] *= s
    out["c2"][1] *= s
    return out


def _exp_recipe(kind, data_scales=(1.0,)):
    """(message, parameters, one input per entry of `data_scales`, the oracle's maxima per input).

    "flag": the input lifts max |c0| to about 4096 (c0's bias stays), then `up` is scaled to max |up| = 2 x 65504 on the FIRST input;
    "low": `up` x 2^-12; "high": `up` x the power of two that puts max |up| into [2^13.5, 2^14.5)."""
    msg, params, data = _exp_base()
    onet = O.OracleNet(msg, params=params)
    m = _oracle_forward(onet, data)
    if kind == "flag":
        data = data * np.float32(4096.0 / m["c0"])
        m = _oracle_forward(onet, data)
        params = _scale_up(params, 2 * 65504.0 / m["up"])
    elif kind == "low":
        params = _scale_up(params, 2.0 ** -12)
    elif kind == "high":
        params = _scale_up(params, 2.0 ** int(np.round(14 - np.log2(m["up"]))))
    else:
        assert kind == "base"
    onet = O.OracleNet(msg, params=params)
    datas = [data * np.float32(s) for s in data_scales]
    return msg, params, datas, [_oracle_forward(onet, d) for d in datas]


def _assert_recipe(kind, m, member=0):
    """The oracle's maxima are where the test of `kind` needs them (member 1 of a group: the off-magnitude one)."""
    if kind == "flag":
        if member == 0:
            assert 2048 < m["c0"] < 8192 and 1.99 * 65504 < m["up"] < 2.01 * 65504 and m["c2"] < 65504
        else:          # the member that must NOT overflow: 1/64 of the input
            assert m["c0"] < 256 and m["up"] < 65504 / 8 and m["c2"] < 65504 / 8
    elif kind == "low":
        s = 1.0 if member == 0 else 0.25
        assert 0.5 * s < m["c0"] < 32 * s                                   # c0 is O(1) ...
        assert 2.0 ** -12 * 0.5 * s < m["up"] < 2.0 ** -12 * 64 * s         # ... `up` sits at 2^-12
    elif kind == "high":
        s = 1.0 if member == 0 else 1.0 / 16
        assert 0.5 * s < m["c0"] < 32 * s
        if member == 0:
            assert 2.0 ** 13 < m["up"] < 2.0 ** 15
        else:
            assert 2.0 ** 9 < m["up"] < 2.0 ** 12
        assert m["c2"] < 65504 / 2          # no fallback is due
        # an exponent taken from c0's maximum would lift `up` out of fp16 (conv_act_exponent: c0's max to [2^13, 2^14))
        assert m["up"] / m["c0"] * 2.0 ** 13 > 65504
    else:
        assert 0.5 < m["c0"] < 32 and m["up"] < 1024 and m["c2"] < 1024


EXP_GROUP_SCALES = {"flag": (1.0, 1.0 / 64), "low": (1.0, 0.25), "high": (1.0, 1.0 / 16)}


@pytest.mark.parametrize("kind", ["base", "flag", "low", "high"])
def test_scaling_recipes_put_the_maxima_where_the_tests_say(kind):
    msg, params, datas, maxima = _exp_recipe(kind, EXP_GROUP_SCALES.get(kind, (1.0,)))
    _assert_asymmetric(params["up"][0])
    for member, m in enumerate(maxima):
        print(kind, member, m)
        _assert_recipe(kind, m, member)


# ---- 1. + 2. the single-unit kernel -----------------------------------------------------------------------------------------
@gpu
def test_first_layer_refuses_other_channel_counts():
    """Why the small cases have the layer `pre`: a convolution on the net input with 8 output channels is refused by name."""
    from smallhardface_amd import _lib
    net = _net(H.single_layer_net(_conv("c0", "data", 8, 1, 0), 8, 3, 5))
    with pytest.raises(_lib.ShfError, match="conv_first: Cout must be a multiple of 16"):
        _forward(net, np.zeros((1, 8, 3, 5), np.float32))


def _run_single_deconv(C, h, w, k, stride, pad, integer, bias=True):
    txt, cin = _front(C)
    net = _net(H.single_layer_net(txt + _deconv(C, k, stride, pad, bias), cin, h, w))
    front, wt, bs, data = _up_problem(C + h + 10 * k, C, k, integer, bias)
    assert len(net.params["up"]) == (2 if bias else 1)
    H.load_params(net, _up_params(front, wt, bs))
    x = data(h, w, 0)
    for mode in MODES:
        net.set_conv_mode(mode)
        falls = net.range_fallbacks
        out, prof = _profiled(net, lambda: _forward(net, x))
        assert prof["deconv_depthwise"] == 1 and net.range_fallbacks == falls
        c0 = _blob(net, "c0")[0]
        if integer:
            np.testing.assert_array_equal(c0, x[0, :C])
        assert out["up"].shape == (1, C) + _deconv_shape(h, w, k, stride, pad)
        _check_up(c0, np.array(out["up"][0]), wt, bs, k, stride, pad, integer,
                  "%s C%d %dx%d k%d s%d p%d" % (mode, C, h, w, k, stride, pad))


@gpu
@pytest.mark.parametrize("C,h,w,k,stride,pad", DECONV_CASES)
def test_deconvolution_integer_data_is_exact(C, h, w, k, stride, pad):
    _run_single_deconv(C, h, w, k, stride, pad, True)


@gpu
@pytest.mark.parametrize("C,h,w,k,stride,pad", DECONV_CASES)
def test_deconvolution_random_data_per_element_bound(C, h, w, k, stride, pad):
    _run_single_deconv(C, h, w, k, stride, pad, False)


@gpu
@pytest.mark.parametrize("integer", [True, False])
def test_deconvolution_without_bias(integer):
    _run_single_deconv(8, 3, 5, 4, 2, 1, integer, bias=False)


# ---- 3. the grouped kernels ---------------------------------------------------------------------------------------------------
def _run_grouped_deconv(k, stride, pad, C, n, bias=True):
    sizes = GROUP_SIZES[n]
    shapes = [_deconv_shape(h, w, k, stride, pad) for h, w in sizes]
    assert any(ho % 8 for ho, _ in shapes)                       # a block's 8 rows end inside some member
    assert len(set(wo for _, wo in shapes)) > 1                  # the widest member sets the grid, the others are masked
    txt, cin = _front(C)
    txt = H.single_layer_net(txt + _deconv(C, k, stride, pad, bias), cin, *sizes[0])
    root, solo = _net(txt), _net(txt)
    lanes = [root] + [root.clone() for _ in range(n - 1)]
    for integer in (True, False):
        front, wt, bs, data = _up_problem(7 * k + C + n, C, k, integer, bias)
        for net in (root, solo):                                   # (the lanes hold the root's parameter tensors)
            H.load_params(net, _up_params(front, wt, bs))
        xs = [data(h, w, j) for j, (h, w) in enumerate(sizes)]
        for mode in MODES:
            root.set_conv_mode(mode)
            solo.set_conv_mode(mode)
            falls = root.range_fallbacks
            outs, prof = _profiled(root, lambda: root.forward_group(lanes, [_stage(m, x) for m, x in zip(lanes, xs)]))
            assert prof["deconv_depthwise"] == 1, "the group's deconvolutions are one launch"
            assert root.range_fallbacks == falls and len(outs) == n
            for j, (m, x, out) in enumerate(zip(lanes, xs, outs)):
                what = "%s n%d member %d C%d %dx%d k%d s%d p%d" % ((mode, n, j, C) + sizes[j] + (k, stride, pad))
                assert out["up"].shape == (1, C) + shapes[j], what
                up = np.array(out["up"][0])
                np.testing.assert_array_equal(up, _blob(m, "up")[0])
                _check_up(_blob(m, "c0")[0], up, wt, bs, k, stride, pad, integer, what)
                # bit for bit what its own forward() gives (Net.forward_group's promise), from the single-unit kernel
                want, sprof = _profiled(solo, lambda: _forward(solo, x))
                assert sprof["deconv_depthwise"] == 1
                np.testing.assert_array_equal(_bits(_blob(m, "c0")), _bits(_blob(solo, "c0")))
                np.testing.assert_array_equal(_bits(up), _bits(want["up"][0]), err_msg=what)


@gpu
@pytest.mark.parametrize("n", [2, 3, 16])
@pytest.mark.parametrize("C", [8, 64])
@pytest.mark.parametrize("k,stride,pad", GROUP_GEOMETRIES)
def test_grouped_deconvolution(k, stride, pad, C, n):
    _run_grouped_deconv(k, stride, pad, C, n)


@gpu
@pytest.mark.parametrize("k,stride,pad", [(4, 2, 1), (3, 1, 1)])
def test_grouped_deconvolution_without_bias(k, stride, pad):
    _run_grouped_deconv(k, stride, pad, 8, 3, bias=False)


# ---- 4. range flag and activation exponent after a deconvolution -----------------------------------------------------------------
def _exp_nets(msg, params, n=1):
    from smallhardface_amd import caffe
    root = caffe.Net(None, prototxt_text=P.dumps(msg))
    H.load_params(root, params)
    root.set_conv_mode("f16x3")
    return [root] + [root.clone() for _ in range(n - 1)], O.OracleNet(msg, params=params)


def _assert_c2_at_the_bar(net, onet, data, what):
    _oracle_forward(onet, data)
    for name in ("c0", "up", "c2"):
        a, b = _blob(net, name), onet.blobs[name].data
        assert a.shape == b.shape, (what, name)
        assert np.isfinite(a).all(), (what, name)
        err = H.rel_err(a, b)
        print("%s: %s rel err %.3e" % (what, name, err))
        assert err < ACT_TOL, (what, name, err)


@gpu
@pytest.mark.parametrize("n", [1, 2])
def test_range_flag_after_a_deconvolution(n):
    """max |up| = 2 x 65504 under a c0 that stays at 4096: only the deconvolution can raise the flag in time -- c2, which
    splits `up` to fp16, would read inf.  n = 2: only the SECOND member overflows and the whole group is redone."""
    scales = EXP_GROUP_SCALES["flag"] if n == 2 else (1.0,)
    msg, params, datas, maxima = _exp_recipe("flag", scales)
    for member, m in enumerate(maxima):
        _assert_recipe("flag", m, member)
    assert maxima[0]["up"] > 65504 > maxima[0]["c0"]
    lanes, onet = _exp_nets(msg, params, n)
    root = lanes[0]
    order = list(range(n))[::-1]                     # the overflowing unit goes last
    before = root.range_fallbacks
    if n == 1:
        _, prof = _profiled(root, lambda: _forward(root, datas[0]))
    else:
        _, prof = _profiled(root, lambda: root.forward_group(lanes, [_stage(m, datas[j]) for m, j in zip(lanes, order)]))
    assert root.range_fallbacks == before + 1
    assert prof["deconv_depthwise"] == 2             # the split-fp16 pass and its fp32 redo, one launch each
    for m, j in zip(lanes, order):
        _assert_c2_at_the_bar(m, onet, datas[j], "flag n%d unit %d" % (n, j))
    # the next forward, unscaled, is clean again
    bmsg, bparams, bdatas, bmax = _exp_recipe("base")
    _assert_recipe("base", bmax[0])
    H.load_params(root, bparams)
    before = root.range_fallbacks
    if n == 1:
        _forward(root, bdatas[0])
    else:
        root.forward_group(lanes, [_stage(m, bdatas[0]) for m in lanes])
    assert root.range_fallbacks == before
    bonet = O.OracleNet(bmsg, params=bparams)
    for m in lanes:
        _assert_c2_at_the_bar(m, bonet, bdatas[0], "after the flag, n%d" % n)


@gpu
@pytest.mark.parametrize("n", [1, 2, 3])
@pytest.mark.parametrize("C,k,stride,pad", [(64, 4, 2, 1), (64, 3, 1, 1)])
def test_deconvolution_output_alone_raises_the_range_flag(C, k, stride, pad, n):
    """c0 -> up with nothing behind it: no convolution can raise the flag in the deconvolution's place.  One element of the
    last member's `up` beyond 65504 (c0 itself stays below 16) costs one fp32 redo, in the single-unit kernel (n = 1) and in
    both grouped ones; `up` is within the bound either way, and an input that stays in range costs none."""
    sizes = [(3, 5), (5, 3), (9, 4)][:n]
    txt, cin = _front(C)
    root = _net(H.single_layer_net(txt + _deconv(C, k, stride, pad), cin, *sizes[0]))
    lanes = [root] + [root.clone() for _ in range(n - 1)]
    front, wt, bs, data = _up_problem(5, C, k, True)
    big = wt.copy()
    big[C - 1, 0, 1, 2] = 65536.0 / 4            # x an input of +-8 at most: 131072 where |data| > 4, exact in fp32
    H.load_params(root, _up_params(front, big, bs))
    root.set_conv_mode("f16x3")
    xs = [data(h, w, j) for j, (h, w) in enumerate(sizes)]
    xs[-1][0, C - 1, 0, 0] = 8.0
    for j in range(n - 1):
        xs[j][0, C - 1] = np.clip(xs[j][0, C - 1], -1, 1)        # the other members stay far below the range
    for overflow in (True, False, True):
        if not overflow:
            xs_ = [x.copy() for x in xs]
            xs_[-1][0, C - 1] = np.clip(xs_[-1][0, C - 1], -1, 1)
        else:
            xs_ = xs
        before = root.range_fallbacks
        outs, prof = _profiled(root, lambda: root.forward_group(lanes, [_stage(m, x) for m, x in zip(lanes, xs_)]) if n > 1
                               else [_forward(root, xs_[0])])
        tops = [float(np.abs(o["up"]).max()) for o in outs]
        assert all(t < 65504 / 2 for t in tops[:-1]) and (tops[-1] > 65504) == overflow, tops
        assert root.range_fallbacks == before + (1 if overflow else 0), (overflow, tops)
        assert prof["deconv_depthwise"] == (2 if overflow else 1)
        for m, out in zip(lanes, outs):
            ref, _ = _deconv_ref(_blob(m, "c0")[0], big, bs, k, stride, pad, np.int64)
            np.testing.assert_array_equal(out["up"][0], ref.astype(np.float32))


@gpu
@pytest.mark.parametrize("n", [1, 2])
@pytest.mark.parametrize("kind", ["low", "high"])
def test_activation_exponent_after_a_deconvolution(kind, n):
    """c2 belongs to the single-accumulator family, which lifts its input by the exponent its producer published.  "low":
    `up` at 2^-12 under an O(1) c0 -- without a published maximum c2's low parts are fp16 subnormals (6.8e-5 per layer,
    tests/test_gpu_magnitudes.py).  "high": max |up| about 2^14 -- c0's exponent would lift it beyond 65504.  n = 2: two
    members at different magnitudes, each with its own slot, the larger one first ("low") or last ("high")."""
    scales = EXP_GROUP_SCALES[kind] if n == 2 else (1.0,)
    msg, params, datas, maxima = _exp_recipe(kind, scales)
    for member, m in enumerate(maxima):
        _assert_recipe(kind, m, member)
    lanes, onet = _exp_nets(msg, params, n)
    root = lanes[0]
    order = list(range(n)) if kind == "low" else list(range(n))[::-1]
    before = root.range_fallbacks
    if n == 1:
        _, prof = _profiled(root, lambda: _forward(root, datas[0]))
    else:
        _, prof = _profiled(root, lambda: root.forward_group(lanes, [_stage(m, datas[j]) for m, j in zip(lanes, order)]))
    assert prof["deconv_depthwise"] == 1
    assert sum(v for name, v in prof.items() if "f16x3_w4d_kernel" in name) >= 1, prof    # c2 ran in the dual-tile family
    assert root.range_fallbacks == before
    for m, j in zip(lanes, order):
        _assert_c2_at_the_bar(m, onet, datas[j], "%s n%d unit %d" % (kind, n, j))


# ---- 5. max-pool beyond 2x2 stride 2 --------------------------------------------------------------------------------------------
def _pool_net(C, h, w, k, stride, pad):
    txt, cin = _front(C, k=3)
    return _net(H.single_layer_net(txt + _pool("c0", k, stride, pad), cin, h, w))


def _run_pool(net, C, h, w, k, stride, pad, params, x):
    H.load_params(net, params)
    for mode in MODES:
        net.set_conv_mode(mode)
        out, prof = _profiled(net, lambda: _forward(net, x))
        assert prof["maxpool_kernel"] == 1
        c0 = _blob(net, "c0")
        assert c0.shape == (1, C, h, w)
        want = O.max_pool(c0, k, stride, pad)
        assert out["p"].shape == want.shape, (mode, out["p"].shape, want.shape)
        np.testing.assert_array_equal(_bits(out["p"]), _bits(want), err_msg=mode)
    return c0, want


@gpu
@pytest.mark.parametrize("C,h,w,k,stride,pad", POOL_CASES)
def test_max_pool_is_pure_selection(C, h, w, k, stride, pad):
    rng = np.random.default_rng(C + 10 * h + k)
    c0, want = _run_pool(_pool_net(C, h, w, k, stride, pad), C, h, w, k, stride, pad, _random_front(rng, C, k=3),
                         rng.normal(0, 4, (1, 3, h, w)).astype(np.float32))
    assert (c0 < 0).any() and (c0 > 0).any() and len(np.unique(c0)) > c0.size // 2      # signed, no ties to speak of
    if (h, w, k, stride, pad) == (3, 5, 2, 2, 1):
        assert want.shape[2:] == (2, 3) and (-(-(h + 2 * pad - k) // stride) + 1, -(-(w + 2 * pad - k) // stride) + 1) == (3, 4)


@gpu
def test_max_pool_of_an_all_negative_map():
    """Every value of c0 is negative and the windows reach into the padding: the neutral element is -FLT_MAX, no padding
    zero may win."""
    C, h, w, k, stride, pad = 64, 6, 8, 3, 2, 1
    rng = np.random.default_rng(8)
    params = _random_front(rng, C, k=3)
    params["c0"][1][...] = -100.0 - np.abs(params["c0"][1])
    c0, want = _run_pool(_pool_net(C, h, w, k, stride, pad), C, h, w, k, stride, pad, params,
                         rng.normal(0, 1, (1, 3, h, w)).astype(np.float32))
    assert (c0 < 0).all() and (want < 0).all() and want.min() > -1000


@gpu
def test_activation_exponent_after_a_stand_alone_pool():
    """c0 -> c1 -> MAX 3/2/1 -> c2 in split-fp16 mode with everything at 2^-12, as test_conv_small_magnitudes has it: the
    pool cannot be folded into c1 (it is not 2x2 stride 2), so the pooled blob's exponent comes from launch_amax_raise --
    without it c2 would read unlifted, subnormal low parts."""
    h, w = 13, 17
    txt = H.single_layer_net(_conv("c0", "data", 128, 3, 1, True) + _conv("c1", "c0", 128, 3, 1, True) + _pool("c1", 3, 2, 1) +
                             _conv("c2", "p", 256, 3, 1, True), 3, h, w)
    gnet, onet = H.make_pair(P.parse(txt), seed=5)
    gnet.set_conv_mode("f16x3")
    rng = np.random.default_rng(3)
    sc = np.float32(2.0 ** -12)
    for name in ("c0", "c1", "c2"):   # biases of the layer's own magnitude
        onet.params[name][1][...] = (rng.normal(0, 0.5, onet.params[name][1].shape) * sc).astype(np.float32)
    H.load_params(gnet, onet.params)
    data = (rng.normal(0, 1, (1, 3, h, w)) * sc).astype(np.float32)
    _, prof = _profiled(gnet, lambda: _forward(gnet, data))
    _oracle_forward(onet, data)
    assert prof["maxpool_kernel"] == 1
    assert 0 < np.abs(onet.blobs["p"].data).max() < 64 * sc
    assert gnet.blobs["p"].data.shape == onet.blobs["p"].data.shape == (1, 128, 7, 9)
    for name in ("c0", "c1", "p", "c2"):
        err = H.rel_err(gnet.blobs[name].data, onet.blobs[name].data)
        print("pool at 2^-12: %s rel err %.3e" % (name, err))
        assert err < ACT_TOL, (name, err)
    assert gnet.range_fallbacks == 0
